"""Generates tests/golden/lossls_s01.npz and lossls_s03.npz: the reference's label-smoothed training loss on a 36 -> 5 action head,
made by the REAL reference class (graphs/losses/label_smoothing.py LabelSmoothing, imported from the reference tree through
oracle/_ref_import.py; build machine only) behind a float64 nn.Linear.  TEST INFRASTRUCTURE.

    python tools/make_golden_loss.py         # rewrites both fixtures

Layout (all float64 but `target`, int64): X (37, 36), W (5, 36), b (5,), target (37,) with every class present, logits (37, 5),
loss (), dX, dW, db from loss.backward(), smoothing ().  Every X, W and b is a float32 value, so that the device path
differentiates the same function.
"""
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle._ref_import import REF_ROOT, import_reference  # noqa: E402
from oracle.make_golden import OUT  # noqa: E402

M, WIDTH, CLASSES = 37, 36, 5
CASES = [("s01", 0.1, 7101), ("s03", 0.3, 7303)]       # (name, smoothing, seed)


def reference_label_smoothing():
    import_reference()                                  # (registers the bare `graphs` package and the import path)
    if "graphs.losses" not in sys.modules:              # graphs/losses/__init__.py is not needed for the one file
        pkg = types.ModuleType("graphs.losses")
        pkg.__path__ = [os.path.join(REF_ROOT, "graphs", "losses")]
        sys.modules["graphs.losses"] = pkg
    return importlib.import_module("graphs.losses.label_smoothing").LabelSmoothing


def fixture(LabelSmoothing, smoothing, seed):
    g = torch.Generator().manual_seed(seed)
    f32 = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).float().double()      # noqa: E731
    lin = torch.nn.Linear(WIDTH, CLASSES).double()
    with torch.no_grad():
        lin.weight.copy_(f32(CLASSES, WIDTH, scale=0.4))
        lin.bias.copy_(f32(CLASSES, scale=0.2))
    X = f32(M, WIDTH).requires_grad_(True)
    target = torch.cat((torch.arange(CLASSES), torch.randint(0, CLASSES, (M - CLASSES,), generator=g)))
    target = target[torch.randperm(M, generator=g)]
    crit = LabelSmoothing(CLASSES, smoothing)
    logits = lin(X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # (the reference's size_average= and implicit LogSoftmax dim)
        loss = crit(logits, target)
    loss.backward()
    assert set(target.tolist()) == set(range(CLASSES))
    return {"X": X.detach().numpy(), "W": lin.weight.detach().numpy(), "b": lin.bias.detach().numpy(),
            "target": target.numpy().astype(np.int64), "logits": logits.detach().numpy(), "loss": loss.detach().numpy(),
            "dX": X.grad.numpy(), "dW": lin.weight.grad.numpy(), "db": lin.bias.grad.numpy(),
            "smoothing": np.float64(smoothing)}


def main():
    LabelSmoothing = reference_label_smoothing()
    for name, smoothing, seed in CASES:
        fx = fixture(LabelSmoothing, smoothing, seed)
        path = os.path.join(OUT, "lossls_%s.npz" % name)
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < 1 << 20, (path, size)
        print("wrote", path, size // 1024, "KB", "loss", float(fx["loss"]))


if __name__ == "__main__":
    main()
