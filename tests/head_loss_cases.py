"""Shapes, inputs and the float64 reference of the fused action head + loss (csrc/head_loss.hip, magat_pathplanning_amd/loss.py),
shared by tests/test_host_head_loss.py and tests/test_gpu_head_loss.py.  The reference is written out here in torch float64 ops
on the CPU (tnf.cross_entropy; the KL sum of the reference's label smoothing term by term) - it never calls the package."""
import functools

import torch
import torch.nn.functional as tnf

CLASSES = 5
SMOOTHING = 0.1

# (M, width, ldx or None)
SHAPES = [
    (1, 4, None),            # one row, the smallest width
    (63, 36, None),          # the wave boundary; skip-concat widths of the published shapes
    (64, 128, None),
    (65, 132, None),
    (65, 128, 256),          # rows of a wider matrix
    (257, 640, None),        # ragged blocks; the widest head the configs produce (4 heads x 128 + the 128-wide feature map)
    (6400, 128, None),       # the 64 x 100 step: many block partials
    (8, 1024, None),         # the width limit
]
MODES = [(0, 0.0), (1, SMOOTHING)]          # (mode, smoothing): cross-entropy (mean) | the reference's LabelSmoothing (KL sum)

# gates: the project's own for float32 FMA kernels against float64 (tests/test_gpu_train.py)
GATE_ROWS = 2e-6             # logits (relative to max(1, max|logits|)) and dX (relative to max|dX|)
GATE_PARAMS = 5e-6           # dW, db (relative to the reference tensor's max-abs)
GATE_LOSS = 2e-6             # relative to max(1, |loss|)


def shape_id(shape):
    M, width, ldx = shape
    return "M%d-w%d" % (M, width) + ("" if ldx is None else "-ld%d" % ldx)


def smoothed_targets(target, smoothing):
    q = torch.full((target.shape[0], CLASSES), smoothing / (CLASSES - 1), dtype=torch.float64)
    return q.scatter_(1, target.unsqueeze(1), 1.0 - smoothing)


def reference_loss(logits, target, mode, smoothing):
    """float64 loss of (M, 5) float64 logits"""
    if mode == 0:
        return tnf.cross_entropy(logits, target)
    logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    q = smoothed_targets(target, smoothing)
    terms = torch.where(q > 0, q * (torch.log(q.clamp_min(1e-300)) - logp), torch.zeros_like(q))
    return terms.sum()


def reference(X, W, b, target, mode, smoothing, grad_scale=1.0):
    """float64 autograd on the CPU over the same float32 values -> dict of float64 tensors"""
    X = X.detach().cpu().double().requires_grad_(True)
    W = W.detach().cpu().double().requires_grad_(True)
    b = None if b is None else b.detach().cpu().double().requires_grad_(True)
    logits = X @ W.t() if b is None else X @ W.t() + b
    logits.retain_grad()
    loss = reference_loss(logits, target.cpu(), mode, smoothing)
    (loss * grad_scale).backward()
    return {"logits": logits.detach(), "loss": loss.detach(), "dlogits": logits.grad, "dX": X.grad, "dW": W.grad,
            "db": None if b is None else b.grad}


def make_inputs(M, width, seed):
    """float32 CPU tensors: X (M, width), W (5, width) scaled for logits of a few units, b (5,), target (M,) int64"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, width, generator=g)
    W = torch.randn(CLASSES, width, generator=g) * (2.0 / width ** 0.5)
    b = torch.randn(CLASSES, generator=g) * 0.3
    target = torch.randint(0, CLASSES, (M,), generator=g)
    return X, W, b, target


@functools.lru_cache(maxsize=None)
def case(shape, mode_key):
    """(inputs, reference) of one (shape, (mode, smoothing)); computed once per session and never written to"""
    M, width, _ = shape
    mode, smoothing = mode_key
    inp = make_inputs(M, width, 1000 + 7 * M + width + mode)
    return inp, reference(*inp, mode, smoothing)


def extreme_inputs():
    """65 rows whose logits span +-1e4 and are exact in float32: X rows are +-one-hot-like small integers, W holds integers, so
    every product and sum is an integer below 2^24"""
    M, width = 65, 36
    g = torch.Generator().manual_seed(77)
    X = torch.randint(-3, 4, (M, width), generator=g).float()
    W = torch.randint(-150, 151, (CLASSES, width), generator=g).float()
    b = torch.tensor([0.0, 1.0, -2.0, 3.0, -1.0])
    X[0], X[1] = 0.0, 0.0
    X[0, 0], X[1, 0] = 3.0, -3.0
    W[:, 0] = torch.tensor([3333.0, -3333.0, 1000.0, 0.0, -2500.0])      # rows 0 / 1: logits +-9999 (+ bias)
    target = torch.randint(0, CLASSES, (M,), generator=g)
    return X, W, b, target
