"""Generates tests/golden/cosgrad_*.npz: float64 gradients of attentionMode 'GAT_Similarity' made by the REAL reference (its own
gml.GraphFilterBatchSimilarityAttentional, imported from the reference tree through oracle/_ref_import.py; build machine only),
at feature widths the HIP training kernels take (gatsim_grad_N6_G8_K3 is at G = 8, which they refuse).  TEST INFRASTRUCTURE.

    python tools/make_golden_similarity_train.py         # rewrites both cosgrad_* fixtures (bit-reproducible)

Layout: that of gatsim_grad_* (tools/make_golden_similarity.py, grad_fixture): x (2,G,N), S (2,1,N,N), wgt, y, dx, g_<parameter>,
none_grads, p_<state_dict key>, all float64 but the parameters; one x row is exactly zero, one is scaled by 1e-12.  Every x is a
float32 value, so that the device path differentiates the same function.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_similarity as mgs  # noqa: E402
from oracle._ref_import import import_reference  # noqa: E402
from oracle.make_golden import OUT  # noqa: E402

SHAPES = [(7, 16, 3, 6565), (12, 32, 2, 6666)]       # (N, G, K, seed)


def main():
    gml, _ = import_reference()
    for N, G, K, seed in SHAPES:
        fx = mgs.grad_fixture(gml, N, G, K, seed)
        # (tricky_x draws float32 values and grad_fixture widens them: the device path differentiates the same function)
        assert np.array_equal(fx["x"], fx["x"].astype(np.float32).astype(np.float64))
        path = os.path.join(OUT, "cosgrad_N%d_G%d_K%d.npz" % (N, G, K))
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < 1 << 20, (path, size)
        print("wrote", path, size // 1024, "KB")


if __name__ == "__main__":
    main()
