"""Times the two halves of magat_gso_csr_build at a given shape (default BASELINE config 5: 128 x 1000 x 1000 float32):
phase 1 = the streaming pass over S (scrub + bit matrix + totals), phase 2 = the structure kernel.  MAGAT_LIB_PATH picks a build.

    python tools/csr_build_bench.py [B N] [--graph edges]

--graph edges times magat_gso_edges_build instead (csrc/gso_edges.hip: the same arrays from the positions, up to 4096 agents) on
positions of the same density, next to what stands in front of the dense builder in a closed loop: batched_gso's tensor (up to
2048 agents) and, up to 1024, the two phases above on that tensor.  20 calls between two events, five rounds: median (smallest ..
largest)."""
import sys, torch
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magat_pathplanning_amd import _native as nat
from magat_pathplanning_amd.graphml import CsrStructure
from magat_pathplanning_amd.synthetic import comm_gso
EDGES = "--graph" in sys.argv and sys.argv[sys.argv.index("--graph") + 1] == "edges"
if "--graph" in sys.argv:
    del sys.argv[sys.argv.index("--graph"):sys.argv.index("--graph") + 2]
B, N = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (128, 1000)
dev = torch.device("cuda:0")


def edges_leg():
    import numpy as np
    from magat_pathplanning_amd.edges import EdgeStructure
    from magat_pathplanning_amd.simulator import batched_gso
    os.environ["MAGAT_CSR_SIDE"] = "0"
    side = int(6.5 * N ** 0.5)
    pos = torch.from_numpy(np.random.default_rng(1).integers(0, side, size=(B, N, 2)).astype(np.int32)).to(dev)

    def rounds(fn, calls=20, n=5):
        us = []
        for _ in range(3):
            fn()
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / calls)
        us.sort()
        return "%.1f us (%.1f .. %.1f)" % (us[n // 2], us[0], us[-1])

    st = EdgeStructure().build(pos, 0, None, 7.0)
    nnz = st.ready(dev)
    print("B %d N %d: %d edges (%.1f per agent), workspace %.1f MB" % (B, N, nnz, nnz / (B * N), st.ws.numel() / 1e6))
    print("edges from positions (magat_gso_edges_build, both kernels):", rounds(lambda: st.build(pos, 0, None, 7.0)))
    if N <= 2048:
        print("batched_gso (float64, lambda_max, the (B,N,N) tensor):     ", rounds(lambda: batched_gso(pos, 7.0)))
    if N <= 1024:
        S, dense = batched_gso(pos, 7.0), CsrStructure()
        print("magat_gso_csr_build on that tensor (scrub, both phases):   ", rounds(lambda: dense.build(S, 0, scrub_nan=1)))


if EDGES:
    edges_leg()
    sys.exit(0)
S = comm_gso(B, N, int(6.5 * N ** 0.5), seed=1).to(dev)
st = CsrStructure()
import os
os.environ["MAGAT_CSR_SIDE"] = "0"
st.build(S, 0, scrub_nan=1)
nnz = st.ready(dev)
lib = nat.lib()
def phase(ph):
    nat.check(lib.magat_gso_csr_build_phase(nat.ptr(S), 0, 1, 0, 0, nat.ptr(st.rowptr), nat.ptr(st.colidx), nat.ptr(st.cscptr),
                                            nat.ptr(st.csc[0]), nat.ptr(st.csc[1]), st.cap, nat.ptr(st.nnz_dev), nat.ptr(st.ws),
                                            st.ws.numel(), B, N, ph, nat.current_stream(dev)), "build")
for ph in (1, 2):
    for _ in range(3):
        phase(ph)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        phase(ph)
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 20
    print("phase %d: %.1f us%s" % (ph, us, "  (%.2f TB/s over S)" % (S.numel() * 4 / us / 1e6) if ph == 1 else ""), "nnz", nnz)
