"""Planning cases made on the device: the first step of the expert pipeline, the reference's offlineExpert/CasesGenerator.py
- an obstacle map, its largest free component, and a start and a goal per agent - for C cases in one launch
(csrc/sim_cases.hip).  With it a training or evaluation loop is device-resident from the case to the sample:

    cases = generate_cases(C, H, W, N, density=0.1, complexity=0.01, seed=epoch)
    res = solve_cases(cases["map"], cases["start"], cases["goal"])
    s = expert_samples(cases["map"].index_select(0, pack_cases(res)), comm_radius=config.commR, **solved_pack(res))

The generator is the package's own, as the solver is: it follows the reference's recipe, but its random numbers are a
counter-based hash of (seed, global case index, stream, index) - not numpy's Mersenne Twister and Python's random.sample -
so a case depends on its GLOBAL index first_case + c alone, not on C or on its place in the batch, and it keeps the LARGEST
free component where the reference keeps the component of cell (0, 0).  Duplicate cases of a pool are not removed.

HIP only: a CPU obstacle_map or a non-GPU device raises MagatNativeError.  generate_cases is stream ordered and never waits
for the device; valid_cases reads `valid` back once."""
import torch

from . import _native as nat
from . import _sim_host as sh

KINDS = {"maze": 0, "uniform": 1, "given": 2}      # include/magat_hip.h MAGAT_CASES_*
CASE_KEYS = ("map", "start", "goal", "free_cells", "valid")
MAX_SIDE = 64      # above it: the wide form (csrc/sim_cases_wide.hip), maps up to 256 x 256


def maze_steps(H, W, density, complexity):
    """(aisles, walk) of the reference's mapGen (CasesGenerator.py:111-113), rounded here and nowhere else."""
    return int(density * (H // 2) * (W // 2)), int(complexity * 5 * (H + W))


def uniform_threshold(density):
    """floor(density * 2^32), clamped to 0 .. 2^32: a cell is an obstacle iff its 32-bit draw is below it."""
    return min(max(int(density * 4294967296.0), 0), 1 << 32)


def generate_cases(C, H, W, N, density=0.1, complexity=0.01, kind="maze", obstacle_map=None, seed=0, first_case=0,
                   device="cuda", wide=False):
    """One call of magat_sim_cases_generate: C cases of N agents on H x W maps (H, W <= 64; N <= H * W).  Returns a dict of
    device tensors: map (C,H,W) uint8 (1: obstacle), start / goal (C,N,2) int32 (row, col), free_cells (C,) int32 and valid
    (C,) uint8.

    kind "maze" is the reference's mapGen (H, W >= 4): int(density * (H//2) * (W//2)) aisles start on the even lattice and
    walk int(complexity * 5 * (H + W)) steps of length 2, each to neighbours[randint(0, len - 1)] of the neighbours listed
    left, right, up, down.  The bound is EXCLUSIVE, as numpy's is in the reference: the last listed neighbour is never
    taken - the reference's rule, kept.  kind "uniform": every cell is an obstacle with probability `density`.
    obstacle_map (H,W) or (C,H,W), non-zero: obstacle, implies kind "given" (the reference's CasesSolver_cropfromMap family).

    Of the raw map the LARGEST 4-connected free component is kept (ties: the one holding the lowest row-major cell); all
    other free cells are obstacles in `map`, and free_cells is its size F.  Starts are N distinct cells of it, uniform over
    ordered tuples; goals likewise, redrawn as a whole, at most 64 times, until goal[a] != start[a] for every agent (a start
    may be another agent's goal) - the reference's acceptance rule.  valid = 1 iff F >= N + 1 and a goal tuple was accepted;
    an invalid case has start = goal = -1 and must not be fed to the solver: valid_cases(cases) drops it.

    seed (0 .. 2^64 - 1) and the global case index first_case + c fix a case: generate_cases(40, ...) equals
    generate_cases(20, ...) followed by generate_cases(20, ..., first_case=20).

    wide=True lifts the limits to H, W <= 256 (and N <= 4096): a shape with H, W <= 64 still goes to
    magat_sim_cases_generate, a larger one to magat_sim_cases_generate_wide - the same cases from the same draws, one
    workgroup per case.  wide=False refuses H or W above 64 as before.  Stream ordered, no host synchronisation."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise nat.MagatNativeError("generate_cases: device must be a GPU (no CPU fallback), got %r" % (device,))
    if obstacle_map is not None:
        sh.dev_tensor(obstacle_map, "obstacle_map")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    m = None
    if obstacle_map is not None:
        if kind not in ("maze", "given"):
            raise ValueError("obstacle_map implies kind='given', got kind=%r" % (kind,))
        kind = "given"
        m, _, mH, mW = sh.dev_map(obstacle_map.to(dev), C)
        assert (mH, mW) == (H, W), "obstacle_map must be (H,W) or (C,H,W)"
    if kind not in KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
    if kind == "given" and m is None:
        raise ValueError("kind='given' needs an obstacle_map")
    C, H, W, N = int(C), int(H), int(W), int(N)
    aisles, walk = maze_steps(H, W, density, complexity) if kind == "maze" else (0, 0)
    threshold = uniform_threshold(density) if kind == "uniform" else 0
    out = dict(map=torch.empty(max(C, 0), max(H, 0), max(W, 0), dtype=torch.uint8, device=dev),
               start=torch.empty(max(C, 0), max(N, 0), 2, dtype=torch.int32, device=dev),
               goal=torch.empty(max(C, 0), max(N, 0), 2, dtype=torch.int32, device=dev),
               free_cells=torch.empty(max(C, 0), dtype=torch.int32, device=dev),
               valid=torch.empty(max(C, 0), dtype=torch.uint8, device=dev))
    entry = "magat_sim_cases_generate_wide" if wide and (H > MAX_SIDE or W > MAX_SIDE) else "magat_sim_cases_generate"
    sh.call(dev, entry, KINDS[kind], nat.ptr(m), 1 if m is not None and m.dim() == 3 else 0, H, W, aisles, walk, threshold,
            int(seed) & ((1 << 64) - 1), int(first_case), nat.ptr(out["map"]), nat.ptr(out["start"]), nat.ptr(out["goal"]),
            nat.ptr(out["free_cells"]), nat.ptr(out["valid"]), C, N)
    return out


def valid_cases(cases):
    """The valid cases of a generate_cases result: every tensor index_select-ed to them, plus index (K,) int64 - their places
    in the batch (global case index = first_case + index).  (Synchronises.)"""
    idx = torch.nonzero(cases["valid"] != 0).flatten()
    out = {key: cases[key].index_select(0, idx) for key in CASE_KEYS}
    out["index"] = idx
    return out
