"""The rule of ExpertMemory / magat_sim_expert_pick in numpy, written from include/magat_hip.h: the store (packed cells,
prefix sums), sample -> (case, step), the per-agent decode, and the clamp of an index outside the range.  Plain loops; no
torch, no kernel text."""
import numpy as np

NO_ROW = 0x7fffffff
MOVES = [(-1, 0), (0, -1), (1, 0), (0, 1), (0, 0)]      # up, left, down, right, stop


def make_store(paths, lengths, goal, makespan, max_length, radii=None, maps=None):
    """paths (C,N,Lmax,2), lengths (C,N), goal (C,N,2), makespan (C,) -> the store as a dict of arrays: cells (C,N,max_length)
    uint16 = row << 8 | col, padded behind lengths with the path's last cell (whatever stands behind lengths in `paths`), ...,
    cum (C,) int64 the inclusive prefix sums of makespan + 1."""
    paths, lengths, goal = np.asarray(paths), np.asarray(lengths), np.asarray(goal)
    makespan = np.asarray(makespan).reshape(-1)
    C, N = lengths.shape
    assert lengths.min() >= 1 and lengths.max() <= max_length and lengths.max() <= paths.shape[2]
    assert paths.min() >= 0 and paths.max() <= 255
    cells = np.zeros((C, N, max_length), dtype=np.uint16)
    for c in range(C):
        for n in range(N):
            L = int(lengths[c, n])
            for l in range(max_length):
                r, q = paths[c, n, min(l, L - 1)]
                cells[c, n, l] = (int(r) << 8) | int(q)
    return dict(cells=cells, lengths=lengths.astype(np.int32), goal=goal.astype(np.int32), makespan=makespan.astype(np.int32),
                radii=np.ones(C) if radii is None else np.asarray(radii, dtype=np.float64),
                cum=np.cumsum(makespan.astype(np.int64) + 1), maps=maps)


def concat_stores(stores):
    """Several appends: the stores one behind the other (the same max_length); cum runs on."""
    out = {key: np.concatenate([s[key] for s in stores]) for key in ("cells", "lengths", "goal", "makespan", "radii")}
    out["cum"] = np.cumsum(out["makespan"].astype(np.int64) + 1)
    out["maps"] = None if stores[0]["maps"] is None else np.concatenate([s["maps"] for s in stores])
    return out


def locate(cum, j):
    """Sample j -> (case, step, clamped): the first case whose inclusive prefix sum is above j, by binary search; j outside
    [0, cum[-1]) is clamped into it first."""
    total = int(cum[-1])
    clamped = j < 0 or j >= total
    if clamped:
        j = 0 if j < 0 else total - 1
    lo, hi, steps = 0, len(cum) - 1, 0
    while lo < hi:
        mid = (lo + hi) // 2
        if cum[mid] > j:
            hi = mid
        else:
            lo = mid + 1
        steps += 1
    assert steps <= 20 or len(cum) > 1 << 20
    return lo, int(j - (cum[lo - 1] if lo else 0)), clamped


def decode(store, c, t):
    """(pos (N,2), target (N,5), action (N,)) of step t of case c: expert_schedule's rule on the packed cells."""
    N = store["lengths"].shape[1]
    pos = np.zeros((N, 2), dtype=np.int32)
    target = np.zeros((N, 5), dtype=np.float32)
    action = np.zeros(N, dtype=np.int64)
    for n in range(N):
        L = int(store["lengths"][c, n])
        g = tuple(int(v) for v in store["goal"][c, n])
        cell = lambda l: (int(store["cells"][c, n, l]) >> 8, int(store["cells"][c, n, l]) & 255)      # noqa: E731
        cur = cell(t) if t < L else g
        nxt = cell(t + 1) if t < L - 1 else g
        d = (nxt[0] - cur[0], nxt[1] - cur[1])
        pos[n] = cur
        if d in MOVES:
            target[n, MOVES.index(d)] = 1.0
            action[n] = MOVES.index(d)
    return pos, target, action


def pick(store, indices):
    """The whole entry: dict(case, step (M,), pos (M,N,2), target (M,N,5), action (M,N), goal (M,N,2), radii (M,), map (M,H,W) or
    None, flag = the smallest row whose index was clamped, NO_ROW without one)."""
    M, N = len(indices), store["lengths"].shape[1]
    out = dict(case=np.zeros(M, dtype=np.int32), step=np.zeros(M, dtype=np.int32), pos=np.zeros((M, N, 2), dtype=np.int32),
               target=np.zeros((M, N, 5), dtype=np.float32), action=np.zeros((M, N), dtype=np.int64),
               goal=np.zeros((M, N, 2), dtype=np.int32), radii=np.zeros(M), flag=NO_ROW,
               map=None if store["maps"] is None else np.zeros((M,) + store["maps"].shape[1:], dtype=np.uint8))
    for m, j in enumerate(indices):
        c, t, clamped = locate(store["cum"], int(j))
        if clamped:
            out["flag"] = min(out["flag"], m)
        out["case"][m], out["step"][m] = c, t
        out["pos"][m], out["target"][m], out["action"][m] = decode(store, c, t)
        out["goal"][m], out["radii"][m] = store["goal"][c], store["radii"][c]
        if out["map"] is not None:
            out["map"][m] = store["maps"][c]
    return out


def one_step_store(max_length=10):
    """Makespans [0, 3, 0, 0, 7, 1], two agents, on a 12 x 12 open map: cases of one step next to each other.  In the makespan-0
    cases both agents stand on their goals; agent 1 of the longer cases arrives early (L < T_c) and agent 0 takes every step."""
    makespans = [0, 3, 0, 0, 7, 1]
    paths, goals = [], []
    for c, mk in enumerate(makespans):
        a0 = [(c, l) for l in range(mk + 1)]                                   # walks right along row c
        a1 = [(11 - l, c) for l in range(mk // 2 + 1)]                         # walks up along column c, half as far
        paths.append([a0, a1])
        goals.append([a0[-1], a1[-1]])
    Lmax = max(len(p) for case in paths for p in case)
    arr = np.zeros((len(paths), 2, Lmax, 2), dtype=np.int32)
    lengths = np.zeros((len(paths), 2), dtype=np.int32)
    for c, case in enumerate(paths):
        for n, p in enumerate(case):
            arr[c, n, :len(p)] = p
            arr[c, n, len(p):] = p[-1]
            lengths[c, n] = len(p)
    maps = np.zeros((len(paths), 12, 12), dtype=np.uint8)
    return dict(paths=arr, lengths=lengths, goal=np.asarray(goals, dtype=np.int32), makespan=np.asarray(makespans, dtype=np.int32),
                maps=maps, start=arr[:, :, 0].copy()), make_store(arr, lengths, goals, makespans, max_length,
                                                                  radii=1.5 + np.arange(len(paths)), maps=maps)
