"""Plain restatement of the package's schedule improver (magat_pathplanning_amd/mapf.py improve_schedules,
csrc/sim_mapf_lns.hip): large-neighbourhood re-planning on top of prioritized planning, written from DESIGN 4.11 on
mapf_restatement's _search / _backtrace with boolean arrays - TEST HELPER, deliberately not bitboards.

    out = improve(obstacle_map (H,W), paths (N,T,2), lengths (N,), makespan, solved, iterations, k)      # one case
    out = improve_batch(maps, res, iterations, k)                                                        # a plan_batch / solve_batch dict

Integer only, no random numbers.  Per case, on a solved schedule with horizon T = paths.shape[1]:
  * status 1 (skipped) when solved == 0; else status 2 (refused) when a length lies outside 1..T, one of the T cells of a path
    lies off the map or on an obstacle, or one of its T - 1 steps is none of the five moves.  Both come back as they came,
    with flowtime_before = flowtime_after = accepted = 0.  Conflicts BETWEEN agents are not looked for.
  * an agent's cell at t is paths[a, min(t, lengths[a] - 1)]; its start is the cell at 0, its goal the cell at lengths[a] - 1;
  * set-up: reserve all N paths (V[t] along the path and at the goal behind it, A_d[t] at the entered cell of every real
    move); d0[a] = the length of a's FREE path - search and backtrace on empty boards;
  * iteration i: delay = lengths - d0; the seed is the (i mod N)-th agent by (-delay, index); nb = [seed]; along the seed's
    free path, t = 0 .. d0 - 1, the agents b in index order that stand on the free-path cell at t, or swap with it (t >= 1:
    b at t on the cell of t - 1 and b at t - 1 on the cell of t), join nb while it holds fewer than k; then seed + 1, seed + 2,
    ... (mod N) fill it up to min(k, N); the paths of nb are un-reserved, its agents re-planned in list order, each against
    everything reserved at that moment; the new paths are kept iff every agent arrived and the sum of the new lengths is
    STRICTLY below the old sum - else what was reserved is cleared and the old paths are reserved again.
Returns paths (N,T,2) int32 padded with the last cell (an agent that was never re-planned keeps its row as it came), lengths,
makespan = max(lengths) - 1, flowtime_before / flowtime_after = sum(lengths - 1), accepted, status and history: the flowtime
before the first iteration and after each one."""
import functools

import numpy as np

from mapf_restatement import MOVES, _backtrace, _case_map, _search, random_batch, solve_batch

STATUS_OK, STATUS_SKIPPED, STATUS_REFUSED = 0, 1, 2


def screen(obstacle_map, paths, lengths):
    """True when the input must be refused."""
    m = np.asarray(obstacle_map)
    H, W = m.shape
    N, T, _ = paths.shape
    for a in range(N):
        if not 1 <= int(lengths[a]) <= T:
            return True
        for t in range(T):
            r, c = int(paths[a, t, 0]), int(paths[a, t, 1])
            if not (0 <= r < H and 0 <= c < W) or m[r, c] != 0:
                return True
            if t and (r - int(paths[a, t - 1, 0]), c - int(paths[a, t - 1, 1])) not in MOVES:
                return True
    return False


class _Boards:
    def __init__(self, H, W, T):
        self.T = T
        self.V = [np.zeros((H, W), dtype=bool) for _ in range(T)]
        self.A = [[np.zeros((H, W), dtype=bool) for _ in range(T)] for _ in range(4)]

    def mark(self, cells, value):
        """Reserve (True) or un-reserve (False) one path, given as the list of its cells."""
        L = len(cells)
        for t in range(self.T):
            cell = cells[min(t, L - 1)]
            self.V[t][cell] = value
            if 1 <= t <= L - 1:
                d = MOVES.index((cell[0] - cells[t - 1][0], cell[1] - cells[t - 1][1]))
                if d < 4:
                    self.A[d][t][cell] = value

    def plan(self, free, start, goal):
        """The solver's search and backtrace against these boards: the cells of the path, or None."""
        R, tstar = _search(free, self.V, self.A, start, goal, self.T)
        return None if tstar < 0 else _backtrace(R, self.A, goal, tstar)


def neighbourhood(seed, free_cells, cells, k):
    """cells[b]: agent b's path as a list of cells."""
    N = len(cells)

    def at(b, t):
        return cells[b][min(t, len(cells[b]) - 1)]

    nb = [seed]
    for t in range(len(free_cells)):
        for b in range(N):
            if b in nb or len(nb) >= k:
                continue
            on_it = at(b, t) == free_cells[t]
            swaps = t >= 1 and at(b, t) == free_cells[t - 1] and at(b, t - 1) == free_cells[t]
            if on_it or swaps:
                nb.append(b)
    step = 1
    while len(nb) < min(k, N):
        b = (seed + step) % N
        if b not in nb:
            nb.append(b)
        step += 1
    return nb


def improve(obstacle_map, paths, lengths, makespan, solved, iterations, k):
    m = np.asarray(obstacle_map)
    free = m == 0
    H, W = free.shape
    paths = np.array(paths, dtype=np.int32)
    lengths = np.array(lengths, dtype=np.int32)
    N, T, _ = paths.shape
    out = dict(paths=paths, lengths=lengths, makespan=int(makespan), flowtime_before=0, flowtime_after=0, accepted=0,
               status=STATUS_OK, history=[])
    if not solved:
        out["status"] = STATUS_SKIPPED
        return out
    if screen(m, paths, lengths):
        out["status"] = STATUS_REFUSED
        return out
    cells = [[(int(r), int(c)) for r, c in paths[a, :lengths[a]]] for a in range(N)]
    boards, empty = _Boards(H, W, T), _Boards(H, W, T)
    for a in range(N):
        boards.mark(cells[a], True)
    d0 = [len(empty.plan(free, cells[a][0], cells[a][-1])) for a in range(N)]
    flow = sum(len(p) - 1 for p in cells)
    out["flowtime_before"] = flow
    history = [flow]
    for i in range(int(iterations)):
        rank = sorted(range(N), key=lambda a: (-(len(cells[a]) - d0[a]), a))
        seed = rank[i % N]
        free_cells = empty.plan(free, cells[seed][0], cells[seed][-1])
        nb = neighbourhood(seed, free_cells, cells, int(k))
        for a in nb:
            boards.mark(cells[a], False)
        new = []
        for a in nb:
            p = boards.plan(free, cells[a][0], cells[a][-1])
            if p is None:
                break
            boards.mark(p, True)
            new.append(p)
        if len(new) == len(nb) and sum(len(p) for p in new) < sum(len(cells[a]) for a in nb):
            for a, p in zip(nb, new):
                cells[a] = p
                lengths[a] = len(p)
                paths[a] = np.asarray(p + [p[-1]] * (T - len(p)), dtype=np.int32)
            out["accepted"] += 1
        else:
            for p in new:
                boards.mark(p, False)
            for a in nb:
                boards.mark(cells[a], True)
        history.append(sum(len(p) - 1 for p in cells))
    out.update(makespan=int(lengths.max()) - 1, flowtime_after=history[-1], history=history)
    return out


def improve_batch(maps, res, iterations, k):
    """res: a plan_batch / solve_batch dict (paths (C,N,T,2), lengths, makespan, solved).  The results stacked, history as a
    list of lists."""
    outs = [improve(_case_map(maps, c), res["paths"][c], res["lengths"][c], res["makespan"][c], res["solved"][c], iterations, k)
            for c in range(len(res["paths"]))]
    stacked = {key: np.stack([np.asarray(o[key]) for o in outs]).astype(np.int32) for key in outs[0] if key != "history"}
    stacked["history"] = [o["history"] for o in outs]
    return stacked


def hand_case():
    """Agent 0 goes from (0, 0) to (1, 1) on an open 2 x 3 map and, planned first, takes (0, 1) - the backtrace prefers the
    move `down` into its goal; agent 1 runs the top row from (0, 2) to (0, 0), needs (0, 1) at t = 1 and has to wait one step.
    One iteration with k = 2: agent 1 is the seed (delay 1), agent 0 stands on its free path at t = 1; re-planned in the order
    1, 0, agent 1 walks straight and agent 0 goes round through (1, 0): the flowtime drops from 5 to 4."""
    m = np.zeros((2, 3), dtype=np.uint8)
    start = np.array([(0, 0), (0, 2)], dtype=np.int32)
    goal = np.array([(1, 1), (0, 0)], dtype=np.int32)
    T = 8
    before = [[(0, 0), (0, 1), (1, 1)], [(0, 2), (0, 2), (0, 1), (0, 0)]]
    after = [[(0, 0), (1, 0), (1, 1)], [(0, 2), (0, 1), (0, 0)]]
    return dict(map=m, start=start, goal=goal, T=T, before=before, after=after)


NEWCOMER_FREE_PATH = [(1, 0), (1, 1), (1, 2), (1, 3), (1, 4)]


def newcomer_case(H, N, s, p, q, T=12):
    """Two agents join the neighbourhood in ONE step of the seed's free path.  H x 20, walled but for row 1 columns 0 .. 4 (a
    corridor), the pockets (0, 1), (0, 2) and (2, 2), and the rows 4 .. H - 1, where the other N - 3 agents stand on their goals
    (length 1, delay 0).  Agent s waits at (1, 0) until t = 2 and then walks the corridor to (1, 4): delay 2, the seed of iteration
    0, its free path NEWCOMER_FREE_PATH.  Agent q comes the other way, (1, 3) (1, 2) (1, 1) (0, 1): between t = 1 and 2 it SWAPS
    with the free path.  Agent p waits in (2, 2) and steps up, (2, 2) (2, 2) (1, 2) (0, 2): at t = 2 it STANDS ON the free path's
    cell.  Nobody else is in the way at any t.  What comes of it depends on who is re-planned first: behind s and q, p finds a way
    and the flowtime drops; behind s and p, q is shut in, and with p alone next to s nothing is gained."""
    m = np.ones((H, 20), dtype=np.uint8)
    m[1, 0:5] = 0
    m[0, 1] = m[0, 2] = m[2, 2] = 0
    m[4:, :] = 0
    walks = {s: [(1, 0)] * 3 + NEWCOMER_FREE_PATH[1:], q: [(1, 3), (1, 2), (1, 1), (0, 1)], p: [(2, 2), (2, 2), (1, 2), (0, 2)]}
    assert len(walks) == 3 and N - 3 <= (H - 4) * 20
    field = iter((r, c) for r in range(4, H) for c in range(20))
    cells = [walks[a] if a in walks else [next(field)] for a in range(N)]
    lengths = np.array([len(w) for w in cells], dtype=np.int32)
    return dict(map=m, T=T, cells=cells, start=np.array([w[0] for w in cells], dtype=np.int32)[None],
                goal=np.array([w[-1] for w in cells], dtype=np.int32)[None],
                res=dict(paths=padded(cells, T)[None], lengths=lengths[None], makespan=np.array([lengths.max() - 1], dtype=np.int32),
                         solved=np.ones(1, dtype=np.uint8)))


# arrangement -> (N, the seed, the smaller and the larger index of the two newcomers): in one wavefront; in two wavefronts of one
# chunk of a workgroup of 128 threads (a map of 65 rows or more); in two chunks of 64 threads; in two chunks of 128 threads
NEWCOMERS = {"one_wave": (6, 2, 1, 4), "two_waves": (72, 2, 10, 70), "two_chunks64": (70, 2, 3, 66), "two_chunks128": (140, 2, 5, 130)}


def newcomer_named(name, H):
    """"newcomers_<arrangement>_<qp | pq>_k<k>" -> (newcomer_case(...), s, p, q, k); qp: q has the smaller index."""
    arrangement, order, k = name[len("newcomers_"):].rsplit("_", 2)
    N, s, lo, hi = NEWCOMERS[arrangement]
    p, q = (hi, lo) if order == "qp" else (lo, hi)
    return newcomer_case(H, N, s, p, q), s, p, q, int(k[1:])


def newcomer_names(arrangements):
    return ["newcomers_%s_%s_k%d" % (a, order, k) for a in arrangements for order in ("qp", "pq") for k in (2, 3)]


def joiners(free_cells, cells, t):
    """The agents that stand on the free path's cell at t or swap with it between t - 1 and t, in index order."""
    at = lambda b, u: cells[b][min(u, len(cells[b]) - 1)]      # noqa: E731
    return [b for b in range(len(cells)) if at(b, t) == free_cells[t]
            or (t >= 1 and at(b, t) == free_cells[t - 1] and at(b, t - 1) == free_cells[t])]


def padded(cells, T):
    """Paths given as lists of cells -> (N,T,2) int32 padded with the last cell."""
    return np.asarray([p + [p[-1]] * (T - len(p)) for p in cells], dtype=np.int32)


# The two random batches of the property test (CPU) and of the equality test (GPU): solved and improved once per session.
BATCHES = {"10x10": dict(args=(11, 8, 10, 10, 8, 0.2), T=48, iterations=16, k=3),
           "12x12": dict(args=(12, 6, 12, 12, 16, 0.15), T=64, iterations=16, k=4)}


@functools.lru_cache(maxsize=None)
def solved_and_improved(name):
    """name -> (map, start, goal, solve_batch's result, improve_batch's result); treat them as read-only."""
    b = BATCHES[name]
    m, start, goal = random_batch(*b["args"])
    res = solve_batch(m, start, goal, b["T"], retries=8)
    return m, start, goal, res, improve_batch(m, res, b["iterations"], b["k"])
