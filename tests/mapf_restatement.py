"""Plain restatement of the package's multi-agent path-finding expert (magat_pathplanning_amd/mapf.py, csrc/sim_mapf.hip):
prioritized planning with an exact space-time search per agent, written from DESIGN 4.11 with per-cell loops over boolean
arrays - TEST HELPER, deliberately not bitboards, so that it shares no trick with the kernel it is the yardstick of.

    out = plan(obstacle_map (H,W), start (N,2), goal (N,2), order=None, T=...)      # one case, one priority order
    out = solve_with_retries(obstacle_map, start, goal, T, retries=8)               # + order, rounds
    err = check_schedule(obstacle_map, start, goal, out["paths"], out["lengths"])   # None, or what is wrong (independent of plan)
    m, start, goal = random_case(rng, H, W, N, density)                            # starts / goals in the largest free component
    plan_batch / solve_batch                                                        # the same over C cases, stacked

Cells are (row, col); moves in the package's key order up, left, down, right, stop.  Per case, in `order`:
  * an `order` that is no permutation of 0..N-1: unsolved, failed_agent -2, every agent gets its start cell with length 1;
  * agent a fails BEFORE any search when its start or goal is off the map or on an obstacle, or equals the start / goal of
    an agent earlier in the order;
  * otherwise R_0 = {start}, R_{t+1} = free & ~V[t+1] & (R_t | U_d shift_d(R_t & ~A_opp(d)[t+1])); t* = the first t > last
    with the goal in R_t (last: the largest t with the goal in V[t], or -1); the search ends at t*, at an empty R_t, or at
    t = T - 1; no t*: the agent fails;
  * backtrace from (goal, t*): the move INTO the current cell is the first of up, left, down, right, stop whose source cell
    lies on the map, in R_{t-1} and (real moves) not in A_opp(d)[t];
  * reserve V[t] along the path and at the goal for t* < t < T, A_d[t] at the entered cell of every real move.
A failed case keeps the paths of the agents planned before the failure; the failing agent and those behind it get their
start cell with length 1.  paths (N,T,2) int32 are padded with their last cell, lengths = t* + 1, makespan = max(lengths) - 1."""
import numpy as np

MOVES = ((-1, 0), (0, -1), (1, 0), (0, 1), (0, 0))      # up, left, down, right, stop
OPP = (2, 3, 0, 1)


def _inside(cell, H, W):
    return 0 <= cell[0] < H and 0 <= cell[1] < W


def _search(free, V, A, start, goal, T):
    """The reachable layers of one agent and its arrival time (or -1)."""
    H, W = free.shape
    last = -1
    for t in range(T):
        if V[t][goal]:
            last = t
    R = [np.zeros((H, W), dtype=bool)]
    R[0][start] = True
    t = 0
    while True:
        if t > last and R[t][goal]:
            return R, t
        if t == T - 1 or not R[t].any():
            return R, -1
        nxt = np.zeros((H, W), dtype=bool)
        for r, c in np.argwhere(R[t]):                                       # cell by cell
            nxt[r, c] = True                                                 # stop
            for d in range(4):
                if A[OPP[d]][t + 1][r, c]:                                   # a planned agent enters (r, c) from (r, c) + d
                    continue
                v = (r + MOVES[d][0], c + MOVES[d][1])
                if _inside(v, H, W):
                    nxt[v] = True
        nxt &= free & ~V[t + 1]
        R.append(nxt)
        t += 1


def _backtrace(R, A, goal, tstar):
    H, W = R[0].shape
    path = [goal]
    cur = goal
    for t in range(tstar, 0, -1):
        for d in range(5):
            u = (cur[0] - MOVES[d][0], cur[1] - MOVES[d][1])
            if not _inside(u, H, W) or not R[t - 1][u]:
                continue
            if d < 4 and A[OPP[d]][t][u]:
                continue
            break
        else:
            raise AssertionError("backtrace: no predecessor at t = %d" % t)
        cur = u
        path.append(cur)
    return path[::-1]


def plan(obstacle_map, start, goal, order=None, T=None):
    m = np.asarray(obstacle_map)
    free = m == 0
    H, W = free.shape
    start, goal = np.asarray(start, dtype=np.int64).reshape(-1, 2), np.asarray(goal, dtype=np.int64).reshape(-1, 2)
    N = len(start)
    T = int(T)
    order = list(range(N)) if order is None else [int(a) for a in np.asarray(order).reshape(-1)]
    paths = np.repeat(start[:, None, :], T, axis=1).astype(np.int32)
    lengths = np.ones(N, dtype=np.int32)
    out = dict(paths=paths, lengths=lengths, makespan=0, solved=0, failed_agent=-2)
    if len(order) != N or sorted(order) != list(range(N)):
        return out
    V = [np.zeros((H, W), dtype=bool) for _ in range(T)]
    A = [[np.zeros((H, W), dtype=bool) for _ in range(T)] for _ in range(4)]
    failed = -1
    for k, a in enumerate(order):
        s, g = tuple(int(v) for v in start[a]), tuple(int(v) for v in goal[a])
        ok = _inside(s, H, W) and _inside(g, H, W) and bool(free[s]) and bool(free[g])
        for b in order[:k]:
            if tuple(start[b]) == s or tuple(goal[b]) == g:
                ok = False
        tstar = -1
        if ok:
            R, tstar = _search(free, V, A, s, g, T)
        if tstar < 0:
            failed = a
            break
        p = _backtrace(R, A, g, tstar)
        for t in range(T):
            cell = p[t] if t <= tstar else g
            V[t][cell] = True
            paths[a, t] = cell
            if 1 <= t <= tstar:
                d = MOVES.index((p[t][0] - p[t - 1][0], p[t][1] - p[t - 1][1]))
                if d < 4:
                    A[d][t][cell] = True
        lengths[a] = tstar + 1
    out.update(makespan=int(lengths.max()) - 1, solved=int(failed < 0), failed_agent=failed)
    return out


def promote(order, agent):
    """`agent` to the front, the others keep their relative order."""
    return [agent] + [a for a in order if a != agent]


def solve_with_retries(obstacle_map, start, goal, T, retries=8):
    """plan in index order; while unsolved and re-plans remain: the failed agent goes to the front of the order.  rounds =
    the number of plans made.  Returns plan's dict of the LAST plan plus order and rounds."""
    N = len(np.asarray(start).reshape(-1, 2))
    order = list(range(N))
    out = plan(obstacle_map, start, goal, order, T)
    rounds = 1
    while not out["solved"] and rounds <= retries:
        order = promote(order, out["failed_agent"])
        out = plan(obstacle_map, start, goal, order, T)
        rounds += 1
    out.update(order=np.asarray(order, dtype=np.int32), rounds=rounds)
    return out


def _stack(outs):
    res = {}
    for key in outs[0]:
        res[key] = np.stack([np.asarray(o[key]) for o in outs]).astype(np.uint8 if key == "solved" else np.int32)
    return res


def _case_map(maps, c):
    maps = np.asarray(maps)
    return maps if maps.ndim == 2 else maps[c]


def plan_batch(maps, start, goal, order=None, T=None):
    return _stack([plan(_case_map(maps, c), start[c], goal[c], None if order is None else order[c], T)
                   for c in range(len(start))])


def solve_batch(maps, start, goal, T, retries=8):
    return _stack([solve_with_retries(_case_map(maps, c), start[c], goal[c], T, retries) for c in range(len(start))])


def check_schedule(obstacle_map, start, goal, paths, lengths):
    """None when the padded schedule (N,T,2) is a valid MAPF solution, else a sentence naming the first fault.  Works on the
    cells alone: it knows nothing of reservation tables."""
    m = np.asarray(obstacle_map)
    H, W = m.shape
    paths, lengths = np.asarray(paths, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    N, T, _ = paths.shape
    for n in range(N):
        L = int(lengths[n])
        if not 1 <= L <= T:
            return "agent %d: length %d outside 1..%d" % (n, L, T)
        if tuple(paths[n, 0]) != tuple(np.asarray(start)[n]):
            return "agent %d does not begin at its start" % n
        if tuple(paths[n, L - 1]) != tuple(np.asarray(goal)[n]):
            return "agent %d does not end at its goal" % n
        for t in range(T):
            r, c = paths[n, t]
            if not (0 <= r < H and 0 <= c < W) or m[r, c] != 0:
                return "agent %d at t = %d stands on (%d, %d), which is not a free cell" % (n, t, r, c)
            if t >= L and tuple(paths[n, t]) != tuple(paths[n, L - 1]):
                return "agent %d: padding at t = %d is not its last cell" % (n, t)
            if t and (paths[n, t, 0] - paths[n, t - 1, 0], paths[n, t, 1] - paths[n, t - 1, 1]) not in MOVES:
                return "agent %d: step %d is none of the five moves" % (n, t)
    for t in range(T):
        for i in range(N):
            for j in range(i + 1, N):
                if tuple(paths[i, t]) == tuple(paths[j, t]):
                    return "agents %d and %d share (%d, %d) at t = %d" % (i, j, paths[i, t, 0], paths[i, t, 1], t)
                if t and tuple(paths[i, t]) == tuple(paths[j, t - 1]) and tuple(paths[j, t]) == tuple(paths[i, t - 1]) \
                        and tuple(paths[i, t]) != tuple(paths[i, t - 1]):
                    return "agents %d and %d swap at t = %d" % (i, j, t)
    return None


def largest_component(free):
    """Cells (K,2) of the largest 4-connected component of `free`, in row-major order."""
    H, W = free.shape
    label = np.full((H, W), -1, dtype=np.int64)
    best, best_size, n = -1, 0, 0
    for r0 in range(H):
        for c0 in range(W):
            if not free[r0, c0] or label[r0, c0] >= 0:
                continue
            stack, size = [(r0, c0)], 0
            label[r0, c0] = n
            while stack:
                r, c = stack.pop()
                size += 1
                for dr, dc in MOVES[:4]:
                    v = (r + dr, c + dc)
                    if 0 <= v[0] < H and 0 <= v[1] < W and free[v] and label[v] < 0:
                        label[v] = n
                        stack.append(v)
            if size > best_size:
                best, best_size = n, size
            n += 1
    return np.argwhere(label == best) if best >= 0 else np.zeros((0, 2), dtype=np.int64)


def random_case(rng, H, W, N, density):
    """A random obstacle map of the given density (redrawn until its largest free component holds 2 N cells) and N distinct
    starts and N distinct goals from that component.  uint8 map (1: obstacle), int32 (N,2) starts and goals."""
    while True:
        m = (rng.random((H, W)) < density).astype(np.uint8)
        cells = largest_component(m == 0)
        if len(cells) >= 2 * N:
            break
    start = cells[rng.permutation(len(cells))[:N]].astype(np.int32)
    goal = cells[rng.permutation(len(cells))[:N]].astype(np.int32)
    return m, start, goal


def random_batch(seed, C, H, W, N, density, batched_map=False):
    """C seeded cases on one map (H,W), or each on a map of its own (C,H,W)."""
    rng = np.random.default_rng(seed)
    if batched_map:
        cases = [random_case(rng, H, W, N, density) for _ in range(C)]
        return np.stack([k[0] for k in cases]), np.stack([k[1] for k in cases]), np.stack([k[2] for k in cases])
    m, _, _ = random_case(rng, H, W, N, density)
    cells = largest_component(m == 0)
    start = np.stack([cells[rng.permutation(len(cells))[:N]] for _ in range(C)]).astype(np.int32)
    goal = np.stack([cells[rng.permutation(len(cells))[:N]] for _ in range(C)]).astype(np.int32)
    return m, start, goal


# Hand cases (map rows as strings, '#': obstacle), shared by the CPU and the GPU tests -----------------------------------------
def grid(rows):
    return np.array([[1 if ch == "#" else 0 for ch in row] for row in rows], dtype=np.uint8)


def hand_cases():
    """name -> dict(map, start, goal, T).  All maps are 5 x 7 so that they stack into one (C,H,W) batch."""
    cases = {}
    # one-wide corridor (row 1) with a pocket at (2, 4): agent 0 runs left to right, agent 1 right to left and has to wait in
    # the pocket while agent 0 passes
    corridor = grid(["#######", ".......", "####.##", "#######", "#######"])
    cases["wait_in_pocket"] = dict(map=corridor, start=[(1, 0), (1, 6)], goal=[(1, 6), (1, 0)], T=24)
    # the same corridor without the pocket: a head-on pair cannot pass in either order
    closed = grid(["#######", ".......", "#######", "#######", "#######"])
    cases["head_on_closed"] = dict(map=closed, start=[(1, 0), (1, 6)], goal=[(1, 6), (1, 0)], T=24)
    cases["start_is_goal"] = dict(map=corridor, start=[(1, 2), (2, 4)], goal=[(1, 2), (2, 4)], T=8)
    # agent 0 walks row 1 from column 0 to column 6 and stands on (1, 5) at time 5; agent 1's goal IS (1, 5), one step from
    # its start (0, 5): it may not hold its goal before agent 0 has passed
    cross = grid(["#####.#", ".......", "#######", "#######", "#######"])
    cases["goal_crossed_at_5"] = dict(map=cross, start=[(1, 0), (0, 5)], goal=[(1, 6), (1, 5)], T=24)
    # agent 0 (first in index order) is at home at once and blocks the corridor that agent 1 has to leave through; planned
    # second it steps into the pocket (2, 1) and returns
    dead_end = grid(["#######", "...####", "#.#####", "#######", "#######"])
    cases["needs_promotion"] = dict(map=dead_end, start=[(1, 1), (1, 2)], goal=[(1, 1), (1, 0)], T=16)
    for k in cases.values():
        k["start"], k["goal"] = np.asarray(k["start"], dtype=np.int32), np.asarray(k["goal"], dtype=np.int32)
    return cases
