"""Plain restatement of the package's case generator (magat_pathplanning_amd/cases.py, csrc/sim_cases.hip), written from
DESIGN 4.12 over cells and Python ints - TEST HELPER, deliberately no bitboards: components by breadth-first search over
cells, the k-th free cell from a sorted list - so that it shares no trick with the kernel it is the yardstick of.

    out = generate(kind, C, H, W, N, density=, complexity=, seed=, first_case=, maps=None)
    # map (C,H,W) uint8, start / goal (C,N,2) int32, free_cells (C,) int32, valid (C,) uint8 - what the device returns -
    # plus raw (C,H,W) uint8 (the map before the fill) and trace: per case the maze walk's log (origins, steps)

Random numbers (all arithmetic mod 2^64): M = 0x9E3779B97F4A7C15,
    mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
    draw(seed, case, stream, i) = mix(mix(seed + M * (case + 1)) + M * ((stream << 40 | i) + 1))
    u32 = draw >> 32, below(n) = (u32 * n) >> 32
streams: 0 aisle x [aisle], 1 aisle y [aisle], 2 walk step [aisle * walk + j], 3 uniform cell [r * W + c], 4 start [a],
5 goal [round * N + a]; case is the GLOBAL index first_case + c.

Per case: (a) the raw map - maze: aisles = int(density * (H//2) * (W//2)) walks of walk = int(complexity * 5 * (H + W)) steps;
an aisle starts at x = 2 below(W//2), y = 2 below(H//2) and sets that cell; a step lists the distance-2 neighbours left (x > 1),
right (x < W - 2), up (y > 1), down (y < H - 2), picks neighbours[below(len - 1)] (the last listed one is never taken) and,
if that cell is free, sets it and the cell between and moves there; uniform: cell (r, c) is an obstacle iff u32 < floor(density
* 2^32); given: the caller's map, non-zero = obstacle.  (b) the kept region = the largest 4-connected free component, ties to the
one holding the lowest row-major cell; every other cell is an obstacle of `map`.  (c) starts: for a = 0 .. N-1 the below(F - a)-th
cell, in row-major order, of the region's cells not taken yet; goals: the same from the full region, in rounds - a round stands
only if goal[a] != start[a] for every a, else the next round draws the whole tuple again, 64 rounds at most.  (d) valid iff
F >= N + 1 and a round stood; otherwise start = goal = -1."""
import numpy as np

MASK = (1 << 64) - 1
M = 0x9E3779B97F4A7C15
ROUNDS = 64
AISLE_X, AISLE_Y, WALK, CELL, START, GOAL = range(6)


def mix(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def draw(seed, case, stream, i):
    return mix(mix(seed + M * (case + 1)) + M * (((stream << 40) | i) + 1))


def u32(seed, case, stream, i):
    return draw(seed, case, stream, i) >> 32


def below(seed, case, stream, i, n):
    return (u32(seed, case, stream, i) * n) >> 32


def maze_steps(H, W, density, complexity):
    return int(density * (H // 2) * (W // 2)), int(complexity * 5 * (H + W))


def raw_maze(seed, case, H, W, aisles, walk):
    """(map, trace): trace = dict(origins=[(y, x)], steps=[(len(neighbours), picked index, taken?)])."""
    maze = np.zeros((H, W), dtype=np.uint8)
    trace = dict(origins=[], steps=[])
    for i in range(aisles):
        x, y = 2 * below(seed, case, AISLE_X, i, W // 2), 2 * below(seed, case, AISLE_Y, i, H // 2)
        maze[y, x] = 1
        trace["origins"].append((y, x))
        for j in range(walk):
            neighbours = []
            if x > 1:
                neighbours.append((y, x - 2))
            if x < W - 2:
                neighbours.append((y, x + 2))
            if y > 1:
                neighbours.append((y - 2, x))
            if y < H - 2:
                neighbours.append((y + 2, x))
            if not neighbours:
                continue
            pick = below(seed, case, WALK, i * walk + j, len(neighbours) - 1)
            y_, x_ = neighbours[pick]
            taken = maze[y_, x_] == 0
            trace["steps"].append((len(neighbours), pick, bool(taken)))
            if taken:
                maze[y_, x_] = 1
                maze[y_ + (y - y_) // 2, x_ + (x - x_) // 2] = 1
                x, y = x_, y_
    return maze, trace


def raw_uniform(seed, case, H, W, threshold):
    m = np.zeros((H, W), dtype=np.uint8)
    for r in range(H):
        for c in range(W):
            m[r, c] = 1 if u32(seed, case, CELL, r * W + c) < threshold else 0
    return m


def components(free):
    """The 4-connected components of the free cells, each a sorted list of (r, c), in the order of their lowest cell."""
    H, W = free.shape
    seen = np.zeros((H, W), dtype=bool)
    comps = []
    for r0 in range(H):
        for c0 in range(W):
            if not free[r0, c0] or seen[r0, c0]:
                continue
            seen[r0, c0] = True
            queue = [(r0, c0)]
            for r, c in queue:
                for dr, dc in ((-1, 0), (0, -1), (1, 0), (0, 1)):
                    v = (r + dr, c + dc)
                    if 0 <= v[0] < H and 0 <= v[1] < W and free[v] and not seen[v]:
                        seen[v] = True
                        queue.append(v)
            comps.append(sorted(queue))
    return comps


def kept_region(raw):
    """Sorted cells of the largest free component; ties: the component with the lowest row-major cell ([] when none is free)."""
    best = []
    for comp in components(np.asarray(raw) == 0):      # in the order of their lowest cells: a later one must be LARGER to win
        if len(comp) > len(best):
            best = comp
    return best


def draw_tuple(seed, case, stream, first_index, region, N):
    """N distinct cells of `region` (sorted): the below(F - a)-th of those not taken yet."""
    left = list(region)
    F = len(region)
    return [left.pop(below(seed, case, stream, first_index + a, F - a)) for a in range(N)]


def one_case(kind, seed, case, H, W, N, aisles=0, walk=0, threshold=0, given=None):
    trace = None
    if kind == "maze":
        raw, trace = raw_maze(seed, case, H, W, aisles, walk)
    elif kind == "uniform":
        raw = raw_uniform(seed, case, H, W, threshold)
    elif kind == "given":
        raw = (np.asarray(given) != 0).astype(np.uint8)
        assert raw.shape == (H, W)
    else:
        raise KeyError(kind)
    region = kept_region(raw)
    F = len(region)
    out_map = np.ones((H, W), dtype=np.uint8)
    for cell in region:
        out_map[cell] = 0
    start = np.full((N, 2), -1, dtype=np.int32)
    goal = np.full((N, 2), -1, dtype=np.int32)
    valid = 0
    if F >= N + 1:
        starts = draw_tuple(seed, case, START, 0, region, N)
        for rnd in range(ROUNDS):
            goals = draw_tuple(seed, case, GOAL, rnd * N, region, N)
            if all(goals[a] != starts[a] for a in range(N)):
                valid = 1
                start[:] = starts
                goal[:] = goals
                break
    return dict(map=out_map, start=start, goal=goal, free_cells=F, valid=valid, raw=raw, trace=trace)


def generate(kind, C, H, W, N, density=0.1, complexity=0.01, seed=0, first_case=0, maps=None):
    """C cases, stacked.  maps: (H,W) or (C,H,W) for kind "given"."""
    aisles, walk = maze_steps(H, W, density, complexity) if kind == "maze" else (0, 0)
    threshold = min(max(int(density * 4294967296.0), 0), 1 << 32) if kind == "uniform" else 0
    cases = []
    for c in range(C):
        given = None
        if kind == "given":
            given = np.asarray(maps)
            given = given if given.ndim == 2 else given[c]
        cases.append(one_case(kind, int(seed) & MASK, first_case + c, H, W, N, aisles, walk, threshold, given))
    out = {key: np.stack([k[key] for k in cases]) for key in ("map", "start", "goal", "raw")}
    out["free_cells"] = np.array([k["free_cells"] for k in cases], dtype=np.int32)
    out["valid"] = np.array([k["valid"] for k in cases], dtype=np.uint8)
    out["trace"] = [k["trace"] for k in cases]
    out["aisles"], out["walk"] = aisles, walk
    return out


# Hand maps with known answers (rows as strings, '#': obstacle), shared by the CPU and the GPU tests ---------------------------
def grid(rows):
    return np.array([[1 if ch == "#" else 0 for ch in row] for row in rows], dtype=np.uint8)


def serpentine(H, W):
    """Even rows free over the full width, odd rows a wall with one gap at alternating ends: ONE corridor through every free cell."""
    m = np.zeros((H, W), dtype=np.uint8)
    for r in range(1, H, 2):
        m[r, :] = 1
        m[r, W - 1 if (r // 2) % 2 == 0 else 0] = 0
    return m


def checkerboard(H, W):
    return np.fromfunction(lambda r, c: (r + c) % 2, (H, W), dtype=np.int64).astype(np.uint8)


def hand_maps():
    """name -> dict(map, N, free_cells, valid, kept: the cells that must be free in the output, or None).  All 6 x 8, so that
    they stack into one (C,H,W) batch."""
    maps = {}
    # (0, 0) is an obstacle: the reference's flood from (0, 0) would leave nothing; here the 9-cell room is kept
    corner = grid(["#.......",
                   "########",
                   "###...##",
                   "###...##",
                   "###...##",
                   "########"])
    maps["corner_obstacle"] = dict(map=corner, N=3, free_cells=9, valid=1, kept=[(r, c) for r in (2, 3, 4) for c in (3, 4, 5)])
    # two rooms of 6 cells: the one that holds the lower cell index - (0, 5), in the upper right - wins over (1, 0)'s
    tie = grid(["#####...",
                "...##...",
                "...#####",
                "########",
                "########",
                "########"])
    maps["equal_components"] = dict(map=tie, N=2, free_cells=6, valid=1, kept=[(0, 5), (0, 6), (0, 7), (1, 5), (1, 6), (1, 7)])
    snake = serpentine(6, 8)
    maps["serpentine"] = dict(map=snake, N=4, free_cells=int((snake == 0).sum()), valid=1,
                              kept=[tuple(c) for c in np.argwhere(snake == 0)])
    maps["checkerboard"] = dict(map=checkerboard(6, 8), N=1, free_cells=1, valid=0, kept=[(0, 0)])
    # exactly N free cells: invalid; exactly N + 1: valid
    row4 = grid(["########", "##....##", "########", "########", "########", "########"])
    maps["n_free_cells"] = dict(map=row4, N=4, free_cells=4, valid=0, kept=[(1, 2), (1, 3), (1, 4), (1, 5)])
    maps["n_plus_1_free_cells"] = dict(map=row4, N=3, free_cells=4, valid=1, kept=[(1, 2), (1, 3), (1, 4), (1, 5)])
    return maps
