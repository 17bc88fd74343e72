"""Numpy restatement of the reference's A*-guided state encodings (dataloader/statetransformer_Guidance.py:241-495 with
offlineExpert/a_star.py:75-189), written from their specification - TEST HELPER, no reference code is imported.

tests/test_host_guidance.py pins it against every guid_* fixture (made by the real AgentState), after which the GPU tests use it
as the expected value on scenarios the fixtures do not hold.

    x = guided_states(obstacle_map (H,W), pos (N,2), goal (N,2), guidance, FOV=9, agent_view=None)     # (N,3,FOV+2,FOV+2) uint8
    view = new_agent_view(N, H, W, FOV)            # SemiLG_*: the agents' remembered maps, updated in place by every call
"""
import heapq

import numpy as np

GUIDANCE = ("LocalG_S", "LocalG_SD", "GlobalG_S", "GlobalG_SD", "SemiLG_S", "SemiLG_SD")
MOVES = ((-1, 0), (0, -1), (1, 0), (0, 1))            # up, left, down, right: the order the neighbours are pushed in


def a_star(grid, start, goal):
    """The reference's planner: pop = lexicographic minimum of (f, g, row, col); a cell is closed when PUSHED and keeps its
    first pusher as parent; only cells with grid == 0 are entered (the start is never tested); no path -> [start].
    Returns (path as a list of (row, col) from start to goal, number of pops)."""
    R, C = grid.shape
    closed = np.zeros((R, C), dtype=bool)
    parent = np.full((R, C), -1, dtype=np.int64)
    closed[start] = True
    heap = [(abs(start[0] - goal[0]) + abs(start[1] - goal[1]), 0, start[0], start[1])]
    pops = 0
    while heap:
        _, g, r, c = heapq.heappop(heap)              # entries are unique in (row, col): the heap order IS the sorted order
        pops += 1
        if (r, c) == tuple(goal):
            path = [(r, c)]
            while (r, c) != tuple(start):
                d = MOVES[parent[r, c]]
                r, c = r - d[0], c - d[1]
                path.append((r, c))
            return path[::-1], pops
        for i, (dr, dc) in enumerate(MOVES):
            r2, c2 = r + dr, c + dc
            if 0 <= r2 < R and 0 <= c2 < C and not closed[r2, c2] and grid[r2, c2] == 0:
                closed[r2, c2] = True
                parent[r2, c2] = i
                heapq.heappush(heap, (g + 1 + abs(r2 - goal[0]) + abs(c2 - goal[1]), g + 1, r2, c2))
    return [tuple(start)], pops


def projected_goal(pos, goal, FOV):
    """(row, col) of the goal marker in the (FOV+2)^2 window when the goal lies outside the FOV (projectedgoal, :101-120)."""
    dist = (FOV + 2) // 2
    dx, dy = float(goal[0] - pos[0]), float(goal[1] - pos[1])
    angle = np.arctan2(dy, dx)
    if (np.pi / 4 <= angle <= np.pi * 3 / 4) or (-np.pi * 3 / 4 <= angle <= -np.pi / 4):
        return int(dist + np.round(dist * dx / abs(dy))), int(dist * (np.sign(dy) + 1))
    return int(dist * (np.sign(dx) + 1)), int(dist + np.round(dist * dy / abs(dx)))


def new_agent_view(N, H, W, FOV=9):
    half = FOV // 2
    return np.zeros((N, H + 2 * half, W + 2 * half), dtype=np.uint8)


def guided_states(obstacle_map, pos, goal, guidance, FOV=9, agent_view=None, stats=None):
    if guidance not in GUIDANCE:
        raise ValueError("guidance must be one of %s" % (GUIDANCE,))
    mode, dyn = guidance.split("_")[0], guidance.endswith("_SD")
    m = (np.asarray(obstacle_map) != 0).astype(np.int64)
    H, W = m.shape
    pos, goal = np.asarray(pos).astype(np.int64), np.asarray(goal).astype(np.int64)
    N = pos.shape[0]
    half, Wt = FOV // 2, FOV + 2
    dist = Wt // 2
    map_pad = np.pad(m, half, constant_values=1)
    occ = np.zeros((H, W), dtype=np.int64)
    occ[pos[:, 0], pos[:, 1]] = 1
    occ_pad = np.pad(occ, half, constant_values=0)
    if mode == "SemiLG":
        if agent_view is None:
            raise ValueError("SemiLG_* needs agent_view")
        assert agent_view.shape == (N,) + map_pad.shape
    x = np.zeros((N, 3, Wt, Wt), dtype=np.uint8)
    for n in range(N):
        cx, cy = int(pos[n, 0]), int(pos[n, 1])
        gx, gy = int(goal[n, 0]), int(goal[n, 1])
        wmap = map_pad[cx:cx + FOV, cy:cy + FOV]
        wocc = occ_pad[cx:cx + FOV, cy:cy + FOV]
        x[n, 0, 1:-1, 1:-1] = wmap
        if not (mode == "LocalG" and not dyn):         # LocalG_S writes the agent channel as zeros
            x[n, 2, 1:-1, 1:-1] = wocc
        if mode == "LocalG":
            if abs(gx - cx) <= half and abs(gy - cy) <= half:
                g = (gx - cx + half + 1, gy - cy + half + 1)
            else:
                g = projected_goal((cx, cy), (gx, gy), FOV)
            grid = np.zeros((Wt, Wt), dtype=np.int64)                     # free border ring
            grid[1:-1, 1:-1] = wmap + (wocc if dyn else 0)
            grid[dist, dist] = 0
            if dyn and 1 <= g[0] <= FOV and 1 <= g[1] <= FOV and wocc[g[0] - 1, g[1] - 1]:
                grid[g] = 0                                               # an agent stands on the goal cell
            path, pops = a_star(grid, (dist, dist), g)
            x[n, 1][g] = 1
            for r, c in path:
                x[n, 1, r, c] = 1
        else:
            if mode == "SemiLG":
                agent_view[n, cx:cx + FOV, cy:cy + FOV] = wmap            # BEFORE the search
                base = agent_view[n].astype(np.int64)
            else:
                base = map_pad.copy()
            if dyn or mode == "SemiLG":
                base[cx:cx + FOV, cy:cy + FOV] += wocc
            grid = np.pad(base, 1, constant_values=0)                     # free one-cell ring
            s, g = (cx + half + 1, cy + half + 1), (gx + half + 1, gy + half + 1)
            if grid[g] == 1:
                grid[g] = 0
            path, pops = a_star(grid, s, g)
            canvas = np.zeros_like(grid)
            for r, c in path:
                canvas[r, c] = 1
            x[n, 1] = canvas[cx:cx + Wt, cy:cy + Wt]
        if stats is not None:
            stats.append(dict(pops=pops, path=path, goal=g))
    return x
