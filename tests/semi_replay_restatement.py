"""Numpy restatement of the replayed SemiLG view (csrc/sim_guidance_parts.h: guide_history_walk, guide_canvas_cell_replay) on
top of tests/guidance_restatement.py - TEST HELPER, no reference code is imported.

The maps are static and the SemiLG encoding writes the map's own crop into the agent's remembered map, so after step t

    half = FOV // 2, padded coordinates (row + half, col + half)
    seen(n)   = union over s = 0..t, with cell_s(n) on the map and goal(n) on the map, of the FOV x FOV window
                rows cell_s.row .. cell_s.row + FOV - 1, columns cell_s.col .. cell_s.col + FOV - 1     (padded coordinates)
    view(r,c) = seen(r,c) AND blocked(r - half, c - half)          blocked = off the map, or map != 0

cell_s(n) follows the rule of expert_schedule: path[s] while s < length, the agent's goal afterwards.

    cells = table_cells(table (T,N,2), t)                                  # (t + 1, N, 2): history source (a), a position table
    cells = store_cells(packed (N,Lcap) uint16, lengths (N,), goal (N,2), t)      # ... source (b), the memory's packed store
    view  = replayed_view(obstacle_map, cells, goal, FOV)                  # (N, H + 2 half, W + 2 half) uint8
    x     = replayed_states(obstacle_map, pos, goal, cells, guidance, FOV)  # (N,3,FOV+2,FOV+2): guided_states on that view
    text  = dump_case(...), parse_result(...)                              # the files of tools/host_wave/semi_replay_check.cpp
"""
import numpy as np

from guidance_restatement import guided_states


def table_cells(table, t):
    """History source (a): rows 0..t of one case's (T,N,2) position table."""
    table = np.asarray(table)
    return table[:int(t) + 1].astype(np.int64)


def pack_cells(paths, lengths, Lcap):
    """One case's (N,Lmax,2) padded paths -> the memory's packed cells (N,Lcap) uint16 = row << 8 | col, cell l of a path being
    its cell min(l, L - 1) (ExpertMemory.append's write)."""
    paths, lengths = np.asarray(paths).astype(np.int64), np.asarray(lengths).astype(np.int64)
    N = paths.shape[0]
    out = np.zeros((N, Lcap), dtype=np.uint16)
    for n in range(N):
        for l in range(Lcap):
            r, c = paths[n, min(l, lengths[n] - 1)]
            out[n, l] = (int(r) << 8) | int(c)
    return out


def store_cells(packed, lengths, goal, t):
    """History source (b): the cells of steps 0..t decoded from the packed store by expert_schedule's rule."""
    packed, lengths, goal = np.asarray(packed), np.asarray(lengths), np.asarray(goal).astype(np.int64)
    N, Lcap = packed.shape
    out = np.zeros((int(t) + 1, N, 2), dtype=np.int64)
    for n in range(N):
        L = min(max(int(lengths[n]), 0), Lcap)
        for s in range(int(t) + 1):
            out[s, n] = (int(packed[n, s]) >> 8, int(packed[n, s]) & 255) if s < L else goal[n]
    return out


def replayed_view(obstacle_map, cells, goal, FOV=9):
    m = np.asarray(obstacle_map) != 0
    H, W = m.shape
    half = FOV // 2
    cells, goal = np.asarray(cells).astype(np.int64), np.asarray(goal).astype(np.int64)
    N = cells.shape[1]
    blocked = np.pad(m, half, constant_values=True)
    seen = np.zeros((N, H + 2 * half, W + 2 * half), dtype=bool)
    for n in range(N):
        if not (0 <= goal[n, 0] < H and 0 <= goal[n, 1] < W):
            continue
        for r, c in cells[:, n]:
            if 0 <= r < H and 0 <= c < W:
                seen[n, r:r + FOV, c:c + FOV] = True
    return (seen & blocked[None]).astype(np.uint8)


def replayed_states(obstacle_map, pos, goal, cells, guidance, FOV=9):
    """The states of the step whose history is `cells`: guided_states on the replayed view (which writes the current crop into
    it, as the carried form does)."""
    view = replayed_view(obstacle_map, cells, goal, FOV)
    return guided_states(obstacle_map, pos, goal, guidance, FOV, agent_view=view)


# ---- the text files of tools/host_wave/semi_replay_check.cpp ------------------------------------------------------------------------
def dump_case(maps, pos, goal, row_case, row_step, FOV, wide, table=None, store=None):
    """maps (B,H,W), pos / goal (B,N,2), row_case / row_step (B,), table (cases,T,N,2) or store = (packed (cases,N,Lcap), lengths
    (cases,N), goal (cases,N,2)) -> the check program's input."""
    maps, pos, goal = np.asarray(maps), np.asarray(pos), np.asarray(goal)
    B, H, W = maps.shape
    N = pos.shape[1]
    flat = lambda a: " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))      # noqa: E731
    if table is not None:
        cases, T = table.shape[0], table.shape[1]
        head, body = [cases, T, 0], [flat(table)]
    else:
        packed, lengths, hgoal = store
        cases, Lcap = packed.shape[0], packed.shape[2]
        head, body = [cases, 0, Lcap], [flat(packed), flat(lengths), flat(hgoal)]
    lines = [flat([B, N, H, W, FOV, 1 if wide else 0, 1 if table is not None else 0] + head), flat(maps), flat(pos), flat(goal),
             flat(row_case), flat(row_step)] + body
    return "\n".join(lines) + "\n"


def parse_result(text, B, N, FOV):
    """-> (return code, x (B,N,3,FOV+2,FOV+2) uint8)."""
    lines = text.strip().split("\n")
    rc = int(lines[0])
    x = np.array(lines[1].split(), dtype=np.int64).reshape(B, N, 3, FOV + 2, FOV + 2).astype(np.uint8)
    return rc, x
