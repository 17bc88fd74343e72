"""Plain restatement of the package's conflict-based search (magat_pathplanning_amd/mapf.py cbs_cases, csrc/sim_mapf_cbs.hip),
written from DESIGN 4.11 / include/magat_hip.h with per-cell loops over boolean arrays - TEST HELPER, deliberately not
bitboards.  The low-level search and its backtrace are mapf_restatement's (the planner's own), run on boards that hold one
agent's CONSTRAINTS instead of other agents' paths; the first-conflict scan is written out here, in the audit's stage-2 order.

    out = cbs(obstacle_map (H,W), start (N,2), goal (N,2), T, max_nodes=256)      # one case
    out = cbs_batch(maps, start (C,N,2), goal (C,N,2), T, max_nodes=256)          # stacked, the layout of cbs_cases

Per case:
  * screening - a start or goal off the map or on an obstacle, or a start (goal) shared by two agents: status 3; else the root:
    every agent's free path (the search on empty boards); an agent without an arrival inside T: status 2, horizon_hit 1.
    Neither creates a node.
  * node - parent, the re-planned agent, ONE constraint (board, t, cell), cost = sum(lengths - 1), that agent's new path.  A
    node's schedule is, per agent, the path of the nearest ancestor (itself included) that re-planned it, else the root's.  An
    agent's constraints are those of the nodes on the chain to the root that re-planned it.
  * constraint - vertex (agent, cell u, t): u in V[t]; "may not step from u in direction d, arriving at t": u in A_opp(d)[t].
  * loop - take the open node with the smallest (cost, index); find the first conflict of its schedule: the smallest (t, a, b),
    a < b, vertex before swap.  None: status 0.  nodes + 2 > max_nodes: status 1, lower_bound = this node's cost.  Otherwise
    expanded += 1 and two children, for a then for b: the cell at t (vertex) or the agent's own step at t (swap) is forbidden,
    the agent is searched again under all its constraints; cost = the parent's - old length + new length.  A child without
    an arrival keeps its slot, never opens, and sets horizon_hit.  An empty open list: status 2.
  * outputs - paths (N,T,2) int32 padded with the last cell, lengths, makespan, solved = (status == 0), status, flowtime (-1
    unless status 0), lower_bound (status 0: the flowtime; 1: the cost of the node it stopped at; else -1), nodes (created,
    the root included), expanded (nodes whose two children were made), horizon_hit.  Unsolved: every agent's start cell,
    length 1, makespan 0."""
import numpy as np

from mapf_restatement import MOVES, OPP, _backtrace, _case_map, _inside, _search


def first_conflict(paths, lengths):
    """(kind, t, a, b) - kind 0 vertex, 1 swap - of the first conflict of per-agent cell lists (an agent holds its last cell),
    or None.  Behind the longest path nothing moves and every pair was compared on its last cells, so the scan ends there."""
    N = len(paths)
    span = max(lengths)
    at = lambda a, t: paths[a][t if t < lengths[a] else lengths[a] - 1]      # noqa: E731
    for t in range(span):
        for a in range(N):
            for b in range(a + 1, N):
                if at(a, t) == at(b, t):
                    return 0, t, a, b
                if t >= 1 and at(a, t) == at(b, t - 1) and at(b, t) == at(a, t - 1) and at(a, t) != at(a, t - 1):
                    return 1, t, a, b
    return None


def _constraint(kind, t, path, length):
    """The constraint that forbids an agent's own part of a conflict at t: (board, t, cell) - board 0: V, 1 + k: A_k."""
    here = path[t if t < length else length - 1]
    if kind == 0:
        return 0, t, here
    src = path[t - 1]
    d = MOVES.index((here[0] - src[0], here[1] - src[1]))
    return 1 + OPP[d], t, src


def cbs(obstacle_map, start, goal, T, max_nodes=256):
    m = np.asarray(obstacle_map)
    free = m == 0
    H, W = free.shape
    start, goal = np.asarray(start, dtype=np.int64).reshape(-1, 2), np.asarray(goal, dtype=np.int64).reshape(-1, 2)
    N, T, max_nodes = len(start), int(T), int(max_nodes)
    out = dict(paths=np.repeat(start[:, None, :], T, axis=1).astype(np.int32), lengths=np.ones(N, dtype=np.int32), makespan=0,
               solved=0, status=3, flowtime=-1, lower_bound=-1, nodes=0, expanded=0, horizon_hit=0)
    S, G = [tuple(int(v) for v in s) for s in start], [tuple(int(v) for v in g) for g in goal]
    for a in range(N):
        if not (_inside(S[a], H, W) and _inside(G[a], H, W) and bool(free[S[a]]) and bool(free[G[a]])):
            return out
        if S[a] in S[:a] or G[a] in G[:a]:
            return out
    boards = [[np.zeros((H, W), dtype=bool) for _ in range(T)] for _ in range(5)]      # V, A_up, A_left, A_down, A_right
    V, A = boards[0], boards[1:]
    root_paths, root_len = [], []
    for a in range(N):
        R, tstar = _search(free, V, A, S[a], G[a], T)
        if tstar < 0:
            out.update(status=2, horizon_hit=1)
            return out
        root_paths.append(_backtrace(R, A, G[a], tstar))
        root_len.append(tstar + 1)
    nodes = [dict(parent=-1, agent=-1, con=None, cost=sum(root_len) - N, path=None, length=0, open=True)]
    expanded = hit = 0

    def chain(i):
        while i > 0:
            yield nodes[i]
            i = nodes[i]["parent"]

    while True:
        best = -1
        for i, nd in enumerate(nodes):
            if nd["open"] and (best < 0 or nd["cost"] < nodes[best]["cost"]):
                best = i
        if best < 0:
            out.update(status=2, nodes=len(nodes), expanded=expanded, horizon_hit=hit)
            return out
        nodes[best]["open"] = False
        paths, lengths = list(root_paths), list(root_len)
        seen = set()
        for nd in chain(best):
            if nd["agent"] not in seen:
                seen.add(nd["agent"])
                paths[nd["agent"]], lengths[nd["agent"]] = nd["path"], nd["length"]
        cost = nodes[best]["cost"]
        conflict = first_conflict(paths, lengths)
        if conflict is None:
            for a in range(N):
                for t in range(T):
                    out["paths"][a, t] = paths[a][min(t, lengths[a] - 1)]
            out["lengths"][:] = lengths
            assert cost == sum(lengths) - N
            out.update(makespan=max(lengths) - 1, solved=1, status=0, flowtime=cost, lower_bound=cost, nodes=len(nodes),
                       expanded=expanded, horizon_hit=hit)
            return out
        if len(nodes) + 2 > max_nodes:
            out.update(status=1, lower_bound=cost, nodes=len(nodes), expanded=expanded, horizon_hit=hit)
            return out
        expanded += 1
        kind, t, a, b = conflict
        for x in (a, b):
            con = _constraint(kind, t, paths[x], lengths[x])
            mine = [con] + [nd["con"] for nd in chain(best) if nd["agent"] == x]
            for bd, tt, cell in mine:
                boards[bd][tt][cell] = True
            R, tstar = _search(free, V, A, S[x], G[x], T)
            child = dict(parent=best, agent=x, con=con, cost=-1, path=None, length=0, open=False)
            if tstar >= 0:
                child.update(path=_backtrace(R, A, G[x], tstar), length=tstar + 1, cost=cost - lengths[x] + tstar + 1, open=True)
            else:
                hit = 1
            for bd, tt, cell in mine:
                boards[bd][tt][cell] = False
            nodes.append(child)


def cbs_batch(maps, start, goal, T, max_nodes=256):
    outs = [cbs(_case_map(maps, c), start[c], goal[c], T, max_nodes) for c in range(len(start))]
    return {key: np.stack([np.asarray(o[key]) for o in outs]).astype(np.uint8 if key == "solved" else np.int32) for key in outs[0]}


def pocket_swap():
    """Two agents swap the ends of a corridor with one pocket: prioritized planning fails in every order."""
    from mapf_restatement import grid
    return dict(map=grid(["#####", ".....", "## ##"]), start=np.array([(1, 1), (1, 3)], dtype=np.int32),
                goal=np.array([(1, 3), (1, 1)], dtype=np.int32), T=16)
