"""A multi-agent path-finding expert on the device: the solver at the head of the expert pipeline (expert.py turns ITS
schedules into training samples), for C cases at once.  The reference calls pre-built ecbs / cbs / sipp binaries, one
subprocess per case (onlineExpert/ECBS_onlineExpert.py:81-104); this is prioritized planning with an exact space-time search
per agent (csrc/sim_mapf.hip).  The planner is NOT ECBS: it gives no bound on the flowtime, and it is incomplete - a
case can fail in one priority order and succeed in another, or stay unsolved.  Behind it stand an optimal solver that is
complete up to a node budget, conflict-based search (cbs_cases, csrc/sim_mapf_cbs.hip; solve_cases(..., optimal=K)), and ECBS
itself, its bounded-suboptimal form (ecbs_cases, csrc/sim_mapf_ecbs.hip; solve_cases(..., bounded=w)) - see below.

    res = solve_cases(obstacle_map, start, goal)                          # plans, re-plans the unsolved cases in a new order
    pack = solved_pack(res)                                               # the solved cases, as pack_schedules lays them out
    s = expert_samples(obstacle_map, comm_radius=config.commR, **pack)    # (a (C,H,W) map: index it with pack_cases(res))

The online expert - re-solving the cases a running episode is failing at, from where the agents stand now:

    ep = BatchedEpisode(obstacle_map, pos, goal, maxstep, comm_radius=config.commR)
    ... ep.step(logits) ...
    res = solve_cases(ep.map, ep.pos, ep.goal)                            # schedules that start at the current positions
    online_expert(ep, mem)                                                # memory.py: the failed cases only, ECBS(1.1), appended to mem

Prioritized planning in index order never revisits a choice: agents early in the order get shortest paths, the late ones what
is left.  improve_schedules (csrc/sim_mapf_lns.hip) repairs some of that by neighbourhood re-planning (MAPF-LNS): per
iteration it takes the most delayed agents' turn, pulls the agents standing in its free path out of the reservation table
with it, plans them again in that order and keeps the result only when their summed length drops.  solve_cases(...,
improve=I) runs it on the final batch.  This is STILL not ECBS and bounds nothing - the flowtime never rises, that is all.

    better = improve_schedules(obstacle_map, res, iterations=32, neighbourhood=4)      # the same keys, + flowtime_before / _after

What the solver does not promise can be checked after the fact, case by case: audit_schedules (csrc/sim_mapf_audit.hip)
looks for the first fault of every schedule - a cell off the map, a step that is no move, a vertex conflict or a swap between
two agents - and computes the classic lower bound of the optimal flowtime, the sum over the agents of the obstacle-avoiding
shortest distance from start to goal.  A valid schedule with flowtime <= w * bound is certified w-suboptimal: ECBS(w)'s promise,
given afterwards.  It takes any schedules in pack_schedules' layout, the solver's or somebody else's.

    audit = audit_schedules(obstacle_map, res)              # status, fault, dist, flowtime_bound, makespan_bound, flowtime, makespan
    keep = certified(audit, 1.05)                           # (C,) bool on the device
    pack = certified_pack(res, audit, 1.05)                 # solved_pack restricted to the certified cases
    res = solve_cases(obstacle_map, start, goal, certify=1.05)      # the audit's keys and `certified` in the result

What the planner cannot do at all - two agents that must pass each other in a corridor with one pocket fail in EVERY priority
order - conflict-based search does: cbs_cases (csrc/sim_mapf_cbs.hip) branches on the first conflict of a schedule, re-plans one
agent per child under that agent's constraints with the planner's own search, and takes nodes best-first.  It is optimal in the
flowtime, deterministic and complete up to max_nodes; where the budget runs out, the cost of the node it stopped at is still a
lower bound of the optimal flowtime - a much tighter denominator for `certified` than the sum of the free distances.

    opt = cbs_cases(obstacle_map, start, goal, max_nodes=256)             # status, flowtime, lower_bound, nodes, expanded, horizon_hit
    res = solve_cases(obstacle_map, start, goal, optimal=256, certify=1.0)      # the planner's schedule unless CBS proved an optimum

CBS proves optima and therefore runs out of its budget on anything crowded.  ecbs_cases (csrc/sim_mapf_ecbs.hip) is ECBS(w): the
same tree with a focal search on both levels - the low level prefers paths that break few of the other agents' reservations among
those at most w times the shortest, the high level takes the node with the fewest conflicts among those whose cost is within w of
the smallest bound of the open list.  A solved case promises flowtime <= w * lower_bound <= w * optimum.

    sub = ecbs_cases(obstacle_map, start, goal, w=1.5, max_nodes=256)           # cbs_cases' keys
    res = solve_cases(obstacle_map, start, goal, bounded=1.5, certify=1.5)      # ECBS's schedule where it is the better one

Maps above 64 x 64 and horizons above 256 are opt-in everywhere: plan_prioritized, solve_cases, improve_schedules and
audit_schedules take wide=True (csrc/sim_mapf_wide.hip, csrc/sim_mapf_lns_wide.hip, csrc/sim_mapf_audit_wide.hip: maps up to
256 x 256, horizons up to 1024), and solve_cases(..., wide=True, improve=I, certify=w) hands it on; without it such shapes raise
MagatNativeError as before.  ECBS's wide form comes under a name of its own, ecbs_cases_wide (csrc/sim_mapf_ecbs_wide.hip: the
same rule on maps up to 256 x 256 with horizons up to 1024), with adopt_bounded - solve_cases(bounded=)'s replacement rule as a
function - to put its schedules into a result:

    res = solve_cases(obstacle_map, start, goal, wide=True, improve=32)
    sub = ecbs_cases_wide(obstacle_map, start, goal, 1.5, horizon=res["paths"].shape[2])
    res = adopt_bounded(res, sub)                           # + ecbs_status, ecbs_bound, ecbs_nodes, bounded
    audit = audit_schedules(obstacle_map, res, wide=True)

ecbs_cases and solve_cases(bounded=) themselves refuse such shapes with or without wide=True, as before.  cbs_cases has no wide
form yet (ecbs_cases_wide at w = 1 gives the optimal flowtime).

HIP only: CPU tensors raise MagatNativeError.  plan_prioritized is stream ordered and never waits for the device;
solve_cases reads `solved` back once per round."""
import torch

from . import _native as nat
from . import _sim_host as sh

MAX_HORIZON = 256
MAX_SIDE = 64
WIDE_MAX_HORIZON = 1024      # the wide forms (csrc/sim_mapf_wide.hip, csrc/sim_mapf_lns_wide.hip): maps up to 256 x 256
WIDE_MAX_SIDE = 256
PACK_KEYS = ("paths", "lengths", "goal", "start", "makespan")
MAX_AGENTS_AUDIT = 4096      # audit_schedules: agents per case
AUDIT_KEYS = ("status", "fault", "dist", "flowtime_bound", "makespan_bound", "flowtime", "makespan")
MAX_NODES_CBS = 4096         # cbs_cases, ecbs_cases: nodes per case
MAX_LEVELS_ECBS = 4          # ecbs_cases: planes of the low-level focal search
MAX_W_MILLI_ECBS = 1 << 20   # ecbs_cases: round(1000 w)


def default_horizon(H, W, N, wide=False):
    return min(WIDE_MAX_HORIZON if wide else MAX_HORIZON, 2 * (H + W) + N)


def _route(H, W, T, wide, refuses=True):
    """Which form serves an H x W map with horizon T: "narrow", "wide" or "refuse".  A shape inside the narrow limits goes to the
    narrow entry with or without wide=True (plan_prioritized's rule).  Beyond them improve_schedules, audit_schedules and the
    searches refuse in Python, in _limits' words, unless wide=True and the shape is inside the wide limits.  plan_prioritized
    (refuses=False) never does: it hands the shape to the entry the keyword names, and the library refuses."""
    if H <= MAX_SIDE and W <= MAX_SIDE and T <= MAX_HORIZON:
        return "narrow"
    if not refuses:
        return "wide" if wide else "narrow"
    return "wide" if wide and H <= WIDE_MAX_SIDE and W <= WIDE_MAX_SIDE and T <= WIDE_MAX_HORIZON else "refuse"


def _limits(who, H, W, T, N=None, max_nodes=None, levels=None, wide=False, keyword=False):
    """The shape refusal of improve_schedules, audit_schedules, cbs_cases, ecbs_cases, ecbs_cases_wide and of solve_cases'
    early check, in the name of `who`: MagatNativeError naming what the caller takes and what it got.  N, max_nodes, levels: given
    where the caller has that limit.  wide: the wide forms' limits apply.  keyword: the caller takes wide= itself (the message
    says what the keyword would lift, and N has a refusal of its own behind the shape's)."""
    side, horizon = (WIDE_MAX_SIDE, WIDE_MAX_HORIZON) if wide else (MAX_SIDE, MAX_HORIZON)
    takes, got = ["maps up to %d x %d" % (side, side), "horizons up to %d" % horizon], ["%d x %d" % (H, W), "%d" % T]
    bad = _route(H, W, T, wide) == "refuse"
    name = who + "(wide=True)" if keyword and wide else who
    if keyword:
        tail = "" if wide else (" (wide=True takes maps up to %d x %d and horizons up to %d)"
                                % (WIDE_MAX_SIDE, WIDE_MAX_SIDE, WIDE_MAX_HORIZON))
    else:
        tail = "" if wide else " (it has no wide form)"
        for value, text, least, most in ((N, "%d agents", 0, MAX_AGENTS_AUDIT), (max_nodes, "1..%d nodes per case", 1, MAX_NODES_CBS),
                                         (levels, "1..%d levels", 1, MAX_LEVELS_ECBS)):
            if value is not None:
                takes.append(text % most)
                got.append("%d" % value)
                bad = bad or not least <= value <= most
    if bad:
        raise nat.MagatNativeError("%s takes %s and %s, not %s%s" % (name, ", ".join(takes[:-1]), takes[-1], " / ".join(got), tail))
    if keyword and N is not None and N > MAX_AGENTS_AUDIT:
        raise nat.MagatNativeError("%s takes at most %d agents per case, not %d" % (who, MAX_AGENTS_AUDIT, N))


def plan_prioritized(obstacle_map, start, goal, order=None, horizon=None, wide=False):
    """One call of magat_sim_mapf_plan: obstacle_map (H,W) or (C,H,W) (non-zero: obstacle; H, W <= 64), start / goal (C,N,2)
    (row, col), order (C,N): each case's priority order, a permutation of its agents (None: index order).  Agents are planned
    one after another; each takes the earliest arrival that the agents before it leave open, waits included, and holds its
    goal from then on.  Returns a dict of device tensors: paths (C,N,horizon,2) int32 padded with each path's last cell,
    lengths (C,N), goal, start (C,N,2), makespan (C,) = max lengths - 1 (pack_schedules' layout), solved (C,) uint8 and
    failed_agent (C,) int32 - -1, or the agent at which the case stopped: no arrival inside the horizon, a start or goal off
    the map, on an obstacle or shared with an agent earlier in the order; -2: the order row is no permutation.  In an unsolved
    case the agents before the failure keep their paths, the others get their start cell with length 1.

    horizon: the most cells a path may have, at most 256; the default min(256, 2 * (H + W) + N) is a default, not a
    guarantee - it has not been measured against any family of maps, and a case whose agents need longer comes back unsolved.

    wide=True lifts the limits to H, W <= 256 and horizon <= 1024 (default min(1024, 2 * (H + W) + N), likewise not measured
    against any family of maps): a shape with H, W <= 64 and horizon <= 256 still goes to magat_sim_mapf_plan, with the same
    result as wide=False; a larger one to magat_sim_mapf_plan_wide - the same algorithm, one workgroup per case, and a
    workspace of horizon * 6 * 64 ceil(H / 64) * (1, 2 or 4 words >= W / 64) * 8 bytes per case.  wide=False refuses H or W
    above 64 and horizons above 256 as before.
    Stream ordered, no host synchronisation."""
    m, batched, start, goal, C, N, H, W = sh.dev_cases(obstacle_map, start, goal)
    if order is not None:
        order = sh.dev_i32(order, "order")
        assert tuple(order.shape) == (C, N), "order must be (C,N)"
    T = default_horizon(H, W, N, wide) if horizon is None else int(horizon)
    dev = start.device
    lib = nat.lib()
    to_wide = _route(H, W, T, wide, refuses=False) == "wide"
    paths = torch.empty(C, N, T, 2, dtype=torch.int32, device=dev)
    lengths = torch.empty(C, N, dtype=torch.int32, device=dev)
    makespan = torch.empty(C, dtype=torch.int32, device=dev)
    solved = torch.empty(C, dtype=torch.uint8, device=dev)
    failed = torch.empty(C, dtype=torch.int32, device=dev)
    ws = sh.scratch(lib.magat_sim_mapf_wide_workspace_bytes(C, H, W, T) if to_wide else lib.magat_sim_mapf_workspace_bytes(C, T), dev)
    sh.call(dev, "magat_sim_mapf_plan_wide" if to_wide else "magat_sim_mapf_plan", nat.ptr(m), batched, H, W, nat.ptr(start),
            nat.ptr(goal), nat.ptr(order), nat.ptr(paths), nat.ptr(lengths), nat.ptr(makespan), nat.ptr(solved), nat.ptr(failed),
            nat.ptr(ws), ws.numel(), C, N, T)
    return dict(paths=paths, lengths=lengths, goal=goal, start=start, makespan=makespan, solved=solved, failed_agent=failed)


def promote(order, agent):
    """order (K,N), agent (K,): each row with its agent moved to the front, the others keeping their relative order (tensor
    ops on the device)."""
    hit = order == agent[:, None].to(order.dtype)
    rest = torch.argsort(hit.to(torch.int8), dim=1, descending=True, stable=True)      # the hit first, then the old order
    return torch.gather(order, 1, rest)


def improve_schedules(obstacle_map, res, iterations=32, neighbourhood=4, wide=False):
    """One call of magat_sim_mapf_improve on a plan_prioritized / solve_cases result `res` (obstacle_map: the map it was planned
    on, (H,W) or (C,H,W)): `iterations` rounds of neighbourhood re-planning per case with neighbourhoods of up to
    `neighbourhood` (1..8) agents - the rule is in include/magat_hip.h and DESIGN 4.11; deterministic, no random numbers.
    Returns a NEW dict with every key of `res` - paths, lengths and makespan are new tensors, the others are shared - plus
    flowtime_before, flowtime_after (C,) int32 = sum(lengths - 1), accepted (C,) int32 and status (C,) int32: 0 improved or
    unchanged; 1 skipped, the case is unsolved; 2 refused - a length outside 1..horizon, a cell off the map or on an obstacle,
    a step that is none of the five moves.  Skipped and refused cases come back as they were.  The tensors of `res` are not
    modified; a `T` key (solve_cases) is left out of the copy, since it would need a synchronisation - solved_pack computes it.
    Not ECBS: no bound on the flowtime; it never rises, and a valid schedule stays valid.  Conflicts between the agents of
    `res` are not looked for - the result is then unspecified (audit_schedules looks for them).
    wide=False: maps above 64 x 64 and horizons above 256 (results of wide=True at such shapes) raise MagatNativeError.
    wide=True lifts the limits to H, W <= 256 and horizons up to 1024, by plan_prioritized's rule: a shape with H, W <= 64 and
    horizon <= 256 still goes to magat_sim_mapf_improve, with the same result as wide=False; a larger one to
    magat_sim_mapf_improve_wide (csrc/sim_mapf_lns_wide.hip) - the same rule, one workgroup per case, and a workspace of
    horizon * 6 * 64 ceil(H / 64) * (1, 2 or 4 words >= W / 64) * 8 + 8 ceil(N / 2) bytes per case.  Beyond those limits it
    raises MagatNativeError.
    Stream ordered, no host synchronisation."""
    paths = res["paths"]
    m, batched, C, N, T, H, W = sh.dev_schedules(obstacle_map, paths)
    _limits("improve_schedules", H, W, T, wide=bool(wide), keyword=True)
    to_wide = _route(H, W, T, wide) == "wide"
    dev = paths.device
    out = {key: value for key, value in res.items() if key != "T"}
    out["paths"] = sh.dev_i32(paths, "paths").clone()
    out["lengths"] = sh.dev_i32(res["lengths"], "lengths").clone()
    out["makespan"] = sh.dev_i32(res["makespan"], "makespan").clone()
    solved = res["solved"].to(torch.uint8).contiguous()
    assert tuple(out["lengths"].shape) == (C, N) and out["makespan"].numel() == C and solved.numel() == C
    extra = torch.empty(4, C, dtype=torch.int32, device=dev)
    lib = nat.lib()
    ws = sh.scratch(lib.magat_sim_mapf_improve_wide_workspace_bytes(C, H, W, N, T) if to_wide
                    else lib.magat_sim_mapf_improve_workspace_bytes(C, N, T), dev)
    sh.call(dev, "magat_sim_mapf_improve_wide" if to_wide else "magat_sim_mapf_improve", nat.ptr(m), batched, H, W, nat.ptr(solved),
            nat.ptr(out["paths"]), nat.ptr(out["lengths"]), nat.ptr(out["makespan"]), nat.ptr(extra[0]), nat.ptr(extra[1]),
            nat.ptr(extra[2]), nat.ptr(extra[3]), nat.ptr(ws), ws.numel(), C, N, T, int(iterations), int(neighbourhood))
    out.update(flowtime_before=extra[0], flowtime_after=extra[1], accepted=extra[2], status=extra[3])
    return out


def audit_schedules(obstacle_map, res, wide=False):
    """One call of magat_sim_mapf_audit on schedules in pack_schedules' layout: `res` is any dict with paths (C,N,T,2), lengths
    (C,N), start and goal (C,N,2) and optionally solved (C,) - a plan_prioritized, solve_cases or improve_schedules result or a
    pack_schedules pack; a `T` or `makespan` key is ignored.  obstacle_map (H,W) or (C,H,W), non-zero: obstacle.  Returns a dict
    of new int32 device tensors (the rule is in include/magat_hip.h and DESIGN 4.11):
      status (C,)          0 valid; 1 skipped (`solved` given and zero); 2 a fault was found
      fault (C,4)          (kind, t, a, b) of the FIRST fault, (0,-1,-1,-1) without one or when skipped.  Stage 1, agents in index
                           order, per agent in this order: 1 a length outside 1..T (t = -1); 2 paths[a,0] != start[a]; 3
                           paths[a,L-1] != goal[a]; then for t ascending 4 a cell off the map or on an obstacle, 5 t >= L and the
                           cell differs from the one at L-1, 6 a step that is none of the five moves (b = -1).  Stage 2, only
                           without a stage-1 fault: the smallest (t, a, b), a < b, vertex before swap - 7 both on one cell at t
                           (padding counts: an agent holds its goal), 8 they exchange their cells between t-1 and t.
      dist (C,N)           the shortest 4-connected distance over free cells from start[a] to goal[a], other agents ignored; -1
                           when a cell is off the map or on an obstacle or there is no way
      flowtime_bound, makespan_bound (C,)      sum and max of dist, -1 when a dist of the case is -1 - for EVERY case: the
                           optimal flowtime / makespan of the case is at least this
      flowtime, makespan (C,)                  sum and max of lengths - 1 for status 0, otherwise -1
    Bad input is reported, never followed: no cell indexes anything before it was screened.  The inputs are not modified.
    wide=False: maps above 64 x 64 and horizons above 256 raise MagatNativeError.  wide=True lifts the limits to H, W <= 256
    and horizons up to 1024, by plan_prioritized's rule: a shape inside the 64 limits still goes to magat_sim_mapf_audit, a
    larger one to magat_sim_mapf_audit_wide (csrc/sim_mapf_audit_wide.hip) - the same rule, one workgroup per case.  At most
    4096 agents per case.  Stream ordered, no host synchronisation."""
    paths = res["paths"]
    m, batched, C, N, T, H, W = sh.dev_schedules(obstacle_map, paths)
    _limits("audit_schedules", H, W, T, N, wide=bool(wide), keyword=True)
    to_wide = _route(H, W, T, wide) == "wide"
    paths = sh.dev_i32(paths, "paths")
    lengths, start, goal = sh.dev_i32(res["lengths"], "lengths"), sh.dev_i32(res["start"], "start"), sh.dev_i32(res["goal"], "goal")
    assert tuple(lengths.shape) == (C, N) and tuple(start.shape) == (C, N, 2) and tuple(goal.shape) == (C, N, 2)
    solved = res["solved"].to(torch.uint8).contiguous() if res.get("solved") is not None else None
    assert solved is None or solved.numel() == C
    dev = paths.device
    status = torch.empty(C, dtype=torch.int32, device=dev)
    fault = torch.empty(C, 4, dtype=torch.int32, device=dev)
    dist = torch.empty(C, N, dtype=torch.int32, device=dev)
    extra = torch.empty(4, C, dtype=torch.int32, device=dev)
    lib = nat.lib()
    ws = sh.scratch(lib.magat_sim_mapf_audit_wide_workspace_bytes(C, H, W, N, T) if to_wide
                    else lib.magat_sim_mapf_audit_workspace_bytes(C, N, T), dev)
    sh.call(dev, "magat_sim_mapf_audit_wide" if to_wide else "magat_sim_mapf_audit", nat.ptr(m), batched, H, W, nat.ptr(solved),
            nat.ptr(paths), nat.ptr(lengths), nat.ptr(start), nat.ptr(goal), nat.ptr(status), nat.ptr(fault), nat.ptr(dist),
            nat.ptr(extra[0]), nat.ptr(extra[1]), nat.ptr(extra[2]), nat.ptr(extra[3]), nat.ptr(ws), ws.numel(), C, N, T)
    return dict(status=status, fault=fault, dist=dist, flowtime_bound=extra[0], makespan_bound=extra[1], flowtime=extra[2],
                makespan=extra[3])


def certified(audit, w):
    """(C,) bool device tensor: the cases of an audit_schedules result whose schedule is valid and provably within the factor w
    of the optimal flowtime - status == 0 and flowtime_bound >= 0 and flowtime <= w * flowtime_bound, compared in float64 (a
    case with bound 0 and flowtime 0 is certified).  w < 1 raises ValueError.  No host synchronisation."""
    w = float(w)
    if not w >= 1.0:
        raise ValueError("certified: w must be at least 1, not %r" % (w,))
    bound = audit["flowtime_bound"]
    return (audit["status"] == 0) & (bound >= 0) & (audit["flowtime"].to(torch.float64) <= w * bound.to(torch.float64))


def certified_pack(res, audit, w):
    """solved_pack restricted to the cases certified(audit, w): the same keys, for expert_schedule / expert_samples (**pack).
    Raises ValueError when no case is left.  (Synchronises.)"""
    idx = torch.nonzero(certified(audit, w)).flatten()
    if idx.numel() == 0:
        raise ValueError("certified_pack: no case of the batch is certified at w = %r" % (w,))
    pack = {key: res[key].index_select(0, idx) for key in PACK_KEYS}
    pack["T"] = int(pack["makespan"].max().item()) + 1
    return pack


def _tree_search(entry, cases, T, ws_args, tail):
    """One launch of a tree search - `entry`, with its workspace sized by entry_workspace_bytes(*ws_args) - over `cases`
    (sh.dev_cases' tuple) with horizon T; tail: the entry's integers behind T.  Returns cbs_cases' dict."""
    m, batched, start, goal, C, N, H, W = cases
    dev = start.device
    paths = torch.empty(C, N, T, 2, dtype=torch.int32, device=dev)
    lengths = torch.empty(C, N, dtype=torch.int32, device=dev)
    solved = torch.empty(C, dtype=torch.uint8, device=dev)
    extra = torch.empty(7, C, dtype=torch.int32, device=dev)
    ws = sh.scratch(getattr(nat.lib(), entry + "_workspace_bytes")(*ws_args), dev)
    sh.call(dev, entry, nat.ptr(m), batched, H, W, nat.ptr(start), nat.ptr(goal), nat.ptr(paths), nat.ptr(lengths), nat.ptr(extra[0]),
            nat.ptr(solved), nat.ptr(extra[1]), nat.ptr(extra[2]), nat.ptr(extra[3]), nat.ptr(extra[4]), nat.ptr(extra[5]),
            nat.ptr(extra[6]), nat.ptr(ws), ws.numel(), C, N, T, *tail)
    return dict(paths=paths, lengths=lengths, goal=goal, start=start, makespan=extra[0], solved=solved, status=extra[1],
                flowtime=extra[2], lower_bound=extra[3], nodes=extra[4], expanded=extra[5], horizon_hit=extra[6])


def cbs_cases(obstacle_map, start, goal, horizon=None, max_nodes=256):
    """One call of magat_sim_mapf_cbs: conflict-based search on every case, one wavefront per case, all nodes and searches in one
    launch (the rule is in include/magat_hip.h and DESIGN 4.11).  obstacle_map (H,W) or (C,H,W), start / goal (C,N,2) as in
    plan_prioritized; horizon: the most cells a path may have (default default_horizon(H, W, N)); max_nodes: the budget of tree
    nodes per case, 1..4096.  Returns a dict of device tensors in plan_prioritized's layout - paths (C,N,horizon,2) int32 padded
    with each path's last cell, lengths (C,N), goal, start, makespan (C,), solved (C,) uint8 - so that solved_pack,
    audit_schedules and improve_schedules take it as it is, plus, all (C,) int32:
      status        0 solved: the schedule is optimal in the flowtime among schedules of at most `horizon` cells per path;
                    1 the budget ran out; 2 no schedule inside the horizon (or none at all); 3 a start or goal off the map, on an
                    obstacle or shared by two agents
      flowtime      sum(lengths - 1) for status 0, otherwise -1
      lower_bound   status 0: the flowtime; status 1: the cost of the node the search stopped at, the minimum over the open
                    list; status 2, 3: -1.  A bound of the optimal flowtime where horizon_hit == 0, otherwise of the optimum
                    over schedules of at most `horizon` cells per path
      nodes, expanded      tree nodes created (the root included) and nodes that got their two children
      horizon_hit   1 when a child was dropped because its agent had no arrival inside the horizon, else 0
    A case that is not solved gets every agent's start cell with length 1, as the planner's failing agents do.
    No focal search (that is ecbs_cases), and no pruning by an incumbent, disjoint splitting or conflict prioritisation either.
    Limits: H, W <= 64, horizon <= 256, N <= 4096 - anything else raises MagatNativeError; there is no wide form yet.
    Stream ordered, no host synchronisation."""
    cases = sh.dev_cases(obstacle_map, start, goal)
    C, N, H, W = cases[4:]
    T = default_horizon(H, W, N) if horizon is None else int(horizon)
    max_nodes = int(max_nodes)
    _limits("cbs_cases", H, W, T, N, max_nodes)
    return _tree_search("magat_sim_mapf_cbs", cases, T, (C, N, T, max_nodes), (max_nodes,))


def _w_milli(w, who):
    if not float(w) >= 1.0:
        raise ValueError("%s: w must be at least 1, not %r" % (who, w))
    w_milli = int(round(1000.0 * float(w)))
    if w_milli > MAX_W_MILLI_ECBS:
        raise ValueError("%s: w must be at most %g, not %r" % (who, MAX_W_MILLI_ECBS / 1000.0, w))
    return w_milli


def ecbs_cases(obstacle_map, start, goal, w=1.5, horizon=None, max_nodes=256, levels=4):
    """One call of magat_sim_mapf_ecbs: ECBS(w) - conflict-based search with a focal search on both levels - on every case, one
    wavefront per case, all nodes and searches in one launch (the rule is in include/magat_hip.h and DESIGN 4.11).  Arguments as
    cbs_cases, plus w >= 1, the suboptimality factor (handed to the device as round(1000 w); every comparison is integer
    arithmetic), and levels, 1..4: the planes of the low-level focal search - the last one is the planner's own search, plane k
    below it holds the cells reached with at most k steps that break another agent's reservation; levels=1 leaves the focal
    choice to the high level alone.  Returns cbs_cases' dict, the same keys with the same meanings, except
      status 0      the schedule is valid and flowtime <= w * lower_bound <= w * optimum (1000 * flowtime <= w_milli *
                    lower_bound on the device) - it is not proven optimal unless w == 1
      lower_bound   status 0 and 1: the smallest bound over the open list, a lower bound of the optimal flowtime under
                    cbs_cases' horizon caveat; status 2, 3: -1
    so solved_pack, audit_schedules and improve_schedules take it as it is.
    Limits: H, W <= 64, horizon <= 256, N <= 4096, max_nodes and levels as above - anything else raises MagatNativeError, a w
    below 1 or above 1048.576 ValueError; the wide form is ecbs_cases_wide.  Stream ordered, no host synchronisation."""
    w_milli = _w_milli(w, "ecbs_cases")
    cases = sh.dev_cases(obstacle_map, start, goal)
    C, N, H, W = cases[4:]
    T = default_horizon(H, W, N) if horizon is None else int(horizon)
    max_nodes, levels = int(max_nodes), int(levels)
    _limits("ecbs_cases", H, W, T, N, max_nodes, levels)
    return _tree_search("magat_sim_mapf_ecbs", cases, T, (C, N, T, max_nodes, levels), (max_nodes, w_milli, levels))


def ecbs_cases_wide(obstacle_map, start, goal, w=1.5, horizon=None, max_nodes=256, levels=4):
    """ecbs_cases on maps up to 256 x 256 with horizons up to 1024: the same arguments, the same rule cell for cell and node for
    node, the same dict - so solved_pack, audit_schedules(wide=True), improve_schedules(wide=True) and expert_samples(wide=True)
    take it as it is.  horizon defaults to default_horizon(H, W, N, wide=True).  By plan_prioritized's rule a shape with H, W <= 64
    and horizon <= 256 goes to magat_sim_mapf_ecbs and gives ecbs_cases' bits; a larger one goes to magat_sim_mapf_ecbs_wide
    (csrc/sim_mapf_ecbs_wide.hip): one workgroup of rows = 64 ceil(H / 64) threads per case, words = 1, 2 or 4 64-bit words >= W / 64
    per row, and a workspace of
      8 * (horizon * rows * words * (10 + levels) + ceil(N * horizon / 4) + ceil(max_nodes * horizon / 4) + 4 * max_nodes
           + ceil(5 * N / 2) + H * W) bytes per case
    - 10.6 MB at 65 x 65 / 100 agents / horizon 360, 91 MB at 160 x 160 / 1000 agents / horizon 1024, with 256 nodes and 4 levels.
    The search is sequential in the tree and in the steps of a flood: one run on one MI355X took 54 ms for 32 such 65 x 65 cases
    and 4.6 s for 4 such 160 x 160 cases, which all ended at the node budget (tools/mapf_bench.py, the _ecbs_wide rows).  w = 1 gives the optimal flowtime, as cbs_cases would.
    Limits: H, W <= 256, horizon <= 1024, N <= 4096, max_nodes 1..4096, levels 1..4 - anything else raises MagatNativeError with a
    message that names them, a w below 1 or above 1048.576 ValueError, CPU tensors MagatNativeError.
    Stream ordered, no host synchronisation; one launch."""
    w_milli = _w_milli(w, "ecbs_cases_wide")
    m, batched, start, goal, C, N, H, W = cases = sh.dev_cases(obstacle_map, start, goal)
    T = default_horizon(H, W, N, wide=True) if horizon is None else int(horizon)
    max_nodes, levels = int(max_nodes), int(levels)
    _limits("ecbs_cases_wide", H, W, T, N, max_nodes, levels, wide=True)
    if _route(H, W, T, True) == "narrow":
        return ecbs_cases(m, start, goal, w=w, horizon=T, max_nodes=max_nodes, levels=levels)
    return _tree_search("magat_sim_mapf_ecbs_wide", cases, T, (C, H, W, N, T, max_nodes, levels), (max_nodes, w_milli, levels))


# the flag an adoption adds -> (the prefix of its other keys, whether a solved case is replaced only by a smaller flowtime)
_ADOPTION = {"optimal": ("cbs_", False), "bounded": ("ecbs_", True)}


def _adopt(res, sub, flag):
    """A tree search's schedules put into a result - solve_cases(optimal=) with flag "optimal", solve_cases(bounded=) and
    adopt_bounded with "bounded".  Where sub["status"] == 0 (and, by the flag's rule, the case in `res` is unsolved or has a larger
    flowtime) sub's paths, lengths and makespan replace the case's, solved becomes 1 and failed_agent -1 (where `res` has that
    key).  Returns a new dict with every key of `res` but `T`, plus <prefix>status, <prefix>bound (sub's lower_bound where
    horizon_hit == 0, else -1), <prefix>nodes and the flag, (C,) bool: status 0.  Tensor ops only."""
    prefix, only_better = _ADOPTION[flag]
    done = sub["status"] == 0
    take = done & ((res["solved"] == 0) | ((res["lengths"] - 1).sum(1) > sub["flowtime"])) if only_better else done
    out = {key: value for key, value in res.items() if key != "T"}
    out.update(paths=torch.where(take[:, None, None, None], sub["paths"], res["paths"]),
               lengths=torch.where(take[:, None], sub["lengths"], res["lengths"]),
               makespan=torch.where(take, sub["makespan"], res["makespan"]),
               solved=torch.where(take, torch.ones_like(res["solved"]), res["solved"]))
    if "failed_agent" in res:
        out["failed_agent"] = torch.where(take, torch.full_like(res["failed_agent"], -1), res["failed_agent"])
    bound = torch.where(sub["horizon_hit"] == 0, sub["lower_bound"], torch.full_like(sub["lower_bound"], -1))
    out.update({prefix + "status": sub["status"], prefix + "bound": bound, prefix + "nodes": sub["nodes"], flag: done})
    return out


def adopt_bounded(res, sub):
    """solve_cases(bounded=)'s replacement rule as a function: `res` a plan_prioritized / solve_cases / improve_schedules result,
    `sub` an ecbs_cases / ecbs_cases_wide result on the same cases with the same horizon (otherwise ValueError).  Where
    sub["status"] == 0 AND the case in `res` is unsolved or has a larger flowtime, sub's paths, lengths and makespan replace the
    case's, solved becomes 1 and failed_agent -1 (where `res` has that key).  Returns a NEW dict with every key of `res` but `T`
    (solved_pack computes it), plus ecbs_status, ecbs_bound (sub's lower_bound where horizon_hit == 0, else -1), ecbs_nodes (C,) int32
    and bounded (C,) bool (status 0: flowtime <= w * ecbs_bound holds for the case's schedule).  For `certified`, take the audit's
    flowtime_bound to torch.maximum(audit["flowtime_bound"], res["ecbs_bound"]).  Tensor ops only: no launch of the package's own,
    no host synchronisation; neither input is modified."""
    if tuple(res["paths"].shape) != tuple(sub["paths"].shape):
        raise ValueError("adopt_bounded: res and sub must hold the same cases with the same horizon, not paths of %s and %s"
                         % (tuple(res["paths"].shape), tuple(sub["paths"].shape)))
    return _adopt(res, sub, "bounded")


def solve_cases(obstacle_map, start, goal, horizon=None, retries=8, wide=False, improve=0, optimal=None, bounded=None, bounded_nodes=256,
                certify=None):
    """plan_prioritized in index order, then up to `retries` re-plans of the cases still unsolved, each with that case's
    failed_agent moved to the front of its order.  Returns plan_prioritized's dict (every case holds its LAST plan) plus order
    (C,N) int32 (the order of that plan), rounds (C,) int32 (the plans made for the case, 1 = solved at once) and T =
    int(makespan.max()) + 1 over the solved cases (1 when there is none).

    Cases still unsolved STAY in the batch with solved == 0, and their paths are not schedules: expert_samples, expert_stats
    and BatchedEpisode replays must only be fed solved cases.  solved_pack(res) drops the others -
    idx = res["solved"].nonzero().flatten(); tensor.index_select(0, idx) for every tensor of the dict - and returns exactly
    the keys that expert_samples takes as **pack.

    wide: as in plan_prioritized, for the first plan and every re-plan.
    improve=I > 0: improve_schedules(obstacle_map, res, iterations=I, wide=wide) on the final batch (its limits apply; `wide` is
    handed on, so a wide batch is improved by the wide form) - the returned dict
    then also holds flowtime_before, flowtime_after, accepted and status, and T is taken from the improved makespans.  The
    default 0 leaves the result and the calls made as they were.
    optimal=K (1..4096): cbs_cases(obstacle_map, start, goal, horizon=T, max_nodes=K) on the whole batch, behind the last plan and
    behind `improve`, before `certify`'s audit.  Where it ends with status 0 its paths, lengths and makespan replace the case's and
    solved becomes 1 (failed_agent -1); every other case stays as it was.  The returned dict then also holds cbs_status, cbs_bound (the search's
    lower_bound where horizon_hit == 0, else -1), cbs_nodes (C,) int32 and optimal (C,) bool.  With certify=w as well, certified is
    taken against max(the audit's flowtime_bound, cbs_bound), and flowtime_bound in the result is that maximum.  Tensor ops only,
    no added synchronisation; cbs_cases' limits apply (no wide form).  The default None leaves the result and the calls made as
    they were.  (It stands in front of `certify` in the signature, as in the pipeline.)
    bounded=w (a number >= 1; not together with `optimal`: ValueError): ecbs_cases(obstacle_map, start, goal, w, horizon=T,
    max_nodes=bounded_nodes) where `optimal` would run cbs_cases.  Where it ends with status 0 AND the case's plan is unsolved or
    has a larger flowtime, its paths, lengths and makespan replace the case's and solved becomes 1 (failed_agent -1).  The returned
    dict then also holds ecbs_status, ecbs_bound (the search's lower_bound where horizon_hit == 0, else -1), ecbs_nodes (C,) int32
    and bounded (C,) bool (status 0: flowtime <= w * ecbs_bound holds for the case's schedule).  With certify as well,
    flowtime_bound = max(the audit's bound, ecbs_bound).  ecbs_cases' limits apply and are checked before anything is planned.
    The default None leaves the result and the calls made as they were.
    certify=w (a number >= 1): audit_schedules(obstacle_map, res, wide=wide) on the final batch, behind the last plan and
    behind `improve` - the returned dict then also holds the audit's keys (status, fault, dist, flowtime_bound, makespan_bound,
    flowtime; the audit's makespan equals the result's where status is 0 and is not copied) and certified = certified(audit, w),
    (C,) bool; it adds no host synchronisation.  With improve > 0 as well, `status` is the AUDIT's (the improver's is 0 on every
    solved case the audit calls valid).  The default None leaves the result and the calls made as they were.
    One host synchronisation per round (the read of `solved`), one more for T."""
    if certify is not None and not float(certify) >= 1.0:
        raise ValueError("solve_cases: certify must be at least 1, not %r" % (certify,))
    search = None      # the search behind the plan, as _limits takes it: (who, max_nodes, levels)
    if bounded is not None:
        if optimal is not None:
            raise ValueError("solve_cases: bounded and optimal exclude each other")
        _w_milli(bounded, "solve_cases(bounded=)")
        search = ("ecbs_cases", int(bounded_nodes), MAX_LEVELS_ECBS)
    elif optimal is not None:
        search = ("cbs_cases", int(optimal), None)
    if search is not None and isinstance(obstacle_map, torch.Tensor) and obstacle_map.dim() >= 2 and getattr(start, "ndim", 0) == 3:
        H, W, N = obstacle_map.shape[-2], obstacle_map.shape[-1], start.shape[1]      # refused before anything is planned
        _limits(search[0], H, W, default_horizon(H, W, N, wide) if horizon is None else int(horizon), N, *search[1:])
    res = plan_prioritized(obstacle_map, start, goal, None, horizon, wide)
    C, N, _ = res["start"].shape
    dev = res["start"].device
    order = torch.arange(N, dtype=torch.int32, device=dev).repeat(C, 1)
    rounds = torch.ones(C, dtype=torch.int32, device=dev)
    T = res["paths"].shape[2]
    batched = obstacle_map.dim() == 3
    for _ in range(int(retries)):
        idx = torch.nonzero(res["solved"] == 0).flatten()      # (the host learns how many are left: the synchronisation)
        if idx.numel() == 0:
            break
        again = promote(order.index_select(0, idx), res["failed_agent"].index_select(0, idx))
        sub = plan_prioritized(obstacle_map.index_select(0, idx) if batched else obstacle_map,
                               res["start"].index_select(0, idx), res["goal"].index_select(0, idx), again, T, wide)
        for key in ("paths", "lengths", "makespan", "solved", "failed_agent"):
            res[key].index_copy_(0, idx, sub[key])
        order.index_copy_(0, idx, again)
        rounds.index_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))
    if int(improve) > 0:
        res = improve_schedules(obstacle_map, res, iterations=int(improve), wide=wide)
    cbs_bound = None
    if optimal is not None:
        res = _adopt(res, cbs_cases(obstacle_map, res["start"], res["goal"], horizon=T, max_nodes=int(optimal)), "optimal")
        cbs_bound = res["cbs_bound"]
    if bounded is not None:
        res = _adopt(res, ecbs_cases(obstacle_map, res["start"], res["goal"], w=bounded, horizon=T, max_nodes=int(bounded_nodes)),
                     "bounded")
        cbs_bound = res["ecbs_bound"]
    if certify is not None:
        audit = audit_schedules(obstacle_map, res, wide=wide)
        if cbs_bound is not None:
            audit["flowtime_bound"] = torch.maximum(audit["flowtime_bound"], cbs_bound)
        res.update({key: audit[key] for key in AUDIT_KEYS if key != "makespan"}, certified=certified(audit, certify))
    done = res["makespan"][res["solved"] != 0]
    res.update(order=order, rounds=rounds, T=int(done.max().item()) + 1 if done.numel() else 1)
    return res


def pack_cases(res):
    """Indices (K,) int64 of the solved cases of a plan_prioritized / solve_cases result."""
    return torch.nonzero(res["solved"] != 0).flatten()


def solved_pack(res):
    """The solved cases of a result in pack_schedules' form - paths, lengths, goal, start, makespan and T = max(makespan) + 1
    - for expert_schedule / expert_samples (**pack).  Raises ValueError when no case is solved.  (Synchronises.)"""
    idx = pack_cases(res)
    if idx.numel() == 0:
        raise ValueError("solved_pack: no case of the batch is solved")
    pack = {key: res[key].index_select(0, idx) for key in PACK_KEYS}
    pack["T"] = int(pack["makespan"].max().item()) + 1
    return pack
