"""Closed-loop evaluation on the device: the reference's validation / test run
(agents/decentralplannerlocal_OnlineExpert_GAT.py:859-957 with utils/metrics.py: MonitoringMultiAgentPerformance) over a whole
set of cases, without a batch that waits for its slowest case.

    results = evaluate_cases(net, maps, start, goal, maxstep, slots=256, comm_radius=config.commR)
    summary = summarize_rollouts(results, stats["makespan"], stats["flowtime"])        # expert_stats' targets

An EpisodePool has B slots over a queue of C cases.  Every case has its own step limit (reference_maxstep: the reference's
int(makespanTarget * rate)); a slot whose episode is over writes its case's result row and takes the next case, on the device, in
the step() that ends the episode.  The host only asks finished() now and then.  HIP only (csrc/sim_pool.hip and the move step of
csrc/sim_frontend.hip): CPU tensors raise MagatNativeError."""
import ctypes

import numpy as np
import torch

from . import _native as nat
from . import _sim_host as sh
from .edges import GraphEdges
from .simulator import GUIDANCE_MODES, POLICIES, batched_fov_states, batched_gso, move_needs_wide, new_agent_view

RADIUS_MAX_STEPS = 64           # batched_connect_radius' growth limit


def reference_maxstep(makespanTarget, N, rate_maxstep):
    """multiRobotSimNew.setup's step limit (utils/new_simulator.py:204-210): int(makespanTarget * rate), rate 3 from 20 agents and
    config.rate_maxstep below - a float64 product, truncated.  makespanTarget: a number or an array / tensor of them; returns an
    int or a numpy int32 array."""
    rate = 3 if int(N) >= 20 else rate_maxstep
    if isinstance(makespanTarget, torch.Tensor):
        makespanTarget = makespanTarget.cpu().numpy()
    mk = np.asarray(makespanTarget).astype(np.int32)      # the reference: makespanTarget.type(torch.int32)
    out = np.trunc(mk.astype(np.float64) * np.float64(rate)).astype(np.int32)
    return int(out) if out.ndim == 0 else out


class EpisodePool:
    """`slots` episodes stepped together over a queue of C cases, all state on the device.

    obstacle_map (H,W) or (C,H,W); start / goal (C,N,2); maxstep an int or a (C,) int32 tensor, every value >= 1;
    1 <= slots <= C.  first_step=1 is the agent's loop (currentStep = step + 1; the call at currentStep == maxstep finalises),
    first_step=0 numbers the calls from 0 like BatchedEpisode.  The slot tensors have BatchedEpisode's names and types - pos, goal,
    map, reach_goal, first_move, end_step, actions, moves, flags, radii - plus slot_case and slot_step (B,) int32: the case a slot
    holds (-1: none left, the slot idles on its last positions) and the step number its next call gets.

        x = pool.states(); S = pool.gso(); pool.step(logits=...)      # no host synchronisation, no allocation: capturable
        pool.finished()                                               # the one read-back
        pool.results()

    The multinomial policies draw from magat_sim_pool_uniforms - a function of (seed, case, step, agent), so a case's episode
    does not depend on the slot it lands in or on `slots` - unless step() is given uniforms.  record=True keeps every case's
    trajectory (trajectory_pack)."""

    def __init__(self, obstacle_map, start, goal, maxstep, slots, comm_radius, action_select="soft_max", symmetric_norm=False,
                 FOV=9, guidance="Project_G", wide=False, seed=0, first_step=1, record=False):
        if action_select not in POLICIES:
            raise ValueError("action_select must be one of %s" % sorted(POLICIES))
        if guidance not in GUIDANCE_MODES:
            raise ValueError("guidance must be one of %s, got %r" % (sorted(GUIDANCE_MODES), guidance))
        if not isinstance(start, torch.Tensor) or start.dim() != 3 or start.shape[2] != 2:
            raise ValueError("start must be a (C,N,2) tensor")
        if not 1 <= int(slots) <= start.shape[0]:
            raise ValueError("slots must be in 1 .. %d (the number of cases), got %d" % (start.shape[0], int(slots)))
        if not isinstance(maxstep, torch.Tensor) and int(maxstep) < 1:
            raise ValueError("every maxstep must be >= 1, got %d" % int(maxstep))
        self.q_map, batched, self.q_start, self.q_goal, C, N, H, W = sh.dev_cases(obstacle_map, start, goal)
        dev = self.q_start.device
        B = int(slots)
        if not 1 <= B <= C:
            raise ValueError("slots must be in 1 .. %d (the number of cases), got %d" % (C, B))
        if isinstance(maxstep, torch.Tensor):
            if not maxstep.is_cuda:
                raise nat.MagatNativeError("maxstep must be an int or a device tensor (no CPU fallback)")
            self.q_maxstep = maxstep.to(torch.int32).contiguous().reshape(-1)
            if self.q_maxstep.numel() != C:
                raise ValueError("maxstep must hold one limit per case (%d), got %d" % (C, self.q_maxstep.numel()))
            lo, hi = (int(v) for v in torch.stack([self.q_maxstep.min(), self.q_maxstep.max()]).tolist())      # the one read
        else:
            lo = hi = int(maxstep)
            self.q_maxstep = torch.full((C,), lo, dtype=torch.int32, device=dev)
        if lo < 1:
            raise ValueError("every maxstep must be >= 1, got %d" % lo)
        if int(first_step) not in (0, 1):
            raise ValueError("first_step must be 0 or 1")
        if record and (H > 256 or W > 256):
            raise nat.MagatNativeError("record=True takes maps up to 256 x 256 (a cell is row << 8 | col)")
        self.C, self.B, self.N, self.H, self.W, self.dev = C, B, N, H, W, dev
        self.max_maxstep, self.first_step, self.record = hi, int(first_step), bool(record)
        self.policy = POLICIES[action_select]
        self.comm_radius, self.symmetric_norm, self.FOV = float(comm_radius), bool(symmetric_norm), int(FOV)
        self.guidance, self.wide, self.seed = guidance, bool(wide), int(seed) & 0xFFFFFFFFFFFFFFFF
        self._guide_ws = sh._Workspace()
        self._edges = self._valued_edges = None
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)      # noqa: E731
        self.pos, self.goal = i32(B, N, 2), i32(B, N, 2)
        self.map = torch.zeros(B, H, W, dtype=torch.uint8, device=dev) if batched else self.q_map
        self.reach_goal = torch.zeros(B, N, dtype=torch.uint8, device=dev)
        self.first_move, self.end_step, self.actions = i32(B, N), i32(B, N), i32(B, N)
        self.moves = torch.zeros(B, N, 2, dtype=torch.int8, device=dev)
        self.flags, self.done, self.flowtime, self.makespan = i32(B), i32(B), i32(B), i32(B)
        self.radii = torch.zeros(B, dtype=torch.float64, device=dev)
        self.slot_case = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.slot_step, self.slot_maxstep, self.over, self.sticky = i32(B), i32(B), i32(B), i32(B)
        self.counters = torch.tensor([0, C, 0, 0], dtype=torch.int32, device=dev)      # next, remaining, the turn's hand-over
        self.agent_view = None
        if guidance.startswith("SemiLG"):
            self.agent_view = new_agent_view(B, N, H, W, self.FOV, dev)
        self._rows = i32(len(nat.POOL_COLUMNS), C)
        self._radius = torch.zeros(C, dtype=torch.float64, device=dev)
        self._end_pos, self._first_move, self._end_step = i32(C, N, 2), i32(C, N), i32(C, N)
        self.traj_cells = max(hi - self.first_step + 1, 1)
        self._traj = torch.zeros(C, N, self.traj_cells, dtype=torch.int16, device=dev) if record else None
        self._traj_len = i32(C) if record else None
        self._uniforms = torch.zeros(B, N, dtype=torch.float64, device=dev)
        self._to_wide = self.wide and move_needs_wide(H, W, N)
        self._move_ws = sh.scratch(nat.lib().magat_sim_move_wide_workspace_bytes(B, H, W, N), dev) if self._to_wide else None
        d = nat.SimPoolDesc()
        d.q_map, d.q_start, d.q_goal, d.q_maxstep = (t.data_ptr() for t in (self.q_map, self.q_start, self.q_goal, self.q_maxstep))
        d.map_batched, d.H, d.W, d.C, d.B, d.N = batched, H, W, C, B, N
        d.first_step, d.record, d.traj_cells, d.radius_max_steps = self.first_step, 1 if record else 0, self.traj_cells, RADIUS_MAX_STEPS
        d.comm_radius = self.comm_radius
        d.slot_case, d.slot_step, d.slot_maxstep = self.slot_case.data_ptr(), self.slot_step.data_ptr(), self.slot_maxstep.data_ptr()
        d.over, d.sticky = self.over.data_ptr(), self.sticky.data_ptr()
        d.map = self.map.data_ptr() if batched else None
        d.pos, d.goal, d.reach_goal = self.pos.data_ptr(), self.goal.data_ptr(), self.reach_goal.data_ptr()
        d.first_move, d.end_step = self.first_move.data_ptr(), self.end_step.data_ptr()
        d.done, d.flowtime, d.makespan = self.done.data_ptr(), self.flowtime.data_ptr(), self.makespan.data_ptr()
        d.radii = self.radii.data_ptr()
        if self.agent_view is not None:
            d.agent_view, d.agent_view_bytes = self.agent_view.data_ptr(), self.agent_view[0].numel()
        d.counters, d.rows, d.r_radius = self.counters.data_ptr(), self._rows.data_ptr(), self._radius.data_ptr()
        d.r_end_pos, d.r_first_move, d.r_end_step = self._end_pos.data_ptr(), self._first_move.data_ptr(), self._end_step.data_ptr()
        if record:
            d.traj, d.traj_len = self._traj.data_ptr(), self._traj_len.data_ptr()
        self._desc = d
        s = nat.SimStepDesc()
        s.map, s.map_batched, s.H, s.W, s.B, s.N = self.map.data_ptr(), d.map_batched, H, W, B, N
        s.pos, s.goal, s.reach_goal = d.pos, d.goal, d.reach_goal
        s.first_move, s.end_step = d.first_move, d.end_step
        s.actions_out, s.moves_out, s.flags_out = self.actions.data_ptr(), self.moves.data_ptr(), self.flags.data_ptr()
        s.done_out, s.flowtime_out, s.makespan_out = d.done, d.flowtime, d.makespan
        self._step_desc = s
        sh.call(dev, "magat_sim_pool_turn", ctypes.byref(d), 1)      # the first fill: every slot takes a case, radii included

    def gso(self, dtype=torch.float64):
        """getGSO for every slot, with the radius its case grew to at the refill."""
        return batched_gso(self.pos, self.radii, symmetric_norm=self.symmetric_norm, dtype=dtype)

    def edges(self, values=False):
        """gso()'s graph as a GraphEdges over the slots' own positions and radii, for DecentralPlannerGATNet.addGSO: one object
        per pool, refreshed by every call (BatchedEpisode.edges).  No host synchronisation here.  values=True: with gso()'s
        values under the pool's symmetric_norm, for the GNN planners' addGSO."""
        if values:
            if self._valued_edges is None:
                self._valued_edges = GraphEdges(self.pos, radii=self.radii, values=True, symmetric_norm=self.symmetric_norm)
            return self._valued_edges.refresh()
        if self._edges is None:
            self._edges = GraphEdges(self.pos, radii=self.radii)
        return self._edges.refresh()

    def states(self):
        return batched_fov_states(self.map, self.pos, self.goal, self.FOV, self.guidance, self.agent_view, self.wide,
                                  self._guide_ws)

    def step(self, logits=None, actions=None, uniforms=None):
        """move() for every slot that holds a case, then the turn: result rows and refills.  Returns nothing."""
        B, N, dev = self.B, self.N, self.dev
        lg, ac = sh.dev_actions(logits, actions, B, N)
        policy = self.policy if lg is not None else 0
        if policy and uniforms is None:
            uniforms = self._uniforms
            sh.call(dev, "magat_sim_pool_uniforms", nat.ptr(self.slot_case), nat.ptr(self.slot_step), nat.ptr(uniforms), self.seed, B, N)
        if uniforms is not None:
            uniforms = sh.dev_uniforms(uniforms, B, N)
        s = self._step_desc
        s.logits, s.actions_in = nat.ptr(lg), nat.ptr(ac)
        s.policy, s.uniforms = policy, nat.ptr(uniforms)
        sh.call(dev, "magat_sim_pool_step", ctypes.byref(s), nat.ptr(self.slot_case), nat.ptr(self.slot_step), nat.ptr(self.slot_maxstep),
                nat.ptr(self.over), nat.ptr(self.sticky), ws=self._move_ws)
        sh.call(dev, "magat_sim_pool_turn", ctypes.byref(self._desc), 0)

    def finished(self):
        """True once every case is retired (reads one word back: synchronises)."""
        return int(self.counters[1].item()) == 0

    def max_calls(self):
        """A bound on the step() calls until finished(): every slot serves at most ceil(C / B) cases, a case at most
        max(maxstep) - first_step + 1 calls."""
        return -(-self.C // self.B) * (self.max_maxstep - self.first_step + 1)

    def results(self):
        """Per case, device tensors (views of the pool's own): retired, all_reach (all agents had arrived before the last call,
        as move() returns it), num_reach, steps (the currentStep at the break), makespan, flowtime, predicted_collision (sticky
        flag bits 0-3), flag_bits, status (bit 1: the communication graph was still disconnected at the radius growth limit) -
        (C,) int32; radius (C,) float64; end_pos (C,N,2), first_move, end_step (C,N) int32; and maxstep (C,), the limits the pool
        was given.  A row is valid once retired."""
        out = {name: self._rows[i] for i, name in enumerate(nat.POOL_COLUMNS)}
        out.update(radius=self._radius, end_pos=self._end_pos, first_move=self._first_move, end_step=self._end_step)
        out["maxstep"] = self.q_maxstep       # the cases' limits, for summarize_rollouts
        return out

    def trajectory_pack(self):
        """record=True: the trajectories in pack_schedules' layout, for audit_schedules - paths (C,N,T,2) int32 (a case's last
        cell repeated behind its end), lengths (C,N), start, goal := the last cell, solved := retired."""
        if not self.record:
            raise ValueError("trajectory_pack needs EpisodePool(record=True)")
        cells = self._traj.to(torch.int32) & 0xFFFF
        T = self.traj_cells
        length = self._traj_len.clamp(min=1)
        t = torch.arange(T, device=self.dev).view(1, 1, T).minimum((length - 1).view(-1, 1, 1).to(torch.int64))
        cells = cells.gather(2, t.expand(self.C, self.N, T))
        paths = torch.stack([cells >> 8, cells & 255], dim=-1).to(torch.int32).contiguous()
        return dict(paths=paths, lengths=length.view(-1, 1).expand(self.C, self.N).contiguous(), start=self.q_start,
                    goal=paths[:, :, -1].contiguous(), solved=self._rows[0].to(torch.uint8))


def evaluate_cases(net, obstacle_map, start, goal, maxstep, slots, comm_radius, poll=16, graph="gso", **pool_kw):
    """The validation / test run over a set of cases: every case rolled out in closed loop with `net` (addGSO + forward on the
    pool's states) until it ends, `slots` at a time; finished() is asked every `poll` steps.  Returns EpisodePool.results().
    graph: 'gso' hands the model the pool's GSO tensor; 'edges' its edge structure from the positions (EpisodePool.edges: the
    attention models, up to 4096 agents); 'valued_edges' that structure with the GSO's values on it (EpisodePool.edges(values=True):
    the GNN planners, up to 4096 agents)."""
    if graph not in ("gso", "edges", "valued_edges"):
        raise ValueError("graph must be 'gso', 'edges' or 'valued_edges', got %r" % (graph,))
    pool = EpisodePool(obstacle_map, start, goal, maxstep, slots, comm_radius, **pool_kw)
    the_graph = {"gso": pool.gso, "edges": pool.edges, "valued_edges": lambda: pool.edges(values=True)}[graph]
    poll = max(int(poll), 1)
    calls, bound = 0, pool.max_calls()
    with torch.no_grad():
        while True:
            for _ in range(poll):
                net.addGSO(the_graph())
                pool.step(logits=net(pool.states()))
            calls += poll
            if pool.finished():
                return pool.results()
            if calls > bound + poll:
                raise nat.MagatNativeError("evaluate_cases: cases left after %d steps (bound %d)" % (calls, bound))


def summarize_rollouts(results, makespanTarget, flowtimeTarget):
    """The reference's per-case log_result (mutliAgent_ActionPolicy :918-957, without its two wall-clock entries) and the fields
    of MonitoringMultiAgentPerformance.summary (utils/metrics.py:113-207, 246-248) from EpisodePool.results() and the expert's
    targets (expert_stats).  One read-back, then numpy float64 on the host.  results may hold device tensors or arrays; a
    `maxstep` entry is needed ((C,) limits or one int): pass dict(results, maxstep=...)."""
    keys = ("all_reach", "num_reach", "steps", "makespan", "flowtime", "predicted_collision", "maxstep")
    if "maxstep" not in results:
        raise ValueError("summarize_rollouts: results needs a 'maxstep' entry (the cases' step limits)")
    vals = [results[k] for k in keys] + [makespanTarget, flowtimeTarget]
    if any(isinstance(v, torch.Tensor) for v in vals):
        dev = next(v.device for v in vals if isinstance(v, torch.Tensor))
        C = int(results["steps"].shape[0])
        cols = [torch.as_tensor(v, device=dev).to(torch.int64).reshape(-1).expand(C) for v in vals]
        vals = list(torch.stack(cols).cpu().numpy())      # the one read-back
    vals = [np.asarray(v).astype(np.int64).reshape(-1) for v in vals]
    all_reach, num_reach, steps, mk, ft, predicted, maxstep, mkT, ftT = vals
    C = len(steps)
    maxstep, mkT, ftT = (np.broadcast_to(v, (C,)) for v in (maxstep, mkT, ftT))
    all_reach, predicted = all_reach != 0, predicted != 0
    timeout = steps >= maxstep
    # checkOptimality(True) after an arrival, overruled by checkOptimality(False) once currentStep >= maxstep (:921-936)
    optimal = all_reach & ~timeout & (mk <= mkT) & (ft <= ftT)
    shield = timeout & ~all_reach & predicted
    rate_mp = np.abs(mk - mkT).astype(np.float64) / mkT.astype(np.float64)
    rate_ft = np.abs(ft - ftT).astype(np.float64) / ftT.astype(np.float64)
    N = int(np.asarray(results["end_pos"].shape)[1]) if "end_pos" in results else int(num_reach.max())
    std = lambda a: float(np.std(a, ddof=1)) if C > 1 else float("nan")      # noqa: E731
    return dict(
        allReachGoal=all_reach, noReachGoalbyCollisionShielding=shield, findOptimalSolution=optimal,
        check_collisionFreeSol=all_reach.copy(), check_CollisionPredictedinLoop=predicted,
        compare_makespan=np.stack([mk, mkT], axis=1), compare_flowtime=np.stack([ft, ftT], axis=1),
        num_agents_reachgoal=num_reach, rate_deltaMP=rate_mp, rate_deltaFT=rate_ft,
        count_validset=C, rateReachGoal=float(all_reach.sum()) / C, rateFailedReachGoalSH=float(shield.sum()) / C,
        ratefindOptimalSolution=float(optimal.sum()) / C, rateCollsionFreeSol=float(all_reach.sum()) / C,
        rateCollisionPredictedinLoop=float(predicted.sum()) / C,
        avg_rate_deltaMP=float(np.mean(rate_mp)), std_rate_deltaMP=std(rate_mp),
        avg_rate_deltaFT=float(np.mean(rate_ft)), std_rate_deltaFT=std(rate_ft),
        hist_numAgentReachGoal=np.bincount(num_reach, minlength=N + 1)[:N + 1].astype(np.int64))
