"""Batched on-device simulator front-end: what the reference does per instance, per
step, in numpy on the host right before the model call -

    multiRobotSimNew.getGSO / computeAdjacencyMatrix   (utils/new_simulator.py:301-321, 745-806)
    multiRobotSimNew.getCurrentState -> AgentState.toInputTensor, guidance 'Project_G'
                                                        (utils/new_simulator.py:279-296; dataloader/statetransformer_Guidance.py:136-239)

- for B independent planning instances at once, on the GPU, so that a batched closed loop never leaves the device:

    S = batched_gso(pos, config.commR)                   # (B,N,N), what model.addGSO() takes
    E = batched_edges(pos, config.commR)                 # the same graph as an edge structure (edges.py): what the attention
                                                         # models' addGSO() takes as well - no (B,N,N) tensor, up to 4096 agents
    x = batched_fov_states(obstacle_map, pos, goal, 9)   # (B,N,3,11,11), what model.forward() takes
    x = batched_fov_states(obstacle_map, pos, goal, 9, guidance="GlobalG_SD")      # config.guidance: the A*-guided encodings

and the step behind it (multiRobotSimNew.move, :471-549) with the episode state on the device:

    ep = BatchedEpisode(obstacle_map, pos, goal, maxstep, comm_radius=config.commR, action_select='exp_multinorm')
    S = ep.gso(); x = ep.states(); done = ep.step(logits)        # radius grown at step 0 like the reference

HIP only (csrc/sim_frontend.hip, csrc/sim_guidance.hip): CPU tensors raise MagatNativeError."""
import ctypes

import torch

from . import _native as nat
from . import _sim_host as sh
from ._sim_host import _Workspace, dev_i32 as _dev_i32      # noqa: F401  (the names other modules and tools import from here)
from .edges import GraphEdges, batched_edges                # noqa: F401  (the graph as edges from positions: edges.py)


def batched_connect_radius(pos, comm_radius, max_steps=64, return_steps=False):
    """Step-0 branch of computeAdjacencyMatrix (utils/new_simulator.py:759-768) for B instances: r = R / 1.1, then
    r *= 1.1 until the graph (distance < r) is connected.  Returns radii (B,) float64 on the device (bit-equal to the
    reference's), to be passed to batched_gso for the rest of the episode."""
    pos = _dev_i32(pos, "pos")
    assert pos.dim() == 3 and pos.shape[2] == 2, "pos must be (B,N,2)"
    B, N, _ = pos.shape
    radii = torch.empty(B, dtype=torch.float64, device=pos.device)
    steps = torch.empty(B, dtype=torch.int32, device=pos.device)
    sh.call(pos.device, "magat_sim_connect_radius", nat.ptr(pos), float(comm_radius), nat.ptr(radii), nat.ptr(steps), B, N,
            int(max_steps))
    return (radii, steps) if return_steps else radii


def batched_gso(pos, comm_radius, symmetric_norm=False, normalize=True, dtype=torch.float64, return_lambda=False):
    """pos (B,N,2) integer agent coordinates (row, col) on the device -> S (B,N,N) `dtype` (float64 like the simulator
    hands it over, or float32 like the dataloader).  `comm_radius`: one number, or a (B,) float64 device tensor of
    per-instance radii (batched_connect_radius: the radius each instance grew to at step 0)."""
    pos = _dev_i32(pos, "pos")
    assert pos.dim() == 3 and pos.shape[2] == 2, "pos must be (B,N,2)"
    if dtype not in (torch.float32, torch.float64):      # (the kernels write 4- or 8-byte entries: nothing else fits S)
        raise TypeError("batched_gso: dtype must be torch.float32 or torch.float64, got %s" % (dtype,))
    if isinstance(comm_radius, torch.Tensor):
        B, N, _ = pos.shape
        if not comm_radius.is_cuda or comm_radius.dtype != torch.float64 or comm_radius.numel() != B:
            raise nat.MagatNativeError("per-instance radii must be a (B,) float64 device tensor")
        radii = comm_radius.contiguous()
        S = torch.empty(B, N, N, dtype=dtype, device=pos.device)
        lam = torch.empty(B, dtype=torch.float64, device=pos.device)
        sh.call(pos.device, "magat_sim_gso_radii", nat.ptr(pos), nat.ptr(radii), 1 if symmetric_norm else 0, 1 if normalize else 0,
                nat.ptr(S), int(dtype == torch.float64), nat.ptr(lam), B, N)
        return (S, lam) if return_lambda else S
    B, N, _ = pos.shape
    S = torch.empty(B, N, N, dtype=dtype, device=pos.device)
    lam = torch.empty(B, dtype=torch.float64, device=pos.device)
    sh.call(pos.device, "magat_sim_gso", nat.ptr(pos), float(comm_radius), 1 if symmetric_norm else 0, 1 if normalize else 0,
            nat.ptr(S), int(dtype == torch.float64), nat.ptr(lam), B, N)
    return (S, lam) if return_lambda else S


# config.guidance -> (MAGAT_GUIDE_* mode, dynamic obstacles); 'Project_G' is magat_sim_fov_states
GUIDANCE_MODES = {"Project_G": None,
                  "LocalG_S": (nat.GUIDE_LOCAL, 0), "LocalG_SD": (nat.GUIDE_LOCAL, 1),
                  "GlobalG_S": (nat.GUIDE_GLOBAL, 0), "GlobalG_SD": (nat.GUIDE_GLOBAL, 1),
                  "SemiLG_S": (nat.GUIDE_SEMI, 0), "SemiLG_SD": (nat.GUIDE_SEMI, 1)}


def new_agent_view(B, N, H, W, FOV=9, device="cuda"):
    """The per-agent map memory of guidance 'SemiLG_*' at the start of an episode (AgentState.setmap: all unknown = free):
    (B, N, H + 2 (FOV // 2), W + 2 (FOV // 2)) uint8 zeros.  batched_fov_states updates it in place."""
    half = int(FOV) // 2
    return torch.zeros(B, N, H + 2 * half, W + 2 * half, dtype=torch.uint8, device=device)


GUIDE_CANVAS = 64               # csrc/sim_guidance.hip: the narrow form's search canvas, H + 2 (FOV // 2) + 2 rows at most
MOVE_LDS_BYTES = 160 * 1024     # csrc/sim_frontend.hip: the narrow move step keeps 4 H W + 16 N bytes in LDS


_guide_workspaces = {}          # device -> _Workspace, for batched_fov_states calls that bring none


def _guide_workspace(workspace, B, N, H, W, FOV, device):
    """The open lists of magat_sim_guided_states_wide / magat_sim_replayed_states_wide: in `workspace`, or in the device's own"""
    if workspace is None:
        workspace = _guide_workspaces.setdefault(device, _Workspace())
    return workspace.get(nat.lib().magat_sim_guided_states_wide_workspace_bytes(B, N, H, W, FOV), device)


def guided_needs_wide(H, W, FOV):
    """True where GlobalG_* / SemiLG_* on an H x W map is beyond the narrow kernel's 64 x 64 canvas."""
    return max(H, W) + 2 * (int(FOV) // 2) + 2 > GUIDE_CANVAS


def guided_wide_geometry(B, N, H, W, FOV=9):
    """(workgroups, agents the busiest workgroup walks) of magat_sim_guided_states_wide, from the library's own workspace
    size: one slab of canvas rows * canvas columns * 8 bytes per workgroup."""
    half = int(FOV) // 2
    slab = (H + 2 * half + 2) * (W + 2 * half + 2) * 8
    groups = int(nat.lib().magat_sim_guided_states_wide_workspace_bytes(B, N, H, W, int(FOV))) // slab
    return groups, (-(-(B * N) // groups) if groups else 0)


def move_needs_wide(H, W, N):
    """True where the narrow move step's LDS limit refuses the shape."""
    return 4 * H * W + 16 * N > MOVE_LDS_BYTES


def batched_fov_states(obstacle_map, pos, goal, FOV=9, guidance="Project_G", agent_view=None, wide=False, workspace=None):
    """obstacle_map (H,W) or (B,H,W) uint8/bool device tensor (non-zero = obstacle), pos / goal (B,N,2) integer
    (row, col) -> x (B,N,3,FOV+2,FOV+2) float32, identical to stacking AgentState.toInputTensor over the instances.

    guidance = config.guidance of the reference: 'Project_G' (default: channel 1 is the goal or its projection onto the window's
    border), or the A*-guided encodings whose channel 1 is the reference's A* path, cell for cell (csrc/sim_guidance.hip, one
    launch): 'LocalG_S' / 'LocalG_SD' search the agent's own window, 'GlobalG_S' / 'GlobalG_SD' the whole padded map,
    'SemiLG_S' / 'SemiLG_SD' the map the agent has seen so far - `agent_view` (new_agent_view(...)), a caller-owned uint8
    tensor (B, N, H + 2 (FOV // 2), W + 2 (FOV // 2)) that the call updates IN PLACE.  '_SD' counts the agents inside the FOV
    as obstacles.  Without `wide`, GlobalG / SemiLG take maps up to 54 x 54 at FOV 9 (a 64 x 64 search canvas; larger maps
    raise MagatNativeError, nothing is launched).  wide=True lifts that to 256 x 256: a map the narrow kernel takes still goes
    to it, with the same bits; a larger one goes to magat_sim_guided_states_wide (csrc/sim_guidance_wide.hip, the same search
    with its open list in a device workspace - cached per device and grown only when it must, or `workspace`, a _Workspace the
    caller owns).  'Project_G' and 'LocalG_*' do not depend on the keyword.  The whole path is drawn: the reference itself
    raises IndexError once a path is longer than its max_localPath (4 (FOV + 2) cells for LocalG, rows + columns of the padded
    map otherwise)."""
    if guidance not in GUIDANCE_MODES:
        raise ValueError("guidance must be one of %s, got %r" % (sorted(GUIDANCE_MODES), guidance))
    pos, goal = _dev_i32(pos, "pos"), _dev_i32(goal, "goal")
    B, N, _ = pos.shape
    assert goal.shape == pos.shape
    m, batched, H, W = sh.dev_map(obstacle_map, B)
    guided = GUIDANCE_MODES[guidance]
    if guided is not None and guided[0] == nat.GUIDE_SEMI:
        half = int(FOV) // 2
        if agent_view is None:
            raise ValueError("guidance %r needs agent_view (new_agent_view(B, N, H, W, FOV))" % guidance)
        if (not isinstance(agent_view, torch.Tensor) or not agent_view.is_cuda or agent_view.dtype != torch.uint8
                or not agent_view.is_contiguous() or tuple(agent_view.shape) != (B, N, H + 2 * half, W + 2 * half)):
            raise nat.MagatNativeError("agent_view must be a contiguous uint8 device tensor of shape %s (it is updated in "
                                       "place)" % ((B, N, H + 2 * half, W + 2 * half),))
    x = torch.empty(B, N, 3, FOV + 2, FOV + 2, dtype=torch.float32, device=pos.device)
    if guided is None:
        sh.call(pos.device, "magat_sim_fov_states", nat.ptr(m), batched, H, W, nat.ptr(pos), nat.ptr(goal), nat.ptr(x), FOV, B, N)
        return x
    ws = None
    if wide and guided[0] != nat.GUIDE_LOCAL and guided_needs_wide(H, W, FOV):
        ws = _guide_workspace(workspace, B, N, H, W, FOV, pos.device)
    sh.call(pos.device, "magat_sim_guided_states", nat.ptr(m), batched, H, W, nat.ptr(pos), nat.ptr(goal), nat.ptr(x), FOV, B, N,
            guided[0], guided[1], nat.ptr(agent_view) if guided[0] == nat.GUIDE_SEMI else None, ws=ws)
    return x


def replayed_semi_states(obstacle_map, pos, goal, history, FOV=9, guidance="SemiLG_S", wide=False, workspace=None):
    """'SemiLG_*' states of ANY step of a known schedule, in one call and without an agent_view: the map each agent remembers
    is rebuilt on the device from the cells it has stood on (csrc/sim_guidance_parts.h: the maps are static, so that map is
    "seen so far AND blocked") - the tensors batched_fov_states gives when the case is stepped from its start with a carried
    agent_view.  obstacle_map (H,W) or (B,H,W), pos / goal (B,N,2): the rows' current cells and goals, as in batched_fov_states
    -> x (B,N,3,FOV+2,FOV+2) float32.  history: a dict with case, step - (B,) int32 device tensors: row b is step step[b] of
    case case[b] - and ONE source of the cells,
        table                  (cases,T,N,2) int32, expert_schedule's pos (T <= 1024), or
        cells, lengths, goal   ExpertMemory's store: (cases,N,Lcap) uint16 = row << 8 | col, (cases,N), (cases,N,2) int32 - cell s of
                               an agent is cells[s] while s < lengths, its goal behind that (expert_schedule's rule).
    A step whose cell is off the map, or an agent whose goal is, contributes nothing.  The refusals of batched_fov_states: CPU
    tensors, and without `wide` a map above 54 x 54 at FOV 9 (wide, workspace: its keywords).  One launch, no host
    synchronisation, no read-back; counted in form 'sim_replay'."""
    if guidance not in GUIDANCE_MODES or GUIDANCE_MODES[guidance] is None or GUIDANCE_MODES[guidance][0] != nat.GUIDE_SEMI:
        raise ValueError("replayed_semi_states: guidance must be 'SemiLG_S' or 'SemiLG_SD', got %r" % (guidance,))
    pos, goal = _dev_i32(pos, "pos"), _dev_i32(goal, "goal")
    B, N, _ = pos.shape
    assert goal.shape == pos.shape
    m, batched, H, W = sh.dev_map(obstacle_map, B)
    keys = set(history)
    if not {"case", "step"} <= keys or ("table" in keys) == bool(keys & {"cells", "lengths", "goal"}):
        raise ValueError("replayed_semi_states: history holds case, step and either table or cells, lengths, goal - not %s"
                         % sorted(keys))
    case, step = _dev_i32(history["case"], "history['case']"), _dev_i32(history["step"], "history['step']")
    if case.numel() != B or step.numel() != B:
        raise ValueError("replayed_semi_states: history's case and step must hold one entry per row (%d)" % B)
    d = nat.SimHistoryDesc()
    d.row_case, d.row_step = case.data_ptr(), step.data_ptr()
    if "table" in keys:
        table = _dev_i32(history["table"], "history['table']")
        if table.dim() != 4 or table.shape[2] != N or table.shape[3] != 2:
            raise ValueError("replayed_semi_states: history['table'] must be (cases,T,%d,2), not %s" % (N, tuple(table.shape)))
        d.pos_table, d.cases, d.T = table.data_ptr(), table.shape[0], table.shape[1]
    else:
        if not {"cells", "lengths", "goal"} <= keys:
            raise ValueError("replayed_semi_states: a store history holds cells, lengths and goal")
        cells = history["cells"]
        if (not isinstance(cells, torch.Tensor) or not cells.is_cuda or cells.dtype not in (torch.uint16, torch.int16)
                or cells.dim() != 3 or cells.shape[1] != N or not cells.is_contiguous()):
            raise nat.MagatNativeError("history['cells'] must be a contiguous (cases,%d,Lcap) uint16 device tensor" % N)
        lengths, hgoal = _dev_i32(history["lengths"], "history['lengths']"), _dev_i32(history["goal"], "history['goal']")
        cases = cells.shape[0]
        if tuple(lengths.shape) != (cases, N) or tuple(hgoal.shape) != (cases, N, 2):
            raise ValueError("replayed_semi_states: history's lengths and goal must be (%d,%d) and (%d,%d,2)" % (cases, N, cases, N))
        d.cells, d.lengths, d.goal = cells.data_ptr(), lengths.data_ptr(), hgoal.data_ptr()
        d.cases, d.Lcap = cases, cells.shape[2]
    x = torch.empty(B, N, 3, FOV + 2, FOV + 2, dtype=torch.float32, device=pos.device)
    ws = _guide_workspace(workspace, B, N, H, W, FOV, pos.device) if wide and guided_needs_wide(H, W, FOV) else None
    sh.call(pos.device, "magat_sim_replayed_states", nat.ptr(m), batched, H, W, nat.ptr(pos), nat.ptr(goal), nat.ptr(x), FOV, B, N,
            ctypes.byref(d), ws=ws)
    return x


def batched_move(obstacle_map, pos, logits=None, actions=None, goal=None, wide=False, workspace=None):
    """One closed-loop step for B instances on the device (multiRobotSimNew.move, utils/new_simulator.py:471-520):
    decode the action keys from the model's logits (B*N,5) (or take `actions` (B,N)), shield the proposed moves exactly
    like check_collision (:334-454; lowest index instead of random.choice among moving claimants) and advance `pos`
    IN PLACE.  Returns dict(actions (B,N) int32, moves (B,N,2) int8, reached (B,N) bool or None, flags (B,) int32).
    The cell grid lives in LDS, 4 H W + 16 N bytes <= 160 KB (about 200 x 200); wide=True takes maps up to 256 x 256 with up to
    4096 agents: a shape inside the LDS limit keeps its kernel, a larger one goes to magat_sim_move_wide, the same rules with the
    grid in a device workspace of 4 B H W bytes (`workspace`, a _Workspace the caller keeps, or a fresh buffer)."""
    m = sh.dev_u8(obstacle_map, "obstacle_map")
    if pos.dtype != torch.int32 or not pos.is_cuda or not pos.is_contiguous():
        raise nat.MagatNativeError("pos must be a contiguous int32 device tensor (it is updated in place)")
    B, N, _ = pos.shape
    dev = pos.device
    H, W = m.shape[-2], m.shape[-1]
    lg, ac = sh.dev_actions(logits, actions, B, N)
    gl = None if goal is None else _dev_i32(goal, "goal")
    a_out = torch.empty(B, N, dtype=torch.int32, device=dev)
    mv = torch.empty(B, N, 2, dtype=torch.int8, device=dev)
    reached = torch.empty(B, N, dtype=torch.uint8, device=dev) if gl is not None else None
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    ws = None
    if wide and move_needs_wide(H, W, N):
        ws = (workspace or _Workspace()).get(nat.lib().magat_sim_move_wide_workspace_bytes(B, H, W, N), dev)
    sh.call(dev, "magat_sim_move", nat.ptr(lg), nat.ptr(ac), nat.ptr(m), 1 if m.dim() == 3 else 0, H, W, nat.ptr(pos), nat.ptr(gl),
            nat.ptr(a_out), nat.ptr(mv), nat.ptr(reached), nat.ptr(flags), B, N, ws=ws)
    return dict(actions=a_out, moves=mv, reached=None if reached is None else reached.bool(), flags=flags)


POLICIES = {"soft_max": 0, "sum_multinorm": 1, "exp_multinorm": 2}


class BatchedEpisode:
    """B planning cases stepped together with ALL simulator state on the device - the batched counterpart of one
    multiRobotSimNew between setup() and the end of the episode (utils/new_simulator.py:108-221, 471-549):
    current positions, reach_goal / first_move / end_step, the step-0 communication radius, makespan and flowtime.

    action_select: 'soft_max' | 'sum_multinorm' | 'exp_multinorm' (config.action_select; the reference's default outside
    'test_trainingSet' mode is exp_multinorm, :134-145).  The multinomial policies draw from `generator` (a device
    torch.Generator; seeded runs repeat exactly) - one float64 uniform per agent and step, inverse CDF on the device.

    wide=True: maps up to 256 x 256 (batched_fov_states' and batched_move's keyword).  states() with 'GlobalG_*' / 'SemiLG_*'
    and step() take the wide kernels where the narrow limits are exceeded, each with a workspace the episode owns; `moves`
    (B,N,2) int8 holds the last step's shielded moves."""

    def __init__(self, obstacle_map, pos, goal, maxstep, comm_radius, action_select="soft_max", symmetric_norm=False,
                 FOV=9, generator=None, guidance="Project_G", wide=False):
        if action_select not in POLICIES:
            raise ValueError("action_select must be one of %s" % sorted(POLICIES))
        if guidance not in GUIDANCE_MODES:
            raise ValueError("guidance must be one of %s, got %r" % (sorted(GUIDANCE_MODES), guidance))
        self.pos = _dev_i32(pos, "pos").clone()
        self.goal = _dev_i32(goal, "goal")
        self.map = sh.dev_u8(obstacle_map, "obstacle_map")
        B, N, _ = self.pos.shape
        dev = self.pos.device
        self.B, self.N, self.dev = B, N, dev
        self.policy = POLICIES[action_select]
        self.maxstep = int(maxstep)
        self.comm_radius, self.symmetric_norm, self.FOV = float(comm_radius), bool(symmetric_norm), int(FOV)
        self.generator = generator
        self.guidance = guidance
        self.wide = bool(wide)
        self._guide_ws, self._move_ws = _Workspace(), _Workspace()
        # 'SemiLG_*': what every agent has seen so far, empty at the start of the episode (AgentState.setmap, once per episode in
        # multiRobotSimNew.setup) and owned by the episode
        self.agent_view = None
        if guidance.startswith("SemiLG"):
            self.agent_view = new_agent_view(B, N, self.map.shape[-2], self.map.shape[-1], self.FOV, dev)
        self.currentstep = 0
        self.radii = None
        self._edges = self._valued_edges = None
        self.reach_goal = torch.zeros(B, N, dtype=torch.uint8, device=dev)
        self.first_move = torch.zeros(B, N, dtype=torch.int32, device=dev)
        self.end_step = torch.zeros(B, N, dtype=torch.int32, device=dev)
        self.done = torch.zeros(B, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(B, dtype=torch.int32, device=dev)
        self.actions = torch.empty(B, N, dtype=torch.int32, device=dev)
        self.moves = torch.zeros(B, N, 2, dtype=torch.int8, device=dev)
        # makespanPredict / flowtimePredict start at maxstep and maxstep * N (:220-221)
        self.makespan = torch.full((B,), self.maxstep, dtype=torch.int32, device=dev)
        self.flowtime = torch.full((B,), self.maxstep * N, dtype=torch.int32, device=dev)

    def _grow_radii(self):
        if self.radii is None:
            self.radii, steps = batched_connect_radius(self.pos, self.comm_radius, return_steps=True)
            # once per episode (the reference grows the radius until the graph IS connected, new_simulator.py:759-768):
            # an instance still disconnected after the kernel's step limit must not be used silently
            if bool((steps < 0).any().item()):
                bad = torch.nonzero(steps < 0).flatten().tolist()
                raise nat.MagatNativeError("communication graph still disconnected after the radius growth limit in "
                                           "instances %s" % bad[:8])

    def gso(self, dtype=torch.float64):
        """getGSO(step): at the first call the radius grows until each instance's graph is connected and is kept."""
        self._grow_radii()
        return batched_gso(self.pos, self.radii, symmetric_norm=self.symmetric_norm, dtype=dtype)

    def edges(self, values=False):
        """gso()'s graph as a GraphEdges over the episode's own positions and kept radii (the same growth and the same check at
        the first call) - for DecentralPlannerGATNet.addGSO.  One object per episode, refreshed by every call: its structure is
        built from the positions as they are when addGSO asks for it, and the forward orders the stream behind that build.
        values=True: the graph with gso()'s values under the episode's symmetric_norm (GraphEdges.values) - for the GNN planners'
        addGSO; an object of its own, refreshed in the same way."""
        self._grow_radii()
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
        """move(actionVec, currentstep) for every instance; returns `done` (B,) int32 = allReachGoal as the reference
        returns it (evaluated before the move).  No host synchronisation."""
        B, N, dev = self.B, self.N, self.dev
        lg, ac = sh.dev_actions(logits, actions, B, N)
        policy = self.policy if lg is not None else 0
        if policy and uniforms is None:
            uniforms = torch.rand(B, N, dtype=torch.float64, device=dev, generator=self.generator)
        if uniforms is not None:
            uniforms = sh.dev_uniforms(uniforms, B, N)
        d = nat.SimStepDesc()
        d.logits, d.actions_in, d.map = nat.ptr(lg), nat.ptr(ac), nat.ptr(self.map)
        d.map_batched = 1 if self.map.dim() == 3 else 0
        d.H, d.W, d.B, d.N = self.map.shape[-2], self.map.shape[-1], B, N
        d.policy, d.uniforms = policy, nat.ptr(uniforms)
        d.pos, d.goal = nat.ptr(self.pos), nat.ptr(self.goal)
        d.reach_goal, d.first_move, d.end_step = nat.ptr(self.reach_goal), nat.ptr(self.first_move), nat.ptr(self.end_step)
        d.currentstep, d.maxstep = self.currentstep, self.maxstep
        d.actions_out, d.moves_out, d.flags_out = nat.ptr(self.actions), nat.ptr(self.moves), nat.ptr(self.flags)
        d.done_out, d.flowtime_out, d.makespan_out = nat.ptr(self.done), nat.ptr(self.flowtime), nat.ptr(self.makespan)
        ws = None
        if self.wide and move_needs_wide(d.H, d.W, N):
            ws = self._move_ws.get(nat.lib().magat_sim_move_wide_workspace_bytes(B, d.H, d.W, N), dev)
        sh.call(dev, "magat_sim_step", ctypes.byref(d), ws=ws)
        self.currentstep += 1
        return self.done
