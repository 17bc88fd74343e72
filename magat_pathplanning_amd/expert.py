"""Expert schedules -> imitation-learning samples on the device: what the reference's data transformers do on the host per
case, per step, per agent, in numpy -

    DataTransformer.obtainSchedule / computeAdjacencyMatrix[_fixedCommRadius] / pathtransformer_RelativeCoordinate
                                                    (onlineExpert/DataTransformer_local_onlineExpert.py:181-265, 291-397;
                                                     offlineExpert/DataGen_Transformer_split_IDMap.py does the same offline)
    multiRobotSimNew.getPathTarget                  (utils/new_simulator.py:226-277: the expert's makespan / flowtime)

- for C cases at once.  A schedule is plain data, one (L_i, 2) integer path per agent, whatever solver produced it:

    pack = pack_schedules(paths_per_case, goals_per_case)                 # host lists -> padded device tensors
    s = expert_samples(obstacle_map, comm_radius=config.commR, dynamic_commR=config.dynamic_commR,
                       guidance=config.guidance, **pack)                  # inputTensor, target, GSO, ... (C,T,...)
    b = flatten_samples(s)                                                # (M,N,...) batches, M = sum of the cases' steps
    net.addGSO(b["GSO"]); loss = CrossEntropyLoss()(net(b["inputTensor"]), b["target"].argmax(-1).reshape(-1))
    st = expert_stats(s["target"], pack["start"], pack["goal"], s["valid"])     # makespanTarget sets each episode's maxstep

HIP only (csrc/sim_expert.hip, plus the state / GSO kernels behind simulator.py): CPU tensors raise MagatNativeError.
expert_schedule (check=False), expert_radius and expert_stats are stream ordered and never wait for the device.  expert_samples
and flatten_samples DO synchronise with the host (the valid steps are data dependent; see their docstrings): call them outside
graph capture."""
import numpy as np
import torch

from . import _native as nat
from . import _sim_host as sh
from .simulator import GUIDANCE_MODES, batched_fov_states, batched_gso, new_agent_view, replayed_semi_states

# expert_samples works on chunks of cases that hold at most this many (case, step, agent) samples (padded steps included)
MAX_AGENT_STEPS = 1 << 18


def pack_schedules(paths, goals, makespan=None, device="cuda"):
    """Host helper.  paths[c][n]: the (L, 2) integer (row, col) path of agent n in case c (lists or arrays, lengths ragged, every
    case with the same number of agents); goals[c]: (N, 2).  Returns a dict of device tensors - paths (C,N,Lmax,2) int32 padded
    with the path's last cell, lengths (C,N), goal (C,N,2), start (C,N,2) (the first cell of each path), makespan (C,) - and
    T = max(makespan) + 1 as a Python int (so that expert_schedule / expert_samples need not read it back from the device).
    makespan defaults to max_n(L) - 1 per case; the reference reads it from the solver's statistics, pass it to override."""
    C = len(paths)
    if C == 0 or len(goals) != C:
        raise ValueError("pack_schedules: paths and goals must hold the same, non-zero number of cases")
    per_case = [[np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in case] for case in paths]
    N = len(per_case[0])
    if N == 0 or any(len(case) != N for case in per_case):
        raise ValueError("pack_schedules: every case must hold the same, non-zero number of agents")
    if any(len(p) == 0 for case in per_case for p in case):
        raise ValueError("pack_schedules: an agent's path holds at least its start cell")
    Lmax = max(len(p) for case in per_case for p in case)
    arr = np.zeros((C, N, Lmax, 2), dtype=np.int32)
    lengths = np.zeros((C, N), dtype=np.int32)
    for c, case in enumerate(per_case):
        for n, p in enumerate(case):
            arr[c, n, :len(p)] = p
            arr[c, n, len(p):] = p[-1]
            lengths[c, n] = len(p)
    goal = np.asarray([np.asarray(g, dtype=np.int64).reshape(N, 2) for g in goals]).astype(np.int32)
    if makespan is None:
        mk = lengths.max(axis=1) - 1
    else:
        mk = np.asarray(makespan, dtype=np.int64).reshape(C)
    dev = torch.device(device)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return dict(paths=to(arr), lengths=to(lengths), goal=to(goal), start=to(arr[:, :, 0].copy()),
                makespan=to(mk.astype(np.int32)), T=int(mk.max()) + 1)


def bad_move_message(bad, N):
    """The ValueError text for a `bad` tensor of expert_schedule (host copy), or None when every move is legal."""
    bad = [int(v) for v in bad.reshape(-1).tolist()]
    hits = [(c, v // N, v % N) for c, v in enumerate(bad) if v >= 0]
    if not hits:
        return None
    c, t, n = hits[0]
    return ("expert schedule: case %d step %d agent %d moves by something other than up / left / down / right / stop "
            "(%d case(s) with such a move)" % (c, t, n, len(hits)))


def expert_schedule(paths, lengths, goal, makespan, T=None, check=False):
    """DataTransformer.obtainSchedule for C cases: paths (C,N,Lmax,2), lengths (C,N), goal (C,N,2), makespan (C,) device
    tensors -> dict(pos (C,T,N,2) int32, target (C,T,N,5) float32 one-hot in the order up, left, down, right, stop, valid (C,T)
    uint8, bad (C,) int32).  Case c has makespan[c] + 1 steps; rows behind them are zero and not valid.  T = max(makespan) + 1:
    pass it when the host knows it (pack_schedules returns it), None reads it from the device once.  A move that is none of
    the five leaves its target row zero and sets bad[c] = t * N + n of the first one in (t, n) order (-1: none); check=True
    reads `bad` (the one host synchronisation) and raises ValueError naming case, step and agent, as the reference's
    list.index does."""
    paths, lengths = sh.dev_i32(paths, "paths"), sh.dev_i32(lengths, "lengths")
    goal, makespan = sh.dev_i32(goal, "goal"), sh.dev_i32(makespan, "makespan")
    assert paths.dim() == 4 and paths.shape[3] == 2, "paths must be (C,N,Lmax,2)"
    C, N, Lmax, _ = paths.shape
    assert tuple(lengths.shape) == (C, N) and tuple(goal.shape) == (C, N, 2) and makespan.numel() == C
    if T is None:
        T = int(makespan.max().item()) + 1
    T = int(T)
    dev = paths.device
    pos = torch.empty(C, T, N, 2, dtype=torch.int32, device=dev)
    target = torch.empty(C, T, N, 5, dtype=torch.float32, device=dev)
    valid = torch.empty(C, T, dtype=torch.uint8, device=dev)
    bad = torch.empty(C, dtype=torch.int32, device=dev)
    sh.call(dev, "magat_sim_expert_schedule", nat.ptr(paths), nat.ptr(lengths), nat.ptr(goal), nat.ptr(makespan), nat.ptr(pos),
            nat.ptr(target), nat.ptr(valid), nat.ptr(bad), C, N, Lmax, T)
    if check:
        msg = bad_move_message(bad.cpu(), N)
        if msg is not None:
            raise ValueError(msg)
    return dict(pos=pos, target=target, valid=valid, bad=bad)


def expert_radius(pos, valid, comm_radius, max_steps=64, return_step_grow=False):
    """The dynamic_commR branch of DataTransformer.computeAdjacencyMatrix (:291-353) for C cases: NOT the simulator's step-0 rule
    (batched_connect_radius) - the threshold starts at comm_radius itself, is carried across all steps of a case and grows by
    threshold *= 1.1 (float64) until every valid step's graph is connected; that one radius serves every step.  pos (C,T,N,2),
    valid (C,T) -> radii (C,) float64 (bit-equal to the reference's chain of multiplications), grow_steps (C,) int32 (the
    number of multiplications; -1: a step is still disconnected after max_steps of them)."""
    pos, valid = sh.dev_i32(pos, "pos"), sh.dev_u8(valid, "valid")
    assert pos.dim() == 4 and pos.shape[3] == 2, "pos must be (C,T,N,2)"
    C, T, N, _ = pos.shape
    assert tuple(valid.shape) == (C, T)
    dev = pos.device
    step_grow = torch.empty(C, T, dtype=torch.int32, device=dev)
    radii = torch.empty(C, dtype=torch.float64, device=dev)
    grow = torch.empty(C, dtype=torch.int32, device=dev)
    sh.call(dev, "magat_sim_expert_radius", nat.ptr(pos), nat.ptr(valid), float(comm_radius), nat.ptr(step_grow), nat.ptr(radii),
            nat.ptr(grow), C, T, N, int(max_steps))
    return (radii, grow, step_grow) if return_step_grow else (radii, grow)


def expert_stats(target, start, goal, valid):
    """multiRobotSimNew.getPathTarget (utils/new_simulator.py:226-277) for C cases: follows the argmax actions of target
    (C,T,N,5) from start (C,N,2) over the valid steps.  Returns dict(expert_first_move, expert_end_step (C,N) int32 - step + 1 of
    the first non-stop action / first arrival, 0 when the agent never moves / never arrives, like the reference -,
    makespanTarget = max(end) - min(first) + 1 and flowtimeTarget = sum(end - first + 1) (C,) int32, expert_pos (C,T+1,N,2)
    int32)."""
    target = sh.dev_tensor(target, "target").float().contiguous()
    start, goal, valid = sh.dev_i32(start, "start"), sh.dev_i32(goal, "goal"), sh.dev_u8(valid, "valid")
    assert target.dim() == 4 and target.shape[3] == 5, "target must be (C,T,N,5)"
    C, T, N, _ = target.shape
    assert tuple(start.shape) == (C, N, 2) and tuple(goal.shape) == (C, N, 2) and tuple(valid.shape) == (C, T)
    dev = target.device
    first = torch.empty(C, N, dtype=torch.int32, device=dev)
    end = torch.empty(C, N, dtype=torch.int32, device=dev)
    mk = torch.empty(C, dtype=torch.int32, device=dev)
    flow = torch.empty(C, dtype=torch.int32, device=dev)
    epos = torch.empty(C, T + 1, N, 2, dtype=torch.int32, device=dev)
    sh.call(dev, "magat_sim_expert_stats", nat.ptr(target), nat.ptr(start), nat.ptr(goal), nat.ptr(valid), nat.ptr(first), nat.ptr(end),
            nat.ptr(mk), nat.ptr(flow), nat.ptr(epos), C, T, N)
    return dict(expert_first_move=first, expert_end_step=end, makespanTarget=mk, flowtimeTarget=flow, expert_pos=epos)


def expert_samples(obstacle_map, paths, lengths, goal, makespan, comm_radius, dynamic_commR=False, symmetric_norm=False, FOV=9,
                   guidance="Project_G", gso_dtype=torch.float32, T=None, check=True, max_steps=64,
                   max_agent_steps=MAX_AGENT_STEPS, start=None, wide=False, replay=False):
    """DataTransformer.pathtransformer_RelativeCoordinate (:237-265) for C cases: obstacle_map (H,W) or (C,H,W), the padded
    schedule (pack_schedules) -> dict(inputTensor (C,T,N,3,FOV+2,FOV+2) float32, target (C,T,N,5), GSO (C,T,N,N) gso_dtype,
    pos (C,T,N,2), valid (C,T), radii (C,) float64, grow_steps (C,) int32, makespan (C,), bad (C,)).  Steps at or behind a case's
    makespan + 1 are zero in every tensor and not valid.

    States are batched_fov_states of config.guidance (wide=True: its keyword, 'GlobalG_*' / 'SemiLG_*' on maps up to
    256 x 256 - without it they stop at 54 x 54 at FOV 9), GSOs batched_gso with comm_radius
    (computeAdjacencyMatrix_fixedCommRadius) or, with dynamic_commR, the per-case radii of expert_radius; an instance still
    disconnected after max_steps growth steps raises MagatNativeError (BatchedEpisode.gso's rule).  check=True (default) raises
    ValueError for an illegal move.  Only the valid (case, step) pairs reach those kernels: they are compacted first, so cases
    of different lengths cost their own steps and no kernel sees a padded row's all-zero positions.  The memoryless encodings
    and the GSO take one call over the compacted pairs; 'SemiLG_*' takes one call per step with ONE agent_view per case carried
    from step to step (AgentState.toSeqInputTensor's order), over the cases that still have that step (longest case first,
    so they are a prefix of the batch).  replay=True serves 'SemiLG_*' like the memoryless encodings instead: ONE
    replayed_semi_states call per chunk over the compacted pairs, each agent's remembered map rebuilt on the device from the
    schedule's own `pos` - the same bits, no per-step loop and no carried view; with any other guidance the keyword has no effect.

    SYNCHRONISES with the host, so it cannot be captured into a graph: the step validity is read back once to build the
    compaction index, and so are `bad` (check=True) and grow_steps (dynamic_commR).

    Chunking: the cases are processed in chunks of at most max_agent_steps // (T * N) cases (at least one), so that no
    INTERMEDIATE tensor holds more than max_agent_steps = 2^18 (case, step, agent) samples - 381 MB of float32 states at FOV 9.
    That bound does not cover the results: inputTensor and GSO are allocated at their full (C,T,...) size before the first
    chunk, and the chunks are written into them.  `start` (a key of pack_schedules' dict) is accepted so that **pack works and
    is not used: the schedule's first cells are the starts."""
    if guidance not in GUIDANCE_MODES:
        raise ValueError("guidance must be one of %s, got %r" % (sorted(GUIDANCE_MODES), guidance))
    if gso_dtype not in (torch.float32, torch.float64):
        raise TypeError("expert_samples: gso_dtype must be torch.float32 or torch.float64, got %s" % (gso_dtype,))
    sh.dev_tensor(obstacle_map, "obstacle_map")      # refused before the schedule's launch
    sched = expert_schedule(paths, lengths, goal, makespan, T=T, check=check)
    pos, target, valid = sched["pos"], sched["target"], sched["valid"]
    goal = sh.dev_i32(goal, "goal")
    C, T, N, _ = pos.shape
    dev = pos.device
    m, _, H, W = sh.dev_map(obstacle_map, C)
    if dynamic_commR:
        radii, grow = expert_radius(pos, valid, comm_radius, max_steps=max_steps)
        if bool((grow < 0).any().item()):
            bad = torch.nonzero(grow < 0).flatten().tolist()
            raise nat.MagatNativeError("communication graph still disconnected after the radius growth limit in cases %s"
                                       % bad[:8])
    else:
        radii = torch.full((C,), float(comm_radius), dtype=torch.float64, device=dev)
        grow = torch.zeros(C, dtype=torch.int32, device=dev)
    live = valid.cpu().bool()                                        # (C,T) on the host: the compaction index is built there
    Wt = int(FOV) + 2
    x = torch.zeros(C, T, N, 3, Wt, Wt, dtype=torch.float32, device=dev)
    S = torch.zeros(C, T, N, N, dtype=gso_dtype, device=dev)
    xf, Sf, pf = x.view(C * T, N, 3, Wt, Wt), S.view(C * T, N, N), pos.view(C * T, N, 2)
    semi = guidance.startswith("SemiLG")
    chunk = max(1, int(max_agent_steps) // (T * N))
    for c0 in range(0, C, chunk):
        c1 = min(C, c0 + chunk)
        idx = torch.nonzero(live[c0:c1].reshape(-1)).flatten() + c0 * T      # the chunk's valid rows of the (C * T, ...) views
        if idx.numel() == 0:
            continue
        case = torch.div(idx, T, rounding_mode="floor").to(dev)
        idx = idx.to(dev)
        p = pf.index_select(0, idx)
        if semi and replay:
            step = (idx - case * T).to(torch.int32)
            mm = m if m.dim() == 2 else m.index_select(0, case)
            hist = dict(case=(case - c0).to(torch.int32), step=step, table=pos[c0:c1])
            xf.index_copy_(0, idx, replayed_semi_states(mm, p, goal.index_select(0, case), hist, FOV, guidance, wide))
        elif semi:
            # longest case first: the cases that still have step t are the first k of the batch, and so are their views
            steps = live[c0:c1].sum(dim=1)
            order = torch.argsort(steps, descending=True, stable=True)
            steps = steps[order]
            live_cases = (steps[None, :] > torch.arange(int(steps[0]))[:, None]).sum(dim=1).tolist()      # k of every step t
            order = (order + c0).to(dev)
            ps, gs = pos.index_select(0, order), goal.index_select(0, order)
            ms = m if m.dim() == 2 else m.index_select(0, order)
            view = new_agent_view(c1 - c0, N, H, W, FOV, dev)
            for t, k in enumerate(live_cases):
                mk = ms if ms.dim() == 2 else ms[:k]
                x[order[:k], t] = batched_fov_states(mk, ps[:k, t], gs[:k], FOV, guidance, view[:k], wide)
        else:
            mm = m if m.dim() == 2 else m.index_select(0, case)
            xf.index_copy_(0, idx, batched_fov_states(mm, p, goal.index_select(0, case), FOV, guidance, None, wide))
        r = radii.index_select(0, case) if dynamic_commR else float(comm_radius)
        Sf.index_copy_(0, idx, batched_gso(p, r, symmetric_norm=symmetric_norm, dtype=gso_dtype))
    return dict(inputTensor=x, target=target, GSO=S, pos=pos, valid=valid, radii=radii, grow_steps=grow,
                makespan=sh.dev_i32(makespan, "makespan"), bad=sched["bad"])


def flatten_samples(samples):
    """Drops the invalid steps: every (C,T,...) tensor of expert_samples becomes (M,...) with M = sum of the cases' step
    counts, in (case, step) order - inputTensor (M,N,3,W,W), target (M,N,5), GSO (M,N,N), pos (M,N,2) - plus case (M,) and step
    (M,) int64 indices.  These are what net.addGSO(GSO); net(inputTensor) and CrossEntropyLoss(pred, target.argmax(-1)) take.
    (M is data dependent: the one host synchronisation is the index of the valid steps.)"""
    valid = samples["valid"].bool()
    C, T = valid.shape
    idx = torch.nonzero(valid.reshape(-1)).flatten()
    out = {}
    for key in ("inputTensor", "target", "GSO", "pos"):
        if key in samples:
            v = samples[key]
            out[key] = v.reshape((C * T,) + tuple(v.shape[2:])).index_select(0, idx)
    out["case"] = torch.div(idx, T, rounding_mode="floor")
    out["step"] = idx - out["case"] * T
    return out
