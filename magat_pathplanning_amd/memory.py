"""A device-resident training set and the online-expert harvest: what joins the expert pipeline - generate_cases, solve_cases /
ecbs_cases, expert.py's transformer, BatchedEpisode - into the loop the reference is named after
(agents/decentralplannerlocal_OnlineExpert_GAT.py).

    mem = ExpertMemory(capacity, N, H, W, max_length, comm_radius=config.commR, guidance=config.guidance)
    mem.append(obstacle_map, **solved_pack(res))                  # schedules, a few KB per case; an illegal move is refused here
    for b in mem.epoch(64, generator=g):                          # every (case, step) sample once, shuffled
        net.addGSO(b["GSO"]); loss = CrossEntropyLoss()(net(b["inputTensor"]).reshape(-1, 5), b["action"].reshape(-1))
    ...
    ep = BatchedEpisode(maps, start, goal, maxstep, comm_radius=config.commR); ... ep.step(logits) until ep.maxstep ...
    online_expert(ep, mem)                                         # the failed cases, solved from where the agents stand, appended

The reference's loader (dataloader/Dataloader_dcplocal_notTF_onlineExpert.py:117-175, 243-259) keeps every case as a file of
its materialised steps; an item is one (case, step) pair over range(makespan) of every case, items are shuffled, a batch has 64.
expert_samples is that materialisation - inputTensor (C,T,N,3,11,11) and GSO (C,T,N,N) at full size - and 128 cases of
50 x 50 / 100 agents come to gigabytes.  ExpertMemory stores the schedules only and encodes exactly the drawn steps when a
minibatch is asked for: one launch of magat_sim_expert_pick (csrc/sim_expert_pick.h) decodes positions, targets, goals, radii
and maps of the drawn samples, then batched_fov_states and batched_gso run on those rows - the kernels and the arguments
expert_samples uses, so a minibatch equals the same rows of flatten_samples(expert_samples(...)) bit for bit.  guidance
'SemiLG_*' (replay=True) encodes the rows with replayed_semi_states instead, the store itself as the agents' history.

HIP only: CPU tensors raise MagatNativeError.  minibatch never waits for the device; append, check and online_expert do."""
import torch

from . import _native as nat
from . import _sim_host as sh
from . import mapf
from .expert import MAX_AGENT_STEPS, bad_move_message, expert_radius, expert_schedule
from .simulator import GUIDANCE_MODES, batched_fov_states, batched_gso, replayed_semi_states

MAX_SIDE = 256               # a stored cell is row << 8 | col
NO_ROW = 0x7fffffff          # the error flag's value while every index has been in range
PICK_KEYS = ("case", "step", "pos", "target", "action", "goal", "radii", "map")      # the outputs of the pick launch


class ExpertMemory:
    """Schedules of up to `capacity` cases of N agents on H x W maps (at most 256 x 256), paths of at most max_length cells.
    All storage is allocated here, once: cells (capacity,N,max_length) uint16 = row << 8 | col, padded behind lengths with the
    path's last cell; lengths (capacity,N), goal (capacity,N,2), makespan (capacity,) int32; radii (capacity,) float64; cum
    (capacity,) int64, the inclusive prefix sums of makespan + 1; maps (capacity,H,W) uint8 - or `shared_map` (H,W), one map for
    every case, and maps is None; flag (1,) int32, the sticky error flag of minibatch.  len(mem) is the number of stored
    samples, sum(makespan + 1); mem.cases the number of stored cases.  There is no eviction: a full memory refuses.

    comm_radius, dynamic_commR, symmetric_norm, FOV, guidance, gso_dtype, wide: expert_samples' arguments, fixed for the memory.
    guidance 'SemiLG_*' raises ValueError unless replay=True: an agent's view is the history of its whole episode, so one step
    cannot be encoded without replaying the case (expert_samples does).  With replay=True the memory is built and a minibatch
    replays on the device: replayed_semi_states rebuilds each drawn agent's remembered map from the stored cells 0 .. step (the
    store itself is the history), in the one launch that encodes the states.  Other guidances do not read the keyword."""

    def __init__(self, capacity, N, H, W, max_length, comm_radius, dynamic_commR=False, symmetric_norm=False, FOV=9,
                 guidance="Project_G", gso_dtype=torch.float32, shared_map=None, wide=False, device="cuda", replay=False):
        if guidance not in GUIDANCE_MODES:
            raise ValueError("guidance must be one of %s, got %r" % (sorted(GUIDANCE_MODES), guidance))
        if guidance.startswith("SemiLG") and not replay:
            raise ValueError("ExpertMemory: guidance %r encodes an agent's view of its whole episode so far; one step cannot be "
                             "encoded without replaying the case (use expert_samples, or replay=True)" % guidance)
        if gso_dtype not in (torch.float32, torch.float64):
            raise TypeError("ExpertMemory: gso_dtype must be torch.float32 or torch.float64, got %s" % (gso_dtype,))
        capacity, N, H, W, max_length = int(capacity), int(N), int(H), int(W), int(max_length)
        if min(capacity, N, H, W, max_length) <= 0 or H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError("ExpertMemory: capacity, N, H, W, max_length must be positive and H, W at most %d, not %s"
                             % (MAX_SIDE, (capacity, N, H, W, max_length)))
        dev = torch.device(device)
        if dev.type != "cuda":
            raise nat.MagatNativeError("ExpertMemory lives on the device (no CPU fallback), not on %s" % (dev,))
        if shared_map is not None:
            sh.dev_tensor(shared_map, "shared_map")
            if tuple(shared_map.shape) != (H, W):
                raise ValueError("shared_map must be (%d, %d), not %s" % (H, W, tuple(shared_map.shape)))
            dev = shared_map.device
            shared_map = shared_map.to(torch.uint8).contiguous()
        self.capacity, self.N, self.H, self.W, self.max_length = capacity, N, H, W, max_length
        self.comm_radius, self.dynamic_commR, self.symmetric_norm = float(comm_radius), bool(dynamic_commR), bool(symmetric_norm)
        self.FOV, self.guidance, self.gso_dtype, self.wide, self.device = int(FOV), guidance, gso_dtype, bool(wide), dev
        self.shared_map = shared_map
        self.replay = bool(replay) and guidance.startswith("SemiLG")
        self._cells = torch.zeros(capacity, N, max_length, dtype=torch.int16, device=dev)      # (the bits of `cells`)
        self.cells = self._cells.view(torch.uint16)
        self.lengths = torch.zeros(capacity, N, dtype=torch.int32, device=dev)
        self.goal = torch.zeros(capacity, N, 2, dtype=torch.int32, device=dev)
        self.makespan = torch.zeros(capacity, dtype=torch.int32, device=dev)
        self.radii = torch.zeros(capacity, dtype=torch.float64, device=dev)
        self.cum = torch.zeros(capacity, dtype=torch.int64, device=dev)
        self.maps = None if shared_map is not None else torch.zeros(capacity, H, W, dtype=torch.uint8, device=dev)
        self.flag = torch.full((1,), NO_ROW, dtype=torch.int32, device=dev)
        self.cases = 0
        self._samples = 0

    def __len__(self):
        return self._samples

    def append(self, obstacle_map, paths, lengths, goal, makespan, start=None, T=None):
        """Stores C cases: obstacle_map (C,H,W) - for a shared-map memory (H,W) or None - and the **pack of pack_schedules /
        solved_pack / certified_pack (`start` is accepted and not used: the schedule's first cells are the starts).  The cases
        go through expert_schedule, in expert_samples' chunks of at most MAX_AGENT_STEPS (case, step, agent) samples, and an
        illegal move raises ValueError; with dynamic_commR their radii come from expert_radius, and a graph still disconnected
        at its growth limit raises MagatNativeError, as in expert_samples.  MagatNativeError also for: more cases than there is
        room for, a path longer than max_length, a cell or a goal off the map, a negative makespan, another N, H or W, a
        per-case map given to a shared-map memory (or another map than the shared one) or the reverse, CPU tensors.  Whatever
        is refused is refused BEFORE anything is written: len(mem), mem.cases and every stored bit stay as they were.  Cells
        are packed from `lengths`, not from the padding, so appends with different Lmax leave the state one append of their
        concatenation leaves.  Reads back once (twice when T is None); not for the hot path.  Returns the number of samples
        added."""
        paths, lengths = sh.dev_i32(paths, "paths"), sh.dev_i32(lengths, "lengths")
        goal, makespan = sh.dev_i32(goal, "goal"), sh.dev_i32(makespan, "makespan").reshape(-1)
        if obstacle_map is not None:
            sh.dev_tensor(obstacle_map, "obstacle_map")
        N, H, W, cap = self.N, self.H, self.W, self.max_length
        if paths.dim() != 4 or paths.shape[3] != 2 or paths.shape[1] != N or paths.shape[2] < 1:
            raise nat.MagatNativeError("ExpertMemory.append: paths must be (C,%d,Lmax,2), not %s" % (N, tuple(paths.shape)))
        C, _, Lmax, _ = paths.shape
        if C < 1 or tuple(lengths.shape) != (C, N) or tuple(goal.shape) != (C, N, 2) or makespan.numel() != C:
            raise nat.MagatNativeError("ExpertMemory.append: lengths, goal and makespan must be (C,N), (C,N,2) and (C,) of paths' "
                                       "C = %d and N = %d" % (C, N))
        if self.shared_map is not None:
            if obstacle_map is not None and obstacle_map.dim() != 2:
                raise nat.MagatNativeError("ExpertMemory.append: this memory holds one shared map; per-case maps are refused")
            if obstacle_map is not None and tuple(obstacle_map.shape) != (H, W):
                raise nat.MagatNativeError("ExpertMemory.append: the map must be %d x %d, not %s" % (H, W, tuple(obstacle_map.shape)))
        else:
            if obstacle_map is None or obstacle_map.dim() != 3:
                raise nat.MagatNativeError("ExpertMemory.append: this memory holds per-case maps (C,H,W); a shared map is refused")
            if tuple(obstacle_map.shape) != (C, H, W):
                raise nat.MagatNativeError("ExpertMemory.append: the maps must be (%d, %d, %d), not %s"
                                           % (C, H, W, tuple(obstacle_map.shape)))
        if self.cases + C > self.capacity:
            raise nat.MagatNativeError("ExpertMemory.append: %d cases do not fit: %d of %d are taken" % (C, self.cases, self.capacity))
        if paths.device != self.device:
            raise nat.MagatNativeError("ExpertMemory.append: the schedules are on %s, the memory on %s" % (paths.device, self.device))
        if T is None:
            T = int(makespan.max().item()) + 1
        T = max(1, int(T))
        # the schedules' own check and the radii, chunked like expert_samples; nothing of the memory is touched yet
        chunk = max(1, MAX_AGENT_STEPS // (T * N))
        bad, radii, grow = [], [], []
        for c0 in range(0, C, chunk):
            c1 = min(C, c0 + chunk)
            sched = expert_schedule(paths[c0:c1], lengths[c0:c1], goal[c0:c1], makespan[c0:c1], T=T, check=False)
            bad.append(sched["bad"])
            if self.dynamic_commR:
                r, g = expert_radius(sched["pos"], sched["valid"], self.comm_radius)
                radii.append(r)
                grow.append(g)
        bad = torch.cat(bad)
        if self.dynamic_commR:
            radii, grow = torch.cat(radii), torch.cat(grow)
        else:
            radii = torch.full((C,), self.comm_radius, dtype=torch.float64, device=self.device)
            grow = torch.zeros(C, dtype=torch.int32, device=self.device)
        live = torch.arange(Lmax, device=self.device)[None, None, :] < lengths[:, :, None]            # (C,N,Lmax): cells of a path
        limit = torch.tensor([H, W], dtype=torch.int32, device=self.device)
        off_map = (((paths < 0) | (paths >= limit)).any(dim=3) & live).any() | ((goal < 0) | (goal >= limit)).any()
        steps = (makespan.to(torch.int64) + 1)
        other_map = torch.zeros((), dtype=torch.bool, device=self.device)
        if self.shared_map is not None and obstacle_map is not None:
            other_map = (obstacle_map.to(torch.uint8) != self.shared_map).any()
        report = torch.cat([torch.stack([lengths.max(), lengths.min(), makespan.min()]).to(torch.int64),
                            torch.stack([off_map, other_map]).to(torch.int64), steps.sum().reshape(1), bad.to(torch.int64),
                            grow.to(torch.int64)]).cpu()      # the one read-back
        longest, shortest, least, off, other, added = [int(v) for v in report[:6].tolist()]
        if longest > cap or longest > Lmax or shortest < 1:
            raise nat.MagatNativeError("ExpertMemory.append: paths hold %d to %d cells; the memory takes 1 to %d (paths' Lmax is %d)"
                                       % (shortest, longest, cap, Lmax))
        if least < 0:
            raise nat.MagatNativeError("ExpertMemory.append: a makespan is negative")
        if off:
            raise nat.MagatNativeError("ExpertMemory.append: a cell of a path or a goal is off the %d x %d map" % (H, W))
        if other:
            raise nat.MagatNativeError("ExpertMemory.append: the map is not the memory's shared map")
        msg = bad_move_message(report[6:6 + C], N)
        if msg is not None:
            raise ValueError(msg)
        if bool((report[6 + C:] < 0).any()):
            cases = torch.nonzero(report[6 + C:] < 0).flatten().tolist()
            raise nat.MagatNativeError("communication graph still disconnected after the radius growth limit in cases %s" % cases[:8])
        # the write: cell l of a path is its cell min(l, L - 1)
        lo, hi = self.cases, self.cases + C
        packed = (paths[..., 0] << 8) | paths[..., 1]                                                # (C,N,Lmax) int32
        take = torch.minimum(torch.arange(cap, device=self.device)[None, None, :], (lengths[:, :, None] - 1).to(torch.int64))
        self._cells[lo:hi] = torch.gather(packed, 2, take.expand(C, N, cap)).to(torch.int16)      # (the low 16 bits)
        self.lengths[lo:hi] = lengths
        self.goal[lo:hi] = goal
        self.makespan[lo:hi] = makespan
        self.radii[lo:hi] = radii
        self.cum[lo:hi] = torch.cumsum(steps, 0) + self._samples
        if self.maps is not None:
            self.maps[lo:hi] = obstacle_map.to(torch.uint8)
        self.cases = hi
        self._samples += added
        return added

    def minibatch(self, M=None, generator=None, indices=None, out=None):
        """M samples, encoded now.  indices: an (M,) int64 device tensor of sample numbers in [0, len(mem)); without it
        torch.randint(len(mem), (M,), generator=generator) is drawn on the device.  Returns a dict: inputTensor
        (M,N,3,FOV+2,FOV+2) float32, target (M,N,5) float32 one-hot, action (M,N) int64 = target.argmax(-1) (what CrossEntropyLoss
        takes), GSO (M,N,N) gso_dtype, pos (M,N,2) int32, case, step (M,) int32 - and the pick's other outputs goal (M,N,2) int32,
        radii (M,) float64, map (M,H,W) uint8 (the shared map itself in a shared-map memory), plus indices.

        One launch of magat_sim_expert_pick, then batched_fov_states on the picked positions, goals and maps (a replay memory:
        replayed_semi_states on them, with the store as the history of the picked case / step) and batched_gso with
        comm_radius (dynamic_commR: the picked radii) - expert_samples' calls on the same rows.  No host synchronisation.  An index
        outside the range is clamped into it (the row is then still a real sample) and remembered: check() raises.  out: a dict
        from an earlier call with the same M - the pick's outputs are written into its tensors and nothing is allocated for them,
        so the call can be captured into a graph (inputTensor and GSO are the encoders' own allocations, as everywhere)."""
        if self.cases == 0:
            raise ValueError("ExpertMemory.minibatch: the memory is empty")
        dev, N, H, W = self.device, self.N, self.H, self.W
        if indices is None:
            if M is None:
                raise ValueError("ExpertMemory.minibatch: give M or indices")
            indices = torch.randint(self._samples, (int(M),), generator=generator, device=dev)
        else:
            sh.dev_tensor(indices, "indices")
            if indices.dtype != torch.int64 or indices.dim() != 1 or not indices.is_contiguous() or indices.numel() == 0:
                raise nat.MagatNativeError("indices must be a contiguous, non-empty (M,) int64 device tensor")
            if M is not None and int(M) != indices.numel():
                raise ValueError("ExpertMemory.minibatch: M = %d, but %d indices" % (int(M), indices.numel()))
        M = indices.numel()
        shapes = dict(case=((M,), torch.int32), step=((M,), torch.int32), pos=((M, N, 2), torch.int32),
                      target=((M, N, 5), torch.float32), action=((M, N), torch.int64), goal=((M, N, 2), torch.int32),
                      radii=((M,), torch.float64))
        if self.maps is not None:
            shapes["map"] = ((M, H, W), torch.uint8)
        if out is None:
            b = {key: torch.empty(shape, dtype=dtype, device=dev) for key, (shape, dtype) in shapes.items()}
        else:
            b = {}
            for key, (shape, dtype) in shapes.items():
                t = out.get(key)
                if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or tuple(t.shape) != shape
                        or not t.is_contiguous()):
                    raise ValueError("ExpertMemory.minibatch: out[%r] must be a contiguous %s device tensor of shape %s (a dict of "
                                     "an earlier call with the same M)" % (key, dtype, shape))
                b[key] = t
        sh.call(dev, "magat_sim_expert_pick", nat.ptr(self._cells), nat.ptr(self.lengths), nat.ptr(self.goal), nat.ptr(self.makespan),
                nat.ptr(self.radii), nat.ptr(self.cum), nat.ptr(self.maps), nat.ptr(indices), nat.ptr(b["case"]), nat.ptr(b["step"]),
                nat.ptr(b["pos"]), nat.ptr(b["target"]), nat.ptr(b["action"]), nat.ptr(b["goal"]), nat.ptr(b["radii"]),
                nat.ptr(b.get("map")), nat.ptr(self.flag), self.cases, N, self.max_length, H, W, M)
        if self.maps is None:
            b["map"] = self.shared_map
        if self.replay:
            hist = dict(case=b["case"], step=b["step"], cells=self.cells, lengths=self.lengths, goal=self.goal)
            b["inputTensor"] = replayed_semi_states(b["map"], b["pos"], b["goal"], hist, self.FOV, self.guidance, self.wide)
        else:
            b["inputTensor"] = batched_fov_states(b["map"], b["pos"], b["goal"], self.FOV, self.guidance, None, self.wide)
        b["GSO"] = batched_gso(b["pos"], b["radii"] if self.dynamic_commR else self.comm_radius,
                               symmetric_norm=self.symmetric_norm, dtype=self.gso_dtype)
        b["indices"] = indices
        return b

    def epoch(self, M, generator=None, drop_last=False):
        """Minibatches of M over torch.randperm(len(mem), generator=generator): every sample exactly once; the last batch is
        shorter unless drop_last."""
        M = int(M)
        if M <= 0:
            raise ValueError("ExpertMemory.epoch: M must be positive")
        perm = torch.randperm(self._samples, generator=generator, device=self.device)
        for i in range(0, self._samples, M):
            idx = perm[i:i + M]
            if drop_last and idx.numel() < M:
                return
            yield self.minibatch(indices=idx)

    def check(self):
        """Reads the error flag (one synchronisation): raises MagatNativeError naming the smallest row of a minibatch that was
        given an index outside [0, len(mem)), if there has been one since the memory was made."""
        row = int(self.flag.item())
        if row != NO_ROW:
            raise nat.MagatNativeError("ExpertMemory: a minibatch was given an index outside [0, len(mem)) - first in row %d of its "
                                       "indices (the row was clamped into the range)" % row)


def _narrow(H, W, N, wide):
    return H <= mapf.MAX_SIDE and W <= mapf.MAX_SIDE and mapf.default_horizon(H, W, N, wide) <= mapf.MAX_HORIZON


def online_expert(ep, mem, w=1.1, nodes=256, certify=None):
    """The reference's online expert (agents/decentralplannerlocal_OnlineExpert_GAT.py:400-413, 928-931; utils/new_simulator.py:
    651-681; onlineExpert/ECBS_onlineExpert.py:97-101: ecbs -w 1.1) on a BatchedEpisode that has run to its maxstep: the cases
    whose agents are not all on their goals are solved again from where the agents stand NOW - ECBS(w) with `nodes` nodes per
    case behind the prioritized planner: solve_cases(bounded=w) on shapes it takes, solve_cases(wide=True) + ecbs_cases_wide +
    adopt_bounded on larger ones - and solved_pack of the result (certified_pack at `certify`, when given) is appended to `mem`
    with those cases' maps.  Returns dict(failed (B,) bool, solved (F,) bool over the failed cases - the ones appended -,
    added_cases, added_samples).  When no case failed, no solver is called and nothing is appended.  An episode that has not
    reached maxstep raises ValueError.  Synchronises (one read-back of the failed cases, the solvers' own, append's)."""
    if ep.currentstep < ep.maxstep:
        raise ValueError("online_expert: the episode stands at step %d of %d; the online expert takes the cases that failed by "
                         "maxstep" % (ep.currentstep, ep.maxstep))
    failed = ~(ep.reach_goal != 0).all(dim=1)
    f = torch.nonzero(failed).flatten()                   # (the read-back)
    F = f.numel()
    none = torch.zeros(F, dtype=torch.bool, device=ep.dev)
    if F == 0:
        return dict(failed=failed, solved=none, added_cases=0, added_samples=0)
    batched = ep.map.dim() == 3
    m = ep.map.index_select(0, f) if batched else ep.map
    pos, goal = ep.pos.index_select(0, f), ep.goal.index_select(0, f)
    H, W = ep.map.shape[-2], ep.map.shape[-1]
    if _narrow(H, W, ep.N, ep.wide):
        res = mapf.solve_cases(m, pos, goal, bounded=w, bounded_nodes=nodes, certify=certify, wide=ep.wide)
        audit = res
    else:
        res = mapf.solve_cases(m, pos, goal, wide=True)
        sub = mapf.ecbs_cases_wide(m, pos, goal, w, horizon=res["paths"].shape[2], max_nodes=nodes)
        res = mapf.adopt_bounded(res, sub)
        audit = None
        if certify is not None:
            audit = mapf.audit_schedules(m, res, wide=True)
            audit["flowtime_bound"] = torch.maximum(audit["flowtime_bound"], res["ecbs_bound"])
    # (the audit skips an unsolved case - status 1 -, so the certified cases are solved ones)
    solved = res["solved"] != 0 if certify is None else mapf.certified(audit, certify)
    if not bool(solved.any()):
        return dict(failed=failed, solved=solved, added_cases=0, added_samples=0)
    pack = mapf.solved_pack(res) if certify is None else mapf.certified_pack(res, audit, certify)
    keep = torch.nonzero(solved).flatten()
    if mem.shared_map is not None:
        maps = m if not batched else None
    else:
        maps = m.index_select(0, keep) if batched else m.unsqueeze(0).expand(keep.numel(), H, W)
    added = mem.append(maps, **pack)
    return dict(failed=failed, solved=solved, added_cases=int(keep.numel()), added_samples=added)
