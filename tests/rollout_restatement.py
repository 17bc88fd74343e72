"""Plain restatement of the case pool (magat_pathplanning_amd/rollout.py, csrc/sim_pool.hip), written from DESIGN 4.13 over
Python ints and numpy cells - TEST HELPER.  The move itself is the simulator oracle's (oracle/sim_oracle.py: episode_step,
connect_radius), which tests/test_sim_oracle_golden.py pins to the reference; everything around it is restated here:

    pool = Pool(maps, start, goal, maxstep, slots, comm_radius, policy=0, seed=0, first_step=1, record=False)
    pool.step(logits_of(pool) | keys, uniforms=None)       # one call for every slot, then the turn
    pool.finished(); pool.rows                             # per case: the result row, a dict

Rules.  A slot holds a case (slot_case, -1: none), the step number of its next call (slot_step) and the case's limit.  step():
every slot with a case makes ONE move() call with its own step number and limit; the call finalises when every agent had
arrived before it or step >= limit (it then moves nothing).  The flag word of a call that moved is or-ed into the slot's sticky
word: bit 0 out of the arena, 1 swap, 2 obstacle, 3 cell conflict.  turn(): the slots whose call finalised write their case's row
and are refilled - in ascending slot order they take the cases next, next + 1, ...; beyond the queue a slot goes idle and keeps
its positions.  A refill copies start / goal / map, zeroes the bookkeeping, sets slot_step = first_step and grows the step-0
radius r = R / 1.1; r *= 1.1 until connected (64 growth steps at most, else status bit 1).  Every other slot with a case appends
its positions to its case's trajectory (record) and its step number grows by one.

Uniforms (all arithmetic mod 2^64; cases_restatement.py: mix, M):
    u(seed, case, step, agent) = ((hi << 21) | (lo >> 11)) * 2^-53,
    hi, lo = draw(seed, case, 16 + step, 2 agent) >> 32, draw(seed, case, 16 + step, 2 agent + 1) >> 32

summary(rows, makespanTarget, flowtimeTarget): the reference's log_result per case and MonitoringMultiAgentPerformance's numbers,
loops over Python numbers."""
import math

import numpy as np

from cases_restatement import draw
from oracle import sim_oracle as so

STREAM_UNIFORM = 16
RADIUS_MAX_STEPS = 64
COLUMNS = ("retired", "all_reach", "num_reach", "steps", "makespan", "flowtime", "predicted_collision", "flag_bits", "status",
           "radius", "end_pos", "first_move", "end_step")


def uniform(seed, case, step, agent):
    hi = draw(seed, case, STREAM_UNIFORM + step, 2 * agent) >> 32
    lo = draw(seed, case, STREAM_UNIFORM + step, 2 * agent + 1) >> 32
    return float((hi << 21) | (lo >> 11)) * 2.0 ** -53


def case_uniforms(seed, case, step, N):
    return np.array([uniform(seed, case, step, n) for n in range(N)], np.float64)


def reference_maxstep(makespan_target, N, rate_maxstep):
    rate = 3 if N >= 20 else rate_maxstep
    return int(int(makespan_target) * rate)


def grow_radius(pos, comm_radius, max_steps=RADIUS_MAX_STEPS):
    """(radius, connected): so.connect_radius with the growth limit."""
    pos = np.asarray(pos, np.float64)
    d = np.sqrt(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1))
    r = comm_radius / 1.1
    for _ in range(max_steps):
        r = r * 1.1
        W = (d < r).astype(np.float64)
        np.fill_diagonal(W, 0.0)
        if so.is_connected(W):
            return r, True
    return r, False


def flag_word(st, keys):
    """The kernel's flag bits 0-3 of one move, from the oracle's shielding report (recomputed on the positions BEFORE the move)."""
    _, fl = so.shield_moves(st.map, st.pos, so.MOVES[keys])
    return (1 if fl["out_boundary"].any() else 0) | (2 if fl["swap"] else 0) | (4 if fl["wall"] else 0) | (8 if fl["collide"] else 0)


class Pool:
    def __init__(self, maps, start, goal, maxstep, slots, comm_radius, policy=0, seed=0, first_step=1, record=False):
        self.maps = np.asarray(maps)
        self.start, self.goal = np.asarray(start, np.int64), np.asarray(goal, np.int64)
        self.C, self.N = self.start.shape[:2]
        self.maxstep = np.broadcast_to(np.asarray(maxstep, np.int64), (self.C,)).copy()
        assert 1 <= slots <= self.C and (self.maxstep >= 1).all()
        self.B, self.R, self.policy, self.seed, self.first_step, self.record = slots, float(comm_radius), policy, seed, first_step, record
        self.next, self.remaining = 0, self.C
        self.slot_case = [-1] * slots
        self.slot_step = [0] * slots
        self.state = [None] * slots             # so.EpisodeState of the slot's case; kept when the slot goes idle
        self.sticky = [0] * slots
        self.radii = [0.0] * slots
        self.over = [False] * slots
        self.done = [False] * slots
        self.rows = [None] * self.C
        self.status = [0] * self.C
        self.radius = [0.0] * self.C
        self.traj = [None] * self.C             # per case: list of (N,2) arrays, the start first
        self.refills = []                       # (call number, slot, case) in the order they happened
        self.calls = 0
        self._turn(init=True)

    def _map(self, c):
        return self.maps if self.maps.ndim == 2 else self.maps[c]

    def pos(self):
        return np.stack([s.pos for s in self.state])

    def slot_goal(self):
        return np.stack([s.goal for s in self.state])

    def uniforms(self):
        return np.stack([case_uniforms(self.seed, c, t, self.N) if c >= 0 else np.zeros(self.N)
                         for c, t in zip(self.slot_case, self.slot_step)])

    def step(self, logits=None, keys=None, uniforms=None):
        """logits (B,N,5) or keys (B,N); uniforms (B,N) or None (the pool's own)."""
        if self.policy and logits is not None and uniforms is None:
            uniforms = self.uniforms()
        for b in range(self.B):
            self.over[b] = False
            c = self.slot_case[b]
            if c < 0:
                continue
            st, t = self.state[b], self.slot_step[b]
            before = st.pos.copy()
            if logits is not None:
                done, _, k = so.episode_step(st, logits[b], t, self.policy, None if uniforms is None else uniforms[b])
            else:                               # given keys: a one-hot per agent decodes to the key
                oh = np.zeros((self.N, 5), np.float32)
                oh[np.arange(self.N), np.clip(keys[b], 0, 4)] = 1
                done, _, k = so.episode_step(st, oh, t, 0, None)
            if k is not None:
                after = st.pos
                st.pos = before
                self.sticky[b] |= flag_word(st, k)
                st.pos = after
            self.done[b] = bool(done)
            self.over[b] = bool(done) or t >= st.maxstep
        self._turn()
        self.calls += 1

    def _turn(self, init=False):
        finished = [b for b in range(self.B) if init or self.over[b]]
        base = self.next
        self.next += len(finished)
        if not init:
            self.remaining -= len(finished)
        for b in range(self.B):
            c = self.slot_case[b]
            if b not in finished:
                if c >= 0:
                    if self.record:
                        self.traj[c].append(self.state[b].pos.copy())
                    self.slot_step[b] += 1
                continue
            if not init:
                st = self.state[b]
                self.rows[c] = dict(retired=1, all_reach=int(self.done[b]), num_reach=int(np.count_nonzero(st.reach_goal)),
                                    steps=self.slot_step[b], makespan=int(st.makespan), flowtime=int(st.flowtime),
                                    predicted_collision=int(self.sticky[b] & 15 != 0), flag_bits=self.sticky[b],
                                    status=self.status[c], radius=self.radius[c], end_pos=st.pos.copy(),
                                    first_move=st.first_move.copy(), end_step=st.end_step.copy())
            new = base + finished.index(b)      # the rank: finished slots below this one
            if new >= self.C:
                self.slot_case[b] = -1
                continue
            self.slot_case[b] = new
            self.slot_step[b] = self.first_step
            self.state[b] = so.EpisodeState(self._map(new), self.start[new], self.goal[new], int(self.maxstep[new]))
            self.sticky[b] = 0
            r, ok = grow_radius(self.start[new], self.R)
            self.radii[b] = self.radius[new] = r
            self.status[new] = 0 if ok else 2
            if self.record:
                self.traj[new] = [self.start[new].copy()]
            self.refills.append((self.calls + (0 if init else 1), b, new))

    def finished(self):
        return self.remaining == 0

    def column(self, name):
        return np.array([r[name] for r in self.rows])


def run(pool, policy_logits, limit=100000):
    """Steps `pool` with logits = policy_logits(pool) (B,N,5) until every case is retired."""
    while not pool.finished():
        pool.step(logits=policy_logits(pool))
        assert pool.calls < limit
    return pool.rows


def summary(rows, maxstep, makespan_target, flowtime_target, N):
    """rows: per case a dict with all_reach, num_reach, steps, makespan, flowtime, predicted_collision.  Returns (log, summary):
    log = the per-case log_result lists of mutliAgent_ActionPolicy (:918-957), summary = MonitoringMultiAgentPerformance's fields."""
    log, dmp, dft = [], [], []
    for c, r in enumerate(rows):
        all_reach, timeout = bool(r["all_reach"]), int(r["steps"]) >= int(maxstep[c])
        mk, ft, mkT, ftT = int(r["makespan"]), int(r["flowtime"]), int(makespan_target[c]), int(flowtime_target[c])
        optimal = False
        if all_reach:                           # no collision ever "happens" in move(): check_collisionFreeSol = allReachGoal
            optimal = mk <= mkT and ft <= ftT
        if timeout:
            optimal = False
        shield = timeout and not all_reach and bool(r["predicted_collision"])
        log.append(dict(allReachGoal=all_reach, noReachGoalbyCollisionShielding=shield, findOptimalSolution=optimal,
                        check_collisionFreeSol=all_reach, check_CollisionPredictedinLoop=bool(r["predicted_collision"]),
                        compare_makespan=[mk, mkT], compare_flowtime=[ft, ftT], num_agents_reachgoal=int(r["num_reach"])))
        dmp.append(abs(mk - mkT) / mkT)
        dft.append(abs(ft - ftT) / ftT)
    C = len(rows)

    def mean_std(v):
        m = math.fsum(v) / C
        return m, (math.sqrt(math.fsum((x - m) ** 2 for x in v) / (C - 1)) if C > 1 else float("nan"))

    count = lambda key: sum(1 for l in log if l[key])      # noqa: E731
    (amp, smp), (aft, sft) = mean_std(dmp), mean_std(dft)
    nums = [l["num_agents_reachgoal"] for l in log]
    return log, dict(count_validset=C, rateReachGoal=count("allReachGoal") / C,
                     rateFailedReachGoalSH=count("noReachGoalbyCollisionShielding") / C,
                     ratefindOptimalSolution=count("findOptimalSolution") / C, rateCollsionFreeSol=count("check_collisionFreeSol") / C,
                     rateCollisionPredictedinLoop=count("check_CollisionPredictedinLoop") / C, avg_rate_deltaMP=amp,
                     std_rate_deltaMP=smp, avg_rate_deltaFT=aft, std_rate_deltaFT=sft, rate_deltaMP=dmp, rate_deltaFT=dft,
                     hist_numAgentReachGoal=[nums.count(i) for i in range(N + 1)])
