"""CPU-only: the one copy of the simulator family's host layer - the limit refusals and the narrow / wide routing of mapf.py, the
adoption rule behind solve_cases(optimal=), solve_cases(bounded=) and adopt_bounded, and the CPU-tensor refusal of every entry
point that takes an obstacle map (magat_pathplanning_amd/_sim_host.py).  The message literals were produced by the code these
functions replaced - _cbs_limits, _ecbs_limits, _ecbs_wide_limits and the two format strings of improve_schedules /
audit_schedules, evaluated at these shapes - not by the functions under test."""
import itertools

import pytest

torch = pytest.importorskip("torch")

from magat_pathplanning_amd import _native as nat  # noqa: E402
from magat_pathplanning_amd import cases, expert, mapf, rollout, simulator  # noqa: E402

SHAPES = [(65, 64, 64), (64, 64, 257), (257, 5, 64), (5, 5, 1025)]      # (H, W, T)
KEYWORD = " (wide=True takes maps up to 256 x 256 and horizons up to 1024)"
NARROW = "takes maps up to 64 x 64 and horizons up to 256, not "
WIDE = "(wide=True) takes maps up to 256 x 256 and horizons up to 1024, not "
CBS = "cbs_cases takes maps up to 64 x 64, horizons up to 256, 4096 agents and 1..4096 nodes per case, not "
ECBS = "ecbs_cases takes maps up to 64 x 64, horizons up to 256, 4096 agents, 1..4096 nodes per case and 1..4 levels, not "
ECBS_WIDE = "ecbs_cases_wide takes maps up to 256 x 256, horizons up to 1024, 4096 agents, 1..4096 nodes per case and 1..4 levels, not "
NO_WIDE = " (it has no wide form)"


def _message(*args, **kw):
    try:
        mapf._limits(*args, **kw)
    except nat.MagatNativeError as e:
        return str(e)
    return None


@pytest.mark.parametrize("who", ["improve_schedules", "audit_schedules"])
def test_limit_messages_of_the_keyword_callers(who):
    got = ["65 x 64 / 64", "64 x 64 / 257", "257 x 5 / 64", "5 x 5 / 1025"]
    for (H, W, T), text in zip(SHAPES, got):
        assert _message(who, H, W, T, wide=False, keyword=True) == who + " " + NARROW + text + KEYWORD
    for (H, W, T), text in zip(SHAPES, [None, None, "257 x 5 / 64", "5 x 5 / 1025"]):      # wide=True takes the first two
        assert _message(who, H, W, T, wide=True, keyword=True) == (None if text is None else who + WIDE + text)
    for wide in (False, True):
        assert _message(who, 64, 64, 256, wide=wide, keyword=True) is None


def test_limit_message_of_the_audit_for_agents():
    for wide in (False, True):
        assert (_message("audit_schedules", 5, 5, 64, 4097, wide=wide, keyword=True)
                == "audit_schedules takes at most 4096 agents per case, not 4097")
        assert _message("audit_schedules", 5, 5, 64, 4096, wide=wide, keyword=True) is None
    # the shape's refusal stands in front of the agents'
    assert _message("audit_schedules", 65, 64, 64, 4097, keyword=True) == "audit_schedules " + NARROW + "65 x 64 / 64" + KEYWORD


def test_limit_messages_of_the_searches():
    cbs = lambda H, W, T, N=3, nodes=16: _message("cbs_cases", H, W, T, N, nodes)      # noqa: E731
    ecbs = lambda H, W, T, N=3, nodes=16, levels=2: _message("ecbs_cases", H, W, T, N, nodes, levels)      # noqa: E731
    wide = lambda H, W, T, N=3, nodes=16, levels=2: _message("ecbs_cases_wide", H, W, T, N, nodes, levels, wide=True)      # noqa: E731
    got = ["65 x 64 / 64", "64 x 64 / 257", "257 x 5 / 64", "5 x 5 / 1025"]
    for (H, W, T), text in zip(SHAPES, got):
        assert cbs(H, W, T) == CBS + text + " / 3 / 16" + NO_WIDE
        assert ecbs(H, W, T) == ECBS + text + " / 3 / 16 / 2" + NO_WIDE
    assert wide(65, 64, 64) is None and wide(64, 64, 257) is None
    assert wide(257, 5, 64) == ECBS_WIDE + "257 x 5 / 64 / 3 / 16 / 2"
    assert wide(5, 5, 1025) == ECBS_WIDE + "5 x 5 / 1025 / 3 / 16 / 2"
    for nodes in (0, 4097):
        assert cbs(5, 5, 64, nodes=nodes) == CBS + "5 x 5 / 64 / 3 / %d" % nodes + NO_WIDE
        assert ecbs(5, 5, 64, nodes=nodes) == ECBS + "5 x 5 / 64 / 3 / %d / 2" % nodes + NO_WIDE
        assert wide(5, 5, 64, nodes=nodes) == ECBS_WIDE + "5 x 5 / 64 / 3 / %d / 2" % nodes
    for levels in (0, 5):
        assert ecbs(5, 5, 64, levels=levels) == ECBS + "5 x 5 / 64 / 3 / 16 / %d" % levels + NO_WIDE
        assert wide(5, 5, 64, levels=levels) == ECBS_WIDE + "5 x 5 / 64 / 3 / 16 / %d" % levels
    assert cbs(5, 5, 64, N=4097) == CBS + "5 x 5 / 64 / 4097 / 16" + NO_WIDE
    assert ecbs(5, 5, 64, N=4097) == ECBS + "5 x 5 / 64 / 4097 / 16 / 2" + NO_WIDE
    assert wide(5, 5, 64, N=4097) == ECBS_WIDE + "5 x 5 / 64 / 4097 / 16 / 2"
    # inside every limit, at the limits themselves
    assert cbs(64, 64, 256, 4096, 4096) is None and cbs(5, 5, 64, nodes=1) is None
    assert ecbs(64, 64, 256, 4096, 4096, 4) is None and ecbs(5, 5, 64, nodes=1, levels=1) is None
    assert wide(256, 256, 1024, 4096, 4096, 4) is None and wide(5, 5, 64, nodes=1, levels=1) is None


# rows: the side 64, 65, 256, 257 (the other side is 5); columns: the horizon 256, 257, 1024, 1025
SIDES, HORIZONS = (64, 65, 256, 257), (256, 257, 1024, 1025)
ROUTES = {
    # improve_schedules, audit_schedules, the searches: what no form takes is refused in Python
    (True, False): ["narrow refuse refuse refuse", "refuse refuse refuse refuse", "refuse refuse refuse refuse", "refuse refuse refuse refuse"],
    (True, True): ["narrow wide wide refuse", "wide wide wide refuse", "wide wide wide refuse", "refuse refuse refuse refuse"],
    # plan_prioritized: never refused in Python - wide=False calls the narrow entry whatever the shape, and the library refuses
    (False, False): ["narrow narrow narrow narrow"] * 4,
    (False, True): ["narrow wide wide wide", "wide wide wide wide", "wide wide wide wide", "wide wide wide wide"],
}


@pytest.mark.parametrize("refuses,wide", sorted(ROUTES))
def test_routing_table(refuses, wide):
    for (i, side), (j, T) in itertools.product(enumerate(SIDES), enumerate(HORIZONS)):
        want = ROUTES[refuses, wide][i].split()[j]
        assert mapf._route(side, 5, T, wide, refuses=refuses) == want, (side, 5, T)
        assert mapf._route(5, side, T, wide, refuses=refuses) == want, (5, side, T)
    assert mapf._route(64, 5, 256, wide) == mapf._route(64, 5, 256, wide, refuses=True)      # the default is the refusing rule


def _res(paths, lengths, solved, **more):
    paths = torch.tensor(paths, dtype=torch.int32)
    lengths = torch.tensor(lengths, dtype=torch.int32)
    out = dict(paths=paths, lengths=lengths, makespan=lengths.max(1).values - 1, solved=torch.tensor(solved, dtype=torch.uint8),
               start=paths[:, :, 0].clone(), goal=paths[:, :, -1].clone())
    out.update({key: torch.tensor(value, dtype=torch.int32) for key, value in more.items()})
    return out


def test_adoption_rules_on_hand_made_dicts():
    """Four cases of one agent, T = 4: an unsolved plan, a plan with a larger flowtime, a plan with the SAME flowtime, each with
    a search that ended with status 0, and a search that ran out of its budget.  solve_cases(optimal=)'s rule takes the first
    three, solve_cases(bounded=)'s the first two."""
    walk = [[(0, 0), (0, 1), (0, 2), (0, 3)]]
    short = [[(0, 0), (0, 1), (0, 3), (0, 3)]]      # (only told apart here)
    park = [[(0, 0), (0, 0), (0, 0), (0, 0)]]
    res = _res([park, walk, walk, walk], [[1], [4], [4], [4]], [0, 1, 1, 1], failed_agent=[0, -1, -1, -1])
    sub = _res([walk, short, short, park], [[4], [3], [4], [1]], [1, 1, 1, 0], status=[0, 0, 0, 1], flowtime=[3, 2, 3, -1],
               lower_bound=[3, 2, 3, 2], nodes=[1, 3, 5, 8], horizon_hit=[0, 1, 0, 0])
    before = {key: value.clone() for key, value in list(res.items()) + [("sub_" + k, v) for k, v in sub.items()]}
    out = mapf._adopt(res, sub, "optimal")
    assert out["paths"].tolist() == _res([walk, short, short, walk], [[4], [3], [4], [4]], [1] * 4)["paths"].tolist()
    assert out["lengths"].tolist() == [[4], [3], [4], [4]] and out["makespan"].tolist() == [3, 2, 3, 3]
    assert out["solved"].tolist() == [1, 1, 1, 1] and out["failed_agent"].tolist() == [-1, -1, -1, -1]
    assert out["cbs_status"].tolist() == [0, 0, 0, 1] and out["cbs_bound"].tolist() == [3, -1, 3, 2]
    assert out["cbs_nodes"].tolist() == [1, 3, 5, 8] and out["optimal"].tolist() == [True, True, True, False]
    assert out["optimal"].dtype == torch.bool and out["paths"].dtype == torch.int32 and out["solved"].dtype == torch.uint8
    assert list(out) == list(res) + ["cbs_status", "cbs_bound", "cbs_nodes", "optimal"]
    assert out["start"] is res["start"] and out["goal"] is res["goal"]      # what is not replaced is shared
    for key, value in before.items():      # neither input is modified
        assert torch.equal(sub[key[4:]] if key.startswith("sub_") else res[key], value), key
    bare = {key: value for key, value in res.items() if key != "failed_agent"}
    assert "failed_agent" not in mapf._adopt(bare, sub, "optimal") and "failed_agent" not in mapf._adopt(bare, sub, "bounded")
    assert "T" not in mapf._adopt(dict(res, T=4), sub, "optimal")
    # the ECBS rule is adopt_bounded, key for key and bit for bit
    got, want = mapf._adopt(res, sub, "bounded"), mapf.adopt_bounded(res, sub)
    assert list(got) == list(want) == list(res) + ["ecbs_status", "ecbs_bound", "ecbs_nodes", "bounded"]
    for key in want:
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    assert want["paths"].tolist() == _res([walk, short, walk, walk], [[4], [3], [4], [4]], [1] * 4)["paths"].tolist()


def _cpu_calls():
    m = torch.zeros(5, 5, dtype=torch.uint8)
    s = torch.zeros(2, 3, 2, dtype=torch.int32)
    res = dict(paths=torch.zeros(2, 3, 4, 2, dtype=torch.int32), lengths=torch.ones(2, 3, dtype=torch.int32), start=s, goal=s,
               makespan=torch.zeros(2, dtype=torch.int32), solved=torch.ones(2, dtype=torch.uint8))
    return {
        "plan_prioritized": lambda: mapf.plan_prioritized(m, s, s),
        "improve_schedules": lambda: mapf.improve_schedules(m, res),
        "audit_schedules": lambda: mapf.audit_schedules(m, res),
        "cbs_cases": lambda: mapf.cbs_cases(m, s, s),
        "ecbs_cases": lambda: mapf.ecbs_cases(m, s, s),
        "ecbs_cases_wide": lambda: mapf.ecbs_cases_wide(m, s, s),
        "solve_cases": lambda: mapf.solve_cases(m, s, s),
        "batched_fov_states": lambda: simulator.batched_fov_states(m, s, s),
        "replayed_semi_states": lambda: simulator.replayed_semi_states(m, s, s, dict(case=res["makespan"], step=res["makespan"],
                                                                                      table=res["paths"])),
        "batched_move": lambda: simulator.batched_move(m, s, actions=torch.zeros(2, 3, dtype=torch.int32)),
        "BatchedEpisode": lambda: simulator.BatchedEpisode(m, s, s, 10, comm_radius=7.0),
        "EpisodePool": lambda: rollout.EpisodePool(m, s, s, 5, 1, 7.0),
        "expert_samples": lambda: expert.expert_samples(m, res["paths"], res["lengths"], s, res["makespan"], 7.0),
        "generate_cases": lambda: cases.generate_cases(2, 5, 5, 3, obstacle_map=m),
    }


@pytest.mark.parametrize("name", sorted(_cpu_calls()))
def test_cpu_tensors_are_refused(name):
    """Every entry point that takes an obstacle map: CPU tensors raise before anything is launched, so this needs no GPU."""
    with pytest.raises(nat.MagatNativeError, match="no CPU fallback"):
        _cpu_calls()[name]()
