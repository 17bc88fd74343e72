"""CPU-only checks of the GSO's values on the edge structure (csrc/gso_edge_values.hip, magat_pathplanning_amd/edges.py): the numpy
restatement against numpy's eigenvalues and against closed forms, the kernel itself compiled for the host (tools/host_wave) against
the restatement, the entry points' declaration / export / binding and their refusals, and the Python surface on CPU tensors."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import edge_values_restatement as ev
from conftest import ROOT


# ---- the restatement against numpy.linalg.eigvalsh (1e-9 relative: the project's gate for lambda_max) ----------------------------
def _check_against_eigvalsh(pos, radius, sym):
    out = ev.edge_values(pos[None], radius, sym)
    M = ev.matrix(pos, radius, sym)
    want = float(np.linalg.eigvalsh(M)[-1]) if out["nnz"] else 0.0
    assert abs(out["lam"][0] - want) <= 1e-9 * abs(want), (out["lam"][0], want, out["steps"])
    i, j = np.nonzero(M)
    assert np.array_equal(j, out["colidx"])                                # CSR order is numpy's row-major order
    if out["nnz"]:
        assert (ev.ulps32(out["vals"], (M[i, j] / want).astype(np.float32)) <= 1).all()
    return out


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "symmetric_norm"])
@pytest.mark.parametrize("N,side", [(37, 20), (150, 45), (300, 62)])
def test_restatement_equals_eigvalsh_on_random_scatters(N, side, sym):
    pos = ev.random_cells(N, side, seed=3)[0]
    out = _check_against_eigvalsh(pos, 7.0, sym)
    assert out["nnz"] > 4 * N and out["steps"][0] > 8                       # (a graph the walk has to work on)


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "symmetric_norm"])
def test_restatement_with_an_isolated_agent_an_edgeless_instance_and_a_clique(sym):
    pos = ev.random_cells(60, 20, seed=5)[0]
    pos[17] = (400, 400)                                                   # nobody within radius 7
    out = _check_against_eigvalsh(pos, 7.0, sym)
    rp = out["rowptr"]
    assert rp[18] == rp[17] and np.isfinite(out["vals"]).all()             # the isolated agent: inv = 0 is never divided by
    out = ev.edge_values(pos[None], 0.5, sym)
    assert out["nnz"] == 0 and out["lam"][0] == 0.0 and len(out["vals"]) == 0 and out["steps"][0] == 0
    N = 41
    out = _check_against_eigvalsh(pos[:N], 1.0e6, sym)
    want = 1.0 if sym else N - 1.0
    assert abs(out["lam"][0] - want) <= 1e-12 * want and out["nnz"] == N * (N - 1)
    assert (ev.ulps32(out["vals"], np.float32((1.0 / (N - 1) if sym else 1.0) / want)) <= 1).all()


def test_unnormalised_values_need_no_eigenvalue():
    pos, radii = ev.case_positions(3, 70)
    out = ev.edge_values(pos, radii, False, normalize=False)
    assert (out["lam"] == 0).all() and (out["steps"] == 0).all() and (out["vals"] == 1).all() and out["nnz"] > 0


# ---- the restatement against closed forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(64, 64), (33, 63), (45, 46)])
def test_restatement_on_lattices_reaches_the_closed_forms(a, b):
    """the 4-neighbour grid under radius 1.2: lambda_max = 2 cos(pi / (a + 1)) + 2 cos(pi / (b + 1)); 1 under symmetric_norm"""
    pos = ev.lattice(a, b)
    out = ev.edge_values(pos, 1.2, False)
    assert out["nnz"] == 2 * (a * (b - 1) + b * (a - 1))
    want = ev.lattice_lambda(a, b)
    assert abs(out["lam"][0] - want) <= 1e-12 * want and 0 < out["steps"][0] < a * b, (out["lam"][0], want, out["steps"])
    assert (out["vals"] == np.float32(1.0 / out["lam"][0])).all()
    out = ev.edge_values(pos, 1.2, True)
    assert abs(out["lam"][0] - 1.0) <= 1e-12 and 0 < out["steps"][0] < a * b
    # a corner (degree 2) next to an edge cell (degree 3): 1 / sqrt(6)
    assert ev.ulps32(out["vals"][0], np.float32(np.sqrt(0.5) * np.sqrt(1.0 / 3.0) / out["lam"][0])) <= 1


@pytest.mark.parametrize("N", [2100, 4096])
def test_restatement_on_random_cells_of_a_wide_map(N):
    """distinct random cells of a 256 x 256 map at radius 7, beyond batched_gso's 2048 agents: 1 under symmetric_norm"""
    pos = ev.random_cells(N)
    out = ev.edge_values(pos, 7.0, True)
    print("random cells", N, "steps", out["steps"][0], "edges", out["nnz"])
    assert out["nnz"] > 2 * N                                                    # (about five neighbours per agent and more)
    # (the walk ends by its stopping rule, long before N steps; how many it takes depends on the cells drawn)
    assert abs(out["lam"][0] - 1.0) <= 1e-12 and 160 < out["steps"][0] < N // 4, (out["lam"][0], out["steps"])


# ---- the kernel itself, compiled for the host (tools/host_wave) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def values_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "gso_edge_values_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "gso_edge_values_check.cpp"), "-o", exe], check=True)
    return exe


def run_check(exe, tmp_path, arrays, B, N, cap, sym, normalize, lds_limit=128 * 1024):
    (tmp_path / "case.txt").write_text(ev.dump_case(arrays, B, N, cap, sym, normalize, lds_limit))
    run = subprocess.run([exe, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    return ev.parse_result(run.stdout)


def assert_values(got, want, lam_rtol=1e-12):
    assert got["rc"] == 0
    same = got["lam"] == want["lam"]
    assert (same | (np.abs(got["lam"] - want["lam"]) <= lam_rtol * np.abs(want["lam"]))).all(), (got["lam"], want["lam"])
    nnz = want["nnz"]
    assert len(got["vals"]) >= nnz and np.isnan(got["vals"][nnz:]).all()         # nothing behind the edges is written
    if nnz:
        assert (ev.ulps32(got["vals"][:nnz], want["vals"]) <= 1).all()


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "symmetric_norm"])
@pytest.mark.parametrize("B,N", [(1, 1), (3, 2), (3, 63), (1, 64), (3, 65), (3, 129), (2, 257), (1, 600)])
def test_host_kernel_equals_the_restatement(values_check, tmp_path, B, N, sym):
    """one thread per lane, per-instance radii (typical, edgeless, clique): lambda within 1e-12 relative (equal where the bits are
    equal), the values within one float32 ulp, with the tridiagonal matrix in LDS and - the plan of 4096 agents - in the workspace"""
    pos, radii = ev.case_positions(B, N)
    want = ev.edge_values(pos, radii, sym)
    if B >= 3:
        clique = 1.0 if sym else N - 1.0
        assert want["lam"][1] == 0 and abs(want["lam"][2] - clique) <= 1e-12 * clique
    for limit in (128 * 1024, 24 * N + 144 + 8):                                 # (the three vectors and the static 144 bytes alone)
        assert_values(run_check(values_check, tmp_path, want, B, N, want["nnz"] + 3, sym, 1, limit), want)


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "symmetric_norm"])
@pytest.mark.parametrize("N,side", [(150, 45), (300, 62)])
def test_host_kernel_on_scatters_without_a_planted_cluster(values_check, tmp_path, N, side, sym):
    """case_positions' instance 0 carries a clique of 65 agents, which owns the spectrum (lambda 64, or 1) up to some hundred
    agents; here the cells are a plain random scatter: the walk takes tens of steps and lambda is no round number"""
    pos = ev.random_cells(N, side, seed=3)
    want = ev.edge_values(pos, 7.0, sym)
    assert want["steps"][0] >= 16 and (sym or abs(want["lam"][0] - round(want["lam"][0])) > 1e-3), (want["steps"], want["lam"])
    for limit in (128 * 1024, 24 * N + 144 + 8):
        assert_values(run_check(values_check, tmp_path, want, 1, N, want["nnz"], sym, 1, limit), want)


def test_host_kernel_without_normalisation_and_beyond_the_capacity(values_check, tmp_path):
    B, N = 3, 129
    pos, radii = ev.case_positions(B, N)
    radii[1] = 7.0                                                               # (three instances with edges)
    for sym in (False, True):
        assert_values(run_check(values_check, tmp_path, ev.edge_values(pos, radii, sym, False), B, N, 1 << 16, sym, 0),
                      ev.edge_values(pos, radii, sym, False))
    assert (ev.edge_values(pos, radii, True, False)["vals"] < 1).any()           # (gso_kernel's expression: inv[i] inv[j] / 1)
    # a capacity inside instance 1: instance 0 is walked, the others are not (lambda 0, no value written)
    want = ev.edge_values(pos, radii, True)
    rp = want["rowptr"].reshape(B, N + 1)
    cap = int(rp[1, 0] + rp[1, -1]) // 2
    got = run_check(values_check, tmp_path, want, B, N, cap, 1, 1)
    assert got["rc"] == 0 and got["lam"][0] == pytest.approx(want["lam"][0], rel=1e-12) and (got["lam"][1:] == 0).all()
    n0 = int(rp[0, -1])
    assert (ev.ulps32(got["vals"][:n0], want["vals"][:n0]) <= 1).all() and np.isnan(got["vals"][n0:]).all() and len(got["vals"]) == cap
    got = run_check(values_check, tmp_path, want, B, N, 0, 1, 1)                 # cap == 0: no colidx, no vals
    assert got["rc"] == 0 and (got["lam"] == 0).all() and len(got["vals"]) == 0


# ---- the C entry points --------------------------------------------------------------------------------------------------------------
ENTRIES = ("magat_gso_edge_values_workspace_bytes", "magat_gso_edge_values")


def test_entry_points_are_declared_exported_and_bound_behind_abi_9():
    from magat_pathplanning_amd import _native as nat, build_native
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    assert "gso_edge_values.hip" in build_native.SOURCES
    lib = nat.lib()
    assert lib.magat_abi_version() == 9
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS and re.search(r"\b(int|size_t) %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None
    assert len(set(nat.FORMS.values())) == len(nat.FORMS) and len(set(nat.TAGS.values())) == len(nat.TAGS)
    c, ms = ctypes.c_longlong(-1), ctypes.c_double(-1)
    assert lib.magat_profile_read(34, ctypes.byref(c), ctypes.byref(ms)) != 0      # 34 stays refused
    # which graphs the bottleneck planners hand to the one-launch dense kernel (edges.gso()) instead of the CSR route: the query
    # answers as the entry itself does (MAGAT_ERR_UNSUPPORTED before it looks at a pointer)
    q = lib.magat_gnn_dense_supported
    assert "magat_gnn_dense_supported" in nat.EXPORTED_SYMBOLS and re.search(r"\bint magat_gnn_dense_supported\(", hdr)
    for N, G, F, K in ((1, 16, 16, 1), (128, 32, 32, 3), (20, 128, 64, 8), (129, 32, 32, 3), (0, 32, 32, 3), (20, 48, 32, 3),
                       (20, 32, 256, 3), (20, 32, 32, 9), (20, 32, 32, 0)):
        rc = lib.magat_gnn_forward_dense_f32(None, G, None, 0, None, None, None, F, 1, N, N, G, F, K, 1, None)
        assert q(N, G, F, K) == (0 if rc == -2 else 1) and rc != 0, (N, G, F, K, rc)
    assert q(128, 32, 32, 3) == 1 and q(129, 32, 32, 3) == 0


def test_workspace_size_and_refusals_without_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    size = lib.magat_gso_edge_values_workspace_bytes
    assert size(1, 4097) == 0 and size(0, 8) == 0 and size(8, 0) == 0 and size(-1, -1) == 0
    for B, N in ((1, 1), (3, 65), (128, 100), (8, 1000), (1, 4096), (8, 4096)):
        tri = B * (16 * max(N, 160) + 16)                                       # alpha [cap], beta [cap + 2], float64
        assert size(B, N) % 256 == 0 and tri <= size(B, N) < tri + 256
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    before = lib.magat_form_count(nat.FORMS["gso_edges"])

    def call(rowptr=p, colidx=p, nnz=p, cap=8, sym=0, normalize=1, lam=p, vals=p, ws=p, nbytes=1 << 30, B=2, N=70):
        return lib.magat_gso_edge_values(rowptr, colidx, nnz, cap, sym, normalize, lam, vals, ws, nbytes, B, N, None)

    # host dummies: a launch would not survive them - everything below is answered before one
    for k in ("rowptr", "colidx", "nnz", "lam", "vals"):
        assert call(**{k: None}) == -5, k
    assert call(rowptr=None, B=0) == -5 and call(vals=None, cap=-1) == -5 and call(nnz=None, N=5000) == -5      # NULL pointers first ...
    for kw in (dict(B=0), dict(N=0), dict(cap=-1), dict(N=0, ws=None), dict(B=0, N=5000)):
        assert call(**kw) == -1, kw                                               # ... then the sizes ...
    assert call(N=4097) == -2 and call(N=4097, ws=None) == -2                    # ... then the agent limit ...
    assert call(ws=None) == -3 and call(nbytes=1024) == -3                       # ... then the workspace
    assert call(ws=ctypes.c_void_p((p.value | 255) + 1 + 8)) == -3               # (not 256-byte aligned)
    assert lib.magat_form_count(nat.FORMS["gso_edges"]) == before                # nothing was launched


# ---- the Python surface --------------------------------------------------------------------------------------------------------------
def test_python_surface_on_cpu_tensors():
    import magat_pathplanning_amd as pkg
    from magat_pathplanning_amd._native import MagatNativeError
    from magat_pathplanning_amd.edges import GraphEdges
    from magat_pathplanning_amd.graphml import GraphFilterBatch
    from magat_pathplanning_amd.synthetic import make_config
    pos = torch.zeros(2, 5, 2, dtype=torch.int32)
    with pytest.raises(MagatNativeError, match="no CPU fallback"):
        pkg.batched_edges(pos, 7.0, values=True, symmetric_norm=True)
    plain = GraphEdges(pos, comm_radius=7.0)
    valued = GraphEdges(pos, comm_radius=7.0, values=True, symmetric_norm=True)
    assert not plain.valued and valued.valued and valued.symmetric_norm and not plain.symmetric_norm
    assert (valued.B, valued.N) == (2, 5) and valued.refresh() is valued
    with pytest.raises(ValueError, match="values=True"):
        plain.values()
    for edges in (plain, valued):
        with pytest.raises(ValueError, match="edge rule"):
            edges.structure(2)
    layer = GraphFilterBatch(8, 16, 3)
    with pytest.raises(TypeError, match="batched_gso"):
        layer.addGSO(plain)
    assert layer.S is None
    layer.addGSO(valued)
    assert layer.S is valued and layer.N == 5
    with pytest.raises(MagatNativeError, match="no CPU fallback"):
        layer(torch.zeros(2, 8, 5))
    import pickle
    assert pickle.loads(pickle.dumps(layer)).S is None                           # (streams and events do not travel)
    for cls, kw in ((pkg.DecentralPlannerNet, {}), (pkg.DecentralPlannerBottleneckNet, dict(bottleneckMode="BottomNeck_only")),
                    (pkg.DecentralPlannerBottleneckNet, dict(bottleneckMode="BottomNeck_skipConcat"))):
        net = cls(make_config(num_agents=5, device="cpu", CNN_mode="Default", **kw))
        with pytest.raises(TypeError, match="batched_gso"):
            net.addGSO(plain)
        assert net.S is None
    net = pkg.DecentralPlannerNet(make_config(num_agents=5, device="cpu", CNN_mode="Default")).eval()
    valued.structure = lambda rule=0: None                                       # (the device build: not on this machine)
    net.addGSO(valued)
    assert net.S is valued and not net.GFL[0].unit_values and pickle.loads(pickle.dumps(net)).S is None
    with pytest.raises(ValueError, match=r"2 instances x 5 agents, forward a batch of 3 x 5"):
        net._check_gso_shape(3, 5)
    with pytest.raises(ValueError, match=r"forward a batch of 2 x 4"):
        net._check_gso_shape(2, 4)
    net._check_gso_shape(2, 5)
    net.config.GSO_mode = "dist_GSO_one"
    net.addGSO(valued)
    assert net.S is valued and net.GFL[0].unit_values
    # evaluate_cases: the new graph name is accepted (the pool then asks for device tensors), an unknown one is not
    with pytest.raises(ValueError, match="graph"):
        pkg.evaluate_cases(None, None, None, None, 3, 1, 7.0, graph="dense")
    with pytest.raises(Exception) as info:
        pkg.evaluate_cases(None, None, None, None, 3, 1, 7.0, graph="valued_edges")
    assert "graph must be" not in str(info.value)
    import inspect
    for fn in (pkg.BatchedEpisode.edges, pkg.EpisodePool.edges):
        assert inspect.signature(fn).parameters["values"].default is False
    sig = inspect.signature(pkg.batched_edges).parameters
    assert sig["values"].default is False and sig["symmetric_norm"].default is False
