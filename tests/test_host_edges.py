"""CPU-only checks of the edge structure from agent positions (csrc/gso_edges.hip, magat_pathplanning_amd/edges.py): the numpy
restatement against the fixtures the real reference made, its own properties, the entry points' declaration / export / binding and
their refusals, the Python surface on CPU tensors, and the kernels themselves compiled for the host (tools/host_wave) against the
restatement."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import edges_restatement as er
from conftest import ROOT, golden_paths

SIM = golden_paths("sim_")
ARRAYS = ("rowptr", "colidx", "cscptr", "cscsrc", "cscpos")


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_there_are_eleven_reference_fixtures():
    assert len(SIM) == 11


@pytest.mark.parametrize("path", SIM, ids=[os.path.basename(p)[:-4] for p in SIM])
def test_pattern_equals_the_edge_test_of_the_reference_gso(path):
    """edges from positions are the edges addGSO finds in the simulator's GSO: |S| > 1e-9 of S and of its symmetric normalisation,
    in float64 and behind the dataloader's cast to float32"""
    z = np.load(path)
    A = er.edge_pattern(z["pos"], float(z["commR"]), 0)
    assert A.any()
    for key in ("S", "S_symnorm"):
        for dtype in (np.float64, np.float32):
            S = z[key].astype(dtype)
            assert np.array_equal(A, np.abs(S) > dtype(1e-9)), (key, dtype)
            eye = np.eye(S.shape[-1], dtype=np.float32)
            assert np.array_equal(er.edge_pattern(z["pos"], float(z["commR"]), 1), np.abs(S.astype(np.float32) + eye) > np.float32(1e-9))


@pytest.mark.parametrize("B,N", [(1, 1), (1, 2), (3, 65), (3, 129), (2, 300)])
def test_restatement_properties(B, N):
    pos, radii = er.case_positions(B, N)
    for rule in (0, 1):
        A = er.edge_pattern(pos, radii, rule)
        a = er.arrays_of_pattern(A)
        assert np.array_equal(A, A.transpose(0, 2, 1))                        # the graph is symmetric ...
        assert np.array_equal(a["cscptr"], a["rowptr"]) and np.array_equal(a["cscsrc"], a["colidx"])      # ... so is its column view
        rp = a["rowptr"].reshape(B, N + 1)
        assert a["nnz"] == int(A.sum()) == rp[-1, -1] and rp[0, 0] == 0 and (np.diff(rp, axis=1) >= 0).all()
        assert (rp[1:, 0] == rp[:-1, -1]).all()                               # absolute offsets: an instance starts where the last ended
        for b in range(B):
            for j in range(N):
                lo, hi = rp[b, j], rp[b, j + 1]
                assert (np.diff(a["colidx"][lo:hi]) > 0).all() and (np.diff(a["cscsrc"][lo:hi]) > 0).all()      # ascending
                assert np.array_equal(a["colidx"][lo:hi], np.nonzero(A[b, j])[0])
                # the in-edge i -> j stands in row i at the position cscpos names: there colidx is j
                assert (a["colidx"][a["cscpos"][lo:hi]] == j).all()
                src = a["cscsrc"][lo:hi]
                assert ((rp[b, src] <= a["cscpos"][lo:hi]) & (a["cscpos"][lo:hi] < rp[b, src + 1])).all()
        assert np.array_equal(np.diagonal(A, axis1=1, axis2=2), np.full((B, N), bool(rule)))
        for cap in (0, 1, a["nnz"] // 2, a["nnz"] + 3):                       # truncation keeps the first cap entries and the offsets
            t = er.arrays_of_pattern(A, cap)
            assert np.array_equal(t["rowptr"], a["rowptr"]) and t["nnz"] == a["nnz"]
            for k in ("colidx", "cscsrc", "cscpos"):
                assert np.array_equal(t[k], a[k][:cap])
    if B > 1:                                                                 # one radius per instance
        for b in range(B):
            assert np.array_equal(er.edge_pattern(pos, radii, 0)[b], er.edge_pattern(pos[b:b + 1], radii[b], 0)[0])
        assert not er.edge_pattern(pos, radii, 0)[B - 1].any() and er.edge_arrays(pos[B - 1:], 0.5, 0)["nnz"] == 0


def test_the_boundary_of_the_radius_is_strict():
    pos = np.array([[[0, 0], [3, 4], [0, 5], [6, 8]]])
    assert not er.edge_pattern(pos, 5.0)[0, 0, 1] and not er.edge_pattern(pos, 5.0)[0, 0, 2]      # distance 5 is not < 5
    assert er.edge_pattern(pos, np.nextafter(5.0, 6.0))[0, 0, 1] and er.edge_pattern(pos, 5.0)[0, 1, 2] and not er.edge_pattern(pos, 5.0)[0, 1, 3]
    assert not er.edge_pattern(pos, 10.0)[0, 0, 3] and er.edge_pattern(pos, 10.000001)[0, 0, 3]


# ---- the C entry points ----------------------------------------------------------------------------------------------------------------
ENTRIES = ("magat_gso_edges_workspace_bytes", "magat_gso_edges_build")


def test_entry_points_are_declared_exported_and_bound_behind_abi_9():
    from magat_pathplanning_amd import _native as nat, build_native
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert "gso_edges.hip" in build_native.SOURCES
    lib = nat.lib()
    assert lib.magat_abi_version() == 9
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS and re.search(r"\b(int|size_t) %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None
    tag = int(re.search(r"#define MAGAT_TAG_GSO_EDGES (\d+)", common).group(1))
    form = int(re.search(r"#define MAGAT_FORM_GSO_EDGES (\d+)", common).group(1))
    assert tag == nat.TAG_GSO_EDGES == 35 and nat.TAGS[tag] == "gso_edges" and form == nat.FORMS["gso_edges"] == 26
    assert len(set(nat.FORMS.values())) == len(nat.FORMS) and len(set(nat.TAGS.values())) == len(nat.TAGS)
    assert re.search(r"#define MAGAT_PROF_TAGS 26\b", hdr) and re.search(r"#define MAGAT_FORMS 16\b", hdr)      # ABI 9's public counts
    c, ms = ctypes.c_longlong(-1), ctypes.c_double(-1)
    assert lib.magat_profile_read(tag, ctypes.byref(c), ctypes.byref(ms)) == 0 and c.value >= 0
    assert lib.magat_profile_read(tag - 1, ctypes.byref(c), ctypes.byref(ms)) != 0      # 34 stays unassigned
    assert lib.magat_form_count(form) >= 0      # (what lies behind this tag and form is not pinned here: the next entry takes them)


def test_workspace_size_and_refusals_without_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    size = lib.magat_gso_edges_workspace_bytes
    assert size(1, 4097) == 0 and size(0, 8) == 0 and size(8, 0) == 0 and size(-1, -1) == 0
    for B, N in ((1, 1), (3, 65), (128, 1000), (1, 4096), (8, 4096)):
        words = B * N * ((N + 63) // 64)
        assert size(B, N) % 256 == 0 and size(B, N) >= words * 10 + B * N * 4      # bit matrix, word prefixes, row degrees
        assert size(B, N) <= words * 10 + B * N * 4 + B * ((N + 15) // 16) * 4 + 4 * 256      # ... and the chunk totals, no more
    assert size(1, 4096) < 3 << 20 and size(128, 1000) < 22 << 20
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    before = lib.magat_form_count(nat.FORMS["gso_edges"])

    def call(pos=p, radii=p, R=0.0, rule=0, rowptr=p, colidx=p, cscptr=p, cscsrc=p, cscpos=p, cap=8, nnz=p, ws=p, nbytes=1 << 30, B=2, N=70):
        return lib.magat_gso_edges_build(pos, radii, R, rule, rowptr, colidx, cscptr, cscsrc, cscpos, cap, nnz, ws, nbytes, B, N, None)

    # host dummies: a launch would not survive them - everything below is answered before one
    for k in ("pos", "rowptr", "cscptr", "nnz", "colidx", "cscsrc", "cscpos"):
        assert call(**{k: None}) == -5, k
    assert call(pos=None, B=0) == -5 and call(cscpos=None, cap=-1) == -5 and call(nnz=None, N=5000) == -5      # NULL pointers first ...
    for kw in (dict(B=0), dict(N=0), dict(cap=-1), dict(rule=2), dict(rule=-1), dict(radii=None), dict(radii=None, R=-2.0),
               dict(radii=None, R=float("nan")), dict(N=0, ws=None), dict(B=0, N=5000)):
        assert call(**kw) == -1, kw                                            # ... then the sizes ...
    assert call(N=4097) == -2 and call(N=4097, ws=None) == -2                 # ... then the agent limit ...
    assert call(ws=None) == -3 and call(nbytes=1024) == -3                    # ... then the workspace
    assert call(ws=ctypes.c_void_p((p.value | 255) + 1 + 8)) == -3            # (not 256-byte aligned)
    assert lib.magat_form_count(nat.FORMS["gso_edges"]) == before             # nothing was launched


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses_cpu_tensors_wrong_shapes_and_the_gnn_classes():
    import magat_pathplanning_amd as pkg
    from magat_pathplanning_amd import simulator
    from magat_pathplanning_amd._native import MagatNativeError
    from magat_pathplanning_amd.edges import GraphEdges
    from magat_pathplanning_amd.synthetic import make_config
    for name in ("batched_edges", "GraphEdges"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(simulator, name)
    pos = torch.zeros(2, 5, 2, dtype=torch.int32)
    with pytest.raises(MagatNativeError, match="no CPU fallback"):
        pkg.batched_edges(pos, 7.0)
    for bad in (pos[0], pos[:, :, :1], torch.zeros(2, 0, 2, dtype=torch.int32), [[0, 0]]):
        with pytest.raises(ValueError, match=r"\(B,N,2\)"):
            pkg.batched_edges(bad, 7.0)
    with pytest.raises(MagatNativeError, match="4096"):
        pkg.batched_edges(torch.zeros(1, 4097, 2, dtype=torch.int32), 7.0)
    edges = GraphEdges(pos, comm_radius=7.0)                                   # (the class itself holds what it is given)
    assert (edges.B, edges.N) == (2, 5) and edges.refresh() is edges
    with pytest.raises(ValueError, match="edge rule"):
        edges.structure(2)
    for cls, kw in ((pkg.DecentralPlannerNet, {}), (pkg.DecentralPlannerBottleneckNet, dict(bottleneckMode="BottomNeck_skipConcat"))):
        net = cls(make_config(num_agents=5, device="cpu", CNN_mode="Default", **kw))
        with pytest.raises(TypeError, match="batched_gso"):
            net.addGSO(edges)
        assert net.S is None
    with pytest.raises(ValueError, match="graph"):
        pkg.evaluate_cases(None, None, None, None, 3, 1, 7.0, graph="dense")
    assert callable(pkg.BatchedEpisode.edges) and callable(pkg.EpisodePool.edges)


def test_a_tensor_still_takes_the_tensor_path_and_drops_the_edges():
    """addGSO(tensor) behaves as before in DecentralPlannerGATNet, also behind an addGSO(edges) that was never forwarded"""
    import pickle
    from magat_pathplanning_amd import DecentralPlannerGATNet
    from magat_pathplanning_amd.edges import GraphEdges
    from magat_pathplanning_amd.synthetic import comm_gso, make_config
    net = DecentralPlannerGATNet(make_config(num_agents=5, device="cpu", CNN_mode="Default")).eval()
    edges = GraphEdges(torch.zeros(2, 5, 2, dtype=torch.int32), comm_radius=7.0)
    net._edges = net.S = edges                                                 # what addGSO(edges) leaves on the CSR route
    assert pickle.loads(pickle.dumps(net))._edges is None and pickle.loads(pickle.dumps(net)).S is None
    S = comm_gso(2, 5, 12)
    net.addGSO(S)
    assert net._edges is None and torch.is_tensor(net.S) and tuple(net.S.shape) == (2, 1, 5, 5)
    # autograd switched on behind an addGSO(edges) that chose the CSR route: the training forward takes edges.dense() through the
    # tensor path (here a stand-in for the device build: the adjacency of the GSO above)
    from magat_pathplanning_amd.synthetic import fov_states
    x = fov_states(2, 5, seed=3)
    net.train()
    want = net(x)
    edges.dense = lambda dtype=torch.float32: (S != 0).to(dtype)
    net._edges = net.S = edges
    got = net(x)
    assert got.requires_grad and net._edges is None and torch.is_tensor(net.S) and torch.equal(net.S[:, 0], (S != 0).float())
    assert torch.equal(got, want)                                              # the composite reads the edge test only


# ---- the kernels themselves, compiled for the host (tools/host_wave) -----------------------------------------------------------------
@pytest.fixture(scope="module")
def edges_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "gso_edges_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "gso_edges_check.cpp"), "-o", exe], check=True)
    return exe


def run_check(exe, tmp_path, pos, radii, rule, cap):
    (tmp_path / "case.txt").write_text(er.dump_case(pos, radii, rule, cap))
    run = subprocess.run([exe, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    return er.parse_result(run.stdout)


@pytest.mark.parametrize("B,N", [(1, 1), (3, 2), (3, 63), (1, 64), (3, 65), (1, 128), (3, 129), (1, 200)])
def test_host_kernels_equal_the_restatement(edges_check, tmp_path, B, N):
    """the two kernels, one thread per lane: all five arrays and the count for both rules, per-instance radii (the clique and the
    edgeless instance of case_positions), then a capacity below the count and cap == 0 without index arrays.  (Batches that take
    64 rows per workgroup cost the host form a quarter of a minute: tests/test_gpu_edges.py runs them on the device.)"""
    pos, radii = er.case_positions(B, N)
    for rule in (0, 1):
        want = er.edge_arrays(pos, radii, rule)
        got = run_check(edges_check, tmp_path, pos, radii, rule, want["nnz"] + 3)
        assert got["rc"] == 0 and got["nnz"] == want["nnz"]
        for k in ARRAYS:
            assert np.array_equal(got[k], want[k]), (rule, k)
    for cap in (want["nnz"] // 2, 0):
        got = run_check(edges_check, tmp_path, pos, radii, 1, cap)
        assert got["rc"] == 0 and got["nnz"] == want["nnz"]
        for k in ARRAYS:
            assert np.array_equal(got[k], want[k] if k.endswith("ptr") else want[k][:cap]), (cap, k)
    if B == 1:                                                                 # one radius as the entry's number
        got = run_check(edges_check, tmp_path, pos, float(radii[0]), 0, 1 << 16)
        assert np.array_equal(got["colidx"], er.edge_arrays(pos, radii, 0)["colidx"])


def test_host_kernels_take_cells_anywhere_in_int32(edges_check, tmp_path):
    """coordinates beyond +-16383 leave the 32-bit distance test: the same edges, shifted and at the corners of int32"""
    pos, radii = er.case_positions(2, 70)
    want = er.edge_arrays(pos, radii, 0)
    far = pos.astype(np.int64) + np.array([2 ** 31 - 200, -2 ** 31 + 3])
    got = run_check(edges_check, tmp_path, far, radii, 0, want["nnz"])
    assert got["nnz"] == want["nnz"] and np.array_equal(got["colidx"], want["colidx"]) and np.array_equal(got["cscpos"], want["cscpos"])
    corners = np.array([[[-2 ** 31, -2 ** 31], [2 ** 31 - 1, 2 ** 31 - 1], [-2 ** 31, -2 ** 31 + 3], [2 ** 31 - 1, -2 ** 31]]])
    got = run_check(edges_check, tmp_path, corners, 5.0, 0, 16)
    assert got["nnz"] == 2 and got["colidx"].tolist() == [2, 0]              # only the two cells three apart
