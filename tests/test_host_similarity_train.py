"""CPU-only: the training path of attentionMode 'GAT_Similarity' on the HIP kernels (hip_backward=True, _GatCosTrainFunction,
magat_gat_train_forward_cos_f32 / magat_gat_train_backward_cos_f32).  The backward rule the kernels implement - restated with
torch ops in tests/similarity_train_cases.py - against autograd of the float64 composite; the composite against two
reference-made gradient fixtures at widths the kernels take; the properties of the inputs the device test relies on; the float32
composite's own error; the entry points and their refusals; and the new kernel itself compiled for the host
(tools/host_wave/gat_cos_check.cpp) against the restatement."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import similarity_train_cases as sc
from conftest import ROOT, golden_paths, load_layer_fixture

COSGRAD = golden_paths("cosgrad_")
CIDS = list(sc.CASES)


def test_case_list_covers_the_issue_matrix():
    shapes = {(k.group, k.B, k.N, k.G, k.K, k.concat, k.nin) for k in sc.CASES.values()}
    for want in [("rounds", 9, 10, 32, 3, True, 10), ("rounds", 17, 10, 32, 3, False, 10), ("long", 2, 130, 64, 3, True, 130),
                 ("long", 1, 70, 64, 3, False, 70), ("wide", 2, 300, 32, 2, True, 300), ("width", 3, 21, 16, 3, True, 21),
                 ("width", 3, 21, 128, 3, False, 21), ("width", 3, 21, 256, 2, True, 21), ("depth", 3, 12, 32, 5, True, 12),
                 ("depth", 3, 12, 32, 1, False, 12), ("clamp", 3, 12, 32, 3, True, 12), ("clamp", 3, 12, 32, 3, False, 10)]:
        assert want in shapes, want
    assert sum(k.group == "edgeless" for k in sc.CASES.values()) == 3


@pytest.mark.parametrize("cid", CIDS)
def test_closed_form_matches_autograd_of_the_float64_composite(cid):
    """The restated rule (no autograd) against autograd of the float64 composite: 1e-9 of max(1, max|want|) per tensor, the clamped
    rows of dx relative to their own largest entry.  The clamp of this torch is invisible to autograd; another torch shows here."""
    r = sc.reference(cid)
    got = sc.restated_result(r.case, r)
    assert r.want["mixer"] is None and r.want["weight_bias"] is None
    sc.compare(cid, got, r.want, r.clamped, gate=1e-9)
    if r.case.K == 1:
        assert r.want["weight"] is None or not r.want["weight"].any()


def test_fixture_set():
    assert [os.path.basename(p) for p in COSGRAD] == ["cosgrad_N12_G32_K2.npz", "cosgrad_N7_G16_K3.npz"]
    for path in COSGRAD:
        assert os.path.getsize(path) < 1 << 20
        z, p = load_layer_fixture(path)
        norms = np.linalg.norm(z["x"], axis=1)
        assert (norms == 0).any() and ((norms > 0) & (norms < 1e-9)).any()
        assert z["x"].dtype == np.float64 and np.array_equal(z["x"], z["x"].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("path", COSGRAD, ids=[os.path.basename(p)[:-4] for p in COSGRAD])
def test_composite_gradients_match_reference_made_gradients(path):
    """float64 composite on the CPU against the reference's autograd, by the rule of the test of the same name in
    test_host_similarity.py (1e-6: outputs to tol * max(1, |y|), gradients to tol * (10 |g| + 1e-2 max |g|)); None where the
    reference has None."""
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    z, p = load_layer_fixture(path)
    G, K, tol = int(z["G"]), int(z["K"]), 1e-6
    layer = GraphFilterBatchSimilarityAttentional(G, G, K, 1)
    layer.load_state_dict(p, strict=True)
    layer = layer.double()
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    layer.addGSO(torch.from_numpy(z["S"]))
    y = layer(x)
    (y * torch.from_numpy(z["wgt"])).sum().backward()
    np.testing.assert_allclose(y.detach().numpy(), z["y"], rtol=0, atol=tol * max(1.0, float(np.abs(z["y"]).max())))
    grads = {"dx": x.grad}
    grads.update({"g_" + k: v.grad for k, v in layer.named_parameters()})
    none = set(str(z["none_grads"]).split(","))
    assert none == {"mixer", "weight_bias"}
    gmax = max(float(np.abs(z[k]).max()) for k in z.files if k == "dx" or k.startswith("g_"))
    for k, g in grads.items():
        if k[2:] in none and k != "dx":
            assert g is None, k
            continue
        want = z[k]
        np.testing.assert_allclose(g.numpy(), want, rtol=0, atol=tol * (10 * float(np.abs(want).max()) + 1e-2 * gmax), err_msg=k)


@pytest.mark.parametrize("cid", CIDS)
def test_inputs_keep_the_properties_they_were_made_for(cid):
    """A condition on the inputs: every number is a float32 value; every |x_m| and |q_m| (float64) is exactly 0, at most 1e-11 or
    at least 1e-6 - float32 and float64 agree on which rows are clamped; the graphs reach their branch; the clamp case holds a
    zero row and a tiny row that have edges and are someone's neighbour."""
    r = sc.reference(cid)
    k = r.case
    for t in [r.x, r.wgt] + list(r.state.values()):
        assert t.dtype == torch.float32
    assert torch.equal(r.S, r.S.float().double())
    X, Q = sc.rows_and_maps(k, r)
    for n in (X.norm(dim=2), Q.norm(dim=2)):
        assert bool(((n == 0) | (n <= 1e-11) | (n >= 1e-6)).all()), cid
        n32 = n.float()      # (what a float32 norm rounds to decides the same way)
        assert torch.equal(n32 < 1e-9, n < 1e-9)
    assert r.row_deg >= k.row_deg and r.col_deg >= k.col_deg, (r.row_deg, r.col_deg)
    M = sc.edge_mask(r.S)
    off = M & ~torch.eye(k.N, dtype=torch.bool)
    if k.gso is sc.tg.gso_edgeless:
        assert not off.any() and bool(M.diagonal(dim1=1, dim2=2).all())
    if k.gso is sc.tg.gso_first_edgeless:
        assert not off[0].any() and off[1].any()
    if k.gso is sc.gso_no_edge_row:
        assert not M[0, 4].any() and M[0, :, 4].any() and not M[1, 2, 2] and M[1, 2].any()
    if k.clamp:
        nx = X.norm(dim=2)
        (bz, iz), (bt, it) = sc.ZERO_ROW, sc.TINY_ROW
        assert nx[bz, iz] == 0 and 0 < nx[bt, it] <= 1e-11
        for b, i in (sc.ZERO_ROW, sc.TINY_ROW):
            assert off[b, i].any() and off[b, :, i].any(), "has edges and is someone's neighbour"
        assert int(r.clamped.sum()) == 2
    elif k.nin != k.N:
        assert not r.clamped.any() and bool((X[:, k.nin:] == 0).all())
    else:
        assert not r.clamped.any()


def test_float32_composite_error_stays_far_from_the_gate():
    """The float32 composite against the float64 one, per case, on the CPU: the rounding the device path may show as well.  It must
    stay under a tenth of the gate of the device test (2e-4) in every case - else the case is to be made milder."""
    worst = (0.0, None)
    for cid in CIDS:
        r = sc.reference(cid)
        got = sc.composite_result(r.case, r, torch.float32)
        err = sc.compare(cid, got, r.want, r.clamped, gate=sc.GATE / 10)
        worst = max(worst, (err, cid))
    print("float32 composite against float64, worst over all cases: %.2e (%s)" % worst)


def test_layer_keyword_attribute_and_model_key():
    from magat_pathplanning_amd import DecentralPlannerGATNet, GraphFilterBatchSimilarityAttentional
    from magat_pathplanning_amd import graphml
    from magat_pathplanning_amd.synthetic import make_config
    assert GraphFilterBatchSimilarityAttentional(16, 16, 2, 1).hip_backward is False
    layer = GraphFilterBatchSimilarityAttentional(16, 16, 2, 1, 1, True, torch.relu, True, "GAT_Similarity", hip_backward=True)
    assert layer.hip_backward is True and "hip_backward" not in layer.state_dict()
    assert issubclass(graphml._GatCosTrainFunction, torch.autograd.Function)
    # CPU tensors keep the composite, with or without the keyword: the same numbers
    k = sc.CASES["clamp-cat-rounds-B3N12G32K3-tiny"]
    r = sc.reference(k.id)
    layer = sc.make_layer(k, r.state, hip_backward=True)
    layer.addGSO(r.S.unsqueeze(1))
    x = r.x.clone().requires_grad_(True)
    y = layer(x)
    assert type(y.grad_fn).__name__ != "_GatCosTrainFunctionBackward"
    plain = sc.make_layer(k, r.state)
    plain.addGSO(r.S.unsqueeze(1))
    assert torch.equal(y, plain(r.x))
    for key, want in ((None, False), (True, True), (False, False)):
        kw = {} if key is None else {"gat_hip_backward": key}
        net = DecentralPlannerGATNet(make_config(num_agents=5, attentionMode="GAT_Similarity", nAttentionHeads=1, device="cpu", **kw))
        assert net.GFL[0].hip_backward is want
    net = DecentralPlannerGATNet(make_config(num_agents=5, attentionMode="KeyQuery", device="cpu", gat_hip_backward=True))
    assert not hasattr(net.GFL[0], "hip_backward")


def test_entry_points_are_bound_and_refuse_in_the_documented_order():
    from magat_pathplanning_amd import _native as nat
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert int(re.search(r"#define MAGAT_FORMS (\d+)", hdr).group(1)) == 16
    assert int(re.search(r"#define MAGAT_FORM_GAT_COS_TRAIN (\d+)", common).group(1)) == nat.FORMS["gat_cos_train"] == 25
    assert int(re.search(r"#define MAGAT_FORMS_TABLE (\d+)", common).group(1)) == 26
    assert int(re.search(r"#define MAGAT_FORMS_ALL (\d+)", common).group(1)) == 19
    for name in ("magat_gat_train_forward_cos_f32", "magat_gat_train_backward_cos_f32"):
        assert name in nat.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % name, hdr), name
    lib = nat.lib()
    assert lib.magat_abi_version() == 9
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    B, N, G, K = 3, 20, 32, 3
    before = lib.magat_form_count(nat.FORMS["gat_cos_train"])

    def fwd(X=p, colidx=p, nnz=50, T=p, Xhat=p, norms=p, csctmp=p, B=B, N=N, G=G, K=K):
        return lib.magat_gat_train_forward_cos_f32(X, p, colidx, nnz, p, None, p, p, p, T, Xhat, norms, p, p, p, csctmp, B, N, G, K, None)

    def bwd(dY=p, colidx=p, nnz=50, T=p, norms=p, datt=p, B=B, N=N, G=G, K=K):
        return lib.magat_gat_train_backward_cos_f32(dY, p, p, p, T, norms, p, colidx, p, p, p, nnz, p, p, datt, B, N, G, K, None)

    # host dummies: a launch would not survive them - everything below is answered before one
    for call in (fwd, bwd):
        assert call(norms=None) == -5 and call(colidx=None) == -5 and call(T=None) == -5      # NULL pointers first ...
        assert call(norms=None, B=0) == -5 and call(T=None, G=8) == -5
        assert call(B=0) == -1 and call(N=0) == -1 and call(K=0) == -1 and call(nnz=-1) == -1      # ... then the sizes ...
        assert call(B=0, G=8) == -1 and call(K=0, N=8191) == -1
        for g in (8, 24, 48, 512):
            assert call(G=g) == -2, g                                                            # ... then width and N ...
        assert call(N=8191) == -2 and call(N=8191, B=1 << 30) == -2
        assert call(B=1 << 30, N=8190) == -1                                                     # ... then the 2^31 - 1 limits
    assert fwd(X=None) == -5 and fwd(Xhat=None) == -5 and fwd(csctmp=None) == -5
    assert bwd(dY=None) == -5 and bwd(datt=None) == -5
    assert bwd(T=None, K=2, B=0) == -1      # (T is not needed up to K = 2)
    assert lib.magat_form_count(nat.FORMS["gat_cos_train"]) == before      # a refused call counts nothing
    # the existing pair keeps refusing the mode
    assert lib.magat_gat_train_forward_f32(p, p, p, 50, p, None, p, p, p, p, p, p, p, p, B, N, G, G, K, 1, 4, None) == -2
    assert lib.magat_gat_train_backward_f32(p, p, p, p, p, p, p, p, p, p, 50, p, p, p, B, N, G, G, K, 1, 4, None) == -2


# ---- the normalisation-backward kernel, compiled for the host (tools/host_wave) ------------------------------------------------
@pytest.fixture(scope="module")
def cos_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "gat_cos_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "gat_cos_check.cpp"), "-o", exe], check=True)
    return exe


def write_cos_case(path, G, M, K, blocks, seed):
    """A case of gat_cos_check: normalised rows as the forward leaves them (a zero row, a tiny row), random incoming gradients.
    Returns the arrays."""
    g = torch.Generator().manual_seed(seed)
    NC = G + K * G
    v = torch.randn(2, M, G, generator=g) * 0.6
    v[0, 1] = 0.0
    v[1, 1] = 0.0
    v[0, M - 2] *= 1e-12
    v[1, M - 2] *= 1e-12
    n = v.double().norm(dim=2).float()
    vh = (v / n.clamp_min(1e-9).unsqueeze(2)).float()
    Z = torch.randn(M, NC, generator=g)
    Z[:, :G] = vh[1]
    dXd, dZ = torch.randn(M, G, generator=g), torch.randn(M, NC, generator=g)
    arrays = [vh[0].contiguous(), Z, n.contiguous(), dXd, dZ]
    with open(path, "w") as f:
        f.write("%d %d %d 0 %d\n" % (G, M, NC, blocks))
        for a in arrays:
            f.write(" ".join(map(str, a.numpy().view(np.uint32).reshape(-1).tolist())) + "\n")
    return vh, Z, n, dXd, dZ


@pytest.mark.parametrize("G,M,blocks", [(16, 150, 2), (256, 11, 2), (64, 37, 1)])
def test_normalisation_backward_kernel_on_the_host(cos_check, tmp_path, G, M, blocks):
    """gat_cos_backward_kernel, thread-emulated: G = 16 (sixteen rows per wave, masked rows in the last wave) and G = 256 (a wave
    per row), M no multiple of the rows per workgroup, more rows than one grid pass, a zero row and a tiny row - dXd and the
    score columns of dZ against the restatement's rule in float64 (2e-6 of each row's largest entry: float32 rounding of a G-term
    dot product), everything else in dZ untouched."""
    K = 2
    vh, Z, n, dXd, dZ = write_cos_case(str(tmp_path / "case.txt"), G, M, K, blocks, seed=G + M)
    assert M % (1024 // G) != 0 and (n[0] == 0).any() and ((n[0] > 0) & (n[0] < 1e-9)).any()
    run = subprocess.run([cos_check, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 2
    got_dx = torch.from_numpy(np.array(lines[0].split(), dtype=np.uint32).view(np.float32).reshape(M, G).copy())
    got_dz = torch.from_numpy(np.array(lines[1].split(), dtype=np.uint32).view(np.float32).reshape(M, G + K * G).copy())
    assert torch.equal(got_dz[:, G:], dZ[:, G:])
    for got, dvh, h, nn in ((got_dx, dXd, vh[0], n[0]), (got_dz[:, :G], dZ[:, :G], vh[1], n[1])):
        want = sc.norm_backward(dvh.double(), h.double(), nn.double())
        scale = want.abs().amax(dim=1, keepdim=True)
        assert bool((scale > 0).all())
        err = float(((got.double() - want).abs() / scale).max())
        print("G = %d: worst error / row maximum %.2e" % (G, err))
        assert err <= 2e-6, err
        assert float(want[1].abs().max()) > 1e8      # the zero row: dv = dv^ 1e9
