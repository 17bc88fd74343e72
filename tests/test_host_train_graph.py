"""CPU-only checks around the training kernels of the graph layers: the argument checks of magat_gat_train_forward_f32,
magat_gat_train_backward_f32 and magat_gnn_backward_csr_f32 answer before anything touches a device, and the inputs of
tests/test_gpu_train_graph_shapes.py (tests/train_graph_cases.py) keep the shape properties they were made for."""
import ctypes

import pytest
import torch

import train_graph_cases as tg

ERR_NULL, BAD_SHAPE, UNSUPPORTED = -5, -1, -2
ONE = ctypes.c_void_p(16)          # a non-null pointer no refused call may dereference
HUGE_B = 1 << 20                   # instances whose rows (x N = 8190) no int counts: a refusal BEHIND the limits, before any launch


def _lib():
    from magat_pathplanning_amd import _native as nat
    return nat.lib()


def _forward(X=ONE, rowptr=ONE, colidx=ONE, nnz=8, packed=ONE, bias=ONE, Ypre=ONE, att=ONE, Z=ONE, T=ONE, cscptr=ONE,
             cscsrc=ONE, cscpos=ONE, csctmp=ONE, B=2, N=8, G=32, F=32, K=3, P=2, mode=0):
    return _lib().magat_gat_train_forward_f32(X, rowptr, colidx, nnz, packed, bias, Ypre, att, Z, T, cscptr, cscsrc, cscpos,
                                              csctmp, B, N, G, F, K, P, mode, None)


def _backward(dYpre=ONE, X=ONE, Z=ONE, att=ONE, T=ONE, rowptr=ONE, colidx=ONE, cscptr=ONE, cscsrc=ONE, cscpos=ONE, nnz=8,
              dZ=ONE, dXd=ONE, datt=ONE, B=2, N=8, G=32, F=32, K=3, P=2, mode=0):
    return _lib().magat_gat_train_backward_f32(dYpre, X, Z, att, T, rowptr, colidx, cscptr, cscsrc, cscpos, nnz, dZ, dXd, datt,
                                               B, N, G, F, K, P, mode, None)


def _gnn_backward(dY=ONE, rowptr=ONE, colidx=ONE, vals=ONE, nnz=8, dZ=ONE, B=2, N=8, F=32, K=3):
    return _lib().magat_gnn_backward_csr_f32(dY, rowptr, colidx, vals, nnz, dZ, B, N, F, K, None)


def test_train_forward_argument_checks_answer_before_anything_touches_a_device():
    f = _forward
    for name in ("X", "rowptr", "colidx", "packed", "Ypre", "att", "Z", "T", "cscptr", "cscsrc", "cscpos", "csctmp"):
        assert f(**{name: None}) == ERR_NULL, name
    for name in ("B", "N", "K", "P"):
        assert f(**{name: 0}) == BAD_SHAPE and f(**{name: -3}) == BAD_SHAPE, name
    assert f(nnz=-1) == BAD_SHAPE
    assert f(G=32, F=64) == UNSUPPORTED and f(G=48, F=48) == UNSUPPORTED
    assert f(mode=-1) == UNSUPPORTED and f(mode=3) == UNSUPPORTED          # (3: MAGAT_MODE_GNN has its own entries)
    # null, then sizes, then what the kernels do not cover
    assert f(X=None, B=0, G=48) == ERR_NULL and f(B=0, G=48, F=48) == BAD_SHAPE
    # (2 N + 2) * 4 bytes of LDS in the transpose: N = 8191 is the first over 64 KiB.  N = 8190 gets past that check - shown by
    # the refusal behind it (more rows than the maps GEMM's int row count holds), which N = 8191 never reaches
    assert f(N=8191) == UNSUPPORTED and f(N=8191, B=HUGE_B) == UNSUPPORTED
    assert f(N=8190, B=HUGE_B) == BAD_SHAPE
    assert f(N=16, B=1 << 26, P=8) == BAD_SHAPE          # rows fit an int, the hop grid (B x P x N / 4 workgroups) does not
    # pointers a shape does not use may be null: no edges -> no colidx, K <= 2 -> no T  (again up to the last refusal)
    assert f(colidx=None, nnz=0, N=8190, B=HUGE_B) == BAD_SHAPE and f(T=None, K=2, N=8190, B=HUGE_B) == BAD_SHAPE


def test_train_backward_argument_checks_answer_before_anything_touches_a_device():
    f = _backward
    for name in ("dYpre", "X", "Z", "att", "T", "rowptr", "colidx", "cscptr", "cscsrc", "cscpos", "dZ", "dXd", "datt"):
        assert f(**{name: None}) == ERR_NULL, name
    for name in ("B", "N", "K", "P"):
        assert f(**{name: 0}) == BAD_SHAPE and f(**{name: -3}) == BAD_SHAPE, name
    assert f(nnz=-1) == BAD_SHAPE
    assert f(G=32, F=64) == UNSUPPORTED and f(G=48, F=48) == UNSUPPORTED
    assert f(mode=-1) == UNSUPPORTED and f(mode=3) == UNSUPPORTED
    assert f(dZ=None, B=0, G=48) == ERR_NULL and f(B=0, G=48, F=48) == BAD_SHAPE
    # the backward has no transpose and with it no limit on N; a supported call ends at the refusal behind the width checks:
    # a hop grid (B x P x N / 4 workgroups) past 2^31, answered before the memsets and the seed launch
    assert f(N=8191, B=HUGE_B) == BAD_SHAPE and f(N=8191, B=HUGE_B, G=48, F=48) == UNSUPPORTED
    assert f(colidx=None, nnz=0, N=8191, B=HUGE_B) == BAD_SHAPE and f(T=None, K=2, N=8191, B=HUGE_B) == BAD_SHAPE


def test_gnn_backward_argument_checks_answer_before_anything_touches_a_device():
    f = _gnn_backward
    for name in ("dY", "rowptr", "colidx", "vals", "dZ"):
        assert f(**{name: None}) == ERR_NULL, name
    for name in ("B", "N", "K"):
        assert f(**{name: 0}) == BAD_SHAPE and f(**{name: -3}) == BAD_SHAPE, name
    assert f(nnz=-1) == BAD_SHAPE
    assert f(F=48) == UNSUPPORTED and f(F=0) == UNSUPPORTED
    assert f(dY=None, B=0, F=48) == ERR_NULL and f(B=0, F=48) == BAD_SHAPE
    # supported widths end at the refusal behind the width check (a hop grid past 2^31), before the seed launch
    for F in (16, 32, 64, 128, 256):
        assert f(F=F, N=8191, B=HUGE_B) == BAD_SHAPE, F
    assert f(F=48, N=8191, B=HUGE_B) == UNSUPPORTED
    assert f(colidx=None, vals=None, nnz=0, N=8191, B=HUGE_B) == BAD_SHAPE


@pytest.mark.parametrize("cid", list(tg.GAT_CASES))
def test_gat_case_inputs_keep_their_shape_property(cid):
    """The float64 composite alone on every attention input: finite everywhere, the long rows / columns a case was made for
    are there under the layer's own edge rule, and where a wrong instance index has to show, no two instances agree."""
    r = tg.gat_reference(cid)
    k = r.case
    assert r.row_deg >= k.row_deg and r.col_deg >= k.col_deg, (r.row_deg, r.col_deg)
    if k.group == "long":           # (the figures of the case list, spelled out: more than two strides / more than one)
        assert min(r.row_deg, r.col_deg) > (128 if k.N == 130 else 64)
    if k.group == "wide":
        assert k.N > 256 and r.col_deg > 64
        m = r.S.abs() > 1e-9
        assert not m[:, 5, :].any() and not m[:, :, 5].any() and not m[:, :, 9].any() and m[:, 9, :].any()
    if k.gso is tg.gso_edgeless:
        assert r.row_deg == (1 if k.mode == tg.GO else 0)
    if k.gso is tg.gso_first_edgeless:
        assert not r.S[0].any() and r.S[1].any()
    assert r.want["y"].shape == (k.B, k.P * k.G if k.concat else k.G, k.nin) and r.want["dx"].shape == (k.B, k.G, k.nin)
    for name, t in r.want.items():
        assert torch.isfinite(t).all(), name
    for name in tg.used_names(k):
        if k.gso is not tg.gso_edgeless or name in ("filterWeight", "bias"):
            assert float(r.want[name].abs().max()) > 0, name
    if k.distinct:
        dx = r.want["dx"]
        for a in range(k.B):
            for b in range(a + 1, k.B):
                assert not torch.equal(dx[a], dx[b]) and not torch.equal(r.S[a], r.S[b]), (a, b)
    if k.K == 1:                    # no graph term: the attention parameters have no gradient
        assert not r.want["mixer"].any()
        if k.mode == tg.GM:
            assert not r.want["weight"].any() and not r.want["weight_bias"].any()


@pytest.mark.parametrize("cid", list(tg.GNN_CASES))
def test_gnn_case_inputs_keep_their_shape_property(cid):
    r = tg.gnn_reference(cid)
    k = r.case
    assert r.row_deg >= k.row_deg
    assert r.want["y"].shape == (k.B, k.F, k.N)
    for name, t in r.want.items():
        assert torch.isfinite(t).all() and float(t.abs().max()) > 0, name
    for a in range(k.B):
        for b in range(a + 1, k.B):
            assert not torch.equal(r.want["dx"][a], r.want["dx"][b]), (a, b)
