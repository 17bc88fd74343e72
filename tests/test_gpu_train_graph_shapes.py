"""The training kernels of the graph layers (csrc/gat_train.hip, magat_gat_train_forward_f32) at the shapes training uses and
the branches those shapes take: instance indices past the first round of eight, rows and columns longer than one wave stride,
N past one pass of the transpose kernel, every feature width with graph terms, K = 5 and K = 1, graphs without edges, padded
inputs, two backward passes over one graph, and the column view the training forward builds for itself.

Yardstick: graphml._composite in float64 on the CPU (GraphFilterBatch: the float64 hop algebra), inputs and references from
tests/train_graph_cases.py.  Gate: max|got - want| <= 2e-4 * max(1, max|want|) per tensor - the gate of the existing training
tests.  It holds for every case: the float32 composite's own error against the float64 one, measured on the CPU, is at most
7.7e-7 of that scale over all cases (worst: long-GAT_modified-mean-hubs, mixer).  Every case runs twice and must repeat bit
for bit (the kernels sum without atomics)."""
import pytest
import torch

import train_graph_cases as tg
from test_gpu_config5 import _legacy_structure

pytestmark = pytest.mark.gpu


def _ran(fn, name):
    """Is an autograd node called `name` among fn and its ancestors?"""
    seen, todo = set(), [fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if type(f).__name__ == name:
            return True
        todo += [g for g, _ in f.next_functions]
    return False


def _device_pass(layer, r, dev, function):
    layer.zero_grad(set_to_none=True)
    xg = r.x.to(dev).requires_grad_(True)
    y = layer(xg)
    assert _ran(y.grad_fn, function)           # the HIP function, not the composite
    (y * r.wgt.to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = {"y": y.detach(), "dx": xg.grad}
    got.update({n: None if p.grad is None else p.grad.clone() for n, p in layer.named_parameters()})
    return got


def _compare(cid, got, again, want):
    """got == again bit for bit; got within the gate of want, tensor by tensor; prints the worst relative error per group."""
    worst = {"y": 0.0, "dx": 0.0, "params": 0.0}
    fails = []
    for name, b in want.items():
        a, a2 = got[name], again[name]
        assert (a is None) == (a2 is None) and (a is None or torch.equal(a, a2)), (cid, name, "differs from run to run")
        if not b.any():                       # no gradient in the reference: none, or exact zeros
            assert a is None or not a.any(), (cid, name, "reference gradient is zero")
            continue
        assert a is not None and a.shape == b.shape, (cid, name)
        scale = max(1.0, float(b.abs().max()))
        err = float((a.cpu().double() - b).abs().max()) / scale
        group = name if name in worst else "params"
        worst[group] = max(worst[group], err)
        if not err <= tg.GATE:
            fails.append((name, err))
    print("%s: worst error / max(1, max|want|): y %.2e  dx %.2e  parameter gradients %.2e" % (cid, worst["y"], worst["dx"],
                                                                                            worst["params"]))
    assert not fails, (cid, fails)


@pytest.mark.parametrize("cid", list(tg.GAT_CASES))
def test_gat_training_shapes_match_float64_composite(gpu_device, cid):
    """One forward + backward in train() mode through the HIP training kernels against the float64 composite: y, dx and every
    parameter gradient (a parameter the reference leaves without gradient: None or zeros), twice, bit-identical."""
    r = tg.gat_reference(cid)
    k = r.case
    assert r.row_deg >= k.row_deg and r.col_deg >= k.col_deg, (r.row_deg, r.col_deg)       # the input still reaches its branch
    layer = tg.gat_layer(k, r.state).to(gpu_device).train()
    layer.addGSO(r.S.unsqueeze(1).to(gpu_device))
    got = _device_pass(layer, r, gpu_device, "_GatTrainFunctionBackward")
    again = _device_pass(layer, r, gpu_device, "_GatTrainFunctionBackward")
    assert got["y"].shape == (k.B, k.P * k.G if k.concat else k.G, k.nin)
    _compare(cid, got, again, r.want)
    if k.distinct:                  # every instance has its own graph and input: its own gradient, too
        dx = got["dx"]
        assert all(not torch.equal(dx[a], dx[b]) for a in range(k.B) for b in range(a + 1, k.B))


@pytest.mark.parametrize("cid", list(tg.GNN_CASES))
def test_graph_filter_batch_training_shapes_match_float64_algebra(gpu_device, cid):
    from magat_pathplanning_amd import GraphFilterBatch
    r = tg.gnn_reference(cid)
    k = r.case
    assert r.row_deg >= k.row_deg
    layer = GraphFilterBatch(k.G, k.F, k.K)
    layer.load_state_dict(r.state)
    layer = layer.to(gpu_device).train()
    layer.addGSO(r.S.unsqueeze(1).to(gpu_device))
    got = _device_pass(layer, r, gpu_device, "_GnnTrainFunctionBackward")
    again = _device_pass(layer, r, gpu_device, "_GnnTrainFunctionBackward")
    _compare(cid, got, again, r.want)
    dx = got["dx"]
    assert all(not torch.equal(dx[a], dx[b]) for a in range(k.B) for b in range(a + 1, k.B))


@pytest.mark.parametrize("cid", ["width-KeyQuery-mean-rounds-B3N21G32K3P2", "depth-GAT_origin-mean-rounds-B3N12G32K5P2"])
def test_two_backward_passes_over_one_graph_double_every_gradient(gpu_device, cid):
    """backward(retain_graph=True) twice without zeroing: every .grad is exactly twice the single-pass value - nothing the
    forward saved (Z, the attention values, the kept hop results, the column view) was overwritten by the first pass."""
    r = tg.gat_reference(cid)
    layer = tg.gat_layer(r.case, r.state).to(gpu_device).train()
    layer.addGSO(r.S.unsqueeze(1).to(gpu_device))
    xg = r.x.to(gpu_device).requires_grad_(True)
    loss = (layer(xg) * r.wgt.to(gpu_device)).sum()
    loss.backward(retain_graph=True)
    leaves = [("dx", xg)] + list(layer.named_parameters())
    # (a parameter the mode does not use - KeyQuery's mixer and weight_bias - has no gradient, after either pass)
    first = {n: None if t.grad is None else t.grad.clone() for n, t in leaves}
    for n, g in first.items():
        b = r.want[n]
        if not b.any():
            assert g is None or not g.any(), n
        else:
            assert float((g.cpu().double() - b).abs().max()) <= tg.GATE * max(1.0, float(b.abs().max())), n
    assert all(first[n] is not None for n in ["dx"] + tg.used_names(r.case))
    loss.backward()
    torch.cuda.synchronize()
    for n, t in leaves:
        if first[n] is None:
            assert t.grad is None, n
        else:
            assert torch.equal(t.grad, 2 * first[n]), n


@pytest.mark.parametrize("gso,B,N", [(tg.gso_hubs, 2, 130), (tg.gso_full, 1, 70)])
def test_training_forward_builds_the_column_view_of_the_definition(gpu_device, gso, B, N):
    """magat_gat_train_forward_f32 called directly: the cscptr / cscsrc / cscpos it leaves behind (csr_transpose_kernel +
    csr_sort_columns_kernel, columns of in-degree > 64 and > 128) equal the host construction bit for bit - independently of
    the gradients that are computed through them."""
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd.graphml import dense_gso_to_csr
    G, K, P, mode = 32, 2, 1, nat.MODE_KEYQUERY
    S = gso(B, N, 7)
    assert tg.degrees(S, tg.KQ)[1] > (128 if N == 130 else 64)
    w_rowptr, w_colidx, w_cscptr, w_cscsrc, w_cscpos, w_nnz = _legacy_structure(S, 0, gpu_device)
    dev, lib = gpu_device, nat.lib()
    rowptr, colidx, nnz = dense_gso_to_csr(S.to(dev))
    assert nnz == w_nnz and torch.equal(rowptr.cpu().long(), w_rowptr) and torch.equal(colidx[:nnz].cpu().long(), w_colidx)
    M, NC = B * N, P * G + P * K * G
    X = (torch.randn(M, G, generator=torch.Generator().manual_seed(3)) * 0.6).to(dev)
    packed = torch.zeros(lib.magat_gat_packed_floats(G, G, K, P, mode), dtype=torch.float32, device=dev)
    Ypre, att, Z = torch.empty(M, P * G, device=dev), torch.empty(P, nnz, device=dev), torch.empty(M, NC, device=dev)
    cscptr = torch.full((B * (N + 1),), -1, dtype=torch.int32, device=dev)
    csc = torch.full((3, nnz), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.magat_gat_train_forward_f32(
            nat.ptr(X), nat.ptr(rowptr), nat.ptr(colidx), nnz, nat.ptr(packed), None, nat.ptr(Ypre), nat.ptr(att), nat.ptr(Z),
            None, nat.ptr(cscptr), nat.ptr(csc[0]), nat.ptr(csc[1]), nat.ptr(csc[2]), B, N, G, G, K, P, mode,
            nat.current_stream(dev)), "magat_gat_train_forward_f32")
    torch.cuda.synchronize()
    assert torch.equal(cscptr.cpu().long(), w_cscptr)
    assert torch.equal(csc[0].cpu().long(), w_cscsrc)
    assert torch.equal(csc[1].cpu().long(), w_cscpos)


def test_layer_with_other_output_width_is_refused_under_autograd(gpu_device):
    """What a G != F layer does in train() mode on the GPU today: the training entries refuse it (MAGAT_ERR_UNSUPPORTED), the
    layer hands that on as the typed error - no composite takes over - and no parameter has seen a gradient."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    from magat_pathplanning_amd import _native as nat
    B, N, G, F = 2, 8, 32, 64
    layer = GraphFilterBatchAttentional(G, F, 3, 2, attentionMode=tg.KQ).to(gpu_device).train()
    layer.addGSO(tg.gso_rounds(B, N, 5).unsqueeze(1).to(gpu_device))
    xg = (torch.randn(B, G, N, generator=torch.Generator().manual_seed(4)) * 0.6).to(gpu_device).requires_grad_(True)
    with pytest.raises(nat.MagatNativeError):
        layer(xg)
    torch.cuda.synchronize()
    assert xg.grad is None and all(p.grad is None for p in layer.parameters())
