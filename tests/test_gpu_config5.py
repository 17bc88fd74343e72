"""BASELINE config 5 at its OWN size: 1000 agents, sparse comm-radius GSO, K=2, P=4, bf16 storage inside the graph layer
(and the same shape with fp32 storage).  The oracle's dense op sequence on (B,P,1000,1000) tensors finishes in seconds
at B = 2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N5, K5, P5, G5, MAP5 = 1000, 2, 4, 128, 160


def _legacy_structure(S, rule, device):
    """CSR + CSC of a dense GSO by plain torch on the host: the definition the device builder must reproduce."""
    B, N, _ = S.shape
    if rule == 0:
        m = S.abs() > 1e-9
    elif rule == 1:
        m = (S.float() + torch.eye(N)).abs() > 1e-9
    else:
        m = S.float() != 0
    rowptr = torch.zeros(B, N + 1, dtype=torch.int64)
    cscptr = torch.zeros(B, N + 1, dtype=torch.int64)
    cols, srcs, poss = [], [], []
    base = 0
    for b in range(B):
        deg = m[b].sum(1)
        rowptr[b, 0] = base
        rowptr[b, 1:] = base + torch.cumsum(deg, 0)
        ii, jj = torch.nonzero(m[b], as_tuple=True)            # row-major: ascending j inside a row
        cols.append(jj)
        pos = base + torch.arange(ii.numel())
        cdeg = m[b].sum(0)
        cscptr[b, 0] = base
        cscptr[b, 1:] = base + torch.cumsum(cdeg, 0)
        order = torch.argsort(jj * N + ii)                      # by column, then source row
        srcs.append(ii[order])
        poss.append(pos[order])
        base += ii.numel()
    return rowptr.reshape(-1), torch.cat(cols), cscptr.reshape(-1), torch.cat(srcs), torch.cat(poss), base


@pytest.mark.parametrize("N,dtype,rule", [(1000, torch.float32, 0), (1000, torch.float64, 0), (333, torch.float32, 1),
                                          (64, torch.float64, 2), (1024, torch.float32, 0),
                                          # float32 rows of N % 4 == 0 take the four-columns-per-lane pass: every edge rule,
                                          # a row shorter than one request, a row that ends inside the second 256-column step
                                          (200, torch.float32, 1), (132, torch.float32, 2), (8, torch.float32, 0),
                                          (260, torch.float32, 0)])
def test_gso_csr_build_matches_the_definition(gpu_device, N, dtype, rule):
    """magat_gso_csr_build: rowptr / colidx / cscptr / cscsrc / cscpos bit-exact against a host construction, the device
    edge total, and the fused in-place scrub (NaN -> 0, dist_GSO_one) against torch on the same tensor."""
    from magat_pathplanning_amd.graphml import CsrStructure
    from magat_pathplanning_amd.synthetic import comm_gso
    B = 3
    S = comm_gso(B, N, int(6.5 * N ** 0.5), seed=N + rule, dtype=dtype)
    S[0, 5, 7] = float("nan")
    S[1, 2, 3] = 5e-10          # below the 1e-9 threshold: not an edge under rule 0
    S[2, N - 1, 0] = -3e-9
    S[1, 4, :] = 0              # isolated row
    Sd = S.clone().to(gpu_device)
    st = CsrStructure().build(Sd, rule, scrub_nan=1, gso_mode=0)
    torch.cuda.synchronize()
    want_S = S.clone()
    want_S[torch.isnan(want_S)] = 0
    assert torch.equal(Sd.cpu(), want_S)                     # scrubbed in place, nothing else touched
    rowptr, colidx, cscptr, cscsrc, cscpos, nnz = _legacy_structure(want_S, rule, gpu_device)
    assert st.exact_nnz() == nnz
    assert torch.equal(st.rowptr.cpu().long(), rowptr)
    assert torch.equal(st.cscptr.cpu().long(), cscptr)
    assert torch.equal(st.colidx[:nnz].cpu().long(), colidx)
    assert torch.equal(st.csc[0][:nnz].cpu().long(), cscsrc)
    assert torch.equal(st.csc[1][:nnz].cpu().long(), cscpos)
    # dist_GSO_one: positive entries become 1 in place
    Sd2 = S.clone().to(gpu_device)
    CsrStructure().build(Sd2, rule, scrub_nan=1, gso_mode=1)
    w2 = want_S.clone()
    w2[w2 > 0] = 1
    assert torch.equal(Sd2.cpu(), w2)


@pytest.mark.parametrize("N,density", [(1000, 0.05), (512, 0.06), (1000, 0.011)])
def test_gso_csr_build_dense_instances(gpu_device, N, density):
    """Instances with more edges than the structure kernel's LDS stage holds (12 288) are written and sorted through global
    memory; instances around the limit take either way - the arrays are the host construction's in both."""
    from magat_pathplanning_amd.graphml import CsrStructure
    g = torch.Generator().manual_seed(N + int(1000 * density))
    B = 3
    S = (torch.rand(B, N, N, generator=g) < density).float() * (torch.rand(B, N, N, generator=g) + 0.5)
    S[1] = S[1] * (torch.rand(N, N, generator=g) < 0.1).float()          # one sparse instance between two dense ones
    Sd = S.clone().to(gpu_device)
    st = CsrStructure().build(Sd, 0, scrub_nan=1, gso_mode=0)
    rowptr, colidx, cscptr, cscsrc, cscpos, nnz = _legacy_structure(S, 0, gpu_device)
    assert st.exact_nnz() == nnz
    assert torch.equal(st.rowptr.cpu().long(), rowptr)
    assert torch.equal(st.cscptr.cpu().long(), cscptr)
    assert torch.equal(st.colidx[:nnz].cpu().long(), colidx)
    assert torch.equal(st.csc[0][:nnz].cpu().long(), cscsrc)
    assert torch.equal(st.csc[1][:nnz].cpu().long(), cscpos)


@pytest.mark.parametrize("kind,N,B", [("star", 1000, 3), ("leader", 600, 2), ("dense", 1000, 2), ("dense", 1024, 1), ("star", 100, 5)])
def test_gso_csr_build_hub_columns_and_dense_instances_are_bounded(gpu_device, kind, N, B):
    """a hub COLUMN (star / leader graph: every row points at one node - a column list of N entries) and a fully
    dense instance (N^2 edges: far beyond the LDS stage) used to cost O(deg^2) serial work per column (LDS reads in the staged
    path, L2 round trips in the global one: up to seconds).  Round 6: hub lists are ranked by the whole workgroup, an instance
    beyond the stage places every in-edge by its rank in the transposed bit matrix.  Same arrays as the host construction,
    and the build is timed: milliseconds, not seconds."""
    import time
    from magat_pathplanning_amd.graphml import CsrStructure
    g = torch.Generator().manual_seed(N + B)
    if kind == "dense":
        S = torch.rand(B, N, N, generator=g) + 0.5
        S[0, 5, :] = 0                                     # (one empty row, one empty column)
        S[0, :, 9] = 0
    else:
        S = (torch.rand(B, N, N, generator=g) < 4.0 / N).float()
        S[:, :, 7] = 1.0                                   # every row -> node 7
        if kind == "leader":
            S[:, 3, :] = 1.0                               # ... and node 3 -> every node
            S[:, :, N - 1] = 1.0
    Sd = S.to(gpu_device)
    st = CsrStructure().build(Sd, 0)
    nnz = st.ready(gpu_device)                             # (dense: the capacity guess is exceeded once and regrown)
    rowptr, colidx, cscptr, cscsrc, cscpos, want = _legacy_structure(S, 0, gpu_device)
    assert nnz == want
    assert torch.equal(st.rowptr.cpu().long(), rowptr) and torch.equal(st.cscptr.cpu().long(), cscptr)
    assert torch.equal(st.colidx[:nnz].cpu().long(), colidx)
    assert torch.equal(st.csc[0][:nnz].cpu().long(), cscsrc)
    assert torch.equal(st.csc[1][:nnz].cpu().long(), cscpos)
    times = []
    for _ in range(3):      # (best of three: a process's first few hundred launches can carry a one-off 60-90 ms runtime stall)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.build(Sd, 0)
        st.ready(gpu_device)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    ms = min(times)
    print("CSR + CSC build, %s N=%d B=%d (%d edges): %.2f ms (three builds: %s)" % (kind, N, B, nnz, ms, ["%.2f" % t for t in times]))
    assert ms < 50.0, times


def test_gso_csr_build_at_config5_size(gpu_device):
    """BASELINE config 5's full shape (128 instances x 1000 agents, 512 MB of GSO) through size-independent properties: the
    device edge total equals torch's count over the scrubbed tensor, every row's degree equals its row count, column indices
    ascend inside a row and hit edges only, the CSC view holds every edge exactly once, and a second build is bit-identical."""
    from magat_pathplanning_amd.graphml import CsrStructure
    from magat_pathplanning_amd.synthetic import comm_gso
    B, N = 128, 1000
    S = comm_gso(B, N, 160, seed=9).to(gpu_device)
    S[5, 17, 400] = float("nan")
    st = CsrStructure().build(S, 0, scrub_nan=1)
    nnz = st.ready(gpu_device)
    assert not bool(torch.isnan(S).any())
    edges = S.abs() > 1e-9
    assert nnz == int(edges.sum())
    rp = st.rowptr.view(B, N + 1).long()
    deg = rp[:, 1:] - rp[:, :-1]
    assert torch.equal(deg, edges.sum(-1))
    assert int(rp[0, 0]) == 0 and int(rp[-1, -1]) == nnz and bool((rp[1:, 0] == rp[:-1, -1]).all())
    rows = torch.repeat_interleave(torch.arange(B * N, device=gpu_device), deg.reshape(-1))
    cols = st.colidx[:nnz].long()
    assert bool(edges.view(B * N, N)[rows, cols].all())                       # every stored index is an edge
    same_row = rows[1:] == rows[:-1]
    assert bool((cols[1:][same_row] > cols[:-1][same_row]).all())             # ascending inside a row
    pos = st.csc[1][:nnz].long()
    assert torch.equal(torch.sort(pos).values, torch.arange(nnz, device=gpu_device))      # CSC = a permutation of the edges
    src = st.csc[0][:nnz].long()
    assert torch.equal(src, (rows % N)[pos])                                  # ... whose sources are those edges' rows
    first = [t.clone() for t in (st.rowptr, st.colidx[:nnz], st.cscptr, st.csc[0][:nnz], st.csc[1][:nnz])]
    st2 = CsrStructure().build(S, 0, scrub_nan=1)
    assert st2.ready(gpu_device) == nnz
    for a, b in zip(first, (st2.rowptr, st2.colidx[:nnz], st2.cscptr, st2.csc[0][:nnz], st2.csc[1][:nnz])):
        assert torch.equal(a, b)


def test_gso_csr_capacity_guess_regrows(gpu_device):
    """The index arrays are sized by a guess (32 edges per node), not by the dense bound B*N*N: a graph denser than the guess
    makes the kernel drop the overflow, the count that travels back shows it, and ready() re-builds with room - same
    structure as a construction on the host, and the layer's result equals the dense-kernel result for the same graph."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    from magat_pathplanning_amd.graphml import CsrStructure, gat_forward_rows_csr
    from magat_pathplanning_amd.synthetic import directed_gso
    B, N = 3, 120
    S = torch.nan_to_num(directed_gso(B, N, 0.6, seed=5, dtype=torch.float32))
    Sd = S.to(gpu_device)
    st = CsrStructure().build(Sd, 0)
    first_cap = st.cap
    nnz = st.ready(gpu_device)
    rowptr, colidx, cscptr, cscsrc, cscpos, want = _legacy_structure(S, 0, gpu_device)
    assert want > first_cap and nnz == want and st.cap >= nnz and st.cap < B * N * N
    assert torch.equal(st.rowptr.cpu().long(), rowptr) and torch.equal(st.colidx[:nnz].cpu().long(), colidx)
    assert torch.equal(st.csc[0][:nnz].cpu().long(), cscsrc) and torch.equal(st.csc[1][:nnz].cpu().long(), cscpos)
    torch.manual_seed(3)
    layer = GraphFilterBatchAttentional(32, 32, 3, 2, attentionMode="KeyQuery").to(gpu_device).eval()
    X = torch.randn(B, N, 32, device=gpu_device)
    out, _ = gat_forward_rows_csr(X, st.rowptr, st.colidx, nnz, layer, csc=(st.cscptr, st.csc[0], st.csc[1]))
    layer.addGSO(Sd.unsqueeze(1))
    with torch.no_grad():
        dense = layer(X.permute(0, 2, 1).contiguous()).permute(0, 2, 1).reshape(B * N, -1)
    np.testing.assert_allclose(out.cpu().numpy(), dense.cpu().numpy(), rtol=0, atol=2e-5)


def test_addgso_scrub_is_ordered_for_the_callers_stream(gpu_device):
    """the CSR branch of addGSO scrubs S on a side stream - every reader on the caller's stream after addGSO
    returns must see the scrubbed tensor (the reference's addGSO has mutated S when it returns), without a device sync."""
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd import DecentralPlannerGATNet
    from magat_pathplanning_amd.synthetic import comm_gso, make_config
    B, N = 16, 1000
    cfg = make_config(num_agents=N, nGraphFilterTaps=2, nAttentionHeads=4, GSO_mode="dist_GSO_one", device=str(gpu_device))
    cfg.gat_storage = "bf16"
    net = DecentralPlannerGATNet(cfg).to(gpu_device).eval()
    S = comm_gso(B, N, 206, seed=3)
    S[:, 7, 9] = float("nan")
    want = S.clone()
    want[torch.isnan(want)] = 0
    want[want > 0] = 1
    for _ in range(3):
        Sd = S.to(gpu_device)
        big = torch.randn(64, 1024, 1024, device=gpu_device)
        (big @ big).sum()                                   # the caller's stream is busy: the side stream starts behind it
        net.addGSO(Sd)
        seen = Sd.clone()                                   # caller's stream, no synchronisation in between
        assert torch.equal(seen.cpu(), want)


@pytest.mark.parametrize("tiled", [3, 0])
@pytest.mark.parametrize("storage", ["bf16", "fp32"])
def test_config5_layer_at_1000_agents(gpu_device, storage, tiled, libopt):
    """GraphFilterBatchAttentional at N=1000, K=2, P=4, G=F=128 on the CSR kernels with the device-built structure:
    fp32 storage against the pinned oracle (1e-4 of the output scale), bf16 storage against the oracle's bf16-storage
    emulation (same rounding points, ~1 bf16 ulp of the output scale) and within the bf16 budget of the fp32 oracle."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    from magat_pathplanning_amd.synthetic import comm_gso
    from oracle import magat_oracle as orc
    libopt.set("CSR_TILED", tiled)  # 3: LDS-tiled kernels (default), 0: the L2-gather kernels
    libopt.set("CSR_FUSED", 0)      # the SPLIT form (maps GEMM + score / hop kernels); the fused form: tests/test_gpu_csr_fused.py
    B = 2
    g = torch.Generator().manual_seed(15)
    layer = GraphFilterBatchAttentional(G5, G5, K5, P5, attentionMode="KeyQuery")
    x = torch.randn(B, G5, N5, generator=g) * 0.5
    S = comm_gso(B, N5, MAP5, seed=8)
    params = {k: v.detach() for k, v in layer.state_dict().items()}
    y_ref, _ = orc.gat_layer_forward(x, S.unsqueeze(1), params, "KeyQuery", True)
    layer = layer.to(gpu_device).eval()
    if storage == "bf16":
        layer.storage_dtype = torch.bfloat16
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad():
        y = layer(x.to(gpu_device)).cpu()
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, P5 * G5, N5)
    scale = float(y_ref.abs().max())
    err = float((y - y_ref).abs().max())
    print("config-5 layer (%s storage): scale %.3g, err vs fp32 oracle %.3g" % (storage, scale, err))
    if storage == "fp32":
        assert err <= 1e-4 * max(1.0, scale), (err, scale)
    else:
        y_emul, _ = orc.gat_layer_forward_bf16_storage(x, S.unsqueeze(1), params, "KeyQuery", True)
        assert float((y - y_emul).abs().max()) <= 2.0 ** -7 * scale
        assert err <= 2e-2 * scale


@pytest.mark.parametrize("concat", [True, False])
def test_bf16_storage_float32_result_is_the_cast_of_the_bf16_result(gpu_device, concat):
    """magat_gat_forward_csc_bf16_f32out: the layer's last kernel widens its bf16-rounded rows itself - bit for bit the values
    a bf16 result gives after a cast (the planner's bf16-storage branch uses it instead of a cast kernel)."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    from magat_pathplanning_amd.graphml import CsrStructure, gat_forward_rows_csr
    from magat_pathplanning_amd.synthetic import comm_gso
    B, N = 3, 200
    torch.manual_seed(4)
    layer = GraphFilterBatchAttentional(G5, G5, K5, P5, attentionMode="KeyQuery", concatenate=concat).to(gpu_device).eval()
    X = (torch.randn(B, N, G5, device=gpu_device) * 0.5).to(torch.bfloat16)
    S = comm_gso(B, N, 40, seed=2).to(gpu_device)
    st = CsrStructure().build(S, 0)
    nnz = st.ready(gpu_device)
    csc = (st.cscptr, st.csc[0], st.csc[1])
    width = P5 * G5 if concat else G5
    y16 = torch.empty(B * N, width, dtype=torch.bfloat16, device=gpu_device)
    y32 = torch.full((B * N, width + 4), -7.0, dtype=torch.float32, device=gpu_device)      # (a wider buffer: ld > width)
    gat_forward_rows_csr(X, st.rowptr, st.colidx, nnz, layer, out=y16, csc=csc)
    gat_forward_rows_csr(X, st.rowptr, st.colidx, nnz, layer, out=y32, csc=csc)
    assert torch.equal(y32[:, :width].cpu(), y16.float().cpu())
    assert bool((y32[:, width:] == -7.0).all())
    assert float(y16.float().abs().max()) > 0


def test_config5_model_bf16_at_1000_agents(gpu_device):
    """The whole module at config 5's shape (B=2 instances of 1000 agents, K=2, P=4, gat_storage='bf16') against the fp32
    oracle: error reported and bounded, greedy actions agree; no host synchronisation between addGSO and the logits."""
    from magat_pathplanning_amd import DecentralPlannerGATNet
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    from oracle import magat_oracle as orc
    B = 2
    cfg = make_config(num_agents=N5, nGraphFilterTaps=K5, nAttentionHeads=P5, gat_storage="bf16", device=str(gpu_device))
    sd = orc.init_state_dict(cfg, seed=21)
    x = fov_states(B, N5, seed=5)
    S = comm_gso(B, N5, MAP5, seed=6)
    ref = orc.planner_forward(x, S.clone(), sd, cfg)
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd)
    net = net.to(gpu_device).eval()
    with torch.no_grad():
        net.addGSO(S.to(gpu_device))
        assert net._rt.csr.key is not None            # structure made at addGSO, on the device
        got = net(x.to(gpu_device)).cpu()
    err = (got - ref).abs().max().item()
    agree = (got.argmax(1) == ref.argmax(1)).float().mean().item()
    print("config 5 (N=1000, bf16 GAT storage): max|dlogit| = %.3e of scale %.3g, argmax agreement = %.4f"
          % (err, ref.abs().max().item(), agree))
    assert err <= 2e-2 * max(1.0, ref.abs().max().item()), err
    assert agree >= 0.97, agree
    # fp32 storage at the same shape: the 1e-4 gate
    cfg32 = make_config(num_agents=N5, nGraphFilterTaps=K5, nAttentionHeads=P5, device=str(gpu_device))
    net32 = DecentralPlannerGATNet(cfg32)
    net32.load_state_dict(sd)
    net32 = net32.to(gpu_device).eval()
    with torch.no_grad():
        net32.addGSO(S.to(gpu_device))
        got32 = net32(x.to(gpu_device)).cpu()
    assert (got32 - ref).abs().max().item() <= 1e-4


def test_gat_forward_rows_keeps_the_structure_built_at_addgso_time(gpu_device):
    """The structure is keyed on the GSO's data_ptr() and _version (CsrStructure.matches): the layer's GSO intake must hand a
    contiguous device f32 GSO - here as the (B,1,N,N) view the model stores - back as itself, or every step would re-build
    the structure and wait for its edge count.  Proof by state: the key stays, the layer never builds a structure of its own."""
    from magat_pathplanning_amd.graphml import CsrStructure, GraphFilterBatchAttentional, dense_route, gat_forward_rows
    from magat_pathplanning_amd.synthetic import comm_gso
    B, N, G, K, P = 2, 130, 16, 2, 2                       # 130 agents: just past the LDS-resident kernels
    torch.manual_seed(5)
    layer = GraphFilterBatchAttentional(G, G, K, P, attentionMode="KeyQuery").to(gpu_device).eval()
    assert not dense_route(N, layer) and CsrStructure.supported(B, N)
    S = comm_gso(B, N, 40, seed=11, dtype=torch.float32).to(gpu_device)
    X = torch.randn(B, N, G, device=gpu_device)
    csr = CsrStructure().build(S, layer.edge_rule)         # "addGSO time"
    key = csr.key
    outs = []
    with torch.no_grad():
        for _ in range(2):
            assert csr.matches(S, layer.edge_rule)
            out, _ = gat_forward_rows(X, S.view(B, 1, N, N), layer, csr=csr)
            outs.append(out.clone())
    torch.cuda.synchronize()
    assert csr.key == key and csr.matches(S, layer.edge_rule)
    assert layer._scratch.csr is None
    assert csr.nnz == int((S.abs() > 1e-9).sum())
    assert outs[0].shape == (B * N, P * G) and bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0], outs[1])
