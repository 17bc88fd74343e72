"""The fused bf16 CSR layer (csrc/gat_csr_fused.hip: csr_rank_kernel, csr_fused_scores_kernel<P>, csr_fused_hop_kernel<HP>,
csr_fused_pack_kernel) STAGE BY STAGE, with probe weights that make the stages around the one under test exact, each stage
gated at the precision of its own arithmetic against a float64 reference written from the edge lists
(tests/csr_fused_cases.py; its properties and the gates' sensitivity: tests/test_host_csr_fused_cases.py).

  probe X    H_p0 = signed permutation, H_p1 = 0 (a bf16-exact bias on one result type per case): y = relu(+-x[perm] + bias)
             VALUE FOR VALUE, no tolerance - row ownership of the degree ranking, padding lanes, instance / XCD dealing, the
             fragment pack's layout, head placement, ldy, the LDS stage of the bf16 rows and the float32 store path; the
             sentinel behind float32 rows untouched; a second run gives identical bits (-0 and +0 are one value here)
  attention  probe Q (exact scores) and probe U (all scores 0), per head: row sums within 1e-5; per row
             max|a - a*| / max a* <= max(3e-6, 4 x the float32 restatement's own value on that row); under U every value
             within one float32 ulp of 1 / outdeg and exact where outdeg is a power of two
  hop        probe Z on top of Q and of U, both signs: |y - relu(+-z*[perm])| <= 2^-8 |z*| + t, t = 4 x the restatement's own
             distance from float64 on that (column, head), floor 1e-6 max|x|; columns without in-edges exactly 0
  random     random weights against the oracle's emulation per ROW: max_f |y - y_emul| <= c max(row scale, floor), c and floor
             from the emulation's own distance to float64 arithmetic of the same order (host test: c = 9.3e-3 / 1.9e-2,
             floor = 9.8e-4 / 2.0e-3 at ladder-P4 / N257-B9-P4)

Every run asserts that the csr_fused form counter moved by one.  Graphs of up to 1024 agents go through
CsrStructure().build(S, 0), whose arrays must equal the ones the cases module makes; beyond the structure builder's 1024
agents (N = 2500, and the 64 x 1100 case whose 40 items per XCD take the persistent loops round twice) the cases module's
arrays go to gat_forward_rows_csr as they are; one case takes the arrays batched_edges makes from agent positions - what
DecentralPlannerGATNet.addGSO(batched_edges(..)) hands to these kernels.

MEASURED (MI355X, unmodified build; printed by the tests):
  probe X    0 values differ in all 28 runs (14 cases x 2 result types, 18.0 M values at 64 x 1100), sentinel intact, second run
             identical
  attention  max|a - a*| / max a* per row, worst row (float32 restatement; online-softmax restatement in the kernel's slot order
             with exp2(x log2 e)) | row sums.  The kernel's figure equals the online restatement's to three digits in every
             case, so the plain restatement's 3e-6 / 4 x gate holds unchanged (worst: 0.25 of the bound, on the N - 1 rows).
               case                 probe Q                             row sums   probe U    row sums
               ladder-P4            2.97e-7 (3.81e-7; 2.97e-7)          2.96e-7    5.77e-8    5.77e-8
               ladder-P2            2.65e-7 (2.59e-7; 2.65e-7)          2.56e-7    5.77e-8    5.77e-8
               ladder-P1            2.84e-7 (2.31e-7; 2.84e-7)          3.08e-7    5.77e-8    5.77e-8
               N1-B3-P4             0                                   0          0          0
               N31-B8-P2            2.18e-7 (2.43e-7; 2.18e-7)          2.12e-7    5.22e-8    5.22e-8
               N32-B9-P1            1.54e-7 (1.54e-7; 1.54e-7)          1.49e-7    4.47e-8    4.47e-8
               N33-B17-P4           1.86e-7 (2.13e-7; 1.86e-7)          1.92e-7    4.47e-8    4.47e-8
               N255-B1-P2           2.60e-7 (2.26e-7; 2.60e-7)          2.35e-7    5.22e-8    5.22e-8
               N256-B1-P4           2.12e-7 (2.66e-7; 2.12e-7)          2.12e-7    5.22e-8    5.22e-8
               N257-B9-P4           4.08e-7 (2.52e-7; 4.08e-7)          3.77e-7    5.22e-8    5.22e-8
               N1024-B1-P2          1.47e-6 (1.47e-6; 1.47e-6)          1.45e-6    5.22e-8    5.22e-8
               N2500-B1-P4          1.47e-6 (1.47e-6; 1.47e-6)          1.50e-6    5.22e-8    5.22e-8
               trip2-B64-N1100-P2   -                                   -          4.47e-8    4.47e-8
               edges-B2-N300-P4     2.31e-7 (1.98e-7; 2.31e-7)          2.09e-7    4.47e-8    4.47e-8
             probe U: every value within one ulp of 1 / outdeg, exact at powers of two, in every case
  hop        worst |y - relu(+-z*)| as a fraction of its bound, over both signs and both score probes: 0.979 .. 0.996 in every
             case with an edge beyond a self-loop (N1-B3-P4: 0), equal to the restatement's own fraction to three digits in
             all 54 runs - the bf16 rounding's worst case, nothing of the kernel's on top
  random     max_f |y - y_emul| / row scale: 4.7e-3 at ladder-P4 (c = 9.3e-3; 94 of 337 920 values differ from the emulation,
             each by one bf16 unit), 4.5e-3 at N257-B9-P4 (c = 1.9e-2; 438 of 1 184 256)
  58 tests, 6.7 s together; the slowest is the hop test of the 64 x 1100 case at 1.9 s (its float64 reference).
MUTATIONS of gat_csr_fused.hip, one at a time on a scratch build, this file run once each:
  (a) score kernel, memory-slot loop: the last edge of a row with more than 8 edges neither `put` nor `track`ed - 54 red: the
      attention test of all 13 cases with such a row, and with it (the slot is read back unwritten: stale values, NaN among
      them, travel through the hop) every hop, probe-X and random-weights test of those cases; green: the four N1-B3-P4 tests
  (b) hop kernel, `load4i` tail: the last in-edge treated as absent when deg % 4 == 1 - 16 red: the hop test of all 14 cases
      (under Q and under U) and both random-weights tests; attention and probe X green
  (c) `own[1] = swap_add(sc[3], sc[1])` - 14 red: attention and hop of the six P = 4 cases with more than one edge in a row
      (ladder-P4, N33, N256, N257, N2500, edges), both random-weights tests; every P = 1, 2 test and all of probe X green
  (d) pack kernel reading tap `1 - (k >> 7)` - 44 red: probe X (28) and the hop test (14) of every case, both random-weights
      tests; attention green
  (e) the ranking's shared bin at 31 instead of 63 edges - nothing red (58 passed): the order inside the ranking moves work
      between waves and changes no value"""
import functools

import pytest
import torch

import csr_fused_cases as C

pytestmark = pytest.mark.gpu
G = C.G
F32, F64 = torch.float32, torch.float64
NAMES = [c.name for c in C.CASES]


class _Bench:
    """the device side of one case: inputs, structure arrays, and one call of the layer per run"""

    def __init__(self, case, dev):
        from magat_pathplanning_amd.graphml import CsrStructure
        self.case, self.dev = case, dev
        g = case.graph
        host = g.arrays()
        if case.route == "edges":
            from magat_pathplanning_amd import batched_edges
            st = batched_edges(case.positions.to(dev), C.EDGES_RADIUS).structure(0)
        elif case.N <= C.CSR_BUILD_MAX_N:
            st = CsrStructure().build(g.dense().to(dev), 0)
        else:
            st = None
        if st is not None:
            self.nnz = st.ready(dev)
            assert self.nnz == g.nnz
            self.arr = {"rowptr": st.rowptr, "colidx": st.colidx, "cscptr": st.cscptr, "cscsrc": st.csc[0], "cscpos": st.csc[1]}
            for k, v in host.items():          # the builders' conventions, and the cases module's reading of them
                n = g.nnz if k in ("colidx", "cscsrc", "cscpos") else v.numel()
                assert torch.equal(self.arr[k][:n].cpu(), v), k
            self.keep = st
        else:
            self.nnz = g.nnz
            self.arr = {k: v.to(dev) for k, v in host.items()}
        self.X = case.X.to(torch.bfloat16).view(case.B, case.N, G).to(dev)

    def run(self, W, H, bias, f32out, X=None):
        """-> (y (B N, P 128) float32 on the host, attention (P, nnz) on the host)"""
        from magat_pathplanning_amd import GraphFilterBatchAttentional, _native as nat
        from magat_pathplanning_amd.graphml import gat_forward_rows_csr
        case, dev, a = self.case, self.dev, self.arr
        P = case.P
        layer = GraphFilterBatchAttentional(G, G, 2, P, attentionMode="KeyQuery")
        with torch.no_grad():
            layer.weight.copy_(W.unsqueeze(1))
            layer.filterWeight.copy_(H.unsqueeze(2))
            layer.bias.copy_((torch.zeros(G) if bias is None else bias).view(G, 1))
        layer = layer.to(dev).eval()
        width, rows = P * G, case.B * case.N
        if f32out:
            out = torch.full((rows, width + 8), -7.0, dtype=F32, device=dev)
        else:
            out = torch.full((rows, width), -7.0, dtype=torch.bfloat16, device=dev)
        before = int(nat.lib().magat_form_count(nat.FORMS["csr_fused"]))
        _, att = gat_forward_rows_csr(self.X if X is None else X, a["rowptr"], a["colidx"], self.nnz, layer, out=out,
                                      csc=(a["cscptr"], a["cscsrc"], a["cscpos"]), want_attention=True)
        torch.cuda.synchronize()
        assert int(nat.lib().magat_form_count(nat.FORMS["csr_fused"])) == before + 1
        if f32out:
            assert bool((out[:, width:] == -7.0).all())                      # the sentinel behind the rows
        return out[:, :width].float().cpu().contiguous(), att[:, :self.nnz].cpu().contiguous()


@functools.lru_cache(maxsize=2)
def _bench(name, dev):
    return _Bench(C.CASE[name], dev)


@pytest.mark.parametrize("f32out", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_probe_x_own_row_and_plumbing_bit_for_bit(gpu_device, name, f32out):
    case = C.CASE[name]
    pr = case.probes
    bench = _bench(name, gpu_device)
    bias = pr.bias if case.bias_on == ("f32" if f32out else "bf16") else None
    want = pr.read(case.X.unsqueeze(0).expand(case.P, -1, -1), 0, 1.0, bias)
    y, att = bench.run(pr.w_q(), pr.h(0), bias, f32out)
    y2, att2 = bench.run(pr.w_q(), pr.h(0), bias, f32out)
    wrong = y != want
    print("probe X %s %s: %d of %d values differ" % (name, "f32" if f32out else "bf16", int(wrong.sum()), wrong.numel()))
    assert not bool(torch.isnan(y).any())
    assert not bool(wrong.any()), (int(wrong.sum()), torch.nonzero(wrong)[:8].tolist())
    assert torch.equal(y, y2) and torch.equal(att.view(torch.int32), att2.view(torch.int32))
    assert float(want.max()) > 0


@pytest.mark.parametrize("name", NAMES)
def test_attention_per_head_against_float64(gpu_device, name):
    case = C.CASE[name]
    g, pr = case.graph, case.probes
    bench = _bench(name, gpu_device)
    for probe in case.score_probes:
        s32, s64 = C.stages(name, probe, F32), C.stages(name, probe, F64)
        own = C.attention_error(g, s32.att, s64.att)
        _, att = bench.run(pr.w_q() if probe == "Q" else pr.w_u(), pr.h(0), None, True)
        assert tuple(att.shape) == (case.P, g.nnz)
        bad, sum_err, ratio, err = C.attention_gate(g, att, s64.att, own)
        online = float(C.attention_error(g, C.online_softmax_f32(g, s32.scores), s64.att).max()) if probe == "Q" else 0.0
        print("attention %s probe %s: row sums %.3g, max|a - a*| / max a* %.3g (restatement %.3g, online restatement %.3g), "
              "%.3f of the bound" % (name, probe, sum_err, err, float(own.max()), online, ratio))
        assert not bool(bad.any()), (probe, int(bad.sum()), torch.nonzero(bad)[:8].tolist())
        if probe == "U":
            off = C.uniform_gate(g, att)
            assert not bool(off.any()), (int(off.sum()), torch.nonzero(off)[:8].tolist())


@pytest.mark.parametrize("name", NAMES)
def test_hop_readout_against_float64(gpu_device, name):
    case = C.CASE[name]
    pr = case.probes
    bench = _bench(name, gpu_device)
    for probe in case.score_probes:
        s32, s64 = C.stages(name, probe, F32), C.stages(name, probe, F64)
        t = C.hop_bound(case, s64, s32)
        W = pr.w_q() if probe == "Q" else pr.w_u()
        for flip, f32out in ((1.0, True), (-1.0, False)):
            y, _ = bench.run(W, pr.h(1, flip), None, f32out)
            bad, ratio = C.hop_gate(case, y, s64, t, flip)
            own = C.hop_gate(case, C.bf16(C.taps(case.X, s32.z16, pr.h(1, flip), None)), s64, t, flip)[1]
            print("hop %s probe %s sign %+d: %.3f of the bound (restatement %.3f)" % (name, probe, flip, ratio, own))
            assert not bool(bad.any()), (probe, flip, int(bad.sum()), torch.nonzero(bad)[:8].tolist())
            assert float(y.max()) > 0


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.random])
def test_random_weights_against_the_emulation_per_row(gpu_device, name):
    case = C.CASE[name]
    bench = _bench(name, gpu_device)
    W, H, b = C.random_weights(case.P, case.seed)
    X = C.random_inputs(case)
    y_emul = C.emulation(case, W, H, b, X)
    c, floor = C.row_budget(y_emul, C.same_order_f64(case, W, H, b, X))
    y, _ = bench.run(W, H, b, True, X=X.to(torch.bfloat16).view(case.B, case.N, G).to(gpu_device))
    d = (y.double() - y_emul.double()).abs().amax(dim=1)
    scale = torch.clamp(y_emul.double().abs().amax(dim=1), min=floor)
    print("random weights %s: max_f |y - y_emul| / row scale %.3g at the most, c = %.3g, floor = %.3g; %d of %d values differ"
          % (name, float((d / scale).max()), c, floor, int((y != y_emul).sum()), y.numel()))
    assert bool((d <= c * scale).all()), (float((d / scale).max()), c)
