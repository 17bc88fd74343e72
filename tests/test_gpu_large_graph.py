"""The inference kernels of the graph layers for graphs that do not fit LDS (csrc/gat_csr_f32.hip, csrc/gso_csr.hip) against a
float64 reference: the per-edge family (csr_scores_kernel, csr_hop_kernel, csr_k1_kernel behind the in-call csr_transpose_kernel
and csr_sort_columns_kernel) with the LDS-tiled kernels switched off, the tiled family on the same graphs, and every layer type
at 1025 ... 8190 agents - the only route there, up to the limit include/magat_hip.h documents - through the module, in eval and
in train() mode, with dense_gso_to_csr's structure, the C ABI at N = 8190 / 8191 and the whole models at 1025 agents.

Cases, inputs and references: tests/large_graph_cases.py (tests/test_host_large_graph.py checks them on the CPU).  No tag tells the
tiled and the per-edge kernels apart, so a case fixes its route itself: N > 1024, or option CSR_TILED set and read back; tags,
form counters and autograd node names show that nothing else took over.

Gates (none is made from the output of the kernel under test):
  y, float32 storage     max|got - want| <= g * max(1, max|want|), g the larger of 2e-5 (test_gat_csr_path_vs_oracle) and four
                         times the float32 composite's own error against the float64 one in the same measure (both sides are
                         float32 sums in another order, the rule of tests/test_gpu_train_cnn_shapes.py)
  attention              exact zero off the edges, every row with edges sums to 1 within 1e-5, every value within 3e-6, and per
                         row with edges max_j |a - a*| / max_j a* <= r, r the larger of 3e-6 and four times the float32
                         composite's value - the check that still says something on a row of 8190 edges, where every value is
                         far below the absolute gate
  bf16 storage           2^-7 of the output scale against the oracle's emulation of the rounding points, 2e-2 of it against the
                         float64 composite, attention within 4e-3 of the emulation (tests/test_gpu_kernels.py)
  training               2e-4 of max(1, max|want|) per tensor (tests/train_graph_cases.py)
  models                 1e-4 on the logits (tests/test_gpu_model.py); bf16 storage: 2e-2 of the scale, argmax agreement >= 0.97
Every device result is produced twice and must repeat bit for bit - with the caller's column view and behind the in-call
transpose, whose slot order depends on timing until csr_sort_columns_kernel has undone it.

The degree-8190 column of the 8190-agent cases is csr_sort_columns_kernel's worst input (its rank loop is quadratic in the
in-degree): two training passes at that size - transpose and sort included - take 0.14 s together, the whole inference case (four
forwards, the dense attention tensor twice, both composites on the CPU) 3.5 s.

Measured on an MI355X - kernel error/float32 composite's error/gate used: y of max(1, max|want|), `row` the per-row attention
measure, then the largest absolute attention error and the largest |row sum - 1|:
  CSR_TILED = 0, the per-edge kernels
    tails-KeyQuery-cat-tiny-B3N1G256K3P2                y 2.4e-7/1.5e-7/2.0e-5  row 0.0e+0/0.0e+0/3.0e-6  abs 0.0e+0  sum 0.0e+0
    tails-GAT_modified-mean-tiny-B3N3G16K2P3            y 5.5e-8/5.5e-8/2.0e-5  row 1.1e-7/1.2e-7/3.0e-6  abs 3.9e-8  sum 8.9e-8
    tails-GAT_origin-cat-tiny-B3N3G256K3P1-noatt        y 1.8e-8/1.3e-8/2.0e-5
    tails-KeyQuery-mean-degrees-B2N33G16K3P4            y 3.7e-8/3.7e-8/2.0e-5  row 1.3e-7/1.3e-7/3.0e-6  abs 7.6e-8  sum 1.0e-7
    tails-KeyQuery-cat-degrees-B2N33G32K2P4-f64         y 1.2e-7/1.3e-7/2.0e-5  row 2.4e-7/2.9e-7/3.0e-6  abs 1.1e-7  sum 1.0e-7
    tails-GAT_modified-cat-degrees-B2N65G16K3P1         y 1.4e-7/1.4e-7/2.0e-5  row 1.1e-7/1.1e-7/3.0e-6  abs 5.2e-8  sum 1.0e-7
    tails-GAT_origin-mean-degrees-B2N33G128K2P2-f64     y 1.3e-8/1.9e-8/2.0e-5  row 1.2e-7/1.3e-7/3.0e-6  abs 4.6e-8  sum 8.9e-8
    tails-GAT_modified-mean-degrees-B3N65G256K2P4-noatt y 1.2e-7/1.1e-7/2.0e-5
    tails-KeyQuery-cat-degrees-B2N65G64K4P3             y 1.5e-7/2.6e-7/2.0e-5  row 2.8e-7/5.5e-7/3.0e-6  abs 1.5e-7  sum 1.2e-7
    tails-GAT_origin-cat-degrees-B2N65G16K5P2           y 2.7e-8/4.2e-8/2.0e-5  row 1.3e-7/1.4e-7/3.0e-6  abs 6.1e-8  sum 1.0e-7
    degree-KeyQuery-cat-hubs-B2N130G64K3P2              y 3.4e-7/2.5e-7/2.0e-5  row 4.4e-7/5.1e-7/3.0e-6  abs 1.6e-7  sum 1.8e-7
    degree-GAT_modified-mean-hubs-B2N130G32K2P1         y 2.9e-7/3.3e-7/2.0e-5  row 1.7e-7/1.6e-7/3.0e-6  abs 5.8e-8  sum 1.0e-7
    degree-GAT_origin-cat-hubs-B2N130G64K3P4-f64        y 2.7e-8/1.9e-8/2.0e-5  row 1.7e-7/1.8e-7/3.0e-6  abs 3.5e-8  sum 1.3e-7
    degree-KeyQuery-mean-full-B1N70G128K2P3             y 1.5e-7/1.3e-7/2.0e-5  row 7.1e-7/1.3e-6/5.2e-6  abs 1.4e-7  sum 3.7e-7
    degree-GAT_modified-cat-full-B1N70G64K3P2           y 4.0e-7/2.4e-7/2.0e-5  row 1.7e-7/1.7e-7/3.0e-6  abs 3.2e-9  sum 1.3e-7
    degree-GAT_origin-mean-full-B1N70G32K2P4-noatt      y 1.1e-8/9.3e-9/2.0e-5
    degree-KeyQuery-cat-edgeless-B2N8G64K3P1            y 1.3e-7/2.3e-7/2.0e-5  row 0.0e+0/0.0e+0/3.0e-6  abs 0.0e+0  sum 0.0e+0
    degree-GAT_origin-cat-edgeless-B2N8G128K2P1         y 2.8e-8/5.4e-8/2.0e-5  row 0.0e+0/0.0e+0/3.0e-6  abs 0.0e+0  sum 0.0e+0
    degree-GAT_modified-cat-first_edgeless-B2N8G128K3P3 y 1.5e-7/2.7e-7/2.0e-5  row 1.6e-7/1.6e-7/3.0e-6  abs 3.4e-8  sum 1.2e-7
    degree-GAT_origin-mean-no_edge_row-B2N12G32K3P3     y 9.5e-9/9.5e-9/2.0e-5  row 1.3e-7/1.7e-7/3.0e-6  abs 2.5e-8  sum 8.2e-8
    depth-KeyQuery-cat-degrees-B2N33G32K1P2             y 1.5e-7/1.7e-7/2.0e-5  row 1.8e-7/3.9e-7/3.0e-6  abs 9.3e-8  sum 8.9e-8
    depth-GAT_modified-mean-degrees-B2N33G64K1P3-noatt  y 6.1e-8/1.0e-7/2.0e-5
    depth-KeyQuery-mean-rounds-B3N21G128K5P4            y 1.3e-7/1.5e-7/2.0e-5  row 5.0e-7/1.6e-6/6.2e-6  abs 1.9e-7  sum 1.7e-7
    depth-GAT_modified-cat-rounds-B3N21G256K4P3         y 3.3e-7/2.7e-7/2.0e-5  row 1.8e-7/1.9e-7/3.0e-6  abs 4.9e-8  sum 1.2e-7
    rounds-KeyQuery-cat-rounds-B9N10G32K3P3             y 1.4e-7/1.7e-7/2.0e-5  row 2.5e-7/3.5e-7/3.0e-6  abs 7.5e-8  sum 1.6e-7
    rounds-GAT_modified-mean-rounds-B17N10G64K2P2       y 1.7e-7/2.3e-7/2.0e-5  row 1.8e-7/1.6e-7/3.0e-6  abs 4.9e-8  sum 1.0e-7
    rounds-GAT_origin-cat-rounds-B9N10G16K3P4           y 1.0e-8/8.8e-9/2.0e-5  row 1.5e-7/1.8e-7/3.0e-6  abs 3.9e-8  sum 1.3e-7
    gnn-GNN-cat-degrees-B2N33G32K3P1F64-f64-noatt       y 1.4e-7/1.2e-7/2.0e-5
    gnn-GNN-cat-hubs-B2N130G64K2P1F16-noatt             y 1.9e-7/2.4e-7/2.0e-5
  the same, bf16 storage: y against the emulation and against float64, of the output scale; attention against the emulation
    bf16-KeyQuery-cat-hubs-B2N130G32K3P2-bf16           y 0.0e+0  3.4e-3  attention 1.2e-7
    bf16-GAT_modified-mean-degrees-B2N65G64K2P4-bf16    y 0.0e+0  5.0e-3  attention 3.0e-8
    bf16-KeyQuery-cat-degrees-B2N33G128K2P4-bf16        y 4.7e-4  4.0e-3  attention 1.2e-7
    bf16-GAT_origin-cat-hubs-B2N130G128K3P1-bf16        y 0.0e+0  3.5e-3  attention 4.5e-8
  CSR_TILED = 3, the tiled kernels
    tails-KeyQuery-cat-degrees-B2N33G32K2P4-f64         y 1.2e-7/1.3e-7/2.0e-5  row 2.4e-7/2.9e-7/3.0e-6  abs 1.1e-7  sum 1.0e-7
    tails-GAT_origin-mean-degrees-B2N33G128K2P2-f64     y 1.3e-8/1.9e-8/2.0e-5  row 1.2e-7/1.3e-7/3.0e-6  abs 4.6e-8  sum 8.9e-8
    tails-GAT_modified-mean-degrees-B3N65G256K2P4-noatt y 1.2e-7/1.1e-7/2.0e-5
    tails-KeyQuery-cat-degrees-B2N65G64K4P3             y 1.9e-7/2.6e-7/2.0e-5  row 3.7e-7/5.5e-7/3.0e-6  abs 1.8e-7  sum 1.0e-7
    degree-KeyQuery-cat-hubs-B2N130G64K3P2              y 4.1e-7/2.5e-7/2.0e-5  row 5.0e-7/5.1e-7/3.0e-6  abs 2.0e-7  sum 1.2e-7
    degree-GAT_modified-mean-hubs-B2N130G32K2P1         y 2.9e-7/3.3e-7/2.0e-5  row 1.7e-7/1.6e-7/3.0e-6  abs 5.8e-8  sum 1.0e-7
    degree-GAT_origin-cat-hubs-B2N130G64K3P4-f64        y 2.7e-8/1.9e-8/2.0e-5  row 1.7e-7/1.8e-7/3.0e-6  abs 3.5e-8  sum 1.3e-7
    degree-KeyQuery-mean-full-B1N70G128K2P3             y 1.5e-7/1.3e-7/2.0e-5  row 9.7e-7/1.3e-6/5.2e-6  abs 3.2e-7  sum 3.9e-7
    degree-GAT_modified-cat-full-B1N70G64K3P2           y 4.0e-7/2.4e-7/2.0e-5  row 1.7e-7/1.7e-7/3.0e-6  abs 3.2e-9  sum 1.3e-7
    degree-GAT_origin-mean-full-B1N70G32K2P4-noatt      y 1.1e-8/9.3e-9/2.0e-5
    degree-KeyQuery-cat-edgeless-B2N8G64K3P1            y 1.3e-7/2.3e-7/2.0e-5  row 0.0e+0/0.0e+0/3.0e-6  abs 0.0e+0  sum 0.0e+0
    degree-GAT_origin-cat-edgeless-B2N8G128K2P1         y 2.8e-8/5.4e-8/2.0e-5  row 0.0e+0/0.0e+0/3.0e-6  abs 0.0e+0  sum 0.0e+0
    degree-GAT_modified-cat-first_edgeless-B2N8G128K3P3 y 1.5e-7/2.7e-7/2.0e-5  row 1.6e-7/1.6e-7/3.0e-6  abs 3.4e-8  sum 1.2e-7
    degree-GAT_origin-mean-no_edge_row-B2N12G32K3P3     y 9.5e-9/9.5e-9/2.0e-5  row 1.3e-7/1.7e-7/3.0e-6  abs 2.5e-8  sum 8.2e-8
    depth-KeyQuery-cat-degrees-B2N33G32K1P2             y 1.5e-7/1.7e-7/2.0e-5  row 1.8e-7/3.9e-7/3.0e-6  abs 9.3e-8  sum 9.7e-8
    depth-KeyQuery-mean-rounds-B3N21G128K5P4            y 1.2e-7/1.5e-7/2.0e-5  row 5.0e-7/1.6e-6/6.2e-6  abs 2.3e-7  sum 1.3e-7
    depth-GAT_modified-cat-rounds-B3N21G256K4P3         y 3.3e-7/2.7e-7/2.0e-5  row 1.8e-7/1.9e-7/3.0e-6  abs 4.9e-8  sum 1.2e-7
    rounds-KeyQuery-cat-rounds-B9N10G32K3P3             y 1.4e-7/1.7e-7/2.0e-5  row 2.3e-7/3.5e-7/3.0e-6  abs 8.0e-8  sum 1.2e-7
    rounds-GAT_modified-mean-rounds-B17N10G64K2P2       y 1.7e-7/2.3e-7/2.0e-5  row 1.8e-7/1.6e-7/3.0e-6  abs 4.9e-8  sum 1.0e-7
    gnn-GNN-cat-degrees-B2N33G32K3P1F64-f64-noatt       y 1.4e-7/1.2e-7/2.0e-5
    tiled-KeyQuery-cat-hubs-B2N255G128K2P4              y 4.7e-7/4.6e-7/2.0e-5  row 6.2e-7/1.2e-6/4.6e-6  abs 2.3e-7  sum 4.4e-7
    tiled-KeyQuery-mean-dense-B2N513G64K3P1             y 2.9e-7/3.0e-7/2.0e-5  row 9.4e-7/1.6e-6/6.5e-6  abs 3.5e-7  sum 3.9e-7
    tiled-GAT_modified-cat-empty-B3N9G64K2P2            y 1.5e-7/2.0e-7/2.0e-5  row 9.6e-8/1.2e-7/3.0e-6  abs 3.9e-8  sum 6.0e-8
    tiled-GAT_origin-cat-hubs-B1N1024G32K3P2            y 3.7e-7/6.5e-8/2.0e-5  row 2.6e-7/1.8e-7/3.0e-6  abs 5.5e-8  sum 2.2e-7
    tiled-KeyQuery-cat-empty-B1N1024G256K4P1-f64        y 3.3e-7/2.3e-7/2.0e-5  row 1.0e-6/1.0e-6/4.1e-6  abs 5.9e-7  sum 1.1e-7
    tiled-GNN-cat-dense-B2N255G32K3P1F64-noatt          y 3.2e-7/1.9e-7/2.0e-5
  the same, bf16 storage
    bf16-GAT_modified-mean-degrees-B2N65G64K2P4-bf16    y 0.0e+0  5.0e-3  attention 3.0e-8
    bf16-KeyQuery-cat-degrees-B2N33G128K2P4-bf16        y 4.7e-4  4.0e-3  attention 1.2e-7
    bf16-GAT_origin-cat-hubs-B2N130G128K3P1-bf16        y 0.0e+0  3.5e-3  attention 4.5e-8
    tiled-KeyQuery-cat-hubs-B2N513G64K3P2-bf16          y 1.8e-4  4.4e-3  attention 4.8e-7
    tiled-GAT_modified-mean-dense-B3N9G128K2P4-bf16     y 0.0e+0  4.5e-3  attention 3.0e-8
  past 1024 agents, through the module
    past-KeyQuery-cat-past-B1N1025G32K3P2               y 4.6e-7/2.0e-7/2.0e-5  row 7.7e-7/4.0e-7/3.0e-6  abs 1.7e-7  sum 7.2e-7
    past-GAT_modified-mean-past-B1N1025G128K2P4-f64     y 7.5e-7/3.0e-7/2.0e-5  row 1.8e-7/2.0e-7/3.0e-6  abs 4.0e-8  sum 1.3e-7
    past-GAT_origin-cat-past-B1N1100G64K4P2             y 4.4e-7/8.5e-8/2.0e-5  row 1.8e-7/1.7e-7/3.0e-6  abs 3.5e-8  sum 1.3e-7
    past-KeyQuery-cat-past-B2N2048G256K2P1              y 1.1e-6/2.9e-7/2.0e-5  row 2.0e-6/3.7e-6/1.5e-5  abs 8.5e-7  sum 1.4e-6
    past-GAT_Similarity-cat-past-B1N1025G16K2P1         y 3.8e-7/3.3e-7/2.0e-5  row 2.1e-7/1.9e-7/3.0e-6  abs 4.9e-8  sum 1.7e-7
    past-GAT_Similarity-cat-past-B1N1025G64K3P1-f64     y 6.4e-7/3.0e-7/2.0e-5  row 4.9e-7/1.7e-7/3.0e-6  abs 3.7e-8  sum 4.8e-7
    past-GNN-cat-past-B1N1025G32K3P1F64-noatt           y 5.6e-7/2.3e-7/2.0e-5
    limit-GNN-cat-limit-B1N8190G16K2P1-noatt            y 9.0e-7/1.5e-7/2.0e-5
    limit-KeyQuery-cat-limit-B1N8190G16K3P1             y 1.1e-6/1.7e-7/2.0e-5  row 2.7e-6/4.7e-7/3.0e-6  abs 1.5e-7  sum 2.9e-6
    limit-GAT_origin-cat-limit-B1N8190G16K2P1           y 4.5e-7/2.0e-7/2.0e-5  row 9.6e-7/2.2e-7/3.0e-6  abs 5.6e-8  sum 9.4e-7
  the same, bf16 storage
    past-KeyQuery-cat-past-B1N1025G128K2P4-bf16         y 2.3e-4  4.2e-3  attention 3.6e-5
    past-KeyQuery-cat-past-B1N2048G64K2P2-bf16          y 9.1e-5  4.3e-3  attention 1.5e-5
  training past 1024 agents: error/max(1, max|want|) per tensor, gate 2e-4
    past-KeyQuery-cat-past-B1N1025G32K3P2               y 5.4e-7  dx 4.2e-7  filterWeight 9.2e-7  bias 1.4e-7  weight 1.2e-6
    past-GAT_Similarity-cat-past-B1N1025G16K2P1         y 3.8e-7  dx 3.6e-7  dx[clamped rows] 2.0e-7  weight 8.1e-7  filterWeight 6.6e-7
                                                        bias 1.1e-7
    past-GNN-cat-past-B1N1025G32K3P1F64-noatt           y 5.6e-7  dx 7.3e-7  weight 1.1e-6  bias 8.5e-8
    past-GAT_origin-mean-past-B1N1025G64K2P2            y 7.7e-8  dx 1.9e-8  mixer 1.7e-7  weight 1.3e-6  filterWeight 4.8e-6  bias 6.7e-8
    limit-KeyQuery-cat-limit-B1N8190G16K3P1             y 1.1e-6  dx 1.0e-6  filterWeight 1.8e-6  bias 1.1e-7  weight 6.4e-6
  raw entry points at N = 8190, of max(1, max|want|): float32 1.5e-7, bf16 4.9e-3 (budget 2e-2), GraphFilterBatch 1.5e-7
  whole models at N = 1025, max|dlogit|: float32 storage 2.1e-7, bf16 storage 1.2e-3 of scale 1 with every argmax equal; bottleneck GNN
    7.2e-7 of scale 2.78
The 8190-edge row of limit-KeyQuery is the one case near a gate (2.7e-6 of 3.0e-6): csr_scores_kernel carries that row's softmax sum
as ONE float32 running sum over 8190 terms per lane group, and its row sum is off by 2.9e-6 accordingly; the results are
bit-repeatable, so the margin does not move from run to run."""
import ctypes

import pytest
import torch

import large_graph_cases as lg
import similarity_train_cases as sc
from test_gpu_train_graph_shapes import _device_pass, _ran

pytestmark = pytest.mark.gpu
FORCED_IDS, TILED_IDS, INFER_IDS, TRAIN_IDS = list(lg.FORCED), list(lg.TILED), lg.LARGE_INFER, lg.LARGE_TRAIN
UNSUPPORTED = -2
ONE_LAUNCH = "gat_layer (one launch)"


def _nat():
    from magat_pathplanning_amd import _native as nat
    return nat


def _forms(name):
    nat = _nat()
    return int(nat.lib().magat_form_count(nat.FORMS[name]))


def _graph_launches(k, att):
    """Launches under tag gat_graph: the score kernel (GraphFilterBatch has none; at K = 1 only when the attention is asked for)
    and one hop kernel per tap behind the first (csr_k1_kernel carries no tag)."""
    scores = 0 if k.mode == lg.GNN or (k.K == 1 and not att) else 1
    return scores + k.K - 1


def _check_tags(cid, k, tc, att, transposed):
    """Nothing but the split CSR form ran: its graph kernels, the maps GEMM, the head mean where the heads are averaged, the
    in-call transpose exactly where the caller brought no column view - no fused form, no one-launch kernel."""
    want = {"gat_graph": _graph_launches(k, att), "head_mean": 0 if k.concat or k.mode == lg.GNN else 1,
            "gso_to_csr": 1 if transposed and k.K > 1 else 0, ONE_LAUNCH: 0, "gnn_dense": 0}
    if k.mode != lg.SIM:
        want["gat_prepare"] = 0
    got = {name: tc[name] for name in want}
    assert got == want and tc["gat_maps_gemm"] >= 1 and (k.mode != lg.SIM or tc["gat_prepare"] >= 1), (cid, tc.counts)


def _rows_to_y(out, k):
    return out.float().view(k.B, k.N, -1).permute(0, 2, 1)


def _check_structure(r, rowptr, colidx, nnz):
    assert nnz == r.nnz
    assert torch.equal(rowptr.cpu().long(), lg.csr_rowptr(r)) and torch.equal(colidx[:nnz].cpu().long(), r.colidx)


def _check_values(cid, r, y, att, route):
    """y (B, width, N) and att (edges, P) | None of the device against the case's yardstick, at the gates of the module docstring;
    prints the figures first."""
    k = r.case
    ref = r.want["y"]
    if k.bf16:
        scale = float(ref.abs().max())
        e_emul = float((y.cpu() - r.emul["y"]).abs().max()) / scale
        e_fp32 = float((y.cpu().double() - ref).abs().max()) / scale
        line = "y %.2e of scale against the emulation (%.2e), %.2e against float64 (%.2e)" % (e_emul, lg.BF16_EMUL, e_fp32, lg.BF16_FP32)
        ok = e_emul <= lg.BF16_EMUL and e_fp32 <= lg.BF16_FP32
        if att is not None:
            a_emul = float((att.cpu() - r.emul["att"]).abs().max()) if r.nnz else 0.0
            a_sum = lg.attention_errors(att, r.emul["att"], r.rowid, k.B * k.N)[1]
            line += "  attention %.2e against the emulation (%.2e), row sums %.2e" % (a_emul, lg.BF16_ATT, a_sum)
            ok = ok and a_emul <= lg.BF16_ATT and a_sum <= lg.ATT_SUM
    else:
        err = lg.y_error(y, ref)
        line = "y %.2e / %.2e / %.2e" % (err, r.f32_y, r.y_gate)
        ok = err <= r.y_gate
        if att is not None:
            a_abs, a_sum, a_row = lg.attention_errors(att, r.want["att"], r.rowid, k.B * k.N)
            line += "  attention per row %.2e / %.2e / %.2e  abs %.2e  row sums %.2e" % (a_row, r.f32_att[2], r.att_gate, a_abs, a_sum)
            ok = ok and a_abs <= lg.ATT_ABS and a_sum <= lg.ATT_SUM and a_row <= r.att_gate
    print("%s [%s]: %s" % (cid, route, line))
    assert bool(torch.isfinite(y).all()) and ok, (cid, route, line)


def _run_rows_case(cid, tiled, dev, libopt, tag_counts):
    """One case through gat_forward_rows_csr (GraphFilterBatch: through its module) under CSR_TILED = tiled: with the column view
    of a CsrStructure and without (the in-call transpose and sort), twice each, all four bit-identical."""
    from magat_pathplanning_amd.graphml import CsrStructure, dense_gso_to_csr, gat_forward_rows_csr
    nat = _nat()
    r = lg.reference(cid)
    k = r.case
    libopt.set("CSR_TILED", tiled)
    libopt.set("CSR_FUSED", 0)
    assert nat.get_option("CSR_TILED") == tiled and nat.get_option("CSR_FUSED") == 0
    route = "tiled" if tiled else "per-edge"
    fused, cos = _forms("csr_fused"), _forms("gat_cos_train")
    layer = lg.make_layer(k, r.state).to(dev).eval()
    S = r.S.to(dev)
    rowptr, colidx, nnz = dense_gso_to_csr(S, self_loops=layer.edge_rule)
    _check_structure(r, rowptr, colidx, nnz)
    runs = []
    if k.mode == lg.GNN:
        layer.addGSO(S.unsqueeze(1))
        x = r.x.to(dev)
        for _ in range(2):
            with torch.no_grad(), tag_counts() as tc:
                y = layer(x).clone()
            _check_tags(cid, k, tc, False, True)
            runs.append((y, None))
        y, att = runs[0][0], None
    else:
        st = CsrStructure().build(S.clone(), layer.edge_rule)
        assert st.ready(dev) == r.nnz
        _check_structure(r, st.rowptr, st.colidx, r.nnz)
        X = r.x.permute(0, 2, 1).contiguous().to(dev)
        if k.bf16:
            X = X.to(torch.bfloat16)
        for view in ((st.rowptr, st.colidx, (st.cscptr, st.csc[0], st.csc[1])), (rowptr, colidx, None)):
            for _ in range(2):
                with torch.no_grad(), tag_counts() as tc:
                    out, a = gat_forward_rows_csr(X, view[0], view[1], nnz, layer, want_attention=k.att, csc=view[2])
                _check_tags(cid, k, tc, k.att, view[2] is None)
                assert out.dtype == X.dtype and out.shape == (k.B * k.N, lg.out_width(k))
                runs.append((out.clone(), None if a is None else a.clone()))
        y = _rows_to_y(runs[0][0], k)
        att = None if runs[0][1] is None else runs[0][1][:, :nnz].t().contiguous()
    for out, a in runs[1:]:
        assert torch.equal(out, runs[0][0]), (cid, route, "y differs between runs / between the two column views")
        assert (a is None) == (runs[0][1] is None) and (a is None or torch.equal(a[:, :nnz], runs[0][1][:, :nnz])), (cid, route)
    assert _forms("csr_fused") == fused and _forms("gat_cos_train") == cos
    _check_values(cid, r, y, att, route)
    if k.distinct:
        assert all(not torch.equal(y[a], y[b]) for a in range(k.B) for b in range(a + 1, k.B))


@pytest.mark.parametrize("cid", FORCED_IDS)
def test_forced_per_edge_kernels_match_float64(gpu_device, libopt, tag_counts, cid):
    """CSR_TILED = 0: csr_scores_kernel / csr_hop_kernel / csr_k1_kernel at their tile tails, degrees 0 ... N, every width, mode
    and depth, instance rounds, GraphFilterBatch and the bf16 instantiations."""
    _run_rows_case(cid, 0, gpu_device, libopt, tag_counts)


@pytest.mark.parametrize("cid", TILED_IDS)
def test_tiled_kernels_match_float64(gpu_device, libopt, tag_counts, cid):
    """CSR_TILED = 3: csr_tiled_scores_kernel / csr_tiled_hop_kernel on the forced cases they accept and on hubs, dense and
    half-empty graphs at N = 9, 255, 513, 1024 - against float64 this time, not against their siblings."""
    _run_rows_case(cid, 3, gpu_device, libopt, tag_counts)


@pytest.mark.parametrize("cid", INFER_IDS)
def test_layers_past_1024_agents_match_float64(gpu_device, tag_counts, cid):
    """addGSO + forward of the module in eval mode, return_attention off and on, twice each: the structure comes from
    dense_gso_to_csr, the column view from the in-call transpose, the kernels are the per-edge ones."""
    from magat_pathplanning_amd.graphml import CsrStructure
    r = lg.reference(cid)
    k = r.case
    dev = gpu_device
    assert k.N > lg.TILED_MAX_N and not CsrStructure.supported(k.B, k.N)
    fused, cos = _forms("csr_fused"), _forms("gat_cos_train")
    layer = lg.make_layer(k, r.state).to(dev).eval()
    if k.bf16:
        layer.storage_dtype = torch.bfloat16
    layer.addGSO(r.S.unsqueeze(1).to(dev))
    x, mask = r.x.to(dev), r.mask.to(dev)
    ys, atts = [], []
    for want_att in ((False,) if k.mode == lg.GNN else (False, True)):
        layer.return_attention = want_att
        for _ in range(2):
            with torch.no_grad(), tag_counts() as tc:
                y = layer(x)
            _check_tags(cid, k, tc, want_att, True)
            assert y.dtype == torch.float32 and y.shape == (k.B, lg.out_width(k), k.N)
            ys.append(y.clone())
            if want_att:
                aij = layer.aij
                assert aij.shape == (k.B, k.P, 1, k.N, k.N)
                edges = aij[:, :, 0].permute(0, 2, 3, 1)[mask]
                assert int(torch.count_nonzero(aij)) == int(torch.count_nonzero(edges)), (cid, "attention off the edges")
                atts.append(edges)
                del aij
                layer.aij = None
    assert all(torch.equal(y, ys[0]) for y in ys[1:]), (cid, "y differs from run to run or with return_attention")
    assert all(torch.equal(a, atts[0]) for a in atts[1:]), (cid, "attention differs from run to run")
    assert _forms("csr_fused") == fused and _forms("gat_cos_train") == cos
    _check_values(cid, r, ys[0], atts[0] if atts else None, "module")


@pytest.mark.parametrize("cid", TRAIN_IDS)
def test_training_past_1024_agents_matches_float64(gpu_device, tag_counts, cid):
    """One forward + backward in train() mode through the HIP training kernels against the float64 yardstick: y, dx and every
    parameter gradient at the gate of the training tests, twice, bit-identical."""
    r = lg.reference(cid)
    k = r.case
    dev = gpu_device
    node = {lg.SIM: "_GatCosTrainFunctionBackward", lg.GNN: "_GnnTrainFunctionBackward"}.get(k.mode, "_GatTrainFunctionBackward")
    kw = {"hip_backward": True} if k.mode == lg.SIM else {}
    layer = lg.make_layer(k, r.state, **kw).to(dev).train()
    layer.addGSO(r.S.unsqueeze(1).to(dev))
    cos = _forms("gat_cos_train")
    passes = []
    for _ in range(2):
        with tag_counts() as tc:
            passes.append(_device_pass(layer, r, dev, node))
        assert tc["gat_graph"] > 0 and tc["gat_maps_gemm"] > 0 and tc[ONE_LAUNCH] == 0, (cid, tc.counts)
        assert (tc["gat_prepare"] > 0) == (k.mode == lg.SIM), (cid, tc.counts)
    assert _forms("gat_cos_train") == cos + (2 if k.mode == lg.SIM else 0)
    got, again = passes
    assert got["y"].shape == (k.B, lg.out_width(k), k.N)
    want = {n: t for n, t in r.want.items() if n != "att"}
    sc.compare(cid, got, want, r.clamped, gate=lg.TRAIN_GATE, again=again)
    if k.tiny:
        assert float(got["dx"][r.clamped.unsqueeze(1).expand_as(got["dx"])].abs().max()) > 1e6


STRUCTURE = [(N, rule, f64) for N in (1025, 2048, lg.MAX_N) for rule in (0, 1, 2) for f64 in (False, True)]


@pytest.mark.parametrize("N,rule,f64", STRUCTURE)
def test_dense_gso_to_csr_matches_the_definition_past_1024_agents(gpu_device, N, rule, f64):
    """magat_gso_row_degrees / magat_gso_fill_csr, the structure of every graph past the one-pass builder: rowptr and colidx exactly
    those of the definition made with torch on the host, every edge rule and GSO dtype, with a row of degree N, empty rows, the
    two rule-sensitive entries and edges in column N - 1 (the last, short 64-lane chunk of a row)."""
    from magat_pathplanning_amd.graphml import CsrStructure, dense_gso_to_csr
    assert CsrStructure.supported(1, 1024) and not CsrStructure.supported(1, N)
    S = lg.gso_structure(1, N, 6000 + N)
    if not f64:
        S = S.float()
    m = lg.edge_mask(S, {0: lg.KQ, 1: lg.GO, 2: lg.GNN}[rule])[0]
    assert int(m[3].sum()) == N and bool(m[30, N - 1]) and bool(m[20, 21]) == (rule == 2)
    assert int(m[41].sum()) == (1 if rule == 1 else 0)          # an empty row (GAT_origin's rule: its self-loop alone)
    i, j = torch.nonzero(m, as_tuple=True)
    want_ptr = torch.zeros(N + 1, dtype=torch.int64)
    want_ptr[1:] = torch.cumsum(m.sum(1), 0)
    for _ in range(2):
        rowptr, colidx, nnz = dense_gso_to_csr(S.to(gpu_device), self_loops=rule)
        assert nnz == int(i.numel()) and rowptr.dtype == torch.int32 and colidx.dtype == torch.int32
        assert torch.equal(rowptr.cpu().long(), want_ptr)
        assert torch.equal(colidx[:nnz].cpu().long(), j)          # (row-major nonzero: ascending columns inside every row)


def _ring_inputs(entry, N, dev):
    """A ring i -> i + 1 of N agents for the raw entry points: G = F = 32, K = 2, one head; every buffer behind a sentinel."""
    from magat_pathplanning_amd import GraphFilterBatch, GraphFilterBatchAttentional
    from magat_pathplanning_amd.graphml import _packed_weights
    nat = _nat()
    lib = nat.lib()
    G, K = 32, 2
    g = torch.Generator().manual_seed(N)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(77)
        layer = (GraphFilterBatch(G, G, K) if entry == "gnn" else GraphFilterBatchAttentional(G, G, K, 1, attentionMode=lg.KQ)).to(dev)
    mode = nat.MODE_GNN if entry == "gnn" else nat.MODE_KEYQUERY
    X = (torch.randn(N, G, generator=g) * 0.5).to(dev)
    vals = torch.rand(N, generator=g).to(dev) + 0.5
    rowptr = torch.arange(N + 1, dtype=torch.int32, device=dev)
    colidx = ((torch.arange(N) + 1) % N).to(torch.int32).to(dev)
    with torch.cuda.device(dev):
        packed = _packed_weights(layer, dev, nat.current_stream(dev), G, G, K, 1, mode)
    size = (lib.magat_gat_csr_bf16_workspace_bytes if entry == "bf16" else lib.magat_gat_csr_workspace_bytes)(1, N, N, G, G, K, 1, mode, 1)
    assert size > 0
    ws = torch.full((size,), 0x5A, dtype=torch.uint8, device=dev)
    ws[:256] = 0                                          # the status block, zeroed by the caller
    bf16 = entry == "bf16"
    Y = torch.full((N, G), -7.0, dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
    att = torch.full((1, N), -7.0, dtype=torch.float32, device=dev)
    bias = layer.bias.detach().reshape(-1).contiguous()
    Xs = X.to(torch.bfloat16) if bf16 else X

    def call():
        with torch.cuda.device(dev):
            st = nat.current_stream(dev)
            if entry == "gnn":
                return lib.magat_gnn_forward_csr_f32(nat.ptr(X), nat.ptr(rowptr), nat.ptr(colidx), nat.ptr(vals), N, nat.ptr(packed),
                                                     nat.ptr(bias), nat.ptr(Y), G, nat.ptr(ws), size, 1, N, G, G, K, st)
            fn = lib.magat_gat_forward_csr_bf16 if bf16 else lib.magat_gat_forward_csr_f32
            return fn(nat.ptr(Xs), nat.ptr(rowptr), nat.ptr(colidx), N, nat.ptr(packed), nat.ptr(bias), nat.ptr(Y), G,
                      nat.ptr(att), nat.ptr(ws), size, 1, N, G, G, K, 1, mode, 1, st)

    # float64 on the host: every row has one edge, so its attention is 1 and y_j = [relu] (H_0 x_j + w H_1 x_{j-1} + b)
    Xd, prev = X.cpu().double(), torch.roll(X.cpu().double(), 1, 0)
    if entry == "gnn":
        H = layer.weight.detach().cpu().double()[:, 0]          # (F,K,G)
        want = Xd @ H[:, 0].t() + (prev * torch.roll(vals.cpu().double(), 1, 0).unsqueeze(1)) @ H[:, 1].t() + bias.cpu().double()
    else:
        H = layer.filterWeight.detach().cpu().double()[0, :, 0]
        want = torch.relu(Xd @ H[:, 0].t() + prev @ H[:, 1].t() + bias.cpu().double())
    return call, Y, att, ws, want


@pytest.mark.parametrize("entry", ["f32", "bf16", "gnn"])
def test_c_abi_takes_8190_agents_and_refuses_8191(gpu_device, tag_counts, entry):
    """magat_gat_forward_csr_f32 / magat_gat_forward_csr_bf16 / magat_gnn_forward_csr_f32 called directly: N = 8190 runs and is
    right, N = 8191 answers MAGAT_ERR_UNSUPPORTED with nothing launched and nothing written (tag counts, sentinels)."""
    dev = gpu_device
    call, Y, att, ws, want = _ring_inputs(entry, lg.MAX_N, dev)
    with tag_counts() as tc:
        rc = call()
    assert rc == 0 and tc["gat_graph"] == (1 if entry == "gnn" else 2) and tc["gso_to_csr"] == 1, (rc, tc.counts)
    err = float((Y.cpu().double() - want).abs().max()) / max(1.0, float(want.abs().max()))
    print("%s at N = %d: %.2e of max(1, max|want|)" % (entry, lg.MAX_N, err))
    assert err <= (lg.BF16_FP32 if entry == "bf16" else lg.Y_GATE)
    if entry != "gnn":
        assert bool((att == 1.0).all())
    call, Y, att, ws, _ = _ring_inputs(entry, lg.MAX_N + 1, dev)
    with tag_counts() as tc:
        rc = call()
    assert rc == UNSUPPORTED and tc.counts == {}, (rc, tc.counts)
    assert bool((Y == -7.0).all()) and bool((att == -7.0).all()) and bool((ws[256:] == 0x5A).all()) and not ws[:256].any()


def test_gat_model_at_1025_agents(gpu_device, tag_counts):
    """DecentralPlannerGATNet in eval mode at B = 1, N = 1025 - config 5's layer one agent past the one-pass structure builder and
    the fused form: addGSO only scrubs (no structure), the forward takes dense_gso_to_csr and the split per-edge kernels.  float32
    storage against the oracle at the model tolerance, bf16 storage at the budget of test_fused_model_matches_split_model_at_config5_shape."""
    from magat_pathplanning_amd import DecentralPlannerGATNet
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    from oracle import magat_oracle as orc
    B, N = 1, 1025
    cfg = make_config(num_agents=N, nGraphFilterTaps=2, nAttentionHeads=4, device=str(gpu_device))
    sd = orc.init_state_dict(cfg, seed=23)
    x, S = fov_states(B, N, seed=5), comm_gso(B, N, 160, seed=6)
    ref = orc.planner_forward(x, S.clone(), sd, cfg)
    scale = max(1.0, float(ref.abs().max()))
    fused = _forms("csr_fused")
    for storage in ("fp32", "bf16"):
        if storage == "bf16":
            cfg = make_config(num_agents=N, nGraphFilterTaps=2, nAttentionHeads=4, gat_storage="bf16", device=str(gpu_device))
        net = DecentralPlannerGATNet(cfg)
        net.load_state_dict(sd)
        net = net.to(gpu_device).eval()
        with torch.no_grad():
            net.addGSO(S.to(gpu_device))
            assert net._rt.csr.key is None                # the scrub-only branch: no structure at addGSO time
            net(x.to(gpu_device))                         # (weights folded, activation scales calibrated)
            with tag_counts() as tc:
                got = net(x.to(gpu_device)).cpu()
        assert tc["gat_graph"] == 2 and tc["gat_maps_gemm"] >= 1 and tc["gso_to_csr"] == 1 and tc[ONE_LAUNCH] == 0, tc.counts
        err = float((got - ref).abs().max())
        agree = float((got.argmax(1) == ref.argmax(1)).float().mean())
        print("N = 1025, %s storage: max|dlogit| %.3e of scale %.3g, argmax agreement %.4f" % (storage, err, scale, agree))
        if storage == "fp32":
            assert err <= 1e-4
        else:
            assert err <= 2e-2 * scale and agree >= 0.97
    assert _forms("csr_fused") == fused


def test_bottleneck_gnn_model_at_1025_agents(gpu_device, tag_counts):
    """DecentralPlannerBottleneckNet with GSO_mode = 'dist_GSO_one' at B = 1, N = 1025: the dense kernel declines, GraphFilterBatch's
    CSR route runs.  Yardstick: the same module on the CPU (test_large_graph_falls_back_to_csr_and_matches); gate 1e-4 of
    max(1, max|want|) - with every positive GSO entry turned into 1 the rows sum unnormalised neighbours, so the logits are not
    of order 1 as they are behind a normalised GSO."""
    import copy
    from magat_pathplanning_amd import DecentralPlannerBottleneckNet
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    B, N = 1, 1025
    cfg = make_config(num_agents=N, bottleneckMode="BottomNeck_only", CNN_mode="Default", bottleneckFeature=32, nGraphFilterTaps=3,
                      GSO_mode="dist_GSO_one", device="cpu")
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(9)
        cpu = DecentralPlannerBottleneckNet(copy.deepcopy(cfg)).eval()
    cfg.device = str(gpu_device)
    net = DecentralPlannerBottleneckNet(cfg)
    net.load_state_dict(cpu.state_dict())
    net = net.to(gpu_device).eval()
    x, S = fov_states(B, N, seed=4), comm_gso(B, N, 160, seed=5, dtype=torch.float64)
    with torch.no_grad():
        cpu.addGSO(S.clone())
    for p_ in cpu.parameters():
        p_.requires_grad_(True)
    with torch.enable_grad():
        want = cpu(x).detach()
    Sd = S.clone().to(gpu_device)
    with torch.no_grad(), tag_counts() as tc:
        net.addGSO(Sd)
        got = net(x.to(gpu_device)).cpu()
    one = S.clone()
    one[one > 0] = 1
    assert torch.equal(Sd.cpu(), one)                      # dist_GSO_one, in place
    assert tc["gnn_dense"] == 0 and tc["gat_graph"] == 2 and tc["gso_to_csr"] == 1, tc.counts
    err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
    print("bottleneck GNN at N = 1025: max|dlogit| %.3e of scale %.3g" % (err, scale))
    assert err <= 1e-4 * scale
