"""The case matrix of the dense graph layer's routes (tests/test_gpu_gat_routes.py, tools/gat_ab.py): shapes at the edges of every
size class, two configurations per shape, every option set; how a case is built, run through the C entry and predicted from
tests/gat_route_restatement.py."""
import ctypes

import torch

import gat_route_restatement as rr

OK, UNSUPPORTED = 0, -2
MODE_NAMES = {rr.KEYQUERY: "KeyQuery", rr.GAT_MODIFIED: "GAT_modified", rr.GAT_ORIGIN: "GAT_origin", rr.SIMILARITY: "GAT_Similarity"}
N256 = max(n for n in range(1, 129) if rr.dense_supported(n, 256, 256))      # the largest graph whose 256-wide tiles fit
SHAPES = ([(G, N) for G in (32, 64) for N in (1, 32, 33, 64, 65, 96, 97, 128)] +
          [(128, N) for N in (16, 32, 33, 64, 65, 102, 103, 105, 106, 128)] + [(16, 8), (256, N256), (256, N256 + 1)])
OPTION_SETS = ({}, {"RANGE_GUARD": 0}, {"GAT_MFMA": 0}, {"GAT_SPLIT": 0}, {"GAT_WIDE_FROM": 106}, {"GAT_PACK": 0}, {"GAT_PACK": 2},
               {"GAT_CHUNK_MB": 1})      # (1 MB: chunks of 8 instances wherever N x NC >= 32 K floats: B = 17 is 8 + 8 + 1)


def shape_id(s):
    return "G%d_N%d" % s


def configs(shape):
    """Two configurations per shape - KeyQuery, and the other modes in turn - with B, P, K and the merge cycling over the shapes
    so that every value meets every size class; B = 520 where the pack form exists; K = 1 on the two-launch-only widths."""
    G, N = shape
    i = SHAPES.index(shape)
    a = dict(G=G, N=N, mode=rr.KEYQUERY, B=(1, 3, 17)[i % 3], P=(4, 1)[i % 2], K=(2, 3)[(i // 2) % 2], concat=(i // 3) % 2)
    b = dict(G=G, N=N, mode=(rr.GAT_MODIFIED, rr.GAT_ORIGIN, rr.SIMILARITY, rr.KEYQUERY)[i % 4], B=(17, 1, 3)[i % 3], P=(1, 4)[i % 2],
             K=(3, 2)[(i // 2) % 2], concat=1 - (i // 3) % 2)
    if b["mode"] == rr.SIMILARITY:
        b["P"] = 1
    if G in (16, 256):
        b["K"] = 1
    out = [a, b]
    if G == 128 and N <= 32:
        out.append(dict(a, B=520, P=4))
    return out


def config_id(c):
    return "%s_B%d_P%d_K%d_%s" % (MODE_NAMES[c["mode"]], c["B"], c["P"], c["K"], "cat" if c["concat"] else "mean")


def _params(c, seed, small_weights=False):
    import test_gpu_abi_contract as abi
    if c["mode"] == rr.SIMILARITY:
        from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
        torch.manual_seed(seed)
        layer = GraphFilterBatchSimilarityAttentional(c["G"], c["G"], c["K"], 1, concatenate=bool(c["concat"]))
        return {k: v.detach().clone() for k, v in layer.state_dict().items()}
    p = abi._layer(c["G"], c["K"], c["P"], MODE_NAMES[c["mode"]], bool(c["concat"]), seed)
    if small_weights:      # (tests/test_gpu_range.py: the scores stay where float32 follows the reference)
        p["weight"] = p["weight"] * 1e-4
    return p


def reference(c, p, x, S):
    """float64 rows (B N, width) and the attention tensor (or None): oracle/magat_oracle.py; GAT_Similarity from the restatement
    tests/test_host_similarity.py pins on the reference's fixtures"""
    if c["mode"] == rr.SIMILARITY:
        from similarity_restatement import similarity_layer
        y, _ = similarity_layer(x.numpy(), S.numpy(), p["weight"].numpy(), p["filterWeight"].numpy(), p["bias"].numpy())
        y = torch.as_tensor(y).double()
        return y.permute(0, 2, 1).reshape(-1, y.shape[1]), None
    from oracle import magat_oracle as orc
    y, aij = orc.gat_layer_forward(x.double(), S.double().unsqueeze(1), {k: v.double() for k, v in p.items()},
                                   MODE_NAMES[c["mode"]], bool(c["concat"]))
    return y.permute(0, 2, 1).reshape(-1, y.shape[1]), aij


class Case:
    """one configuration on the device: inputs, packed weights, workspace, float64 reference"""

    def __init__(self, c, dev, clamp=False, want_ref=True):
        import test_gpu_abi_contract as abi
        from magat_pathplanning_amd import _native as nat
        self.c, self.dev, self.lib = c, dev, nat.lib()
        B, N, G, K, P, mode = (c[k] for k in ("B", "N", "G", "K", "P", "mode"))
        self.width, self.M = (P * G if c["concat"] else G), B * N
        x, S = abi._inputs(B, N, G, False, seed=G + N + K)
        if clamp:          # (tests/test_gpu_range.py: every seventh instance leaves the f16 range)
            x = x * (0.5 / 0.7)
            x[::7] *= 4.0e5
        self.p = _params(c, seed=N + P, small_weights=clamp)
        self.x, self.S = x, S
        self.ref, self.aij = reference(c, self.p, x, S) if want_ref else (None, None)
        self.packed, self.bias, _ = abi._pack(self.p, G, K, P, mode, dev)
        self.Sd = S.to(dev).contiguous()
        self.X = x.permute(0, 2, 1).reshape(self.M, G).contiguous().to(dev)
        self.cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def call_input(self, opts, attention=False, odd=False, tail=None):
        c = self.c
        return dict(B=c["B"], N=c["N"], G=c["G"], F=c["G"], K=c["K"], P=c["P"], mode=c["mode"], concat=c["concat"], attention=attention,
                    y_aligned=not odd, tail=tail is not None, tail_cout=5 if tail else 0, tail_m=self.M if tail else 0,
                    tail_k=self.width if tail else 0, opt=dict(rr.DEFAULT_OPT, **opts), conv_direct=True, cus=self.cus)

    def run(self, tag_counts, attention=False, odd=False, tail=False):
        """-> dict(rc, y, att, tags, forms, status, tail_done, logits); the options are the caller's business"""
        from magat_pathplanning_amd import _native as nat
        lib, c, dev = self.lib, self.c, self.dev
        B, N, G, K, P, mode, concat = (c[k] for k in ("B", "N", "G", "K", "P", "mode", "concat"))
        ws = torch.zeros(lib.magat_gat_workspace_bytes(B, N, G, G, K, P, mode, concat), dtype=torch.uint8, device=dev)
        ld = self.width + (12 if odd else 0)
        buf = torch.zeros(self.M + 1, ld, device=dev)
        yp = buf.data_ptr() + (4 if odd else 0)
        att = torch.zeros(B, P, 1, N, N, device=dev) if attention else None
        stream = torch.cuda.current_stream().cuda_stream
        head = (self.X.data_ptr(), self.Sd.data_ptr(), 0, self.packed.data_ptr(), self.bias.data_ptr(), yp, ld)
        shape = (ws.data_ptr(), ws.numel(), B, N, G, G, K, P, mode, concat)
        done, logits = ctypes.c_int(0), None
        if tail:
            g = torch.Generator().manual_seed(11)
            Wd = (torch.randn(5, self.width, generator=g) * 0.05).to(dev)
            bd = (torch.randn(5, generator=g) * 0.1).to(dev)
            logits = torch.full((self.M, 5), float("nan"), device=dev)
            d = nat.ConvGemmDesc()
            d.inp, d.Cin, d.lda = yp, self.width, ld
            d.wt, d.bias, d.out = Wd.data_ptr(), bd.data_ptr(), logits.data_ptr()
            d.M, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad, d.Hout, d.Wout = self.M, 1, 1, 1, 1, 1, 0, 1, 1
            d.Cout, d.ldc, d.relu, d.tag = 5, 5, 0, nat.TAG_ACTIONS
            self.tail_w = (Wd.cpu().double(), bd.cpu().double())
        lib.magat_form_reset()
        with tag_counts() as tc:
            if tail:
                rc = lib.magat_gat_forward_tail_f32(*head, *shape, ctypes.byref(d), ctypes.byref(done), stream)
            else:
                rc = lib.magat_gat_forward_packed_f32(*head, None if att is None else att.data_ptr(), *shape, stream)
        forms = {k: int(lib.magat_form_count(nat.FORMS[k])) for k in rr.COUNTERS}
        st = (ctypes.c_int32 * 2)()
        if rc == OK:
            nat.check(lib.magat_gat_read_status(ws.data_ptr(), st, stream), "magat_gat_read_status")
        col = 1 if odd else 0
        return dict(rc=rc, y=buf[:self.M, col:col + self.width].contiguous().cpu(), att=None if att is None else att.cpu(),
                    tags=dict(tc.counts), forms=forms, status=(int(st[0]), int(st[1])), tail_done=done.value,
                    logits=None if logits is None else logits.cpu())


def mismatches(route, got):
    """what the library did against what the restatement says: the return code; for an admitted call the launch counts of the
    layer's six tags and the five form counters"""
    if route["refusal"] != "none":
        bad = [] if got["rc"] == UNSUPPORTED else [("rc", got["rc"])]
        return bad + ([("launched", got["tags"])] if sum(got["tags"].values()) else [])
    if got["rc"] != OK:
        return [("rc", got["rc"])]
    tags, forms = rr.launches(route)
    bad = [(t, n, got["tags"].get(t, 0)) for t, n in tags.items() if got["tags"].get(t, 0) != n]
    return bad + [(k, n, got["forms"][k]) for k, n in forms.items() if got["forms"][k] != n]
