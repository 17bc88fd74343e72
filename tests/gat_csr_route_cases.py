"""The case matrix of the CSR graph layer's routes (tests/test_gpu_gat_csr_routes.py, tools/gat_csr_ab.py): the smallest shapes at
which a decision of csrc/gat_csr_route.h flips, built with the builders of tests/large_graph_cases.py; how a case is run through
the library, and what tests/gat_csr_route_restatement.py predicts for it."""
import functools

import torch

import gat_csr_route_restatement as cr
import large_graph_cases as lg
import train_graph_cases as tg

MODES = {lg.KQ: cr.KQ, lg.GM: cr.GAT_MODIFIED, lg.GO: cr.GAT_ORIGIN, lg.GNN: cr.GNN, lg.SIM: cr.SIMILARITY}
TAGS = dict(GSO_CSR="gso_to_csr", GAT_MAPS="gat_maps_gemm", GAT_PREPARE="gat_prepare", GAT_GRAPH="gat_graph", HEAD_MEAN="head_mean",
            GAT_CAST="gat_cast")
FORMS = dict(CSR_FUSED="csr_fused", GAT_COS_TRAIN="gat_cos_train")
BOTH, OFF = dict(CSR_TILED=3), dict(CSR_TILED=0)
PAST = "past-KeyQuery-cat-past-B1N1025G32K3P2"        # a case of large_graph_cases.py: one agent past the tiled kernels


def _c(variants, *a, group="route", **kw):
    k = lg._case(group, *a, **kw)
    k.variants = variants         # (column view brought, options) per run
    return k


def _infer_cases():
    deg, full = lg.gso_degrees, tg.gso_full
    plain = [(False, BOTH)]
    c = [  # N = 7 is below the tiled kernels whatever the option says, N = 8 the first they take
        _c([(False, BOTH), (True, BOTH)], lg.KQ, True, full, 2, 7, 32, 2, 2),
        _c([(False, BOTH), (False, OFF), (False, dict(CSR_TILED=1)), (False, dict(CSR_TILED=2))], lg.KQ, True, full, 2, 8, 32, 2, 2),
        # hop buffers: none (K = 2, above), one, two, two reused; head mean; a width the tiled kernels do not take
        _c([(False, BOTH), (True, OFF)], lg.KQ, False, deg, 3, 33, 64, 3, 2),
        _c(plain, lg.GM, True, deg, 2, 33, 32, 4, 1, att=False),
        _c(plain, lg.GO, True, deg, 2, 33, 16, 5, 2),
        # K = 1: scores + csr_k1_kernel when the attention is wanted, csr_k1_kernel alone when not
        _c(plain, lg.KQ, True, deg, 2, 33, 32, 1, 2),
        _c(plain, lg.KQ, True, deg, 2, 33, 32, 1, 2, att=False),
        _c([(False, BOTH), (False, OFF)], lg.GNN, True, deg, 2, 33, 32, 3, 1, F=64, att=False),
        _c(plain, lg.SIM, True, deg, 2, 33, 32, 2, 1, tiny=True),
        # bf16 storage with and without the column view; the fused form's shape with the option on and off, every head count
        _c([(False, BOTH), (True, BOTH)], lg.KQ, True, deg, 2, 33, 64, 2, 2, bf16=True)]
    c += [_c([(True, dict(CSR_FUSED=1)), (True, dict(CSR_FUSED=0)), (False, dict(CSR_FUSED=1))], lg.KQ, True, deg, 2, 33, 128, 2, P, bf16=True)
          for P in (1, 2, 4)]
    out = lg._index(c, 7000)
    past = lg.CASES[PAST]
    past.variants = [(False, BOTH)]
    out[PAST] = past
    return out


def _train_cases():
    c = [_c(None, mode, concat, lg.gso_degrees, 2, 33, 32, K, P, group="train", train=True, tiny=mode == lg.SIM)
         for mode, concat, P in ((lg.KQ, True, 2), (lg.GO, False, 2), (lg.SIM, True, 1)) for K in (1, 2, 3)]
    return lg._index(c, 7100)


INFER, TRAIN = _infer_cases(), _train_cases()


@functools.lru_cache(maxsize=None)
def reference(cid):
    if cid == PAST:
        return lg.reference(cid)
    r = lg.reference_of(INFER[cid] if cid in INFER else TRAIN[cid])
    k = r.case
    if k.bf16 and k.G == 128:       # the fused form rounds elsewhere: the oracle's emulation of ITS order
        from oracle import magat_oracle as orc
        r.emul_fused = orc.gat_layer_forward_bf16_fused(r.x, r.S.unsqueeze(1), r.state)[0]
    return r


def nat():
    from magat_pathplanning_amd import _native
    return _native


def set_options(libopt, opts):
    libopt.restore()
    for name, v in opts.items():
        libopt.set(name, v)
    return dict(cr.DEFAULT_OPT, **opts)


def route_input(k, nnz, csc, opt, dev, pas="infer", att=None):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    gnn = k.mode == lg.GNN
    return dict(B=k.B, N=k.N, nnz=nnz, G=k.G, F=k.F, K=k.K, P=k.P, mode=cr.KQ if pas == "train_cos" else MODES[k.mode],
                concat=1 if gnn or pas != "infer" else int(k.concat), ldy=lg.out_width(k), esz=2 if k.bf16 else 4, have_csc=csc,
                attention=bool(k.att if att is None else att), edge_vals=True, y_f32=False, x_aligned=True, opt=opt, cus=cus,
                **{"pass": pas})


def forms():
    n = nat()
    return {name: int(n.lib().magat_form_count(n.FORMS[f])) for name, f in FORMS.items()}


def counted(tag_counts, fn):
    """fn() -> (its result, launches per tag of TAGS, increments of the form counters of FORMS)"""
    before = forms()
    with torch.no_grad(), tag_counts() as tc:
        out = fn()
    after = forms()
    return out, {t: tc.counts.get(name, 0) for t, name in TAGS.items()}, {f: after[f] - before[f] for f in FORMS}


def workspace_exports(i):
    """the three exports at this call's scalars -> (float32 CSR, bf16 CSR, CSC in the call's storage type)"""
    lib = nat().lib()
    a = (i["B"], i["N"], i["nnz"], i["G"], i["F"], i["K"], i["P"], i["mode"], i["concat"])
    return (int(lib.magat_gat_csr_workspace_bytes(*a)), int(lib.magat_gat_csr_bf16_workspace_bytes(*a)),
            int(lib.magat_gat_csc_workspace_bytes(*a, 1 if i["esz"] == 2 else 0)))


def workspace_restated(i):
    a = (i["B"], i["N"], i["nnz"], i["G"], i["F"], i["K"], i["P"], i["mode"], i["concat"])
    return (cr.workspace_bytes(*a, 4, False, i["opt"]), cr.workspace_bytes(*a, 2, False, i["opt"]),
            cr.workspace_bytes(*a, i["esz"], True, i["opt"]))


class Infer:
    """One inference case on the device: the layer, its rows, the CSR structure with and without the column view."""

    def __init__(self, cid, dev):
        from magat_pathplanning_amd.graphml import CsrStructure, dense_gso_to_csr
        self.r = r = reference(cid)
        self.k = k = r.case
        self.dev = dev
        self.layer = lg.make_layer(k, r.state).to(dev).eval()
        S = r.S.to(dev)
        if k.mode == lg.GNN:
            self.layer.addGSO(S.unsqueeze(1))
            self.x = r.x.to(dev)
            self.nnz = r.nnz
            return
        self.rowptr, self.colidx, self.nnz = dense_gso_to_csr(S, self_loops=self.layer.edge_rule)
        self.st = None
        if any(csc for csc, _ in k.variants):
            self.st = CsrStructure().build(S.clone(), self.layer.edge_rule)
            assert self.st.ready(dev) == self.nnz
        X = r.x.permute(0, 2, 1).contiguous().to(dev)
        self.X = X.to(torch.bfloat16) if k.bf16 else X
        torch.cuda.synchronize()

    def run(self, csc, tag_counts):
        """-> dict(y (B, width, N) float32, att (edges, P) | None, tags, forms)"""
        from magat_pathplanning_amd.graphml import gat_forward_rows_csr
        k = self.k
        if k.mode == lg.GNN:
            y, tags, fm = counted(tag_counts, lambda: self.layer(self.x).clone())
            return dict(y=y, att=None, tags=tags, forms=fm)
        view = (self.st.rowptr, self.st.colidx, (self.st.cscptr, self.st.csc[0], self.st.csc[1])) if csc else (self.rowptr, self.colidx, None)
        (out, a), tags, fm = counted(tag_counts, lambda: gat_forward_rows_csr(self.X, view[0], view[1], self.nnz, self.layer,
                                                                               want_attention=k.att, csc=view[2]))
        y = out.float().view(k.B, k.N, -1).permute(0, 2, 1).contiguous()
        return dict(y=y, att=None if a is None else a[:, :self.nnz].t().contiguous(), tags=tags, forms=fm)


class Train:
    """One training case through the C entries themselves: magat_gat_train_forward_f32 / _cos_f32 and their backward."""

    def __init__(self, cid, dev):
        from magat_pathplanning_amd.graphml import dense_gso_to_csr
        self.r = r = reference(cid)
        self.k = k = r.case
        self.dev = dev
        self.cos = k.mode == lg.SIM
        self.layer = lg.make_layer(k, r.state, **({"hip_backward": True} if self.cos else {})).to(dev).train()
        self.rowptr, self.colidx, self.nnz = dense_gso_to_csr(r.S.to(dev), self_loops=self.layer.edge_rule)
        self.X = r.x.permute(0, 2, 1).contiguous().to(dev)
        torch.cuda.synchronize()

    def run(self, tag_counts, seed_dy=5):
        """forward (counted) and backward on buffers of this call -> dict of rc, the kept tensors, tags and forms of the forward"""
        from magat_pathplanning_amd.graphml import _packed_cols, _packed_weights
        n, k, dev = nat(), self.k, self.dev
        lib, p = n.lib(), n.ptr
        B, N, G, K, P = k.B, k.N, k.G, k.K, k.P
        M, nnz = B * N, self.nnz
        mode = n.MODE_SIMILARITY if self.cos else MODES[k.mode]
        f32 = dict(dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = n.current_stream(dev)
            packed = _packed_weights(self.layer, dev, st, G, G, K, P, mode)
            NC = _packed_cols(self.layer.attentionMode, G, G, K, P)
            t = dict(Ypre=torch.empty(M, P * G, **f32), att=torch.empty(P, max(nnz, 1), **f32), Z=torch.empty(M, NC, **f32),
                     T=torch.empty(max(K - 2, 1), M, P * G, **f32), dZ=torch.empty(M, NC, **f32), dXd=torch.empty(M, G, **f32),
                     datt=torch.empty(P, max(nnz, 1), **f32))
            Xhat, norms = torch.empty(M, G, **f32), torch.empty(2, M, **f32)
            cscptr = torch.empty(B * (N + 1), dtype=torch.int32, device=dev)
            csc = torch.empty(3, max(nnz, 1), dtype=torch.int32, device=dev)
            bias = self.layer.bias.detach().reshape(-1).contiguous().float()
            Tp = p(t["T"]) if K > 2 else None
            head = (p(self.X), p(self.rowptr), p(self.colidx), nnz, p(packed), p(bias), p(t["Ypre"]), p(t["att"]), p(t["Z"]), Tp)
            tail = (p(cscptr), p(csc[0]), p(csc[1]), p(csc[2]), B, N, G)
            if self.cos:
                fwd = lambda: lib.magat_gat_train_forward_cos_f32(*head, p(Xhat), p(norms), *tail, K, st)
            else:
                fwd = lambda: lib.magat_gat_train_forward_f32(*head, *tail, G, K, P, mode, st)
            rc, tags, fm = counted(tag_counts, fwd)
            dY = torch.randn(M, P * G, generator=torch.Generator().manual_seed(seed_dy)).to(dev)
            struct = (p(self.rowptr), p(self.colidx), p(cscptr), p(csc[0]), p(csc[1]), nnz, p(t["dZ"]), p(t["dXd"]), p(t["datt"]), B, N, G)
            if rc == 0 and self.cos:
                rc_b = lib.magat_gat_train_backward_cos_f32(p(dY), p(Xhat), p(t["Z"]), p(t["att"]), Tp, p(norms), *struct, K, st)
            elif rc == 0:
                rc_b = lib.magat_gat_train_backward_f32(p(dY), p(self.X), p(t["Z"]), p(t["att"]), Tp, *struct, G, K, P, mode, st)
            else:
                rc_b = None
            torch.cuda.synchronize()
        if K <= 2:
            del t["T"]
        return dict(rc=rc, rc_backward=rc_b, tensors=t, tags=tags, forms=fm)

    def y_of(self, Ypre):
        """the layer's rows from the pre-activation per-head rows, as the module makes them"""
        k = self.k
        Yh = Ypre.view(k.B, k.N, k.P, k.G)
        y = torch.relu(Yh).reshape(k.B, k.N, k.P * k.G) if k.concat else torch.relu(Yh.mean(dim=2))
        return y.permute(0, 2, 1).contiguous()


def predicted(i):
    """(route, tags, forms) of an admitted call.  The float32 maps of the inference entries take the guarded split GEMM at these
    shapes (its re-run is booked under the range guard's tag, which the route does not speak of)."""
    r = cr.route(i)
    assert r["refusal"] == "none", (i, r["refusal"])
    return (r,) + cr.launches(r)


# ---- refused calls: one tiny ring, the scalars of the call varied; nothing is read or written before the answer ----------------
def refusal_calls():
    """[(name, entry, changes to the base call, workspace handed over or not)] - every refusal of the route, the workspace check
    in front of the late one, and every return code"""
    return [("dims", "f32", dict(K=0), True), ("mode", "f32", dict(mode=7), True), ("cosine", "f32", dict(mode=cr.SIMILARITY, P=2), True),
            ("gnn", "gnn", dict(G=30), True), ("shape", "f32", dict(G=48, F=48), True), ("agents", "f32", dict(N=cr.MAX_N + 1), True),
            ("ldy", "f32", dict(ldy_off=2), True), ("xalign", "f32", dict(x_off=1), True), ("bf16_maps", "bf16", dict(G=16, F=16), True),
            ("bf16_maps", "bf16", dict(G=16, F=16), False), ("none", "f32", dict(), False),
            ("grid", "train", dict(B=1 << 20, N=cr.MAX_N), True), ("agents", "train", dict(N=cr.MAX_N + 1), True),
            ("mode", "train", dict(mode=cr.GNN), True), ("shape", "train_cos", dict(G=48, F=48), True)]


class Ring:
    """Buffers of a ring of 16 agents, 32 features, K = 2, one head: big enough for every admitted variation of refusal_calls."""

    def __init__(self, dev):
        self.dev = dev
        self.base = dict(B=1, N=16, G=32, F=32, K=2, P=1, mode=cr.KQ, concat=1, nnz=16, ldy_off=0, x_off=0)
        f32 = dict(dtype=torch.float32, device=dev)
        self.X = torch.zeros(16 * 32 + 4, **f32)
        self.rowptr = torch.arange(17, dtype=torch.int32, device=dev)
        self.colidx = ((torch.arange(16) + 1) % 16).to(torch.int32).to(dev)
        self.vals = torch.ones(16, **f32)
        self.packed = torch.zeros(1 << 16, **f32)
        self.Y = torch.full((16, 64), -7.0, **f32)
        self.ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        self.scratch = torch.zeros(1 << 16, **f32)
        self.iscratch = torch.zeros(4, 64, dtype=torch.int32, device=dev)

    def call(self, entry, change, workspace, tag_counts):
        """-> (return code, launches in all, the restatement's route input)"""
        n = nat()
        lib, p = n.lib(), n.ptr
        c = dict(self.base, **change)
        B, N, G, F, K, P, mode, nnz = (c[x] for x in ("B", "N", "G", "F", "K", "P", "mode", "nnz"))
        ldy = P * F + c["ldy_off"]
        X = self.X[c["x_off"]:]
        size = self.ws.numel() if workspace else 256
        i = dict(B=B, N=N, nnz=nnz, G=G, F=F, K=K, P=P, mode=mode, concat=1, ldy=ldy, esz=2 if entry == "bf16" else 4, have_csc=False,
                 attention=False, edge_vals=True, y_f32=False, x_aligned=c["x_off"] == 0, opt=dict(cr.DEFAULT_OPT), cus=256,
                 **{"pass": entry if entry.startswith("train") else "infer"})
        with torch.cuda.device(self.dev):
            st = n.current_stream(self.dev)
            s, ip = self.scratch, self.iscratch
            with tag_counts() as tc:
                if entry == "gnn":
                    i["mode"] = cr.GNN
                    rc = lib.magat_gnn_forward_csr_f32(p(X), p(self.rowptr), p(self.colidx), p(self.vals), nnz, p(self.packed), None,
                                                       p(self.Y), ldy, p(self.ws), size, B, N, G, F, K, st)
                elif entry == "train":
                    rc = lib.magat_gat_train_forward_f32(p(X), p(self.rowptr), p(self.colidx), nnz, p(self.packed), None, p(s), p(s), p(s),
                                                         p(s), p(ip[0]), p(ip[1]), p(ip[2]), p(ip[3]), B, N, G, F, K, P, mode, st)
                elif entry == "train_cos":
                    rc = lib.magat_gat_train_forward_cos_f32(p(X), p(self.rowptr), p(self.colidx), nnz, p(self.packed), None, p(s), p(s),
                                                             p(s), p(s), p(s), p(s), p(ip[0]), p(ip[1]), p(ip[2]), p(ip[3]), B, N, G, K, st)
                else:
                    fn = lib.magat_gat_forward_csr_bf16 if entry == "bf16" else lib.magat_gat_forward_csr_f32
                    rc = fn(p(X), p(self.rowptr), p(self.colidx), nnz, p(self.packed), None, p(self.Y), ldy, None, p(self.ws), size,
                            B, N, G, F, K, P, mode, 1, st)
        return rc, sum(tc.counts.values()), i
