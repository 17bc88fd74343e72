"""The communication graph as an edge structure straight from agent positions (csrc/gso_edges.hip).

The attention layers read the GSO through its edge test only, and the simulator's GSO is a function of the positions:

    edges = batched_edges(pos, config.commR)          # or ep.edges() / pool.edges(): the radii the episode keeps
    net.addGSO(edges); logits = net(x)                # DecentralPlannerGATNet, up to 4096 agents

builds the arrays the CSR kernels take from the distance test - no (B,N,N) tensor, no eigenvalue, no second pass that recovers
the bits the simulator had before it divided.  The layers that multiply by the GSO's VALUES (GraphFilterBatch and the GNN planners)
take the same route with values=True: one more launch (csrc/gso_edge_values.hip) leaves lambda_max per instance and one float32
per edge on the structure's arrays.

    edges = batched_edges(pos, config.commR, values=True, symmetric_norm=...)       # or ep.edges(values=True)
    net.addGSO(edges); logits = net(x)                # DecentralPlannerNet, DecentralPlannerBottleneckNet

HIP only: CPU tensors raise MagatNativeError."""
import os

import torch

from . import _native as nat
from . import _sim_host as sh
from .graphml import CsrStructure

MAX_AGENTS = 4096            # csrc/gso_edges.hip: a lane per 64-column word of a row


class EdgeStructure(CsrStructure):
    """CsrStructure's arrays and capacity protocol (a guess of 32 edges per node, the true count copied to pinned memory
    behind the build, a re-build when the guess was too small) with magat_gso_edges_build as the builder: it reads positions
    and radii, never a GSO tensor.  rowptr, colidx, cscptr, csc, ready(dev), exact_nnz() are CsrStructure's."""

    @staticmethod
    def supported(B, N):
        return nat.lib().magat_gso_edges_workspace_bytes(B, N) > 0

    @staticmethod
    def _workspace_bytes(B, N):
        return nat.lib().magat_gso_edges_workspace_bytes(B, N)

    def build(self, pos, rule, radii=None, comm_radius=0.0, min_cap=0):
        """pos (B,N,2) contiguous int32 device tensor, radii (B,) float64 device tensor or None (then comm_radius)"""
        lib = nat.lib()
        B, N, _ = pos.shape
        dev = pos.device
        with torch.cuda.device(dev):
            if self.rowptr is not None and (self.rowptr.numel() != B * (N + 1) or self.rowptr.device != dev):
                self.cap = 0
            cap = max(self.cap, min(B * N * N, max(int(min_cap), 32 * B * N, 1 << 12)))
            if cap >= self._CAP_LIMIT:
                raise nat.MagatNativeError("an edge structure of %d entries: the CSR index arrays are int32" % cap)
            cur = torch.cuda.current_stream(dev)
            # the side stream and its switch are CsrStructure.build's: the build needs nothing but the positions, so it may run
            # under the per-agent CNN; the layer's kernels wait for its event
            side = os.environ.get("MAGAT_CSR_SIDE", "1") == "1"
            if side and self.side is None:
                self.side = torch.cuda.Stream(device=dev)
            run = self.side if side else cur
            if side:
                self.side.wait_stream(cur)
            self.run = run                           # (GraphEdges.values launches behind the build, on its stream)
            with torch.cuda.stream(run):
                self._alloc(B, N, cap, dev)          # (allocated under the stream that writes them)
                nat.check(lib.magat_gso_edges_build(
                    nat.ptr(pos), nat.ptr(radii), float(comm_radius), int(rule), nat.ptr(self.rowptr), nat.ptr(self.colidx),
                    nat.ptr(self.cscptr), nat.ptr(self.csc[0]), nat.ptr(self.csc[1]), self.cap, nat.ptr(self.nnz_dev),
                    nat.ptr(self.ws), self.ws.numel(), B, N, nat.current_stream(dev)), "magat_gso_edges_build")
                self.nnz_host.copy_(self.nnz_dev, non_blocking=True)
                self.event = run.record_event()
            if side:
                pos.record_stream(self.side)
                if radii is not None:
                    radii.record_stream(self.side)
                for t in (self.rowptr, self.colidx, self.cscptr, self.csc, self.nnz_dev, self.ws):
                    t.record_stream(cur)             # (read by the layer's kernels on the caller's stream)
        self.key = None                              # (CsrStructure.matches keys on a GSO tensor: never a match)
        self.args = (pos, rule, radii, comm_radius)  # kept until ready(): a re-build reads the positions once more
        self.nnz = None
        return self

    def ready(self, dev):
        nnz = super().ready(dev)
        if nnz >= self._CAP_LIMIT:
            raise nat.MagatNativeError("a graph of %d edges: the CSR index arrays are int32" % nnz)
        return nnz


class GraphEdges:
    """The communication graph of B instances, kept as positions and radii; what DecentralPlannerGATNet.addGSO takes in place of
    the GSO tensor (batched_edges, BatchedEpisode.edges, EpisodePool.edges).

    structure(rule)   the EdgeStructure under edge rule 0 (KeyQuery, GAT_modified: no self-loops) or 1 (GAT_origin,
                      GAT_Similarity: every (i, i) added) - built at the first request, on the side stream, and kept per rule
    dense(dtype)      the 0 / 1 adjacency (B,N,N) without the diagonal, for the routes that need a tensor
    refresh()         the positions (or radii) were changed in place: what was built is stale.  The index arrays are kept and
                      reused by the next build.

    values=True (with symmetric_norm as batched_gso takes it) marks the graph as one whose VALUES may be asked for - what
    GraphFilterBatch and the GNN planners accept in addGSO; the attention models treat it like a plain one:
    values()          (the rule-0 EdgeStructure, vals float32 [cap] in CSR order, lam (B,) float64): batched_gso's GSO on the
                      structure's arrays, by magat_gso_edge_values - W / lambda_max(W), or D^-1/2 W D^-1/2 / lambda_max
    gso(dtype)        batched_gso's tensor of the same graph, for the routes that need one (its limit: 2048 agents)"""

    def __init__(self, pos, radii=None, comm_radius=None, values=False, symmetric_norm=False):
        self.pos, self.radii = pos, radii
        self.comm_radius = 0.0 if comm_radius is None else float(comm_radius)
        self.B, self.N = int(pos.shape[0]), int(pos.shape[1])
        self.device = pos.device
        self.valued, self.symmetric_norm = bool(values), bool(symmetric_norm)
        self._structures = {}
        self._fresh = set()
        self._values = {}            # normalize -> (event of the structure's build they belong to, vals, lam)
        self._value_ws = None

    def refresh(self):
        self._fresh.clear()
        self._values.clear()
        return self

    def structure(self, rule=0):
        rule = int(rule)
        if rule not in (0, 1):
            raise ValueError("edge rule must be 0 or 1 (the layers that read the GSO's values take batched_gso), got %r" % (rule,))
        st = self._structures.get(rule)
        if st is None:
            st = self._structures[rule] = EdgeStructure()
        if rule not in self._fresh:
            st.build(self.pos, rule, self.radii, self.comm_radius)
            self._fresh.add(rule)
        return st

    def values(self, normalize=True):
        """-> (structure, vals, lam).  Launched on the stream the structure was built on, right behind the build and before its
        edge count is known on the host; kept until refresh().  Where the count exceeds the capacity guess, ready() re-builds the
        structure and the values are launched again behind that build (the kernel walks no instance that reaches beyond the
        capacity).  normalize=False: no eigenvalue, every value is 1 (the planners' GSO_mode 'dist_GSO_one'), lam is 0.
        The current stream is ordered behind the launch."""
        if not self.valued:
            raise ValueError("values() needs a GraphEdges made with values=True")
        normalize = bool(normalize)
        st = self.structure(0)
        dev = self.device
        hit = self._values.get(normalize)
        if hit is None or hit[0] is not st.event:
            hit = self._launch_values(st, normalize)
        st.ready(dev)                                # the host wait for the edge count; may re-build
        if hit[0] is not st.event:
            hit = self._launch_values(st, normalize)
        torch.cuda.current_stream(dev).wait_event(hit[3])
        return st, hit[1], hit[2]

    def _launch_values(self, st, normalize):
        lib = nat.lib()
        B, N, dev = self.B, self.N, self.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            run = st.run
            with torch.cuda.stream(run):
                # fresh vals and lam per launch (a training step may still hold the last ones for its backward); the workspace
                # is the kernel's own scratch, reused: launches on this stream run one after another
                vals = torch.empty(st.cap, dtype=torch.float32, device=dev)
                lam = torch.empty(B, dtype=torch.float64, device=dev)
                need = lib.magat_gso_edge_values_workspace_bytes(B, N)
                if self._value_ws is None or self._value_ws.numel() < need or self._value_ws.device != dev:
                    self._value_ws = torch.empty(need, dtype=torch.uint8, device=dev)
                # the plain form and 'every value is 1' are the kernel's symmetric_norm = 0
                sym = 1 if self.symmetric_norm and normalize else 0
                nat.check(lib.magat_gso_edge_values(
                    nat.ptr(st.rowptr), nat.ptr(st.colidx), nat.ptr(st.nnz_dev), st.cap, sym, 1 if normalize else 0, nat.ptr(lam),
                    nat.ptr(vals), nat.ptr(self._value_ws), self._value_ws.numel(), B, N, nat.current_stream(dev)),
                    "magat_gso_edge_values")
                done = run.record_event()
            if run is not cur:
                for t in (vals, lam, self._value_ws):
                    t.record_stream(cur)
        hit = self._values[normalize] = (st.event, vals, lam, done)
        return hit

    def gso(self, dtype=torch.float64):
        """batched_gso's tensor of this graph (B,N,N): its radii or radius, its symmetric_norm."""
        from .simulator import batched_gso
        return batched_gso(self.pos, self.radii if self.radii is not None else self.comm_radius,
                           symmetric_norm=self.symmetric_norm, dtype=dtype)

    def dense(self, dtype=torch.float32):
        st = self.structure(0)
        B, N, dev = self.B, self.N, self.device
        nnz = st.ready(dev)
        out = torch.zeros(B * N, N, dtype=dtype, device=dev)
        if nnz:
            rp = st.rowptr.view(B, N + 1).long()
            rows = torch.repeat_interleave(torch.arange(B * N, device=dev), (rp[:, 1:] - rp[:, :-1]).reshape(-1), output_size=nnz)
            out[rows, st.colidx[:nnz].long()] = 1
        return out.view(B, N, N)


def batched_edges(pos, comm_radius, values=False, symmetric_norm=False):
    """pos (B,N,2) integer agent coordinates (row, col) on the device, comm_radius one number or a (B,) float64 device tensor
    of per-instance radii - batched_gso's arguments -> GraphEdges.  N <= 4096.  Nothing is launched here.
    values=True: the graph may be asked for the GSO's values (GraphEdges.values; symmetric_norm as batched_gso's) - what the GNN
    classes' addGSO takes."""
    if not isinstance(pos, torch.Tensor) or pos.dim() != 3 or pos.shape[2] != 2 or pos.shape[0] < 1 or pos.shape[1] < 1:
        raise ValueError("pos must be a (B,N,2) tensor, got %s" % (tuple(pos.shape) if isinstance(pos, torch.Tensor) else type(pos),))
    B, N, _ = pos.shape
    if N > MAX_AGENTS:
        raise nat.MagatNativeError("batched_edges takes up to %d agents, got %d" % (MAX_AGENTS, N))
    pos = sh.dev_i32(pos, "pos")
    if isinstance(comm_radius, torch.Tensor):
        if not comm_radius.is_cuda or comm_radius.dtype != torch.float64 or comm_radius.numel() != B:
            raise nat.MagatNativeError("per-instance radii must be a (B,) float64 device tensor")
        return GraphEdges(pos, radii=comm_radius.contiguous().reshape(-1), values=values, symmetric_norm=symmetric_norm)
    if not float(comm_radius) > 0.0:
        raise ValueError("comm_radius must be > 0, got %r" % (comm_radius,))
    return GraphEdges(pos, comm_radius=comm_radius, values=values, symmetric_norm=symmetric_norm)
