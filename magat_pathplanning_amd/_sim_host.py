"""The host side that the simulator / expert family shares (simulator.py, rollout.py, mapf.py, expert.py, cases.py, memory.py):
tensor intake - device tensors or MagatNativeError, never a CPU fallback -, workspaces, and the one way a native entry is called.
A new entry point of the family calls these; it does not write a copy."""
import torch

from . import _native as nat


CPU_REFUSAL = "%s must be a device tensor (no CPU fallback)"


# (the three spell the test out instead of calling one another: they stand on the per-step path of a closed loop)
def dev_tensor(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise nat.MagatNativeError(CPU_REFUSAL % name)
    return t


def dev_i32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise nat.MagatNativeError(CPU_REFUSAL % name)
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    return t.contiguous()


def dev_u8(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise nat.MagatNativeError(CPU_REFUSAL % name)
    return t.to(torch.uint8).contiguous()


def dev_map(obstacle_map, cases):
    """obstacle_map (H,W) or (cases,H,W), non-zero: obstacle -> (m uint8 contiguous, batched 0 / 1, H, W)"""
    m = dev_u8(obstacle_map, "obstacle_map")
    assert m.dim() in (2, 3) and (m.dim() == 2 or m.shape[0] == cases), "obstacle_map must be (H,W) or (C,H,W)"
    return m, 1 if m.dim() == 3 else 0, m.shape[-2], m.shape[-1]


def dev_cases(obstacle_map, start, goal):
    """The cases of a solver or a pool: start / goal (C,N,2) and their map -> (m, batched, start, goal, C, N, H, W)"""
    start, goal = dev_i32(start, "start"), dev_i32(goal, "goal")
    assert start.dim() == 3 and start.shape[2] == 2 and goal.shape == start.shape, "start and goal must be (C,N,2)"
    C, N, _ = start.shape
    m, batched, H, W = dev_map(obstacle_map, C)
    return m, batched, start, goal, C, N, H, W


def dev_schedules(obstacle_map, paths):
    """Schedules in pack_schedules' layout and the map they were planned on: paths (C,N,T,2), left in their dtype (a conversion
    is a launch, and the caller's limits come first) -> (m, batched, C, N, T, H, W)"""
    if not isinstance(obstacle_map, torch.Tensor) or not obstacle_map.is_cuda or not paths.is_cuda:
        raise nat.MagatNativeError("obstacle_map and the schedules must be device tensors (no CPU fallback)")
    assert paths.dim() == 4 and paths.shape[3] == 2, "paths must be (C,N,T,2)"
    C, N, T, _ = paths.shape
    m, batched, H, W = dev_map(obstacle_map, C)
    return m, batched, C, N, T, H, W


def dev_actions(logits, actions, B, N):
    """What a move step takes, the model's logits or ready actions -> (logits (B*N,5) float32 or None, actions (B*N,) int32 or
    None)"""
    assert (logits is None) != (actions is None), "give logits or actions"
    lg = None if logits is None else logits.reshape(B * N, 5).contiguous().float()
    ac = None if actions is None else dev_i32(actions, "actions").reshape(B * N)
    return lg, ac


def dev_uniforms(uniforms, B, N):
    if not uniforms.is_cuda or uniforms.dtype != torch.float64 or uniforms.numel() != B * N:
        raise nat.MagatNativeError("uniforms must be a (B,N) float64 device tensor")
    return uniforms.contiguous()


def scratch(nbytes, device):
    """A workspace of a size the library names (never empty: the entries refuse a null workspace)"""
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


class _Workspace:
    """A cached device buffer for the wide kernels: reallocated only when a call needs more than it holds."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.device != device or self.buf.numel() < nbytes:
            self.buf = scratch(nbytes, device)
        return self.buf


def call(dev, entry, *args, ws=None):
    """One checked native call on `dev`, on its current stream: entry(*args, stream).  With `ws`, the workspace the wide route of
    a narrow / wide pair needs, the wide form instead: it takes the narrow one's arguments and (workspace, bytes) in front of the
    stream - entry_wide(*args, ws, ws.numel(), stream)."""
    if ws is not None:
        entry, args = entry + "_wide", args + (nat.ptr(ws), ws.numel())
    with torch.cuda.device(dev):
        nat.check(getattr(nat.lib(), entry)(*args, nat.current_stream(dev)), entry)
