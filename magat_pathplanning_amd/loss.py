"""The training loss of the reference's agent on the HIP kernels (csrc/head_loss.hip).

agents/decentralplannerlocal_OnlineExpert_GAT.py:103-107 trains with nn.CrossEntropyLoss() or, when config.label_smoothing != 0,
with graphs/losses/label_smoothing.py: LogSoftmax + KLDivLoss(size_average=False) against a smoothed one-hot (1 - s on the
target, s / 4 on the four other actions) - a SUM over the rows that includes the target distribution's entropy term.

  head_loss(x, weight, bias, target, label_smoothing)   the last Linear of actionsMLP (width -> 5) fused with the loss: forward in
                                                        one pass over the head's input rows, backward in one more
                                                        (magat_head_loss_forward_f32 / _backward_f32)
  ActionLoss(label_smoothing)                           drop-in for the agent's self.loss: crit(logits, target) on logits that
                                                        something else produced (magat_action_loss_f32)
  loss_composite(logits, target, label_smoothing)       the same semantics in torch ops: the reference the host tests pin

The kernels take CUDA float32 rows of a width that is a multiple of 4, at most 1024; the composite covers everything else (CPU
tensors - under nat.require_device_or_composite's rule -, float64, other widths, rows the kernels' row stride cannot describe).
"""
import torch
import torch.nn as nn
import torch.nn.functional as tnf

from . import _native as nat

CLASSES = 5            # the reference's action count (csrc/head_loss.hip is built for it)
MAX_WIDTH = 1024


def as_indices(target):
    """(M,) int64 class indices from indices of any integer type, or from one-hot rows (M, 5) / (B, N, 5) reduced with argmax(-1)
    like the reference's torch.max(target, 1)[1]."""
    if target.dim() == 1:
        return target.long()
    return target.reshape(-1, target.shape[-1]).argmax(-1)


def _smoothing(label_smoothing):
    s = 0.0 if label_smoothing is None else float(label_smoothing)
    if not 0.0 <= s < 1.0:
        raise ValueError("label_smoothing must be in [0, 1), got %r" % (label_smoothing,))
    return s


def loss_composite(logits, target, label_smoothing=0.0):
    """label_smoothing == 0: nn.CrossEntropyLoss() (a mean over the rows); > 0: the reference's LabelSmoothing(C, s) (a sum)."""
    s = _smoothing(label_smoothing)
    target = as_indices(target)
    if s == 0.0:
        return tnf.cross_entropy(logits, target)
    logp = torch.log_softmax(logits, dim=1)
    q = torch.full_like(logp, s / (logits.shape[1] - 1)).scatter_(1, target.unsqueeze(1), 1.0 - s)
    return tnf.kl_div(logp, q, reduction="sum")


def _rows_ok(t, width):
    """rows of `width` float32 the kernels can walk: unit column stride, a row stride that keeps every row 16-byte aligned"""
    return (t.dim() == 2 and t.shape[0] > 0 and t.shape[1] == width and t.stride(1) == 1 and t.stride(0) >= width and
            t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0)


def _workspace(M, width, dev):
    return torch.empty(nat.lib().magat_head_loss_workspace_floats(M, width), dtype=torch.float32, device=dev)


class _HeadLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, target, smoothing):
        lib = nat.lib()
        M, width = x.shape
        dev = x.device
        w = weight.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        logits = torch.empty(M, CLASSES, dtype=torch.float32, device=dev)
        dlogits = torch.empty(M, CLASSES, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = _workspace(M, width, dev)
        with torch.cuda.device(dev):
            nat.check(lib.magat_head_loss_forward_f32(nat.ptr(x), x.stride(0), nat.ptr(w), nat.ptr(b), nat.ptr(target),
                                                      1 if smoothing > 0.0 else 0, smoothing, nat.ptr(logits), nat.ptr(dlogits),
                                                      None, nat.ptr(loss), nat.ptr(ws), M, width, nat.current_stream(dev)),
                      "magat_head_loss_forward_f32")
        ctx.save_for_backward(x, w, dlogits)
        ctx.has_bias = bias is not None
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, gloss, _glogits):
        lib = nat.lib()
        x, w, dlogits = ctx.saved_tensors
        M, width = x.shape
        dev = x.device
        g = gloss.detach().to(torch.float32).contiguous()
        dx = torch.empty(M, width, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.empty(CLASSES, width, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        db = torch.empty(CLASSES, dtype=torch.float32, device=dev) if ctx.has_bias and ctx.needs_input_grad[2] else None
        ws = _workspace(M, width, dev)
        with torch.cuda.device(dev):
            nat.check(lib.magat_head_loss_backward_f32(nat.ptr(dlogits), nat.ptr(g), nat.ptr(x), x.stride(0), nat.ptr(w), nat.ptr(dx),
                                                       width, nat.ptr(dw), nat.ptr(db), nat.ptr(ws), M, width,
                                                       nat.current_stream(dev)), "magat_head_loss_backward_f32")
        return dx, dw, db, None, None


def head_loss(x, weight, bias, target, label_smoothing=0.0):
    """(loss, logits) of the head `logits = x @ weight.T + bias` (x (M, width), weight (5, width), bias (5,) or None) and the
    training loss on them, fused: one pass over x forward, one backward, on the HIP kernels.

    target: (M,) int64 indices, or one-hot rows (M, 5) / (B, N, 5) reduced with argmax(-1).
    label_smoothing == 0 gives nn.CrossEntropyLoss() semantics - the MEAN over the rows of -log p[target]; label_smoothing > 0
    gives the reference's LabelSmoothing(5, s) semantics - the SUM over the rows of KL(q || p), q = 1 - s on the target and
    s / 4 elsewhere.  The jump between the two at s -> 0 (a factor M, and KL's entropy term) is the reference's own: its agent
    picks one or the other criterion on `config.label_smoothing != 0`.

    Gradients flow to x, weight and bias through the loss.  `logits` is returned DETACHED from the fused graph (for the
    agent's bookkeeping - accuracy, argmax -, not for a second loss): a function of it sends no gradient back."""
    s = _smoothing(label_smoothing)
    target = as_indices(target)
    width = x.shape[-1]
    hip = (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.device == x.device and
           (bias is None or (bias.dtype == torch.float32 and bias.device == x.device)) and
           tuple(weight.shape) == (CLASSES, width) and width % 4 == 0 and width <= MAX_WIDTH and _rows_ok(x, width) and
           target.shape[0] == x.shape[0])
    if not hip:
        nat.require_device_or_composite(x, "head_loss")
        logits = tnf.linear(x, weight, bias)
        return loss_composite(logits, target, s), logits.detach()
    return _HeadLossFunction.apply(x, weight, bias, target.to(x.device).contiguous(), s)


class _ActionLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, smoothing):
        lib = nat.lib()
        M = logits.shape[0]
        dev = logits.device
        need = ctx.needs_input_grad[0]
        dlogits = torch.empty(M, CLASSES, dtype=torch.float32, device=dev) if need else None
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = _workspace(M, 4, dev)
        with torch.cuda.device(dev):
            nat.check(lib.magat_action_loss_f32(nat.ptr(logits), logits.stride(0), nat.ptr(target), 1 if smoothing > 0.0 else 0,
                                                smoothing, nat.ptr(dlogits), None, nat.ptr(loss), nat.ptr(ws), M,
                                                nat.current_stream(dev)), "magat_action_loss_f32")
        if need:
            ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        (dlogits,) = ctx.saved_tensors
        return dlogits * gloss, None, None


class ActionLoss(nn.Module):
    """Drop-in for the agent's `self.loss` (CrossEntropyLoss() or LabelSmoothing(5, s), see head_loss): crit(logits, target) with
    logits (M, 5) and target (M,) indices or one-hot rows.  CUDA float32 logits run on magat_action_loss_f32 (the backward is the
    saved d loss / d logits times the incoming gradient); anything else on the torch composite."""

    def __init__(self, label_smoothing=0.0):
        super().__init__()
        self.label_smoothing = _smoothing(label_smoothing)

    def extra_repr(self):
        return "label_smoothing=%g" % self.label_smoothing

    def forward(self, logits, target):
        target = as_indices(target)
        hip = (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[1] == CLASSES and
               logits.shape[0] > 0 and logits.stride(1) == 1 and logits.stride(0) >= CLASSES and
               target.shape[0] == logits.shape[0])
        if not hip:
            nat.require_device_or_composite(logits, "ActionLoss")
            return loss_composite(logits, target, self.label_smoothing)
        return _ActionLossFunction.apply(logits, target.to(logits.device).contiguous(), self.label_smoothing)
