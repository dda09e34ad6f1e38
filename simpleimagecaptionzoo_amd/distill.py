"""Word-level knowledge distillation (beyond the reference; include/icz.h: icz_*_xe_backward_distill, csrc/distill.hip): one
student decoder handle is trained on the word distribution of an ensemble of 1..4 teachers of the same vocabulary,

    q = sum_m w_m softmax(z_m / temperature),    loss = ((1 - alpha) sum hard + alpha sum kd) / N,
    kd = temperature^2 KL(q || softmax(s / temperature)),    hard = the LabelSmoothingLoss term of xe_backward,

in the place of the XE loss of the handle's xe_backward.  The teachers' logits are what their evaluation-mode xe_forward writes
for the same captions (teacher_logits); the combined row q is formed inside the loss kernel and never stored.  The entry points
are functions: the handles and captioners keep their public surface."""
import ctypes as C
import math
import numbers

import torch

from ._lib import DistillOpts, IczError, check, lib, ptr, stream_ptr
from .ensemble import check_members, check_weights
from .handle import grad_args

MIN_TEMPERATURE, MAX_TEMPERATURE = 0.25, 8.0


def _real(x, what, lo, hi, open_hi=False):
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(float(x)) or not (
            lo <= float(x) < hi if open_hi else lo <= float(x) <= hi):
        raise ValueError("%s %r outside [%g, %g%s" % (what, x, lo, hi, ")" if open_hi else "]"))
    return float(x)


def check_opts(m, weights=None, alpha=0.5, temperature=1.0, smoothing=0.1):
    """The host-side rules of a distillation step for m teachers: 1..4 teachers, alpha in [0, 1], temperature in [0.25, 8],
    smoothing in [0, 1), weights None or m finite reals >= 0 with a positive sum -> (weights as floats or None, alpha, temperature,
    smoothing); ValueError otherwise, before anything touches a device."""
    check_members(m)
    alpha = _real(alpha, "alpha", 0.0, 1.0)
    temperature = _real(temperature, "temperature", MIN_TEMPERATURE, MAX_TEMPERATURE)
    smoothing = _real(smoothing, "smoothing", 0.0, 1.0, open_hi=True)
    return check_weights(weights, m), alpha, temperature, smoothing


def _rows(t, what, V=None):
    """a tensor of logit rows: fp32, on the device, [rows, V] with unit column stride -> its row stride (a view of wider rows may pad)"""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise IczError("%s must be an fp32 CUDA tensor [rows, V] with unit column stride" % what)
    if V is not None and t.shape[1] != V:
        raise IczError("%s has %d columns for a vocabulary of %d" % (what, t.shape[1], V))
    return int(t.stride(0))


def _opts(teachers, rows, V, weights, alpha, temperature, smoothing):
    """icz_distill_opts over the teachers' tensors -> (the struct, what must stay alive while the call is queued)"""
    teachers = list(teachers)
    w, alpha, temperature, smoothing = check_opts(len(teachers), weights, alpha, temperature, smoothing)
    M = len(teachers)
    ld = [_rows(t, "teacher logits %d" % i, V) for i, t in enumerate(teachers)]
    for i, t in enumerate(teachers):
        if t.shape[0] != rows:
            raise IczError("teacher logits %d hold %d rows for %d tokens" % (i, t.shape[0], rows))
    arr_t = (C.c_void_p * M)(*[t.data_ptr() for t in teachers])
    arr_ld = (C.c_int32 * M)(*ld)
    arr_w = (C.c_float * M)(*w) if w is not None else None
    o = DistillOpts(M, arr_t, arr_ld, arr_w, alpha, temperature, smoothing)
    return o, (teachers, arr_t, arr_ld, arr_w)


def teacher_logits(handles, feats_list, captions, lengths):
    """Each teacher handle's evaluation-mode xe_forward on its own features and the shared captions / lengths (lengths = caption
    lengths minus one, sorted descending: the student's xe_forward arguments) -> one (sum(lengths), V) tensor per teacher, rows
    in packed order."""
    handles, feats_list = list(handles), list(feats_list)
    check_members(len(handles))
    if len(feats_list) != len(handles):
        raise ValueError("%d feature tensors for %d teachers" % (len(feats_list), len(handles)))
    if len({h.V for h in handles}) != 1:
        raise ValueError("the teachers have different vocabulary sizes %s" % [h.V for h in handles])
    return [h.xe_forward(f, captions, list(lengths), None, train=False, want_logits=True) for h, f in zip(handles, feats_list)]


def xe_backward_distill(handle, grads, teacher_logits, weights=None, alpha=0.5, temperature=1.0, smoothing=0.1, n_tokens_global=0.0, *,
                        want_dfeats=False):
    """xe_backward of `handle` (a ButdHandle, AoaHandle or NicHandle holding a training-mode xe_forward without scheduled sampling)
    with the distillation loss: teacher_logits = 1..4 tensors (sum(lengths), V) of the same captions, e.g. teacher_logits(); fills
    `grads`; returns (loss, hard, kd) as 1-element device tensors -- the mixed loss, sum hard / N and sum kd / N -- and, for a
    NicHandle with want_dfeats, d features (B, E) behind them.  alpha = 0 is xe_backward bit for bit and reads no teacher.
    ValueError for a bad count, alpha, temperature, smoothing or weights before the library is called."""
    rows = getattr(handle, "_xe_tokens", None)
    teachers = list(teacher_logits)
    o, keep = _opts(teachers, teachers[0].shape[0] if rows is None and teachers else rows, handle.V, weights, alpha, temperature, smoothing)
    out3 = torch.zeros(3, dtype=torch.float32, device=handle.device)
    ga, dfe = grad_args(handle, handle._grad_struct(grads), want_dfeats)
    check(handle._e.xe_backward_distill(handle._h, C.byref(o), *ga, ptr(out3), float(n_tokens_global), stream_ptr()))
    handle._distill_live = keep      # the kernel reads the teachers' tensors in stream order
    res = (out3[0:1], out3[1:2], out3[2:3])
    return res + (dfe,) if want_dfeats else res


def xe_backward_dlogits(handle, dpacked, grads, *, want_dfeats=False):
    """The backward pass of the handle's last xe_forward for an upstream gradient w.r.t. its packed logits (sum(lengths), V), for
    every family (include/icz.h: icz_*_xe_backward_dlogits); fills `grads`.  A NicHandle with want_dfeats returns d features (B, E)."""
    dpacked = dpacked.to(device=handle.device, dtype=torch.float32).contiguous()
    ga, dfe = grad_args(handle, handle._grad_struct(grads), want_dfeats)
    check(handle._e.xe_backward_dlogits(handle._h, ptr(dpacked), *ga, stream_ptr()))
    return dfe


def distill_loss(student, teacher_logits, targets, weights=None, alpha=0.5, temperature=1.0, smoothing=0.1, n_tokens=None, ld_out=None):
    """icz_distill_loss, the loss kernel alone: student (rows, V) and 1..4 teacher tensors (rows, V) -- views of wider rows are read
    at their row stride -- with int64 targets (rows,) -> (d loss / d student (rows, ld_out) with zeros in the pad columns [V, ld_out)
    (ld_out defaults to V), [loss, sum hard / N, sum kd / N] as a 3-element device tensor).  N = n_tokens (default: rows)."""
    ld_s = _rows(student, "student logits")
    rows, V = student.shape
    o, keep = _opts(teacher_logits, rows, V, weights, alpha, temperature, smoothing)
    if not torch.is_tensor(targets) or targets.dtype != torch.int64 or not targets.is_cuda or targets.shape != (rows,):
        raise IczError("targets must be an int64 CUDA tensor (%d,)" % rows)
    targets = targets.contiguous()
    ld_out = V if ld_out is None else int(ld_out)
    if ld_out < V:
        raise IczError("ld_out %d below the vocabulary size %d" % (ld_out, V))
    n = float(rows if n_tokens is None else n_tokens)
    out = torch.empty(rows, ld_out, dtype=torch.float32, device=student.device)
    out3 = torch.zeros(3, dtype=torch.float32, device=student.device)
    with torch.cuda.device(student.device):
        check(lib().icz_distill_loss(ptr(student), ld_s, C.byref(o), ptr(targets), rows, V, n, ptr(out), ld_out, ptr(out3), stream_ptr()))
    return out, out3


__all__ = ["xe_backward_distill", "xe_backward_dlogits", "distill_loss", "teacher_logits", "check_opts", "MIN_TEMPERATURE", "MAX_TEMPERATURE"]
