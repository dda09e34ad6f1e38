"""Multi-sample SCST rollouts for every decoder family (include/icz.h: icz_butd_sample_n, icz_aoa_sample_n, icz_nic_sample_n): K
sampled captions per image in training mode, decoder row img * K + k, each later baselined by the mean CIDEr-D of the image's other
K - 1 (CiderDReward.reward_loo).  The entry point is a function: the handles keep their public surface."""
import ctypes as C
import numbers

import torch

from ._lib import IczError, check, ptr, stream_ptr

MIN_SAMPLES, MAX_SAMPLES = 2, 8


def check_samples(n, what="samples_per_image"):
    """samples per image: an integer 2..8 -> int; ValueError otherwise (bools and non-integers included)"""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not MIN_SAMPLES <= int(n) <= MAX_SAMPLES:
        raise ValueError("%s must be an integer in %d..%d, got %r" % (what, MIN_SAMPLES, MAX_SAMPLES, n))
    return int(n)


def sample_n(handle, feats, n, max_len=20, rng=None):
    """n = 2..8 sampled captions per image under `handle` (a ButdHandle, AoaHandle or NicHandle) in training mode -> (seq int64
    (B n, max_len), logprobs (B n, max_len)), row img * n + k.  The per-image work (BUTD: the hoisted attention tensors; AoA: the
    refiner pass and linear_K / linear_V; NIC: nothing, the image embedding is expanded) runs once per image.  Explicit rng arrays
    are laid out for B n rows (AoA: the refiner's masks per image).  The handle's sample_backward then takes a (B n, max_len)
    reward; NicHandle.sample_backward(want_dfeats=True) returns d features per image, (B, E).  For a ButdHandle this is its
    sample_n.  A bad n or B n above the handle's row capacity raises IczError before anything is queued or allocated."""
    from .butd import ButdHandle
    if isinstance(handle, ButdHandle):
        return handle.sample_n(feats, n, max_len, rng)
    feats = handle._feats(feats)
    B = int(feats.shape[0])
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not MIN_SAMPLES <= int(n) <= MAX_SAMPLES:
        raise IczError("sample_n: n=%r samples per image outside %d..%d" % (n, MIN_SAMPLES, MAX_SAMPLES))
    n = int(n)
    if B * n > handle.max_rows:
        raise IczError("sample_n: %d images x %d samples exceed the handle's row capacity %d" % (B, n, handle.max_rows))
    entry = getattr(handle._e, "sample_n", None)
    if entry is None:
        raise IczError("sample_n: the %s library has no multi-sample rollout" % handle.family)
    rng = rng or handle._make_rng(0)
    seq = handle._buf("sample_n_seq", (B * n, max_len), torch.int64)
    lp = handle._buf("sample_n_lp", (B * n, max_len), torch.float32)
    check(entry(handle._h, ptr(feats), B, n, max_len, C.byref(rng), ptr(seq), ptr(lp), stream_ptr()))
    handle._live = (feats, rng, seq, lp)
    return seq, lp


__all__ = ["sample_n", "check_samples", "MIN_SAMPLES", "MAX_SAMPLES"]
