"""Sampling decode (include/icz.h: icz_*_sample_decode): option validation and the call shared by the BUTD, AoA and NIC handles."""
import ctypes as C
import math
import numbers

import torch

from ._lib import SampleOpts, check, lib, ptr, stream_ptr

MAX_SAMPLES = 8


def _real(x):
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


def make_sample_opts(temperature=1.0, top_k=0, top_p=1.0, n=1, vocab_size=None):
    """icz_sample_opts from Python values; ValueError (before any device work) for n outside 1..8, temperature <= 0 or not finite,
    top_k < 0 (or above vocab_size, where given) and top_p outside (0, 1]."""
    if not isinstance(n, numbers.Integral) or isinstance(n, bool) or not 1 <= n <= MAX_SAMPLES:
        raise ValueError("samples per image %r outside 1..%d" % (n, MAX_SAMPLES))
    if not _real(temperature) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError("temperature %r not positive or not finite" % (temperature,))
    if not isinstance(top_k, numbers.Integral) or isinstance(top_k, bool) or top_k < 0:
        raise ValueError("top_k %r negative or not an integer" % (top_k,))
    if vocab_size is not None and top_k > vocab_size:
        raise ValueError("top_k %d above the vocabulary size %d" % (top_k, vocab_size))
    if not _real(top_p) or not 0 < top_p <= 1:
        raise ValueError("top_p %r outside (0, 1]" % (top_p,))
    return SampleOpts(float(temperature), int(top_k), float(top_p))


def rng_args(rng):
    """rng: None (seed 0), an int seed (Philox), or an fp32 CUDA tensor of explicit uniforms [max_len, rows] -> (seed, uniforms)"""
    if rng is None:
        return 0, None
    if torch.is_tensor(rng):
        if rng.dtype != torch.float32 or not rng.is_cuda:
            raise ValueError("explicit uniforms must be an fp32 CUDA tensor [max_len, rows]")
        return 0, rng.contiguous()
    if isinstance(rng, numbers.Integral) and not isinstance(rng, bool):
        return int(rng) & 0xFFFFFFFFFFFFFFFF, None
    raise ValueError("rng must be None, an integer seed or a tensor of uniforms")


def decode(entry, handle, feats, n, max_len, opts, rng, max_rows):
    """Calls icz_*_sample_decode `entry` -> (ids int64 (rows, max_len), logp (rows, max_len), score (rows,)), rows = images x n,
    row img * n + j"""
    seed, uniforms = rng_args(rng)
    n_img, rows = feats.shape[0], feats.shape[0] * n
    if rows > max_rows:
        raise ValueError("%d images x %d samples exceed the handle's row capacity %d" % (n_img, n, max_rows))
    if uniforms is not None and tuple(uniforms.shape) != (max_len, rows):
        raise ValueError("uniforms must be (%d, %d), got %s" % (max_len, rows, tuple(uniforms.shape)))
    ids = torch.zeros(rows, max_len, dtype=torch.int64, device=feats.device)
    logp = torch.zeros(rows, max_len, dtype=torch.float32, device=feats.device)
    score = torch.zeros(rows, dtype=torch.float32, device=feats.device)
    check(entry(handle, ptr(feats), n_img, n, max_len, C.byref(opts), seed, ptr(uniforms), ptr(ids), ptr(logp), ptr(score), stream_ptr()))
    return ids, logp, score


def filter_draw(logits, bias, nsplit, ld, rows, V, uniforms, temperature=1.0, top_k=0, top_p=1.0):
    """icz_sample_filter_draw (the kernel alone, tests) -> (tokens (rows,), logp (rows,), keep (rows, V) uint8)"""
    opts = make_sample_opts(temperature, top_k, top_p, 1, V)
    tok = torch.zeros(rows, dtype=torch.int64, device=logits.device)
    logp = torch.zeros(rows, dtype=torch.float32, device=logits.device)
    keep = torch.zeros(rows, V, dtype=torch.uint8, device=logits.device)
    check(lib().icz_sample_filter_draw(ptr(logits), ptr(bias), nsplit, ld, rows, V, C.byref(opts), ptr(uniforms), ptr(tok), ptr(logp),
                                       ptr(keep), stream_ptr()))
    return tok, logp, keep
