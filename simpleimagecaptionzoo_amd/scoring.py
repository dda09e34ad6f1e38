"""Scoring given captions (include/icz.h: icz_*_score_captions): the log-probability a decoder handle, or an ensemble of them,
assigns to captions it is handed -- teacher forcing in evaluation mode on the device (csrc/score_captions.hip).  The entry points
are functions: the handles and captioners keep their public surface.

Captions travel as `ids` [rows, T] int64 in the format sample_decode / greedy write: no leading <sta>, <end> (2) included, 0 behind
it; row img * n + j is caption j of image img.  The scored length of a row is the index of its first 2 plus one if a 2 occurs
before any 0, else the index of its first 0, else T."""
import ctypes as C
import numbers

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr

MAX_CAPTIONS = 8          # captions per image in one call
MAX_LEN = 256             # columns of ids
MAX_WORDS = MAX_LEN - 1   # words of an encoded caption: <end> takes a column


def check_n(n):
    """captions per image: an integer 1..8 -> int; ValueError otherwise"""
    if not isinstance(n, numbers.Integral) or isinstance(n, bool) or not 1 <= n <= MAX_CAPTIONS:
        raise ValueError("captions per image %r outside 1..%d" % (n, MAX_CAPTIONS))
    return int(n)


def check_ids(ids, n=1):
    """ids -> an int64 tensor [rows, T] with rows a multiple of n and 1 <= T <= 256; ValueError otherwise.  A numpy array is taken
    as it is, a tensor stays on its device."""
    if isinstance(ids, np.ndarray):
        if ids.dtype != np.int64:
            raise ValueError("ids must be int64, got %s" % ids.dtype)
        ids = torch.from_numpy(np.ascontiguousarray(ids))
    if not torch.is_tensor(ids) or ids.dtype != torch.int64:
        raise ValueError("ids must be an int64 tensor [rows, T], got %s" % (ids.dtype if torch.is_tensor(ids) else type(ids).__name__))
    if ids.dim() != 2 or ids.shape[0] < 1 or not 1 <= ids.shape[1] <= MAX_LEN:
        raise ValueError("ids must be [rows >= 1, 1 <= T <= %d], got %s" % (MAX_LEN, tuple(ids.shape)))
    if ids.shape[0] % n:
        raise ValueError("%d rows of ids are not a multiple of %d captions per image" % (ids.shape[0], n))
    return ids


def scored_lengths(ids):
    """the scored length of every row of ids (numpy [rows, T]) by the rule at the top -> int64 [rows]"""
    ids = np.asarray(ids)
    stop = (ids == 0) | (ids == 2)
    first = np.where(stop.any(1), stop.argmax(1), ids.shape[1])
    at = np.minimum(first, ids.shape[1] - 1)
    return first + ((first < ids.shape[1]) & (ids[np.arange(ids.shape[0]), at] == 2))


def score_captions(handle, feats, ids, n=1):
    """Scores `ids` [rows, T] under `handle` -- a ButdHandle / AoaHandle / NicHandle with its features [rows / n, ...], or an
    EnsembleHandle with `feats` a list of one per member -- as n captions per image.  Returns (logp [rows, T] float32: the
    log-probability of every scored token, 0 behind the row's length; score [rows] float32: their sum in step order).
    ValueError, before the library is called, for n outside 1..8, ids of another dtype or shape, an id outside [0, V), an image
    count that is not rows / n, or more rows than the handle's capacity."""
    n = check_n(n)
    return _score(handle, feats, check_ids(ids, n), n)


def _score(handle, feats, ids, n):
    """score_captions behind check_n / check_ids: what needs the handle"""
    from .ensemble import EnsembleHandle
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= handle.V:
        raise ValueError("ids hold %d: outside the vocabulary [0, %d)" % (lo if lo < 0 else hi, handle.V))
    rows, T = ids.shape
    if rows > handle.max_rows:
        raise ValueError("%d images x %d captions exceed the handle's row capacity %d" % (rows // n, n, handle.max_rows))
    if isinstance(handle, EnsembleHandle):
        arr, n_img = handle._feats(feats)
        entry, h, f = lib().icz_ensemble_score_captions, handle._h, arr
    else:
        feats = handle._feats(feats)
        n_img = int(feats.shape[0])
        entry, h, f = handle._e.score_captions, handle._h, ptr(feats)
    if n_img * n != rows:
        raise ValueError("%d images x %d captions per image, but ids hold %d rows" % (n_img, n, rows))
    ids = ids.to(handle.device).contiguous()
    logp = torch.zeros(rows, T, dtype=torch.float32, device=handle.device)
    score = torch.zeros(rows, dtype=torch.float32, device=handle.device)
    check(entry(h, f, n_img, n, T, ptr(ids), ptr(logp), ptr(score), stream_ptr()))
    return logp, score


def captioner_score(captioner, visual_inputs, ids, n=1):
    """score_captions for a captioner (BUTD / AoA / NIC) on its `visual_inputs`, or for a CaptionEnsemble on one `visual_inputs`
    per member: the features and the (re)bound handle are the ones the captioner's own sample_decode uses."""
    from .ensemble import CaptionEnsemble, member_features
    n = check_n(n)
    ids = check_ids(ids, n)
    if isinstance(captioner, CaptionEnsemble):
        feats = captioner._feats(visual_inputs)
    else:
        feats = member_features(captioner, visual_inputs)
    return _score(captioner._handle(), feats, ids, n)


def encode_captions(captions, vocab, max_len=None):
    """Caption strings -> ids [len(captions), T] int64 (numpy): the words through the vocabulary's <unk> fallback, <end> appended,
    zero padded.  T = max_len, or the longest caption's words + 1.  ValueError for a caption above 255 words or above max_len - 1."""
    rows = []
    for cap in captions:
        words = cap.split()
        if len(words) > MAX_WORDS:
            raise ValueError("caption with %d words: at most %d can be scored" % (len(words), MAX_WORDS))
        rows.append([int(vocab(w)) for w in words] + [2])
    T = max([len(r) for r in rows] + [1]) if max_len is None else int(max_len)
    if not 1 <= T <= MAX_LEN:
        raise ValueError("max_len %r outside 1..%d" % (max_len, MAX_LEN))
    out = np.zeros((len(rows), T), np.int64)
    for i, r in enumerate(rows):
        if len(r) > T:
            raise ValueError("caption with %d words does not fit max_len %d (<end> takes a column)" % (len(r) - 1, T))
        out[i, :len(r)] = r
    return out


def ids_from_beam(seqs, lens):
    """The float32 beam rows of beam_search / beam_search_opts (seqs [..., L] with the leading <sta>, lens [...]) -> ids
    [rows, L - 1] int64 (numpy): row[:len - 1] = seq[1:len], 0 behind."""
    seqs = seqs.cpu().numpy() if torch.is_tensor(seqs) else np.asarray(seqs)
    lens = lens.cpu().numpy() if torch.is_tensor(lens) else np.asarray(lens)
    if seqs.ndim < 2 or seqs.shape[:-1] != lens.shape or seqs.shape[-1] < 2:
        raise ValueError("seqs %s and lens %s are not beam rows [..., L >= 2] and their lengths" % (seqs.shape, lens.shape))
    seqs, lens = seqs.reshape(-1, seqs.shape[-1]), lens.reshape(-1).astype(np.int64)
    if (lens < 0).any() or (lens > seqs.shape[1]).any():
        raise ValueError("a beam length lies outside 0..%d" % seqs.shape[1])
    keep = np.arange(1, seqs.shape[1])[None, :] < lens[:, None]
    return np.where(keep, seqs[:, 1:].astype(np.int64), 0)


def score_tokens(logits, bias, nsplit, ld, rows, V, targets):
    """icz_score_tokens (the kernel alone, tests) -> logp (rows,) = log_softmax(row)[target]"""
    logp = torch.zeros(rows, dtype=torch.float32, device=logits.device)
    check(lib().icz_score_tokens(ptr(logits), ptr(bias), nsplit, ld, rows, V, ptr(targets), ptr(logp), stream_ptr()))
    return logp


def ensemble_score_tokens(members, weights, rows, V, targets):
    """icz_ensemble_score_tokens (the kernel alone, tests): members = [(logits tensor, bias or None, nsplit, ld)], weights = None or
    one per member -> logp (rows,) = log(sum_m w_m softmax(logits_m)[target])"""
    from .ensemble import check_members, check_weights
    members = list(members)
    check_members(len(members))
    w = check_weights(weights, len(members))
    M, dev = len(members), members[0][0].device
    lg = (C.c_void_p * M)(*[t.data_ptr() for t, _, _, _ in members])
    bs = (C.c_void_p * M)(*[b.data_ptr() if b is not None else None for _, b, _, _ in members])
    ns = (C.c_int32 * M)(*[int(k) for _, _, k, _ in members])
    ld = (C.c_int32 * M)(*[int(l) for _, _, _, l in members])
    arr_w = (C.c_float * M)(*w) if w is not None else None
    logp = torch.zeros(rows, dtype=torch.float32, device=dev)
    check(lib().icz_ensemble_score_tokens(M, lg, bs, ns, ld, arr_w, rows, V, ptr(targets), ptr(logp), stream_ptr()))
    return logp


__all__ = ["score_captions", "captioner_score", "encode_captions", "ids_from_beam", "score_tokens", "ensemble_score_tokens", "scored_lengths",
           "check_n", "check_ids"]
