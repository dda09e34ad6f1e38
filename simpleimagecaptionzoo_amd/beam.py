"""Beam-search options of the three decoders (include/icz.h: icz_beam_opts): n-best lists, length penalty and n-gram blocking.
The search itself runs on the device (csrc/beam_kernels.h); this module parses the options and shapes the results."""
import ctypes as C
import math

import torch

from ._lib import BeamOpts, check, ptr, stream_ptr

LP_KINDS = {"avg": 1, "wu": 2}


def parse_length_penalty(length_penalty):
    """None | ("avg", alpha) | ("wu", alpha) | "avg_<alpha>" | "wu_<alpha>" -> (lp_kind, alpha) of icz_beam_opts.
    avg: score / len^alpha; wu: score / ((5 + len) / 6)^alpha (len = generated tokens, <end> counted).  ValueError otherwise."""
    if length_penalty is None:
        return 0, 0.0
    if isinstance(length_penalty, str):
        kind, sep, a = length_penalty.partition("_")
        try:
            alpha = float(a) if sep else None
        except ValueError:
            alpha = None
        if alpha is None:
            raise ValueError("length_penalty %r: expected 'avg_<alpha>' or 'wu_<alpha>'" % length_penalty)
    elif isinstance(length_penalty, (tuple, list)) and len(length_penalty) == 2:
        kind, alpha = length_penalty
        try:
            alpha = float(alpha)
        except (TypeError, ValueError):
            raise ValueError("length_penalty %r: alpha is not a number" % (length_penalty,)) from None
    else:
        raise ValueError("length_penalty %r: expected None, ('avg' | 'wu', alpha) or 'avg_<alpha>' / 'wu_<alpha>'" % (length_penalty,))
    if kind not in LP_KINDS:
        raise ValueError("length_penalty %r: kind must be 'avg' or 'wu'" % (length_penalty,))
    if not math.isfinite(alpha) or alpha < 0:
        raise ValueError("length_penalty %r: alpha must be finite and >= 0" % (length_penalty,))
    return LP_KINDS[kind], alpha


def make_opts(n_best=1, length_penalty=None, block_ngram=0):
    kind, alpha = parse_length_penalty(length_penalty)
    return BeamOpts(int(n_best), int(block_ngram), kind, alpha)


def search_opts(entry, handle, feats, beam_size, max_steps, opts):
    """Calls icz_*_beam_search_opts `entry` on checked features -> (seqs float32 (n, m, L), lens int32 (n, m), scores (n, m))."""
    n, m, dev = feats.shape[0], max(1, int(opts.n_best)), feats.device
    seqs = torch.zeros(n, m, max_steps + 1, dtype=torch.float32, device=dev)
    lens = torch.zeros(n, m, dtype=torch.int32, device=dev)
    scores = torch.zeros(n, m, dtype=torch.float32, device=dev)
    check(entry(handle, ptr(feats), n, beam_size, max_steps, C.byref(opts), ptr(seqs), ptr(lens), ptr(scores), stream_ptr()))
    return seqs, lens, scores


def nbest_lists(seqs, lens, scores):
    """(seqs (n, m, L), lens (n, m), scores (n, m)) -> per image a list of (ids (1, L_i) float32, raw score), best first."""
    lens, scores = lens.tolist(), scores.tolist()
    return [[(seqs[i, j:j + 1, :lens[i][j]], scores[i][j]) for j in range(len(lens[i])) if lens[i][j] > 0] for i in range(len(lens))]
