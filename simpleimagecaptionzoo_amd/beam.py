"""Beam-search options of the three decoders (include/icz.h: icz_beam_opts, icz_beam_diversity): n-best lists, length penalty,
n-gram blocking and diverse beam search (grouped beams with a diversity penalty).  The search itself runs on the device
(csrc/beam_kernels.h); this module parses the options and shapes the results."""
import ctypes as C
import math
import numbers

import torch

from ._lib import BEAM_STEP_FIELDS, BeamDiversity, BeamOpts, BeamStepState, check, lib, ptr, stream_ptr

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


def make_diversity(groups=1, diversity=0.0, beam=None):
    """-> icz_beam_diversity: `groups` (an int in 1..beam dividing beam) groups of beam / groups beams; `diversity` lambda (a finite
    real >= 0) penalises, at every step, a token once per earlier group that picked it at that step.  ValueError otherwise (bools
    included), before any device work."""
    if isinstance(groups, bool) or not isinstance(groups, numbers.Integral):
        raise ValueError("groups %r: expected an int" % (groups,))
    if isinstance(diversity, bool) or not isinstance(diversity, numbers.Real):
        raise ValueError("diversity %r: expected a real number" % (diversity,))
    groups, diversity = int(groups), float(diversity)
    if groups < 1 or (beam is not None and (groups > int(beam) or int(beam) % groups != 0)):
        raise ValueError("groups %d: must lie in 1..beam (%s) and divide it" % (groups, beam))
    if not math.isfinite(diversity) or diversity < 0:
        raise ValueError("diversity %r: must be finite and >= 0" % (diversity,))
    return BeamDiversity(groups, diversity)


def _outputs(feats, max_steps, opts):
    n, m, dev = feats.shape[0], max(1, int(opts.n_best)), feats.device
    return (torch.zeros(n, m, max_steps + 1, dtype=torch.float32, device=dev), torch.zeros(n, m, dtype=torch.int32, device=dev),
            torch.zeros(n, m, dtype=torch.float32, device=dev))


def search_opts(entry, handle, feats, beam_size, max_steps, opts):
    """Calls icz_*_beam_search_opts `entry` on checked features -> (seqs float32 (n, m, L), lens int32 (n, m), scores (n, m))."""
    seqs, lens, scores = _outputs(feats, max_steps, opts)
    check(entry(handle, ptr(feats), feats.shape[0], beam_size, max_steps, C.byref(opts), ptr(seqs), ptr(lens), ptr(scores), stream_ptr()))
    return seqs, lens, scores


def search_diverse(entry, handle, feats, beam_size, max_steps, opts, div):
    """Calls icz_*_beam_search_diverse `entry`; the outputs of search_opts."""
    seqs, lens, scores = _outputs(feats, max_steps, opts)
    check(entry(handle, ptr(feats), feats.shape[0], beam_size, max_steps, C.byref(opts), C.byref(div), ptr(seqs), ptr(lens), ptr(scores),
                stream_ptr()))
    return seqs, lens, scores


def search(entries, handle, feats, beam_size, max_steps, opts, div):
    """a family's beam_search_opts entry for one group (today's search), its beam_search_diverse entry otherwise"""
    if div.groups == 1:
        return search_opts(entries.beam_search_opts, handle, feats, beam_size, max_steps, opts)
    return search_diverse(entries.beam_search_diverse, handle, feats, beam_size, max_steps, opts, div)


def rowtopk_route_for(V, ldl, base_aligned=True):
    """The kernel a search's row top-k takes (icz_beam_rowtopk_route_for, host only): 1 register <3>, 2 register <10>, 3 sweep."""
    r = lib().icz_beam_rowtopk_route_for(int(V), int(ldl), int(bool(base_aligned)))
    if r < 0:
        check(r)
    return r


def entry_rowtopk(route, logits, n_img, k, V, ldl, step, n_act, run, compact, seqs_in, L, ngram, groups, cand_val, cand_idx):
    """Test entry icz_test_beam_rowtopk: the row top-k kernel of `route` on device tensors (include/icz.h)."""
    check(lib().icz_test_beam_rowtopk(int(route), ptr(logits), int(n_img), int(k), int(V), int(ldl), int(step), ptr(n_act), ptr(run), int(compact),
                                      ptr(seqs_in), int(L), int(ngram), int(groups), ptr(cand_val), ptr(cand_idx), stream_ptr()))


def entry_step(route, state, n_img, k, V, ldl, step, L, compact=0, ngram=0, groups=1, lam=0.0):
    """Test entry icz_test_beam_step: row top-k + merge on `state`, a dict of device tensors keyed as icz_beam_step_state (a missing or
    None entry is a null pointer)."""
    s = BeamStepState(*[None if state.get(n) is None else state[n].data_ptr() for n in BEAM_STEP_FIELDS])
    check(lib().icz_test_beam_step(int(route), C.byref(s), int(n_img), int(k), int(V), int(ldl), int(step), int(L), int(compact), int(ngram),
                                   int(groups), float(lam), stream_ptr()))


def entry_finalize(form, n_img, k, L, steps_done, n_best, lp_kind, lp_alpha, groups, n_act, run, seqs, has_complete, best_score, best_len,
                  best_seq, hyp_cnt, hyp_score, hyp_len, hyp_seq, out, lens, scores):
    """Test entry icz_test_beam_finalize: form 0 best hypothesis, 1 n-best, 2 grouped n-best, on device tensors (None: null)."""
    check(lib().icz_test_beam_finalize(int(form), int(n_img), int(k), int(L), int(steps_done), int(n_best), int(lp_kind), float(lp_alpha),
                                       int(groups), ptr(n_act), ptr(run), ptr(seqs), ptr(has_complete), ptr(best_score), ptr(best_len),
                                       ptr(best_seq), ptr(hyp_cnt), ptr(hyp_score), ptr(hyp_len), ptr(hyp_seq), ptr(out), ptr(lens), ptr(scores),
                                       stream_ptr()))


def nbest_lists(seqs, lens, scores):
    """(seqs (n, m, L), lens (n, m), scores (n, m)) -> per image a list of (ids (1, L_i) float32, raw score), best first."""
    lens, scores = lens.tolist(), scores.tolist()
    return [[(seqs[i, j:j + 1, :lens[i][j]], scores[i][j]) for j in range(len(lens[i])) if lens[i][j] > 0] for i in range(len(lens))]
