"""Constrained beam search (include/icz.h: icz_beam_constraints; Anderson et al., "Guided Open Vocabulary Image Captioning with
Constrained Beam Search", EMNLP 2017): captions that must contain given words.  Per image up to 3 constraints, each a set of up to 4
alternative word ids (singular / plural, synonyms) satisfied by any one of them; the search keeps `beam_size` beams for every
subset of satisfied constraints and ranks hypotheses that satisfy more of them first.  The search runs on the device
(csrc/beam_kernels.h); this module checks and packs the constraints and shapes the results.  The entry points are functions: the
handles and captioners keep their public surface."""
import ctypes as C
import numbers

import numpy as np
import torch

from . import beam as _beam
from ._lib import BEAM_CONSTRAINED_FIELDS, BeamConstrainedState, BeamConstraints, check, lib, ptr, stream_ptr

MAX_CONSTRAINTS = 3       # per image
MAX_ALTS = 4              # alternative words of one constraint
MAX_BEAM = 8
MAX_STATE_ROWS = 32       # 2^C * beam decoder rows per image
SLOTS = MAX_CONSTRAINTS * MAX_ALTS


def make_constraints(constraints, n_img, V):
    """constraints: per image a list of constraints, each a list of 1..4 alternative word ids (an int is a one-word constraint;
    None or [] = the image is unconstrained) -> int32 numpy array [n_img, C, A] padded with -1 from the right, C = the most
    constraints of any image, A = the most alternatives of any constraint (A >= 1; C may be 0).  ValueError for: another image
    count, more than 3 constraints or 4 alternatives, an empty constraint, an id that is no integer, outside [0, V), or <pad> /
    <sta> / <end> (0, 1, 2), an id that appears twice among the words of one image."""
    constraints = list(constraints)
    if len(constraints) != n_img:
        raise ValueError("%d constraint lists for %d images" % (len(constraints), n_img))
    per_img = []
    for img, cs in enumerate(constraints):
        cs = [] if cs is None else list(cs)
        if len(cs) > MAX_CONSTRAINTS:
            raise ValueError("image %d: %d constraints, at most %d" % (img, len(cs), MAX_CONSTRAINTS))
        seen, out = set(), []
        for c in cs:
            alts = [c] if isinstance(c, numbers.Integral) else list(c)
            if not 1 <= len(alts) <= MAX_ALTS:
                raise ValueError("image %d: a constraint has %d alternatives, expected 1..%d" % (img, len(alts), MAX_ALTS))
            for w in alts:
                if isinstance(w, bool) or not isinstance(w, numbers.Integral):
                    raise ValueError("image %d: word id %r is not an integer" % (img, w))
                if not 0 <= w < V:
                    raise ValueError("image %d: word id %d outside the vocabulary [0, %d)" % (img, w, V))
                if w <= 2:
                    raise ValueError("image %d: word id %d is <pad>, <sta> or <end>" % (img, w))
                if int(w) in seen:
                    raise ValueError("image %d: word id %d appears twice" % (img, w))
                seen.add(int(w))
            out.append([int(w) for w in alts])
        per_img.append(out)
    Cm = max([len(cs) for cs in per_img] + [0])
    Am = max([len(a) for cs in per_img for a in cs] + [1])
    words = np.full((n_img, Cm, Am), -1, dtype=np.int32)
    for img, cs in enumerate(per_img):
        for q, alts in enumerate(cs):
            words[img, q, :len(alts)] = alts
    return words


def check_beam(beam_size, n_constraints, n_best=1):
    """beam_size in 1..8 with 2^C * beam_size <= 32 and n_best in 1..beam_size -> int; ValueError otherwise"""
    if isinstance(beam_size, bool) or not isinstance(beam_size, numbers.Integral) or not 1 <= beam_size <= MAX_BEAM:
        raise ValueError("beam_size %r outside 1..%d" % (beam_size, MAX_BEAM))
    if (int(beam_size) << n_constraints) > MAX_STATE_ROWS:
        raise ValueError("2^%d states x beam_size %d exceed %d rows per image" % (n_constraints, beam_size, MAX_STATE_ROWS))
    if isinstance(n_best, bool) or not isinstance(n_best, numbers.Integral) or not 1 <= n_best <= beam_size:
        raise ValueError("n_best %r outside 1..beam_size (%d)" % (n_best, beam_size))
    return int(beam_size)


def rows_per_image(words, beam_size):
    """decoder rows one image of a search takes: 2^C * beam_size (beam_size when no image has a constraint)"""
    return (int(beam_size) << words.shape[1]) if (words >= 0).any() else int(beam_size)


def _call(handle, feats, words, beam_size, max_steps, opts):
    from .ensemble import EnsembleHandle
    if isinstance(handle, EnsembleHandle):
        f, n = handle._feats(feats)
        entry, dev = lib().icz_ensemble_beam_search_constrained, handle.device
    else:
        feats = handle._feats(feats)
        f, n, dev = ptr(feats), int(feats.shape[0]), feats.device
        entry = handle._e.beam_search_constrained
    if n != words.shape[0]:
        raise ValueError("%d images of features, constraints for %d" % (n, words.shape[0]))
    if n * rows_per_image(words, beam_size) > handle.max_rows:
        raise ValueError("%d images x %d rows exceed the handle's row capacity %d" % (n, rows_per_image(words, beam_size), handle.max_rows))
    words = np.ascontiguousarray(words, dtype=np.int32)
    words_dev = torch.from_numpy(words).to(dev) if words.size else None
    cons = BeamConstraints(words.shape[1], words.shape[2], None if words_dev is None else words_dev.data_ptr(),
                           words.ctypes.data if words.size else None)
    m = int(opts.n_best)
    seqs = torch.zeros(n, m, max_steps + 1, dtype=torch.float32, device=dev)
    lens = torch.zeros(n, m, dtype=torch.int32, device=dev)
    scores = torch.zeros(n, m, dtype=torch.float32, device=dev)
    sat = torch.zeros(n, m, dtype=torch.int32, device=dev)
    check(entry(handle._h, f, n, int(beam_size), int(max_steps), C.byref(opts), C.byref(cons), ptr(seqs), ptr(lens), ptr(scores), ptr(sat),
                stream_ptr()))
    return seqs, lens, scores, sat


def beam_search(handle, feats, constraints, beam_size=3, max_steps=50, n_best=1, length_penalty=None, block_ngram=0):
    """Constrained beam search under `handle` -- a ButdHandle / AoaHandle / NicHandle with its features, or an EnsembleHandle with
    `feats` a list of one per member.  constraints: per image a list of constraints (make_constraints), or the packed int32 array
    [n_img, C, A] it returns.  The options are beam_search_opts's.  Returns (seqs float32 (n_img, n_best, max_steps + 1)
    zero-padded, lens int32 (n_img, n_best), raw log-prob scores (n_img, n_best), sat int32 (n_img, n_best): bit c set = the
    hypothesis contains a word of constraint c), ranked by the number of satisfied constraints, then as beam_search_opts ranks.
    With no constraint at all the first three are beam_search_opts's bit for bit.  ValueError, before the library is called, for
    bad options or constraints, an image count that differs from the features', or more rows (n_img x 2^C x beam_size) than the
    handle's capacity."""
    opts = _beam.make_opts(n_best, length_penalty, block_ngram)
    if opts.block_ngram not in (0, 2, 3, 4):
        raise ValueError("block_ngram %r not 0, 2, 3 or 4" % (block_ngram,))
    shape = None
    if isinstance(constraints, np.ndarray):       # a packed array: unpacked and checked like any other input, its C and A kept
        if constraints.ndim != 3 or constraints.shape[1] > MAX_CONSTRAINTS or not 1 <= constraints.shape[2] <= MAX_ALTS:
            raise ValueError("packed constraints must be [n_img, C <= %d, 1 <= A <= %d], got shape %s"
                             % (MAX_CONSTRAINTS, MAX_ALTS, constraints.shape))
        shape = constraints.shape
        constraints = [[[int(w) for w in alts if w >= 0] for alts in img if (alts >= 0).any()] for img in constraints]
    constraints = list(constraints)
    words = make_constraints(constraints, len(constraints), handle.V)
    if shape is not None:
        wide = np.full(shape, -1, dtype=np.int32)
        wide[:, :words.shape[1], :words.shape[2]] = words
        words = wide
    check_beam(beam_size, words.shape[1], n_best)
    return _call(handle, feats, words, beam_size, max_steps, opts)


def captioner_beam_search(captioner, visual_inputs, constraints, beam_size=3, n_best=1, length_penalty=None, block_ngram=0, max_steps=50):
    """beam_search for a captioner (BUTDDetection / AoADetection / NICDecoder) on its `visual_inputs`, or a CaptionEnsemble on one
    `visual_inputs` per member -> per image a list of (ids float32 (1, L_i) with <sta> and, if finished, <end>; raw summed log-prob;
    sat), best first."""
    from .ensemble import CaptionEnsemble
    constraints = list(constraints)
    _beam.make_opts(n_best, length_penalty, block_ngram)               # ValueError before the features are looked at
    feats = captioner._feats(visual_inputs) if isinstance(captioner, CaptionEnsemble) else captioner._features(visual_inputs)
    seqs, lens, scores, sat = beam_search(captioner._handle(), feats, constraints, beam_size, max_steps, n_best, length_penalty, block_ngram)
    lens, scores, sat = lens.tolist(), scores.tolist(), sat.tolist()
    return [[(seqs[i, j:j + 1, :lens[i][j]], scores[i][j], sat[i][j]) for j in range(len(lens[i])) if lens[i][j] > 0] for i in range(len(lens))]


def encode_constraints(words_per_image, vocab):
    """words_per_image: per image a list of constraints, each a word or a list of alternative words; vocab: a Caption_Vocabulary (or
    anything with word2ix) -> (constraints as make_constraints takes them, dropped): out-of-vocabulary alternatives and the
    special words are dropped, as are alternatives already used by the image; a constraint left without a word is dropped and
    reported in `dropped` as (image index, constraint index, its words).  More than 3 constraints / 4 alternatives are left for
    make_constraints to refuse."""
    w2i = vocab.word2ix
    out, dropped = [], []
    for img, cs in enumerate(words_per_image):
        ids, seen = [], set()
        for q, c in enumerate(cs or []):
            alts = [c] if isinstance(c, str) else list(c)
            keep = []
            for w in alts:
                i = w2i.get(w)
                if i is None or int(i) <= 2 or int(i) in seen:
                    continue
                seen.add(int(i))
                keep.append(int(i))
            if keep:
                ids.append(keep)
            else:
                dropped.append((img, q, alts))
        out.append(ids)
    return out, dropped


def satisfied_flags(sat, n_constraints):
    """the state `sat` of a hypothesis -> one boolean per constraint of its image"""
    return [bool((int(sat) >> c) & 1) for c in range(n_constraints)]


# ---- test entries (include/icz.h): the constrained step's kernels on device tensors ---------------------------------------------
def entry_rowtopk(route, logits, n_img, beam, Cn, A, words, V, ldl, step, n_act, cap, run, compact, seqs_in, L, ngram, cand_val, cand_idx,
                  force_val):
    check(lib().icz_test_beam_rowtopk_constrained(int(route), ptr(logits), int(n_img), int(beam), int(Cn), int(A), ptr(words), int(V), int(ldl),
                                                  int(step), ptr(n_act), ptr(cap), ptr(run), int(compact), ptr(seqs_in), int(L), int(ngram),
                                                  ptr(cand_val), ptr(cand_idx), ptr(force_val), stream_ptr()))


def entry_step(route, state, n_img, beam, Cn, A, V, ldl, step, L, compact=0, ngram=0):
    """icz_test_beam_constrained_step on `state`, a dict of device tensors keyed as icz_beam_constrained_state (missing / None: null)"""
    s = BeamConstrainedState(*[None if state.get(n) is None else state[n].data_ptr() for n in BEAM_CONSTRAINED_FIELDS])
    check(lib().icz_test_beam_constrained_step(int(route), C.byref(s), int(n_img), int(beam), int(Cn), int(A), int(V), int(ldl), int(step), int(L),
                                               int(compact), int(ngram), stream_ptr()))


def entry_finalize(n_img, beam, Cn, L, steps_done, n_best, lp_kind, lp_alpha, n_act, run, seqs, hyp_cnt, hyp_score, hyp_len, hyp_state, hyp_seq,
                   out, lens, scores, sat):
    check(lib().icz_test_beam_finalize_states(int(n_img), int(beam), int(Cn), int(L), int(steps_done), int(n_best), int(lp_kind), float(lp_alpha),
                                              ptr(n_act), ptr(run), ptr(seqs), ptr(hyp_cnt), ptr(hyp_score), ptr(hyp_len), ptr(hyp_state),
                                              ptr(hyp_seq), ptr(out), ptr(lens), ptr(scores), ptr(sat), stream_ptr()))


__all__ = ["make_constraints", "beam_search", "captioner_beam_search", "encode_constraints", "satisfied_flags", "check_beam", "rows_per_image"]
