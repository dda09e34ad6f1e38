"""CPU-only checks of constrained beam search (include/icz.h: icz_beam_constraints): the argument errors of the four
icz_*_beam_search_constrained entries in their documented order before any device work, the Python ValueErrors, encode_constraints,
the host oracle of tests/_beam_constrained.py against independent statements, and the input conditions the GPU tests rely on (the
share of comparable whole-search pairs; the margin of every deciding comparison of the step cases)."""
import ctypes

import numpy as np
import pytest

import _beam_constrained as bc
import _beam_opts_oracle as bo
import _beam_step as bs
from test_gpu_beam_opts import GOLDENS, LP

ENTRIES = ("butd", "aoa", "nic", "ensemble")
DUMMY = tuple(ctypes.c_void_p(256 * (i + 1)) for i in range(5))


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _opts(n_best=1, block_ngram=0, lp_kind=0, lp_alpha=0.0):
    from simpleimagecaptionzoo_amd._lib import BeamOpts
    return BeamOpts(n_best, block_ngram, lp_kind, lp_alpha)


class _Cons:
    """an icz_beam_constraints over a host array (the device pointer is a dummy: nothing dereferences it before the handle check)"""

    def __init__(self, words, C=None, A=None, dev=True, host=True):
        from simpleimagecaptionzoo_amd._lib import BeamConstraints
        self.words = np.ascontiguousarray(words, dtype=np.int32)
        C = self.words.shape[1] if C is None else C
        A = self.words.shape[2] if A is None else A
        self.struct = BeamConstraints(C, A, 4096 if dev else None, self.words.ctypes.data if host else None)


def _call(entry, opts, cons, ptrs=(None,) * 5, beam=3, n_img=2):
    feats, seqs, lens, scores, sat = ptrs
    if entry == "ensemble" and feats is not None:
        feats = (ctypes.c_void_p * 1)(feats)
    fn = getattr(_lib(), "icz_%s_beam_search_constrained" % entry)
    return fn(None, feats, n_img, beam, 20, None if opts is None else ctypes.byref(opts), None if cons is None else ctypes.byref(cons.struct),
              seqs, lens, scores, sat, None)


def _words(*imgs, C=2, A=2):
    w = np.full((len(imgs), C, A), -1, dtype=np.int32)
    for i, cons in enumerate(imgs):
        for q, alts in enumerate(cons):
            w[i, q, :len(alts)] = alts
    return w


def test_constraints_struct_layout():
    from simpleimagecaptionzoo_amd._lib import BeamConstrainedState, BeamConstraints
    assert ctypes.sizeof(BeamConstraints) == 24
    assert [f[0] for f in BeamConstraints._fields_] == ["max_constraints", "max_alts", "words_dev", "words_host"]
    assert ctypes.sizeof(BeamConstrainedState) == 18 * ctypes.sizeof(ctypes.c_void_p)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_in_order(entry):
    name = b"icz_%s_beam_search_constrained" % entry.encode()
    ok = _Cons(_words([[5], [11, 12]], [[7]]))
    bad = _Cons(_words([[5], [5]], []))                    # a repeated id: reported only behind the options
    cases = [
        # 1. the options, as _opts
        (None, bad, 3, b"null options"),
        (_opts(n_best=4), bad, 3, b"n_best 4 outside 1..beam"),
        (_opts(block_ngram=5), bad, 3, b"block_ngram 5"),
        (_opts(lp_kind=3), None, 3, b"lp_kind 3 unknown"),
        (_opts(lp_kind=1, lp_alpha=float("nan")), None, 3, b"lp_alpha"),
        # 2. the constraints
        (_opts(), None, 3, b"null constraints"),
        (_opts(), _Cons(_words([], []), C=4), 3, b"max_constraints 4 outside 0..3"),
        (_opts(), _Cons(_words([], []), C=-1), 3, b"max_constraints -1"),
        (_opts(), _Cons(_words([], []), A=5), 3, b"max_alts 5 outside 1..4"),
        (_opts(), _Cons(_words([], []), A=0), 3, b"max_alts 0"),
        (_opts(), _Cons(_words([[5]], []), dev=False), 3, b"null constraint words"),
        (_opts(), _Cons(_words([[5]], []), host=False), 3, b"null constraint words"),
        (_opts(), ok, 9, b"beam size 9 out of range 1..8"),
        (_opts(), _Cons(_words([[5]], [], C=3)), 5, b"2^3 states x 5 beams exceed 32"),
        (_opts(), _Cons(_words([[], [5]], [])), 3, b"constraint 1 behind an empty one"),
        (_opts(), _Cons(np.array([[[-1, 5], [-1, -1]], [[-1, -1], [-1, -1]]])), 3, b"word behind an empty slot"),
        (_opts(), _Cons(_words([[5, -2]], [])), 3, b"word id -2"),
        (_opts(), _Cons(_words([[5], [2]], [])), 3, b"word id 2 is <pad>, <sta> or <end>"),
        (_opts(), _Cons(_words([[0]], [])), 3, b"word id 0 is <pad>"),
        (_opts(), _Cons(_words([[5, 6], [7, 5]], [])), 3, b"word id 5 appears twice"),
        (_opts(), _Cons(_words([[5]], [[9], [9]])), 3, b"image 1: word id 9 appears twice"),
        # 3. null arguments
        (_opts(n_best=3, block_ngram=3, lp_kind=2, lp_alpha=0.9), ok, 3, b"null argument"),
    ]
    for opts, cons, beam, msg in cases:
        assert _call(entry, opts, cons, beam=beam) == -1
        err = _lib().icz_last_error()
        assert msg in err and name in err, (entry, msg, err)
    out0 = 0 if entry != "ensemble" else 1                 # the ensemble's features are checked with its members, behind the handle
    for i in range(out0, 5):
        ptrs = tuple(None if j == i else DUMMY[j] for j in range(5))
        assert _call(entry, _opts(), ok, ptrs) == -1
        assert b"null argument" in _lib().icz_last_error()
    # 4. the null handle last -- with constraints, with none (C = 0; every slot empty), at the row limit
    for cons, beam in ((ok, 3), (_Cons(np.zeros((2, 0, 1))), 8), (_Cons(_words([], [])), 8), (_Cons(_words([[5]], [], C=3)), 4), (_Cons(_words([[5]], [], C=2)), 8)):
        assert _call(entry, _opts(), cons, DUMMY, beam) == -1
        assert (name + b": null handle") in _lib().icz_last_error()


def test_make_constraints():
    from simpleimagecaptionzoo_amd.constrained import check_beam, make_constraints, rows_per_image
    w = make_constraints([[[5], [11, 12]], [], None, [7]], 4, 53)
    assert w.dtype == np.int32 and w.shape == (4, 2, 2)
    assert w.tolist() == [[[5, -1], [11, 12]], [[-1, -1], [-1, -1]], [[-1, -1], [-1, -1]], [[7, -1], [-1, -1]]]
    assert make_constraints([[], []], 2, 53).shape == (2, 0, 1)
    assert make_constraints([[[3, 4, 5, 6], [7], [52]]], 1, 53).shape == (1, 3, 4)
    assert rows_per_image(w, 3) == 12 and rows_per_image(make_constraints([[], []], 2, 53), 3) == 3
    assert rows_per_image(np.full((2, 2, 2), -1, dtype=np.int32), 5) == 5
    for cons, n_img, V in (([[[5]]], 2, 53), ([[[5], [6], [7], [8]]], 1, 53), ([[[3, 4, 5, 6, 7]]], 1, 53), ([[[]]], 1, 53),
                           ([[[53]]], 1, 53), ([[[-1]]], 1, 53), ([[[0]]], 1, 53), ([[[1]]], 1, 53), ([[[2]]], 1, 53),
                           ([[[5], [5]]], 1, 53), ([[[5, 5]]], 1, 53), ([[[5.0]]], 1, 53), ([[["5"]]], 1, 53), ([[[True]]], 1, 53)):
        with pytest.raises(ValueError):
            make_constraints(cons, n_img, V)
    assert check_beam(8, 2) == 8 and check_beam(4, 3, 4) == 4 and check_beam(1, 0) == 1
    for beam, C, n_best in ((0, 0, 1), (9, 0, 1), (5, 3, 1), (3, 1, 4), (3, 1, 0), (True, 0, 1), (3.0, 0, 1), (3, 1, True)):
        with pytest.raises(ValueError):
            check_beam(beam, C, n_best)


def test_beam_search_raises_before_the_device():
    """bad options, constraints or beam raise ValueError before the handle's features or library entries are looked at"""
    import types
    from simpleimagecaptionzoo_amd.constrained import beam_search
    h = types.SimpleNamespace(V=53)
    for cons, kw in (([[[5]]], {"n_best": 0}), ([[[5]]], {"block_ngram": 5}), ([[[5]]], {"length_penalty": "bad"}), ([[[2]]], {}),
                     ([[[60]]], {}), ([[[5], [6], [7]]], {"beam_size": 5}), ([[[5]]], {"beam_size": 9}), ([[[5]]], {"beam_size": 3, "n_best": 4})):
        with pytest.raises(ValueError):
            beam_search(h, None, cons, **kw)


def test_encode_constraints():
    from simpleimagecaptionzoo_amd.constrained import encode_constraints, satisfied_flags
    from simpleimagecaptionzoo_amd.vocab import Caption_Vocabulary
    vocab = Caption_Vocabulary()
    for w in ("<pad>", "<sta>", "<end>", "dog", "dogs", "frisbee", "park"):
        vocab.add_word(w)
    ids = {w: vocab.word2ix[w] for w in ("dog", "dogs", "frisbee", "park")}
    got, dropped = encode_constraints([[["dog", "dogs", "puppy"], "frisbee", ["zebra", "zebras"]], [], None, ["<end>", ["park", "dog", "park"]]], vocab)
    assert got == [[[ids["dog"], ids["dogs"]], [ids["frisbee"]]], [], [], [[ids["park"], ids["dog"]]]]
    assert dropped == [(0, 2, ["zebra", "zebras"]), (3, 0, ["<end>"])]
    assert satisfied_flags(5, 3) == [True, False, True] and satisfied_flags(0, 2) == [False, False]


# ---- the oracle against independent statements ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_without_constraints_is_beam_nbest(golden_dir, name):
    model, p, feats = bc.golden_case(golden_dir, name, "track")
    for k in (1, 3, 5):
        for block, lp in ((0, None), (3, ("wu", 0.9))):
            for i in range(feats.shape[0]):
                want = bo.nbest(model, feats[i:i + 1], p, k, 50, block, *LP[lp])
                for C, cons in ((0, []), (2, [])):               # no state but 0 is ever entered
                    got = bc.nbest(model, feats[i:i + 1], p, k, C, cons, 50, block, *LP[lp])
                    assert [h.tokens for h in got] == [w[0] for w in want] and [h.finished for h in got] == [w[2] for w in want]
                    assert all(h.state == 0 for h in got)
                    # the oracle steps its live rows only, and torch's matmul rounds a 1-row and a k-row batch differently: the
                    # project's beam-score tolerance (up to 50 fp32 additions at |score| < 64, half an ulp of 3.8e-6 each)
                    np.testing.assert_allclose([h.score for h in got], [w[1] for w in want], atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("regime", ["nat", "track"])
def test_oracle_states_are_earned_and_comparable_share(golden_dir, name, regime):
    """every hypothesis is listed in exactly the state its tokens earn (so a full-state one holds a word of every constraint), ranks
    by popcount first, and blocked n-grams do not repeat; the pairs whose selections stay GAP_MIN apart are counted for the share"""
    model, p, feats = bc.golden_case(golden_dir, name, regime)
    for cfg in bc.configs():
        beam, si, block, lp = cfg
        cons = bc.batch_constraints(si, feats.shape[0])
        C = max(len(c) for c in cons)
        for i in range(feats.shape[0]):
            hyps, _ = bc.oracle_pair(golden_dir, name, regime, cfg, i)
            assert 1 <= len(hyps) <= beam << C
            pcs = [bc.popcount(h.state) for h in hyps]
            assert pcs == sorted(pcs, reverse=True)
            per_state = {}
            for h in hyps:
                assert h.state == bc.earned_state(h.tokens, cons[i]), (cfg, i, h)
                assert h.state < (1 << len(cons[i]))
                assert h.finished == (h.tokens[-1] == 2) and h.tokens[0] == 1 and 2 not in h.tokens[1:-1]
                assert not (block and bo.repeats_ngram(h.tokens, block))
                per_state[h.state] = per_state.get(h.state, 0) + 1
            assert max(per_state.values()) <= beam
            full = (1 << len(cons[i])) - 1
            for h in hyps:
                if h.state == full:
                    assert all(bc.contains(h.tokens, alts) for alts in cons[i])


def test_comparable_share_of_the_whole_search_pairs(golden_dir):
    """at most 10 % of the (config, image) pairs of tests/test_gpu_beam_constrained.py have a selection closer than GAP_MIN"""
    left = total = 0
    by_beam = {}
    for name in GOLDENS:
        for regime in ("nat", "track"):
            n = bc.golden_case(golden_dir, name, regime)[2].shape[0]
            for cfg in bc.configs():
                for i in range(n):
                    gap = bc.oracle_pair(golden_dir, name, regime, cfg, i)[1]
                    total += 1
                    left += gap < bc.GAP_MIN
                    by_beam[cfg[0]] = by_beam.get(cfg[0], 0) + (gap < bc.GAP_MIN)
    print("left out %d of %d pairs (%.1f %%), by beam %s" % (left, total, 100.0 * left / total, by_beam))
    assert total == 720 and left <= bc.MAX_LEFT_OUT * total


# ---- the step cases: purposes and margins ------------------------------------------------------------------------------------------
def test_step_cases_cover_the_shapes():
    names = [c.name for c in bc.CONS_CASES]
    assert len(set(names)) == len(names)
    shapes = {(c.V, c.beam, c.C) for c in bc.CONS_CASES}
    for V in (53, 3072, 3073, 10102, 10300):
        for beam, C in ((4, 1), (3, 2), (2, 3)):
            assert (V, beam, C) in shapes
    assert any(c.beam << c.C == 32 for c in bc.CONS_CASES)
    assert {r for c in bc.CONS_CASES for r in c.routes} == {0, 1, 2, 3}
    assert any(c.step == 1 and c.compact for c in bc.CONS_CASES) and any(c.step == 1 and not c.compact for c in bc.CONS_CASES)
    for c in bc.CONS_CASES:
        inp = bc.cons_inputs(c)
        assert (inp["n_act"] <= inp["cap"]).all() and (inp["cap"] <= c.beam).all()
        assert all(3 <= w < c.V for img in c.words for alts in img for w in alts)


@pytest.mark.parametrize("case", bc.CONS_CASES, ids=lambda c: c.name)
def test_step_case_margins_and_purposes(case):
    c = case
    inp = bc.cons_inputs(c)
    log = []
    rt = bc.cons_rowtopk_ref(c, inp, log)
    st = bc.cons_step_ref(c, inp, bc.cons_new_state(c, inp), log)
    ratios = [r for _, r in log]
    assert all(r >= bs.MARGIN for r in ratios), (c.name, sorted(log, key=lambda x: x[1])[:3])
    K = c.beam << c.C
    for row, (idx, _, force, _) in rt.items():
        img = row // K
        words = [w for alts in c.words[img] for w in alts]
        assert not set(idx.tolist()) & set(words)                         # the ordinary list holds no constraint word
        assert np.isfinite(force).sum() <= len(words)
    pu = c.purpose
    if pu.get("step1"):
        assert st["n_act"][:, 0].tolist() == [c.beam] * c.n_img           # state 0 fills from the one scored row
        assert all(0 < st["n_act"][img, 1 << q] <= len(alts) for img in range(c.n_img) for q, alts in enumerate(c.words[img]))
    if pu.get("cap0"):
        assert st["n_act"][0, 1] == 0 and st["cap"][0, 1] == 0 and st["n_act"][1, 2] == 0
        assert st["n_act"][0, 3] == 1                                     # the empty full state is entered from state 2
    if pu.get("banned_words"):
        for row, (_, _, force, _) in rt.items():
            for q, alts in enumerate(c.words[0]):
                for a, w in enumerate(alts):
                    assert np.isfinite(force[q * 4 + a]) == (w not in pu["banned_words"])
        assert any(np.isfinite(f[2]).any() for f in rt.values())
    if pu.get("reuse"):
        src = st["src_row"][1 * c.beam:2 * c.beam]                         # state 1's new rows: from state 0 (forced) and from state 1 (re-use)
        toks = st["it_next"][1 * c.beam:2 * c.beam]
        assert any(s // c.beam == 0 and t == 5 for s, t in zip(src, toks)) and any(s // c.beam == 1 and t == 5 for s, t in zip(src, toks))
    if pu.get("ends_states"):
        assert sorted(set(st["hyp_state"][:st["hyp_cnt"][0]].tolist())) == [0, 1]
        assert st["cap"][0].tolist() == [1, 1] and st["hyp_cnt"][1] == 1 + 3
    if pu.get("tie") == "states":
        assert st["src_row"][2:4].tolist() == [0, 2] and st["it_next"][2:4].tolist() == [5, 5] and st["run"][2] == st["run"][3]
    if pu.get("tie") == "forced":
        assert st["src_row"][2] == 0 and st["it_next"][2] == 5 and st["n_act"][0, 1] == 1 and st["run"][2] == -1.0


def test_finalize_cases():
    for name, f in bc.CFIN_CASES.items():
        out, lens, scores, sat = bc.cons_finalize_ref(f)
        S = 1 << f["C"]
        for img in range(f["n_img"]):
            got = [(bc.popcount(s), ln) for s, ln in zip(sat[img], lens[img]) if ln > 0]
            assert [g[0] for g in got] == sorted((g[0] for g in got), reverse=True), name
            assert (sat[img] < S).all()
    _, lens, scores, _ = bc.cons_finalize_ref(bc.CFIN_CASES["c2_lp0"])
    assert lens[2].tolist() == [0, 0, 0] and np.isneginf(scores[2]).all()


def test_aoa_adaptive_pairs_are_comparable_and_the_oracle_is_good_enough(golden_dir):
    """the input conditions of test_gpu_beam_constrained.py::test_aoa_per_image_region_counts, on the oracle alone: at least 90 % of
    its (config, image) pairs keep their selections GAP_MIN apart, and on every hypothesis compared the fp32 oracle's own score is
    within OWN_ERROR_MAX (a fifth of the 1e-4 it is used at) of the float64 oracle's for the same tokens"""
    _, _, p, f, counts = bc.aoa_adaptive_case(golden_dir)
    compared = total = 0
    worst = 0.0
    for cfg in bc.AOA_ADAPTIVE_CONFIGS:
        for i in range(3):
            hyps, gap = bc.aoa_adaptive_pair(golden_dir, cfg, i)
            total += 1
            if gap < bc.GAP_MIN:
                continue
            compared += 1
            for h in hyps[:cfg[0]]:
                worst = max(worst, bc.oracle_own_error("aoa", f[i:i + 1, :counts[i]], p, h.tokens, h.score))
    print("compared %d of %d pairs, the oracle's largest own error %.3g" % (compared, total, worst))
    assert compared >= 0.9 * total and worst <= bc.OWN_ERROR_MAX
