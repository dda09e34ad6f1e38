"""CPU-only checks of model ensembles (include/icz.h: icz_ensemble_*): the argument errors of create, greedy, beam search and the
combine kernel's entry reported through icz_last_error before any device work, and the Python-level ValueErrors of
eval_ensemble_captions_json_generation, EnsembleHandle and CaptionEnsemble."""
import ctypes as C

import pytest


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _err():
    return _lib().icz_last_error()


FAKE = [C.c_void_p(256 * (i + 1)).value for i in range(5)]      # never dereferenced: every check below runs before the members are


def _create(kinds, members, weights, M):
    out = C.c_void_p()
    k = (C.c_int32 * max(1, len(kinds)))(*kinds) if kinds is not None else None
    m = (C.c_void_p * max(1, len(members)))(*members) if members is not None else None
    w = (C.c_float * len(weights))(*weights) if weights is not None else None
    st = _lib().icz_ensemble_create(k, m, w, M, C.byref(out))
    assert not out.value
    return st


@pytest.mark.parametrize("kinds, members, weights, M, msg", [
    ([0], FAKE[:1], None, 0, b"0 members outside 1..4"),
    ([0] * 5, FAKE, None, 5, b"5 members outside 1..4"),
    (None, FAKE[:2], None, 2, b"null argument"),
    ([0, 0], None, None, 2, b"null argument"),
    ([0, 3], FAKE[:2], None, 2, b"member 1 has unknown kind 3"),
    ([0, -1], FAKE[:2], None, 2, b"unknown kind -1"),
    ([0, 1], [FAKE[0], None], None, 2, b"member 1 is null"),
    ([0, 1, 2], [FAKE[0], FAKE[1], FAKE[0]], None, 3, b"members 0 and 2 are one handle"),
    ([0, 1], FAKE[:2], [1.0, -0.5], 2, b"weight 1 (-0.5) negative"),
    ([0, 1], FAKE[:2], [float("nan"), 1.0], 2, b"weight 0 (nan)"),
    ([0, 1], FAKE[:2], [float("inf"), 1.0], 2, b"not finite"),
    ([0, 1], FAKE[:2], [0.0, 0.0], 2, b"the weights sum to 0"),
])
def test_create_errors(kinds, members, weights, M, msg):
    assert _create(kinds, members, weights, M) == -1
    assert msg in _err(), _err()


def test_create_null_out():
    k, m = (C.c_int32 * 1)(0), (C.c_void_p * 1)(FAKE[0])
    assert _lib().icz_ensemble_create(k, m, None, 1, None) == -1
    assert b"null argument" in _err()


def _opts(n_best=1, block_ngram=0, lp_kind=0, lp_alpha=0.0):
    from simpleimagecaptionzoo_amd._lib import BeamOpts
    return BeamOpts(n_best, block_ngram, lp_kind, lp_alpha)


def _div(groups=1, diversity=0.0):
    from simpleimagecaptionzoo_amd._lib import BeamDiversity
    return BeamDiversity(groups, diversity)


def test_beam_errors_in_order():
    feats = (C.c_void_p * 2)(FAKE[0], FAKE[1])
    out = C.c_void_p(FAKE[2])
    cases = [
        (None, _div(), (out, out, out), b"null options"),
        (_opts(n_best=7), _div(), (out, out, out), b"n_best 7 outside 1..beam"),
        (_opts(block_ngram=5), _div(), (out, out, out), b"block_ngram 5"),
        (_opts(lp_kind=3), _div(), (out, out, out), b"lp_kind 3 unknown"),
        (_opts(lp_kind=1, lp_alpha=-1.0), _div(), (out, out, out), b"lp_alpha"),
        (_opts(), None, (out, out, out), b"null diversity"),
        (_opts(), _div(groups=4), (out, out, out), b"groups 4 outside 1..beam"),
        (_opts(), _div(groups=2, diversity=float("nan")), (out, out, out), b"diversity nan"),
        (_opts(), _div(), (out, None, out), b"null argument"),
        (_opts(), _div(), (out, out, out), b"null handle"),
    ]
    for opts, div, (s, l, sc), msg in cases:
        st = _lib().icz_ensemble_beam_search_diverse(None, feats, 2, 6, 20, None if opts is None else C.byref(opts),
                                                     None if div is None else C.byref(div), s, l, sc, None)
        assert st == -1 and msg in _err(), (msg, _err())
        assert b"icz_ensemble_beam_search_diverse" in _err()


def test_greedy_null_handle():
    feats = (C.c_void_p * 1)(FAKE[0])
    assert _lib().icz_ensemble_greedy(None, feats, 2, 20, C.c_void_p(FAKE[1]), None) == -1
    assert b"icz_ensemble_greedy: null handle" in _err()


def _logprob(M=1, logits=True, bias=None, nsplit=(1,), ld=(8,), weights=None, rows=2, V=5, lp=True, ldo=8, argmax=False):
    n = max(1, len(nsplit))
    lg = (C.c_void_p * n)(*([FAKE[0]] * n)) if logits else None
    bs = (C.c_void_p * n)(*bias) if bias is not None else None
    ns = (C.c_int32 * n)(*nsplit)
    ldv = (C.c_int32 * n)(*ld)
    w = (C.c_float * len(weights))(*weights) if weights is not None else None
    return _lib().icz_ensemble_logprob(M, lg, bs, ns, ldv, w, rows, V, C.c_void_p(FAKE[1]) if lp else None, ldo,
                                       C.c_void_p(FAKE[2]) if argmax else None, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(M=0), b"0 members outside 1..4"),
    (dict(M=5), b"5 members outside 1..4"),
    (dict(logits=False), b"bad arguments"),
    (dict(rows=0), b"bad arguments"),
    (dict(lp=False), b"no output"),
    (dict(ldo=4), b"no output"),
    (dict(weights=[-1.0]), b"weight 0 (-1) negative"),
    (dict(ld=(4,)), b"member 0: null logits, ld < V"),
    (dict(nsplit=(0,)), b"nsplit < 1"),
    (dict(nsplit=(2,)), b"split-K slabs need a bias"),
    (dict(M=2, nsplit=(1, 3), ld=(8, 8), bias=[FAKE[3], None]), b"member 1: split-K slabs need a bias"),
])
def test_logprob_errors(kw, msg):
    assert _logprob(**kw) == -1
    assert msg in _err(), _err()


# ---- Python level ----------------------------------------------------------------------------------------------------------
def test_check_weights():
    from simpleimagecaptionzoo_amd.ensemble import check_weights
    assert check_weights(None, 3) is None
    assert check_weights([1, 3], 2) == [1.0, 3.0]
    assert check_weights((0.0, 2.5), 2) == [0.0, 2.5]
    for bad in ([1.0], [1.0, -1.0], [float("nan"), 1.0], [float("inf"), 1.0], [0, 0], [True, 1.0], ["1", 1.0]):
        with pytest.raises(ValueError):
            check_weights(bad, 2)


def test_handle_and_captioner_refusals():
    from simpleimagecaptionzoo_amd.ensemble import CaptionEnsemble, EnsembleHandle
    with pytest.raises(ValueError, match="1..4 members"):
        EnsembleHandle([])
    with pytest.raises(ValueError, match="expected a ButdHandle"):
        EnsembleHandle([object()])
    with pytest.raises(ValueError, match="1..4 members"):
        CaptionEnsemble([object()] * 5)
    with pytest.raises(ValueError, match="captioner"):
        CaptionEnsemble([object()])


class _FakeEng:
    """enough of an Engine for the argument checks, which run before anything else is touched"""

    def __init__(self, V=10, device="cuda:0"):
        self.caption_vocab = [None] * V
        self.device = device

    def __getattr__(self, name):
        raise AssertionError("the argument checks touched Engine.%s" % name)


@pytest.mark.parametrize("engines, kw, match", [
    (0, {}, "1..4 members"),
    (5, {}, "1..4 members"),
    ([_FakeEng(10), _FakeEng(11)], {}, "vocabularies differ"),
    ([_FakeEng(device="cuda:0"), _FakeEng(device="cuda:1")], {}, "different devices"),
    (2, dict(weights=[1.0]), "2 members"),
    (2, dict(weights=[1.0, -2.0]), "finite real >= 0"),
    (2, dict(weights=[0.0, 0.0]), "sum to 0"),
    (2, dict(length_penalty="wu_0.6"), "need beam search"),
    (2, dict(block_ngram=3), "need beam search"),
    (2, dict(beam_groups=2), "need beam search"),
    (2, dict(eval_beam_size=3, length_penalty="xx_1"), "length_penalty"),
    (2, dict(eval_beam_size=3, block_ngram=5), "block_ngram 5"),
    (2, dict(eval_beam_size=4, beam_groups=3), "groups 3"),
    (2, dict(eval_beam_size=4, beam_groups=2, diversity=-1.0), "diversity"),
    (2, dict(eval_beam_size=0), "eval_beam_size"),
    (2, dict(eval_beam_size=True), "eval_beam_size"),
])
def test_eval_refusals(engines, kw, match):
    from simpleimagecaptionzoo_amd.engine import eval_ensemble_captions_json_generation
    if isinstance(engines, int):
        engines = [_FakeEng() for _ in range(engines)]
    with pytest.raises(ValueError, match=match):
        eval_ensemble_captions_json_generation(engines, [], tqdm_visible=False, **kw)
