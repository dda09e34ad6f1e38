"""CPU-only checks of the beam-search options (include/icz.h: icz_beam_opts): argument errors of icz_*_beam_search_opts reported
through icz_last_error before any device work, the Python parsing of the length penalty, and the Engine's refusal of the options
without beam search."""
import ctypes

import pytest

MODELS = ("butd", "aoa", "nic")


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _opts(n_best=1, block_ngram=0, lp_kind=0, lp_alpha=0.0):
    from simpleimagecaptionzoo_amd._lib import BeamOpts
    return BeamOpts(n_best, block_ngram, lp_kind, lp_alpha)


def _call(model, h, opts, ptrs=(None, None, None, None), beam=5):
    feats, seqs, lens, scores = ptrs
    fn = getattr(_lib(), "icz_%s_beam_search_opts" % model)
    return fn(h, feats, 4, beam, 20, None if opts is None else ctypes.byref(opts), seqs, lens, scores, None)


def test_opts_struct_layout():
    from simpleimagecaptionzoo_amd._lib import BeamOpts
    assert ctypes.sizeof(BeamOpts) == 16
    assert [f[0] for f in BeamOpts._fields_] == ["n_best", "block_ngram", "lp_kind", "lp_alpha"]


@pytest.mark.parametrize("model", MODELS)
def test_bad_options_are_reported_before_the_handle(model):
    L = _lib()
    cases = [
        (None, b"null options"),
        (_opts(n_best=0), b"n_best 0 outside 1..beam"),
        (_opts(n_best=6), b"n_best 6 outside 1..beam"),
        (_opts(block_ngram=1), b"block_ngram 1"),
        (_opts(block_ngram=5), b"block_ngram 5"),
        (_opts(block_ngram=-2), b"block_ngram -2"),
        (_opts(lp_kind=3), b"lp_kind 3 unknown"),
        (_opts(lp_kind=-1), b"lp_kind -1 unknown"),
        (_opts(lp_kind=1, lp_alpha=-0.5), b"lp_alpha"),
        (_opts(lp_kind=2, lp_alpha=float("nan")), b"lp_alpha"),
        (_opts(lp_kind=2, lp_alpha=float("inf")), b"lp_alpha"),
    ]
    for opts, msg in cases:
        assert _call(model, None, opts) == -1
        err = L.icz_last_error()
        assert msg in err, (model, msg, err)
        assert (b"icz_%s_beam_search_opts" % model.encode()) in err


@pytest.mark.parametrize("model", MODELS)
def test_null_argument_then_null_handle(model):
    L = _lib()
    good = _opts(n_best=5, block_ngram=3, lp_kind=2, lp_alpha=0.9)
    assert _call(model, None, good) == -1
    assert b"null argument" in L.icz_last_error()
    # the pointers are never dereferenced before the handle check: any non-null values do
    dummy = tuple(ctypes.c_void_p(256 * (i + 1)) for i in range(4))
    for i in range(4):
        ptrs = tuple(None if j == i else dummy[j] for j in range(4))
        assert _call(model, None, good, ptrs) == -1
        assert b"null argument" in L.icz_last_error()
    assert _call(model, None, good, dummy) == -1
    assert b"null handle" in L.icz_last_error()
    for ok in (_opts(), _opts(n_best=1, block_ngram=2), _opts(block_ngram=4, lp_kind=1, lp_alpha=0.0)):
        assert _call(model, None, ok, dummy) == -1
        assert b"null handle" in L.icz_last_error()


def test_length_penalty_parsing():
    from simpleimagecaptionzoo_amd.beam import make_opts, parse_length_penalty
    assert parse_length_penalty(None) == (0, 0.0)
    assert parse_length_penalty("avg_0.7") == (1, 0.7)
    assert parse_length_penalty("wu_0.9") == (2, 0.9)
    assert parse_length_penalty(("avg", 0.7)) == (1, 0.7)
    assert parse_length_penalty(("wu", 0)) == (2, 0.0)
    assert parse_length_penalty("avg_0") == (1, 0.0)
    for bad in ("avg", "wu_", "avg_x", "foo_0.7", "avg_-0.1", "wu_nan", "wu_inf", ("lin", 0.5), ("avg", -1.0), ("avg", "x"),
                ("avg",), 0.7, ""):
        with pytest.raises(ValueError):
            parse_length_penalty(bad)
    o = make_opts(3, "wu_0.9", 3)
    assert (o.n_best, o.block_ngram, o.lp_kind) == (3, 3, 2)
    assert abs(o.lp_alpha - 0.9) < 1e-7


@pytest.mark.parametrize("eng", ["BUTDDetection_Eng", "AoADetection_Eng", "NIC_Eng"])
def test_engine_options_need_beam_search(eng):
    from simpleimagecaptionzoo_amd import engine
    fn = getattr(engine, eng).eval_captions_json_generation
    # raised before the engine (or a device) is touched: no engine object needed
    for kw in ({"block_ngram": 3}, {"length_penalty": "wu_0.9"}, {"length_penalty": ("avg", 0.7), "block_ngram": 2}):
        with pytest.raises(ValueError, match="beam search"):
            fn(object(), [], eval_beam_size=-1, tqdm_visible=False, **kw)
    with pytest.raises(ValueError):
        fn(object(), [], eval_beam_size=3, tqdm_visible=False, length_penalty="avg_x")
    with pytest.raises(ValueError):
        fn(object(), [], eval_beam_size=3, tqdm_visible=False, block_ngram=5)
