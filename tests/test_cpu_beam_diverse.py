"""CPU-only checks of diverse beam search (include/icz.h: icz_beam_diversity): the struct layout, the argument errors of
icz_*_beam_search_diverse reported through icz_last_error in their documented order before any device work, the Python
validation of groups / diversity, and the Engine's refusals."""
import ctypes

import pytest

MODELS = ("butd", "aoa", "nic")


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _opts(n_best=1, block_ngram=0, lp_kind=0, lp_alpha=0.0):
    from simpleimagecaptionzoo_amd._lib import BeamOpts
    return BeamOpts(n_best, block_ngram, lp_kind, lp_alpha)


def _div(groups=1, diversity=0.0):
    from simpleimagecaptionzoo_amd._lib import BeamDiversity
    return BeamDiversity(groups, diversity)


DUMMY = tuple(ctypes.c_void_p(256 * (i + 1)) for i in range(4))


def _call(model, opts, div, ptrs=(None, None, None, None), beam=6):
    feats, seqs, lens, scores = ptrs
    fn = getattr(_lib(), "icz_%s_beam_search_diverse" % model)
    return fn(None, feats, 4, beam, 20, None if opts is None else ctypes.byref(opts), None if div is None else ctypes.byref(div),
              seqs, lens, scores, None)


def _err():
    return _lib().icz_last_error()


def test_diversity_struct_layout():
    from simpleimagecaptionzoo_amd._lib import BeamDiversity
    assert ctypes.sizeof(BeamDiversity) == 8
    assert [f[0] for f in BeamDiversity._fields_] == ["groups", "diversity"]
    assert BeamDiversity._fields_[0][1] is ctypes.c_int32 and BeamDiversity._fields_[1][1] is ctypes.c_float


@pytest.mark.parametrize("model", MODELS)
def test_argument_errors_in_order(model):
    entry = b"icz_%s_beam_search_diverse" % model.encode()
    bad_div = _div(groups=4)                     # does not divide 6
    cases = [
        # 1. the options, before anything else
        (None, None, (), b"null options"),
        (_opts(n_best=7), bad_div, (), b"n_best 7 outside 1..beam"),
        (_opts(block_ngram=5), bad_div, (), b"block_ngram 5"),
        (_opts(lp_kind=3), None, (), b"lp_kind 3 unknown"),
        (_opts(lp_kind=1, lp_alpha=float("nan")), None, (), b"lp_alpha"),
        # 2. a null diversity
        (_opts(), None, (), b"null diversity"),
        # 3. groups
        (_opts(), _div(groups=0), (), b"groups 0 outside 1..beam (6) or not dividing it"),
        (_opts(), _div(groups=7), (), b"groups 7 outside"),
        (_opts(), _div(groups=4, diversity=-1.0), (), b"groups 4 outside"),
        (_opts(), _div(groups=-2), (), b"groups -2 outside"),
        # 4. diversity
        (_opts(), _div(groups=3, diversity=-0.5), (), b"diversity -0.5 negative or not finite"),
        (_opts(), _div(groups=2, diversity=float("nan")), (), b"diversity nan"),
        (_opts(), _div(groups=1, diversity=float("inf")), (), b"diversity inf"),
        # 5. null arguments
        (_opts(n_best=6, block_ngram=3, lp_kind=2, lp_alpha=0.9), _div(3, 0.5), (), b"null argument"),
    ]
    for opts, div, _, msg in cases:
        assert _call(model, opts, div) == -1
        err = _err()
        assert msg in err, (model, msg, err)
        assert entry in err, err
    # 5. every output pointer must be non-null (never dereferenced before the handle check)
    for i in range(4):
        ptrs = tuple(None if j == i else DUMMY[j] for j in range(4))
        assert _call(model, _opts(), _div(2, 0.5), ptrs) == -1
        assert b"null argument" in _err()
    # 6. null handle last
    for opts, div, beam in ((_opts(), _div(), 6), (_opts(n_best=6, lp_kind=2, lp_alpha=0.9), _div(3, 0.5), 6),
                            (_opts(), _div(6, 2.0), 6), (_opts(n_best=8, block_ngram=3), _div(4, 0.3), 8), (_opts(), _div(1, 0.0), 1)):
        assert _call(model, opts, div, DUMMY, beam) == -1
        assert (entry + b": null handle") in _err()


def test_make_diversity():
    from simpleimagecaptionzoo_amd.beam import make_diversity
    d = make_diversity(3, 0.5, 6)
    assert (d.groups, d.diversity) == (3, 0.5)
    d = make_diversity(1, 0, 5)
    assert (d.groups, d.diversity) == (1, 0.0)
    assert make_diversity(8, 2, 8).groups == 8
    for groups, diversity, beam in ((0, 0.5, 6), (4, 0.5, 6), (7, 0.5, 6), (-1, 0.5, 6), (2, 0.5, 5), (2, -0.1, 6),
                                    (2, float("nan"), 6), (2, float("inf"), 6), (True, 0.5, 6), (2, True, 6), (2, False, 6),
                                    (2.0, 0.5, 6), ("2", 0.5, 6), (2, "0.5", 6), (None, 0.5, 6), (2, None, 6)):
        with pytest.raises(ValueError):
            make_diversity(groups, diversity, beam)


@pytest.mark.parametrize("cls", ["ButdHandle", "AoaHandle", "NicHandle"])
def test_handles_raise_before_the_device(cls):
    """bad groups / diversity raise ValueError before the handle or the features are looked at"""
    import importlib
    mod = importlib.import_module("simpleimagecaptionzoo_amd." + {"ButdHandle": "butd", "AoaHandle": "aoa", "NicHandle": "nic"}[cls])
    fn = getattr(mod, cls).beam_search_opts
    for kw in ({"groups": 4}, {"groups": 2, "diversity": -1.0}, {"groups": True}, {"diversity": float("nan")}):
        with pytest.raises(ValueError):
            fn(object(), None, 6, 20, **kw)


@pytest.mark.parametrize("eng", ["BUTDDetection_Eng", "AoADetection_Eng", "NIC_Eng"])
def test_engine_diversity_errors(eng):
    from simpleimagecaptionzoo_amd import engine
    fn = getattr(engine, eng).eval_captions_json_generation
    # raised before the engine (or a device) is touched: no engine object needed
    for kw in ({"beam_groups": 3}, {"diversity": 0.5}, {"beam_groups": 2, "diversity": 0.5, "block_ngram": 3}):
        with pytest.raises(ValueError, match="beam search"):
            fn(object(), [], eval_beam_size=-1, tqdm_visible=False, **kw)
    for kw in ({"beam_groups": 4}, {"beam_groups": 0}, {"beam_groups": 7}, {"beam_groups": 3, "diversity": -0.5},
               {"beam_groups": 3, "diversity": float("inf")}, {"beam_groups": True}):
        with pytest.raises(ValueError):
            fn(object(), [], eval_beam_size=6, tqdm_visible=False, **kw)
