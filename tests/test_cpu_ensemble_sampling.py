"""CPU-only checks of an ensemble's sampling decode (include/icz.h: icz_ensemble_sample_decode, icz_ensemble_sample_filter_draw): the
argument errors of both entries through icz_last_error in their stated order, the ValueErrors of EnsembleHandle, CaptionEnsemble and
the two engine functions raised before any device work, and the ensemble oracle of tests/_ens_sampling_cases.py against itself."""
import ctypes as C

import pytest

FAKE = [C.c_void_p(256 * (i + 1)) for i in range(6)]      # never dereferenced: every check below runs before they would be


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _err():
    return _lib().icz_last_error()


def _opts(temperature=1.0, top_k=0, top_p=1.0):
    from simpleimagecaptionzoo_amd._lib import SampleOpts
    return SampleOpts(temperature, top_k, top_p)


def test_symbols():
    L = _lib()
    for name in ("icz_ensemble_sample_decode", "icz_ensemble_sample_filter_draw"):
        assert hasattr(L, name), name
    from simpleimagecaptionzoo_amd import engine, ensemble
    assert callable(ensemble.EnsembleHandle.sample_decode) and callable(ensemble.CaptionEnsemble.sample_decode)
    assert callable(engine.sample_ensemble_captions_json_generation) and callable(engine.consensus_ensemble_captions_json_generation)


# (options, n) -> message, in the order the entry reports them
BAD_OPTS = [
    (None, 1, b"null options"),
    (_opts, 0, b"n=0 samples per image outside 1..8"),
    (_opts, 9, b"n=9 samples per image outside 1..8"),
    (lambda: _opts(temperature=0.0), 1, b"temperature 0 not positive"),
    (lambda: _opts(temperature=float("nan")), 1, b"temperature nan"),
    (lambda: _opts(temperature=float("inf")), 1, b"temperature inf"),
    (lambda: _opts(top_k=-1), 1, b"top_k -1 outside 0..V"),
    (lambda: _opts(top_p=0.0), 1, b"top_p 0 outside (0, 1]"),
    (lambda: _opts(top_p=1.5), 1, b"top_p 1.5 outside (0, 1]"),
    (lambda: _opts(top_p=float("nan")), 1, b"top_p nan"),
]


def test_sample_decode_reports_arguments_before_the_handle():
    L = _lib()
    entry = b"icz_ensemble_sample_decode"
    feats = (C.c_void_p * 2)(FAKE[0].value, FAKE[1].value)
    for mk, n, msg in BAD_OPTS:
        o = mk() if mk else None
        # every other argument null as well: the options are reported first
        assert L.icz_ensemble_sample_decode(None, None, 4, n, 20, None if o is None else C.byref(o), 0, None, None, None, None, None) == -1
        assert msg in _err() and entry in _err(), (msg, _err())
    o = _opts(0.8, 5, 0.9)
    d = [feats, FAKE[2], FAKE[3], FAKE[4]]
    for i in range(4):                            # null arguments, then the null handle
        a = [None if j == i else d[j] for j in range(4)]
        assert L.icz_ensemble_sample_decode(None, a[0], 4, 2, 20, C.byref(o), 0, None, a[1], a[2], a[3], None) == -1
        assert (entry + b": null argument") in _err(), _err()
    assert L.icz_ensemble_sample_decode(None, feats, 4, 2, 20, C.byref(o), 0, None, FAKE[2], FAKE[3], FAKE[4], None) == -1
    assert (entry + b": null handle") in _err(), _err()


def _filter_draw(M=1, opts=_opts, logits=True, bias=None, nsplit=(1,), ld=(8,), weights=None, rows=2, V=5, uniforms=True, tok=True, logp=True):
    n = max(1, len(nsplit))
    lg = (C.c_void_p * n)(*([FAKE[0].value] * n)) if logits else None
    bs = (C.c_void_p * n)(*bias) if bias is not None else None
    ns = (C.c_int32 * n)(*nsplit)
    ldv = (C.c_int32 * n)(*ld)
    w = (C.c_float * len(weights))(*weights) if weights is not None else None
    o = opts() if opts else None
    return _lib().icz_ensemble_sample_filter_draw(M, lg, bs, ns, ldv, w, rows, V, None if o is None else C.byref(o), FAKE[1] if uniforms else None,
                                                  FAKE[2] if tok else None, FAKE[3] if logp else None, None, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(opts=None, M=0, logits=False), b"null options"),                      # the options in front of everything else
    (dict(opts=lambda: _opts(temperature=-1.0), M=0), b"temperature -1 not positive"),
    (dict(opts=lambda: _opts(top_k=6), M=5), b"top_k 6 outside 0..V (5)"),
    (dict(opts=lambda: _opts(top_p=0.0), logits=False), b"top_p 0 outside (0, 1]"),
    (dict(M=0, logits=False), b"0 members outside 1..4"),
    (dict(M=5), b"5 members outside 1..4"),
    (dict(logits=False), b"bad arguments"),
    (dict(uniforms=False), b"bad arguments"),
    (dict(tok=False), b"bad arguments"),
    (dict(logp=False), b"bad arguments"),
    (dict(rows=0), b"bad arguments"),
    (dict(weights=[-1.0]), b"weight 0 (-1) negative"),
    (dict(ld=(4,)), b"member 0: null logits, ld < V"),
    (dict(nsplit=(0,)), b"nsplit < 1"),
    (dict(nsplit=(2,)), b"split-K slabs need a bias"),
    (dict(M=2, nsplit=(1, 3), ld=(8, 8), bias=[FAKE[4].value, None]), b"member 1: split-K slabs need a bias"),
])
def test_filter_draw_errors(kw, msg):
    assert _filter_draw(**kw) == -1
    assert msg in _err() and b"icz_ensemble_sample_filter_draw" in _err(), _err()


# ---- Python level ----------------------------------------------------------------------------------------------------------
PY_BAD = [{"n": 0}, {"n": 9}, {"n": 2.0}, {"n": True}, {"temperature": 0}, {"temperature": -0.5}, {"temperature": float("nan")},
          {"temperature": float("inf")}, {"temperature": "1"}, {"top_k": -1}, {"top_k": 1.5}, {"top_k": True}, {"top_p": 0}, {"top_p": 1.01},
          {"top_p": float("nan")}, {"top_p": None}]


class _Untouched:
    """stands for self: the option checks run before anything of it is looked at, except what a test hands it"""

    def __init__(self, **attrs):
        self.__dict__.update(attrs)

    def __getattr__(self, name):
        raise AssertionError("the argument checks touched .%s" % name)


@pytest.mark.parametrize("cls", ["EnsembleHandle", "CaptionEnsemble"])
def test_handle_and_captioner_raise_before_the_device(cls):
    from simpleimagecaptionzoo_amd import ensemble
    fn = getattr(ensemble, cls).sample_decode
    for kw in PY_BAD:
        with pytest.raises(ValueError):
            fn(_Untouched(), None, **kw)
    for rng in (1.5, "seed", True, [0.5]):
        with pytest.raises(ValueError, match="rng"):
            fn(_Untouched(V=10), None, rng=rng)
    with pytest.raises(ValueError, match="vocabulary"):
        ensemble.EnsembleHandle.sample_decode(_Untouched(V=10), None, top_k=11)


class _FakeEng(_Untouched):
    def __init__(self, V=10, device="cuda:0"):
        super().__init__(caption_vocab=[None] * V, device=device)


@pytest.mark.parametrize("fn", ["sample_ensemble_captions_json_generation", "consensus_ensemble_captions_json_generation"])
def test_engine_function_refusals(fn):
    from simpleimagecaptionzoo_amd import engine
    consensus = fn.startswith("consensus")
    fn = getattr(engine, fn)
    two = lambda: [_FakeEng(), _FakeEng()]
    for engines, kw, match in [
        ([], {}, "1..4 members"),
        ([_FakeEng() for _ in range(5)], {}, "1..4 members"),
        ([_FakeEng(10), _FakeEng(11)], {}, "vocabularies differ"),
        ([_FakeEng(device="cuda:0"), _FakeEng(device="cuda:1")], {}, "different devices"),
        (two(), dict(weights=[1.0]), "2 members"),
        (two(), dict(weights=[1.0, -2.0]), "finite real >= 0"),
        (two(), dict(weights=[0.0, 0.0]), "sum to 0"),
        (two(), dict(top_k=11), "vocabulary"),
    ]:
        with pytest.raises(ValueError, match=match):
            fn(engines, [], tqdm_visible=False, **kw)
    for kw in PY_BAD:
        kw = {("samples_per_image" if k == "n" else k): v for k, v in kw.items()}
        with pytest.raises(ValueError):
            fn(two(), [], tqdm_visible=False, **kw)
    for seed in (-1, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            fn(two(), [], seed=seed, tqdm_visible=False)
    if consensus:
        with pytest.raises(ValueError, match="samples_per_image 1 outside 2..8"):
            fn(two(), [], samples_per_image=1, tqdm_visible=False)


def test_signatures():
    import inspect
    from simpleimagecaptionzoo_amd import engine, ensemble
    want = [("n", 1), ("max_len", 20), ("temperature", 1.0), ("top_k", 0), ("top_p", 1.0), ("rng", None)]
    for cls in (ensemble.EnsembleHandle, ensemble.CaptionEnsemble):
        sig = inspect.signature(cls.sample_decode)
        assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == want, cls
    sig = inspect.signature(engine.sample_ensemble_captions_json_generation)
    assert [(k, v.default) for k, v in sig.parameters.items()][2:] == [
        ("samples_per_image", 1), ("temperature", 1.0), ("top_k", 0), ("top_p", 1.0), ("seed", 0), ("tqdm_visible", True), ("weights", None)]
    assert sig.parameters["weights"].kind is inspect.Parameter.KEYWORD_ONLY


# ---- the oracle against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["butd2", "aoa2", "nic2", "mixed3"])
def test_ensemble_oracle_fp32_filter_against_float64(golden_dir, case):
    """The reference alone stays inside the cap of the GPU test: on the inputs of test_gpu_ensemble_sampling's oracle cases, the
    draws along the oracle's own rows change in at most 2 of the 48 rows when its filter runs in fp32, and every such row shows
    one of the margins that excuse a row there."""
    import _ens_sampling_cases as ec
    specs, weights, counts = ec.CASES[case]
    members = [ec.host_member(golden_dir, name, seed)[:3] for name, seed in specs]
    parts = ec.host_parts(members, counts)
    V = members[0][1][[k for k in members[0][1] if k.endswith("predict.bias")][0]].shape[0]
    differing, rows_total = 0, 0
    for n in (1, 3):
        rows = ec.N_IMG * n
        for i, opts in enumerate(ec.option_sets(V)):
            u = ec.uniforms(rows, 7 * n + i)
            traces = []
            w_ids, _ = ec.oracle_decode(parts, weights, n, u, opts, traces)
            differing += ec.self_differences(traces, w_ids, u, n, opts)
            rows_total += rows
    print("ensemble oracle %s: fp32 filter against float64 filter: %d of %d rows differ" % (case, differing, rows_total))
    assert rows_total == 48
    assert differing <= ec.MAX_DIFFERING_ROWS
