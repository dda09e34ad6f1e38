"""CPU-only checks of the sampling decode (include/icz.h: icz_sample_opts, icz_*_sample_decode): the exported symbols and the struct
layout, every argument error through the host-only check, the entries themselves (no handle, no device) and the Engine method,
and the host oracle of tests/_sampling_oracle.py against itself."""
import ctypes

import numpy as np
import pytest
import torch

MODELS = ("butd", "aoa", "nic")
ENGINES = ("BUTDDetection_Eng", "AoADetection_Eng", "NIC_Eng")


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _opts(temperature=1.0, top_k=0, top_p=1.0):
    from simpleimagecaptionzoo_amd._lib import SampleOpts
    return SampleOpts(temperature, top_k, top_p)


def test_symbols_and_struct_layout():
    from simpleimagecaptionzoo_amd._lib import SampleOpts
    L = _lib()
    for name in ("icz_sample_decode_check", "icz_butd_sample_decode", "icz_aoa_sample_decode", "icz_nic_sample_decode", "icz_sample_filter_draw"):
        assert hasattr(L, name), name
    assert ctypes.sizeof(SampleOpts) == 12
    assert [f[0] for f in SampleOpts._fields_] == ["temperature", "top_k", "top_p"]
    from simpleimagecaptionzoo_amd import aoa, butd, captioner, engine, nic
    for cls in (butd.ButdHandle, aoa.AoaHandle, nic.NicHandle, captioner.BUTDDetection_Captioner, aoa.AoADetection_Captioner,
                nic.NICDecoder_Captioner):
        assert callable(getattr(cls, "sample_decode")), cls
    for eng in ENGINES:
        assert callable(getattr(getattr(engine, eng), "sample_captions_json_generation"))


# (options, n_img, n, V, max_rows) -> message
BAD = [
    ((None, 4, 1, 100, 64), b"null options"),
    ((_opts, 4, 0, 100, 64), b"n=0 samples per image outside 1..8"),
    ((_opts, 4, 9, 100, 64), b"n=9 samples per image outside 1..8"),
    ((lambda: _opts(temperature=0.0), 4, 1, 100, 64), b"temperature 0 not positive"),
    ((lambda: _opts(temperature=-1.0), 4, 1, 100, 64), b"temperature -1 not positive"),
    ((lambda: _opts(temperature=float("nan")), 4, 1, 100, 64), b"temperature nan"),
    ((lambda: _opts(temperature=float("inf")), 4, 1, 100, 64), b"temperature inf"),
    ((lambda: _opts(top_k=-1), 4, 1, 100, 64), b"top_k -1 outside 0..V (100)"),
    ((lambda: _opts(top_k=101), 4, 1, 100, 64), b"top_k 101 outside 0..V (100)"),
    ((lambda: _opts(top_p=0.0), 4, 1, 100, 64), b"top_p 0 outside (0, 1]"),
    ((lambda: _opts(top_p=1.5), 4, 1, 100, 64), b"top_p 1.5 outside (0, 1]"),
    ((lambda: _opts(top_p=float("nan")), 4, 1, 100, 64), b"top_p nan"),
    ((_opts, 33, 2, 100, 64), b"33 images x 2 samples exceed row capacity 64"),
    ((_opts, 0, 1, 100, 64), b"exceed row capacity"),
]


def test_host_only_check():
    L = _lib()
    for (mk, n_img, n, V, cap), msg in BAD:
        o = mk() if mk else None
        assert L.icz_sample_decode_check(None if o is None else ctypes.byref(o), n_img, n, V, cap) == -1, msg
        assert msg in L.icz_last_error(), (msg, L.icz_last_error())
    for o, n_img, n in ((_opts(), 64, 1), (_opts(0.7, 100, 0.9), 8, 8), (_opts(2.0, 1, 1e-6), 1, 1)):
        assert L.icz_sample_decode_check(ctypes.byref(o), n_img, n, 100, 64) == 0


@pytest.mark.parametrize("model", MODELS)
def test_entries_report_arguments_before_the_handle(model):
    L = _lib()
    fn = getattr(L, "icz_%s_sample_decode" % model)
    entry = b"icz_%s_sample_decode" % model.encode()
    d = [ctypes.c_void_p(256 * (i + 1)) for i in range(4)]
    for (mk, n_img, n, V, cap), msg in BAD:
        if b"capacity" in msg or b"outside 0..V" in msg and b"101" in msg:
            continue                              # these need the handle's V / capacity
        o = mk() if mk else None
        assert fn(None, d[0], n_img, n, 20, None if o is None else ctypes.byref(o), 0, None, d[1], d[2], d[3], None) == -1
        msg = msg.split(b" (100)")[0]             # without a handle the vocabulary size is not known
        assert msg in L.icz_last_error() and entry in L.icz_last_error(), (msg, L.icz_last_error())
    o = _opts(0.8, 5, 0.9)
    for i in range(4):                            # null arguments, then the null handle
        ptrs = [None if j == i else d[j] for j in range(4)]
        assert fn(None, ptrs[0], 4, 2, 20, ctypes.byref(o), 0, None, ptrs[1], ptrs[2], ptrs[3], None) == -1
        assert (entry + b": null argument") in L.icz_last_error()
    assert fn(None, d[0], 4, 2, 20, ctypes.byref(o), 0, None, d[1], d[2], d[3], None) == -1
    assert (entry + b": null handle") in L.icz_last_error()


PY_BAD = [{"n": 0}, {"n": 9}, {"n": 2.0}, {"n": True}, {"temperature": 0}, {"temperature": -0.5}, {"temperature": float("nan")},
          {"temperature": float("inf")}, {"temperature": "1"}, {"top_k": -1}, {"top_k": 1.5}, {"top_k": True}, {"top_p": 0}, {"top_p": 1.01},
          {"top_p": float("nan")}, {"top_p": None}]


@pytest.mark.parametrize("cls", ["ButdHandle", "AoaHandle", "NicHandle"])
def test_handles_raise_before_the_device(cls):
    import importlib
    mod = importlib.import_module("simpleimagecaptionzoo_amd." + {"ButdHandle": "butd", "AoaHandle": "aoa", "NicHandle": "nic"}[cls])
    fn = getattr(mod, cls).sample_decode
    for kw in PY_BAD:
        with pytest.raises(ValueError):
            fn(object(), None, **kw)

    class V10:
        V = 10
    with pytest.raises(ValueError, match="vocabulary"):
        fn(V10(), None, top_k=11)


@pytest.mark.parametrize("eng", ENGINES)
def test_engine_errors(eng):
    from simpleimagecaptionzoo_amd import engine
    fn = getattr(engine, eng).sample_captions_json_generation
    for kw in PY_BAD:
        kw = {("samples_per_image" if k == "n" else k): v for k, v in kw.items()}
        with pytest.raises(ValueError):
            fn(object(), [], tqdm_visible=False, **kw)       # raised before the engine (or a device) is touched
    for seed in (-1, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            fn(object(), [], seed=seed, tqdm_visible=False)

    class Stub:
        caption_vocab = list(range(10))
    with pytest.raises(ValueError, match="vocabulary"):
        fn(Stub(), [], top_k=11, tqdm_visible=False)


def test_eval_signature_unchanged():
    import inspect
    from simpleimagecaptionzoo_amd import engine
    sig = inspect.signature(engine.BUTDDetection_Eng.eval_captions_json_generation)
    assert list(sig.parameters) == ["self", "dataloader", "eval_beam_size", "tqdm_visible", "length_penalty", "block_ngram", "beam_groups",
                                    "diversity"]
    sig = inspect.signature(engine.BUTDDetection_Eng.sample_captions_json_generation)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [
        ("samples_per_image", 1), ("temperature", 1.0), ("top_k", 0), ("top_p", 1.0), ("seed", 0), ("tqdm_visible", True)]


# ---- the oracle against itself ------------------------------------------------------------------------------------------------
def _rows(V, rows, seed, scale=3.0):
    return (np.random.RandomState(seed).randn(rows, V) * scale).astype(np.float32)


def test_oracle_top_k_1_is_the_argmax():
    import _sampling_oracle as so
    x = _rows(300, 6, 0)
    x[2, [7, 90]] = x[2].max() + 1.0                 # a tie of the two largest: the lowest index
    for r in range(x.shape[0]):
        for u in (0.0, 0.3, 0.999999):
            for temp in (0.5, 1.0, 3.0):
                tok, _, keep = so.sample_row(x[r], u, temp, 1, 1.0)
                assert tok == int(np.argmax(x[r])) and keep.sum() == 1
    assert so.sample_row(x[2], 0.9, 1.0, 1, 1.0)[0] == 7


def test_oracle_top_p_to_zero_keeps_one_token():
    import _sampling_oracle as so
    x = _rows(300, 4, 1)
    for r in range(4):
        for k in (0, 40):
            tok, _, keep = so.sample_row(x[r], 0.77, 1.3, k, 1e-9)
            assert keep.sum() == 1 and tok == int(np.argmax(x[r]))


def test_oracle_filters_off_is_the_plain_draw():
    import _sampling_oracle as so
    from oracle import butd as ob
    V = 257
    x = _rows(V, 8, 2)
    u = np.random.RandomState(3).rand(8).astype(np.float32)
    want = ob.inverse_cdf_draw(torch.softmax(torch.from_numpy(x).double(), 1), u.astype(np.float64))
    for r in range(8):
        for k in (0, V):
            tok, lp, keep = so.sample_row(x[r], u[r], 1.0, k, 1.0)
            assert tok == int(want[r]) and keep.all()
            assert abs(lp - float(torch.log_softmax(torch.from_numpy(x[r]).double(), 0)[tok])) < 1e-12


def test_oracle_filter_sets():
    import _sampling_oracle as so
    x = np.array([0.0, 2.0, 2.0, 1.0, 2.0, -1.0, 1.0], np.float32)
    assert (so.filter_masses(x, 1.0, 2, 1.0) > 0).tolist() == [False, True, True, False, False, False, False]      # ties: lowest index
    assert (so.filter_masses(x, 1.0, 4, 1.0) > 0).tolist() == [False, True, True, True, True, False, False]
    # nucleus: q = (e^2, e^2, e^2, e, e, 1, e^-1) / Z in order 1, 2, 4, 3, 6, 0, 5; keep while the mass before is < top_p
    z = 3 * np.e ** 2 + 2 * np.e + 1 + np.e ** -1
    p_two = 2 * np.e ** 2 / z
    assert (so.filter_masses(x, 1.0, 0, p_two - 1e-6) > 0).sum() == 2
    assert (so.filter_masses(x, 1.0, 0, p_two + 1e-6) > 0).tolist() == [False, True, True, False, True, False, False]
    # the temperature sharpens: at 0.25 the three 2.0s hold more of the mass
    assert (so.filter_masses(x, 0.25, 0, 0.99) > 0).sum() < (so.filter_masses(x, 4.0, 0, 0.99) > 0).sum()
    # filtered tokens are never drawn
    m = so.filter_masses(x, 1.0, 3, 1.0)
    for u in np.linspace(0, 0.999, 50):
        assert so.draw(m, u) in (1, 2, 4)
