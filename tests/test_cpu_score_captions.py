"""CPU-only checks of scoring given captions (include/icz.h: icz_*_score_captions): every documented argument error of the
host-only check and of the six entries (no handle, no device) in the documented order, encode_captions / ids_from_beam on
hand-written cases, the ValueErrors of scoring.score_captions and of the five engine functions before an engine or a device is
touched, and the host oracle of tests/_scoring_oracle.py against the decode the project already pins."""
import ctypes

import numpy as np
import pytest
import torch

MODELS = ("butd", "aoa", "nic")
ENGINES = ("BUTDDetection_Eng", "AoADetection_Eng", "NIC_Eng", "BUTDSpatial_Eng")


def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _err():
    return _lib().icz_last_error()


def test_symbols_and_python_surface():
    L = _lib()
    for name in ("icz_score_captions_check", "icz_butd_score_captions", "icz_aoa_score_captions", "icz_nic_score_captions",
                 "icz_ensemble_score_captions", "icz_score_tokens", "icz_ensemble_score_tokens"):
        assert getattr(L, name).argtypes is not None, name
    from simpleimagecaptionzoo_amd import aoa, butd, engine, nic, scoring
    for cls in (butd.ButdHandle, aoa.AoaHandle, nic.NicHandle):
        assert cls._entries().score_captions.__name__ == "icz_%s_score_captions" % cls.family
        assert not hasattr(cls, "score_captions")                  # the frozen classes get no new method
    for name in ("score_captions", "captioner_score", "encode_captions", "ids_from_beam", "score_tokens", "ensemble_score_tokens"):
        assert callable(getattr(scoring, name)), name
    for eng in ENGINES:
        for name in ("score_captions_json", "rescore_captions_json", "reference_perplexity"):
            assert callable(getattr(getattr(engine, eng), name)), (eng, name)
    assert callable(engine.score_ensemble_captions_json) and callable(engine.rescore_ensemble_captions_json)


# (n_img, n, max_len, max_rows) -> message, in the documented order: n, max_len, the capacity
BAD = [
    ((4, 0, 8, 64), b"n=0 captions per image outside 1..8"),
    ((4, 9, 8, 64), b"n=9 captions per image outside 1..8"),
    ((4, 0, 0, 1), b"n=0 captions per image outside 1..8"),          # n is reported in front of max_len and the capacity
    ((4, 2, 0, 64), b"max_len=0 outside 1..256"),
    ((4, 2, 257, 64), b"max_len=257 outside 1..256"),
    ((99, 2, 0, 64), b"max_len=0 outside 1..256"),                   # max_len in front of the capacity
    ((33, 2, 8, 64), b"33 images x 2 captions exceed row capacity 64"),
    ((0, 1, 8, 64), b"0 images x 1 captions exceed row capacity 64"),
    ((-1, 1, 8, 64), b"exceed row capacity"),
]


def test_host_only_check():
    L = _lib()
    for args, msg in BAD:
        assert L.icz_score_captions_check(*args) == -1, msg
        assert msg in _err() and b"icz_score_captions_check" in _err(), (msg, _err())
    for args in ((64, 1, 1, 64), (8, 8, 256, 64), (1, 1, 20, 1)):
        assert L.icz_score_captions_check(*args) == 0, args


@pytest.mark.parametrize("model", MODELS + ("ensemble",))
def test_entries_report_arguments_before_the_handle(model):
    L = _lib()
    fn = getattr(L, "icz_%s_score_captions" % model)
    entry = b"icz_%s_score_captions" % model.encode()
    d = [ctypes.c_void_p(256 * (i + 1)) for i in range(4)]
    feats = (lambda p: ctypes.cast(p, ctypes.POINTER(ctypes.c_void_p))) if model == "ensemble" else (lambda p: p)
    for (n_img, n, max_len, cap), msg in BAD:
        if b"capacity 64" in msg and n_img > 0:
            continue                              # needs the handle's capacity
        assert fn(None, feats(d[0]), n_img, n, max_len, d[1], d[2], d[3], None) == -1
        msg = msg.split(b" 64")[0]                # without a handle the capacity is not known
        assert msg in _err() and entry in _err(), (msg, _err())
    for i in range(4):                            # null arguments, then the null handle
        ptrs = [None if j == i else d[j] for j in range(4)]
        assert fn(None, feats(ptrs[0]) if ptrs[0] is not None else None, 4, 2, 8, ptrs[1], ptrs[2], ptrs[3], None) == -1
        assert (entry + b": null argument") in _err(), _err()
    assert fn(None, feats(d[0]), 4, 2, 8, d[1], d[2], d[3], None) == -1
    assert (entry + b": null handle") in _err()


def test_kernel_alone_entries_refuse_bad_arguments():
    L = _lib()
    d = [ctypes.c_void_p(256 * (i + 1)) for i in range(4)]
    for args in ((None, None, 1, 64, 2, 53, d[1], d[2]), (d[0], None, 1, 64, 2, 53, None, d[2]), (d[0], None, 1, 64, 2, 53, d[1], None),
                 (d[0], None, 1, 64, 0, 53, d[1], d[2]), (d[0], None, 1, 64, 2, 0, d[1], d[2]), (d[0], None, 1, 52, 2, 53, d[1], d[2]),
                 (d[0], None, 0, 64, 2, 53, d[1], d[2])):
        assert L.icz_score_tokens(*args, None) == -1
        assert b"icz_score_tokens: bad arguments" in _err(), _err()
    assert L.icz_score_tokens(d[0], None, 2, 64, 2, 53, d[1], d[2], None) == -1
    assert b"icz_score_tokens: split-K slabs need a bias" in _err()
    one = lambda t, v: (t * 1)(v)
    lg, ns, ld = one(ctypes.c_void_p, 256), one(ctypes.c_int32, 1), one(ctypes.c_int32, 64)
    ens = L.icz_ensemble_score_tokens
    assert ens(0, lg, None, ns, ld, None, 2, 53, d[1], d[2], None) == -1 and b"0 members outside 1..4" in _err()
    assert ens(5, lg, None, ns, ld, None, 2, 53, d[1], d[2], None) == -1 and b"5 members outside 1..4" in _err()
    assert ens(1, None, None, ns, ld, None, 2, 53, d[1], d[2], None) == -1 and b"icz_ensemble_score_tokens: bad arguments" in _err()
    assert ens(1, lg, None, ns, ld, None, 2, 53, None, d[2], None) == -1 and b"bad arguments" in _err()
    assert ens(1, lg, None, ns, ld, one(ctypes.c_float, -1.0), 2, 53, d[1], d[2], None) == -1 and b"weight 0" in _err()
    assert ens(1, lg, None, ns, one(ctypes.c_int32, 52), None, 2, 53, d[1], d[2], None) == -1 and b"member 0: null logits, ld < V" in _err()
    assert ens(1, lg, None, one(ctypes.c_int32, 2), ld, None, 2, 53, d[1], d[2], None) == -1 and b"member 0: split-K slabs need a bias" in _err()


# ---- encode_captions / ids_from_beam ------------------------------------------------------------------------------------------
def test_encode_captions():
    from simpleimagecaptionzoo_amd.scoring import encode_captions
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    v = synthetic_vocab(12)                       # <pad> <sta> <end> <unk> w0 .. w7
    got = encode_captions(["w0 w3  w7", "", "zebra w1", "w2"], v)
    assert got.dtype == np.int64
    assert got.tolist() == [[4, 7, 11, 2], [2, 0, 0, 0], [3, 5, 2, 0], [6, 2, 0, 0]]          # <unk> = 3, an empty string is <end> alone
    assert encode_captions(["w0"], v, max_len=5).tolist() == [[4, 2, 0, 0, 0]]
    assert encode_captions([], v).shape == (0, 1)
    assert encode_captions([" ".join(["w1"] * 255)], v).shape == (1, 256)
    with pytest.raises(ValueError, match="256 words"):
        encode_captions([" ".join(["w1"] * 256)], v)
    with pytest.raises(ValueError, match="does not fit max_len 3"):
        encode_captions(["w0 w1 w2"], v, max_len=3)
    for bad in (0, 257):
        with pytest.raises(ValueError, match="max_len"):
            encode_captions(["w0"], v, max_len=bad)


def test_ids_from_beam():
    from simpleimagecaptionzoo_amd.scoring import ids_from_beam
    seqs = np.array([[1, 5, 6, 2, 0, 0], [1, 5, 6, 7, 8, 9], [1, 2, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]], np.float32)
    lens = np.array([4, 6, 2, 1], np.int32)
    want = [[5, 6, 2, 0, 0], [5, 6, 7, 8, 9], [2, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    got = ids_from_beam(seqs, lens)
    assert got.dtype == np.int64 and got.tolist() == want
    assert ids_from_beam(torch.tensor(seqs), torch.tensor(lens)).tolist() == want
    nb = ids_from_beam(seqs.reshape(2, 2, 6), lens.reshape(2, 2))                             # n-best lists [n_img, n_best, L]
    assert nb.tolist() == want
    junk = seqs.copy()
    junk[0, 4:] = 9                               # whatever lies behind the length is dropped
    assert ids_from_beam(junk, lens).tolist() == want
    for s, l in ((seqs, lens[:3]), (seqs[:, :1], lens), (seqs, np.array([4, 7, 2, 1]))):
        with pytest.raises(ValueError):
            ids_from_beam(s, l)


def test_scored_lengths_agree_with_the_oracle_rule():
    import _scoring_oracle as sco
    from simpleimagecaptionzoo_amd.scoring import scored_lengths
    ids = np.array([[2, 5, 5, 5], [5, 6, 7, 8], [0, 0, 0, 0], [5, 0, 2, 0], [5, 6, 2, 9], [0, 2, 0, 0], [5, 6, 7, 2]], np.int64)
    assert scored_lengths(ids).tolist() == sco.lengths(ids).tolist() == [1, 4, 0, 1, 3, 0, 4]
    rs = np.random.RandomState(0)
    ids = rs.randint(0, 5, size=(200, 7)).astype(np.int64)
    assert scored_lengths(ids).tolist() == sco.lengths(ids).tolist()
    assert sco.lengths(np.array([[5, 12, 2], [5, -1, 2]]), V=10).tolist() == [1, 1]            # outside [0, V): as a 0


# ---- Python level ------------------------------------------------------------------------------------------------------------
class _Untouched:
    """stands for a handle or an engine: the argument checks run before anything of it is looked at, except what a test hands it"""

    def __init__(self, **attrs):
        self.__dict__.update(attrs)

    def __getattr__(self, name):
        raise AssertionError("the argument checks touched .%s" % name)


GOOD_IDS = torch.tensor([[5, 2, 0], [6, 7, 2]])
BAD_N = [0, 9, 2.0, True, None, "2"]
BAD_IDS = [[], None, [[5, 2]], torch.tensor([[5.0, 2.0]]), torch.tensor([[5, 2]], dtype=torch.int32), torch.tensor([5, 2]),
           torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 4, dtype=torch.int64), torch.zeros(1, 257, dtype=torch.int64),
           np.zeros((2, 3), np.int32), torch.zeros(2, 3, 1, dtype=torch.int64)]


@pytest.mark.parametrize("fn", ["score_captions", "captioner_score"])
def test_score_captions_raises_before_the_device(fn):
    from simpleimagecaptionzoo_amd import scoring
    fn = getattr(scoring, fn)
    for n in BAD_N:
        with pytest.raises(ValueError, match="captions per image"):
            fn(_Untouched(), [], GOOD_IDS, n=n)
    for ids in BAD_IDS:
        with pytest.raises(ValueError, match="ids"):
            fn(_Untouched(), [], ids)
    with pytest.raises(ValueError, match="multiple of 3"):
        fn(_Untouched(), [], GOOD_IDS, n=3)


def test_score_captions_checks_ids_and_capacity_against_the_handle():
    from simpleimagecaptionzoo_amd.scoring import score_captions
    with pytest.raises(ValueError, match="7: outside the vocabulary \\[0, 7\\)"):
        score_captions(_Untouched(V=7), [], GOOD_IDS)
    with pytest.raises(ValueError, match="-1: outside the vocabulary"):
        score_captions(_Untouched(V=10), [], torch.tensor([[5, -1, 2]]))
    with pytest.raises(ValueError, match="1 images x 2 captions exceed the handle's row capacity 1"):
        score_captions(_Untouched(V=10, max_rows=1), [], GOOD_IDS, n=2)


ENTRY = {"image_id": 1, "caption": "a b"}
BAD_ENTRIES = [
    (None, 1, "entries must be a list"),
    ([ENTRY] * 3, 2, "3 entries are not a multiple of 2"),
    ([ENTRY, "a b"], 1, "entry 1: expected a dict"),
    ([{"caption": "a"}], 1, "entry 0: expected a dict"),
    ([{"image_id": 1}], 1, "entry 0: expected a dict"),
    ([{"image_id": 1, "caption": 5}], 1, "entry 0: expected a dict"),
    ([{"image_id": 1, "caption": " ".join(["a"] * 256)}], 1, "entry 0: caption with 256 words"),
    ([ENTRY, {"image_id": 2, "caption": "c"}], 2, "entry 1: image_id 2 inside the group of image 1"),
]


def _engine_fns():
    from simpleimagecaptionzoo_amd import engine
    out = []
    for eng in ENGINES:
        out.append(("%s.score_captions_json" % eng, getattr(engine, eng).score_captions_json, False, _Untouched))
        out.append(("%s.rescore_captions_json" % eng, getattr(engine, eng).rescore_captions_json, True, _Untouched))
    out.append(("score_ensemble_captions_json", engine.score_ensemble_captions_json, False, lambda: [_Untouched(), _Untouched()]))
    out.append(("rescore_ensemble_captions_json", engine.rescore_ensemble_captions_json, True, lambda: [_Untouched(), _Untouched()]))
    return out


def test_engine_functions_raise_before_an_engine_is_touched():
    for name, fn, rescore, who in _engine_fns():
        for n in BAD_N:
            with pytest.raises(ValueError, match="captions per image"):
                fn(who(), [], [ENTRY], n, tqdm_visible=False)
        for entries, n, match in BAD_ENTRIES:
            with pytest.raises(ValueError, match=match):
                fn(who(), [], entries, n, tqdm_visible=False)
        if rescore:
            for lp in ("avg", ("avg", -1.0), ("mean", 1.0), 3, ("wu", float("nan"))):
                with pytest.raises(ValueError, match="length_penalty"):
                    fn(who(), [], [ENTRY], 1, lp, tqdm_visible=False)


class _FakeEng(_Untouched):
    def __init__(self, V=10, device="cuda:0"):
        super().__init__(caption_vocab=[None] * V, device=device)


@pytest.mark.parametrize("fn", ["score_ensemble_captions_json", "rescore_ensemble_captions_json"])
def test_ensemble_engine_function_refusals(fn):
    from simpleimagecaptionzoo_amd import engine
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
    ]:
        with pytest.raises(ValueError, match=match):
            fn(engines, [], [ENTRY], 1, tqdm_visible=False, **kw)


def test_signatures():
    import inspect
    from simpleimagecaptionzoo_amd import engine, scoring
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(scoring.score_captions) == [("handle", E), ("feats", E), ("ids", E), ("n", 1)]
    assert sig(scoring.captioner_score)[2:] == [("ids", E), ("n", 1)]
    assert sig(scoring.encode_captions) == [("captions", E), ("vocab", E), ("max_len", None)]
    assert sig(scoring.ids_from_beam) == [("seqs", E), ("lens", E)]
    B = engine.BUTDDetection_Eng
    assert sig(B.score_captions_json)[1:] == [("dataloader", E), ("entries", E), ("captions_per_image", 1), ("tqdm_visible", True)]
    assert sig(B.rescore_captions_json)[1:] == [("dataloader", E), ("entries", E), ("captions_per_image", E), ("length_penalty", None),
                                                 ("tqdm_visible", True)]
    assert sig(B.reference_perplexity)[1:] == [("dataloader", E), ("tqdm_visible", True)]
    assert sig(engine.score_ensemble_captions_json) == [("engines", E), ("dataloader", E), ("entries", E), ("captions_per_image", 1),
                                                        ("tqdm_visible", True), ("weights", None)]
    assert sig(engine.rescore_ensemble_captions_json) == [("engines", E), ("dataloader", E), ("entries", E), ("captions_per_image", E),
                                                          ("length_penalty", None), ("tqdm_visible", True), ("weights", None)]
    for f in (engine.score_ensemble_captions_json, engine.rescore_ensemble_captions_json):
        assert inspect.signature(f).parameters["weights"].kind is inspect.Parameter.KEYWORD_ONLY


def test_pick_by_likelihood():
    """the host side of rescore_captions_json: the penalised argmax, ties to the first"""
    from simpleimagecaptionzoo_amd.beam import parse_length_penalty
    from simpleimagecaptionzoo_amd.engine import _pick_by_likelihood
    mk = lambda i, c, lp, t: {"image_id": i, "caption": c, "logprob": lp, "tokens": t, "logprobs": [], "score": 0.0}
    scored = [mk(7, "short", -4.0, 2), mk(7, "a much longer one", -6.0, 6), mk(7, "tie", -4.0, 2),
              mk(8, "", -0.5, 1), mk(8, "x", -0.5, 2), mk(8, "y z", -0.75, 3)]
    got = _pick_by_likelihood(scored, 3, parse_length_penalty(None))
    assert got == [{"image_id": 7, "caption": "short", "logprob": -4.0, "rank_score": -4.0},
                   {"image_id": 8, "caption": "", "logprob": -0.5, "rank_score": -0.5}]
    got = _pick_by_likelihood(scored, 3, parse_length_penalty(("avg", 1.0)))
    assert [g["caption"] for g in got] == ["a much longer one", "x"] and [g["rank_score"] for g in got] == [-1.0, -0.25]
    got = _pick_by_likelihood(scored, 3, parse_length_penalty(("wu", 0.7)))
    want = [-4.0 / (7 / 6.0) ** 0.7, -6.0 / (11 / 6.0) ** 0.7]
    assert got[0]["caption"] == ("short" if want[0] >= want[1] else "a much longer one") and got[0]["rank_score"] == max(want)


# ---- the oracle against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_tiny"])
def test_oracle_reproduces_the_sampling_oracle(golden_dir, name):
    """ids and float64 log-probs of _sampling_oracle.decode_model, scored by the new oracle: the same log-probs to 1e-12 -- the
    length rule and the feeding order agree with the decode the project pins"""
    import _ens_sampling_cases as ec
    import _sampling_oracle as so
    import _scoring_oracle as sco
    model, p, feats, _ = ec.host_member(golden_dir, name, end_boost=3.0)
    T, ended = 12, False
    for n, counts in ((1, None), (3, None)) + (((2, [36, 20, 11]),) if model == "aoa" else ()):
        u = np.random.RandomState(5 + n).rand(T, feats.shape[0] * n).astype(np.float32)
        ids, lps = so.decode_model(model, feats, p, n, u, T, counts=counts)
        ended = ended or bool((ids == 2).any())
        got = sco.score_model(model, feats, p, n, ids, counts=counts)
        # the sampler may draw <pad> (0) and go on; a given caption ends at its first 0: compared up to the scored length
        scored = np.arange(T)[None, :] < sco.lengths(ids)[:, None]
        assert np.abs(got - lps)[scored].max() <= 1e-12, (name, n, np.abs(got - lps)[scored].max())
        assert (got[~scored] == 0).all() and 2 * scored.sum() > (lps != 0).sum()          # most drawn tokens are compared
        if n == 3 and counts is None:             # a one-member "ensemble" of weight 1 is the model
            assert np.abs(sco.score_ensemble([(model, p, feats)], [2.0], n, ids) - lps)[scored].max() <= 1e-12
    assert ended                                  # finished rows were exercised


def test_ensemble_oracle_is_the_log_of_the_mean_probability(golden_dir):
    import _ens_sampling_cases as ec
    import _scoring_oracle as sco
    a = ec.host_member(golden_dir, "butd_dec_tiny", 0)[:3]
    b = ec.host_member(golden_dir, "butd_dec_tiny", 1)[:3]
    ids = np.array([[5, 9, 2, 0], [7, 7, 7, 7], [0, 0, 0, 0]], np.int64)
    la, lb = sco.score_model(*a[:1], a[2], a[1], 1, ids), sco.score_model(*b[:1], b[2], b[1], 1, ids)
    # only step 0 sees the same input under both: there the ensemble is the mean of the two probabilities
    both = sco.score_ensemble([a, b], [1.0, 3.0], 1, ids)
    want0 = np.log(0.25 * np.exp(la[:, 0]) + 0.75 * np.exp(lb[:, 0]))
    assert np.abs(both[:2, 0] - want0[:2]).max() <= 1e-12 and both[2].tolist() == [0, 0, 0, 0]
    assert np.abs(sco.score_ensemble([a, b], [1.0, 0.0], 1, ids) - la).max() <= 1e-12        # a zero weight drops the member
    assert np.abs(sco.score_ensemble([a, a], [0.2, 0.8], 1, ids) - la).max() <= 1e-12        # identical copies are the model
    x = (np.random.RandomState(1).randn(3, 50) * 3).astype(np.float32)
    assert abs(sco.ensemble_row_logp([x[0]], None, 7) - sco.row_logp(x[0], 7)) <= 1e-12
    assert abs(sco.ensemble_row_logp(list(x), [1, 1, 2], 7)
               - np.log(sum(w * np.exp(sco.row_logp(r, 7)) for w, r in zip([0.25, 0.25, 0.5], x)))) <= 1e-12
