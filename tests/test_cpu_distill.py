"""Host side of word-level distillation (no GPU): the new symbols and the Python surface, every argument error of icz_distill_check
and of the three icz_*_xe_backward_distill entries in the documented order (no handle, no device), the Engine's refusals before an
engine is touched, and the float64 oracle of the loss (tests/_distill_oracle.py) against itself."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

import _distill_oracle as do
from simpleimagecaptionzoo_amd import _lib
from simpleimagecaptionzoo_amd._lib import AoaParams, ButdParams, DistillOpts, NicParams

FAKE = 4096          # a non-null "device pointer" that no host-only path dereferences


def test_symbols_and_python_surface():
    L = _lib.lib()
    for name in ("icz_distill_check", "icz_distill_loss", "icz_butd_xe_backward_distill", "icz_aoa_xe_backward_distill",
                 "icz_nic_xe_backward_distill", "icz_aoa_xe_backward_dlogits", "icz_nic_xe_backward_dlogits"):
        assert getattr(L, name).argtypes is not None, name
    from simpleimagecaptionzoo_amd import distill, engine, handle
    from simpleimagecaptionzoo_amd.aoa import AoaHandle
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.nic import NicHandle
    assert "xe_backward_distill" in handle._ENTRIES
    for cls in (ButdHandle, AoaHandle, NicHandle):
        table = vars(cls._entries())
        assert table["xe_backward_distill"].__name__ == "icz_%s_xe_backward_distill" % cls.family
        assert table["xe_backward_dlogits"].__name__ == "icz_%s_xe_backward_dlogits" % cls.family
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(distill.xe_backward_distill)[:8] == [("handle", E), ("grads", E), ("teacher_logits", E), ("weights", None), ("alpha", 0.5),
                                                    ("temperature", 1.0), ("smoothing", 0.1), ("n_tokens_global", 0.0)]
    assert sig(distill.distill_loss)[:3] == [("student", E), ("teacher_logits", E), ("targets", E)]
    assert sig(distill.teacher_logits) == [("handles", E), ("feats_list", E), ("captions", E), ("lengths", E)]
    want = [("dataloader", E), ("optimizer", E), ("criterion", E), ("teachers", E), ("tqdm_visible", True), ("rngs", None), ("alpha", 0.5),
            ("temperature", 1.0), ("weights", None)]
    for eng in ("BUTDDetection_Eng", "AoADetection_Eng", "NIC_Eng", "BUTDSpatial_Eng"):
        fn = getattr(engine, eng).distill_training_epoch
        assert sig(fn)[1:] == want, eng
        kinds = [p.kind for p in inspect.signature(fn).parameters.values()]
        assert kinds[-3:] == [inspect.Parameter.KEYWORD_ONLY] * 3


# ---- the argument rules of icz_distill_opts ----------------------------------------------------------------------------------------
def _arrays(M, ld=100, null_member=None):
    t = (C.c_void_p * 4)(*[None if m == null_member else FAKE + 64 * m for m in range(4)])
    l = (C.c_int32 * 4)(*([ld] * 4))
    return t, l


def _opts(M=2, teacher=True, ld=True, weights=None, alpha=0.5, tau=1.0, sigma=0.1, ldv=100, null_member=None):
    t, l = _arrays(M, ldv, null_member)
    w = (C.c_float * 4)(*weights) if weights is not None else None
    o = DistillOpts(M, t if teacher else None, l if ld else None, w, alpha, tau, sigma)
    o._keep = (t, l, w)
    return o


# every rule in the documented order: each entry breaks rule i and every rule behind it that it can, so that the message shows which
# one was tested first
BAD_TAIL = dict(weights=[-1.0, 1.0, 1.0, 1.0], ldv=10, null_member=1)
RULES = [
    ("null options", None),
    ("teachers outside 1..4", dict(M=0, alpha=2.0, tau=0.1, sigma=1.0, **BAD_TAIL)),
    ("teachers outside 1..4", dict(M=5, alpha=2.0, tau=0.1, sigma=1.0, **BAD_TAIL)),
    ("alpha 2 outside", dict(alpha=2.0, tau=0.1, sigma=1.0, **BAD_TAIL)),
    ("alpha -0.5 outside", dict(alpha=-0.5, tau=0.1, sigma=1.0, **BAD_TAIL)),
    ("alpha nan outside", dict(alpha=float("nan"), tau=0.1, sigma=1.0, **BAD_TAIL)),
    ("temperature 0.1 outside", dict(tau=0.1, sigma=1.0, **BAD_TAIL)),
    ("temperature 9 outside", dict(tau=9.0, sigma=1.0, **BAD_TAIL)),
    ("temperature nan outside", dict(tau=float("nan"), sigma=1.0, **BAD_TAIL)),
    ("smoothing 1 outside", dict(sigma=1.0, **BAD_TAIL)),
    ("smoothing -0.1 outside", dict(sigma=-0.1, **BAD_TAIL)),
    ("null teacher or ld", dict(teacher=False, weights=[-1.0, 1.0, 1.0, 1.0], ldv=10)),
    ("null teacher or ld", dict(ld=False, weights=[-1.0, 1.0, 1.0, 1.0], ldv=10)),
    ("teacher 1 is null", dict(**BAD_TAIL)),
    ("ld[0]=10 below the vocabulary size 53", dict(weights=[-1.0, 1.0, 1.0, 1.0], ldv=10)),          # (needs V: icz_distill_check only)
    ("weight 0 (-1) negative", dict(weights=[-1.0, 1.0, 1.0, 1.0])),
    ("weight 1 (nan) negative or not finite", dict(weights=[1.0, float("nan"), 1.0, 1.0])),
    ("the weights sum to 0", dict(weights=[0.0, 0.0, 1.0, 1.0])),
]


def _err():
    return _lib.lib().icz_last_error().decode()


def test_distill_check_errors_in_the_documented_order():
    L = _lib.lib()
    for match, kw in RULES:
        o = None if kw is None else _opts(**kw)
        assert L.icz_distill_check(C.byref(o) if o is not None else None, 53) == -1, match
        assert match in _err(), (match, _err())
        assert _err().startswith("icz_distill_check: ")
    for kw in (dict(), dict(M=1), dict(M=4, weights=[0.0, 1.0, 2.0, 0.5]), dict(alpha=0.0), dict(alpha=1.0), dict(tau=0.25), dict(tau=8.0),
               dict(sigma=0.0), dict(ldv=53)):
        o = _opts(**kw)
        assert L.icz_distill_check(C.byref(o), 53) == 0, (kw, _err())


@pytest.mark.parametrize("family, Params", [("butd", ButdParams), ("aoa", AoaParams), ("nic", NicParams)])
def test_entry_errors_in_the_documented_order_without_a_handle(family, Params):
    """rules 1 - 6 and 8 (rule 7 needs the handle's vocabulary), then 9 (null grads or loss) and 10 (null handle): nothing touches a device"""
    L = _lib.lib()
    fn = getattr(L, "icz_%s_xe_backward_distill" % family)
    who = "icz_%s_xe_backward_distill: " % family
    grads = Params()
    loss = C.c_void_p(FAKE)

    def call(o, g, l):
        args = [None, C.byref(o) if o is not None else None, C.byref(g) if g is not None else None]
        if family == "nic":
            args.append(None)          # dfeatures_out
        return fn(*args, l, 0.0, None)
    for match, kw in RULES:
        if "below the vocabulary" in match:
            continue
        o = None if kw is None else _opts(**kw)
        assert call(o, None, None) == -1, match          # (grads, loss and the handle are bad too: the options come first)
        assert match in _err() and _err().startswith(who), (match, _err())
    good = _opts(ldv=10)             # (ld below any vocabulary: without a handle rule 7 waits)
    assert call(good, None, loss) == -1 and "null grads or loss" in _err()
    assert call(good, grads, None) == -1 and "null grads or loss" in _err()
    assert call(good, grads, loss) == -1 and _err() == who + "null handle"
    # the backward entries for an upstream gradient: a null handle is refused as icz_butd_xe_backward_dlogits refuses it
    dl = getattr(L, "icz_%s_xe_backward_dlogits" % family)
    assert (dl(None, C.c_void_p(FAKE), C.byref(grads), None, None) if family == "nic" else dl(None, C.c_void_p(FAKE), C.byref(grads), None)) == -1


def test_python_option_checks():
    from simpleimagecaptionzoo_amd.distill import check_opts
    assert check_opts(2, [1, 3], 0.0, 0.25, 0.0) == ([1.0, 3.0], 0.0, 0.25, 0.0)
    assert check_opts(1, None, 1, 8, 0.5) == (None, 1.0, 8.0, 0.5)
    for kw, match in [(dict(m=0), "1..4 members"), (dict(m=5), "1..4 members"), (dict(alpha=1.5), "alpha"), (dict(alpha=True), "alpha"),
                      (dict(alpha=float("nan")), "alpha"), (dict(temperature=0.2), "temperature"), (dict(temperature=8.5), "temperature"),
                      (dict(temperature="1"), "temperature"), (dict(smoothing=1.0), "smoothing"), (dict(weights=[1.0]), "2 members"),
                      (dict(weights=[1.0, -1.0]), "finite real >= 0"), (dict(weights=[0, 0]), "sum to 0")]:
        args = dict(m=2, weights=None, alpha=0.5, temperature=1.0, smoothing=0.1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            check_opts(**args)


# ---- the Engine's refusals ---------------------------------------------------------------------------------------------------------
class _FakeEng:
    """enough of an Engine for the argument checks, which run before anything else is touched"""

    def __init__(self, V=10, device="cuda:0", ss=(False, 0.0)):
        self.caption_vocab = [None] * V
        self.device = device
        self.model = types.SimpleNamespace(scheduled_sampling=ss[0], ss_prob=ss[1])

    def __getattr__(self, name):
        raise AssertionError("the argument checks touched Engine.%s" % name)


@pytest.mark.parametrize("eng", ["BUTDDetection_Eng", "AoADetection_Eng", "NIC_Eng", "BUTDSpatial_Eng"])
def test_engine_refusals_come_before_any_device_work(eng, monkeypatch):
    from simpleimagecaptionzoo_amd import engine
    fn = getattr(engine, eng).distill_training_epoch
    crit = types.SimpleNamespace(smoothing=0.1)
    me = _FakeEng()
    two = lambda: [_FakeEng(), _FakeEng()]
    shared = _FakeEng()
    shared.model = me.model
    for student, teachers, kw, match in [
        (me, [], {}, "1..4 members"),
        (me, [_FakeEng() for _ in range(5)], {}, "1..4 members"),
        (me, two(), dict(alpha=1.5), "alpha"),
        (me, two(), dict(alpha=-0.1), "alpha"),
        (me, two(), dict(temperature=0.1), "temperature"),
        (me, two(), dict(temperature=16.0), "temperature"),
        (me, two(), dict(weights=[1.0]), "2 members"),
        (me, two(), dict(weights=[1.0, -2.0]), "finite real >= 0"),
        (me, two(), dict(weights=[0.0, 0.0]), "sum to 0"),
        (me, [_FakeEng(), me], {}, "the student is among its teachers"),
        (me, [shared], {}, "the student is among its teachers"),
        (me, [_FakeEng(10), _FakeEng(11)], {}, "vocabularies differ"),
        (_FakeEng(12), two(), {}, "vocabularies differ"),
        (me, [_FakeEng(device="cuda:1")], {}, "different devices"),
        (_FakeEng(ss=(True, 0.25)), two(), {}, "scheduled sampling is live on the student"),
        (me, [_FakeEng(ss=(True, 0.5))], {}, "scheduled sampling is live on a teacher"),
    ]:
        with pytest.raises(ValueError, match=match):
            fn(student, [], None, crit, teachers, tqdm_visible=False, **kw)
    with pytest.raises(ValueError, match="smoothing"):
        fn(me, [], None, types.SimpleNamespace(smoothing=1.0), two(), tqdm_visible=False)
    # the reference's default, ss_prob set on the captioner but not live (scheduled.py), is no obstacle: the checks pass and the epoch
    # goes on to the engine's stream

    class Reached(Exception):
        pass

    def on_stream(eng):
        raise Reached()
    monkeypatch.setattr(engine, "_on_stream", on_stream)
    with pytest.raises(Reached):
        fn(_FakeEng(ss=(False, 0.25)), [], None, crit, two(), tqdm_visible=False)


# ---- the oracle against itself -----------------------------------------------------------------------------------------------------
def test_case_list_covers_every_value_the_issue_names():
    cases = do.kernel_cases()
    assert len({do.case_id(c) for c in cases}) == len(cases) <= 30
    for V in do.VOCABS:
        mine = [c for c in cases if c["V"] == V]
        assert {(c["rows"], c["M"]) for c in mine} == {(r, m) for r in do.ROWS for m in (1, 2, 3, 4)}
        for key, vals in (("tau", do.TAUS), ("alpha", do.ALPHAS), ("sigma", do.SIGMAS), ("weights", do.WEIGHT_KINDS), ("ld_s", do.LD_KINDS),
                          ("ld_t", do.LD_KINDS), ("ld_out", do.LD_KINDS)):
            assert {c[key] for c in mine} == set(vals), (V, key)
        assert any(c["tau"] == 0.25 and c["rows"] == 5 for c in mine)
    for V in do.VOCABS:               # what the stride kinds mean for alignment
        assert do.stride_of("pad4", V) % 4 == 0 and do.stride_of("pad4", V) > V and do.stride_of("odd", V) % 2 == 1 and do.stride_of("tight", V) == V
    c = cases[-1]
    s, t, w, tg = do.case_inputs(c)
    assert tg[0] == 0 and tg[4] == c["V"] - 1 and (t[0][0].max() - np.sort(t[0][0])[-2]) > 70 and np.abs(t[0][2]).max() < 1e-2
    zero = next(c for c in cases if c["weights"] == "zero")
    s, t, w, tg = do.case_inputs(zero)
    assert w[1] == 0.0 and np.isnan(t[1]).all() and np.isfinite(do.terms(s, t, w, tg, 0.1, 0.5, 1.0, 1.0)[3]).all()


@pytest.mark.parametrize("tau", do.TAUS)
def test_oracle_q_sums_to_one_and_a_student_equal_to_its_teacher_has_no_soft_loss(tau):
    rs = np.random.RandomState(3)
    t = [rs.randn(4, 37) * 3, rs.randn(4, 37), rs.randn(4, 37) * 0.1]
    t[0][0, 5] += 80.0
    q = do.teacher_q(t, [0.2, 0.5, 0.3], tau)
    np.testing.assert_allclose(q.sum(1), 1.0, rtol=0, atol=1e-14)
    assert (q >= 0).all()
    tg = np.array([0, 36, 5, 7])
    loss, hard, kd, ds = do.terms(t[0], [t[0]], None, tg, 0.1, 1.0, tau, 4.0)
    assert abs(kd) < 1e-14 and np.abs(ds).max() < 1e-15 and abs(loss) < 1e-14 and hard > 0
    # alpha = 0: the label-smoothing loss of the project's oracle
    from oracle import butd as ob
    loss, hard, kd, ds = do.terms(t[1], [t[0]], None, tg, 0.1, 0.0, tau, 4.0)
    want = ob.label_smoothing_loss(torch.from_numpy(t[1]), torch.from_numpy(tg), 0.1)
    assert abs(loss - float(want)) < 1e-12 and abs(hard - float(want)) < 1e-12


@pytest.mark.parametrize("tau, alpha, sigma", [(0.25, 0.5, 0.1), (1.0, 1.0, 0.0), (2.0, 0.7, 0.1)])
def test_oracle_gradient_equals_central_differences_and_its_torch_twin(tau, alpha, sigma):
    rs = np.random.RandomState(int(tau * 100))
    s = rs.randn(3, 11)
    t = [rs.randn(3, 11) * 2, rs.randn(3, 11)]
    w, tg, n = [0.3, 0.7], np.array([0, 10, 4]), 3.0
    loss, hard, kd, ds = do.terms(s, t, w, tg, sigma, alpha, tau, n)
    eps = 1e-6
    for i in range(3):
        for v in range(11):
            d = np.zeros_like(s)
            d[i, v] = eps
            num = (do.terms(s + d, t, w, tg, sigma, alpha, tau, n)[0] - do.terms(s - d, t, w, tg, sigma, alpha, tau, n)[0]) / (2 * eps)
            assert abs(num - ds[i, v]) < 1e-8, (i, v, num, ds[i, v])
    x = torch.from_numpy(s).requires_grad_(True)
    tl, th, tk = do.loss_torch(x, t, w, tg, sigma, alpha, tau, n)
    tl.backward()
    assert abs(tl.item() - loss) < 1e-12 and abs(th.item() - hard) < 1e-12 and abs(tk.item() - kd) < 1e-12
    np.testing.assert_allclose(x.grad.numpy(), ds, rtol=0, atol=1e-13)


# ---- the dropout compensation behind the Engine test "a teacher equal to the student has no soft loss" -----------------------------
def _ones_like_masks(masks):
    return {k: np.ones_like(v, dtype=bool) for k, v in masks.items()}


def test_full_keep_training_forward_equals_the_compensated_evaluation_forward():
    """undo_full_keep_dropout: float64 oracles, small shapes, every family"""
    from oracle import butd as ob
    from oracle import nic as on
    import _aoa_refiner as ar
    from simpleimagecaptionzoo_amd.synth import random_butd_params, random_nic_params
    lengths = [4, 3, 1]
    # BUTD
    R, D, H, E, A, V = 5, 12, 8, 6, 7, 23
    p = {k: v.double() for k, v in random_butd_params(R, D, H, E, A, V, "cpu", seed=1).items()}
    caps = ar.captions_of((3, R, D, H, E, V), lengths, 2)
    feats = torch.relu(torch.randn(3, R, D, dtype=torch.float64))
    T = max(lengths)
    ones = (np.ones((T, 3, E), bool), np.ones((T, 3, R, A), bool), np.ones((T, 3, H), bool))
    q = ob.strip_prefix(do.undo_full_keep_dropout("butd", {"decoder." + k: v for k, v in p.items()}, (H, D, E)))
    with ar.oracle_dtype(8, torch.float64):                   # (the oracles' zero states take the default dtype)
        train = ob.forward_xe(feats, caps, lengths, p, *ones)
        plain = ob.forward_xe(feats, caps, lengths, p)
        comp = ob.forward_xe(feats, caps, lengths, q)
    assert float((train - plain).abs().max()) > 1e-2          # dropout that keeps everything still scales what it keeps
    assert float((train - comp).abs().max()) < 1e-12
    # NIC
    p = {k: v.double() for k, v in random_nic_params(E, H, V, "cpu", seed=2).items()}
    f = torch.randn(3, E, dtype=torch.float64)
    q = ob.strip_prefix(do.undo_full_keep_dropout("nic", {"decoder." + k: v for k, v in p.items()}, None))
    with ar.oracle_dtype(8, torch.float64):
        train = on.forward_xe(f, caps, lengths, p, np.ones((T, 3, H), bool))
        plain = on.forward_xe(f, caps, lengths, p)
        comp = on.forward_xe(f, caps, lengths, q)
    assert float((train - plain).abs().max()) > 1e-2
    assert float((train - comp).abs().max()) < 1e-12
    # AoA, fixed and per-image region counts
    for counts in (None, [5, 2, 4]):
        cfg = (3, 5, 12, 16, 6, 23, 4, T, counts, None)
        sd = {k: v.double() for k, v in ar.state_dict_of(cfg, 5).items()}
        feats = ar.feats_of(cfg, 6).double()
        masks = _ones_like_masks(ar.masks_of(cfg, 7)[0])
        with ar.oracle_dtype(cfg[6], torch.float64) as oa:
            train = oa.forward_xe(feats, caps, lengths, sd, masks, counts)
            plain = oa.forward_xe(feats, caps, lengths, sd, None, counts)
            comp = oa.forward_xe(feats, caps, lengths, do.undo_full_keep_dropout("aoa", sd, (16, 6)), None, counts)
        assert float((train - plain).abs().max()) > 1e-2
        assert float((train - comp).abs().max()) < 1e-11, counts
