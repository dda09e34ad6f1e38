"""SCST on without-replacement samples, host side (simpleimagecaptionzoo_amd/swor.py, Engine.SCST_distinct_training_epoch): the float64
statement of tests/_swor_oracle.py against torch.autograd of the surrogate with detached c, the unbiasedness of "unbiased" and the bias
order of the two normalised forms on a toy categorical, the two log q branches where they meet, make_batch, and every host-side refusal
(check_args, icz_swor_check in its documented order, the entries in front of their handle, the Engine)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import _swor_oracle as so


# ---- the statement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v53_n3_1img_t1", "v1000_n5_3img_t7_unbiased", "v53_n8_7img_t7_big", "zero_coef_image_n5_3img"])
def test_statement_equals_autograd_of_the_surrogate_with_detached_c(name):
    c = so.CASE_BY_NAME[name]
    inp = so.inputs(c)
    want = so.ref(c, inp)
    V, B, T = c.V, len(inp["lengths"]), max(inp["lengths"])
    x = torch.from_numpy(np.nan_to_num(inp["x"][:, :V].astype(np.float64))).requires_grad_(True)
    coef = torch.from_numpy(want["coef"])                                  # detached: a constant of the backward pass
    lp = torch.log_softmax(x, 1)
    loss = 0.0
    for b in range(B):
        for t in range(inp["lengths"][b]):
            loss = loss + coef[int(inp["perm"][b])] * lp[t * B + b, int(inp["caps"][b, t + 1])]
    g, = torch.autograd.grad(loss, x)
    g = g.numpy()
    assert abs(float(loss.detach()) - want["loss"]) <= 1e-12 * max(1.0, abs(want["loss"]))
    # rows the statement says are never read hold 0 there and in autograd alike (a coefficient of 0, or an inactive (b, t))
    assert np.abs(g - want["g"]).max() <= 1e-12 * max(1.0, np.abs(want["g"]).max())
    assert not g[~want["read"]].any() and T == c.T


def test_threshold_slot_has_no_coefficient_and_n_img_global_scales():
    c = so.CASE_BY_NAME["v1000_n5_3img_t7"]
    inp = so.inputs(c)
    one, _, _ = so.coefs(inp["phi"], inp["G"], inp["scores"], c.n, "normalised", 3.0)
    two, _, _ = so.coefs(inp["phi"], inp["G"], inp["scores"], c.n, "normalised", 6.0)
    assert not one[c.n - 1::c.n].any() and np.array_equal(one, two * 2)


@pytest.mark.parametrize("n", [4, 6])
def test_unbiased_form_is_unbiased_on_a_toy_categorical(n):
    """V = 6: the mean "unbiased" gradient over 4e5 Gumbel top-n draws equals the exact gradient of E[f] within 5 standard errors"""
    rs = np.random.RandomState(100 + n)
    theta = np.array([1.2, 0.3, -0.5, 0.9, -1.4, 0.1])
    f = np.array([0.2, 1.7, 0.9, 0.1, 2.5, 1.1])
    est = so.toy_gradients(theta, f, n, 400000, rs, "unbiased")
    mean, se = est.mean(0), est.std(0, ddof=1) / np.sqrt(est.shape[0])
    exact = so.toy_exact(theta, f)
    print("n=%d  mean %s\n      exact %s\n      |diff| / se %s" % (n, mean, exact, np.abs(mean - exact) / se))
    assert (np.abs(mean - exact) <= 5 * se).all()


@pytest.mark.parametrize("n", [3, 4])
def test_normalised_form_is_less_biased_than_the_form_without_its_correction(n):
    theta = np.array([1.2, 0.3, -0.5, 0.9, -1.4, 0.1])
    f = np.array([0.2, 1.7, 0.9, 0.1, 2.5, 1.1])
    exact = so.toy_exact(theta, f)
    bias = {}
    for form in ("normalised", "plain"):
        est = so.toy_gradients(theta, f, n, 400000, np.random.RandomState(7), form)          # the same draws for both forms
        bias[form] = np.abs(est.mean(0) - exact).max()
        se = (est.std(0, ddof=1) / np.sqrt(est.shape[0])).max()
        print("n=%d %-10s largest coordinate bias %.4f (largest standard error %.4f)" % (n, form, bias[form], se))
    assert bias["normalised"] < bias["plain"]


def test_log_q_branches_agree_where_they_meet():
    """at the switch point the series differs from log(-expm1(-exp(d))) by its first dropped term x^2 / 24 (< 1e-17) and rounding"""
    d = so.D_SWITCH + np.linspace(-1e-3, 1e-3, 21)
    taken, series, direct = so.log_q(d)
    x = np.exp(d)
    assert np.abs(series - direct).max() <= (x * x / 24).max() + 4 * so.U64 * np.abs(d).max()
    assert np.array_equal(taken, np.where(d < so.D_SWITCH, series, direct))
    # far below, expm1's own answer still agrees: the switch is a matter of the series' cost, not of a loss of digits
    lo = np.array([-60.0, -40.0, -25.0])
    assert np.abs(so.log_q(lo)[1] - so.log_q(lo)[2]).max() <= 4 * so.U64 * 60
    # q -> 1: log q = -exp(-x) to first order, then exactly 0
    hi = np.array([3.0, 10.0])
    assert np.allclose(so.log_q(hi)[0], -np.exp(-np.exp(hi)), rtol=1e-6, atol=0) and so.log_q(np.array([10.0]))[0][0] == 0.0


def test_equal_scores_give_a_zero_normalised_coefficient():
    rs = np.random.RandomState(3)
    n, n_img = 5, 4
    phi = (-rs.rand(n * n_img) * 12).astype(np.float32)
    G = np.sort(rs.randn(n_img, n) * 3, axis=1)[:, ::-1].reshape(-1).copy()
    f = np.repeat(rs.rand(n_img) * 3, n)
    coef, _, _ = so.coefs(phi, G, f, n, "normalised", float(n_img))
    assert np.abs(coef).max() <= 8 * so.U64 * 3          # Bu / W is f up to the rounding of m products and sums
    exact = np.repeat(2.0 ** rs.randint(-2, 3, size=n_img), n)
    assert not so.coefs(phi, G, exact, n, "normalised", float(n_img))[0].any()      # powers of two: to the bit
    assert so.coefs(phi, G, exact, n, "unbiased", float(n_img))[0].any()


# ---- make_batch -------------------------------------------------------------------------------------------------------------------
def test_make_batch_ties_unfinished_rows_and_a_sampled_zero():
    from simpleimagecaptionzoo_amd.swor import make_batch
    n, T, sta = 3, 5, 1
    # image 0: slots (len 3 with a sampled 0 inside, len 5 unfinished: no <end>, threshold); image 1: (len 3, len 3: a tie, threshold)
    ids = torch.tensor([[7, 0, 2, 0, 0], [4, 5, 6, 7, 8], [9, 2, 0, 0, 0],
                        [5, 5, 2, 0, 0], [6, 6, 2, 0, 0], [3, 3, 3, 2, 0]], dtype=torch.int64)
    lens = torch.tensor([3, 5, 2, 3, 3, 4], dtype=torch.int32)
    b = make_batch(ids, lens, sta, n)
    assert b.perm.tolist() == [1, 0, 3, 4] and b.perm.dtype == torch.int32         # stable: the ties keep their slot order
    assert b.lengths == [5, 3, 3, 3]
    assert b.captions.tolist() == [[1, 4, 5, 6, 7, 8], [1, 7, 0, 2, 0, 0], [1, 5, 5, 2, 0, 0], [1, 6, 6, 2, 0, 0]]
    assert b.rows_of_image.tolist() == [[1, 0], [2, 3]]
    assert b.captions.dtype == torch.int64 and tuple(b) == (b.captions, b.lengths, b.perm, b.rows_of_image)
    assert so.sorted_rows([3, 5, 3, 3], [0, 1, 3, 4]) == b.perm.tolist()            # the oracle's sort is this one


def test_make_batch_refuses():
    from simpleimagecaptionzoo_amd.swor import make_batch
    ids = torch.ones(6, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="image 1 has an empty slot"):
        make_batch(ids, torch.tensor([2, 2, 2, 2, 2, 0], dtype=torch.int32), 1, 3)
    with pytest.raises(ValueError, match="not images x n"):
        make_batch(ids, torch.tensor([2] * 6, dtype=torch.int32), 1, 4)
    with pytest.raises(ValueError, match="not images x n"):
        make_batch(ids, torch.tensor([2] * 5, dtype=torch.int32), 1, 3)
    with pytest.raises(ValueError, match="length of 5"):
        make_batch(ids, torch.tensor([2, 2, 5, 2, 2, 2], dtype=torch.int32), 1, 3)
    for n in (2, 9, True, 3.0, "5"):
        with pytest.raises(ValueError, match="slots per image"):
            make_batch(ids, torch.tensor([2] * 6, dtype=torch.int32), 1, n)


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_check_args_refuses_in_order():
    from simpleimagecaptionzoo_amd.swor import check_args
    assert check_args() == (5, 0, 0.0) and check_args(3, "unbiased", 7) == (3, 1, 7.0)
    with pytest.raises(ValueError, match="slots per image"):
        check_args(2, "mean", -1.0)
    with pytest.raises(ValueError, match="estimator"):
        check_args(8, "mean", -1.0)
    for g in (-1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="n_img_global"):
            check_args(8, "normalised", g)
    for e in (None, 0, "Normalised"):
        with pytest.raises(ValueError, match="estimator"):
            check_args(5, e)


def _check(rows=8, null=False, perm_host=None, lengths=None, **kw):
    from simpleimagecaptionzoo_amd._lib import SworOpts, lib
    L = lib()
    keep = C.create_string_buffer(64)
    a = C.addressof(keep)
    f = dict(n=5, estimator=0, n_img_global=0.0, phi=a, G=a, scores=a, perm=a, stats_out=None)
    f.update(kw)
    o = SworOpts(**f)
    arr = lambda v: None if v is None else (C.c_int32 * len(v))(*v)
    st = L.icz_swor_check(None if null else C.byref(o), rows, arr(perm_host), arr(lengths))
    return st, L.icz_last_error().decode()


def test_swor_check_accepts_and_refuses_in_the_documented_order():
    nan = float("nan")
    assert _check()[0] == 0 and _check(n=3, rows=2)[0] == 0 and _check(n=8, rows=7, estimator=1, n_img_global=3.0)[0] == 0
    assert _check(perm_host=[0, 1, 2, 3, 5, 6, 7, 8], lengths=[4, 4, 3, 3, 2, 1, 1, 1])[0] == 0
    st, msg = _check(null=True)
    assert st == -1 and "null options" in msg
    # every later rule is broken as well: the message names the first one
    bad = [("n", 9, "n=9"), ("estimator", 2, "estimator=2"), ("n_img_global", nan, "n_img_global"), ("rows", 7, "multiple"), ("phi", None, "null phi")]
    for i, (_, _, word) in enumerate(bad):
        kw = {k: v for k, v, _ in bad[i:]}
        if "n" not in kw:
            kw["n"] = 5
        st, msg = _check(**kw)
        assert st == -1 and word in msg, (kw, msg)
    for kw, word in ((dict(n=2), "n=2"), (dict(estimator=-1), "estimator=-1"), (dict(n_img_global=-1.0), "n_img_global"),
                     (dict(n_img_global=float("inf")), "n_img_global"), (dict(rows=0), "multiple"), (dict(rows=9), "multiple"),
                     (dict(G=None), "null phi"), (dict(scores=None), "null phi"), (dict(perm=None), "null phi"),
                     (dict(perm_host=[0, 1, 2, 3, 5, 6, 7, 10]), "perm[7]=10"), (dict(perm_host=[0, 1, 2, 4, 5, 6, 7, 8]), "perm[3]=4"),
                     (dict(perm_host=[0, 1, 2, 3, 5, 6, 7, 7]), "perm[7]=7"), (dict(perm_host=[-1, 1, 2, 3, 5, 6, 7, 8]), "perm[0]=-1"),
                     (dict(lengths=[4, 4, 3, 3, 2, 1, 1, 0]), "lengths[7]=0"), (dict(lengths=[4, 4, 3, 3, 2, 1, 1, 2]), "lengths[7]=2"),
                     (dict(perm_host=[0, 1, 2, 3, 5, 6, 7, 9], lengths=[0] * 8), "perm[7]=9")):
        st, msg = _check(**kw)
        assert st == -1 and word in msg, (kw, msg)


def test_every_family_binds_the_new_entry_and_refuses_before_its_handle():
    from simpleimagecaptionzoo_amd._lib import SworOpts, lib
    from simpleimagecaptionzoo_amd.aoa import AoaHandle
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.nic import NicHandle
    L = lib()
    keep = C.create_string_buffer(64)
    a = C.addressof(keep)
    good, bad = SworOpts(5, 0, 0.0, a, a, a, a, None), SworOpts(5, 3, 0.0, a, a, a, a, None)
    for cls, extra in ((ButdHandle, ()), (AoaHandle, ()), (NicHandle, (None,))):
        fn = getattr(L, "icz_%s_xe_backward_swor" % cls.family)
        assert cls._entries().xe_backward_swor is fn
        assert fn(None, C.byref(bad), 8, None, *extra, None, None) == -1 and "estimator=3" in L.icz_last_error().decode()
        assert fn(None, C.byref(good), 9, None, *extra, None, None) == -1 and "multiple" in L.icz_last_error().decode()
        assert fn(None, C.byref(good), 8, None, *extra, None, None) == -1 and "null grads or loss" in L.icz_last_error().decode()
        out = C.create_string_buffer(64)
        assert fn(None, C.byref(good), 8, C.byref(cls._Params()), *extra, C.cast(out, C.c_void_p), None) == -1
        assert "null handle" in L.icz_last_error().decode()
    assert L.icz_test_swor_objective(C.byref(bad), None, 53, 64, None, 8, 8, 7, None, None, None, None, None) == -1
    assert "estimator=3" in L.icz_last_error().decode()
    assert L.icz_test_swor_objective(C.byref(good), None, 53, 64, None, 8, 8, 7, None, None, None, None, None) == -1
    assert "null argument" in L.icz_last_error().decode()


# ---- Engine -----------------------------------------------------------------------------------------------------------------------
def test_engine_signature_on_every_engine():
    import inspect
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, BUTDDetection_Eng, BUTDSpatial_Eng, Engine, NIC_Eng
    assert str(inspect.signature(Engine.SCST_distinct_training_epoch)) == \
        "(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, samples_per_image=5, estimator='normalised')"
    for cls in (BUTDDetection_Eng, AoADetection_Eng, NIC_Eng, BUTDSpatial_Eng):
        assert cls.SCST_distinct_training_epoch is Engine.SCST_distinct_training_epoch


@pytest.mark.parametrize("kw,word", [(dict(samples_per_image=2), "slots per image"), (dict(samples_per_image=9), "slots per image"),
                                     (dict(samples_per_image=True), "slots per image"), (dict(samples_per_image=4.0), "slots per image"),
                                     (dict(estimator="loo"), "estimator"), (dict(estimator=None), "estimator")])
def test_engine_refuses_bad_arguments_before_anything_is_touched(kw, word):
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, BUTDDetection_Eng, NIC_Eng
    for cls in (BUTDDetection_Eng, AoADetection_Eng, NIC_Eng):
        fake = cls.__new__(cls)            # no constructor: the checks come before the model, the stream or the loader is looked at
        with pytest.raises(ValueError, match=word):
            cls.SCST_distinct_training_epoch(fake, [], None, None, **kw)


def test_engine_refuses_live_scheduled_sampling_a_full_handle_and_region_counts():
    from simpleimagecaptionzoo_amd.engine import BUTDDetection_Eng, _check_distinct_batch
    fake = BUTDDetection_Eng.__new__(BUTDDetection_Eng)
    fake.model = types.SimpleNamespace(scheduled_sampling=True, ss_prob=0.25)      # no stream, no scorer: they are never reached
    with pytest.raises(ValueError, match="scheduled sampling is live"):
        BUTDDetection_Eng.SCST_distinct_training_epoch(fake, [], None, None)
    feats = {"bu_feats": torch.zeros(4, 36, 8)}
    _check_distinct_batch(4, 5, 20, feats)
    with pytest.raises(ValueError, match="4 images x 5 slots exceed the handle's row capacity 19"):
        _check_distinct_batch(4, 5, 19, feats)
    with pytest.raises(ValueError, match="per-image region counts"):
        _check_distinct_batch(4, 5, 20, dict(feats, bu_counts=[36, 20, 36, 36]))
    with pytest.raises(ValueError, match="per-image region counts"):
        _check_distinct_batch(2, 5, 20, [{"bu_feat": np.zeros((36, 8))}, {"bu_feat": np.zeros((20, 8))}])
    _check_distinct_batch(2, 5, 20, [{"bu_feat": np.zeros((36, 8))}, {"bu_feat": np.zeros((36, 8))}])


def test_swor_forward_refuses_a_region_batch():
    from simpleimagecaptionzoo_amd.regions import RegionBatch
    from simpleimagecaptionzoo_amd.swor import make_batch, swor_forward
    b = make_batch(torch.ones(3, 4, dtype=torch.int64), torch.tensor([2, 2, 2], dtype=torch.int32), 1, 3)
    with pytest.raises(ValueError, match="region counts"):
        swor_forward(None, RegionBatch(torch.zeros(1, 36, 8), [20]), b)
