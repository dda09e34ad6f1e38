"""The SCST objectives (include/icz.h "SCST objectives") without a GPU: the float64 statement of tests/_scst_objective.py against
torch.autograd and central differences, the zero sum of the risk coefficients, and every host-side refusal (make_objective,
icz_scst_objective_check in its documented order, the Engine)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scst_objective as so  # noqa: E402


def _f64_case(kind, n_img=2, K=3, T=4, V=11, a=1.0, b=0.25, row0=0, msum=0.0, n_glob=0.0, seed=0):
    """a small case with float64 inputs whose lse / logp are the exact ones of the logits (what autograd differentiates)"""
    c = types.SimpleNamespace(kind=kind, K=K, T=T, V=V, a=a, b=b, row0=row0, msum=msum, n_glob=n_glob)
    rs = np.random.RandomState(seed)
    B = n_img * K
    Bs = row0 + B if row0 else 0
    stride = Bs or B
    seq = rs.randint(1, V, size=(B, T)).astype(np.int64)
    seq[0, 0:] = 0                         # ends at step 1
    seq[1, 2:] = 0
    x = rs.randn(T * stride, V)
    draw = rs.randint(0, V, size=T * stride).astype(np.int32)
    if row0:
        draw.reshape(T, stride)[:, :row0] = -1
    inp = {"seq": seq, "x": x, "draw": draw, "Bs": Bs, "reward": rs.randn(B, 1) * np.ones((1, T)), "scores": rs.rand(B) * 3}
    _fill(inp, c)
    return c, inp


def _fill(inp, c):
    """lse and logp from the logits, in float64"""
    x, draw = inp["x"], inp["draw"]
    B, T = inp["seq"].shape
    stride = inp["Bs"] or B
    m = x.max(1)
    inp["lse"] = m + np.log(np.exp(x - m[:, None]).sum(1))
    lp = np.zeros((B, T))
    for t in range(T):
        for r in range(B):
            row = t * stride + c.row0 + r
            lp[r, t] = x[row, draw[row]] - inp["lse"][row]
    inp["logp"] = lp


def _torch_loss(c, inp, x):
    """the definitions of include/icz.h written with torch ops on the logits x (float64, requires_grad)"""
    seq = torch.from_numpy(inp["seq"])
    B, T = seq.shape
    stride = inp["Bs"] or B
    mask = torch.ones(B, T, dtype=torch.float64)
    mask[:, 1:] = (seq[:, :-1] > 0).double()
    M = c.msum if c.msum else mask.sum()
    lsm = torch.log_softmax(x, 1).view(T, stride, -1)[:, c.row0:c.row0 + B]              # [T, B, V]
    draw = torch.from_numpy(inp["draw"].astype(np.int64)).view(T, stride)[:, c.row0:c.row0 + B]
    logp = lsm.gather(2, draw.unsqueeze(2)).squeeze(2).t()                               # [B, T]
    H = -(lsm.exp() * lsm).sum(2).t()
    if c.kind == 0:
        obj = -(logp * torch.from_numpy(inp["reward"]) * mask).sum() / M
    else:
        N = c.n_glob if c.n_glob else B // c.K
        s = (logp * mask).sum(1).view(-1, c.K)
        Q = torch.softmax(c.a * s, 1)
        obj = (Q * -torch.from_numpy(inp["scores"]).view(-1, c.K)).sum() / N
    ent = (mask * H).sum() / M
    return obj - c.b * ent, obj, ent


CONFIGS = [dict(kind=0, b=0.0), dict(kind=0, b=0.25), dict(kind=0, b=0.25, row0=2, K=1, n_img=4), dict(kind=1, b=0.0), dict(kind=1, b=0.25, a=0.25),
           dict(kind=1, b=0.75, a=4.0, K=5, msum=37.0, n_glob=9.0), dict(kind=0, b=0.5, msum=50.0, K=1, n_img=5)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda d: "-".join("%s%s" % kv for kv in sorted(d.items())))
def test_statement_is_the_autograd_gradient(cfg):
    c, inp = _f64_case(**cfg)
    r = so.ref(c, inp)
    x = torch.from_numpy(inp["x"]).clone().requires_grad_(True)
    loss, obj, ent = _torch_loss(c, inp, x)
    loss.backward()
    assert abs(loss.item() - r["loss"]) < 1e-12 and abs(obj.item() - r["obj"]) < 1e-12
    assert abs(ent.item() - r["ent"]) < 1e-12 if c.b > 0 else r["ent"] == 0.0         # b = 0: no row is read for H, ent is reported as 0
    np.testing.assert_allclose(r["g"], x.grad.numpy(), rtol=0, atol=1e-12)
    stride = inp["Bs"] or inp["seq"].shape[0]
    dead = r["zero_rows"]
    assert dead.reshape(c.T, stride)[:, :c.row0].all() and not np.abs(r["g"][dead]).any()


@pytest.mark.parametrize("cfg", CONFIGS[1:], ids=lambda d: "-".join("%s%s" % kv for kv in sorted(d.items())))
def test_statement_against_central_differences(cfg):
    c, inp = _f64_case(seed=3, **cfg)
    r = so.ref(c, inp)
    rs = np.random.RandomState(5)
    live = np.flatnonzero(~r["zero_rows"])
    eps = 1e-6
    for _ in range(12):
        row, v = int(rs.choice(live)), int(rs.randint(0, c.V))
        vals = []
        for sgn in (1.0, -1.0):
            q = dict(inp)
            q["x"] = inp["x"].copy()
            q["x"][row, v] += sgn * eps
            _fill(q, c)
            vals.append(so.loss_of(c, q))
        assert abs((vals[0] - vals[1]) / (2 * eps) - r["g"][row, v]) < 1e-8


@pytest.mark.parametrize("name", [c.name for c in so.CASES if c.kind == 1])
def test_risk_coefficients_of_an_image_sum_to_zero_under_a_step_mask(name):
    """d obj / d s sums to 0 over the K rows of an image (Q is a distribution): with every row's mask on at a step, so does coef"""
    c = so.CASE_BY_NAME[name]
    inp = so.inputs(c)
    inp["seq"][:] = 5                      # every step on
    mask = np.ones_like(inp["logp"], dtype=np.float64)
    N = float(c.n_glob or c.n_img)
    _, coef, _, _, L, Q = so.risk_terms(inp["logp"], mask, inp["scores"], c.K, c.a, N)
    per_img = coef.reshape(c.n_img, c.K, c.T)
    # the statement's own float64 rounding: each Q_k carries at most 2 K + 8 roundings, c_k - L one, the products three
    scale = c.a / N * (Q.reshape(c.n_img, c.K) * (np.abs(inp["scores"]).reshape(c.n_img, c.K) + np.abs(L)[:, None])).sum(1)
    assert (np.abs(per_img.sum(1)) <= ((2 * c.K + 12) * so.U64 * scale)[:, None] + 1e-300).all()
    assert np.abs(per_img).max() > 0 or c.design == "equal"


def test_case_table_covers_what_the_kernels_can_get_wrong():
    cs = so.CASES
    assert {53, 1000, 10102, 40003} <= {c.V for c in cs} and so.pad_vocab(53) == 64 and so.pad_vocab(10102) == 10112
    assert {(1, 2, 1), (3, 5, 5), (2, 8, 7)} <= {(c.n_img, c.K, c.T) for c in cs if c.kind == 1}
    assert any((c.n_img, c.K, c.T) == (5, 1, 4) and c.kind == 0 for c in cs)
    assert any(c.n_img * c.K * c.T > 256 for c in cs) and any(c.row0 > 0 for c in cs)
    assert {0.25, 1.0, 4.0} <= {c.a for c in cs if c.kind == 1} and {0.0, 0.01, 0.5} <= {c.b for c in cs if c.kind == 0}
    assert any(c.msum and c.n_glob for c in cs) and any(c.msum and not c.n_glob for c in cs) and any(c.n_glob and not c.msum for c in cs)
    for c in cs:
        inp = so.inputs(c)
        r = so.ref(c, inp)
        on = r["mask"].sum(1)
        assert on.min() == 1 and on.max() == c.T                       # a row that ends at step 1, one that never ends
        assert np.isfinite(r["g"]).all() and np.isfinite(r["g_bound"]).all() and np.isfinite(r["loss"])
        if c.design == "s300":
            s = (inp["logp"] * r["mask"]).sum(1).reshape(c.n_img, c.K)
            assert (s.max(1) - s.min(1) > 250).all()
        if c.design == "equal":
            assert np.abs(r["coef"]).max() < 1e-15                     # equal costs: nothing to prefer
        if c.b > 0 and c.T * c.n_img * c.K >= 10:
            h = r["H"][r["mask"] > 0]
            assert h.min() < 1e-3 and h.max() > 0.99 * np.log(c.V)     # a peaked row and a near-uniform one


# ---- make_objective ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(kind="margin"), dict(kind=1), dict(K=0), dict(K=9), dict(K=True), dict(K=2.0), dict(kind="risk", K=1),
                                dict(risk_alpha=0.0), dict(risk_alpha=-1.0), dict(risk_alpha=float("inf")), dict(risk_alpha=float("nan")),
                                dict(risk_alpha="1"), dict(entropy_weight=-0.1), dict(entropy_weight=float("nan")), dict(entropy_weight=True),
                                dict(n_img_global=-1.0), dict(n_img_global=float("inf")), dict(reward=[1.0]), dict(scores=3)])
def test_make_objective_refuses(kw):
    from simpleimagecaptionzoo_amd.scst_objective import make_objective
    with pytest.raises(ValueError):
        make_objective(**kw)


def test_make_objective_keeps_its_arguments():
    from simpleimagecaptionzoo_amd.scst_objective import make_objective
    o = make_objective("risk", 5, 0.25, 0.01)
    assert (o.kind, o.K, o.risk_alpha, o.entropy_weight, o.n_img_global) == ("risk", 5, 0.25, 0.01, 0.0)
    s = torch.zeros(10, dtype=torch.float64)
    o2 = o.with_data(scores=s, n_img_global=4.0)
    assert o2.scores is s and o2.n_img_global == 4.0 and o.scores is None
    assert make_objective().kind == "reinforce" and make_objective().K == 1


# ---- icz_scst_objective_check -----------------------------------------------------------------------------
def _check(rows=10, T=4, null=False, **kw):
    from simpleimagecaptionzoo_amd._lib import ScstObjective, lib
    L = lib()
    keep = C.create_string_buffer(64)
    f = dict(kind=1, K=5, risk_alpha=1.0, entropy_weight=0.0, n_img_global=0.0, reward=C.addressof(keep), scores=C.addressof(keep))
    f.update(kw)
    o = ScstObjective(**f)
    st = L.icz_scst_objective_check(None if null else C.byref(o), rows, T)
    return st, L.icz_last_error().decode()


def test_objective_check_accepts_and_refuses_in_the_documented_order():
    nan, inf = float("nan"), float("inf")
    assert _check()[0] == 0 and _check(kind=0, K=1, scores=None)[0] == 0 and _check(reward=None)[0] == 0
    assert _check(kind=0, K=3, rows=9, scores=None)[0] == 0
    # every later rule is broken as well: the message names the first one
    bad = dict(kind=7, K=0, risk_alpha=nan, entropy_weight=-1.0, n_img_global=-1.0, reward=None, scores=None)
    order = [("kind", "kind="), ("K", "K=0"), ("risk_alpha", "risk_alpha"), ("entropy_weight", "entropy_weight"), ("n_img_global", "n_img_global"),
             ("scores", "scores")]
    st, msg = _check(null=True)
    assert st == -1 and "null objective" in msg
    for i, (field, word) in enumerate(order):
        kw = {k: bad[k] for k, _ in order[i:] if k != "scores"}
        kw["scores"] = None
        if field != "kind":
            kw.pop("kind", None)
        st, msg = _check(**kw)
        assert st == -1 and word in msg, (field, msg)
    for kw, word in ((dict(K=1), "K=1"), (dict(K=9), "K=9"), (dict(kind=0, K=9), "K=9"), (dict(rows=11), "multiple"), (dict(rows=0), "multiple"),
                     (dict(T=0), "multiple"), (dict(risk_alpha=0.0), "risk_alpha"), (dict(risk_alpha=inf), "risk_alpha"),
                     (dict(kind=0, K=1, risk_alpha=-1.0), "risk_alpha"), (dict(entropy_weight=inf), "entropy_weight"),
                     (dict(n_img_global=nan), "n_img_global"), (dict(kind=0, K=1, reward=None), "reward"), (dict(scores=None), "scores")):
        st, msg = _check(**kw)
        assert st == -1 and word in msg, (kw, msg)


def test_every_family_binds_the_new_entry():
    from simpleimagecaptionzoo_amd._lib import lib
    from simpleimagecaptionzoo_amd.aoa import AoaHandle
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.nic import NicHandle
    for cls in (ButdHandle, AoaHandle, NicHandle):
        assert cls._entries().sample_backward_objective is getattr(lib(), "icz_%s_sample_backward_objective" % cls.family)


def test_entries_refuse_a_bad_objective_and_null_arguments_before_the_handle():
    from simpleimagecaptionzoo_amd._lib import ScstObjective, lib
    L = lib()
    keep = C.create_string_buffer(64)
    good = ScstObjective(1, 5, 1.0, 0.0, 0.0, None, C.addressof(keep))
    bad = ScstObjective(1, 5, 1.0, -1.0, 0.0, None, C.addressof(keep))
    for fam, extra in (("butd", ()), ("aoa", ()), ("nic", (None,))):
        fn = getattr(L, "icz_%s_sample_backward_objective" % fam)
        assert fn(None, C.byref(bad), None, *extra, None, None, None, 0.0, None) == -1 and "entropy_weight" in L.icz_last_error().decode()
        assert fn(None, C.byref(good), None, *extra, None, None, None, 0.0, None) == -1 and "null argument" in L.icz_last_error().decode()


# ---- Engine -----------------------------------------------------------------------------------------------
def test_engine_signatures():
    """the new method takes SCST_multisample_training_epoch's arguments in front; that method is left as it was"""
    import inspect
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, BUTDDetection_Eng, Engine, NIC_Eng
    old = str(inspect.signature(Engine.SCST_multisample_training_epoch))
    assert old == "(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, samples_per_image=5)"
    assert str(inspect.signature(Engine.SCST_objective_training_epoch)) == old[:-1] + ", objective='loo', risk_alpha=1.0, entropy_weight=0.0)"
    for cls in (BUTDDetection_Eng, AoADetection_Eng, NIC_Eng):
        assert cls.SCST_objective_training_epoch is Engine.SCST_objective_training_epoch
        assert list(inspect.signature(cls.SCST_training_epoch).parameters)[-2:] == ["samples_per_image", "entropy_weight"]


@pytest.mark.parametrize("kw,word", [(dict(objective="mrt"), "objective"), (dict(objective=None), "objective"), (dict(objective="risk", risk_alpha=0.0), "risk_alpha"),
                                     (dict(objective="risk", risk_alpha=float("nan")), "risk_alpha"), (dict(entropy_weight=-0.5), "entropy_weight"),
                                     (dict(entropy_weight=float("inf")), "entropy_weight"), (dict(entropy_weight="0.1"), "entropy_weight"),
                                     (dict(samples_per_image=9, objective="risk"), "samples_per_image")])
def test_engine_refuses_bad_objective_arguments_before_anything_is_touched(kw, word):
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, BUTDDetection_Eng, NIC_Eng
    for cls in (BUTDDetection_Eng, AoADetection_Eng, NIC_Eng):
        fake = cls.__new__(cls)            # no constructor: the checks come before the model, the stream or the loader is looked at
        with pytest.raises(ValueError, match=word):
            cls.SCST_objective_training_epoch(fake, [], None, None, **kw)


@pytest.mark.parametrize("w", [-1.0, float("nan"), float("inf"), True, "x"])
def test_single_sample_epoch_refuses_a_bad_entropy_weight(w):
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, BUTDDetection_Eng, NIC_Eng
    for cls in (BUTDDetection_Eng, AoADetection_Eng, NIC_Eng):
        with pytest.raises(ValueError, match="entropy_weight"):
            cls.SCST_training_epoch(cls.__new__(cls), [], None, None, entropy_weight=w)
    with pytest.raises(ValueError, match="entropy_weight"):
        BUTDDetection_Eng.SCST_training_epoch(BUTDDetection_Eng.__new__(BUTDDetection_Eng), [], None, None, samples_per_image=4, entropy_weight=w)
