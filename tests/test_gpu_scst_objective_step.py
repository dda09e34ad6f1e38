"""The kernels of the SCST objectives alone, through icz_test_scst_objective (include/icz.h "SCST objectives"): scst_risk_kernel +
scst_risk_sum_kernel, scst_entropy_dlogits_kernel, scst_finish_kernel and, where the objective asks for them, the REINFORCE kernels,
on the case table of tests/_scst_objective.py against its float64 statement, within its counted bounds.

Every tensor lies between guards; dead rows of the logits, their lse and the pad columns hold NaN (a dead row must come out as zeros
without being read); every output starts as a fill.  Every case runs twice and must repeat bit for bit."""
import numpy as np
import pytest
import torch

import _scst_objective as so

pytestmark = pytest.mark.gpu

PAD = 16
NAN = float("nan")
FILL = -12345.5
CANARY = -7777
_worst = {}


class Dev:
    """device copies of numpy arrays, each inside a buffer of `guard` with PAD guard elements on both sides"""

    def __init__(self):
        self.items = []

    def put(self, a, guard):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a).reshape(-1)
        buf = torch.full((PAD + t.numel() + PAD,), guard, dtype=t.dtype, device="cuda")
        buf[PAD:PAD + t.numel()] = t.cuda()
        self.items.append((buf, t.numel(), guard))
        return buf[PAD:PAD + t.numel()].view(a.shape)

    def check(self):
        for buf, n, guard in self.items:
            g = torch.cat([buf[:PAD], buf[PAD + n:]])
            ok = torch.isnan(g).all() if guard != guard else (g == guard).all()
            assert ok.item(), "a write outside a tensor"


def _close(got, ref, bound, what):
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.abs(got - ref)
    ok = (got == ref) | (err <= bound)
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    if frac.size:
        _worst[what[-1]] = max(_worst.get(what[-1], 0.0), float(np.nanmax(np.where(ok, frac, 0.0))))
        print("scst objective: %-28s %-10s worst error / bound %.3f" % (what[0], what[-1], float(np.nanmax(frac))))
    assert ok.all(), (what, "first at", np.argwhere(~ok)[0].tolist(), got[~ok][:4], ref[~ok][:4], np.broadcast_to(bound, got.shape)[~ok][:4])


def _objective(c, inp, d):
    from simpleimagecaptionzoo_amd.scst_objective import make_objective
    kw = {}
    if c.kind == 0:
        kw["reward"] = d.put(inp["reward"], NAN)
    else:
        kw["scores"] = d.put(inp["scores"], NAN)
    return make_objective("risk" if c.kind else "reinforce", c.K, c.a, c.b, n_img_global=c.n_glob, **kw)


def _put_inputs(c, inp, d):
    lg = d.put(inp["x"], NAN)
    assert lg.data_ptr() % 16 == 0 and lg.stride(0) == inp["ldl"]
    return (lg, d.put(inp["logp"], NAN), d.put(inp["seq"], CANARY), d.put(inp["draw"], CANARY), d.put(inp["lse"], NAN),
            None if not c.msum else d.put(np.array([c.msum], dtype=np.float32), NAN))


def _run(c, inp):
    from simpleimagecaptionzoo_amd._lib import check, lib, ptr, stream_ptr
    import ctypes as C
    B, T = inp["seq"].shape
    d = Dev()
    lg, logp, seq, draw, lse, msum = _put_inputs(c, inp, d)
    obj = _objective(c, inp, d)
    coef = d.put(np.full((B, T), FILL, dtype=np.float32), FILL)
    out3, ms = d.put(np.full(3, FILL, dtype=np.float32), FILL), d.put(np.full(1, FILL, dtype=np.float32), FILL)
    ent = d.put(np.full((B, T), FILL, dtype=np.float32), FILL)
    o, keep = obj.struct(lg.device, B, T)
    check(lib().icz_test_scst_objective(C.byref(o), ptr(logp), ptr(seq), B, T, ptr(msum), ptr(coef), ptr(out3), ptr(ent), ptr(ms), ptr(lg), c.V,
                                        inp["ldl"], ptr(draw), ptr(lse), inp["Bs"], c.row0, stream_ptr()))
    torch.cuda.synchronize()
    d.check()
    return {"g": lg.cpu().numpy(), "coef": coef.cpu().numpy(), "out3": out3.cpu().numpy(), "ms": ms.cpu().numpy(), "ent": ent.cpu().numpy()}


@pytest.mark.parametrize("c", so.CASES, ids=lambda c: c.name)
def test_objective_kernels_against_the_float64_statement(c):
    inp = so.inputs(c)
    ref = so.ref(c, inp)
    out = _run(c, inp)
    again = _run(c, inp)
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), (c.name, k, "two runs differ")
    assert float(out["ms"][0]) == ref["ms"], (c.name, "mask sum", out["ms"], ref["ms"])
    _close(out["coef"], ref["coef"], ref["coef_bound"], (c.name, "coef"))
    assert (out["coef"][ref["mask"] == 0] == 0).all()
    _close(out["out3"][1], ref["obj"], ref["obj_bound"], (c.name, "obj"))
    _close(out["out3"][2], ref["ent"], ref["ent_bound"], (c.name, "ent"))
    _close(out["out3"][0], ref["loss"], ref["loss_bound"], (c.name, "loss"))
    _close(out["ent"], ref["H"], ref["H_bound"], (c.name, "ent_out"))
    assert (out["ent"][ref["mask"] == 0] == 0).all()
    if c.b == 0:
        assert out["out3"][2] == 0 and not out["ent"].any() and out["out3"][0] == out["out3"][1]
    z = ref["zero_rows"]
    assert (out["g"][z] == 0).all() and (out["g"][:, c.V:] == 0).all(), (c.name, "dead rows / pad columns")
    _close(out["g"][~z, :c.V], ref["g"][~z], ref["g_bound"][~z], (c.name, "grad"))


@pytest.mark.parametrize("name", ["kind0_5img_k1_t4_b0", "merged_b0"])
def test_kind0_without_entropy_is_icz_test_reinforce_bit_for_bit(name):
    from simpleimagecaptionzoo_amd.token_choice import entry_reinforce
    c = so.CASE_BY_NAME[name]
    inp = so.inputs(c)
    out = _run(c, inp)
    B, T = inp["seq"].shape
    d = Dev()
    lg, logp, seq, draw, lse, msum = _put_inputs(c, inp, d)
    reward = d.put(inp["reward"], NAN)
    coef = d.put(np.full((B, T), FILL, dtype=np.float32), FILL)
    loss, ms = d.put(np.full(1, FILL, dtype=np.float32), FILL), d.put(np.full(1, FILL, dtype=np.float32), FILL)
    entry_reinforce(logp, seq, reward, B, T, msum, coef, loss, ms, lg, c.V, inp["ldl"], draw, lse, inp["Bs"], c.row0)
    torch.cuda.synchronize()
    d.check()
    assert out["g"].tobytes() == lg.cpu().numpy().tobytes() and out["coef"].tobytes() == coef.cpu().numpy().tobytes()
    assert out["out3"][0:1].tobytes() == loss.cpu().numpy().tobytes() and out["ms"].tobytes() == ms.cpu().numpy().tobytes()
    assert out["out3"][1:2].tobytes() == loss.cpu().numpy().tobytes() and out["out3"][2] == 0


def test_refusals_leave_every_output_alone():
    from simpleimagecaptionzoo_amd._lib import ScstObjective, lib, ptr, stream_ptr
    import ctypes as C
    c = so.CASE_BY_NAME["v53_1img_k2_t1"]
    inp = so.inputs(c)
    B, T = inp["seq"].shape
    d = Dev()
    lg, logp, seq, draw, lse, _ = _put_inputs(c, inp, d)
    scores = d.put(inp["scores"], NAN)
    coef = d.put(np.full((B, T), FILL, dtype=np.float32), FILL)
    out3 = d.put(np.full(3, FILL, dtype=np.float32), FILL)
    before = lg.clone()

    def call(o, V=c.V, ldl=inp["ldl"], Bs=0, row0=0, logits=lg):
        return lib().icz_test_scst_objective(C.byref(o), ptr(logp), ptr(seq), B, T, None, ptr(coef), ptr(out3), None, None, ptr(logits), V, ldl,
                                             ptr(draw), ptr(lse), Bs, row0, stream_ptr())
    good = dict(kind=1, K=2, risk_alpha=1.0, entropy_weight=0.5, n_img_global=0.0, reward=None, scores=scores.data_ptr())
    for kw in (dict(kind=2), dict(K=3), dict(risk_alpha=0.0), dict(entropy_weight=-1.0), dict(n_img_global=-2.0), dict(scores=None)):
        assert call(ScstObjective(**dict(good, **kw))) == -1, kw
    o = ScstObjective(**good)
    assert call(o, V=0) == -1 and call(o, ldl=52) == -1 and call(o, Bs=5, row0=2) == -1
    assert call(o, logits=lg.view(-1)[1:]) == -1          # 16-byte loads need aligned rows
    torch.cuda.synchronize()
    d.check()
    assert (coef == FILL).all() and (out3 == FILL).all() and before.view(torch.int32).equal(lg.view(torch.int32))


def test_zz_report_worst_error_fractions():
    """Last in the file: the largest error / bound per compared quantity over whatever ran above in this process (_close itself
    asserts every bound, so nothing here depends on which tests were selected)."""
    for k in sorted(_worst):
        print("scst objective: %-10s worst error / bound %.3f" % (k, _worst[k]))
    assert all(f <= 1.0 for f in _worst.values())
