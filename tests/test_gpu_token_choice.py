"""The kernels that turn a row of logits into a token, a log-probability or a gradient, each on given logits through icz_test_greedy_select,
icz_test_sample_select, icz_test_ss_select, icz_test_xe_loss and icz_test_reinforce (include/icz.h) against the
float64 reference of tests/_token_choice.py.  The cases and what each is there for: tests/_token_choice.py; tests/test_cpu_token_choice.py
holds them to it, the margin condition included -- no row here is excused.

Tokens, draws, flags, counters, ids, embeddings and the stored finished logits are compared exactly; logp, lse, losses and gradients
within the counted bounds of tests/_token_choice.py (0 for an exact row: bits).  Every tensor lies between guards; pad columns, the gaps
between slabs and rows a kernel must not read are NaN; every slot a kernel has no business writing holds a fill that must survive.
Every case runs twice and must repeat bit for bit."""
import numpy as np
import pytest
import torch

import _token_choice as S

pytestmark = pytest.mark.gpu

PAD = 16
NAN = float("nan")
G8 = 0xAA                # guard and fill of uint8 buffers
_worst = {}              # what -> largest error / bound seen


class Dev:
    """device copies of numpy arrays, each inside a buffer of `guard` with PAD guard elements on both sides"""

    def __init__(self):
        self.items = []

    def put(self, a, guard, off=0):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a).reshape(-1)
        buf = torch.full((PAD + off + t.numel() + PAD,), guard, dtype=t.dtype, device="cuda")
        buf[PAD + off:PAD + off + t.numel()] = t.cuda()
        self.items.append((buf, PAD + off, t.numel(), guard))
        v = buf[PAD + off:PAD + off + t.numel()].view(a.shape)
        assert (v.data_ptr() % 16 == 0) == ((off * t.element_size()) % 16 == 0)
        return v

    def check(self):
        for buf, at, n, guard in self.items:
            g = torch.cat([buf[:at], buf[at + n:]])
            ok = torch.isnan(g).all() if guard != guard else (g == guard).all()
            assert ok.item(), "a write outside a tensor"


def _close(got, ref, bound, what):
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    err = np.abs(got - ref)
    ok = (got == ref) | (err <= bound)
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    if frac.size:
        _worst[what[-1]] = max(_worst.get(what[-1], 0.0), float(np.nanmax(np.where(ok, frac, 0.0))))
    assert ok.all(), (what, "first at", np.argwhere(~ok)[0].tolist(), got[~ok][:4], ref[~ok][:4], np.broadcast_to(bound, got.shape)[~ok][:4])


def _exact(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and (got == ref).all(), (what, "first at", np.argwhere(got != ref)[:1].tolist(), got[got != ref][:6],
                                                          ref[got != ref][:6])


def _bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    same = got.view(np.uint32) == ref.view(np.uint32)
    assert same.all(), (what, "first at", np.argwhere(~same)[:1].tolist(), got[~same][:4], ref[~same][:4])


def _column(a, t, fill, what):
    """column t of a [rows, T] output; every other column must still hold its fill"""
    rest = np.delete(a, t, axis=1)
    assert (rest == fill).all(), (what, "a column that is not the step's was written")
    return a[:, t]


def _same_twice(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, "two runs differ")


# =====================================================================================================================
# greedy choice
G_T = 3


def _run_greedy(c, inp, route, t=1, unf_in=None, nunf_in=None):
    from simpleimagecaptionzoo_amd.token_choice import entry_greedy_select
    lay, rows = S.LAYOUTS[c.layout], len(c.specs)
    ldl, stride = S.geometry(lay, c.V, rows, c.ns)
    d = Dev()
    lg = d.put(S.place(inp["slabs"], lay, ldl, stride), NAN, off=lay.off)
    bias = d.put(inp["bias"], NAN, off=lay.bias_off) if c.bias else None
    table = d.put(inp["table"], NAN)
    ids = d.put(np.full((rows, G_T), S.CANARY, dtype=np.int64), S.CANARY)
    it = d.put(np.full(rows, S.CANARY, dtype=np.int64), S.CANARY)
    emb = d.put(np.full((rows, c.E), S.FILL, dtype=np.float32), S.FILL)
    pv = d.put(np.full((rows, S.PARTS), S.FILL, dtype=np.float32), S.FILL)
    pi = d.put(np.full((rows, S.PARTS), S.CANARY, dtype=np.int32), S.CANARY)
    unf = d.put(unf_in, G8) if unf_in is not None else None
    nunf = d.put(nunf_in, S.CANARY) if nunf_in is not None else None
    entry_greedy_select(route, lg, rows, c.V, ldl, c.ns, stride, bias, table, c.E, c.relu, t, G_T, ids, it, emb, unf, nunf, pv, pi)
    torch.cuda.synchronize()
    d.check()
    out = {"ids": ids.cpu().numpy(), "it": it.cpu().numpy(), "emb": emb.cpu().numpy()}
    if unf is not None:
        out.update(unf=unf.cpu().numpy(), nunf=nunf.cpu().numpy())
    return out


@pytest.mark.parametrize("c", S.GREEDY_CASES, ids=lambda c: c.name)
def test_greedy_forms_against_the_argmax_rule(c):
    inp = S.greedy_inputs(c)
    ref = S.greedy_ref(c, inp)
    for route in S.greedy_routes(c):
        out = _run_greedy(c, inp, route)
        _same_twice(out, _run_greedy(c, inp, route), (c.name, route))
        what = (c.name, "route", route)
        _exact(_column(out["ids"], 1, S.CANARY, what), ref["ids"], what + ("ids",))
        _exact(out["it"], ref["ids"], what + ("it_next",))
        _bits(out["emb"], ref["emb"], what + ("emb",))


@pytest.mark.parametrize("name", ["V1025", "V4097_ns2_aligned", "V4097_ns2_ldl_odd"])
def test_greedy_select_end_bookkeeping(name):
    c = S.GREEDY_BY_NAME[name]
    inp = S.greedy_inputs(c)
    ref = S.greedy_ref(c, inp)
    rows = len(c.specs)
    unf_in = np.array([0 if r % 4 == 3 else 1 for r in range(rows)], dtype=np.uint8)
    for t, n_prev in ((0, None), (1, 3), (2, 0)):
        nunf_in = np.array([5, 5, 5], dtype=np.int32)
        nunf_in[t] = 0
        if t > 0:
            nunf_in[t - 1] = n_prev
        out = _run_greedy(c, inp, 2, t=t, unf_in=unf_in, nunf_in=nunf_in)
        unf, count = S.greedy_bookkeeping(ref["ids"], t, unf_in, n_prev)
        what = (name, "t", t)
        if unf is None:          # the dead step: ids_out[row, t] = 0 and nothing else
            assert not _column(out["ids"], t, S.CANARY, what).any()
            assert (out["it"] == S.CANARY).all() and (out["emb"] == S.FILL).all() and (out["unf"] == unf_in).all() and (out["nunf"] == nunf_in).all()
            continue
        _exact(_column(out["ids"], t, S.CANARY, what), ref["ids"], what + ("ids",))
        _exact(out["unf"], unf, what + ("unfinished",))
        want = nunf_in.copy()
        want[t] = count
        _exact(out["nunf"], want, what + ("n_unfinished",))
        assert 0 < count < rows
        _bits(out["emb"], ref["emb"], what + ("emb",))


# =====================================================================================================================
# multinomial step
def _run_sample(c, inp, philox_mode=False):
    from simpleimagecaptionzoo_amd.token_choice import entry_sample_select
    lay, rows, B, T, V = S.LAYOUTS[c.layout], inp["rows"], inp["B"], S.T_STEPS, c.V
    ldl, stride = S.geometry(lay, V, rows, c.ns)
    d = Dev()
    emb_mode = c.emb_mode
    kw = dict(V=V, ldl=ldl, ns=c.ns, slab_stride=stride, t=c.t, T=T, E=c.E, emb_mode=emb_mode, row0=c.row0)
    kw["logits"] = d.put(S.place(inp["slabs"], lay, ldl, stride), NAN, off=lay.off)
    if c.ns > 1:
        kw["bias"] = d.put(inp["bias"], NAN, off=lay.bias_off)
        kw["logits_store"] = d.put(np.full((rows, ldl), S.FILL, dtype=np.float32), S.FILL, off=lay.store_off)
    if not (c.philox and philox_mode):
        kw["uniforms"] = d.put(inp["u"], NAN)
    kw["seed"] = torch.tensor([inp["seed"]], dtype=torch.int64, device="cuda")
    kw["unfinished"] = d.put(inp["unf"], G8)
    kw["n_unfinished"] = d.put(inp["nunf"], S.CANARY)
    kw["seq_out"] = d.put(np.full((B, T), S.CANARY, dtype=np.int64), S.CANARY)
    kw["logp_out"] = d.put(np.full((B, T), S.FILL, dtype=np.float32), S.FILL)
    kw["it_next"] = d.put(np.full(rows, S.CANARY, dtype=np.int64), S.CANARY)
    kw["draw_out"] = d.put(np.full(rows, S.CANARY, dtype=np.int32), S.CANARY)
    kw["lse_out"] = d.put(np.full(rows, S.FILL, dtype=np.float32), S.FILL)
    kw["live_rows"] = d.put(np.full(1, S.CANARY, dtype=np.int32), S.CANARY)
    if c.t + 1 < T:              # as the decoders: the last step gathers no next embedding
        kw["emb_table"] = d.put(inp["table"], NAN)
        kw["emb_next"] = d.put(np.full((rows, c.E), S.FILL, dtype=np.float32), S.FILL)
        if emb_mode == 1:
            kw["emb_mask"] = d.put(inp["mask"], G8)
    if c.row0:
        kw["ids_out"] = d.put(np.full((c.row0, T), S.CANARY, dtype=np.int64), S.CANARY)
        kw["g_unfinished"] = d.put(inp["gunf"], G8)
        kw["n_any"] = d.put(inp["nany"], S.CANARY)
    entry_sample_select(rows, **kw)
    torch.cuda.synchronize()
    d.check()
    return {k: kw[k].cpu().numpy() for k in ("logits_store", "unfinished", "n_unfinished", "seq_out", "logp_out", "it_next", "draw_out", "lse_out",
                                             "live_rows", "emb_next", "ids_out", "g_unfinished", "n_any") if k in kw}


def _check_sample(c, inp, ref, out):
    what = (c.name,)
    t, row0, V = c.t, c.row0, c.V
    _exact(_column(out["seq_out"], t, S.CANARY, what), ref["seq"], what + ("seq",))
    _close(_column(out["logp_out"], t, S.FILL, what), ref["logp"][0], ref["logp"][1], what + ("logp",))
    _exact(out["it_next"], ref["it_next"], what + ("it_next",))
    _exact(out["draw_out"], ref["draw"], what + ("draw",))
    _close(out["lse_out"], ref["lse"][0], ref["lse"][1], what + ("lse",))
    _exact(out["unfinished"], ref["unf"], what + ("unfinished",))
    _exact(out["n_unfinished"], ref["nunf"], what + ("n_unfinished",))
    assert int(out["live_rows"][0]) == (S.CANARY if ref["live_rows"] is None else ref["live_rows"]), what + ("live_rows", out["live_rows"])
    if row0:
        ids = out["ids_out"]
        if ref["dead_all"]:
            assert not _column(ids, t, S.CANARY, what).any()
        else:
            _exact(_column(ids, t, S.CANARY, what), ref["ids"], what + ("ids",))
        _exact(out["g_unfinished"], ref["gunf"], what + ("g_unfinished",))
        _exact(out["n_any"], ref["nany"], what + ("n_any",))
    if "emb_next" in out:
        if ref["emb"] is None:
            assert (out["emb_next"] == S.FILL).all(), what + ("emb_next written by a dead step",)
        else:
            _bits(out["emb_next"], ref["emb"], what + ("emb_next",))
    if "logits_store" in out:
        st = out["logits_store"]
        n = 0 if ref["x"] is None else ref.get("x_rows", st.shape[0])
        if n:
            _bits(st[:n, :V], ref["x"][:n], what + ("logits_store",))
        assert (st[:n, V:] == S.FILL).all() and (st[n:] == S.FILL).all(), what + ("logits_store: pad columns or dead rows written",)


@pytest.mark.parametrize("c", S.SAMPLE_CASES, ids=lambda c: c.name)
def test_sample_select_against_float64(c):
    inp = S.sample_inputs(c)
    log = []
    ref = S.sample_ref(c, inp, log)
    assert all(m >= S.MARGIN for _, m in log), min(log, key=lambda e: e[1])
    out = _run_sample(c, inp, philox_mode=c.philox)
    _same_twice(out, _run_sample(c, inp, philox_mode=c.philox), c.name)
    _check_sample(c, inp, ref, out)
    if c.philox or c.emb_mode == 2:      # explicit mode on the bits the numpy twin draws from the same seed: the same launch, bit for bit
        twin = _run_sample(c._replace(emb_mode=1) if c.emb_mode == 2 else c, inp, philox_mode=False)
        _same_twice(out, twin, (c.name, "Philox mode against explicit mode"))


def test_three_greedy_forms_agree_bit_for_bit():
    """argmax_part_kernel + embed_argmax_kernel, greedy_select_kernel and the greedy rows of sample_select_kernel<true> on the same rows"""
    g = S.GREEDY_BY_NAME["V4097"]
    ginp = S.greedy_inputs(g)
    rows = len(g.specs)
    a, b = _run_greedy(g, ginp, 1, t=1), _run_greedy(g, ginp, 2, t=1)
    c = S._s("three_forms", g.V, E=g.E, t=1, row0=rows)
    inp = S.sample_inputs(c)
    inp["slabs"] = np.concatenate([ginp["slabs"], inp["slabs"][:, rows:]], axis=1)
    inp["table"] = ginp["table"]
    m = _run_sample(c, inp)
    for k, v in (("ids", m["ids_out"][:, 1]), ("it", m["it_next"][:rows]), ("emb", m["emb_next"][:rows])):
        ref = a[k][:, 1] if k == "ids" else a[k]
        got = b[k][:, 1] if k == "ids" else b[k]
        assert ref.tobytes() == got.tobytes() and ref.tobytes() == np.ascontiguousarray(v).tobytes(), k


@pytest.mark.parametrize("kernel", ["sample_select", "ss_select"])
def test_the_longest_row_is_taken_and_the_next_is_refused(kernel):
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.token_choice import entry_sample_select, entry_ss_select, sample_select_max_vocab
    V = sample_select_max_vocab()
    rs = S.seeded("lds")
    slabs, _ = S.make_slabs(V, [("onehot", V - 1), ("const",)], 1, False, rs)
    u = np.array([1.0 - 2.0 ** -24, (V - 0.5) / V], dtype=np.float32)
    d = Dev()
    LD = V + 64                                                   # room for the row that must be refused
    wide = np.full((2, LD), np.nan, dtype=np.float32)
    wide[:, :V] = slabs[0]
    lg = d.put(wide, NAN)
    ud = d.put(u, NAN)
    if kernel == "ss_select":
        tok = d.put(np.full(2, S.CANARY, dtype=np.int64), S.CANARY)
        gate = d.put(np.zeros(2, dtype=np.float32), NAN)
        call = lambda v: entry_ss_select(lg, 2, 2, v, LD, 0, 0.5, gate, ud, None, tok)
    else:
        unf, nunf = d.put(np.ones(2, dtype=np.uint8), G8), d.put(np.zeros(1, dtype=np.int32), S.CANARY)
        seq, lp = d.put(np.full((2, 1), S.CANARY, dtype=np.int64), S.CANARY), d.put(np.full((2, 1), S.FILL, dtype=np.float32), S.FILL)
        tok, dr, ls = (d.put(np.full(2, S.CANARY, dtype=np.int64), S.CANARY), d.put(np.full(2, S.CANARY, dtype=np.int32), S.CANARY),
                       d.put(np.full(2, S.FILL, dtype=np.float32), S.FILL))
        call = lambda v: entry_sample_select(2, logits=lg, V=v, ldl=LD, t=0, T=1, uniforms=ud, unfinished=unf, n_unfinished=nunf, seq_out=seq,
                                             logp_out=lp, it_next=tok, draw_out=dr, lse_out=ls)
    call(V)
    torch.cuda.synchronize()
    d.check()
    _exact(tok.cpu().numpy(), [V - 1, V - 1], (kernel, "V", V))
    tok.fill_(S.CANARY)
    with pytest.raises(IczError, match="%d logits does not fit in LDS" % (V + 1)):
        call(V + 1)
    torch.cuda.synchronize()
    d.check()
    _exact(tok.cpu().numpy(), [S.CANARY, S.CANARY], (kernel, "a refused shape reached a launch"))


# =====================================================================================================================
# scheduled sampling
def _run_ss(c, inp, philox_mode):
    from simpleimagecaptionzoo_amd.token_choice import entry_ss_select
    B, V = inp["B"], c.V
    ldl = S.pad_vocab(V)
    d = Dev()
    wide = np.full((B, ldl), np.nan, dtype=np.float32)
    wide[:, :V] = inp["x"]
    lg = d.put(wide, NAN)
    tok = d.put(inp["tok"], S.CANARY)
    seed = torch.tensor([inp["seed"]], dtype=torch.int64, device="cuda")
    gate, draw = (None, None) if philox_mode else (d.put(inp["gate"], NAN), d.put(inp["draw"], NAN))
    entry_ss_select(lg, B, B, V, ldl, S.SS_T - 1, c.ss_prob, gate, draw, seed, tok)
    torch.cuda.synchronize()
    d.check()
    return {"tok": tok.cpu().numpy()}


@pytest.mark.parametrize("c", S.SS_CASES, ids=lambda c: c.name)
def test_ss_select_against_float64(c):
    inp = S.ss_inputs(c)
    log = []
    ref = S.ss_ref(c, inp, log)
    assert all(m >= S.MARGIN for _, m in log)
    out = _run_ss(c, inp, c.philox)
    _same_twice(out, _run_ss(c, inp, c.philox), c.name)
    _exact(out["tok"], ref, (c.name, "tok"))
    if c.philox:
        _same_twice(out, _run_ss(c, inp, False), (c.name, "Philox mode against explicit mode"))


# =====================================================================================================================
# losses
def _run_xe(c, inp):
    from simpleimagecaptionzoo_amd.token_choice import entry_xe_loss
    B, T, V = c.B, c.T, c.V
    ldl = S.pad_vocab(V)
    d = Dev()
    wide = np.full((T * B, ldl), np.nan, dtype=np.float32)
    act = np.array([b < inp["rows_t"][t] for t in range(T) for b in range(B)])
    wide[act, :V] = inp["x"][act]                                 # inactive rows and pad columns: NaN, never read
    lg = d.put(wide, NAN)
    cap = d.put(inp["cap"], S.CANARY)
    n_dev = None if c.n_dev is None else d.put(np.array([c.n_dev], dtype=np.float32), NAN)
    rows = d.put(np.full(T * B, S.FILL, dtype=np.float32), S.FILL)
    loss = d.put(np.full(1, S.FILL, dtype=np.float32), S.FILL)
    entry_xe_loss(lg, V, ldl, cap, inp["L"], B, T, inp["rows_t"], c.smoothing, inp["n_tokens"], n_dev, rows, loss)
    torch.cuda.synchronize()
    d.check()
    return {"g": lg.cpu().numpy(), "rows": rows.cpu().numpy(), "loss": loss.cpu().numpy()}


@pytest.mark.parametrize("c", S.XE_CASES, ids=lambda c: c.name)
def test_xe_loss_and_gradient_against_float64(c):
    inp = S.xe_inputs(c)
    g, gb, rows, rb, loss, lb, act = S.xe_ref(c, inp)
    out = _run_xe(c, inp)
    _same_twice(out, _run_xe(c, inp), c.name)
    assert (out["g"][~act] == 0).all() and (out["g"][:, c.V:] == 0).all() and (out["rows"][~act] == 0).all(), (c.name, "inactive rows / pad columns")
    _close(out["g"][act, :c.V], g[act], gb[act], (c.name, "xe_grad"))
    _close(out["rows"][act], rows[act], rb[act], (c.name, "xe_row_loss"))
    _close(out["loss"][0], loss, lb, (c.name, "xe_loss"))


def _run_rf(c, inp):
    from simpleimagecaptionzoo_amd.token_choice import entry_reinforce
    B, T, V, Bs = c.B, c.T, c.V, inp["Bs"]
    ldl = S.pad_vocab(V)
    d = Dev()
    wide = np.full((T * Bs, ldl), np.nan, dtype=np.float32)
    wide[:, :V] = inp["x"]
    lg = d.put(wide, NAN)
    logp, seq, reward = d.put(inp["logp"], NAN), d.put(inp["seq"], S.CANARY), d.put(inp["reward"], NAN)
    draw, lse = d.put(inp["draw"], S.CANARY), d.put(inp["lse"], NAN)
    msum = None if c.msum is None else d.put(np.array([c.msum], dtype=np.float32), NAN)
    coef = d.put(np.full((B, T), S.FILL, dtype=np.float32), S.FILL)
    loss, ms = d.put(np.full(1, S.FILL, dtype=np.float32), S.FILL), d.put(np.full(1, S.FILL, dtype=np.float32), S.FILL)
    entry_reinforce(logp, seq, reward, B, T, msum, coef, loss, ms, lg, V, ldl, draw, lse, c.Bs, c.row0)
    torch.cuda.synchronize()
    d.check()
    return {"g": lg.cpu().numpy(), "coef": coef.cpu().numpy(), "loss": loss.cpu().numpy(), "ms": ms.cpu().numpy()}


@pytest.mark.parametrize("c", S.RF_CASES, ids=lambda c: c.name)
def test_reinforce_loss_and_gradient_against_float64(c):
    inp = S.rf_inputs(c)
    ref = S.rf_ref(c, inp)
    out = _run_rf(c, inp)
    _same_twice(out, _run_rf(c, inp), c.name)
    assert float(out["ms"][0]) == ref["ms"], (c.name, "mask sum", out["ms"], ref["ms"])
    _close(out["coef"], ref["coef"], ref["coef_bound"], (c.name, "rf_coef"))
    assert (out["coef"][ref["mask"] == 0] == 0).all() and (out["coef"][inp["reward"] == 0] == 0).all()
    _close(out["loss"][0], ref["loss"], ref["loss_bound"], (c.name, "rf_loss"))
    z = ref["zero_rows"]
    assert (out["g"][z] == 0).all() and (out["g"][:, c.V:] == 0).all(), (c.name, "zero rows / pad columns")
    _close(out["g"][~z, :c.V], ref["g"][~z], ref["g_bound"][~z], (c.name, "rf_grad"))


def test_zz_report_worst_error_fractions():
    """Last in the file: the largest error / bound per compared quantity over whatever ran above in this process (DESIGN.md section 3
    quotes the figures of a whole run; _close itself asserts every bound, so nothing here depends on which tests were selected)."""
    for k in sorted(_worst):
        print("token choice: %-12s worst error / bound %.3f" % (k, _worst[k]))
    assert all(f <= 1.0 for f in _worst.values())
