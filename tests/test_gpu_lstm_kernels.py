"""The kernels of csrc/lstm_kernels.h, each alone through its icz_test_* entry (include/icz.h), against the float64 references and the
a-priori bounds of tests/_lstm_kernels.py (its docstring derives them; tests/test_cpu_lstm_kernels.py holds the tables and references
to their purposes on the host).

Exact, compared by value with == (the sign of a zero is not judged): both embedding kernels against the fp32 gather; embed_steps row
(t, b) against embed_kernel run for step t alone; the dropped copy of h' against the kernel's own h'; lstm_point_kernel against
lstm_point_gw_kernel in every output at every shape both take; every launch against its repetition; a dead step's outputs.
Bounded, no element excused: h', c', the activated gates, d gates and dc_prev against float64.

Every operand lies in a buffer of NaN (the unused columns of rows wider than H too), every output between guards of 7.0 that are
checked after every launch; what a dead step or a dead carry must not use is NaN.  Each test prints its largest error as a fraction of
its bound and the kernel route 0 took."""
import numpy as np
import pytest
import torch

import _lstm_kernels as K
from _philox import RNG_EMB, RNG_OUT

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 16


def _fenced(a, ld=None, off=0):
    """The fp32 array [n, cols] as rows of stride ld (starting `off` floats into the row) of a NaN buffer with NaN in front and behind"""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, a.shape[-1])
    n, cols = a.shape
    ld = ld or cols
    buf = torch.full((2 * PAD + n * ld,), NAN, device="cuda")
    view = torch.as_strided(buf, (n, cols), (ld, 1), PAD + off)
    view.copy_(torch.from_numpy(a))
    return buf, view


class Guarded:
    """Outputs of the given sizes in one buffer of 7.0 with PAD guard floats around each (every output starts on 16 bytes)"""

    def __init__(self, sizes):
        at, pos = [], PAD
        for n in sizes:
            at.append(pos)
            pos = (pos + n + PAD + 3) // 4 * 4
        self.buf = torch.full((pos,), K.GUARD, device="cuda")
        self.views = [self.buf[a:a + n] for a, n in zip(at, sizes)]

    def take(self):
        outs = [v.clone() for v in self.views]
        for v in self.views:
            v.fill_(K.GUARD)
        assert torch.all(self.buf == K.GUARD).item(), "a write outside the outputs"
        return outs


def _within(what, got, ref, bound):
    g = got.cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert np.isfinite(g).all(), (what, "a value that is not finite: something read outside its operands")
    err = np.abs(g - ref)
    frac = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    bad = np.argwhere(err > bound)
    assert not len(bad), (what, "%d elements outside the bound, first at %s: %r vs %r, error / bound %.3g" % (
        len(bad), bad[0].tolist(), g[tuple(bad[0])], ref[tuple(bad[0])], frac))
    return frac


def _untouched(t):
    return bool(torch.all(t == K.GUARD).item())


_flags = {}


def _flag(v):
    if v not in _flags:
        _flags[v] = None if v is None else torch.tensor([v], dtype=torch.int32, device="cuda")
    return _flags[v]


def _seed():
    if "seed" not in _flags:
        _flags["seed"] = torch.tensor([K.SEED], dtype=torch.int64, device="cuda")
    return _flags["seed"]


def _bytes(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _drop(mode, mask, stream, step, row0=0):
    from simpleimagecaptionzoo_amd.lstm_kernels import drop
    return drop(mode, mask=mask if mode == 1 else None, seed=_seed() if mode == 2 else None, stream=stream, step=step, row0=row0)


# ======================================================================================================================
# embed_kernel
@pytest.mark.parametrize("E", K.EMB_E)
def test_embed_is_the_fp32_gather(E):
    from simpleimagecaptionzoo_amd.lstm_kernels import entry_embed
    rows = K.EMB_ROWS
    table = K.emb_table(E)
    tbuf, tdev = _fenced(table)
    it = torch.tensor(K.EMB_TOKENS, dtype=torch.int64, device="cuda")
    n = 0
    for c in (cc for cc in K.EMB_CASES if cc.E == E):
        mask = K.emb_mask(c.name, rows * E)
        mdev = _bytes(mask[:(rows - c.row0) * E])              # the flags of the sampled rows and no more
        out = Guarded([rows * E])
        got = []
        for _ in range(2):
            entry_embed(tdev, it, out.views[0], rows, relu=c.relu, drop=_drop(c.mode, mdev, RNG_EMB, K.EMB_STEP, c.row0), live=_flag(c.live))
            got.append(out.take()[0])
        assert torch.equal(got[0], got[1]), (c.name, "two runs differ")
        if c.live == 0:
            assert _untouched(got[0]), (c.name, "a dead step wrote")
            continue
        keep = K.row_keep(c.mode, c.row0, rows, E, mask, K.SEED, RNG_EMB, K.EMB_STEP)
        ref = torch.from_numpy(K.embed_ref(table, K.EMB_TOKENS, c.relu, keep))
        assert bool((got[0].cpu().view(rows, E) == ref).all()), (c.name, "not the gather")
        n += 1
    print("E %d: %d cases equal the fp32 gather" % (E, n))


@pytest.mark.parametrize("c", K.ST_CASES, ids=lambda c: c.name)
def test_embed_steps_is_embed_step_by_step(c):
    from simpleimagecaptionzoo_amd.lstm_kernels import entry_embed, entry_embed_steps
    table, tok = K.emb_table(c.E), K.steps_tokens(c)
    tbuf, tdev = _fenced(table)
    tokdev = torch.from_numpy(tok).cuda()
    mask = K.emb_mask(c.name, c.T * c.B * c.E).reshape(c.T, c.B, c.E) if c.mode == 1 else None
    mdev = None if mask is None else _bytes(mask)
    out = Guarded([c.T * c.B * c.E])
    got = []
    for _ in range(2):
        entry_embed_steps(tdev, tokdev, out.views[0], c.T, c.B, c.rows_t, drop=_drop(c.mode, mdev, RNG_EMB, 99))     # (the step field is not read)
        got.append(out.take()[0])
    assert torch.equal(got[0], got[1]), "two runs differ"
    all_steps = got[0].view(c.T, c.B, c.E)
    ref = torch.from_numpy(K.steps_ref(c, table, tok, mask))
    assert bool((all_steps.cpu() == ref).all()), "not the gather of every step, or a row at b >= rows_t[t] was written"
    one = Guarded([c.B * c.E])
    for t in range(c.T):            # step t alone: its mask slice, its Philox step, its rows
        n = c.rows_t[t]
        entry_embed(tdev, tokdev[t], one.views[0], n, relu=1, drop=_drop(c.mode, None if mdev is None else mdev[t], RNG_EMB, t))
        alone = one.take()[0].view(c.B, c.E)
        assert _untouched(alone[n:]) and torch.equal(alone[:n], all_steps[t, :n]), (t, "differs from embed_kernel on step t alone")
    print("%s: %d steps equal the fp32 gather and embed_kernel alone" % (c.name, c.T))


# ======================================================================================================================
# lstm_point_kernel / lstm_point_gw_kernel
def _fwd_device(c, d):
    """-> (the operands' device views by name, their NaN buffers)"""
    fenced = {k: _fenced(d[k]) for k in ("slab", "b_ih", "b_hh", "c_prev") + (("pre",) if c.pre else ())}
    return {k: v[1] for k, v in fenced.items()}, [v[0] for v in fenced.values()]


def _fwd_run(route, c, d, dev, mdev):
    from simpleimagecaptionzoo_amd.lstm_kernels import entry_lstm_point
    rows, H = c.rows, c.H
    sizes = [rows * H, rows * H] + ([rows * 4 * H] if c.gates_out else []) + ([rows * H] if c.hdrop_out else [])
    out = Guarded(sizes)
    v = list(out.views)
    kw = dict(slab=dev["slab"], ns=c.ns, b_ih=dev["b_ih"], b_hh=dev["b_hh"], c_prev=dev["c_prev"], h_out=v[0], c_out=v[1], rows=rows, H=H, live=_flag(c.live))
    if c.gates_out:
        kw["gates_out"] = v[2]
    if c.hdrop_out:
        kw["hdrop_out"] = v[-1]
    if c.pre:
        kw.update(pre=dev["pre"], n_pre=d["pre"].shape[0])
        if c.pre == "gather":
            kw["pre_row"] = dev["pre_row"]
    taken = entry_lstm_point(route, drop=_drop(c.mode, mdev, RNG_OUT, K.FWD_STEP, c.row0), **kw)
    got = out.take()
    res = {"h": got[0], "c": got[1]}
    if c.gates_out:
        res["gates"] = got[2]
    if c.hdrop_out:
        res["hdrop"] = got[-1]
    return taken, res


def _fwd_check(c):
    """every route twice, the routes against each other, the outputs against float64 -> (largest error / bound, route 0's kernel)"""
    d = K.fwd_inputs(c)
    dev, keepalive = _fwd_device(c, d)
    if c.pre == "gather":
        dev["pre_row"] = torch.from_numpy(d["pre_row"]).cuda()
    mdev = _bytes(d["mask"][:(c.rows - c.row0) * c.H])
    runs = {}
    for route in (0,) + c.routes:
        a, b = _fwd_run(route, c, d, dev, mdev), _fwd_run(route, c, d, dev, mdev)
        assert a[0] == b[0] == (route or c.purpose["route0"]), (c.name, "route", route, "took", a[0])
        assert all(torch.equal(a[1][k], b[1][k]) for k in a[1]), (c.name, "route", route, "two runs differ")
        runs[route] = a[1]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[c.purpose["route0"]][k]), (c.name, k, "route 0 differs from the kernel it reports")
        if 2 in c.routes:
            assert torch.equal(runs[1][k], runs[2][k]), (c.name, k, "the gate-per-wave kernel differs from the one-unit kernel")
    worst = 0.0
    if c.live == 0:
        assert all(_untouched(t) for r in runs.values() for t in r.values()), (c.name, "a dead step wrote")
        return worst, c.purpose["route0"]
    ref = K.fwd_ref(c, d)
    for route, r in runs.items():
        for k in ("h", "c", "gates"):
            if k in r:
                worst = max(worst, _within((c.name, "route", route, k), r[k], *ref[k]))
        if c.hdrop_out:             # exactly the kernel's own h', doubled where kept, zero where dropped, itself in front of row0 and in mode 0
            keep = torch.from_numpy(ref["keep"].reshape(-1)).cuda()
            h = r["h"]
            want = torch.where(keep < 0, h, torch.where(keep > 0, h * 2, torch.zeros_like(h)))
            assert bool((r["hdrop"] == want).all()), (c.name, "route", route, "hdrop is not the kernel's own h' kept and doubled")
    return worst, c.purpose["route0"]


@pytest.mark.parametrize("H", K.FWD_H + K.FWD_H_ROUTE1)
def test_lstm_point_kernels_agree_bit_for_bit_and_are_near_float64(H):
    worst, routes, n = 0.0, set(), 0
    for c in (cc for cc in K.FWD_CASES if cc.H == H):
        w, r0 = _fwd_check(c)
        worst, n = max(worst, w), n + 1
        routes.add(r0)
    assert len(routes) == 1
    print("forward H %d: %d cases, route 0 took kernel %d, largest error / bound %.3f" % (H, n, routes.pop(), worst))


# ======================================================================================================================
# lstm_bwd_point_kernel
def _bwd_run(c, d, mdev, gates=None, c_cur=None, c_prev=None, step=K.BWD_STEP):
    """-> (dgates, dc_prev).  gates / c_cur / c_prev: device tensors in place of the case's own operands (the chained case)"""
    from simpleimagecaptionzoo_amd.lstm_kernels import entry_lstm_bwd_point
    rows, H = c.rows, c.H
    keepalive = []

    def fenced(a, **kw):
        buf, view = _fenced(a, **kw)
        keepalive.append(buf)
        return view

    def nan_like(n):
        keepalive.append(torch.full((n + 2 * PAD,), NAN, device="cuda"))
        return keepalive[-1][PAD:]

    dead, carry = c.live == 0, c.carry_live != 0
    kw = dict(rows=rows, H=H, live=_flag(c.live), carry_live=_flag(c.carry_live))
    for i, (k, s) in enumerate(zip("abc", K.bwd_sets(c))):
        if s:
            ns, lda, off, rows_x = s
            # a dead carry: set a must not be read and holds NaN
            kw["dh_" + k] = nan_like(ns * rows_x * lda) if (i == 0 and not carry) else fenced(d["dh_" + k], ld=lda, off=off)
            kw.update({"ns_" + k: ns, "lda_" + k: lda, "rows_" + k: rows_x})
    if c.dhdrop:
        kw["dhdrop"] = nan_like(rows * H) if dead else fenced(d["dhdrop"])
    if c.dc_in:
        n = K.bwd_dc_rows(c)
        kw["dc_in"] = nan_like(n * H) if not carry else fenced(d["dc_in"][:n])         # NaN behind dc_in_rows
        kw["dc_in_rows"] = n
    kw["gates"] = nan_like(rows * 4 * H) if dead else (gates if gates is not None else fenced(d["gates"]))
    kw["c_cur"] = nan_like(rows * H) if dead else (c_cur if c_cur is not None else fenced(d["c_cur"]))
    if c.c_prev:
        kw["c_prev"] = c_prev if c_prev is not None else fenced(d["c_prev"])
    out = Guarded([rows * 4 * H, rows * H])
    kw.update(dgates=out.views[0], dc_prev=out.views[1])
    res = []
    for _ in range(2):
        entry_lstm_bwd_point(drop=_drop(c.mode, mdev, RNG_OUT, step), **kw)
        res.append(out.take())
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (c.name, "two runs differ")
    return res[0]


def _bwd_judge(c, got, ref):
    (rg, bg), rc = ref
    worst = _within((c.name, "d gates"), got[0], rg, bg)
    if rc is None:                  # a dead step: zero d gates rows and nothing else
        assert bool(torch.all(got[0] == 0).item()) and _untouched(got[1]), (c.name, "a dead step wrote dc_prev, or its d gates rows are not zero")
        return worst
    return max(worst, _within((c.name, "dc_prev"), got[1], *rc))


@pytest.mark.parametrize("H", K.BWD_H)
def test_lstm_backward_pointwise_is_near_float64(H):
    worst, n = 0.0, 0
    for c in (cc for cc in K.BWD_CASES if cc.H == H):
        d = K.bwd_inputs(c)
        got = _bwd_run(c, d, _bytes(d["mask"]))
        worst, n = max(worst, _bwd_judge(c, got, K.bwd_ref(c, d))), n + 1
    print("backward H %d: %d cases, largest error / bound %.3f" % (H, n, worst))


# ======================================================================================================================
# forward into backward: the one place that ties the two sides' dropout indexing together
@pytest.mark.parametrize("mode", K.CHAIN_MODES)
def test_forward_outputs_through_the_backward_give_the_float64_gradient(mode):
    """The forward kernel with two evaluation-mode rows in front (row0 = 2) stores gates and c'; the backward kernel runs on the sampled
    rows alone with the same mask / seed.  Its d gates and dc_prev lie within the bound around the float64 gradient of the float64
    cell (the forward's bounds carried through), and with nothing but dhdrop carrying gradient they are zero exactly where forward
    row r + 2 dropped"""
    fwd, full, only = K.chain_cases(mode)
    r0, H = K.CHAIN_ROW0, fwd.H
    fd = K.fwd_inputs(fwd)
    dev, keepalive = _fwd_device(fwd, fd)
    mdev = _bytes(fd["mask"][:(fwd.rows - r0) * H])
    taken, f = _fwd_run(0, fwd, fd, dev, mdev)
    assert taken == 2
    fref = K.fwd_ref(fwd, fd)
    worst = max(_within(("chain forward", k), f[k], *fref[k]) for k in ("h", "c", "gates"))
    dropped = torch.from_numpy(fref["keep"][r0:] == 0).cuda()
    hd, h = f["hdrop"].view(fwd.rows, H), f["h"].view(fwd.rows, H)
    assert torch.equal(hd[:r0], h[:r0]) and bool((hd[r0:][dropped] == 0).all()) and bool((hd[r0:][~dropped] == 2 * h[r0:][~dropped]).all())
    assert bool(dropped.any()) and bool((~dropped).any()) and bool((h != 0).all())
    gates, c_cur, c_prev = f["gates"].view(fwd.rows, 4 * H)[r0:], f["c"].view(fwd.rows, H)[r0:], dev["c_prev"][r0:]
    for bc in (full, only):
        bd = K.bwd_inputs(bc)
        got = _bwd_run(bc, bd, mdev, gates=gates, c_cur=c_cur, c_prev=c_prev, step=K.FWD_STEP)
        worst = max(worst, _bwd_judge(bc, got, K.chain_ref(mode, fd, bd, bc)))
        if bc is only:
            dg = got[0].view(bc.rows, 4, H)
            assert bool((dg[dropped[:, None, :].expand(-1, 4, -1)] == 0).all()), "gradient where the forward dropped"
            assert bool((dg[~dropped[:, None, :].expand(-1, 4, -1)] != 0).all()), "no gradient where the forward kept"
    print("chain mode %d: largest error / bound %.3f" % (mode, worst))
