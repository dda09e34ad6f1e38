"""One "X2 = d dec . w_dec, then the TD-LSTM backward" step of the BUTD reverse-time loop, alone, through icz_test_bptt_dh1_step: the fused
launch (lstm_bwd_dh1_fused_kernel) against the two launches it replaces (the NN product into split-K slabs, then lstm_bwd_point_kernel)
and both against float64 on the same fp32 inputs.

The fused kernel promises the two launches' bits (it cuts K into the ranges the library's split rule gives the product, accumulates
each range with the same MFMA over the same k groups, and adds the ranges in slab order behind the carry and X1 terms), so bits are
asserted between the routes; every case also runs twice.

The bound is a-priori, derived as tests/_support_kernels.py derives its bounds (u = 2^-24, one fp32 rounding), never fitted:
  dh1      (fp32 additions on the element's path + 2) u sum|addends|: A products' additions + one per K range + one per slab of X1
           and of the carry + 3 to join the terms; magnitudes in float64
  tanh     10 u relative (the 5 ulp an OpenCL-conformant tanh may be off), so 1 - tanh^2 is off by at most 22 u absolutely
  dc       the dh1 bound times |o (1 - tanh^2)| + |dh1 o| 22 u + 4 u (|dc_in| + |dh1 o (1 - tanh^2)|)
  d gates  the dc (resp. dh1) bound times the element's pointwise factors + 5 u of the result's magnitude (its own roundings), and for
           d g the 2 u that 1 - g^2 may be off times |dc i|;  dc_prev: the dc bound times |f| + 2 u |dc_prev|
No element is excused.  Every output lies between guards of 7.0; everything the kernels have no business reading is NaN: the columns of
X1's rows outside [D, D + H), the floats around every operand, the carry and dc_in of a step whose carry is dead, and the slab buffer of
X2 is not even handed to the fused route.  Each test prints its largest error as a fraction of its bound.

Shapes are the smallest at which a branch can go wrong, not the model's: H = 16 (one tile: the smallest the kernel takes) and 48 (three
tiles, no multiple of the product's 64 columns), A = 64 (the smallest; one 64-deep range), the smallest A the library cuts into several
ranges (asked of the entry), 2112 and 4224 (33 stages 64 resp. 128 deep: 16 ranges of two stages and one of one, more ranges than waves),
rows on both sides of the 16-row tile and of two and four tiles."""
import itertools

import numpy as np
import pytest
import torch

import _support_kernels as S

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 16
U = S.U
D_OFF = 20                       # X1 = [d ctx | d h1]: the TD-LSTM reads columns D_OFF .. D_OFF + H of rows D_OFF + H wide
NS_X1, NS_CARRY = 3, 2
TANH_U = 10.0                    # 5 ulp
ROWS = (1, 15, 16, 17, 33, 64)
_worst = {}


def _fenced(a, ld=None, off=0):
    """The fp32 array [n, cols] as rows of stride ld (starting `off` floats into the row) of a NaN buffer with NaN in front and behind"""
    n, cols = a.shape
    ld = ld or cols
    buf = torch.full((2 * PAD + n * ld,), NAN, device="cuda")
    view = torch.as_strided(buf, (n, cols), (ld, 1), PAD + off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, view


class Guarded:
    """Outputs of the given sizes in one buffer of 7.0 with PAD guard floats around each"""

    def __init__(self, sizes):
        at, pos = [], PAD
        for n in sizes:
            at.append(pos)
            pos = (pos + n + PAD + 3) // 4 * 4
        self.buf = torch.full((pos,), S.GUARD, device="cuda")
        self.views = [self.buf[a:a + n] for a, n in zip(at, sizes)]

    def take(self):
        outs = [v.clone() for v in self.views]
        for v in self.views:
            v.fill_(S.GUARD)
        assert torch.all(self.buf == S.GUARD).item(), "a write outside the outputs"
        return outs


def _split_of(rows, H, A):
    """the K ranges the library picks for the shape: asked of the entry (a two-launch run on zeros)"""
    from simpleimagecaptionzoo_amd.butd import bptt_dh1_step
    z = lambda *s: torch.zeros(*s, device="cuda")
    ns, _ = bptt_dh1_step(0, rows, H, A, z(rows, A), z(A, H), z(1, rows, H), 1, H, z(rows, 4 * H), z(rows, H), z(rows, 4 * H), z(rows, H),
                          x2_slabs=z(64 * rows * H))
    return ns


_a_cache = {}


def _a_of(kind, H):
    """A by purpose: 'one' = the smallest the kernel takes (one range), 'several' = the smallest the library cuts into two or more ranges,
    'unequal64' / 'unequal128' = 33 stages of 64 / 128: ranges of two stages and a last one of one"""
    if (kind, H) not in _a_cache:
        if kind == "one":
            A = 64
            assert _split_of(64, H, A) == 1
        elif kind == "several":
            A = next(a for a in range(64, 1025, 64) if _split_of(64, H, a) >= 2)
        else:
            A = 33 * (64 if kind == "unequal64" else 128)
            ns = _split_of(64, H, A)
            assert 33 % ns != 0 and ns > 4, (A, ns)       # the last range is shorter, and a wave takes more than one range
        _a_cache[(kind, H)] = A
    return _a_cache[(kind, H)]


_in_cache = {}


def _inputs(rows, H, A):
    """fp32 operands of a shape, made once and never written: numpy arrays and their NaN-fenced device copies"""
    key = (rows, H, A)
    if key not in _in_cache:
        rs = S.seeded("dh1 %d %d %d" % key)
        n = {"ddec": rs.standard_normal((rows, A)), "w": rs.standard_normal((A, H)) * 0.25,
             "x1": rs.standard_normal((NS_X1 * rows, H)), "carry": rs.standard_normal((NS_CARRY * rows, H)),
             "dc_in": rs.standard_normal((rows, H)), "c_prev": rs.standard_normal((rows, H)), "c_cur": rs.standard_normal((rows, H)),
             "gates": np.concatenate([rs.uniform(0.02, 0.98, (rows, H)), rs.uniform(0.02, 0.98, (rows, H)),
                                      rs.uniform(-0.98, 0.98, (rows, H)), rs.uniform(0.02, 0.98, (rows, H))], axis=1)}
        n = {k: v.astype(np.float32) for k, v in n.items()}
        d = {k: _fenced(v) for k, v in n.items() if k != "x1"}
        d["x1"] = _fenced(n["x1"], ld=D_OFF + H, off=D_OFF)           # NaN in columns 0 .. D_OFF of every row
        _in_cache[key] = (n, d)
    return _in_cache[key]


def _reference(n, rows, H, A, ns2, rows_a, has_carry, carry_on, has_dc, has_cp, live_on):
    """float64 values and bounds of (dgates [rows, 4H], dc_prev [rows, H]); a dead step: zero d gates, bound 0, dc_prev None"""
    if not live_on:
        return np.zeros((rows, 4 * H)), np.zeros((rows, 4 * H)), None, None
    f = lambda k: n[k].astype(np.float64)
    dh = f("ddec") @ f("w")
    mag = np.abs(f("ddec")) @ np.abs(f("w"))
    adds = A + ns2 + NS_X1 + 3
    x1 = f("x1").reshape(NS_X1, rows, H)
    dh += x1.sum(0)
    mag += np.abs(x1).sum(0)
    if has_carry and carry_on:
        c = f("carry")[:NS_CARRY * rows_a].reshape(NS_CARRY, rows_a, H)
        dh[:rows_a] += c.sum(0)
        mag[:rows_a] += np.abs(c).sum(0)
        adds += NS_CARRY
    e_dh = (adds + 2) * U * mag
    dcin = np.zeros((rows, H))
    if has_dc and carry_on:
        dcin[:rows_a] = f("dc_in")[:rows_a]
    g = f("gates")
    gi, gf, gg, go = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
    cp = f("c_prev") if has_cp else np.zeros((rows, H))
    tc = np.tanh(f("c_cur"))
    s = 1.0 - tc * tc
    e_s = (2 * TANH_U + 2) * U
    dcv = dcin + dh * go * s
    e_dcv = e_dh * np.abs(go) * s + np.abs(dh * go) * e_s + 4 * U * (np.abs(dcin) + np.abs(dh * go * s))
    out = [dcv * gg * gi * (1 - gi), dcv * cp * gf * (1 - gf), dcv * gi * (1 - gg * gg), dh * tc * go * (1 - go)]
    bnd = [e_dcv * np.abs(gg * gi * (1 - gi)) + 5 * U * np.abs(out[0]),
           e_dcv * np.abs(cp * gf * (1 - gf)) + 5 * U * np.abs(out[1]),
           e_dcv * np.abs(gi * (1 - gg * gg)) + np.abs(dcv * gi) * 2 * U + 5 * U * np.abs(out[2]),
           e_dh * np.abs(tc * go * (1 - go)) + np.abs(dh * go * (1 - go)) * TANH_U * U * np.abs(tc) + 5 * U * np.abs(out[3])]
    dcp = dcv * gf
    return np.concatenate(out, 1), np.concatenate(bnd, 1), dcp, e_dcv * np.abs(gf) + 2 * U * np.abs(dcp)


def _within(what, got, ref, bound):
    g = got.cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert np.isfinite(g).all(), (what, "a value that is not finite: something read outside its operands")
    err = np.abs(g - ref)
    frac = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    bad = np.argwhere(err > bound)
    assert not len(bad), (what, "%d elements outside the bound, first at %s: %r vs %r, error / bound %.3g" % (
        len(bad), bad[0].tolist(), g[tuple(bad[0])], ref[tuple(bad[0])], frac))
    return frac


_flags = {}


def _flag(v):
    if v not in _flags:
        _flags[v] = None if v is None else torch.tensor([v], dtype=torch.int32, device="cuda")
    return _flags[v]


def _run(route, rows, H, A, d, rows_a, has_carry, has_dc, has_cp, live, carry_live, nan_carry):
    from simpleimagecaptionzoo_amd.butd import bptt_dh1_step
    out = Guarded([rows * 4 * H, rows * H])
    carry = dc_in = None
    if has_carry:       # ns slabs of rows_a rows, dense: the first NS_CARRY * rows_a rows of the operand
        carry = nan_carry[:NS_CARRY * rows_a * H] if carry_live == 0 else d["carry"][1].reshape(-1)[:NS_CARRY * rows_a * H]
    if has_dc:
        dc_in = nan_carry[:rows_a * H] if carry_live == 0 else d["dc_in"][1]
    x2 = None if route == 1 else torch.full((64 * rows * H,), NAN, device="cuda")
    ns, taken = bptt_dh1_step(route, rows, H, A, d["ddec"][1], d["w"][1], d["x1"][1], NS_X1, D_OFF + H, d["gates"][1], d["c_cur"][1],
                              out.views[0], out.views[1], carry=carry, ns_carry=NS_CARRY if has_carry else 0, rows_carry=rows_a,
                              dc_in=dc_in, c_prev=d["c_prev"][1] if has_cp else None, live=_flag(live), carry_live=_flag(carry_live),
                              x2_slabs=x2)
    assert taken == route
    dg, dcp = out.take()
    return ns, dg, dcp


# (live, carry_live): no flags at all (XE), both alive, the step behind this one dead, this step dead
FLAGS = ((None, None), (1, 1), (1, 0), (0, 1))


# every row count and every A at one tile of hidden units; at three tiles the row counts on the tile's edges and the 64-deep stages
CASES = [(rows, kind, 16) for rows in ROWS for kind in ("one", "several", "unequal64", "unequal128")] + \
        [(rows, kind, 48) for rows in (1, 16, 17, 64) for kind in ("one", "several", "unequal64")]


@pytest.mark.parametrize("rows,kind,H", CASES, ids=lambda v: str(v))
def test_fused_step_is_the_two_launches_bit_for_bit_and_both_are_near_float64(rows, kind, H):
    """rows_a absent / fewer than rows / equal, dc_in and c_prev present and null, step and carry dead and alive, X1 with a column
    offset in wider rows: the fused outputs equal the two-launch route's bit for bit, each route twice the same, both within the bound"""
    A = _a_of(kind, H)
    n, d = _inputs(rows, H, A)
    nan_carry = torch.full((NS_CARRY * rows * H + PAD,), NAN, device="cuda")
    worst = 0.0
    fewer = max(1, rows // 2)             # (one row: "fewer" is the row itself)
    for (rows_a, has_carry), has_dc, has_cp, (live, carry_live) in itertools.product(
            ((rows, False), (fewer, True), (rows, True)), (True, False), (True, False), FLAGS):
        what = (rows, H, A, "rows_a", rows_a if has_carry else None, "dc_in", has_dc, "c_prev", has_cp, "live", live, "carry", carry_live)
        runs = {r: [_run(r, rows, H, A, d, rows_a, has_carry, has_dc, has_cp, live, carry_live, nan_carry) for _ in range(2)] for r in (0, 1)}
        ns2 = runs[0][0][0]
        assert runs[1][0][0] == ns2
        for r in (0, 1):
            assert torch.equal(runs[r][0][1], runs[r][1][1]) and torch.equal(runs[r][0][2], runs[r][1][2]), (what, "route", r, "two runs differ")
        assert torch.equal(runs[0][0][1], runs[1][0][1]), (what, "d gates: the fused launch differs from the two launches")
        assert torch.equal(runs[0][0][2], runs[1][0][2]), (what, "dc_prev: the fused launch differs from the two launches")
        ref_g, bnd_g, ref_c, bnd_c = _reference(n, rows, H, A, ns2, rows_a, has_carry, carry_live != 0, has_dc, has_cp, live != 0)
        for r in (0, 1):
            worst = max(worst, _within(what + ("route", r, "d gates"), runs[r][0][1], ref_g, bnd_g))
            if ref_c is None:       # a dead step touches nothing but its d gates rows
                assert torch.all(runs[r][0][2] == S.GUARD).item(), (what, "route", r, "a dead step wrote dc_prev")
                assert torch.all(runs[r][0][1] == 0).item(), (what, "route", r, "a dead step's d gates rows are not zero")
            else:
                worst = max(worst, _within(what + ("route", r, "dc_prev"), runs[r][0][2], ref_c, bnd_c))
    _worst[(rows, kind, H)] = worst
    print("rows %d H %d A %d: largest error / bound %.3f" % (rows, H, A, worst))


def test_a_width_the_kernel_refuses_falls_to_the_two_launches():
    """H = 24 (no whole 16-column tiles) and A = 96 (no whole 64-deep stages): the loop's choice (route -1) is the two launches, which
    give what float64 gives; forcing the fused kernel there is refused without a launch.  At a width it takes, route -1 is the fused launch."""
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import bptt_dh1_step
    for H, A in ((24, 64), (16, 96)):
        rows = 17
        n, d = _inputs(rows, H, A)
        out = Guarded([rows * 4 * H, rows * H])
        args = (rows, H, A, d["ddec"][1], d["w"][1], d["x1"][1], NS_X1, D_OFF + H, d["gates"][1], d["c_cur"][1], out.views[0], out.views[1])
        x2 = torch.full((64 * rows * H,), NAN, device="cuda")
        ns2, taken = bptt_dh1_step(-1, *args, c_prev=d["c_prev"][1], x2_slabs=x2)
        assert taken == 0
        dg, dcp = out.take()
        ref_g, bnd_g, ref_c, bnd_c = _reference(n, rows, H, A, ns2, rows, False, True, False, True, True)
        _within((H, A, "d gates"), dg, ref_g, bnd_g)
        _within((H, A, "dc_prev"), dcp, ref_c, bnd_c)
        with pytest.raises(IczError, match="does not take"):
            bptt_dh1_step(1, *args, c_prev=d["c_prev"][1])
        out.take()
    rows, H, A = 17, 16, 64
    n, d = _inputs(rows, H, A)
    out = Guarded([rows * 4 * H, rows * H])
    _, taken = bptt_dh1_step(-1, rows, H, A, d["ddec"][1], d["w"][1], d["x1"][1], NS_X1, D_OFF + H, d["gates"][1], d["c_cur"][1], out.views[0],
                             out.views[1])
    assert taken == 1
    out.take()
