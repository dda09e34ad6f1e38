"""Host-side half of the embedding and LSTM pointwise kernels' own tests (tests/_lstm_kernels.py; the device half is
tests/test_gpu_lstm_kernels.py): every case takes the branch its purpose names (recomputed here from the shape, with the kernels'
loop headers written out); every reference equals an explicit scalar loop on a small case, and the backward reference equals
torch.autograd of the float64 cell; the input scales keep every gate away from saturation; the a-priori bounds reject every listed
wrong formula on every case it applies to; and the entries refuse on the host what their kernels cannot take."""
import ctypes as C
import math

import numpy as np
import torch

import _lstm_kernels as K
from _philox import RNG_EMB, RNG_OUT


def _outside(val, ref, bound):
    return int((np.abs(val - ref) > bound).sum())


# ======================================================================================================================
# the tables hold what they are asked to hold, and every case takes its branch
def _gw_loops(ns):
    """trips of lstm_point_gw_kernel's three slab loops, their headers copied"""
    z, n8, n4, n1 = 0, 0, 0, 0
    while z + 8 <= ns:
        z, n8 = z + 8, n8 + 1
    while z + 4 <= ns:
        z, n4 = z + 4, n4 + 1
    while z < ns:
        z, n1 = z + 1, n1 + 1
    return n8, n4, n1


def _geometry(H):
    """(workgroups per row, threads of the last workgroup with j < H, lanes of one of its waves with j4 = j0 + 4 lane < H)"""
    wgs = K.cdiv(H, 256)
    j0 = (wgs - 1) * 256
    return wgs, sum(1 for tid in range(256) if j0 + tid < H), (sum(1 for lane in range(64) if j0 + 4 * lane < H) if H % 4 == 0 else 0)


def test_forward_table_covers_the_branches():
    assert set(K.NS_LOOPS) == set(K.FWD_NS) == {1, 3, 4, 5, 8, 12, 13, 16, 29}
    # the tail alone, the fours alone, 4 + 1, the eights alone, 8 + 4, 8 + 4 + 1, 8 + 8, 3 x 8 + 4 + 1
    assert [K.NS_LOOPS[n] for n in (1, 4, 5, 8, 12, 13, 16, 29)] == [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 0, 0), (3, 1, 1)]
    for c in K.FWD_CASES + [K.chain_cases(m)[0] for m in K.CHAIN_MODES]:
        pp = c.purpose
        assert pp["loops"] == _gw_loops(c.ns), c.name
        assert (pp["wgs"], pp["units"], pp["quads"]) == _geometry(c.H), c.name
        assert pp["route0"] == (1 if c.H % 4 else 2) and c.routes == ((1,) if c.H % 4 else (1, 2)), c.name
        assert c.row0 < c.rows and 1 <= c.ns <= 32
        if c.pre == "gather":       # fewer parents than rows, some of them repeated, every one of them used
            assert K.GATHER_N_PRE < c.rows and sorted(set(K.GATHER_ROWS)) == list(range(K.GATHER_N_PRE)) and len(K.GATHER_ROWS) == c.rows
    cs = K.FWD_CASES
    assert {c.H for c in cs if 2 in c.routes} == {4, 20, 252, 256, 260, 516} and {c.H for c in cs if c.routes == (1,)} == {5, 255, 257}
    # one quad, a partial wave, the last lane-quad of a workgroup, exactly one workgroup, a second workgroup of one quad (twice)
    assert [_geometry(H) for H in K.FWD_H] == [(1, 4, 1), (1, 20, 5), (1, 252, 63), (1, 256, 64), (2, 4, 1), (3, 4, 1)]
    small = [c for c in cs if c.H == 4]
    assert {(c.ns, c.rows, c.pre) for c in small} >= {(ns, rows, pre) for ns in K.FWD_NS for rows in (1, 5) for pre in (None, "identity")}
    assert {(c.ns, c.pre) for c in small} >= {(ns, "gather") for ns in K.FWD_NS}
    assert {(c.gates_out, c.hdrop_out, c.mode, c.row0, c.live) for c in small} >= {
        (g, h, m, r, l) for g in (True, False) for h in (True, False) for m in (0, 1, 2) for r in (0, 2) for l in (None, 1, 0)}
    for H in K.FWD_H[1:] + K.FWD_H_ROUTE1:      # every width: all three loops at once with a gather and Philox behind row0, a mask, dead steps
        mine = [c for c in cs if c.H == H]
        assert any(min(c.purpose["loops"]) >= 1 and c.pre == "gather" and c.mode == 2 and c.row0 == 2 and c.live == 1 for c in mine), H
        assert any(c.mode == 1 for c in mine) and {c.rows for c in mine} == {1, 5}, H
        # a dead step whose first loads are a batch of eight, and one whose first load is a single slab
        assert {c.purpose["loops"][0] > 0 for c in mine if c.live == 0} == {True, False}, H
    # a dead step in front of each of the three loops
    assert {next(i for i, n in enumerate(c.purpose["loops"]) if n) for c in cs if c.live == 0} == {0, 1, 2}


def test_backward_table_covers_the_branches():
    cs = K.BWD_CASES
    for c in cs + [b for m in K.CHAIN_MODES for b in K.chain_cases(m)[1:]]:
        sets = K.bwd_sets(c)
        assert c.purpose["slabs"] == tuple(0 if s is None else s[0] for s in sets), c.name
        assert (c.purpose["wgs"], c.purpose["units"]) == _geometry(c.H)[:2], c.name
        for s in sets:
            if s:
                ns, lda, off, rows_x = s
                assert 1 <= ns <= 32 and lda >= c.H + off and 1 <= rows_x <= c.rows, c.name
        assert K.bwd_dc_rows(c) is None or 1 <= K.bwd_dc_rows(c) <= c.rows
    assert {c.H for c in cs} == set(K.BWD_H) == {4, 20, 255, 257, 516} and {c.rows for c in cs} == {1, 5, 65}
    small = [c for c in cs if c.H == 4]
    # slab counts 1, 4 and 5 spread over the three sets, each set absent in turn, both row widths, fewer and equal rows
    assert {c.purpose["slabs"] for c in small} >= {(1, 4, 5), (5, 1, 4), (4, 5, 1), (0, 4, 1), (1, 0, 5), (5, 1, 0), (1, 0, 0), (0, 0, 4)}
    for k in range(3):
        on = [K.bwd_sets(c)[k] for c in small if K.bwd_sets(c)[k]]
        assert {s[0] for s in on} == {1, 4, 5} and {s[1] > 4 for s in on} == {True, False} and {s[2] for s in on} == {0, K.WIDE_OFF}
        assert any(s[3] < c.rows for c in small for s in [K.bwd_sets(c)[k]] if s) and any(s[3] == c.rows for c in small for s in [K.bwd_sets(c)[k]] if s)
    assert {(c.sets, c.rows, c.live, c.carry_live) for c in small} >= {(s, r, l, cl) for s in K.BWD_SETS for r in K.BWD_ROWS for l, cl in K.FLAGS}
    assert {(c.mode, c.c_prev, c.dc_in) for c in small if c.dhdrop and c.sets == "abc_514"} >= {
        (m, p, d) for m in (0, 1, 2) for p in (True, False) for d in (None, "fewer", "all")}
    assert any(K.bwd_dc_rows(c) is not None and K.bwd_dc_rows(c) < c.rows for c in small) and any(K.bwd_dc_rows(c) == c.rows for c in small)
    # the language LSTM's shape (set a and dhdrop only) in every mode, NIC's image step (set a only, no c_prev)
    assert {c.mode for c in small if c.sets == "a" and c.dhdrop and c.purpose["slabs"] == (1, 0, 0)} == {0, 1, 2}
    assert any(c.sets == "a" and not c.dhdrop and not c.c_prev and c.dc_in is None for c in small)
    for H in K.BWD_H[1:]:
        mine = [c for c in cs if c.H == H]
        assert {c.rows for c in mine} == {1, 5, 65} and {c.mode for c in mine if c.dhdrop} == {0, 1, 2} and {c.live for c in mine} >= {None, 1, 0}, H
        assert any(c.carry_live == 0 for c in mine) and any(not c.c_prev for c in mine)


def test_embedding_tables_cover_the_branches():
    assert K.EMB_TOKENS[0] == 0 and K.EMB_V - 1 in K.EMB_TOKENS and len(set(K.EMB_TOKENS)) < len(K.EMB_TOKENS) == K.EMB_ROWS
    for E in K.EMB_E:
        t = K.emb_table(E)
        assert (t > 0).any(1).all() and (t < 0).any(1).all() and np.abs(t[0]).min() > 0
        groups = E // 4
        assert K.EMB_GEOMETRY[E] == (K.cdiv(groups, 256), groups - (K.cdiv(groups, 256) - 1) * 256) and E % 4 == 0
    assert [K.EMB_GEOMETRY[E][0] for E in K.EMB_E] == [1, 1, 1, 1, 2, 3]
    cs = K.EMB_CASES
    assert {(c.relu, c.mode, c.row0, c.live) for c in cs if c.E == 4} == {(r, m, r0, l) for r in (0, 1) for m in (0, 1, 2) for r0 in (0, 2) for l in (None, 1, 0)}
    for E in K.EMB_E:
        mine = [c for c in cs if c.E == E]
        assert {c.mode for c in mine} == {0, 1, 2} and {c.live for c in mine} == {None, 1, 0} and {c.relu for c in mine} == {0, 1}
        assert all((c.purpose["wgs"], c.purpose["last"]) == K.EMB_GEOMETRY[E] and c.row0 < K.EMB_ROWS for c in mine)
    assert {c.T for c in K.ST_CASES} == {1, 4, 128} and {(c.T, c.mode) for c in K.ST_CASES} == {(T, m) for T in (1, 4, 128) for m in (0, 1, 2)}
    assert any(c.rows_t == (5, 5, 3, 1) for c in K.ST_CASES) and any(c.purpose["wgs"] == 2 for c in K.ST_CASES)
    for c in K.ST_CASES:
        assert len(c.rows_t) == c.T <= 128 and c.rows_t[0] == c.B == 5 and all(a >= b for a, b in zip(c.rows_t, c.rows_t[1:]))
        assert c.purpose["ragged"] == (min(c.rows_t) < c.B) and c.purpose["last_t"] == c.T - 1
        tok = K.steps_tokens(c)
        assert tok.min() == 0 and tok.max() == K.EMB_V - 1


# ======================================================================================================================
# every reference against an explicit scalar loop
def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def test_forward_reference_is_the_scalar_cell():
    for name in ("H4_ns5_rows5_gather", "H4_g1_hd1_mode1_row02_liveNone", "H4_g1_hd1_mode2_row02_live1", "H4_ns13_rows1_identity"):
        c = K.FWD_BY_NAME[name]
        d = K.fwd_inputs(c)
        ref = K.fwd_ref(c, d)
        H = c.H
        flags = None if c.mode == 0 else K.keep_flags(c.mode, d["mask"], K.SEED, RNG_OUT, K.FWD_STEP, c.rows * H)
        for r in range(c.rows):
            for j in range(H):
                p = []
                for q in range(4):
                    s = 0.0
                    for z in range(c.ns):
                        s += float(d["slab"][z, r, q * H + j])
                    if c.pre:
                        s += float(d["pre"][d["pre_row"][r] if c.pre == "gather" else r, q * H + j])
                    s += float(d["b_ih"][q * H + j])
                    s += float(d["b_hh"][q * H + j])
                    p.append(s)
                gi, gf, gg, go = _sig(p[0]), _sig(p[1]), math.tanh(p[2]), _sig(p[3])
                cn = gf * float(d["c_prev"][r, j]) + gi * gg
                hn = go * math.tanh(cn)
                hd = hn
                if c.mode and r >= c.row0:
                    hd = 2 * hn if flags[(r - c.row0) * H + j] else 0.0
                got = [ref["gates"][0][r, q * H + j] for q in range(4)] + [ref["c"][0][r, j], ref["h"][0][r, j], ref["hdrop"][0][r, j]]
                assert np.allclose(got, [gi, gf, gg, go, cn, hn, hd], rtol=1e-13, atol=1e-15), (name, r, j)
        for k in ("gates", "c", "h"):
            assert (ref[k][1] > 0).all() and (ref[k][1] < 1e-4 * (1 + np.abs(ref[k][0]))).all(), (name, k)


def test_backward_reference_is_the_scalar_formula():
    for name in ("H4_abc_514_rows5_live1_carry1", "H4_drop_mode1_cp1_dcfewer", "H4_drop_mode2_cp0_dcall", "H4_ab_rows5_live1_carry0", "H4_lm_mode1"):
        c = K.BWD_BY_NAME[name]
        d = K.bwd_inputs(c)
        (dg, e_dg), (dcp, e_dcp) = K.bwd_ref(c, d)
        H, sets, carry = c.H, K.bwd_sets(c), c.carry_live != 0
        flags = None if c.mode == 0 else K.keep_flags(c.mode, d["mask"], K.SEED, RNG_OUT, K.BWD_STEP, c.rows * H)
        for r in range(c.rows):
            for j in range(H):
                dh = 0.0
                for i, s in enumerate(sets):
                    if s and (i or carry) and r < s[3]:
                        dh += sum(float(d["dh_" + "abc"[i]][z, r, j]) for z in range(s[0]))
                if c.dhdrop:
                    x = float(d["dhdrop"][r, j])
                    dh += x if c.mode == 0 else (2 * x if flags[r * H + j] else 0.0)
                dcin = float(d["dc_in"][r, j]) if c.dc_in and carry and r < K.bwd_dc_rows(c) else 0.0
                gi, gf, gg, go = (float(d["gates"][r, q * H + j]) for q in range(4))
                cp = float(d["c_prev"][r, j]) if c.c_prev else 0.0
                tc = math.tanh(float(d["c_cur"][r, j]))
                dcv = dcin + dh * go * (1 - tc * tc)
                want = [dcv * gg * gi * (1 - gi), dcv * cp * gf * (1 - gf), dcv * gi * (1 - gg * gg), dh * tc * go * (1 - go), dcv * gf]
                got = [dg[r, q * H + j] for q in range(4)] + [dcp[r, j]]
                assert np.allclose(got, want, rtol=1e-13, atol=1e-15), (name, r, j)
        assert (e_dg >= 0).all() and (e_dcp >= 0).all() and (e_dg < 1e-4 * (1 + np.abs(dg))).all()


def test_chained_reference_is_autograd_of_the_float64_cell():
    """sum(dh h') + sum(dhdrop drop(h')) + sum(dc_in c') differentiated by torch.autograd in float64 with respect to the pre-activation
    gates and c_prev equals the chained reference (forward reference's gates and c' through the backward reference)"""
    for mode in K.CHAIN_MODES:
        fwd, full, only = K.chain_cases(mode)
        assert fwd.rows == K.CHAIN_ROW0 + full.rows and fwd.row0 == K.CHAIN_ROW0 and fwd.H == full.H == only.H and fwd.mode == full.mode == mode
        assert K.FWD_STEP == K.BWD_STEP            # both sides draw the same Philox step
        fd = K.fwd_inputs(fwd)
        f = K.fwd_ref(fwd, fd)
        r0, H = K.CHAIN_ROW0, fwd.H
        assert (f["keep"][:r0] == -1).all() and set(np.unique(f["keep"][r0:])) == {0, 1}
        for bc in (full, only):
            bd = K.bwd_inputs(bc)
            (dg, e_dg), (dcp, e_dcp) = K.chain_ref(mode, fd, bd, bc)
            p = sum(fd["slab"].astype(np.float64)) + fd["pre"].astype(np.float64) + fd["b_ih"].astype(np.float64) + fd["b_hh"].astype(np.float64)
            p = torch.tensor(p[r0:], requires_grad=True)
            cp = torch.tensor(fd["c_prev"][r0:].astype(np.float64), requires_grad=True)
            i, fg, g, o = (p[:, k * H:(k + 1) * H] for k in range(4))
            cn = torch.sigmoid(fg) * cp + torch.sigmoid(i) * torch.tanh(g)
            hn = torch.sigmoid(o) * torch.tanh(cn)
            keep = torch.tensor(f["keep"][r0:].astype(np.float64))
            loss = (torch.tensor(bd["dhdrop"].astype(np.float64)) * hn * 2 * keep).sum()
            if bc is full:
                loss = loss + (torch.tensor(bd["dh_a"].astype(np.float64).sum(0)) * hn[:bd["dh_a"].shape[1]]).sum()
                loss = loss + (torch.tensor(bd["dc_in"].astype(np.float64)) * cn).sum()
            gp, gc = torch.autograd.grad(loss, (p, cp))
            assert np.allclose(dg, gp.numpy(), rtol=1e-11, atol=1e-14) and np.allclose(dcp, gc.numpy(), rtol=1e-11, atol=1e-14), (mode, bc.name)
            if bc is only:      # nothing but dhdrop carries gradient: zero exactly where the forward dropped
                dropped = np.tile(f["keep"][r0:] == 0, (1, 4))
                assert (dg[dropped] == 0).all() and (e_dg[dropped] == 0).all() and (dg[~dropped] != 0).all() and dropped.any() and (~dropped).any()
            # the forward's bounds reach the backward's: wider than on exact gates, and still far below the values
            (_, e_plain), _ = K.bwd_ref(bc, dict(bd, c_prev=fd["c_prev"][r0:]), gates=f["gates"][0][r0:], c_cur=f["c"][0][r0:], keep=f["keep"][r0:])
            assert (e_dg >= e_plain).all() and (e_dg > e_plain).any() and (e_dg < 1e-4 * (1 + np.abs(dg))).all()


def test_embedding_references_are_the_scalar_gather():
    for c in (cc for cc in K.EMB_CASES if cc.E in (4, 12) and cc.live != 0):
        table, mask = K.emb_table(c.E), K.emb_mask(c.name, K.EMB_ROWS * c.E)
        keep = K.row_keep(c.mode, c.row0, K.EMB_ROWS, c.E, mask, K.SEED, RNG_EMB, K.EMB_STEP)
        ref = K.embed_ref(table, K.EMB_TOKENS, c.relu, keep)
        flags = None if c.mode == 0 else K.keep_flags(c.mode, mask, K.SEED, RNG_EMB, K.EMB_STEP, K.EMB_ROWS * c.E)
        for r, tok in enumerate(K.EMB_TOKENS):
            for e in range(c.E):
                x = table[tok, e]
                if c.relu and x < 0:
                    x = np.float32(0)
                if c.mode and r >= c.row0:
                    x = x * np.float32(2) if flags[(r - c.row0) * c.E + e] else np.float32(0)
                assert ref[r, e] == x, (c.name, r, e)
    for c in (cc for cc in K.ST_CASES if cc.T == 4 and cc.E == 4):
        table, tok = K.emb_table(c.E), K.steps_tokens(c)
        mask = K.emb_mask(c.name, c.T * c.B * c.E).reshape(c.T, c.B, c.E) if c.mode == 1 else None
        ref = K.steps_ref(c, table, tok, mask)
        for t in range(c.T):
            flags = None if c.mode == 0 else K.keep_flags(c.mode, None if mask is None else mask[t].reshape(-1), K.SEED, RNG_EMB, t, c.B * c.E)
            for b in range(c.B):
                for e in range(c.E):
                    x = max(table[tok[t, b], e], np.float32(0))
                    if c.mode:
                        x = x * np.float32(2) if flags[b * c.E + e] else np.float32(0)
                    assert ref[t, b, e] == (x if b < c.rows_t[t] else K.GUARD), (c.name, t, b, e)


# ======================================================================================================================
# the scales keep the gates away from saturation, and the bounds tell the wrong formulas from the right one
def test_pre_activations_are_of_order_one():
    for c in K.FWD_CASES:
        d = K.fwd_inputs(c)
        g = K.fwd_ref(c, d)["gates"][0]
        H = c.H
        sig, tanh = np.concatenate([g[:, :2 * H], g[:, 3 * H:]], 1), g[:, 2 * H:3 * H]
        assert 0.002 < sig.min() and sig.max() < 0.998 and np.abs(tanh).max() < 0.9999, c.name       # |p| below about 6
        assert 0.2 < sig.std() / 0.21 < 2.0 or c.rows * H < 40, c.name


def test_bounds_reject_the_wrong_formulas():
    applied = {m: 0 for m in K.FWD_MUTATIONS + K.BWD_MUTATIONS}
    for c in K.FWD_CASES:
        d = K.fwd_inputs(c)
        ref = K.fwd_ref(c, d)
        for mut in K.FWD_MUTATIONS:
            if not K.fwd_mutation_applies(c, mut):
                continue
            applied[mut] += 1
            bad = K.fwd_ref(c, d, mut=mut)
            if mut == "keep_at_row":
                assert _outside(bad["hdrop"][0], *ref["hdrop"]), (c.name, mut)
                assert not _outside(bad["h"][0], *ref["h"])
            else:
                assert _outside(bad["h"][0], *ref["h"]) and _outside(bad["c"][0], *ref["c"]), (c.name, mut)
                if mut != "c_prev_next":
                    assert _outside(bad["gates"][0], *ref["gates"]), (c.name, mut)
    for c in K.BWD_CASES:
        d = K.bwd_inputs(c)
        ref = K.bwd_ref(c, d)
        for mut in K.BWD_MUTATIONS:
            if not K.bwd_mutation_applies(c, mut):
                continue
            applied[mut] += 1
            bad = K.bwd_ref(c, d, mut=mut)
            assert _outside(bad[0][0], *ref[0]), (c.name, mut)
            if mut not in ("c_prev_next", "g_deriv"):        # (those two touch d f resp. d g alone)
                assert _outside(bad[1][0], *ref[1]), (c.name, mut)
    assert all(n >= 3 for n in applied.values()), applied
    # the right formula in fp32 numpy, one rounding per operation, lies within the bounds: they are not too tight either
    for c in K.FWD_CASES[::7]:
        d = K.fwd_inputs(c)
        ref = K.fwd_ref(c, d)
        H = c.H
        p = np.zeros((c.rows, 4 * H), dtype=np.float32)
        for z in range(c.ns):
            p = p + d["slab"][z]
        if c.pre:
            p = p + d["pre"][d["pre_row"] if c.pre == "gather" else np.arange(c.rows)]
        p = (p + d["b_ih"]) + d["b_hh"]
        one = np.float32(1)
        sg = lambda x: one / (one + np.exp(-x))
        gi, gf, gg, go = sg(p[:, :H]), sg(p[:, H:2 * H]), np.tanh(p[:, 2 * H:3 * H]), sg(p[:, 3 * H:])
        cn = gf * d["c_prev"] + gi * gg
        hn = go * np.tanh(cn)
        assert cn.dtype == np.float32 and not _outside(cn.astype(np.float64), *ref["c"]) and not _outside(hn.astype(np.float64), *ref["h"]), c.name
        assert not _outside(np.concatenate([gi, gf, gg, go], 1).astype(np.float64), *ref["gates"]), c.name


# ======================================================================================================================
# refusals: returned by the host checks, before anything touches a device
FAKE = 0x1000                       # a 16-byte aligned non-null address that a refused call never reads


def _refused(status, *needles):
    from simpleimagecaptionzoo_amd._lib import lib
    msg = lib().icz_last_error().decode()
    assert status == -1 and all(n in msg for n in needles), (status, msg)


def _vp(a):
    return None if a is None else C.c_void_p(a)


def _bad_drops(DropArgs):
    return [DropArgs(3, FAKE, FAKE, 0, 0, 0), DropArgs(-1, FAKE, FAKE, 0, 0, 0), DropArgs(1, None, FAKE, 0, 0, 0), DropArgs(2, FAKE, None, 0, 0, 0),
            DropArgs(1, FAKE, None, 0, 0, -1)]


def test_embed_entries_refuse_on_the_host():
    from simpleimagecaptionzoo_amd._lib import DropArgs, lib
    L = lib()
    who = "icz_test_embed"
    for E, rows, t_off, e_off, null in K.EMB_REFUSED:
        ptrs = {"table": FAKE + 4 * t_off, "it": FAKE, "emb": FAKE + 4 * e_off}
        if null:
            ptrs[null] = None
        _refused(L.icz_test_embed(_vp(ptrs["table"]), 7, E, _vp(ptrs["it"]), rows, _vp(ptrs["emb"]), 1, None, None, None), who)
    _refused(L.icz_test_embed(_vp(FAKE + 4), 7, 8, _vp(FAKE), 5, _vp(FAKE), 1, None, None, None), who, "16-byte")
    _refused(L.icz_test_embed(_vp(FAKE), 7, 6, _vp(FAKE), 5, _vp(FAKE), 1, None, None, None), who, "E=6", "multiple of 4")
    _refused(L.icz_test_embed(_vp(FAKE), 7, 8, _vp(FAKE), 0, _vp(FAKE), 1, None, None, None), who, "rows=0")
    _refused(L.icz_test_embed(_vp(FAKE), 7, 8, None, 5, _vp(FAKE), 1, None, None, None), who, "null")
    _refused(L.icz_test_embed(_vp(FAKE), 0, 8, _vp(FAKE), 5, _vp(FAKE), 1, None, None, None), who, "V=0")
    for bad in _bad_drops(DropArgs):
        _refused(L.icz_test_embed(_vp(FAKE), 7, 8, _vp(FAKE), 5, _vp(FAKE), 1, C.byref(bad), None, None), who, "dropout")
    for off in (1, 2, 3):           # four keep flags are read with one load
        _refused(L.icz_test_embed(_vp(FAKE), 7, 8, _vp(FAKE), 5, _vp(FAKE), 1, C.byref(DropArgs(1, FAKE + off, None, 0, 0, 0)), None, None), who, "4-byte aligned")
    who = "icz_test_embed_steps"
    for T, B, rows_t in K.ST_REFUSED:
        rt = (C.c_int32 * max(len(rows_t), 1))(*rows_t)
        _refused(L.icz_test_embed_steps(_vp(FAKE), 7, 8, _vp(FAKE), T, B, rt, _vp(FAKE), None, None), who)
    rt = (C.c_int32 * 129)(*([5] * 129))
    _refused(L.icz_test_embed_steps(_vp(FAKE), 7, 8, _vp(FAKE), 129, 5, rt, _vp(FAKE), None, None), who, "T=129", "1..128")
    _refused(L.icz_test_embed_steps(_vp(FAKE), 7, 8, _vp(FAKE), 0, 5, rt, _vp(FAKE), None, None), who, "T=0")
    _refused(L.icz_test_embed_steps(_vp(FAKE), 7, 8, _vp(FAKE), 2, 5, (C.c_int32 * 2)(5, 6), _vp(FAKE), None, None), who, "rows_t[1]=6", "0..B")
    _refused(L.icz_test_embed_steps(_vp(FAKE), 7, 8, _vp(FAKE), 3, 5, (C.c_int32 * 3)(3, 4, 1), _vp(FAKE), None, None), who, "rows_t[1]=4 above rows_t[0]=3")
    _refused(L.icz_test_embed_steps(_vp(FAKE), 7, 8, _vp(FAKE), 2, 5, None, _vp(FAKE), None, None), who, "null")
    _refused(L.icz_test_embed_steps(_vp(FAKE), 7, 10, _vp(FAKE), 2, 5, (C.c_int32 * 2)(5, 5), _vp(FAKE), None, None), who, "E=10")
    _refused(L.icz_test_embed_steps(_vp(FAKE), 7, 8, _vp(FAKE), 2, 5, (C.c_int32 * 2)(5, 5), _vp(FAKE), C.byref(DropArgs(1, FAKE + 2, None, 0, 0, 0)), None),
             who, "4-byte aligned")
    _refused(L.icz_test_embed_steps(_vp(FAKE), 7, 8, _vp(FAKE), 2, 5, (C.c_int32 * 2)(5, 5), _vp(FAKE), C.byref(DropArgs(2, None, FAKE, 0, 0, 2)), None),
             who, "row0=2")


def test_lstm_entries_refuse_on_the_host():
    from simpleimagecaptionzoo_amd._lib import DropArgs, lib
    from simpleimagecaptionzoo_amd.lstm_kernels import LSTM_BWD_POINTERS, LSTM_POINT_POINTERS, lstm_bwd_args, lstm_point_args
    L = lib()

    class P:                        # stands for a device tensor at a given address
        def __init__(self, a):
            self.a = a

        def data_ptr(self):
            return self.a

    who = "icz_test_lstm_point"

    def fwd(route=1, drop=None, **kw):
        base = {n: P(FAKE) for n in LSTM_POINT_POINTERS if n not in ("pre", "pre_row", "live")}
        base.update(ns=3, rows=5, H=8, n_pre=0)
        base.update(kw)
        a = lstm_point_args(**base)
        return L.icz_test_lstm_point(route, C.byref(a), None if drop is None else C.byref(drop), None, None)

    _refused(L.icz_test_lstm_point(1, None, None, None, None), who, "null")
    for route in (-1, 3):
        _refused(fwd(route), who, "route=%d" % route)
    for kw, word in (({"ns": 0}, "ns=0"), ({"ns": 33}, "ns=33"), ({"rows": 0}, "rows=0"), ({"H": 0}, "H=0"), ({"pre_row": P(FAKE)}, "pre_row without pre"),
                     ({"pre": P(FAKE), "n_pre": 0}, "n_pre=0"), ({"pre": P(FAKE), "n_pre": 3}, "without pre_row")):
        _refused(fwd(**kw), who, word)
    for n in ("slab", "b_ih", "b_hh", "c_prev", "h_out", "c_out"):
        _refused(fwd(**{n: None}), who, "null")
    # the gate-per-wave kernel: whole groups of 4 and 16-byte loads, forced (route 2) or as launch_lstm_point's choice (route 0)
    _refused(fwd(2, H=6), who, "gate-per-wave", "H=6")
    for route in (0, 2):
        for kw in ({"slab": P(FAKE + 4)}, {"b_ih": P(FAKE + 8)}, {"b_hh": P(FAKE + 4)}, {"pre": P(FAKE + 4), "n_pre": 5}):
            _refused(fwd(route, **kw), who, "gate-per-wave", "16-byte")
    for bad in _bad_drops(DropArgs):
        _refused(fwd(drop=bad), who, "dropout")

    who = "icz_test_lstm_bwd_point"

    def bwd(drop=None, **kw):
        base = {n: P(FAKE) for n in ("gates", "c_cur", "dgates", "dc_prev", "dh_a")}
        base.update(rows=5, H=8, ns_a=2, lda_a=8, rows_a=5)
        base.update(kw)
        a = lstm_bwd_args(**base)
        return L.icz_test_lstm_bwd_point(C.byref(a), None if drop is None else C.byref(drop), None)

    assert set(LSTM_BWD_POINTERS) >= {"dh_a", "dh_b", "dh_c", "dhdrop", "dc_in", "c_prev", "live", "carry_live"}
    _refused(L.icz_test_lstm_bwd_point(None, None, None), who, "null")
    for n in ("gates", "c_cur", "dgates", "dc_prev"):
        _refused(bwd(**{n: None}), who, "null")
    for kw, word in (({"rows": 0}, "rows=0"), ({"H": 0}, "H=0"), ({"lda_a": 7}, "set a with lda=7 below H=8"), ({"rows_a": 6}, "set a with 6 rows"),
                     ({"rows_a": 0}, "set a with 0 rows"), ({"ns_a": 0}, "set a with ns=0"), ({"ns_a": 33}, "set a with ns=33"),
                     ({"dh_b": P(FAKE), "ns_b": 0, "lda_b": 8, "rows_b": 5}, "set b with ns=0"),
                     ({"dh_b": P(FAKE), "ns_b": 1, "lda_b": 4, "rows_b": 5}, "set b with lda=4"),
                     ({"dh_c": P(FAKE), "ns_c": 1, "lda_c": 8, "rows_c": 9}, "set c with 9 rows"),
                     ({"dh_c": P(FAKE), "ns_c": -1, "lda_c": 8, "rows_c": 5}, "set c with ns=-1"),
                     ({"dc_in": P(FAKE), "dc_in_rows": 6}, "dc_in_rows=6"), ({"dc_in": P(FAKE), "dc_in_rows": 0}, "dc_in_rows=0")):
        _refused(bwd(**kw), who, word)
    for bad in _bad_drops(DropArgs):
        _refused(bwd(drop=bad), who, "dropout")
    _refused(bwd(drop=DropArgs(2, None, FAKE, 0, 0, 2)), who, "row0=2")
