"""Host-side checks of tests/_support_kernels.py (no GPU): every case serves the purpose its table states -- recomputed here, from
icz_embed_grad_route_for where the threshold is the library's, so a retuned threshold names the case that lost its purpose --; every
float64 reference agrees with an independent statement of the same operation; the references rounded to fp32 (and an fp32 numpy
walk of the Adam formula) pass the a-priori bounds with room; and the icz_test_* entries refuse what they list before any launch
(the pointers handed to them here are not memory)."""
import ctypes

import numpy as np
import pytest
import torch

import _support_kernels as S


def _route_for(n_tok, E):
    from simpleimagecaptionzoo_amd.butd import embed_grad_route_for
    return embed_grad_route_for(n_tok, E)


# ---------------------------------------------------------------------------------------------------------------------
# purposes
@pytest.mark.parametrize("c", S.EG_CASES, ids=lambda c: c.name)
def test_embedding_case_serves_its_purpose(c):
    tok = S.eg_tokens(c)
    assert tok.shape == (c.n_tok,) and tok.min() >= 0 and tok.max() < c.V and c.E % 4 == 0
    assert c.purpose, "a case without a stated purpose"
    counts = np.bincount(tok, minlength=c.V)
    p = c.purpose
    unknown = set(p) - {"counts", "last_block_rows", "windows", "straddle", "live_cut", "e_trips", "e_wave", "lds_side", "route0", "slabs"}
    assert not unknown, unknown
    if "counts" in p:
        assert set(p["counts"]) <= set(counts.tolist()), (p["counts"], sorted(set(counts.tolist())))
    if "last_block_rows" in p:
        assert c.V % S.EG_ROWS == p["last_block_rows"] and 0 < p["last_block_rows"] < S.EG_ROWS
        assert counts[c.V - c.V % S.EG_ROWS:].sum() > 0, "no token in the last vocabulary block"
    if "windows" in p:
        assert -(-c.n_tok // S.EG_WIN) == p["windows"]
    if "straddle" in p:
        t, i, j = p["straddle"]
        assert np.flatnonzero(tok == t).tolist() == [i, j] and j == i + 1 and i // S.EG_WIN + 1 == j // S.EG_WIN
    if "live_cut" in p:
        heavy = np.flatnonzero(tok == c.tokens[1])
        want = {"empty": c.live == 0, "first": c.live == 1, "boundary": c.live == S.EG_WIN < c.n_tok,
                "inside": S.EG_WIN < c.live < c.n_tok and c.live % S.EG_WIN != 0 and heavy[0] < c.live <= heavy[-1]
                and (heavy >= S.EG_WIN).sum() > 0 and ((heavy >= S.EG_WIN) & (heavy < c.live)).sum() > 0,
                "beyond": c.live > c.n_tok}[p["live_cut"]]
        assert want, (c.name, c.live)
    else:
        assert c.live is None
    if "e_trips" in p:
        assert -(-c.E // 1024) == p["e_trips"]
    if "e_wave" in p:
        assert np.sign(c.E - 256) == p["e_wave"]
    if "lds_side" in p:
        route, lds = _route_for(c.n_tok, c.E)
        assert route == 1 and (lds > 48 * 1024) == (p["lds_side"] > 0)
        other = _route_for(c.n_tok - p["lds_side"], c.E)          # the neighbouring length lies on the other side
        assert (other[1] > 48 * 1024) != (lds > 48 * 1024)
    if "route0" in p:
        assert _route_for(c.n_tok, c.E)[0] == p["route0"]
    if "slabs" in p:
        assert c.ns == p["slabs"]
    for r in c.routes:       # a forced form must be able to take the case
        assert r in (0, 1, 2)
        assert r != 2 or c.E <= 1024
        assert r != 1 or _route_for(c.n_tok, c.E)[0] == 1


def test_embedding_table_covers_what_the_kernels_branch_on():
    by = S.EG_BY_NAME
    b = S.EG_BATCH
    assert set(by["hits"].purpose["counts"]) == {0, 1, b - 1, b, b + 1, 2 * b, 2 * b + 1}
    assert [by[n].n_tok for n in ("whole_1023", "whole_1024", "whole_1025", "whole_2049")] == [S.EG_WIN - 1, S.EG_WIN, S.EG_WIN + 1, 2 * S.EG_WIN + 1]
    assert {by[n].live for n in by if by[n].live is not None} == {0, 1, 1024, 1030, 5000}
    assert sorted(c.E for c in S.EG_CASES if c.name.startswith("wide_") and 1 in c.routes) == [4, 252, 256, 260, 1024, 1028]
    assert sorted(c.E for c in S.EG_CASES if c.name.startswith("wide_") and 2 in c.routes) == [4, 1020, 1024]
    # the switch between the forms: adjacent lengths, one on each side of the library's threshold
    lo, hi = by["switch_4522"], by["switch_4523"]
    assert hi.n_tok == lo.n_tok + 1 and _route_for(lo.n_tok, lo.E)[0] == 1 and _route_for(hi.n_tok, hi.E)[0] == 2
    assert _route_for(lo.n_tok, lo.E)[1] == 36 * lo.n_tok and _route_for(hi.n_tok, hi.E)[1] == 0
    assert {by["slabs_1"].ns, by["slabs_3"].ns} == {1, 3}
    assert max(c.n_tok * c.E for c in S.EG_CASES) <= 64 * 1024, "nothing at model size"
    # the known places of emb
    tok, demb, emb = S.eg_inputs(by["hits"])
    assert demb.shape == (1, 58, 8) and (emb[0, 0], emb[2, 3]) == (0.0, 0.0) and emb[0, 1] < 0 and emb[3, 3] < 0
    assert (emb == 0).sum() > 50 and (emb > 0).sum() > 50 and np.isfinite(demb).all()


def test_table_kernels_cases_serve_their_purposes():
    # weight_norm: columns on both sides of one wave's 256-column trip, rows on both sides of a 4-row block
    assert {252, 256, 260} <= set(S.WN_COLS) and max(S.WN_COLS) > 1024 and {3, 4, 5} <= set(S.WN_ROWS) and all(c % 4 == 0 for c in S.WN_COLS)
    assert [len(j) for j in S.WN_TABLES.values()] == [1, 2, 3, 4] and max(len(j) for j in S.WN_TABLES.values()) == S.WN_MAX_JOBS
    for name, jobs in S.WN_TABLES.items():
        ragged = tuple(i for i, (r, _) in enumerate(jobs) if r % 4 and i + 1 < len(jobs))
        assert ragged == S.WN_RAGGED[name], name
        assert len({shape for shape in jobs}) == len(jobs), "mixed shapes"
    assert any(0 < i for name in S.WN_TABLES for i in S.WN_RAGGED[name]), "no ragged job in the middle of a table"
    # transpose: 1..4 jobs, the shape sets, padded and offset sources
    assert [len(j) for j in S.TR_TABLES.values()] == [1, 2, 3, 4]
    jobs = [j for t in S.TR_TABLES.values() for j in t]
    assert {j[0] for j in jobs} == {64, 128, 192} and {j[1] for j in jobs} == {64, 192}
    assert all(r % 64 == 0 and c % 64 == 0 and ld % 4 == 0 and off % 4 == 0 and off + c <= ld for r, c, ld, off in jobs)
    assert any(ld > c for _, c, ld, _ in jobs) and any(off > 0 for *_, off in jobs)
    # colsum: K on both sides of the 8-row batch of the first and the last row group, N on both sides of a 32-column block
    nb = S.colsum_batches
    assert (nb(56, 0), nb(57, 0), nb(57, 1), nb(63, 6), nb(63, 7), nb(64, 7), nb(65, 7)) == (0, 1, 0, 1, 0, 1, 1)
    assert (nb(120, 0), nb(121, 0), nb(121, 1), nb(129, 7), nb(129, 0)) == (1, 2, 1, 2, 2)
    assert {0, 1, 7, 8, 9, 56, 57, 63, 64, 65, 121, 129} == set(S.COLSUM_K) and {1, 31, 32, 33, 65} == set(S.COLSUM_N)
    assert max(len(t) for t in S.COLSUM_TABLES.values()) == S.COLSUM_MAX_JOBS
    for name, t in S.COLSUM_TABLES.items():
        assert all(ldx >= N >= 1 and K >= 0 for K, N, ldx, _ in t), name
    big = [j for t in S.COLSUM_TABLES.values() for j in t]
    assert any(o2 for *_, o2 in big) and any(not o2 for *_, o2 in big) and any(K == 0 for K, *_ in big) and any(ldx > N for _, N, ldx, _ in big)
    assert any(K == 0 and i + 1 < len(t) for t in S.COLSUM_TABLES.values() for i, (K, *_) in enumerate(t)), "a K = 0 job with a job behind it"
    # the depth sums: both sides of one 256-thread block of four floats each
    assert {1020, 1024, 1028} <= set(S.SUM_WIDTHS) and 4 in S.SUM_WIDTHS and set(S.SUM_DEPTHS) == {1, 2, 5, 8} and set(S.SUM_IMAGES) == {1, 3}
    # Adam: both sides of a group of four and of a 1024-element block; 32 tensors with block-exact ones among ragged ones
    assert {3, 4, 5} <= set(S.ADAM_SIZES) and {S.ADAM_BLOCK - 1, S.ADAM_BLOCK, S.ADAM_BLOCK + 1} <= set(S.ADAM_SIZES) and 4 * S.ADAM_BLOCK + 1 in S.ADAM_SIZES
    assert len(S.ADAM_32) == S.ADAM_MAX_TENSORS and sum(n % S.ADAM_BLOCK == 0 for n in S.ADAM_32) >= 4 and sum(n % 4 != 0 for n in S.ADAM_32) >= 8
    assert any(a % S.ADAM_BLOCK == 0 and b % S.ADAM_BLOCK for a, b in zip(S.ADAM_32, S.ADAM_32[1:])), "a block-exact tensor with a tensor behind it"
    offs = set(S.ADAM_VARIANTS.values())
    assert {(0,) * 4, (1,) * 4, (2,) * 4, (3,) * 4} <= offs and {(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)} <= offs
    p, g, m, v = S.adam_inputs(1025)
    clip = np.float32(S.ADAM_CLIP)
    assert (g == clip).any() and (g == -clip).any() and (g > clip).any() and (g < -clip).any() and (np.abs(g) < clip).any()
    assert (g[g < -clip] > -1.0001 * clip).all(), "one ulp outside the clip"
    z = S.adam_zero_state(1025)
    assert z[500:520].all() and z[5] and not (g[z].any() or m[z].any() or v[z].any()) and (v[~z] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# references against independent statements
def test_embedding_reference_equals_an_explicit_loop():
    for name, relu, scale, live in (("hits", 1, 2.0, None), ("slabs_3", 1, 1.0, None), ("slabs_3", 0, 2.0, 33), ("wide_4", 1, 2.0, 0)):
        c = S.EG_BY_NAME[name]
        tok, demb, emb = S.eg_inputs(c)
        ref, bound = S.embed_grad_ref(tok, demb, emb, scale, relu, c.V, live)
        want, mag = np.zeros((c.V, c.E)), np.zeros((c.V, c.E))
        n = c.n_tok if live is None else min(live, c.n_tok)
        for i in range(n):
            for j in range(c.E):
                if relu and not emb[i, j] > 0:
                    continue
                for z in range(c.ns):
                    want[tok[i], j] += float(demb[z, i, j]) * scale
                    mag[tok[i], j] += abs(float(demb[z, i, j])) * scale
        np.testing.assert_allclose(ref, want, rtol=1e-13, atol=1e-13)
        nh = np.array([(tok[:n] == v).sum() for v in range(c.V)])
        np.testing.assert_allclose(bound, (nh * c.ns + 2)[:, None] * 2.0 ** -24 * mag, rtol=1e-12, atol=0)
        assert (bound[nh == 0] == 0).all() and (ref[nh == 0] == 0).all()


def test_weight_norm_references_equal_autograd_in_float64():
    for rows, cols in ((3, 4), (5, 260), (9, 1028)):
        v, g, dw = S.wn_inputs(rows, cols)
        (w, _), (nrm, _) = S.weight_norm_ref(v, g)
        vt = torch.tensor(v, dtype=torch.float64, requires_grad=True)
        gt = torch.tensor(g, dtype=torch.float64, requires_grad=True)
        wt = vt * (gt / vt.norm(dim=1))[:, None]
        np.testing.assert_allclose(w, wt.detach().numpy(), rtol=1e-13)
        np.testing.assert_allclose(nrm, vt.norm(dim=1).detach().numpy(), rtol=1e-13)
        wt.backward(torch.tensor(dw, dtype=torch.float64))
        # the kernel is handed the fp32 norm: the reference follows it, autograd the exact one -> 2^-24 apart, three factors deep
        (dv, bdv), (dg, bdg) = S.weight_norm_bwd_ref(dw, v, g, nrm.astype(np.float32))
        np.testing.assert_allclose(dg, gt.grad.numpy(), rtol=2e-7, atol=1e-9)
        assert (np.abs(dv - vt.grad.numpy()) <= 4 * 2.0 ** -24 * bdv / ((cols + 8) * 2.0 ** -24) + 1e-12).all()
        (dv_x, _), (dg_x, _) = S.weight_norm_bwd_ref(dw, v, g, nrm)         # with the exact norm: autograd to float64 rounding
        np.testing.assert_allclose(dv_x, vt.grad.numpy(), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(dg_x, gt.grad.numpy(), rtol=1e-12, atol=1e-13)


def test_adam_reference_equals_torch_adam_on_clamped_gradients():
    n = 1025
    p, _, _, _ = S.adam_inputs(n)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=float(np.float32(S.ADAM_LR)), betas=(0.9, 0.999), eps=1e-8)
    clip = float(np.float32(S.ADAM_CLIP))
    pc, m, v = p.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        g = S.adam_inputs(n, "step %d" % step)[1]
        pt.grad = torch.tensor(g, dtype=torch.float64).clamp(-clip, clip)
        opt.step()
        r = S.adam_ref(pc, g, m, v, S.ADAM_LR, S.ADAM_CLIP, step)
        pc, m, v = r["p"][0], r["m"][0], r["v"][0]
        # torch in float64 multiplies by 0.9, 0.1, 0.999, 0.001; the reference by the kernels' 0.9f, 1.f - 0.9f (2.4e-7 from 0.1),
        # 0.999f and 1.f - 0.999f (1.3e-5 from 0.001): that far apart and no further, a step being at most ~lr
        st = opt.state[pt]
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=5e-7, atol=1e-8)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=3e-5, atol=1e-15)
        np.testing.assert_allclose(pc, pt.detach().numpy(), rtol=0, atol=step * 2e-5 * S.ADAM_LR)
    bc1, sbc2 = S.adam_constants(1000)[:2]
    assert bc1 == 1.0 and abs(sbc2 - np.sqrt(1 - 0.999 ** 1000)) < 1e-7 and S.adam_constants(1)[0] == float(np.float32(0.1))


def test_sum_references_are_the_plain_sums():
    rs = np.random.RandomState(3)
    X = rs.standard_normal((9, 5)).astype(np.float32)
    ref, bound = S.colsum_ref(X)
    assert np.allclose(ref, [sum(float(X[k, n]) for k in range(9)) for n in range(5)], rtol=1e-14)
    assert np.allclose(bound, (2 + 8) * 2.0 ** -24 * np.abs(X.astype(np.float64)).sum(0), rtol=1e-14)
    ref, bound = S.colsum_ref(np.zeros((0, 3), dtype=np.float32))
    assert (ref == 0).all() and (bound == 0).all()
    ref, bound = S.depth_sum_ref(X)
    assert np.allclose(bound, 10 * 2.0 ** -24 * np.abs(X.astype(np.float64)).sum(0), rtol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs leave room under the bounds
def _room(ref, bound):
    """The float64 reference rounded to fp32 lies within half of its bound."""
    err = np.abs(ref.astype(np.float32).astype(np.float64) - ref)
    assert (err <= 0.5 * bound).all(), float((err / np.maximum(bound, 1e-300)).max())


def test_rounded_references_pass_every_bound_with_room():
    for c in S.EG_CASES:
        tok, demb, emb = S.eg_inputs(c)
        for relu in S.EG_RELU:
            _room(*S.embed_grad_ref(tok, demb, emb, 2.0, relu, c.V, c.live))
    for rows, cols in S.WN_SINGLE:
        v, g, dw = S.wn_inputs(rows, cols)
        (w, nrm) = S.weight_norm_ref(v, g)
        _room(*w), _room(*nrm)
        dv, dg = S.weight_norm_bwd_ref(dw, v, g, nrm[0].astype(np.float32))
        _room(*dv), _room(*dg)
    rs = np.random.RandomState(5)
    for K in S.COLSUM_K:
        _room(*S.colsum_ref(rs.standard_normal((K, 65)).astype(np.float32)))
    for T in S.SUM_DEPTHS:
        _room(*S.depth_sum_ref(rs.standard_normal((T, 1028)).astype(np.float32)))
    for n in S.ADAM_SIZES:
        for step in S.ADAM_STEPS:
            r = S.adam_ref(*S.adam_inputs(n), S.ADAM_LR, S.ADAM_CLIP, step)
            for k in "pmv":
                _room(*r[k])


def test_fp32_walk_of_the_adam_formula_passes_the_bounds():
    """The kernels' formula in numpy fp32 (no fused multiply-add; a device may fuse, which only removes roundings): within the bounds,
    and the parameter does not move where g = m = v = 0."""
    f = np.float32
    worst = 0.0
    for n in (5, 1025, 4097):
        for step in S.ADAM_STEPS:
            p, g, m, v = S.adam_inputs(n)
            bc1, sbc2 = f(S.adam_constants(step)[0]), f(S.adam_constants(step)[1])
            gv = np.minimum(np.maximum(g, -f(S.ADAM_CLIP)), f(S.ADAM_CLIP))
            mn = m * f(0.9) + gv * (f(1) - f(0.9))
            vn = v * f(0.999) + (gv * gv) * (f(1) - f(0.999))
            pn = p - (f(S.ADAM_LR) / bc1) * (mn / (np.sqrt(vn) / sbc2 + f(1e-8)))
            assert mn.dtype == vn.dtype == pn.dtype == np.float32
            r = S.adam_ref(p, g, m, v, S.ADAM_LR, S.ADAM_CLIP, step)
            for got, k in ((pn, "p"), (mn, "m"), (vn, "v")):
                ref, bound = r[k]
                frac = np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)
                assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (n, step, k, float(frac.max()))
                worst = max(worst, float(frac[bound > 0].max()))
            z = S.adam_zero_state(n)
            assert (pn[z] == p[z]).all() and not mn[z].any() and not vn[z].any()
    assert worst < 0.75, worst


# ---------------------------------------------------------------------------------------------------------------------
# refusals, all before any launch
def _lib():
    from simpleimagecaptionzoo_amd._lib import lib
    return lib()


def _fake(n, at=4096):
    return (ctypes.c_void_p * n)(*[at] * n)


def _i32(*xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def _refused(status, *words):
    err = _lib().icz_last_error()
    assert status == -1, (status, err)
    for w in words:
        assert w in err, (w, err)


def test_embedding_entry_refusals():
    L = _lib()
    P = ctypes.c_void_p(4096)
    call = lambda tok=P, n_tok=40, demb=P, ns=1, stride=0, emb=P, E=8, dE=P, V=21, relu=1, route=0: L.icz_test_embed_grad(
        tok, n_tok, demb, ns, stride, emb, 1.0, E, dE, V, relu, None, route, None)
    for n_tok, E, route in S.EG_REFUSED:
        _refused(call(n_tok=n_tok, E=E, route=route), b"icz_test_embed_grad")
    _refused(call(n_tok=40, E=1028, route=2), b"windowed form takes E <= 1024")
    _refused(call(n_tok=4523, E=4, route=1), b"LDS form holds no list of 4523")
    for hole in ("tok", "demb", "dE", "emb"):
        _refused(call(**{hole: None}), b"null argument")
    assert call(emb=None, relu=0, n_tok=0) == -1          # emb may be null without the ReLU; then n_tok is what is refused
    _refused(call(n_tok=0), b"n_tok=0")
    _refused(call(V=0), b"V=0")
    _refused(call(relu=2), b"relu=2")
    _refused(call(route=3), b"route=3")
    _refused(call(ns=0), b"ns=0")
    _refused(call(ns=3, stride=40 * 8 - 4), b"ns=3 slabs of stride 316")
    _refused(call(ns=3, stride=40 * 8 + 2), b"ns=3 slabs of stride 322")
    for hole in ("demb", "emb", "dE"):
        _refused(call(**{hole: ctypes.c_void_p(4100)}), b"16-byte aligned")
    # the host-only route
    lds = ctypes.c_size_t(7)
    assert L.icz_embed_grad_route_for(100, 8, ctypes.byref(lds)) == 1 and lds.value == 3600
    assert L.icz_embed_grad_route_for(100, 8, None) == 1
    assert L.icz_embed_grad_route_for(5000, 1024, ctypes.byref(lds)) == 2 and lds.value == 0
    lds = ctypes.c_size_t(7)
    for n_tok, E in ((0, 8), (100, 6), (100, 0), (5000, 1028)):
        _refused(L.icz_embed_grad_route_for(n_tok, E, ctypes.byref(lds)), b"icz_embed_grad_route_for")
    assert lds.value == 7


def test_table_entry_refusals():
    L = _lib()
    f5, odd5 = _fake(5), _fake(5, 4100)
    r5, c5 = _i32(4, 4, 4, 4, 4), _i32(8, 8, 8, 8, 8)
    wn = lambda multi, count, v=f5, g=f5, w=f5, norm=f5, rows=r5, cols=c5: L.icz_test_weight_norm(multi, count, v, g, w, norm, rows, cols, None)
    for multi, count in ((1, 5), (1, 0), (0, 2), (0, 0), (1, -1)):
        _refused(wn(multi, count), b"icz_test_weight_norm: count")
    for hole in ("v", "g", "w", "norm", "rows", "cols"):
        _refused(wn(1, 2, **{hole: None}), b"null table")
    _refused(wn(1, 2, v=(ctypes.c_void_p * 2)(4096, None)), b"job 1: null pointer")
    _refused(wn(1, 2, cols=_i32(8, 6)), b"job 1: 4 x 6")
    _refused(wn(1, 2, cols=_i32(0, 8)), b"job 0: 4 x 0")
    _refused(wn(1, 2, rows=_i32(4, 0)), b"job 1: 0 x 8")
    _refused(wn(1, 1, v=odd5), b"16-byte aligned")
    _refused(wn(0, 1, w=odd5), b"16-byte aligned")
    ld5 = _i32(8, 8, 8, 8, 8)
    bwd = lambda multi, count, dw=f5, lddw=ld5, v=f5, g=f5, norm=f5, dv=f5, dg=f5, rows=r5, cols=c5: L.icz_test_weight_norm_bwd(
        multi, count, dw, lddw, v, g, norm, dv, dg, rows, cols, None)
    for multi, count in ((1, 5), (1, 0), (0, 2)):
        _refused(bwd(multi, count), b"icz_test_weight_norm_bwd: count")
    for hole in ("dw", "lddw", "v", "g", "norm", "dv", "dg", "rows", "cols"):
        _refused(bwd(1, 2, **{hole: None}), b"null table")
    _refused(bwd(1, 2, lddw=_i32(8, 4)), b"job 1: lddw 4")
    _refused(bwd(1, 2, lddw=_i32(10, 8)), b"job 0: lddw 10")
    _refused(bwd(1, 2, cols=_i32(8, 6)), b"job 1: 4 x 6")
    for hole in ("dw", "v", "dv"):
        _refused(bwd(0, 1, **{hole: odd5}), b"16-byte aligned")
    s5 = _i32(64, 64, 64, 64, 64)
    tr = lambda count, src=f5, ld=s5, rows=s5, cols=s5, dst=f5: L.icz_test_transpose(count, src, ld, rows, cols, dst, None)
    for count in (0, 5, -1):
        _refused(tr(count), b"icz_test_transpose: count")
    for hole in ("src", "ld", "rows", "cols", "dst"):
        _refused(tr(2, **{hole: None}), b"null table")
    for rows, cols, ld in S.TR_REFUSED:
        _refused(tr(1, rows=_i32(rows), cols=_i32(cols), ld=_i32(ld)), b"icz_test_transpose: job 0")
    _refused(tr(2, rows=_i32(64, 65)), b"job 1: 65 x 64")
    _refused(tr(1, src=odd5), b"16-byte aligned")
    _refused(tr(1, dst=odd5), b"16-byte aligned")
    f9, k9, n9 = _fake(9), _i32(*[8] * 9), _i32(*[32] * 9)
    cs = lambda multi, count, X=f9, K=k9, N=n9, ldx=n9, out=f9, out2=None: L.icz_test_colsum(multi, count, X, K, N, ldx, out, out2, None)
    for multi, count in ((1, 9), (1, 0), (0, 2), (0, 0)):
        _refused(cs(multi, count), b"icz_test_colsum: count")
    for hole in ("X", "K", "N", "ldx", "out"):
        _refused(cs(1, 2, **{hole: None}), b"null table")
    _refused(cs(1, 2, K=_i32(8, -1)), b"job 1: K=-1")
    _refused(cs(1, 2, N=_i32(0, 32)), b"job 0: K=8, N=0")
    _refused(cs(1, 2, ldx=_i32(32, 31)), b"job 1: K=8, N=32, ldx=31")
    _refused(cs(0, 1, out2=f9), b"the single sum writes no copy")
    P, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    for X, T, BN, out in ((None, 2, 8, P), (P, 2, 8, None), (P, 0, 8, P), (P, 2, 0, P), (P, 2, 6, P), (odd, 2, 8, P), (P, 2, 8, odd)):
        _refused(L.icz_test_timesum(X, T, BN, out, None), b"icz_test_timesum")
    for X, n_img, G, N, out in ((None, 1, 2, 8, P), (P, 1, 2, 8, None), (P, 0, 2, 8, P), (P, 1, 0, 8, P), (P, 1, 2, 6, P), (P, 1, 2, 0, P),
                                (odd, 1, 2, 8, P), (P, 1, 2, 8, odd)):
        _refused(L.icz_test_rowgroup_sum(X, n_img, G, N, out, None), b"icz_test_rowgroup_sum")


def test_adam_entries_refuse_bad_tables():
    L = _lib()
    n33 = (ctypes.c_int64 * 33)(*[4] * 33)
    f33 = _fake(33)
    call = lambda count, p=f33, g=f33, m=f33, v=f33, n=n33, step=1: L.icz_adam_clamp_multi(count, p, g, m, v, n, 0.05, 0.1, step, None)
    for count in (33, 0, -1):
        _refused(call(count), b"icz_adam_clamp_multi: count %d out of range 1..32" % count)
    for hole in ("p", "g", "m", "v", "n"):
        _refused(call(2, **{hole: None}), b"bad arguments")
    _refused(call(2, step=0), b"bad arguments")
    _refused(call(2, n=(ctypes.c_int64 * 2)(4, 0)), b"tensor 1 invalid")
    _refused(call(2, m=(ctypes.c_void_p * 2)(4096, None)), b"tensor 1 invalid")
    P = ctypes.c_void_p(4096)
    for args in ((None, P, P, P, 4, 1), (P, None, P, P, 4, 1), (P, P, None, P, 4, 1), (P, P, P, None, 4, 1), (P, P, P, P, 0, 1), (P, P, P, P, 4, 0)):
        _refused(L.icz_adam_clamp_step(*args[:5], 0.05, 0.1, args[5], None), b"icz_adam_clamp_step: bad arguments")
