"""The twelve kernels of csrc/butd_kernels.h, each alone through its icz_test_att_* entry (include/icz.h; the entries launch through the
helpers of csrc/butd_impl.h that Butd::step and the BPTT launch through), against the float64 references and the a-priori bounds of
tests/_butd_att_kernels.py (its docstring derives them; tests/test_cpu_butd_att_kernels.py holds the tables and references to their
purposes on the host).

Bounded, no element excused: scores, alpha, ctx, the mean, dalpha (each part and the parts summed in part order), ds, ddec, denc, each
part of dwaff_part and its column sum.  Exact, compared by value with ==: dec_ctx_out against its fp32 twin; alpha = 1 and ds = 0 with one
region; zeros behind an image's count; every launch against its repetition; Philox against the explicit mask of its host twin; scores
and denc at other `parts`; a grouped kernel against the per-row kernel on the same rows (d enc_ctx: per row, then icz_test_rowgroup_sum);
an image of c <= 64 regions under <true> against <false> alone at R = c; the counted mean against the plain one at R = c; saved_alphas
against the fp32 mean in head order; what a dead step leaves.

Every operand lies in a buffer of NaN, and NaN are: the columns D .. ldc of dctx, the pad regions of feats and enc_ctx, the scores and
alpha behind an image's count, dalpha_part behind the count where d dec reads it, the images no row refers to, the first half of a
merged chain's rows.  Every output lies between guards of 7.0 that are checked after every launch.  Each test prints its largest error
as a fraction of its bound."""
import numpy as np
import pytest
import torch

import _butd_att_kernels as K
from _philox import RNG_ATT
from test_gpu_support_kernels import Laid, _fenced

pytestmark = pytest.mark.gpu

_worst = {}              # kernel -> largest error / bound seen
_cache = {}


def _within(kernel, what, got, ref, bound):
    """got within `bound` of `ref`, element by element; == where the bound is 0"""
    g = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    assert np.isfinite(g).all(), (kernel, what, "a value that is not finite: something read outside its operands")
    err = np.abs(g - ref)
    frac = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    _worst[kernel] = max(_worst.get(kernel, 0.0), frac)
    bad = np.argwhere(err > bound)
    assert not len(bad), (kernel, what, "%d elements outside the bound, first at %s: %r vs %r, error / bound %.3g" % (
        len(bad), bad[0].tolist(), g[tuple(bad[0])], ref[tuple(bad[0])], frac))
    return frac


def _dev(a):
    """the fp32 array, flat, in a buffer of NaN (16-byte aligned)"""
    return _fenced(np.ascontiguousarray(a, dtype=np.float32).reshape(1, -1))[0]


def _i32(v):
    return None if v is None else torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _flag(v):
    return None if v is None else _i32([v])


def _seed():
    if "seed" not in _cache:
        _cache["seed"] = torch.tensor([K.SEED], dtype=torch.int64, device="cuda")
    return _cache["seed"]


def _bytes(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t, shape):
    return t.cpu().numpy().reshape(shape)


def _untouched(a):
    return bool((np.asarray(a) == K.GUARD).all())


def _same(a, b, what):
    for x, y in zip(a, b):
        if x is not None:
            assert np.array_equal(x, y), (what, "first difference at", np.argwhere(x != y)[:1].tolist())


# ======================================================================================================================
# runners: explicit operands in, outputs as numpy out (the guards are checked inside Laid.take)
def run_scores(route, enc, img, slab, b_dec, w, b_aff, R, counts, mode, mask, row0, live, G, parts, want_dec=True):
    from simpleimagecaptionzoo_amd.butd_att_kernels import drop, entry_att_scores
    nsplit, rows, A = slab.shape
    out = Laid([rows * R, rows * A])
    mdev = _bytes(mask[:(rows - row0) * R * A]) if mode == 1 else None            # the flags of the sampled rows and no more
    d = drop(mode, mask=mdev, seed=_seed() if mode == 2 else None, stream=RNG_ATT, step=K.STEP, row0=row0)
    entry_att_scores(route, drop=d, G=G, parts=parts, enc_ctx=_dev(enc), n_img=enc.shape[0], img_of_row=_i32(img), dec_slab=_dev(slab), nsplit=nsplit,
                     b_dec=_dev(b_dec), w_aff=_dev(w), b_aff=_dev(b_aff), dec_ctx_out=out.views[1] if want_dec else None, scores=out.views[0],
                     rows=rows, R=R, A=A, live=_flag(live), counts=_i32(counts))
    s, dc = out.take()
    return _np(s, (rows, R)), _np(dc, (rows, A))


def _score_kw(c, x):
    return dict(route=c.route, enc=x["enc"], img=c.img, slab=x["slab"], b_dec=x["b_dec"], w=x["w"], b_aff=x["b_aff"], R=c.R, counts=c.counts,
                mode=c.mode, mask=x["mask"], row0=c.row0, live=c.live, G=c.G, parts=c.parts)


def run_ctx(feats, img, scores, R, counts, G, alpha2, live):
    from simpleimagecaptionzoo_amd.butd_att_kernels import entry_att_ctx
    rows, D = scores.shape[0], feats.shape[2]
    st = R + K.ALPHA2_PAD
    out = Laid([rows * R, rows * D, rows * st])
    entry_att_ctx(_dev(feats), feats.shape[0], _dev(scores), out.views[0], out.views[1], rows, R, D, G=G, img_of_row=_i32(img),
                  alpha_out2=out.views[2] if alpha2 else None, alpha2_stride=st if alpha2 else 0, live=_flag(live), counts=_i32(counts))
    al, cx, a2 = out.take()
    return _np(al, (rows, R)), _np(cx, (rows, D)), _np(a2, (rows, st))


def run_dalpha(slab, feats, img, R, D, counts, live):
    from simpleimagecaptionzoo_amd.butd_att_kernels import entry_att_bwd_dalpha
    ns, rows, ldc = slab.shape
    P = K.cdiv(D, K.CONST["DALPHA_COLS"])
    out = Laid([rows * P * R])
    entry_att_bwd_dalpha(_dev(slab), ns, ldc, rows, _dev(feats), feats.shape[0], R, D, out.views[0], live=_flag(live), img_of_row=_i32(img),
                         counts=_i32(counts))
    return _np(out.take()[0], (rows, P, R))


def run_ddec(enc, img, dec, w, alpha, parts, R, counts, mode, mask, live):
    from simpleimagecaptionzoo_amd.butd_att_kernels import drop, entry_att_bwd_ddec
    rows, A = dec.shape
    out = Laid([rows * A, rows * R])
    mdev = _bytes(mask) if mode == 1 else None             # (kept alive over the call: drop() takes its address)
    d = drop(mode, mask=mdev, seed=_seed() if mode == 2 else None, stream=RNG_ATT, step=K.STEP)
    entry_att_bwd_ddec(drop=d, enc_ctx=_dev(enc), n_img=enc.shape[0], dec_ctx=_dev(dec), w_aff=_dev(w), alpha=_dev(alpha), dalpha=_dev(parts),
                       ddec=out.views[0], ds_out=out.views[1], rows=rows, R=R, A=A, nparts=parts.shape[1], live=_flag(live), img_of_row=_i32(img),
                       counts=_i32(counts))
    dd, ds = out.take()
    return _np(ds, (rows, R)), _np(dd, (rows, A))


MASK_GAP = 8             # bytes between the keep flags of two steps (mask_step = B R A + 8)


def run_denc(enc, img, dec_all, ds_all, off, w, B, R, counts, mode, mask, G, parts):
    """-> denc [B or B / G, R, A], dwaff_part [B or B / G, parts, A], parts"""
    from simpleimagecaptionzoo_amd.butd_att_kernels import entry_att_bwd_denc
    T, Bs, A = dec_all.shape
    n_out = B // G if G else B
    np_ = parts or K.denc_parts(type("c", (), dict(parts=0, G=G, R=R)))
    out = Laid([n_out * R * A, n_out * np_ * A])
    mdev, step = None, 0
    if mode == 1:
        step = B * R * A + MASK_GAP
        m = np.full((T, step), 255, dtype=np.uint8)
        m[:, :B * R * A] = mask
        mdev = _bytes(m)
    used = entry_att_bwd_denc(G=G, parts=parts, enc_ctx=_dev(enc), n_img=enc.shape[0], dec_all=_dev(dec_all)[off * A:], ds_all=_dev(ds_all)[off * R:],
                              w_aff=_dev(w), denc=out.views[0], dwaff_part=out.views[1], B=B, R=R, A=A, T=T, mode=mode, mask=mdev, mask_step=step,
                              seed=_seed() if mode == 2 else None, stream=RNG_ATT, Bs=0 if Bs == B else Bs, img_of_row=_i32(img), counts=_i32(counts))
    assert used == np_, (used, np_)
    de, dw = out.take()
    return _np(de, (n_out, R, A)), _np(dw, (n_out, np_, A)), np_


def _denc_kw(c, x):
    return dict(enc=x["enc"], img=c.img, dec_all=x["dec_all"], ds_all=x["ds_all"], off=x["off"], w=x["w"], B=c.B, R=c.R, counts=c.counts, mode=c.mode,
                mask=x["mask"], G=c.G, parts=c.parts)


def _keep_as_mask(keep):
    """the host twin's Philox keep bits as the explicit mask of mode 1"""
    return (keep > 0).astype(np.uint8).reshape(keep.shape[0], -1) if keep.ndim == 4 else (keep > 0).astype(np.uint8).reshape(-1)


# ======================================================================================================================
# scores
@pytest.mark.parametrize("c", K.SCORE_CASES, ids=lambda c: c.name)
def test_scores_against_float64_and_dec_ctx_to_the_bit(c):
    x = K.score_inputs(c)
    kw = _score_kw(c, x)
    got = run_scores(**kw)
    _same(got, run_scores(**kw), (c.name, "two runs differ"))
    if c.live == 0:
        assert _untouched(got[0]) and _untouched(got[1]), (c.name, "a dead step wrote")
        return
    assert np.array_equal(got[1], x["dec"]), (c.name, "dec_ctx_out is not slab 0 + slab 1 + ... + b_dec in fp32")
    ref, bound = K.scores_ref(c, x)
    frac = _within("att_scores" + ("", "_group", "_group_train")[c.route], (c.name, "scores"), got[0], ref, bound)
    assert np.array_equal(run_scores(**dict(kw, want_dec=False))[0], got[0]), (c.name, "scores depend on dec_ctx_out")
    for parts in (1, 4, 7):
        if parts != (c.parts or 4):
            assert np.array_equal(run_scores(**dict(kw, parts=parts))[0], got[0]), (c.name, "scores depend on parts", parts)
    if c.mode == 2:          # Philox = the explicit mask of its host twin (keep3 lays the flags out by row; the mask starts at row0)
        flags = (x["keep"][c.row0:] > 0).astype(np.uint8).reshape(-1)
        _same(got, run_scores(**dict(kw, mode=1, mask=flags)), (c.name, "Philox is not its host twin"))
    if c.route:              # a grouped kernel = the per-row kernel on the same rows
        per_row = run_scores(**dict(kw, route=0, G=0, img=K.images(c)))
        _same(got, per_row, (c.name, "the grouped kernel differs from the per-row kernel"))
    if c.counts is not None and c.route == 0 and c.mode < 2 and c.img is None:
        for mode in (0, c.mode):         # an image of c <= 64 regions under <true> = <false> alone at R = c
            whole = run_scores(**dict(kw, mode=mode)) if mode != c.mode else got
            for row, n in enumerate(c.counts):
                if n <= 64:
                    m = None if mode == 0 else np.ascontiguousarray(x["mask"].reshape(c.rows, c.R, c.A)[row, :n]).reshape(-1)
                    alone = run_scores(0, x["enc"][row:row + 1, :n], None, x["slab"][:, row:row + 1], x["b_dec"], x["w"], x["b_aff"], n, None, mode, m, 0,
                                       None, 0, c.parts)
                    assert np.array_equal(alone[0][0], whole[0][row, :n]) and np.array_equal(alone[1][0], whole[1][row]), (c.name, row, n, mode)
    print("scores %s: worst error / bound %.3g" % (c.name, frac))


# ======================================================================================================================
# softmax and context
@pytest.mark.parametrize("c", K.CTX_CASES, ids=lambda c: c.name)
def test_alpha_and_context_against_float64(c):
    x = K.ctx_inputs(c)
    kw = dict(feats=x["feats"], img=c.img, scores=x["scores"], R=c.R, counts=c.counts, G=c.G, alpha2=c.alpha2, live=c.live)
    al, cx, a2 = got = run_ctx(**kw)
    _same(got, run_ctx(**kw), (c.name, "two runs differ"))
    if c.live == 0:
        assert _untouched(al) and _untouched(cx) and _untouched(a2), (c.name, "a dead step wrote")
        return
    ral, balpha, rcx, bcx = K.ctx_ref(c, x)
    kernel = "att_ctx_group" if c.G else "att_ctx"
    frac = max(_within(kernel, (c.name, "alpha"), al, ral, balpha), _within(kernel, (c.name, "ctx"), cx, rcx, bcx))
    sums = al.astype(np.float64).sum(1)
    assert (np.abs(sums - 1.0) <= 4 * 2.0 ** -23).all(), (c.name, "alpha rows do not sum to 1 within 4 ulps", sums)
    if c.alpha2:
        assert np.array_equal(a2[:, :c.R], al) and _untouched(a2[:, c.R:]), (c.name, "alpha_out2")
    else:
        assert _untouched(a2)
    if c.G:
        _same(got[:2], run_ctx(**dict(kw, G=0, img=K.images(c)))[:2], (c.name, "the grouped kernel differs from the per-row kernel"))
    if c.counts is not None and not c.G and c.img is None:
        for row, n in enumerate(c.counts):
            if n <= 64:
                alone = run_ctx(x["feats"][row:row + 1, :n], None, x["scores"][row:row + 1, :n], n, None, 0, False, None)
                assert np.array_equal(alone[0][0], al[row, :n]) and np.array_equal(alone[1][0], cx[row]), (c.name, row, n, "<true> is not <false> at R = c")
    print("ctx %s: worst error / bound %.3g" % (c.name, frac))


# ======================================================================================================================
# mean and saved alphas
@pytest.mark.parametrize("c", K.MEAN_CASES, ids=lambda c: c.name)
def test_mean_against_float64_and_counted_equals_plain(c):
    from simpleimagecaptionzoo_amd.butd_att_kernels import entry_att_mean
    feats = K.mean_inputs(c)

    def run(f, R, counts):
        out = Laid([f.shape[0] * c.D])
        entry_att_mean(_dev(f), f.shape[0], R, c.D, out.views[0], counts=_i32(counts))
        return _np(out.take()[0], (f.shape[0], c.D))
    got = run(feats, c.R, c.counts)
    assert np.array_equal(got, run(feats, c.R, c.counts)), (c.name, "two runs differ")
    ref, bound = K.mean_ref(c, feats)
    frac = _within("mean_feats_counts" if c.counts else "mean_feats", c.name, got, ref, bound)
    for i, n in enumerate(c.counts or ()):
        assert np.array_equal(run(feats[i:i + 1, :n], n, None)[0], got[i]), (c.name, i, "the counted mean is not the plain mean at R = c")
    print("mean %s: worst error / bound %.3g" % (c.name, frac))


@pytest.mark.parametrize("c", K.SAVED_CASES, ids=lambda c: c.name)
def test_saved_alphas_is_the_fp32_mean_in_head_order(c):
    from simpleimagecaptionzoo_amd.butd_att_kernels import entry_att_saved_alphas
    src = np.abs(K.seeded("saved " + c.name).standard_normal((c.T, c.B, c.NH, c.R))).astype(np.float32)
    out = Laid([c.B * c.T * c.R])
    entry_att_saved_alphas(_dev(src), c.T, c.B, c.NH, c.R, out.views[0])
    got = _np(out.take()[0], (c.B, c.T, c.R))
    assert np.array_equal(got, K.saved_alphas_twin(src)), c.name
    _worst.setdefault("saved_alphas", 0.0)


# ======================================================================================================================
# d alpha
@pytest.mark.parametrize("c", K.DALPHA_CASES, ids=lambda c: c.name)
def test_dalpha_parts_against_float64(c):
    x = K.dalpha_inputs(c)
    kw = dict(slab=x["slab"], feats=x["feats"], img=c.img, R=c.R, D=c.D, counts=c.counts, live=c.live)
    got = run_dalpha(**kw)
    assert np.array_equal(got, run_dalpha(**kw)), (c.name, "two runs differ")
    if c.live == 0:
        assert _untouched(got), (c.name, "a dead step wrote")
        return
    ref, bound, written = K.dalpha_ref(c, x)
    assert _untouched(got[~written]), (c.name, "dalpha_part written behind the count")
    g = np.where(written, got, 0.0)
    frac = _within("att_bwd_dalpha", (c.name, "parts"), g, ref, bound)
    frac = max(frac, _within("att_bwd_dalpha", (c.name, "parts summed"), g.astype(np.float64).sum(1), ref.sum(1), bound.sum(1)))
    if c.counts is not None and c.img is None:
        for row, n in enumerate(c.counts):
            if n <= 64:
                alone = run_dalpha(x["slab"][:, row:row + 1], x["feats"][row:row + 1, :n], None, n, c.D, None, None)
                assert np.array_equal(alone[0], got[row, :, :n]), (c.name, row, n, "<true> is not <false> at R = c")
    print("dalpha %s: worst error / bound %.3g" % (c.name, frac))


# ======================================================================================================================
# d dec
@pytest.mark.parametrize("c", K.DDEC_CASES, ids=lambda c: c.name)
def test_ds_and_ddec_against_float64(c):
    x = K.ddec_inputs(c)
    kw = dict(enc=x["enc"], img=c.img, dec=x["dec"], w=x["w"], alpha=x["alpha"], parts=x["parts"], R=c.R, counts=c.counts, mode=c.mode, mask=x["mask"],
              live=c.live)
    ds, dd = got = run_ddec(**kw)
    _same(got, run_ddec(**kw), (c.name, "two runs differ"))
    if c.live == 0:
        assert not ds.any() and not dd.any(), (c.name, "the ds and ddec rows of a dead step are zeros")
        return
    rds, bds, rdd, bdd = K.ddec_ref(c, x)
    frac = max(_within("att_bwd_ddec", (c.name, "ds"), ds, rds, bds), _within("att_bwd_ddec", (c.name, "ddec"), dd, rdd, bdd))
    if c.mode == 2:
        _same(got, run_ddec(**dict(kw, mode=1, mask=_keep_as_mask(x["keep"]))), (c.name, "Philox is not its host twin"))
    if c.counts is not None and c.mode < 2 and c.img is None:
        for mode in (0, c.mode):
            whole = run_ddec(**dict(kw, mode=mode)) if mode != c.mode else got
            for row, n in enumerate(c.counts):
                if n <= 64:
                    m = None if mode == 0 else np.ascontiguousarray(x["mask"].reshape(c.rows, c.R, c.A)[row, :n]).reshape(-1)
                    alone = run_ddec(x["enc"][row:row + 1, :n], None, x["dec"][row:row + 1], x["w"], x["alpha"][row:row + 1, :n],
                                     x["parts"][row:row + 1, :, :n], n, None, mode, m, None)
                    assert np.array_equal(alone[0][0], whole[0][row, :n]) and np.array_equal(alone[1][0], whole[1][row]), (c.name, row, n, mode)
    print("ddec %s: worst error / bound %.3g" % (c.name, frac))


# ======================================================================================================================
# d enc_ctx
@pytest.mark.parametrize("c", K.DENC_CASES, ids=lambda c: c.name)
def test_denc_and_dwaff_parts_against_float64(c):
    from simpleimagecaptionzoo_amd.butd import rowgroup_sum
    x = K.denc_inputs(c)
    kw = _denc_kw(c, x)
    de, dw, parts = got = run_denc(**kw)
    _same(got[:2], run_denc(**kw)[:2], (c.name, "two runs differ"))
    assert parts == K.denc_parts(c)
    rde, bde, rdw, bdw = K.denc_ref(c, x, parts)
    kernel = "att_bwd_denc_group" if c.G else "att_bwd_denc"
    if c.G:
        rde, bde = K.group_fold(rde, bde, c.G)
        rdw, bdw = K.group_fold(rdw, bdw, c.G)
    frac = max(_within(kernel, (c.name, "denc"), de, rde, bde), _within(kernel, (c.name, "dwaff_part"), dw, rdw, bdw))
    frac = max(frac, _within(kernel, (c.name, "dwaff column sum"), dw.astype(np.float64).sum((0, 1)), rdw.sum((0, 1)), bdw.sum((0, 1))))
    if c.mode == 2:
        _same(got[:2], run_denc(**dict(kw, mode=1, mask=_keep_as_mask(x["keep"])))[:2], (c.name, "Philox is not its host twin"))
    if not c.G:
        for p in (1, 4):
            if p != parts:
                assert np.array_equal(run_denc(**dict(kw, parts=p))[0], de), (c.name, "denc depends on parts", p)
    else:                    # the grouped kernel = the per-row kernel, then the G rows of an image added in k order
        row_de, row_dw, row_parts = run_denc(**dict(kw, G=0, parts=c.parts, img=K.images(c)))
        n_img = c.B // c.G

        def fold(a):
            out = Laid([a.size // c.G])
            rowgroup_sum(_dev(a), n_img, c.G, a.size // c.B, out.views[0])
            return _np(out.take()[0], (n_img,) + a.shape[1:])
        assert np.array_equal(fold(row_de), de), (c.name, "grouped denc is not the per-row kernel's, summed in k order")
        if row_parts == parts:
            assert np.array_equal(fold(row_dw), dw), (c.name, "grouped dwaff_part is not the per-row kernel's, summed in k order")
    if c.counts is not None and c.mode < 2 and not c.G and c.img is None:
        for mode in (0, c.mode):
            whole = run_denc(**dict(kw, mode=mode)) if mode != c.mode else got
            for row, n in enumerate(c.counts):
                if n <= 64:
                    m = None if mode == 0 else np.ascontiguousarray(x["mask"].reshape(c.T, c.B, c.R, c.A)[:, row, :n]).reshape(c.T, -1)
                    o = x["off"] + row
                    alone = run_denc(x["enc"][row:row + 1, :n], None, x["dec_all"][:, o:o + 1], np.ascontiguousarray(x["ds_all"][:, o:o + 1, :n]), 0, x["w"],
                                     1, n, None, mode, m, 0, parts)
                    assert np.array_equal(alone[0][0], whole[0][row, :n]) and np.array_equal(alone[1][0], whole[1][row]), (c.name, row, n, mode)
    print("denc %s (%d parts): worst error / bound %.3g" % (c.name, parts, frac))


# ======================================================================================================================
# refused calls
def test_refused_calls_launch_nothing():
    """ICZ_ERR_INVALID, and every output as the guards left it"""
    from simpleimagecaptionzoo_amd import butd_att_kernels as E
    from simpleimagecaptionzoo_amd._lib import IczError
    out = Laid([4096, 4096])
    a, b = out.views
    src = _dev(np.zeros(1 << 16))
    cnt_bad, img_bad = _i32([5, 0]), _i32([0, 2])
    sc = dict(enc_ctx=src, n_img=2, dec_slab=src, nsplit=1, b_dec=src, w_aff=src, b_aff=src, dec_ctx_out=b, scores=a, rows=2, R=5, A=8)
    dd = dict(enc_ctx=src, n_img=2, dec_ctx=src, w_aff=src, alpha=src, dalpha=src, ddec=a, ds_out=b, rows=2, R=5, A=8, nparts=1)
    de = dict(enc_ctx=src, n_img=2, dec_all=src, ds_all=src, w_aff=src, denc=a, dwaff_part=b, B=2, R=5, A=8, T=2, mode=0)
    calls = [
        lambda: E.entry_att_scores(0, **dict(sc, A=6)),                          # a width that is no multiple of 4
        lambda: E.entry_att_scores(0, **dict(sc, R=129)),                        # R > ATT_MAX_R
        lambda: E.entry_att_scores(1, G=9, **dict(sc, rows=18, n_img=2)),        # G > ATT_CTX_MAX_G
        lambda: E.entry_att_scores(1, G=8, **dict(sc, rows=16, A=2048)),         # a grouped request above its LDS limit
        lambda: E.entry_att_scores(1, G=2, **dict(sc, rows=3)),                  # rows that are not whole groups
        lambda: E.entry_att_scores(2, G=2, drop=E.drop(1, mask=src, row0=1), **dict(sc, rows=4)),
        lambda: E.entry_att_scores(0, **dict(sc, nsplit=0)),
        lambda: E.entry_att_scores(0, **dict(sc, counts=cnt_bad)),               # a count of 0
        lambda: E.entry_att_scores(0, **dict(sc, img_of_row=img_bad)),           # an image that does not exist
        lambda: E.entry_att_scores(0, **dict(sc, rows=3)),                       # more rows than images without img_of_row
        lambda: E.entry_att_scores(0, **dict(sc, dec_slab=src[1:])),             # not 16-byte aligned
        lambda: E.entry_att_ctx(src, 2, src, a, b, 2, 5, 6),
        lambda: E.entry_att_ctx(src, 2, src, a, b, 2, 5, 8, G=9),
        lambda: E.entry_att_ctx(src, 2, src, a, b, 2, 5, 8, alpha_out2=a, alpha2_stride=4),
        lambda: E.entry_att_ctx(src, 2, src, a, b, 2, 5, 8, G=2, alpha_out2=a, alpha2_stride=5),
        lambda: E.entry_att_ctx(src, 2, src, a, b, 2, 5, 8, counts=cnt_bad),
        lambda: E.entry_att_mean(src, 2, 0, 8, a),
        lambda: E.entry_att_mean(src, 2, 5, 8, a, counts=cnt_bad),
        lambda: E.entry_att_saved_alphas(src, 0, 2, 1, 5, a),
        lambda: E.entry_att_bwd_dalpha(src, 1, 4, 2, src, 2, 5, 8, a),           # ldc < D
        lambda: E.entry_att_bwd_dalpha(src, 33, 8, 2, src, 2, 5, 8, a),
        lambda: E.entry_att_bwd_dalpha(src, 1, 8, 2, src, 2, 5, 8, a, img_of_row=img_bad),
        lambda: E.entry_att_bwd_ddec(**dict(dd, nparts=0)),
        lambda: E.entry_att_bwd_ddec(drop=E.drop(1, mask=src, row0=1), **dd),
        lambda: E.entry_att_bwd_ddec(**dict(dd, ds_out=None)),
        lambda: E.entry_att_bwd_denc(**dict(de, T=0)),
        lambda: E.entry_att_bwd_denc(**dict(de, Bs=1)),
        lambda: E.entry_att_bwd_denc(**dict(de, mode=1)),                        # mode 1 without keep flags
        lambda: E.entry_att_bwd_denc(G=2, parts=1, **dict(de, R=17)),            # parts that do not cover R
        lambda: E.entry_att_bwd_denc(G=2, **dict(de, B=3)),
        lambda: E.entry_att_bwd_denc(**dict(de, counts=cnt_bad)),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(IczError, match="status -1"):
            call()
        torch.cuda.synchronize()
        assert torch.all(out.buf == K.GUARD).item(), (i, "a refused call wrote")


def test_zz_report():
    """the largest error / bound per kernel over this file's tests (DESIGN.md section 3 quotes them)"""
    for k in sorted(_worst):
        print("butd attention kernels: %-24s worst error / bound %.3f" % (k, _worst[k]))
        assert _worst[k] <= 1.0
