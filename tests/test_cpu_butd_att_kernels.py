"""Host-side half of the BUTD attention kernels' own tests (tests/_butd_att_kernels.py; the device half is
tests/test_gpu_butd_att_kernels.py): the constants the case tables assume are the ones in the source; every case is there for what its
tags say, recomputed from its shape and those constants, and every value the tables must contain occurs; every float64 reference
equals a scalar loop; the chain of the references (scores, softmax and context, d alpha, d s and d dec, d enc_ctx and d w_aff) equals
torch.autograd in float64 on oracle.butd's soft attention at the same inputs and explicit masks; the keep-bit helper equals
tests/_philox.py; and the entries refuse bad arguments on the host, before anything touches a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _butd_att_kernels as K
from _philox import RNG_ATT, _keep_bits, butd_rng_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simpleimagecaptionzoo_amd", "csrc")


def _source_constants():
    kern = open(os.path.join(CSRC, "butd_kernels.h")).read()
    impl = open(os.path.join(CSRC, "butd_impl.h")).read()

    def one(src, name):
        vals = set(re.findall(r"constexpr int %s = (\d+);" % name, src))
        assert len(vals) == 1, (name, vals)          # (RB is declared by three kernels: the table takes one value for all)
        return int(vals.pop())
    out = {n: one(kern, n) for n in ("NB", "RB", "NR", "DALPHA_COLS", "DENC_GROUP_REGS", "ATT_CTX_MAX_G", "ATT_MAX_R")}
    out["ATT_PARTS"] = one(impl, "ATT_PARTS")
    out["TT"] = one(impl, "ATT_DENC_TT")
    return out


def test_the_tables_assume_the_constants_of_the_source():
    src = _source_constants()
    assert src == K.CONST, {k: (src[k], K.CONST[k]) for k in src if src[k] != K.CONST[k]}
    impl = open(os.path.join(CSRC, "butd_impl.h")).read()
    assert "att_bwd_denc_kernel<ATT_DENC_TT, true>" in impl and "att_bwd_denc_group_kernel<ATT_DENC_TT, true>" in impl


@pytest.mark.parametrize("table", sorted(K.ALL_CASES))
def test_every_case_is_there_for_what_it_says(table):
    src = _source_constants()
    cases = K.ALL_CASES[table]
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.tags, (c.name, "a case without a purpose")
        for t in c.tags:
            assert K.TAGS[t](c, src), (table, c.name, t)

    def holds(t, c):
        try:
            return bool(K.TAGS[t](c, src))
        except (AttributeError, TypeError):
            return False
    for t in {t for c in cases for t in c.tags}:         # and is no empty word: some case of the table is on its other side
        assert [c.name for c in cases if not holds(t, c)], (table, t, "true of every case")
    for field, vals in K.REQUIRED[table]:
        have = {getattr(c, field) for c in cases} | ({src["ATT_PARTS"]} if field == "parts" else set())
        assert set(vals) <= have, (table, field, sorted(set(vals) - have))
    for c in cases:                                      # shapes the entries take, and small
        assert c.R <= src["ATT_MAX_R"] and (c.counts is None or (len(c.counts) == c.n_img and all(1 <= n <= c.R for n in c.counts)))
        assert c.counts is not None or c.R <= 64 or "adaptive" in c.tags
        if c.img is not None:
            assert len(c.img) == (c.B if table == "denc" else c.rows) and all(0 <= i < c.n_img for i in c.img)


def test_counted_cases_cover_both_sides_of_64_and_the_dead_step_every_kernel():
    assert set(K.AD_COUNTS) >= {1, 63, 64, 65, 100, 128}
    for table in ("scores", "ctx", "dalpha", "ddec"):
        assert [c for c in K.ALL_CASES[table] if c.live == 0], table
        assert [c for c in K.ALL_CASES[table] if c.counts and min(c.counts) <= 64 < max(c.counts)], table
    assert [c for c in K.SCORE_CASES if c.route == 2 and c.live == 0] and [c for c in K.CTX_CASES if c.G and c.live == 0]
    assert {c.mode for c in K.SCORE_CASES if c.route == 2 and c.G >= 2} == {0, 1, 2}
    assert [c for c in K.DENC_CASES if c.G and c.counts and K.denc_parts(c) > K.CONST["ATT_PARTS"]]
    assert {(n.R, n.D) for n in K.MEAN_CASES if n.counts is None} == {(R, D) for R in (1, 36, 64) for D in (4, 516)}
    assert {(n.NH, n.R) for n in K.SAVED_CASES} == {(NH, R) for NH in (1, 8) for R in (1, 36, 64)}


def test_inputs_hold_zeros_of_both_signs_and_about_half_of_the_relus_are_on():
    for c in (K.SCORE_CASES[4], K.DDEC_CASES[7], K.DENC_CASES[5]):
        x = K.score_inputs(c) if hasattr(c, "nsplit") else K.ddec_inputs(c) if hasattr(c, "nparts") else K.denc_inputs(c)
        dec = x["dec"] if "dec" in x else x["dec_all"][0, x["off"]:]
        z = (x["enc"][0] + dec[0][None]).astype(np.float32)
        assert (z == 0).any() and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all(), c.name
        assert 0.3 < (z > 0).mean() < 0.7, c.name


# ======================================================================================================================
# every reference against a scalar loop
def _close(a, b):
    assert np.allclose(a, b, rtol=1e-12, atol=1e-15), np.abs(np.asarray(a) - np.asarray(b)).max()


def _g(k):
    return 1.0 if k < 0 else (2.0 if k > 0 else 0.0)


SMALL_SCORES = [K._sc("loop", (), A=8, mode=1, nsplit=3), K._sc("loop_ad", (), rows=3, n_img=2, R=70, A=4, counts=(3, 66), img=(1, 0, 1), mode=2, row0=1)]


@pytest.mark.parametrize("c", SMALL_SCORES, ids=lambda c: c.name)
def test_scores_reference_is_the_scalar_loop(c):
    x = K.score_inputs(c)
    ref, _ = K.scores_ref(c, x)
    for row, img in enumerate(K.images(c)):
        for a in range(c.A):                              # the fp32 twin of dec_ctx: additions in slab order, then the bias
            s = x["slab"][0, row, a]
            for z in range(1, c.nsplit):
                s = np.float32(s + x["slab"][z, row, a])
            assert np.float32(s + x["b_dec"][a]) == x["dec"][row, a]
        for r in range(c.R):
            if r >= K.count_of(c, img):
                assert ref[row, r] == 0
                continue
            s = 0.0
            for a in range(c.A):
                s += float(x["w"][a]) * _g(x["keep"][row, r, a]) * max(float(x["enc"][img, r, a]) + float(x["dec"][row, a]), 0.0)
            _close(ref[row, r], s + float(x["b_aff"][0]))
    assert (x["keep"][:c.row0] == -1).all() and (x["keep"][c.row0:] >= 0).all()


@pytest.mark.parametrize("c", [K._cc("loop", (), R=5, D=8), K._cc("loop_ad", (), rows=3, n_img=2, R=70, D=4, counts=(1, 66), img=(1, 0, 1))], ids=lambda c: c.name)
def test_context_reference_is_the_scalar_loop(c):
    x = K.ctx_inputs(c)
    al, _, cx, _ = K.ctx_ref(c, x)
    for row, img in enumerate(K.images(c)):
        n = K.count_of(c, img)
        s = [float(v) for v in x["scores"][row, :n]]
        e = [math.exp(v - max(s)) for v in s]
        for r in range(c.R):
            _close(al[row, r], e[r] / sum(e) if r < n else 0.0)
        for d in range(c.D):
            _close(cx[row, d], sum(e[r] / sum(e) * float(x["feats"][img, r, d]) for r in range(n)))


def test_mean_and_saved_alphas_references_are_the_scalar_loops():
    c = K.MeanCase("loop", 2, 5, 4, (5, 2))
    f = K.mean_inputs(c)
    ref, _ = K.mean_ref(c, f)
    for i in range(2):
        for d in range(4):
            _close(ref[i, d], sum(float(f[i, r, d]) for r in range(c.counts[i])) / c.counts[i])
    src = K.seeded("saved loop").standard_normal((3, 2, 4, 5)).astype(np.float32)
    out = K.saved_alphas_twin(src)
    for b in range(2):
        for t in range(3):
            for r in range(5):
                s = np.float32(0)
                for h in range(4):
                    s = np.float32(s + src[t, b, h, r])
                assert out[b, t, r] == np.float32(s / np.float32(4))


@pytest.mark.parametrize("c", [K._dac("loop", (), R=3, D=516, ns=2), K._dac("loop_ad", (), rows=3, n_img=2, R=70, D=8, counts=(2, 66), img=(1, 0, 1))],
                         ids=lambda c: c.name)
def test_dalpha_reference_is_the_scalar_loop(c):
    x = K.dalpha_inputs(c)
    ref, _, written = K.dalpha_ref(c, x)
    for row, img in enumerate(K.images(c)):
        for r in range(c.R):
            for p in range(ref.shape[1]):
                assert written[row, p, r] == (r < K.count_of(c, img))
                if written[row, p, r]:
                    s = 0.0
                    for d in range(512 * p, min(c.D, 512 * p + 512)):
                        s += sum(float(x["slab"][z, row, d]) for z in range(c.ns)) * float(x["feats"][img, r, d])
                    _close(ref[row, p, r], s)
    assert np.isnan(x["slab"][..., c.D:]).all() and x["ldc"] == c.D + K.DCTX_PAD


@pytest.mark.parametrize("c", [K._ddc("loop", (), R=5, A=8, nparts=2, mode=1), K._ddc("loop_ad", (), rows=3, n_img=2, R=70, A=4, counts=(1, 66), img=(1, 0, 1), mode=2)],
                         ids=lambda c: c.name)
def test_ds_and_ddec_references_are_the_scalar_loops(c):
    x = K.ddec_inputs(c)
    ds, _, dd, _ = K.ddec_ref(c, x)
    sc = 2.0 if c.mode else 1.0
    for row, img in enumerate(K.images(c)):
        n = K.count_of(c, img)
        da = [sum(float(x["parts"][row, p, r]) for p in range(c.nparts)) for r in range(n)]
        al = [float(v) for v in x["alpha"][row, :n]]
        dot = sum(a * d for a, d in zip(al, da))
        for r in range(c.R):
            _close(ds[row, r], al[r] * (da[r] - dot) if r < n and n > 1 else 0.0)
        for a in range(c.A):
            s = 0.0
            for r in range(n):
                on = np.float32(x["enc"][img, r, a] + x["dec"][row, a]) > 0 and x["keep"][row, r, a] != 0
                s += ds[row, r] * float(x["w"][a]) * sc if on else 0.0
            _close(dd[row, a], s)


@pytest.mark.parametrize("c", [K._dec("loop", (), R=5, A=8, T=3, mode=1, bs2=True), K._dec("loop_ad", (), B=3, n_img=2, R=70, A=4, T=2, counts=(2, 66), img=(1, 0, 1), mode=2),
                               K._dec("loop_g", (), B=4, n_img=2, G=2, R=5, A=4, T=2, mode=0)], ids=lambda c: c.name)
def test_denc_and_dwaff_references_are_the_scalar_loops(c):
    x = K.denc_inputs(c)
    parts = K.denc_parts(c)
    de, deb, dw, dwb = K.denc_ref(c, x, parts)
    sc = 2.0 if c.mode else 1.0
    loop_dw = np.zeros_like(dw)
    for row, img in enumerate(K.images(c)):
        for r in range(c.R):
            for a in range(c.A):
                s = 0.0
                if r < K.count_of(c, img):
                    for t in range(c.T):
                        zp = np.float32(x["enc"][img, r, a] + x["dec_all"][t, x["off"] + row, a])
                        if zp > 0 and x["keep"][t, row, r, a] != 0:
                            dst = float(x["ds_all"][t, x["off"] + row, r])
                            s += dst * float(x["w"][a]) * sc
                            loop_dw[row, r % parts, a] += float(zp) * sc * dst
                _close(de[row, r, a], s)
    _close(dw, loop_dw)
    if c.G:
        f, _ = K.group_fold(de, deb, c.G)
        _close(f[1], de[2] + de[3])


# ======================================================================================================================
# the chain of the references against torch.autograd on the oracle's soft attention
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_chained_references_equal_autograd_on_the_oracles_soft_attention(train):
    from oracle import butd as ob
    B, R, A, D, T = 3, 7, 12, 8, 3
    mode = 1 if train else 0
    ce = K._dec("chain", (), B=B, n_img=B, R=R, A=A, T=T, mode=mode)
    x = K.denc_inputs(ce)
    rs = K.seeded("chain")
    feats = rs.standard_normal((B, R, D)).astype(np.float32)
    dctx = rs.standard_normal((T, B, D)).astype(np.float32)
    b_aff = K.f32([0.37])
    ds_all = np.zeros((T, B, R), dtype=np.float32)
    ddec = np.zeros((T, B, A))
    for t in range(T):
        cs = K._sc("chain", (), rows=B, n_img=B, R=R, A=A, mode=mode)
        scores, _ = K.scores_ref(cs, dict(enc=x["enc"], dec=x["dec_all"][t], w=x["w"], b_aff=b_aff, keep=x["keep"][t]))
        cc = K._cc("chain", (), rows=B, n_img=B, R=R, D=D)
        alpha, _, _, _ = K.ctx_ref(cc, dict(feats=feats, scores=scores.astype(np.float32)))
        cd = K._dac("chain", (), rows=B, n_img=B, R=R, D=D, ns=1)
        parts, _, _ = K.dalpha_ref(cd, dict(slab=dctx[t][None], feats=feats))
        cdd = K._ddc("chain", (), rows=B, n_img=B, R=R, A=A, nparts=parts.shape[1], mode=mode)
        ds, _, ddec[t], _ = K.ddec_ref(cdd, dict(enc=x["enc"], dec=x["dec_all"][t], w=x["w"], alpha=alpha.astype(np.float32), parts=parts.astype(np.float32),
                                                 keep=x["keep"][t]))
        ds_all[t] = ds.astype(np.float32)
    denc, _, dwp, _ = K.denc_ref(ce, dict(x, ds_all=ds_all), K.denc_parts(ce))

    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))          # noqa: E731
    enc_t, w_t = f64(x["enc"]).requires_grad_(), f64(x["w"]).requires_grad_()
    dec_t = f64(x["dec_all"]).requires_grad_()
    p = {"atten.dec_att.bias": torch.zeros(A, dtype=torch.float64), "atten.affine.bias": f64(b_aff)}
    pre = {"w": {"atten.dec_att": torch.eye(A, dtype=torch.float64), "atten.affine": w_t.view(1, A)}, "enc_ctx": enc_t}
    loss = 0.0
    for t in range(T):
        mask = torch.tensor((x["keep"][t] > 0).astype(np.float64)) if train else None
        ctx, _ = ob.soft_attention(f64(feats), dec_t[t], p, att_mask=mask, pre=pre)
        loss = loss + (ctx * f64(dctx[t])).sum()
    loss.backward()
    for name, mine, theirs in (("d enc_ctx", denc, enc_t.grad), ("d dec", ddec, dec_t.grad), ("d w_aff", dwp.sum((0, 1)), w_t.grad)):
        theirs = theirs.numpy()
        assert np.allclose(mine, theirs, rtol=1e-5, atol=1e-6 * np.abs(theirs).max()), (name, np.abs(mine - theirs).max())


# ======================================================================================================================
# keep bits
def test_keep_helper_is_the_philox_twin():
    rows, R, A, row0 = 4, 3, 132, 1
    k = K.keep3(2, row0, rows, R, A, None, K.STEP)
    bits = _keep_bits(K.SEED, RNG_ATT, K.STEP, rows * R * A).reshape(rows, R, A)
    assert (k[:row0] == -1).all() and np.array_equal(k[row0:], bits[:rows - row0].astype(np.int8))
    T, B = 3, 2
    am = butd_rng_arrays(K.SEED, T, B, R, 4, A, 4)[2]
    assert np.array_equal(np.stack([K.keep3(2, 0, B, R, A, None, t) for t in range(T)]), am.astype(np.int8))
    mask = np.array([0, 1, 2, 255] * 3, dtype=np.uint8)
    assert K.keep3(1, 0, 1, 3, 4, mask, 0).reshape(-1).tolist() == [0, 1, 1, 1] * 3
    assert (K.keep3(0, 0, 2, 3, 4, None, 0) == -1).all() and K.gain(np.array([-1, 0, 1])).tolist() == [1.0, 0.0, 2.0]


# ======================================================================================================================
# the entries refuse on the host
FAKE = 0x1000                       # a 16-byte aligned non-null address that a refused call never reads


class P:                            # stands for a device tensor at a given address
    def __init__(self, a):
        self.a = a

    def data_ptr(self):
        return self.a


def _refused(status, *needles):
    from simpleimagecaptionzoo_amd._lib import lib
    msg = lib().icz_last_error().decode()
    assert status == -1 and all(n in msg for n in needles), (status, msg)


def _vp(a):
    return None if a is None else C.c_void_p(a)


def test_wrappers_name_every_field_of_their_structs():
    from simpleimagecaptionzoo_amd import _lib
    from simpleimagecaptionzoo_amd import butd_att_kernels as E
    for struct, pointers, scalars in ((_lib.AttScoresArgs, _lib.ATT_SCORES_POINTERS, E.ATT_SCORES_SCALARS),
                                      (_lib.AttDdecArgs, _lib.ATT_DDEC_POINTERS, E.ATT_DDEC_SCALARS),
                                      (_lib.AttDencArgs, _lib.ATT_DENC_POINTERS, E.ATT_DENC_SCALARS)):
        fields = dict(struct._fields_)
        assert set(fields) == set(pointers) | set(scalars) and not set(pointers) & set(scalars)
        assert all(fields[n] is C.c_void_p for n in pointers) and all(fields[n] is not C.c_void_p for n in scalars)
    header = open(os.path.join(ROOT, "include", "icz.h")).read()
    for name in ("icz_test_att_mean", "icz_test_att_scores", "icz_test_att_ctx", "icz_test_att_saved_alphas", "icz_test_att_bwd_dalpha",
                 "icz_test_att_bwd_ddec", "icz_test_att_bwd_denc"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(_lib.lib(), name)


def test_attention_entries_refuse_on_the_host():
    from simpleimagecaptionzoo_amd._lib import DropArgs, lib
    from simpleimagecaptionzoo_amd.butd_att_kernels import att_ddec_args, att_denc_args, att_scores_args
    L = lib()
    f = _vp(FAKE)
    who = "icz_test_att_mean"
    _refused(L.icz_test_att_mean(None, 2, 5, 8, None, f, None), who, "null")
    _refused(L.icz_test_att_mean(f, 0, 5, 8, None, f, None), who, "n_img=0")
    _refused(L.icz_test_att_mean(f, 2, 0, 8, None, f, None), who, "R=0")
    _refused(L.icz_test_att_mean(f, 2, 129, 8, None, f, None), who, "R=129", "1..128")
    _refused(L.icz_test_att_mean(f, 2, 5, 6, None, f, None), who, "D=6", "multiple of 4")
    _refused(L.icz_test_att_mean(_vp(FAKE + 4), 2, 5, 8, None, f, None), who, "16-byte")

    who = "icz_test_att_scores"

    def scores(route=0, G=0, parts=0, drop=None, **kw):
        base = {n: P(FAKE) for n in ("enc_ctx", "dec_slab", "b_dec", "w_aff", "b_aff", "dec_ctx_out", "scores")}
        base.update(n_img=2, nsplit=2, rows=2, R=5, A=8)
        base.update(kw)
        a = att_scores_args(**base)
        return L.icz_test_att_scores(route, C.byref(a), None if drop is None else C.byref(drop), G, parts, None)

    _refused(L.icz_test_att_scores(0, None, None, 0, 0, None), who, "null")
    for route in (-1, 3):
        _refused(scores(route), who, "route=%d" % route)
    for n in ("enc_ctx", "dec_slab", "b_dec", "w_aff", "b_aff", "scores"):
        _refused(scores(**{n: None}), who, "null")
    for kw, word in (({"A": 6}, "A=6"), ({"A": 0}, "A=0"), ({"R": 0}, "R=0"), ({"R": 129}, "R=129"), ({"rows": 0}, "rows=0"), ({"rows": 3}, "without img_of_row"),
                     ({"nsplit": 0}, "nsplit=0"), ({"nsplit": 33}, "nsplit=33"), ({"n_img": 0}, "n_img=0"), ({"dec_slab": P(FAKE + 4)}, "16-byte"),
                     ({"dec_ctx_out": P(FAKE + 8)}, "16-byte")):
        _refused(scores(**kw), who, word)
    _refused(scores(parts=-1), who, "parts=-1")
    _refused(scores(G=2), who, "G=2 with the per-row kernel")
    _refused(scores(0, A=16384), who, "LDS")
    for route in (1, 2):
        _refused(scores(route, G=0), who, "G=0")
        _refused(scores(route, G=9, rows=18), who, "G=9")
        _refused(scores(route, G=2, rows=3), who, "rows=3")
        _refused(scores(route, G=2, rows=6), who, "n_img=2")
        _refused(scores(route, G=8, rows=16, A=2048), who, "LDS")
    _refused(scores(2, G=2, rows=4, drop=DropArgs(2, None, FAKE, 0, 0, 1)), who, "row0=1")
    _refused(scores(1, G=2, rows=4, drop=DropArgs(2, None, FAKE, 0, 0, 0)), who, "neither dropout nor live")
    _refused(scores(1, G=2, rows=4, live=P(FAKE)), who, "neither dropout nor live")
    for bad in (DropArgs(3, FAKE, FAKE, 0, 0, 0), DropArgs(1, None, FAKE, 0, 0, 0), DropArgs(2, FAKE, None, 0, 0, 0), DropArgs(1, FAKE + 2, None, 0, 0, 0),
                DropArgs(1, FAKE, None, 0, 0, -1)):
        _refused(scores(drop=bad), who, "dropout")

    who = "icz_test_att_ctx"

    def ctx(feats=FAKE, scores=FAKE, alpha=FAKE, alpha2=None, stride=0, out=FAKE, rows=2, R=5, D=8, G=0, n_img=2):
        return L.icz_test_att_ctx(_vp(feats), n_img, None, _vp(scores), _vp(alpha), _vp(alpha2), stride, _vp(out), rows, R, D, G, None, None, None)
    for kw, word in (({"feats": None}, "null"), ({"scores": None}, "null"), ({"alpha": None}, "null"), ({"out": None}, "null"), ({"D": 6}, "D=6"),
                     ({"R": 129}, "R=129"), ({"rows": 3}, "without img_of_row"), ({"feats": FAKE + 4}, "16-byte"), ({"G": -1}, "G=-1"),
                     ({"G": 9, "rows": 18}, "G=9"), ({"G": 2, "rows": 3}, "rows=3"), ({"G": 2, "alpha2": FAKE, "stride": 5}, "second alpha"),
                     ({"alpha2": FAKE, "stride": 4}, "alpha2_stride=4")):
        _refused(ctx(**kw), who, word)

    who = "icz_test_att_saved_alphas"
    for args in ((None, 1, 1, 1, 1, f), (f, 0, 1, 1, 1, f), (f, 1, 0, 1, 1, f), (f, 1, 1, 0, 1, f), (f, 1, 1, 1, 0, f), (f, 1, 1, 1, 1, None),
                 (f, 1 << 12, 1 << 12, 1, 1 << 8, f)):
        _refused(L.icz_test_att_saved_alphas(*args, None), who)

    who = "icz_test_att_bwd_dalpha"

    def dalpha(dctx=FAKE, ns=2, ldc=16, rows=2, feats=FAKE, n_img=2, R=5, D=8, out=FAKE):
        return L.icz_test_att_bwd_dalpha(_vp(dctx), ns, ldc, rows, _vp(feats), n_img, R, D, _vp(out), None, None, None, None)
    for kw, word in (({"dctx": None}, "null"), ({"out": None}, "null"), ({"ns": 0}, "ns=0"), ({"ns": 33}, "ns=33"), ({"ldc": 4}, "ldc=4"), ({"ldc": 10}, "ldc=10"),
                     ({"D": 6, "ldc": 8}, "D=6"), ({"rows": 3}, "without img_of_row"), ({"R": 129}, "R=129"), ({"dctx": FAKE + 8}, "16-byte")):
        _refused(dalpha(**kw), who, word)

    who = "icz_test_att_bwd_ddec"

    def ddec(drop=None, **kw):
        base = {n: P(FAKE) for n in ("enc_ctx", "dec_ctx", "w_aff", "alpha", "dalpha", "ddec", "ds_out")}
        base.update(n_img=2, rows=2, R=5, A=8, nparts=2)
        base.update(kw)
        a = att_ddec_args(**base)
        return L.icz_test_att_bwd_ddec(C.byref(a), None if drop is None else C.byref(drop), None)
    _refused(L.icz_test_att_bwd_ddec(None, None, None), who, "null")
    for n in ("enc_ctx", "dec_ctx", "w_aff", "alpha", "dalpha", "ddec", "ds_out"):
        _refused(ddec(**{n: None}), who, "null")
    for kw, word in (({"nparts": 0}, "nparts=0"), ({"A": 10}, "A=10"), ({"R": 129}, "R=129"), ({"rows": 3}, "without img_of_row"), ({"ddec": P(FAKE + 4)}, "16-byte")):
        _refused(ddec(**kw), who, word)
    _refused(ddec(drop=DropArgs(2, None, FAKE, 0, 0, 2)), who, "row0=2")
    _refused(ddec(drop=DropArgs(1, FAKE + 1, None, 0, 0, 0)), who, "4-byte aligned")

    who = "icz_test_att_bwd_denc"

    def denc(G=0, parts=0, **kw):
        base = {n: P(FAKE) for n in ("enc_ctx", "dec_all", "ds_all", "w_aff", "denc", "dwaff_part")}
        base.update(n_img=2, B=2, R=5, A=8, T=3, mode=0)
        base.update(kw)
        a = att_denc_args(**base)
        return L.icz_test_att_bwd_denc(C.byref(a), G, parts, None, None)
    _refused(L.icz_test_att_bwd_denc(None, 0, 0, None, None), who, "null")
    for n in ("enc_ctx", "dec_all", "ds_all", "w_aff", "denc", "dwaff_part"):
        _refused(denc(**{n: None}), who, "null")
    for kw, word in (({"T": 0}, "T=0"), ({"T": 200, "R": 128}, "LDS"), ({"Bs": 1}, "Bs=1"), ({"mode": 3}, "mode 3"), ({"mode": 1}, "mode 1"),
                     ({"mode": 1, "mask": P(FAKE + 2), "mask_step": 80}, "mode 1"), ({"mode": 1, "mask": P(FAKE), "mask_step": 82}, "mode 1"),
                     ({"mode": 1, "mask": P(FAKE), "mask_step": 76}, "mode 1"), ({"mode": 2}, "mode 2"), ({"A": 6}, "A=6"), ({"B": 3}, "without img_of_row"),
                     ({"denc": P(FAKE + 4)}, "16-byte")):
        _refused(denc(**kw), who, word)
    _refused(denc(G=-1), who, "G=-1")
    _refused(denc(G=2, B=3, n_img=3), who, "B=3")
    _refused(denc(G=1, B=3, n_img=2), who, "n_img=2")
    _refused(denc(G=2, parts=1, R=17), who, "do not cover R=17")
    _refused(denc(G=2, img_of_row=P(FAKE)), who, "img_of_row")
