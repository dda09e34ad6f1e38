"""The AoA kernels, each on its own through the icz_test_aoa_* entries: layer_norm_kernel in both launch
geometries, mha_self_kernel at any query chunk and mha_self_mfma_kernel, mha_self_bwd_kernel, aoa_dec_attn_kernel and its backward,
aoa_dkv_kernel, aoa_ln_bwd_kernel and aoa_ln_bwd_dense_kernel -- against float64 references of the same fp32 inputs and keep flags,
under the a-priori rounding bounds of tests/_aoa_kernels.py (cases, references and bounds live there; tests/test_cpu_aoa_kernels.py
holds them to their purposes).  No element is excused.

Where the code promises bits, bits are asserted: every case run twice; Philox dropout against the explicit mask of its host twin; a forced
query chunk against another chunk; route 0 against the route it names; P and Pd exactly 0 behind an image's count; P == 1 with one
valid key; Qp_store and dx_out against the fp32 slab sum in slab order; aoa_dkv_kernel at every chunk of (k, t) pairs; a dead step
(live = 0) and a refused call leave every output untouched.
Inputs lie in NaN-fenced buffers (the gaps between slabs and the K / V rows of images that no row attends are NaN), every output between
guards of 7.0.  Each test prints its largest error as a fraction of its bound."""
import numpy as np
import pytest
import torch

import _aoa_kernels as A
from _aoa_refiner import keep_bits
from test_gpu_support_kernels import PAD, Laid, _fenced

pytestmark = pytest.mark.gpu

NAN = float("nan")
STEP = 3                 # the Philox step of every draw here (a refiner layer / a decoder step)
_worst = {}              # kernel -> largest error / bound seen
_refs = {}               # (kind, case, mask kind) -> reference, computed once


def _within(kernel, what, got, ref, bound):
    """got (fp32 tensor) within `bound` of `ref`, element by element; exactly `ref` where the bound is 0."""
    g = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert np.isfinite(g).all(), (kernel, what, "a value that is not finite: something read outside its operands")
    err = np.abs(g - ref)
    frac = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    _worst[kernel] = max(_worst.get(kernel, 0.0), frac)
    bad = np.argwhere(err > bound)
    assert not len(bad), (kernel, what, "%d elements outside the bound, first at %s: %r vs %r, error / bound %.3g" % (
        len(bad), bad[0].tolist(), g[tuple(bad[0])], ref[tuple(bad[0])], frac))
    return frac


def _vec(a):
    return _fenced(np.asarray(a, dtype=np.float32).reshape(1, -1))


def _i32(v):
    return None if v is None else torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _seed():
    return torch.tensor([A.SEED], dtype=torch.int64, device="cuda")


def _masks(c, draws, keep, stream):
    """mask kind -> (mode, keep flags as the reference reads them, the device mask or None): off, explicit, Philox with its host twin."""
    twin = keep_bits(A.SEED, stream, STEP, draws - c.idx0, A.ATT_P).astype(np.uint8)
    return {"off": (0, None, None), "explicit": (1, keep, torch.from_numpy(keep).cuda()), "philox": (2, twin, None),
            "twin": (1, twin, torch.from_numpy(twin).cuda())}


def _dropp(c, mode, mask_dev, seed, stream):
    from simpleimagecaptionzoo_amd.aoa_kernels import dropp
    return dropp(mode, mask=mask_dev, seed=seed if mode == 2 else None, stream=stream, step=STEP, p=A.ATT_P, idx0=c.idx0)


# =====================================================================================================================
# layer_norm_kernel
def _ln_run(c, dev):
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_layer_norm
    out = Laid([c.rows * c.n, 2 * c.rows])
    entry_layer_norm(c.geometry, dev["x"], dev["g"], dev["b"], out.views[0], c.rows, c.n, out.views[1] if c.stats else None, dev["live"])
    return out.take()


@pytest.mark.parametrize("c", A.LN_CASES, ids=lambda c: c.name)
def test_layer_norm_against_float64(c):
    """y, and (mean, 1 / (std + eps)) where stats are asked for, within the bound; without stats the stats buffer keeps its guard; live = 0
    writes nothing at all; two runs give the same bits."""
    x, g, b = A.ln_inputs(c)
    dev = dict(x=_fenced(x), g=_vec(g), b=_vec(b), live=None if c.live is None else _i32([c.live]))
    y, st = _ln_run(c, dev)
    if c.live == 0:
        assert torch.all(y == A.GUARD).item() and torch.all(st == A.GUARD).item(), "a dead step wrote"
        print("layer_norm %s: nothing written" % c.name)
        return
    ref = A.layer_norm_ref(x, g, b)
    frac = _within("layer_norm", (c.name, "y"), y, *ref["y"])
    if c.stats:
        st = st.view(c.rows, 2)
        frac = max(frac, _within("layer_norm", (c.name, "mean"), st[:, 0], *ref["mean"]), _within("layer_norm", (c.name, "inv"), st[:, 1], *ref["inv"]))
    else:
        assert torch.all(st == A.GUARD).item(), "stats written without being asked for"
    y2, st2 = _ln_run(c, dev)
    assert torch.equal(y, y2) and torch.equal(st.reshape(-1), st2.reshape(-1)), "two runs differ"
    print("layer_norm %s (%s, %d idle waves): worst error / bound %.3g" % (c.name, c.purpose["path"], c.purpose["idle_waves"], frac))


def test_layer_norm_geometries_give_the_same_bits():
    """A row's arithmetic does not depend on the launch geometry: four rows per workgroup and one wave per workgroup agree bit for bit."""
    by = {c.name: c for c in A.LN_CASES}
    for n in A.LN_N:
        c0, c1 = by["g0_n%d" % n], by["g1_n%d" % n]
        x, g, b = A.ln_inputs(c0)
        dev = dict(x=_fenced(x), g=_vec(g), b=_vec(b), live=None)
        assert torch.equal(_ln_run(c0, dev)[0], _ln_run(c1._replace(stats=False), dev)[0]), n


def test_layer_norm_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_layer_norm
    out = Laid([64])
    x = torch.zeros(68, device="cuda")
    for geometry, rows, n, odd in A.LN_REFUSED:
        with pytest.raises(IczError):
            entry_layer_norm(geometry, x[1:] if odd else x, x, x, out.views[0], rows, n)
    torch.cuda.synchronize()
    assert torch.all(out.take()[0] == A.GUARD).item()


# =====================================================================================================================
# refiner self-attention
def _sa_ref(c, kind, qkv, keep):
    key = ("sa", c.name, kind)
    if key not in _refs:
        _refs[key] = A.self_attn_ref(c, qkv, 0 if kind == "off" else 1, keep)
    return _refs[key]


def _sa_run(c, dev, route, qc, drop):
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_self_attn
    out = Laid([dev["rows"] * c.Hd])
    r, q = entry_self_attn(route, dev["qkv"], out.views[0], c.n_img, c.R, c.Hd, c.NH, counts=dev["counts"], qc=qc, drop=drop)
    return out.take()[0], r, q


@pytest.mark.parametrize("c", A.SA_CASES, ids=lambda c: c.name)
def test_self_attention_against_float64(c):
    """Every route the case lists, dropout off / explicit / Philox: within the bound of the float64 reference of the same inputs and keep
    flags; two runs the same bits; Philox the bits of the explicit mask of its twin; route 0 the bits of the route it names; and on route
    1 another query chunk the same bits (a query row's arithmetic does not depend on the chunk it travels in)."""
    from simpleimagecaptionzoo_amd.aoa_kernels import self_attn_route_for
    qkv = A.sa_inputs(c)
    dev = dict(qkv=_fenced(qkv), counts=_i32(c.counts), rows=qkv.shape[0])
    seed = _seed()
    d = c.Hd // c.NH
    qc_lib = self_attn_route_for(c.R, c.Hd, c.NH, False)[1]
    qc_here = c.qc or qc_lib
    qc_other = c.R if A.self_lds(c.R, d, c.R) <= A.LDS_BUDGET and qc_here != c.R else (4 if c.R > 4 else 0)
    masks = _masks(c, A.sa_draws(c), A.sa_keep(c), A.RNG_REF_ATT)
    frac, got = 0.0, {}
    for kind in ("off", "explicit", "philox", "twin"):
        mode, keep, mask_dev = masks[kind]
        drop = _dropp(c, mode, mask_dev, seed, A.RNG_REF_ATT)
        ref, bound = _sa_ref(c, "philox" if kind == "twin" else kind, qkv, keep)
        for route in c.routes:
            o, r, q = _sa_run(c, dev, route, c.qc, drop)
            got[kind, route] = o
            assert r == (c.purpose["route0"] if route == 0 else route) and (r == 2 or q == qc_here), (c.name, route, r, q)
            frac = max(frac, _within("mha_self_mfma" if r == 2 else "mha_self", (c.name, kind, "route", route), o, ref, bound))
            assert torch.equal(o, _sa_run(c, dev, route, c.qc, drop)[0]), (c.name, kind, route, "two runs differ")
        if 0 in c.routes:
            assert torch.equal(got[kind, 0], got[kind, c.purpose["route0"]]), (c.name, kind, "route 0 is not the route it names")
        if qc_other:
            o, r, q = _sa_run(c, dev, 1, qc_other, drop)
            assert (r, q) == (1, qc_other)
            assert torch.equal(o, got[kind, 1]), (c.name, kind, "chunks of %d and of %d query rows differ" % (qc_here, qc_other))
    for route in c.routes:
        assert torch.equal(got["philox", route], got["twin", route]), (c.name, route, "Philox draws differ from their host twin")
        assert not torch.equal(got["philox", route], got["off", route]) or max(A.offsets(c.counts, c.n_img, c.R)[0]) == 1 or c.R == 1
    print("self-attention %s routes %s, chunks of %d and %d: worst error / bound %.3g" % (c.name, c.routes, qc_here, qc_other, frac))


def test_self_attention_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_self_attn
    out = Laid([2 * 128 * 256])
    x = torch.zeros(2 * 129 * 3 * 256 + 4, device="cuda")
    for route, R, Hd, NH, qc in A.SA_REFUSED:
        with pytest.raises(IczError):
            entry_self_attn(route, x, out.views[0], 2, R, Hd, NH, qc=qc)
    for counts in ([36, 0], [37, 5], [-1, 5]):          # read back and checked before anything is launched
        with pytest.raises(IczError):
            entry_self_attn(1, x, out.views[0], 2, 36, 16, 2, counts=_i32(counts))
    with pytest.raises(IczError):                       # heads of 128 columns at 128 regions in one pass: above the LDS budget
        entry_self_attn(1, x, out.views[0], 2, 128, 256, 2, qc=128)
    torch.cuda.synchronize()
    assert torch.all(out.take()[0] == A.GUARD).item()


# =====================================================================================================================
# decoder attention
def _da_ref(c, kind, q, Kd, Vd, keep):
    key = ("da", c.name, kind)
    if key not in _refs:
        _refs[key] = A.dec_attn_ref(c, q, Kd, Vd, 0 if kind == "off" else 1, keep)
    return _refs[key]


def _da_device(c):
    slabs, bias, Kd, Vd = A.da_inputs(c)
    lens, off = A.offsets(c.counts, c.n_img, c.R)
    for i in set(range(c.n_img)) - set(A.da_images(c)):          # images no row attends: nothing may read their rows
        Kd[off[i]:off[i + 1]] = NAN
        Vd[off[i]:off[i + 1]] = NAN
    n = c.rows * c.Hd
    stride = n + A.DA_SLAB_PAD
    qb = torch.full((2 * PAD + c.qns * stride,), NAN, device="cuda")
    for z in range(c.qns):
        qb[PAD + z * stride:PAD + z * stride + n] = torch.from_numpy(slabs[z].reshape(-1)).cuda()
    return dict(host=(slabs, bias, Kd, Vd), qbuf=qb, Qp=qb[PAD:], stride=stride, bias=_vec(bias), Kd=_fenced(Kd), Vd=_fenced(Vd),
                counts=_i32(c.counts), ior=_i32(c.img_of_row), live=None if c.live is None else _i32([c.live]))


def _da_run(c, dev, drop):
    """-> xatt, P, Pd, Qp_store as flat tensors (P / Pd / Qp_store keep their guard where the case does not ask for them)."""
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_dec_attn
    n, m = c.rows * c.Hd, c.rows * c.NH * c.R
    out = Laid([n, m, m, n])
    xatt, P, Pd, store = out.views
    entry_dec_attn(dev["Qp"], dev["Kd"], dev["Vd"], xatt, c.rows, c.n_img, c.R, c.Hd, c.NH, qns=c.qns, q_stride=dev["stride"] if c.qns > 1 else 0,
                   q_bias=dev["bias"] if c.qns > 1 else None, Qp_store=store if c.qns > 1 else None, img_of_row=dev["ior"],
                   P_out=P if c.p_out else None, Pd_out=Pd if c.p_out else None, counts=dev["counts"], drop=drop, live=dev["live"])
    return out.take()


@pytest.mark.parametrize("c", A.DA_CASES, ids=lambda c: c.name)
def test_decoder_attention_against_float64(c):
    """xatt, P and Pd within the bound, dropout off / explicit / Philox; P and Pd exactly 0 behind the image's count, P exactly 1 where the
    image has one region, rows of P summing to 1 within 4 ulps; Qp_store the fp32 slab sum in slab order plus the bias, bit for bit;
    Philox the bits of its twin's explicit mask; two runs the same bits; live = 0 and outputs not asked for stay at their guard."""
    dev = _da_device(c)
    slabs, bias, Kd, Vd = dev["host"]
    q = A.da_query(c, slabs, bias)
    lens, off = A.offsets(c.counts, c.n_img, c.R)
    att = np.array([lens[i] for i in A.da_images(c)])
    behind = torch.from_numpy(np.broadcast_to(np.arange(c.R)[None, None, :] >= att[:, None, None], (c.rows, c.NH, c.R)).copy()).cuda()
    seed = _seed()
    masks = _masks(c, A.da_draws(c), A.da_keep(c), A.RNG_ATT)
    frac, got = 0.0, {}
    for kind in ("off", "explicit", "philox", "twin"):
        mode, keep, mask_dev = masks[kind]
        drop = _dropp(c, mode, mask_dev, seed, A.RNG_ATT)
        outs = _da_run(c, dev, drop)
        got[kind] = outs
        xatt, P, Pd, store = outs
        if c.live == 0:
            assert all(torch.all(o == A.GUARD).item() for o in outs), "a dead step wrote"
            continue
        ref = _da_ref(c, "philox" if kind == "twin" else kind, q, Kd, Vd, keep)
        frac = max(frac, _within("aoa_dec_attn", (c.name, kind, "xatt"), xatt, *ref["xatt"]))
        if c.p_out:
            P, Pd = P.view(c.rows, c.NH, c.R), Pd.view(c.rows, c.NH, c.R)
            frac = max(frac, _within("aoa_dec_attn", (c.name, kind, "P"), P, *ref["P"]), _within("aoa_dec_attn", (c.name, kind, "Pd"), Pd, *ref["Pd"]))
            assert not P[behind].any().item() and not Pd[behind].any().item(), (c.name, kind, "P or Pd behind the count is not exactly 0")
            one = torch.from_numpy(att == 1).cuda()
            assert torch.all(P[one][:, :, 0] == 1.0).item(), (c.name, kind, "one valid key does not give P == 1")
            assert (P.double().sum(2) - 1.0).abs().max().item() <= 8 * A.U, (c.name, kind, "a row of P is more than 4 ulps from 1")
        else:
            assert torch.all(P == A.GUARD).item() and torch.all(Pd == A.GUARD).item(), "P written without being asked for"
        if c.qns > 1:
            assert torch.equal(store.cpu(), torch.from_numpy(q.reshape(-1))), (c.name, kind, "Qp_store is not the slab sum in slab order")
        else:
            assert torch.all(store == A.GUARD).item()
        again = _da_run(c, dev, drop)
        assert all(torch.equal(a, b_) for a, b_ in zip(outs, again)), (c.name, kind, "two runs differ")
    assert all(torch.equal(a, b_) for a, b_ in zip(got["philox"], got["twin"])), (c.name, "Philox draws differ from their host twin")
    if c.live != 0 and c.R > 1:
        assert not torch.equal(got["philox"][0], got["off"][0])
    print("decoder attention %s: worst error / bound %.3g" % (c.name, frac))


def test_decoder_attention_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_dec_attn
    out = Laid([6 * 16])
    x = torch.zeros(4 * 129 * 520 + 4, device="cuda")
    for R, Hd, NH, qns, rows, n_img in A.DA_REFUSED:
        with pytest.raises(IczError):
            entry_dec_attn(x, x, x, out.views[0], rows, n_img, R, Hd, NH, qns=qns)
    for ior in ([0, 1, 3], [0, -1, 2]):                 # a row that decodes an image the batch does not have
        with pytest.raises(IczError):
            entry_dec_attn(x, x, x, out.views[0], 3, 3, 36, 16, 2, img_of_row=_i32(ior))
    with pytest.raises(IczError):
        entry_dec_attn(x, x, x, out.views[0], 3, 3, 36, 16, 2, counts=_i32([36, 0, 5]))
    with pytest.raises(IczError):
        entry_dec_attn(x, x[1:], x, out.views[0], 3, 3, 36, 16, 2)
    torch.cuda.synchronize()
    assert torch.all(out.take()[0] == A.GUARD).item()


# =====================================================================================================================
# aoa_dec_attn_bwd_kernel
@pytest.mark.parametrize("b", A.DB_CASES, ids=lambda b: b.name)
def test_decoder_attention_backward_against_float64(b):
    """dQp and dS within the bound of the analytic float64 backward on the same P, Pd and slabs; dx_out the fp32 slab sum in slab order,
    bit for bit; dS exactly 0 behind the image's count; two runs the same bits; live = 0 writes nothing.  The slabs' columns [Hd, 2 Hd),
    the P / Pd columns behind the count and the K / V rows of images no row attends are NaN."""
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_dec_attn_bwd
    c, q, Kd, Vd, P, Pd, dxq = A.db_inputs(b)
    ks = A.db_keep_scale(b)
    lens, off = A.offsets(c.counts, c.n_img, c.R)
    imgs = A.da_images(c)
    ref = A.dec_attn_bwd_ref(c, q, Kd, Vd, P, Pd, dxq, ks)
    Kn, Vn, Pn, Pdn, dn = Kd.copy(), Vd.copy(), P.copy(), Pd.copy(), dxq.copy()
    for i in set(range(c.n_img)) - set(imgs):
        Kn[off[i]:off[i + 1]] = NAN
        Vn[off[i]:off[i + 1]] = NAN
    for row, i in enumerate(imgs):
        Pn[row, :, lens[i]:] = NAN
        Pdn[row, :, lens[i]:] = NAN
    dn[:, :, c.Hd:] = NAN
    n, m = c.rows * c.Hd, c.rows * c.NH * c.R
    dev = [_fenced(dn.reshape(b.ns * c.rows, -1)), _fenced(Pn.reshape(c.rows, -1)), _fenced(Pdn.reshape(c.rows, -1)), _fenced(q), _fenced(Kn), _fenced(Vn)]
    counts, ior, live = _i32(c.counts), _i32(c.img_of_row), None if c.live is None else _i32([c.live])
    runs = []
    for _ in range(2):
        out = Laid([n, m, n])
        entry_dec_attn_bwd(dev[0], b.ns, c.rows, dev[1], dev[2], dev[3], dev[4], dev[5], out.views[0], out.views[1], out.views[2], c.n_img, c.R, c.Hd,
                           c.NH, counts=counts, keep_scale=ks, live=live, img_of_row=ior)
        runs.append(out.take())
    assert all(torch.equal(x, y) for x, y in zip(*runs)), (b.name, "two runs differ")
    dQp, dS, dx = runs[0]
    if c.live == 0:
        assert all(torch.all(o == A.GUARD).item() for o in runs[0]), "a dead step wrote"
        print("decoder attention backward %s: nothing written" % b.name)
        return
    frac = max(_within("aoa_dec_attn_bwd", (b.name, "dQp"), dQp, *ref["dQp"]), _within("aoa_dec_attn_bwd", (b.name, "dS"), dS, *ref["dS"]))
    assert torch.equal(dx.cpu(), torch.from_numpy(A.db_dx(c, dxq).reshape(-1))), (b.name, "dx_out is not the slab sum in slab order")
    behind = np.broadcast_to(np.arange(c.R)[None, None, :] >= np.array([lens[i] for i in imgs])[:, None, None], (c.rows, c.NH, c.R))
    assert not dS.view(c.rows, c.NH, c.R)[torch.from_numpy(behind.copy()).cuda()].any().item(), (b.name, "dS behind the count is not 0")
    print("decoder attention backward %s: worst error / bound %.3g" % (b.name, frac))


def test_decoder_attention_backward_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_dec_attn_bwd
    out = Laid([6 * 16, 6 * 2 * 36, 6 * 16])
    x = torch.zeros(4 * 129 * 520 + 4, device="cuda")
    for R, Hd, NH, ns, rows, n_img, ks in A.DB_REFUSED:
        with pytest.raises(IczError):
            entry_dec_attn_bwd(x, ns, rows, x, x, x, x, x, *out.views, n_img, R, Hd, NH, keep_scale=ks)
    with pytest.raises(IczError):
        entry_dec_attn_bwd(x, 1, 3, x, x, x, x, x, *out.views, 3, 36, 16, 2, img_of_row=_i32([0, 3, 1]))
    with pytest.raises(IczError):
        entry_dec_attn_bwd(x, 1, 3, x, x, x, x, x, *out.views, 3, 36, 16, 2, counts=_i32([36, 40, 5]))
    torch.cuda.synchronize()
    assert all(torch.all(o == A.GUARD).item() for o in out.take())


# =====================================================================================================================
# aoa_dkv_kernel
@pytest.mark.parametrize("c", A.DK_CASES, ids=lambda c: c.name)
def test_dkv_against_float64_and_the_same_bits_for_every_chunk(c):
    """dKd and dVd within (G T + 2) roundings of the float64 sums for every chunk the case lists; tc = 0 launches the chunk of the handle's
    rule; every chunk gives the bits of every other (one fp32 accumulation in one order, passed through dKd / dVd between the passes);
    two runs the same bits.  The dS / Pd columns behind an image's count are NaN: staged, never used."""
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_dkv
    dS, Pd, Qp, dx = A.dk_inputs(c)
    lens, off = A.offsets(c.counts, c.n_img, c.R)
    ref = A.dkv_ref(c, dS, Pd, Qp, dx)
    B, d, pairs = c.n_img * c.G, c.Hd // c.NH, c.G * c.T
    for img in range(c.n_img):
        dS[:, img * c.G:(img + 1) * c.G, :, lens[img]:] = NAN
        Pd[:, img * c.G:(img + 1) * c.G, :, lens[img]:] = NAN
    dev = [_fenced(a.reshape(c.T * B, -1)) for a in (dS, Pd, Qp, dx)]
    counts = _i32(c.counts)
    frac, first = 0.0, None
    for tc in c.tcs:
        runs = []
        for _ in range(2):
            out = Laid([off[-1] * c.Hd] * 2)
            used = entry_dkv(*dev, out.views[0], out.views[1], c.n_img, B, c.T, c.R, c.Hd, c.NH, tc=tc, counts=counts, G=c.G)
            runs.append(out.take())
        assert used == (tc or A.dkv_tc(pairs, c.R, d)), (c.name, tc, used)
        assert all(torch.equal(a, b_) for a, b_ in zip(*runs)), (c.name, tc, "two runs differ")
        for what, got, (val, bound) in zip(("dKd", "dVd"), runs[0], ref):
            frac = max(frac, _within("aoa_dkv", (c.name, tc, what), got, val, bound))
        first = first or runs[0]
        assert all(torch.equal(a, b_) for a, b_ in zip(first, runs[0])), (c.name, "chunks of %d pairs and of %d differ" % (c.tcs[0], tc))
    print("dkv %s chunks %s (the handle's rule: passes of %s): worst error / bound %.3g" % (c.name, c.tcs, c.purpose["lib_chunks"], frac))


def test_dkv_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_dkv
    out = Laid([2 * 36 * 16] * 2)
    x = torch.zeros(7 * 7 * 2 * 129 * 520 // 64, device="cuda")
    for n_img, B, T, tc, R, Hd, NH, G in A.DK_REFUSED:
        with pytest.raises(IczError):
            entry_dkv(x, x, x, x, out.views[0], out.views[1], n_img, B, T, R, Hd, NH, tc=tc, G=G)
    with pytest.raises(IczError):
        entry_dkv(x, x, x, x, out.views[0], out.views[1], 2, 6, 5, 36, 16, 2, counts=_i32([36, 37]), G=3)
    torch.cuda.synchronize()
    assert all(torch.all(o == A.GUARD).item() for o in out.take())


# =====================================================================================================================
# LayerNorm backward: aoa_ln_bwd_kernel (form 0) and aoa_ln_bwd_dense_kernel (form 1)
def _slabs(a):
    """[ns, rows, cols] -> the slabs back to back in one NaN-fenced buffer (the kernels take them rows * cols apart: no gap between them)."""
    return _fenced(a.reshape(a.shape[0] * a.shape[1], -1))


@pytest.mark.parametrize("c", A.LB_CASES, ids=lambda c: c.name)
def test_layer_norm_backward_against_float64(c):
    """dx, dq_tot and (form 1) prod within the bound of the analytic float64 backward; operands the case leaves out are null pointers;
    the columns [0, n) of form 0's dq_b slabs are NaN (never read); two runs the same bits; live = 0 writes nothing."""
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_ln_bwd
    x, gain, dq_a, dq_b, res, stats = A.lb_inputs(c)
    ref = A.ln_bwd_ref(c, x, gain, dq_a, dq_b, res, stats)
    bn = None
    if dq_b is not None:
        bn = dq_b.copy()
        if c.form == 0:
            bn[:, :, :c.n] = NAN
    dev = dict(x=_fenced(x), g=_vec(gain), a=None if dq_a is None else _slabs(dq_a), b=None if bn is None else (_slabs(bn) if c.form == 0 else _fenced(bn)),
               res=None if res is None else _fenced(res), stats=_fenced(stats) if c.form == 0 else None, live=None if c.live is None else _i32([c.live]))
    m = c.rows * c.n
    runs = []
    for _ in range(2):
        out = Laid([m, m, m])
        dx, dq_tot, prod = out.views
        entry_ln_bwd(c.form, dev["a"], c.ns_a, dev["b"], c.ns_b, c.rows, dev["x"], dev["g"], dx, c.n, stats=dev["stats"], res=dev["res"], dq_tot=dq_tot,
                     prod=prod if c.form == 1 else None, live=dev["live"])
        runs.append(out.take())
    assert all(torch.equal(p, q) for p, q in zip(*runs)), (c.name, "two runs differ")
    dx, dq_tot, prod = runs[0]
    if c.live == 0:
        assert all(torch.all(o == A.GUARD).item() for o in runs[0]), "a dead step wrote"
        print("LayerNorm backward %s: nothing written" % c.name)
        return
    kernel = "aoa_ln_bwd" if c.form == 0 else "aoa_ln_bwd_dense"
    frac = max(_within(kernel, (c.name, "dx"), dx, *ref["dx"]), _within(kernel, (c.name, "dq_tot"), dq_tot, *ref["dq_tot"]))
    if c.form == 1:
        frac = max(frac, _within(kernel, (c.name, "prod"), prod, *ref["prod"]))
    else:
        assert torch.all(prod == A.GUARD).item()
    print("LayerNorm backward %s (%d vectors per thread): worst error / bound %.3g" % (c.name, A.lb_vectors(c.n), frac))


def test_layer_norm_backward_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_ln_bwd
    out = Laid([3 * 4100])
    x = torch.zeros(2 * 3 * 2 * 4100 + 4, device="cuda")
    for form, n, what in A.LB_REFUSED:
        with pytest.raises(IczError):
            entry_ln_bwd(form, x, 1, x[1:] if what == "odd" else x, 1 if form == 0 else 0, 3, x, x, out.views[0], n, stats=x if form == 0 or what == "stats" else None,
                         res=x if what == "res" or form == 1 else None, dq_tot=x, prod=x if form == 1 else None)
    torch.cuda.synchronize()
    assert torch.all(out.take()[0] == A.GUARD).item()


# =====================================================================================================================
# mha_self_bwd_kernel
@pytest.mark.parametrize("c", A.SB_CASES, ids=lambda c: c.name)
def test_self_attention_backward_against_float64(c):
    """[dQ | dK | dV] within the bound of the analytic float64 backward of the same inputs and keep flags, dropout off / explicit / Philox;
    Philox the bits of its twin's explicit mask; two runs the same bits."""
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_self_attn_bwd
    qkv, dO = A.sb_inputs(c)
    dev = dict(qkv=_fenced(qkv), dO=_fenced(dO), counts=_i32(c.counts))
    seed = _seed()
    masks = _masks(c, A.sa_draws(c), A.sa_keep(c), A.RNG_REF_ATT)
    frac, got = 0.0, {}
    for kind in ("off", "explicit", "philox", "twin"):
        mode, keep, mask_dev = masks[kind]
        drop = _dropp(c, mode, mask_dev, seed, A.RNG_REF_ATT)
        runs = []
        for _ in range(2):
            out = Laid([qkv.shape[0] * 3 * c.Hd])
            entry_self_attn_bwd(dev["qkv"], dev["dO"], out.views[0], c.n_img, c.R, c.Hd, c.NH, counts=dev["counts"], drop=drop)
            runs.append(out.take()[0])
        assert torch.equal(*runs), (c.name, kind, "two runs differ")
        got[kind] = runs[0]
        key = ("sb", c.name, "philox" if kind == "twin" else kind)
        if key not in _refs:
            _refs[key] = A.self_attn_bwd_ref(c, qkv, dO, mode, keep)
        frac = max(frac, _within("mha_self_bwd", (c.name, kind), runs[0], *_refs[key]))
    assert torch.equal(got["philox"], got["twin"]), (c.name, "Philox draws differ from their host twin")
    if c.R > 1:
        assert not torch.equal(got["philox"], got["off"])
    print("self-attention backward %s (%d bytes of LDS): worst error / bound %.3g" % (c.name, A.sb_lds(c.R, c.Hd // c.NH), frac))


def test_self_attention_backward_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.aoa_kernels import entry_self_attn_bwd
    out = Laid([2 * 36 * 48])
    x = torch.zeros(2 * 129 * 3 * 256 + 4, device="cuda")
    for R, Hd, NH in A.SB_REFUSED:
        with pytest.raises(IczError):
            entry_self_attn_bwd(x, x, out.views[0], 2, R, Hd, NH)
    with pytest.raises(IczError):
        entry_self_attn_bwd(x, x, out.views[0], 2, 36, 16, 2, counts=_i32([36, 0]))
    torch.cuda.synchronize()
    assert torch.all(out.take()[0] == A.GUARD).item()


def test_dynamic_lds_limit_only_grows():
    """The kernels' dynamic-LDS limit belongs to the process: a launch that needs less (still above 48 KB) must not take it away from a
    later launch that needs more.  Self-attention: 128 regions x 64 columns, then 49 x 128 on route 1, then the first again, same bits.
    Decoder attention: 36 regions x 260 columns, then 128 x 64, then the first again."""
    big, small = A.SA_BY_NAME["auto_chunk_r128_w64"], A.SA_BY_NAME["m128_r49"]
    assert A.self_lds(big.R, 64, A.self_qc(big.R, 64)) > A.self_lds(small.R, 128, small.R) > A.LDS_OPTIN
    devs = {c.name: dict(qkv=_fenced(A.sa_inputs(c)), counts=None, rows=c.n_img * c.R) for c in (big, small)}
    first = _sa_run(big, devs[big.name], 1, 0, None)[0]
    _sa_run(small, devs[small.name], 1, 0, None)
    assert torch.equal(first, _sa_run(big, devs[big.name], 1, 0, None)[0])
    dbig, dsmall = A.DA_BY_NAME["r36_w260"], A.DA_BY_NAME["r128_w64"]
    assert A.dec_lds(dbig.R, 260) > A.dec_lds(dsmall.R, 64) > A.LDS_OPTIN
    ddev = {c.name: _da_device(c) for c in (dbig, dsmall)}
    first = _da_run(dbig, ddev[dbig.name], None)
    _da_run(dsmall, ddev[dsmall.name], None)
    assert all(torch.equal(a, b_) for a, b_ in zip(first, _da_run(dbig, ddev[dbig.name], None)))


def test_zz_report_worst_error_fractions():
    """Runs last in this file: the largest error / bound of every kernel over all its cases (EXPERIMENTS.md records them)."""
    for k in sorted(_worst):
        print("aoa kernels: %-16s worst error / bound %.3f" % (k, _worst[k]))
    assert all(f <= 1.0 for f in _worst.values())
