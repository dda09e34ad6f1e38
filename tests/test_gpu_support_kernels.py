"""The kernels that finish a backward pass and apply the update, each on its own through the icz_test_* entries:
embed_grad_kernel / embed_grad_win_kernel, weight_norm(_multi) and its backward, transpose_multi, colsum(_multi), timesum,
rowgroup_sum, adam_clamp(_multi) -- against float64 references of the same fp32 inputs, at the shapes where each kernel takes
another branch.  The cases and what each is there for: tests/_support_kernels.py; tests/test_cpu_support_kernels.py holds them to it.

Bounds are the a-priori rounding bounds of tests/_support_kernels.py (u = 2^-24):
  sums            (fp32 additions on the element's path + 2) u sum|addends|: nh ns + 2 for a token with nh occurrences over ns slabs,
                  ceil(K / 8) + 8 for a column sum, depth + 1 for the sums over time / over an image's rows
  weight_norm     (cols + 8) u relative; backward: the same count on |dw| + |v| sum|v dw| / ||v||^2, times |g| / ||v||
  Adam            4 u on m and v, 16 u on the step against |p| + |update|
No element is excused.  Where the code promises bits, bits are asserted: the two embedding forms, a table job against the
single-matrix kernel, out2 against out, Adam's 16-byte path against its scalar path against the one-element kernel, and every case
run twice.  Every output lies between guards of 7.0 (a table's outputs between each other's), and everything a kernel has no business
reading -- row padding, rows behind rows_live, the gaps between slabs -- is NaN.  Each test prints its largest error as a fraction of
its bound."""
import numpy as np
import pytest
import torch

import _support_kernels as S

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 16                 # guard floats around every output
_worst = {}              # kernel -> largest error / bound seen


class Laid:
    """Flat views of the given sizes in ONE buffer of 7.0, PAD guard floats around each; view i starts `offs[i]` floats behind a
    16-byte boundary.  take() returns copies, puts the guard value back and asserts that nothing but the views was written."""

    def __init__(self, sizes, offs=None):
        offs = offs or [0] * len(sizes)
        at, pos = [], PAD
        for n, o in zip(sizes, offs):
            at.append(pos + o)
            pos = (pos + o + n + PAD + 3) // 4 * 4
        self.buf = torch.full((pos,), S.GUARD, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[a:a + n] for a, n in zip(at, sizes)]

    def fill(self, arrays):
        for v, a in zip(self.views, arrays):
            v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))

    def take(self):
        outs = [v.clone() for v in self.views]
        for v in self.views:
            v.fill_(S.GUARD)
        assert torch.all(self.buf == S.GUARD).item(), "a write outside the outputs"
        return outs


def _fenced(a, ld=None, off=0):
    """The 2-d fp32 array as a strided view [rows, cols] (row stride ld, starting `off` floats into the first row) of a NaN buffer,
    PAD NaN floats in front and behind.  An array without rows gives one row of NaN (an empty tensor has no pointer to hand over)."""
    rows, cols = a.shape
    ld = ld or cols
    assert off + cols <= ld
    buf = torch.full((2 * PAD + max(rows, 1) * ld,), NAN, device="cuda")
    view = torch.as_strided(buf, (max(rows, 1), cols), (ld, 1), PAD + off)
    if rows:
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


def _vec(a):
    return _fenced(np.asarray(a, dtype=np.float32).reshape(1, -1))


def _within(kernel, what, got, ref, bound):
    """got (fp32 tensor) within `bound` of `ref`, element by element; 0 where the bound is 0."""
    g = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert np.isfinite(g).all(), (kernel, what, "a value that is not finite: something read outside its operands")
    err = np.abs(g - ref)
    frac = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    _worst[kernel] = max(_worst.get(kernel, 0.0), frac)
    bad = np.argwhere(err > bound)
    assert not len(bad), (kernel, what, "%d elements outside the bound, first at %s: %r vs %r, error / bound %.3g" % (
        len(bad), bad[0].tolist(), g[tuple(bad[0])], ref[tuple(bad[0])], frac))
    return frac


def _same(a, b, what):
    assert all(torch.equal(x, y) for x, y in zip(a, b)), what


# =====================================================================================================================
# embedding gradient
_eg_cache = {}


def _eg_device(c):
    """Device operands of a case (made once, never written): slabs NaN-separated, rows behind rows_live NaN in demb and emb."""
    if c.name not in _eg_cache:
        tok, demb, emb = S.eg_inputs(c)
        n_live = c.n_tok if c.live is None else min(c.live, c.n_tok)
        stride = c.n_tok * c.E + S.EG_SLAB_PAD
        d = torch.full((2 * PAD + c.ns * stride,), NAN, device="cuda")
        for z in range(c.ns):
            d[PAD + z * stride:PAD + z * stride + n_live * c.E] = torch.from_numpy(demb[z, :n_live].reshape(-1)).cuda()
        e = torch.full((2 * PAD + c.n_tok * c.E,), NAN, device="cuda")
        e[PAD:PAD + n_live * c.E] = torch.from_numpy(emb[:n_live].reshape(-1)).cuda()
        live = None if c.live is None else torch.tensor([c.live], dtype=torch.int32, device="cuda")
        _eg_cache[c.name] = (torch.from_numpy(tok).cuda(), d, d[PAD:], e, e[PAD:], stride, live, (tok, demb, emb))
    return _eg_cache[c.name]


def _eg_run(c, relu, scale, route):
    from simpleimagecaptionzoo_amd.butd import embed_grad
    tok, _, demb, _, emb, stride, live, _ = _eg_device(c)
    out = Laid([c.V * c.E])
    embed_grad(tok, c.n_tok, demb, emb, scale, c.E, out.views[0], c.V, relu, ns=c.ns, slab_stride=stride, rows_live=live, route=route)
    return out.take()[0]


@pytest.mark.parametrize("c", S.EG_CASES, ids=lambda c: c.name)
def test_embedding_gradient_both_forms_against_float64(c):
    """Each route the case lists, ReLU on and off, scale 1 and 2: within nh ns + 2 roundings of the float64 sum, all routes the same
    bits (the header's claim: the same additions in the same order), two runs the same bits, rows without occurrences exactly 0."""
    from simpleimagecaptionzoo_amd.butd import embed_grad_route_for
    tok, demb, emb = _eg_device(c)[-1]
    frac = 0.0
    for relu in S.EG_RELU:
        for scale in S.EG_SCALES:
            ref, bound = S.embed_grad_ref(tok, demb, emb, scale, relu, c.V, c.live)
            outs = {r: _eg_run(c, relu, scale, r) for r in c.routes}
            for r, o in outs.items():
                frac = max(frac, _within("embed_grad", (c.name, "route", r, "relu", relu, "scale", scale), o, ref, bound))
                assert torch.equal(o, _eg_run(c, relu, scale, r)), (c.name, r, "two runs differ")
            first = outs[c.routes[0]]
            for r in c.routes[1:]:
                assert torch.equal(first, outs[r]), (c.name, "routes %d and %d differ" % (c.routes[0], r), relu, scale)
            if c.live == 0:
                assert not first.any().item()
    if 0 in c.routes:
        assert embed_grad_route_for(c.n_tok, c.E)[0] == c.purpose["route0"]
    print("embed_grad %s routes %s: worst error / bound %.3g" % (c.name, c.routes, frac))


def test_embedding_gradient_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import embed_grad
    out = Laid([21 * 1028])
    for n_tok, E, route in S.EG_REFUSED:
        tok = torch.zeros(n_tok, dtype=torch.int64, device="cuda")
        x = torch.zeros(n_tok * E + 4, device="cuda")
        with pytest.raises(IczError):
            embed_grad(tok, n_tok, x, x, 1.0, E, out.views[0], 21, 1, route=route)
        with pytest.raises(IczError):           # one float off a 16-byte boundary
            embed_grad(tok, n_tok, x[1:], x, 1.0, 4, out.views[0], 21, 1)
    torch.cuda.synchronize()
    assert torch.all(out.take()[0] == S.GUARD).item()


# =====================================================================================================================
# weight_norm and its backward
def _wn_job(rows, cols, tag=""):
    v, g, dw = S.wn_inputs(rows, cols, tag)
    nrm32 = S.weight_norm_ref(v, g)[1][0].astype(np.float32)
    dev = dict(v=_fenced(v), g=_vec(g), dw=_fenced(dw, ld=cols + S.WN_BWD_PAD), norm=_vec(nrm32))
    return (v, g, dw, nrm32), dev


def _wn_forward(jobs, multi):
    """jobs = [(rows, cols, dev)] -> [w...], [norm...] of one launch, every output between guards."""
    from simpleimagecaptionzoo_amd.butd import weight_norm
    out = Laid([r * c for r, c, _ in jobs] + [r for r, _, _ in jobs])
    n = len(jobs)
    weight_norm([(d["v"], d["g"], out.views[i], out.views[n + i], r, c) for i, (r, c, d) in enumerate(jobs)], multi)
    got = out.take()
    return got[:n], got[n:]


def _wn_backward(jobs, multi):
    from simpleimagecaptionzoo_amd.butd import weight_norm_bwd
    out = Laid([r * c for r, c, _ in jobs] + [r for r, _, _ in jobs])
    n = len(jobs)
    weight_norm_bwd([(d["dw"], c + S.WN_BWD_PAD, d["v"], d["g"], d["norm"], out.views[i], out.views[n + i], r, c)
                     for i, (r, c, d) in enumerate(jobs)], multi)
    got = out.take()
    return got[:n], got[n:]


def _wn_check(rows, cols, host, w, norm, dv, dg, what):
    v, g, dw, nrm32 = host
    (rw, bw), (rn, bn) = S.weight_norm_ref(v, g)
    (rdv, bdv), (rdg, bdg) = S.weight_norm_bwd_ref(dw, v, g, nrm32)
    return max(_within("weight_norm", what + ("w",), w, rw, bw), _within("weight_norm", what + ("norm",), norm, rn, bn),
               _within("weight_norm_bwd", what + ("dv",), dv, rdv, bdv), _within("weight_norm_bwd", what + ("dg",), dg, rdg, bdg))


@pytest.mark.parametrize("rows,cols", S.WN_SINGLE)
def test_weight_norm_single_matrix_forward_and_backward(rows, cols):
    """One matrix on the single-matrix kernels and as a table of one job: (cols + 8) u, the same bits, twice the same bits.  dw has
    NaN row padding."""
    host, dev = _wn_job(rows, cols)
    job = [(rows, cols, dev)]
    w, norm = _wn_forward(job, False)
    dv, dg = _wn_backward(job, False)
    frac = _wn_check(rows, cols, host, w[0], norm[0], dv[0], dg[0], (rows, cols))
    for multi in (False, True):
        _same(w + norm, sum(_wn_forward(job, multi), []), (rows, cols, multi, "forward bits"))
        _same(dv + dg, sum(_wn_backward(job, multi), []), (rows, cols, multi, "backward bits"))
    print("weight_norm %d x %d: worst error / bound %.3g" % (rows, cols, frac))


@pytest.mark.parametrize("name", list(S.WN_TABLES))
def test_weight_norm_tables_equal_the_jobs_alone(name):
    """1..4 jobs of mixed shapes in one launch, ragged jobs in the middle: every job bit for bit what the single-matrix kernel gives
    for it alone, every job's outputs between the other jobs' outputs and guards."""
    shapes = S.WN_TABLES[name]
    made = [_wn_job(r, c, "%s job %d" % (name, i)) for i, (r, c) in enumerate(shapes)]
    jobs = [(r, c, dev) for (r, c), (_, dev) in zip(shapes, made)]
    w, norm = _wn_forward(jobs, True)
    dv, dg = _wn_backward(jobs, True)
    _same(w + norm, sum(_wn_forward(jobs, True), []), (name, "two forward runs differ"))
    _same(dv + dg, sum(_wn_backward(jobs, True), []), (name, "two backward runs differ"))
    frac = 0.0
    for i, ((r, c), (host, dev)) in enumerate(zip(shapes, made)):
        w1, n1 = _wn_forward([(r, c, dev)], False)
        dv1, dg1 = _wn_backward([(r, c, dev)], False)
        assert torch.equal(w[i], w1[0]) and torch.equal(norm[i], n1[0]), (name, i, "forward: table and single kernel differ")
        assert torch.equal(dv[i], dv1[0]) and torch.equal(dg[i], dg1[0]), (name, i, "backward: table and single kernel differ")
        frac = max(frac, _wn_check(r, c, host, w[i], norm[i], dv[i], dg[i], (name, i)))
    print("weight_norm table %s: worst error / bound %.3g" % (name, frac))


def test_weight_norm_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import weight_norm, weight_norm_bwd
    _, d = _wn_job(4, 8)
    out = Laid([32, 4])
    fwd = (d["v"], d["g"], out.views[0], out.views[1], 4, 8)
    bwd = (d["dw"], 8 + S.WN_BWD_PAD, d["v"], d["g"], d["norm"], out.views[0], out.views[1], 4, 8)
    for call in (lambda: weight_norm([fwd] * 5, True), lambda: weight_norm([fwd] * 2, False), lambda: weight_norm([], True),
                 lambda: weight_norm([fwd[:5] + (6,)], True), lambda: weight_norm([fwd[:2] + (out.views[0][1:],) + fwd[3:]], True),
                 lambda: weight_norm_bwd([bwd] * 5, True), lambda: weight_norm_bwd([bwd] * 2, False),
                 lambda: weight_norm_bwd([bwd[:1] + (6,) + bwd[2:]], True), lambda: weight_norm_bwd([bwd[:8] + (6,)], True)):
        with pytest.raises(IczError):
            call()
    torch.cuda.synchronize()
    out.take()


# =====================================================================================================================
# transpose_multi
@pytest.mark.parametrize("name", list(S.TR_TABLES))
def test_transpose_tables_are_exact(name):
    from simpleimagecaptionzoo_amd.butd import transpose_multi
    rs = np.random.RandomState(len(name))
    shapes = S.TR_TABLES[name]
    host = [rs.standard_normal((r, c)).astype(np.float32) for r, c, _, _ in shapes]
    src = [_fenced(a, ld=ld, off=off) for a, (_, _, ld, off) in zip(host, shapes)]

    def run():
        out = Laid([r * c for r, c, _, _ in shapes])
        transpose_multi([(s, ld, r, c, o) for s, (r, c, ld, _), o in zip(src, shapes, out.views)])
        return out.take()
    got = run()
    for a, o, (r, c, _, _) in zip(host, got, shapes):
        assert torch.equal(o.view(c, r).cpu(), torch.from_numpy(a).t()), (name, r, c)
    _same(got, run(), (name, "two runs differ"))


def test_transpose_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import transpose_multi
    src = _fenced(np.zeros((192, 192), dtype=np.float32))
    out = Laid([192 * 192])
    calls = [lambda: transpose_multi([(src, 192, 64, 64, out.views[0])] * 5), lambda: transpose_multi([]),
             lambda: transpose_multi([(src[:, 1:], 192, 64, 64, out.views[0])]), lambda: transpose_multi([(src, 192, 64, 64, out.views[0][1:])])]
    calls += [lambda r=r, c=c, ld=ld: transpose_multi([(src, ld, r, c, out.views[0])]) for r, c, ld in S.TR_REFUSED]
    for call in calls:
        with pytest.raises(IczError):
            call()
    torch.cuda.synchronize()
    out.take()


# =====================================================================================================================
# column sums
def _colsum_x(K, N, ldx, tag):
    x = S.seeded("colsum %d %d %s" % (K, N, tag)).standard_normal((K, N)).astype(np.float32)
    return x, _fenced(x, ld=ldx)


def _colsum_single(dev, K, N, ldx):
    from simpleimagecaptionzoo_amd.butd import colsum
    out = Laid([N])
    colsum([(dev, K, N, ldx, out.views[0], None)], multi=False)
    return out.take()[0]


@pytest.mark.parametrize("K", S.COLSUM_K)
def test_column_sum_single_kernel(K):
    """K on both sides of the 8-row load batch, N on both sides of a 32-column block, NaN row padding: ceil(K / 8) + 8 roundings."""
    frac = 0.0
    for N in S.COLSUM_N:
        x, dev = _colsum_x(K, N, N + S.COLSUM_PAD, "single")
        got = _colsum_single(dev, K, N, N + S.COLSUM_PAD)
        frac = max(frac, _within("colsum", (K, N), got, *S.colsum_ref(x)))
        assert torch.equal(got, _colsum_single(dev, K, N, N + S.COLSUM_PAD)), (K, N, "two runs differ")
        if K == 0:
            assert not got.any().item()
    print("colsum K = %d: worst error / bound %.3g" % (K, frac))


@pytest.mark.parametrize("name", list(S.COLSUM_TABLES))
def test_column_sum_tables_equal_the_jobs_alone(name):
    from simpleimagecaptionzoo_amd.butd import colsum
    shapes = S.COLSUM_TABLES[name]
    made = [_colsum_x(K, N, ldx, "%s %d" % (name, i)) for i, (K, N, ldx, _) in enumerate(shapes)]
    with2 = [i for i, s in enumerate(shapes) if s[3]]

    def run():
        out = Laid([N for _, N, _, _ in shapes] + [shapes[i][1] for i in with2])
        o2 = {i: out.views[len(shapes) + j] for j, i in enumerate(with2)}
        colsum([(dev, K, N, ldx, out.views[i], o2.get(i)) for i, ((K, N, ldx, _), (_, dev)) in enumerate(zip(shapes, made))], multi=True)
        return out.take()
    got = run()
    _same(got, run(), (name, "two runs differ"))
    frac = 0.0
    for i, ((K, N, ldx, _), (x, dev)) in enumerate(zip(shapes, made)):
        assert torch.equal(got[i], _colsum_single(dev, K, N, ldx)), (name, i, "table and single kernel differ")
        frac = max(frac, _within("colsum_multi", (name, i), got[i], *S.colsum_ref(x)))
        if K == 0:
            assert not got[i].any().item()
    for j, i in enumerate(with2):
        assert torch.equal(got[len(shapes) + j], got[i]), (name, i, "out2 differs from out")
    print("colsum table %s: worst error / bound %.3g" % (name, frac))


def test_column_sum_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import colsum
    _, dev = _colsum_x(8, 32, 32, "refusal")
    out = Laid([32, 32])
    job = (dev, 8, 32, 32, out.views[0], None)
    for call in (lambda: colsum([job] * 9, True), lambda: colsum([job] * 2, False), lambda: colsum([], True),
                 lambda: colsum([job[:3] + (31,) + job[4:]], True), lambda: colsum([job[:5] + (out.views[1],)], False)):
        with pytest.raises(IczError):
            call()
    torch.cuda.synchronize()
    out.take()


# =====================================================================================================================
# sums over time and over an image's rows
@pytest.mark.parametrize("depth", S.SUM_DEPTHS)
def test_time_sum_and_row_group_sum(depth):
    """Depth 1, 2, 5, 8; rows of 4, 1020, 1024, 1028 floats (both sides of one block of 256 threads); 1 and 3 images."""
    from simpleimagecaptionzoo_amd.butd import rowgroup_sum, timesum
    frac = 0.0
    for width in S.SUM_WIDTHS:
        x = S.seeded("timesum %d %d" % (depth, width)).standard_normal((depth, width)).astype(np.float32)
        dev = _fenced(x)

        def run():
            out = Laid([width])
            timesum(dev, depth, width, out.views[0])
            return out.take()[0]
        got = run()
        frac = max(frac, _within("timesum", (depth, width), got, *S.depth_sum_ref(x)))
        assert torch.equal(got, run()), (depth, width, "two runs differ")
        for n_img in S.SUM_IMAGES:
            x = S.seeded("rowgroup %d %d %d" % (depth, width, n_img)).standard_normal((n_img, depth, width)).astype(np.float32)
            dev = _fenced(x.reshape(n_img * depth, width))

            def run():
                out = Laid([n_img * width])
                rowgroup_sum(dev, n_img, depth, width, out.views[0])
                return out.take()[0]
            got = run()
            ref, bound = S.depth_sum_ref(np.moveaxis(x, 1, 0))
            frac = max(frac, _within("rowgroup_sum", (n_img, depth, width), got, ref, bound))
            assert torch.equal(got, run()), (n_img, depth, width, "two runs differ")
    print("timesum / rowgroup_sum depth %d: worst error / bound %.3g" % (depth, frac))


def test_depth_sum_refusals_write_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import rowgroup_sum, timesum
    x = _fenced(np.zeros((4, 16), dtype=np.float32))
    out = Laid([16])
    o = out.views[0]
    for call in (lambda: timesum(x, 0, 16, o), lambda: timesum(x, 2, 6, o), lambda: timesum(x[:, 1:], 2, 8, o), lambda: timesum(x, 2, 8, o[1:]),
                 lambda: rowgroup_sum(x, 0, 2, 8, o), lambda: rowgroup_sum(x, 1, 0, 8, o), lambda: rowgroup_sum(x, 1, 2, 6, o),
                 lambda: rowgroup_sum(x[:, 1:], 1, 2, 8, o), lambda: rowgroup_sum(x, 1, 2, 8, o[1:])):
        with pytest.raises(IczError):
            call()
    torch.cuda.synchronize()
    out.take()


# =====================================================================================================================
# Adam
def _adam_launch(sizes, offsets, step, kind, tag=""):
    """One update of len(sizes) tensors, tensor i's (p, g, m, v) offs[i] floats behind a 16-byte boundary, all of them in one
    guarded buffer.  kind "multi": one icz_adam_clamp_multi launch; "step": icz_adam_clamp_step per tensor.  -> [(p, m, v)] after
    the update; g must come back as it went in."""
    from simpleimagecaptionzoo_amd.butd import adam_clamp_multi, adam_clamp_step
    host = [S.adam_inputs(n, tag + str(i)) for i, n in enumerate(sizes)]
    lay = Laid([n for n in sizes for _ in range(4)], [o for offs in offsets for o in offs])
    lay.fill([a for h in host for a in h])
    t = [tuple(lay.views[4 * i:4 * i + 4]) + (n,) for i, n in enumerate(sizes)]
    if kind == "multi":
        adam_clamp_multi(t, S.ADAM_LR, S.ADAM_CLIP, step)
    else:
        for p, g, m, v, n in t:
            adam_clamp_step(p, g, m, v, n, S.ADAM_LR, S.ADAM_CLIP, step)
    got = lay.take()
    for i, h in enumerate(host):
        assert torch.equal(got[4 * i + 1].cpu(), torch.from_numpy(h[1])), "the gradient was written"
    return host, [(got[4 * i], got[4 * i + 2], got[4 * i + 3]) for i in range(len(sizes))]


def _adam_check(n, host, got, step, what):
    r = S.adam_ref(*host, S.ADAM_LR, S.ADAM_CLIP, step)
    frac = max(_within("adam", what + (k,), t, *r[k]) for k, t in zip("pmv", got))
    z = torch.from_numpy(S.adam_zero_state(n))
    p0 = torch.from_numpy(host[0])
    assert torch.equal(got[0].cpu()[z], p0[z]), (what, "the parameter moved where g = m = v = 0")
    assert not got[1].cpu()[z].any() and not got[2].cpu()[z].any(), (what, "zero state")
    return frac


@pytest.mark.parametrize("n", S.ADAM_SIZES)
def test_adam_aligned_offset_and_single_tensor_agree(n):
    """Steps 1, 2 and 1000: the one-element kernel within the bounds; the table kernel on a 16-byte aligned tensor (its 16-byte path,
    the scalar path at the tail), with every array offset by 1, 2, 3 floats and with only one of the four arrays offset (the scalar
    path throughout): bit for bit the same."""
    frac = 0.0
    for step in S.ADAM_STEPS:
        host, base = _adam_launch([n], [(0, 0, 0, 0)], step, "step")
        frac = max(frac, _adam_check(n, host[0], base[0], step, (n, step)))
        for name, offs in S.ADAM_VARIANTS.items():
            for kind in ("multi", "step"):
                _, got = _adam_launch([n], [offs], step, kind)
                _same(base[0], got[0], (n, step, name, kind, "differs from the aligned one-element kernel"))
    print("adam n = %d: worst error / bound %.3g" % (n, frac))


def test_adam_32_tensors_in_one_launch():
    """32 tensors of mixed sizes, block-exact ones among them, in one launch: aligned, and tensor i laid out by variant i % 8 --
    every tensor bit for bit what the one-element kernel gives for it alone, within the bounds, twice the same bits."""
    sizes = list(S.ADAM_32)
    variants = list(S.ADAM_VARIANTS.values())
    aligned = [(0, 0, 0, 0)] * len(sizes)
    mixed = [variants[i % len(variants)] for i in range(len(sizes))]
    host, alone = _adam_launch(sizes, aligned, 2, "step", "t")
    frac = 0.0
    for offs in (aligned, mixed):
        _, got = _adam_launch(sizes, offs, 2, "multi", "t")
        _, again = _adam_launch(sizes, offs, 2, "multi", "t")
        for i, n in enumerate(sizes):
            _same(alone[i], got[i], (i, n, "table and one-element kernel differ"))
            _same(got[i], again[i], (i, n, "two runs differ"))
    for i, n in enumerate(sizes):
        frac = max(frac, _adam_check(n, host[i], alone[i], 2, (i, n)))
    print("adam 32 tensors: worst error / bound %.3g" % frac)


def test_adam_33_tensors_are_refused():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import adam_clamp_multi
    lay = Laid([4] * 4)
    with pytest.raises(IczError, match="count 33 out of range"):
        adam_clamp_multi([tuple(lay.views) + (4,)] * 33, S.ADAM_LR, S.ADAM_CLIP, 1)
    torch.cuda.synchronize()
    lay.take()


def test_zz_report_worst_error_fractions():
    """Last in the file: the largest error / bound per kernel over everything above (DESIGN.md section 3 quotes these)."""
    for k in sorted(_worst):
        print("support kernels: %-16s worst error / bound %.3f" % (k, _worst[k]))
    assert all(f <= 1.0 for f in _worst.values())
