"""The GEMMs over several K segments on their own: every kernel behind gemm_f32 with the operands a decoder
step hands it -- column slices of wider activation and weight buffers, one (lda, ldb, K) per segment, split-K ranges that start and
end inside a segment, the live flag, accumulate -- against the float64 product of the same fp32 operands.

Bound: 3e-6 of max|C|, the bound of test_gemm_against_float64 (every K total here is below 4096; the fp32-MFMA kernels multiply
exactly, the split-precision ones drop terms below 3 * 2^-24).  No row is excused.  Everything outside a segment's own K range is
NaN: a load that strays, even one that is later multiplied by zero, makes the result non-finite.  Outputs sit between guards of 7.0.
The cases and what each is there for: tests/_gemm_segments.py; tests/test_cpu_gemm_segments.py holds their routes to their claims.
"""
import pytest
import torch

import _gemm_segments as T

pytestmark = pytest.mark.gpu

BOUND = 3e-6
NAN = float("nan")
_ref_cache = {}


def _fenced(rows, cols, row0, col0, gen):
    """A [rows, cols] block of normal values inside a wider NaN tensor, one NaN row above and below, NaN columns around."""
    wide = torch.full((rows + 2, col0 + cols + 4), NAN, device="cuda")
    blk = wide[row0:row0 + rows, col0:col0 + cols]
    blk.copy_(torch.randn(rows, cols, device="cuda", generator=gen))
    return blk


def _operands(layout, M, N, Ks, seed):
    """Segment operands the way the decoders pass them.  NT / NN: one activation tensor [M, sum(K_s) + 4 nseg] holds every A_s as a
    column slice with four NaN columns behind it; NT: every B_s is a column block [N, K_s] of one wider weight tensor, at a non-zero
    offset that is a multiple of 4, four NaN columns between blocks; NN / TN: every k-major operand is a block of its own wider
    tensor at column offset 4.  Cached per (case shape, seed) with the float64 product, and never written again."""
    key = (layout, M, N, tuple(Ks), seed)
    if key in _ref_cache:
        return _ref_cache[key]
    gen = torch.Generator(device="cuda").manual_seed(seed)
    nseg, tot = len(Ks), sum(Ks)
    As, Bs = [], []
    if layout in ("nt", "nn"):
        act = torch.full((M + 2, tot + 4 * nseg), NAN, device="cuda")
        off = 0
        for k in Ks:
            a = act[1:1 + M, off:off + k]
            a.copy_(torch.randn(M, k, device="cuda", generator=gen))
            As.append(a)
            off += k + 4
    if layout == "nt":
        w = torch.full((N + 2, 8 + tot + 4 * nseg), NAN, device="cuda")
        off = 8
        for k in Ks:
            b = w[1:1 + N, off:off + k]
            b.copy_(torch.randn(N, k, device="cuda", generator=gen))
            Bs.append(b)
            off += k + 4
    elif layout == "nn":
        Bs = [_fenced(k, N, 1, 4, gen) for k in Ks]
    else:
        As = [_fenced(k, M, 1, 4, gen) for k in Ks]
        Bs = [_fenced(k, N, 1, 4, gen) for k in Ks]
    bias = torch.randn(N, device="cuda", generator=gen) if layout != "tn" else None
    ref = torch.zeros(M, N, device="cuda", dtype=torch.float64)
    for a, b in zip(As, Bs):
        ref += {"nt": lambda: a.double() @ b.double().t(), "nn": lambda: a.double() @ b.double(), "tn": lambda: a.double().t() @ b.double()}[layout]()
    if bias is not None:
        ref += bias.double()
    assert torch.isfinite(ref).all()
    _ref_cache[key] = (As, Bs, bias, ref)
    return _ref_cache[key]


def _err(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _pad4(n):
    return (n + 3) // 4 * 4


def _run(layout, M, N, As, Bs, bias, nsplit, ns, live=None, accumulate=False, c0=None):
    """One guarded launch -> the [M, N] result.  ns (the split that will run) picks the form: one split -> C is a column slice
    (ldc > N, a multiple of 4) of a tensor of 7.0 with four guard rows above and below; more -> 4096 guard floats behind the slabs,
    which the library sums into a dense C between guard rows, or, where its float4 sum does not apply (M N, or N under a bias, no
    multiple of 4), the test sums in slab order as a decoder's consumer kernel would."""
    from simpleimagecaptionzoo_amd.butd import gemm_seg
    info = {}
    if ns == 1:
        buf = torch.full((M + 8, _pad4(N) + 8), 7.0, device="cuda")
        C = buf[4:4 + M, 4:4 + N]
        if c0 is not None:
            C.copy_(c0)
        gemm_seg(layout, As, Bs, bias, nsplit, out=C, accumulate=accumulate, live=live, info=info)
        out = C.clone()
        C.fill_(7.0)
        assert torch.all(buf == 7.0), "a write outside C"
    else:
        ws = torch.full((ns * M * N + 4096,), 7.0, device="cuda")
        if (M * N) % 4 == 0 and (bias is None or N % 4 == 0):
            buf = torch.full((M + 8, N), 7.0, device="cuda")
            out = gemm_seg(layout, As, Bs, bias, nsplit, out=buf[4:4 + M], live=live, workspace=ws[:ns * M * N], info=info).clone()
            assert torch.all(buf[:4] == 7.0) and torch.all(buf[4 + M:] == 7.0), "a write outside C"
        else:
            slabs = gemm_seg(layout, As, Bs, None, nsplit, live=live, workspace=ws[:ns * M * N], raw_slabs=True, info=info)
            out = slabs[0].clone()
            for z in range(1, ns):
                out += slabs[z]
            if bias is not None:
                out += bias
        assert torch.all(ws[ns * M * N:] == 7.0), "a write behind the slabs"
    assert info["nsplit"] == ns, (info, ns)
    return out


def _check_case(c, split, tag=""):
    As, Bs, bias, ref = _operands(c.layout, c.M, c.N, c.Ks, 1000 + T.CASES.index(c))
    ns = c.picked if split == 0 else split
    out = _run(c.layout, c.M, c.N, As, Bs, bias, split, ns)
    err = _err(out, ref)
    print("gemm_seg %s%s split %d -> %d: err %.3g" % (c.name, tag, split, ns, err))
    assert torch.isfinite(out).all(), (c.name, split, "a load outside a segment's K range")
    assert err < BOUND, (c.name, split, ns, err)
    again = _run(c.layout, c.M, c.N, As, Bs, bias, split, ns)
    assert torch.equal(out, again), (c.name, split, "two runs differ")
    return out


@pytest.mark.parametrize("c", [c for c in T.CASES if c.route != "x3" and not c.accumulate_only], ids=lambda c: c.name)
def test_segmented_gemm_against_float64_with_nan_fences_and_guards(c):
    from simpleimagecaptionzoo_amd.butd import gemm_route_for
    for split in c.splits:
        assert gemm_route_for(c.layout, c.M, c.N, c.Ks, split) == c.route
        _check_case(c, split)


@pytest.mark.parametrize("c", [c for c in T.CASES if c.route == "x3"], ids=lambda c: c.name)
def test_many_row_segmented_gemm_under_every_large_tile_switch(c):
    """The 128 x 128 two-barrier kernel (0), the per-shape choice (-1) and the three-per-CU large tile (4): same split-K decomposition,
    same arithmetic per accumulator -> the same bits (tests/test_gpu_gemm.py holds that for one segment)."""
    from simpleimagecaptionzoo_amd.butd import gemm_route_for, gemm_set_big_cfg
    try:
        outs = {}
        for cfg in T.X3_CFGS:
            gemm_set_big_cfg(cfg)
            for split in c.splits:
                assert gemm_route_for(c.layout, c.M, c.N, c.Ks, split) in T.X3_ROUTES[cfg]
                outs[cfg, split] = _check_case(c, split, " cfg %d" % cfg)
        for split in c.splits:
            assert torch.equal(outs[0, split], outs[4, split]) and torch.equal(outs[0, split], outs[-1, split]), (c.name, split)
    finally:
        gemm_set_big_cfg(-2)


@pytest.mark.parametrize("name", T.LIVE_CASES)
def test_live_flag_zero_writes_nothing_and_nonzero_changes_nothing(name):
    from simpleimagecaptionzoo_amd.butd import gemm_seg
    c = T.BY_NAME[name]
    M, N = c.M, c.N
    As, Bs, bias, ref = _operands(c.layout, M, N, c.Ks, 1000 + T.CASES.index(c))
    acc = c.accumulate_only
    ns = 1 if acc else c.picked
    split = 1 if acc else 0
    c0 = torch.randn(M, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) if acc else None
    dead = torch.zeros(1, device="cuda", dtype=torch.int32)
    three = torch.full((1,), 3, device="cuda", dtype=torch.int32)
    if ns == 1:
        fill = c0 if acc else torch.full((M, N), 7.0, device="cuda")
        out = _run(c.layout, M, N, As, Bs, bias, split, 1, live=dead, accumulate=acc, c0=fill)      # guards checked inside
        assert torch.equal(out, fill), (name, "a dead step wrote C")
    else:
        ws = torch.full((ns * M * N + 4096,), 7.0, device="cuda")
        info = {}
        gemm_seg(c.layout, As, Bs, None, 0, live=dead, workspace=ws[:ns * M * N], raw_slabs=True, info=info)
        assert info["nsplit"] == ns
        assert torch.all(ws == 7.0), (name, "a dead step wrote its slabs")
    plain = _run(c.layout, M, N, As, Bs, bias, split, ns, accumulate=acc, c0=c0)
    flagged = _run(c.layout, M, N, As, Bs, bias, split, ns, live=three, accumulate=acc, c0=c0)
    assert torch.equal(plain, flagged), name
    want = ref + c0.double() if acc else ref
    assert _err(plain, want) < BOUND


@pytest.mark.parametrize("name", ["tn_acc", "res_512_two[64]", "res_512_two[36]"])
def test_accumulate_adds_the_product_to_c(name):
    """C += product: the NIC `w_ih +=` product (TN), and a decoder-gate shape which the resident kernel refuses under accumulate and
    the fp32-MFMA kernel takes in one split."""
    c = T.BY_NAME[name]
    As, Bs, bias, ref = _operands(c.layout, c.M, c.N, c.Ks, 1000 + T.CASES.index(c))
    c0 = torch.randn(c.M, c.N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    want = ref + c0.double()
    for split in (0, 1, 3):       # accumulate forces one split whatever is asked
        out = _run(c.layout, c.M, c.N, As, Bs, bias, split, 1, accumulate=True, c0=c0)
        err = _err(out, want)
        print("gemm_seg %s accumulate (nsplit %d asked): err %.3g" % (name, split, err))
        assert torch.isfinite(out).all() and err < BOUND, (name, split, err)


def _pair_operands(p, seed):
    M, N, Ks = p
    return _operands("nt", M, N, Ks, seed)


@pytest.mark.parametrize("i", range(len(T.PAIRS)))
def test_resident_pair_launch_equals_the_two_launches(i):
    from simpleimagecaptionzoo_amd.butd import gemm_resident_pair, gemm_seg
    pa, pb, nsr, nranges = T.PAIRS[i]
    ops = [_pair_operands(pa, 2000 + 2 * i), _pair_operands(pb, 2001 + 2 * i)]
    sizes = [nranges * p[0] * p[1] for p in (pa, pb)]

    def launch():
        bufs = [torch.full((n + 4096,), 7.0, device="cuda") for n in sizes]
        sa, sb = gemm_resident_pair(ops[0][0], ops[0][1], ops[1][0], ops[1][1], bufs[0][:sizes[0]], bufs[1][:sizes[1]])
        for b, n in zip(bufs, sizes):
            assert torch.all(b[n:] == 7.0), "a write behind the slabs"
        return sa, sb
    first, second = launch(), launch()
    for (M, N, Ks), (As, Bs, bias, ref), slabs, again in zip((pa, pb), ops, first, second):
        assert slabs.shape == (nranges, M, N)
        assert torch.equal(slabs, again)
        total = slabs[0].clone()
        for z in range(1, nranges):
            total += slabs[z]
        err = _err(total + bias, ref)
        print("resident pair %d x %d x %s (%d stages per range): err %.3g" % (M, N, Ks, nsr, err))
        assert torch.isfinite(slabs).all() and err < BOUND, (M, N, Ks, err)
        alone = gemm_seg("nt", As, Bs, None, 0, raw_slabs=True)
        assert alone.shape == slabs.shape and torch.equal(alone, slabs), (M, N, Ks, "the pair's slabs differ from the launch alone")


def test_resident_pair_refuses_two_stage_forms():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import gemm_resident_pair
    pa, pb = T.PAIR_MIXED
    a, b = _pair_operands(pa, 2000), _pair_operands(pb, 2003)
    bufs = [torch.full((4 * p[0] * p[1],), 7.0, device="cuda") for p in (pa, pb)]
    with pytest.raises(IczError):
        gemm_resident_pair(a[0], a[1], b[0], b[1], bufs[0], bufs[1])
    torch.cuda.synchronize()
    assert torch.all(bufs[0] == 7.0) and torch.all(bufs[1] == 7.0)


def test_segment_entry_refusals_leave_the_output_untouched():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import gemm_seg
    M, N = 20, 64
    gen = torch.Generator(device="cuda").manual_seed(3)
    X = torch.randn(M, 5 * 64 + 8, device="cuda", generator=gen)
    W = torch.randn(N, 5 * 64 + 8, device="cuda", generator=gen)
    odd_x, odd_w = torch.randn(M, 67, device="cuda", generator=gen), torch.randn(N, 67, device="cuda", generator=gen)
    bias = torch.randn(N, device="cuda", generator=gen)
    out = torch.full((M, N), 7.0, device="cuda")
    ws = torch.full((8 * M * N,), 7.0, device="cuda")
    seg = lambda t, s, k=64, o=0: t[:, 64 * s + o:64 * s + o + k]
    five = ([seg(X, s) for s in range(5)], [seg(W, s) for s in range(5)])
    refused = {
        "nseg 0": lambda: gemm_seg("nt", [], [], out=out, workspace=ws),
        "nseg 5": lambda: gemm_seg("nt", five[0], five[1], out=out, workspace=ws),
        "K % 4": lambda: gemm_seg("nt", [seg(X, 0), seg(X, 1, 62)], [seg(W, 0), seg(W, 1, 62)], out=out, workspace=ws),
        "odd A offset": lambda: gemm_seg("nt", [seg(X, 0), seg(X, 1, 64, 1)], [seg(W, 0), seg(W, 1)], out=out, workspace=ws),
        "odd B offset": lambda: gemm_seg("nt", [seg(X, 0), seg(X, 1)], [seg(W, 0), seg(W, 1, 64, 3)], out=out, workspace=ws),
        "lda % 4": lambda: gemm_seg("nt", [seg(X, 0), odd_x[:, :64]], [seg(W, 0), seg(W, 1)], out=out, workspace=ws),
        "ldb % 4": lambda: gemm_seg("nt", [seg(X, 0), seg(X, 1)], [seg(W, 0), odd_w[:, :64]], out=out, workspace=ws),
        "bias with raw slabs": lambda: gemm_seg("nt", [seg(X, 0), seg(X, 1)], [seg(W, 0), seg(W, 1)], bias, 2, workspace=ws, raw_slabs=True),
        "empty split": lambda: gemm_seg("nt", [seg(X, 0), seg(X, 1), seg(X, 2)], [seg(W, 0), seg(W, 1), seg(W, 2)], None, 5, out=out, workspace=ws),
        "more splits than stages": lambda: gemm_seg("nt", [seg(X, 0), seg(X, 1)], [seg(W, 0), seg(W, 1)], None, 3, out=out, workspace=ws),
        "workspace too small": lambda: gemm_seg("nt", [seg(X, 0), seg(X, 1)], [seg(W, 0), seg(W, 1)], None, 2, out=out, workspace=ws[:2 * M * N - 4]),
        "strided C with slabs": lambda: gemm_seg("nt", [seg(X, 0), seg(X, 1)], [seg(W, 0), seg(W, 1)], None, 2, out=X[:, :N], workspace=ws),
    }
    x0 = X.clone()
    for what, call in refused.items():
        with pytest.raises(IczError):
            call()
            pytest.fail("not refused: " + what)
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and torch.all(ws == 7.0) and torch.equal(X, x0)
    # and the same operands, legal, are taken
    got = gemm_seg("nt", [seg(X, 0), seg(X, 1)], [seg(W, 0), seg(W, 1)], bias, 2, out=out, workspace=ws)
    ref = X[:, :128].double() @ W[:, :128].double().t() + bias.double()
    assert _err(got, ref) < BOUND


@pytest.mark.parametrize("case", T.SWEEP, ids=lambda s: s[0])
def test_seeded_sweep_on_the_fp32_kernels(case):
    from simpleimagecaptionzoo_amd.butd import gemm_split_for
    name, layout, M, N, Ks, nsplit = case
    As, Bs, bias, ref = _operands(layout, M, N, Ks, 3000 + int(name[5:]))
    ns = 1 if nsplit == 1 else gemm_split_for(layout, M, N, Ks)
    out = _run(layout, M, N, As, Bs, bias, nsplit, ns)
    err = _err(out, ref)
    print("gemm_seg %s %s %d x %d x %s split %d -> %d: err %.3g" % (name, layout, M, N, Ks, nsplit, ns, err))
    assert torch.isfinite(out).all(), (case, "a load outside a segment's K range")
    assert err < BOUND, (case, ns, err)
    assert torch.equal(out, _run(layout, M, N, As, Bs, bias, nsplit, ns)), (case, "two runs differ")
