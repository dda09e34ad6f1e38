"""Host-side authority for tests/_gemm_segments.py: every case reaches the kernel it claims, at every split it runs, and the split
ranges said to hold a segment boundary do (recomputed here from the stage counts).  No GPU: the library's routing entries are host
logic.  A retuned threshold turns these red; tests/test_gpu_gemm_segments.py then no longer runs what its names say."""
import ctypes

import pytest

import _gemm_segments as T


def _ns(c, split):
    return c.picked if split == 0 else split


@pytest.mark.parametrize("c", [c for c in T.CASES if c.route != "x3"], ids=lambda c: c.name)
def test_case_reaches_its_route_at_every_split(c):
    from simpleimagecaptionzoo_amd.butd import GEMM_ROUTES, gemm_route_for, gemm_split_for
    assert c.route in GEMM_ROUTES
    assert gemm_split_for(c.layout, c.M, c.N, c.Ks) == c.picked
    for split in c.splits:
        assert gemm_route_for(c.layout, c.M, c.N, c.Ks, split) == c.route, (c.name, split)
    if not c.accumulate_only:
        assert 0 in c.splits


@pytest.mark.parametrize("c", [c for c in T.CASES if c.route == "x3"], ids=lambda c: c.name)
def test_many_row_case_reaches_the_split_precision_kernels_under_every_switch(c):
    from simpleimagecaptionzoo_amd.butd import gemm_route_for, gemm_set_big_cfg, gemm_split_for
    try:
        seen = set()
        for cfg in T.X3_CFGS:
            gemm_set_big_cfg(cfg)
            assert gemm_split_for(c.layout, c.M, c.N, c.Ks) == c.picked, (c.name, cfg)
            for split in c.splits:
                r = gemm_route_for(c.layout, c.M, c.N, c.Ks, split)
                assert r in T.X3_ROUTES[cfg], (c.name, cfg, split, r)
                seen.add(r)
        assert seen == {"x3_128tile", "large_tile"}
    finally:
        gemm_set_big_cfg(-2)


@pytest.mark.parametrize("c", T.CASES, ids=lambda c: c.name)
def test_split_ranges_cross_the_segment_boundaries_the_table_says(c):
    assert all(k % 4 == 0 for k in c.Ks)
    for split in c.splits:
        ns = _ns(c, split) if not c.accumulate_only else 1
        assert T.split_ranges(c.Ks, c.bk, ns) is not None, (c.name, split, "empty split")
        assert T.crossing_ranges(c.Ks, c.bk, ns) == c.crossing[ns], (c.name, split)
    if c.route == "resident_512deep":
        assert T.half_crossing(c.Ks, c.picked) == c.half_crossing, c.name
        assert sum(T.stages(c.Ks, 64)) == 8 * c.picked
    if c.route in ("resident_4stage", "resident_128row"):
        assert sum(T.stages(c.Ks, 64)) == 4 * c.picked


def test_stage_depths_are_the_library_s():
    """The depth a case counts its stages in is the kernel's: a split one above the stage count at that depth is refused (an empty
    split), the stage count itself is taken -- on the fp32 kernels, whose split is free."""
    from simpleimagecaptionzoo_amd.butd import gemm_route_for
    for c in T.CASES:
        if c.route not in T.FP32_ROUTES:
            continue
        tot = sum(T.stages(c.Ks, c.bk))
        assert gemm_route_for(c.layout, c.M, c.N, c.Ks, tot) == c.route, c.name
        assert gemm_route_for(c.layout, c.M, c.N, c.Ks, tot + 1) is None, c.name


def test_every_route_has_a_multi_segment_case_with_a_crossing_range_and_a_live_case():
    routes = {}
    for c in T.CASES:
        if len(c.Ks) > 1 and any(c.crossing[_ns(c, s)] for s in c.splits):
            routes.setdefault(c.route, c.name)
    want = {"nt_fp32_mt1", "nt_fp32_mt2", "nt_fp32_mt4", "resident_4stage", "resident_512deep", "resident_128row", "x3", "nn_fp32"}
    assert set(routes) == want, routes
    live_routes = {T.BY_NAME[n].route for n in T.LIVE_CASES}
    assert live_routes == want | {"tn_fp32_64"}
    # both pipelines of the fp32 NT kernel at 64-row tiles, with and without the K tail, and the spread variant at both ends
    kinds = {(c.bk, any(k % 64 for k in c.Ks), c.M <= 64 or c.M >= 1024) for c in T.CASES if c.route == "nt_fp32_mt4"}
    assert {(64, True, True), (128, False, False), (128, False, True)} <= kinds


def test_pair_problems_take_the_stage_form_the_table_says():
    from simpleimagecaptionzoo_amd.butd import gemm_route_for, gemm_split_for
    form = {8: "resident_512deep", 4: "resident_4stage"}
    for pa, pb, nsr, nranges in T.PAIRS:
        for (M, N, Ks) in (pa, pb):
            assert 33 <= M <= 64 and N >= 2048          # each problem routes to the resident kernel by itself
            assert gemm_route_for("nt", M, N, Ks, 0) == form[nsr], (M, N, Ks)
            assert gemm_split_for("nt", M, N, Ks) == nranges == sum(T.stages(Ks, 64)) // nsr
    (Ma, Na, Ka), (Mb, Nb, Kb) = T.PAIR_MIXED
    assert gemm_route_for("nt", Ma, Na, Ka, 0) == "resident_512deep" and gemm_route_for("nt", Mb, Nb, Kb, 0) == "resident_4stage"


def test_sweep_is_fixed_and_stays_on_the_fp32_kernels():
    from simpleimagecaptionzoo_amd.butd import gemm_route_for
    assert len(T.SWEEP) == 40 and T.SWEEP == T._sweep(40, T.SWEEP_SEED)
    assert T.SWEEP[0] == T.SWEEP_FIRST and T.SWEEP[-1] == T.SWEEP_LAST
    nsegs, layouts = set(), set()
    for name, layout, M, N, Ks, nsplit in T.SWEEP:
        assert 1 <= len(Ks) <= 4 and 1 <= M <= 130 and 1 <= N <= 300 and all(4 <= k <= 260 and k % 4 == 0 for k in Ks), name
        assert nsplit in (0, 1) and (nsplit == 1 or (M * N) % 4 == 0) and (layout == "nt" or N % 4 == 0), name
        assert gemm_route_for(layout, M, N, Ks, nsplit) in T.FP32_ROUTES, name
        nsegs.add(len(Ks))
        layouts.add(layout)
    assert nsegs == {1, 2, 3, 4} and layouts == {"nt", "nn"}


def test_segment_entry_refuses_bad_tables_before_any_launch():
    """nseg outside 1..4 and null tables: an error with a message, nothing dereferenced (the pointers here are not memory)."""
    from simpleimagecaptionzoo_amd._lib import lib
    L = lib()
    i32x5 = (ctypes.c_int32 * 5)(64, 64, 64, 64, 64)
    fake = (ctypes.c_void_p * 5)(*[4096] * 5)
    used = ctypes.c_int32(-7)
    call = lambda nseg, A, lda, B, ldb, K: L.icz_gemm_f32_seg(0, nseg, A, lda, B, ldb, K, None, None, 64, 8, 64, 1, 0, None, None, 0, ctypes.byref(used), None)
    for nseg in (0, 5, -1):
        assert call(nseg, fake, i32x5, fake, i32x5, i32x5) == -1
        assert b"nseg" in L.icz_last_error()
    for hole in range(5):
        args = [fake, i32x5, fake, i32x5, i32x5]
        args[hole] = None
        assert call(2, *args) == -1
        assert b"null segment table" in L.icz_last_error()
    assert L.icz_gemm_f32_seg(3, 1, fake, i32x5, fake, i32x5, i32x5, None, None, 64, 8, 64, 1, 0, None, None, 0, None, None) == -1
    assert used.value == -7
    assert L.icz_gemm_resident_pair(0, fake, i32x5, fake, i32x5, i32x5, 40, 2048, None, 0, None,
                                    1, fake, i32x5, fake, i32x5, i32x5, 40, 2048, None, 0, None, None, None) == -1
    assert L.icz_gemm_split_for(0, 8, 64, 0, i32x5, 0) == -1 and L.icz_gemm_split_for(0, 8, 64, 1, None, 0) == -1
