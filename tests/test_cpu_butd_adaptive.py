"""BUTD over adaptive region sets, the part that needs no GPU: the committed seeds of tests/_butd_adaptive.py give a per-image reference
that needs no excuse, and the Python plumbing (RegionBatch, counts_from_masks, the Captioner's region_masks switch, argument errors)."""
import numpy as np
import pytest
import torch

import _butd_adaptive as ad
from _butd_adaptive import CAP, D, MAIN_COUNTS, MAIN_SEED, SMALL, T


def test_greedy_reference_needs_no_excuse():
    """fp32 and float64 passes of the per-image oracle draw the same tokens in every row, and the two largest greedy logits differ by at
    least 1e-4 at every step (the rule of test_cpu_attention_geometry.py): a device row that differs cannot be a near-tie"""
    feats = ad.batch(MAIN_SEED, MAIN_COUNTS, CAP)
    for f, counts, steps in ((feats, MAIN_COUNTS, 20), (feats[list(SMALL)], tuple(MAIN_COUNTS[i] for i in SMALL), T)):
        ref = ad.greedy_reference(f, counts, steps=steps)
        assert torch.equal(ref["f32"][0], ref["f64"][0])
        top2 = torch.topk(ref["f32"][2], 2, dim=2).values
        margin = float((top2[..., 0] - top2[..., 1]).min())
        print("smallest greedy margin over %d images x %d steps: %.3e" % (len(counts), steps, margin))
        assert margin >= 1e-4
    for R in (100, 128):
        f = ad.wide_batch(R)
        ref = ad.greedy_reference(f, (R,) * 6)
        top2 = torch.topk(ref["f32"][2], 2, dim=2).values
        assert torch.equal(ref["f32"][0], ref["f64"][0]) and float((top2[..., 0] - top2[..., 1]).min()) >= 1e-4


@pytest.mark.parametrize("case", ["sample", "small_k1", "small_k4", "wide100", "wide128"])
def test_sampled_reference_needs_no_excuse(case):
    """the sampled rollouts of the GPU file: fp32 and float64 draw the same tokens, and no draw lies within 1e-6 of a CDF boundary"""
    if case.startswith("wide"):
        R = int(case[4:])
        counts, K, seed = (R,) * 6, 1, 51
        feats = ad.wide_batch(R)
    else:
        K, seed, R = (4 if case == "small_k4" else 1), 31, CAP
        feats = ad.batch(MAIN_SEED, MAIN_COUNTS, CAP)
        counts = MAIN_COUNTS
        if case != "sample":
            feats, counts = feats[list(SMALL)], tuple(MAIN_COUNTS[i] for i in SMALL)
    rows = len(counts) * K
    arrays = ad.rng_arrays(seed, rows, R)
    ref = ad.scst_reference(feats, counts, K, np.zeros((rows, T), np.float32), arrays)
    assert torch.equal(ref["f32"][0], ref["f64"][0])
    seq, lg = ref["f64"][0], ref["f64"][2]
    worst = 1.0
    for b in range(rows):
        for t in range(T):
            c = torch.cumsum(torch.softmax(lg[b, t], 0), 0)
            worst = min(worst, float((c[:-1] - float(arrays[0][t, b]) * float(c[-1])).abs().min()))
            if int(seq[b, t]) == 0:
                break
    print(case, "closest draw to a CDF boundary: %.3e" % worst)
    assert worst >= 1e-6


def test_region_batch_plumbing():
    from simpleimagecaptionzoo_amd import aoa, regions
    assert aoa.RegionBatch is regions.RegionBatch and aoa.counts_from_masks is regions.counts_from_masks
    m = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.float32)
    assert regions.counts_from_masks(m) == [3, 5]
    with pytest.raises(ValueError, match="leading run"):
        regions.counts_from_masks(m.flip(1))
    f = torch.zeros(2, 5, D)
    assert regions.region_features({"bu_feats": f, "bu_masks": None}) is not None
    assert torch.equal(regions.region_features({"bu_feats": f, "bu_masks": None}), f)
    rb = regions.region_features({"bu_feats": f, "bu_masks": m})
    assert isinstance(rb, regions.RegionBatch) and rb.counts == [3, 5]
    rb = regions.region_features({"bu_feats": f, "bu_masks": m, "bu_counts": (3, 5)})
    assert rb.counts == [3, 5]                                       # the Engine's counts are taken as they are: the mask is not read


def test_captioner_region_masks_switch():
    from simpleimagecaptionzoo_amd.captioner import BUTDDetection_Captioner
    from simpleimagecaptionzoo_amd.regions import RegionBatch
    f = torch.zeros(2, 5, D)
    m = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.float32)
    vi = {"bu_feats": f, "bu_masks": m}
    off = BUTDDetection_Captioner(16, 8, 8, 11, enc_dim=D, num_regions=CAP)
    assert off.region_masks is False and off._features(vi) is f     # the reference's behaviour: the mask is ignored
    on = BUTDDetection_Captioner(16, 8, 8, 11, enc_dim=D, num_regions=CAP)
    on.region_masks = True
    got = on._features(vi)
    assert isinstance(got, RegionBatch) and got.counts == [3, 5]
    with pytest.raises(ValueError, match="leading run"):
        on._features({"bu_feats": f, "bu_masks": m.flip(1)})
    assert on._features({"bu_feats": f, "bu_masks": None}) is not None and not isinstance(on._features({"bu_feats": f, "bu_masks": None}), RegionBatch)


def test_feature_check_errors_without_a_library_call():
    """RegionSets._feats refuses before it calls the library: wrong device / dtype / rank / width, more regions than the capacity"""
    from simpleimagecaptionzoo_amd import _lib
    from simpleimagecaptionzoo_amd.regions import RegionBatch, RegionSets

    class Stub(RegionSets):
        R, D = CAP, D

        def _set_regions(self, regions, counts=None):
            raise AssertionError("reached the library")

    s = Stub()
    for bad in (torch.zeros(2, 5, D), torch.zeros(2, 5, D, dtype=torch.float64), torch.zeros(2, D)):
        with pytest.raises(_lib.IczError, match="bu_feats must be"):
            s._feats(bad)
    with pytest.raises(_lib.IczError, match="bu_feats must be"):
        s._feats(RegionBatch(torch.zeros(2, CAP + 1, D), [1, 1]))


def test_create_entries_refuse_before_touching_the_device():
    """icz_butd_create keeps its bound of 64 regions; icz_butd_create_regions takes a capacity of up to 128"""
    import ctypes
    from simpleimagecaptionzoo_amd._lib import ButdDims, lib
    L, h = lib(), ctypes.c_void_p()
    assert L.icz_butd_create(ctypes.byref(ButdDims(65, D, 64, 32, 256, 203, 8, 20)), ctypes.byref(h)) == -1
    assert b"R=65" in L.icz_last_error() and b"icz_butd_create_regions" in L.icz_last_error()
    for bad in (129, 0):
        assert L.icz_butd_create_regions(ctypes.byref(ButdDims(bad, D, 64, 32, 256, 203, 8, 20)), ctypes.byref(h)) == -1
        assert ("R=%d" % bad).encode() in L.icz_last_error()
    assert L.icz_butd_create_regions(None, ctypes.byref(h)) == -1
