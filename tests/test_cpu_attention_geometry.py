"""The table of attention shapes (tests/_fullwidth.py: ATT_GEOMETRY) without a GPU: every entry is there for what it says, every branch
condition of the nine attention kernels (csrc/butd_kernels.h: att_scores*, att_ctx*, att_bwd_*) is taken by one entry and not taken by
another, and on the committed seeds of tests/test_gpu_butd_attention.py the reference alone needs no excuse: its fp32 and float64
passes draw the same tokens in every row and no greedy step is a near-tie, so a device row that differs is the device's doing."""
import numpy as np
import pytest
import torch

from _fullwidth import (ATT_CTX_MAX_G, ATT_GEOMETRY, ATT_ROWS, ATT_SEEDS, ATT_STEPS, ATT_XE_LENGTHS, ATT_XE_SEEDS, MIDWIDTH, TT,  # noqa: E402
                        _butd_scst_inputs, _butd_scst_oracle, _butd_xe_inputs, att_branches, att_geometry_claims, relu_band_count)

NAMES = sorted(ATT_GEOMETRY)


@pytest.mark.parametrize("name", NAMES)
def test_every_shape_is_there_for_what_it_says(name):
    claims = att_geometry_claims(name)
    assert len(claims) >= 4 and all(claims.values()), [k for k, v in claims.items() if not v]
    assert name in ATT_SEEDS and len(ATT_GEOMETRY[name][1]) > 20


def test_every_branch_condition_is_taken_by_one_shape_and_not_by_another():
    table = {name: att_branches(dims) for name, (dims, _) in ATT_GEOMETRY.items()}
    # the step count is one number for the whole table: its other side (T <= TT, one time pass) is every case of the mid-width table
    table.update({name: att_branches(dims, steps=max(T for _, T, _ in cases)) for name, (dims, cases, _) in MIDWIDTH.items()})
    assert ATT_STEPS > TT and all(T <= TT for _, cases, _ in MIDWIDTH.values() for _, T, _ in cases)
    for cond in next(iter(table.values())):
        taken = [n for n in NAMES if table[n][cond]]
        other = [n for n in table if not table[n][cond]]
        assert taken and other, (cond, taken, other)
        if cond != "denc: second time pass (T > TT)":
            assert [n for n in NAMES if not table[n][cond]], (cond, "never false inside ATT_GEOMETRY")
    assert 2 <= 4 <= ATT_CTX_MAX_G and ATT_ROWS % 4 == 0          # the sample_n cases: 4 samples per image


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_reference_needs_no_excuse_on_the_committed_seeds(name, K):
    """what _butd_scst_case runs beside the device, alone: the rows of the fp32 and the float64 pass agree token for token (so every row
    takes part in the gradient comparison) and the two largest greedy logits are at least 1e-4 apart at every step (_excuse_greedy
    has nothing to excuse).  K = 4: the inputs of the sample_n cases (3 images, 4 rows each)."""
    dims = ATT_GEOMETRY[name][0]
    params, img_feats, feats_c, em, am, om, u, _ = _butd_scst_inputs(ATT_ROWS, ATT_STEPS, ATT_SEEDS[name], dims=dims, samples_per_image=K, device="cpu")
    out, w_greedy, w_glog = _butd_scst_oracle(params, img_feats, feats_c, em, am, om, u, ATT_STEPS)
    s32, s64 = out["f32"][1].numpy(), out["f64"][1].numpy()
    agree = (s32 == s64).all(1)
    assert agree.all(), (name, K, "rows whose fp32 / float64 draws differ", np.nonzero(~agree)[0])
    top2 = torch.topk(w_glog, 2, dim=2).values
    margin = float((top2[..., 0] - top2[..., 1]).min())
    assert margin >= 1e-4, (name, K, margin)
    assert torch.get_default_dtype() == torch.float32


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", [n for n in NAMES if n != "g_a2304"])
def test_xe_seeds_hold_no_relu_within_rounding_of_zero(name, train):
    """the XE cases (captions of 22..30 tokens, a token's embedding row fed once or twice): in float64 no kept attention pre-activation
    lies within 2e-7 (|enc_ctx| + |dec_ctx| + 1) of zero, so no fp32 evaluation can switch a relu the float64 pass has the other way"""
    from oracle import butd as ob
    dims = ATT_GEOMETRY[name][0]
    params, feats, caps, lengths, _, em, am, om = _butd_xe_inputs(dims, ATT_ROWS, ATT_XE_SEEDS[name], train, ATT_XE_LENGTHS, device="cpu")
    assert ATT_XE_LENGTHS[0] <= min(lengths) < max(lengths) <= ATT_XE_LENGTHS[1] and max(lengths) > TT
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            p = {k: v.double() for k, v in params.items()}
            trace = {}
            ob.forward_xe(feats.double(), caps, lengths, p, em, am, om, trace=trace)
            n = relu_band_count(feats.double(), p, trace["h1"], am, [sum(l > t for l in lengths) for t in range(max(lengths))])
    finally:
        torch.set_default_dtype(torch.float32)
    assert n == 0, (name, train, n)
