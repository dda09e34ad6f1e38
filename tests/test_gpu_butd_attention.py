"""BUTD attention at any region count and attention width, in both dropout modes.  tests/_fullwidth.py: ATT_GEOMETRY lists the shapes
and which branch of the nine attention kernels (csrc/butd_kernels.h: att_scores*, att_ctx*, att_bwd_*) each one takes;
tests/test_cpu_attention_geometry.py asserts that from the numbers.  Every shape runs ATT_ROWS = 12 rows x ATT_STEPS = 24 steps (two time
passes of att_bwd_denc_kernel<20>):

  explicit masks   one decoder step, greedy decoding with attention maps, beam search at k = 1, 2, 3, 5, 8, an SCST step in four forms
                   and an XE step on captions of 22..30 tokens in evaluation and in training mode -- against the CPU oracle in fp32 /
                   float64 under the rules of the golden, full-width and mid-width tests;
  Philox           the same device calls with make_rng(seed) and with the masks and uniforms a numpy twin of csrc/rng.h builds from that
                   seed: tokens, log-probs, loss and every gradient tensor bit for bit (forward and backward regenerate the keep-bits in
                   Philox mode, three kernels sharing one Philox call among lanes in three different ways).
"""
import functools

import numpy as np
import pytest
import torch

from _fullwidth import (ATT_GEOMETRY, ATT_ROWS, ATT_SEEDS, ATT_STEPS, ATT_XE_LENGTHS, ATT_XE_SEEDS, _butd_inputs, _butd_scst_case, _butd_scst_inputs, _butd_xe_case,  # noqa: E402
                        _end_biased_params, _full_params, _ragged_captions)
from _philox import butd_rng_arrays  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(ATT_GEOMETRY)
B, T = ATT_ROWS, ATT_STEPS
XE_LENGTHS = ATT_XE_LENGTHS
ATT_TENSORS = ("atten.enc_att.weight_v", "atten.enc_att.weight_g", "atten.enc_att.bias", "atten.dec_att.weight_v", "atten.dec_att.weight_g",
               "atten.dec_att.bias", "atten.affine.weight_v", "atten.affine.weight_g", "atten.affine.bias")


def _handle(dims, params, max_rows=B, options=None):
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    h = ButdHandle(*dims, max(max_rows, 8), T)
    h.bind(params)
    for k, v in (options or {}).items():
        h.set_option(k, v)
    return h


@functools.lru_cache(maxsize=None)
def _decode_case(name):
    """parameters, the 12 images of the shape's SCST case and the oracle's greedy decode of them (computed once, shared, left unchanged)"""
    from oracle import butd as ob
    dims = ATT_GEOMETRY[name][0]
    params, img_feats, *_ = _butd_scst_inputs(B, T, ATT_SEEDS[name], dims=dims)
    p = {k: v.detach().cpu() for k, v in params.items()}
    with torch.no_grad():
        ids, alphas, _ = ob.greedy(img_feats, p, T, hoisted=True)
    return dims, params, p, img_feats, ids.numpy(), alphas.numpy()


# ---- explicit masks: against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_attention_step_matches_float64_oracle(name):
    """h.step from an explicit state against oracle.butd.step in float64 under the rule of test_step_matches_reference (atol = rtol =
    1e-4): alpha, ctx, logits and the four states.  Every alpha row sums to 1 within 4 fp32 ulps; one region: alpha is exactly 1."""
    from oracle import butd as ob
    dims = ATT_GEOMETRY[name][0]
    R = dims[0]
    seed = ATT_SEEDS[name]
    params = _full_params(seed=seed, dims=dims)
    h = _handle(dims, params)
    feats_np, st_np, it_np = _butd_inputs(seed, B, dims)
    st = [torch.tensor(x, device="cuda") for x in st_np]
    ctx, alpha, logits = h.step(torch.tensor(feats_np, device="cuda"), torch.tensor(it_np, device="cuda"), *st)
    torch.cuda.synchronize()
    got = dict(zip(("h1", "c1", "h2", "c2"), (x.cpu().double().numpy() for x in st)), ctx=ctx.cpu().double().numpy(),
               alpha=alpha.cpu().double().numpy(), logits=logits.cpu().double().numpy())
    want = {}
    for dt in (torch.float32, torch.float64):
        with torch.no_grad():
            p = {k: v.detach().cpu().to(dt) for k, v in params.items()}
            f = torch.tensor(feats_np).to(dt)
            lg, al, state = ob.step(f, f.mean(1), torch.tensor(it_np), tuple(torch.tensor(x).to(dt) for x in st_np), p)
            cx = (f * al.unsqueeze(2)).sum(1)
        want[dt] = dict(zip(("h1", "c1", "h2", "c2"), (x.double().numpy() for x in state)), ctx=cx.double().numpy(), alpha=al.double().numpy(),
                        logits=lg.double().numpy())
    w32, w64 = want[torch.float32], want[torch.float64]
    for key in ("alpha", "ctx", "logits", "h1", "c1", "h2", "c2"):
        e_hip, e_t32 = float(np.abs(got[key] - w64[key]).max()), float(np.abs(w32[key] - w64[key]).max())
        print("step %s %-6s max|HIP - f64| %.3e  max|torch32 - f64| %.3e  ratio %.2f" % (name, key, e_hip, e_t32, e_hip / max(e_t32, 1e-30)))
    for key in ("alpha", "ctx", "logits", "h1", "c1", "h2", "c2"):
        np.testing.assert_allclose(got[key], w64[key], atol=1e-4, rtol=1e-4, err_msg=key)
    sums = alpha.cpu().double().sum(1)
    assert float((sums - 1.0).abs().max()) <= 4 * 2.0 ** -23, sums
    if R == 1:
        assert bool((alpha == 1.0).all())
    h.close()


@pytest.mark.parametrize("name", NAMES)
def test_attention_greedy_ids_and_alphas_match_oracle(name):
    """greedy(..., want_alphas=True): ids exact, attention maps within the 2e-5 of test_fullsize_greedy_matches_oracle"""
    dims, params, _, img_feats, want_ids, want_al = _decode_case(name)
    h = _handle(dims, params)
    ids, alphas = h.greedy(img_feats.cuda(), T, want_alphas=True)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    print("greedy", name, "max|alpha - oracle|", float(np.abs(alphas.cpu().numpy() - want_al).max()))
    np.testing.assert_allclose(alphas.cpu().numpy(), want_al, atol=2e-5)
    h.close()


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("name", NAMES)
def test_attention_beam_search_matches_oracle(name, k):
    """beam search over the 12 images (12 k decoder rows; the grouped scores / context kernels for k > 1) against the oracle's one-image
    beam search, per image, token for token, as test_beam5_at_125_rows_matches_oracle"""
    from oracle import butd as ob
    dims, params, p, img_feats, _, _ = _decode_case(name)
    h = _handle(dims, params, max_rows=B * k)
    seqs, lens = h.beam_search(img_feats.cuda(), k, 20)
    seqs, lens = seqs.cpu().numpy(), lens.cpu().numpy()
    for i in (0, 5, 11):
        want = ob.beam_search(img_feats[i:i + 1], p, k, 20).numpy().ravel()
        got = seqs[i, :lens[i]]
        assert got.shape == want.shape and np.array_equal(got, want), (name, k, i, got.tolist(), want.tolist())
    h.close()


SCST_FORMS = {"plain": ({"merge_small": 0}, 1), "merged": ({"merge_small": 32}, 1),
              "sample_n4": ({"group_att": 0}, 4), "sample_n4_grouped": ({"group_att": 1}, 4)}


@pytest.mark.parametrize("form", sorted(SCST_FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_attention_scst_step_matches_oracle(name, form):
    """_butd_scst_case at the shape: two chains, the merged chain (row0 > 0), 4 samples per image on the per-row and on the grouped
    attention kernels; every gradient under check_grads_against_float64, unchanged -- that rule is the whole check: at 64 hidden units and up
    to 2304 attention units one relu at zero moves a unit's gradient by more than the 2e-2 the mid-width tests see, in the fp32 oracle as
    on the device, and the rule holds the device to twice the oracle's own error there.  One region: the attention gradients are identically
    zero in float64 and come back within that rule's floor."""
    options, K = SCST_FORMS[form]
    excused = {}
    rep, kink = _butd_scst_case(B, T, ATT_SEEDS[name], options=options, dims=ATT_GEOMETRY[name][0], samples_per_image=K, excused=excused)
    zero = [k for k in rep if k in ATT_TENSORS] if ATT_GEOMETRY[name][0][0] == 1 else []
    worst = max((k for k in rep if k not in zero), key=lambda k: rep[k][0])
    print("scst", name, form, "excused", excused, "kink units", int(kink.sum()), "worst |HIP - f64| / max, beside torch32's, units outside:", worst, rep[worst])
    # one region: no unit of an attention tensor outside the rule (its floor: 1e-7 + 2 |torch32 - f64|), none excused as a relu kink
    assert all(rep[k][2] == 0 for k in zero) and len(zero) == (8 if zero else 0), rep


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", NAMES)
def test_attention_xe_step_matches_oracle(name, train):
    """_butd_xe_case on captions of 22..30 tokens (more steps than one time pass of att_bwd_denc_kernel, the batch shrinking with t), in
    evaluation mode and in training mode with explicit embedding, attention and output masks"""
    rep, kink = _butd_xe_case(ATT_GEOMETRY[name][0], B, seed=ATT_XE_SEEDS[name], train=train, length_range=XE_LENGTHS)
    worst = max(rep, key=lambda k: rep[k][0])
    print("xe", name, "train" if train else "eval", "kink units", int(kink.sum()), "worst", worst, rep[worst])


@pytest.mark.parametrize("name", NAMES)
def test_attention_sample_n_routes_draw_the_same_bits(name):
    """sample_n with 4 samples per image on the per-row attention kernels and on the grouped ones (option group_att): the grouped kernels
    promise the per-row kernels' arithmetic and summation order per row (csrc/butd_kernels.h), so tokens and log-probs are the same bit
    for bit -- as tests/test_gpu_scst_multisample.py holds them at 36 regions, here at odd and tiny region counts and every width."""
    from simpleimagecaptionzoo_amd.butd import make_rng
    dims, params, _, img_feats, _, _ = _decode_case(name)
    h = _handle(dims, params)
    feats = img_feats[:B // 4].cuda()
    runs = []
    for group in (0, 1):
        h.set_option("group_att", group)
        seq, lp = h.sample_n(feats, 4, T, make_rng(_philox_seed(name)))
        runs.append((seq.clone(), lp.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (name, float((runs[0][1] - runs[1][1]).abs().max()))
    assert bool((runs[0][1] < 0).any())
    h.close()


# ---- Philox mode equals explicit-mask mode, bit for bit -------------------------------------------------------------------------------
PHILOX_FORMS = ("sample", "merged", "sample_n4", "sample_n4_grouped", "xe_train", "end_biased")
PHILOX_T = max(T, XE_LENGTHS[1])


def _philox_seed(name):
    return 0x1234ABCD5678 + 0x100000001 * ATT_SEEDS[name]


@functools.lru_cache(maxsize=None)
def _twin(name):
    """what Philox mode draws at the shape for 12 rows and up to 30 steps, from the numpy twin (once per shape, shared by the forms)"""
    R, D, H, E, A, V = ATT_GEOMETRY[name][0]
    return butd_rng_arrays(_philox_seed(name), PHILOX_T, B, R, E, A, H)


@pytest.mark.parametrize("form", PHILOX_FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_attention_philox_mode_equals_explicit_masks(name, form):
    """One handle, one call sequence twice: with make_rng(seed), and with the uniforms and keep-masks of the numpy twin of csrc/rng.h for
    that seed.  sample + sample_backward; rollouts on the merged chain (row0 > 0); sample_n with 4 samples per image on both attention
    routes; training-mode xe_forward + xe_backward on captions of 22..30 tokens; sample with a raised <end> logit (rows finish early and
    the early-out of the dead steps fires).  Every output and every gradient tensor is the same, bit for bit."""
    from simpleimagecaptionzoo_amd.butd import make_rng
    dims = ATT_GEOMETRY[name][0]
    R, D, H, E, A, V = dims
    seed = _philox_seed(name)
    if form == "end_biased":
        params, feats = _end_biased_params(ATT_SEEDS[name], 0.3, B=B, dims=dims)
    else:
        params, img_feats, *_ = _butd_scst_inputs(B, T, ATT_SEEDS[name], dims=dims)
        feats = (img_feats[:B // 4] if form.startswith("sample_n4") else img_feats).cuda()
    options = {"merged": {"merge_small": 32}, "sample_n4": {"group_att": 0}, "sample_n4_grouped": {"group_att": 1}}.get(form, {"merge_small": 0})
    h = _handle(dims, params, options=options)
    g = torch.Generator(device="cpu")
    g.manual_seed(ATT_SEEDS[name])
    reward = torch.randn(B, T, generator=g).cuda()
    steps = T
    if form == "xe_train":
        caps, lengths = _ragged_captions(B, V, ATT_SEEDS[name], XE_LENGTHS)
        steps = max(lengths)
        assert steps > 20 and min(lengths) < steps
    u, em, am, om = (x[:steps] for x in _twin(name))
    assert 0.45 < am.mean() < 0.55 and 0.4 < em.mean() < 0.6 and 0.4 < om.mean() < 0.6
    dev = "cuda"
    explicit = make_rng(0, torch.tensor(u, device=dev), torch.tensor(em, device=dev), torch.tensor(am, device=dev), torch.tensor(om, device=dev))

    def run(rng):
        if form == "xe_train":
            out = [h.xe_forward(feats, caps.cuda(), lengths, rng, train=True, want_logits=True).clone()]
            grads = h.new_grads()
            loss = h.xe_backward(grads, smoothing=0.1)
        else:
            if form == "merged":
                out = h.rollouts(feats, T, rng)
            elif form.startswith("sample_n4"):
                out = h.sample_n(feats, 4, T, rng)
            else:
                out = h.sample(feats, T, rng)
            out = [x.clone() for x in out]
            grads = h.new_grads()
            loss, _ = h.sample_backward(reward, grads)
        torch.cuda.synchronize()
        return out, loss.item(), grads

    out1, loss1, g1 = run(make_rng(seed))
    out2, loss2, g2 = run(explicit)
    for a, b in zip(out1, out2):
        assert torch.equal(a, b), (name, form, "outputs differ", int((a != b).sum()))
    assert loss1 == loss2, (loss1, loss2)
    differ = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not differ, (name, form, differ, [float((g1[k] - g2[k]).abs().max()) for k in differ])
    assert all(torch.isfinite(v).all() for v in g1.values())
    assert any(float(v.abs().max()) > 0 for k, v in g1.items() if k not in ATT_TENSORS)
    if R > 1:           # one region: alpha = 1 whatever the scores are, the attention block's gradients are exactly zero
        assert all(float(g1[k].abs().max()) > 0 for k in ATT_TENSORS if k != "atten.affine.bias")
    if form == "end_biased":
        seq = out1[0]
        assert bool((seq[:, T - 2] == 0).all()) and bool((seq[:, 0] != 0).any())       # every row done before the last step: dead steps
    h.close()
