"""BUTD over adaptive region sets: per-image region counts and sets of up to 128 regions (icz_butd_set_regions, the <true> instances of
the attention kernels in csrc/butd_kernels.h).  tests/_butd_adaptive.py holds the shapes, the inputs and the references: oracle.butd run
per image on feats[i, :counts[i]].  Bounds are the project's standing ones -- tokens exact up to the excuse rules of _fullwidth.py, logits
2e-4, log-probs and loss 1e-4, alphas 1e-4, gradients under _fullwidth.check_grads_against_float64 (_butd_adaptive.check_grads says how
that rule sits inside the bound this feature was given)."""
import numpy as np
import pytest
import torch

import _butd_adaptive as ad
from _butd_adaptive import A, CAP, D, E, H, MAIN_COUNTS, MAIN_SEED, SMALL, T, V
from _fullwidth import _excuse_greedy, _excuse_sampled
from _philox import butd_rng_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _handle(seed=MAIN_SEED, R=CAP, max_rows=96, options=None, steps=T):
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    h = ButdHandle(R, D, H, E, A, V, max_rows, steps)
    h.bind({k: v.to(DEV) for k, v in ad.params_cpu(seed, R).items()})
    for k, v in (options or {}).items():
        h.set_option(k, v)
    return h


def _rb(feats, counts):
    from simpleimagecaptionzoo_amd.regions import RegionBatch
    return RegionBatch(feats.to(DEV), list(counts)) if counts is not None else feats.to(DEV)


def _explicit(arrays):
    from simpleimagecaptionzoo_amd.butd import make_rng
    u, em, am, om = arrays
    return make_rng(0, torch.tensor(u, device=DEV), *(torch.tensor(np.ascontiguousarray(m).astype(np.uint8), device=DEV) for m in (em, am, om)))


def _scst(h, fb, form, rng, reward):
    """one SCST forward + backward in the form -> ([outputs], loss, grads)"""
    if form == "merged":
        out = h.rollouts(fb, T, rng)
    elif form.startswith("sample_n"):
        out = h.sample_n(fb, 4, T, rng)
    else:
        out = h.sample(fb, T, rng)
    out = [x.clone() for x in out]
    grads = h.new_grads()
    loss, _ = h.sample_backward(torch.as_tensor(reward, device=DEV), grads)
    torch.cuda.synchronize()
    return out, loss.item(), grads


FORMS = {"sample": ({"merge_small": 0}, None, 1), "merged": ({"merge_small": 8}, SMALL, 1),
         "sample_n4": ({"group_att": 0}, SMALL, 4), "sample_n4_grouped": ({"group_att": 1}, SMALL, 4)}


def _form_case(form, counts=MAIN_COUNTS, regions=CAP):
    options, pick, K = FORMS[form]
    cs = tuple(counts[i] for i in pick) if pick else tuple(counts)
    feats = ad.batch(MAIN_SEED, tuple(counts), regions)
    feats = feats[list(pick)] if pick else feats
    rows = len(cs) * K
    rs = np.random.RandomState(17)
    reward = rs.randn(rows, 1).astype(np.float32).repeat(T, 1)
    return options, cs, feats, K, rows, reward


# ---- the main case: capacity 100, regions 100, 12 images -------------------------------------------------------------------------------
def test_greedy_ids_and_alphas_match_the_per_image_oracle():
    ref = ad.greedy_reference(ad.batch(MAIN_SEED, MAIN_COUNTS, CAP), MAIN_COUNTS)["f32"]
    h = _handle()
    ids, alphas = h.greedy(_rb(ad.batch(MAIN_SEED, MAIN_COUNTS, CAP), MAIN_COUNTS), 20, want_alphas=True)
    ids, alphas = ids.cpu().numpy(), alphas.cpu().numpy()
    excused = _excuse_greedy(ids, ref[0], ref[2], 1)
    ok = np.setdiff1d(np.arange(len(MAIN_COUNTS)), excused)
    print("greedy: excused rows", list(excused), "max|alpha - oracle|", float(np.abs(alphas[ok] - ref[1].numpy()[ok]).max()))
    np.testing.assert_allclose(alphas[ok], ref[1].numpy()[ok], atol=1e-4)
    for i, c in enumerate(MAIN_COUNTS):
        assert not alphas[i, :, c:].any(), (i, c)                  # exact zeros behind the count
        assert abs(float(alphas[i, 0].sum()) - 1.0) < 1e-5
    h.close()


@pytest.mark.parametrize("k", [3, 5, 8])
def test_beam_search_matches_the_per_image_oracle(k):
    """k = 3, 5, 8 rows per image on the grouped scores / context kernels (8 = ATT_CTX_MAX_G), per image, token for token"""
    images = (0, 1, 3, 4, 5, 7)                                    # counts 1, 2, 63, 64, 65, 100
    want = ad.beam_reference(ad.batch(MAIN_SEED, MAIN_COUNTS, CAP), MAIN_COUNTS, k, images)
    h = _handle()
    seqs, lens = h.beam_search(_rb(ad.batch(MAIN_SEED, MAIN_COUNTS, CAP), MAIN_COUNTS), k, 20)
    seqs, lens = seqs.cpu().numpy(), lens.cpu().numpy()
    for i in images:
        got = seqs[i, :lens[i]]
        assert got.shape == want[i].shape and np.array_equal(got, want[i]), (k, i, got.tolist(), want[i].tolist())
    h.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_scst_step_matches_the_per_image_oracle(form):
    """sample (12 images, explicit masks, 24 steps: two time passes of the d enc_ctx kernel), the merged chain of 3 images, sample_n with
    4 rows per image on the per-row and on the grouped kernels: tokens, log-probs, loss and every gradient"""
    options, cs, feats, K, rows, reward = _form_case(form)
    arrays = ad.rng_arrays(31, rows, CAP)
    ref = ad.scst_reference(feats, cs, K, reward, arrays)
    h = _handle(options=options)
    out, loss, grads = _scst(h, _rb(feats, cs), form, _explicit(arrays), reward)
    seq, lp = out[-2].cpu().numpy(), out[-1].cpu().numpy()
    w_seq, w_lp, w_lg, w_loss, _ = ref["f32"]
    same = _excuse_sampled(seq, w_seq, w_lg, arrays[0], 0)         # no row excused: the seeds were picked so (test_cpu_butd_adaptive.py)
    assert same.all() and np.array_equal(ref["f64"][0].numpy(), seq)
    np.testing.assert_allclose(lp, w_lp.numpy(), atol=1e-4)
    assert abs(loss - w_loss) < 1e-4, (loss, w_loss)
    if form == "merged":
        g = ad.greedy_reference(feats, cs, steps=T)["f32"]
        _excuse_greedy(out[0].cpu().numpy(), g[0], g[2], 0)
    ad.check_grads(form, grads, ref)
    h.close()


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_xe_step_matches_the_per_image_oracle(train):
    arrays = ad.rng_arrays(41, len(MAIN_COUNTS), CAP)
    caps, lengths, ref = ad.xe_reference(ad.batch(MAIN_SEED, MAIN_COUNTS, CAP), MAIN_COUNTS, arrays, train)
    h = _handle()
    from simpleimagecaptionzoo_amd.butd import make_rng
    rng = make_rng(0, None, *(torch.tensor(np.ascontiguousarray(m).astype(np.uint8), device=DEV) for m in arrays[1:])) if train else None
    logits = h.xe_forward(_rb(ad.batch(MAIN_SEED, MAIN_COUNTS, CAP), MAIN_COUNTS), caps.to(DEV), lengths, rng, train=train, want_logits=True)
    alphas = h.saved_alphas(len(MAIN_COUNTS), max(lengths)).cpu().numpy()         # (the backward pass consumes the stored forward pass)
    grads = h.new_grads()
    loss = h.xe_backward(grads, smoothing=0.1).item()
    w_logits, w_loss, _ = ref["f32"]
    np.testing.assert_allclose(logits.cpu().numpy(), w_logits.numpy(), atol=2e-4, rtol=1e-4)
    assert abs(loss - w_loss) < 1e-4, (loss, w_loss)
    ad.check_grads("xe " + ("train" if train else "eval"), grads, ref)
    for i, c in enumerate(MAIN_COUNTS):
        assert not alphas[i, :lengths[i], c:].any() and abs(float(alphas[i, 0].sum()) - 1.0) < 1e-5
    h.close()


# ---- fixed region sets of 65..128 regions, no counts: against oracle.butd directly ------------------------------------------------------
@pytest.mark.parametrize("R", [100, 128])
def test_wide_fixed_sets_match_the_oracle(R):
    from oracle import butd as ob
    counts = (R,) * 6
    feats, p = ad.wide_batch(R), ad.params_cpu(MAIN_SEED, R)
    h = _handle(R=R, max_rows=32)
    with torch.no_grad():
        w_ids, w_al, w_lg = ob.greedy(feats, p, 20, hoisted=True)
    ids, alphas = h.greedy(feats.to(DEV), 20, want_alphas=True)
    _excuse_greedy(ids.cpu().numpy(), w_ids, w_lg, 0)
    np.testing.assert_allclose(alphas.cpu().numpy(), w_al.numpy(), atol=1e-4)
    seqs, lens = h.beam_search(feats.to(DEV), 5, 20)
    for i in (0, 5):
        with torch.no_grad():
            want = ob.beam_search(feats[i:i + 1], p, 5, 20).numpy().ravel()
        assert np.array_equal(seqs[i, :int(lens[i])].cpu().numpy(), want), (R, i)
    # XE and SCST gradients: the per-image reference with counts = R is the oracle on each image's whole tensor
    arrays = ad.rng_arrays(51, 6, R)
    caps, lengths, ref = ad.xe_reference(feats, counts, arrays, True)
    from simpleimagecaptionzoo_amd.butd import make_rng
    rng = make_rng(0, None, *(torch.tensor(np.ascontiguousarray(m).astype(np.uint8), device=DEV) for m in arrays[1:]))
    logits = h.xe_forward(feats.to(DEV), caps.to(DEV), lengths, rng, train=True, want_logits=True)
    grads = h.new_grads()
    loss = h.xe_backward(grads, smoothing=0.1).item()
    np.testing.assert_allclose(logits.cpu().numpy(), ref["f32"][0].numpy(), atol=2e-4, rtol=1e-4)
    assert abs(loss - ref["f32"][1]) < 1e-4
    ad.check_grads("xe R=%d" % R, grads, ref)
    reward = np.random.RandomState(3).randn(6, 1).astype(np.float32).repeat(T, 1)
    sref = ad.scst_reference(feats, counts, 1, reward, arrays)
    h.set_option("merge_small", 0)
    out, loss, grads = _scst(h, feats.to(DEV), "sample", _explicit(arrays), reward)
    assert _excuse_sampled(out[0].cpu().numpy(), sref["f32"][0], sref["f32"][2], arrays[0], 0).all()
    assert np.array_equal(sref["f64"][0].numpy(), out[0].cpu().numpy())
    np.testing.assert_allclose(out[1].cpu().numpy(), sref["f32"][1].numpy(), atol=1e-4)
    assert abs(loss - sref["f32"][3]) < 1e-4
    ad.check_grads("scst R=%d" % R, grads, sref)
    h.close()


# ---- bit-for-bit invariants -------------------------------------------------------------------------------------------------------------
def _everything(h, fb, seed=77, philox=True):
    """greedy ids + alphas, beam 3, a Philox SCST step (sample) and a training-mode XE step: every output and gradient, cloned"""
    from simpleimagecaptionzoo_amd.butd import make_rng
    n = (fb.feats if hasattr(fb, "feats") else fb).shape[0]
    ids, al = h.greedy(fb, 20, want_alphas=True)
    res = [ids.clone(), al.clone()]
    res += [x.clone() for x in h.beam_search(fb, 3, 20)]
    reward = np.random.RandomState(2).randn(n, 1).astype(np.float32).repeat(T, 1)
    out, loss, grads = _scst(h, fb, "sample", make_rng(seed), reward)
    res += out + [torch.tensor(loss)] + [grads[k] for k in sorted(grads)]
    caps, lengths = ad.xe_case(MAIN_SEED, n)
    res.append(h.xe_forward(fb, caps.to(DEV), lengths, make_rng(seed + 1), train=True, want_logits=True).clone())
    grads = h.new_grads()
    res.append(h.xe_backward(grads, smoothing=0.1).clone())
    res += [grads[k] for k in sorted(grads)]
    torch.cuda.synchronize()
    return res


def _same(a, b):
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if x.shape != y.shape or not torch.equal(x.cpu(), y.cpu())]
    assert len(a) == len(b) and not bad, bad


@pytest.mark.parametrize("R", [36, 64])
def test_counts_equal_to_regions_change_nothing(R):
    """counts all equal to `regions` (the <true> kernels) against no counts (the fixed-set kernels), every output bit for bit"""
    feats = ad.batch(MAIN_SEED, (R,) * 5, R)
    h = _handle(R=R, max_rows=16, options={"merge_small": 0})
    plain = _everything(h, feats.to(DEV))
    counted = _everything(h, _rb(feats, (R,) * 5))
    _same(plain, counted)
    h.close()


def test_pad_rows_never_reach_a_result_and_runs_repeat():
    """pad rows of finite junk instead of zeros change no output and no gradient; two runs are bit-equal"""
    h = _handle(options={"merge_small": 0})
    feats = ad.batch(MAIN_SEED, MAIN_COUNTS, CAP)
    a = _everything(h, _rb(feats, MAIN_COUNTS))
    b = _everything(h, _rb(feats, MAIN_COUNTS))
    c = _everything(h, _rb(ad.junk_pads(feats, MAIN_COUNTS), MAIN_COUNTS))
    _same(a, b)
    _same(a, c)
    h.close()


def test_narrower_and_fixed_batches_on_a_capacity_100_handle_equal_a_fresh_handle():
    """37 regions on the capacity-100 handle = a fresh capacity-37 handle; a fixed 36-region batch after an adaptive one = the same
    batch on a fresh capacity-36 handle (nothing of the counted batch is left behind)"""
    h = _handle(options={"merge_small": 0})
    _everything(h, _rb(ad.batch(MAIN_SEED, MAIN_COUNTS, CAP), MAIN_COUNTS))
    for R in (37, 36):
        feats = ad.batch(MAIN_SEED + 1, (R,) * 5, R).to(DEV)
        fresh = _handle(R=R, max_rows=96, options={"merge_small": 0})
        _same(_everything(fresh, feats), _everything(h, feats))
        fresh.close()
    h.close()


def test_philox_mode_equals_the_regenerated_masks():
    """make_rng(seed) against the uniforms and keep-masks the numpy twin of csrc/rng.h builds for that seed with R = regions: the keep-bit
    index stays ((row * regions + r) * A + c) on a counted batch"""
    from simpleimagecaptionzoo_amd.butd import make_rng
    seed = 0x51ED5EED
    n = len(MAIN_COUNTS)
    arrays = butd_rng_arrays(seed, T, n, CAP, E, A, H)
    reward = np.random.RandomState(2).randn(n, 1).astype(np.float32).repeat(T, 1)
    h = _handle(options={"merge_small": 0})
    fb = _rb(ad.batch(MAIN_SEED, MAIN_COUNTS, CAP), MAIN_COUNTS)
    o1, l1, g1 = _scst(h, fb, "sample", make_rng(seed), reward)
    o2, l2, g2 = _scst(h, fb, "sample", make_rng(0, *(torch.tensor(x, device=DEV) for x in arrays)), reward)
    _same(o1 + [g1[k] for k in sorted(g1)], o2 + [g2[k] for k in sorted(g2)])
    assert l1 == l2
    h.close()


# ---- the Python layer and the refusals ---------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing():
    from simpleimagecaptionzoo_amd import _lib
    import ctypes as C
    h = _handle(max_rows=16)
    f = ad.batch(MAIN_SEED, (10, 10), 10).to(DEV)
    ids = h.greedy(f, 4).clone()
    for bad in ([0, 10], [11, 10]):                               # count 0, count > regions
        with pytest.raises(_lib.IczError, match="regions"):
            h.greedy(_rb(f, bad), 4)
    with pytest.raises(_lib.IczError):                            # regions above the capacity (Python check, then the library's)
        h.greedy(torch.zeros(2, CAP + 1, D, device=DEV), 4)
    assert _lib.lib().icz_butd_set_regions(h._h, CAP + 1, None, None, 0) == -1
    dev = torch.tensor([5, 5], dtype=torch.int32, device=DEV)
    host = (C.c_int32 * 2)(5, 5)
    assert _lib.lib().icz_butd_set_regions(h._h, 10, _lib.ptr(dev), None, 2) == -1       # one NULL pointer of the pair
    assert _lib.lib().icz_butd_set_regions(h._h, 10, None, host, 2) == -1
    h._set_regions(10, [5, 5])                                     # counts for 2 images, then a batch of 3
    f3 = ad.batch(MAIN_SEED, (10, 10, 10), 10).to(DEV)
    for call in (lambda: h._e.greedy(h._h, _lib.ptr(f3), 3, 4, _lib.ptr(torch.zeros(3, 4, dtype=torch.int64, device=DEV)), None, _lib.stream_ptr()),):
        assert call() == -1 and b"counts were set for 2 images" in _lib.lib().icz_last_error()
    with pytest.raises(_lib.IczError, match="region counts for"):
        h.greedy(_rb(f3, [5, 5]), 4)
    h._set_regions(10)                                            # the refused calls left the handle usable and unchanged
    assert torch.equal(h.greedy(f, 4), ids)
    h.close()


def test_captioner_region_masks_and_eval_test_image_alphas():
    """BUTDDetection_Captioner with region_masks = True: the sampler on a masked batch = the handle on the RegionBatch; region_masks=False
    ignores the mask (the reference's behaviour: the padded tensor, bit for bit); eval_test_image returns alphas of the batch's width
    with zeros behind the count."""
    from simpleimagecaptionzoo_amd.captioner import BUTDDetection_Captioner
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    counts = (7, 12, 3)
    feats = ad.batch(MAIN_SEED, counts, 12).to(DEV)
    masks = (torch.arange(12).unsqueeze(0) < torch.tensor(counts).unsqueeze(1)).float().to(DEV)
    sd = {"decoder." + k: v for k, v in ad.params_cpu(MAIN_SEED).items()}
    outs = {}
    for on in (False, True):
        cap = BUTDDetection_Captioner(A, E, H, V, enc_dim=D, num_regions=CAP, max_batch=4).to(DEV)
        cap.region_masks = on
        cap.load_state_dict(sd)
        cap.eval()
        outs[on] = cap.sampler({"bu_feats": feats, "bu_masks": masks}, 20).clone()
        if on:
            words, (al,) = cap.eval_test_image({"bu_feats": feats[:1], "bu_masks": masks[:1], "bu_counts": [7]}, synthetic_vocab(V))
            assert al.shape[0] == 1 and al.shape[2] == 12 and not al[0, :, 7:].any() and abs(float(al[0, 0].sum()) - 1) < 1e-5
            with pytest.raises(ValueError, match="leading run"):
                cap.sampler({"bu_feats": feats, "bu_masks": masks.flip(1)}, 20)
    h = _handle(max_rows=16)
    assert torch.equal(outs[True], h.greedy(_rb(feats, counts), 20))
    assert torch.equal(outs[False], h.greedy(feats, 20))
    h.close()


def test_butd_and_aoa_ensemble_takes_one_adaptive_batch():
    """a BUTD + AoA ensemble on one counted batch: a one-member 'ensemble' of the BUTD handle decodes what the handle decodes, and the
    two-member ensemble runs greedy and beam 3 with both members on their counts (rows of different counts finish, ids in range)"""
    from _fullwidth import _aoa_model
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    counts = (7, 12, 3, 12)
    feats = ad.batch(MAIN_SEED, counts, 12)
    hb = _handle(max_rows=16)
    aoa = _aoa_model((CAP, D, 64, E, V, 4), 16, 5).to(DEV)
    ha = aoa._handle()
    solo = EnsembleHandle([hb])
    assert torch.equal(solo.greedy([_rb(feats, counts)], 20), hb.greedy(_rb(feats, counts), 20))
    ens = EnsembleHandle([hb, ha])
    ids = ens.greedy([_rb(feats, counts), _rb(feats, counts)], 20)
    ids_junk = ens.greedy([_rb(ad.junk_pads(feats, counts), counts), _rb(feats, counts)], 20)
    assert torch.equal(ids, ids_junk) and int(ids.max()) < V
    seqs, lens, _ = ens.beam_search_opts([_rb(feats, counts), _rb(feats, counts)], 3, 20)
    seqs2, lens2, _ = ens.beam_search_opts([_rb(ad.junk_pads(feats, counts), counts), _rb(feats, counts)], 3, 20)
    assert torch.equal(seqs, seqs2) and torch.equal(lens, lens2) and bool((lens > 0).all())
    solo.close(), ens.close(), hb.close()


# ---- the Engine ----------------------------------------------------------------------------------------------------------------------------
class _Crit:
    smoothing = 0.1


ENG_COUNTS = (12, 7, 3, 12, 9)


def _engine(cider_df=None):
    from simpleimagecaptionzoo_amd.engine import BUTDDetection_Eng
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    eng = BUTDDetection_Eng({"model_type": "BUTDDetection", "atten_dim": A, "embed_dim": E, "hidden_dim": H, "enc_dim": D}, "SYN",
                            synthetic_vocab(V), data_dir="/tmp/", use_bu="adaptive", device="cuda:0", cider_df=cider_df, max_batch=8)
    eng.model.load_state_dict({"decoder." + k: v for k, v in ad.params_cpu(MAIN_SEED).items()})
    return eng


def _supp(feats, counts):
    return tuple({"bu_feat": feats[i, :c].numpy().copy(), "bu_bbox": np.zeros((c, 4), np.float32)} for i, c in enumerate(counts))


def _caption(ids, words):
    out = []
    for t in ids:
        if words[int(t)] == "<end>":
            break
        if words[int(t)] != "<sta>":
            out.append(words[int(t)])
    return " ".join(out)


def test_engine_use_bu_adaptive_end_to_end():
    """BUTDDetection_Eng(use_bu='adaptive') on ragged per-image features: capacity 100, region_masks on; the evaluation JSON (greedy and
    beam 3) = the entries built by hand from the per-image oracle; one XE step = the per-image oracle's loss; one SCST step trains"""
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    from simpleimagecaptionzoo_amd.butd import make_rng
    from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    n = len(ENG_COUNTS)
    feats = ad.batch(MAIN_SEED, ENG_COUNTS, max(ENG_COUNTS))
    vocab = synthetic_vocab(V)
    words = [vocab.ix2word[i] for i in range(V)]
    gts = synthetic_references(n, words, seed=5)
    eng = _engine(document_frequency(gts))
    assert eng.model.dims["R"] == CAP and eng.model.region_masks
    supp = _supp(feats, ENG_COUNTS)
    ref = ad.greedy_reference(feats, ENG_COUNTS)["f32"]
    res = eng.eval_captions_json_generation([(tuple(range(n)), None, supp)], eval_beam_size=-1, tqdm_visible=False)
    assert res == [{"image_id": i, "caption": _caption(ref[0][i], words)} for i in range(n)]
    beams = ad.beam_reference(feats, ENG_COUNTS, 3, range(n), steps=50)        # the Engine searches for up to 50 steps
    res = eng.eval_captions_json_generation([(tuple(range(n)), None, supp)], eval_beam_size=3, tqdm_visible=False)
    assert [r["caption"] for r in res] == [_caption(beams[i][1:], words) for i in range(n)]
    arrays = ad.rng_arrays(41, n, max(ENG_COUNTS))
    caps, lengths, xref = ad.xe_reference(feats, ENG_COUNTS, arrays, True)
    rng = make_rng(0, None, *(torch.tensor(np.ascontiguousarray(m).astype(np.uint8), device=DEV) for m in arrays[1:]))
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 4e-4}), 4e-4)
    losses = eng.training_epoch([(tuple(range(n)), None, caps, [l + 1 for l in lengths], supp)], opt, _Crit(), tqdm_visible=False, rngs=[rng])
    assert abs(losses[0].item() - xref["f32"][1]) < 1e-4, (losses[0].item(), xref["f32"][1])
    before = {k: v.clone() for k, v in eng.model.state_dict().items()}
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    losses = eng.SCST_training_epoch([(tuple(range(n)), None, gts, supp)], opt, None, tqdm_visible=False)
    assert np.isfinite(losses[0].item())
    now = eng.model.state_dict()
    assert any(not torch.equal(now[k], before[k]) for k in now)


def test_engine_adaptive_through_packed_store_and_prefetcher(tmp_path):
    """per-image adaptive .npz files -> ragged packed store -> DevicePrefetcher (padded batch + bu_counts in HBM) -> the same JSON as from
    the ragged host arrays, in one batch and in two batches of other widths"""
    import os
    from simpleimagecaptionzoo_amd.features import DevicePrefetcher, PackedFeatureStore, pack_npz_dir
    n = len(ENG_COUNTS)
    supp = _supp(ad.batch(MAIN_SEED, ENG_COUNTS, max(ENG_COUNTS)), ENG_COUNTS)
    root = str(tmp_path / "supp")
    os.makedirs(os.path.join(root, "adaptive_bu_feat"))
    os.makedirs(os.path.join(root, "adaptive_bu_bbox"))
    ids = [100 + i for i in range(n)]
    for i, s_ in zip(ids, supp):
        np.savez_compressed(os.path.join(root, "adaptive_bu_feat", "%d.npz" % i), feat=s_["bu_feat"])
        np.save(os.path.join(root, "adaptive_bu_bbox", "%d.npy" % i), s_["bu_bbox"])
    store = PackedFeatureStore(pack_npz_dir(root, ids, str(tmp_path / "packed"), kind="adaptive"))
    eng = _engine()
    want = eng.eval_captions_json_generation([(tuple(ids), None, supp)], eval_beam_size=-1, tqdm_visible=False)
    loader = [(tuple(ids[:2]), None, None), (tuple(ids[2:]), None, None)]
    assert eng.eval_captions_json_generation(DevicePrefetcher(loader, "cuda:0", store), eval_beam_size=-1, tqdm_visible=False) == want
    assert eng.eval_captions_json_generation(DevicePrefetcher([(tuple(ids), None, supp)], "cuda:0"), eval_beam_size=-1, tqdm_visible=False) == want


# ---- the decoder seams: sampling decode and scoring on a counted batch ---------------------------------------------------------------------
def test_sample_decode_and_score_captions_on_counts_match_the_host_oracles():
    """sample_decode (n = 1 and 3, two option sets) token-exact against _sampling_oracle over per-image step closures on feats[i, :c], its
    log-probs within 1e-4; score_captions of the drawn captions within 1e-4 of _scoring_oracle run per image"""
    import _sampling_oracle as so
    import _scoring_oracle as sc
    from simpleimagecaptionzoo_amd.scoring import score_captions
    counts = (7, 12, 3, 12)
    feats, p = ad.batch(MAIN_SEED, counts, 12), ad.params_cpu(MAIN_SEED)
    h = _handle(max_rows=16)
    for n, opts in ((1, (1.0, 0, 1.0)), (3, (0.8, 5, 0.9))):
        u = np.random.RandomState(60 + n).rand(20, len(counts) * n).astype(np.float32)
        ids, logp, _ = h.sample_decode(_rb(feats, counts), n, 20, *opts, rng=torch.tensor(u, device=DEV))
        w_ids, w_lp = so.decode_model("butd", feats, p, n, u, 20, *opts, counts=list(counts))
        assert np.array_equal(ids.cpu().numpy(), w_ids), (n, opts)
        np.testing.assert_allclose(logp.cpu().numpy(), w_lp, atol=1e-4, rtol=0)
        got, _ = score_captions(h, _rb(feats, counts), ids, n)
        want = np.concatenate([sc.score_model("butd", feats[i:i + 1, :c], p, n, w_ids[i * n:(i + 1) * n]) for i, c in enumerate(counts)])
        np.testing.assert_allclose(got.cpu().numpy(), want, atol=1e-4, rtol=0)
    h.close()
