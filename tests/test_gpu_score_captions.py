"""GPU tests of scoring given captions (include/icz.h: icz_*_score_captions; simpleimagecaptionzoo_amd/scoring.py):
score_tokens_kernel alone against float64 on the same fp32 inputs, whole passes of the BUTD, AoA and NIC decoders against the host
oracle of tests/_scoring_oracle.py on captions that walk every branch of the length rule, the identities with what exists (the
sampling decode's own log-probs, the beam scores, xe_forward, n captions = repeated features, one-member ensembles and identical
copies, run-to-run bits), a full-width BUTD pass, the refusals and the Engine methods.  Scoring selects nothing: no row is excused."""
import ctypes as C
import gc
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ens_sampling_cases as ec  # noqa: E402
import _scoring_oracle as sco  # noqa: E402
import test_gpu_beam_opts as tbo  # noqa: E402
import test_gpu_ensemble as tge  # noqa: E402
import test_gpu_ensemble_sampling as tges  # noqa: E402
import test_gpu_sampling as tgs  # noqa: E402
from oracle import butd as ob  # noqa: E402

T = 8
GOLDENS = ["butd_dec_tiny", "butd_dec_odd", "aoa_tiny", "nic_dec_tiny", "nic_dec_odd"]


def _kernel_err(got, want):
    """the project's rule for such kernels (tests/test_gpu_ensemble.py, tests/test_gpu_sampling.py:62): 1e-6 absolute, widened by
    two fp32 ulps of the value -> what is left of the error above the widening"""
    return abs(float(got) - want) - abs(want) * 2.0 ** -22


def _targets(full):
    """per row the targets 0, V - 1, the argmax and the argmin of the first member's row -> [4][rows]"""
    x = full[0] if isinstance(full, list) else full
    rows, V = x.shape
    return [np.zeros(rows, np.int64), np.full(rows, V - 1, np.int64), x.argmax(1).astype(np.int64), x.argmin(1).astype(np.int64)]


# ---- the kernel alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [53, 1000, 10102, 40003])
@pytest.mark.parametrize("form", ["finished", "unpadded", "slabs2", "slabs4"])
def test_kernel_against_float64(V, form):
    """40 003 lies above the sampling kernel's LDS cap: this kernel holds no row"""
    from simpleimagecaptionzoo_amd.scoring import score_tokens
    for rows in (1, 5):
        rs = np.random.RandomState(V + rows)
        x = (rs.randn(rows, V) * 3.0).astype(np.float32)
        dev, bias, ns, ld, full = tgs._forms(x, form, rs)
        for k, tg in enumerate(_targets(full)):
            got = score_tokens(dev, bias, ns, ld, rows, V, torch.tensor(tg).cuda()).cpu().numpy()
            for r in range(rows):
                err = _kernel_err(got[r], sco.row_logp(full[r], int(tg[r])))
                print("kernel V=%d %s rows=%d target kind %d row %d err %.3g" % (V, form, rows, k, r, err))
                assert err <= 1e-6, (V, form, rows, k, r, float(got[r]))
        # a target outside [0, V) is never used as an index: the row reports 0
        bad = torch.tensor(([-1, V, 2 ** 40, -2 ** 40, V + 7] * rows)[:rows]).cuda()
        assert (score_tokens(dev, bias, ns, ld, rows, V, bad) == 0).all()


@pytest.mark.parametrize("V", [53, 1000, 10102, 40003])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_ensemble_kernel_against_float64(V, M):
    """mixed views (member m's form rotates through finished rows, unpadded rows, 2 slabs, 4 slabs) under uniform, unequal and
    one-zero weights"""
    from simpleimagecaptionzoo_amd.scoring import ensemble_score_tokens
    for rows in (1, 5):
        for vi in ((0, 1) if M < 4 else (0,)):
            members, full = tges._kernel_members(V, M, rows, vi, 1000 * V + 10 * M + rows + vi)
            for weights in tges._weight_sets(M):
                for k, tg in enumerate(_targets(full)):
                    got = ensemble_score_tokens(members, weights, rows, V, torch.tensor(tg).cuda()).cpu().numpy()
                    for r in range(rows):
                        err = _kernel_err(got[r], sco.ensemble_row_logp([f[r] for f in full], weights, int(tg[r])))
                        assert err <= 1e-6, (V, M, rows, vi, weights, k, r, float(got[r]), err)
            bad = torch.tensor(([V, -1, 2 ** 33, V + 1, -V] * rows)[:rows]).cuda()
            assert (ensemble_score_tokens(members, None, rows, V, bad) == 0).all()


# ---- whole passes against the host oracle ---------------------------------------------------------------------------------------
def _captions(rows, V, seed, early=False):
    """ids [rows, T] whose rows rotate through every branch of the length rule; early: every row ends by step 3"""
    rs = np.random.RandomState(seed)
    w = lambda k: rs.randint(3, V, size=k).tolist()           # words: neither <pad>, <sta> nor <end>
    kinds = [
        lambda: [2] + w(T - 1),                               # <end> as the first token, garbage behind it
        lambda: w(T),                                         # no <end> within max_len
        lambda: [0] * T,                                      # an empty caption
        lambda: w(1) + [0] + w(1) + [2] + [0] * (T - 4),      # a 0 in front of a later 2
        lambda: w(3) + [2] + [0] * (T - 4),                   # the plain case
        lambda: w(2) + [2] + w(2) + [0] + w(1) + [2],         # garbage (valid ids) behind the end
        lambda: w(T - 1) + [2],                               # <end> in the last column
        lambda: [0, 2] + w(T - 2),                            # empty, with an <end> and garbage behind the 0
        lambda: w(2) + [0] * (T - 2),                         # no <end>: the first 0 ends it
        lambda: [1] + w(2) + [2] + [0] * (T - 4),             # <sta> (1) is an ordinary word inside a caption
    ]
    if early:
        kinds = [lambda: [2] + w(T - 1), lambda: w(2) + [2] + w(T - 3), lambda: [0] * T, lambda: w(1) + [0] + w(T - 2),
                 lambda: w(3) + [0] * (T - 3), lambda: w(1) + [2] + [0] * (T - 2)]
    off = rs.randint(len(kinds))
    return np.array([kinds[(off + r) % len(kinds)]() for r in range(rows)], np.int64)


def _check_pass(got, want, ids, V, label):
    logp, score = got[0].cpu().numpy(), got[1].cpu().numpy()
    lens = sco.lengths(ids, V)
    scored = np.arange(ids.shape[1])[None, :] < lens[:, None]
    err = np.abs(logp - want)[scored].max() if scored.any() else 0.0
    print("%s: %d tokens, max logp err %.3g" % (label, int(scored.sum()), err))
    assert err <= 1e-4, (label, err)                          # the project's rule for log-probs
    assert (logp[~scored] == 0).all(), label                  # zeros are exact
    for r in range(ids.shape[0]):                             # the fp32 sum of the row's own log-probs in step order, bit for bit
        acc = np.float32(0)
        for t in range(lens[r]):
            acc = np.float32(acc + logp[r, t])
        assert np.float32(score[r]).tobytes() == np.float32(acc).tobytes(), (label, r, float(score[r]), float(acc))
    return lens


@pytest.mark.parametrize("name", GOLDENS)
def test_passes_against_the_oracle(golden_dir, name):
    from simpleimagecaptionzoo_amd.scoring import score_captions
    model, h, p, feats = tbo._setup(golden_dir, name, "nat")
    seen = set()
    for n, seeds in ((1, (1, 2, 3, 4)), (3, (5, 6))):
        for seed in seeds:
            ids = _captions(feats.shape[0] * n, h.V, seed)
            got = score_captions(h, feats, ids, n)
            lens = _check_pass(got, sco.score_model(model, feats.cpu(), p, n, ids), ids, h.V, "%s n=%d seed %d" % (name, n, seed))
            seen |= {(int(l), int(ids[r, 0]) == 2, bool((ids[r, l:] != 0).any()) if l < T else False) for r, l in enumerate(lens)}
        # every row ends by step 3: the early-out fires and the remaining columns are 0
        ids = _captions(feats.shape[0] * n, h.V, 40 + n, early=True)
        got = score_captions(h, feats, ids, n)
        lens = _check_pass(got, sco.score_model(model, feats.cpu(), p, n, ids), ids, h.V, "%s n=%d early" % (name, n))
        assert lens.max() <= 3 and (got[0][:, 3:] == 0).all()
    assert {0, 1, T} <= {s[0] for s in seen} and any(s[1] for s in seen) and any(s[2] for s in seen)      # the branches were walked
    h.close()


def test_pass_aoa_with_region_counts(golden_dir):
    from simpleimagecaptionzoo_amd.aoa import RegionBatch
    from simpleimagecaptionzoo_amd.scoring import score_captions
    model, h, p, feats = tbo._setup(golden_dir, "aoa_tiny", "nat")
    counts = [36, 20, 11]
    for n in (1, 3):
        for seed in (11, 12):
            ids = _captions(3 * n, h.V, seed)
            got = score_captions(h, RegionBatch(feats, counts), ids, n)
            _check_pass(got, sco.score_model(model, feats.cpu(), p, n, ids, counts=counts), ids, h.V, "aoa counts n=%d seed %d" % (n, seed))
    h.close()


@pytest.mark.parametrize("case", ["butd2", "mixed3", "aoa2_counts"])
def test_ensemble_passes_against_the_oracle(golden_dir, case):
    from simpleimagecaptionzoo_amd.scoring import score_captions
    specs, weights, counts = ec.CASES[case]
    ens, dev, _, V = tges._build(golden_dir, case)
    members = [ec.host_member(golden_dir, name, seed)[:3] for name, seed in specs]
    for n in (1, 3):
        for seed in (21, 22):
            ids = _captions(ec.N_IMG * n, V, seed)
            got = score_captions(ens, dev, ids, n)
            _check_pass(got, sco.score_ensemble(members, weights, n, ids, counts), ids, V, "%s n=%d seed %d" % (case, n, seed))
        ids = _captions(ec.N_IMG * n, V, 60 + n, early=True)
        got = score_captions(ens, dev, ids, n)
        _check_pass(got, sco.score_ensemble(members, weights, n, ids, counts), ids, V, "%s n=%d early" % (case, n))
        assert (got[0][:, 3:] == 0).all()


# ---- identities with what exists ------------------------------------------------------------------------------------------------
def _step_sums(logp, lens):
    """the fp32 sum of each row's log-probs in step order, as both kernels keep score_out"""
    out = np.zeros(logp.shape[0], np.float32)
    for r in range(logp.shape[0]):
        acc = np.float32(0)
        for t in range(lens[r]):
            acc = np.float32(acc + logp[r, t])
        out[r] = acc
    return out


def _sampled_agree(score_fn, ids, logp, score, label, single=False):
    """scoring the ids a sampling decode drew gives its log-probs and its score back within 1e-4.  The sampler may draw <pad> (0) and
    go on, a given caption ends at its first 0: the tokens are compared up to the scored length, the sums on the rows where the two
    lengths agree (most rows).  single: the single-model instances, where more holds -- see the test that asks for it."""
    got_lp, got_sc = [x.cpu().numpy() for x in score_fn(ids)]
    ids, logp, score = ids.cpu().numpy(), logp.cpu().numpy(), score.cpu().numpy()
    lens = sco.lengths(ids)
    scored = np.arange(ids.shape[1])[None, :] < lens[:, None]
    whole = (scored == (logp != 0)).all(1)
    assert whole.sum() * 2 > len(whole), label                 # most rows are compared in full
    err = np.abs(got_lp - logp)[scored].max()
    err_sc = np.abs(got_sc - score)[whole].max()
    same_tok = ((got_lp == logp) | ~scored).all(1)
    print("%s: sampled log-probs reproduced, max err %.3g, score max err %.3g, %d of %d rows whole, bit-equal tokens %d of %d, rows %d" % (
        label, err, err_sc, whole.sum(), len(whole), int((got_lp == logp)[scored].sum()), int(scored.sum()), int(same_tok.sum())))
    assert err <= 1e-4, (label, err)
    assert err_sc <= 1e-4, (label, err_sc)
    if single:
        want = logp
        assert (np.abs(got_lp - want) - np.abs(want) * 2.0 ** -21)[scored].max() <= 2e-6, label
        # both kernels keep the score as the fp32 sum of their own log-probs in step order ...
        assert np.array_equal(got_sc.view(np.uint32), _step_sums(got_lp, lens).view(np.uint32)), label
        assert np.array_equal(score[whole].view(np.uint32), _step_sums(logp, lens)[whole].view(np.uint32)), label
        # ... so a row whose tokens are reproduced bit for bit has its score reproduced bit for bit
        both = whole & same_tok
        assert np.array_equal(got_sc[both].view(np.uint32), score[both].view(np.uint32)), label


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd"])
def test_scores_of_sampled_captions_are_their_log_probs(golden_dir, name):
    """The logits of a step are the same bits in both drivers (the same decoder step on the same tokens); the two kernels reduce
    them differently (the sampler: row maximum first, then the sum; this kernel: one online pass), so the log-probs need not be
    bit-equal, and are not (the run prints how many tokens and rows are).  What holds and is asserted beyond the contract's 1e-4:
    each kernel is held to 1e-6 + two fp32 ulps of the value against float64 on the same logits, so the tokens agree within twice
    that; and both keep score_out as the fp32 sum of their own log-probs in step order, so each score is that sum bit for bit and
    a row whose tokens are reproduced bit for bit has its score reproduced bit for bit."""
    from simpleimagecaptionzoo_amd.scoring import score_captions
    _, h, _, feats = tbo._setup(golden_dir, name, "track")
    for n, seed in ((1, 3), (3, 4)):
        ids, logp, score = h.sample_decode(feats, n, 20, 0.9, 20, 0.95, rng=seed)
        _sampled_agree(lambda x: score_captions(h, feats, x, n), ids, logp, score, "%s n=%d" % (name, n), single=True)
    h.close()


@pytest.mark.parametrize("case", ["butd2", "mixed3"])
def test_ensemble_scores_of_sampled_captions_are_their_log_probs(golden_dir, case):
    from simpleimagecaptionzoo_amd.scoring import score_captions
    ens, dev, _, _ = tges._build(golden_dir, case, end_boost=4.0)
    for n, seed in ((1, 3), (3, 4)):
        ids, logp, score = [x.clone() for x in ens.sample_decode(dev, n, 20, 0.9, 20, 0.95, rng=seed)]
        _sampled_agree(lambda x: score_captions(ens, dev, x, n), ids, logp, score, "%s n=%d" % (case, n))


def _handle_or_ensemble(golden_dir, which, regime="track", end_boost=4.0):
    """a golden's handle, or the ensemble of a case of tests/_ens_sampling_cases.py (regime "track": its first member's <end> bias
    raised, so that it ends captions) -> (handle, its features)"""
    if which in ec.CASES:
        return tges._build(golden_dir, which, end_boost=end_boost if regime == "track" else 0.0)[:2]
    _, h, _, feats = tbo._setup(golden_dir, which, regime)
    return h, feats


@pytest.mark.parametrize("which", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd", "butd2", "mixed3"])
def test_scores_of_beam_hypotheses_are_the_beam_scores(golden_dir, which):
    """three decoders, a two-member and a three-member (BUTD + AoA + NIC) ensemble: the n-best hypotheses of beam_search_opts,
    scored five per image, give the reported scores back within 1e-4 per token.  A beam may pick <pad> (0) inside a hypothesis (the
    AoA golden does); ids cannot carry such a caption, which ends at its first 0: the hypotheses without one (most) are compared."""
    from simpleimagecaptionzoo_amd.scoring import ids_from_beam, score_captions
    h, feats = _handle_or_ensemble(golden_dir, which, end_boost=6.0)
    n_img = ec.N_IMG
    k, kinds = 5, set()
    for steps in (20, 12, 6):                     # 6 steps: beams still live at the step limit
        seqs, lens, scores = h.beam_search_opts(feats, k, steps, n_best=k, length_penalty="wu_0.9", block_ngram=3)
        ids = ids_from_beam(seqs, lens)
        assert ids.shape == (n_img * k, steps)
        logp, score = score_captions(h, feats, ids, k)
        tokens = sco.lengths(ids)
        whole = tokens == lens.cpu().numpy().reshape(-1) - 1
        inside = np.arange(steps)[None, :] < lens.cpu().numpy().reshape(-1, 1) - 1
        assert np.array_equal(whole, ~((ids == 0) & inside).any(1))       # short of the beam's length only by a <pad> inside it
        assert whole.sum() * 2 > len(whole), (which, steps, int(whole.sum()))
        err = np.abs(score.cpu().numpy() - scores.cpu().numpy().reshape(-1))[whole]
        print("%s beam %d steps: max score err %.3g over up to %d tokens, %d of %d hypotheses" % (
            which, steps, err.max(), tokens.max(), whole.sum(), len(whole)))
        assert (err <= 1e-4 * np.maximum(tokens[whole], 1)).all(), (which, steps, err.max())
        kinds |= {bool(ids[r, tokens[r] - 1] == 2) for r in np.nonzero(whole)[0]}
    assert kinds == {True, False}                 # finished and live-at-the-limit hypotheses both checked


def test_butd_agrees_with_xe_forward(golden_dir):
    """the parent's only route: xe_forward(train=False, want_logits=True) + float64 log_softmax, which wants the rows sorted by
    length and one image's features per row; the new entry takes the same captions unsorted, three per image"""
    from simpleimagecaptionzoo_amd.scoring import score_captions
    _, h, _, feats = tbo._setup(golden_dir, "butd_dec_tiny", "nat")
    n = 3
    rs = np.random.RandomState(9)
    lens = [3, 8, 1, 5, 2, 7, 4, 6, 8]             # unsorted, every caption scored in full
    ids = np.zeros((9, T), np.int64)
    for r, l in enumerate(lens):
        ids[r, :l] = rs.randint(3, h.V, size=l)
        if l < T or r == 1:
            ids[r, l - 1] = 2
    logp = score_captions(h, feats, ids, n)[0].cpu().numpy()
    assert sco.lengths(ids).tolist() == lens
    order = sorted(range(9), key=lambda r: -lens[r])
    caps = torch.ones(9, T + 1, dtype=torch.int64)
    caps[:, 1:] = torch.tensor(ids[order])
    steps = [lens[r] for r in order]
    f = feats.repeat_interleave(n, 0)[order].contiguous()
    logits = h.xe_forward(f, caps.cuda(), steps, None, train=False, want_logits=True)
    lsm = torch.log_softmax(logits.double().cpu(), 1).numpy()
    worst = 0.0
    for row, (b, t) in enumerate(ob.packed_order(steps)):
        worst = max(worst, abs(lsm[row, int(caps[b, t + 1])] - float(logp[order[b], t])))
    print("xe_forward route: max err %.3g over %d tokens" % (worst, sum(lens)))
    assert worst <= 1e-4
    h.close()


@pytest.mark.parametrize("which", ["butd_dec_odd", "aoa_tiny", "nic_dec_tiny", "butd2", "aoa2", "mixed3"])
def test_n_captions_equal_repeated_features(golden_dir, which):
    """bit for bit at the shapes at which tests/test_gpu_sampling.py and tests/test_gpu_ensemble_sampling.py hold the same identity
    for sample_decode: 3 images x 3 rows, three decoders and two- and three-member ensembles (the ensemble driver's prologue
    expansion through img_of_row); at these widths the per-image work computes a row independently of the row count"""
    from simpleimagecaptionzoo_amd.scoring import score_captions
    h, feats = _handle_or_ensemble(golden_dir, which)
    rep = lambda f: f.repeat_interleave(3, 0).contiguous()
    for seed in (31, 32):
        ids = _captions(ec.N_IMG * 3, h.V, seed)
        a = [x.clone() for x in score_captions(h, feats, ids, 3)]
        b = score_captions(h, [rep(f) for f in feats] if isinstance(feats, list) else rep(feats), ids, 1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (which, seed)
        assert (a[0] != 0).any()


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd"])
@pytest.mark.parametrize("copies", [1, 2, 3])
def test_ensemble_of_copies_equals_the_member(golden_dir, name, copies):
    """a one-member ensemble equals its member, identical copies under any weights equal the single model: within the kernel
    tolerance (the ensemble instance goes through log w_m and one more log / exp)"""
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    from simpleimagecaptionzoo_amd.scoring import score_captions
    _, h, _, feats = ec.device_member(golden_dir, name)
    others = [ec.device_member(golden_dir, name)[1] for _ in range(copies - 1)]
    ens = EnsembleHandle([h] + others, [0.2, 1.5, 0.7][:copies])
    for n in (1, 3):
        ids = _captions(feats.shape[0] * n, h.V, 70 + n)
        want = score_captions(h, feats, ids, n)[0].cpu().numpy()
        got = score_captions(ens, [feats] * copies, ids, n)[0].cpu().numpy()
        err = (np.abs(got - want) - np.abs(want) * 2.0 ** -22).max()
        print("%s x%d n=%d: max err above two ulps %.3g" % (name, copies, n, err))
        assert err <= 1e-6 and ((want == 0) == (got == 0)).all()


@pytest.mark.parametrize("which", ["butd_dec_odd", "aoa_tiny", "nic_dec_odd", "butd2", "mixed3"])
def test_two_runs_are_bit_equal(golden_dir, which):
    from simpleimagecaptionzoo_amd.scoring import score_captions
    h, feats = _handle_or_ensemble(golden_dir, which, "nat")
    ids = _captions(9, h.V, 81)
    a = [x.clone() for x in score_captions(h, feats, ids, 3)]
    other = score_captions(h, feats, _captions(9, h.V, 82), 3)        # another call in between
    b = score_captions(h, feats, ids, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], other[0])


# ---- full width -----------------------------------------------------------------------------------------------------------------
def test_fullwidth_butd_16_images_2_captions():
    """the benchmark width: the resident / split-K predict route of the real step.  The ids are the device's own sample_decode's,
    whose log-probs are reproduced; no CPU oracle at this width"""
    from _fullwidth import A, D, E, H, R, V, _full_params
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.scoring import score_captions
    n_img, n = 16, 2
    h = ButdHandle(R, D, H, E, A, V, n_img * n, 20)
    h.bind(_full_params(seed=78))
    g = torch.Generator(device="cpu")
    g.manual_seed(1007)
    feats = torch.relu(torch.randn(n_img, R, D, generator=g)).cuda()
    ids, logp, score = h.sample_decode(feats, n, T, 0.8, 50, 0.9, rng=77)
    _sampled_agree(lambda x: score_captions(h, feats, x, n), ids, logp, score, "full width", single=True)
    h.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _raw(fn, handle, feats, n_img, n, max_len, ids, outs):
    """the C entry itself, past the Python checks -> (status, message)"""
    from simpleimagecaptionzoo_amd._lib import lib, stream_ptr
    st = fn(handle, feats, n_img, n, max_len, C.c_void_p(ids.data_ptr()), C.c_void_p(outs[0].data_ptr()), C.c_void_p(outs[1].data_ptr()),
            stream_ptr())
    return st, lib().icz_last_error()


def test_refusals_queue_nothing(golden_dir):
    from simpleimagecaptionzoo_amd._lib import IczError, lib
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    from simpleimagecaptionzoo_amd.scoring import score_captions
    _, h, _, feats = tbo._setup(golden_dir, "butd_dec_tiny", "nat", max_rows=8)
    _, raw, _, _ = tbo._setup(golden_dir, "butd_dec_tiny", "nat", max_rows=8, bind=False)      # never bound: not refreshed
    _, nic, _, fn = ec.device_member(golden_dir, "nic_dec_tiny", max_rows=8)
    ens, ens_raw = EnsembleHandle([h, nic]), EnsembleHandle([h, raw])
    good = _captions(6, h.V, 91)
    before = [x.clone() for x in score_captions(h, feats, good, 2)]
    before_ens = [x.clone() for x in score_captions(ens, [feats, fn], good, 2)]
    ids9 = torch.tensor(_captions(9, h.V, 92)).cuda()
    outs = [torch.full((16, T), -7.0, device="cuda"), torch.full((16,), -7.0, device="cuda")]
    arr = (C.c_void_p * 2)(feats.data_ptr(), fn.data_ptr())
    arr_raw = (C.c_void_p * 2)(feats.data_ptr(), feats.data_ptr())
    gc.collect()                                  # what earlier tests left behind goes now, not inside the window below
    torch.cuda.synchronize()
    mem0, bufs0 = torch.cuda.memory_allocated(), dict(h._bufs)
    L = lib()
    for who, hd, f in ((h, h, feats), (ens, ens, [feats, fn])):
        for n in (0, 9):
            with pytest.raises(ValueError, match="captions per image"):
                score_captions(hd, f, good, n)
        with pytest.raises(ValueError, match="row capacity 8"):
            score_captions(hd, f, ids9, 3)                                        # 3 images x 3 captions > 8 rows
        for bad in (h.V, -1):
            ids = good.copy()
            ids[4, 2] = bad
            with pytest.raises(ValueError, match="outside the vocabulary"):
                score_captions(hd, f, ids, 2)
        with pytest.raises(ValueError, match="ids hold 6 rows"):
            score_captions(hd, f, good, 1)
    with pytest.raises(IczError, match="refresh"):
        score_captions(raw, feats, good, 2)
    with pytest.raises(IczError, match="not refreshed"):
        score_captions(ens_raw, [feats, feats], good, 2)
    for fnc, hd, f in ((L.icz_butd_score_captions, h._h, C.c_void_p(feats.data_ptr())), (L.icz_ensemble_score_captions, ens._h, arr)):
        for n in (0, 9):
            st, msg = _raw(fnc, hd, f, 1, n, T, ids9, outs)
            assert st == -1 and b"captions per image outside 1..8" in msg, msg
        st, msg = _raw(fnc, hd, f, 3, 3, T, ids9, outs)
        assert st == -1 and b"3 images x 3 captions exceed row capacity 8" in msg, msg
        st, msg = _raw(fnc, hd, f, 3, 2, 257, ids9, outs)
        assert st == -1 and b"max_len=257 outside 1..256" in msg, msg
    st, msg = _raw(L.icz_butd_score_captions, raw._h, C.c_void_p(feats.data_ptr()), 3, 2, T, ids9, outs)
    assert st == -1 and b"refresh_weights" in msg, msg
    st, msg = _raw(L.icz_ensemble_score_captions, ens_raw._h, arr_raw, 3, 2, T, ids9, outs)
    assert st == -1 and b"not refreshed" in msg, msg
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem0 and h._bufs == bufs0
    assert (outs[0] == -7.0).all() and (outs[1] == -7.0).all()                    # a refused call wrote nothing
    # the C level never reads out of range: an id outside [0, V) ends the row as a 0 does
    ids = good.copy()
    ids[4, 2], ids[1, 0] = h.V + 5, -3
    as_zero = good.copy()
    as_zero[4, 2], as_zero[1, 0] = 0, 0
    dev, lp, sc = torch.tensor(ids).cuda(), torch.zeros(6, T, device="cuda"), torch.zeros(6, device="cuda")
    st, msg = _raw(L.icz_butd_score_captions, h._h, C.c_void_p(feats.data_ptr()), 3, 2, T, dev, [lp, sc])
    assert st == 0, msg
    want = score_captions(h, feats, as_zero, 2)
    assert torch.equal(lp, want[0]) and torch.equal(sc, want[1])
    # the handles' buffers are as they were: the same calls give the same bits
    after, after_ens = score_captions(h, feats, good, 2), score_captions(ens, [feats, fn], good, 2)
    assert all(torch.equal(x, y) for x, y in zip(before + before_ens, after + after_ens))


# ---- Engine ---------------------------------------------------------------------------------------------------------------------
def _stub_env():
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    import test_gpu_caption_sets as tcs
    return types.SimpleNamespace(vocab=synthetic_vocab(tcs.V), tables={"big": {"dfd": None}})


def _golden_engine(golden_dir, model):
    import test_gpu_caption_sets as tcs
    env = _stub_env()
    return tcs._butd_engine(env) if model == "butd" else tcs._golden_engine(env, golden_dir, model)


def _host_pick(scored, n, kind, alpha):
    out = []
    for i in range(0, len(scored), n):
        ranks = []
        for e in scored[i:i + n]:
            t = e["tokens"]
            ranks.append(e["logprob"] / (t ** alpha if kind == "avg" else ((5 + t) / 6.0) ** alpha if kind == "wu" else 1.0))
        j = int(np.argmax(ranks))                             # the first of equals
        e = scored[i + j]
        out.append({"image_id": e["image_id"], "caption": e["caption"], "logprob": e["logprob"], "rank_score": float(ranks[j])})
    return out


@pytest.mark.parametrize("model", ["butd", "aoa", "nic"])
def test_engine_score_and_rescore(golden_dir, model):
    """score_captions_json on the output of sample_captions_json_generation.  Every caption is compared token by token on the words it
    shares with the sampled row (a drawn <pad> or <sta> leaves the caption's words).  Where the words are the whole sampled row: if
    the sampler drew <end>, "logprob" is the entry's "score"; if it ran to its 20 steps without one, the caption's appended <end> is
    one token more than was sampled, and "logprob" without that last token is the entry's "score".  Most captions must be such whole
    rows: the engine's <pad> and <sta> biases are lowered, as a trained model's are, so that the sampler does not draw them (the
    AoA golden as it is prefers them)."""
    from simpleimagecaptionzoo_amd.scoring import encode_captions
    eng, loader, vocab, _, B = _golden_engine(golden_dir, model)
    K, opts, seed = 5, (0.9, 20, 0.95), 4
    with torch.no_grad():
        eng.model.decoder.predict.bias[:2] -= 30.0
    entries = eng.sample_captions_json_generation(loader, K, *opts, seed=seed, tqdm_visible=False)
    scored = eng.score_captions_json(loader, entries, K, tqdm_visible=False)
    assert len(scored) == B * K and scored == eng.score_captions_json(loader, entries, K, tqdm_visible=False)
    same = 0
    at = 0
    for bi, (bids, _, bsupp) in enumerate(loader):
        with torch.cuda.stream(eng.stream):
            feats = eng._features(eng.modify_visual_inputs(None, bsupp))
            tok, lp, _ = eng._hot_handle().sample_decode(feats, K, 20, *opts, rng=(seed << 20) + bi)
        eng.stream.synchronize()
        tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
        for r in range(tok.shape[0]):
            e, s = entries[at], scored[at]
            at += 1
            words = len(e["caption"].split())
            assert {k: s[k] for k in e} == e and s["tokens"] == words + 1 == len(s["logprobs"])
            # "logprob" is the fp32 sum in step order: one rounding of at most half an ulp of the largest partial sum per token
            total = float(np.sum(np.float32(s["logprobs"]), dtype=np.float64))
            assert abs(s["logprob"] - total) <= (words + 1) * 2.0 ** -24 * max(1.0, float(np.abs(s["logprobs"]).sum()))
            clean = words < 20 and sco.length(tok[r]) == words + 1 and tok[r, words] == 2 and not (tok[r, :words] == 1).any()
            stop = np.nonzero(tok[r] <= 2)[0]                 # the first <pad>, <sta> or <end> of the sampled row
            shared = min(words, int(stop[0]) if len(stop) else 20)
            assert encode_captions([e["caption"]], vocab)[0, :shared].tolist() == tok[r, :shared].tolist()
            np.testing.assert_allclose(s["logprobs"][:shared], lp[r, :shared], atol=1e-4, rtol=0)
            if clean:
                same += 1
                assert abs(s["logprob"] - e["score"]) <= 1e-4, (model, at, s["logprob"], e["score"])
            elif words == 20 and shared == 20:
                same += 1
                assert abs(s["logprob"] - s["logprobs"][-1] - e["score"]) <= 1e-4, (model, at, s["logprob"], e["score"])
    print("engine %s: %d of %d captions are the whole sampled row" % (model, same, B * K))
    assert same * 2 > B * K                                   # most captions are compared in full
    for lp_arg, kind, alpha in ((None, None, 0.0), ("avg_1.0", "avg", 1.0), (("wu", 0.7), "wu", 0.7)):
        got = eng.rescore_captions_json(loader, entries, K, lp_arg, tqdm_visible=False)
        assert got == _host_pick(scored, K, kind, alpha), (model, lp_arg)
        assert [g["image_id"] for g in got] == [i for b in loader for i in b[0]]
    with pytest.raises(ValueError, match="the loader's image is"):
        eng.score_captions_json(loader, entries[K:2 * K] + entries[:K] + entries[2 * K:], K, tqdm_visible=False)
    with pytest.raises(ValueError, match="entries"):
        eng.score_captions_json(loader, entries[:-K], K, tqdm_visible=False)


def test_engine_reference_perplexity(golden_dir):
    """images with 2, 5 and 9 references: fewer than the batch's maximum are padded with empty captions, 9 are scored as 8 + 1"""
    from simpleimagecaptionzoo_amd.scoring import encode_captions, score_captions, scored_lengths
    eng, loader, vocab, _, B = _golden_engine(golden_dir, "butd")
    rs = np.random.RandomState(3)
    words = [vocab.ix2word[i] for i in range(4, len(vocab))]
    sent = lambda: " ".join(words[rs.randint(len(words))] for _ in range(rs.randint(1, 9)))
    gts = {i: [sent() for _ in range(c)] for i, c in zip(range(B), (2, 5, 9, 5))}
    gts[1][2] = "zebra " + gts[1][2]                          # an unknown word scores as <unk>
    scst = [(ids, None, gts, supp) for ids, _, supp in loader]
    got = eng.reference_perplexity(scst, tqdm_visible=False)
    total, tokens = 0.0, 0
    for ids, _, supp in loader:
        with torch.cuda.stream(eng.stream):
            feats = eng._features(eng.modify_visual_inputs(None, supp))
            for j, i in enumerate(ids):
                for ref in gts[i]:                            # one caption at a time, by hand
                    enc = encode_captions([ref], vocab)
                    lp = score_captions(eng._hot_handle(), feats[j:j + 1], enc, 1)[0].cpu().numpy().astype(np.float64)
                    total += lp[0, :scored_lengths(enc)[0]].sum()
                    tokens += int(scored_lengths(enc)[0])
    assert got["captions"] == 21 and got["tokens"] == tokens == sum(len(r.split()) + 1 for g in gts.values() for r in g)
    print("reference perplexity %.6f (by hand %.6f) over %d tokens" % (got["ppl"], np.exp(-total / tokens), tokens))
    assert abs(got["nll_per_token"] - (-total / tokens)) <= 1e-4 and abs(got["ppl"] - np.exp(-total / tokens)) <= 1e-4 * got["ppl"]


def test_engine_ensemble_functions(golden_dir):
    from simpleimagecaptionzoo_amd.engine import rescore_ensemble_captions_json, score_ensemble_captions_json
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    from simpleimagecaptionzoo_amd.scoring import encode_captions, score_captions, scored_lengths
    e1, g, _ = tge._perturbed_engine(golden_dir, 0)
    e2, _, _ = tge._perturbed_engine(golden_dir, 5)
    ids, supp = tge._batch(g)
    loader = [(ids[:3], None, supp[:3]), (ids[3:], None, supp[3:])]
    n, w = 3, [1.0, 2.0]
    entries = e1.sample_captions_json_generation(loader, n, 0.9, 20, 0.9, seed=5, tqdm_visible=False)
    got = score_ensemble_captions_json([e1, e2], loader, entries, n, tqdm_visible=False, weights=w)
    want, at = [], 0
    for bids, _, bsupp in loader:
        with torch.cuda.stream(e1.stream):
            feats = [e._features(e.modify_visual_inputs(None, bsupp)) for e in (e1, e2)]
            ens = EnsembleHandle([e1._hot_handle(), e2._hot_handle()], w)
            enc = encode_captions([e["caption"] for e in entries[at:at + len(bids) * n]], e1.caption_vocab)
            lp, sc = [x.cpu().numpy() for x in score_captions(ens, feats, enc, n)]
        for r, l in enumerate(scored_lengths(enc)):
            want.append(dict(entries[at + r], logprob=float(sc[r]), tokens=int(l), logprobs=[float(x) for x in lp[r, :l]]))
        at += len(bids) * n
    assert got == want
    for lp_arg, kind, alpha in ((None, None, 0.0), ("avg_0.5", "avg", 0.5)):
        assert rescore_ensemble_captions_json([e1, e2], loader, entries, n, lp_arg, tqdm_visible=False, weights=w) == _host_pick(got, n, kind, alpha)
    # one engine through the ensemble's kernel: the engine's own method within the kernel tolerance
    one = score_ensemble_captions_json([e1], loader, entries, n, tqdm_visible=False)
    own = e1.score_captions_json(loader, entries, n, tqdm_visible=False)
    for a, b in zip(one, own):
        assert a["tokens"] == b["tokens"]
        assert all(_kernel_err(x, y) <= 1e-6 for x, y in zip(a["logprobs"], b["logprobs"]))


def _butd_tiny_engine(golden_dir, max_batch):
    import test_gpu_engine as tgen
    from simpleimagecaptionzoo_amd.engine import BUTDDetection_Eng
    g, fx = tgen._load(golden_dir)
    _, vocab = tgen._engine(g, fx)
    B, R, D, H, E, A, V = [int(x) for x in g["dims"]]
    eng = BUTDDetection_Eng({"model_type": "BUTDDetection", "atten_dim": A, "embed_dim": E, "hidden_dim": H}, "SYN", vocab, data_dir="/tmp/",
                            use_bu="fixed", device="cuda:0", max_batch=max_batch)
    eng.model.load_state_dict({k[4:]: torch.tensor(v) for k, v in g.items() if k.startswith("sd0.")}, strict=True)
    return eng, g, vocab


def test_engine_scores_a_large_batch_in_chunks(golden_dir):
    """max_batch 1 gives the handle 5 rows: a batch of all golden images x 3 captions is scored one image at a time, and matches an
    engine of the same weights that holds the batch in one piece.  Observed on the MI355X: bit-equal (at this width every decoder
    GEMM computes a row independently of the row count); asserted so."""
    small, g, vocab = _butd_tiny_engine(golden_dir, 1)
    big, _, _ = _butd_tiny_engine(golden_dir, 32)
    ids, supp = tge._batch(g)
    assert len(ids) * 3 > small.model.max_rows == 5
    loader = [(ids, None, supp)]
    entries = big.sample_captions_json_generation(loader, 3, 0.9, 20, 0.9, seed=8, tqdm_visible=False)
    a = small.score_captions_json(loader, entries, 3, tqdm_visible=False)
    b = big.score_captions_json(loader, entries, 3, tqdm_visible=False)
    worst = max(abs(x - y) for p, q in zip(a, b) for x, y in zip(p["logprobs"], q["logprobs"]))
    print("chunked against whole: max difference %.3g, equal %s" % (worst, a == b))
    assert [p["tokens"] for p in a] == [q["tokens"] for q in b] and worst <= 1e-4
    assert a == b
    with pytest.raises(ValueError, match="6 captions per image exceed the handle's row capacity 5"):
        small.score_captions_json(loader, [dict(e) for e in entries for _ in range(2)], 6, tqdm_visible=False)
