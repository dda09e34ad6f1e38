"""GPU tests of constrained beam search (include/icz.h: icz_beam_constraints -- captions that must contain given words) for the BUTD,
AoA and NIC decoders and their ensembles: with no constraint it is today's options search bit for bit, and with constraints the n-best
lists and states equal the host oracle of tests/_beam_constrained.py token for token on every (config, image) pair whose selections
the oracle keeps at least GAP_MIN apart (tests/test_cpu_beam_constrained.py holds their share above 90 %)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _beam_constrained as bc  # noqa: E402
from test_gpu_beam_opts import GOLDENS, LP, _setup, _teacher_forced_scores  # noqa: E402


def _search(h, feats, cons, beam, steps=50, n_best=None, lp=None, block=0):
    from simpleimagecaptionzoo_amd import constrained
    return constrained.beam_search(h, feats, cons, beam, steps, beam if n_best is None else n_best, lp, block)


def _lists(seqs, lens, scores, sat):
    seqs, lens, scores, sat = seqs.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy(), sat.cpu().numpy()
    return [[(seqs[i, j, :lens[i, j]].astype(int).tolist(), float(scores[i, j]), int(sat[i, j])) for j in range(lens.shape[1])]
            for i in range(lens.shape[0])]


_worst = {}              # test -> largest score error seen (printed, so that a run's log shows how far inside the tolerance it was)


def _check(got, want, what):
    """got: the device's n_best list of one image; want: the oracle's full ranked list.  Scores within 1e-4, the project's beam-score
    tolerance."""
    want = want[:len(got)]
    got = [g for g in got if g[0]]                       # ranks past the image's hypotheses have length 0
    assert [g[0] for g in got] == [w.tokens for w in want], what
    assert [g[2] for g in got] == [w.state for w in want], what
    for g, w in zip(got, want):
        err = abs(g[1] - w.score)
        _worst[what[0]] = max(_worst.get(what[0], 0.0), err)
        assert err <= 1e-4, (what, g, w, err)


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("regime", ["nat", "track"])
def test_no_constraints_is_beam_search_opts_bit_for_bit(golden_dir, name, regime):
    _, h, _, feats = _setup(golden_dir, name, regime)
    n = feats.shape[0]
    for k in (1, 3, 5):
        for block, lp in ((0, None), (3, None), (0, ("wu", 0.9)), (3, ("avg", 0.7))):
            for n_best in sorted({1, k}):
                want = h.beam_search_opts(feats, k, 50, n_best, lp, block)
                for cons in ([[] for _ in range(n)], np.full((n, 2, 3), -1, dtype=np.int32)):      # C = 0; every slot empty
                    got = _search(h, feats, cons, k, 50, n_best, lp, block)
                    assert all(torch.equal(a, b) for a, b in zip(got[:3], want)), (name, regime, k, block, lp, n_best)
                    assert got[3].shape == (n, n_best) and not got[3].any()


_COMPARED = {}           # (golden, regime) -> (pairs whose device lists were compared with the oracle's, pairs in all)


def _compare_golden(golden_dir, name, regime):
    """every (config, image) pair of one golden whose oracle selections stay GAP_MIN apart, device against oracle; once per process"""
    if (name, regime) not in _COMPARED:
        _, h, _, feats = _setup(golden_dir, name, regime, max_rows=96)
        n = feats.shape[0]
        compared = total = 0
        for cfg in bc.configs():
            beam, si, block, lp = cfg
            got = _lists(*_search(h, feats, bc.batch_constraints(si, n), beam, 50, beam, lp, block))
            for i in range(n):
                want, gap = bc.oracle_pair(golden_dir, name, regime, cfg, i)
                total += 1
                if gap < bc.GAP_MIN:
                    continue
                assert len(got[i]) == beam
                _check(got[i], want, (name, regime, cfg, i))
                compared += 1
        print("compared %d of %d pairs, largest score error %.3g" % (compared, total, _worst.get(name, 0.0)))
        _COMPARED[(name, regime)] = (compared, total)
    return _COMPARED[(name, regime)]


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("regime", ["nat", "track"])
def test_nbest_token_exact_against_the_oracle(golden_dir, name, regime):
    compared, total = _compare_golden(golden_dir, name, regime)
    assert total == 72 and compared > 0              # 24 configs x 3 images


def test_at_least_90_percent_of_the_pairs_were_compared(golden_dir):
    """over the five goldens and both regimes the device lists of at least 90 % of the 720 (config, image) pairs were compared with the
    oracle's (a golden that test_nbest_token_exact_against_the_oracle has not run in this process is compared here)"""
    counts = [_compare_golden(golden_dir, name, regime) for name in GOLDENS for regime in ("nat", "track")]
    compared, total = sum(c for c, _ in counts), sum(t for _, t in counts)
    print("compared %d of %d pairs" % (compared, total))
    assert total == 720 and compared >= 0.9 * total


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd"])
def test_scores_are_model_log_probs(golden_dir, name):
    """every returned score is the model's log-probability of its tokens: scoring.score_captions and a teacher-forced forward pass"""
    from simpleimagecaptionzoo_amd import scoring
    model, h, _, feats = _setup(golden_dir, name, "track", max_rows=96)
    n = feats.shape[0]
    kinds = set()
    for steps in (50, 8):                    # 8 steps: beams still live at the step limit
        beam = 3
        got = _lists(*_search(h, feats, bc.batch_constraints(2, n), beam, steps, beam, "wu_0.9", 3))
        ids = torch.zeros(n * beam, steps, dtype=torch.int64)
        for i, img in enumerate(got):
            for j, (toks, _, _) in enumerate(img):
                ids[i * beam + j, :len(toks) - 1] = torch.tensor(toks[1:])
                kinds.add(toks[-1] == 2)
        _, score = scoring.score_captions(h, feats, ids.cuda(), beam)
        np.testing.assert_allclose([x[1] for img in got for x in img], score.cpu().numpy(), atol=1e-4, rtol=0)
        want = _teacher_forced_scores(model, golden_dir, name, "track", feats, [[(t, s) for t, s, _ in img] for img in got])
        for img, w in zip(got, want):
            for (toks, sc, _), ws in zip(img, w):
                assert abs(sc - ws) <= 1e-4, (toks, sc, ws)
    assert kinds == {True, False}


@pytest.mark.parametrize("name", GOLDENS)
def test_repeatable_and_batch_independent(golden_dir, name):
    """two runs are bit-equal, n images give what the images give one by one, and n_best = 1 is the head of the full list"""
    _, h, _, feats = _setup(golden_dir, name, "track", max_rows=96)
    n = feats.shape[0]
    for beam, si, block, lp in ((3, 2, 3, "wu_0.9"), (2, 3, 0, None), (4, 1, 0, None)):
        cons = bc.batch_constraints(si, n)
        a = _search(h, feats, cons, beam, 50, beam, lp, block)
        b = _search(h, feats, cons, beam, 50, beam, lp, block)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        # one image at a time, in a call of its own constraint count: the states the batch adds for its largest count stay empty
        for i in range(n):
            one = _search(h, feats[i:i + 1].contiguous(), [cons[i]], beam, 50, beam, lp, block)
            assert all(torch.equal(a[j][i:i + 1], one[j]) for j in (0, 1, 3)), (name, beam, si, i)
            # the decoder's GEMMs may split differently at another row count: the project's beam-score tolerance
            np.testing.assert_allclose(one[2].cpu().numpy(), a[2][i:i + 1].cpu().numpy(), atol=1e-4, rtol=0)
        head = _search(h, feats, cons, beam, 50, 1, lp, block)
        assert all(torch.equal(x[:, :1], y) for x, y in zip(a, head))


def test_aoa_per_image_region_counts(golden_dir):
    """a batch padded to its largest region count with per-image counts searches each image as the oracle does on its unpadded
    features: tokens and states exactly, scores within 1e-4.  It runs bc.AOA_ADAPTIVE_STEPS steps, not 50: on this golden the fp32
    recurrence drifts along the longest hypotheses, so that the fp32 oracle's own 50-step score is 1.5e-4 off its float64 value
    (tests/_beam_constrained.py: AOA_ADAPTIVE_STEPS).  tests/test_cpu_beam_constrained.py holds the oracle's own error below 2e-5 for
    every hypothesis compared here."""
    from test_gpu_aoa_adaptive import batch_of, make
    g, sd = bc.aoa_adaptive_case(golden_dir)[:2]
    h = make(g, sd, max_rows=96)
    compared = total = 0
    for cfg in bc.AOA_ADAPTIVE_CONFIGS:
        beam, si, block, lp = cfg
        got = _lists(*_search(h, batch_of(g, slice(0, 3)), bc.batch_constraints(si, 3), beam, bc.AOA_ADAPTIVE_STEPS, beam, lp, block))
        for i in range(3):
            want, gap = bc.aoa_adaptive_pair(golden_dir, cfg, i)
            total += 1
            if gap >= bc.GAP_MIN:
                compared += 1
                _check(got[i], want, ("aoa_adaptive", cfg, i))
    print("compared %d of %d pairs, largest score error %.3g" % (compared, total, _worst.get("aoa_adaptive", 0.0)))
    assert compared >= 0.9 * total


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_tiny"])
def test_unrefreshed_handle_is_refused(golden_dir, name):
    from simpleimagecaptionzoo_amd._lib import IczError
    model, h, p, feats = _setup(golden_dir, name, bind=False, max_rows=72)
    with pytest.raises(IczError, match="icz_%s_refresh_weights" % model):
        _search(h, feats, bc.batch_constraints(2, feats.shape[0]), 3)
    with pytest.raises(ValueError, match="row capacity"):
        _search(h, feats, bc.batch_constraints(3, feats.shape[0]), 4)          # 3 images x 32 rows > 72
    h.bind({k: v.cuda() for k, v in p.items()})
    got = _search(h, feats, bc.batch_constraints(2, feats.shape[0]), 3)
    _, ref, _, _ = _setup(golden_dir, name, max_rows=72)
    want = _search(ref, feats, bc.batch_constraints(2, feats.shape[0]), 3)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and (got[1] > 1).all()


# ---- ensembles ---------------------------------------------------------------------------------------------------------------------
ENSEMBLE_CONFIGS = ((3, 2, 0, None), (2, 3, 3, ("wu", 0.9)), (4, 0, 0, None), (3, 1, 3, ("wu", 0.9)))


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd"])
def test_one_member_equals_the_member_bit_for_bit(golden_dir, name):
    """an ensemble of one member runs the member's own search (its weight normalises to 1): every output of every config and image is
    the member's, bit for bit, with nothing left out"""
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    from test_gpu_ensemble import _member
    _, h, _, feats = _member(golden_dir, name, max_rows=96)
    one = EnsembleHandle([h], weights=[0.7])
    n = feats.shape[0]
    for beam, si, block, lp in ENSEMBLE_CONFIGS:
        cons = bc.batch_constraints(si, n)
        for n_best in sorted({1, beam}):
            want = _search(h, feats, cons, beam, 50, n_best, lp, block)
            got = _search(one, [feats], cons, beam, 50, n_best, lp, block)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (name, beam, si, block, lp, n_best)
            assert (want[3] > 0).any()
    none = _search(one, [feats], [[] for _ in range(n)], 3, 50, 3, ("wu", 0.9), 3)
    assert all(torch.equal(a, b) for a, b in zip(none[:3], h.beam_search_opts(feats, 3, 50, 3, ("wu", 0.9), 3))) and not none[3].any()


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_tiny"])
def test_identical_copies_equal_the_single_model(golden_dir, name):
    """two copies at weights 0.5 / 0.5 go through the combine kernel: every config and image gives the single model's tokens and
    states (no pair is left out), scores within the beam-score tolerance, and two runs of the ensemble are bit-equal"""
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    from test_gpu_ensemble import _member
    _, h, _, feats = _member(golden_dir, name, max_rows=96)
    _, h2, _, _ = _member(golden_dir, name, max_rows=96)
    two = EnsembleHandle([h, h2], weights=[0.5, 0.5])
    n = feats.shape[0]
    for beam, si, block, lp in ENSEMBLE_CONFIGS:
        cons = bc.batch_constraints(si, n)
        w = _lists(*_search(h, feats, cons, beam, 50, beam, lp, block))
        e = _search(two, [feats, feats], cons, beam, 50, beam, lp, block)
        assert all(torch.equal(a, b) for a, b in zip(e, _search(two, [feats, feats], cons, beam, 50, beam, lp, block)))
        e = _lists(*e)
        for i in range(n):
            assert [x[0] for x in e[i]] == [x[0] for x in w[i]] and [x[2] for x in e[i]] == [x[2] for x in w[i]], (name, beam, si, i)
            np.testing.assert_allclose([x[1] for x in e[i]], [x[1] for x in w[i]], atol=1e-4, rtol=0)


def test_mixed_ensemble_against_the_oracle(golden_dir):
    """BUTD + AoA + NIC (V = 53) against the oracle over the combined step (float64 log of the weighted mean).  Of the 12 (config,
    image) pairs the oracle keeps 10 at least GAP_MIN apart (measured; every run prints the count); at least 9 must be compared."""
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    from test_gpu_ensemble import _ens_closure, _member
    weights = [1.0, 2.0, 1.5]
    members = [_member(golden_dir, nm, seed, max_rows=96) for nm, seed in (("butd_dec_tiny", 0), ("aoa_tiny", 4), ("nic_dec_tiny", 0))]
    n = members[0][3].shape[0]
    ens = EnsembleHandle([m[1] for m in members], weights)
    compared = total = 0
    for beam, si, block, lp in ENSEMBLE_CONFIGS:
        cons = bc.batch_constraints(si, n)
        C = max(len(c) for c in cons)
        got = _lists(*_search(ens, [m[3] for m in members], cons, beam, 50, beam, lp, block))
        for i in range(n):
            parts = [(model, f[i:i + 1].cpu(), p) for model, _, p, f in members]
            gaps = []
            with torch.no_grad():
                step, state, V = _ens_closure(parts, weights, 1)
                want = bc.constrained_nbest(step, state, beam, C, cons[i], V, 50, block, *LP[lp], gaps=gaps)
            total += 1
            if min(gaps) < bc.GAP_MIN:
                continue
            compared += 1
            _check(got[i], want, ("mixed", beam, si, block, lp, i))
    print("compared %d of %d pairs, largest score error %.3g" % (compared, total, _worst.get("mixed", 0.0)))
    assert compared >= 0.75 * total


def test_fullwidth_butd_16_images_two_constraints():
    """16 images, beam 3, two constraints at the benchmark width (sharpened weights, tests/_fullwidth.py), against the oracle on three"""
    from _fullwidth import A, D, E, H, R, V, _cpu, _full_params
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    params = _full_params(seed=78)
    n_img, beam, steps = 16, 3, 20
    h = ButdHandle(R, D, H, E, A, V, n_img * 4 * beam, 20)
    h.bind(params)
    torch.manual_seed(6)
    feats = torch.relu(torch.randn(n_img, R, D, device="cuda"))
    cons = [[[5 + 7 * i, 900 + i], [4000 + 11 * i]] if i % 4 else [[5 + 7 * i]] for i in range(n_img)]
    got = _lists(*_search(h, feats, cons, beam, steps, beam))
    p = _cpu(params)
    for i in (1, 8, 15):
        gaps = []
        want = bc.nbest("butd", feats[i:i + 1].cpu(), p, beam, 2, cons[i], steps, gaps=gaps)
        assert min(gaps) >= bc.GAP_MIN, (i, min(gaps))          # sharpened weights: no near-ties (as the existing full-width beam tests)
        _check(got[i], want, ("fullwidth", i))
    print("largest score error %.3g" % _worst.get("fullwidth", 0.0))
    h.close()


# ---- Engine ------------------------------------------------------------------------------------------------------------------------
def _engine(golden_dir):
    import json
    from simpleimagecaptionzoo_amd.engine import BUTDDetection_Eng
    from simpleimagecaptionzoo_amd.vocab import Caption_Vocabulary
    from synth import feats_from_seed
    g = dict(np.load(os.path.join(golden_dir, "butd_engine_tiny.npz")))
    fx = json.load(open(os.path.join(golden_dir, "butd_engine_tiny.json")))
    B, R, D, H, E, A, V = [int(x) for x in g["dims"]]
    vocab = Caption_Vocabulary()
    for w in fx["vocab"]:
        vocab.add_word(w)
    df = {"document_frequency": {tuple(k): v for k, v in fx["df"]["document_frequency"]}, "ref_len": fx["df"]["ref_len"]}
    eng = BUTDDetection_Eng({"model_type": "BUTDDetection", "atten_dim": A, "embed_dim": E, "hidden_dim": H},
                            "SYN", vocab, data_dir="/tmp/", use_bu="fixed", device="cuda:0", cider_df=df, max_batch=16)
    eng.model.load_state_dict({k[4:]: torch.tensor(v) for k, v in g.items() if k.startswith("sd0.")}, strict=True)
    feats = feats_from_seed(int(g["eval_feats_seed"]), B, R, D)
    ids = tuple(int(i) for i in g["eval_img_ids"])
    supp = tuple({"bu_feat": feats[i], "bu_bbox": np.zeros((R, 4), np.float32)} for i in range(B))
    return eng, vocab, ids, supp, fx


def test_engine_constrained_json(golden_dir):
    from simpleimagecaptionzoo_amd import constrained as cst
    from simpleimagecaptionzoo_amd import engine as engine_mod
    eng, vocab, ids, supp, fx = _engine(golden_dir)
    B = len(ids)
    assert B >= 4
    loader = [(ids[:3], None, supp[:3]), (ids[3:], None, supp[3:])]
    # image 0: two constraints; 1: alternatives, one of them unknown; 2: an unknown constraint beside a known one; 3: absent
    given = {ids[0]: ["w5", ["w7", "w9"]], ids[1]: [["w3", "zebra"]], ids[2]: ["zebra", "w11"]}
    res = eng.constrained_captions_json_generation(loader, given, 3, False)
    assert [r["image_id"] for r in res] == list(ids)
    # the entries built by hand, one image at a time through the captioner
    for i, r in enumerate(res):
        cons = [[c] if isinstance(c, str) else list(c) for c in given.get(ids[i], [])]
        enc, dropped = cst.encode_constraints([cons], vocab)
        hyp = cst.captioner_beam_search(eng.model, eng.modify_visual_inputs(None, supp[i:i + 1]), enc, 3)[0][0]
        words = [vocab.ix2word[int(t)] for t in hyp[0][0].tolist()]
        words = words[1:words.index("<end>")] if "<end>" in words else words[1:]
        assert r["caption"] == " ".join(words), (i, r)
        lost = {q for _, q, _ in dropped}
        bits = iter(cst.satisfied_flags(hyp[2], len(enc[0])))
        assert r["satisfied"] == [False if q in lost else next(bits) for q in range(len(cons))], (i, r)
        # "satisfied" agrees with the words of the caption
        assert r["satisfied"] == [any(w in r["caption"].split() for w in alts) for alts in cons], (i, r)
    assert res[3]["satisfied"] == [] and res[2]["satisfied"][0] is False
    assert any(any(r["satisfied"]) for r in res)
    # chunked equals whole: one image per call against the engine's own chunks (16 x 5 rows hold the 4 x 12 of the whole batch)
    one = engine_mod._constrained_captions_json_generation([eng], None, False, [(ids, None, supp)], given, 3, False, None, 0, max_chunk=1)
    whole = eng.constrained_captions_json_generation([(ids, None, supp)], given, 3, False)
    assert one == whole == res
    # no constraints: today's beam search
    plain = eng.constrained_captions_json_generation(loader, {}, 3, False)
    assert [{"image_id": r["image_id"], "caption": r["caption"]} for r in plain] == fx["eval_beam3_json"]
    assert all(r["satisfied"] == [] for r in plain)
    assert [{k: r[k] for k in ("image_id", "caption")} for r in plain] == eng.eval_captions_json_generation(loader, eval_beam_size=3, tqdm_visible=False)
    # the ensemble of the one engine: the same images, and flags that agree with its own captions
    ens = engine_mod.constrained_ensemble_captions_json_generation([eng], loader, given, 3, False)
    assert [r["image_id"] for r in ens] == list(ids)
    for i, r in enumerate(ens):
        cons = [[c] if isinstance(c, str) else list(c) for c in given.get(ids[i], [])]
        assert r["satisfied"] == [any(w in r["caption"].split() for w in alts) for alts in cons], (i, r)
    for bad in ([], {ids[0]: ["w5", "w6", "w7", "w8"]}, {ids[0]: [["w5", "w6", "w7", "w8", "w9"]]}):
        with pytest.raises(ValueError):
            eng.constrained_captions_json_generation(loader, bad, 3, False)
    with pytest.raises(ValueError):
        eng.constrained_captions_json_generation(loader, {ids[0]: ["w5", "w6", "w7"]}, 5, False)          # 2^3 x 5 rows
