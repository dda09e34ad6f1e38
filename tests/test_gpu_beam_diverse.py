"""GPU tests of diverse beam search (include/icz.h: icz_beam_diversity -- grouped beams with a diversity penalty) for the BUTD,
AoA and NIC decoders: one group is today's options search bit for bit, and the n-best lists equal the host oracle of
tests/_diverse_beam_oracle.py token for token."""
import collections
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _diverse_beam_oracle as dv  # noqa: E402
from synth import feats_from_seed  # noqa: E402
from test_gpu_beam_opts import GOLDENS, LP, _lists, _setup, _teacher_forced_scores  # noqa: E402

# (beam, groups, diversity).  0.7 times a count of 3, 5, 6 or 7 is inexact in fp32, so a key fused into one fma would differ from
# the spec's.  Every config keeps the oracle's selections at least 6e-5 apart on these goldens; small lambdas with many one-beam
# groups (e.g. (8, 8, 0.1)) let groups re-converge onto equal beams and leave ties within an ulp, which the device's and torch's
# log-softmax (different summation orders) may break differently.
CONFIGS = [(4, 2, 0.5), (6, 3, 1.0), (8, 4, 0.3), (6, 6, 2.0), (8, 4, 0.7), (6, 2, 0.7)]
VARIANTS = [(0, None), (3, ("wu", 0.9))]                                  # (block_ngram, length penalty)


def _entry(model, h, feats, k, steps, n_best=1, lp=None, block=0, groups=1, diversity=0.0):
    """icz_<model>_beam_search_diverse called directly (the handles route one group to icz_*_beam_search_opts)"""
    from simpleimagecaptionzoo_amd import beam as _beam
    from simpleimagecaptionzoo_amd._lib import BeamDiversity, lib
    feats = h._feats(feats)
    entry = getattr(lib(), "icz_%s_beam_search_diverse" % model)
    return _beam.search_diverse(entry, h._h, feats, k, steps, _beam.make_opts(n_best, lp, block), BeamDiversity(groups, diversity))


def _check_against_oracle(got, want, what):
    assert [w[0] for w in want] == [x[0] for x in got], what
    np.testing.assert_allclose([x[1] for x in got], [w[1] for w in want], atol=1e-4, rtol=0, err_msg=str(what))


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("regime", ["nat", "track"])
def test_one_group_is_beam_search_opts_bit_for_bit(golden_dir, name, regime):
    model, h, _, feats = _setup(golden_dir, name, regime)
    for k in (1, 3, 5):
        for block, lp in ((0, None), (3, None), (0, ("wu", 0.9)), (3, ("avg", 0.7))):
            for n_best in sorted({1, k}):
                want = h.beam_search_opts(feats, k, 50, n_best, lp, block)
                for lam in (0.0, 0.7):                   # one group: nothing precedes it, lambda has no effect
                    got = _entry(model, h, feats, k, 50, n_best, lp, block, 1, lam)
                    assert all(torch.equal(a, b) for a, b in zip(got, want)), (name, regime, k, block, lp, n_best, lam)
                assert all(torch.equal(a, b) for a, b in zip(h.beam_search_opts(feats, k, 50, n_best, lp, block, 1, 0.7), want))


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("regime", ["nat", "track"])
def test_nbest_token_exact_against_the_oracle(golden_dir, name, regime):
    model, h, p, feats = _setup(golden_dir, name, regime, max_rows=24)
    for B, G, lam in CONFIGS:
        for block, lp in VARIANTS:
            got = _lists(*h.beam_search_opts(feats, B, 50, n_best=B, length_penalty=lp, block_ngram=block, groups=G, diversity=lam))
            for i in range(feats.shape[0]):
                assert len(got[i]) == B
                want = dv.nbest(model, feats[i:i + 1].cpu(), p, B, G, lam, 50, block, *LP[lp])
                _check_against_oracle(got[i], want, (name, regime, B, G, lam, block, lp, i))


@pytest.mark.parametrize("name", GOLDENS)
def test_zero_diversity_repeats_the_group_search(golden_dir, name):
    """lambda = 0: G independent copies of the kg-beam search; every hypothesis of its n-best list appears G times in a row"""
    _, h, _, feats = _setup(golden_dir, name, "track", max_rows=24)
    for B, G in ((4, 2), (6, 3), (8, 4), (6, 2)):
        kg = B // G
        for block, lp in VARIANTS:
            got = _lists(*h.beam_search_opts(feats, B, 50, n_best=B, length_penalty=lp, block_ngram=block, groups=G, diversity=0.0))
            one = _lists(*h.beam_search_opts(feats, kg, 50, n_best=kg, length_penalty=lp, block_ngram=block))
            for i in range(feats.shape[0]):
                assert [x[0] for x in got[i]] == [x[0] for x in one[i] for _ in range(G)], (name, B, G, block, lp, i)
                np.testing.assert_allclose([x[1] for x in got[i]], [x[1] for x in one[i] for _ in range(G)], atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd"])
def test_scores_are_model_log_probs(golden_dir, name):
    """the penalty only steers the selection: every reported score is the teacher-forced log-probability of its tokens"""
    model, h, _, feats = _setup(golden_dir, name, "track", max_rows=24)
    kinds = set()
    for steps in (50, 8):                    # 8 steps: beams still live at the step limit
        got = _lists(*h.beam_search_opts(feats, 6, steps, n_best=6, length_penalty="wu_0.9", block_ngram=3, groups=3, diversity=1.0))
        want = _teacher_forced_scores(model, golden_dir, name, "track", feats, got)
        for img, w in zip(got, want):
            for (toks, sc), ws in zip(img, w):
                kinds.add(toks[-1] == 2)
                assert abs(sc - ws) <= 1e-4, (toks, sc, ws)
    assert kinds == {True, False}            # finished and live-at-the-limit hypotheses both checked


@pytest.mark.parametrize("name", GOLDENS)
def test_one_step_groups_pick_distinct_tokens(golden_dir, name):
    """max_steps = 1: with a penalty far above any log-prob gap the B one-token hypotheses are pairwise distinct; without a
    penalty every token the kg-beam search picks appears G times"""
    _, h, _, feats = _setup(golden_dir, name, "track", max_rows=24)
    for B, G in ((6, 3), (8, 4), (6, 6), (4, 2)):
        far = _lists(*h.beam_search_opts(feats, B, 1, n_best=B, groups=G, diversity=100.0))
        same = _lists(*h.beam_search_opts(feats, B, 1, n_best=B, groups=G, diversity=0.0))
        for img in far:
            toks = [tuple(t) for t, _ in img]
            assert len(toks) == B and all(len(t) == 2 for t in toks)
            assert len(set(toks)) == B, (name, B, G, toks)
        for img in same:
            counts = collections.Counter(tuple(t) for t, _ in img)
            assert len(img) == B and set(counts.values()) == {G}, (name, B, G, counts)


def test_aoa_per_image_region_counts(golden_dir):
    """a batch padded to its largest region count with per-image counts (icz_aoa_set_regions) searches each image as the oracle
    does on its unpadded features"""
    from test_gpu_aoa import regime_sd
    from test_gpu_aoa_adaptive import batch_of, counts_of, make, padded_feats
    g = dict(np.load(os.path.join(golden_dir, "aoa_adaptive.npz")))
    counts = counts_of(g)
    f = torch.from_numpy(padded_feats(g))
    for regime in ("nat", "track"):
        sd = regime_sd(g, regime)
        h = make(g, sd, max_rows=24)
        p = {k: torch.tensor(np.asarray(v), dtype=torch.float32) for k, v in sd.items()}
        for B, G, lam in ((6, 3, 1.0), (4, 2, 0.5), (8, 8, 0.7)):
            for block, lp in VARIANTS:
                got = _lists(*h.beam_search_opts(batch_of(g, slice(0, 3)), B, 50, n_best=B, length_penalty=lp, block_ngram=block,
                                                 groups=G, diversity=lam))
                for i in range(3):
                    want = dv.nbest("aoa", f[i:i + 1, :counts[i]], p, B, G, lam, 50, block, *LP[lp])
                    _check_against_oracle(got[i], want, (regime, B, G, lam, block, lp, i))


def test_fullwidth_butd_beam6_three_groups_128_images():
    """Beam 6 over 128 images at the benchmark width (sharpened weights, tests/_fullwidth.py): one group through the new entry is
    beam_search_opts bit for bit; with G = 3, lambda = 0.5 the lists of six images equal the oracle's."""
    from _fullwidth import A, D, E, H, R, V, _cpu, _full_params
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    params = _full_params(seed=78)
    n_img, k, steps = 128, 6, 20
    h = ButdHandle(R, D, H, E, A, V, n_img * k, 20)
    h.bind(params)
    torch.manual_seed(6)
    feats = torch.relu(torch.randn(n_img, R, D, device="cuda"))
    for n_best, lp, block in ((1, None, 0), (6, "wu_0.9", 3)):
        want = h.beam_search_opts(feats, k, steps, n_best, lp, block)
        got = _entry("butd", h, feats, k, steps, n_best, lp, block, 1, 0.0)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), (n_best, lp, block)
    got = _lists(*h.beam_search_opts(feats, k, steps, n_best=k, groups=3, diversity=0.5))
    p = _cpu(params)
    differ = []
    for i in (0, 25, 50, 77, 101, 127):
        want = dv.nbest("butd", feats[i:i + 1].cpu(), p, k, 3, 0.5, steps)
        if [w[0] for w in want] != [x[0] for x in got[i]]:
            differ.append((i, got[i], want))
        else:
            np.testing.assert_allclose([x[1] for x in got[i]], [w[1] for w in want], atol=1e-4, rtol=0)
    assert not differ, differ          # sharpened weights: no near-ties (as the existing full-width beam tests)
    h.close()


@pytest.mark.parametrize("model", ["butd", "aoa", "nic"])
def test_diverse_search_across_buffer_regrowth(golden_dir, model):
    """a handle whose beam buffers regrow (60 steps > the 51 columns they start with) gives the lists of fresh handles"""
    from test_gpu_beam_regrowth import _factory
    make, feats = _factory(model, golden_dir)
    h = make()
    for steps in (20, 60, 20):
        got = h.beam_search_opts(feats, 3, steps, n_best=3, groups=3, diversity=0.5)
        want = make().beam_search_opts(feats, 3, steps, n_best=3, groups=3, diversity=0.5)
        assert got[1].cpu().tolist() == want[1].cpu().tolist() == [[steps + 1] * 3] * feats.shape[0], steps
        assert torch.equal(got[0].cpu(), want[0].cpu()) and torch.equal(got[2].cpu(), want[2].cpu()), steps


def test_engine_eval_json_with_groups(golden_dir):
    from simpleimagecaptionzoo_amd.engine import BUTDDetection_Eng
    from simpleimagecaptionzoo_amd.vocab import Caption_Vocabulary
    g = dict(np.load(os.path.join(golden_dir, "butd_engine_tiny.npz")))
    fx = json.load(open(os.path.join(golden_dir, "butd_engine_tiny.json")))
    B, R, D, H, E, A, V = [int(x) for x in g["dims"]]
    vocab = Caption_Vocabulary()
    for w in fx["vocab"]:
        vocab.add_word(w)
    df = {"document_frequency": {tuple(k): v for k, v in fx["df"]["document_frequency"]}, "ref_len": fx["df"]["ref_len"]}
    eng = BUTDDetection_Eng({"model_type": "BUTDDetection", "atten_dim": A, "embed_dim": E, "hidden_dim": H},
                            "SYN", vocab, data_dir="/tmp/", use_bu="fixed", device="cuda:0", cider_df=df, max_batch=8)
    eng.model.load_state_dict({k[4:]: torch.tensor(v) for k, v in g.items() if k.startswith("sd0.")}, strict=True)
    feats = feats_from_seed(int(g["eval_feats_seed"]), B, R, D)
    ids = tuple(int(i) for i in g["eval_img_ids"])
    supp = tuple({"bu_feat": feats[i], "bu_bbox": np.zeros((R, 4), np.float32)} for i in range(B))
    loader = [(ids, None, supp)]
    assert eng.eval_captions_json_generation(loader, eval_beam_size=3, tqdm_visible=False) == fx["eval_beam3_json"]
    res = eng.eval_captions_json_generation(loader, eval_beam_size=3, tqdm_visible=False, beam_groups=3, diversity=0.5)
    lists = eng.model.beam_search_nbest(eng.modify_visual_inputs(None, supp), 3, groups=3, diversity=0.5)
    want = []
    for image_id, hyps in zip(ids, lists):
        words = [vocab.ix2word[int(t)] for t in hyps[0][0][0].tolist()]
        words = words[1:words.index("<end>")] if "<end>" in words else words[1:]
        want.append({"image_id": image_id, "caption": " ".join(words)})
    assert res == want
    # one group with a penalty is today's search
    assert eng.eval_captions_json_generation(loader, eval_beam_size=3, tqdm_visible=False, beam_groups=1, diversity=0.5) == fx["eval_beam3_json"]
