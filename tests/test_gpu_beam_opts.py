"""GPU tests of the beam-search options (include/icz.h: icz_beam_opts -- n-best lists, length penalty, n-gram blocking) for the BUTD,
AoA and NIC decoders against the host oracle of tests/_beam_opts_oracle.py, teacher-forced log-probabilities and today's search."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _beam_opts_oracle as bo  # noqa: E402
from oracle import butd as ob  # noqa: E402
from synth import feats_from_seed  # noqa: E402

GOLDENS = ["butd_dec_tiny", "butd_dec_odd", "aoa_tiny", "nic_dec_tiny", "nic_dec_odd"]
LP = {None: (0, 0.0), ("avg", 0.7): (1, 0.7), ("wu", 0.9): (2, 0.9)}


def _regime(sd, g, regime, pre):
    sd = {k: v.copy() for k, v in sd.items()}
    if regime == "track":          # <end> competes in mid-sentence: finished and live hypotheses side by side
        tok = int(g["beam_track_tok"])
        for s in ("weight_v", "weight_g"):
            sd[pre + "predict." + s][2] = sd[pre + "predict." + s][tok]
        sd[pre + "predict.bias"][2] = sd[pre + "predict.bias"][tok] - 0.2
    return sd


def _setup(golden_dir, name, regime="nat", max_rows=16, max_len=20, bind=True):
    """-> (model, device handle, CPU parameters for the oracle, device features of up to 3 images); bind=False: the handle is left
    unbound"""
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
    if name.startswith("butd"):
        from simpleimagecaptionzoo_amd.butd import ButdHandle
        model, sd = "butd", _regime(ob.strip_prefix(sd), g, regime, "")
        B, R, D, H, E, A, V = [int(x) for x in g["dims"]]
        h = ButdHandle(R, D, H, E, A, V, max_rows, max_len)
        feats = torch.tensor(g["feats"])
    elif name.startswith("aoa"):
        from simpleimagecaptionzoo_amd.aoa import AoaHandle
        model, sd = "aoa", _regime(sd, g, regime, "decoder.")
        B, R, D, Hd, E, V, NH = [int(x) for x in g["dims"]]
        h = AoaHandle(R, D, Hd, E, V, NH, max_rows, max_len)
        feats = torch.from_numpy(feats_from_seed(int(g["feats_seed"]), B, R, D))
    else:
        from simpleimagecaptionzoo_amd.nic import NicHandle
        model, sd = "nic", _regime(sd, g, regime, "")
        B, H, E, V = [int(x) for x in g["dims"]]
        h = NicHandle(E, H, V, max_rows, max_len)
        feats = torch.tensor(g["feats"])
    params = {k: torch.tensor(np.asarray(v), dtype=torch.float32, device="cuda") for k, v in sd.items()}
    if bind:
        h.bind(params)
    p = {k: v.cpu() for k, v in params.items()}
    return model, h, p, feats[:min(3, feats.shape[0])].contiguous().cuda()


def _lists(seqs, lens, scores):
    seqs, lens, scores = seqs.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()
    return [[(seqs[i, j, :lens[i, j]].astype(int).tolist(), float(scores[i, j])) for j in range(lens.shape[1])]
            for i in range(lens.shape[0])]


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("regime", ["nat", "track"])
def test_defaults_are_todays_beam_search(golden_dir, name, regime):
    _, h, _, feats = _setup(golden_dir, name, regime)
    for k in (1, 3, 5):
        seqs, lens = h.beam_search(feats, k, 50)
        s2, l2, sc = h.beam_search_opts(feats, k, 50)
        assert s2.shape == (feats.shape[0], 1, 51) and l2.shape == sc.shape == (feats.shape[0], 1)
        assert torch.equal(s2[:, 0], seqs) and torch.equal(l2[:, 0], lens), (name, regime, k)
        assert torch.isfinite(sc).all()


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_tiny"])
def test_unrefreshed_handle_is_refused_by_every_beam_entry(golden_dir, name):
    """The refresh check of the shared beam driver: a handle that was never bound is refused by icz_*_beam_search, _opts and
    _diverse with the family's own hint; once bound, the same handle searches as test_defaults_are_todays_beam_search expects."""
    from simpleimagecaptionzoo_amd._lib import IczError
    model, h, p, feats = _setup(golden_dir, name, bind=False)
    assert feats.shape[0] == 3
    hint = "icz_%s_refresh_weights" % model
    with pytest.raises(IczError, match=hint):
        h.beam_search(feats, 3, 20)
    with pytest.raises(IczError, match=hint):
        h.beam_search_opts(feats, 3, 20)
    with pytest.raises(IczError, match=hint):
        h.beam_search_opts(feats, 3, 20, groups=3, diversity=0.5)
    h.bind({k: v.cuda() for k, v in p.items()})
    seqs, lens = h.beam_search(feats, 3, 20)
    s2, l2, sc = h.beam_search_opts(feats, 3, 20)
    assert s2.shape == (3, 1, 21) and l2.shape == sc.shape == (3, 1)
    assert torch.equal(s2[:, 0], seqs) and torch.equal(l2[:, 0], lens)
    assert torch.isfinite(sc).all()
    _, ref, _, _ = _setup(golden_dir, name)                # a handle bound from the start
    want_seqs, want_lens = ref.beam_search(feats, 3, 20)
    assert torch.equal(seqs, want_seqs) and torch.equal(lens, want_lens) and (lens > 1).all()


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("regime", ["nat", "track"])
def test_nbest_token_exact_against_the_oracle(golden_dir, name, regime):
    model, h, p, feats = _setup(golden_dir, name, regime)
    for k in (1, 3, 5):
        for block, lp in ((2, None), (3, None), (0, ("avg", 0.7)), (0, ("wu", 0.9)), (3, ("wu", 0.9))):
            got = _lists(*h.beam_search_opts(feats, k, 50, n_best=k, length_penalty=lp, block_ngram=block))
            for i in range(feats.shape[0]):
                want = bo.nbest(model, feats[i:i + 1].cpu(), p, k, 50, block, *LP[lp])
                assert [w[0] for w in want] == [x[0] for x in got[i]], (name, regime, k, block, lp, i)
                np.testing.assert_allclose([x[1] for x in got[i]], [w[1] for w in want], atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", GOLDENS)
def test_blocking_removes_repeated_ngrams(golden_dir, name):
    _, h, _, feats = _setup(golden_dir, name, "nat")
    k = 5
    free = _lists(*h.beam_search_opts(feats, k, 50, n_best=k))
    # the regime does what it is for: the unblocked beam loops on these small decoders
    assert any(bo.repeats_ngram(x[0], 3) for img in free for x in img)
    for n in (2, 3, 4):
        got = _lists(*h.beam_search_opts(feats, k, 50, n_best=k, block_ngram=n))
        for img in got:
            assert len(img) == k
            for toks, sc in img:
                assert not bo.repeats_ngram(toks, n), (n, toks)
                assert np.isfinite(sc)


def _teacher_forced_scores(model, golden_dir, name, regime, feats, hyps):
    """fp32 sums of eval-mode log_softmax over each hypothesis's tokens, from one teacher-forced xe_forward per image"""
    _, h, _, _ = _setup(golden_dir, name, regime, max_rows=16, max_len=52)
    out = []
    for i, img in enumerate(hyps):
        order = sorted(range(len(img)), key=lambda j: -len(img[j][0]))        # xe_forward wants lengths sorted descending
        steps = [len(img[j][0]) - 1 for j in order]
        caps = torch.zeros(len(img), max(steps) + 1, dtype=torch.int64)
        for b, j in enumerate(order):
            caps[b, :len(img[j][0])] = torch.tensor(img[j][0])
        f = feats[i:i + 1].expand(len(img), *feats.shape[1:]).contiguous()
        logits = h.xe_forward(f, caps.cuda(), steps, None, train=False, want_logits=True)
        lsm = torch.log_softmax(logits.double().cpu(), 1).float().numpy()
        acc = [np.float32(0)] * len(img)
        for row, (b, t) in enumerate(ob.packed_order(steps)):
            acc[b] = np.float32(acc[b] + lsm[row, int(caps[b, t + 1])])
        res = [0.0] * len(img)
        for b, j in enumerate(order):
            res[j] = float(acc[b])
        out.append(res)
    return out


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd"])
def test_scores_are_model_log_probs(golden_dir, name):
    model, h, _, feats = _setup(golden_dir, name, "track")
    kinds = set()
    for steps in (50, 8):                    # 8 steps: beams still live at the step limit
        got = _lists(*h.beam_search_opts(feats, 5, steps, n_best=5, length_penalty="wu_0.9", block_ngram=3))
        want = _teacher_forced_scores(model, golden_dir, name, "track", feats, got)
        for img, w in zip(got, want):
            for (toks, sc), ws in zip(img, w):
                kinds.add(toks[-1] == 2)
                assert abs(sc - ws) <= 1e-4, (toks, sc, ws)
    assert kinds == {True, False}            # finished and live-at-the-limit hypotheses both checked


@pytest.mark.parametrize("name", GOLDENS)
def test_list_is_well_formed(golden_dir, name):
    from simpleimagecaptionzoo_amd.beam import parse_length_penalty
    _, h, _, feats = _setup(golden_dir, name, "track")
    k = 5
    for block, lp in ((3, "wu_0.9"), (0, "avg_0.7"), (2, None)):
        seqs, lens, scores = h.beam_search_opts(feats, k, 50, n_best=k, length_penalty=lp, block_ngram=block)
        kind, alpha = parse_length_penalty(lp)
        for img in _lists(seqs, lens, scores):
            assert len(img) == k and all(len(t) >= 2 for t, _ in img)
            fin = [t[-1] == 2 for t, _ in img]
            assert fin == sorted(fin, reverse=True)                       # finished before live
            for a, b in zip(img, img[1:]):
                if (a[0][-1] == 2) == (b[0][-1] == 2):
                    assert bo.lp_norm(a[1], len(a[0]) - 1, kind, alpha) >= bo.lp_norm(b[1], len(b[0]) - 1, kind, alpha)
        one = h.beam_search_opts(feats, k, 50, n_best=1, length_penalty=lp, block_ngram=block)
        assert torch.equal(one[0][:, 0], seqs[:, 0]) and torch.equal(one[1][:, 0], lens[:, 0]) and torch.equal(one[2][:, 0], scores[:, 0])
    # avg with alpha = 0 divides by 1: the order of no penalty
    a0 = h.beam_search_opts(feats, k, 50, n_best=k, length_penalty=("avg", 0.0), block_ngram=3)
    no = h.beam_search_opts(feats, k, 50, n_best=k, block_ngram=3)
    assert all(torch.equal(x, y) for x, y in zip(a0, no))


def test_fullwidth_butd_beam5_128_images(golden_dir):
    """Beam 5 over 128 images at the benchmark width (sharpened weights, tests/_fullwidth.py): defaults equal today's search bit
    for bit; blocking + penalty + the whole n-best list of 6 images equal the oracle's."""
    from _fullwidth import A, D, E, H, R, V, _cpu, _full_params
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    params = _full_params(seed=78)
    n_img, k, steps = 128, 5, 20
    h = ButdHandle(R, D, H, E, A, V, n_img * k, 20)
    h.bind(params)
    torch.manual_seed(6)
    feats = torch.relu(torch.randn(n_img, R, D, device="cuda"))
    seqs, lens = h.beam_search(feats, k, steps)
    s2, l2, _ = h.beam_search_opts(feats, k, steps)
    assert torch.equal(s2[:, 0], seqs) and torch.equal(l2[:, 0], lens)
    got = _lists(*h.beam_search_opts(feats, k, steps, n_best=k, length_penalty="wu_0.9", block_ngram=3))
    one = h.beam_search_opts(feats, k, steps, n_best=1, length_penalty="wu_0.9", block_ngram=3)
    p = _cpu(params)
    differ = []
    for i in (0, 25, 50, 77, 101, 127):
        want = bo.nbest("butd", feats[i:i + 1].cpu(), p, k, steps, 3, 2, 0.9)
        if [w[0] for w in want] != [x[0] for x in got[i]]:
            differ.append((i, got[i], want))
        assert one[1][i, 0] == len(got[i][0][0]) and one[0][i, 0, :len(got[i][0][0])].long().tolist() == got[i][0][0]
    assert not differ, differ          # sharpened weights: no near-ties (as the existing full-width beam tests)
    h.close()


def test_engine_eval_json_with_options(golden_dir):
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
    res = eng.eval_captions_json_generation(loader, eval_beam_size=3, tqdm_visible=False, block_ngram=3, length_penalty="wu_0.9")
    vi = eng.modify_visual_inputs(None, supp)
    seqs, lens, _ = eng._hot_handle().beam_search_opts(eng._features(vi), 3, 50, 1, "wu_0.9", 3)
    want = []
    for i, image_id in enumerate(ids):
        words = [vocab.ix2word[int(t)] for t in seqs[i, 0, :int(lens[i, 0])].tolist()]
        words = words[1:words.index("<end>")] if "<end>" in words else words[1:]
        want.append({"image_id": image_id, "caption": " ".join(words)})
    assert res == want
