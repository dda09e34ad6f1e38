"""GPU tests of stochastic beam search as a whole (include/icz.h: icz_*_sample_distinct) at the tiny golden dims, except where said:
BUTD, AoA and NIC and their ensembles against the float64 oracle of tests/_sbs_oracle.py, the Philox path against the host's
restatement, distinctness, the prefix property, log-probabilities against score_captions, determinism, the early-out, refusals
and the Engine methods.  Token-for-token comparisons cover the images whose oracle margins are all above GAP_MIN; the share of those
is asserted (tests/test_cpu_sample_distinct.py asserts it on the oracle alone)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ens_sampling_cases as ec  # noqa: E402
import _sbs_oracle as so  # noqa: E402
from test_gpu_beam_opts import _setup  # noqa: E402

L = so.DECODE_LEN
PHI_TOL = 1e-4                                   # the project's log-prob tolerance


def _sd(*a, **kw):
    from simpleimagecaptionzoo_amd.stochastic_beam import sample_distinct
    out = sample_distinct(*a, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _explicit(u, root):
    return (torch.from_numpy(u).cuda(), torch.from_numpy(root.astype(np.float32)).cuda())


def _captions(ids, lens, n):
    """per image the n captions cut at their length, as tuples"""
    return [[tuple(ids[i * n + j, :lens[i * n + j]].tolist()) for j in range(n)] for i in range(ids.shape[0] // n)]


def _assert_distinct(ids, lens, n, label):
    for i, caps in enumerate(_captions(ids, lens, n)):
        assert len(set(caps)) == n and all(len(c) > 0 for c in caps), (label, i, caps)


def _assert_phi_is_the_score(h, feats, run, n, floor):
    """phi = score_captions on the returned ids, within the project's log-prob tolerance.  score_captions reads a 0 as the end of a
    caption (its rule 1), so a hypothesis that sampled <pad> (0) as a token -- the tiny goldens give it mass -- is scored only up to
    there: those rows are left to the oracle comparison, which holds every phi to the same tolerance; at least `floor` of the rows must remain
    (the tiny goldens, V = 53 .. 70 and 12 steps: a half; full width: 95 %)."""
    from simpleimagecaptionzoo_amd.scoring import score_captions
    ids, lens, _, phi, _ = run
    _, score = score_captions(h, feats, torch.from_numpy(ids).cuda(), n)
    clean = np.array([not (ids[r, :lens[r]] == 0).any() for r in range(ids.shape[0])])
    assert clean.mean() >= floor, clean.mean()
    np.testing.assert_allclose(phi[clean], score.cpu().numpy()[clean], rtol=0, atol=PHI_TOL)


def _same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name,regime", so.DECODE_GOLDENS)
def test_against_the_oracle(golden_dir, name, regime):
    model, h, p, feats = _setup(golden_dir, name, regime, max_rows=24, max_len=L)
    n_img, compared, total = feats.shape[0], 0, 0
    for n, T in so.DECODE_NT:
        u, root = so.decode_noise(so.DECODE_SEEDS.get((name, n, T), 0), n_img, n, h.V)
        ids, lens, fin, phi, G = _sd(h, feats, n, L, T, _explicit(u, root))
        _assert_distinct(ids, lens, n, (name, n, T))
        for img in range(n_img):
            hyps, margin = so.decode_pair(golden_dir, name, regime, n, T, img)
            total += 1
            if margin <= so.GAP_MIN:
                continue
            compared += 1
            w_ids, w_lens, w_fin, w_phi, _ = so.outputs(hyps, n, L)
            sl = slice(img * n, (img + 1) * n)
            assert ids[sl].tolist() == w_ids.tolist() and lens[sl].tolist() == w_lens.tolist() and fin[sl].tolist() == w_fin.tolist(), (name, n, T, img)
            np.testing.assert_allclose(phi[sl], w_phi, rtol=0, atol=PHI_TOL)
            assert (np.diff(G[sl]) < 0).all() and G[img * n] <= so.gumbel(root[img]) + 1e-12
    assert compared >= so.MIN_SHARE * total, (name, compared, total)


def test_aoa_on_per_image_region_counts(golden_dir):
    from simpleimagecaptionzoo_amd.aoa import RegionBatch
    model, h, p, feats = _setup(golden_dir, "aoa_tiny", "track", max_rows=24, max_len=L)
    counts = [feats.shape[1], 20, 11]
    n, T, compared = 5, 1.0, 0
    u, root = so.decode_noise(11, 3, n, h.V)
    ids, lens, fin, phi, G = _sd(h, RegionBatch(feats, counts), n, L, T, _explicit(u, root))
    _assert_distinct(ids, lens, n, "aoa counts")
    for img in range(3):
        gaps = []
        hyps = so.search_model("aoa", feats[img:img + 1, :counts[img]].cpu(), p, n, L, T, so.explicit_noise(u, img), root[img], gaps)
        if min(gaps) <= so.GAP_MIN:
            continue
        compared += 1
        w_ids, w_lens, w_fin, w_phi, _ = so.outputs(hyps, n, L)
        sl = slice(img * n, (img + 1) * n)
        assert ids[sl].tolist() == w_ids.tolist() and lens[sl].tolist() == w_lens.tolist() and fin[sl].tolist() == w_fin.tolist(), img
        np.testing.assert_allclose(phi[sl], w_phi, rtol=0, atol=PHI_TOL)
    assert compared >= 2


@pytest.mark.parametrize("name,regime", so.DECODE_GOLDENS)
def test_philox_determinism_prefix_and_log_probs(golden_dir, name, regime):
    """The seeds are tests/_sbs_oracle.py's: the CPU test asserts that under them EVERY image keeps all its margins above GAP_MIN, so
    the token-for-token comparisons below take all three images."""
    model, h, p, feats = _setup(golden_dir, name, regime, max_rows=24, max_len=L)
    n_img, seed = feats.shape[0], so.PHILOX_SEEDS[name]
    assert n_img == 3
    runs = {}
    for n in (1, 3, 5, 8):
        runs[n] = _sd(h, feats, n, L, 1.0, seed)
        _assert_distinct(runs[n][0], runs[n][1], n, (name, n))
        assert _same_bits(runs[n], _sd(h, feats, n, L, 1.0, seed))                     # two runs are bit-equal
        u, root = so.philox_uniforms(seed, L, n_img, n, h.V)
        assert _same_bits(runs[n], _sd(h, feats, n, L, 1.0, _explicit(u, root))), (name, n)      # Philox = the host's restatement of it
        # log-probabilities: phi is the model's log-probability of the returned caption (T = 1)
        _assert_phi_is_the_score(h, feats, runs[n], n, 0.5)
        for img in range(n_img):                               # and the run is the oracle's under the Philox noise
            w = so.outputs(so.philox_pair(golden_dir, name, regime, n, 1.0, img, seed)[0], n, L)
            assert [runs[n][k][img * n:(img + 1) * n].tolist() for k in (0, 1, 2)] == [w[k].tolist() for k in (0, 1, 2)], (name, n, img)
    # the prefix property: the first j hypotheses of the n = 8 run are the n = j run on the same seed
    for img in range(n_img):
        for j in (1, 3, 5):
            for k in (0, 1, 2):                                    # ids, lens, finished
                assert runs[8][k][img * 8:img * 8 + j].tolist() == runs[j][k][img * j:(img + 1) * j].tolist(), (name, img, j, k)
    # a chunk of a batch (first_image) draws the batch's noise: images 1 .. 2 alone are rows 5 .. of the batch
    tail = _sd(h, feats[1:], 5, L, 1.0, (seed, 1))
    assert [t.tolist() for t in tail[:3]] == [t[5:].tolist() for t in runs[5][:3]]
    # a batch equals its images one by one
    n, T = so.BATCH_NT
    ue, re_ = so.decode_noise(so.BATCH_SEED, n_img, n, h.V)
    whole = _sd(h, feats, n, L, T, _explicit(ue, re_))
    for img in range(n_img):
        one = _sd(h, feats[img:img + 1], n, L, T, _explicit(np.ascontiguousarray(ue[:, img:img + 1]), re_[img:img + 1]))
        assert [t.tolist() for t in one[:3]] == [t[img * n:(img + 1) * n].tolist() for t in whole[:3]], (name, img)
        np.testing.assert_allclose(one[3], whole[3][img * n:(img + 1) * n], rtol=0, atol=PHI_TOL)


@pytest.mark.parametrize("name", ["butd_dec_tiny", "nic_dec_tiny"])
def test_early_out_equals_all_steps(golden_dir, name):
    """A raised <end> bias freezes every row by step 3.  The driver reads the live count back at steps 6, 9, .. below max_len: the
    max_len = 20 run stops at the step-6 read-back, the max_len = 6 run has no read-back and runs every one of its steps, the
    max_len = 5 run likewise.  All three must agree bit for bit on what they share."""
    model, h, p, feats = ec.device_member(golden_dir, name, 0, 40.0, max_rows=24, max_len=20)
    n, seed = 5, 77
    long = _sd(h, feats, n, 20, 1.0, seed)
    assert (long[2] == 1).all() and long[1].max() <= 3
    _assert_distinct(long[0], long[1], n, name)
    for steps in (6, 5):
        every = _sd(h, feats, n, steps, 1.0, seed)
        assert long[0][:, :steps].tolist() == every[0].tolist() and (long[0][:, steps:] == 0).all(), (name, steps)
        assert _same_bits(long[1:], every[1:]), (name, steps)      # lens, finished, phi and G


def _ens_oracle(parts, weights, n, T, u, root, img, gaps):
    step64, state, _ = ec._ens_closure(parts[img], weights, 1)

    def step(prev, st):
        lp, st = step64(prev, st)
        return lp.float(), st
    return so.search(step, state, n, L, T, so.explicit_noise(u, img), root[img], gaps)


def test_ensembles(golden_dir):
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    # an ensemble of one equals its member bit for bit; identical copies equal the single model token for token
    for name in ("butd_dec_tiny", "aoa_tiny", "nic_dec_tiny"):
        members = [ec.device_member(golden_dir, name, 0, max_rows=24, max_len=L) for _ in range(3)]
        h, feats = members[0][1], members[0][3]
        alone = _sd(h, feats, 5, L, 0.7, 31)
        assert _same_bits(alone, _sd(EnsembleHandle([h]), [feats], 5, L, 0.7, 31)), name
        n, T = so.COPIES_NT                                    # every image is separated under this seed (the CPU test asserts it)
        u, root = so.decode_noise(so.COPIES_SEEDS[name], ec.N_IMG, n, h.V)
        single = _sd(h, feats, n, L, T, _explicit(u, root))
        copies = _sd(EnsembleHandle([m[1] for m in members[1:]]), [m[3] for m in members[1:]], n, L, T, _explicit(u, root))
        assert [t.tolist() for t in single[:3]] == [t.tolist() for t in copies[:3]], name
        np.testing.assert_allclose(single[3], copies[3], rtol=0, atol=PHI_TOL)
        for img in range(ec.N_IMG):                            # and both are the oracle's
            w = so.outputs(so.decode_pair(golden_dir, name, "nat", n, T, img, so.COPIES_SEEDS[name])[0], n, L)
            assert [single[k][img * n:(img + 1) * n].tolist() for k in (0, 1, 2)] == [w[k].tolist() for k in (0, 1, 2)], (name, img)
    # BUTD + AoA + NIC against the oracle over the combined closures
    specs, weights, _ = ec.CASES["mixed3"]
    members = [ec.device_member(golden_dir, nm, sd_, max_rows=24, max_len=L) for nm, sd_ in specs]
    ens = EnsembleHandle([m[1] for m in members], weights)
    parts = ec.host_parts([(model, p, f.cpu()) for model, _, p, f in members])
    compared, total = 0, 0
    for n, T in ((3, 1.0), (5, 0.7)):
        u, root = so.decode_noise(8, ec.N_IMG, n, ens.V)
        ids, lens, fin, phi, G = _sd(ens, [m[3] for m in members], n, L, T, _explicit(u, root))
        _assert_distinct(ids, lens, n, ("mixed3", n))
        for img in range(ec.N_IMG):
            gaps = []
            hyps = _ens_oracle(parts, weights, n, T, u, root, img, gaps)
            total += 1
            if min(gaps) <= so.GAP_MIN:
                continue
            compared += 1
            w_ids, w_lens, w_fin, w_phi, _ = so.outputs(hyps, n, L)
            sl = slice(img * n, (img + 1) * n)
            assert ids[sl].tolist() == w_ids.tolist() and lens[sl].tolist() == w_lens.tolist() and fin[sl].tolist() == w_fin.tolist(), (n, T, img)
            np.testing.assert_allclose(phi[sl], w_phi, rtol=0, atol=PHI_TOL)
    assert compared >= so.MIN_SHARE * total - 1e-9, (compared, total)


def test_fullwidth_butd_16_images(golden_dir):
    """BUTD at full width, 16 images x 5, Philox: distinct captions, two runs bit-equal, phi against score_captions"""
    h, feats = _fullwidth_butd(16, 80)
    a = _sd(h, feats, 5, 20, 1.0, 5)
    assert _same_bits(a, _sd(h, feats, 5, 20, 1.0, 5))
    _assert_distinct(a[0], a[1], 5, "full width")
    _assert_phi_is_the_score(h, feats, a, 5, 0.95)             # V = 10 102: <pad> is hardly ever drawn
    assert (np.diff(a[4].reshape(16, 5), axis=1) < 0).all()


def _fullwidth_butd(n_img, max_rows):
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    R, D, H, E, A, V = 36, 2048, 1024, 1024, 1024, 10102
    h = ButdHandle(R, D, H, E, A, V, max_rows, 20)
    params = random_butd_params(R, D, H, E, A, V, "cuda:0", seed=3)
    params["embed.0.weight"] *= 30
    params["predict.weight_g"] *= 15
    h.bind(params)
    torch.manual_seed(0)
    return h, torch.relu(torch.randn(n_img, R, D)).cuda()


def test_refusals_queue_nothing(golden_dir):
    from simpleimagecaptionzoo_amd import stochastic_beam as sb
    from simpleimagecaptionzoo_amd._lib import IczError, SampleDistinctOut, lib, ptr, stream_ptr
    model, h, p, feats = _setup(golden_dir, "butd_dec_tiny", max_rows=8, max_len=L)
    good = _sd(h, feats[:1], 5, L, 1.0, 3)
    outs, st = sb._outputs(8, L, feats.device)
    for t in outs:
        t.fill_(7)
    # rule 6 (capacity: 3 x 5 rows > 8; first_image out of range) and rule 3 (max_len 300) with a live handle, straight at the entry:
    # nothing is written
    assert lib().icz_butd_sample_distinct(h._h, ptr(feats), 3, 5, L, 1.0, 0, 0, None, None, C.byref(st), stream_ptr()) == -1
    assert b"row capacity" in lib().icz_last_error()
    assert lib().icz_butd_sample_distinct(h._h, ptr(feats), 1, 5, L, 1.0, 0, -1, None, None, C.byref(st), stream_ptr()) == -1
    assert b"first_image" in lib().icz_last_error()
    assert lib().icz_butd_sample_distinct(h._h, ptr(feats), 1, 5, 300, 1.0, 0, 0, None, None, C.byref(st), stream_ptr()) == -1
    assert b"max_len" in lib().icz_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)
    with pytest.raises(ValueError, match="row capacity"):
        sb.sample_distinct(h, feats, 5, L)
    # rule 7: an unbound handle
    _, h2, _, _ = _setup(golden_dir, "butd_dec_tiny", max_rows=8, max_len=L, bind=False)
    with pytest.raises(IczError, match="refresh_weights"):
        sb.sample_distinct(h2, feats[:1], 5, L)
    assert _same_bits(good, _sd(h, feats[:1], 5, L, 1.0, 3))       # the handle is as it was


def _butd_engine(env, max_batch, param_seed):
    """tests/test_gpu_caption_sets.py's BUTD engine with a row capacity and parameters of the caller's choice"""
    import test_gpu_caption_sets as tcs
    from simpleimagecaptionzoo_amd.engine import BUTDDetection_Eng
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    R, D, H, E, A = 36, 128, 64, 64, 64
    eng = BUTDDetection_Eng({"model_type": "BUTDDetection", "atten_dim": A, "embed_dim": E, "hidden_dim": H, "enc_dim": D},
                            "SYN", env.vocab, data_dir="/tmp/", device="cuda:0", cider_df=env.tables["big"]["dfd"], max_batch=max_batch)
    params = random_butd_params(R, D, H, E, A, tcs.V, "cuda:0", seed=param_seed)
    params["embed.0.weight"] *= 30
    params["predict.weight_g"] *= 15
    eng.model.load_state_dict({"decoder." + k: v for k, v in params.items()})
    return eng


def _entries_by_hand(vocab, loader, K, decode):
    """decode(batch index, supp) -> (ids, lens, finished, phi, G) of the batch; the entries the Engine methods document"""
    want = []
    for bi, (image_ids, _, supp) in enumerate(loader):
        ids, lens, fin, phi, G = decode(bi, supp)
        for r in range(ids.shape[0]):
            toks = ids[r, :lens[r]].tolist()
            toks = toks[:min([i for i, w in enumerate(toks) if w in (0, 2)] + [len(toks)])]      # the caption ends at <end> or <pad>
            words = [vocab.ix2word[w] for w in toks if w != 1]
            want.append({"image_id": image_ids[r // K], "caption": " ".join(words), "score": float(phi[r]), "perturbed": float(G[r])})
    return want


def test_engine_methods(golden_dir):
    import test_gpu_caption_sets as tcs
    from simpleimagecaptionzoo_amd import engine as E
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    from simpleimagecaptionzoo_amd.stochastic_beam import captioner_sample_distinct
    env = tcs._Env()
    try:
        eng, loader, vocab, dfd, B = tcs._butd_engine(env)
        K, T, seed = 5, 0.8, 6
        feats_of = lambda e, supp: e._features(e.modify_visual_inputs(img_tensors=None, supp_info_datas=supp))      # noqa: E731
        entries = eng.sample_distinct_captions_json_generation(loader, K, T, seed, tqdm_visible=False)
        assert len(entries) == B * K and [e["image_id"] for e in entries] == [i for i in range(B) for _ in range(K)]
        # the entries driven by hand: batch i draws from seed * 2^20 + i
        assert entries == _entries_by_hand(vocab, loader, K, lambda bi, supp: _sd(eng._hot_handle(), feats_of(eng, supp), K, 20, T, (seed << 20) + bi))
        vi = eng.modify_visual_inputs(img_tensors=None, supp_info_datas=loader[0][2])
        cap = [t.cpu().numpy() for t in captioner_sample_distinct(eng.model, vi, K, 20, T, seed << 20)]
        assert _same_bits(cap, _sd(eng._hot_handle(), eng._features(vi), K, 20, T, seed << 20))
        for i in range(B):
            g = [e["perturbed"] for e in entries[i * K:(i + 1) * K]]
            assert all(a > b for a, b in zip(g, g[1:]))
        # chunked equals whole: an engine of the same parameters whose handle holds one image's rows decodes every batch of two images
        # in two chunks, each drawing its image's noise within the batch
        small = _butd_engine(env, 1, 3)
        assert small._hot_handle().max_rows // K == 1 and all(len(b[0]) == 2 for b in loader)
        chunked = small.sample_distinct_captions_json_generation(loader, K, T, seed, tqdm_visible=False)
        assert [(e["image_id"], e["caption"]) for e in chunked] == [(e["image_id"], e["caption"]) for e in entries]
        np.testing.assert_allclose([e["score"] for e in chunked], [e["score"] for e in entries], rtol=0, atol=PHI_TOL)
        # the consensus method = the sampling method followed by rerank_captions_json
        assert eng.consensus_distinct_captions_json_generation(loader, K, T, seed, tqdm_visible=False) == eng.rerank_captions_json(entries, K)
        # ensembles: of one engine = the engine; an engine twice is refused (one handle cannot serve two members); two engines = the
        # EnsembleHandle over their handles driven by hand, through the combined rows
        assert E.sample_distinct_ensemble_captions_json_generation([eng], loader, K, T, seed, tqdm_visible=False) == entries
        with pytest.raises(ValueError, match="twice"):
            E.sample_distinct_ensemble_captions_json_generation([eng, eng], loader, K, T, seed, tqdm_visible=False)
        eng2 = _butd_engine(env, 32, 4)
        got2 = E.sample_distinct_ensemble_captions_json_generation([eng, eng2], loader, K, T, seed, tqdm_visible=False, weights=[1.0, 3.0])
        ens = EnsembleHandle([eng._hot_handle(), eng2._hot_handle()], [1.0, 3.0])
        want2 = _entries_by_hand(vocab, loader, K, lambda bi, supp: _sd(ens, [feats_of(eng, supp), feats_of(eng2, supp)], K, 20, T, (seed << 20) + bi))
        assert got2 == want2 and [e["caption"] for e in got2] != [e["caption"] for e in entries]
        with pytest.raises(ValueError):
            eng.sample_distinct_captions_json_generation(loader, 9, T, seed, tqdm_visible=False)
        with pytest.raises(ValueError):
            eng.sample_distinct_captions_json_generation(loader, K, 0.0, seed, tqdm_visible=False)
        with pytest.raises(ValueError):
            eng.consensus_distinct_captions_json_generation(loader, 1, T, seed, tqdm_visible=False)
    finally:
        for t in env.tables.values():
            t["scorer"].close()
