"""Multi-sample SCST with a leave-one-out baseline (beyond the reference: K sampled captions per image, each baselined by the mean
CIDEr-D of the other K - 1, no greedy rollout): the BUTD rollout icz_butd_sample_n against icz_butd_sample on the features repeated
K times, its two attention routes (option group_att), graphs and early-out against themselves, its REINFORCE gradients, the device
leave-one-out reward against a host restatement, the Engine's samples_per_image step against the same step built by hand, the
argument errors, and two data-parallel ranks against one process."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _fullwidth import A, D, E, H, R, V, _end_biased_params, attention_kink_units, check_grads_against_float64  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
T = 20


def _rng(rows, seed, explicit, r=R, e=E, a=A, h=H, steps=T):
    """explicit: uniforms / keep-masks laid out for `rows` decoder rows (the B K space), else Philox from `seed`"""
    from simpleimagecaptionzoo_amd.butd import make_rng
    if not explicit:
        return make_rng(seed)
    rs = np.random.RandomState(seed)
    em, am, om = rs.rand(steps, rows, e) < 0.5, rs.rand(steps, rows, r, a) < 0.5, rs.rand(steps, rows, h) < 0.5
    u = rs.rand(steps, rows).astype(np.float32)
    dev = "cuda"
    return make_rng(0, torch.tensor(u, device=dev), torch.tensor(em.astype(np.uint8), device=dev),
                    torch.tensor(am.astype(np.uint8), device=dev), torch.tensor(om.astype(np.uint8), device=dev))


def _feats(B, seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.relu(torch.randn(B, R, D, generator=g)).cuda()


def _run(h, feats, K, rng, **opts):
    """sample_n under one option ({"graphs": 1} captures and replays: the second call is a replay), options restored after"""
    for k, v in opts.items():
        h.enable_graphs(True) if k == "graphs" else h.set_option(k, v)
    try:
        for _ in range(2 if "graphs" in opts else 1):
            seq, lp = h.sample_n(feats, K, T, rng)
        return seq.cpu().numpy().copy(), lp.cpu().numpy().copy()
    finally:
        for k in opts:
            h.enable_graphs(False) if k == "graphs" else h.set_option(k, {"group_att": 0}.get(k, 1))


@pytest.fixture(scope="module")
def full():
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    params = random_butd_params(R, D, H, E, A, V, "cuda", seed=61)
    params["predict.weight_g"].mul_(6.0)
    h = ButdHandle(R, D, H, E, A, V, 320, T)
    h.bind(params)
    yield h, params
    h.close()


def _compare_to_repeated(h, feats, K, rng_n, rng_r):
    B = feats.shape[0]
    seq_n, lp_n = (x.cpu().numpy().copy() for x in h.sample_n(feats, K, T, rng_n))
    seq_r, lp_r = (x.cpu().numpy().copy() for x in h.sample(feats.repeat_interleave(K, 0).contiguous(), T, rng_r))
    same = (seq_n == seq_r).all(1)
    # the per-image GEMMs run at M = B R here against B K R there: a draw within fp32 rounding of a CDF edge may go the other way
    assert (~same).sum() <= max(1, B * K // 32), int((~same).sum())
    np.testing.assert_allclose(lp_n[same], lp_r[same], atol=1e-5, rtol=0)
    return seq_n, lp_n


@pytest.mark.parametrize("B,K", [(1, 2), (13, 5), (64, 5), (16, 8)])
@pytest.mark.parametrize("explicit", [True, False])
def test_sample_n_draws_what_sample_draws_on_repeated_features(full, B, K, explicit):
    h, _ = full
    feats = _feats(B, 100 + B)
    seed = 7 * B + K
    seq, lp = _compare_to_repeated(h, feats, K, _rng(B * K, seed, explicit), _rng(B * K, seed, explicit))
    # the two attention routes, graphs on / off (Philox: explicit arrays bypass the graphs) and early-out on / off: bitwise
    for opts in ({"group_att": 1}, {"graphs": 1}, {"early_out": 0}):
        if "graphs" in opts and explicit:
            continue
        s2, l2 = _run(h, feats, K, _rng(B * K, seed, explicit), **opts)
        assert np.array_equal(s2, seq) and np.array_equal(l2.view(np.int32), lp.view(np.int32)), opts


def test_sample_n_with_the_break_firing():
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    params, feats = _end_biased_params(91, 0.35, B=16)
    K = 4
    h = ButdHandle(R, D, H, E, A, V, 64, T)
    h.bind(params)
    seq, lp = _compare_to_repeated(h, feats, K, _rng(16 * K, 3, True), _rng(16 * K, 3, True))
    ended = [int(np.nonzero(r == 0)[0][0]) if (r == 0).any() else T for r in seq]
    assert max(ended) < T - 2, ended                      # every row has ended well before the last step: the break fired
    for opts in ({"group_att": 1}, {"early_out": 0}):
        s2, l2 = _run(h, feats, K, _rng(16 * K, 3, True), **opts)
        assert np.array_equal(s2, seq) and np.array_equal(l2.view(np.int32), lp.view(np.int32)), opts
    h.close()


def _grads_behind(h, run, reward):
    run()
    g = h.new_grads()
    h.sample_backward(reward, g)
    return {k: v.cpu().numpy().copy() for k, v in g.items()}


def _close_per_unit(got, want, k, tol, rows):
    """|got - want| <= tol max|want| per tensor, except for attention units (rows of enc_att / dec_att, elements of affine) that a relu
    kink explains: the per-image enc_ctx of sample_n rounds differently from the repeated features' (another GEMM M), and an element
    within fp32 rounding of zero flips its relu -- a finite change of the unit's gradient.  tests/_fullwidth.py
    check_grads_against_float64 admits 1 % of the units at 64 rows, capped at 2e-2 of the maximum; the number of (row, region, step)
    elements that can flip grows with the rows, so the share here is 1 % per 64 rows (320 rows: 5 %)"""
    scale = max(1e-30, float(np.abs(want).max()))
    e = np.abs(got.astype(np.float64) - want).reshape(got.shape[0], -1).max(1) if got.ndim >= 2 else np.abs(got.astype(np.float64) - want)
    bad = e > tol * scale
    if not bad.any():
        return
    assert k.startswith("atten."), (k, float(e.max() / scale))
    assert bad.sum() <= max(1, bad.size * rows // 6400) and e.max() <= 2e-2 * scale, (k, int(bad.sum()), float(e.max() / scale))


@pytest.mark.parametrize("B,K,seed", [(6, 4, 11), (64, 5, 12)])
def test_sample_n_gradients(full, B, K, seed):
    """(64, 5): 6 400 (t, b) pairs, the windowed embedding-gradient kernel"""
    h, _ = full
    feats = _feats(B, 5)
    rows = B * K
    seq_n, _ = h.sample_n(feats, K, T, _rng(rows, seed, True))
    seq_r, _ = h.sample(feats.repeat_interleave(K, 0).contiguous(), T, _rng(rows, seed, True))
    same = (seq_n.cpu().numpy() == seq_r.cpu().numpy()).all(1)
    rw = np.random.RandomState(2).randn(rows, 1).astype(np.float32).repeat(T, 1)
    if rows <= 32:
        assert same.all()                                   # this seed: every id matches
    else:       # 320 rows: a draw at a CDF edge may differ (test above); such a row gets reward 0 and adds nothing to any gradient
        assert (~same).sum() <= max(1, rows // 32), int((~same).sum())
        rw[~same] = 0.0
    rw = torch.tensor(rw, device="cuda")
    h.set_option("group_att", 1)
    try:
        g_grp = _grads_behind(h, lambda: h.sample_n(feats, K, T, _rng(rows, seed, True)), rw)
    finally:
        h.set_option("group_att", 0)
    g_row = _grads_behind(h, lambda: h.sample_n(feats, K, T, _rng(rows, seed, True)), rw)
    g_rep = _grads_behind(h, lambda: h.sample(feats.repeat_interleave(K, 0).contiguous(), T, _rng(rows, seed, True)), rw)
    for k in g_grp:
        _close_per_unit(g_grp[k], g_rep[k], k, 1e-4, rows)
        if k.startswith(("atten.enc_att", "atten.affine")) or k == "TD_atten.weight_ih":
            # the K rows of an image are summed in another order on the two routes
            assert float(np.abs(g_grp[k] - g_row[k]).max()) <= 1e-5 * max(1e-30, float(np.abs(g_grp[k]).max())), k
        else:
            assert np.array_equal(g_grp[k].view(np.int32), g_row[k].view(np.int32)), k


def test_sample_n_gradients_against_float64_oracle():
    from oracle import butd as ob
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.ciderd import loo_baseline_reward
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    r, d, hh, e, a, v = 10, 128, 64, 64, 64, 203
    B, K = 3, 4
    rows = B * K
    params = random_butd_params(r, d, hh, e, a, v, "cuda", seed=4)
    h = ButdHandle(r, d, hh, e, a, v, rows, T)
    h.bind(params)
    g = torch.Generator(device="cpu")
    g.manual_seed(12)
    feats = torch.relu(torch.randn(B, r, d, generator=g))
    rs = np.random.RandomState(8)
    em, am, om = rs.rand(T, rows, e) < 0.5, rs.rand(T, rows, r, a) < 0.5, rs.rand(T, rows, hh) < 0.5
    u = rs.rand(T, rows).astype(np.float32)
    dev = "cuda"
    from simpleimagecaptionzoo_amd.butd import make_rng
    rng = make_rng(0, torch.tensor(u, device=dev), torch.tensor(em.astype(np.uint8), device=dev),
                   torch.tensor(am.astype(np.uint8), device=dev), torch.tensor(om.astype(np.uint8), device=dev))
    seq, _ = h.sample_n(feats.cuda(), K, T, rng)
    seq = seq.cpu().numpy()
    scores = np.random.RandomState(3).rand(rows)                    # per-caption scores -> the leave-one-out reward
    rw = np.repeat(loo_baseline_reward(scores, K)[:, None], T, 1)
    grads = h.new_grads()
    h.sample_backward(torch.tensor(rw, device=dev), grads)
    gsets, trace = {}, {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            p = {k: t.detach().cpu().to(dt).requires_grad_(True) for k, t in params.items()}
            w_seq, w_lp, _ = ob.sample_rl(feats.to(dt).repeat_interleave(K, 0), p, u.astype(np.float64), em, am, om, T,
                                          trace=trace if name == "f64" else None)
            assert np.array_equal(w_seq.numpy(), seq), name
            ob.reward_criterion(w_lp, w_seq, torch.from_numpy(rw).to(dt)).backward()
            gsets[name] = {k: t.grad.numpy() for k, t in p.items()}
            if name == "f64":
                p64 = {k: t.detach() for k, t in p.items()}
        finally:
            torch.set_default_dtype(torch.float32)
    kink = attention_kink_units(feats.double().repeat_interleave(K, 0), p64, trace["h1"], am)
    check_grads_against_float64(grads, gsets["f32"], gsets["f64"], {"atten.enc_att": kink, "atten.dec_att": kink})
    h.close()


# ---- reward ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scorer():
    from simpleimagecaptionzoo_amd.ciderd import CiderDReward
    from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    vocab = synthetic_vocab(203)
    words = [vocab.ix2word[i] for i in range(203)]
    dfd = document_frequency(synthetic_references(300, words, seed=0))
    refs = synthetic_references(40, words, seed=9)
    return CiderDReward(dfd["document_frequency"], dfd["ref_len"], vocab.word2ix, "cuda"), {i: refs[i] for i in range(40)}


def _loo_check(sc, gts, gen, K, ids):
    from simpleimagecaptionzoo_amd.ciderd import loo_baseline_reward
    gen = torch.as_tensor(gen, dtype=torch.int64, device="cuda")
    rep_ids = [i for i in ids for _ in range(K)]
    _, scores = sc.reward(gen, gen, gts, rep_ids, return_scores=True)
    s = scores.cpu().numpy()[:gen.shape[0]]
    reward, s2 = sc.reward_loo(gen, K, gts, ids, return_scores=True)
    assert np.array_equal(s2.cpu().numpy(), s)
    want = np.repeat(loo_baseline_reward(s, K)[:, None], gen.shape[1], 1)
    got = reward.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    return got


def _captions(rows, seed, vocab=203):
    rs = np.random.RandomState(seed)
    gen = rs.randint(4, vocab, size=(rows, T))
    for i, L in enumerate(rs.randint(3, T, size=rows)):
        gen[i, L:] = 0
    return gen


def test_reward_loo_matches_host_leave_one_out(scorer):
    sc, gts = scorer
    _loo_check(sc, gts, _captions(2 * 5, 1), 2, [0, 1, 2, 3, 4])                     # K = 2
    same = np.repeat(_captions(3, 2), 4, 0)                                       # K identical samples: reward 0
    assert (_loo_check(sc, gts, same, 4, [5, 6, 7]) == 0).all()
    ends = np.zeros((2 * 3, T), np.int64)                                         # all-<end> rows
    _loo_check(sc, gts, ends, 3, [8, 9])
    _loo_check(sc, gts, _captions(4 * 4, 3), 4, [1, 2, 20, 21])                   # stored images (1, 2) beside new ones (20, 21)


def test_reward_loo_rejects_bad_arguments(scorer):
    from simpleimagecaptionzoo_amd._lib import IczError
    sc, gts = scorer
    gen = torch.zeros(6, T, dtype=torch.int64, device="cuda")
    for n, ids in ((1, [0] * 6), (9, [0]), (3, [0, 1, 2])):
        with pytest.raises(IczError):
            sc.reward_loo(gen, n, gts, ids)


# ---- engine ------------------------------------------------------------------------------------------------------------------
def _engine(g, fx, cls=None):
    from simpleimagecaptionzoo_amd.engine import BUTDDetection_Eng
    from simpleimagecaptionzoo_amd.vocab import Caption_Vocabulary
    B, R_, D_, H_, E_, A_, V_ = [int(x) for x in g["dims"]]
    vocab = Caption_Vocabulary()
    for w in fx["vocab"]:
        vocab.add_word(w)
    df = {"document_frequency": {tuple(k): v for k, v in fx["df"]["document_frequency"]}, "ref_len": fx["df"]["ref_len"]}
    eng = BUTDDetection_Eng({"model_type": "BUTDDetection", "atten_dim": A_, "embed_dim": E_, "hidden_dim": H_},
                            "SYN", vocab, data_dir="/tmp/", use_bu="fixed", device="cuda:0", cider_df=df, max_batch=32)
    sd = {k[4:]: torch.tensor(v) for k, v in g.items() if k.startswith("sd0.")}
    eng.model.load_state_dict(sd, strict=True)
    return eng


def _steps(golden_dir, K, rows_rng_seed=5):
    import test_gpu_engine as tge
    from synth import feats_from_seed
    g, fx = tge._load(golden_dir)
    B, R_, D_, H_, E_, A_, V_ = [int(x) for x in g["dims"]]
    batches, rngs = [], []
    for s in range(2):
        pre = "rl%d_" % s
        feats = feats_from_seed(int(g[pre + "feats_seed"]), B, R_, D_)
        ids = tuple(int(i) for i in g[pre + "img_ids"])
        gts = {int(k): v for k, v in fx[pre + "gts"].items()}
        batches.append((ids, None, gts, tge._supp(feats)))
        rngs.append(lambda s=s: _rng(B * K, rows_rng_seed + s, True, R_, E_, A_, H_))
    return g, fx, batches, rngs


def _params(eng):
    return {k: v.detach().cpu().numpy().copy() for k, v in eng.model.state_dict().items()}


def test_engine_samples_per_image_step_equals_the_step_built_by_hand(golden_dir):
    from simpleimagecaptionzoo_amd.ciderd import loo_baseline_reward
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    K = 5
    g, fx, batches, rngs = _steps(golden_dir, K)
    eng = _engine(g, fx)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    for b, r in zip(batches, rngs):
        eng.SCST_training_epoch([b], opt, None, tqdm_visible=False, rngs=[r()], samples_per_image=K)
    torch.cuda.synchronize()
    got = _params(eng)
    # the same two steps by hand on a second engine: sample_n, the host leave-one-out reward, sample_backward, clamp 0.25 + Adam
    ref = _engine(g, fx)
    opt2 = init_optimizer("Adam", ref.model.get_param_groups({"lr": 2e-5}), 2e-5)
    with torch.cuda.stream(ref.stream):
        for (ids, _, gts, supp), r in zip(batches, rngs):
            ref.model.train()
            feats = ref._features(ref.modify_visual_inputs(None, supp))
            h = ref._hot_handle()
            seq, _ = h.sample_n(feats, K, 20, r())
            rep_ids = [i for i in ids for _ in range(K)]
            _, scores = ref.scorer().reward(seq, seq, gts, rep_ids, return_scores=True)
            s = scores.cpu().numpy()[:seq.shape[0]]
            rw = torch.tensor(np.repeat(loo_baseline_reward(s, K)[:, None], 20, 1), device="cuda")
            grads = ref._grads()
            h.sample_backward(rw, grads)
            ref._apply(opt2, 0.25)
    torch.cuda.synchronize()
    want = _params(ref)
    # same kernels, same launch order, the Engine's own stream: bitwise
    for k in want:
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k


def test_engine_samples_per_image_none_is_todays_step(golden_dir):
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    g, fx, batches, _ = _steps(golden_dir, 1)
    import test_gpu_engine as tge
    B, R_, D_, H_, E_, A_, V_ = [int(x) for x in g["dims"]]
    out = []
    for kw in ({}, {"samples_per_image": None}):
        eng = _engine(g, fx)
        opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
        for s, b in enumerate(batches):
            eng.SCST_training_epoch([b], opt, None, tqdm_visible=False, rngs=[_rng(B, 40 + s, True, R_, E_, A_, H_)], **kw)
        torch.cuda.synchronize()
        out.append(_params(eng))
    for k in out[0]:
        assert np.array_equal(out[0][k].view(np.int32), out[1][k].view(np.int32)), k


def test_errors_queue_nothing(golden_dir, full):
    import test_gpu_engine as tge
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, NIC_Eng, init_optimizer
    h, _ = full
    feats = _feats(64, 1)
    torch.cuda.synchronize()
    g, fx = tge._load(golden_dir)
    eng = _engine(g, fx)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    torch.cuda.synchronize()
    mem0, bufs0 = torch.cuda.memory_allocated(), dict(h._bufs)
    for n in (1, 9):
        with pytest.raises(IczError, match="samples per image"):
            h.sample_n(feats, n, T)
    with pytest.raises(IczError, match="capacity"):
        h.sample_n(feats, 6, T)                                     # 384 rows > 320
    for n in (1, 9):
        with pytest.raises(ValueError, match="samples_per_image"):
            eng.SCST_training_epoch([], opt, None, tqdm_visible=False, samples_per_image=n)
    for cls in (AoADetection_Eng, NIC_Eng):
        fake = cls.__new__(cls)                                     # the check runs before anything the constructor sets up
        with pytest.raises(ValueError, match="samples_per_image"):
            cls.SCST_training_epoch(fake, [], None, None, samples_per_image=4)
    # no output buffer was made (a zero fill would be the first device work of a call) and nothing was allocated
    assert torch.cuda.memory_allocated() == mem0 and h._bufs == bufs0


# ---- data parallelism --------------------------------------------------------------------------------------------------------
def _rank_rng(rows_all, lo, hi, seed, r, e, a, h):
    """rows [lo, hi) of the explicit arrays _rng(rows_all, seed, True) makes (what one rank's share of the B K rows draws)"""
    from simpleimagecaptionzoo_amd.butd import make_rng
    rs = np.random.RandomState(seed)
    em, am, om = rs.rand(T, rows_all, e) < 0.5, rs.rand(T, rows_all, r, a) < 0.5, rs.rand(T, rows_all, h) < 0.5
    u = rs.rand(T, rows_all).astype(np.float32)
    cut = lambda x: torch.tensor(np.ascontiguousarray(x[:, lo:hi]), device="cuda")
    return make_rng(0, cut(u), cut(em.astype(np.uint8)), cut(am.astype(np.uint8)), cut(om.astype(np.uint8)))


def dp_reference(golden_dir, K=4):
    """the parameters after two samples_per_image = K steps of one process on all six golden images"""
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    g, fx, batches, rngs = _steps(golden_dir, K)
    eng = _engine(g, fx)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    for b, r in zip(batches, rngs):
        eng.SCST_training_epoch([b], opt, None, tqdm_visible=False, rngs=[r()], samples_per_image=K)
    torch.cuda.synchronize()
    return _params(eng)


@pytest.mark.gpu_slow
def test_two_ranks_equal_one_process(golden_dir, tmp_path):
    want = dp_reference(golden_dir)
    ref_file = str(tmp_path / "one_process.npz")
    np.savez(ref_file, **want)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   ICZ_TEST_REF=ref_file)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "scst_multisample_dp_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        try:
            out, err = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, out, err))
    for r, (rc, out, err) in enumerate(outs):
        assert rc == 0 and ("rank %d ok" % r) in out, err[-3000:]
