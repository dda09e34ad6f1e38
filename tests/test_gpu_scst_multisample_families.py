"""Multi-sample SCST for the AoA and NIC families on the device (icz_aoa_sample_n, icz_nic_sample_n, multisample.sample_n,
Engine.SCST_multisample_training_epoch).  AoA: the rollout over B K rows that share B refiner passes against the float64 oracle on the
features repeated K times (tokens, log-probs, every gradient), early-out, Philox determinism, graph replay, argument errors.  NIC:
bitwise the sampled rollout on the features repeated K times.  Engine: the new method against the same steps built by hand.
Cases, inputs and the oracle rollout: tests/test_cpu_scst_multisample_families.py (which also shows that no oracle draw of a case sits at a
CDF edge, so an excused row here is the device's)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _aoa_refiner as ar
import test_cpu_scst_multisample_families as fam
from _fullwidth import _excuse_sampled

pytestmark = pytest.mark.gpu

EXCUSED = 2          # rows per case whose draw fell within 1e-6 of a CDF edge (the full-width rule; a sampled rollout has no greedy near-ties)
_CASES = {}


def case(name):
    """inputs, a reward per row and the float64 oracle rollout with its autograd graph (made once per case, shared, never changed)"""
    if name not in _CASES:
        c = fam.aoa_inputs(name)
        cfg, K = c["cfg"], c["K"]
        c["reward"] = np.random.RandomState(fam.aoa_cases()[name][2] + 4).randn(cfg[0] * K, 1).astype(np.float32).repeat(cfg[7], 1)
        c["oracle"] = fam.oracle_rollout(c, torch.float64, grad=True)
        _CASES[name] = c
    return _CASES[name]


def make_handle(c, train_refiner=False, options=None, max_rows=None):
    from simpleimagecaptionzoo_amd.aoa import AoaHandle
    B, R, D, Hd, E, V, NH = c["cfg"][:7]
    h = AoaHandle(R, D, Hd, E, V, NH, max_rows or B * c["K"], 24)
    h.bind({k: v.to("cuda").contiguous() for k, v in c["sd"].items()})
    if train_refiner:
        h.set_option("train_refiner", 1)
    for k, v in (options or {}).items():
        if k == "graphs":
            h.enable_graphs(bool(v))
        else:
            h.set_option(k, v)
    return h


def run(h, c, rng=None, reward=None, grads=None):
    """sample_n + sample_backward -> (seq, logprobs, loss, grads), copies (with graphs on the handle's outputs are persistent buffers)"""
    from simpleimagecaptionzoo_amd.multisample import sample_n
    seq, lp = sample_n(h, ar.batch_of(c["cfg"], c["feats"]), c["K"], c["cfg"][7], rng or ar.device_rng(c["masks"], c["u"]))
    seq, lp = seq.clone(), lp.clone()
    grads = h.new_grads() if grads is None else grads
    loss, _ = h.sample_backward(torch.tensor(c["reward"] if reward is None else reward, device="cuda"), grads)
    return seq, lp, loss.clone(), grads


def check_grads(grads, want, what):
    """the project's gradient tolerance (tests/test_gpu_aoa_refiner_train.py): 2e-4 of each tensor's maximum"""
    for k, v in grads.items():
        w = want[k]
        got = v.cpu().double().numpy()
        scale = max(1e-3, float(np.abs(w).max()))
        err = float(np.abs(got - w).max())
        print("%s %-55s max|want| %.3e  err/scale %.3e" % (what, k, float(np.abs(w).max()), err / scale))
        assert np.isfinite(got).all() and err <= 2e-4 * scale + 2e-6, (what, k, err, scale)


def against_oracle(name, train_refiner):
    from oracle import butd as ob
    c = case(name)
    cfg, K = c["cfg"], c["K"]
    rows, T = cfg[0] * K, cfg[7]
    p, w_seq, w_lp, w_logits = c["oracle"]
    h = make_handle(c, train_refiner)
    from simpleimagecaptionzoo_amd.multisample import sample_n
    seq, lp = sample_n(h, ar.batch_of(cfg, c["feats"]), K, T, ar.device_rng(c["masks"], c["u"]))
    assert seq.shape == (rows, T) and lp.shape == (rows, T)
    seq_h, lp_h = seq.cpu().numpy(), lp.cpu().numpy()
    same = _excuse_sampled(seq_h, w_seq, w_logits, c["u"], EXCUSED)       # token-exact up to EXCUSED draws at a CDF edge
    print("%s: %d of %d rows token-exact" % (name, int(same.sum()), rows))
    np.testing.assert_allclose(lp_h[same], w_lp.detach().numpy()[same], atol=1e-4)
    rw = c["reward"] * same[:, None].astype(np.float32)                   # excused rows leave the loss
    grads = h.new_grads()
    assert len(grads) == (82 if train_refiner else sum(k.startswith("decoder.") for k in c["sd"]))
    loss, _ = h.sample_backward(torch.tensor(rw, device="cuda"), grads)
    with ar.oracle_dtype(cfg[6], torch.float64):
        seq_m = torch.from_numpy(np.where(same[:, None], w_seq.numpy(), seq_h))
        w_loss = ob.reward_criterion(w_lp, seq_m, torch.from_numpy(rw).double())
        keys = list(grads)
        gs = torch.autograd.grad(w_loss, [p[k] for k in keys], retain_graph=True, allow_unused=True)
    print("%s: loss %.7f oracle %.7f" % (name, loss.item(), float(w_loss.detach())))
    assert abs(loss.item() - float(w_loss.detach())) < 1e-4
    want = {k: (g.numpy() if g is not None else np.zeros(tuple(p[k].shape))) for k, g in zip(keys, gs)}
    check_grads(grads, want, name)
    return h, c


@pytest.mark.parametrize("name", ["tiny_1x2", "tiny_3x5", "tiny_2x8", "packed", "w64", "chunk"])
def test_aoa_sample_n_matches_the_oracle_on_repeated_features(name):
    against_oracle(name, False)


@pytest.mark.parametrize("name", ["tiny_3x5", "packed"])
def test_aoa_sample_n_train_refiner_gradients_of_every_parameter(name):
    against_oracle(name, True)


def test_aoa_train_refiner_off_leaves_the_refiner_gradients_untouched():
    c = case("tiny_3x5")
    on = run(make_handle(c, True), c)
    full = {k: torch.full_like(v, 7.5, device="cuda") for k, v in c["sd"].items()}
    off = run(make_handle(c, False), c, grads=full)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
    for k, v in full.items():
        if k.startswith("decoder."):
            assert torch.equal(v, on[3][k]), k
        else:
            assert bool((v == 7.5).all()), k


def test_aoa_early_out_changes_no_bit():
    c = case("early")
    a = run(make_handle(c, True), c)
    b = run(make_handle(c, True, {"early_out": 0}), c)
    s = a[0].cpu().numpy()
    assert (s[:, 3:] == 0).all() and s[:, 2].any() and np.array_equal(s, c["oracle"][1].numpy())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def _equal_runs(a, b, what=""):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), what
    assert set(a[3]) == set(b[3])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), (what, k)


@pytest.mark.parametrize("train_refiner", [False, True])
def test_aoa_philox_runs_are_bit_equal_and_graph_replay_equals_eager(train_refiner):
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    c = case("tiny_3x5")
    h = make_handle(c, train_refiner)
    first = run(h, c, make_aoa_rng(4242))
    second = run(h, c, make_aoa_rng(4242))
    _equal_runs(first, second, "two eager runs")
    other = run(h, c, make_aoa_rng(4243))
    assert not torch.equal(first[0], other[0])
    assert all(bool(torch.isfinite(v).all()) for v in first[3].values()) and bool(first[3]["decoder.aoa_block.linear_V.weight"].any())
    g = make_handle(c, train_refiner, {"graphs": 1})
    feats = ar.batch_of(c["cfg"], c["feats"])
    reward = torch.tensor(c["reward"], device="cuda")
    from simpleimagecaptionzoo_amd.multisample import sample_n
    for i in range(3):        # the capture, then two replays
        seq, lp = sample_n(g, feats, c["K"], c["cfg"][7], make_aoa_rng(4242 + (i == 1)))
        grads = g.new_grads() if i == 0 else grads
        loss, _ = g.sample_backward(reward, grads)
        _equal_runs((seq, lp, loss, grads), other if i == 1 else first, "graphs, call %d" % i)


def test_aoa_graph_keys_tell_the_samples_per_image_apart():
    """One handle with graphs on: sample_n of 2 images x 4, sample of 8 rows, sample_n of 4 images x 2, then 2 x 4 again -- 8 decoder rows
    each, the same reward and output buffers -- against fresh eager handles: a graph replayed under a key without K would compute the
    other grouping."""
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    from simpleimagecaptionzoo_amd.multisample import sample_n
    c = case("tiny_2x8")
    cfg = c["cfg"]
    T = cfg[7]
    feats = ar.feats_of((8,) + cfg[1:], 991).cuda()
    reward = torch.tensor(np.random.RandomState(5).randn(8, 1).astype(np.float32).repeat(T, 1), device="cuda")
    ops = [("n", 2, 4, 71), ("s", 8, 1, 72), ("n", 4, 2, 73), ("n", 2, 4, 74), ("n", 4, 2, 75)]

    def play(h, op, grads):
        kind, B, K, seed = op
        if kind == "n":
            seq, lp = sample_n(h, feats[:B], K, T, make_aoa_rng(seed))
        else:
            seq, lp = h.sample(feats[:B], T, make_aoa_rng(seed))
        loss, _ = h.sample_backward(reward, grads)
        return seq.clone(), lp.clone(), loss.clone(), {k: v.clone() for k, v in grads.items()}

    g = make_handle(c, True, {"graphs": 1}, max_rows=8)
    grads = g.new_grads()
    for op in ops:
        got = play(g, op, grads)
        e = make_handle(c, True, max_rows=8)
        _equal_runs(got, play(e, op, e.new_grads()), str(op))
        e.close()


def test_aoa_errors_allocate_and_queue_nothing():
    from simpleimagecaptionzoo_amd._lib import IczError, lib, ptr, stream_ptr
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    from simpleimagecaptionzoo_amd.multisample import sample_n
    c = case("tiny_3x5")
    h = make_handle(c, max_rows=8)
    feats = c["feats"].cuda()
    seq = torch.zeros(9, 5, dtype=torch.int64, device="cuda")
    lp = torch.zeros(9, 5, device="cuda")
    rng = make_aoa_rng(1)
    torch.cuda.synchronize()
    mem0, bufs0 = torch.cuda.memory_allocated(), dict(h._bufs)
    for n in (1, 9, True, 2.5):
        with pytest.raises(IczError, match="samples per image"):
            sample_n(h, feats, n, 5)
    with pytest.raises(IczError, match="capacity"):
        sample_n(h, feats, 3, 5)                      # 9 rows > 8
    L = lib()
    assert L.icz_aoa_sample_n(h._h, ptr(feats), 3, 9, 5, C.byref(rng), ptr(seq), ptr(lp), stream_ptr()) == -1
    assert b"K=9" in L.icz_last_error()
    assert L.icz_aoa_sample_n(h._h, None, 3, 2, 5, C.byref(rng), ptr(seq), ptr(lp), stream_ptr()) == -1
    assert b"null argument" in L.icz_last_error()
    assert L.icz_aoa_sample_n(h._h, ptr(feats), 3, 3, 5, C.byref(rng), ptr(seq), ptr(lp), stream_ptr()) == -1
    assert b"exceed the row capacity 8" in L.icz_last_error()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem0 and h._bufs == bufs0 and not bool(seq.any()) and not bool(lp.any())
    with pytest.raises(IczError, match="no rollout stored"):          # nothing was stored either: there is no rollout to differentiate
        h.sample_backward(torch.zeros(9, 5, device="cuda"), h.new_grads())


# ---- NIC ----------------------------------------------------------------------------------------------------------------------
def _nic(golden_dir, name, max_rows):
    from simpleimagecaptionzoo_amd.nic import NicHandle
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    _, H, E, V = [int(x) for x in g["dims"]][:4]
    h = NicHandle(E, H, V, max_rows, 20)
    h.bind({k[3:]: torch.tensor(v, device="cuda") for k, v in g.items() if k.startswith("sd.")})
    return h, (H, E, V)


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("B,K", [(1, 2), (5, 3), (4, 8)])
@pytest.mark.parametrize("name", ["nic_dec_tiny", "nic_dec_odd"])
def test_nic_sample_n_is_sample_on_repeated_features_bit_for_bit(golden_dir, name, B, K, explicit):
    from simpleimagecaptionzoo_amd.butd import make_rng
    from simpleimagecaptionzoo_amd.multisample import sample_n
    T, rows = 7, B * K
    h, (H, E, V) = _nic(golden_dir, name, rows)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(B * 10 + K)
    feats = torch.randn(B, E, generator=gen).cuda()
    rs = np.random.RandomState(B + K)

    def rng():
        if not explicit:
            return make_rng(77)
        return make_rng(0, torch.tensor(rs_u, device="cuda"), None, None, torch.tensor(rs_m, device="cuda"))

    rs_u, rs_m = rs.rand(T, rows).astype(np.float32), (rs.rand(T, rows, H) < 0.5).astype(np.uint8)
    reward = torch.tensor(rs.randn(rows, 1).astype(np.float32).repeat(T, 1), device="cuda")
    seq_n, lp_n = sample_n(h, feats, K, T, rng())
    g_n = h.new_grads()
    loss_n, msum_n, df_n = h.sample_backward(reward, g_n, want_dfeats=True)
    seq_r, lp_r = h.sample(feats.repeat_interleave(K, 0), T, rng())
    g_r = h.new_grads()
    loss_r, msum_r, df_r = h.sample_backward(reward, g_r, want_dfeats=True)
    assert seq_n.shape == (rows, T) and torch.equal(seq_n, seq_r) and torch.equal(lp_n, lp_r)
    assert bool(seq_n[:, 0].any()) and torch.equal(loss_n, loss_r) and torch.equal(msum_n, msum_r)
    for k in g_r:
        assert torch.equal(g_n[k], g_r[k]) and bool(g_r[k].any()), k
    want = df_r.view(B, K, E)[:, 0].clone()
    for k in range(1, K):             # the fp32 sum in k order
        want = want + df_r.view(B, K, E)[:, k]
    assert df_n.shape == (B, E) and torch.equal(df_n, want) and bool(df_n.any())


def test_nic_errors_queue_nothing(golden_dir):
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.multisample import sample_n
    h, (H, E, V) = _nic(golden_dir, "nic_dec_tiny", 8)
    feats = torch.randn(3, E, device="cuda")
    torch.cuda.synchronize()
    mem0, bufs0 = torch.cuda.memory_allocated(), dict(h._bufs)
    for n in (1, 9):
        with pytest.raises(IczError, match="samples per image"):
            sample_n(h, feats, n, 5)
    with pytest.raises(IczError, match="capacity"):
        sample_n(h, feats, 3, 5)
    assert torch.cuda.memory_allocated() == mem0 and h._bufs == bufs0


# ---- Engine -------------------------------------------------------------------------------------------------------------------
def _by_hand(ref, opt, batches, rngs, K):
    """the multi-sample step built from its parts on the engine's own stream: multisample.sample_n, the host leave-one-out reward,
    sample_backward, clamp 0.25 + Adam"""
    from simpleimagecaptionzoo_amd.ciderd import loo_baseline_reward
    from simpleimagecaptionzoo_amd.multisample import sample_n
    with torch.cuda.stream(ref.stream):
        for (ids, _, gts, supp), r in zip(batches, rngs):
            ref.model.train()
            feats = ref._features(ref.modify_visual_inputs(None, supp))
            h = ref._hot_handle()
            seq, _ = sample_n(h, feats, K, 20, r())
            rep_ids = [i for i in ids for _ in range(K)]
            _, scores = ref.scorer().reward(seq, seq, gts, rep_ids, return_scores=True)
            s = scores.cpu().numpy()[:seq.shape[0]]
            rw = torch.tensor(np.repeat(loo_baseline_reward(s, K)[:, None], 20, 1), device="cuda")
            grads = ref._grads()
            h.sample_backward(rw, grads)
            ref._apply(opt, 0.25)
    torch.cuda.synchronize()


def _params(eng):
    return {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}


def _two_steps_both_ways(make_engine, batches, rngs, K):
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    eng = make_engine()
    start = _params(eng)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    for b, r in zip(batches, rngs):
        losses = eng.SCST_multisample_training_epoch([b], opt, None, tqdm_visible=False, rngs=[r()], samples_per_image=K)
        assert len(losses) == 1 and np.isfinite(losses[0].item())
    torch.cuda.synchronize()
    got = _params(eng)
    ref = make_engine()
    opt2 = init_optimizer("Adam", ref.model.get_param_groups({"lr": 2e-5}), 2e-5)
    _by_hand(ref, opt2, batches, rngs, K)
    want = _params(ref)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    return start, got


@pytest.mark.parametrize("train_refiner", [False, True])
def test_aoa_engine_steps_equal_the_steps_built_by_hand(golden_dir, train_refiner):
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng
    from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    from test_gpu_aoa import _supp
    B, R, D, Hd, E, V, NH = (4,) + fam._tiny_dims()
    cfg = (B, R, D, Hd, E, V, NH, 20, None, None)
    K = 5
    vocab = synthetic_vocab(V)
    words = [vocab.ix2word[i] for i in range(V)]
    gts = synthetic_references(B, words, seed=5)
    dfd = document_frequency(gts)
    sd0 = ar.state_dict_of(cfg, 300)
    settings = {"model_type": "AoADetection", "embed_dim": E, "hidden_dim": Hd, "num_heads": NH, "num_regions": R, "enc_dim": D}

    def engine():
        eng = AoADetection_Eng(dict(settings), "SYN", vocab, data_dir="/tmp/", use_bu="fixed", device="cuda:0", cider_df=dfd, max_batch=8,
                               train_refiner=train_refiner)
        eng.model.load_state_dict(sd0, strict=True)
        return eng

    batches = [(tuple(range(B)), None, gts, _supp(ar.feats_of(cfg, 320 + s).numpy())) for s in range(2)]
    rngs = [lambda s=s: make_aoa_rng(900 + s) for s in range(2)]
    start, got = _two_steps_both_ways(engine, batches, rngs, K)
    moved = [k for k in got if not torch.equal(got[k], start[k])]
    assert any(k.startswith("decoder.") for k in moved)
    assert any(not k.startswith("decoder.") for k in moved) == train_refiner


def test_nic_engine_steps_equal_the_steps_built_by_hand(golden_dir):
    from simpleimagecaptionzoo_amd.butd import make_rng
    from simpleimagecaptionzoo_amd.engine import NIC_Eng
    from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    g = dict(np.load(os.path.join(golden_dir, "nic_dec_tiny.npz")))
    B, H, E, V = [int(x) for x in g["dims"]]
    K = 5
    vocab = synthetic_vocab(V)
    words = [vocab.ix2word[i] for i in range(V)]
    gts = synthetic_references(B, words, seed=5)
    dfd = document_frequency(gts)
    sd0 = {"decoder." + k[3:]: torch.tensor(v) for k, v in g.items() if k.startswith("sd.")}

    def engine():
        eng = NIC_Eng({"model_type": "NIC", "embed_dim": E, "hidden_dim": H}, "SYN", vocab, data_dir="/tmp/", device="cuda:0", cider_df=dfd,
                      max_batch=8)
        eng.model.load_state_dict(sd0, strict=True)
        return eng

    feats = torch.tensor(g["feats"], device="cuda")
    batches = [(tuple(range(B)), None, gts, {"img_feats": feats * (1.0 + s)}) for s in range(2)]
    rngs = [lambda s=s: make_rng(800 + s) for s in range(2)]
    start, got = _two_steps_both_ways(engine, batches, rngs, K)
    assert all(not torch.equal(got[k], start[k]) for k in got)


def test_butd_engine_new_method_is_the_samples_per_image_step(golden_dir):
    import test_gpu_scst_multisample as tms
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    K = 4
    g, fx, batches, rngs = tms._steps(golden_dir, K)
    out = []
    for new in (False, True):
        eng = tms._engine(g, fx)
        opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
        for b, r in zip(batches, rngs):
            if new:
                eng.SCST_multisample_training_epoch([b], opt, None, tqdm_visible=False, rngs=[r()], samples_per_image=K)
            else:
                eng.SCST_training_epoch([b], opt, None, tqdm_visible=False, rngs=[r()], samples_per_image=K)
        torch.cuda.synchronize()
        out.append(_params(eng))
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
