"""Option "train_refiner" of the AoA handle (csrc/aoa_refine_train.hip): gradients of img_feats_porjection.* and aoa_refine.*
behind the decoder's BPTT, against torch autograd over the float64 oracle with every parameter requiring a gradient."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _aoa_refiner as ar

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("a", "b", "c", "d", "e")
# shift invariance of a softmax row: the reference's gradient of every linear_K.bias is rounding noise around zero
ZERO_GRAD = lambda k: k.endswith("linear_K.bias")


@pytest.fixture(scope="module")
def shapes(golden_dir):
    g = np.load(os.path.join(golden_dir, "aoa_tiny.npz"))
    B, R, D, Hd, E, V, NH = [int(x) for x in g["dims"]]
    out = dict(ar.SHAPES)
    out["a"] = (B, R, D, Hd, E, V, NH, 5, None, None)      # the tiny golden's own dims
    return out


_ORACLE = {}


def setup_case(shapes, name, mode):
    """The case's parameters, inputs and float64 oracle gradients (computed once per (case, mode) and shared, never changed)."""
    key = (name, mode)
    if key not in _ORACLE:
        cfg = shapes[name]
        B, T = cfg[0], cfg[7]
        seed = 100 + CASES.index(name)
        sd = ar.state_dict_of(cfg, seed)
        feats = ar.feats_of(cfg, seed + 1)
        masks, u = ar.masks_of(cfg, seed + 2)
        c = {"cfg": cfg, "sd": sd, "feats": feats, "masks": masks, "u": u}
        if mode == "xe":
            c["lengths"] = sorted([max(1, T - d) for d in (0, 2, 3, 4, 4, 4)][:B], reverse=True)      # ragged: e.g. [5, 3, 2]
            c["caps"] = ar.captions_of(cfg, c["lengths"], seed + 3)
            c["loss"], c["grads"] = ar.oracle_xe(cfg, sd, feats, c["caps"], c["lengths"], masks)
        else:
            c["reward"] = np.random.RandomState(seed + 4).randn(B, 1).astype(np.float32).repeat(T, 1)
            c["seq"], c["lp"], c["loss"], c["grads"] = ar.oracle_rl(cfg, sd, feats, masks, u, c["reward"], T)
        _ORACLE[key] = c
    return _ORACLE[key]


def make_handle(c, train_refiner=True, max_rows=8, sd=None):
    from simpleimagecaptionzoo_amd.aoa import AoaHandle
    B, R, D, Hd, E, V, NH = c["cfg"][:7]
    h = AoaHandle(R, D, Hd, E, V, NH, max_rows, 20)
    h.bind({k: v.to("cuda").contiguous() for k, v in (sd or c["sd"]).items()})
    if train_refiner:
        h.set_option("train_refiner", 1)
    return h


def run_xe(h, c):
    h.xe_forward(ar.batch_of(c["cfg"], c["feats"]), c["caps"].cuda(), c["lengths"], ar.device_rng(c["masks"]), True)
    grads = h.new_grads()
    loss = h.xe_backward(grads, 0.1)
    return loss, grads


def run_rl(h, c, rng=None, T=None):
    seq, lp = h.sample(ar.batch_of(c["cfg"], c["feats"]), T or c["cfg"][7], rng or ar.device_rng(c["masks"], c["u"]))
    grads = h.new_grads()
    loss, _ = h.sample_backward(torch.tensor(c["reward"], device="cuda"), grads)
    return seq, lp, loss, grads


def check_against_oracle(grads, want, what):
    """The project's gradient tolerance (tests/test_gpu_aoa.py: check_grads): 2e-4 of each tensor's maximum."""
    assert set(grads) == set(want)
    for k, v in grads.items():
        w = want[k]
        got = v.cpu().double().numpy()
        scale = max(1e-3, float(np.abs(w).max()))
        err = float(np.abs(got - w).max())
        print("%s %-55s max|want| %.3e  err/scale %.3e" % (what, k, float(np.abs(w).max()), err / scale))
        assert err <= 2e-4 * scale + 2e-6, (what, k, err, scale)


@pytest.mark.parametrize("name", CASES)
def test_xe_gradients_of_every_parameter(shapes, name):
    c = setup_case(shapes, name, "xe")
    h = make_handle(c)
    loss, grads = run_xe(h, c)
    assert abs(loss.item() - c["loss"]) < 1e-4
    assert len(grads) == 82
    check_against_oracle(grads, c["grads"], "xe/" + name)


@pytest.mark.parametrize("name", CASES)
def test_scst_gradients_of_every_parameter(shapes, name):
    c = setup_case(shapes, name, "rl")
    h = make_handle(c)
    seq, lp, loss, grads = run_rl(h, c)
    assert np.array_equal(seq.cpu().numpy(), c["seq"])
    if name == "e":         # the <end> bias: every row has finished by step 3, the steps behind never ran
        assert (c["seq"][:, 3:] == 0).all() and c["seq"][:, 0].any()
    np.testing.assert_allclose(lp.cpu().numpy(), c["lp"], atol=1e-4)
    assert abs(loss.item() - c["loss"]) < 1e-4
    check_against_oracle(grads, c["grads"], "rl/" + name)


@pytest.mark.parametrize("mode", ["xe", "rl"])
def test_the_option_changes_nothing_else(shapes, mode):
    """Decoder gradients, loss, seq and log-probs with the option on equal those with it off bit for bit; with it off the refiner's
    gradient slots may be null, and buffers passed there stay untouched."""
    c = setup_case(shapes, "b", mode)
    run = run_xe if mode == "xe" else run_rl
    off, on = run(make_handle(c, False), c), run(make_handle(c, True), c)
    assert set(off[-1]) == {k for k in c["sd"] if k.startswith("decoder.")} and len(on[-1]) == 82
    for a, b in zip(off[:-1], on[:-1]):
        assert torch.equal(a, b)
    for k, v in off[-1].items():
        assert torch.equal(v, on[-1][k]), k
    h = make_handle(c, False)
    full = {k: torch.full_like(v, 7.5, device="cuda") for k, v in c["sd"].items()}
    if mode == "xe":
        h.xe_forward(ar.batch_of(c["cfg"], c["feats"]), c["caps"].cuda(), c["lengths"], ar.device_rng(c["masks"]), True)
        h.xe_backward(full, 0.1)
    else:
        h.sample(ar.batch_of(c["cfg"], c["feats"]), c["cfg"][7], ar.device_rng(c["masks"], c["u"]))
        h.sample_backward(torch.tensor(c["reward"], device="cuda"), full)
    for k, v in full.items():
        if k.startswith("decoder."):
            assert torch.equal(v, off[-1][k]), k
        else:
            assert bool((v == 7.5).all()), k


def test_null_refiner_slot_is_an_error_before_any_launch(shapes):
    from simpleimagecaptionzoo_amd._lib import IczError
    c = setup_case(shapes, "c", "xe")
    h = make_handle(c)
    h.xe_forward(ar.batch_of(c["cfg"], c["feats"]), c["caps"].cuda(), c["lengths"], ar.device_rng(c["masks"]), True)
    grads = h.new_grads()
    h._frozen_keys = type(h)._frozen_keys           # the host side leaves the refiner's slots null again
    dec = {k: v for k, v in grads.items() if k.startswith("decoder.")}
    with pytest.raises(IczError, match="train_refiner is on and the gradient buffer of img_feats_porjection.0.weight is null"):
        h.xe_backward(dec, 0.1)
    assert all(not bool(v.any()) for v in dec.values())
    with pytest.raises(IczError, match="unknown option 'train_refine'"):
        h.set_option("train_refine", 1)


def _equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_two_runs_and_philox_against_explicit_masks_are_bit_equal(shapes):
    """Same inputs, same bits: explicit masks twice on one handle, Philox on two handles."""
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    c = setup_case(shapes, "b", "rl")
    h = make_handle(c)
    first = run_rl(h, c)
    second = run_rl(h, c)
    assert torch.equal(first[0], second[0])
    _equal(first[-1], second[-1])
    p1 = run_rl(h, c, make_aoa_rng(4242))
    p2 = run_rl(make_handle(c), c, make_aoa_rng(4242))
    assert torch.equal(p1[0], p2[0]) and torch.equal(p1[1], p2[1])
    _equal(p1[-1], p2[-1])
    assert all(bool(torch.isfinite(v).all()) for v in p1[-1].values())
    assert bool(p1[-1]["img_feats_porjection.0.weight"].any()) and bool(p1[-1]["aoa_refine.aoa_layers.0.aoa_block.linear_V.weight"].any())


def test_philox_masks_equal_the_same_masks_passed_explicitly(shapes):
    """The Philox keep bits (csrc/rng.h, DropP) restated on the host (tests/_aoa_refiner.py): a Philox run must equal bit for bit the
    run that is handed these bits as explicit masks, at every dropout site of the refiner and the attention block."""
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    c = setup_case(shapes, "c", "xe")
    B, R, D, Hd, E, V, NH = c["cfg"][:7]
    T = max(c["lengths"])
    seed = 0x1234ABCD5
    sites = {"proj": (10, 0.5, (1, B, R, Hd)), "ref_att": (11, 0.1, (6, B, NH, R, R)), "ref_aoa": (12, 0.3, (6, B, R, 2 * Hd)),
             "ref_sc": (13, 0.1, (6, B, R, Hd)), "ctx": (20, 0.5, (T, B, Hd)), "att": (21, 0.1, (T, B, NH, R)), "out": (22, 0.5, (T, B, Hd))}
    masks = {k: np.stack([ar.keep_bits(seed, stream, s, int(np.prod(shape[1:])), p).reshape(shape[1:]) for s in range(shape[0])])
             for k, (stream, p, shape) in sites.items()}
    masks["proj"] = masks["proj"][0]
    assert 0.85 < masks["ref_sc"].mean() < 0.95 and 0.4 < masks["proj"].mean() < 0.6
    explicit = {k: torch.tensor(v.astype(np.uint8), device="cuda") for k, v in masks.items()}      # (the embedding keeps its Philox stream)
    h = make_handle(c)
    feats, caps = ar.batch_of(c["cfg"], c["feats"]), c["caps"].cuda()
    h.xe_forward(feats, caps, c["lengths"], make_aoa_rng(seed), True)
    g1 = h.new_grads()
    l1 = h.xe_backward(g1, 0.1)
    h.xe_forward(feats, caps, c["lengths"], make_aoa_rng(seed, None, explicit), True)
    g2 = h.new_grads()
    l2 = h.xe_backward(g2, 0.1)
    assert torch.equal(l1, l2)
    _equal(g1, g2)


def _scst_step(h, feats, T, reward, n=1):
    """n SCST steps through scst_rollouts on one handle (under graphs the first call captures, the others replay)."""
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    grads = h.new_grads()
    for _ in range(n):
        ids, seq, lp = h.rollouts(feats, T, make_aoa_rng(77))
        loss, _ = h.sample_backward(reward, grads)
    return ids.clone(), seq.clone(), lp.clone(), loss.clone(), grads


def _same_step(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    _equal(a[4], b[4])


def test_graph_replay_equals_eager_launches(shapes):
    """The refiner's backward pass is captured with the backward graph (the option, the stored layer inputs and the feature pointer are
    in its key): capture + two replays against eager launches, bit for bit."""
    c = setup_case(shapes, "b", "rl")
    feats, T = ar.batch_of(c["cfg"], c["feats"]), c["cfg"][7]
    reward = torch.tensor(c["reward"], device="cuda")
    eager = _scst_step(make_handle(c), feats, T, reward)
    hg = make_handle(c)
    hg.enable_graphs(True)
    _same_step(eager, _scst_step(hg, feats, T, reward, 3))
    assert bool(eager[4]["aoa_refine.norm.gain"].any()) and bool(eager[4]["img_feats_porjection.0.bias"].any())


def test_refine_pair_on_and_off_are_bit_equal_at_the_baseline_batch():
    """Through scst_rollouts at the BASELINE batch (64 images, full width), where every GEMM of the paired refiner pass takes the
    split-K decomposition of the single passes and so both leave the same bits (tests/test_gpu_aoa_handle.py): the layer inputs copied
    out of the pair's training half give the refiner gradients of a pass of its own, bit for bit -- every one of the 82 tensors."""
    from _fullwidth import D, E, H, V
    from simpleimagecaptionzoo_amd.aoa import AoADetection_Captioner
    B, T = 64, 20
    torch.manual_seed(11)
    cap = AoADetection_Captioner(vocab_size=V, num_heads=8, hidden_dim=H, embed_dim=E, device="cuda:0", num_regions=36, enc_dim=D, max_batch=B)
    cap.to("cuda:0")
    cap.train_refiner = True
    feats = torch.relu(torch.randn(B, 36, D, device="cuda"))
    reward = torch.linspace(-1, 1, B, device="cuda").unsqueeze(1).repeat(1, T).contiguous()
    out = []
    for pair in (0, 1):
        h = cap._handle()
        h.set_option("refine_pair", pair)
        out.append(_scst_step(h, feats, T, reward))
    assert len(out[0][4]) == 82
    _same_step(out[0], out[1])
    assert all(bool(torch.isfinite(v).all()) for v in out[1][4].values())
    assert bool(out[1][4]["aoa_refine.aoa_layers.0.aoa_block.linear_Q.weight"].any())


def test_regrown_training_buffers_still_give_the_right_gradients(shapes):
    """A larger batch (and more steps) between two steps re-allocates every training buffer, the stored layer inputs included; the
    small step behind it must still match the oracle."""
    c = setup_case(shapes, "c", "xe")
    h = make_handle(c, max_rows=8)
    _, first = run_xe(h, c)
    cfg = c["cfg"]
    big_B, big_T = 7, 9
    masks, u = ar.masks_of(cfg, 5, big_B, big_T)
    seq, _ = h.sample(ar.feats_of(cfg, 6, big_B).cuda(), big_T, ar.device_rng(masks, u))
    h.sample_backward(torch.ones(seq.shape, device="cuda"), h.new_grads())
    _, again = run_xe(h, c)
    _equal(first, again)
    check_against_oracle(again, c["grads"], "regrown")


def test_engine_steps_match_autograd_clamp_and_adam(shapes, golden_dir):
    """Two XE and two SCST steps of AoADetection_Eng(train_refiner=True) at the tiny golden's dims against the same steps done by
    hand: autograd over the oracle (every parameter), the clamps of the Engine (0.1 / 0.25) and torch.optim.Adam.  Tolerance:
    tests/test_gpu_engine.py's for the decoder (5e-6 per step at these learning rates; the zero-gradient linear_K biases move by
    Adam's rounding noise, at most lr per step, as decoder.aoa_block.linear_K.bias does in tests/test_gpu_aoa.py).  With the default
    engine the refiner and the projection stay bit-unchanged."""
    from oracle import butd as ob
    from oracle import ciderd as oc
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, init_optimizer
    from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    from test_gpu_aoa import _Crit, _supp
    cfg = shapes["a"]
    B, R, D, Hd, E, V, NH = cfg[:7]
    vocab = synthetic_vocab(V)
    words = [vocab.ix2word[i] for i in range(V)]
    gts = synthetic_references(B, words, seed=5)
    dfd = document_frequency(gts)
    sd0 = ar.state_dict_of(cfg, 300)
    settings = {"model_type": "AoADetection", "embed_dim": E, "hidden_dim": Hd, "num_heads": NH, "num_regions": R, "enc_dim": D}

    def engine(**kw):
        eng = AoADetection_Eng(dict(settings), "SYN", vocab, data_dir="/tmp/", use_bu="fixed", device="cuda:0", cider_df=dfd, max_batch=8, **kw)
        eng.model.load_state_dict(sd0, strict=True)
        return eng

    lengths = sorted([5, 4, 4, 3, 2, 2, 1, 1][:B], reverse=True)
    steps = []
    for s in range(4):
        masks, u = ar.masks_of(cfg, 310 + s, B, 20 if s >= 2 else max(lengths))
        steps.append((ar.feats_of(cfg, 320 + s), ar.captions_of(cfg, lengths, 330 + s), masks, u))

    def run(eng):
        lr = 4e-4
        opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": lr}), lr)
        for feats, caps, masks, u in steps[:2]:
            batch = (tuple(range(B)), None, caps, [n + 1 for n in lengths], _supp(feats.numpy()))
            eng.training_epoch([batch], opt, _Crit(), tqdm_visible=False, rngs=[ar.device_rng(masks)])
        opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
        for feats, caps, masks, u in steps[2:]:
            eng.SCST_training_epoch([(tuple(range(B)), None, gts, _supp(feats.numpy()))], opt, None, tqdm_visible=False,
                                    rngs=[ar.device_rng(masks, u)])
        torch.cuda.synchronize()
        return {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}

    got = run(engine(train_refiner=True))
    # ---- by hand, in fp32 (the arithmetic of the reference)
    p = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}

    def hand(opt, clip, loss):
        opt.zero_grad()
        loss.backward()
        for v in p.values():
            v.grad.clamp_(-clip, clip)
        opt.step()

    with ar.oracle_dtype(NH, torch.float32) as oa:
        opt = torch.optim.Adam(list(p.values()), lr=4e-4)
        for feats, caps, masks, u in steps[:2]:
            logits = oa.forward_xe(feats, caps, lengths, p, masks)
            tgt = torch.tensor([caps[b, t + 1] for b, t in ob.packed_order(lengths)])
            hand(opt, 0.1, ob.label_smoothing_loss(logits, tgt, 0.1))
        opt = torch.optim.Adam(list(p.values()), lr=2e-5)
        for feats, caps, masks, u in steps[2:]:
            with torch.no_grad():
                greedy, _ = oa.greedy(feats, p, 20)
            seq, lp = oa.sample_rl(feats, p, u.astype(np.float64), masks, 20)
            reward = oc.self_critical_reward(seq.numpy(), greedy.numpy(), {i: gts[i] for i in range(B)}, list(range(B)), dict(enumerate(words)),
                                             oc.DocFreq(dfd["document_frequency"], dfd["ref_len"]))
            hand(opt, 0.25, ob.reward_criterion(lp, seq, torch.from_numpy(reward)))
    moved = 0
    for k, v in got.items():
        tol = 2 * (4e-4 + 2e-5) * 1.01 if ZERO_GRAD(k) else 4 * 5e-6
        np.testing.assert_allclose(v.numpy(), p[k].detach().numpy(), atol=tol, rtol=0, err_msg=k)
        moved += int(not k.startswith("decoder.") and not torch.equal(v, sd0[k]))
    assert moved == 64
    plain = run(engine())
    for k, v in plain.items():
        assert k.startswith("decoder.") or torch.equal(v, sd0[k]), k


def test_two_ranks_reproduce_one_process():
    """tests/aoa_refiner_dp_worker.py: two data-parallel ranks on this GPU, each with its share of the batch, end with the
    parameters (the refiner's and the projection's too) of one process on the whole batch."""
    import socket
    with socket.socket() as sk:          # a free rendezvous port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", LOCAL_RANK="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "aoa_refiner_dp_worker.py")], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "rank %d ok" % r in out, out[-3000:]
