"""SCST on without-replacement samples on the device (csrc/swor_objective.hip, simpleimagecaptionzoo_amd/swor.py,
Engine.SCST_distinct_training_epoch).  The three decoders' xe_backward_swor at their tiny golden dims with explicit dropout masks:
every gradient, the loss and the stats against autograd of the same loss over the float64 decoder oracles; against the kernels alone
followed by xe_backward_dlogits, bit for bit; at a doubled image count; run twice; and refused.  The Engine method against the same
steps built by hand, and two data-parallel ranks against one process.
Tolerances: a gradient tensor |got - want|max <= 2e-4 max(1e-3, |want|max) + 2e-6, a loss 1e-4."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _aoa_refiner as ar
import _swor_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
# family case -> (slots per image, estimator): B = 5 rows are one image of n = 6, B = 4 rows two images of n = 3
FAMILY_CASES = {"butd": (6, "normalised"), "nic": (6, "unbiased"), "aoa": (3, "normalised"), "aoa_refiner": (3, "unbiased")}
_CASES = {}


def close(got, want, what):
    """the project's gradient rule on one tensor (got: a device tensor, want: numpy float64)"""
    got = got.detach().cpu().double().numpy()
    scale = max(1e-3, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print("%-70s max|want| %.3e  err/scale %.3e" % (what, float(np.abs(want).max()), err / scale))
    assert np.isfinite(got).all() and err <= 2e-4 * scale + 2e-6, (what, err, scale)


def check_grads(grads, want, what):
    assert set(grads) == set(want)
    for k, v in grads.items():
        close(v, want[k], what + " " + k)


def _golden(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name + ".npz")))


def family_case(golden_dir, name):
    """inputs, a handle factory and the float64 oracle gradients of one family case (made once, shared, never changed): the golden's
    teacher-forced batch stands for the sorted sampled captions, with made-up phi, G, scores and a shuffled way back (perm)"""
    if name in _CASES:
        return _CASES[name]
    from oracle import butd as ob
    from oracle import nic as on
    from simpleimagecaptionzoo_amd.butd import make_rng
    from simpleimagecaptionzoo_amd.swor import SworBatch
    n, estimator = FAMILY_CASES[name]
    c = {"name": name, "n": n, "estimator": estimator}
    if name == "butd":
        from test_gpu_butd import _masks, make_handle, sd_of
        g = _golden(golden_dir, "butd_dec_tiny")
        B, R, D, H, E, A, V = [int(x) for x in g["dims"]]
        lengths, caps = g["xe_lengths"].tolist(), g["xe_captions"]
        with ar.oracle_dtype(8, torch.float64):
            p = {k: torch.tensor(np.asarray(v)).double().requires_grad_(True) for k, v in ob.strip_prefix(sd_of(g)).items()}
            att = np.unpackbits(g["xe_att_mask"], axis=-1)[..., :A]
            logits = ob.forward_xe(torch.from_numpy(g["feats"]).double(), torch.from_numpy(caps), lengths, p, g["xe_emb_mask"], att, g["xe_out_mask"])
        from simpleimagecaptionzoo_amd._lib import BUTD_PARAM_KEYS
        c["leaves"] = {k: p[k] for k in BUTD_PARAM_KEYS}
        c["make"] = lambda: make_handle(g)[0]
        feats = torch.tensor(g["feats"], device=DEV)
        c["forward"] = lambda h, logits=False, train=True: h.xe_forward(feats, torch.tensor(caps, device=DEV), lengths,
                                                                        make_rng(0, None, *_masks(g, "xe_", A)), train, logits)
    elif name == "nic":
        from test_gpu_nic import make
        g = _golden(golden_dir, "nic_dec_tiny")
        B, H, E, V = [int(x) for x in g["dims"]]
        lengths, caps = g["xe_lengths"].tolist(), g["xe_captions"]
        with ar.oracle_dtype(8, torch.float64):
            p = {k[3:]: torch.tensor(np.asarray(v)).double().requires_grad_(True) for k, v in g.items() if k.startswith("sd.")}
            f64 = torch.from_numpy(g["feats"]).double().requires_grad_(True)
            logits = on.forward_xe(f64, torch.from_numpy(caps), lengths, p, g["xe_out_mask"])
        c["leaves"] = dict(p)
        c["leaves"]["d features"] = f64
        c["make"] = lambda: make(g)
        feats = torch.tensor(g["feats"], device=DEV)
        c["forward"] = lambda h, logits=False, train=True: h.xe_forward(feats, torch.tensor(caps, device=DEV), lengths,
                                                                        make_rng(0, None, None, None, torch.tensor(g["xe_out_mask"], device=DEV)),
                                                                        train, logits)
    else:
        from simpleimagecaptionzoo_amd.aoa import AoaHandle
        from test_gpu_aoa import rng_of
        from test_oracle_golden import aoa_inputs, aoa_masks
        g = _golden(golden_dir, "aoa_tiny")
        refiner = "refiner" in name
        B, R, D, Hd, E, V, NH = [int(x) for x in g["dims"]]
        lengths, caps = g["xe_lengths"].tolist(), g["xe_captions"]
        feats, counts = aoa_inputs(g)
        assert counts is None
        sd = {k[3:]: torch.tensor(np.asarray(v)) for k, v in g.items() if k.startswith("sd.")}
        with ar.oracle_dtype(NH, torch.float64) as oa:
            p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
            logits = oa.forward_xe(feats.double(), torch.from_numpy(caps), lengths, p, aoa_masks(g, "xe_mask."), counts)
        c["leaves"] = {k: v for k, v in p.items() if refiner or k.startswith("decoder.")}

        def make():
            h = AoaHandle(R, D, Hd, E, V, NH, 16, 20)
            h.bind({k: v.to(DEV).contiguous() for k, v in sd.items()})
            if refiner:
                h.set_option("train_refiner", 1)
            return h
        c["make"] = make
        fd = feats.to(DEV)
        c["forward"] = lambda h, logits=False, train=True: h.xe_forward(fd, torch.tensor(caps, device=DEV), lengths, rng_of(g, "xe_mask."), train, logits)
    c["ss"] = (float(g["ss_prob"]), g["ss_gate"], g["ss_draw"].astype(np.float32))
    assert len(set(lengths)) > 1 and B % (n - 1) == 0                  # ragged: some (t, b) are inactive
    rs = np.random.RandomState(500 + list(FAMILY_CASES).index(name))
    n_img, m = B // (n - 1), n - 1
    total = n_img * n
    kept = [r for r in range(total) if r % n != m]
    perm = [kept[i] for i in rs.permutation(B)]
    rows_of_image = torch.empty(n_img, m, dtype=torch.int64)
    for b, r in enumerate(perm):
        rows_of_image[r // n, r % n] = b
    c["batch"] = SworBatch(torch.from_numpy(caps), lengths, torch.tensor(perm, dtype=torch.int32), rows_of_image)
    phi = (-rs.rand(total) * 15.0 - 0.1).astype(np.float32)
    G = np.sort(rs.rand(n_img, n) * 10.0 - 12.0, axis=1)[:, ::-1].reshape(-1).copy()
    scores = rs.rand(total) * 3.0
    c["phi"], c["G"], c["scores"] = phi, G, scores
    c["V"], c["B"], c["n_img"], c["order"] = V, B, n_img, ob.packed_order(lengths)
    coef, _, (stats, _) = so.coefs(phi, G, scores, n, estimator, float(n_img))
    lp = torch.log_softmax(logits, 1)
    loss = sum(float(coef[perm[b]]) * lp[k, int(caps[b, t + 1])] for k, (b, t) in enumerate(c["order"]))
    keys = list(c["leaves"])
    gs = torch.autograd.grad(loss, [c["leaves"][k] for k in keys], allow_unused=True)
    c["want"] = {k: (g_.numpy() if g_ is not None else np.zeros(tuple(c["leaves"][k].shape))) for k, g_ in zip(keys, gs)}
    c["loss"], c["stats"] = float(loss.detach()), stats
    by_img, lp = np.zeros(n_img), lp.detach().numpy()
    for k, (b, t) in enumerate(c["order"]):
        by_img[perm[b] // n] += float(coef[perm[b]]) * float(lp[k, int(caps[b, t + 1])])
    c["by_image"] = by_img
    _CASES[name] = c
    return c


def backward(c, h, **kw):
    """xe_backward_swor on the handle's stored forward with the case's inputs -> (loss buffer (1 + images,), stats, gradients by the
    oracle's names)"""
    from simpleimagecaptionzoo_amd.swor import xe_backward_swor
    opts = dict(estimator=c["estimator"])
    opts.update(kw)
    grads = h.new_grads()
    nic = h.family == "nic"
    res = xe_backward_swor(h, grads, *(torch.from_numpy(c[k]) for k in ("phi", "G", "scores")), c["batch"], want_dfeats=nic, **opts)
    out = dict(grads)
    if nic:
        out["d features"] = res[2]
    (loss, by_image), stats = res[:2]
    return torch.cat([loss, by_image]).clone(), stats.clone(), out


@pytest.mark.parametrize("name", list(FAMILY_CASES))
def test_handle_against_the_oracle_and_the_kernels_alone_route(golden_dir, name):
    from simpleimagecaptionzoo_amd.distill import xe_backward_dlogits
    from simpleimagecaptionzoo_amd.swor import swor_loss
    c = family_case(golden_dir, name)
    h = c["make"]()
    c["forward"](h)
    l, stats, grads = backward(c, h)
    print("loss %r  oracle %r" % (l.tolist(), [c["loss"]] + c["by_image"].tolist()))
    np.testing.assert_allclose(l.cpu().double().numpy(), np.array([c["loss"]] + c["by_image"].tolist()), rtol=0, atol=1e-4)
    np.testing.assert_allclose(stats.cpu().numpy(), c["stats"], rtol=1e-9, atol=0)
    check_grads(grads, c["want"], name)
    assert any(bool(v.any()) for v in grads.values())
    # the same step as: packed logits -> the kernels alone -> the backward pass for an upstream gradient, bit for bit
    V, B, T = c["V"], c["B"], max(c["batch"].lengths)
    packed = c["forward"](h, True)
    x = torch.full((T * B, (V + 63) & ~63), float("nan"), device=DEV)
    rows = torch.tensor([t * B + b for b, t in c["order"]], device=DEV)
    x[rows, :V] = packed
    _, _, l2, stats2 = swor_loss(x, V, c["batch"], *(torch.from_numpy(c[k]) for k in ("phi", "G", "scores")), c["estimator"])
    via = h.new_grads()
    dfe = xe_backward_dlogits(h, x[rows, :V].contiguous(), via, want_dfeats=h.family == "nic")
    if dfe is not None:
        via["d features"] = dfe
    assert torch.equal(l, l2) and torch.equal(stats, stats2)
    for k, v in grads.items():
        assert torch.equal(v, via[k]), k


@pytest.mark.parametrize("name", list(FAMILY_CASES))
def test_handle_doubled_image_count_two_runs_and_refusals(golden_dir, name):
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.swor import SworBatch, xe_backward_swor
    c = family_case(golden_dir, name)
    h = c["make"]()
    tensors = [torch.from_numpy(c[k]) for k in ("phi", "G", "scores")]
    with pytest.raises(IczError, match="no XE forward stored"):
        xe_backward_swor(h, h.new_grads(), *tensors, c["batch"])
    # two runs: the same bits; N = 2 N_local: exactly half of the loss and of every gradient
    c["forward"](h)
    l_one, s_one, g_one = backward(c, h)
    c["forward"](h)
    l_again, s_again, g_again = backward(c, h)
    assert torch.equal(l_again, l_one) and torch.equal(s_again, s_one) and all(torch.equal(g_again[k], v) for k, v in g_one.items())
    c["forward"](h)
    l_two, s_two, g_two = backward(c, h, n_img_global=2.0 * c["n_img"])
    assert torch.equal(l_two * 2, l_one) and torch.equal(s_two, s_one)
    for k, v in g_one.items():
        assert torch.equal(g_two[k] * 2, v), k
    assert any(bool(v.any()) for v in g_one.values())
    # refusals: nothing is queued (the gradient buffers keep their fill) and the stored forward stays usable
    full = {k: torch.full_like(v, 7.5) for k, v in h.new_grads().items()}

    def refused(match, batch=c["batch"], exc=IczError, **kw):
        with pytest.raises(exc, match=match):
            xe_backward_swor(h, full, *tensors, batch, **kw)
        torch.cuda.synchronize()
        assert all(bool((v == 7.5).all()) for v in full.values())
    c["forward"](h)
    refused("estimator", exc=ValueError, estimator="mean")
    refused("n_img_global", exc=ValueError, n_img_global=-1.0)
    b = c["batch"]
    if c["B"] == 5:                    # four rows (two images of n = 3) against the stored five
        short = SworBatch(b.captions[:4], b.lengths[:4], torch.tensor([0, 1, 3, 4], dtype=torch.int32), torch.tensor([[0, 1], [2, 3]]))
        with pytest.raises(IczError, match="4 sample rows, the stored forward pass has 5"):
            xe_backward_swor(h, full, *(t[:6] for t in tensors), short)
    twice = SworBatch(b.captions, b.lengths, torch.cat([b.perm[:1], b.perm[:-1]]), b.rows_of_image)
    refused("taken twice", batch=twice)
    assert np.isfinite(h.xe_backward(h.new_grads(), 0.1).item())       # the stored forward is still there
    c["forward"](h, train=False)
    refused("evaluation mode")
    h.set_scheduled_sampling(*c["ss"])
    c["forward"](h)
    refused("scheduled sampling")
    assert np.isfinite(h.xe_backward(h.new_grads(), 0.1).item())
    h.set_scheduled_sampling(0.0)
    c["forward"](h)
    l_last, _, g_last = backward(c, h)
    assert torch.equal(l_last, l_one) and all(torch.equal(g_last[k], v) for k, v in g_one.items())


# ---- the Engines -------------------------------------------------------------------------------------------------------------------
def _params(eng):
    return {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}


def _by_hand(ref, opt, batches, rngs, n, estimator):
    """the step from its parts on the engine's own stream"""
    from simpleimagecaptionzoo_amd.stochastic_beam import sample_distinct
    from simpleimagecaptionzoo_amd.swor import make_batch, swor_forward, xe_backward_swor
    out = []
    sta = ref.caption_vocab.word2ix["<sta>"]
    with torch.cuda.stream(ref.stream):
        for (ids, _, gts, supp), r in zip(batches, rngs):
            ref.model.train()
            feats = ref._features(ref.modify_visual_inputs(None, supp))
            h = ref.model._handle()
            s_rng, f_rng = r()
            cap, lens, _, phi, G = sample_distinct(h, feats, n, 20, 1.0, s_rng)
            _, scores = ref.scorer().reward_loo(cap, n, gts, ids, return_scores=True)
            batch = make_batch(cap, lens, sta, n)
            swor_forward(h, feats, batch, f_rng)
            (loss, _), stats = xe_backward_swor(h, ref._grads(), phi, G, scores, batch, estimator)
            out.append((loss.clone(), stats.clone()))
            ref._apply(opt, 0.25)
    torch.cuda.synchronize()
    return out


def _engine_against_hand(make_engine, batches, rngs, n, estimator):
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    eng = make_engine()
    start = _params(eng)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    losses, stats = [], []
    for bt, r in zip(batches, rngs):
        losses += eng.SCST_distinct_training_epoch([bt], opt, None, tqdm_visible=False, rngs=[r()], samples_per_image=n, estimator=estimator)
        stats += eng.last_swor_stats
    torch.cuda.synchronize()
    got = _params(eng)
    ref = make_engine()
    hand = _by_hand(ref, init_optimizer("Adam", ref.model.get_param_groups({"lr": 2e-5}), 2e-5), batches, rngs, n, estimator)
    want = _params(ref)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert any(not torch.equal(got[k], start[k]) for k in got)              # the steps moved the model
    assert len(losses) == len(hand) == len(stats) == 2
    for l, s, (hl, hs) in zip(losses, stats, hand):
        assert torch.equal(l, hl) and torch.equal(s, hs) and np.isfinite(l.item())
        ess = s[:, 2].cpu().numpy()
        assert s.shape == (len(batches[0][0]), 3) and (ess >= 1 - 1e-9).all() and (ess <= n - 1 + 1e-9).all()


def test_butd_engine_steps_equal_the_steps_built_by_hand(golden_dir):
    import test_gpu_scst_multisample as tms
    from simpleimagecaptionzoo_amd.butd import make_rng
    g, fx, batches, _ = tms._steps(golden_dir, 1)
    rngs = [lambda s=s: (70 + s, make_rng(40 + s)) for s in range(2)]
    _engine_against_hand(lambda: tms._engine(g, fx), batches, rngs, 5, "normalised")


def test_aoa_engine_steps_equal_the_steps_built_by_hand(golden_dir):
    import test_cpu_scst_multisample_families as fam
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng
    from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
    from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
    from test_gpu_aoa import _supp
    B, R, D, Hd, E, V, NH = (4,) + fam._tiny_dims()
    cfg = (B, R, D, Hd, E, V, NH, 20, None, None)
    vocab = synthetic_vocab(V)
    words = [vocab.ix2word[i] for i in range(V)]
    gts = synthetic_references(B, words, seed=5)
    dfd = document_frequency(gts)
    sd0 = ar.state_dict_of(cfg, 300)
    settings = {"model_type": "AoADetection", "embed_dim": E, "hidden_dim": Hd, "num_heads": NH, "num_regions": R, "enc_dim": D}

    def engine():
        eng = AoADetection_Eng(dict(settings), "SYN", vocab, data_dir="/tmp/", use_bu="fixed", device="cuda:0", cider_df=dfd, max_batch=8)
        eng.model.load_state_dict(sd0, strict=True)
        return eng

    batches = [(tuple(range(B)), None, gts, _supp(ar.feats_of(cfg, 320 + s).numpy())) for s in range(2)]
    rngs = [lambda s=s: ((80 + s, 0), make_aoa_rng(900 + s)) for s in range(2)]
    _engine_against_hand(engine, batches, rngs, 4, "unbiased")


# ---- data parallelism ----------------------------------------------------------------------------------------------------------------
DP_N = 4


def dp_rng(rows, seed, first_image, g):
    """(sample_distinct's rng, the forward's rng) of a data-parallel step: the batch's noise from image `first_image` on, and dropout
    masks that are the same for every row, so that a rank's rows -- sorted among themselves -- see what they see in one process"""
    from simpleimagecaptionzoo_amd.butd import make_rng
    B, R, D, H, E, A, V = [int(x) for x in g["dims"]]
    rs = np.random.RandomState(seed)
    row = lambda *s: torch.tensor(np.repeat((rs.rand(20, 1, *s) < 0.5).astype(np.uint8), rows, 1), device=DEV)
    return (seed, first_image), make_rng(0, None, row(E), row(R, A), row(H))


def dp_reference(golden_dir):
    """the parameters after two steps of one process on all six golden images"""
    import test_gpu_scst_multisample as tms
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    g, fx, batches, _ = tms._steps(golden_dir, 1)
    eng = tms._engine(g, fx)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    for s, b in enumerate(batches):
        eng.SCST_distinct_training_epoch([b], opt, None, tqdm_visible=False, rngs=[dp_rng(len(b[0]) * (DP_N - 1), 60 + s, 0, g)],
                                         samples_per_image=DP_N)
    torch.cuda.synchronize()
    return {k: v.numpy() for k, v in _params(eng).items()}


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
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ICZ_TEST_REF=ref_file)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "swor_dp_worker.py")], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
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
