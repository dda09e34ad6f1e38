"""The SCST objectives behind the three decoders (icz_*_sample_backward_objective, scst_objective.sample_backward_objective,
Engine.SCST_objective_training_epoch(objective=..., entropy_weight=...)): every parameter gradient against autograd of the same loss
over the float64 decoder oracles, the bit-for-bit equalities (kind 0 without entropy = sample_backward, two runs, graph replay =
eager, early-out = every step run), the n_img_global scaling, refusals that queue nothing, and the Engine's steps against the same
steps built by hand, on one process and on two ranks.

The oracle side is the oracle's own sampled rollout on the same uniforms and keep-masks (the device's tokens must be its tokens),
kept with the logits of every step in the autograd graph: the entropy term needs the whole distribution.  Tolerances are those of
tests/test_gpu_butd.py / test_gpu_nic.py / test_gpu_scst_multisample_families.py for the same gradients and the loss."""
import contextlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _aoa_refiner as ar
import test_cpu_scst_multisample_families as fam

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
END_BIAS = 4.0           # the <end> bias of the cases: some rows end within the 6 - 8 steps, some do not


@contextlib.contextmanager
def f64():
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(torch.float32)


def oracle_rollout(step, rows, T, u):
    """the reference's sample_rl loop (oracle/butd.py: sample_rl) over a step closure, every step's logits kept in the graph"""
    from oracle.butd import END, STA, inverse_cdf_draw
    it = torch.full((rows,), STA, dtype=torch.long)
    seq = torch.zeros(rows, T, dtype=torch.long)
    lps, lgs = [], []
    unfinished = torch.ones(rows, dtype=torch.bool)
    for t in range(T):
        logits = step(t, it)
        logp = torch.log_softmax(logits, dim=1)
        draw = inverse_cdf_draw(torch.exp(logp.detach()), u[t])
        lps.append(logp.gather(1, draw.unsqueeze(1)).squeeze(1))
        unfinished = unfinished & (draw != END)
        it = draw * unfinished.long()
        seq[:, t] = it
        lgs.append(logits)
        if not bool(unfinished.any()):
            break
    return seq, torch.stack(lps, 1), torch.stack(lgs, 1)


def objective_loss(lp, logits, seq, spec, data, M=None, N=None):
    """the definitions of include/icz.h ("SCST objectives") in torch float64 on the oracle's log-probs and logits [rows, steps run, V]"""
    rows, T = seq.shape
    run = logits.shape[1]              # (oracle.butd.sample_rl pads its log-probs to T with zeros)
    lp = lp[:, :run]
    mask = torch.ones(rows, T, dtype=torch.float64)
    mask[:, 1:] = (seq[:, :-1] > 0).double()
    assert not bool(mask[:, run:].any())
    msum = mask.sum()
    M = msum if M is None else M
    mk = mask[:, :run]
    if spec["kind"] == "reinforce":
        obj = -(lp * torch.as_tensor(data).double()[:, :run] * mk).sum() / M
    else:
        K = spec["K"]
        s = (lp * mk).sum(1).view(-1, K)
        Q = torch.softmax(spec["a"] * s, 1)
        obj = (Q * -torch.as_tensor(data).double().view(-1, K)).sum() / (N if N is not None else rows // K)
    lsm = torch.log_softmax(logits, 2)
    ent = (mk * -(lsm.exp() * lsm).sum(2)).sum() / M
    return obj - spec["b"] * ent, obj, ent, float(msum)


def device_objective(spec, data, n_img_global=0.0):
    from simpleimagecaptionzoo_amd.scst_objective import make_objective
    kw = {"reward": torch.tensor(data, dtype=torch.float32, device="cuda")} if spec["kind"] == "reinforce" else \
        {"scores": torch.tensor(data, dtype=torch.float64, device="cuda")}
    return make_objective(spec["kind"], spec["K"], spec["a"], spec["b"], n_img_global=n_img_global, **kw)


def spec_of(kind, K, a=1.0, b=0.0):
    return {"kind": kind, "K": K, "a": a, "b": b}


def data_of(spec, rows, T, seed):
    rs = np.random.RandomState(seed)
    if spec["kind"] == "reinforce":
        return rs.randn(rows, 1).astype(np.float32).repeat(T, 1)
    return rs.rand(rows) * 3.0


def check_grads(grads, want, what):
    """2e-4 of each tensor's maximum (tests/test_gpu_butd.py _check_grads, test_gpu_nic.py check_grads, the families' check_grads)"""
    for k, v in grads.items():
        w = np.asarray(want[k], dtype=np.float64)
        got = v.cpu().double().numpy()
        scale = max(1e-3, float(np.abs(w).max()))
        err = float(np.abs(got - w).max())
        print("%s %-50s max|want| %.3e  err/scale %.3e" % (what, k, float(np.abs(w).max()), err / scale))
        assert np.isfinite(got).all() and err <= 2e-4 * scale + 2e-6, (what, k, err, scale)


def check_loss3(loss3, want, what):
    got = loss3.cpu().numpy()
    print("%s loss3 %s oracle %s" % (what, got, [float(x) for x in want]))
    for g, w in zip(got, want):
        assert abs(float(g) - float(w)) < 1e-4, (what, got, want)


def copy_run(out, grads):
    return [t.clone() for t in out if t is not None], {k: v.clone() for k, v in grads.items()}


def equal_runs(a, b, what=""):
    assert len(a[0]) == len(b[0])
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y), what
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), (what, k)


# ---- BUTD ---------------------------------------------------------------------------------------------------
class Butd:
    """the tiny golden's decoder on its first n_img images, K rows per image (K = 1: sample(), or rollouts() when merged)"""

    def __init__(self, golden_dir, n_img, K, T, seed, merged=False, end_bias=END_BIAS):
        from oracle import butd as ob
        import test_gpu_butd as tb
        g = tb.load(golden_dir, "butd_dec_tiny")
        self.dims = [int(x) for x in g["dims"]]
        sd = tb.sd_of(g)
        sd["predict.bias"] = sd["predict.bias"].copy()
        sd["predict.bias"][2] = end_bias
        self.sd = ob.strip_prefix(sd)
        self.g, self.n_img, self.K, self.T, self.merged = g, n_img, K, T, merged
        self.rows = n_img * K
        _, R, D, H, E, A, V = self.dims
        rs = np.random.RandomState(seed)
        self.em, self.am, self.om = rs.rand(T, self.rows, E) < 0.5, rs.rand(T, self.rows, R, A) < 0.5, rs.rand(T, self.rows, H) < 0.5
        self.u = rs.rand(T, self.rows).astype(np.float32)
        self.feats = torch.tensor(g["feats"][:n_img])

    def handle(self, graphs=False, **options):
        import test_gpu_butd as tb
        h, _ = tb.make_handle(self.g, self.sd, max_rows=max(8, 2 * self.rows), max_len=20)
        for k, v in options.items():
            h.set_option(k, v)
        if graphs:
            h.enable_graphs(True)
        return h

    def rng(self, seed=None):
        from simpleimagecaptionzoo_amd.butd import make_rng
        if seed is not None:
            return make_rng(seed)
        t = lambda x: torch.tensor(np.ascontiguousarray(x), device="cuda")
        return make_rng(0, t(self.u), t(self.em.astype(np.uint8)), t(self.am.astype(np.uint8)), t(self.om.astype(np.uint8)))

    def roll(self, h, rng):
        f = self.feats.cuda()
        if self.K > 1:
            return h.sample_n(f, self.K, self.T, rng)
        if self.merged:
            return h.rollouts(f, self.T, rng)[1:]
        return h.sample(f, self.T, rng)

    def oracle(self, loss_fn):
        from oracle import butd as ob
        with f64():
            p = {k: torch.tensor(np.asarray(v), dtype=torch.float64).requires_grad_(True) for k, v in self.sd.items()}
            seq, lp, logits = ob.sample_rl(self.feats.double().repeat_interleave(self.K, 0), p, self.u.astype(np.float64), self.em, self.am,
                                           self.om, self.T)
            out = loss_fn(lp, logits, seq)
            gs = torch.autograd.grad(out[0], list(p.values()), allow_unused=True)
        return seq.numpy(), out, {k: (g.numpy() if g is not None else np.zeros(tuple(p[k].shape))) for k, g in zip(p, gs)}, None


# ---- NIC ----------------------------------------------------------------------------------------------------
class Nic:
    def __init__(self, golden_dir, n_img, K, T, seed, end_bias=END_BIAS):
        import test_gpu_nic as tn
        g = tn.load(golden_dir, "nic_dec_tiny")
        _, H, E, V = [int(x) for x in g["dims"]]
        self.sd = {k[3:]: v.copy() for k, v in g.items() if k.startswith("sd.")}
        self.sd["predict.bias"][2] = end_bias
        self.g, self.n_img, self.K, self.T, self.rows = g, n_img, K, T, n_img * K
        rs = np.random.RandomState(seed)
        self.om = rs.rand(T, self.rows, H) < 0.5
        self.u = rs.rand(T, self.rows).astype(np.float32)
        self.feats = torch.tensor(g["feats"][:n_img])

    def handle(self, graphs=False, **options):
        import test_gpu_nic as tn
        from simpleimagecaptionzoo_amd._lib import check
        h = tn.make(self.g, self.sd, max_rows=max(16, self.rows))
        for k, v in options.items():      # (NicHandle has no set_option method: tests/test_cpu_handle_surface.py holds it to that)
            check(h._e.set_option(h._h, k.encode(), int(v)))
        return h

    def rng(self, seed=None):
        from simpleimagecaptionzoo_amd.butd import make_rng
        if seed is not None:
            return make_rng(seed)
        return make_rng(0, torch.tensor(self.u, device="cuda"), None, None, torch.tensor(self.om.astype(np.uint8), device="cuda"))

    def roll(self, h, rng):
        from simpleimagecaptionzoo_amd.multisample import sample_n
        f = self.feats.cuda()
        return sample_n(h, f, self.K, self.T, rng) if self.K > 1 else h.sample(f, self.T, rng)

    def oracle(self, loss_fn):
        from oracle import nic as on
        with f64():
            p = {k: torch.tensor(np.asarray(v), dtype=torch.float64).requires_grad_(True) for k, v in self.sd.items()}
            feats = self.feats.double().requires_grad_(True)
            state = list(on.init_state(feats.repeat_interleave(self.K, 0), p))

            def step(t, it):
                logits, state[0], state[1] = on.step(it, state[0], state[1], p, torch.as_tensor(self.om[t]))
                return logits
            seq, lp, logits = oracle_rollout(step, self.rows, self.T, self.u.astype(np.float64))
            out = loss_fn(lp, logits, seq)
            gs = torch.autograd.grad(out[0], list(p.values()) + [feats], allow_unused=True)
        return seq.numpy(), out, {k: g.numpy() for k, g in zip(p, gs)}, gs[-1].numpy()


# ---- AoA ----------------------------------------------------------------------------------------------------
class Aoa:
    def __init__(self, golden_dir, n_img, K, T, seed, lens=None, train_refiner=False, end_bias=END_BIAS):
        cfg = (n_img,) + fam._tiny_dims() + (T, lens, end_bias)
        sd = ar.state_dict_of(cfg, seed)
        per_img, _ = ar.masks_of(cfg, seed + 2, n_img, T)
        per_row, u = ar.masks_of(cfg, seed + 3, n_img * K, T)
        masks = {k: (per_img if k in ("proj", "ref_att", "ref_aoa", "ref_sc") else per_row)[k] for k in ar.MASKS}
        self.c = {"cfg": cfg, "K": K, "sd": sd, "feats": ar.feats_of(cfg, seed + 1), "masks": masks, "u": u}
        self.n_img, self.K, self.T, self.rows, self.train_refiner = n_img, K, T, n_img * K, train_refiner

    def handle(self, graphs=False, **options):
        import test_gpu_scst_multisample_families as tf
        if graphs:
            options = dict(options, graphs=1)
        return tf.make_handle(self.c, self.train_refiner, options, max_rows=max(8, self.rows))

    def rng(self, seed=None):
        from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
        return make_aoa_rng(seed) if seed is not None else ar.device_rng(self.c["masks"], self.c["u"])

    def roll(self, h, rng):
        from simpleimagecaptionzoo_amd.multisample import sample_n
        f = ar.batch_of(self.c["cfg"], self.c["feats"])
        return sample_n(h, f, self.K, self.T, rng) if self.K > 1 else h.sample(f, self.T, rng)

    def oracle(self, loss_fn):
        c = self.c
        rep, feats, masks = fam.repeated(c)
        with ar.oracle_dtype(rep[6], torch.float64) as oa:
            p = {k: v.detach().double().requires_grad_(True) for k, v in c["sd"].items()}
            enc = oa.refine(feats.double(), p, masks, rep[8])
            bu = oa.key_mask(rep[8], enc.shape[1])
            meanf, st = oa.masked_mean(enc, bu), [oa._zero(enc.shape[0], enc.shape[2])]

            def step(t, it):
                logits, _, st[0] = oa.dec_step(it, st[0], enc, meanf, p, oa._step_masks(masks, t), bu)
                return logits
            seq, lp, logits = oracle_rollout(step, self.rows, self.T, c["u"].astype(np.float64))
            out = loss_fn(lp, logits, seq)
            gs = torch.autograd.grad(out[0], list(p.values()), allow_unused=True)
        return seq.numpy(), out, {k: (g.numpy() if g is not None else np.zeros(tuple(p[k].shape))) for k, g in zip(p, gs)}, None


def against_oracle(m, spec, what, M_global=None, n_glob=None):
    """rollout on the device (the oracle's tokens), the objective's backward pass, every gradient and {loss, obj, ent} against autograd"""
    from simpleimagecaptionzoo_amd.scst_objective import sample_backward_objective
    data = data_of(spec, m.rows, m.T, 77)
    w_seq, (w_loss, w_obj, w_ent, w_msum), want, w_dfe = m.oracle(
        lambda lp, lg, seq: objective_loss(lp, lg, seq, spec, data, M_global, n_glob))
    h = m.handle()
    seq, _ = m.roll(h, m.rng())
    assert np.array_equal(seq.cpu().numpy(), w_seq), (what, "the device drew other tokens than the oracle")
    on = np.concatenate([np.ones((m.rows, 1), bool), w_seq[:, :-1] > 0], 1)
    assert on.sum(1).min() < m.T or m.T <= 2, (what, "no row ends early")
    grads = h.new_grads()
    nic = h.family == "nic"
    out = sample_backward_objective(h, device_objective(spec, data, n_glob or 0.0), grads, M_global or 0.0, want_entropy=True, want_dfeats=nic)
    check_loss3(out[0], (w_loss.item(), w_obj.item(), w_ent.item() if spec["b"] > 0 else 0.0), what)
    assert float(out[1].item()) == w_msum
    ent = out[2].cpu().numpy()
    assert (ent[~on] == 0).all() and ((ent[on] > 0).all() if spec["b"] > 0 else not ent.any())
    check_grads(grads, want, what)
    if nic:
        np.testing.assert_allclose(out[3].cpu().numpy(), w_dfe, atol=2e-5, rtol=2e-4)      # tests/test_gpu_nic.py's d features tolerance
    h.close()


@pytest.mark.parametrize("n_img,K,T,kind,a,b", [(3, 5, 6, "risk", 1.0, 0.01), (2, 3, 7, "risk", 4.0, 0.0), (2, 2, 8, "reinforce", 1.0, 0.5)])
def test_butd_gradients_against_the_oracle(golden_dir, n_img, K, T, kind, a, b):
    against_oracle(Butd(golden_dir, n_img, K, T, 11 + K), spec_of(kind, K, a, b), "butd %dx%d %s" % (n_img, K, kind))


@pytest.mark.parametrize("n_img,K,T,kind,a,b", [(3, 3, 7, "risk", 0.25, 0.01), (2, 5, 6, "reinforce", 1.0, 0.5)])
def test_nic_gradients_and_d_features_against_the_oracle(golden_dir, n_img, K, T, kind, a, b):
    against_oracle(Nic(golden_dir, n_img, K, T, 21 + K), spec_of(kind, K, a, b), "nic %dx%d %s" % (n_img, K, kind))


@pytest.mark.parametrize("n_img,K,T,kind,a,b,lens,refiner", [
    (3, 5, 6, "risk", 1.0, 0.01, None, False), (2, 2, 8, "reinforce", 1.0, 0.5, None, False),
    (2, 3, 6, "risk", 1.0, 0.5, None, True),                       # train_refiner: the gradients of all 82 tensors
    (3, 2, 6, "risk", 0.25, 0.01, [36, 5, 17], False)])            # per-image region counts
def test_aoa_gradients_against_the_oracle(golden_dir, n_img, K, T, kind, a, b, lens, refiner):
    against_oracle(Aoa(golden_dir, n_img, K, T, 640 + K, lens, refiner), spec_of(kind, K, a, b), "aoa %dx%d %s" % (n_img, K, kind))


@pytest.mark.parametrize("family", ["butd", "butd_merged", "nic", "aoa"])
def test_entropy_after_a_single_sample_rollout_gives_the_oracle_gradient(golden_dir, family):
    """K = 1: sample(), and for BUTD the merged chain of rollouts() (at most 8 images: 2 B rows per step slot, the baseline's in front)"""
    m = {"butd": lambda: Butd(golden_dir, 3, 1, 7, 31), "butd_merged": lambda: Butd(golden_dir, 4, 1, 7, 32, merged=True),
         "nic": lambda: Nic(golden_dir, 3, 1, 7, 33), "aoa": lambda: Aoa(golden_dir, 3, 1, 6, 650)}[family]()
    against_oracle(m, spec_of("reinforce", 1, 1.0, 0.5), family + " single sample")


# ---- bit-for-bit equalities ---------------------------------------------------------------------------------
# (<end> biases under which, on the cases' explicit uniforms, every row has ended by step 13 of 20 and some run 3 to 7 steps: the
# early-out has steps to leave out)
FAMILIES = {"butd": lambda gd: Butd(gd, 3, 4, 20, 45, end_bias=8.0), "nic": lambda gd: Nic(gd, 3, 4, 20, 45, end_bias=10.0),
            "aoa": lambda gd: Aoa(gd, 3, 4, 20, 703, None, True, end_bias=4.0)}


def _backward(m, h, spec, data, rng, n_glob=0.0, want_entropy=True):
    from simpleimagecaptionzoo_amd.scst_objective import sample_backward_objective
    seq, lp = m.roll(h, rng)
    grads = h.new_grads()
    out = sample_backward_objective(h, device_objective(spec, data, n_glob), grads, want_entropy=want_entropy, want_dfeats=h.family == "nic")
    return copy_run((seq, lp) + tuple(out), grads)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_kind0_without_entropy_is_sample_backward_bit_for_bit(golden_dir, family):
    from simpleimagecaptionzoo_amd.scst_objective import sample_backward_objective
    m = FAMILIES[family](golden_dir)
    spec = spec_of("reinforce", m.K)
    data = data_of(spec, m.rows, m.T, 5)
    for graphs in ((False, True) if family != "nic" else (False,)):
        h = m.handle(graphs)
        for i in range(2):              # with graphs: the capture, then a replay
            m.roll(h, m.rng(900))
            g0 = h.new_grads()
            kw = {"want_dfeats": True} if family == "nic" else {}
            old = [t.clone() for t in h.sample_backward(torch.tensor(data, device="cuda"), g0, **kw)]
            m.roll(h, m.rng(900))
            g1 = h.new_grads()
            new = sample_backward_objective(h, device_objective(spec, data), g1, **kw)
            assert torch.equal(new[0][0:1], old[0]) and torch.equal(new[0][1:2], old[0]) and float(new[0][2]) == 0.0, (family, graphs, i)
            assert torch.equal(new[1], old[1]) and (family != "nic" or torch.equal(new[2], old[2]))
            for k in g0:
                assert torch.equal(g0[k], g1[k]), (family, graphs, i, k)
            assert any(bool(v.any()) for v in g0.values())
        h.close()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_two_runs_graph_replay_and_early_out_change_no_bit(golden_dir, family):
    m = FAMILIES[family](golden_dir)
    spec = spec_of("risk", m.K, 1.0, 0.01)
    data = data_of(spec, m.rows, m.T, 6)
    h = m.handle()
    # explicit uniforms and masks: every row ends well before the last step (the oracle's rollout on them says so), some after 3 or more
    known = _backward(m, h, spec, data, m.rng())
    equal_runs(known, _backward(m, h, spec, data, m.rng()), "two eager runs")
    seq = known[0][0].cpu().numpy()
    assert not seq[:, -2:].any() and seq[:, 2].any(), "the rollout should end before its last steps for the early-out to matter"
    e = m.handle(early_out=0)
    equal_runs(known, _backward(m, e, spec, data, m.rng()), "every step run")
    e.close()
    # Philox draws: what the captured graphs take
    first = _backward(m, h, spec, data, m.rng(4242))
    equal_runs(first, _backward(m, h, spec, data, m.rng(4242)), "two eager Philox runs")
    other = _backward(m, h, spec, data, m.rng(4243))
    assert not torch.equal(first[0][1], other[0][1])
    h.close()
    if family == "nic":
        return
    g = m.handle(True)
    for i in range(3):                  # the capture, then two replays; the middle one on other draws
        got = _backward(m, g, spec, data, m.rng(4242 + (i == 1)))
        equal_runs(got, other if i == 1 else first, "graphs, call %d" % i)
    # another objective on the same buffers must not replay the first one's graph
    spec2 = spec_of("risk", m.K, 1.0, 0.5)
    e2 = m.handle()
    equal_runs(_backward(m, g, spec2, data, m.rng(4242)), _backward(m, e2, spec2, data, m.rng(4242)), "graphs, another entropy weight")
    g.close()
    e2.close()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_twice_the_image_count_halves_every_risk_gradient_exactly(golden_dir, family):
    m = FAMILIES[family](golden_dir)
    spec = spec_of("risk", m.K, 1.0, 0.0)
    data = data_of(spec, m.rows, m.T, 7)
    h = m.handle()
    one = _backward(m, h, spec, data, m.rng(77), 0.0)
    two = _backward(m, h, spec, data, m.rng(77), 2.0 * m.n_img)
    assert torch.equal(two[0][2][1], one[0][2][1] * 0.5)
    for k in one[1]:
        assert torch.equal(two[1][k], one[1][k] * 0.5), k
    assert sum(bool(v.any()) for v in one[1].values()) >= len(one[1]) - 2      # (d affine.bias is 0: a softmax ignores a shift)
    h.close()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_refusals_queue_nothing_and_leave_the_rollout_stored(golden_dir, family):
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.scst_objective import make_objective, sample_backward_objective
    m = FAMILIES[family](golden_dir)
    h = m.handle()
    rw = data_of(spec_of("reinforce", 1), m.rows, m.T, 8)
    m.roll(h, m.rng(55))
    want = h.new_grads()
    ref = [t.clone() for t in h.sample_backward(torch.tensor(rw, device="cuda"), want)[:2]]
    m.roll(h, m.rng(55))
    grads = {k: torch.full_like(v, 7.5) for k, v in want.items()}
    scores = torch.rand(m.rows, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(IczError, match="stored rollout has %d" % m.K):
        sample_backward_objective(h, make_objective("risk", 2 if m.K != 2 else 4, scores=scores), grads)
    with pytest.raises(IczError, match="scores"):
        sample_backward_objective(h, make_objective("risk", m.K), grads)
    with pytest.raises(IczError, match="multiple of K=5"):
        sample_backward_objective(h, make_objective("reinforce", 5, reward=torch.tensor(rw, device="cuda")), grads)
    torch.cuda.synchronize()
    assert all(bool((v == 7.5).all()) for v in grads.values())
    got = h.sample_backward(torch.tensor(rw, device="cuda"), grads)          # the rollout is still there
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    for k in want:
        assert torch.equal(grads[k], want[k]), k
    with pytest.raises(IczError, match="no rollout stored"):
        sample_backward_objective(h, make_objective("risk", m.K, scores=scores), grads)
    h.close()


# ---- Engine -------------------------------------------------------------------------------------------------
def _params(eng):
    return {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}


def _by_hand(ref, opt, batches, rngs, K, a, b):
    """the step from its parts on the engine's own stream: sample_n, reward_loo's scores, sample_backward_objective, clamp 0.25 + Adam"""
    from simpleimagecaptionzoo_amd.multisample import sample_n
    from simpleimagecaptionzoo_amd.scst_objective import make_objective, sample_backward_objective
    losses = []
    with torch.cuda.stream(ref.stream):
        for (ids, _, gts, supp), r in zip(batches, rngs):
            ref.model.train()
            feats = ref._features(ref.modify_visual_inputs(None, supp))
            h = ref._hot_handle()
            seq, _ = sample_n(h, feats, K, 20, r())
            _, scores = ref.scorer().reward_loo(seq, K, gts, ids, return_scores=True)
            grads = ref._grads()
            loss3, _ = sample_backward_objective(h, make_objective("risk", K, a, b, scores=scores), grads)
            losses.append(loss3.clone())
            ref._apply(opt, 0.25)
    torch.cuda.synchronize()
    return losses


def _engine_against_hand(make_engine, batches, rngs, K):
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    a, b = 1.0, 0.01
    eng = make_engine()
    start = _params(eng)
    eng.scst_terms = []
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    losses = []
    for bt, r in zip(batches, rngs):
        losses += eng.SCST_objective_training_epoch([bt], opt, None, tqdm_visible=False, rngs=[r()], samples_per_image=K, objective="risk",
                                                    risk_alpha=a, entropy_weight=b)
    torch.cuda.synchronize()
    got = _params(eng)
    ref = make_engine()
    opt2 = init_optimizer("Adam", ref.model.get_param_groups({"lr": 2e-5}), 2e-5)
    hand = _by_hand(ref, opt2, batches, rngs, K, a, b)
    want = _params(ref)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert any(not torch.equal(got[k], start[k]) for k in got)
    assert len(losses) == len(hand) == len(eng.scst_terms) == 2
    for l, h3, (o, e) in zip(losses, hand, eng.scst_terms):
        assert torch.equal(l, h3[0:1]) and torch.equal(o, h3[1:2]) and torch.equal(e, h3[2:3]) and float(e) > 0


def test_butd_engine_risk_steps_equal_the_steps_built_by_hand(golden_dir):
    import test_gpu_scst_multisample as tms
    K = 4
    g, fx, batches, rngs = tms._steps(golden_dir, K)
    _engine_against_hand(lambda: tms._engine(g, fx), batches, rngs, K)


def test_aoa_engine_risk_steps_equal_the_steps_built_by_hand(golden_dir):
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
    rngs = [lambda s=s: make_aoa_rng(900 + s) for s in range(2)]
    _engine_against_hand(engine, batches, rngs, 5)


def test_default_arguments_reproduce_the_existing_epochs(golden_dir):
    import test_gpu_scst_multisample as tms
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    K = 4
    g, fx, batches, rngs = tms._steps(golden_dir, K)
    B, R_, D_, H_, E_, A_, V_ = [int(x) for x in g["dims"]]
    for multi, kws in ((True, ({}, {"objective": "loo", "risk_alpha": 1.0, "entropy_weight": 0.0})), (False, ({}, {"entropy_weight": 0.0}))):
        out = []
        for kw in kws:
            eng = tms._engine(g, fx)
            eng.scst_terms = []
            opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
            for s, (b, r) in enumerate(zip(batches, rngs)):
                if multi:
                    epoch = eng.SCST_objective_training_epoch if kw else eng.SCST_multisample_training_epoch
                    epoch([b], opt, None, tqdm_visible=False, rngs=[r()], samples_per_image=K, **kw)
                else:
                    eng.SCST_training_epoch([b], opt, None, tqdm_visible=False, rngs=[tms._rng(B, 40 + s, True, R_, E_, A_, H_)], **kw)
            torch.cuda.synchronize()
            assert eng.scst_terms == []          # today's calls: no objective ran
            out.append(_params(eng))
        for k in out[0]:
            assert torch.equal(out[0][k], out[1][k]), k


def test_single_sample_epoch_with_entropy_moves_the_parameters_off_the_plain_step(golden_dir):
    """SCST_training_epoch(entropy_weight > 0): the greedy-baseline step (six images: the merged chain) and the samples_per_image form"""
    import test_gpu_scst_multisample as tms
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    g, fx, batches, _ = tms._steps(golden_dir, 1)
    B, R_, D_, H_, E_, A_, V_ = [int(x) for x in g["dims"]]
    for K in (None, 3):
        out = []
        for w in (0.0, 0.5):
            eng = tms._engine(g, fx)
            eng.scst_terms = []
            opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
            loss = eng.SCST_training_epoch([batches[0]], opt, None, tqdm_visible=False, rngs=[tms._rng(B * (K or 1), 40, True, R_, E_, A_, H_)],
                                           samples_per_image=K, entropy_weight=w)
            torch.cuda.synchronize()
            assert len(eng.scst_terms) == (1 if w else 0) and np.isfinite(loss[0].item())
            if w:
                obj, ent = eng.scst_terms[0]
                assert 0 < float(ent) <= np.log(V_) and abs(float(loss[0]) - (float(obj) - w * float(ent))) < 1e-5
            out.append(_params(eng))
        assert any(not torch.equal(out[0][k], out[1][k]) for k in out[0])


# ---- data parallelism ---------------------------------------------------------------------------------------
def dp_reference(golden_dir, K=4):
    """the parameters after two risk + entropy steps of one process on all six golden images"""
    import test_gpu_scst_multisample as tms
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    g, fx, batches, rngs = tms._steps(golden_dir, K)
    eng = tms._engine(g, fx)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    for b, r in zip(batches, rngs):
        eng.SCST_objective_training_epoch([b], opt, None, tqdm_visible=False, rngs=[r()], samples_per_image=K, objective="risk",
                                          entropy_weight=0.01)
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
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   ICZ_TEST_REF=ref_file)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "scst_objective_dp_worker.py")], env=env,
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
