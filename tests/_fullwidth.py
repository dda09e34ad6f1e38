"""Helpers shared by the full-width GPU parity tests (not collected by pytest): parameters / inputs at the benchmark width (36 x 2048
features, H = E = A = 1024, V = 10102), the excuse rules of SURVEY.md section 7 (near-ties of the two largest logits, draws within
fp32 rounding of a CDF edge), the float64 gradient yardstick, and the full-width SCST case every BUTD row-count test runs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from synth import feats_from_seed, probe_indices  # noqa: E402,F401

R, D, H, E, A, V = 36, 2048, 1024, 1024, 1024, 10102
FULL_DIMS = (R, D, H, E, A, V)


def _cpu(params, grad=False):
    return {k: v.detach().cpu().clone().requires_grad_(grad) for k, v in params.items()}


def _full_params(seed=77, sharpen=6.0, dims=FULL_DIMS):
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    params = random_butd_params(*dims, "cuda", seed=seed)
    params["predict.weight_g"].mul_(sharpen)      # trained decoders are far from uniform: well separated argmax / draws
    return params


def _first_divergence(got, want):
    """per row: index of the first differing step, or -1"""
    ne = got != want
    return np.where(ne.any(1), ne.argmax(1), -1)


def _excuse_greedy(greedy, w_greedy, w_glog, limit):
    """token-exact up to near-ties (< 1e-4) of the two largest logits at the first differing step; returns the excused rows"""
    div = _first_divergence(greedy, w_greedy.numpy())
    rows = np.nonzero(div >= 0)[0]
    for b in rows:
        top2 = torch.topk(w_glog[b, div[b]], 2).values
        assert float(top2[0] - top2[1]) < 1e-4, "greedy row %d differs at step %d with margin %g" % (b, div[b], float(top2[0] - top2[1]))
    assert len(rows) <= limit, "greedy: %d rows excused" % len(rows)
    return rows


def _excuse_sampled(seq, w_seq, w_slog, u, limit):
    """exact up to draws within 1e-6 of a CDF boundary (float64 softmax of the oracle's logits); returns the boolean mask of equal rows"""
    sdiv = _first_divergence(seq, w_seq.numpy())
    rows = np.nonzero(sdiv >= 0)[0]
    for b in rows:
        t = sdiv[b]
        c = torch.cumsum(torch.softmax(w_slog[b, t].detach().double(), 0), 0)
        tgt = float(u[t, b]) * float(c[-1])
        assert float((c - tgt).abs().min()) < 1e-6, "sampled row %d differs at step %d away from a CDF boundary" % (b, t)
    assert len(rows) <= limit, "sampled: %d rows excused" % len(rows)
    return sdiv < 0


def _units(x):
    """per-unit maxima: rows of a matrix (one output unit each), elements of a vector"""
    return x.reshape(x.shape[0], -1).max(1) if x.ndim >= 2 else x


def check_grads_against_float64(grads, g32, g64, kink_units=None, skip=("atten.affine.bias",)):
    """Every unit of every gradient tensor: |HIP - f64| <= 2 |torch32 - f64| + 2e-4 max|f64|.  `kink_units` ({tensor name prefix:
    boolean [A]}): attention units with a kept relu pre-activation within fp32 rounding of zero in the float64 pass; only those
    may leave the bound (a flipped relu element moves the unit's gradient by a finite amount in ANY fp32 evaluation), they are
    counted (at most 1 % of the units) and capped at 2e-2 of the maximum."""
    report = {}
    for k, gt in grads.items():
        if k in skip:
            continue
        got, w32, w64 = gt.cpu().double().numpy(), g32[k].astype(np.float64), g64[k]
        scale = max(1e-6, float(np.abs(w64).max()))
        e_hip, e_o32 = _units(np.abs(got - w64)), _units(np.abs(w32 - w64))
        bad = e_hip > 2.0 * e_o32 + 2e-4 * scale + 1e-7
        report[k] = (float(e_hip.max() / scale), float(e_o32.max() / scale), int(bad.sum()))
        if not bad.any():
            continue
        kink = None
        for pre, m in (kink_units or {}).items():
            if k.startswith(pre):
                kink = m
        assert kink is not None, (k, "units outside the float64 bound", np.nonzero(bad)[0][:8], report[k])
        unexplained = bad & ~kink
        assert not unexplained.any(), (k, "units outside the bound without a relu pre-activation at zero", np.nonzero(unexplained)[0][:8], report[k])
        assert bad.sum() <= max(1, bad.size // 100) and e_hip[bad].max() <= 2e-2 * scale, (k, int(bad.sum()), float(e_hip[bad].max()), scale)
    return report


def attention_kink_units(feats64, p64, h1_steps, att_masks, tol=3e-6, active_rows=None):
    """[A] boolean: attention unit a has an element z[t, b, r, a] = enc_ctx[b, r, a] + dec_ctx_t[b, a] (float64) that dropout keeps
    and that lies within `tol` x (|enc_ctx| + |dec_ctx| + 1) of zero -- the resolution at which two fp32 evaluations of the two
    dot products (2048 and 1024 terms) can disagree about the sign."""
    from oracle import butd as ob
    with torch.no_grad():
        enc = feats64 @ ob.wn_weight(p64, "atten.enc_att").t() + p64["atten.enc_att.bias"]          # [B, R, A]
        w_dec, b_dec = ob.wn_weight(p64, "atten.dec_att"), p64["atten.dec_att.bias"]
        hit = torch.zeros(enc.shape[2], dtype=torch.bool)
        for t, h1 in enumerate(h1_steps):
            dec = (h1 @ w_dec.t() + b_dec).unsqueeze(1)                                               # [B, 1, A]
            z = enc + dec
            near = z.abs() <= tol * (enc.abs() + dec.abs() + 1.0)
            if att_masks is not None:
                near &= torch.as_tensor(att_masks[t]).reshape(near.shape)
            if active_rows is not None:                                                               # XE: the batch shrinks with t
                near[active_rows[t]:] = False
            hit |= near.any(0).any(0)
    return hit.numpy()


def _butd_scst_inputs(B, T, seed, sharpen=6.0, dims=FULL_DIMS, samples_per_image=1, device="cuda"):
    """the inputs of _butd_scst_case (every value comes from CPU generators, so the oracle alone can run on them without a GPU):
    (params on `device`, image features [B / K, R, D], features per decoder row [B, R, D], keep-masks em / am / om, uniforms u [T, B],
    the RandomState behind them)"""
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    R, D, H, E, A, V = dims
    K = samples_per_image
    assert B % K == 0
    params = random_butd_params(R, D, H, E, A, V, device, seed=seed)
    params["predict.weight_g"].mul_(sharpen)
    g = torch.Generator(device="cpu")
    g.manual_seed(1000 + seed)
    img_feats = torch.relu(torch.randn(B // K, R, D, generator=g))
    feats_c = img_feats.repeat_interleave(K, 0) if K > 1 else img_feats         # what each decoder row attends over
    rs = np.random.RandomState(seed)
    em, am, om = rs.rand(T, B, E) < 0.5, rs.rand(T, B, R, A) < 0.5, rs.rand(T, B, H) < 0.5
    u = rs.rand(T, B).astype(np.float32)
    return params, img_feats, feats_c, em, am, om, u, rs


def _butd_scst_oracle(params, img_feats, feats_c, em, am, om, u, T):
    """the fp32 and the float64 oracle pass of _butd_scst_case: ({"f32" / "f64": (params, seq, log-probs, logits, trace)}, greedy ids
    and greedy logits of the fp32 pass)"""
    from oracle import butd as ob
    out = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            p = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in params.items()}
            trace = {}
            w_seq, w_lp, w_slog = ob.sample_rl(feats_c.to(dt), p, u.astype(np.float64), em, am, om, T, early_exit=False, trace=trace, hoisted=True)
            out[name] = (p, w_seq, w_lp, w_slog, trace)
        finally:
            torch.set_default_dtype(torch.float32)
    p32 = out["f32"][0]
    with torch.no_grad():
        w_greedy, _, w_glog = ob.greedy(img_feats, {k: v.detach() for k, v in p32.items()}, T, hoisted=True)
    return out, w_greedy, w_glog


def _butd_scst_case(B, T, seed, sharpen=6.0, options=None, with_reward=False, dims=FULL_DIMS, samples_per_image=1, excused=None):
    """device rollouts + REINFORCE gradients of B rows x T steps at full width (or at the widths `dims` = (R, D, H, E, A, V)), and the
    fp32 / float64 oracle passes on the same inputs (options: {handle option: value} set before the run).  samples_per_image = K > 1:
    the B rows are K sampled captions of each of B / K images (sample_n; the greedy decode of the images runs beside it).
    with_reward: the step's CIDEr-D reward as well -- computed on the device from the ids the device produced, bit-exact against the oracle's (Utils.py:319-367) -- and used as the REINFORCE reward (plus a per-row
    signal: a random-init model scores ~0 against random references).  excused: a dict that receives the number of excused greedy rows,
    of excused sampled rows and of rows left out of the gradient comparison."""
    from oracle import butd as ob
    from simpleimagecaptionzoo_amd.butd import ButdHandle, make_rng
    R, D, H, E, A, V = dims
    K = samples_per_image
    params, img_feats, feats_c, em, am, om, u, rs = _butd_scst_inputs(B, T, seed, sharpen, dims, K)
    h = ButdHandle(R, D, H, E, A, V, max(B, 8), T)
    h.bind(params)
    for name, value in (options or {}).items():
        h.set_option(name, value)
    dev = "cuda"
    rng = make_rng(0, torch.tensor(u, device=dev), torch.tensor(em.astype(np.uint8), device=dev),
                   torch.tensor(am.astype(np.uint8), device=dev), torch.tensor(om.astype(np.uint8), device=dev))
    if K > 1:
        greedy = h.greedy(img_feats.cuda(), T).clone()
        seq, lp = h.sample_n(img_feats.cuda(), K, T, rng)
    else:
        greedy, seq, lp = h.rollouts(feats_c.cuda(), T, rng)
    greedy, seq, lp = greedy.cpu().numpy(), seq.cpu().numpy(), lp.cpu().numpy()
    out, w_greedy, w_glog = _butd_scst_oracle(params, img_feats, feats_c, em, am, om, u, T)
    limit = max(1, B // 32)
    ex_greedy = _excuse_greedy(greedy, w_greedy, w_glog, limit)
    ok = _excuse_sampled(seq, out["f32"][1], out["f32"][3], u, limit)
    ex_sampled = int((~ok).sum())
    ok &= (out["f64"][1].numpy() == seq).all(1)         # rows whose float64 draws agree as well take part in the gradient comparison
    assert ok.sum() >= B - 2 * limit
    if excused is not None:
        excused.update(greedy=len(ex_greedy), sampled=ex_sampled, left_out=int((~ok).sum()))
    np.testing.assert_allclose(lp[ok], out["f32"][2].detach().numpy()[ok], atol=1e-4)
    rw = (rs.randn(B, 1).astype(np.float32) * ok[:, None].astype(np.float32)).repeat(T, 1)
    if with_reward:
        from oracle import ciderd as oc
        from simpleimagecaptionzoo_amd.ciderd import CiderDReward
        from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
        from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
        vocab = synthetic_vocab(V)
        words = [vocab.ix2word[i] for i in range(V)]
        dfd = document_frequency(synthetic_references(2000, words, seed=0))
        refs = synthetic_references(B, words, seed=9)
        gts = {i: refs[i] for i in range(B)}
        scorer = CiderDReward(dfd["document_frequency"], dfd["ref_len"], vocab.word2ix, dev)
        reward = scorer.reward(torch.tensor(seq, device=dev), torch.tensor(greedy, device=dev), gts, list(range(B)))
        w_reward = oc.self_critical_reward(seq, greedy, gts, list(range(B)), dict(enumerate(words)),
                                           oc.DocFreq(dfd["document_frequency"], dfd["ref_len"]))
        assert reward.dtype == torch.float32 and reward.shape == (B, T) and np.array_equal(reward.cpu().numpy(), w_reward)
        rw = rw + np.where(ok[:, None], w_reward, 0.0).astype(np.float32)
    grads = h.new_grads()
    loss, _ = h.sample_backward(torch.tensor(rw, device=dev), grads)
    gsets = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            p, w_seq, w_lp, _, _ = out[name]
            w_seq_m = torch.from_numpy(np.where(ok[:, None], w_seq.numpy(), seq))
            w_loss = ob.reward_criterion(w_lp, w_seq_m, torch.from_numpy(rw).to(dt))
            w_loss.backward()
            gsets[name] = {k: v.grad.numpy() for k, v in p.items()}
            if name == "f32":
                assert abs(loss.item() - w_loss.item()) < 1e-4, (loss.item(), w_loss.item())
        finally:
            torch.set_default_dtype(torch.float32)
    p64, trace64 = out["f64"][0], out["f64"][4]
    kink = attention_kink_units(feats_c.double(), {k: v.detach() for k, v in p64.items()}, trace64["h1"], am)
    rep = check_grads_against_float64(grads, gsets["f32"], gsets["f64"], {"atten.enc_att": kink, "atten.dec_att": kink})
    h.close()
    return rep, kink


def _butd_inputs(seed, B, dims=FULL_DIMS):      # as tests/golden/make_fullwidth_goldens.py: butd_inputs
    R, D, H, E, A, V = dims
    rs = np.random.RandomState(seed)
    feats = feats_from_seed(seed + 1, B, R, D)
    st = [(rs.randn(B, H) * 0.5).astype(np.float32) for _ in range(4)]
    it = rs.randint(4, V, size=(B,)).astype(np.int64)
    return feats, st, it


def _aoa_captioner(seed):        # as make_fullwidth_goldens.py: aoa_captioner (the weights are a function of the seed)
    from simpleimagecaptionzoo_amd.aoa import AoADetection_Captioner
    torch.manual_seed(seed)
    m = AoADetection_Captioner(vocab_size=V, num_heads=8, hidden_dim=H, embed_dim=E, device="cpu")
    with torch.no_grad():
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed + 17)
        for name, prm in m.named_parameters():
            if name.endswith("norm.gain"):
                prm.add_(torch.randn(prm.shape, generator=gen) * 0.2)
            if name.endswith("norm.bias"):
                prm.add_(torch.randn(prm.shape, generator=gen) * 0.1)
    return m


# The 128-row resident GEMM inside real decodes (65..128 decoder rows): greedy evaluation at batch 128 and beam 5 over 25 images
# (125 rows; its first step runs one row per image = 25 rows, the later ones 125) at full width against the CPU oracle.
def _sharp_params(seed):
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    params = random_butd_params(R, D, H, E, A, V, "cuda", seed=seed)
    params["predict.weight_g"].mul_(6.0)        # trained decoders are far from uniform: well separated argmax (tests/test_gpu_butd_fullwidth.py)
    return params


def _end_biased_params(seed, p_end, B=64, dims=FULL_DIMS):
    """full-width parameters (or at `dims`) whose <end> logit is raised until a sampled step draws <end> with probability ~ p_end"""
    from simpleimagecaptionzoo_amd.butd import ButdHandle, make_rng
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    R, D, H, E, A, V = dims
    params = random_butd_params(R, D, H, E, A, V, "cuda", seed=seed)
    h = ButdHandle(R, D, H, E, A, V, B, 20)
    h.bind(params)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    feats = torch.relu(torch.randn(B, R, D, generator=g)).cuda()
    params["predict.bias"][2] += float(np.log(p_end * V / (1.0 - p_end)))
    for _ in range(3):
        h.refresh()
        seq, _ = h.sample(feats, 20, make_rng(123))
        p = float((seq[:, 0] == 0).float().mean().clamp(1.0 / (4 * B), 1 - 1.0 / (4 * B)))
        params["predict.bias"][2] += float(np.log(p_end / (1 - p_end)) - np.log(p / (1 - p)))
    h.close()
    return params, feats


# ---- merged greedy + sampled chain of a small SCST batch (Butd::sample_chain with row0 = B) ---------------------------------------
def _small_case(B, merged, params, feats, seed, end_bias=None, small_nt=1):
    from simpleimagecaptionzoo_amd.butd import ButdHandle, make_rng
    T = 20
    p = {k: v.clone() for k, v in params.items()}
    if end_bias is not None:
        p["predict.weight_g"][2] = 0.0
        p["predict.bias"][2] = end_bias
    h = ButdHandle(R, D, H, E, A, V, B, T)
    h.bind(p)
    h.set_option("merge_small", 32 if merged else 0)
    h.set_option("small_nt", small_nt)
    rs = np.random.RandomState(seed)
    em, am, om = rs.rand(T, B, E) < 0.5, rs.rand(T, B, R, A) < 0.5, rs.rand(T, B, H) < 0.5
    u = rs.rand(T, B).astype(np.float32)
    dev = "cuda"
    rng = make_rng(0, torch.tensor(u, device=dev), torch.tensor(em.astype(np.uint8), device=dev),
                   torch.tensor(am.astype(np.uint8), device=dev), torch.tensor(om.astype(np.uint8), device=dev))
    greedy, seq, lp = h.rollouts(feats, T, rng)
    rw = torch.tensor(rs.randn(B, 1).astype(np.float32).repeat(T, 1), device=dev)
    grads = h.new_grads()
    for v in grads.values():
        v.fill_(float("nan"))
    loss, msum = h.sample_backward(rw, grads)
    out = (greedy.cpu().numpy(), seq.cpu().numpy(), lp.cpu().numpy(), loss.item(), msum.item(), {k: v.cpu().numpy() for k, v in grads.items()})
    h.close()
    return out


# Large-tile split-precision GEMM (csrc/gemm_big_x3.hip): every tile configuration against float64 and against the 128 x 128 kernel
def _gemm_operands(layout, M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if layout == "nt":
        return torch.randn(M, K, device="cuda", generator=g), torch.randn(N, K, device="cuda", generator=g)
    if layout == "nn":
        return torch.randn(M, K, device="cuda", generator=g), torch.randn(K, N, device="cuda", generator=g)
    return torch.randn(K, M, device="cuda", generator=g), torch.randn(K, N, device="cuda", generator=g)


def _gemm_ref64(layout, X, W):
    X, W = X.double(), W.double()
    return X @ W.t() if layout == "nt" else (X @ W if layout == "nn" else X.t() @ W)


BIG_SHAPES = [("nt", 700, 4100, 1024, 1), ("nt", 700, 4100, 1024, 2), ("nt", 640, 1024, 1024, 4), ("nt", 2304, 1024, 1024, 1),
              ("nt", 129, 8200, 1152, 3), ("nt", 1280, 10102, 1024, 1),
              ("nn", 300, 260, 128, 1), ("nn", 1280, 1028, 2176, 4), ("nn", 130, 516, 2176, 1), ("nn", 1280, 1024, 4096, 2),
              ("tn", 2052, 2060, 96, 1), ("tn", 4096, 1024, 320, 1), ("tn", 2048, 2048, 64, 1), ("tn", 4100, 2044, 304, 1)]


def _check_dp_fields(j):
    """round 5: the N > 1 line explains itself -- per-phase times (max over ranks) and the same steps with the gradient exchange not
    overlapped with the backward pass"""
    ph = j["phases_ms"]
    assert set(("rollouts", "reward", "backward", "allreduce_exposed", "adam")) <= set(ph) and all(ph[k] >= 0 for k in ph)
    assert ph["rollouts"] > 0 and ph["backward"] > 0 and ph["adam"] > 0
    ov = j["dp_overlap"]
    assert ov["on_ms"] > 0 and ov["off_ms"] > 0 and ov["allreduce_exposed_off_ms"] > 0 and ov["allreduce_exposed_on_ms"] >= 0
    assert j["vs_baseline"] is None and j["vs_reference_in_container"] > 0


# ---- BUTD between the golden widths and the benchmark width -------------------------------------------------------------------------
# One table for the GPU parity tests (tests/test_gpu_butd_midwidth.py) and the CPU route test (tests/test_cpu_abi_and_host.py):
# name -> (dims = (R, D, H, E, A, V), [(rows, steps, kind)], what the width is there for).  kind: "scst" = rollouts + sample_backward,
# "merged" = the same on the merged chain of a small batch (merge_small), "sample_n4" = 4 samples per image.  `midwidth_routes` states
# each purpose as host predicates; the CPU test asserts them, so a retuned threshold names the width that lost its purpose.
MIDWIDTH = {
    "w512": ((36, 2048, 512, 512, 512, 3000), [(64, 20, "scst")],
             "gates N = 2048, the first width on the resident kernel; TD group not taken, LM group taken; td_w_hh, dWdec, dWenc and "
             "predict's weight gradient all on split-K slabs (gemm_tn_split) from two streams"),
    "w640": ((36, 2048, 640, 512, 384, 5000), [(64, 20, "scst")],
             "60 / 52 stages: the resident kernel's four-stage form; A != H != E; no weight-gradient group taken (640 % 256), td_w_hh and "
             "lm_w_hh both on split-K slabs beside the attention tail's and predict's"),
    "w768": ((36, 2048, 768, 512, 768, 10102), [(64, 20, "scst"), (100, 8, "scst")],
             "stage counts % 8 == 0 (512-deep resident form) away from 1024; 100 rows: the 128-row resident kernel; both weight-gradient "
             "groups taken with column groups of 768 and 512"),
    "w256": ((36, 1024, 256, 192, 320, 2051), [(48, 20, "scst"), (16, 20, "merged"), (48, 20, "sample_n4")],
             "gates N = 1024 < 2048: every decoder-step product on the fp32-MFMA kernels, no transposed weight copies; odd V; the merged "
             "chain of a 16-row batch; 4 samples per image"),
    "w336": ((49, 512, 336, 160, 224, 1237), [(20, 12, "scst")],
             "H and E no multiples of 64 (tail kernels), 4 H no multiple of 128 (the split-precision NN / NT kernels refuse the dgrad "
             "products); <= 32 rows (32-row NT tiles); 49 regions; no weight gradient on slabs"),
}


def midwidth_routes(name):
    """{claim: bool} -- what MIDWIDTH[name] is there for, from the library's host-only routing entries (no GPU needed)"""
    from simpleimagecaptionzoo_amd.butd import gemm_route_for as route, gemm_tn_grouped_fits as grouped, gemm_tn_split_pick as split
    (R_, D_, H_, E_, A_, V_), cases, _ = MIDWIDTH[name]
    B, T, _ = cases[0]
    TB, Vp = B * T, (V_ + 63) // 64 * 64
    td, lm = route("nt", B, 4 * H_, [H_, E_, H_]), route("nt", B, 4 * H_, [D_, H_, H_])
    td_grp, lm_grp = grouped(4 * H_, TB, [H_, E_, H_]), grouped(4 * H_, TB, [D_, H_, H_])
    s_hh, s_dec, s_enc, s_p = split(4 * H_, H_, TB), split(A_, H_, TB), split(A_, D_, B * R_), split(Vp, H_, TB)
    fp32_nt = ("nt_fp32_mt1", "nt_fp32_mt2", "nt_fp32_mt4")
    if name == "w512":
        return {"gates on the resident kernel": td.startswith("resident") and lm.startswith("resident"),
                "one width below (N = 1984) not": route("nt", B, 4 * 496, [496, E_, 496]) in fp32_nt,
                "TD group not taken, LM group taken": not td_grp and lm_grp,
                "td_w_hh, dWdec, dWenc, dWp on slabs": min(s_hh, s_dec, s_enc, s_p) > 1}
    if name == "w640":
        return {"four-stage resident form": td == lm == "resident_4stage",
                "no group taken": not td_grp and not lm_grp,
                "td_w_hh / lm_w_hh, dWdec, dWenc, dWp on slabs": min(s_hh, s_dec, s_enc, s_p) > 1}
    if name == "w768":
        B2, T2, _ = cases[1]
        return {"512-deep resident form at 64 rows": td == lm == "resident_512deep",
                "128-row resident kernel at 100 rows": route("nt", B2, 4 * H_, [H_, E_, H_]) == route("nt", B2, 4 * H_, [D_, H_, H_]) == "resident_128row",
                "both groups taken": td_grp and lm_grp and grouped(4 * H_, B2 * T2, [H_, E_, H_]) and grouped(4 * H_, B2 * T2, [D_, H_, H_]),
                "attention tail on slabs": s_dec > 1 and s_enc > 1}
    if name == "w256":
        small = [route("nt", 32, 4 * H_, [H_, E_, H_]), route("nt", 32, 4 * H_, [D_, H_, H_]), route("nt", 32, A_, [H_])]
        return {"decoder step on the fp32-MFMA NT kernel": td == lm == route("nt", B, A_, [H_]) == route("nt", B, Vp, [H_]) == "nt_fp32_mt4",
                "merged chain (32 rows) on 32-row tiles": all(r == "nt_fp32_mt2" for r in small),
                "per-step dgrad on the fp32 NN kernel": route("nn", B, D_ + H_, [4 * H_], 1) == "nn_fp32",
                "no group taken, weight gradients of the LSTMs on the 64 x 64 TN kernel": not td_grp and not lm_grp and route("tn", 4 * H_, D_, [TB], 1) == "tn_fp32_64",
                "odd V": V_ % 2 == 1 and V_ % 64 != 0}
    if name == "w336":
        return {"32-row NT tiles": td == lm == "nt_fp32_mt2",
                "K % 64 != 0 in the gate segments": H_ % 64 != 0 and E_ % 64 != 0,
                "dgrad over all steps refused by the split-precision NN kernel": route("nn", TB, E_, [4 * H_], 1) == "nn_fp32" and (4 * H_) % 128 != 0,
                "XE vocabulary projection on the fp32 NT kernel": route("nt", TB, Vp, [H_], 1) == "nt_fp32_mt4",
                "no weight gradient on slabs": max(s_hh, s_dec, s_enc, s_p) == 1 and not td_grp and not lm_grp}
    raise KeyError(name)


# ---- BUTD attention at any region count and attention width ------------------------------------------------------------------------
# One table for the GPU tests (tests/test_gpu_butd_attention.py) and the CPU test of the table itself (tests/test_cpu_attention_geometry.py):
# name -> (dims = (R, D, H, E, A, V), what the shape is there for).  The nine attention kernels of csrc/butd_kernels.h branch on R, D and
# A alone (H, E and V are kept small); `att_geometry_claims` states each purpose as a predicate on those numbers and on the kernels'
# constants below.  Every case runs ATT_ROWS rows x ATT_STEPS steps: more steps than att_bwd_denc_kernel<TT> keeps in registers, so
# d enc_ctx is re-read and re-written by a second time pass.
ATT_PARTS, TT, ATT_CTX_MAX_G = 4, 20, 8          # csrc/butd_impl.h, the <20> of csrc/butd_train.hip, csrc/butd_kernels.h
ATT_NB, ATT_GROUP_LDS = 3, 60 * 1024             # regions per wave and pass of att_scores_kernel; Butd::step's limit for the grouped scores
ATT_ROWS, ATT_STEPS = 12, 24
ATT_GEOMETRY = {
    "g_r1": ((1, 64, 32, 32, 32, 53),
             "one region: alpha = 1 and ds = 0 exactly; the empty upper half of att_ctx_kernel (r_lo == r_hi)"),
    "g_r2": ((2, 36, 32, 16, 20, 53),
             "Rh = 1: one region per half; A = 20, less than one 32-bit keep word; D = 36, one partly filled column part"),
    "g_r17": ((17, 512, 64, 32, 1280, 203),
              "A > 1024: the second c0 pass of the scores and d enc_ctx kernels (the scores kernel's prefetch serves the first only); "
              "A % 256 == 0: shared Philox words in all three kernels; R = the 16 (part, wave) slots + 1"),
    "g_r33": ((33, 128, 128, 64, 128, 1237),
              "A % 128 == 0 but A % 256 != 0: scores and d dec_ctx draw per element, d enc_ctx on shared words; odd R"),
    "g_r63": ((63, 1028, 64, 64, 256, 203),
              "R > 48: the second region group of att_scores_kernel; one softmax lane of -inf; D % 512 == 4: a column part of one float4; "
              "the smallest width with shared words in scores and d dec_ctx"),
    "g_r64": ((64, 516, 64, 36, 132, 203),
              "a full wave of regions (no -inf lane); A % 128 != 0: no shared words anywhere, the clamped tail loads"),
    "g_a2304": ((36, 256, 64, 32, 2304, 203),
                "beam 8: 4 A 8 bytes of dec_ctx rows exceed the grouped scores kernel's LDS limit (and the 64 KB a launch may ask for without "
                "an opt-in: without the limit the launch is refused), so scores go per row while the context stays grouped; beam 5: both "
                "grouped; a third c0 pass"),
}
# XE cases (captions of 22..30 tokens): seeds at which no kept attention pre-activation lies within fp32 rounding of zero in float64
# (relu_band_count; tests/test_cpu_attention_geometry.py).  Such an element switching its relu moves the embedding rows of the one or two
# tokens that caption was fed beyond check_grads_against_float64 (g_r17 at seed 793: z[22, 0, 0, 727] = -2.9e-8; switched on in float64 it
# moves rows 93 and 58 by 7.17e-4 and 3.2e-4 of the maximum, the device's figures).  g_a2304 has 29 million pre-activations per pass and
# always a few in that band; there the 203 embedding rows get the rule's own judgement.
ATT_XE_SEEDS = {"g_r1": 751, "g_r2": 752, "g_r17": 816, "g_r33": 754, "g_r63": 783, "g_r64": 786, "g_a2304": 827}
ATT_XE_LENGTHS = (22, 30)
ATT_SEEDS = {"g_r1": 701, "g_r2": 702, "g_r17": 743, "g_r33": 704, "g_r63": 715, "g_r64": 736, "g_a2304": 777}


def att_branches(dims, steps=ATT_STEPS):
    """{branch condition of the attention kernels: bool} for dims = (R, D, H, E, A, V) -- the conditions the code of csrc/butd_kernels.h,
    Butd::step and Butd::bptt decides on, written out on the host"""
    R_, D_, _, _, A_, _ = dims
    slots = ATT_PARTS * 4                             # (part, wave) pairs of att_scores_kernel's grid
    return {"scores: a wave holds more than one region": R_ > slots,
            "scores: second group of regions (R > parts x waves x NB)": R_ > slots * ATT_NB,
            "ctx: odd R, the halves (R + 1) / 2 and R / 2 differ": R_ % 2 == 1,
            "ctx: empty upper half": R_ - (R_ + 1) // 2 == 0,
            "softmax: lanes >= R padded with -inf": R_ < 64,
            "scores / denc: second 1024-column pass": A_ > 1024,
            "loads clamped with min(c, A - 4)": A_ % 256 != 0,
            "ctx / dalpha: more than one 512-column part of D": D_ > 512,
            "ctx / dalpha: last column part partly filled": D_ % 512 != 0,
            "denc: second time pass (T > TT)": steps > TT,
            "grouped scores dropped at beam 8, grouped context kept": 4 * A_ * ATT_CTX_MAX_G > ATT_GROUP_LDS,
            "Philox words shared in scores and ddec (A % 256 == 0)": A_ % 256 == 0,
            "Philox words shared in denc (A % 128 == 0)": A_ % 128 == 0}


def att_geometry_claims(name):
    """{claim: bool} -- what ATT_GEOMETRY[name] is there for, as predicates on its numbers and on ATT_PARTS, TT, ATT_CTX_MAX_G"""
    (R_, D_, H_, E_, A_, V_), _ = ATT_GEOMETRY[name]
    Rh = (R_ + 1) // 2
    slots = ATT_PARTS * 4
    base = {"accepted by icz_butd_create": 1 <= R_ <= 64 and all(x % 4 == 0 for x in (D_, H_, E_, A_)) and V_ > 3,
            "two time passes of denc": TT < ATT_STEPS <= 2 * TT}
    if name == "g_r1":
        own = {"one region": R_ == 1, "upper half of att_ctx_kernel empty": Rh == R_}
    elif name == "g_r2":
        own = {"one region per half": Rh == 1 and R_ - Rh == 1,
               "A below one 32-bit keep word": A_ < 32,
               "one partly filled column part": D_ < 512}
    elif name == "g_r17":
        own = {"second c0 pass, shorter than the first": 1024 < A_ < 2048,
               "shared words in scores, ddec and denc": A_ % 256 == 0,
               "R = (part, wave) slots + 1": R_ == slots + 1}
    elif name == "g_r33":
        own = {"denc on shared words": A_ % 128 == 0,
               "scores and ddec per element": A_ % 256 != 0,
               "odd R": R_ % 2 == 1 and Rh != R_ - Rh}
    elif name == "g_r63":
        own = {"second region group of att_scores_kernel": R_ > slots * ATT_NB,
               "one lane of -inf": 64 - R_ == 1,
               "a column part of one float4": D_ % 512 == 4,
               "smallest width with shared words in scores and ddec": A_ == 256}
    elif name == "g_r64":
        own = {"a full wave of regions": R_ == 64,
               "no shared words": A_ % 128 != 0,
               "clamped tail loads inside the first 256-column strip": A_ % 256 != 0 and A_ < 256,
               "a column part of one float4": D_ % 512 == 4}
    elif name == "g_a2304":
        own = {"beam 8: scores per row": 4 * A_ * 8 > ATT_GROUP_LDS,
               "beam 8: the grouped request would be above the 64 KB of a launch without opt-in": 4 * A_ * 8 > 64 * 1024,
               "beam 8: context grouped": 8 <= ATT_CTX_MAX_G,
               "beam 5: both grouped": 4 * A_ * 5 <= ATT_GROUP_LDS,
               "a third c0 pass": A_ > 2048 and A_ % 256 == 0}
    else:
        raise KeyError(name)
    return dict(base, **own)


def _ragged_captions(B, V_, seed, length_range=(5, 14)):
    """B captions of 5 .. 14 tokens (or of length_range = (shortest, longest)), sorted by length (descending): (captions [B, L] int64, lengths)"""
    rs = np.random.RandomState(seed)
    lengths = sorted(rs.randint(length_range[0], length_range[1] + 1, size=B).tolist(), reverse=True)
    caps = torch.zeros(B, max(lengths) + 1, dtype=torch.int64)
    for b, n in enumerate(lengths):
        caps[b, 0] = 1
        caps[b, 1:n] = torch.from_numpy(rs.randint(4, V_, size=n - 1))
        caps[b, n] = 2
    return caps, lengths


def _butd_xe_inputs(dims, B, seed, train=False, length_range=(5, 14), device="cuda"):
    """the inputs of _butd_xe_case, every value from CPU generators: (params on `device`, features, captions, lengths, the upstream
    gradient G of via = "dlogits", the keep-masks em / am / om [T, B, ...] of training mode or None)"""
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    R_, D_, H_, E_, A_, V_ = dims
    params = random_butd_params(R_, D_, H_, E_, A_, V_, device, seed=seed)
    params["predict.weight_g"].mul_(6.0)
    g = torch.Generator(device="cpu")
    g.manual_seed(2000 + seed)
    feats = torch.relu(torch.randn(B, R_, D_, generator=g))
    caps, lengths = _ragged_captions(B, V_, seed, length_range)
    G = torch.randn(sum(lengths), V_, generator=g) / sum(lengths)
    em = am = om = None
    if train:
        rs, T_ = np.random.RandomState(seed + 1), max(lengths)
        em, am, om = rs.rand(T_, B, E_) < 0.5, rs.rand(T_, B, R_, A_) < 0.5, rs.rand(T_, B, H_) < 0.5
    return params, feats, caps, lengths, G, em, am, om


def relu_band_count(feats64, p64, h1_steps, att_masks, active_rows, tol=2e-7):
    """how many kept attention pre-activations z[t, b, r, a] = enc_ctx + dec_ctx_t (float64) lie within `tol` x (|enc_ctx| + |dec_ctx| + 1)
    of zero: two fp32 evaluations can disagree about the sign of such an element, and its relu switching moves EVERY gradient behind
    step t of row b by a finite amount -- among them the embedding rows of the few tokens that row was fed, which no rule excuses"""
    from oracle import butd as ob
    n = 0
    with torch.no_grad():
        enc = feats64 @ ob.wn_weight(p64, "atten.enc_att").t() + p64["atten.enc_att.bias"]
        w_dec, b_dec = ob.wn_weight(p64, "atten.dec_att"), p64["atten.dec_att.bias"]
        for t, h1 in enumerate(h1_steps):
            dec = (h1 @ w_dec.t() + b_dec).unsqueeze(1)
            near = (enc + dec).abs() <= tol * (enc.abs() + dec.abs() + 1.0)
            if att_masks is not None:
                near &= torch.as_tensor(att_masks[t]).reshape(near.shape)
            near[active_rows[t]:] = False
            n += int(near.sum())
    return n


def _butd_xe_case(dims, B, seed, via="loss", options=None, train=False, length_range=(5, 14)):
    """Teacher-forced XE forward (evaluation mode, ragged caption lengths: the batch shrinks with t) + backward at the widths `dims`
    against the fp32 / float64 oracle: packed logits 2e-4 / 1e-4 (as the 49-region full-width test), loss 1e-4, every gradient under
    check_grads_against_float64.  via: "loss" = xe_backward with label smoothing 0.1; "callback" = the same with a gradient callback set
    (phases as separate calls, stages 0, 1, 2 in order); "dlogits" = xe_backward_dlogits for a random upstream gradient G, the oracle's
    loss being sum(logits * G).  train: training mode with explicit embedding / attention / output keep-masks [T, B, ...], the same
    masks in the oracle's forward_xe.  length_range: the shortest and the longest caption."""
    from oracle import butd as ob
    from simpleimagecaptionzoo_amd.butd import ButdHandle, make_rng
    R_, D_, H_, E_, A_, V_ = dims
    params, feats, caps, lengths, G, em, am, om = _butd_xe_inputs(dims, B, seed, train, length_range)
    h = ButdHandle(R_, D_, H_, E_, A_, V_, B, 20)
    h.bind(params)
    for name, value in (options or {}).items():
        h.set_option(name, value)
    order = ob.packed_order(lengths)
    tgt = torch.tensor([int(caps[b, t + 1]) for b, t in order])
    stages = []
    if via == "callback":
        h.set_grad_callback(stages.append)
    rng = make_rng(0, None, *(torch.tensor(m.astype(np.uint8), device="cuda") for m in (em, am, om))) if train else None
    logits = h.xe_forward(feats.cuda(), caps.cuda(), lengths, rng, train=train, want_logits=True)
    grads = h.new_grads()
    if via == "dlogits":
        h.xe_backward_dlogits(G.cuda(), grads)
        loss = None
    else:
        loss = h.xe_backward(grads, smoothing=0.1).item()
    torch.cuda.synchronize()
    if via == "callback":
        assert stages == [0, 1, 2], stages
        h.set_grad_callback(None)
    gsets, trace64, p64 = {}, None, None
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            p = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in params.items()}
            trace = {}
            w_logits = ob.forward_xe(feats.to(dt), caps, lengths, p, em, am, om, trace=trace)
            w_loss = (w_logits * G.to(dt)).sum() if via == "dlogits" else ob.label_smoothing_loss(w_logits, tgt, 0.1)
            w_loss.backward()
            gsets[name] = {k: v.grad.numpy() for k, v in p.items()}
            if name == "f32":
                np.testing.assert_allclose(logits.cpu().numpy(), w_logits.detach().numpy(), atol=2e-4, rtol=1e-4)
                if loss is not None:
                    assert abs(loss - float(w_loss.item())) < 1e-4, (loss, float(w_loss.item()))
            else:
                trace64, p64 = trace, {k: v.detach() for k, v in p.items()}
        finally:
            torch.set_default_dtype(torch.float32)
    kink = attention_kink_units(feats.double(), p64, trace64["h1"], am, active_rows=[sum(l > t for l in lengths) for t in range(max(lengths))])
    rep = check_grads_against_float64(grads, gsets["f32"], gsets["f64"], {"atten.enc_att": kink, "atten.dec_att": kink})
    h.close()
    return rep, kink


def _device_scst_runs(dims, B, T, seed, schedule):
    """Device only: one handle, one SCST step (rollouts with Philox dropout / draws from `seed`, REINFORCE backward with a fixed random
    reward) once per entry of `schedule` = [{handle option: value}, ...], options applied in front of the run and kept for the next.
    Returns per run (greedy ids, sampled ids, log-probs, {name: gradient}) as CPU tensors."""
    from simpleimagecaptionzoo_amd.butd import ButdHandle, make_rng
    R_, D_, H_, E_, A_, V_ = dims
    params = _full_params(seed=seed, dims=dims)
    h = ButdHandle(R_, D_, H_, E_, A_, V_, max(B, 8), T)
    h.bind(params)
    g = torch.Generator(device="cpu")
    g.manual_seed(3000 + seed)
    feats = torch.relu(torch.randn(B, R_, D_, generator=g)).cuda()
    rw = torch.randn(B, 1, generator=g).repeat(1, T).cuda()
    runs = []
    for opts in schedule:
        for name, value in opts.items():
            if name == "graphs":
                h.enable_graphs(bool(value))
            else:
                h.set_option(name, value)
        greedy, seq, lp = h.rollouts(feats, T, make_rng(seed))
        grads = h.new_grads()
        for v in grads.values():
            v.fill_(float("nan"))                   # every element is written by the backward, none accumulated
        h.sample_backward(rw, grads)
        torch.cuda.synchronize()
        runs.append((greedy.cpu().clone(), seq.cpu().clone(), lp.cpu().clone(), {k: v.cpu().clone() for k, v in grads.items()}))
    h.close()
    return runs


# ---- AoA and NIC between the golden widths and the benchmark width ------------------------------------------------------------------
# The bodies of test_fullsize_aoa_scst_step_64x20_matches_oracle and test_nic_config1_size_matches_oracle with the dimensions as an
# argument (those two tests call them with their own sizes, seeds and rules), the XE cases beside them, and the tables of widths of
# tests/test_gpu_aoa_midwidth.py / tests/test_gpu_nic_midwidth.py.
AOA_ZERO_GRAD = ("decoder.aoa_block.linear_K.bias",)      # identically zero (shift invariance of a softmax row): rounding noise in any evaluation
MID_EXCUSED = 2                                           # excused rows per case, greedy and sampled each


class _oracle_heads:
    """oracle.aoa with the case's head count (as test_aoa_random_shapes_match_oracle sets it), restored on exit"""

    def __init__(self, NH):
        self.NH = NH

    def __enter__(self):
        from oracle import aoa as oa
        self.oa, self.old = oa, oa.NH
        oa.NH = self.NH
        return oa

    def __exit__(self, *exc):
        self.oa.NH = self.old
        return False


def _aoa_model(dims, max_batch, seed, jitter_on="cpu"):
    """A seeded AoADetection_Captioner of dims = (R, D, Hd, E, V, NH): predict.weight_g x 6 (trained decoders are far from uniform), the six
    refiner layers made to differ (clones() starts them identical).  jitter_on = "cpu": every value comes from the CPU generator, so the
    oracle alone can be run on the same model without a GPU; "cuda": the layers are perturbed on the device (the full-width case)."""
    from simpleimagecaptionzoo_amd.aoa import AoADetection_Captioner
    R_, D_, Hd, E_, V_, NH = dims
    torch.manual_seed(seed)
    cap = AoADetection_Captioner(V_, NH, Hd, E_, num_regions=R_, enc_dim=D_, max_batch=max_batch, max_beam=1)
    if jitter_on == "cuda":
        cap = cap.cuda()
    with torch.no_grad():
        cap.decoder.predict.weight_g.mul_(6.0)
        for l in cap.aoa_refine.aoa_layers:
            for p_ in l.parameters():
                p_.add_(torch.randn_like(p_) * 0.01)
    return cap


def _aoa_scst_inputs(dims, B, T, s_feats, s_masks):
    """features, keep-masks of every dropout site (the layouts of icz_aoa_rng), uniforms [T, B] and the generator behind them"""
    R_, D_, Hd, E_, V_, NH = dims
    g = torch.Generator(device="cpu")
    g.manual_seed(s_feats)
    feats_c = torch.relu(torch.randn(B, R_, D_, generator=g))
    rs = np.random.RandomState(s_masks)
    keep = lambda shape, p: (rs.rand(*shape) >= p)
    masks = {"proj": keep((B, R_, Hd), 0.5), "ref_att": keep((6, B, NH, R_, R_), 0.1), "ref_aoa": keep((6, B, R_, 2 * Hd), 0.3),
             "ref_sc": keep((6, B, R_, Hd), 0.1), "emb": keep((T, B, E_), 0.5), "ctx": keep((T, B, Hd), 0.5),
             "att": keep((T, B, NH, R_), 0.1), "out": keep((T, B, Hd), 0.5)}
    u = rs.rand(T, B).astype(np.float32)
    return feats_c, masks, u, rs


def _aoa_scst_oracle(oa, sd, feats_c, masks, u, T):
    """the oracle's sampled rollout in fp32 (the reference's arithmetic: ids, log-probs, loss) and in float64 (the truth the gradients
    are held to), gradients for the decoder only (the only parameters in the reference's optimizer, AoA_Model.py:669-674):
    {"f32" / "f64": (params, seq, logprobs, logits [B, T, V])}"""
    runs = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            pp = {k: v.detach().cpu().to(dt).requires_grad_(k.startswith("decoder.")) for k, v in sd.items()}
            lg = []
            seq, lp = oa.sample_rl(feats_c.to(dt), pp, u.astype(np.float64), masks, T, early_exit=False, hoisted=True, logits_out=lg)
            runs[name] = (pp, seq, lp, torch.stack(lg, 1))
        finally:
            torch.set_default_dtype(torch.float32)
    return runs


def _aoa_scst_case(dims, B, T, seed, options=None, with_reward=False, seeds=None, jitter_on="cpu", sampled_rule="cdf"):
    """One whole AoADetection SCST step of B rows x T steps at dims = (R, D, Hd, E, V, NH): refiner in evaluation and in training mode
    (all four dropout sites of the six layers injected), greedy and sampled rollout as the two concurrent chains
    (icz_aoa_scst_rollouts), REINFORCE loss and the decoder gradients -- against the CPU oracle on the same features / parameters /
    uniforms / keep-masks.  Greedy ids exact up to MID_EXCUSED near-ties; sampled ids exact up to MID_EXCUSED draws at a CDF edge
    (sampled_rule "cdf": _excuse_sampled; "neighbour": the full-width test's rule, the device's token at most two ids from the
    oracle's); log-probs 1e-4 on the agreeing rows, loss 1e-4, gradients under check_grads_against_float64.  with_reward: the CIDEr-D
    reward on the device, bit-exact on the ids the device produced, as the REINFORCE reward.  seeds = (model, features, masks)
    overrides the seeds derived from `seed`."""
    from oracle import butd as ob
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    R_, D_, Hd, E_, V_, NH = dims
    s_model, s_feats, s_masks = seeds or (seed, 1000 + seed, seed)
    cap = _aoa_model(dims, B, s_model, jitter_on).cuda()
    h = cap._handle()
    for name, value in (options or {}).items():
        h.set_option(name, value)
    feats_c, masks, u, rs = _aoa_scst_inputs(dims, B, T, s_feats, s_masks)
    feats = feats_c.cuda()
    dev = "cuda"
    rng = make_aoa_rng(0, torch.tensor(u, device=dev), {k: torch.tensor(v.astype(np.uint8), device=dev) for k, v in masks.items()})
    greedy, seq, lp = h.rollouts(feats, T, rng)
    greedy, seq, lp = greedy.cpu().numpy(), seq.cpu().numpy(), lp.cpu().numpy()
    with _oracle_heads(NH) as oa:
        runs = _aoa_scst_oracle(oa, cap.state_dict(), feats_c, masks, u, T)
        p, w_seq, w_lp, w_slog = runs["f32"]
        with torch.no_grad():
            w_greedy, w_glog = oa.greedy(feats_c, p, T, hoisted=True)
    _excuse_greedy(greedy, w_greedy, w_glog, MID_EXCUSED)
    if sampled_rule == "cdf":
        same = _excuse_sampled(seq, w_seq, w_slog, u, MID_EXCUSED)
    else:
        sdiv = _first_divergence(seq, w_seq.numpy())
        assert (sdiv >= 0).sum() <= MID_EXCUSED, "sampled: %d rows differ" % int((sdiv >= 0).sum())
        for b in np.nonzero(sdiv >= 0)[0]:              # a draw within fp32 rounding of a CDF boundary lands on the neighbouring token
            assert abs(int(seq[b, sdiv[b]]) - int(w_seq[b, sdiv[b]])) <= 2, (b, seq[b], w_seq[b])
        same = sdiv < 0
    ok = same & (runs["f64"][1].numpy() == seq).all(1)
    assert ok.sum() >= B - 2 * MID_EXCUSED
    np.testing.assert_allclose(lp[ok], w_lp.detach().numpy()[ok], atol=1e-4)
    rw = np.zeros((B, T), dtype=np.float32)
    if with_reward:                                     # bit-exact on the ids the device produced
        from oracle import ciderd as oc
        from simpleimagecaptionzoo_amd.ciderd import CiderDReward
        from simpleimagecaptionzoo_amd.synth import document_frequency, synthetic_references
        from simpleimagecaptionzoo_amd.vocab import synthetic_vocab
        vocab = synthetic_vocab(V_)
        words = [vocab.ix2word[i] for i in range(V_)]
        dfd = document_frequency(synthetic_references(2000, words, seed=0))
        refs = synthetic_references(B, words, seed=9)
        gts = {i: refs[i] for i in range(B)}
        scorer = CiderDReward(dfd["document_frequency"], dfd["ref_len"], vocab.word2ix, dev)
        reward = scorer.reward(torch.tensor(seq, device=dev), torch.tensor(greedy, device=dev), gts, list(range(B)))
        w_reward = oc.self_critical_reward(seq, greedy, gts, list(range(B)), dict(enumerate(words)),
                                           oc.DocFreq(dfd["document_frequency"], dfd["ref_len"]))
        assert np.array_equal(reward.cpu().numpy(), w_reward)
        rw = w_reward.copy()
        rw[~ok] = 0.0
    rw = rw + rs.randn(B, 1).astype(np.float32) * ok[:, None].astype(np.float32)
    grads = h.new_grads()
    loss, msum = h.sample_backward(torch.tensor(rw, device=dev), grads)
    gsets = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            pp, ws, wl, _ = runs[name]
            w_seq_m = torch.from_numpy(np.where(ok[:, None], ws.numpy(), seq))
            w_loss = ob.reward_criterion(wl, w_seq_m, torch.from_numpy(rw).to(dt))
            w_loss.backward()
            gsets[name] = {k: v.grad.numpy() for k, v in pp.items() if v.grad is not None}
            if name == "f32":
                assert abs(loss.item() - w_loss.item()) < 1e-4, (loss.item(), w_loss.item())
        finally:
            torch.set_default_dtype(torch.float32)
    return check_grads_against_float64(grads, gsets["f32"], gsets["f64"], None, skip=AOA_ZERO_GRAD)


def _aoa_xe_case(dims, B, seed, train_refiner=False):
    """Teacher-forced XE step of the AoA decoder at dims = (R, D, Hd, E, V, NH) on ragged caption lengths (the batch shrinks with t),
    label smoothing 0.1.  Default: evaluation mode against the fp32 / float64 oracle -- packed logits 2e-4 / 1e-4 and loss 1e-4 (as
    _butd_xe_case), the decoder gradients under check_grads_against_float64.  train_refiner: training mode with every dropout site
    injected and the option "train_refiner" on -- the loss (1e-4) and all 82 gradient tensors against autograd over the float64 oracle
    under the bound of tests/test_gpu_aoa_refiner_train.py (2e-4 of each tensor's maximum).  Returns {tensor: error / scale}."""
    import _aoa_refiner as ar
    from oracle import butd as ob
    R_, D_, Hd, E_, V_, NH = dims
    cap = _aoa_model(dims, B, seed).cuda()
    cap.train_refiner = bool(train_refiner)
    sd = {k: v.detach().cpu().clone() for k, v in cap.state_dict().items()}
    h = cap._handle()
    g = torch.Generator(device="cpu")
    g.manual_seed(2000 + seed)
    feats = torch.relu(torch.randn(B, R_, D_, generator=g))
    caps, lengths = _ragged_captions(B, V_, seed)
    tgt = torch.tensor([int(caps[b, t + 1]) for b, t in ob.packed_order(lengths)])
    if train_refiner:
        cfg = (B, R_, D_, Hd, E_, V_, NH, max(lengths), None, None)
        masks, _ = ar.masks_of(cfg, seed + 1)
        h.xe_forward(feats.cuda(), caps.cuda(), lengths, ar.device_rng(masks), True)
        grads = h.new_grads()
        loss = h.xe_backward(grads, 0.1).item()
        w_loss, want = ar.oracle_xe(cfg, sd, feats, caps, lengths, masks)
        assert abs(loss - w_loss) < 1e-4, (loss, w_loss)
        assert len(grads) == 82 and set(grads) == set(want)
        rep = {}
        for k, v in grads.items():
            scale = max(1e-3, float(np.abs(want[k]).max()))
            err = float(np.abs(v.cpu().double().numpy() - want[k]).max())
            rep[k] = err / scale
            assert err <= 2e-4 * scale + 2e-6, (k, err, scale)
        return rep
    logits = h.xe_forward(feats.cuda(), caps.cuda(), lengths, None, train=False, want_logits=True)
    grads = h.new_grads()
    loss = h.xe_backward(grads, 0.1).item()
    gsets = {}
    with _oracle_heads(NH) as oa:
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            torch.set_default_dtype(dt)
            try:
                p = {k: v.detach().clone().to(dt).requires_grad_(k.startswith("decoder.")) for k, v in sd.items()}
                w_logits = oa.forward_xe(feats.to(dt), caps, lengths, p)
                w_loss = ob.label_smoothing_loss(w_logits, tgt, 0.1)
                w_loss.backward()
                gsets[name] = {k: v.grad.numpy() for k, v in p.items() if v.grad is not None}
                if name == "f32":
                    print("xe", dims, "logits max|err|", float((logits.cpu() - w_logits.detach()).abs().max()), "loss", loss, float(w_loss.detach()))
                    np.testing.assert_allclose(logits.cpu().numpy(), w_logits.detach().numpy(), atol=2e-4, rtol=1e-4)
                    assert abs(loss - float(w_loss.item())) < 1e-4, (loss, float(w_loss.item()))
            finally:
                torch.set_default_dtype(torch.float32)
    rep = check_grads_against_float64(grads, gsets["f32"], gsets["f64"], None, skip=AOA_ZERO_GRAD)
    return {k: v[0] for k, v in rep.items()}


def _aoa_device_scst_runs(dims, B, T, seed, schedule):
    """Device only (as _device_scst_runs): one AoA handle, one SCST step (Philox dropout / draws from `seed`, fixed reward) once per
    entry of `schedule`; per run (greedy ids, sampled ids, log-probs, loss, {name: gradient}) as CPU tensors."""
    from simpleimagecaptionzoo_amd.aoa import make_aoa_rng
    R_, D_, Hd, E_, V_, NH = dims
    cap = _aoa_model(dims, B, seed).cuda()
    h = cap._handle()
    g = torch.Generator(device="cpu")
    g.manual_seed(3000 + seed)
    feats = torch.relu(torch.randn(B, R_, D_, generator=g)).cuda()
    rw = torch.randn(B, 1, generator=g).repeat(1, T).cuda()
    runs = []
    for opts in schedule:
        for name, value in opts.items():
            if name == "graphs":
                h.enable_graphs(bool(value))
            else:
                h.set_option(name, value)
        greedy, seq, lp = h.rollouts(feats, T, make_aoa_rng(seed))
        grads = h.new_grads()
        for v in grads.values():
            v.fill_(float("nan"))                   # every element is written by the backward, none accumulated
        loss, _ = h.sample_backward(rw, grads)
        torch.cuda.synchronize()
        runs.append((greedy.cpu().clone(), seq.cpu().clone(), lp.cpu().clone(), loss.cpu().clone(), {k: v.cpu().clone() for k, v in grads.items()}))
    return runs


def _nic_inputs(dims, B, T, s_par, s_feats, s_masks, sharpen, device):
    from simpleimagecaptionzoo_amd.synth import random_nic_params
    E_, H_, V_ = dims
    params = random_nic_params(E_, H_, V_, device, seed=s_par)
    if sharpen != 1.0:
        params["predict.weight_g"].mul_(sharpen)
    g = torch.Generator(device="cpu")
    g.manual_seed(s_feats)
    feats_c = torch.randn(B, E_, generator=g)
    rs = np.random.RandomState(s_masks)
    om = rs.rand(T, B, H_) < 0.5
    u = rs.rand(T, B).astype(np.float32)
    return params, feats_c, om, u, rs


def _nic_grad_bound(grads, want):
    """NIC's gradient bound (tests/test_gpu_nic.py): 2e-4 of each tensor's maximum against the fp32 oracle"""
    rep = {}
    for k, gt in grads.items():
        w = want[k]
        scale = max(1e-6, float(np.abs(w).max()))
        err = float(np.abs(gt.cpu().numpy() - w).max())
        rep[k] = err / scale
        assert err <= 2e-4 * scale + 1e-7, (k, err, scale)
    return rep


def _nic_scst_case(dims, B, T, seed, sharpen=1.0, seeds=None, limit=MID_EXCUSED, sampled_rule="cdf"):
    """NIC decoder at dims = (E, H, V), B rows x T steps: greedy ids exact up to `limit` near-ties, sampled ids exact up to `limit` draws
    at a CDF edge (sampled_rule "cdf": _excuse_sampled; "count": the config-1 test's rule, the differing rows counted only), log-probs
    1e-4, loss 1e-4, REINFORCE gradients 2e-4 (NIC_Model.py:100-151).  seeds = (parameters, features, masks) overrides the seeds derived
    from `seed`."""
    from oracle import butd as ob
    from oracle import nic as onic
    from simpleimagecaptionzoo_amd.butd import make_rng
    from simpleimagecaptionzoo_amd.nic import NicHandle
    E_, H_, V_ = dims
    s_par, s_feats, s_masks = seeds or (seed, 1000 + seed, seed)
    params, feats_c, om, u, rs = _nic_inputs(dims, B, T, s_par, s_feats, s_masks, sharpen, "cuda")
    h = NicHandle(E_, H_, V_, B, T)
    h.bind(params)
    feats = feats_c.cuda()
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in params.items()}
    ids = h.greedy(feats, T).cpu().numpy()
    with torch.no_grad():
        w_ids, w_glog = onic.greedy(feats_c, p, T)
    _excuse_greedy(ids, w_ids, w_glog, limit)
    rng = make_rng(0, torch.tensor(u, device="cuda"), None, None, torch.tensor(om.astype(np.uint8), device="cuda"))
    seq, lp = h.sample(feats, T, rng)
    seq, lp = seq.cpu().numpy(), lp.cpu().numpy()
    lg = []
    w_seq, w_lp = onic.sample_rl(feats_c, p, u.astype(np.float64), om, T, early_exit=False, logits_out=lg)
    if sampled_rule == "cdf":
        ok = _excuse_sampled(seq, w_seq, torch.stack(lg, 1), u, limit)
    else:
        sdiv = _first_divergence(seq, w_seq.numpy())
        assert (sdiv >= 0).sum() <= limit
        ok = sdiv < 0
    np.testing.assert_allclose(lp[ok], w_lp.detach().numpy()[ok], atol=1e-4)
    rw = (rs.randn(B, 1).astype(np.float32) * ok[:, None]).repeat(T, 1)
    grads = h.new_grads()
    loss, _ = h.sample_backward(torch.tensor(rw, device="cuda"), grads)
    w_loss = ob.reward_criterion(w_lp, torch.from_numpy(np.where(ok[:, None], w_seq.numpy(), seq)), torch.from_numpy(rw))
    w_loss.backward()
    assert abs(loss.item() - w_loss.item()) < 1e-4
    rep = _nic_grad_bound(grads, {k: v.grad.numpy() for k, v in p.items()})
    h.close()
    return rep


def _nic_xe_case(dims, B, seed, sharpen=1.0):
    """NIC teacher-forced XE step (training mode, explicit output-dropout masks) at dims = (E, H, V) on ragged caption lengths, label
    smoothing 0.1, against the fp32 oracle: packed logits 2e-4 / 1e-4, loss 1e-4 (tests/test_gpu_nic.py), the decoder gradients and the
    gradient w.r.t. the image embedding 2e-4 of each tensor's maximum."""
    from oracle import butd as ob
    from oracle import nic as onic
    from simpleimagecaptionzoo_amd.butd import make_rng
    from simpleimagecaptionzoo_amd.nic import NicHandle
    E_, H_, V_ = dims
    caps, lengths = _ragged_captions(B, V_, seed)
    T = max(lengths)
    params, feats_c, om, _, _ = _nic_inputs(dims, B, T, seed, 2000 + seed, seed + 1, sharpen, "cuda")
    h = NicHandle(E_, H_, V_, B, 20)
    h.bind(params)
    rng = make_rng(0, None, None, None, torch.tensor(om.astype(np.uint8), device="cuda"))
    logits = h.xe_forward(feats_c.cuda(), caps.cuda(), lengths, rng, True, True)
    grads = h.new_grads()
    loss, dfe = h.xe_backward(grads, 0.1, want_dfeats=True)
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in params.items()}
    f = feats_c.clone().requires_grad_(True)
    w_logits = onic.forward_xe(f, caps, lengths, p, om)
    tgt = torch.tensor([int(caps[b, t + 1]) for b, t in ob.packed_order(lengths)])
    w_loss = ob.label_smoothing_loss(w_logits, tgt, 0.1)
    w_loss.backward()
    print("nic xe", dims, "logits max|err|", float((logits.cpu() - w_logits.detach()).abs().max()), "loss", loss.item(), float(w_loss.detach()))
    np.testing.assert_allclose(logits.cpu().numpy(), w_logits.detach().numpy(), atol=2e-4, rtol=1e-4)
    assert abs(loss.item() - float(w_loss.item())) < 1e-4, (loss.item(), float(w_loss.item()))
    want = {k: v.grad.numpy() for k, v in p.items()}
    rep = _nic_grad_bound(dict(grads, dfeats=dfe), dict(want, dfeats=f.grad.numpy()))
    h.close()
    return rep


# name -> (dims = (R, D, Hd, E, V, NH), [(rows, steps, kind)], purpose); seeds in AOA_SEEDS.  Where a number differs from the starting set
# of the issue that asked for these widths, the purpose says why.  aoa_midwidth_routes states each purpose as host predicates.
AOA_MIDWIDTH = {
    "a256": ((36, 1024, 256, 192, 2051, 4), [(48, 8, "scst"), (16, 8, "scst")],
             "head width 64 with 4 heads on the matrix-pipe attention; gates N = 1024: every decoder-step product on the fp32-MFMA kernels; odd "
             "V; 16 rows on the 16-row tiles (the 32-row tiles are a336's)"),
    "a336": ((49, 512, 336, 160, 1237, 6), [(20, 8, "scst")],
             "head width 56: the blocked attention with a padded pitch (60) and d / 4 = 14; Hd and E no multiples of 64; 4 Hd no multiple of "
             "128 (the split-precision NN / NT kernels refuse); 49 regions; 20 rows on the 32-row tiles; self-attention tiles just under 48 KB"),
    "a512": ((36, 2048, 512, 512, 3000, 8), [(64, 8, "scst")],
             "head width 64 on the matrix-pipe kernel (one j0 trip) with 8 heads; the first width with the gates on the resident kernel; the AoA "
             "linear (N = 1024) below it on the fp32 kernel; LSTM and AoA-linear weight gradients on split-K slabs"),
    "a640": ((36, 2048, 640, 512, 5000, 10), [(64, 8, "scst")],
             "the resident kernel's four-stage form (E = 512, not 384: 6 + 10 + 10 stages are no multiple of 4 and the resident kernel would "
             "refuse the gates); Hd % 256 != 0: neither weight-gradient group taken; E != Hd; 10 heads"),
    "a768": ((49, 2048, 768, 512, 5000, 8), [(64, 8, "scst"), (100, 4, "scst")],
             "head width 96: the blocked attention at a large width, above the 48 KB opt-in; 512-deep resident form; 100 rows on the 128-row "
             "resident kernel; the LSTM group taken with column groups 512, 768, 768 -- the AoA-linear group is not (12 x 12 tiles of 128: "
             "only Hd >= 1024 fills 256), its two products stay separate TN launches"),
    "a1024h4": ((36, 2048, 1024, 1024, 3000, 4), [(40, 6, "scst")],
                "head width 256: four j0 trips of the matrix-pipe kernel; the decoder attention's K / V tiles above 48 KB (the opt-in of "
                "aoa_dec_attn_kernel); gates and AoA linear both on the 512-deep resident form at 40 rows"),
}
AOA_SEEDS = {"a256": 411, "a336": 412, "a512": 413, "a640": 414, "a768": 415, "a1024h4": 416}


def aoa_pitch(n):
    """csrc/aoa_kernels.h:152 aoa_pitch"""
    n4 = (n + 3) // 4
    return 4 * (n4 + 1 if n4 % 2 == 0 else n4)


def aoa_attention_routes(R_, Hd, NH):
    """The attention choices of csrc/aoa.hip written out: (matrix-pipe self-attention, csrc/aoa.hip:117; bytes of mha_self_kernel's tiles,
    csrc/aoa_impl.h:131-133 with every query row resident; bytes of aoa_dec_attn_kernel's tiles, csrc/aoa.hip:19).  Aoa::init opts in
    above 48 KB (csrc/aoa.hip:20-23)."""
    d, R4 = Hd // NH, (R_ + 3) & ~3
    self_lds = 4 * (2 * R4 * aoa_pitch(d) + R4 * aoa_pitch(d) + R4 * aoa_pitch(R_))
    assert self_lds <= 156 * 1024          # LDS_BUDGET: all queries in one pass (self_qc = R)
    return R_ <= 64 and d % 64 == 0, self_lds, (2 * R_ * (d + 1) + d + 128 + 4) * 4


def aoa_midwidth_routes(name):
    """{claim: bool} -- what AOA_MIDWIDTH[name] is there for, from the library's host-only routing entries and the attention predicates"""
    from simpleimagecaptionzoo_amd.butd import gemm_route_for as route, gemm_tn_grouped_fits as grouped, gemm_tn_split_pick as split
    (R_, D_, Hd, E_, V_, NH), cases, _ = AOA_MIDWIDTH[name]
    B, T, _ = cases[0]
    TB, Vp, d, KB = B * T, (V_ + 63) // 64 * 64, Hd // NH, 48 * 1024
    mfma, self_lds, lds_dec = aoa_attention_routes(R_, Hd, NH)
    gates, lin, pred = route("nt", B, 4 * Hd, [E_, Hd, Hd]), route("nt", B, 2 * Hd, [Hd, Hd]), route("nt", B, Vp, [Hd])
    g_lstm, g_aoa = grouped(4 * Hd, TB, [E_, Hd, Hd]), grouped(2 * Hd, TB, [Hd, Hd])
    if name == "a256":
        B2 = cases[1][0]
        return {"matrix-pipe attention at head width 64, 4 heads": mfma and d == 64 and NH == 4,
                "decoder step on the 64-row fp32-MFMA tiles": gates == lin == pred == route("nt", B, Hd, [Hd]) == "nt_fp32_mt4",
                "16 rows on the 16-row tiles": route("nt", B2, 4 * Hd, [E_, Hd, Hd]) == route("nt", B2, Vp, [Hd]) == "nt_fp32_mt1",
                "odd V": V_ % 2 == 1 and V_ % 64 != 0,
                "no opt-in, no group, no slabs": max(self_lds, lds_dec) <= KB and not g_lstm and not g_aoa and split(4 * Hd, Hd, TB) == 1}
    if name == "a336":
        return {"blocked attention at head width 56 with a padded pitch": not mfma and d == 56 and aoa_pitch(d) == 60 and (d // 4) & (d // 4 - 1) != 0,
                "32-row NT tiles": gates == lin == pred == "nt_fp32_mt2",
                "K % 64 != 0 in the gate segments": Hd % 64 != 0 and E_ % 64 != 0,
                "dgrad over all steps refused by the split-precision NN kernel": route("nn", TB, E_, [4 * Hd], 1) == "nn_fp32" and (4 * Hd) % 128 != 0,
                "49 regions, self-attention tiles under the opt-in": R_ == 49 and self_lds <= KB and lds_dec <= KB}
    if name == "a512":
        return {"matrix-pipe attention at head width 64 (one j0 trip), 8 heads": mfma and d == 64 and NH == 8,
                "gates and vocabulary projection on the resident kernel": gates.startswith("resident") and pred.startswith("resident"),
                "one width below (N = 1984) not": route("nt", B, 4 * 496, [E_, 496, 496]) == "nt_fp32_mt4",
                "AoA linear (N = 1024) on the fp32 kernel": 2 * Hd == 1024 and lin == "nt_fp32_mt4",
                "lstm.weight_hh, AoA-linear and predict weight gradients on slabs": min(split(4 * Hd, Hd, TB), split(2 * Hd, Hd, TB), split(Vp, Hd, TB)) > 1}
    if name == "a640":
        return {"gates on the four-stage resident form": gates == "resident_4stage",
                "with E = 384 the resident kernel refuses": route("nt", B, 4 * Hd, [384, Hd, Hd]) == "nt_fp32_mt4",
                "no group taken (Hd % 256 != 0), E != Hd": Hd % 256 != 0 and not g_lstm and not g_aoa and E_ != Hd,
                "matrix-pipe attention with 10 heads": mfma and NH == 10 and d == 64,
                "lstm.weight_hh and AoA-linear weight gradients on slabs": min(split(4 * Hd, Hd, TB), split(2 * Hd, Hd, TB)) > 1}
    if name == "a768":
        B2, T2, _ = cases[1]
        return {"blocked attention at head width 96 above the opt-in": not mfma and d == 96 and aoa_pitch(d) == 100 and self_lds > KB,
                "decoder attention under the opt-in": lds_dec <= KB,
                "gates on the 512-deep resident form at 64 rows": gates == "resident_512deep",
                "128-row resident kernel at 100 rows": route("nt", B2, 4 * Hd, [E_, Hd, Hd]) == route("nt", B2, Vp, [Hd]) == "resident_128row",
                "LSTM group taken, AoA-linear group not": g_lstm and not g_aoa and Hd % 256 == 0}
    if name == "a1024h4":
        return {"matrix-pipe attention at head width 256 (four j0 trips)": mfma and d == 256,
                "decoder attention above the opt-in": lds_dec > KB,
                "gates, AoA linear and predict on the 512-deep resident form": gates == lin == pred == "resident_512deep",
                "40 rows: more than the 32-row tiles, one resident row block": 32 < B <= 64}
    raise KeyError(name)


# name -> (dims = (E, H, V), [(rows, steps, kind)], purpose); seeds in NIC_SEEDS
NIC_MIDWIDTH = {
    "n336": ((160, 336, 1237), [(20, 8, "scst")],
             "E and H no multiples of 64, 4 H no multiple of 128 (the split-precision NN kernel refuses the dgrad); 20 rows on 32-row tiles"),
    "n640": ((384, 640, 5000), [(64, 8, "scst")],
             "gates on the 512-deep resident form (6 + 10 stages), predict (10 stages) on the fp32 kernel; lstm weight gradients and predict's on slabs"),
    "n768": ((512, 768, 5000), [(64, 8, "scst"), (100, 4, "scst")],
             "gates (8 + 12 stages) and predict (12) on the four-stage resident form; 100 rows on the 128-row resident kernel"),
    "n1024": ((1024, 1024, 3000), [(40, 6, "scst")],
              "the benchmark width at 40 rows: gates and predict on the 512-deep resident form, predict through gemm_predict with two k ranges"),
    "n512r40": ((512, 512, 2543), [(40, 8, "scst")],
                "the single 512-deep k range of gemm_predict at 33..64 rows (EXPERIMENTS.md, round 6), this time against the oracle"),
}
NIC_SEEDS = {"n336": 512, "n640": 514, "n768": 515, "n1024": 516, "n512r40": 517}
NIC_SHARPEN = 1.0


def nic_midwidth_routes(name):
    """{claim: bool} -- what NIC_MIDWIDTH[name] is there for, from the library's host-only routing entries"""
    from simpleimagecaptionzoo_amd.butd import gemm_route_for as route, gemm_tn_grouped_fits as grouped, gemm_tn_split_pick as split
    (E_, H_, V_), cases, _ = NIC_MIDWIDTH[name]
    B, T, _ = cases[0]
    TB, Vp = B * T, (V_ + 63) // 64 * 64
    gates, pred = route("nt", B, 4 * H_, [E_, H_]), route("nt", B, Vp, [H_])
    s_hh, s_ih, s_p = split(4 * H_, H_, TB), split(4 * H_, E_, TB), split(Vp, H_, TB)
    if name == "n336":
        return {"32-row NT tiles": gates == pred == "nt_fp32_mt2",
                "K % 64 != 0": H_ % 64 != 0 and E_ % 64 != 0,
                "dgrad over all steps refused by the split-precision NN kernel": route("nn", TB, E_, [4 * H_], 1) == "nn_fp32" and (4 * H_) % 128 != 0,
                "no weight gradient on slabs": max(s_hh, s_ih, s_p) == 1}
    if name == "n640":
        return {"gates on the 512-deep resident form": gates == "resident_512deep",
                "predict on the fp32 kernel": pred == "nt_fp32_mt4",
                "lstm and predict weight gradients on slabs": min(s_hh, s_ih, s_p) > 1,
                "no group taken": not grouped(4 * H_, TB, [E_, H_])}
    if name == "n768":
        B2, T2, _ = cases[1]
        return {"gates and predict on the four-stage resident form": gates == pred == "resident_4stage",
                "128-row resident kernel at 100 rows": route("nt", B2, 4 * H_, [E_, H_]) == route("nt", B2, Vp, [H_]) == "resident_128row",
                "lstm weight gradients on slabs": min(s_hh, s_ih) > 1}
    if name == "n1024":
        return {"gates and predict on the 512-deep resident form": gates == pred == "resident_512deep",
                "40 rows: 33..64": 32 < B <= 64,
                "predict over two 512-deep k ranges": H_ // 512 == 2}
    if name == "n512r40":
        return {"gates and predict on the 512-deep resident form": gates == pred == "resident_512deep",
                "40 rows: 33..64": 32 < B <= 64,
                "predict is one 512-deep k range": H_ == 512}
    raise KeyError(name)
