"""Shared by tests/test_gpu_butd_adaptive.py and tests/test_cpu_butd_adaptive.py: BUTD over adaptive region sets (icz_butd_set_regions).

The ground truth is oracle.butd run PER IMAGE on feats[i, :counts[i]] (explicit attention masks sliced to [:counts[i]]): an image of a
counted batch must behave exactly as it would alone with its own regions.  Everything here is generated on the CPU, so the oracle side
runs without a GPU; the feature tensors are made once per process and shared (lru_cache), and nobody writes to them."""
import functools

import numpy as np
import torch

CAP = 100                                   # the handle's region capacity and the padded width of the main case
D, H, E, A, V = 132, 64, 32, 256, 203       # D % 512 != 0 (one partial column part), A = one whole 256-column strip (shared Philox bits)
T = 24                                      # more steps than one time pass of att_bwd_denc_kernel<20>
# 1 / 2: one region, an empty upper half; 63 / 64 / 65: the single-lane boundary; 99 / 100: odd and even halves, no padding at all;
# 4 random ones.  12 images: more than merge_small.
MAIN_COUNTS = (1, 2, 10, 63, 64, 65, 99, 100, 37, 81, 23, 52)
MAIN_SEED = 4
SMALL = (0, 5, 7)                           # the images of the 3-image batch (merged chain; sample_n with 4 rows each): counts 1, 65, 100


def params_cpu(seed, R=CAP, sharpen=6.0):
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    p = random_butd_params(R, D, H, E, A, V, "cpu", seed=seed)
    p["predict.weight_g"].mul_(sharpen)
    return p


@functools.lru_cache(maxsize=None)
def batch(seed, counts, regions):
    """the padded features [B, regions, D] of a counted batch, pad rows ZERO"""
    g = torch.Generator(device="cpu")
    g.manual_seed(2000 + seed)
    f = torch.relu(torch.randn(len(counts), regions, D, generator=g))
    for i, c in enumerate(counts):
        f[i, c:] = 0
    return f


def wide_batch(R, n=6):
    """a fixed set of R > 64 regions, no padding (the seed offset: picked so that the reference needs no excuse)"""
    return batch(MAIN_SEED + R + 1000, (R,) * n, R)


def junk_pads(feats, counts, seed=5):
    """the same batch with finite junk (uniform +-100) in the pad rows"""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    out = feats.clone()
    for i, c in enumerate(counts):
        out[i, c:] = (torch.rand(out.shape[1] - c, out.shape[2], generator=g) * 2 - 1) * 100
    return out


def rng_arrays(seed, rows, regions, steps=T):
    """uniforms [T, rows] and the keep-masks em / am / om of `rows` decoder rows (am laid out [T, rows, regions, A])"""
    rs = np.random.RandomState(seed)
    em, am, om = rs.rand(steps, rows, E) < 0.5, rs.rand(steps, rows, regions, A) < 0.5, rs.rand(steps, rows, H) < 0.5
    return rs.rand(steps, rows).astype(np.float32), em, am, om


def _typed(p, dt, grad=False):
    return {k: v.detach().to(dt).clone().requires_grad_(grad) for k, v in p.items()}


def greedy_reference(feats, counts, seed=MAIN_SEED, steps=20):
    """per image, fp32 and float64: (ids [B, steps], alphas [B, steps, regions] zero at r >= c, logits [B, steps, V])"""
    from oracle import butd as ob
    p, regions = params_cpu(seed), feats.shape[1]
    out = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            pp = _typed(p, dt)
            ids, als, lgs = [], [], []
            with torch.no_grad():
                for i, c in enumerate(counts):
                    a, b, l = ob.greedy(feats[i:i + 1, :c].to(dt), pp, steps, hoisted=True)
                    al = torch.zeros(1, steps, regions, dtype=dt)
                    al[:, :, :c] = b
                    ids.append(a), als.append(al), lgs.append(l)
            out[name] = (torch.cat(ids), torch.cat(als), torch.cat(lgs))
        finally:
            torch.set_default_dtype(torch.float32)
    return out


def beam_reference(feats, counts, k, images, seed=MAIN_SEED, steps=20):
    from oracle import butd as ob
    p = params_cpu(seed)
    with torch.no_grad():
        return {i: ob.beam_search(feats[i:i + 1, :counts[i]], p, k, steps).numpy().ravel() for i in images}


def scst_reference(feats, counts, K, reward, arrays, seed=MAIN_SEED):
    """Per decoder row (row = img * K + k attends over image img's valid regions; its masks sliced to them), fp32 and float64:
    {"f32" / "f64": (seq [rows, T], logp, logits, REINFORCE loss over ALL rows, gradients), "kink": attention units with a kept relu
    pre-activation at zero in some row's float64 pass (_fullwidth.attention_kink_units)}."""
    from oracle import butd as ob
    from _fullwidth import attention_kink_units
    p = params_cpu(seed)
    u, em, am, om = arrays
    out, kink = {}, np.zeros(A, bool)
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            pp = _typed(p, dt, True)
            seqs, lps, lgs = [], [], []
            for row in range(len(counts) * K):
                i = row // K
                c = counts[i]
                trace = {}
                s, lp, lg = ob.sample_rl(feats[i:i + 1, :c].to(dt), pp, u[:, row:row + 1].astype(np.float64), em[:, row:row + 1],
                                         am[:, row:row + 1, :c], om[:, row:row + 1], T, early_exit=False, hoisted=True, trace=trace)
                seqs.append(s), lps.append(lp), lgs.append(lg.detach())
                if dt == torch.float64:
                    kink = kink | attention_kink_units(feats[i:i + 1, :c].double(), {k: v.detach() for k, v in pp.items()}, trace["h1"],
                                                       [am[t, row:row + 1, :c] for t in range(T)])
            seq, lp = torch.cat(seqs), torch.cat(lps)
            loss = ob.reward_criterion(lp, seq, torch.as_tensor(reward).to(dt))
            loss.backward()
            out[name] = (seq, lp.detach(), torch.cat(lgs), float(loss.detach()), {k: v.grad.double().numpy() for k, v in pp.items()})
        finally:
            torch.set_default_dtype(torch.float32)
    out["kink"] = kink
    return out


def xe_case(seed, n):
    """ragged captions of n rows, lengths sorted descending (5..14 tokens after <sta>)"""
    rs = np.random.RandomState(300 + seed)
    lengths = sorted((int(x) for x in rs.randint(5, 15, n)), reverse=True)
    caps = np.zeros((n, max(lengths) + 1), np.int64)
    for b, l in enumerate(lengths):
        caps[b, 0] = 1
        caps[b, 1:l] = rs.randint(3, V, l - 1)
        caps[b, l] = 2
    return torch.from_numpy(caps), lengths


def xe_reference(feats, counts, arrays, train, seed=MAIN_SEED):
    """per image: packed logits in pack_padded_sequence order, label-smoothing loss over the batch and its gradients, fp32 / float64"""
    from oracle import butd as ob
    from _fullwidth import attention_kink_units
    p = params_cpu(seed)
    caps, lengths = xe_case(seed, len(counts))
    _, em, am, om = arrays
    order = ob.packed_order(lengths)
    out, kink = {}, np.zeros(A, bool)
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dt)
        try:
            pp = _typed(p, dt, True)
            per = []
            for i, c in enumerate(counts):
                m = (em[:, i:i + 1], am[:, i:i + 1, :c], om[:, i:i + 1]) if train else (None, None, None)
                trace = {}
                per.append(ob.forward_xe(feats[i:i + 1, :c].to(dt), caps[i:i + 1], [lengths[i]], pp, *m, trace=trace))
                if dt == torch.float64:
                    kink = kink | attention_kink_units(feats[i:i + 1, :c].double(), {k: v.detach() for k, v in pp.items()}, trace["h1"],
                                                       [am[t, i:i + 1, :c] for t in range(lengths[i])] if train else None)
            packed = torch.stack([per[b][t] for b, t in order])
            target = torch.stack([caps[b, t + 1] for b, t in order])
            loss = ob.label_smoothing_loss(packed, target, 0.1)
            loss.backward()
            out[name] = (packed.detach(), float(loss.detach()), {k: v.grad.double().numpy() for k, v in pp.items()})
        finally:
            torch.set_default_dtype(torch.float32)
    out["kink"] = kink
    return caps, lengths, out


def check_grads(what, grads, ref):
    """Every gradient tensor under the project's standing rule, _fullwidth.check_grads_against_float64, unchanged: per unit
    |HIP - f64| <= 2 |torch32 - f64| + 2e-4 max|f64| -- inside the 2e-4 of the maximum, or 4 x the fp32 oracle's own error where that
    is larger, that this feature's issue sets -- and, as in every BUTD gradient test of the suite, only attention units with a kept relu
    pre-activation at zero in the float64 pass may leave it (counted, at most 1 % of the units, capped at 2e-2): a flipped relu element
    moves a unit's gradient by a finite amount in ANY fp32 evaluation, the fp32 oracle's included (measured on the MI355X: 5.5e-3 of the
    maximum at R = 100 on the device where the fp32 oracle has none; 9.3e-3 in the fp32 oracle itself at sample_n)."""
    from _fullwidth import check_grads_against_float64
    kink = ref["kink"]
    rep = check_grads_against_float64(grads, ref["f32"][-1], ref["f64"][-1], {"atten.enc_att": kink, "atten.dec_att": kink})
    worst = max(rep, key=lambda k: rep[k][0])
    print(what, "kink units", int(kink.sum()), "worst |HIP - f64| / max, beside torch32's, units outside:", worst, rep[worst])
    return rep
