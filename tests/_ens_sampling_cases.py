"""Shared by tests/test_gpu_ensemble_sampling.py and tests/test_cpu_ensemble_sampling.py, not collected by pytest: the ensemble
cases of the sampling decode (members built from the goldens, perturbed as tests/test_gpu_ensemble.py's _member perturbs them), the
host oracle over test_gpu_ensemble._ens_closure handing fp32 rows to _sampling_oracle.decode, and the excuse rule of a differing row."""
import os

import numpy as np
import torch

import _sampling_oracle as so
from oracle import butd as ob
from synth import feats_from_seed
from test_gpu_ensemble import _ens_closure

T = 20
N_IMG = 3
# name -> (members (golden, perturbation seed), weights, AoA region counts per image or None)
CASES = {
    "butd2": ([("butd_dec_tiny", 0), ("butd_dec_tiny", 1)], None, None),
    "aoa2": ([("aoa_tiny", 0), ("aoa_tiny", 2)], [0.3, 0.7], None),
    "nic2": ([("nic_dec_odd", 0), ("nic_dec_odd", 3)], [2.0, 1.0], None),
    "mixed3": ([("butd_dec_tiny", 0), ("aoa_tiny", 4), ("nic_dec_tiny", 0)], [1.0, 2.0, 1.0], None),
    "aoa2_counts": ([("aoa_tiny", 0), ("aoa_tiny", 2)], [0.3, 0.7], [36, 20, 11]),
}
ORACLE_CASES = ["butd2", "aoa2", "nic2", "mixed3"]
# whole-decode excuse thresholds (tests/test_gpu_sampling.py's full-width ones, the CDF one widened from 1e-6 to 1e-5)
CDF_EDGE, TOPK_MARGIN, NUCLEUS_MARGIN = 1e-5, 1e-4, 2e-4
MAX_DIFFERING_ROWS = 2


def option_sets(V):
    k = min(50, V)
    return [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, k, 1.0), (0.8, k, 0.9)]


def uniforms(rows, seed):
    return np.random.RandomState(seed).rand(T, rows).astype(np.float32)


def host_member(golden_dir, name, seed=0, end_boost=0.0):
    """-> (model, CPU parameters, CPU features of N_IMG images, the handle's constructor arguments): the parameters
    test_gpu_ensemble._member binds for (name, seed); end_boost is added to the <end> bias (a member that ends its captions)"""
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
    dims = [int(x) for x in g["dims"]]
    if name.startswith("butd"):
        model, sd, bias = "butd", ob.strip_prefix(sd), "predict.bias"
        feats = torch.tensor(g["feats"])
        ctor = dims[1:]                              # R, D, H, E, A, V
    elif name.startswith("aoa"):
        model, bias = "aoa", "decoder.predict.bias"
        feats = torch.from_numpy(feats_from_seed(int(g["feats_seed"]), dims[0], dims[1], dims[2]))
        ctor = dims[1:]                              # R, D, Hd, E, V, NH
    else:
        model, bias = "nic", "predict.bias"
        feats = torch.tensor(g["feats"])
        ctor = [dims[2], dims[1], dims[3]]           # E, H, V
    rs = np.random.RandomState(seed)
    p = {}
    for k in sorted(sd):
        v = np.asarray(sd[k], np.float32)
        if seed:
            v = (v * (1.0 + 0.35 * rs.randn(*v.shape))).astype(np.float32)
        p[k] = torch.tensor(v)
    if end_boost:
        p[bias] = p[bias].clone()
        p[bias][2] += end_boost
    return model, p, feats[:N_IMG].contiguous(), ctor


def device_member(golden_dir, name, seed=0, end_boost=0.0, max_rows=16, max_len=T, bind=True):
    """host_member on the device -> (model, handle, CPU parameters, device features)"""
    model, p, feats, ctor = host_member(golden_dir, name, seed, end_boost)
    if model == "butd":
        from simpleimagecaptionzoo_amd.butd import ButdHandle as H
    elif model == "aoa":
        from simpleimagecaptionzoo_amd.aoa import AoaHandle as H
    else:
        from simpleimagecaptionzoo_amd.nic import NicHandle as H
    h = H(*ctor, max_rows, max_len)
    if bind:
        h.bind({k: v.cuda() for k, v in p.items()})
    return model, h, p, feats.cuda()


def host_parts(members, counts=None):
    """members: [(model, p, CPU feats)] -> per image the parts of test_gpu_ensemble._ens_closure"""
    n_img = members[0][2].shape[0]
    return [[(model, f[i:i + 1, :counts[i]] if model == "aoa" and counts is not None else f[i:i + 1], p) for model, p, f in members]
            for i in range(n_img)]


def oracle_decode(parts, weights, n, u, opts, traces=None):
    """The ensemble's sampling decode on the host: per image the closure of the combined log-probabilities, its rows cast to fp32
    (the row the kernel filters is fp32), through _sampling_oracle.decode.  u [T, n_img n].  traces (a list) receives per image
    the per-step fp32 rows [n, V].  -> ids [n_img n, T], log-probs [n_img n, T] float64"""
    ids, lps = [], []
    for i, part in enumerate(parts):
        with torch.no_grad():
            step64, state, _ = _ens_closure(part, weights, n)

        def step(prev, st):
            lp, st = step64(prev, st)
            return lp.float(), st
        trace = []
        a, b = so.decode(step, state, n, u[:, i * n:(i + 1) * n], T, *opts, trace=trace)
        if traces is not None:
            traces.append(trace)
        ids.append(a)
        lps.append(b)
    return np.concatenate(ids), np.concatenate(lps)


def row_excused(traces, u, n, r, t, opts):
    """row r first differs at step t: does the float64 oracle show a margin under the whole-decode thresholds there?"""
    info = {}
    so.sample_row(traces[r // n][t][r % n], u[t, r], *opts, info=info)
    ok = info["cdf_margin"] < CDF_EDGE or info["topk_margin"] < TOPK_MARGIN or info["nucleus_margin"] < NUCLEUS_MARGIN
    return ok, info


def self_differences(traces, w_ids, u, n, opts):
    """the reference against itself: rows whose draws change when the filter runs in fp32 on the oracle's own rows"""
    bad = 0
    for r in range(w_ids.shape[0]):
        trace = traces[r // n]
        for t in range(len(trace)):
            if t > 0 and w_ids[r, t - 1] in (0, 2):
                break
            m32 = so.filter_masses(trace[t][r % n], *opts, dtype=np.float32)
            if so.draw(m32, u[t, r]) != w_ids[r, t]:
                bad += 1
                break
    return bad
