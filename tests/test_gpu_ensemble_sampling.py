"""GPU tests of an ensemble's sampling decode (include/icz.h: icz_ensemble_sample_decode, icz_ensemble_sample_filter_draw): the
ensemble instance of the filter-and-draw kernel alone against the float64 oracle, a one-member ensemble and identical copies against
the member's own sampling decode, two and three members against the host oracle of tests/_ens_sampling_cases.py, the identities
(top_k = 1 is greedy, n samples = repeated features, Philox determinism), the argument errors and the engine functions."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _beam_opts_oracle as bo  # noqa: E402
import _ens_sampling_cases as ec  # noqa: E402
import _philox  # noqa: E402
import _sampling_oracle as so  # noqa: E402
import test_gpu_ensemble as tge  # noqa: E402
import test_gpu_sampling as tgs  # noqa: E402
from oracle import butd as ob  # noqa: E402

T = ec.T
RNG_DECODE = 7                                   # csrc/rng.h: the stream of the sampling decode's draws
FORMS = ["finished", "unpadded", "slabs2", "slabs4"]


# ---- the kernel alone -----------------------------------------------------------------------------------------------------
def _weight_sets(M):
    """uniform, unequal, one zero (an ensemble of one has only its own weight)"""
    if M == 1:
        return [None, [2.5]]
    unequal = [1.0, 3.0, 0.5, 4.0][:M]
    zero = list(unequal)
    zero[1] = 0.0
    return [None, unequal, zero]


def _kernel_members(V, M, rows, vi, seed):
    """M members' logits in mixed forms -> ([(device tensor, bias, nsplit, ld)], [the fp32 logits the kernel must see])"""
    rs = np.random.RandomState(seed)
    members, full = [], []
    for m in range(M):
        x = (rs.randn(rows, V) * 3.0).astype(np.float32)
        dev, bias, ns, ld, f = tgs._forms(x, FORMS[(m + vi) % 4], rs)
        members.append((dev, bias, ns, ld))
        full.append(f)
    return members, full


def _check_rows(members, full, weights, opts, u, label, strict=False):
    """one launch against the oracle on the host's fp32 combined rows -> the number of excused rows (strict: none may be)"""
    from simpleimagecaptionzoo_amd.ensemble import sample_filter_draw
    rows, V = full[0].shape
    lp = tge._host_lp([f.astype(np.float64) for f in full], weights if weights is not None else [1.0] * len(full)).astype(np.float32)
    tok, logp, keep = sample_filter_draw(members, weights, rows, V, torch.tensor(u).cuda(), *opts)
    torch.cuda.synchronize()
    tok, logp, keep = tok.cpu().numpy(), logp.cpu().numpy(), keep.cpu().numpy().astype(bool)
    excused = 0
    for r in range(rows):
        info = {}
        w_tok, w_lp, w_keep = so.sample_row(lp[r], u[r], *opts, info=info)
        if not np.array_equal(keep[r], w_keep) or tok[r] != w_tok:
            print("kernel %s %s row %d differs: %s" % (label, opts, r, info))
            assert not strict, (label, opts, r)
            assert info["cdf_margin"] < 1e-5 or info["topk_margin"] < 1e-5 or info["nucleus_margin"] < 1e-5, (label, opts, r, info)
            excused += 1
            continue
        # the project's rule (tests/test_gpu_ensemble.py): 1e-6 absolute, widened by two fp32 ulps of the value
        err = abs(float(logp[r]) - w_lp) - abs(w_lp) * 2.0 ** -22
        assert err <= 1e-6, (label, opts, r, float(logp[r]), w_lp)
    return excused


@pytest.mark.parametrize("V", [53, 70, 203, 10102])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_kernel_against_float64(V, M):
    rows, vi = 12, [53, 70, 203, 10102].index(V)
    members, full = _kernel_members(V, M, rows, vi, 1000 * M + V)
    rs = np.random.RandomState(V + M)
    excused = 0
    for weights in _weight_sets(M):
        for opts in tgs._option_sets(V) + [(2.0, 1, 1.0)]:
            u = rs.rand(rows).astype(np.float32)
            excused += _check_rows(members, full, weights, opts, u, "V=%d M=%d w=%s" % (V, M, weights))
    print("kernel V=%d M=%d: %d rows excused (cap 1)" % (V, M, excused))
    assert excused <= 1


@pytest.mark.parametrize("V", [70, 10102])
@pytest.mark.parametrize("M", [1, 2])
def test_kernel_ties_across_the_top_k_cut(V, M):
    """every member's logits on one grid of 0.5: equal logits give equal combined log-probabilities, every top_k lands inside a
    group of them, and the lowest indices win"""
    rs = np.random.RandomState(V + 1)
    x = (np.round(rs.randn(8, V) * 2.0) * 0.5).astype(np.float32)
    x[3, :] = 1.25                                   # a whole row of one value
    x[4, ::7] = -0.0                                  # -0 and +0 are one value
    u = rs.rand(8).astype(np.float32)
    members = [(torch.tensor(x).cuda(), None, 1, V) for _ in range(M)]
    weights = [None, [1.0, 3.0]][M - 1]
    lp = tge._host_lp([x.astype(np.float64)] * M, weights if weights is not None else [1.0]).astype(np.float32)
    for r in range(8):                               # the premise: ties of x are ties of the row the kernel filters
        assert len(np.unique(lp[r])) == len(np.unique(x[r] + np.float32(0.0)))
    from simpleimagecaptionzoo_amd.ensemble import sample_filter_draw
    excused = 0
    for k in (1, 2, 5, 17, V // 2, V - 1):
        _, _, keep = sample_filter_draw(members, weights, 8, V, torch.tensor(u).cuda(), 1.0, k, 1.0)
        assert (keep.cpu().numpy().sum(1) == k).all(), k
        assert _check_rows(members, [x] * M, weights, (1.0, k, 1.0), u, "ties V=%d M=%d" % (V, M), strict=True) == 0
        excused += _check_rows(members, [x] * M, weights, (0.7, k, 0.8), u, "ties V=%d M=%d" % (V, M))
    assert excused <= 1


# ---- whole decodes ----------------------------------------------------------------------------------------------------------
def _compare(got, w_ids, w_lp, excuse, label):
    """got = (ids, logp, score) of the device; rows may differ from w_ids only where excuse(row, step) holds -> differing rows"""
    ids, logp, score = [x.cpu().numpy() for x in got]
    bad = np.nonzero((ids != w_ids).any(1))[0]
    for r in bad:
        t = int(np.nonzero(ids[r] != w_ids[r])[0][0])
        ok, info = excuse(int(r), t)
        print("%s: row %d differs at step %d: %s" % (label, r, t, info))
        assert ok, (label, r, t, info)
    good = np.ones(ids.shape[0], bool)
    good[bad] = False
    if good.any():
        print("%s: max logp err %.3g" % (label, np.abs(logp[good] - w_lp[good]).max()))
        np.testing.assert_allclose(logp[good], w_lp[good], atol=1e-4, rtol=0)
    # score = the fp32 sum of the row's log-probs in step order (test_gpu_sampling._check_decode's rule)
    tol = T * 2.0 ** -24 * np.maximum(1.0, np.abs(logp).sum(1))
    assert (np.abs(score - logp.astype(np.float64).sum(1)) <= tol).all(), label
    assert ((ids == 2).cumsum(1) - (ids == 2) == 0)[ids != 0].all(), label          # nothing but 0 behind a drawn <end>
    return len(bad)


def _member_excuse(model, p, feats_cpu, n, w_ids, u, opts):
    """excuse(row, step) along a single member's own ids: its host logits at that step, teacher-forced on the ids in front"""
    def excuse(r, t):
        with torch.no_grad():
            step, state, _ = bo.CLOSURES[model](feats_cpu[r // n:r // n + 1], p, 1)
            prev = torch.tensor([1])
            for s in range(t + 1):
                logits, state = step(prev, state)
                prev = torch.tensor([int(w_ids[r, s])])
        info = {}
        so.sample_row(logits[0].numpy(), u[t, r], *opts, info=info)
        return info["cdf_margin"] < ec.CDF_EDGE or info["topk_margin"] < ec.TOPK_MARGIN or info["nucleus_margin"] < ec.NUCLEUS_MARGIN, info
    return excuse


def _against_the_member(golden_dir, name, copies):
    """an ensemble of `copies` handles of one golden against one handle's own sampling decode: explicit uniforms, then Philox"""
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    model, h, p, feats = ec.device_member(golden_dir, name)
    others = [ec.device_member(golden_dir, name)[1] for _ in range(copies - 1)]
    ens = EnsembleHandle([h] + others, [1.0 / copies] * copies if copies > 1 else None)
    fl = [feats] * copies
    for kind in ("uniforms", "philox"):
        differing = 0
        for n in (1, 3):
            rows = feats.shape[0] * n
            for i, opts in enumerate(ec.option_sets(h.V)):
                seed = 7 * n + i
                u = ec.uniforms(rows, seed) if kind == "uniforms" else _philox._uniforms(seed, T, rows, RNG_DECODE)
                rng = torch.tensor(u).cuda() if kind == "uniforms" else seed
                want = h.sample_decode(feats, n, T, *opts, rng=rng)
                got = ens.sample_decode(fl, n, T, *opts, rng=rng)
                torch.cuda.synchronize()
                w_ids, w_lp = want[0].cpu().numpy(), want[1].cpu().numpy()
                differing += _compare(got, w_ids, w_lp, _member_excuse(model, p, feats.cpu(), n, w_ids, u, opts),
                                      "%s x%d %s n=%d %s" % (name, copies, kind, n, opts))
        print("%s x%d %s: %d of 48 rows differ (cap %d)" % (name, copies, kind, differing, ec.MAX_DIFFERING_ROWS))
        assert differing <= ec.MAX_DIFFERING_ROWS


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd"])
def test_one_member_equals_the_member(golden_dir, name):
    _against_the_member(golden_dir, name, 1)


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd"])
def test_identical_copies_equal_the_single_model(golden_dir, name):
    _against_the_member(golden_dir, name, 2)


def _build(golden_dir, case, end_boost=0.0, **kw):
    """-> (EnsembleHandle, device features (an AoA member's through RegionBatch on counts), the oracle's parts, V)"""
    from simpleimagecaptionzoo_amd.aoa import RegionBatch
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    specs, weights, counts = ec.CASES[case]
    members = [ec.device_member(golden_dir, name, seed, end_boost if j == 0 else 0.0, **kw) for j, (name, seed) in enumerate(specs)]
    dev = [RegionBatch(f, counts) if model == "aoa" and counts is not None else f for model, _, _, f in members]
    parts = ec.host_parts([(model, p, f.cpu()) for model, _, p, f in members], counts)
    return EnsembleHandle([m[1] for m in members], weights), dev, parts, members[0][1].V


def _against_the_oracle(ens, dev, parts, weights, V, runs, label):
    """runs: [(n, option set, uniforms seed)] -> (differing rows, rows, whether a row drew <end>)"""
    differing, total, ended = 0, 0, False
    for n, opts, seed in runs:
        rows = ec.N_IMG * n
        u = ec.uniforms(rows, seed)
        got = ens.sample_decode(dev, n, T, *opts, rng=torch.tensor(u).cuda())
        torch.cuda.synchronize()
        traces = []
        w_ids, w_lp = ec.oracle_decode(parts, weights, n, u, opts, traces)
        differing += _compare(got, w_ids, w_lp, lambda r, t: ec.row_excused(traces, u, n, r, t, opts), "%s n=%d %s" % (label, n, opts))
        total += rows
        ended = ended or bool((got[0] == 2).any())
    return differing, total, ended


@pytest.mark.parametrize("case", list(ec.CASES))
def test_members_against_the_oracle(golden_dir, case):
    """Token-exact against the float64 oracle of the combined log-probabilities, 3 images, n = 1 and 3, the four option sets.  A row
    may differ only from a first step where the oracle shows the draw within 1e-5 of a CDF edge, logits within 1e-4 across the top-k
    cut or a nucleus mass within 2e-4 of top_p; at most 2 of the 48 rows.  Then the same ensemble with a first member whose <end>
    bias is raised by 4 (18 rows under the same rule), so that finished rows beside live ones are exercised in every case."""
    weights = ec.CASES[case][1]
    ens, dev, parts, V = _build(golden_dir, case)
    runs = [(n, opts, 7 * n + i) for n in (1, 3) for i, opts in enumerate(ec.option_sets(V))]
    differing, total, ended = _against_the_oracle(ens, dev, parts, weights, V, runs, case)
    print("%s: %d of %d rows differ (cap %d)" % (case, differing, total, ec.MAX_DIFFERING_ROWS))
    assert total == 48 and differing <= ec.MAX_DIFFERING_ROWS
    ens, dev, parts, V = _build(golden_dir, case, end_boost=4.0)
    runs = [(3, opts, 90 + i) for i, opts in enumerate(ec.option_sets(V)[::3])]
    differing, total, ended_boost = _against_the_oracle(ens, dev, parts, weights, V, runs, case + " <end>+4")
    print("%s <end>+4: %d of %d rows differ (cap %d)" % (case, differing, total, ec.MAX_DIFFERING_ROWS))
    assert differing <= ec.MAX_DIFFERING_ROWS
    assert ended_boost and (ended or case != "nic2")          # the NIC members end their captions as they are


# ---- identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["butd2", "mixed3"])
def test_top_k_1_is_greedy(golden_dir, case):
    ens, dev, _, _ = _build(golden_dir, case, end_boost=4.0)
    want = ens.greedy(dev, T).cpu().numpy()
    for temp, seed in ((1.0, 1), (0.3, 2), (2.5, 3)):
        u = torch.tensor(ec.uniforms(ec.N_IMG, seed)).cuda()
        ids = ens.sample_decode(dev, 1, T, temp, 1, 1.0, rng=u)[0].cpu().numpy()
        for r in range(ids.shape[0]):
            end = np.nonzero(want[r] == 2)[0]
            stop = int(end[0]) + 1 if len(end) else T                 # greedy goes on behind <end>; the sampled row stops
            assert np.array_equal(ids[r, :stop], want[r, :stop]) and (ids[r, stop:] == 0).all(), (case, temp, r)


@pytest.mark.parametrize("case", ["aoa2", "mixed3"])
def test_n_samples_equal_repeated_features(golden_dir, case):
    ens, dev, _, _ = _build(golden_dir, case, end_boost=4.0)
    u = torch.tensor(ec.uniforms(ec.N_IMG * 3, 11)).cuda()
    rep = [f.repeat_interleave(3, 0).contiguous() for f in dev]
    for opts in ((1.0, 0, 1.0), (0.8, 20, 0.9)):
        a = ens.sample_decode(dev, 3, T, *opts, rng=u)
        a = [x.clone() for x in a]
        b = ens.sample_decode(rep, 1, T, *opts, rng=u)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (case, opts)


@pytest.mark.parametrize("case", ["butd2", "nic2", "mixed3"])
def test_philox_runs(golden_dir, case):
    ens, dev, _, _ = _build(golden_dir, case)
    for opts in ((1.0, 0, 1.0), (0.9, 30, 0.95)):
        a = [x.clone() for x in ens.sample_decode(dev, 3, T, *opts, rng=1234)]
        b = [x.clone() for x in ens.sample_decode(dev, 3, T, *opts, rng=1234)]          # two consecutive runs: bit-equal
        c = ens.sample_decode(dev, 3, T, *opts, rng=1235)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (case, opts)
        assert not torch.equal(a[0], c[0])
        assert len({tuple(r) for r in a[0].cpu().numpy()[:3]}) > 1        # the rows of one image are different draws
        # the uniforms are those of the single-model driver: stream RNG_DECODE keyed by (seed, step, row)
        u = torch.tensor(_philox._uniforms(1234, T, ec.N_IMG * 3, RNG_DECODE)).cuda()
        d = ens.sample_decode(dev, 3, T, *opts, rng=u)
        assert all(torch.equal(x, y) for x, y in zip(a, d)), (case, opts)


# ---- errors -------------------------------------------------------------------------------------------------------------------
def _raw(ens, feats, n_img, n, opts, outs):
    """icz_ensemble_sample_decode itself, past the Python checks -> (status, message)"""
    from simpleimagecaptionzoo_amd._lib import SampleOpts, lib, stream_ptr
    arr = (C.c_void_p * len(feats))(*[f.data_ptr() for f in feats])
    o = SampleOpts(*opts)
    st = lib().icz_ensemble_sample_decode(ens._h, arr, n_img, n, T, C.byref(o), 0, None, *[C.c_void_p(x.data_ptr()) for x in outs], stream_ptr())
    return st, lib().icz_last_error()


def test_errors_queue_nothing(golden_dir):
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    _, h53, _, f53 = ec.device_member(golden_dir, "butd_dec_tiny")
    _, n53, _, fn = ec.device_member(golden_dir, "nic_dec_tiny", max_rows=8)
    _, raw, _, _ = ec.device_member(golden_dir, "butd_dec_tiny", bind=False)        # never bound: not refreshed
    ens = EnsembleHandle([h53, n53])
    ens_raw = EnsembleHandle([h53, raw])
    assert ens.max_rows == 8
    before = [x.clone() for x in ens.sample_decode([f53[:2], fn[:2]], 3, T, 0.9, 20, 0.9, rng=5)]
    outs = [torch.full((16, T), -7, dtype=torch.int64, device="cuda"), torch.full((16, T), -7.0, device="cuda"), torch.full((16,), -7.0, device="cuda")]
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated()
    for n in (0, 9):
        with pytest.raises(ValueError, match="outside 1..8"):
            ens.sample_decode([f53, fn], n, T)
        st, msg = _raw(ens, [f53, fn], 1, n, (1.0, 0, 1.0), outs)
        assert st == -1 and b"samples per image outside 1..8" in msg, msg
    with pytest.raises(ValueError, match="top_p"):
        ens.sample_decode([f53, fn], 1, T, top_p=0)
    st, msg = _raw(ens, [f53, fn], 1, 1, (1.0, 0, 0.0), outs)
    assert st == -1 and b"top_p 0 outside (0, 1]" in msg, msg
    st, msg = _raw(ens, [f53, fn], 1, 1, (1.0, 54, 1.0), outs)
    assert st == -1 and b"top_k 54 outside 0..V (53)" in msg, msg
    with pytest.raises(ValueError, match="row capacity 8"):
        ens.sample_decode([f53, fn], 3, T)                             # 3 images x 3 samples > the NIC member's 8 rows
    st, msg = _raw(ens, [f53, fn], 3, 3, (1.0, 0, 1.0), outs)
    assert st == -1 and b"3 images x 3 samples exceed row capacity 8" in msg, msg
    with pytest.raises(IczError, match="not refreshed"):
        ens_raw.sample_decode([f53, f53], 1, T)
    with pytest.raises(ValueError, match="image counts"):
        ens.sample_decode([f53, fn[:2]], 1, T)
    with pytest.raises(ValueError, match="2 members"):
        ens.sample_decode([f53], 1, T)
    with pytest.raises(ValueError, match="uniforms must be"):
        ens.sample_decode([f53, fn], 2, T, rng=torch.zeros(T, 5, device="cuda"))
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem0
    assert (outs[0] == -7).all() and (outs[1] == -7.0).all() and (outs[2] == -7.0).all()      # a refused call wrote nothing
    # the handle's buffers are as they were: the same call gives the same bits
    after = ens.sample_decode([f53[:2], fn[:2]], 3, T, 0.9, 20, 0.9, rng=5)
    assert all(torch.equal(x, y) for x, y in zip(before, after))


# ---- engine functions -----------------------------------------------------------------------------------------------------------
def _entries(vocab, image_ids, tok, score, n):
    out = []
    for r in range(tok.shape[0]):
        words = []
        for t in tok[r]:
            if int(t) in (0, 2):
                break
            if int(t) != 1:
                words.append(vocab.ix2word[int(t)])
        out.append({"image_id": image_ids[r // n], "caption": " ".join(words), "score": float(score[r])})
    return out


def test_engine_functions(golden_dir):
    from simpleimagecaptionzoo_amd.engine import consensus_ensemble_captions_json_generation, sample_ensemble_captions_json_generation
    from simpleimagecaptionzoo_amd.ensemble import CaptionEnsemble
    e1, g, _ = tge._perturbed_engine(golden_dir, 0)
    e2, _, _ = tge._perturbed_engine(golden_dir, 5)
    ids, supp = tge._batch(g)
    loader = [(ids[:3], None, supp[:3]), (ids[3:], None, supp[3:])]
    n, opts, seed, w = 3, (0.9, 20, 0.9), 5, [1.0, 2.0]
    res = sample_ensemble_captions_json_generation([e1, e2], loader, n, *opts, seed=seed, tqdm_visible=False, weights=w)
    again = sample_ensemble_captions_json_generation([e1, e2], loader, n, *opts, seed=seed, tqdm_visible=False, weights=w)
    assert res == again                                                                  # stable run to run
    assert [r["image_id"] for r in res] == [i for i in ids for _ in range(n)]          # n entries per image, loader order
    ce = CaptionEnsemble([e1.model, e2.model], weights=w)
    want = []
    for bi, (bids, _, bsupp) in enumerate(loader):
        vis = [e.modify_visual_inputs(None, bsupp) for e in (e1, e2)]
        tok, _, score = ce.sample_decode(vis, n, 20, *opts, rng=(seed << 20) + bi)
        torch.cuda.synchronize()
        want += _entries(e1.caption_vocab, bids, tok.cpu().numpy(), score.cpu().numpy(), n)
    assert res == want
    assert all(np.isfinite(r["score"]) and r["score"] <= 0 for r in res)
    other = sample_ensemble_captions_json_generation([e1, e2], loader, n, *opts, seed=seed + 1, tqdm_visible=False, weights=w)
    assert [r["caption"] for r in other] != [r["caption"] for r in res]
    # consensus = sampling followed by the lead engine's rerank
    cons = consensus_ensemble_captions_json_generation([e1, e2], loader, n, *opts, seed=seed, tqdm_visible=False, weights=w)
    assert cons == e1.rerank_captions_json(res, n) and len(cons) == len(ids)
    # one engine = that engine's own method, under the one-member rule
    single = e1.sample_captions_json_generation(loader, n, *opts, seed=seed, tqdm_visible=False)
    one = sample_ensemble_captions_json_generation([e1], loader, n, *opts, seed=seed, tqdm_visible=False)
    assert [r["image_id"] for r in one] == [r["image_id"] for r in single]
    p = ob.strip_prefix({k: v.detach().cpu() for k, v in e1.model.state_dict().items()})
    differing = 0
    for j, (a, b) in enumerate(zip(one, single)):
        if a["caption"] == b["caption"]:
            assert abs(a["score"] - b["score"]) <= 20 * 1e-4, (j, a, b)              # 20 log-probs, each within 1e-4
            continue
        differing += 1
        bi, r = (0, j) if j < 3 * n else (1, j - 3 * n)
        bsupp = loader[bi][2]
        with torch.cuda.stream(e1.stream):
            feats = e1._features(e1.modify_visual_inputs(None, bsupp))
            w_ids = e1._hot_handle().sample_decode(feats, n, 20, *opts, rng=(seed << 20) + bi)[0]
        e1.stream.synchronize()
        w_ids = w_ids.cpu().numpy()
        o_ids = EnsembleOne(e1).decode(feats, n, opts, (seed << 20) + bi)
        t = int(np.nonzero(o_ids[r] != w_ids[r])[0][0])
        u = _philox._uniforms((seed << 20) + bi, 20, feats.shape[0] * n, RNG_DECODE)
        ok, info = _member_excuse("butd", p, feats.cpu(), n, w_ids, u, opts)(r, t)
        print("engine: entry %d differs at step %d: %s" % (j, t, info))
        assert ok, (j, t, info)
    assert differing <= ec.MAX_DIFFERING_ROWS


class EnsembleOne:
    """the one-engine ensemble's ids of a batch (for the excuse of a differing entry)"""

    def __init__(self, eng):
        self.eng = eng

    def decode(self, feats, n, opts, seed):
        from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
        with torch.cuda.stream(self.eng.stream):
            ids = EnsembleHandle([self.eng._hot_handle()]).sample_decode([feats], n, 20, *opts, rng=seed)[0]
        self.eng.stream.synchronize()
        return ids.cpu().numpy()
