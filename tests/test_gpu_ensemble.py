"""GPU tests of model ensembles (include/icz.h: icz_ensemble_*): the combine kernel against float64, a one-member ensemble against
the member's own decodes, identical copies, mixed BUTD / AoA / NIC ensembles against a host oracle built from the per-model step
closures of tests/_beam_opts_oracle.py, the Engine-level evaluation and the argument errors."""
import gc
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _beam_opts_oracle as bo  # noqa: E402
import _diverse_beam_oracle as dbo  # noqa: E402
from oracle import butd as ob  # noqa: E402
from synth import feats_from_seed  # noqa: E402

# beam option sets: (n_best, length_penalty, block_ngram, groups)
OPTION_SETS = [(1, None, 0, 1), ("all", None, 0, 1), (1, "wu_0.6", 0, 1), ("all", None, 3, 1), ("all", None, 0, 2)]
LP = {None: (0, 0.0), "wu_0.6": (2, 0.6)}
DIVERSITY = 0.7


# ---- the combine kernel ---------------------------------------------------------------------------------------------------
def _host_lp(logits, weights):
    w = np.asarray(weights, np.float64)
    w = w / w.sum()
    with np.errstate(divide="ignore"):           # a zero weight: log 0 = -inf, the member drops out
        logw = np.log(w)
    terms = [logw[m] + x - np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)) - x.max(1, keepdims=True)
             for m, x in enumerate(logits)]
    t = np.stack(terms)
    top = t.max(0)
    return top + np.log(np.exp(t - top).sum(0))


def _run_logprob(members, weights, rows, V, argmax=False):
    """members: [(device tensor, bias or None, nsplit, ld)] -> lp (rows, V) or argmax ids (rows,)"""
    import ctypes as C
    from simpleimagecaptionzoo_amd._lib import check, lib, stream_ptr
    M = len(members)
    lg = (C.c_void_p * M)(*[t.data_ptr() for t, _, _, _ in members])
    bs = (C.c_void_p * M)(*[b.data_ptr() if b is not None else None for _, b, _, _ in members])
    ns = (C.c_int32 * M)(*[n for _, _, n, _ in members])
    ld = (C.c_int32 * M)(*[l for _, _, _, l in members])
    w = (C.c_float * M)(*weights) if weights is not None else None
    ldo = (V + 63) & ~63
    out = torch.full((rows, ldo), 7.0, device="cuda")
    ids = torch.full((rows,), -5, dtype=torch.int64, device="cuda")
    check(lib().icz_ensemble_logprob(M, lg, bs, ns, ld, w, rows, V, None if argmax else C.c_void_p(out.data_ptr()), ldo,
                                     C.c_void_p(ids.data_ptr()) if argmax else None, stream_ptr()))
    torch.cuda.synchronize()
    return ids.cpu().numpy() if argmax else out.cpu().numpy()


@pytest.mark.parametrize("V", [203, 1001, 9487])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_combine_kernel_against_float64(V, M):
    rs = np.random.RandomState(V + 10 * M)
    rows = 37
    weights = [None, [1.0, 3.0], [0.2, 0.0, 1.3], [1.0, 2.0, 0.5, 4.0]][M - 1]
    members, full = [], []
    for m in range(M):
        form = ("finished", "slabs", "finished_unpadded", "slabs")[(m + V) % 4]
        x = (rs.randn(rows, V) * 1.5).astype(np.float32)
        if form == "finished":
            ld = (V + 63) & ~63
            buf = np.zeros((rows, ld), np.float32)
            buf[:, :V] = x
            members.append((torch.tensor(buf).cuda(), None, 1, ld))
        elif form == "finished_unpadded":        # ld = V (not a multiple of 4): the scalar path
            members.append((torch.tensor(x).cuda(), None, 1, V))
        else:
            ns, ld = 3 + m % 2, (V + 63) & ~63
            slabs = (rs.randn(ns, rows, ld) * 0.7).astype(np.float32)
            bias = (rs.randn(ld) * 0.5).astype(np.float32)
            x = slabs[0, :, :V].copy()
            for z in range(1, ns):
                x = (x + slabs[z, :, :V]).astype(np.float32)
            x = (x + bias[:V]).astype(np.float32)
            members.append((torch.tensor(slabs).cuda(), torch.tensor(bias).cuda(), ns, ld))
        full.append(x.astype(np.float64))
    want = _host_lp(full, weights if weights is not None else [1.0] * M)
    got = _run_logprob(members, weights, rows, V)
    # 1e-6 absolute, widened by two fp32 ulps of the value: at V ~ 9.5k log-probs reach -13, where one ulp is ~1e-6
    err = np.abs(got[:, :V] - want) - np.abs(want) * 2.0 ** -22
    assert err.max() <= 1e-6, err.max()
    assert (got[:, V:] == 7.0).all()                  # nothing written past V
    ids = _run_logprob(members, weights, rows, V, argmax=True)
    lp32 = got[:, :V]
    assert (ids == lp32.argmax(1)).all()


def test_combine_kernel_ties_to_lowest_index():
    V, rows = 300, 4
    x = np.zeros((rows, V), np.float32)
    x[:, [17, 40, 299]] = 5.0
    x[1, 3] = 5.0
    ids = _run_logprob([(torch.tensor(x).cuda(), None, 1, V)], None, rows, V, argmax=True)
    assert ids.tolist() == [17, 3, 17, 17]


# ---- members built from the goldens ---------------------------------------------------------------------------------------
def _member(golden_dir, name, seed=0, max_rows=16, max_len=20, n_img=3):
    """-> (model, handle, CPU parameters, device features of n_img images); seed > 0 perturbs every parameter (another checkpoint)"""
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
    if name.startswith("butd"):
        from simpleimagecaptionzoo_amd.butd import ButdHandle
        model, sd = "butd", ob.strip_prefix(sd)
        B, R, D, H, E, A, V = [int(x) for x in g["dims"]]
        h = ButdHandle(R, D, H, E, A, V, max_rows, max_len)
        feats = torch.tensor(g["feats"])
    elif name.startswith("aoa"):
        from simpleimagecaptionzoo_amd.aoa import AoaHandle
        model = "aoa"
        B, R, D, Hd, E, V, NH = [int(x) for x in g["dims"]]
        h = AoaHandle(R, D, Hd, E, V, NH, max_rows, max_len)
        feats = torch.from_numpy(feats_from_seed(int(g["feats_seed"]), B, R, D))
    else:
        from simpleimagecaptionzoo_amd.nic import NicHandle
        model = "nic"
        B, H, E, V = [int(x) for x in g["dims"]]
        h = NicHandle(E, H, V, max_rows, max_len)
        feats = torch.tensor(g["feats"])
    rs = np.random.RandomState(seed)
    params = {}
    for k in sorted(sd):
        v = np.asarray(sd[k], np.float32)
        if seed:
            v = (v * (1.0 + 0.35 * rs.randn(*v.shape))).astype(np.float32)
        params[k] = torch.tensor(v, device="cuda")
    h.bind(params)
    p = {k: v.cpu() for k, v in params.items()}
    return model, h, p, feats[:n_img].contiguous().cuda()


def _lists(seqs, lens, scores):
    seqs, lens, scores = seqs.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()
    return [[(seqs[i, j, :lens[i, j]].astype(int).tolist(), float(scores[i, j])) for j in range(lens.shape[1])]
            for i in range(lens.shape[0])]


def _cases():
    """(beam, option set): beams 3 and 5, the two-group set at beam 4 (groups divide the beam)"""
    return [(k, o) for k in (3, 5) for o in OPTION_SETS if o[3] == 1] + [(4, o) for o in OPTION_SETS if o[3] > 1]


def _beam_kw(k, opt):
    n_best, lp, block, groups = opt
    return dict(n_best=k if n_best == "all" else n_best, length_penalty=lp, block_ngram=block, groups=groups,
                diversity=DIVERSITY if groups > 1 else 0.0)


# ---- one member = the member ----------------------------------------------------------------------------------------------
def _margin_excuse(step_lp_rows, got, want):
    """the existing tests' excuse rule for a greedy row: at the first step where the ids differ the top-2 margin is < 1e-5"""
    t = next(i for i in range(len(want)) if got[i] != want[i])
    top2 = np.sort(step_lp_rows[t])[-2:]
    return top2[1] - top2[0] < 1e-5


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_odd"])
def test_one_member_equals_the_member(golden_dir, name):
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    model, h, p, feats = _member(golden_dir, name)
    ens = EnsembleHandle([h])
    want = h.greedy(feats, 20).cpu().numpy()
    got = ens.greedy([feats], 20).cpu().numpy()
    bad = [i for i in range(feats.shape[0]) if not np.array_equal(got[i], want[i])]
    assert len(bad) <= 2
    for i in bad:                                        # host log-probs along the member's own ids
        step, state, V = bo.CLOSURES[model](feats[i:i + 1].cpu(), p, 1)
        prev, rows = torch.tensor([1]), []
        with torch.no_grad():
            for t in range(20):
                logits, state = step(prev, state)
                rows.append(torch.log_softmax(logits.double(), 1)[0].numpy())
                prev = torch.tensor([int(want[i][t])])
        assert _margin_excuse(rows, got[i].tolist(), want[i].tolist()), (name, i)
    for k, opt in _cases():
        kw = _beam_kw(k, opt)
        w = _lists(*h.beam_search_opts(feats, k, 50, **kw))
        e = _lists(*ens.beam_search_opts([feats], k, 50, **kw))
        assert [[x[0] for x in img] for img in e] == [[x[0] for x in img] for img in w], (name, k, opt)
        np.testing.assert_allclose([x[1] for img in e for x in img], [x[1] for img in w for x in img], atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", ["butd_dec_tiny", "aoa_tiny", "nic_dec_tiny"])
def test_identical_copies_equal_the_single_model(golden_dir, name):
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    _, h, _, feats = _member(golden_dir, name)
    _, h2, _, _ = _member(golden_dir, name)
    ens = EnsembleHandle([h, h2], weights=[0.5, 0.5])
    assert torch.equal(ens.greedy([feats, feats], 20), h.greedy(feats, 20))
    for k in (3, 5):
        w = _lists(*h.beam_search_opts(feats, k, 50, n_best=k))
        e = _lists(*ens.beam_search_opts([feats, feats], k, 50, n_best=k))
        assert [[x[0] for x in img] for img in e] == [[x[0] for x in img] for img in w], (name, k)


# ---- against the oracle ---------------------------------------------------------------------------------------------------
def _ens_closure(parts, weights, k):
    """parts: [(model, feats1 (CPU, one image), params)] -> the oracle step closure of the ensemble:
    logits = log(sum_m w_m softmax(logits_m)), in float64"""
    w = np.asarray(weights if weights is not None else [1.0] * len(parts), np.float64)
    logw = torch.tensor(np.log(w / w.sum()))
    closures = [bo.CLOSURES[m](f, p, k) for m, f, p in parts]
    sizes = [len(c[1]) for c in closures]

    def step(prev, st):
        terms, new, i = [], [], 0
        for (fn, _, _), n, lw in zip(closures, sizes, logw):
            logits, s2 = fn(prev, st[i:i + n])
            i += n
            terms.append(torch.log_softmax(logits.double(), 1) + lw)
            new += list(s2)
        return torch.logsumexp(torch.stack(terms), 0), tuple(new)
    return step, tuple(x for c in closures for x in c[1]), closures[0][2]


def _oracle_greedy(parts, weights, max_len=20):
    step, state, _ = _ens_closure(parts, weights, 1)
    prev, ids, rows = torch.tensor([1]), [], []
    with torch.no_grad():
        for _ in range(max_len):
            lp, state = step(prev, state)
            rows.append(lp[0].numpy())
            prev = lp.argmax(1)
            ids.append(int(prev[0]))
    return ids, rows


def _check_ensemble(golden_dir, specs, weights, counts=None):
    from simpleimagecaptionzoo_amd.aoa import RegionBatch
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    members = [_member(golden_dir, name, seed) for name, seed in specs]
    handles = [m[1] for m in members]
    n_img = members[0][3].shape[0]
    dev_feats, host = [], []
    for model, _, p, f in members:
        if model == "aoa" and counts is not None:
            dev_feats.append(RegionBatch(f, counts))
            host.append([(model, f[i:i + 1, :counts[i]].cpu(), p) for i in range(n_img)])
        else:
            dev_feats.append(f)
            host.append([(model, f[i:i + 1].cpu(), p) for i in range(n_img)])
    parts = [[h[i] for h in host] for i in range(n_img)]
    ens = EnsembleHandle(handles, weights)
    got = ens.greedy(dev_feats, 20).cpu().numpy()
    bad = 0
    for i in range(n_img):
        want, rows = _oracle_greedy(parts[i], weights)
        if got[i].tolist() != want:
            bad += 1
            assert _margin_excuse(rows, got[i].tolist(), want), (specs, i)
    assert bad <= 2
    for k, opt in _cases():
        kw = _beam_kw(k, opt)
        e = _lists(*ens.beam_search_opts(dev_feats, k, 50, **kw))
        lp_kind, lp_alpha = LP[kw["length_penalty"]]
        for i in range(n_img):
            with torch.no_grad():
                step, state, V = _ens_closure(parts[i], weights, k)
                if kw["groups"] > 1:
                    want = dbo.diverse_nbest(step, state, k, kw["groups"], DIVERSITY, V, 50, kw["block_ngram"], lp_kind, lp_alpha)
                else:
                    want = bo.beam_nbest(step, state, k, V, 50, kw["block_ngram"], lp_kind, lp_alpha)
            want = want[:kw["n_best"]]
            assert [x[0] for x in e[i]] == [w[0] for w in want], (specs, k, opt, i)
            np.testing.assert_allclose([x[1] for x in e[i]], [w[1] for w in want], atol=1e-4, rtol=0)


@pytest.mark.parametrize("specs, weights", [
    ([("butd_dec_tiny", 0), ("butd_dec_tiny", 1)], None),
    ([("aoa_tiny", 0), ("aoa_tiny", 2)], [0.3, 0.7]),
    ([("nic_dec_odd", 0), ("nic_dec_odd", 3)], [2.0, 1.0]),
])
def test_two_members_against_the_oracle(golden_dir, specs, weights):
    _check_ensemble(golden_dir, specs, weights)


def test_mixed_butd_aoa_nic_against_the_oracle(golden_dir):
    """one member of each kind (V = 53), the AoA member on per-image region counts"""
    _check_ensemble(golden_dir, [("butd_dec_tiny", 0), ("aoa_tiny", 4), ("nic_dec_tiny", 0)], [1.0, 2.0, 1.5], counts=[36, 20, 11])


# ---- Engine level ---------------------------------------------------------------------------------------------------------
def _perturbed_engine(golden_dir, seed):
    import test_gpu_engine as tge
    g, fx = tge._load(golden_dir)
    eng, _ = tge._engine(g, fx)
    if seed:
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for prm in eng.model.parameters():
                prm.mul_(1.0 + 0.35 * torch.randn(prm.shape, generator=gen).to(prm.device))
    return eng, g, fx


def _batch(g):
    import test_gpu_engine as tge
    B, R, D = [int(x) for x in g["dims"]][:3]
    feats = feats_from_seed(int(g["eval_feats_seed"]), B, R, D)
    ids = tuple(int(i) for i in g["eval_img_ids"])
    return ids, tge._supp(feats)


def test_eval_one_engine_equals_the_engine(golden_dir):
    from simpleimagecaptionzoo_amd.engine import eval_ensemble_captions_json_generation
    eng, g, _ = _perturbed_engine(golden_dir, 0)
    ids, supp = _batch(g)
    loader = [(ids[:3], None, supp[:3]), (ids[3:], None, supp[3:])]
    for beam in (-1, 3):
        want = eng.eval_captions_json_generation(loader, eval_beam_size=beam, tqdm_visible=False)
        got = eval_ensemble_captions_json_generation([eng], loader, eval_beam_size=beam, tqdm_visible=False)
        assert got == want, beam


def test_eval_two_engines_equals_caption_ensemble(golden_dir):
    from simpleimagecaptionzoo_amd.engine import eval_ensemble_captions_json_generation
    from simpleimagecaptionzoo_amd.ensemble import CaptionEnsemble
    e1, g, _ = _perturbed_engine(golden_dir, 0)
    e2, _, _ = _perturbed_engine(golden_dir, 5)
    ids, supp = _batch(g)
    loader = [(ids, None, supp)]
    got = eval_ensemble_captions_json_generation([e1, e2], loader, eval_beam_size=3, tqdm_visible=False, weights=[1.0, 2.0])
    ce = CaptionEnsemble([e1.model, e2.model], weights=[1.0, 2.0])
    vis = [e.modify_visual_inputs(None, supp) for e in (e1, e2)]
    seqs = ce.beam_search_sampler(vis, 3)
    ix2word = e1.caption_vocab.ix2word
    want = []
    for image_id, s in zip(ids, seqs):
        words = []
        for w in s[0].tolist():
            word = ix2word[int(w)]
            if word == "<end>":
                break
            if word != "<sta>":
                words.append(word)
        want.append({"image_id": image_id, "caption": " ".join(words)})
    assert got == want
    # and the ensemble differs from either member alone somewhere in its scores (the members do disagree)
    nb = ce.beam_search_nbest(vis, 3, n_best=3)
    single = CaptionEnsemble([e1.model]).beam_search_nbest(vis[:1], 3, n_best=3)
    assert [[round(x[1], 4) for x in img] for img in nb] != [[round(x[1], 4) for x in img] for img in single]


# ---- argument errors ------------------------------------------------------------------------------------------------------
def test_errors_queue_nothing(golden_dir):
    import ctypes as C
    from simpleimagecaptionzoo_amd._lib import IczError, lib
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.ensemble import EnsembleHandle
    _, h53, _, f53 = _member(golden_dir, "butd_dec_tiny")
    _, h70, _, f70 = _member(golden_dir, "butd_dec_odd")
    _, n53, _, fn = _member(golden_dir, "nic_dec_tiny", max_rows=8)
    raw = ButdHandle(h53.R, h53.D, h53.H, h53.E, h53.A, h53.V, 16, 20)        # never bound: not refreshed
    ens = EnsembleHandle([h53, n53])
    ens_raw = EnsembleHandle([h53, raw])
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated()
    # V mismatch: the Python check, and the library's own
    with pytest.raises(ValueError, match="vocabulary"):
        EnsembleHandle([h53, h70])
    out = C.c_void_p()
    st = lib().icz_ensemble_create((C.c_int32 * 2)(0, 0), (C.c_void_p * 2)(h53._h.value, h70._h.value), None, 2, C.byref(out))
    assert st == -1 and b"member 1 has vocabulary 70, member 0 has 53" in lib().icz_last_error() and not out.value
    with pytest.raises(ValueError, match="appears twice"):
        EnsembleHandle([h53, h53])
    with pytest.raises(IczError, match="not refreshed"):
        ens_raw.greedy([f53, f53], 20)
    with pytest.raises(IczError, match="row capacity 8"):
        ens.beam_search_opts([f53, fn], 3, 20)                     # 3 images x 3 beams > the NIC member's 8 rows
    with pytest.raises(IczError, match="n_best 3 outside 1..beam"):
        ens.beam_search_opts([f53, fn], 2, 20, n_best=3)
    with pytest.raises(ValueError, match="groups"):
        ens.beam_search_opts([f53, fn], 2, 20, groups=3)
    with pytest.raises(ValueError, match="image counts"):
        ens.greedy([f53, fn[:2]], 20)
    with pytest.raises(ValueError, match="2 members"):
        ens.greedy([f53], 20)
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem0
    # the ensemble still decodes after its refusals
    assert ens.greedy([f53[:2], fn[:2]], 20).shape == (2, 20)
