"""XE training on K captions per image on the device (icz_butd_xe_forward_n + icz_butd_xe_backward, Engine.training_epoch_grouped)
against the float64 statement of tests/_xe_grouped_oracle.py at the tiny golden dims: logits, loss, every gradient and the stored
attention maps, with explicit dropout masks in training and evaluation mode; against the ordinary xe_forward / xe_backward on the
repeated, length-sorted features; the three forms of the token normaliser; Philox masks against their regenerated explicit arrays;
option group_att on against off; per-image region counts; the images permuted; every refusal; one full-width case; the Engine method
against the same steps built by hand, and two data-parallel ranks against one process.
Tolerances (as tests/test_gpu_butd.py and tests/test_gpu_swor.py): logits 2e-4 (+ 1e-4 relative), a loss 1e-4, a
gradient tensor |got - want|max <= 2e-4 max(1e-3, |want|max) + 2e-6."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _philox
import _xe_grouped_oracle as xo

pytestmark = pytest.mark.gpu

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
T_STEPS = 6
_CASES = {}


def close(got, want, what):
    """the project's gradient rule on one tensor (got: a device tensor, want: numpy float64)"""
    got = got.detach().cpu().double().numpy()
    scale = max(1e-3, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print("%-60s max|want| %.3e  err/scale %.3e" % (what, float(np.abs(want).max()), err / scale))
    assert np.isfinite(got).all() and err <= 2e-4 * scale + 2e-6, (what, err, scale)


def case(golden_dir, name, B, K, train, counts=None, seed=0):
    """inputs and the statement of one case (made once, shared, never changed)"""
    key = (name, B, K, train, counts, seed)
    if key not in _CASES:
        g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
        B0, R, D, H, E, A, V = [int(x) for x in g["dims"]]
        rs = np.random.RandomState(1000 + 10 * K + seed)
        feats = np.ascontiguousarray(np.resize(g["feats"], (B, R, D)) if B > B0 else g["feats"][:B]).astype(np.float32)
        if B > B0:
            feats = np.abs(feats + 0.1 * rs.randn(B, R, D).astype(np.float32))        # distinct images
        caps, lens = xo.batch(rs, V, B, K, T_STEPS)
        masks = xo.keep_masks(rs, T_STEPS, B * K, E, R, A, H) if train else None
        sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
        want = xo.run(sd, feats, caps, lens, K, masks, 0.1, counts)
        _CASES[key] = {"g": g, "dims": (R, D, H, E, A, V), "feats": feats, "caps": caps, "lens": lens, "masks": masks, "K": K, "B": B,
                       "train": train, "counts": counts, "want": want}
    return _CASES[key]


def make_handle(c, max_rows=32, group_att=0):
    from test_gpu_butd import make_handle as mh
    h, _ = mh(c["g"], max_rows=max_rows)
    if group_att:
        h.set_option("group_att", 1)
    return h


def rng_of(c, masks="case", seed=0):
    from simpleimagecaptionzoo_amd.butd import make_rng
    masks = c["masks"] if isinstance(masks, str) else masks
    if masks is None:
        return make_rng(seed) if c["train"] else None
    return make_rng(seed, None, *(torch.tensor(np.ascontiguousarray(m), device=DEV) for m in masks))


def feats_of(c, feats=None, counts="case"):
    from simpleimagecaptionzoo_amd.regions import RegionBatch
    f = torch.tensor(c["feats"] if feats is None else feats, device=DEV)
    counts = c["counts"] if isinstance(counts, str) else counts
    return RegionBatch(f, list(counts)) if counts is not None else f


def grouped(h, c, rng=None, n_glob=0.0, logits=True, alphas=True, **over):
    """xe_forward_n + saved_alphas + xe_backward of a case on a handle -> (logits, alphas, loss, grads)"""
    d = dict(c, **over)
    from simpleimagecaptionzoo_amd.grouped import xe_forward_n
    lg = xe_forward_n(h, feats_of(d), torch.tensor(d["caps"], device=DEV), d["lens"], d["K"], rng if rng is not None else rng_of(d), d["train"],
                        want_logits=logits)
    al = h.saved_alphas(d["B"] * d["K"], max(d["lens"])) if alphas else None
    grads = h.new_grads()
    loss = h.xe_backward(grads, 0.1, n_glob)
    torch.cuda.synchronize()
    return lg, al, loss, grads


def packed(h, c):
    """the route of the parent: xe_forward + xe_backward on the features repeated K times, rows sorted by length -> (logits [B K, T, V]
    mapped back to img * K + k, loss, grads)"""
    K, lens = c["K"], c["lens"]
    order = xo.sorted_rows(lens)
    ls = [lens[r] for r in order]
    f = torch.tensor(c["feats"], device=DEV).repeat_interleave(K, 0)[order].contiguous()
    masks = None if c["masks"] is None else tuple(m[:, order] for m in c["masks"])
    pk = h.xe_forward(f, torch.tensor(c["caps"][order], device=DEV), ls, rng_of(c, masks), c["train"], want_logits=True)
    grads = h.new_grads()
    loss = h.xe_backward(grads, 0.1)
    torch.cuda.synchronize()
    from oracle import butd as ob
    out = torch.zeros(len(lens), max(lens), pk.shape[1], device=DEV)
    for i, (b, t) in enumerate(ob.packed_order(ls)):
        out[order[b], t] = pk[i]
    return out, loss, grads


def same(a, b):
    (la, aa, lo_a, ga), (lb, ab, lo_b, gb) = a, b
    assert torch.equal(lo_a, lo_b) and all(torch.equal(ga[k], gb[k]) for k in ga)
    assert (la is None or lb is None or torch.equal(la, lb)) and (aa is None or ab is None or torch.equal(aa, ab))


def against_statement(c, got, what):
    lg, al, loss, grads = got
    want = c["want"]
    act = want["active"]
    np.testing.assert_allclose(lg.cpu().numpy(), want["logits"], atol=2e-4, rtol=1e-4, err_msg=what)
    assert not lg.cpu().numpy()[~act].any()                                   # behind a row's end: exactly 0
    assert abs(loss.item() - want["loss"]) < 1e-4, (what, loss.item(), want["loss"])
    assert set(grads) == set(want["grads"])
    for k, v in grads.items():
        close(v, want["grads"][k], what + " " + k)
    if al is not None:
        np.testing.assert_allclose(al.cpu().numpy()[act], want["alphas"][act], atol=1e-4, err_msg=what)


# K = 2, 3, 5, 8 on both goldens, both modes, both attention routes; "cap": the handle holds exactly B K rows
STATEMENT_CASES = [("butd_dec_tiny", 2, True, 0, False), ("butd_dec_tiny", 3, False, 1, False), ("butd_dec_tiny", 5, True, 1, True),
                   ("butd_dec_tiny", 8, True, 0, False), ("butd_dec_odd", 2, False, 0, False), ("butd_dec_odd", 3, True, 1, False),
                   ("butd_dec_odd", 5, False, 0, False), ("butd_dec_odd", 8, True, 1, False)]


@pytest.mark.parametrize("name,K,train,group_att,cap", STATEMENT_CASES)
def test_against_the_statement_and_twice(golden_dir, name, K, train, group_att, cap):
    c = case(golden_dir, name, 3, K, train)
    h = make_handle(c, 3 * K if cap else 32, group_att)
    assert not cap or h.max_rows == 3 * K
    one = grouped(h, c)
    against_statement(c, one, "%s K=%d" % (name, K))
    same(one, grouped(h, c))                                                   # two runs: the same bits
    h.close()


@pytest.mark.parametrize("name,K,train", [("butd_dec_tiny", 3, True), ("butd_dec_odd", 5, False)])
def test_equals_the_packed_route_on_repeated_sorted_features(golden_dir, name, K, train):
    c = case(golden_dir, name, 3, K, train)
    h = make_handle(c)
    lg, _, loss, grads = grouped(h, c)
    plg, ploss, pgrads = packed(h, c)
    np.testing.assert_allclose(lg.cpu().numpy(), plg.cpu().numpy(), atol=2e-4, rtol=1e-4)
    assert abs(loss.item() - ploss.item()) < 1e-4
    for k, v in grads.items():
        close(v, pgrads[k].cpu().double().numpy(), "packed route " + k)
    # and the ordinary route is not moved by the grouped call that ran in between: the same bits before and after, and as on a fresh handle
    again = packed(h, c)
    fresh = packed(make_handle(c), c)
    for other in (again, fresh):
        assert torch.equal(plg, other[0]) and torch.equal(ploss, other[1]) and all(torch.equal(pgrads[k], other[2][k]) for k in pgrads)
    h.close()


def test_token_normaliser_in_its_three_forms(golden_dir):
    c = case(golden_dir, "butd_dec_tiny", 3, 3, True)
    h = make_handle(c)
    N = float(sum(c["lens"]))
    local = grouped(h, c)
    same(local, grouped(h, c, n_glob=N))                                       # the host count is the default
    _, _, l2, g2 = grouped(h, c, n_glob=2 * N)
    assert torch.equal(l2 * 2, local[2])
    for k, v in g2.items():                                                    # doubled: every gradient halves exactly
        assert torch.equal(v * 2, local[3][k]), k
    h.set_mask_sum_global(torch.tensor([2 * N], device=DEV))
    _, _, l3, g3 = grouped(h, c, n_glob=-1.0)                                  # the device scalar
    assert torch.equal(l3, l2) and all(torch.equal(g3[k], g2[k]) for k in g2)
    h.close()


def test_philox_masks_equal_the_regenerated_explicit_masks(golden_dir):
    c = case(golden_dir, "butd_dec_tiny", 3, 3, True)
    R, D, H, E, A, V = c["dims"]
    seed = 0xC0FFEE
    h = make_handle(c)
    by_seed = grouped(h, c, rng=rng_of(c, None, seed))
    _, em, am, om = _philox.butd_rng_arrays(seed, max(c["lens"]), 9, R, E, A, H)     # row r of the B K space, as sample_n's
    same(by_seed, grouped(h, c, rng=rng_of(c, (em, am, om))))
    assert not torch.equal(by_seed[2], grouped(h, c, rng=rng_of(c, None, seed + 1))[2])
    h.close()


@pytest.mark.parametrize("name,K,train", [("butd_dec_tiny", 5, True), ("butd_dec_odd", 2, False)])
def test_group_att_on_equals_off(golden_dir, name, K, train):
    c = case(golden_dir, name, 3, K, train)
    off, on = grouped(make_handle(c, group_att=0), c), grouped(make_handle(c, group_att=1), c)
    np.testing.assert_allclose(on[0].cpu().numpy(), off[0].cpu().numpy(), atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(on[1].cpu().numpy(), off[1].cpu().numpy(), atol=1e-4)
    assert abs(on[2].item() - off[2].item()) < 1e-4
    for k, v in on[3].items():
        close(v, off[3][k].cpu().double().numpy(), "group_att " + k)


@pytest.mark.parametrize("group_att", [0, 1])
def test_region_counts_per_image(golden_dir, group_att):
    """counts 1, 10 and 36: every image as it would be alone on feats[i, :count]"""
    c = case(golden_dir, "butd_dec_tiny", 3, 3, True, counts=(1, 10, 36))
    h = make_handle(c, group_att=group_att)
    got = grouped(h, c)
    against_statement(c, got, "counts")
    al = got[1].cpu().numpy()
    for i, n in enumerate(c["counts"]):
        assert not al[i * 3:(i + 1) * 3, :, n:].any()
    h.close()


def test_the_order_of_the_images_does_not_matter(golden_dir):
    c = case(golden_dir, "butd_dec_odd", 3, 3, True)
    K = 3
    h = make_handle(c)
    lg, al, loss, grads = grouped(h, c)
    img = [2, 0, 1]
    rows = [i * K + k for i in img for k in range(K)]
    plg, pal, ploss, pgrads = grouped(h, c, feats=c["feats"][img], caps=c["caps"][rows], lens=[c["lens"][r] for r in rows],
                                      masks=tuple(m[:, rows] for m in c["masks"]))
    back = np.argsort(rows)
    np.testing.assert_allclose(plg.cpu().numpy()[back], lg.cpu().numpy(), atol=2e-4, rtol=1e-4)
    act = c["want"]["active"]
    np.testing.assert_allclose(pal.cpu().numpy()[back][act], al.cpu().numpy()[act], atol=1e-4)
    assert abs(ploss.item() - loss.item()) < 1e-4
    for k, v in pgrads.items():
        close(v, grads[k].cpu().double().numpy(), "permuted " + k)
    h.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _raw(h, c, B=None, K=None, L=None, lens=None, rng="case", train=1):
    from simpleimagecaptionzoo_amd._lib import lib, ptr, stream_ptr
    B, K = c["B"] if B is None else B, c["K"] if K is None else K
    lens = c["lens"] if lens is None else lens
    f, caps = torch.tensor(c["feats"], device=DEV), torch.tensor(c["caps"], device=DEV)
    r = rng_of(c) if rng == "case" else rng
    st = h._e.xe_forward_n(h._h, ptr(f), ptr(caps), B, K, c["caps"].shape[1] if L is None else L, (C.c_int32 * len(lens))(*lens),
                           C.byref(r) if r is not None else None, train, None, stream_ptr())
    return st, lib().icz_last_error().decode()


def test_every_refusal_leaves_the_handle_as_it_was(golden_dir):
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.grouped import xe_forward_n
    c = case(golden_dir, "butd_dec_tiny", 3, 3, True)
    want = packed(make_handle(c), c)                                           # an ordinary step on a fresh handle
    h = make_handle(c, max_rows=9)
    order = xo.sorted_rows(c["lens"])
    ls = [c["lens"][r] for r in order]
    f = torch.tensor(c["feats"], device=DEV).repeat_interleave(3, 0)[order].contiguous()
    masks = tuple(m[:, order] for m in c["masks"])
    # an ordinary forward pass is stored; the refused grouped calls in between must not touch it
    pk = h.xe_forward(f, torch.tensor(c["caps"][order], device=DEV), ls, rng_of(c, masks), True, want_logits=True)
    bad_len = list(c["lens"])
    bad_len[4] = c["caps"].shape[1]
    for kw, word in ((dict(K=1), "K=1 captions per image outside 2..8"), (dict(K=9), "K=9"), (dict(B=0), "B=0 images"), (dict(L=1), "L=1 columns"),
                     (dict(lens=bad_len), "lengths_host[4]=7 outside 1..6"), (dict(B=4, lens=c["lens"] + [1, 1, 1]), "4 images x 3 captions exceed the row capacity 9"),
                     (dict(rng=None), "training mode needs an icz_rng")):
        st, msg = _raw(h, c, **kw)
        assert st == -1 and word in msg, (kw, msg)
    h.set_scheduled_sampling(0.5)
    st, msg = _raw(h, c)
    assert st == -1 and "scheduled sampling is switched on" in msg, msg
    h.set_scheduled_sampling(0.0)
    grads = h.new_grads()
    loss = h.xe_backward(grads, 0.1)
    torch.cuda.synchronize()
    out = torch.zeros_like(want[0])
    from oracle import butd as ob
    for i, (b, t) in enumerate(ob.packed_order(ls)):
        out[order[b], t] = pk[i]
    assert torch.equal(out, want[0]) and torch.equal(loss, want[1]) and all(torch.equal(grads[k], want[2][k]) for k in grads)
    # weights never refreshed: a handle without bound parameters
    R, D, H, E, A, V = c["dims"]
    bare = ButdHandle(R, D, H, E, A, V, 16, 20)
    st, msg = _raw(bare, c)
    assert st == -1 and "icz_butd_refresh_weights" in msg, msg
    bare.close()
    # the wrapper refuses what it can before it reaches the library
    with pytest.raises(IczError, match="exceed the handle's row capacity 9"):
        xe_forward_n(h, torch.zeros(4, R, D, device=DEV), torch.zeros(12, 7, dtype=torch.int64), [1] * 12, 3)
    with pytest.raises(IczError, match="are not 3 images x 3 rows"):
        xe_forward_n(h, feats_of(c), torch.tensor(c["caps"][:8]), c["lens"][:8], 3)
    h.close()


def test_packed_backward_entries_refuse_a_grouped_forward_by_name(golden_dir):
    from simpleimagecaptionzoo_amd._lib import DistillOpts, IczError, SworOpts, lib, stream_ptr
    c = case(golden_dir, "butd_dec_tiny", 3, 3, True)
    R, D, H, E, A, V = c["dims"]
    h = make_handle(c)
    want = grouped(h, c)
    from simpleimagecaptionzoo_amd.grouped import xe_forward_n
    xe_forward_n(h, feats_of(c), torch.tensor(c["caps"], device=DEV), c["lens"], 3, rng_of(c), True)
    n = sum(c["lens"])
    grads = h.new_grads()
    with pytest.raises(IczError, match="icz_butd_xe_backward_dlogits: the stored forward pass is a grouped one"):
        h.xe_backward_dlogits(torch.zeros(n, V, device=DEV), grads)
    gs = h._grad_struct(grads)
    t_logits = torch.zeros(n, V, device=DEV)
    teacher, ld = (C.c_void_p * 1)(t_logits.data_ptr()), (C.c_int32 * 1)(V)
    o = DistillOpts(1, teacher, ld, None, 0.5, 1.0, 0.1)
    out3 = torch.zeros(3, device=DEV)
    assert lib().icz_butd_xe_backward_distill(h._h, C.byref(o), C.byref(gs), out3.data_ptr(), 0.0, stream_ptr()) == -1
    assert "icz_butd_xe_backward_distill: the stored forward pass is a grouped one" in lib().icz_last_error().decode()
    buf = torch.zeros(64, dtype=torch.float64, device=DEV)
    so = SworOpts(4, 0, 0.0, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None)
    assert lib().icz_butd_xe_backward_swor(h._h, C.byref(so), 9, C.byref(gs), out3.data_ptr(), stream_ptr()) == -1
    assert "icz_butd_xe_backward_swor: the stored forward pass is a grouped one" in lib().icz_last_error().decode()
    # the grouped forward pass is still stored, and its backward pass gives the bits of an undisturbed step
    loss = h.xe_backward(grads, 0.1)
    torch.cuda.synchronize()
    assert torch.equal(loss, want[2]) and all(torch.equal(grads[k], want[3][k]) for k in grads)
    h.close()


# ---- full width ---------------------------------------------------------------------------------------------------------------------
def test_full_width_four_images_by_five_captions_against_the_packed_route():
    """the benchmark's widths, training mode with explicit masks: xe_forward_n + xe_backward against xe_forward + xe_backward on the
    repeated, sorted features -- logits 2e-4 / 1e-4, loss 1e-4 (tests/_fullwidth.py: _butd_xe_case), a gradient tensor within 2e-4 of
    the packed route's largest element + 1e-7 (the device-side part of check_grads_against_float64's rule)"""
    import _fullwidth as fw
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.synth import random_butd_params
    R, D, H, E, A, V = fw.FULL_DIMS
    B, K = 4, 5
    params = random_butd_params(R, D, H, E, A, V, DEV, seed=31)
    params["predict.weight_g"].mul_(6.0)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(2031)
    rs = np.random.RandomState(31)
    caps, lens = xo.batch(rs, V, B, K, 12, pattern=False)
    T = max(lens)
    c = {"feats": torch.relu(torch.randn(B, R, D, generator=gen)).numpy(), "caps": caps, "lens": lens, "K": K, "B": B, "train": True,
         "counts": None, "masks": xo.keep_masks(rs, T, B * K, E, R, A, H)}
    h = ButdHandle(R, D, H, E, A, V, B * K, 20)
    h.bind(params)
    lg, _, loss, grads = grouped(h, c, alphas=False)
    plg, ploss, pgrads = packed(h, c)
    np.testing.assert_allclose(lg.cpu().numpy(), plg.cpu().numpy(), atol=2e-4, rtol=1e-4)
    assert abs(loss.item() - ploss.item()) < 1e-4
    for k, v in grads.items():
        want = pgrads[k].cpu().double().numpy()
        err, scale = float(np.abs(v.cpu().double().numpy() - want).max()), float(np.abs(want).max())
        print("%-32s max|want| %.3e  err/scale %.3e" % (k, scale, err / max(scale, 1e-30)))
        assert err <= 2e-4 * scale + 1e-7, (k, err, scale)
    h.close()


# ---- the Engine ---------------------------------------------------------------------------------------------------------------------
def _params(eng):
    return {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}


def engine_rng(rows, seed, g):
    """explicit masks of a step for `rows` decoder rows, the same for every row: a rank's rows then see what they see in one process"""
    from simpleimagecaptionzoo_amd.butd import make_rng
    B, R, D, H, E, A, V = [int(x) for x in g["dims"]]
    rs = np.random.RandomState(seed)
    row = lambda *s: torch.tensor(np.repeat((rs.rand(20, 1, *s) < 0.5).astype(np.uint8), rows, 1), device=DEV)
    return make_rng(0, None, row(E), row(R, A), row(H))


def test_engine_steps_equal_the_steps_built_by_hand(golden_dir):
    import test_gpu_scst_multisample as tms
    from simpleimagecaptionzoo_amd.butd import make_rng
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    from simpleimagecaptionzoo_amd.grouped import make_batch, xe_forward_n
    g, fx, batches, _ = tms._steps(golden_dir, 1)
    K = 5
    crit = type("Crit", (), {"smoothing": 0.1})()
    eng = tms._engine(g, fx)
    start = _params(eng)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    losses = []
    for s, bt in enumerate(batches):
        losses += eng.training_epoch_grouped([bt], opt, crit, tqdm_visible=False, rngs=[make_rng(40 + s)], captions_per_image=K)
    torch.cuda.synchronize()
    got = _params(eng)
    ref = tms._engine(g, fx)
    ropt = init_optimizer("Adam", ref.model.get_param_groups({"lr": 2e-5}), 2e-5)
    hand = []
    with torch.cuda.stream(ref.stream):
        for s, (ids, _, gts, supp) in enumerate(batches):
            ref.model.train()
            caps, lens = make_batch(ref.caption_vocab, ids, gts, K)
            feats = ref._features(ref.modify_visual_inputs(None, supp))
            h = ref.model._handle()
            xe_forward_n(h, feats, caps, [n - 1 for n in lens], K, make_rng(40 + s), train=True)
            hand.append(h.xe_backward(ref._grads(), 0.1, 0.0).clone())
            ref._apply(ropt, 0.1)
    torch.cuda.synchronize()
    want = _params(ref)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert any(not torch.equal(got[k], start[k]) for k in got)                 # the steps moved the model
    assert len(losses) == len(hand) == 2
    for l, hl in zip(losses, hand):
        assert torch.equal(l, hl) and np.isfinite(l.item()) and l.item() > 0


def dp_reference(golden_dir):
    """the parameters after two grouped steps of one process on all six golden images"""
    import test_gpu_scst_multisample as tms
    from simpleimagecaptionzoo_amd.engine import init_optimizer
    g, fx, batches, _ = tms._steps(golden_dir, 1)
    eng = tms._engine(g, fx)
    opt = init_optimizer("Adam", eng.model.get_param_groups({"lr": 2e-5}), 2e-5)
    crit = type("Crit", (), {"smoothing": 0.1})()
    for s, b in enumerate(batches):
        eng.training_epoch_grouped([b], opt, crit, tqdm_visible=False, rngs=[engine_rng(len(b[0]) * DP_K, 60 + s, g)], captions_per_image=DP_K)
    torch.cuda.synchronize()
    return {k: v.numpy() for k, v in _params(eng).items()}


DP_K = 3


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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "xe_grouped_dp_worker.py")], env=env, stdout=subprocess.PIPE,
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
