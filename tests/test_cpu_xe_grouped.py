"""XE training on K captions per image, host side (include/icz.h: icz_butd_xe_forward_n, icz_test_xe_group_loss;
simpleimagecaptionzoo_amd/grouped.py; Engine.training_epoch_grouped): the argument errors that stand in front of the handle in their
documented order, make_batch against a hand-written encoding, the float64 statement of tests/_xe_grouped_oracle.py against the oracle's
own forward_xe on a batch that is sorted already, the Engine refusals, and the input conditions the GPU tests rely on."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import _xe_grouped_oracle as xo
from oracle import butd as ob


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def _forward_n(feats=True, caps=True, lens=(3, 2, 1, 3), B=2, K=2, L=4, handle=None):
    from simpleimagecaptionzoo_amd._lib import lib
    L_ = lib()
    keep = C.create_string_buffer(256)
    a = C.addressof(keep)
    arr = None if lens is None else (C.c_int32 * len(lens))(*lens)
    st = L_.icz_butd_xe_forward_n(handle, a if feats else None, a if caps else None, B, K, L, arr, None, 0, None, None)
    return st, L_.icz_last_error().decode()


def test_forward_n_refuses_in_the_documented_order_in_front_of_its_handle():
    # every later rule is broken as well: the message names the first one
    st, msg = _forward_n(feats=False, K=9, B=0, L=1)
    assert st == -1 and "null feats, captions or lengths_host" in msg
    for kw in (dict(caps=False), dict(lens=None)):
        st, msg = _forward_n(K=9, B=0, **kw)
        assert st == -1 and "null feats, captions or lengths_host" in msg, msg
    for K in (1, 9, 0, -2):
        st, msg = _forward_n(K=K, B=0, L=1)
        assert st == -1 and "K=%d captions per image outside 2..8" % K in msg, msg
    for kw, word in ((dict(B=0, lens=(9,)), "B=0 images"), (dict(B=-1), "B=-1 images"), (dict(L=1), "L=1 columns"),
                     (dict(lens=(3, 2, 0, 3)), "lengths_host[2]=0 outside 1..3"), (dict(lens=(3, 2, 1, 4)), "lengths_host[3]=4 outside 1..3"),
                     (dict(lens=(1, 1, 1, 1, 1, 9), B=3), "lengths_host[5]=9")):
        st, msg = _forward_n(**kw)
        assert st == -1 and word in msg, (kw, msg)
    for K in (2, 8):       # all of 1 - 3 hold: the handle is looked at next
        st, msg = _forward_n(K=K, B=1, lens=(1,) * K)
        assert st == -1 and "null handle" in msg, msg


def test_group_loss_entry_refuses_on_the_host():
    from simpleimagecaptionzoo_amd._lib import lib
    L = lib()
    keep = C.create_string_buffer(4096)
    a = (C.addressof(keep) + 15) & ~15

    def call(logits=a, V=53, ldl=64, caps=a, Lc=9, rows=4, T=7, lens=a, s=0.1, n=5.0, loss_rows=a):
        st = L.icz_test_xe_group_loss(logits, V, ldl, caps, Lc, rows, T, lens, s, n, None, loss_rows, None, None)
        return st, L.icz_last_error().decode()
    for kw, word in ((dict(logits=None), "null argument"), (dict(lens=None), "null argument"), (dict(loss_rows=None), "null argument"),
                     (dict(V=1), "V=1"), (dict(ldl=52), "ldl=52"), (dict(ldl=54), "ldl=54"), (dict(logits=a + 4), "16-byte aligned"),
                     (dict(T=0), "T=0"), (dict(T=129, Lc=200), "T=129"), (dict(Lc=7), "L=7"), (dict(rows=0), "rows=0"),
                     (dict(s=1.5), "smoothing"), (dict(n=-1.0), "n_tokens")):
        st, msg = call(**kw)
        assert st == -1 and word in msg, (kw, msg)


def test_xe_forward_n_refuses_k_before_it_looks_at_anything():
    from simpleimagecaptionzoo_amd._lib import IczError
    from simpleimagecaptionzoo_amd.butd import ButdHandle
    from simpleimagecaptionzoo_amd.grouped import xe_forward_n
    for K in (1, 9):                               # no handle at all: K is checked before the handle, the features or the library
        with pytest.raises(IczError, match="K=%d captions per image outside 2..8" % K):
            xe_forward_n(None, None, None, None, K)
    assert ButdHandle._entries().xe_forward_n is not None and not hasattr(ButdHandle, "xe_forward_n")      # the handle's surface stays


# ---- make_batch ---------------------------------------------------------------------------------------------------------------------
def _vocab():
    from simpleimagecaptionzoo_amd.vocab import SPECIALS, Caption_Vocabulary
    return Caption_Vocabulary(SPECIALS + ("a", "dog", "runs", "cat", "sits", "on", "mat"))


def test_make_batch_against_a_hand_written_encoding():
    from simpleimagecaptionzoo_amd.grouped import make_batch
    v = _vocab()
    assert [v(w) for w in ("<pad>", "<sta>", "<end>", "<unk>", "a", "dog", "runs", "cat", "sits", "on", "mat")] == list(range(11))
    gts = {7: ["a dog runs", "a zebra runs on a mat", "dog"],                       # three references, K = 2: the third is not taken
           "x": ["cat sits on a mat", "a cat", "a"],
           3: ["quokka", "a dog sits"]}                                             # exactly K
    caps, lengths = make_batch(v, ["x", 7, 3], gts, 2)
    assert caps.dtype == torch.int64 and lengths == [7, 4, 5, 8, 3, 5]
    assert caps.tolist() == [[1, 7, 8, 9, 4, 10, 2, 0],          # image "x" first: the order of img_ids, not of the dictionary
                             [1, 4, 7, 2, 0, 0, 0, 0],
                             [1, 4, 5, 6, 2, 0, 0, 0],
                             [1, 4, 3, 6, 9, 4, 10, 2],          # zebra -> <unk>
                             [1, 3, 2, 0, 0, 0, 0, 0],           # quokka -> <unk>
                             [1, 4, 5, 8, 2, 0, 0, 0]]
    caps3, lengths3 = make_batch(v, [7, "x"], gts, 3, max_len=2)                    # at most two words of every reference
    assert lengths3 == [4, 4, 3, 4, 4, 3] and caps3[1].tolist() == [1, 4, 3, 2] and caps3[5].tolist() == [1, 4, 2, 0]
    with pytest.raises(ValueError, match="image 3 has 2 references, fewer than the 3 captions per image"):
        make_batch(v, [7, 3], gts, 3)
    for k in (1, 9, True, 5.0, "5", None):
        with pytest.raises(ValueError, match="captions per image"):
            make_batch(v, [7], gts, k)
    for m in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="max_len"):
            make_batch(v, [7], gts, 2, max_len=m)
    with pytest.raises(ValueError, match="without images"):
        make_batch(v, [], gts, 2)


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def test_statement_equals_forward_xe_on_a_batch_that_is_sorted_already(golden_dir):
    """B = 2 images x K = 2 with lengths already descending: the statement's rows are forward_xe's rows on the repeated features, its
    loss label_smoothing_loss on them, its gradients autograd's -- float64 against the oracle's fp32 run of the same batch."""
    g = dict(np.load(os.path.join(golden_dir, "butd_dec_tiny.npz")))
    B0, R, D, H, E, A, V = [int(x) for x in g["dims"]]
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd.")}
    rs = np.random.RandomState(5)
    feats = g["feats"][:2]
    caps = np.zeros((4, 6), dtype=np.int64)
    lengths = [5, 4, 4, 2]
    for r, l in enumerate(lengths):
        caps[r, 0], caps[r, 1:l], caps[r, l] = 1, rs.randint(4, V, size=l - 1), 2
    masks = xo.keep_masks(rs, 5, 4, E, R, A, H)
    got = xo.run(sd, feats, caps, lengths, 2, masks, 0.1)
    p = ob.to_params(sd, requires_grad=True)
    packed = ob.forward_xe(torch.from_numpy(feats).repeat_interleave(2, 0), torch.from_numpy(caps), lengths, p, *masks)
    po = ob.packed_order(lengths)
    loss = ob.label_smoothing_loss(packed, torch.tensor([int(caps[b, t + 1]) for b, t in po]), 0.1)
    loss.backward()
    for i, (b, t) in enumerate(po):
        np.testing.assert_allclose(got["logits"][b, t], packed[i].detach().numpy(), atol=2e-5, rtol=1e-5)
    assert not got["logits"][~got["active"]].any() and got["active"].sum() == sum(lengths)
    assert abs(got["loss"] - loss.item()) < 1e-5
    for k, v in p.items():
        scale = max(1e-3, float(np.abs(got["grads"][k]).max()))
        # (+ 1e-7: the affine bias has gradient zero, which the fp32 run leaves as 2e-8 of rounding)
        assert np.abs(got["grads"][k] - v.grad.numpy()).max() <= 2e-5 * scale + 1e-7, k
    assert got["alphas"].shape == (4, 5, R) and np.allclose(got["alphas"][got["active"]].sum(-1), 1.0)
    # the order of the rows does not matter to the statement: the same batch with its rows reversed gives the same rows back
    rev = [3, 2, 1, 0]
    again = xo.run(sd, feats[::-1].copy(), caps[rev], [lengths[r] for r in rev], 2, tuple(m[:, rev] for m in masks), 0.1)
    np.testing.assert_allclose(again["logits"][rev], got["logits"], atol=1e-12)
    assert abs(again["loss"] - got["loss"]) < 1e-12


def test_kernel_statement_on_sorted_lengths_is_the_token_choice_statement():
    """on lengths sorted descending the mask t < len[row] is the prefix mask b < rows_t[t] of _token_choice.xe_ref"""
    import _token_choice as tc
    c = xo.CASE_BY_NAME["v53_7x8_t7"]
    inp = xo.inputs(c, sort=True)
    rows = c.n_img * c.K
    rows_t = [sum(l > t for l in inp["lengths"]) for t in range(c.T)]
    g, gb, lr, rb, loss, lb, act = xo.loss_ref(c, inp)
    fake = tc.Xe("x", rows, c.T, c.V, c.smoothing, None, {})
    ti = {"x": np.nan_to_num(inp["x"][:, :c.V]), "cap": inp["caps"], "rows_t": rows_t, "n_tokens": xo.n_of(inp)}
    g2, gb2, lr2, rb2, loss2, lb2, act2 = tc.xe_ref(fake, ti)
    assert np.array_equal(act, act2) and np.array_equal(g, g2) and np.array_equal(lr, lr2) and loss == loss2
    # the row stride differs (16 against 64 floats of padding): the row-loss bound counts ceil(ldl / 256) additions
    assert np.all(gb == gb2) and np.all(rb <= rb2) and lb <= lb2


# ---- Engine -------------------------------------------------------------------------------------------------------------------------
def test_engine_signature_and_refusals():
    import inspect
    from simpleimagecaptionzoo_amd.engine import AoADetection_Eng, BUTDDetection_Eng, BUTDSpatial_Eng, NIC_Eng
    assert str(inspect.signature(BUTDDetection_Eng.training_epoch_grouped)) == \
        "(self, dataloader, optimizer, criterion, tqdm_visible=True, rngs=None, captions_per_image=5)"
    assert BUTDSpatial_Eng.training_epoch_grouped is BUTDDetection_Eng.training_epoch_grouped and BUTDSpatial_Eng._grouped_xe
    for cls, word in ((AoADetection_Eng, "AoADetection_Eng has no grouped XE forward yet"), (NIC_Eng, "NIC_Eng has no grouped XE forward yet")):
        fake = cls.__new__(cls)            # no constructor: the refusal comes before the model, the stream or the loader is looked at
        with pytest.raises(NotImplementedError, match=word) as e:
            cls.training_epoch_grouped(fake, [], None, None)
        assert "follow-up" in str(e.value)
    fake = BUTDDetection_Eng.__new__(BUTDDetection_Eng)
    for k in (1, 9, True, 5.0, None):
        with pytest.raises(ValueError, match="captions per image"):
            BUTDDetection_Eng.training_epoch_grouped(fake, [], None, None, captions_per_image=k)
    fake.model = types.SimpleNamespace(scheduled_sampling=True, ss_prob=0.25)
    with pytest.raises(ValueError, match="scheduled sampling is live"):
        BUTDDetection_Eng.training_epoch_grouped(fake, [], None, None)


def test_engine_refuses_a_batch_above_the_row_capacity_and_too_few_references_before_device_work():
    from simpleimagecaptionzoo_amd.engine import BUTDDetection_Eng
    fake = BUTDDetection_Eng.__new__(BUTDDetection_Eng)
    touched = []
    fake.model = types.SimpleNamespace(max_rows=9, train=lambda: None)
    fake.caption_vocab = _vocab()
    fake.modify_visual_inputs = lambda *a, **k: touched.append("staged")
    gts = {0: ["a dog", "a cat"], 1: ["a mat", "dog runs"]}
    with pytest.raises(ValueError, match="2 images x 5 captions exceed the handle's row capacity 9"):
        fake._training_epoch_grouped([((0, 1), None, gts, None)], None, None, False, None, 5)
    fake.model.max_rows = 10
    with pytest.raises(ValueError, match="image 0 has 2 references, fewer than the 5"):
        fake._training_epoch_grouped([((0, 1), None, gts, None)], None, None, False, None, 5)
    assert not touched


# ---- what the GPU tests rely on -----------------------------------------------------------------------------------------------------
def test_kernel_cases_hold_the_patterns_they_are_chosen_for():
    seen = collections_counter()
    for c in xo.CASES:
        inp = xo.inputs(c)
        lens, rows, T = inp["lengths"], c.n_img * c.K, c.T
        assert inp["ldl"] == {53: 64, 1000: 1008, 10102: 10112}[c.V] and inp["x"].shape == (T * rows, inp["ldl"])
        assert (c.n_img, c.K) in ((1, 2), (3, 5), (7, 8)) and T in (1, 7)
        assert lens[0] == 1 and lens[1] == T and max(lens) == T
        act = np.array([[lens[r] > t for r in range(rows)] for t in range(T)]).reshape(-1)
        assert np.isnan(inp["x"][~act]).all() and np.isnan(inp["x"][:, c.V:]).all() and np.isfinite(inp["x"][act][:, :c.V]).all()
        if T > 1:
            assert lens != sorted(lens, reverse=True), "lengths not sorted"
            assert (~act).any()
            tg = [int(inp["caps"][r, t + 1]) for t in range(T) for r in range(rows) if lens[r] > t]
            assert 0 in tg and c.V - 1 in tg
            if c.n_img >= 2:
                assert max(lens[(c.n_img - 1) * c.K:]) < T, "an image all of whose rows are shorter than T"
            x = inp["x"][act][:, :c.V]
            top2 = np.sort(x, axis=1)[:, -2:]
            assert ((top2[:, 1] - top2[:, 0]) > 70).any() and (np.ptp(x, axis=1) < 0.02).any()      # a logit 80 above; near uniform
        elif rows > 2:
            assert 0 in lens
        s = xo.inputs(c, sort=True)
        assert s["lengths"] == sorted(lens, reverse=True)
        seen[("s", c.smoothing)] += 1
        seen[("n", c.n)] += 1
        seen[("big", T * rows > 256)] += 1
    assert seen[("s", 0.0)] and seen[("s", 0.1)] and seen[("n", "value")] and seen[("n", "dev")] and seen[("n", "none")] and seen[("big", True)]


def collections_counter():
    import collections
    return collections.Counter()


def test_handle_batches_hold_the_patterns_they_are_chosen_for():
    for B, K, T in ((3, 2, 6), (3, 3, 6), (3, 5, 6), (3, 8, 6)):
        caps, lens = xo.batch(np.random.RandomState(B * 10 + K), 53, B, K, T)
        assert caps.shape == (B * K, T + 1) and lens[0] == 1 and lens[1] == T and max(lens[(B - 1) * K:]) < T
        assert lens != sorted(lens, reverse=True)
        for r, l in enumerate(lens):
            assert caps[r, 0] == 1 and caps[r, l] == 2 and not caps[r, l + 1:].any() and (caps[r, 1:l] >= 4).all()
