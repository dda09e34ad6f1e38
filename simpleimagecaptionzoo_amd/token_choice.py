"""Test entries of the token-choice and loss kernels (include/icz.h: icz_test_greedy_select, icz_test_sample_select, icz_test_ss_select,
icz_test_xe_loss, icz_test_reinforce): each kernel on given logits, through the launch helpers of the decoders.  Arguments are device
tensors (None: a null pointer); nothing is computed here."""
import ctypes as C

from ._lib import SampleSelectArgs, check, lib, ptr, stream_ptr

SAMPLE_SELECT_POINTERS = ("logits", "bias", "logits_store", "uniforms", "seed", "unfinished", "n_unfinished", "seq_out", "logp_out", "it_next",
                          "draw_out", "lse_out", "emb_table", "emb_next", "emb_mask", "live_rows", "ids_out", "g_unfinished", "n_any")
SAMPLE_SELECT_SCALARS = ("V", "ldl", "ns", "slab_stride", "t", "T", "E", "emb_mode", "row0")


def sample_select_max_vocab():
    """The longest row the multinomial and scheduled-sampling kernels take (icz_sample_select_max_vocab, host only)."""
    return lib().icz_sample_select_max_vocab()


def entry_greedy_select(route, logits, rows, V, ldl, ns, slab_stride, bias, table, E, relu, t, T, ids_out, it_next, emb, unfinished=None,
                        n_unfinished=None, part_val=None, part_idx=None):
    """Test entry icz_test_greedy_select: route 1 argmax_part_kernel + embed_argmax_kernel, 2 greedy_select_kernel, 0 as the decoders."""
    check(lib().icz_test_greedy_select(int(route), ptr(logits), int(rows), int(V), int(ldl), int(ns), int(slab_stride), ptr(bias), ptr(table), int(E),
                                       int(relu), int(t), int(T), ptr(ids_out), ptr(it_next), ptr(emb), ptr(unfinished), ptr(n_unfinished),
                                       ptr(part_val), ptr(part_idx), stream_ptr()))


def sample_select_args(**kw):
    """icz_sample_select_args from device tensors (SAMPLE_SELECT_POINTERS; missing or None: null) and ints (SAMPLE_SELECT_SCALARS; ns = 1)."""
    unknown = set(kw) - set(SAMPLE_SELECT_POINTERS) - set(SAMPLE_SELECT_SCALARS)
    assert not unknown, unknown
    a = SampleSelectArgs()
    a.ns = 1
    for n in SAMPLE_SELECT_POINTERS:
        if kw.get(n) is not None:
            setattr(a, n, kw[n].data_ptr())
    for n in SAMPLE_SELECT_SCALARS:
        if n in kw:
            setattr(a, n, int(kw[n]))
    return a


def entry_sample_select(rows, **kw):
    """Test entry icz_test_sample_select: one multinomial step (row0 > 0: the merged greedy + sampled kernel) on `rows` rows."""
    a = sample_select_args(**kw)
    check(lib().icz_test_sample_select(C.byref(a), int(rows), stream_ptr()))


def entry_ss_select(logits_prev, rows, B, V, ldl, t, ss_prob, gate, draw, seed, tok):
    """Test entry icz_test_ss_select: the scheduled-sampling draw of XE step t for the `rows` active rows; gate / draw [T, B] or None (Philox)."""
    check(lib().icz_test_ss_select(ptr(logits_prev), int(rows), int(B), int(V), int(ldl), int(t), float(ss_prob), ptr(gate), ptr(draw), ptr(seed),
                                   ptr(tok), stream_ptr()))


def entry_xe_loss(logits, V, ldl, captions, L, B, T, rows_t, smoothing, n_tokens, n_dev, loss_rows, loss_out):
    """Test entry icz_test_xe_loss: label-smoothing loss and its gradient (in place) over all steps; rows_t: a host list of T counts."""
    rt = (C.c_int32 * len(rows_t))(*[int(r) for r in rows_t])
    check(lib().icz_test_xe_loss(ptr(logits), int(V), int(ldl), ptr(captions), int(L), int(B), int(T), rt, float(smoothing), float(n_tokens),
                                 ptr(n_dev), ptr(loss_rows), ptr(loss_out), stream_ptr()))


def entry_xe_group_loss(logits, V, ldl, captions, L, rows, T, lengths, smoothing, n_tokens, n_dev, loss_rows, loss_out):
    """Test entry icz_test_xe_group_loss: the same loss over image-major rows; lengths: a device int32 tensor of per-row step counts,
    (row, t) active while t < lengths[row]; n_tokens 0: N is their sum."""
    check(lib().icz_test_xe_group_loss(ptr(logits), int(V), int(ldl), ptr(captions), int(L), int(rows), int(T), ptr(lengths), float(smoothing),
                                       float(n_tokens), ptr(n_dev), ptr(loss_rows), ptr(loss_out), stream_ptr()))


def entry_reinforce(logp, seq, reward, B, T, mask_sum_global, coef, loss_out, mask_sum_out, logits, V, ldl, draw, lse, Bs=0, row0=0):
    """Test entry icz_test_reinforce: the REINFORCE loss, its mask sum and the gradient (in place) of a stored rollout."""
    check(lib().icz_test_reinforce(ptr(logp), ptr(seq), ptr(reward), int(B), int(T), ptr(mask_sum_global), ptr(coef), ptr(loss_out),
                                   ptr(mask_sum_out), ptr(logits), int(V), int(ldl), ptr(draw), ptr(lse), int(Bs), int(row0), stream_ptr()))
