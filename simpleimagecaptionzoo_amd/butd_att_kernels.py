"""Test entries of the BUTD soft-attention kernels (include/icz.h: icz_test_att_mean, icz_test_att_scores, icz_test_att_ctx,
icz_test_att_saved_alphas, icz_test_att_bwd_dalpha, icz_test_att_bwd_ddec, icz_test_att_bwd_denc): each kernel of csrc/butd_kernels.h
on given operands, through the launch helper the decoders use.  Arguments are device tensors (None: a null pointer); nothing is
computed here."""
import ctypes as C

from ._lib import (ATT_DDEC_POINTERS, ATT_DENC_POINTERS, ATT_SCORES_POINTERS, AttDdecArgs, AttDencArgs, AttScoresArgs, check, lib, ptr,
                   stream_ptr)
from .lstm_kernels import _dp, _fill, drop  # noqa: F401  (icz_test_drop is shared with the LSTM entries)

ROUTE_PER_ROW, ROUTE_GROUP, ROUTE_GROUP_TRAIN = 0, 1, 2
ATT_SCORES_SCALARS = ("n_img", "nsplit", "rows", "R", "A")
ATT_DDEC_SCALARS = ("n_img", "rows", "R", "A", "nparts")
ATT_DENC_SCALARS = ("n_img", "B", "R", "A", "T", "mode", "mask_step", "stream", "Bs")


def entry_att_mean(feats, n_img, R, D, mean, counts=None):
    """Test entry icz_test_att_mean: mean_feats_kernel, or mean_feats_counts_kernel where counts are given."""
    check(lib().icz_test_att_mean(ptr(feats), int(n_img), int(R), int(D), ptr(counts), ptr(mean), stream_ptr()))


def att_scores_args(**kw):
    """icz_test_att_scores_args from device tensors (ATT_SCORES_POINTERS; missing or None: null) and ints (ATT_SCORES_SCALARS)."""
    return _fill(AttScoresArgs(), ATT_SCORES_POINTERS, ATT_SCORES_SCALARS, kw)


def entry_att_scores(route, drop=None, G=0, parts=0, **kw):
    """Test entry icz_test_att_scores: route 0 att_scores_kernel, 1 att_scores_group_kernel, 2 att_scores_group_train_kernel."""
    a = att_scores_args(**kw)
    check(lib().icz_test_att_scores(int(route), C.byref(a), _dp(drop), int(G), int(parts), stream_ptr()))


def entry_att_ctx(feats, n_img, scores, alpha_out, ctx, rows, R, D, G=0, img_of_row=None, alpha_out2=None, alpha2_stride=0, live=None, counts=None):
    """Test entry icz_test_att_ctx: att_ctx_kernel (G = 0) or att_ctx_group_kernel (G rows per image)."""
    check(lib().icz_test_att_ctx(ptr(feats), int(n_img), ptr(img_of_row), ptr(scores), ptr(alpha_out), ptr(alpha_out2), int(alpha2_stride), ptr(ctx),
                                 int(rows), int(R), int(D), int(G), ptr(live), ptr(counts), stream_ptr()))


def entry_att_saved_alphas(src, T, B, NH, R, out):
    """Test entry icz_test_att_saved_alphas: src [T, B, NH, R] -> out [B, T, R]."""
    check(lib().icz_test_att_saved_alphas(ptr(src), int(T), int(B), int(NH), int(R), ptr(out), stream_ptr()))


def entry_att_bwd_dalpha(dctx, ns, ldc, rows, feats, n_img, R, D, dalpha_part, live=None, img_of_row=None, counts=None):
    """Test entry icz_test_att_bwd_dalpha: dalpha_part [rows][ceil(D / 512)][R]."""
    check(lib().icz_test_att_bwd_dalpha(ptr(dctx), int(ns), int(ldc), int(rows), ptr(feats), int(n_img), int(R), int(D), ptr(dalpha_part), ptr(live),
                                        ptr(img_of_row), ptr(counts), stream_ptr()))


def att_ddec_args(**kw):
    """icz_test_att_ddec_args from device tensors (ATT_DDEC_POINTERS) and ints (ATT_DDEC_SCALARS)."""
    return _fill(AttDdecArgs(), ATT_DDEC_POINTERS, ATT_DDEC_SCALARS, kw)


def entry_att_bwd_ddec(drop=None, **kw):
    """Test entry icz_test_att_bwd_ddec: att_bwd_ddec_kernel on given operands."""
    a = att_ddec_args(**kw)
    check(lib().icz_test_att_bwd_ddec(C.byref(a), _dp(drop), stream_ptr()))


def att_denc_args(**kw):
    """icz_test_att_denc_args from device tensors (ATT_DENC_POINTERS) and ints (ATT_DENC_SCALARS)."""
    return _fill(AttDencArgs(), ATT_DENC_POINTERS, ATT_DENC_SCALARS, kw)


def entry_att_bwd_denc(G=0, parts=0, **kw):
    """Test entry icz_test_att_bwd_denc -> the parts launched: att_bwd_denc_kernel (G = 0) or att_bwd_denc_group_kernel."""
    a, out = att_denc_args(**kw), C.c_int32(0)
    check(lib().icz_test_att_bwd_denc(C.byref(a), int(G), int(parts), C.byref(out), stream_ptr()))
    return out.value
