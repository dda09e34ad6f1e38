"""Test entries of the kernels of an LSTM decoder step (include/icz.h: icz_test_embed, icz_test_embed_steps, icz_test_lstm_point,
icz_test_lstm_bwd_point): each kernel of csrc/lstm_kernels.h on given operands, with the grid the decoders launch it with.  Arguments
are device tensors (None: a null pointer); nothing is computed here."""
import ctypes as C

from ._lib import LSTM_BWD_POINTERS, LSTM_POINT_POINTERS, DropArgs, LstmBwdArgs, LstmPointArgs, check, lib, ptr, stream_ptr

LSTM_POINT_SCALARS = ("ns", "n_pre", "rows", "H")
LSTM_BWD_SCALARS = ("ns_a", "lda_a", "rows_a", "ns_b", "lda_b", "rows_b", "ns_c", "lda_c", "rows_c", "dc_in_rows", "rows", "H")


def drop(mode=0, mask=None, seed=None, stream=0, step=0, row0=0):
    """icz_test_drop: mode 0 off, 1 keep flags (uint8 device tensor `mask`), 2 Philox (`seed`: a device uint64 / int64 tensor of one
    element); rows < row0 of a forward kernel are not dropped.  The caller keeps mask and seed alive for the call."""
    d = DropArgs()
    d.mode, d.stream, d.step, d.row0 = int(mode), int(stream), int(step), int(row0)
    d.mask = None if mask is None else mask.data_ptr()
    d.seed = None if seed is None else seed.data_ptr()
    return d


def _dp(d):
    return None if d is None else C.byref(d)


def _fill(a, pointers, scalars, kw):
    unknown = set(kw) - set(pointers) - set(scalars)
    assert not unknown, unknown
    for n in pointers:
        if kw.get(n) is not None:
            setattr(a, n, kw[n].data_ptr())
    for n in scalars:
        if n in kw:
            setattr(a, n, int(kw[n]))
    return a


def entry_embed(table, it, emb, rows, relu=1, drop=None, live=None):
    """Test entry icz_test_embed: embed_kernel on `rows` token ids; table [V, E]."""
    V, E = table.shape
    check(lib().icz_test_embed(ptr(table), int(V), int(E), ptr(it), int(rows), ptr(emb), int(relu), _dp(drop), ptr(live), stream_ptr()))


def entry_embed_steps(table, tok, emb, T, B, rows_t, drop=None):
    """Test entry icz_test_embed_steps: embed_steps_kernel over tok [T, B]; rows_t: a host list of T counts."""
    V, E = table.shape
    rt = (C.c_int32 * len(rows_t))(*[int(r) for r in rows_t])
    check(lib().icz_test_embed_steps(ptr(table), int(V), int(E), ptr(tok), int(T), int(B), rt, ptr(emb), _dp(drop), stream_ptr()))


def lstm_point_args(**kw):
    """icz_test_lstm_point_args from device tensors (LSTM_POINT_POINTERS; missing or None: null) and ints (LSTM_POINT_SCALARS)."""
    return _fill(LstmPointArgs(), LSTM_POINT_POINTERS, LSTM_POINT_SCALARS, kw)


def entry_lstm_point(route, drop=None, **kw):
    """Test entry icz_test_lstm_point -> the kernel taken: 1 lstm_point_kernel, 2 lstm_point_gw_kernel (route 0: as launch_lstm_point)."""
    a, out = lstm_point_args(**kw), C.c_int32(0)
    check(lib().icz_test_lstm_point(int(route), C.byref(a), _dp(drop), C.byref(out), stream_ptr()))
    return out.value


def lstm_bwd_args(**kw):
    """icz_test_lstm_bwd_args from device tensors (LSTM_BWD_POINTERS; missing or None: null) and ints (LSTM_BWD_SCALARS)."""
    return _fill(LstmBwdArgs(), LSTM_BWD_POINTERS, LSTM_BWD_SCALARS, kw)


def entry_lstm_bwd_point(drop=None, **kw):
    """Test entry icz_test_lstm_bwd_point: lstm_bwd_point_kernel on given operands."""
    a = lstm_bwd_args(**kw)
    check(lib().icz_test_lstm_bwd_point(C.byref(a), _dp(drop), stream_ptr()))
