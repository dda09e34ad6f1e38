"""Test entries of the AoA kernels (include/icz.h: icz_test_aoa_layer_norm, icz_aoa_self_attn_route_for, icz_test_aoa_self_attn,
icz_test_aoa_dec_attn, icz_test_aoa_dec_attn_bwd, icz_test_aoa_dkv, icz_test_aoa_ln_bwd, icz_test_aoa_self_attn_bwd): each kernel on given operands, through the launch helpers of the AoA
handle.  Arguments are device tensors (None: a null pointer); nothing is computed here."""
import ctypes as C

from ._lib import DropPArgs, IczError, lib, check, ptr, stream_ptr


def dropp(mode=0, mask=None, seed=None, stream=0, step=0, p=0.0, idx0=0):
    """icz_test_dropp: mode 0 off, 1 keep flags (uint8 device tensor `mask`), 2 Philox (`seed`: a device uint64 / int64 tensor of one
    element).  The caller keeps mask and seed alive for the call."""
    d = DropPArgs()
    d.mode, d.stream, d.step, d.p, d.idx0 = int(mode), int(stream), int(step), float(p), int(idx0)
    d.mask = None if mask is None else mask.data_ptr()
    d.seed = None if seed is None else seed.data_ptr()
    return d


def _dp(d):
    return None if d is None else C.byref(d)


def self_attn_route_for(R, Hd, NH, mha_mfma=True):
    """-> (route, qc, lds bytes) of the refiner self-attention (icz_aoa_self_attn_route_for, host logic only); IczError for a shape
    the handle refuses."""
    qc, lds = C.c_int32(0), C.c_size_t(0)
    route = lib().icz_aoa_self_attn_route_for(int(R), int(Hd), int(NH), int(bool(mha_mfma)), C.byref(qc), C.byref(lds))
    if route < 0:
        raise IczError("libicz status %d: %s" % (route, lib().icz_last_error().decode()))
    return route, qc.value, lds.value


def entry_layer_norm(geometry, x, gain, bias, y, rows, n, stats=None, live=None):
    """Test entry icz_test_aoa_layer_norm: geometry 0 four rows per workgroup (refiner), 1 one wave per workgroup (decoder)."""
    check(lib().icz_test_aoa_layer_norm(int(geometry), ptr(x), ptr(gain), ptr(bias), ptr(y), int(rows), int(n), ptr(stats), ptr(live), stream_ptr()))


def entry_self_attn(route, qkv, o, n_img, R, Hd, NH, counts=None, qc=0, drop=None):
    """Test entry icz_test_aoa_self_attn -> (route, qc) that were launched."""
    r, q = C.c_int32(0), C.c_int32(0)
    check(lib().icz_test_aoa_self_attn(int(route), ptr(qkv), ptr(o), int(n_img), int(R), int(Hd), int(NH), ptr(counts), int(qc), _dp(drop),
                                       C.byref(r), C.byref(q), stream_ptr()))
    return r.value, q.value


def entry_dec_attn(Qp, Kd, Vd, xatt, rows, n_img, R, Hd, NH, qns=1, q_stride=0, q_bias=None, Qp_store=None, img_of_row=None, P_out=None,
                   Pd_out=None, counts=None, drop=None, live=None):
    """Test entry icz_test_aoa_dec_attn."""
    check(lib().icz_test_aoa_dec_attn(ptr(Qp), int(qns), int(q_stride), ptr(q_bias), ptr(Qp_store), ptr(Kd), ptr(Vd), ptr(img_of_row), ptr(xatt),
                                      ptr(P_out), ptr(Pd_out), int(rows), int(n_img), int(R), int(Hd), int(NH), ptr(counts), _dp(drop), ptr(live),
                                      stream_ptr()))


def entry_dkv(dS_all, Pd_all, Qp_all, dx_all, dKd, dVd, n_img, B, T, R, Hd, NH, tc=0, counts=None, G=1):
    """Test entry icz_test_aoa_dkv -> the chunk of (k, t) pairs that was launched (tc 0: the handle's rule)."""
    out = C.c_int32(0)
    check(lib().icz_test_aoa_dkv(ptr(dS_all), ptr(Pd_all), ptr(Qp_all), ptr(dx_all), ptr(dKd), ptr(dVd), int(n_img), int(B), int(T), int(tc), int(R),
                                 int(Hd), int(NH), ptr(counts), int(G), C.byref(out), stream_ptr()))
    return out.value


def entry_dec_attn_bwd(dxq, ns, rows, P, Pd, Qp, Kd, Vd, dQp, dS_out, dx_out, n_img, R, Hd, NH, counts=None, keep_scale=1.0, live=None, img_of_row=None):
    """Test entry icz_test_aoa_dec_attn_bwd."""
    check(lib().icz_test_aoa_dec_attn_bwd(ptr(dxq), int(ns), int(rows), ptr(P), ptr(Pd), ptr(Qp), ptr(Kd), ptr(Vd), ptr(dQp), ptr(dS_out), ptr(dx_out),
                                          int(n_img), int(R), int(Hd), int(NH), ptr(counts), float(keep_scale), ptr(live), ptr(img_of_row), stream_ptr()))


def entry_ln_bwd(form, dq_a, ns_a, dq_b, ns_b, rows, x, gain, dx, n, stats=None, res=None, dq_tot=None, prod=None, live=None):
    """Test entry icz_test_aoa_ln_bwd: form 0 aoa_ln_bwd_kernel (stats, two slab sets), form 1 aoa_ln_bwd_dense_kernel (res, prod)."""
    check(lib().icz_test_aoa_ln_bwd(int(form), ptr(dq_a), int(ns_a), ptr(dq_b), int(ns_b), int(rows), ptr(x), ptr(stats), ptr(gain), ptr(res),
                                    ptr(dq_tot), ptr(prod), ptr(dx), int(n), ptr(live), stream_ptr()))


def entry_self_attn_bwd(qkv, dO, dqkv, n_img, R, Hd, NH, counts=None, drop=None):
    """Test entry icz_test_aoa_self_attn_bwd: dqkv = [dQ | dK | dV] of the refiner self-attention."""
    check(lib().icz_test_aoa_self_attn_bwd(ptr(qkv), ptr(dO), ptr(dqkv), int(n_img), int(R), int(Hd), int(NH), ptr(counts), _dp(drop), stream_ptr()))
