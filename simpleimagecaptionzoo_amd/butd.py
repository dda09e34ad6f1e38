"""Host-side owner of one libicz BUTD decoder handle (thin: shapes, pointers, stream)."""
import ctypes as C

import torch

from . import _lib
from ._lib import BUTD_PARAM_KEYS, ButdDims, ButdParams, Rng, check, lib, ptr, stream_ptr
from .handle import GraphDecoderHandle
from .regions import RegionSets


def make_rng(seed=0, uniforms=None, emb_mask=None, att_mask=None, out_mask=None):
    """icz_rng: explicit arrays (uint8 keep-masks / fp32 uniforms on the device) or Philox from `seed` for None."""
    r = Rng()
    r.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    keep = []
    for name, t, dt in (("uniforms", uniforms, torch.float32), ("emb_mask", emb_mask, torch.uint8),
                        ("att_mask", att_mask, torch.uint8), ("out_mask", out_mask, torch.uint8)):
        if t is not None:
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise _lib.IczError("%s must be a contiguous %s CUDA tensor" % (name, dt))
            setattr(r, name, t.data_ptr())
            keep.append(t)
    r._keep = keep
    return r


class ButdHandle(RegionSets, GraphDecoderHandle):
    """Wraps icz_butd_* for a fixed architecture (D, H, E, A, V), a region capacity R (<= 128) and row / step capacity.  Features are
    (B, 1..R, D) tensors, or a RegionBatch with the valid count of each image (`regions.py`, icz_butd_set_regions: an image then
    behaves as it would alone at R = its count); the layout is set by the feature check of every call, there is no method to call
    for it.  Alpha outputs are as wide as the batch."""

    family, kind = "butd", 0
    _Params, _param_keys = ButdParams, BUTD_PARAM_KEYS
    _make_rng = staticmethod(make_rng)
    _own_entries = ("create_regions", "set_regions", "step", "sample_n", "xe_forward_n", "sample_mask_sum", "saved_alphas", "sample_backward_dlogp", "xe_backward_dlogits")
    _entry_names = {"set_norm_global": "set_mask_sum_global"}
    _sample_bufs = True

    def __init__(self, R, D, H, E, A, V, max_rows, max_len=20, device="cuda:0"):
        # icz_butd_create keeps its bound of 64 regions; a larger capacity (the 'adaptive' sets) goes through icz_butd_create_regions
        self._create(ButdDims(R, D, H, E, A, V, max_rows, max_len), device, "create_regions" if R > 64 else "create")
        self._regions_init()

    def enable_graphs(self, on=True):
        """Capture greedy / sample / sample_backward into hipGraphs and replay them.  Implies persistent output
        buffers: the tensors returned by those calls are reused (overwritten) by the next call of the same shape."""
        super().enable_graphs(on)

    def set_concurrent(self, on=True):
        self.set_option("concurrent", 1 if on else 0)

    def greedy(self, feats, max_len=20, want_alphas=False):
        """DecoderRNN.sample (Models/BUTD_Model.py:153-189) -> ids (B,max_len) int64 [, alphas (B,max_len,regions)]."""
        feats = self._feats(feats)
        B = feats.shape[0]
        ids = self._buf("greedy_ids", (B, max_len), torch.int64)
        alphas = self._buf("greedy_alphas", (B, max_len, feats.shape[1]), torch.float32) if want_alphas else None
        check(self._e.greedy(self._h, ptr(feats), B, max_len, ptr(ids), ptr(alphas), stream_ptr()))
        return (ids, alphas) if want_alphas else ids

    def sample_n(self, feats, n, max_len=20, rng=None):
        """Beyond the reference: n = 2..8 sampled captions per image (multi-sample SCST, include/icz.h icz_butd_sample_n) ->
        (seq int64 (B n, T), logprobs (B n, T)), row img * n + k.  Row img * n + k draws what row img * n + k of
        sample(feats.repeat_interleave(n, 0), rng) draws; explicit rng arrays are laid out for B n rows.  sample_backward then
        takes a (B n, T) reward."""
        feats = self._feats(feats)
        B, n = feats.shape[0], int(n)
        if not 2 <= n <= 8:          # checked before any buffer is made: nothing is queued on a bad call
            raise _lib.IczError("sample_n: n=%d samples per image outside 2..8" % n)
        if B * n > self.max_rows:
            raise _lib.IczError("sample_n: %d images x %d samples exceed the handle's row capacity %d" % (B, n, self.max_rows))
        rng = rng or make_rng(0)
        seq = self._buf("sample_n_seq", (B * n, max_len), torch.int64)
        lp = self._buf("sample_n_lp", (B * n, max_len), torch.float32)
        check(self._e.sample_n(self._h, ptr(feats), B, n, max_len, C.byref(rng), ptr(seq), ptr(lp), stream_ptr()))
        self._live = (feats, rng, seq, lp)
        return seq, lp

    def sample_mask_sum(self):
        out = torch.zeros(1, device=self.device)
        check(self._e.sample_mask_sum(self._h, ptr(out), stream_ptr()))
        return out

    def sample_backward_dlogp(self, dlogp, grads):
        """BPTT of the last sample() for an upstream gradient d loss / d logprobs (B,T)."""
        dlogp = dlogp.to(device=self.device, dtype=torch.float32).contiguous()
        gs = self._grad_struct(grads)
        check(self._e.sample_backward_dlogp(self._h, ptr(dlogp), C.byref(gs), stream_ptr()))

    def saved_alphas(self, B, T):
        """Attention maps [B, T, regions] of the forward pass the handle holds (the last xe_forward / sample of B rows, T steps)."""
        out = torch.empty(B, T, self.regions, device=self.device)
        check(self._e.saved_alphas(self._h, ptr(out), stream_ptr()))
        return out

    def xe_backward_dlogits(self, dpacked, grads):
        """BPTT of the last xe_forward() for an upstream gradient w.r.t. the packed logits (sum(lengths), V)."""
        dpacked = dpacked.to(device=self.device, dtype=torch.float32).contiguous()
        gs = self._grad_struct(grads)
        check(self._e.xe_backward_dlogits(self._h, ptr(dpacked), C.byref(gs), stream_ptr()))

    def step(self, feats, it, h1, c1, h2, c2):
        """One decoder step from an explicit state (BUTD_Model.py:172-182); state tensors are updated in place.
        Returns (ctx, alpha, logits)."""
        feats = self._feats(feats)
        B = feats.shape[0]
        dev = feats.device
        ctx = torch.empty(B, self.D, device=dev)
        alpha = torch.empty(B, feats.shape[1], device=dev)
        logits = torch.empty(B, self.V, device=dev)
        check(self._e.step(self._h, ptr(feats), B, ptr(it), ptr(h1), ptr(c1), ptr(h2), ptr(c2), ptr(ctx), ptr(alpha), ptr(logits),
                           stream_ptr()))
        return ctx, alpha, logits


def gemm(layout, X, W, bias=None, nsplit=0):
    """Test/bench entry for icz_gemm_f32.  layout 'nt': X[M,K] W[N,K]; 'nn': X[M,K] W[K,N]; 'tn': X[K,M] W[K,N]."""
    code = {"nt": 0, "nn": 1, "tn": 2}[layout]
    if layout == "nt":
        M, K = X.shape
        N = W.shape[0]
    elif layout == "nn":
        M, K = X.shape
        N = W.shape[1]
    else:
        K, M = X.shape
        N = W.shape[1]
    out = torch.empty(M, N, device=X.device, dtype=torch.float32)
    ws = torch.empty(max(lib().icz_gemm_workspace_floats(M, N), max(nsplit, 1) * M * N), device=X.device,
                     dtype=torch.float32)
    check(lib().icz_gemm_f32(code, ptr(X), X.stride(0), ptr(W), W.stride(0), ptr(bias), ptr(out), N, M, N, K,
                             nsplit, ptr(ws), ws.numel(), stream_ptr()))
    return out


def _seg_tables(layout, As, Bs):
    """(nseg, A pointers, lda, B pointers, ldb, K, M, N) of a product over K segments; M, N are None without segments."""
    n = len(As)
    if len(Bs) != n:
        raise _lib.IczError("gemm_seg: %d A segments, %d B segments" % (n, len(Bs)))
    for t in list(As) + list(Bs):
        if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise _lib.IczError("gemm_seg: operands must be 2-d fp32 CUDA tensors with unit column stride")
    M = N = None
    if n:
        M = As[0].shape[1] if layout == "tn" else As[0].shape[0]
        N = Bs[0].shape[0] if layout == "nt" else Bs[0].shape[1]
    Ks = [a.shape[0] if layout == "tn" else a.shape[1] for a in As]
    ap = (C.c_void_p * n)(*[a.data_ptr() for a in As])
    bp = (C.c_void_p * n)(*[b.data_ptr() for b in Bs])
    lda = (C.c_int32 * n)(*[a.stride(0) for a in As])
    ldb = (C.c_int32 * n)(*[b.stride(0) for b in Bs])
    kk = (C.c_int32 * n)(*Ks)
    return n, ap, lda, bp, ldb, kk, M, N


def gemm_seg(layout, As, Bs, bias=None, nsplit=0, out=None, accumulate=False, live=None, workspace=None, raw_slabs=False, info=None):
    """Test/bench entry for icz_gemm_f32_seg: the product over K segments the way a decoder step issues it, C = sum_s A_s B_s (+ bias).
    Segment shapes per layout as for gemm(); every tensor's stride(0) is its leading dimension, so column slices of wider tensors
    work unchanged.  nsplit 0: the split of a decoder step; accumulate: out += product (one split); live: a device int32, 0 = nothing
    is written.  raw_slabs: no C -- returns the slabs [nsplit, M, N] the launch left in `workspace` (one split: the finished product).
    Otherwise returns `out` (a new [M, N] tensor when None).  info: a dict that receives the split that ran as info["nsplit"]."""
    code = {"nt": 0, "nn": 1, "tn": 2}[layout]
    n, ap, lda, bp, ldb, kk, M, N = _seg_tables(layout, As, Bs)
    if M is None:      # no segments: the library refuses; the shape is the output's
        M, N = (int(out.shape[0]), int(out.shape[1])) if out is not None else (1, 1)
    dev = out.device if out is not None else (As[0].device if n else "cuda")
    if out is None and not raw_slabs:
        out = torch.empty(M, N, device=dev, dtype=torch.float32)
    if workspace is None:
        workspace = torch.empty(max(lib().icz_gemm_workspace_floats(M, N), max(nsplit, 1) * M * N), device=dev, dtype=torch.float32)
    used = C.c_int32(0)
    c = None if raw_slabs else out
    check(lib().icz_gemm_f32_seg(code, n, ap, lda, bp, ldb, kk, ptr(bias), ptr(c), c.stride(0) if c is not None else N, M, N, int(nsplit),
                                 1 if accumulate else 0, ptr(live), ptr(workspace), workspace.numel(), C.byref(used), stream_ptr()))
    if info is not None:
        info["nsplit"] = used.value
    return workspace[:used.value * M * N].view(used.value, M, N) if raw_slabs else out


def _ptrs(ts):
    """Host array of the tensors' pointers (None -> NULL)."""
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _i32s(xs):
    return (C.c_int32 * len(xs))(*[int(x) for x in xs])


def embed_grad_route_for(n_tok, E):
    """icz_embed_grad_route_for (host logic, no GPU): (form, dynamic LDS bytes) of the embedding gradient over n_tok list entries --
    1 = the list in LDS, 2 = windowed -- or None where the library refuses."""
    lds = C.c_size_t(0)
    r = int(lib().icz_embed_grad_route_for(int(n_tok), int(E), C.byref(lds)))
    return (r, int(lds.value)) if r > 0 else None


def embed_grad(tok, n_tok, demb, emb, scale, E, dE, V, relu, ns=1, slab_stride=0, rows_live=None, route=0):
    """Test entry for icz_test_embed_grad: dE [V, E] from the list tok [n_tok], demb (ns slabs of stride slab_stride) and emb; the
    tensors are taken as they are (views at any offset), the library checks them."""
    check(lib().icz_test_embed_grad(ptr(tok), int(n_tok), ptr(demb), int(ns), int(slab_stride), ptr(emb), float(scale), int(E), ptr(dE),
                                    int(V), int(relu), ptr(rows_live), int(route), stream_ptr()))


def weight_norm(jobs, multi=True):
    """Test entry for icz_test_weight_norm: jobs = [(v, g, w, norm, rows, cols)]; multi: the table kernel, else the single-matrix one."""
    c = list(zip(*jobs)) if jobs else [()] * 6
    check(lib().icz_test_weight_norm(int(multi), len(jobs), _ptrs(c[0]), _ptrs(c[1]), _ptrs(c[2]), _ptrs(c[3]), _i32s(c[4]), _i32s(c[5]),
                                     stream_ptr()))


def weight_norm_bwd(jobs, multi=True):
    """Test entry for icz_test_weight_norm_bwd: jobs = [(dw, lddw, v, g, norm, dv, dg, rows, cols)]."""
    c = list(zip(*jobs)) if jobs else [()] * 9
    check(lib().icz_test_weight_norm_bwd(int(multi), len(jobs), _ptrs(c[0]), _i32s(c[1]), _ptrs(c[2]), _ptrs(c[3]), _ptrs(c[4]), _ptrs(c[5]),
                                         _ptrs(c[6]), _i32s(c[7]), _i32s(c[8]), stream_ptr()))


def transpose_multi(jobs):
    """Test entry for icz_test_transpose: jobs = [(src, ld, rows, cols, dst)], dst[c, r] = src[r * ld + c]."""
    c = list(zip(*jobs)) if jobs else [()] * 5
    check(lib().icz_test_transpose(len(jobs), _ptrs(c[0]), _i32s(c[1]), _i32s(c[2]), _i32s(c[3]), _ptrs(c[4]), stream_ptr()))


def colsum(jobs, multi=True):
    """Test entry for icz_test_colsum: jobs = [(X, K, N, ldx, out, out2 or None)]; multi: the table kernel, else the single sum."""
    c = list(zip(*jobs)) if jobs else [()] * 6
    check(lib().icz_test_colsum(int(multi), len(jobs), _ptrs(c[0]), _i32s(c[1]), _i32s(c[2]), _i32s(c[3]), _ptrs(c[4]), _ptrs(c[5]),
                                stream_ptr()))


def timesum(X, T, BN, out):
    """Test entry for icz_test_timesum: out[i] = sum_t X[t * BN + i]."""
    check(lib().icz_test_timesum(ptr(X), int(T), int(BN), ptr(out), stream_ptr()))


def rowgroup_sum(X, n_img, G, N, out):
    """Test entry for icz_test_rowgroup_sum: out[i, n] = sum_k X[(i * G + k) * N + n]."""
    check(lib().icz_test_rowgroup_sum(ptr(X), int(n_img), int(G), int(N), ptr(out), stream_ptr()))


def bptt_dh1_step(route, rows, H, A, ddec, w_dec, x1, ns_x1, ld_x1, gates, c_cur, dgates, dc_prev, carry=None, ns_carry=0, rows_carry=0,
                  dc_in=None, c_prev=None, live=None, carry_live=None, x2_slabs=None):
    """Test entry for icz_test_bptt_dh1_step: one "X2, then the TD-LSTM backward" step of the BUTD reverse-time loop; route 1 = the fused
    kernel, 0 = the two launches, -1 = as the loop picks.  Returns (K ranges the library picks for the shape, route taken)."""
    ns, taken = C.c_int32(0), C.c_int32(-1)
    check(lib().icz_test_bptt_dh1_step(int(route), int(rows), int(H), int(A), ptr(ddec), ptr(w_dec), ptr(carry), int(ns_carry), int(rows_carry),
                                       ptr(x1), int(ns_x1), int(ld_x1), ptr(dc_in), ptr(gates), ptr(c_prev), ptr(c_cur), ptr(dgates), ptr(dc_prev),
                                       ptr(live), ptr(carry_live), ptr(x2_slabs), 0 if x2_slabs is None else x2_slabs.numel(), C.byref(ns),
                                       C.byref(taken), stream_ptr()))
    return int(ns.value), int(taken.value)


def adam_clamp_step(p, g, m, v, n, lr, clip, step):
    """icz_adam_clamp_step on the first n floats of four tensors (views at any offset)."""
    check(lib().icz_adam_clamp_step(ptr(p), ptr(g), ptr(m), ptr(v), int(n), float(lr), float(clip), int(step), stream_ptr()))


def adam_clamp_multi(tensors, lr, clip, step):
    """icz_adam_clamp_multi: tensors = [(p, g, m, v, n)], one launch."""
    c = list(zip(*tensors)) if tensors else [()] * 5
    numel = (C.c_int64 * len(tensors))(*[int(n) for n in c[4]])
    check(lib().icz_adam_clamp_multi(len(tensors), _ptrs(c[0]), _ptrs(c[1]), _ptrs(c[2]), _ptrs(c[3]), numel, float(lr), float(clip), int(step),
                                     stream_ptr()))


def gemm_resident_pair(As_a, Bs_a, As_b, Bs_b, slabs_a=None, slabs_b=None, live=None):
    """Test/bench entry for icz_gemm_resident_pair: two NT products over K segments (33..64 rows each) as one launch of the
    resident-activation kernel, what a BPTT step does for its two recurrent dgrad products.  Returns their split-K slabs
    ([nsplit_a, M_a, N_a], [nsplit_b, M_b, N_b]) as views of slabs_a / slabs_b (flat fp32 buffers, allocated when None).  Raises
    where the two problems do not share a stage form of the kernel."""
    ta, tb = _seg_tables("nt", As_a, Bs_a), _seg_tables("nt", As_b, Bs_b)
    bufs = []
    for (n, _, _, _, _, kk, M, N), buf, As in ((ta, slabs_a, As_a), (tb, slabs_b, As_b)):
        if M is None:
            raise _lib.IczError("gemm_resident_pair: a problem without segments")
        if buf is None:       # at most one slab per 256-deep k range
            buf = torch.empty(max(sum(kk) // 256, 1) * M * N, device=As[0].device, dtype=torch.float32)
        bufs.append(buf)
    na, nb = C.c_int32(0), C.c_int32(0)
    args = []
    for (n, ap, lda, bp, ldb, kk, M, N), buf, used in ((ta, bufs[0], na), (tb, bufs[1], nb)):
        args += [n, ap, lda, bp, ldb, kk, M, N, ptr(buf), buf.numel(), C.byref(used)]
    check(lib().icz_gemm_resident_pair(*args, ptr(live), stream_ptr()))
    return tuple(buf[:u.value * t[6] * t[7]].view(u.value, t[6], t[7]) for t, buf, u in ((ta, bufs[0], na), (tb, bufs[1], nb)))


def gemm_set_big_cfg(cfg):
    """icz_gemm_set_big_cfg: -1 per shape (default), 0 the 128 x 128 two-barrier kernel, 1..5 one large-tile configuration, -2 environment."""
    check(lib().icz_gemm_set_big_cfg(int(cfg)))


def gemm_tn_grouped(dY, Xs, outs=None, rows_live=None):
    """Test/bench entry for icz_gemm_tn_grouped: out_j = dY[K,M]^T Xs[j][K,cols_j] in one launch.  Returns the list of outputs."""
    K, M = dY.shape
    n = len(Xs)
    if outs is None:
        outs = [torch.empty(M, x.shape[1], device=dY.device, dtype=torch.float32) for x in Xs]
    xp = (C.c_void_p * n)(*[x.data_ptr() for x in Xs])
    op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    ldx = (C.c_int32 * n)(*[x.stride(0) for x in Xs])
    cols = (C.c_int32 * n)(*[x.shape[1] for x in Xs])
    ldo = (C.c_int32 * n)(*[o.stride(0) for o in outs])
    check(lib().icz_gemm_tn_grouped(ptr(dY), dY.stride(0), M, K, n, xp, ldx, cols, op, ldo, ptr(rows_live), stream_ptr()))
    return outs


def gemm_tn_split_pick(M, N, K):
    """icz_gemm_tn_split_pick (host logic, no GPU): the slabs Butd::wgrad splits dY[K,M]^T X[K,N] into; 1 = shape not taken."""
    return int(lib().icz_gemm_tn_split_pick(int(M), int(N), int(K)))


def gemm_tn_split(dY, X, out=None, workspace=None, rows_live=None):
    """Test/bench entry for icz_gemm_tn_split: out[M,N] = dY[K,M]^T X[K,N] through split-K slabs in `workspace` and their ordered sum
    (what Butd::wgrad does for a weight gradient with few tiles), on the current stream.  Raises where the shape is not taken."""
    K, M = dY.shape
    N = X.shape[1]
    if out is None:
        out = torch.empty(M, N, device=dY.device, dtype=torch.float32)
    if workspace is None:
        workspace = torch.empty(max(gemm_tn_split_pick(M, N, K), 1) * M * N, device=dY.device, dtype=torch.float32)
    check(lib().icz_gemm_tn_split(ptr(dY), dY.stride(0), M, ptr(X), X.stride(0), N, K, ptr(out), out.stride(0), ptr(workspace),
                                  workspace.numel(), ptr(rows_live), stream_ptr()))
    return out


GEMM_ROUTES = ("nt_fp32_mt1", "nt_fp32_mt2", "nt_fp32_mt4", "resident_4stage", "resident_512deep", "resident_128row", "x3_128tile",
               "large_tile", "nn_fp32", "tn_fp32_64", "tn_fp32_128")


def gemm_route_for(layout, M, N, Ks, nsplit=0):
    """icz_gemm_route_for (host logic, no GPU): the name of the kernel a product over the K segments `Ks` is launched on (GEMM_ROUTES),
    None where the library refuses the call."""
    Ks = [int(k) for k in (Ks if isinstance(Ks, (list, tuple)) else [Ks])]
    arr = (C.c_int32 * len(Ks))(*Ks)
    r = int(lib().icz_gemm_route_for({"nt": 0, "nn": 1, "tn": 2}[layout], int(M), int(N), len(Ks), arr, int(nsplit)))
    return GEMM_ROUTES[r] if r >= 0 else None


def gemm_split_for(layout, M, N, Ks, workspace_floats=1 << 40):
    """icz_gemm_split_for (host logic, no GPU): the split gemm_seg takes for nsplit = 0 with that much workspace, None for bad arguments."""
    Ks = [int(k) for k in (Ks if isinstance(Ks, (list, tuple)) else [Ks])]
    arr = (C.c_int32 * len(Ks))(*Ks)
    r = int(lib().icz_gemm_split_for({"nt": 0, "nn": 1, "tn": 2}[layout], int(M), int(N), len(Ks), arr, int(workspace_floats)))
    return r if r >= 1 else None


def gemm_tn_grouped_fits(M, K, cols):
    """icz_gemm_tn_grouped_fits (host logic, no GPU): whether the grouped weight-gradient launch takes these column groups."""
    arr = (C.c_int32 * len(cols))(*[int(c) for c in cols])
    return int(lib().icz_gemm_tn_grouped_fits(int(M), int(K), len(cols), arr)) == 1
