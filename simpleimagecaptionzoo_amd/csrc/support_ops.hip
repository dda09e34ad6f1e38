// C entry points that belong to no decoder family (include/icz.h): the clamped Adam update, the route of the embedding gradient
// and the test entries of the kernels that finish a backward pass (support_kernels.h).
#include <math.h>

#include "gemm_ops.h"
#include "support_kernels.h"

using namespace icz;
extern "C" {

int icz_adam_clamp_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                        float clip, int32_t step, void* stream) {
    ICZ_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && step >= 1, "icz_adam_clamp_step: bad arguments");
    const double b1 = 0.9, b2 = 0.999;
    const float bc1 = (float)(1.0 - pow(b1, (double)step));
    const float sbc2 = (float)sqrt(1.0 - pow(b2, (double)step));
    hipLaunchKernelGGL(adam_clamp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                       exp_avg, exp_avg_sq, (size_t)n, lr, clip, bc1, sbc2);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_adam_clamp_multi(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, const int64_t* numel, float lr, float clip, int32_t step, void* stream) {
    ICZ_REQUIRE(count >= 1 && count <= ADAM_MAX_TENSORS, "icz_adam_clamp_multi: count %d out of range 1..%d", count, ADAM_MAX_TENSORS);
    ICZ_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && step >= 1, "icz_adam_clamp_multi: bad arguments");
    AdamTable tab;
    tab.count = count;
    size_t blocks = 0;
    for (int i = 0; i < count; ++i) {
        ICZ_REQUIRE(params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i] && numel[i] > 0, "icz_adam_clamp_multi: tensor %d invalid", i);
        tab.t[i] = {params[i], grads[i], exp_avg[i], exp_avg_sq[i], (size_t)numel[i], blocks};
        blocks += ((size_t)numel[i] + 1023) / 1024;
    }
    const double b1 = 0.9, b2 = 0.999;
    const float bc1 = (float)(1.0 - pow(b1, (double)step));
    const float sbc2 = (float)sqrt(1.0 - pow(b2, (double)step));
    hipLaunchKernelGGL(adam_clamp_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tab, lr, clip, bc1, sbc2);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// ------------------------------------------------------------------------------------------------
// Test entries of the kernels that finish a backward pass (include/icz.h): each checks on the host what its kernel needs of the shape
// and the pointers, fills the kernel's arguments the way the decoders do (tables: blocks job after job) and launches, nothing more.
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int icz_embed_grad_route_for(int32_t n_tok, int32_t E, size_t* lds_bytes_out) {
    ICZ_REQUIRE(n_tok >= 1 && E >= 4 && E % 4 == 0, "icz_embed_grad_route_for: n_tok=%d, E=%d", n_tok, E);
    const int route = embed_grad_route(n_tok);
    ICZ_REQUIRE(route != EG_ROUTE_WIN || E <= 1024, "icz_embed_grad_route_for: the windowed form takes E <= 1024 (n_tok=%d, E=%d)", n_tok, E);
    if (lds_bytes_out) *lds_bytes_out = route == EG_ROUTE_LDS ? embed_grad_lds(n_tok) : 0;
    return route;
}

int icz_test_embed_grad(const int64_t* tok, int32_t n_tok, const float* demb, int32_t ns, int64_t slab_stride, const float* emb, float scale,
                        int32_t E, float* dE, int32_t V, int32_t relu, const int32_t* rows_live, int32_t route, void* stream) {
    const char* who = "icz_test_embed_grad";
    ICZ_REQUIRE(tok && demb && dE && (emb || !relu), "%s: null argument", who);
    ICZ_REQUIRE(n_tok >= 1 && V >= 1 && E >= 4 && E % 4 == 0, "%s: n_tok=%d, V=%d, E=%d (E in whole groups of 4 columns)", who, n_tok, V, E);
    ICZ_REQUIRE(relu == 0 || relu == 1, "%s: relu=%d", who, relu);
    ICZ_REQUIRE(ns >= 1 && slab_stride >= 0 && slab_stride % 4 == 0 && (ns == 1 || slab_stride >= (int64_t)n_tok * E),
                "%s: ns=%d slabs of stride %lld (a multiple of 4, at least n_tok * E)", who, ns, (long long)slab_stride);
    ICZ_REQUIRE(al16(demb) && al16(dE) && (!relu || al16(emb)), "%s: demb, emb and dE must be 16-byte aligned", who);
    ICZ_REQUIRE(route >= 0 && route <= 2, "%s: route=%d", who, route);
    const int r = route ? route : embed_grad_route(n_tok);
    ICZ_REQUIRE(r != EG_ROUTE_WIN || E <= 1024, "%s: the windowed form takes E <= 1024 (E=%d)", who, E);
    ICZ_REQUIRE(r != EG_ROUTE_LDS || embed_grad_lds(n_tok) <= EG_LDS_MAX, "%s: the LDS form holds no list of %d tokens", who, n_tok);
    ICZ_CHECK_HIP(embed_grad_launch((hipStream_t)stream, tok, n_tok, demb, ns, (size_t)slab_stride, emb, scale, E, dE, V, relu, rows_live, route));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_weight_norm(int32_t multi, int32_t count, const float* const* v, const float* const* g, float* const* w, float* const* norm,
                         const int32_t* rows, const int32_t* cols, void* stream) {
    const char* who = "icz_test_weight_norm";
    ICZ_REQUIRE(multi ? count >= 1 && count <= 4 : count == 1, "%s: count %d (table: 1..4 jobs, single: 1)", who, count);
    ICZ_REQUIRE(v && g && w && norm && rows && cols, "%s: null table", who);
    WeightNormTable wt = {};
    int nb = 0;
    for (int i = 0; i < count; ++i) {
        ICZ_REQUIRE(v[i] && g[i] && w[i] && norm[i], "%s: job %d: null pointer", who, i);
        ICZ_REQUIRE(rows[i] >= 1 && cols[i] >= 4 && cols[i] % 4 == 0, "%s: job %d: %d x %d (columns in whole groups of 4)", who, i, rows[i], cols[i]);
        ICZ_REQUIRE(al16(v[i]) && al16(w[i]), "%s: job %d: v and w must be 16-byte aligned", who, i);
        wt.j[wt.count++] = {v[i], g[i], w[i], norm[i], rows[i], cols[i], nb};
        nb += cdiv(rows[i], 4);
    }
    if (multi) hipLaunchKernelGGL(weight_norm_multi_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, wt);
    else launch_weight_norm(v[0], g[0], w[0], norm[0], rows[0], cols[0], (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_weight_norm_bwd(int32_t multi, int32_t count, const float* const* dw, const int32_t* lddw, const float* const* v, const float* const* g,
                             const float* const* norm, float* const* dv, float* const* dg, const int32_t* rows, const int32_t* cols, void* stream) {
    const char* who = "icz_test_weight_norm_bwd";
    ICZ_REQUIRE(multi ? count >= 1 && count <= 4 : count == 1, "%s: count %d (table: 1..4 jobs, single: 1)", who, count);
    ICZ_REQUIRE(dw && lddw && v && g && norm && dv && dg && rows && cols, "%s: null table", who);
    WeightNormBwdTable wt = {};
    int nb = 0;
    for (int i = 0; i < count; ++i) {
        ICZ_REQUIRE(dw[i] && v[i] && g[i] && norm[i] && dv[i] && dg[i], "%s: job %d: null pointer", who, i);
        ICZ_REQUIRE(rows[i] >= 1 && cols[i] >= 4 && cols[i] % 4 == 0, "%s: job %d: %d x %d (columns in whole groups of 4)", who, i, rows[i], cols[i]);
        ICZ_REQUIRE(lddw[i] >= cols[i] && lddw[i] % 4 == 0, "%s: job %d: lddw %d (a multiple of 4, at least %d)", who, i, lddw[i], cols[i]);
        ICZ_REQUIRE(al16(dw[i]) && al16(v[i]) && al16(dv[i]), "%s: job %d: dw, v and dv must be 16-byte aligned", who, i);
        wt.j[wt.count++] = {dw[i], lddw[i], v[i], g[i], norm[i], dv[i], dg[i], rows[i], cols[i], nb};
        nb += cdiv(rows[i], 4);
    }
    if (multi) hipLaunchKernelGGL(weight_norm_bwd_multi_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, wt);
    else launch_weight_norm_bwd(dw[0], lddw[0], v[0], g[0], norm[0], dv[0], dg[0], rows[0], cols[0], (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_transpose(int32_t count, const float* const* src, const int32_t* ld, const int32_t* rows, const int32_t* cols, float* const* dst,
                       void* stream) {
    const char* who = "icz_test_transpose";
    ICZ_REQUIRE(count >= 1 && count <= 4, "%s: count %d outside 1..4", who, count);
    ICZ_REQUIRE(src && ld && rows && cols && dst, "%s: null table", who);
    TransposeTable tt = {};
    int nb = 0;
    for (int i = 0; i < count; ++i) {
        ICZ_REQUIRE(src[i] && dst[i], "%s: job %d: null pointer", who, i);
        ICZ_REQUIRE(rows[i] >= 64 && cols[i] >= 64 && rows[i] % 64 == 0 && cols[i] % 64 == 0, "%s: job %d: %d x %d (whole 64 x 64 tiles)", who, i,
                    rows[i], cols[i]);
        ICZ_REQUIRE(ld[i] >= cols[i] && ld[i] % 4 == 0, "%s: job %d: ld %d (a multiple of 4, at least %d)", who, i, ld[i], cols[i]);
        ICZ_REQUIRE(al16(src[i]) && al16(dst[i]), "%s: job %d: src and dst must be 16-byte aligned", who, i);
        tt.j[tt.count++] = {src[i], ld[i], rows[i], cols[i], dst[i], nb};
        nb += (rows[i] / 64) * (cols[i] / 64);
    }
    hipLaunchKernelGGL(transpose_multi_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, tt);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_colsum(int32_t multi, int32_t count, const float* const* X, const int32_t* K, const int32_t* N, const int32_t* ldx, float* const* out,
                    float* const* out2, void* stream) {
    const char* who = "icz_test_colsum";
    ICZ_REQUIRE(multi ? count >= 1 && count <= 8 : count == 1, "%s: count %d (table: 1..8 jobs, single: 1)", who, count);
    ICZ_REQUIRE(X && K && N && ldx && out, "%s: null table", who);
    ColsumTable ct = {};
    int nb = 0;
    for (int i = 0; i < count; ++i) {
        ICZ_REQUIRE(X[i] && out[i], "%s: job %d: null pointer", who, i);
        ICZ_REQUIRE(K[i] >= 0 && N[i] >= 1 && ldx[i] >= N[i], "%s: job %d: K=%d, N=%d, ldx=%d", who, i, K[i], N[i], ldx[i]);
        ICZ_REQUIRE(multi || !out2 || !out2[i], "%s: the single sum writes no copy", who);
        ct.j[ct.count++] = {X[i], K[i], N[i], ldx[i], out[i], out2 ? out2[i] : nullptr, nb};
        nb += cdiv(N[i], 32);
    }
    if (!multi) return launch_colsum(X[0], K[0], N[0], ldx[0], out[0], (hipStream_t)stream);
    hipLaunchKernelGGL(colsum_multi_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, ct);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_timesum(const float* X, int32_t T, int64_t BN, float* out, void* stream) {
    ICZ_REQUIRE(X && out, "icz_test_timesum: null argument");
    ICZ_REQUIRE(T >= 1 && BN >= 4 && BN % 4 == 0 && BN / 4 <= 0x7fffffff, "icz_test_timesum: T=%d, BN=%lld (whole groups of 4 floats)", T, (long long)BN);
    ICZ_REQUIRE(al16(X) && al16(out), "icz_test_timesum: X and out must be 16-byte aligned");
    launch_timesum(X, T, (size_t)BN, out, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_rowgroup_sum(const float* X, int32_t n_img, int32_t G, int64_t N, float* out, void* stream) {
    ICZ_REQUIRE(X && out, "icz_test_rowgroup_sum: null argument");
    ICZ_REQUIRE(n_img >= 1 && G >= 1 && N >= 4 && N % 4 == 0 && n_img * N / 4 <= 0x7fffffff,
                "icz_test_rowgroup_sum: n_img=%d, G=%d, N=%lld (whole groups of 4 floats)", n_img, G, (long long)N);
    ICZ_REQUIRE(al16(X) && al16(out), "icz_test_rowgroup_sum: X and out must be 16-byte aligned");
    launch_rowgroup_sum(X, n_img, G, (size_t)N, out, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
