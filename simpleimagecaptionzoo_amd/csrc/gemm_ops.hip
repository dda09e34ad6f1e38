// The GEMM-ops layer (gemm_ops.h): split policy, products to slabs / to a finished output, the slab sum and the column sum, and the
// weight-gradient forms.  Host code around gemm_f32 plus the two small kernels it owns.
#include "gemm_ops.h"

namespace icz {
namespace {

// ---------------------------------------------------------------------------------------------------------
// sum split-K slabs (+ bias):  out[m, n] = sum_z slab[z, m, n] + bias[n]
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slab, int nsplit, size_t MN, int N,
                                                          const float* __restrict__ bias, float* __restrict__ out) {
    size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= MN) return;
    f32x4 s = *reinterpret_cast<const f32x4*>(slab + i);
    for (int z = 1; z < nsplit; ++z) s += *reinterpret_cast<const f32x4*>(slab + (size_t)z * MN + i);
    if (bias) {
        int n = (int)(i % N);
        s += *reinterpret_cast<const f32x4*>(bias + n);
    }
    *reinterpret_cast<f32x4*>(out + i) = s;
}

// ---------------------------------------------------------------------------------------------------------
// out[n] = sum_k X[k, n] (column sums over K rows; bias gradients) in one launch, fixed order -> reproducible.
// Grid (N/32), 256 threads = 32 columns x 8 row groups: thread (c, g) adds rows g, g+8, ... of its column (eight independent
// loads in flight), the eight groups meet in LDS and are added in group order.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ X, int K, int N, int ldx, float* __restrict__ out) {
    __shared__ float part[8][33];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int n = blockIdx.x * 32 + c;
    float s = 0.f;
    if (n < N) {
        const float* x = X + n;
        int k = g;
        for (; k + 56 < K; k += 64) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = x[(size_t)(k + 8 * u) * ldx];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; k < K; k += 8) s += x[(size_t)k * ldx];
    }
    part[g][c] = s;
    __syncthreads();
    if (g == 0 && n < N) {
        float t = part[0][c];
#pragma unroll
        for (int q = 1; q < 8; ++q) t += part[q][c];
        out[n] = t;
    }
}

// what slab_reduce_kernel needs of the shape: float4 steps over M N, and over a row of N when the bias is added
int slab_reduce_check(int M, int N, const float* bias) {
    ICZ_REQUIRE(M > 0 && N > 0 && ((size_t)M * N) % 4 == 0, "slab sum: M*N must be a multiple of 4 (%d x %d)", M, N);
    ICZ_REQUIRE(!bias || N % 4 == 0, "slab sum: the bias is added four columns at a time (N %d)", N);
    return ICZ_OK;
}

}  // namespace

int launch_slab_reduce(const float* slab, int ns, int M, int N, const float* bias, float* out, hipStream_t st) {
    ICZ_REQUIRE(slab && out && ns >= 1, "slab sum: null buffer or %d slabs", ns);
    ICZ_TRY(slab_reduce_check(M, N, bias));
    const size_t MN = (size_t)M * N;
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(cdiv((int)(MN / 4), 256)), dim3(256), 0, st, slab, ns, MN, N, bias, out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int launch_colsum(const float* X, int K, int N, int ldx, float* out, hipStream_t st) {
    hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(N, 32)), dim3(256), 0, st, X, K, N, ldx, out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int gemm_split(GemmLayout layout, const GemmArgs& g, const SplitPolicy& p, size_t cap_floats) {
    if (g.M > p.balance_above) return gemm_pick_split_balanced(g, layout, cap_floats);
    const int ns = gemm_pick_split(g, p.target_wgs, layout);
    return p.fit ? gemm_fit_split(layout, g, ns, cap_floats) : ns;
}

int gemm_slabs(GemmLayout layout, GemmArgs& g, int ns, float* slab, size_t cap_floats, hipStream_t st, const char* who) {
    g.nsplit = ns;
    if (ns > 1) {
        ICZ_REQUIRE(slab && gemm_slab_floats(g.M, g.N, ns) <= cap_floats, "%s: slab buffer too small (%d x %d x %d)", who, ns, g.M, g.N);
        g.out = slab; g.ldo = g.N; g.bias = nullptr; g.accumulate = 0;
    }
    return gemm_f32(layout, g, st);
}

int gemm_slabs(GemmLayout layout, GemmArgs& g, const SplitPolicy& p, float* slab, size_t cap_floats, int* ns_out, hipStream_t st, const char* who) {
    const int ns = gemm_split(layout, g, p, slab ? cap_floats : 0);
    if (ns_out) *ns_out = ns;
    return gemm_slabs(layout, g, ns, slab, cap_floats, st, who);
}

int gemm_finished(GemmLayout layout, GemmArgs& g, const SplitPolicy& p, const float* bias, float* ws, size_t ws_floats, hipStream_t st,
                  const char* who) {
    return gemm_finished(layout, g, gemm_split(layout, g, p, ws ? ws_floats : 0), bias, ws, ws_floats, st, who);
}

int gemm_finished(GemmLayout layout, GemmArgs& g, int ns, const float* bias, float* ws, size_t ws_floats, hipStream_t st, const char* who) {
    if (ns <= 1) {
        g.nsplit = 1; g.bias = bias;
        return gemm_f32(layout, g, st);
    }
    float* const out = g.out;
    ICZ_REQUIRE(g.ldo == g.N, "%s: the slab sum writes a dense output (row stride %d, N %d)", who, g.ldo, g.N);
    ICZ_TRY(slab_reduce_check(g.M, g.N, bias));
    ICZ_TRY(gemm_slabs(layout, g, ns, ws, ws_floats, st, who));
    return launch_slab_reduce(ws, ns, g.M, g.N, bias, out, st);
}

int gemm_tn(const float* dY, int ldy, int M, const float* X, int ldx, int N, int K, float* out, int ldo, int accumulate, const int* rows_live,
            hipStream_t st) {
    GemmArgs g = gemm_args({{dY, X, ldy, ldx, K}}, M, N, out, ldo);
    g.accumulate = accumulate; g.rows_live = rows_live;
    return gemm_f32(GEMM_TN, g, st);
}

int gemm_tn_split_sum(const float* dY, int ldy, int M, const float* X, int ldx, int N, int K, int ns, float* slab, const int* rows_live, float* out,
                      hipStream_t st) {
    ICZ_TRY(gemm_tn_split(dY, ldy, M, X, ldx, N, K, ns, slab, rows_live, st));
    return launch_slab_reduce(slab, ns, M, N, nullptr, out, st);
}

int gemm_tn_auto(const float* dY, int ldy, int M, const float* X, int ldx, int N, int K, float* out, int ldo, float* slab, size_t slab_floats,
                 const int* rows_live, hipStream_t st) {
    if (slab && ldo == N) {
        const int ns = gemm_tn_split_pick(M, N, K);      // > 1 only with M % 4 == 0 and N % 4 == 0: the slab sum's shape
        if (ns > 1 && (size_t)ns * M * N <= slab_floats) return gemm_tn_split_sum(dY, ldy, M, X, ldx, N, K, ns, slab, rows_live, out, st);
    }
    return gemm_tn(dY, ldy, M, X, ldx, N, K, out, ldo, 0, rows_live, st);
}

int gemm_tn_groups(const float* dY, int ldy, int M, int K, const GemmColGroup* groups, int ngroups, float* slab, size_t slab_floats,
                   const int* rows_live, hipStream_t st) {
    if (gemm_tn_grouped_fits(M, K, groups, ngroups)) return gemm_tn_grouped(dY, ldy, M, K, groups, ngroups, rows_live, st);
    for (int j = 0; j < ngroups; ++j) {
        const GemmColGroup& q = groups[j];
        ICZ_TRY(gemm_tn_auto(dY, ldy, M, q.B, q.ldb, q.cols, K, q.out, q.ldo, slab, slab_floats, rows_live, st));
    }
    return ICZ_OK;
}

}  // namespace icz
