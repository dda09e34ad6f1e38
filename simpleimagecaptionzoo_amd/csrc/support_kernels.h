// Family-agnostic device kernels around the decoders: weight norm forward and backward, table transposes, buffer fills, the column,
// time and row-group sums, the embedding gradient and the clamped Adam update, with the launchers their call sites share.
#pragma once
#include "icz_common.h"

namespace icz {
namespace {   // internal linkage: this header is included by several translation units

// ---------------------------------------------------------------------------------------------------------
// weight_norm (old style, dim 0): w[r,:] = v[r,:] * g[r] / ||v[r,:]||   (:43-45, :84).  One wave per row.
// Also keeps ||v[r]|| for the backward pass.  weight_norm_row: the wave's row, for the single layer and the table kernel alike.
__device__ __forceinline__ void weight_norm_row(const float* v, const float* g, float* w, float* norm, int row, int cols) {
    const int lane = threadIdx.x & 63;
    const float* vr = v + (size_t)row * cols;
    float ss = 0.f;
    for (int c = lane * 4; c < cols; c += 256) {
        f32x4 x = *reinterpret_cast<const f32x4*>(vr + c);
        ss += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
    }
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    const float s = g[row] / nrm;
    float* wr = w + (size_t)row * cols;
    for (int c = lane * 4; c < cols; c += 256) {
        f32x4 x = *reinterpret_cast<const f32x4*>(vr + c);
        *reinterpret_cast<f32x4*>(wr + c) = x * s;
    }
    if (lane == 0) norm[row] = nrm;
}
__global__ __launch_bounds__(256) void weight_norm_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                                          float* __restrict__ w, float* __restrict__ norm,
                                                          int rows, int cols) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < rows) weight_norm_row(v, g, w, norm, row, cols);
}
inline void launch_weight_norm(const float* v, const float* g, float* w, float* norm, int rows, int cols, hipStream_t st) {
    hipLaunchKernelGGL(weight_norm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, v, g, w, norm, rows, cols);
}

// The four weight-normed layers of the decoder in ONE launch (blocks laid out job after job, 4 rows per block).
struct WeightNormJob { const float* v; const float* g; float* w; float* norm; int rows, cols, block0; };
struct WeightNormTable { WeightNormJob j[4]; int count; };
__global__ __launch_bounds__(256) void weight_norm_multi_kernel(WeightNormTable tab) {
    int k = 0;
#pragma unroll 1
    for (int i = 1; i < tab.count; ++i)
        if ((int)blockIdx.x >= tab.j[i].block0) k = i;
    const WeightNormJob& jb = tab.j[k];
    const int row = ((int)blockIdx.x - jb.block0) * 4 + (threadIdx.x >> 6);
    if (row < jb.rows) weight_norm_row(jb.v, jb.g, jb.w, jb.norm, row, jb.cols);
}

__global__ void set_scalars_kernel(uint64_t* seed_p, uint64_t seed, float* f_p, float f) {
    if (seed_p) *seed_p = seed;
    if (f_p) *f_p = f;
}

// dst[c][r] = src[r * ld + c] for up to four matrices in one launch (rows, cols multiples of 64; dst row stride = rows): the
// transposed LSTM weight copies behind the per-step dgrad GEMMs of BPTT, refreshed once per optimiser step.
struct TransposeJob { const float* src; int ld, rows, cols; float* dst; int block0; };
struct TransposeTable { TransposeJob j[4]; int count; };
__global__ __launch_bounds__(256) void transpose_multi_kernel(TransposeTable tab) {
    __shared__ float tile[64][65];
    int ji = 0;
    for (int k = 1; k < tab.count; ++k) if ((int)blockIdx.x >= tab.j[k].block0) ji = k;
    const TransposeJob& jb = tab.j[ji];
    const int b = blockIdx.x - jb.block0, ntc = jb.cols / 64;
    const int r0 = (b / ntc) * 64, c0 = (b % ntc) * 64;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = ty + 16 * i;
        const f32x4 v = *reinterpret_cast<const f32x4*>(jb.src + (size_t)(r0 + r) * jb.ld + c0 + 4 * tx);
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[r][4 * tx + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = ty + 16 * i;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tile[4 * tx + e][c];
        *reinterpret_cast<f32x4*>(jb.dst + (size_t)(c0 + c) * jb.rows + r0 + 4 * tx) = v;
    }
}

// zero up to 8 float buffers of n floats each (n % 4 == 0) in one launch (recurrent-state resets)
struct ZeroList { float* p[8]; int count; };
__global__ __launch_bounds__(256) void zero_bufs_kernel(ZeroList z, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < z.count; ++k) *reinterpret_cast<f32x4*>(z.p[k] + i) = zero;
}

__global__ void fill_i64_kernel(int64_t* p, int64_t v, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// out[i, n] = sum_{k < G} X[i G + k, n], added in k order (multi-sample SCST: the G sampled rows of an image folded onto it).
// N % 4 == 0; one thread per 4 consecutive columns.
__global__ __launch_bounds__(256) void rowgroup_sum_kernel(const float* __restrict__ X, int n_img, int G, size_t N, float* __restrict__ out) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= (size_t)n_img * N) return;
    const size_t img = i / N, n = i % N;
    const float* x = X + img * G * N + n;
    f32x4 s = *reinterpret_cast<const f32x4*>(x);
    for (int k = 1; k < G; ++k) s += *reinterpret_cast<const f32x4*>(x + (size_t)k * N);
    *reinterpret_cast<f32x4*>(out + i) = s;
}
inline void launch_rowgroup_sum(const float* X, int n_img, int G, size_t N, float* out, hipStream_t st) {
    hipLaunchKernelGGL(rowgroup_sum_kernel, dim3(cdiv((int)((size_t)n_img * N / 4), 256)), dim3(256), 0, st, X, n_img, G, N, out);
}

constexpr int SAMPLE_N_MAX_K = 8;      // rows per image of the AoA / NIC multi-sample rollouts (icz_aoa_sample_n, icz_nic_sample_n)
// img[row] = row / G: the image of each decoder row of a multi-sample rollout (row = img * G + k; the AoA and NIC rollouts)
__global__ void row_image_kernel(int32_t* __restrict__ img, int rows, int G) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) img[i] = i / G;
}

// ---------------------------------------------------------------------------------------------------------
// Several column sums in ONE launch (the bias gradients at the end of BPTT; a single sum is launch_colsum, gemm_ops.h, with the same
// scheme: 32 columns x 8 row groups per block, the groups added in group order): blocks laid out job after job; out2 (optional)
// receives a copy (b_ih and b_hh have the same gradient); a job with K = 0 writes zeros.
struct ColsumJob { const float* X; int K, N, ldx; float* out; float* out2; int block0; };
struct ColsumTable { ColsumJob j[8]; int count; };
__global__ __launch_bounds__(256) void colsum_multi_kernel(ColsumTable tab) {
    __shared__ float part[8][33];
    int k = 0;
#pragma unroll 1
    for (int i = 1; i < tab.count; ++i)
        if ((int)blockIdx.x >= tab.j[i].block0) k = i;
    const ColsumJob& jb = tab.j[k];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int n = ((int)blockIdx.x - jb.block0) * 32 + c;
    float s = 0.f;
    if (n < jb.N) {
        const float* x = jb.X + n;
        int kk = g;
        for (; kk + 56 < jb.K; kk += 64) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = x[(size_t)(kk + 8 * u) * jb.ldx];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; kk < jb.K; kk += 8) s += x[(size_t)kk * jb.ldx];
    }
    part[g][c] = s;
    __syncthreads();
    if (g == 0 && n < jb.N) {
        float t = part[0][c];
#pragma unroll
        for (int q = 1; q < 8; ++q) t += part[q][c];
        jb.out[n] = t;
        if (jb.out2) jb.out2[n] = t;
    }
}

// out[b, n] = sum_t X[t, b, n]   (time sum of the TD gate gradients for the hoisted mean-feature weights)
__global__ __launch_bounds__(256) void timesum_kernel(const float* __restrict__ X, int T, size_t BN, float* __restrict__ out) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= BN) return;
    f32x4 s = *reinterpret_cast<const f32x4*>(X + i);
    for (int t = 1; t < T; ++t) s += *reinterpret_cast<const f32x4*>(X + (size_t)t * BN + i);
    *reinterpret_cast<f32x4*>(out + i) = s;
}
inline void launch_timesum(const float* X, int T, size_t BN, float* out, hipStream_t st) {
    hipLaunchKernelGGL(timesum_kernel, dim3(cdiv((int)(BN / 4), 256)), dim3(256), 0, st, X, T, BN, out);
}

// ---------------------------------------------------------------------------------------------------------
// Embedding gradient (Embedding -> ReLU -> Dropout backward):
//   dE[v,:] = sum over (t,b) with tok[t,b] == v of demb[t,b,:] * (emb[t,b,:] > 0 ? scale : 0)
// No atomics: a workgroup takes 8 vocabulary rows.  The (t,b) token list is loaded into LDS once per workgroup and each wave
// finds the occurrences of two of the rows by ballot, in list order.  Then wave w adds the rows' occurrences for the columns
// 256 w .. 256 w + 255 (+ 1024 k), in list order, eight occurrences' loads in flight: the kernel lasts as long as its most
// frequent token (<sta> once per caption; in XE batches the most frequent word), so its chain of dependent loads is what to
// keep short.  Rows without occurrences (almost all of them) are written as zeros.
constexpr int EG_ROWS = 8;
__global__ __launch_bounds__(256) void embed_grad_kernel(const int64_t* __restrict__ tok, int n_tok,
                                                         const float* __restrict__ demb, int ns, size_t slab_stride,
                                                         const float* __restrict__ emb, float scale, int E,
                                                         float* __restrict__ dE, int V, int relu, const int* __restrict__ rows_live) {
    extern __shared__ int eg_sm[];     // tokens [n_tok], then the occurrence lists of the eight rows [8][n_tok]
    __shared__ int snh[EG_ROWS];
    int* stok = eg_sm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (rows_live) n_tok = min(n_tok, *rows_live);       // the (t, b) prefix of the steps a sampled rollout really ran (d emb rows behind it are stale)
    for (int i = tid; i < n_tok; i += 256) stok[i] = (int)tok[i];
    __syncthreads();
    for (int rr = 0; rr < EG_ROWS / 4; ++rr) {
        const int row8 = wave + 4 * rr, v = blockIdx.x * EG_ROWS + row8;
        int* hits = eg_sm + n_tok + row8 * n_tok;
        int nh = 0;
        for (int i0 = 0; i0 < n_tok; i0 += 64) {
            const int i = i0 + lane;
            const bool m = i < n_tok && stok[i] == v;
            const unsigned long long bal = __ballot(m);
            if (m) hits[nh + __popcll(bal & ((1ull << lane) - 1ull))] = i;
            nh += __popcll(bal);
        }
        if (lane == 0) snh[row8] = nh;
    }
    __syncthreads();
    for (int row8 = 0; row8 < EG_ROWS; ++row8) {
        const int v = blockIdx.x * EG_ROWS + row8;
        if (v >= V) break;
        const int nh = snh[row8];
        const int* hits = eg_sm + n_tok + row8 * n_tok;
        for (int e = 256 * wave + lane * 4; e < E; e += 1024) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            for (int h0 = 0; h0 < nh; h0 += 8) {
                f32x4 g[8], x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const size_t off = (size_t)hits[min(h0 + u, nh - 1)] * E + e;
                    g[u] = sum_slabs4(demb, ns, slab_stride, off);
                    if (relu) x[u] = *reinterpret_cast<const f32x4*>(emb + off);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (h0 + u < nh) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) s[j] += (!relu || x[u][j] > 0.f) ? g[u][j] * scale : 0.f;
                    }
            }
            *reinterpret_cast<f32x4*>(dE + (size_t)v * E + e) = s;
        }
    }
}
// The same for token lists longer than embed_grad_kernel's LDS holds (more than ~4500 (t, b) pairs: the multi-sample rollout's B K rows
// x T steps).  The list is walked in windows of EG_WIN tokens: per window each wave finds the occurrences of two of the rows (ballot,
// list order), then every wave adds them for its columns; the partial sums are carried across windows in registers -- the same
// additions in the same order as embed_grad_kernel (the same bits: tests/test_gpu_support_kernels.py runs both on one list).  E <= 1024
// (one group of four columns per lane).
constexpr int EG_WIN = 1024;
__global__ __launch_bounds__(256) void embed_grad_win_kernel(const int64_t* __restrict__ tok, int n_tok,
                                                             const float* __restrict__ demb, int ns, size_t slab_stride,
                                                             const float* __restrict__ emb, float scale, int E,
                                                             float* __restrict__ dE, int V, int relu, const int* __restrict__ rows_live) {
    __shared__ int stok[EG_WIN];
    __shared__ int shits[EG_ROWS][EG_WIN];
    __shared__ int snh[EG_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (rows_live) n_tok = min(n_tok, *rows_live);
    const int e = 256 * wave + lane * 4;
    const bool ev = e < E;
    f32x4 s[EG_ROWS];
#pragma unroll
    for (int r = 0; r < EG_ROWS; ++r) s[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int w0 = 0; w0 < n_tok; w0 += EG_WIN) {
        const int nw = min(EG_WIN, n_tok - w0);
        __syncthreads();                                  // the previous window's lists have been read
        for (int i = tid; i < nw; i += 256) stok[i] = (int)tok[w0 + i];
        __syncthreads();
        for (int rr = 0; rr < EG_ROWS / 4; ++rr) {
            const int row8 = wave + 4 * rr, v = blockIdx.x * EG_ROWS + row8;
            int nh = 0;
            for (int i0 = 0; i0 < nw; i0 += 64) {
                const int i = i0 + lane;
                const bool m = i < nw && stok[i] == v;
                const unsigned long long bal = __ballot(m);
                if (m) shits[row8][nh + __popcll(bal & ((1ull << lane) - 1ull))] = w0 + i;
                nh += __popcll(bal);
            }
            if (lane == 0) snh[row8] = nh;
        }
        __syncthreads();
#pragma unroll
        for (int row8 = 0; row8 < EG_ROWS; ++row8) {
            const int nh = snh[row8];
            if (!ev) continue;
            for (int h0 = 0; h0 < nh; h0 += 8) {
                f32x4 g[8], x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const size_t off = (size_t)shits[row8][min(h0 + u, nh - 1)] * E + e;
                    g[u] = sum_slabs4(demb, ns, slab_stride, off);
                    if (relu) x[u] = *reinterpret_cast<const f32x4*>(emb + off);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (h0 + u < nh) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) s[row8][j] += (!relu || x[u][j] > 0.f) ? g[u][j] * scale : 0.f;
                    }
            }
        }
    }
#pragma unroll
    for (int row8 = 0; row8 < EG_ROWS; ++row8) {
        const int v = blockIdx.x * EG_ROWS + row8;
        if (v < V && ev) *reinterpret_cast<f32x4*>(dE + (size_t)v * E + e) = s[row8];
    }
}

// host side: grid, LDS size (above the 64 KB default the kernel needs the explicit opt-in); longer token lists: the windowed form.
// route: 0 = by the list's length (every decoder), 1 = embed_grad_kernel, 2 = embed_grad_win_kernel (icz_test_embed_grad); a forced
// form that cannot take the shape is refused.
constexpr int EG_ROUTE_LDS = 1, EG_ROUTE_WIN = 2;
constexpr size_t EG_LDS_MAX = 160 * 1024 - 1024;
inline size_t embed_grad_lds(int n_tok) { return sizeof(int) * (1 + EG_ROWS) * (size_t)n_tok; }
inline int embed_grad_route(int n_tok) { return embed_grad_lds(n_tok) > EG_LDS_MAX ? EG_ROUTE_WIN : EG_ROUTE_LDS; }
inline hipError_t embed_grad_launch(hipStream_t st, const int64_t* tok, int n_tok, const float* demb, int ns, size_t slab_stride,
                                    const float* emb, float scale, int E, float* dE, int V, int relu, const int* rows_live = nullptr,
                                    int route = 0) {
    const size_t lds = embed_grad_lds(n_tok);
    if (route == 0) route = embed_grad_route(n_tok);
    if (route != EG_ROUTE_WIN && lds > EG_LDS_MAX) return hipErrorInvalidValue;
    if (route == EG_ROUTE_WIN) {
        if (E > 1024 || E % 4 != 0) return hipErrorInvalidValue;
        hipLaunchKernelGGL(embed_grad_win_kernel, dim3((V + EG_ROWS - 1) / EG_ROWS), dim3(256), 0, st, tok, n_tok, demb, ns, slab_stride, emb, scale,
                           E, dE, V, relu, rows_live);
        return hipSuccess;
    }
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(embed_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(embed_grad_kernel, dim3((V + EG_ROWS - 1) / EG_ROWS), dim3(256), lds, st, tok, n_tok, demb, ns, slab_stride, emb, scale, E, dE,
                       V, relu, rows_live);
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------------------
// weight_norm backward (one wave per row):  w = g v / ||v||
//   dg[r] = dw[r,:] . v[r,:] / ||v||;   dv[r,:] = (g/||v||) (dw[r,:] - (dg/||v||) v[r,:])
// weight_norm_bwd_row: the wave's row, for the single layer and the table kernel alike.
__device__ __forceinline__ void weight_norm_bwd_row(const float* dw, int lddw, const float* v, const float* g, const float* norm, float* dv, float* dg,
                                                    int row, int cols) {
    const int lane = threadIdx.x & 63;
    const float* vr = v + (size_t)row * cols;
    const float* dr = dw + (size_t)row * lddw;
    float dot = 0.f;
    for (int c = lane * 4; c < cols; c += 256) {
        f32x4 x = *reinterpret_cast<const f32x4*>(vr + c);
        f32x4 d = *reinterpret_cast<const f32x4*>(dr + c);
        dot += x[0] * d[0] + x[1] * d[1] + x[2] * d[2] + x[3] * d[3];
    }
    dot = wave_sum(dot);
    const float nrm = norm[row];
    const float dgv = dot / nrm;
    const float s = g[row] / nrm;
    float* o = dv + (size_t)row * cols;
    for (int c = lane * 4; c < cols; c += 256) {
        f32x4 x = *reinterpret_cast<const f32x4*>(vr + c);
        f32x4 d = *reinterpret_cast<const f32x4*>(dr + c);
        *reinterpret_cast<f32x4*>(o + c) = (d - x * (dgv / nrm)) * s;
    }
    if (lane == 0) dg[row] = dgv;
}
__global__ __launch_bounds__(256) void weight_norm_bwd_kernel(const float* __restrict__ dw, int lddw, const float* __restrict__ v,
                                                              const float* __restrict__ g, const float* __restrict__ norm,
                                                              float* __restrict__ dv, float* __restrict__ dg, int rows, int cols) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < rows) weight_norm_bwd_row(dw, lddw, v, g, norm, dv, dg, row, cols);
}
inline void launch_weight_norm_bwd(const float* dw, int lddw, const float* v, const float* g, const float* norm, float* dv, float* dg, int rows,
                                   int cols, hipStream_t st) {
    hipLaunchKernelGGL(weight_norm_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, dw, lddw, v, g, norm, dv, dg, rows, cols);
}

// The attention block's three weight-normed layers in ONE launch (blocks job after job, 4 rows per block).
struct WeightNormBwdJob { const float* dw; int lddw; const float* v; const float* g; const float* norm; float* dv; float* dg; int rows, cols, block0; };
struct WeightNormBwdTable { WeightNormBwdJob j[4]; int count; };
__global__ __launch_bounds__(256) void weight_norm_bwd_multi_kernel(WeightNormBwdTable tab) {
    int k = 0;
#pragma unroll 1
    for (int i = 1; i < tab.count; ++i)
        if ((int)blockIdx.x >= tab.j[i].block0) k = i;
    const WeightNormBwdJob& jb = tab.j[k];
    const int row = ((int)blockIdx.x - jb.block0) * 4 + (threadIdx.x >> 6);
    if (row < jb.rows) weight_norm_bwd_row(jb.dw, jb.lddw, jb.v, jb.g, jb.norm, jb.dv, jb.dg, row, jb.cols);
}

// ---------------------------------------------------------------------------------------------------------
// clip_gradient (Utils.py:241-250) + Adam (Utils.py:219-220) of ONE element, the only statement of the update: adam_clamp_kernel and
// both paths of adam_clamp_multi_kernel call it, and the three fused multiply-adds are written out -- left to the compiler's
// contraction, the 16-byte path fused m and v while the one-element sites did not, and the same element came out with other bits
// depending on its tensor's alignment (tests/test_gpu_support_kernels.py).  These are the bits of the 16-byte path.
__device__ __forceinline__ void adam_clamp_update(float g, float& m, float& v, float& p, float lr, float clip, float bc1, float sqrt_bc2) {
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
    const float gv = fminf(fmaxf(g, -clip), clip);
    m = __builtin_fmaf(m, b1, gv * (1.f - b1));
    v = __builtin_fmaf(v, b2, (gv * gv) * (1.f - b2));
    p = __builtin_fmaf(-(lr / bc1), m / (sqrtf(v) / sqrt_bc2 + eps), p);
}

// The update over a table of tensors in ONE launch (21 parameter tensors per step otherwise cost 21 launches).
struct AdamTensor { float* p; const float* g; float* m; float* v; size_t n; size_t block0; };
constexpr int ADAM_MAX_TENSORS = 32;
struct AdamTable { AdamTensor t[ADAM_MAX_TENSORS]; int count; };
__global__ __launch_bounds__(256) void adam_clamp_multi_kernel(AdamTable tab, float lr, float clip, float bc1, float sqrt_bc2) {
    // find the tensor of this block (blocks are laid out tensor after tensor)
    int k = 0;
#pragma unroll 1
    for (int i = 1; i < tab.count; ++i)
        if (blockIdx.x >= tab.t[i].block0) k = i;
    const AdamTensor T = tab.t[k];
    const size_t i = ((size_t)blockIdx.x - T.block0) * 1024 + threadIdx.x * 4;
    if (i >= T.n) return;
    if (i + 4 <= T.n && (((uintptr_t)(T.p + i) | (uintptr_t)(T.g + i) | (uintptr_t)(T.m + i) | (uintptr_t)(T.v + i)) & 15) == 0) {
        f32x4 g = *reinterpret_cast<const f32x4*>(T.g + i), m = *reinterpret_cast<f32x4*>(T.m + i);
        f32x4 v = *reinterpret_cast<f32x4*>(T.v + i), p = *reinterpret_cast<f32x4*>(T.p + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float me = m[e], ve = v[e], pe = p[e];
            adam_clamp_update(g[e], me, ve, pe, lr, clip, bc1, sqrt_bc2);
            m[e] = me; v[e] = ve; p[e] = pe;
        }
        *reinterpret_cast<f32x4*>(T.m + i) = m;
        *reinterpret_cast<f32x4*>(T.v + i) = v;
        *reinterpret_cast<f32x4*>(T.p + i) = p;
    } else {      // a tensor's tail, or a tensor that is not 16-byte aligned
        for (size_t e = i; e < T.n && e < i + 4; ++e) {
            float me = T.m[e], ve = T.v[e], pe = T.p[e];
            adam_clamp_update(T.g[e], me, ve, pe, lr, clip, bc1, sqrt_bc2);
            T.m[e] = me; T.v[e] = ve; T.p[e] = pe;
        }
    }
}

// The update of one tensor, one element per thread.
__global__ __launch_bounds__(256) void adam_clamp_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, size_t n, float lr, float clip, float bc1,
                                                         float sqrt_bc2) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float me = m[i], ve = v[i], pe = p[i];
    adam_clamp_update(g[i], me, ve, pe, lr, clip, bc1, sqrt_bc2);
    m[i] = me;
    v[i] = ve;
    p[i] = pe;
}

}  // namespace
}  // namespace icz
