// Device kernels of the BUTD soft attention: the mean over regions, attention scores, softmax and context (per row and grouped
// per image), their backward kernels and the saved attention maps.  HBM-bound byte movers: coalesced 16-byte accesses, wave-shuffle
// reductions, no atomics (bitwise reproducible).  Reference line numbers: Models/BUTD_Model.py.
// Every kernel here is launched through a helper of butd_impl.h (saved_alphas: below) and tested alone on given operands through the
// icz_test_att_* entries (butd_att_test_entries.hip): tests/test_gpu_butd_att_kernels.py holds each to a float64 reference under an
// a-priori rounding bound, and the promises made in the comments below -- no load outside the operands, nothing read or written behind
// an image's count, <true> = <false> at R = c, grouped = per row -- to bits.
#pragma once
#include "icz_common.h"
#include "rng.h"

namespace icz {
namespace {   // internal linkage: this header is included by several translation units

// ---------------------------------------------------------------------------------------------------------
// mean over regions (:117,:167,:205,:251): mean[b,d] = sum_r feats[b,r,d] / R
__global__ __launch_bounds__(256) void mean_feats_kernel(const float* __restrict__ feats, float* __restrict__ mean,
                                                         int R, int D) {
    const int b = blockIdx.y;
    const int d = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (d >= D) return;
    const float* f = feats + (size_t)b * R * D + d;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < R; ++r) s += *reinterpret_cast<const f32x4*>(f + (size_t)r * D);
    const float fr = (float)R;
    f32x4 o = {s[0] / fr, s[1] / fr, s[2] / fr, s[3] / fr};
    *reinterpret_cast<f32x4*>(mean + (size_t)b * D + d) = o;
}

// The same over an adaptive region set (icz_butd_set_regions): image b has counts[b] valid leading rows of its R-row block; the
// mean is their sum, in row order, over counts[b] -- what the kernel above gives the image alone at R = counts[b].  Pad rows are not read.
__global__ __launch_bounds__(256) void mean_feats_counts_kernel(const float* __restrict__ feats, float* __restrict__ mean,
                                                                int R, int D, const int32_t* __restrict__ counts) {
    const int b = blockIdx.y;
    const int d = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (d >= D) return;
    const int Rc = counts ? counts[b] : R;
    const float* f = feats + (size_t)b * R * D + d;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < Rc; ++r) s += *reinterpret_cast<const f32x4*>(f + (size_t)r * D);
    const float fr = (float)Rc;
    f32x4 o = {s[0] / fr, s[1] / fr, s[2] / fr, s[3] / fr};
    *reinterpret_cast<f32x4*>(mean + (size_t)b * D + d) = o;
}

// ---------------------------------------------------------------------------------------------------------
// SoftAttention scores (:57-59):  score[row,r] = w_aff . drop(relu(enc_ctx[img,r,:] + dec_ctx[row,:])) + b_aff
// with dec_ctx[row,:] = sum_z slab[z,row,:] + b_dec (the dec_att GEMM's split-K partials are summed here).
// Grid (rows, parts): a workgroup builds dec_ctx[row] in LDS once and its 4 waves walk the regions of its part;
// each region row of enc_ctx (A floats) is read once with 16-byte loads and reduced by wave shuffles.
struct AttScoreArgs {
    const float* enc_ctx;        // [n_img, R, A] hoisted enc_att(feats) + bias
    const int32_t* img_of_row;   // null = identity
    const float* dec_slab; int nsplit;
    const float* b_dec;          // [A]
    const float* w_aff;          // [A] weight-normed
    const float* b_aff;          // [1]
    float* dec_ctx_out;          // [rows, A] or null (kept for backward)
    float* scores;               // [rows, R]
    int rows, R, A;
    const int* live;             // step_dead(live): return at entry
    const int32_t* counts;       // <true> instances only: valid leading regions per image (null = all R); R stays the row stride
};
// Adaptive region sets (icz_butd_set_regions).  The attention kernels below are templates on AD: <false> is the fixed-set kernel of
// R <= 64 regions ("lane r holds score r"); <true> serves per-image counts and sets of up to 128 regions.  A <true> kernel reads its
// image's count c with one scalar load and uses it as the bound of every region loop -- pad rows of feats / enc_ctx are never
// loaded -- while R remains the row stride of every tensor and of the mask / Philox index; what it writes at r >= c (scores, alpha,
// ds, d enc_ctx) is zero.  Softmax, dot and ds hold two regions per lane (lane, lane + 64): at c <= 64 the second is the
// identity of every reduction, so an image gets bit for bit what <false> gives it alone at R = c.
constexpr int ATT_MAX_R = 128;
// dec_ctx[row, :] built into LDS (sdec, A floats) by the whole workgroup: slab 0, then slabs 1 .. nsplit - 1 in order (MN = rows * A
// floats apart), then b_dec; `keep`: the row also goes to dec_ctx_out (where the caller keeps one).  The three score kernels
// build their rows here.
__device__ __forceinline__ void att_build_dec_ctx(const AttScoreArgs& a, size_t MN, int row, float* sdec, bool keep) {
    for (int c = threadIdx.x * 4; c < a.A; c += 1024) {
        const size_t off = (size_t)row * a.A + c;
        f32x4 s = *reinterpret_cast<const f32x4*>(a.dec_slab + off);
        for (int z = 1; z < a.nsplit; ++z) s += *reinterpret_cast<const f32x4*>(a.dec_slab + (size_t)z * MN + off);
        s += *reinterpret_cast<const f32x4*>(a.b_dec + c);
        *reinterpret_cast<f32x4*>(sdec + c) = s;
        if (a.dec_ctx_out && keep) *reinterpret_cast<f32x4*>(a.dec_ctx_out + off) = s;
    }
}
// Grid (rows, parts), 256 threads.  Part p owns regions p, p + parts, p + 2 parts, ...; a wave takes up to three of them
// at a time and issues all their loads (3 regions x 4 float4 per lane) before the first use: the kernel moves
// R*A*4 bytes per row once and is bound by how many bytes each CU keeps in flight, not by arithmetic.
template <bool AD>
__global__ __launch_bounds__(256) void att_scores_kernel(AttScoreArgs a, DropCfg dc) {
    extern __shared__ __attribute__((aligned(16))) float sdec[];   // A floats
    const int lflag = live_flag(a.live);
    const int row = blockIdx.x, part = blockIdx.y, nparts = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t MN = (size_t)a.rows * a.A;
    const int img = a.img_of_row ? a.img_of_row[row] : row;
    const int Rc = (AD && a.counts) ? a.counts[img] : a.R;
    constexpr int NB = 3;
    // the projected features do not depend on dec_ctx: the loads of the wave's first group of regions (its only one at 36
    // regions, A <= 1024) are issued before the split-K slabs are summed, so both round trips overlap
    f32x4 xf[NB][4];
    if (part + nparts * wave < Rc) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int r = part + nparts * (wave + 4 * b);
            const float* e = a.enc_ctx + ((size_t)img * a.R + (r < Rc ? r : part + nparts * wave)) * a.A;
#pragma unroll
            for (int u = 0; u < 4; ++u) xf[b][u] = *reinterpret_cast<const f32x4*>(e + min(lane * 4 + 256 * u, a.A - 4));
        }
    }
    if (flag_dead(lflag)) return;                 // behind the first loads, in front of the first write (icz_common.h)
    att_build_dec_ctx(a, MN, row, sdec, part == 0);
    __syncthreads();
    const float baff = a.b_aff[0];
    const int drow = row - dc.row0;                    // (DropCfg::row0: evaluation-mode rows of a merged chain in front)
    if (drow < 0) dc.mode = 0;
    const float sc = dc.mode ? 2.0f : 1.0f;
    const bool shared_bits = dc.mode == 2 && (a.A & 255) == 0;       // whole 256-column strips: every lane runs every c0 iteration
    for (int i0 = wave; part + nparts * i0 < Rc; i0 += 4 * NB) {
        int rr[NB];
        bool ok[NB];
        const float* e[NB];
        float acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int r = part + nparts * (i0 + 4 * b);
            ok[b] = r < Rc;
            rr[b] = ok[b] ? r : part + nparts * i0;
            e[b] = a.enc_ctx + ((size_t)img * a.R + rr[b]) * a.A;
            acc[b] = 0.f;
        }
        for (int c0 = lane * 4; c0 < a.A; c0 += 1024) {
            f32x4 x[NB][4];
            if (i0 == wave && c0 == lane * 4) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int u = 0; u < 4; ++u) x[b][u] = xf[b][u];
            } else {
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int u = 0; u < 4; ++u) x[b][u] = *reinterpret_cast<const f32x4*>(e[b] + min(c0 + 256 * u, a.A - 4));
            }
            // Philox keep-bits: a call covers 128 consecutive columns = one half-wave of one u; the 8 blocks of each of the NB
            // regions are computed once (lane 8 b + block) and handed round by shuffles instead of 64 lanes calling it 4 NB times
            uint32_t kq[NB][4];
            if (shared_bits) {
                const int pb = lane >> 3, pg = lane & 7;
                const int pr = pb == 0 ? rr[0] : (pb == 1 ? rr[1] : rr[NB - 1]);
                const uint64_t g = (((uint64_t)drow * a.R + pr) * a.A + (c0 - lane * 4) + 128 * pg) >> 7;
                const uint64_t seed = *dc.seed_p;
                uint4_ ctr = {(uint32_t)g, (uint32_t)(g >> 32), dc.step, dc.stream};
                const uint4_ pw = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int src = 8 * b + 2 * u + (lane >> 5);
                        const uint32_t w0 = __shfl(pw.x, src), w1 = __shfl(pw.y, src), w2 = __shfl(pw.z, src), w3 = __shfl(pw.w, src);
                        const int wi = (lane >> 3) & 3;
                        const uint32_t ww = wi == 0 ? w0 : (wi == 1 ? w1 : (wi == 2 ? w2 : w3));
                        kq[b][u] = (ww >> ((4 * lane) & 31)) & 0xFu;
                    }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + 256 * u;
                if (c < a.A) {
                    const f32x4 d = *reinterpret_cast<const f32x4*>(sdec + c);
                    const f32x4 w = *reinterpret_cast<const f32x4*>(a.w_aff + c);
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const uint32_t k = shared_bits ? kq[b][u] : (dc.mode ? dc.keep4(((uint64_t)drow * a.R + rr[b]) * a.A + c) : 0xFu);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float zv = fmaxf(x[b][u][j] + d[j], 0.f);
                            zv = ((k >> j) & 1u) ? zv * sc : 0.f;
                            acc[b] += zv * w[j];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float v = wave_sum(acc[b]);
            if (lane == 0 && ok[b]) a.scores[(size_t)row * a.R + rr[b]] = v + baff;
        }
    }
    if constexpr (AD) {
        if (part == 0)
            for (int r = Rc + tid; r < a.R; r += 256) a.scores[(size_t)row * a.R + r] = 0.f;
    }
}

constexpr int ATT_CTX_MAX_G = 8;
// The same with the G rows of an image next to each other (row = img * G + g) sharing its projected features: one workgroup per
// (image, part) builds the G dec_ctx rows in LDS and walks its regions once, so every region row of enc_ctx (A floats) is fetched
// once instead of G times.  Same arithmetic and summation order per row as att_scores_kernel.  Grid (n_img, parts).  One body, two
// kernels below: TRAIN adds the early-out flag and the attention dropout per row (the row's own keep-bits, indexed as
// att_scores_kernel indexes them); without it `dc` is not read.
template <bool AD, bool TRAIN>
__device__ __forceinline__ void att_scores_group_body(const AttScoreArgs& a, const DropCfg& dc, int G, float* sdec) {
    int lflag = 1;
    if constexpr (TRAIN) lflag = live_flag(a.live);
    const int img = blockIdx.x, part = blockIdx.y, nparts = gridDim.y;
    const int Rc = (AD && a.counts) ? a.counts[img] : a.R;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t MN = (size_t)a.rows * a.A;
    if constexpr (TRAIN) {
        if (flag_dead(lflag)) return;
    }
    for (int g = 0; g < G; ++g) att_build_dec_ctx(a, MN, img * G + g, sdec + (size_t)g * a.A, part == 0);
    __syncthreads();
    const float baff = a.b_aff[0];
    const float sc = (TRAIN && dc.mode) ? 2.0f : 1.0f;
    for (int i0 = wave; part + nparts * i0 < Rc; i0 += 4) {
        const int r = part + nparts * i0;
        const float* e = a.enc_ctx + ((size_t)img * a.R + r) * a.A;
        float acc[ATT_CTX_MAX_G];
#pragma unroll
        for (int g = 0; g < ATT_CTX_MAX_G; ++g) acc[g] = 0.f;
        for (int c0 = lane * 4; c0 < a.A; c0 += 1024) {
            f32x4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const f32x4*>(e + min(c0 + 256 * u, a.A - 4));
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + 256 * u;
                if (c < a.A) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(a.w_aff + c);
#pragma unroll
                    for (int g = 0; g < ATT_CTX_MAX_G; ++g)
                        if (g < G) {
                            const f32x4 d = *reinterpret_cast<const f32x4*>(sdec + (size_t)g * a.A + c);
                            if constexpr (TRAIN) {
                                const uint64_t drow = (uint64_t)(img * G + g - dc.row0);
                                const uint32_t k = dc.mode ? dc.keep4((drow * a.R + r) * a.A + c) : 0xFu;
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    float zv = fmaxf(x[u][j] + d[j], 0.f);
                                    zv = ((k >> j) & 1u) ? zv * sc : 0.f;
                                    acc[g] += zv * w[j];
                                }
                            } else {
#pragma unroll
                                for (int j = 0; j < 4; ++j) acc[g] += fmaxf(x[u][j] + d[j], 0.f) * w[j];
                            }
                        }
                }
            }
        }
#pragma unroll
        for (int g = 0; g < ATT_CTX_MAX_G; ++g)
            if (g < G) {
                const float v = wave_sum(acc[g]);
                if (lane == 0) a.scores[(size_t)(img * G + g) * a.R + r] = v + baff;
            }
    }
    if constexpr (AD) {
        if (part == 0)
            for (int i = tid; i < G * (a.R - Rc); i += 256) a.scores[(size_t)(img * G + i / (a.R - Rc)) * a.R + Rc + i % (a.R - Rc)] = 0.f;
    }
}
// Beam search (the G = beam rows of an image; at 640 rows the per-row kernel re-reads 47 MB of enc_ctx per step through the caches):
// evaluation mode only, beam search has no dropout.
template <bool AD>
__global__ __launch_bounds__(256) void att_scores_group_kernel(AttScoreArgs a, int G) {
    extern __shared__ __attribute__((aligned(16))) float sdec[];   // [G][A]
    att_scores_group_body<AD, false>(a, DropCfg{}, G, sdec);
}
// The multi-sample SCST rollout (Butd::sample_n: the G = K sampled rows of an image): training mode, with the same DropCfg the rows'
// scores are those of att_scores_kernel.
template <bool AD>
__global__ __launch_bounds__(256) void att_scores_group_train_kernel(AttScoreArgs a, DropCfg dc, int G) {
    extern __shared__ __attribute__((aligned(16))) float sdec[];   // [G][A]
    att_scores_group_body<AD, true>(a, dc, G, sdec);
}

// ---------------------------------------------------------------------------------------------------------
// softmax over regions + attention-weighted feature sum (:60-61):
//   alpha = softmax_r(score[row,:]);  ctx[row, d] = sum_r alpha[r] * feats[img, r, d]
// Grid (rows, D/512), 256 threads: thread (half, cg) sums one half of the regions for 4 consecutive d (16-byte loads,
// 9 in flight per thread); the two halves meet in LDS.  Every wave recomputes the R <= 64 softmax (lane r holds score r).
// <true> (see AttScoreArgs): the halves are cut at (c + 1) / 2 of the image's count c, so the row sums as it would at R = c.
template <bool AD>
__global__ __launch_bounds__(256) void att_ctx_kernel(const float* __restrict__ feats, const int32_t* __restrict__ img_of_row,
                                                      const float* __restrict__ scores, float* __restrict__ alpha_out,
                                                      float* __restrict__ alpha_out2, int alpha2_stride,
                                                      float* __restrict__ ctx, int R, int D, const int* __restrict__ live,
                                                      const int32_t* __restrict__ counts) {
    __shared__ float sal[AD ? ATT_MAX_R : 64];
    __shared__ __attribute__((aligned(16))) float spart[128 * 4];
    const int lflag = live_flag(live);
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int cg = tid & 127, half = tid >> 7;
    const int d = blockIdx.y * 512 + cg * 4;
    const bool valid = d < D;
    const int img = img_of_row ? img_of_row[row] : row;
    const int Rc = (AD && counts) ? counts[img] : R;
    const int Rh = (Rc + 1) / 2;
    const int r_lo = half ? Rh : 0, r_hi = half ? Rc : Rh;
    const float* f = feats + (size_t)img * R * D + (valid ? d : 0);
    // the feature loads do not depend on the weights: the first two rounds (all of them at 36 regions) are issued before the
    // scores are read, so the softmax runs while they are in flight instead of in front of them
    constexpr int RB = 9;
    f32x4 x0[RB], x1[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) x0[u] = *reinterpret_cast<const f32x4*>(f + (size_t)min(r_lo + u, r_hi - 1) * D);
#pragma unroll
    for (int u = 0; u < RB; ++u) x1[u] = *reinterpret_cast<const f32x4*>(f + (size_t)min(r_lo + RB + u, r_hi - 1) * D);
    if (flag_dead(lflag)) return;                 // behind the first loads, in front of the first write (icz_common.h)
    if constexpr (AD) {          // two regions per lane; the weights of r >= c are exact zeros, and are written as such
        const float scv = lane < Rc ? scores[(size_t)row * R + lane] : -INFINITY;
        const float scw = lane + 64 < Rc ? scores[(size_t)row * R + lane + 64] : -INFINITY;
        float al[2];
        wave_softmax2(scv, lane < Rc, scw, lane + 64 < Rc, al[0], al[1]);
        if (tid < 64) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int r = tid + 64 * q;
                sal[r] = al[q];
                if (blockIdx.y == 0 && r < R) {
                    alpha_out[(size_t)row * R + r] = al[q];
                    if (alpha_out2) alpha_out2[(size_t)row * alpha2_stride + r] = al[q];
                }
            }
        }
    } else {
        const float scv = lane < R ? scores[(size_t)row * R + lane] : -INFINITY;
        const float al = wave_softmax(scv, lane < R);
        if (tid < 64) {
            sal[tid] = al;
            if (blockIdx.y == 0 && tid < R) {
                alpha_out[(size_t)row * R + tid] = al;
                if (alpha_out2) alpha_out2[(size_t)row * alpha2_stride + tid] = al;
            }
        }
    }
    __syncthreads();
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
#pragma unroll
        for (int u = 0; u < RB; ++u)
            if (r_lo + u < r_hi) acc += x0[u] * sal[r_lo + u];
#pragma unroll
        for (int u = 0; u < RB; ++u)
            if (r_lo + RB + u < r_hi) acc += x1[u] * sal[r_lo + RB + u];
        for (int r0 = r_lo + 2 * RB; r0 < r_hi; r0 += RB) {
            f32x4 x[RB];
#pragma unroll
            for (int u = 0; u < RB; ++u) x[u] = *reinterpret_cast<const f32x4*>(f + (size_t)min(r0 + u, r_hi - 1) * D);
#pragma unroll
            for (int u = 0; u < RB; ++u)
                if (r0 + u < r_hi) acc += x[u] * sal[r0 + u];
        }
    }
    if (half) *reinterpret_cast<f32x4*>(spart + cg * 4) = acc;
    __syncthreads();
    if (!half && valid) *reinterpret_cast<f32x4*>(ctx + (size_t)row * D + d) = acc + *reinterpret_cast<const f32x4*>(spart + cg * 4);
}

// The same for beam search, where the G = beam rows of an image sit next to each other (row = img * G + b) and share its
// features: one workgroup does the G rows of one image for its 512 columns, so every feature vector is fetched once
// instead of G times (at 640 rows the per-row kernel moves 189 MB through the caches per step).  Same arithmetic and
// summation order per row as att_ctx_kernel.  Grid (n_img, D/512).  `live`: the multi-sample rollout's early-out (null for beam search).
template <bool AD>
__global__ __launch_bounds__(256) void att_ctx_group_kernel(const float* __restrict__ feats, const float* __restrict__ scores,
                                                            float* __restrict__ alpha_out, float* __restrict__ ctx, int R, int D, int G,
                                                            const int* __restrict__ live, const int32_t* __restrict__ counts) {
    __shared__ float sal[ATT_CTX_MAX_G][AD ? ATT_MAX_R : 64];
    __shared__ __attribute__((aligned(16))) float spart[ATT_CTX_MAX_G][128 * 4];
    if (step_dead(live)) return;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Rc = (AD && counts) ? counts[img] : R;
    for (int g = wave; g < G; g += 4) {                 // wave w: softmax of rows w, w + 4
        const int row = img * G + g;
        if constexpr (AD) {      // two regions per lane, as in att_ctx_kernel<true>
            const float scv = lane < Rc ? scores[(size_t)row * R + lane] : -INFINITY;
            const float scw = lane + 64 < Rc ? scores[(size_t)row * R + lane + 64] : -INFINITY;
            float al[2];
            wave_softmax2(scv, lane < Rc, scw, lane + 64 < Rc, al[0], al[1]);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int r = lane + 64 * q;
                sal[g][r] = al[q];
                if (blockIdx.y == 0 && r < R) alpha_out[(size_t)row * R + r] = al[q];
            }
        } else {
            const float scv = lane < R ? scores[(size_t)row * R + lane] : -INFINITY;
            const float al = wave_softmax(scv, lane < R);
            sal[g][lane] = al;
            if (blockIdx.y == 0 && lane < R) alpha_out[(size_t)row * R + lane] = al;
        }
    }
    __syncthreads();
    const int cg = tid & 127, half = tid >> 7;
    const int d = blockIdx.y * 512 + cg * 4;
    const bool valid = d < D;
    const int Rh = (Rc + 1) / 2;
    const int r_lo = half ? Rh : 0, r_hi = half ? Rc : Rh;
    const float* f = feats + (size_t)img * R * D + (valid ? d : 0);
    f32x4 acc[ATT_CTX_MAX_G];
#pragma unroll
    for (int g = 0; g < ATT_CTX_MAX_G; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (valid) {
        constexpr int RB = 9;
        for (int r0 = r_lo; r0 < r_hi; r0 += RB) {
            f32x4 x[RB];
#pragma unroll
            for (int u = 0; u < RB; ++u) x[u] = *reinterpret_cast<const f32x4*>(f + (size_t)min(r0 + u, r_hi - 1) * D);
#pragma unroll
            for (int g = 0; g < ATT_CTX_MAX_G; ++g)
                if (g < G) {
#pragma unroll
                    for (int u = 0; u < RB; ++u)
                        if (r0 + u < r_hi) acc[g] += x[u] * sal[g][r0 + u];
                }
        }
    }
    if (half) {
#pragma unroll
        for (int g = 0; g < ATT_CTX_MAX_G; ++g)
            if (g < G) *reinterpret_cast<f32x4*>(spart[g] + cg * 4) = acc[g];
    }
    __syncthreads();
    if (!half && valid) {
#pragma unroll
        for (int g = 0; g < ATT_CTX_MAX_G; ++g)
            if (g < G) *reinterpret_cast<f32x4*>(ctx + (size_t)(img * G + g) * D + d) = acc[g] + *reinterpret_cast<const f32x4*>(spart[g] + cg * 4);
    }
}

// attention maps of a stored forward pass, [T, B, NH, R] -> [B, T, R] averaged over the NH heads (BUTD: NH = 1)
__global__ void saved_alphas_kernel(const float* __restrict__ src, int T, int B, int NH, int R, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * T * R) return;
    const int r = i % R, t = (i / R) % T, b = i / (R * T);
    const float* p = src + ((size_t)(t * B + b) * NH) * R + r;
    float s = 0.f;
    for (int h = 0; h < NH; ++h) s += p[(size_t)h * R];
    out[i] = s / (float)NH;
}
inline void launch_saved_alphas(const float* src, int T, int B, int NH, int R, float* out, hipStream_t st) {
    hipLaunchKernelGGL(saved_alphas_kernel, dim3(cdiv(B * T * R, 256)), dim3(256), 0, st, src, T, B, NH, R, out);
}

// ---------------------------------------------------------------------------------------------------------
// SoftAttention backward in three full-chip kernels (each moves its bytes once, with many loads in flight per lane):
//   per step   att_bwd_dalpha_kernel   dalpha[row,r] = dctx[row,:] . feats[row,r,:]
//   per step   att_bwd_ddec_kernel     ds = softmax'(alpha, dalpha);  ddec[row,a] = sum_r on(row,r,a) ds_r w_aff[a] scale
//   once       att_bwd_denc_kernel     denc[row,r,a] = sum_t on_t ds_t w_aff scale;  dwaff partials   (after the time loop)
// with zpre = enc_ctx[row,r,a] + dec_ctx_t[row,a] and on = zpre > 0 && keep-bit (relu + dropout).  enc_ctx is shared by all
// time steps, so its gradient is a sum over t: accumulating it step by step would read-modify-write R*A floats per row
// and step; instead the steps only record ds_t (R floats per row) and the sum over t is formed once, in registers.

// dctx = sum of slabs [ns][rows][ldc] columns 0..D (the LM-LSTM dgrad GEMM output).  Grid (rows, parts = ceil(D / 512)), 256 threads:
// a workgroup sums the slabs of ITS 512 columns only (with 16 slabs per step the slab sum is as many bytes as the features: every
// part summing the whole row, as before round 3, quadrupled it) and emits partial dot products dalpha_part[row][part][r] over
// those columns for all regions; att_bwd_ddec_kernel adds the parts in order.  Wave w takes regions w, w + 4, ...: two 16-byte
// feature loads per lane and region, all of a wave's loads independent.
constexpr int DALPHA_COLS = 512;
// <true> (see AttScoreArgs): the passes stop at the image's count; dalpha_part at r >= c is neither written nor read.
template <bool AD>
__global__ __launch_bounds__(256) void att_bwd_dalpha_kernel(const float* __restrict__ dctx, int ns, int ldc, int rows,
                                                             const float* __restrict__ feats, int R, int D,
                                                             float* __restrict__ dalpha_part, const int* __restrict__ live,
                                                             const int32_t* __restrict__ img_of_row,       // null = identity
                                                             const int32_t* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float sd[DALPHA_COLS];
    const int lflag = live_flag(live);
    const int row = blockIdx.x, part = blockIdx.y, nparts = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = part * DALPHA_COLS;
    const size_t ss = (size_t)rows * ldc;
    constexpr int NR = 5;                         // regions per wave and pass (R <= 64: at most 16 per wave)
    const int ca = c0 + 4 * lane, cb = ca + 256;
    const bool va = ca < D, vb = cb < D;
    const int img = img_of_row ? img_of_row[row] : row;
    const int Rc = (AD && counts) ? counts[img] : R;
    const float* frow = feats + (size_t)img * R * D;
    f32x4 xa[NR], xb[NR];
    auto load_pass = [&](int r0) {                // clamped: a pass past the last region re-reads it and is not stored
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int r = min(r0 + 4 * u, Rc - 1);
            xa[u] = *reinterpret_cast<const f32x4*>(frow + (size_t)r * D + (va ? ca : 0));
            xb[u] = *reinterpret_cast<const f32x4*>(frow + (size_t)r * D + (vb ? cb : 0));
        }
    };
    load_pass(wave);                              // in flight behind the slab sum
    if (flag_dead(lflag)) return;                 // behind the first loads, in front of the first write (icz_common.h)
    if (tid < DALPHA_COLS / 4) {
        const int c = c0 + 4 * tid;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c < D) v = sum_slabs4(dctx, ns, ss, (size_t)row * ldc + c);
        *reinterpret_cast<f32x4*>(sd + 4 * tid) = v;
    }
    __syncthreads();
    const f32x4 ga = *reinterpret_cast<const f32x4*>(sd + 4 * lane), gb = *reinterpret_cast<const f32x4*>(sd + 256 + 4 * lane);
    for (int r0 = wave; r0 < Rc; r0 += 4 * NR) {
        if (r0 != wave) load_pass(r0);
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            float acc = 0.f;
            if (va) acc += xa[u][0] * ga[0] + xa[u][1] * ga[1] + xa[u][2] * ga[2] + xa[u][3] * ga[3];
            if (vb) acc += xb[u][0] * gb[0] + xb[u][1] * gb[1] + xb[u][2] * gb[2] + xb[u][3] * gb[3];
            acc = wave_sum(acc);
            const int r = r0 + 4 * u;
            if (lane == 0 && r < Rc) dalpha_part[((size_t)row * nparts + part) * R + r] = acc;
        }
    }
}

// Grid (rows, A/256), 256 threads: thread (wq = wave, cg) sums regions wq, wq+4, ... for 4 consecutive attention columns;
// the four waves meet in LDS.  ds_out (block y = 0) keeps ds for att_bwd_denc_kernel.
struct AttBwdDdecArgs {
    const float* enc_ctx; const float* dec_ctx; const float* w_aff; const float* alpha; const float* dalpha;   // dalpha: [rows][nparts][R] partials
    float* ddec; float* ds_out;
    int R, A, nparts;
    const int* live;              // step_dead(live): ddec and ds rows of this step are ZERO (read by the GEMMs / kernels over all steps)
    const int32_t* img_of_row;    // image of each row (enc_ctx row); null = identity
    const int32_t* counts;        // <true> only: valid leading regions per image (null = all R)
};
// <true> (see AttScoreArgs): alpha, dalpha and ds of regions lane and lane + 64; ds at r >= c is written as zero.
template <bool AD>
__global__ __launch_bounds__(256) void att_bwd_ddec_kernel(AttBwdDdecArgs a, DropCfg dc) {
    __shared__ float sds[AD ? ATT_MAX_R : 64];
    __shared__ __attribute__((aligned(16))) float spart[3 * 64 * 4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wq = tid >> 6;
    const int lflag = live_flag(a.live);
    const int img = a.img_of_row ? a.img_of_row[row] : row;
    const int Rc = (AD && a.counts) ? a.counts[img] : a.R;
    const float al = lane < Rc ? a.alpha[(size_t)row * a.R + lane] : 0.f;
    const float da0 = lane < Rc ? a.dalpha[(size_t)row * a.nparts * a.R + lane] : 0.f;
    float al2 = 0.f, da2 = 0.f;                   // <true>: region lane + 64
    if constexpr (AD) {
        if (lane + 64 < Rc) {
            al2 = a.alpha[(size_t)row * a.R + lane + 64];
            da2 = a.dalpha[(size_t)row * a.nparts * a.R + lane + 64];
        }
    }
    if (flag_dead(lflag)) {                       // behind the first loads (icz_common.h); a dead step's d dec / ds rows are zeros
        if (blockIdx.y == 0 && tid < a.R) a.ds_out[(size_t)row * a.R + tid] = 0.f;
        const int c = blockIdx.y * 256 + tid;
        if (c < a.A) a.ddec[(size_t)row * a.A + c] = 0.f;
        return;
    }
    float da = da0;
    if (lane < Rc)
        for (int p = 1; p < a.nparts; ++p) da += a.dalpha[((size_t)row * a.nparts + p) * a.R + lane];
    if constexpr (AD) {
        if (lane + 64 < Rc)
            for (int p = 1; p < a.nparts; ++p) da2 += a.dalpha[((size_t)row * a.nparts + p) * a.R + lane + 64];
        // Up to 64 regions the sum must come out as the fixed-set instance's wave_sum(al * da) does, bit for bit.  There the compiler
        // fuses the product into the reduction's first add (v_fmac on the shuffled rounded product); spelled out here, because next to
        // the two-region form it would share one rounded product between the branches and add it unfused (one ulp apart; seen in the
        // saved assembly and on the device).  tests/test_gpu_butd_adaptive.py holds the two instances together.  Rc is uniform.
        float dot;
        if (Rc <= 64) {
            dot = __builtin_fmaf(al, da, __shfl_xor(al * da, 32, 64));
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
        } else {
            dot = wave_sum(al * da + al2 * da2);
        }
        const float ds_l[2] = {al * (da - dot), al2 * (da2 - dot)};
        if (tid < 64) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int r = tid + 64 * q;
                sds[r] = ds_l[q];
                if (blockIdx.y == 0 && r < a.R) a.ds_out[(size_t)row * a.R + r] = r < Rc ? ds_l[q] : 0.f;
            }
        }
    } else {
        const float dot = wave_sum(al * da);
        const float ds_l = al * (da - dot);
        if (tid < 64) {
            sds[tid] = ds_l;
            if (blockIdx.y == 0 && tid < a.R) a.ds_out[(size_t)row * a.R + tid] = ds_l;
        }
    }
    __syncthreads();
    const int c = blockIdx.y * 256 + lane * 4;
    const bool valid = c < a.A;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(a.dec_ctx + (size_t)row * a.A + c);
        const f32x4 w = *reinterpret_cast<const f32x4*>(a.w_aff + c);
        const float sc = dc.mode ? 2.0f : 1.0f;
        constexpr int RB = 9;
        const bool shared_bits = dc.mode == 2 && (a.A & 255) == 0;      // every lane of the wave is valid and takes every iteration
        for (int r0 = wq; r0 < Rc; r0 += 4 * RB) {
            f32x4 x[RB];
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int r = min(r0 + 4 * u, Rc - 1);
                x[u] = *reinterpret_cast<const f32x4*>(a.enc_ctx + ((size_t)img * a.R + r) * a.A + c);
            }
            // Philox keep-bits, shared as in att_scores_kernel: lane 2 u + half computes the block of region u's half-strip
            uint32_t kq[RB];
            if (shared_bits) {
                const int pu = min(lane >> 1, RB - 1), ph = lane & 1;
                const int pr = min(r0 + 4 * pu, Rc - 1);
                const uint64_t g = (((uint64_t)row * a.R + pr) * a.A + blockIdx.y * 256 + 128 * ph) >> 7;
                const uint64_t seed = *dc.seed_p;
                uint4_ ctr = {(uint32_t)g, (uint32_t)(g >> 32), dc.step, dc.stream};
                const uint4_ pw = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
                for (int u = 0; u < RB; ++u) {
                    const int src = 2 * u + (lane >> 5);
                    const uint32_t w0 = __shfl(pw.x, src), w1 = __shfl(pw.y, src), w2 = __shfl(pw.z, src), w3 = __shfl(pw.w, src);
                    const int wi = (lane >> 3) & 3;
                    const uint32_t ww = wi == 0 ? w0 : (wi == 1 ? w1 : (wi == 2 ? w2 : w3));
                    kq[u] = (ww >> ((4 * lane) & 31)) & 0xFu;
                }
            }
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int r = r0 + 4 * u;
                if (r < Rc) {
                    const float ds = sds[r];
                    const uint32_t k = shared_bits ? kq[u] : (dc.mode ? dc.keep4(((uint64_t)row * a.R + r) * a.A + c) : 0xFu);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool on = (x[u][j] + d[j] > 0.f) && ((k >> j) & 1u);
                        acc[j] += on ? ds * w[j] * sc : 0.f;
                    }
                }
            }
        }
    }
    if (wq > 0) *reinterpret_cast<f32x4*>(spart + ((wq - 1) * 64 + lane) * 4) = acc;
    __syncthreads();
    if (wq == 0 && valid) {
#pragma unroll
        for (int w = 0; w < 3; ++w) acc += *reinterpret_cast<const f32x4*>(spart + (w * 64 + lane) * 4);
        *reinterpret_cast<f32x4*>(a.ddec + (size_t)row * a.A + c) = acc;
    }
}

// Grid (B, parts), 256 threads.  Part p owns regions p, p + parts, ...; a thread owns 4 consecutive attention columns,
// keeps dec_ctx_t of up to TT time steps in registers and walks its regions: one read of enc_ctx, one write of denc.
//   denc[row,r,a]          = sum_t on_t ds_t[row,r] w_aff[a] scale
//   dwaff_part[row,p,a]    = sum_{r in p} sum_t on_t ds_t[row,r] zpre scale        (column-summed over rows x parts afterwards)
struct AttBwdDencArgs {
    const float* enc_ctx; const float* dec_all; const float* ds_all; const float* w_aff;
    float* denc; float* dwaff_part;
    int B, R, A, T;
    int mode; const uint8_t* mask; size_t mask_step; const uint64_t* seed_p; uint32_t stream;
    int Bs;          // rows per time step in dec_all / ds_all (0 = B; a merged chain stores 2 B, the pointers then start at its second half)
    const int32_t* img_of_row;   // image of each row (enc_ctx row); null = identity.  denc, the masks and the Philox index stay per row
    const int32_t* counts;       // <.., true> only: valid leading regions per image (null = all R)
};
// What att_bwd_denc_kernel and att_bwd_denc_group_kernel share of a region's work: where the keep-bits come from.  (The on / de / dw
// update behind them is written out in both: as a helper it changed the register allocation of both kernels, which sit at the
// register limit, and moved the grouped one into scratch.)
// Philox keep-bits: one call covers 128 consecutive elements = the 32 lanes of a half-wave (4 columns each), so instead
// of every lane calling it for every time step, lane j of a half-wave calls it for step t0 + j and the words are handed
// round through LDS: TT calls per half-wave and region instead of 32 * TT.  Called by the whole workgroup (the first barrier: the
// previous region's words have been read); eoff = the thread's element of the row's mask / Philox index, cv = its columns exist.
template <int TT>
__device__ __forceinline__ void denc_share_bits(const AttBwdDencArgs& a, uint32_t (&sbits)[4][2][TT][4], size_t eoff, int t0, bool cv) {
    static_assert(TT <= 32, "one half-wave computes the TT Philox words of its 128-column group");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, hl = lane & 31;
    __syncthreads();
    if (cv && hl < TT && t0 + hl < a.T) {
        const uint64_t g = (eoff - (size_t)(4 * hl)) >> 7;          // the half-wave's group: its first lane's element
        const uint64_t seed = *a.seed_p;
        uint4_ ctr = {(uint32_t)g, (uint32_t)(g >> 32), (uint32_t)(t0 + hl), a.stream};
        const uint4_ rr = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
        uint32_t* o = sbits[wave][half][hl];
        o[0] = rr.x; o[1] = rr.y; o[2] = rr.z; o[3] = rr.w;
    }
    __syncthreads();
}
// keep nibble of the thread's 4 columns at step t = t0 + j: explicit mask, the words denc_share_bits left in LDS, or Philox
template <int TT>
__device__ __forceinline__ uint32_t denc_keep4(const AttBwdDencArgs& a, const uint32_t (&sbits)[4][2][TT][4], bool shared_bits, int t, int j, size_t eoff) {
    uint32_t k = 0xFu;
    if (a.mode == 1) {
        k = mask_keep4(a.mask + (size_t)t * a.mask_step + eoff);
    } else if (shared_bits) {
        k = (sbits[threadIdx.x >> 6][(threadIdx.x >> 5) & 1][j][(eoff >> 5) & 3] >> (eoff & 31)) & 0xFu;      // [wave][half-wave]
    } else if (a.mode == 2) {
        k = (rng_group_bits(*a.seed_p, a.stream, (uint32_t)t, eoff) >> (eoff & 31)) & 0xFu;
    }
    return k;
}
// <TT, true> (see AttScoreArgs): the region walk stops at the image's count; d enc_ctx rows at r >= c are written as zeros (the
// enc_att weight-gradient GEMM and the bias sum run over all B R rows).
template <int TT, bool AD = false>
__global__ __launch_bounds__(256) void att_bwd_denc_kernel(AttBwdDencArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sds_t[];     // [T][R] ds of this row
    __shared__ uint32_t sbits[4][2][TT][4];                           // (denc_share_bits)
    const int row = blockIdx.x, part = blockIdx.y, nparts = gridDim.y, tid = threadIdx.x;
    const int Bst = a.Bs > 0 ? a.Bs : a.B;
    const int img = a.img_of_row ? a.img_of_row[row] : row;
    const int Rc = (AD && a.counts) ? a.counts[img] : a.R;
    for (int i = tid; i < a.T * a.R; i += 256) {
        const int t = i / a.R, r = i % a.R;
        sds_t[i] = a.ds_all[((size_t)t * Bst + row) * a.R + r];
    }
    __syncthreads();
    const float sc = a.mode ? 2.0f : 1.0f;
    const bool shared_bits = a.mode == 2 && (a.A & 127) == 0;
    for (int c0 = 0; c0 < a.A; c0 += 1024) {          // uniform over the workgroup (barriers inside)
        const int c = c0 + tid * 4;
        const bool cv = c < a.A;
        const f32x4 w = cv ? *reinterpret_cast<const f32x4*>(a.w_aff + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 dw = {0.f, 0.f, 0.f, 0.f};
        for (int t0 = 0; t0 < a.T; t0 += TT) {
            f32x4 d[TT];
#pragma unroll
            for (int j = 0; j < TT; ++j) {
                const int t = min(t0 + j, a.T - 1);
                d[j] = cv ? *reinterpret_cast<const f32x4*>(a.dec_all + ((size_t)t * Bst + row) * a.A + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            for (int r = part; r < a.R; r += nparts) {
                const size_t eoff = ((size_t)row * a.R + r) * a.A + c;
                if (AD && r >= Rc) {            // pad rows (uniform over the workgroup): zeros, once
                    if (cv && t0 == 0) *reinterpret_cast<f32x4*>(a.denc + eoff) = (f32x4){0.f, 0.f, 0.f, 0.f};
                    continue;
                }
                if (shared_bits) denc_share_bits<TT>(a, sbits, eoff, t0, cv);
                if (!cv) continue;
                const f32x4 x = *reinterpret_cast<const f32x4*>(a.enc_ctx + ((size_t)img * a.R + r) * a.A + c);
                f32x4 de = {0.f, 0.f, 0.f, 0.f};
                if (t0 > 0) de = *reinterpret_cast<const f32x4*>(a.denc + eoff);
#pragma unroll
                for (int j = 0; j < TT; ++j) {
                    const int t = t0 + j;
                    if (t < a.T) {
                        const float ds = sds_t[t * a.R + r];
                        const uint32_t k = denc_keep4<TT>(a, sbits, shared_bits, t, j, eoff);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float zp = x[q] + d[j][q];
                            const bool on = (zp > 0.f) && ((k >> q) & 1u);
                            de[q] += on ? ds * w[q] * sc : 0.f;
                            dw[q] += on ? zp * sc * ds : 0.f;
                        }
                    }
                }
                *reinterpret_cast<f32x4*>(a.denc + eoff) = de;
            }
        }
        if (cv) *reinterpret_cast<f32x4*>(a.dwaff_part + ((size_t)row * nparts + part) * a.A + c) = dw;
    }
}

// Multi-sample SCST (Butd::sample_n): the G rows img * G + k of an image share its enc_ctx.  One workgroup per (image, part) does
// what att_bwd_denc_kernel does for each of the G rows, in k order: a thread reads its enc_ctx elements of the part's regions ONCE
// (registers, for all G rows), forms each row's d enc_ctx exactly as the per-row kernel forms it, and adds the G of them in k order
// into denc[img] (the per-row route, att_bwd_denc_kernel + rowgroup_sum_kernel, gets the same sums).  dwaff_part[img, part] = the
// rows' partials added in k order.  Grid (n_img, parts) with parts * DENC_GROUP_REGS >= R; a.B = rows, a.img_of_row unused.
constexpr int DENC_GROUP_REGS = 16;
// <TT, true> (see AttScoreArgs): regions at or behind the image's count are neither loaded nor walked; their d enc_ctx rows are zeros.
template <int TT, bool AD = false>
__global__ __launch_bounds__(256) void att_bwd_denc_group_kernel(AttBwdDencArgs a, int G) {
    extern __shared__ __attribute__((aligned(16))) float sds_t[];     // [T][R] ds of the current row
    __shared__ uint32_t sbits[4][2][TT][4];                           // (denc_share_bits)
    const int img = blockIdx.x, part = blockIdx.y, nparts = gridDim.y, tid = threadIdx.x;
    const int Bst = a.Bs > 0 ? a.Bs : a.B;
    const int Rc = (AD && a.counts) ? a.counts[img] : a.R;
    const float sc = a.mode ? 2.0f : 1.0f;
    const bool shared_bits = a.mode == 2 && (a.A & 127) == 0;
    for (int c0 = 0; c0 < a.A; c0 += 1024) {          // uniform over the workgroup (barriers inside)
        const int c = c0 + tid * 4;
        const bool cv = c < a.A;
        const f32x4 w = cv ? *reinterpret_cast<const f32x4*>(a.w_aff + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 x[DENC_GROUP_REGS];
#pragma unroll
        for (int i = 0; i < DENC_GROUP_REGS; ++i) {
            const int r = part + i * nparts;
            x[i] = (cv && r < Rc) ? *reinterpret_cast<const f32x4*>(a.enc_ctx + ((size_t)img * a.R + r) * a.A + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        f32x4 dwsum = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < G; ++k) {
            const int row = img * G + k;
            __syncthreads();                            // the previous row's ds have been read
            for (int i = tid; i < a.T * a.R; i += 256) {
                const int t = i / a.R, r = i % a.R;
                sds_t[i] = a.ds_all[((size_t)t * Bst + row) * a.R + r];
            }
            __syncthreads();
            f32x4 de[DENC_GROUP_REGS];
#pragma unroll
            for (int i = 0; i < DENC_GROUP_REGS; ++i) de[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            f32x4 dw = {0.f, 0.f, 0.f, 0.f};
            for (int t0 = 0; t0 < a.T; t0 += TT) {
                f32x4 d[TT];
#pragma unroll
                for (int j = 0; j < TT; ++j) {
                    const int t = min(t0 + j, a.T - 1);
                    d[j] = cv ? *reinterpret_cast<const f32x4*>(a.dec_all + ((size_t)t * Bst + row) * a.A + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int i = 0; i < DENC_GROUP_REGS; ++i) {
                    const int r = part + i * nparts;
                    if (r >= Rc) break;                 // uniform
                    const size_t eoff = ((size_t)row * a.R + r) * a.A + c;      // the row's element: mask / Philox index
                    if (shared_bits) denc_share_bits<TT>(a, sbits, eoff, t0, cv);
                    if (!cv) continue;
#pragma unroll
                for (int j = 0; j < TT; ++j) {
                    const int t = t0 + j;
                    if (t < a.T) {
                        const float ds = sds_t[t * a.R + r];
                        const uint32_t k = denc_keep4<TT>(a, sbits, shared_bits, t, j, eoff);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float zp = x[i][q] + d[j][q];
                            const bool on = (zp > 0.f) && ((k >> q) & 1u);
                            de[i][q] += on ? ds * w[q] * sc : 0.f;
                            dw[q] += on ? zp * sc * ds : 0.f;
                        }
                    }
                }
                }
            }
            if (cv) {
#pragma unroll
                for (int i = 0; i < DENC_GROUP_REGS; ++i) {
                    const int r = part + i * nparts;
                    if (r >= a.R) break;
                    f32x4* o = reinterpret_cast<f32x4*>(a.denc + ((size_t)img * a.R + r) * a.A + c);
                    *o = k == 0 ? de[i] : *o + de[i];
                }
                dwsum = k == 0 ? dw : dwsum + dw;
            }
        }
        if (cv) *reinterpret_cast<f32x4*>(a.dwaff_part + ((size_t)img * nparts + part) * a.A + c) = dwsum;
    }
}

}  // namespace
}  // namespace icz
