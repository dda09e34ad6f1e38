// The call pattern around gemm_f32 (gemm_f32.h), owned once: describe a product, pick its split-K factor, write it (dense, or as slabs
// that a consumer kernel sums, or as slabs summed here into a finished output), and the weight-gradient / bias-gradient forms of BPTT.
// Free functions without handle state: the decoder families (butd*.hip, aoa*.hip, nic.hip) and the GEMM entries of the C ABI
// (gemm_f32.hip) pass their own buffers, capacities and streams.  Nothing outside gemm_ops.hip launches slab_reduce_kernel or
// colsum_kernel.
#pragma once
#include <initializer_list>

#include "gemm_f32.h"

namespace icz {

// ---- describing a product: one to GEMM_MAX_SEG segments {A, B, lda, ldb, K} + M, N, out, ldo (+ live: step_dead, icz_common.h).
// nsplit is left at 1 (direct into `out`); bias / accumulate / rows_live are set by the few callers that need them.  More segments
// than GEMM_MAX_SEG are recorded in nseg and refused by gemm_f32.
inline GemmArgs gemm_args(std::initializer_list<GemmSeg> segs, int M, int N, float* out, int ldo, const int* live = nullptr) {
    GemmArgs g = {};
    g.nseg = (int)segs.size();
    int s = 0;
    for (const GemmSeg& sg : segs)
        if (s < GEMM_MAX_SEG) g.seg[s++] = sg;
    g.M = M; g.N = N; g.out = out; g.ldo = ldo; g.live = live; g.nsplit = 1;
    return g;
}

// ---- the split policy.  Products of at most `balance_above` rows (the skinny decoder steps; INT_MAX = every product, the forward
// side and the C ABI) aim at `target_wgs` workgroups (gemm_pick_split), and with `fit` the split shrinks until its slabs fit
// `cap_floats`; products of more rows balance whole rounds of workgroups over the chip under that capacity
// (gemm_pick_split_balanced, which never exceeds it).  Without `fit` the small branch can exceed the capacity: gemm_slabs refuses then.
struct SplitPolicy {
    int target_wgs;
    bool fit;
    int balance_above;
};
constexpr int GEMM_NEVER_BALANCE = 0x7fffffff;
constexpr SplitPolicy split_forward(int target_wgs) { return {target_wgs, true, GEMM_NEVER_BALANCE}; }      // y = x W^T + b, C ABI
constexpr SplitPolicy split_backward(int target_wgs, bool fit = false) { return {target_wgs, fit, 64}; }  // dgrad: steps / all (t, b) rows
int gemm_split(GemmLayout layout, const GemmArgs& g, const SplitPolicy& p, size_t cap_floats);

// ---- product to slabs: g.nsplit = ns as given (>= 1).  ns == 1: the dense product where the caller pointed g.out / g.ldo (bias and
// accumulate as set); ns > 1: slabs [ns][M][N] in `slab` (capacity cap_floats, checked; bias and accumulate dropped) for a consumer
// that sums them (sum_slabs*, launch_slab_reduce).  `who` prefixes the refusal.
int gemm_slabs(GemmLayout layout, GemmArgs& g, int ns, float* slab, size_t cap_floats, hipStream_t st, const char* who);
// the same with ns = gemm_split(p) under the slab capacity (a null `slab` has none), reported in *ns_out.  With a policy that fits or
// balances, the capacity check cannot fail.
int gemm_slabs(GemmLayout layout, GemmArgs& g, const SplitPolicy& p, float* slab, size_t cap_floats, int* ns_out, hipStream_t st, const char* who);

// ---- product to finished output: C = product + bias in g.out (row stride g.ldo).  ns == 1: written directly; else slabs through `ws`
// and launch_slab_reduce (which needs g.ldo == N and M N % 4 == 0: checked before anything is launched).
int gemm_finished(GemmLayout layout, GemmArgs& g, int ns, const float* bias, float* ws, size_t ws_floats, hipStream_t st, const char* who);
// the same with ns = gemm_split(p) under the workspace capacity
int gemm_finished(GemmLayout layout, GemmArgs& g, const SplitPolicy& p, const float* bias, float* ws, size_t ws_floats, hipStream_t st,
                  const char* who);

// out[m, n] = sum_z slab[z][m][n] (+ bias[n]), fixed z order.  M N % 4 == 0 (and N % 4 == 0 with a bias: four columns at a time).
// ns == 1 copies (+ bias): callers rely on it where a dense product sits in a slab buffer.
int launch_slab_reduce(const float* slab, int ns, int M, int N, const float* bias, float* out, hipStream_t st);
// out[n] = sum_k X[k, n] over K rows of stride ldx (bias gradients), fixed order; several sums in one launch: colsum_multi_kernel, support_kernels.h
int launch_colsum(const float* X, int K, int N, int ldx, float* out, hipStream_t st);

// ---- weight gradients: out[M x N] (ldo) (+)= dY^T X over K rows, unsplit; rows_live as in GemmArgs
int gemm_tn(const float* dY, int ldy, int M, const float* X, int ldx, int N, int K, float* out, int ldo, int accumulate, const int* rows_live,
            hipStream_t st);
// gemm_tn_split (gemm_f32.h) with its slabs summed into the dense `out` (ns = gemm_tn_split_pick > 1, slabs of ns M N floats)
int gemm_tn_split_sum(const float* dY, int ldy, int M, const float* X, int ldx, int N, int K, int ns, float* slab, const int* rows_live, float* out,
                      hipStream_t st);
// the split form where the shape is taken (too few 128 x 128 tiles to fill the chip), `out` is dense and the slabs fit `slab`; else
// gemm_tn.  `slab` must belong to the stream `st` alone (null: always gemm_tn).
int gemm_tn_auto(const float* dY, int ldy, int M, const float* X, int ldx, int N, int K, float* out, int ldo, float* slab, size_t slab_floats,
                 const int* rows_live, hipStream_t st);
// weight gradients that share dY: one launch over the column groups if gemm_tn_grouped_fits, else group by group through gemm_tn_auto
int gemm_tn_groups(const float* dY, int ldy, int M, int K, const GemmColGroup* groups, int ngroups, float* slab, size_t slab_floats,
                   const int* rows_live, hipStream_t st);

}  // namespace icz
