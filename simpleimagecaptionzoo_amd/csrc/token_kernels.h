// Device kernels that turn a row of logits into a token, a log-probability or a gradient: greedy argmax, multinomial and scheduled
// sampling selects, the REINFORCE and label-smoothing XE losses, and the two kernels the decoders launch from their beam seams.
// Reference line numbers: Models/BUTD_Model.py.
#pragma once
#include "icz_common.h"
#include "rng.h"

namespace icz {
namespace {   // internal linkage: this header is included by several translation units

// ---------------------------------------------------------------------------------------------------------
// greedy epilogue (:183): id = argmax_v logits[row, v] (first maximum wins, as torch.max does), in two stages:
//   argmax_part_kernel  grid (rows, P): block-wide (value, index) of its slice of the vocabulary -> part[row, p]
//   embed_argmax_kernel grid (E/1024, rows): reduces the P partials (tiny), records the id, and gathers the next
//                       step's embedding row (Embedding -> ReLU; eval mode, no dropout) in the same launch.
__device__ __forceinline__ void argmax_combine(float& best, int& bi, float ob, int oi) {
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
}
// (finished rows only: a step whose predict GEMM left split-K slabs goes to greedy_select_kernel, launch_greedy_select)
__global__ __launch_bounds__(256) void argmax_part_kernel(const float* __restrict__ logits, int V, int ldl, int P,
                                                          float* __restrict__ part_val, int* __restrict__ part_idx) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int row = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = ((V + P - 1) / P + 3) & ~3;
    const int v0 = p * per, v1 = min(V, v0 + per);
    const float* l = logits + (size_t)row * ldl;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = v0 + tid; v < v1; v += 256) {
        const float x = l[v];
        if (x > best) { best = x; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_combine(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
    if (lane == 0) { sv[wave] = best; si[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) argmax_combine(best, bi, sv[w], si[w]);
        part_val[row * P + p] = best;
        part_idx[row * P + p] = bi;
    }
}
__global__ __launch_bounds__(256) void embed_argmax_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx, int P,
                                                           const float* __restrict__ table, int E, float* __restrict__ emb,
                                                           int64_t* __restrict__ it_next, int64_t* __restrict__ ids_out,
                                                           int ids_stride, int t, int relu = 1) {
    const int row = blockIdx.y;
    float best = part_val[row * P];
    int bi = part_idx[row * P];
    for (int p = 1; p < P; ++p) argmax_combine(best, bi, part_val[row * P + p], part_idx[row * P + p]);
    if (bi == 0x7fffffff) bi = 0;       // a row of NaN / -inf logits never updates bi (greedy_select_kernel has the same rule): <pad>, not a wild read
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        it_next[row] = bi;
        if (ids_out) ids_out[(size_t)row * ids_stride + t] = bi;
    }
    const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= E) return;
    f32x4 x = *reinterpret_cast<const f32x4*>(table + (size_t)bi * E + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = relu ? fmaxf(x[j], 0.f) : x[j];
    *reinterpret_cast<f32x4*>(emb + (size_t)row * E + e) = x;
}

// Greedy token choice of a decoder step in ONE launch (round 3), one 1024-thread workgroup per row like the multinomial kernel:
// logits = sum of the predict GEMM's split-K slabs + bias (never written back: greedy decoding keeps no logits), argmax with ties to
// the lowest index (torch.max, :183), the id recorded, and the next step's input embedding (Embedding -> ReLU, eval mode) gathered
// by the same workgroup.  Replaces argmax_part_kernel + embed_argmax_kernel (5.6 + 4.8 us) at 33 - 64 rows; 64 workgroups leave
// the other three quarters of the chip to the sampled chain that runs beside the greedy one in an SCST step.
__global__ __launch_bounds__(1024) void greedy_select_kernel(const float* __restrict__ logits, int V, int ldl, int ns, size_t slab_stride,
                                                            const float* __restrict__ bias, const float* __restrict__ table, int E,
                                                            float* __restrict__ emb, int64_t* __restrict__ it_next,
                                                            int64_t* __restrict__ ids_out, int ids_stride, int t, int relu = 1,
                                                            uint8_t* __restrict__ unfinished = nullptr, int* __restrict__ n_unfinished = nullptr) {
    __shared__ float sv[16];
    __shared__ int si[16];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // SCST baseline only (n_unfinished != null): once EVERY row has emitted <end> nothing downstream reads the greedy ids any more
    // (get_self_critical_reward cuts each row at its <end>, Utils.py:354) -- the steps behind that point return at entry, ids = 0
    if (n_unfinished && t > 0 && n_unfinished[t - 1] == 0) {
        if (tid == 0 && ids_out) ids_out[(size_t)row * ids_stride + t] = 0;
        return;
    }
    const float* l = logits + (size_t)row * ldl;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    const bool vec = ((ldl | (int)(slab_stride & 3)) & 3) == 0 && (((uintptr_t)logits | (uintptr_t)bias) & 15) == 0;
    const int Vv = vec ? (V & ~3) : 0;
    for (int v = tid * 4; v < Vv; v += 4096) {
        f32x4 x = *reinterpret_cast<const f32x4*>(l + v);
        for (int z = 1; z < ns; ++z) x += *reinterpret_cast<const f32x4*>(l + (size_t)z * slab_stride + v);
        if (bias) x += *reinterpret_cast<const f32x4*>(bias + v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x[j] > best) { best = x[j]; bi = v + j; }
    }
    for (int v = Vv + tid; v < V; v += 1024) {
        float x = l[v];
        for (int z = 1; z < ns; ++z) x += l[(size_t)z * slab_stride + v];
        if (bias) x += bias[v];
        // strictly greater, as in the body: a thread meets its elements in ascending order, so an equal value is never at a lower index
        // -- an "equal and lower" clause here only ever fired for -inf against the start value, and sent a row of -inf logits to
        // token V & ~3 instead of <pad> whenever V % 4 != 0 on the 16-byte path
        if (x > best) { best = x; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_combine(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
    if (lane == 0) { sv[wave] = best; si[wave] = bi; }
    __syncthreads();
    best = sv[0]; bi = si[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) argmax_combine(best, bi, sv[w], si[w]);
    if ((unsigned)bi >= (unsigned)V) bi = 0;        // a row of NaN / -inf logits (diverged training) never updates bi: <pad>, not a wild read
    if (tid == 0) {
        it_next[row] = bi;
        if (ids_out) ids_out[(size_t)row * ids_stride + t] = bi;
        if (n_unfinished) {
            const bool unf = (t == 0 || unfinished[row] != 0) && bi != 2;
            unfinished[row] = unf ? 1 : 0;
            if (unf) atomicAdd(&n_unfinished[t], 1);
        }
    }
    for (int e = tid * 4; e < E; e += 4096) {
        f32x4 x = *reinterpret_cast<const f32x4*>(table + (size_t)bi * E + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = relu ? fmaxf(x[j], 0.f) : x[j];      // NIC embeds without the ReLU (NIC_Model.py:112)
        *reinterpret_cast<f32x4*>(emb + (size_t)row * E + e) = x;
    }
}

// start of a greedy chain: first input token <sta>; the per-step counters of unfinished rows (SCST baseline, may be null) = 0
__global__ void greedy_init_kernel(int64_t* it, int rows, int* n_unfinished, int T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) it[i] = 1;
    if (n_unfinished && i < T) n_unfinished[i] = 0;
}

// ---- beam search: launched by the decoders' seams (DecodeMember::gather / prologue); the search's own kernels: beam_kernels.h ----
// state re-gather: out[row,:] = in[src_row[row],:] for the four state tensors
__global__ __launch_bounds__(256) void beam_gather_kernel(const int32_t* __restrict__ src_row, int H,
                                                          const float* __restrict__ a0, const float* __restrict__ a1,
                                                          const float* __restrict__ a2, const float* __restrict__ a3,
                                                          float* __restrict__ o0, float* __restrict__ o1,
                                                          float* __restrict__ o2, float* __restrict__ o3, int src_div) {
    const int row = blockIdx.y;
    const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (j >= H) return;
    // src_div = k after a compact first step (the state of image img sits in row img, src_row says img k + 0), else 1
    const size_t s = (size_t)(src_row[row] / src_div) * H + j, d = (size_t)row * H + j;
    *reinterpret_cast<f32x4*>(o0 + d) = *reinterpret_cast<const f32x4*>(a0 + s);
    *reinterpret_cast<f32x4*>(o1 + d) = *reinterpret_cast<const f32x4*>(a1 + s);
    *reinterpret_cast<f32x4*>(o2 + d) = *reinterpret_cast<const f32x4*>(a2 + s);
    *reinterpret_cast<f32x4*>(o3 + d) = *reinterpret_cast<const f32x4*>(a3 + s);
}

// out[row,:] = in[img_of_row[row],:]   (features.expand(k, ...) of the reference's beam search)
__global__ __launch_bounds__(256) void beam_expand_rows_kernel(const float* __restrict__ in, const int32_t* __restrict__ img_of_row, int E,
                                                               float* __restrict__ out) {
    const int row = blockIdx.y;
    const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= E) return;
    *reinterpret_cast<f32x4*>(out + (size_t)row * E + e) = *reinterpret_cast<const f32x4*>(in + (size_t)img_of_row[row] * E + e);
}

// ---------------------------------------------------------------------------------------------------------
// sample_rl epilogue (:221-233): logp = log_softmax(logits); draw ~ multinomial(exp(logp)) by inverse CDF
// (smallest i with cumsum(p)[i] > u * sum(p), float64 -- the contract shared with the oracle); store logp[draw];
// unfinished &= (draw != <end>); it = draw * unfinished.  A row block = one workgroup; each thread owns a
// contiguous slice of the vocabulary so the global "first index above target" is the minimum over threads.
// Steps after every row has finished are left zero, as the reference's early break does (:233).
struct SampleSelArgs {
    const float* logits; int V; int ldl;
    const float* uniforms;        // [rows] for this step or null (Philox)
    const uint64_t* seed_p; int t; int T;
    uint8_t* unfinished;          // [rows] in/out
    int* n_unfinished;            // [T] counters (zeroed before the rollout)
    int64_t* seq_out; float* logp_out;   // [rows, T]
    int64_t* it_next;             // [rows]
    int32_t* draw_out;            // [rows] raw draw (for backward)
    float* lse_out;               // [rows] max + log(sum exp) (for backward)
    // optional fused epilogue: the next step's input embedding emb_next[row,:] = drop(relu(table[it_next[row],:])) (the
    // embed_kernel of step t + 1, :77-81) with that step's dropout configuration
    const float* emb_table; float* emb_next; int E; DropCfg emb_drop;
    // ns > 1: `logits` holds the ns split-K slabs of the predict GEMM (slab z at + z * slab_stride, no bias yet); the kernel
    // sums them in slab order, adds bias[v] and leaves the finished row in logits_store (the saved logits of backward)
    int ns; size_t slab_stride; const float* bias; float* logits_store;
    int* live_rows;               // optional: (number of steps the reference ran so far) x rows -- the (t, b) rows the batched GEMMs of
                                  // the backward pass need to read (GemmArgs::rows_live, embed_grad_kernel)
    // merged chain (row0 > 0, sample_select_kernel<true>): rows < row0 are the greedy baseline's
    int row0; int64_t* ids_out; uint8_t* g_unfinished; int* n_any;
};
constexpr int SEL_THREADS = 1024;       // 16 waves per row: the row (40 KB) sits in LDS
// the largest row of the select kernels (sample_select_kernel, ss_select_kernel): dynamic LDS beside their static arrays in the 160 KB
// of a workgroup; both launch helpers raise the kernels' dynamic-LDS limit to it once and refuse a longer row on the host
constexpr size_t SEL_LDS_MAX = 159 * 1024;
inline bool sel_row_fits_lds(int V) { return V >= 1 && sizeof(float) * (size_t)V <= SEL_LDS_MAX; }
__device__ __forceinline__ float block_max_n(float v, float* sm, int nw) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0];
    for (int w = 1; w < nw; ++w) r = fmaxf(r, sm[w]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_sum_n(float v, float* sm, int nw) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0];
    for (int w = 1; w < nw; ++w) r += sm[w];
    __syncthreads();
    return r;
}
// Inverse-CDF draw over the probabilities in LDS (the sampler contract of torch.multinomial's stand-in, oracle/butd.py
// inverse_cdf_draw): smallest v with cumsum(p)[v] > u * sum(p), sums in float64.  Every thread of the SEL_THREADS-wide
// workgroup calls it; the result (clamped to V - 1) is valid in thread 0 after the call.
__device__ __forceinline__ int block_inverse_cdf(const float* srow, int V, float u, double* smd, int* smi) {
    constexpr int NW = SEL_THREADS / 64;
    const int tid = threadIdx.x;
    // contiguous slice per thread -> the global "first index above target" is the minimum over threads
    const int per = (V + SEL_THREADS - 1) / SEL_THREADS;
    const int v0 = min(V, tid * per), v1 = min(V, v0 + per);
    double loc = 0.0;
    for (int v = v0; v < v1; ++v) loc += (double)srow[v];
    // exclusive prefix over the slice sums: wave-level inclusive scan (shuffles) + the wave totals
    double inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(inc, o, 64);
        if ((tid & 63) >= o) inc += up;
    }
    if ((tid & 63) == 63) smd[tid >> 6] = inc;
    __syncthreads();
    double wave_off = 0.0, total = 0.0;
    for (int w = 0; w < NW; ++w) {
        if (w < (tid >> 6)) wave_off += smd[w];
        total += smd[w];
    }
    const double prefix = wave_off + inc - loc;
    const double target = (double)u * total;
    int cand = 0x7fffffff;
    {
        double run = prefix;
        for (int v = v0; v < v1; ++v) {
            run += (double)srow[v];
            if (run > target) { cand = v; break; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    if ((tid & 63) == 0) smi[tid >> 6] = cand;
    __syncthreads();
    int d = 0;
    if (tid == 0) {          // only thread 0 reads smi[]: the caller may reuse it right away
        d = smi[0];
        for (int w = 1; w < NW; ++w) d = min(d, smi[w]);
        if (d > V - 1) d = V - 1;
    }
    return d;
}

// Scheduled sampling, DecoderRNN.forward (BUTD_Model.py:120-130): from time step 2 on, row b of the XE forward feeds a draw
// from softmax(logits of step t-1) instead of its caption token when gate < ss_prob.  One workgroup per active row; a row
// whose gate is not below ss_prob leaves at once (its token stays the caption's).
struct SsSelArgs {
    const float* logits_prev;  // [rows, ldl] logits of step t - 1
    int ldl, V, t;
    float ss_prob;
    const float* gate;         // [B] explicit uniforms for this step, or nullptr -> Philox (RNG_SS_GATE)
    const float* draw;         // [B] explicit uniforms for the inverse-CDF draw, or nullptr -> Philox (RNG_SS_DRAW)
    const uint64_t* seed_p;
    int64_t* tok;              // [B] tokens fed at step t (in: caption tokens; out: mixed)
};
__global__ __launch_bounds__(SEL_THREADS) void ss_select_kernel(SsSelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float srow[];
    __shared__ float smf[16];
    __shared__ double smd[16];
    __shared__ int smi[16];
    constexpr int NW = SEL_THREADS / 64;
    const int row = blockIdx.x, tid = threadIdx.x;
    const float g = a.gate ? a.gate[row] : rng_uniform(*a.seed_p, (uint32_t)a.t, (uint64_t)row, RNG_SS_GATE);
    if (!(g < a.ss_prob)) return;
    const float* l = a.logits_prev + (size_t)row * a.ldl;
    float mx = -INFINITY;
    for (int v = tid; v < a.V; v += SEL_THREADS) { const float x = l[v]; srow[v] = x; mx = fmaxf(mx, x); }
    mx = block_max_n(mx, smf, NW);
    float se = 0.f;
    for (int v = tid; v < a.V; v += SEL_THREADS) { const float e = expf(srow[v] - mx); srow[v] = e; se += e; }
    se = block_sum_n(se, smf, NW);
    for (int v = tid; v < a.V; v += SEL_THREADS) srow[v] = srow[v] / se;                  // torch.softmax
    __syncthreads();
    const float u = a.draw ? a.draw[row] : rng_uniform(*a.seed_p, (uint32_t)a.t, (uint64_t)row, RNG_SS_DRAW);
    const int d = block_inverse_cdf(srow, a.V, u, smd, smi);
    if (tid == 0) a.tok[row] = d;
}
// tokens of XE step t (t >= 2) for the `rows` active rows; gate / draw: explicit [T, B] arrays or nullptr (Philox)
inline int ss_select_launch(hipStream_t st, int rows, const float* logits_prev, int ldl, int V, int t, int B, float ss_prob,
                            const float* gate, const float* draw, const uint64_t* seed_p, int64_t* tok_t) {
    static bool lds_set = false;
    if (!lds_set) {
        ICZ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ss_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEL_LDS_MAX));
        lds_set = true;
    }
    ICZ_REQUIRE(sel_row_fits_lds(V), "scheduled sampling: a row of %d logits does not fit in LDS (at most %d)", V, (int)(SEL_LDS_MAX / sizeof(float)));
    SsSelArgs sa = {};
    sa.logits_prev = logits_prev; sa.ldl = ldl; sa.V = V; sa.t = t; sa.ss_prob = ss_prob;
    sa.gate = gate ? gate + (size_t)t * B : nullptr;
    sa.draw = draw ? draw + (size_t)t * B : nullptr;
    sa.seed_p = seed_p; sa.tok = tok_t;
    hipLaunchKernelGGL(ss_select_kernel, dim3(rows), dim3(SEL_THREADS), sizeof(float) * V, st, sa);
    return ICZ_OK;
}
// One workgroup of 16 waves per row.  Passes: (1) finished logits x = sum of the predict GEMM's split-K slabs + bias -> LDS (and
// the saved-logits slot of backward), row maximum M; (2) every thread takes a contiguous slice of the row: float32 sum of
// exp(x - M) -> lse, then the float64 sum of p_v = expf((x_v - M) - lse) over its slice and a block scan -> total and the slice's
// prefix; (3) the thread whose slice crosses u * total walks it again (p recomputed: the same float expression) and reports the
// first index above the target.  Round 2's kernel made two more passes over the row (p written back to LDS, strided re-reads).
// MEASURED (round 3, same box): a two-launch form over the whole chip (rows x 16 slice workgroups for the sums, then one small
// workgroup per row for the draw: 7.9 + 8.1 us against 15.4 us for round 2's kernel) made the SCST rollouts SLOWER, 2.83 -> 3.09 ms:
// the sampled chain runs beside the greedy chain, and a launch that fills every CU stalls the other chain's kernels, while this
// one leaves three quarters of the chip to them.
// MG = true: the merged chain of a small SCST batch (Butd::merged_chain): rows [0, row0) are the GREEDY baseline's rows (evaluation
// mode: argmax with ties to the lowest index, BUTD_Model.py:183, next embedding without dropout, ids to ids_out), rows >= row0 the
// sampled rollout's (row - row0 of every per-row array of the sampled batch).  Two counters: n_unfinished[t] = sampled rows still
// unfinished (the reference's break, :233: behind it seq / logp are zeros and BPTT has nothing to do), n_any[t] = those + the
// greedy rows that have not emitted <end> (0 = no kernel of the remaining steps runs).
template <bool MG>
__global__ __launch_bounds__(SEL_THREADS) void sample_select_kernel(SampleSelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float srow[];     // V floats: the finished logits of the row
    __shared__ float smf[16];
    __shared__ double smd[16];
    __shared__ int smi[16];
    constexpr int NW = SEL_THREADS / 64;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sr = MG ? row - a.row0 : row;                 // row of the sampled batch; < 0: a greedy row of the merged chain
    const bool greedy_row = MG && sr < 0;
    const float sc = a.emb_drop.mode ? 2.0f : 1.0f;
    const int* const gate = MG ? a.n_any : a.n_unfinished;
    const bool all_dead = a.t > 0 && gate[a.t - 1] == 0;    // the kernels of this step returned at entry (step_dead)
    if (all_dead || (MG && !greedy_row && a.t > 0 && a.n_unfinished[a.t - 1] == 0)) {
        // every (sampled) row has finished: zeros, as the reference's early break leaves them (:233)
        if (tid == 0) {
            if (greedy_row) a.ids_out[(size_t)row * a.T + a.t] = 0;
            else { a.seq_out[(size_t)sr * a.T + a.t] = 0; a.logp_out[(size_t)sr * a.T + a.t] = 0.f; }
            a.it_next[row] = 0;
            a.draw_out[row] = -1;
            a.lse_out[row] = 0.f;
        }
        if (MG && !all_dead && a.emb_next)                  // the greedy half goes on: this row keeps running on <pad> (finite, never read)
            for (int e = tid * 4; e < a.E; e += 4 * SEL_THREADS) {
                f32x4 x = *reinterpret_cast<const f32x4*>(a.emb_table + e);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = fmaxf(x[j], 0.f);
                *reinterpret_cast<f32x4*>(a.emb_next + (size_t)row * a.E + e) = x;
            }
        return;
    }
    if (a.live_rows && sr == 0 && tid == 0) *a.live_rows = (a.t + 1) * (int)gridDim.x;
    const float* l = a.logits + (size_t)row * a.ldl;
    const float u = greedy_row ? 0.f : (a.uniforms ? a.uniforms[sr] : rng_uniform(*a.seed_p, (uint32_t)a.t, (uint64_t)sr));
    const bool was_unf = greedy_row ? (a.t == 0 || a.g_unfinished[row] != 0) : a.unfinished[sr] != 0;   // loaded early: the tail below is a chain of dependent accesses
    // pass 1: one coalesced pass over HBM / L2; every later pass runs out of LDS
    float mx = -INFINITY;
    if (a.ns > 1) {
        float* ls = a.logits_store + (size_t)row * a.ldl;
        const bool vec = ((a.ldl | (int)(a.slab_stride & 3)) & 3) == 0 &&
                         (((uintptr_t)a.logits | (uintptr_t)a.bias | (uintptr_t)a.logits_store) & 15) == 0;
        const int Vv = vec ? (a.V & ~3) : 0;
        for (int v = tid * 4; v < Vv; v += 4 * SEL_THREADS) {
            f32x4 x = *reinterpret_cast<const f32x4*>(l + v);
            for (int z = 1; z < a.ns; ++z) x += *reinterpret_cast<const f32x4*>(l + (size_t)z * a.slab_stride + v);
            x += *reinterpret_cast<const f32x4*>(a.bias + v);
            *reinterpret_cast<f32x4*>(ls + v) = x;
            *reinterpret_cast<f32x4*>(srow + v) = x;
            mx = fmaxf(mx, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
        }
        for (int v = Vv + tid; v < a.V; v += SEL_THREADS) {
            float x = l[v];
            for (int z = 1; z < a.ns; ++z) x += l[(size_t)z * a.slab_stride + v];
            x += a.bias[v];
            ls[v] = x; srow[v] = x; mx = fmaxf(mx, x);
        }
    } else {
        for (int v = tid; v < a.V; v += SEL_THREADS) { const float x = l[v]; srow[v] = x; mx = fmaxf(mx, x); }
    }
    mx = block_max_n(mx, smf, NW);
    if (greedy_row) {
        // argmax, ties to the lowest index: the first element of the row that equals its maximum
        const int per = (a.V + SEL_THREADS - 1) / SEL_THREADS;
        const int v0 = min(a.V, tid * per), v1 = min(a.V, v0 + per);
        int cand = 0x7fffffff;
        for (int v = v0; v < v1; ++v)
            if (srow[v] == mx) { cand = v; break; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
        if (lane == 0) smi[wave] = cand;
        __syncthreads();
        int bi = smi[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) bi = min(bi, smi[w]);
        if ((unsigned)bi >= (unsigned)a.V) bi = 0;      // a row of NaN logits (diverged training): <pad>, not a wild read
        if (tid == 0) {
            const bool unf = was_unf && bi != 2;
            a.g_unfinished[row] = unf ? 1 : 0;
            a.ids_out[(size_t)row * a.T + a.t] = bi;
            a.it_next[row] = bi;
            a.draw_out[row] = -1;                       // no gradient flows into an evaluation-mode row (reinforce_dlogits_kernel)
            a.lse_out[row] = 0.f;
            if (unf) atomicAdd(&a.n_any[a.t], 1);
        }
        if (a.emb_next)
            for (int e = tid * 4; e < a.E; e += 4 * SEL_THREADS) {
                f32x4 x = *reinterpret_cast<const f32x4*>(a.emb_table + (size_t)bi * a.E + e);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = fmaxf(x[j], 0.f);
                *reinterpret_cast<f32x4*>(a.emb_next + (size_t)row * a.E + e) = x;
            }
        return;
    }
    // pass 2: contiguous slice per thread -> the first index above the target is the minimum over threads.
    // p_v = exp(log_softmax(x)_v) = expf((x_v - M) - lse) with lse = logf(sum expf(x - M)) in float32 -- the reference's own
    // float expression (:221-223), so that the float64 CDF below agrees with the oracle's to the last bit in all but a few draws in 10^5
    const int per = (a.V + SEL_THREADS - 1) / SEL_THREADS;
    const int v0 = min(a.V, tid * per), v1 = min(a.V, v0 + per);
    float se = 0.f;
    for (int v = v0; v < v1; ++v) se += expf(srow[v] - mx);
    se = block_sum_n(se, smf, NW);
    const float lse = logf(se);
    double loc = 0.0;
    for (int v = v0; v < v1; ++v) loc += (double)expf((srow[v] - mx) - lse);
    double inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) smd[wave] = inc;
    __syncthreads();
    double wave_off = 0.0, total = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const double t = smd[w];
        if (w < wave) wave_off += t;
        total += t;
    }
    const double target = (double)u * total;
    // pass 3: only the slice that crosses the target is walked again
    int cand = 0x7fffffff;
    {
        // [lower, upper) of this thread's slice: lower IS the previous lane's upper (the scan's own value, shuffled -- not
        // inc - loc, which can differ from it in the last place and leave a one-ulp gap that no thread claims: the draw then fell
        // through to V - 1); across waves the lower bound of lane 0 is the same sum of wave totals as the previous wave's upper
        const double prev = __shfl_up(inc, 1, 64);
        double run = wave_off + (lane ? prev : 0.0);
        if (run <= target && wave_off + inc > target) {
            cand = v1 - 1;                               // the slice's last element carries the scan's own cumulative value
            for (int v = v0; v < v1 - 1; ++v) {
                run += (double)expf((srow[v] - mx) - lse);
                if (run > target) { cand = v; break; }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    if (lane == 0) smi[wave] = cand;
    __syncthreads();
    int tok = 0;
    {
        int d = smi[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) d = min(d, smi[w]);
        if (d > a.V - 1) d = a.V - 1;                // rounding at u -> 1: the last token
        const bool unf = was_unf && (d != 2);
        tok = unf ? d : 0;
        if (tid == 0) {
            a.unfinished[sr] = unf ? 1 : 0;
            a.seq_out[(size_t)sr * a.T + a.t] = tok;
            a.logp_out[(size_t)sr * a.T + a.t] = (srow[d] - mx) - lse;
            a.it_next[row] = tok;
            a.draw_out[row] = d;
            a.lse_out[row] = mx + lse;
            if (unf) {
                atomicAdd(&a.n_unfinished[a.t], 1);
                if (MG) atomicAdd(&a.n_any[a.t], 1);
            }
        }
    }
    if (a.emb_next)
        for (int e = tid * 4; e < a.E; e += 4 * SEL_THREADS) {
            f32x4 x = *reinterpret_cast<const f32x4*>(a.emb_table + (size_t)tok * a.E + e);
            const uint32_t k = a.emb_drop.mode ? a.emb_drop.keep4((uint64_t)sr * a.E + e) : 0xFu;
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = ((k >> j) & 1u) ? fmaxf(x[j], 0.f) * sc : 0.f;
            *reinterpret_cast<f32x4*>(a.emb_next + (size_t)row * a.E + e) = x;
        }
}
// One rule for every caller (the rollouts of the three decoders and icz_test_sample_select): the row sits in dynamic LDS beside the
// kernel's 256 bytes of static arrays, the dynamic limit is raised once to SEL_LDS_MAX (as ss_select_launch does), and a row above it is
// refused on the host -- without the raised limit a vocabulary above 16384 (64 KB) could not launch, and nothing said so.
// (`lds_set` is the project's pattern for such attributes, ss_select_launch and the GEMMs included: once per translation unit and
// process, for the device current at the first call, unsynchronised -- one GPU and one launching thread per process, as every
// caller here is; a process that drove a second device would have to raise the limit there itself.)
inline int launch_sample_select(hipStream_t st, int rows, const SampleSelArgs& a) {
    static bool lds_set = false;
    ICZ_REQUIRE(sel_row_fits_lds(a.V), "sample select: a row of %d logits does not fit in LDS (at most %d)", a.V, (int)(SEL_LDS_MAX / sizeof(float)));
    if (!lds_set) {
        ICZ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sample_select_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEL_LDS_MAX));
        ICZ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sample_select_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEL_LDS_MAX));
        lds_set = true;
    }
    if (a.row0 > 0) hipLaunchKernelGGL(sample_select_kernel<true>, dim3(rows), dim3(SEL_THREADS), sizeof(float) * a.V, st, a);
    else hipLaunchKernelGGL(sample_select_kernel<false>, dim3(rows), dim3(SEL_THREADS), sizeof(float) * a.V, st, a);
    return ICZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// RewardCriterion (Utils.py:295-317): mask[b,0] = 1, mask[b,t] = (seq[b,t-1] > 0);
//   loss = -sum(logp * reward * mask) / sum(mask).   One workgroup; also emits coef[b,t] = -reward*mask/denom
// (= d loss / d logp) for the gradient kernel.  denom = mask_sum_global if > 0 else the local mask sum.
__global__ __launch_bounds__(256) void reinforce_loss_kernel(const float* __restrict__ logp, const int64_t* __restrict__ seq,
                                                             const float* __restrict__ reward, int B, int T,
                                                             const float* __restrict__ mask_sum_global_p, float* __restrict__ coef,
                                                             float* __restrict__ loss_out, float* __restrict__ mask_sum_out) {
    __shared__ float smf[4];
    const int tid = threadIdx.x;
    float ms = 0.f, ls = 0.f;
    for (int i = tid; i < B * T; i += 256) {
        const int t = i % T;
        const float m = (t == 0) ? 1.f : (seq[i - 1] > 0 ? 1.f : 0.f);
        ms += m;
        ls += -logp[i] * reward[i] * m;
    }
    ms = block_sum_256(ms, smf);
    ls = block_sum_256(ls, smf);
    const float msg = mask_sum_global_p ? mask_sum_global_p[0] : 0.f;
    const float denom = msg > 0.f ? msg : ms;
    for (int i = tid; i < B * T; i += 256) {
        const int t = i % T;
        const float m = (t == 0) ? 1.f : (seq[i - 1] > 0 ? 1.f : 0.f);
        coef[i] = -reward[i] * m / denom;
    }
    if (tid == 0) {
        if (loss_out) loss_out[0] = ls / denom;
        if (mask_sum_out) mask_sum_out[0] = ms;
    }
}

// d loss / d logits for the whole rollout (row = t*B + b):
//   dlogits[row,v] = coef[b,t] * (1[v == draw] - softmax(logits)[v])         (log_softmax + gather backward)
// Written in place over the saved logits; pad columns [V, ldl) are zeroed.
__global__ __launch_bounds__(256) void reinforce_dlogits_kernel(float* __restrict__ logits, int V, int ldl,
                                                                const int32_t* __restrict__ draw, const float* __restrict__ lse,
                                                                const float* __restrict__ coef, int B, int T, int Bs = 0, int row0 = 0) {
    // Bs > 0: the slots hold Bs rows per step, of which rows [row0, row0 + B) are the sampled rollout's (merged chain); the rows in
    // front are evaluation-mode rows (draw = -1): zero gradient
    const int row = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= ldl) return;
    const int stride = Bs > 0 ? Bs : B;
    const int t = row / stride, b = row % stride - row0;
    float* l = logits + (size_t)row * ldl;
    const float c = b >= 0 ? coef[(size_t)b * T + t] : 0.f;
    const int d = draw[row];
    float g = 0.f;
    if (v < V && d >= 0 && c != 0.f) g = c * ((v == d ? 1.f : 0.f) - expf(l[v] - lse[row]));
    l[v] = g;
}

// ---------------------------------------------------------------------------------------------------------
// LabelSmoothingLoss (Utils.py:268-286) on one time step of the XE forward (rows = rows active at t):
//   loss_row = sum_v true_v (log true_v - logp_v),  true = 1-s at the target, s/(V-1) elsewhere
//   dlogits  = (softmax - true) / N_tokens          (KLDiv(log_softmax) backward)
// One workgroup per row; per-row loss goes to loss_rows (summed later in fixed order).
// All time steps in one launch: grid (B, T), block (b, t) = row t * B + b of the saved logits, active while b < rows.n[t] (the
// captions are sorted by decreasing length, Engine.py:178); target = captions[b, t + 1].  One launch per step left the chip
// to at most B workgroups seventeen times per XE step.
constexpr int XE_MAX_T = 128;
struct XeRows { int n[XE_MAX_T]; };
// One active row l [ldl] (target *tgp, read behind the sum-exp) by the workgroup's 256 threads: the loss of the row comes back (on every thread), the gradient goes
// over the row, zeros into the pad columns [V, ldl).  Shared by the two kernels below, so that a row gives the same bits through either.
__device__ __forceinline__ float xe_row_loss_dlogits(float* __restrict__ l, int V, int ldl, const int64_t* __restrict__ tgp, float smoothing, float inv_n,
                                                     float* smf) {
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, l[v]);
    mx = block_max_256(mx, smf);
    float se = 0.f;
    for (int v = tid; v < V; v += 256) se += expf(l[v] - mx);
    se = block_sum_256(se, smf);
    const float lse = mx + logf(se);
    const int tg = (int)tgp[0];
    const float conf = 1.f - smoothing, low = smoothing / (float)(V - 1);
    const float lconf = conf > 0.f ? logf(conf) : 0.f, llow = low > 0.f ? logf(low) : 0.f;
    float ls = 0.f;
    for (int v = tid; v < ldl; v += 256) {
        float g = 0.f;
        if (v < V) {
            const float lp = l[v] - lse;
            const float tr = (v == tg) ? conf : low;
            if (tr > 0.f) ls += tr * (((v == tg) ? lconf : llow) - lp);
            g = (expf(lp) - tr) * inv_n;
        }
        l[v] = g;
    }
    return block_sum_256(ls, smf);
}

__global__ __launch_bounds__(256) void xe_loss_dlogits_kernel(float* __restrict__ logits, int V, int ldl,
                                                              const int64_t* __restrict__ captions, int L, int B, XeRows rows,
                                                              float smoothing, float inv_n_host, const float* __restrict__ n_dev,
                                                              float* __restrict__ loss_rows) {
    __shared__ float smf[4];
    const int b = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    if (b >= rows.n[t]) {          // inactive (t, b): its gradient row must be zero for the batched GEMMs of the backward pass (the batched
        float* z = logits + (size_t)(t * B + b) * ldl;      // vocabulary projection of the forward pass fills every row)
        for (int v = tid; v < ldl; v += 256) z[v] = 0.f;
        return;
    }
    // data-parallel: the all-reduced token count, a device scalar (0 = never handed over: the local count, as the SCST path does)
    const float inv_n = (n_dev && n_dev[0] > 0.f) ? 1.0f / n_dev[0] : inv_n_host;
    const int row = t * B + b;
    const float ls = xe_row_loss_dlogits(logits + (size_t)row * ldl, V, ldl, captions + (size_t)b * L + t + 1, smoothing, inv_n, smf);
    if (tid == 0) loss_rows[row] = ls;
}

// The same loss over the image-major rows of a grouped XE forward (K captions per image, row = img * K + k, in no length order): the
// active (row, t) are not a prefix of the rows of step t, so the mask is t < len[row], read from a device array of per-row step counts.
// One workgroup (four waves) per (row, t) = row t * rows + row of the stored logits [T rows, ldl] (ldl % 4 == 0, 16-byte aligned rows).
// An inactive (row, t) is written as zeros, 16 bytes per thread and store, WITHOUT BEING READ (the forward pass ran it on <pad>; NaN
// there does not matter) and leaves 0 in loss_rows.  An active one goes through xe_row_loss_dlogits: the row is read three times (max,
// sum-exp, gradient; 40 KB at V = 10 102, the second and third time from L2), nothing of it is kept in LDS, so there is no cap on V.
__global__ __launch_bounds__(256) void xe_group_loss_dlogits_kernel(float* __restrict__ logits, int V, int ldl,
                                                                    const int64_t* __restrict__ captions, int L, int rows,
                                                                    const int32_t* __restrict__ len, float smoothing, float inv_n_host,
                                                                    const float* __restrict__ n_dev, float* __restrict__ loss_rows) {
    __shared__ float smf[4];
    const int r = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const size_t row = (size_t)t * rows + r;
    float* l = logits + row * ldl;
    if (t >= len[r]) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int v = tid * 4; v < ldl; v += 1024) *reinterpret_cast<f32x4*>(l + v) = z;
        if (tid == 0) loss_rows[row] = 0.f;
        return;
    }
    const float inv_n = (n_dev && n_dev[0] > 0.f) ? 1.0f / n_dev[0] : inv_n_host;
    const float ls = xe_row_loss_dlogits(l, V, ldl, captions + (size_t)r * L + t + 1, smoothing, inv_n, smf);
    if (tid == 0) loss_rows[row] = ls;
}

// sum of n floats in fixed order by one workgroup, scaled
__global__ __launch_bounds__(256) void sum_scale_kernel(const float* __restrict__ x, int n, float scale_host, const float* __restrict__ n_dev,
                                                        float* __restrict__ out) {
    __shared__ float smf[4];
    const float scale = (n_dev && n_dev[0] > 0.f) ? 1.0f / n_dev[0] : scale_host;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += x[i];
    s = block_sum_256(s, smf);
    if (threadIdx.x == 0) out[0] = s * scale;
}

}  // namespace
}  // namespace icz
