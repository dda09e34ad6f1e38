// Per-image beam expand / prune kernels of the shared beam-search driver (beam.hip); the state re-gather and the row expansion the
// decoders launch from their seams live in token_kernels.h.
#pragma once
#include "icz_common.h"

namespace icz {

// A constrained search's side of one step (icz_beam_constraints): the image's k = 2^C * beam rows are 2^C states of `beam` slots.
constexpr int BEAM_CONS_MAX_C = 3, BEAM_CONS_MAX_A = 4, BEAM_CONS_SLOTS = BEAM_CONS_MAX_C * BEAM_CONS_MAX_A, BEAM_CONS_MAX_ROWS = 32;
struct BeamCons {
    const int32_t* words;   // [n_img, C, A] word ids, -1 = empty slot
    int C, A, beam;
    int* cap;               // [n_img, 2^C] capacity of a state: beam minus its <end> retirements (n_act [n_img, 2^C] <= cap)
    float* force_val;       // [rows, 12] score of constraint word c * 4 + a on every scored row (-inf: n-gram-banned or empty slot)
    int32_t* hyp_state;     // [rows] state of every listed retirement, beside hyp_seq / hyp_score / hyp_len
};

namespace {

constexpr int BEAM_MAX_K = 8;

struct BeamArgs {
    const float* logits; int V; int ldl; int k; int step; int L;   // L = max_steps + 1 (sequence capacity)
    int* n_act;             // [n_img]   active beams (the reference's shrinking k); grouped search: [n_img, groups]
    float* run;             // [n_img,k] running scores of the active beams
    const int32_t* seqs_in; int32_t* seqs_out;     // [n_img,k,L]
    int32_t* src_row;       // [n_img*k] decoder row whose state feeds this row next step
    int64_t* it_next;       // [n_img*k]
    float* best_score; int* best_len; int32_t* best_seq; int* has_complete;   // best finished hypothesis per image
    int* n_live;            // [1] number of images that still have active beams after this step
    // n-best list (null = off): every retirement of image img in order, slot img * k + h, h < hyp_cnt[img] <= k
    int32_t* hyp_seq; float* hyp_score; int* hyp_len; int* hyp_cnt;      // [n_img,k,L] [n_img,k] [n_img,k] [n_img]
};

// n-gram blocking (ngram = n > 0): the row with prefix y_0 .. y_s (s = step - 1) may not take token v when the n-gram
// (y_{s-n+2} .. y_s, v) already occurs in the prefix.  The first s - n + 2 threads test one start position i each and append
// y_{i+n-1} to the LDS list on a match (duplicates are harmless); at most step - n + 1 <= 255 entries, usually none.  Returns the
// count.  Called by every thread of the workgroup (it synchronises), with step >= ngram.
__device__ inline int beam_ban_list(const int32_t* __restrict__ prefix, int step, int ngram, int* s_ban, int* s_nban) {
    if (threadIdx.x == 0) *s_nban = 0;
    __syncthreads();
    const int s = step - 1, i = threadIdx.x;
    if (i < s - ngram + 2) {
        bool hit = true;
        for (int t = 0; t < ngram - 1; ++t) hit &= prefix[i + t] == prefix[s - ngram + 2 + t];
        if (hit) s_ban[atomicAdd(s_nban, 1)] = prefix[i + ngram - 1];
    }
    __syncthreads();
    return *s_nban;
}

__device__ inline bool beam_banned(int v, const int* s_ban, int nban) {
    bool b = false;
    for (int q = 0; q < nban; ++q) b |= s_ban[q] == v;
    return b;
}

// Constrained search (BeamCons, decoder_core.h): the image's constraint words in LDS, slot c * 4 + a (-1: empty).  Every thread calls
// it; the caller synchronises before reading s_cw.
__device__ inline void beam_cons_words(const BeamCons& cn, int img, int* s_cw) {
    const int t = threadIdx.x;
    if (t < BEAM_CONS_SLOTS) {
        const int c = t / BEAM_CONS_MAX_A, a = t % BEAM_CONS_MAX_A;
        s_cw[t] = (c < cn.C && a < cn.A) ? cn.words[((size_t)img * cn.C + c) * cn.A + a] : -1;
    }
}

// Constrained search, rows state-major (row img * k + s * beam + j, k = 2^C * beam), n_act / cap [n_img, 2^C]: a live row of state s
// emits cap[s] ordinary candidates (the state's remaining capacity; its live beams never exceed it).  Step 1 needs no special case:
// the search starts with n_act = 1 in state 0 and 0 elsewhere.
__device__ inline int beam_row_cands_states(const int* __restrict__ n_act, const BeamCons& cn, int img, int r) {
    const int S = 1 << cn.C, s = r / cn.beam, j = r % cn.beam;
    return j < n_act[img * S + s] ? min(max(cn.cap[img * S + s], 0), BEAM_MAX_K) : 0;
}

// Candidates the row-top-k emits for row `row` (r = its slot within its image) this step; 0: the row is not scored.
// Plain search: every live row emits n_act[img]; step 1 scores row 0 only (:273-274).
// Grouped (diverse) search, rows group-major (row img * k + g * kg + j, kg = k / groups), n_act [n_img, groups]: a live row of
// group g emits min(k, n_act[0] + ... + n_act[g]) -- at most that many tokens are penalised before group g selects and a penalty
// only lowers a key, so the group's top n_act[g] lie within each row's unpenalised top (n_act[g] + #penalised).  Step 1 scores
// the image's row 0 with k candidates, which every group reads.
template <bool GROUPED>
__device__ inline int beam_row_cands(const int* __restrict__ n_act, int img, int r, int k, int groups, int step) {
    if (!GROUPED) {
        const int na = n_act[img];
        return r < ((step == 1) ? 1 : na) ? na : 0;
    }
    if (step == 1) return r == 0 ? k : 0;
    const int kg = k / groups, g = r / kg;
    int c = 0;
    for (int q = 0; q <= g; ++q) c += n_act[img * groups + q];
    return (r % kg) < n_act[img * groups + g] ? min(k, c) : 0;
}

// Beam expand / prune of one step (:271-300) in two launches:
//   beam_rowtopk_kernel  grid (n_img * k): one workgroup per decoder row -> its log-softmax normaliser and its own best
//                        n_act candidates (value = run + log_softmax, index v); every row of every image in parallel
//   beam_merge_kernel    grid (n_img), one wave: top-n_act of the <= k*k row candidates (ties -> lower flat index r*V+v,
//                        the order of a top-k over the flattened [k, V] scores), retire finished beams, compact the rest
// The global top-n_act are contained in the union of the per-row top-n_act, so the result equals a search over all k*V.
// Blocking (ngram > 0, from step ngram on; seqs_in / L: the rows' prefixes): a banned token scores -inf after the log-softmax,
// whose normaliser still runs over the whole row.  Here a banned token is skipped where it would enter a thread's list; BAN = false
// (no list this step) compiles the kernel without the test (the list check costs it 20 VGPRs and its occupancy).
// CONS (a constrained search, always with BAN): the image's constraint words join the list behind the n-gram bans (at most 255 + 12
// entries), so the row's top cap[state] covers the other tokens only, and the score of every constraint word goes to force_val
// [rows, 12] (slot c * 4 + a; -inf: n-gram-banned or an empty slot) with the mx / ls of the row's top-k.
template <bool BAN, bool GROUPED, bool CONS = false>
__global__ __launch_bounds__(256) void beam_rowtopk_kernel(const float* __restrict__ logits, int V, int ldl, int k, int step,
                                                           const int* __restrict__ n_act, const float* __restrict__ run,
                                                           float* __restrict__ cand_val, int* __restrict__ cand_idx, int compact,
                                                           const int32_t* __restrict__ seqs_in, int L, int ngram, int groups, BeamCons cn) {
    __shared__ float smf[4];
    __shared__ float s_val[4];
    __shared__ int s_idx[4], s_who[4];
    __shared__ int s_ban[256 + BEAM_CONS_SLOTS], s_nban, s_cw[BEAM_CONS_SLOTS];
    const int row = blockIdx.x, img = row / k, r = row % k, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int na = CONS ? beam_row_cands_states(n_act, cn, img, r) : beam_row_cands<GROUPED>(n_act, img, r, k, groups, step);     // candidates of this row (0: not scored)
    if (na == 0) return;
    int nban = 0, nban_ngram = 0;          // entries of the list; those of them that are n-gram bans (the first ones)
    if (CONS) {
        beam_cons_words(cn, img, s_cw);
        if (ngram && step >= ngram) nban_ngram = beam_ban_list(seqs_in + (size_t)row * L, step, ngram, s_ban, &s_nban);
        else { if (tid == 0) s_nban = 0; __syncthreads(); }
        if (tid < BEAM_CONS_SLOTS && s_cw[tid] >= 0) s_ban[atomicAdd(&s_nban, 1)] = s_cw[tid];
        __syncthreads();
        nban = s_nban;
    } else if (BAN) {
        nban = beam_ban_list(seqs_in + (size_t)row * L, step, ngram, s_ban, &s_nban);
    }
    const float* l = logits + (size_t)(compact ? img : row) * ldl;      // compact (step 1 only): one decoder row per image
    // Every sweep fetches the thread's strided slice (40 logits at V = 10102) in batches of U independent loads: one memory
    // latency per batch instead of one per element.  (All 40 in registers across the three sweeps: the unrolled kernel
    // outgrows the instruction cache; the row staged in LDS for the second and third sweep: no faster, 36 -> 37 us.)
    constexpr int U = 8;
    auto slice = [&](int v0, float (&x)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) { const int v = v0 + 256 * u; x[u] = v < V ? l[v] : -INFINITY; }
    };
    float mx = -INFINITY;
    for (int v0 = tid; v0 < V; v0 += 256 * U) {
        float x[U];
        slice(v0, x);
#pragma unroll
        for (int u = 0; u < U; ++u) mx = fmaxf(mx, x[u]);
    }
    mx = block_max_256(mx, smf);
    float se = 0.f;
    for (int v0 = tid; v0 < V; v0 += 256 * U) {
        float x[U];
        slice(v0, x);
#pragma unroll
        for (int u = 0; u < U; ++u) if (v0 + 256 * u < V) se += expf(x[u] - mx);
    }
    se = block_sum_256(se, smf);
    const float ls = logf(se);
    const float rs = (step == 1) ? 0.f : run[row];
    if (CONS && tid < BEAM_CONS_SLOTS) {
        const int w = s_cw[tid];
        const bool ok = w >= 0 && w < V && !beam_banned(w, s_ban, nban_ngram);
        cn.force_val[(size_t)row * BEAM_CONS_SLOTS + tid] = ok ? rs + ((l[w] - mx) - ls) : -INFINITY;
    }
    // thread-local best `na` of its strided slice (sorted: value descending, index ascending on ties)
    float tv[BEAM_MAX_K];
    int ti[BEAM_MAX_K];
#pragma unroll
    for (int j = 0; j < BEAM_MAX_K; ++j) { tv[j] = -INFINITY; ti[j] = 0x7fffffff; }
    // The list is sorted, so an element enters it only if it beats the last kept entry (position na - 1): nearly all of a
    // thread's ~40 elements fail that one test and skip the insertion chain.
    float worst = -INFINITY;
    int worst_i = 0x7fffffff;
    for (int v0 = tid; v0 < V; v0 += 256 * U) {
        float x[U];
        slice(v0, x);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (v0 + 256 * u >= V) continue;
            float val = rs + ((x[u] - mx) - ls);
            int idx = v0 + 256 * u;
            if (!(val > worst || (val == worst && idx < worst_i))) continue;
            if (BAN && nban && beam_banned(idx, s_ban, nban)) continue;
#pragma unroll
            for (int j = 0; j < BEAM_MAX_K; ++j) {          // branch-free insertion: swap down the list
                const bool take = (j < na) & ((val > tv[j]) | ((val == tv[j]) & (idx < ti[j])));
                const float ov = tv[j]; const int oi = ti[j];
                tv[j] = take ? val : ov; ti[j] = take ? idx : oi;
                val = take ? ov : val; idx = take ? oi : idx;
            }
#pragma unroll
            for (int j = 0; j < BEAM_MAX_K; ++j) {
                worst = (j == na - 1) ? tv[j] : worst;
                worst_i = (j == na - 1) ? ti[j] : worst_i;
            }
        }
    }
    // na rounds: every thread offers the head of its list, the block takes the best and that thread pops it
    int head = 0;
    for (int j = 0; j < na; ++j) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < BEAM_MAX_K; ++q)
            if (q == head) { best = tv[q]; bi = ti[q]; }
        int who = tid;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64), ow = __shfl_xor(who, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; who = ow; }
        }
        if (lane == 0) { s_val[wave] = best; s_idx[wave] = bi; s_who[wave] = who; }
        __syncthreads();
        best = s_val[0]; bi = s_idx[0]; who = s_who[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (s_val[w] > best || (s_val[w] == best && s_idx[w] < bi)) { best = s_val[w]; bi = s_idx[w]; who = s_who[w]; }
        if (tid == who) ++head;
        if (tid == 0) { cand_val[row * BEAM_MAX_K + j] = best; cand_idx[row * BEAM_MAX_K + j] = bi; }
        __syncthreads();
    }
}

// The same result from a row held in registers (16-byte loads, one pass over memory) and a threshold instead of per-thread
// sorted lists.  The sorted insertion above is VALU-bound: a wave skips an element only when none of its 64 lanes inserts it,
// so nearly all of the 40 x 8-deep insertion chains execute (36 us per step at 640 rows).  Here every thread takes the maximum
// of its 4 NV4 candidate scores; tau = the n-th largest of the 256 thread maxima (n = active beams; equal maxima of different
// threads count separately).  At least n scores are >= tau, so every member of the row's top n is: the threads append their
// scores >= tau to an LDS list (a handful unless the row is full of ties) and one wave picks the top n of the list by
// (score descending, index ascending) -- the order of a top-k over the flattened scores.  A list that overflows (massive ties,
// e.g. constant logits) sends the workgroup through the insertion algorithm on the LDS-staged scores instead.
// Needs V <= 1024 NV4, 16-byte aligned rows (ldl % 4 == 0).  The log-sum-exp is summed in a different element order than in
// the kernel above (thread t holds elements 4 (t + 256 u) + j): scores may differ in the last bit.
// Blocking: the thread that owns a banned token sets its score to -inf before its maximum is taken (a fully unrolled select:
// no dynamic register index), so tau, the candidate list and the overflow path never see it.  The ban list lives at the
// start of the overflow path's LDS row, which is written only after the list has been read.
// CONS (a constrained search): behind the n-gram bans the thread that owns a constraint word of the image writes its score to
// force_val [rows, 12] (slot c * 4 + a; an n-gram-banned word is -inf by then, an empty slot is written as -inf) and sets it to
// -inf in its registers, the same unrolled select: tau, the list and the overflow path see the other tokens only.
constexpr int BEAM_CAND_CAP = 128;
template <int NV4, bool GROUPED, bool CONS = false>
__global__ __launch_bounds__(256) void beam_rowtopk_reg_kernel(const float* __restrict__ logits, int V, int ldl, int k, int step,
                                                               const int* __restrict__ n_act, const float* __restrict__ run,
                                                               float* __restrict__ cand_val, int* __restrict__ cand_idx, int compact,
                                                               const int32_t* __restrict__ seqs_in, int L, int ngram, int groups, BeamCons cn) {
    __shared__ float smf[4];
    __shared__ float s_val[4];
    __shared__ int s_idx[4], s_who[4];
    __shared__ int s_cnt, s_taken, s_nban, s_cw[BEAM_CONS_SLOTS];
    __shared__ float s_cv[BEAM_CAND_CAP];
    __shared__ int s_ci[BEAM_CAND_CAP];
    extern __shared__ __attribute__((aligned(16))) float s_row[];          // overflow path only: 1024 NV4 floats
    const int row = blockIdx.x, img = row / k, r = row % k, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int na = CONS ? beam_row_cands_states(n_act, cn, img, r) : beam_row_cands<GROUPED>(n_act, img, r, k, groups, step);     // candidates of this row (0: not scored)
    if (na == 0) return;
    if (CONS) beam_cons_words(cn, img, s_cw);      // read behind the barriers of the block reductions below
    const float* l = logits + (size_t)(compact ? img : row) * ldl;      // compact (step 1 only): one decoder row per image
    f32x4 x[NV4];
#pragma unroll
    for (int u = 0; u < NV4; ++u) {
        const int v = 4 * (tid + 256 * u);
        x[u] = v < V ? *reinterpret_cast<const f32x4*>(l + v) : (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int j = 0; j < 4; ++j) if (v + j >= V) x[u][j] = -INFINITY;
    }
    if (tid == 0) { s_cnt = 0; s_taken = 0; }
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < NV4; ++u) mx = fmaxf(mx, fmaxf(fmaxf(x[u][0], x[u][1]), fmaxf(x[u][2], x[u][3])));
    mx = block_max_256(mx, smf);
    float se = 0.f;
#pragma unroll
    for (int u = 0; u < NV4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) se += expf(x[u][j] - mx);          // exp(-inf) = 0 for the slots beyond V
    se = block_sum_256(se, smf);
    const float ls = logf(se);
    const float rs = (step == 1) ? 0.f : run[row];
#pragma unroll
    for (int u = 0; u < NV4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) x[u][j] = rs + ((x[u][j] - mx) - ls);      // the candidate score (beyond V: -inf)
    if (ngram && step >= ngram) {
        int* s_ban = reinterpret_cast<int*>(s_row);
        const int nban = beam_ban_list(seqs_in + (size_t)row * L, step, ngram, s_ban, &s_nban);
        for (int b = 0; b < nban; ++b) {
            const int q = s_ban[b] >> 2, bu = q >> 8, bj = s_ban[b] & 3;
            if ((q & 255) != tid) continue;
#pragma unroll
            for (int u = 0; u < NV4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) x[u][j] = (u == bu && j == bj) ? -INFINITY : x[u][j];
        }
    }
    if (CONS) {
        for (int q = 0; q < BEAM_CONS_SLOTS; ++q) {
            const int w = s_cw[q];
            float* fv = cn.force_val + (size_t)row * BEAM_CONS_SLOTS + q;
            if (w < 0 || w >= V) { if (tid == 0) *fv = -INFINITY; continue; }
            const int e = w >> 2, bu = e >> 8, bj = w & 3;
            if ((e & 255) != tid) continue;
            float got = -INFINITY;
#pragma unroll
            for (int u = 0; u < NV4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool hit = u == bu && j == bj;
                    got = hit ? x[u][j] : got;
                    x[u][j] = hit ? -INFINITY : x[u][j];
                }
            *fv = got;
        }
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int u = 0; u < NV4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) tmax = fmaxf(tmax, x[u][j]);
    // tau: rounds of block maximum over the thread maxima not yet counted, until na of them are
    float tau = -INFINITY;
    {
        float cur = tmax;
        for (int round = 0; round < BEAM_MAX_K; ++round) {
            const float m = block_max_256(cur, smf);
            const bool hit = cur == m && m > -INFINITY;
            const unsigned long long b = __ballot(hit);
            if (lane == 0 && b) atomicAdd(&s_taken, __popcll(b));
            if (hit) cur = -INFINITY;
            __syncthreads();
            tau = m;
            const int taken = s_taken;
            __syncthreads();
            if (taken >= na || m == -INFINITY) break;
        }
    }
#pragma unroll
    for (int u = 0; u < NV4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x[u][j] >= tau && x[u][j] > -INFINITY) {
                const int pos = atomicAdd(&s_cnt, 1);
                if (pos < BEAM_CAND_CAP) { s_cv[pos] = x[u][j]; s_ci[pos] = 4 * (tid + 256 * u) + j; }
            }
    __syncthreads();
    const int cnt = s_cnt;
    if (cnt <= BEAM_CAND_CAP) {
        if (wave != 0) return;
        float v0 = lane < cnt ? s_cv[lane] : -INFINITY, v1 = lane + 64 < cnt ? s_cv[lane + 64] : -INFINITY;
        int i0 = lane < cnt ? s_ci[lane] : 0x7fffffff, i1 = lane + 64 < cnt ? s_ci[lane + 64] : 0x7fffffff;
        for (int j = 0; j < na; ++j) {
            float best = v0;
            int bi = i0;
            if (v1 > best || (v1 == best && i1 < bi)) { best = v1; bi = i1; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (i0 == bi) { v0 = -INFINITY; i0 = 0x7fffffff; }      // taken (indices are unique)
            if (i1 == bi) { v1 = -INFINITY; i1 = 0x7fffffff; }
            if (lane == 0) { cand_val[row * BEAM_MAX_K + j] = best; cand_idx[row * BEAM_MAX_K + j] = bi; }
        }
        return;
    }
    // ---- overflow: the insertion algorithm of beam_rowtopk_kernel on the scores, staged in LDS in index order
#pragma unroll
    for (int u = 0; u < NV4; ++u) *reinterpret_cast<f32x4*>(s_row + 4 * (tid + 256 * u)) = x[u];
    __syncthreads();
    float tv[BEAM_MAX_K];
    int ti[BEAM_MAX_K];
#pragma unroll
    for (int j = 0; j < BEAM_MAX_K; ++j) { tv[j] = -INFINITY; ti[j] = 0x7fffffff; }
    float worst = -INFINITY;
    int worst_i = 0x7fffffff;
    for (int v = tid; v < V; v += 256) {
        float val = s_row[v];
        int idx = v;
        if (!(val > worst || (val == worst && idx < worst_i))) continue;
#pragma unroll
        for (int j = 0; j < BEAM_MAX_K; ++j) {
            const bool take = (j < na) & ((val > tv[j]) | ((val == tv[j]) & (idx < ti[j])));
            const float ov = tv[j]; const int oi = ti[j];
            tv[j] = take ? val : ov; ti[j] = take ? idx : oi;
            val = take ? ov : val; idx = take ? oi : idx;
        }
#pragma unroll
        for (int j = 0; j < BEAM_MAX_K; ++j) {
            worst = (j == na - 1) ? tv[j] : worst;
            worst_i = (j == na - 1) ? ti[j] : worst_i;
        }
    }
    int head = 0;
    for (int j = 0; j < na; ++j) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < BEAM_MAX_K; ++q)
            if (q == head) { best = tv[q]; bi = ti[q]; }
        int who = tid;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64), ow = __shfl_xor(who, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; who = ow; }
        }
        if (lane == 0) { s_val[wave] = best; s_idx[wave] = bi; s_who[wave] = who; }
        __syncthreads();
        best = s_val[0]; bi = s_idx[0]; who = s_who[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (s_val[w] > best || (s_val[w] == best && s_idx[w] < bi)) { best = s_val[w]; bi = s_idx[w]; who = s_who[w]; }
        if (tid == who) ++head;
        if (tid == 0) { cand_val[row * BEAM_MAX_K + j] = best; cand_idx[row * BEAM_MAX_K + j] = bi; }
        __syncthreads();
    }
}

// per-row candidates of one beam step: the register kernel where the vocabulary fits it, else the sweep kernel
// (ngram > 0: n-gram blocking on the prefixes seqs_in [rows, L]; groups > 1: the grouped instances, n_act [n_img, groups])
// The one owner of that choice (icz_beam_rowtopk_route_for is its host entry): the register kernels move 16 bytes at a time, so
// they need rows that start on 16 bytes (aligned base, ldl % 4 == 0) and a vocabulary of at most 1024 NV4 tokens.
enum { BEAM_ROUTE_AUTO = 0, BEAM_ROUTE_REG3 = 1, BEAM_ROUTE_REG10 = 2, BEAM_ROUTE_SWEEP = 3 };
inline int beam_rowtopk_route(int V, int ldl, bool base_aligned) {
    const bool ok = ldl % 4 == 0 && base_aligned;
    return ok && V <= 1024 * 3 ? BEAM_ROUTE_REG3 : ok && V <= 1024 * 10 ? BEAM_ROUTE_REG10 : BEAM_ROUTE_SWEEP;
}
inline bool beam_rowtopk_route_fits(int route, int V, int ldl, bool base_aligned) {      // whether a forced route can take the shape
    if (route == BEAM_ROUTE_REG3 || route == BEAM_ROUTE_REG10)
        return ldl % 4 == 0 && ldl >= ((V + 3) & ~3) && base_aligned && V <= 1024 * (route == BEAM_ROUTE_REG3 ? 3 : 10);
    return route == BEAM_ROUTE_AUTO || route == BEAM_ROUTE_SWEEP;
}
// route: BEAM_ROUTE_AUTO (every search) or a kernel forced by icz_test_beam_rowtopk / icz_test_beam_step, which check that it fits
template <bool GROUPED>
inline void launch_beam_rowtopk_t(hipStream_t st, int rows, const float* logits, int V, int ldl, int k, int step, const int* n_act,
                                  const float* run, float* cand_val, int* cand_idx, int compact, const int32_t* seqs_in, int L,
                                  int ngram, int groups, int route) {
    const int r = route != BEAM_ROUTE_AUTO ? route : beam_rowtopk_route(V, ldl, ((uintptr_t)logits & 15) == 0);
    const BeamCons cn = {};
    if (r == BEAM_ROUTE_REG3) hipLaunchKernelGGL((beam_rowtopk_reg_kernel<3, GROUPED>), dim3(rows), dim3(256), sizeof(float) * 1024 * 3, st, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, groups, cn);
    else if (r == BEAM_ROUTE_REG10) hipLaunchKernelGGL((beam_rowtopk_reg_kernel<10, GROUPED>), dim3(rows), dim3(256), sizeof(float) * 1024 * 10, st, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, groups, cn);
    else if (ngram && step >= ngram) hipLaunchKernelGGL((beam_rowtopk_kernel<true, GROUPED>), dim3(rows), dim3(256), 0, st, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, groups, cn);
    else hipLaunchKernelGGL((beam_rowtopk_kernel<false, GROUPED>), dim3(rows), dim3(256), 0, st, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, groups, cn);
}
inline void launch_beam_rowtopk(hipStream_t st, int rows, const float* logits, int V, int ldl, int k, int step, const int* n_act,
                                const float* run, float* cand_val, int* cand_idx, int compact = 0, const int32_t* seqs_in = nullptr,
                                int L = 0, int ngram = 0, int groups = 1, int route = BEAM_ROUTE_AUTO) {
    if (groups > 1) launch_beam_rowtopk_t<true>(st, rows, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, groups, route);
    else launch_beam_rowtopk_t<false>(st, rows, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, 1, route);
}
// the constrained instances of the same three routes (k = 2^C * beam rows per image, n_act / cn.cap [n_img, 2^C])
inline void launch_beam_rowtopk_cons(hipStream_t st, int rows, const float* logits, int V, int ldl, int k, int step, const int* n_act,
                                     const float* run, float* cand_val, int* cand_idx, int compact, const int32_t* seqs_in, int L, int ngram,
                                     int route, const BeamCons& cn) {
    const int r = route != BEAM_ROUTE_AUTO ? route : beam_rowtopk_route(V, ldl, ((uintptr_t)logits & 15) == 0);
    if (r == BEAM_ROUTE_REG3) hipLaunchKernelGGL((beam_rowtopk_reg_kernel<3, false, true>), dim3(rows), dim3(256), sizeof(float) * 1024 * 3, st, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, 1, cn);
    else if (r == BEAM_ROUTE_REG10) hipLaunchKernelGGL((beam_rowtopk_reg_kernel<10, false, true>), dim3(rows), dim3(256), sizeof(float) * 1024 * 10, st, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, 1, cn);
    else hipLaunchKernelGGL((beam_rowtopk_kernel<true, false, true>), dim3(rows), dim3(256), 0, st, logits, V, ldl, k, step, n_act, run, cand_val, cand_idx, compact, seqs_in, L, ngram, 1, cn);
}

__global__ __launch_bounds__(64) void beam_merge_kernel(BeamArgs a, const float* __restrict__ cand_val, const int* __restrict__ cand_idx) {
    __shared__ float pick_val[BEAM_MAX_K];
    __shared__ int pick_idx[BEAM_MAX_K];
    __shared__ int new_src[BEAM_MAX_K], new_tok[BEAM_MAX_K], s_newn;
    __shared__ float new_run[BEAM_MAX_K];
    const int img = blockIdx.x, lane = threadIdx.x;
    const int k = a.k, V = a.V;
    const int na = a.n_act[img];
    const int row0 = img * k;
    if (na == 0) {
        for (int j = lane; j < k; j += 64) { a.src_row[row0 + j] = row0 + j; a.it_next[row0 + j] = 0; }
        return;
    }
    const int nr = (a.step == 1) ? 1 : na;
    // lane c <-> candidate (row r = c / BEAM_MAX_K, rank j = c % BEAM_MAX_K)
    const int cr = lane / BEAM_MAX_K, cj = lane % BEAM_MAX_K;
    float val = -INFINITY;
    int idx = 0x7fffffff;
    if (cr < nr && cj < na) {
        const int ci = cand_idx[(row0 + cr) * BEAM_MAX_K + cj];
        if (ci < V) {          // a row with fewer than na admissible tokens (every other one banned) leaves empty slots
            val = cand_val[(row0 + cr) * BEAM_MAX_K + cj];
            idx = cr * V + ci;
        }
    }
    for (int j = 0; j < na; ++j) {
        float best = val;
        int bi = idx;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (idx == bi) { val = -INFINITY; idx = 0x7fffffff; }      // taken (flat indices are unique)
        if (lane == 0) { pick_val[j] = best; pick_idx[j] = bi; }
    }
    __syncthreads();
    // retire finished beams, compact the rest (:279-300)
    if (lane == 0) {
        int nn = 0;
        for (int j = 0; j < na; ++j) {
            if (pick_idx[j] == 0x7fffffff) continue;       // no admissible candidate left for this beam: it ends unfinished and unlisted
            const int src = pick_idx[j] / V, tok = pick_idx[j] % V;
            if (tok == 2) {
                const int32_t* ss = a.seqs_in + (size_t)(row0 + src) * a.L;
                if (!a.has_complete[img] || pick_val[j] > a.best_score[img]) {
                    a.has_complete[img] = 1;
                    a.best_score[img] = pick_val[j];
                    a.best_len[img] = a.step + 1;
                    int32_t* bs = a.best_seq + (size_t)img * a.L;
                    for (int i = 0; i < a.step; ++i) bs[i] = ss[i];
                    bs[a.step] = 2;
                }
                if (a.hyp_cnt && a.hyp_cnt[img] < k) {      // the n-best list: every retirement, in order
                    const int slot = row0 + a.hyp_cnt[img]++;
                    a.hyp_score[slot] = pick_val[j];
                    a.hyp_len[slot] = a.step + 1;
                    int32_t* hs = a.hyp_seq + (size_t)slot * a.L;
                    for (int i = 0; i < a.step; ++i) hs[i] = ss[i];
                    hs[a.step] = 2;
                }
            } else {
                new_src[nn] = src; new_tok[nn] = tok; new_run[nn] = pick_val[j];
                ++nn;
            }
        }
        s_newn = nn;
        a.n_act[img] = nn;
        if (nn > 0) atomicAdd(a.n_live, 1);
    }
    __syncthreads();
    const int nn = s_newn;
    for (int j = 0; j < k; ++j) {
        if (j < nn) {
            const int32_t* ss = a.seqs_in + (size_t)(row0 + new_src[j]) * a.L;
            int32_t* so = a.seqs_out + (size_t)(row0 + j) * a.L;
            for (int i = lane; i < a.step; i += 64) so[i] = ss[i];
            if (lane == 0) {
                so[a.step] = new_tok[j];
                a.run[row0 + j] = new_run[j];
                a.src_row[row0 + j] = row0 + new_src[j];
                a.it_next[row0 + j] = new_tok[j];
            }
        } else if (lane == 0) {
            a.src_row[row0 + j] = row0 + j;
            a.it_next[row0 + j] = 0;
        }
    }
}

// key of a diverse-search candidate: score - fp32(lambda * c), the product rounded on its own.  The build contracts by default,
// which would fuse the two into one fma (one rounding) and move the key off the spec by an ulp whenever lambda * c is inexact.
__device__ inline float beam_diverse_key(float score, float lambda, int c) {
#pragma clang fp contract(off)
    const float pen = lambda * (float)c;
    return score - pen;
}

// Diverse beam search (Vijayakumar et al., "Diverse Beam Search", AAAI 2018), one wave per image: the k rows of the image form
// `groups` groups of kg = k / groups beams (group-major rows, n_act [n_img, groups]).  The groups select in order; group g ranks
// its candidates by key = score - fp32(lambda * c), c = how often groups 0 .. g-1 picked the token at this step (an LDS table of
// at most k entries), with the tie rule of beam_merge_kernel over its own rows (flat index r * V + v), and keeps the raw score.
// Every pick counts, <end> included.  Retirements go to the n-best list in order (step, group, merge rank); each group's
// survivors are compacted into the group's own slots.  Step 1: every group reads the k candidates of the image's row 0.
__global__ __launch_bounds__(64) void beam_merge_groups_kernel(BeamArgs a, int groups, float lambda, const float* __restrict__ cand_val,
                                                               const int* __restrict__ cand_idx) {
    __shared__ float pick_val[BEAM_MAX_K];
    __shared__ int pick_idx[BEAM_MAX_K];
    __shared__ int new_src[BEAM_MAX_K], new_tok[BEAM_MAX_K], s_newn;
    __shared__ float new_run[BEAM_MAX_K];
    __shared__ int s_na[BEAM_MAX_K];                             // live beams per group when the step began
    __shared__ int cnt_tok[BEAM_MAX_K], cnt_n[BEAM_MAX_K], s_ncnt;
    const int img = blockIdx.x, lane = threadIdx.x;
    const int k = a.k, V = a.V, kg = k / groups, row0 = img * k;
    if (lane < groups) s_na[lane] = a.n_act[img * groups + lane];
    if (lane == 0) s_ncnt = 0;
    __syncthreads();
    // lane c <-> candidate (row r = c / BEAM_MAX_K of the group, rank j = c % BEAM_MAX_K): kg x k <= 64
    const int cr = lane / BEAM_MAX_K, cj = lane % BEAM_MAX_K;
    int csum = 0, live = 0;
    for (int g = 0; g < groups; ++g) {                           // uniform: s_na, s_ncnt and s_newn are read after a barrier
        const int na = s_na[g], gr0 = row0 + g * kg;
        csum += na;
        if (na == 0) {
            for (int j = lane; j < kg; j += 64) { a.src_row[gr0 + j] = gr0 + j; a.it_next[gr0 + j] = 0; }
            continue;
        }
        const int nr = (a.step == 1) ? 1 : na, nc = (a.step == 1) ? k : min(k, csum);     // beam_row_cands<true>
        float key = -INFINITY, val = -INFINITY;
        int idx = 0x7fffffff;
        if (cr < nr && cj < nc) {
            const int crow = (a.step == 1) ? row0 : gr0 + cr;
            const int ci = cand_idx[crow * BEAM_MAX_K + cj];
            if (ci < V) {
                val = cand_val[crow * BEAM_MAX_K + cj];
                int c = 0;
                for (int q = 0; q < s_ncnt; ++q) c += cnt_tok[q] == ci ? cnt_n[q] : 0;
                key = beam_diverse_key(val, lambda, c);
                idx = cr * V + ci;
            }
        }
        for (int j = 0; j < na; ++j) {
            float best = key, bv = val;
            int bi = idx;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o, 64), ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; bv = ov; }
            }
            if (idx == bi) { key = -INFINITY; idx = 0x7fffffff; }      // taken (flat indices are unique)
            if (lane == 0) { pick_val[j] = bv; pick_idx[j] = bi; }
        }
        __syncthreads();
        if (lane == 0) {
            int nn = 0, nt = s_ncnt;
            for (int j = 0; j < na; ++j) {
                if (pick_idx[j] == 0x7fffffff) continue;       // no admissible candidate left for this beam: it ends unfinished and unlisted
                const int src = pick_idx[j] / V, tok = pick_idx[j] % V;
                int q = 0;
                while (q < nt && cnt_tok[q] != tok) ++q;
                if (q == nt) { cnt_tok[q] = tok; cnt_n[q] = 0; ++nt; }
                ++cnt_n[q];
                if (tok == 2) {
                    if (a.hyp_cnt[img] < k) {
                        const int32_t* ss = a.seqs_in + (size_t)(gr0 + src) * a.L;
                        const int slot = row0 + a.hyp_cnt[img]++;
                        a.hyp_score[slot] = pick_val[j];
                        a.hyp_len[slot] = a.step + 1;
                        int32_t* hs = a.hyp_seq + (size_t)slot * a.L;
                        for (int i = 0; i < a.step; ++i) hs[i] = ss[i];
                        hs[a.step] = 2;
                    }
                } else {
                    new_src[nn] = src; new_tok[nn] = tok; new_run[nn] = pick_val[j];
                    ++nn;
                }
            }
            s_ncnt = nt;
            s_newn = nn;
            a.n_act[img * groups + g] = nn;
            live += nn;
        }
        __syncthreads();
        const int nn = s_newn;
        for (int j = 0; j < kg; ++j) {
            if (j < nn) {
                const int32_t* ss = a.seqs_in + (size_t)(gr0 + new_src[j]) * a.L;
                int32_t* so = a.seqs_out + (size_t)(gr0 + j) * a.L;
                for (int i = lane; i < a.step; i += 64) so[i] = ss[i];
                if (lane == 0) {
                    so[a.step] = new_tok[j];
                    a.run[gr0 + j] = new_run[j];
                    a.src_row[gr0 + j] = gr0 + new_src[j];
                    a.it_next[gr0 + j] = new_tok[j];
                }
            } else if (lane == 0) {
                a.src_row[gr0 + j] = gr0 + j;
                a.it_next[gr0 + j] = 0;
            }
        }
        __syncthreads();                                         // the next group overwrites pick_* / new_*
    }
    if (lane == 0 && live > 0) atomicAdd(a.n_live, 1);
}

// final selection (:302-313): best finished hypothesis if any, else the best-scoring live beam (scores: its raw score, if non-null)
__global__ void beam_finalize_kernel(int k, int L, int steps_done, const int* __restrict__ n_act, const float* __restrict__ run,
                                     const int32_t* __restrict__ seqs, const int* __restrict__ has_complete,
                                     const int* __restrict__ best_len, const int32_t* __restrict__ best_seq,
                                     float* __restrict__ out, int32_t* __restrict__ lens, const float* __restrict__ best_score = nullptr,
                                     float* __restrict__ scores = nullptr) {
    const int img = blockIdx.x;
    const int32_t* src;
    int len;
    float sc;
    if (has_complete[img]) {
        src = best_seq + (size_t)img * L;
        len = best_len[img];
        sc = scores ? best_score[img] : 0.f;
    } else {
        int bi = 0;
        float bv = -INFINITY;
        for (int j = 0; j < n_act[img]; ++j)
            if (run[img * k + j] > bv) { bv = run[img * k + j]; bi = j; }
        src = seqs + (size_t)(img * k + bi) * L;
        len = steps_done + 1;
        sc = bv;
    }
    for (int i = threadIdx.x; i < L; i += blockDim.x) out[(size_t)img * L + i] = i < len ? (float)src[i] : 0.f;
    if (threadIdx.x == 0) {
        lens[img] = len;
        if (scores) scores[img] = sc;
    }
}

// length penalty of the final ranking (tokens = generated tokens, <end> counted): 1 avg: s / tokens^a, 2 wu: s / ((5 + tokens) / 6)^a
__device__ inline float beam_lp_norm(float s, int tokens, int kind, float alpha) {
    if (kind == 1) return s / powf((float)tokens, alpha);
    if (kind == 2) return s / powf((5.f + (float)tokens) / 6.f, alpha);
    return s;
}

// n-best selection, one wave per image: the image's k hypotheses are its retirements (hyp_*, in retirement order) and the beams
// still live when the step limit ran out (rows 0 .. n_act - 1 of `seqs`, in merge order; grouped: group by group).  Ranked: finished before live, then by
// the length-normalised score (descending), then by that order.  Writes the first n_best: ids out [n_img, n_best, L] (float32,
// zero-padded), lens [n_img, n_best], raw scores [n_img, n_best]; a rank past the image's hypotheses (only when every token of
// some beam was banned) is written as length 0, score -inf.
// GROUPED (diverse search, n_act [n_img, groups]): the live beams are enumerated in (group, slot) order.
template <bool GROUPED>
__device__ inline int beam_live_total(const int* __restrict__ n_act, int img, int groups) {
    if (!GROUPED) return n_act[img];
    int t = 0;
    for (int g = 0; g < groups; ++g) t += n_act[img * groups + g];
    return t;
}
template <bool GROUPED>
__device__ inline int beam_live_row(const int* __restrict__ n_act, int img, int k, int groups, int q) {     // row of live beam q
    if (!GROUPED) return img * k + q;
    const int kg = k / groups;
    for (int g = 0; g < groups; ++g) {
        const int na = n_act[img * groups + g];
        if (q < na) return img * k + g * kg + q;
        q -= na;
    }
    return img * k;      // q < beam_live_total: not reached
}
template <bool GROUPED>
__global__ __launch_bounds__(64) void beam_finalize_nbest_kernel(int k, int L, int steps_done, int n_best, int lp_kind, float lp_alpha,
                                                                 const int* __restrict__ n_act, const float* __restrict__ run,
                                                                 const int32_t* __restrict__ seqs, const int* __restrict__ hyp_cnt,
                                                                 const float* __restrict__ hyp_score, const int* __restrict__ hyp_len,
                                                                 const int32_t* __restrict__ hyp_seq, float* __restrict__ out,
                                                                 int32_t* __restrict__ lens, float* __restrict__ scores, int groups) {
    __shared__ int s_pick[BEAM_MAX_K];
    const int img = blockIdx.x, lane = threadIdx.x, row0 = img * k;
    const int nf = hyp_cnt[img], tot = min(nf + beam_live_total<GROUPED>(n_act, img, groups), k);
    const bool fin = lane < nf;
    float raw = -INFINITY;
    int len = 1;
    if (lane < tot) {
        raw = fin ? hyp_score[row0 + lane] : run[beam_live_row<GROUPED>(n_act, img, k, groups, lane - nf)];
        len = fin ? hyp_len[row0 + lane] : steps_done + 1;
    }
    const float ns = beam_lp_norm(raw, len - 1, lp_kind, lp_alpha);
    int rank = 0;
    for (int f = 0; f < tot; ++f) {
        const float nf_s = __shfl(ns, f, 64);
        const bool f_fin = f < nf;
        rank += (f_fin && !fin) || (f_fin == fin && (nf_s > ns || (nf_s == ns && f < lane)));
    }
    if (lane < BEAM_MAX_K) s_pick[lane] = -1;
    __syncthreads();
    if (lane < tot) s_pick[rank] = lane;
    __syncthreads();
    for (int m = 0; m < n_best; ++m) {
        const int e = s_pick[m], o = img * n_best + m;
        const int lr = e < nf ? 0 : beam_live_row<GROUPED>(n_act, img, k, groups, e - nf);
        const int32_t* src = e < 0 ? nullptr : e < nf ? hyp_seq + (size_t)(row0 + e) * L : seqs + (size_t)lr * L;
        const int ln = e < 0 ? 0 : e < nf ? hyp_len[row0 + e] : steps_done + 1;
        for (int i = lane; i < L; i += 64) out[(size_t)o * L + i] = i < ln ? (float)src[i] : 0.f;
        if (lane == 0) {
            lens[o] = ln;
            scores[o] = e < 0 ? -INFINITY : e < nf ? hyp_score[row0 + e] : run[lr];
        }
    }
}

__global__ void beam_init_kernel(int n_img, int k, int L, int* n_act, int32_t* seqs, int32_t* img_of_row, int64_t* it,
                                 int* has_complete, float* best_score, int* hyp_cnt) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_img * k) return;
    seqs[(size_t)row * L] = 1;      // <sta>
    img_of_row[row] = row / k;
    it[row] = 1;
    if (row % k == 0) {
        const int img = row / k;
        n_act[img] = k;
        has_complete[img] = 0;
        best_score[img] = -INFINITY;
        hyp_cnt[img] = 0;
    }
}

// grouped search: n_act [n_img, groups] = kg, after beam_init_kernel (which wrote n_act [n_img] = k)
__global__ void beam_init_groups_kernel(int n, int kg, int* n_act) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) n_act[i] = kg;
}

// ---- constrained beam search (Anderson et al., "Guided Open Vocabulary Image Captioning with Constrained Beam Search", EMNLP 2017) ----
// The k = S * beam rows of an image are S = 2^C states of `beam` slots (state-major); a hypothesis's state is the bit mask of the
// constraints it has satisfied.  Every state runs the search of beam_merge_kernel on its own capacity cap[s] (beam minus its <end>
// retirements) and live count n_act[s] <= cap[s]; a candidate (row of state s, token v) belongs to target state s | bit(v).

// constrained search: n_act [n_img, S] = 1 for state 0 (the hypothesis [<sta>]) and 0 elsewhere, cap [n_img, S] = beam, after
// beam_init_kernel (which wrote n_act [n_img] = k)
__global__ void beam_init_states_kernel(int n, int S, int beam, int* n_act, int* cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { n_act[i] = (i % S) == 0 ? 1 : 0; cap[i] = beam; }
}

// The per-image merge of a constrained step, one wave per image.  The targets select in ascending order.  The candidates of target t
// sit at fixed LDS positions (no atomics): 64 ordinary slots -- candidate cj of live row cr of t's own rows, the row's top cap[t]
// over the tokens that are no constraint word of the image -- and k * 12 forced slots -- force_val[row, q] of every live row of a
// state s with s | bit(word q) == t, which covers every move between states and every re-use of a satisfied word.  t takes its
// best cap[t] finite candidates, ties to the lower flat index (s * beam + j) * V + v (beam_merge_kernel's rule over the image's k
// rows); an <end> pick retires into the image's list with its state and lowers cap[t], every other pick is compacted into t's slots
// in pick order.  n_act and cap are read once when the step begins: a target's sources are states s <= t, rewritten by then.
constexpr int BEAM_STATES_CAND = BEAM_MAX_K * BEAM_MAX_K + BEAM_CONS_MAX_ROWS * BEAM_CONS_SLOTS;
__global__ __launch_bounds__(64) void beam_merge_states_kernel(BeamArgs a, BeamCons cn, const float* __restrict__ cand_val,
                                                               const int* __restrict__ cand_idx) {
    __shared__ float s_cv[BEAM_STATES_CAND];
    __shared__ int s_cf[BEAM_STATES_CAND];
    __shared__ float pick_val[BEAM_MAX_K];
    __shared__ int pick_idx[BEAM_MAX_K];
    __shared__ int new_src[BEAM_MAX_K], new_tok[BEAM_MAX_K], s_newn;
    __shared__ float new_run[BEAM_MAX_K];
    __shared__ int s_na[1 << BEAM_CONS_MAX_C], s_cap[1 << BEAM_CONS_MAX_C], s_cw[BEAM_CONS_SLOTS];
    const int img = blockIdx.x, lane = threadIdx.x;
    const int k = a.k, V = a.V, beam = cn.beam, S = 1 << cn.C, row0 = img * k;
    if (lane < S) {
        s_na[lane] = min(max(a.n_act[img * S + lane], 0), beam);
        s_cap[lane] = min(max(cn.cap[img * S + lane], 0), beam);
    }
    beam_cons_words(cn, img, s_cw);
    __syncthreads();
    const int cr = lane / BEAM_MAX_K, cj = lane % BEAM_MAX_K, nslot = BEAM_MAX_K * BEAM_MAX_K + k * BEAM_CONS_SLOTS;
    int live = 0;
    for (int t = 0; t < S; ++t) {                                // uniform: the LDS words it branches on are read after a barrier
        const int capt = s_cap[t], tr0 = row0 + t * beam;
        {
            float val = -INFINITY;
            int idx = 0x7fffffff;
            if (cr < s_na[t] && cj < capt) {
                const int ci = cand_idx[(tr0 + cr) * BEAM_MAX_K + cj];
                if (ci >= 0 && ci < V) {          // a row with fewer than cap[t] admissible tokens leaves empty slots
                    val = cand_val[(tr0 + cr) * BEAM_MAX_K + cj];
                    idx = (t * beam + cr) * V + ci;
                }
            }
            if (!(val > -INFINITY)) idx = 0x7fffffff;
            s_cv[lane] = val; s_cf[lane] = idx;
        }
        for (int p = lane; p < k * BEAM_CONS_SLOTS; p += 64) {
            const int r = p / BEAM_CONS_SLOTS, q = p % BEAM_CONS_SLOTS, s = r / beam, j = r % beam, w = s_cw[q];
            float val = -INFINITY;
            int idx = 0x7fffffff;
            if (w >= 0 && w < V && j < s_na[s] && (s | (1 << (q / BEAM_CONS_MAX_A))) == t) {
                val = cn.force_val[(size_t)(row0 + r) * BEAM_CONS_SLOTS + q];
                if (val > -INFINITY) idx = r * V + w;
            }
            s_cv[BEAM_MAX_K * BEAM_MAX_K + p] = idx == 0x7fffffff ? -INFINITY : val;
            s_cf[BEAM_MAX_K * BEAM_MAX_K + p] = idx;
        }
        // a lane reads and clears only the positions it wrote: no barrier inside the rounds
        for (int j = 0; j < capt; ++j) {
            float best = -INFINITY;
            int bi = 0x7fffffff;
            for (int p = lane; p < nslot; p += 64) {
                const float v = s_cv[p];
                const int f = s_cf[p];
                if (v > best || (v == best && f < bi)) { best = v; bi = f; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (bi != 0x7fffffff)
                for (int p = lane; p < nslot; p += 64)
                    if (s_cf[p] == bi) { s_cv[p] = -INFINITY; s_cf[p] = 0x7fffffff; }      // taken (flat indices are unique)
            if (lane == 0) { pick_val[j] = best; pick_idx[j] = bi; }
        }
        __syncthreads();
        if (lane == 0) {
            int nn = 0, left = capt;
            for (int j = 0; j < capt; ++j) {
                if (pick_idx[j] == 0x7fffffff) continue;       // fewer finite candidates than capacity: the slot stays empty
                const int src = pick_idx[j] / V, tok = pick_idx[j] % V;
                if (tok == 2) {
                    --left;
                    if (a.hyp_cnt[img] < k) {
                        const int32_t* ss = a.seqs_in + (size_t)(row0 + src) * a.L;
                        const int slot = row0 + a.hyp_cnt[img]++;
                        a.hyp_score[slot] = pick_val[j];
                        a.hyp_len[slot] = a.step + 1;
                        cn.hyp_state[slot] = t;
                        int32_t* hs = a.hyp_seq + (size_t)slot * a.L;
                        for (int i = 0; i < a.step; ++i) hs[i] = ss[i];
                        hs[a.step] = 2;
                    }
                } else {
                    new_src[nn] = src; new_tok[nn] = tok; new_run[nn] = pick_val[j];
                    ++nn;
                }
            }
            s_newn = nn;
            a.n_act[img * S + t] = nn;
            cn.cap[img * S + t] = left;
            live += nn;
        }
        __syncthreads();
        const int nn = s_newn;
        for (int j = 0; j < beam; ++j) {
            if (j < nn) {
                const int32_t* ss = a.seqs_in + (size_t)(row0 + new_src[j]) * a.L;
                int32_t* so = a.seqs_out + (size_t)(tr0 + j) * a.L;
                for (int i = lane; i < a.step; i += 64) so[i] = ss[i];
                if (lane == 0) {
                    so[a.step] = new_tok[j];
                    a.run[tr0 + j] = new_run[j];
                    a.src_row[tr0 + j] = row0 + new_src[j];
                    a.it_next[tr0 + j] = new_tok[j];
                }
            } else if (lane == 0) {
                a.src_row[tr0 + j] = tr0 + j;
                a.it_next[tr0 + j] = 0;
            }
        }
        __syncthreads();                                         // the next target overwrites the candidates and pick_* / new_*
    }
    if (lane == 0 && live > 0) atomicAdd(a.n_live, 1);
}

// n-best selection of a constrained search, one wave per image: the image's at most k hypotheses are its retirements (hyp_*, in
// order of step, target state, merge rank) and the beams live at the limit in (state, slot) order.  Ranked: more satisfied
// constraints first (popcount of the state), then finished before live, then by the length-normalised score (descending), then
// by that order.  Writes the first n_best as beam_finalize_nbest_kernel does, and each one's state to sat [n_img, n_best] (0 for a
// rank past the image's hypotheses).
__global__ __launch_bounds__(64) void beam_finalize_states_kernel(int k, int beam, int S, int L, int steps_done, int n_best, int lp_kind,
                                                                  float lp_alpha, const int* __restrict__ n_act, const float* __restrict__ run,
                                                                  const int32_t* __restrict__ seqs, const int* __restrict__ hyp_cnt,
                                                                  const float* __restrict__ hyp_score, const int* __restrict__ hyp_len,
                                                                  const int32_t* __restrict__ hyp_state, const int32_t* __restrict__ hyp_seq,
                                                                  float* __restrict__ out, int32_t* __restrict__ lens,
                                                                  float* __restrict__ scores, int32_t* __restrict__ sat) {
    __shared__ int s_pick[BEAM_CONS_MAX_ROWS], s_src[BEAM_CONS_MAX_ROWS], s_state[BEAM_CONS_MAX_ROWS];
    const int img = blockIdx.x, lane = threadIdx.x, row0 = img * k;
    const int nf = min(max(hyp_cnt[img], 0), k);
    int nl = 0;
    for (int s = 0; s < S; ++s) nl += min(max(n_act[img * S + s], 0), beam);
    const int tot = min(nf + nl, k);
    const bool fin = lane < nf;
    float raw = -INFINITY;
    int len = 1, state = 0, src = row0;
    if (lane < tot) {
        if (fin) {
            src = row0 + lane;
            raw = hyp_score[src]; len = hyp_len[src]; state = hyp_state[src];
        } else {
            int q = lane - nf;
            for (int s = 0; s < S; ++s) {
                const int na = min(max(n_act[img * S + s], 0), beam);
                if (q < na) { state = s; src = row0 + s * beam + q; break; }
                q -= na;
            }
            raw = run[src]; len = steps_done + 1;
        }
    }
    const float ns = beam_lp_norm(raw, len - 1, lp_kind, lp_alpha);
    const int pc = __popc(state);
    int rank = 0;
    for (int f = 0; f < tot; ++f) {
        const float f_ns = __shfl(ns, f, 64);
        const int f_pc = __shfl(pc, f, 64);
        const bool f_fin = f < nf;
        rank += f_pc > pc || (f_pc == pc && ((f_fin && !fin) || (f_fin == fin && (f_ns > ns || (f_ns == ns && f < lane)))));
    }
    if (lane < BEAM_CONS_MAX_ROWS) s_pick[lane] = -1;
    __syncthreads();
    if (lane < tot) { s_pick[rank] = lane; s_src[lane] = src; s_state[lane] = state; }
    __syncthreads();
    for (int m = 0; m < n_best; ++m) {
        const int e = s_pick[m], o = img * n_best + m;
        const int32_t* sp = e < 0 ? nullptr : e < nf ? hyp_seq + (size_t)s_src[e] * L : seqs + (size_t)s_src[e] * L;
        const int ln = e < 0 ? 0 : e < nf ? hyp_len[s_src[e]] : steps_done + 1;
        for (int i = lane; i < L; i += 64) out[(size_t)o * L + i] = i < ln ? (float)sp[i] : 0.f;
        if (lane == 0) {
            lens[o] = ln;
            scores[o] = e < 0 ? -INFINITY : e < nf ? hyp_score[s_src[e]] : run[s_src[e]];
            sat[o] = e < 0 ? 0 : s_state[e];
        }
    }
}

}  // namespace
}  // namespace icz
