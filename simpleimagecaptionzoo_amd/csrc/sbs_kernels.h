// Kernels of stochastic beam search (Kool, van Hoof and Welling, "Stochastic Beams and Where to Find Them", ICML 2019): n distinct
// captions per image that are a sample without replacement from the model's sequence distribution (include/icz.h:
// icz_*_sample_distinct; the driver is stochastic_beam.hip).  Row img * n + slot holds a hypothesis: its tokens, phi (fp32 running
// sum of its token log-probs), G (its perturbed value, float64) and a frozen flag (it has emitted <end>); the occupied slots of an
// image are 0 .. occ[img] - 1, sorted by G descending.
//   sbs_rowtopk_kernel   grid (rows), 256 threads: the row's log-softmax at the temperature, g[v] = phi + lp[v] + gumbel(u[v]) with
//                        the noise made inside the selection sweep, and the row's n largest g with their phi + lp and v
//   sbs_merge_kernel     grid (n_img), one wave: conditions the <= n * n candidates on their parents' G in float64, keeps the n
//                        largest and writes the image's new slots
// The conditioning map is monotone in g, so a row's top n by g are its top n after conditioning: only those are transformed.
#pragma once
#include "ens_sample.h"
#include "rng.h"

namespace icz {
namespace {

constexpr int SBS_MAX_N = 8;          // slots per image; also the slot stride of the Philox counter (not n: a run's first j hypotheses
                                      // are then the run with n = j on the same seed)
constexpr int SBS_NONE = 0x7fffffff;
constexpr int SBS_MAX_LEN = 256;      // steps of one search
constexpr int SBS_MAX_IMAGES = 1 << 28;      // (first image + image) * 8 + slot is one 32-bit word of the Philox counter

// uniform strictly inside (0, 1) from 32 random bits: ((r >> 9) + 0.5) * 2^-23, exact in fp32
__host__ __device__ inline float sbs_uniform(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-07f; }
__device__ __forceinline__ float sbs_gumbel(float u) { return -logf(-logf(u)); }
// the four words of tokens 4 q .. 4 q + 3 of (image, slot) at `step` (the root: step 0, slot 0, q = 0, word 0)
__host__ __device__ inline uint4_ sbs_philox(uint64_t seed, int q, int img, int slot, int step) {
    const uint4_ c = {(uint32_t)q, (uint32_t)(img * SBS_MAX_N + slot), (uint32_t)step, (uint32_t)RNG_GUMBEL};
    return philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// log(1 - exp(a)), a <= 0 (a = 0: -inf)
__device__ inline double sbs_log1mexp(double a) { return a > -0.6931471805599453 ? log(-expm1(a)) : log1p(-exp(a)); }
// G~ = -log(exp(-Tp) - exp(-Z) + exp(-g)) in its stable form: the row's argmax (g = Z) gets exactly Tp, everything else less
__device__ inline double sbs_condition(double Tp, double g, double Z) {
    const double w = Tp - g + sbs_log1mexp(g - Z);
    return Tp - fmax(0.0, w) - log1p(exp(-fabs(w)));
}

struct SbsRowArgs {
    LogitsView lv; int V, n, step, compact;      // compact (step 1 only): the logits hold one row per image
    float temperature;
    const int* occ; const uint8_t* frozen; const float* phi;      // [n_img] [rows] [rows]
    const float* uniforms;            // [n_img, n, V] of this step, or null: Philox (seed, step, image, slot, v) under RNG_GUMBEL
    uint64_t seed; int img0;          // Philox: the key, and the index of image 0 of this call within its batch (a chunked batch)
    float* cand_g; float* cand_phi; int* cand_idx;                // [rows, 8]: the first n of a scored row, g descending
};

// one finished logit (the slabs summed in slab order, then the bias: the bits of ens_load4)
__device__ __forceinline__ float sbs_load1(const LogitsView& l, int row, int v) {
    const float* r = l.p + (size_t)row * l.ld;
    float y = r[v];
    for (int z = 1; z < l.ns; ++z) y += r[(size_t)z * l.slab_stride + v];
    if (l.ns > 1) y += l.bias[v];
    return y;
}

// The sweeps of beam_rowtopk_kernel (batched independent loads; a max sweep, a sum-exp sweep, a selection sweep with per-thread
// sorted lists and n rounds of block-wide best), over quads of tokens: thread t owns tokens 4 (t + 256 i) .. + 3, one 16-byte load
// per slab and one Philox call per quad.  The list keeps (g, v); phi + lp of the n winners is recomputed from their logits by the
// same fp32 expression.  A token whose g is -inf (or NaN) is never emitted: a row may emit fewer than n (cand_idx -1, g and phi -inf).
// A frozen or unoccupied row returns at entry: its logits are never read, its candidates never written.
__global__ __launch_bounds__(256) void sbs_rowtopk_kernel(SbsRowArgs a) {
    __shared__ float smf[4];
    __shared__ float s_val[4];
    __shared__ int s_idx[4], s_who[4];
    __shared__ int s_ci[SBS_MAX_N];
    const int row = blockIdx.x, n = a.n, img = row / n, slot = row % n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = a.V;
    if (slot >= a.occ[img] || a.frozen[row]) return;
    const int lrow = a.compact ? img : row;
    const bool vec = ens_vec_ok(a.lv);
    const float T = a.temperature;
    const int NQ = (V + 3) >> 2;
    constexpr int U = 4;
    auto slice = [&](int q0, f32x4 (&x)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            x[u] = ens_load4(a.lv, lrow, 4 * (q0 + 256 * u), V, vec);      // columns >= V: -inf, not read
#pragma unroll
            for (int j = 0; j < 4; ++j) x[u][j] = x[u][j] / T;
        }
    };
    float mx = -INFINITY;
    for (int q0 = tid; q0 < NQ; q0 += 256 * U) {
        f32x4 x[U];
        slice(q0, x);
#pragma unroll
        for (int u = 0; u < U; ++u) mx = fmaxf(mx, fmaxf(fmaxf(x[u][0], x[u][1]), fmaxf(x[u][2], x[u][3])));
    }
    mx = block_max_256(mx, smf);
    float se = 0.f;
    for (int q0 = tid; q0 < NQ; q0 += 256 * U) {
        f32x4 x[U];
        slice(q0, x);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) se += expf(x[u][j] - mx);          // exp(-inf) = 0 beyond V
    }
    se = block_sum_256(se, smf);
    const float ls = logf(se);
    const float ph = a.phi[row];
    const float* un = a.uniforms ? a.uniforms + (size_t)row * V : nullptr;
    float tv[SBS_MAX_N];
    int ti[SBS_MAX_N];
#pragma unroll
    for (int j = 0; j < SBS_MAX_N; ++j) { tv[j] = -INFINITY; ti[j] = SBS_NONE; }
    float worst = -INFINITY;
    int worst_i = SBS_NONE;
    for (int q0 = tid; q0 < NQ; q0 += 256 * U) {
        f32x4 x[U];
        slice(q0, x);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + 256 * u;
            if (q >= NQ) continue;
            float uu[4];
            if (un) {
#pragma unroll
                for (int j = 0; j < 4; ++j) uu[j] = 4 * q + j < V ? un[4 * q + j] : 0.5f;
            } else {
                const uint4_ r = sbs_philox(a.seed, q, a.img0 + img, slot, a.step);
                uu[0] = sbs_uniform(r.x); uu[1] = sbs_uniform(r.y); uu[2] = sbs_uniform(r.z); uu[3] = sbs_uniform(r.w);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float pc = ph + ((x[u][j] - mx) - ls);
                float val = pc + sbs_gumbel(uu[j]);
                int idx = 4 * q + j;
                if (!(val > -INFINITY)) continue;                          // -inf (beyond V, a -inf logit) and NaN: never emitted
                if (!(val > worst || (val == worst && idx < worst_i))) continue;
#pragma unroll
                for (int p = 0; p < SBS_MAX_N; ++p) {                      // branch-free insertion: swap down the list
                    const bool take = (p < n) & ((val > tv[p]) | ((val == tv[p]) & (idx < ti[p])));
                    const float ov = tv[p]; const int oi = ti[p];
                    tv[p] = take ? val : ov; ti[p] = take ? idx : oi;
                    val = take ? ov : val; idx = take ? oi : idx;
                }
#pragma unroll
                for (int p = 0; p < SBS_MAX_N; ++p) {
                    worst = (p == n - 1) ? tv[p] : worst;
                    worst_i = (p == n - 1) ? ti[p] : worst_i;
                }
            }
        }
    }
    // n rounds: every thread offers the head of its list, the block takes the best and that thread pops it
    int head = 0;
    for (int j = 0; j < n; ++j) {
        float best = -INFINITY;
        int bi = SBS_NONE;
#pragma unroll
        for (int q = 0; q < SBS_MAX_N; ++q)
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
        if (tid == who && bi != SBS_NONE) ++head;
        if (tid == 0) {
            const bool some = bi != SBS_NONE;
            a.cand_g[row * SBS_MAX_N + j] = some ? best : -INFINITY;
            a.cand_idx[row * SBS_MAX_N + j] = some ? bi : -1;
            s_ci[j] = some ? bi : -1;
        }
        __syncthreads();
    }
    if (tid < n) {
        const int v = s_ci[tid];
        a.cand_phi[row * SBS_MAX_N + tid] = v >= 0 ? ph + ((sbs_load1(a.lv, lrow, v) / T - mx) - ls) : -INFINITY;
    }
}

struct SbsMergeArgs {
    int V, n, step, L;                // step 1 ..; L = max_len, the sequence capacity (no <sta> is stored)
    int* occ; uint8_t* frozen; float* phi; double* G; int* len;   // [n_img] [rows] ..: read, then rewritten in place
    const int32_t* seqs_in; int32_t* seqs_out;                    // [rows, L]
    int32_t* src_row; int64_t* it_next;                           // [rows]
    int* n_live;                      // [1] rows occupied and not frozen after this step, over all images
    const float* cand_g; const float* cand_phi; const int* cand_idx;
};

// One wave per image; lane c <-> candidate (parent slot c / 8, rank c % 8).  A live parent offers its emitted candidates with
// G~ = sbs_condition(G[parent], g, Z), Z = its rank-0 g; a frozen parent offers itself once with its G unchanged.  The n largest G~
// (ties: the lower (parent slot, v); a frozen parent counts as v = 0) become slots 0 .. n-1 in that order.  Every value of the old
// slots is in registers before the first new one is written.  A new hypothesis whose token is <end> is frozen on entry; a frozen
// hypothesis keeps its tokens, phi, G and length and steps on <pad>.  Slots past the survivors: src_row = itself, <pad>, nothing else.
__global__ __launch_bounds__(64) void sbs_merge_kernel(SbsMergeArgs a) {
    __shared__ double pick_G[SBS_MAX_N];
    __shared__ int pick_lane[SBS_MAX_N];
    __shared__ int s_src[SBS_MAX_N], s_tok[SBS_MAX_N], s_len[SBS_MAX_N];
    const int img = blockIdx.x, lane = threadIdx.x, n = a.n, V = a.V, row0 = img * n;
    const int oc = min(max(a.occ[img], 0), n);
    const int cr = lane / SBS_MAX_N, cj = lane % SBS_MAX_N;
    double Gt = -INFINITY;
    int flat = SBS_NONE;
    if (cr < oc) {
        const int row = row0 + cr;
        const double Tp = a.G[row];
        if (a.frozen[row]) {
            if (cj == 0) { Gt = Tp; flat = cr * V; }
        } else if (cj < n) {
            const int ci = a.cand_idx[row * SBS_MAX_N + cj];
            if (ci >= 0 && ci < V) {
                Gt = sbs_condition(Tp, (double)a.cand_g[row * SBS_MAX_N + cj], (double)a.cand_g[row * SBS_MAX_N]);
                flat = cr * V + ci;
            }
        }
        if (!(Gt > -INFINITY)) flat = SBS_NONE;      // -inf or NaN: no candidate
    }
    if (flat == SBS_NONE) Gt = -INFINITY;
    for (int j = 0; j < n; ++j) {
        double best = Gt;
        int bf = flat, bl = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int of = __shfl_xor(bf, o, 64), ol = __shfl_xor(bl, o, 64);
            if (ob > best || (ob == best && of < bf)) { best = ob; bf = of; bl = ol; }
        }
        if (flat == bf && bf != SBS_NONE) { Gt = -INFINITY; flat = SBS_NONE; }      // taken (flat indices are unique)
        if (lane == 0) { pick_G[j] = best; pick_lane[j] = bf == SBS_NONE ? -1 : bl; }
    }
    __syncthreads();
    bool valid = false, nfz = false;
    int srow = 0, tok = 0, nlen = 0;
    float nphi = 0.f;
    double nG = 0.0;
    if (lane < n && pick_lane[lane] >= 0) {
        const int pl = pick_lane[lane], src = pl / SBS_MAX_N, rk = pl % SBS_MAX_N;
        valid = true;
        srow = row0 + src;
        const bool fz = a.frozen[srow] != 0;
        tok = fz ? -1 : a.cand_idx[srow * SBS_MAX_N + rk];
        nphi = fz ? a.phi[srow] : a.cand_phi[srow * SBS_MAX_N + rk];
        nlen = fz ? min(max(a.len[srow], 0), a.L) : a.step;
        nG = pick_G[lane];
        nfz = fz || tok == 2;
    }
    const int cnt = __popcll(__ballot(valid)), live = __popcll(__ballot(valid && !nfz));
    __syncthreads();                  // every read of the old slots is done
    if (lane < n) {
        const int row = row0 + lane;
        if (valid) {
            a.phi[row] = nphi; a.G[row] = nG; a.frozen[row] = nfz ? 1 : 0; a.len[row] = nlen;
            a.src_row[row] = srow;
            a.it_next[row] = nfz ? 0 : tok;
            s_src[lane] = srow; s_tok[lane] = tok; s_len[lane] = nlen;
        } else {
            a.src_row[row] = row;
            a.it_next[row] = 0;
        }
    }
    if (lane == 0) {
        a.occ[img] = cnt;
        if (live > 0) atomicAdd(a.n_live, live);
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
        const int32_t* ss = a.seqs_in + (size_t)s_src[j] * a.L;
        int32_t* so = a.seqs_out + (size_t)(row0 + j) * a.L;
        const int t = s_tok[j], keep = t < 0 ? s_len[j] : s_len[j] - 1;      // a frozen parent: all its tokens; else its step - 1
        for (int i = lane; i < keep; i += 64) so[i] = ss[i];
        if (lane == 0 && t >= 0) so[s_len[j] - 1] = t;
    }
}

// start of a search: <sta> on every row, the image of each row, slot 0 of every image occupied with phi = 0 and G = gumbel(u_root) in
// float64 (root_uniforms [n_img], or null: Philox step 0, slot 0, v = 0, image img0 + img), every other slot empty
__global__ void sbs_init_kernel(int n_img, int n, const float* root_uniforms, uint64_t seed, int img0, int* occ, uint8_t* frozen, float* phi, double* G,
                                int* len, int64_t* it, int32_t* img_of_row, int32_t* src_row) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_img * n) return;
    const int img = row / n, slot = row % n;
    it[row] = 1;
    img_of_row[row] = img;
    src_row[row] = row;
    frozen[row] = 0;
    len[row] = 0;
    if (slot == 0) {
        const float u = root_uniforms ? root_uniforms[img] : sbs_uniform(sbs_philox(seed, 0, img0 + img, 0, 0).x);
        occ[img] = 1;
        phi[row] = 0.f;
        G[row] = -log(-log((double)u));
    } else {
        phi[row] = -INFINITY;
        G[row] = -INFINITY;
    }
}

// The outputs, one wave per image, slot order (G descending): ids [n_img n, L] int64 in the format of icz_*_sample_decode (no <sta>,
// <end> included, 0 behind it), the length, finished (0: cut at the step limit), phi and G; an unoccupied slot: zeros, phi = G = -inf.
__global__ __launch_bounds__(64) void sbs_finalize_kernel(int n, int L, const int* __restrict__ occ, const uint8_t* __restrict__ frozen,
                                                          const float* __restrict__ phi, const double* __restrict__ G,
                                                          const int* __restrict__ len, const int32_t* __restrict__ seqs,
                                                          int64_t* __restrict__ ids_out, int32_t* __restrict__ len_out,
                                                          int32_t* __restrict__ fin_out, float* __restrict__ phi_out, double* __restrict__ g_out) {
    const int img = blockIdx.x, lane = threadIdx.x, oc = min(max(occ[img], 0), n);
    for (int j = 0; j < n; ++j) {
        const int row = img * n + j;
        const bool has = j < oc;
        const int ln = has ? min(max(len[row], 0), L) : 0;
        for (int i = lane; i < L; i += 64) ids_out[(size_t)row * L + i] = i < ln ? (int64_t)seqs[(size_t)row * L + i] : 0;
        if (lane == 0) {
            len_out[row] = ln;
            fin_out[row] = has && frozen[row] ? 1 : 0;
            phi_out[row] = has ? phi[row] : -INFINITY;
            g_out[row] = has ? G[row] : -INFINITY;
        }
    }
}

}  // namespace
}  // namespace icz
