// Sampling decode (beyond the reference; include/icz.h: icz_*_sample_decode): n captions per image drawn in evaluation mode with
// temperature, top-k and nucleus (top-p) filtering.  One kernel per step, sample_decode_kernel, behind the member's own decoder
// step (DecodeMember, decoder_core.h); the SCST rollout's sample_select_kernel and the greedy / beam kernels are not touched.
// A model ensemble (ensemble.hip) draws through the same kernel: its second instance fills the row from the members' logits.
#include <cmath>
#include <type_traits>

#include "ens_sample.h"
#include "token_kernels.h"

namespace icz {

constexpr int SD_THREADS = 1024;              // 16 waves per row: the row (40 KB at V = 10 102) sits in LDS, as in sample_select_kernel
constexpr int SD_NW = SD_THREADS / 64;
constexpr double SD_FIX = 1099511627776.0;    // 2^40: a survivor's mass exp(y - max y) in (0, 1] as a fixed-point integer

// float -> unsigned key of the same order (-0 = +0)
__device__ __forceinline__ uint32_t sd_key(float x) {
    const uint32_t b = __float_as_uint(x == 0.f ? 0.f : x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// a token's mass exp(x / temperature - max), in float64 as the definition says
__device__ __forceinline__ double sd_mass(float x, double temp, double ymax) { return exp((double)x / temp - ymax); }
__device__ __forceinline__ unsigned long long sd_fix(double m) { return (unsigned long long)(m * SD_FIX); }

// The prefix of the order (key descending, index ascending): key > cut_key, or key == cut_key and index <= cut_idx.
struct SdCut { uint32_t key; int idx; };
__device__ __forceinline__ bool sd_in(const SdCut& c, uint32_t key, int v) { return key > c.key || (key == c.key && v <= c.idx); }

// Radix select over the keys of the row in LDS, 8 bits per pass with a 256-bin integer histogram: the shortest prefix of the order
// whose weight reaches `need`, over the tokens inside `dom`.  MASS = false: weight 1 per token (top-k, need = k); MASS = true:
// weight = the token's fixed-point mass (nucleus, need = ceil(top_p x the mass of dom)).  Integer sums only: the result does not
// depend on the order the atomics land in.  Every thread of the workgroup calls it and gets the cut.
template <bool MASS>
__device__ SdCut sd_select(const float* srow, int V, const SdCut dom, unsigned long long need, double temp, double ymax,
                           unsigned long long* hist, unsigned long long* s_u64, int* s_i32) {
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t prefix = 0;
    unsigned long long above = 0;             // weight of the tokens whose key lies above the prefix's range
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int v = tid; v < V; v += SD_THREADS) {
            const float x = srow[v];
            const uint32_t key = sd_key(x);
            if (!sd_in(dom, key, v)) continue;
            if (pass > 0 && (key >> (shift + 8)) != (prefix >> (shift + 8))) continue;
            const unsigned long long w = MASS ? sd_fix(sd_mass(x, temp, ymax)) : 1ull;
            if (w) atomicAdd(&hist[(key >> shift) & 255u], w);
        }
        __syncthreads();
        if (tid < 64) {       // wave 0: lane l owns bins 255 - 4 l .. 252 - 4 l; the first bin (descending) where the running weight reaches need
            unsigned long long loc[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { loc[j] = hist[255 - 4 * lane - j]; sum += loc[j]; }
            unsigned long long inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long up = __shfl_up(inc, o, 64);
                if (lane >= o) inc += up;
            }
            unsigned long long c = above + inc - sum;
            int bin = -1;
            unsigned long long ab = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (bin < 0 && loc[j] != 0 && c + loc[j] >= need) { bin = 255 - 4 * lane - j; ab = c; }
                c += loc[j];
            }
            const unsigned long long hit = __ballot(bin >= 0);
            const int first = hit ? __ffsll((long long)hit) - 1 : 63;
            if (!hit && lane == 63) { bin = 0; ab = c - loc[3]; }          // need above the whole weight (rounding): everything
            if (lane == first) { s_i32[0] = bin; s_u64[0] = ab; }
        }
        __syncthreads();
        prefix |= (uint32_t)s_i32[0] << shift;
        above = s_u64[0];
        __syncthreads();
    }
    // the tokens whose key IS the cut's: the lowest indices first, until the weight is reached
    const int per = (V + SD_THREADS - 1) / SD_THREADS;
    const int v0 = min(V, tid * per), v1 = min(V, v0 + per);
    int cnt = 0;
    unsigned long long w = 0;
    for (int v = v0; v < v1; ++v) {
        const float x = srow[v];
        if (sd_key(x) == prefix && sd_in(dom, prefix, v)) {
            ++cnt;
            if (MASS) w = sd_fix(sd_mass(x, temp, ymax));
        }
    }
    if (MASS) {       // one mass for all of them (one key = one x): hand it to every thread
        if (tid == 0) s_u64[1] = 0;
        __syncthreads();
        if (w) atomicMax(&s_u64[1], w);
        __syncthreads();
        w = s_u64[1];
    } else {
        w = 1;
    }
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) s_i32[1 + (tid >> 6)] = inc;
    if (tid == 0) s_i32[0] = V - 1;
    __syncthreads();
    int before = inc - cnt, total = 0;
    for (int wv = 0; wv < SD_NW; ++wv) {
        if (wv < (tid >> 6)) before += s_i32[1 + wv];
        total += s_i32[1 + wv];
    }
    const unsigned long long rem = need > above ? need - above : 1;
    unsigned long long nk = w ? (rem + w - 1) / w : (unsigned long long)total;
    if (nk > (unsigned long long)total) nk = total;
    if (nk < 1) nk = 1;
    if (cnt && (unsigned long long)before < nk && nk <= (unsigned long long)(before + cnt)) {      // the nk-th of them is in this slice
        int seen = before;
        for (int v = v0; v < v1; ++v)
            if (sd_key(srow[v]) == prefix && sd_in(dom, prefix, v) && (unsigned long long)++seen == nk) { s_i32[0] = v; break; }
    }
    __syncthreads();
    SdCut out = {prefix, s_i32[0]};
    __syncthreads();
    return out;
}

// One workgroup of 16 waves per row.  Passes: (1) finished logits x = the predict GEMM's split-K slabs summed in slab order + bias
// -> LDS, row maximum, lse of x (the reported log-probability is the model's own); (2) top-k: sd_select on counts; (3) nucleus:
// the survivors' mass as an integer sum, sd_select on masses; (4) the float64 prefix sums of the survivors' masses over contiguous
// slices (one fixed order) and the inverse-CDF draw; (5) token, log-probability, finished flag, the count of unfinished rows and the
// next step's input embedding.  With both filters off passes 2 and 3 are skipped.
// Two instances, one per row source (A).  SampleDecArgs: pass 1 as above.  EnsSampleDecArgs (a model ensemble): pass 1 fills the row
// with lp[v] = log(sum_m w_m softmax(logits_m)[v]) as ensemble_logprob_kernel defines it -- per member one online max / sum-exp pass
// over its logits, then one pass that writes lp shifted by the largest term over m; the members' logits are read twice from global
// memory (L2), the combined row never leaves LDS -- and the tail writes every member's next input embedding.  Passes 2 - 5 are one code.
__device__ __forceinline__ const SampleDecArgs& sd_args(const SampleDecArgs& a) { return a; }
__device__ __forceinline__ const SampleDecArgs& sd_args(const EnsSampleDecArgs& a) { return a.s; }

// emb_next[row, :E] = table[tok] (relu: behind a ReLU)
__device__ __forceinline__ void sd_write_emb(const float* table, float* emb_next, int E, int relu, int row, int tok) {
    for (int e = threadIdx.x * 4; e < E; e += 4 * SD_THREADS) {
        f32x4 x = *reinterpret_cast<const f32x4*>(table + (size_t)tok * E + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = relu ? fmaxf(x[j], 0.f) : x[j];
        *reinterpret_cast<f32x4*>(emb_next + (size_t)row * E + e) = x;
    }
}
template <class A>
__device__ __forceinline__ void sd_next_emb(const A& args, int row, int tok) {
    if constexpr (std::is_same_v<A, EnsSampleDecArgs>) {
        for (int m = 0; m < args.ens.M; ++m) {
            const DecodeMember::EmbSlot& s = args.emb[m];
            if (s.emb) sd_write_emb(s.table, s.emb, s.E, s.relu, row, tok);
        }
    } else {
        if (args.emb_next) sd_write_emb(args.emb_table, args.emb_next, args.E, args.relu, row, tok);
    }
}

template <class A>
__global__ __launch_bounds__(SD_THREADS) void sample_decode_kernel(A args) {
    constexpr bool ENS = std::is_same_v<A, EnsSampleDecArgs>;
    const SampleDecArgs& a = sd_args(args);
    extern __shared__ __attribute__((aligned(16))) float srow[];     // V floats: the finished logits of the row
    __shared__ unsigned long long hist[256];
    __shared__ unsigned long long s_u64[SD_NW];
    __shared__ double smd[SD_NW];
    __shared__ float smf[SD_NW];
    __shared__ int s_i32[SD_NW + 1];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = a.V;
    const bool all_dead = a.n_unf && a.t > 0 && a.n_unf[a.t - 1] == 0;      // the kernels of this step returned at entry (step_dead)
    const bool was_fin = a.fin && a.t > 0 && a.fin[row] != 0;
    if (all_dead || was_fin) {
        if (tid == 0) {
            a.ids_out[(size_t)row * a.T + a.t] = 0;
            a.logp_out[(size_t)row * a.T + a.t] = 0.f;
            if (a.it_next) a.it_next[row] = 0;
        }
        if (!all_dead) sd_next_emb(args, row, 0);       // the others go on: this row keeps running on <pad> (finite, never read)
        return;
    }
    const float u = a.uniforms ? a.uniforms[row] : rng_uniform(a.seed, (uint32_t)a.t, (uint64_t)row, RNG_DECODE);
    // pass 1
    float mx = -INFINITY;
    if constexpr (ENS) {
        __shared__ float sms[SD_NW];
        const EnsArgs& en = args.ens;
        float shift[ENS_MAX_M];           // log w_m - lse_m
        bool vec[ENS_MAX_M];
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m) {
            shift[m] = -INFINITY;
            vec[m] = false;
            if (m >= en.M) continue;
            const LogitsView& l = en.m[m];
            vec[m] = ens_vec_ok(l);
            float mm = -INFINITY, s = 0.f;
            for (int v = tid * 4; v < V; v += 4 * SD_THREADS) {
                const f32x4 x = ens_load4(l, row, v, V, vec[m]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float y = x[j];
                    if (y > mm) { s = s * expf(mm - y) + 1.f; mm = y; }
                    else if (y != -INFINITY) s += expf(y - mm);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) lse_combine(mm, s, __shfl_xor(mm, o, 64), __shfl_xor(s, o, 64));
            if (lane == 0) { smf[wave] = mm; sms[wave] = s; }
            __syncthreads();
            mm = smf[0]; s = sms[0];
            for (int w = 1; w < SD_NW; ++w) lse_combine(mm, s, smf[w], sms[w]);      // one fixed order
            __syncthreads();              // smf / sms are rewritten by the next member
            shift[m] = en.logw[m] - (mm + logf(s));
        }
        for (int v = tid * 4; v < V; v += 4 * SD_THREADS) {
            f32x4 term[ENS_MAX_M];
            f32x4 top = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int m = 0; m < ENS_MAX_M; ++m) {
                if (m >= en.M) continue;
                term[m] = ens_load4(en.m[m], row, v, V, vec[m]) + shift[m];
#pragma unroll
                for (int j = 0; j < 4; ++j) top[j] = fmaxf(top[j], term[m][j]);
            }
            f32x4 lp;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = 0.f;
#pragma unroll
                for (int m = 0; m < ENS_MAX_M; ++m)
                    if (m < en.M && term[m][j] != -INFINITY) s += expf(term[m][j] - top[j]);
                lp[j] = top[j] == -INFINITY ? -INFINITY : top[j] + logf(s);
            }
            if (v + 4 <= V) {
                *reinterpret_cast<f32x4*>(srow + v) = lp;
                mx = fmaxf(mx, fmaxf(fmaxf(lp[0], lp[1]), fmaxf(lp[2], lp[3])));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (v + j < V) { srow[v + j] = lp[j]; mx = fmaxf(mx, lp[j]); }
            }
        }
    } else {
        const LogitsView& L = a.lv;
        const float* l = L.p + (size_t)row * L.ld;
        const bool vec = ((L.ld | (int)(L.slab_stride & 3)) & 3) == 0 && (((uintptr_t)L.p | (uintptr_t)L.bias) & 15) == 0;
        const int Vv = vec ? (V & ~3) : 0;
        for (int v = tid * 4; v < Vv; v += 4 * SD_THREADS) {
            f32x4 x = *reinterpret_cast<const f32x4*>(l + v);
            for (int z = 1; z < L.ns; ++z) x += *reinterpret_cast<const f32x4*>(l + (size_t)z * L.slab_stride + v);
            if (L.ns > 1) x += *reinterpret_cast<const f32x4*>(L.bias + v);
            *reinterpret_cast<f32x4*>(srow + v) = x;
            mx = fmaxf(mx, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
        }
        for (int v = Vv + tid; v < V; v += SD_THREADS) {
            float x = l[v];
            for (int z = 1; z < L.ns; ++z) x += l[(size_t)z * L.slab_stride + v];
            if (L.ns > 1) x += L.bias[v];
            srow[v] = x;
            mx = fmaxf(mx, x);
        }
    }
    mx = block_max_n(mx, smf, SD_NW);
    const int per = (V + SD_THREADS - 1) / SD_THREADS;
    const int v0 = min(V, tid * per), v1 = min(V, v0 + per);
    double lse;
    {   // log(sum exp(x - M)): fp32 terms, float64 sums in one fixed order
        double se = 0.0;
        for (int v = v0; v < v1; ++v) se += (double)expf(srow[v] - mx);
        se = wave_sum_d(se);
        if (lane == 0) smd[wave] = se;
        __syncthreads();
        se = 0.0;
        for (int w = 0; w < SD_NW; ++w) se += smd[w];
        __syncthreads();
        lse = log(se);
    }
    const double temp = (double)a.temperature, ymax = (double)mx / temp;
    SdCut cut = {0u, V - 1};          // every token
    if (a.top_k > 0 && a.top_k < V) cut = sd_select<false>(srow, V, cut, (unsigned long long)a.top_k, temp, ymax, hist, s_u64, s_i32);
    if (a.top_p < 1.0f) {
        unsigned long long tot = 0;
        for (int v = tid; v < V; v += SD_THREADS) {
            const float x = srow[v];
            if (sd_in(cut, sd_key(x), v)) tot += sd_fix(sd_mass(x, temp, ymax));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
        if (lane == 0) s_u64[wave] = tot;
        __syncthreads();
        tot = 0;
        for (int w = 0; w < SD_NW; ++w) tot += s_u64[w];
        __syncthreads();
        unsigned long long need = (unsigned long long)ceil((double)a.top_p * (double)tot);
        if (need < 1) need = 1;
        cut = sd_select<true>(srow, V, cut, need, temp, ymax, hist, s_u64, s_i32);
    }
    if (a.keep_out)
        for (int v = tid; v < V; v += SD_THREADS) a.keep_out[(size_t)row * V + v] = sd_in(cut, sd_key(srow[v]), v) ? 1 : 0;
    // pass 4: contiguous slice per thread -> the first index above the target is the minimum over the threads
    double loc = 0.0;
    for (int v = v0; v < v1; ++v) {
        const float x = srow[v];
        if (sd_in(cut, sd_key(x), v)) loc += sd_mass(x, temp, ymax);
    }
    double inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) smd[wave] = inc;
    __syncthreads();
    double wave_off = 0.0, total = 0.0;
    for (int w = 0; w < SD_NW; ++w) {
        const double s = smd[w];
        if (w < wave) wave_off += s;
        total += s;
    }
    const double target = (double)u * total;
    int cand = 0x7fffffff;
    {
        // [lower, upper) of this thread's slice: lower IS the previous lane's upper (sample_select_kernel has the reason); the
        // slice's last survivor carries the scan's own cumulative value
        const double prev = __shfl_up(inc, 1, 64);
        double run = wave_off + (lane ? prev : 0.0);
        if (run <= target && wave_off + inc > target) {
            int last = -1;
            for (int v = v0; v < v1; ++v) {
                const float x = srow[v];
                if (!sd_in(cut, sd_key(x), v)) continue;
                last = v;
                run += sd_mass(x, temp, ymax);
                if (run > target) break;
            }
            if (last >= 0) cand = last;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    if (lane == 0) s_i32[wave] = cand;
    __syncthreads();
    int d = s_i32[0];
#pragma unroll
    for (int w = 1; w < SD_NW; ++w) d = min(d, s_i32[w]);
    if ((unsigned)d >= (unsigned)V) {         // no slice claimed the target (a row of NaN logits): the largest token, which always survives
        d = V - 1;
        for (int v = 0; v < V; ++v)
            if (srow[v] == mx) { d = v; break; }
    }
    const bool unf = d != 2;
    const int nxt = unf ? d : 0;
    if (tid == 0) {
        const float lp = (float)((double)(srow[d] - mx) - lse);
        a.ids_out[(size_t)row * a.T + a.t] = d;
        a.logp_out[(size_t)row * a.T + a.t] = lp;
        if (a.score_out) a.score_out[row] = a.t == 0 ? lp : a.score_out[row] + lp;
        if (a.it_next) a.it_next[row] = nxt;
        if (a.fin) a.fin[row] = unf ? 0 : 1;
        if (a.n_unf && unf) atomicAdd(&a.n_unf[a.t], 1);
    }
    sd_next_emb(args, row, nxt);
}

// start of a decode: <sta>, no row finished, row r belongs to image r / n, the per-step counters of unfinished rows = 0
__global__ void sample_decode_init_kernel(int64_t* it, uint8_t* fin, int32_t* img_of_row, int rows, int n, int* n_unf, int T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) { it[i] = 1; fin[i] = 0; img_of_row[i] = i / n; }
    if (i < T) n_unf[i] = 0;
}

void launch_sample_decode_init(int64_t* it, uint8_t* fin, int32_t* img_of_row, int rows, int n, int* n_unf, int T, hipStream_t st) {
    hipLaunchKernelGGL(sample_decode_init_kernel, dim3(cdiv(rows > T ? rows : T, 256)), dim3(256), 0, st, it, fin, img_of_row, rows, n, n_unf, T);
}

template <class A>
static int launch_sample_decode_t(const A& a, int V, int rows, hipStream_t st) {
    static bool lds_set = false;          // one per instance
    if (!lds_set) {
        ICZ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sample_decode_kernel<A>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          160 * 1024 - 4096));
        lds_set = true;
    }
    hipLaunchKernelGGL(sample_decode_kernel<A>, dim3(rows), dim3(SD_THREADS), sizeof(float) * V, st, a);
    return ICZ_OK;
}
int launch_sample_decode(const SampleDecArgs& a, int rows, hipStream_t st) { return launch_sample_decode_t(a, a.V, rows, st); }
int launch_sample_decode(const EnsSampleDecArgs& a, int rows, hipStream_t st) { return launch_sample_decode_t(a, a.s.V, rows, st); }

// V < 0: no handle yet, the vocabulary is not known (its rules are checked once it is)
int check_sample_opts(const char* who, const icz_sample_opts* o, int n_img, int n, int V, int max_rows) {
    ICZ_REQUIRE(o, "%s: null options", who);
    ICZ_REQUIRE(n >= 1 && n <= 8, "%s: n=%d samples per image outside 1..8", who, n);
    ICZ_REQUIRE(std::isfinite(o->temperature) && o->temperature > 0.f, "%s: temperature %g not positive or not finite", who, (double)o->temperature);
    ICZ_REQUIRE(o->top_k >= 0 && (V < 0 || o->top_k <= V), "%s: top_k %d outside 0..V (%d)", who, o->top_k, V);
    ICZ_REQUIRE(o->top_p > 0.f && o->top_p <= 1.f, "%s: top_p %g outside (0, 1]", who, (double)o->top_p);      // false for NaN
    ICZ_REQUIRE(n_img > 0 && (long)n_img * n <= max_rows, "%s: %d images x %d samples exceed row capacity %d", who, n_img, n, max_rows);
    // a row of V floats beside the histograms in the 160 KB of LDS (the guard scheduled sampling has)
    ICZ_REQUIRE(V < 0 || sizeof(float) * (size_t)V <= 152 * 1024, "%s: a row of %d logits does not fit in LDS", who, V);
    return ICZ_OK;
}

int ensure_sample_buf(DecodeMember* m, int rows, int T) {
    DecodeMember::SampleBuf& b = m->sb;
    if (b.cap_rows >= rows && b.cap_T >= T) return ICZ_OK;
    DeviceBuffers& mem = m->buffers();
    const size_t R_ = rows > m->row_capacity() ? rows : m->row_capacity(), T_ = T > 64 ? T : 64;
    ICZ_TRY(mem.alloc((void**)&b.it, sizeof(int64_t) * R_));
    ICZ_TRY(mem.alloc((void**)&b.fin, R_));
    ICZ_TRY(mem.alloc((void**)&b.n_unf, sizeof(int) * T_));
    ICZ_TRY(mem.alloc((void**)&b.img_of_row, sizeof(int32_t) * R_));
    ICZ_TRY(mem.synced());
    b.cap_rows = (int)R_;
    b.cap_T = (int)T_;
    return ICZ_OK;
}

int sample_decode(DecodeMember* m, const char* who, const float* feats, int n_img, int n, int max_len, const icz_sample_opts* opts,
                  uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, hipStream_t st) {
    // the arguments first: no handle needed to report them (V and the capacity are checked again once there is one)
    ICZ_TRY(check_sample_opts(who, opts, n_img > 0 ? n_img : 1, n, m ? m->vocab() : -1, m ? m->row_capacity() : 0x7fffffff));
    ICZ_REQUIRE(feats && ids_out && logp_out && score_out, "%s: null argument", who);
    ICZ_REQUIRE(m, "%s: null handle", who);
    ICZ_REQUIRE(n_img > 0 && max_len >= 1 && max_len <= 256, "%s: n_img / max_len out of range", who);
    ICZ_REQUIRE(m->refreshed(), "%s: call icz_*_refresh_weights after binding/updating parameters", who);
    const int rows = n_img * n;
    ICZ_TRY(ensure_sample_buf(m, rows, max_len));
    const DecodeMember::SampleBuf& b = m->sb;
    launch_sample_decode_init(b.it, b.fin, b.img_of_row, rows, n, b.n_unf, max_len, st);
    const int32_t* const img_of_row = n > 1 ? b.img_of_row : nullptr;      // one row per image: row i is image i
    ICZ_TRY(m->prologue(feats, n_img, n, img_of_row, st));
    const DecodeMember::EmbSlot es = m->emb_slot();
    SampleDecArgs a = {};
    a.V = m->vocab(); a.temperature = opts->temperature; a.top_k = opts->top_k; a.top_p = opts->top_p;
    a.seed = seed; a.T = max_len;
    a.fin = b.fin; a.n_unf = b.n_unf;
    a.ids_out = ids_out; a.logp_out = logp_out; a.score_out = score_out; a.it_next = b.it;
    a.emb_table = es.table; a.emb_next = es.emb; a.E = es.E; a.relu = es.relu;
    int cur = 0, status = ICZ_OK;
    for (int t = 0; t < max_len && status == ICZ_OK; ++t) {
        m->seam_emb_ready = t > 0;                                  // written by the previous step's sample_decode_kernel
        m->seam_live = t > 0 ? b.n_unf + (t - 1) : nullptr;
        status = m->step(rows, b.it, img_of_row, 1, cur, true, &a.lv, st);
        m->seam_emb_ready = false;
        m->seam_live = nullptr;
        if (status != ICZ_OK) break;
        a.t = t;
        a.uniforms = uniforms ? uniforms + (size_t)t * rows : nullptr;
        status = launch_sample_decode(a, rows, st);
        cur ^= 1;
    }
    ICZ_TRY(status);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // namespace icz

// ================================================================================================
using namespace icz;
extern "C" {

int icz_sample_decode_check(const icz_sample_opts* opts, int32_t n_img, int32_t n, int32_t V, int32_t max_rows) {
    return check_sample_opts("icz_sample_decode_check", opts, n_img, n, V, max_rows);
}

int icz_butd_sample_decode(icz_butd_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, const icz_sample_opts* opts,
                           uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, void* stream) {
    return sample_decode(h ? butd_member(h) : nullptr, "icz_butd_sample_decode", feats, n_img, n, max_len, opts, seed, uniforms, ids_out, logp_out,
                         score_out, (hipStream_t)stream);
}
int icz_aoa_sample_decode(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, const icz_sample_opts* opts,
                          uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, void* stream) {
    return sample_decode(h ? aoa_member(h) : nullptr, "icz_aoa_sample_decode", feats, n_img, n, max_len, opts, seed, uniforms, ids_out, logp_out,
                         score_out, (hipStream_t)stream);
}
int icz_nic_sample_decode(icz_nic_t* h, const float* features, int32_t n_img, int32_t n, int32_t max_len, const icz_sample_opts* opts,
                          uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, void* stream) {
    return sample_decode(h ? nic_member(h) : nullptr, "icz_nic_sample_decode", features, n_img, n, max_len, opts, seed, uniforms, ids_out, logp_out,
                         score_out, (hipStream_t)stream);
}

int icz_sample_filter_draw(const float* logits, const float* bias, int32_t nsplit, int32_t ld, int32_t rows, int32_t V,
                           const icz_sample_opts* opts, const float* uniforms, int64_t* tok_out, float* logp_out, uint8_t* keep_out,
                           void* stream) {
    const char* who = "icz_sample_filter_draw";
    ICZ_TRY(check_sample_opts(who, opts, 1, 1, V > 0 ? V : 0, 1));
    ICZ_REQUIRE(logits && uniforms && tok_out && logp_out && rows > 0 && V > 0 && ld >= V && nsplit >= 1, "%s: bad arguments", who);
    ICZ_REQUIRE(nsplit == 1 || bias, "%s: split-K slabs need a bias", who);
    SampleDecArgs a = {};
    a.lv = LogitsView{logits, nsplit > 1 ? bias : nullptr, (size_t)rows * ld, ld, nsplit};
    a.V = V; a.temperature = opts->temperature; a.top_k = opts->top_k; a.top_p = opts->top_p;
    a.uniforms = uniforms; a.T = 1;
    a.ids_out = tok_out; a.logp_out = logp_out; a.keep_out = keep_out;
    ICZ_TRY(launch_sample_decode(a, rows, (hipStream_t)stream));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
