// Scoring given captions (beyond the reference; include/icz.h: icz_*_score_captions): the log-probability a decoder, or a model
// ensemble, assigns to captions it is handed -- teacher forcing in evaluation mode.  A driver on the decoder seams (DecodeMember,
// decoder_core.h) shaped as the sampling decode (sample_decode.hip): one prologue per image, the rows reached through img_of_row,
// then per step the member's own decoder step on the fed tokens and ONE launch of score_tokens_kernel, which reports the fed
// token's log-probability, keeps the finished flags and the count of unfinished rows (the early-out) and writes the next step's
// input embedding.  The ensemble's driver (Ensemble::score_captions, ensemble.hip) runs the kernel's second instance.
#include <cmath>
#include <type_traits>

#include "ens_sample.h"

namespace icz {

constexpr int SC_THREADS = 512;               // 8 waves per row: at V = 10 102 five 16-byte loads per thread and slab, all in flight at once
constexpr int SC_NW = SC_THREADS / 64;

// running (max, sum of exp(x - max)) pairs as lse_combine (ens_sample.h) keeps them, the sum in float64
__device__ __forceinline__ void sc_combine(float& m, double& s, float om, double os) {
    const float n = fmaxf(m, om);
    if (n == -INFINITY) return;
    s = s * (double)expf(m - n) + os * (double)expf(om - n);
    m = n;
}

__device__ __forceinline__ const ScoreArgs& sc_args(const ScoreArgs& a) { return a; }
__device__ __forceinline__ const ScoreArgs& sc_args(const EnsScoreArgs& a) { return a.s; }

// emb_next[row, :E] = table[tok] (relu: behind a ReLU)
__device__ __forceinline__ void sc_write_emb(const float* table, float* emb_next, int E, int relu, int row, int tok) {
    for (int e = threadIdx.x * 4; e < E; e += 4 * SC_THREADS) {
        f32x4 x = *reinterpret_cast<const f32x4*>(table + (size_t)tok * E + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = relu ? fmaxf(x[j], 0.f) : x[j];
        *reinterpret_cast<f32x4*>(emb_next + (size_t)row * E + e) = x;
    }
}
template <class A>
__device__ __forceinline__ void sc_next_emb(const A& args, int row, int tok) {
    if constexpr (std::is_same_v<A, EnsScoreArgs>) {
        for (int m = 0; m < args.ens.M; ++m) {
            const DecodeMember::EmbSlot& s = args.emb[m];
            if (s.emb) sc_write_emb(s.table, s.emb, s.E, s.relu, row, tok);
        }
    } else {
        if (args.emb_next) sc_write_emb(args.emb_table, args.emb_next, args.E, args.relu, row, tok);
    }
}

// One workgroup of 8 waves per row; nothing of the row is kept: V is not bounded by LDS.  Per member ONE pass over its finished
// logits (the predict GEMM's split-K slabs summed in slab order + bias, ens_load4): an online max / sum-exp (fp32 terms, float64
// sums) while the thread that meets the target keeps its logit; the partial pairs meet in one fixed order (lanes by xor distance,
// then the waves 0..7).  Then log_softmax(x)[target] = (x[target] - max) - log(sum), or for an ensemble
// log(sum_m exp(log w_m + x_m[target] - lse_m)) shifted by the largest term -- the combined row is never formed, and a member of
// weight 0 is not read.  The tail writes logp and the running score, looks one token ahead for the row's finished flag (the target was <end>, the last column, or the
// next id is 0 or outside [0, V)), counts the unfinished rows of step t and writes the next step's input embedding of the fed
// token.  Rows past their length write zeros and the <pad> embedding; once no row is unfinished the launch returns at entry.
// Two instances, one per row source (A): ScoreArgs reads a LogitsView, EnsScoreArgs the members of an EnsArgs.
template <class A>
__global__ __launch_bounds__(SC_THREADS) void score_tokens_kernel(A args) {
    constexpr bool ENS = std::is_same_v<A, EnsScoreArgs>;
    const ScoreArgs& a = sc_args(args);
    __shared__ float smx[SC_NW];
    __shared__ double ssum[SC_NW];
    __shared__ float sx[ENS_MAX_M];           // the target's logit of every member
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = a.V;
    const size_t o = (size_t)row * a.T + a.t;
    const bool all_dead = a.n_unf && a.t > 0 && a.n_unf[a.t - 1] == 0;      // the kernels of this step returned at entry (step_dead)
    const bool was_fin = a.fin && a.fin[row] != 0;
    const int64_t c = (all_dead || was_fin) ? 0 : a.ids[o];
    const bool valid = c >= 0 && c < (int64_t)V;                            // the drivers never leave a row live on such an id
    if (all_dead || was_fin || !valid) {
        if (tid == 0) {
            a.logp_out[o] = 0.f;
            if (a.score_out && a.t == 0) a.score_out[row] = 0.f;
            if (a.it_next) a.it_next[row] = 0;
            if (a.fin) a.fin[row] = 1;
        }
        if (!all_dead) sc_next_emb(args, row, 0);       // the others go on: this row keeps running on <pad> (finite, never read)
        return;
    }
    const int tok = (int)c;
    int M = 1;
    if constexpr (ENS) M = args.ens.M;
    double term[ENS_MAX_M];                   // x_m[tok] - lse_m
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) {
        term[m] = 0.0;
        if (m >= M) continue;
        const LogitsView* lp = &a.lv;
        if constexpr (ENS) {
            lp = &args.ens.m[m];
            if (args.ens.logw[m] == -INFINITY) { term[m] = -INFINITY; continue; }      // a zero weight: the member's logits are not read
        }
        const LogitsView& l = *lp;
        const bool vec = ens_vec_ok(l);
        float mm = -INFINITY;
        double s = 0.0;
        for (int v = tid * 4; v < V; v += 4 * SC_THREADS) {
            const f32x4 x = ens_load4(l, row, v, V, vec);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float y = x[j];
                if (v + j == tok) sx[m] = y;
                if (y > mm) { s = s * (double)expf(mm - y) + 1.0; mm = y; }
                else if (y != -INFINITY) s += (double)expf(y - mm);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sc_combine(mm, s, __shfl_xor(mm, off, 64), __shfl_xor(s, off, 64));
        if (lane == 0) { smx[wave] = mm; ssum[wave] = s; }
        __syncthreads();
        mm = smx[0]; s = ssum[0];
        for (int w = 1; w < SC_NW; ++w) sc_combine(mm, s, smx[w], ssum[w]);      // one fixed order
        term[m] = (double)(sx[m] - mm) - log(s);
        __syncthreads();                      // smx / ssum are rewritten by the next member
    }
    float lp;
    if constexpr (ENS) {
        double top = -INFINITY, sum = 0.0;
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m)
            if (m < M) { term[m] += (double)args.ens.logw[m]; top = fmax(top, term[m]); }
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m)
            if (m < M && term[m] != -INFINITY) sum += exp(term[m] - top);
        lp = top == -INFINITY ? -INFINITY : (float)(top + log(sum));
    } else {
        lp = (float)term[0];
    }
    bool done = true;                         // the kernel alone: one target per row
    if (a.fin) {
        done = tok == 2 || a.t + 1 >= a.T;
        if (!done) {
            const int64_t nx = a.ids[o + 1];
            done = nx <= 0 || nx >= (int64_t)V;
        }
    }
    const int nxt = done ? 0 : tok;
    if (tid == 0) {
        a.logp_out[o] = lp;
        if (a.score_out) a.score_out[row] = a.t == 0 ? lp : a.score_out[row] + lp;
        if (a.it_next) a.it_next[row] = nxt;
        if (a.fin) a.fin[row] = done ? 1 : 0;
        if (a.n_unf && !done) atomicAdd(&a.n_unf[a.t], 1);
    }
    sc_next_emb(args, row, nxt);
}

// start of a scoring pass: <sta>, a row whose first token is 0 or outside [0, V) has nothing to score, row r belongs to image r / n,
// the per-step counters of unfinished rows = 0
__global__ void score_init_kernel(const int64_t* ids, int64_t* it, uint8_t* fin, int32_t* img_of_row, int rows, int n, int* n_unf, int T,
                                  int V) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) {
        const int64_t c = ids[(size_t)i * T];
        it[i] = 1;
        fin[i] = (c <= 0 || c >= (int64_t)V) ? 1 : 0;
        img_of_row[i] = i / n;
    }
    if (i < T) n_unf[i] = 0;
}

void launch_score_init(const int64_t* ids, int64_t* it, uint8_t* fin, int32_t* img_of_row, int rows, int n, int* n_unf, int T, int V,
                       hipStream_t st) {
    hipLaunchKernelGGL(score_init_kernel, dim3(cdiv(rows > T ? rows : T, 256)), dim3(256), 0, st, ids, it, fin, img_of_row, rows, n, n_unf, T, V);
}
void launch_score_tokens(const ScoreArgs& a, int rows, hipStream_t st) {
    hipLaunchKernelGGL(score_tokens_kernel<ScoreArgs>, dim3(rows), dim3(SC_THREADS), 0, st, a);
}
void launch_score_tokens(const EnsScoreArgs& a, int rows, hipStream_t st) {
    hipLaunchKernelGGL(score_tokens_kernel<EnsScoreArgs>, dim3(rows), dim3(SC_THREADS), 0, st, a);
}

int check_score_args(const char* who, int n_img, int n, int max_len, int max_rows) {
    ICZ_REQUIRE(n >= 1 && n <= 8, "%s: n=%d captions per image outside 1..8", who, n);
    ICZ_REQUIRE(max_len >= 1 && max_len <= 256, "%s: max_len=%d outside 1..256", who, max_len);
    ICZ_REQUIRE(n_img > 0 && (long)n_img * n <= max_rows, "%s: %d images x %d captions exceed row capacity %d", who, n_img, n, max_rows);
    return ICZ_OK;
}

int score_captions(DecodeMember* m, const char* who, const float* feats, int n_img, int n, int max_len, const int64_t* ids,
                   float* logp_out, float* score_out, hipStream_t st) {
    // the arguments first: no handle needed to report them (the capacity is checked once there is one)
    ICZ_TRY(check_score_args(who, n_img, n, max_len, m ? m->row_capacity() : 0x7fffffff));
    ICZ_REQUIRE(feats && ids && logp_out && score_out, "%s: null argument", who);
    ICZ_REQUIRE(m, "%s: null handle", who);
    ICZ_REQUIRE(m->refreshed(), "%s: call icz_*_refresh_weights after binding/updating parameters", who);
    const int rows = n_img * n;
    ICZ_TRY(ensure_sample_buf(m, rows, max_len));
    const DecodeMember::SampleBuf& b = m->sb;
    launch_score_init(ids, b.it, b.fin, b.img_of_row, rows, n, b.n_unf, max_len, m->vocab(), st);
    const int32_t* const img_of_row = n > 1 ? b.img_of_row : nullptr;      // one row per image: row i is image i
    ICZ_TRY(m->prologue(feats, n_img, n, img_of_row, st));
    const DecodeMember::EmbSlot es = m->emb_slot();
    ScoreArgs a = {};
    a.V = m->vocab(); a.ids = ids; a.T = max_len;
    a.fin = b.fin; a.n_unf = b.n_unf;
    a.logp_out = logp_out; a.score_out = score_out; a.it_next = b.it;
    a.emb_table = es.table; a.emb_next = es.emb; a.E = es.E; a.relu = es.relu;
    int cur = 0, status = ICZ_OK;
    for (int t = 0; t < max_len && status == ICZ_OK; ++t) {
        m->seam_emb_ready = t > 0;                                  // written by the previous step's score_tokens_kernel
        m->seam_live = t > 0 ? b.n_unf + (t - 1) : nullptr;
        status = m->step(rows, b.it, img_of_row, 1, cur, true, &a.lv, st);
        m->seam_emb_ready = false;
        m->seam_live = nullptr;
        if (status != ICZ_OK) break;
        a.t = t;
        launch_score_tokens(a, rows, st);
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

int icz_score_captions_check(int32_t n_img, int32_t n, int32_t max_len, int32_t max_rows) {
    return check_score_args("icz_score_captions_check", n_img, n, max_len, max_rows);
}

int icz_butd_score_captions(icz_butd_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, const int64_t* ids,
                            float* logp_out, float* score_out, void* stream) {
    return score_captions(h ? butd_member(h) : nullptr, "icz_butd_score_captions", feats, n_img, n, max_len, ids, logp_out, score_out,
                          (hipStream_t)stream);
}
int icz_aoa_score_captions(icz_aoa_t* h, const float* feats, int32_t n_img, int32_t n, int32_t max_len, const int64_t* ids, float* logp_out,
                           float* score_out, void* stream) {
    return score_captions(h ? aoa_member(h) : nullptr, "icz_aoa_score_captions", feats, n_img, n, max_len, ids, logp_out, score_out,
                          (hipStream_t)stream);
}
int icz_nic_score_captions(icz_nic_t* h, const float* features, int32_t n_img, int32_t n, int32_t max_len, const int64_t* ids,
                           float* logp_out, float* score_out, void* stream) {
    return score_captions(h ? nic_member(h) : nullptr, "icz_nic_score_captions", features, n_img, n, max_len, ids, logp_out, score_out,
                          (hipStream_t)stream);
}

int icz_score_tokens(const float* logits, const float* bias, int32_t nsplit, int32_t ld, int32_t rows, int32_t V, const int64_t* targets,
                     float* logp_out, void* stream) {
    const char* who = "icz_score_tokens";
    ICZ_REQUIRE(logits && targets && logp_out && rows > 0 && V > 0 && ld >= V && nsplit >= 1, "%s: bad arguments", who);
    ICZ_REQUIRE(nsplit == 1 || bias, "%s: split-K slabs need a bias", who);
    ScoreArgs a = {};
    a.lv = LogitsView{logits, nsplit > 1 ? bias : nullptr, (size_t)rows * ld, ld, nsplit};
    a.V = V; a.ids = targets; a.T = 1;
    a.logp_out = logp_out;
    launch_score_tokens(a, rows, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_ensemble_score_tokens(int32_t M, const float* const* logits, const float* const* bias, const int32_t* nsplit, const int32_t* ld,
                              const float* weights, int32_t rows, int32_t V, const int64_t* targets, float* logp_out, void* stream) {
    const char* who = "icz_ensemble_score_tokens";
    ICZ_REQUIRE(M >= 1 && M <= ENS_MAX_M, "%s: %d members outside 1..%d", who, M, ENS_MAX_M);
    ICZ_REQUIRE(logits && nsplit && ld && targets && logp_out && rows > 0 && V > 0, "%s: bad arguments", who);
    EnsScoreArgs a = {};
    ICZ_TRY(ens_log_weights(who, weights, M, a.ens.logw));
    for (int i = 0; i < M; ++i) {
        ICZ_REQUIRE(logits[i] && ld[i] >= V && nsplit[i] >= 1, "%s: member %d: null logits, ld < V or nsplit < 1", who, i);
        ICZ_REQUIRE(nsplit[i] == 1 || (bias && bias[i]), "%s: member %d: split-K slabs need a bias", who, i);
        a.ens.m[i] = LogitsView{logits[i], nsplit[i] > 1 ? bias[i] : nullptr, (size_t)rows * ld[i], ld[i], nsplit[i]};
    }
    a.ens.M = M; a.ens.V = V;
    a.s.V = V; a.s.ids = targets; a.s.T = 1;
    a.s.logp_out = logp_out;
    launch_score_tokens(a, rows, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
