// Model ensembles (beyond the reference; self-critical.pytorch's AttEnsemble): M = 1..4 BUTD / AoA / NIC decoder handles of one
// vocabulary decode together.  Every step each member runs its own step (DecodeMember, decoder_core.h) on the shared tokens, then
// ensemble_logprob_kernel combines the members' logits into lp[v] = log(sum_m w_m softmax(logits_m)[v]): greedy takes its argmax in
// the same launch, beam search hands the rows to the shared driver (beam_search, beam.hip) with every option it has, and the
// sampling decode draws from lp in the ensemble instance of sample_decode_kernel (sample_decode.hip), which combines in its pass 1.
// Given captions are scored by the ensemble instance of score_tokens_kernel (score_captions.hip), which never forms lp.
#include <cmath>

#include "ens_sample.h"
#include "support_kernels.h"
#include "token_kernels.h"

namespace icz {

// One workgroup (four waves) per row.  Pass 1: lse_m of every member in one online max / sum-exp pass over its logits (read
// straight from the member's finished row or its split-K slabs + bias).  Pass 2: lp[v] = log(sum_m w_m exp(x_m[v] - lse_m)), shifted
// by the largest term over m.  GREEDY: lp is not stored; its argmax (ties to the lowest index, as torch.max) becomes the row's next
// token it_next[row] and ids_out[row, t].
template <bool GREEDY>
__global__ __launch_bounds__(256) void ensemble_logprob_kernel(EnsArgs a, float* __restrict__ out, int ldo, int64_t* __restrict__ it_next,
                                                               int64_t* __restrict__ ids_out, int ids_stride, int t) {
    __shared__ float sm[4], ss[4];
    __shared__ float sv[4];
    __shared__ int si[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = a.V;
    float shift[ENS_MAX_M];           // log w_m - lse_m
    bool vec[ENS_MAX_M];
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) {
        shift[m] = -INFINITY;
        vec[m] = false;
        if (m >= a.M) continue;
        const LogitsView l = a.m[m];
        vec[m] = ens_vec_ok(l);
        float mx = -INFINITY, s = 0.f;
        for (int v = tid * 4; v < V; v += 1024) {
            const f32x4 x = ens_load4(l, row, v, V, vec[m]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float y = x[j];
                if (y > mx) { s = s * expf(mx - y) + 1.f; mx = y; }
                else if (y != -INFINITY) s += expf(y - mx);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lse_combine(mx, s, __shfl_xor(mx, o, 64), __shfl_xor(s, o, 64));
        if (lane == 0) { sm[wave] = mx; ss[wave] = s; }
        __syncthreads();
        mx = sm[0]; s = ss[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) lse_combine(mx, s, sm[w], ss[w]);
        __syncthreads();              // sm / ss are rewritten by the next member
        shift[m] = a.logw[m] - (mx + logf(s));
    }
    float* o_row = out ? out + (size_t)row * ldo : nullptr;
    const bool ovec = !GREEDY && ((ldo & 3) == 0) && (((uintptr_t)out & 15) == 0);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = tid * 4; v < V; v += 1024) {
        f32x4 term[ENS_MAX_M];
        f32x4 top = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m) {
            if (m >= a.M) continue;
            term[m] = ens_load4(a.m[m], row, v, V, vec[m]) + shift[m];
#pragma unroll
            for (int j = 0; j < 4; ++j) top[j] = fmaxf(top[j], term[m][j]);
        }
        f32x4 lp;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < ENS_MAX_M; ++m)
                if (m < a.M && term[m][j] != -INFINITY) s += expf(term[m][j] - top[j]);
            lp[j] = top[j] == -INFINITY ? -INFINITY : top[j] + logf(s);
        }
        if (GREEDY) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v + j < V && lp[j] > best) { best = lp[j]; bi = v + j; }
        } else if (ovec && v + 4 <= V) {
            *reinterpret_cast<f32x4*>(o_row + v) = lp;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v + j < V) o_row[v + j] = lp[j];
        }
    }
    if (GREEDY) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) argmax_combine(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
        if (lane == 0) { sv[wave] = best; si[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            best = sv[0]; bi = si[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) argmax_combine(best, bi, sv[w], si[w]);
            if ((unsigned)bi >= (unsigned)V) bi = 0;       // a row of NaN / -inf log-probs never updates bi: <pad>, not a wild id
            it_next[row] = bi;
            if (ids_out) ids_out[(size_t)row * ids_stride + t] = bi;
        }
    }
}

// weights: null = uniform; else finite, >= 0, sum > 0 -> log of the normalised weights
int ens_log_weights(const char* who, const float* weights, int M, float* logw) {
    double sum = 0.0;
    for (int i = 0; i < M; ++i) {
        const double w = weights ? (double)weights[i] : 1.0;
        ICZ_REQUIRE(std::isfinite(w) && w >= 0.0, "%s: weight %d (%g) negative or not finite", who, i, w);
        sum += w;
    }
    ICZ_REQUIRE(sum > 0.0, "%s: the weights sum to 0", who);
    for (int i = 0; i < M; ++i) {
        const double w = weights ? (double)weights[i] : 1.0;
        logw[i] = w > 0.0 ? (float)std::log(w / sum) : -INFINITY;
    }
    return ICZ_OK;
}

static void launch_combine(const EnsArgs& a, int rows, float* out, int ldo, int64_t* it_next, int64_t* ids_out, int ids_stride, int t,
                           hipStream_t st) {
    if (it_next)
        hipLaunchKernelGGL(ensemble_logprob_kernel<true>, dim3(rows), dim3(256), 0, st, a, (float*)nullptr, 0, it_next, ids_out, ids_stride, t);
    else
        hipLaunchKernelGGL(ensemble_logprob_kernel<false>, dim3(rows), dim3(256), 0, st, a, out, ldo, (int64_t*)nullptr, (int64_t*)nullptr, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// The ensemble: owns the greedy and sampling loops' tokens `it`, its beam buffers, the combined rows lp [rows, Vp] and the sampling
// decode's finished flags, per-step counts of unfinished rows and image of each row; the members stay the caller's.
constexpr int ENS_MAX_T = 256;        // steps of a sampling decode (the single-model driver's limit)
struct Ensemble {
    int M = 0, V = 0, Vp = 0, cap = 0;
    DecodeMember* m[ENS_MAX_M] = {};
    const char* family[ENS_MAX_M] = {};      // "butd" / "aoa" / "nic": names a member in the errors of a search it runs on its own
    float logw[ENS_MAX_M] = {};
    DeviceBuffers mem;
    BeamBuf bm;
    SbsBuf sbs;
    int64_t* it = nullptr;
    float* lp = nullptr;
    uint8_t* fin = nullptr;
    int* n_unf = nullptr;
    int32_t* img_of_row = nullptr;

    int init(const int32_t* kinds, void* const* members, const float* weights, int n);
    EnsArgs args(const LogitsView* lv) const {
        EnsArgs a = {};
        for (int i = 0; i < M; ++i) { a.m[i] = lv[i]; a.logw[i] = logw[i]; }
        a.M = M; a.V = V;
        return a;
    }
    int greedy(const float* const* feats, int B, int max_len, int64_t* ids_out, hipStream_t st);
    int sample_decode(const char* who, const float* const* feats, int n_img, int n, int max_len, const icz_sample_opts* opts, uint64_t seed,
                      const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, hipStream_t st);
    int score_captions(const char* who, const float* const* feats, int n_img, int n, int max_len, const int64_t* ids, float* logp_out,
                       float* score_out, hipStream_t st);
};

int Ensemble::init(const int32_t* kinds, void* const* members, const float* weights, int n) {
    const char* who = "icz_ensemble_create";
    ICZ_REQUIRE(n >= 1 && n <= ENS_MAX_M, "%s: %d members outside 1..%d", who, n, ENS_MAX_M);
    ICZ_REQUIRE(kinds && members, "%s: null argument", who);
    for (int i = 0; i < n; ++i) {
        ICZ_REQUIRE(kinds[i] >= ICZ_MEMBER_BUTD && kinds[i] <= ICZ_MEMBER_NIC, "%s: member %d has unknown kind %d (0 BUTD, 1 AoA, 2 NIC)", who, i,
                    kinds[i]);
        ICZ_REQUIRE(members[i], "%s: member %d is null", who, i);
        for (int j = 0; j < i; ++j)
            ICZ_REQUIRE(members[j] != members[i], "%s: members %d and %d are one handle (its decoder state cannot serve two members)", who, j, i);
    }
    ICZ_TRY(ens_log_weights(who, weights, n, logw));
    for (int i = 0; i < n; ++i)
        m[i] = kinds[i] == ICZ_MEMBER_BUTD ? butd_member(members[i]) : kinds[i] == ICZ_MEMBER_AOA ? aoa_member(members[i]) : nic_member(members[i]);
    for (int i = 0; i < n; ++i) family[i] = kinds[i] == ICZ_MEMBER_BUTD ? "butd" : kinds[i] == ICZ_MEMBER_AOA ? "aoa" : "nic";
    V = m[0]->vocab();
    cap = m[0]->row_capacity();
    for (int i = 1; i < n; ++i) {
        ICZ_REQUIRE(m[i]->vocab() == V, "%s: member %d has vocabulary %d, member 0 has %d", who, i, m[i]->vocab(), V);
        if (m[i]->row_capacity() < cap) cap = m[i]->row_capacity();
    }
    M = n;
    Vp = pad_vocab(V);
    ICZ_TRY(mem.alloc((void**)&it, sizeof(int64_t) * cap));
    ICZ_TRY(mem.alloc((void**)&lp, sizeof(float) * (size_t)cap * Vp));
    ICZ_TRY(mem.alloc((void**)&fin, cap));
    ICZ_TRY(mem.alloc((void**)&n_unf, sizeof(int) * ENS_MAX_T));
    ICZ_TRY(mem.alloc((void**)&img_of_row, sizeof(int32_t) * cap));
    return mem.synced();
}

// one row per image for max_len steps, no early stop (the reference's sample)
int Ensemble::greedy(const float* const* feats, int B, int max_len, int64_t* ids_out, hipStream_t st) {
    const char* who = "icz_ensemble_greedy";
    ICZ_REQUIRE(ids_out && B > 0 && max_len > 0, "%s: bad arguments", who);
    ICZ_TRY(check_members(who, m, M, feats, B));
    for (int i = 0; i < M; ++i) ICZ_TRY(m[i]->prologue(feats[i], B, 1, nullptr, st));
    hipLaunchKernelGGL(fill_i64_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, it, (int64_t)1, B);       // <sta>
    LogitsView lv[ENS_MAX_M];
    int cur = 0;
    for (int t = 0; t < max_len; ++t) {
        for (int i = 0; i < M; ++i) ICZ_TRY(m[i]->step(B, it, nullptr, 1, cur, true, &lv[i], st));
        launch_combine(args(lv), B, nullptr, 0, it, ids_out, max_len, t, st);
        cur ^= 1;
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// The sampling decode (sample_decode(), sample_decode.hip, over M members): row img * n + j is sample j of image img; every member
// runs its prologue once per image and its step over all rows on the shared tokens, then ONE launch of sample_decode_kernel's
// ensemble instance combines the members' logits, filters, draws and writes every member's next input embedding.  The caller
// (icz_ensemble_sample_decode) has checked the options and the null arguments.
int Ensemble::sample_decode(const char* who, const float* const* feats, int n_img, int n, int max_len, const icz_sample_opts* opts,
                            uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, hipStream_t st) {
    ICZ_REQUIRE(n_img > 0 && max_len >= 1 && max_len <= ENS_MAX_T, "%s: n_img / max_len out of range", who);
    ICZ_REQUIRE((long)n_img * n <= cap, "%s: %d images x %d samples exceed row capacity %d (the smallest member's)", who, n_img, n, cap);
    const int rows = n_img * n;
    ICZ_TRY(check_members(who, m, M, feats, rows));
    launch_sample_decode_init(it, fin, img_of_row, rows, n, n_unf, max_len, st);
    const int32_t* const rows_img = n > 1 ? img_of_row : nullptr;        // one row per image: row i is image i
    for (int i = 0; i < M; ++i) ICZ_TRY(m[i]->prologue(feats[i], n_img, n, rows_img, st));
    EnsSampleDecArgs a = {};
    a.s.V = V; a.s.temperature = opts->temperature; a.s.top_k = opts->top_k; a.s.top_p = opts->top_p;
    a.s.seed = seed; a.s.T = max_len;
    a.s.fin = fin; a.s.n_unf = n_unf;
    a.s.ids_out = ids_out; a.s.logp_out = logp_out; a.s.score_out = score_out; a.s.it_next = it;
    for (int i = 0; i < M; ++i) a.emb[i] = m[i]->emb_slot();
    LogitsView lv[ENS_MAX_M];
    int cur = 0, status = ICZ_OK;
    for (int t = 0; t < max_len && status == ICZ_OK; ++t) {
        for (int i = 0; i < M && status == ICZ_OK; ++i) {
            m[i]->seam_emb_ready = t > 0;                               // written by the previous step's sample_decode_kernel
            m[i]->seam_live = t > 0 ? n_unf + (t - 1) : nullptr;
            status = m[i]->step(rows, it, rows_img, 1, cur, true, &lv[i], st);
            m[i]->seam_emb_ready = false;
            m[i]->seam_live = nullptr;
        }
        if (status != ICZ_OK) break;
        a.ens = args(lv);
        a.s.t = t;
        a.s.uniforms = uniforms ? uniforms + (size_t)t * rows : nullptr;
        status = launch_sample_decode(a, rows, st);
        cur ^= 1;
    }
    ICZ_TRY(status);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// Scoring given captions (score_captions(), score_captions.hip, over M members): row img * n + j scores caption j of image img;
// every member runs its prologue once per image and its step over all rows on the shared fed tokens, then ONE launch of
// score_tokens_kernel's ensemble instance reads every member's logits once (lse_m and the target's logit; the combined row is never
// formed) and writes every member's next input embedding.  The caller (icz_ensemble_score_captions) has checked the arguments.
int Ensemble::score_captions(const char* who, const float* const* feats, int n_img, int n, int max_len, const int64_t* ids,
                             float* logp_out, float* score_out, hipStream_t st) {
    const int rows = n_img * n;
    ICZ_TRY(check_members(who, m, M, feats, rows));
    launch_score_init(ids, it, fin, img_of_row, rows, n, n_unf, max_len, V, st);
    const int32_t* const rows_img = n > 1 ? img_of_row : nullptr;        // one row per image: row i is image i
    for (int i = 0; i < M; ++i) ICZ_TRY(m[i]->prologue(feats[i], n_img, n, rows_img, st));
    EnsScoreArgs a = {};
    a.s.V = V; a.s.ids = ids; a.s.T = max_len;
    a.s.fin = fin; a.s.n_unf = n_unf;
    a.s.logp_out = logp_out; a.s.score_out = score_out; a.s.it_next = it;
    for (int i = 0; i < M; ++i) a.emb[i] = m[i]->emb_slot();
    LogitsView lv[ENS_MAX_M];
    int cur = 0, status = ICZ_OK;
    for (int t = 0; t < max_len && status == ICZ_OK; ++t) {
        for (int i = 0; i < M && status == ICZ_OK; ++i) {
            m[i]->seam_emb_ready = t > 0;                               // written by the previous step's score_tokens_kernel
            m[i]->seam_live = t > 0 ? n_unf + (t - 1) : nullptr;
            status = m[i]->step(rows, it, rows_img, 1, cur, true, &lv[i], st);
            m[i]->seam_emb_ready = false;
            m[i]->seam_live = nullptr;
        }
        if (status != ICZ_OK) break;
        a.ens = args(lv);
        a.s.t = t;
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

int icz_ensemble_create(const int32_t* kinds, void* const* members, const float* weights, int32_t M, icz_ensemble_t** out) {
    ICZ_REQUIRE(out, "icz_ensemble_create: null argument");
    Ensemble* e = new Ensemble();
    const int s = e->init(kinds, members, weights, M);
    if (s != ICZ_OK) { delete e; return s; }
    *out = reinterpret_cast<icz_ensemble_t*>(e);
    return ICZ_OK;
}

int icz_ensemble_destroy(icz_ensemble_t* h) {
    delete reinterpret_cast<Ensemble*>(h);
    return ICZ_OK;
}

int icz_ensemble_greedy(icz_ensemble_t* h, const float* const* feats, int32_t B, int32_t max_len, int64_t* ids_out, void* stream) {
    ICZ_REQUIRE(h, "icz_ensemble_greedy: null handle");
    return reinterpret_cast<Ensemble*>(h)->greedy(feats, B, max_len, ids_out, (hipStream_t)stream);
}

int icz_ensemble_beam_search_diverse(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                     const icz_beam_opts* opts, const icz_beam_diversity* div, float* seqs_out, int32_t* lens_out,
                                     float* scores_out, void* stream) {
    ICZ_TRY(BeamBuf::check_opts("icz_ensemble_beam_search_diverse", beam, opts));      // the arguments first: no handle needed to report them
    ICZ_TRY(BeamBuf::check_diversity("icz_ensemble_beam_search_diverse", beam, div));
    ICZ_REQUIRE(seqs_out && lens_out && scores_out, "icz_ensemble_beam_search_diverse: null argument");
    ICZ_REQUIRE(h, "icz_ensemble_beam_search_diverse: null handle");
    // the combined rows also for M = 1: the member's logits go through ensemble_logprob_kernel, not straight to the search
    Ensemble* e = reinterpret_cast<Ensemble*>(h);
    hipStream_t st = (hipStream_t)stream;
    const BeamCombine ens = {"icz_ensemble_beam_search_diverse", &e->bm, &e->mem, e->cap, e->lp, e->Vp, [=](const LogitsView* lv, int rows) {
                                 launch_combine(e->args(lv), rows, e->lp, e->Vp, nullptr, nullptr, 0, 0, st);
                             }};
    return beam_search("ensemble", e->m, e->M, &ens, feats, n_img, beam, max_steps, *opts, *div, seqs_out, lens_out, scores_out, st);
}

int icz_ensemble_beam_search_constrained(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t beam, int32_t max_steps,
                                         const icz_beam_opts* opts, const icz_beam_constraints* cons, float* seqs_out, int32_t* lens_out,
                                         float* scores_out, int32_t* sat_out, void* stream) {
    const char* who = "icz_ensemble_beam_search_constrained";
    const icz_beam_constraints* use = nullptr;
    ICZ_TRY(beam_constrained_args(who, n_img, beam, opts, cons, seqs_out && lens_out && scores_out && sat_out, &use));
    ICZ_REQUIRE(h, "%s: null handle", who);
    Ensemble* e = reinterpret_cast<Ensemble*>(h);
    hipStream_t st = (hipStream_t)stream;
    // One member: its weight normalises to 1, so the combined row is its own log-softmax.  The search runs on the member's finished
    // logits as the member's own entry does -- the same launches, so the same bits -- and the combine kernel is not launched.
    if (e->M == 1) {
        ICZ_REQUIRE(feats, "%s: null features", who);
        return beam_search(e->family[0], e->m, 1, nullptr, feats, n_img, beam, max_steps, *opts, BeamBuf::no_diversity, seqs_out, lens_out,
                           scores_out, st, use, sat_out);
    }
    const BeamCombine ens = {who, &e->bm, &e->mem, e->cap, e->lp, e->Vp, [=](const LogitsView* lv, int rows) {
                                 launch_combine(e->args(lv), rows, e->lp, e->Vp, nullptr, nullptr, 0, 0, st);
                             }};
    return beam_search("ensemble", e->m, e->M, &ens, feats, n_img, beam, max_steps, *opts, BeamBuf::no_diversity, seqs_out, lens_out, scores_out, st,
                       use, sat_out);
}

int icz_ensemble_sample_decode(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t n, int32_t max_len,
                               const icz_sample_opts* opts, uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out,
                               float* score_out, void* stream) {
    const char* who = "icz_ensemble_sample_decode";
    Ensemble* e = reinterpret_cast<Ensemble*>(h);
    // the arguments first: no handle needed to report them (the capacity is checked once there is one)
    ICZ_TRY(check_sample_opts(who, opts, n_img > 0 ? n_img : 1, n, e ? e->V : -1, 0x7fffffff));
    ICZ_REQUIRE(feats && ids_out && logp_out && score_out, "%s: null argument", who);
    ICZ_REQUIRE(e, "%s: null handle", who);
    return e->sample_decode(who, feats, n_img, n, max_len, opts, seed, uniforms, ids_out, logp_out, score_out, (hipStream_t)stream);
}

int icz_ensemble_sample_distinct(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t n, int32_t max_len, float temperature,
                                 uint64_t seed, int32_t first_image, const float* uniforms, const float* root_uniforms,
                                 const icz_sample_distinct_out* out, void* stream) {
    const char* who = "icz_ensemble_sample_distinct";
    Ensemble* e = reinterpret_cast<Ensemble*>(h);
    // the arguments first: no handle needed to report them (the vocabulary and the capacity are checked once there is one)
    ICZ_TRY(sample_distinct_check(who, n_img, n, max_len, temperature, e ? e->V : -1, -1, 0));
    ICZ_REQUIRE(feats && out && out->ids && out->lens && out->finished && out->phi && out->g && (uniforms == nullptr) == (root_uniforms == nullptr),
                "%s: null argument (uniforms and root_uniforms: both or neither)", who);
    ICZ_REQUIRE(e, "%s: null handle", who);
    hipStream_t st = (hipStream_t)stream;
    // One member: its weight normalises to 1, so the combined row is its own log-softmax.  The search runs on the member's own
    // logits as the member's entry does -- the same launches, so the same bits -- and the combine kernel is not launched.
    if (e->M == 1) {
        ICZ_REQUIRE(feats[0], "%s: null features of member 0", who);
        return sample_distinct(who, e->m, 1, nullptr, feats, n_img, n, max_len, temperature, seed, first_image, uniforms, root_uniforms, out, st);
    }
    BeamCombine ens = {who, &e->bm, &e->mem, e->cap, e->lp, e->Vp, [=](const LogitsView* lv, int rows) {
                           launch_combine(e->args(lv), rows, e->lp, e->Vp, nullptr, nullptr, 0, 0, st);
                       }};
    ens.sbs = &e->sbs;
    return sample_distinct(who, e->m, e->M, &ens, feats, n_img, n, max_len, temperature, seed, first_image, uniforms, root_uniforms, out, st);
}

int icz_ensemble_score_captions(icz_ensemble_t* h, const float* const* feats, int32_t n_img, int32_t n, int32_t max_len, const int64_t* ids,
                                float* logp_out, float* score_out, void* stream) {
    const char* who = "icz_ensemble_score_captions";
    Ensemble* e = reinterpret_cast<Ensemble*>(h);
    // the arguments first: no handle needed to report them (the capacity, the smallest member's, is checked once there is one)
    ICZ_TRY(check_score_args(who, n_img, n, max_len, e ? e->cap : 0x7fffffff));
    ICZ_REQUIRE(feats && ids && logp_out && score_out, "%s: null argument", who);
    ICZ_REQUIRE(e, "%s: null handle", who);
    return e->score_captions(who, feats, n_img, n, max_len, ids, logp_out, score_out, (hipStream_t)stream);
}

int icz_ensemble_sample_filter_draw(int32_t M, const float* const* logits, const float* const* bias, const int32_t* nsplit,
                                    const int32_t* ld, const float* weights, int32_t rows, int32_t V, const icz_sample_opts* opts,
                                    const float* uniforms, int64_t* tok_out, float* logp_out, uint8_t* keep_out, void* stream) {
    const char* who = "icz_ensemble_sample_filter_draw";
    ICZ_TRY(check_sample_opts(who, opts, 1, 1, V > 0 ? V : 0, 1));
    ICZ_REQUIRE(M >= 1 && M <= ENS_MAX_M, "%s: %d members outside 1..%d", who, M, ENS_MAX_M);
    ICZ_REQUIRE(logits && nsplit && ld && uniforms && tok_out && logp_out && rows > 0 && V > 0, "%s: bad arguments", who);
    EnsSampleDecArgs a = {};
    ICZ_TRY(ens_log_weights(who, weights, M, a.ens.logw));
    for (int i = 0; i < M; ++i) {
        ICZ_REQUIRE(logits[i] && ld[i] >= V && nsplit[i] >= 1, "%s: member %d: null logits, ld < V or nsplit < 1", who, i);
        ICZ_REQUIRE(nsplit[i] == 1 || (bias && bias[i]), "%s: member %d: split-K slabs need a bias", who, i);
        a.ens.m[i] = LogitsView{logits[i], nsplit[i] > 1 ? bias[i] : nullptr, (size_t)rows * ld[i], ld[i], nsplit[i]};
    }
    a.ens.M = M; a.ens.V = V;
    a.s.V = V; a.s.temperature = opts->temperature; a.s.top_k = opts->top_k; a.s.top_p = opts->top_p;
    a.s.uniforms = uniforms; a.s.T = 1;
    a.s.ids_out = tok_out; a.s.logp_out = logp_out; a.s.keep_out = keep_out;
    ICZ_TRY(launch_sample_decode(a, rows, (hipStream_t)stream));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_ensemble_logprob(int32_t M, const float* const* logits, const float* const* bias, const int32_t* nsplit, const int32_t* ld,
                         const float* weights, int32_t rows, int32_t V, float* lp_out, int32_t ldo, int64_t* argmax_out, void* stream) {
    const char* who = "icz_ensemble_logprob";
    ICZ_REQUIRE(M >= 1 && M <= ENS_MAX_M, "%s: %d members outside 1..%d", who, M, ENS_MAX_M);
    ICZ_REQUIRE(logits && nsplit && ld && rows > 0 && V > 0, "%s: bad arguments", who);
    ICZ_REQUIRE(argmax_out || (lp_out && ldo >= V), "%s: no output (lp_out with ldo >= V, or argmax_out)", who);
    EnsArgs a = {};
    ICZ_TRY(ens_log_weights(who, weights, M, a.logw));
    for (int i = 0; i < M; ++i) {
        ICZ_REQUIRE(logits[i] && ld[i] >= V && nsplit[i] >= 1, "%s: member %d: null logits, ld < V or nsplit < 1", who, i);
        ICZ_REQUIRE(nsplit[i] == 1 || (bias && bias[i]), "%s: member %d: split-K slabs need a bias", who, i);
        a.m[i] = LogitsView{logits[i], nsplit[i] > 1 ? bias[i] : nullptr, (size_t)rows * ld[i], ld[i], nsplit[i]};
    }
    a.M = M; a.V = V;
    launch_combine(a, rows, lp_out, ldo, argmax_out, nullptr, 0, 0, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
