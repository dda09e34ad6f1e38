// What ensemble.hip, sample_decode.hip, score_captions.hip and distill.hip share: the ensemble's view of its members' logits with the device
// helpers that read and reduce them (ensemble_logprob_kernel and the ensemble instances of sample_decode_kernel and
// score_tokens_kernel), and the arguments / launchers of those two kernels that the ensemble's drivers (Ensemble::sample_decode,
// Ensemble::score_captions) need.
#pragma once
#include "decoder_core.h"

namespace icz {

struct EnsArgs {
    LogitsView m[ENS_MAX_M];
    float logw[ENS_MAX_M];            // log of the normalised weights (-inf for a zero weight)
    int M, V;
};

__device__ __forceinline__ bool ens_vec_ok(const LogitsView& l) {
    return ((l.ld | (int)(l.slab_stride & 3)) & 3) == 0 && (((uintptr_t)l.p | (uintptr_t)l.bias) & 15) == 0;
}

// logits v .. v + 3 of `row` (v % 4 == 0), the slabs summed in slab order then the bias; columns >= V read as -inf
__device__ __forceinline__ f32x4 ens_load4(const LogitsView& l, int row, int v, int V, bool vec) {
    const float* r = l.p + (size_t)row * l.ld;
    f32x4 x;
    if (vec && v + 4 <= V) {
        x = *reinterpret_cast<const f32x4*>(r + v);
        for (int z = 1; z < l.ns; ++z) x += *reinterpret_cast<const f32x4*>(r + (size_t)z * l.slab_stride + v);
        if (l.ns > 1) x += *reinterpret_cast<const f32x4*>(l.bias + v);
        return x;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float y = -INFINITY;
        if (v + j < V) {
            y = r[v + j];
            for (int z = 1; z < l.ns; ++z) y += r[(size_t)z * l.slab_stride + v + j];
            if (l.ns > 1) y += l.bias[v + j];
        }
        x[j] = y;
    }
    return x;
}

// running (max, sum of exp(x - max)) pairs
__device__ __forceinline__ void lse_combine(float& m, float& s, float om, float os) {
    const float n = fmaxf(m, om);
    if (n == -INFINITY) return;
    s = s * expf(m - n) + os * expf(om - n);
    m = n;
}

// ---- sample_decode_kernel (sample_decode.hip) ----
struct SampleDecArgs {
    LogitsView lv; int V;             // lv: the single-model instance's row source (the ensemble instance reads EnsSampleDecArgs::ens)
    float temperature; int top_k; float top_p;
    const float* uniforms;            // [rows] of this step, or null: Philox (seed, t, row) under RNG_DECODE
    uint64_t seed; int t, T;
    uint8_t* fin;                     // [rows] in / out: the row has drawn <end>; null (with n_unf): the kernel alone, every row live
    int* n_unf;                       // [T] rows still unfinished after each step (zeroed in front of the decode)
    int64_t* ids_out; float* logp_out;        // [rows, T]
    float* score_out;                 // [rows] (may be null)
    int64_t* it_next;                 // [rows] (may be null)
    const float* emb_table; float* emb_next; int E, relu;     // the next step's input embedding (emb_next may be null)
    uint8_t* keep_out;                // [rows, V] or null: 1 = the token survived the filters
};
// The ensemble instance: the row is lp[v] = log(sum_m w_m softmax(logits_m)[v]) of `ens`, and the tail writes the next step's input
// embedding of every member (emb[m].emb null: none, the kernel alone); s.lv and s.emb_* are not read.
struct EnsSampleDecArgs {
    SampleDecArgs s;
    EnsArgs ens;
    DecodeMember::EmbSlot emb[ENS_MAX_M];
};

// the argument rules of icz_sample_opts (V < 0: no handle yet, the vocabulary is not known and its rules wait for one)
int check_sample_opts(const char* who, const icz_sample_opts* o, int n_img, int n, int V, int max_rows);
// start of a decode: <sta> in `it`, no row finished, row r belongs to image r / n, the per-step counters of unfinished rows = 0
void launch_sample_decode_init(int64_t* it, uint8_t* fin, int32_t* img_of_row, int rows, int n, int* n_unf, int T, hipStream_t st);
int launch_sample_decode(const SampleDecArgs& a, int rows, hipStream_t st);
int launch_sample_decode(const EnsSampleDecArgs& a, int rows, hipStream_t st);
// the member's SampleBuf (tokens, finished flags, per-step counts, image of each row) for `rows` rows and T steps
int ensure_sample_buf(DecodeMember* m, int rows, int T);

// ---- score_tokens_kernel (score_captions.hip) ----
struct ScoreArgs {
    LogitsView lv; int V;             // lv: the single-model instance's row source (the ensemble instance reads EnsScoreArgs::ens)
    const int64_t* ids;               // [rows, T] the given captions; the kernel alone: [rows] targets with T = 1
    int t, T;
    uint8_t* fin;                     // [rows] in / out: the row is past its length; null (with n_unf): the kernel alone, every row live
    int* n_unf;                       // [T] rows with a token left to score after each step (zeroed in front of the pass)
    float* logp_out;                  // [rows, T]
    float* score_out;                 // [rows] (may be null)
    int64_t* it_next;                 // [rows] (may be null)
    const float* emb_table; float* emb_next; int E, relu;     // the next step's input embedding (emb_next may be null)
};
// The ensemble instance: logp = log(sum_m w_m softmax(logits_m)[target]) of `ens`, and the tail writes the next step's input embedding
// of every member (emb[m].emb null: none, the kernel alone); s.lv and s.emb_* are not read.
struct EnsScoreArgs {
    ScoreArgs s;
    EnsArgs ens;
    DecodeMember::EmbSlot emb[ENS_MAX_M];
};
// the host-only argument rules of icz_*_score_captions
int check_score_args(const char* who, int n_img, int n, int max_len, int max_rows);
// start of a scoring pass: <sta> in `it`, a row whose first token is 0 or outside [0, V) finished, image of each row, counters = 0
void launch_score_init(const int64_t* ids, int64_t* it, uint8_t* fin, int32_t* img_of_row, int rows, int n, int* n_unf, int T, int V,
                       hipStream_t st);
void launch_score_tokens(const ScoreArgs& a, int rows, hipStream_t st);
void launch_score_tokens(const EnsScoreArgs& a, int rows, hipStream_t st);
// weights: null = uniform; else finite, >= 0, sum > 0 -> log of the normalised weights (ensemble.hip)
int ens_log_weights(const char* who, const float* weights, int M, float* logw);

// ---- distill_loss_dlogits_kernel (distill.hip) ----
// ens: the teachers' packed logits [N, ld_m] as finished rows (ns 1) with the log of their normalised weights
struct DistillArgs {
    EnsArgs ens;
    float alpha, temperature, smoothing;
};
// the argument rules 1 - 8 of icz_distill_opts in their documented order (V < 0: no handle yet, rule 7 waits for one) -> the kernel's view
int distill_args(const char* who, const icz_distill_opts* o, int V, DistillArgs* out);

}  // namespace icz
