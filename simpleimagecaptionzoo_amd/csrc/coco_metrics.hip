// Integer statistics of the evaluation report's BLEU and ROUGE-L on the device, replacing the pure-Python scorers of the
// reference's coco_eval (COCO_Eval_Utils.py:15-35 -> coco_caption/pycocoevalcap/eval.py:24-69):
//   bleu_stats_kernel: precook / cook_refs / cook_test (bleu/bleu_scorer.py:26-86) with option "closest";
//   rouge_lcs_kernel:  my_lcs (rouge/rouge.py:15-36) for every (hypothesis, reference) pair.
// Both kernels produce integers only; every floating-point step of the scores (bleu_scorer.py:201-266, rouge.py:47-104) stays
// on the host in the reference's order, so there is no device rounding to match.  Tokens are corpus-local ids >= 0 laid out
// in CSR form: hypothesis i = hyp_tok[hyp_ptr[i] .. hyp_ptr[i+1]), reference r = ref_tok[ref_ptr[r] .. ref_ptr[r+1]), image i
// owns references img_ref_ptr[i] .. img_ref_ptr[i+1].  One wave per image; hypotheses are at most CM_MAXT tokens (checked on
// the host), references are streamed from global memory and have no length bound.
#include "icz_common.h"

namespace icz {

constexpr int CM_MAXT = 60;                   // max tokens per hypothesis (coco_eval.py: Cider.MAX_TOKENS)
constexpr int CM_SLOTS = (4 * CM_MAXT + 63) / 64;    // n-gram positions held per lane

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// stats [n_img, 6] = testlen, closest reflen, correct1..4.  Position p of the hypothesis' n-grams (precook order: order k =
// 1..4, start i = 0..len-k) lives on lane p % 64.  A position that is the first occurrence of its n-gram contributes
// min(count in the hypothesis, largest count in one reference) to correct[k] (cook_test, :80-84; maxcounts of cook_refs, :45-49).
__global__ __launch_bounds__(64) void bleu_stats_kernel(const int32_t* __restrict__ hyp_tok, const int32_t* __restrict__ hyp_ptr,
                                                       const int32_t* __restrict__ ref_tok, const int32_t* __restrict__ ref_ptr,
                                                       const int32_t* __restrict__ img_ref_ptr, int n_img, int32_t* __restrict__ stats) {
    __shared__ int tok[CM_MAXT + 3];       // + 3: the unrolled comparisons below may read past the n-gram (never used)
    const int img = blockIdx.x, lane = threadIdx.x;
    if (img >= n_img) return;
    const int h0 = hyp_ptr[img];
    const int len = min(hyp_ptr[img + 1] - h0, CM_MAXT);       // the host rejects longer hypotheses; the clamp only guards LDS
    if (lane < len) tok[lane] = hyp_tok[h0 + lane];
    __syncthreads();
    int start[5], npos = 0;
    for (int k = 1; k <= 4; ++k) { start[k] = npos; npos += max(len - k + 1, 0); }
    // this lane's positions: order, key (token ids last-first, -1 padded: matches the sliding window below), hypothesis count
    int ord[CM_SLOTS], key[CM_SLOTS][4], cnt_h[CM_SLOTS], maxref[CM_SLOTS];
#pragma unroll
    for (int s = 0; s < CM_SLOTS; ++s) {
        const int p = lane + 64 * s;
        ord[s] = 0; cnt_h[s] = 0; maxref[s] = 0;
        key[s][0] = key[s][1] = key[s][2] = key[s][3] = -1;
        if (p >= npos) continue;
        int k = 4;
        while (k > 1 && p < start[k]) --k;
        const int i = p - start[k];
        bool first = true;
        int c = 0;
        for (int q = 0; q + k <= len; ++q) {
            bool same = true;
#pragma unroll
            for (int j = 0; j < 4; ++j) same = same && (j >= k || tok[q + j] == tok[i + j]);
            if (same) { ++c; if (q < i) first = false; }
        }
        if (!first) continue;
        ord[s] = k;
        cnt_h[s] = c;
#pragma unroll
        for (int j = 0; j < 4; ++j) key[s][j] = j < k ? tok[i + max(k - 1 - j, 0)] : -1;
    }
    // references: every lane walks every reference token (uniform loads); w0..w3 = the last four tokens, newest first
    const int r0 = img_ref_ptr[img], r1 = img_ref_ptr[img + 1];
    int reflen = 0, best_d = 0x7fffffff;
    for (int r = r0; r < r1; ++r) {
        const int b = ref_ptr[r], e = ref_ptr[r + 1];
        int cnt_r[CM_SLOTS];
#pragma unroll
        for (int s = 0; s < CM_SLOTS; ++s) cnt_r[s] = 0;
        int w0 = -1, w1 = -1, w2 = -1, w3 = -1;
        for (int t = b; t < e; ++t) {
            w3 = w2; w2 = w1; w1 = w0; w0 = ref_tok[t];
#pragma unroll
            for (int s = 0; s < CM_SLOTS; ++s) {
                const int k = ord[s];
                const bool hit = k > 0 && key[s][0] == w0 && (k < 2 || key[s][1] == w1) && (k < 3 || key[s][2] == w2) &&
                                 (k < 4 || key[s][3] == w3);
                cnt_r[s] += hit;
            }
        }
#pragma unroll
        for (int s = 0; s < CM_SLOTS; ++s) maxref[s] = max(maxref[s], cnt_r[s]);
        // "closest": min over (|l - testlen|, l) -- a tie goes to the shorter reference (:73-74, :190-191)
        const int l = e - b, d = abs(l - len);
        if (d < best_d || (d == best_d && l < reflen)) { best_d = d; reflen = l; }
    }
    int corr[4] = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < CM_SLOTS; ++s)
        if (ord[s] > 0) corr[ord[s] - 1] += min(cnt_h[s], maxref[s]);
#pragma unroll
    for (int k = 0; k < 4; ++k) corr[k] = wave_sum_i(corr[k]);
    if (lane == 0) {
        int32_t* o = stats + (size_t)img * 6;
        o[0] = len; o[1] = reflen;
        o[2] = corr[0]; o[3] = corr[1]; o[4] = corr[2]; o[5] = corr[3];
    }
}

// lcs [n_ref]: LCS length of image i's hypothesis with each of its references, bit-parallel (Allison-Dix / Hyyro): lane j < m
// holds hypothesis token j; per reference token t, M = the lanes that hold t and V = (V + (V & M)) | (V & ~M).  The zeros of V
// in its low m bits count the LCS.  Carries out of bit m - 1 only move upwards, so V starts as all ones and is masked once.
__global__ __launch_bounds__(64) void rouge_lcs_kernel(const int32_t* __restrict__ hyp_tok, const int32_t* __restrict__ hyp_ptr,
                                                      const int32_t* __restrict__ ref_tok, const int32_t* __restrict__ ref_ptr,
                                                      const int32_t* __restrict__ img_ref_ptr, int n_img, int32_t* __restrict__ lcs) {
    const int img = blockIdx.x, lane = threadIdx.x;
    if (img >= n_img) return;
    const int h0 = hyp_ptr[img];
    const int m = min(hyp_ptr[img + 1] - h0, CM_MAXT);
    const int h = lane < m ? hyp_tok[h0 + lane] : -1;         // token ids are >= 0: -1 never matches
    const unsigned long long mask = m >= 64 ? ~0ull : ((1ull << m) - 1ull);
    const int r0 = img_ref_ptr[img], r1 = img_ref_ptr[img + 1];
    for (int r = r0; r < r1; ++r) {
        unsigned long long V = ~0ull;
        const int e = ref_ptr[r + 1];
        for (int t = ref_ptr[r]; t < e; ++t) {
            const unsigned long long M = __ballot(h == ref_tok[t]);
            V = (V + (V & M)) | (V & ~M);
        }
        if (lane == 0) lcs[r] = __popcll(~V & mask);
    }
}

}  // namespace icz

using namespace icz;
extern "C" {

int icz_bleu_stats(const int32_t* hyp_tok, const int32_t* hyp_ptr, const int32_t* ref_tok, const int32_t* ref_ptr,
                   const int32_t* img_ref_ptr, int32_t n_img, int32_t* stats_out, void* stream) {
    ICZ_REQUIRE(hyp_tok && hyp_ptr && ref_tok && ref_ptr && img_ref_ptr && stats_out, "icz_bleu_stats: null argument");
    ICZ_REQUIRE(n_img >= 0, "icz_bleu_stats: n_img=%d < 0", n_img);
    if (n_img == 0) return ICZ_OK;
    hipLaunchKernelGGL(bleu_stats_kernel, dim3(n_img), dim3(64), 0, (hipStream_t)stream, hyp_tok, hyp_ptr, ref_tok, ref_ptr,
                       img_ref_ptr, (int)n_img, stats_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_rouge_lcs(const int32_t* hyp_tok, const int32_t* hyp_ptr, const int32_t* ref_tok, const int32_t* ref_ptr,
                  const int32_t* img_ref_ptr, int32_t n_img, int32_t* lcs_out, void* stream) {
    ICZ_REQUIRE(hyp_tok && hyp_ptr && ref_tok && ref_ptr && img_ref_ptr && lcs_out, "icz_rouge_lcs: null argument");
    ICZ_REQUIRE(n_img >= 0, "icz_rouge_lcs: n_img=%d < 0", n_img);
    if (n_img == 0) return ICZ_OK;
    hipLaunchKernelGGL(rouge_lcs_kernel, dim3(n_img), dim3(64), 0, (hipStream_t)stream, hyp_tok, hyp_ptr, ref_tok, ref_ptr,
                       img_ref_ptr, (int)n_img, lcs_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
