// CIDEr-D reward on the device (float64), replacing the per-batch pure-Python scorer of the reference:
//   Utils.py:319-367 get_self_critical_reward -> ciderD.py:30-55 -> ciderD_scorer.py:17-32 (precook),
//   :127-206 (compute_cider).
// One workgroup of CD_NW waves per hypothesis (2B of them: B sampled, B greedy).  Hypotheses are at most T <= 60 tokens,
// so a hypothesis has at most 4T n-gram positions; threads work on positions in parallel (dedup, df lookup) and each wave
// matches the hypothesis against one of the image's cooked references at a time.  Every floating-point accumulation is
// performed by one lane in the reference's dict-insertion order (per reference by the wave's lane 0, across references
// by thread 0 in reference order), which makes the scores bit-identical to the reference's float64 results.
// Caption sets (include/icz.h "Caption sets"): the same kernel with int32 CSR hypotheses, against the reference store or against the
// image's other candidates cooked on the device (ciderd_cook_kernel), and the n-gram counts of the diversity metrics.
#include <math.h>

#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "icz_common.h"

namespace icz {

struct CiderD {
    int32_t* keys = nullptr;     // [cap,4]
    double* idf = nullptr;       // [cap]
    double* penalty = nullptr;   // [64]
    int64_t cap = 0;
    double default_idf = 0.0;
};

constexpr int CD_MAXT = 60;                 // max tokens per hypothesis
constexpr int CD_MAXP = 4 * CD_MAXT;        // max n-gram positions
constexpr int CD_NW = 8;                    // waves per hypothesis = references matched at a time

__host__ __device__ inline uint32_t ngram_hash(int a, int b, int c, int d) {
    uint32_t h = 2166136261u;
    h = (h ^ (uint32_t)a) * 16777619u;
    h = (h ^ (uint32_t)b) * 16777619u;
    h = (h ^ (uint32_t)c) * 16777619u;
    h = (h ^ (uint32_t)d) * 16777619u;
    h ^= h >> 15;
    return h;
}

struct CiderArgs {
    const int32_t* keys; const double* idf; const double* penalty; int64_t cap; double default_idf;
    const int64_t* gen; const int64_t* greedy; int B, T;
    const int32_t* img_slot;     // [B] slot of image b in the reference store, or null = b (the arrays below are the batch's own)
    const int32_t* img_ref_ptr; const int32_t* ref_ent_ptr; const int32_t* ent_key; const int32_t* ent_order;
    const double* ent_w; const double* ref_norm; const int32_t* ref_len;
    double* scores;      // [2B] ([B] without greedy)
    int rows_per_img;    // hypothesis b belongs to image b / rows_per_img (img_slot index; 0 = 1): the multi-sample reward
    // caption sets (SRC_CSR, SRC_CSR_PAIRS): hypothesis b = csr_tok[csr_ptr[b] .. csr_ptr[b+1]), every token a word
    const int32_t* csr_tok; const int32_t* csr_ptr;
    double* pair_out;    // SRC_CSR_PAIRS: [B, K] per-reference scores, K = rows_per_img; `scores` receives the consensus
};

// Where a hypothesis comes from and what it is matched against:
//   SRC_ROWS       int64 rows with the length rules of Utils.py:337-356 against the references of its image (the SCST rewards);
//   SRC_CSR        int32 CSR tokens against the references of its image (icz_ciderd_scores_csr);
//   SRC_CSR_PAIRS  int32 CSR tokens against the cooked hypotheses of its own image, which icz_ciderd_cook_device laid out as one
//                  reference each: reference index = hypothesis index, image i owns i K .. (i + 1) K (icz_ciderd_pairwise).
enum { SRC_ROWS = 0, SRC_CSR = 1, SRC_CSR_PAIRS = 2 };

template <int SRC>
__global__ __launch_bounds__(64 * CD_NW) void ciderd_kernel(CiderArgs a) {
    __shared__ int tok[CD_MAXT];
    __shared__ int pkey[CD_MAXP][4];
    __shared__ int porder[CD_MAXP];       // 1..4
    __shared__ int pcount[CD_MAXP];       // occurrences if this position is the first occurrence, else 0
    __shared__ double pw[CD_MAXP];        // tf-idf weight of the n-gram first seen at this position
    __shared__ double pmatch[CD_NW][CD_MAXP];    // per wave: weight of the same n-gram in the wave's current reference (0 if absent)
    __shared__ double rval[CD_NW][4];     // per wave: the reference's contribution to the four n-gram orders
    constexpr int NT = 64 * CD_NW;
    const int hyp = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = hyp % a.B;
    const bool is_greedy = hyp >= a.B;            // (no greedy hypotheses without a.greedy: B blocks)
    const int bi = a.rows_per_img > 1 ? b / a.rows_per_img : b;
    int len;
    if (SRC == SRC_ROWS) {
        const int64_t* ids = (is_greedy ? a.greedy : a.gen) + (size_t)b * a.T;
        // ---- sentence length (Utils.py:337-356)
        if (is_greedy) {
            len = a.T;
            for (int i = 0; i < a.T; ++i)
                if (ids[i] == 2) { len = i; break; }
        } else {
            int end = 0;
            for (int e = a.T - 1; e >= 0; --e) {
                end = e;
                if (ids[e] != 0) break;
            }
            len = end + 1;
        }
        for (int i = tid; i < len; i += NT) tok[i] = (int)ids[i];
    } else {
        const int t0 = a.csr_ptr[hyp];
        len = a.csr_ptr[hyp + 1] - t0;
        len = len < 0 ? 0 : (len > CD_MAXT ? CD_MAXT : len);      // the host rejects longer candidates; the clamp only guards LDS
        for (int i = tid; i < len; i += NT) tok[i] = a.csr_tok[t0 + i];
    }
    __syncthreads();
    // ---- n-gram positions in precook order: k = 1..4, i = 0..len-k
    int npos = 0, start[5];
    for (int k = 1; k <= 4; ++k) { start[k] = npos; npos += (len - k + 1 > 0) ? (len - k + 1) : 0; }
    for (int p = tid; p < npos; p += NT) {
        int k = 4;
        while (k > 1 && p < start[k]) --k;
        const int i = p - start[k];
        porder[p] = k;
        for (int j = 0; j < 4; ++j) pkey[p][j] = (j < k) ? tok[i + j] : -1;
    }
    __syncthreads();
    // ---- dedup: a position is "first" if no earlier position holds the same n-gram; count = #occurrences
    for (int p = tid; p < npos; p += NT) {
        const int k = porder[p];
        bool first = true;
        int cnt = 0;
        const int s0 = start[k], s1 = s0 + (len - k + 1);
        for (int q = s0; q < s1; ++q) {
            const bool same = pkey[q][0] == pkey[p][0] && pkey[q][1] == pkey[p][1] && pkey[q][2] == pkey[p][2] && pkey[q][3] == pkey[p][3];
            if (same) { ++cnt; if (q < p) first = false; }
        }
        pcount[p] = first ? cnt : 0;
        double w = 0.0;
        if (first) {
            // document-frequency lookup (open addressing, linear probing)
            double idfv = a.default_idf;
            uint32_t h = ngram_hash(pkey[p][0], pkey[p][1], pkey[p][2], pkey[p][3]);
            for (int64_t probe = 0; probe < a.cap; ++probe) {
                const int64_t s = (int64_t)((h + (uint32_t)probe) & (uint32_t)(a.cap - 1));
                const int32_t* kk = a.keys + s * 4;
                if (kk[0] == -1) break;   // empty slot (token ids are >= 0, so key[0] == -1 marks empty)
                if (kk[0] == pkey[p][0] && kk[1] == pkey[p][1] && kk[2] == pkey[p][2] && kk[3] == pkey[p][3]) { idfv = a.idf[s]; break; }
            }
            w = (double)cnt * idfv;      // float(term_freq) * (ref_len - df)   (ciderD_scorer.py:145)
        }
        pw[p] = w;
    }
    __syncthreads();
    // ---- hypothesis norms and length (thread 0, insertion order)   (:146-152)
    __shared__ double hnorm[4];
    __shared__ int hlen;
    if (tid == 0) {
        double nn[4] = {0.0, 0.0, 0.0, 0.0};
        int l2 = 0;
        for (int p = 0; p < npos; ++p)
            if (pcount[p]) {
                nn[porder[p] - 1] += pw[p] * pw[p];
                if (porder[p] == 2) l2 += pcount[p];
            }
        for (int n = 0; n < 4; ++n) hnorm[n] = sqrt(nn[n]);
        hlen = l2;
    }
    __syncthreads();
    // ---- references of this image, CD_NW at a time: wave w takes reference rc + w
    int r0, r1;
    if (SRC == SRC_CSR_PAIRS) {
        r0 = bi * a.rows_per_img;
        r1 = r0 + a.rows_per_img;
    } else {
        const int slot = a.img_slot ? a.img_slot[bi] : bi;
        r0 = a.img_ref_ptr[slot];
        r1 = a.img_ref_ptr[slot + 1];
    }
    double score[4] = {0.0, 0.0, 0.0, 0.0};
    for (int rc = r0; rc < r1; rc += CD_NW) {
        const int r = rc + wave;
        if (r < r1) {
            const int e0 = a.ref_ent_ptr[r], e1 = a.ref_ent_ptr[r + 1];
            for (int p = lane; p < npos; p += 64) {
                double m = 0.0;
                if (pcount[p]) {
                    for (int e = e0; e < e1; ++e) {
                        const int32_t* kk = a.ent_key + (size_t)e * 4;
                        if (a.ent_order[e] == porder[p] && kk[0] == pkey[p][0] && kk[1] == pkey[p][1] && kk[2] == pkey[p][2] && kk[3] == pkey[p][3]) {
                            m = a.ent_w[e];
                            break;
                        }
                    }
                }
                pmatch[wave][p] = m;
            }
        }
        __syncthreads();
        if (r < r1 && lane == 0) {
            double val[4] = {0.0, 0.0, 0.0, 0.0};
            for (int p = 0; p < npos; ++p)
                if (pcount[p]) {
                    const double h = pw[p], rr = pmatch[wave][p];
                    val[porder[p] - 1] += (h < rr ? h : rr) * rr;       // min(vec_hyp, vec_ref) * vec_ref  (:172-175)
                }
            int d = hlen - a.ref_len[r];
            if (d < 0) d = -d;
            const double pen = a.penalty[d > 63 ? 63 : d];
            for (int n = 0; n < 4; ++n) {
                const double nr = a.ref_norm[(size_t)r * 4 + n];
                if (hnorm[n] != 0.0 && nr != 0.0) val[n] /= (hnorm[n] * nr);
                val[n] *= pen;
                rval[wave][n] = val[n];
            }
        }
        __syncthreads();
        if (tid == 0) {
            const int nr_ = r1 - rc < CD_NW ? r1 - rc : CD_NW;
            for (int w = 0; w < nr_; ++w) {
                if (SRC == SRC_CSR_PAIRS) {
                    // sibling rc + w as the ONLY reference: compute_cider with one reference (mean over n, / 1, * 10)
                    double s = rval[w][0];
                    s += rval[w][1]; s += rval[w][2]; s += rval[w][3];
                    s = s / 4.0;
                    s *= 10.0;
                    a.pair_out[(size_t)hyp * a.rows_per_img + (rc - r0 + w)] = s;
                    if (rc + w == hyp) continue;      // the consensus leaves the hypothesis itself out of its reference set
                }
                for (int n = 0; n < 4; ++n) score[n] += rval[w][n];       // reference order, as the scorer's loop (:186-196)
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double s = score[0];
        s += score[1]; s += score[2]; s += score[3];
        s = s / 4.0;                      // np.mean over n
        s /= (double)(SRC == SRC_CSR_PAIRS ? r1 - r0 - 1 : r1 - r0);           // / len(refs)
        s *= 10.0;
        a.scores[hyp] = s;
    }
}

__global__ void ciderd_reward_kernel(const double* __restrict__ scores, int B, int T, float* __restrict__ reward) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * T) return;
    int b = i / T;
    reward[i] = (float)(scores[b] - scores[B + b]);
}

// Leave-one-out baseline of the multi-sample reward (the "new self-critical" variant): hypothesis i = img * K + k,
//   base_i = (sum_{j != i, ascending j} s_j) / (K - 1)   over the K hypotheses of its image,   reward[i, :] = (float)(s_i - base_i)
// in float64, the sum in a fixed order (one thread per element recomputes its row's K - 1 terms: K <= 8).
__global__ void ciderd_loo_kernel(const double* __restrict__ scores, int BK, int K, int T, float* __restrict__ reward) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BK * T) return;
    const int h = i / T, j0 = h - h % K;
    double s = 0.0;
    for (int j = j0; j < j0 + K; ++j)
        if (j != h) s += scores[j];
    const double base = s / (double)(K - 1);
    reward[i] = (float)(scores[h] - base);
}

// ---- caption sets: cooking on the device -----------------------------------------------------------------------------------------
// icz_ciderd_cook_host for candidates that are already on the device: one workgroup per candidate, one thread per n-gram position
// (precook order: k = 1..4, i ascending; at most CD_MAXP = 240 <= CK_NT).  A position that is the first occurrence of its n-gram
// becomes an entry; its slot is the number of first occurrences in front of it (wave ballots + a prefix over the four waves), which
// is the scorer's dict-insertion order.  COUNT: only the number of entries is written (the pass in front of the prefix sum over
// candidates that packs the entries); otherwise keys, orders and weights go to ent_ptr[c] + slot and thread 0 sums the squared
// weights in entry order for the norms, as the host cooker's loop does.
constexpr int CK_NT = 256;
static_assert(CD_MAXP <= CK_NT, "one thread per n-gram position");

struct CookArgs {
    const int32_t* keys; const double* idf; int64_t cap; double default_idf;
    const int32_t* tok; const int32_t* ptr; int n_cand;
    int32_t* ent_key; int32_t* ent_order; double* ent_w; int32_t* ent_ptr; double* norm; int32_t* len;
};

template <bool COUNT>
__global__ __launch_bounds__(CK_NT) void ciderd_cook_kernel(CookArgs a) {
    __shared__ int tok[CD_MAXT + 3];
    __shared__ int wave_n[CK_NT / 64];
    __shared__ double sw[CD_MAXP];        // entry slot -> weight
    __shared__ int so[CD_MAXP];           // entry slot -> order * 256 + term frequency
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (c >= a.n_cand) return;
    const int t0 = a.ptr[c];
    int len = a.ptr[c + 1] - t0;
    len = len < 0 ? 0 : (len > CD_MAXT ? CD_MAXT : len);          // the host rejects longer candidates; the clamp only guards LDS
    if (tid < CD_MAXT + 3) tok[tid] = tid < len ? a.tok[t0 + tid] : -1;
    __syncthreads();
    int npos = 0, start[5];
    for (int k = 1; k <= 4; ++k) { start[k] = npos; npos += (len - k + 1 > 0) ? (len - k + 1) : 0; }
    const int p = tid;
    bool first = false;
    int k = 0, i = 0, cnt = 0;
    if (p < npos) {
        k = 4;
        while (k > 1 && p < start[k]) --k;
        i = p - start[k];
        first = true;
        for (int q = 0; q + k <= len; ++q) {
            bool same = true;
            for (int j = 0; j < k; ++j) same = same && tok[q + j] == tok[i + j];
            if (same) { ++cnt; if (q < i) first = false; }
        }
    }
    // ---- prefix sum of the first-occurrence flags in position order
    const unsigned long long bal = __ballot(first);
    if (lane == 0) wave_n[wave] = __popcll(bal);
    __syncthreads();
    int slot = __popcll(bal & ((1ull << lane) - 1ull)), n_ent = 0;
    for (int w = 0; w < CK_NT / 64; ++w) {
        if (w < wave) slot += wave_n[w];
        n_ent += wave_n[w];
    }
    if (COUNT) {
        if (tid == 0) a.ent_ptr[c + 1] = n_ent;
        return;
    }
    const int e0 = a.ent_ptr[c];
    if (first) {
        int key[4];
        for (int j = 0; j < 4; ++j) key[j] = j < k ? tok[i + j] : -1;
        // document-frequency lookup (open addressing, linear probing)
        double idfv = a.default_idf;
        const uint32_t h = ngram_hash(key[0], key[1], key[2], key[3]);
        for (int64_t probe = 0; probe < a.cap; ++probe) {
            const int64_t s = (int64_t)((h + (uint32_t)probe) & (uint32_t)(a.cap - 1));
            const int32_t* kk = a.keys + s * 4;
            if (kk[0] == -1) break;
            if (kk[0] == key[0] && kk[1] == key[1] && kk[2] == key[2] && kk[3] == key[3]) { idfv = a.idf[s]; break; }
        }
        const double w = (double)cnt * idfv;          // float(term_freq) * (ref_len - df)   (ciderD_scorer.py:145)
        int32_t* o = a.ent_key + (size_t)(e0 + slot) * 4;
        o[0] = key[0]; o[1] = key[1]; o[2] = key[2]; o[3] = key[3];
        a.ent_order[e0 + slot] = k;
        a.ent_w[e0 + slot] = w;
        sw[slot] = w;
        so[slot] = k * 256 + cnt;
    }
    __syncthreads();
    if (tid == 0) {
        double nn[4] = {0.0, 0.0, 0.0, 0.0};
        int l2 = 0;
        for (int e = 0; e < n_ent; ++e) {
            const int ord = so[e] >> 8;
            nn[ord - 1] += sw[e] * sw[e];             // norm[n] += pow(vec[n][ngram], 2)   (:147)
            if (ord == 2) l2 += so[e] & 255;
        }
        for (int n = 0; n < 4; ++n) a.norm[(size_t)c * 4 + n] = sqrt(nn[n]);
        a.len[c] = l2;
    }
}

// ent_ptr[0] = 0, ent_ptr[c + 1] = counts of candidates 0..c summed (the counts arrive in ent_ptr[1..n]).  One workgroup: every
// thread owns a contiguous chunk, the chunk totals are scanned in LDS, integers only.
constexpr int SCAN_NT = 1024;
__global__ __launch_bounds__(SCAN_NT) void ciderd_ent_scan_kernel(int32_t* __restrict__ ent_ptr, int n) {
    __shared__ int part[SCAN_NT];
    const int tid = threadIdx.x;
    const int chunk = (n + SCAN_NT - 1) / SCAN_NT;
    const int lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += ent_ptr[1 + i];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < SCAN_NT; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;              // total of the chunks in front of this one
    for (int i = lo; i < hi; ++i) {
        run += ent_ptr[1 + i];
        ent_ptr[1 + i] = run;
    }
    if (tid == 0) ent_ptr[0] = 0;
}

// best[i] = the hypothesis of image i with the largest consensus; ties go to the lowest index
__global__ void ciderd_best_kernel(const double* __restrict__ consensus, int n_img, int K, int32_t* __restrict__ best) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    int arg = 0;
    double top = consensus[(size_t)i * K];
    for (int k = 1; k < K; ++k) {
        const double v = consensus[(size_t)i * K + k];
        if (v > top) { top = v; arg = k; }
    }
    best[i] = arg;
}

// ---- caption sets: distinct and total n-grams of an image's K candidates (Div-n) ---------------------------------------------------
// One workgroup per image with the image's tokens and the start of every n-gram position in LDS.  Per order n, position p (over
// the candidates in order, n-grams never cross a candidate's end) is distinct if no earlier position holds the same n-gram; the
// flags are counted with ballots and summed over the waves.  Integers only, no atomics.
constexpr int DV_NT = 256;
constexpr int DV_MAXK = 8;
constexpr int DV_MAXTOK = DV_MAXK * CD_MAXT;

__global__ __launch_bounds__(DV_NT) void ngram_diversity_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ ptr, int n_img,
                                                                 int K, int32_t* __restrict__ counts) {
    __shared__ int tok[DV_MAXTOK];
    __shared__ int pstart[DV_MAXTOK];
    __shared__ int cstart[DV_MAXK + 1];
    __shared__ int wave_n[DV_NT / 64];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (img >= n_img) return;
    if (tid == 0) {
        int at = 0;
        for (int c = 0; c < K; ++c) {
            cstart[c] = at;
            int len = ptr[img * K + c + 1] - ptr[img * K + c];
            at += len < 0 ? 0 : (len > CD_MAXT ? CD_MAXT : len);      // the host rejects longer candidates; the clamp only guards LDS
        }
        cstart[K] = at;
    }
    __syncthreads();
    for (int c = 0; c < K; ++c) {
        const int t0 = ptr[img * K + c], len = cstart[c + 1] - cstart[c];
        for (int i = tid; i < len; i += DV_NT) tok[cstart[c] + i] = tokens[t0 + i];
    }
    for (int n = 1; n <= 4; ++n) {
        __syncthreads();                  // tokens loaded / the previous order's pstart and wave_n are no longer read
        int P = 0;
        for (int c = 0; c < K; ++c) {
            const int m = cstart[c + 1] - cstart[c] - n + 1;
            for (int i = tid; i < m; i += DV_NT) pstart[P + i] = cstart[c] + i;
            P += m > 0 ? m : 0;
        }
        __syncthreads();
        int distinct = 0;
        for (int p = tid; p < P; p += DV_NT) {
            const int sp = pstart[p];
            bool first = true;
            for (int q = 0; q < p && first; ++q) {
                const int sq = pstart[q];
                bool same = true;
                for (int j = 0; j < n; ++j) same = same && tok[sq + j] == tok[sp + j];
                if (same) first = false;
            }
            distinct += first;
        }
        for (int o = 32; o > 0; o >>= 1) distinct += __shfl_xor(distinct, o, 64);
        if (lane == 0) wave_n[wave] = distinct;
        __syncthreads();
        if (tid == 0) {
            int d = 0;
            for (int w = 0; w < DV_NT / 64; ++w) d += wave_n[w];
            counts[((size_t)img * 4 + (n - 1)) * 2] = d;
            counts[((size_t)img * 4 + (n - 1)) * 2 + 1] = P;
        }
    }
}

}  // namespace icz

using namespace icz;
extern "C" {

int icz_ciderd_create(const int32_t* df_keys, const double* df_idf, int64_t cap, double default_idf,
                      const double* penalty, icz_ciderd_t** out) {
    ICZ_REQUIRE(df_keys && df_idf && penalty && out, "icz_ciderd_create: null argument");
    ICZ_REQUIRE(cap >= 2 && (cap & (cap - 1)) == 0, "icz_ciderd_create: cap must be a power of two");
    CiderD* c = new CiderD();
    c->cap = cap;
    c->default_idf = default_idf;
    c->keys = const_cast<int32_t*>(df_keys);
    c->idf = const_cast<double*>(df_idf);
    c->penalty = const_cast<double*>(penalty);
    *out = reinterpret_cast<icz_ciderd_t*>(c);
    return ICZ_OK;
}

int icz_ciderd_destroy(icz_ciderd_t* h) {
    delete reinterpret_cast<CiderD*>(h);
    return ICZ_OK;
}

static int ciderd_reward_impl(icz_ciderd_t* h, const int64_t* gen, const int64_t* greedy, int32_t B, int32_t T, const int32_t* img_slot,
                              const int32_t* img_ref_ptr, const int32_t* ref_ent_ptr, const int32_t* ent_key,
                              const int32_t* ent_order, const double* ent_w, const double* ref_norm, const int32_t* ref_len,
                              float* reward_out, double* scores_out, void* stream) {
    ICZ_REQUIRE(h && gen && greedy && img_ref_ptr && ref_ent_ptr && ent_key && ent_order && ent_w && ref_norm && ref_len,
                "icz_ciderd_reward: null argument");
    ICZ_REQUIRE(scores_out, "icz_ciderd_reward: scores_out (2B float64 scratch) is required");
    ICZ_REQUIRE(B > 0 && T > 0 && T <= CD_MAXT, "icz_ciderd_reward: T=%d out of range 1..%d", T, CD_MAXT);
    CiderD* c = reinterpret_cast<CiderD*>(h);
    CiderArgs a = {c->keys, c->idf, c->penalty, c->cap, c->default_idf, gen, greedy, B, T, img_slot,
                   img_ref_ptr, ref_ent_ptr, ent_key, ent_order, ent_w, ref_norm, ref_len, scores_out};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ciderd_kernel<SRC_ROWS>, dim3(2 * B), dim3(64 * CD_NW), 0, st, a);
    if (reward_out) hipLaunchKernelGGL(ciderd_reward_kernel, dim3(cdiv(B * T, 256)), dim3(256), 0, st, scores_out, B, T, reward_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// Host side of the reference store: "cooking" references (ciderD_scorer.py:17-32 precook + :128-153 counts2vec) from token
// ids -- the reference does this in Python dict loops for every batch; here once per image, ~100x faster than the Python
// restatement in ciderd.py (which stays as the checker of this function, tests/test_cpu_abi_and_host.py).  Pure host code:
// no device memory is touched.  Entries of a reference come out in the scorer's dict-insertion order (order k ascending,
// first occurrence ascending), weights / norms in the scorer's float64 arithmetic (pow(w, 2) summed in that order, sqrt).
int icz_ciderd_cook_host(const int32_t* df_keys_host, const double* df_idf_host, int64_t cap, double default_idf,
                         const int32_t* tokens, const int32_t* ref_tok_ptr, int32_t n_refs, int64_t max_ent,
                         int32_t* ent_key_out, int32_t* ent_order_out, double* ent_w_out, int32_t* ref_ent_ptr_out,
                         double* ref_norm_out, int32_t* ref_len_out, int64_t* n_ent_out) {
    ICZ_REQUIRE(df_keys_host && df_idf_host && tokens && ref_tok_ptr && ent_key_out && ent_order_out && ent_w_out && ref_ent_ptr_out &&
                ref_norm_out && ref_len_out && n_ent_out, "icz_ciderd_cook_host: null argument");
    ICZ_REQUIRE(cap >= 2 && (cap & (cap - 1)) == 0 && n_refs >= 0, "icz_ciderd_cook_host: bad table size / reference count");
    int64_t ne = 0;
    ref_ent_ptr_out[0] = 0;
    std::vector<int32_t> cnt;
    for (int32_t r = 0; r < n_refs; ++r) {
        const int32_t* t = tokens + ref_tok_ptr[r];
        const int L = ref_tok_ptr[r + 1] - ref_tok_ptr[r];
        const int64_t e0 = ne;
        cnt.clear();
        for (int k = 1; k <= 4; ++k) {
            const int64_t k0 = ne;                       // entries of order k start here
            for (int i = 0; i + k <= L; ++i) {
                int32_t key[4] = {-1, -1, -1, -1};
                for (int j = 0; j < k; ++j) key[j] = t[i + j];
                int64_t hit = -1;
                for (int64_t e = k0; e < ne; ++e) {
                    const int32_t* kk = ent_key_out + e * 4;
                    if (kk[0] == key[0] && kk[1] == key[1] && kk[2] == key[2] && kk[3] == key[3]) { hit = e; break; }
                }
                if (hit >= 0) { ++cnt[(size_t)(hit - e0)]; continue; }
                ICZ_REQUIRE(ne < max_ent, "icz_ciderd_cook_host: more than %lld n-gram entries", (long long)max_ent);
                int32_t* o = ent_key_out + ne * 4;
                o[0] = key[0]; o[1] = key[1]; o[2] = key[2]; o[3] = key[3];
                ent_order_out[ne] = k;
                cnt.push_back(1);
                ++ne;
            }
        }
        double norm[4] = {0.0, 0.0, 0.0, 0.0};
        int32_t len2 = 0;
        for (int64_t e = e0; e < ne; ++e) {
            const int32_t* kk = ent_key_out + e * 4;
            double idfv = default_idf;
            const uint32_t hsh = ngram_hash(kk[0], kk[1], kk[2], kk[3]);
            for (int64_t probe = 0; probe < cap; ++probe) {
                const int64_t s = (int64_t)((hsh + (uint32_t)probe) & (uint32_t)(cap - 1));
                const int32_t* tk = df_keys_host + s * 4;
                if (tk[0] == -1) break;
                if (tk[0] == kk[0] && tk[1] == kk[1] && tk[2] == kk[2] && tk[3] == kk[3]) { idfv = df_idf_host[s]; break; }
            }
            const double w = (double)cnt[(size_t)(e - e0)] * idfv;     // float(term_freq) * (ref_len - df)   (ciderD_scorer.py:145)
            ent_w_out[e] = w;
            norm[ent_order_out[e] - 1] += pow(w, 2.0);                   // norm[n] += pow(vec[n][ngram], 2)   (:147)
            if (ent_order_out[e] == 2) len2 += cnt[(size_t)(e - e0)];
        }
        for (int n = 0; n < 4; ++n) ref_norm_out[(size_t)r * 4 + n] = sqrt(norm[n]);
        ref_len_out[r] = len2;
        ref_ent_ptr_out[r + 1] = (int32_t)ne;
    }
    *n_ent_out = ne;
    return ICZ_OK;
}

// Word -> id map of the scorer on the host side of the library: the caption vocabulary plus private ids (>= V, in order of first
// appearance) for words outside it, which the references and the document-frequency table may contain (they count in the
// reference norms and never match a hypothesis).  One owner for those private ids: the Python cooker asks here too
// (icz_ciderd_vocab_oov_id), so that references tokenised in C++ (icz_ciderd_cook_text) and n-grams keyed in Python agree.
struct CiderVocab {
    std::unordered_map<std::string, int32_t> base, ext;
    int32_t V = 0;
    std::mutex mu;
    int32_t id_of(const std::string& w) {
        auto it = base.find(w);
        if (it != base.end()) return it->second;
        std::lock_guard<std::mutex> lk(mu);
        auto e = ext.find(w);
        if (e != ext.end()) return e->second;
        const int32_t id = V + (int32_t)ext.size();
        ext.emplace(w, id);
        return id;
    }
};

int icz_ciderd_vocab_create(const char* words, const int64_t* word_off, const int32_t* word_id, int32_t n_words, int32_t V,
                            icz_ciderd_vocab_t** out) {
    ICZ_REQUIRE(words && word_off && word_id && n_words >= 0 && V > 0 && out, "icz_ciderd_vocab_create: bad arguments");
    CiderVocab* v = new CiderVocab();
    v->V = V;
    v->base.reserve((size_t)n_words * 2);
    for (int32_t i = 0; i < n_words; ++i) v->base.emplace(std::string(words + word_off[i], (size_t)(word_off[i + 1] - word_off[i])), word_id[i]);
    *out = reinterpret_cast<icz_ciderd_vocab_t*>(v);
    return ICZ_OK;
}
int icz_ciderd_vocab_destroy(icz_ciderd_vocab_t* v) {
    delete reinterpret_cast<CiderVocab*>(v);
    return ICZ_OK;
}
int icz_ciderd_vocab_oov_id(icz_ciderd_vocab_t* v, const char* word, int32_t len, int32_t* id_out) {
    ICZ_REQUIRE(v && word && len >= 0 && id_out, "icz_ciderd_vocab_oov_id: bad arguments");
    *id_out = reinterpret_cast<CiderVocab*>(v)->id_of(std::string(word, (size_t)len));
    return ICZ_OK;
}

// icz_ciderd_cook_host with the tokenisation in front of it: `text` holds n_refs references separated by '\n', words separated
// by runs of ASCII whitespace (str.split() of an ASCII string: the caller checks that the text is ASCII and has exactly
// n_refs - 1 newlines).  Everything between the caller's join() and the flat arrays happens here, outside the interpreter lock:
// the loader thread that cooks the next batch's references no longer competes with the training thread's kernel launches.
int icz_ciderd_cook_text(icz_ciderd_vocab_t* vocab, const int32_t* df_keys_host, const double* df_idf_host, int64_t cap, double default_idf,
                         const char* text, int64_t text_len, int32_t n_refs, int64_t max_ent,
                         int32_t* ent_key_out, int32_t* ent_order_out, double* ent_w_out, int32_t* ref_ent_ptr_out,
                         double* ref_norm_out, int32_t* ref_len_out, int64_t* n_ent_out) {
    ICZ_REQUIRE(vocab && text && text_len >= 0 && n_refs >= 0, "icz_ciderd_cook_text: bad arguments");
    CiderVocab* v = reinterpret_cast<CiderVocab*>(vocab);
    std::vector<int32_t> tok, ptr;
    tok.reserve((size_t)text_len / 2 + 8);
    ptr.reserve((size_t)n_refs + 1);
    ptr.push_back(0);
    std::string w;
    int64_t i = 0;
    int32_t refs = 0;
    auto is_space = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f' || (c >= 0x1c && c <= 0x1f); };    // str.split()'s ASCII whitespace minus '\n'
    while (refs < n_refs) {
        while (i < text_len && text[i] != '\n') {
            while (i < text_len && is_space(text[i])) ++i;
            const int64_t b = i;
            while (i < text_len && text[i] != '\n' && !is_space(text[i])) ++i;
            if (i > b) { w.assign(text + b, (size_t)(i - b)); tok.push_back(v->id_of(w)); }
        }
        ++i;                                     // the newline (or one past the end after the last reference)
        ptr.push_back((int32_t)tok.size());
        ++refs;
    }
    ICZ_REQUIRE(i >= text_len, "icz_ciderd_cook_text: text holds more than %d references", n_refs);
    if (tok.empty()) tok.push_back(0);           // keep the pointer valid
    return icz_ciderd_cook_host(df_keys_host, df_idf_host, cap, default_idf, tok.data(), ptr.data(), n_refs, max_ent, ent_key_out, ent_order_out,
                                ent_w_out, ref_ent_ptr_out, ref_norm_out, ref_len_out, n_ent_out);
}

int icz_ciderd_reward(icz_ciderd_t* h, const int64_t* gen, const int64_t* greedy, int32_t B, int32_t T,
                      const int32_t* img_ref_ptr, const int32_t* ref_ent_ptr, const int32_t* ent_key,
                      const int32_t* ent_order, const double* ent_w, const double* ref_norm, const int32_t* ref_len,
                      float* reward_out, double* scores_out, void* stream) {
    return ciderd_reward_impl(h, gen, greedy, B, T, nullptr, img_ref_ptr, ref_ent_ptr, ent_key, ent_order, ent_w, ref_norm, ref_len,
                              reward_out, scores_out, stream);
}

int icz_ciderd_reward_loo(icz_ciderd_t* h, const int64_t* gen, int32_t B, int32_t K, int32_t T, const int32_t* img_slot,
                          const int32_t* img_ref_ptr, const int32_t* ref_ent_ptr, const int32_t* ent_key, const int32_t* ent_order,
                          const double* ent_w, const double* ref_norm, const int32_t* ref_len, float* reward_out, double* scores_out,
                          void* stream) {
    ICZ_REQUIRE(K >= 2 && K <= 8, "icz_ciderd_reward_loo: K=%d samples per image outside 2..8", K);
    ICZ_REQUIRE(h, "icz_ciderd_reward_loo: null handle");
    ICZ_REQUIRE(gen && img_slot && img_ref_ptr && ref_ent_ptr && ent_key && ent_order && ent_w && ref_norm && ref_len && reward_out,
                "icz_ciderd_reward_loo: null argument");
    ICZ_REQUIRE(scores_out, "icz_ciderd_reward_loo: scores_out (B K float64 scratch) is required");
    ICZ_REQUIRE(B > 0 && T > 0 && T <= CD_MAXT, "icz_ciderd_reward_loo: B=%d, T=%d out of range (T 1..%d)", B, T, CD_MAXT);
    ICZ_REQUIRE((int64_t)B * K * T < (1ll << 31), "icz_ciderd_reward_loo: B K T too large");
    CiderD* c = reinterpret_cast<CiderD*>(h);
    const int BK = B * K;
    CiderArgs a = {c->keys, c->idf, c->penalty, c->cap, c->default_idf, gen, nullptr, BK, T, img_slot,
                   img_ref_ptr, ref_ent_ptr, ent_key, ent_order, ent_w, ref_norm, ref_len, scores_out, K};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ciderd_kernel<SRC_ROWS>, dim3(BK), dim3(64 * CD_NW), 0, st, a);
    hipLaunchKernelGGL(ciderd_loo_kernel, dim3(cdiv(BK * T, 256)), dim3(256), 0, st, (const double*)scores_out, BK, K, T, reward_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_ciderd_reward_indexed(icz_ciderd_t* h, const int64_t* gen, const int64_t* greedy, int32_t B, int32_t T,
                              const int32_t* img_slot, const int32_t* img_ref_ptr, const int32_t* ref_ent_ptr,
                              const int32_t* ent_key, const int32_t* ent_order, const double* ent_w, const double* ref_norm,
                              const int32_t* ref_len, float* reward_out, double* scores_out, void* stream) {
    ICZ_REQUIRE(img_slot, "icz_ciderd_reward_indexed: null img_slot");
    return ciderd_reward_impl(h, gen, greedy, B, T, img_slot, img_ref_ptr, ref_ent_ptr, ent_key, ent_order, ent_w, ref_norm, ref_len,
                              reward_out, scores_out, stream);
}

// ---- caption sets ------------------------------------------------------------------------------------------------------------------
static int cook_device_launch(const CiderD* c, const int32_t* tok, const int32_t* ptr, int32_t n_cand, int32_t* ent_key, int32_t* ent_order,
                              double* ent_w, int32_t* ent_ptr, double* norm, int32_t* len, hipStream_t st) {
    CookArgs a = {c->keys, c->idf, c->cap, c->default_idf, tok, ptr, n_cand, ent_key, ent_order, ent_w, ent_ptr, norm, len};
    hipLaunchKernelGGL(ciderd_cook_kernel<true>, dim3(n_cand), dim3(CK_NT), 0, st, a);
    hipLaunchKernelGGL(ciderd_ent_scan_kernel, dim3(1), dim3(SCAN_NT), 0, st, ent_ptr, (int)n_cand);
    hipLaunchKernelGGL(ciderd_cook_kernel<false>, dim3(n_cand), dim3(CK_NT), 0, st, a);
    return ICZ_OK;
}

int icz_ciderd_cook_device(icz_ciderd_t* h, const int32_t* tok, const int32_t* ptr, int32_t n_cand, int32_t* ent_key_out,
                           int32_t* ent_order_out, double* ent_w_out, int32_t* ent_ptr_out, double* norm_out, int32_t* len_out, void* stream) {
    ICZ_REQUIRE(n_cand > 0 && (int64_t)n_cand * CD_MAXP < (1ll << 31), "icz_ciderd_cook_device: n_cand=%d out of range", n_cand);
    ICZ_REQUIRE(tok && ptr && ent_key_out && ent_order_out && ent_w_out && ent_ptr_out && norm_out && len_out,
                "icz_ciderd_cook_device: null argument");
    ICZ_REQUIRE(h, "icz_ciderd_cook_device: null handle");
    ICZ_TRY(cook_device_launch(reinterpret_cast<CiderD*>(h), tok, ptr, n_cand, ent_key_out, ent_order_out, ent_w_out, ent_ptr_out, norm_out,
                               len_out, (hipStream_t)stream));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// workspace of icz_ciderd_pairwise for n = n_img K candidates, 8-byte units first:
//   ent_w [240 n] f64 | norm [4 n] f64 | consensus [n] f64 | ent_key [240 n, 4] i32 | ent_order [240 n] i32 | ent_ptr [n + 1] i32 | len [n] i32
size_t icz_ciderd_pairwise_workspace_bytes(int32_t n_img, int32_t K) {
    if (n_img <= 0 || K < 2 || K > 8) return 0;
    const size_t n = (size_t)n_img * (size_t)K;
    return n * CD_MAXP * 8 + n * 4 * 8 + n * 8 + n * CD_MAXP * 16 + n * CD_MAXP * 4 + (n + 1) * 4 + n * 4 + 8;
}

int icz_ciderd_pairwise(icz_ciderd_t* h, const int32_t* tok, const int32_t* ptr, int32_t n_img, int32_t K, double* pair_out,
                        double* consensus_out, int32_t* best_out, void* workspace, size_t workspace_bytes, void* stream) {
    ICZ_REQUIRE(K >= 2 && K <= 8, "icz_ciderd_pairwise: K=%d candidates per image outside 2..8", K);
    ICZ_REQUIRE(n_img > 0 && (int64_t)n_img * K * CD_MAXP < (1ll << 31), "icz_ciderd_pairwise: n_img=%d out of range", n_img);
    ICZ_REQUIRE(tok && ptr && pair_out && workspace, "icz_ciderd_pairwise: null argument");
    ICZ_REQUIRE(h, "icz_ciderd_pairwise: null handle");
    ICZ_REQUIRE(workspace_bytes >= icz_ciderd_pairwise_workspace_bytes(n_img, K) && ((uintptr_t)workspace & 7) == 0,
                "icz_ciderd_pairwise: workspace of %zu bytes (need %zu, 8-byte aligned)", workspace_bytes,
                icz_ciderd_pairwise_workspace_bytes(n_img, K));
    CiderD* c = reinterpret_cast<CiderD*>(h);
    const size_t n = (size_t)n_img * (size_t)K;
    double* ent_w = reinterpret_cast<double*>(workspace);
    double* norm = ent_w + n * CD_MAXP;
    double* cons = norm + n * 4;
    int32_t* ent_key = reinterpret_cast<int32_t*>(cons + n);
    int32_t* ent_order = ent_key + n * CD_MAXP * 4;
    int32_t* ent_ptr = ent_order + n * CD_MAXP;
    int32_t* len = ent_ptr + n + 1;
    if (consensus_out) cons = consensus_out;
    hipStream_t st = (hipStream_t)stream;
    ICZ_TRY(cook_device_launch(c, tok, ptr, (int32_t)n, ent_key, ent_order, ent_w, ent_ptr, norm, len, st));
    CiderArgs a = {c->keys, c->idf, c->penalty, c->cap, c->default_idf, nullptr, nullptr, (int)n, 0, nullptr,
                   nullptr, ent_ptr, ent_key, ent_order, ent_w, norm, len, cons, K, tok, ptr, pair_out};
    hipLaunchKernelGGL(ciderd_kernel<SRC_CSR_PAIRS>, dim3((unsigned)n), dim3(64 * CD_NW), 0, st, a);
    if (best_out) hipLaunchKernelGGL(ciderd_best_kernel, dim3(cdiv(n_img, 256)), dim3(256), 0, st, (const double*)cons, (int)n_img, (int)K, best_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_ciderd_scores_csr(icz_ciderd_t* h, const int32_t* tok, const int32_t* ptr, int32_t n_img, int32_t K, const int32_t* img_slot,
                          const int32_t* img_ref_ptr, const int32_t* ref_ent_ptr, const int32_t* ent_key, const int32_t* ent_order,
                          const double* ent_w, const double* ref_norm, const int32_t* ref_len, double* scores_out, void* stream) {
    ICZ_REQUIRE(K >= 1 && K <= 8, "icz_ciderd_scores_csr: K=%d candidates per image outside 1..8", K);
    ICZ_REQUIRE(n_img > 0 && (int64_t)n_img * K < (1ll << 31), "icz_ciderd_scores_csr: n_img=%d out of range", n_img);
    ICZ_REQUIRE(tok && ptr && img_slot && img_ref_ptr && ref_ent_ptr && ent_key && ent_order && ent_w && ref_norm && ref_len && scores_out,
                "icz_ciderd_scores_csr: null argument");
    ICZ_REQUIRE(h, "icz_ciderd_scores_csr: null handle");
    CiderD* c = reinterpret_cast<CiderD*>(h);
    const int n = n_img * K;
    CiderArgs a = {c->keys, c->idf, c->penalty, c->cap, c->default_idf, nullptr, nullptr, n, 0, img_slot,
                   img_ref_ptr, ref_ent_ptr, ent_key, ent_order, ent_w, ref_norm, ref_len, scores_out, K, tok, ptr, nullptr};
    hipLaunchKernelGGL(ciderd_kernel<SRC_CSR>, dim3(n), dim3(64 * CD_NW), 0, (hipStream_t)stream, a);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_ngram_diversity(const int32_t* tok, const int32_t* ptr, int32_t n_img, int32_t K, int32_t* counts_out, void* stream) {
    ICZ_REQUIRE(K >= 1 && K <= DV_MAXK, "icz_ngram_diversity: K=%d candidates per image outside 1..%d", K, DV_MAXK);
    ICZ_REQUIRE(n_img > 0 && (int64_t)n_img * K < (1ll << 31), "icz_ngram_diversity: n_img=%d out of range", n_img);
    ICZ_REQUIRE(tok && ptr && counts_out, "icz_ngram_diversity: null argument");
    hipLaunchKernelGGL(ngram_diversity_kernel, dim3(n_img), dim3(DV_NT), 0, (hipStream_t)stream, tok, ptr, (int)n_img, (int)K, counts_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
