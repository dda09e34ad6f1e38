// SCST on samples drawn WITHOUT replacement (beyond the reference; include/icz.h "SCST on without-replacement samples"): the loss head
// that trains on the n distinct captions per image of stochastic beam search (sample_distinct) with the importance-weighted
// estimators of Kool, van Hoof and Welling ("Buy 4 REINFORCE Samples, Get a Baseline for Free!", 2019; "Estimating Gradients for
// Discrete Random Variables by Sampling without Replacement", ICLR 2020), in the place of xe_loss behind a training-mode xe_forward on
// the sampled captions.  Per image, slots 0..n-1 sorted by G descending; kappa = G of slot n - 1 (the threshold: that slot is no
// sample), the m = n - 1 slots in front of it are the samples; f = the CIDEr-D scores, phi the sampler's log-probabilities.  float64,
// sums in ascending slot order:
//   d_i = phi_i - kappa,  q_i = -expm1(-exp(d_i)),  log q_i = d_i - exp(d_i) / 2 where d_i < SWOR_D_SWITCH (the series
//   log((1 - e^-x) / x) = -x / 2 + x^2 / 24 - ..., cut behind its first term: x^2 / 24 <= e^-36 / 24 < 1e-17 there)
//   p_i = exp(phi_i),  w_i = exp(phi_i - log q_i),  W = sum w_j,  Bu = sum w_j f_j
//   "normalised": c_i = w_i / (W - w_i + p_i) (f_i - Bu / W)          "unbiased": c_i = w_i (f_i (1 + w_i - p_i) - Bu)
//   loss = -(1 / N) sum_img sum_{i < m} c_i logp_i,   logp_i = sum_{t < len_i} log softmax(z_{i,t})[y_{i,t}]
//   d loss / d z[row, t, v] = -(c_row / N) (1[v == y] - softmax(z)[v])                      (c is a constant of the backward pass)
// THE WEIGHTS USE THE SAMPLER'S EVALUATION-MODE phi; THE GRADIENT FLOWS THROUGH THE TRAINING-MODE FORWARD (dropout on): logp above is
// the stored forward's, and it enters the loss and the gradient only, never c.
// swor_weights_kernel fills coef [n_img n] = -c / N (0 in the threshold slot) and the per-image stats; swor_dlogits_kernel writes the
// gradient over the stored logits (the addressing of xe_loss_dlogits_kernel; the row's coefficient is coef[perm[b]], perm mapping
// the length-sorted row b of the forward back to img n + slot) and the target's log-prob of every (b, t); swor_finish_kernel sums
// them to {loss, sum c logp by image} in one fixed order.  No float atomics: two runs give the same bits.  In the softmax rows every
// exponent is taken behind its row's maximum; the weights' exponents are of phi <= 0, of -exp(d) <= 0 and of phi - log q (kappa up
// to the cut series, or at most -SWOR_D_SWITCH above phi), none of which float64 can overflow on.
#include <cmath>

#include "decoder_core.h"
#include "ens_sample.h"
#include "token_kernels.h"

namespace icz {

constexpr int SWOR_MIN_N = 3, SWOR_MAX_N = 8;
constexpr double SWOR_D_SWITCH = -18.0;

// One wave per image, lane = slot.  Every lane of a sample slot forms its own (p, w); the sums over the image's m samples are taken
// by every lane in ascending slot order from LDS.
__global__ __launch_bounds__(64) void swor_weights_kernel(const float* __restrict__ phi, const double* __restrict__ G,
                                                          const double* __restrict__ scores, int n, int estimator, double inv_n,
                                                          float* __restrict__ coef, double* __restrict__ stats) {
    __shared__ double s_w[SWOR_MAX_N], s_f[SWOR_MAX_N];
    const int img = blockIdx.x, lane = threadIdx.x, m = n - 1;
    const size_t r0 = (size_t)img * n;
    double p = 0.0, w = 0.0, f = 0.0;
    if (lane < m) {
        const double ph = (double)phi[r0 + lane], kappa = G[r0 + m];
        const double d = ph - kappa, ed = exp(d);
        const double logq = d < SWOR_D_SWITCH ? d - 0.5 * ed : log(-expm1(-ed));
        p = exp(ph);
        w = exp(ph - logq);
        f = scores[r0 + lane];
        s_w[lane] = w;
        s_f[lane] = f;
    }
    __syncthreads();
    double W = 0.0, Bu = 0.0;
    for (int j = 0; j < m; ++j) { W += s_w[j]; Bu += s_w[j] * s_f[j]; }
    const double base = Bu / W;
    if (lane < m) {
        const double c = estimator == ICZ_SWOR_NORMALISED ? w / (W - w + p) * (f - base) : w * (f * (1.0 + w - p) - Bu);
        coef[r0 + lane] = (float)(-c * inv_n);
    } else if (lane == m) {
        coef[r0 + lane] = 0.f;
    }
    if (lane == 0 && stats) {
        double s2 = 0.0;
        for (int j = 0; j < m; ++j) { const double r = s_w[j] / W; s2 += r * r; }
        stats[(size_t)img * 3 + 0] = W;
        stats[(size_t)img * 3 + 1] = base;
        stats[(size_t)img * 3 + 2] = 1.0 / s2;
    }
}

__device__ __forceinline__ void swor_lse_add(float& m, float& s, float y) {
    if (y > m) { s = s * expf(m - y) + 1.f; m = y; }
    else if (y != -INFINITY) s += expf(y - m);
}

// One workgroup (four waves) per (b, t) = row t B + b of the stored logits [T B, ldl] (ldl % 4 == 0, 16-byte aligned rows), active
// while b < rows.n[t].  An inactive row, and a row whose coefficient coef[perm[b]] is exactly 0 (a perm entry outside [0, n_coef)
// counts as 0), is written as zeros WITHOUT BEING READ and leaves 0 in loss_rows.  Else pass 1: 16-byte loads, an online (max,
// sum-exp) per thread, combined over the lanes by xor distance and the waves 0..3; lse = max + log(sum); the target's logit is read
// before any store.  Pass 2 re-reads the row (40 KB at V = 10 102: from L2) and writes c (1[v == y] - exp(x - lse)) over it, zeros in
// the pad columns [V, ldl); thread 0 leaves x[y] - lse in loss_rows[row].  Nothing of the row is kept in LDS: no cap on V.
__global__ __launch_bounds__(256) void swor_dlogits_kernel(float* __restrict__ logits, int V, int ldl, const int64_t* __restrict__ captions, int L,
                                                           int B, XeRows rows, const float* __restrict__ coef, int n_coef,
                                                           const int32_t* __restrict__ perm, float* __restrict__ loss_rows) {
    __shared__ float sm[4], ss[4];
    const int b = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int row = t * B + b;
    float* l = logits + (size_t)row * ldl;
    float c = 0.f;
    if (b < rows.n[t]) {
        const int r = perm[b];
        if (r >= 0 && r < n_coef) c = coef[r];
    }
    if (c == 0.f) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int v = tid * 4; v < ldl; v += 1024) *reinterpret_cast<f32x4*>(l + v) = z;
        if (tid == 0) loss_rows[row] = 0.f;
        return;
    }
    const int64_t y = captions[(size_t)b * L + t + 1];
    const bool y_ok = y >= 0 && y < (int64_t)V;
    const float xy = y_ok ? l[y] : 0.f;
    float mx = -INFINITY, se = 0.f;
    for (int v = tid * 4; v < V; v += 1024) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(l + v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (v + j < V) swor_lse_add(mx, se, x[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_combine(mx, se, __shfl_xor(mx, o, 64), __shfl_xor(se, o, 64));
    if ((tid & 63) == 0) { sm[tid >> 6] = mx; ss[tid >> 6] = se; }
    __syncthreads();                  // also: every thread has read its part of the row and the target's logit
    mx = sm[0]; se = ss[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) lse_combine(mx, se, sm[w], ss[w]);
    const float lse = mx + logf(se);
    for (int v = tid * 4; v < ldl; v += 1024) {
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (v < V) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(l + v);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v + j < V) g[j] = c * (((int64_t)(v + j) == y ? 1.f : 0.f) - expf(x[j] - lse));
        }
        *reinterpret_cast<f32x4*>(l + v) = g;
    }
    if (tid == 0) loss_rows[row] = y_ok ? xy - lse : 0.f;
}

// {loss, sum c logp by image} in one fixed order, one workgroup.  cs [n_img n] (float64 scratch) is zeroed; the thread of sorted row b
// sums the row's target log-probs over its active steps in ascending t (float64) and leaves coef logp in cs[perm[b]]; the thread of
// an image adds its slots in ascending order; the images are added by thread i over i, i + 256, ..., then the lanes by xor distance
// and the waves 0..3.  loss_out [1 + n_img] = {loss, the per-image sums}.
__global__ __launch_bounds__(256) void swor_finish_kernel(const float* __restrict__ loss_rows, int B, int T, XeRows rows,
                                                          const float* __restrict__ coef, int n, int n_img,
                                                          const int32_t* __restrict__ perm, double* __restrict__ cs, float* __restrict__ loss_out) {
    __shared__ double sd[4];
    const int tid = threadIdx.x, n_coef = n * n_img;
    for (int i = tid; i < n_coef; i += 256) cs[i] = 0.0;
    __syncthreads();
    for (int b = tid; b < B; b += 256) {
        const int r = perm[b];
        if (r < 0 || r >= n_coef) continue;
        double s = 0.0;
        for (int t = 0; t < T; ++t)
            if (b < rows.n[t]) s += (double)loss_rows[(size_t)t * B + b];
        cs[r] = (double)coef[r] * s;
    }
    __syncthreads();
    double tot = 0.0;
    for (int i = tid; i < n_img; i += 256) {
        double s = 0.0;
        for (int j = 0; j < n - 1; ++j) s += cs[(size_t)i * n + j];
        loss_out[1 + i] = (float)s;
        tot += s;
    }
    tot = wave_sum_d(tot);
    if ((tid & 63) == 0) sd[tid >> 6] = tot;
    __syncthreads();
    if (tid == 0) loss_out[0] = (float)(((sd[0] + sd[1]) + sd[2]) + sd[3]);
}

// Rules 1 - 6 of icz_swor_opts (include/icz.h) in their documented order
int swor_args(const char* who, const icz_swor_opts* o, int rows, SworArgs* out) {
    ICZ_REQUIRE(o, "%s: null options", who);
    ICZ_REQUIRE(o->n >= SWOR_MIN_N && o->n <= SWOR_MAX_N, "%s: n=%d slots per image outside %d..%d", who, o->n, SWOR_MIN_N, SWOR_MAX_N);
    ICZ_REQUIRE(o->estimator == ICZ_SWOR_NORMALISED || o->estimator == ICZ_SWOR_UNBIASED, "%s: estimator=%d (0 normalised, 1 unbiased)", who,
                o->estimator);
    ICZ_REQUIRE(std::isfinite(o->n_img_global) && o->n_img_global >= 0.f, "%s: n_img_global %g not finite and >= 0", who,
                (double)o->n_img_global);
    ICZ_REQUIRE(rows >= 1 && rows % (o->n - 1) == 0, "%s: %d rows are not a positive multiple of the n - 1 = %d samples per image", who, rows,
                o->n - 1);
    ICZ_REQUIRE(o->phi && o->G && o->scores && o->perm, "%s: null phi, G, scores or perm", who);
    if (out) *out = SworArgs{o->n, o->estimator, o->n_img_global, o->phi, o->G, o->scores, o->perm, o->stats_out};
    return ICZ_OK;
}

int launch_swor_objective(const SworArgs& a, float* logits, int V, int ldl, const int64_t* captions, int L, int B, int T, const int* rows_t,
                          const SworScratch& w, float* loss_rows, float* loss_out, hipStream_t st) {
    ICZ_REQUIRE(T <= XE_MAX_T, "swor objective: %d steps exceed %d", T, XE_MAX_T);
    ICZ_REQUIRE(ldl % 4 == 0 && ((uintptr_t)logits & 15) == 0, "swor objective: the kernels move 16 bytes at a time: ldl=%d, logits %p", ldl,
                (void*)logits);
    const int n_img = B / (a.n - 1);
    const double inv_n = 1.0 / (a.n_img_global > 0.f ? (double)a.n_img_global : (double)n_img);
    XeRows xr = {};
    for (int t = 0; t < T; ++t) xr.n[t] = rows_t[t];
    hipLaunchKernelGGL(swor_weights_kernel, dim3(n_img), dim3(64), 0, st, a.phi, a.G, a.scores, a.n, a.estimator, inv_n, w.coef, a.stats_out);
    hipLaunchKernelGGL(swor_dlogits_kernel, dim3(B, T), dim3(256), 0, st, logits, V, ldl, captions, L, B, xr, (const float*)w.coef, n_img * a.n,
                       a.perm, loss_rows);
    hipLaunchKernelGGL(swor_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)loss_rows, B, T, xr, (const float*)w.coef, a.n, n_img, a.perm,
                       w.cs, loss_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// rules 10 - 12 of icz_*_xe_backward_swor against the stored XE forward pass (rule 9, that there is one: check_loss_head); nothing is
// queued and the stored forward stays usable
int CaptionHead::check_swor(const char* who, int rows) const {
    ICZ_REQUIRE(cur_train, "%s xe_backward_swor: the stored forward pass ran in evaluation mode: it keeps no state for a backward pass", who);
    ICZ_REQUIRE(cur_ss_prob <= 0.f, "%s xe_backward_swor: the stored forward pass ran with scheduled sampling (ss_prob %g): it was fed other "
                "tokens than the sampled captions", who, (double)cur_ss_prob);
    ICZ_REQUIRE(rows == cur_B, "%s xe_backward_swor: %d sample rows, the stored forward pass has %d", who, rows, cur_B);
    return ICZ_OK;
}

int CaptionHead::swor_loss(const SworArgs& a, float* logits, int V, int ldl, float* loss_out, hipStream_t st) {
    const SworScratch w = {swor_coef, swor_cs};
    return launch_swor_objective(a, logits, V, ldl, cur_captions, cur_L, cur_B, cur_T, rows_t.data(), w, loss_rows, loss_out, st);
}

}  // namespace icz

using namespace icz;
extern "C" {

int icz_swor_check(const icz_swor_opts* opts, int32_t rows, const int32_t* perm_host, const int32_t* lengths_host) {
    const char* who = "icz_swor_check";
    ICZ_TRY(swor_args(who, opts, rows, nullptr));
    const int n = opts->n, total = rows / (n - 1) * n;
    if (perm_host) {
        std::vector<uint8_t> seen((size_t)total, 0);
        for (int b = 0; b < rows; ++b) {
            const int r = perm_host[b];
            ICZ_REQUIRE(r >= 0 && r < total && r % n != n - 1 && !seen[r], "%s: perm[%d]=%d is outside 0..%d, a threshold slot or taken twice", who, b,
                        r, total - 1);
            seen[r] = 1;
        }
    }
    if (lengths_host)
        for (int b = 0; b < rows; ++b)
            ICZ_REQUIRE(lengths_host[b] >= 1 && (b == 0 || lengths_host[b] <= lengths_host[b - 1]),
                        "%s: lengths[%d]=%d below 1 or not sorted in decreasing order", who, b, lengths_host[b]);
    return ICZ_OK;
}

int icz_test_swor_objective(const icz_swor_opts* opts, float* logits, int32_t V, int32_t ldl, const int64_t* captions, int32_t L, int32_t B,
                            int32_t T, const int32_t* rows_t, float* coef_out, float* loss_rows, float* loss_out, void* stream) {
    const char* who = "icz_test_swor_objective";
    SworArgs a;
    ICZ_TRY(swor_args(who, opts, B, &a));
    ICZ_REQUIRE(logits && captions && rows_t && coef_out && loss_rows && loss_out, "%s: null argument", who);
    ICZ_REQUIRE(V >= 1 && ldl >= V, "%s: V=%d, ldl=%d", who, V, ldl);
    ICZ_REQUIRE(T >= 1 && T <= XE_MAX_T && L > T, "%s: T=%d outside 1..%d or not below L=%d", who, T, XE_MAX_T, L);
    ICZ_REQUIRE(B <= 65535 && (long)B * T <= (1 << 20), "%s: B=%d, T=%d", who, B, T);
    for (int t = 0; t < T; ++t) ICZ_REQUIRE(rows_t[t] >= 0 && rows_t[t] <= B, "%s: rows_t[%d]=%d outside 0..B", who, t, rows_t[t]);
    hipStream_t st = (hipStream_t)stream;
    double* cs = nullptr;             // the finish kernel's float64 scratch
    ICZ_CHECK_HIP(hipMallocAsync((void**)&cs, sizeof(double) * (size_t)(B / (a.n - 1)) * a.n, st));
    const SworScratch w = {coef_out, cs};
    const int status = launch_swor_objective(a, logits, V, ldl, captions, L, B, T, rows_t, w, loss_rows, loss_out, st);
    ICZ_CHECK_HIP(hipFreeAsync(cs, st));
    return status;
}

}  // extern "C"
