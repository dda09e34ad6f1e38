// Word-level knowledge distillation (beyond the reference): one student decoder is trained on the word distribution of an ensemble
// of M = 1..4 teachers, q[v] = sum_m w_m softmax(z_m / tau)[v] (the probabilities averaged, as the ensemble decodes), mixed with the
// label-smoothing loss of the XE step:
//   loss = ((1 - alpha) sum_rows hard + alpha sum_rows kd) / N,   kd = tau^2 KL(q || softmax(s / tau)),   hard = xe_loss_dlogits_kernel's
//   d s  = ((1 - alpha) (softmax(s) - true) + alpha tau (softmax(s / tau) - q)) / N
// distill_loss_dlogits_kernel forms q in registers from the teachers' packed logits and writes d s over the student's stored logits;
// CaptionHead::distill_loss puts it in the place of xe_loss (LossHead::XE_DISTILL), and the three decoders' backward() run their
// backward pass behind it (butd_train.hip, aoa_train.hip, nic.hip).
#include <cmath>

#include "ens_sample.h"
#include "token_kernels.h"

namespace icz {

__device__ __forceinline__ void online_lse_add(float& m, float& s, float y) {
    if (y > m) { s = s * expf(m - y) + 1.f; m = y; }
    else if (y != -INFINITY) s += expf(y - m);
}
// the workgroup's (max, sum-exp) pairs -> log-sum-exp, combined in a fixed order (lanes by xor distance, then waves 0..3)
__device__ __forceinline__ float block_lse_256(float m, float s, float* sm, float* ss) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_combine(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = m; ss[threadIdx.x >> 6] = s; }
    __syncthreads();
    m = sm[0]; s = ss[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) lse_combine(m, s, sm[w], ss[w]);
    __syncthreads();                  // sm / ss are rewritten by the next reduction
    return m + logf(s);
}

// One workgroup (four waves) per (b, t) = row t B + b of the student's logits s [T B, ld_s]; d s goes to the same row of out
// [T B, ld_out] (out may be s: every element is read and written by the same thread, and pass 2 starts behind pass 1's barrier).
// Inactive rows (b >= rows.n[t]) and the pad columns [V, ld_out) become zeros: the backward GEMMs read every row.  The teachers' row
// of (t, b) is packed row rows.off[t] + b of each member's [N, ld_m] tensor; the target is targets[row] (the kernel alone) or
// captions[b, t + 1].
// Pass 1: online (max, sum-exp) of the student's row at scale 1 and at 1 / tau in one read, and of every member of non-zero weight
// at 1 / tau (a member of weight 0 is never read).  Pass 2: q[v] from the members' terms log w_m + z_m[v] / tau - lse_m, shifted by the
// largest term over m as ensemble_logprob_kernel does; both loss terms; d s.  The rows are re-read from cache in pass 2 (a row of
// 10 102 floats is 40 KB: M + 1 of them stay in L2, and LDS would cap V); q never leaves the registers.  Every exponent is taken
// behind its row's maximum.  The per-row losses go to hard_rows / kd_rows, summed later in fixed order: no float atomics.
constexpr int DISTILL_MAX_T = XE_MAX_T;
struct DistillRows { int n[DISTILL_MAX_T]; int off[DISTILL_MAX_T]; };
__global__ __launch_bounds__(256) void distill_loss_dlogits_kernel(const float* s_in, int ld_s, float* out, int ld_out, DistillArgs a,
                                                                   const int64_t* __restrict__ targets, const int64_t* __restrict__ captions,
                                                                   int L, int B, DistillRows rows, float inv_n_host,
                                                                   const float* __restrict__ n_dev, float* __restrict__ hard_rows,
                                                                   float* __restrict__ kd_rows) {
    __shared__ float sm[4], ss[4];
    const int b = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, V = a.ens.V;
    const int row = t * B + b;
    float* o = out + (size_t)row * ld_out;
    if (b >= rows.n[t]) {
        for (int v = tid; v < ld_out; v += 256) o[v] = 0.f;
        return;
    }
    const float inv_n = (n_dev && n_dev[0] > 0.f) ? 1.0f / n_dev[0] : inv_n_host;
    const float tau = a.temperature, inv_tau = 1.0f / tau, alpha = a.alpha;
    const int trow = rows.off[t] + b;
    const LogitsView sv = {s_in, nullptr, 0, ld_s, 1};
    const bool svec = ens_vec_ok(sv);
    float lse1, lseT;
    {
        float m1 = -INFINITY, s1 = 0.f, mT = -INFINITY, sT = 0.f;
        for (int v = tid * 4; v < V; v += 1024) {
            const f32x4 x = ens_load4(sv, row, v, V, svec);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                online_lse_add(m1, s1, x[j]);
                online_lse_add(mT, sT, x[j] * inv_tau);
            }
        }
        lse1 = block_lse_256(m1, s1, sm, ss);
        lseT = block_lse_256(mT, sT, sm, ss);
    }
    float shift[ENS_MAX_M];           // log w_m - lse_m (-inf: the member is not read)
    bool vec[ENS_MAX_M];
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) {
        shift[m] = -INFINITY;
        vec[m] = false;
        if (m >= a.ens.M || a.ens.logw[m] == -INFINITY) continue;
        const LogitsView l = a.ens.m[m];
        vec[m] = ens_vec_ok(l);
        float mx = -INFINITY, s = 0.f;
        for (int v = tid * 4; v < V; v += 1024) {
            const f32x4 x = ens_load4(l, trow, v, V, vec[m]);
#pragma unroll
            for (int j = 0; j < 4; ++j) online_lse_add(mx, s, x[j] * inv_tau);
        }
        shift[m] = a.ens.logw[m] - block_lse_256(mx, s, sm, ss);
    }
    const int64_t tg = targets ? targets[row] : captions[(size_t)b * L + t + 1];
    const float conf = 1.f - a.smoothing, low = a.smoothing / (float)(V - 1);
    const float lconf = conf > 0.f ? logf(conf) : 0.f, llow = low > 0.f ? logf(low) : 0.f;
    const float c_hard = (1.f - alpha) * inv_n, c_kd = alpha * tau * inv_n;
    const bool ovec = (ld_out & 3) == 0 && ((uintptr_t)out & 15) == 0;
    float hard = 0.f, kd = 0.f;
    for (int v = tid * 4; v < ld_out; v += 1024) {
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (v < V) {
            const f32x4 x = ens_load4(sv, row, v, V, svec);
            f32x4 term[ENS_MAX_M];
            f32x4 top = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int m = 0; m < ENS_MAX_M; ++m) {
                if (shift[m] == -INFINITY) continue;
                term[m] = ens_load4(a.ens.m[m], trow, v, V, vec[m]) * inv_tau + shift[m];
#pragma unroll
                for (int j = 0; j < 4; ++j) top[j] = fmaxf(top[j], term[m][j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (v + j >= V) continue;
                float q = 0.f, lq = -INFINITY;
                if (top[j] != -INFINITY) {
                    float s = 0.f;
#pragma unroll
                    for (int m = 0; m < ENS_MAX_M; ++m)
                        if (shift[m] != -INFINITY && term[m][j] != -INFINITY) s += expf(term[m][j] - top[j]);
                    lq = top[j] + logf(s);
                    q = expf(lq);
                }
                const float lp1 = x[j] - lse1, lpT = x[j] * inv_tau - lseT;
                const bool hit = (int64_t)(v + j) == tg;
                const float tr = hit ? conf : low;
                if (tr > 0.f) hard += tr * ((hit ? lconf : llow) - lp1);
                if (q > 0.f) kd += q * (lq - lpT);
                g[j] = c_hard * (expf(lp1) - tr) + c_kd * (expf(lpT) - q);
            }
        }
        if (ovec) {                   // (ld_out % 4 == 0: the four columns are inside the row)
            *reinterpret_cast<f32x4*>(o + v) = g;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v + j < ld_out) o[v + j] = g[j];
        }
    }
    hard = block_sum_256(hard, sm);
    kd = block_sum_256(kd, sm);
    if (tid == 0) { hard_rows[row] = hard; kd_rows[row] = tau * tau * kd; }
}

// out3 = {((1 - alpha) H + alpha K) / N, H / N, K / N}: the two arrays of n per-row terms summed in fixed order by one workgroup
__global__ __launch_bounds__(256) void distill_sum_kernel(const float* __restrict__ hard_rows, const float* __restrict__ kd_rows, int n, float alpha,
                                                          float scale_host, const float* __restrict__ n_dev, float* __restrict__ out3) {
    __shared__ float smf[4];
    const float scale = (n_dev && n_dev[0] > 0.f) ? 1.0f / n_dev[0] : scale_host;
    float h = 0.f, k = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { h += hard_rows[i]; k += kd_rows[i]; }
    h = block_sum_256(h, smf);
    k = block_sum_256(k, smf);
    if (threadIdx.x == 0) {
        out3[0] = ((1.f - alpha) * h + alpha * k) * scale;
        out3[1] = h * scale;
        out3[2] = k * scale;
    }
}
// alpha = 0: the XE loss is the whole loss
__global__ void distill_hard_only_kernel(float* __restrict__ out3) { out3[1] = out3[0]; out3[2] = 0.f; }

// The rules of icz_distill_opts (include/icz.h), in their documented order; V < 0: no handle yet, the rule that needs the vocabulary
// waits for one.
int distill_args(const char* who, const icz_distill_opts* o, int V, DistillArgs* out) {
    ICZ_REQUIRE(o, "%s: null options", who);
    ICZ_REQUIRE(o->M >= 1 && o->M <= ENS_MAX_M, "%s: M=%d teachers outside 1..%d", who, o->M, ENS_MAX_M);
    ICZ_REQUIRE(o->alpha >= 0.f && o->alpha <= 1.f, "%s: alpha %g outside [0, 1]", who, (double)o->alpha);
    ICZ_REQUIRE(o->temperature >= 0.25f && o->temperature <= 8.f, "%s: temperature %g outside [0.25, 8]", who, (double)o->temperature);
    ICZ_REQUIRE(o->smoothing >= 0.f && o->smoothing < 1.f, "%s: smoothing %g outside [0, 1)", who, (double)o->smoothing);
    ICZ_REQUIRE(o->teacher && o->ld, "%s: null teacher or ld array", who);
    for (int m = 0; m < o->M; ++m) ICZ_REQUIRE(o->teacher[m], "%s: teacher %d is null", who, m);
    if (V >= 0)
        for (int m = 0; m < o->M; ++m) ICZ_REQUIRE(o->ld[m] >= V, "%s: ld[%d]=%d below the vocabulary size %d", who, m, o->ld[m], V);
    *out = {};
    ICZ_TRY(ens_log_weights(who, o->weights, o->M, out->ens.logw));
    for (int m = 0; m < o->M; ++m) out->ens.m[m] = LogitsView{o->teacher[m], nullptr, 0, o->ld[m], 1};
    out->ens.M = o->M;
    out->ens.V = V;
    out->alpha = o->alpha; out->temperature = o->temperature; out->smoothing = o->smoothing;
    return ICZ_OK;
}

int CaptionHead::require_teacher_forced(const char* who) const {
    ICZ_REQUIRE(cur_ss_prob <= 0.f, "%s: the stored forward pass ran with scheduled sampling (ss_prob %g): the teachers were fed other "
                "tokens than the student", who, (double)cur_ss_prob);
    return ICZ_OK;
}

int CaptionHead::distill_loss(const DistillArgs& a, float n_tokens_global, float* logits, int V, int ldl, float* loss_out3, hipStream_t st) {
    if (a.alpha == 0.f) {             // today's launches: no teacher is read
        ICZ_TRY(xe_loss(a.smoothing, n_tokens_global, logits, V, ldl, loss_out3, st));
        hipLaunchKernelGGL(distill_hard_only_kernel, dim3(1), dim3(1), 0, st, loss_out3);
        ICZ_CHECK_HIP(hipGetLastError());
        return ICZ_OK;
    }
    const int B = cur_B, T = cur_T;
    ICZ_REQUIRE(T <= DISTILL_MAX_T, "xe_backward_distill: %d steps exceed %d", T, DISTILL_MAX_T);
    const float n = n_tokens_global > 0.f ? n_tokens_global : (float)n_tokens;
    const float* n_dev = n_tokens_global < 0.f ? d_msum : nullptr;      // < 0: the device scalar handed over by *_set_*_global
    ICZ_CHECK_HIP(hipMemsetAsync(loss_rows, 0, sizeof(float) * T * B, st));
    ICZ_CHECK_HIP(hipMemsetAsync(kd_rows, 0, sizeof(float) * T * B, st));
    DistillRows dr = {};
    for (int t = 0, acc = 0; t < T; ++t) { dr.n[t] = rows_t[t]; dr.off[t] = acc; acc += rows_t[t]; }
    DistillArgs k = a;
    k.ens.V = V;
    hipLaunchKernelGGL(distill_loss_dlogits_kernel, dim3(B, T), dim3(256), 0, st, (const float*)logits, ldl, logits, ldl, k,
                       (const int64_t*)nullptr, cur_captions, cur_L, B, dr, 1.0f / n, n_dev, loss_rows, kd_rows);
    hipLaunchKernelGGL(distill_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)loss_rows, (const float*)kd_rows, T * B, a.alpha, 1.0f / n,
                       n_dev, loss_out3);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // namespace icz

using namespace icz;
extern "C" {

int icz_distill_check(const icz_distill_opts* opts, int32_t V) {
    DistillArgs a;
    ICZ_REQUIRE(V > 3, "icz_distill_check: vocabulary size %d", V);
    return distill_args("icz_distill_check", opts, V, &a);
}

int icz_distill_loss(const float* student, int32_t ld_s, const icz_distill_opts* opts, const int64_t* targets, int32_t rows, int32_t V,
                     float n_tokens, float* dlogits_out, int32_t ld_out, float* loss_out3, void* stream) {
    const char* who = "icz_distill_loss";
    DistillArgs a;
    ICZ_REQUIRE(V > 3, "%s: vocabulary size %d", who, V);
    ICZ_TRY(distill_args(who, opts, V, &a));
    ICZ_REQUIRE(student && targets && dlogits_out && loss_out3, "%s: null argument", who);
    ICZ_REQUIRE(rows > 0 && ld_s >= V && ld_out >= V && n_tokens > 0.f, "%s: rows=%d ld_s=%d ld_out=%d n_tokens=%g for V=%d", who, rows, ld_s,
                ld_out, (double)n_tokens, V);
    if (a.alpha == 0.f) a.ens.M = 0;  // no teacher is read: q = 0, kd = 0
    hipStream_t st = (hipStream_t)stream;
    float* part = nullptr;            // the per-row losses: hard [rows] | kd [rows]
    ICZ_CHECK_HIP(hipMallocAsync((void**)&part, sizeof(float) * 2 * rows, st));
    DistillRows dr = {};
    dr.n[0] = rows;
    hipLaunchKernelGGL(distill_loss_dlogits_kernel, dim3(rows, 1), dim3(256), 0, st, student, ld_s, dlogits_out, ld_out, a, targets,
                       (const int64_t*)nullptr, 0, rows, dr, 1.0f / n_tokens, (const float*)nullptr, part, part + rows);
    hipLaunchKernelGGL(distill_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)part, (const float*)(part + rows), rows, a.alpha,
                       1.0f / n_tokens, (const float*)nullptr, loss_out3);
    const hipError_t le = hipGetLastError();
    ICZ_CHECK_HIP(hipFreeAsync(part, st));
    ICZ_CHECK_HIP(le);
    return ICZ_OK;
}

}  // extern "C"
