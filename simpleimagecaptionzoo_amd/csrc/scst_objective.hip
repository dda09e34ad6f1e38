// SCST objectives beyond RewardCriterion (beyond the reference; include/icz.h "SCST objectives"): a minimum-risk term over the K
// samples of an image and an entropy bonus on the per-step word distribution, both in the place of the REINFORCE loss head of a
// stored rollout (CaptionHead::reinforce, decoder_core.hip).  Rows r = img K + k, mask[r, 0] = 1, mask[r, t] = seq[r, t - 1] > 0.
//   risk:    s_r = sum_t mask logp,  Q_r = softmax_k(a s)_r,  L_img = sum_k Q_k c_k,  obj = sum_img L_img / N,
//            coef[r, t] = mask a Q_r (c_r - L_img) / N = d obj / d logp                                  (c_r = -scores[r])
//   entropy: H[r, t] = -sum_v p_v log p_v,  ent = sum(mask H) / M,  loss = obj - b ent,
//            dlogits[row, v] = coef (1[v == draw] - p_v) + (b mask / M) p_v (log p_v + H)
// scst_risk_kernel fills coef as reinforce_loss_kernel does for a reward; scst_entropy_dlogits_kernel stands in for
// reinforce_dlogits_kernel when b > 0; scst_finish_kernel sums the per-row entropies in a fixed order.  No float atomics: two runs
// give the same bits.  CaptionHead::scst_objective puts them in the place of reinforce (LossHead::ROLLOUT with an objective), and the
// three decoders' backward() run their backward pass behind it (butd_train.hip, aoa_train.hip, nic.hip).
#include <cmath>

#include "decoder_core.h"
#include "token_kernels.h"

namespace icz {

constexpr int SCST_MAX_K = 8;

// One wave per image.  Lane k < K sums its row's masked log-probs in float64 in ascending t and counts its mask; every lane then
// forms Q over the image's K rows in the same fixed order (shifted by the largest a s_j, j ascending) and the lanes share the K T
// elements of coef.  L_img and the image's mask count go to per-image slots: scst_risk_sum_kernel adds them in a fixed order.
__global__ __launch_bounds__(64) void scst_risk_kernel(const float* __restrict__ logp, const int64_t* __restrict__ seq,
                                                       const double* __restrict__ scores, int K, int T, double alpha, double inv_n,
                                                       float* __restrict__ coef, double* __restrict__ L_img, int* __restrict__ m_img) {
    __shared__ double s_s[SCST_MAX_K];
    __shared__ int s_m[SCST_MAX_K];
    const int img = blockIdx.x, lane = threadIdx.x;
    const size_t r0 = (size_t)img * K;
    if (lane < K) {
        const size_t o = (r0 + lane) * T;
        double s = 0.0;
        int m = 0;
        for (int t = 0; t < T; ++t)
            if (t == 0 || seq[o + t - 1] > 0) { s += (double)logp[o + t]; ++m; }
        s_s[lane] = s;
        s_m[lane] = m;
    }
    __syncthreads();
    double mx = -INFINITY;
    for (int j = 0; j < K; ++j) mx = fmax(mx, alpha * s_s[j]);
    double e[SCST_MAX_K], z = 0.0;
#pragma unroll
    for (int j = 0; j < SCST_MAX_K; ++j) {
        e[j] = j < K ? exp(alpha * s_s[j] - mx) : 0.0;
        z += e[j];                        // (the lanes past K add zeros: the order over j < K is the ascending one)
    }
    double L = 0.0;
#pragma unroll
    for (int j = 0; j < SCST_MAX_K; ++j)
        if (j < K) { e[j] /= z; L += e[j] * -scores[r0 + j]; }
    for (int i = lane; i < K * T; i += 64) {
        const int k = i / T, t = i - k * T;
        const size_t o = (r0 + k) * T + t;
        const bool on = t == 0 || seq[o - 1] > 0;
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < SCST_MAX_K; ++j) q = j == k ? e[j] : q;      // (no runtime-indexed register array)
        coef[o] = on ? (float)(alpha * q * (-scores[r0 + k] - L) * inv_n) : 0.f;
    }
    if (lane == 0) {
        int m = 0;
        for (int j = 0; j < K; ++j) m += s_m[j];
        L_img[img] = L;
        m_img[img] = m;
    }
}

// obj = sum_img L_img / N and the local mask sum, one workgroup: thread i adds the images i, i + 256, ... in ascending order, then the
// lanes by xor distance and the waves 0..3 -- one fixed order
__global__ __launch_bounds__(256) void scst_risk_sum_kernel(const double* __restrict__ L_img, const int* __restrict__ m_img, int n_img,
                                                            double inv_n, float* __restrict__ obj_out, float* __restrict__ msum_loc) {
    __shared__ double sd[4];
    __shared__ int si[4];
    double s = 0.0;
    int m = 0;
    for (int i = threadIdx.x; i < n_img; i += 256) { s += L_img[i]; m += m_img[i]; }
    s = wave_sum_d(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
    if ((threadIdx.x & 63) == 0) { sd[threadIdx.x >> 6] = s; si[threadIdx.x >> 6] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        obj_out[0] = (float)((((sd[0] + sd[1]) + sd[2]) + sd[3]) * inv_n);
        msum_loc[0] = (float)(si[0] + si[1] + si[2] + si[3]);
    }
}

// M of the entropy term: the global mask sum (a device scalar, > 0) or the local one
__device__ __forceinline__ float scst_mask_sum(const float* msum_dev, const float* msum_loc) {
    const float g = msum_dev ? msum_dev[0] : 0.f;
    return g > 0.f ? g : msum_loc[0];
}

// One workgroup of four waves per stored row (row = t stride + row0 + b, stride = Bs or B as reinforce_dlogits_kernel addresses a merged
// chain); nothing of the row is kept in LDS: V is not bounded by it.  A dead row (in front of row0, draw < 0, or mask = 0, derived
// from seq here) is written as zeros without being read -- it may hold anything, steps behind the early-out included.
// Pass 1: 16-byte loads (ldl % 4 == 0, 16-byte aligned rows), S = sum_v p_v (l_v - lse) with p_v = exp(l_v - lse): fp32 terms,
// float64 sums per thread, then the lanes by xor distance and the waves 0..3, one fixed order (score_tokens_kernel's).  A column with
// p_v == 0 adds exactly 0: no log(p) is taken.  H = -S.
// Pass 2 re-reads the row (40 KB at V = 10 102: from L2) and writes coef (1[v == draw] - p_v) + w p_v ((l_v - lse) + H), w = b / M,
// over it, zeros in the pad columns [V, ldl); thread 0 leaves H in ent_rows[row] for scst_finish_kernel.
__global__ __launch_bounds__(256) void scst_entropy_dlogits_kernel(float* __restrict__ logits, int V, int ldl, const int32_t* __restrict__ draw,
                                                                   const float* __restrict__ lse, const float* __restrict__ coef,
                                                                   const int64_t* __restrict__ seq, int B, int T, int Bs, int row0,
                                                                   float weight, const float* __restrict__ msum_dev,
                                                                   const float* __restrict__ msum_loc, float* __restrict__ ent_rows) {
    __shared__ double sd[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int stride = Bs > 0 ? Bs : B;
    const int t = row / stride, b = row % stride - row0;
    float* l = logits + (size_t)row * ldl;
    const int d = draw[row];
    const bool live = b >= 0 && d >= 0 && (t == 0 || seq[(size_t)b * T + t - 1] > 0);
    if (!live) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int v = tid * 4; v < ldl; v += 1024) *reinterpret_cast<f32x4*>(l + v) = z;
        if (tid == 0) ent_rows[row] = 0.f;
        return;
    }
    const float ls = lse[row];
    double s = 0.0;
    for (int v = tid * 4; v < V; v += 1024) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(l + v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dl = x[j] - ls, p = expf(dl);
            if (v + j < V && p > 0.f) s += (double)(p * dl);
        }
    }
    s = wave_sum_d(s);
    if ((tid & 63) == 0) sd[tid >> 6] = s;
    __syncthreads();
    const float H = (float)-(((sd[0] + sd[1]) + sd[2]) + sd[3]);
    const float c = coef[(size_t)b * T + t];
    const float w = weight / scst_mask_sum(msum_dev, msum_loc);
    for (int v = tid * 4; v < ldl; v += 1024) {
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (v < V) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(l + v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (v + j >= V) continue;
                const float dl = x[j] - ls, p = expf(dl);
                g[j] = c * ((v + j == d ? 1.f : 0.f) - p) + (p > 0.f ? w * p * (dl + H) : 0.f);
            }
        }
        *reinterpret_cast<f32x4*>(l + v) = g;
    }
    if (tid == 0) ent_rows[row] = H;
}

// The tail of every objective but today's: out3 = {obj - b ent, obj, ent}, the local mask sum and the optional ent_out [B, T].
// ent_rows null (b = 0): ent = 0.  Else ent = sum over the rollout's (b, t) of ent_rows (0 on dead rows) / M: thread i adds the
// elements i, i + 256, ... of the [B, T] order in float64, then the lanes and the waves in one fixed order.
__global__ __launch_bounds__(256) void scst_finish_kernel(const float* __restrict__ ent_rows, int B, int T, int Bs, int row0, float weight,
                                                          const float* __restrict__ msum_dev, const float* __restrict__ msum_loc,
                                                          const float* obj_src, float* out3, float* __restrict__ ent_out,
                                                          float* __restrict__ msum_out) {
    __shared__ double sd[4];
    const int stride = Bs > 0 ? Bs : B;
    double s = 0.0;
    for (int i = threadIdx.x; i < B * T; i += 256) {
        const int b = i / T, t = i - b * T;
        const float h = ent_rows ? ent_rows[(size_t)t * stride + row0 + b] : 0.f;
        s += (double)h;
        if (ent_out) ent_out[i] = h;
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sd[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float obj = obj_src[0];
        float ent = 0.f;
        if (ent_rows) ent = (float)((((sd[0] + sd[1]) + sd[2]) + sd[3]) / (double)scst_mask_sum(msum_dev, msum_loc));
        out3[0] = ent_rows ? obj - weight * ent : obj;
        out3[1] = obj;
        out3[2] = ent;
        if (msum_out) msum_out[0] = msum_loc[0];
    }
}
// today's head has written out3[0] = loss: obj = loss, ent = 0
__global__ void scst_reinforce_only_kernel(float* __restrict__ out3) { out3[1] = out3[0]; out3[2] = 0.f; }

// The rules of icz_scst_objective (include/icz.h) in their documented order
int scst_objective_args(const char* who, const icz_scst_objective* o, int rows, int T, ScstObjective* out) {
    ICZ_REQUIRE(o, "%s: null objective", who);
    ICZ_REQUIRE(o->kind == ICZ_SCST_REINFORCE || o->kind == ICZ_SCST_RISK, "%s: kind=%d (0 REINFORCE, 1 minimum risk)", who, o->kind);
    ICZ_REQUIRE(o->K >= (o->kind == ICZ_SCST_RISK ? 2 : 1) && o->K <= SCST_MAX_K, "%s: K=%d samples per image outside %d..%d", who, o->K,
                o->kind == ICZ_SCST_RISK ? 2 : 1, SCST_MAX_K);
    ICZ_REQUIRE(rows >= 1 && T >= 1 && rows % o->K == 0, "%s: %d rows of %d steps are not a positive multiple of K=%d", who, rows, T, o->K);
    ICZ_REQUIRE(std::isfinite(o->risk_alpha) && o->risk_alpha > 0.f, "%s: risk_alpha %g not finite and positive", who, (double)o->risk_alpha);
    ICZ_REQUIRE(std::isfinite(o->entropy_weight) && o->entropy_weight >= 0.f, "%s: entropy_weight %g not finite and >= 0", who,
                (double)o->entropy_weight);
    ICZ_REQUIRE(std::isfinite(o->n_img_global) && o->n_img_global >= 0.f, "%s: n_img_global %g not finite and >= 0", who,
                (double)o->n_img_global);
    ICZ_REQUIRE(o->kind != ICZ_SCST_REINFORCE || o->reward, "%s: the REINFORCE term needs reward [rows, T]", who);
    ICZ_REQUIRE(o->kind != ICZ_SCST_RISK || o->scores, "%s: the risk term needs scores [rows]", who);
    if (out) *out = ScstObjective{o->kind, o->K, o->risk_alpha, o->entropy_weight, o->n_img_global, o->reward, o->scores};
    return ICZ_OK;
}

void ScstObjective::key(std::vector<uintptr_t>& k) const {
    uint32_t a, b, n;
    memcpy(&a, &risk_alpha, 4); memcpy(&b, &entropy_weight, 4); memcpy(&n, &n_img_global, 4);
    k.insert(k.end(), {(uintptr_t)0x5C57, (uintptr_t)kind, (uintptr_t)K, (uintptr_t)a, (uintptr_t)b, (uintptr_t)n, (uintptr_t)reward, (uintptr_t)scores});
}

int launch_scst_objective(const ScstObjective& o, const float* logp, const int64_t* seq, int B, int T, const float* msum_dev,
                          const ScstScratch& w, float* coef, float* out3, float* ent_out, float* msum_out, float* logits, int V, int ldl,
                          const int32_t* draw, const float* lse, int rows, int row0, hipStream_t st) {
    const bool ent = o.entropy_weight > 0.f;
    if (o.kind == ICZ_SCST_REINFORCE && !ent) {      // today's launches
        ICZ_TRY(launch_reinforce(logp, seq, o.reward, B, T, msum_dev, coef, out3, msum_out, logits, V, ldl, draw, lse, rows, row0, st));
        hipLaunchKernelGGL(scst_reinforce_only_kernel, dim3(1), dim3(1), 0, st, out3);
        if (ent_out) ICZ_CHECK_HIP(hipMemsetAsync(ent_out, 0, sizeof(float) * B * T, st));
        ICZ_CHECK_HIP(hipGetLastError());
        return ICZ_OK;
    }
    ICZ_REQUIRE(!ent || (ldl % 4 == 0 && ((uintptr_t)logits & 15) == 0), "scst objective: the entropy kernel moves 16 bytes at a time: ldl=%d, logits %p",
                ldl, (void*)logits);
    float* const msum_loc = w.scal;
    float* const obj = out3 + 1;
    if (o.kind == ICZ_SCST_REINFORCE) {
        hipLaunchKernelGGL(reinforce_loss_kernel, dim3(1), dim3(256), 0, st, logp, seq, o.reward, B, T, msum_dev, coef, obj, msum_loc);
    } else {
        const int n_img = B / o.K;
        const double inv_n = 1.0 / (o.n_img_global > 0.f ? (double)o.n_img_global : (double)n_img);
        hipLaunchKernelGGL(scst_risk_kernel, dim3(n_img), dim3(64), 0, st, logp, seq, o.scores, o.K, T, (double)o.risk_alpha, inv_n, coef, w.L_img,
                           w.m_img);
        hipLaunchKernelGGL(scst_risk_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)w.L_img, (const int*)w.m_img, n_img, inv_n, obj, msum_loc);
    }
    const int slot_rows = T * (rows ? rows : B);
    if (ent)
        hipLaunchKernelGGL(scst_entropy_dlogits_kernel, dim3(slot_rows), dim3(256), 0, st, logits, V, ldl, draw, lse, (const float*)coef, seq, B, T,
                           rows, row0, o.entropy_weight, msum_dev, (const float*)msum_loc, w.ent_rows);
    else
        hipLaunchKernelGGL(reinforce_dlogits_kernel, dim3(cdiv(ldl, 256), slot_rows), dim3(256), 0, st, logits, V, ldl, draw, lse,
                           (const float*)coef, B, T, rows, row0);
    hipLaunchKernelGGL(scst_finish_kernel, dim3(1), dim3(256), 0, st, ent ? (const float*)w.ent_rows : (const float*)nullptr, B, T, rows, row0,
                       o.entropy_weight, msum_dev, (const float*)msum_loc, (const float*)obj, out3, ent_out, msum_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int CaptionHead::check_objective(const char* who, const icz_scst_objective* obj) const {
    ICZ_TRY(scst_objective_args(who, obj, cur_B, cur_T, nullptr));
    ICZ_REQUIRE(obj->kind != ICZ_SCST_RISK || obj->K == cur_K, "%s: the risk term over K=%d samples per image, the stored rollout has %d", who,
                obj->K, cur_K);
    return ICZ_OK;
}

int CaptionHead::scst_objective(const ScstObjective& o, float* logits, int V, int ldl, float* loss_out3, float* ent_out, float* msum_out,
                                hipStream_t st, int rows, int row0) {
    const ScstScratch w = {loss_rows, obj_img, obj_mimg, obj_scal};      // (loss_rows: the XE head's per-row losses, free behind a rollout)
    return launch_scst_objective(o, cur_logp, cur_seq, cur_B, cur_T, d_msum, w, coef, loss_out3, ent_out, msum_out, logits, V, ldl, draw, lse,
                                 rows, row0, st);
}

int CaptionHead::rollout_head(const RolloutHead& hd, float* logits, int V, int ldl, hipStream_t st, int rows, int row0) {
    if (!hd.obj) return reinforce(hd.reward, logits, V, ldl, hd.loss_out, hd.msum_out, st, rows, row0);
    return scst_objective(*hd.obj, logits, V, ldl, hd.loss_out, hd.ent_out, hd.msum_out, st, rows, row0);
}

}  // namespace icz

using namespace icz;
extern "C" {

int icz_scst_objective_check(const icz_scst_objective* obj, int32_t rows, int32_t T) {
    return scst_objective_args("icz_scst_objective_check", obj, rows, T, nullptr);
}

int icz_test_scst_objective(const icz_scst_objective* obj, const float* logp, const int64_t* seq, int32_t B, int32_t T,
                            const float* mask_sum_global, float* coef, float* loss_out3, float* ent_out, float* mask_sum_out, float* logits,
                            int32_t V, int32_t ldl, const int32_t* draw, const float* lse, int32_t Bs, int32_t row0, void* stream) {
    const char* who = "icz_test_scst_objective";
    ScstObjective o;
    ICZ_TRY(scst_objective_args(who, obj, B, T, &o));
    ICZ_REQUIRE(logp && seq && coef && loss_out3 && logits && draw && lse, "%s: null argument", who);
    ICZ_REQUIRE(V >= 1 && ldl >= V, "%s: V=%d, ldl=%d", who, V, ldl);
    ICZ_REQUIRE((long)B * T <= (1 << 20), "%s: B=%d, T=%d", who, B, T);
    ICZ_REQUIRE((Bs == 0 && row0 == 0) || (row0 >= 0 && Bs == row0 + B), "%s: Bs=%d rows per step are not row0=%d + B=%d", who, Bs, row0, B);
    ICZ_REQUIRE((long)T * (Bs ? Bs : B) <= 65535, "%s: %ld logits rows exceed the grid", who, (long)T * (Bs ? Bs : B));
    ICZ_REQUIRE(o.entropy_weight == 0.f || (ldl % 4 == 0 && ((uintptr_t)logits & 15) == 0), "%s: the entropy kernel needs ldl %% 4 == 0 and 16-byte aligned logits",
                who);
    hipStream_t st = (hipStream_t)stream;
    // scratch: ent_rows [T Bs'] | scal [4] floats, L_img [n_img] doubles, m_img [n_img] ints
    const size_t slot_rows = (size_t)T * (Bs ? Bs : B), n_img = (size_t)B / o.K;
    const size_t off_L = (sizeof(float) * (slot_rows + 4) + 7) & ~(size_t)7, off_m = off_L + sizeof(double) * n_img;
    char* part = nullptr;
    ICZ_CHECK_HIP(hipMallocAsync((void**)&part, off_m + sizeof(int) * n_img, st));
    const ScstScratch w = {(float*)part, (double*)(part + off_L), (int*)(part + off_m), (float*)part + slot_rows};
    const int status = launch_scst_objective(o, logp, seq, B, T, mask_sum_global, w, coef, loss_out3, ent_out, mask_sum_out, logits, V, ldl, draw,
                                             lse, Bs, row0, st);
    ICZ_CHECK_HIP(hipFreeAsync(part, st));
    return status;
}

}  // extern "C"
