// AoADetection captioner, training paths: sampled rollout (sampler_rl, AoA_Model.py:716-734 -> AoA_Decoder.sample_rl :347-401),
// teacher-forced forward (:676-696 -> AoA_Decoder.forward :231-287) and BPTT for the decoder parameters.
//
// Backward layout (same scheme as the BUTD decoder): the reverse-time loop only runs what is truly sequential -- per step
// three NN dgrad GEMMs (GLU input, attention query, LSTM recurrence) and four pointwise kernels; every weight gradient is
// one TN GEMM over all (t, b) rows after the loop.  The gradients of the hoisted linear_K / linear_V outputs are
// accumulated per image over time by the one workgroup that owns the (image, head) slice (no atomics, fixed order).
#include "aoa_impl.h"
#include "aoa_test_support.h"
#include "butd_kernels.h"
#include "ens_sample.h"
#include "lstm_kernels.h"
#include "support_kernels.h"
#include "token_kernels.h"

namespace icz {
namespace {

// GLU backward + the two dropouts that feed ctx_t:
//   dctx = drop_out'(dCd) + drop_ctx'(du_{t+1})      (ctx_t is the predict input at t and the LSTM input at t+1)
//   z = [a | b], ctx = a * sigmoid(b):  da = dctx * s,  db = dctx * a * s * (1 - s)
__global__ __launch_bounds__(256) void aoa_glu_bwd_kernel(const float* __restrict__ dCd, DropP d_out, const float* __restrict__ du_next, int ns,
                                                          int rows_next, DropP d_ctx_next, const float* __restrict__ z, float* __restrict__ dz,
                                                          int rows, int Hd, const int* __restrict__ live = nullptr,
                                                          const int* __restrict__ carry_live = nullptr) {
    if (step_dead(live)) return;               // the step never ran (icz_common.h); its dz rows were zeroed in front of the loop
    if (step_dead(carry_live)) du_next = nullptr;      // the step behind this one never ran: no carry
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * Hd) return;
    const size_t row = i / Hd;
    const int c = (int)(i % Hd);
    float d = d_out.apply(dCd[i], i);
    if (du_next && row < (size_t)rows_next) {
        const float g = sum_slabs1(du_next, ns, (size_t)rows_next * 2 * Hd, row * 2 * Hd + c);
        d += d_ctx_next.apply(g, i);
    }
    const float a = z[row * 2 * Hd + c], b = z[row * 2 * Hd + Hd + c];
    const float s = sigmoidf_(b);
    dz[row * 2 * Hd + c] = d * s;
    dz[row * 2 * Hd + Hd + c] = d * a * s * (1.f - s);
}

// Decoder attention backward, one workgroup per (row, head); row b attends image b, or image img_of_row[b] behind the multi-sample
// rollout (Aoa::sample_n: K rows per image, which share the image's K / V tiles and region count).
//   dPd_r = dx_h . V_h[r];  dP = keep/(1-p) * dPd;  dS = P (dP - sum P dP);  dQ_h = sum_r dS_r K_h[r] / sqrt(d)
// dK_h[r] = sum_t dS_t[r] Q_t,h / sqrt(d) and dV_h[r] = sum_t Pd_t[r] dx_t,h are sums over time: the steps only record dS_t
// (already scaled by 1/sqrt(d)) and dx_t, and aoa_dkv_kernel forms both sums once after the loop -- accumulating them
// step by step would read-modify-write the two [B, R, Hd] tensors (38 MB) in every step.
// dx = columns [0, Hd) of the GLU-input gradient slabs [ns][rows][2Hd].
__global__ __launch_bounds__(256) void aoa_dec_attn_bwd_kernel(const float* __restrict__ dxq, int ns, int rows, const float* __restrict__ Pm,
                                                               const float* __restrict__ Pdm, const float* __restrict__ Qp,
                                                               const float* __restrict__ Kd, const float* __restrict__ Vd,
                                                               float* __restrict__ dQp, float* __restrict__ dS_out, float* __restrict__ dx_out, int R, int Hd,
                                                               int NH, RegionRows rr, float keep_scale, const int* __restrict__ live = nullptr,
                                                               const int32_t* __restrict__ img_of_row = nullptr) {
    extern __shared__ __attribute__((aligned(16))) float sm_db[];    // K tile, V tile [R][d+1], q [d], dx [d], dS [128], red [4]
    if (step_dead(live)) return;
    const int row = blockIdx.x, hd = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = Hd / NH, ld = d + 1;
    float* sk = sm_db;
    float* sv = sk + R * ld;
    float* sq = sv + R * ld;
    float* sdx = sq + d;
    float* sds = sdx + d;
    float* red = sds + 128;
    const int img = img_of_row ? img_of_row[row] : row;
    const int len = rr.count(img);
    const size_t base = rr.first(img) * Hd + (size_t)hd * d;
    aoa_stage_kv<256>(Kd + base, Vd + base, sk, sv, len, d, Hd, tid);
    const size_t MN = (size_t)rows * 2 * Hd;
    for (int j = tid; j < d; j += 256) {
        sq[j] = Qp[(size_t)row * Hd + (size_t)hd * d + j];
        sdx[j] = sum_slabs1(dxq, ns, MN, (size_t)row * 2 * Hd + (size_t)hd * d + j);
    }
    __syncthreads();
    const size_t pidx = ((size_t)row * NH + hd) * R + tid;
    float p = 0.f, dP = 0.f;
    if (tid < len) {
        p = Pm[pidx];
        float acc = 0.f;
        for (int j = 0; j < d; ++j) acc += sdx[j] * sv[tid * ld + j];
        dP = Pdm[pidx] != 0.f ? acc * keep_scale : 0.f;
    }
    const float wdot = wave_sum(p * dP);
    if (lane == 0) red[wave] = wdot;
    __syncthreads();
    const float dot = red[0] + red[1];
    if (tid < 128) {
        const float dS = p * (dP - dot) / sqrtf((float)d);
        sds[tid] = dS;
        if (tid < R) dS_out[pidx] = dS;
    }
    __syncthreads();
    for (int j = tid; j < d; j += 256) {
        float acc = 0.f;
        for (int r = 0; r < len; ++r) acc += sds[r] * sk[r * ld + j];
        dQp[(size_t)row * Hd + (size_t)hd * d + j] = acc;
        dx_out[(size_t)row * Hd + (size_t)hd * d + j] = sdx[j];
    }
}

// dKd[img, r, head cols] = sum_t dS_t[row, head, r] Qp_t[row, head cols];  dVd = sum_t Pd_t[r] dx_t   (grid (n_img, NH), 256 threads).
// B = decoder rows per step, G = rows per image: the image's rows are img * G + k (G = 1: row b is image b; G > 1: the multi-sample
// rollout, Aoa::sample_n, whose K rows of an image add into the image's d K / d V).  The (k, t) pairs are walked k-major, t-minor and go
// through LDS in chunks of TC pairs (all of them at the usual 20 steps x 36 regions of one row): one workgroup owns the (image, head)
// slice, so the sum has a fixed order and needs no atomics.
__global__ __launch_bounds__(256) void aoa_dkv_kernel(const float* __restrict__ dS_all, const float* __restrict__ Pd_all,
                                                      const float* __restrict__ Qp_all, const float* __restrict__ dx_all,
                                                      float* __restrict__ dKd, float* __restrict__ dVd, int B, int T, int TC, int R, int Hd, int NH,
                                                      RegionRows rr, int G) {
    extern __shared__ __attribute__((aligned(16))) float sm_kv[];       // dS [TC][R], Pd [TC][R], Qp [TC][d], dx [TC][d]
    const int img = blockIdx.x, hd = blockIdx.y, tid = threadIdx.x;
    const int d = Hd / NH;
    float* sds = sm_kv;
    float* spd = sds + TC * R;
    float* sq = spd + TC * R;
    float* sdx = sq + TC * d;
    const size_t base = rr.first(img) * Hd + (size_t)hd * d;
    const int len = rr.count(img);
    const int S = G * T;                // (k, t) pairs of the image: pair s = k * T + t is row img * G + k at step t
    for (int s0 = 0; s0 < S; s0 += TC) {
        const int nt = min(TC, S - s0);
        for (int i = tid; i < nt * R; i += 256) {
            const int sp = s0 + i / R, r = i % R, k = sp / T, t = sp - k * T;
            const size_t g = (((size_t)t * B + (size_t)img * G + k) * NH + hd) * R + r;
            sds[i] = dS_all[g];
            spd[i] = Pd_all[g];
        }
        for (int i = tid; i < nt * d; i += 256) {
            const int sp = s0 + i / d, j = i % d, k = sp / T, t = sp - k * T;
            const size_t g = ((size_t)t * B + (size_t)img * G + k) * Hd + (size_t)hd * d + j;
            sq[i] = Qp_all[g];
            sdx[i] = dx_all[g];
        }
        __syncthreads();
        for (int i = tid; i < len * d; i += 256) {
            const int r = i / d, j = i % d;
            const size_t o = base + (size_t)r * Hd + j;
            float dk = s0 ? dKd[o] : 0.f, dv = s0 ? dVd[o] : 0.f;
            for (int t = 0; t < nt; ++t) {
                dk += sds[t * R + r] * sq[t * d + j];
                dv += spd[t * R + r] * sdx[t * d + j];
            }
            dKd[o] = dk;
            dVd[o] = dv;
        }
        __syncthreads();
    }
}

// Custom LayerNorm backward (AoA_Model.py:14-25: unbiased std, eps outside the sqrt), one workgroup per row.
//   dq = dq_a (slabs [ns_a][rows][Hd], linear_Q dgrad) + dq_b (slabs [ns_b][rows][2Hd] at column offset Hd, GLU-input dgrad)
//   y = g (x - mean) inv + b, inv = 1/(std + eps):  dy = dq g;  dstd = -inv^2 sum(dy xh);
//   dxh = dy inv + dstd xh / (std (n-1));  dx = dxh - mean(dxh)
__global__ __launch_bounds__(256) void aoa_ln_bwd_kernel(const float* __restrict__ dq_a, int ns_a, const float* __restrict__ dq_b, int ns_b, int rows,
                                                         const float* __restrict__ x, const float* __restrict__ stats,
                                                         const float* __restrict__ gain, float* __restrict__ dq_tot, float* __restrict__ dx, int n,
                                                         const int* __restrict__ live = nullptr) {
    // one workgroup per row; a thread keeps its columns (4 adjacent ones per 1024) in registers between the two passes
    __shared__ float sm_red[4];
    if (step_dead(live)) return;
    constexpr int NV = 4;                         // n <= 4096, n % 4 == 0 (checked by the host)
    const int row = blockIdx.x, tid = threadIdx.x;
    const float mean = stats[2 * row], inv = stats[2 * row + 1];
    const float stdv = 1.0f / inv - 1e-6f;
    const float* xr = x + (size_t)row * n;
    f32x4 dy[NV], xc[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int c = 4 * tid + 1024 * u;
        dy[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        xc[u] = dy[u];
        if (c < n) {
            const f32x4 dq = sum_slabs4(dq_a, ns_a, (size_t)rows * n, (size_t)row * n + c) +
                             sum_slabs4(dq_b, ns_b, (size_t)rows * 2 * n, (size_t)row * 2 * n + n + c);
            *reinterpret_cast<f32x4*>(dq_tot + (size_t)row * n + c) = dq;
            const f32x4 g = *reinterpret_cast<const f32x4*>(gain + c);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dy[u][j] = dq[j] * g[j];
                xc[u][j] = xv[j] - mean;
                s1 += dy[u][j];
                s2 += dy[u][j] * xc[u][j];
            }
        }
    }
    s1 = block_sum_256(s1, sm_red);
    s2 = block_sum_256(s2, sm_red);
    const float dstd = -inv * inv * s2;
    const float kx = dstd / (stdv * (float)(n - 1));
    const float mdx = inv * s1 / (float)n;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int c = 4 * tid + 1024 * u;
        if (c < n) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = dy[u][j] * inv + kx * xc[u][j] - mdx;
            *reinterpret_cast<f32x4*>(dx + (size_t)row * n + c) = o;
        }
    }
}

// prod[row, c] = dq[row, c] * (x[row, c] - mean) * inv     (column sums of it = d gain)
__global__ __launch_bounds__(256) void aoa_ln_prod_kernel(const float* __restrict__ dq, const float* __restrict__ x, const float* __restrict__ stats,
                                                          float* __restrict__ prod, size_t rows, int n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * n) return;
    const size_t row = i / n;
    prod[i] = dq[i] * (x[i] - stats[2 * row]) * stats[2 * row + 1];
}

}  // namespace

// Training buffers sized by what the batches ask for (the reference never truncates captions, Datasets.py:47-51: the step
// count of an XE batch is only known when it arrives); growing re-allocates them all.
// Bq = decoder rows, Iq = images (< Bq behind the multi-sample rollout, whose per-image tensors stay sized per image; 0 = one row per image)
int Aoa::ensure_train(int Bq, int Tq, int Iq) {
    if (Iq <= 0) Iq = Bq;
    if (Bq <= tcap_B && Tq <= tcap_T && Iq <= tcap_I) return ICZ_OK;
    ICZ_REQUIRE(dims.Hd <= 4096, "aoa: training paths keep a LayerNorm row in registers (hidden size %d > 4096)", dims.Hd);
    ICZ_REQUIRE(Tq <= XE_MAX_T, "aoa: %d steps exceed the limit of %d", Tq, XE_MAX_T);
    if (tcap_B > Bq) Bq = tcap_B;
    if (tcap_T > Tq) Tq = tcap_T;
    if (tcap_I > Iq) Iq = tcap_I;
    if (dims.max_len > Tq) Tq = dims.max_len;
    if (!mem.training.empty()) {
        ICZ_TRY(mem.release_training(&gc));
        tcap_B = tcap_T = tcap_I = 0;
        drop_loss_buffers();
        drop_refiner_buffers();
    }
    DeviceBuffers::TrainingScope scope(mem);
    const size_t B = Bq, T = Tq, I = Iq, Hd = dims.Hd, E = dims.E, R = dims.R, NH = dims.NH;
    ICZ_TRY(aoa_dec_attn_bwd_optin(aoa_dec_attn_bwd_lds((int)R, (int)(Hd / NH))));
    const size_t TB = T * B;
    ICZ_TRY(alloc((void**)&tok, sizeof(int64_t) * (TB + B)));
    float** st1[] = {&th, &tm, &tctx};
    for (float** p : st1) ICZ_TRY(alloc((void**)p, sizeof(float) * (TB + B) * Hd));
    ICZ_TRY(alloc((void**)&temb, sizeof(float) * TB * E));
    float** sth[] = {&tu, &tqn, &tQp, &txatt, &tcd, &dCd, &dQp, &dQn, &prod, &tdX};
    for (float** p : sth) ICZ_TRY(alloc((void**)p, sizeof(float) * TB * Hd));
    ICZ_TRY(alloc((void**)&tg, sizeof(float) * TB * 4 * Hd));
    ICZ_TRY(alloc((void**)&dG, sizeof(float) * TB * 4 * Hd));
    ICZ_TRY(alloc((void**)&tz, sizeof(float) * TB * 2 * Hd));
    ICZ_TRY(alloc((void**)&dZ, sizeof(float) * TB * 2 * Hd));
    ICZ_TRY(alloc((void**)&tstats, sizeof(float) * TB * 2));
    ICZ_TRY(alloc((void**)&tP, sizeof(float) * TB * NH * R));
    ICZ_TRY(alloc((void**)&tPd, sizeof(float) * TB * NH * R));
    ICZ_TRY(alloc((void**)&tdS, sizeof(float) * TB * NH * R));
    ICZ_TRY(alloc((void**)&tlogit, sizeof(float) * TB * Vp));
    ICZ_TRY(alloc((void**)&dEmb, sizeof(float) * TB * E));
    ICZ_TRY(alloc((void**)&dKd, sizeof(float) * I * R * Hd));
    ICZ_TRY(alloc((void**)&dVd, sizeof(float) * I * R * Hd));
    ICZ_TRY(alloc((void**)&dHln, sizeof(float) * B * Hd));
    ICZ_TRY(alloc((void**)&dcb[0], sizeof(float) * B * Hd));
    ICZ_TRY(alloc((void**)&dcb[1], sizeof(float) * B * Hd));
    xfloats = (size_t)TARGET_WGS * 4096 * 2 + TB * (Hd > E ? Hd : E) + B * 4 * Hd;
    ICZ_TRY(alloc((void**)&X, sizeof(float) * xfloats));
    ICZ_TRY(alloc((void**)&X2, sizeof(float) * xfloats));
    ICZ_TRY(alloc((void**)&dWp, sizeof(float) * (size_t)Vp * Hd));
    ICZ_TRY(alloc_loss_buffers(mem, TB, B, T));
    if (train_refiner) ICZ_TRY(alloc_refiner_train(I, TB));
    ICZ_TRY(mem.synced());
    tcap_B = Bq; tcap_T = Tq; tcap_I = Iq;
    return ICZ_OK;
}

// step t of a training-mode pass over cur_B rows: inputs / outputs are slots of the saved [T, B, ...] tensors
AoaStepIO Aoa::train_io(int rows, int t, bool train) {
    const size_t B = cur_B, Hd = dims.Hd, E = dims.E, NH = dims.NH, R = cur_R;
    const size_t s0 = (size_t)t * B, s1 = s0 + B;
    AoaStepIO s = {};
    s.rows = rows; s.img_of_row = cur_K > 1 ? imgk : nullptr; s.it = tok + s0; s.emb_ready = false;
    s.h_in = th + s0 * Hd; s.m_in = tm + s0 * Hd; s.ctx_in = tctx + s0 * Hd;
    s.h_out = th + s1 * Hd; s.m_out = tm + s1 * Hd; s.ctx_out = tctx + s1 * Hd;
    s.emb = temb + s0 * E; s.u = tu + s0 * Hd; s.gates_out = tg + s0 * 4 * Hd; s.ln_stats = tstats + s0 * 2;
    s.qn = tqn + s0 * Hd; s.Qp = tQp + s0 * Hd; s.P_out = tP + s0 * NH * R; s.Pd_out = tPd + s0 * NH * R;
    s.xatt = txatt + s0 * Hd; s.z_out = tz + s0 * 2 * Hd; s.ctxdrop = tcd + s0 * Hd; s.logits = tlogit + s0 * Vp;
    s.d_emb = dropbits(train, rng.emb_mask, s0 * E, RNG_EMB, t);
    s.d_ctx = dropp(train, rng.ctx_mask, s0 * Hd, AOA_RNG_CTX, t, 0.5f);
    s.d_att = dropp(train, rng.att_mask, s0 * NH * R, AOA_RNG_ATT, t, 0.1f);
    s.d_out = dropp(train, rng.out_mask, s0 * Hd, AOA_RNG_OUT, t, 0.5f);
    return s;
}

static bool aoa_explicit_rng(const icz_aoa_rng& r) {
    return r.uniforms || r.proj_mask || r.ref_att_mask || r.ref_aoa_mask || r.ref_sc_mask || r.emb_mask || r.ctx_mask || r.att_mask || r.out_mask;
}

// everything of a sampled rollout that is host state or must not sit inside a captured graph: buffers, the Philox seed in device
// memory, what the backward pass will read back
// B = decoder rows; K > 1: the multi-sample rollout's B / K images with K rows each
int Aoa::sample_prelude(const float* feats, int B, int T, const icz_aoa_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st, int K) {
    ICZ_REQUIRE(feats && seq_out && logp_out && r && B > 0 && B <= dims.max_rows && T > 0, "aoa sample: bad arguments");
    ICZ_REQUIRE(fresh, "aoa: call icz_aoa_refresh_weights after binding/updating parameters");
    ICZ_TRY(ensure_train(B, T, B / K));
    rng = *r;
    begin_rollout(B, T, seq_out, logp_out, rng.seed, st);
    cur_K = K;
    xs_valid = false;                  // set by the training-mode refiner pass of this rollout (option "train_refiner")
    return ICZ_OK;
}

int Aoa::sample(const float* feats, int B, int T, const icz_aoa_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_TRY(sample_prelude(feats, B, T, r, seq_out, logp_out, st));
    return sample_impl(feats, B, T, seq_out, logp_out, st);
}

// Multi-sample rollout (beyond the reference: K sampled captions per image, the "new self-critical" variant): the training-mode refiner
// pass, its region mean and the hoisted linear_K / linear_V run once over the B images, the sampled chain over B K decoder rows,
// row = img * K + k, whose kernels find their image through imgk (train_io).  Dropout keep-bits and draws are indexed by the row in the
// B K space -- row img * K + k gets what row img * K + k of sample(feats.repeat_interleave(K, 0)) gets; the refiner's by the image.
int Aoa::sample_n(const float* feats, int B, int K, int T, const icz_aoa_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_REQUIRE(feats && seq_out && logp_out && r, "aoa sample_n: null argument");
    ICZ_REQUIRE(K >= 2 && K <= SAMPLE_N_MAX_K, "aoa sample_n: K=%d samples per image outside 2..%d", K, SAMPLE_N_MAX_K);
    ICZ_REQUIRE(B > 0 && T > 0, "aoa sample_n: bad B/T");
    ICZ_REQUIRE((int64_t)B * K <= dims.max_rows, "aoa sample_n: %d images x %d samples exceed the row capacity %d", B, K, dims.max_rows);
    ICZ_REQUIRE(!lens || lens_n == B, "aoa: region counts were set for %d images, the batch has %d (icz_aoa_set_regions)", lens_n, B);
    ICZ_REQUIRE(fresh, "aoa: call icz_aoa_refresh_weights after binding/updating parameters");
    const int rows = B * K;
    if (!imgk) {
        ICZ_TRY(alloc((void**)&imgk, sizeof(int32_t) * (size_t)dims.max_rows));
        ICZ_TRY(mem.synced());
    }
    ICZ_TRY(sample_prelude(feats, rows, T, r, seq_out, logp_out, st, K));
    // host state, outside any captured graph (a replay runs no host code): the bank's own tensors, what the refiner's backward will read
    point_bank_at_own(1);
    use_bank(1);
    if (train_refiner && !lens) { ref_feats = feats; xs_valid = true; }
    if (!use_graphs || lens || aoa_explicit_rng(rng)) return sample_n_impl(feats, B, K, T, seq_out, logp_out, st);
    const std::vector<uintptr_t> key = {3, (uintptr_t)feats, (uintptr_t)B, (uintptr_t)K, (uintptr_t)T, (uintptr_t)cur_R, (uintptr_t)seq_out,
                                        (uintptr_t)logp_out, (uintptr_t)train_refiner, (uintptr_t)xs[0]};
    return gc.run(key, st, [&](hipStream_t s) { return sample_n_impl(feats, B, K, T, seq_out, logp_out, s); });
}

int Aoa::sample_n_impl(const float* feats, int B, int K, int T, int64_t* seq_out, float* logp_out, hipStream_t st) {
    hipLaunchKernelGGL(row_image_kernel, dim3(cdiv(B * K, 256)), dim3(256), 0, st, imgk, B * K, K);
    return sample_impl(feats, B * K, T, seq_out, logp_out, st, nullptr, false, B);
}

// B = decoder rows of n_img images (0 = one row per image)
int Aoa::sample_impl(const float* feats, int B, int T, int64_t* seq_out, float* logp_out, hipStream_t st, const float* proj, bool refined_ready,
                     int n_img) {
    use_bank(1);
    if (!refined_ready) ICZ_TRY(refine(feats, n_img > 0 ? n_img : B, true, st, proj));
    const size_t sH = (size_t)B * dims.Hd;
    ICZ_CHECK_HIP(hipMemsetAsync(th, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tm, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tctx, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(unf, 1, B, st));
    ICZ_CHECK_HIP(hipMemsetAsync(nunf, 0, sizeof(int) * T, st));
    hipLaunchKernelGGL(fill_i64_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, tok, (int64_t)1, B);
    for (int t = 0; t < T; ++t) {
        const size_t slot = (size_t)t * B;
        AoaStepIO io = train_io(B, t, true);
        io.emb_ready = t > 0;           // written by the previous step's sample_select_kernel
        io.u_ready = t > 0;             // written by the previous step's GLU kernel
        if (t + 1 < T) { const AoaStepIO nx = train_io(B, t + 1, true); io.u_next = nx.u; io.d_ctx_next = nx.d_ctx; }
        int pns = 1;
        io.pred_nsplit = &pns;
        // step t > 0 is dead when step t - 1 left no row unfinished (the reference breaks out of its loop there, AoA_Model.py:400)
        if (t > 0 && early_out) io.live = nunf + (t - 1);
        ICZ_TRY(step(io, st));
        SampleSelArgs a = {};
        a.live_rows = live_rows;
        a.logits = tlogit + slot * Vp; a.V = dims.V; a.ldl = Vp;
        if (pns > 1) {          // the predict GEMM left split-K slabs in the bank's workspace
            a.logits = ws; a.ns = pns; a.slab_stride = (size_t)B * Vp; a.bias = P.predict_b; a.logits_store = tlogit + slot * Vp;
        }
        a.uniforms = rng.uniforms ? rng.uniforms + slot : nullptr;
        a.seed_p = d_seed; a.t = t; a.T = T;
        a.unfinished = unf; a.n_unfinished = nunf; a.seq_out = seq_out; a.logp_out = logp_out;
        a.it_next = tok + slot + B; a.draw_out = draw + slot; a.lse_out = lse + slot;
        if (t + 1 < T) {                // the next step's input embedding (its slot, its dropout stream), fused
            a.emb_table = P.embed_weight; a.emb_next = temb + (slot + B) * dims.E; a.E = dims.E;
            a.emb_drop = dropbits(true, rng.emb_mask, (slot + B) * dims.E, RNG_EMB, t + 1);
        }
        ICZ_TRY(launch_sample_select(st, B, a));
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// Greedy baseline (evaluation mode, bank 0, side stream) and sampled rollout (training mode, bank 1) of one SCST step
// (Engine.py:256-261) enqueued as two concurrent chains; identical to greedy() followed by sample().  Round 5: the feature projection
// (2048 -> 1024 over B x 36 rows, 9.7 GFLOP at B = 64) is the same product in both passes up to its ReLU / dropout epilogue
// (AoA_Model.py:661-665, 712-713): computed once in front of the fork; and with option "graphs" the pair is ONE captured hipGraph
// (fixed region counts, Philox randomness), replayed like the BUTD pair.
int Aoa::rollouts(const float* feats, int B, int T, const icz_aoa_rng* r, int64_t* ids_out, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_REQUIRE(ids_out, "aoa rollouts: null argument");
    ICZ_TRY(side.ensure());
    ICZ_TRY(sample_prelude(feats, B, T, r, seq_out, logp_out, st));
    if (!lens && !proj_shared) {
        ICZ_TRY(alloc((void**)&proj_shared, sizeof(float) * (size_t)dims.max_rows * dims.R * dims.Hd));
        ICZ_TRY(mem.synced());
    }
    if (!lens && pair_refine && !dual.xa) {      // the pair buffers: twice the rows of a bank's
        const size_t RR2 = (size_t)2 * dims.max_rows * dims.R, Hd = dims.Hd;
        float** ref[] = {&dual.xa, &dual.xb, &dual.ln, &dual.o, &dual.refined, &dual.Kd, &dual.Vd};
        for (float** p : ref) ICZ_TRY(alloc((void**)p, sizeof(float) * RR2 * Hd));
        ICZ_TRY(alloc((void**)&dual.qkv, sizeof(float) * RR2 * 3 * Hd));
        ICZ_TRY(alloc((void**)&dual.z, sizeof(float) * RR2 * 2 * Hd));
        ICZ_TRY(alloc((void**)&dual.meanf, sizeof(float) * (size_t)2 * dims.max_rows * Hd));
        ICZ_TRY(mem.synced());
    }
    // (host state, outside any captured graph: a replayed rollout pair leaves the banks where this call's batch size puts them)
    if (!lens && pair_refine) point_banks_at_pair(B); else { point_bank_at_own(0); point_bank_at_own(1); }
    // (host state too: a replayed graph does not run the refiner's host code) fixed region counts project the caller's features
    if (train_refiner && !lens) { ref_feats = feats; xs_valid = true; }
    if (!use_graphs || lens || aoa_explicit_rng(rng)) return rollouts_impl(feats, B, T, ids_out, seq_out, logp_out, st);
    const std::vector<uintptr_t> key = {1, (uintptr_t)feats, (uintptr_t)B, (uintptr_t)T, (uintptr_t)cur_R, (uintptr_t)ids_out, (uintptr_t)seq_out,
                                        (uintptr_t)logp_out};
    return gc.run(key, st, [&](hipStream_t s) { return rollouts_impl(feats, B, T, ids_out, seq_out, logp_out, s); });
}

int Aoa::rollouts_impl(const float* feats, int B, int T, int64_t* ids_out, int64_t* seq_out, float* logp_out, hipStream_t st) {
    const float* proj = nullptr;
    if (!lens) {                        // (an 'adaptive' batch packs its rows per bank: each pass projects its own)
        ICZ_TRY(project(feats, B, proj_shared, st));
        proj = proj_shared;
    }
    const bool pair = proj && pair_refine && dual.xa;
    if (pair) ICZ_TRY(refine_pair(B, st, proj));          // both refiner passes in one, in front of the fork
    SideStream::Branch baseline(&side, 0);
    ICZ_TRY(baseline.fork(st));
    ICZ_TRY(baseline.start());
    ICZ_TRY(greedy(feats, B, T, ids_out, baseline.st(), proj, true, pair));
    ICZ_TRY(sample_impl(feats, B, T, seq_out, logp_out, st, proj, pair));
    return baseline.join();
}

int Aoa::backward(const LossHead& head, const icz_aoa_params* G, hipStream_t st) {
    ICZ_TRY(check_loss_head(head, G));
    if (train_refiner) ICZ_TRY(refiner_backward_check(*G));
    const bool eo = head.rollout_kind() && early_out;
    // the REINFORCE / objective head goes into the captured graph with its bptt(); every other head is queued here
    const bool in_graph = head.kind == LossHead::ROLLOUT;
    ICZ_TRY(begin_backward(head, in_graph, tlogit, dims.V, Vp, st));
    // the side stream of bptt, created here, outside any capture.  A plain stream: eager launches on a PRIORITISED stream beside other
    // streams' work can serialise on this runtime (EXPERIMENTS.md, round 4, section 8), and the AoA paths are eager
    ICZ_TRY(low.ensure());
    if (!in_graph) return bptt(*G, st, eo);
    const RolloutHead& hd = head.rollout;
    const icz_aoa_params Gc = *G;
    auto run = [&](hipStream_t s) -> int {
        ICZ_TRY(launch_loss_head(head, tlogit, dims.V, Vp, s));
        return bptt(Gc, s, eo);
    };
    // with a DP callback the hook must fire on every call: eager launches (a replayed graph would not call it)
    if (!use_graphs || lens || grad_cb || aoa_explicit_rng(rng)) return run(st);
    // the captured graph carries the objective in its key (ScstObjective::key) beside the output pointers
    std::vector<uintptr_t> key = {2, (uintptr_t)hd.reward, (uintptr_t)hd.loss_out, (uintptr_t)hd.msum_out, (uintptr_t)cur_B, (uintptr_t)cur_T, (uintptr_t)cur_R,
                                  (uintptr_t)cur_seq, (uintptr_t)cur_logp, (uintptr_t)cur_K,      // sample_n of B K rows against sample of B K rows: other launches
                                  (uintptr_t)bank[0].refined, (uintptr_t)bank[0].Kd, (uintptr_t)bank[1].refined, (uintptr_t)bank[1].Kd, (uintptr_t)bank[1].Vd, (uintptr_t)cur_bank,      // paired-refine banks (rollouts) or the handle's own (sample)
                                  (uintptr_t)train_refiner, (uintptr_t)xs[0], (uintptr_t)ref_feats};      // the refiner's backward pass behind bptt
    const float* const* gp = reinterpret_cast<const float* const*>(G);
    for (size_t i = 0; i < sizeof(icz_aoa_params) / sizeof(float*); ++i) key.push_back((uintptr_t)gp[i]);
    if (hd.obj) { hd.obj->key(key); key.push_back((uintptr_t)hd.ent_out); }
    return gc.run(key, st, run);
}

int Aoa::xe_forward(const float* feats, const int64_t* captions, int B, int L, const int32_t* lengths, const icz_aoa_rng* r, int train,
                    float* packed_out, hipStream_t st) {
    ICZ_REQUIRE(feats && captions && lengths && B > 0 && B <= dims.max_rows && L > 1, "aoa xe_forward: bad arguments");
    ICZ_REQUIRE(fresh, "aoa: call icz_aoa_refresh_weights after binding/updating parameters");
    ICZ_REQUIRE(!train || r, "aoa xe_forward: training mode needs an icz_aoa_rng");
    int T = 0;
    ICZ_TRY(xe_steps("aoa", lengths, B, L, &T));
    ICZ_TRY(ensure_train(B, T));
    cur_K = 1;
    use_bank(1);
    if (r) rng = *r; else rng = {};
    begin_xe(lengths, B, T, L, captions, train != 0, rng.seed, st);
    xs_valid = false;
    ICZ_TRY(refine(feats, B, cur_train, st));
    const size_t sH = (size_t)B * dims.Hd;
    ICZ_CHECK_HIP(hipMemsetAsync(th, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tm, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tctx, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tlogit, 0, sizeof(float) * (size_t)T * B * Vp, st));
    captions_to_tok(tok, st);
    // teacher forcing: one vocabulary projection over all (t, b) rows after the loop unless scheduled sampling needs the previous
    // step's logits (butd_train.hip: xe_forward); rows b >= rows_t[t] are zeroed by xe_loss_dlogits_kernel / the scatter kernel
    const bool batched_predict = ss_prob <= 0.f && T * B >= 128;
    for (int t = 0; t < T; ++t) {
        if (t >= 2 && ss_prob > 0.f)          // scheduled sampling (AoA_Model.py:258-270): this step's tokens, mixed with draws from the previous logits
            ICZ_TRY(ss_select_launch(st, rows_t[t], tlogit + (size_t)(t - 1) * B * Vp, (int)Vp, dims.V, t, B, ss_prob, ss_gate, ss_draw, d_seed,
                                     tok + (size_t)t * B));
        AoaStepIO io = train_io(rows_t[t], t, cur_train);
        io.u_ready = t > 0;             // the next step's rows are a prefix of this step's: its u comes from this step's GLU kernel
        if (t + 1 < T) { const AoaStepIO nx = train_io(rows_t[t + 1], t + 1, cur_train); io.u_next = nx.u; io.d_ctx_next = nx.d_ctx; }
        io.skip_predict = batched_predict;
        ICZ_TRY(step(io, st));
    }
    if (batched_predict) {
        GemmArgs g = gemm_args({{tcd, w_pred, dims.Hd, dims.Hd, dims.Hd}}, T * B, dims.V, tlogit, Vp);
        g.bias = P.predict_b;
        ICZ_TRY(gemm_f32(GEMM_NT, g, st));
    }
    if (packed_out) ICZ_TRY(gather_packed(tlogit, dims.V, Vp, packed_out, st));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int Aoa::nn(const float* A, int lda, int M, int K, const float* Bm, int ldb, int N, float* slab, size_t cap, int* ns_out, const SplitPolicy& p,
            hipStream_t st, const int* live, const int* rows_live) {
    GemmArgs g = gemm_args({{A, Bm, lda, ldb, K}}, M, N, slab, N, live);
    g.rows_live = rows_live;
    return gemm_slabs(GEMM_NN, g, p, slab, cap, ns_out, st, "aoa");
}

// What the parts of one bptt() call share.  The two branches live as long as the call: whatever a part returns, a branch it has
// started is joined before bptt() returns (SideStream::Branch).
struct Aoa::BpttCall {
    const icz_aoa_params& G;
    hipStream_t st;
    int B, T, TB;
    // behind sample_n: K rows per image (row = img * K + k) -- the attention backward finds the image's K / V tiles through imgk, and
    // d K / d V are summed per image over its rows and the steps; everything over (t, row) simply sees B = n_img K rows
    int K, n_img;
    // backward of a sampled rollout: the steps behind the reference's break (AoA_Model.py:400) never ran -- their kernels return at
    // entry (the buffers the batched GEMMs read are zeroed in front of the loop) and the GEMMs over all (t, b) stop behind the last live step
    bool eo;
    const int* rl;
    SideStream::Branch predict;      // the predict layer's weight / bias gradients beside the reverse-time loop
    SideStream::Branch tail;         // the attention block's small products beside the batched weight gradients
};

int Aoa::bptt(const icz_aoa_params& G, hipStream_t st, bool eo) {
    use_bank(1);
    // Without a DP callback the two branches go to the side stream (a plain one, see backward()); with a callback they stay in line,
    // because the stages report their gradients complete in stream order.
    const bool side = !grad_cb;
    static const bool tail_side_on = [] { const char* e = getenv("ICZ_AOA_TAIL_SIDE"); return e ? atoi(e) != 0 : true; }();      // A/B switch (read once)
    BpttCall c = {G, st, cur_B, cur_T, cur_T * cur_B, cur_K, cur_B / cur_K, eo, eo ? live_rows : nullptr,
                  {side ? &low : nullptr, 0}, {side && tail_side_on ? &low : nullptr, 1}};
    ICZ_TRY(bptt_predict(c));
    if (grad_cb) grad_cb(grad_cb_user, 0);      // predict.* complete in stream order: reduced beside the reverse-time loop
    ICZ_TRY(bptt_loop(c));
    ICZ_TRY(c.predict.join());                  // the predict branch has long finished beside the loop
    // the attention block's tail depends on the loop only: forked at the loop's end, ISSUED last, joined behind it (as Butd::bptt's tail)
    ICZ_TRY(c.tail.fork(st));
    ICZ_TRY(bptt_embed_lstm_wgrad(c));
    if (grad_cb) grad_cb(grad_cb_user, 1);      // embed + lstm.*: reduced beside the attention block's weight gradients
    ICZ_TRY(bptt_aoa_wgrad(c));
    ICZ_TRY(c.tail.start());
    ICZ_TRY(bptt_attention_tail(c));
    ICZ_TRY(c.tail.join());
    ICZ_CHECK_HIP(hipGetLastError());
    // option "train_refiner": d refined -> the refiner and the feature projection, on the caller's stream behind every join above
    // (dKd / dVd from the tail, d gates from the loop)
    if (train_refiner) return refiner_backward(G, st);
    return ICZ_OK;
}

// ---- predict layer over all time steps: d(dropped ctx), weight-norm gradients
int Aoa::bptt_predict(BpttCall& c) {
    const int TB = c.TB, Hd = dims.Hd, V = dims.V;
    int ns = 1;
    ICZ_TRY(nn(tlogit, Vp, TB, Vp, w_pred, Hd, Hd, X, xfloats, &ns, split_backward(TARGET_WGS), c.st, nullptr, c.rl));
    ICZ_TRY(launch_slab_reduce(X, ns, TB, Hd, nullptr, dCd, c.st));      // (one slab: a copy)
    // The predict layer's weight / bias gradients need dlogits only: their branch is forked and ISSUED behind the d(ctx) product above
    // (the head of the critical chain, as in Butd::bptt) and joined behind the loop.
    ICZ_TRY(c.predict.fork(c.st));
    ICZ_TRY(c.predict.start());
    hipStream_t const ps = c.predict.st();
    ICZ_TRY(gemm_tn(tlogit, Vp, Vp, tcd, Hd, Hd, TB, dWp, Hd, 0, c.rl, ps));
    (void)launch_colsum(tlogit, TB, V, Vp, c.G.predict_b, ps);
    launch_weight_norm_bwd(dWp, Hd, P.predict_v, P.predict_g, n_pred, c.G.predict_v, c.G.predict_g, V, Hd, ps);
    return c.predict.finish();
}

// ---- the reverse-time loop
int Aoa::bptt_loop(BpttCall& c) {
    const int B = c.B, T = c.T, TB = c.TB, Hd = dims.Hd, NH = dims.NH, R = cur_R;
    const bool eo = c.eo;
    const int32_t* const rows_img = c.K > 1 ? imgk : nullptr;
    hipStream_t const st = c.st;
    if (rows_t[T - 1] < B || eo) {      // ragged batch / steps that never ran: those rows contribute exact zeros to the batched GEMMs
        ICZ_CHECK_HIP(hipMemsetAsync(dZ, 0, sizeof(float) * (size_t)TB * 2 * Hd, st));
        ICZ_CHECK_HIP(hipMemsetAsync(dQp, 0, sizeof(float) * (size_t)TB * Hd, st));
        ICZ_CHECK_HIP(hipMemsetAsync(dQn, 0, sizeof(float) * (size_t)TB * Hd, st));
        ICZ_CHECK_HIP(hipMemsetAsync(dG, 0, sizeof(float) * (size_t)TB * 4 * Hd, st));
        ICZ_CHECK_HIP(hipMemsetAsync(tdS, 0, sizeof(float) * (size_t)TB * NH * R, st));
        ICZ_CHECK_HIP(hipMemsetAsync(tdX, 0, sizeof(float) * (size_t)TB * Hd, st));
    }
    DropCfg off = {0, nullptr, nullptr, 0, 0};
    int cur = 0, nsx = 1, bnext = 0;
    for (int t = T - 1; t >= 0; --t) {
        const int bt = rows_t[t];
        const size_t s0 = (size_t)t * B;
        const AoaStepIO io = train_io(bt, t, cur_train);
        const AoaStepIO io_next = train_io(bnext, t + 1 < T ? t + 1 : t, cur_train);
        const unsigned eb = (unsigned)(((size_t)bt * Hd + 255) / 256);
        const int* const live = (eo && t > 0) ? nunf + (t - 1) : nullptr;
        const int* const carry_live = (eo && t + 1 < T) ? nunf + t : nullptr;
        hipLaunchKernelGGL(aoa_glu_bwd_kernel, dim3(eb), dim3(256), 0, st, dCd + s0 * Hd, io.d_out, bnext ? (const float*)X : nullptr, nsx, bnext,
                           io_next.d_ctx, tz + s0 * 2 * Hd, dZ + s0 * 2 * Hd, bt, Hd, live, carry_live);
        int ns2 = 1, nsq = 1;
        ICZ_TRY(nn(dZ + s0 * 2 * Hd, 2 * Hd, bt, 2 * Hd, P.dec.aoa_w, 2 * Hd, 2 * Hd, X2, xfloats, &ns2, split_backward(STEP_WGS), st, live));
        aoa_launch_dec_attn_bwd(X2, ns2, bt, tP + s0 * NH * R, tPd + s0 * NH * R, tQp + s0 * Hd, Kd, Vd, dQp + s0 * Hd, tdS + s0 * NH * R, tdX + s0 * Hd, R,
                                Hd, NH, region_rows(), io.d_att.mode ? io.d_att.scale : 1.0f, live, rows_img, st);
        ICZ_TRY(nn(dQp + s0 * Hd, Hd, bt, Hd, P.dec.q_w, Hd, Hd, ws, ws_floats, &nsq, split_backward(STEP_WGS), st, live));
        aoa_launch_ln_bwd(ws, nsq, X2, ns2, bt, th + (s0 + B) * Hd, tstats + s0 * 2, P.dec.ln_g, dQn + s0 * Hd, dHln, Hd, live, st);
        LstmBwdArgs a = {};
        a.dh_a = bnext ? X + Hd : nullptr; a.ns_a = nsx; a.lda_a = 2 * Hd; a.rows_a = bnext;
        a.dh_b = dHln; a.ns_b = 1; a.lda_b = Hd; a.rows_b = bt;
        a.dc_in = bnext ? dcb[cur] : nullptr; a.dc_in_rows = bnext;
        a.gates = tg + s0 * 4 * Hd;
        a.c_prev = tm + s0 * Hd; a.c_cur = tm + (s0 + B) * Hd;
        a.dgates = dG + s0 * 4 * Hd; a.dc_prev = dcb[cur ^ 1];
        a.rows = bt; a.H = Hd; a.live = live; a.carry_live = carry_live;
        hipLaunchKernelGGL(lstm_bwd_point_kernel, dim3(cdiv(Hd, 256), bt), dim3(256), 0, st, a, off);
        // [du_t | dh_{t-1}] = dgates_t . [W_ih[:, E:] | W_hh]
        if (t > 0) ICZ_TRY(nn(dG + s0 * 4 * Hd, 4 * Hd, bt, 4 * Hd, w_rec, 2 * Hd, 2 * Hd, X, xfloats, &nsx, split_backward(STEP_WGS), st, live));
        bnext = bt;
        cur ^= 1;
    }
    return ICZ_OK;
}

// ---- embedding gradient and the LSTM's weight gradients
int Aoa::bptt_embed_lstm_wgrad(BpttCall& c) {
    const int TB = c.TB, Hd = dims.Hd, E = dims.E, V = dims.V;
    const icz_aoa_params& G = c.G;
    const int* const rl = c.rl;
    hipStream_t const st = c.st;
    int ns = 1;
    ICZ_TRY(nn(dG, 4 * Hd, TB, 4 * Hd, P.lstm_w_ih, E + Hd, E, X, xfloats, &ns, split_backward(TARGET_WGS), st, nullptr, rl));
    ICZ_TRY(launch_slab_reduce(X, ns, TB, E, nullptr, dEmb, st));      // (one slab: a copy)
    ICZ_CHECK_HIP(embed_grad_launch(st, tok, TB, dEmb, 1, (size_t)0, temb, cur_train ? 2.0f : 1.0f, E, G.embed_weight, V, 1, rl));
    // ---- weight gradients: one TN GEMM each over all (t, b) rows
    // (round 5) products that share d y go as one launch over column groups where the shape is taken (gemm_big_x3.hip)
    const GemmColGroup lstm_groups[3] = {{temb, E, E, G.lstm_w_ih, E + Hd}, {tu, Hd, Hd, G.lstm_w_ih + E, E + Hd}, {th, Hd, Hd, G.lstm_w_hh, Hd}};
    ICZ_TRY(gemm_tn_groups(dG, 4 * Hd, 4 * Hd, TB, lstm_groups, 3, nullptr, 0, rl, st));
    ICZ_TRY(launch_colsum(dG, TB, 4 * Hd, 4 * Hd, G.lstm_b_ih, st));
    ICZ_CHECK_HIP(hipMemcpyAsync(G.lstm_b_hh, G.lstm_b_ih, sizeof(float) * 4 * Hd, hipMemcpyDeviceToDevice, st));
    return ICZ_OK;
}

// ---- the AoA linear layer's gradients
int Aoa::bptt_aoa_wgrad(BpttCall& c) {
    const int Hd = dims.Hd;
    const GemmColGroup aoa_groups[2] = {{txatt, Hd, Hd, c.G.dec.aoa_w, 2 * Hd}, {tqn, Hd, Hd, c.G.dec.aoa_w + Hd, 2 * Hd}};
    ICZ_TRY(gemm_tn_groups(dZ, 2 * Hd, 2 * Hd, c.TB, aoa_groups, 2, nullptr, 0, c.rl, c.st));
    return launch_colsum(dZ, c.TB, 2 * Hd, 2 * Hd, c.G.dec.aoa_b, c.st);
}

// ---- the attention block's small products (three Hd x Hd weight gradients, d K / d V, seven column sums: 240 us of kernels that fill a
//      fraction of the chip, eager timeline round 6) depend on the loop only: without a DP callback they run on the side stream beside
//      the embedding / LSTM / AoA-linear gradients
int Aoa::bptt_attention_tail(BpttCall& c) {
    const int B = c.B, T = c.T, TB = c.TB, K = c.K, n_img = c.n_img, Hd = dims.Hd, NH = dims.NH, R = cur_R, dh = Hd / NH;
    const size_t sH = (size_t)B * Hd;
    const icz_aoa_params& G = c.G;
    const int* const rl = c.rl;
    hipStream_t const ts = c.tail.st();
    ICZ_TRY(gemm_tn(dQp, Hd, Hd, tqn, Hd, Hd, TB, G.dec.q_w, Hd, 0, rl, ts));
    ICZ_TRY(launch_colsum(dQp, TB, Hd, Hd, G.dec.q_b, ts));
    aoa_launch_dkv(tdS, tPd, tQp, tdX, dKd, dVd, n_img, B, T, aoa_dkv_tc(K * T, R, dh), R, Hd, NH, region_rows(), K, ts);
    const int rrows = (int)region_row_count(n_img);      // region rows of the batch (packed valid rows with per-image counts)
    ICZ_TRY(gemm_tn(dKd, Hd, Hd, refined, Hd, Hd, rrows, G.dec.k_w, Hd, 0, nullptr, ts));
    ICZ_TRY(launch_colsum(dKd, rrows, Hd, Hd, G.dec.k_b, ts));
    ICZ_TRY(gemm_tn(dVd, Hd, Hd, refined, Hd, Hd, rrows, G.dec.v_w, Hd, 0, nullptr, ts));
    ICZ_TRY(launch_colsum(dVd, rrows, Hd, Hd, G.dec.v_b, ts));
    // ---- h_norm gain / bias
    {
        const size_t n = (size_t)TB * Hd;
        hipLaunchKernelGGL(aoa_ln_prod_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ts, dQn, th + sH, tstats, prod, (size_t)TB, Hd);
        ICZ_TRY(launch_colsum(prod, TB, Hd, Hd, G.dec.ln_g, ts));
        ICZ_TRY(launch_colsum(dQn, TB, Hd, Hd, G.dec.ln_b, ts));
    }
    return ICZ_OK;
}

void aoa_launch_ln_bwd(const float* dq_a, int ns_a, const float* dq_b, int ns_b, int rows, const float* x, const float* stats, const float* gain,
                       float* dq_tot, float* dx, int n, const int* live, hipStream_t st) {
    hipLaunchKernelGGL(aoa_ln_bwd_kernel, dim3(rows), dim3(256), 0, st, dq_a, ns_a, dq_b, ns_b, rows, x, stats, gain, dq_tot, dx, n, live);
}

// decoder attention backward of one step (the limit of its dynamic LDS: aoa_raise_lds_limit, aoa.hip)
int aoa_dec_attn_bwd_optin(size_t lds) {
    static size_t raised[AOA_LDS_LIMIT_DEVICES] = {};
    return aoa_raise_lds_limit(reinterpret_cast<const void*>(aoa_dec_attn_bwd_kernel), lds, raised);
}
void aoa_launch_dec_attn_bwd(const float* dxq, int ns, int rows, const float* Pm, const float* Pdm, const float* Qp, const float* Kd, const float* Vd,
                             float* dQp, float* dS_out, float* dx_out, int R, int Hd, int NH, const RegionRows& rr, float keep_scale, const int* live,
                             const int32_t* img_of_row, hipStream_t st) {
    hipLaunchKernelGGL(aoa_dec_attn_bwd_kernel, dim3(rows, NH), dim3(256), aoa_dec_attn_bwd_lds(R, Hd / NH), st, dxq, ns, rows, Pm, Pdm, Qp, Kd, Vd, dQp,
                       dS_out, dx_out, R, Hd, NH, rr, keep_scale, live, img_of_row);
}

// d K / d V of the hoisted projections: the (k, t) pairs of an image go through LDS in chunks of tc pairs (aoa_dkv_tc: all of them when they
// fit 48 KB)
void aoa_launch_dkv(const float* dS_all, const float* Pd_all, const float* Qp_all, const float* dx_all, float* dKd, float* dVd, int n_img, int B, int T,
                    int tc, int R, int Hd, int NH, const RegionRows& rr, int G, hipStream_t st) {
    hipLaunchKernelGGL(aoa_dkv_kernel, dim3(n_img, NH), dim3(256), aoa_dkv_lds(tc, R, Hd / NH), st, dS_all, Pd_all, Qp_all, dx_all, dKd, dVd, B, T, tc,
                       R, Hd, NH, rr, G);
}

}  // namespace icz

// ================================================================================================
using namespace icz;
extern "C" {

// Test entry of aoa_dec_attn_bwd_kernel (include/icz.h): host checks, the handle's opt-in and launch.
int icz_test_aoa_dec_attn_bwd(const float* dxq, int32_t ns, int32_t rows, const float* P, const float* Pd, const float* Qp, const float* Kd,
                              const float* Vd, float* dQp, float* dS_out, float* dx_out, int32_t n_img, int32_t R, int32_t Hd, int32_t NH,
                              const int32_t* counts, float keep_scale, const int32_t* live, const int32_t* img_of_row, void* stream) {
    const char* who = "icz_test_aoa_dec_attn_bwd";
    ICZ_REQUIRE(dxq && P && Pd && Qp && Kd && Vd && dQp && dS_out && dx_out && rows >= 1 && n_img >= 1, "%s: null argument, no row or no image", who);
    ICZ_TRY(aoa_test_heads(who, R, Hd, NH));
    ICZ_REQUIRE(aoa_al16(Kd) && aoa_al16(Vd), "%s: Kd and Vd must be 16-byte aligned", who);
    ICZ_REQUIRE(ns >= 1 && ns <= 16, "%s: %d slabs of the GLU-input gradient (1..16)", who, ns);
    ICZ_REQUIRE(keep_scale >= 1.0f, "%s: keep_scale %g (1 without dropout, else 1 / (1 - p))", who, (double)keep_scale);
    ICZ_REQUIRE(img_of_row || rows <= n_img, "%s: %d rows over %d images need img_of_row", who, rows, n_img);
    const size_t lds = aoa_dec_attn_bwd_lds(R, Hd / NH);
    ICZ_REQUIRE(lds <= AOA_LDS_BUDGET, "%s: K and V head tiles of %d regions x %d columns need %zu bytes of LDS (limit %zu)", who, R, Hd / NH, lds,
                AOA_LDS_BUDGET);
    if (img_of_row) {
        std::vector<int32_t> ior;
        ICZ_TRY(aoa_test_read_i32(img_of_row, rows, &ior));
        for (int i = 0; i < rows; ++i) ICZ_REQUIRE(ior[i] >= 0 && ior[i] < n_img, "%s: row %d decodes image %d of %d", who, i, ior[i], n_img);
    }
    ICZ_TRY(aoa_dec_attn_bwd_optin(lds));
    AoaTestRegions reg;
    RegionRows rr;
    ICZ_TRY(reg.build(who, counts, n_img, R, (hipStream_t)stream, &rr));
    aoa_launch_dec_attn_bwd(dxq, ns, rows, P, Pd, Qp, Kd, Vd, dQp, dS_out, dx_out, R, Hd, NH, rr, keep_scale, live, img_of_row, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// Test entry of the two LayerNorm backward kernels (include/icz.h): form 0 aoa_ln_bwd_kernel, form 1 aoa_ln_bwd_dense_kernel.
int icz_test_aoa_ln_bwd(int32_t form, const float* dq_a, int32_t ns_a, const float* dq_b, int32_t ns_b, int32_t rows, const float* x, const float* stats,
                        const float* gain, const float* res, float* dq_tot, float* prod, float* dx, int32_t n, const int32_t* live, void* stream) {
    const char* who = "icz_test_aoa_ln_bwd";
    ICZ_REQUIRE(form == 0 || form == 1, "%s: form %d (0: aoa_ln_bwd_kernel, 1: aoa_ln_bwd_dense_kernel)", who, form);
    ICZ_REQUIRE(x && gain && dx && rows >= 1, "%s: null argument or no row", who);
    ICZ_REQUIRE(n >= 4 && n % 4 == 0 && n <= 4096, "%s: a row of %d columns (a multiple of 4, at most 4096: the row is kept in registers)", who, n);
    ICZ_REQUIRE(aoa_al16(dq_a) && aoa_al16(dq_b) && aoa_al16(x) && aoa_al16(gain) && aoa_al16(res) && aoa_al16(dq_tot) && aoa_al16(prod) && aoa_al16(dx),
                "%s: every tensor must be 16-byte aligned", who);
    if (form == 0) {
        ICZ_REQUIRE(dq_a && dq_b && stats && dq_tot && !res && !prod, "%s: form 0 takes dq_a, dq_b, stats and dq_tot, and neither res nor prod", who);
        ICZ_REQUIRE(ns_a >= 1 && ns_a <= 16 && ns_b >= 1 && ns_b <= 16, "%s: form 0 with %d and %d slabs (1..16 each)", who, ns_a, ns_b);
        aoa_launch_ln_bwd(dq_a, ns_a, dq_b, ns_b, rows, x, stats, gain, dq_tot, dx, n, live, (hipStream_t)stream);
    } else {
        ICZ_REQUIRE(prod && !stats && !live && ns_b == 0, "%s: form 1 takes prod, and neither stats nor live nor slabs of dq_b", who);
        ICZ_REQUIRE(dq_a ? (ns_a >= 1 && ns_a <= 16) : ns_a == 0, "%s: form 1 with %d slabs of %s dq_a", who, ns_a, dq_a ? "a given" : "a null");
        aoa_launch_ln_bwd_dense(dq_a, ns_a, dq_b, rows, x, gain, res, dq_tot, prod, dx, n, (hipStream_t)stream);
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// Test entry of aoa_dkv_kernel (include/icz.h): host checks, the handle's chunk rule or a forced chunk, the handle's launch.
int icz_test_aoa_dkv(const float* dS_all, const float* Pd_all, const float* Qp_all, const float* dx_all, float* dKd, float* dVd, int32_t n_img,
                     int32_t B, int32_t T, int32_t tc, int32_t R, int32_t Hd, int32_t NH, const int32_t* counts, int32_t G, int32_t* tc_out,
                     void* stream) {
    const char* who = "icz_test_aoa_dkv";
    ICZ_REQUIRE(dS_all && Pd_all && Qp_all && dx_all && dKd && dVd, "%s: null argument", who);
    ICZ_TRY(aoa_test_heads(who, R, Hd, NH));
    ICZ_REQUIRE(n_img >= 1 && G >= 1 && T >= 1, "%s: n_img=%d, G=%d, T=%d", who, n_img, G, T);
    // the handle's decoder rows are the images' rows and nothing else (row img * G + k): any other row count is not the library's layout
    ICZ_REQUIRE((int64_t)B == (int64_t)n_img * G, "%s: %d decoder rows per step are not %d images x %d rows", who, B, n_img, G);
    const int d = Hd / NH, pairs = G * T;
    const int chunk = tc ? tc : aoa_dkv_tc(pairs, R, d);
    ICZ_REQUIRE(chunk >= 1 && chunk <= pairs && aoa_dkv_lds(chunk, R, d) <= 48 * 1024, "%s: a chunk of %d of the %d (k, t) pairs (0: the handle's rule, "
                "else 1..%d; at most 48 KB of LDS: %zu bytes)", who, chunk, pairs, pairs, chunk > 0 ? aoa_dkv_lds(chunk, R, d) : (size_t)0);
    if (tc_out) *tc_out = chunk;
    AoaTestRegions reg;
    RegionRows rr;
    ICZ_TRY(reg.build(who, counts, n_img, R, (hipStream_t)stream, &rr));
    aoa_launch_dkv(dS_all, Pd_all, Qp_all, dx_all, dKd, dVd, n_img, B, T, chunk, R, Hd, NH, rr, G, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_aoa_sample(icz_aoa_t* h, const float* feats, int32_t B, int32_t max_len, const icz_aoa_rng* rng, int64_t* seq_out,
                   float* logprobs_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Aoa*>(h)->sample(feats, B, max_len, rng, seq_out, logprobs_out, (hipStream_t)stream);
}
int icz_aoa_sample_n(icz_aoa_t* h, const float* feats, int32_t B, int32_t K, int32_t max_len, const icz_aoa_rng* rng, int64_t* seq_out,
                     float* logprobs_out, void* stream) {
    ICZ_REQUIRE(K >= 2 && K <= SAMPLE_N_MAX_K, "icz_aoa_sample_n: K=%d samples per image outside 2..%d", K, SAMPLE_N_MAX_K);
    ICZ_REQUIRE(h, "icz_aoa_sample_n: null handle");
    return reinterpret_cast<Aoa*>(h)->sample_n(feats, B, K, max_len, rng, seq_out, logprobs_out, (hipStream_t)stream);
}
int icz_aoa_scst_rollouts(icz_aoa_t* h, const float* feats, int32_t B, int32_t max_len, const icz_aoa_rng* rng, int64_t* ids_out,
                          int64_t* seq_out, float* logprobs_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Aoa*>(h)->rollouts(feats, B, max_len, rng, ids_out, seq_out, logprobs_out, (hipStream_t)stream);
}
int icz_aoa_sample_backward(icz_aoa_t* h, const float* reward, const icz_aoa_params* grads, float* loss_out, float* mask_sum_out,
                            float mask_sum_global, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::ROLLOUT, "aoa", "aoa sample_backward"};
    hd.rollout = {reward, nullptr, loss_out, nullptr, mask_sum_out};
    hd.norm_global = mask_sum_global;
    return reinterpret_cast<Aoa*>(h)->backward(hd, grads, (hipStream_t)stream);
}
// sample_backward with an SCST objective (scst_objective.hip) in the place of RewardCriterion
int icz_aoa_sample_backward_objective(icz_aoa_t* h, const icz_scst_objective* obj, const icz_aoa_params* grads, float* loss_out3, float* ent_out,
                                      float* mask_sum_out, float mask_sum_global, void* stream) {
    ScstObjective o;
    ICZ_TRY(icz::scst_objective_args("icz_aoa_sample_backward_objective", obj, obj ? obj->K : 1, 1, &o));
    ICZ_REQUIRE(grads && loss_out3, "icz_aoa_sample_backward_objective: null argument");
    ICZ_REQUIRE(h, "icz_aoa_sample_backward_objective: null handle");
    LossHead hd = {LossHead::ROLLOUT, "aoa", "aoa sample_backward_objective"};
    hd.rollout = {nullptr, &o, loss_out3, ent_out, mask_sum_out};
    hd.objective = obj;
    hd.norm_global = mask_sum_global;
    return reinterpret_cast<Aoa*>(h)->backward(hd, grads, (hipStream_t)stream);
}
int icz_aoa_set_scheduled_sampling(icz_aoa_t* h, float ss_prob, const float* gate_uniforms, const float* draw_uniforms) {
    return set_scheduled_sampling("icz_aoa_set_scheduled_sampling", reinterpret_cast<Aoa*>(h), ss_prob, gate_uniforms, draw_uniforms);
}
int icz_aoa_xe_forward(icz_aoa_t* h, const float* feats, const int64_t* captions, int32_t B, int32_t L, const int32_t* lengths_host,
                       const icz_aoa_rng* rng, int32_t train, float* packed_logits_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Aoa*>(h)->xe_forward(feats, captions, B, L, lengths_host, rng, train, packed_logits_out, (hipStream_t)stream);
}
int icz_aoa_saved_alphas(icz_aoa_t* h, float* alphas_out, void* stream) {
    ICZ_REQUIRE(h && alphas_out, "icz_aoa_saved_alphas: null argument");
    Aoa* a = reinterpret_cast<Aoa*>(h);
    ICZ_REQUIRE(a->mode != 0 && a->tP, "icz_aoa_saved_alphas: no forward pass stored");
    launch_saved_alphas(a->tP, a->cur_T, a->cur_B, a->dims.NH, a->cur_R, alphas_out, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}
int icz_aoa_set_grad_callback(icz_aoa_t* h, icz_grad_ready_cb cb, void* user) {
    ICZ_REQUIRE(h, "null handle");
    Aoa* a = reinterpret_cast<Aoa*>(h);
    a->grad_cb = cb; a->grad_cb_user = user;
    return ICZ_OK;
}
int icz_aoa_set_norm_global(icz_aoa_t* h, const float* norm_dev, void* stream) {
    return set_norm_global("icz_aoa_set_norm_global", reinterpret_cast<Aoa*>(h), norm_dev, stream);
}
int icz_aoa_xe_backward(icz_aoa_t* h, float smoothing, const icz_aoa_params* grads, float* loss_out, float n_tokens_global, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::XE, "aoa", "aoa xe_backward"};
    hd.smoothing = smoothing; hd.loss_out = loss_out; hd.norm_global = n_tokens_global;
    return reinterpret_cast<Aoa*>(h)->backward(hd, grads, (hipStream_t)stream);
}
int icz_aoa_xe_backward_distill(icz_aoa_t* h, const icz_distill_opts* opts, const icz_aoa_params* grads, float* loss_out3, float n_tokens_global,
                                void* stream) {
    Aoa* a = reinterpret_cast<Aoa*>(h);
    DistillArgs d;
    ICZ_TRY(distill_args("icz_aoa_xe_backward_distill", opts, a ? a->dims.V : -1, &d));
    ICZ_REQUIRE(grads && loss_out3, "icz_aoa_xe_backward_distill: null grads or loss");
    ICZ_REQUIRE(h, "icz_aoa_xe_backward_distill: null handle");
    LossHead hd = {LossHead::XE_DISTILL, "aoa", "aoa xe_backward_distill"};
    hd.distill = &d; hd.loss_out = loss_out3; hd.norm_global = n_tokens_global;
    return a->backward(hd, grads, (hipStream_t)stream);
}
int icz_aoa_xe_backward_swor(icz_aoa_t* h, const icz_swor_opts* opts, int32_t rows, const icz_aoa_params* grads, float* loss_out, void* stream) {
    SworArgs a;
    ICZ_TRY(swor_args("icz_aoa_xe_backward_swor", opts, rows, &a));
    ICZ_REQUIRE(grads && loss_out, "icz_aoa_xe_backward_swor: null grads or loss");
    ICZ_REQUIRE(h, "icz_aoa_xe_backward_swor: null handle");
    LossHead hd = {LossHead::XE_SWOR, "aoa", "aoa xe_backward_swor"};
    hd.swor = &a; hd.swor_rows = rows; hd.loss_out = loss_out;
    return reinterpret_cast<Aoa*>(h)->backward(hd, grads, (hipStream_t)stream);
}
// xe_backward driven by an upstream gradient w.r.t. the packed logits
int icz_aoa_xe_backward_dlogits(icz_aoa_t* h, const float* dpacked, const icz_aoa_params* grads, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::XE_DLOGITS, "aoa", "aoa xe_backward_dlogits"};
    hd.upstream = dpacked;
    return reinterpret_cast<Aoa*>(h)->backward(hd, grads, (hipStream_t)stream);
}

}  // extern "C"
