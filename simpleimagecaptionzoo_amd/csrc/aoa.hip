// AoADetection captioner, inference paths: feature projection + AoA refiner, decoder step, greedy and beam decoding
// (Models/AoA_Model.py:122-162, 319-336, 403-502, 698-753).  Training paths live in aoa_train.hip.
#include <mutex>

#include "aoa_impl.h"
#include "aoa_test_support.h"
#include "lstm_kernels.h"
#include "support_kernels.h"
#include "token_kernels.h"

namespace icz {

int Aoa::init(const icz_aoa_dims& d) {
    dims = d;
    ICZ_REQUIRE(d.NH > 0 && d.Hd % d.NH == 0 && (d.Hd / d.NH) % 4 == 0, "aoa: hidden size %d must split into %d heads of a multiple of 4 columns", d.Hd, d.NH);
    ICZ_REQUIRE(d.E % 4 == 0 && d.Hd % 4 == 0 && d.D % 4 == 0 && d.V > 3 && d.max_rows > 0 && d.max_len > 0, "aoa: bad dimensions");
    ICZ_REQUIRE(d.R >= 1 && d.R <= 128, "aoa: %d regions per image (supported: 1..128)", d.R);
    const size_t dh = d.Hd / d.NH;
    // per-(image, head) tiles live in LDS: K, V [R][dh+1] + a chunk of queries with its P rows in the refiner, K, V in the
    // decoder.  gfx950 has 160 KB per CU; above the 64 KB default the kernels need the explicit opt-in below (49 regions x
    // 128 columns: 86 KB; 100 regions: K and V take 103 KB and the queries go through in chunks, see self_qc())
    cur_R = d.R;
    ICZ_REQUIRE(self_qc(d.R) >= 1, "aoa: K and V head tiles of %d regions do not fit the LDS budget", d.R);
    ICZ_TRY(aoa_self_attn_optin(self_lds(d.R, self_qc(d.R))));
    ICZ_TRY(aoa_dec_attn_optin(aoa_dec_attn_lds(d.R, (int)dh)));
    Vp = pad_vocab(d.V);
    const size_t rows = d.max_rows, Hd = d.Hd, E = d.E, RR = rows * d.R;
    ICZ_TRY(alloc((void**)&w_pred, sizeof(float) * Vp * Hd));
    ICZ_TRY(alloc((void**)&n_pred, sizeof(float) * d.V));
    ICZ_TRY(alloc((void**)&w_rec, sizeof(float) * 4 * Hd * 2 * Hd));
    static_assert(NL <= AOA_QKV_MAX_LAYERS, "QkvPackTable too small");
    for (int l = 0; l < NL; ++l) {
        ICZ_TRY(alloc((void**)&w_qkv[l], sizeof(float) * 3 * Hd * Hd));
        ICZ_TRY(alloc((void**)&b_qkv[l], sizeof(float) * 3 * Hd));
    }
    ICZ_TRY(alloc((void**)&zeros, sizeof(float) * rows * Hd));
    const size_t nmax = 4 * Hd > (size_t)Vp ? 4 * Hd : (size_t)Vp;
    ws_floats = (size_t)TARGET_WGS * 4096 * 2 + rows * nmax;
    {   // the resident decoder-step GEMMs (33..128 rows) leave one slab per 256-deep k range (Butd::init's rule): the LSTM gates take
        // K = E + 2 Hd, the AoA linear K = 2 Hd with N = 2 Hd -- without this the split shrinks to fit and the launch falls to the fp32 kernel
        const size_t kmax = E + 2 * Hd, r128 = rows < 128 ? rows : 128;
        const size_t need = (kmax / 256 + 1) * r128 * 4 * Hd;
        if (need > ws_floats) ws_floats = need;
    }
    for (int b = 0; b < 2; ++b) {
        Bank& s = bank[b];
        float** ref[] = {&s.xa, &s.xb, &s.ln, &s.o, &s.od, &s.nd, &s.refined, &s.Kd, &s.Vd};
        for (float** p : ref) ICZ_TRY(alloc((void**)p, sizeof(float) * RR * Hd));
        ICZ_TRY(alloc((void**)&s.qkv, sizeof(float) * RR * 3 * Hd));
        ICZ_TRY(alloc((void**)&s.z, sizeof(float) * RR * 2 * Hd));
        ICZ_TRY(alloc((void**)&s.meanf, sizeof(float) * rows * Hd));
        ICZ_TRY(alloc((void**)&s.ws, sizeof(float) * ws_floats));
        ICZ_TRY(alloc((void**)&s.off, sizeof(int32_t) * (rows + 1)));
        ICZ_TRY(alloc((void**)&s.rowmap, sizeof(int32_t) * RR));
    }
    own[0] = bank[0]; own[1] = bank[1];
    use_bank(0);
    for (int i = 0; i < 2; ++i) {
        ICZ_TRY(alloc((void**)&h[i], sizeof(float) * rows * Hd));
        ICZ_TRY(alloc((void**)&m[i], sizeof(float) * rows * Hd));
        ICZ_TRY(alloc((void**)&ctx[i], sizeof(float) * rows * Hd));
    }
    ICZ_TRY(alloc((void**)&emb, sizeof(float) * rows * E));
    float** st[] = {&u, &qn, &Qp, &xatt, &ctxdrop};
    for (float** p : st) ICZ_TRY(alloc((void**)p, sizeof(float) * rows * Hd));
    ICZ_TRY(alloc((void**)&logits, sizeof(float) * rows * Vp));
    ICZ_TRY(alloc((void**)&it, sizeof(int64_t) * rows));
    ICZ_TRY(alloc((void**)&amax_val, sizeof(float) * rows * ARGMAX_PARTS));
    ICZ_TRY(alloc((void**)&amax_idx, sizeof(int) * rows * ARGMAX_PARTS));
    ICZ_TRY(alloc_scalars(mem));
    return mem.synced();
}

__global__ __launch_bounds__(256) void aoa_pack_rec_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, float* __restrict__ w_rec,
                                                           int Hd, int E) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)4 * Hd * 2 * Hd) return;
    const size_t row = i / (2 * Hd);
    const int c = (int)(i % (2 * Hd));
    w_rec[i] = c < Hd ? w_ih[row * (E + Hd) + E + c] : w_hh[row * Hd + (c - Hd)];
}

int Aoa::refresh(hipStream_t st) {
    ICZ_REQUIRE(bound, "aoa: parameters not bound");
    launch_weight_norm(P.predict_v, P.predict_g, w_pred, n_pred, dims.V, dims.Hd, st);
    const size_t n = (size_t)4 * dims.Hd * 2 * dims.Hd;
    hipLaunchKernelGGL(aoa_pack_rec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P.lstm_w_ih, P.lstm_w_hh, w_rec, dims.Hd, dims.E);
    QkvPackTable qt = {};
    for (int l = 0; l < NL; ++l) {
        const icz_aoa_block& b = P.layer[l];
        qt.w[l][0] = b.q_w; qt.w[l][1] = b.k_w; qt.w[l][2] = b.v_w;
        qt.b[l][0] = b.q_b; qt.b[l][1] = b.k_b; qt.b[l][2] = b.v_b;
        qt.wdst[l] = w_qkv[l]; qt.bdst[l] = b_qkv[l];
    }
    hipLaunchKernelGGL(aoa_qkv_pack_kernel, dim3(cdiv(dims.Hd * dims.Hd / 4, 256), 3, NL), dim3(256), 0, st, qt, dims.Hd);
    ICZ_CHECK_HIP(hipGetLastError());
    fresh = true;
    return ICZ_OK;
}


// refiner self-attention of one layer over n_img images: the matrix-pipe kernel up to 64 regions, the register-blocked one beyond
void aoa_launch_mha_self(int n_img, int R, int Hd, int NH, bool mha_mfma, int qc, size_t lds, const RegionRows& rr, const float* qkv_, float* o_,
                         const DropP& dp, hipStream_t st) {
    if (aoa_self_route(R, Hd, NH, mha_mfma) == 2)
        hipLaunchKernelGGL(mha_self_mfma_kernel, dim3(n_img, NH), dim3(256), AOA_SELF_MFMA_LDS, st, qkv_, qkv_ + Hd, qkv_ + 2 * Hd, o_, R, Hd, NH, rr, dp, 3 * Hd);
    else
        hipLaunchKernelGGL(mha_self_kernel, dim3(n_img, NH), dim3(256), lds, st, qkv_, qkv_ + Hd, qkv_ + 2 * Hd, o_, R, Hd, NH, qc, rr, dp, 3 * Hd);
}

// The dynamic-LDS limit of a kernel is process-wide: it is raised to the largest launch any handle or test entry has asked for and never
// lowered (a second, smaller handle must not take the limit away from under the first one's launches).  One mutex for all kernels:
// handles may be created from several threads.
int aoa_raise_lds_limit(const void* kernel, size_t lds, size_t* raised) {
    static std::mutex mu;
    if (lds <= 48 * 1024) return ICZ_OK;
    int dev = 0;
    ICZ_CHECK_HIP(hipGetDevice(&dev));
    const bool known = dev >= 0 && dev < AOA_LDS_LIMIT_DEVICES;
    std::lock_guard<std::mutex> lock(mu);
    if (known && lds <= raised[dev]) return ICZ_OK;
    ICZ_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (known) raised[dev] = lds;
    return ICZ_OK;
}
int aoa_self_attn_optin(size_t lds) {
    static size_t raised[AOA_LDS_LIMIT_DEVICES] = {};
    return aoa_raise_lds_limit(reinterpret_cast<const void*>(mha_self_kernel), lds, raised);
}
int aoa_dec_attn_optin(size_t lds) {
    static size_t raised[AOA_LDS_LIMIT_DEVICES] = {};
    return aoa_raise_lds_limit(reinterpret_cast<const void*>(aoa_dec_attn_kernel), lds, raised);
}

void aoa_launch_layer_norm(int geometry, const float* x, const float* gain, const float* bias, float* y, int rows, int n, float* stats,
                           const int* live, hipStream_t st) {
    if (geometry == 0) hipLaunchKernelGGL(layer_norm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, gain, bias, y, rows, n, stats, live);
    else hipLaunchKernelGGL(layer_norm_kernel, dim3(rows), dim3(64), 0, st, x, gain, bias, y, rows, n, stats, live);
}

void aoa_launch_dec_attn(const float* Qp, int qns, size_t q_stride, const float* q_bias, float* Qp_store, const float* Kd, const float* Vd,
                         const int32_t* img_of_row, float* xatt, float* P_out, float* Pd_out, int rows, int R, int Hd, int NH, const RegionRows& rr,
                         const DropP& dp, const int* live, hipStream_t st) {
    const size_t lds = aoa_dec_attn_lds(R, Hd / NH);
    if (qns == 1)
        hipLaunchKernelGGL(aoa_dec_attn_kernel, dim3(rows, NH), dim3(256), lds, st, Qp, Kd, Vd, img_of_row, xatt, P_out, Pd_out, R, Hd, NH, rr, dp, 1,
                           (size_t)0, (const float*)nullptr, (float*)nullptr, live);
    else
        hipLaunchKernelGGL(aoa_dec_attn_kernel, dim3(rows, NH), dim3(256), lds, st, Qp, Kd, Vd, img_of_row, xatt, P_out, Pd_out, R, Hd, NH, rr, dp, qns,
                           q_stride, q_bias, Qp_store, live);
}

void Aoa::mha_self_layer(int n_img, int l, bool train, hipStream_t st) {
    const int R = cur_R, qc = self_qc(R);
    launch_mha_self(n_img, R, qc, self_lds(R, qc), region_rows(), qkv, o,
                    dropp(train, rng.ref_att_mask, (size_t)l * n_img * dims.NH * R * R, AOA_RNG_REF_ATT, l, 0.1f), st);
}

// (the split is fitted to the workspace: the capacity check of gemm_finished cannot fail)
int Aoa::linear(GemmArgs g, const float* bias, hipStream_t st) {
    return gemm_finished(GEMM_NT, g, split_forward(STEP_WGS), bias, ws, ws_floats, st, "aoa");
}

int Aoa::lin(const float* A, int M, int K, const float* W, const float* bias, int N, float* out, hipStream_t st) {
    return linear(gemm_args({{A, W, K, K, K}}, M, N, out, N), bias, st);
}

// img_feats_porjection + AoA_Refine_Core (AoA_Model.py:661-665, 140-162) -> refined [n_img,R,Hd], its region mean, and the
// decoder block's linear_K / linear_V of it (time-invariant, hoisted out of the decoding loop)
// proj != null: img_feats_porjection(feats) has been computed (Aoa::project, packed rows for 'adaptive' batches): only its ReLU / dropout runs
int Aoa::refine(const float* feats, int n_img, bool train, hipStream_t st, const float* proj) {
    point_bank_at_own(cur_bank);          // (a pass of its own never writes into the halves of a paired pass another chain may still read)
    const int R = cur_R, Hd = dims.Hd, NH = dims.NH;
    ICZ_REQUIRE(!lens || lens_n == n_img, "aoa: region counts were set for %d images, the batch has %d (icz_aoa_set_regions)", lens_n, n_img);
    const int rows = (int)region_row_count(n_img);
    const RegionRows rr = region_rows();
    const size_t nel = (size_t)rows * Hd;
    const unsigned eb = (unsigned)((nel + 255) / 256);
    const float* xin = feats;
    if (lens && !proj) {      // 'adaptive' features: the refiner runs on the valid rows only (packed)
        if (!bank[0].featp)
        {
            for (int b = 0; b < 2; ++b) ICZ_TRY(alloc((void**)&bank[b].featp, sizeof(float) * (size_t)dims.max_rows * dims.R * dims.D));
            ICZ_TRY(mem.synced());
        }
        float* featp = bank[cur_bank].featp;
        hipLaunchKernelGGL(aoa_offsets_kernel, dim3(1), dim3(256), 0, st, lens, n_img, R, off, rowmap);
        const size_t n4 = (size_t)rows * (dims.D / 4);
        hipLaunchKernelGGL(aoa_pack_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, feats, (const int32_t*)rowmap, featp,
                           (size_t)rows, dims.D);
        xin = featp;
    }
    if (!proj) ICZ_TRY(lin(xin, rows, dims.D, P.proj_w, P.proj_b, Hd, xa, st));
    // option "train_refiner": a training-mode pass runs its residual chain through xs[0..NL] instead of the ping-pong pair and so leaves
    // the input of every layer behind for the backward pass (same kernels, same values)
    const bool store = train && train_refiner;
    if (store) {
        ICZ_REQUIRE(xs[0] && n_img <= tcap_I, "aoa: the refiner's training buffers are not allocated for %d images", n_img);
        ref_feats = xin; xs_valid = true;
    }
    hipLaunchKernelGGL(relu_drop_kernel, dim3(eb), dim3(256), 0, st, proj ? proj : (const float*)xa, store ? xs[0] : xa, nel,
                       dropp(train, rng.proj_mask, 0, AOA_RNG_PROJ, 0, 0.5f), rr, Hd);
    const int qc = self_qc(R);
    const size_t lds = self_lds(R, qc);
    float *cur = store ? xs[0] : xa, *nxt = store ? xs[1] : xb;
    for (int l = 0; l < NL; ++l) {
        const icz_aoa_block& b = P.layer[l];
        aoa_launch_layer_norm(0, cur, b.ln_g, b.ln_b, ln, rows, Hd, nullptr, nullptr, st);
        ICZ_TRY(lin(ln, rows, Hd, w_qkv[l], b_qkv[l], 3 * Hd, qkv, st));         // linear_Q | linear_K | linear_V in one GEMM
        launch_mha_self(n_img, R, qc, lds, rr, qkv, o, dropp(train, rng.ref_att_mask, (size_t)l * n_img * NH * R * R, AOA_RNG_REF_ATT, l, 0.1f), st);
        const float *xo = o, *xn = ln;
        if (train) {
            hipLaunchKernelGGL(drop_concat_kernel, dim3(eb), dim3(256), 0, st, o, ln, od, nd, (size_t)rows, Hd, rr,
                               dropp(true, rng.ref_aoa_mask, (size_t)l * n_img * R * 2 * Hd, AOA_RNG_REF_AOA, l, 0.3f));
            xo = od; xn = nd;
        }
        ICZ_TRY(linear(gemm_args({{xo, b.aoa_w, Hd, 2 * Hd, Hd}, {xn, b.aoa_w + Hd, Hd, 2 * Hd, Hd}}, rows, 2 * Hd, z, 2 * Hd), b.aoa_b, st));
        hipLaunchKernelGGL(glu_residual_kernel, dim3(eb), dim3(256), 0, st, z, cur, nxt, (size_t)rows, Hd, rr,
                           dropp(train, rng.ref_sc_mask, (size_t)l * n_img * R * Hd, AOA_RNG_REF_SC, l, 0.1f));
        if (store) { cur = nxt; nxt = l + 2 <= NL ? xs[l + 2] : nullptr; }
        else { float* t_ = cur; cur = nxt; nxt = t_; }
    }
    aoa_launch_layer_norm(0, cur, P.ref_ln_g, P.ref_ln_b, refined, rows, Hd, nullptr, nullptr, st);
    hipLaunchKernelGGL(mean_rows_kernel, dim3(cdiv(Hd, 256), n_img), dim3(256), 0, st, refined, meanf, Hd, rr);
    ICZ_TRY(lin(refined, rows, Hd, P.dec.k_w, P.dec.k_b, Hd, Kd, st));
    ICZ_TRY(lin(refined, rows, Hd, P.dec.v_w, P.dec.v_b, Hd, Vd, st));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// The two refiner passes of an SCST step -- evaluation mode for the greedy baseline (Engine.py:256-258), training mode for the sampled
// rollout (:259-262) -- as ONE pass over [evaluation rows; training rows] (fixed region counts): every Linear is one GEMM of twice the rows
// (at 2 x 2304: the fused Q/K/V projection fills 216 tiles of 256 x 256 and runs on the eight-wave kernel), every small kernel one launch;
// dropout applies to the second half only, with the indices a pass of its own would use (DropP::idx0), so both halves hold the bits of
// the separate passes.  proj = img_feats_porjection(feats) before ReLU / dropout (Aoa::project), shared by both halves.
int Aoa::refine_pair(int n_img, hipStream_t st, const float* proj) {
    ICZ_REQUIRE(!lens && proj && dual.xa, "aoa refine_pair: fixed region counts, a shared projection and the pair buffers are needed");
    const int R = cur_R, Hd = dims.Hd, NH = dims.NH;
    const int rows = n_img * R, rows2 = 2 * rows, n2 = 2 * n_img;
    const RegionRows rr = region_rows();
    const size_t nel = (size_t)rows * Hd;
    const unsigned eb = (unsigned)((nel + 255) / 256), eb2 = (unsigned)((2 * nel + 255) / 256);
    const Bank& w = dual;
    auto second = [&](DropP d, size_t elems_first) { d.idx0 = elems_first; return d; };
    hipLaunchKernelGGL(relu_drop_kernel, dim3(eb), dim3(256), 0, st, proj, w.xa, nel, dropp(false, nullptr, 0, AOA_RNG_PROJ, 0, 0.5f), rr, Hd);
    hipLaunchKernelGGL(relu_drop_kernel, dim3(eb), dim3(256), 0, st, proj, w.xa + nel, nel, dropp(true, rng.proj_mask, 0, AOA_RNG_PROJ, 0, 0.5f), rr, Hd);
    // option "train_refiner": the training half's layer inputs are copied out for the backward pass (7 x nel floats)
    const bool store = train_refiner;
    if (store) {
        ICZ_REQUIRE(xs[0] && n_img <= tcap_I, "aoa: the refiner's training buffers are not allocated for %d images", n_img);
        ICZ_CHECK_HIP(hipMemcpyAsync(xs[0], w.xa + nel, sizeof(float) * nel, hipMemcpyDeviceToDevice, st));
    }
    const int qc = self_qc(R);
    const size_t lds = self_lds(R, qc);
    float *cur = w.xa, *nxt = w.xb;
    for (int l = 0; l < NL; ++l) {
        const icz_aoa_block& b = P.layer[l];
        aoa_launch_layer_norm(0, cur, b.ln_g, b.ln_b, w.ln, rows2, Hd, nullptr, nullptr, st);
        ICZ_TRY(lin(w.ln, rows2, Hd, w_qkv[l], b_qkv[l], 3 * Hd, w.qkv, st));
        launch_mha_self(n2, R, qc, lds, rr, w.qkv, w.o,
                        second(dropp(true, rng.ref_att_mask, (size_t)l * n_img * NH * R * R, AOA_RNG_REF_ATT, l, 0.1f), (size_t)n_img * NH * R * R), st);
        // dropout of [attention output | normed input] for the training half, in place (each thread rewrites the element it read)
        hipLaunchKernelGGL(drop_concat_kernel, dim3(eb), dim3(256), 0, st, w.o + nel, w.ln + nel, w.o + nel, w.ln + nel, (size_t)rows, Hd, rr,
                           dropp(true, rng.ref_aoa_mask, (size_t)l * n_img * R * 2 * Hd, AOA_RNG_REF_AOA, l, 0.3f));
        ICZ_TRY(linear(gemm_args({{w.o, b.aoa_w, Hd, 2 * Hd, Hd}, {w.ln, b.aoa_w + Hd, Hd, 2 * Hd, Hd}}, rows2, 2 * Hd, w.z, 2 * Hd), b.aoa_b, st));
        hipLaunchKernelGGL(glu_residual_kernel, dim3(eb2), dim3(256), 0, st, w.z, cur, nxt, (size_t)rows2, Hd, rr,
                           second(dropp(true, rng.ref_sc_mask, (size_t)l * n_img * R * Hd, AOA_RNG_REF_SC, l, 0.1f), nel));
        if (store) ICZ_CHECK_HIP(hipMemcpyAsync(xs[l + 1], nxt + nel, sizeof(float) * nel, hipMemcpyDeviceToDevice, st));
        float* t_ = cur; cur = nxt; nxt = t_;
    }
    aoa_launch_layer_norm(0, cur, P.ref_ln_g, P.ref_ln_b, w.refined, rows2, Hd, nullptr, nullptr, st);
    hipLaunchKernelGGL(mean_rows_kernel, dim3(cdiv(Hd, 256), n2), dim3(256), 0, st, w.refined, w.meanf, Hd, rr);
    ICZ_TRY(lin(w.refined, rows2, Hd, P.dec.k_w, P.dec.k_b, Hd, w.Kd, st));
    ICZ_TRY(lin(w.refined, rows2, Hd, P.dec.v_w, P.dec.v_b, Hd, w.Vd, st));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// img_feats_porjection alone (fixed region counts), for the two refiner passes of an SCST step to share (Aoa::rollouts)
int Aoa::project(const float* feats, int n_img, float* out, hipStream_t st) {
    return lin(feats, n_img * cur_R, dims.D, P.proj_w, P.proj_b, dims.Hd, out, st);
}

// One decoder step (AoA_Model.py:319-336)
int Aoa::step(const AoaStepIO& s, hipStream_t st) {
    const int rows = s.rows, Hd = dims.Hd, E = dims.E, NH = dims.NH, R = cur_R;
    const unsigned eb = (unsigned)(((size_t)rows * Hd + 255) / 256);
    if (!s.emb_ready) hipLaunchKernelGGL(embed_kernel, dim3(cdiv(E, 1024), rows), dim3(256), 0, st, P.embed_weight, s.it, s.emb, rows, E, s.d_emb, 1);
    if (!s.u_ready) hipLaunchKernelGGL(aoa_u_kernel, dim3(eb), dim3(256), 0, st, meanf, s.img_of_row, s.ctx_in, s.u, rows, Hd, s.d_ctx);
    // the step's products leave slabs [ns][rows][N] in the bank's workspace (one: the dense product) for the kernel behind them to
    // sum; the split is fitted to the workspace, so the capacity check of gemm_slabs cannot fail
    int ns;
    GemmArgs g = gemm_args({{s.emb, P.lstm_w_ih, E, E + Hd, E}, {s.u, P.lstm_w_ih + E, Hd, E + Hd, Hd}, {s.h_in, P.lstm_w_hh, Hd, Hd, Hd}},
                           rows, 4 * Hd, ws, 4 * Hd, s.live);
    ICZ_TRY(gemm_slabs(GEMM_NT, g, split_forward(STEP_WGS), ws, ws_floats, &ns, st, "aoa"));
    LstmPointArgs a = {ws, ns, nullptr, nullptr, P.lstm_b_ih, P.lstm_b_hh, s.m_in, s.h_out, s.m_out, s.gates_out, nullptr, rows, Hd, s.live};
    DropCfg off = {0, nullptr, nullptr, 0, 0};
    launch_lstm_point(a, off, st);
    aoa_launch_layer_norm(1, s.h_out, P.dec.ln_g, P.dec.ln_b, s.qn, rows, Hd, s.ln_stats, s.live, st);
    {   // query projection; when it is split over K its slabs go straight to the attention kernel, which sums them
        GemmArgs qg = gemm_args({{s.qn, P.dec.q_w, Hd, Hd, Hd}}, rows, Hd, s.Qp, Hd, s.live);      // one split: finished in Qp, with the bias
        qg.bias = P.dec.q_b;
        ICZ_TRY(gemm_slabs(GEMM_NT, qg, split_forward(STEP_WGS), ws, ws_floats, &ns, st, "aoa"));
        aoa_launch_dec_attn(ns == 1 ? s.Qp : ws, ns, (size_t)rows * Hd, P.dec.q_b, s.Qp, Kd, Vd, s.img_of_row, s.xatt, s.P_out, s.Pd_out, rows, R, Hd, NH,
                            region_rows(), s.d_att, s.live, st);
    }
    GemmArgs zg = gemm_args({{s.xatt, P.dec.aoa_w, Hd, 2 * Hd, Hd}, {s.qn, P.dec.aoa_w + Hd, Hd, 2 * Hd, Hd}}, rows, 2 * Hd, ws, 2 * Hd, s.live);
    ICZ_TRY(gemm_slabs(GEMM_NT, zg, split_forward(STEP_WGS), ws, ws_floats, &ns, st, "aoa"));
    hipLaunchKernelGGL(aoa_glu_kernel, dim3(eb), dim3(256), 0, st, ws, ns, P.dec.aoa_b, s.z_out, s.ctx_out, s.ctxdrop, rows, Hd, s.d_out,
                       (const float*)meanf, s.img_of_row, s.u_next, s.d_ctx_next, s.live);
    if (!s.skip_predict) ICZ_TRY(gemm_predict(s.ctxdrop, Hd, w_pred, P.predict_b, rows, dims.V, Vp, s.logits, Vp, ws, ws_floats, s.pred_nsplit, st, s.live));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

static AoaStepIO scratch_io(Aoa& a, int rows, const int32_t* img_of_row, int cur) {
    AoaStepIO s = {};
    s.rows = rows; s.img_of_row = img_of_row; s.it = a.it;
    s.h_in = a.h[cur]; s.m_in = a.m[cur]; s.ctx_in = a.ctx[cur];
    s.h_out = a.h[cur ^ 1]; s.m_out = a.m[cur ^ 1]; s.ctx_out = a.ctx[cur ^ 1];
    s.emb = a.emb; s.u = a.u; s.qn = a.qn; s.Qp = a.Qp; s.xatt = a.xatt; s.ctxdrop = a.ctxdrop; s.logits = a.logits;
    s.d_emb = a.dropbits(false, nullptr, 0, 0, 0);
    s.d_ctx = s.d_att = s.d_out = a.dropp(false, nullptr, 0, 0, 0, 0.5f);
    return s;
}

static int zero_state(Aoa& a, int rows, hipStream_t st) {
    ZeroList zl = {};
    zl.p[0] = a.h[0]; zl.p[1] = a.m[0]; zl.p[2] = a.ctx[0]; zl.count = 3;
    const size_t n = (size_t)rows * a.dims.Hd;
    hipLaunchKernelGGL(zero_bufs_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, zl, n);
    return ICZ_OK;
}

// AoA_Decoder.sample (AoA_Model.py:289-345) behind AoADetection_Captioner.sampler (:698-714)
// scst = true (the baseline of an SCST step, rollouts_impl): once EVERY row has emitted <end> the kernels of the remaining steps return
// at entry and their ids are 0 -- nothing behind a row's <end> reaches the reward (Utils.py:354); icz_aoa_greedy never does this
int Aoa::greedy(const float* feats, int B, int T, int64_t* ids_out, hipStream_t st, const float* proj, bool scst, bool refined_ready) {
    ICZ_REQUIRE(feats && ids_out && B > 0 && B <= dims.max_rows && T > 0, "aoa greedy: bad arguments");
    ICZ_REQUIRE(fresh, "aoa: call icz_aoa_refresh_weights after binding/updating parameters");
    use_bank(0);
    if (!refined_ready) ICZ_TRY(refine(feats, B, false, st, proj));
    ICZ_TRY(zero_state(*this, B, st));
    int* const gn = (scst && early_out && gnunf && tcap_T >= T && tcap_B >= B) ? gnunf : nullptr;
    hipLaunchKernelGGL(greedy_init_kernel, dim3(cdiv(B > T ? B : T, 256)), dim3(256), 0, st, it, B, gn, T);
    int cur = 0;
    bool track = false;
    for (int t = 0; t < T; ++t) {
        AoaStepIO s = scratch_io(*this, B, nullptr, cur);
        s.emb_ready = t > 0;
        s.u_ready = t > 0;                       // left by the previous step's GLU kernel (evaluation mode: no dropout)
        if (t + 1 < T) { s.u_next = u; s.d_ctx_next = s.d_ctx; }
        int pns = 1;
        s.pred_nsplit = &pns;
        if (track && t > 0) s.live = gn + (t - 1);
        ICZ_TRY(step(s, st));
        if (t == 0) track = gn && pns > 1;       // the one-launch select keeps the count (the two-kernel argmax of <= 32 rows does not)
        launch_greedy_select(logits_view(ws, P.predict_b, logits, B, Vp, pns), emb_slot(), B, dims.V, amax_val, amax_idx, it, ids_out, T, t,
                             track ? gunf : nullptr, track ? gn : nullptr, st);
        cur ^= 1;
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// ---- decoder seams (DecodeMember) ------------------------------------------------------------------------------------------------
// AoA_Decoder.beam_search_sample (AoA_Model.py:403-502), batched over images, is the shared driver (beam.hip) on these seams; the
// state (h, m, ctx) is re-gathered by source beam.
// prologue: the refiner pass (evaluation mode, bank 0; the region counts of icz_aoa_set_regions) and k zeroed state rows per image
int Aoa::prologue(const float* feats, int n_img, int k, const int32_t*, hipStream_t st) {
    ICZ_REQUIRE(fresh, "aoa: call icz_aoa_refresh_weights after binding/updating parameters");
    use_bank(0);
    ICZ_TRY(refine(feats, n_img, false, st));
    return zero_state(*this, n_img * k, st);
}

int Aoa::step(int rows, const int64_t* it_, const int32_t* img_of_row, int, int cur, bool slabs, LogitsView* out, hipStream_t st) {
    AoaStepIO s = scratch_io(*this, rows, img_of_row, cur);
    s.it = it_;
    s.emb_ready = seam_emb_ready; s.live = seam_live;
    int pns = 1;
    if (slabs) s.pred_nsplit = &pns;
    ICZ_TRY(step(s, st));
    if (out) *out = logits_view(ws, P.predict_b, logits, rows, Vp, pns);
    return ICZ_OK;
}

void Aoa::gather(const int32_t* src_row, int rows, int fan, hipStream_t st) {
    hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(dims.Hd, 1024), rows), dim3(256), 0, st, src_row, dims.Hd, h[1], m[1], ctx[1], h[1],
                       h[0], m[0], ctx[0], u, fan);
}

DecodeMember* aoa_member(void* handle) { return static_cast<DecodeMember*>(reinterpret_cast<Aoa*>(handle)); }

}  // namespace icz

// ================================================================================================
using namespace icz;
extern "C" {

int icz_aoa_create(const icz_aoa_dims* dims, icz_aoa_t** out) { return abi_create<Aoa>("icz_aoa_create", dims, out); }
int icz_aoa_destroy(icz_aoa_t* h) { delete reinterpret_cast<Aoa*>(h); return ICZ_OK; }
int icz_aoa_bind_params(icz_aoa_t* h, const icz_aoa_params* p) {
    ICZ_REQUIRE(h && p, "icz_aoa_bind_params: null argument");
    ICZ_TRY(check_param_table("icz_aoa_bind_params", p, sizeof(*p)));
    Aoa* n = reinterpret_cast<Aoa*>(h);
    if (n->bound && memcmp(&n->P, p, sizeof(*p)) != 0) {      // captured graphs carry the old parameter addresses
        ICZ_CHECK_HIP(hipDeviceSynchronize());
        n->gc.clear();
    }
    n->P = *p; n->bound = true; n->fresh = false;
    return ICZ_OK;
}
int icz_aoa_set_option(icz_aoa_t* h, const char* name, int32_t value) {
    ICZ_REQUIRE(h && name, "icz_aoa_set_option: null argument");
    Aoa* n = reinterpret_cast<Aoa*>(h);
    if (strcmp(name, "graphs") == 0) { n->use_graphs = value != 0; return ICZ_OK; }
    if (strcmp(name, "train_refiner") == 0) {
        ICZ_REQUIRE(value == 0 || value == 1, "icz_aoa_set_option: train_refiner takes 0 or 1, got %d", (int)value);
        return n->set_train_refiner(value != 0);
    }
    const bool eo = strcmp(name, "early_out") == 0, rp = strcmp(name, "refine_pair") == 0, mm = strcmp(name, "mha_mfma") == 0;
    if (eo || rp || mm) {
        ICZ_CHECK_HIP(hipDeviceSynchronize());      // a replay of a graph about to be destroyed may still be in flight
        n->gc.clear();
        if (eo) n->early_out = value != 0;
        if (rp) n->pair_refine = value != 0;
        if (mm) n->mha_mfma = value != 0;
        return ICZ_OK;
    }
    set_error("icz_aoa_set_option: unknown option '%s'", name);
    return ICZ_ERR_INVALID;
}
int icz_aoa_refresh_weights(icz_aoa_t* h, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Aoa*>(h)->refresh((hipStream_t)stream);
}
int icz_aoa_refine(icz_aoa_t* h, const float* feats, int32_t B, float* refined_out, void* stream) {
    ICZ_REQUIRE(h && feats && refined_out, "icz_aoa_refine: null argument");
    Aoa* n = reinterpret_cast<Aoa*>(h);
    ICZ_REQUIRE(B > 0 && B <= n->dims.max_rows, "icz_aoa_refine: B out of range");
    ICZ_REQUIRE(n->fresh, "aoa: call icz_aoa_refresh_weights after binding/updating parameters");
    n->use_bank(0);
    hipStream_t st = (hipStream_t)stream;
    ICZ_TRY(n->refine(feats, B, false, st));
    const size_t bytes = sizeof(float) * (size_t)B * n->cur_R * n->dims.Hd;
    if (!n->lens) {
        ICZ_CHECK_HIP(hipMemcpyAsync(refined_out, n->refined, bytes, hipMemcpyDeviceToDevice, st));
    } else {         // packed rows back to [B, regions, Hd]; the padding rows (never computed) are zero
        ICZ_CHECK_HIP(hipMemsetAsync(refined_out, 0, bytes, st));
        const size_t rows = n->region_row_count(B), n4 = rows * (n->dims.Hd / 4);
        hipLaunchKernelGGL(aoa_unpack_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float*)n->refined,
                           (const int32_t*)n->rowmap, refined_out, rows, n->dims.Hd);
    }
    return ICZ_OK;
}
int icz_aoa_set_regions(icz_aoa_t* h, int32_t regions, const int32_t* counts_dev, const int32_t* counts_host, int32_t n_img) {
    ICZ_REQUIRE(h, "null handle");
    Aoa* n = reinterpret_cast<Aoa*>(h);
    ICZ_REQUIRE(regions >= 1 && regions <= n->dims.R, "icz_aoa_set_regions: %d regions outside 1..%d (the handle's capacity)", regions, n->dims.R);
    ICZ_REQUIRE((counts_dev == nullptr) == (counts_host == nullptr), "icz_aoa_set_regions: pass the counts on both sides or on neither");
    if (counts_host) {
        ICZ_REQUIRE(n_img >= 1 && n_img <= n->dims.max_rows, "icz_aoa_set_regions: %d images out of range", n_img);
        for (int i = 0; i < n_img; ++i)
            ICZ_REQUIRE(counts_host[i] >= 1 && counts_host[i] <= regions, "icz_aoa_set_regions: image %d has %d regions (1..%d)", i, counts_host[i], regions);
    }
    n->cur_R = regions; n->lens = counts_dev; n->lens_n = counts_dev ? n_img : 0;
    n->cur_total = 0;
    for (int i = 0; counts_host && i < n_img; ++i) n->cur_total += counts_host[i];
    n->mode = 0;
    return ICZ_OK;
}
// ------------------------------------------------------------------------------------------------
// Test entries of the forward AoA kernels (include/icz.h): each checks on the host what its kernel needs, fills the kernel's arguments
// the way the handle does and goes through the handle's launch helper, nothing more.
int icz_test_aoa_layer_norm(int32_t geometry, const float* x, const float* gain, const float* bias, float* y, int32_t rows, int32_t n, float* stats,
                            const int32_t* live, void* stream) {
    const char* who = "icz_test_aoa_layer_norm";
    ICZ_REQUIRE(x && gain && bias && y, "%s: null argument", who);
    ICZ_REQUIRE(geometry == 0 || geometry == 1, "%s: geometry %d (0: four rows per workgroup, 1: one wave per workgroup)", who, geometry);
    ICZ_REQUIRE(rows >= 1 && n >= 2, "%s: %d rows of %d columns (the unbiased std needs two)", who, rows, n);
    if (n <= 2048 && n % 4 == 0)       // the register path reads and writes 16 bytes at a time
        ICZ_REQUIRE(aoa_al16(x) && aoa_al16(gain) && aoa_al16(bias) && aoa_al16(y), "%s: x, gain, bias and y must be 16-byte aligned", who);
    aoa_launch_layer_norm(geometry, x, gain, bias, y, rows, n, stats, live, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_aoa_self_attn_route_for(int32_t R, int32_t Hd, int32_t NH, int32_t mha_mfma, int32_t* qc_out, size_t* lds_out) {
    const char* who = "icz_aoa_self_attn_route_for";
    ICZ_TRY(aoa_test_heads(who, R, Hd, NH));
    const int d = Hd / NH, qc = aoa_self_qc(R, d), route = aoa_self_route(R, Hd, NH, mha_mfma != 0);
    ICZ_REQUIRE(qc >= 1, "%s: K and V head tiles of %d regions x %d columns do not fit the LDS budget", who, R, d);
    if (qc_out) *qc_out = qc;
    if (lds_out) *lds_out = route == 2 ? AOA_SELF_MFMA_LDS : aoa_self_lds(R, d, qc);
    return route;
}

int icz_test_aoa_self_attn(int32_t route, const float* qkv, float* o, int32_t n_img, int32_t R, int32_t Hd, int32_t NH, const int32_t* counts,
                           int32_t qc, const icz_test_dropp* dropp, int32_t* route_out, int32_t* qc_out, void* stream) {
    const char* who = "icz_test_aoa_self_attn";
    ICZ_REQUIRE(qkv && o && n_img >= 1, "%s: null argument or no image", who);
    ICZ_TRY(aoa_test_heads(who, R, Hd, NH));
    ICZ_REQUIRE(route >= 0 && route <= 2, "%s: route %d (0: the handle's choice, 1: mha_self_kernel, 2: mha_self_mfma_kernel)", who, route);
    ICZ_REQUIRE(aoa_al16(qkv) && aoa_al16(o), "%s: qkv and o must be 16-byte aligned", who);
    const int d = Hd / NH;
    const int r = route ? route : aoa_self_route(R, Hd, NH, true);
    ICZ_REQUIRE(r != 2 || aoa_self_route(R, Hd, NH, true) == 2, "%s: mha_self_mfma_kernel takes at most 64 regions and heads of a multiple of 64 columns "
                "(%d regions, %d columns)", who, R, d);
    int q = qc;
    if (q == 0) q = aoa_self_qc(R, d);
    else ICZ_REQUIRE(q == R || (q >= 4 && q % 4 == 0 && q < R), "%s: a forced chunk of %d query rows (a multiple of 4 up to %d regions)", who, q, R);
    ICZ_REQUIRE(q >= 1 && aoa_self_lds(R, d, q) <= AOA_LDS_BUDGET, "%s: %d regions x %d columns in chunks of %d rows need %zu bytes of LDS (limit %zu)", who,
                R, d, q, aoa_self_lds(R, d, q), AOA_LDS_BUDGET);
    DropP dp;
    ICZ_TRY(aoa_test_dropp(who, dropp, &dp));
    if (route_out) *route_out = r;
    if (qc_out) *qc_out = q;
    const size_t lds = aoa_self_lds(R, d, q);
    if (r == 1) ICZ_TRY(aoa_self_attn_optin(lds));
    AoaTestRegions reg;
    RegionRows rr;
    ICZ_TRY(reg.build(who, counts, n_img, R, (hipStream_t)stream, &rr));
    aoa_launch_mha_self(n_img, R, Hd, NH, r == 2, q, lds, rr, qkv, o, dp, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_aoa_dec_attn(const float* Qp, int32_t qns, int64_t q_stride, const float* q_bias, float* Qp_store, const float* Kd, const float* Vd,
                          const int32_t* img_of_row, float* xatt, float* P_out, float* Pd_out, int32_t rows, int32_t n_img, int32_t R, int32_t Hd,
                          int32_t NH, const int32_t* counts, const icz_test_dropp* dropp, const int32_t* live, void* stream) {
    const char* who = "icz_test_aoa_dec_attn";
    ICZ_REQUIRE(Qp && Kd && Vd && xatt && rows >= 1 && n_img >= 1, "%s: null argument, no row or no image", who);
    ICZ_TRY(aoa_test_heads(who, R, Hd, NH));
    ICZ_REQUIRE(aoa_al16(Kd) && aoa_al16(Vd), "%s: Kd and Vd must be 16-byte aligned", who);
    ICZ_REQUIRE(qns >= 1 && qns <= 16, "%s: %d slabs of the query projection (1..16)", who, qns);
    ICZ_REQUIRE(qns == 1 || (q_bias && Qp_store && q_stride >= (int64_t)rows * Hd), "%s: %d slabs need q_bias, Qp_store and a stride of at least rows * Hd "
                "(%lld)", who, qns, (long long)q_stride);
    ICZ_REQUIRE(img_of_row || rows <= n_img, "%s: %d rows over %d images need img_of_row", who, rows, n_img);
    const size_t lds = aoa_dec_attn_lds(R, Hd / NH);
    ICZ_REQUIRE(lds <= AOA_LDS_BUDGET, "%s: K and V head tiles of %d regions x %d columns need %zu bytes of LDS (limit %zu)", who, R, Hd / NH, lds,
                AOA_LDS_BUDGET);
    DropP dp;
    ICZ_TRY(aoa_test_dropp(who, dropp, &dp));
    if (img_of_row) {
        std::vector<int32_t> ior;
        ICZ_TRY(aoa_test_read_i32(img_of_row, rows, &ior));
        for (int i = 0; i < rows; ++i) ICZ_REQUIRE(ior[i] >= 0 && ior[i] < n_img, "%s: row %d decodes image %d of %d", who, i, ior[i], n_img);
    }
    ICZ_TRY(aoa_dec_attn_optin(lds));
    AoaTestRegions reg;
    RegionRows rr;
    ICZ_TRY(reg.build(who, counts, n_img, R, (hipStream_t)stream, &rr));
    aoa_launch_dec_attn(Qp, qns, (size_t)q_stride, q_bias, Qp_store, Kd, Vd, img_of_row, xatt, P_out, Pd_out, rows, R, Hd, NH, rr, dp, live,
                        (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_aoa_greedy(icz_aoa_t* h, const float* feats, int32_t B, int32_t max_len, int64_t* ids_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Aoa*>(h)->greedy(feats, B, max_len, ids_out, (hipStream_t)stream);
}
}  // extern "C"
