// AoADetection captioner, option "train_refiner": the backward pass through aoa_refine.* and img_feats_porjection.* behind Aoa::bptt
// (beyond the reference, which optimises the decoder only, AoA_Model.py:669-674).
//
// Memory route: a training-mode refiner pass keeps the input of each of the six layers and of the final norm (xs[0..6], region rows x Hd
// each); the backward pass walks the layers 5 -> 0 and RECOMPUTES a layer's forward (LayerNorm, fused Q/K/V projection, self-attention,
// dropout of [o | ln], AoA linear) into the bank's scratch buffers in front of its backward step.  The dropout draws come back from Philox
// or the explicit mask pointers with the indices the forward pass used, as the decoder's backward regenerates its own.
// Everything runs on the caller's stream behind the joins of bptt: every workspace here has one writer at a time.
#include "aoa_impl.h"
#include "aoa_test_support.h"

namespace icz {

int Aoa::set_train_refiner(bool on) {
    if (on == train_refiner) return ICZ_OK;
    // the training buffers change their set and the captured graphs their launches: both are dropped and come back on the next call
    ICZ_TRY(mem.release_training(&gc));
    ICZ_CHECK_HIP(hipDeviceSynchronize());
    gc.clear();
    tcap_B = tcap_T = tcap_I = 0;
    drop_loss_buffers();
    drop_refiner_buffers();
    train_refiner = on;
    mode = 0;
    return ICZ_OK;
}

// called inside ensure_train's TrainingScope: released with the other training buffers.  B = images, TB = steps x decoder rows
int Aoa::alloc_refiner_train(size_t B, size_t TB) {
    const size_t RR = B * dims.R, Hd = dims.Hd;
    for (float*& p : xs) ICZ_TRY(alloc((void**)&p, sizeof(float) * RR * Hd));
    float** one[] = {&rdx[0], &rdx[1], &rdo, &rdln, &rdq, &rprod};
    for (float** p : one) ICZ_TRY(alloc((void**)p, sizeof(float) * RR * Hd));
    ICZ_TRY(alloc((void**)&rdz, sizeof(float) * RR * 2 * Hd));
    ICZ_TRY(alloc((void**)&rdqkv, sizeof(float) * RR * 3 * Hd));
    ICZ_TRY(alloc((void**)&rdmean, sizeof(float) * B * Hd));
    // split-K slabs of the dgrad products: two slabs of the widest one (rows x 2Hd) -- or one of d u over all (t, row), which the K rows per
    // image of a multi-sample rollout can make the larger -- and the small-launch reserve of the decoder's slabs
    const size_t widest = 2 * RR * 2 * Hd > TB * Hd ? 2 * RR * 2 * Hd : TB * Hd;
    rslab_floats = (size_t)TARGET_WGS * 4096 * 2 + widest;
    ICZ_TRY(alloc((void**)&rslab, sizeof(float) * rslab_floats));
    // (a narrower batch may fit where the handle's capacity does not: refiner_backward_check decides per call)
    return aoa_self_attn_bwd_optin(aoa_self_bwd_lds(dims.R, dims.Hd / dims.NH));
}

int Aoa::refiner_backward_check(const icz_aoa_params& G) const {
    static const char* const block_names[10] = {"linear_Q.weight", "linear_Q.bias", "linear_K.weight", "linear_K.bias", "linear_V.weight",
                                                "linear_V.bias", "aoa_module.0.weight", "aoa_module.0.bias", "norm.gain", "norm.bias"};
    ICZ_REQUIRE(G.proj_w && G.proj_b, "aoa: option train_refiner is on and the gradient buffer of img_feats_porjection.0.%s is null",
                G.proj_w ? "bias" : "weight");
    for (int l = 0; l < NL; ++l) {
        const float* const* slot = reinterpret_cast<const float* const*>(&G.layer[l]);
        for (int i = 0; i < 10; ++i)
            ICZ_REQUIRE(slot[i], "aoa: option train_refiner is on and the gradient buffer of aoa_refine.aoa_layers.%d %s is null", l, block_names[i]);
    }
    ICZ_REQUIRE(G.ref_ln_g && G.ref_ln_b, "aoa: option train_refiner is on and the gradient buffer of aoa_refine.norm.%s is null",
                G.ref_ln_g ? "bias" : "gain");
    ICZ_REQUIRE(xs_valid && xs[0] && ref_feats, "aoa: option train_refiner needs a training-mode forward pass made while it was on "
                "(an evaluation-mode pass stores nothing)");
    const size_t lds = sizeof(float) * mha_self_bwd_lds_floats(cur_R, dims.Hd / dims.NH);
    ICZ_REQUIRE(lds <= LDS_BUDGET, "aoa: train_refiner: the self-attention backward needs %zu bytes of LDS for %d regions and heads of %d "
                "columns (limit %zu)", lds, cur_R, dims.Hd / dims.NH, LDS_BUDGET);
    return ICZ_OK;
}

namespace {

// slabs [ns][M][N] = A[M,K] . B[K,N] into `slab` (capacity `cap` floats).  The split shrinks to fit on the small branch too (the
// refiner's slab buffer is sized for its widest products only), so here the capacity check of gemm_slabs can never fail.
int rnn(const float* A, int lda, int M, int K, const float* Bm, int ldb, int N, float* slab, size_t cap, int* ns_out, hipStream_t st) {
    return Aoa::nn(A, lda, M, K, Bm, ldb, N, slab, cap, ns_out, split_backward(Aoa::TARGET_WGS, true), st);
}

}  // namespace

void aoa_launch_ln_bwd_dense(const float* dq_a, int ns_a, const float* dq_b, int rows, const float* x, const float* gain, const float* res,
                             float* dq_tot, float* prod, float* dx, int n, hipStream_t st) {
    hipLaunchKernelGGL(aoa_ln_bwd_dense_kernel, dim3(rows), dim3(256), 0, st, dq_a, ns_a, dq_b, rows, x, gain, res, dq_tot, prod, dx, n);
}
int aoa_self_attn_bwd_optin(size_t lds) {
    static size_t raised[AOA_LDS_LIMIT_DEVICES] = {};
    return aoa_raise_lds_limit(reinterpret_cast<const void*>(mha_self_bwd_kernel), lds < AOA_LDS_BUDGET ? lds : AOA_LDS_BUDGET, raised);
}
void aoa_launch_mha_self_bwd(const float* qkv, const float* dO, float* dqkv, int n_img, int R, int Hd, int NH, const RegionRows& rr, const DropP& dp,
                             hipStream_t st) {
    hipLaunchKernelGGL(mha_self_bwd_kernel, dim3(n_img, NH), dim3(256), aoa_self_bwd_lds(R, Hd / NH), st, qkv, dO, dqkv, R, Hd, NH, rr, dp);
}

int Aoa::refiner_backward(const icz_aoa_params& G, hipStream_t st) {
    use_bank(1);
    // B = images; behind the multi-sample rollout (sample_n) the decoder ran cur_K rows per image: only d meanf tells rows from images
    const int K = cur_K, B = cur_B / K, T = cur_T, Hd = dims.Hd, E = dims.E, NH = dims.NH, R = cur_R, D = dims.D, TB = T * cur_B;
    const int rows = (int)region_row_count(B);
    const RegionRows rr = region_rows();
    const size_t nel = (size_t)rows * Hd;
    const unsigned eb = (unsigned)((nel + 255) / 256);
    const bool train = cur_train;
    // ---- 1. d refined = dKd k_w + dVd v_w + d meanf / count;  d meanf[img] = sum over the image's rows and t of du_t[row], du = d gates . W_ih[:, E:]
    //         over all (t, row) rows
    //         (the rows of steps that never ran and rows b >= rows_t[t] hold zero d gates: bptt zeroed them in front of its loop)
    int nsu = 1, nsk = 1, nsv = 1;
    ICZ_TRY(rnn(dG, 4 * Hd, TB, 4 * Hd, P.lstm_w_ih + E, E + Hd, Hd, rslab, rslab_floats, &nsu, st));
    hipLaunchKernelGGL(aoa_dmean_kernel, dim3((unsigned)(((size_t)B * Hd + 255) / 256)), dim3(256), 0, st, rslab, nsu, T, cur_B, Hd, rdmean, K);
    const size_t half = rslab_floats / 2;
    ICZ_TRY(rnn(dKd, Hd, rows, Hd, P.dec.k_w, Hd, Hd, rslab, half, &nsk, st));
    ICZ_TRY(rnn(dVd, Hd, rows, Hd, P.dec.v_w, Hd, Hd, rslab + half, half, &nsv, st));
    hipLaunchKernelGGL(aoa_dref_kernel, dim3(cdiv(Hd, 256), B), dim3(256), 0, st, rslab, nsk, rslab + half, nsv, nel, rdmean, rdq, Hd, rr);
    // ---- 2. aoa_refine.norm
    int c = 0;
    aoa_launch_ln_bwd_dense(nullptr, 0, rdq, rows, xs[NL], P.ref_ln_g, nullptr, nullptr, rprod, rdx[c], Hd, st);
    ICZ_TRY(launch_colsum(rprod, rows, Hd, Hd, G.ref_ln_g, st));
    ICZ_TRY(launch_colsum(rdq, rows, Hd, Hd, G.ref_ln_b, st));
    // ---- 3. the layers, last to first
    for (int l = NL - 1; l >= 0; --l) {
        const icz_aoa_block& b = P.layer[l];
        const icz_aoa_block& gb = G.layer[l];
        const DropP d_att = dropp(train, rng.ref_att_mask, (size_t)l * B * NH * R * R, AOA_RNG_REF_ATT, l, 0.1f);
        const DropP d_aoa = dropp(train, rng.ref_aoa_mask, (size_t)l * B * R * 2 * Hd, AOA_RNG_REF_AOA, l, 0.3f);
        const DropP d_sc = dropp(train, rng.ref_sc_mask, (size_t)l * B * R * Hd, AOA_RNG_REF_SC, l, 0.1f);
        // forward of layer l from its stored input (Aoa::refine's launches)
        aoa_launch_layer_norm(0, xs[l], b.ln_g, b.ln_b, ln, rows, Hd, nullptr, nullptr, st);
        ICZ_TRY(lin(ln, rows, Hd, w_qkv[l], b_qkv[l], 3 * Hd, qkv, st));
        mha_self_layer(B, l, train, st);
        const float *xo = o, *xn = ln;
        if (train) {
            hipLaunchKernelGGL(drop_concat_kernel, dim3(eb), dim3(256), 0, st, (const float*)o, (const float*)ln, od, nd, (size_t)rows, Hd, rr, d_aoa);
            xo = od; xn = nd;
        }
        ICZ_TRY(linear(gemm_args({{xo, b.aoa_w, Hd, 2 * Hd, Hd}, {xn, b.aoa_w + Hd, Hd, 2 * Hd, Hd}}, rows, 2 * Hd, z, 2 * Hd), b.aoa_b, st));
        // GLU + residual: rdx[c] = d x_{l+1} stays the residual branch's gradient
        hipLaunchKernelGGL(glu_residual_bwd_kernel, dim3(eb), dim3(256), 0, st, (const float*)rdx[c], (const float*)z, rdz, (size_t)rows, Hd, rr, d_sc);
        // AoA linear: weight gradient against the dropped inputs (two column groups of aoa_w), bias, input gradient
        const GemmColGroup groups[2] = {{xo, Hd, Hd, gb.aoa_w, 2 * Hd}, {xn, Hd, Hd, gb.aoa_w + Hd, 2 * Hd}};
        ICZ_TRY(gemm_tn_groups(rdz, 2 * Hd, 2 * Hd, rows, groups, 2, nullptr, 0, nullptr, st));
        ICZ_TRY(launch_colsum(rdz, rows, 2 * Hd, 2 * Hd, gb.aoa_b, st));
        int ns = 1;
        ICZ_TRY(rnn(rdz, 2 * Hd, rows, 2 * Hd, b.aoa_w, 2 * Hd, 2 * Hd, rslab, rslab_floats, &ns, st));
        hipLaunchKernelGGL(drop_concat_bwd_kernel, dim3(eb), dim3(256), 0, st, (const float*)rslab, ns, rdo, rdln, (size_t)rows, Hd, rr, d_aoa);
        // self-attention
        aoa_launch_mha_self_bwd(qkv, rdo, rdqkv, B, R, Hd, NH, rr, d_att, st);
        // fused Q/K/V projection: the three weight gradients go to the separate reference tensors
        float* const gw[3] = {gb.q_w, gb.k_w, gb.v_w};
        float* const gbias[3] = {gb.q_b, gb.k_b, gb.v_b};
        for (int w = 0; w < 3; ++w) {
            ICZ_TRY(gemm_tn(rdqkv + (size_t)w * Hd, 3 * Hd, Hd, ln, Hd, Hd, rows, gw[w], Hd, 0, nullptr, st));
            ICZ_TRY(launch_colsum(rdqkv + (size_t)w * Hd, rows, Hd, 3 * Hd, gbias[w], st));
        }
        ICZ_TRY(rnn(rdqkv, 3 * Hd, rows, 3 * Hd, w_qkv[l], Hd, Hd, rslab, rslab_floats, &ns, st));
        // LayerNorm (its output fed the projection and the [o | ln] concatenation) + the residual
        aoa_launch_ln_bwd_dense(rslab, ns, rdln, rows, xs[l], b.ln_g, rdx[c], rdq, rprod, rdx[c ^ 1], Hd, st);
        ICZ_TRY(launch_colsum(rprod, rows, Hd, Hd, gb.ln_g, st));
        ICZ_TRY(launch_colsum(rdq, rows, Hd, Hd, gb.ln_b, st));
        c ^= 1;
    }
    // ---- 4. img_feats_porjection: ReLU + dropout backward from the stored output, weight gradient over the region rows
    hipLaunchKernelGGL(relu_drop_bwd_kernel, dim3(eb), dim3(256), 0, st, (const float*)xs[0], (const float*)rdx[c], rdo, nel, train ? 2.0f : 1.0f);
    ICZ_TRY(gemm_tn(rdo, Hd, Hd, ref_feats, D, D, rows, G.proj_w, D, 0, nullptr, st));
    ICZ_TRY(launch_colsum(rdo, rows, Hd, Hd, G.proj_b, st));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // namespace icz

// ================================================================================================
using namespace icz;
extern "C" {

// Test entry of mha_self_bwd_kernel (include/icz.h): host checks (the library's refusal above the LDS budget), the handle's opt-in and launch.
int icz_test_aoa_self_attn_bwd(const float* qkv, const float* dO, float* dqkv, int32_t n_img, int32_t R, int32_t Hd, int32_t NH, const int32_t* counts,
                               const icz_test_dropp* dropp, void* stream) {
    const char* who = "icz_test_aoa_self_attn_bwd";
    ICZ_REQUIRE(qkv && dO && dqkv && n_img >= 1, "%s: null argument or no image", who);
    ICZ_TRY(aoa_test_heads(who, R, Hd, NH));
    ICZ_REQUIRE(aoa_al16(qkv) && aoa_al16(dO), "%s: qkv and dO must be 16-byte aligned", who);
    const size_t lds = aoa_self_bwd_lds(R, Hd / NH);
    ICZ_REQUIRE(lds <= AOA_LDS_BUDGET, "aoa: train_refiner: the self-attention backward needs %zu bytes of LDS for %d regions and heads of %d "
                "columns (limit %zu)", lds, R, Hd / NH, AOA_LDS_BUDGET);
    DropP dp;
    ICZ_TRY(aoa_test_dropp(who, dropp, &dp));
    ICZ_TRY(aoa_self_attn_bwd_optin(lds));
    AoaTestRegions reg;
    RegionRows rr;
    ICZ_TRY(reg.build(who, counts, n_img, R, (hipStream_t)stream, &rr));
    aoa_launch_mha_self_bwd(qkv, dO, dqkv, n_img, R, Hd, NH, rr, dp, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
