// Internal declarations of the BUTD decoder handle.
#pragma once
#include <vector>
#include <stdint.h>

#include "butd_kernels.h"
#include "decoder_core.h"
#include "rng.h"

namespace icz {

// Inputs / outputs of one decoder step.  Null outputs fall back to the handle's scratch buffers.
struct StepIO {
    int rows;
    const float* feats;              // [n_img, R, D]
    const int32_t* img_of_row;       // beam search: image of each decoder row; null = identity
    int rows_per_img;                // beam search: > 1 = the rows img * rows_per_img + b belong to image img (img_of_row agrees)
    const int64_t* it;               // [rows] input token ids
    bool emb_ready;                  // the embedding of `it` is already in the emb buffer (skip embed_kernel)
    const float *h1_in, *c1_in, *h2_in, *c2_in;
    float *h1_out, *c1_out, *h2_out, *c2_out;
    float* emb_out;                  // [rows,E]
    float* gates_td_out;             // [rows,4H] activated gates (backward)
    float* gates_lm_out;
    float* dec_ctx_out;              // [rows,A]
    float* alpha_out;                // [rows,R]
    float* alpha_out2; int alpha2_stride;   // second copy laid out [rows, T, R] (caller's alphas tensor)
    float* ctx_out;                  // [rows,D]
    float* h2drop_out;               // [rows,H]
    float* logits_out;               // [rows,V]
    int logits_ld;                   // row stride of logits_out (0 = V)
    int* pred_nsplit;                // non-null: the caller's consumer of the logits can sum split-K slabs (greedy_select_kernel,
                                     // sample_select_kernel): step() may leave the predict GEMM's slabs [ns][rows][Vp] in the
                                     // chain's workspace instead of finished logits and reports ns here (1 = logits_out is final)
    float* ws_alt;                   // split-K slab workspace / attention scores of this chain (null = the handle's):
    float* scores_alt;               // two decode chains running concurrently must not share them
    DropCfg drop_emb, drop_att, drop_out;
    bool skip_predict;               // teacher-forced XE forward: the vocabulary projection of ALL time steps is one GEMM after the loop
    const int* live;                 // sampled rollout: the count of unfinished rows after the previous step; 0 = every kernel of this step
                                     // returns at entry (step_dead, icz_common.h: the reference's break, BUTD_Model.py:233)
};

// Activations kept by a training-mode forward (slot t = time step, slot stride = B rows) and backward scratch.
struct TrainBuf {
    int B = 0, T = 0;
    int64_t* tok = nullptr;                                   // [(T+1), B] input token of each step
    float *emb = nullptr, *h1 = nullptr, *c1 = nullptr, *h2 = nullptr, *c2 = nullptr;   // states: [(T+1), B, H], slot 0 = zeros
    float *gtd = nullptr, *glm = nullptr, *dec = nullptr, *alpha = nullptr, *ctx = nullptr, *h2d = nullptr, *logit = nullptr;
    int* nany = nullptr;                                      // merged chain: unfinished sampled rows + greedy rows that have not ended, per step
    int32_t* img2 = nullptr;                                  // merged chain: image of each decoder row (row r of 2 B -> image r mod B)
    int32_t* imgk = nullptr;                                  // multi-sample rollout: image of each decoder row (row r of B K -> image r / K)
    float* dEncImg = nullptr;                                 // multi-sample backward: d enc_ctx folded onto the images [n_img, R, A]
    int32_t* lenk = nullptr;                                  // grouped XE forward: steps of each decoder row (row r of B K, in any length order)
    float *dGtd = nullptr, *dGlm = nullptr, *dDec = nullptr, *dEmb = nullptr, *dH2d = nullptr, *dEnc = nullptr;
    float *dwaff = nullptr, *dalpha = nullptr, *dS = nullptr, *dGsum = nullptr;
    float *dc1[2] = {nullptr, nullptr}, *dc2[2] = {nullptr, nullptr};
    float* X[4] = {nullptr, nullptr, nullptr, nullptr}; size_t xfloats = 0;
    float *dWp = nullptr, *dWenc = nullptr, *dWdec = nullptr, *dWaff = nullptr, *scalars = nullptr;
    // split-K slabs of the weight gradients that take gemm_tn_split (Butd::wgrad), one region per stream that can be inside bptt() at the
    // same time: [0] the stream bptt() was called on, [1] the low-priority side stream (predict branch, then the attention tail)
    float* wslab[2] = {nullptr, nullptr}; size_t wslab_floats[2] = {0, 0};
};

struct Butd : CaptionHead, DecodeMember {
    static constexpr int TARGET_WGS = 512;   // ~2 workgroups per CU on 256 CUs
    static constexpr int ATT_PARTS = 4;
    static constexpr int STEP_WGS = 256;     // skinny decoder-step GEMMs: split-K for ~1 workgroup per CU
    icz_butd_dims dims;
    icz_butd_params P;
    bool bound = false, fresh = false;
    DeviceBuffers mem;                   // training list: TrainBuf and the loss head, re-allocated when a batch needs more rows / steps

    // weight-normed weights (w = g v / ||v||) and the row norms ||v||
    float *w_enc = nullptr, *w_dec = nullptr, *w_aff = nullptr, *w_pred = nullptr;
    float *n_enc = nullptr, *n_dec = nullptr, *n_aff = nullptr, *n_pred = nullptr;
    // per-image hoisted tensors
    float *mean = nullptr, *premean = nullptr, *enc_ctx = nullptr;
    // recurrent state (double buffered) and per-step scratch
    float *h1[2], *c1[2], *h2[2], *c2[2];
    float *emb = nullptr, *ctx = nullptr, *scores = nullptr, *alpha = nullptr, *h2drop = nullptr, *logits = nullptr;
    int64_t* it = nullptr;
    float* amax_val = nullptr; int* amax_idx = nullptr;
    float* ws = nullptr;
    size_t ws_floats = 0;
    // Transposed copies of the LSTM weights: the per-step dgrad products of BPTT, dx = dy W, run as NT products on W^T through the
    // resident-activation kernel (weights streamed once, split-precision MFMA) instead of the fp32 NN kernel.  Allocated with the
    // first training buffers where the sizes fit that kernel, refreshed once per optimiser step (refresh / first backward after it).
    float *wt_lm_ih = nullptr, *wt_lm_hh = nullptr, *wt_td_ih_h2 = nullptr, *wt_td_hh = nullptr;
    bool wt_fresh = false;
    bool wt_possible() const;
    int refresh_transposes(hipStream_t st);

    int alloc(void** p, size_t bytes) { return mem.alloc(p, bytes); }
    int init(const icz_butd_dims& d, int r_max = 64);      // r_max: 64 through icz_butd_create, ATT_MAX_R through icz_butd_create_regions
    int refresh(hipStream_t st);
    int gemm_nt(GemmArgs& g, const float* bias, hipStream_t st);
    int prologue(const float* feats, int n_img, hipStream_t st);
    int step(const StepIO& s, hipStream_t st);
    int zero_state(int rows, int which, hipStream_t st);
    int greedy(const float* feats, int B, int max_len, int64_t* ids_out, float* alphas_out, hipStream_t st);

    // regions per image of the current batch (icz_butd_set_regions): row stride cur_R <= dims.R of feats and of every per-image
    // buffer and, for the 'adaptive' bottom-up features (10..100 boxes), the valid count per image (device, caller-owned; null = all
    // cur_R).  adaptive(): the launches take the <true> instances of the attention kernels (butd_kernels.h) -- with no counts and
    // cur_R <= 64 every launch is the fixed-set instance.
    int cur_R = 0, cnt_n = 0;
    const int32_t* cnt = nullptr;
    bool adaptive() const { return cnt != nullptr || cur_R > 64; }
    int check_counts(int n_img) const {
        ICZ_REQUIRE(!cnt || n_img <= cnt_n, "butd: region counts were set for %d images, the batch has %d (icz_butd_set_regions)", cnt_n, n_img);
        return ICZ_OK;
    }

    GraphCache gc{24};                   // keys end with opt_bits(); bypassed unless graphs_on()
    bool use_graphs = false;
    bool graphs_on() const { return use_graphs && !cnt; }       // calls made while counts are set stay eager (as AoA's do)
    bool concurrent = true;      // run independent chains on side streams (off: one stream, for per-kernel timing)
    uintptr_t opt_bits() const {         // the options that change the captured launch sequence, and the row stride of the region tensors
        return (concurrent ? 1 : 0) + (early_out ? 2 : 0) + 4 * merge_small + (small_nt ? 256 : 0) + (group_att ? 512 : 0) + (fused_dh1 ? 1024 : 0) + ((uintptr_t)cur_R << 16);
    }
    int greedy_impl(const float* feats, int B, int max_len, int64_t* ids_out, float* alphas_out, hipStream_t st);
    int sample_impl(const float* feats, int B, int T, int64_t* seq_out, float* logp_out, hipStream_t st);
    int greedy_chain(const float* feats, int B, int max_len, int64_t* ids_out, float* alphas_out, hipStream_t st, bool scst = false);
    int sample_chain(const float* feats, int B, int T, int64_t* seq_out, float* logp_out, hipStream_t st, int row0 = 0, int64_t* ids_out = nullptr);
    int rollouts(const float* feats, int B, int T, const icz_rng* r, int64_t* ids_out, int64_t* seq_out, float* logp_out, hipStream_t st);
    int rollouts_impl(const float* feats, int B, int T, int64_t* ids_out, int64_t* seq_out, float* logp_out, hipStream_t st);
    SideStream side;                     // the greedy chain of the SCST rollout pair
    SideStream low;                      // lowest priority, for work overlapped with the BPTT chain; its second event pair: the attention
                                         // block's tail beside the LSTM weight gradients (bptt)
    icz_grad_ready_cb grad_cb = nullptr; void* grad_cb_user = nullptr;   // DP overlap hook (icz_butd_set_grad_callback)
    int merge_small = 8;                 // option "merge_small" = n: SCST rollouts of <= n images (n <= 32) run as ONE chain of 2 B decoder rows
                                         // (sample_chain with row0 = B); 0 = never.  Default 8: measured round 5 (EXPERIMENTS.md), the
                                         // merged chain saves 0.2 ms of rollouts at every size but costs the backward pass 0.06 / 0.15 /
                                         // 0.37 ms at 8 / 16 / 32 images (its batched GEMMs then run over 2 B rows per step)
    int cur_rows = 0, cur_row0 = 0;      // rows per step slot of the stored forward pass and the offset of the rows the backward pass works on
                                         // (a merged chain stores 2 B rows per step, the sampled rollout's are rows B .. 2 B - 1)
    bool small_nt = true;                // option "small_nt": BPTT steps of <= 32 rows take their dgrad products on the transposed weight copies (fp32 NT kernel)
    bool fused_dh1 = true;               // option "fused_dh1": BPTT steps of <= 64 rows at widths lstm_bwd_dh1_fused_takes accepts form X2 = d dec . w_dec
                                         // inside the TD-LSTM backward launch (six launches per step); 0 = the product and the pointwise
                                         // kernel as two launches (seven).  The same bits either way
    // multi-sample SCST rollout (sample_n, beyond the reference): K sampled rows per image, row = img * K + k, sharing the image's
    // hoisted tensors.  cur_K (CaptionHead) = rows per image of the stored rollout, cur_nimg = its image count.
    // xe_forward_n stores its teacher-forced forward pass in the same layout (mode 2 with cur_K > 1: xe_grouped()).
    int cur_nimg = 0;
    bool group_att = false;              // option "group_att": 1 = sample_n's attention (forward scores / context, backward d enc_ctx) runs on
                                         // the grouped kernels (each image's features / enc_ctx read once for its K rows); 0 (default) = the
                                         // per-row kernels through img_of_row.  Measured (tools/perf_scst_n.py): the
                                         // grouped route is slower, 16.3 against 15.9 ms at 64 images x 5 and 5.65 against 4.94 ms at 16 x 4
                                         // (fewer, longer workgroups; the features fit the Infinity Cache either way)

    // the decoder seams (DecodeMember, decoder_core.h): beam search (beam.hip), the sampling decode and the ensemble run on them
    const float* seam_feats = nullptr;   // the features of the last prologue(feats, n_img, k, ...): the steps that follow attend over them
    int vocab() const override { return dims.V; }
    int row_capacity() const override { return dims.max_rows; }
    bool refreshed() const override { return fresh; }
    bool compact_step() const override { return true; }
    EmbSlot emb_slot() const override { return {P.embed_weight, emb, dims.E, 1}; }
    DeviceBuffers& buffers() override { return mem; }
    int prologue(const float* feats, int n_img, int k, const int32_t* img_of_row, hipStream_t st) override;
    int step(int rows, const int64_t* it, const int32_t* img_of_row, int rows_per_img, int cur, bool slabs, LogitsView* out,
             hipStream_t st) override;
    void gather(const int32_t* src_row, int rows, int fan, hipStream_t st) override;

    // training paths (butd_train.hip)
    TrainBuf tb;
    icz_rng rng = {};
    const float* cur_feats = nullptr;
    int ensure_train(int B, int T);
    int train_step(const float* feats, int rows, int Bs, int t, bool train, hipStream_t st, bool emb_ready = false, int* pred_nsplit = nullptr,
                   bool skip_predict = false, const int* live = nullptr, int row0 = 0);
    int sample(const float* feats, int B, int T, const icz_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st);
    int sample_n(const float* feats, int B, int K, int T, const icz_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st);
    int sample_n_impl(const float* feats, int B, int K, int T, int64_t* seq_out, float* logp_out, hipStream_t st);
    int sample_mask_sum(float* out, hipStream_t st);
    int xe_forward(const float* feats, const int64_t* captions, int B, int L, const int32_t* lengths, const icz_rng* r,
                   int train, float* packed_out, hipStream_t st);
    // teacher-forced XE on K captions per image (beyond the reference): sample_n's layout -- the prologue once per image, the chain over
    // the B K image-major rows, every row stored at every step (a row that has ended is fed <pad>; rows_t = B K throughout)
    int xe_forward_n(const float* feats, const int64_t* captions, int B, int K, int L, const int32_t* lengths, const icz_rng* r,
                     int train, float* logits_out, hipStream_t st);
    bool xe_grouped() const { return mode == 2 && cur_K > 1; }      // the stored forward pass is xe_forward_n's
    // The backward pass of the stored forward pass behind the loss head `hd` (every icz_butd_*_backward* entry): the refusals of a
    // grouped forward, the head's own rules, the head, bptt().  A ROLLOUT head and its bptt() replay as captured graphs (graphs_on()).
    int backward(LossHead hd, const icz_butd_params* G, hipStream_t st);
    int gemm_auto(GemmLayout layout, GemmArgs& g, float* slab, size_t slab_floats, int* ns_out, hipStream_t st);
    // the wgrad slab region of the stream a product is issued on: never shared between streams (TrainBuf::wslab)
    int wslab_of(hipStream_t st) const { return st == low.st ? 1 : 0; }
    int wgrad(const float* dY, int ldy, int M, const float* X, int ldx, int N, int K, float* out, int ldo, hipStream_t st, const int* rows_live = nullptr);
    int bptt_prelude(hipStream_t st);
    // phases: one bit per phase function below.  A call joins every branch it forked before it returns.  Values other than 0xF arise
    // only in the callback path of backward() (one captured graph per phase), where the only branch, phase 0's predict branch,
    // is joined behind the loop of that same call.  eo: the early-out of a sampled rollout applies (a rollout head and option "early_out").
    int bptt(const icz_butd_params& G, hipStream_t st, bool eo, int phases = 0xF, bool fire_cb = true);
    struct BpttCall;
    int bptt_predict(BpttCall& c);              // bit 0: d h2drop, the predict layer's gradients (side branch) ...
    int bptt_loop(BpttCall& c);                 //        ... and the reverse-time loop
    int bptt_embed_td_wgrad(BpttCall& c);       // bit 1: embedding gradient, TD-LSTM weight gradients
    int bptt_lm_wgrad(BpttCall& c);             // bit 2: LM-LSTM weight gradients
    int bptt_attention_tail(BpttCall& c);       // bit 3: attention block, bias sums, weight-norm backward
};

// ---------------------------------------------------------------------------------------------------------
// The launches of the attention kernels (butd_kernels.h): template instance, grid and dynamic LDS size of each, in one place.  Butd::step,
// the BPTT and the kernel-alone test entries (butd_att_test_entries.hip, tests/test_gpu_butd_att_kernels.py) all launch through these,
// so what the tests run is what the decoders run.  `ad`: the <true> instances (Butd::adaptive()).  `parts`: Butd::ATT_PARTS in the decoders.
inline void launch_mean_feats(const float* feats, float* mean, int n_img, int R, int D, const int32_t* counts, hipStream_t st) {
    if (counts) hipLaunchKernelGGL(mean_feats_counts_kernel, dim3(cdiv(D, 1024), n_img), dim3(256), 0, st, feats, mean, R, D, counts);
    else hipLaunchKernelGGL(mean_feats_kernel, dim3(cdiv(D, 1024), n_img), dim3(256), 0, st, feats, mean, R, D);
}
enum AttRoute { ATT_PER_ROW = 0, ATT_GROUP = 1, ATT_GROUP_TRAIN = 2 };
constexpr size_t ATT_GROUP_LDS = 60 * 1024;      // the G dec_ctx rows of a grouped score kernel
// what a grouped score launch needs of its shape (Butd::step asks G > 1 besides: one row per image is the per-row kernel's)
inline bool att_scores_group_fits(int rows, int G, int A) {
    return G >= 1 && G <= ATT_CTX_MAX_G && rows % G == 0 && sizeof(float) * A * G <= ATT_GROUP_LDS;
}
inline void launch_att_scores(AttRoute route, bool ad, const AttScoreArgs& a, const DropCfg& dc, int G, int parts, hipStream_t st) {
    if (route == ATT_GROUP)                   // beam search
        hipLaunchKernelGGL(ad ? att_scores_group_kernel<true> : att_scores_group_kernel<false>, dim3(a.rows / G, parts), dim3(256),
                           sizeof(float) * a.A * G, st, a, G);
    else if (route == ATT_GROUP_TRAIN)        // the multi-sample rollout (sample_n): dropout per row, early-out
        hipLaunchKernelGGL(ad ? att_scores_group_train_kernel<true> : att_scores_group_train_kernel<false>, dim3(a.rows / G, parts), dim3(256),
                           sizeof(float) * a.A * G, st, a, dc, G);
    else
        hipLaunchKernelGGL(ad ? att_scores_kernel<true> : att_scores_kernel<false>, dim3(a.rows, parts), dim3(256), sizeof(float) * a.A, st, a, dc);
}
// G > 0: the grouped kernel (rows = n_img G, img_of_row and alpha_out2 are not taken); G = 0: the per-row kernel
inline void launch_att_ctx(bool ad, const float* feats, const int32_t* img_of_row, const float* scores, float* alpha_out, float* alpha_out2,
                           int alpha2_stride, float* ctx, int rows, int R, int D, int G, const int* live, const int32_t* counts, hipStream_t st) {
    if (G > 0)
        hipLaunchKernelGGL(ad ? att_ctx_group_kernel<true> : att_ctx_group_kernel<false>, dim3(rows / G, cdiv(D, 512)), dim3(256), 0, st, feats, scores,
                           alpha_out, ctx, R, D, G, live, counts);
    else
        hipLaunchKernelGGL(ad ? att_ctx_kernel<true> : att_ctx_kernel<false>, dim3(rows, cdiv(D, 512)), dim3(256), 0, st, feats, img_of_row, scores,
                           alpha_out, alpha_out2, alpha2_stride, ctx, R, D, live, counts);
}
inline int att_dalpha_parts(int D) { return cdiv(D, DALPHA_COLS); }
// dalpha_part: [rows][att_dalpha_parts(D)][R]
inline void launch_att_bwd_dalpha(bool ad, const float* dctx, int ns, int ldc, int rows, const float* feats, int R, int D, float* dalpha_part,
                                  const int* live, const int32_t* img_of_row, const int32_t* counts, hipStream_t st) {
    hipLaunchKernelGGL(ad ? att_bwd_dalpha_kernel<true> : att_bwd_dalpha_kernel<false>, dim3(rows, att_dalpha_parts(D)), dim3(256), 0, st, dctx, ns, ldc,
                       rows, feats, R, D, dalpha_part, live, img_of_row, counts);
}
inline void launch_att_bwd_ddec(bool ad, const AttBwdDdecArgs& a, const DropCfg& dc, int rows, hipStream_t st) {
    hipLaunchKernelGGL(ad ? att_bwd_ddec_kernel<true> : att_bwd_ddec_kernel<false>, dim3(rows, cdiv(a.A, 256)), dim3(256), 0, st, a, dc);
}
constexpr int ATT_DENC_TT = 20;                  // time steps of dec_ctx a d enc_ctx thread keeps in registers
// parts of the grouped d enc_ctx kernel: DENC_GROUP_REGS regions each (more than `parts` only above parts * DENC_GROUP_REGS regions)
inline int att_denc_group_parts(int R, int parts) { return parts * DENC_GROUP_REGS >= R ? parts : cdiv(R, DENC_GROUP_REGS); }
// G > 0: the grouped kernel over the n_img images of a.B = n_img G rows with `parts` = att_denc_group_parts(...); G = 0: the per-row kernel over a.B rows
inline void launch_att_bwd_denc(bool ad, const AttBwdDencArgs& a, int n_img, int G, int parts, hipStream_t st) {
    if (G > 0)
        hipLaunchKernelGGL((ad ? att_bwd_denc_group_kernel<ATT_DENC_TT, true> : att_bwd_denc_group_kernel<ATT_DENC_TT, false>), dim3(n_img, parts),
                           dim3(256), sizeof(float) * a.T * a.R, st, a, G);
    else
        hipLaunchKernelGGL((ad ? att_bwd_denc_kernel<ATT_DENC_TT, true> : att_bwd_denc_kernel<ATT_DENC_TT, false>), dim3(a.B, parts), dim3(256),
                           sizeof(float) * a.T * a.R, st, a);
}

}  // namespace icz
