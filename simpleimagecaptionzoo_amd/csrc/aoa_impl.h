// AoADetection captioner (Models/AoA_Model.py:657-753): feature projection + 6-layer AoA refiner (once per image) and
// the AoA decoder (LSTM + LayerNorm + 8-head attention over the 36 refined regions + GLU gate) -- greedy / sampled /
// beam decoding and teacher-forced XE, with BPTT for the decoder parameters (the only ones the reference optimises,
// AoA_Model.py:669-674).  linear_K / linear_V of the decoder block are hoisted out of the time loop (the reference
// recomputes them every step, :114-115).
#pragma once
#include <math.h>

#include <vector>

#include "aoa_kernels.h"
#include "decoder_core.h"

namespace icz {

enum AoaRngStream : uint32_t { AOA_RNG_PROJ = 10, AOA_RNG_REF_ATT = 11, AOA_RNG_REF_AOA = 12, AOA_RNG_REF_SC = 13,
                               AOA_RNG_CTX = 20, AOA_RNG_ATT = 21, AOA_RNG_OUT = 22 };

struct AoaStepIO {
    int rows;
    const int32_t* img_of_row;      // null = identity (row b decodes image b)
    const int64_t* it;
    bool emb_ready;
    const float *h_in, *m_in, *ctx_in;
    float *h_out, *m_out, *ctx_out;
    // per-step tensors; training passes slots of the saved [T,B,...] buffers, inference the scratch ones
    float *emb, *u, *gates_out, *ln_stats, *qn, *Qp, *P_out, *Pd_out, *xatt, *z_out, *ctxdrop, *logits;
    DropCfg d_emb;                   // embedding dropout (p = 0.5) through the BUTD embedding kernel
    DropP d_ctx, d_att, d_out;
    bool u_ready;                    // s.u was written by the previous step's GLU kernel (skip aoa_u_kernel)
    float* u_next;                   // where this step's GLU kernel leaves the next step's u (null: it does not)
    DropP d_ctx_next;                // the next step's ctx dropout
    int* pred_nsplit;                // non-null: the caller's consumer sums split-K slabs of the predict GEMM (gemm_predict)
    bool skip_predict;               // teacher-forced XE forward: the vocabulary projection of all time steps is one GEMM after the loop
    const int* live;                 // rollouts: the count of unfinished rows after the previous step; 0 = every kernel of this step returns at
                                     // entry (step_dead, icz_common.h: the reference's break, AoA_Model.py:400)
};

// ---- launch code of the AoA kernels, shared by the handle and the kernel-alone test entries (icz_test_aoa_*, include/icz.h) -------
// They take the shape, never a handle: what they decide (route, chunk, LDS bytes, opt-in) is a function of their arguments alone.
constexpr size_t AOA_LDS_BUDGET = 156 * 1024;
// the one owner of a DropP: mode 0 off, 1 explicit keep-mask, 2 Philox word >= floor(p 2^32) of (*seed, stream, step)
inline DropP aoa_dropp(int mode, const uint8_t* mask, const uint64_t* seed, uint32_t stream, int step, float p, uint64_t idx0 = 0) {
    DropP d = {0, nullptr, seed, stream, (uint32_t)step, (uint32_t)((double)p * 4294967296.0), 1.0f / (1.0f - p)};
    d.idx0 = idx0;
    if (mode == 0) return d;
    if (mode == 1) { d.mode = 1; d.mask = mask; } else d.mode = 2;
    return d;
}
// mha_self_kernel's LDS for heads of d columns: K, V [R4][ld] + Q chunk [qc4][ld] + P [qc4][lp]
inline size_t aoa_self_lds(int R, int d, int qc) {
    const size_t ld = aoa_pitch(d), lp = aoa_pitch(R), R4 = (R + 3) & ~3, q4 = (qc + 3) & ~3;
    return sizeof(float) * (2 * R4 * ld + q4 * ld + q4 * lp);
}
// query rows per pass of mha_self_kernel: all of them when the tiles fit, else the largest multiple of 4 that does (0: none)
inline int aoa_self_qc(int R, int d) {
    if (aoa_self_lds(R, d, R) <= AOA_LDS_BUDGET) return R;
    int qc = R & ~3;
    while (qc >= 4 && aoa_self_lds(R, d, qc) > AOA_LDS_BUDGET) qc -= 4;
    return qc >= 4 ? qc : 0;
}
constexpr size_t AOA_SELF_MFMA_LDS = sizeof(float) * 64 * 68;      // mha_self_mfma_kernel: [RP][RP + 4], RP <= 64
// the refiner self-attention's kernel: 2 = mha_self_mfma_kernel (<= 64 regions, heads of whole 64-column trips), 1 = mha_self_kernel
inline int aoa_self_route(int R, int Hd, int NH, bool mha_mfma) { return mha_mfma && R <= 64 && (Hd / NH) % 64 == 0 ? 2 : 1; }
inline size_t aoa_dec_attn_lds(int R, int d) { return sizeof(float) * (2 * (size_t)R * (d + 1) + d + 128 + 4); }
// The one owner of the kernels' dynamic-LDS limits (aoa.hip): a launch of `lds` bytes above the 48 KB default needs its kernel's limit
// raised first.  The limit is a property of the process, not of a handle, so it only ever grows: `raised` (one slot per device, owned by
// the caller, one array per kernel) remembers what was set; calls are serialised.
constexpr int AOA_LDS_LIMIT_DEVICES = 64;
int aoa_raise_lds_limit(const void* kernel, size_t lds, size_t* raised);
int aoa_self_attn_optin(size_t lds);
int aoa_dec_attn_optin(size_t lds);
void aoa_launch_mha_self(int n_img, int R, int Hd, int NH, bool mha_mfma, int qc, size_t lds, const RegionRows& rr, const float* qkv_, float* o_,
                         const DropP& dp, hipStream_t st);
// geometry 0: four rows per workgroup (the refiner); 1: one wave per workgroup, with stats and live (the decoder)
void aoa_launch_layer_norm(int geometry, const float* x, const float* gain, const float* bias, float* y, int rows, int n, float* stats,
                           const int* live, hipStream_t st);
// Qp: the finished query projection (qns == 1) or its qns split-K slabs, q_stride apart, summed with q_bias into Qp_store
void aoa_launch_dec_attn(const float* Qp, int qns, size_t q_stride, const float* q_bias, float* Qp_store, const float* Kd, const float* Vd,
                         const int32_t* img_of_row, float* xatt, float* P_out, float* Pd_out, int rows, int R, int Hd, int NH, const RegionRows& rr,
                         const DropP& dp, const int* live, hipStream_t st);

// LayerNorm backward, one workgroup per row (n % 4 == 0, n <= 4096): aoa_ln_bwd_kernel on stored statistics (the decoder's h_norm;
// aoa_train.hip) and aoa_ln_bwd_dense_kernel on recomputed ones (the refiner's norms; aoa_refine_train.hip)
void aoa_launch_ln_bwd(const float* dq_a, int ns_a, const float* dq_b, int ns_b, int rows, const float* x, const float* stats, const float* gain,
                       float* dq_tot, float* dx, int n, const int* live, hipStream_t st);
void aoa_launch_ln_bwd_dense(const float* dq_a, int ns_a, const float* dq_b, int rows, const float* x, const float* gain, const float* res,
                             float* dq_tot, float* prod, float* dx, int n, hipStream_t st);
// mha_self_bwd_kernel (aoa_refine_train.hip): LDS bytes for images of up to R regions, the opt-in (capped at the budget: a narrower batch
// may fit where a handle's capacity does not) and the launch
inline size_t aoa_self_bwd_lds(int R, int d) { return sizeof(float) * mha_self_bwd_lds_floats(R, d); }
int aoa_self_attn_bwd_optin(size_t lds);
void aoa_launch_mha_self_bwd(const float* qkv, const float* dO, float* dqkv, int n_img, int R, int Hd, int NH, const RegionRows& rr, const DropP& dp,
                             hipStream_t st);
// aoa_dec_attn_bwd_kernel (aoa_train.hip): K tile, V tile [R][d + 1], q [d], dx [d], dS [128], red [4]
inline size_t aoa_dec_attn_bwd_lds(int R, int d) { return sizeof(float) * (2 * (size_t)R * (d + 1) + 2 * (size_t)d + 128 + 4); }
int aoa_dec_attn_bwd_optin(size_t lds);
void aoa_launch_dec_attn_bwd(const float* dxq, int ns, int rows, const float* Pm, const float* Pdm, const float* Qp, const float* Kd, const float* Vd,
                             float* dQp, float* dS_out, float* dx_out, int R, int Hd, int NH, const RegionRows& rr, float keep_scale, const int* live,
                             const int32_t* img_of_row, hipStream_t st);
// aoa_dkv_kernel: (k, t) pairs per pass -- all `pairs` of an image when their dS / Pd / Qp / dx rows fit 48 KB of LDS, else as many as do
inline size_t aoa_dkv_lds(int tc, int R, int d) { return sizeof(float) * (size_t)tc * 2 * (R + d); }
inline int aoa_dkv_tc(int pairs, int R, int d) {
    const int tc_fit = (int)(48 * 1024 / (sizeof(float) * 2 * (R + d)));
    return pairs < tc_fit ? pairs : tc_fit;
}
void aoa_launch_dkv(const float* dS_all, const float* Pd_all, const float* Qp_all, const float* dx_all, float* dKd, float* dVd, int n_img, int B, int T,
                    int tc, int R, int Hd, int NH, const RegionRows& rr, int G, hipStream_t st);

struct Aoa : CaptionHead, DecodeMember {
    static constexpr int STEP_WGS = 256, TARGET_WGS = 512, NL = 6;
    icz_aoa_dims dims;
    icz_aoa_params P;
    bool bound = false, fresh = false;
    DeviceBuffers mem;
    int Vp = 0;
    float *w_pred = nullptr, *n_pred = nullptr, *zeros = nullptr;
    float* w_qkv[NL] = {}; float* b_qkv[NL] = {};       // per refiner layer [3Hd, Hd] / [3Hd]: linear_Q | linear_K | linear_V (refresh)
    float* w_rec = nullptr;          // [4Hd, 2Hd] = [W_ih[:, E:] | W_hh]: one dgrad GEMM per BPTT step for (du, dh_prev)
    // refiner scratch / per-image tensors (rows = max_rows * R).  Two banks: bank 0 serves the evaluation-mode paths (greedy,
    // beam), bank 1 the training-mode ones (sample, XE, backward), so that the greedy baseline and the sampled rollout of
    // one SCST step can be in flight together; use_bank() points the members below at a bank before a chain is enqueued.
    struct Bank { float *xa, *xb, *ln, *qkv, *o, *od, *nd, *z, *refined, *meanf, *Kd, *Vd, *ws; int32_t *off, *rowmap; float* featp; };
    Bank bank[2] = {};
    int cur_bank = 0;
    // (round 5) the two refiner passes of an SCST step as ONE pass over [evaluation rows; training rows] (refine_pair): buffers of twice the
    // rows; while a pair is current, the banks' result pointers (refined, meanf, Kd, Vd) point at its halves, own[] keeps the banks' own
    Bank dual = {};
    Bank own[2] = {};
    bool pair_refine = true;             // icz_aoa_set_option("refine_pair")
    void point_banks_at_pair(int n_img) {
        const size_t nel = (size_t)n_img * cur_R * dims.Hd, nm = (size_t)n_img * dims.Hd;
        bank[0].refined = dual.refined; bank[0].meanf = dual.meanf; bank[0].Kd = dual.Kd; bank[0].Vd = dual.Vd;
        bank[1].refined = dual.refined + nel; bank[1].meanf = dual.meanf + nm; bank[1].Kd = dual.Kd + nel; bank[1].Vd = dual.Vd + nel;
        use_bank(cur_bank);
    }
    void point_bank_at_own(int b) {
        bank[b].refined = own[b].refined; bank[b].meanf = own[b].meanf; bank[b].Kd = own[b].Kd; bank[b].Vd = own[b].Vd;
        use_bank(cur_bank);
    }
    void use_bank(int b) {
        cur_bank = b;
        const Bank& s = bank[b];
        xa = s.xa; xb = s.xb; ln = s.ln; qkv = s.qkv; o = s.o; od = s.od; nd = s.nd; z = s.z;
        refined = s.refined; meanf = s.meanf; Kd = s.Kd; Vd = s.Vd; ws = s.ws; off = s.off; rowmap = s.rowmap;
    }
    // hipGraph replay of the SCST rollout pair and of the REINFORCE backward pass (option "graphs"; fixed region counts and Philox
    // randomness only: an 'adaptive' batch changes its grid sizes, explicit mask arrays their addresses)
    GraphCache gc{16};
    bool use_graphs = false;
    float* proj_shared = nullptr;        // rollouts: img_feats_porjection(feats) before ReLU / dropout, computed ONCE for the evaluation-
                                         // mode pass of the greedy baseline and the training-mode pass of the sampled rollout
    SideStream side;                     // the greedy chain of the SCST rollout pair
    SideStream low;                      // backward: the predict layer's weight gradient beside the reverse-time loop (plain priority); its second
                                         // event pair: (round 6) the attention block's small products beside the weight-gradient GEMMs of bptt's tail
    float *xa = nullptr, *xb = nullptr, *ln = nullptr, *qkv = nullptr, *o = nullptr, *od = nullptr, *nd = nullptr,
          *z = nullptr, *refined = nullptr, *meanf = nullptr, *Kd = nullptr, *Vd = nullptr;
    // decoder state + scratch
    float *h[2], *m[2], *ctx[2];
    float *emb = nullptr, *u = nullptr, *qn = nullptr, *Qp = nullptr, *xatt = nullptr, *ctxdrop = nullptr, *logits = nullptr, *ws = nullptr;
    size_t ws_floats = 0;
    int64_t* it = nullptr;
    float* amax_val = nullptr; int* amax_idx = nullptr;
    icz_grad_ready_cb grad_cb = nullptr; void* grad_cb_user = nullptr;      // DP overlap hook (icz_aoa_set_grad_callback)
    // training buffers (aoa_train.hip), slot stride = max_rows: th/tm/tctx slot 0 = zeros, slot t+1 = after step t
    int tcap_B = 0, tcap_T = 0, tcap_I = 0;      // capacity of the training buffers in decoder rows, steps and images (grown on demand by ensure_train)
    int64_t* tok = nullptr;
    float *th = nullptr, *tm = nullptr, *tctx = nullptr, *temb = nullptr, *tu = nullptr, *tg = nullptr, *tstats = nullptr, *tqn = nullptr,
          *tQp = nullptr, *tP = nullptr, *tPd = nullptr, *tdS = nullptr, *tdX = nullptr, *txatt = nullptr, *tz = nullptr, *tcd = nullptr, *tlogit = nullptr;
    float *dCd = nullptr, *dZ = nullptr, *dQp = nullptr, *dQn = nullptr, *dHln = nullptr, *dG = nullptr, *dEmb = nullptr, *dKd = nullptr,
          *dVd = nullptr, *dcb[2] = {nullptr, nullptr}, *X = nullptr, *X2 = nullptr, *dWp = nullptr, *prod = nullptr;
    size_t xfloats = 0;
    // option "train_refiner" (aoa_refine_train.hip): a training-mode refiner pass keeps the input of every layer and of the final norm
    // (xs[l], xs[NL]: region rows x Hd each); the backward pass recomputes one layer at a time from them.  Training buffers, allocated
    // only while the option is on.
    bool train_refiner = false;
    float* xs[NL + 1] = {};
    bool xs_valid = false;               // xs hold the pass the stored forward state belongs to
    const float* ref_feats = nullptr;    // what that pass projected: the caller's features, or the bank's packed rows
    float *rdx[2] = {nullptr, nullptr}, *rdz = nullptr, *rdo = nullptr, *rdln = nullptr, *rdqkv = nullptr, *rdq = nullptr, *rprod = nullptr,
          *rslab = nullptr, *rdmean = nullptr;
    size_t rslab_floats = 0;
    void drop_refiner_buffers() {
        for (float*& p : xs) p = nullptr;
        rdx[0] = rdx[1] = rdz = rdo = rdln = rdqkv = rdq = rprod = rslab = rdmean = nullptr;
        rslab_floats = 0; xs_valid = false; ref_feats = nullptr;
    }
    int set_train_refiner(bool on);
    int alloc_refiner_train(size_t B, size_t TB);
    int refiner_backward_check(const icz_aoa_params& G) const;      // argument / capacity errors, raised before any launch
    int refiner_backward(const icz_aoa_params& G, hipStream_t st);
    icz_aoa_rng rng = {};
    // regions per image of the current batch: row stride cur_R <= dims.R and, for the 'adaptive' bottom-up features
    // (10..100 boxes, AoA_Engine.py:37-44), the valid count per image (device, caller-owned; null = all cur_R)
    int cur_R = 0, lens_n = 0, cur_total = 0;      // cur_total = sum of the counts = rows of the packed refiner tensors
    const int32_t* lens = nullptr;
    int32_t *off = nullptr, *rowmap = nullptr;     // per bank: row offsets / padded indices of the packed rows (RegionRows)
    RegionRows region_rows() const { return lens ? RegionRows{off, rowmap, lens, cur_R} : RegionRows{nullptr, nullptr, nullptr, cur_R}; }
    size_t region_row_count(int n_img) const { return lens ? (size_t)cur_total : (size_t)n_img * cur_R; }
    static constexpr size_t LDS_BUDGET = AOA_LDS_BUDGET;
    size_t self_lds(int R, int qc) const { return aoa_self_lds(R, dims.Hd / dims.NH, qc); }
    int self_qc(int R) const { return aoa_self_qc(R, dims.Hd / dims.NH); }

    int alloc(void** p, size_t bytes) { return mem.alloc(p, bytes); }
    int init(const icz_aoa_dims& d);
    int refresh(hipStream_t st);
    // out[M,N] = A[M,K] W[N,K]^T + bias  (split-K through `ws` when the launch would be too small)
    int lin(const float* A, int M, int K, const float* W, const float* bias, int N, float* out, hipStream_t st);
    int refine(const float* feats, int n_img, bool train, hipStream_t st, const float* proj = nullptr);
    int refine_pair(int n_img, hipStream_t st, const float* proj);
    bool mha_mfma = true;                // icz_aoa_set_option("mha_mfma"): refiner self-attention on the fp32 matrix pipe (<= 64 regions)
    void launch_mha_self(int n_img, int R, int qc, size_t lds, const RegionRows& rr, const float* qkv_, float* o_, const DropP& dp, hipStream_t st) {
        aoa_launch_mha_self(n_img, R, dims.Hd, dims.NH, mha_mfma, qc, lds, rr, qkv_, o_, dp, st);
    }
    // layer l's self-attention of a pass of its own over n_img images, qkv -> o of the current bank (the backward pass's recompute)
    void mha_self_layer(int n_img, int l, bool train, hipStream_t st);
    int project(const float* feats, int n_img, float* out, hipStream_t st);
    int step(const AoaStepIO& s, hipStream_t st);
    int greedy(const float* feats, int B, int T, int64_t* ids_out, hipStream_t st, const float* proj = nullptr, bool scst = false, bool refined_ready = false);
    int rollouts_impl(const float* feats, int B, int T, int64_t* ids_out, int64_t* seq_out, float* logp_out, hipStream_t st);
    int rollouts(const float* feats, int B, int T, const icz_aoa_rng* r, int64_t* ids_out, int64_t* seq_out, float* logp_out, hipStream_t st);
    // decoder seams (DecodeMember, decoder_core.h): the refiner pass, one decoder step, the beam-state gather
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
    DropP dropp(bool train, const uint8_t* mask, size_t off, uint32_t stream, int step, float p) const {
        return aoa_dropp(!train ? 0 : mask ? 1 : 2, mask ? mask + off : nullptr, d_seed, stream, step, p);
    }
    DropCfg dropbits(bool train, const uint8_t* mask, size_t off, uint32_t stream, int step) const {
        DropCfg d = {0, nullptr, d_seed, stream, (uint32_t)step};
        if (!train) return d;
        if (mask) { d.mode = 1; d.mask = mask + off; } else d.mode = 2;
        return d;
    }
    // training paths (aoa_train.hip)
    int ensure_train(int B, int T, int n_img = 0);
    // multi-sample SCST rollout (sample_n, beyond the reference): cur_K (CaptionHead) sampled rows per image, row = img * K + k; cur_B
    // stays the decoder rows; imgk = the image of each row, allocated by the first sample_n
    int32_t* imgk = nullptr;
    int sample_n(const float* feats, int B, int K, int T, const icz_aoa_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st);
    int sample_n_impl(const float* feats, int B, int K, int T, int64_t* seq_out, float* logp_out, hipStream_t st);
    AoaStepIO train_io(int rows, int t, bool train);
    int sample(const float* feats, int B, int T, const icz_aoa_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st);
    int sample_prelude(const float* feats, int B, int T, const icz_aoa_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st, int K = 1);
    int sample_impl(const float* feats, int B, int T, int64_t* seq_out, float* logp_out, hipStream_t st, const float* proj = nullptr, bool refined_ready = false,
                    int n_img = 0);
    int xe_forward(const float* feats, const int64_t* captions, int B, int L, const int32_t* lengths, const icz_aoa_rng* r, int train,
                   float* packed_out, hipStream_t st);
    // The backward pass of the stored forward pass behind the loss head `hd` (every icz_aoa_*_backward* entry): the head's rules, the
    // refiner's, the head, bptt().  A ROLLOUT head and its bptt() replay as one captured graph (option "graphs").
    int backward(const LossHead& hd, const icz_aoa_params* G, hipStream_t st);
    // the driver over the parts below, then refiner_backward; eo: the early-out of a sampled rollout applies
    int bptt(const icz_aoa_params& G, hipStream_t st, bool eo);
    struct BpttCall;
    int bptt_predict(BpttCall& c);              // d(dropped ctx) and the predict layer's gradients (side branch)
    int bptt_loop(BpttCall& c);                 // the reverse-time loop
    int bptt_embed_lstm_wgrad(BpttCall& c);     // embedding gradient, LSTM weight / bias gradients
    int bptt_aoa_wgrad(BpttCall& c);            // the AoA linear layer's gradients
    int bptt_attention_tail(BpttCall& c);       // the attention block's small products (tail branch)
    // g.out (dense [M,N]) = sum_s A_s W_s^T + bias; split-K slabs through `ws` when one pass would leave most CUs idle
    int linear(GemmArgs g, const float* bias, hipStream_t st);
    // slabs [ns][M][N] = A[M,K] . B[K,N] (ns == 1: the dense product) in `slab` of `cap` floats, for the consumer to sum
    static int nn(const float* A, int lda, int M, int K, const float* Bm, int ldb, int N, float* slab, size_t cap, int* ns, const SplitPolicy& p,
                  hipStream_t st, const int* live = nullptr, const int* rows_live = nullptr);
};

}  // namespace icz
