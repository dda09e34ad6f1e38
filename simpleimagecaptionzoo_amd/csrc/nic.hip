// NIC decoder (Models/NIC_Model.py:39-212): single LSTM over a plain embedding; the image embedding enters through one
// LSTM step from the zero state.  Same kernels as the BUTD decoder (GEMMs, LSTM pointwise, select / beam / loss
// kernels); only the launch sequences differ.
#include <math.h>

#include <vector>

#include "ens_sample.h"
#include "lstm_kernels.h"
#include "support_kernels.h"
#include "token_kernels.h"

namespace icz {

struct Nic : CaptionHead, DecodeMember {
    static constexpr int STEP_WGS = 256, TARGET_WGS = 512;
    icz_nic_dims dims;
    icz_nic_params P;
    bool bound = false, fresh = false;
    DeviceBuffers mem;
    int Vp = 0;
    float *w_pred = nullptr, *n_pred = nullptr, *zeros = nullptr;
    float *h[2], *c[2];
    float *emb = nullptr, *hdrop = nullptr, *logits = nullptr, *ws = nullptr;
    size_t ws_floats = 0;
    int64_t* it = nullptr;
    float* amax_val = nullptr; int* amax_idx = nullptr;
    // training buffers (slot stride = capacity rows): th/tc slot 0 = zeros, slot 1 = after the image step, slot t+2 =
    // after token step t; tg / dG slot 0 = image step, slot t+1 = token step t
    int tcap_B = 0, tcap_T = 0;          // capacity of the training buffers (grown on demand by ensure_train)
    int64_t* tok = nullptr;
    float *th = nullptr, *tc = nullptr, *temb = nullptr, *tg = nullptr, *thd = nullptr, *tlogit = nullptr;
    float *dG = nullptr, *dHd = nullptr, *dEmb = nullptr, *dcb[2] = {nullptr, nullptr}, *X = nullptr, *dWp = nullptr;
    size_t xfloats = 0;
    float* feat_rows = nullptr;          // beam search: the image embedding replicated per beam row (prologue)
    // multi-sample SCST rollout (sample_n, beyond the reference): cur_K (CaptionHead) sampled rows per image, row = img * K + k; the
    // rollout runs on the image embeddings expanded to the rows, the backward pass folds d features back onto the images
    int32_t* imgk = nullptr;             // image of each decoder row
    float *feat_n = nullptr, *dfeat_n = nullptr;      // [max_rows, E]: the expanded embeddings (kept for the backward pass), their gradient per row
    icz_rng rng = {};
    const float* cur_feats = nullptr;

    int alloc(void** p, size_t bytes) { return mem.alloc(p, bytes); }
    int init(const icz_nic_dims& d);
    int refresh(hipStream_t st);
    int image_step(const float* feats, int rows, float* h_out, float* c_out, float* gates_out, hipStream_t st);
    int token_step(int rows, const int64_t* tokens, bool emb_ready, const float* h_in, const float* c_in, float* h_out, float* c_out,
                   float* emb_out, float* gates_out, float* hdrop_out, float* logits_out, DropCfg drop_out, hipStream_t st, int* pred_nsplit = nullptr,
                   const int* live = nullptr);
    int greedy(const float* feats, int B, int T, int64_t* ids_out, hipStream_t st);
    int ensure_train(int B, int T);
    int sample(const float* feats, int B, int T, const icz_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st);
    int sample_n(const float* feats, int B, int K, int T, const icz_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st);
    int xe_forward(const float* feats, const int64_t* captions, int B, int L, const int32_t* lengths, const icz_rng* r, int train,
                   float* packed_out, hipStream_t st);
    // the backward pass of the stored forward pass behind the loss head `hd` (every icz_nic_*_backward* entry; eager, as every NIC path)
    int backward(const LossHead& hd, const icz_nic_params* G, float* dfeats, hipStream_t st);
    // eo: rollout / BPTT steps behind sample_rl's break (NIC_Model.py:150) return at entry (a rollout head and option "early_out")
    int bptt(const icz_nic_params& G, float* dfeats, hipStream_t st, bool eo);
    int nn(const float* A, int lda, int M, int K, const float* Bm, int ldb, int N, float* out, int* ns, int target, hipStream_t st,
           const int* live = nullptr);
    // decoder seams (DecodeMember, decoder_core.h): the image step, one token step, the beam-state gather
    int vocab() const override { return dims.V; }
    int row_capacity() const override { return dims.max_rows; }
    bool refreshed() const override { return fresh; }
    bool compact_step() const override { return false; }
    EmbSlot emb_slot() const override { return {P.embed_weight, emb, dims.E, 0}; }
    DeviceBuffers& buffers() override { return mem; }
    int prologue(const float* feats, int n_img, int k, const int32_t* img_of_row, hipStream_t st) override;
    int step(int rows, const int64_t* it, const int32_t* img_of_row, int rows_per_img, int cur, bool slabs, LogitsView* out,
             hipStream_t st) override;
    void gather(const int32_t* src_row, int rows, int fan, hipStream_t st) override;
};

int Nic::init(const icz_nic_dims& d) {
    dims = d;
    ICZ_REQUIRE(d.E % 4 == 0 && d.H % 4 == 0 && d.V > 3 && d.max_rows > 0 && d.max_len > 0, "nic: bad dimensions");
    Vp = pad_vocab(d.V);
    const size_t rows = d.max_rows, H = d.H, E = d.E;
    ICZ_TRY(alloc((void**)&w_pred, sizeof(float) * Vp * H));
    ICZ_TRY(alloc((void**)&n_pred, sizeof(float) * d.V));
    ICZ_TRY(alloc((void**)&zeros, sizeof(float) * rows * H));
    for (int i = 0; i < 2; ++i) { ICZ_TRY(alloc((void**)&h[i], sizeof(float) * rows * H)); ICZ_TRY(alloc((void**)&c[i], sizeof(float) * rows * H)); }
    ICZ_TRY(alloc((void**)&emb, sizeof(float) * rows * E));
    ICZ_TRY(alloc((void**)&hdrop, sizeof(float) * rows * H));
    ICZ_TRY(alloc((void**)&logits, sizeof(float) * rows * Vp));
    ICZ_TRY(alloc((void**)&it, sizeof(int64_t) * rows));
    ICZ_TRY(alloc((void**)&amax_val, sizeof(float) * rows * ARGMAX_PARTS));
    ICZ_TRY(alloc((void**)&amax_idx, sizeof(int) * rows * ARGMAX_PARTS));
    ICZ_TRY(alloc_scalars(mem));
    const size_t nmax = 4 * H > (size_t)Vp ? 4 * H : (size_t)Vp;
    ws_floats = (size_t)TARGET_WGS * 4096 * 2 + rows * nmax;
    {   // the resident decoder-step GEMM (33..128 rows) leaves one slab per 256-deep k range of K = E + H (Butd::init's rule)
        const size_t kmax = (size_t)d.E + H, r128 = rows < 128 ? rows : 128;
        const size_t need = (kmax / 256 + 1) * r128 * 4 * H;
        if (need > ws_floats) ws_floats = need;
    }
    ICZ_TRY(alloc((void**)&ws, sizeof(float) * ws_floats));
    return mem.synced();
}

int Nic::refresh(hipStream_t st) {
    ICZ_REQUIRE(bound, "nic: parameters not bound");
    launch_weight_norm(P.predict_v, P.predict_g, w_pred, n_pred, dims.V, dims.H, st);
    ICZ_CHECK_HIP(hipGetLastError());
    fresh = true;
    return ICZ_OK;
}

// h, c = LSTMCell(features, (0, 0))   (NIC_Model.py:52-56)
int Nic::image_step(const float* feats, int rows, float* h_out, float* c_out, float* gates_out, hipStream_t st) {
    const int H = dims.H, E = dims.E;
    int ns;      // (the split is fitted to the workspace: the capacity check cannot fail)
    GemmArgs g = gemm_args({{feats, P.w_ih, E, E, E}}, rows, 4 * H, ws, 4 * H);
    ICZ_TRY(gemm_slabs(GEMM_NT, g, split_forward(STEP_WGS), ws, ws_floats, &ns, st, "nic"));
    LstmPointArgs a = {ws, ns, nullptr, nullptr, P.b_ih, P.b_hh, zeros, h_out, c_out, gates_out, nullptr, rows, H};
    DropCfg off = {0, nullptr, nullptr, 0, 0};
    launch_lstm_point(a, off, st);
    return ICZ_OK;
}

// embed -> LSTMCell -> predict(dropout(h))   (NIC_Model.py:112-114)
// live: step_dead (icz_common.h) -- every kernel of a rollout step behind the reference's break returns at entry
int Nic::token_step(int rows, const int64_t* tokens, bool emb_ready, const float* h_in, const float* c_in, float* h_out, float* c_out,
                    float* emb_out, float* gates_out, float* hdrop_out, float* logits_out, DropCfg drop_out, hipStream_t st, int* pred_nsplit,
                    const int* live) {
    const int H = dims.H, E = dims.E, V = dims.V;
    DropCfg off = {0, nullptr, nullptr, 0, 0};
    if (!emb_ready) hipLaunchKernelGGL(embed_kernel, dim3(cdiv(E, 1024), rows), dim3(256), 0, st, P.embed_weight, tokens, emb_out, rows, E, off, 0, live);
    int ns;      // (fitted split, as in image_step)
    GemmArgs g = gemm_args({{emb_out, P.w_ih, E, E, E}, {h_in, P.w_hh, H, H, H}}, rows, 4 * H, ws, 4 * H, live);
    ICZ_TRY(gemm_slabs(GEMM_NT, g, split_forward(STEP_WGS), ws, ws_floats, &ns, st, "nic"));
    LstmPointArgs a = {ws, ns, nullptr, nullptr, P.b_ih, P.b_hh, c_in, h_out, c_out, gates_out, hdrop_out, rows, H, live};
    launch_lstm_point(a, drop_out, st);
    ICZ_TRY(gemm_predict(hdrop_out, H, w_pred, P.predict_b, rows, V, Vp, logits_out, Vp, ws, ws_floats, pred_nsplit, st, live));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int Nic::greedy(const float* feats, int B, int T, int64_t* ids_out, hipStream_t st) {
    ICZ_REQUIRE(feats && ids_out && B > 0 && B <= dims.max_rows && T > 0, "nic greedy: bad arguments");
    ICZ_REQUIRE(fresh, "nic: call icz_nic_refresh_weights after binding/updating parameters");
    ICZ_TRY(image_step(feats, B, h[0], c[0], nullptr, st));
    hipLaunchKernelGGL(fill_i64_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, it, (int64_t)1, B);
    DropCfg off = {0, nullptr, nullptr, 0, 0};
    int cur = 0;
    for (int t = 0; t < T; ++t) {
        int pns = 1;
        ICZ_TRY(token_step(B, it, t > 0, h[cur], c[cur], h[cur ^ 1], c[cur ^ 1], emb, nullptr, hdrop, logits, off, st, &pns));
        launch_greedy_select(logits_view(ws, P.predict_b, logits, B, Vp, pns), emb_slot(), B, dims.V, amax_val, amax_idx, it, ids_out, T, t, nullptr,
                             nullptr, st);
        cur ^= 1;
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// Training buffers sized by what the batches ask for (the reference never truncates captions, Datasets.py:47-51: the step
// count of an XE batch is only known when it arrives); growing re-allocates them all.
int Nic::ensure_train(int Bq, int Tq) {
    if (Bq <= tcap_B && Tq <= tcap_T) return ICZ_OK;
    ICZ_REQUIRE(Tq <= XE_MAX_T, "nic: %d steps exceed the limit of %d", Tq, XE_MAX_T);
    if (tcap_B > Bq) Bq = tcap_B;
    if (tcap_T > Tq) Tq = tcap_T;
    if (dims.max_len > Tq) Tq = dims.max_len;
    if (!mem.training.empty()) {
        ICZ_TRY(mem.release_training(nullptr));
        tcap_B = tcap_T = 0;
        drop_loss_buffers();
    }
    DeviceBuffers::TrainingScope scope(mem);
    const size_t B = Bq, T = Tq, H = dims.H, E = dims.E;
    const size_t TB = T * B;
    ICZ_TRY(alloc((void**)&tok, sizeof(int64_t) * (TB + B)));
    ICZ_TRY(alloc((void**)&th, sizeof(float) * (TB + 2 * B) * H));
    ICZ_TRY(alloc((void**)&tc, sizeof(float) * (TB + 2 * B) * H));
    ICZ_TRY(alloc((void**)&temb, sizeof(float) * TB * E));
    ICZ_TRY(alloc((void**)&tg, sizeof(float) * (TB + B) * 4 * H));
    ICZ_TRY(alloc((void**)&thd, sizeof(float) * TB * H));
    ICZ_TRY(alloc((void**)&tlogit, sizeof(float) * TB * Vp));
    ICZ_TRY(alloc((void**)&dG, sizeof(float) * (TB + B) * 4 * H));
    ICZ_TRY(alloc((void**)&dHd, sizeof(float) * TB * H));
    ICZ_TRY(alloc((void**)&dEmb, sizeof(float) * TB * E));
    ICZ_TRY(alloc((void**)&dcb[0], sizeof(float) * B * H));
    ICZ_TRY(alloc((void**)&dcb[1], sizeof(float) * B * H));
    xfloats = (size_t)TARGET_WGS * 4096 * 2 + B * H;
    ICZ_TRY(alloc((void**)&X, sizeof(float) * xfloats));
    ICZ_TRY(alloc((void**)&dWp, sizeof(float) * (size_t)Vp * H));
    ICZ_TRY(alloc_loss_buffers(mem, TB, B, T));
    ICZ_TRY(mem.synced());
    tcap_B = Bq; tcap_T = Tq;
    return ICZ_OK;
}

static DropCfg nic_drop(const uint64_t* seed_p, bool train, const uint8_t* base, size_t per_step, int t) {
    DropCfg d = {0, nullptr, seed_p, RNG_OUT, (uint32_t)t};
    if (!train) return d;
    if (base) { d.mode = 1; d.mask = base + per_step * t; }
    else d.mode = 2;
    return d;
}

int Nic::sample(const float* feats, int B, int T, const icz_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_REQUIRE(feats && seq_out && logp_out && r && B > 0 && B <= dims.max_rows && T > 0, "nic sample: bad arguments");
    ICZ_REQUIRE(fresh, "nic: call icz_nic_refresh_weights after binding/updating parameters");
    ICZ_TRY(ensure_train(B, T));
    rng = *r;
    begin_rollout(B, T, seq_out, logp_out, rng.seed, st);
    cur_feats = feats; cur_K = 1;
    const size_t H = dims.H, E = dims.E, sH = (size_t)B * H;
    ICZ_CHECK_HIP(hipMemsetAsync(th, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tc, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(unf, 1, B, st));
    ICZ_CHECK_HIP(hipMemsetAsync(nunf, 0, sizeof(int) * T, st));
    hipLaunchKernelGGL(fill_i64_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, tok, (int64_t)1, B);
    ICZ_TRY(image_step(feats, B, th + sH, tc + sH, tg, st));
    for (int t = 0; t < T; ++t) {
        const size_t slot = (size_t)t * B;
        int pns = 1;
        ICZ_TRY(token_step(B, tok + slot, false, th + (slot + B) * H, tc + (slot + B) * H, th + (slot + 2 * B) * H, tc + (slot + 2 * B) * H,
                           temb + slot * E, tg + (slot + B) * 4 * H, thd + slot * H, tlogit + slot * Vp,
                           nic_drop(d_seed, true, rng.out_mask, sH, t), st, &pns, (t > 0 && early_out) ? nunf + (t - 1) : nullptr));
        SampleSelArgs a = {};
        a.logits = tlogit + slot * Vp; a.V = dims.V; a.ldl = Vp;
        if (pns > 1) { a.logits = ws; a.ns = pns; a.slab_stride = (size_t)B * Vp; a.bias = P.predict_b; a.logits_store = tlogit + slot * Vp; }
        a.uniforms = rng.uniforms ? rng.uniforms + slot : nullptr;
        a.seed_p = d_seed; a.t = t; a.T = T;
        a.unfinished = unf; a.n_unfinished = nunf; a.seq_out = seq_out; a.logp_out = logp_out;
        a.it_next = tok + slot + B; a.draw_out = draw + slot; a.lse_out = lse + slot;
        ICZ_TRY(launch_sample_select(st, B, a));
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// Multi-sample rollout (beyond the reference: K sampled captions per image): the image embeddings are expanded to the B K decoder rows,
// row = img * K + k, with the kernel the beam-search prologue uses, and the sampled rollout runs on those rows -- every launch is the
// launch of sample() on the embeddings repeated K times, so tokens, log-probs and parameter gradients are bitwise that call's.
int Nic::sample_n(const float* feats, int B, int K, int T, const icz_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_REQUIRE(feats && seq_out && logp_out && r, "nic sample_n: null argument");
    ICZ_REQUIRE(K >= 2 && K <= SAMPLE_N_MAX_K, "nic sample_n: K=%d samples per image outside 2..%d", K, SAMPLE_N_MAX_K);
    ICZ_REQUIRE(B > 0 && T > 0, "nic sample_n: bad B/T");
    ICZ_REQUIRE((int64_t)B * K <= dims.max_rows, "nic sample_n: %d images x %d samples exceed the row capacity %d", B, K, dims.max_rows);
    ICZ_REQUIRE(fresh, "nic: call icz_nic_refresh_weights after binding/updating parameters");
    const int rows = B * K;
    if (!imgk) {
        ICZ_TRY(alloc((void**)&imgk, sizeof(int32_t) * (size_t)dims.max_rows));
        ICZ_TRY(alloc((void**)&feat_n, sizeof(float) * (size_t)dims.max_rows * dims.E));
        ICZ_TRY(alloc((void**)&dfeat_n, sizeof(float) * (size_t)dims.max_rows * dims.E));
        ICZ_TRY(mem.synced());
    }
    hipLaunchKernelGGL(row_image_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, imgk, rows, K);
    hipLaunchKernelGGL(beam_expand_rows_kernel, dim3(cdiv(dims.E, 1024), rows), dim3(256), 0, st, feats, (const int32_t*)imgk, dims.E, feat_n);
    ICZ_TRY(sample(feat_n, rows, T, r, seq_out, logp_out, st));
    cur_K = K;
    return ICZ_OK;
}

int Nic::backward(const LossHead& hd, const icz_nic_params* G, float* dfeats, hipStream_t st) {
    ICZ_TRY(check_loss_head(hd, G));
    ICZ_TRY(begin_backward(hd, false, tlogit, dims.V, Vp, st));
    const bool eo = hd.rollout_kind() && early_out;
    if (!hd.rollout_kind() || cur_K == 1 || !dfeats) return bptt(*G, dfeats, st, eo);
    // behind sample_n: d features of the B K rows, then the K rows of an image added in k order -> [B, E]
    ICZ_TRY(bptt(*G, dfeat_n, st, eo));
    const int n_img = cur_B / cur_K;
    launch_rowgroup_sum(dfeat_n, n_img, cur_K, (size_t)dims.E, dfeats, st);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int Nic::xe_forward(const float* feats, const int64_t* captions, int B, int L, const int32_t* lengths, const icz_rng* r, int train,
                    float* packed_out, hipStream_t st) {
    ICZ_REQUIRE(feats && captions && lengths && B > 0 && B <= dims.max_rows && L > 1, "nic xe_forward: bad arguments");
    ICZ_REQUIRE(fresh, "nic: call icz_nic_refresh_weights after binding/updating parameters");
    ICZ_REQUIRE(!train || r, "nic xe_forward: training mode needs an icz_rng");
    int T = 0;
    ICZ_TRY(xe_steps("nic", lengths, B, L, &T));
    ICZ_TRY(ensure_train(B, T));
    if (r) rng = *r; else rng = {};
    begin_xe(lengths, B, T, L, captions, train != 0, rng.seed, st);
    cur_feats = feats;
    const size_t H = dims.H, E = dims.E, sH = (size_t)B * H;
    ICZ_CHECK_HIP(hipMemsetAsync(th, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tc, 0, sizeof(float) * sH, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tlogit, 0, sizeof(float) * (size_t)T * B * Vp, st));
    captions_to_tok(tok, st);
    ICZ_TRY(image_step(feats, B, th + sH, tc + sH, tg, st));
    for (int t = 0; t < T; ++t) {
        const size_t slot = (size_t)t * B;
        if (t >= 2 && ss_prob > 0.f)          // NIC_Model.py:77-89
            ICZ_TRY(ss_select_launch(st, rows_t[t], tlogit + (slot - B) * Vp, (int)Vp, dims.V, t, B, ss_prob, ss_gate, ss_draw, d_seed, tok + slot));
        ICZ_TRY(token_step(rows_t[t], tok + slot, false, th + (slot + B) * H, tc + (slot + B) * H, th + (slot + 2 * B) * H,
                           tc + (slot + 2 * B) * H, temb + slot * E, tg + (slot + B) * 4 * H, thd + slot * H, tlogit + slot * Vp,
                           nic_drop(d_seed, train != 0, rng.out_mask, sH, t), st));
    }
    if (packed_out) ICZ_TRY(gather_packed(tlogit, dims.V, Vp, packed_out, st));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// A[M,K] . B[K,N]: with ns_out, slabs [ns][M][N] in `out` (= X, one slab: the dense product) for the consumer to sum; without, the
// finished dense product in `out`, split-K slabs going through `ws`
int Nic::nn(const float* A, int lda, int M, int K, const float* Bm, int ldb, int N, float* out, int* ns_out, int target, hipStream_t st,
            const int* live) {
    GemmArgs g = gemm_args({{A, Bm, lda, ldb, K}}, M, N, out, N, live);
    if (ns_out) return gemm_slabs(GEMM_NN, g, split_backward(target), out, xfloats, ns_out, st, "nic");
    return gemm_finished(GEMM_NN, g, split_backward(target), nullptr, ws, ws_floats, st, "nic");
}

int Nic::bptt(const icz_nic_params& G, float* dfeats, hipStream_t st, bool eo) {
    const int B = cur_B, T = cur_T, H = dims.H, E = dims.E, V = dims.V;
    const int TB = T * B;
    const size_t sH = (size_t)B * H;
    // predict layer over all time steps
    ICZ_TRY(nn(tlogit, Vp, TB, Vp, w_pred, H, H, dHd, nullptr, TARGET_WGS, st));
    ICZ_TRY(gemm_tn(tlogit, Vp, Vp, thd, H, H, TB, dWp, H, 0, nullptr, st));
    ICZ_TRY(launch_colsum(tlogit, TB, V, Vp, G.predict_b, st));
    launch_weight_norm_bwd(dWp, H, P.predict_v, P.predict_g, n_pred, G.predict_v, G.predict_g, V, H, st);
    const bool ragged = rows_t[T - 1] < B;
    if (ragged) ICZ_CHECK_HIP(hipMemsetAsync(dG, 0, sizeof(float) * (size_t)(TB + B) * 4 * H, st));
    DropCfg off = {0, nullptr, nullptr, 0, 0};
    int cur = 0, nsx = 1, bnext = 0;
    for (int t = T - 1; t >= -1; --t) {       // t = -1: the image step
        const int bt = t >= 0 ? rows_t[t] : B;
        const size_t slot = (size_t)(t + 1) * B;      // gate / dG slot; state-after slot = slot + B, state-before slot = slot
        LstmBwdArgs a = {};
        a.dh_a = bnext ? X : nullptr; a.ns_a = nsx; a.lda_a = H; a.rows_a = bnext;
        a.dhdrop = t >= 0 ? dHd + (size_t)t * B * H : nullptr;
        a.dc_in = bnext ? dcb[cur] : nullptr; a.dc_in_rows = bnext;
        a.gates = tg + slot * 4 * H;
        a.c_prev = tc + slot * H; a.c_cur = tc + (slot + B) * H;
        a.dgates = dG + slot * 4 * H; a.dc_prev = dcb[cur ^ 1];
        a.rows = bt; a.H = H;
        // backward of a sampled rollout: a step behind the reference's break (NIC_Model.py:150) never ran -- zero d gates, no carry
        const int* const live = (eo && t > 0) ? nunf + (t - 1) : nullptr;
        a.live = live; a.carry_live = (eo && t >= 0 && t + 1 < T) ? nunf + t : nullptr;
        DropCfg d = t >= 0 ? nic_drop(d_seed, cur_train, rng.out_mask, sH, t) : off;
        hipLaunchKernelGGL(lstm_bwd_point_kernel, dim3(cdiv(H, 256), bt), dim3(256), 0, st, a, d);
        if (t >= 0) ICZ_TRY(nn(dG + slot * 4 * H, 4 * H, bt, 4 * H, P.w_hh, H, H, X, &nsx, STEP_WGS, st, live));   // d h_{t-1}
        bnext = bt;
        cur ^= 1;
    }
    // embedding gradient, image-feature gradient
    ICZ_TRY(nn(dG + (size_t)B * 4 * H, 4 * H, TB, 4 * H, P.w_ih, E, E, dEmb, nullptr, TARGET_WGS, st));
    ICZ_CHECK_HIP(embed_grad_launch(st, tok, TB, dEmb, 1, (size_t)0, temb, 1.0f, E, G.embed_weight, V, 0));
    if (dfeats) ICZ_TRY(nn(dG, 4 * H, B, 4 * H, P.w_ih, E, E, dfeats, nullptr, TARGET_WGS, st));
    // weight gradients
    ICZ_TRY(gemm_tn(dG + (size_t)B * 4 * H, 4 * H, 4 * H, temb, E, E, TB, G.w_ih, E, 0, nullptr, st));
    ICZ_TRY(gemm_tn(dG, 4 * H, 4 * H, cur_feats, E, E, B, G.w_ih, E, 1, nullptr, st));
    ICZ_TRY(gemm_tn(dG, 4 * H, 4 * H, th, H, H, TB + B, G.w_hh, H, 0, nullptr, st));
    ICZ_TRY(launch_colsum(dG, TB + B, 4 * H, 4 * H, G.b_ih, st));
    ICZ_CHECK_HIP(hipMemcpyAsync(G.b_hh, G.b_ih, sizeof(float) * 4 * H, hipMemcpyDeviceToDevice, st));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// ---- decoder seams (DecodeMember) ------------------------------------------------------------------------------------------------
// img_of_row null: the image step of the n_img images (k = 1, greedy); else every beam row starts from the image step of its image
// (features.expand(k, ...), NIC_Model.py:164), through the handle's expanded-feature rows
int Nic::prologue(const float* feats, int n_img, int k, const int32_t* img_of_row, hipStream_t st) {
    ICZ_REQUIRE(fresh, "nic: call icz_nic_refresh_weights after binding/updating parameters");
    if (!img_of_row) return image_step(feats, n_img * k, h[0], c[0], nullptr, st);
    const int rows = n_img * k;
    if (!feat_rows) {
        ICZ_TRY(alloc((void**)&feat_rows, sizeof(float) * (size_t)dims.max_rows * dims.E));
        ICZ_TRY(mem.synced());
    }
    hipLaunchKernelGGL(beam_expand_rows_kernel, dim3(cdiv(dims.E, 1024), rows), dim3(256), 0, st, feats, img_of_row, dims.E, feat_rows);
    return image_step(feat_rows, rows, h[0], c[0], nullptr, st);
}

int Nic::step(int rows, const int64_t* it_, const int32_t*, int, int cur, bool slabs, LogitsView* out, hipStream_t st) {
    DropCfg off = {0, nullptr, nullptr, 0, 0};
    int pns = 1;
    ICZ_TRY(token_step(rows, it_, seam_emb_ready, h[cur], c[cur], h[cur ^ 1], c[cur ^ 1], emb, nullptr, hdrop, logits, off, st, slabs ? &pns : nullptr,
                       seam_live));
    if (out) *out = logits_view(ws, P.predict_b, logits, rows, Vp, pns);
    return ICZ_OK;
}

void Nic::gather(const int32_t* src_row, int rows, int fan, hipStream_t st) {
    hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(dims.H, 1024), rows), dim3(256), 0, st, src_row, dims.H, h[1], c[1], h[1], c[1], h[0], c[0],
                       h[0], c[0], fan);
}

DecodeMember* nic_member(void* handle) { return static_cast<DecodeMember*>(reinterpret_cast<Nic*>(handle)); }

}  // namespace icz

// ================================================================================================
using namespace icz;
extern "C" {

int icz_nic_create(const icz_nic_dims* dims, icz_nic_t** out) { return abi_create<Nic>("icz_nic_create", dims, out); }
int icz_nic_destroy(icz_nic_t* h) { delete reinterpret_cast<Nic*>(h); return ICZ_OK; }
int icz_nic_bind_params(icz_nic_t* h, const icz_nic_params* p) {
    ICZ_REQUIRE(h && p, "icz_nic_bind_params: null argument");
    ICZ_TRY(check_param_table("icz_nic_bind_params", p, sizeof(*p)));
    Nic* n = reinterpret_cast<Nic*>(h);
    n->P = *p; n->bound = true; n->fresh = false;
    return ICZ_OK;
}
int icz_nic_refresh_weights(icz_nic_t* h, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Nic*>(h)->refresh((hipStream_t)stream);
}
int icz_nic_greedy(icz_nic_t* h, const float* features, int32_t B, int32_t max_len, int64_t* ids_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Nic*>(h)->greedy(features, B, max_len, ids_out, (hipStream_t)stream);
}
int icz_nic_sample(icz_nic_t* h, const float* features, int32_t B, int32_t max_len, const icz_rng* rng, int64_t* seq_out,
                   float* logprobs_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Nic*>(h)->sample(features, B, max_len, rng, seq_out, logprobs_out, (hipStream_t)stream);
}
int icz_nic_sample_n(icz_nic_t* h, const float* features, int32_t B, int32_t K, int32_t max_len, const icz_rng* rng, int64_t* seq_out,
                     float* logprobs_out, void* stream) {
    ICZ_REQUIRE(K >= 2 && K <= SAMPLE_N_MAX_K, "icz_nic_sample_n: K=%d samples per image outside 2..%d", K, SAMPLE_N_MAX_K);
    ICZ_REQUIRE(h, "icz_nic_sample_n: null handle");
    return reinterpret_cast<Nic*>(h)->sample_n(features, B, K, max_len, rng, seq_out, logprobs_out, (hipStream_t)stream);
}
int icz_nic_sample_backward(icz_nic_t* h, const float* reward, const icz_nic_params* grads, float* dfeatures_out, float* loss_out,
                            float* mask_sum_out, float mask_sum_global, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::ROLLOUT, "nic", "nic sample_backward"};
    hd.rollout = {reward, nullptr, loss_out, nullptr, mask_sum_out};
    hd.norm_global = mask_sum_global;
    return reinterpret_cast<Nic*>(h)->backward(hd, grads, dfeatures_out, (hipStream_t)stream);
}
// sample_backward with an SCST objective (scst_objective.hip) in the place of RewardCriterion
int icz_nic_sample_backward_objective(icz_nic_t* h, const icz_scst_objective* obj, const icz_nic_params* grads, float* dfeatures_out,
                                      float* loss_out3, float* ent_out, float* mask_sum_out, float mask_sum_global, void* stream) {
    ScstObjective o;
    ICZ_TRY(icz::scst_objective_args("icz_nic_sample_backward_objective", obj, obj ? obj->K : 1, 1, &o));
    ICZ_REQUIRE(grads && loss_out3, "icz_nic_sample_backward_objective: null argument");
    ICZ_REQUIRE(h, "icz_nic_sample_backward_objective: null handle");
    LossHead hd = {LossHead::ROLLOUT, "nic", "nic sample_backward_objective"};
    hd.rollout = {nullptr, &o, loss_out3, ent_out, mask_sum_out};
    hd.objective = obj;
    hd.norm_global = mask_sum_global;
    return reinterpret_cast<Nic*>(h)->backward(hd, grads, dfeatures_out, (hipStream_t)stream);
}
int icz_nic_set_scheduled_sampling(icz_nic_t* h, float ss_prob, const float* gate_uniforms, const float* draw_uniforms) {
    return set_scheduled_sampling("icz_nic_set_scheduled_sampling", reinterpret_cast<Nic*>(h), ss_prob, gate_uniforms, draw_uniforms);
}
int icz_nic_xe_forward(icz_nic_t* h, const float* features, const int64_t* captions, int32_t B, int32_t L, const int32_t* lengths_host,
                       const icz_rng* rng, int32_t train, float* packed_logits_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Nic*>(h)->xe_forward(features, captions, B, L, lengths_host, rng, train, packed_logits_out, (hipStream_t)stream);
}
int icz_nic_set_option(icz_nic_t* h, const char* name, int32_t value) {
    ICZ_REQUIRE(h && name, "icz_nic_set_option: null argument");
    if (strcmp(name, "early_out") == 0) { reinterpret_cast<Nic*>(h)->early_out = value != 0; return ICZ_OK; }
    set_error("icz_nic_set_option: unknown option '%s'", name);
    return ICZ_ERR_INVALID;
}
int icz_nic_set_norm_global(icz_nic_t* h, const float* norm_dev, void* stream) {
    return set_norm_global("icz_nic_set_norm_global", reinterpret_cast<Nic*>(h), norm_dev, stream);
}
int icz_nic_xe_backward(icz_nic_t* h, float smoothing, const icz_nic_params* grads, float* dfeatures_out, float* loss_out,
                        float n_tokens_global, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::XE, "nic", "nic xe_backward"};
    hd.smoothing = smoothing; hd.loss_out = loss_out; hd.norm_global = n_tokens_global;
    return reinterpret_cast<Nic*>(h)->backward(hd, grads, dfeatures_out, (hipStream_t)stream);
}
int icz_nic_xe_backward_distill(icz_nic_t* h, const icz_distill_opts* opts, const icz_nic_params* grads, float* dfeatures_out,
                                float* loss_out3, float n_tokens_global, void* stream) {
    Nic* n = reinterpret_cast<Nic*>(h);
    DistillArgs a;
    ICZ_TRY(distill_args("icz_nic_xe_backward_distill", opts, n ? n->dims.V : -1, &a));
    ICZ_REQUIRE(grads && loss_out3, "icz_nic_xe_backward_distill: null grads or loss");
    ICZ_REQUIRE(h, "icz_nic_xe_backward_distill: null handle");
    LossHead hd = {LossHead::XE_DISTILL, "nic", "nic xe_backward_distill"};
    hd.distill = &a; hd.loss_out = loss_out3; hd.norm_global = n_tokens_global;
    return n->backward(hd, grads, dfeatures_out, (hipStream_t)stream);
}
int icz_nic_xe_backward_swor(icz_nic_t* h, const icz_swor_opts* opts, int32_t rows, const icz_nic_params* grads, float* dfeatures_out,
                             float* loss_out, void* stream) {
    SworArgs a;
    ICZ_TRY(swor_args("icz_nic_xe_backward_swor", opts, rows, &a));
    ICZ_REQUIRE(grads && loss_out, "icz_nic_xe_backward_swor: null grads or loss");
    ICZ_REQUIRE(h, "icz_nic_xe_backward_swor: null handle");
    LossHead hd = {LossHead::XE_SWOR, "nic", "nic xe_backward_swor"};
    hd.swor = &a; hd.swor_rows = rows; hd.loss_out = loss_out;
    return reinterpret_cast<Nic*>(h)->backward(hd, grads, dfeatures_out, (hipStream_t)stream);
}
// xe_backward driven by an upstream gradient w.r.t. the packed logits
int icz_nic_xe_backward_dlogits(icz_nic_t* h, const float* dpacked, const icz_nic_params* grads, float* dfeatures_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::XE_DLOGITS, "nic", "nic xe_backward_dlogits"};
    hd.upstream = dpacked;
    return reinterpret_cast<Nic*>(h)->backward(hd, grads, dfeatures_out, (hipStream_t)stream);
}
}  // extern "C"
