// BUTD decoder: handle, launch sequences and C ABI (include/icz.h).  gfx950 only.
#include <vector>

#include "butd_impl.h"
#include "butd_kernels.h"
#include "lstm_kernels.h"
#include "support_kernels.h"
#include "token_kernels.h"

namespace icz {

// ------------------------------------------------------------------------------------------------
int Butd::init(const icz_butd_dims& d, int r_max) {
    dims = d;
    ICZ_REQUIRE(d.R > 0 && d.R <= r_max, "butd: R=%d must be in 1..%d (36 boxes / 49 grid cells; icz_butd_create_regions: adaptive sets, up to %d)",
                d.R, r_max, ATT_MAX_R);
    cur_R = d.R;
    ICZ_REQUIRE(d.D % 4 == 0 && d.H % 4 == 0 && d.E % 4 == 0 && d.A % 4 == 0, "butd: D,H,E,A must be multiples of 4");
    ICZ_REQUIRE(d.V > 3 && d.max_rows > 0 && d.max_len > 0, "butd: bad V/max_rows/max_len");
    const size_t rows = d.max_rows, H = d.H, D = d.D, E = d.E, A = d.A, V = d.V, R = d.R;
    ICZ_TRY(alloc((void**)&w_enc, sizeof(float) * A * D));
    ICZ_TRY(alloc((void**)&w_dec, sizeof(float) * A * H));
    ICZ_TRY(alloc((void**)&w_aff, sizeof(float) * A));
    const size_t Vp = pad_vocab(d.V);           // padded rows stay zero: the dgrad GEMM reads K = Vp rows
    ICZ_TRY(alloc((void**)&w_pred, sizeof(float) * Vp * H));
    ICZ_TRY(alloc((void**)&n_enc, sizeof(float) * A));
    ICZ_TRY(alloc((void**)&n_dec, sizeof(float) * A));
    ICZ_TRY(alloc((void**)&n_aff, sizeof(float) * 4));
    ICZ_TRY(alloc((void**)&n_pred, sizeof(float) * V));
    ICZ_TRY(alloc((void**)&mean, sizeof(float) * rows * D));
    ICZ_TRY(alloc((void**)&premean, sizeof(float) * rows * 4 * H));
    ICZ_TRY(alloc((void**)&enc_ctx, sizeof(float) * rows * R * A));
    for (int i = 0; i < 2; ++i) {
        ICZ_TRY(alloc((void**)&h1[i], sizeof(float) * rows * H));
        ICZ_TRY(alloc((void**)&c1[i], sizeof(float) * rows * H));
        ICZ_TRY(alloc((void**)&h2[i], sizeof(float) * rows * H));
        ICZ_TRY(alloc((void**)&c2[i], sizeof(float) * rows * H));
    }
    ICZ_TRY(alloc((void**)&emb, sizeof(float) * rows * E));
    ICZ_TRY(alloc((void**)&ctx, sizeof(float) * rows * D));
    ICZ_TRY(alloc((void**)&scores, sizeof(float) * rows * R));
    ICZ_TRY(alloc((void**)&alpha, sizeof(float) * rows * R));
    ICZ_TRY(alloc((void**)&h2drop, sizeof(float) * rows * H));
    ICZ_TRY(alloc((void**)&logits, sizeof(float) * rows * Vp));      // rows padded to Vp: 16-byte aligned rows
    ICZ_TRY(alloc((void**)&amax_val, sizeof(float) * rows * ARGMAX_PARTS));
    ICZ_TRY(alloc((void**)&amax_idx, sizeof(int) * rows * ARGMAX_PARTS));
    ICZ_TRY(alloc((void**)&it, sizeof(int64_t) * rows));
    ICZ_TRY(alloc_scalars(mem));
    size_t nmax = 4 * H;
    if (A > nmax) nmax = A;
    if (V > nmax) nmax = V;
    ws_floats = (size_t)TARGET_WGS * 4096 * 2 + rows * nmax;
    {   // the resident decoder-step GEMMs leave one slab per 256-deep k range: (2H + max(E, D)) / 256 slabs of rows x 4H at up to 128 rows
        const size_t kmax = 2 * H + (E > D ? E : D), r128 = rows < 128 ? rows : 128;
        const size_t need = (kmax / 256 + 1) * r128 * 4 * H;
        if (need > ws_floats) ws_floats = need;
    }
    ICZ_TRY(alloc((void**)&ws, sizeof(float) * ws_floats));
    ICZ_TRY(mem.synced());
    // defaults of the options "early_out" / "fused_dh1" / "merge_small" from the environment (A/B runs of whole programs; icz_butd_set_option overrides)
    if (const char* e = getenv("ICZ_EARLY_OUT")) early_out = atoi(e) != 0;
    if (const char* e = getenv("ICZ_BPTT_FUSED_DH1")) fused_dh1 = atoi(e) != 0;
    if (const char* e = getenv("ICZ_MERGE_SMALL")) { const int n = atoi(e); if (n >= 0 && n <= 32) merge_small = n; }
    return ICZ_OK;
}

// ------------------------------------------------------------------------------------------------
int Butd::refresh(hipStream_t st) {
    ICZ_REQUIRE(bound, "butd: parameters not bound");
    const int A = dims.A, D = dims.D, H = dims.H, V = dims.V;
    WeightNormTable wt = {};
    int nb = 0;
    auto add = [&](const float* v, const float* g, float* w, float* norm, int rows, int cols) {
        wt.j[wt.count++] = {v, g, w, norm, rows, cols, nb};
        nb += cdiv(rows, 4);
    };
    add(P.enc_att_v, P.enc_att_g, w_enc, n_enc, A, D);
    add(P.dec_att_v, P.dec_att_g, w_dec, n_dec, A, H);
    add(P.affine_v, P.affine_g, w_aff, n_aff, 1, A);
    add(P.predict_v, P.predict_g, w_pred, n_pred, V, H);
    hipLaunchKernelGGL(weight_norm_multi_kernel, dim3(nb), dim3(256), 0, st, wt);
    ICZ_CHECK_HIP(hipGetLastError());
    fresh = true;
    wt_fresh = false;       // the transposed copies (117 MB) are rebuilt by the first backward pass that follows, outside its captured
    return ICZ_OK;          // graph (Butd::backward: bptt_prelude): evaluation loops refresh per batch and never read them
}

// the transposed copies serve 33..64-row dgrad steps through gemm_resident_x3: K = 4H in whole k ranges, N = D + H / H wide enough
bool Butd::wt_possible() const {
    const GemmSeg s = {w_enc, w_enc, 4 * dims.H, 4 * dims.H, 4 * dims.H};       // placeholders: only the shape is looked at
    const GemmArgs g = gemm_args({s}, 64, dims.D + dims.H, nullptr, 0);
    const GemmArgs p = gemm_args({s, s}, 64, dims.H, nullptr, 0), q = gemm_args({s}, 64, dims.H, nullptr, 0);
    return dims.H % 64 == 0 && dims.D % 64 == 0 && gemm_resident_x3_fits(g) && gemm_resident_x3_pair_fits(p, q);
}

int Butd::refresh_transposes(hipStream_t st) {
    ICZ_REQUIRE(bound && wt_lm_ih, "butd: no transposed weight buffers");
    const int H = dims.H, D = dims.D, E = dims.E;
    TransposeTable tt = {};
    int nb = 0;
    auto add = [&](const float* src, int ld, int cols, float* dst) {
        tt.j[tt.count++] = {src, ld, 4 * H, cols, dst, nb};
        nb += (4 * H / 64) * (cols / 64);
    };
    add(P.lm_w_ih, D + H, D + H, wt_lm_ih);
    add(P.lm_w_hh, H, H, wt_lm_hh);
    add(P.td_w_ih, H + D + E, H, wt_td_ih_h2);          // the h2 columns only: mean features and embedding have no recurrent gradient
    add(P.td_w_hh, H, H, wt_td_hh);
    hipLaunchKernelGGL(transpose_multi_kernel, dim3(nb), dim3(256), 0, st, tt);
    ICZ_CHECK_HIP(hipGetLastError());
    wt_fresh = true;
    return ICZ_OK;
}

// generic "y = x W^T + bias" into g.out, with automatic split-K through the workspace (the split is fitted to it: the capacity
// check of gemm_finished cannot fail here)
int Butd::gemm_nt(GemmArgs& g, const float* bias, hipStream_t st) {
    return gemm_finished(GEMM_NT, g, split_forward(TARGET_WGS), bias, ws, ws_floats, st, "butd");
}

// Once per batch of images (K0 in SURVEY.md 2.3): mean features, the time-invariant part of the TD-LSTM gates
// (mean . W_ih[:, H:H+D]^T) and enc_att(feats) -- the reference recomputes the latter every step (:57).
int Butd::prologue(const float* feats, int n_img, hipStream_t st) {
    const int R = cur_R, D = dims.D, H = dims.H, E = dims.E, A = dims.A;
    ICZ_REQUIRE(fresh, "butd: call icz_butd_refresh_weights after binding/updating parameters");
    ICZ_REQUIRE(n_img > 0 && n_img <= dims.max_rows, "butd: %d images exceed capacity %d", n_img, dims.max_rows);
    ICZ_TRY(check_counts(n_img));
    launch_mean_feats(feats, mean, n_img, R, D, cnt, st);
    {   // premean = mean . W_ih[:, H:H+D]^T   [n_img, 4H]
        GemmArgs g = gemm_args({{mean, P.td_w_ih + H, D, H + D + E, D}}, n_img, 4 * H, premean, 4 * H);
        ICZ_TRY(gemm_nt(g, nullptr, st));
    }
    {   // enc_ctx = feats . w_enc^T + b_enc   [n_img*R, A]  (over the padded rows too: the counted kernels never read those of enc_ctx)
        GemmArgs g = gemm_args({{feats, w_enc, D, D, D}}, n_img * R, A, enc_ctx, A);
        ICZ_TRY(gemm_nt(g, P.enc_att_b, st));
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// One decoder step (:172-182) for `rows` decoder rows.  State is read from s.*_in and written to s.*_out.
int Butd::step(const StepIO& s, hipStream_t st) {
    const int R = cur_R, D = dims.D, H = dims.H, E = dims.E, A = dims.A, V = dims.V;
    const int Vp = pad_vocab(V);
    const int rows = s.rows;
    const bool ad = adaptive();
    float* const ws = s.ws_alt ? s.ws_alt : this->ws;
    float* const scores = s.scores_alt ? s.scores_alt : this->scores;
    DropCfg off = {0, nullptr, nullptr, 0, 0};
    // embedding -> relu -> dropout (greedy decode gets it from the previous step's fused argmax epilogue)
    if (!s.emb_ready)
        hipLaunchKernelGGL(embed_kernel, dim3(cdiv(E, 1024), rows), dim3(256), 0, st, P.embed_weight, s.it, s.emb_out ? s.emb_out : emb, rows, E, s.drop_emb);
    const float* embp = s.emb_out ? s.emb_out : emb;
    const size_t ws_cap = s.ws_alt ? (tb.xfloats < ws_floats ? tb.xfloats : ws_floats) : ws_floats;      // ws_alt = tb.X[0]
    // the gates of an LSTM as slabs [ns][rows][4H] in the chain's workspace (one slab: the dense product); the split is fitted to it
    auto gates = [&](GemmArgs g, int* ns) -> int {
        ICZ_REQUIRE((size_t)rows * 4 * H <= ws_cap, "butd: workspace too small");
        return gemm_slabs(GEMM_NT, g, split_forward(STEP_WGS), ws, ws_cap, ns, st, "butd");
    };
    int ns;
    {   // TD-attention LSTM: [h2, mean, emb] W_ih^T + h1 W_hh^T  (mean part hoisted into premean)
        ICZ_TRY(gates(gemm_args({{s.h2_in, P.td_w_ih, H, H + D + E, H}, {embp, P.td_w_ih + H + D, E, H + D + E, E}, {s.h1_in, P.td_w_hh, H, H, H}},
                                rows, 4 * H, ws, 4 * H, s.live), &ns));
        LstmPointArgs a = {ws, ns, premean, s.img_of_row, P.td_b_ih, P.td_b_hh, s.c1_in, s.h1_out, s.c1_out, s.gates_td_out, nullptr, rows, H, s.live};
        kprof_mark(KP_LSTM_POINT, true, st);
        launch_lstm_point(a, off, st);
        kprof_mark(KP_LSTM_POINT, false, st);
    }
    {   // attention
        kprof_mark(KP_ATTENTION, true, st);
        GemmArgs g = gemm_args({{s.h1_out, w_dec, H, H, H}}, rows, A, ws, A, s.live);
        ns = gemm_pick_split(g, STEP_WGS);
        ICZ_TRY(gemm_slabs(GEMM_NT, g, ns, ws, ws_cap, st, "butd"));
        AttScoreArgs a = {enc_ctx, s.img_of_row, ws, ns, P.dec_att_b, w_aff, P.affine_b, s.dec_ctx_out, scores, rows, R, A, s.live, cnt};
        const int G = s.rows_per_img;
        // compare the accumulation order: the per-row kernel sums a region row in the lane order of three regions at a time, the
        // grouped one region by region -- identical per (row, region): a wave's lanes cover the same columns in the same order
        const bool grouped = G > 1 && att_scores_group_fits(rows, G, A);
        // (the <true> instances: per-image counts or more than 64 regions, Butd::adaptive)
        // grouped without dropout and early-out: beam search; grouped with them: the multi-sample rollout (sample_n)
        launch_att_scores(!grouped ? ATT_PER_ROW : (s.drop_att.mode == 0 && !s.live ? ATT_GROUP : ATT_GROUP_TRAIN), ad, a, s.drop_att, G, ATT_PARTS, st);
        const bool ctx_grouped = G > 1 && G <= ATT_CTX_MAX_G && rows % G == 0 && !s.alpha_out2;
        launch_att_ctx(ad, s.feats, s.img_of_row, scores, s.alpha_out ? s.alpha_out : alpha, s.alpha_out2, s.alpha2_stride, s.ctx_out ? s.ctx_out : ctx,
                       rows, R, D, ctx_grouped ? G : 0, s.live, cnt, st);
        kprof_mark(KP_ATTENTION, false, st);
    }
    const float* ctxp = s.ctx_out ? s.ctx_out : ctx;
    {   // language LSTM: [ctx, h1] W_ih^T + h2 W_hh^T
        ICZ_TRY(gates(gemm_args({{ctxp, P.lm_w_ih, D, D + H, D}, {s.h1_out, P.lm_w_ih + D, H, D + H, H}, {s.h2_in, P.lm_w_hh, H, H, H}},
                                rows, 4 * H, ws, 4 * H, s.live), &ns));
        LstmPointArgs a = {ws, ns, nullptr, nullptr, P.lm_b_ih, P.lm_b_hh, s.c2_in, s.h2_out, s.c2_out, s.gates_lm_out,
                           s.h2drop_out ? s.h2drop_out : h2drop, rows, H, s.live};
        launch_lstm_point(a, s.drop_out, st);
    }
    if (!s.skip_predict) {   // predict: logits = drop(h2) w_pred^T + b  (finished logits, or split-K slabs in the chain's workspace for a consumer that sums them)
        ICZ_TRY(gemm_predict(s.h2drop_out ? s.h2drop_out : h2drop, H, w_pred, P.predict_b, rows, V, Vp, s.logits_out ? s.logits_out : logits,
                             s.logits_ld ? s.logits_ld : Vp, ws, ws_cap, s.pred_nsplit, st, s.live));
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int Butd::zero_state(int rows, int which, hipStream_t st) {
    ZeroList z = {{h1[which], c1[which], h2[which], c2[which]}, 4};
    const size_t n = (size_t)rows * dims.H;
    hipLaunchKernelGGL(zero_bufs_kernel, dim3(cdiv((int)(n / 4), 256)), dim3(256), 0, st, z, n);
    return ICZ_OK;
}

int Butd::greedy(const float* feats, int B, int max_len, int64_t* ids_out, float* alphas_out, hipStream_t st) {
    ICZ_REQUIRE(feats && ids_out && B > 0 && B <= dims.max_rows && max_len > 0, "butd greedy: bad arguments");
    ICZ_REQUIRE(fresh, "butd: call icz_butd_refresh_weights after binding/updating parameters");
    ICZ_TRY(check_counts(B));
    if (!graphs_on()) return greedy_impl(feats, B, max_len, ids_out, alphas_out, st);
    const std::vector<uintptr_t> key = {1, (uintptr_t)feats, (uintptr_t)B, (uintptr_t)max_len, (uintptr_t)ids_out, (uintptr_t)alphas_out, opt_bits()};
    return gc.run(key, st, [&](hipStream_t s) { return greedy_impl(feats, B, max_len, ids_out, alphas_out, s); });
}

int Butd::greedy_impl(const float* feats, int B, int max_len, int64_t* ids_out, float* alphas_out, hipStream_t st) {
    ICZ_TRY(prologue(feats, B, st));
    return greedy_chain(feats, B, max_len, ids_out, alphas_out, st);
}

// the decode loop after the per-image prologue
// scst = true (the baseline of an SCST step, rollouts_impl): the chain keeps count of the rows that have not emitted <end> yet and,
// once there is none, the kernels of the remaining steps return at entry (ids = 0 there).  The reference's greedy loop has no break
// (BUTD_Model.py:171-186), but nothing behind a row's <end> reaches the reward (Utils.py:354 cuts there): the SCST step's results
// are the same.  icz_butd_greedy (evaluation, `sampler`) never does this: its ids are the reference's in every column.
int Butd::greedy_chain(const float* feats, int B, int max_len, int64_t* ids_out, float* alphas_out, hipStream_t st, bool scst) {
    ICZ_TRY(zero_state(B, 0, st));
    int* const gn = (scst && early_out && gnunf && tb.T >= max_len && tb.B >= B) ? gnunf : nullptr;
    hipLaunchKernelGGL(greedy_init_kernel, dim3(cdiv(B > max_len ? B : max_len, 256)), dim3(256), 0, st, it, B, gn, max_len);   // <sta>
    int cur = 0;
    const int Vp = pad_vocab(dims.V);
    bool track = false;
    for (int t = 0; t < max_len; ++t) {
        StepIO s = {};
        s.rows = B; s.feats = feats; s.it = it;
        s.emb_ready = t > 0;           // produced by the previous step's embed_argmax_kernel
        s.h1_in = h1[cur]; s.c1_in = c1[cur]; s.h2_in = h2[cur]; s.c2_in = c2[cur];
        s.h1_out = h1[cur ^ 1]; s.c1_out = c1[cur ^ 1]; s.h2_out = h2[cur ^ 1]; s.c2_out = c2[cur ^ 1];
        if (alphas_out) { s.alpha_out2 = alphas_out + (size_t)t * cur_R; s.alpha2_stride = max_len * cur_R; }
        int pns = 1;
        s.pred_nsplit = &pns;
        if (track && t > 0) s.live = gn + (t - 1);
        ICZ_TRY(step(s, st));
        if (t == 0) track = gn && pns > 1;     // the one-launch select below keeps the count (the two-kernel argmax of <= 32 rows does not)
        kprof_mark(KP_GREEDY_SELECT, true, st);
        launch_greedy_select(logits_view(ws, P.predict_b, logits, B, Vp, pns), emb_slot(), B, dims.V, amax_val, amax_idx, it, ids_out, max_len, t,
                             track ? gunf : nullptr, track ? gn : nullptr, st);
        kprof_mark(KP_GREEDY_SELECT, false, st);
        cur ^= 1;
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// ---- decoder seams (DecodeMember) ------------------------------------------------------------------------------------------------
// the per-image prologue, then k zeroed state rows per image
int Butd::prologue(const float* feats, int n_img, int k, const int32_t*, hipStream_t st) {
    ICZ_TRY(prologue(feats, n_img, st));
    seam_feats = feats;
    return zero_state(n_img * k, 0, st);
}

int Butd::step(int rows, const int64_t* it_, const int32_t* img_of_row, int rows_per_img, int cur, bool slabs, LogitsView* out,
               hipStream_t st) {
    StepIO s = {};
    s.rows = rows; s.feats = seam_feats; s.img_of_row = img_of_row; s.it = it_;
    s.rows_per_img = rows_per_img;
    s.emb_ready = seam_emb_ready; s.live = seam_live;
    s.h1_in = h1[cur]; s.c1_in = c1[cur]; s.h2_in = h2[cur]; s.c2_in = c2[cur];
    s.h1_out = h1[cur ^ 1]; s.c1_out = c1[cur ^ 1]; s.h2_out = h2[cur ^ 1]; s.c2_out = c2[cur ^ 1];
    int pns = 1;
    if (slabs) s.pred_nsplit = &pns;
    ICZ_TRY(step(s, st));
    if (out) *out = logits_view(ws, P.predict_b, logits, rows, pad_vocab(dims.V), pns);
    return ICZ_OK;
}

void Butd::gather(const int32_t* src_row, int rows, int fan, hipStream_t st) {
    hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(dims.H, 1024), rows), dim3(256), 0, st, src_row, dims.H, h1[1], c1[1], h2[1], c2[1],
                       h1[0], c1[0], h2[0], c2[0], fan);
}

DecodeMember* butd_member(void* handle) { return static_cast<DecodeMember*>(reinterpret_cast<Butd*>(handle)); }

}  // namespace icz

// ================================================================================================
using namespace icz;

extern "C" {

int icz_butd_create(const icz_butd_dims* dims, icz_butd_t** out) { return abi_create<Butd>("icz_butd_create", dims, out); }

// a handle whose dims.R is a region capacity of up to ATT_MAX_R (icz_butd_create keeps its bound of 64)
int icz_butd_create_regions(const icz_butd_dims* dims, icz_butd_t** out) {
    ICZ_REQUIRE(dims && out, "icz_butd_create_regions: null argument");
    Butd* h = new Butd();
    const int s = h->init(*dims, ATT_MAX_R);
    if (s != ICZ_OK) { delete h; return s; }
    *out = reinterpret_cast<icz_butd_t*>(h);
    return ICZ_OK;
}

int icz_butd_destroy(icz_butd_t* h) {
    delete reinterpret_cast<Butd*>(h);
    return ICZ_OK;
}

int icz_butd_bind_params(icz_butd_t* h, const icz_butd_params* p) {
    ICZ_REQUIRE(h && p, "icz_butd_bind_params: null argument");
    ICZ_TRY(check_param_table("icz_butd_bind_params", p, sizeof(*p), (1u << 16) | (1u << 17)));
    Butd* b = reinterpret_cast<Butd*>(h);
    // the captured graphs carry the old parameter pointers in their kernel arguments (embed_weight, the LSTM weights and
    // biases ...): a rebind to other tensors must not replay them
    if (b->bound && memcmp(&b->P, p, sizeof(*p)) != 0) {
        ICZ_CHECK_HIP(hipDeviceSynchronize());
        b->gc.clear();
    }
    b->P = *p;
    b->bound = true;
    b->fresh = false;
    return ICZ_OK;
}

int icz_butd_set_option(icz_butd_t* h, const char* name, int32_t value) {
    ICZ_REQUIRE(h && name, "icz_butd_set_option: null argument");
    Butd* b = reinterpret_cast<Butd*>(h);
    if (strcmp(name, "graphs") == 0) { b->use_graphs = value != 0; return ICZ_OK; }
    if (strcmp(name, "concurrent") == 0) { b->concurrent = value != 0; return ICZ_OK; }
    if (strcmp(name, "early_out") == 0) { b->early_out = value != 0; return ICZ_OK; }
    if (strcmp(name, "small_nt") == 0) { b->small_nt = value != 0; return ICZ_OK; }
    if (strcmp(name, "fused_dh1") == 0) { b->fused_dh1 = value != 0; return ICZ_OK; }
    if (strcmp(name, "group_att") == 0) { b->group_att = value != 0; return ICZ_OK; }
    if (strcmp(name, "merge_small") == 0) {
        ICZ_REQUIRE(value >= 0 && value <= 32, "icz_butd_set_option: merge_small %d outside 0..32", value);
        b->merge_small = value;
        return ICZ_OK;
    }
    set_error("icz_butd_set_option: unknown option '%s'", name);
    return ICZ_ERR_INVALID;
}

int icz_butd_set_mask_sum_global(icz_butd_t* h, const float* mask_sum_global_dev, void* stream) {
    return set_norm_global("icz_butd_set_mask_sum_global", reinterpret_cast<Butd*>(h), mask_sum_global_dev, stream);
}

int icz_butd_set_grad_callback(icz_butd_t* h, icz_grad_ready_cb cb, void* user) {
    ICZ_REQUIRE(h, "null handle");
    Butd* b = reinterpret_cast<Butd*>(h);
    b->grad_cb = cb; b->grad_cb_user = user;
    return ICZ_OK;
}

int icz_butd_refresh_weights(icz_butd_t* h, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Butd*>(h)->refresh((hipStream_t)stream);
}

int icz_butd_set_regions(icz_butd_t* h, int32_t regions, const int32_t* counts_dev, const int32_t* counts_host, int32_t n_img) {
    ICZ_REQUIRE(h, "null handle");
    Butd* b = reinterpret_cast<Butd*>(h);
    ICZ_REQUIRE(regions >= 1 && regions <= b->dims.R, "icz_butd_set_regions: %d regions outside 1..%d (the handle's capacity)", regions, b->dims.R);
    ICZ_REQUIRE((counts_dev == nullptr) == (counts_host == nullptr), "icz_butd_set_regions: pass the counts on both sides or on neither");
    if (counts_host) {
        ICZ_REQUIRE(n_img >= 1 && n_img <= b->dims.max_rows, "icz_butd_set_regions: %d images out of range", n_img);
        for (int i = 0; i < n_img; ++i)
            ICZ_REQUIRE(counts_host[i] >= 1 && counts_host[i] <= regions, "icz_butd_set_regions: image %d has %d regions (1..%d)", i, counts_host[i], regions);
    }
    b->cur_R = regions; b->cnt = counts_dev; b->cnt_n = counts_dev ? n_img : 0;
    b->mode = 0;         // a stored forward pass was laid out with the previous stride
    return ICZ_OK;
}

int icz_butd_greedy(icz_butd_t* h, const float* feats, int32_t B, int32_t max_len, int64_t* ids_out,
                    float* alphas_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Butd*>(h)->greedy(feats, B, max_len, ids_out, alphas_out, (hipStream_t)stream);
}

int icz_butd_step(icz_butd_t* h, const float* feats, int32_t B, const int64_t* it, float* h1, float* c1,
                  float* h2, float* c2, float* ctx_out, float* alpha_out, float* logits_out, void* stream) {
    ICZ_REQUIRE(h && feats && it && h1 && c1 && h2 && c2 && logits_out, "icz_butd_step: null argument");
    Butd* b = reinterpret_cast<Butd*>(h);
    hipStream_t st = (hipStream_t)stream;
    ICZ_REQUIRE(B > 0 && B <= b->dims.max_rows, "icz_butd_step: B out of range");
    ICZ_TRY(b->prologue(feats, B, st));
    StepIO s = {};
    s.rows = B; s.feats = feats; s.it = it;
    s.h1_in = h1; s.c1_in = c1; s.h2_in = h2; s.c2_in = c2;
    // in-place update is safe: every consumer of *_in has been launched before the kernel that overwrites it
    // only if input/output buffers differ, so run into the handle's buffers and copy back.
    s.h1_out = b->h1[0]; s.c1_out = b->c1[0]; s.h2_out = b->h2[0]; s.c2_out = b->c2[0];
    s.ctx_out = ctx_out; s.alpha_out = alpha_out; s.logits_out = logits_out; s.logits_ld = b->dims.V;
    ICZ_TRY(b->step(s, st));
    const size_t n = sizeof(float) * B * b->dims.H;
    ICZ_CHECK_HIP(hipMemcpyAsync(h1, b->h1[0], n, hipMemcpyDeviceToDevice, st));
    ICZ_CHECK_HIP(hipMemcpyAsync(c1, b->c1[0], n, hipMemcpyDeviceToDevice, st));
    ICZ_CHECK_HIP(hipMemcpyAsync(h2, b->h2[0], n, hipMemcpyDeviceToDevice, st));
    ICZ_CHECK_HIP(hipMemcpyAsync(c2, b->c2[0], n, hipMemcpyDeviceToDevice, st));
    return ICZ_OK;
}

}  // extern "C"
