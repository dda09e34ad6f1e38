// BUTD training paths: sample_rl rollout + REINFORCE backward, teacher-forced XE forward + backward.
// Both share one BPTT (Butd::bptt): per-step dgrad GEMMs (NN) and pointwise kernels run sequentially in
// reverse time; every weight gradient is one batched GEMM (TN) over all (time, row) pairs at the end.
#include <math.h>

#include "butd_impl.h"
#include "butd_kernels.h"
#include "ens_sample.h"
#include "lstm_kernels.h"
#include "support_kernels.h"
#include "token_kernels.h"

namespace icz {

__global__ void sample_init_kernel(uint8_t* unf, int* nunf, int64_t* tok, int B, int T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) { unf[i] = 1; tok[i] = 1; }
    if (i < T) nunf[i] = 0;
}

int Butd::ensure_train(int B, int T) {
    if (tb.B >= B && tb.T >= T) return ICZ_OK;
    ICZ_REQUIRE(B <= 2 * dims.max_rows, "butd: batch %d exceeds capacity %d", B, dims.max_rows);      // (2 x: the merged chain of a small SCST batch)
    ICZ_REQUIRE(T <= XE_MAX_T, "butd: %d steps exceed the limit of %d", T, XE_MAX_T);
    // Sized by what the batches ask for, not by the handle's row capacity (which also covers images x beam rows): the
    // reference never truncates captions (Datasets.py:47-51), so the step count of an XE batch is only known when it
    // arrives.  Growing re-allocates everything: the rollout / XE activations kept for a pending backward are lost (callers
    // run forward and backward of one batch back to back) and every captured graph holds stale addresses.
    if (tb.B > B) B = tb.B;
    if (tb.T > T) T = tb.T;
    if (dims.max_len > T) T = dims.max_len;
    if (!mem.training.empty()) {
        ICZ_TRY(mem.release_training(&gc));
        tb = TrainBuf();
        drop_loss_buffers();
    }
    if (!wt_lm_ih && wt_possible()) {      // permanent (not re-allocated when the training buffers grow)
        const size_t G4 = 4 * (size_t)dims.H;
        ICZ_TRY(alloc((void**)&wt_lm_ih, sizeof(float) * G4 * (dims.D + dims.H)));
        ICZ_TRY(alloc((void**)&wt_lm_hh, sizeof(float) * G4 * dims.H));
        ICZ_TRY(alloc((void**)&wt_td_ih_h2, sizeof(float) * G4 * dims.H));
        ICZ_TRY(alloc((void**)&wt_td_hh, sizeof(float) * G4 * dims.H));
        wt_fresh = false;
    }
    DeviceBuffers::TrainingScope scope(mem);
    const size_t H = dims.H, D = dims.D, E = dims.E, A = dims.A, R = dims.R, V = dims.V;
    const size_t Vp = pad_vocab(dims.V);
    const size_t TB = (size_t)T * B;
    ICZ_TRY(alloc((void**)&tb.tok, sizeof(int64_t) * (TB + B)));
    ICZ_TRY(alloc((void**)&tb.emb, sizeof(float) * TB * E));
    ICZ_TRY(alloc((void**)&tb.h1, sizeof(float) * (TB + B) * H));
    ICZ_TRY(alloc((void**)&tb.c1, sizeof(float) * (TB + B) * H));
    ICZ_TRY(alloc((void**)&tb.h2, sizeof(float) * (TB + B) * H));
    ICZ_TRY(alloc((void**)&tb.c2, sizeof(float) * (TB + B) * H));
    ICZ_TRY(alloc((void**)&tb.gtd, sizeof(float) * TB * 4 * H));
    ICZ_TRY(alloc((void**)&tb.glm, sizeof(float) * TB * 4 * H));
    ICZ_TRY(alloc((void**)&tb.dec, sizeof(float) * TB * A));
    ICZ_TRY(alloc((void**)&tb.alpha, sizeof(float) * TB * R));
    ICZ_TRY(alloc((void**)&tb.ctx, sizeof(float) * TB * D));
    ICZ_TRY(alloc((void**)&tb.h2d, sizeof(float) * TB * H));
    ICZ_TRY(alloc((void**)&tb.logit, sizeof(float) * TB * Vp));
    ICZ_TRY(alloc_loss_buffers(mem, TB, B, T));
    ICZ_TRY(alloc((void**)&tb.nany, sizeof(int) * T));
    ICZ_TRY(alloc((void**)&tb.img2, sizeof(int32_t) * B));
    ICZ_TRY(alloc((void**)&tb.imgk, sizeof(int32_t) * B));
    ICZ_TRY(alloc((void**)&tb.lenk, sizeof(int32_t) * B));
    ICZ_TRY(alloc((void**)&tb.dGtd, sizeof(float) * TB * 4 * H));
    ICZ_TRY(alloc((void**)&tb.dGlm, sizeof(float) * TB * 4 * H));
    ICZ_TRY(alloc((void**)&tb.dDec, sizeof(float) * TB * A));
    ICZ_TRY(alloc((void**)&tb.dEmb, sizeof(float) * TB * E));
    ICZ_TRY(alloc((void**)&tb.dH2d, sizeof(float) * TB * H));
    ICZ_TRY(alloc((void**)&tb.dEnc, sizeof(float) * (size_t)B * R * A));
    ICZ_TRY(alloc((void**)&tb.dEncImg, sizeof(float) * (size_t)(B / 2) * R * A));      // sample_n: at most B / 2 images (K >= 2)
    ICZ_TRY(alloc((void**)&tb.dwaff, sizeof(float) * (size_t)B * ATT_PARTS * A));
    ICZ_TRY(alloc((void**)&tb.dalpha, sizeof(float) * (size_t)B * R * cdiv((int)D, DALPHA_COLS)));
    ICZ_TRY(alloc((void**)&tb.dS, sizeof(float) * TB * R));
    ICZ_TRY(alloc((void**)&tb.dGsum, sizeof(float) * (size_t)(B + B / 2) * 4 * H));     // + sample_n's per-image sums behind the B rows
    for (int i = 0; i < 2; ++i) {
        ICZ_TRY(alloc((void**)&tb.dc1[i], sizeof(float) * (size_t)B * H));
        ICZ_TRY(alloc((void**)&tb.dc2[i], sizeof(float) * (size_t)B * H));
    }
    tb.xfloats = (size_t)TARGET_WGS * 4096 * 2 + (size_t)B * (D + H);
    {   // X[0] is the sampled chain's slab workspace (train_step): same rule as Butd::init's ws_floats
        const size_t kmax = 2 * H + (E > D ? E : D), r128 = B < 128 ? B : 128;
        const size_t need = (kmax / 256 + 1) * r128 * 4 * H;
        if (need > tb.xfloats) tb.xfloats = need;
    }
    for (int i = 0; i < 4; ++i) ICZ_TRY(alloc((void**)&tb.X[i], sizeof(float) * tb.xfloats));
    ICZ_TRY(alloc((void**)&tb.dWp, sizeof(float) * Vp * H));
    ICZ_TRY(alloc((void**)&tb.dWenc, sizeof(float) * A * D));
    ICZ_TRY(alloc((void**)&tb.dWdec, sizeof(float) * A * H));
    {   // Split-K slabs of the weight gradients Butd::wgrad sends through gemm_tn_split (fewer than 256 tiles of 128 x 128, written with
        // ldo == N): W_hh of the two LSTMs when their column group is not taken (4H x H over T B rows), the two attention projections
        // (A x H over T B rows, A x D over B R rows), predict (Vp x H over T B rows).  One region per stream that can be inside bptt() at
        // the same time -- products of one stream run one after the other and share theirs: [1] belongs to the low-priority side stream
        // (predict branch, then the attention tail), [0] to the stream bptt() was called on (the LSTM products; all five when nothing is
        // forked: `concurrent` off, a gradient callback, phases as separate calls).  A product whose slabs do not fit takes the plain route.
        auto slabs = [](size_t M, size_t N, size_t K) { return (size_t)gemm_tn_split_pick((int)M, (int)N, (int)K) * M * N; };   // M N = no split
        const size_t side[3] = {slabs(A, H, TB), slabs(A, D, B * R), slabs(Vp, H, TB)}, own = slabs(4 * H, H, TB);
        const size_t direct[3] = {A * H, A * D, Vp * H};
        for (int i = 0; i < 3; ++i)
            if (side[i] > direct[i] && side[i] > tb.wslab_floats[1]) tb.wslab_floats[1] = side[i];
        tb.wslab_floats[0] = tb.wslab_floats[1];
        if (own > 4 * H * H && own > tb.wslab_floats[0]) tb.wslab_floats[0] = own;
        for (int i = 0; i < 2; ++i)
            if (tb.wslab_floats[i]) ICZ_TRY(alloc((void**)&tb.wslab[i], sizeof(float) * tb.wslab_floats[i]));
    }
    ICZ_TRY(alloc((void**)&tb.dWaff, sizeof(float) * A));
    ICZ_TRY(alloc((void**)&tb.scalars, sizeof(float) * 16));
    (void)V;
    ICZ_TRY(mem.synced());
    tb.B = B;
    tb.T = T;
    return ICZ_OK;
}

static DropCfg make_drop(const uint64_t* seed_p, bool train, const uint8_t* base, size_t per_step, uint32_t stream, int t, int row0 = 0) {
    DropCfg d = {0, nullptr, seed_p, stream, (uint32_t)t, row0};
    if (!train) return d;
    if (base) { d.mode = 1; d.mask = base + per_step * t; }
    else d.mode = 2;
    return d;
}

// ------------------------------------------------------------------------------------------------
// forward step into the saved-activation slots of time t (rows = active rows; slot stride = Bs rows)
// row0 > 0: the merged chain -- rows [0, row0) are evaluation-mode rows, the dropout arrays / Philox indices belong to the Bs - row0 rows behind
int Butd::train_step(const float* feats, int rows, int Bs, int t, bool train, hipStream_t st, bool emb_ready, int* pred_nsplit, bool skip_predict,
                     const int* live, int row0) {
    const size_t H = dims.H, D = dims.D, E = dims.E, A = dims.A, R = cur_R;
    const size_t Vp = pad_vocab(dims.V);
    const size_t slot = (size_t)t * Bs;
    StepIO s = {};
    s.emb_ready = emb_ready;         // written by the previous step's sample_select_kernel
    s.rows = rows; s.feats = feats; s.it = tb.tok + slot;
    s.h1_in = tb.h1 + slot * H; s.c1_in = tb.c1 + slot * H; s.h2_in = tb.h2 + slot * H; s.c2_in = tb.c2 + slot * H;
    s.h1_out = tb.h1 + (slot + Bs) * H; s.c1_out = tb.c1 + (slot + Bs) * H;
    s.h2_out = tb.h2 + (slot + Bs) * H; s.c2_out = tb.c2 + (slot + Bs) * H;
    s.emb_out = tb.emb + slot * E;
    s.gates_td_out = tb.gtd + slot * 4 * H; s.gates_lm_out = tb.glm + slot * 4 * H;
    s.dec_ctx_out = tb.dec + slot * A; s.alpha_out = tb.alpha + slot * R; s.ctx_out = tb.ctx + slot * D;
    s.h2drop_out = tb.h2d + slot * H; s.logits_out = tb.logit + slot * Vp; s.logits_ld = (int)Vp;
    // own slab workspace / score scratch (backward-only buffers, idle during the forward): the sampled rollout can
    // then run concurrently with the greedy rollout, which uses the handle's
    s.ws_alt = tb.X[0]; s.scores_alt = tb.dalpha;
    const size_t Bd = (size_t)(Bs - row0);            // rows the dropout arrays are laid out for
    s.drop_emb = make_drop(d_seed, train, rng.emb_mask, Bd * E, RNG_EMB, t, row0);
    s.drop_att = make_drop(d_seed, train, rng.att_mask, Bd * R * A, RNG_ATT, t, row0);
    s.drop_out = make_drop(d_seed, train, rng.out_mask, Bd * H, RNG_OUT, t, row0);
    if (row0 > 0) s.img_of_row = tb.img2;
    else if (cur_K > 1) {             // sample_n: K rows per image
        s.img_of_row = tb.imgk;
        s.rows_per_img = group_att ? cur_K : 1;
    }
    s.pred_nsplit = pred_nsplit;
    s.skip_predict = skip_predict;
    s.live = live;
    return step(s, st);
}

int Butd::sample(const float* feats, int B, int T, const icz_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_REQUIRE(feats && seq_out && logp_out && r, "butd sample: null argument");
    ICZ_REQUIRE(B > 0 && T > 0, "butd sample: bad B/T");
    ICZ_TRY(check_counts(B));
    ICZ_REQUIRE(fresh, "butd: call icz_butd_refresh_weights after binding/updating parameters");
    ICZ_TRY(ensure_train(B, T));
    rng = *r;
    begin_rollout(B, T, seq_out, logp_out, rng.seed, st);
    cur_feats = feats; cur_rows = B; cur_row0 = 0; cur_K = 1; cur_nimg = B;
    const bool explicit_rng = rng.uniforms || rng.emb_mask || rng.att_mask || rng.out_mask;
    if (explicit_rng || !graphs_on()) return sample_impl(feats, B, T, seq_out, logp_out, st);
    const std::vector<uintptr_t> key = {2, (uintptr_t)feats, (uintptr_t)B, (uintptr_t)T, (uintptr_t)seq_out, (uintptr_t)logp_out, opt_bits()};
    return gc.run(key, st, [&](hipStream_t s) { return sample_impl(feats, B, T, seq_out, logp_out, s); });
}

int Butd::sample_impl(const float* feats, int B, int T, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_TRY(prologue(feats, B, st));
    return sample_chain(feats, B, T, seq_out, logp_out, st);
}

// Multi-sample SCST rollout (beyond the reference: the "new self-critical" variant, K sampled captions per image): the per-image
// prologue runs once over the B images, the sampled chain over B K decoder rows, row = img * K + k, whose kernels find their image's
// hoisted tensors / features through tb.imgk (the grouped attention kernels take the K rows of an image in one workgroup).  Dropout
// keep-bits and draws are indexed by the row in the B K space: row img * K + k gets what row img * K + k of
// sample(feats.repeat_interleave(K, 0)) gets.
int Butd::sample_n(const float* feats, int B, int K, int T, const icz_rng* r, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_REQUIRE(feats && seq_out && logp_out && r, "butd sample_n: null argument");
    ICZ_REQUIRE(K >= 2 && K <= ATT_CTX_MAX_G, "butd sample_n: K=%d samples per image outside 2..%d", K, ATT_CTX_MAX_G);
    ICZ_REQUIRE(B > 0 && T > 0, "butd sample_n: bad B/T");
    ICZ_TRY(check_counts(B));
    ICZ_REQUIRE((int64_t)B * K <= dims.max_rows, "butd sample_n: %d images x %d samples exceed the row capacity %d", B, K, dims.max_rows);
    ICZ_REQUIRE(fresh, "butd: call icz_butd_refresh_weights after binding/updating parameters");
    const int rows = B * K;
    ICZ_TRY(ensure_train(rows, T));
    rng = *r;
    begin_rollout(rows, T, seq_out, logp_out, rng.seed, st);
    cur_feats = feats; cur_rows = rows; cur_row0 = 0; cur_K = K; cur_nimg = B;
    const bool explicit_rng = rng.uniforms || rng.emb_mask || rng.att_mask || rng.out_mask;
    if (explicit_rng || !graphs_on()) return sample_n_impl(feats, B, K, T, seq_out, logp_out, st);
    const std::vector<uintptr_t> key = {5, (uintptr_t)feats, (uintptr_t)B, (uintptr_t)K, (uintptr_t)T, (uintptr_t)seq_out, (uintptr_t)logp_out, opt_bits()};
    return gc.run(key, st, [&](hipStream_t s) { return sample_n_impl(feats, B, K, T, seq_out, logp_out, s); });
}

int Butd::sample_n_impl(const float* feats, int B, int K, int T, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_TRY(prologue(feats, B, st));
    hipLaunchKernelGGL(row_image_kernel, dim3(cdiv(B * K, 256)), dim3(256), 0, st, tb.imgk, B * K, K);
    return sample_chain(feats, B * K, T, seq_out, logp_out, st);
}

// Greedy baseline and sampled rollout of one SCST step (Engine.py:258-262) as two concurrent chains: they share the
// per-image prologue and the weights, nothing else, so they run on two streams (fork / join with events; inside a
// capture this becomes two parallel branches of the graph) and fill each other's idle CUs -- a skinny decoder-step
// GEMM occupies one workgroup per CU with its MFMA pipe about half busy.
int Butd::rollouts(const float* feats, int B, int T, const icz_rng* r, int64_t* ids_out, int64_t* seq_out, float* logp_out,
                   hipStream_t st) {
    ICZ_REQUIRE(feats && ids_out && seq_out && logp_out && r, "butd rollouts: null argument");
    ICZ_REQUIRE(B > 0 && T > 0 && B <= dims.max_rows, "butd rollouts: bad B/T");
    ICZ_TRY(check_counts(B));
    ICZ_REQUIRE(fresh, "butd: call icz_butd_refresh_weights after binding/updating parameters");
    // <= 32 images: ONE chain of 2 B decoder rows (sample_chain with row0 = B) instead of two chains that each stream the weights
    const bool merged = B <= merge_small;
    ICZ_TRY(ensure_train(merged ? 2 * B : B, T));
    ICZ_TRY(side.ensure());
    rng = *r;
    begin_rollout(B, T, seq_out, logp_out, rng.seed, st);
    cur_feats = feats; cur_rows = merged ? 2 * B : B; cur_row0 = merged ? B : 0; cur_K = 1; cur_nimg = B;
    const bool explicit_rng = rng.uniforms || rng.emb_mask || rng.att_mask || rng.out_mask;
    if (explicit_rng || !graphs_on()) return rollouts_impl(feats, B, T, ids_out, seq_out, logp_out, st);
    const std::vector<uintptr_t> key = {4, (uintptr_t)feats, (uintptr_t)B, (uintptr_t)T, (uintptr_t)ids_out, (uintptr_t)seq_out, (uintptr_t)logp_out, opt_bits()};
    return gc.run(key, st, [&](hipStream_t s) { return rollouts_impl(feats, B, T, ids_out, seq_out, logp_out, s); });
}

int Butd::rollouts_impl(const float* feats, int B, int T, int64_t* ids_out, int64_t* seq_out, float* logp_out, hipStream_t st) {
    ICZ_TRY(prologue(feats, B, st));
    if (cur_row0 > 0) return sample_chain(feats, B, T, seq_out, logp_out, st, cur_row0, ids_out);
    if (!concurrent) {
        ICZ_TRY(greedy_chain(feats, B, T, ids_out, nullptr, st, true));
        return sample_chain(feats, B, T, seq_out, logp_out, st);
    }
    SideStream::Branch baseline(&side, 0);
    ICZ_TRY(baseline.fork(st));
    ICZ_TRY(baseline.start());
    // the sampled chain (the longer one: multinomial draw, dropout) is issued -- and captured -- first: when kernels of both chains are
    // ready the runtime then takes its first.  Measured round 4, three same-box rounds: rollouts 2.758 / 2.774 / 2.769 ms against
    // 2.783 / 2.785 / 2.806 ms with the greedy chain first (profiles/r04_chain_issue_order.log)
    const int ss = sample_chain(feats, B, T, seq_out, logp_out, st);
    const int sg = greedy_chain(feats, B, T, ids_out, nullptr, baseline.st(), true);
    ICZ_TRY(baseline.join());
    return sg != ICZ_OK ? sg : ss;
}

__global__ void merged_init_kernel(int32_t* img2, int B, int* nany, int T, int64_t* tok_greedy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * B) img2[i] = i % B;
    if (i < T) nany[i] = 0;
    if (i < B) tok_greedy[i] = 1;
}

// The sampled rollout of B rows into the saved-activation slots.  row0 = B (and ids_out): the MERGED chain of a small SCST batch --
// every step carries 2 B decoder rows, the greedy baseline's (evaluation mode, argmax) in front of the sampled rollout's, so that
// the weights are streamed once per step pair instead of once per chain (at <= 32 rows a decoder step is bound by its weight
// stream: 196.68 MB against 8 - 32 x 0.49 MB of per-row data).  Per-row modes live in the kernels (DropCfg::row0,
// sample_select_kernel<true>); the slots hold 2 B rows per step, the backward pass works on the second half (Butd::bptt).
int Butd::sample_chain(const float* feats, int B, int T, int64_t* seq_out, float* logp_out, hipStream_t st, int row0, int64_t* ids_out) {
    const size_t H = dims.H;
    const size_t Vp = pad_vocab(dims.V);
    const int Bs = B + row0;
    // slot 0 of the state buffers = zeros; unfinished flags = 1, counters = 0, first token = <sta>
    {
        ZeroList z = {{tb.h1, tb.c1, tb.h2, tb.c2}, 4};
        const size_t n = (size_t)Bs * H;
        hipLaunchKernelGGL(zero_bufs_kernel, dim3(cdiv((int)(n / 4), 256)), dim3(256), 0, st, z, n);
    }
    hipLaunchKernelGGL(sample_init_kernel, dim3(cdiv(B > T ? B : T, 256)), dim3(256), 0, st, unf, nunf, tb.tok + row0, B, T);
    if (row0) hipLaunchKernelGGL(merged_init_kernel, dim3(cdiv(2 * B > T ? 2 * B : T, 256)), dim3(256), 0, st, tb.img2, B, tb.nany, T, tb.tok);
    const int* const counts = row0 ? tb.nany : nunf;           // what keeps a step alive
    for (int t = 0; t < T; ++t) {
        int pns = 1;
        // step t > 0 is dead when no row was left unfinished by step t - 1 (the reference breaks out of its loop there, :233): every
        // kernel of it returns at entry, sample_select_kernel writes the zeros the reference's pre-allocated outputs keep
        ICZ_TRY(train_step(feats, Bs, Bs, t, true, st, t > 0, &pns, false, (t > 0 && early_out) ? counts + (t - 1) : nullptr, row0));
        SampleSelArgs a = {};
        a.logits = tb.logit + (size_t)t * Bs * Vp; a.V = dims.V; a.ldl = (int)Vp;
        if (pns > 1) {          // the predict GEMM left split-K slabs in the chain's workspace (train_step: tb.X[0])
            a.logits = tb.X[0]; a.ns = pns; a.slab_stride = (size_t)Bs * Vp; a.bias = P.predict_b;
            a.logits_store = tb.logit + (size_t)t * Bs * Vp;
        }
        a.uniforms = rng.uniforms ? rng.uniforms + (size_t)t * B : nullptr;
        a.seed_p = d_seed; a.t = t; a.T = T;
        a.unfinished = unf; a.n_unfinished = nunf;
        a.live_rows = live_rows;
        a.seq_out = seq_out; a.logp_out = logp_out;
        a.row0 = row0; a.ids_out = ids_out; a.g_unfinished = gunf; a.n_any = tb.nany;
        a.it_next = tb.tok + (size_t)(t + 1) * Bs;
        a.draw_out = draw + (size_t)t * Bs; a.lse_out = lse + (size_t)t * Bs;
        if (t + 1 < T) {             // the next step's input embedding, fused (step t + 1's slot and dropout stream)
            a.emb_table = P.embed_weight; a.emb_next = tb.emb + (size_t)(t + 1) * Bs * dims.E; a.E = dims.E;
            a.emb_drop = make_drop(d_seed, true, rng.emb_mask, (size_t)B * dims.E, RNG_EMB, t + 1);
        }
        kprof_mark(KP_SAMPLE_SELECT, true, st);
        ICZ_TRY(launch_sample_select(st, Bs, a));
        kprof_mark(KP_SAMPLE_SELECT, false, st);
    }
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int Butd::sample_mask_sum(float* out, hipStream_t st) {
    ICZ_TRY(require_mode(1, "butd"));
    ICZ_REQUIRE(out, "null output");
    // reuse the loss kernel with zero reward (coef scratch is overwritten later by backward)
    ICZ_CHECK_HIP(hipMemsetAsync(loss_rows, 0, sizeof(float) * cur_B * cur_T, st));
    hipLaunchKernelGGL(reinforce_loss_kernel, dim3(1), dim3(256), 0, st, cur_logp, cur_seq, loss_rows, cur_B, cur_T,
                       (const float*)nullptr, coef, (float*)nullptr, out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int Butd::backward(LossHead head, const icz_butd_params* G, hipStream_t st) {
    // behind xe_forward_n only the XE loss itself runs, over image-major rows; cur_K stays, so bptt() folds the image-side products onto the images
    if (xe_grouped()) {
        ICZ_REQUIRE(head.kind != LossHead::XE_DLOGITS, "icz_butd_xe_backward_dlogits: the stored forward pass is a grouped one (icz_butd_xe_forward_n): its logits are not packed");
        ICZ_REQUIRE(head.kind != LossHead::XE_DISTILL, "icz_butd_xe_backward_distill: the stored forward pass is a grouped one (icz_butd_xe_forward_n): the teachers' logits are packed");
        ICZ_REQUIRE(head.kind != LossHead::XE_SWOR, "icz_butd_xe_backward_swor: the stored forward pass is a grouped one (icz_butd_xe_forward_n): its rows are not sorted by length");
        head.group_len = tb.lenk;
    }
    ICZ_TRY(check_loss_head(head, G));
    const int V = dims.V, Vp = pad_vocab(dims.V);
    const bool eo = head.rollout_kind() && early_out;
    // the REINFORCE / objective head goes into the captured graph with its bptt(); every other head is queued here
    const bool in_graph = head.kind == LossHead::ROLLOUT;
    ICZ_TRY(begin_backward(head, in_graph, tb.logit, V, Vp, st, cur_rows, cur_row0));
    ICZ_TRY(bptt_prelude(st));      // outside the captured graph
    if (!in_graph) return bptt(*G, st, eo);
    const RolloutHead& hd = head.rollout;
    const icz_butd_params Gc = *G;
    auto run = [&](hipStream_t s, int phases, bool fire_cb) -> int {
        if (phases & 1) ICZ_TRY(launch_loss_head(head, tb.logit, V, Vp, s, cur_rows, cur_row0));
        return bptt(Gc, s, eo, phases, fire_cb);
    };
    const bool explicit_rng = rng.uniforms || rng.emb_mask || rng.att_mask || rng.out_mask;
    if (explicit_rng || !graphs_on()) return run(st, 0xF, true);
    // the captured graphs carry the objective in their key (ScstObjective::key) beside the output pointers
    std::vector<uintptr_t> key = {3, (uintptr_t)hd.reward, (uintptr_t)hd.loss_out, (uintptr_t)hd.msum_out, (uintptr_t)cur_B, (uintptr_t)cur_T,
                                  (uintptr_t)cur_feats, (uintptr_t)cur_seq, (uintptr_t)cur_logp,
                                  (uintptr_t)cur_rows, (uintptr_t)cur_row0,       // merged / unmerged rollouts share the caller's buffers: slot strides differ
                                  (uintptr_t)cur_K};                              // sample_n of B K rows against sample of B K rows: other kernels
    const float* const* gp = reinterpret_cast<const float* const*>(G);
    for (size_t i = 0; i < sizeof(icz_butd_params) / sizeof(float*); ++i) key.push_back((uintptr_t)gp[i]);
    if (hd.obj) { hd.obj->key(key); key.push_back((uintptr_t)hd.ent_out); }
    if (!grad_cb) {
        key.push_back(opt_bits());
        return gc.run(key, st, [&](hipStream_t s) { return run(s, 0xF, true); });
    }
    // The DP hook must fire on every call (a replayed graph would not call it): the backward is cut at the three points where a
    // gradient group is complete, every piece is its own captured graph, and the hook is called between the replays -- the
    // all-reduce of a group then starts beside the remaining pieces exactly as in the eager form.
    for (int ph = 0; ph < 4; ++ph) {
        std::vector<uintptr_t> k2 = key;
        k2.push_back(0x100 + ph);
        k2.push_back(opt_bits());
        ICZ_TRY(gc.run(k2, st, [&](hipStream_t s) { return run(s, 1 << ph, false); }));
        if (ph < 3) grad_cb(grad_cb_user, ph);
    }
    return ICZ_OK;
}

// ------------------------------------------------------------------------------------------------
int Butd::xe_forward(const float* feats, const int64_t* captions, int B, int L, const int32_t* lengths, const icz_rng* r,
                     int train, float* packed_out, hipStream_t st) {
    ICZ_REQUIRE(feats && captions && lengths && B > 0 && L > 1, "butd xe_forward: bad arguments");
    ICZ_TRY(check_counts(B));
    int T = 0;
    ICZ_TRY(xe_steps("butd", lengths, B, L, &T));
    ICZ_TRY(ensure_train(B, T));
    if (r) rng = *r; else { rng = {}; }
    ICZ_REQUIRE(!train || r, "butd xe_forward: training mode needs an icz_rng");
    begin_xe(lengths, B, T, L, captions, train != 0, rng.seed, st);
    cur_feats = feats;
    cur_rows = B; cur_row0 = 0; cur_K = 1; cur_nimg = B;
    const size_t H = dims.H;
    const size_t Vp = pad_vocab(dims.V);
    ICZ_TRY(prologue(feats, B, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tb.h1, 0, sizeof(float) * B * H, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tb.c1, 0, sizeof(float) * B * H, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tb.h2, 0, sizeof(float) * B * H, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tb.c2, 0, sizeof(float) * B * H, st));
    ICZ_CHECK_HIP(hipMemsetAsync(tb.logit, 0, sizeof(float) * (size_t)T * B * Vp, st));
    captions_to_tok(tb.tok, st);
    // Teacher forcing: no step needs the previous step's logits unless scheduled sampling draws from them -> one vocabulary projection
    // over all time steps after the loop (T B >= 128 rows: a single GEMM on the big-tile kernel instead of T decoder-step GEMMs)
    const bool batched_predict = ss_prob <= 0.f && T * B >= 128;
    const bool batched_embed = ss_prob <= 0.f && T <= EMB_MAX_T && dims.E % 4 == 0;       // likewise the embeddings of all steps: one launch
    if (batched_embed) {
        EmbRows er = {};
        for (int t = 0; t < T; ++t) er.n[t] = rows_t[t];
        hipLaunchKernelGGL(embed_steps_kernel, dim3(cdiv(dims.E, 1024), T * B), dim3(256), 0, st, P.embed_weight, tb.tok, tb.emb, B, dims.E, er,
                           make_drop(d_seed, train != 0, rng.emb_mask, (size_t)B * dims.E, RNG_EMB, 0));
    }
    for (int t = 0; t < T; ++t) {
        if (t >= 2 && ss_prob > 0.f)          // BUTD_Model.py:120-130: this step's tokens, mixed with draws from the previous step's logits
            ICZ_TRY(ss_select_launch(st, rows_t[t], tb.logit + (size_t)(t - 1) * B * Vp, (int)Vp, dims.V, t, B, ss_prob, ss_gate, ss_draw,
                                     d_seed, tb.tok + (size_t)t * B));
        ICZ_TRY(train_step(feats, rows_t[t], B, t, train != 0, st, batched_embed, nullptr, batched_predict));
    }
    if (batched_predict) {
        // logits of all (t, b) rows at once: [T B, H] x w_pred^T + b through the 128 x 128 split-precision kernel (one pass over the
        // vocabulary matrix instead of T).  Rows b >= rows_t[t] hold whatever their h2 slots held: nothing reads them before
        // xe_loss_dlogits_kernel / scatter_packed_kernel overwrite them with zeros.
        GemmArgs g = gemm_args({{tb.h2d, w_pred, (int)H, (int)H, (int)H}}, T * B, dims.V, tb.logit, (int)Vp);
        g.bias = P.predict_b;
        ICZ_TRY(gemm_f32(GEMM_NT, g, st));
    }
    if (packed_out) ICZ_TRY(gather_packed(tb.logit, dims.V, (int)Vp, packed_out, st));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// Teacher-forced XE on K captions per image (beyond the reference; the regime of seq_per_img = 5): sample_n's layout with the captions'
// tokens in the place of the draws.  The prologue runs once over the B images; the chain runs over the B K rows, row = img * K + k in
// any length order, on the stored-activation slots (slot stride B K rows), finding the image through tb.imgk.  Every row runs every
// step: a row that has ended is fed <pad>, its later steps are masked by the loss (xe_group_loss: t < tb.lenk[row]) and so carry
// zero gradient rows through bptt().  Dropout keep-bits are those of row img * K + k in the B K space, as sample_n's.
// The refusals of include/icz.h in their order (1 - 3 stand in front of the handle, in the C entry's xe_forward_n_args), each before
// anything is queued or any state of the handle is touched.
static int xe_forward_n_args(const char* who, const float* feats, const int64_t* captions, int B, int K, int L, const int32_t* lengths) {
    ICZ_REQUIRE(feats && captions && lengths, "%s: null feats, captions or lengths_host", who);
    ICZ_REQUIRE(K >= 2 && K <= ATT_CTX_MAX_G, "%s: K=%d captions per image outside 2..%d", who, K, ATT_CTX_MAX_G);
    ICZ_REQUIRE(B >= 1 && B <= (1 << 20) && L >= 2, "%s: B=%d images (at least 1) or L=%d columns (at least 2)", who, B, L);
    for (int i = 0; i < B * K; ++i)
        ICZ_REQUIRE(lengths[i] >= 1 && lengths[i] <= L - 1, "%s: lengths_host[%d]=%d outside 1..%d", who, i, lengths[i], L - 1);
    return ICZ_OK;
}

int Butd::xe_forward_n(const float* feats, const int64_t* captions, int B, int K, int L, const int32_t* lengths, const icz_rng* r,
                       int train, float* logits_out, hipStream_t st) {
    const char* who = "butd xe_forward_n";
    ICZ_TRY(xe_forward_n_args(who, feats, captions, B, K, L, lengths));
    ICZ_REQUIRE((int64_t)B * K <= dims.max_rows, "%s: %d images x %d captions exceed the row capacity %d", who, B, K, dims.max_rows);
    ICZ_TRY(check_counts(B));
    ICZ_REQUIRE(fresh, "%s: call icz_butd_refresh_weights after binding/updating parameters", who);
    ICZ_REQUIRE(!train || r, "%s: training mode needs an icz_rng", who);
    ICZ_REQUIRE(ss_prob <= 0.f, "%s: scheduled sampling is switched on (ss_prob %g); the grouped forward feeds the captions' own tokens", who,
                (double)ss_prob);
    const int rows = B * K;
    int T = 0;
    for (int i = 0; i < rows; ++i) T = lengths[i] > T ? lengths[i] : T;
    ICZ_TRY(ensure_train(rows, T));
    if (r) rng = *r; else { rng = {}; }
    begin_xe(lengths, rows, T, L, captions, train != 0, rng.seed, st);
    rows_t.assign(T, rows);            // every row is stored at every step; n_tokens stays the sum of the lengths
    cur_feats = feats;
    cur_rows = rows; cur_row0 = 0; cur_K = K; cur_nimg = B;
    const size_t H = dims.H;
    const size_t Vp = pad_vocab(dims.V);
    ICZ_TRY(prologue(feats, B, st));
    hipLaunchKernelGGL(row_image_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, tb.imgk, rows, K);
    upload_lengths(tb.lenk, lengths, rows, st);
    {
        ZeroList z = {{tb.h1, tb.c1, tb.h2, tb.c2}, 4};
        const size_t n = (size_t)rows * H;
        hipLaunchKernelGGL(zero_bufs_kernel, dim3(cdiv((int)(n / 4), 256)), dim3(256), 0, st, z, n);
    }
    launch_captions_to_tok_len(captions, rows, L, T, tb.lenk, tb.tok, st);
    // as xe_forward: one embedding launch and one vocabulary projection over all (t, row), the slot addressing being the same
    const bool batched_predict = T * rows >= 128;
    const bool batched_embed = T <= EMB_MAX_T && dims.E % 4 == 0;
    if (batched_embed) {
        EmbRows er = {};
        for (int t = 0; t < T; ++t) er.n[t] = rows;
        hipLaunchKernelGGL(embed_steps_kernel, dim3(cdiv(dims.E, 1024), T * rows), dim3(256), 0, st, P.embed_weight, tb.tok, tb.emb, rows, dims.E, er,
                           make_drop(d_seed, train != 0, rng.emb_mask, (size_t)rows * dims.E, RNG_EMB, 0));
    }
    for (int t = 0; t < T; ++t) ICZ_TRY(train_step(feats, rows, rows, t, train != 0, st, batched_embed, nullptr, batched_predict));
    if (batched_predict) {
        GemmArgs g = gemm_args({{tb.h2d, w_pred, (int)H, (int)H, (int)H}}, T * rows, dims.V, tb.logit, (int)Vp);
        g.bias = P.predict_b;
        ICZ_TRY(gemm_f32(GEMM_NT, g, st));
    }
    if (logits_out) launch_gather_rows(tb.logit, dims.V, (int)Vp, rows, T, tb.lenk, logits_out, st);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// ------------------------------------------------------------------------------------------------
// helpers for the backward GEMMs
// direct output (ns = 1, where g.out points) if there are already enough tiles, else slabs in `slab` (null: never split above 64 rows)
int Butd::gemm_auto(GemmLayout layout, GemmArgs& g, float* slab, size_t slab_floats, int* ns_out, hipStream_t st) {
    return gemm_slabs(layout, g, split_backward(STEP_WGS), slab, slab_floats, ns_out, st, "butd");
}

// C (ldc) = A^T B over K rows: weight gradients.  Too few 128 x 128 tiles to fill the chip (at full width the attention projections):
// split K on the large-tile split-precision kernel, sum the slabs (gemm_tn_auto) -- in the slab region of the stream the product is
// issued on (no two streams share slab memory: the side stream's products have a region of their own, see ensure_train)
int Butd::wgrad(const float* dY, int ldy, int M, const float* X, int ldx, int N, int K, float* out, int ldo, hipStream_t st, const int* rows_live) {
    const int r = wslab_of(st);
    return gemm_tn_auto(dY, ldy, M, X, ldx, N, K, out, ldo, tb.wslab[r], tb.wslab_floats[r], rows_live, st);
}

// The transposed weight copies of the per-step dgrad products are rebuilt lazily, by the first backward call after an optimizer
// step: backward() calls this in front of bptt(), OUTSIDE its captured graph (a replayed graph must not rebuild them).
int Butd::bptt_prelude(hipStream_t st) {
    if (wt_lm_ih && !wt_fresh) ICZ_TRY(refresh_transposes(st));
    // the side stream of bptt, created here, outside any capture.  Lowest priority: its big GEMMs only fill CUs the BPTT chain leaves idle
    ICZ_TRY(low.ensure(true));
    return ICZ_OK;
}

// What the phases of one bptt() call share.  The two branches live as long as the call: whatever a phase returns, a branch it has
// started is joined before bptt() returns (SideStream::Branch).
struct Butd::BpttCall {
    const icz_butd_params& G;
    hipStream_t st;
    // B rows are worked on per step; the buffers hold Bs rows per step, of which those are rows [roff, roff + B) (Bs = B, roff = 0
    // except behind a merged chain, whose evaluation-mode rows in front carry zero gradient rows through the GEMMs over all steps)
    int B, T, Bs, roff, TB;
    // backward of a sampled rollout (eo): the steps behind the reference's break never ran -- their kernels return at entry, and the
    // GEMMs over all (t, b) rows stop behind the last step the rollout ran (rl: GemmArgs::rows_live)
    bool eo;
    const int* rl;
    // behind sample_n: K rows per image (row = img * K + k) -- the kernels that read the image's features / enc_ctx per row find it
    // through tb.imgk, and the image-side products (d enc_ctx, the mean-feature weights) are folded onto the n_img images first
    int K, n_img;
    const int32_t* imgk;
    SideStream::Branch predict;      // the predict layer's weight / bias gradients beside the reverse-time loop
    SideStream::Branch tail;         // the attention block's tail beside the LSTM weight gradients
};

// phases: bit 0 = predict layer + reverse-time loop, bit 1 = embedding and TD-LSTM weight gradients, bit 2 = LM-LSTM weight
// gradients, bit 3 = attention block, biases.  After each of the first three the corresponding gradient group is complete
// in stream order (icz_butd_set_grad_callback); fire_cb = false leaves the callbacks to the caller, which replays every phase
// as its own captured graph and calls them in between.
int Butd::bptt(const icz_butd_params& G, hipStream_t st, bool eo, int phases, bool fire_cb) {
    const bool cb = grad_cb && fire_cb;
    // The attention block's tail (phase 3: d enc_ctx, two small weight gradients, bias sums, weight-norm backward: ~0.2 ms of kernels
    // that fill a fraction of the chip) depends on the loop only.  When the whole backward is one call without a DP callback it is
    // forked at the loop's end and issued LAST, on the low-priority stream, beside the LSTM weight gradients: backward 2.685 / 2.684 /
    // 2.698 -> 2.659 / 2.662 / 2.649 ms in three same-box rounds (profiles/r04_backward_issue_order.log; forked behind the TD gradients
    // instead: slower, 2.73 - 2.75 ms; round 2 had issued such a branch FIRST and lost 0.25 ms).  With a callback the phases are
    // separate graphs and stay in line.
    const bool tail_side = phases == 0xF && !grad_cb && concurrent;
    const int K = cur_K;
    BpttCall c = {G, st, cur_B, cur_T, cur_rows, cur_row0, cur_T * cur_rows, eo, eo ? live_rows : nullptr,
                  K, K > 1 ? cur_nimg : cur_B, K > 1 ? tb.imgk : nullptr, {concurrent ? &low : nullptr, 0}, {tail_side ? &low : nullptr, 1}};
    if (phases & 1) {
        ICZ_TRY(bptt_predict(c));
        ICZ_TRY(bptt_loop(c));
        // with a DP callback the predict branch, long finished beside the loop, is joined here: its gradients are complete in stream
        // order when the hook fires, and each phase is its own captured graph
        if (grad_cb) ICZ_TRY(c.predict.join());
        if (cb) grad_cb(grad_cb_user, 0);
    }
    ICZ_TRY(c.tail.fork(st));
    if (phases & 2) {
        ICZ_TRY(bptt_embed_td_wgrad(c));
        if (cb) grad_cb(grad_cb_user, 1);
    }
    if (phases & 4) {
        ICZ_TRY(bptt_lm_wgrad(c));
        if (cb) grad_cb(grad_cb_user, 2);
    }
    if (phases & 8) {
        ICZ_TRY(c.tail.start());
        ICZ_TRY(bptt_attention_tail(c));
    }
    ICZ_TRY(c.tail.join());
    ICZ_TRY(c.predict.join());
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// ---- predict layer, all time steps at once.  d h2drop feeds the BPTT chain; the weight / bias gradients of `predict` depend only
//      on dlogits, so they run on the side stream concurrently with the (skinny, latency-bound) BPTT chain.
int Butd::bptt_predict(BpttCall& c) {
    const int H = dims.H, A = dims.A, R = dims.R, V = dims.V, Vp = pad_vocab(V), TB = c.TB;
    hipStream_t const st = c.st;
    // The side branch is forked here (it depends on dlogits only) but ISSUED behind the d h2drop GEMM below, the head of the critical
    // chain: issued first, its 10112 x 1024 x 1280 GEMM took the CUs ahead of that product.  Round 4, three same-box rounds: backward
    // 2.738 / 2.718 / 2.729 ms against 2.777 / 2.828 / 2.803 ms (profiles/r04_backward_issue_order.log); forking it behind the
    // product as well (no overlap with it at all): 2.762 / 2.779 / 2.750 ms.
    ICZ_TRY(c.predict.fork(st));
    {
        GemmArgs g = gemm_args({{tb.logit, w_pred, Vp, H, Vp}}, TB, H, tb.dH2d, H);
        g.rows_live = c.rl;
        // nothing is forked yet: the side branch is issued behind this product
        ICZ_TRY(gemm_finished(GEMM_NN, g, split_backward(STEP_WGS), nullptr, ws, ws_floats, st, "butd"));
    }
    ICZ_TRY(c.predict.start());
    hipStream_t const sb = c.predict.st();
    ICZ_TRY(wgrad(tb.logit, Vp, Vp, tb.h2d, H, H, TB, tb.dWp, H, sb, c.rl));
    (void)launch_colsum(tb.logit, TB, V, Vp, c.G.predict_b, sb);
    launch_weight_norm_bwd(tb.dWp, H, P.predict_v, P.predict_g, n_pred, c.G.predict_v, c.G.predict_g, V, H, sb);
    ICZ_TRY(c.predict.finish());
    // ---- XE only: rows that dropped out of the batch must contribute zero (the sample path writes every row, and its
    //      accumulators are initialised by the first processed step)
    const bool ragged = rows_t[c.T - 1] < c.B || c.roff > 0;
    if (ragged) {
        ICZ_CHECK_HIP(hipMemsetAsync(tb.dGtd, 0, sizeof(float) * (size_t)TB * 4 * H, st));
        ICZ_CHECK_HIP(hipMemsetAsync(tb.dGlm, 0, sizeof(float) * (size_t)TB * 4 * H, st));
        ICZ_CHECK_HIP(hipMemsetAsync(tb.dDec, 0, sizeof(float) * (size_t)TB * A, st));
        ICZ_CHECK_HIP(hipMemsetAsync(tb.dS, 0, sizeof(float) * (size_t)TB * R, st));
    }
    return ICZ_OK;
}

// ---- "X2 = d dec . w_dec, then the TD-LSTM backward" as one launch (lstm_bwd_dh1_fused_kernel, lstm_kernels.h).  Its K ranges are
//      the two-launch route's: the split gemm_auto gives the same product, in the stage depth gemm_f32 takes for it.
static int dh1_split(int rows, int H, int A) {
    const GemmArgs g = gemm_args({{nullptr, nullptr, A, H, A}}, rows, H, nullptr, H);      // shapes only
    return gemm_split(GEMM_NN, g, split_backward(Butd::STEP_WGS), 0);
}
static int launch_dh1_fused(const LstmBwdArgs& p, const float* ddec, const float* w_dec, int A, hipStream_t st) {
    ICZ_REQUIRE(lstm_bwd_dh1_fused_takes(p.rows, p.H, A), "butd: the fused d h1 step does not take rows=%d, H=%d, A=%d", p.rows, p.H, A);
    const int bkc = lstm_bwd_dh1_stage_k(A), tot = A / bkc, ns = dh1_split(p.rows, p.H, A);
    ICZ_REQUIRE(ns >= 1 && ns <= DH1_MAX_SPLIT && ns <= tot, "butd: the fused d h1 step cannot mirror %d K ranges over %d stages", ns, tot);
    const int cps = cdiv(tot, ns);
    ICZ_REQUIRE(cdiv(tot, cps) == ns, "butd: the fused d h1 step cannot mirror %d K ranges over %d stages", ns, tot);
    const Dh1FusedArgs f = {p, ddec, w_dec, A, ns, cps};
    const dim3 grid(p.H / DH1_TILE, cdiv(p.rows, DH1_TILE));
    if (bkc == 128) hipLaunchKernelGGL(lstm_bwd_dh1_fused_kernel<128>, grid, dim3(256), 0, st, f);
    else hipLaunchKernelGGL(lstm_bwd_dh1_fused_kernel<64>, grid, dim3(256), 0, st, f);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// ---- the reverse-time loop: per step the pointwise LSTM / attention backward kernels and the dgrad products between them
int Butd::bptt_loop(BpttCall& c) {
    const int B = c.B, T = c.T, Bs = c.Bs, roff = c.roff;
    const int H = dims.H, D = dims.D, E = dims.E, A = dims.A, R = cur_R;
    const bool ad = adaptive();
    const size_t sH = (size_t)Bs * H;
    const float* const feats = cur_feats;
    const int32_t* const imgk = c.imgk;
    hipStream_t const st = c.st;
    int cur = 0;
    int ns1 = 1, ns2 = 1, ns3 = 1, ns4 = 1;
    int bnext = 0;
    for (int t = T - 1; t >= 0; --t) {
        const int bt = rows_t[t];
        const size_t slot = (size_t)t * Bs + roff;
        // REINFORCE backward of a sampled rollout: the steps behind the reference's break never ran (sample_chain) -- their kernels
        // return at entry, the producers of d gates / d dec / ds rows write zeros (the GEMMs over all steps read them), and the
        // first live step takes no carry from the dead one behind it
        const int* const live = (c.eo && t > 0) ? nunf + (t - 1) : nullptr;
        const int* const carry_live = (c.eo && t + 1 < T) ? nunf + t : nullptr;
        DropCfg d_out = make_drop(d_seed, cur_train, rng.out_mask, (size_t)B * H, RNG_OUT, t);
        DropCfg d_att = make_drop(d_seed, cur_train, rng.att_mask, (size_t)B * R * A, RNG_ATT, t);
        DropCfg d_off = {0, nullptr, nullptr, 0, 0};
        {   // language LSTM backward (pointwise)
            LstmBwdArgs a = {};
            a.dh_a = bnext ? tb.X[2] : nullptr; a.ns_a = ns3; a.lda_a = H; a.rows_a = bnext;
            a.dhdrop = tb.dH2d + slot * H;
            a.dc_in = bnext ? tb.dc2[cur] : nullptr; a.dc_in_rows = bnext;
            a.gates = tb.glm + slot * 4 * H;
            a.c_prev = tb.c2 + slot * H; a.c_cur = tb.c2 + slot * H + sH;
            a.dgates = tb.dGlm + slot * 4 * H; a.dc_prev = tb.dc2[cur ^ 1];
            a.rows = bt; a.H = H; a.live = live; a.carry_live = carry_live;
            hipLaunchKernelGGL(lstm_bwd_point_kernel, dim3(cdiv(H, 256), bt), dim3(256), 0, st, a, d_out);
        }
        // 33 .. 64 rows: the per-step dgrad products as NT products on the transposed weight copies (resident-activation kernel)
        // (capacity: 4H / 256 slabs of bt x (D + H) resp. (2 x) 4H / 256 slabs of bt x H must fit tb.X[*]; larger models -- H = 1536
        // with D = 2048 already -- take the NN path below, whose split is fitted to the buffer)
        const bool rdg = wt_lm_ih && wt_fresh && bt > 32 && bt <= 64 && gemm_slab_floats(bt, D + H, 4 * H / 256) <= tb.xfloats &&
                         gemm_slab_floats(bt, H, 2 * (4 * H / 256)) <= tb.xfloats;
        // <= 32 rows (small batches, the tail of a ragged XE batch): the NN kernel streams W[k][n] at ~2 TB/s there, the fp32 NT kernel
        // the transposed copies at 3.4 - 4.4 (profiles/r05_scst_b8_*: 12 us for 26 MB against 12 us for 40 MB)
        const bool tdg = small_nt && wt_lm_ih && wt_fresh && bt <= 32;
        // The route selects only the weight operand and the layout of a per-step dgrad product dx = d gates . W over K = 4H: rdg and tdg
        // take the transposed copy (NT), else W itself (NN).  Each product leaves ns slabs [bt, N] (one: dense) in its tb.X buffer.
        const GemmLayout lay = (rdg || tdg) ? GEMM_NT : GEMM_NN;
        // X2 and the TD-LSTM backward as one launch (option "fused_dh1"), whatever route the other products take; steps the kernel
        // does not take -- more than 64 rows, other widths -- keep the two launches
        const bool fdh = fused_dh1 && lstm_bwd_dh1_fused_takes(bt, H, A);
        const float* const dglm = tb.dGlm + slot * 4 * H;
        const float* const dgtd = tb.dGtd + slot * 4 * H;      // (written by this step's TD-LSTM kernel below, before the products that read it)
        auto wseg = [&](const float* dg, const float* w_t, const float* w, int ldw) -> GemmSeg {
            return lay == GEMM_NT ? GemmSeg{dg, w_t, 4 * H, 4 * H, 4 * H} : GemmSeg{dg, w, 4 * H, ldw, 4 * H};
        };
        auto dgrad = [&](GemmArgs g, float* slab, int* ns) -> int {
            if (!rdg) return gemm_auto(lay, g, slab, tb.xfloats, ns, st);
            *ns = gemm_resident_x3_nsplit(g);      // the resident kernel's fixed decomposition (sized by the rdg condition above)
            return gemm_slabs(GEMM_NT, g, *ns, slab, tb.xfloats, st, "butd");
        };
        // X1 = dG_lm . W_ih_lm   [bt, D+H]
        ICZ_TRY(dgrad(gemm_args({wseg(dglm, wt_lm_ih, P.lm_w_ih, D + H)}, bt, D + H, tb.X[0], D + H, live), tb.X[0], &ns1));
        {   // attention backward
            const int dparts = att_dalpha_parts(D);
            launch_att_bwd_dalpha(ad, tb.X[0], ns1, D + H, bt, feats, R, D, tb.dalpha, live, imgk, cnt, st);
            AttBwdDdecArgs da = {enc_ctx, tb.dec + slot * A, w_aff, tb.alpha + slot * R, tb.dalpha, tb.dDec + slot * A, tb.dS + slot * R, R, A, dparts, live, imgk, cnt};
            launch_att_bwd_ddec(ad, da, d_att, bt, st);
            // X2 = dDec . w_dec   [bt, H] (the fused route forms it inside the TD-LSTM launch below: tb.X[1] is not written then, and
            // nothing else reads it)
            if (!fdh) {
                GemmArgs g = gemm_args({{tb.dDec + slot * A, w_dec, A, H, A}}, bt, H, tb.X[1], H, live);
                ICZ_TRY(gemm_auto(GEMM_NN, g, tb.X[1], tb.xfloats, &ns2, st));
            }
        }
        {   // TD LSTM backward (pointwise): dh1 = carry + X1[:, D:] + X2
            LstmBwdArgs a = {};
            a.dh_a = bnext ? tb.X[3] : nullptr; a.ns_a = ns4; a.lda_a = H; a.rows_a = bnext;
            a.dh_b = tb.X[0] + D; a.ns_b = ns1; a.lda_b = D + H; a.rows_b = bt;
            if (!fdh) { a.dh_c = tb.X[1]; a.ns_c = ns2; a.lda_c = H; a.rows_c = bt; }
            a.dc_in = bnext ? tb.dc1[cur] : nullptr; a.dc_in_rows = bnext;
            a.gates = tb.gtd + slot * 4 * H;
            a.c_prev = tb.c1 + slot * H; a.c_cur = tb.c1 + slot * H + sH;
            a.dgates = tb.dGtd + slot * 4 * H; a.dc_prev = tb.dc1[cur ^ 1];
            a.rows = bt; a.H = H; a.live = live; a.carry_live = carry_live;
            if (fdh) ICZ_TRY(launch_dh1_fused(a, tb.dDec + slot * A, w_dec, A, st));
            else hipLaunchKernelGGL(lstm_bwd_point_kernel, dim3(cdiv(H, 256), bt), dim3(256), 0, st, a, d_off);
        }
        if (t > 0) {
            // X3 = dG_lm . W_hh_lm + dG_td . W_ih_td[:, :H]   -> d h2_{t-1};   X4 = dG_td . W_hh_td   -> d h1_{t-1}
            const GemmArgs g3 = gemm_args({wseg(dglm, wt_lm_hh, P.lm_w_hh, H), wseg(dgtd, wt_td_ih_h2, P.td_w_ih, H + D + E)}, bt, H, tb.X[2], H, live);
            const GemmArgs g4 = gemm_args({wseg(dgtd, wt_td_hh, P.td_w_hh, H)}, bt, H, tb.X[3], H, live);
            if (rdg) {   // both in one launch
                ns3 = gemm_resident_x3_nsplit(g3); ns4 = gemm_resident_x3_nsplit(g4);
                ICZ_REQUIRE(gemm_slab_floats(bt, H, ns3) <= tb.xfloats, "butd: slab buffer too small for the dgrad slabs");
                ICZ_TRY(gemm_resident_x3_pair(g3, g4, st));
            } else {
                ICZ_TRY(dgrad(g3, tb.X[2], &ns3));
                ICZ_TRY(dgrad(g4, tb.X[3], &ns4));
            }
        }
        bnext = bt;
        cur ^= 1;
    }
    return ICZ_OK;
}

// ---- embedding gradient and the TD-LSTM weight gradients
int Butd::bptt_embed_td_wgrad(BpttCall& c) {
    const int B = c.B, T = c.T, Bs = c.Bs, roff = c.roff, TB = c.TB, K = c.K, n_img = c.n_img;
    const int H = dims.H, D = dims.D, E = dims.E, V = dims.V, ldtd = H + D + E;
    const icz_butd_params& G = c.G;
    const int* const rl = c.rl;
    hipStream_t const st = c.st;
    // ---- embedding gradient: dEmb = dG_td . W_ih_td[:, H+D:] for all steps, then ordered scatter
    {
        GemmArgs g = gemm_args({{tb.dGtd, P.td_w_ih + H + D, 4 * H, H + D + E, 4 * H}}, TB, E, tb.dEmb, E);
        g.rows_live = rl;
        ICZ_TRY(gemm_finished(GEMM_NN, g, split_backward(STEP_WGS), nullptr, ws, ws_floats, st, "butd"));
        // inactive (t,b) rows have dG = 0 -> dEmb = 0; their token ids are whatever the buffer held (valid ids)
        ICZ_CHECK_HIP(embed_grad_launch(st, tb.tok, TB, tb.dEmb, 1, (size_t)0, tb.emb, cur_train ? 2.0f : 1.0f, E, G.embed_weight, V, 1, rl));
    }
    // ---- weight gradients: one TN GEMM each over all (t, b)
    // (round 5) the three products over all (t, b) share d gates: one launch over the column groups [h2 | emb | h1] (4096 x 3072 at the
    // BASELINE sizes: 183 us against 3 x 85, gemm_big_x3.hip); shapes it does not take go one by one
    const GemmColGroup td_groups[3] = {{tb.h2, H, H, G.td_w_ih, ldtd},                       // h2_{t-1}
                                       {tb.emb, E, E, G.td_w_ih + H + D, ldtd},              // embedding
                                       {tb.h1, H, H, G.td_w_hh, H}};                         // h1_{t-1}
    const bool td_grouped = gemm_tn_grouped_fits(4 * H, TB, td_groups, 3);
    if (td_grouped) ICZ_TRY(gemm_tn_grouped(tb.dGtd, 4 * H, 4 * H, TB, td_groups, 3, rl, st));
    else ICZ_TRY(wgrad(tb.dGtd, 4 * H, 4 * H, tb.h2, H, H, TB, G.td_w_ih, ldtd, st, rl));
    launch_timesum(tb.dGtd, T, (size_t)Bs * 4 * H, tb.dGsum, st);
    if (K > 1) {      // sample_n: the K rows of an image share its mean features -- their time sums are added in k order first
        float* const gimg = tb.dGsum + (size_t)Bs * 4 * H;
        const size_t N4 = (size_t)4 * H;
        launch_rowgroup_sum(tb.dGsum, n_img, K, N4, gimg, st);
        ICZ_TRY(wgrad(gimg, 4 * H, 4 * H, mean, D, D, n_img, G.td_w_ih + H, ldtd, st));
    } else
        ICZ_TRY(wgrad(tb.dGsum + (size_t)roff * 4 * H, 4 * H, 4 * H, mean, D, D, B, G.td_w_ih + H, ldtd, st));      // mean features
    if (!td_grouped) {
        ICZ_TRY(wgrad(tb.dGtd, 4 * H, 4 * H, tb.emb, E, E, TB, G.td_w_ih + H + D, ldtd, st, rl));
        ICZ_TRY(wgrad(tb.dGtd, 4 * H, 4 * H, tb.h1, H, H, TB, G.td_w_hh, H, st, rl));
    }
    return ICZ_OK;
}

// ---- the LM-LSTM weight gradients
int Butd::bptt_lm_wgrad(BpttCall& c) {
    const int H = dims.H, D = dims.D, ldlm = D + H;
    const size_t sH = (size_t)c.Bs * H;
    const icz_butd_params& G = c.G;
    const GemmColGroup lm_groups[3] = {{tb.ctx, D, D, G.lm_w_ih, ldlm},                      // ctx_t
                                       {tb.h1 + sH, H, H, G.lm_w_ih + D, ldlm},              // h1_t
                                       {tb.h2, H, H, G.lm_w_hh, H}};                         // h2_{t-1}
    const int r = wslab_of(c.st);
    return gemm_tn_groups(tb.dGlm, 4 * H, 4 * H, c.TB, lm_groups, 3, tb.wslab[r], tb.wslab_floats[r], c.rl, c.st);   // grouped at 4096 x 4096: 227 us against 123 + 2 x 85
}

// ---- the attention block's tail, on the tail branch's stream: its two weight gradients, d enc_ctx, the bias sums of every layer
//      below `predict` and weight-norm backward of the block's three layers
int Butd::bptt_attention_tail(BpttCall& c) {
    const int B = c.B, T = c.T, Bs = c.Bs, roff = c.roff, TB = c.TB, K = c.K, n_img = c.n_img;
    const int H = dims.H, D = dims.D, A = dims.A, R = cur_R;
    const bool ad = adaptive();
    // parts of the grouped d enc_ctx kernel: DENC_GROUP_REGS regions each (more than ATT_PARTS only above 64 regions; n_img <= B / 2
    // images there, so tb.dwaff's B x ATT_PARTS blocks still hold them)
    const int gparts = att_denc_group_parts(R, ATT_PARTS);
    const size_t sH = (size_t)Bs * H;
    const icz_butd_params& G = c.G;
    const float* const feats = cur_feats;
    const int32_t* const imgk = c.imgk;
    hipStream_t const st = c.tail.st();
    ICZ_TRY(wgrad(tb.dDec, A, A, tb.h1 + sH, H, H, TB, tb.dWdec, H, st));
    {   // d enc_ctx (sum over time) and the affine-weight partials, from the ds_t recorded by the loop
        AttBwdDencArgs ea = {enc_ctx, tb.dec + (size_t)roff * A, tb.dS + (size_t)roff * R, w_aff, tb.dEnc, tb.dwaff, B, R, A, T,
                             cur_train ? (rng.att_mask ? 1 : 2) : 0, rng.att_mask, (size_t)B * R * A, d_seed, (uint32_t)RNG_ATT, Bs, imgk, cnt};
        if (K > 1 && group_att) {       // sample_n, grouped: the K rows of an image in one workgroup, summed into d enc_ctx[img]
            ea.denc = tb.dEncImg;
            launch_att_bwd_denc(ad, ea, n_img, K, gparts, st);
        } else {
            launch_att_bwd_denc(ad, ea, B, 0, ATT_PARTS, st);
            if (K > 1) {                // sample_n, per row: d enc_ctx of the B K rows, then the K rows of an image added in k order
                const size_t N = (size_t)R * A;
                launch_rowgroup_sum(tb.dEnc, n_img, K, N, tb.dEncImg, st);
            }
        }
    }
    const float* const denc = K > 1 ? tb.dEncImg : tb.dEnc;
    // d affine partials: one [parts, A] block per decoder row, or per image behind the grouped kernel
    const int waff_rows = K > 1 && group_att ? n_img * gparts : B * ATT_PARTS;
    ICZ_TRY(wgrad(denc, A, A, feats, D, D, n_img * R, tb.dWenc, D, st));
    {   // bias gradients: five column sums (+ the b_hh copies, + the identically zero affine bias: softmax shift invariance) in one launch
        ColsumTable ct = {};
        int nb = 0;
        auto add = [&](const float* X, int K, int N, int ldx, float* out, float* out2) {
            ct.j[ct.count++] = {X, K, N, ldx, out, out2, nb};
            nb += cdiv(N, 32);
        };
        add(tb.dGtd, TB, 4 * H, 4 * H, G.td_b_ih, G.td_b_hh);
        add(tb.dGlm, TB, 4 * H, 4 * H, G.lm_b_ih, G.lm_b_hh);
        add(tb.dDec, TB, A, A, G.dec_att_b, nullptr);
        add(denc, n_img * R, A, A, G.enc_att_b, nullptr);
        add(tb.dwaff, waff_rows, A, A, tb.dWaff, nullptr);
        add(tb.dwaff, 0, 1, 1, G.affine_b, nullptr);
        hipLaunchKernelGGL(colsum_multi_kernel, dim3(nb), dim3(256), 0, st, ct);
    }
    {   // the attention block's three weight-normed layers
        WeightNormBwdTable wt = {};
        int nb = 0;
        auto add = [&](const float* dw, int lddw, const float* v, const float* g, const float* norm, float* dv, float* dg, int rows, int cols) {
            wt.j[wt.count++] = {dw, lddw, v, g, norm, dv, dg, rows, cols, nb};
            nb += cdiv(rows, 4);
        };
        add(tb.dWenc, D, P.enc_att_v, P.enc_att_g, n_enc, G.enc_att_v, G.enc_att_g, A, D);
        add(tb.dWdec, H, P.dec_att_v, P.dec_att_g, n_dec, G.dec_att_v, G.dec_att_g, A, H);
        add(tb.dWaff, A, P.affine_v, P.affine_g, n_aff, G.affine_v, G.affine_g, 1, A);
        hipLaunchKernelGGL(weight_norm_bwd_multi_kernel, dim3(nb), dim3(256), 0, st, wt);
    }
    return ICZ_OK;
}

}  // namespace icz

// ================================================================================================
using namespace icz;
extern "C" {

int icz_butd_sample(icz_butd_t* h, const float* feats, int32_t B, int32_t max_len, const icz_rng* rng,
                    int64_t* seq_out, float* logprobs_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Butd*>(h)->sample(feats, B, max_len, rng, seq_out, logprobs_out, (hipStream_t)stream);
}
int icz_butd_sample_n(icz_butd_t* h, const float* feats, int32_t B, int32_t K, int32_t max_len, const icz_rng* rng,
                      int64_t* seq_out, float* logprobs_out, void* stream) {
    ICZ_REQUIRE(K >= 2 && K <= ATT_CTX_MAX_G, "icz_butd_sample_n: K=%d samples per image outside 2..%d", K, ATT_CTX_MAX_G);
    ICZ_REQUIRE(h, "icz_butd_sample_n: null handle");
    return reinterpret_cast<Butd*>(h)->sample_n(feats, B, K, max_len, rng, seq_out, logprobs_out, (hipStream_t)stream);
}
int icz_butd_scst_rollouts(icz_butd_t* h, const float* feats, int32_t B, int32_t max_len, const icz_rng* rng,
                           int64_t* greedy_ids_out, int64_t* seq_out, float* logprobs_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Butd*>(h)->rollouts(feats, B, max_len, rng, greedy_ids_out, seq_out, logprobs_out, (hipStream_t)stream);
}
int icz_butd_sample_backward(icz_butd_t* h, const float* reward, const icz_butd_params* grads, float* loss_out,
                             float* mask_sum_out, float mask_sum_global, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::ROLLOUT, "butd", "butd sample_backward"};
    hd.rollout = {reward, nullptr, loss_out, nullptr, mask_sum_out};
    hd.norm_global = mask_sum_global;
    return reinterpret_cast<Butd*>(h)->backward(hd, grads, (hipStream_t)stream);
}
// sample_backward with an SCST objective (scst_objective.hip) in the place of RewardCriterion
int icz_butd_sample_backward_objective(icz_butd_t* h, const icz_scst_objective* obj, const icz_butd_params* grads, float* loss_out3,
                                       float* ent_out, float* mask_sum_out, float mask_sum_global, void* stream) {
    ScstObjective o;
    ICZ_TRY(icz::scst_objective_args("icz_butd_sample_backward_objective", obj, obj ? obj->K : 1, 1, &o));
    ICZ_REQUIRE(grads && loss_out3, "icz_butd_sample_backward_objective: null argument");
    ICZ_REQUIRE(h, "icz_butd_sample_backward_objective: null handle");
    LossHead hd = {LossHead::ROLLOUT, "butd", "butd sample_backward_objective"};
    hd.rollout = {nullptr, &o, loss_out3, ent_out, mask_sum_out};
    hd.objective = obj;
    hd.norm_global = mask_sum_global;
    return reinterpret_cast<Butd*>(h)->backward(hd, grads, (hipStream_t)stream);
}
int icz_butd_sample_backward_dlogp(icz_butd_t* h, const float* dlogp, const icz_butd_params* grads, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::ROLLOUT_DLOGP, "butd", "butd sample_backward_dlogp"};
    hd.upstream = dlogp;
    return reinterpret_cast<Butd*>(h)->backward(hd, grads, (hipStream_t)stream);
}
int icz_butd_xe_backward_dlogits(icz_butd_t* h, const float* dpacked, const icz_butd_params* grads, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::XE_DLOGITS, "butd", "butd xe_backward_dlogits"};
    hd.upstream = dpacked;
    return reinterpret_cast<Butd*>(h)->backward(hd, grads, (hipStream_t)stream);
}
int icz_butd_sample_mask_sum(icz_butd_t* h, float* mask_sum_out, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Butd*>(h)->sample_mask_sum(mask_sum_out, (hipStream_t)stream);
}
int icz_butd_saved_alphas(icz_butd_t* h, float* alphas_out, void* stream) {
    ICZ_REQUIRE(h && alphas_out, "icz_butd_saved_alphas: null argument");
    Butd* b = reinterpret_cast<Butd*>(h);
    ICZ_REQUIRE(b->mode != 0 && b->tb.alpha, "icz_butd_saved_alphas: no forward pass stored");
    ICZ_REQUIRE(b->cur_row0 == 0, "icz_butd_saved_alphas: not available behind a merged SCST rollout (set option merge_small = 0)");
    launch_saved_alphas(b->tb.alpha, b->cur_T, b->cur_B, 1, b->cur_R, alphas_out, (hipStream_t)stream);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}
int icz_butd_set_scheduled_sampling(icz_butd_t* h, float ss_prob, const float* gate_uniforms, const float* draw_uniforms) {
    return set_scheduled_sampling("icz_butd_set_scheduled_sampling", reinterpret_cast<Butd*>(h), ss_prob, gate_uniforms, draw_uniforms);
}
int icz_butd_xe_forward(icz_butd_t* h, const float* feats, const int64_t* captions, int32_t B, int32_t L,
                        const int32_t* lengths_host, const icz_rng* rng, int32_t train, float* packed_logits_out,
                        void* stream) {
    ICZ_REQUIRE(h, "null handle");
    return reinterpret_cast<Butd*>(h)->xe_forward(feats, captions, B, L, lengths_host, rng, train, packed_logits_out, (hipStream_t)stream);
}
int icz_butd_xe_forward_n(icz_butd_t* h, const float* feats, const int64_t* captions, int32_t B, int32_t K, int32_t L,
                          const int32_t* lengths_host, const icz_rng* rng, int32_t train, float* logits_out, void* stream) {
    ICZ_TRY(xe_forward_n_args("icz_butd_xe_forward_n", feats, captions, B, K, L, lengths_host));
    ICZ_REQUIRE(h, "icz_butd_xe_forward_n: null handle");
    return reinterpret_cast<Butd*>(h)->xe_forward_n(feats, captions, B, K, L, lengths_host, rng, train, logits_out, (hipStream_t)stream);
}
int icz_butd_xe_backward(icz_butd_t* h, float smoothing, const icz_butd_params* grads, float* loss_out,
                         float n_tokens_global, void* stream) {
    ICZ_REQUIRE(h, "null handle");
    LossHead hd = {LossHead::XE, "butd", "butd xe_backward"};
    hd.smoothing = smoothing; hd.loss_out = loss_out; hd.norm_global = n_tokens_global;
    return reinterpret_cast<Butd*>(h)->backward(hd, grads, (hipStream_t)stream);
}
int icz_butd_xe_backward_distill(icz_butd_t* h, const icz_distill_opts* opts, const icz_butd_params* grads, float* loss_out3,
                                 float n_tokens_global, void* stream) {
    Butd* b = reinterpret_cast<Butd*>(h);
    DistillArgs a;
    ICZ_TRY(distill_args("icz_butd_xe_backward_distill", opts, b ? b->dims.V : -1, &a));
    ICZ_REQUIRE(grads && loss_out3, "icz_butd_xe_backward_distill: null grads or loss");
    ICZ_REQUIRE(h, "icz_butd_xe_backward_distill: null handle");
    LossHead hd = {LossHead::XE_DISTILL, "butd", "butd xe_backward_distill"};
    hd.distill = &a; hd.loss_out = loss_out3; hd.norm_global = n_tokens_global;
    return b->backward(hd, grads, (hipStream_t)stream);
}
int icz_butd_xe_backward_swor(icz_butd_t* h, const icz_swor_opts* opts, int32_t rows, const icz_butd_params* grads, float* loss_out,
                              void* stream) {
    SworArgs a;
    ICZ_TRY(swor_args("icz_butd_xe_backward_swor", opts, rows, &a));
    ICZ_REQUIRE(grads && loss_out, "icz_butd_xe_backward_swor: null grads or loss");
    ICZ_REQUIRE(h, "icz_butd_xe_backward_swor: null handle");
    LossHead hd = {LossHead::XE_SWOR, "butd", "butd xe_backward_swor"};
    hd.swor = &a; hd.swor_rows = rows; hd.loss_out = loss_out;
    return reinterpret_cast<Butd*>(h)->backward(hd, grads, (hipStream_t)stream);
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// One "X2 = d dec . w_dec, then the TD-LSTM backward" step of Butd::bptt_loop on given buffers (include/icz.h)
int icz_test_bptt_dh1_step(int32_t route, int32_t rows, int32_t H, int32_t A, const float* ddec, const float* w_dec, const float* carry,
                           int32_t ns_carry, int32_t rows_carry, const float* x1, int32_t ns_x1, int32_t ld_x1, const float* dc_in,
                           const float* gates, const float* c_prev, const float* c_cur, float* dgates, float* dc_prev, const int32_t* live,
                           const int32_t* carry_live, float* x2_slabs, size_t x2_floats, int32_t* nsplit_out, int32_t* route_out, void* stream) {
    const char* who = "icz_test_bptt_dh1_step";
    ICZ_REQUIRE(route >= -1 && route <= 1, "%s: route=%d (-1: as the loop picks, 0: two launches, 1: fused)", who, route);
    ICZ_REQUIRE(rows >= 1 && rows <= 64 && H >= 4 && H % 4 == 0 && A >= 4 && A % 4 == 0, "%s: rows=%d (1..64), H=%d, A=%d (H and A in whole groups of 4)", who, rows, H, A);
    ICZ_REQUIRE(ddec && w_dec && x1 && gates && c_cur && dgates && dc_prev, "%s: null argument", who);
    ICZ_REQUIRE(al16(ddec) && al16(w_dec), "%s: ddec and w_dec must be 16-byte aligned", who);
    ICZ_REQUIRE(ns_x1 >= 1 && ld_x1 >= H, "%s: ns_x1=%d, ld_x1=%d (at least H)", who, ns_x1, ld_x1);
    ICZ_REQUIRE(!carry || (ns_carry >= 1 && rows_carry >= 1), "%s: ns_carry=%d, rows_carry=%d", who, ns_carry, rows_carry);
    ICZ_REQUIRE(!dc_in || rows_carry >= 1, "%s: dc_in with rows_carry=%d", who, rows_carry);
    const bool takes = lstm_bwd_dh1_fused_takes(rows, H, A);
    ICZ_REQUIRE(route != 1 || takes, "%s: the fused kernel does not take rows=%d, H=%d, A=%d", who, rows, H, A);
    const bool fdh = route == 1 || (route == -1 && takes);
    const int ns = dh1_split(rows, H, A);
    if (nsplit_out) *nsplit_out = ns;
    if (route_out) *route_out = fdh ? 1 : 0;
    hipStream_t const st = (hipStream_t)stream;
    LstmBwdArgs a = {};
    a.dh_a = carry; a.ns_a = ns_carry; a.lda_a = H; a.rows_a = rows_carry;
    a.dh_b = x1; a.ns_b = ns_x1; a.lda_b = ld_x1; a.rows_b = rows;
    a.dc_in = dc_in; a.dc_in_rows = rows_carry;
    a.gates = gates; a.c_prev = c_prev; a.c_cur = c_cur; a.dgates = dgates; a.dc_prev = dc_prev;
    a.rows = rows; a.H = H; a.live = live; a.carry_live = carry_live;
    if (fdh) return launch_dh1_fused(a, ddec, w_dec, A, st);
    ICZ_REQUIRE(x2_slabs && al16(x2_slabs) && gemm_slab_floats(rows, H, ns) <= x2_floats, "%s: the two-launch route needs %d slabs of rows x H floats (16-byte aligned)", who, ns);
    GemmArgs g = gemm_args({{ddec, w_dec, A, H, A}}, rows, H, x2_slabs, H, live);
    int ns2 = 1;
    ICZ_TRY(gemm_slabs(GEMM_NN, g, split_backward(Butd::STEP_WGS), x2_slabs, x2_floats, &ns2, st, who));
    a.dh_c = x2_slabs; a.ns_c = ns2; a.lda_c = H; a.rows_c = rows;
    const DropCfg d_off = {0, nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL(lstm_bwd_point_kernel, dim3(cdiv(H, 256), rows), dim3(256), 0, st, a, d_off);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
