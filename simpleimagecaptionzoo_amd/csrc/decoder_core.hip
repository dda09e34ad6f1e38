// The out-of-line half of decoder_core.h (caption loss head, greedy select tail, C ABI helpers) and the library's error slot.
#include <stdarg.h>

#include "decoder_core.h"
#include "support_kernels.h"
#include "token_kernels.h"

namespace icz {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ------------------------------------------------------------------------------------------------
__global__ void captions_to_tok_kernel(const int64_t* __restrict__ cap, int B, int L, int T, int64_t* __restrict__ tok) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;   // i = t*B + b
    if (i >= T * B) return;
    int t = i / B, b = i % B;
    tok[i] = cap[(size_t)b * L + t];
}
__global__ void gather_packed_kernel(const float* __restrict__ logit, int V, int ldl, int B, const int* __restrict__ row_off,
                                     const int* __restrict__ rows_t, int T, float* __restrict__ out) {
    // grid (V/256, T*B): copy logits of active (t,b) to packed row row_off[t] + b
    const int tb_ = blockIdx.y, t = tb_ / B, b = tb_ % B;
    if (b >= rows_t[t]) return;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    out[(size_t)(row_off[t] + b) * V + v] = logit[(size_t)tb_ * ldl + v];
}
__global__ void scatter_packed_kernel(const float* __restrict__ dpacked, int V, int ldl, int B, const int* __restrict__ row_off,
                                      const int* __restrict__ rows_t, int T, float* __restrict__ logit) {
    // inverse of gather_packed_kernel; inactive rows and pad columns become zero
    const int tb_ = blockIdx.y, t = tb_ / B, b = tb_ % B;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= ldl) return;
    float g = 0.f;
    if (b < rows_t[t] && v < V) g = dpacked[(size_t)(row_off[t] + b) * V + v];
    logit[(size_t)tb_ * ldl + v] = g;
}

int CaptionHead::alloc_scalars(DeviceBuffers& m) {
    ICZ_TRY(m.alloc((void**)&d_seed, 16));
    return m.alloc((void**)&d_msum, 16);
}

int CaptionHead::alloc_loss_buffers(DeviceBuffers& m, size_t TB, size_t B, size_t T) {
    ICZ_TRY(m.alloc((void**)&coef, sizeof(float) * TB));
    ICZ_TRY(m.alloc((void**)&lse, sizeof(float) * TB));
    ICZ_TRY(m.alloc((void**)&loss_rows, sizeof(float) * TB));
    ICZ_TRY(m.alloc((void**)&kd_rows, sizeof(float) * TB));
    ICZ_TRY(m.alloc((void**)&draw, sizeof(int32_t) * TB));
    ICZ_TRY(m.alloc((void**)&unf, B));
    ICZ_TRY(m.alloc((void**)&nunf, sizeof(int) * T));
    ICZ_TRY(m.alloc((void**)&gunf, B));
    ICZ_TRY(m.alloc((void**)&gnunf, sizeof(int) * T));
    ICZ_TRY(m.alloc((void**)&live_rows, 16));
    ICZ_TRY(m.alloc((void**)&pack_idx, sizeof(int) * 2 * T));
    pack_cap = (int)(2 * T);
    ICZ_TRY(m.alloc((void**)&obj_img, sizeof(double) * B));
    ICZ_TRY(m.alloc((void**)&obj_mimg, sizeof(int) * B));
    ICZ_TRY(m.alloc((void**)&obj_scal, 16));
    ICZ_TRY(m.alloc((void**)&swor_coef, sizeof(float) * 2 * B));
    ICZ_TRY(m.alloc((void**)&swor_cs, sizeof(double) * 2 * B));
    return ICZ_OK;
}

void CaptionHead::drop_loss_buffers() {
    coef = lse = loss_rows = kd_rows = nullptr; draw = nullptr; unf = gunf = nullptr; nunf = gnunf = live_rows = pack_idx = nullptr;
    pack_cap = 0;
    obj_img = nullptr; obj_mimg = nullptr; obj_scal = nullptr;
    swor_coef = nullptr; swor_cs = nullptr;
    mode = 0;
}

int CaptionHead::require_mode(int want, const char* who) const {
    ICZ_REQUIRE(mode == want, want == 1 ? "%s: no rollout stored (call icz_%s_sample first)" : "%s: no XE forward stored (call icz_%s_xe_forward first)",
                who, who);
    return ICZ_OK;
}

int CaptionHead::xe_steps(const char* who, const int32_t* lengths, int B, int L, int* T_out) {
    int T = 0;
    for (int b = 0; b < B; ++b) {
        ICZ_REQUIRE(lengths[b] >= 1 && lengths[b] <= L - 1, "%s xe_forward: length %d out of range 1..%d", who, lengths[b], L - 1);
        ICZ_REQUIRE(b == 0 || lengths[b] <= lengths[b - 1], "%s xe_forward: lengths must be sorted in decreasing order (Engine.py:179)", who);
        if (lengths[b] > T) T = lengths[b];
    }
    *T_out = T;
    return ICZ_OK;
}

void CaptionHead::begin_xe(const int32_t* lengths, int B, int T, int L, const int64_t* captions, bool train, uint64_t seed, hipStream_t st) {
    hipLaunchKernelGGL(set_scalars_kernel, dim3(1), dim3(1), 0, st, d_seed, seed, (float*)nullptr, 0.f);
    mode = 2; cur_B = B; cur_T = T; cur_L = L; cur_train = train; cur_captions = captions; cur_ss_prob = ss_prob;
    rows_t.assign(T, 0);
    n_tokens = 0;
    for (int t = 0; t < T; ++t) {
        int c = 0;
        for (int b = 0; b < B; ++b) c += lengths[b] > t;
        rows_t[t] = c;
        n_tokens += c;
    }
}

void CaptionHead::begin_rollout(int rows, int T, const int64_t* seq_out, const float* logp_out, uint64_t seed, hipStream_t st) {
    hipLaunchKernelGGL(set_scalars_kernel, dim3(1), dim3(1), 0, st, d_seed, seed, (float*)nullptr, 0.f);
    mode = 1; cur_B = rows; cur_T = T; cur_train = true; cur_seq = seq_out; cur_logp = logp_out;
    rows_t.assign(T, rows);
}

int CaptionHead::check_loss_head(const LossHead& hd, const void* grads) const {
    ICZ_TRY(require_mode(hd.rollout_kind() ? 1 : 2, hd.fam));
    switch (hd.kind) {
    case LossHead::XE: ICZ_REQUIRE(grads, "%s: null grads", hd.who); break;
    case LossHead::XE_DISTILL: ICZ_TRY(require_teacher_forced(hd.who)); break;
    case LossHead::XE_SWOR: ICZ_TRY(check_swor(hd.fam, hd.swor_rows)); break;
    case LossHead::XE_DLOGITS:
    case LossHead::ROLLOUT_DLOGP: ICZ_REQUIRE(hd.upstream && grads, "%s: null argument", hd.who); break;
    case LossHead::ROLLOUT:
        if (hd.objective) ICZ_TRY(check_objective(hd.who, hd.objective));
        else ICZ_REQUIRE(hd.rollout.reward && grads, "%s: null argument", hd.who);
        break;
    }
    return ICZ_OK;
}

int CaptionHead::launch_loss_head(const LossHead& hd, float* logits, int V, int ldl, hipStream_t st, int rows, int row0) {
    switch (hd.kind) {
    case LossHead::XE:
        if (hd.group_len) return xe_group_loss(hd.group_len, hd.smoothing, hd.norm_global, logits, V, ldl, hd.loss_out, st);
        return xe_loss(hd.smoothing, hd.norm_global, logits, V, ldl, hd.loss_out, st);
    case LossHead::XE_DISTILL: return distill_loss(*hd.distill, hd.norm_global, logits, V, ldl, hd.loss_out, st);
    case LossHead::XE_SWOR: return swor_loss(*hd.swor, logits, V, ldl, hd.loss_out, st);
    case LossHead::XE_DLOGITS: return scatter_packed(hd.upstream, V, ldl, logits, st);
    case LossHead::ROLLOUT: return rollout_head(hd.rollout, logits, V, ldl, st, rows, row0);
    case LossHead::ROLLOUT_DLOGP:       // the upstream d loss / d logprobs in the place of reinforce's coefficients
        ICZ_CHECK_HIP(hipMemcpyAsync(coef, hd.upstream, sizeof(float) * cur_B * cur_T, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(reinforce_dlogits_kernel, dim3(cdiv(ldl, 256), cur_T * (rows ? rows : cur_B)), dim3(256), 0, st, logits, V, ldl, draw, lse,
                           (const float*)coef, cur_B, cur_T, rows, row0);
        ICZ_CHECK_HIP(hipGetLastError());
        return ICZ_OK;
    }
    return ICZ_OK;
}

int CaptionHead::begin_backward(const LossHead& hd, bool in_graph, float* logits, int V, int ldl, hipStream_t st, int rows, int row0) {
    if (hd.kind == LossHead::ROLLOUT) set_msum_global(hd.norm_global, st);      // (a captured graph reads the device scalar)
    if (!in_graph) ICZ_TRY(launch_loss_head(hd, logits, V, ldl, st, rows, row0));
    mode = 0;                     // the stored logits are consumed
    return ICZ_OK;
}

void CaptionHead::captions_to_tok(int64_t* tok, hipStream_t st) const {
    hipLaunchKernelGGL(captions_to_tok_kernel, dim3(cdiv(cur_T * cur_B, 256)), dim3(256), 0, st, cur_captions, cur_B, cur_L, cur_T, tok);
}

// device copy of the packed-sequence index: row_off[t] (first packed row of step t) and rows_t[t]
int CaptionHead::upload_pack_index(hipStream_t st) {
    const int T = cur_T;
    std::vector<int> hostv(2 * T);
    int acc = 0;
    for (int t = 0; t < T; ++t) { hostv[t] = acc; hostv[T + t] = rows_t[t]; acc += rows_t[t]; }
    ICZ_REQUIRE(pack_idx && 2 * T <= pack_cap, "pack index capacity");
    ICZ_CHECK_HIP(hipMemcpyAsync(pack_idx, hostv.data(), sizeof(int) * 2 * T, hipMemcpyHostToDevice, st));
    ICZ_CHECK_HIP(hipStreamSynchronize(st));   // the host vector goes out of scope
    return ICZ_OK;
}

int CaptionHead::gather_packed(const float* logit, int V, int ldl, float* packed_out, hipStream_t st) {
    ICZ_TRY(upload_pack_index(st));
    const int T = cur_T;
    hipLaunchKernelGGL(gather_packed_kernel, dim3(cdiv(V, 256), T * cur_B), dim3(256), 0, st, logit, V, ldl, cur_B, pack_idx, pack_idx + T, T,
                       packed_out);
    return ICZ_OK;
}

int CaptionHead::scatter_packed(const float* dpacked, int V, int ldl, float* logit, hipStream_t st) {
    ICZ_TRY(upload_pack_index(st));
    const int T = cur_T;
    hipLaunchKernelGGL(scatter_packed_kernel, dim3(cdiv(ldl, 256), T * cur_B), dim3(256), 0, st, dpacked, V, ldl, cur_B, pack_idx, pack_idx + T, T,
                       logit);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int launch_xe_loss(float* logits, int V, int ldl, const int64_t* captions, int L, int B, int T, const int* rows_t, float smoothing, float n,
                   const float* n_dev, float* loss_rows, float* loss_out, hipStream_t st) {
    ICZ_CHECK_HIP(hipMemsetAsync(loss_rows, 0, sizeof(float) * T * B, st));
    ICZ_REQUIRE(T <= XE_MAX_T, "xe_backward: %d steps exceed %d", T, XE_MAX_T);
    XeRows xr = {};
    for (int t = 0; t < T; ++t) xr.n[t] = rows_t[t];
    hipLaunchKernelGGL(xe_loss_dlogits_kernel, dim3(B, T), dim3(256), 0, st, logits, V, ldl, captions, L, B, xr, smoothing, 1.0f / n, n_dev,
                       loss_rows);
    if (loss_out) hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, st, loss_rows, T * B, 1.0f / n, n_dev, loss_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int CaptionHead::xe_loss(float smoothing, float n_tokens_global, float* logits, int V, int ldl, float* loss_out, hipStream_t st) {
    const float n = n_tokens_global > 0.f ? n_tokens_global : (float)n_tokens;
    const float* n_dev = n_tokens_global < 0.f ? d_msum : nullptr;      // < 0: the device scalar handed over by *_set_*_global
    return launch_xe_loss(logits, V, ldl, cur_captions, cur_L, cur_B, cur_T, rows_t.data(), smoothing, n, n_dev, loss_rows, loss_out, st);
}

// ------------------------------------------------------------------------------------------------
// The grouped XE forward (K captions per image, rows image-major in any length order): per-row step counts on the device in the place
// of rows_t.  The host array reaches the device as kernel arguments, 256 counts per launch: no copy from the caller's pageable memory,
// so nothing to wait for and nothing that outlives the call.
struct LenChunk { int32_t n[256]; };
__global__ void set_lengths_kernel(int32_t* __restrict__ dst, int n, LenChunk c) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = c.n[threadIdx.x];
}
void upload_lengths(int32_t* dst, const int32_t* lengths_host, int n, hipStream_t st) {
    for (int i = 0; i < n; i += 256) {
        LenChunk c = {};
        const int m = n - i < 256 ? n - i : 256;
        for (int j = 0; j < m; ++j) c.n[j] = lengths_host[i + j];
        hipLaunchKernelGGL(set_lengths_kernel, dim3(1), dim3(256), 0, st, dst + i, m, c);
    }
}
// tok[t, row] = captions[row, t] while the row runs, <pad> behind its end (whatever the caller's row holds there)
__global__ void captions_to_tok_len_kernel(const int64_t* __restrict__ cap, int rows, int L, int T, const int32_t* __restrict__ len,
                                           int64_t* __restrict__ tok) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // i = t * rows + row
    if (i >= T * rows) return;
    const int t = i / rows, r = i % rows;
    tok[i] = t < len[r] ? cap[(size_t)r * L + t] : 0;
}
void launch_captions_to_tok_len(const int64_t* captions, int rows, int L, int T, const int32_t* len, int64_t* tok, hipStream_t st) {
    hipLaunchKernelGGL(captions_to_tok_len_kernel, dim3(cdiv(T * rows, 256)), dim3(256), 0, st, captions, rows, L, T, len, tok);
}
// out [rows, T, V] = logit [T rows, ldl] at the active (row, t), zeros elsewhere
__global__ void gather_rows_kernel(const float* __restrict__ logit, int V, int ldl, int rows, int T, const int32_t* __restrict__ len,
                                   float* __restrict__ out) {
    const int tr = blockIdx.y, t = tr / rows, r = tr % rows;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    out[((size_t)r * T + t) * V + v] = t < len[r] ? logit[(size_t)tr * ldl + v] : 0.f;
}
void launch_gather_rows(const float* logit, int V, int ldl, int rows, int T, const int32_t* len, float* out, hipStream_t st) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(cdiv(V, 256), T * rows), dim3(256), 0, st, logit, V, ldl, rows, T, len, out);
}

int launch_xe_group_loss(float* logits, int V, int ldl, const int64_t* captions, int L, int rows, int T, const int32_t* len, float smoothing,
                         float n, const float* n_dev, float* loss_rows, float* loss_out, hipStream_t st) {
    ICZ_REQUIRE(ldl % 4 == 0 && ((uintptr_t)logits & 15) == 0, "grouped xe loss: inactive rows are zeroed 16 bytes at a time: ldl=%d, logits %p", ldl,
                (void*)logits);
    ICZ_REQUIRE(T >= 1 && T <= 65535, "grouped xe loss: %d steps exceed the grid", T);
    hipLaunchKernelGGL(xe_group_loss_dlogits_kernel, dim3(rows, T), dim3(256), 0, st, logits, V, ldl, captions, L, rows, len, smoothing, 1.0f / n,
                       n_dev, loss_rows);
    if (loss_out) hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, st, loss_rows, T * rows, 1.0f / n, n_dev, loss_out);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int CaptionHead::xe_group_loss(const int32_t* len, float smoothing, float n_tokens_global, float* logits, int V, int ldl, float* loss_out,
                               hipStream_t st) {
    const float n = n_tokens_global > 0.f ? n_tokens_global : (float)n_tokens;
    const float* n_dev = n_tokens_global < 0.f ? d_msum : nullptr;
    return launch_xe_group_loss(logits, V, ldl, cur_captions, cur_L, cur_B, cur_T, len, smoothing, n, n_dev, loss_rows, loss_out, st);
}

void CaptionHead::set_msum_global(float msum_global, hipStream_t st) const {
    if (msum_global >= 0.f)
        hipLaunchKernelGGL(set_scalars_kernel, dim3(1), dim3(1), 0, st, (uint64_t*)nullptr, (uint64_t)0, d_msum, msum_global);
}

int launch_reinforce(const float* logp, const int64_t* seq, const float* reward, int B, int T, const float* msum_dev, float* coef, float* loss_out,
                     float* msum_out, float* logits, int V, int ldl, const int32_t* draw, const float* lse, int rows, int row0, hipStream_t st) {
    hipLaunchKernelGGL(reinforce_loss_kernel, dim3(1), dim3(256), 0, st, logp, seq, reward, B, T, msum_dev, coef, loss_out, msum_out);
    hipLaunchKernelGGL(reinforce_dlogits_kernel, dim3(cdiv(ldl, 256), T * (rows ? rows : B)), dim3(256), 0, st, logits, V, ldl, draw, lse,
                       (const float*)coef, B, T, rows, row0);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int CaptionHead::reinforce(const float* reward, float* logits, int V, int ldl, float* loss_out, float* msum_out, hipStream_t st, int rows, int row0) {
    return launch_reinforce(cur_logp, cur_seq, reward, cur_B, cur_T, d_msum, coef, loss_out, msum_out, logits, V, ldl, draw, lse, rows, row0, st);
}

// ------------------------------------------------------------------------------------------------
// route: 0 = by the view (every decoder), 1 = the two-kernel form, 2 = greedy_select_kernel (icz_test_greedy_select, which checks that
// the form can take the view: the two-kernel form reads finished rows only and keeps no <end> counters)
void launch_greedy_select(const LogitsView& lv, const DecodeMember::EmbSlot& e, int rows, int V, float* amax_val, int* amax_idx, int64_t* it,
                          int64_t* ids_out, int T, int t, uint8_t* gunf, int* gn, hipStream_t st, int route) {
    if (route == 2 || (route == 0 && lv.ns > 1))         // 33 - 64 rows: the slabs of the vocabulary projection -> token + next embedding in one launch
        hipLaunchKernelGGL(greedy_select_kernel, dim3(rows), dim3(1024), 0, st, lv.p, V, lv.ld, lv.ns, lv.slab_stride, lv.bias, e.table, e.E, e.emb,
                           it, ids_out, T, t, e.relu, gunf, gn);
    else {
        hipLaunchKernelGGL(argmax_part_kernel, dim3(rows, ARGMAX_PARTS), dim3(256), 0, st, lv.p, V, lv.ld, ARGMAX_PARTS, amax_val, amax_idx);
        hipLaunchKernelGGL(embed_argmax_kernel, dim3(cdiv(e.E, 1024), rows), dim3(256), 0, st, (const float*)amax_val, (const int*)amax_idx,
                           ARGMAX_PARTS, e.table, e.E, e.emb, it, ids_out, T, t, e.relu);
    }
}

// ------------------------------------------------------------------------------------------------
int check_param_table(const char* who, const void* params, size_t bytes, uint32_t unaligned_ok) {
    const float* const* q = reinterpret_cast<const float* const*>(params);
    for (size_t i = 0; i < bytes / sizeof(float*); ++i) {
        ICZ_REQUIRE(q[i] != nullptr, "%s: parameter pointer %zu is null", who, i);
        ICZ_REQUIRE(((uintptr_t)q[i] & 15) == 0 || ((unaligned_ok >> i) & 1), "%s: parameter %zu not 16-byte aligned", who, i);
    }
    return ICZ_OK;
}

int set_scheduled_sampling(const char* who, CaptionHead* h, float ss_prob, const float* gate, const float* draw) {
    ICZ_REQUIRE(h, "%s: null handle", who);
    ICZ_REQUIRE(ss_prob >= 0.f && ss_prob <= 1.f, "%s: ss_prob %g outside [0, 1]", who, (double)ss_prob);
    h->ss_prob = ss_prob; h->ss_gate = gate; h->ss_draw = draw;
    return ICZ_OK;
}

int set_norm_global(const char* who, CaptionHead* h, const float* norm_dev, void* stream) {
    ICZ_REQUIRE(h && norm_dev, "%s: null argument", who);
    ICZ_CHECK_HIP(hipMemcpyAsync(h->d_msum, norm_dev, sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ICZ_OK;
}

}  // namespace icz

extern "C" {
int icz_test_side_branch(int32_t fail_at, int32_t inline_branch, float* out2, void* stream) {
    using namespace icz;
    ICZ_REQUIRE(out2 && fail_at >= -1 && fail_at <= 3, "icz_test_side_branch: bad arguments");
    static SideStream* const side = new SideStream();      // (never destroyed: they would outlive the runtime at process exit)
    static GraphCache* const gc = new GraphCache(4);
    ICZ_TRY(side->ensure());
    // (fail_at in the key: a failing call must capture, not replay the graph of an earlier call; it leaves no entry behind)
    return gc->run({(uintptr_t)(fail_at + 1), (uintptr_t)(inline_branch != 0), (uintptr_t)out2}, (hipStream_t)stream, [&](hipStream_t st) -> int {
        int stage = 0;
        auto behind = [&]() -> int {
            ICZ_REQUIRE(stage++ != fail_at, "side-branch test: stage %d", fail_at);
            return ICZ_OK;
        };
        SideStream::Branch b(inline_branch ? nullptr : side, 0);
        ICZ_TRY(b.fork(st));
        hipLaunchKernelGGL(set_scalars_kernel, dim3(1), dim3(1), 0, st, (uint64_t*)nullptr, (uint64_t)0, out2, 1.0f);
        ICZ_TRY(behind());
        ICZ_TRY(b.start());
        ICZ_TRY(behind());
        hipLaunchKernelGGL(set_scalars_kernel, dim3(1), dim3(1), 0, b.st(), (uint64_t*)nullptr, (uint64_t)0, out2 + 1, 2.0f);
        ICZ_TRY(behind());
        ICZ_TRY(b.finish());
        ICZ_TRY(behind());
        return b.join();
    });
}

// ------------------------------------------------------------------------------------------------
// Test entries of the token-choice and loss kernels (include/icz.h): the arguments are checked on the host, then the kernels go through
// the launch helpers the decoders use (launch_greedy_select, launch_sample_select, ss_select_launch, launch_xe_loss, launch_reinforce).
static inline bool tc_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int tc_embed_shape(const char* who, const float* table, const float* emb, int E) {
    ICZ_REQUIRE(table && emb, "%s: null embedding table or output", who);
    ICZ_REQUIRE(E >= 4 && E % 4 == 0, "%s: E=%d is not a positive multiple of 4", who, E);
    ICZ_REQUIRE(tc_al16(table) && tc_al16(emb), "%s: table and emb must be 16-byte aligned", who);
    return ICZ_OK;
}
static int tc_logits_shape(const char* who, const float* logits, int rows, int V, int ldl, int ns, int64_t slab_stride) {
    ICZ_REQUIRE(logits, "%s: null logits", who);
    ICZ_REQUIRE(rows >= 1 && rows <= (1 << 20), "%s: rows=%d", who, rows);
    ICZ_REQUIRE(V >= 1 && ldl >= V, "%s: V=%d, ldl=%d", who, V, ldl);
    ICZ_REQUIRE(ns >= 1 && ns <= 16, "%s: ns=%d outside 1..16", who, ns);
    ICZ_REQUIRE(ns == 1 || slab_stride >= (int64_t)(rows - 1) * ldl + V, "%s: slab_stride=%lld overlaps the rows of a slab", who, (long long)slab_stride);
    return ICZ_OK;
}

int icz_test_greedy_select(int32_t route, const float* logits, int32_t rows, int32_t V, int32_t ldl, int32_t ns, int64_t slab_stride,
                           const float* bias, const float* table, int32_t E, int32_t relu, int32_t t, int32_t T, int64_t* ids_out,
                           int64_t* it_next, float* emb, uint8_t* unfinished, int32_t* n_unfinished, float* part_val, int32_t* part_idx,
                           void* stream) {
    using namespace icz;
    const char* who = "icz_test_greedy_select";
    ICZ_REQUIRE(route >= 0 && route <= 2, "%s: route=%d (0 as the decoders, 1 two kernels, 2 one kernel)", who, route);
    ICZ_TRY(tc_logits_shape(who, logits, rows, V, ldl, ns, slab_stride));
    ICZ_TRY(tc_embed_shape(who, table, emb, E));
    ICZ_REQUIRE(it_next, "%s: null it_next", who);
    ICZ_REQUIRE(T >= 1 && t >= 0 && t < T, "%s: t=%d outside 0..T-1 (T=%d)", who, t, T);
    ICZ_REQUIRE((unfinished == nullptr) == (n_unfinished == nullptr), "%s: unfinished and n_unfinished go together", who);
    const bool one_kernel = route == 2 || (route == 0 && ns > 1);
    if (!one_kernel) {
        ICZ_REQUIRE(ns == 1 && !bias && !unfinished, "%s: the two-kernel form reads finished rows (ns = 1, no bias) and keeps no <end> counters", who);
        ICZ_REQUIRE(part_val && part_idx, "%s: the two-kernel form needs part_val / part_idx [rows, %d]", who, ARGMAX_PARTS);
    }
    const LogitsView lv = {logits, bias, (size_t)slab_stride, ldl, ns};
    const DecodeMember::EmbSlot e = {table, emb, E, relu != 0};
    launch_greedy_select(lv, e, rows, V, part_val, part_idx, it_next, ids_out, T, t, unfinished, n_unfinished, (hipStream_t)stream, route);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_sample_select_max_vocab(void) { return (int)(icz::SEL_LDS_MAX / sizeof(float)); }

int icz_test_sample_select(const icz_sample_select_args* s, int32_t rows, void* stream) {
    using namespace icz;
    const char* who = "icz_test_sample_select";
    ICZ_REQUIRE(s, "%s: null arguments", who);
    ICZ_TRY(tc_logits_shape(who, s->logits, rows, s->V, s->ldl, s->ns, s->slab_stride));
    ICZ_REQUIRE(sel_row_fits_lds(s->V), "%s: a row of %d logits does not fit in LDS (at most %d)", who, s->V, icz_sample_select_max_vocab());
    ICZ_REQUIRE(s->ns == 1 || (s->bias && s->logits_store), "%s: slabs need bias and logits_store", who);
    ICZ_REQUIRE(s->T >= 1 && s->t >= 0 && s->t < s->T, "%s: t=%d outside 0..T-1 (T=%d)", who, s->t, s->T);
    ICZ_REQUIRE(s->unfinished && s->n_unfinished && s->seq_out && s->logp_out && s->it_next && s->draw_out && s->lse_out, "%s: null argument", who);
    ICZ_REQUIRE(s->uniforms || s->seed, "%s: uniforms or a seed", who);
    ICZ_REQUIRE(s->row0 >= 0 && s->row0 < rows, "%s: row0=%d outside 0..rows-1 (rows=%d)", who, s->row0, rows);
    ICZ_REQUIRE(s->row0 == 0 || (s->ids_out && s->g_unfinished && s->n_any), "%s: a merged launch needs ids_out, g_unfinished and n_any", who);
    ICZ_REQUIRE(s->emb_mode >= 0 && s->emb_mode <= 2, "%s: emb_mode=%d (0 none, 1 mask, 2 Philox)", who, s->emb_mode);
    SampleSelArgs a = {};
    a.logits = s->logits; a.V = s->V; a.ldl = s->ldl;
    if (s->ns > 1) { a.ns = s->ns; a.slab_stride = (size_t)s->slab_stride; a.bias = s->bias; a.logits_store = s->logits_store; }
    a.uniforms = s->uniforms; a.seed_p = s->seed; a.t = s->t; a.T = s->T;
    a.unfinished = s->unfinished; a.n_unfinished = s->n_unfinished; a.seq_out = s->seq_out; a.logp_out = s->logp_out;
    a.it_next = s->it_next; a.draw_out = s->draw_out; a.lse_out = s->lse_out; a.live_rows = s->live_rows;
    a.row0 = s->row0; a.ids_out = s->ids_out; a.g_unfinished = s->g_unfinished; a.n_any = s->n_any;
    if (s->emb_next) {
        ICZ_TRY(tc_embed_shape(who, s->emb_table, s->emb_next, s->E));
        ICZ_REQUIRE(s->emb_mode != 1 || (s->emb_mask && ((uintptr_t)s->emb_mask & 3) == 0), "%s: emb_mask null or not 4-byte aligned", who);
        ICZ_REQUIRE(s->emb_mode != 2 || s->seed, "%s: Philox keep bits need a seed", who);
        a.emb_table = s->emb_table; a.emb_next = s->emb_next; a.E = s->E;
        a.emb_drop = DropCfg{s->emb_mode, s->emb_mask, s->seed, RNG_EMB, (uint32_t)(s->t + 1), 0};     // step t + 1's embedding dropout
    }
    ICZ_TRY(launch_sample_select((hipStream_t)stream, rows, a));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_ss_select(const float* logits_prev, int32_t rows, int32_t B, int32_t V, int32_t ldl, int32_t t, float ss_prob, const float* gate,
                       const float* draw, const uint64_t* seed, int64_t* tok, void* stream) {
    using namespace icz;
    const char* who = "icz_test_ss_select";
    ICZ_TRY(tc_logits_shape(who, logits_prev, rows, V, ldl, 1, 0));
    ICZ_REQUIRE(sel_row_fits_lds(V), "%s: a row of %d logits does not fit in LDS (at most %d)", who, V, icz_sample_select_max_vocab());
    ICZ_REQUIRE(B >= rows && t >= 0 && t <= 65535, "%s: B=%d below rows=%d, or t=%d", who, B, rows, t);
    ICZ_REQUIRE(ss_prob >= 0.f && ss_prob <= 1.f, "%s: ss_prob %g outside [0, 1]", who, (double)ss_prob);
    ICZ_REQUIRE(tok && ((gate && draw) || seed), "%s: null argument (tok; gate and draw, or a seed)", who);
    ICZ_TRY(ss_select_launch((hipStream_t)stream, rows, logits_prev, ldl, V, t, B, ss_prob, gate, draw, seed, tok));
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_xe_loss(float* logits, int32_t V, int32_t ldl, const int64_t* captions, int32_t L, int32_t B, int32_t T, const int32_t* rows_t,
                     float smoothing, float n_tokens, const float* n_dev, float* loss_rows, float* loss_out, void* stream) {
    using namespace icz;
    const char* who = "icz_test_xe_loss";
    ICZ_REQUIRE(logits && captions && rows_t && loss_rows, "%s: null argument", who);
    ICZ_REQUIRE(V >= 2 && ldl >= V, "%s: V=%d (at least 2: the smoothing mass is spread over V - 1 tokens), ldl=%d", who, V, ldl);
    ICZ_REQUIRE(T >= 1 && T <= XE_MAX_T && L > T, "%s: T=%d outside 1..%d or not below L=%d", who, T, XE_MAX_T, L);
    ICZ_REQUIRE(B >= 1 && (long)B * T <= (1 << 20), "%s: B=%d", who, B);
    for (int t = 0; t < T; ++t) ICZ_REQUIRE(rows_t[t] >= 0 && rows_t[t] <= B, "%s: rows_t[%d]=%d outside 0..B", who, t, rows_t[t]);
    ICZ_REQUIRE(smoothing >= 0.f && smoothing <= 1.f && n_tokens > 0.f, "%s: smoothing=%g outside [0, 1] or n_tokens=%g not positive", who,
                (double)smoothing, (double)n_tokens);
    return launch_xe_loss(logits, V, ldl, captions, L, B, T, rows_t, smoothing, n_tokens, n_dev, loss_rows, loss_out, (hipStream_t)stream);
}

int icz_test_xe_group_loss(float* logits, int32_t V, int32_t ldl, const int64_t* captions, int32_t L, int32_t rows, int32_t T, const int32_t* lengths,
                           float smoothing, float n_tokens, const float* n_dev, float* loss_rows, float* loss_out, void* stream) {
    using namespace icz;
    const char* who = "icz_test_xe_group_loss";
    ICZ_REQUIRE(logits && captions && lengths && loss_rows, "%s: null argument", who);
    ICZ_REQUIRE(V >= 2 && ldl >= V && ldl % 4 == 0 && tc_al16(logits), "%s: V=%d (at least 2), ldl=%d (at least V, a multiple of 4), logits 16-byte aligned",
                who, V, ldl);
    ICZ_REQUIRE(T >= 1 && T <= XE_MAX_T && L > T, "%s: T=%d outside 1..%d or not below L=%d", who, T, XE_MAX_T, L);
    ICZ_REQUIRE(rows >= 1 && (long)rows * T <= (1 << 20), "%s: rows=%d", who, rows);
    ICZ_REQUIRE(smoothing >= 0.f && smoothing <= 1.f && n_tokens >= 0.f, "%s: smoothing=%g outside [0, 1] or n_tokens=%g negative", who,
                (double)smoothing, (double)n_tokens);
    // the step counts are read back and checked; n_tokens == 0: N is their sum, as behind icz_butd_xe_forward_n
    std::vector<int32_t> len(rows);
    hipStream_t const st = (hipStream_t)stream;
    ICZ_CHECK_HIP(hipMemcpyAsync(len.data(), lengths, sizeof(int32_t) * rows, hipMemcpyDeviceToHost, st));
    ICZ_CHECK_HIP(hipStreamSynchronize(st));
    long sum = 0;
    for (int r = 0; r < rows; ++r) {
        ICZ_REQUIRE(len[r] >= 0 && len[r] <= T, "%s: lengths[%d]=%d outside 0..T", who, r, len[r]);
        sum += len[r];
    }
    ICZ_REQUIRE(n_tokens > 0.f || sum > 0, "%s: no active (row, t) and no n_tokens", who);
    return launch_xe_group_loss(logits, V, ldl, captions, L, rows, T, lengths, smoothing, n_tokens > 0.f ? n_tokens : (float)sum, n_dev, loss_rows,
                                loss_out, st);
}

int icz_test_reinforce(const float* logp, const int64_t* seq, const float* reward, int32_t B, int32_t T, const float* mask_sum_global, float* coef,
                       float* loss_out, float* mask_sum_out, float* logits, int32_t V, int32_t ldl, const int32_t* draw, const float* lse, int32_t Bs,
                       int32_t row0, void* stream) {
    using namespace icz;
    const char* who = "icz_test_reinforce";
    ICZ_REQUIRE(logp && seq && reward && coef && logits && draw && lse, "%s: null argument", who);
    ICZ_REQUIRE(V >= 1 && ldl >= V, "%s: V=%d, ldl=%d", who, V, ldl);
    ICZ_REQUIRE(B >= 1 && T >= 1 && (long)B * T <= (1 << 20), "%s: B=%d, T=%d", who, B, T);
    ICZ_REQUIRE((Bs == 0 && row0 == 0) || (row0 >= 0 && Bs == row0 + B), "%s: Bs=%d rows per step are not row0=%d + B=%d", who, Bs, row0, B);
    ICZ_REQUIRE((long)T * (Bs ? Bs : B) <= 65535, "%s: %ld logits rows exceed the grid", who, (long)T * (Bs ? Bs : B));
    return launch_reinforce(logp, seq, reward, B, T, mask_sum_global, coef, loss_out, mask_sum_out, logits, V, ldl, draw, lse, Bs, row0,
                            (hipStream_t)stream);
}
const char* icz_last_error(void) { return icz::g_err; }
const char* icz_version(void) { return "libicz 0.1 (gfx950)"; }
}
