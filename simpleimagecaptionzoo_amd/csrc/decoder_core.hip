// The out-of-line half of decoder_core.h (caption loss head, greedy select tail, C ABI helpers) and the library's error slot.
#include <stdarg.h>

#include "decoder_core.h"

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
    return ICZ_OK;
}

void CaptionHead::drop_loss_buffers() {
    coef = lse = loss_rows = kd_rows = nullptr; draw = nullptr; unf = gunf = nullptr; nunf = gnunf = live_rows = pack_idx = nullptr;
    pack_cap = 0;
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

int CaptionHead::xe_loss(float smoothing, float n_tokens_global, float* logits, int V, int ldl, float* loss_out, hipStream_t st) {
    const int B = cur_B, T = cur_T;
    const float n = n_tokens_global > 0.f ? n_tokens_global : (float)n_tokens;
    const float* n_dev = n_tokens_global < 0.f ? d_msum : nullptr;      // < 0: the device scalar handed over by *_set_*_global
    ICZ_CHECK_HIP(hipMemsetAsync(loss_rows, 0, sizeof(float) * T * B, st));
    ICZ_REQUIRE(T <= XE_MAX_T, "xe_backward: %d steps exceed %d", T, XE_MAX_T);
    XeRows xr = {};
    for (int t = 0; t < T; ++t) xr.n[t] = rows_t[t];
    hipLaunchKernelGGL(xe_loss_dlogits_kernel, dim3(B, T), dim3(256), 0, st, logits, V, ldl, cur_captions, cur_L, B, xr, smoothing, 1.0f / n, n_dev,
                       loss_rows);
    if (loss_out) hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, st, loss_rows, T * B, 1.0f / n, n_dev, loss_out);
    ICZ_CHECK_HIP(hipGetLastError());
    mode = 0;
    return ICZ_OK;
}

void CaptionHead::set_msum_global(float msum_global, hipStream_t st) const {
    if (msum_global >= 0.f)
        hipLaunchKernelGGL(set_scalars_kernel, dim3(1), dim3(1), 0, st, (uint64_t*)nullptr, (uint64_t)0, d_msum, msum_global);
}

int CaptionHead::reinforce(const float* reward, float* logits, int V, int ldl, float* loss_out, float* msum_out, hipStream_t st, int rows, int row0) {
    const int B = cur_B, T = cur_T;
    hipLaunchKernelGGL(reinforce_loss_kernel, dim3(1), dim3(256), 0, st, cur_logp, cur_seq, reward, B, T, (const float*)d_msum, coef, loss_out, msum_out);
    hipLaunchKernelGGL(reinforce_dlogits_kernel, dim3(cdiv(ldl, 256), T * (rows ? rows : B)), dim3(256), 0, st, logits, V, ldl, draw, lse, coef, B, T,
                       rows, row0);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

// ------------------------------------------------------------------------------------------------
void launch_greedy_select(const LogitsView& lv, const DecodeMember::EmbSlot& e, int rows, int V, float* amax_val, int* amax_idx, int64_t* it,
                          int64_t* ids_out, int T, int t, uint8_t* gunf, int* gn, hipStream_t st) {
    if (lv.ns > 1)         // 33 - 64 rows: the slabs of the vocabulary projection -> token + next embedding in one launch
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
const char* icz_last_error(void) { return icz::g_err; }
const char* icz_version(void) { return "libicz 0.1 (gfx950)"; }
}
