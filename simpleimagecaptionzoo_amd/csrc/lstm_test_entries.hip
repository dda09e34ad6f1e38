// Test entries of the kernels in lstm_kernels.h, each on given operands (include/icz.h: icz_test_embed, icz_test_embed_steps,
// icz_test_lstm_point, icz_test_lstm_bwd_point; tests/test_gpu_lstm_kernels.py): the arguments are checked on the host, then the
// kernel is launched with the grid the decoders give it.
#include <vector>

#include "lstm_kernels.h"

namespace icz {

static inline bool lt_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr int LT_MAX_ROWS = 65535;        // grid.y
constexpr int LT_MAX_SLABS = 32;          // the cap of gemm_pick_split

// icz_test_drop -> DropCfg.  keep4: the kernel reads four keep flags with one 4-byte load (the embedding kernels).
static int lt_drop(const char* who, const icz_test_drop* t, bool keep4, DropCfg* out) {
    *out = DropCfg{0, nullptr, nullptr, 0, 0, 0};
    if (!t) return ICZ_OK;
    ICZ_REQUIRE(t->mode >= 0 && t->mode <= 2, "%s: dropout mode %d (0 off, 1 keep flags, 2 Philox)", who, t->mode);
    ICZ_REQUIRE(t->mode != 1 || t->mask, "%s: dropout mode 1 without keep flags", who);
    ICZ_REQUIRE(t->mode != 1 || !keep4 || ((uintptr_t)t->mask & 3) == 0, "%s: dropout keep flags must be 4-byte aligned (four are read at once)", who);
    ICZ_REQUIRE(t->mode != 2 || t->seed, "%s: dropout mode 2 without a device seed", who);
    ICZ_REQUIRE(t->row0 >= 0, "%s: dropout row0=%d is negative", who, t->row0);
    *out = DropCfg{t->mode, t->mask, t->seed, t->stream, t->step, t->row0};
    return ICZ_OK;
}
static int lt_embed_shape(const char* who, const float* table, const float* emb, int V, int E) {
    ICZ_REQUIRE(table && emb, "%s: null embedding table or output", who);
    ICZ_REQUIRE(V >= 1, "%s: V=%d", who, V);
    ICZ_REQUIRE(E >= 4 && E % 4 == 0, "%s: E=%d is not a positive multiple of 4", who, E);
    ICZ_REQUIRE(lt_al16(table) && lt_al16(emb), "%s: table and emb must be 16-byte aligned", who);
    return ICZ_OK;
}
// token ids are device data that index the table: read back and checked before the launch
static int lt_tokens(const char* who, const int64_t* dev, size_t n, int V, hipStream_t st) {
    std::vector<int64_t> host(n);
    ICZ_CHECK_HIP(hipStreamSynchronize(st));
    ICZ_CHECK_HIP(hipMemcpy(host.data(), dev, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) ICZ_REQUIRE(host[i] >= 0 && host[i] < V, "%s: token %lld at %zu outside 0..V-1 (V=%d)", who, (long long)host[i], i, V);
    return ICZ_OK;
}

}  // namespace icz

extern "C" {

int icz_test_embed(const float* table, int32_t V, int32_t E, const int64_t* it, int32_t rows, float* emb, int32_t relu, const icz_test_drop* drop,
                   const int32_t* live, void* stream) {
    using namespace icz;
    const char* who = "icz_test_embed";
    ICZ_TRY(lt_embed_shape(who, table, emb, V, E));
    ICZ_REQUIRE(it, "%s: null token ids", who);
    ICZ_REQUIRE(rows >= 1 && rows <= LT_MAX_ROWS, "%s: rows=%d outside 1..%d", who, rows, LT_MAX_ROWS);
    DropCfg dc;
    ICZ_TRY(lt_drop(who, drop, true, &dc));
    hipStream_t const st = (hipStream_t)stream;
    ICZ_TRY(lt_tokens(who, it, (size_t)rows, V, st));
    hipLaunchKernelGGL(embed_kernel, dim3(cdiv(E, 1024), rows), dim3(256), 0, st, table, it, emb, rows, E, dc, relu != 0 ? 1 : 0, live);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_embed_steps(const float* table, int32_t V, int32_t E, const int64_t* tok, int32_t T, int32_t B, const int32_t* rows_t, float* emb,
                         const icz_test_drop* drop, void* stream) {
    using namespace icz;
    const char* who = "icz_test_embed_steps";
    ICZ_TRY(lt_embed_shape(who, table, emb, V, E));
    ICZ_REQUIRE(tok && rows_t, "%s: null tokens or rows_t", who);
    ICZ_REQUIRE(T >= 1 && T <= EMB_MAX_T, "%s: T=%d outside 1..%d", who, T, EMB_MAX_T);
    ICZ_REQUIRE(B >= 1 && (long)T * B <= LT_MAX_ROWS, "%s: B=%d (T B at most %d)", who, B, LT_MAX_ROWS);
    EmbRows er = {};
    for (int t = 0; t < T; ++t) {
        ICZ_REQUIRE(rows_t[t] >= 0 && rows_t[t] <= B, "%s: rows_t[%d]=%d outside 0..B (B=%d)", who, t, rows_t[t], B);
        ICZ_REQUIRE(t == 0 || rows_t[t] <= rows_t[t - 1], "%s: rows_t[%d]=%d above rows_t[%d]=%d (the batch only shrinks with t)", who, t, rows_t[t], t - 1,
                    rows_t[t - 1]);
        er.n[t] = rows_t[t];
    }
    DropCfg dc;
    ICZ_TRY(lt_drop(who, drop, true, &dc));
    ICZ_REQUIRE(dc.row0 == 0, "%s: dropout row0=%d (a teacher-forced pass has no evaluation-mode rows)", who, dc.row0);
    hipStream_t const st = (hipStream_t)stream;
    ICZ_TRY(lt_tokens(who, tok, (size_t)T * B, V, st));
    hipLaunchKernelGGL(embed_steps_kernel, dim3(cdiv(E, 1024), T * B), dim3(256), 0, st, table, tok, emb, B, E, er, dc);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_lstm_point(int32_t route, const icz_test_lstm_point_args* s, const icz_test_drop* drop, int32_t* route_out, void* stream) {
    using namespace icz;
    const char* who = "icz_test_lstm_point";
    ICZ_REQUIRE(s, "%s: null arguments", who);
    ICZ_REQUIRE(route >= 0 && route <= 2, "%s: route=%d (0 as the decoders, 1 one unit per thread, 2 gate per wave)", who, route);
    ICZ_REQUIRE(s->rows >= 1 && s->rows <= LT_MAX_ROWS && s->H >= 1, "%s: rows=%d (1..%d), H=%d", who, s->rows, LT_MAX_ROWS, s->H);
    ICZ_REQUIRE(s->ns >= 1 && s->ns <= LT_MAX_SLABS, "%s: ns=%d outside 1..%d", who, s->ns, LT_MAX_SLABS);
    ICZ_REQUIRE(s->slab && s->b_ih && s->b_hh && s->c_prev && s->h_out && s->c_out, "%s: null argument", who);
    ICZ_REQUIRE(s->pre || !s->pre_row, "%s: pre_row without pre", who);
    ICZ_REQUIRE(!s->pre || s->n_pre >= 1, "%s: pre with n_pre=%d rows", who, s->n_pre);
    ICZ_REQUIRE(!s->pre || s->pre_row || s->n_pre >= s->rows, "%s: pre of %d rows read by %d rows without pre_row", who, s->n_pre, s->rows);
    const int taken = route != 0 ? route : (s->H % 4 != 0 ? 1 : 2);
    if (taken == 2) {
        ICZ_REQUIRE(s->H % 4 == 0, "%s: the gate-per-wave kernel does not take H=%d (whole groups of 4)", who, s->H);
        ICZ_REQUIRE(lt_al16(s->slab) && lt_al16(s->pre) && lt_al16(s->b_ih) && lt_al16(s->b_hh),
                    "%s: the gate-per-wave kernel needs 16-byte aligned slab, pre and biases", who);
    }
    DropCfg dc;
    ICZ_TRY(lt_drop(who, drop, false, &dc));
    hipStream_t const st = (hipStream_t)stream;
    if (s->pre_row) {
        std::vector<int32_t> host(s->rows);
        ICZ_CHECK_HIP(hipStreamSynchronize(st));
        ICZ_CHECK_HIP(hipMemcpy(host.data(), s->pre_row, sizeof(int32_t) * s->rows, hipMemcpyDeviceToHost));
        for (int r = 0; r < s->rows; ++r) ICZ_REQUIRE(host[r] >= 0 && host[r] < s->n_pre, "%s: pre_row[%d]=%d outside 0..n_pre-1 (n_pre=%d)", who, r, host[r], s->n_pre);
    }
    if (route_out) *route_out = taken;
    const LstmPointArgs a = {s->slab, s->ns, s->pre, s->pre_row, s->b_ih, s->b_hh, s->c_prev, s->h_out, s->c_out, s->gates_out, s->hdrop_out,
                             s->rows, s->H, s->live};
    const dim3 grid(cdiv(a.H, 256), a.rows);
    if (route == 0) launch_lstm_point(a, dc, st);
    else if (route == 1) hipLaunchKernelGGL(lstm_point_kernel, grid, dim3(256), 0, st, a, dc);
    else hipLaunchKernelGGL(lstm_point_gw_kernel, grid, dim3(256), 0, st, a, dc);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

int icz_test_lstm_bwd_point(const icz_test_lstm_bwd_args* s, const icz_test_drop* drop, void* stream) {
    using namespace icz;
    const char* who = "icz_test_lstm_bwd_point";
    ICZ_REQUIRE(s, "%s: null arguments", who);
    ICZ_REQUIRE(s->rows >= 1 && s->rows <= LT_MAX_ROWS && s->H >= 1, "%s: rows=%d (1..%d), H=%d", who, s->rows, LT_MAX_ROWS, s->H);
    ICZ_REQUIRE(s->gates && s->c_cur && s->dgates && s->dc_prev, "%s: null argument (gates, c_cur, dgates, dc_prev)", who);
    const struct { const char* name; const float* p; int ns, lda, rows; } sets[3] = {
        {"a", s->dh_a, s->ns_a, s->lda_a, s->rows_a}, {"b", s->dh_b, s->ns_b, s->lda_b, s->rows_b}, {"c", s->dh_c, s->ns_c, s->lda_c, s->rows_c}};
    for (const auto& x : sets) {
        if (!x.p) continue;
        ICZ_REQUIRE(x.ns >= 1 && x.ns <= LT_MAX_SLABS, "%s: slab set %s with ns=%d outside 1..%d", who, x.name, x.ns, LT_MAX_SLABS);
        ICZ_REQUIRE(x.lda >= s->H, "%s: slab set %s with lda=%d below H=%d", who, x.name, x.lda, s->H);
        ICZ_REQUIRE(x.rows >= 1 && x.rows <= s->rows, "%s: slab set %s with %d rows outside 1..rows (rows=%d)", who, x.name, x.rows, s->rows);
    }
    ICZ_REQUIRE(!s->dc_in || (s->dc_in_rows >= 1 && s->dc_in_rows <= s->rows), "%s: dc_in with dc_in_rows=%d outside 1..rows (rows=%d)", who, s->dc_in_rows,
                s->rows);
    DropCfg dc;
    ICZ_TRY(lt_drop(who, drop, false, &dc));
    ICZ_REQUIRE(dc.row0 == 0, "%s: dropout row0=%d (the backward runs over the sampled rows alone)", who, dc.row0);
    LstmBwdArgs a = {};
    a.dh_a = s->dh_a; a.ns_a = s->ns_a; a.lda_a = s->lda_a; a.rows_a = s->rows_a;
    a.dh_b = s->dh_b; a.ns_b = s->ns_b; a.lda_b = s->lda_b; a.rows_b = s->rows_b;
    a.dh_c = s->dh_c; a.ns_c = s->ns_c; a.lda_c = s->lda_c; a.rows_c = s->rows_c;
    a.dhdrop = s->dhdrop; a.dc_in = s->dc_in; a.dc_in_rows = s->dc_in_rows;
    a.gates = s->gates; a.c_prev = s->c_prev; a.c_cur = s->c_cur; a.dgates = s->dgates; a.dc_prev = s->dc_prev;
    a.rows = s->rows; a.H = s->H; a.live = s->live; a.carry_live = s->carry_live;
    hipLaunchKernelGGL(lstm_bwd_point_kernel, dim3(cdiv(a.H, 256), a.rows), dim3(256), 0, (hipStream_t)stream, a, dc);
    ICZ_CHECK_HIP(hipGetLastError());
    return ICZ_OK;
}

}  // extern "C"
