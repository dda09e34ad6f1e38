// Device kernels of an LSTM decoder step shared by the BUTD, AoA and NIC decoders: the input embedding (Embedding -> ReLU -> Dropout),
// the LSTMCell pointwise part behind the gate GEMMs and its backward, the fused d dec step of BPTT included.
// Reference line numbers: Models/BUTD_Model.py.
#pragma once
#include "icz_common.h"
#include "rng.h"

namespace icz {
namespace {   // internal linkage: this header is included by several translation units

// ---------------------------------------------------------------------------------------------------------
// Embedding -> ReLU -> Dropout (:77-81):  emb[row,:] = relu(E[it[row],:]) * keep * 2
__global__ __launch_bounds__(256) void embed_kernel(const float* __restrict__ table, const int64_t* __restrict__ it,
                                                    float* __restrict__ emb, int rows, int E, DropCfg dc, int relu = 1,
                                                    const int* __restrict__ live = nullptr) {
    if (step_dead(live)) return;               // a rollout step behind the reference's break (icz_common.h)
    const int row = blockIdx.y;
    const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= E) return;
    f32x4 x = *reinterpret_cast<const f32x4*>(table + (size_t)it[row] * E + e);
    const int drow = row - dc.row0;                    // (DropCfg::row0: evaluation-mode rows of a merged chain in front)
    if (drow < 0) dc.mode = 0;
    uint32_t k = dc.mode ? dc.keep4((uint64_t)drow * E + e) : 0xFu;
    const float sc = dc.mode ? 2.0f : 1.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = ((k >> j) & 1u) ? (relu ? fmaxf(x[j], 0.f) : x[j]) * sc : 0.f;
    *reinterpret_cast<f32x4*>(emb + (size_t)row * E + e) = x;
}

// The same for every time step of a teacher-forced forward pass at once (the tokens are all known up front): block (x, t B + b),
// active while b < rows_t[t]; dropout of step t = the per-step configuration (Philox step t / mask slice t of [T][B][E]).
constexpr int EMB_MAX_T = 128;
struct EmbRows { int n[EMB_MAX_T]; };
__global__ __launch_bounds__(256) void embed_steps_kernel(const float* __restrict__ table, const int64_t* __restrict__ tok,
                                                          float* __restrict__ emb, int B, int E, EmbRows rows, DropCfg dc) {
    const int t = blockIdx.y / B, b = blockIdx.y % B;
    if (b >= rows.n[t]) return;
    const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= E) return;
    dc.step = (uint32_t)t;
    if (dc.mode == 1) dc.mask += (size_t)t * B * E;
    f32x4 x = *reinterpret_cast<const f32x4*>(table + (size_t)tok[blockIdx.y] * E + e);
    uint32_t k = dc.mode ? dc.keep4((uint64_t)b * E + e) : 0xFu;
    const float sc = dc.mode ? 2.0f : 1.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = ((k >> j) & 1u) ? fmaxf(x[j], 0.f) * sc : 0.f;
    *reinterpret_cast<f32x4*>(emb + (size_t)blockIdx.y * E + e) = x;
}

// ---------------------------------------------------------------------------------------------------------
// LSTMCell pointwise part (:82-83; gate order i,f,g,o):
//   gates[row, :] = sum_z slab[z,row,:] + pre[pre_row,:] (optional) + b_ih + b_hh
//   c' = sig(f) c + sig(i) tanh(g);  h' = sig(o) tanh(c')
// Optionally stores the activated gates (for backward) and a dropped copy of h' (input of `predict`, :146).
struct LstmPointArgs {
    const float* slab; int nsplit;
    const float* pre; const int32_t* pre_row;     // pre may be null; pre_row null = identity
    const float* b_ih; const float* b_hh;
    const float* c_prev; float* h_out; float* c_out;
    float* gates_out;                              // [rows,4H] activated i,f,g,o or null
    float* hdrop_out;                              // [rows,H] or null
    int rows, H;
    const int* live;                               // step_dead(live): return at entry (icz_common.h)
};

// The cell of (row, hidden unit j) from its four finished pre-activation gates, the tail of both kernels below: activations, c', h',
// the optional gate store and the dropped copy of h'.
__device__ __forceinline__ void lstm_cell_tail(const LstmPointArgs& a, const DropCfg& dc, int row, int j, float pi, float pf, float pg, float po) {
    const int H = a.H, G = 4 * H;
    const float cp = a.c_prev[(size_t)row * H + j];
    const float gi = sigmoidf_(pi), gf = sigmoidf_(pf), gg = tanhf(pg), go = sigmoidf_(po);
    const float cn = gf * cp + gi * gg;
    const float hn = go * tanhf(cn);
    a.h_out[(size_t)row * H + j] = hn;
    a.c_out[(size_t)row * H + j] = cn;
    if (a.gates_out) {
        float* go_ = a.gates_out + (size_t)row * G + j;
        go_[0] = gi; go_[H] = gf; go_[2 * H] = gg; go_[3 * H] = go;
    }
    if (a.hdrop_out) {
        float hd = hn;
        const int drow = row - dc.row0;                // (DropCfg::row0)
        if (dc.mode && drow >= 0) hd = dc.keep((uint64_t)drow * H + j) ? hn * 2.0f : 0.f;
        a.hdrop_out[(size_t)row * H + j] = hd;
    }
}

// grid (H/256, rows): one hidden unit per thread (4-byte accesses, 256 B per wave instruction, 4x the workgroups of
// a float4 layout -- at 64 rows the kernel is latency-bound, not bandwidth-bound)
__global__ __launch_bounds__(256) void lstm_point_kernel(LstmPointArgs a, DropCfg dc) {
    if (step_dead(a.live)) return;
    const int row = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.H) return;
    const int H = a.H, G = 4 * H;
    const size_t MN = (size_t)a.rows * G;
    float gt[4];
    const int pr = (a.pre && a.pre_row) ? a.pre_row[row] : row;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const size_t off = (size_t)row * G + q * H + j;
        float s = sum_slabs1(a.slab, a.nsplit, MN, off);
        if (a.pre) s += a.pre[(size_t)pr * G + q * H + j];
        s += a.b_ih[q * H + j];
        s += a.b_hh[q * H + j];
        gt[q] = s;
    }
    lstm_cell_tail(a, dc, row, j, gt[0], gt[1], gt[2], gt[3]);
}

// Gate-per-wave form, grid (H / 256, rows), 256 threads: wave q sums gate q of the workgroup's 256 hidden units (16 bytes per
// lane and slab, the loads of up to eight slabs independent), the four gates meet in LDS and thread j finishes unit j.  The
// resident-activation gate GEMM (gemm_resident_x3.hip) leaves 12 - 16 split-K slabs (16.8 MB at 64 rows): the one-unit kernel
// above then issues 64 four-byte wave loads per thread (8.3 us), a four-units-per-thread form with one wave per workgroup
// has ONE wave per compute unit waiting on 64 KB (9.5 us in the SCST trace); here four waves per compute unit wait on 16 KB
// each (5.1 us).  Same summation order per element (slabs ascending, pre, b_ih, b_hh): bit-identical to the kernel above, which
// tests/test_gpu_lstm_kernels.py::test_lstm_point_kernels_agree_bit_for_bit_and_are_near_float64 asserts in every output, for every
// combination of the three slab loops below (through icz_test_lstm_point, routes 1 and 2).
__global__ __launch_bounds__(256) void lstm_point_gw_kernel(LstmPointArgs a, DropCfg dc) {
    __shared__ __attribute__((aligned(16))) float sg[4][256];
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int H = a.H, G = 4 * H;
    const int j0 = blockIdx.x * 256, j4 = j0 + lane * 4;
    const size_t MN = (size_t)a.rows * G;
    // early-out of a dead rollout step (live_flag / flag_dead, icz_common.h): tested once, behind the first batch of slab loads
    const int lflag = live_flag(a.live);
    bool tested = false;
#define ICZ_LIVE_TEST() do { if (!tested) { if (flag_dead(lflag)) return; tested = true; } } while (0)
    if (j4 < H) {
        const size_t off = (size_t)row * G + (size_t)q * H + j4;
        const float* p = a.slab + off;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        int z = 0;
        for (; z + 8 <= a.nsplit; z += 8) {
            f32x4 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x4*>(p + (size_t)(z + i) * MN);
            ICZ_LIVE_TEST();
#pragma unroll
            for (int i = 0; i < 8; ++i) s += v[i];
        }
        for (; z + 4 <= a.nsplit; z += 4) {
            f32x4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const f32x4*>(p + (size_t)(z + i) * MN);
            ICZ_LIVE_TEST();
#pragma unroll
            for (int i = 0; i < 4; ++i) s += v[i];
        }
        for (; z < a.nsplit; ++z) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + (size_t)z * MN);
            ICZ_LIVE_TEST();
            s += v;
        }
        if (a.pre) {
            const int pr = a.pre_row ? a.pre_row[row] : row;
            s += *reinterpret_cast<const f32x4*>(a.pre + (size_t)pr * G + (size_t)q * H + j4);
        }
        s += *reinterpret_cast<const f32x4*>(a.b_ih + (size_t)q * H + j4);
        s += *reinterpret_cast<const f32x4*>(a.b_hh + (size_t)q * H + j4);
        *reinterpret_cast<f32x4*>(&sg[q][lane * 4]) = s;
    }
    ICZ_LIVE_TEST();          // (lanes past H, no slabs)
#undef ICZ_LIVE_TEST
    __syncthreads();
    const int j = j0 + tid;
    if (j >= H) return;
    lstm_cell_tail(a, dc, row, j, sg[0][tid], sg[1][tid], sg[2][tid], sg[3][tid]);
}

// the gate-per-wave kernel wherever the hidden size allows 16-byte accesses
inline void launch_lstm_point(const LstmPointArgs& a, const DropCfg& dc, hipStream_t st) {
    const dim3 grid(cdiv(a.H, 256), a.rows);
    if (a.H % 4 != 0) hipLaunchKernelGGL(lstm_point_kernel, grid, dim3(256), 0, st, a, dc);
    else hipLaunchKernelGGL(lstm_point_gw_kernel, grid, dim3(256), 0, st, a, dc);
}

// ---------------------------------------------------------------------------------------------------------
// LSTMCell backward, pointwise part.  dh = sum of up to three slab sets (+ optional dropped-output term),
// dc = dc_in (optional).  Emits d(pre-activation gates) [rows,4H] and dc_prev.
struct LstmBwdArgs {
    const float* dh_a; int ns_a;      // slabs [ns][rows][lda_a] read at column offset 0..H
    int lda_a;
    const float* dh_b; int ns_b; int lda_b;
    const float* dh_c; int ns_c; int lda_c;
    const float* dhdrop;              // [rows,H] gradient w.r.t. the dropped copy of h (predict input) or null
    const float* dc_in;               // [rows,H] or null
    const float* gates;               // [rows,4H] activated i,f,g,o
    const float* c_prev;              // [rows,H] or null (= zeros)
    const float* c_cur;               // [rows,H]
    float* dgates;                    // [rows,4H]
    float* dc_prev;                   // [rows,H]
    int rows, H;
    int rows_a, rows_b, rows_c;       // row counts of the slab sets (slab stride = rows_x * lda_x)
    int dc_in_rows;                   // valid rows of dc_in
    const int* live;                  // step_dead(live): this step never ran -> its dgates rows are ZERO (the weight-gradient GEMMs read
                                      // every (t, b) row) and nothing else is touched
    const int* carry_live;            // step_dead(carry_live): the step behind this one (t + 1) never ran -> no dh_a, no dc_in
};
// The arithmetic of one (row, hidden unit) has ONE owner, in three parts that both kernels below call in this order:
//   lstm_bwd_load    the loads that do not depend on the step's liveness (issued in front of the flag test, icz_common.h)
//   lstm_bwd_dh_ab   dh = 0 + slab set a (the carry, if live) + slab set b, each set summed in slab order first
//   lstm_bwd_finish  + the dropped-output term, then gates, dc, d gates and dc_prev
// with the third dh term (slab set c, or the fused kernel's own product) added between the last two; lstm_bwd_dead is the dead step.
struct LstmBwdIn { float gi, gf, gg, go, cc, cp, dhd; };
__device__ __forceinline__ LstmBwdIn lstm_bwd_load(const LstmBwdArgs& a, int row, int j) {
    const int H = a.H, G = 4 * H;
    const float* g = a.gates + (size_t)row * G + j;
    LstmBwdIn in;
    in.gi = g[0]; in.gf = g[H]; in.gg = g[2 * H]; in.go = g[3 * H];
    in.cc = a.c_cur[(size_t)row * H + j];
    in.cp = a.c_prev ? a.c_prev[(size_t)row * H + j] : 0.f;
    in.dhd = 0.f;
    if (a.dhdrop) in.dhd = a.dhdrop[(size_t)row * H + j];
    return in;
}
__device__ __forceinline__ void lstm_bwd_dead(const LstmBwdArgs& a, int row, int j) {
    const int H = a.H;
    float* o = a.dgates + (size_t)row * 4 * H + j;
    o[0] = 0.f; o[H] = 0.f; o[2 * H] = 0.f; o[3 * H] = 0.f;
}
// a slab set only holds rows_x rows (XE: the batch shrinks with t); rows beyond contribute zero
__device__ __forceinline__ float lstm_bwd_dh_ab(const LstmBwdArgs& a, int row, int j, bool carry) {
    float dh = 0.f;
    if (a.dh_a && carry && row < a.rows_a) dh += sum_slabs1(a.dh_a, a.ns_a, (size_t)a.rows_a * a.lda_a, (size_t)row * a.lda_a + j);
    if (a.dh_b && row < a.rows_b) dh += sum_slabs1(a.dh_b, a.ns_b, (size_t)a.rows_b * a.lda_b, (size_t)row * a.lda_b + j);
    return dh;
}
__device__ __forceinline__ void lstm_bwd_finish(const LstmBwdArgs& a, const DropCfg& dc, int row, int j, const LstmBwdIn& in, float dh, bool carry) {
    const int H = a.H, G = 4 * H;
    const float gi = in.gi, gf = in.gf, gg = in.gg, go = in.go, cc = in.cc, cp = in.cp;
    if (a.dhdrop) {
        float d = in.dhd;
        if (dc.mode) d = dc.keep((uint64_t)row * H + j) ? d * 2.0f : 0.f;
        dh += d;
    }
    const float dcin = (a.dc_in && carry && row < a.dc_in_rows) ? a.dc_in[(size_t)row * H + j] : 0.f;
    const float tc = tanhf(cc);
    const float dcv = dcin + dh * go * (1.f - tc * tc);
    float* o = a.dgates + (size_t)row * G + j;
    o[0] = dcv * gg * gi * (1.f - gi);
    o[H] = dcv * cp * gf * (1.f - gf);
    o[2 * H] = dcv * gi * (1.f - gg * gg);
    o[3 * H] = dh * tc * go * (1.f - go);
    a.dc_prev[(size_t)row * H + j] = dcv * gf;
}
// grid (H/256, rows): one hidden unit per thread (see lstm_point_kernel)
__global__ __launch_bounds__(256) void lstm_bwd_point_kernel(LstmBwdArgs a, DropCfg dc) {
    const int row = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.H) return;
    // loads that do not depend on the step's liveness first: the two flags are tested behind them (live_flag / flag_dead, icz_common.h)
    const int lflag = live_flag(a.live), cflag = live_flag(a.carry_live);
    const LstmBwdIn in = lstm_bwd_load(a, row, j);
    if (flag_dead(lflag)) {
        lstm_bwd_dead(a, row, j);
        return;
    }
    const bool carry = cflag != 0;
    float dh = lstm_bwd_dh_ab(a, row, j, carry);
    if (a.dh_c && row < a.rows_c) dh += sum_slabs1(a.dh_c, a.ns_c, (size_t)a.rows_c * a.lda_c, (size_t)row * a.lda_c + j);
    lstm_bwd_finish(a, dc, row, j, in, dh, carry);
}

// ---------------------------------------------------------------------------------------------------------
// The TD-LSTM backward of a BPTT step with its third dh term computed in place: dh1 = carry + X1[:, D:] + d dec . w_dec, where the
// two-launch route writes X2 = d dec . w_dec [rows, H] as split-K slabs (gemm_nn_kernel) and lstm_bwd_point_kernel reads them back
// at the very (row, hidden unit) positions a GEMM output tile holds -- no reduction over rows or columns lies between the two, so the
// pointwise part is the product's epilogue and no workgroup waits for another.
//
// Grid (H / 16, ceil(rows / 16)), 256 threads: a workgroup owns 16 rows x 16 hidden units and the whole K = A (at H = 1024 and 64 rows:
// 256 workgroups that pull 64 KB of d dec and 64 KB of w_dec each -- sized by bytes per compute unit, not by tile count).
//
// Bitwise the two-launch route.  That route cuts K into `ns` ranges of `cps` stages (gemm_pick_split; a stage is BKC = 128 deep, 64 if
// A is no multiple of 128), accumulates every range with k ascending through v_mfma_f32_16x16x4_f32 -- MFMA number m of a stage takes
// the four k = 16 (m / 4) + (m % 4) + 4 q, q = 0..3 -- into an accumulator of its own, and sum_slabs1 adds the ranges in slab order
// into one number that is then added behind the carry and X1 terms.  Here wave w takes the ranges w, w + 4, ... with the same
// instruction over the same k groups in the same order, one accumulator per range; the ranges meet in LDS and every thread adds
// those of its element in slab order.
struct Dh1FusedArgs {
    LstmBwdArgs p;                    // dh_c is not read: the product below takes its place
    const float* ddec;                // [rows, A] dense (16-byte aligned)
    const float* w_dec;               // [A, H] dense
    int A;
    int ns, cps;                      // K ranges and stages per range of the two-launch route (every range non-empty, ns <= DH1_MAX_SPLIT)
};
constexpr int DH1_TILE = 16, DH1_MAX_SPLIT = 32;      // 32: the cap of gemm_pick_split
// what the kernel needs of a step (the route, the test entry and the tests ask here): at most 64 rows -- above, the two-launch route
// picks its split by another rule --, hidden units in whole tiles, K in whole 64-deep stages (no zero-filled tail stage)
inline bool lstm_bwd_dh1_fused_takes(int rows, int H, int A) {
    return rows >= 1 && rows <= 64 && H >= DH1_TILE && H % DH1_TILE == 0 && A >= 64 && A % 64 == 0;
}
inline int lstm_bwd_dh1_stage_k(int A) { return A % 128 == 0 ? 128 : 64; }      // the stage depth gemm_f32 takes for the NN product over K = A

template <int BKC>
__global__ __launch_bounds__(256) void lstm_bwd_dh1_fused_kernel(Dh1FusedArgs f) {
    constexpr int NS = BKC / 16;                  // k-groups of 16 per stage
    __shared__ float part[DH1_MAX_SPLIT][DH1_TILE * DH1_TILE];
    const LstmBwdArgs& a = f.p;
    const int lflag = live_flag(a.live), cflag = live_flag(a.carry_live);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int n0 = blockIdx.x * DH1_TILE, m0 = blockIdx.y * DH1_TILE;
    // the element this thread finishes: tile position tid = 16 (row in tile) + (column in tile)
    const int row = m0 + (tid >> 4), j = n0 + (tid & 15);
    const bool valid = row < a.rows;
    LstmBwdIn in = {};
    if (valid) in = lstm_bwd_load(a, row, j);

    // MFMA operands of lane (i, q): A[i][k] = d dec[m0 + i][k], B[k][i] = w_dec[k][n0 + i] at k = k0 + 16 s + e + 4 q for MFMA 4 s + e.
    // Rows beyond the batch are read from a clamped (valid) row: they feed accumulator rows that are never stored.
    const int mrow = m0 + li;
    const float* const arow = f.ddec + (size_t)(mrow < a.rows ? mrow : a.rows - 1) * f.A + 4 * lq;
    const float* const bcol = f.w_dec + (size_t)(4 * lq) * a.H + n0 + li;
    const int tot = f.A / BKC;
    f32x4 av[NS], an[NS];
    float bv[4 * NS], bn[4 * NS];
    auto load_stage = [&](int c, f32x4 (&x)[NS], float (&w)[4 * NS]) {
        const int k0 = c * BKC;
#pragma unroll
        for (int s = 0; s < NS; ++s) x[s] = *reinterpret_cast<const f32x4*>(arow + k0 + 16 * s);
#pragma unroll
        for (int m = 0; m < 4 * NS; ++m) w[m] = bcol[(size_t)(k0 + 16 * (m >> 2) + (m & 3)) * a.H];
    };
    int z = wave, c = z * f.cps, c_end = c + f.cps < tot ? c + f.cps : tot;
    bool have = z < f.ns;
    if (have) load_stage(c, av, bv);
    if (flag_dead(lflag)) {                       // behind the first loads, in front of the first write
        if (valid) lstm_bwd_dead(a, row, j);
        return;
    }
    const bool carry = cflag != 0;
    float dh = 0.f;
    if (valid) dh = lstm_bwd_dh_ab(a, row, j, carry);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    while (have) {
        // the next stage of this wave: the same range, or the first of the range four further on
        int z2 = z, c2 = c + 1, c_end2 = c_end;
        if (c2 >= c_end) { z2 = z + 4; c2 = z2 * f.cps; c_end2 = c2 + f.cps < tot ? c2 + f.cps : tot; }
        const bool more = z2 < f.ns;
        if (more) load_stage(c2, an, bn);
        __builtin_amdgcn_sched_barrier(0);        // the next stage's loads stay in front of this stage's MFMAs
#pragma unroll
        for (int m = 0; m < 4 * NS; ++m) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m >> 2][m & 3], bv[m], acc, 0, 0, 0);
        if (c + 1 >= c_end) {                     // range z is complete: acc[r] <-> row 4 q + r, column i of the tile
#pragma unroll
            for (int r = 0; r < 4; ++r) part[z][(4 * lq + r) * DH1_TILE + li] = acc[r];
            acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) av[s] = an[s];
#pragma unroll
        for (int m = 0; m < 4 * NS; ++m) bv[m] = bn[m];
        z = z2; c = c2; c_end = c_end2; have = more;
    }
    __syncthreads();
    if (!valid) return;
    float x2 = 0.f;                               // as sum_slabs1 adds the slabs of X2
    for (int s = 0; s < f.ns; ++s) x2 += part[s][tid];
    dh += x2;
    const DropCfg off = {};                       // the TD-LSTM's output is not dropped: p.dhdrop is null
    lstm_bwd_finish(a, off, row, j, in, dh, carry);
}

}  // namespace
}  // namespace icz
