// Host-side machinery shared by the BUTD, AoA and NIC decoder handles: device allocations, the hipGraph cache, side
// streams, the caption loss head (the state of the stored forward pass, packed logits, the loss heads that start a backward pass: LossHead), the decoder seams (DecodeMember)
// with the drivers that run on them (beam search: beam.hip, sampling: sample_decode.hip, scoring given captions: score_captions.hip) and the greedy select tail.
// Each rule below ("free => clear graphs", "zero-fill then sync", "sync => destroy a graph") has this one owner.
// Destroying a captured graph: a replay of it may still be in flight on the caller's stream, so whoever destroys one synchronises the
// device first -- GraphCache::run before it evicts (rare: only a working set above the capacity evicts), and the callers of
// GraphCache::clear (DeviceBuffers::release_training, the rebind and option paths of the handles) before they clear; a handle's
// destruction (icz_*_destroy right behind a call) through ~GraphCache, which synchronises itself when it still holds a graph.
#pragma once
#include <functional>
#include <vector>
#include <stdint.h>

#include "gemm_ops.h"
#include "icz_common.h"

namespace icz {

void gemm_set_capturing(bool on);
bool gemm_prof_on();                  // gemm_f32.hip: event timing active (graphs captured now contain event nodes)

// hipGraph cache: a whole rollout / backward is ~300-700 launches of 2-30 us kernels; replaying a captured graph removes the
// per-launch host cost and shrinks the inter-kernel gaps.  Capture on first use of a key, replay afterwards.  The key holds every
// pointer / size / option baked into the captured kernel arguments, so it only pays when the caller reuses its buffers (the Engine does).
struct GraphCache {
    struct Entry { std::vector<uintptr_t> key; hipGraphExec_t exec; uint64_t last_use; };
    explicit GraphCache(size_t capacity) : capacity(capacity) {}
    GraphCache(const GraphCache&) = delete;
    GraphCache& operator=(const GraphCache&) = delete;
    ~GraphCache() {
        if (!graphs.empty()) (void)hipDeviceSynchronize();      // the handle is destroyed: a replay may still be in flight
        clear();
        if (cap_st) (void)hipStreamDestroy(cap_st);
    }
    void clear() {                    // captured kernel arguments hold parameter / buffer addresses: drop them when those change
                                      // (the caller has synchronised, ~GraphCache included: see the rule at the top of this file)
        for (auto& e : graphs) (void)hipGraphExecDestroy(e.exec);
        graphs.clear();
    }
    template <class F>
    int run(std::vector<uintptr_t> key, hipStream_t st, F&& fn) {
        ++tick;
        key.push_back((gemm_prof_on() ? 1 : 0) + 2 * (uintptr_t)(gemm_big_switch() + 2));      // the tile-configuration override changes the captured launches
        for (auto& e : graphs)
            if (e.key == key) {
                e.last_use = tick;
                ICZ_CHECK_HIP(hipGraphLaunch(e.exec, st));
                return ICZ_OK;
            }
        if (!cap_st) ICZ_CHECK_HIP(hipStreamCreateWithFlags(&cap_st, hipStreamNonBlocking));
        ICZ_CHECK_HIP(hipStreamBeginCapture(cap_st, hipStreamCaptureModeThreadLocal));
        gemm_set_capturing(true);
        const int status = fn(cap_st);
        gemm_set_capturing(false);
        hipGraph_t g = nullptr;
        hipError_t ce = hipStreamEndCapture(cap_st, &g);
        if (status != ICZ_OK) { if (g) (void)hipGraphDestroy(g); return status; }
        if (ce != hipSuccess || !g) { set_error("hipStreamEndCapture failed: %s", hipGetErrorString(ce)); return ICZ_ERR_HIP; }
        hipGraphExec_t exec = nullptr;
        hipError_t ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ie != hipSuccess) { set_error("hipGraphInstantiate failed: %s", hipGetErrorString(ie)); return ICZ_ERR_HIP; }
        if (graphs.size() >= capacity) {      // evict the least recently used entry, once no replay of it can still be in flight
            size_t lru = 0;
            for (size_t i = 1; i < graphs.size(); ++i) if (graphs[i].last_use < graphs[lru].last_use) lru = i;
            const hipError_t se = hipDeviceSynchronize();
            if (se != hipSuccess) {
                (void)hipGraphExecDestroy(exec);
                set_error("hipDeviceSynchronize failed before a graph eviction: %s", hipGetErrorString(se));
                return ICZ_ERR_HIP;
            }
            (void)hipGraphExecDestroy(graphs[lru].exec);
            graphs.erase(graphs.begin() + lru);
        }
        graphs.push_back({key, exec, tick});
        ICZ_CHECK_HIP(hipGraphLaunch(exec, st));
        return ICZ_OK;
    }
    std::vector<Entry> graphs;
    size_t capacity;
    hipStream_t cap_st = nullptr;
    uint64_t tick = 0;
};

// Owner of a handle's device allocations: a persistent list and a training list (grown on demand).  Every allocation is
// zero-filled on the NULL stream; callers enqueue on NON-BLOCKING streams (torch's), which are not ordered behind it, so each
// growth ends with synced(): without it a kernel of the first call after a (re)allocation could run BEFORE the zero-fill of its
// buffer and then be wiped by it (round 5: sample_init_kernel's unfinished flags, seen as an all-zero rollout in 1 of 3 five-rank runs).
struct DeviceBuffers {
    std::vector<void*> persistent, training;
    bool to_training = false;        // alloc() target while a TrainingScope is alive
    struct TrainingScope {
        DeviceBuffers& m;
        explicit TrainingScope(DeviceBuffers& x) : m(x) { m.to_training = true; }
        ~TrainingScope() { m.to_training = false; }
    };
    DeviceBuffers() = default;
    DeviceBuffers(const DeviceBuffers&) = delete;
    DeviceBuffers& operator=(const DeviceBuffers&) = delete;
    ~DeviceBuffers() {
        for (void* p : training) (void)hipFree(p);
        for (void* p : persistent) (void)hipFree(p);
    }
    int alloc(void** p, size_t bytes) {
        if (!bytes) bytes = 16;
        ICZ_CHECK_HIP(hipMalloc(p, bytes));
        ICZ_CHECK_HIP(hipMemset(*p, 0, bytes));
        (to_training ? training : persistent).push_back(*p);
        return ICZ_OK;
    }
    int synced() {
        ICZ_CHECK_HIP(hipDeviceSynchronize());
        return ICZ_OK;
    }
    // sync -> clear the graph cache -> free: the captured graphs carry the freed addresses in their kernel arguments
    int release_training(GraphCache* gc) {
        if (training.empty()) return ICZ_OK;
        ICZ_CHECK_HIP(hipDeviceSynchronize());
        if (gc) gc->clear();
        for (void* p : training) (void)hipFree(p);
        training.clear();
        return ICZ_OK;
    }
};

// A stream for work beside the caller's stream and its fork / join events (two pairs: the backward passes fork twice),
// created lazily -- outside any capture -- by ensure().
struct SideStream {
    hipStream_t st = nullptr;
    hipEvent_t fork[2] = {}, join[2] = {};
    SideStream() = default;
    SideStream(const SideStream&) = delete;
    SideStream& operator=(const SideStream&) = delete;
    ~SideStream() {
        if (st) (void)hipStreamDestroy(st);
        for (int i = 0; i < 2; ++i) {
            if (fork[i]) (void)hipEventDestroy(fork[i]);
            if (join[i]) (void)hipEventDestroy(join[i]);
        }
    }
    int ensure(bool lowest_priority = false) {
        if (st) return ICZ_OK;
        if (lowest_priority) {
            int lo = 0, hi = 0;
            ICZ_CHECK_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));      // lo = least urgent
            ICZ_CHECK_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, lo));
        } else {
            ICZ_CHECK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        }
        for (int i = 0; i < 2; ++i) {
            ICZ_CHECK_HIP(hipEventCreateWithFlags(&fork[i], hipEventDisableTiming));
            ICZ_CHECK_HIP(hipEventCreateWithFlags(&join[i], hipEventDisableTiming));
        }
        return ICZ_OK;
    }
    // One fork / join pair of a side stream for the life of one branch beside the caller's stream, and the owner of the rule
    // "a forked branch is joined on every way out": inside a capture an unjoined fork would hide the error that caused the early
    // return behind a capture failure, so the destructor closes whatever a started branch still has open (statuses dropped, the
    // error text of the first failure kept).  The four moments are apart because the call sites keep them apart: a branch is forked
    // at one point of the caller's stream and issued behind later work of it.
    // side null: the branch runs in line -- st() is the caller's stream and nothing is recorded or waited on.
    struct Branch {
        Branch(SideStream* side, int pair) : s(side), i(pair) {}
        Branch(const Branch&) = delete;
        Branch& operator=(const Branch&) = delete;
        ~Branch() {
            if (started && !finished) (void)hipEventRecord(s->join[i], s->st);
            if (started && !joined) (void)hipStreamWaitEvent(main, s->join[i], 0);
        }
        hipStream_t st() const { return s ? s->st : main; }      // where the branch's launches go (behind fork())
        int fork(hipStream_t caller) {      // the fork point on the caller's stream
            main = caller;
            if (s) ICZ_CHECK_HIP(hipEventRecord(s->fork[i], main));
            return ICZ_OK;
        }
        int start() {                       // the side stream waits for the fork point: the branch is issued behind this
            if (s) { ICZ_CHECK_HIP(hipStreamWaitEvent(s->st, s->fork[i], 0)); started = true; }
            return ICZ_OK;
        }
        int finish() {                      // behind the branch's last launch
            if (started && !finished) { finished = true; ICZ_CHECK_HIP(hipEventRecord(s->join[i], s->st)); }
            return ICZ_OK;
        }
        int join() {                        // the caller's stream waits for the branch (finished here if it is not yet); idempotent
            ICZ_TRY(finish());
            if (started && !joined) { joined = true; ICZ_CHECK_HIP(hipStreamWaitEvent(main, s->join[i], 0)); }
            return ICZ_OK;
        }
      private:
        SideStream* s; int i; hipStream_t main = nullptr;
        bool started = false, finished = false, joined = false;
    };
};

struct DistillArgs;                   // ens_sample.h: the teachers' packed logits and the options of a distillation step
// An SCST objective (scst_objective.hip; include/icz.h: icz_scst_objective, checked by scst_objective_args) as the loss head takes it;
// key(): what a captured backward pass bakes in of it -- kind, K, the bit patterns of the three reals, the reward / scores pointers.
struct ScstObjective {
    int kind, K; float risk_alpha, entropy_weight, n_img_global; const float* reward; const double* scores;
    void key(std::vector<uintptr_t>& k) const;
};
// scratch of the objective's kernels: per-row entropies [T rows], per-image risk and mask count [images], the local mask sum
struct ScstScratch { float* ent_rows; double* L_img; int* m_img; float* scal; };
// The loss head of a rollout's backward pass as a decoder calls it: obj null = RewardCriterion on `reward` (loss_out [1]), else the
// objective (loss_out [3] = {loss, obj, ent}, ent_out [rows, T] or null)
struct RolloutHead { const float* reward; const ScstObjective* obj; float* loss_out; float* ent_out; float* msum_out; };
// SCST on without-replacement samples (swor_objective.hip; include/icz.h: icz_swor_opts, checked by swor_args) as the loss head takes it
struct SworArgs { int n, estimator; float n_img_global; const float* phi; const double* G; const double* scores; const int32_t* perm; double* stats_out; };
// scratch of its kernels: coef [images n] (-c / N per slot), cs [images n] (coef logp per slot, float64)
struct SworScratch { float* coef; double* cs; };
// What starts a backward pass: the loss head that turns the stored logits into dlogits in place, as a kind with that kind's arguments.
// A C entry fills one in and hands it to its family's backward(); CaptionHead checks it against the stored pass (check_loss_head),
// queues it (launch_loss_head) and marks the pass consumed (begin_backward); the family runs its BPTT behind it.
struct LossHead {
    enum Kind { XE, XE_DISTILL, XE_SWOR, XE_DLOGITS, ROLLOUT, ROLLOUT_DLOGP };
    Kind kind;
    const char* fam;                  // "butd" / "aoa" / "nic" and ...
    const char* who;                  // ... the entry ("butd xe_backward_distill"), as the error texts name them
    float norm_global = 0.f;          // n_tokens_global (XE kinds) / mask_sum_global (ROLLOUT): > 0 the value, 0 the local one, < 0 the device
                                      // scalar handed over by icz_*_set_*_global
    float* loss_out = nullptr;        // XE [1], XE_DISTILL [3], XE_SWOR [1 + images]; ROLLOUT keeps its outputs in `rollout`
    float smoothing = 0.f;            // XE
    const DistillArgs* distill = nullptr;
    const SworArgs* swor = nullptr;   // XE_SWOR, with the caller's row count
    int swor_rows = 0;
    const float* upstream = nullptr;  // XE_DLOGITS: dpacked [n_tokens, V]; ROLLOUT_DLOGP: dlogp [rows, T]
    RolloutHead rollout = {};         // ROLLOUT
    const icz_scst_objective* objective = nullptr;      // ROLLOUT with an objective: the caller's struct, checked against the stored rollout
    const int32_t* group_len = nullptr;                 // XE behind a grouped forward (Butd::xe_forward_n): steps per row (device) -> xe_group_loss
    bool rollout_kind() const { return kind >= ROLLOUT; }      // the stored pass is a sampled rollout: the early-out of its backward pass applies
};
// The caption loss head: host-side state of a stored training-mode forward pass and the loss buffers of all three decoders.
struct CaptionHead {
    int mode = 0;                 // 0 none, 1 sample rollout stored, 2 XE forward stored
    int cur_B = 0, cur_T = 0, cur_L = 0, n_tokens = 0;
    // rows per image of the stored pass, row = img * K + k (sample_n, beyond the reference; Butd::xe_forward_n); 1 = every other entry
    // point.  Set by the family behind begin_rollout / begin_xe.
    int cur_K = 1;
    bool early_out = true;        // option "early_out": rollout / BPTT steps behind the reference's break return at entry (0: they run, A/B)
    bool cur_train = false;
    const int64_t* cur_seq = nullptr; const float* cur_logp = nullptr; const int64_t* cur_captions = nullptr;
    std::vector<int> rows_t;      // active rows per step of the XE batch (lengths sorted in decreasing order)
    float ss_prob = 0.f;          // scheduled sampling in xe_forward (icz_*_set_scheduled_sampling)
    float cur_ss_prob = 0.f;      // ss_prob of the stored XE forward pass
    const float* ss_gate = nullptr; const float* ss_draw = nullptr;      // explicit [T, B] uniforms (device) or Philox
    uint64_t* d_seed = nullptr;   // Philox seed of the current training-mode call (device resident)
    float* d_msum = nullptr;      // data-parallel loss normaliser (0 = use the local one)
    // training buffers (alloc_loss_buffers): TB = steps x rows
    float *coef = nullptr, *lse = nullptr, *loss_rows = nullptr, *kd_rows = nullptr;
    int32_t* draw = nullptr;
    uint8_t* unf = nullptr; int* nunf = nullptr;
    uint8_t* gunf = nullptr; int* gnunf = nullptr;     // the same for the greedy baseline of an SCST step
    int* live_rows = nullptr;     // (steps the sampled rollout ran) x B: row limit of the backward pass's batched GEMMs
    int* pack_idx = nullptr; int pack_cap = 0;         // packed-sequence index: row_off[T] | rows_t[T]
    double* obj_img = nullptr; int* obj_mimg = nullptr; float* obj_scal = nullptr;      // ScstScratch beside loss_rows (scst_objective)
    float* swor_coef = nullptr; double* swor_cs = nullptr;      // SworScratch [2 B]: n / (n - 1) <= 3 / 2 slots per stored row (swor_loss)

    int alloc_scalars(DeviceBuffers& m);
    int alloc_loss_buffers(DeviceBuffers& m, size_t TB, size_t B, size_t T);
    void drop_loss_buffers();     // the training list was released: forget its pointers
    int require_mode(int want, const char* who) const;
    // teacher-forced XE input: lengths checked (per-model prefix `who`), T = the longest
    static int xe_steps(const char* who, const int32_t* lengths, int B, int L, int* T_out);
    // the state of an XE forward pass (rows_t, n_tokens) and the Philox seed upload
    void begin_xe(const int32_t* lengths, int B, int T, int L, const int64_t* captions, bool train, uint64_t seed, hipStream_t st);
    // its twin for a sampled rollout of `rows` rows (every row stored at every step) into the caller's seq_out / logp_out [rows, T]
    void begin_rollout(int rows, int T, const int64_t* seq_out, const float* logp_out, uint64_t seed, hipStream_t st);
    // The start of a backward pass.  check_loss_head: the rules of `hd` against the stored pass, on the host before anything is queued
    // (grads: the entry's gradient table, for the null-argument rule of the entries that leave it to the handle).  launch_loss_head:
    // its launches alone, dlogits over `logits` in place (rows / row0 as reinforce); a ROLLOUT head may sit inside a captured graph.
    // begin_backward: the one place that marks the stored pass consumed, outside any capture -- the normaliser of a ROLLOUT head, then
    // either the head's launches (consumed once they all went through: a head that fails leaves the pass stored) or, in_graph, a head
    // the caller launches itself inside its captured graph (consumed at once, whatever the capture returns).
    int check_loss_head(const LossHead& hd, const void* grads) const;
    int launch_loss_head(const LossHead& hd, float* logits, int V, int ldl, hipStream_t st, int rows = 0, int row0 = 0);
    int begin_backward(const LossHead& hd, bool in_graph, float* logits, int V, int ldl, hipStream_t st, int rows = 0, int row0 = 0);
    void captions_to_tok(int64_t* tok, hipStream_t st) const;
    // logits [T B, ldl] <-> packed rows [n_tokens, V] through the packed-sequence index
    int gather_packed(const float* logit, int V, int ldl, float* packed_out, hipStream_t st);
    int scatter_packed(const float* dpacked, int V, int ldl, float* logit, hipStream_t st);
    // LabelSmoothingLoss: loss and dlogits (in place) of the stored XE forward pass
    int xe_loss(float smoothing, float n_tokens_global, float* logits, int V, int ldl, float* loss_out, hipStream_t st);
    // the same behind a grouped XE forward (cur_B image-major rows, every row stored at every step): the mask is t < len[row] (device)
    int xe_group_loss(const int32_t* len, float smoothing, float n_tokens_global, float* logits, int V, int ldl, float* loss_out, hipStream_t st);
    // Distillation (distill.hip): the mixed hard / soft-target loss and dlogits (in place) of the stored XE forward pass against the
    // teachers' packed logits; loss_out3 = {loss, sum hard / N, sum kd / N}.  alpha = 0 is xe_loss.
    int distill_loss(const DistillArgs& a, float n_tokens_global, float* logits, int V, int ldl, float* loss_out3, hipStream_t st);
    // SCST on without-replacement samples (swor_objective.hip): loss and dlogits (in place) of the stored XE forward pass on the sampled
    // captions; loss_out [1 + images] = {loss, sum c logp by image}.  check_swor: the rules against the stored XE forward pass (a
    // training-mode one, teacher-forced, of `rows` rows), before anything is queued.
    int check_swor(const char* who, int rows) const;
    int swor_loss(const SworArgs& a, float* logits, int V, int ldl, float* loss_out, hipStream_t st);
    int require_teacher_forced(const char* who) const;      // the stored XE forward pass fed the captions' own tokens (no scheduled sampling)
    // REINFORCE: loss, mask sum and dlogits (in place) of the stored rollout; rows / row0: rows per step slot and the first of the
    // sampled rollout's (a merged SCST chain stores 2 B rows per slot)
    int reinforce(const float* reward, float* logits, int V, int ldl, float* loss_out, float* msum_out, hipStream_t st, int rows = 0, int row0 = 0);
    // An SCST objective in the place of reinforce (scst_objective.hip): kind 0 with entropy_weight 0 calls reinforce itself;
    // loss_out3 = {loss, obj, ent}, ent_out [rows of the rollout, T] optional.  check_objective: the rules of icz_scst_objective
    // against the stored rollout (cur_K = its samples per image), before anything is queued.
    int check_objective(const char* who, const icz_scst_objective* obj) const;
    int scst_objective(const ScstObjective& o, float* logits, int V, int ldl, float* loss_out3, float* ent_out, float* msum_out, hipStream_t st,
                       int rows = 0, int row0 = 0);
    int rollout_head(const RolloutHead& hd, float* logits, int V, int ldl, hipStream_t st, int rows = 0, int row0 = 0);
    void set_msum_global(float msum_global, hipStream_t st) const;       // < 0: keep the device value handed over by icz_*_set_norm_global
    int upload_pack_index(hipStream_t st);
};

// The launch sites of the two loss heads, shared by CaptionHead::xe_loss / reinforce and the test entries icz_test_xe_loss /
// icz_test_reinforce (include/icz.h).  xe: rows_t[T] active rows per step, 1 / n the host normaliser, n_dev the optional device one;
// loss_rows [T B] is zeroed first.  reinforce: rows / row0 as CaptionHead::reinforce.
int launch_xe_loss(float* logits, int V, int ldl, const int64_t* captions, int L, int B, int T, const int* rows_t, float smoothing, float n,
                   const float* n_dev, float* loss_rows, float* loss_out, hipStream_t st);
int launch_reinforce(const float* logp, const int64_t* seq, const float* reward, int B, int T, const float* msum_dev, float* coef, float* loss_out,
                     float* msum_out, float* logits, int V, int ldl, const int32_t* draw, const float* lse, int rows, int row0, hipStream_t st);
// The XE loss head over image-major rows (xe_group_loss_dlogits_kernel + sum_scale_kernel), shared by CaptionHead::xe_group_loss and
// icz_test_xe_group_loss: len [rows] (device) = steps of each row, the active (row, t) are those with t < len[row]; every (row, t) of
// loss_rows [T rows] is written.  Beside it the other pieces of a grouped XE forward: the host step counts -> device (kernel arguments,
// no copy), the token rows (<pad> behind a row's end) and the logits out [rows, T, V] (zeros behind a row's end).
int launch_xe_group_loss(float* logits, int V, int ldl, const int64_t* captions, int L, int rows, int T, const int32_t* len, float smoothing,
                         float n, const float* n_dev, float* loss_rows, float* loss_out, hipStream_t st);
void upload_lengths(int32_t* dst, const int32_t* lengths_host, int n, hipStream_t st);
void launch_captions_to_tok_len(const int64_t* captions, int rows, int L, int T, const int32_t* len, int64_t* tok, hipStream_t st);
void launch_gather_rows(const float* logit, int V, int ldl, int rows, int T, const int32_t* len, float* out, hipStream_t st);

// The launch site of the SCST objectives, shared by CaptionHead::scst_objective and icz_test_scst_objective; arguments as launch_reinforce
int scst_objective_args(const char* who, const icz_scst_objective* o, int rows, int T, ScstObjective* out);
int launch_scst_objective(const ScstObjective& o, const float* logp, const int64_t* seq, int B, int T, const float* msum_dev,
                          const ScstScratch& w, float* coef, float* out3, float* ent_out, float* msum_out, float* logits, int V, int ldl,
                          const int32_t* draw, const float* lse, int rows, int row0, hipStream_t st);

// The launch site of the without-replacement SCST head, shared by CaptionHead::swor_loss and icz_test_swor_objective
int swor_args(const char* who, const icz_swor_opts* o, int rows, SworArgs* out);
int launch_swor_objective(const SworArgs& a, float* logits, int V, int ldl, const int64_t* captions, int L, int B, int T, const int* rows_t,
                          const SworScratch& w, float* loss_rows, float* loss_out, hipStream_t st);

// Where one decoder step left its logits: ns == 1 finished rows [rows][ld]; ns > 1 the predict GEMM's split-K slabs [ns][rows][ld]
// (slab z at p + z * slab_stride, no bias yet) + bias[v], summed in slab order as greedy_select_kernel / sample_select_kernel do.
struct LogitsView { const float* p; const float* bias; size_t slab_stride; int ld; int ns; };
// the view of a step whose predict GEMM (gemm_predict) reported `pns` slabs in `ws`, or finished rows in `logits`
inline LogitsView logits_view(const float* ws, const float* bias, const float* logits, int rows, int Vp, int pns) {
    return pns > 1 ? LogitsView{ws, bias, (size_t)rows * Vp, Vp, pns} : LogitsView{logits, nullptr, 0, Vp, 1};
}

struct DecodeMember;
constexpr int ENS_MAX_M = 4;          // members of one beam search / ensemble

struct BeamBuf;
struct SbsBuf;
// An ensemble's side of a beam search (ensemble.hip): its own beam buffers, allocated from `mem` for `cap` rows, and its route to the
// rows the search scores: run(lv, rows) combines the members' views of one step into lp [rows, ld].  A single handle has none: the
// search runs on the member's own bm / buffers() / row_capacity() and reads its finished rows.
struct BeamCombine {
    const char* who;                  // the entry, named by the member checks
    BeamBuf* bm; DeviceBuffers* mem; int cap;
    const float* lp; int ld;
    std::function<void(const LogitsView* lv, int rows)> run;
    SbsBuf* sbs = nullptr;            // its stochastic-beam buffers (sample_distinct); the beam searches leave it unset
};

// Beam-search buffers and the step loop shared by the decoders (beam.hip).
struct BeamBuf {
    int cap_rows = 0, cap_L = 0;
    int* n_act = nullptr; float* run = nullptr; int32_t* seqs[2] = {nullptr, nullptr};
    int32_t *src_row = nullptr, *img_of_row = nullptr, *best_seq = nullptr;
    float* best_score = nullptr; int *best_len = nullptr, *has_complete = nullptr, *n_live = nullptr, *n_live_host = nullptr;
    int64_t* it = nullptr;            // the token rows of the search: every member steps on them
    float* cand_val = nullptr; int* cand_idx = nullptr;     // [rows, BEAM_MAX_K] per-row candidates of one step
    int32_t* hyp_seq = nullptr; float* hyp_score = nullptr; int *hyp_len = nullptr, *hyp_cnt = nullptr;    // n-best list (BeamArgs)
    // constrained search (BeamCons, beam_kernels.h): capacity per (image, state), forced-candidate scores [rows, 12], state of a retirement
    int* cap = nullptr; float* force_val = nullptr; int32_t* hyp_state = nullptr;
    BeamBuf() = default;
    BeamBuf(const BeamBuf&) = delete;
    BeamBuf& operator=(const BeamBuf&) = delete;
    ~BeamBuf() { if (n_live_host) (void)hipHostFree(n_live_host); }

    static int check(const char* who, int n_img, int k, int max_steps, int max_rows);
    static int check_opts(const char* who, int k, const icz_beam_opts* o);      // the icz_*_beam_search_opts argument rules
    static const icz_beam_opts defaults;                                       // n_best 1, no blocking, no length penalty
    static int check_diversity(const char* who, int k, const icz_beam_diversity* d);   // the icz_*_beam_search_diverse rules
    static const icz_beam_diversity no_diversity;                             // one group: the plain search
    // The icz_*_beam_search_constrained rules that need no handle, in their documented order: the struct (C in 0..3, A in 1..4, the
    // host words), beam in 1..8, 2^C * beam <= 32, and every image's words (filled from the left, in no constraint twice, not
    // <pad> / <sta> / <end>).  *any = whether some image has a constraint (none: the call is the _opts search).
    static int check_constraints(const char* who, int n_img, int beam, const icz_beam_constraints* c, bool* any);
    static int check_constraint_vocab(const char* who, int n_img, int V, const icz_beam_constraints* c);      // every word below V
    int ensure(DeviceBuffers& m, int max_rows, int L);
    // scores, live counts and the <sta> rows of every image; states > 1 (a constrained search, k = states * beam): state 0 starts
    // with one live beam, the others empty, every capacity at beam
    int begin(int n_img, int k, int L, hipStream_t st, int states = 1);
    // The step loop (DecoderRNN.beam_search_sample, BUTD_Model.py:236-318, batched over images): every member's step runs the
    // decoder on `it`; the rows scored are the one member's finished logits or the ensemble's combined rows (BeamCombine); then a
    // row-top-k, the per-image merge and every member's gather re-gathering the model state by source row; every few steps one
    // 4-byte read-back asks whether any image still has live beams.  Step 1 is compact when every member's compact_step() holds:
    // one decoder row per image (the k rows of an image are identical and only row 0 is scored, :273-274).
    // Options (icz_beam_opts, checked by check_opts): block_ngram goes to the row-top-k; n_best > 1 or a length penalty keeps the
    // n-best list in the merge and ranks it in beam_finalize_nbest_kernel (seqs_out [n_img, n_best, L], lens_out / scores_out
    // [n_img, n_best]).  At the defaults the launches are today's; scores_out (may be null) receives the raw score of the caption.
    // Diversity (icz_beam_diversity, checked by check_diversity): groups > 1 keeps n_act per (image, group), runs the grouped
    // row-top-k instances and beam_merge_groups_kernel, and always keeps the n-best list; one group launches the plain kernels.
    // Constraints (icz_beam_constraints, checked by check_constraints; null = none, with one group only): k = 2^C * beam rows per
    // image, state-major; n_act and cap per (image, state); the constrained row-top-k instances, beam_merge_states_kernel and
    // beam_finalize_states_kernel, which also writes sat_out [n_img, n_best].  The decoder steps are the same.
    int search(DecodeMember* const* m, int M, const BeamCombine* ens, int n_img, int k, int max_steps, float* seqs_out, int32_t* lens_out,
               const icz_beam_opts& o, const icz_beam_diversity& d, float* scores_out, hipStream_t st,
               const icz_beam_constraints* cons = nullptr, int32_t* sat_out = nullptr);
};

// Buffers of stochastic beam search (stochastic_beam.hip, sbs_kernels.h): per row the hypothesis (tokens ping-pong, phi, G, frozen,
// length), per image the occupied slots, the per-row candidates of one step and the per-step counts of live rows with their pinned
// read-back word; sized once for the owner's row capacity and 256 steps.  Allocated from a handle's or an ensemble's DeviceBuffers, beside its beam buffers.
struct SbsBuf {
    int cap_rows = 0;
    int *occ = nullptr, *len = nullptr, *n_live = nullptr, *n_live_host = nullptr;
    uint8_t* frozen = nullptr; float* phi = nullptr; double* G = nullptr;
    int32_t* seqs[2] = {nullptr, nullptr};
    int32_t *src_row = nullptr, *img_of_row = nullptr;
    int64_t* it = nullptr;
    float *cand_g = nullptr, *cand_phi = nullptr; int* cand_idx = nullptr;
    SbsBuf() = default;
    SbsBuf(const SbsBuf&) = delete;
    SbsBuf& operator=(const SbsBuf&) = delete;
    ~SbsBuf() { if (n_live_host) (void)hipHostFree(n_live_host); }
    int ensure(DeviceBuffers& m, int max_rows);
};

// The per-image work, one decoder step and the beam-state gather of a decoder: the BUTD, AoA and NIC handles implement it, the
// drivers below run on it -- beam_search on one member (a handle's own search) or on several at once (the model ensemble, ensemble.hip).
// State: a step reads slot `cur` of the recurrent state and writes slot cur ^ 1; gather() moves slot 1 into slot 0 by source row.
struct DecodeMember {
    virtual ~DecodeMember() = default;
    virtual int vocab() const = 0;
    virtual int row_capacity() const = 0;
    virtual bool refreshed() const = 0;
    virtual bool compact_step() const = 0;      // beam step 1 may run one row per image (gather then fans it out to the k rows)
    // per-image work for n_img images, k state rows each (zeroed, or NIC's image step; img_of_row: image of each of the n_img k rows)
    virtual int prologue(const float* feats, int n_img, int k, const int32_t* img_of_row, hipStream_t st) = 0;
    // one step over `rows` rows on the caller's tokens `it`; img_of_row null = row i is image i.  slabs: the caller's consumer sums
    // split-K slabs (the view reports which form the logits are in)
    virtual int step(int rows, const int64_t* it, const int32_t* img_of_row, int rows_per_img, int cur, bool slabs, LogitsView* out,
                     hipStream_t st) = 0;
    virtual void gather(const int32_t* src_row, int rows, int fan, hipStream_t st) = 0;
    // ---- the sampling decode (sample_decode.hip) ----
    // where step() reads its input embedding: emb[row, :E] = table[it[row]] (relu: behind a ReLU), no dropout in evaluation mode
    struct EmbSlot { const float* table; float* emb; int E; int relu; };
    virtual EmbSlot emb_slot() const = 0;
    virtual DeviceBuffers& buffers() = 0;       // the handle's allocations: the driver's buffers live and die with them
    // Set around a step() by a driver whose select kernel has written emb_slot() for the rows' tokens itself (the step skips its
    // embedding kernel) and keeps the count of unfinished rows (step_dead, icz_common.h); every other caller leaves them alone.
    bool seam_emb_ready = false;
    const int* seam_live = nullptr;
    struct SampleBuf { int cap_rows = 0, cap_T = 0; int64_t* it = nullptr; uint8_t* fin = nullptr; int* n_unf = nullptr; int32_t* img_of_row = nullptr; } sb;
    BeamBuf bm;                                 // a handle's own beam search (beam_search with no BeamCombine); an ensemble keeps its own
    SbsBuf sbs;                                 // a handle's own stochastic beam search (sample_distinct), likewise
};
// an ensemble call of `rows` decoder rows: features, refreshed weights and row capacity of every member (`who` names the entry)
int check_members(const char* who, DecodeMember* const* m, int M, const float* const* feats, int rows);
// Beam search over M >= 1 members on the caller's stream (include/icz.h: icz_*_beam_search*): every check, then BeamBuf::ensure,
// begin, every member's prologue, the step loop and the final selection (BeamBuf::search).  `who` names the family in the errors.
// ens null: M = 1, a handle's own search, scoring the member's finished logits.
// cons (null = none): a constrained search of `k` beams per state (icz_*_beam_search_constrained), its words checked against the
// vocabulary here; sat_out [n_img, n_best] receives the states.
int beam_search(const char* who, DecodeMember* const* m, int M, const BeamCombine* ens, const float* const* feats, int n_img, int k,
                int max_steps, const icz_beam_opts& o, const icz_beam_diversity& d, float* seqs_out, int32_t* lens_out, float* scores_out,
                hipStream_t st, const icz_beam_constraints* cons = nullptr, int32_t* sat_out = nullptr);
// The argument checks of an icz_*_beam_search_constrained entry that come before its handle: the options as _opts, the constraints
// (BeamBuf::check_constraints), null arguments.  *cons_out = `cons` if some image has a constraint, else null (the _opts search).
int beam_constrained_args(const char* entry, int n_img, int beam, const icz_beam_opts* opts, const icz_beam_constraints* cons, bool ptrs_ok,
                          const icz_beam_constraints** cons_out);
// The greedy select tail of a decoder step: the argmax of the step's logits becomes it[row] and ids_out[row, t] (row stride T) and its
// embedding row goes to the member's EmbSlot for the next step.  Split-K slabs (lv.ns > 1; 33 - 64 rows): one launch of
// greedy_select_kernel, which also keeps the SCST baseline's count of unfinished rows (gunf / gn, may be null); finished rows: the
// two-kernel argmax over ARGMAX_PARTS slices of the vocabulary (amax_val / amax_idx [rows, ARGMAX_PARTS]), which does not.
constexpr int ARGMAX_PARTS = 8;
void launch_greedy_select(const LogitsView& lv, const DecodeMember::EmbSlot& e, int rows, int V, float* amax_val, int* amax_idx, int64_t* it,
                          int64_t* ids_out, int T, int t, uint8_t* gunf, int* gn, hipStream_t st, int route = 0);
// The sampling decode on a member: prologue once per image, the rows expanded through img_of_row, then max_len steps of the
// member's step + sample_decode_kernel (include/icz.h: icz_*_sample_decode; `who` names the entry in its errors).
int sample_decode(DecodeMember* m, const char* who, const float* feats, int n_img, int n, int max_len, const icz_sample_opts* opts,
                  uint64_t seed, const float* uniforms, int64_t* ids_out, float* logp_out, float* score_out, hipStream_t st);
// Stochastic beam search over M >= 1 members (stochastic_beam.hip; include/icz.h: icz_*_sample_distinct): n distinct captions per
// image, a sample without replacement from the (tempered) sequence distribution.  On the seams of beam_search: every check, then
// SbsBuf::ensure, the start state, every member's prologue, and per step every member's step, the ensemble's run (ens non-null: the
// combined rows; null: M = 1, the member's own logits, split-K slabs included), sbs_rowtopk_kernel, sbs_merge_kernel and every
// member's gather.  `who` names the entry in the errors.  The argument rules that need no handle: sample_distinct_check.
// first_image: the index of this call's image 0 within its batch, added to the image index of the Philox counter, so that a batch
// decoded in chunks draws the noise of the whole batch (explicit uniforms ignore it).
int sample_distinct_check(const char* who, int n_img, int n, int max_len, float temperature, int V, int max_rows, int first_image);
int sample_distinct(const char* who, DecodeMember* const* m, int M, const BeamCombine* ens, const float* const* feats, int n_img, int n,
                    int max_len, float temperature, uint64_t seed, int first_image, const float* uniforms, const float* root_uniforms,
                    const icz_sample_distinct_out* out, hipStream_t st);
// Scoring given captions on a member (score_captions.hip; include/icz.h: icz_*_score_captions): prologue once per image, then
// max_len steps of the member's step on the fed tokens + score_tokens_kernel.
int score_captions(DecodeMember* m, const char* who, const float* feats, int n_img, int n, int max_len, const int64_t* ids,
                   float* logp_out, float* score_out, hipStream_t st);
enum { ICZ_MEMBER_BUTD = 0, ICZ_MEMBER_AOA = 1, ICZ_MEMBER_NIC = 2 };
DecodeMember* butd_member(void* handle);        // the seams of an icz_butd_t / icz_aoa_t / icz_nic_t
DecodeMember* aoa_member(void* handle);
DecodeMember* nic_member(void* handle);

// C ABI helpers (butd.hip, aoa.hip, nic.hip)
template <class Handle, class Dims, class Opaque>
int abi_create(const char* who, const Dims* dims, Opaque** out) {
    ICZ_REQUIRE(dims && out, "%s: null argument", who);
    Handle* h = new Handle();
    const int s = h->init(*dims);
    if (s != ICZ_OK) { delete h; return s; }
    *out = reinterpret_cast<Opaque*>(h);
    return ICZ_OK;
}
// every parameter pointer non-null and 16-byte aligned (bit i of `unaligned_ok`: parameter i may be unaligned)
int check_param_table(const char* who, const void* params, size_t bytes, uint32_t unaligned_ok = 0);
int set_scheduled_sampling(const char* who, CaptionHead* h, float ss_prob, const float* gate, const float* draw);
int set_norm_global(const char* who, CaptionHead* h, const float* norm_dev, void* stream);

}  // namespace icz
