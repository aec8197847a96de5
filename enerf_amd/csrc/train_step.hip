// train_step.hip -- one closed-form training step as ONE call (host code only: every launch is one of the library's
// own entry points, in the order the Python harness issues them -- enerf_amd/fused_render.train_step_mse +
// fused_network.nerf_forward / nerf_backward + FusedAdam.step_grid_table -- so the two routes are bit-identical).
//
// Why: with the kernels of a 4096-ray step at ~0.32 ms, the ~28 launches of a step cost the Python harness ~0.4 ms of
// host time (argument marshalling, tensor checks, dispatcher calls between the launches): the host, not the device,
// bounds the step.  Here the host's share of a step is one struct and one call.
//
// The step has three forms -- the RGB step (enerf_train_step_mse), the event step with both renders as one batch of 2 M
// rows, the event step render by render -- and ONE body: a Batch of rows goes through
//     forward():        grid_encode_forward (extra workgroups of its launch build the fused MLP's operand fragments)
//                       -> nerf_mlp_forward, or mlp32 forward x 2 (sigma net + SH columns, colour net)
//     [the form's own compositing forward, loss gradient, compositing backward]
//     backward():       nerf_mlp_backward, or mlp32 backward x 2 (weight-gradient sums: a reduce launch, or the optimizer's)
//     table_backward(): grid_encode_backward (record lists)
//     optimizer():      table Adam from the records + the MLP weights' Adam (one launch)
// The NEXT batch's march runs on the side stream behind the MLP backward, whose last launch carries the signal that stream
// waits for (marches_side), or without a second stream: its count pass rides in the optimizer's launch, scan + write follow
// it (marches_begin, optimizer).  What rides in another kernel's launch -- the fragments' build, the weight-gradient sums,
// the count passes -- and what modifies an MLP launch -- the rows that count, the arithmetic mode, the completion signal, the
// two nets' shared reduce launch -- is an argument of that launch's internal entry point (common.h) and a local value here;
// so are the next march's near / far request and count mirror (next_count_host).  The step neither reads nor changes the
// process's enerf_mlp32_* settings, bar the arithmetic mode where mlp_precision < 0, nor the public marches' one-shot requests
// (enerf_march_fuse_near_far, enerf_march_mirror_count).  Where its next marches ran it says in the struct's `report`.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>

#include "common.h"

using namespace enerf;

// development aid (enerf_debug_step_timing): host microseconds spent in each call of the step, summed over steps
static double g_host_us[16];
static uint64_t g_host_steps = 0;
static bool g_host_timing = false;
// the fused MLP's operand fragments built inside the grid forward's launch (ENERF_NO_CARRY_FRAGS: by their own launch)
static bool g_carry_frags = getenv("ENERF_NO_CARRY_FRAGS") == nullptr;      // enerf_debug_carry_frags
// the fused MLP's weight-gradient partial sums summed by the optimizer's launch (ENERF_NO_FOLD_REDUCE: by k_mlp32_reduce_w2)
static bool g_fold_reduce = getenv("ENERF_NO_FOLD_REDUCE") == nullptr;      // enerf_debug_fold_reduce
// the next batch's march without a second stream: its count pass rides in the table optimizer's launch, scan + write are one
// launch behind it (common.h MarchCountJob; ENERF_NO_CARRY_COUNT / enerf_debug_carry_count(0): the side-stream march)
static bool g_carry_count = getenv("ENERF_NO_CARRY_COUNT") == nullptr;
static int g_carried_steps = 0;          // steps whose next batch was marched that way so far (enerf_debug_carry_count(-2))
extern "C" int enerf_debug_carry_count(int on) {
    if (on == -2) return g_carried_steps;
    const int prev = g_carry_count ? 1 : 0;
    if (on >= 0) g_carry_count = on != 0;
    return prev;
}

namespace {

// What one function of the step hands a later one, and the host timer.
class Step {
public:
    int mode;                              // the MLP launches' arithmetic: the call's mlp_precision, or the process's
    bool fused;                            // both nets as one launch each way (csrc/nerf_mlp.hip: the split-bf16 default)
    hipEvent_t signalled = nullptr;        // the event the MLP backward's last launch carried, for the side stream to wait on
    // for the optimizer's launch: the fused backward's weight-gradient partial sums (has_sums) ...
    PartialSums sums{nullptr, nullptr, 0, 0, 0};
    bool has_sums = false;
    // ... and the next marches' count passes, with the scan + write that follow them (the first `counts`)
    MarchCountJob count_jobs[2] = {};
    CarriedMarch marches[2] = {};
    uint32_t counts = 0;

    template <class A>
    Step(const A* a, bool timed) : timed_(timed) {
        mode = (a->mlp_precision >= 0 && a->mlp_precision <= 3) ? a->mlp_precision : enerf_mlp32_precision(-1);
        fused = a->nh_s == 1 && a->nh_c == 2 && nerf_mlp_available(mode);
        if (timed_) {
            g_host_steps++;
            t_prev_ = std::chrono::steady_clock::now();
        }
    }

    // Every timed call of the step passes its result through here: the host time since the previous one goes to the call's
    // slot (enerf_debug_step_timing).  A call that stands for `slots` calls of the unfused route occupies as many; 0: the time
    // is counted with the call that follows.
    int run(int rc, int slots = 1) {
        if (timed_) {
            const auto t_now = std::chrono::steady_clock::now();
            g_host_us[slot_ < 15 ? slot_ : 15] += std::chrono::duration<double, std::micro>(t_now - t_prev_).count();
            t_prev_ = t_now;
            slot_ += slots;
        }
        return rc;
    }

private:
    bool timed_;
    int slot_ = 0;
    std::chrono::steady_clock::time_point t_prev_;
};

// A batch of rows through the networks: the RGB step's M rows, the merged event step's 2 M, one render of the event step.
struct Batch {
    uint32_t rows, total;                  // total: the rows the record lists of the table backward reserve
    const int32_t* counter;                // valid rows = base + min(*counter, cap) (cap == 0: *counter); nullptr: all
    uint32_t base, cap;
    const float *xyzs, *dirs;
    float *feats, *h32, *fb_s, *fb_c, *sigma, *rgb, *g_sigmas, *g_rgbs, *dx32, *dfeat;
    uint32_t overwrite;                    // weight gradients: 1 written, 0 added to what is there
};
// (enerf_train_step_args and enerf_step_render name these fields alike; flags: the call's, for ENERF_STEP_EVERY_ROW)
template <class R>
Batch batch_of(const R& r, uint32_t total, uint32_t overwrite, uint32_t flags) {
    return {r.M,    total,  (flags & ENERF_STEP_EVERY_ROW) ? nullptr : r.counter, 0, 0, r.xyzs, r.dirs, r.feats, r.h32,
            r.fb_s, r.fb_c, r.sigma, r.rgb, r.g_sigmas, r.g_rgbs, r.dx32, r.dfeat, overwrite};
}

struct NextMarch {
    const float *rays_o, *rays_d;
    uint32_t N, M;
    float *nears, *fars, *xyzs, *dirs, *deltas;
    int32_t *rays, *counter;
    int32_t* count_host;                   // the counter's mirror in pinned host memory (next_count_host), or nullptr
};
template <class R>
uint32_t add_next(const R& r, NextMarch* list, uint32_t n, int32_t* count_host = nullptr) {
    if (!r.next_rays_o) return n;
    list[n] = {r.next_rays_o, r.next_rays_d, r.next_N,      r.next_M,    r.next_nears,   r.next_fars,
               r.next_xyzs,   r.next_dirs,   r.next_deltas, r.next_rays, r.next_counter, count_host};
    return n + 1;
}

// A: enerf_train_step_args or enerf_event_step_args (their network, march and optimizer fields carry the same names)

// `carry`: the fused MLP's fragments may be built by the grid forward's launch (common.h SplitJob); `frags`: they are current
template <class A>
int forward(Step& st, const A* a, const Batch& b, bool carry, uint32_t frags) {
    enerf_stream_t s = a->stream;
    SplitJob job{};
    const bool ride = st.fused && carry && g_carry_frags;
    if (ride)
        if (int rc = st.run(nerf_mlp_frag_job(a->wseg_s, a->wseg_c, a->w0_cols_c, a->out_c, (hipStream_t)s, &job), 0)) return rc;
    bool carried = false;
    if (int rc = st.run(grid_encode_forward(b.xyzs, a->embeddings, a->offsets, b.feats, b.rows, 3, 2, 16, a->level_scale_log2,
                                            a->base_resolution, 0, b.feats, a->gridtype, ENERF_F32, 2, a->bound,
                                            a->inv_two_bound, s, {b.counter, b.base, b.cap}, ride ? &job : nullptr, &carried)))
        return rc;
    if (carried) {                         // the grid forward built the fragments, the MLP calls are told so
        nerf_mlp_frags_built(job, a->w0_cols_c, a->out_c);
        frags = 1;
    }
    // (the budget's unfilled rows are skipped by the MLP launches as by the grid's)
    const MlpCall c = {{b.counter, b.base, b.cap}, st.mode, false};
    if (st.fused)
        return st.run(nerf_mlp_forward(b.feats, b.dirs, a->wseg_s, a->wseg_c, a->w0_cols_c, b.rows, a->out_c, b.sigma, b.rgb,
                                       frags, s, c),
                      2);
    if (int rc = st.run(mlp32_forward_p(b.feats, a->wseg_s, 32, 0, b.rows, 32, 16, a->nh_s, 0, 6, b.fb_s, b.h32, 1, 32, b.sigma,
                                        b.dirs, s, c)))
        return rc;
    return st.run(mlp32_forward_p(b.h32, a->wseg_c, a->w0_cols_c, 1, b.rows, 32, a->out_c, a->nh_c, 0, 3, b.fb_c, b.rgb, 0, 0,
                                  nullptr, nullptr, s, c));
}

// `signal`: the last launch carries the signal the side stream's marches wait for; `fold`: the optimizer follows in this call
// and may sum the fused backward's weight-gradient partial sums in its own launch (common.h PartialSums: no reduce launch)
template <class A>
int backward(Step& st, const A* a, const Batch& b, bool signal, bool fold) {
    enerf_stream_t s = a->stream;
    const MlpCall c = {{b.counter, b.base, b.cap}, st.mode, false};
    if (st.fused) {
        if (fold && g_fold_reduce)
            st.has_sums = nerf_mlp_partial_job(a->dwseg_s, a->dwseg_c, a->w0_cols_c, a->out_c, a->small_g, a->small_n, a->n_small,
                                               b.rows, (hipStream_t)s, &st.sums) == 0;
        return st.run(nerf_mlp_backward(b.g_rgbs, b.g_sigmas, 1.0f, b.feats, b.dirs, b.rgb, a->wseg_s, a->wseg_c, a->dwseg_s,
                                        a->dwseg_c, a->w0_cols_c, b.overwrite, b.rows, a->out_c, b.dfeat, st.has_sums ? 3u : 1u,
                                        s, c, signal, &st.signalled),
                      2);
    }
    DeferredReduce pair = {};              // (the colour net's partial sums wait for the sigma net's reduce launch)
    if (int rc = st.run(mlp32_backward_p(b.g_rgbs, b.h32, a->wseg_c, a->dwseg_c, a->w0_cols_c, 1, b.overwrite, b.fb_c, b.rows, 32,
                                         a->out_c, a->nh_c, 0, nullptr, b.dx32, 0, 0, b.rgb, a->out_c, nullptr, nullptr, 0, s, c,
                                         false, nullptr, &pair)))
        return rc;
    return st.run(mlp32_backward_p(b.dx32, b.feats, a->wseg_s, a->dwseg_s, 32, 0, b.overwrite, b.fb_s, b.rows, 32, 16, a->nh_s, 0,
                                   nullptr, b.dfeat, 1, 32, nullptr, 0, b.g_sigmas, b.h32, 32, s, c, signal, &st.signalled, &pair));
}

// The next marches carried by the optimizer's launch where that applies: all of them or none (st.counts).  Decided in front
// of the MLP backward, because the side-stream form has that call's last launch carry its signal.
template <class A>
int marches_begin(Step& st, const A* a, const NextMarch* next, uint32_t n, bool carry) {
    if (!carry || !g_carry_count || (a->march_flags & 16u)) return 0;
    for (uint32_t q = 0; q < n; q++)
        if (next[q].count_host) return 0;  // (the carried scan + write has no mirror store)
    for (uint32_t q = 0; q < n; q++) {
        const NextMarch& m = next[q];
        // (near / far inside the count pass; the second pending march logs into a workspace of its own)
        const int b = march_carry_begin(m.rays_o, m.rays_d, a->bitfield, a->bound, a->dt_gamma, a->max_steps, m.N, a->cascade,
                                        a->grid_size, m.M, m.nears, m.fars, m.xyzs, m.dirs, m.deltas, m.rays, m.counter,
                                        a->perturb, a->march_flags, a->aabb, a->min_near, (hipStream_t)a->stream,
                                        q == 0 ? WS_MARCH : WS_MARCH2, &st.count_jobs[q], &st.marches[q], n);
        if (b < 0) return b;
        if (b != 0) return 0;              // not this way after all: every march takes the side stream
    }
    st.counts = n;
    return 0;
}

// ... and on the side stream, behind the MLP backward (a march reads no parameter)
template <class A>
int marches_side(Step& st, const A* a, const NextMarch* next, uint32_t n) {
    enerf_stream_t ss = a->side_stream;
    if (!st.signalled) ENERF_BADARG("train_step: no launch of the MLP backward carried the signal the side stream waits for");
    if (int rc = st.run(check_hip(hipStreamWaitEvent((hipStream_t)ss, st.signalled, 0), "train_step: side stream wait")))
        return rc;
    for (uint32_t q = 0; q < n; q++) {
        const NextMarch& m = next[q];
        // (near / far inside the march's count pass: one launch less at the head of the chain the next step waits for)
        if (int rc = st.run(march_rays_train(m.rays_o, m.rays_d, a->bitfield, a->bound, a->dt_gamma, a->max_steps, m.N,
                                             a->cascade, a->grid_size, m.M, m.nears, m.fars, m.xyzs, m.dirs, m.deltas, m.rays,
                                             m.counter, a->perturb, a->march_flags, a->aabb, a->min_near, m.count_host, ss)))
            return rc;
    }
    return 0;
}

// defer 1: record lists for the optimizer pass (b.total rows reserved); 0: the backward's own flush into the dense buffer
template <class A>
int table_backward(Step& st, const A* a, const Batch& b, uint32_t defer) {
    return st.run(grid_encode_backward(b.dfeat, b.xyzs, a->offsets, a->table_grad, b.rows, 3, 2, 16, a->level_scale_log2,
                                       a->base_resolution, 0, b.dfeat, b.dfeat, a->gridtype, ENERF_F32, 2, a->bound,
                                       a->inv_two_bound, defer, defer ? b.total : 0u, a->stream, {b.counter, b.base, b.cap}));
}

// Table Adam from the records + the MLP weights' Adam, with what the step hands the launch (weight-gradient sums, count
// passes), and the carried marches' scan + write behind it
template <class A>
int optimizer(Step& st, A* a, const char* who) {
    enerf_stream_t s = a->stream;
    uint32_t taken = 0;
    if (int rc = st.run(grid_adam_from_records(a->table, a->table_grad, a->table_m, a->table_v, a->offsets, 16, 2, a->lr, a->beta1,
                                               a->beta2, a->eps, a->table_step, a->n_small, a->small_p, a->small_g, a->small_m,
                                               a->small_v, a->small_n, a->small_lr, a->small_step, s,
                                               st.has_sums ? &st.sums : nullptr, st.count_jobs, st.counts, &taken)))
        return rc;
    if (st.has_sums && !(taken & ADAM_TOOK_SUMS))
        ENERF_BADARG("%s: the optimizer launch did not take the weight gradients' partial sums", who);
    if (!st.counts) return 0;
    // (an optimizer form that carries nothing -- loss scaling armed -- did not take the jobs: counted by launches of their own)
    if (!(taken & ADAM_TOOK_COUNTS))
        for (uint32_t q = 0; q < st.counts; q++)
            if (int rc = st.run(march_carry_count_now(&st.count_jobs[q], (hipStream_t)s))) return rc;
    if (int rc = st.run(march_carry_end(st.marches, st.counts, (hipStream_t)s))) return rc;
    g_carried_steps++;
    a->report |= ENERF_STEP_MARCH_CARRIED;
    return 0;
}

// compositing of one render of the event step, on its sigma / rgb rows and their gradients
int blend(const enerf_event_step_args* a, const enerf_step_render& r, const float* sigma, const float* rgb) {
    return enerf_composite_rays_train_forward_blend_c(sigma, rgb, r.deltas, r.rays, r.M, r.N, r.weights_sum, nullptr, r.image,
                                                      a->bg_color, 0, 0.0f, r.out_image, a->out_c, a->stream);
}
int blend_backward(const enerf_event_step_args* a, const enerf_step_render& r, const float* sigma, const float* rgb,
                   float* g_sigmas, float* g_rgbs) {
    // (its tail blocks zero the gradients of rows [counter, M): merged, the padding between the two renders' samples)
    return enerf_composite_rays_train_backward_mse_c(r.g_image, nullptr, 1.0f, a->bg_color, 0, 0.0f, r.counter, sigma, rgb,
                                                     r.deltas, r.rays, r.weights_sum, r.image, r.M, r.N, g_sigmas, g_rgbs,
                                                     nullptr, a->out_c, a->stream);
}
// the event loss and its gradient with respect to the two images
int event_loss(const enerf_event_step_args* a) {
    return enerf_event_loss_fwd_bwd_c(a->r[0].out_image, a->r[1].out_image, a->pols, a->r[0].N, a->use_luma, a->linlog,
                                      a->C_thres, a->log_thres, a->upstream, a->r[0].g_image, a->r[1].g_image, a->delta, a->loss,
                                      a->out_c, a->stream);
}

}  // namespace

extern "C" int enerf_train_step_mse(enerf_train_step_args* a) {
    if (!a) ENERF_BADARG("train_step_mse: null arguments");
    if (a->struct_bytes != sizeof(enerf_train_step_args))
        ENERF_BADARG("train_step_mse: struct of %u bytes, this library expects %zu", a->struct_bytes,
                     sizeof(enerf_train_step_args));
    a->report = 0;
    if (a->M == 0 || a->N == 0) return 0;
    Step st(a, g_host_timing);
    // flags bit 0, data parallel: the gradient has to exist to be averaged -- no optimizer here, so nothing rides in its launch
    const bool dp = (a->flags & 1u) != 0;
    const Batch b = batch_of(*a, a->M, 1, a->flags);
    NextMarch next[1];
    const uint32_t n_next = add_next(*a, next, 0, a->next_count_host);
    if (int rc = forward(st, a, b, true, 0)) return rc;
    // compositing forward + loss gradient + compositing backward
    if (int rc = st.run(enerf_composite_rays_train_fwd_bwd_mse_c(a->sigma, a->rgb, a->deltas, a->rays, a->M, a->N, a->weights_sum,
                                                                 a->image, nullptr, 0, a->bg_scalar, a->out_image, a->target,
                                                                 a->grad_scale, a->counter, a->g_sigmas, a->g_rgbs, a->loss,
                                                                 a->out_c, a->stream)))
        return rc;
    if (int rc = marches_begin(st, a, next, n_next, !dp)) return rc;
    const bool side = n_next && !st.counts;
    if (int rc = backward(st, a, b, side, !dp)) return rc;
    if (side)
        if (int rc = marches_side(st, a, next, n_next)) return rc;
    // (flags bit 1: the sharded tail with an owner range set -- enerf_grid_owner_range -- keeps this rank's own slice as
    //  record lists for the optimizer pass and flushes the rest)
    if (dp) return table_backward(st, a, b, (a->flags & 2u) ? 1u : 0u);
    if (int rc = table_backward(st, a, b, 1)) return rc;
    return optimizer(st, a, "train_step_mse");
}

// The event-only step with both renders' samples as ONE batch of 2 M rows (enerf_event_step_args.flags bit 1): compositing
// stays per render, on the halves.  Real rows: the first render's M + min(counter_2, M).
static int train_step_events_merged(enerf_event_step_args* a) {
    const enerf_step_render &r0 = a->r[0], &r1 = a->r[1];
    const uint32_t M = r0.M, M2 = 2 * M;
    if (r1.M != M || r1.xyzs != r0.xyzs + (size_t)3 * M || r1.dirs != r0.dirs + (size_t)3 * M ||
        r1.deltas != r0.deltas + (size_t)2 * M)
        ENERF_BADARG("train_step_events(merged): the second render's samples must follow the first's M rows");
    if (!a->m_feats || !a->m_h32 || !a->m_sigma || !a->m_rgb || !a->m_g_sigmas || !a->m_g_rgbs || !a->m_dx32 || !a->m_dfeat)
        ENERF_BADARG("train_step_events(merged): the m_* scratch buffers are required");
    Step st(a, false);
    const bool skip = !(a->flags & ENERF_STEP_EVERY_ROW) && r0.counter != nullptr && r1.counter != nullptr;
    const Batch b = {M2,         M2,      skip ? r1.counter : nullptr, M, M, r0.xyzs, r0.dirs, a->m_feats, a->m_h32, a->m_fb_s,
                     a->m_fb_c,  a->m_sigma, a->m_rgb, a->m_g_sigmas, a->m_g_rgbs, a->m_dx32, a->m_dfeat, 1};
    NextMarch next[2];
    const uint32_t n_next = add_next(r1, next, add_next(r0, next, 0));
    if (int rc = forward(st, a, b, true, 0)) return rc;
    for (size_t k = 0; k < 2; k++)
        if (int rc = blend(a, a->r[k], b.sigma + k * M, b.rgb + k * M * a->out_c)) return rc;
    if (int rc = event_loss(a)) return rc;
    for (size_t k = 0; k < 2; k++)
        if (int rc = blend_backward(a, a->r[k], b.sigma + k * M, b.rgb + k * M * a->out_c, b.g_sigmas + k * M,
                                    b.g_rgbs + k * M * a->out_c))
            return rc;
    if (int rc = marches_begin(st, a, next, n_next, true)) return rc;
    const bool side = n_next && !st.counts;
    if (int rc = backward(st, a, b, side, true)) return rc;
    if (side)
        if (int rc = marches_side(st, a, next, n_next)) return rc;
    if (int rc = table_backward(st, a, b, 1)) return rc;
    return optimizer(st, a, "train_step_events");
}

// The event-only step (two renders, one loss, one optimizer pass): events.train_step_events_manual +
// FusedAdam.step_grid_table, call for call.  Render by render, nothing rides in another launch: no fragments, weight-gradient
// sums or marches are carried; the second render finds the first's fragments and adds its weight gradients to the first's.
extern "C" int enerf_train_step_events(enerf_event_step_args* a) {
    if (!a) ENERF_BADARG("train_step_events: null arguments");
    if (a->struct_bytes != sizeof(enerf_event_step_args))
        ENERF_BADARG("train_step_events: struct of %u bytes, this library expects %zu", a->struct_bytes,
                     sizeof(enerf_event_step_args));
    a->report = 0;
    if (a->r[0].N == 0 || a->r[0].N != a->r[1].N || a->r[0].M == 0 || a->r[1].M == 0)
        ENERF_BADARG("train_step_events: both renders take the same (non-zero) number of rays and a sample budget");
    if (!a->bg_color || !a->pols) ENERF_BADARG("train_step_events: bg_color and pols are required");
    if (a->flags & 2u) return train_step_events_merged(a);
    Step st(a, false);
    const uint32_t total = a->r[0].M + a->r[1].M;
    const Batch b[2] = {batch_of(a->r[0], total, 1, a->flags), batch_of(a->r[1], total, 0, a->flags)};
    NextMarch next[2];
    const uint32_t n_next = add_next(a->r[1], next, add_next(a->r[0], next, 0));
    for (uint32_t k = 0; k < 2; k++) {
        if (int rc = forward(st, a, b[k], false, k)) return rc;
        if (int rc = blend(a, a->r[k], b[k].sigma, b[k].rgb)) return rc;
    }
    if (int rc = event_loss(a)) return rc;
    for (uint32_t k = 0; k < 2; k++) {
        if (int rc = blend_backward(a, a->r[k], b[k].sigma, b[k].rgb, b[k].g_sigmas, b[k].g_rgbs)) return rc;
        // the next step's marches, on the side stream, behind this step's last MLP backward
        const bool side = k == 1 && n_next;
        if (int rc = backward(st, a, b[k], side, false)) return rc;
        if (side)
            if (int rc = marches_side(st, a, next, n_next)) return rc;
        if (int rc = table_backward(st, a, b[k], 1)) return rc;
    }
    return optimizer(st, a, "train_step_events");
}

extern "C" int enerf_debug_fold_reduce(int on) {
    const int prev = g_fold_reduce ? 1 : 0;
    if (on >= 0) g_fold_reduce = on != 0;
    return prev;
}

extern "C" int enerf_debug_carry_frags(int on) {
    const int prev = g_carry_frags ? 1 : 0;
    if (on >= 0) g_carry_frags = on != 0;
    return prev;
}

// development aid: on != 0 starts (and clears) the per-call host timers of enerf_train_step_mse; out (16 doubles, may
// be NULL) receives the microseconds per call slot, in call order, averaged over the steps since the last start
extern "C" int enerf_debug_step_timing(int on, double* out) {
    if (out)
        for (int k = 0; k < 16; k++) out[k] = g_host_steps ? g_host_us[k] / (double)g_host_steps : 0.0;
    if (on >= 0) {
        g_host_timing = on != 0;
        for (int k = 0; k < 16; k++) g_host_us[k] = 0.0;
        g_host_steps = 0;
    }
    return 0;
}
