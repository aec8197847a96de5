// common.h -- shared host/device helpers for libenerf_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/enerf_hip.h"

namespace enerf {

constexpr int kWave = 64;  // CDNA wavefront

// ---- error plumbing -------------------------------------------------------
void set_error(const char* fmt, ...);

inline int check_hip(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

#define ENERF_BADARG(...)            \
    do {                             \
        enerf::set_error(__VA_ARGS__); \
        return ENERF_E_BADARG;       \
    } while (0)

#define ENERF_LAUNCH_CHECK(name)                                   \
    do {                                                           \
        int _e = enerf::check_hip(hipGetLastError(), name);        \
        if (_e) return _e;                                         \
    } while (0)

// ---- per-kernel-family event timing (include/enerf_hip.h: enerf_prof_*) ---
struct ProfScope {
    int id;
    hipStream_t s;
    void* slot;
    bool ext;
    // ext = true: the caller launches ONE kernel with hipExtLaunchKernelGGL(..., start(), stop(), ...), which stamps the
    // events with the kernel's own begin / end (what rocprofv3 reports) instead of the time between two event packets
    ProfScope(int kernel_id, hipStream_t stream, bool ext = false);
    ~ProfScope();
    hipEvent_t start() const;      // nullptr when this launch is not being timed
    hipEvent_t stop() const;
    void units(double n) const;    // work units of this call (points, samples): summed over the TIMED calls only
};

// ---- loss scaling of the fp16 regime (include/enerf_hip.h: enerf_amp_begin / enerf_amp_end, csrc/optim.hip) ----------
// Between the two calls: the closed-form loss gradient is multiplied by *scale (compositing / event-loss kernels), the MLP
// weight-gradient reduce launch raises *found_inf when a sum is not finite, and the table / MLP Adam launch divides the
// gradients by *scale, counts its step as (host step - *skipped) and leaves p / m / v alone when *found_inf is set.
struct AmpState {
    const float* scale;        // nullptr: loss scaling is off
    uint32_t* found_inf;
    const uint32_t* skipped;
};
AmpState amp_state();

// ---- workspace owned by the library (grow-only, per process) --------------
// Returns a device buffer of at least `bytes`; nullptr on failure.  Slots are independent.
void* workspace(int slot, size_t bytes);
uint64_t workspace_generation();    // bumped whenever a slot is re-allocated (its old pointer dies)
uint32_t num_cus();                    // compute units of the current device (256 when it cannot be asked)
// The workspaces of one kernel family are shared by every stream of the device.  An entry point that is about to use
// them on stream `s` calls this first: if the family's previous user was another stream, `s` is made to wait for
// everything queued on that stream so far (an event recorded there now).  Costs nothing while one stream keeps the
// family to itself.  `family`: 0 = the marcher (chunk log, scan tiles, compaction counters, occupied box).
int workspace_family_enter(int family, hipStream_t s);
// process-wide session state belongs to the first device that used it: != 0 (error set) when another device is current
int single_device_guard(const char* what);
enum { WS_SCAN = 0, WS_COMPACT = 1, WS_FFMLP = 2, WS_GRIDBWD = 3, WS_MARCH = 4, WS_DENSITY = 5, WS_MLP32_DEFER = 6, WS_AABB = 7, WS_AABB_CALL = 8, WS_FFMLP_W = 9, WS_NERF_FRAGS = 10, WS_NERF_PART = 11, WS_MARCH2 = 12, WS_BACKGROUND = 13, WS_SLOTS = 14 };

__host__ __device__ inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// ---- a small job that another kernel's launch carries in a few extra workgroups ------------------------------------
// Gather-and-split: thread t makes values 8t .. 8t+7, value i = src[map[i] >> 16][map[i] & 0xffff] (map 0xffffffff: 0.0f),
// as bf16 hi (round to nearest even) and lo = bf16(value - hi); the 16 bytes of hi go to out + (t / 64) * 512 + (t % 64) * 4
// (in 32-bit words), the 16 bytes of lo 256 words further.  (What csrc/nerf_mlp.hip's operand fragments are: the training
// step's grid forward builds them beside its own work instead of a 5 us launch in front of the MLP forward.)
struct SplitJob {
    const float* src[5];
    const uint32_t* map;
    uint32_t* out;
    uint32_t threads;
};
// grid_valid_rows -- the rows of a budget that are real: with count != nullptr the grid encoder's forward / backward treat
// their B rows as a budget of which only base + min(*count, cap) (cap == 0: *count), rounded up to 32, are real -- the
// convention of enerf_mlp32_valid_rows(_ex), whose kernels sit between the two and skip the same rows.  Results for real
// rows are unchanged; the rest is neither encoded nor binned.  count == nullptr (the extern "C" entry points): all B rows.
struct ValidRows {
    const int32_t* count;      // device-side
    uint32_t base, cap;
};
// gridencoder.hip: enerf_grid_encode_forward with the rows that count and, optionally, a job for its launch to carry.  The
// fp32 D = 3, C = 2 launch carries a job of at most kCarryBlocks * kPtsPerBlock threads; *carried says whether it did.
int grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs, uint32_t B,
                        uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, int calc_grad_inputs, void* dy_dx,
                        uint32_t gridtype, int dtype, int out_layout, float in_add, float in_mul, enerf_stream_t stream,
                        const ValidRows& grid_valid_rows, const SplitJob* job = nullptr, bool* carried = nullptr);
// ... and enerf_grid_encode_backward_ex with the same rows
int grid_encode_backward(const void* grad, const float* inputs, const int32_t* offsets, void* grad_embeddings, uint32_t B,
                         uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, int calc_grad_inputs, const void* dy_dx,
                         void* grad_inputs, uint32_t gridtype, int dtype, int grad_layout, float in_add, float in_mul,
                         uint32_t flags, uint32_t reserve_B, enerf_stream_t stream, const ValidRows& grid_valid_rows);
// mlp32.hip: what an MLP call takes from its caller, where the public calls take the process's settings: the rows that
// count (as above), the arithmetic mode (enerf_mlp32_precision's 0..3) and whether X / Y / dY / dX are 16-bit
struct MlpCall {
    ValidRows rows;
    int mode;
    bool io16;
};
// The weight-gradient partial sums of a backward that launched no reduce, for the backward that follows to reduce with its
// own in one launch (the colour net's, then the sigma net's).  Not `filled` to begin with and after the reduce; `job` is
// storage for mlp32.hip's own ReduceJob, which only that file reads.
struct DeferredReduce {
    bool filled;
    uint64_t job[10];
};
// mlp32.hip: enerf_mlp32_forward_p / _backward_p, enerf_nerf_mlp_available / _forward / _backward with their modifiers as
// arguments; no process setting is read or changed.  Backward, `signal`: the last launch carries the completion signal and
// *signalled becomes the event that carried it (for hipStreamWaitEvent; left alone when no launch did; pass one wherever
// `signal` is set: with a null `signalled` the launch still carries the signal, but nobody can wait on it).  `pair`, empty:
// this call's sums are left in it and no reduce is launched; filled: the reduce launch takes both and empties it.
int mlp32_forward_p(const float* X, const float* const* wseg, uint32_t w0_cols, uint32_t nerf_perm, uint32_t B,
                    uint32_t in_dim, uint32_t out_dim, uint32_t num_hidden, uint32_t activation, uint32_t output_activation,
                    float* fb, float* Y, uint32_t x_layout, uint32_t y_stride, float* y0_exp, const float* sh_dirs,
                    enerf_stream_t stream, const MlpCall& c);
int mlp32_backward_p(const float* dY, const float* X, const float* const* wseg, float* const* dwseg, uint32_t w0_cols,
                     uint32_t nerf_perm, uint32_t overwrite, const float* fb, uint32_t B, uint32_t in_dim, uint32_t out_dim,
                     uint32_t num_hidden, uint32_t activation, float* bb, float* dX, uint32_t x_layout, uint32_t dy_stride,
                     const float* y_sigmoid, uint32_t y_sigmoid_stride, const float* dsigma, const float* h0,
                     uint32_t h0_stride, enerf_stream_t stream, const MlpCall& c, bool signal, hipEvent_t* signalled,
                     DeferredReduce* pair);
bool nerf_mlp_available(int mode);
int nerf_mlp_forward(const float* feats, const float* dirs, const float* const* wseg_s, const float* const* wseg_c,
                     uint32_t w0_cols_c, uint32_t B, uint32_t out_c, float* sigma, float* rgb, uint32_t flags,
                     enerf_stream_t stream, const MlpCall& c);
int nerf_mlp_backward(const float* g_rgb, const float* g_sigma, float sigma_scale, const float* feats, const float* dirs,
                      const float* rgb, const float* const* wseg_s, const float* const* wseg_c, float* const* dwseg_s,
                      float* const* dwseg_c, uint32_t w0_cols_c, uint32_t overwrite, uint32_t B, uint32_t out_c, float* dfeat,
                      uint32_t flags, enerf_stream_t stream, const MlpCall& c, bool signal, hipEvent_t* signalled);
// mlp32.hip: the job that builds the fragments enerf_nerf_mlp_forward / _backward would build for these weights (a launch
// on `s` in front of them carries it) ...
int nerf_mlp_frag_job(const float* const* wseg_s, const float* const* wseg_c, uint32_t w0_cols_c, uint32_t out_c,
                      hipStream_t s, SplitJob* job);
// ... and, once a launch has carried it: the fragments are current for these weights, the calls that follow with flags
// bit 0 use them as they are.  (Not called: nothing is recorded and the next MLP call builds them itself.)
void nerf_mlp_frags_built(const SplitJob& job, uint32_t w0_cols_c, uint32_t out_c);
// Per-workgroup partial sums that the table optimizer's launch reduces on the fly: value i (< n) = sum over b < parts of
// partial[b * stride + i], the gradient of element map[i] & 0xffffff of that launch's small tensor map[i] >> 24
// (0xffffffff: of nobody).  (The fused MLP backward's weight gradients: k_mlp32_reduce_w2 and its 5 us leave the chain.)
struct PartialSums {
    const float* partial;
    const uint32_t* map;
    uint32_t parts, stride, n;
};
// mlp32.hip: the job for the enerf_nerf_mlp_backward call that follows on `s` with flags bit 1 (B rows, same gradient
// segments); small_g / small_n: the optimizer call's small tensors.  0: `job` is set; 1: does not apply (the small tensors
// are not exactly the five gradient matrices, or loss scaling is armed); < 0: error.
int nerf_mlp_partial_job(float* const* dwseg_s, float* const* dwseg_c, uint32_t w0_cols_c, uint32_t out_c,
                         const float* const* small_g, const uint32_t* small_n, uint32_t n_small, uint32_t B, hipStream_t s,
                         PartialSums* job);

// The count pass of the wave-per-ray lattice marcher as data (csrc/march_lattice.h: march_count_block runs it as workgroup
// `bid` of `blocks` workgroups of 256 threads).  In the one-call training step the NEXT batch's count pass rides in the
// table optimizer's launch -- one queue, no second stream, none of the two cross-stream hand-overs (a signal behind the MLP
// backward, an event wait at the head of the next step: ~17 us of idle queue per step) -- and one small launch behind the
// optimizer scans the counts and writes the samples.
struct MarchCountJob {
    const float* rays_o;
    const float* rays_d;
    const uint8_t* grid;
    float bound;
    uint32_t max_steps, N, C, H;
    const float* nears;          // (nf_nears / nf_fars alias them when near / far are computed in the count pass)
    const float* fars;
    int32_t* rays;
    uint32_t perturb;
    void* log;                   // ChunkEntry[N][kLogCap]
    uint32_t* nlog;
    const int* occ_keys;
    const float* nf_aabb;
    float nf_min_near;
    float* nf_nears;
    float* nf_fars;
    uint32_t blocks;
};
// gridencoder.hip: enerf_grid_adam_from_records_ex with what rides in its launch.  `sums` (n != 0) is summed for the small
// tensors' gradients, and stored where the launch would have read them, by the plain form with C = 2 and five small
// tensors; the `n_counts` (<= 2: the event step's two renders) jobs of `counts`, each with blocks != 0 and N != 0, are
// carried in their blocks extra workgroups by the plain C = 2 form.  The owner-range and loss-scaling forms take neither.
// *taken: which of the two the launch took.
enum { ADAM_TOOK_SUMS = 1u, ADAM_TOOK_COUNTS = 2u };
int grid_adam_from_records(float* p, float* g, float* m, float* v, const int32_t* offsets, uint32_t L, uint32_t C, float lr,
                           float beta1, float beta2, float eps, uint32_t step, uint32_t n_small, float* const* sp,
                           const float* const* sg, float* const* sm, float* const* sv, const uint32_t* sn, const float* slr,
                           const uint32_t* sstep, enerf_stream_t stream, const PartialSums* sums, const MarchCountJob* counts,
                           uint32_t n_counts, uint32_t* taken);
// raymarching.hip: what is left of a march whose count pass another launch carries -- its scan + write (march_carry_end)
struct CarriedMarch {
    const float *rays_o, *rays_d, *nears, *fars;
    const uint8_t* grid;
    float bound;
    uint32_t max_steps, N, C, H, M, perturb, zero_unwritten;
    float *xyzs, *dirs, *deltas;
    int32_t *rays, *counter;
    const void* log;             // ChunkEntry[N][kLogCap]
    const uint32_t* nlog;
};
// raymarching.hip: march_rays_train_ex(...) split around a carrying launch, near / far computed inside the count pass from
// nf_aabb / nf_min_near (enerf_march_fuse_near_far's arguments).  begin: 0 = *job is the call's count pass (the workspace
// is prepared) and *march its scan + write; 1 = this call cannot be served that way (another marcher, a kept counter ...):
// make the ordinary call; < 0 = error.  The carried form stores no count mirror: whether one is wanted is the caller's
// knowledge, who then makes the ordinary call.  end: scan + write of the n marches on `s` (behind the launch that carried
// the jobs), in order.  Two marches may be pending at a time, each with a chunk log of its own: `ws_slot` is WS_MARCH or
// WS_MARCH2.  `share`: how many marches will ride in the launch (splits the workgroups).
int march_carry_begin(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma,
                      uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float* nears,
                      const float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays, int32_t* counter,
                      uint32_t perturb, uint32_t flags, const float* nf_aabb, float nf_min_near, hipStream_t s, int ws_slot,
                      MarchCountJob* job, CarriedMarch* march, uint32_t share = 1);
int march_carry_end(const CarriedMarch* marches, uint32_t n, hipStream_t s);
int march_carry_count_now(const MarchCountJob* job, hipStream_t s);     // (the carrying launch did not take the job)
// raymarching.hip: enerf_march_rays_train_ex with the near / far request and the count mirror (enerf_march_mirror_count's
// host pointer, or nullptr) as arguments: the process's one-shot requests are neither read nor cleared
int march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma,
                     uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float* nears,
                     const float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays, int32_t* counter,
                     uint32_t perturb, uint32_t zero_unwritten, const float* nf_aabb, float nf_min_near, int32_t* count_host,
                     enerf_stream_t stream);

// ---- wave-level primitives (wave64) ----------------------------------------
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// Inclusive scans of a wavefront with DPP lane exchanges (no LDS crossbar, no per-step select): Hillis-Steele steps
// 1, 2, 4, 8 inside each 16-lane row (row_shr; a lane without a source keeps the operation's identity), then the row
// totals: lane 15 of rows 0 / 2 into rows 1 / 3 (row_bcast15, row mask 0xA), lane 31 into rows 2 and 3 (row_bcast31,
// row mask 0xC).  All 64 lanes must be active.
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ int dpp_take(int identity, int v) {
    return __builtin_amdgcn_update_dpp(identity, v, CTRL, ROWS, 0xf, false);
}
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ float dpp_take(float identity, float v) {
    return __int_as_float(dpp_take<CTRL, ROWS>(__float_as_int(identity), __float_as_int(v)));
}
__device__ __forceinline__ float wave_incl_scan_add(float v, int) {
    v += dpp_take<0x111>(0.0f, v);
    v += dpp_take<0x112>(0.0f, v);
    v += dpp_take<0x114>(0.0f, v);
    v += dpp_take<0x118>(0.0f, v);
    v += dpp_take<0x142, 0xa>(0.0f, v);
    v += dpp_take<0x143, 0xc>(0.0f, v);
    return v;
}
__device__ __forceinline__ float wave_incl_scan_mul(float v, int) {
    v *= dpp_take<0x111>(1.0f, v);
    v *= dpp_take<0x112>(1.0f, v);
    v *= dpp_take<0x114>(1.0f, v);
    v *= dpp_take<0x118>(1.0f, v);
    v *= dpp_take<0x142, 0xa>(1.0f, v);
    v *= dpp_take<0x143, 0xc>(1.0f, v);
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan_add_u32(uint32_t x, int) {
    int v = (int)x;
    v += dpp_take<0x111>(0, v);
    v += dpp_take<0x112>(0, v);
    v += dpp_take<0x114>(0, v);
    v += dpp_take<0x118>(0, v);
    v += dpp_take<0x142, 0xa>(0, v);
    v += dpp_take<0x143, 0xc>(0, v);
    return (uint32_t)v;
}
// value of the lane below (wave_shr:1); lane 0 gets `first`
__device__ __forceinline__ float wave_prev(float v, float first) { return dpp_take<0x138>(first, v); }
// a lane's value in every lane (v_readlane: `src` is wave-uniform)
__device__ __forceinline__ float wave_bcast(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

}  // namespace enerf
