/*
 * enerf_hip.h -- C ABI of libenerf_hip.so, the MI355X (gfx950) implementation of the
 * instant-ngp hot path that knelk/enerf sits on.
 *
 * This is the drop-in boundary.  The reference binds its native code through four
 * pybind11 modules (`_raymarching`, `_gridencoder`, `_shencoder`, `_ffmlp`) whose
 * functions take at::Tensor arguments that the *caller* has already allocated
 * (and zero-filled where the kernels only partially write).  Each entry point below
 * replaces exactly one of those bound functions; the argument order is the
 * reference's, with every tensor flattened to a raw device pointer, followed by
 *   - explicit dtype selectors where the reference dispatches on tensor dtype,
 *   - `stream`: the hipStream_t to launch on (the reference uses the legacy default
 *     stream; pass torch's current stream).
 * All pointers are DEVICE pointers unless marked [host].  All functions are
 * asynchronous, allocate nothing the caller can see, and return 0 on success or a
 * negative ENERF_E_* / positive hipError_t code; enerf_last_error() describes the
 * failure (the reference throws c10::Error / std::runtime_error at the same places).
 * enerf_amd/backends/_*.py are the ctypes shims that re-create the reference's
 * pybind signatures on top of this ABI.
 *
 * Reference interfaces replaced (paths relative to the knelk/enerf tree):
 *   raymarching/src/raymarching.h:7-19, raymarching/src/bindings.cpp:5-20
 *   gridencoder/src/gridencoder.h:12-13, gridencoder/src/bindings.cpp:5-8
 *   shencoder/src/shencoder.h:9,12,     shencoder/src/bindings.cpp:5-8
 *   ffmlp/src/ffmlp.h:8-14,             ffmlp/src/bindings.cpp:5-11
 */
#ifndef ENERF_HIP_H
#define ENERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* enerf_stream_t; /* hipStream_t */

/* error codes (negative; positive values are hipError_t) */
#define ENERF_OK 0
#define ENERF_E_BADARG (-1)      /* unsupported D / C / degree / width / dtype ...           */
#define ENERF_E_NOMEM (-2)       /* internal workspace allocation failed                      */
#define ENERF_E_UNSUPPORTED (-3) /* feature the reference asserts off as well                 */

/* element types for entry points that the reference dispatches on tensor dtype */
#define ENERF_F32 0
#define ENERF_F16 1
#define ENERF_BF16 2

const char* enerf_last_error(void);
/* ABI version of this header; bumped on any signature change.  This #define is the ONE place the number lives:
 * the library returns it (csrc/runtime.hip), enerf_amd/_lib.py parses it and refuses a library that answers differently,
 * __graft_entry__.build() and tests/test_abi.py compare against the parsed value.
 * 2: enerf_train_step_args lost its RCCL-tail fields, enerf_dp_* retired, enerf_nerf_mlp_* added.
 * 3: enerf_stratified_* added (the stratified sampler of NeRFRenderer.run).
 * 4: enerf_stratified_*_ex (fp16 storage of the colour rows / rgb / d rgb / dx) and enerf_mlp32_io16 (16-bit I/O of the
 *    enerf_mlp32_*_p calls) added: the stratified sampler's fp16 regime.
 * 5: enerf_mesh_lattice and enerf_marching_cubes_* added (mesh export, Trainer.save_mesh).
 * 6: enerf_eval_* added (held-out metrics, Trainer.evaluate_one_epoch).
 * 7: enerf_train_step_args gained next_count_host; `reserved` of both step structs became `report`, written by the library
 *    (the argument pointers lost their const); flags bit 2 of both = every row through the networks.
 * 8: enerf_frame_batch and enerf_error_map_* added (frame batches, the reference's --error_map).
 * 9: enerf_debug_nerf_bwd_transpose added (how the fused MLP backward transposes its weight-gradient operands).
 * 10: enerf_event_single_pair_rays and enerf_no_event_rays added (the event side of collate with accumulate_evs off, and
 *     the rays of --negative_event_sampling).
 * 11: enerf_ema_update_multi added (the parameters' exponential moving average, Trainer's ema_decay).
 * 12: enerf_view_finish and enerf_view_minmax added (a rendered frame to display bytes: Trainer.test / test_gui, the GUI's
 *     running mean, scripts/render.py's min-max scaling).
 * 13: the _c forms of the compositing entry points and of enerf_event_loss_fwd_bwd added (1..3 colour channels on the
 *     marching route); both one-call steps honour out_c in their compositing and loss (target / g_image [N,out_c]).
 *     Still 13: enerf_debug_sigma_head added (a testing aid: the density-only head's load pipeline against the form shipped
 *     before) -- no signature changed, and tests/test_composite_channels_host.py holds the header at 13.
 *     Still 13: enerf_no_event_loss_fwd_bwd_c added, and enerf_event_loss_fwd_bwd_c serves C_thres == -1 (the normalised
 *     loss) where it answered ENERF_E_BADARG -- nothing existing changed meaning or layout.
 *     Still 13: enerf_composite_rays_train_fwd_bwd_frames_c added (the frame term's compositing) -- a new
 *     symbol beside the old ones; two test files hold the header at 13.
 *     Still 13: enerf_event_c_estimate added (the implicit contrast threshold's four medians) -- a new
 *     symbol, nothing existing changed.
 *     Still 13: enerf_event_tables_workspace / _count / _fill and enerf_no_event_coords added (a raw event stream to the
 *     pair kernels' tables) -- new symbols, nothing existing changed.
 *     Still 13: enerf_background_forward / _backward added (the background model in one launch each way, DESIGN.md
 *     4.21) -- new symbols, nothing existing changed.
 *     Still 13: enerf_debug_event_segment_sort added (a testing aid: the segment sorts of enerf_event_tables_fill on
 *     segments of the caller's choice) -- a new symbol, nothing existing changed.
 *     Still 13: enerf_event_pixel_stats, enerf_event_accumulation_image, enerf_event_count_moments, enerf_event_hot_mask
 *     and enerf_event_stream_compact_workspace / _compact added (pixel counts, accumulation images, hot pixels and the
 *     stream without them) -- new symbols, nothing existing changed. */
#define ENERF_ABI_VERSION 13
int enerf_abi_version(void);
/* The library keeps grow-only scratch buffers per device (march chunk log, grid-backward record lists, ...).  Growing one
 * frees the old allocation; the counter returned here moves every time that happens.  A caller that captured library
 * launches into a HIP graph must re-capture when the counter has moved since the capture (the graph holds the old
 * pointers). */
uint64_t enerf_workspace_generation(void);

/* ------------------------------------------------------------------ raymarching
 * raymarching/src/raymarching.cu; all float tensors are fp32 (the wrappers
 * custom_fwd(cast_inputs=torch.float32), raymarching/raymarching.py:21,54,131,163). */

/* raymarching.cu:150-158  near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars) */
int enerf_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N,
                             float min_near, float* nears, float* fars, enerf_stream_t stream);

/* raymarching.cu:203-211  polar_from_ray(rays_o, rays_d, radius, N, coords) */
int enerf_polar_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords,
                         enerf_stream_t stream);

/* raymarching.cu:231-234  morton3D(coords, N, indices) */
int enerf_morton3D(const int32_t* coords, uint32_t N, int32_t* indices, enerf_stream_t stream);

/* raymarching.cu:259-262  morton3D_invert(indices, N, coords) */
int enerf_morton3D_invert(const int32_t* indices, uint32_t N, int32_t* coords, enerf_stream_t stream);

/* raymarching.cu:294-302  packbits(grid, N, density_thresh, bitfield); N = number of output bytes */
int enerf_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield, enerf_stream_t stream);

/* ---- density-grid maintenance: the device side of NeRFRenderer.update_extra_state (nerf/renderer.py:472-560) --------
 * The reference builds the candidate cells and applies the results with ~40 torch ops per cascade and three host
 * synchronisations; these two entry points are that logic around the density network evaluation, which stays with the
 * caller (hash grid + sigma MLP on `xyzs`, giving `sigmas`).  H must be a power of two (the Morton layout), 1 <= C <= 8.
 *
 * enerf_density_grid_cells: Morton indices (int32, per cascade) and jittered query positions [P,3] of the cells to evaluate,
 * cascades concatenated.
 *   density_grid == NULL : full sweep (renderer.py:484-512), P = C * H^3, cells in x-fastest order.
 *   density_grid != NULL : partial update (renderer.py:514-538), P = C * 2 * n_uniform: per cascade n_uniform uniformly
 *                          drawn cells and n_uniform draws with replacement from the cells with density > 0 (all uniform
 *                          when none is), emitted sorted by Morton index.
 * Positions: (2 * coord / (H - 1) - 1) * (bound_c - half) + U(-half, half), bound_c = min(2^cas, bound), half =
 * bound_c / H.  Random numbers come from a counter-based generator keyed by `seed` (same distribution as the reference's
 * torch.randint / rand_like calls, not the same stream). */
int enerf_density_grid_cells(const float* density_grid, uint32_t C, uint32_t H, float bound, uint32_t n_uniform,
                             uint64_t seed, int32_t* indices, float* xyzs, enerf_stream_t stream);

/* enerf_mark_untrained_grid (renderer.py:408-469): density_grid[cas, cell] = -1 for every cell whose centre no camera
 * sees: cam = R^T (centre - t) for each c2w pose ([B,4,4] row-major fp32, pose_stride 16, or [B,3,4], 12); seen when
 * cam.z > 0 and |cam.x| < cx/fx * cam.z + 2*half_cell and |cam.y| < cy/fy * cam.z + 2*half_cell. */
int enerf_mark_untrained_grid(const float* poses, uint32_t n_poses, uint32_t pose_stride, float fx, float fy, float cx,
                              float cy, uint32_t C, uint32_t H, float bound, float* density_grid,
                              enerf_stream_t stream);

/* enerf_density_grid_update (renderer.py:541-558): tmp_grid = -1; tmp_grid[cas, indices] = sigmas * sigma_scale (n_per_cascade
 * entries per cascade); where density_grid >= 0 and tmp_grid >= 0: density_grid = max(density_grid * decay, tmp_grid);
 * mean = mean(clamp(density_grid, 0)); bitfield = packbits(density_grid, min(mean, density_thresh)).
 * stats (device, 2 doubles) receives {mean, sum of step_counter[0:total_step][0]} -- the one read-back of the update
 * (mean_density, mean_count).  step_counter: int32 [16,2] (may be NULL when total_step == 0). */
int enerf_density_grid_update(const int32_t* indices /* NULL: the full sweep's own order */, const float* sigmas, uint32_t n_per_cascade, uint32_t C, uint32_t H,
                              float sigma_scale, float decay, float density_thresh, float* density_grid,
                              uint8_t* bitfield, const int32_t* step_counter, uint32_t total_step, double* stats,
                              enerf_stream_t stream);

/* raymarching.cu:482-490  march_rays_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M,
 *                                          nears, fars, xyzs, dirs, deltas, rays, counter, perturb)
 * xyzs/dirs/deltas must be zero-filled by the caller (raymarching.py:205-207).
 * Slot allocation is deterministic here: rays[n] = (n, counter[0]@entry + exclusive_scan(num_steps)[n],
 * num_steps[n]); counter[0] += sum(num_steps); counter[1] += N.  (The reference's atomics give the same
 * multiset in hardware order.) */
int enerf_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound,
                           float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                           const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                           int32_t* rays, int32_t* counter, uint32_t perturb, enerf_stream_t stream);

/* Extension of march_rays_train for callers that hand over UNINITIALISED sample buffers (zero_unwritten != 0): every
 * row no ray writes -- past the last reservation, and a dropped ray's reservation clipped to M -- is zero-filled by the
 * write pass itself, so the three torch.zeros of raymarching.py:205-207 become torch.empty.  zero_unwritten == 0 is
 * exactly enerf_march_rays_train.  `zero_unwritten` is a flag word: bit 0 as above; bit 1 says the batch is being
 * prepared ahead of its step on a side stream: the count pass then runs with one wavefront per SIMD (rays in turn) so
 * that it leaves the registers of the chip to the step it runs beside; bit 2: test rays against the occupied cells'
 * bounding box first (enerf_occupied_box_update); bit 3 (value 8): `counter` is taken as (0, 0) whatever it holds --
 * the wrapper's counter.zero_() (raymarching.py:198) without its launch.  Same rows, same counts, bit for bit. */
int enerf_march_rays_train_ex(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound,
                              float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                              const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                              int32_t* rays, int32_t* counter, uint32_t perturb, uint32_t zero_unwritten,
                              enerf_stream_t stream);

/* Arms the NEXT enerf_march_rays_train(_ex / _count) call: the two words of `counter` it leaves on the device -- samples
 * reserved, rays marched -- are also written to host_counter[0], [1] (pinned, device-visible host memory, e.g. a torch
 * tensor with pin_memory=True), word 1 last: a host that pre-set both to -1 and watches them has the count without
 * queueing a copy (and an event) behind the march.  Batches above 16 384 rays get the copy. */
int enerf_march_mirror_count(int32_t* host_counter);

/* Arms the NEXT enerf_march_rays_train(_ex / _count) call: its count pass computes near / far of every ray against `aabb`
 * itself (enerf_near_far_from_aabb's arithmetic, bit for bit) and WRITES them to the nears / fars arrays the call is
 * given (they need not be initialised) -- the near_far launch at the head of a march that is prepared ahead of its step
 * disappears.  Marchers that do not take the wave-per-ray route run the near_far kernel first, on the call's stream.
 * `aabb` is read by that march's kernels, not here: it must stay valid until they have run. */
int enerf_march_fuse_near_far(const float* aabb, float min_near);

/* Bounding box of the occupied cells of a density bitfield, kept by the library for the fixed-step training marcher.
 * A sample can only be emitted inside an occupied cell's box, so a ray that misses the union's bounding box emits
 * nothing and a ray emits nothing after leaving it: with flag bit 2 (value 4) of enerf_march_rays_train_ex /
 * enerf_march_rays_train_count the count pass tests every ray against the box first and marches only to the box's far
 * side -- identical rays / counter / samples (tests), half of the synthetic scene's rays settled without marching.
 * The caller sets the flag only while the box computed here is current for `grid`: call this again (same stream
 * order as the marches that follow) whenever the bitfield's contents change.  The flag is ignored when the box was
 * computed for another pointer / C / H / bound. */
int enerf_occupied_box_update(const uint8_t* grid, uint32_t C, uint32_t H, float bound, enerf_stream_t stream);

/* The two halves of enerf_march_rays_train_ex, for callers that size the sample buffers from the count instead of the
 * reference's worst case (raymarching.py:195-228: while no sample budget exists the wrapper allocates and zero-fills
 * M = N * max_steps rows -- 134 MB at 4096 rays -- marches, reads counter[0] back and crops to that count rounded up to
 * `align`).  The count pass already knows the total on the device:
 *   _count: near/far -> per-ray sample counts -> deterministic scan: rays[n] = (n, offset, count), counter[0] += sum,
 *           counter[1] += N.  Nothing is written to sample buffers.  flags bit 1 = background launch (see _ex),
 *           bit 2 = use the occupied box (enerf_occupied_box_update), bit 3 = counter starts from (0, 0).
 *   _write: the write pass of the SAME batch (same rays / nears / fars / grid / perturb; the fixed-step marcher keeps a
 *           per-process chunk log between the two calls, so no other training march may run in between) into buffers of
 *           M rows; `M` is also the M of the reference's drop rule (`offset + count >= M`: the ray writes nothing).
 *           zero_unwritten bit 0 as in _ex.
 * _count followed by _write with the same M is exactly enerf_march_rays_train_ex. */
int enerf_march_rays_train_count(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound,
                                 float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
                                 const float* nears, const float* fars, int32_t* rays, int32_t* counter,
                                 uint32_t perturb, uint32_t flags, enerf_stream_t stream);
int enerf_march_rays_train_write(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound,
                                 float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                                 const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                                 const int32_t* rays, const int32_t* counter, uint32_t perturb,
                                 uint32_t zero_unwritten, enerf_stream_t stream);

/* raymarching.cu:581-589  composite_rays_train_forward(sigmas, rgbs, deltas, rays, M, N, weights_sum, depth, image) */
int enerf_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas,
                                       const int32_t* rays, uint32_t M, uint32_t N, float* weights_sum,
                                       float* depth, float* image, enerf_stream_t stream);

/* raymarching.cu:685-693  composite_rays_train_backward(grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays,
 *                                                       weights_sum, image, M, N, grad_sigmas, grad_rgbs)
 * grad_sigmas / grad_rgbs must be zero-filled by the caller (raymarching.py:277-278). */
int enerf_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                        const float* rgbs, const float* deltas, const int32_t* rays,
                                        const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                        float* grad_sigmas, float* grad_rgbs, enerf_stream_t stream);

/* composite_rays_train_forward + the background blend that follows it in the renderer (nerf/renderer.py:352
 * `image = image + (1 - weights_sum).unsqueeze(-1) * bg_color`), one launch: out_image[N,3] receives the blend, `image`
 * still receives the unblended colour (the backward needs it).  bg_color: NULL -> the scalar bg_scalar; else [3]
 * (bg_stride 0) or [N,3] (bg_stride 3).  depth may be NULL (a training step that does not use it). */
int enerf_composite_rays_train_forward_blend(const float* sigmas, const float* rgbs, const float* deltas,
                                             const int32_t* rays, uint32_t M, uint32_t N, float* weights_sum,
                                             float* depth, float* image, const float* bg_color, uint32_t bg_stride,
                                             float bg_scalar, float* out_image, enerf_stream_t stream);

/* composite_rays_train_backward for loss = mean((out_image - target)^2) * upstream (nerf/utils.py:628 with the default
 * MSE criterion): grad_image = (out_image - target) * grad_scale with grad_scale = 2 / (3 N) * upstream, and
 * grad_weights_sum = -(grad_image . bg), both formed in the kernel.  grad_sigmas / grad_rgbs may be UNINITIALISED: rows no
 * ray covers are zero-filled here (counter = the march's counter, counter[0] = samples reserved).
 * target == NULL: `out_image` is taken to hold d loss / d out_image of some other loss (times grad_scale), everything
 * else as above -- the general backward of "composite + background blend" into uninitialised buffers.
 * loss (optional, device scalar): mean((out_image - target)^2) is ADDED to it (one float atomic per workgroup, so the
 * value is reproducible to rounding only) -- the caller zeroes it; the gradients do not depend on it. */
int enerf_composite_rays_train_backward_mse(const float* out_image, const float* target, float grad_scale,
                                            const float* bg_color, uint32_t bg_stride, float bg_scalar,
                                            const int32_t* counter, const float* sigmas, const float* rgbs,
                                            const float* deltas, const int32_t* rays, const float* weights_sum,
                                            const float* image, uint32_t M, uint32_t N, float* grad_sigmas,
                                            float* grad_rgbs, float* loss, enerf_stream_t stream);

/* composite_rays_train forward (+ blend) and its MSE backward in ONE launch, for steps whose loss is
 * mean((out_image - target)^2) * upstream (the reference's default criterion, nerf/utils.py:628): equals
 * enerf_composite_rays_train_forward_blend (depth not computed) followed by
 * enerf_composite_rays_train_backward_mse(out_image, target, ...), bit for bit; weights_sum / image / out_image are
 * still written. */
int enerf_composite_rays_train_fwd_bwd_mse(const float* sigmas, const float* rgbs, const float* deltas,
                                           const int32_t* rays, uint32_t M, uint32_t N, float* weights_sum,
                                           float* image, const float* bg_color, uint32_t bg_stride, float bg_scalar,
                                           float* out_image, const float* target, float grad_scale,
                                           const int32_t* counter, float* grad_sigmas, float* grad_rgbs, float* loss,
                                           enerf_stream_t stream);

/* The five calls above for `channels` = 1, 2 or 3 colour channels (the colour net's output width; the reference's marching
 * route is three-channel by construction): rgbs / grad_rgbs [M,channels], image / out_image / grad_image / target
 * [N,channels], bg_color [channels] (bg_stride 0) or [N,channels] (bg_stride = channels); the MSE forms use
 * grad_scale = 2 / (channels N) * upstream and report mean over N * channels values.  Everything else as documented above;
 * the calls above are these with channels = 3.  channels outside 1..3: ENERF_E_BADARG. */
int enerf_composite_rays_train_forward_c(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                         uint32_t M, uint32_t N, float* weights_sum, float* depth, float* image,
                                         uint32_t channels, enerf_stream_t stream);
int enerf_composite_rays_train_forward_blend_c(const float* sigmas, const float* rgbs, const float* deltas,
                                               const int32_t* rays, uint32_t M, uint32_t N, float* weights_sum,
                                               float* depth, float* image, const float* bg_color, uint32_t bg_stride,
                                               float bg_scalar, float* out_image, uint32_t channels,
                                               enerf_stream_t stream);
int enerf_composite_rays_train_backward_c(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                          const float* rgbs, const float* deltas, const int32_t* rays,
                                          const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                          float* grad_sigmas, float* grad_rgbs, uint32_t channels, enerf_stream_t stream);
int enerf_composite_rays_train_backward_mse_c(const float* out_image, const float* target, float grad_scale,
                                              const float* bg_color, uint32_t bg_stride, float bg_scalar,
                                              const int32_t* counter, const float* sigmas, const float* rgbs,
                                              const float* deltas, const int32_t* rays, const float* weights_sum,
                                              const float* image, uint32_t M, uint32_t N, float* grad_sigmas,
                                              float* grad_rgbs, float* loss, uint32_t channels, enerf_stream_t stream);
int enerf_composite_rays_train_fwd_bwd_mse_c(const float* sigmas, const float* rgbs, const float* deltas,
                                             const int32_t* rays, uint32_t M, uint32_t N, float* weights_sum,
                                             float* image, const float* bg_color, uint32_t bg_stride, float bg_scalar,
                                             float* out_image, const float* target, float grad_scale,
                                             const int32_t* counter, float* grad_sigmas, float* grad_rgbs, float* loss,
                                             uint32_t channels, enerf_stream_t stream);

/* enerf_composite_rays_train_fwd_bwd_mse_c with a FRAME tail in place of the finished target: the frame term of
 * Trainer.train_step (nerf/utils.py:595-604,634) and of train_step_events with event_only = 0 (:546), formed in the
 * launch.  Per ray (indexed by the ray id rays[n][0], as everything here):
 *   gt       = pixels[ray]                                    (pix_stride == channels), or
 *              fl(fl(p a) + fl(bg fl(1 - a))), a = pixels[ray][channels]   (pix_stride == channels + 1: alpha images,
 *              mixed on THIS call's background at that ray -- bit for bit torch's images[..., :C] * a + bg * (1 - a));
 *   err      = sum_c (out_image - gt)^2 / channels            for every ray: marched, missed or dropped;
 *   loss    += weight * sum_rays err / N                      (one float atomic per workgroup; the caller zeroes it);
 *   g_image  = 2 / (channels N) * (out_image - gt)            (times the loss scale between enerf_amp_begin / _end),
 * and from g_image on everything is the MSE form's: weights_sum / image / out_image written, grad_sigmas / grad_rgbs may
 * be UNINITIALISED -- with `weight` multiplied into the finished grad_sigmas / grad_rgbs, one rounding each (d sigma is a
 * sum that cancels: a weight folded into g_image sends its rounding through that sum, 67 ulp at weight 0.3; this way a
 * weighted call's gradients are fl(weight * the unweighted call's)).  With pix_stride == channels and weight == 1 the
 * images and gradients equal those of
 * enerf_composite_rays_train_fwd_bwd_mse_c(target = pixels, grad_scale = 2 / (channels N)) bit for bit.
 * gt_out [N,channels], err_out [N], loss: optional.  pix_stride outside {channels, channels + 1}, or counter / pixels /
 * weights_sum / image / out_image == NULL: ENERF_E_BADARG.  N == 0: the gradients are zero-filled, nothing else. */
int enerf_composite_rays_train_fwd_bwd_frames_c(const float* sigmas, const float* rgbs, const float* deltas,
                                                const int32_t* rays, uint32_t M, uint32_t N, float* weights_sum,
                                                float* image, const float* bg_color, uint32_t bg_stride,
                                                float bg_scalar, float* out_image, const float* pixels,
                                                uint32_t pix_stride, float weight, float* gt_out, float* err_out,
                                                const int32_t* counter, float* grad_sigmas, float* grad_rgbs,
                                                float* loss, uint32_t channels, enerf_stream_t stream);

/* raymarching.cu:807-813  march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma,
 *                                    max_steps, C, H, grid, nears, fars, xyzs, dirs, deltas, perturb) */
int enerf_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                     const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                     uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars,
                     float* xyzs, float* dirs, float* deltas, uint32_t perturb, enerf_stream_t stream);

/* Extension of march_rays for UNINITIALISED xyzs / dirs / deltas of `zero_rows_to` rows (>= n_alive * n_step; 0 =
 * plain enerf_march_rays): every slot a ray does not fill and the alignment rows past the last ray are zero-filled by
 * the march itself (delta == 0 is what ends a ray in composite_rays), so the three torch.zeros of
 * raymarching.py:318-320 become torch.empty. */
int enerf_march_rays_ex(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                        const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                        uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars,
                        float* xyzs, float* dirs, float* deltas, uint32_t perturb, uint32_t zero_rows_to,
                        enerf_stream_t stream);

/* raymarching.cu:903-909  composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas,
 *                                        weights_sum, depth, image)   -- in place */
int enerf_composite_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, float* rays_t,
                         const float* sigmas, const float* rgbs, const float* deltas, float* weights_sum,
                         float* depth, float* image, enerf_stream_t stream);

/* Whole-frame inference compositing -- the reference's inference loop (nerf/renderer.py:364-401: per round
 * compact_rays -> alive_counter.item() -> march_rays(n_step) -> network -> composite_rays) needs the rounds only because
 * it marches a fixed n_step slots per alive ray.  With every ray's samples marched contiguously up front
 * (enerf_march_rays_train_count / _write: rays = (id, offset, count); same cells, same lattice of t, perturb = 0) one
 * pass composites a ray exactly as the rounds do: the arithmetic and order of composite_rays (raymarching.cu:817-909:
 * T = 1 - weights_sum, termination once a sample's pre-sample T < 1e-5 -- that sample is still accumulated), starting
 * from t = nears[id], then image += (1 - weights_sum) * bg and depth = clamp(depth - near, 0) / (far - near).  The image
 * equals the iterated schedule's bit for bit whenever no ray reaches the loop's 1024-step cap.  bg: scalar (bg_color NULL),
 * one RGB (stride 0) or one per ray (stride 3).  used_samples (device u32, may be NULL) += samples accumulated. */
int enerf_composite_rays_frame(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                               uint32_t N, uint32_t M, const float* nears, const float* fars, const float* bg_color,
                               uint32_t bg_stride, float bg_scalar, float* weights_sum, float* depth, float* image,
                               uint32_t* used_samples, enerf_stream_t stream);

/* enerf_composite_rays / enerf_composite_rays_frame for `channels` = 1, 2 or 3 colour channels: rgbs [.., channels],
 * image [N,channels], bg as in the training forms (one colour of `channels` values, or one per ray with
 * bg_stride = channels).  channels outside 1..3: ENERF_E_BADARG. */
int enerf_composite_rays_c(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, float* rays_t,
                           const float* sigmas, const float* rgbs, const float* deltas, float* weights_sum,
                           float* depth, float* image, uint32_t channels, enerf_stream_t stream);
int enerf_composite_rays_frame_c(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                 uint32_t N, uint32_t M, const float* nears, const float* fars, const float* bg_color,
                                 uint32_t bg_stride, float bg_scalar, float* weights_sum, float* depth, float* image,
                                 uint32_t* used_samples, uint32_t channels, enerf_stream_t stream);

/* raymarching.cu:933-939  compact_rays(n_alive, rays_alive, rays_alive_old, rays_t, rays_t_old, alive_counter)
 * Order-preserving (stable) here; alive_counter[0] += number of survivors. */
int enerf_compact_rays(uint32_t n_alive, int32_t* rays_alive, const int32_t* rays_alive_old, float* rays_t,
                       const float* rays_t_old, int32_t* alive_counter, enerf_stream_t stream);

/* ------------------------------------------------------------------ gridencoder
 * gridencoder/src/gridencoder.cu:416-471.  `inputs` is always fp32 (gridencoder.cu:437);
 * embeddings / outputs / dy_dx / grad share `dtype` (ENERF_F32 or ENERF_F16).
 * out_layout 0 = the reference's [L,B,C]; 1 = [B,L*C] written directly (saves the permute copy of
 * gridencoder/grid.py:52,70 -- used by enerf_amd's own wrapper, not by the reference's); 2 = [L,Bp,C] with
 * Bp = B rounded up to a multiple of 32 and the pad rows zero-filled (the level-major input of enerf_mlp32_*).
 * in_add / in_mul: the kernels read every input coordinate as (x + in_add) * in_mul -- (0, 1) for inputs already in
 * [0,1] as the reference passes them, (bound, 1/(2*bound)) to fold the wrapper's normalisation (grid.py:150) in.
 * NOTE with a non-identity transform dy_dx / grad_inputs are with respect to the transformed coordinates. */

/* grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H, calc_grad_inputs, dy_dx, gridtype) */
int enerf_grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                              uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                              int calc_grad_inputs, void* dy_dx, uint32_t gridtype, int dtype, int out_layout,
                              float in_add, float in_mul, enerf_stream_t stream);

/* grid_encode_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, calc_grad_inputs,
 *                      dy_dx, grad_inputs, gridtype); grad_embeddings must be zero-filled (grid.py:72);
 * grad_layout as out_layout above. */
int enerf_grid_encode_backward(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                               void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                               uint32_t H, int calc_grad_inputs, const void* dy_dx, void* grad_inputs,
                               uint32_t gridtype, int dtype, int grad_layout, float in_add, float in_mul,
                               enerf_stream_t stream);

/* grid_encode_forward over the query points of a full density-grid sweep (NeRFRenderer.update_extra_state,
 * nerf/renderer.py:484-512: one uniformly drawn point inside every cell of every cascade, x fastest) WITHOUT an input
 * array: point b = (cascade b / grid_size^3, cell b % grid_size^3) is generated inside the kernel from `seed` -- the
 * same points, bit for bit, as enerf_density_grid_cells(density_grid = NULL, ..., seed) writes out (csrc/sweep_points.h).
 * fp32 tables, D = 3; outputs as enerf_grid_encode_forward with B = n_cascades * grid_size^3. */
int enerf_grid_encode_forward_sweep(const void* embeddings, const int32_t* offsets, void* outputs, uint32_t n_cascades,
                                    uint32_t grid_size, float bound, uint64_t seed, uint32_t C, uint32_t L, float S,
                                    uint32_t H, uint32_t gridtype, int out_layout, float in_add, float in_mul,
                                    enerf_stream_t stream);

/* Deferred flush: the table gradient's only consumer in training is the optimizer (main_nerf.py:211, Adam), which streams
 * over the whole table anyway.  With flags bit 0 set, enerf_grid_encode_backward_ex leaves the binned levels' record
 * lists pending instead of summing them into `grad_embeddings` (levels too small to bin, and batches below the binning
 * threshold, still add into it); further calls with the flag append to the same lists (`reserve_B`: samples of ALL calls
 * of the session, which sizes the lists; 0 = this call's B).  enerf_grid_adam_from_records then visits every 128-KiB
 * tile of the table once: sums the tile's records in LDS (fp64), adds the dense gradient where one was written (and
 * clears it), and applies torch.optim.Adam's update (no weight decay / amsgrad; `step` counts from 1) to the tile's
 * rows of p, m, v.  With nothing pending it is a plain fused Adam over the dense gradient.  Until it runs, only calls
 * that join the session are accepted.  flags == 0 is exactly enerf_grid_encode_backward. */
int enerf_grid_encode_backward_ex(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                  void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                  uint32_t H, int calc_grad_inputs, const void* dy_dx, void* grad_inputs,
                                  uint32_t gridtype, int dtype, int grad_layout, float in_add, float in_mul,
                                  uint32_t flags, uint32_t reserve_B, enerf_stream_t stream);
int enerf_grid_adam_from_records(float* p, float* g, float* m, float* v, const int32_t* offsets, uint32_t L, uint32_t C,
                                 float lr, float beta1, float beta2, float eps, uint32_t step, enerf_stream_t stream);
/* The same with up to 8 further (small, dense-gradient) fp32 parameters updated in the same launch -- the model's MLP
 * weights: arrays of n_small device pointers / element counts / learning rates / step counts (host memory); their
 * gradients are read, not cleared. */
int enerf_grid_adam_from_records_ex(float* p, float* g, float* m, float* v, const int32_t* offsets, uint32_t L, uint32_t C,
                                    float lr, float beta1, float beta2, float eps, uint32_t step, uint32_t n_small,
                                    float* const* sp, const float* const* sg, float* const* sm, float* const* sv,
                                    const uint32_t* sn, const float* slr, const uint32_t* sstep, enerf_stream_t stream);
/* Sharded data-parallel tail ("scaling risk (b)"): elements [lo, hi) of the flat table -- multiples of 4,
 * this rank's slice of the reduce-scatter -- and `rec_scale` = 1 / ranks.  While a range is set (hi > lo):
 *   enerf_grid_encode_backward_ex(flags bit 0) keeps the record lists of the tiles wholly inside the range pending and
 *     flushes every other list into the dense gradient at once (that part travels through the reduce-scatter);
 *   enerf_grid_adam_from_records(_ex) updates the range only: rec_scale x (dense gradient -- what a SUM reduce-scatter
 *     delivered -- + this rank's own lists, summed in LDS as on one GPU); the dense gradient is cleared everywhere.
 * lo == hi clears the range.  The caller reduce-scatters the dense gradient between the two calls and all-gathers the
 * parameters after the second. */
int enerf_grid_owner_range(uint64_t lo, uint64_t hi, float rec_scale);
/* Abandon a pending deferred flush (error recovery: the record lists are emptied, nothing is applied). */
int enerf_grid_records_discard(enerf_stream_t stream);

/* ------------------------------------------------------------------ shencoder
 * shencoder/src/shencoder.cu:402-441; `dtype` ENERF_F32 or ENERF_F16 for every tensor. */

/* sh_encode_forward(inputs, outputs, B, D, C, calc_grad_inputs, dy_dx);  D must be 3, 1 <= C <= 8 */
int enerf_sh_encode_forward(const void* inputs, void* outputs, uint32_t B, uint32_t D, uint32_t C,
                            int calc_grad_inputs, void* dy_dx, int dtype, enerf_stream_t stream);

/* extension: fp32 forward, no Jacobian, rows of `outputs` out_stride floats apart (e.g. a 16-column slice of a
 * [B,32] buffer; 16-byte aligned rows when degree^2 % 4 == 0) */
int enerf_sh_encode_forward_strided(const float* inputs, float* outputs, uint32_t B, uint32_t C, uint32_t out_stride,
                                    enerf_stream_t stream);

/* sh_encode_backward(grad, inputs, B, D, C, dy_dx, grad_inputs); accumulates into grad_inputs */
int enerf_sh_encode_backward(const void* grad, const void* inputs, uint32_t B, uint32_t D, uint32_t C,
                             const void* dy_dx, void* grad_inputs, int dtype, enerf_stream_t stream);

/* ------------------------------------------------------------------ ffmlp
 * ffmlp/src/ffmlp.cu:632-895.  16-bit storage (`dtype` ENERF_F16 as the reference, or ENERF_BF16),
 * fp32 MFMA accumulation (the reference accumulates in fp16).  Weight blob layout
 * [W_in hid*in | W_h (k-1)*hid*hid | W_out out*hid], each W[out][in] row-major, y = x W^T, no bias.
 * B must be a multiple of 128 (ffmlp/ffmlp.py:157-159 pads), hidden_dim == 64, input_dim in {16,32,48,64},
 * output_dim == 16 (ffmlp.py:112-121 pads to 16), activation relu(0)/none(6). */

int enerf_ffmlp_forward(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim, uint32_t output_dim,
                        uint32_t hidden_dim, uint32_t num_layers, uint32_t activation, uint32_t output_activation,
                        void* forward_buffer, void* outputs, int dtype, enerf_stream_t stream);

int enerf_ffmlp_inference(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim,
                          uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                          uint32_t output_activation, void* inference_buffer, void* outputs, int dtype,
                          enerf_stream_t stream);

/* grad_weights (same 16-bit dtype, zero-filled by the caller) receives the batch-summed weight gradient;
 * backward_buffer [k,B,hid] receives the per-layer activation gradients as in the reference. */
int enerf_ffmlp_backward(const void* grad, const void* inputs, const void* weights, const void* forward_buffer,
                         uint32_t B, uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim,
                         uint32_t num_layers, uint32_t activation, uint32_t output_activation,
                         int calc_grad_inputs, void* backward_buffer, void* grad_inputs, void* grad_weights,
                         int dtype, enerf_stream_t stream);

/* 1 (default): enerf_ffmlp_forward / enerf_ffmlp_backward take the recomputing data flow where the shape allows (input_dim
 * 32, two or three hidden layers -- the two nets of nerf/network_ff.py --, ReLU / no hidden activation, no output
 * activation): the backward recomputes the hidden activations from the inputs (bit-identical to the forward's) and
 * `forward_buffer` / `backward_buffer` -- scratch to the reference's wrapper, ffmlp/ffmlp.py:34-83 -- are neither written nor
 * read: 160 B per sample instead of ~1.4 KB through HBM.  0: the buffered kernels (ffmlp.cu:410-518,711-895's data flow).
 * Forward and backward of a batch must run under the same setting.  Returns the previous setting; < 0 only queries. */
int enerf_ffmlp_recompute(int on);
/* ffmlp.cu:723-743: the reference (re)creates its split-K side streams here.  This implementation reduces weight
 * gradients inside the fused backward kernel, so these only (re)size the fp32 partial-sum workspace. */
int enerf_allocate_splitk(size_t size);
int enerf_free_splitk(void);

/* ------------------------------------------------------------------ extensions beyond the reference's native surface
 * (callers of the hot path: the nn.Linear MLPs of nerf/network.py:40-77 and the optimizer of main_nerf.py:211) */

/* Fused fp32 MLP on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains): X -> 64-wide hidden x num_hidden (1..3) ->
 * Y [B,out_dim <= 32], no bias; W = [W0 64x32 | Wh (num_hidden-1)x64x64 | Wout out_dim x 64], each W[out][in].
 * B is ragged; Bp = B rounded up to a multiple of 32.  x_layout 0: X is [B,32] row-major; x_layout 1: X is the
 * level-major [16,Bp,2] tensor enerf_grid_encode_forward writes with out_layout 2 (column k = 2*level + c).
 * fb (num_hidden * Bp * 64 floats) receives the post-activation hidden states in the library's own tile order -- opaque
 * to the caller, read back only by enerf_mlp32_backward (NULL = inference).
 * activation: relu (0) / none (6); output_activation additionally sigmoid (3).  Rows of Y are y_stride floats apart
 * (0 = out_dim), so the result can land in a slice of a wider buffer; y0_exp (optional, [B]) receives
 * exp(Y[:,0]) -- the trunc_exp forward of the density column (activation.py:5-17); Y may be NULL when only y0_exp is
 * wanted (density-grid updates). */
/* The whole network of nerf/network_ff.py (network_ff.py:60-88) as one inference kernel on the matrix cores:
 *   sigma_net = FFMLP(32 -> 64 -> 64 -> 16), sigma = exp(h[0]), geo_feat = h[1:16];
 *   color_net = FFMLP([SH(4) 16 | geo_feat 15 | 0] -> 64 -> 64 -> 64 -> 16), rgb = sigmoid(h[0:3]).
 * feats: the grid encoder's level-major fp32 output [16, Mp, 2], Mp = M rounded up to 32, pad rows zero
 * (enerf_grid_encode_forward, out_layout 2); dirs [M,3] fp32; w_sigma / w_color: the two FFMLP `weights` parameters as
 * they are (fp32, [W0 64x32 | Wh 64x64 x (layers-1) | Wout 16x64], 7168 and 11264 floats), converted to `dtype`
 * (ENERF_BF16 / ENERF_F16) on the way into LDS.  sigma [M], rgb [M,3] fp32, holding the 16-bit-rounded values the
 * op-by-op route produces (16-bit net outputs; exp / sigmoid in fp32 on the rounded value, rounded again). */
int enerf_ffnerf_inference(const float* feats, const float* dirs, const float* w_sigma, const float* w_color, uint32_t M,
                           int dtype, float* sigma, float* rgb, enerf_stream_t stream);

/* enerf_mlp32_forward / _backward with the weights (and weight gradients) where the caller keeps them, instead of one
 * packed blob: wseg / dwseg = {first layer [64, w0_cols], hidden 0 [64,64], hidden 1 [64,64], output layer
 * [out_dim,64]} (unused hidden slots NULL).  nerf_perm != 0 (w0_cols = 31): the first layer is color_net[0].weight of
 * nerf/network.py:95 as it is -- memory columns [SH 16 | geo_feat 15] -- while the kernels' input rows are [raw density
 * | geo_feat 15 | SH 16]; the permutation and the zero column are applied while the weights are staged into LDS, and
 * undone when the weight gradient is written.  overwrite != 0: dwseg receives the gradient (may be uninitialised). */
int enerf_mlp32_forward_p(const float* X, const float* const* wseg, uint32_t w0_cols, uint32_t nerf_perm, uint32_t B,
                          uint32_t in_dim, uint32_t out_dim, uint32_t num_hidden, uint32_t activation,
                          uint32_t output_activation, float* fb, float* Y, uint32_t x_layout, uint32_t y_stride,
                          float* y0_exp, const float* sh_dirs, enerf_stream_t stream);
int enerf_mlp32_backward_p(const float* dY, const float* X, const float* const* wseg, float* const* dwseg,
                           uint32_t w0_cols, uint32_t nerf_perm, uint32_t overwrite, const float* fb, uint32_t B,
                           uint32_t in_dim, uint32_t out_dim, uint32_t num_hidden, uint32_t activation, float* bb,
                           float* dX, uint32_t x_layout, uint32_t dy_stride, const float* y_sigmoid,
                           uint32_t y_sigmoid_stride, const float* dsigma, const float* h0, uint32_t h0_stride,
                           enerf_stream_t stream);

/* The two networks of nerf/network.py:104-132 as ONE launch per direction (csrc/nerf_mlp.hip; replaces the
 * sigma_net / color_net loops and the torch glue between them, nerf/network.py:108-130):
 *   h = sigma_net(feats);  sigma = exp(h[0]);  rgb = sigmoid(color_net([SH4(dirs) | h[1:16]]))
 * feats: the grid encoder's level-major fp32 output [16, Bp, 2] (enerf_grid_encode_forward, out_layout 2; Bp = B rounded
 * up to 32, pad rows zero), dirs [B,3]; wseg_s = {sigma_net[0].weight [64,32], NULL, NULL, sigma_net[1].weight [16,64]},
 * wseg_c = {color_net[0].weight [64,w0_cols_c] with memory columns [SH 16 | geo_feat 15], color_net[1].weight [64,64],
 * NULL, color_net[2].weight [out_c,64]}; sigma [B], rgb [B,out_c] (out_c <= 16).  The sigma net's 16 outputs never leave
 * the registers: they are the first half of the colour net's input as they stand, the SH basis is evaluated in registers.
 * Arithmetic: split-bf16 (enerf_mlp32_precision 1) -- enerf_nerf_mlp_available() says whether the process's current
 * arithmetic is served (callers fall back to enerf_mlp32_*_p otherwise).  Both calls honour enerf_mlp32_valid_rows; the
 * backward recomputes both forwards, honours enerf_mlp32_signal_next_reduce and writes (overwrite != 0) or adds the weight
 * gradients through dwseg_* (same shapes as wseg_*), the feature gradient level-major into dfeat [16, Bp, 2] (pad rows
 * zero: ready for enerf_grid_encode_backward with grad_layout 2).  g_sigma is multiplied by sigma_scale on the fly.
 * flags bit 0: the operand fragments an earlier call built from these very weight tensors are still current (no
 * optimizer step since) -- skips the 44-wavefront rebuild.  Backward, flags bit 1 (library-internal: enerf_train_step_mse
 * sets it): the weight gradients stay per-workgroup partial sums in the library's workspace for the optimizer launch that
 * follows; dwseg_* are not written by this call. */
int enerf_nerf_mlp_available(void);
int enerf_debug_nerf_mlp_fused(int on);
/* Testing aid, process-wide: how enerf_nerf_mlp_backward's kernel transposes the operands of its weight-gradient products.
 * 0: on the matrix pipe (products with 0/1 selection matrices), 1: through LDS with transposed reads (default; the same
 * operand bits, so the same gradients), -1: query only.  Returns the previous value. */
int enerf_debug_nerf_bwd_transpose(int mode);
/* Testing aid: the operand fragments (44 x 2048 bytes) as the last build left them, copied to device memory `dst`. */
int enerf_debug_nerf_frags_copy(void* dst, enerf_stream_t stream);
int enerf_nerf_mlp_forward(const float* feats, const float* dirs, const float* const* wseg_s, const float* const* wseg_c,
                           uint32_t w0_cols_c, uint32_t B, uint32_t out_c, float* sigma, float* rgb, uint32_t flags,
                           enerf_stream_t stream);
int enerf_nerf_mlp_backward(const float* g_rgb, const float* g_sigma, float sigma_scale, const float* feats,
                            const float* dirs, const float* rgb, const float* const* wseg_s, const float* const* wseg_c,
                            float* const* dwseg_s, float* const* dwseg_c, uint32_t w0_cols_c, uint32_t overwrite,
                            uint32_t B, uint32_t out_c, float* dfeat, uint32_t flags, enerf_stream_t stream);

/* enerf_mlp32_forward that also writes the degree-4 SH encoding of sh_dirs [B,3] (shencoder.cu:27-128) into columns
 * 16..31 of each row of Y: for the sigma net of nerf/network.py, whose output row is the colour net's input row
 * (num_hidden 1, level-major X, out_dim <= 16, y_stride >= 32).  sh_dirs == NULL: plain enerf_mlp32_forward. */
int enerf_mlp32_forward_sh(const float* X, const float* W, uint32_t B, uint32_t in_dim, uint32_t out_dim,
                           uint32_t num_hidden, uint32_t activation, uint32_t output_activation, float* fb, float* Y,
                           uint32_t x_layout, uint32_t y_stride, float* y0_exp, const float* sh_dirs,
                           enerf_stream_t stream);

/* dY [B,out_dim] with rows dy_stride floats apart (0 = out_dim); bb [num_hidden,Bp,64] is scratch (written); dX NULL
 * or laid out like X (x_layout 1: pad rows are written as zeros, ready for enerf_grid_encode_backward with
 * grad_layout 2); dW (fp32 blob) is accumulated (+=).  Optional fused epilogue gradients:
 *   y_sigmoid (rows y_sigmoid_stride apart): the forward's sigmoid output; dY is then the gradient of the sigmoid's
 *     output and (dY * (1 - y)) * y is back-propagated;
 *   dsigma [B] + h0 (rows h0_stride apart): the gradient of output column 0 is dsigma * exp(clamp(h0, -15, 15))
 *     (trunc_exp backward) instead of dY[:,0]. */
int enerf_mlp32_backward(const float* dY, const float* X, const float* W, const float* fb, uint32_t B, uint32_t in_dim,
                         uint32_t out_dim, uint32_t num_hidden, uint32_t activation, float* bb, float* dX, float* dW,
                         uint32_t x_layout, uint32_t dy_stride, const float* y_sigmoid, uint32_t y_sigmoid_stride,
                         const float* dsigma, const float* h0, uint32_t h0_stride, enerf_stream_t stream);

/* Rows of a training batch that are real: `device_count` points at a device int32 (the march's counter[0]); the
 * enerf_mlp32_* calls that follow skip the tiles beyond min(*device_count, B) -- the sample budget's padding, which no
 * ray covers (forward: left unwritten; fused backward: zero input gradients) -- until it is set again; NULL: every row
 * is real. */
int enerf_mlp32_valid_rows(const int32_t* device_count);
/* The same with real rows = base + min(*device_count, cap): two renders' samples as one batch (the first render's M rows,
 * its padding included, then the second's counter capped at its own M).  cap == 0: as enerf_mlp32_valid_rows. */
int enerf_mlp32_valid_rows_ex(const int32_t* device_count, uint32_t base, uint32_t cap);
/* 1: the enerf_mlp32_forward_p / _backward_p calls that follow, until set again, take 16-bit (IEEE half) row-major
 * tensors where they otherwise take fp32 ones: X [B,32], Y [B,y_stride], dY [B,dy_stride], y_sigmoid [B,y_sigmoid_stride]
 * and dX [B,32]; weights, weight gradients, dsigma and h0 stay fp32.  Served with enerf_mlp32_precision(3) only, for
 * two or three hidden layers, out_dim <= 16, x_layout 0 and no SH / density epilogue; the backward recomputes the hidden
 * activations (fb is not read).  Outputs are the 16-bit values mode 3 rounds them to (a sigmoid output: sigmoid of the
 * half-rounded net output, rounded to half).  Honours enerf_mlp32_valid_rows.  Returns the previous setting; < 0 only
 * queries. */
int enerf_mlp32_io16(int on);
/* Arithmetic of the enerf_mlp32_* kernels (the nn.Linear nets of nerf/network.py:40-77 are fp32):
 *   0  v_mfma_f32_32x32x2_f32: every dot product an fp32 fmaf chain, bit-comparable with an fp32 GEMM;
 *   1  (default) split-bf16: every fp32 operand as bf16 hi + lo, three bf16 MFMA products per fp32 product (hi*hi +
 *      hi*lo + lo*hi), fp32 accumulation: ~2^-16 relative per product, inside the path's 1e-4, at 3/16 of the fp32
 *      MFMA's pipe time.  Applies to forward, dgrad and wgrad (the fused backward; nets with three hidden layers or
 *      more than 16 outputs keep mode 0 in the backward).
 *   2  bf16 operands: inputs, weights and each layer's activations / activation gradients rounded to bf16, one MFMA
 *      product, fp32 accumulation, outputs (and exp / sigmoid of them) rounded to bf16 -- the arithmetic of the FFMLP
 *      nets (enerf_ffmlp_*, ffmlp/src/ffmlp.cu:410-895) over this family's fp32 buffers and fused epilogues; serves the
 *      fused training step of nerf/network_ff.py (sigma net: two hidden layers + SH epilogue, colour net: three).
 *   3  fp16 operands: mode 2's kernels and rounding points on IEEE half (v_mfma_f32_32x32x16_f16; trunc_exp of the density
 *      head stays in fp32, activation.py:5-17 `cast_inputs=torch.float`) -- the arithmetic autocast(float16) gives the
 *      nn.Linear nets in the reference's `fp16 = True` regime (nerf/utils.py:964-975).  fp16's range is why that regime
 *      scales its loss: use with enerf_amp_begin / enerf_amp_end.
 * Returns the previous mode (NOT a status); a negative `mode` only queries. */
int enerf_mlp32_precision(int mode);
/* 1 (default): in modes 1 / 2 the fused backward recomputes the hidden activations from X with the forward's own
 * instruction sequence (bit-identical values and ReLU masks) and the training forward does not store them -- `fb` is
 * then neither written nor read (two thirds of these kernels' HBM traffic at the training batch).  0: the forward
 * stores them and the backward loads them (the reference's data flow, ffmlp.cu:711-895 / autograd's saved tensors).
 * Forward and backward of a batch must run under the same setting.  Nets with three hidden layers (16-bit operands) recompute
 * under either setting.  Returns the previous setting (NOT a status);
 * a negative `on` only queries. */
int enerf_mlp32_recompute(int on);
/* Testing aid: 1 (default) lets enerf_mlp32_backward use its fused dgrad + wgrad kernel (num_hidden <= 2; `bb` is then
 * not written), 0 forces the separate dgrad / wgrad kernels. */
int enerf_debug_mlp32_fused_backward(int on);
/* One-shot: the NEXT enerf_mlp32_backward[_p] call on this process leaves its weight-gradient partial sums pending,
 * and the call after it reduces both networks' sums in a single launch (a network's two MLPs are always run
 * back to back: one reduce launch and one launch gap less per step).  The pending sums live in their own workspace;
 * nothing is written to the first call's dW until the second call. */
int enerf_mlp32_defer_reduce(int on);
/* Cross-stream hand-over without an event record in the launching stream: once armed (on = 1), the next weight-gradient
 * reduce launch of enerf_mlp32_backward[_p] carries a completion signal; enerf_stream_wait_mlp32_signal makes `stream`
 * wait for that launch (and, the launching stream being in order, for everything queued before it).  Error if no
 * launch has carried the signal since it was armed. */
int enerf_mlp32_signal_next_reduce(int on);
int enerf_stream_wait_mlp32_signal(enerf_stream_t stream);
/* Loss scaling of the reference's fp16 regime (nerf/utils.py:964-975: scaler.scale(loss).backward(); scaler.step(optimizer);
 * scaler.update()) around a closed-form step, on the device.  `scale` (fp32) and `growth_tracker` (int32) are the
 * torch.amp.GradScaler's own device tensors, `found_inf` and `skipped` two zero-initialised uint32 words kept by the caller.
 * Between enerf_amp_begin and enerf_amp_end: the compositing backward multiplies the loss gradient by *scale; the MLP
 * weight-gradient reduce launch raises *found_inf when a sum is not finite; enerf_grid_adam_from_records(_ex) divides the
 * gradients by *scale, counts its step as (step - *skipped) and leaves the parameters alone when *found_inf is set.
 * enerf_amp_end queues GradScaler.update() (backoff after a non-finite step, growth after growth_interval clean ones),
 * counts a skipped step in *skipped, clears *found_inf and disarms; enerf_amp_cancel only disarms.  No host
 * synchronisation.  Use with enerf_mlp32_precision(3) (fp16 operands). */
int enerf_amp_begin(float* scale, int32_t* growth_tracker, uint32_t* found_inf, uint32_t* skipped);
int enerf_amp_end(float growth_factor, float backoff_factor, int32_t growth_interval, enerf_stream_t stream);
int enerf_amp_cancel(void);
/* 1 while armed.  Only the kernels named above unscale and skip: the record-list Adam launch (table + up to 8 small tensors).
 * The table's gradient itself is not inspected for non-finite values -- it is dL/dfeature (whose overflow the first layer's
 * weight gradient, which IS inspected, shares) times trilinear weights <= 1. */
int enerf_amp_armed(void);
/* Tuning aid: number of workgroups (= partial weight-gradient sums) enerf_mlp32_backward launches; 0 restores the
 * default (768 for one hidden layer, 512 otherwise). */
int enerf_debug_mlp32_wgrad_blocks(uint32_t blocks);
/* tuning aid: largest alive-ray count for which enerf_march_rays runs one wavefront per ray (when n_step < 16) */
int enerf_debug_march_wave_max_rays(uint32_t n);
/* test / measurement aid: 0 switches off the occupied-box test (below) globally */
int enerf_debug_march_clip(int on);
/* While on, enerf_march_rays(_ex) trust the box enerf_occupied_box_update last computed when it was computed for the same
 * bitfield pointer / C / H / bound (the caller vouches that the bitfield has not changed since: a frame's rounds); off
 * (default), a round of 32 768+ rays computes the box for itself and smaller rounds march without it.  A ray emits no
 * sample outside the box, so the walk stops at its far side: same samples, slots and termination. */
int enerf_march_rays_use_box(int on);
/* tuning / test aid: smallest ray count for which the fixed-step enerf_march_rays_train* counts with one thread per ray
 * and a run log (instead of one wavefront per ray and a chunk log); 0 only reads.  Returns the previous value.  The
 * count and the write pass of a batch must see the same setting. */
int enerf_debug_march_thread_min_rays(uint32_t n);
/* Testing aid: 0 switches off the cross-stream ordering of the library's shared workspaces (a stream that is about to
 * use a kernel family's scratch waits for the family's previous user when that was another stream); 1 = default. */
int enerf_debug_workspace_ordering(int on);
/* tuning aid: workgroups of the background training march (enerf_march_rays_train_ex flag bit 1); 0 = one per CU */
int enerf_debug_march_bg_blocks(uint32_t n);
/* tuning aid: workgroup caps of the mlp32 forward and fused-backward grids (0 = built-in defaults) */
int enerf_debug_mlp32_grid_caps(uint32_t fwd_blocks, uint32_t bwd_blocks);
/* Testing aid, process-wide: form of the density-only head (the mlp32 forward with Y == NULL, y0_exp set, one hidden layer,
 * level-major X: update_extra_state's and the mesh lattice's sigma).  1 (default): a wavefront keeps the inputs of several
 * of its tiles on request (the load pipeline of csrc/mlp32s.hip) on a grid that fills the device; 0: one tile ahead on 512
 * workgroups, the form shipped before -- the same per-tile arithmetic, so the same sigma bit for bit; -1: query only.
 * Returns the previous value.  enerf_debug_mlp32_grid_caps' forward cap applies to both.  enerf_mlp32_precision(0) (exact
 * fp32, bound by its fp32 MFMAs) runs the old form whatever is selected here. */
int enerf_debug_sigma_head(int form);

/* Event-pair ray generation (the caller that feeds the event step: EventNeRFDataset.collate, nerf/provider.py:1364-1441,
 * accumulate_evs branch with poses "computed online", + get_event_rays, nerf/utils.py:184-216), one thread per pair:
 *   s = start_draw[k] - no_successor[start_draw[k]];  ns = min(num_successor[s], acc_max_num_evs + 1) (0 = no cap);
 *   e = s + 1 + min(floor(u_end[k] * ns), ns - 1);    pols[k] = pol_cumsum[e + 1] - pol_cumsum[s + 1];
 *   pose(t) for t = events[s].t and events[e].t from the track: R = rot[i] * exp(alpha * rotvec[i]) (scipy Slerp),
 *   translation = cubic tcoef[i] in (t - knots[i]) (interp1d(kind="cubic") as a piecewise polynomial), segment i by
 *   binary search over knots[K], evaluated in double, rounded to fp32; rays: pixel (x, y) of event s -> unit camera
 *   direction -> rays_d = R d, rays_o = translation, at both poses.
 * events [N,4] fp32 rows (x, y, t, polarity) grouped by pixel (enerf_amd/event_sampler.build_event_tables);
 * no_successor u8 [N]; num_successor i64 [N]; pol_cumsum f64 [N+1]; start_draw i64 [M] in [0,N); u_end f64 [M] in [0,1);
 * rot f64 [K,9]; rotvec f64 [K-1,3]; tcoef f64 [K-1,4,3] (highest power first); outputs [M,3] fp32, pols [M] fp32,
 * start/end i64 [M]; *outside_track += pairs whose times fall outside [knots[0], knots[K-1]]. */
int enerf_event_pair_rays(const float* events, const uint8_t* no_successor, const int64_t* num_successor,
                          const double* pol_cumsum, uint32_t N, const int64_t* start_draw, const double* u_end,
                          uint32_t M, uint32_t acc_max_num_evs, const double* knots, const double* rot,
                          const double* rotvec, const double* tcoef, uint32_t K, float fx, float fy, float cx, float cy,
                          float* rays_o1, float* rays_d1, float* rays_o2, float* rays_d2, float* pols,
                          int64_t* start_out, int64_t* end_out, int32_t* outside_track, enerf_stream_t stream);

/* The same with accumulate_evs off (nerf/provider.py:1400-1405, the branch every shipped config takes), one thread per
 * pair: c = choice[k]; s = (int64) trunc(u_xy[c] * (double) num_at_xy[c] - 1.0) + first_at_xy[c] (the product and the
 * difference each rounded; truncation toward zero: (np.random.rand(P) * num - 1).astype(int) + first); e = s + 1;
 * pols[k] = events[e].polarity; pixel of event s, poses at events[s].t and events[e].t, rays as above.
 * num_at_xy / first_at_xy i64 [P] (events per kept pixel, index of its first event); u_xy f64 [P] in [0,1); choice i64 [M].
 * A choice[k] outside [0, P) -- or an s outside [0, N - 2], which no valid table and u_xy > 0 produce -- reads nothing:
 * the pair's outputs are zero and *bad_choice += 1.  *outside_track as above.  M == 0: no launch. */
int enerf_event_single_pair_rays(const float* events, uint32_t N, const int64_t* num_at_xy, const int64_t* first_at_xy,
                                 uint32_t P, const double* u_xy, const int64_t* choice, uint32_t M, const double* knots,
                                 const double* rot, const double* rotvec, const double* tcoef, uint32_t K, float fx,
                                 float fy, float cx, float cy, float* rays_o1, float* rays_d1, float* rays_o2,
                                 float* rays_d2, float* pols, int64_t* start_out, int64_t* end_out,
                                 int32_t* outside_track, int32_t* bad_choice, enerf_stream_t stream);
/* The no-event rays of --negative_event_sampling (nerf/provider.py:1443-1476), one thread per pixel: pixel
 * coords[idx[k]] (x, y) of one chunk's event-free pixels; ta = t0_us + (t1_us - t0_us) * u[k][0], tb likewise (each
 * operation rounded), tss_out[k] = (min, max) in microseconds; poses at 1000 * those (the track is in nanoseconds), rays as
 * above.  coords fp32 [n_coords,2]; idx i64 [n]; u f64 [n,2]; tss_out f64 [n,2].  An idx[k] outside [0, n_coords) reads
 * nothing: zero outputs, *bad_index += 1.  *outside_track += pixels with a time outside the track.  n == 0: no launch. */
int enerf_no_event_rays(const float* coords, uint32_t n_coords, const int64_t* idx, const double* u, uint32_t n,
                        double t0_us, double t1_us, const double* knots, const double* rot, const double* rotvec,
                        const double* tcoef, uint32_t K, float fx, float fy, float cx, float cy, float* rays_o1,
                        float* rays_d1, float* rays_o2, float* rays_d2, double* tss_out, int32_t* outside_track,
                        int32_t* bad_index, enerf_stream_t stream);

/* From a raw event stream to the tables above (csrc/event_tables.hip): the grouping loop of
 * EventNeRFDataset.__init__ (nerf/provider.py:1152-1199) and the no-event search of load_events_at_frame_idxs
 * (provider.py:1283-1351), keyed on the SENSOR pixel y * W + x.  The stream, all on the device: x, y u16 [>= last] sensor
 * pixel; t i64, ascending, in stream units; p i8 polarity (+1 where p > 0, -1 otherwise: serves 0/1 and -1/+1 files).  A
 * call works on the window [first, last) of 1 .. 2^30 events; H * W <= 2^26, H, W <= 65536.  Event time in nanoseconds:
 * t_ns = (double)(t + t_offset) * ns_per_unit (the sum in int64, one rounded product).
 *
 * enerf_event_tables_workspace: *bytes = size of the scratch buffer the two calls below share for a window of n_events
 * events.  Its layout depends on the exact n_events, H, W and n_chunks: ask per window.  The caller allocates it (256-byte
 * aligned, contents arbitrary) and may free it once _fill's launches have run. */
#define ENERF_EVT_SEGMENT_TILE 4096 /* events of one pixel that are ordered in LDS; longer segments: in global memory */
int enerf_event_tables_workspace(uint64_t n_events, uint32_t H, uint32_t W, uint32_t n_chunks, uint64_t* bytes);
/* Pass one over the window.  Per event, its coordinates compared with W, H BEFORE anything is indexed (an event outside
 * the sensor is skipped and counted): with `tables` != 0 the per-pixel event count and the window position of the pixel's
 * first event; with n_chunks != 0 the pixel's bit in the bitmap of chunk j, where edges_us[j] <= tt < edges_us[j + 1],
 * tt = t_ns * 1e-3 (rounded; an event before edges_us[0] or at / after edges_us[n_chunks] is in no chunk).  Then, with
 * `tables`: the kept pixels (two events or more) ranked by the position of their first event, their counts and the
 * prefix sum of the counts, left in the workspace for _fill.  With n_chunks: no_event_pixels i64 [n_chunks, H * W] row j
 * = the linear indices of the pixels WITHOUT an event in chunk j, ascending; the rest of the row is not written.
 * edges_us f64 [n_chunks + 1] on the device, ascending.  report i64 [4 + n_chunks] on the device: N (events of kept
 * pixels), P (kept pixels), bad (events outside the sensor), 0, then the n_chunks row lengths; N and P are 0 without
 * `tables`.  t may be NULL when n_chunks == 0; edges_us / no_event_pixels when n_chunks == 0.  All launches on `stream`;
 * the host reads `report` after synchronising. */
int enerf_event_tables_count(const uint16_t* x, const uint16_t* y, const int64_t* t, uint64_t first, uint64_t last,
                             uint32_t H, uint32_t W, double ns_per_unit, int64_t t_offset, uint32_t tables,
                             const double* edges_us, uint32_t n_chunks, void* workspace, int64_t* report,
                             int64_t* no_event_pixels, enerf_stream_t stream);
/* Pass two, after a _count with `tables` on the same window, workspace and n_chunks, with the N >= 2 and P >= 1 it
 * reported: the tables build_event_tables returns, in the kernels' layout.  Pixels in the order of their first event, a
 * pixel's events in stream order (which, the stream being time-sorted and fp32 rounding monotone, is the reference's stable
 * sort on the fp32 time, ties included).  events f32 [N, 4] rows (x', y', (float) t_ns, +-1) with (x', y') =
 * rect[y][x][0 .. 1] (rect f32 [H, W, 2]) or, rect == NULL, the integer coordinates as floats; no_successor u8 [N] (last
 * event of its pixel); num_successor i64 [N] (later events of the pixel); pol_cumsum f64 [N + 1], the exclusive prefix sum
 * of the polarities (an integer scan, converted: exact); num_at_xy / first_at_xy i64 [P].  events must be 16-byte aligned.
 * Every output has the same bits on every run.  May be repeated on the same workspace.  An N, P that cannot belong to the
 * window answers ENERF_E_BADARG; one that merely differs from the report writes nothing out of bounds (rows it cannot
 * fill are NaN). */
int enerf_event_tables_fill(const uint16_t* x, const uint16_t* y, const int64_t* t, const int8_t* p, uint64_t first,
                            uint64_t last, uint32_t H, uint32_t W, const float* rect, double ns_per_unit, int64_t t_offset,
                            void* workspace, uint32_t n_chunks, uint32_t N, uint32_t P, float* events, uint8_t* no_successor,
                            int64_t* num_successor, double* pol_cumsum, int64_t* num_at_xy, int64_t* first_at_xy,
                            enerf_stream_t stream);
/* The chosen event-free pixels of one chunk through the map (provider.py:1337-1343), one thread per pixel: coords f32
 * [max(n, 1), 2] row k = rect[pixels[k] / W][pixels[k] % W][0 .. 1], or (pixels[k] % W, pixels[k] / W) with rect == NULL.
 * n == 0: the one dummy row (0, 0).  A pixels[k] outside [0, H * W) reads nothing: its row is NaN and *bad_index += 1
 * (bad_index may be NULL). */
int enerf_no_event_coords(const int64_t* pixels, uint32_t n, const float* rect, uint32_t H, uint32_t W, float* coords,
                          int32_t* bad_index, enerf_stream_t stream);
/* Testing aid: the two sort launches of enerf_event_tables_fill (a thread per segment of at most 32 entries, a workgroup
 * per longer one, on the grid _fill uses for P segments) on segments of the caller's choice, so that a test decides what
 * the sort is handed -- in _fill it only ever sees the nearly ascending arrival order of the placement's atomics.
 * idx u32 [N] on the device; segment r is idx[first[r] .. first[r] + num[r]) (num, first u32 [P], 1 <= P <= N) and comes
 * back ascending; a segment that does not lie inside [0, N) is left alone, and so is every entry outside the segments.
 * workspace: 20 * P + 32 bytes on the device, 8-byte aligned, contents arbitrary; afterwards it begins with num and first
 * as i64 [P] each (the num_at_xy / first_at_xy of _fill). */
int enerf_debug_event_segment_sort(uint32_t* idx, uint32_t N, const uint32_t* num, const uint32_t* first, uint32_t P,
                                   void* workspace, enerf_stream_t stream);

/* The loader's side of the same stream (csrc/event_stats.hip): per-pixel counts, the accumulation images
 * of utils/plot_utils.py render_ev_accumulation (nerf/provider.py:227-230, :313-316), a hot-pixel mask, and the stream
 * without the events of masked pixels.  x, y, t, p as above; windows [first, last) of 1 .. 2^30 events; H * W <= 2^26,
 * H, W <= 65536.  Integer work: every output has the same bits on every run.
 *
 * enerf_event_pixel_stats: one pass over the window.  Per event, its coordinates compared with W, H BEFORE anything is
 * indexed (an event outside the sensor is skipped and counted in *bad); then counts[y][x][p > 0 ? 1 : 0] += 1 (counts i32
 * [H, W, 2]: polarity -1, polarity +1) and, where the arrays are given, last_sensor[y][x] = max(., i + 1) with i the
 * event's index in the window, and last_rect[(int) yr][(int) xr] = max(., i + 1) with (xr, yr) = rect[y][x][0 .. 1] (f32
 * [H, W, 2]) kept only if xr >= 0 && yr >= 0 && xr < W && yr < H in fp32 (false for NaN), truncated.  last_sensor,
 * last_rect u32 [H, W] or NULL; 0 = no event.  last_rect needs rect.  The call zeroes counts, the arrays given and *bad
 * (u64 [1]) first.  counts, rect and bad 8-byte aligned. */
int enerf_event_pixel_stats(const uint16_t* x, const uint16_t* y, const int8_t* p, uint64_t first, uint64_t last, uint32_t H,
                            uint32_t W, const float* rect, int32_t* counts, uint32_t* last_sensor, uint32_t* last_rect,
                            uint64_t* bad, enerf_stream_t stream);
/* A last-event array of enerf_event_pixel_stats on the same window to the picture: image u8 [H, W, 3], 4-byte aligned;
 * a cell without an event (255, 255, 255), one whose last event has p <= 0 (255, 0, 0), p > 0 (0, 0, 255).  An entry
 * above last - first reads nothing and is drawn as no event. */
int enerf_event_accumulation_image(const uint32_t* last_event, const int8_t* p, uint64_t first, uint64_t last, uint32_t H,
                                   uint32_t W, uint8_t* image, enerf_stream_t stream);
/* moments u64 [3] = n, S, Q: the pixels with c > 0, the sum of c and the sum of c * c, c = counts[y][x][0] +
 * counts[y][x][1] (each read as u32).  An integer reduction: any order gives the same bits.  The call zeroes moments
 * first.  counts and moments 8-byte aligned. */
int enerf_event_count_moments(const int32_t* counts, uint32_t H, uint32_t W, uint64_t* moments, enerf_stream_t stream);
/* mask u8 [H, W] = c > threshold (1 / 0), every byte written; report u64 [2] = the number of such pixels and the sum of
 * their c.  The call zeroes report first.  counts and report 8-byte aligned. */
int enerf_event_hot_mask(const int32_t* counts, uint32_t H, uint32_t W, uint64_t threshold, uint8_t* mask, uint64_t* report,
                         enerf_stream_t stream);
/* The stream without the events of masked pixels, order kept: a keep flag per event (on the sensor -- compared before
 * the mask is indexed -- and mask[y][x] == 0; mask u8 [H, W]), the exclusive scan of the flags, and x, y, t, p of every
 * kept event written at its scanned position.  The outputs hold n_events entries each (1 .. 2^30); entries from the kept
 * count on are not written.  report u32 [2] on the device = the kept count, the events outside the sensor (dropped);
 * the call zeroes it first.  _workspace: *bytes = the scratch buffer of a call on n_events events (4-byte aligned,
 * contents arbitrary, free once the launches have run). */
int enerf_event_stream_compact_workspace(uint64_t n_events, uint64_t* bytes);
int enerf_event_stream_compact(const uint16_t* x, const uint16_t* y, const int64_t* t, const int8_t* p, uint64_t n_events,
                               uint32_t H, uint32_t W, const uint8_t* mask, void* workspace, uint16_t* x_out,
                               uint16_t* y_out, int64_t* t_out, int8_t* p_out, uint32_t* report, enerf_stream_t stream);

/* The event loss of Trainer.train_step_events (nerf/utils.py:499-516, C_thres != -1) and its gradient with respect to
 * the two rendered images, one launch: image1 / image2 [N,3] fp32, pols [N] -> delta [N,1] (use_luma) or [N,3],
 * grad_image1 / grad_image2 [N,3] (d (upstream * loss) / d image), loss [1] (may be NULL).  (utils/event_utils.py:23-66:
 * BT.601 luma, lin-log with threshold 20 on the 0..255 scale, or log(max(., log_thres)); without lin-log and with luma
 * the reference evaluates both terms on the first image -- kept.)  Replaces ~50 elementwise / reduction launches of
 * the autograd route per step. */
int enerf_event_loss_fwd_bwd(const float* image1, const float* image2, const float* pols, uint32_t N, uint32_t use_luma,
                             uint32_t linlog, float C_thres, float log_thres, float upstream, float* grad_image1,
                             float* grad_image2, float* delta, float* loss, enerf_stream_t stream);

/* The same for images of `channels` = 1, 2 or 3 channels: without luma, image1 / image2 / delta / grad_image1 /
 * grad_image2 are [N,channels] and the mean runs over N * channels values.  Luma is a three-channel operation: use_luma
 * with channels != 3 is ENERF_E_BADARG, as is channels outside 1..3. */
int enerf_event_loss_fwd_bwd_c(const float* image1, const float* image2, const float* pols, uint32_t N, uint32_t use_luma,
                               uint32_t linlog, float C_thres, float log_thres, float upstream, float* grad_image1,
                               float* grad_image2, float* delta, float* loss, uint32_t channels, enerf_stream_t stream);
/* C_thres == -1 selects the normalised loss (nerf/utils.py:521-528), also one launch: per channel k over the N rays,
 * loss = upstream * mean_{rays,channels} (d_k / (|d_k|_2 + 1e-9) - pol / (|pol|_2 + 1e-9))^2, the N rays taken as ONE batch
 * entry.  delta receives the un-normalised p2 - p1 as above.  Where |d_k|_2 == 0 the norm's gradient is taken as zero
 * (torch's subgradient).  The reference weights this loss by 20, and by 20 again when frames are trained too
 * (event_only = 0): that weight is not the kernel's business, the caller folds it into `upstream`. */

/* The no-event term of --negative_event_sampling (nerf/utils.py:548-566) and its gradient, one launch:
 * loss = upstream * mean(relu(|p2 - p1| - C_no)) over N * channels values (use_luma: over the N lumas; three channels
 * only), p always the lin-log intensity.  grad_image1 / grad_image2 [N,channels] = upstream / count * sign(p2 - p1) *
 * [|p2 - p1| > C_no] * dp/dl: zero at the kink and at p2 == p1.  loss [1] may be NULL.  Refusals as above; N == 0: no
 * launch. */
int enerf_no_event_loss_fwd_bwd_c(const float* image1, const float* image2, uint32_t N, uint32_t use_luma, float C_no,
                                  float upstream, float* grad_image1, float* grad_image2, float* loss, uint32_t channels,
                                  enerf_stream_t stream);

/* The implicit contrast threshold of an event step (utils/event_utils.py:69-107 estimate_C_thres_from_pol_dL with its
 * documented (N,1) / (N,C) shapes), one launch, nothing read back: delta [N,channels] (the event loss's delta), pols [N]
 * -> medians [4] of delta[i,k] / pols[i] over the classes  on: pol > 0;  off: pol < 0;  on_sign: pol > 0 and
 * delta[i,0] >= 0;  off_sign: pol < 0 and delta[i,0] <= 0  (an event with pol == 0 or a NaN pol is in no class; a NaN
 * delta[i,0] fails both sign conditions).  A class's values are the quotients of all its events' channels, counts [4]
 * (may be NULL) their number.  Median as torch.median: the value of rank (count - 1) / 2, ascending; NaN when the class
 * holds a NaN; 0 for an empty class.  The quotient is the correctly rounded fp32 one.  No luma is formed (the reference
 * forms one when N == 3 -- the caller's business).  N == 0: four zeros and zero counts.  channels outside 1..3, N *
 * channels above 2^32 - 65536, or a NULL among delta / pols / medians with N > 0: ENERF_E_BADARG.  The same bits on every run. */
int enerf_event_c_estimate(const float* delta, const float* pols, uint32_t N, uint32_t channels, float* medians,
                           uint32_t* counts, enerf_stream_t stream);

/* One fused Adam update (torch.optim.Adam semantics, no weight decay / amsgrad) of a contiguous fp32 tensor:
 * reads p, g, m, v once and writes p, m, v (and g = 0 when zero_grad != 0).  `step` counts from 1. */
int enerf_adam_step(float* p, float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                    uint32_t step, int zero_grad, enerf_stream_t stream);
/* The same update for up to 16 parameters in one launch: arrays of `count` device pointers / sizes / learning rates /
 * step counts (host memory), shared betas and eps. */
int enerf_adam_step_multi(uint32_t count, float* const* p, float* const* g, float* const* m, float* const* v,
                          const size_t* n, const float* lr, const uint32_t* step, float beta1, float beta2, float eps,
                          int zero_grad, enerf_stream_t stream);
/* The exponential moving average of the parameters (torch_ema's update as nerf/utils.py:1005-1006 calls it; semantics in
 * enerf_amd/ema.py and DESIGN.md 4.14): shadow[i] = shadow[i] - ((shadow[i] - p[i]) * one_minus_decay) element by element,
 * three fp32 operations each rounded once, for up to 16 contiguous fp32 tensors in one launch.  Arrays of `count` device
 * pointers / sizes (host memory).  A tensor whose two pointers are 16-byte aligned is walked in 16-byte accesses with a
 * scalar tail, any other one element by element.  n[i] == 0 is a no-op (its pointers are not looked at); count == 0
 * returns 0; count > 16, or a null pointer with n[i] > 0, is ENERF_E_BADARG. */
int enerf_ema_update_multi(uint32_t count, float* const* shadow, const float* const* p, const size_t* n,
                           float one_minus_decay, enerf_stream_t stream);

/* ------------------------------------------------------------------ one training step as one call (not in the reference)
 * The closed-form RGB step of the nn.Linear / FFMLP networks on one GPU -- render of a batch whose samples have been
 * marched already, MSE against `target`, backward, the hash table's Adam from the backward's record lists together with
 * the MLP weights' Adam, and (optionally) near_far + march_rays_train of the NEXT batch on `side_stream` behind the MLP
 * backward -- issued by the library itself, in the order and with the arguments of the entry points above
 * (grid_encode_forward, mlp32_forward_p x 2, composite_rays_train_fwd_bwd_mse, mlp32_backward_p x 2, near_far_from_aabb,
 * march_rays_train_ex, grid_encode_backward_ex(defer), grid_adam_from_records_ex): results are those of the calls made
 * one by one.  What it removes is the host's work between the launches (nerf/utils.py:575-640 + main_nerf.py:211 run
 * ~60 framework calls per step).  All pointers are device pointers unless noted; every buffer is the caller's.
 * Scalar background (bg_scalar), density_scale 1, fp32 table with L = 16, C = 2, D = 3.
 * The step's grid and MLP launches take their valid rows from its own `counter` field (NULL, or flags bit 2: every row) and
 * their arithmetic from its own `mlp_precision` field; its next march takes near / far and the count mirror from the struct:
 * the step neither consumes nor clears the process-wide enerf_mlp32_valid_rows, enerf_mlp32_signal_next_reduce,
 * enerf_mlp32_defer_reduce, enerf_march_fuse_near_far or enerf_march_mirror_count requests, and leaves enerf_mlp32_precision
 * as it is. */
#define ENERF_STEP_EVERY_ROW 4u      /* `flags` bit 2 of both step structs: the grid and MLP launches take every row of the
                                      * budget, as with counter == NULL; the compositing keeps `counter`, which it requires */
#define ENERF_STEP_MARCH_CARRIED 1u  /* `report` bit 0 of both: the next march(es) ran in this call's own launches on `stream`;
                                      * side_stream saw nothing (no event to wait for) */
typedef struct enerf_train_step_args {
    uint32_t struct_bytes;              /* sizeof(enerf_train_step_args): checked */
    int mlp_precision;                  /* enerf_mlp32_precision's mode for this call's MLP launches; < 0: the process's */
    enerf_stream_t stream, side_stream; /* side_stream only used when next_rays_o != NULL */
    /* this batch: samples from march_rays_train (M rows budgeted, counter[0] real), N rays */
    uint32_t N, M;
    const float *xyzs, *dirs, *deltas;
    const int32_t *rays, *counter;
    const float* target;                /* [N,out_c] */
    float bg_scalar, grad_scale;        /* d loss / d image = (out_image - target) * grad_scale */
    float* loss;                        /* device scalar the loss value is added into, or NULL */
    /* networks */
    const float* embeddings;            /* == table below */
    const int32_t* offsets;
    float level_scale_log2, bound, inv_two_bound;
    uint32_t base_resolution, gridtype;
    const float* const* wseg_s;         /* host arrays of 4 device pointers, as enerf_mlp32_forward_p takes them */
    const float* const* wseg_c;
    float* const* dwseg_s;              /* where the weight gradients are written (overwrite) */
    float* const* dwseg_c;
    uint32_t nh_s, nh_c, w0_cols_c, out_c;   /* out_c: colour channels, 1..3 (the compositing's channel count) */
    /* scratch of the step, all fp32: feats [16,Mp,2], h32 [M,32], fb_s [nh_s,Mp,64], fb_c [nh_c,Mp,64], sigma [M],
     * rgb [M,out_c], weights_sum [N], image [N,out_c], out_image [N,out_c], g_sigmas [M], g_rgbs [M,out_c], dx32 [M,32],
     * dfeat [16,Mp,2] (Mp = M rounded up to 32) */
    float *feats, *h32, *fb_s, *fb_c, *sigma, *rgb, *weights_sum, *image, *out_image, *g_sigmas, *g_rgbs, *dx32, *dfeat;
    /* next batch's march (next_rays_o == NULL: none).  march_flags: enerf_march_rays_train_ex's zero_unwritten bits 0-3,
     * plus bit 4 = keep this march on side_stream (the caller reads its counter back behind it there); without bit 4 the
     * march may ride in this call's own launches on `stream` (`report` says whether it did) and side_stream sees nothing.
     * next_count_host [host]: two words of pinned, device-visible memory, or NULL; the next march also stores its counter
     * there (enerf_march_mirror_count's semantics, for this march only) and then never rides on `stream` */
    const float *next_rays_o, *next_rays_d, *aabb;
    const uint8_t* bitfield;
    float min_near, dt_gamma;
    uint32_t next_N, next_M, cascade, grid_size, max_steps, perturb, march_flags;
    float *next_nears, *next_fars, *next_xyzs, *next_dirs, *next_deltas;
    int32_t *next_rays, *next_counter, *next_count_host;
    /* optimizer: the table (dense gradient buffer for the levels too small to bin, zero-filled, comes back clean) and up
     * to 8 small tensors whose gradients the backward has just written through dwseg_* */
    float *table, *table_grad, *table_m, *table_v;
    float lr, beta1, beta2, eps;
    uint32_t table_step, n_small;
    float* const* small_p;              /* host arrays of n_small entries, as enerf_grid_adam_from_records_ex takes them */
    const float* const* small_g;
    float* const* small_m;
    float* const* small_v;
    const uint32_t* small_n;
    const float* small_lr;
    const uint32_t* small_step;
    /* bit 0: data parallel -- the table's gradient is SUMMED INTO the dense buffer table_grad (grid_encode_backward's
     * own flush, no record lists left behind) and no optimizer runs: the caller averages table_grad and the buffers
     * behind dwseg_* over the ranks (torch.distributed over RCCL: enerf_amd/trainer.py) and steps the optimizer itself.
     * bit 1 (with bit 0, enerf_grid_owner_range set): the sharded tail that keeps this rank's slice as record lists -- the
     * backward defers, flushing only the other slices into table_grad; the caller reduce-scatters, runs
     * enerf_grid_adam_from_records_ex and all-gathers.
     * bit 2: ENERF_STEP_EVERY_ROW.  (ABI 2 .. 6: unused, after the tail on the library's own RCCL communicator went.)
     * report: written by the library -- zeroed at entry, ENERF_STEP_* report bits set before a call returns 0. */
    uint32_t flags, report;
} enerf_train_step_args;
int enerf_train_step_mse(enerf_train_step_args* args);
/* Development aid: host microseconds enerf_train_step_mse spends in each of its calls (in call order, 16 slots, averaged
 * over the steps since timing was switched on); on >= 0 switches the timers (and clears them), on < 0 only reads. */
int enerf_debug_step_timing(int on, double* out16);
/* enerf_train_step_mse builds the fused MLP's operand fragments inside its grid forward's launch (sixteen extra
 * workgroups) instead of a launch of their own; on = 0 switches that off (testing aid; < 0 only reads).  Returns the
 * previous setting. */
int enerf_debug_carry_frags(int on);
/* ... and leaves the fused MLP backward's weight-gradient partial sums to the optimizer's launch, which sums them for its
 * small tensors (no k_mlp32_reduce_w2 launch in between; the sums land in the gradient tensors all the same); on = 0
 * switches that off (testing aid; < 0 only reads).  Returns the previous setting. */
int enerf_debug_fold_reduce(int on);
/* ... and marches the NEXT batch without a second stream: the march's count pass rides in the table optimizer's launch
 * (extra workgroups; enerf_debug_march_carry_blocks sets how many, 0 = two per compute unit), its scan + write are one launch
 * behind it on the step's own stream -- no cross-stream signal behind the MLP backward, no event wait at the head of the next
 * step.  Same samples, same offsets.  Served where the wave-per-ray fixed-step marcher is (dt_gamma = 0, at most 16384 rays)
 * and the call asks for no count mirror (next_count_host); everything else keeps the side-stream march.  on = 0 switches
 * it off (-1 only reads).  Returns the previous setting; on = -2 returns the number of steps marched that way so far (a
 * test's counter: a caller learns where its march ran from the call's own `report`). */
int enerf_debug_carry_count(int on);
int enerf_debug_march_carry_blocks(uint32_t blocks);

/* The event-only step (Trainer.train_step_events, nerf/utils.py:482-546, event_only = 1; C_thres == -1, the normalised
 * loss, with the caller's weight of 20 in `upstream`) the same way: TWO
 * renders -- the event pairs' rays at the two poses -- blended with one background colour, the event loss on the two
 * images and its gradient (enerf_event_loss_fwd_bwd), both renders' backward, ONE optimizer pass; optionally the two
 * marches of the next step on `side_stream` behind the second render's MLP backward.  Calls, in order (what
 * enerf_amd/events.train_step_events_manual + FusedAdam.step_grid_table issue): per render grid_encode_forward,
 * mlp32_forward_p x 2, composite_rays_train_forward_blend; event_loss_fwd_bwd; per render
 * composite_rays_train_backward_mse(target = NULL), mlp32_backward_p x 2 (the second render's weight gradients are
 * added to the first's), grid_encode_backward_ex(defer, reserve = M1 + M2); grid_adam_from_records_ex.
 * As in enerf_train_step_mse, the grid and MLP launches take their valid rows from the renders' own `counter` fields and
 * their arithmetic from `mlp_precision`: no process-wide request is consumed or cleared. */
typedef struct enerf_step_render {
    uint32_t N, M;                      /* rays, sample rows budgeted (counter[0] real) */
    const float *xyzs, *dirs, *deltas;
    const int32_t *rays, *counter;
    /* scratch, fp32 (shapes as in enerf_train_step_args; g_image [N,out_c] receives d loss / d out_image) */
    float *feats, *h32, *fb_s, *fb_c, *sigma, *rgb, *weights_sum, *image, *out_image, *g_image, *g_sigmas, *g_rgbs, *dx32,
        *dfeat;
    /* the next step's march of this render's rays (next_rays_o == NULL: none) */
    const float *next_rays_o, *next_rays_d;
    uint32_t next_N, next_M;
    float *next_nears, *next_fars, *next_xyzs, *next_dirs, *next_deltas;
    int32_t *next_rays, *next_counter;
} enerf_step_render;
typedef struct enerf_event_step_args {
    uint32_t struct_bytes;              /* sizeof(enerf_event_step_args): checked */
    int mlp_precision;
    enerf_stream_t stream, side_stream;
    enerf_step_render r[2];
    const float* bg_color;              /* [out_c] device floats: one colour for both renders (nerf/utils.py:497) */
    const float* pols;                  /* [N] */
    uint32_t use_luma, linlog;
    float C_thres, log_thres, upstream;
    float *delta, *loss;                /* [N,1] (use_luma, out_c = 3) or [N,out_c]; device scalar (written, may be NULL) */
    /* networks, march parameters, optimizer: as in enerf_train_step_args */
    const float* embeddings;
    const int32_t* offsets;
    float level_scale_log2, bound, inv_two_bound;
    uint32_t base_resolution, gridtype;
    const float* const* wseg_s;
    const float* const* wseg_c;
    float* const* dwseg_s;
    float* const* dwseg_c;
    uint32_t nh_s, nh_c, w0_cols_c, out_c;
    const float* aabb;
    const uint8_t* bitfield;
    float min_near, dt_gamma;
    uint32_t cascade, grid_size, max_steps, perturb, march_flags, reserved0;
    float *table, *table_grad, *table_m, *table_v;
    float lr, beta1, beta2, eps;
    uint32_t table_step, n_small;
    float* const* small_p;
    const float* const* small_g;
    float* const* small_m;
    float* const* small_v;
    const uint32_t* small_n;
    const float* small_lr;
    const uint32_t* small_step;
    /* flags bit 1: MERGED layout.  Both renders have the same M, r[1].xyzs / dirs / deltas are the M rows that follow
     * r[0]'s in one buffer, and the m_* pointers hold scratch for 2 M rows (shapes of the per-render scratch with 2 M
     * for M).  Then grid_encode_forward, the four mlp32 launches, grid_encode_backward run ONCE over the 2 M rows (rows
     * [counter0, M) are padding whose gradients the first render's composite backward zero-fills; the MLP kernels take
     * M + min(counter1, M) as their valid-row count: enerf_mlp32_valid_rows_ex's rule); compositing and its backward stay per
     * render, on the halves.  Same per-sample values; the weight gradients are summed over both renders in one pass
     * instead of two passes added.
     * flags bit 2: ENERF_STEP_EVERY_ROW.  report: as in enerf_train_step_args. */
    uint32_t flags, report;
    float *m_feats, *m_h32, *m_fb_s, *m_fb_c, *m_sigma, *m_rgb, *m_g_sigmas, *m_g_rgbs, *m_dx32, *m_dfeat;
} enerf_event_step_args;
int enerf_train_step_events(enerf_event_step_args* args);

/* profiling aid: restrict grid_encode_forward/backward to the levels whose bit is set (default all) */
int enerf_debug_grid_level_mask(uint32_t mask);
/* Testing / profiling aid: route of grid_encode_forward_sweep.  0 (default): the static balanced schedule over the XCD
 * pairs with the coarse levels 0 .. walk-1 taken by one thread per point (walk 0, 4 or 5; default 5); 1: the whole-level
 * snake deal of the training forward. */
int enerf_debug_sweep_route(uint32_t route, uint32_t walk);
/* Testing aid: the sweep schedule of L levels of `nchunks` 256-point chunks as (XCD pair, unit, first chunk, chunks)
 * rows, unit = level or 0x80000000 (the walker).  Returns the number of rows (at most `cap`), -1 on error. */
int enerf_debug_sweep_schedule(uint32_t L, uint32_t walk, uint32_t nchunks, uint32_t* out, uint32_t cap);
/* Testing / profiling aid: fp32 grid_encode_backward batches of at least `min_batch` samples send the levels spanning
 * at least `min_tiles` 128-KiB tiles through the binned path (per-tile record lists summed in LDS, no global float
 * atomics); everything else takes the global-atomic kernel.  Defaults 16384 / 8. */
int enerf_debug_grid_bwd_binned(uint32_t min_batch, uint32_t min_tiles);

/* ------------------------------------------------------------------ measurement hooks (not in the reference)
 * When enabled, every launch of the selected kernel family is bracketed by hipEvents on its own stream so that
 * bench.py can report the average launch duration of the dominant kernel (roofline.achieved). */
#define ENERF_K_GRID_FWD 0
#define ENERF_K_GRID_BWD 1
#define ENERF_K_MARCH_TRAIN 2
#define ENERF_K_COMPOSITE_FWD 3
#define ENERF_K_COMPOSITE_BWD 4
#define ENERF_K_SH_FWD 5
#define ENERF_K_FFMLP_FWD 6
#define ENERF_K_FFMLP_BWD 7
#define ENERF_K_MARCH_INFER 8
#define ENERF_K_COMPOSITE_INFER 9
#define ENERF_K_TABLE_ADAM 10 /* enerf_grid_adam_from_records[_ex]: table flush + table Adam (+ the small tensors) */
#define ENERF_K_MLP_REDUCE 11 /* the weight-gradient reduce launch of enerf_mlp32_backward[_p] */
#define ENERF_K_COUNT 12

/* Measurement aid: samples reserved (counter[0] increments) by all enerf_march_rays_train[_ex] calls of this process
 * since the last reset, kept on the device by the march's own scan pass.  Synchronises `stream`, then reads (total may
 * be NULL) and optionally resets. */
int enerf_march_train_samples(uint64_t* total, int reset, enerf_stream_t stream);
int enerf_prof_enable(int on);
/* bit k of `mask` enables timing of kernel family k only (each timed call costs two event records on the stream) */
int enerf_prof_enable_mask(uint32_t mask);
int enerf_prof_reset(void);
/* Time one eligible call in `n` per kernel family (default 1: every call).  A timed launch carries completion signals
 * (and, for kernel-stamped families, a one-wavefront marker launch before it): ~10 us of queue time per timed call, so a
 * benchmark that must not perturb what it measures samples.  enerf_prof_read_units: the work units (grid_encode: points;
 * mlp32: samples) of the TIMED calls only -- the denominator that goes with enerf_prof_read's time -- and the number of
 * eligible calls seen since the last reset. [host ptrs] */
int enerf_prof_sample_every(uint32_t n);
int enerf_prof_read_units(int kernel_id, double* units, uint64_t* calls_seen);
/* Synchronises the recorded events; returns total milliseconds and launch count for `kernel_id`. [host ptrs] */
int enerf_prof_read(int kernel_id, double* total_ms, uint64_t* launches);

/* ------------------------------------------------------------------ stratified sampler (cuda_ray off)
 * NeRFRenderer.run with upsample_steps = 0 (nerf/renderer.py:150-278; enerf_amd/sampler.py), csrc/stratified.hip.  One
 * wavefront per ray; N rays of T samples, sample s = n * T + k; all float tensors fp32, contiguous.
 *
 * points: near / far of every ray (enerf_near_far_from_aabb's arithmetic) into nears / fars [N], the depths z [N,T]
 * (torch.linspace(0, 1, T) on the device, with step lin_step = 1 / (T - 1) rounded to fp32, near + (far - near) * g, plus
 * (u - 0.5) * width when u [N,T] is given; width = (far - near) * inv_T) and the points clamped to the box, xyz [N*T,3]:
 * bit-equal with sampler.stratified_depths + sampler._points. */
int enerf_stratified_points(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, uint32_t T,
                            float min_near, float lin_step, float inv_T, const float* u, float* nears, float* fars,
                            float* z, float* xyz, enerf_stream_t stream);
/* weights: alpha = 1 - exp(-step * density_scale * sigma) (step: next depth minus this one, the last one width),
 * w = alpha * exclusive product of (1 - alpha + 1e-15) [N,T], opacity = sum w [N], depth = sum w * clamp((z - near) /
 * (far - near), 0, 1) [N], count [N] = samples with w > 1e-4 per ray.  The compact list of masked samples is ordered by
 * ray, then depth; its offsets are the inclusive scan `incl` of count (int32, on the device: incl[N-1] is its length). */
int enerf_stratified_weights(const float* z, const float* sigma, const float* nears, const float* fars, uint32_t N,
                             uint32_t T, float inv_T, float density_scale, float* w, float* opacity, float* depth,
                             int32_t* count, enerf_stream_t stream);
/* The colour net's input rows of the compact list, cin [cap,32] (cap >= N*T): [0 | h16[s,1..15] | SH4(rays_d[n])] -- the
 * row order enerf_mlp32_*_p read with w0_cols 31, nerf_perm 1.  h16 [N*T,16]: the sigma net's outputs.  Rows incl[N-1]
 * up to the next multiple of 32 are zeroed (the MLP kernels' valid-row count covers whole 32-row tiles). */
int enerf_stratified_color_input(const float* w, const int32_t* incl, const int32_t* count, const float* h16,
                                 const float* rays_d, uint32_t N, uint32_t T, uint32_t cap, float* cin,
                                 enerf_stream_t stream);
/* image [N,C] = sum over masked samples of w * rgb + (1 - opacity) * bg; rgb [cap,C] by compact row; bg [C]
 * (bg_per_ray 0) or [N,C] (bg_per_ray 1); C = 1..3. */
int enerf_stratified_composite_forward(const float* w, const int32_t* incl, const int32_t* count, const float* opacity,
                                       const float* rgb, const float* bg, uint32_t bg_per_ray, uint32_t N, uint32_t T,
                                       uint32_t C, float* image, enerf_stream_t stream);
/* From g_image [N,C] and g_depth [N] (NULL: depth takes no part in the loss): g_sigma [N*T] for every sample and g_rgb
 * [cap,C] for the compact rows (the rows up to the next multiple of 32 zeroed).  No division by 1 - alpha + 1e-15. */
int enerf_stratified_composite_backward(const float* g_image, const float* g_depth, const float* z, const float* sigma,
                                        const float* w, const float* nears, const float* fars, const int32_t* incl,
                                        const int32_t* count, const float* rgb, const float* bg, uint32_t bg_per_ray,
                                        uint32_t N, uint32_t T, uint32_t C, float inv_T, float density_scale,
                                        uint32_t cap, float* g_sigma, float* g_rgb, enerf_stream_t stream);
/* dh16 [N*T,16]: columns 0..15 of the colour net's input gradient dx [cap,32] (nerf_perm layout: 1..15 are geo_feat) at
 * the masked samples' rows, zero elsewhere -- the sigma net's output gradient (its backward replaces column 0 by
 * dsigma * exp(clamp(h0, -15, 15))). */
int enerf_stratified_scatter_geo_grad(const float* w, const int32_t* incl, const int32_t* count, const float* dx,
                                      uint32_t N, uint32_t T, float* dh16, enerf_stream_t stream);
/* The same four with the storage of cin / rgb / g_rgb / dx chosen by `storage`: ENERF_F32 (the forms above) or ENERF_F16
 * (the fp16 regime: cin [cap,32] and dx [cap,32] half, 64 B per row; rgb and g_rgb [cap,C] half; g_rgb = g_image * w
 * rounded to half).  In ENERF_F16 the directions are rounded to half before the SH basis, which is evaluated in fp32 on
 * them and stored as half (enerf_sh_encode_forward's ENERF_F16 values).  Everything else stays fp32. */
int enerf_stratified_color_input_ex(const float* w, const int32_t* incl, const int32_t* count, const float* h16,
                                    const float* rays_d, uint32_t N, uint32_t T, uint32_t cap, void* cin, uint32_t storage,
                                    enerf_stream_t stream);
int enerf_stratified_composite_forward_ex(const float* w, const int32_t* incl, const int32_t* count,
                                          const float* opacity, const void* rgb, const float* bg, uint32_t bg_per_ray,
                                          uint32_t N, uint32_t T, uint32_t C, float* image, uint32_t storage,
                                          enerf_stream_t stream);
int enerf_stratified_composite_backward_ex(const float* g_image, const float* g_depth, const float* z, const float* sigma,
                                           const float* w, const float* nears, const float* fars, const int32_t* incl,
                                           const int32_t* count, const void* rgb, const float* bg, uint32_t bg_per_ray,
                                           uint32_t N, uint32_t T, uint32_t C, float inv_T, float density_scale,
                                           uint32_t cap, float* g_sigma, void* g_rgb, uint32_t storage,
                                           enerf_stream_t stream);
int enerf_stratified_scatter_geo_grad_ex(const float* w, const int32_t* incl, const int32_t* count, const void* dx,
                                         uint32_t N, uint32_t T, float* dh16, uint32_t storage, enerf_stream_t stream);

/* ------------------------------------------------------------------ mesh export
 * Trainer.save_mesh (nerf/utils.py:219-249, 712-732), csrc/mesh.hip; semantics in enerf_amd/mesh.py and DESIGN.md 4.10.
 * R (lattice points per axis) must be 2 .. 512.  The field u [R,R,R] is fp32, x slowest.
 *
 * lattice: the points of x-planes [x0, x0 + nx) in field order, pts [nx*R*R, 3] fp32.  box [host]: lo[3], hi[3], step[3]
 * with step = (hi - lo) / (R - 1) in fp32; coordinate i = fmaf(i, step, lo) for i < R / 2, else
 * fmaf(-(R - 1 - i), step, hi): torch.linspace(lo, hi, R) on the CPU, bit for bit. */
int enerf_mesh_lattice(const float* box, uint32_t R, uint32_t x0, uint32_t nx, float* pts, enerf_stream_t stream);
/* Marching cubes in two calls around one read-back.  workspace: bytes of `ws` for R [host ptr].  count: classifies every
 * point and cell and scans the counts; totals [3] int64 (device) = vertices, triangles, non-finite values of u.  emit (the
 * same u, threshold and ws, V and F as counted; nothing is written when u held a non-finite value and the caller stopped):
 * verts [V,3] fp64 in index space, tris [F,3] int32, in the order and with the table of mc_tables.h. */
int enerf_marching_cubes_workspace(uint32_t R, uint64_t* bytes);
int enerf_marching_cubes_count(const float* u, uint32_t R, double threshold, void* ws, int64_t* totals,
                               enerf_stream_t stream);
int enerf_marching_cubes_emit(const float* u, uint32_t R, double threshold, void* ws, uint64_t V, uint64_t F,
                              double* verts, int32_t* tris, enerf_stream_t stream);

/* ------------------------------------------------------------------ evaluation metrics
 * Trainer.evaluate_one_epoch (nerf/utils.py:44-92, 1028-1293), csrc/eval_metrics.hip; semantics in enerf_amd/evaluate.py
 * and DESIGN.md 4.11.  V views of H x W pixels (H, W >= 7), C = 1 or 3 channels, fp32, stacked [V, H, W, C].  Every
 * call writes its per-view results into res [V, ENERF_EVAL_COLS] fp64 (device), one column group per call, through
 * per-workgroup partials in `ws` and a fixed-order second pass: no atomics, the same bits on every run.
 *
 * workspace: bytes of `ws` for V, H, W [host ptr]; one workspace serves the three calls in turn on one stream.
 * stats: column 0 = sum over H*W*C of (pred - gt)^2 (the difference in fp32, squared and summed in fp64); log_mode != 0
 *   adds columns 1..4 = the sums of x, y, x^2, xy with x = log(255 l(pred) + 1e-3), y = the same of gt in fp32, l = the
 *   pixel (C = 1) or its esim luma (C = 3).
 * correct (after stats with log_mode): ab [2] (device) = a, b of the least-squares fit of y on [1, x] over all V views
 *   (fp64; a NaN becomes 5); pred_cor = exp(a x + b), gt_j = l(255 gt) as [V, H, W] fp32 planes; column 5 = the sum of
 *   (gt_j - pred_cor)^2.
 * ssim: column 6 = the mean over the (H - 6) x (W - 6) interior of skimage's SSIM map (7 x 7 uniform window, sample
 *   covariance, K1 = 0.01, K2 = 0.03) of the planes x and y, read at pixel stride `stride` (1 .. 4) from [V, H, W, stride]. */
#define ENERF_EVAL_COLS 7
#define ENERF_EVAL_COL_SSE_COR 5
#define ENERF_EVAL_COL_SSIM 6
int enerf_eval_workspace(uint32_t V, uint32_t H, uint32_t W, uint64_t* bytes);
int enerf_eval_stats(const float* pred, const float* gt, uint32_t V, uint32_t H, uint32_t W, int C, int log_mode,
                     void* ws, double* res, enerf_stream_t stream);
int enerf_eval_correct(const float* pred, const float* gt, uint32_t V, uint32_t H, uint32_t W, int C, void* ws,
                       double* res, double* ab, float* pred_cor, float* gt_j, enerf_stream_t stream);
int enerf_eval_ssim(const float* x, const float* y, uint32_t V, uint32_t H, uint32_t W, uint32_t stride,
                    double data_range, void* ws, double* res, enerf_stream_t stream);

/* ------------------------------------------------------------------ frame batches and the error map
 * The frame side of the reference's collate (nerf/utils.py:111-174 get_rays, provider.py:645-663) and the error-map
 * write-back of Trainer.train_step (nerf/utils.py:610-632), csrc/frame_batch.hip; semantics in enerf_amd/frame_sampler.py
 * and DESIGN.md 4.12.  Every operation below is rounded to fp32 on its own (the library is built with -ffp-contract=off).
 *
 * frame_batch: one thread per ray.  poses [V,4,4] fp32 cam2world, view < V; pixel p = inds[k] (inds == NULL: p = k, and
 *   N must be H*W); i = p % W, j = p / W; x = (i - cx) / fx, y = (j - cy) / fy; d = (x, y, 1) / sqrt(x^2 + y^2 + 1);
 *   rays_d[k] = R d, rays_o[k] = t of poses[view]; target[k, :] = images[view, p, :] with images [V,H,W,Ci] fp32,
 *   Ci in 1..4 (images == NULL: target is not written).  A pixel outside [0, H*W) reads nothing and gives NaN rows.
 * error_map_sample: ONE workgroup, the ENERF_ERROR_MAP_CELLS cells sorted in LDS.  weights, e fp32 [16384];
 *   key_c = weights[c] > 0 ? weights[c] / e[c] : 0 (IEEE fp32; e[c] == 0 gives +inf); the N <= 16384 cells of the largest
 *   key, ties to the smaller cell index, go to inds_coarse i64 [N] in that order: sampling without replacement with
 *   probability proportional to the weights when e holds independent Exp(1) draws.  Cells of weight <= 0 sort last and
 *   are taken only when fewer than N cells are positive (torch.multinomial raises there).  weights == NULL: inds_coarse
 *   is read instead of written (the selection is skipped).  Then, with r = c / 128, q = c % 128, sx = fp32(H / 128.0),
 *   sy = fp32(W / 128.0): row = min((int64)(fp32(r) sx + u_row[k] sx), H - 1), col likewise with q, sy, u_col, W - 1;
 *   inds[k] = row W + col, i64 [N].  u_row, u_col fp32 [N] in [0, 1).
 * error_map_update: one thread per ray; map[inds_coarse[k]] = fp32(0.1) map[inds_coarse[k]] + fp32(0.9) err[k] on the
 *   view's row map [16384].  inds_coarse must hold no duplicates (it comes from the selection above): no atomics.  A
 *   cell outside [0, 16384) is skipped. */
#define ENERF_ERROR_MAP_CELLS 16384
int enerf_frame_batch(const float* poses, uint32_t V, uint32_t view, float fx, float fy, float cx, float cy, uint32_t H,
                      uint32_t W, const int64_t* inds, uint32_t N, const float* images, uint32_t Ci, float* rays_o,
                      float* rays_d, float* target, enerf_stream_t stream);
int enerf_error_map_sample(const float* weights, const float* e, const float* u_row, const float* u_col, uint32_t N,
                           uint32_t H, uint32_t W, int64_t* inds_coarse, int64_t* inds, enerf_stream_t stream);
int enerf_error_map_update(float* map, const int64_t* inds_coarse, const float* err, uint32_t N, enerf_stream_t stream);
/* error_map_sample's sorting network and pixel mapping run on the HOST, thread by thread, on host pointers (tests without
 * a GPU hold the network to the statement with it). */
int enerf_debug_error_map_sample_host(const float* weights, const float* e, const float* u_row, const float* u_col,
                                      uint32_t N, uint32_t H, uint32_t W, int64_t* inds_coarse, int64_t* inds);

/* ------------------------------------------------------------------ display frames
 * What the reference does on the host between a rendered fp32 frame and what is shown or written (nerf/utils.py:768-804
 * Trainer.test, :870-918 test_gui, nerf/gui.py:119-149, scripts/render.py:489-509), csrc/view_finish.hip; semantics in
 * enerf_amd/view.py and DESIGN.md 4.15.  Every fp32 operation below is rounded on its own (-ffp-contract=off).
 *
 * view_finish: ONE launch, one thread per output pixel, no intermediate in memory.  image fp32 [h*w, C] (C in 1..3), depth
 *   fp32 [h*w] or NULL; the output is H x W.  Per output pixel (y, x) and channel:
 *     1. source pixel: row = min((int)floorf(y * s_h), h - 1) with s_h = (float)h / (float)H, the column likewise: the
 *        index of F.interpolate(mode="nearest", size=(H, W)) (the identity when (h, w) == (H, W));
 *     2. minmax != NULL (device, fp32 [2] = min, max): v = max == min ? 0 : (v - min) / (max - min);
 *     3. flags & ENERF_VIEW_LINEAR: v = v < 0.0031308 ? 12.92 v : 1.055 powf(v, 0.41666) - 0.055   (linear_to_srgb);
 *     4. accum != NULL (fp32 [H*W, C], read and written): a = spp == 0 ? v : (a (float)spp + v) / (float)(spp + 1),
 *        stored back, and v = a from here on (the GUI's running mean in numpy fp32); out_f32 may be accum itself (the
 *        running buffer is then the fp32 result and is written once);
 *     5. out_f32 [H*W, C] = v; out_u8 [H*W, C] = (uint8) of v * 255 clamped to [0, 255], truncated; NaN gives 0.
 *   depth_f32 [H*W] / depth_u8 [H*W] take steps 1 and 5 only.  Every output pointer may be NULL.  Bad arguments: C outside
 *   1..3; H*W == 0 together with a non-NULL output; accum with neither out_f32 nor out_u8; a depth output without depth;
 *   an image of 0 or more than 2^30 pixels.
 * view_minmax: minmax [2] (device) = the smallest and largest of the n image values, NaNs skipped; (0, 1) when there is
 *   none.  Two launches (per-workgroup partials in ws, fp32 [ENERF_VIEW_MINMAX_WS] on the device, then one workgroup over
 *   them), nothing is read back. */
#define ENERF_VIEW_LINEAR 1u
#define ENERF_VIEW_MINMAX_WS 512
int enerf_view_finish(const float* image, const float* depth, uint32_t h, uint32_t w, uint32_t C, uint32_t H, uint32_t W,
                      uint32_t flags, const float* minmax, float* accum, uint32_t spp, float* out_f32, uint8_t* out_u8,
                      float* depth_f32, uint8_t* depth_u8, enerf_stream_t stream);
int enerf_view_minmax(const float* image, uint64_t n, float* ws, float* minmax, enerf_stream_t stream);

/* ------------------------------------------------------------------ background model (bg_radius > 0)
 * nerf/network.py `background` behind raymarching.polar_from_ray, csrc/background.hip; DESIGN.md 4.21.  Per ray:
 *   p = enerf_polar_from_ray's pair (the same arithmetic);  grid = the D = 2, level_dim 2 encoder of (p + 1) / 2 over
 *   `embeddings` [offsets[L], 2] fp32, level geometry (offsets [L + 1] on the device, S, H, gridtype) as
 *   enerf_grid_encode_forward takes it;  sh = the 16 values of enerf_sh_encode_forward(degree 4) of rays_d, or zeros when
 *   use_dirs == 0;  bg = sigmoid(W1 relu(W0 [sh | grid])), w0 [64, 16 + 2L] and w1 [C, 64] row-major as nn.Linear.weight.
 * forward: ONE launch, bg [N, C].  trace (NULL in production) receives [N, 2 + 16 + 2L]: p and the MLP's input row.
 * backward: one launch plus one small reduce over its workgroups' sums.  g_bg = (1 - weights_sum[n]) * grad_image
 *   [N, C] (weights_sum NULL: the factor is 1); the forward is recomputed from the rays.  grad_w0 [64, 16 + 2L] and grad_w1
 *   [C, 64] are WRITTEN, summed in a fixed order (the same bits on every run); grad_embeddings [offsets[L], 2] is ADDED
 *   into with float atomics (the caller zero-fills it; its last bits depend on arrival order).
 * Both: C outside 1..3, hidden != 64, level_dim != 2, L outside 1..8 or a NULL pointer other than trace / weights_sum
 * answer ENERF_E_BADARG and write nothing; N == 0 returns 0 and touches nothing. */
int enerf_background_forward(const float* rays_o, const float* rays_d, float radius, uint32_t N, const float* embeddings,
                             const int32_t* offsets, uint32_t L, uint32_t level_dim, float S, uint32_t H, uint32_t gridtype,
                             uint32_t use_dirs, const float* w0, const float* w1, uint32_t hidden, uint32_t C, float* bg,
                             float* trace, enerf_stream_t stream);
int enerf_background_backward(const float* rays_o, const float* rays_d, float radius, uint32_t N, const float* embeddings,
                              const int32_t* offsets, uint32_t L, uint32_t level_dim, float S, uint32_t H,
                              uint32_t gridtype, uint32_t use_dirs, const float* w0, const float* w1, uint32_t hidden,
                              uint32_t C, const float* grad_image, const float* weights_sum, float* grad_w0, float* grad_w1,
                              float* grad_embeddings, enerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ENERF_HIP_H */
