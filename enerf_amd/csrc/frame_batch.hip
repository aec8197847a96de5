// frame_batch.hip -- the frame side of the reference's collate and its --error_map option for gfx950: get_rays
// (nerf/utils.py:111-174) with the image gather of provider.py:645-663, the weighted cell selection of its error_map
// branch, and the error map's EMA write-back in Trainer.train_step (nerf/utils.py:610-632).  The semantics are written out
// in enerf_amd/frame_sampler.py (whose torch statements are the CPU path and the tests' reference) and DESIGN.md 4.12.
//
//   k_frame_batch        one thread per ray: pixel -> unit camera direction -> rays_d = R d, rays_o = t, target = the
//                        pixel's Ci channels.  No H*W-sized temporary: the pixel grid is never materialised.
//   k_error_map_sample   ONE workgroup of 1024 threads.  Each of the 16384 cells becomes a 64-bit composite (its key
//                        weight / e as order-preserving bits above, 16383 - cell below: equal keys order by the smaller
//                        cell) and the composites are sorted, largest first, by a bitonic network in LDS; then thread k
//                        maps the k-th cell to its jittered pixel.  A pass of the network resolves up to four of a
//                        stage's compare distances at once: a thread holds the 16 elements that differ in those four index
//                        bits in registers, so the 105 compare steps of 16384 elements take 32 passes over the LDS.  The
//                        array is padded by one element per 16 so that the pass over the four lowest bits (lanes 16
//                        elements apart) does not put a wave's lanes on two banks.
//   k_error_map_pixels   the pixel mapping alone, from given cells (the selection is the caller's)
//   k_error_map_update   one thread per ray: the EMA of the view's row at the sampled cells
//
// Compiled with -ffp-contract=off: every product and every sum below is rounded to fp32 on its own, as the element-wise
// torch kernels of the statement do.
#include <math.h>

#include "common.h"

using namespace enerf;

namespace {

constexpr int kThreads = 256;
constexpr int kCells = ENERF_ERROR_MAP_CELLS;   // 128 x 128
constexpr int kCellsLog2 = 14;
constexpr int kSide = 128;
constexpr int kSortThreads = 1024;
constexpr int kPadShift = 4;                    // one element of padding per 16
constexpr int kPadded = kCells + (kCells >> kPadShift);

static_assert((1 << kCellsLog2) == kCells && kSide * kSide == kCells, "the error map is 128 x 128 cells");
static_assert(kPadded * sizeof(uint64_t) <= 160 * 1024, "the composites must fit the CU's 160 KiB of LDS");

__host__ __device__ __forceinline__ uint32_t padded(uint32_t i) { return i + (i >> kPadShift); }

// One group of a pass of the bitonic network in stage `k` (a power of two: runs of k elements are being merged): the
// 2^NB elements whose indices differ only in bits lo .. lo + NB - 1, compare distances 2^(lo+NB-1) down to 2^lo.
// Largest first overall: a pair is ordered descending where its index has bit k clear.  Groups touch disjoint elements.
template <int NB>
__host__ __device__ __forceinline__ void sort_group(uint64_t* a, uint32_t g, int lo, uint32_t k) {
    constexpr int CNT = 1 << NB;
    const uint32_t base = ((g >> lo) << (lo + NB)) | (g & ((1u << lo) - 1u));
    const bool desc = (base & k) == 0;
    uint64_t v[CNT];
#pragma unroll
    for (int r = 0; r < CNT; ++r) v[r] = a[padded(base | ((uint32_t)r << lo))];
#pragma unroll
    for (int b = NB - 1; b >= 0; --b) {
#pragma unroll
        for (int r = 0; r < CNT; ++r) {
            if ((r >> b) & 1) continue;
            const int p = r | (1 << b);
            const uint64_t x = v[r], y = v[p];
            const bool sw = desc ? x < y : x > y;
            v[r] = sw ? y : x;
            v[p] = sw ? x : y;
        }
    }
#pragma unroll
    for (int r = 0; r < CNT; ++r) a[padded(base | ((uint32_t)r << lo))] = v[r];
}

// thread `tid` of `threads`: its share of the pass of stage k over index bits lo .. lo + nb - 1 (nb in 1 .. 4)
__host__ __device__ __forceinline__ void sort_pass(uint64_t* a, uint32_t tid, uint32_t threads, int lo, int nb,
                                                   uint32_t k) {
    const uint32_t groups = (uint32_t)kCells >> nb;
    for (uint32_t g = tid; g < groups; g += threads) {
        switch (nb) {
            case 4: sort_group<4>(a, g, lo, k); break;
            case 3: sort_group<3>(a, g, lo, k); break;
            case 2: sort_group<2>(a, g, lo, k); break;
            default: sort_group<1>(a, g, lo, k); break;
        }
    }
}

// the cell's key and index as one unsigned word whose order is (key descending, cell ascending) when sorted largest first
__host__ __device__ __forceinline__ uint64_t composite(float w, float e, uint32_t c) {
    float key = w > 0.0f ? w / e : 0.0f;
    if (key == 0.0f) key = 0.0f;                // (-0 and +0 are one key)
    union {
        float f;
        uint32_t u;
    } bits;
    bits.f = key;
    const uint32_t b = (bits.u & 0x80000000u) ? ~bits.u : (bits.u | 0x80000000u);      // float order -> unsigned order
    return ((uint64_t)b << 32) | (uint32_t)(kCells - 1 - c);
}

__host__ __device__ __forceinline__ uint32_t composite_cell(uint64_t v) { return (uint32_t)(kCells - 1) - (uint32_t)v; }

// get_rays lines 145-149: cell c, jitters (u_row, u_col) -> pixel index row * W + col
__host__ __device__ __forceinline__ int64_t cell_to_pixel(int64_t c, float u_row, float u_col, float sx, float sy,
                                                          uint32_t H, uint32_t W) {
    const float r = (float)(c / kSide), q = (float)(c % kSide);
    const float fr = r * sx + u_row * sx;       // (two products and a sum, each rounded: -ffp-contract=off)
    const float fq = q * sy + u_col * sy;
    int64_t row = (int64_t)fr, col = (int64_t)fq;
    row = row > (int64_t)H - 1 ? (int64_t)H - 1 : (row < 0 ? 0 : row);
    col = col > (int64_t)W - 1 ? (int64_t)W - 1 : (col < 0 ? 0 : col);
    return row * (int64_t)W + col;
}

__global__ void __launch_bounds__(kThreads) k_frame_batch(const float* __restrict__ pose, float fx, float fy, float cx,
                                                          float cy, uint32_t H, uint32_t W,
                                                          const int64_t* __restrict__ inds, uint32_t N,
                                                          const float* __restrict__ image, uint32_t Ci,
                                                          float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                          float* __restrict__ target) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= N) return;
    const int64_t p = inds ? inds[k] : (int64_t)k;
    float* o = rays_o + (size_t)k * 3;
    float* d = rays_d + (size_t)k * 3;
    if (p < 0 || p >= (int64_t)H * (int64_t)W) {        // not a pixel: nothing is read for it
        for (int a = 0; a < 3; ++a) o[a] = d[a] = NAN;
        if (image)
            for (uint32_t c = 0; c < Ci; ++c) target[(size_t)k * Ci + c] = NAN;
        return;
    }
    const float i = (float)(uint32_t)(p % W), j = (float)(uint32_t)(p / W);
    const float x = (i - cx) / fx, y = (j - cy) / fy;
    const float n = sqrtf((x * x + y * y) + 1.0f);
    const float dx = x / n, dy = y / n, dz = 1.0f / n;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d[a] = (pose[4 * a + 0] * dx + pose[4 * a + 1] * dy) + pose[4 * a + 2] * dz;
        o[a] = pose[4 * a + 3];
    }
    if (image) {
        const float* src = image + (size_t)p * Ci;
        for (uint32_t c = 0; c < Ci; ++c) target[(size_t)k * Ci + c] = src[c];
    }
}

__global__ void __launch_bounds__(kSortThreads) k_error_map_sample(const float* __restrict__ weights,
                                                                   const float* __restrict__ e,
                                                                   const float* __restrict__ u_row,
                                                                   const float* __restrict__ u_col, uint32_t N, float sx,
                                                                   float sy, uint32_t H, uint32_t W,
                                                                   int64_t* __restrict__ inds_coarse,
                                                                   int64_t* __restrict__ inds) {
    __shared__ uint64_t cells[kPadded];
    const uint32_t tid = threadIdx.x;
    for (uint32_t c = tid; c < (uint32_t)kCells; c += kSortThreads) cells[padded(c)] = composite(weights[c], e[c], c);
    __syncthreads();
    for (int s = 1; s <= kCellsLog2; ++s) {
        const uint32_t k = 1u << s;             // (s == 14: bit k is clear in every index -- the last merge is descending)
        for (int hi = s - 1; hi >= 0; hi -= 4) {
            const int lo = hi >= 3 ? hi - 3 : 0;
            sort_pass(cells, tid, kSortThreads, lo, hi - lo + 1, k);
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < N; i += kSortThreads) {
        const int64_t c = (int64_t)composite_cell(cells[padded(i)]);
        inds_coarse[i] = c;
        inds[i] = cell_to_pixel(c, u_row[i], u_col[i], sx, sy, H, W);
    }
}

__global__ void __launch_bounds__(kThreads) k_error_map_pixels(const int64_t* __restrict__ inds_coarse,
                                                               const float* __restrict__ u_row,
                                                               const float* __restrict__ u_col, uint32_t N, float sx,
                                                               float sy, uint32_t H, uint32_t W,
                                                               int64_t* __restrict__ inds) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    int64_t c = inds_coarse[i];
    c = c < 0 ? 0 : (c > kCells - 1 ? kCells - 1 : c);
    inds[i] = cell_to_pixel(c, u_row[i], u_col[i], sx, sy, H, W);
}

__global__ void __launch_bounds__(kThreads) k_error_map_update(float* __restrict__ map,
                                                               const int64_t* __restrict__ inds_coarse,
                                                               const float* __restrict__ err, uint32_t N) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const int64_t c = inds_coarse[i];
    if (c < 0 || c >= kCells) return;
    const float old_part = 0.1f * map[c], new_part = 0.9f * err[i];
    map[c] = old_part + new_part;
}

int check_image(uint32_t H, uint32_t W, const char* what) {
    if (H == 0 || W == 0 || (uint64_t)H * W > (1u << 30)) ENERF_BADARG("%s: %u x %u image outside 1 .. 2^30 pixels", what, H, W);
    return 0;
}

}  // namespace

int enerf_frame_batch(const float* poses, uint32_t V, uint32_t view, float fx, float fy, float cx, float cy, uint32_t H,
                      uint32_t W, const int64_t* inds, uint32_t N, const float* images, uint32_t Ci, float* rays_o,
                      float* rays_d, float* target, enerf_stream_t stream) {
    if (int err = check_image(H, W, "frame_batch")) return err;
    if (!poses || !rays_o || !rays_d) ENERF_BADARG("frame_batch: null pointer");
    if (view >= V) ENERF_BADARG("frame_batch: view %u of %u", view, V);
    if (images && (Ci < 1 || Ci > 4 || !target)) ENERF_BADARG("frame_batch: %u image channels (1 .. 4), target %p", Ci, (void*)target);
    if (!inds && N != H * W) ENERF_BADARG("frame_batch: the full frame has %u rays, not %u", H * W, N);
    if (N > (1u << 30)) ENERF_BADARG("frame_batch: %u rays", N);
    if (N == 0) return 0;
    const float* image = images ? images + (size_t)view * H * W * Ci : nullptr;
    k_frame_batch<<<div_up(N, kThreads), kThreads, 0, (hipStream_t)stream>>>(poses + (size_t)view * 16, fx, fy, cx, cy, H, W,
                                                                            inds, N, image, Ci, rays_o, rays_d, target);
    ENERF_LAUNCH_CHECK("frame_batch");
    return 0;
}

int enerf_error_map_sample(const float* weights, const float* e, const float* u_row, const float* u_col, uint32_t N,
                           uint32_t H, uint32_t W, int64_t* inds_coarse, int64_t* inds, enerf_stream_t stream) {
    if (int err = check_image(H, W, "error_map_sample")) return err;
    if (N > (uint32_t)kCells) ENERF_BADARG("error_map_sample: %u samples without replacement from %d cells", N, kCells);
    if (!u_row || !u_col || !inds_coarse || !inds) ENERF_BADARG("error_map_sample: null pointer");
    if ((weights == nullptr) != (e == nullptr)) ENERF_BADARG("error_map_sample: weights and e come together");
    if (N == 0) return 0;
    const float sx = (float)((double)H / 128.0), sy = (float)((double)W / 128.0);
    hipStream_t s = (hipStream_t)stream;
    if (weights)
        k_error_map_sample<<<1, kSortThreads, 0, s>>>(weights, e, u_row, u_col, N, sx, sy, H, W, inds_coarse, inds);
    else
        k_error_map_pixels<<<div_up(N, kThreads), kThreads, 0, s>>>(inds_coarse, u_row, u_col, N, sx, sy, H, W, inds);
    ENERF_LAUNCH_CHECK("error_map_sample");
    return 0;
}

int enerf_error_map_update(float* map, const int64_t* inds_coarse, const float* err, uint32_t N, enerf_stream_t stream) {
    if (!map || !inds_coarse || !err) ENERF_BADARG("error_map_update: null pointer");
    if (N > (uint32_t)kCells) ENERF_BADARG("error_map_update: %u cells of %d", N, kCells);
    if (N == 0) return 0;
    k_error_map_update<<<div_up(N, kThreads), kThreads, 0, (hipStream_t)stream>>>(map, inds_coarse, err, N);
    ENERF_LAUNCH_CHECK("error_map_update");
    return 0;
}

// The sorting network and the pixel mapping of k_error_map_sample on the host, thread by thread (a pass's groups are
// disjoint, so running its threads one after the other is the same computation): what the tests without a GPU hold to the
// statement.  Host pointers.
int enerf_debug_error_map_sample_host(const float* weights, const float* e, const float* u_row, const float* u_col,
                                      uint32_t N, uint32_t H, uint32_t W, int64_t* inds_coarse, int64_t* inds) {
    if (int err = check_image(H, W, "debug_error_map_sample_host")) return err;
    if (N > (uint32_t)kCells) ENERF_BADARG("debug_error_map_sample_host: %u samples from %d cells", N, kCells);
    if (!weights || !e || !u_row || !u_col || !inds_coarse || !inds) ENERF_BADARG("debug_error_map_sample_host: null pointer");
    uint64_t* cells = new uint64_t[kPadded];
    const float sx = (float)((double)H / 128.0), sy = (float)((double)W / 128.0);
    for (uint32_t c = 0; c < (uint32_t)kCells; ++c) cells[padded(c)] = composite(weights[c], e[c], c);
    for (int s = 1; s <= kCellsLog2; ++s)
        for (int hi = s - 1; hi >= 0; hi -= 4) {
            const int lo = hi >= 3 ? hi - 3 : 0;
            for (uint32_t tid = 0; tid < (uint32_t)kSortThreads; ++tid)
                sort_pass(cells, tid, kSortThreads, lo, hi - lo + 1, 1u << s);
        }
    for (uint32_t i = 0; i < N; ++i) {
        const int64_t c = (int64_t)composite_cell(cells[padded(i)]);
        inds_coarse[i] = c;
        inds[i] = cell_to_pixel(c, u_row[i], u_col[i], sx, sy, H, W);
    }
    delete[] cells;
    return 0;
}
