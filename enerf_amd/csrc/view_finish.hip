// view_finish.hip -- a rendered fp32 frame to what is shown or written, for gfx950: what the reference does on the host
// after a test render (nerf/utils.py:768-804 Trainer.test, :870-918 test_gui: F.interpolate(mode="nearest"),
// linear_to_srgb, * 255, astype(uint8); nerf/gui.py:119-149: the running mean over samples per pixel; scripts/render.py:502:
// the per-frame min-max scaling).  The semantics are written out in enerf_amd/view.py (whose torch statement is the CPU
// path and the tests' reference) and DESIGN.md 4.15.
//
//   k_view_finish      one thread per OUTPUT pixel: nearest source pixel -> min-max scaling -> linear_to_srgb -> running
//                      mean -> fp32 and 8-bit stores; the depth plane takes the gather and the stores only.  No LDS, no
//                      intermediate in memory; a frame is read once and every output written once.
//   k_view_minmax      min and max of the image values, NaNs skipped, per workgroup into `ws` ...
//   k_view_minmax_end  ... and one workgroup over the partials into minmax[2]; (0, 1) when no value was seen.
//
// Compiled with -ffp-contract=off: every product, quotient and sum below is rounded to fp32 on its own, as the
// element-wise torch kernels of the statement do.
#include <math.h>

#include "common.h"

using namespace enerf;

namespace {

constexpr int kThreads = 256;
constexpr int kMinmaxBlocks = ENERF_VIEW_MINMAX_WS / 2;

// evaluate.to_u8: clip(v * 255, 0, 255) truncated; a NaN fails both comparisons' first and becomes 0
__device__ __forceinline__ uint8_t to_u8(float v) {
    const float s = v * 255.0f;
    return (uint8_t)(s > 0.0f ? (s < 255.0f ? s : 255.0f) : 0.0f);
}

// F.interpolate(mode="nearest")'s source index of output index `dst`
__device__ __forceinline__ uint32_t nearest(uint32_t dst, float scale, uint32_t in_size) {
    const uint32_t s = (uint32_t)(int)floorf((float)dst * scale);
    return s < in_size - 1 ? s : in_size - 1;
}

template <int C>
__global__ void __launch_bounds__(kThreads) k_view_finish(const float* __restrict__ image, const float* __restrict__ depth,
                                                          uint32_t h, uint32_t w, uint32_t H, uint32_t W, float scale_h,
                                                          float scale_w, uint32_t linear,
                                                          const float* __restrict__ minmax, float* accum, uint32_t spp,
                                                          float* out_f32,
                                                          uint8_t* __restrict__ out_u8, float* __restrict__ depth_f32,
                                                          uint8_t* __restrict__ depth_u8) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= H * W) return;
    const uint32_t y = p / W, x = p - y * W;
    const size_t src = (size_t)nearest(y, scale_h, h) * w + nearest(x, scale_w, w);
    if (depth) {
        const float d = depth[src];
        if (depth_f32) depth_f32[p] = d;
        if (depth_u8) depth_u8[p] = to_u8(d);
    }
    if (!image) return;
    float mn = 0.0f, range = 0.0f;
    if (minmax) {
        mn = minmax[0];
        range = minmax[1] - mn;
    }
    const bool flat = minmax && minmax[1] == mn;
    const float n_old = (float)spp, n_new = (float)(spp + 1);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float v = image[src * C + c];
        if (minmax) v = flat ? 0.0f : (v - mn) / range;
        if (linear) v = v < 0.0031308f ? 12.92f * v : 1.055f * powf(v, 0.41666f) - 0.055f;
        const size_t o = (size_t)p * C + c;
        if (accum) {
            if (spp != 0) v = (accum[o] * n_old + v) / n_new;
            accum[o] = v;
        }
        if (out_f32 && out_f32 != accum) out_f32[o] = v;       // (out_f32 == accum: the running buffer is the result)
        if (out_u8) out_u8[o] = to_u8(v);
    }
}

// fminf / fmaxf return the operand that is a number: NaN is "nothing seen yet" and a NaN value changes nothing
__device__ __forceinline__ void block_minmax(float& mn, float& mx) {
    __shared__ float s_mn[kThreads / kWave], s_mx[kThreads / kWave];
    for (int off = kWave / 2; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_down(mn, off, kWave));
        mx = fmaxf(mx, __shfl_down(mx, off, kWave));
    }
    if (lane_id() == 0) {
        s_mn[threadIdx.x / kWave] = mn;
        s_mx[threadIdx.x / kWave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < kThreads / kWave; ++k) {
            mn = fminf(mn, s_mn[k]);
            mx = fmaxf(mx, s_mx[k]);
        }
}

__global__ void __launch_bounds__(kThreads) k_view_minmax(const float* __restrict__ image, uint64_t n,
                                                          float* __restrict__ ws) {
    float mn = NAN, mx = NAN;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const float v = image[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    block_minmax(mn, mx);
    if (threadIdx.x == 0) {
        ws[2 * blockIdx.x] = mn;
        ws[2 * blockIdx.x + 1] = mx;
    }
}

__global__ void __launch_bounds__(kThreads) k_view_minmax_end(const float* __restrict__ ws, uint32_t nb,
                                                              float* __restrict__ minmax) {
    float mn = NAN, mx = NAN;
    for (uint32_t b = threadIdx.x; b < nb; b += kThreads) {
        mn = fminf(mn, ws[2 * b]);
        mx = fmaxf(mx, ws[2 * b + 1]);
    }
    block_minmax(mn, mx);
    if (threadIdx.x == 0) {
        const bool none = isnan(mn);
        minmax[0] = none ? 0.0f : mn;
        minmax[1] = none ? 1.0f : mx;
    }
}

}  // namespace

int enerf_view_finish(const float* image, const float* depth, uint32_t h, uint32_t w, uint32_t C, uint32_t H, uint32_t W,
                      uint32_t flags, const float* minmax, float* accum, uint32_t spp, float* out_f32, uint8_t* out_u8,
                      float* depth_f32, uint8_t* depth_u8, enerf_stream_t stream) {
    if (C < 1 || C > 3) ENERF_BADARG("view_finish: %u channels (1 .. 3)", C);
    const bool any_out = out_f32 || out_u8 || depth_f32 || depth_u8 || accum;
    if ((uint64_t)H * W == 0) {
        if (any_out) ENERF_BADARG("view_finish: a %u x %u output with output pointers", H, W);
        return 0;
    }
    if ((uint64_t)H * W > (1u << 30)) ENERF_BADARG("view_finish: %u x %u output beyond 2^30 pixels", H, W);
    if (h == 0 || w == 0 || (uint64_t)h * w > (1u << 30)) ENERF_BADARG("view_finish: %u x %u image outside 1 .. 2^30 pixels", h, w);
    if (accum && !out_f32 && !out_u8) ENERF_BADARG("view_finish: accum without out_f32 or out_u8");
    if ((depth_f32 || depth_u8) && !depth) ENERF_BADARG("view_finish: a depth output without depth");
    const bool colour = out_f32 || out_u8;
    if (colour && !image) ENERF_BADARG("view_finish: a colour output without image");
    if (spp == 0xffffffffu) ENERF_BADARG("view_finish: spp %u", spp);
    if (!any_out) return 0;
    if (!colour) image = nullptr;                       // (nothing of it would be stored)
    if (!depth_f32 && !depth_u8) depth = nullptr;
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    const uint32_t linear = flags & ENERF_VIEW_LINEAR;
    const dim3 grid(div_up(H * W, kThreads)), block(kThreads);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1:
            k_view_finish<1><<<grid, block, 0, s>>>(image, depth, h, w, H, W, sh, sw, linear, minmax, accum, spp, out_f32,
                                                    out_u8, depth_f32, depth_u8);
            break;
        case 2:
            k_view_finish<2><<<grid, block, 0, s>>>(image, depth, h, w, H, W, sh, sw, linear, minmax, accum, spp, out_f32,
                                                    out_u8, depth_f32, depth_u8);
            break;
        default:
            k_view_finish<3><<<grid, block, 0, s>>>(image, depth, h, w, H, W, sh, sw, linear, minmax, accum, spp, out_f32,
                                                    out_u8, depth_f32, depth_u8);
            break;
    }
    ENERF_LAUNCH_CHECK("view_finish");
    return 0;
}

int enerf_view_minmax(const float* image, uint64_t n, float* ws, float* minmax, enerf_stream_t stream) {
    if (!minmax || !ws) ENERF_BADARG("view_minmax: null pointer");
    if (n && !image) ENERF_BADARG("view_minmax: %llu values of a null image", (unsigned long long)n);
    if (n > (3ull << 30)) ENERF_BADARG("view_minmax: %llu values", (unsigned long long)n);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t want = (n + kThreads - 1) / kThreads;
    const uint32_t nb = (uint32_t)(want < (uint64_t)kMinmaxBlocks ? want : (uint64_t)kMinmaxBlocks);
    if (nb) {
        k_view_minmax<<<nb, kThreads, 0, s>>>(image, n, ws);
        ENERF_LAUNCH_CHECK("view_minmax");
    }
    k_view_minmax_end<<<1, kThreads, 0, s>>>(ws, nb, minmax);
    ENERF_LAUNCH_CHECK("view_minmax_end");
    return 0;
}
