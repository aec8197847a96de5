// eval_metrics.hip -- the metrics of the reference's Trainer.evaluate_one_epoch (nerf/utils.py:44-92, 1028-1293) for
// gfx950: per-view squared error and log-intensity sums, the event-only affine correction, and SSIM.  The semantics are
// written out in enerf_amd/evaluate.py (whose torch statement is the CPU path and the tests' reference) and DESIGN.md 4.11.
//
//   k_eval_stats    one pass over V stacked views [V, H, W, C] fp32: per view the fp64 SSE of pred - gt over H*W*C and,
//                   in log mode, with x = log(255 l(pred) + 1e-3), y = log(255 l(gt) + 1e-3) in fp32 (l = identity for
//                   C = 1, the esim luma for C = 3), the fp64 sums of x, y, x^2 and xy
//   k_eval_correct  a, b: least squares of y on [1, x] over every view's pixels (fp64, from the stats' sums); then per pixel
//                   pred_cor = exp(a x + b) and gt_j = l(255 gt) in fp32, both written as [V, H, W] planes, and the fp64
//                   SSE of gt_j - pred_cor
//   k_eval_ssim     skimage's structural_similarity defaults: 7x7 uniform window, sample covariance, K1 = 0.01,
//                   K2 = 0.03, mean of S over the (H - 6) x (W - 6) interior.  A workgroup loads a 32 x 16 output tile
//                   and its 6-pixel apron into LDS, takes the horizontal then the vertical 7-tap sums of x, y, x^2, y^2
//                   and xy in fp64 (exact products of fp32 values: no E[x^2] - E[x]^2 cancellation at data_range 255)
//   k_eval_reduce   the fixed-order second pass: per view, the workgroup partials summed by one workgroup
//
// Every sum is per-thread partials in a fixed stride, a fixed shuffle tree, then k_eval_reduce: no atomics, the same bits
// from run to run whatever the GPU's scheduling.  Compiled with -ffp-contract=off: a x + b is two roundings, as torch's
// two element-wise kernels are.
#include <math.h>

#include "common.h"

using namespace enerf;

namespace {

constexpr int kThreads = 256;
constexpr int kStatBlocks = 64;                 // workgroups per view of the stats and correct passes (at most)
constexpr int kTileX = 32, kTileY = 16;         // SSIM output tile
constexpr int kWin = 7, kPad = 3;
constexpr int kInX = kTileX + kWin - 1, kInY = kTileY + kWin - 1;
constexpr int kStatsK = 5;                      // sse, sx, sy, sxx, sxy

__device__ __forceinline__ float luma(float r, float g, float b) {
    return (r * 0.299f + g * 0.587f) + b * 0.114f;  // torch.sum(rgb * factors, -1): left to right in fp32
}

__device__ __forceinline__ float log_intensity(const float* p, int C) {
    float l = C == 3 ? luma(p[0], p[1], p[2]) : p[0];
    return logf(255.0f * l + 1e-3f);
}

// sum of v over the workgroup (kThreads), in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (lane == 0) lds[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kThreads / kWave; ++i) s += lds[i];
    __syncthreads();                            // (lds is reused by the next call)
    return s;
}

__global__ void __launch_bounds__(kThreads) k_eval_stats(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         uint32_t P, int C, int log_mode, double* __restrict__ part) {
    __shared__ double lds[kThreads / kWave];
    const uint32_t v = blockIdx.y, nb = gridDim.x;
    const size_t base = (size_t)v * P * C;
    double sse = 0.0, sx = 0.0, sy = 0.0, sxx = 0.0, sxy = 0.0;
    for (uint32_t p = blockIdx.x * kThreads + threadIdx.x; p < P; p += nb * kThreads) {
        const float* pp = pred + base + (size_t)p * C;
        const float* gg = gt + base + (size_t)p * C;
        for (int c = 0; c < C; ++c) {
            double d = (double)(pp[c] - gg[c]);
            sse += d * d;
        }
        if (log_mode) {
            float x = log_intensity(pp, C), y = log_intensity(gg, C);
            sx += (double)x;
            sy += (double)y;
            sxx += (double)x * (double)x;
            sxy += (double)x * (double)y;
        }
    }
    const int K = log_mode ? kStatsK : 1;
    double* o = part + ((size_t)v * nb + blockIdx.x) * K;
    double r = block_sum(sse, lds);
    if (threadIdx.x == 0) o[0] = r;
    if (log_mode) {
        double q[4] = {sx, sy, sxx, sxy};
        for (int k = 0; k < 4; ++k) {
            r = block_sum(q[k], lds);
            if (threadIdx.x == 0) o[1 + k] = r;
        }
    }
}

// a, b of solve_normal_equations from the per-view sums (res rows of ENERF_EVAL_COLS: sx, sy, sxx, sxy in columns 1..4),
// summed over the views in order; a NaN becomes 5
__device__ __forceinline__ void fit(const double* res, uint32_t V, double n, double& a, double& b) {
    double sx = 0.0, sy = 0.0, sxx = 0.0, sxy = 0.0;
    for (uint32_t v = 0; v < V; ++v) {
        const double* r = res + (size_t)v * ENERF_EVAL_COLS;
        sx += r[1];
        sy += r[2];
        sxx += r[3];
        sxy += r[4];
    }
    double det = n * sxx - sx * sx;
    b = (sxx * sy - sx * sxy) / det;
    a = (n * sxy - sx * sy) / det;
    if (isnan(b)) b = 5.0;
    if (isnan(a)) a = 5.0;
}

__global__ void __launch_bounds__(kThreads) k_eval_correct(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           uint32_t V, uint32_t P, int C, const double* __restrict__ res,
                                                           double* __restrict__ ab, float* __restrict__ pred_cor,
                                                           float* __restrict__ gt_j, double* __restrict__ part) {
    __shared__ double lds[kThreads / kWave];
    const uint32_t v = blockIdx.y, nb = gridDim.x;
    double a, b;
    fit(res, V, (double)V * (double)P, a, b);
    if (v == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        ab[0] = a;
        ab[1] = b;
    }
    const float af = (float)a, bf = (float)b;
    const size_t base = (size_t)v * P;
    double sse = 0.0;
    for (uint32_t p = blockIdx.x * kThreads + threadIdx.x; p < P; p += nb * kThreads) {
        const float* pp = pred + (base + p) * C;
        const float* gg = gt + (base + p) * C;
        float x = log_intensity(pp, C);
        float ax = af * x;
        float pc = expf(ax + bf);
        float gj = C == 3 ? luma(255.0f * gg[0], 255.0f * gg[1], 255.0f * gg[2]) : 255.0f * gg[0];
        pred_cor[base + p] = pc;
        gt_j[base + p] = gj;
        double d = (double)(gj - pc);
        sse += d * d;
    }
    double r = block_sum(sse, lds);
    if (threadIdx.x == 0) part[(size_t)v * nb + blockIdx.x] = r;
}

__global__ void __launch_bounds__(kThreads) k_eval_ssim(const float* __restrict__ x, const float* __restrict__ y,
                                                        uint32_t H, uint32_t W, uint32_t stride, double c1, double c2,
                                                        double* __restrict__ part) {
    __shared__ float sx[kInY][kInX], sy[kInY][kInX];
    __shared__ double hs[5][kInY][kTileX];
    __shared__ double lds[kThreads / kWave];
    const uint32_t v = blockIdx.y;
    const uint32_t tiles_x = div_up(W - 2 * kPad, kTileX);
    const uint32_t ox0 = (blockIdx.x % tiles_x) * kTileX, oy0 = (blockIdx.x / tiles_x) * kTileY;
    const size_t plane = (size_t)H * W * stride;
    const float* xv = x + v * plane;
    const float* yv = y + v * plane;
    // the input window of the tile: rows oy0 .. oy0 + kInY - 1, columns ox0 .. ox0 + kInX - 1 (0 outside the image: only
    // outputs outside the interior read those, and they are not counted)
    for (int i = threadIdx.x; i < kInY * kInX; i += kThreads) {
        const int r = i / kInX, c = i % kInX;
        const uint32_t gy = oy0 + r, gx = ox0 + c;
        float a = 0.0f, b = 0.0f;
        if (gy < H && gx < W) {
            const size_t o = ((size_t)gy * W + gx) * stride;
            a = xv[o];
            b = yv[o];
        }
        sx[r][c] = a;
        sy[r][c] = b;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kInY * kTileX; i += kThreads) {
        const int r = i / kTileX, c = i % kTileX;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const double a = sx[r][c + k], b = sy[r][c + k];
            s0 += a;
            s1 += b;
            s2 += a * a;
            s3 += b * b;
            s4 += a * b;
        }
        hs[0][r][c] = s0;
        hs[1][r][c] = s1;
        hs[2][r][c] = s2;
        hs[3][r][c] = s3;
        hs[4][r][c] = s4;
    }
    __syncthreads();
    const double inv_np = 1.0 / (kWin * kWin), cov_norm = (double)(kWin * kWin) / (kWin * kWin - 1);
    double acc = 0.0;
    for (int i = threadIdx.x; i < kTileY * kTileX; i += kThreads) {
        const int r = i / kTileX, c = i % kTileX;
        if (oy0 + r >= H - 2 * kPad || ox0 + c >= W - 2 * kPad) continue;
        double s[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < kWin; ++k) t += hs[q][r + k][c];
            s[q] = t * inv_np;
        }
        const double ux = s[0], uy = s[1];
        const double vx = cov_norm * (s[2] - ux * ux), vy = cov_norm * (s[3] - uy * uy);
        const double vxy = cov_norm * (s[4] - ux * uy);
        const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2;
        const double b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
        acc += (a1 * a2) / (b1 * b2);
    }
    const double t = block_sum(acc, lds);
    if (threadIdx.x == 0) part[(size_t)v * gridDim.x + blockIdx.x] = t;
}

// res[v * ENERF_EVAL_COLS + col + k] = (sum over the nb partials of view v (K per partial)) / div, in a fixed order
__global__ void __launch_bounds__(kThreads) k_eval_reduce(const double* __restrict__ part, uint32_t nb, int K,
                                                          double div, double* __restrict__ res, int col) {
    __shared__ double lds[kThreads / kWave];
    const uint32_t v = blockIdx.x;
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (uint32_t i = threadIdx.x; i < nb; i += kThreads) s += part[((size_t)v * nb + i) * K + k];
        s = block_sum(s, lds);
        if (threadIdx.x == 0) res[(size_t)v * ENERF_EVAL_COLS + col + k] = s / div;
    }
}

uint32_t stat_blocks(uint32_t P) {
    uint32_t nb = div_up(P, kThreads * 4);
    return nb < 1 ? 1 : (nb > kStatBlocks ? kStatBlocks : nb);
}

uint32_t ssim_tiles(uint32_t H, uint32_t W) {
    return div_up(W - 2 * kPad, kTileX) * div_up(H - 2 * kPad, kTileY);
}

int check_shape(uint32_t V, uint32_t H, uint32_t W, const char* what) {
    if (V == 0 || V > 65535) ENERF_BADARG("%s: %u views outside 1 .. 65535", what, V);
    if (H < kWin || W < kWin) ENERF_BADARG("%s: %u x %u image smaller than the 7 x 7 window", what, H, W);
    if ((uint64_t)H * W > (1u << 30)) ENERF_BADARG("%s: %u x %u image too large", what, H, W);
    return 0;
}

int check_channels(int C, const char* what) {
    if (C != 1 && C != 3) ENERF_BADARG("%s: %d channels (1 or 3 expected)", what, C);
    return 0;
}

}  // namespace

int enerf_eval_workspace(uint32_t V, uint32_t H, uint32_t W, uint64_t* bytes) {
    if (int e = check_shape(V, H, W, "eval_workspace")) return e;
    if (!bytes) ENERF_BADARG("eval_workspace: null pointer");
    uint64_t per_view = (uint64_t)stat_blocks(H * W) * kStatsK;
    uint64_t t = ssim_tiles(H, W);
    if (t > per_view) per_view = t;
    *bytes = per_view * V * sizeof(double);
    return 0;
}

int enerf_eval_stats(const float* pred, const float* gt, uint32_t V, uint32_t H, uint32_t W, int C, int log_mode,
                     void* ws, double* res, enerf_stream_t stream) {
    if (int e = check_shape(V, H, W, "eval_stats")) return e;
    if (int e = check_channels(C, "eval_stats")) return e;
    if (!pred || !gt || !ws || !res) ENERF_BADARG("eval_stats: null pointer");
    const uint32_t P = H * W, nb = stat_blocks(P);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    k_eval_stats<<<dim3(nb, V), kThreads, 0, s>>>(pred, gt, P, C, log_mode ? 1 : 0, part);
    ENERF_LAUNCH_CHECK("eval_stats");
    k_eval_reduce<<<V, kThreads, 0, s>>>(part, nb, log_mode ? kStatsK : 1, 1.0, res, 0);
    ENERF_LAUNCH_CHECK("eval_stats_reduce");
    return 0;
}

int enerf_eval_correct(const float* pred, const float* gt, uint32_t V, uint32_t H, uint32_t W, int C, void* ws,
                       double* res, double* ab, float* pred_cor, float* gt_j, enerf_stream_t stream) {
    if (int e = check_shape(V, H, W, "eval_correct")) return e;
    if (int e = check_channels(C, "eval_correct")) return e;
    if (!pred || !gt || !ws || !res || !ab || !pred_cor || !gt_j) ENERF_BADARG("eval_correct: null pointer");
    const uint32_t P = H * W, nb = stat_blocks(P);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    k_eval_correct<<<dim3(nb, V), kThreads, 0, s>>>(pred, gt, V, P, C, res, ab, pred_cor, gt_j, part);
    ENERF_LAUNCH_CHECK("eval_correct");
    k_eval_reduce<<<V, kThreads, 0, s>>>(part, nb, 1, 1.0, res, ENERF_EVAL_COL_SSE_COR);
    ENERF_LAUNCH_CHECK("eval_correct_reduce");
    return 0;
}

int enerf_eval_ssim(const float* x, const float* y, uint32_t V, uint32_t H, uint32_t W, uint32_t stride,
                    double data_range, void* ws, double* res, enerf_stream_t stream) {
    if (int e = check_shape(V, H, W, "eval_ssim")) return e;
    if (stride == 0 || stride > 4) ENERF_BADARG("eval_ssim: pixel stride %u outside 1 .. 4", stride);
    if (!x || !y || !ws || !res) ENERF_BADARG("eval_ssim: null pointer");
    if (!(data_range > 0.0)) ENERF_BADARG("eval_ssim: data_range %g", data_range);
    const uint32_t nt = ssim_tiles(H, W);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    k_eval_ssim<<<dim3(nt, V), kThreads, 0, s>>>(x, y, H, W, stride, c1, c2, part);
    ENERF_LAUNCH_CHECK("eval_ssim");
    const double interior = (double)(H - 2 * kPad) * (double)(W - 2 * kPad);
    k_eval_reduce<<<V, kThreads, 0, s>>>(part, nt, 1, interior, res, ENERF_EVAL_COL_SSIM);
    ENERF_LAUNCH_CHECK("eval_ssim_reduce");
    return 0;
}
