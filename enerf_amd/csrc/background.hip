// background.hip -- the background model of NeRFNetwork(bg_radius > 0) for gfx950: rays -> bg [N,C] in one launch, and its
// backward (weight gradients, table gradient) in one launch plus a small reduce.
//
// Replaces, per ray, the launch chain of network.py's `background` behind raymarching.polar_from_ray:
//     polar coordinates of the ray's exit from the sphere of radius bg_radius      (k_polar's arithmetic, raymarching.hip)
//     (p + 1) / 2 -> 2-D multiresolution grid, level_dim 2, L levels, hash or tiled (gridencoder.hip's D = 2 arithmetic)
//     the 16 SH values of the direction, or zeros (disable_view_direction)          (sh_basis.h: sh4)
//     sigmoid(W1 relu(W0 [sh | grid]))                                              (fp32 VALU, weights in LDS)
// About 3.5 kFLOP a ray: the matrix cores are not needed, and every stage is the plain fp32 of the kernels it restates, so
// the stages can be compared bit for bit through `trace`.
//
// The D = 2 index arithmetic (BgGeom / bg_make_geom / bg_grid_row / the acc order of the four corners) is restated from
// gridencoder.hip: make_geom, grid_row, acc_feat, grid_fwd_block.  Keep the two in step.
//
// Backward: a workgroup takes tiles of 128 rays.  Per tile every thread recomputes its ray's forward (nothing but the
// rays is kept from it), leaves relu(h) / d h, the input row and d out in LDS, and the workgroup then sums the products
// over the tile's rays: thread (j, k mod 2) owns the entries (j, k), (j, k + 2), ... of grad_W0 and up to two of grad_W1
// in registers across all its tiles, rays in ascending order.  The per-workgroup sums go to a slab and one reducer adds
// the slab's rows in order, so both weight gradients have the same bits on every run.  The table gradient is added with
// float atomics (2 * 4 * L adds a ray): its last bits depend on arrival order.
//
// Compiled with -ffp-contract=off; fused multiply-adds are explicit.
#include <math.h>

#include "common.h"
#include "sh_basis.h"

using namespace enerf;

namespace {

constexpr int kBgMaxLevels = 8;        // levels the kernels are built for (the model's own: 4)
constexpr int kBgHidden = 64;
constexpr int kBgFwdThreads = 256;
constexpr int kBgTile = 128;           // rays per backward tile = threads per backward workgroup
constexpr uint32_t kBgMaxBlocks = 256; // backward workgroups (rows of the slab); more tiles than that are walked in a loop
constexpr float kBgRPi = 0.3183098861837907f;

struct BgLevels {
    float scale[kBgMaxLevels];
    uint32_t resolution[kBgMaxLevels];
};

struct BgArgs {
    const float* rays_o;
    const float* rays_d;
    float radius;
    uint32_t N;
    const float* embeddings;
    const int32_t* offsets;
    uint32_t gridtype, use_dirs, C;
    const float* w0;
    const float* w1;
    BgLevels lv;
    ShNorm4 nrm;
};

// gridencoder.hip: LevelGeom<2> / make_geom<2> / grid_row<2>
struct BgGeom {
    uint32_t size, mask;
    uint32_t stride[2];
    bool hash;
    int wrap;
};
__device__ __forceinline__ BgGeom bg_make_geom(uint32_t gridtype, uint32_t size, uint32_t resolution) {
    BgGeom g;
    g.size = size;
    g.mask = size - 1u;
    uint32_t stride = 1;
    unsigned long long max_index = 0;
#pragma unroll
    for (int d = 0; d < 2; d++) {
        if (stride <= size) {
            g.stride[d] = stride;
            max_index += (unsigned long long)resolution * stride;
            stride *= (resolution + 1);
        } else {
            g.stride[d] = 0;
        }
    }
    g.hash = gridtype == 0 && stride > size;
    g.wrap = (size & (size - 1u)) == 0u ? 1 : ((!g.hash && max_index < size) ? 0 : 2);
    return g;
}
__device__ __forceinline__ uint32_t bg_grid_row(const BgGeom& g, uint32_t px, uint32_t py) {
    uint32_t index;
    if (g.hash) index = (px * 1u) ^ (py * 2654435761u);
    else index = px * g.stride[0] + py * g.stride[1];
    index = g.wrap == 0 ? index : (g.wrap == 1 ? (index & g.mask) : index % g.size);
    return index < g.size ? index : g.size - 1u;       // (never taken for inputs in [0, 1]: keeps a NaN input inside the level)
}

// one level's cell: rows of the four corners (corner idx adds bit d of idx to coordinate d) and their weights
struct BgCell {
    uint32_t row[4];
    float w[4];
};
__device__ __forceinline__ BgCell bg_cell(const float (&in)[2], float scale, const BgGeom& geom) {
    float pos[2];
    uint32_t pg[2];
#pragma unroll
    for (int d = 0; d < 2; d++) {
        pos[d] = fmaf(in[d], scale, 0.5f);
        const float fl = floorf(pos[d]);
        pg[d] = (uint32_t)fl;
        pos[d] -= (float)pg[d];
    }
    BgCell c;
#pragma unroll
    for (int idx = 0; idx < 4; idx++) {
        float wi = 1;
#pragma unroll
        for (int d = 0; d < 2; d++) wi *= (idx & (1 << d)) ? pos[d] : 1 - pos[d];
        c.w[idx] = wi;
        c.row[idx] = bg_grid_row(geom, pg[0] + (idx & 1), pg[1] + ((idx >> 1) & 1));
    }
    return c;
}

// k_polar's arithmetic (raymarching.hip; the oracle's orc_polar_from_ray)
__device__ __forceinline__ void bg_polar(const BgArgs& a, uint32_t n, float (&p)[2], float (&d)[3]) {
    const float ox = a.rays_o[(size_t)n * 3], oy = a.rays_o[(size_t)n * 3 + 1], oz = a.rays_o[(size_t)n * 3 + 2];
    const float dx = a.rays_d[(size_t)n * 3], dy = a.rays_d[(size_t)n * 3 + 1], dz = a.rays_d[(size_t)n * 3 + 2];
    const float A = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const float B = fmaf(oz, dz, fmaf(oy, dy, ox * dx));
    const float C = fmaf(oz, oz, fmaf(oy, oy, ox * ox)) - a.radius * a.radius;
    const float t = (-B + sqrtf(fmaf(B, B, -(A * C)))) / A;
    const float x = fmaf(t, dx, ox), y = fmaf(t, dy, oy), z = fmaf(t, dz, oz);
    const float theta = atan2f(sqrtf(fmaf(z, z, x * x)), y);
    const float phi = atan2f(z, x);
    p[0] = fmaf(2 * theta, kBgRPi, -1.0f);
    p[1] = phi * kBgRPi;
    d[0] = dx;
    d[1] = dy;
    d[2] = dz;
}

// the MLP's input row [sh | grid] of ray n, its polar pair, and the grid's input (p + 1) / 2 with its in-range flag
template <int L>
__device__ __forceinline__ void bg_input_row(const BgArgs& a, uint32_t n, float (&p)[2], float (&in)[2], bool& oob,
                                             float (&x)[16 + 2 * L]) {
    float d[3];
    bg_polar(a, n, p, d);
    if (a.use_dirs) {
        float Y[16];
        sh4(d[0], d[1], d[2], a.nrm, Y);
#pragma unroll
        for (int i = 0; i < 16; i++) x[i] = Y[i];
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) x[i] = 0.0f;
    }
    oob = false;
#pragma unroll
    for (int d2 = 0; d2 < 2; d2++) {
        in[d2] = (p[d2] + 1.0f) * 0.5f;
        oob |= (in[d2] < 0 || in[d2] > 1);
    }
    const float2* __restrict__ table = reinterpret_cast<const float2*>(a.embeddings);
#pragma unroll
    for (int l = 0; l < L; l++) {
        float r0 = 0, r1 = 0;
        if (!oob) {
            const uint32_t off0 = (uint32_t)a.offsets[l];
            const BgGeom geom = bg_make_geom(a.gridtype, (uint32_t)a.offsets[l + 1] - off0, a.lv.resolution[l]);
            const BgCell c = bg_cell(in, a.lv.scale[l], geom);
            float2 f[4];
#pragma unroll
            for (int idx = 0; idx < 4; idx++) f[idx] = table[(size_t)off0 + c.row[idx]];
#pragma unroll
            for (int idx = 0; idx < 4; idx++) {
                r0 = fmaf(c.w[idx], f[idx].x, r0);
                r1 = fmaf(c.w[idx], f[idx].y, r1);
            }
        }
        x[16 + 2 * l] = r0;
        x[16 + 2 * l + 1] = r1;
    }
}

template <int K>
__device__ __forceinline__ void bg_load_weights(const BgArgs& a, float* sW0, float* sW1, int nthreads) {
    for (int i = threadIdx.x; i < kBgHidden * K; i += nthreads) sW0[i] = a.w0[i];
    for (int i = threadIdx.x; i < 3 * kBgHidden; i += nthreads) sW1[i] = i < (int)a.C * kBgHidden ? a.w1[i] : 0.0f;
}

__device__ __forceinline__ float bg_sigmoid(float o) { return 1.0f / (1.0f + expf(-o)); }

template <int L>
__global__ void __launch_bounds__(kBgFwdThreads) k_bg_fwd(BgArgs a, float* __restrict__ bg, float* __restrict__ trace) {
    constexpr int K = 16 + 2 * L;
    __shared__ float sW0[kBgHidden * K];
    __shared__ float sW1[3 * kBgHidden];
    bg_load_weights<K>(a, sW0, sW1, kBgFwdThreads);
    __syncthreads();
    const uint32_t n = blockIdx.x * kBgFwdThreads + threadIdx.x;
    if (n >= a.N) return;
    float p[2], in[2], x[K];
    bool oob;
    bg_input_row<L>(a, n, p, in, oob, x);
    if (trace) {
        float* t = trace + (size_t)n * (2 + K);
        t[0] = p[0];
        t[1] = p[1];
#pragma unroll
        for (int k = 0; k < K; k++) t[2 + k] = x[k];
    }
    float out[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int j = 0; j < kBgHidden; j++) {
        float h = 0.0f;
#pragma unroll
        for (int k = 0; k < K; k++) h = fmaf(sW0[j * K + k], x[k], h);
        h = fmaxf(h, 0.0f);
#pragma unroll
        for (int c = 0; c < 3; c++) out[c] = fmaf(sW1[c * kBgHidden + j], h, out[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
        if (c < (int)a.C) bg[(size_t)n * a.C + c] = bg_sigmoid(out[c]);
}

template <int L>
__global__ void __launch_bounds__(kBgTile) k_bg_bwd(BgArgs a, const float* __restrict__ grad_image,
                                                    const float* __restrict__ weights_sum, float* __restrict__ part,
                                                    uint32_t part_stride, float* __restrict__ grad_emb) {
    constexpr int K = 16 + 2 * L;
    constexpr int SA = kBgHidden + 1;     // odd row strides: a lane per ray writes its row without bank conflicts
    constexpr int SX = K + 1;
    constexpr int NK = K / 2;             // entries of grad_W0 per thread
    __shared__ float sW0[kBgHidden * K];
    __shared__ float sW1[3 * kBgHidden];
    __shared__ float sA[kBgTile * SA];    // relu(h), then d h
    __shared__ float sX[kBgTile * SX];
    __shared__ float sG[kBgTile * 4];     // d out
    bg_load_weights<K>(a, sW0, sW1, kBgTile);
    const int t = threadIdx.x;
    const int j_own = t & 63, half = t >> 6;
    float acc0[NK], acc1[2] = {0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < NK; i++) acc0[i] = 0.0f;
    const uint32_t tiles = div_up(a.N, (uint32_t)kBgTile);
    float2* __restrict__ gtable = reinterpret_cast<float2*>(grad_emb);

    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        __syncthreads();                  // the weights are in LDS; the previous tile's sums are done with sA / sX / sG
        const uint32_t n = tile * kBgTile + t;
        const bool valid = n < a.N;
        float p[2], in[2] = {0.0f, 0.0f}, x[K];
        bool oob = true;
        if (valid) {
            bg_input_row<L>(a, n, p, in, oob, x);
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) x[k] = 0.0f;
        }
#pragma unroll
        for (int k = 0; k < K; k++) sX[t * SX + k] = x[k];
        float out[3] = {0.0f, 0.0f, 0.0f};
        unsigned long long mask = 0;
#pragma unroll 4
        for (int j = 0; j < kBgHidden; j++) {
            float h = 0.0f;
#pragma unroll
            for (int k = 0; k < K; k++) h = fmaf(sW0[j * K + k], x[k], h);
            if (h > 0.0f) mask |= 1ull << j;
            h = fmaxf(h, 0.0f);
            sA[t * SA + j] = h;
#pragma unroll
            for (int c = 0; c < 3; c++) out[c] = fmaf(sW1[c * kBgHidden + j], h, out[c]);
        }
        float go[3] = {0.0f, 0.0f, 0.0f};
        if (valid) {
            const float f = weights_sum ? 1.0f - weights_sum[n] : 1.0f;
#pragma unroll
            for (int c = 0; c < 3; c++)
                if (c < (int)a.C) {
                    const float y = bg_sigmoid(out[c]);
                    go[c] = (f * grad_image[(size_t)n * a.C + c]) * (y * (1.0f - y));
                }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) sG[t * 4 + c] = go[c];
        __syncthreads();
        // grad_W1[c][j] += sum over the tile's rays of d out[c] * relu(h[j])
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int c = half + 2 * i;
            if (c < (int)a.C) {
                float s = acc1[i];
                for (int r = 0; r < kBgTile; r++) s = fmaf(sG[r * 4 + c], sA[r * SA + j_own], s);
                acc1[i] = s;
            }
        }
        __syncthreads();
        // d h = relu'(h) * W1^T d out (over sA), and this ray's d x of the grid columns
        float gx[2 * L];
#pragma unroll
        for (int k = 0; k < 2 * L; k++) gx[k] = 0.0f;
#pragma unroll 4
        for (int j = 0; j < kBgHidden; j++) {
            float gh = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; c++) gh = fmaf(sW1[c * kBgHidden + j], go[c], gh);
            gh = ((mask >> j) & 1ull) ? gh : 0.0f;
            sA[t * SA + j] = gh;
#pragma unroll
            for (int k = 0; k < 2 * L; k++) gx[k] = fmaf(sW0[j * K + 16 + k], gh, gx[k]);
        }
        __syncthreads();
        // grad_W0[j][k] += sum over the tile's rays of d h[j] * x[k]
        for (int r = 0; r < kBgTile; r++) {
            const float gh = sA[r * SA + j_own];
#pragma unroll
            for (int i = 0; i < NK; i++) acc0[i] = fmaf(gh, sX[r * SX + half + 2 * i], acc0[i]);
        }
        // the table: every corner of every level takes weight * d feature
        if (valid && !oob) {
#pragma unroll
            for (int l = 0; l < L; l++) {
                const uint32_t off0 = (uint32_t)a.offsets[l];
                const BgGeom geom = bg_make_geom(a.gridtype, (uint32_t)a.offsets[l + 1] - off0, a.lv.resolution[l]);
                const BgCell c = bg_cell(in, a.lv.scale[l], geom);
#pragma unroll
                for (int idx = 0; idx < 4; idx++) {
                    float2* row = gtable + (size_t)off0 + c.row[idx];
                    atomicAdd(&row->x, c.w[idx] * gx[2 * l]);
                    atomicAdd(&row->y, c.w[idx] * gx[2 * l + 1]);
                }
            }
        }
    }
    // this workgroup's sums: row blockIdx.x of the slab (or the gradients themselves when it is the only workgroup),
    // grad_W0 [64, K] first, grad_W1 [C, 64] behind it
    float* dst = part + (size_t)blockIdx.x * part_stride;
#pragma unroll
    for (int i = 0; i < NK; i++) dst[j_own * K + half + 2 * i] = acc0[i];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int c = half + 2 * i;
        if (c < (int)a.C) dst[kBgHidden * K + c * kBgHidden + j_own] = acc1[i];
    }
}

// out[i] = slab[0][i] + slab[1][i] + ... in that order; grad_W0's n0 values, then grad_W1's
__global__ void __launch_bounds__(256) k_bg_reduce(const float* __restrict__ part, uint32_t parts, uint32_t stride,
                                                   uint32_t n0, uint32_t n1, float* __restrict__ grad_w0,
                                                   float* __restrict__ grad_w1) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n0 + n1) return;
    float s = 0.0f;
    for (uint32_t b = 0; b < parts; b++) s += part[(size_t)b * stride + i];
    if (i < n0) grad_w0[i] = s;
    else grad_w1[i - n0] = s;
}

int bg_check(const char* what, const float* rays_o, const float* rays_d, const float* embeddings, const int32_t* offsets,
             uint32_t L, uint32_t level_dim, const float* w0, const float* w1, uint32_t hidden, uint32_t C) {
    if (C < 1 || C > 3) ENERF_BADARG("%s: C must be 1..3, got %u", what, C);
    if (hidden != (uint32_t)kBgHidden) ENERF_BADARG("%s: hidden width must be %d, got %u", what, kBgHidden, hidden);
    if (level_dim != 2) ENERF_BADARG("%s: level_dim must be 2, got %u", what, level_dim);
    if (L < 1 || L > (uint32_t)kBgMaxLevels) ENERF_BADARG("%s: L must be in [1, %d], got %u", what, kBgMaxLevels, L);
    if (!rays_o || !rays_d || !embeddings || !offsets || !w0 || !w1) ENERF_BADARG("%s: null pointer", what);
    return 0;
}

BgArgs bg_args(const float* rays_o, const float* rays_d, float radius, uint32_t N, const float* embeddings,
               const int32_t* offsets, uint32_t L, float S, uint32_t H, uint32_t gridtype, uint32_t use_dirs, const float* w0,
               const float* w1, uint32_t C) {
    BgArgs a;
    a.rays_o = rays_o;
    a.rays_d = rays_d;
    a.radius = radius;
    a.N = N;
    a.embeddings = embeddings;
    a.offsets = offsets;
    a.gridtype = gridtype;
    a.use_dirs = use_dirs;
    a.C = C;
    a.w0 = w0;
    a.w1 = w1;
    for (uint32_t l = 0; l < (uint32_t)kBgMaxLevels; l++) {
        // gridencoder.hip fill_level_tab: fp32 exp2f, fp32 multiply / subtract, ceil
        const float scale = l < L ? exp2f((float)l * S) * (float)H - 1.0f : 0.0f;
        a.lv.scale[l] = scale;
        a.lv.resolution[l] = (uint32_t)ceil(scale) + 1;
    }
    a.nrm = make_sh_norm4();
    return a;
}

}  // namespace

extern "C" {

int enerf_background_forward(const float* rays_o, const float* rays_d, float radius, uint32_t N, const float* embeddings,
                             const int32_t* offsets, uint32_t L, uint32_t level_dim, float S, uint32_t H, uint32_t gridtype,
                             uint32_t use_dirs, const float* w0, const float* w1, uint32_t hidden, uint32_t C, float* bg,
                             float* trace, enerf_stream_t stream) {
    if (int e = bg_check("background_forward", rays_o, rays_d, embeddings, offsets, L, level_dim, w0, w1, hidden, C)) return e;
    if (!bg) ENERF_BADARG("background_forward: null pointer");
    if (N == 0) return 0;
    const BgArgs a = bg_args(rays_o, rays_d, radius, N, embeddings, offsets, L, S, H, gridtype, use_dirs, w0, w1, C);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t blocks = div_up(N, (uint32_t)kBgFwdThreads);
    switch (L) {
#define ENERF_BG_F(LL) case LL: k_bg_fwd<LL><<<blocks, kBgFwdThreads, 0, s>>>(a, bg, trace); break;
        ENERF_BG_F(1) ENERF_BG_F(2) ENERF_BG_F(3) ENERF_BG_F(4) ENERF_BG_F(5) ENERF_BG_F(6) ENERF_BG_F(7) ENERF_BG_F(8)
#undef ENERF_BG_F
    }
    ENERF_LAUNCH_CHECK("background_forward");
    return 0;
}

int enerf_background_backward(const float* rays_o, const float* rays_d, float radius, uint32_t N, const float* embeddings,
                              const int32_t* offsets, uint32_t L, uint32_t level_dim, float S, uint32_t H,
                              uint32_t gridtype, uint32_t use_dirs, const float* w0, const float* w1, uint32_t hidden,
                              uint32_t C, const float* grad_image, const float* weights_sum, float* grad_w0, float* grad_w1,
                              float* grad_embeddings, enerf_stream_t stream) {
    if (int e = bg_check("background_backward", rays_o, rays_d, embeddings, offsets, L, level_dim, w0, w1, hidden, C)) return e;
    if (!grad_image || !grad_w0 || !grad_w1 || !grad_embeddings) ENERF_BADARG("background_backward: null pointer");
    if (N == 0) return 0;
    const BgArgs a = bg_args(rays_o, rays_d, radius, N, embeddings, offsets, L, S, H, gridtype, use_dirs, w0, w1, C);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t K = 16 + 2 * L, n0 = kBgHidden * K, n1 = C * kBgHidden;
    const uint32_t tiles = div_up(N, (uint32_t)kBgTile);
    const uint32_t blocks = tiles < kBgMaxBlocks ? tiles : kBgMaxBlocks;
    const uint32_t stride = kBgHidden * (16 + 2 * kBgMaxLevels) + 3 * kBgHidden;
    if (int ew = workspace_family_enter(1, s)) return ew;
    float* part = (float*)workspace(WS_BACKGROUND, (size_t)kBgMaxBlocks * stride * sizeof(float));
    if (!part) return ENERF_E_NOMEM;
    switch (L) {
#define ENERF_BG_B(LL) case LL: k_bg_bwd<LL><<<blocks, kBgTile, 0, s>>>(a, grad_image, weights_sum, part, stride, grad_embeddings); break;
        ENERF_BG_B(1) ENERF_BG_B(2) ENERF_BG_B(3) ENERF_BG_B(4) ENERF_BG_B(5) ENERF_BG_B(6) ENERF_BG_B(7) ENERF_BG_B(8)
#undef ENERF_BG_B
    }
    ENERF_LAUNCH_CHECK("background_backward");
    k_bg_reduce<<<div_up(n0 + n1, 256u), 256, 0, s>>>(part, blocks, stride, n0, n1, grad_w0, grad_w1);
    ENERF_LAUNCH_CHECK("background_backward(reduce)");
    return 0;
}

}  // extern "C"
