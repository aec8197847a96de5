// nerf_mlp.hip -- the two networks of nerf/network.py:104-132 (sigma net 32-64-16, colour net 31-64-64-out, nn.Linear
// without bias, ReLU) as ONE launch per direction on the split-bf16 matrix pipe (the arithmetic of mlp32s.hip: every fp32
// operand as bf16 hi + lo, three v_mfma_f32_32x32x16_bf16 products per fp32 product, fp32 accumulation).
//
// Why a second pair of kernels next to mlp32s.hip's one-net-per-launch ones: at the 4096-ray training batch (133 k
// samples, 4160 tiles over 1024 SIMDs) half of the five MLP launches' time did not depend on the batch at all
// (profiles/r05_base_step_timeline_rays64.txt: the same five launches on 64 rays take 8.8 + 9.3 + 16.7 + 13.2 + 4.6 us
// of the 17 + 16 + 37 + 26 + 6 us they take on 4096) -- kernel start, staging fp32 weights through LDS, every wave
// building every operand fragment from them (strided LDS gathers + hi / lo splits), the per-workgroup weight-gradient sums
// and their reduce launch.  Here
//   * the operand fragments are built ONCE per optimizer step by k_nerf_frags (44 wavefronts, 88 KB: forward order and
//     transposed order, hi and lo) and a kernel's set-up is a straight 16-byte-per-lane copy of them into LDS;
//   * the forward is one launch: x [16, Bp, 2] -> sigma net -> its 16 outputs stay in the accumulator registers and ARE
//     K-step 0 of the colour net's first layer (the SH basis, evaluated in registers from the directions, is K-step 1)
//     -> colour net -> sigma = exp(h0), rgb = sigmoid(.): the [B, 32] hand-over tensor is never written or read;
//   * the backward is one launch: both forwards recomputed (bit-identical instruction sequence), colour net dgrad +
//     wgrad, its input gradient is the sigma net's output gradient in registers (column 0 replaced by trunc_exp's
//     backward), sigma net dgrad + wgrad, dL/dx level-major: neither the [B, 32] input gradient nor the hand-over
//     tensor exist, one set-up, one set of per-workgroup sums.
// Operand layouts, the flips by the matrix pipe and the accuracy argument are those of mlp32s.hip (mlp32s_ops.h).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "mlp32_common.h"
#include "mlp32s_ops.h"

namespace enerf_mlp32 {

// ---- fragment table (one fragment = 64 lanes x 16 B of hi, then 64 lanes x 16 B of lo: 2 KiB)
// forward order (A operand: lane (j, h) = output row 32 ob + j, its 8 values = the K-step's contraction slots of half h)
constexpr int F_S0 = 0;      // [ob][t]      sigma first layer, level-major input order kmap<1>
constexpr int F_SO = 4;      // [ib][t]      sigma output layer (16 rows)
constexpr int F_C0 = 8;      // [ob][t]      colour first layer: K-step 0 = the sigma net's outputs, K-step 1 = SH
constexpr int F_CH = 12;     // [ob][ib][t]  colour hidden layer
constexpr int F_CO = 20;     // [ib][t]      colour output layer (out_c rows)      (forward only)
constexpr int NF_FWD = 24;
// transposed order (dgrad: lane = input index of the layer, values = output rows)
constexpr int B_COT = 24;    // [ib]         colour output layer, outputs in natural order 8h + e
constexpr int B_CHT = 26;    // [ib][ob][t]
constexpr int B_C0T = 34;    // [ob][t]      rows = the colour net's logical input columns [h0 | geo 15 | SH 16]
constexpr int B_SOT = 38;    // [ib]         sigma output layer, outputs in accumulator order nrow(e, h)
constexpr int B_S0T = 40;    // [ob][t]
constexpr int NF_ALL = 44;
constexpr int NF_BWD = 40;   // what the backward keeps in LDS: forward fragments 0..19 + transposed 24..43
constexpr uint32_t kFragWords = 512;      // dwords per fragment (hi + lo)

// sigma blob 64x32 + 16x64, colour blob 64x32 + 64x64 + out_c x 64 (out_c <= 16): per-workgroup partial sums
constexpr uint32_t NW_S = HID * IN + 16 * HID;
constexpr uint32_t NW_C_MAX = HID * IN + HID * HID + 16 * HID;
constexpr uint32_t P_STRIDE = NW_S + NW_C_MAX;

typedef unsigned u32x4n __attribute__((ext_vector_type(4)));

// colour net, first layer: memory column of logical column c ([SH 16 | geo 15 (| pad)] in memory, nerf/network.py:95)
__device__ __forceinline__ int c0_memcol(int c, uint32_t w0_cols) {
    if (c == 0) return -1;                             // the raw density: no weight
    const int m = c < 16 ? c + 15 : c - 16;
    return (uint32_t)m < w0_cols ? m : -1;
}

#ifndef NERF_MLP_BACKWARD_UNIT
// Where value e of lane (j, h) of fragment f comes from: tensor k = {ws0 [64,32], ws1 [16,64], wc0 [64,w0_cols], wc1 [64,64],
// wc2 [out_c,64]} in the upper half-word, the element's flat index in the lower; kFragZero = a padding zero.
constexpr uint32_t kFragZero = 0xffffffffu;
__device__ __forceinline__ uint32_t frag_source(int f, int j, int h, int e, uint32_t w0_cols, uint32_t out_c) {
    auto at = [](uint32_t k, int idx) { return (k << 16) | (uint32_t)idx; };
    if (f < F_SO) {
        const int ob = (f - F_S0) >> 1, t = f & 1;
        return at(0, (32 * ob + j) * IN + kmap<1>(8 * t + e, h));
    } else if (f < F_C0) {
        const int ib = (f - F_SO) >> 1, t = f & 1;
        return j < 16 ? at(1, j * HID + 32 * ib + nrow(8 * t + e, h)) : kFragZero;
    } else if (f < F_CH) {
        const int ob = (f - F_C0) >> 1, t = f & 1;
        const int m = c0_memcol(16 * t + nrow(e, h), w0_cols);
        return m < 0 ? kFragZero : at(2, (32 * ob + j) * (int)w0_cols + m);
    } else if (f < F_CO) {
        const int q = f - F_CH, ob = q >> 2, ib = (q >> 1) & 1, t = q & 1;
        return at(3, (32 * ob + j) * HID + 32 * ib + nrow(8 * t + e, h));
    } else if (f < B_COT) {
        const int ib = (f - F_CO) >> 1, t = f & 1;
        return (uint32_t)j < out_c ? at(4, j * HID + 32 * ib + nrow(8 * t + e, h)) : kFragZero;
    } else if (f < B_CHT) {
        const int ib = f - B_COT, o = 8 * h + e;
        return (uint32_t)o < out_c ? at(4, o * HID + 32 * ib + j) : kFragZero;
    } else if (f < B_C0T) {
        const int q = f - B_CHT, ib = q >> 2, ob = (q >> 1) & 1, t = q & 1;
        return at(3, (32 * ob + nrow(8 * t + e, h)) * HID + 32 * ib + j);
    } else if (f < B_SOT) {
        const int ob = (f - B_C0T) >> 1, t = f & 1;
        const int m = c0_memcol(j, w0_cols);
        return m < 0 ? kFragZero : at(2, (32 * ob + nrow(8 * t + e, h)) * (int)w0_cols + m);
    } else if (f < B_S0T) {
        const int ib = f - B_SOT;
        return at(1, nrow(e, h) * HID + 32 * ib + j);
    }
    const int ob = (f - B_S0T) >> 1, t = f & 1;
    return at(0, (32 * ob + nrow(8 * t + e, h)) * IN + j);
}

// One wavefront per fragment.
__global__ void __launch_bounds__(64) k_nerf_frags(const float* __restrict__ ws0, const float* __restrict__ ws1,
                                                  const float* __restrict__ wc0, const float* __restrict__ wc1,
                                                  const float* __restrict__ wc2, uint32_t w0_cols, uint32_t out_c,
                                                  uint32_t* __restrict__ frags) {
    const int f = blockIdx.x, lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const uint32_t src = frag_source(f, j, h, e, w0_cols, out_c);
        const uint32_t k = src >> 16, idx = src & 0xffffu;
        const float* w = k == 0 ? ws0 : k == 1 ? ws1 : k == 2 ? wc0 : k == 3 ? wc1 : wc2;
        v[e] = src == kFragZero ? 0.0f : w[idx];
    }
    const FragT<3> w = split8<3>(v);
    u32x4n* dst = reinterpret_cast<u32x4n*>(frags + (size_t)f * kFragWords);
    dst[lane] = __builtin_bit_cast(u32x4n, w.hi);
    dst[64 + lane] = __builtin_bit_cast(u32x4n, w.lo);
}

// The same as a table: map[(f * 64 + lane) * 8 + e] = frag_source(...) -- what a kernel that knows nothing of the layout
// needs to build the fragments (enerf_nerf_mlp_frag_job: the grid forward of the one-call training step carries the build).
__global__ void __launch_bounds__(64) k_nerf_frag_map(uint32_t w0_cols, uint32_t out_c, uint32_t* __restrict__ map) {
    const int f = blockIdx.x, lane = threadIdx.x, j = lane & 31, h = lane >> 5;
#pragma unroll
    for (int e = 0; e < 8; e++) map[((size_t)f * 64 + lane) * 8 + e] = frag_source(f, j, h, e, w0_cols, out_c);
}

#endif
struct NerfRows {                   // enerf_mlp32_valid_rows(_ex): see WSrc
    const int32_t* valid_rows;
    uint32_t valid_base, valid_cap;
};

// the 16 SH values of a direction, those of the contraction slots of lane half h: slot e <-> component nrow(e, h)
__device__ __forceinline__ void sh_slots(float d0, float d1, float d2, const ShNorm4& nrm, int h, float (&v)[8]) {
    float sh[16];
    sh4(d0, d1, d2, nrm, sh);
    const uint32_t m = 0u - (uint32_t)h;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int i0 = (e & 3) + 8 * (e >> 2);
        v[e] = __uint_as_float((__float_as_uint(sh[i0]) & ~m) | (__float_as_uint(sh[i0 + 4]) & m));
    }
}

__device__ __forceinline__ void relu_tile(f32x16& a) {
#pragma unroll
    for (int q = 0; q < 16; q++) a[q] = __int_as_float(max(__float_as_int(a[q]), 0));
}

// `COUNT` fragments of the global table -> LDS slots; every load of a thread is issued before its first LDS store (the trip
// count is a compile-time constant: as a plain load / store loop the copy cost one memory latency per iteration, twelve of
// them in the forward's set-up)
template <int COUNT>
__device__ __forceinline__ void load_frags(u32x4n (&v)[COUNT * 128 / 256], const uint32_t* __restrict__ frags, int first) {
    const u32x4n* src = reinterpret_cast<const u32x4n*>(frags + (size_t)first * kFragWords);
#pragma unroll
    for (int k = 0; k < COUNT * 128 / 256; k++) v[k] = src[threadIdx.x + k * 256];
}
template <int COUNT>
__device__ __forceinline__ void store_frags(u32x4n* __restrict__ fr, const u32x4n (&v)[COUNT * 128 / 256], int slot0) {
    u32x4n* dst = fr + slot0 * 128;
#pragma unroll
    for (int k = 0; k < COUNT * 128 / 256; k++) dst[threadIdx.x + k * 256] = v[k];
}

// The set-up of both kernels is ONE memory latency: the valid-row count, the first tile's inputs and the fragments are all
// requested before anything waits, and whatever needs a loaded value -- the zeros of the rows past the batch, the count's
// clamps, the LDS stores -- comes after the last request.  (As load_x, nerf_valid_tiles and the copy in a row the
// compiled code drained each of the three before it issued the next: a select sat between the loads.)
// the first tile's 16 inputs as loaded (load_x<1> without its zeros: rows s >= B of the padded batch are in bounds)
__device__ __forceinline__ void request_x_raw(const float* __restrict__ X, uint32_t tile, int j, int h, uint32_t Bp,
                                              float (&x)[16]) {
    const size_t s = (size_t)tile * 32 + j;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const float2 t = *reinterpret_cast<const float2*>(X + ((size_t)(2 * q + h) * Bp + s) * 2);
        x[2 * q] = t.x; x[2 * q + 1] = t.y;
    }
}
__device__ __forceinline__ void finish_x_raw(uint32_t tile, int j, uint32_t B, float (&x)[16]) {
    if (!((size_t)tile * 32 + j < B)) {
#pragma unroll
        for (int p = 0; p < 16; p++) x[p] = 0.0f;
    }
}
// the count cell as every lane loads it (`safe`: any readable word, for the callers without a count) ...
__device__ __forceinline__ int32_t request_valid_rows(const NerfRows& r, const uint32_t* __restrict__ safe) {
    const int32_t* p = r.valid_rows ? r.valid_rows : reinterpret_cast<const int32_t*>(safe);
    return *p;
}
// ... and nerf_valid_tiles of it, wave-uniform
__device__ __forceinline__ uint32_t finish_valid_tiles(const NerfRows& r, int32_t raw, uint32_t B, uint32_t ntiles) {
    if (!r.valid_rows) return ntiles;
    int32_t v = __builtin_amdgcn_readfirstlane(raw);
    if (r.valid_cap) v = (int32_t)r.valid_base + (v <= 0 ? 0 : (v < (int32_t)r.valid_cap ? v : (int32_t)r.valid_cap));
    const uint32_t rows = v <= 0 ? 0u : ((uint32_t)v < B ? (uint32_t)v : B);
    const uint32_t t = (rows + 31u) / 32u;
    return t < ntiles ? t : ntiles;
}

// Residency.  Rounds 4-5 shipped this kernel with ONE workgroup per CU (84 KiB of LDS, the SIMD's whole register file
// claimed): with three workgroups per CU the colour outputs of samples 16..31 of a tile came out wrong in a few per cent
// of the launches (10^-3..10^-2, different rows every launch, sigma never).  The cause is the operand hazard described in
// mlp32s_ops.h (operand_ready): the conversions that make an MFMA's 16-bit operand were not yet complete in lanes 16..31
// / 48..63 when the matrix pipe read it -- only when three wavefronts' conversions share a SIMD.  With the barrier in
// split8 / exact8 the kernel is bit-stable at any residency (tools/nerf_fwd_residency.py: 0 of 400 launches at three
// workgroups per CU, padded and unpadded builds; tests/test_gpu_mlp32.py soaks it), and the forward shares the CU again:
// 48 KiB of LDS, ~136 registers, three workgroups per CU = three wavefronts per SIMD hiding each other's MFMA and LDS
// latencies.  The backward keeps a CU to itself for what it needs (149 / 160 KiB of LDS, ~480 registers).
// (-DNERF_FWD_ONE_PER_CU: the forward as shipped in round 5's first half, for A/B runs.)
#ifndef NERF_FWD_ONE_PER_CU
#define NERF_FWD_WHOLE_SIMD() do {} while (0)
constexpr uint32_t kFwdLdsWords = 12 * 1024;              // 48 KiB: the fragments alone, three workgroups per CU
#else
#define NERF_FWD_WHOLE_SIMD() asm volatile("v_mov_b32 v255, 0\n\tv_accvgpr_write_b32 a255, 0" ::: "v255", "a255")
constexpr uint32_t kFwdLdsWords = 21 * 1024;              // 84 KiB: two workgroups do not fit a CU's 160 KiB
#endif
// the backward's wave allocation is the SIMD's whole register file (256 + 256): it needs most of it anyway
#define NERF_WHOLE_SIMD() asm volatile("v_mov_b32 v255, 0\n\tv_accvgpr_write_b32 a255, 0" ::: "v255", "a255")
#ifndef NERF_MLP_BACKWARD_UNIT
// ---------------------------------------------------------------------------------------------------- forward
__global__ void __launch_bounds__(256) k_nerf_fwd(const float* __restrict__ X, const float* __restrict__ dirs,
                                                   const uint32_t* __restrict__ frags, float* __restrict__ sigma,
                                                   float* __restrict__ rgb, uint32_t B, uint32_t out_c, NerfRows rows,
                                                   ShNorm4 nrm) {
    static_assert(NF_FWD * kFragWords <= kFwdLdsWords, "LDS");
    __shared__ __attribute__((aligned(16))) uint32_t lds[kFwdLdsWords];
    NERF_FWD_WHOLE_SIMD();
    const int lane = lane_id(), j = lane & 31, h = lane >> 5;
    const uint32_t Bp = (B + 31u) & ~31u;
    const uint32_t gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t nw = gridDim.x * 4;
    float x[16];
    const uint32_t t0 = gw < Bp / 32 ? gw : Bp / 32 - 1;          // (a wave without a tile loads the last one, unused)
    u32x4n* fr = reinterpret_cast<u32x4n*>(lds);
    typedef FragT<3> Frag;
    uint32_t ntiles;
    {
        u32x4n fv[NF_FWD * 128 / 256];
        const int32_t rows_raw = request_valid_rows(rows, frags);
        request_x_raw(X, t0, j, h, Bp, x);
        load_frags<NF_FWD>(fv, frags, 0);
        store_frags<NF_FWD>(fr, fv, 0);
        __syncthreads();
        ntiles = finish_valid_tiles(rows, rows_raw, B, Bp / 32);
    }
    finish_x_raw(t0, j, B, x);
    auto get = [&](int f) -> Frag {
        Frag w;
        w.hi = __builtin_bit_cast(bf16x8, fr[f * 128 + lane]);
        w.lo = __builtin_bit_cast(bf16x8, fr[f * 128 + 64 + lane]);
        return w;
    };
    for (uint32_t tile = gw; tile < ntiles; tile += nw) {
        const size_t s = (size_t)tile * 32 + j;
        const bool valid = s < B;
        asm volatile("" ::: "memory");                    // the operand reads stay inside the loop
        if (tile != gw) load_x<1>(X, tile, j, h, B, Bp, x);
        float d0 = 0.0f, d1 = 0.0f, d2 = 1.0f;
        if (valid) {
            d0 = dirs[s * 3]; d1 = dirs[s * 3 + 1]; d2 = dirs[s * 3 + 2];
        }
        Frag xf[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = x[8 * t + e];
            xf[t] = split8<3>(v);
        }
        // ---- sigma net
        Frag af[2][2];
#pragma unroll
        for (int ob = 0; ob < 2; ob++) {
            f32x16 a = (f32x16)(0.0f);
#pragma unroll
            for (int t = 0; t < 2; t++) a = mmap(get(F_S0 + 2 * ob + t), xf[t], a);
            relu_tile(a);
            split_tile<3>(a, af[ob]);
        }
        f32x16 os = (f32x16)(0.0f);
#pragma unroll
        for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int t = 0; t < 2; t++) os = mmap(get(F_SO + 2 * ib + t), af[ib][t], os);
        if (valid && h == 0) sigma[s] = expf(os[0]);
        // ---- colour net: K-step 0 = the sigma net's outputs (registers 0..7: outputs nrow(e, h)), K-step 1 = SH
        Frag in[2];
        {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = os[e];
            in[0] = split8<3>(v);
            sh_slots(d0, d1, d2, nrm, h, v);
            in[1] = split8<3>(v);
        }
#pragma unroll
        for (int ob = 0; ob < 2; ob++) {
            f32x16 a = (f32x16)(0.0f);
#pragma unroll
            for (int t = 0; t < 2; t++) a = mmap(get(F_C0 + 2 * ob + t), in[t], a);
            relu_tile(a);
            split_tile<3>(a, af[ob]);
        }
        Frag bf[2][2];
#pragma unroll
        for (int ob = 0; ob < 2; ob++) {
            f32x16 n = (f32x16)(0.0f);
#pragma unroll
            for (int ib = 0; ib < 2; ib++)
#pragma unroll
                for (int t = 0; t < 2; t++) n = mmap(get(F_CH + (ob * 2 + ib) * 2 + t), af[ib][t], n);
            relu_tile(n);
            split_tile<3>(n, bf[ob]);
        }
        f32x16 o = (f32x16)(0.0f);
#pragma unroll
        for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int t = 0; t < 2; t++) o = mmap(get(F_CO + 2 * ib + t), bf[ib][t], o);
        // outputs r < out_c sit in the accumulator registers of lane half r / 4 mod 2: r = nrow(q, h)
        if (valid) {
            if (h == 0) {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if ((uint32_t)q < out_c) rgb[s * out_c + q] = out_act_fwd(o[q], 3);
            }
            if (out_c > 4) {
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const uint32_t r = (uint32_t)nrow(q, h);
                    if (r >= 4 && r < out_c) rgb[s * out_c + r] = out_act_fwd(o[q], 3);
                }
            }
        }
    }
}

#endif
#ifdef NERF_MLP_BACKWARD_UNIT
// ---------------------------------------------------------------------------------------------------- backward
struct NerfBwdArgs {
    const float* X;            // [16, Bp, 2]
    const float* dirs;         // [B, 3]
    const float* g_rgb;        // [B, out_c]   dL/d rgb (after the sigmoid)
    const float* rgb;          // [B, out_c]   the forward's rgb
    const float* g_sigma;      // [B]          dL/d sigma (after trunc_exp)
    float sigma_scale;         // multiplies g_sigma (the renderer's density_scale)
    float* dX;                 // [16, Bp, 2]
    float* partial;            // [gridDim.x][P_STRIDE]
    uint32_t B, out_c;
    NerfRows rows;
};

// Register budget: the twelve weight-gradient accumulators (192 registers) live in the AGPR half of the file; the arch
// half holds a tile's working set, which therefore must stay small: the selection matrices of the flips (FLIP_MFMA, below)
// sit in LDS, and the
// two hidden activations that are needed again much later (sigma net hidden layer, colour net first layer) are stashed in
// LDS as the operand halves they were split into (a private 16 KiB per wave: no fence, no barrier) -- the ReLU mask of the
// backward is read off the stashed hi half (an activation is positive iff its bf16 rounding is non-zero).
constexpr uint32_t kSelWords = 5 * 256;                                  // five selection matrices, 64 lanes x 16 B
constexpr uint32_t kStashWords = 8 * 512;                                // per wave: 2 layers x [2 blocks][2 K-steps] fragments
constexpr uint32_t kBwdLdsWords = NF_BWD * kFragWords + kSelWords + 4 * kStashWords;

// How an operand of a weight-gradient product (which contracts over the samples a D tile keeps on the lanes) is transposed.
//   FLIP_MFMA: on the matrix pipe, by products with 0/1 selection matrices (flip_tile / flip_natural of mlp32s_ops.h);
//   FLIP_LDS : through a per-wave LDS image [32 samples][32 neurons] of the 16-bit halves, 64-byte rows: the lane of sample j
//              stores its packed quads (8 bytes: neurons 4k .. 4k+3 of K-step t = k / 4) into row j, and ds_read_b64_tr_b16
//              hands lane (c, h) neuron c of samples 16t + 8u + 4h + 0..3 -- elements 4u .. 4u+3 of K-step t, the very
//              slots the selection matrices fill (nrow(8t + e, h)): every weight-gradient MFMA sees the same operand bits.
//              The 8-byte chunk k of row j sits at chunk position k ^ ((j >> 1) & 7): a transposed read takes four whole
//              rows per 32-lane half (256 contiguous bytes, every bank once) whatever the permutation inside a row, and the
//              sixteen lanes of a ds_write_b64 group, one row each, then cover all 32 banks instead of 4.
//              Five images of 4 KiB (hi + lo) per wave: the two stashed activations (read by rows for the ReLU mask AND
//              transposed for the weight gradient -- no second copy), and one scratch; an image takes the next operand as
//              soon as its tenant is dead.  A wave's LDS operations execute in order and the images are private to the
//              wave: no barrier, no wait between a store and the read of another lane's data.
enum { FLIP_MFMA = 0, FLIP_LDS = 1 };
constexpr uint32_t kImgBytes = 4096, kImgLo = 2048, kWaveImages = 5;
constexpr uint32_t kBwdLdsWordsTr = NF_BWD * kFragWords + 4 * kWaveImages * (kImgBytes / 4);
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
__device__ __forceinline__ bf16x8 tr_read8(const unsigned char* p0, const unsigned char* p1) {
    const s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);       // ds_read_b64_tr_b16
    const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7));
}
// the compiler reasons about one lane's addresses; a transposed read takes other lanes' stores
#define NERF_IMG_FENCE() asm volatile("" ::: "memory")

// g[q] = (element q of the tile whose K-step fragments' hi halves are hi[0], hi[1] is non-zero) ? g[q] : 0   (bf16 pairs)
__device__ __forceinline__ void mask_by_hi(f32x16& g, const bf16x8 (&hi)[2]) {
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const i32x4 w = __builtin_bit_cast(i32x4, hi[t]);
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const uint32_t u = (uint32_t)w[p];
            g[8 * t + 2 * p] = (u & 0xffffu) != 0u ? g[8 * t + 2 * p] : 0.0f;
            g[8 * t + 2 * p + 1] = u > 0xffffu ? g[8 * t + 2 * p + 1] : 0.0f;
        }
    }
}
__device__ __forceinline__ void mask_by_frag(f32x16& g, const FragT<3> (&f)[2]) {
    const bf16x8 hi[2] = {f[0].hi, f[1].hi};
    mask_by_hi(g, hi);
}

// The kernel's body; `lds`: the workgroup's kBwdLdsWords (FLIP_MFMA: operands, then the dW sums; selectors; stashes) or
// kBwdLdsWordsTr (FLIP_LDS: operands; five images per wave) dwords.
// How the four waves' weight-gradient accumulators become the workgroup's partial sum (w0 + w2) + (w1 + w3):
//   TAIL_TWO_PHASE   : waves 0 / 1 store into a region each, barrier, waves 2 / 3 add into the same regions, barrier, one
//                      pass adds the two regions (2 * P_STRIDE dwords of LDS: all the matrix-pipe form has to spare);
//   TAIL_FOUR_REGIONS: every wave stores into a region of its own, barrier, one pass reads the four (16 bytes per lane and
//                      region, every read of a thread issued before its first add) and adds them in the same association.
enum { TAIL_TWO_PHASE = 0, TAIL_FOUR_REGIONS = 1 };
template <int TR, int TAIL>
__device__ __forceinline__ void nerf_bwd_body(uint32_t* lds, const NerfBwdArgs& a, const uint32_t* __restrict__ frags,
                                              const ShNorm4& nrm) {
    static_assert(NF_BWD * kFragWords >= 2 * P_STRIDE, "the two sum regions reuse the operand area");
    static_assert(TAIL == TAIL_TWO_PHASE || (TR == FLIP_LDS && kBwdLdsWordsTr >= 4 * P_STRIDE),
                  "four sum regions need 4 * P_STRIDE dwords: the LDS-transpose form's operands + images");
    static_assert(P_STRIDE % 4 == 0 && (NW_S + HID * IN + HID * HID) % 4 == 0 && HID % 4 == 0, "16-byte reads of the sums");
    static_assert(kBwdLdsWords * 4 <= 160 * 1024 && kBwdLdsWordsTr * 4 <= 160 * 1024, "LDS");
#if defined(MLP32S_NO_OPERAND_BARRIER)
    // nerf_mlp_bwd.hip compiles this kernel without the operand barrier: sound only while ONE workgroup of it fits a CU,
    // i.e. one wavefront per SIMD (mlp32s_ops.h: operand_ready).  More than half of the CU's 160 KiB of LDS guarantees it.
    static_assert(kBwdLdsWords * 4 > 80 * 1024 && kBwdLdsWordsTr * 4 > 80 * 1024,
                  "k_nerf_bwd without the operand barrier must stay at one workgroup per CU");
#endif
    NERF_WHOLE_SIMD();
    typedef FragT<3> Frag;
    const int lane = lane_id(), j = lane & 31, h = lane >> 5;
    const int wid = threadIdx.x >> 6;
    const uint32_t B = a.B, out_c = a.out_c;
    const uint32_t Bp = (B + 31u) & ~31u;
    const uint32_t ntiles = Bp / 32;
    const uint32_t gw = blockIdx.x * 4 + wid;
    const uint32_t nw = gridDim.x * 4;

    // everything a tile reads from global memory is requested for the wave's NEXT tile where the current tile has used it
    // for the last time, into the same registers
    float x[16], dy_raw[4], ys_raw[4], ds_raw = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 1.0f;
    auto request_x = [&](uint32_t t) { load_x<1>(a.X, t, j, h, B, Bp, x); };
    auto request_out = [&](uint32_t t) {
        const size_t sn = (size_t)t * 32 + j;
        const size_t sc = sn < B ? sn : (size_t)B - 1;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t oc = (uint32_t)e < out_c ? (uint32_t)e : out_c - 1;
            dy_raw[e] = a.g_rgb[sc * out_c + oc];
            ys_raw[e] = a.rgb[sc * out_c + oc];
        }
        ds_raw = a.g_sigma[sc];
        d0 = a.dirs[sc * 3]; d1 = a.dirs[sc * 3 + 1]; d2 = a.dirs[sc * 3 + 2];
    };
    u32x4n* fr = reinterpret_cast<u32x4n*>(lds);
    u32x4n* sel = fr + NF_BWD * 128;                     // [kind][lane]
    u32x4n* stash = sel + 5 * 64 + wid * (kStashWords / 4);      // this wave's: [layer][block][K-step][hi, lo][lane]
    // set-up: the count, the first tile's inputs (its index needs no count) and all 40 fragments are requested before the
    // first wait -- the wave owns the SIMD's register file, the fragments sit in registers beside the tile's inputs
    const uint32_t t0 = gw < ntiles ? gw : ntiles - 1;
    const int32_t rows_raw = request_valid_rows(a.rows, frags);
    request_x_raw(a.X, t0, j, h, Bp, x);
    request_out(t0);
    {
        u32x4n fv0[10], fv1[10];
        load_frags<20>(fv0, frags, 0);
        load_frags<20>(fv1, frags, B_COT);
        store_frags<20>(fr, fv0, 0);
        store_frags<20>(fr, fv1, 20);
    }
    if (TR == FLIP_MFMA && wid == 0) {
        // selection matrices of the flips: natural order (dL/dY), a tile's two register halves, and X^T (K-step t of the
        // input operand holds input columns kmap<1>(8t + e, h))
        sel[0 * 64 + lane] = __builtin_bit_cast(u32x4n, selector(j, h, 0));
        sel[1 * 64 + lane] = __builtin_bit_cast(u32x4n, selector(j, h, 1));
        sel[2 * 64 + lane] = __builtin_bit_cast(u32x4n, selector(j, h, 2));
#pragma unroll
        for (int t = 0; t < 2; t++) {
            bf16x8 sx;
#pragma unroll
            for (int e = 0; e < 8; e++) sx[e] = kmap<1>(8 * t + e, h) == j ? (elem16)1.0f : (elem16)0.0f;
            sel[(3 + t) * 64 + lane] = __builtin_bit_cast(u32x4n, sx);
        }
    }
    __syncthreads();
    const uint32_t nreal = finish_valid_tiles(a.rows, rows_raw, B, ntiles);      // the tile loop's bound and its skips
    finish_x_raw(t0, j, B, x);
    auto get = [&](int f) -> Frag {                      // f: index in the global table
        const int slot = f < 20 ? f : f - 4;
        Frag w;
        w.hi = __builtin_bit_cast(bf16x8, fr[slot * 128 + lane]);
        w.lo = __builtin_bit_cast(bf16x8, fr[slot * 128 + 64 + lane]);
        return w;
    };
    auto SEL = [&](int k) -> bf16x8 { return __builtin_bit_cast(bf16x8, sel[k * 64 + lane]); };
    auto put_stash = [&](int layer, int ib, const Frag (&f)[2]) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            u32x4n* p = stash + (((layer * 2 + ib) * 2 + t) * 2) * 64 + lane;
            p[0] = __builtin_bit_cast(u32x4n, f[t].hi);
            p[64] = __builtin_bit_cast(u32x4n, f[t].lo);
        }
    };
    auto get_stash = [&](int layer, int ib, Frag (&f)[2]) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const u32x4n* p = stash + (((layer * 2 + ib) * 2 + t) * 2) * 64 + lane;
            f[t].hi = __builtin_bit_cast(bf16x8, p[0]);
            f[t].lo = __builtin_bit_cast(bf16x8, p[64]);
        }
    };
    // ---- FLIP_LDS: this wave's images 0, 1 (sigma net hidden layer), 2, 3 (colour net first layer), 4 (scratch); byte offsets
    // inside an image half.  Stores: row j, chunk k at wr0 ^ (8 * (k ^ h)) for the quads of a D tile's operands (k = 4t + 2u + h),
    // wn0 ^ 8u for an operand in natural order (k = 2h + u), wx0 ^ 8k (+ 4h inside the chunk) for the pairs of X's operands.
    // Transposed reads: lane 4q + p of a 16-lane group supplies row 16t + 8u + 4h + q, chunk 4 (j / 16) + p.
    unsigned char* img0 = reinterpret_cast<unsigned char*>(fr + NF_BWD * 128) + wid * (kWaveImages * kImgBytes);
    const uint32_t swz = (uint32_t)(j >> 1) & 7u;
    const uint32_t wr0 = 64u * j + 8u * ((uint32_t)h ^ swz);
    const uint32_t wn0 = 64u * j + 8u * ((uint32_t)(2 * h) ^ swz);
    const uint32_t wx0 = 64u * j + 8u * swz + 4u * h;
    auto tr_off = [&](int u) -> uint32_t {
        const uint32_t row = 8u * u + 4u * h + (uint32_t)((j & 15) >> 2), k = 4u * (j >> 4) + (uint32_t)(j & 3);
        return 64u * row + 8u * (k ^ ((row >> 1) & 7u));                 // (+ 1024 t: sixteen rows on, the same swizzle)
    };
    const uint32_t tr0 = tr_off(0), tr1 = tr_off(1);
    auto put_quads = [&](unsigned char* p, const bf16x8& v, uint32_t at) {         // elements 0..3 -> at, 4..7 -> at ^ 16
        const i32x4 w = __builtin_bit_cast(i32x4, v);
        *reinterpret_cast<uint2*>(p + at) = make_uint2((uint32_t)w[0], (uint32_t)w[1]);
        *reinterpret_cast<uint2*>(p + (at ^ 16u)) = make_uint2((uint32_t)w[2], (uint32_t)w[3]);
    };
    auto put_img = [&](int img, const Frag (&f)[2]) {    // the operands of a D tile (or of the colour net's input)
        unsigned char* p = img0 + img * kImgBytes;
        NERF_IMG_FENCE();
#pragma unroll
        for (int t = 0; t < 2; t++) {
            put_quads(p, f[t].hi, wr0 ^ (32u * t));
            put_quads(p + kImgLo, f[t].lo, wr0 ^ (32u * t));
        }
        NERF_IMG_FENCE();
    };
    auto put_nat = [&](int img, const Frag& f, bool acc_order) {      // one K-step of outputs: 8h + e, or nrow(e, h)
        unsigned char* p = img0 + img * kImgBytes;
        NERF_IMG_FENCE();
        if (acc_order) {
            put_quads(p, f.hi, wr0);
            put_quads(p + kImgLo, f.lo, wr0);
        } else {
            const i32x4 wh = __builtin_bit_cast(i32x4, f.hi), wl = __builtin_bit_cast(i32x4, f.lo);
#pragma unroll
            for (int u = 0; u < 2; u++) {
                *reinterpret_cast<uint2*>(p + (wn0 ^ (8u * u))) = make_uint2((uint32_t)wh[2 * u], (uint32_t)wh[2 * u + 1]);
                *reinterpret_cast<uint2*>(p + kImgLo + (wn0 ^ (8u * u))) = make_uint2((uint32_t)wl[2 * u], (uint32_t)wl[2 * u + 1]);
            }
        }
        NERF_IMG_FENCE();
    };
    auto put_x = [&](int img, const Frag (&f)[2]) {      // X's operands: element pair m of K-step t = columns 16t + 4m + 2h + {0, 1}
        unsigned char* p = img0 + img * kImgBytes;
        NERF_IMG_FENCE();
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const i32x4 wh = __builtin_bit_cast(i32x4, f[t].hi), wl = __builtin_bit_cast(i32x4, f[t].lo);
#pragma unroll
            for (int m = 0; m < 4; m++) {
                *reinterpret_cast<uint32_t*>(p + (wx0 ^ (32u * t + 8u * m))) = (uint32_t)wh[m];
                *reinterpret_cast<uint32_t*>(p + kImgLo + (wx0 ^ (32u * t + 8u * m))) = (uint32_t)wl[m];
            }
        }
        NERF_IMG_FENCE();
    };
    auto get_T = [&](int img, Frag (&out)[2]) {          // the image's transpose: what flip_tile returns
        const unsigned char* p = img0 + img * kImgBytes;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            out[t].hi = tr_read8(p + 1024 * t + tr0, p + 1024 * t + tr1);
            out[t].lo = tr_read8(p + kImgLo + 1024 * t + tr0, p + kImgLo + 1024 * t + tr1);
        }
    };
    auto get_T_nat = [&](int img, Frag (&out)[2]) {      // what flip_natural returns: outputs 16..31 do not exist (a select: the
        get_T(img, out);                                 // transposed read itself needs every lane)
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const i32x4 zh = __builtin_bit_cast(i32x4, out[t].hi), zl = __builtin_bit_cast(i32x4, out[t].lo);
            out[t].hi = __builtin_bit_cast(bf16x8, j < 16 ? zh : (i32x4)(0));
            out[t].lo = __builtin_bit_cast(bf16x8, j < 16 ? zl : (i32x4)(0));
        }
    };
    auto get_rows_hi = [&](int img, bf16x8 (&hi)[2]) {   // the hi halves as put_img stored them (the ReLU mask's source)
        const unsigned char* p = img0 + img * kImgBytes;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const uint2 q0 = *reinterpret_cast<const uint2*>(p + (wr0 ^ (32u * t)));
            const uint2 q1 = *reinterpret_cast<const uint2*>(p + (wr0 ^ (32u * t) ^ 16u));
            const i32x4 w = {(int)q0.x, (int)q0.y, (int)q1.x, (int)q1.y};
            hi[t] = __builtin_bit_cast(bf16x8, w);
        }
    };

    f32x16 aw0S[2], awoS[2], aw0C[2], awhC[2][2], awoC[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        aw0S[k] = (f32x16)(0.0f); awoS[k] = (f32x16)(0.0f); aw0C[k] = (f32x16)(0.0f); awoC[k] = (f32x16)(0.0f);
        awhC[k][0] = (f32x16)(0.0f); awhC[k][1] = (f32x16)(0.0f);
    }

    for (uint32_t tile = gw; tile < ntiles; tile += nw) {
        const uint32_t tnext = tile + nw < nreal ? tile + nw : tile;
        const size_t s = (size_t)tile * 32 + j;
        const bool valid = s < B;
        asm volatile("" ::: "memory");
        if (tile >= nreal) {                             // the sample budget's padding: zero input gradients, nothing else
#pragma unroll
            for (int gq = 0; gq < 4; gq++) {
                const size_t lv = (size_t)(4 * gq + 2 * h);
                *reinterpret_cast<float2*>(a.dX + (lv * Bp + s) * 2) = make_float2(0.f, 0.f);
                *reinterpret_cast<float2*>(a.dX + ((lv + 1) * Bp + s) * 2) = make_float2(0.f, 0.f);
            }
            continue;
        }
        // ---- both forwards again, instruction for instruction (k_nerf_fwd)
        Frag xop[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = x[8 * t + e];
            xop[t] = split8<3>(v);
        }
        request_x(tnext);
        f32x16 os = (f32x16)(0.0f);
        {
            Frag af[2][2];
#pragma unroll
            for (int ob = 0; ob < 2; ob++) {
                f32x16 t0 = (f32x16)(0.0f);
#pragma unroll
                for (int t = 0; t < 2; t++) t0 = mmap(get(F_S0 + 2 * ob + t), xop[t], t0);
                relu_tile(t0);
                split_tile<3>(t0, af[ob]);
                if constexpr (TR == FLIP_LDS) put_img(ob, af[ob]);
                else put_stash(0, ob, af[ob]);
            }
#pragma unroll
            for (int ib = 0; ib < 2; ib++)
#pragma unroll
                for (int t = 0; t < 2; t++) os = mmap(get(F_SO + 2 * ib + t), af[ib][t], os);
        }
        const float h0 = os[0];                          // (lanes of half 0: the raw density)
        Frag inop[2];
        {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = os[e];
            inop[0] = split8<3>(v);
            sh_slots(valid ? d0 : 0.0f, valid ? d1 : 0.0f, valid ? d2 : 1.0f, nrm, h, v);
            inop[1] = split8<3>(v);
        }
        Frag c1f[2][2];                                  // the colour net's second hidden layer, as operands
        {
            Frag af[2][2];
#pragma unroll
            for (int ob = 0; ob < 2; ob++) {
                f32x16 t0 = (f32x16)(0.0f);
#pragma unroll
                for (int t = 0; t < 2; t++) t0 = mmap(get(F_C0 + 2 * ob + t), inop[t], t0);
                relu_tile(t0);
                split_tile<3>(t0, af[ob]);
                if constexpr (TR == FLIP_LDS) put_img(2 + ob, af[ob]);
                else put_stash(1, ob, af[ob]);
            }
#pragma unroll
            for (int ob = 0; ob < 2; ob++) {
                f32x16 n = (f32x16)(0.0f);
#pragma unroll
                for (int ib = 0; ib < 2; ib++)
#pragma unroll
                    for (int t = 0; t < 2; t++) n = mmap(get(F_CH + (ob * 2 + ib) * 2 + t), af[ib][t], n);
                relu_tile(n);
                split_tile<3>(n, c1f[ob]);
            }
        }
        // ---- colour net, output layer: dL/dY = (dY (1 - y)) y  (torch's sigmoid_backward), outputs in natural order
        Frag dyf;
        {
            float dy[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float gq = 0.0f;
                if (e < 4) gq = (dy_raw[e] * (1.0f - ys_raw[e])) * ys_raw[e];
                dy[e] = (valid && h == 0 && (uint32_t)e < out_c) ? gq : 0.0f;
            }
            if (out_c > 4) {                             // (wider colour outputs: not prefetched, read here)
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const uint32_t o = (uint32_t)(8 * h + e);
                    if (o >= 4 && o < out_c && valid) {
                        const float y = a.rgb[s * out_c + o];
                        dy[e] = (a.g_rgb[s * out_c + o] * (1.0f - y)) * y;
                    }
                }
            }
            dyf = split8<3>(dy);
        }
        const float dsig = valid ? (ds_raw * a.sigma_scale) * expf(fminf(fmaxf(h0, -15.0f), 15.0f)) : 0.0f;
        request_out(tnext);
        Frag gf[2][2], gT[2][2];                         // a layer's output gradient: as operands, and flipped
        if constexpr (TR == FLIP_LDS) {
            // everything passes through the scratch image, in program order (a store follows the reads of its predecessor)
            Frag dyT[2];
            put_nat(4, dyf, false);
            get_T_nat(4, dyT);
            put_img(4, c1f[0]);
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                f32x16 g = mmap(get(B_COT + ib), dyf, (f32x16)(0.0f));
                mask_by_frag(g, c1f[ib]);
                Frag ft[2];
                get_T(4, ft);
                if (ib == 0) put_img(4, c1f[1]);
#pragma unroll
                for (int t = 0; t < 2; t++) awoC[ib] = mmap(dyT[t], ft[t], awoC[ib]);
                split_tile<3>(g, gf[ib]);
            }
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                put_img(4, gf[ib]);
                get_T(4, gT[ib]);
            }
            put_img(4, inop);                            // (waits there for the colour net's input layer)
        } else {
            Frag dyT[2];
            flip_natural<3>(dyf, SEL(0), dyT);
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                f32x16 g = mmap(get(B_COT + ib), dyf, (f32x16)(0.0f));
                mask_by_frag(g, c1f[ib]);
                Frag ft[2];
                flip_tile<3>(c1f[ib], SEL(1), SEL(2), ft);
#pragma unroll
                for (int t = 0; t < 2; t++) awoC[ib] = mmap(dyT[t], ft[t], awoC[ib]);
                split_tile<3>(g, gf[ib]);
            }
#pragma unroll
            for (int ib = 0; ib < 2; ib++) flip_tile<3>(gf[ib], SEL(1), SEL(2), gT[ib]);
        }
        // ---- colour net, hidden layer
        if constexpr (TR == FLIP_LDS) {
            Frag g0f[2][2];
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                f32x16 n = (f32x16)(0.0f);
#pragma unroll
                for (int ob = 0; ob < 2; ob++)
#pragma unroll
                    for (int t = 0; t < 2; t++) n = mmap(get(B_CHT + (ib * 2 + ob) * 2 + t), gf[ob][t], n);
                bf16x8 c0hi[2];
                Frag ft[2];
                get_rows_hi(2 + ib, c0hi);
                mask_by_hi(n, c0hi);
                get_T(2 + ib, ft);
#pragma unroll
                for (int ob = 0; ob < 2; ob++)
#pragma unroll
                    for (int t = 0; t < 2; t++) awhC[ob][ib] = mmap(gT[ob][t], ft[t], awhC[ob][ib]);
                split_tile<3>(n, g0f[ib]);
                put_img(2 + ib, g0f[ib]);                // (the stashed activation is dead: its image takes the gradient)
            }
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                gf[ib][0] = g0f[ib][0];
                gf[ib][1] = g0f[ib][1];
                get_T(2 + ib, gT[ib]);
            }
            put_x(2, xop);                               // (waits there for the sigma net's input layer)
        } else {
            Frag g0f[2][2];
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                f32x16 n = (f32x16)(0.0f);
#pragma unroll
                for (int ob = 0; ob < 2; ob++)
#pragma unroll
                    for (int t = 0; t < 2; t++) n = mmap(get(B_CHT + (ib * 2 + ob) * 2 + t), gf[ob][t], n);
                Frag c0f[2], ft[2];
                get_stash(1, ib, c0f);
                mask_by_frag(n, c0f);
                flip_tile<3>(c0f, SEL(1), SEL(2), ft);
#pragma unroll
                for (int ob = 0; ob < 2; ob++)
#pragma unroll
                    for (int t = 0; t < 2; t++) awhC[ob][ib] = mmap(gT[ob][t], ft[t], awhC[ob][ib]);
                split_tile<3>(n, g0f[ib]);
            }
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                gf[ib][0] = g0f[ib][0];
                gf[ib][1] = g0f[ib][1];
                flip_tile<3>(gf[ib], SEL(1), SEL(2), gT[ib]);
            }
        }
        // ---- colour net, input layer: its input's transpose is a flip like any other (K-step 0: columns nrow(e, h),
        // K-step 1: 16 + nrow(e, h) -- the selection matrices of a tile's two register halves)
        Frag dysf;
        {
            Frag inT[2];
            if constexpr (TR == FLIP_LDS) get_T(4, inT);
            else flip_tile<3>(inop, SEL(1), SEL(2), inT);
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int t = 0; t < 2; t++) aw0C[ob] = mmap(gT[ob][t], inT[t], aw0C[ob]);
            f32x16 d = (f32x16)(0.0f);
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int t = 0; t < 2; t++) d = mmap(get(B_C0T + 2 * ob + t), gf[ob][t], d);
            // rows 0..15 of d (registers 0..7) = dL/d(sigma net outputs nrow(e, h)); output 0 went through trunc_exp
            float dys[8];
#pragma unroll
            for (int e = 0; e < 8; e++) dys[e] = d[e];
            if (h == 0) dys[0] = dsig;
            dysf = split8<3>(dys);
        }
        // ---- sigma net, output layer
        if constexpr (TR == FLIP_LDS) {
            Frag dyT[2];
            put_nat(4, dysf, true);                      // (slots in accumulator order)
            get_T_nat(4, dyT);
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                f32x16 g = mmap(get(B_SOT + ib), dysf, (f32x16)(0.0f));
                bf16x8 ashi[2];
                Frag ft[2];
                get_rows_hi(ib, ashi);
                mask_by_hi(g, ashi);
                get_T(ib, ft);
#pragma unroll
                for (int t = 0; t < 2; t++) awoS[ib] = mmap(dyT[t], ft[t], awoS[ib]);
                split_tile<3>(g, gf[ib]);
                put_img(ib, gf[ib]);
            }
#pragma unroll
            for (int ib = 0; ib < 2; ib++) get_T(ib, gT[ib]);
        } else {
            Frag dyT[2];
            flip_natural<3>(dysf, SEL(1), dyT);          // (slots in accumulator order: the first half's selection matrix)
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                f32x16 g = mmap(get(B_SOT + ib), dysf, (f32x16)(0.0f));
                Frag asf[2], ft[2];
                get_stash(0, ib, asf);
                mask_by_frag(g, asf);
                flip_tile<3>(asf, SEL(1), SEL(2), ft);
#pragma unroll
                for (int t = 0; t < 2; t++) awoS[ib] = mmap(dyT[t], ft[t], awoS[ib]);
                split_tile<3>(g, gf[ib]);
            }
#pragma unroll
            for (int ib = 0; ib < 2; ib++) flip_tile<3>(gf[ib], SEL(1), SEL(2), gT[ib]);
        }
        // ---- sigma net, input layer
        {
            Frag xT[2];
            if constexpr (TR == FLIP_LDS) get_T(2, xT);
            else flip_tile<3>(xop, SEL(3), SEL(4), xT);
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int t = 0; t < 2; t++) aw0S[ob] = mmap(gT[ob][t], xT[t], aw0S[ob]);
            f32x16 d = (f32x16)(0.0f);
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int t = 0; t < 2; t++) d = mmap(get(B_S0T + 2 * ob + t), gf[ob][t], d);
#pragma unroll
            for (int gq = 0; gq < 4; gq++) {
                const size_t lv = (size_t)(4 * gq + 2 * h);
                *reinterpret_cast<float2*>(a.dX + (lv * Bp + s) * 2) = make_float2(d[4 * gq], d[4 * gq + 1]);
                *reinterpret_cast<float2*>(a.dX + ((lv + 1) * Bp + s) * 2) = make_float2(d[4 * gq + 2], d[4 * gq + 3]);
            }
        }
    }

    // per-workgroup sums in a fixed order (deterministic): (w0 + w2) + (w1 + w3) leaves as this workgroup's partial sum;
    // the operands and the images are dead after this barrier
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds) + (size_t)(TAIL == TAIL_FOUR_REGIONS ? wid : (wid & 1)) * P_STRIDE;
    const uint32_t NW_C = HID * IN + HID * HID + out_c * HID;
    auto flush = [&](const f32x16& acc, uint32_t base, int ld, int ob, int nb, uint32_t nrows, bool add) {
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const uint32_t o = (uint32_t)(32 * ob + nrow(q, h));
            if (o < nrows) {
                float* p = red + base + o * ld + 32 * nb + j;
                *p = add ? *p + acc[q] : acc[q];
            }
        }
    };
    auto flush_all = [&](bool add) {
#pragma unroll
        for (int ob = 0; ob < 2; ob++) flush(aw0S[ob], 0, IN, ob, 0, HID, add);
#pragma unroll
        for (int nb = 0; nb < 2; nb++) flush(awoS[nb], HID * IN, HID, 0, nb, 16, add);
#pragma unroll
        for (int ob = 0; ob < 2; ob++) flush(aw0C[ob], NW_S, IN, ob, 0, HID, add);
#pragma unroll
        for (int ob = 0; ob < 2; ob++)
#pragma unroll
            for (int nb = 0; nb < 2; nb++) flush(awhC[ob][nb], NW_S + HID * IN, HID, ob, nb, HID, add);
#pragma unroll
        for (int nb = 0; nb < 2; nb++) flush(awoC[nb], NW_S + HID * IN + HID * HID, HID, 0, nb, out_c, add);
    };
    float* dst = a.partial + (size_t)blockIdx.x * P_STRIDE;
    if constexpr (TAIL == TAIL_FOUR_REGIONS) {
        flush_all(false);
        __syncthreads();
        // thread i: float4 i, i + 256, ... of the sums -- its whole strip is read before the first add
        constexpr uint32_t kStrip = (P_STRIDE / 4 + 255) / 256;
        const uint32_t total4 = (NW_S + NW_C) / 4;
        const float4* r = reinterpret_cast<const float4*>(lds);
        float4 v[kStrip][4];
#pragma unroll
        for (uint32_t k = 0; k < kStrip; k++) {
            const uint32_t i = threadIdx.x + k * 256;
            if (i < total4) {
#pragma unroll
                for (uint32_t w = 0; w < 4; w++) v[k][w] = r[w * (P_STRIDE / 4) + i];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kStrip; k++) {
            const uint32_t i = threadIdx.x + k * 256;
            if (i < total4) {
                float4 o;
                o.x = (v[k][0].x + v[k][2].x) + (v[k][1].x + v[k][3].x);
                o.y = (v[k][0].y + v[k][2].y) + (v[k][1].y + v[k][3].y);
                o.z = (v[k][0].z + v[k][2].z) + (v[k][1].z + v[k][3].z);
                o.w = (v[k][0].w + v[k][2].w) + (v[k][1].w + v[k][3].w);
                reinterpret_cast<float4*>(dst)[i] = o;
            }
        }
    } else {
        if (wid < 2) flush_all(false);
        __syncthreads();
        if (wid >= 2) flush_all(true);
        __syncthreads();
        const float* r0 = reinterpret_cast<const float*>(lds);
        for (uint32_t i = threadIdx.x; i < NW_S + NW_C; i += blockDim.x) dst[i] = r0[i] + r0[P_STRIDE + i];
    }
}

// The two forms as kernels: k_nerf_bwd transposes through LDS (the default), k_nerf_bwd_mfma on the matrix pipe (the form
// shipped before; enerf_debug_nerf_bwd_transpose(0) selects it for A/B runs and for the bit-identity test).
// The LDS form's 160 KiB hold four sum regions exactly; the matrix-pipe form's 149 KiB do not (it keeps the two-phase sums:
// the comparator of tests/test_gpu_nerf_bwd_sums.py).  -DNERF_BWD_TWO_PHASE_TAIL: the default form with the two-phase sums,
// for A/B timing only.
#ifdef NERF_BWD_TWO_PHASE_TAIL
constexpr int kBwdTail = TAIL_TWO_PHASE;
#else
constexpr int kBwdTail = TAIL_FOUR_REGIONS;
#endif
__global__ void __launch_bounds__(256) k_nerf_bwd(NerfBwdArgs a, const uint32_t* __restrict__ frags, ShNorm4 nrm) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kBwdLdsWordsTr];
    nerf_bwd_body<FLIP_LDS, kBwdTail>(lds, a, frags, nrm);
}
__global__ void __launch_bounds__(256) k_nerf_bwd_mfma(NerfBwdArgs a, const uint32_t* __restrict__ frags, ShNorm4 nrm) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kBwdLdsWords];
    nerf_bwd_body<FLIP_MFMA, TAIL_TWO_PHASE>(lds, a, frags, nrm);
}

#endif
// ---------------------------------------------------------------------------------------------------- launchers
#ifdef NERF_MLP_BACKWARD_UNIT
#define k_nerf_mark k_nerf_mark_bwd_unit          // (one marker kernel per translation unit)
#endif
__global__ void k_nerf_mark() {}

#ifndef NERF_MLP_BACKWARD_UNIT
void nerf_launch_frags(const float* ws0, const float* ws1, const float* wc0, const float* wc1, const float* wc2,
                       uint32_t w0_cols, uint32_t out_c, uint32_t* frags, hipStream_t s) {
    hipLaunchKernelGGL(k_nerf_frags, dim3(NF_ALL), dim3(64), 0, s, ws0, ws1, wc0, wc1, wc2, w0_cols, out_c, frags);
}

void nerf_launch_frag_map(uint32_t w0_cols, uint32_t out_c, uint32_t* map, hipStream_t s) {
    hipLaunchKernelGGL(k_nerf_frag_map, dim3(NF_ALL), dim3(64), 0, s, w0_cols, out_c, map);
}

void nerf_launch_fwd(const float* X, const float* dirs, const uint32_t* frags, float* sigma, float* rgb, uint32_t B,
                     uint32_t out_c, const int32_t* valid_rows, uint32_t valid_base, uint32_t valid_cap, uint32_t grid,
                     hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (ev_start) hipExtLaunchKernelGGL(k_nerf_mark, dim3(1), dim3(64), 0, s, nullptr, ev_start, 0);
    hipExtLaunchKernelGGL(k_nerf_fwd, dim3(grid), dim3(256), 0, s, nullptr, ev_stop, 0, X, dirs, frags, sigma, rgb, B, out_c,
                          NerfRows{valid_rows, valid_base, valid_cap}, make_sh_norm4());
}

#else
#ifndef NERF_BWD_TRANSPOSE_DEFAULT
#define NERF_BWD_TRANSPOSE_DEFAULT 1
#endif
static int g_nerf_bwd_transpose = NERF_BWD_TRANSPOSE_DEFAULT;      // enerf_debug_nerf_bwd_transpose
void nerf_launch_bwd(const float* X, const float* dirs, const float* g_rgb, const float* rgb, const float* g_sigma,
                     float sigma_scale, const uint32_t* frags, float* dX, float* partial, uint32_t B, uint32_t out_c,
                     const int32_t* valid_rows, uint32_t valid_base, uint32_t valid_cap, uint32_t grid, hipStream_t s,
                     hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (ev_start) hipExtLaunchKernelGGL(k_nerf_mark, dim3(1), dim3(64), 0, s, nullptr, ev_start, 0);
    NerfBwdArgs a;
    a.X = X; a.dirs = dirs; a.g_rgb = g_rgb; a.rgb = rgb; a.g_sigma = g_sigma; a.sigma_scale = sigma_scale;
    a.dX = dX; a.partial = partial; a.B = B; a.out_c = out_c;
    a.rows = NerfRows{valid_rows, valid_base, valid_cap};
    if (g_nerf_bwd_transpose)
        hipExtLaunchKernelGGL(k_nerf_bwd, dim3(grid), dim3(256), 0, s, nullptr, ev_stop, 0, a, frags, make_sh_norm4());
    else
        hipExtLaunchKernelGGL(k_nerf_bwd_mfma, dim3(grid), dim3(256), 0, s, nullptr, ev_stop, 0, a, frags, make_sh_norm4());
}
#endif

}  // namespace enerf_mlp32

#ifdef NERF_MLP_BACKWARD_UNIT
// testing aid (include/enerf_hip.h): how k_nerf_bwd transposes its weight-gradient operands -- 0: on the matrix pipe,
// 1: through LDS (default); -1 queries; returns the previous value
extern "C" int enerf_debug_nerf_bwd_transpose(int mode) {
    const int prev = enerf_mlp32::g_nerf_bwd_transpose;
    if (mode >= 0) enerf_mlp32::g_nerf_bwd_transpose = mode != 0 ? 1 : 0;
    return prev;
}
#endif
