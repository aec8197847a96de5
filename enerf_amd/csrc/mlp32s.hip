// mlp32s.hip -- the fused fp32 MLP of mlp32.hip on the bf16 matrix pipe at fp32 accuracy (split operands).
// Its own translation unit because it is compiled with -amdgpu-mfma-vgpr-form: every MFMA result here is post-processed
// by VALU code at once (activation, hi / lo split, repacking of a flipped tile), and in the default AGPR form each of
// those elements costs a v_accvgpr_read first (a third of the tile loop's instructions).  The long-lived weight-gradient
// accumulators spill to AGPRs on their own where the arch VGPRs run out.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "mlp32_common.h"
#include "mlp32s_ops.h"

namespace enerf_mlp32 {

// ================================================================== split-bf16 kernels ("x3")
// The same networks on the bf16 matrix pipe, at fp32 accuracy: every fp32 operand v is carried as hi + lo with
// hi = bf16(v) and lo = bf16(v - hi) (both round-to-nearest: |v - hi - lo| <= 2^-17 |v|), and a product a * b as the
// three bf16 MFMA terms a.hi b.hi + a.hi b.lo + a.lo b.hi accumulated in fp32 (bf16 x bf16 is exact in fp32; the
// dropped a.lo b.lo is <= 2^-18 |a b|): ~2^-16 relative per product, against the 1e-4 the path has to hold, for 3/16 of
// the fp32 MFMA's pipe time (v_mfma_f32_32x32x16_bf16: 16 contraction steps per 32 cycles, v_mfma_f32_32x32x2_f32: 2
// per 64).  enerf_mlp32_precision(0) brings the bit-exact fp32 kernels above back.
//
// Layouts are those of the fp32 kernels with the contraction index grouped in eights: lane (j, h) of an A / B operand
// holds 8 consecutive contraction steps; K-step t of a D tile consumes accumulator registers 8t .. 8t+7, i.e. neurons
// nrow(8t + e, h) -- the weight fragments are gathered in that order, so one layer's D tile is still the next layer's
// B operand as it stands (split into hi / lo on the way).
//
// Weight gradients contract over SAMPLES, which a D tile keeps on the lanes.  Instead of passing every tile through LDS
// (the fp32 kernel above) the tile is flipped by the matrix pipe itself: used as the A operand (row = sample) against a
// 0/1 selection matrix, D[sample][neuron] comes back with the NEURON on the lanes and the samples in the registers
// (order nrow(q, h), the same for both operands of the weight-gradient product, which is all that matters) -- exact,
// since the operands are bf16 values times 1.0, and four MFMAs per 32 x 32 tile (hi and lo).  The backward therefore
// uses LDS only for the staged weights and its final per-workgroup sums, and no wavefront-level fences at all.
// The 16-bit operand type is a property of the translation unit: bf16 here (the split operands of the fp32 nets, and the
// FFMLP's bf16 nets); mlp32s_f16.hip compiles this file once more with ENERF_MLP32S_F16 for IEEE half operands (one
// product, fp32 accumulation: the arithmetic of the reference's `fp16 = True` regime, nerf/utils.py:964-975 -- only the
// P == 1 kernels are launched from there).  The names below keep their bf16 spelling.

// IO16 (the reference's FFMLP entry points, enerf_ffmlp_forward / _backward: row-major 16-bit tensors): a lane's 16 inputs
// ARE its two first-layer operands as they lie in memory -- two 16-byte loads, no conversion -- and outputs / input
// gradients leave as 16-bit values, four to an 8-byte store.
__device__ __forceinline__ void load_x16(const void* __restrict__ X, uint32_t tile, int j, int h, uint32_t B, bf16x8 (&f)[2]) {
    const size_t s = (size_t)tile * 32 + j;
    const bool valid = s < B;
    const size_t sc = valid ? s : (size_t)B - 1;
    const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const elem16*>(X) + sc * IN + 16 * h);
    uint4 a = p[0], b = p[1];
    if (!valid) a = b = make_uint4(0u, 0u, 0u, 0u);
    f[0] = __builtin_bit_cast(bf16x8, a);
    f[1] = __builtin_bit_cast(bf16x8, b);
}
__device__ __forceinline__ void store4_16(void* base, size_t elem, float a, float b, float c, float d) {
    typedef elem16 e4 __attribute__((ext_vector_type(4)));
    const e4 v = {(elem16)a, (elem16)b, (elem16)c, (elem16)d};
    *reinterpret_cast<e4*>(reinterpret_cast<elem16*>(base) + elem) = v;
}

// Weight operands of the forward: in registers for the density-only sweeps (SIG: ~100 tiles per wavefront) and for bf16
// operands; for split operands (P == 3) of a training / rendering batch they are kept in LDS in operand order instead
// (k_mlp32s_bwd's scheme) -- the 96 / 128 registers they would take hold the kernel at two wavefronts per SIMD, and a
// 4096-ray batch is ~4160 tiles: over 2048 resident wavefronts that is a third round for 64 of them, over 3072 it is two.
constexpr bool fwd_weights_in_lds(bool SIG, int P) { return P == 3 && !SIG; }
typedef unsigned u32x4w __attribute__((ext_vector_type(4)));

#ifdef ENERF_MLP32S_F16
#define k_mlp32s_fwd k_mlp32h_fwd
#define k_mlp32s_bwd k_mlp32h_bwd
#define k_mlp32s_mark k_mlp32h_mark
#endif
// D > 0 (SIG only): the load pipeline of the density-only head.  That head is a stream -- 128 B per sample in, 4 B out, ~100
// tiles per wavefront -- bound by bytes in flight over the memory latency, and D == 0, the form shipped before, has none in
// flight while it computes: load_x zeroes the rows past the batch, a use of the data, so the wavefront waits for its next
// tile where it asks for it.  With D > 0 a wavefront keeps the inputs of its next D tiles on request (request_x_lm: no use
// before they are due) in D register sets of 16 floats, which unrolled trips take in turn; no array is indexed at run
// time.  WPS: wavefronts per SIMD the registers must admit (the launcher's grid fills them); NT: non-temporal loads.
template <int NH, bool TRAIN, int XL, bool SIG = false, bool SH = false, int P = 3, bool IO16 = false, int D = 0, int WPS = 1,
          bool NT = false>
__global__ void __launch_bounds__(256, fwd_weights_in_lds(SIG, P) ? 3 : WPS) k_mlp32s_fwd(const float* __restrict__ X, WSrc W,
                                                    float* __restrict__ fb, float* __restrict__ Y, uint32_t B,
                                                    uint32_t out_dim, uint32_t act, uint32_t out_act, uint32_t y_stride,
                                                    float* __restrict__ y0_exp, const float* __restrict__ sh_dirs = nullptr,
                                                    ShNorm4 nrm = ShNorm4{}) {
    extern __shared__ __attribute__((aligned(16))) float wl[];
    const int lane = lane_id(), j = lane & 31, h = lane >> 5;
    const uint32_t Bp = (B + 31u) & ~31u;
    static_assert(!IO16 || (P == 1 && XL == 0 && !SIG && !SH && !TRAIN), "16-bit I/O: bf16 / fp16 operands, row-major, plain");
    static_assert(D >= 0 && ((SIG && XL == 1 && NH == 1) || (D == 0 && WPS == 1 && !NT)),
                  "the load pipeline is the density-only head's");
    constexpr bool PIPE = D > 0;
    float xq[PIPE ? D : 1][16];
    float (&x)[16] = xq[0];
    bf16x8 xraw[2];
    if constexpr (PIPE) {
        // all D requests go out here, before the weights are staged: the kernel's head stays one memory latency
        const uint32_t tile0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        const uint32_t nw0 = gridDim.x * (blockDim.x >> 6);
#pragma unroll
        for (int d = 0; d < D; d++)
            if (tile0 + (uint32_t)d * nw0 < Bp / 32) request_x_lm<NT>(X, tile0 + (uint32_t)d * nw0, j, h, Bp, xq[d]);
    } else {
        const uint32_t tile0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        if (tile0 < Bp / 32) {
            if constexpr (IO16) load_x16(X, tile0, j, h, B, xraw);
            else load_x<XL>(X, tile0, j, h, B, Bp, x);
        }
    }
    stage_rot(wl, W, NH, out_dim);

    typedef FragT<P> Frag;
    constexpr bool WL = fwd_weights_in_lds(SIG, P);
    Frag w0[2][2], wh[NH > 1 ? NH - 1 : 1][2][2][2], wo[2][2];
    float wsig[2][16];                                    // SIG: the output row as fp32 (VALU dot product)
#pragma unroll
    for (int ob = 0; ob < 2; ob++)
#pragma unroll
        for (int t = 0; t < 2; t++) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = wl[rot(32 * ob + j, kmap<XL>(8 * t + e, h), IN)];
            w0[ob][t] = split8<P>(v);
        }
#pragma unroll
    for (int l = 0; l < NH - 1; l++)
#pragma unroll
        for (int ob = 0; ob < 2; ob++)
#pragma unroll
            for (int ib = 0; ib < 2; ib++)
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        v[e] = wl[HID * IN + rot(l * HID + 32 * ob + j, 32 * ib + nrow(8 * t + e, h), HID)];
                    wh[l][ob][ib][t] = split8<P>(v);
                }
    {
        const float* w64 = wl + HID * IN;
        const uint32_t r0 = (NH - 1) * HID;
#pragma unroll
        for (int ib = 0; ib < 2; ib++) {
            if (SIG) {
#pragma unroll
                for (int q = 0; q < 16; q++) wsig[ib][q] = w64[rot(r0, 32 * ib + nrow(q, h), HID)];
            } else {
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        v[e] = (uint32_t)j < out_dim ? w64[rot(r0 + j, 32 * ib + nrow(8 * t + e, h), HID)] : 0.0f;
                    wo[ib][t] = split8<P>(v);
                }
            }
        }
    }

    // operand order in LDS (over the staged fp32 copy, which nobody reads any more): fragment f, hi then lo, 64 lanes x 16 B
    u32x4w* fr = reinterpret_cast<u32x4w*>(wl);
    auto fidx0 = [](int ob, int t) { return 2 * ob + t; };
    auto fidxh = [](int l, int ob, int ib, int t) { return 4 + ((l * 2 + ob) * 2 + ib) * 2 + t; };
    auto fidxo = [](int ib, int t) { return 4 + 8 * (NH - 1) + 2 * ib + t; };
    if (WL) {
        const int wid = threadIdx.x >> 6;
        auto put = [&](int f, const Frag& w) {
            if ((f & 3) == wid) {
                fr[(2 * f) * 64 + lane] = __builtin_bit_cast(u32x4w, w.hi);
                if constexpr (P == 3) fr[(2 * f + 1) * 64 + lane] = __builtin_bit_cast(u32x4w, w.lo);
            }
        };
        __syncthreads();                                   // every wave has read what it needs of the staged weights
#pragma unroll
        for (int ob = 0; ob < 2; ob++)
#pragma unroll
            for (int t = 0; t < 2; t++) put(fidx0(ob, t), w0[ob][t]);
#pragma unroll
        for (int l = 0; l < NH - 1; l++)
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int ib = 0; ib < 2; ib++)
#pragma unroll
                    for (int t = 0; t < 2; t++) put(fidxh(l, ob, ib, t), wh[l][ob][ib][t]);
#pragma unroll
        for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int t = 0; t < 2; t++) put(fidxo(ib, t), wo[ib][t]);
        __syncthreads();
    }
    auto get = [&](int f) -> Frag {
        Frag w;
        w.hi = __builtin_bit_cast(bf16x8, fr[(2 * f) * 64 + lane]);
        if constexpr (P == 3) w.lo = __builtin_bit_cast(bf16x8, fr[(2 * f + 1) * 64 + lane]);
        return w;
    };
    auto W0 = [&](int ob, int t) -> Frag { return WL ? get(fidx0(ob, t)) : w0[ob][t]; };
    auto WH = [&](int l, int ob, int ib, int t) -> Frag { return WL ? get(fidxh(l, ob, ib, t)) : wh[l][ob][ib][t]; };
    auto WO = [&](int ib, int t) -> Frag { return WL ? get(fidxo(ib, t)) : wo[ib][t]; };

    // ReLU as a signed-integer max on the bit pattern against a wave-uniform limit (0: negative floats, -0.0 and negative
    // NaNs are negative integers -> +0.0, everything else unchanged; INT_MIN: no activation): one v_max_i32 per element
    const int relu_lim = act == 0 ? 0 : (int)0x80000000;
    const uint32_t ntiles = valid_tiles(W, B, Bp / 32);
    const uint32_t gw = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t nw = gridDim.x * (blockDim.x >> 6);
    if constexpr (PIPE) {
        // One tile of the pipelined head, the arithmetic of the loop below instruction for instruction.  STEADY: a tile of
        // the full-speed trips -- all of its 32 rows are real and the tile D rounds ahead exists, so nothing in it is
        // conditional: every trip issues the same loads and stores, and the waits the compiler counts out leave exactly
        // the younger requests in flight (a request or a store that MAY have been issued makes it assume it was not, and
        // wait for everything).
        auto sig_tile = [&](uint32_t tile, float (&xs)[16], auto steady) __attribute__((always_inline)) {
            constexpr bool STEADY = decltype(steady)::value;
            const size_t s = (size_t)tile * 32 + j;
            const bool valid = STEADY || s < B;
            if (!STEADY) zero_rows_past(valid, xs);        // (what load_x does where it asks)
            Frag xf[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = xs[8 * t + e];
                xf[t] = split8<P>(v);
            }
            // the operands hold the tile; its registers receive the wave's tile D rounds ahead (past the last: no request)
            if (STEADY || tile + D * nw < ntiles) request_x_lm<NT>(X, tile + D * nw, j, h, Bp, xs);
            f32x16 a[2];
#pragma unroll
            for (int ob = 0; ob < 2; ob++) {
                a[ob] = (f32x16)(0.0f);
#pragma unroll
                for (int t = 0; t < 2; t++) a[ob] = mmap(w0[ob][t], xf[t], a[ob]);
#pragma unroll
                for (int q = 0; q < 16; q++) a[ob][q] = __int_as_float(max(__float_as_int(a[ob][q]), relu_lim));
            }
            float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
            for (int q = 0; q < 16; q++) {
                p0 = fmaf(wsig[0][q], a[0][q], p0);
                p1 = fmaf(wsig[1][q], a[1][q], p1);
            }
            float p = p0 + p1;
            p += __shfl_xor(p, 32, 64);
            // (STEADY: both halves hold p and store it -- the same value to the same address, one store, no branch)
            if (STEADY || (valid && h == 0)) y0_exp[s] = expf(p);
        };
        // A wavefront's k-th tile is served by register set k % D.  Full-speed trips: D tiles each, while every one of them
        // has its successor D rounds ahead; the rest (at most 2 D - 1 tiles) asks before it requests.
        uint32_t tile0 = gw;
        for (; tile0 + (2 * D - 1) * nw < ntiles; tile0 += D * nw)
#pragma unroll
            for (int d = 0; d < D; d++) sig_tile(tile0 + (uint32_t)d * nw, xq[d], std::true_type{});
        for (; tile0 < ntiles; tile0 += D * nw)
#pragma unroll
            for (int d = 0; d < D; d++) {
                if (d > 0 && tile0 + (uint32_t)d * nw >= ntiles) break;
                sig_tile(tile0 + (uint32_t)d * nw, xq[d], std::false_type{});
            }
        return;
    }
    for (uint32_t tile = gw; tile < ntiles; tile += nw) {
        const size_t s = (size_t)tile * 32 + j;
        const bool valid = s < B;
        if (WL) asm volatile("" ::: "memory");             // the operand reads stay inside the loop
        if (!SIG && tile != gw) {
            if constexpr (IO16) load_x16(X, tile, j, h, B, xraw);
            else load_x<XL>(X, tile, j, h, B, Bp, x);
        }
        float dir0 = 0.0f, dir1 = 0.0f, dir2 = 0.0f;
        if (SH && valid) {
            dir0 = sh_dirs[s * 3]; dir1 = sh_dirs[s * 3 + 1]; dir2 = sh_dirs[s * 3 + 2];
        }
        Frag xf[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if constexpr (IO16) {
                xf[t].hi = xraw[t];
            } else {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = x[8 * t + e];
                xf[t] = split8<P>(v);
            }
        }
        if (SIG && tile + nw < ntiles) load_x<XL>(X, tile + nw, j, h, B, Bp, x);
        f32x16 a[2];
        Frag af[2][2];
#pragma unroll
        for (int ob = 0; ob < 2; ob++) {
            a[ob] = (f32x16)(0.0f);
#pragma unroll
            for (int t = 0; t < 2; t++) a[ob] = mmap(W0(ob, t), xf[t], a[ob]);
#pragma unroll
            for (int q = 0; q < 16; q++) a[ob][q] = __int_as_float(max(__float_as_int(a[ob][q]), relu_lim));
            if (TRAIN) store_tile_fb(fb + s * HID, ob, h, a[ob]);
            if (!SIG || NH > 1) split_tile(a[ob], af[ob]);
        }
#pragma unroll
        for (int l = 1; l < NH; l++) {
            f32x16 n[2];
#pragma unroll
            for (int ob = 0; ob < 2; ob++) {
                n[ob] = (f32x16)(0.0f);
#pragma unroll
                for (int ib = 0; ib < 2; ib++)
#pragma unroll
                    for (int t = 0; t < 2; t++) n[ob] = mmap(WH(l - 1, ob, ib, t), af[ib][t], n[ob]);
#pragma unroll
                for (int q = 0; q < 16; q++) n[ob][q] = __int_as_float(max(__float_as_int(n[ob][q]), relu_lim));
                if (TRAIN) store_tile_fb(fb + ((size_t)l * Bp + s) * HID, ob, h, n[ob]);
            }
            a[0] = n[0];
            a[1] = n[1];
            if (!SIG || l < NH - 1) {
                split_tile(a[0], af[0]);
                split_tile(a[1], af[1]);
            }
        }
        if (SIG) {
            float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
            for (int q = 0; q < 16; q++) {
                p0 = fmaf(wsig[0][q], a[0][q], p0);
                p1 = fmaf(wsig[1][q], a[1][q], p1);
            }
            float p = p0 + p1;
            p += __shfl_xor(p, 32, 64);
            if (valid && h == 0) y0_exp[s] = expf(p);
            continue;
        }
        f32x16 o = (f32x16)(0.0f);
#pragma unroll
        for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int t = 0; t < 2; t++) o = mmap(WO(ib, t), af[ib][t], o);
        if (IO16 && !(out_act == 6 && (y_stride & 3u) == 0)) {
            // enerf_mlp32_io16 (the colour net of the stratified sampler's fp16 regime): any stride, any output activation,
            // one 16-bit store per value; the net's output is rounded first, then the activation of it (P == 1 below)
            if (valid) {
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    const uint32_t r = (uint32_t)nrow(q, h);
                    if (r < out_dim)
                        reinterpret_cast<elem16*>(Y)[s * y_stride + r] = (elem16)out_act_fwd(bf16r(o[q]), out_act);
                }
            }
        } else if (IO16) {
            // rows of out_dim <= 16 values: registers 0..3 -> columns 4h .. 4h+3, registers 4..7 -> columns 8 + 4h ..
            if (valid) {
#pragma unroll
                for (int g4 = 0; g4 < 2; g4++) {
                    const uint32_t c0 = (uint32_t)(8 * g4 + 4 * h);
                    if (c0 < out_dim)
                        store4_16(Y, s * y_stride + c0, out_act_fwd(o[4 * g4], out_act), out_act_fwd(o[4 * g4 + 1], out_act),
                                  out_act_fwd(o[4 * g4 + 2], out_act), out_act_fwd(o[4 * g4 + 3], out_act));
                }
            }
        } else if (valid) {
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const uint32_t r = (uint32_t)nrow(q, h);
                // P == 1: the net's outputs are 16-bit numbers, and so is whatever an elementwise op makes of them
                // (torch evaluates exp / sigmoid of a bf16 tensor in fp32 and rounds once)
                const float ov = P == 1 ? bf16r(o[q]) : o[q];
                if (Y && r < out_dim) {
                    const float yv = out_act_fwd(ov, out_act);
                    Y[s * y_stride + r] = (P == 1 && out_act != 6) ? bf16r(yv) : yv;
                }
                if (r == 0 && y0_exp) y0_exp[s] = (P == 1 && kRoundExp) ? bf16r(expf(ov)) : expf(ov);
            }
            if (SH) {
                float sh[16];
                sh4(dir0, dir1, dir2, nrm, sh);
                const uint32_t m = 0u - (uint32_t)h;
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; e++)
                    v[e] = __uint_as_float((__float_as_uint(sh[e]) & ~m) | (__float_as_uint(sh[8 + e]) & m));
                float* dst = Y + s * y_stride + 16 + 8 * h;
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
    }
}

// dgrad + wgrad of a net with one to three hidden layers and out_dim <= 16, one kernel, no LDS traffic for the tiles.
// Two hidden layers: the weight operands (14 fragments, 112 registers) would push the wavefront past its 512 registers,
// so they are kept in LDS in operand order (hi and lo: 64 lanes x 16 B each, one conflict-free ds_read_b128 per half) and
// read where they are used; one hidden layer keeps them in registers.
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
//
// RC (recompute): the hidden activations are not read back from the forward's buffer but computed again from X, by the
// forward's own instruction sequence (bit-identical values, hence identical ReLU masks): 12 (+ 24 per further hidden
// layer) MFMAs per tile on a pipe that is mostly idle here, against 256 B per sample and layer written by the forward
// and read by the backward -- at the 133 k-sample training batch that buffer was two thirds of the MLP kernels' HBM
// traffic.  X arrives once, in the forward's operand layout; its transpose for the first layer's weight gradient is a
// flip by the matrix pipe like every other tile's.  The forward-order weight operands join the others in LDS.
template <int NH, int XL, int P = 3, bool RC = false, bool IO16 = false>
__global__ void __launch_bounds__(256) k_mlp32s_bwd(DySource dys, const float* __restrict__ X, WSrc W,
                                                    const float* __restrict__ fb, float* __restrict__ dX,
                                                    float* __restrict__ partial, uint32_t B, uint32_t out_dim,
                                                    uint32_t act) {
    static_assert(!IO16 || (P == 1 && XL == 0 && RC), "16-bit I/O: bf16 / fp16 operands, row-major, recomputing");
    constexpr uint32_t NW_MAX = HID * IN + (NH - 1) * HID * HID + 16 * HID;
    constexpr bool WL = NH > 1 || RC;                                  // weight operands from LDS
    constexpr int NFRAG_T = 2 + 4 + 8 * (NH - 1);                      // transposed operands (dgrad)
    constexpr int NFRAG = NFRAG_T + (RC ? 4 + 8 * (NH - 1) : 0);       // + forward operands (recompute)
    constexpr int FRQ = P == 3 ? 2 : 1;                                // 64 x 16 B pieces per operand (hi, lo)
    // the final sums: four regions (one per wave) where they fit, two otherwise (three hidden layers: 4 x 44 KiB would
    // not), see the end of the kernel
    constexpr int NRED = NH > 2 ? 2 : 4;
    static_assert(NW_MAX * 4 + NFRAG * FRQ * 1024 <= NRED * NW_MAX * 4, "operand region must fit beside the staged weights");
    typedef FragT<P> Frag;
    __shared__ __attribute__((aligned(16))) float lds[NRED * NW_MAX];   // staged weights (+ operands), then the waves' dW sums
    float* wl = lds;
    const uint32_t NW = blob_size(NH, out_dim);
    const int lane = lane_id(), j = lane & 31, h = lane >> 5;
    const int wid = threadIdx.x >> 6;
    // RC: the forward-order operands (k_mlp32s_fwd's w0 / wh) come straight from the weights in global memory -- rows
    // across lanes is a 32-way bank conflict in the staged (un-rotated) copy -- each built by the wave that stores it
    // (fragment f by wave f % 4).  Their strided loads are requested here, BEFORE the staging, and travel beside it.
    constexpr int NRC_W = RC ? (4 + 8 * (NH - 1)) / 4 : 1;
    float rc_raw[NRC_W][8];
    if constexpr (RC) {
#pragma unroll
        for (int k = 0; k < NRC_W; k++) {
            const int idx = 4 * k + ((wid - NFRAG_T) & 3);                 // fragment NFRAG_T + idx is this wave's
            if (idx < 4) {
                const int ob = idx >> 1, t = idx & 1;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int c = w0_col((uint32_t)kmap<XL>(8 * t + e, h), W.nerf_perm);
                    rc_raw[k][e] = c < 0 ? 0.0f : W.seg[0][(size_t)(32 * ob + j) * W.w0_cols + (c < 0 ? 0 : c)];
                }
            } else {
                const int q = idx - 4, l = q >> 3, ob = (q >> 2) & 1, ib = (q >> 1) & 1, t = q & 1;
                const float* row = W.seg[1 + l] + (size_t)(32 * ob + j) * HID + 32 * ib;
#pragma unroll
                for (int e = 0; e < 8; e++) rc_raw[k][e] = row[nrow(8 * t + e, h)];
            }
        }
    }
    const uint32_t Bp = (B + 31u) & ~31u;
    const uint32_t ntiles = Bp / 32;
    const uint32_t nreal = valid_tiles(W, B, ntiles);
    const uint32_t gw = blockIdx.x * (blockDim.x >> 6) + wid;
    const uint32_t nw = gridDim.x * (blockDim.x >> 6);
    // (the first tile's requests go out here, before the weights are staged: they travel during the set-up)
    // as in the fp32 kernel: everything a tile reads from global memory is requested for the wave's NEXT tile where the
    // current tile has used it for the last time, branch-free, into the same registers
    float dy_raw[8], ys_raw[8], ds_raw = 0.0f, h0_raw = 0.0f;
    f32x16 fwl[NH][2];
    float xT[16];                                      // X^T: lane (input column j, h) holds samples nrow(q, h)
    auto request_out = [&](uint32_t t) {
        const size_t sn = (size_t)t * 32 + j;
        const size_t sc = sn < B ? sn : (size_t)B - 1;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const uint32_t o = (uint32_t)(8 * h + e), oc = o < out_dim ? o : out_dim - 1;
            if constexpr (IO16) dy_raw[e] = (float)reinterpret_cast<const elem16*>(dys.dY)[sc * dys.stride + oc];
            else dy_raw[e] = dys.dY[sc * dys.stride + oc];
            if constexpr (IO16)          // (enerf_mlp32_io16: the forward's 16-bit sigmoid output)
                ys_raw[e] = dys.y_sig ? (float)reinterpret_cast<const elem16*>(dys.y_sig)[sc * dys.y_sig_stride + oc] : 0.0f;
            else
                ys_raw[e] = dys.y_sig ? dys.y_sig[sc * dys.y_sig_stride + oc] : 0.0f;
        }
        if (dys.dsigma) {
            ds_raw = dys.dsigma[sc];
            h0_raw = dys.h0[sc * dys.h0_stride];
        }
        if constexpr (!RC) {
#pragma unroll
            for (int ib = 0; ib < 2; ib++) load_tile_fb(fb + ((size_t)(NH - 1) * Bp + sn) * HID, ib, h, fwl[NH - 1][ib]);
        }
    };
    auto request_hidden = [&](uint32_t t, int l) {
        if constexpr (RC) return;
        const size_t sn = (size_t)t * 32 + j;
#pragma unroll
        for (int ib = 0; ib < 2; ib++) load_tile_fb(fb + ((size_t)l * Bp + sn) * HID, ib, h, fwl[l][ib]);
    };
    float xfw[16];                                     // RC: X in the forward's operand layout (load_x), a tile ahead
    bf16x8 xraw[2];                                    // IO16: the same as the operands themselves
    auto request_x = [&](uint32_t t) {
        if constexpr (IO16) {
            load_x16(X, t, j, h, B, xraw);
            return;
        }
        if constexpr (RC) {
            load_x<XL>(X, t, j, h, B, Bp, xfw);
            return;
        }
        const size_t t0 = (size_t)t * 32;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const size_t row = t0 + nrow(q, h);
            if (XL == 0) {
                const size_t rc = row < B ? row : (size_t)B - 1;
                xT[q] = X[rc * IN + j];
            } else {
                xT[q] = X[((size_t)(j >> 1) * Bp + row) * 2 + (j & 1)];     // pad rows of a level-major X hold zeros
            }
        }
    };
    {
        const uint32_t t0 = gw < ntiles ? gw : ntiles - 1;
        request_out(t0);
#pragma unroll
        for (int l = NH - 2; l >= 0; l--) request_hidden(t0, l);
        request_x(t0);
    }
    stage(wl, W, NW);
    const float* wout = wl + HID * IN + (NH - 1) * HID * HID;
    u32x4v* fr = reinterpret_cast<u32x4v*>(lds + NW_MAX);
    auto put = [&](int f, const Frag& w) {                             // built by every wave, stored by wave f % 4
        if ((f & 3) == wid) {
            fr[(FRQ * f) * 64 + lane] = __builtin_bit_cast(u32x4v, w.hi);
            if constexpr (P == 3) fr[(FRQ * f + 1) * 64 + lane] = __builtin_bit_cast(u32x4v, w.lo);
        }
    };
    auto get = [&](int f) -> Frag {
        Frag w;
        w.hi = __builtin_bit_cast(bf16x8, fr[(FRQ * f) * 64 + lane]);
        if constexpr (P == 3) w.lo = __builtin_bit_cast(bf16x8, fr[(FRQ * f + 1) * 64 + lane]);
        return w;
    };

    Frag woT[2], whT[NH > 1 ? NH - 1 : 1][2][2][2], wiT[2][2];
#pragma unroll
    for (int ib = 0; ib < 2; ib++) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const uint32_t o = (uint32_t)(8 * h + e);
            v[e] = o < out_dim ? wout[o * HID + 32 * ib + j] : 0.0f;
        }
        woT[ib] = split8<P>(v);
        if (WL) put(ib, woT[ib]);
    }
#pragma unroll
    for (int ob = 0; ob < 2; ob++)
#pragma unroll
        for (int t = 0; t < 2; t++) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = wl[(32 * ob + nrow(8 * t + e, h)) * IN + j];
            wiT[ob][t] = split8<P>(v);
            if (WL) put(2 + 2 * ob + t, wiT[ob][t]);
        }
#pragma unroll
    for (int l = 0; l < NH - 1; l++)
#pragma unroll
        for (int ib = 0; ib < 2; ib++)
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        v[e] = wl[HID * IN + l * HID * HID + (32 * ob + nrow(8 * t + e, h)) * HID + 32 * ib + j];
                    whT[l][ib][ob][t] = split8<P>(v);
                    if (WL) put(6 + ((l * 2 + ib) * 2 + ob) * 2 + t, whT[l][ib][ob][t]);
                }
    if constexpr (RC) {
        // forward operands (k_mlp32s_fwd's w0 / wh): the values were requested before the staging (rc_raw above)
#pragma unroll
        for (int k = 0; k < NRC_W; k++) {
            const int f = NFRAG_T + 4 * k + ((wid - NFRAG_T) & 3);
            const Frag w = split8<P>(rc_raw[k]);
            fr[(FRQ * f) * 64 + lane] = __builtin_bit_cast(u32x4v, w.hi);
            if constexpr (P == 3) fr[(FRQ * f + 1) * 64 + lane] = __builtin_bit_cast(u32x4v, w.lo);
        }
    }
    if (WL) __syncthreads();
    auto W0F = [&](int ob, int t) -> Frag { return get(NFRAG_T + 2 * ob + t); };
    auto WHF = [&](int l, int ob, int ib, int t) -> Frag { return get(NFRAG_T + 4 + ((l * 2 + ob) * 2 + ib) * 2 + t); };
    auto WO = [&](int ib) -> Frag { return WL ? get(ib) : woT[ib]; };
    auto WI = [&](int ob, int t) -> Frag { return WL ? get(2 + 2 * ob + t) : wiT[ob][t]; };
    auto WH = [&](int l, int ib, int ob, int t) -> Frag {
        return WL ? get(6 + ((l * 2 + ib) * 2 + ob) * 2 + t) : whT[l][ib][ob][t];
    };
    const bf16x8 selN = selector(j, h, 0), selA = selector(j, h, 1), selB = selector(j, h, 2);

    f32x16 aw0[2], awh[NH > 1 ? NH - 1 : 1][2][2], awo[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
        aw0[a] = (f32x16)(0.0f);
        awo[a] = (f32x16)(0.0f);
#pragma unroll
        for (int l = 0; l < NH - 1; l++)
#pragma unroll
            for (int b = 0; b < 2; b++) awh[l][a][b] = (f32x16)(0.0f);
    }

    for (uint32_t tile = gw; tile < ntiles; tile += nw) {
        const uint32_t tnext = tile + nw < nreal ? tile + nw : tile;
        const size_t s0 = (size_t)tile * 32;
        const size_t s = s0 + j;
        const bool valid = s < B;
        if (WL) asm volatile("" ::: "memory");        // the operand reads stay in the loop (hoisted, they are 112 registers)
        if (tile >= nreal) {
            if (dX) {
                if (IO16) {
                    if (valid) {
#pragma unroll
                        for (int gq = 0; gq < 4; gq++) store4_16(dX, s * IN + 8 * gq + 4 * h, 0.f, 0.f, 0.f, 0.f);
                    }
                } else if (XL == 0) {
                    if (valid) {
#pragma unroll
                        for (int gq = 0; gq < 4; gq++)
                            *reinterpret_cast<float4*>(dX + s * IN + 8 * gq + 4 * h) = make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                } else {
#pragma unroll
                    for (int gq = 0; gq < 4; gq++) {
                        const size_t lv = (size_t)(4 * gq + 2 * h);
                        *reinterpret_cast<float2*>(dX + (lv * Bp + s) * 2) = make_float2(0.f, 0.f);
                        *reinterpret_cast<float2*>(dX + ((lv + 1) * Bp + s) * 2) = make_float2(0.f, 0.f);
                    }
                }
            }
            continue;
        }
        Frag xop[2];                                   // RC: X as the forward's first-layer operand
        if constexpr (RC) {
#pragma unroll
            for (int t = 0; t < 2; t++) {
                if constexpr (IO16) {
                    xop[t].hi = xraw[t];
                } else {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) v[e] = xfw[8 * t + e];
                    xop[t] = split8<P>(v);
                }
            }
            request_x(tnext);
            // the forward, instruction for instruction (k_mlp32s_fwd): same operands, same order of the products
            const int relu_lim = act == 0 ? 0 : (int)0x80000000;
#pragma unroll
            for (int ob = 0; ob < 2; ob++) {
                f32x16 a = (f32x16)(0.0f);
#pragma unroll
                for (int t = 0; t < 2; t++) a = mmap(W0F(ob, t), xop[t], a);
#pragma unroll
                for (int q = 0; q < 16; q++) a[q] = __int_as_float(max(__float_as_int(a[q]), relu_lim));
                fwl[0][ob] = a;
            }
#pragma unroll
            for (int l = 1; l < NH; l++) {
                Frag af[2][2];
                split_tile<P>(fwl[l - 1][0], af[0]);
                split_tile<P>(fwl[l - 1][1], af[1]);
#pragma unroll
                for (int ob = 0; ob < 2; ob++) {
                    f32x16 n = (f32x16)(0.0f);
#pragma unroll
                    for (int ib = 0; ib < 2; ib++)
#pragma unroll
                        for (int t = 0; t < 2; t++) n = mmap(WHF(l - 1, ob, ib, t), af[ib][t], n);
#pragma unroll
                    for (int q = 0; q < 16; q++) n[q] = __int_as_float(max(__float_as_int(n[q]), relu_lim));
                    fwl[l][ob] = n;
                }
            }
        }
        // ---- output layer
        Frag dyf;
        {
            float dy[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const uint32_t o = (uint32_t)(8 * h + e);
                float gq = dy_raw[e];
                if (dys.y_sig) gq = (gq * (1.0f - ys_raw[e])) * ys_raw[e];
                if (dys.dsigma && o == 0) gq = ds_raw * expf(fminf(fmaxf(h0_raw, -15.0f), 15.0f));
                dy[e] = (valid && o < out_dim) ? gq : 0.0f;
            }
            dyf = split8<P>(dy);
        }
        f32x16 g[2];
        Frag ft[2][2], gf[2][2], gT[2][2];             // [block][K-step]: flipped activations, gradients, flipped gradients
#pragma unroll
        for (int ib = 0; ib < 2; ib++) {
            g[ib] = mmap(WO(ib), dyf, (f32x16)(0.0f));
            if (act == 0) {                            // (wave-uniform: a scalar branch, not a select per element)
#pragma unroll
                for (int q = 0; q < 16; q++) g[ib][q] = fwl[NH - 1][ib][q] > 0.0f ? g[ib][q] : 0.0f;
            }
            Frag ff[2];
            split_tile<P>(fwl[NH - 1][ib], ff);
            flip_tile<P>(ff, selA, selB, ft[ib]);
        }
        request_out(tnext);
        {
            // dWout[o][i] += dY[o][s] * fb_last[i][s]
            Frag dyT[2];
            flip_natural<P>(dyf, selN, dyT);
#pragma unroll
            for (int nb = 0; nb < 2; nb++)
#pragma unroll
                for (int t = 0; t < 2; t++) awo[nb] = mmap(dyT[t], ft[nb][t], awo[nb]);
        }
#pragma unroll
        for (int ib = 0; ib < 2; ib++) {
            split_tile<P>(g[ib], gf[ib]);
            flip_tile<P>(gf[ib], selA, selB, gT[ib]);
        }
        // ---- hidden layers
#pragma unroll
        for (int jj = 1; jj < NH; jj++) {
            const int l = NH - jj;
            f32x16 n[2];
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                n[ib] = (f32x16)(0.0f);
#pragma unroll
                for (int ob = 0; ob < 2; ob++)
#pragma unroll
                    for (int t = 0; t < 2; t++) n[ib] = mmap(WH(l - 1, ib, ob, t), gf[ob][t], n[ib]);
            }
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                Frag ff[2];
                split_tile<P>(fwl[l - 1][ib], ff);
                flip_tile<P>(ff, selA, selB, ft[ib]);
            }
            // dWh[l-1][o][i] += G_l[o][s] * fb[l-1][i][s]
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int nb = 0; nb < 2; nb++)
#pragma unroll
                    for (int t = 0; t < 2; t++) awh[l - 1][ob][nb] = mmap(gT[ob][t], ft[nb][t], awh[l - 1][ob][nb]);
#pragma unroll
            for (int ib = 0; ib < 2; ib++)
#pragma unroll
                for (int q = 0; q < 16; q++) g[ib][q] = (act != 0 || fwl[l - 1][ib][q] > 0.0f) ? n[ib][q] : 0.0f;
            request_hidden(tnext, l - 1);
#pragma unroll
            for (int ib = 0; ib < 2; ib++) {
                split_tile<P>(g[ib], gf[ib]);
                flip_tile<P>(gf[ib], selA, selB, gT[ib]);
            }
        }
        // ---- input layer: dW0[o][i] += G_0[o][s] * X[s][i]
        {
            Frag xf[2];
            if constexpr (RC) {
                // X^T by the matrix pipe: K-step t of the operand holds input columns kmap(8t + e, h)
                bf16x8 sx[2];
#pragma unroll
                for (int t = 0; t < 2; t++)
#pragma unroll
                    for (int e = 0; e < 8; e++) sx[t][e] = kmap<XL>(8 * t + e, h) == j ? (elem16)1.0f : (elem16)0.0f;
                flip_tile<P>(xop, sx[0], sx[1], xf);
            } else {
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const int q = 8 * t + e;
                        v[e] = (XL == 0 && s0 + nrow(q, h) >= B) ? 0.0f : xT[q];
                    }
                    xf[t] = split8<P>(v);
                }
                request_x(tnext);
            }
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int t = 0; t < 2; t++) aw0[ob] = mmap(gT[ob][t], xf[t], aw0[ob]);
        }
        if (dX) {
            f32x16 d = (f32x16)(0.0f);
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int t = 0; t < 2; t++) d = mmap(WI(ob, t), gf[ob][t], d);
            if (IO16) {
                if (valid) {
#pragma unroll
                    for (int gq = 0; gq < 4; gq++)
                        store4_16(dX, s * IN + 8 * gq + 4 * h, d[4 * gq], d[4 * gq + 1], d[4 * gq + 2], d[4 * gq + 3]);
                }
            } else if (XL == 0) {
                if (valid) {
#pragma unroll
                    for (int gq = 0; gq < 4; gq++)
                        *reinterpret_cast<float4*>(dX + s * IN + 8 * gq + 4 * h) =
                            make_float4(d[4 * gq], d[4 * gq + 1], d[4 * gq + 2], d[4 * gq + 3]);
                }
            } else {
#pragma unroll
                for (int gq = 0; gq < 4; gq++) {
                    const size_t lv = (size_t)(4 * gq + 2 * h);
                    *reinterpret_cast<float2*>(dX + (lv * Bp + s) * 2) = make_float2(d[4 * gq], d[4 * gq + 1]);
                    *reinterpret_cast<float2*>(dX + ((lv + 1) * Bp + s) * 2) = make_float2(d[4 * gq + 2], d[4 * gq + 3]);
                }
            }
        }
    }

    // per-workgroup sums, as in the fp32 kernel: the waves write their accumulators into regions of their own and the
    // sums are taken in a fixed order on the way out (deterministic).  NRED == 4: one region per wave, ((w0 + w1) + w2) +
    // w3.  NRED == 2: waves 0 / 1 write, waves 2 / 3 add into the same regions, (w0 + w2) + (w1 + w3).
    __syncthreads();
    float* red = lds + (size_t)(wid % NRED) * NW;
    auto flush = [&](const f32x16& a, uint32_t base, int ld, int ob, int nb, uint32_t nrows, bool add) {
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const uint32_t o = (uint32_t)(32 * ob + nrow(q, h));
            if (o < nrows) {
                float* p = red + base + o * ld + 32 * nb + j;
                *p = add ? *p + a[q] : a[q];
            }
        }
    };
    auto flush_all = [&](bool add) {
#pragma unroll
        for (int ob = 0; ob < 2; ob++) flush(aw0[ob], 0, IN, ob, 0, HID, add);
#pragma unroll
        for (int l = 0; l < NH - 1; l++)
#pragma unroll
            for (int ob = 0; ob < 2; ob++)
#pragma unroll
                for (int nb = 0; nb < 2; nb++) flush(awh[l][ob][nb], HID * IN + l * HID * HID, HID, ob, nb, HID, add);
#pragma unroll
        for (int nb = 0; nb < 2; nb++) flush(awo[nb], HID * IN + (NH - 1) * HID * HID, HID, 0, nb, out_dim, add);
    };
    float* dst = partial + (size_t)blockIdx.x * NW;
    if (NRED == 4) {
        flush_all(false);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < NW; i += blockDim.x)
            dst[i] = ((lds[i] + lds[NW + i]) + lds[2 * NW + i]) + lds[3 * NW + i];
    } else {
        if (wid < 2) flush_all(false);
        __syncthreads();
        if (wid >= 2) flush_all(true);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < NW; i += blockDim.x) dst[i] = lds[i] + lds[NW + i];
    }
}

__global__ void k_mlp32s_mark() {}

void MLP32S_LAUNCH_FWD(int prec, uint32_t num_hidden, bool train, uint32_t x_layout, int sig_form, const float* X,
                       const WSrc& W, float* fb, float* Y, uint32_t B, uint32_t out_dim, uint32_t act, uint32_t out_act,
                       uint32_t y_stride, float* y0_exp, const float* sh_dirs, uint32_t grid, size_t lds, hipStream_t s,
                       hipEvent_t ev_start, hipEvent_t ev_stop, bool io16) {
    // timed launches (enerf_prof_*): the interval runs between two kernel-attached stop events -- a one-wavefront marker
    // right before the kernel, and the kernel itself -- i.e. the kernel's own dispatch-to-end, as for grid_encode_forward
    if (ev_start) hipExtLaunchKernelGGL(k_mlp32s_mark, dim3(1), dim3(64), 0, s, nullptr, ev_start, 0);
#define S_FWD(NHV, TR, XLV, SIGV, SHV, PV)                                                                                  \
    hipExtLaunchKernelGGL((k_mlp32s_fwd<NHV, TR, XLV, SIGV, SHV, PV>), dim3(grid), dim3(256), lds, s, nullptr, ev_stop, 0, X, W, \
                          fb, Y, B, out_dim, act, out_act, y_stride, y0_exp, sh_dirs, nrm)
#ifdef ENERF_MLP32S_F16
#define S_FWD_P(NHV, TR, XLV, SIGV, SHV) S_FWD(NHV, TR, XLV, SIGV, SHV, 1)
#else
#define S_FWD_P(NHV, TR, XLV, SIGV, SHV)                 \
    do {                                                 \
        if (prec == 3) S_FWD(NHV, TR, XLV, SIGV, SHV, 3); \
        else S_FWD(NHV, TR, XLV, SIGV, SHV, 1);          \
    } while (0)
#endif
#define S_FWD_IO(NHV)                                                                                                       \
    hipExtLaunchKernelGGL((k_mlp32s_fwd<NHV, false, 0, false, false, 1, true>), dim3(grid), dim3(256), lds, s, nullptr, ev_stop, \
                          0, X, W, fb, Y, B, out_dim, act, out_act, y_stride, y0_exp, sh_dirs, nrm)
#define S_FWD_XL(NHV, TR)                                   \
    do {                                                    \
        if (x_layout == 0) S_FWD_P(NHV, TR, 0, false, false); \
        else S_FWD_P(NHV, TR, 1, false, false);             \
    } while (0)
#define S_FWD_TR(NHV)                   \
    do {                                \
        if (train) S_FWD_XL(NHV, true); \
        else S_FWD_XL(NHV, false);      \
    } while (0)
    const ShNorm4 nrm = sh_dirs ? make_sh_norm4() : ShNorm4{};
    if (io16) {                          // the FFMLP entry points: 16-bit row-major X / Y, two or three hidden layers
        if (num_hidden == 2) S_FWD_IO(2);
        else S_FWD_IO(3);
    } else if (sh_dirs) {                // level-major input, the SH encoding into columns 16..31 of the output rows
        if (num_hidden == 1) {
            if (train) S_FWD_P(1, true, 1, false, true);
            else S_FWD_P(1, false, 1, false, true);
        } else {
            if (train) S_FWD_P(2, true, 1, false, true);
            else S_FWD_P(2, false, 1, false, true);
        }
    } else if (sig_form != kSigOff) {    // the density-only head (mlp32_common.h: its forms)
#define S_SIG(PV, DV, WV, NTV)                                                                                              \
    hipExtLaunchKernelGGL((k_mlp32s_fwd<1, false, 1, true, false, PV, false, DV, WV, NTV>), dim3(grid), dim3(256), lds, s,   \
                          nullptr, ev_stop, 0, X, W, fb, Y, B, out_dim, act, out_act, y_stride, y0_exp, sh_dirs, nrm)
#ifdef ENERF_MLP32S_F16
#define S_SIG_P(DV, WV, NTV) S_SIG(1, DV, WV, NTV)
#else
#define S_SIG_P(DV, WV, NTV)                    \
    do {                                        \
        if (prec == 3) S_SIG(3, DV, WV, NTV);   \
        else S_SIG(1, DV, WV, NTV);             \
    } while (0)
#endif
        if (sig_form == kSigOneAhead) S_SIG_P(0, 1, false);
#if defined(ENERF_SIG_HEAD_LAB) && !defined(ENERF_MLP32S_F16)
        // development aid (tools/sigma_head_lab.py): depth x residency, form 1000 + 100 * NT + 10 * WPS + D, split operands
#define S_SIG_LAB_D(WV, NTV)                                                \
    do {                                                                    \
        const int dv = sig_form % 10;                                       \
        if (dv == 1) S_SIG(3, 1, WV, NTV);                                  \
        else if (dv == 2) S_SIG(3, 2, WV, NTV);                             \
        else if (dv == 3) S_SIG(3, 3, WV, NTV);                             \
        else S_SIG(3, 4, WV, NTV);                                          \
    } while (0)
        else if (sig_form >= 1000 && prec == 3) {
            const bool two = sig_form / 10 % 10 == 2;
            if (sig_form / 100 % 10) {
                if (two) S_SIG_LAB_D(2, true);
                else S_SIG_LAB_D(1, true);
            } else {
                if (two) S_SIG_LAB_D(2, false);
                else S_SIG_LAB_D(1, false);
            }
        }
#undef S_SIG_LAB_D
#endif
        else S_SIG_P(kSigDepth, kSigWaves, kSigNT);
#undef S_SIG_P
#undef S_SIG
    } else if (num_hidden == 1) {
        S_FWD_TR(1);
    } else if (num_hidden == 2) {
        S_FWD_TR(2);
    } else {
        S_FWD_TR(3);
    }
#undef S_FWD_TR
#undef S_FWD_IO
#undef S_FWD_XL
#undef S_FWD_P
#undef S_FWD
}

void MLP32S_LAUNCH_BWD(int prec, uint32_t num_hidden, uint32_t x_layout, const DySource& dys, const float* X,
                       const WSrc& W, const float* fb, float* dX, float* partial, uint32_t B, uint32_t out_dim,
                       uint32_t act, uint32_t grid, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop,
                       bool recompute, bool io16) {
    if (ev_start) hipExtLaunchKernelGGL(k_mlp32s_mark, dim3(1), dim3(64), 0, s, nullptr, ev_start, 0);
    if (io16) {                          // the FFMLP entry points: 16-bit row-major X / dY / dX, recomputing
        if (num_hidden == 2)
            hipExtLaunchKernelGGL((k_mlp32s_bwd<2, 0, 1, true, true>), dim3(grid), dim3(256), 0, s, nullptr, ev_stop, 0, dys, X,
                                  W, fb, dX, partial, B, out_dim, act);
        else
            hipExtLaunchKernelGGL((k_mlp32s_bwd<3, 0, 1, true, true>), dim3(grid), dim3(256), 0, s, nullptr, ev_stop, 0, dys, X,
                                  W, fb, dX, partial, B, out_dim, act);
        return;
    }
#define S_BWD(NHV, XLV, PV, RCV)                                                                                         \
    hipExtLaunchKernelGGL((k_mlp32s_bwd<NHV, XLV, PV, RCV>), dim3(grid), dim3(256), 0, s, nullptr, ev_stop, 0, dys, X, W, fb, \
                          dX, partial, B, out_dim, act)
#define S_BWD_R(NHV, XLV, PV)                     \
    do {                                          \
        if (recompute) S_BWD(NHV, XLV, PV, true); \
        else S_BWD(NHV, XLV, PV, false);          \
    } while (0)
#ifdef ENERF_MLP32S_F16
#define S_BWD_P(NHV, XLV) S_BWD_R(NHV, XLV, 1)
#else
#define S_BWD_P(NHV, XLV)                    \
    do {                                     \
        if (prec == 3) S_BWD_R(NHV, XLV, 3); \
        else S_BWD_R(NHV, XLV, 1);           \
    } while (0)
#endif
    if (num_hidden == 1) {
        if (x_layout == 0) S_BWD_P(1, 0);
        else S_BWD_P(1, 1);
    } else if (num_hidden == 2) {
        if (x_layout == 0) S_BWD_P(2, 0);
        else S_BWD_P(2, 1);
    } else {                                 // three hidden layers: the FFMLP colour net (row-major input), P == 1 only
        // (always recomputing: the activation-loading instance <3, 0, 1, false> crashes this compiler's 'AMDGPU Rewrite
        //  AGPR-Copy-MFMA' pass once mmab carries ENERF_MFMA_GUARD; mlp32.hip's recompute_for() says the same to the forward)
        S_BWD(3, 0, 1, true);
    }
#undef S_BWD_P
#undef S_BWD_R
#undef S_BWD
}

}  // namespace enerf_mlp32
