// stratified.hip -- the stratified sampler of NeRFRenderer.run (reference nerf/renderer.py:150-278 with upsample_steps = 0)
// for gfx950: sample generation, the compositing rule of `run`, the colour mask compacted on the device, and the gradient
// of the compositing.  The networks in between are the library's own kernels (grid encoder, enerf_mlp32_*); the Python
// side (enerf_amd/stratified.py) strings them together as one autograd node.
//
//   k_strat_points      near / far (the slab test of enerf_near_far_from_aabb), T depths and the clamped points; the
//                       same operations in the same order as sampler.stratified_depths + sampler._points, so z and xyz
//                       are bit-equal with them
//   k_strat_weights     alpha, the exclusive product of (1 - alpha + 1e-15), w, opacity, normalised depth, the number of
//                       samples with w > 1e-4 per ray
//   k_strat_color_input the colour net's input rows of the masked samples, in sample order at the ray's offset in the
//                       compact list (offsets: inclusive scan of the per-ray counts; the total stays on the device)
//   k_strat_composite   image = sum_masked w * rgb + (1 - opacity) * bg
//   k_strat_composite_bwd  d(sigma) of every sample (reverse scan, no division by 1 - alpha + 1e-15) and d(rgb) of
//                       the compact rows
//   k_strat_scatter_geo the colour net's input gradient (geo_feat columns) back to the sigma net's output rows
//
// Colour rows, rgb, d rgb and the colour net's input gradient exist in two storages (template parameter E): fp32, and
// fp16 for the fp16 regime (enerf_mlp32_precision 3 with the mlp32 16-bit I/O: DESIGN.md section 4.9).  In fp16 the
// directions are rounded to half before the SH basis (the reference's SHEncoder casts its inputs to half under autocast)
// and the basis is evaluated in fp32 on those half inputs and stored as half -- shencoder.hip's __half path, value for
// value.  Weights, opacity, depth and the compositing stay fp32 in both.
//
// One wavefront per ray in every kernel.  The scans cover 64 lanes x 8 consecutive samples = 512 samples per pass; longer
// rays take several passes with the running product / sum carried from pass to pass.
//
// Compiled with -ffp-contract=off, and no fmaf appears below: every product and sum is rounded where torch rounds it
// (the one fused operation of torch's linspace kernel is evaluated exactly in double and rounded once).
#include <float.h>
#include <hip/hip_fp16.h>
#include <math.h>

#include "common.h"
#include "sh_basis.h"

using namespace enerf;

namespace {

#include "march_lattice.h"

constexpr int kPer = 8;                       // samples per lane and pass
constexpr int kPass = kWave * kPer;           // samples per wave and pass
constexpr int kRaysPerBlock = 4;              // 256 threads

// torch.maximum / torch.minimum: NaN in the first operand propagates (the box bounds are never NaN)
__device__ __forceinline__ float tmax(float a, float b) { return (a != a) ? a : (a < b ? b : a); }
__device__ __forceinline__ float tmin(float a, float b) { return (a != a) ? a : (b < a ? b : a); }
// Tensor.clamp(0, 1), NaN kept
__device__ __forceinline__ float clamp01(float x) { return (x != x) ? x : (x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x)); }

// the two storages of the colour rows / rgb / d rgb / dx: element loads and stores (fp16: round to nearest even)
__device__ __forceinline__ float ld_e(const float* p) { return *p; }
__device__ __forceinline__ float ld_e(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ void st_e(float* p, float v) { *p = v; }
// (the empty asm keeps v an fp32 value: without it the compiler folds a product and this conversion into one
//  v_fma_mixlo_f16, a single rounding of the exact product, which differs from torch's fp32-then-fp16 at fp16 ties)
__device__ __forceinline__ void st_e(__half* p, float v) {
    asm volatile("" : "+v"(v));
    *p = __float2half(v);
}
__device__ __forceinline__ uint32_t pack2h(float a, float b) {
    return (uint32_t)__half_as_ushort(__float2half(a)) | ((uint32_t)__half_as_ushort(__float2half(b)) << 16);
}
__device__ __forceinline__ uint4 pack8h(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
    return make_uint4(pack2h(a0, a1), pack2h(a2, a3), pack2h(a4, a5), pack2h(a6, a7));
}
__device__ __forceinline__ float lo_h(uint32_t v) { return __half2float(__ushort_as_half((unsigned short)(v & 0xFFFFu))); }
__device__ __forceinline__ float hi_h(uint32_t v) { return __half2float(__ushort_as_half((unsigned short)(v >> 16))); }
__device__ __forceinline__ float round_h(float v) { return __half2float(__float2half(v)); }

__device__ __forceinline__ float wave_sum(float v) { return wave_bcast(wave_incl_scan_add(v, 0), kWave - 1); }

// sampler.ray_weights for one sample: alpha, (1 - alpha + 1e-15) and exp(-step * s * sigma)
struct Alpha {
    float a, c, e, step;
};
__device__ __forceinline__ Alpha alpha_of(const float* __restrict__ zr, const float* __restrict__ sr, uint32_t k,
                                          uint32_t T, float width, float density_scale) {
    Alpha r;
    const float zk = zr[k];
    r.step = k + 1 < T ? zr[k + 1] - zk : width * 1.0f;
    r.e = expf(-r.step * density_scale * sr[k]);
    r.a = 1.0f - r.e;
    r.c = 1.0f - r.a + 1e-15f;
    return r;
}

// ------------------------------------------------------------------ samples
__global__ void __launch_bounds__(256) k_strat_points(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                      const float* __restrict__ aabb, uint32_t N, uint32_t T,
                                                      float min_near, float lin_step, float inv_T,
                                                      const float* __restrict__ u, float* __restrict__ nears,
                                                      float* __restrict__ fars, float* __restrict__ z,
                                                      float* __restrict__ xyz) {
    const uint32_t n = blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (n >= N) return;
    const float ox = rays_o[n * 3], oy = rays_o[n * 3 + 1], oz = rays_o[n * 3 + 2];
    const float dx = rays_d[n * 3], dy = rays_d[n * 3 + 1], dz = rays_d[n * 3 + 2];
    float near, far;
    (void)near_far_of(ox, oy, oz, dx, dy, dz, aabb, min_near, near, far);
    if (lane == 0) {
        nears[n] = near;
        fars[n] = far;
    }
    const float span = far - near;               // fars - nears
    const float width = span * inv_T;            // span / n: torch multiplies by the host-rounded reciprocal
    const float lo0 = aabb[0], lo1 = aabb[1], lo2 = aabb[2], hi0 = aabb[3], hi1 = aabb[4], hi2 = aabb[5];
    const uint32_t half = T / 2;
    for (uint32_t k = lane; k < T; k += kWave) {
        // torch.linspace(0, 1, T) on the device: start + step * i below the midpoint, end - step * (T - 1 - i) above.
        // torch's kernel is built with contraction on, so the upper half is one fused multiply-add: rounded once here
        // too, from the exact value in double (step * (T - 1 - i) and 1 minus it are exact in 53 bits)
        float g;
        if (T == 1) g = 0.0f;
        else if (k < half) g = 0.0f + lin_step * (float)k;
        else g = (float)(1.0 - (double)lin_step * (double)(T - 1 - k));
        float zk = near + span * g;
        const size_t s = (size_t)n * T + k;
        if (u) zk = zk + (u[s] - 0.5f) * width;
        z[s] = zk;
        xyz[s * 3 + 0] = tmin(tmax(ox + dx * zk, lo0), hi0);
        xyz[s * 3 + 1] = tmin(tmax(oy + dy * zk, lo1), hi1);
        xyz[s * 3 + 2] = tmin(tmax(oz + dz * zk, lo2), hi2);
    }
}

// ------------------------------------------------------------------ weights, opacity, depth, mask counts
__global__ void __launch_bounds__(256) k_strat_weights(const float* __restrict__ z, const float* __restrict__ sigma,
                                                       const float* __restrict__ nears, const float* __restrict__ fars,
                                                       uint32_t N, uint32_t T, float inv_T, float density_scale,
                                                       float* __restrict__ w, float* __restrict__ opacity,
                                                       float* __restrict__ depth, int32_t* __restrict__ count) {
    const uint32_t n = blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (n >= N) return;                          // (whole waves: one ray per wave)
    const float near = nears[n], far = fars[n];
    const float span = far - near, width = span * inv_T;
    const float* zr = z + (size_t)n * T;
    const float* sr = sigma + (size_t)n * T;
    float* wr = w + (size_t)n * T;
    float carry = 1.0f, osum = 0.0f, dsum = 0.0f;
    uint32_t cnt = 0;
    for (uint32_t base = 0; base < T; base += kPass) {
        const uint32_t k0 = base + lane * kPer;
        float a[kPer], c[kPer];
        float lp = 1.0f;
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const uint32_t k = k0 + i;
            if (k < T) {
                const Alpha al = alpha_of(zr, sr, k, T, width, density_scale);
                a[i] = al.a;
                c[i] = al.c;
            } else {
                a[i] = 0.0f;
                c[i] = 1.0f;
            }
            lp *= c[i];
        }
        const float incl = wave_incl_scan_mul(lp, 0);
        float tk = carry * wave_prev(incl, 1.0f);
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const uint32_t k = k0 + i;
            if (k < T) {
                const float wk = a[i] * tk;
                wr[k] = wk;
                osum += wk;
                dsum += wk * clamp01((zr[k] - near) / (far - near));
                cnt += wk > 1e-4f ? 1u : 0u;
            }
            tk *= c[i];
        }
        carry *= wave_bcast(incl, kWave - 1);
    }
    osum = wave_sum(osum);
    dsum = wave_sum(dsum);
    cnt = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_add_u32(cnt, 0), kWave - 1);
    if (lane == 0) {
        opacity[n] = osum;
        depth[n] = dsum;
        count[n] = (int32_t)cnt;
    }
}

// Masked samples of this lane in this pass (bit i: sample k0 + i) and their first compact row.  `off` = the ray's first
// row before the pass; advanced past the pass on return.
__device__ __forceinline__ uint32_t pass_mask(const float* __restrict__ wr, uint32_t k0, uint32_t T, uint32_t& row,
                                              uint32_t& off) {
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < kPer; i++)
        if (k0 + i < T && wr[k0 + i] > 1e-4f) bits |= 1u << i;
    const uint32_t mine = (uint32_t)__popc(bits);
    const uint32_t incl = wave_incl_scan_add_u32(mine, 0);
    row = off + incl - mine;
    off += (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
    return bits;
}

// first compact row of ray n: inclusive offset minus the ray's own count
__device__ __forceinline__ uint32_t ray_offset(const int32_t* __restrict__ incl, const int32_t* __restrict__ count,
                                               uint32_t n) {
    return (uint32_t)(incl[n] - count[n]);
}

// ------------------------------------------------------------------ colour net input of the compact rows
// Row layout is the one enerf_mlp32_*_p read with nerf_perm = 1 (w0_cols 31): [0 | geo_feat 15 | SH4(d) 16] -- the kernels
// permute color_net[0].weight ([SH 16 | geo_feat 15] in memory) to match while staging it.  Rows total .. pad32(total) - 1
// (the last partial tile the MLP kernels process) are zero-filled.  E = __half: 64 B rows, the SH basis of the
// half-rounded direction; geo_feat is the sigma net's fp16-rounded output (precision 3), so its conversion is exact.
template <typename E>
__global__ void __launch_bounds__(256) k_strat_color_input(const float* __restrict__ w, const int32_t* __restrict__ incl,
                                                           const int32_t* __restrict__ count, const float* __restrict__ h16,
                                                           const float* __restrict__ rays_d, uint32_t N, uint32_t T,
                                                           uint32_t cap, ShNorm4 nrm, E* __restrict__ cin) {
    constexpr bool kHalf = sizeof(E) == 2;
    constexpr int kVec = kHalf ? 4 : 8;           // 16-byte pieces per row
    const uint32_t n = blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (n >= N) return;
    if (n == 0) {
        const uint32_t total = (uint32_t)incl[N - 1];
        const uint32_t end = min((total + 31u) & ~31u, cap);
        for (uint32_t r = total + lane; r < end; r += kWave)
#pragma unroll
            for (int q = 0; q < kVec; q++) reinterpret_cast<uint4*>(cin + (size_t)r * 32)[q] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (count[n] == 0) return;
    float sh[16];
    float d0 = rays_d[n * 3], d1 = rays_d[n * 3 + 1], d2 = rays_d[n * 3 + 2];
    if (kHalf) {
        d0 = round_h(d0);
        d1 = round_h(d1);
        d2 = round_h(d2);
    }
    sh4(d0, d1, d2, nrm, sh);
    uint4 shh[2];
    if (kHalf) {
        shh[0] = pack8h(sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], sh[6], sh[7]);
        shh[1] = pack8h(sh[8], sh[9], sh[10], sh[11], sh[12], sh[13], sh[14], sh[15]);
    }
    const float* wr = w + (size_t)n * T;
    uint32_t off = ray_offset(incl, count, n);
    for (uint32_t base = 0; base < T; base += kPass) {
        const uint32_t k0 = base + lane * kPer;
        uint32_t row;
        const uint32_t bits = pass_mask(wr, k0, T, row, off);
        for (int i = 0; i < kPer; i++) {
            if (!(bits & (1u << i))) continue;
            const size_t s = (size_t)n * T + k0 + i;
            const float4* src = reinterpret_cast<const float4*>(h16 + s * 16);
            float4 q0 = src[0];
            q0.x = 0.0f;                          // raw density: zero weight in the colour net, kept finite
            if constexpr (kHalf) {
                const float4 q1 = src[1], q2 = src[2], q3 = src[3];
                uint4* dst = reinterpret_cast<uint4*>(cin + (size_t)row * 32);
                dst[0] = pack8h(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w);
                dst[1] = pack8h(q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w);
                dst[2] = shh[0];
                dst[3] = shh[1];
            } else {
                float4* dst = reinterpret_cast<float4*>(cin + (size_t)row * 32);
                dst[0] = q0;
                dst[1] = src[1];
                dst[2] = src[2];
                dst[3] = src[3];
                dst[4] = make_float4(sh[0], sh[1], sh[2], sh[3]);
                dst[5] = make_float4(sh[4], sh[5], sh[6], sh[7]);
                dst[6] = make_float4(sh[8], sh[9], sh[10], sh[11]);
                dst[7] = make_float4(sh[12], sh[13], sh[14], sh[15]);
            }
            row++;
        }
    }
}

// ------------------------------------------------------------------ compositing: forward
// bg: [C] (bg_per_ray 0) or [N, C] (bg_per_ray 1); rgb in storage E, accumulated in fp32
template <int C, typename E>
__global__ void __launch_bounds__(256) k_strat_composite(const float* __restrict__ w, const int32_t* __restrict__ incl,
                                                         const int32_t* __restrict__ count,
                                                         const float* __restrict__ opacity, const E* __restrict__ rgb,
                                                         const float* __restrict__ bg, uint32_t bg_per_ray, uint32_t N,
                                                         uint32_t T, float* __restrict__ image) {
    const uint32_t n = blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (n >= N) return;
    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ch++) acc[ch] = 0.0f;
    if (count[n] != 0) {
        const float* wr = w + (size_t)n * T;
        uint32_t off = ray_offset(incl, count, n);
        for (uint32_t base = 0; base < T; base += kPass) {
            const uint32_t k0 = base + lane * kPer;
            uint32_t row;
            const uint32_t bits = pass_mask(wr, k0, T, row, off);
            for (int i = 0; i < kPer; i++) {
                if (!(bits & (1u << i))) continue;
                const float wk = wr[k0 + i];
#pragma unroll
                for (int ch = 0; ch < C; ch++) acc[ch] += wk * ld_e(rgb + (size_t)row * C + ch);
                row++;
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ch++) acc[ch] = wave_sum(acc[ch]);
    }
    if (lane < C) {
        float v = acc[0];
#pragma unroll
        for (int ch = 1; ch < C; ch++)
            if ((int)lane == ch) v = acc[ch];
        const float b = bg[(bg_per_ray ? (size_t)n * C : 0) + lane];
        image[(size_t)n * C + lane] = v + (1.0f - opacity[n]) * b;
    }
}

// ------------------------------------------------------------------ compositing: backward
// With q_k = dL/dw_k = sum_c g_c (rgb_kc - bg_c) + g_depth t_k (rgb_k = 0 off the mask) and T_k the exclusive product,
//   dL/dalpha_k = T_k (q_k - R_{k+1}),   R_k = q_k alpha_k + (1 - alpha_k + 1e-15) R_{k+1},   R_T = 0,
// a reverse linear recurrence, evaluated as a scan of affine maps (lane chunks, then across the wave, then pass to pass).
// Nothing is divided by (1 - alpha + 1e-15).  dL/dsigma_k = dL/dalpha_k * step_k * s * exp(-step_k * s * sigma_k).
// g_sigma doubles as the store of T_k between the two sweeps when the ray takes more than one pass.
// rgb and g_rgb in storage E (fp16: d rgb = g * w rounded to half, the gradient of the reference's `h.to(fp32)`).
template <int C, typename E>
__global__ void __launch_bounds__(256) k_strat_composite_bwd(
    const float* __restrict__ g_image, const float* __restrict__ g_depth, const float* __restrict__ z,
    const float* __restrict__ sigma, const float* __restrict__ w, const float* __restrict__ nears,
    const float* __restrict__ fars, const int32_t* __restrict__ incl, const int32_t* __restrict__ count,
    const E* __restrict__ rgb, const float* __restrict__ bg, uint32_t bg_per_ray, uint32_t N, uint32_t T,
    float inv_T, float density_scale, uint32_t cap, float* __restrict__ g_sigma, E* __restrict__ g_rgb) {
    const uint32_t n = blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (n >= N) return;
    if (n == 0) {                                 // the compact list's last partial tile: zero upstream gradient
        const uint32_t total = (uint32_t)incl[N - 1];
        const uint32_t end = min((total + 31u) & ~31u, cap);
        for (uint32_t r = total + lane; r < end; r += kWave)
#pragma unroll
            for (int ch = 0; ch < C; ch++) st_e(g_rgb + (size_t)r * C + ch, 0.0f);
    }
    const float near = nears[n], far = fars[n];
    const float span = far - near, width = span * inv_T;
    const float* zr = z + (size_t)n * T;
    const float* sr = sigma + (size_t)n * T;
    const float* wr = w + (size_t)n * T;
    float* gr = g_sigma + (size_t)n * T;
    float gi[C], gbg = 0.0f;
#pragma unroll
    for (int ch = 0; ch < C; ch++) {
        gi[ch] = g_image[(size_t)n * C + ch];
        gbg += gi[ch] * bg[(bg_per_ray ? (size_t)n * C : 0) + ch];
    }
    const float gd = g_depth ? g_depth[n] : 0.0f;
    const uint32_t npass = (T + kPass - 1) / kPass;

    // sweep 1: T_k (kept in registers for a one-pass ray, stored in g_sigma otherwise)
    float tk[kPer];
    float carry = 1.0f;
    for (uint32_t p = 0; p < npass; p++) {
        const uint32_t k0 = p * kPass + lane * kPer;
        float c[kPer];
        float lp = 1.0f;
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            c[i] = k0 + i < T ? alpha_of(zr, sr, k0 + i, T, width, density_scale).c : 1.0f;
            lp *= c[i];
        }
        const float inc = wave_incl_scan_mul(lp, 0);
        float t = carry * wave_prev(inc, 1.0f);
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            tk[i] = t;
            if (npass > 1 && k0 + i < T) gr[k0 + i] = t;
            t *= c[i];
        }
        carry *= wave_bcast(inc, kWave - 1);
    }

    // sweep 2, passes in reverse order.  A pass's first compact row is the ray's offset plus the masked samples of the
    // passes before it (recounted from w: nothing per pass is kept, whatever T is).
    const uint32_t off0 = ray_offset(incl, count, n);
    float rcarry = 0.0f;                          // R at the first sample of the pass after this one
    for (int p = (int)npass - 1; p >= 0; p--) {
        const uint32_t base = (uint32_t)p * kPass;
        const uint32_t k0 = base + lane * kPer;
        // rows before this pass: masked samples of the ray below `base`
        uint32_t before = 0;
        for (uint32_t b = 0; b < base; b += kPass) {
            uint32_t r, o = 0;
            (void)pass_mask(wr, b + lane * kPer, T, r, o);
            before += o;
        }
        uint32_t off = off0 + before, row;
        const uint32_t bits = pass_mask(wr, k0, T, row, off);
        float a[kPer], c[kPer], e[kPer], st[kPer], q[kPer];
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const uint32_t k = k0 + i;
            if (k < T) {
                const Alpha al = alpha_of(zr, sr, k, T, width, density_scale);
                a[i] = al.a;
                c[i] = al.c;
                e[i] = al.e;
                st[i] = al.step;
                // (no depth gradient: no depth term at all -- a ray that misses the box has t = NaN)
                float qk = g_depth ? gd * clamp01((zr[k] - near) / (far - near)) : 0.0f;
                qk -= gbg;
                if (bits & (1u << i)) {
                    const float wk = wr[k];
#pragma unroll
                    for (int ch = 0; ch < C; ch++) {
                        qk += gi[ch] * ld_e(rgb + (size_t)row * C + ch);
                        st_e(g_rgb + (size_t)row * C + ch, gi[ch] * wk);
                    }
                    row++;
                }
                q[i] = qk;
                if (npass > 1) tk[i] = gr[k];
            } else {
                a[i] = 0.0f;
                c[i] = 1.0f;
                e[i] = 1.0f;
                st[i] = 0.0f;
                q[i] = 0.0f;
            }
        }
        // this lane's chunk as the map R_in -> A R_in + B (R_in: R just after the chunk)
        float A = 1.0f, B = 0.0f;
#pragma unroll
        for (int i = kPer - 1; i >= 0; i--) {
            B = q[i] * a[i] + c[i] * B;
            A = c[i] * A;
        }
        // inclusive suffix composition over the lanes above: lane l -> chunks l .. 63
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const float A2 = __shfl_down(A, d, kWave), B2 = __shfl_down(B, d, kWave);
            if (lane + d < kWave) {
                B = B + A * B2;
                A = A * A2;
            }
        }
        const float Ax = __shfl_down(A, 1, kWave), Bx = __shfl_down(B, 1, kWave);
        float R = lane + 1 < kWave ? Bx + Ax * rcarry : rcarry;      // R_{k0 + kPer}
#pragma unroll
        for (int i = kPer - 1; i >= 0; i--) {
            const uint32_t k = k0 + i;
            if (k < T) gr[k] = tk[i] * (q[i] - R) * st[i] * density_scale * e[i];
            R = q[i] * a[i] + c[i] * R;
        }
        rcarry = wave_bcast(B, 0) + wave_bcast(A, 0) * rcarry;
    }
}

// ------------------------------------------------------------------ geo_feat gradient back to the sigma net's rows
// dh16 [N*T, 16]: columns 1..15 = the colour net's input gradient of the compact row (columns 1..15 of dx, nerf_perm
// layout), zero off the mask; column 0 is left for the sigma net's backward, which replaces it (dsigma * exp(h0)).
// dx in storage E (fp16: the colour net's 16-bit dX, widened exactly).
template <typename E>
__global__ void __launch_bounds__(256) k_strat_scatter_geo(const float* __restrict__ w, const int32_t* __restrict__ incl,
                                                           const int32_t* __restrict__ count, const E* __restrict__ dx,
                                                           uint32_t N, uint32_t T, float* __restrict__ dh16) {
    const uint32_t n = blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (n >= N) return;
    const float* wr = w + (size_t)n * T;
    uint32_t off = ray_offset(incl, count, n);
    for (uint32_t base = 0; base < T; base += kPass) {
        const uint32_t k0 = base + lane * kPer;
        uint32_t row;
        const uint32_t bits = pass_mask(wr, k0, T, row, off);
        for (int i = 0; i < kPer; i++) {
            if (k0 + i >= T) break;
            float4* dst = reinterpret_cast<float4*>(dh16 + ((size_t)n * T + k0 + i) * 16);
            if (bits & (1u << i)) {
                if constexpr (sizeof(E) == 2) {
                    const uint4* src = reinterpret_cast<const uint4*>(dx + (size_t)row * 32);
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const uint4 v = src[q];
                        dst[2 * q] = make_float4(lo_h(v.x), hi_h(v.x), lo_h(v.y), hi_h(v.y));
                        dst[2 * q + 1] = make_float4(lo_h(v.z), hi_h(v.z), lo_h(v.w), hi_h(v.w));
                    }
                } else {
                    const float4* src = reinterpret_cast<const float4*>(dx + (size_t)row * 32);
#pragma unroll
                    for (int q = 0; q < 4; q++) dst[q] = src[q];
                }
                row++;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) dst[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
}

uint32_t ray_blocks(uint32_t N) { return div_up(N, kRaysPerBlock); }

}  // namespace

extern "C" {

int enerf_stratified_points(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, uint32_t T,
                            float min_near, float lin_step, float inv_T, const float* u, float* nears, float* fars,
                            float* z, float* xyz, enerf_stream_t stream) {
    if (T == 0) ENERF_BADARG("stratified_points: T must be > 0");
    if (!rays_o || !rays_d || !aabb || !nears || !fars || !z || !xyz) ENERF_BADARG("stratified_points: null pointer");
    if ((uint64_t)N * T > 0xFFFFFFFFull / 3) ENERF_BADARG("stratified_points: N * T too large");
    if (N == 0) return 0;
    k_strat_points<<<ray_blocks(N), 256, 0, (hipStream_t)stream>>>(rays_o, rays_d, aabb, N, T, min_near, lin_step, inv_T,
                                                                    u, nears, fars, z, xyz);
    ENERF_LAUNCH_CHECK("stratified_points");
    return 0;
}

int enerf_stratified_weights(const float* z, const float* sigma, const float* nears, const float* fars, uint32_t N,
                             uint32_t T, float inv_T, float density_scale, float* w, float* opacity, float* depth,
                             int32_t* count, enerf_stream_t stream) {
    if (T == 0) ENERF_BADARG("stratified_weights: T must be > 0");
    if (!z || !sigma || !nears || !fars || !w || !opacity || !depth || !count) ENERF_BADARG("stratified_weights: null pointer");
    if (N == 0) return 0;
    k_strat_weights<<<ray_blocks(N), 256, 0, (hipStream_t)stream>>>(z, sigma, nears, fars, N, T, inv_T, density_scale, w,
                                                                     opacity, depth, count);
    ENERF_LAUNCH_CHECK("stratified_weights");
    return 0;
}

int enerf_stratified_color_input_ex(const float* w, const int32_t* incl, const int32_t* count, const float* h16,
                                    const float* rays_d, uint32_t N, uint32_t T, uint32_t cap, void* cin, uint32_t storage,
                                    enerf_stream_t stream) {
    if (!w || !incl || !count || !h16 || !rays_d || !cin) ENERF_BADARG("stratified_color_input: null pointer");
    if ((uint64_t)cap < (uint64_t)N * T) ENERF_BADARG("stratified_color_input: cap %u < N * T", cap);
    if (storage != ENERF_F32 && storage != ENERF_F16) ENERF_BADARG("stratified_color_input: storage must be F32 or F16");
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (storage == ENERF_F16)
        k_strat_color_input<__half><<<ray_blocks(N), 256, 0, s>>>(w, incl, count, h16, rays_d, N, T, cap, make_sh_norm4(),
                                                                   (__half*)cin);
    else
        k_strat_color_input<float><<<ray_blocks(N), 256, 0, s>>>(w, incl, count, h16, rays_d, N, T, cap, make_sh_norm4(),
                                                                  (float*)cin);
    ENERF_LAUNCH_CHECK("stratified_color_input");
    return 0;
}

int enerf_stratified_color_input(const float* w, const int32_t* incl, const int32_t* count, const float* h16,
                                 const float* rays_d, uint32_t N, uint32_t T, uint32_t cap, float* cin,
                                 enerf_stream_t stream) {
    return enerf_stratified_color_input_ex(w, incl, count, h16, rays_d, N, T, cap, cin, ENERF_F32, stream);
}

int enerf_stratified_composite_forward_ex(const float* w, const int32_t* incl, const int32_t* count,
                                          const float* opacity, const void* rgb, const float* bg, uint32_t bg_per_ray,
                                          uint32_t N, uint32_t T, uint32_t C, float* image, uint32_t storage,
                                          enerf_stream_t stream) {
    if (!w || !incl || !count || !opacity || !rgb || !bg || !image) ENERF_BADARG("stratified_composite_forward: null pointer");
    if (storage != ENERF_F32 && storage != ENERF_F16) ENERF_BADARG("stratified_composite_forward: storage must be F32 or F16");
    if (C < 1 || C > 3) ENERF_BADARG("stratified_composite_forward: C must be 1..3, got %u", C);
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
#define STRAT_FWD(CC, EE) \
    k_strat_composite<CC, EE><<<ray_blocks(N), 256, 0, s>>>(w, incl, count, opacity, (const EE*)rgb, bg, bg_per_ray, N, T, image)
#define STRAT_FWD_E(CC)                              \
    do {                                             \
        if (storage == ENERF_F16) STRAT_FWD(CC, __half); \
        else STRAT_FWD(CC, float);                   \
    } while (0)
    switch (C) {
        case 1: STRAT_FWD_E(1); break;
        case 2: STRAT_FWD_E(2); break;
        default: STRAT_FWD_E(3); break;
    }
#undef STRAT_FWD_E
#undef STRAT_FWD
    ENERF_LAUNCH_CHECK("stratified_composite_forward");
    return 0;
}

int enerf_stratified_composite_forward(const float* w, const int32_t* incl, const int32_t* count, const float* opacity,
                                       const float* rgb, const float* bg, uint32_t bg_per_ray, uint32_t N, uint32_t T,
                                       uint32_t C, float* image, enerf_stream_t stream) {
    return enerf_stratified_composite_forward_ex(w, incl, count, opacity, rgb, bg, bg_per_ray, N, T, C, image, ENERF_F32,
                                                 stream);
}

int enerf_stratified_composite_backward_ex(const float* g_image, const float* g_depth, const float* z, const float* sigma,
                                           const float* w, const float* nears, const float* fars, const int32_t* incl,
                                           const int32_t* count, const void* rgb, const float* bg, uint32_t bg_per_ray,
                                           uint32_t N, uint32_t T, uint32_t C, float inv_T, float density_scale,
                                           uint32_t cap, float* g_sigma, void* g_rgb, uint32_t storage,
                                           enerf_stream_t stream) {
    if (!g_image || !z || !sigma || !w || !nears || !fars || !incl || !count || !rgb || !bg || !g_sigma || !g_rgb)
        ENERF_BADARG("stratified_composite_backward: null pointer");
    if ((uint64_t)cap < (uint64_t)N * T) ENERF_BADARG("stratified_composite_backward: cap %u < N * T", cap);
    if (storage != ENERF_F32 && storage != ENERF_F16) ENERF_BADARG("stratified_composite_backward: storage must be F32 or F16");
    if (C < 1 || C > 3) ENERF_BADARG("stratified_composite_backward: C must be 1..3, got %u", C);
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
#define STRAT_BWD(CC, EE)                                                                                                 \
    k_strat_composite_bwd<CC, EE><<<ray_blocks(N), 256, 0, s>>>(g_image, g_depth, z, sigma, w, nears, fars, incl, count,  \
                                                                (const EE*)rgb, bg, bg_per_ray, N, T, inv_T, density_scale, \
                                                                cap, g_sigma, (EE*)g_rgb)
#define STRAT_BWD_E(CC)                              \
    do {                                             \
        if (storage == ENERF_F16) STRAT_BWD(CC, __half); \
        else STRAT_BWD(CC, float);                   \
    } while (0)
    switch (C) {
        case 1: STRAT_BWD_E(1); break;
        case 2: STRAT_BWD_E(2); break;
        default: STRAT_BWD_E(3); break;
    }
#undef STRAT_BWD_E
#undef STRAT_BWD
    ENERF_LAUNCH_CHECK("stratified_composite_backward");
    return 0;
}

int enerf_stratified_composite_backward(const float* g_image, const float* g_depth, const float* z, const float* sigma,
                                        const float* w, const float* nears, const float* fars, const int32_t* incl,
                                        const int32_t* count, const float* rgb, const float* bg, uint32_t bg_per_ray,
                                        uint32_t N, uint32_t T, uint32_t C, float inv_T, float density_scale,
                                        uint32_t cap, float* g_sigma, float* g_rgb, enerf_stream_t stream) {
    return enerf_stratified_composite_backward_ex(g_image, g_depth, z, sigma, w, nears, fars, incl, count, rgb, bg,
                                                  bg_per_ray, N, T, C, inv_T, density_scale, cap, g_sigma, g_rgb,
                                                  ENERF_F32, stream);
}

int enerf_stratified_scatter_geo_grad_ex(const float* w, const int32_t* incl, const int32_t* count, const void* dx,
                                         uint32_t N, uint32_t T, float* dh16, uint32_t storage, enerf_stream_t stream) {
    if (!w || !incl || !count || !dx || !dh16) ENERF_BADARG("stratified_scatter_geo_grad: null pointer");
    if (storage != ENERF_F32 && storage != ENERF_F16) ENERF_BADARG("stratified_scatter_geo_grad: storage must be F32 or F16");
    if (N == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (storage == ENERF_F16)
        k_strat_scatter_geo<__half><<<ray_blocks(N), 256, 0, s>>>(w, incl, count, (const __half*)dx, N, T, dh16);
    else
        k_strat_scatter_geo<float><<<ray_blocks(N), 256, 0, s>>>(w, incl, count, (const float*)dx, N, T, dh16);
    ENERF_LAUNCH_CHECK("stratified_scatter_geo_grad");
    return 0;
}

int enerf_stratified_scatter_geo_grad(const float* w, const int32_t* incl, const int32_t* count, const float* dx,
                                      uint32_t N, uint32_t T, float* dh16, enerf_stream_t stream) {
    return enerf_stratified_scatter_geo_grad_ex(w, incl, count, dx, N, T, dh16, ENERF_F32, stream);
}

}  // extern "C"
