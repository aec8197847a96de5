// event_pairs.hip -- one launch per training step for what EventNeRFDataset.collate does per event pair on the host
// (nerf/provider.py:1364-1441):
//   accumulate_evs branch (:1367-1398): drawn event -> step back if it is the last at its pixel -> window end among
//     its next min(num_successor, acc_max_num_evs + 1) events -> polarity sum over the window (prefix sums);
//   accumulate_evs off (:1400-1405, what every shipped config trains with): per chosen pixel the drawn event that has a
//     successor and that successor, the successor's polarity (k_event_single_pair_rays);
//   --negative_event_sampling (:1443-1476): pixels of a chunk where nothing happened, two ordered times (k_no_event_rays);
//   "computing poses online" (:1411-1420) and get_event_rays (nerf/utils.py:184-216) for all three: pose_track.h.
// One thread per pair; everything a pair needs is 2 table rows + 2 track segments.
#include "common.h"
#include "pose_track.h"

using namespace enerf;

namespace {

__global__ void __launch_bounds__(256) k_event_pair_rays(
    const float* __restrict__ events, const uint8_t* __restrict__ no_successor, const int64_t* __restrict__ num_successor,
    const double* __restrict__ pol_cumsum, uint32_t N, const int64_t* __restrict__ start_draw,
    const double* __restrict__ u_end, uint32_t M, uint32_t acc_max_num_evs, const double* __restrict__ knots,
    const double* __restrict__ rot, const double* __restrict__ rotvec, const double* __restrict__ tcoef, uint32_t K,
    Intr in, float* __restrict__ o1, float* __restrict__ d1, float* __restrict__ o2, float* __restrict__ d2,
    float* __restrict__ pols, int64_t* __restrict__ start_out, int64_t* __restrict__ end_out, int* __restrict__ outside) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= M) return;
    int64_t s = start_draw[k];
    s -= (int64_t)no_successor[s];                                   // last event of its pixel: take the one before
    int64_t ns = num_successor[s];
    if (acc_max_num_evs && ns > (int64_t)acc_max_num_evs + 1) ns = (int64_t)acc_max_num_evs + 1;
    int64_t step = (int64_t)floor(u_end[k] * (double)ns);            // randint(s + 1, s + 1 + ns) from a uniform in [0,1)
    if (step > ns - 1) step = ns - 1;
    const int64_t e = s + 1 + step;
    start_out[k] = s;
    end_out[k] = e;
    pols[k] = (float)(pol_cumsum[e + 1] - pol_cumsum[s + 1]);
    const float x = events[(size_t)s * 4], y = events[(size_t)s * 4 + 1];
    float dx, dy, dz;
    cam_dir(in, x, y, dx, dy, dz);
    float m[3][4];
    const bool ok1 = pose_at(knots, rot, rotvec, tcoef, K, (double)events[(size_t)s * 4 + 2], m);
    ray_of(m, dx, dy, dz, o1 + (size_t)k * 3, d1 + (size_t)k * 3);
    const bool ok2 = pose_at(knots, rot, rotvec, tcoef, K, (double)events[(size_t)e * 4 + 2], m);
    ray_of(m, dx, dy, dz, o2 + (size_t)k * 3, d2 + (size_t)k * 3);
    if (!(ok1 && ok2)) atomicAdd(outside, 1);                        // interp1d(bounds_error=True) would raise
}

// a pair (or pixel) whose index is not one: nothing is read for it, its rays are zero
__device__ __forceinline__ void zero_rays(uint32_t k, float* __restrict__ o1, float* __restrict__ d1,
                                          float* __restrict__ o2, float* __restrict__ d2) {
    const size_t r = (size_t)k * 3;
    for (int a = 0; a < 3; a++) o1[r + a] = d1[r + a] = o2[r + a] = d2[r + a] = 0.0f;
}

// the rays of pixel (x, y) through the camera at t1 and at t2 (track units); false when a time lies outside the track
__device__ __forceinline__ bool ray_pair(const double* __restrict__ knots, const double* __restrict__ rot,
                                         const double* __restrict__ rotvec, const double* __restrict__ tcoef, uint32_t K,
                                         const Intr& in, float x, float y, double t1, double t2, uint32_t k,
                                         float* __restrict__ o1, float* __restrict__ d1, float* __restrict__ o2,
                                         float* __restrict__ d2) {
    float dx, dy, dz;
    cam_dir(in, x, y, dx, dy, dz);
    bool ok = true;
    const double ts[2] = {t1, t2};
    float* const os[2] = {o1, o2};
    float* const ds[2] = {d1, d2};
    for (int j = 0; j < 2; j++) {
        float m[3][4] = {};                                          // (outside the track: a zero pose, counted)
        ok = pose_at(knots, rot, rotvec, tcoef, K, ts[j], m) && ok;
        ray_of(m, dx, dy, dz, os[j] + (size_t)k * 3, ds[j] + (size_t)k * 3);
    }
    return ok;
}

// accumulate_evs off (provider.py:1400-1405): per pixel the drawn event that has a successor,
// (np.random.rand(P) * num - 1).astype(int) + first; pair k is that event of pixel choice[k] and its direct successor.
__global__ void __launch_bounds__(256) k_event_single_pair_rays(
    const float* __restrict__ events, uint32_t N, const int64_t* __restrict__ num_at_xy,
    const int64_t* __restrict__ first_at_xy, uint32_t P, const double* __restrict__ u_xy,
    const int64_t* __restrict__ choice, uint32_t M, const double* __restrict__ knots, const double* __restrict__ rot,
    const double* __restrict__ rotvec, const double* __restrict__ tcoef, uint32_t K, Intr in, float* __restrict__ o1,
    float* __restrict__ d1, float* __restrict__ o2, float* __restrict__ d2, float* __restrict__ pols,
    int64_t* __restrict__ start_out, int64_t* __restrict__ end_out, int* __restrict__ outside, int* __restrict__ bad) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= M) return;
    const int64_t c = choice[k];
    int64_t s = -1;
    if (c >= 0 && c < (int64_t)P) {
        const double v = u_xy[c] * (double)num_at_xy[c] - 1.0;      // product and difference each rounded (no contraction)
        // the cast truncates toward zero: (-1, 0) -> 0.  (u_xy == 0 exactly gives -1 as in the reference: the event
        // before the pixel's first; for pixel 0 that is no event and is counted below.  NaN / huge: not cast.)
        if (v >= -1.0 && v < 4294967296.0) s = (int64_t)v + first_at_xy[c];
    }
    if (s < 0 || s > (int64_t)N - 2) {                               // not a pixel (or tables that are none): no read
        zero_rays(k, o1, d1, o2, d2);
        pols[k] = 0.0f;
        start_out[k] = end_out[k] = 0;
        atomicAdd(bad, 1);
        return;
    }
    const int64_t e = s + 1;
    start_out[k] = s;
    end_out[k] = e;
    pols[k] = events[(size_t)e * 4 + 3];
    const float x = events[(size_t)s * 4], y = events[(size_t)s * 4 + 1];
    if (!ray_pair(knots, rot, rotvec, tcoef, K, in, x, y, (double)events[(size_t)s * 4 + 2],
                  (double)events[(size_t)e * 4 + 2], k, o1, d1, o2, d2))
        atomicAdd(outside, 1);
}

// --negative_event_sampling (provider.py:1443-1476): pixel idx[k] of one chunk's event-free pixels, two uniform times of
// the chunk in ascending order (microseconds; the track is in nanoseconds), rays through the camera at both.
__global__ void __launch_bounds__(256) k_no_event_rays(
    const float* __restrict__ coords, uint32_t n_coords, const int64_t* __restrict__ idx, const double* __restrict__ u,
    uint32_t n, double t0, double t1, const double* __restrict__ knots, const double* __restrict__ rot,
    const double* __restrict__ rotvec, const double* __restrict__ tcoef, uint32_t K, Intr in, float* __restrict__ o1,
    float* __restrict__ d1, float* __restrict__ o2, float* __restrict__ d2, double* __restrict__ tss,
    int* __restrict__ outside, int* __restrict__ bad) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t i = idx[k];
    if (i < 0 || i >= (int64_t)n_coords) {
        zero_rays(k, o1, d1, o2, d2);
        tss[(size_t)k * 2] = tss[(size_t)k * 2 + 1] = 0.0;
        atomicAdd(bad, 1);
        return;
    }
    const double span = t1 - t0;
    const double ta = t0 + span * u[(size_t)k * 2], tb = t0 + span * u[(size_t)k * 2 + 1];
    const double lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;     // np.sort(..., axis=1)
    tss[(size_t)k * 2] = lo;
    tss[(size_t)k * 2 + 1] = hi;
    if (!ray_pair(knots, rot, rotvec, tcoef, K, in, coords[(size_t)i * 2], coords[(size_t)i * 2 + 1], lo * 1000.0,
                  hi * 1000.0, k, o1, d1, o2, d2))
        atomicAdd(outside, 1);
}


// ---- event loss, forward and gradient in one launch (nerf/utils.py:499-516 with C_thres != -1) ------------------------
// Per ray: (luma of) the two renders -> lin-log / log intensities -> delta = p2 - p1 -> (delta - pol * C)^2, mean over
// rays x channels.  Writes delta, d loss / d image1, d loss / d image2 and the loss (one workgroup, fixed summation
// order).  CH = channels of the images (1..3); luma is a three-channel operation.  The arithmetic follows events.py (= utils/event_utils.py:23-66) operation by operation.
struct EventLossCfg {
    uint32_t use_luma, linlog;
    float c_thres, log_thres, upstream;
};
__device__ __forceinline__ float ev_luma(const float* rgb) {
    // torch.sum(rgb * factors, axis=-1): ((r*w0 + g*w1) + b*w2)
    return (rgb[0] * 0.299f + rgb[1] * 0.587f) + rgb[2] * 0.114f;
}
// intensity p(l) and dp/dl for l in image units (the reference scales by 255 first)
__device__ __forceinline__ void ev_intensity(float l, const EventLossCfg& c, float& p, float& dp) {
    const float x = l * 255.0f;
    if (c.linlog) {
        const float slope = (float)(2.995732273553991 / 20.0);          // np.log(20) / 20, rounded to fp32 by torch
        if (x < 20.0f) { p = slope * x; dp = slope * 255.0f; }
        else { p = logf(x); dp = (1.0f / x) * 255.0f; }
    } else {
        if (x > c.log_thres) { p = logf(x); dp = (1.0f / x) * 255.0f; }
        else { p = logf(c.log_thres); dp = 0.0f; }
    }
}
template <int CH>
__global__ void __launch_bounds__(1024) k_event_loss(const float* __restrict__ img1, const float* __restrict__ img2,
                                                     const float* __restrict__ pols, uint32_t N, EventLossCfg c,
                                                     float* __restrict__ g1, float* __restrict__ g2,
                                                     float* __restrict__ delta, float* __restrict__ loss) {
    __shared__ double red[1024];
    const uint32_t ch = (CH == 3 && c.use_luma) ? 1u : (uint32_t)CH;
    const float inv_count = 1.0f / (float)(N * ch);
    double acc = 0.0;
    for (uint32_t r = threadIdx.x; r < N; r += 1024u) {
        const float* a = img1 + (size_t)r * CH;
        const float* b = img2 + (size_t)r * CH;
        const float target = pols[r] * c.c_thres;
        float ga[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f};
        if (CH == 3 && c.use_luma) {
            float p1, d1, p2, d2;
            ev_intensity(ev_luma(a), c, p1, d1);
            // without lin-log the reference evaluates the second term on the FIRST luma (nerf/utils.py:500): delta = 0
            ev_intensity(c.linlog ? ev_luma(b) : ev_luma(a), c, p2, d2);
            const float dl = p2 - p1, res = dl - target;
            delta[r] = dl;
            acc += (double)(res * res);
            const float gd = c.upstream * (2.0f * res * inv_count);
            const float w[3] = {0.299f, 0.587f, 0.114f};
            for (int k = 0; k < 3; k++) {
                if (c.linlog) { ga[k] = -gd * d1 * w[k]; gb[k] = gd * d2 * w[k]; }
                else ga[k] = (gd * d2 - gd * d1) * w[k];
            }
        } else {
            for (int k = 0; k < CH; k++) {
                float p1, d1, p2, d2;
                ev_intensity(a[k], c, p1, d1);
                ev_intensity(b[k], c, p2, d2);
                const float dl = p2 - p1, res = dl - target;
                delta[(size_t)r * CH + k] = dl;
                acc += (double)(res * res);
                const float gd = c.upstream * (2.0f * res * inv_count);
                ga[k] = -gd * d1;
                gb[k] = gd * d2;
            }
        }
        for (int k = 0; k < CH; k++) {
            g1[(size_t)r * CH + k] = ga[k];
            g2[(size_t)r * CH + k] = gb[k];
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t o = 512; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && loss) loss[0] = (float)(red[0] * (double)inv_count) * c.upstream;
}

// ---- sums of a 1024-thread workgroup for the two kernels below: across the 64 lanes of a wave in registers, then the 16
// waves' partials through LDS; every thread leaves with the totals, added in wave order (the same order on every run).
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                                        // (lane 0 holds the wave's sum)
}
template <int NS>
__device__ __forceinline__ void block_sums_1024(double (&v)[NS], double (*part)[NS]) {   // part: LDS, [16][NS]
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (int s = 0; s < NS; s++) {
        const double w = wave_sum(v[s]);
        if (lane == 0) part[wave][s] = w;
    }
    __syncthreads();
    for (int s = 0; s < NS; s++) {
        double t = 0.0;
        for (int w = 0; w < 16; w++) t += part[w][s];
        v[s] = t;
    }
}

// ---- the normalised event loss (nerf/utils.py:521-528, C_thres == -1), forward and gradient in one launch -------------
// Per channel k, over the N rays: u = d_k / (|d_k| + 1e-9), q = pol / (|pol| + 1e-9), loss = upstream * mean (u - q)^2.
// Phase 1 forms delta (written out, un-normalised) and ONE reduction of Sdd_k = sum d_k^2, Spd_k = sum pol d_k and
// Spp = sum pol^2 in double; the loss and sum_i r_i d_i follow from those in closed form (in double: the closed form of
// the loss cancels).  With n = sqrt(Sdd), s = n + eps, sp = sqrt(Spp) + eps, c = 2 upstream / count the gradient is
//   d loss / d d_j = A d_j - B pol_j,   B = c / (s sp),   A = c / s^2 * (eps / s + Spd / (sp n))
// (1 - Sdd / (s n) written as eps / s: no cancellation), and A = c / s^2 when n == 0 -- torch's subgradient of the norm.
// Phase 2: each thread re-reads the delta values it wrote itself and the images for dp/dl, and writes both gradients.
template <int CH>
__global__ void __launch_bounds__(1024) k_event_loss_norm(const float* __restrict__ img1, const float* __restrict__ img2,
                                                          const float* __restrict__ pols, uint32_t N, EventLossCfg c,
                                                          float* __restrict__ g1, float* __restrict__ g2,
                                                          float* delta, float* __restrict__ loss) {
    constexpr int NS = 2 * CH + 1;                                   // Sdd[CH], Spd[CH], Spp
    __shared__ double part[16][NS];
    const bool luma = CH == 3 && c.use_luma;
    const int ch = luma ? 1 : CH;
    double sums[NS];
    for (int s = 0; s < NS; s++) sums[s] = 0.0;
    for (uint32_t r = threadIdx.x; r < N; r += 1024u) {
        const float* a = img1 + (size_t)r * CH;
        const float* b = img2 + (size_t)r * CH;
        const double pol = (double)pols[r];
        sums[2 * CH] += pol * pol;
        if (luma) {
            float p1, d1, p2, d2;
            ev_intensity(ev_luma(a), c, p1, d1);
            // without lin-log the reference evaluates the second term on the FIRST luma (nerf/utils.py:500): delta = 0
            ev_intensity(c.linlog ? ev_luma(b) : ev_luma(a), c, p2, d2);
            const float dl = p2 - p1;
            delta[r] = dl;
            sums[0] += (double)dl * (double)dl;
            sums[CH] += pol * (double)dl;
        } else {
            for (int k = 0; k < CH; k++) {
                float p1, d1, p2, d2;
                ev_intensity(a[k], c, p1, d1);
                ev_intensity(b[k], c, p2, d2);
                const float dl = p2 - p1;
                delta[(size_t)r * CH + k] = dl;
                sums[k] += (double)dl * (double)dl;
                sums[CH + k] += pol * (double)dl;
            }
        }
    }
    block_sums_1024<NS>(sums, part);
    const double eps = 1e-9, count = (double)N * (double)ch;
    const double cc = 2.0 * (double)c.upstream / count;
    const double spp = sums[2 * CH], sp = sqrt(spp) + eps;
    double A[CH], B[CH], total = 0.0;
    for (int k = 0; k < ch; k++) {
        const double sdd = sums[k], spd = sums[CH + k];
        const double n = sqrt(sdd), s = n + eps;
        total += sdd / (s * s) - 2.0 * spd / (s * sp) + spp / (sp * sp);
        B[k] = cc / (s * sp);
        A[k] = n > 0.0 ? cc / (s * s) * (eps / s + spd / (sp * n)) : cc / (s * s);
    }
    if (threadIdx.x == 0 && loss) loss[0] = (float)((double)c.upstream * total / count);
    for (uint32_t r = threadIdx.x; r < N; r += 1024u) {
        const float* a = img1 + (size_t)r * CH;
        const float* b = img2 + (size_t)r * CH;
        const double pol = (double)pols[r];
        float ga[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f};
        if (luma) {
            float p1, d1, p2, d2;
            ev_intensity(ev_luma(a), c, p1, d1);
            ev_intensity(c.linlog ? ev_luma(b) : ev_luma(a), c, p2, d2);
            const float gd = (float)(A[0] * (double)delta[r] - B[0] * pol);
            const float w[3] = {0.299f, 0.587f, 0.114f};
            for (int k = 0; k < 3; k++) {
                if (c.linlog) { ga[k] = -gd * d1 * w[k]; gb[k] = gd * d2 * w[k]; }
                else ga[k] = (gd * d2 - gd * d1) * w[k];
            }
        } else {
            for (int k = 0; k < CH; k++) {
                float p1, d1, p2, d2;
                ev_intensity(a[k], c, p1, d1);
                ev_intensity(b[k], c, p2, d2);
                const float gd = (float)(A[k] * (double)delta[(size_t)r * CH + k] - B[k] * pol);
                ga[k] = -gd * d1;
                gb[k] = gd * d2;
            }
        }
        for (int k = 0; k < CH; k++) {
            g1[(size_t)r * CH + k] = ga[k];
            g2[(size_t)r * CH + k] = gb[k];
        }
    }
}

// ---- the no-event hinge (nerf/utils.py:548-566), forward and gradient in one launch -------------------------------------
// loss = upstream * mean relu(|p2 - p1| - C_no) over rays x channels (luma: rays), p always lin-log (c.linlog is set by the
// entry point).  Gradient upstream / count * sign(p2 - p1) * [|p2 - p1| > C_no] * dp/dl: zero at the kink and at p2 == p1,
// as torch's relu and abs give.  One workgroup, sum in double, fixed order.
template <int CH>
__global__ void __launch_bounds__(1024) k_no_event_loss(const float* __restrict__ img1, const float* __restrict__ img2,
                                                        uint32_t N, EventLossCfg c, float c_no, float* __restrict__ g1,
                                                        float* __restrict__ g2, float* __restrict__ loss) {
    __shared__ double part[16][1];
    const bool luma = CH == 3 && c.use_luma;
    const double count = (double)N * (double)(luma ? 1 : CH);
    const float scale = (float)((double)c.upstream / count);
    double acc[1] = {0.0};
    for (uint32_t r = threadIdx.x; r < N; r += 1024u) {
        const float* a = img1 + (size_t)r * CH;
        const float* b = img2 + (size_t)r * CH;
        float ga[3] = {0.f, 0.f, 0.f}, gb[3] = {0.f, 0.f, 0.f};
        if (luma) {
            float p1, d1, p2, d2;
            ev_intensity(ev_luma(a), c, p1, d1);
            ev_intensity(ev_luma(b), c, p2, d2);
            const float dl = p2 - p1, h = fabsf(dl) - c_no;
            if (h > 0.0f) {
                acc[0] += (double)h;
                const float gd = dl > 0.0f ? scale : (dl < 0.0f ? -scale : 0.0f);
                const float w[3] = {0.299f, 0.587f, 0.114f};
                for (int k = 0; k < 3; k++) { ga[k] = -gd * d1 * w[k]; gb[k] = gd * d2 * w[k]; }
            }
        } else {
            for (int k = 0; k < CH; k++) {
                float p1, d1, p2, d2;
                ev_intensity(a[k], c, p1, d1);
                ev_intensity(b[k], c, p2, d2);
                const float dl = p2 - p1, h = fabsf(dl) - c_no;
                if (h > 0.0f) {
                    acc[0] += (double)h;
                    const float gd = dl > 0.0f ? scale : (dl < 0.0f ? -scale : 0.0f);
                    ga[k] = -gd * d1;
                    gb[k] = gd * d2;
                }
            }
        }
        for (int k = 0; k < CH; k++) {
            g1[(size_t)r * CH + k] = ga[k];
            g2[(size_t)r * CH + k] = gb[k];
        }
    }
    block_sums_1024<1>(acc, part);
    if (threadIdx.x == 0 && loss) loss[0] = (float)((double)c.upstream * acc[0] / count);
}

// ---- the implicit contrast threshold (utils/event_utils.py:69-107 with its documented (N,1) / (N,C) shapes) -------------
// Four medians of delta[i,k] / pol[i]: over the positive events, the negative ones, and the sign-consistent subsets of
// both.  One workgroup per class; a radix select, 8 bits per pass, over keys that order like the floats: each of the four
// passes recomputes the quotients from delta and pols (no scratch buffer), counts the candidates -- the values that share
// the digits found so far -- per next digit, and picks the digit that holds the wanted rank.  After four passes the key IS
// the value of rank (count - 1) / 2, torch.median's lower middle.  Counting is integer adds into LDS, so the answer does
// not depend on their order.  Early in training most deltas are exactly 0 and every key lands in one bin: each wave owns a
// private histogram, and the lanes that share the first taker's bin add once, together (c_hist_add).
__device__ __forceinline__ uint32_t c_key(float v) {                 // -inf < ... < -0 < +0 < ... < +inf, ascending
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float c_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// h: the wave's own 256 bins.  The takers that share the first taker's bin add once, by their first lane; the others
// add for themselves.  (The votes count the lanes inside the branch only.)
__device__ __forceinline__ void c_hist_add(uint32_t* h, bool take, uint32_t bin, uint32_t lane) {
    if (take) {
        const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
        const unsigned long long same = __ballot(bin == b0);
        if (bin != b0) atomicAdd(&h[bin], 1u);
        else if (lane == (uint32_t)__ffsll(same) - 1u) atomicAdd(&h[b0], (uint32_t)__popcll(same));
    }
}
__device__ __forceinline__ bool c_member(uint32_t cls, float pol, float d0) {
    // (a NaN pol fails both comparisons; a NaN d0 fails both sign conditions, as in torch)
    const bool on = pol > 0.0f, off = pol < 0.0f;
    return cls == 0u ? on : cls == 1u ? off : cls == 2u ? (on && d0 >= 0.0f) : (off && d0 <= 0.0f);
}
template <int CH>
__global__ void __launch_bounds__(1024) k_event_c_estimate(const float* __restrict__ delta, const float* __restrict__ pols,
                                                           uint32_t N, float* __restrict__ medians,
                                                           uint32_t* __restrict__ counts) {
    __shared__ uint32_t hist[16][256];
    __shared__ uint32_t tot[256];
    __shared__ uint32_t meta[2];                                     // the class's count, whether it holds a NaN
    __shared__ uint32_t sel[2];                                      // the pass's digit, the rank within it
    // events a thread loads before it counts the first: a step's 20 096 pairs are one round of loads per pass
    constexpr int kUnroll = CH == 1 ? 24 : 16;
    const uint32_t cls = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t prefix = 0u, rank = 0u, count = 0u;
    for (int pass = 0; pass < 4; pass++) {
        const uint32_t shift = 24u - 8u * (uint32_t)pass;
        const uint32_t found = pass == 0 ? 0u : (0xffffffffu << (shift + 8u));   // the key bits earlier passes fixed
        for (uint32_t j = tid; j < 16u * 256u; j += 1024u) (&hist[0][0])[j] = 0u;
        if (pass == 0 && tid < 2u) meta[tid] = sel[tid] = 0u;
        __syncthreads();
        uint32_t n_mine = 0u;
        bool nan_mine = false;
        // (wave-uniform trip count: every lane votes.  kUnroll events per thread are loaded before the first is counted:
        //  the loop is bound by the loads' latency, not by their bytes)
        for (uint32_t base = 0; base < N; base += 1024u * kUnroll) {
            float pol[kUnroll], d[kUnroll][CH];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const uint32_t i = base + (uint32_t)u * 1024u + tid; // (the entry point keeps N + 65536 below 2^32)
                const bool valid = i < N;
                pol[u] = valid ? pols[i] : 0.0f;                     // (a polarity of 0 is in no class)
                for (int k = 0; k < CH; k++) d[u][k] = valid ? delta[(size_t)i * CH + k] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const bool member = c_member(cls, pol[u], d[u][0]);
                for (int k = 0; k < CH; k++) {
                    const float q = d[u][k] / pol[u];                // IEEE division (no fast-math in this build)
                    const bool isnan = q != q;
                    const uint32_t key = c_key(q);
                    const bool take = member && !isnan && ((key ^ prefix) & found) == 0u;
                    c_hist_add(hist[wave], take, (key >> shift) & 255u, lane);
                    if (pass == 0) {
                        n_mine += member ? 1u : 0u;
                        nan_mine = nan_mine || (member && isnan);
                    }
                }
            }
        }
        if (pass == 0) {
            for (int o = 32; o > 0; o >>= 1) n_mine += (uint32_t)__shfl_down((int)n_mine, o, 64);
            const bool any_nan = __ballot(nan_mine) != 0ull;
            if (lane == 0u) {
                atomicAdd(&meta[0], n_mine);
                if (any_nan) atomicOr(&meta[1], 1u);
            }
        }
        __syncthreads();
        if (tid < 256u) {
            uint32_t t = 0u;
            for (int w = 0; w < 16; w++) t += hist[w][tid];
            tot[tid] = t;
        }
        __syncthreads();
        if (pass == 0) {
            count = meta[0];
            if (count == 0u || meta[1] != 0u) {                      // (the same for every thread of the workgroup)
                if (tid == 0u) {
                    medians[cls] = count == 0u ? 0.0f : __uint_as_float(0x7fc00000u);
                    if (counts) counts[cls] = count;
                }
                return;
            }
            rank = (count - 1u) >> 1;
        }
        if (wave == 0u) {                                            // the bin that holds `rank`: 4 bins per lane, one scan
            uint32_t a[4], s = 0u;
            for (int j = 0; j < 4; j++) { a[j] = tot[4u * lane + j]; s += a[j]; }
            uint32_t incl = s;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
                if (lane >= (uint32_t)o) incl += t;
            }
            const uint32_t excl = incl - s;
            if (rank >= excl && rank < incl) {                       // (exactly one lane: rank < the candidates' number)
                uint32_t r = rank - excl;
                for (int j = 0; j < 4; j++) {
                    if (r < a[j]) { sel[0] = 4u * lane + j; sel[1] = r; break; }
                    r -= a[j];
                }
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        rank = sel[1];
    }
    if (tid == 0u) {
        medians[cls] = c_unkey(prefix);
        if (counts) counts[cls] = count;
    }
}
}  // namespace

extern "C" int enerf_event_pair_rays(const float* events, const uint8_t* no_successor, const int64_t* num_successor,
                                     const double* pol_cumsum, uint32_t N, const int64_t* start_draw,
                                     const double* u_end, uint32_t M, uint32_t acc_max_num_evs, const double* knots,
                                     const double* rot, const double* rotvec, const double* tcoef, uint32_t K, float fx,
                                     float fy, float cx, float cy, float* rays_o1, float* rays_d1, float* rays_o2,
                                     float* rays_d2, float* pols, int64_t* start_out, int64_t* end_out,
                                     int32_t* outside_track, enerf_stream_t stream) {
    if (M == 0) return 0;
    if (N < 2 || K < 2) ENERF_BADARG("event_pair_rays: need >= 2 events and >= 2 track poses (N=%u K=%u)", N, K);
    const Intr in = {fx, fy, cx, cy};
    k_event_pair_rays<<<enerf::div_up(M, 256), 256, 0, (hipStream_t)stream>>>(
        events, no_successor, num_successor, pol_cumsum, N, start_draw, u_end, M, acc_max_num_evs, knots, rot, rotvec,
        tcoef, K, in, rays_o1, rays_d1, rays_o2, rays_d2, pols, start_out, end_out, (int*)outside_track);
    ENERF_LAUNCH_CHECK("event_pair_rays");
    return 0;
}

extern "C" int enerf_event_single_pair_rays(const float* events, uint32_t N, const int64_t* num_at_xy,
                                            const int64_t* first_at_xy, uint32_t P, const double* u_xy,
                                            const int64_t* choice, uint32_t M, const double* knots, const double* rot,
                                            const double* rotvec, const double* tcoef, uint32_t K, float fx, float fy,
                                            float cx, float cy, float* rays_o1, float* rays_d1, float* rays_o2,
                                            float* rays_d2, float* pols, int64_t* start_out, int64_t* end_out,
                                            int32_t* outside_track, int32_t* bad_choice, enerf_stream_t stream) {
    if (M == 0) return 0;
    if (N < 2 || P < 1 || K < 2)
        ENERF_BADARG("event_single_pair_rays: need >= 2 events, >= 1 pixel and >= 2 track poses (N=%u P=%u K=%u)", N, P, K);
    if (!events || !num_at_xy || !first_at_xy || !u_xy || !choice || !knots || !rot || !rotvec || !tcoef || !rays_o1 ||
        !rays_d1 || !rays_o2 || !rays_d2 || !pols || !start_out || !end_out || !outside_track || !bad_choice)
        ENERF_BADARG("event_single_pair_rays: null pointer");
    const Intr in = {fx, fy, cx, cy};
    k_event_single_pair_rays<<<div_up(M, 256), 256, 0, (hipStream_t)stream>>>(
        events, N, num_at_xy, first_at_xy, P, u_xy, choice, M, knots, rot, rotvec, tcoef, K, in, rays_o1, rays_d1, rays_o2,
        rays_d2, pols, start_out, end_out, (int*)outside_track, (int*)bad_choice);
    ENERF_LAUNCH_CHECK("event_single_pair_rays");
    return 0;
}

extern "C" int enerf_no_event_rays(const float* coords, uint32_t n_coords, const int64_t* idx, const double* u, uint32_t n,
                                   double t0_us, double t1_us, const double* knots, const double* rot,
                                   const double* rotvec, const double* tcoef, uint32_t K, float fx, float fy, float cx,
                                   float cy, float* rays_o1, float* rays_d1, float* rays_o2, float* rays_d2,
                                   double* tss_out, int32_t* outside_track, int32_t* bad_index, enerf_stream_t stream) {
    if (n == 0) return 0;
    if (n_coords < 1 || K < 2) ENERF_BADARG("no_event_rays: need >= 1 pixel and >= 2 track poses (n_coords=%u K=%u)", n_coords, K);
    if (!coords || !idx || !u || !knots || !rot || !rotvec || !tcoef || !rays_o1 || !rays_d1 || !rays_o2 || !rays_d2 ||
        !tss_out || !outside_track || !bad_index)
        ENERF_BADARG("no_event_rays: null pointer");
    const Intr in = {fx, fy, cx, cy};
    k_no_event_rays<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>(coords, n_coords, idx, u, n, t0_us, t1_us, knots, rot,
                                                                     rotvec, tcoef, K, in, rays_o1, rays_d1, rays_o2,
                                                                     rays_d2, tss_out, (int*)outside_track,
                                                                     (int*)bad_index);
    ENERF_LAUNCH_CHECK("no_event_rays");
    return 0;
}

extern "C" int enerf_event_loss_fwd_bwd(const float* image1, const float* image2, const float* pols, uint32_t N,
                                        uint32_t use_luma, uint32_t linlog, float C_thres, float log_thres, float upstream,
                                        float* grad_image1, float* grad_image2, float* delta, float* loss,
                                        enerf_stream_t stream) {
    return enerf_event_loss_fwd_bwd_c(image1, image2, pols, N, use_luma, linlog, C_thres, log_thres, upstream, grad_image1,
                                      grad_image2, delta, loss, 3, stream);
}

extern "C" int enerf_event_loss_fwd_bwd_c(const float* image1, const float* image2, const float* pols, uint32_t N,
                                          uint32_t use_luma, uint32_t linlog, float C_thres, float log_thres, float upstream,
                                          float* grad_image1, float* grad_image2, float* delta, float* loss,
                                          uint32_t channels, enerf_stream_t stream) {
    if (channels < 1u || channels > 3u) ENERF_BADARG("event_loss_fwd_bwd: %u colour channels (1..3 are served)", channels);
    if (use_luma && channels != 3u)
        ENERF_BADARG("event_loss_fwd_bwd: luma is a three-channel operation (%u channels given)", channels);
    if (N == 0) return 0;
    if (!image1 || !image2 || !pols || !grad_image1 || !grad_image2 || !delta)
        ENERF_BADARG("event_loss_fwd_bwd: images, pols, gradients and delta are required");
    const EventLossCfg c = {use_luma, linlog, C_thres, log_thres, upstream};
    const hipStream_t s = (hipStream_t)stream;
    if (C_thres == -1.0f) {                                          // the normalised loss
        if (channels == 1u)
            k_event_loss_norm<1><<<1, 1024, 0, s>>>(image1, image2, pols, N, c, grad_image1, grad_image2, delta, loss);
        else if (channels == 2u)
            k_event_loss_norm<2><<<1, 1024, 0, s>>>(image1, image2, pols, N, c, grad_image1, grad_image2, delta, loss);
        else
            k_event_loss_norm<3><<<1, 1024, 0, s>>>(image1, image2, pols, N, c, grad_image1, grad_image2, delta, loss);
        ENERF_LAUNCH_CHECK("event_loss_fwd_bwd(normalised)");
        return 0;
    }
    if (channels == 1u)
        k_event_loss<1><<<1, 1024, 0, (hipStream_t)stream>>>(image1, image2, pols, N, c, grad_image1, grad_image2, delta, loss);
    else if (channels == 2u)
        k_event_loss<2><<<1, 1024, 0, (hipStream_t)stream>>>(image1, image2, pols, N, c, grad_image1, grad_image2, delta, loss);
    else
        k_event_loss<3><<<1, 1024, 0, (hipStream_t)stream>>>(image1, image2, pols, N, c, grad_image1, grad_image2, delta, loss);
    ENERF_LAUNCH_CHECK("event_loss_fwd_bwd");
    return 0;
}

extern "C" int enerf_no_event_loss_fwd_bwd_c(const float* image1, const float* image2, uint32_t N, uint32_t use_luma,
                                             float C_no, float upstream, float* grad_image1, float* grad_image2,
                                             float* loss, uint32_t channels, enerf_stream_t stream) {
    if (channels < 1u || channels > 3u) ENERF_BADARG("no_event_loss_fwd_bwd: %u colour channels (1..3 are served)", channels);
    if (use_luma && channels != 3u)
        ENERF_BADARG("no_event_loss_fwd_bwd: luma is a three-channel operation (%u channels given)", channels);
    if (N == 0) return 0;
    if (!image1 || !image2 || !grad_image1 || !grad_image2)
        ENERF_BADARG("no_event_loss_fwd_bwd: images and gradients are required");
    const EventLossCfg c = {use_luma, 1u, 0.0f, 0.0f, upstream};     // lin-log whatever the event loss uses
    const hipStream_t s = (hipStream_t)stream;
    if (channels == 1u)
        k_no_event_loss<1><<<1, 1024, 0, s>>>(image1, image2, N, c, C_no, grad_image1, grad_image2, loss);
    else if (channels == 2u)
        k_no_event_loss<2><<<1, 1024, 0, s>>>(image1, image2, N, c, C_no, grad_image1, grad_image2, loss);
    else
        k_no_event_loss<3><<<1, 1024, 0, s>>>(image1, image2, N, c, C_no, grad_image1, grad_image2, loss);
    ENERF_LAUNCH_CHECK("no_event_loss_fwd_bwd");
    return 0;
}

extern "C" int enerf_event_c_estimate(const float* delta, const float* pols, uint32_t N, uint32_t channels, float* medians,
                                      uint32_t* counts, enerf_stream_t stream) {
    if (channels < 1u || channels > 3u) ENERF_BADARG("event_c_estimate: %u colour channels (1..3 are served)", channels);
    if ((uint64_t)N * channels > 0xffff0000ull)
        ENERF_BADARG("event_c_estimate: %u events x %u channels do not fit 32-bit counts", N, channels);
    if (N > 0 && (!delta || !pols || !medians)) ENERF_BADARG("event_c_estimate: delta, pols and medians are required");
    if (!medians) return 0;                                          // (N == 0 and nowhere to write the zeros)
    const hipStream_t s = (hipStream_t)stream;
    if (channels == 1u) k_event_c_estimate<1><<<4, 1024, 0, s>>>(delta, pols, N, medians, counts);
    else if (channels == 2u) k_event_c_estimate<2><<<4, 1024, 0, s>>>(delta, pols, N, medians, counts);
    else k_event_c_estimate<3><<<4, 1024, 0, s>>>(delta, pols, N, medians, counts);
    ENERF_LAUNCH_CHECK("event_c_estimate");
    return 0;
}
