// pose_track.h -- the camera at an arbitrary time, and the ray of a pixel through it, as device code: the one statement
// of the pose track that every kernel of event_pairs.hip evaluates.
//   pose_at   the reference's "computing poses online" branch (nerf/provider.py:1411-1420): rotation by scipy's Slerp
//             (R_i * exp(alpha * log(R_i^T R_{i+1}))), translation by interp1d(kind="cubic"), from the per-segment tables
//             enerf_amd/pose_interp.py prepares once; in double like scipy, then rounded to fp32 as
//             `torch.Tensor(get_hom_trafos(...))` does;
//   cam_dir / ray_of   get_event_rays (nerf/utils.py:184-216): pixel -> unit camera direction -> world direction / origin.
// Needs -ffp-contract=off (every product and sum rounded on its own), which the whole library is built with.
#pragma once
#include "common.h"

namespace enerf {

struct Intr {
    float fx, fy, cx, cy;
};

// index of the track segment [knots[i], knots[i+1]] holding t (last segment for t == knots[K-1]); -1 outside the track
__device__ __forceinline__ int find_segment(const double* __restrict__ knots, uint32_t K, double t) {
    if (!(t >= knots[0]) || !(t <= knots[K - 1])) return -1;
    uint32_t lo = 0, hi = K - 1;                      // invariant: knots[lo] <= t <= knots[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (knots[mid] <= t) lo = mid; else hi = mid;
    }
    return (int)lo;
}

// c2w[3][4] (fp32) at time t
__device__ __forceinline__ bool pose_at(const double* __restrict__ knots, const double* __restrict__ rot,
                                        const double* __restrict__ rotvec, const double* __restrict__ tcoef, uint32_t K,
                                        double t, float (&m)[3][4]) {
    const int s = find_segment(knots, K, t);
    if (s < 0) return false;
    const double h = knots[s + 1] - knots[s];
    const double alpha = (t - knots[s]) / h;
    // Rodrigues: exp(alpha * w)
    const double wx = alpha * rotvec[s * 3], wy = alpha * rotvec[s * 3 + 1], wz = alpha * rotvec[s * 3 + 2];
    const double th2 = wx * wx + wy * wy + wz * wz;
    const double th = sqrt(th2);
    double a, b;                                      // exp = I + a [w]x + b [w]x^2
    if (th < 1e-6) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
    }
    double E[3][3];
    E[0][0] = 1.0 - b * (wy * wy + wz * wz); E[0][1] = -a * wz + b * wx * wy;        E[0][2] = a * wy + b * wx * wz;
    E[1][0] = a * wz + b * wx * wy;          E[1][1] = 1.0 - b * (wx * wx + wz * wz); E[1][2] = -a * wx + b * wy * wz;
    E[2][0] = -a * wy + b * wx * wz;         E[2][1] = a * wx + b * wy * wz;          E[2][2] = 1.0 - b * (wx * wx + wy * wy);
    const double* R = rot + (size_t)s * 9;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            m[i][j] = (float)(R[i * 3] * E[0][j] + R[i * 3 + 1] * E[1][j] + R[i * 3 + 2] * E[2][j]);
    // translation: cubic in (t - knots[s]), coefficients highest power first: tcoef[s][k][axis]
    const double u = t - knots[s];
    const double* c = tcoef + (size_t)s * 12;
    for (int ax = 0; ax < 3; ax++) m[ax][3] = (float)(((c[ax] * u + c[3 + ax]) * u + c[6 + ax]) * u + c[9 + ax]);
    return true;
}

// unit camera direction of pixel (x, y) (get_event_rays): fp32, z = 1
__device__ __forceinline__ void cam_dir(const Intr& in, float x, float y, float& dx, float& dy, float& dz) {
    const float us = (x - in.cx) / in.fx, vs = (y - in.cy) / in.fy;
    const float nrm = sqrtf((us * us + vs * vs) + 1.0f);
    dx = us / nrm;
    dy = vs / nrm;
    dz = 1.0f / nrm;
}

__device__ __forceinline__ void ray_of(const float (&m)[3][4], float dx, float dy, float dz, float* o, float* d) {
    o[0] = m[0][3]; o[1] = m[1][3]; o[2] = m[2][3];
    // torch.sum(dirs_cams[..., None, :] * c2w[..., :3, :3], axis=-1): products rounded, then summed left to right
    for (int i = 0; i < 3; i++) d[i] = (dx * m[i][0] + dy * m[i][1]) + dz * m[i][2];
}

}  // namespace enerf
