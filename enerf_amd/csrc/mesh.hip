// mesh.hip -- mesh export (the reference's Trainer.save_mesh: nerf/utils.py:219-249, 712-732) for gfx950: the points of
// the density lattice, and marching cubes over the field as classify / scan / emit passes.  The density query in between
// is the library's grid encoder + sigma net (enerf_amd/mesh.py strings them together); the semantics are written out in
// enerf_amd/mesh.py and DESIGN.md section 4.10.
//
//   k_mesh_lattice      the points of x-planes [x0, x0 + nx) in field order (x slowest); coordinate i of an axis is
//                       torch.linspace(lo, hi, R)[i] as the CPU computes it: fmaf(i, step, lo) below R / 2,
//                       fmaf(-(R - 1 - i), step, hi) from there on, step = (hi - lo) / (R - 1) in fp32 (from the host)
//   k_mc_classify       per lattice point p: the crossed edges it owns (+x, +y, +z: 0-3) and, when p is the origin of a
//                       cell, the cell's case and triangle count; (vertices << 32 | triangles) per point, and the sums of
//                       a 4096-point tile (plus its non-finite values) for the scan
//   k_mc_scan_tiles     exclusive scan of the tile sums (one workgroup), the two totals and the non-finite count
//   k_mc_emit_vertices  exclusive scan inside each tile -> per-point offsets (in place), and the point's vertices
//   k_mc_emit_triangles the triangles of every cell at its offset; an edge id -> (owning point, axis) -> vertex index
//                       through the scanned offsets and the owner's edge flags (no hash map, no atomics)
//
// Everything is indexed by the lattice point's linear index, cells by their origin point's, so the order of vertices and
// triangles is the field's whatever the launch geometry.  Lanes run along z: the corner loads of a wavefront are
// contiguous rows of the field.  Compiled with -ffp-contract=off; the one fused operation is the lattice's fmaf, which is
// what torch's CPU linspace computes.
#include <math.h>

#include "common.h"

#define ENERF_MC_CONST static __constant__ const
#include "mc_tables.h"

using namespace enerf;

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 16;                            // points per thread and tile
constexpr uint32_t kTile = kThreads * kItems;         // 4096 points per tile
constexpr int kScanThreads = 1024;

struct Box {
    float lo[3], hi[3], step[3];
};

__device__ __forceinline__ float lin(const Box& b, int a, uint32_t i, uint32_t R) {
    if (i < R / 2) return __fmaf_rn((float)i, b.step[a], b.lo[a]);
    return __fmaf_rn(-(float)(R - 1 - i), b.step[a], b.hi[a]);
}

__global__ void __launch_bounds__(kThreads) k_mesh_lattice(Box box, uint32_t R, uint32_t x0, uint32_t count, float* pts) {
    uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= count) return;
    uint32_t RR = R * R;
    uint32_t x = x0 + n / RR, y = (n / R) % R, z = n % R;
    float* o = pts + (size_t)n * 3;
    o[0] = lin(box, 0, x, R);
    o[1] = lin(box, 1, y, R);
    o[2] = lin(box, 2, z, R);
}

// exclusive scan of one value per thread over the workgroup (NT threads); `total` = the workgroup's sum
template <int NT>
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t* lds, uint64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int i = 0; i < NT / 64; ++i) {
            uint64_t t = lds[i];
            lds[i] = run;
            run += t;
        }
        lds[NT / 64] = run;
    }
    __syncthreads();
    uint64_t r = lds[w] + x - v;
    total = lds[NT / 64];
    __syncthreads();                                  // (lds is reused by the next call)
    return r;
}

__device__ __forceinline__ bool above(float v, double thr) { return (double)v > thr; }

__global__ void __launch_bounds__(kThreads) k_mc_classify(const float* __restrict__ u, uint32_t R, double thr,
                                                          uint64_t* __restrict__ counts, uint16_t* __restrict__ meta,
                                                          uint64_t* __restrict__ tile_sum, uint32_t* __restrict__ tile_bad) {
    __shared__ uint64_t lds[kThreads / 64 + 1];
    const uint32_t RR = R * R, n = RR * R;
    uint64_t sum = 0;
    uint32_t bad = 0;
    for (int i = 0; i < kItems; ++i) {
        uint32_t p = blockIdx.x * kTile + i * kThreads + threadIdx.x;
        if (p >= n) break;
        uint32_t x = p / RR, y = (p / R) % R, z = p % R;
        float v0 = u[p];
        bad += isfinite(v0) ? 0u : 1u;
        bool a0 = above(v0, thr);
        uint32_t f = 0;
        bool ax = false, ay = false, az = false;
        if (x + 1 < R) { ax = above(u[p + RR], thr); f |= (uint32_t)(ax != a0); }
        if (y + 1 < R) { ay = above(u[p + R], thr); f |= (uint32_t)(ay != a0) << 1; }
        if (z + 1 < R) { az = above(u[p + 1], thr); f |= (uint32_t)(az != a0) << 2; }
        uint32_t cs = 0, nt = 0;
        if (x + 1 < R && y + 1 < R && z + 1 < R) {    // corner k = (k >> 2, (k >> 1) & 1, k & 1)
            cs = (uint32_t)a0 | (uint32_t)az << 1 | (uint32_t)ay << 2 | (uint32_t)above(u[p + R + 1], thr) << 3 |
                 (uint32_t)ax << 4 | (uint32_t)above(u[p + RR + 1], thr) << 5 | (uint32_t)above(u[p + RR + R], thr) << 6 |
                 (uint32_t)above(u[p + RR + R + 1], thr) << 7;
            nt = kMcTriCount[cs];
        }
        uint64_t c = ((uint64_t)__popc(f) << 32) | nt;
        counts[p] = c;
        meta[p] = (uint16_t)(cs | f << 8);
        sum += c;
    }
    uint64_t total;
    block_excl_scan<kThreads>(sum, lds, total);
    // (non-finite values: summed per wave, then by thread 0 through the same LDS words)
    uint32_t wsum = bad;
    for (int d = 32; d >= 1; d >>= 1) wsum += __shfl_xor(wsum, d, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t b = 0;
        for (int w = 0; w < kThreads / 64; ++w) b += (uint32_t)lds[w];
        tile_sum[blockIdx.x] = total;
        tile_bad[blockIdx.x] = b;
    }
}

__global__ void __launch_bounds__(kScanThreads) k_mc_scan_tiles(uint64_t* __restrict__ tile_sum,
                                                                const uint32_t* __restrict__ tile_bad, uint32_t tiles,
                                                                int64_t* __restrict__ totals) {
    __shared__ uint64_t lds[kScanThreads / 64 + 1];
    uint64_t carry = 0, bad = 0;
    for (uint32_t base = 0; base < tiles; base += kScanThreads) {
        uint32_t i = base + threadIdx.x;
        uint64_t v = i < tiles ? tile_sum[i] : 0;
        bad += i < tiles ? tile_bad[i] : 0;
        uint64_t t;
        uint64_t ex = block_excl_scan<kScanThreads>(v, lds, t);
        if (i < tiles) tile_sum[i] = carry + ex;
        carry += t;
    }
    uint64_t b;
    block_excl_scan<kScanThreads>(bad, lds, b);
    if (threadIdx.x == 0) {
        totals[0] = (int64_t)(carry >> 32);                  // vertices
        totals[1] = (int64_t)(carry & 0xFFFFFFFFull);        // triangles
        totals[2] = (int64_t)b;                              // non-finite values
    }
}

__global__ void __launch_bounds__(kThreads) k_mc_emit_vertices(const float* __restrict__ u, uint32_t R, double thr,
                                                               uint64_t* __restrict__ counts,
                                                               const uint16_t* __restrict__ meta,
                                                               const uint64_t* __restrict__ tile_off, uint64_t V,
                                                               double* __restrict__ verts) {
    __shared__ uint64_t lds[kThreads / 64 + 1];
    const uint32_t RR = R * R, n = RR * R;
    uint64_t carry = tile_off[blockIdx.x];
    for (int i = 0; i < kItems; ++i) {
        uint32_t p = blockIdx.x * kTile + i * kThreads + threadIdx.x;
        if (blockIdx.x * kTile + i * kThreads >= n) break;          // (uniform over the workgroup)
        uint64_t c = p < n ? counts[p] : 0;
        uint64_t t;
        uint64_t off = carry + block_excl_scan<kThreads>(c, lds, t);
        carry += t;
        if (p >= n) continue;
        counts[p] = off;
        uint32_t f = meta[p] >> 8;
        if (!f) continue;
        uint32_t x = p / RR, y = (p / R) % R, z = p % R;
        double u0 = (double)u[p];
        uint64_t j = off >> 32;
        const uint32_t stride[3] = {RR, R, 1};
        for (int a = 0; a < 3; ++a) {
            if (!(f >> a & 1)) continue;
            double tt = (thr - u0) / ((double)u[p + stride[a]] - u0);
            double c3[3] = {(double)x, (double)y, (double)z};
            c3[a] = c3[a] + tt;
            if (j < V) {
                double* o = verts + j * 3;
                o[0] = c3[0];
                o[1] = c3[1];
                o[2] = c3[2];
            }
            ++j;
        }
    }
}

__global__ void __launch_bounds__(kThreads) k_mc_emit_triangles(uint32_t R, const uint64_t* __restrict__ offs,
                                                                const uint16_t* __restrict__ meta, uint64_t F,
                                                                int32_t* __restrict__ tris) {
    const uint32_t RR = R * R, n = RR * R;
    uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    uint32_t cs = meta[p] & 0xFF;
    uint32_t nt = kMcTriCount[cs];
    if (!nt) return;
    uint64_t t0 = offs[p] & 0xFFFFFFFFull;
    for (uint32_t j = 0; j < nt; ++j) {
        if (t0 + j >= F) return;
        int32_t* o = tris + (t0 + j) * 3;
        for (int k = 0; k < 3; ++k) {
            int e = kMcTriEdges[cs][j * 3 + k];
            int c = kMcEdgeCorner[e], a = kMcEdgeAxis[e];
            uint32_t q = p + (uint32_t)(c >> 2) * RR + (uint32_t)((c >> 1) & 1) * R + (uint32_t)(c & 1);
            uint32_t below = (meta[q] >> 8) & ((1u << a) - 1u);
            o[k] = (int32_t)((offs[q] >> 32) + (uint64_t)__popc(below));
        }
    }
}

struct Workspace {
    uint64_t* counts;
    uint16_t* meta;
    uint64_t* tile_sum;
    uint32_t* tile_bad;
    uint32_t tiles;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t workspace_bytes(uint32_t R, Workspace* w, void* base) {
    size_t n = (size_t)R * R * R;
    uint32_t tiles = (uint32_t)((n + kTile - 1) / kTile);
    size_t o_meta = align256(n * 8), o_sum = o_meta + align256(n * 2), o_bad = o_sum + align256((size_t)tiles * 8);
    size_t total = o_bad + align256((size_t)tiles * 4);
    if (w) {
        char* b = (char*)base;
        w->counts = (uint64_t*)b;
        w->meta = (uint16_t*)(b + o_meta);
        w->tile_sum = (uint64_t*)(b + o_sum);
        w->tile_bad = (uint32_t*)(b + o_bad);
        w->tiles = tiles;
    }
    return total;
}

int check_resolution(uint32_t R, const char* what) {
    if (R < 2 || R > 512) ENERF_BADARG("%s: resolution %u outside 2 .. 512", what, R);
    return 0;
}

}  // namespace

extern "C" {

int enerf_mesh_lattice(const float* box, uint32_t R, uint32_t x0, uint32_t nx, float* pts, enerf_stream_t stream) {
    if (int e = check_resolution(R, "mesh_lattice")) return e;
    if (!box || !pts) ENERF_BADARG("mesh_lattice: null pointer");
    if (nx == 0 || x0 >= R || nx > R - x0) ENERF_BADARG("mesh_lattice: planes [%u, %u + %u) outside 0 .. %u", x0, x0, nx, R);
    Box b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = box[a];
        b.hi[a] = box[3 + a];
        b.step[a] = box[6 + a];
    }
    uint32_t count = nx * R * R;
    k_mesh_lattice<<<div_up(count, kThreads), kThreads, 0, (hipStream_t)stream>>>(b, R, x0, count, pts);
    ENERF_LAUNCH_CHECK("mesh_lattice");
    return 0;
}

int enerf_marching_cubes_workspace(uint32_t R, uint64_t* bytes) {
    if (int e = check_resolution(R, "marching_cubes_workspace")) return e;
    if (!bytes) ENERF_BADARG("marching_cubes_workspace: null pointer");
    *bytes = workspace_bytes(R, nullptr, nullptr);
    return 0;
}

int enerf_marching_cubes_count(const float* u, uint32_t R, double threshold, void* ws, int64_t* totals,
                               enerf_stream_t stream) {
    if (int e = check_resolution(R, "marching_cubes_count")) return e;
    if (!u || !ws || !totals) ENERF_BADARG("marching_cubes_count: null pointer");
    Workspace w;
    workspace_bytes(R, &w, ws);
    hipStream_t s = (hipStream_t)stream;
    k_mc_classify<<<w.tiles, kThreads, 0, s>>>(u, R, threshold, w.counts, w.meta, w.tile_sum, w.tile_bad);
    ENERF_LAUNCH_CHECK("marching_cubes_count(classify)");
    k_mc_scan_tiles<<<1, kScanThreads, 0, s>>>(w.tile_sum, w.tile_bad, w.tiles, totals);
    ENERF_LAUNCH_CHECK("marching_cubes_count(scan)");
    return 0;
}

int enerf_marching_cubes_emit(const float* u, uint32_t R, double threshold, void* ws, uint64_t V, uint64_t F,
                              double* verts, int32_t* tris, enerf_stream_t stream) {
    if (int e = check_resolution(R, "marching_cubes_emit")) return e;
    if (!u || !ws || (V && !verts) || (F && !tris)) ENERF_BADARG("marching_cubes_emit: null pointer");
    if (V == 0 && F == 0) return 0;
    Workspace w;
    workspace_bytes(R, &w, ws);
    hipStream_t s = (hipStream_t)stream;
    k_mc_emit_vertices<<<w.tiles, kThreads, 0, s>>>(u, R, threshold, w.counts, w.meta, w.tile_sum, V, verts);
    ENERF_LAUNCH_CHECK("marching_cubes_emit(vertices)");
    uint32_t n = R * R * R;
    if (F) {
        k_mc_emit_triangles<<<div_up(n, kThreads), kThreads, 0, s>>>(R, w.counts, w.meta, F, tris);
        ENERF_LAUNCH_CHECK("marching_cubes_emit(triangles)");
    }
    return 0;
}

}  // extern "C"
