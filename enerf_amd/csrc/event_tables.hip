// event_tables.hip -- from a raw event stream to the tables the pair kernels read (csrc/event_pairs.hip), for gfx950:
// the grouping loop of EventNeRFDataset.__init__ (nerf/provider.py:1152-1199) keyed on the SENSOR pixel, and the no-event
// search of load_events_at_frame_idxs (provider.py:1283-1351).  The semantics are written out in
// enerf_amd/event_dataset.py (whose torch statement, tables_statement, is the CPU path and the tests' second opinion) and
// DESIGN.md 4.20.
//
// Every phase is a launch of its own on the caller's stream: the kernel boundary is the only ordering between
// workgroups.  No workgroup waits for another, no look-back.  Integer atomics at device scope only, and every value an
// atomic produces that reaches an output is independent of the order the atomics arrived in (counts, minima, bit sets);
// the one that is not -- the slot an event takes inside its pixel's segment -- is undone by sorting the segment, whose
// entries (stream positions) are unique, so every output has the same bits on every run.
//
//   enerf_event_tables_count
//     k_init             count = 0, first_pos = rank_of = ~0, hit bitmaps = 0, counters = 0
//     k_count            per event of the window: bounds check, then count[pix] += 1, first_pos[pix] min= i and, with
//                        no-event tables wanted, bit `pix` of the bitmap of the event's chunk
//     scan "rank"        flag(i) = first_pos[pix(i)] == i && count[pix(i)] > 1; the exclusive scan of the flags at a
//                        flagged event is its pixel's rank in first-occurrence order: rank_of[pix], num[rank] = count[pix]
//     scan "first"       exclusive scan of num over the ranks = first[rank]; its total is N, the rank scan's total is P
//     scan "free"        exclusive scan of the popcounts of the inverted bitmap words, all chunks in a row
//     k_no_event_compact one thread per bitmap word: every clear bit's pixel index at the word's offset inside its
//                        chunk's row, ascending; the rows' lengths
//     k_report           N, P, bad as int64 for the host
//   enerf_event_tables_fill
//     k_clear            cursor = 0, the list of long segments is empty
//     k_place            slot = first[rank] + cursor[pix]++ takes the event's window position
//     k_sort_small       one thread per pixel: segments of at most kThreadSeg entries by insertion; longer ones are
//                        listed; num_at_xy / first_at_xy written
//     k_sort_big         one workgroup per listed segment: a bitonic network whose every comparator is ascending (the
//                        first step of a merge mirrors the upper half), so a length that is no power of two needs no
//                        padding -- the absent entries would be +inf and never move.  Up to ENERF_EVT_SEGMENT_TILE entries
//                        the segment sits in LDS; above, the same network runs on the segment in global memory
//                        (__syncthreads orders a workgroup's global accesses), correct for any length, one round trip to
//                        L2 per comparator.
//     scan "finish"      the integer scan of the +-1 polarities along the grouped order; its write-back also gathers the
//                        event rows (rect lookup, time conversion) and the successor counts
//   enerf_no_event_coords  the chosen event-free pixels through the map
//
// A scan is three launches (csrc/event_scan.h, shared with csrc/event_stats.hip): per-tile sums (2048 values a
// workgroup), one workgroup over the sums, the tiles again with their offsets.  Sums are uint32 and wrap: the polarity
// scan reads them as two's complement.
#include <math.h>

#include "common.h"
#include "event_scan.h"

using namespace enerf;

namespace {

constexpr uint32_t kThreadSeg = 32;                    // longest segment a single thread sorts
constexpr uint32_t kTile = ENERF_EVT_SEGMENT_TILE;     // longest segment sorted in LDS
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kMaxEvents = 1u << 30;
constexpr uint32_t kMaxPixels = 1u << 26;
constexpr uint32_t kMaxChunks = 65535u;
constexpr uint32_t kSortBlocks = 1024;

static_assert((kTile & (kTile - 1)) == 0 && kTile * sizeof(uint32_t) <= 64 * 1024, "the LDS tile is a power of two <= 64 KiB");

// counters of a call, in the workspace
enum { C_P = 0, C_N = 1, C_BAD = 2, C_NBIG = 3, C_POL = 4, C_FREE = 5, C_COUNT = 8 };

struct Workspace {
    uint32_t *count, *first_pos, *rank_of, *cursor;    // [H*W]
    uint32_t *num, *first, *big;                       // [pmax]
    uint32_t* idx;                                     // [E]
    uint32_t* sums;                                    // [tiles + 1]
    uint32_t* ctr;                                     // [C_COUNT]
    uint32_t* hit;                                     // [n_chunks * words]
    uint32_t* offset;                                  // [n_chunks * words]
    uint32_t pmax, words;
    uint64_t bytes;
};

// kept pixels have two events each and are distinct: at most min(E / 2, H * W) of them (+ 1: never an empty array)
Workspace carve(void* base, uint32_t E, uint32_t HW, uint32_t n_chunks) {
    Workspace w;
    w.pmax = (E / 2 < HW ? E / 2 : HW) + 1;
    w.words = div_up(HW, 32);
    uint64_t off = 0;
    auto take = [&](uint64_t n) {
        uint32_t* p = (uint32_t*)((char*)base + off);
        off += (n * sizeof(uint32_t) + 255) / 256 * 256;
        return p;
    };
    w.count = take(HW);
    w.first_pos = take(HW);
    w.rank_of = take(HW);
    w.cursor = take(HW);
    w.num = take(w.pmax);
    w.first = take(w.pmax);
    w.big = take(w.pmax);
    w.idx = take(E);
    const uint32_t n_hit = n_chunks * w.words;
    const uint32_t longest = E > w.pmax ? (E > n_hit ? E : n_hit) : (w.pmax > n_hit ? w.pmax : n_hit);
    w.sums = take(div_up(longest, kScanTile) + 1);
    w.ctr = take(C_COUNT);
    w.hit = take(n_hit);
    w.offset = take(n_hit);
    w.bytes = off;
    return w;
}

// ---- the window --------------------------------------------------------------------------------------------------------
struct Window {
    const uint16_t* x;          // already moved to the window's first event
    const uint16_t* y;
    const int64_t* t;
    const int8_t* p;
    uint32_t E, H, W;
    double ns_per_unit;
    int64_t t_offset;
    // the pixel of event i, or kNone when its coordinates are not on the sensor (compared BEFORE anything is indexed)
    __device__ __forceinline__ uint32_t pixel(uint32_t i) const {
        const uint32_t xi = x[i], yi = y[i];
        return (xi < W && yi < H) ? yi * W + xi : kNone;
    }
    __device__ __forceinline__ double t_ns(uint32_t i) const { return (double)(t[i] + t_offset) * ns_per_unit; }
};

__global__ void __launch_bounds__(kThreads) k_init(uint32_t* __restrict__ count, uint32_t* __restrict__ first_pos,
                                                   uint32_t* __restrict__ rank_of, uint32_t HW, uint32_t* __restrict__ hit,
                                                   uint32_t n_hit, uint32_t* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < HW) {
        count[i] = 0;
        first_pos[i] = kNone;
        rank_of[i] = kNone;
    }
    if (i < n_hit) hit[i] = 0;
    if (i < C_COUNT) ctr[i] = 0;
}

__global__ void __launch_bounds__(kThreads) k_count(Window w, uint32_t tables, const double* __restrict__ edges_us,
                                                    uint32_t n_chunks, uint32_t words, uint32_t* __restrict__ count,
                                                    uint32_t* __restrict__ first_pos, uint32_t* __restrict__ hit,
                                                    uint32_t* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= w.E) return;
    const uint32_t pix = w.pixel(i);
    if (pix == kNone) {
        atomicAdd(&ctr[C_BAD], 1u);
        return;
    }
    if (tables) {
        atomicAdd(&count[pix], 1u);
        // (the minimum only ever falls: a value already below i, however stale, says this event is not the first)
        if (__atomic_load_n(&first_pos[pix], __ATOMIC_RELAXED) > i) atomicMin(&first_pos[pix], i);
    }
    if (n_chunks) {
        const double tt = w.t_ns(i) * 1e-3;             // microseconds; the product above and this one each rounded
        uint32_t lo = 0, hi = n_chunks + 1;             // the number of edges <= tt
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (edges_us[mid] <= tt) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= 1 && lo <= n_chunks) {                // edge[lo - 1] <= tt < edge[lo]
            uint32_t* word = hit + (size_t)(lo - 1) * words + (pix >> 5);
            const uint32_t bit = 1u << (pix & 31);
            // (bits are only ever set: a stale read costs one atomic, never a result)
            if (!(__atomic_load_n(word, __ATOMIC_RELAXED) & bit)) atomicOr(word, bit);
        }
    }
}

struct RankScan {
    Window w;
    const uint32_t* count;
    const uint32_t* first_pos;
    uint32_t* rank_of;
    uint32_t* num;
    uint32_t pmax;
    __device__ __forceinline__ uint32_t load(uint32_t i) const {
        const uint32_t pix = w.pixel(i);
        return (pix != kNone && first_pos[pix] == i && count[pix] > 1u) ? 1u : 0u;
    }
    __device__ __forceinline__ void store(uint32_t i, uint32_t ex, uint32_t v) const {
        if (!v || ex >= pmax) return;
        const uint32_t pix = w.pixel(i);
        rank_of[pix] = ex;
        num[ex] = count[pix];
    }
};

struct FirstScan {
    const uint32_t* num;
    uint32_t* first;
    __device__ __forceinline__ uint32_t load(uint32_t r) const { return num[r]; }
    __device__ __forceinline__ void store(uint32_t r, uint32_t ex, uint32_t) const { first[r] = ex; }
};

// the event-free pixels of word `wd` of a chunk's bitmap as set bits (the last word's tail beyond H * W masked off)
__device__ __forceinline__ uint32_t free_bits(const uint32_t* __restrict__ hit, uint32_t words, uint32_t HW, uint32_t j,
                                              uint32_t wd) {
    const uint32_t left = HW - wd * 32u;                // pixels from this word on (>= 1)
    return ~hit[(size_t)j * words + wd] & (left >= 32u ? kNone : (1u << left) - 1u);
}

// over the words of all chunks' bitmaps, chunk after chunk: offset[w] = the free pixels in front of word w
struct FreeScan {
    const uint32_t* hit;
    uint32_t* offset;
    uint32_t words, HW;
    __device__ __forceinline__ uint32_t load(uint32_t w) const {
        return (uint32_t)__popc(free_bits(hit, words, HW, w / words, w % words));
    }
    __device__ __forceinline__ void store(uint32_t w, uint32_t ex, uint32_t) const { offset[w] = ex; }
};

// one thread per bitmap word: its free pixels' linear indices, ascending, at the word's offset inside its chunk's row
__global__ void __launch_bounds__(kThreads) k_no_event_compact(const uint32_t* __restrict__ hit,
                                                               const uint32_t* __restrict__ offset, uint32_t words,
                                                               uint32_t HW, uint32_t n_chunks, int64_t* __restrict__ cand,
                                                               int64_t* __restrict__ counts) {
    const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
    if (w >= n_chunks * words) return;
    const uint32_t j = w / words, wd = w % words;
    uint32_t m = free_bits(hit, words, HW, j, wd);
    uint32_t o = offset[w] - offset[j * words];         // (<= the chunk's free pixels in front of this word)
    int64_t* out = cand + (size_t)j * HW;
    if (wd == words - 1u) counts[j] = (int64_t)(o + (uint32_t)__popc(m));
    while (m) {
        const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        if (o < HW) out[o] = (int64_t)(wd * 32u + b);
        ++o;
    }
}

__global__ void k_report(const uint32_t* __restrict__ ctr, int64_t* __restrict__ report) {
    report[0] = (int64_t)ctr[C_N];
    report[1] = (int64_t)ctr[C_P];
    report[2] = (int64_t)ctr[C_BAD];
    report[3] = 0;
}

// ---- fill --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_clear(uint32_t* __restrict__ cursor, uint32_t HW, uint32_t* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < HW) cursor[i] = 0;
    if (i == 0) ctr[C_NBIG] = 0;
}

__global__ void __launch_bounds__(kThreads) k_place(Window w, const uint32_t* __restrict__ rank_of,
                                                    const uint32_t* __restrict__ first, uint32_t* __restrict__ cursor,
                                                    uint32_t* __restrict__ idx, uint32_t N, uint32_t P) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= w.E) return;
    const uint32_t pix = w.pixel(i);
    if (pix == kNone) return;
    const uint32_t r = rank_of[pix];
    if (r >= P) return;                                 // (kNone: a pixel with a single event)
    const uint32_t slot = first[r] + atomicAdd(&cursor[pix], 1u);
    if (slot < N) idx[slot] = i;
}

__global__ void __launch_bounds__(kThreads) k_sort_small(const uint32_t* __restrict__ num, const uint32_t* __restrict__ first,
                                                         uint32_t* __restrict__ idx, uint32_t N, uint32_t P,
                                                         uint32_t* __restrict__ big, uint32_t* __restrict__ ctr,
                                                         int64_t* __restrict__ num_at_xy, int64_t* __restrict__ first_at_xy) {
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= P) return;
    const uint32_t n = num[r], b = first[r];
    num_at_xy[r] = (int64_t)n;
    first_at_xy[r] = (int64_t)b;
    if (b >= N || n > N - b) return;                    // (not a table of this N: nothing is touched)
    if (n > kThreadSeg) {
        big[atomicAdd(&ctr[C_NBIG], 1u)] = r;           // (the list's order does not reach any output)
        return;
    }
    uint32_t* a = idx + b;
    for (uint32_t k = 1; k < n; ++k) {
        const uint32_t v = a[k];
        uint32_t m = k;
        while (m > 0 && a[m - 1] > v) {
            a[m] = a[m - 1];
            --m;
        }
        a[m] = v;
    }
}

// the all-ascending bitonic network over a[0 .. n) by the workgroup's threads (entries at n and above are +inf: a
// comparator that reaches one leaves both ends as they are)
__device__ __forceinline__ void compare_swap(uint32_t* a, uint32_t lo, uint32_t hi, uint32_t n) {
    if (hi >= n) return;
    const uint32_t u = a[lo], v = a[hi];
    if (u > v) {
        a[lo] = v;
        a[hi] = u;
    }
}
__device__ void sort_network(uint32_t* a, uint32_t n) {
    uint32_t n2 = 1;
    while (n2 < n) n2 <<= 1;
    const uint32_t pairs = n2 >> 1;
    for (uint32_t k = 2; k <= n2; k <<= 1) {
        const uint32_t h = k >> 1;
        for (uint32_t q = threadIdx.x; q < pairs; q += kThreads) {         // mirror: i with i ^ (k - 1)
            const uint32_t blk = (q / h) * k, off = q % h;
            compare_swap(a, blk + off, blk + (k - 1u - off), n);
        }
        __syncthreads();
        for (uint32_t d = k >> 2; d > 0; d >>= 1) {                        // halves: i with i + d
            for (uint32_t q = threadIdx.x; q < pairs; q += kThreads) {
                const uint32_t lo = (q / d) * 2u * d + q % d;
                compare_swap(a, lo, lo + d, n);
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(kThreads) k_sort_big(const uint32_t* __restrict__ num, const uint32_t* __restrict__ first,
                                                       uint32_t* idx, uint32_t N, uint32_t P, const uint32_t* __restrict__ big,
                                                       const uint32_t* __restrict__ ctr) {
    __shared__ uint32_t tile[kTile];
    const uint32_t n_big = ctr[C_NBIG] < P ? ctr[C_NBIG] : P;
    for (uint32_t q = blockIdx.x; q < n_big; q += gridDim.x) {
        const uint32_t r = big[q];
        if (r >= P) continue;
        const uint32_t n = num[r], b = first[r];
        if (b >= N || n > N - b) continue;
        uint32_t* a = idx + b;
        if (n <= kTile) {
            for (uint32_t k = threadIdx.x; k < n; k += kThreads) tile[k] = a[k];
            __syncthreads();
            sort_network(tile, n);
            for (uint32_t k = threadIdx.x; k < n; k += kThreads) a[k] = tile[k];
            __syncthreads();
        } else {
            sort_network(a, n);
        }
    }
}

struct FinishScan {
    Window w;
    const float* rect;
    const uint32_t* idx;
    const uint32_t* rank_of;
    const uint32_t* first;
    const uint32_t* num;
    uint32_t N, P;
    float* events;
    uint8_t* no_successor;
    int64_t* num_successor;
    double* pol_cumsum;
    __device__ __forceinline__ uint32_t load(uint32_t k) const {
        const uint32_t i = idx[k];
        return (i < w.E && w.p[i] > 0) ? 1u : kNone;    // +1 / -1 in two's complement
    }
    __device__ __forceinline__ void store(uint32_t k, uint32_t ex, uint32_t v) const {
        pol_cumsum[k] = (double)(int32_t)ex;
        if (k == N - 1u) pol_cumsum[N] = (double)(int32_t)(ex + v);
        const uint32_t i = idx[k];
        const uint32_t pix = i < w.E ? w.pixel(i) : kNone;
        const uint32_t r = pix != kNone ? rank_of[pix] : kNone;
        float4 row = make_float4(NAN, NAN, NAN, NAN);
        int64_t after = 0;
        if (r < P) {
            row.x = rect ? rect[2 * (size_t)pix] : (float)w.x[i];
            row.y = rect ? rect[2 * (size_t)pix + 1] : (float)w.y[i];
            row.z = (float)w.t_ns(i);
            row.w = v == 1u ? 1.0f : -1.0f;
            after = (int64_t)(first[r] + num[r]) - (int64_t)k - 1;
        }
        reinterpret_cast<float4*>(events)[k] = row;
        no_successor[k] = after == 0 ? 1 : 0;
        num_successor[k] = after;
    }
};

__global__ void __launch_bounds__(kThreads) k_no_event_coords(const int64_t* __restrict__ pixels, uint32_t n,
                                                              const float* __restrict__ rect, uint32_t H, uint32_t W,
                                                              float* __restrict__ coords, int32_t* __restrict__ bad_index) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (n == 0) {
        if (k == 0) coords[0] = coords[1] = 0.0f;       // the reference's one dummy pixel (provider.py:1342-1343)
        return;
    }
    if (k >= n) return;
    const int64_t p = pixels[k];
    if (p < 0 || p >= (int64_t)H * (int64_t)W) {
        coords[2 * (size_t)k] = coords[2 * (size_t)k + 1] = NAN;
        if (bad_index) atomicAdd(bad_index, 1);
        return;
    }
    coords[2 * (size_t)k] = rect ? rect[2 * (size_t)p] : (float)(uint32_t)(p % W);
    coords[2 * (size_t)k + 1] = rect ? rect[2 * (size_t)p + 1] : (float)(uint32_t)(p / W);
}

int check_window(const char* what, uint64_t first, uint64_t last, uint32_t H, uint32_t W, uint32_t n_chunks) {
    if (H == 0 || W == 0 || H > 65536u || W > 65536u || (uint64_t)H * W > kMaxPixels)
        ENERF_BADARG("%s: a %u x %u sensor (1 .. 2^26 pixels, sides of at most 65536)", what, H, W);
    if (last <= first || last - first > kMaxEvents)
        ENERF_BADARG("%s: window [%llu, %llu) (1 .. 2^30 events)", what, (unsigned long long)first, (unsigned long long)last);
    if (n_chunks > kMaxChunks || (uint64_t)n_chunks * div_up(H * W, 32) > kMaxPixels)
        ENERF_BADARG("%s: %u chunks of a %u x %u sensor (at most %u, and 2^31 pixels in all)", what, n_chunks, H, W, kMaxChunks);
    return 0;
}

}  // namespace

int enerf_event_tables_workspace(uint64_t n_events, uint32_t H, uint32_t W, uint32_t n_chunks, uint64_t* bytes) {
    if (!bytes) ENERF_BADARG("event_tables_workspace: null pointer");
    if (int err = check_window("event_tables_workspace", 0, n_events, H, W, n_chunks)) return err;
    *bytes = carve(nullptr, (uint32_t)n_events, H * W, n_chunks).bytes;
    return 0;
}

int enerf_event_tables_count(const uint16_t* x, const uint16_t* y, const int64_t* t, uint64_t first, uint64_t last,
                             uint32_t H, uint32_t W, double ns_per_unit, int64_t t_offset, uint32_t tables,
                             const double* edges_us, uint32_t n_chunks, void* workspace, int64_t* report,
                             int64_t* no_event_pixels, enerf_stream_t stream) {
    if (int err = check_window("event_tables_count", first, last, H, W, n_chunks)) return err;
    if (!x || !y || !workspace || !report) ENERF_BADARG("event_tables_count: null pointer");
    if (((uintptr_t)workspace & 255) != 0) ENERF_BADARG("event_tables_count: the workspace must be 256-byte aligned");
    if (!tables && !n_chunks) ENERF_BADARG("event_tables_count: neither table kind is wanted");
    if (n_chunks && (!t || !edges_us || !no_event_pixels))
        ENERF_BADARG("event_tables_count: no-event tables need t, the chunk edges and the pixel lists");
    const uint32_t E = (uint32_t)(last - first), HW = H * W;
    const Workspace ws = carve(workspace, E, HW, n_chunks);
    hipStream_t s = (hipStream_t)stream;
    const Window w{x + first, y + first, t ? t + first : nullptr, nullptr, E, H, W, ns_per_unit, t_offset};
    const uint32_t n_hit = n_chunks * ws.words;
    const uint32_t n_init = HW > n_hit ? HW : n_hit;
    k_init<<<div_up(n_init > (uint32_t)C_COUNT ? n_init : (uint32_t)C_COUNT, kThreads), kThreads, 0, s>>>(
        ws.count, ws.first_pos, ws.rank_of, HW, ws.hit, n_hit, ws.ctr);
    ENERF_LAUNCH_CHECK("event_tables_count: init");
    k_count<<<div_up(E, kThreads), kThreads, 0, s>>>(w, tables, edges_us, n_chunks, ws.words, ws.count, ws.first_pos, ws.hit,
                                                    ws.ctr);
    ENERF_LAUNCH_CHECK("event_tables_count: count");
    if (tables) {
        const RankScan rank{w, ws.count, ws.first_pos, ws.rank_of, ws.num, ws.pmax};
        if (int err = scan(rank, E, nullptr, ws.sums, ws.ctr + C_P, s, "event_tables_count: rank scan")) return err;
        const FirstScan fs{ws.num, ws.first};
        if (int err = scan(fs, ws.pmax, ws.ctr + C_P, ws.sums, ws.ctr + C_N, s, "event_tables_count: first scan")) return err;
    }
    if (n_chunks) {
        const FreeScan fr{ws.hit, ws.offset, ws.words, HW};
        if (int err = scan(fr, n_hit, nullptr, ws.sums, ws.ctr + C_FREE, s, "event_tables_count: free-pixel scan")) return err;
        k_no_event_compact<<<div_up(n_hit, kThreads), kThreads, 0, s>>>(ws.hit, ws.offset, ws.words, HW, n_chunks,
                                                                        no_event_pixels, report + 4);
        ENERF_LAUNCH_CHECK("event_tables_count: compact");
    }
    k_report<<<1, 1, 0, s>>>(ws.ctr, report);
    ENERF_LAUNCH_CHECK("event_tables_count: report");
    return 0;
}

int enerf_event_tables_fill(const uint16_t* x, const uint16_t* y, const int64_t* t, const int8_t* p, uint64_t first,
                            uint64_t last, uint32_t H, uint32_t W, const float* rect, double ns_per_unit, int64_t t_offset,
                            void* workspace, uint32_t n_chunks, uint32_t N, uint32_t P, float* events, uint8_t* no_successor,
                            int64_t* num_successor, double* pol_cumsum, int64_t* num_at_xy, int64_t* first_at_xy,
                            enerf_stream_t stream) {
    if (int err = check_window("event_tables_fill", first, last, H, W, n_chunks)) return err;
    if (!x || !y || !t || !p || !workspace || !events || !no_successor || !num_successor || !pol_cumsum || !num_at_xy ||
        !first_at_xy)
        ENERF_BADARG("event_tables_fill: null pointer");
    if (((uintptr_t)workspace & 255) != 0) ENERF_BADARG("event_tables_fill: the workspace must be 256-byte aligned");
    if (((uintptr_t)events & 15) != 0) ENERF_BADARG("event_tables_fill: events must be 16-byte aligned");
    const uint32_t E = (uint32_t)(last - first), HW = H * W;
    const Workspace ws = carve(workspace, E, HW, n_chunks);
    if (N < 2 || N > E || P < 1 || P >= ws.pmax || 2 * (uint64_t)P > N)
        ENERF_BADARG("event_tables_fill: N = %u, P = %u are not the counts of a window of %u events", N, P, E);
    hipStream_t s = (hipStream_t)stream;
    const Window w{x + first, y + first, t + first, p + first, E, H, W, ns_per_unit, t_offset};
    k_clear<<<div_up(HW, kThreads), kThreads, 0, s>>>(ws.cursor, HW, ws.ctr);
    ENERF_LAUNCH_CHECK("event_tables_fill: clear");
    k_place<<<div_up(E, kThreads), kThreads, 0, s>>>(w, ws.rank_of, ws.first, ws.cursor, ws.idx, N, P);
    ENERF_LAUNCH_CHECK("event_tables_fill: place");
    k_sort_small<<<div_up(P, kThreads), kThreads, 0, s>>>(ws.num, ws.first, ws.idx, N, P, ws.big, ws.ctr, num_at_xy,
                                                         first_at_xy);
    ENERF_LAUNCH_CHECK("event_tables_fill: sort");
    k_sort_big<<<P < kSortBlocks ? P : kSortBlocks, kThreads, 0, s>>>(ws.num, ws.first, ws.idx, N, P, ws.big, ws.ctr);
    ENERF_LAUNCH_CHECK("event_tables_fill: segment sort");
    const FinishScan fin{w, rect, ws.idx, ws.rank_of, ws.first, ws.num, N, P, events, no_successor, num_successor, pol_cumsum};
    return scan(fin, N, nullptr, ws.sums, ws.ctr + C_POL, s, "event_tables_fill: finish");
}

// testing aid: the two sort launches of enerf_event_tables_fill on segments of the caller's choice
int enerf_debug_event_segment_sort(uint32_t* idx, uint32_t N, const uint32_t* num, const uint32_t* first, uint32_t P,
                                   void* workspace, enerf_stream_t stream) {
    if (!idx || !num || !first || !workspace) ENERF_BADARG("debug_event_segment_sort: null pointer");
    if (((uintptr_t)workspace & 7) != 0) ENERF_BADARG("debug_event_segment_sort: the workspace must be 8-byte aligned");
    if (N < 1 || N > kMaxEvents || P < 1 || P > N) ENERF_BADARG("debug_event_segment_sort: N = %u, P = %u", N, P);
    int64_t* num_at_xy = (int64_t*)workspace;          // [P], [P], then the list of long segments [P] and the counters
    int64_t* first_at_xy = num_at_xy + P;
    uint32_t* big = (uint32_t*)(first_at_xy + P);
    uint32_t* ctr = big + P;
    hipStream_t s = (hipStream_t)stream;
    k_clear<<<1, kThreads, 0, s>>>(nullptr, 0, ctr);
    ENERF_LAUNCH_CHECK("debug_event_segment_sort: clear");
    k_sort_small<<<div_up(P, kThreads), kThreads, 0, s>>>(num, first, idx, N, P, big, ctr, num_at_xy, first_at_xy);
    ENERF_LAUNCH_CHECK("debug_event_segment_sort: sort");
    k_sort_big<<<P < kSortBlocks ? P : kSortBlocks, kThreads, 0, s>>>(num, first, idx, N, P, big, ctr);
    ENERF_LAUNCH_CHECK("debug_event_segment_sort: segment sort");
    return 0;
}

int enerf_no_event_coords(const int64_t* pixels, uint32_t n, const float* rect, uint32_t H, uint32_t W, float* coords,
                          int32_t* bad_index, enerf_stream_t stream) {
    if (H == 0 || W == 0 || (uint64_t)H * W > kMaxPixels) ENERF_BADARG("no_event_coords: a %u x %u sensor", H, W);
    if (!coords || (n && !pixels)) ENERF_BADARG("no_event_coords: null pointer");
    if (n > kMaxPixels) ENERF_BADARG("no_event_coords: %u pixels", n);
    k_no_event_coords<<<div_up(n ? n : 1u, kThreads), kThreads, 0, (hipStream_t)stream>>>(pixels, n, rect, H, W, coords,
                                                                                        bad_index);
    ENERF_LAUNCH_CHECK("no_event_coords");
    return 0;
}
