// event_stats.hip -- the loader's side of a raw event stream, for gfx950: per-pixel event counts, the accumulation images
// of utils/plot_utils.py render_ev_accumulation (nerf/provider.py:227-230, :313-316), a hot-pixel mask from the counts'
// moments, and the stream without the events of masked pixels.  The semantics are written out in
// enerf_amd/event_dataset.py (whose torch statements are the CPU path) and DESIGN.md 4.22.
//
// Integer work only.  Every value an atomic produces that reaches an output is independent of the order the atomics
// arrived in (counts, maxima, integer sums), and the compaction's positions come from a scan, so every output has the
// same bits on every run.
//
//   enerf_event_pixel_stats
//     k_stats_zero       counts = 0, the last-event arrays that are wanted = 0, bad = 0
//     k_stats            per event of the window: bounds check, then counts[pix][p > 0] += 1; on request
//                        last_sensor[pix] max= i + 1 and, through the map and its in-bounds test, last_rect[cell] max= i + 1
//   enerf_event_accumulation_image
//     k_image            four pixels a thread: a pixel's last event's polarity to its three bytes, 12 bytes = three words
//   enerf_event_count_moments
//     k_moments          n, S, Q of c = counts[pix][0] + counts[pix][1] in uint64: registers, the wavefront, LDS, then three
//                        atomics a workgroup
//   enerf_event_hot_mask
//     k_hot_mask         mask[pix] = c > T; the hot pixels and their events summed the same way
//   enerf_event_stream_compact
//     the scan of csrc/event_scan.h over the keep flags (sensor check, then the mask at the event's pixel); its write-back
//     scatters x, y, t, p to the scanned position.  The flags are recomputed in the write-back (3 bytes read twice) rather
//     than stored (4 bytes written, 4 read).
//
// Atomics: one no-return device-scope atomic per event and array, like k_count of csrc/event_tables.hip.  Events of one
// pixel inside a wavefront are NOT combined first: on the measured workload (2 M events, 20 hot pixels
// holding 5 % of them) the counts pass runs at 17 G atomics a second at 640 x 480 and at 1280 x 720 alike, twice
// torch.bincount's rate, and the hot addresses do not show.
#include "common.h"
#include "event_scan.h"

using namespace enerf;

namespace {

constexpr uint32_t kMaxEvents = 1u << 30;
constexpr uint32_t kMaxPixels = 1u << 26;
constexpr uint32_t kReduceBlocks = 1024;               // most workgroups of a reduction over the sensor

__global__ void __launch_bounds__(kThreads) k_stats_zero(int32_t* __restrict__ counts, uint32_t* __restrict__ last_sensor,
                                                         uint32_t* __restrict__ last_rect, uint32_t HW,
                                                         unsigned long long* __restrict__ bad) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < HW) {
        reinterpret_cast<int2*>(counts)[i] = make_int2(0, 0);
        if (last_sensor) last_sensor[i] = 0;
        if (last_rect) last_rect[i] = 0;
    }
    if (i == 0) *bad = 0;
}

// x, y, p already moved to the window's first event
__global__ void __launch_bounds__(kThreads) k_stats(const uint16_t* __restrict__ x, const uint16_t* __restrict__ y,
                                                    const int8_t* __restrict__ p, uint32_t E, uint32_t H, uint32_t W,
                                                    const float* __restrict__ rect, int32_t* __restrict__ counts,
                                                    uint32_t* __restrict__ last_sensor, uint32_t* __restrict__ last_rect,
                                                    unsigned long long* __restrict__ bad) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= E) return;
    const uint32_t xi = x[i], yi = y[i];
    if (!(xi < W && yi < H)) {                          // compared BEFORE anything is indexed
        atomicAdd(bad, 1ull);
        return;
    }
    const uint32_t pix = yi * W + xi;
    atomicAdd(&counts[2 * (size_t)pix + (p[i] > 0 ? 1 : 0)], 1);
    // (a maximum only ever rises: a value already above i, however stale, says a later event has been here)
    if (last_sensor && __atomic_load_n(&last_sensor[pix], __ATOMIC_RELAXED) < i + 1u) atomicMax(&last_sensor[pix], i + 1u);
    if (last_rect) {
        const float2 r = reinterpret_cast<const float2*>(rect)[pix];
        if (r.x >= 0.0f && r.y >= 0.0f && r.x < (float)W && r.y < (float)H) {           // false for NaN
            const uint32_t cell = (uint32_t)r.y * W + (uint32_t)r.x;                    // truncated; < H * W by the test
            if (__atomic_load_n(&last_rect[cell], __ATOMIC_RELAXED) < i + 1u) atomicMax(&last_rect[cell], i + 1u);
        }
    }
}

// the three bytes of a cell: untouched white, last polarity -1 (255, 0, 0), +1 (0, 0, 255)
__device__ __forceinline__ uint32_t cell_colour(const uint32_t* __restrict__ last_event, const int8_t* __restrict__ p,
                                                uint32_t E, uint32_t pix) {
    const uint32_t l = last_event[pix];
    if (l == 0 || l > E) return 0xffffffu;              // (an l beyond the window reads nothing)
    return p[l - 1u] > 0 ? 0xff0000u : 0x0000ffu;       // byte 0 in the low bits
}

__global__ void __launch_bounds__(kThreads) k_image(const uint32_t* __restrict__ last_event, const int8_t* __restrict__ p,
                                                    uint32_t E, uint32_t HW, uint8_t* __restrict__ image) {
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x;                // pixels 4q .. 4q + 3
    const uint32_t base = 4u * q;
    if (base >= HW) return;
    if (base + 4u <= HW) {
        const uint32_t a = cell_colour(last_event, p, E, base), b = cell_colour(last_event, p, E, base + 1u),
                       c = cell_colour(last_event, p, E, base + 2u), d = cell_colour(last_event, p, E, base + 3u);
        uint32_t* out = reinterpret_cast<uint32_t*>(image) + 3 * (size_t)q;
        out[0] = a | (b << 24);
        out[1] = (b >> 8) | (c << 16);
        out[2] = (c >> 16) | (d << 8);
        return;
    }
    for (uint32_t pix = base; pix < HW; ++pix) {
        const uint32_t c = cell_colour(last_event, p, E, pix);
        image[3 * (size_t)pix] = (uint8_t)c;
        image[3 * (size_t)pix + 1] = (uint8_t)(c >> 8);
        image[3 * (size_t)pix + 2] = (uint8_t)(c >> 16);
    }
}

// the workgroup's sums of up to three uint64 values a thread, added to out[0 .. K) by thread 0 (all threads must call)
template <int K>
__device__ __forceinline__ void block_sum_to(unsigned long long (&v)[K], unsigned long long* __restrict__ out) {
    __shared__ unsigned long long lds[kWaves][K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int d = kWave / 2; d > 0; d >>= 1) v[k] += __shfl_down(v[k], d, kWave);
    if (lane_id() == 0)
        for (int k = 0; k < K; ++k) lds[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < K; ++k) {
            unsigned long long s = 0;
            for (int w = 0; w < kWaves; ++w) s += lds[w][k];
            if (s) atomicAdd(&out[k], s);
        }
}

__device__ __forceinline__ unsigned long long pixel_count(const int32_t* __restrict__ counts, uint32_t pix) {
    const int2 c = reinterpret_cast<const int2*>(counts)[pix];
    return (unsigned long long)(uint32_t)c.x + (unsigned long long)(uint32_t)c.y;
}

__global__ void __launch_bounds__(kThreads) k_moments(const int32_t* __restrict__ counts, uint32_t HW,
                                                      unsigned long long* __restrict__ moments) {
    unsigned long long v[3] = {0, 0, 0};
    for (uint32_t pix = blockIdx.x * kThreads + threadIdx.x; pix < HW; pix += gridDim.x * kThreads) {
        const unsigned long long c = pixel_count(counts, pix);
        v[0] += c > 0 ? 1ull : 0ull;
        v[1] += c;
        v[2] += c * c;
    }
    block_sum_to<3>(v, moments);
}

__global__ void __launch_bounds__(kThreads) k_hot_mask(const int32_t* __restrict__ counts, uint32_t HW,
                                                       unsigned long long threshold, uint8_t* __restrict__ mask,
                                                       unsigned long long* __restrict__ report) {
    unsigned long long v[2] = {0, 0};
    for (uint32_t pix = blockIdx.x * kThreads + threadIdx.x; pix < HW; pix += gridDim.x * kThreads) {
        const unsigned long long c = pixel_count(counts, pix);
        const bool hot = c > threshold;
        mask[pix] = hot ? 1 : 0;
        v[0] += hot ? 1ull : 0ull;
        v[1] += hot ? c : 0ull;
    }
    block_sum_to<2>(v, report);
}

__global__ void k_zero_words(unsigned long long* __restrict__ a, uint32_t* __restrict__ b, uint32_t n) {
    if (threadIdx.x < n) {
        if (a) a[threadIdx.x] = 0;
        if (b) b[threadIdx.x] = 0;
    }
}

// keep flag of event i: on the sensor (compared BEFORE the mask is indexed) and not at a masked pixel.  `bad` is set in the
// functor of the sums pass alone, which sees every event once.
struct CompactScan {
    const uint16_t* x;
    const uint16_t* y;
    const int64_t* t;
    const int8_t* p;
    uint32_t H, W;
    const uint8_t* mask;
    uint16_t* x_out;
    uint16_t* y_out;
    int64_t* t_out;
    int8_t* p_out;
    uint32_t* bad;
    __device__ __forceinline__ uint32_t load(uint32_t i) const {
        const uint32_t xi = x[i], yi = y[i];
        if (!(xi < W && yi < H)) {
            if (bad) atomicAdd(bad, 1u);
            return 0u;
        }
        return mask[yi * W + xi] ? 0u : 1u;
    }
    __device__ __forceinline__ void store(uint32_t i, uint32_t ex, uint32_t v) const {
        if (!v) return;                                 // (ex < the kept events before i + 1 <= i + 1: inside the outputs)
        x_out[ex] = x[i];
        y_out[ex] = y[i];
        t_out[ex] = t[i];
        p_out[ex] = p[i];
    }
};

int check_sensor(const char* what, uint32_t H, uint32_t W) {
    if (H == 0 || W == 0 || H > 65536u || W > 65536u || (uint64_t)H * W > kMaxPixels)
        ENERF_BADARG("%s: a %u x %u sensor (1 .. 2^26 pixels, sides of at most 65536)", what, H, W);
    return 0;
}

uint32_t reduce_blocks(uint32_t HW) {
    const uint32_t nb = div_up(HW, kThreads);
    return nb < kReduceBlocks ? nb : kReduceBlocks;
}

}  // namespace

int enerf_event_pixel_stats(const uint16_t* x, const uint16_t* y, const int8_t* p, uint64_t first, uint64_t last, uint32_t H,
                            uint32_t W, const float* rect, int32_t* counts, uint32_t* last_sensor, uint32_t* last_rect,
                            uint64_t* bad, enerf_stream_t stream) {
    if (int err = check_sensor("event_pixel_stats", H, W)) return err;
    if (last <= first || last - first > kMaxEvents)
        ENERF_BADARG("event_pixel_stats: window [%llu, %llu) (1 .. 2^30 events)", (unsigned long long)first,
                     (unsigned long long)last);
    if (!x || !y || !p || !counts || !bad) ENERF_BADARG("event_pixel_stats: null pointer");
    if (last_rect && !rect) ENERF_BADARG("event_pixel_stats: the rectified last-event array needs the map");
    if (((uintptr_t)counts & 7) != 0 || ((uintptr_t)rect & 7) != 0 || ((uintptr_t)bad & 7) != 0)
        ENERF_BADARG("event_pixel_stats: counts, rect and bad must be 8-byte aligned");
    const uint32_t E = (uint32_t)(last - first), HW = H * W;
    hipStream_t s = (hipStream_t)stream;
    k_stats_zero<<<div_up(HW, kThreads), kThreads, 0, s>>>(counts, last_sensor, last_rect, HW, (unsigned long long*)bad);
    ENERF_LAUNCH_CHECK("event_pixel_stats: zero");
    k_stats<<<div_up(E, kThreads), kThreads, 0, s>>>(x + first, y + first, p + first, E, H, W, rect, counts, last_sensor,
                                                    last_rect, (unsigned long long*)bad);
    ENERF_LAUNCH_CHECK("event_pixel_stats");
    return 0;
}

int enerf_event_accumulation_image(const uint32_t* last_event, const int8_t* p, uint64_t first, uint64_t last, uint32_t H,
                                   uint32_t W, uint8_t* image, enerf_stream_t stream) {
    if (int err = check_sensor("event_accumulation_image", H, W)) return err;
    if (last <= first || last - first > kMaxEvents)
        ENERF_BADARG("event_accumulation_image: window [%llu, %llu) (1 .. 2^30 events)", (unsigned long long)first,
                     (unsigned long long)last);
    if (!last_event || !p || !image) ENERF_BADARG("event_accumulation_image: null pointer");
    if (((uintptr_t)image & 3) != 0) ENERF_BADARG("event_accumulation_image: the image must be 4-byte aligned");
    const uint32_t HW = H * W;
    k_image<<<div_up(div_up(HW, 4u), kThreads), kThreads, 0, (hipStream_t)stream>>>(last_event, p + first,
                                                                                   (uint32_t)(last - first), HW, image);
    ENERF_LAUNCH_CHECK("event_accumulation_image");
    return 0;
}

int enerf_event_count_moments(const int32_t* counts, uint32_t H, uint32_t W, uint64_t* moments, enerf_stream_t stream) {
    if (int err = check_sensor("event_count_moments", H, W)) return err;
    if (!counts || !moments) ENERF_BADARG("event_count_moments: null pointer");
    if (((uintptr_t)counts & 7) != 0 || ((uintptr_t)moments & 7) != 0)
        ENERF_BADARG("event_count_moments: counts and moments must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    k_zero_words<<<1, kWave, 0, s>>>((unsigned long long*)moments, nullptr, 3);
    ENERF_LAUNCH_CHECK("event_count_moments: zero");
    k_moments<<<reduce_blocks(H * W), kThreads, 0, s>>>(counts, H * W, (unsigned long long*)moments);
    ENERF_LAUNCH_CHECK("event_count_moments");
    return 0;
}

int enerf_event_hot_mask(const int32_t* counts, uint32_t H, uint32_t W, uint64_t threshold, uint8_t* mask, uint64_t* report,
                         enerf_stream_t stream) {
    if (int err = check_sensor("event_hot_mask", H, W)) return err;
    if (!counts || !mask || !report) ENERF_BADARG("event_hot_mask: null pointer");
    if (((uintptr_t)counts & 7) != 0 || ((uintptr_t)report & 7) != 0)
        ENERF_BADARG("event_hot_mask: counts and report must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    k_zero_words<<<1, kWave, 0, s>>>((unsigned long long*)report, nullptr, 2);
    ENERF_LAUNCH_CHECK("event_hot_mask: zero");
    k_hot_mask<<<reduce_blocks(H * W), kThreads, 0, s>>>(counts, H * W, (unsigned long long)threshold, mask,
                                                        (unsigned long long*)report);
    ENERF_LAUNCH_CHECK("event_hot_mask");
    return 0;
}

int enerf_event_stream_compact_workspace(uint64_t n_events, uint64_t* bytes) {
    if (!bytes) ENERF_BADARG("event_stream_compact_workspace: null pointer");
    if (n_events < 1 || n_events > kMaxEvents)
        ENERF_BADARG("event_stream_compact_workspace: %llu events (1 .. 2^30)", (unsigned long long)n_events);
    *bytes = ((uint64_t)div_up((uint32_t)n_events, kScanTile) + 1) * sizeof(uint32_t);
    return 0;
}

int enerf_event_stream_compact(const uint16_t* x, const uint16_t* y, const int64_t* t, const int8_t* p, uint64_t n_events,
                               uint32_t H, uint32_t W, const uint8_t* mask, void* workspace, uint16_t* x_out,
                               uint16_t* y_out, int64_t* t_out, int8_t* p_out, uint32_t* report, enerf_stream_t stream) {
    if (int err = check_sensor("event_stream_compact", H, W)) return err;
    if (n_events < 1 || n_events > kMaxEvents)
        ENERF_BADARG("event_stream_compact: %llu events (1 .. 2^30)", (unsigned long long)n_events);
    if (!x || !y || !t || !p || !mask || !workspace || !x_out || !y_out || !t_out || !p_out || !report)
        ENERF_BADARG("event_stream_compact: null pointer");
    if (((uintptr_t)workspace & 3) != 0) ENERF_BADARG("event_stream_compact: the workspace must be 4-byte aligned");
    const uint32_t E = (uint32_t)n_events, nb = div_up(E, kScanTile);
    uint32_t* sums = (uint32_t*)workspace;
    hipStream_t s = (hipStream_t)stream;
    k_zero_words<<<1, kWave, 0, s>>>(nullptr, report, 2);
    ENERF_LAUNCH_CHECK("event_stream_compact: zero");
    CompactScan f{x, y, t, p, H, W, mask, x_out, y_out, t_out, p_out, report + 1};
    k_scan_sums<CompactScan><<<nb, kThreads, 0, s>>>(f, E, nullptr, sums);
    ENERF_LAUNCH_CHECK("event_stream_compact: sums");
    k_scan_top<<<1, kThreads, 0, s>>>(sums, nb, report);
    ENERF_LAUNCH_CHECK("event_stream_compact: top");
    f.bad = nullptr;
    k_scan_apply<CompactScan><<<nb, kThreads, 0, s>>>(f, E, nullptr, sums);
    ENERF_LAUNCH_CHECK("event_stream_compact: scatter");
    return 0;
}
