// scan_tile.h -- the work unit of the scan-parallel effects (compressor.hip, gate.hip, phaser.hip), whose recursions are scans
// over a monoid.
//
// Work unit.  A unit (a group of rows that share one gain curve, or one row) is cut into tiles of ST_TILE = 2048 samples (256
// threads x 8 consecutive samples) and the tiles into `segments` runs of whole tiles; a workgroup owns one (unit, segment) and
// walks its tiles in order with its carries in registers (or LDS).  A tile: stage the input through LDS with coalesced loads;
// every lane runs its 8 samples from nothing for the lane's summary; Kogge-Stone scan of the summaries over the wave (shuffles),
// the 4 wave totals through LDS; second run from the true start; the result goes back through LDS for coalesced stores.
//
// segments == 1: one launch, the final pass.  Otherwise the passes in front of it run over every segment but the last and leave
// each segment's summary in the scratch buffer ([units, segments, words]); the final pass runs over every segment and composes the
// summaries in front of its own (a short loop).  Nothing crosses between workgroups but at a launch boundary: no atomics, no flags.
//
// An effect supplies its monoids (the lane summary, the combine, the carry), its Args struct (which embeds ScanCut) and the tile
// loop's body.  Nothing here multiplies and then adds: phaser.hip rounds every product on its own (fp contract off), and a
// combine's arithmetic stays in the file that derives it.
#pragma once
#include "common.h"

#include <algorithm>

namespace tfx {

constexpr int ST_THREADS = 256, ST_E = 8, ST_WAVES = ST_THREADS / 64;
constexpr int ST_TILE = ST_THREADS * ST_E;
constexpr int ST_PAD = ST_TILE + ST_TILE / ST_E;          // a tile of doubles at a + a/8: a lane's 8 words and a strided sweep both spread over the banks

// the slot of the tile's word a = k * ST_THREADS + t (the strided sweep), and of sample e of lane t (the lane's own words)
__device__ __forceinline__ int st_sweep(int a) { return a + (a >> 3); }
__device__ __forceinline__ int st_own(int t, int e) { return t * (ST_E + 1) + e; }

// the cut of T_ samples into tiles and segments: q = tiles / segments; the first r = tiles % segments segments hold one tile more
struct ScanCut {
    int64_t T_, q;
    int r, segments;
};

// what a workgroup of a pass over nseg segments per unit owns: tiles tile0 .. tile0 + ntile - 1 of `unit`
struct ScanSeg {
    int64_t unit, tile0, ntile;
    int seg;
};

__device__ __forceinline__ ScanSeg scan_segment(const ScanCut &c, int nseg)
{
    const int seg = (int)(blockIdx.x % nseg);
    return {(int64_t)(blockIdx.x / nseg), (int64_t)seg * c.q + (seg < c.r ? seg : c.r), c.q + (seg < c.r ? 1 : 0), seg};
}

// NaN-propagating maximum
__device__ __forceinline__ double st_max(double a, double b) { return (a > b || a != a) ? a : b; }

// a summary of whole 64-bit words, from the lane d in front
template <typename V> __device__ __forceinline__ V scan_shfl_up(const V &v, int d)
{
    static_assert(sizeof(V) % 8 == 0, "a summary is whole 64-bit words");
    unsigned long long w[sizeof(V) / 8];
    __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
    for (size_t k = 0; k < sizeof(V) / 8; ++k) w[k] = __shfl_up(w[k], d);
    V o;
    __builtin_memcpy(&o, w, sizeof(V));
    return o;
}

// Kogge-Stone over the wave: v becomes the summary of the lanes 0 .. lane.  combine(prev, cur, j) -> cur' puts the run of 2^j lanes
// `prev` in front of the lane's own run `cur`; every lane calls it, and its result counts where such lanes exist (lane >= 2^j).
// So a combine has no effect but its result, and must be safe on whatever a lane without lanes in front is handed as `prev`.
// It may record what it saw: the phaser's P[j] (the lane's product before stride j) is set on every lane this way, as its stages
// need it, and with a call only where lane >= 2^j that kernel lost a wave per SIMD.
template <typename V, typename F> __device__ __forceinline__ void scan_wave(V &v, int lane, F combine)
{
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const V prev = scan_shfl_up(v, 1 << j);
        const V next = combine(prev, v, j);
        if (lane >= (1 << j)) v = next;
    }
}

// the signal side of an effect that applies one gain track to the `channels` rows of a group
template <typename T> struct ScanGainIO {
    const T *x;                 // [groups, channels, T_]
    T *y;                       // [groups, channels, T_]
    T *gain;                    // [groups, T_] or null
    int channels;
};

// p = max_ch |x| of the tile at n0, coalesced, into the slots
template <typename T> __device__ __forceinline__ void scan_stage_peak(double *slot, const ScanGainIO<T> &io, int64_t T_, int64_t grp, int64_t n0)
{
    const int t = (int)threadIdx.x;
    double pm[ST_E];
#pragma unroll
    for (int k = 0; k < ST_E; ++k) pm[k] = 0.0;
    for (int ch = 0; ch < io.channels; ++ch) {
        const T *xr = io.x + (grp * io.channels + ch) * T_;
#pragma unroll
        for (int k = 0; k < ST_E; ++k) {
            const int64_t n = n0 + k * ST_THREADS + t;
            const double v = n < T_ ? fabs((double)xr[n]) : 0.0;
            pm[k] = st_max(v, pm[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < ST_E; ++k) slot[st_sweep(k * ST_THREADS + t)] = pm[k];
}

// y = dtype(g x) with the tile's gain g in the slots: coalesced, the tile's re-read comes from cache; then the gain track
template <typename T> __device__ __forceinline__ void scan_apply_gain(const double *slot, const ScanGainIO<T> &io, int64_t T_, int64_t grp, int64_t n0)
{
    const int t = (int)threadIdx.x;
    for (int ch = 0; ch < io.channels; ++ch) {
        const T *xr = io.x + (grp * io.channels + ch) * T_;
        T *yr = io.y + (grp * io.channels + ch) * T_;
#pragma unroll
        for (int k = 0; k < ST_E; ++k) {
            const int a = k * ST_THREADS + t;
            const int64_t n = n0 + a;
            if (n < T_) yr[n] = (T)(slot[st_sweep(a)] * (double)xr[n]);
        }
    }
    if (io.gain) {
#pragma unroll
        for (int k = 0; k < ST_E; ++k) {
            const int a = k * ST_THREADS + t;
            const int64_t n = n0 + a;
            if (n < T_) io.gain[grp * T_ + n] = (T)slot[st_sweep(a)];
        }
    }
}

// ---- host side ----
struct ScanPlan {
    int64_t units, tiles, segments, q, r, scratch_bytes;
};

// The size checks every plan starts with, in this order: negative size, then channels.  An effect with checks of its own that
// callers have always met after these two (the phaser) calls this first, then checks, then plans.
inline void scan_check_sizes(const char *what, int64_t units, int64_t channels, int64_t T)
{
    TFX_CHECK(units >= 0 && T >= 0, "%s: negative size", what);
    TFX_CHECK(channels >= 1 && channels <= (1 << 20), "%s: channels must be in [1, 2^20], got %lld", what, (long long)channels);
}

// Sizes alone.  `units` of `channels` rows each, T samples; segments 0 = the plan's choice: enough workgroups (auto_blocks) unless
// the units alone fill the chip (auto_units).  The order of the checks is part of the contract (a caller with several bad
// arguments sees the same error as ever): scan_check_sizes, segments, the byte count's overflow, and last the grid's.
inline ScanPlan scan_plan(const char *what, int64_t units, int64_t channels, int64_t T, int64_t segments, int64_t auto_blocks,
                          int64_t auto_units, int64_t scratch_bytes_per_unit_segment)
{
    scan_check_sizes(what, units, channels, T);
    TFX_CHECK(segments >= 0, "%s: segments must be >= 0 (0 = chosen by the plan), got %lld", what, (long long)segments);
    TFX_CHECK(units == 0 || T <= INT64_MAX / 16 / units / channels, "%s: size overflows", what);
    ScanPlan pl{};
    pl.units = units;
    pl.tiles = ceil_div(T, ST_TILE);
    int64_t s = segments;
    if (s == 0) s = (units == 0 || units >= auto_units) ? 1 : ceil_div(auto_blocks, units);
    s = std::max<int64_t>(1, std::min(s, pl.tiles));
    pl.segments = s;
    pl.q = pl.tiles / s;
    pl.r = pl.tiles % s;
    pl.scratch_bytes = s > 1 ? units * s * scratch_bytes_per_unit_segment : 0;
    TFX_CHECK(units == 0 || s < (1ll << 31) / units, "%s: size overflows", what);
    return pl;
}

inline void scan_plan_info(const ScanPlan &pl, int64_t *tile, int64_t *tiles, int64_t *segments_out, int64_t *seg_tiles,
                           int64_t *scratch_bytes)
{
    *tile = ST_TILE;
    *tiles = pl.tiles;
    *segments_out = pl.segments;
    *seg_tiles = pl.q + (pl.r ? 1 : 0);
    *scratch_bytes = pl.scratch_bytes;
}

inline ScanCut scan_cut(const ScanPlan &pl, int64_t T) { return {T, pl.q, (int)pl.r, (int)pl.segments}; }

// the buffers every forward entry takes
inline void scan_check_buffers(const char *what, const ScanPlan &pl, int64_t T, const void *x, const void *y, const void *scratch,
                               const double *state_in, const double *state_out)
{
    TFX_CHECK(pl.units * T == 0 || (x && y), "%s: null pointer", what);
    TFX_CHECK(pl.units * T == 0 || pl.segments == 1 || scratch, "%s: %lld segments need a scratch buffer of %lld bytes", what,
              (long long)pl.segments, (long long)pl.scratch_bytes);
    TFX_CHECK(!state_out || state_out != state_in, "%s: the new state needs its own buffer", what);
}

// An empty chunk (nothing in, nothing out): the state of `width` doubles per unit moves on unchanged.  Without a state given the
// new one is what init() writes; without an init, silence (zeros).
template <typename Init>
inline void scan_empty_chunk(int64_t units, int64_t width, const double *state_in, double *state_out, hipStream_t stream, Init init)
{
    const size_t bytes = (size_t)units * (size_t)width * sizeof(double);
    if (!state_out || !bytes) return;
    if (state_in) TFX_HIP(hipMemcpyAsync(state_out, state_in, bytes, hipMemcpyDeviceToDevice, stream));
    else init(bytes);
}

inline void scan_empty_chunk(int64_t units, int64_t width, const double *state_in, double *state_out, hipStream_t stream)
{
    scan_empty_chunk(units, width, state_in, state_out, stream, [&](size_t bytes) { TFX_HIP(hipMemsetAsync(state_out, 0, bytes, stream)); });
}

// One pass of the ladder: its kernel and its name in the profile.
template <typename Args> struct ScanPass {
    void (*kernel)(Args);
    const char *name;
};

// The launch ladder: every pass but the last over `segments - 1` segments per unit (none at all for one segment), then the last
// over all of them.
template <typename Args, int NP> inline void scan_launch(const ScanPass<Args> (&pass)[NP], const Args &p, const ScanPlan &pl, hipStream_t stream)
{
    for (int i = pl.segments > 1 ? 0 : NP - 1; i < NP; ++i) {
        const int64_t nseg = i == NP - 1 ? pl.segments : pl.segments - 1;
        ProfScope ps(pass[i].name, stream);
        hipLaunchKernelGGL(pass[i].kernel, dim3((unsigned)(pl.units * nseg)), dim3(ST_THREADS), 0, stream, p);
        TFX_HIP(hipGetLastError());
    }
}

}  // namespace tfx
