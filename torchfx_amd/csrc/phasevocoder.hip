// phasevocoder.hip -- the phase vocoder (tfx_phase_vocoder_forward, torchaudio.functional.phase_vocoder's meaning): the spectrum
// [rows, F, bins] that stft.hip writes is read once, in place, and the stretched one [rows, Fo, bins] that istft.hip reads is
// written once.  Nothing else touches global memory but, for long rows, one summary per (row, segment, bin).
//
// Definition.  Output frame t stands at p = fl(t rate) (double), i = floor(p), alpha = R(p - i); frames F and F + 1 are zeros.
//     mag[t]   = alpha |X[i+1]| + (1 - alpha) |X[i]|                                   in the signal's real dtype R
//     phase[t] = angle(X[0]) + sum_{s<t} (angle(X[i_s + 1]) - angle(X[i_s]))            (mod one turn)
//     Y[t]     = mag[t] (cos, sin)(phase[t])
// torchaudio's increment wrap(d - pa) + pa differs from d by whole turns, so its expected advance pa never reaches Y.  The phase
// is kept in turns as 64-bit fixed point (2^64 = one turn): A[j] = rint(atan2(im, re) / 2 pi * 2^64) in double, 0 for the zero
// bin, and phase[t] = A[0] + sum (A[i+1] - A[i]) in wrapping unsigned arithmetic.  Integer addition is associative: a value's
// bits depend on its own (row, bin) track up to its frame alone -- not on the bin tile, the segment count, the other rows -- and
// the phase is as exact after 10^7 frames as after ten.  At rate 1 the sum telescopes to A[t].
//
// Work split.  Lanes own neighbouring bins: a wave reads 64 consecutive complex values of one frame (512 B at complex64), so the
// frames need no staging and the kernel uses no LDS.  A workgroup of `tile` threads (64, 128 or 256: one lane per bin) owns one
// (row, bin tile, time segment) and walks the segment's output frames in time order, PV_U at a time: first every load of the
// batch is issued (the frames the batch needs that the lane does not hold yet), then the batch is computed.  Per lane the running
// phase, A[i], A[i+1], |X[i]| and |X[i+1]| live in registers; i never decreases, so an input frame's angle and modulus are computed
// once, when i moves, and reused while it stays (rate < 1: one atan2 per input frame), and a frame that no output stands on
// (rate > 1) is never read.  The only dependence along time is one integer add.
//
// Time segments.  rows x bin tiles seldom fill the chip (64 rows x 513 bins are 576 waves), so a row's Fo output frames are cut
// into `segments` runs of seg_frames.  One segment: one launch.  Otherwise two, the scan kernels' ladder (scan_tile.h): a summary
// pass over all but the last segment leaves each segment's increment sum and its poison flag in `scratch`, the final pass adds
// the summaries in front of its own segment (a short loop) and produces the output.  Nothing crosses between workgroups but at
// the launch boundary: no atomics, no flags to wait on.  The sums are integers, so both routes give the same bits.
//
// Non-finite input.  A NaN has no integer: a bin with a NaN or Inf component counts as angle 0 and sets the lane's poison bit,
// which sticks.  From the first output frame that reads such a bin every later frame of that (row, bin) is NaN in both parts;
// earlier frames, other bins and other rows keep their bits.  The summaries carry the bit across the segments.
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <cmath>

namespace tfx {

namespace {

typedef unsigned long long pv_u64;

template <typename R> struct alignas(2 * sizeof(R)) PvCx {
    R x, y;
};

constexpr int PV_U = 8;                         // output frames per batch: up to 2 PV_U loads of a lane in flight
constexpr int64_t PV_FILL_WAVES = 2048;         // rows x bin tiles of at least two waves per SIMD (256 CUs) run as one launch
constexpr int64_t PV_WANT_WAVES = 4096;         // what a cut row aims at: the summary pass repeats the angles, so it has to pay
constexpr int64_t PV_MIN_SEG_FRAMES = 32;       // a segment shorter than this is all start-up (A[0], two fresh frames, the prefix)

template <typename R> struct PvArgs {
    const PvCx<R> *spec;    // [rows, F, bins]
    PvCx<R> *out;           // [rows, Fo, bins]
    pv_u64 *sums;           // [rows, segments, bins]: the segment's sum of increments (the last segment's is never written)
    unsigned *flags;        // [rows, segments, bins]: 1 where the segment read a non-finite bin
    int64_t F, Fo, bins, seg_frames;
    int tiles, segments;
    double rate;
};

// one bin of one input frame: its angle in 2^-64 turns, its modulus, its share of the poison bit
template <typename R> struct PvBin {
    pv_u64 a;
    R m;
};

template <typename R, bool MAG> __device__ __forceinline__ PvBin<R> pv_bin(const PvCx<R> v, bool &bad)
{
    const double re = (double)v.x, im = (double)v.y;
    const bool finite = (re - re == 0.0) && (im - im == 0.0);
    bad |= !finite;
    PvBin<R> b;
    b.a = 0;
    if (finite && (re != 0.0 || im != 0.0)) {
        // |turns| <= 1/2, so |w| <= 2^63: +2^63 (angle pi) wraps to -2^63, the same point of the circle
        double w = rint(atan2(im, re) * 0.15915494309189533577 * 18446744073709551616.0);
        if (w >= 9223372036854775808.0) w -= 18446744073709551616.0;
        b.a = (pv_u64)(long long)w;
    }
    b.m = (R)0;
    if constexpr (MAG) b.m = sqrt(fma(v.x, v.x, v.y * v.y));
    return b;
}

// frame j of the lane's bin; frames F and F + 1 (and nothing else reaches here) are zeros
template <typename R> __device__ __forceinline__ PvCx<R> pv_load(const PvCx<R> *col, int64_t j, int64_t F, int64_t bins)
{
    PvCx<R> v;
    v.x = (R)0, v.y = (R)0;
    if (j < F) v = col[j * bins];
    return v;
}

// FINAL: the pass that writes the output (every segment); otherwise the summary pass (every segment but the last)
template <typename R, bool FINAL> __global__ __launch_bounds__(256) void phase_vocoder_kernel(const PvArgs<R> p)
{
    const int nseg = FINAL ? p.segments : p.segments - 1;
    const int64_t blk = blockIdx.x;
    const int tile = (int)(blk % p.tiles), seg = (int)((blk / p.tiles) % nseg);
    const int64_t row = blk / ((int64_t)p.tiles * nseg);
    const int64_t bin = (int64_t)tile * blockDim.x + threadIdx.x;
    if (bin >= p.bins) return;                                          // no barrier below
    const int64_t t0 = (int64_t)seg * p.seg_frames, t1 = t0 + p.seg_frames < p.Fo ? t0 + p.seg_frames : p.Fo;
    const PvCx<R> *col = p.spec + row * p.F * p.bins + bin;
    const int64_t sbase = row * p.segments * p.bins + bin;

    bool bad = false;
    pv_u64 P = 0;
    if constexpr (FINAL) {
        bool ignore = false;                                            // a non-finite X[0] is segment 0's to report
        P = pv_bin<R, false>(col[0], ignore).a;
        for (int k = 0; k < seg; ++k) {
            P += p.sums[sbase + (int64_t)k * p.bins];
            bad |= p.flags[sbase + (int64_t)k * p.bins] != 0;
        }
    }

    PvBin<R> b0{}, b1{};                                                 // frames i and i + 1 of the last output frame
    int64_t ip = -2;                                                    // its i; -2: nothing held
    for (int64_t tb = t0; tb < t1; tb += PV_U) {
        PvCx<R> ra[PV_U], rb[PV_U];
        int64_t iq = ip;
#pragma unroll
        for (int u = 0; u < PV_U; ++u) {
            if (tb + u < t1) {
                const int64_t i = (int64_t)floor(__dmul_rn((double)(tb + u), p.rate)), d = i - iq;
                if (d >= 2) ra[u] = pv_load(col, i, p.F, p.bins);       // d == 1: frame i is the frame i + 1 held
                if (d >= 1) rb[u] = pv_load(col, i + 1, p.F, p.bins);
                iq = i;
            }
        }
#pragma unroll
        for (int u = 0; u < PV_U; ++u) {
            const int64_t t = tb + u;
            if (t < t1) {
                const double pos = __dmul_rn((double)t, p.rate);
                const int64_t i = (int64_t)floor(pos), d = i - ip;
                if (d >= 1) {
                    if (d == 1) b0 = b1;
                    else b0 = pv_bin<R, FINAL>(ra[u], bad);
                    b1 = pv_bin<R, FINAL>(rb[u], bad);
                }
                ip = i;
                if constexpr (FINAL) {
                    const R alpha = (R)(pos - (double)i);
                    const R mag = alpha * b1.m + ((R)1 - alpha) * b0.m;
                    double s, c;
                    sincospi((double)(long long)P * 0x1p-63, &s, &c);  // 2 x turns in [-1, 1]
                    PvCx<R> y;
                    y.x = (R)((double)mag * c), y.y = (R)((double)mag * s);
                    if (bad) y.x = y.y = (R)NAN;
                    p.out[(row * p.Fo + t) * p.bins + bin] = y;
                }
                P += b1.a - b0.a;
            }
        }
    }
    if constexpr (!FINAL) {
        p.sums[sbase + (int64_t)seg * p.bins] = P;
        p.flags[sbase + (int64_t)seg * p.bins] = bad ? 1u : 0u;
    }
}

struct PvPlan {
    int64_t Fo = 0, tile = 64, tiles = 0, segments = 1, seg_frames = 0, launches = 0, workgroups = 0, scratch_bytes = 0;
};

// Every check on the sizes, and the geometry, in one place.  segments 0 = the plan's choice.
PvPlan pv_plan(const char *what, int64_t rows, int64_t frames, int64_t bins, double rate, int dtype, int64_t segments)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: dtype must be TFX_F32 or TFX_F64", what);
    TFX_CHECK(rows >= 0 && frames >= 0 && bins >= 0, "%s: negative size (rows %lld, frames %lld, bins %lld)", what, (long long)rows,
              (long long)frames, (long long)bins);
    TFX_CHECK(std::isfinite(rate) && rate > 0.0, "%s: rate must be a finite number > 0, got %g", what, rate);
    TFX_CHECK(segments >= 0, "%s: segments must be >= 0 (0 = chosen by the plan), got %lld", what, (long long)segments);
    TFX_CHECK(frames <= (int64_t)1 << 40 && bins <= (int64_t)1 << 24, "%s: size out of range (frames %lld, bins %lld)", what,
              (long long)frames, (long long)bins);
    const double fo = std::ceil((double)frames / rate);                 // as torch.arange(0, frames, rate) sizes itself
    TFX_CHECK(fo <= (double)((int64_t)1 << 40), "%s: %lld frames at rate %g give more than 2^40 output frames", what, (long long)frames, rate);
    PvPlan pl;
    pl.Fo = (int64_t)fo;
    const int64_t longest = frames > pl.Fo ? frames : pl.Fo;
    TFX_CHECK(rows == 0 || bins == 0 || longest <= INT64_MAX / 32 / rows / bins, "%s: size overflows", what);
    if (rows * bins * frames == 0) {
        pl.segments = 0;
        return pl;
    }
    // the bin tile: one lane per bin, 64 to 256 lanes; the fewest lanes past the last bin win, then the larger workgroup
    int64_t waste = INT64_MAX;
    for (int64_t t = 256; t >= 64; t /= 2)
        if (ceil_div(bins, t) * t - bins < waste) waste = ceil_div(bins, t) * t - bins, pl.tile = t;
    pl.tiles = ceil_div(bins, pl.tile);
    const int64_t waves = rows * ceil_div(bins, 64);
    int64_t s = segments;
    if (s == 0) {
        s = waves >= PV_FILL_WAVES ? 1 : ceil_div(PV_WANT_WAVES, waves);
        // the final pass adds up to s - 1 summaries per lane, one dependent load each: s * s <= Fo keeps that prefix loop
        // shorter than the segment's own frames (one row of 64 bins and 10^6 frames: 1000 segments, not 4096 of 245 frames)
        int64_t most = pl.Fo / PV_MIN_SEG_FRAMES;
        const int64_t root = (int64_t)std::sqrt((double)pl.Fo);
        if (most > root) most = root;
        if (s > most) s = most;
    }
    if (s > pl.Fo) s = pl.Fo;
    if (s < 1) s = 1;
    pl.seg_frames = ceil_div(pl.Fo, s);
    pl.segments = ceil_div(pl.Fo, pl.seg_frames);                        // every segment holds a frame; the last may be short
    pl.launches = pl.segments > 1 ? 2 : 1;
    pl.workgroups = rows * pl.tiles * pl.segments;
    TFX_CHECK(pl.tiles * pl.segments <= 0x7fffffffLL / rows, "%s: %lld workgroups exceed the grid", what,
              (long long)pl.workgroups);
    pl.scratch_bytes = pl.segments > 1 ? rows * pl.segments * bins * (int64_t)(sizeof(pv_u64) + sizeof(unsigned)) : 0;
    return pl;
}

template <typename R>
void pv_launch(const void *spec, void *out, void *scratch, int64_t rows, int64_t frames, int64_t bins, double rate, const PvPlan &pl,
               hipStream_t stream)
{
    PvArgs<R> p{};
    p.spec = (const PvCx<R> *)spec; p.out = (PvCx<R> *)out;
    p.sums = (pv_u64 *)scratch;
    p.flags = (unsigned *)((pv_u64 *)scratch + (pl.segments > 1 ? rows * pl.segments * bins : 0));
    p.F = frames; p.Fo = pl.Fo; p.bins = bins; p.seg_frames = pl.seg_frames;
    p.tiles = (int)pl.tiles; p.segments = (int)pl.segments;
    p.rate = rate;
    if (pl.segments > 1) {
        ProfScope ps("phase_vocoder_summary", stream);
        hipLaunchKernelGGL((phase_vocoder_kernel<R, false>), dim3((unsigned)(rows * pl.tiles * (pl.segments - 1))), dim3((unsigned)pl.tile),
                           0, stream, p);
        TFX_HIP(hipGetLastError());
    }
    ProfScope ps("phase_vocoder_kernel", stream);
    hipLaunchKernelGGL((phase_vocoder_kernel<R, true>), dim3((unsigned)pl.workgroups), dim3((unsigned)pl.tile), 0, stream, p);
    TFX_HIP(hipGetLastError());
}

}  // namespace

void phase_vocoder_forward(const void *spec, void *out, int dtype, int64_t rows, int64_t frames, int64_t bins, double rate,
                           int64_t segments, void *scratch, hipStream_t stream)
{
    const char *what = "phase_vocoder_forward";
    const PvPlan pl = pv_plan(what, rows, frames, bins, rate, dtype, segments);
    if (pl.segments == 0) return;                                       // empty work: nothing to launch
    TFX_CHECK(spec && out, "%s: null pointer", what);
    TFX_CHECK(pl.segments == 1 || scratch, "%s: %lld segments need a scratch buffer of %lld bytes", what, (long long)pl.segments,
              (long long)pl.scratch_bytes);
    if (dtype == TFX_F32) pv_launch<float>(spec, out, scratch, rows, frames, bins, rate, pl, stream);
    else pv_launch<double>(spec, out, scratch, rows, frames, bins, rate, pl, stream);
}

void phase_vocoder_plan_info(int64_t rows, int64_t frames, int64_t bins, double rate, int dtype, int64_t segments, int64_t *out_frames,
                             int64_t *bin_tile, int64_t *segments_out, int64_t *seg_frames, int64_t *launches, int64_t *workgroups,
                             int64_t *scratch_bytes)
{
    const PvPlan pl = pv_plan("phase_vocoder_plan_info", rows, frames, bins, rate, dtype, segments);
    *out_frames = pl.Fo;
    *bin_tile = pl.tile;
    *segments_out = pl.segments;
    *seg_frames = pl.seg_frames;
    *launches = pl.launches;
    *workgroups = pl.workgroups;
    *scratch_bytes = pl.scratch_bytes;
}

}  // namespace tfx
