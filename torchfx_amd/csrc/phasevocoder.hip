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

// ---- identity phase locking (Laroche & Dolson 1999, III-C) ----------------------------------------------------------------------
//
// Definition.  mag, A and the plain update U[t,k] = phi[t-1,k] + (A[i_{t-1}+1,k] - A[i_{t-1},k]) (U[0,k] = A[0,k]) are the plain
// vocoder's.  Bin k is a peak of frame t iff mag[t,k] > mag[t,j] for every in-range j in {k-2, k-1, k+1, k+2} (a comparison with a
// NaN is false); P(k) is the nearest peak, the lower one at equal distance.  A frame without a peak keeps phi = U; otherwise
//     phi[t,k] = U[t,P(k)] + (A[i_t,k] - A[i_t,P(k)])
// so a peak keeps its own update and every other bin the analysis frame's phase relation to its peak.  Peaks depend on the moduli
// alone, never on a phase: the path a bin's phase takes through the bins is decided by the data, not by the state it carries.
//
// Work split.  The bins of a frame are coupled, so one workgroup owns ALL bins of one (row, time segment): `threads` lanes, BPT
// bins each, bin = j threads + tid -- a wave still reads 64 consecutive complex values of a frame.  Per owned bin a lane keeps
// U, A[i], A[i+1], |X[i]|, |X[i+1]| in registers (an input frame's atan2 and modulus once, when i moves; loads batched ahead of use).
//
// LDS, per frame: mag[k] (one buffer), V[k] = U[t,k] - A[i_t,k] (two buffers, by frame parity), the peak mask (one 64-bit word per
// 64 bins, from __ballot) and one sticky poison word.  phi[t,k] = V[P(k)] + A[i_t,k]: storing the difference halves what the
// gather reads, and the lane's own A[i_t,k] never leaves its registers.  Two barriers per frame:
//     write mag, V[par]   | barrier 1 |   neighbours' mag -> peak flag -> ballot -> mask word; poison   | barrier 2 |
//     nearest peak from the mask, gather V[par][P], sincos, store; U for the next frame
// mag and the mask need one buffer each (their readers all stand before the next barrier); V needs two, because the next frame's
// V is written before barrier 1 while a slow wave still gathers this frame's.  The nearest peak is a count-leading-zeros scan
// down from the bin's word and a count-trailing-zeros scan up from it, word by word -- no loop over bins.
//
// Time segments.  As above, but the summary is of another kind: U[t1,k] = U[t0, src[k]] + sum[k] with src the bin of the entry
// state the phase descends from and sum the integers added along that path.  The summary pass runs the same frame loop on
// (src, sum) instead of U (LDS: V = sum - A[i_t,k] and src, both by parity) and writes src, sum per (row, segment, bin) and one
// poison flag per (row, segment).  The writing pass starts from A[0,.], composes the summaries in front of its segment -- one LDS
// gather and one barrier per earlier segment -- and walks its frames.  Integer sums are exact: one launch or two, the same bits.
//
// Non-finite input.  The paths couple the bins, so the poison is the row's: from the first output frame that reads a NaN or Inf bin,
// every bin of every later frame of that row is NaN (the workgroup ORs the lanes' bits per frame), that frame included.
constexpr int64_t PL_MAX_BINS = 4097;           // n_fft 8192: 9 bins per lane at 512 lanes, 4608 slots, 148 040 B of the CU's 160 KB LDS
constexpr int64_t PL_WANT_WAVES = 4096;         // what a cut row aims at, as PV_WANT_WAVES
constexpr int64_t PL_FILL_WAVES = 2048;
constexpr int64_t PL_MIN_SEG_FRAMES = 32;

template <typename R> struct PlArgs {
    const PvCx<R> *spec;    // [rows, F, bins]
    PvCx<R> *out;           // [rows, Fo, bins]
    pv_u64 *sums;           // [rows, segments, bins]: the sum along the path into the segment's exit state
    int *srcs;              // [rows, segments, bins]: the bin of the entry state that path starts from
    unsigned *flags;        // [rows, segments]: 1 where the segment read a non-finite bin
    int64_t F, Fo, bins, seg_frames;
    int segments, slots, words;     // slots = threads x BPT >= bins, words = slots / 64
    double rate;
};

// the peak nearest to bin k (the lower one at equal distance) from the mask words; k itself when the frame has none
__device__ __forceinline__ int pl_nearest(const pv_u64 *mask, int k, int words)
{
    const int w = k >> 6, b = k & 63;
    int lo = -1, hi = -1;
    pv_u64 x = mask[w] & (~0ull >> (63 - b));                           // bits 0 .. b: peaks at or below k
    for (int v = w;;) {
        if (x) { lo = v * 64 + 63 - __builtin_clzll(x); break; }
        if (--v < 0) break;
        x = mask[v];
    }
    x = mask[w] & ((~0ull << b) << 1);                                  // bits b + 1 .. 63: peaks above k
    for (int v = w;;) {
        if (x) { hi = v * 64 + __builtin_ctzll(x); break; }
        if (++v >= words) break;
        x = mask[v];
    }
    if (lo < 0) return hi < 0 ? k : hi;
    return hi < 0 || k - lo <= hi - k ? lo : hi;
}

// FINAL: the pass that writes the output (every segment); otherwise the summary pass (every segment but the last)
template <typename R, int BPT, bool FINAL>
__global__ __launch_bounds__(BPT >= 4 ? 512 : 256) void phase_lock_kernel(const PlArgs<R> p)
{
    constexpr int PL_U = BPT >= 4 ? 1 : 4;                              // output frames per load batch: what the registers hold
    constexpr bool AHEAD = BPT < 9;                                     // 9 bins a lane: no room for 18 loads in flight, each is
                                                                        // issued where it is used and the other waves hide it
    extern __shared__ __attribute__((aligned(16))) unsigned char pl_smem[];
    pv_u64 *V = (pv_u64 *)pl_smem;                                      // [2][slots]
    pv_u64 *mask = V + 2 * p.slots;                                     // [words]
    R *mg = (R *)(mask + p.words);                                      // [slots]
    int *S = (int *)(mg + p.slots);                                     // [2][slots], the summary pass only
    unsigned *poison = (unsigned *)(S + (FINAL ? 0 : 2 * p.slots));

    const int tid = (int)threadIdx.x, nt = (int)blockDim.x, bins = (int)p.bins;
    const int nseg = FINAL ? p.segments : p.segments - 1;
    const int seg = (int)(blockIdx.x % nseg);
    const int64_t row = blockIdx.x / nseg;
    const int64_t t0 = (int64_t)seg * p.seg_frames, t1 = t0 + p.seg_frames < p.Fo ? t0 + p.seg_frames : p.Fo;
    const PvCx<R> *spec = p.spec + row * p.F * p.bins;
    const int64_t sbase = row * p.segments * p.bins;

    if (tid == 0) *poison = 0;                                          // ordered before its first reader by barrier 1
    bool bad = false, rowbad = false;
    pv_u64 Uk[BPT];                                                     // FINAL: U[t,k]; summary: the sum along the path
    int src[BPT];
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int k = j * nt + tid;
        Uk[j] = 0, src[j] = k;
        if constexpr (FINAL) {
            bool ignore = false;                                        // a non-finite X[0] is segment 0's to report
            if (k < bins) Uk[j] = pv_bin<R, false>(spec[k], ignore).a;
        }
    }
    int par = 0;                                                        // which V (and S) the next writer takes
    if constexpr (FINAL) {
        for (int q = 0; q < seg; ++q, par ^= 1) {                       // the entry state, one gather per earlier segment
            pv_u64 *Vq = V + par * p.slots;
#pragma unroll
            for (int j = 0; j < BPT; ++j) Vq[j * nt + tid] = Uk[j];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                const int k = j * nt + tid;
                if (k < bins) Uk[j] = Vq[p.srcs[sbase + (int64_t)q * bins + k]] + p.sums[sbase + (int64_t)q * bins + k];
            }
            rowbad |= p.flags[row * p.segments + q] != 0;
        }
    }

    PvBin<R> b0[BPT], b1[BPT];                                          // frames i and i + 1 of the last output frame
#pragma unroll
    for (int j = 0; j < BPT; ++j) b0[j] = PvBin<R>{}, b1[j] = PvBin<R>{};
    int64_t ip = -2;                                                    // its i; -2: nothing held
    for (int64_t tb = t0; tb < t1; tb += PL_U) {
        PvCx<R> ra[PL_U][BPT], rb[PL_U][BPT];
        int64_t iq = ip;
#pragma unroll
        for (int u = 0; u < PL_U; ++u) {
            if (tb + u < t1) {
                const int64_t i = (int64_t)floor(__dmul_rn((double)(tb + u), p.rate)), d = i - iq;
#pragma unroll
                for (int j = 0; j < BPT; ++j) {
                    const int k = j * nt + tid;
                    ra[u][j].x = ra[u][j].y = rb[u][j].x = rb[u][j].y = (R)0;                   // a slot past the last bin: zeros
                    if (AHEAD && k < bins) {
                        if (d >= 2) ra[u][j] = pv_load(spec + k, i, p.F, p.bins);               // d == 1: frame i is the i + 1 held
                        if (d >= 1) rb[u][j] = pv_load(spec + k, i + 1, p.F, p.bins);
                    }
                }
                iq = i;
            }
        }
#pragma unroll
        for (int u = 0; u < PL_U; ++u) {
            const int64_t t = tb + u;
            if (t < t1) {                                               // uniform: every lane meets every barrier and ballot
                const double pos = __dmul_rn((double)t, p.rate);
                const int64_t i = (int64_t)floor(pos), d = i - ip;
                const R alpha = (R)(pos - (double)i);
                pv_u64 *Vt = V + par * p.slots;
                int *St = S + par * p.slots;
#pragma unroll
                for (int j = 0; j < BPT; ++j) {
                    const int k = j * nt + tid;
                    if (d >= 1) {
                        if constexpr (!AHEAD) {
                            if (k < bins) {
                                if (d >= 2) ra[u][j] = pv_load(spec + k, i, p.F, p.bins);
                                rb[u][j] = pv_load(spec + k, i + 1, p.F, p.bins);
                            }
                        }
                        if (d == 1) b0[j] = b1[j];
                        else b0[j] = pv_bin<R, true>(ra[u][j], bad);
                        b1[j] = pv_bin<R, true>(rb[u][j], bad);
                    }
                    mg[k] = alpha * b1[j].m + ((R)1 - alpha) * b0[j].m;
                    Vt[k] = Uk[j] - b0[j].a;
                    if constexpr (!FINAL) St[k] = src[j];
                }
                ip = i;
                __syncthreads();                                        // 1: the frame's mag (and V, S) stand
#pragma unroll
                for (int j = 0; j < BPT; ++j) {
                    const int k = j * nt + tid;
                    bool pk = k < bins;
                    if (pk) {
                        const R m = mg[k];
                        if (k >= 1) pk &= m > mg[k - 1];
                        if (k >= 2) pk &= m > mg[k - 2];
                        if (k + 1 < bins) pk &= m > mg[k + 1];
                        if (k + 2 < bins) pk &= m > mg[k + 2];
                    }
                    const pv_u64 word = __ballot(pk);                   // the wave's 64 bins are one aligned word
                    if ((tid & 63) == 0) mask[k >> 6] = word;
                }
                if (__ballot(bad) != 0 && (tid & 63) == 0) *poison = 1; // sticky: never cleared
                __syncthreads();                                        // 2: the mask and the poison stand
                rowbad |= *poison != 0;
#pragma unroll
                for (int j = 0; j < BPT; ++j) {
                    const int k = j * nt + tid;
                    const int pkb = pl_nearest(mask, k, p.words);
                    const pv_u64 phi = Vt[pkb] + b0[j].a;
                    if constexpr (FINAL) {
                        if (k < bins) {
                            double s, c;
                            sincospi((double)(long long)phi * 0x1p-63, &s, &c);                // 2 x turns in [-1, 1]
                            const R mag = mg[k];
                            PvCx<R> y;
                            y.x = (R)((double)mag * c), y.y = (R)((double)mag * s);
                            if (rowbad) y.x = y.y = (R)NAN;
                            p.out[(row * p.Fo + t) * p.bins + k] = y;
                        }
                    } else {
                        src[j] = St[pkb];
                    }
                    Uk[j] = phi + (b1[j].a - b0[j].a);
                }
                par ^= 1;
            }
        }
    }
    if constexpr (!FINAL) {
#pragma unroll
        for (int j = 0; j < BPT; ++j) {
            const int k = j * nt + tid;
            if (k < bins) {
                p.sums[sbase + (int64_t)seg * bins + k] = Uk[j];
                p.srcs[sbase + (int64_t)seg * bins + k] = src[j];
            }
        }
        if (tid == 0) p.flags[row * p.segments + seg] = rowbad ? 1u : 0u;
    }
}

struct PlPlan {
    int64_t Fo = 0, threads = 0, bpt = 0, lds_bytes = 0, segments = 0, seg_frames = 0, launches = 0, workgroups = 0, scratch_bytes = 0;
};

int64_t pl_lds_bytes(int64_t slots, int dtype, bool summary)
{
    return slots * (16 + (dtype == TFX_F32 ? 4 : 8) + (summary ? 8 : 0)) + slots / 64 * 8 + 8;
}

// The locked route's geometry, decided here alone (the sizes are pv_plan's to check).  segments 0 = the plan's choice.
PlPlan pl_plan(const char *what, int64_t rows, int64_t frames, int64_t bins, double rate, int dtype, int64_t segments)
{
    const PvPlan base = pv_plan(what, rows, frames, bins, rate, dtype, segments);
    TFX_CHECK(bins <= PL_MAX_BINS, "%s: phase_lock serves at most %lld bins (n_fft 8192), got %lld", what, (long long)PL_MAX_BINS,
              (long long)bins);
    PlPlan pl;
    pl.Fo = base.Fo;
    if (base.segments == 0) return pl;
    // up to 256 lanes while 3 bins a lane serve; then 5 bins a lane, past 2560 bins 9, on up to 512 lanes (256 registers a lane:
    // the state of the owned bins, the double-precision atan2 / sincos and, up to 5 bins a lane, the loads in flight fit them)
    pl.bpt = ceil_div(bins, (int64_t)256);
    if (pl.bpt > 3) pl.bpt = bins <= 5 * 512 ? 5 : 9;
    pl.threads = ceil_div(ceil_div(bins, pl.bpt), (int64_t)64) * 64;
    const int64_t waves = rows * (pl.threads / 64);
    int64_t s = segments;
    if (s == 0) {
        s = waves >= PL_FILL_WAVES ? 1 : ceil_div(PL_WANT_WAVES, waves);
        // the writing pass gathers s - 1 summaries, a barrier each: s * s <= Fo keeps that shorter than the segment's own frames
        int64_t most = pl.Fo / PL_MIN_SEG_FRAMES;
        const int64_t root = (int64_t)std::sqrt((double)pl.Fo);
        if (most > root) most = root;
        if (s > most) s = most;
    }
    if (s > pl.Fo) s = pl.Fo;
    if (s < 1) s = 1;
    pl.seg_frames = ceil_div(pl.Fo, s);
    pl.segments = ceil_div(pl.Fo, pl.seg_frames);
    pl.launches = pl.segments > 1 ? 2 : 1;
    pl.workgroups = rows * pl.segments;
    TFX_CHECK(pl.segments <= 0x7fffffffLL / rows, "%s: %lld workgroups exceed the grid", what, (long long)pl.workgroups);
    pl.lds_bytes = pl_lds_bytes(pl.threads * pl.bpt, dtype, pl.segments > 1);
    pl.scratch_bytes = pl.segments > 1 ? rows * pl.segments * bins * (int64_t)(sizeof(pv_u64) + sizeof(int)) + rows * pl.segments * 4 : 0;
    return pl;
}

template <typename R, int BPT, bool FINAL> void pl_launch_one(const PlArgs<R> &p, int64_t workgroups, int threads, int64_t lds, hipStream_t stream)
{
    static size_t attr[TFX_MAX_DEVICES] = {};
    size_t &have = attr[current_device()];
    if ((size_t)lds > have) {
        TFX_HIP(hipFuncSetAttribute((const void *)phase_lock_kernel<R, BPT, FINAL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        have = (size_t)lds;
    }
    ProfScope ps(FINAL ? "phase_lock_kernel" : "phase_lock_summary", stream);
    hipLaunchKernelGGL((phase_lock_kernel<R, BPT, FINAL>), dim3((unsigned)workgroups), dim3((unsigned)threads), (size_t)lds, stream, p);
    TFX_HIP(hipGetLastError());
}

template <typename R, int BPT>
void pl_launch(const void *spec, void *out, void *scratch, int64_t rows, int64_t frames, int64_t bins, double rate, int dtype,
               const PlPlan &pl, hipStream_t stream)
{
    const int64_t n = pl.segments > 1 ? rows * pl.segments * bins : 0;
    PlArgs<R> p{};
    p.spec = (const PvCx<R> *)spec; p.out = (PvCx<R> *)out;
    p.sums = (pv_u64 *)scratch;
    p.srcs = (int *)((pv_u64 *)scratch + n);
    p.flags = (unsigned *)(p.srcs + n);
    p.F = frames; p.Fo = pl.Fo; p.bins = bins; p.seg_frames = pl.seg_frames;
    p.segments = (int)pl.segments; p.slots = (int)(pl.threads * pl.bpt); p.words = p.slots / 64;
    p.rate = rate;
    if (pl.segments > 1) pl_launch_one<R, BPT, false>(p, rows * (pl.segments - 1), (int)pl.threads, pl.lds_bytes, stream);
    pl_launch_one<R, BPT, true>(p, pl.workgroups, (int)pl.threads, pl_lds_bytes(p.slots, dtype, false), stream);
}

template <typename R>
void pl_launch_bpt(const void *spec, void *out, void *scratch, int64_t rows, int64_t frames, int64_t bins, double rate, int dtype,
                   const PlPlan &pl, hipStream_t stream)
{
    switch (pl.bpt) {
    case 1: return pl_launch<R, 1>(spec, out, scratch, rows, frames, bins, rate, dtype, pl, stream);
    case 2: return pl_launch<R, 2>(spec, out, scratch, rows, frames, bins, rate, dtype, pl, stream);
    case 3: return pl_launch<R, 3>(spec, out, scratch, rows, frames, bins, rate, dtype, pl, stream);
    case 5: return pl_launch<R, 5>(spec, out, scratch, rows, frames, bins, rate, dtype, pl, stream);
    default: return pl_launch<R, 9>(spec, out, scratch, rows, frames, bins, rate, dtype, pl, stream);
    }
}

}  // namespace

void phase_vocoder_locked_forward(const void *spec, void *out, int dtype, int64_t rows, int64_t frames, int64_t bins, double rate,
                                  int64_t segments, void *scratch, hipStream_t stream)
{
    const char *what = "phase_vocoder_locked_forward";
    const PlPlan pl = pl_plan(what, rows, frames, bins, rate, dtype, segments);
    if (pl.segments == 0) return;                                       // empty work: nothing to launch
    TFX_CHECK(spec && out, "%s: null pointer", what);
    TFX_CHECK(pl.segments == 1 || scratch, "%s: %lld segments need a scratch buffer of %lld bytes", what, (long long)pl.segments,
              (long long)pl.scratch_bytes);
    if (dtype == TFX_F32) pl_launch_bpt<float>(spec, out, scratch, rows, frames, bins, rate, dtype, pl, stream);
    else pl_launch_bpt<double>(spec, out, scratch, rows, frames, bins, rate, dtype, pl, stream);
}

void phase_vocoder_locked_plan_info(int64_t rows, int64_t frames, int64_t bins, double rate, int dtype, int64_t segments,
                                    int64_t *out_frames, int64_t *threads, int64_t *bins_per_thread, int64_t *lds_bytes,
                                    int64_t *segments_out, int64_t *seg_frames, int64_t *launches, int64_t *workgroups,
                                    int64_t *scratch_bytes)
{
    const PlPlan pl = pl_plan("phase_vocoder_locked_plan_info", rows, frames, bins, rate, dtype, segments);
    *out_frames = pl.Fo;
    *threads = pl.threads;
    *bins_per_thread = pl.bpt;
    *lds_bytes = pl.lds_bytes;
    *segments_out = pl.segments;
    *seg_frames = pl.seg_frames;
    *launches = pl.launches;
    *workgroups = pl.workgroups;
    *scratch_bytes = pl.scratch_bytes;
}

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
