// yin.hip -- YIN pitch detection (tfx_yin_forward; de Cheveigne & Kawahara, JASA 2002, steps 2 to 5): one launch that reads the
// signal once and writes a frequency and an aperiodicity per frame (and, when asked, the normalised difference function).
//
// Definition, per frame starting at s = f hop - pad, in the signal's dtype R (lags 0 .. Lmax = tau_max + 1):
//     d(tau)  = sum_{j < W} (x[s + j] - x[s + j + tau])^2            every term is a square: nothing cancels
//     S(tau)  = sum_{k = 1 .. tau} d(k),   d'(0) = 1,   d'(tau) = tau d(tau) / S(tau)   (1 where S(tau) = 0)
//     tau     = the smallest lag in [tau_min, tau_max] with d' < threshold, advanced while d'(tau + 1) < d'(tau) (tau < tau_max);
//               with none, the first arg-min of d' over [tau_min, tau_max]
//     delta   = (a - c) / 2 (a - 2 b + c) for a, b, c = d'(tau - 1), d'(tau), d'(tau + 1) when a - 2 b + c > 0, b <= a, b <= c;
//               else 0;     f0 = fs / (tau + delta),     aperiodicity = b
//
// Work split.  A workgroup of 256 threads owns G consecutive frames of one row and stages their span, (G - 1) hop + W + Lmax
// samples, once in LDS; the centre padding is that load's addressing (reflected or zero indices), as in stft.hip.  The span is
// cut into blocks of B samples on the frame grid (B = gcd(W, hop) when hop < W, that is at least YIN_MIN_BLOCK and the plan's cost
// model favours it; else B = W, one block per frame, nothing shared; the choice reads W, hop, Lmax and the dtype alone).  A block's partial p_b(tau) = sum_{j in b} (x[j] - x[j + tau])^2 is computed once and
// used by every frame that holds the block: frame g is the ascending sum of its W / B partials.  A partial is the same number
// whichever frame reads it, so a frame's bits depend on its own samples and (W, hop, Lmax, threshold, fs) alone.
//
// Inner loop.  One work item is (block, tile of YIN_R = 9 neighbouring lags); a thread walks j through the block with the nine
// running sums and the nine samples x[j + tau0 .. j + tau0 + 8] in registers.  A step reads x[j] (the same address in every lane
// of the block: a broadcast) and one new sample for the sliding window, and does nine subtractions and nine fused multiply-adds.
// Neighbouring lanes own neighbouring tiles, so the window reads and the partial stores have a stride of nine words: odd, hence
// free of bank conflicts -- the reason the tile is 9 and not 8.  The j loop is unrolled nine times, which makes the window's
// rotation a renaming of registers.  The arithmetic is scalar fp32 (or fp64): this file is compiled without packed fp32
// instructions (Makefile).  Matrix instructions have no place here: (a - b)^2 as a product is the cancelling form.
//
// Epilogue.  A wave takes one frame at a time: each lane owns a run of `chunk` lags (odd, so the lanes' LDS strides are free of
// conflicts), sums the block partials into d, adds up its run, the runs' totals go through a wave scan, and the second pass
// over the run turns d into d' in LDS and notes the lane's first lag under the threshold and its least value.  Two wave
// reductions, the short walk and the parabola follow; lane 0 stores.  The order of every sum is fixed by the geometry.
// A frame whose W + Lmax samples hold a NaN or an Inf stores NaN in every output; the check reads the staged samples.
// LDS: [samples: span + YIN_R + 1 | partials: blocks x lags_padded | d': min(G, 4) x lags_padded], all of R.
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <cmath>
#include <numeric>

namespace tfx {

namespace {

constexpr int YIN_R = 9, YIN_THREADS = 256, YIN_WAVES = YIN_THREADS / 64, YIN_MAX_G = 32;
constexpr int64_t YIN_MIN_BLOCK = 16;              // a shared block shorter than this is all prologue (9 loads, 9 stores per item)
constexpr int64_t YIN_ITEM_STEPS = 12;             // what an item costs beside its B steps, in steps: fitted at 1024 / 512 / 160
constexpr int64_t YIN_LDS_SOFT = 32 * 1024;        // five workgroups per CU and more: preferred
constexpr int64_t YIN_LDS_HARD = 160 * 1024;       // what a CU has

template <typename R> struct YinArgs {
    const R *x;                 // [rows, T]
    R *f0, *aper, *cmndf;       // [rows, frames], [rows, frames], [rows, frames, Lmax + 1] or null
    int64_t T, frames, groups_per_row, hop, pad;
    int W, B, nb, fstep, bstep, G, Lmax, tiles, nlp, chunk, spanp, tau_min, tau_max, reflect;
    R fs, threshold;
};

__device__ __forceinline__ float yin_shfl_up(float v, int o) { return __shfl_up(v, o, 64); }
__device__ __forceinline__ double yin_shfl_up(double v, int o) { return __shfl_up(v, o, 64); }

template <typename R> __global__ __launch_bounds__(YIN_THREADS) void yin_kernel(const YinArgs<R> p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char yin_smem[];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t grp = blockIdx.x, row = grp / p.groups_per_row, f0 = (grp - row * p.groups_per_row) * p.G;
    const int64_t left = p.frames - f0;
    const int gused = (int)(left < p.G ? left : p.G);
    const int nblk = (gused - 1) * p.fstep + p.nb;                        // the blocks this workgroup's frames hold
    const int nblk_all = (p.G - 1) * p.fstep + p.nb;
    R *xs = (R *)yin_smem;
    R *part = xs + p.spanp;
    R *dbuf = part + (int64_t)nblk_all * p.nlp;

    {   // the span, every global load of the workgroup: four per thread in flight
        const R *xr = p.x + row * p.T;
        const int64_t base = f0 * p.hop - p.pad;
        const int span = (nblk - 1) * p.bstep + p.B + p.Lmax;
        for (int e0 = tid; e0 < p.spanp; e0 += 4 * YIN_THREADS) {
            R val[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + u * YIN_THREADS;
                int64_t i = base + e;
                if (p.reflect) i = i < 0 ? -i : (i >= p.T ? 2 * (p.T - 1) - i : i);
                val[u] = (e < span && i >= 0 && i < p.T) ? xr[i] : (R)0;  // past the span: the window's over-read, and frames that do not exist
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e0 + u * YIN_THREADS < p.spanp) xs[e0 + u * YIN_THREADS] = val[u];
        }
    }
    __syncthreads();

    // the sample x lag sweep: item = (block, lag tile); reads stay below block start + B + nlp <= spanp
    const int items = nblk * p.tiles;
    for (int it = tid; it < items; it += YIN_THREADS) {
        const int b = it / p.tiles, tile = it - b * p.tiles;
        const R *xb = xs + (int64_t)b * p.bstep, *xw = xb + tile * YIN_R;
        R w[YIN_R], acc[YIN_R];
#pragma unroll
        for (int r = 0; r < YIN_R; ++r) w[r] = xw[r], acc[r] = (R)0;
        int j = 0;
        for (; j + YIN_R <= p.B; j += YIN_R) {
#pragma unroll
            for (int u = 0; u < YIN_R; ++u) {
                const R a = xb[j + u];
#pragma unroll
                for (int r = 0; r < YIN_R; ++r) {
                    const R d = a - w[(r + u) % YIN_R];                   // lag tau0 + r at sample j + u
                    acc[r] = fma(d, d, acc[r]);
                }
                w[u] = xw[j + u + YIN_R];                                 // lag tau0 + 8 of the next sample
            }
        }
        for (; j < p.B; ++j) {                                            // B mod 9 samples: the same order, the window shifted by hand
            const R a = xb[j];
#pragma unroll
            for (int r = 0; r < YIN_R; ++r) {
                const R d = a - w[r];
                acc[r] = fma(d, d, acc[r]);
            }
#pragma unroll
            for (int r = 0; r + 1 < YIN_R; ++r) w[r] = w[r + 1];
            w[YIN_R - 1] = xw[j + YIN_R];
        }
        R *pp = part + (int64_t)b * p.nlp + tile * YIN_R;
#pragma unroll
        for (int r = 0; r < YIN_R; ++r) pp[r] = acc[r];
    }
    __syncthreads();

    // the frames: one per wave at a time; every wave makes the same number of rounds, so the barriers are uniform
    R *dw = dbuf + (int64_t)(p.G < YIN_WAVES ? (wave < p.G ? wave : 0) : wave) * p.nlp;
    const int lo = 1 + lane * p.chunk, hi = lo + p.chunk < p.Lmax + 1 ? lo + p.chunk : p.Lmax + 1;    // the lane's lags [lo, hi)
    for (int g0 = 0; g0 < gused; g0 += YIN_WAVES) {
        const int g = g0 + wave;
        const bool active = g < gused;
        R S = (R)0, best_v = (R)INFINITY;
        int cand = INT_MAX, best_i = p.tau_min;
        bool bad = false;
        if (active) {
            const R *xf = xs + (int64_t)g * p.hop;                        // fstep * bstep = hop on either route
            for (int e = lane; e < p.W + p.Lmax; e += 64) {
                const R v = xf[e];
                bad |= !(v - v == (R)0);
            }
            bad = __ballot(bad) != 0;
            const R *p0 = part + (int64_t)g * p.fstep * p.nlp;
            R tot = (R)0;
            for (int t = lo; t < hi; ++t) {
                R d = p0[t];
                for (int k = 1; k < p.nb; ++k) d += p0[(int64_t)k * p.nlp + t];
                dw[t] = d;
                tot += d;
            }
            R inc = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const R up = yin_shfl_up(inc, o);
                if (lane >= o) inc += up;
            }
            S = yin_shfl_up(inc, 1);                                      // the sum of the runs below the lane's
            if (lane == 0) S = (R)0;
            for (int t = lo; t < hi; ++t) {
                const R d = dw[t];
                S += d;
                const R v = S == (R)0 ? (R)1 : (R)t * d / S;
                dw[t] = v;
                if (t >= p.tau_min && t <= p.tau_max) {
                    if (v < p.threshold && cand == INT_MAX) cand = t;
                    if (v < best_v) best_v = v, best_i = t;
                }
            }
            if (lane == 0) dw[0] = (R)1;
        }
        __syncthreads();                                                  // d' of the frame is in LDS
        if (active) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const int oc = __shfl_xor(cand, o, 64), oi = __shfl_xor(best_i, o, 64);
                const R ov = __shfl_xor(best_v, o, 64);
                cand = oc < cand ? oc : cand;
                if (ov < best_v || (ov == best_v && oi < best_i)) best_v = ov, best_i = oi;
            }
            int tau = best_i;
            if (cand != INT_MAX) {
                tau = cand;
                while (tau < p.tau_max && dw[tau + 1] < dw[tau]) ++tau;
            }
            const R a = dw[tau - 1], b = dw[tau], c = dw[tau + 1];        // 0 <= tau - 1, tau + 1 <= Lmax
            const R den = a - (R)2 * b + c;
            R delta = (R)0;
            if (den > (R)0 && b <= a && b <= c) delta = (R)0.5 * (a - c) / den;
            const int64_t fo = row * p.frames + f0 + g;
            if (lane == 0) {
                p.f0[fo] = bad ? (R)NAN : p.fs / ((R)tau + delta);
                p.aper[fo] = bad ? (R)NAN : b;
            }
            if (p.cmndf) {
                R *o = p.cmndf + fo * (p.Lmax + 1);
                for (int t = lane; t <= p.Lmax; t += 64) o[t] = bad ? (R)NAN : dw[t];
            }
        }
        __syncthreads();                                                  // before the wave's buffer takes its next frame
    }
}

struct YinPlan {
    int64_t frames = 0, lags = 0, B = 0, nb = 0, fstep = 0, bstep = 0, G = 0, tiles = 0, nlp = 0, chunk = 0, spanp = 0, lds = 0,
            groups_per_row = 0, workgroups = 0;
};

// Every check on the sizes, and the geometry, in one place.  pad: the samples added at each end (frame_length / 2 when centred);
// block: 0 = the plan's choice, win_length = no sharing, gcd(win_length, hop) = shared blocks.
YinPlan yin_plan(const char *what, int64_t rows, int64_t T, int64_t frame_length, int64_t W, int64_t hop, int64_t tau_min,
                 int64_t tau_max, int dtype, int64_t pad, int pad_mode, int64_t block)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: dtype must be TFX_F32 or TFX_F64", what);
    const int64_t cap = dtype == TFX_F32 ? 8192 : 4096, esz = dtype == TFX_F32 ? 4 : 8;
    TFX_CHECK(frame_length >= 2 && frame_length <= cap, "%s: frame_length %lld is outside [2, %lld], what the kernel serves for this dtype", what,
              (long long)frame_length, (long long)cap);
    TFX_CHECK(W >= 1 && W <= frame_length, "%s: win_length %lld must be in [1, frame_length]", what, (long long)W);
    TFX_CHECK(hop >= 1 && hop <= (int64_t)1 << 30, "%s: hop_length %lld must be in [1, 2^30]", what, (long long)hop);
    TFX_CHECK(tau_min >= 1 && tau_min <= tau_max, "%s: lags [%lld, %lld]: fmax must give a lag of at least 1 that is no longer than fmin's", what,
              (long long)tau_min, (long long)tau_max);
    TFX_CHECK(W + tau_max + 1 <= frame_length, "%s: fmin needs lags up to %lld: win_length %lld + %lld exceed frame_length %lld", what,
              (long long)(tau_max + 1), (long long)W, (long long)(tau_max + 1), (long long)frame_length);
    TFX_CHECK(rows >= 0 && T >= 1 && T <= (int64_t)1 << 40, "%s: bad shape (rows %lld, T %lld)", what, (long long)rows, (long long)T);
    TFX_CHECK(pad >= 0 && pad <= frame_length, "%s: pad %lld must be in [0, frame_length]", what, (long long)pad);
    TFX_CHECK(pad_mode == TFX_STFT_PAD_CONSTANT || pad_mode == TFX_STFT_PAD_REFLECT, "%s: pad_mode must be constant or reflect, got %d", what,
              pad_mode);
    TFX_CHECK(pad == 0 || pad_mode == TFX_STFT_PAD_CONSTANT || pad < T, "%s: pad_mode reflect: padding %lld does not fit a row of %lld samples",
              what, (long long)pad, (long long)T);
    TFX_CHECK(T + 2 * pad >= frame_length, "%s: %lld samples (with padding) are fewer than frame_length %lld", what, (long long)(T + 2 * pad),
              (long long)frame_length);
    const int64_t gcd = std::gcd(W, hop);
    TFX_CHECK(block == 0 || block == W || (block == gcd && hop < W), "%s: block %lld must be 0, win_length or gcd(win_length, hop) with hop < win_length",
              what, (long long)block);

    YinPlan pl;
    pl.frames = 1 + (T + 2 * pad - frame_length) / hop;
    const int64_t Lmax = tau_max + 1;
    pl.lags = Lmax + 1;
    pl.tiles = ceil_div(pl.lags, YIN_R);
    pl.nlp = pl.tiles * YIN_R;
    pl.chunk = ceil_div(Lmax, 64) | 1;
    // One route (block B) under an LDS budget with at most gmax frames per workgroup: the G of the least cost per frame -- rounds
    // of 256 items, each B steps and YIN_ITEM_STEPS of prologue, partial stores and its share of the epilogue's block sums --
    // ties: the smaller G.  Returns the cost, or a negative number when not even G = 1 fits.
    const auto route = [&](int64_t B, int64_t budget, int64_t gmax, YinPlan &out) {
        const int64_t nb = W / B, fstep = B == W ? 1 : hop / B, bstep = B == W ? hop : B;
        double best = -1.0;
        for (int64_t G = 1; G <= gmax; ++G) {
            const int64_t nblk = (G - 1) * fstep + nb;
            const int64_t spanp = (nblk - 1) * bstep + B + Lmax + YIN_R + 1;
            const int64_t lds = esz * (spanp + nblk * pl.nlp + (G < YIN_WAVES ? G : YIN_WAVES) * pl.nlp);
            if (lds > budget) break;
            const double cost = (double)(ceil_div(nblk * pl.tiles, YIN_THREADS) * (B + YIN_ITEM_STEPS)) / (double)G;
            if (best < 0.0 || cost < best) {
                best = cost;
                out.B = B, out.nb = nb, out.fstep = fstep, out.bstep = bstep, out.G = G, out.spanp = spanp, out.lds = lds;
            }
        }
        return best;
    };
    // The block decides the order of a frame's sum, so it is chosen from (W, hop, Lmax, dtype) alone: both routes are weighed as
    // if the row had YIN_MAX_G frames and more.  G is not part of a frame's bits -- a partial is the same number in any workgroup
    // -- and is then chosen again among the G the row has frames for.
    const bool may_share = block ? block != W : (hop < W && gcd >= YIN_MIN_BLOCK), may_alone = block ? block == W : true;
    for (const int64_t budget : {YIN_LDS_SOFT, YIN_LDS_HARD}) {
        YinPlan shared = pl, alone = pl;
        const double cs = may_share ? route(gcd, budget, YIN_MAX_G, shared) : -1.0, ca = may_alone ? route(W, budget, YIN_MAX_G, alone) : -1.0;
        if (cs < 0.0 && ca < 0.0) continue;
        const int64_t B = cs >= 0.0 && (ca < 0.0 || cs <= ca) ? gcd : W;
        route(B, budget, pl.frames < YIN_MAX_G ? pl.frames : YIN_MAX_G, pl);
        break;
    }
    TFX_CHECK(pl.G >= 1, "%s: frame_length %lld does not fit the workgroup's memory", what, (long long)frame_length);
    pl.groups_per_row = ceil_div(pl.frames, pl.G);
    pl.workgroups = rows * pl.groups_per_row;
    TFX_CHECK(pl.workgroups <= 0x7fffffffLL, "%s: %lld workgroups exceed the grid", what, (long long)pl.workgroups);
    TFX_CHECK(rows == 0 || pl.frames * pl.lags <= INT64_MAX / 16 / rows, "%s: size overflows", what);
    return pl;
}

template <typename R>
void yin_launch(const void *x, void *f0, void *aper, void *cmndf, int64_t T, int64_t W, int64_t hop, int64_t tau_min, int64_t tau_max,
                double fs, double threshold, int64_t pad, int pad_mode, const YinPlan &pl, hipStream_t stream)
{
    YinArgs<R> p{};
    p.x = (const R *)x; p.f0 = (R *)f0; p.aper = (R *)aper; p.cmndf = (R *)cmndf;
    p.T = T; p.frames = pl.frames; p.groups_per_row = pl.groups_per_row; p.hop = hop; p.pad = pad;
    p.W = (int)W; p.B = (int)pl.B; p.nb = (int)pl.nb; p.fstep = (int)pl.fstep; p.bstep = (int)pl.bstep; p.G = (int)pl.G;
    p.Lmax = (int)(tau_max + 1); p.tiles = (int)pl.tiles; p.nlp = (int)pl.nlp; p.chunk = (int)pl.chunk; p.spanp = (int)pl.spanp;
    p.tau_min = (int)tau_min; p.tau_max = (int)tau_max;
    p.reflect = pad > 0 && pad_mode == TFX_STFT_PAD_REFLECT;
    p.fs = (R)fs; p.threshold = (R)threshold;
    static size_t attr[TFX_MAX_DEVICES][2] = {};
    size_t &have = attr[current_device()][sizeof(R) == 4 ? 0 : 1];
    if ((size_t)pl.lds > have) {
        TFX_HIP(hipFuncSetAttribute((const void *)yin_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
        have = (size_t)pl.lds;
    }
    ProfScope ps("yin_kernel", stream);
    hipLaunchKernelGGL((yin_kernel<R>), dim3((unsigned)pl.workgroups), dim3(YIN_THREADS), (size_t)pl.lds, stream, p);
    TFX_HIP(hipGetLastError());
}

}  // namespace

void yin_forward(const void *x, void *f0, void *aper, void *cmndf, int dtype, int64_t rows, int64_t T, double fs, int64_t frame_length,
                 int64_t win_length, int64_t hop, int64_t tau_min, int64_t tau_max, double threshold, int64_t pad, int pad_mode,
                 int64_t block, hipStream_t stream)
{
    const char *what = "yin_forward";
    TFX_CHECK(std::isfinite(fs) && fs > 0.0, "%s: fs must be a finite number > 0, got %g", what, fs);
    TFX_CHECK(std::isfinite(threshold), "%s: threshold must be finite, got %g", what, threshold);
    const YinPlan pl = yin_plan(what, rows, T, frame_length, win_length, hop, tau_min, tau_max, dtype, pad, pad_mode, block);
    if (rows == 0) return;
    TFX_CHECK(x && f0 && aper, "%s: null pointer", what);
    if (dtype == TFX_F32)
        yin_launch<float>(x, f0, aper, cmndf, T, win_length, hop, tau_min, tau_max, fs, threshold, pad, pad_mode, pl, stream);
    else
        yin_launch<double>(x, f0, aper, cmndf, T, win_length, hop, tau_min, tau_max, fs, threshold, pad, pad_mode, pl, stream);
}

void yin_plan_info(int64_t rows, int64_t T, int64_t frame_length, int64_t win_length, int64_t hop, int64_t tau_min, int64_t tau_max,
                   int dtype, int64_t pad, int pad_mode, int64_t block, int64_t *frames, int64_t *lags, int64_t *block_out,
                   int64_t *blocks_per_frame, int64_t *frames_per_workgroup, int64_t *lags_per_thread, int64_t *lds_bytes, int64_t *workgroups)
{
    const YinPlan pl = yin_plan("yin_plan_info", rows, T, frame_length, win_length, hop, tau_min, tau_max, dtype, pad, pad_mode, block);
    *frames = pl.frames;
    *lags = pl.lags;
    *block_out = pl.B;
    *blocks_per_frame = pl.nb;
    *frames_per_workgroup = pl.G;
    *lags_per_thread = YIN_R;
    *lds_bytes = pl.lds;
    *workgroups = pl.workgroups;
}

}  // namespace tfx
