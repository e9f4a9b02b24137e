// istft.hip -- the inverse short-time Fourier transform (tfx_istft_forward, torch.istft's onesided semantics): one launch that
// reads the spectrum [rows, frames, n_fft / 2 + 1] in place and writes only the signal [rows, length].  No frame matrix, no
// envelope array and no real intermediate exist in global memory, and no value crosses between workgroups.
//
// A workgroup owns a tile of `tile` consecutive output samples of one row: thread tid owns the positions tid + THREADS u
// (u < tile / THREADS) and keeps their sums num[t] = sum_f fl(w[t - f hop] s_f[t - f hop]) in registers.  It runs over the frames
// that cover the tile in ascending order, G = THREADS / TPF at a time (TPF = n_fft / 32 threads per frame, the forward kernel's
// geometry).  For a frame its threads load the bins, form (pre-twiddle, the inverse of the forward post-twiddle)
//     Z[k] = (X[k] + conj X[M-k]) + i conj(W_n^k) (X[k] - conj X[M-k]),     Z[0] = (Re X[0] + Re X[M]) + i (Re X[0] - Re X[M]),
// and run the FORWARD M-point transform of stft_frame.h on conj Z: conj DFT(conj Z) is the inverse transform, the two sign flips
// are exact, and the result z[n] = s[2n] + i s[2n+1] lies in the frame's exchange buffer.  The imaginary parts of X[0] and X[M]
// are never read.  Then every thread walks its own positions over the batch's frames g = 0 ... G-1 and adds fl(w s) where the
// frame covers the position: ascending frame order per sample, whatever the tile, the batch or the frame's place in it.  A frame
// that straddles two tiles is transformed by both, to the same bits (its transform depends on the frame alone).  After the last
// frame the envelope env[t] = sum_f fl(w[t - f hop]^2) is summed in the same order from the window in LDS, the thread divides,
// stores 1 to the launch's flag where !(|env| > 1e-11) (a plain store: every writer stores the same value) and writes its
// positions, which are consecutive across the threads.  Positions past the last frame read 0.
// LDS: [W_M: M complex | window: n_fft reals | the G frames' exchange buffers of M + M / 16 complex each].
#include "stft_frame.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <cmath>

namespace tfx {

namespace {

template <typename R> struct IstftArgs {
    const cx<R> *spec;      // [rows, frames, M + 1]
    const R *win;           // [win_len] or null (ones)
    const cx<R> *tab;       // [W_M^j, j < M | W_n^k, k < M]
    R *out;                 // [rows, length]
    int *flag;              // set to 1 where the envelope is (nearly) zero
    int64_t frames, tiles_per_row, length, valid, pad;      // valid: outputs below it lie under a frame
    int hop, tile, win_len, win_left;
    R scale;                // 1 / n_fft, or n_fft^-1/2
};

// most output samples a thread owns, one register (pair) each: what two float32 workgroups per CU (256 registers a thread) leave
// beside a transform, and what keeps the float64 kernels (one workgroup per CU) within the 256 architectural registers
constexpr int istft_acc_max(int) { return 32; }
constexpr int istft_threads(int esz) { return esz == 4 ? 256 : 128; }
constexpr int64_t istft_tile_max(int64_t n_fft, int esz)
{
    const int64_t cap = (int64_t)istft_threads(esz) * istft_acc_max(esz);
    return 8 * n_fft < cap ? 8 * n_fft : cap;
}

template <typename R, int M, int THREADS>
__global__ __launch_bounds__(THREADS, sizeof(R) == 4 ? 2 : 1) void istft_kernel(const IstftArgs<R> p)
{
    constexpr int N = 2 * M, TPF = M / 16, G = THREADS / TPF, FS = M + M / 16;
    constexpr int ACC = (int)(istft_tile_max(N, sizeof(R)) / THREADS);
    constexpr int NP = (M + THREADS - 1) / THREADS, NW = (N + THREADS - 1) / THREADS;
    constexpr bool PRE_IN_REGS = sizeof(R) == 4;                        // float64 has no registers to spare for them
    extern __shared__ __attribute__((aligned(16))) unsigned char istft_smem[];
    cx<R> *tw = (cx<R> *)istft_smem;
    R *win = (R *)(tw + M);
    cx<R> *work = (cx<R> *)(win + N);
    const int tid = (int)threadIdx.x, g = tid / TPF, t = tid - g * TPF;
    const int64_t blk = blockIdx.x, row = blk / p.tiles_per_row, j0 = (blk - row * p.tiles_per_row) * p.tile;
    const int hop = p.hop;

    // the frames that cover the tile's positions [t0, t1) of the padded time axis
    const int64_t t0 = j0 + p.pad, jend = j0 + p.tile < p.length ? j0 + p.tile : p.length, t1 = jend + p.pad;
    const int64_t f_lo = t0 - N + 1 <= 0 ? 0 : (t0 - N + hop) / hop;
    const int64_t f_last = (t1 - 1) / hop, f_hi = f_last < p.frames - 1 ? f_last : p.frames - 1;

#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int i = u * THREADS + tid;
        if (M % THREADS == 0 || i < M) tw[i] = p.tab[i];
    }
#pragma unroll
    for (int u = 0; u < NW; ++u) {
        const int i = u * THREADS + tid, j = i - p.win_left;
        if (N % THREADS == 0 || i < N) win[i] = (j >= 0 && j < p.win_len) ? (p.win ? p.win[j] : (R)1) : (R)0;
    }
    R prx[PRE_IN_REGS ? 16 : 1], pry[PRE_IN_REGS ? 16 : 1];               // W_n^k of the thread's own sixteen bins
    if constexpr (PRE_IN_REGS) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const cx<R> w = p.tab[M + t + TPF * e];
            prx[e] = w.x; pry[e] = w.y;
        }
    }
    R num[ACC];
#pragma unroll
    for (int u = 0; u < ACC; ++u) num[u] = (R)0;
    __syncthreads();

    // everything below is relative to the tile and to frame f_lo, in 32 bits
    const int nfr = f_hi < f_lo ? 0 : (int)(f_hi - f_lo + 1);           // <= (tile + n_fft) / hop + 1
    const int d0 = nfr ? (int)(t0 - f_lo * hop) : 0;                    // >= 0: frame f_lo starts at or before the tile
    const cx<R> *xb = p.spec + (row * p.frames + f_lo) * (M + 1);       // uniform; the threads add 32-bit offsets: thirty-two
    const unsigned lo = (unsigned)(g * (M + 1) + t), hi = (unsigned)(g * (M + 1) + M - t);      // 64-bit addresses each would not fit
    for (int i0 = 0; i0 < nfr; i0 += G, xb += G * (M + 1)) {
        const int nb = nfr - i0 < G ? nfr - i0 : G;
        cx<R> v[16];
        if (g < nb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = t + TPF * e;
                const cx<R> a = xb[lo + (unsigned)(TPF * e)], b = xb[hi - (unsigned)(TPF * e)];
                if (k == 0) {                                           // e == 0 only; the imaginary parts are not read
                    v[e] = mk<R>(a.x + b.x, -(a.x - b.x));
                } else {
                    R wx, wy;
                    if constexpr (PRE_IN_REGS) { wx = prx[e]; wy = pry[e]; }
                    else { const cx<R> w = (p.tab + M)[(unsigned)t + (unsigned)(TPF * e)]; wx = w.x; wy = w.y; }        // uniform base again
                    const R ex = a.x + b.x, ey = a.y - b.y, dx = a.x - b.x, dy = a.y + b.y;        // X + conj X', X - conj X'
                    const R ox = wx * dx + wy * dy, oy = wx * dy - wy * dx;                          // conj(W) (X - conj X')
                    v[e] = mk<R>(ex - oy, -(ey + ox));                                              // conj(E + i O)
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = mk<R>((R)0, (R)0);
        }
        stft_transform<R, M>(v, work + g * FS, tw, t, [] {});
        __syncthreads();
        const R *wr = (const R *)work;
        int base = i0 * hop - d0;                                       // the frame's first sample, relative to the tile
        for (int g2 = 0; g2 < nb; ++g2, base += hop) {
            const R *fr = wr + 2 * g2 * FS;
#pragma unroll
            for (int u = 0; u < ACC; ++u) {
                const int n = tid + THREADS * u - base;
                if ((unsigned)n < (unsigned)N) {             // (positions past the tile gather too; they are not stored)
                    const R c = fr[2 * stft_at(n >> 1) + (n & 1)];
                    const R s = ((n & 1) ? -c : c) * p.scale;           // conj: s[2n+1] = -Im
                    num[u] += mul_rn(win[n], s);
                }
            }
        }
        __syncthreads();
    }

    const int64_t nstore64 = p.length - j0, nvalid64 = p.valid - j0;
    const int nstore = (int)(nstore64 < p.tile ? nstore64 : p.tile);
    const int nvalid = nvalid64 <= 0 ? 0 : (int)(nvalid64 < p.tile ? nvalid64 : p.tile);
    R *yr = p.out + row * p.length + j0;
#pragma unroll
    for (int u = 0; u < ACC; ++u) {
        const int r = tid + THREADS * u;
        if (r < nstore) {
            R y = (R)0;
            if (r < nvalid) {                                           // under a frame, so nfr >= 1
                const unsigned d = (unsigned)(d0 + r);                  // distance from frame f_lo's first sample
                unsigned i_hi = d / (unsigned)hop;
                const unsigned i_lo = d < (unsigned)N ? 0u : (d - (unsigned)N + (unsigned)hop) / (unsigned)hop;
                if (i_hi > (unsigned)(nfr - 1)) i_hi = (unsigned)(nfr - 1);
                R env = (R)0;
                for (unsigned i = i_lo; i <= i_hi; ++i) {
                    const R w = win[d - i * (unsigned)hop];
                    env += mul_rn(w, w);
                }
                if (!(fabs(env) > (R)1e-11)) *p.flag = 1;
                y = num[u] / env;
            }
            yr[(unsigned)r] = y;
        }
    }
}

struct IstftPlan {
    int route = 0;          // 1: the kernel above, 0: torch.istft (the caller's business)
    int threads = 0;
    int64_t length = 0, valid = 0, tile = 0, G = 0, tpf = 0, lds = 0, tiles_per_row = 0, workgroups = 0;
    double redundant = 0;   // share of the transforms that a neighbouring tile runs too
};

// every check on the sizes, and the geometry; pad is what is cut from each end (n_fft / 2 when centred), length < 0 the natural
// length (frames - 1) hop + n_fft - 2 pad
IstftPlan istft_plan(const char *what, int64_t n_fft, int64_t hop, int64_t win_length, int64_t frames, int64_t rows, int dtype,
                     int64_t pad, int64_t length, int onesided)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: dtype must be TFX_F32 or TFX_F64", what);
    TFX_CHECK(n_fft >= 1 && n_fft <= (int64_t)1 << 30, "%s: n_fft %lld out of range", what, (long long)n_fft);
    TFX_CHECK(win_length >= 1 && win_length <= n_fft, "%s: win_length %lld must be in [1, n_fft]", what, (long long)win_length);
    TFX_CHECK(hop >= 1 && hop <= win_length, "%s: hop %lld must be in [1, win_length]", what, (long long)hop);
    TFX_CHECK(rows >= 0 && frames >= 1 && frames <= (int64_t)1 << 40, "%s: bad shape (rows %lld, frames %lld)", what, (long long)rows,
              (long long)frames);
    TFX_CHECK(pad >= 0 && pad <= n_fft, "%s: pad %lld must be in [0, n_fft]", what, (long long)pad);
    const int64_t reach = (frames - 1) * hop + n_fft;                   // one past the last sample under a frame
    TFX_CHECK(length == -1 || (length >= 1 && length <= (int64_t)1 << 41), "%s: length %lld must be -1 (natural) or at least 1", what,
              (long long)length);
    IstftPlan pl;
    pl.length = length == -1 ? reach - 2 * pad : length;
    TFX_CHECK(pl.length >= 1, "%s: %lld frames leave no sample after %lld are cut from each end", what, (long long)frames, (long long)pad);
    pl.valid = pl.length < reach - pad ? pl.length : reach - pad;
    const bool size_ok = n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096;
    if (!size_ok || !onesided) return pl;
    const int esz = dtype == TFX_F32 ? 4 : 8;
    pl.route = 1;
    pl.threads = istft_threads(esz);
    pl.tpf = n_fft / 32;
    pl.G = pl.threads / pl.tpf;
    // A tile of `tile` samples transforms tile / hop frames of its own and the ceil(n_fft / hop) - 1 that reach in from the left:
    // 8 (n_fft - hop) samples hold that share near a ninth, 4 n_fft keep a tile from being all edge, and the accumulators
    // (istft_acc_max registers per thread) cap it.
    const int64_t want = ceil_div(8 * (n_fft - hop), pl.threads) * pl.threads;
    pl.tile = want > 4 * n_fft ? want : 4 * n_fft;
    if (pl.tile > istft_tile_max(n_fft, esz)) pl.tile = istft_tile_max(n_fft, esz);
    const int64_t extra = ceil_div(n_fft, hop) - 1;
    pl.redundant = (double)extra / ((double)pl.tile / (double)hop + (double)extra);
    pl.tiles_per_row = ceil_div(pl.length, pl.tile);
    pl.workgroups = rows * pl.tiles_per_row;
    TFX_CHECK(pl.workgroups <= 0x7fffffffLL, "%s: %lld workgroups exceed the grid", what, (long long)pl.workgroups);
    const int64_t M = n_fft / 2;
    pl.lds = (int64_t)esz * (2 * M + n_fft + pl.G * (M + M / 16) * 2);
    return pl;
}

template <typename R, int M, int THREADS> void istft_launch_m(const IstftArgs<R> &p, const IstftPlan &pl, hipStream_t stream)
{
    static size_t attr[TFX_MAX_DEVICES] = {};
    size_t &have = attr[current_device()];
    if ((size_t)pl.lds > have) {
        TFX_HIP(hipFuncSetAttribute((const void *)istft_kernel<R, M, THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
        have = (size_t)pl.lds;
    }
    ProfScope ps("istft_kernel", stream);
    hipLaunchKernelGGL((istft_kernel<R, M, THREADS>), dim3((unsigned)pl.workgroups), dim3(THREADS), (size_t)pl.lds, stream, p);
    TFX_HIP(hipGetLastError());
}

template <typename R>
void istft_launch(const void *spec, const void *window, void *out, int *flag, int64_t frames, int64_t n_fft, int64_t hop,
                  int64_t win_length, int64_t pad, int normalized, const IstftPlan &pl, hipStream_t stream)
{
    constexpr int THREADS = istft_threads(sizeof(R));
    const std::shared_ptr<DeviceBuffer> tab = stft_tables<R>(n_fft, stream);
    TFX_HIP(hipMemsetAsync(flag, 0, sizeof(int), stream));
    IstftArgs<R> p{};
    p.spec = (const cx<R> *)spec; p.win = (const R *)window; p.tab = (const cx<R> *)tab->p; p.out = (R *)out; p.flag = flag;
    p.frames = frames; p.tiles_per_row = pl.tiles_per_row; p.length = pl.length; p.valid = pl.valid; p.pad = pad;
    p.hop = (int)hop; p.tile = (int)pl.tile;
    p.win_len = (int)win_length; p.win_left = (int)((n_fft - win_length) / 2);
    p.scale = (R)(normalized ? 1.0 / std::sqrt((double)n_fft) : 1.0 / (double)n_fft);
    switch (n_fft) {
    case 256: istft_launch_m<R, 128, THREADS>(p, pl, stream); break;
    case 512: istft_launch_m<R, 256, THREADS>(p, pl, stream); break;
    case 1024: istft_launch_m<R, 512, THREADS>(p, pl, stream); break;
    case 2048: istft_launch_m<R, 1024, THREADS>(p, pl, stream); break;
    default: istft_launch_m<R, 2048, THREADS>(p, pl, stream); break;
    }
}

}  // namespace

void istft_forward(const void *spec, const void *window, void *out, int *flag, int dtype, int64_t rows, int64_t frames, int64_t n_fft,
                   int64_t hop, int64_t win_length, int64_t pad, int64_t length, int normalized, hipStream_t stream)
{
    const char *what = "istft_forward";
    const IstftPlan pl = istft_plan(what, n_fft, hop, win_length, frames, rows, dtype, pad, length, 1);
    TFX_CHECK(pl.route == 1, "%s: n_fft %lld is not on the LDS route (tfx_istft_plan_info)", what, (long long)n_fft);
    TFX_CHECK(spec && out && flag, "%s: null pointer", what);
    if (rows == 0) {
        TFX_HIP(hipMemsetAsync(flag, 0, sizeof(int), stream));
        return;
    }
    if (dtype == TFX_F32) istft_launch<float>(spec, window, out, flag, frames, n_fft, hop, win_length, pad, normalized, pl, stream);
    else istft_launch<double>(spec, window, out, flag, frames, n_fft, hop, win_length, pad, normalized, pl, stream);
}

void istft_plan_info(int64_t n_fft, int64_t hop, int64_t win_length, int64_t frames, int64_t rows, int dtype, int center, int64_t length,
                     int onesided, int *route, int64_t *out_length, int64_t *tile, int64_t *frames_per_batch, int64_t *threads_per_frame,
                     int64_t *lds_bytes, int64_t *workgroups, double *redundant_share)
{
    TFX_CHECK(n_fft >= 1, "istft_plan_info: n_fft %lld out of range", (long long)n_fft);
    const IstftPlan pl = istft_plan("istft_plan_info", n_fft, hop, win_length, frames, rows, dtype, center ? n_fft / 2 : 0, length, onesided);
    *route = pl.route;
    *out_length = pl.length;
    *tile = pl.tile;
    *frames_per_batch = pl.G;
    *threads_per_frame = pl.tpf;
    *lds_bytes = pl.lds;
    *workgroups = pl.workgroups;
    *redundant_share = pl.redundant;
}

}  // namespace tfx
