// mel.hip -- the mel spectrogram (tfx_mel_forward): the STFT kernel's front, then the filterbank projection and the logarithm in
// the place of its output loop.  One launch reads the signal once and writes only [rows, frames, n_filters]; the power
// spectrogram [rows, frames, n_fft / 2 + 1] never exists in global memory.
//
// A workgroup owns G consecutive frames of one row, exactly as in stft.hip, and runs stft_frames (stft_frame.h): after it frame
// g's Z lies in its exchange buffer and W_n^k in the first table's place.  Then
//   1. power.  The frame's own TPF = M / 16 threads form P[k] = |X[k]| or |X[k]|^2 for k = t + TPF e (e < 16) and k = M with
//      stft_bin and stft_power -- the expressions of stft_kernel's output loop, so P has spectrogram's bits -- and hold them in 17
//      registers.  Behind a barrier (every Z of the frame has been read) they are written as M + 1 reals over the frame's own
//      exchange buffer, which holds 2 (M + M / 16).
//   2. projection.  The filterbank is a band table: filter m reads the bins lo_m ... lo_m + len_m - 1 with the weights
//      w[off_m ...] (first to last non-zero weight; len_m = 0 for an all-zero filter).  A fixed group of S lanes (a power of two
//      from the plan; G n_filters S fills the workgroup where it can) owns the output (frame f, filter m): lane j runs
//      acc = fma(w[i], P[lo + i], acc) over i = j, j + S, ... in ascending order and the S partial sums combine in a
//      __shfl_xor tree of fixed order (distance 1, 2, ... S / 2).  Lanes of a group read consecutive LDS words of w and of P;
//      the groups of one frame walk the same P.  No frame's sum sees another frame, the frame index, the row or the hop, so a
//      frame's bits depend on its n_fft samples, the window and the table alone.
//   3. store.  v < amin ? amin : v (a NaN passes), c log10 or ln, in registers; lane 0 of each group stores, and consecutive groups
//      hold consecutive filters of [rows, frames, n_filters]: the workgroup's outputs are one contiguous run.
// The band table has an LDS region of its own behind the exchange buffers: its global loads are issued with the tables' and the
// window's, before the samples', and it is stored with them in front of the first barrier (16 words per thread ride in registers
// through the sample loop; what a larger table has left follows in batches).  The alternative -- the 4 M reals of the two tables
// and the window, dead after step 1 -- would have to park the table in registers across the whole transform, up to 68 VGPRs per
// thread for float64 at n_fft 4096, or load it in the middle of the workgroup's life.
// No matrix instructions: a bin feeds at most two triangles, so the dense G x (M + 1) x n_filters product does about
// n_filters / 2 times the multiplications, on a matrix that does not fit LDS beside the frames, in a precision it does not need.
#include "stft_frame.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <cmath>
#include <cstring>

namespace tfx {

namespace {

PlanCache<DeviceBuffer, 1> g_mel_tables(32, "mel_forward");      // device copies of band tables, keyed by the table's bytes

constexpr int MEL_LOG_NONE = 0, MEL_LOG_LOG10 = 1, MEL_LOG_LN = 2;      // in the kernel: TFX_MEL_LOG_DB is log10 with c = 10 / 20
constexpr int MEL_EARLY = 16;                                            // table words a thread loads up front

template <typename R> struct MelArgs {
    StftArgs<R> st;             // st.out: [rows, frames, n_filters] of R
    const uint32_t *table;      // [lo | len | off: n_filters int32 each, padded to 8 bytes | weights: total of R]
    int table_words, table_at;  // 32-bit words of the table; its byte offset in LDS
    int n_filters, lanes_log2, log_mode;
    R amin, c;
};

__device__ __forceinline__ float fma_rn(float a, float b, float c) { return __fmaf_rn(a, b, c); }
__device__ __forceinline__ double fma_rn(double a, double b, double c) { return __fma_rn(a, b, c); }
__device__ __forceinline__ float log10_of(float v) { return log10f(v); }
__device__ __forceinline__ double log10_of(double v) { return log10(v); }
__device__ __forceinline__ float ln_of(float v) { return logf(v); }
__device__ __forceinline__ double ln_of(double v) { return log(v); }

template <typename R, int M, int THREADS>
__global__ __launch_bounds__(THREADS, sizeof(R) == 4 ? 2 : 1) void mel_kernel(const MelArgs<R> p)
{
    constexpr int TPF = M / 16, G = THREADS / TPF, FS = M + M / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char mel_smem[];
    const int tid = (int)threadIdx.x;
    const int64_t grp = blockIdx.x, row = grp / p.st.groups_per_row, f0 = (grp - row * p.st.groups_per_row) * G;
    uint32_t *mtab = (uint32_t *)(mel_smem + p.table_at);

    uint32_t mw[MEL_EARLY];
    auto load_batch = [&](int w0) {
#pragma unroll
        for (int u = 0; u < MEL_EARLY; ++u) {
            const int i = w0 + u * THREADS;
            mw[u] = i < p.table_words ? p.table[i] : 0u;
        }
    };
    auto store_batch = [&](int w0) {
#pragma unroll
        for (int u = 0; u < MEL_EARLY; ++u)
            if (w0 + u * THREADS < p.table_words) mtab[w0 + u * THREADS] = mw[u];
    };
    stft_frames<R, M, THREADS>(p.st, mel_smem, row, f0, [&] { load_batch(tid); }, [&] {
        store_batch(tid);
        for (int w0 = tid + MEL_EARLY * THREADS; w0 < p.table_words; w0 += MEL_EARLY * THREADS) {       // a table past the early words
            load_batch(w0);
            store_batch(w0);
        }
    });

    // 1. power: the frame's own threads, 17 values each, out of and back into the frame's exchange buffer
    const cx<R> *post = (const cx<R> *)mel_smem;                        // W_n^k by now
    cx<R> *work = (cx<R> *)mel_smem + M + M;                            // behind W and the window's n_fft reals
    {
        const int g = tid / TPF, t = tid - g * TPF;
        const cx<R> *wk = work + g * FS;
        R pv[17];
#pragma unroll
        for (int e = 0; e < 16; ++e) pv[e] = stft_power(stft_bin<R, M>(wk, post, t + TPF * e, p.st), p.st.power);
        pv[16] = stft_power(stft_bin<R, M>(wk, post, M, p.st), p.st.power);
        __syncthreads();
        R *P = (R *)wk;
#pragma unroll
        for (int e = 0; e < 16; ++e) P[t + TPF * e] = pv[e];
        if (t == 0) P[M] = pv[16];
    }
    __syncthreads();

    // 2. projection, 3. logarithm and store
    const int nf = p.n_filters, S = 1 << p.lanes_log2, j = tid & (S - 1);
    const int *lo = (const int *)mtab, *len = lo + nf, *off = len + nf;
    const R *w = (const R *)(mtab + ((3 * nf + 1) & ~1));
    const int64_t left = p.st.frames - f0;
    const int total = (int)(left < G ? left : G) * nf;
    R *out = (R *)p.st.out + (row * p.st.frames + f0) * nf;
    for (int o = tid >> p.lanes_log2; o < total; o += THREADS >> p.lanes_log2) {
        const int f = o / nf, m = o - f * nf, L = len[m];
        const R *P = (const R *)(work + f * FS) + lo[m], *wm = w + off[m];
        R acc = (R)0;
#pragma unroll 4                                                        // four steps' LDS reads in flight; the fma order stays
        for (int i = j; i < L; i += S) acc = fma_rn(wm[i], P[i], acc);
        for (int d = 1; d < S; d <<= 1) acc += __shfl_xor(acc, d);
        if (p.log_mode != MEL_LOG_NONE) {
            acc = acc < p.amin ? p.amin : acc;                          // not fmax: a NaN stays
            acc = p.log_mode == MEL_LOG_LN ? ln_of(acc) : p.c * log10_of(acc);
        }
        if (j == 0) out[o] = acc;
    }
}

struct MelPlan {
    StftPlan st;
    int route = 0;              // 1: the kernel above, 0: the composition (the caller's business)
    int lanes_log2 = 0;
    int64_t header_bytes = 0, table_bytes = 0, lds = 0;
};

// the STFT's checks and geometry, then the table's: n_filters filters whose bands hold total_band weights
MelPlan mel_plan(const char *what, int64_t n_fft, int64_t hop, int64_t win_length, int64_t T, int64_t rows, int dtype, int64_t pad,
                 int pad_mode, int64_t n_filters, int64_t total_band)
{
    MelPlan pl;
    pl.st = stft_plan(what, n_fft, hop, win_length, T, rows, dtype, pad, pad_mode, 1);
    TFX_CHECK(n_filters >= 1 && n_filters <= (int64_t)1 << 24, "%s: n_filters %lld out of range", what, (long long)n_filters);
    TFX_CHECK(total_band >= 0 && total_band <= n_filters * (n_fft / 2 + 1), "%s: total band length %lld does not fit %lld filters of %lld bins",
              what, (long long)total_band, (long long)n_filters, (long long)(n_fft / 2 + 1));
    if (!pl.st.route || n_filters > 256) return pl;
    const int64_t esz = dtype == TFX_F32 ? 4 : 8;
    pl.header_bytes = (3 * n_filters * 4 + 7) / 8 * 8;
    pl.table_bytes = pl.header_bytes + total_band * esz;
    pl.lds = pl.st.lds + pl.table_bytes;
    if (pl.table_bytes > 2 * n_fft * esz || pl.lds > 160 * 1024) return pl;     // the table: at most the 4 M reals of W and the window
    while (pl.lanes_log2 < 6 && (pl.st.G * n_filters << (pl.lanes_log2 + 1)) <= pl.st.threads) ++pl.lanes_log2;
    pl.route = 1;
    return pl;
}

template <typename R, int M, int THREADS> void mel_launch_m(const MelArgs<R> &p, const MelPlan &pl, hipStream_t stream)
{
    static size_t attr[TFX_MAX_DEVICES] = {};
    size_t &have = attr[current_device()];
    if ((size_t)pl.lds > have) {
        TFX_HIP(hipFuncSetAttribute((const void *)mel_kernel<R, M, THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
        have = (size_t)pl.lds;
    }
    ProfScope ps("mel_kernel", stream);
    hipLaunchKernelGGL((mel_kernel<R, M, THREADS>), dim3((unsigned)pl.st.workgroups), dim3(THREADS), (size_t)pl.lds, stream, p);
    TFX_HIP(hipGetLastError());
}

template <typename R, int THREADS>
void mel_launch(const void *x, const void *window, const void *table_host, void *out, int64_t T, int64_t n_fft, int64_t hop,
                int64_t win_length, int64_t pad, int pad_mode, int power, int normalized, int log_mode, double amin, int64_t n_filters,
                const MelPlan &pl, hipStream_t stream)
{
    const std::shared_ptr<DeviceBuffer> tab = stft_tables<R>(n_fft, stream);
    const int64_t tail[1] = {n_filters};
    const std::shared_ptr<DeviceBuffer> bands = g_mel_tables.get(table_host, (size_t)pl.table_bytes, tail, stream, [&] {
        return std::make_shared<DeviceBuffer>(table_host, (size_t)pl.table_bytes);
    });
    MelArgs<R> p{};
    p.st = stft_args<R>(x, window, (const cx<R> *)tab->p, out, T, n_fft, hop, win_length, pad, pad_mode, power, normalized, pl.st);
    p.table = (const uint32_t *)bands->p;
    p.table_words = (int)(pl.table_bytes / 4);
    p.table_at = (int)pl.st.lds;
    p.n_filters = (int)n_filters;
    p.lanes_log2 = pl.lanes_log2;
    p.log_mode = log_mode == TFX_MEL_LOG_NONE ? MEL_LOG_NONE : log_mode == TFX_MEL_LOG_LN ? MEL_LOG_LN : MEL_LOG_LOG10;
    p.amin = (R)amin;
    p.c = (R)(log_mode == TFX_MEL_LOG_DB ? (power == STFT_POWER_SQUARE ? 10.0 : 20.0) : 1.0);
    TFX_CHECK(log_mode == TFX_MEL_LOG_NONE || p.amin > (R)0, "mel_forward: amin %g is not positive in the signal's dtype", amin);
    switch (n_fft) {
    case 256: mel_launch_m<R, 128, THREADS>(p, pl, stream); break;
    case 512: mel_launch_m<R, 256, THREADS>(p, pl, stream); break;
    case 1024: mel_launch_m<R, 512, THREADS>(p, pl, stream); break;
    case 2048: mel_launch_m<R, 1024, THREADS>(p, pl, stream); break;
    default: mel_launch_m<R, 2048, THREADS>(p, pl, stream); break;
    }
}

}  // namespace

void mel_clear() { g_mel_tables.clear(); }

void mel_forward(const void *x, const void *window, const void *table_host, int64_t table_bytes, int64_t n_filters, void *out, int dtype,
                 int64_t rows, int64_t T, int64_t n_fft, int64_t hop, int64_t win_length, int64_t pad, int pad_mode, int power,
                 int normalized, int log_mode, double amin, hipStream_t stream)
{
    const char *what = "mel_forward";
    TFX_CHECK(power == STFT_POWER_MAGNITUDE || power == STFT_POWER_SQUARE, "%s: power must be 1 or 2", what);
    TFX_CHECK(log_mode >= TFX_MEL_LOG_NONE && log_mode <= TFX_MEL_LOG_LN, "%s: unknown log mode %d", what, log_mode);
    TFX_CHECK(log_mode == TFX_MEL_LOG_NONE || amin > 0.0, "%s: amin %g must be positive", what, amin);
    TFX_CHECK(table_host && n_filters >= 1 && n_filters <= 256 && table_bytes >= 12 * n_filters, "%s: bad band table (%lld filters, %lld bytes)",
              what, (long long)n_filters, (long long)table_bytes);
    // the table's own indices, before anything reads LDS by them: bands inside the bins, packed one after another
    const int *lo = (const int *)table_host, *len = lo + n_filters, *off = len + n_filters;
    int64_t total = 0;
    for (int64_t m = 0; m < n_filters; ++m) {
        TFX_CHECK(lo[m] >= 0 && len[m] >= 0 && (int64_t)lo[m] + len[m] <= n_fft / 2 + 1 && off[m] == total,
                  "%s: band %lld (first bin %d, length %d, offset %d) does not fit %lld bins packed at %lld", what, (long long)m, lo[m], len[m],
                  off[m], (long long)(n_fft / 2 + 1), (long long)total);
        total += len[m];
    }
    const MelPlan pl = mel_plan(what, n_fft, hop, win_length, T, rows, dtype, pad, pad_mode, n_filters, total);
    TFX_CHECK(pl.route == 1, "%s: n_fft %lld / pad_mode %d / %lld filters with %lld weights are not on the LDS route (tfx_mel_plan_info)", what,
              (long long)n_fft, pad_mode, (long long)n_filters, (long long)total);
    TFX_CHECK(table_bytes == pl.table_bytes, "%s: the band table has %lld bytes, its indices ask for %lld", what, (long long)table_bytes,
              (long long)pl.table_bytes);
    TFX_CHECK(x && out, "%s: null pointer", what);
    if (rows == 0) return;
    if (dtype == TFX_F32)
        mel_launch<float, 256>(x, window, table_host, out, T, n_fft, hop, win_length, pad, pad_mode, power, normalized, log_mode, amin, n_filters, pl, stream);
    else
        mel_launch<double, 128>(x, window, table_host, out, T, n_fft, hop, win_length, pad, pad_mode, power, normalized, log_mode, amin, n_filters, pl, stream);
}

void mel_plan_info(int64_t n_fft, int64_t hop, int64_t win_length, int64_t T, int64_t rows, int dtype, int center, int pad_mode,
                   int64_t n_filters, int64_t total_band, int *route, int64_t *frames, int64_t *frames_per_workgroup,
                   int64_t *lanes_per_filter, int64_t *lds_bytes, int64_t *workgroups)
{
    TFX_CHECK(n_fft >= 1, "mel_plan_info: n_fft %lld out of range", (long long)n_fft);
    const MelPlan pl = mel_plan("mel_plan_info", n_fft, hop, win_length, T, rows, dtype, center ? n_fft / 2 : 0, pad_mode, n_filters, total_band);
    *route = pl.route;
    *frames = pl.st.frames;
    *frames_per_workgroup = pl.route ? pl.st.G : 0;
    *lanes_per_filter = pl.route ? (int64_t)1 << pl.lanes_log2 : 0;
    *lds_bytes = pl.route ? pl.lds : 0;
    *workgroups = pl.route ? pl.st.workgroups : 0;
}

}  // namespace tfx
