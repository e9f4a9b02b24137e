// stft.hip -- the short-time Fourier transform (tfx_stft_forward): one launch that reads the signal once and writes only the
// result, [rows, frames, n_fft / 2 + 1] complex values, magnitudes or powers.
//
// A workgroup owns G consecutive frames of one row.  It stages, once in LDS, the span of the row those frames cover,
// (G - 1) hop + n_fft samples (frame by frame when hop > n_fft, so the image never exceeds G n_fft samples); the centre padding is
// part of that load's addressing (reflected or zero indices), so no padded copy, frame matrix or complex intermediate exists in
// global memory.  TPF = n_fft / 32 threads transform one frame on their own: the windowed samples s = fl(w x) are read as the
// M = n_fft / 2 complex values z[n] = s[2n] + i s[2n+1], transformed by a Stockham autosort FFT of radices (8 | 4 | 2,) 16, 16
// (M = 128: 8, 16) and turned into the real input's spectrum by the post-twiddle
//     X[k] = (Z[k] + conj Z[M-k]) / 2  +  W_n^k (-i) (Z[k] - conj Z[M-k]) / 2,     X[0], X[M] = Re Z[0] +- Im Z[0].
// No two frames share a transform, so a frame's bits depend on its own n_fft samples and the window alone -- not on its index,
// its row, the hop, its place in the workgroup or the batch -- and a non-finite sample reaches exactly the frames that hold it.
//
// Stage (radix r, stride s; s is the product of the earlier radices, m = M / (r s)): butterfly b = q + s p (q < s, p < m) takes
// a_j = x[b + (M / r) j], forms the r-point DFT A_k and stores y[q + s (r p + k)] = A_k W_M^(s p k).  A thread holds the sixteen
// values t + TPF e (e < 16) of its frame: those are the inputs of its 16 / r butterflies in EVERY stage, and the outputs of the
// last one, so each exchange is "store scattered, barrier, load own".  W_M^j (j < M) and W_n^k (k < M) are tables built on the
// host in double and rounded once (plan cache, keyed by n_fft and the element size); W_M is copied to LDS and W_n takes its place
// there before the last stage, which multiplies by no twiddle.
// LDS: [W_M: M complex | window: n_fft reals | staged samples, then -- behind a barrier -- the G frames' exchange buffers of
// M + M / 16 complex each (one pad per 16 keeps the stride-16 stores off one bank)].
// The stages, the exchange and the tables are stft_frame.h's, shared with the inverse (istft.hip).
#include "stft_frame.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <cmath>

namespace tfx {

PlanCache<DeviceBuffer, 2> g_stft_tables(16, "stft_forward");

namespace {

constexpr int STFT_POWER_COMPLEX = 0, STFT_POWER_MAGNITUDE = 1, STFT_POWER_SQUARE = 2;

template <typename R> struct StftArgs {
    const R *x;             // [rows, T]
    const R *win;           // [win_len] or null (ones)
    const cx<R> *tab;       // [W_M^j, j < M | W_n^k, k < M]
    void *out;              // [rows, frames, M + 1] complex or real
    int64_t T, frames, groups_per_row, hop, pad;
    int hop_lds;            // min(hop, n_fft): distance of two frames in the staged image
    int win_len, win_left, reflect, power, normalized;
    R scale;                // n_fft^-1/2
};

template <int M> constexpr int stft_log2n() { return M == 128 ? 8 : M == 256 ? 9 : M == 512 ? 10 : M == 1024 ? 11 : 12; }

template <typename R, int M, int THREADS>
__global__ __launch_bounds__(THREADS, sizeof(R) == 4 ? 2 : 1) void stft_kernel(const StftArgs<R> p)
{
    constexpr int N = 2 * M, TPF = M / 16, G = THREADS / TPF, FS = M + M / 16, LOGN = stft_log2n<M>(), BATCH = 8;
    constexpr int NP = (M + THREADS - 1) / THREADS, NW = (N + THREADS - 1) / THREADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char stft_smem[];
    cx<R> *tw = (cx<R> *)stft_smem;
    R *win = (R *)(tw + M);
    R *stage = win + N;
    cx<R> *work = (cx<R> *)stage;                                       // reuses the staged samples' bytes, behind a barrier
    const int tid = (int)threadIdx.x;
    const int64_t grp = blockIdx.x, row = grp / p.groups_per_row, f0 = (grp - row * p.groups_per_row) * G;

    // Every global load of the workgroup is issued here, before the first one is used: both tables, the window and the samples
    // (in batches).  A workgroup has two or three neighbours on its CU and a few microseconds to live; a load it waits for in the
    // middle -- one per loop iteration, or the post-twiddles in the output loop -- costs it a full memory latency each time.
    R tvx[NP], tvy[NP], pvx[NP], pvy[NP], wv[NW];                        // scalars: arrays of cx<double> end up in scratch
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int i = u * THREADS + tid;
        tvx[u] = tvy[u] = pvx[u] = pvy[u] = (R)0;
        if (M % THREADS == 0 || i < M) {
            const cx<R> a = p.tab[i], b = p.tab[M + i];
            tvx[u] = a.x; tvy[u] = a.y; pvx[u] = b.x; pvy[u] = b.y;
        }
    }
#pragma unroll
    for (int u = 0; u < NW; ++u) {
        const int j = u * THREADS + tid - p.win_left;
        wv[u] = (R)0;
        if (j >= 0 && j < p.win_len) wv[u] = p.win ? p.win[j] : (R)1;
    }
    {
        const R *xr = p.x + row * p.T;
        const int64_t base = f0 * p.hop - p.pad;
        const bool apart = p.hop > N;                                   // frames that do not touch are staged one by one
        const int span = (G - 1) * p.hop_lds + N;
        for (int e0 = tid; e0 < span; e0 += BATCH * THREADS) {
            R val[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int e = e0 + u * THREADS;
                int64_t i = apart ? base + (int64_t)(e >> LOGN) * p.hop + (e & (N - 1)) : base + e;
                if (p.reflect) i = i < 0 ? -i : (i >= p.T ? 2 * (p.T - 1) - i : i);
                val[u] = (e < span && i >= 0 && i < p.T) ? xr[i] : (R)0;     // beyond one reflection: frames past the last one only
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                if (e0 + u * THREADS < span) stage[e0 + u * THREADS] = val[u];
        }
    }
#pragma unroll
    for (int u = 0; u < NP; ++u)
        if (M % THREADS == 0 || u * THREADS + tid < M) tw[u * THREADS + tid] = mk<R>(tvx[u], tvy[u]);
#pragma unroll
    for (int u = 0; u < NW; ++u)
        if (N % THREADS == 0 || u * THREADS + tid < N) win[u * THREADS + tid] = wv[u];
    __syncthreads();

    const int g = tid / TPF, t = tid - g * TPF;
    cx<R> v[16];
    {
        const R *s = stage + g * p.hop_lds;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = 2 * (t + TPF * e);
            v[e] = mk<R>(mul_rn(s[n], win[n]), mul_rn(s[n + 1], win[n + 1]));
        }
    }
    __syncthreads();
    stft_transform<R, M>(v, work + g * FS, tw, t, [&] {
#pragma unroll
        for (int u = 0; u < NP; ++u)
            if (M % THREADS == 0 || u * THREADS + tid < M) tw[u * THREADS + tid] = mk<R>(pvx[u], pvy[u]);
    });
    __syncthreads();

    const int64_t left = p.frames - f0;
    const int total = (int)(left < G ? left : G) * (M + 1);
    const cx<R> *post = tw;                                             // W_n^k by now
    const int64_t o0 = (row * p.frames + f0) * (M + 1);
    for (int idx = tid; idx < total; idx += THREADS) {
        const int f = idx / (M + 1), k = idx - f * (M + 1);
        const cx<R> *wk = work + f * FS;
        cx<R> X;
        if (k == 0 || k == M) {
            const cx<R> z = wk[0];
            X = mk<R>(k == 0 ? z.x + z.y : z.x - z.y, (R)0);
        } else {
            const cx<R> a = wk[stft_at(k)], bz = wk[stft_at(M - k)];
            const cx<R> ev = mk<R>((a.x + bz.x) * (R)0.5, (a.y - bz.y) * (R)0.5);          // (A + conj B) / 2
            const cx<R> od = mk<R>((a.y + bz.y) * (R)0.5, (bz.x - a.x) * (R)0.5);          // -i (A - conj B) / 2
            X = cadd(ev, cmul(post[k], od));
        }
        if (p.normalized) X = mk<R>(X.x * p.scale, X.y * p.scale);
        if (p.power == STFT_POWER_COMPLEX) ((cx<R> *)p.out)[o0 + idx] = X;
        else {
            const R pw = X.x * X.x + X.y * X.y;
            ((R *)p.out)[o0 + idx] = p.power == STFT_POWER_MAGNITUDE ? (R)sqrt(pw) : pw;
        }
    }
}

struct StftPlan {
    int route = 0;          // 1: the kernel above, 0: torch.stft (the caller's business)
    int threads = 0;
    int64_t frames = 0, G = 0, tpf = 0, lds = 0, groups_per_row = 0, workgroups = 0;
};

// every check on the sizes, and the geometry; pad is the samples added at each end (n_fft / 2 when centred)
StftPlan stft_plan(const char *what, int64_t n_fft, int64_t hop, int64_t win_length, int64_t T, int64_t rows, int dtype, int64_t pad,
                   int pad_mode, int onesided)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: dtype must be TFX_F32 or TFX_F64", what);
    TFX_CHECK(n_fft >= 1 && n_fft <= (int64_t)1 << 30, "%s: n_fft %lld out of range", what, (long long)n_fft);
    TFX_CHECK(hop >= 1, "%s: hop %lld must be at least 1", what, (long long)hop);
    TFX_CHECK(win_length >= 1 && win_length <= n_fft, "%s: win_length %lld must be in [1, n_fft]", what, (long long)win_length);
    TFX_CHECK(rows >= 0 && T >= 1 && T <= (int64_t)1 << 40, "%s: bad shape (rows %lld, T %lld)", what, (long long)rows, (long long)T);
    TFX_CHECK(pad >= 0 && pad <= n_fft, "%s: pad %lld must be in [0, n_fft]", what, (long long)pad);
    TFX_CHECK(pad_mode >= TFX_STFT_PAD_CONSTANT && pad_mode <= TFX_STFT_PAD_CIRCULAR, "%s: unknown pad_mode %d", what, pad_mode);
    TFX_CHECK(pad == 0 || pad_mode == TFX_STFT_PAD_CONSTANT || pad_mode == TFX_STFT_PAD_REPLICATE || pad < T || (pad_mode == TFX_STFT_PAD_CIRCULAR && pad <= T),
              "%s: padding %lld does not fit a row of %lld samples", what, (long long)pad, (long long)T);
    TFX_CHECK(T + 2 * pad >= n_fft, "%s: %lld samples (with padding) are fewer than n_fft %lld", what, (long long)(T + 2 * pad),
              (long long)n_fft);
    StftPlan pl;
    pl.frames = 1 + (T + 2 * pad - n_fft) / hop;
    const bool size_ok = n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096;
    if (!size_ok || !onesided || (pad > 0 && pad_mode != TFX_STFT_PAD_CONSTANT && pad_mode != TFX_STFT_PAD_REFLECT)) return pl;
    const int64_t esz = dtype == TFX_F32 ? 4 : 8;
    pl.route = 1;
    pl.threads = dtype == TFX_F32 ? 256 : 128;
    pl.tpf = n_fft / 32;
    pl.G = pl.threads / pl.tpf;
    pl.groups_per_row = ceil_div(pl.frames, pl.G);
    pl.workgroups = rows * pl.groups_per_row;
    TFX_CHECK(pl.workgroups <= 0x7fffffffLL, "%s: %lld workgroups exceed the grid", what, (long long)pl.workgroups);
    const int64_t M = n_fft / 2, span = (pl.G - 1) * (hop < n_fft ? hop : n_fft) + n_fft, work = pl.G * (M + M / 16) * 2;
    pl.lds = esz * (2 * M + n_fft + (span > work ? span : work));
    return pl;
}

template <typename R, int M, int THREADS> void stft_launch_m(const StftArgs<R> &p, const StftPlan &pl, hipStream_t stream)
{
    static size_t attr[TFX_MAX_DEVICES] = {};
    size_t &have = attr[current_device()];
    if ((size_t)pl.lds > have) {
        TFX_HIP(hipFuncSetAttribute((const void *)stft_kernel<R, M, THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
        have = (size_t)pl.lds;
    }
    ProfScope ps("stft_kernel", stream);
    hipLaunchKernelGGL((stft_kernel<R, M, THREADS>), dim3((unsigned)pl.workgroups), dim3(THREADS), (size_t)pl.lds, stream, p);
    TFX_HIP(hipGetLastError());
}

template <typename R, int THREADS>
void stft_launch(const void *x, const void *window, void *out, int64_t T, int64_t n_fft, int64_t hop, int64_t win_length, int64_t pad,
                 int pad_mode, int power, int normalized, const StftPlan &pl, hipStream_t stream)
{
    const std::shared_ptr<DeviceBuffer> tab = stft_tables<R>(n_fft, stream);
    StftArgs<R> p{};
    p.x = (const R *)x; p.win = (const R *)window; p.tab = (const cx<R> *)tab->p; p.out = out;
    p.T = T; p.frames = pl.frames; p.groups_per_row = pl.groups_per_row; p.hop = hop; p.pad = pad;
    p.hop_lds = (int)(hop < n_fft ? hop : n_fft);
    p.win_len = (int)win_length; p.win_left = (int)((n_fft - win_length) / 2);
    p.reflect = pad > 0 && pad_mode == TFX_STFT_PAD_REFLECT; p.power = power; p.normalized = normalized;
    p.scale = (R)(1.0 / std::sqrt((double)n_fft));
    switch (n_fft) {
    case 256: stft_launch_m<R, 128, THREADS>(p, pl, stream); break;
    case 512: stft_launch_m<R, 256, THREADS>(p, pl, stream); break;
    case 1024: stft_launch_m<R, 512, THREADS>(p, pl, stream); break;
    case 2048: stft_launch_m<R, 1024, THREADS>(p, pl, stream); break;
    default: stft_launch_m<R, 2048, THREADS>(p, pl, stream); break;
    }
}

}  // namespace

void stft_clear() { g_stft_tables.clear(); }

void stft_forward(const void *x, const void *window, void *out, int dtype, int64_t rows, int64_t T, int64_t n_fft, int64_t hop,
                  int64_t win_length, int64_t pad, int pad_mode, int power, int normalized, hipStream_t stream)
{
    const char *what = "stft_forward";
    TFX_CHECK(power >= STFT_POWER_COMPLEX && power <= STFT_POWER_SQUARE, "%s: power must be 0 (complex), 1 or 2", what);
    const StftPlan pl = stft_plan(what, n_fft, hop, win_length, T, rows, dtype, pad, pad_mode, 1);
    TFX_CHECK(pl.route == 1, "%s: n_fft %lld / pad_mode %d is not on the LDS route (tfx_stft_plan_info)", what, (long long)n_fft, pad_mode);
    TFX_CHECK(x && out, "%s: null pointer", what);
    if (rows == 0) return;
    if (dtype == TFX_F32) stft_launch<float, 256>(x, window, out, T, n_fft, hop, win_length, pad, pad_mode, power, normalized, pl, stream);
    else stft_launch<double, 128>(x, window, out, T, n_fft, hop, win_length, pad, pad_mode, power, normalized, pl, stream);
}

void stft_plan_info(int64_t n_fft, int64_t hop, int64_t win_length, int64_t T, int64_t rows, int dtype, int center, int pad_mode,
                    int onesided, int *route, int64_t *frames, int64_t *frames_per_workgroup, int64_t *threads_per_frame,
                    int64_t *lds_bytes, int64_t *workgroups)
{
    TFX_CHECK(n_fft >= 1, "stft_plan_info: n_fft %lld out of range", (long long)n_fft);
    const StftPlan pl = stft_plan("stft_plan_info", n_fft, hop, win_length, T, rows, dtype, center ? n_fft / 2 : 0, pad_mode, onesided);
    *route = pl.route;
    *frames = pl.frames;
    *frames_per_workgroup = pl.G;
    *threads_per_frame = pl.tpf;
    *lds_bytes = pl.lds;
    *workgroups = pl.workgroups;
}

}  // namespace tfx
