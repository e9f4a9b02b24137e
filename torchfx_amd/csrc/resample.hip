// resample.hip -- polyphase rational resampling with scipy.signal.resample_poly's semantics (padtype "constant", zero outside
// [0, T)) in ONE launch per call.  With h the designed taps (already scaled by up), h_padded = [0 * n_pre_pad | h | 0 * n_post_pad]
// zero padded to Lp * up taps, hp[p][j] = h_padded[p + j*up] and n = (m + n_pre_remove) * down:
//   y[m] = sum_{j < Lp} hp[n mod up][j] * x[n / up - j]        m in [0, n_out), n_out = ceil(T * up / down)
// Every term SciPy's upfirdn adds is added here (zero taps included, samples outside [0, T) are zeros), so a non-finite sample
// poisons exactly the outputs whose window covers it.
//
// Work split.  Outputs m and m + up share a phase (their windows lie `down` inputs apart): a workgroup takes a tile of up*G*E
// outputs (m0 a multiple of up), thread q < up*G owns the outputs m0 + q + up*G*e (e < E), all of one phase, keeps that phase's
// Lp taps in registers and reads the inputs from the tile's window staged once in LDS.  Per tap: one LDS read and one fma,
// no coefficient traffic.  The HBM floor is e*(T + n_out) bytes per row; the window's halo (Lp - 1 samples per tile) is the
// only input read twice.  Three kernels (tfx_resample_plan_info reports which):
//   REG     window in LDS, taps in registers (Lp <= 64, rounded up to 8, 16, 24, 32, 48 or 64 with zero taps);
//   LDS     window in LDS, taps read through L1/L2 per term (Lp > 64);
//   GATHER  window does not fit in LDS (down or Lp in the thousands): inputs and taps read through L1/L2 (correct, not fast).
// All indices are 64-bit: (m + n_pre_remove) * down passes 2^31 on long rows.
#include "common.h"
#include "plan_cache.h"
#include "polyphase.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <vector>

namespace tfx {

constexpr int RS_THREADS = 512;
constexpr int64_t RS_LDS_BYTES = 49152;                  // three workgroups of 8 waves per CU
constexpr int64_t RS_EMAX = 64;                           // outputs per thread and tile
enum { RS_REG = 0, RS_LDS = 1, RS_GATHER = 2, RS_COPY = 3 };

// workgroup geometry: G phase groups of `up` threads, E outputs per thread, `span` inputs in the tile's window
struct ResampleTiling {
    int kernel;
    int64_t G, E, span, tile_out, lds;
    int64_t G0;                 // G before the halving loop (tfx_resample_tiling_info reports it; no launch reads it)
    int64_t LP;                 // REG: taps held in registers (Lp rounded up to a bucket), else Lp
};

static int64_t window_span(int64_t up, int64_t down, int64_t pre, int64_t Lp, int64_t G, int64_t E)
{
    return (pre + up * G - 1) * down / up - pre * down / up + Lp + G * down * (E - 1);
}

static ResampleTiling resample_tiling(int64_t up, int64_t down, int64_t pre, int64_t Lp, int esz)
{
    ResampleTiling t{};
    if (up == down) {
        t.kernel = RS_COPY;
        return t;
    }
    const int64_t cap = RS_LDS_BYTES / esz;
    t.G = t.G0 = up >= RS_THREADS ? 1 : RS_THREADS / up;
    t.LP = reg_bucket(Lp) ? reg_bucket(Lp) : Lp;              // the window reaches LP - 1 inputs behind the first output
    while (t.G > 1 && window_span(up, down, pre, t.LP, t.G, 1) > cap) t.G = (t.G + 1) / 2;
    const int64_t s1 = window_span(up, down, pre, t.LP, t.G, 1);
    if (s1 > cap) {
        t.kernel = RS_GATHER;
        t.LP = Lp;
        t.E = std::max<int64_t>(1, std::min<int64_t>(RS_EMAX, 4096 / (up * t.G)));
    } else {
        t.kernel = reg_bucket(Lp) ? RS_REG : RS_LDS;
        t.E = std::min<int64_t>(RS_EMAX, 1 + (cap - s1) / (t.G * down));
        t.span = window_span(up, down, pre, t.LP, t.G, t.E);
        t.lds = t.span * esz;
    }
    t.tile_out = up * t.G * t.E;
    return t;
}

template <typename T> struct ResampleArgs {
    const T *x;                 // [rows, T_]
    T *y;                       // [rows, n_out - m_begin]
    const T *hp;                // [up, Lp]
    int64_t T_, n_out, tiles;
    int64_t up, down, pre, pre_div, Lp;
    int64_t halo;               // window inputs behind x[n / up] of the tile's first output: LP - 1 (>= Lp - 1)
    int64_t G, E, span, tile_out;
    // stream only: x holds the absolute inputs [N, N + T_), hist the H before them (null: zeros); the launch computes outputs
    // [m_begin, n_out) in tiles from m_base = m_begin rounded down to a multiple of up, and writes the new history to hist_out
    const T *hist;              // [rows, H]
    T *hist_out;                // [rows, H]
    int64_t N, H, m_begin, m_base;
};

// LP > 0: taps in registers, zero past Lp (LP >= Lp);  LP == 0: taps through the cache.  STAGE: inputs from the LDS window.
// Register taps run LP terms per output: the extra ones are 0 * x[n / up - j] for j >= Lp, exact (+0 or -0 added) while the
// window is finite.  A workgroup whose window holds a NaN or an Inf sums exactly the Lp terms SciPy sums instead, so the
// non-finite samples poison the same outputs.
// STREAM: one chunk of a stream (tfx_resample_stream_forward).  Inputs come from the history and the chunk by absolute index,
// zeros before the history and past the chunk; the per-output sum (order, taps, start from +0) is the one-shot kernel's, so a
// finite stream gives its bits.  Tile 0 of every row also writes the row's new history.
template <typename T, bool STREAM>
__device__ __forceinline__ T rs_load(const ResampleArgs<T> &p, const T *xr, const T *hr, int64_t i)
{
    if (!STREAM) return (i >= 0 && i < p.T_) ? xr[i] : (T)0;
    const int64_t k = i - p.N;
    if (k >= 0) return k < p.T_ ? xr[k] : (T)0;
    return (hr && k >= -p.H) ? hr[k + p.H] : (T)0;
}
// rs_load as tp_stage's row
template <typename T, bool STREAM> struct RsRow {
    const ResampleArgs<T> &p;
    const T *xr, *hr;
    __device__ __forceinline__ T at(int64_t i) const { return rs_load<T, STREAM>(p, xr, hr, i); }
};

template <typename T, int LP, bool STAGE, bool STREAM>
__global__ void __launch_bounds__(RS_THREADS) resample_kernel(const ResampleArgs<T> p)
{
    extern __shared__ unsigned char rs_lds_raw[];
    T *win = (T *)rs_lds_raw;
    const int64_t row = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const T *xr = p.x + row * p.T_;
    const T *hr = STREAM && p.hist ? p.hist + row * p.H : nullptr;
    const int64_t mb = STREAM ? p.m_begin : 0;
    T *yr = p.y + row * (p.n_out - mb);
    if (STREAM) {
        if (tile == 0) {                                            // new history: the last H of [hist | chunk]
            T *ho = p.hist_out + row * p.H;
            for (int64_t k = threadIdx.x; k < p.H; k += RS_THREADS) ho[k] = stream_hist_at(xr, hr, p.T_, p.H, k);
        }
        if (p.n_out <= mb) return;                                  // a chunk that completes no output (uniform per launch)
    }
    const int64_t m0 = (STREAM ? p.m_base : 0) + tile * p.tile_out;     // a multiple of up
    const int64_t s0 = (m0 / p.up) * p.down + p.pre_div - p.halo;    // first input of the window
    bool finite = true;
    if (STAGE) {
        const bool bad = tp_stage<1, 0, RS_THREADS>(win, RsRow<T, STREAM>{p, xr, hr}, s0, (int)p.span, (int)threadIdx.x);
        finite = !__syncthreads_or(bad);
    }
    const int64_t nq = p.up * p.G, step = p.up * p.G;
    const int wstep = (int)(p.G * p.down);
    for (int64_t q = threadIdx.x; q < nq; q += RS_THREADS) {
        // output m0 + q + step*e: n = (m0 + pre + q)*down + step*e*down, phase (pre + q)*down mod up for every e
        const int64_t c = (p.pre + q) * p.down;
        const T *h = p.hp + (c % p.up) * p.Lp;
        const int64_t last = c / p.up - p.pre_div + p.halo;       // window index of x[n / up] for e = 0
        if (LP > 0 && finite) {
            T tap[LP > 0 ? LP : 1];
#pragma unroll
            for (int j = 0; j < (LP > 0 ? LP : 1); ++j) tap[j] = j < p.Lp ? h[j] : (T)0;
#pragma unroll 2
            for (int64_t e = 0; e < p.E; ++e) {
                const int64_t m = m0 + q + step * e;
                if (m >= p.n_out) break;
                if (STREAM && m < mb) continue;
                const T *w = win + ((int)last + wstep * (int)e);
                T acc = (T)0;
#pragma unroll
                for (int j = (LP > 0 ? LP : 1) - 1; j >= 0; --j) acc = fma(tap[j], w[-j], acc);
                yr[m - mb] = acc;
            }
            continue;
        }
        for (int64_t e = 0; e < p.E; ++e) {
            const int64_t m = m0 + q + step * e;
            if (m >= p.n_out) break;
            if (STREAM && m < mb) continue;
            const int64_t li = last + (int64_t)wstep * e;
            T acc = (T)0;
            if (STAGE) {
                const T *w = win + li;
                for (int64_t j = p.Lp - 1; j >= 0; --j) acc = fma(h[j], w[-j], acc);
            } else {
                // x[i - j], j < Lp, inside the inputs there are: [0, T) (stream: [max(0, N - H), N + T))
                const int64_t i = s0 + li;
                const int64_t lo = STREAM ? (p.N - p.H > 0 ? p.N - p.H : 0) : 0, hi = (STREAM ? p.N : 0) + p.T_ - 1;
                const int64_t j_lo = i - hi > 0 ? i - hi : 0, j_hi = i - lo < p.Lp - 1 ? i - lo : p.Lp - 1;
                for (int64_t j = j_hi; j >= j_lo; --j) acc = fma(h[j], STREAM ? rs_load<T, true>(p, xr, hr, i - j) : xr[i - j], acc);
            }
            yr[m - mb] = acc;
        }
    }
}

static void resample_check(const void *x, const void *y, int dtype, int64_t rows, int64_t T, int64_t up, int64_t down,
                           const void *taps_host, int64_t nh)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "resample_forward: bad dtype %d", dtype);
    TFX_CHECK(up >= 1 && down >= 1, "resample_forward: up and down must be >= 1, got %lld / %lld", (long long)up, (long long)down);
    TFX_CHECK(rows >= 0 && T >= 0, "resample_forward: negative size");
    TFX_CHECK(nh >= 1 && taps_host, "resample_forward: no taps");
    TFX_CHECK(up <= (1ll << 24) && down <= (1ll << 24) && nh <= (1ll << 30), "resample_forward: up, down or taps too large");
    TFX_CHECK(T <= (INT64_MAX / 4) / (up * down), "resample_forward: T * up * down overflows");
    const int64_t n_out = ceil_div(T * up, down);
    TFX_CHECK(rows == 0 || (T <= INT64_MAX / 16 / rows && n_out <= INT64_MAX / 16 / rows), "resample_forward: size overflows");
    TFX_CHECK((x || rows * T == 0) && (y || rows * n_out == 0), "resample_forward: null pointer");
}

static int64_t gcd64(int64_t a, int64_t b)
{
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

static void resample_plan(int64_t T, int64_t up, int64_t down, int64_t nh, int esz, ResampleGeom *g, ResampleTiling *t)
{
    const int64_t d = gcd64(up, down);
    up /= d;
    down /= d;
    *g = resample_geometry(T, up, down, nh);
    *t = resample_tiling(up, down, g->pre_remove, g->Lp, esz);
}

// host-only: what resample_forward would do (arguments as resample_check's, without the pointers)
void resample_plan_info(int64_t T, int64_t up, int64_t down, int64_t nh, int dtype, int64_t *n_out, int64_t *pre_remove,
                        int64_t *padded, int64_t *Lp, int *kernel, int64_t *lds_bytes)
{
    const int one = 1;
    resample_check(&one, &one, dtype, 1, T, up, down, &one, nh);
    ResampleGeom g;
    ResampleTiling t;
    resample_plan(T, up, down, nh, dtype == TFX_F32 ? 4 : 8, &g, &t);
    *n_out = g.n_out;
    *pre_remove = g.pre_remove;
    *padded = g.padded;
    *Lp = g.Lp;
    *kernel = t.kernel;
    *lds_bytes = t.lds;
}

// host-only: the workgroup geometry of that launch, from the same resample_plan() call (span is 0 for GATHER, which stages no
// window; everything is 0 for the copy of up == down)
void resample_tiling_info(int64_t T, int64_t up, int64_t down, int64_t nh, int dtype, int *kernel, int64_t *G, int64_t *G_initial,
                          int64_t *E, int64_t *tile_out, int64_t *span, int64_t *LP, int64_t *tiles)
{
    const int one = 1;
    resample_check(&one, &one, dtype, 1, T, up, down, &one, nh);
    ResampleGeom g;
    ResampleTiling t;
    resample_plan(T, up, down, nh, dtype == TFX_F32 ? 4 : 8, &g, &t);
    *kernel = t.kernel;
    *G = t.G;
    *G_initial = t.G0;
    *E = t.E;
    *tile_out = t.tile_out;
    *span = t.span;
    *LP = t.LP;
    *tiles = t.tile_out ? ceil_div(g.n_out, t.tile_out) : 0;
}

// polyphase tables by content: the taps' bytes plus (up, down, dtype, n_pre_pad, Lp).  A stream's table has Lp_s taps per phase,
// a one-shot call's SciPy's Lp >= Lp_s: the two share an entry wherever the geometry agrees.
static PlanCache<DeviceBuffer, 5> g_tables(32, "resample_forward");

template <typename T>
const T *resample_table(const void *taps_host, int64_t nh, int64_t up, int64_t down, int64_t pre_pad, int64_t Lp,
                               hipStream_t stream, std::shared_ptr<DeviceBuffer> *keep)
{
    const int64_t tail[5] = {up, down, (int64_t)sizeof(T), pre_pad, Lp};
    *keep = g_tables.get(taps_host, (size_t)nh * sizeof(T), tail, stream, [&] {
        std::vector<T> hp((size_t)(up * Lp), (T)0);
        const T *h = (const T *)taps_host;
        for (int64_t k = 0; k < nh; ++k) {                       // h_padded[pre_pad + k] = h[k] -> hp[p][j], p + j*up
            const int64_t s = pre_pad + k;
            hp[(size_t)((s % up) * Lp + s / up)] = h[k];
        }
        return std::make_shared<DeviceBuffer>(hp);
    });
    return (const T *)(*keep)->p;
}
template const float *resample_table<float>(const void *, int64_t, int64_t, int64_t, int64_t, int64_t, hipStream_t,
                                             std::shared_ptr<DeviceBuffer> *);
template const double *resample_table<double>(const void *, int64_t, int64_t, int64_t, int64_t, int64_t, hipStream_t,
                                               std::shared_ptr<DeviceBuffer> *);

template <typename T, bool STREAM>
static void resample_dispatch(const ResampleArgs<T> &p, int64_t rows, const ResampleTiling &t, hipStream_t stream)
{
    static const char *const names[2][3] = {{"resample_reg_kernel", "resample_lds_kernel", "resample_gather_kernel"},
                                            {"resample_stream_reg_kernel", "resample_stream_lds_kernel", "resample_stream_gather_kernel"}};
    const int64_t nwg = rows * p.tiles;
    TFX_CHECK(nwg < (1ll << 31), "resample_forward: grid too large");
    const dim3 grid((unsigned)nwg), block(RS_THREADS);
    ProfScope ps(names[STREAM][t.kernel], stream);
    if (t.kernel == RS_REG) {
        switch (t.LP) {
        case 8: hipLaunchKernelGGL((resample_kernel<T, 8, true, STREAM>), grid, block, (size_t)t.lds, stream, p); break;
        case 16: hipLaunchKernelGGL((resample_kernel<T, 16, true, STREAM>), grid, block, (size_t)t.lds, stream, p); break;
        case 24: hipLaunchKernelGGL((resample_kernel<T, 24, true, STREAM>), grid, block, (size_t)t.lds, stream, p); break;
        case 32: hipLaunchKernelGGL((resample_kernel<T, 32, true, STREAM>), grid, block, (size_t)t.lds, stream, p); break;
        case 48: hipLaunchKernelGGL((resample_kernel<T, 48, true, STREAM>), grid, block, (size_t)t.lds, stream, p); break;
        default: hipLaunchKernelGGL((resample_kernel<T, 64, true, STREAM>), grid, block, (size_t)t.lds, stream, p); break;
        }
    } else if (t.kernel == RS_LDS) {
        hipLaunchKernelGGL((resample_kernel<T, 0, true, STREAM>), grid, block, (size_t)t.lds, stream, p);
    } else {
        hipLaunchKernelGGL((resample_kernel<T, 0, false, STREAM>), grid, block, 0, stream, p);
    }
    TFX_HIP(hipGetLastError());
}

template <typename T>
static void resample_launch(const void *x, void *y, int64_t rows, int64_t T_, int64_t up, int64_t down, const void *taps_host,
                            int64_t nh, const ResampleGeom &g, const ResampleTiling &t, hipStream_t stream)
{
    std::shared_ptr<DeviceBuffer> table;
    ResampleArgs<T> p{};
    p.x = (const T *)x; p.y = (T *)y; p.hp = resample_table<T>(taps_host, nh, up, down, g.pre_pad, g.Lp, stream, &table);
    p.T_ = T_; p.n_out = g.n_out; p.up = up; p.down = down; p.pre = g.pre_remove; p.pre_div = g.pre_remove * down / up; p.Lp = g.Lp;
    p.G = t.G; p.E = t.E; p.span = t.span; p.tile_out = t.tile_out; p.halo = t.LP - 1;
    p.tiles = ceil_div(g.n_out, t.tile_out);
    resample_dispatch<T, false>(p, rows, t, stream);
}

void resample_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t up, int64_t down, const void *taps_host,
                      int64_t nh, hipStream_t stream)
{
    resample_check(x, y, dtype, rows, T, up, down, taps_host, nh);
    const int64_t d = gcd64(up, down);
    up /= d;
    down /= d;
    const int esz = dtype == TFX_F32 ? 4 : 8;
    if (up == down) {                                           // resample_poly returns a copy
        if (rows * T) TFX_HIP(hipMemcpyAsync(y, x, (size_t)(rows * T * esz), hipMemcpyDeviceToDevice, stream));
        return;
    }
    ResampleGeom g;
    ResampleTiling t;
    resample_plan(T, up, down, nh, esz, &g, &t);
    if (rows == 0 || g.n_out == 0) return;
    if (dtype == TFX_F32) resample_launch<float>(x, y, rows, T, up, down, taps_host, nh, g, t, stream);
    else resample_launch<double>(x, y, rows, T, up, down, taps_host, nh, g, t, stream);
}

// ---- streams: one chunk per launch --------------------------------------------------------------------------------------
// The geometry a stream fixes up front (up, down reduced): SciPy's n_pre_pad and n_pre_remove, Lp_s = ceil((nh + n_pre_pad) / up)
// taps per phase (no length-dependent post-padding) and the H = Lp_s - 1 inputs each row carries.  After N inputs the stream
// has emitted M(N) = max(0, ceil(N*up/down) - n_pre_remove) outputs: output m reads inputs up to (m + n_pre_remove)*down/up,
// which is < N for every m < M(N), and none older than N - H for m >= M(N).
struct ResampleStreamGeom {
    int64_t pre_pad, pre_remove, Lp, H, m_begin, m_end;
};

static int64_t stream_emitted(int64_t N, int64_t up, int64_t down, int64_t pre)
{
    const int64_t m = ceil_div(N * up, down) - pre;
    return m > 0 ? m : 0;
}

static ResampleStreamGeom resample_stream_geometry(int64_t N, int64_t T, int64_t up, int64_t down, int64_t nh)
{
    ResampleStreamGeom g{};
    if (up == down) {                                           // a copy: nothing held back, nothing carried
        g.m_begin = N;
        g.m_end = N + T;
        return g;
    }
    const int64_t half_len = (nh - 1) / 2;
    g.pre_pad = down - half_len % down;
    g.pre_remove = (half_len + g.pre_pad) / down;
    g.Lp = ceil_div(nh + g.pre_pad, up);
    g.H = g.Lp - 1;
    g.m_begin = stream_emitted(N, up, down, g.pre_remove);
    g.m_end = stream_emitted(N + T, up, down, g.pre_remove);
    return g;
}

struct ResampleStreamPlan {
    int64_t up, down;                    // reduced
    ResampleStreamGeom g;
    ResampleTiling t;
};

// every refusal of resample_stream_forward (host-only); hands back the plan it built on the way
static ResampleStreamPlan resample_stream_check(const void *x, const void *y, int dtype, int64_t rows, int64_t T, int64_t up,
                                                int64_t down, const void *taps_host, int64_t nh, int64_t consumed,
                                                const void *hist_in, const void *hist_out)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "resample_stream_forward: bad dtype %d", dtype);
    TFX_CHECK(up >= 1 && down >= 1, "resample_stream_forward: up and down must be >= 1, got %lld / %lld", (long long)up,
              (long long)down);
    TFX_CHECK(rows >= 0 && T >= 0 && consumed >= 0, "resample_stream_forward: negative size or consumed count");
    TFX_CHECK(nh >= 1 && taps_host, "resample_stream_forward: no taps");
    TFX_CHECK(up <= (1ll << 24) && down <= (1ll << 24) && nh <= (1ll << 30), "resample_stream_forward: up, down or taps too large");
    TFX_CHECK(T <= INT64_MAX / 8 - consumed && consumed + T <= (INT64_MAX / 4) / (up * down),
              "resample_stream_forward: (consumed + T) * up * down overflows");
    const int esz = dtype == TFX_F32 ? 4 : 8;
    const int64_t d = gcd64(up, down);
    ResampleStreamPlan pl{up / d, down / d, {}, {}};
    pl.g = resample_stream_geometry(consumed, T, pl.up, pl.down, nh);
    pl.t = resample_tiling(pl.up, pl.down, pl.g.pre_remove, pl.g.Lp, esz);
    const ResampleStreamGeom &g = pl.g;
    const int64_t n_y = g.m_end - g.m_begin;
    TFX_CHECK(rows == 0 || (T <= INT64_MAX / 16 / rows && n_y <= INT64_MAX / 16 / rows && g.H <= INT64_MAX / 16 / rows),
              "resample_stream_forward: size overflows");
    TFX_CHECK((x || rows * T == 0) && (y || rows * n_y == 0) && (hist_out || rows * g.H == 0), "resample_stream_forward: null pointer");
    check_stream_buffers("resample_stream_forward", esz, x, rows * T, y, rows * n_y, hist_in, hist_out, rows * g.H);
    return pl;
}

// host-only: what resample_stream_forward does with a chunk of T samples after `consumed` (arguments as resample_stream_check's)
void resample_stream_plan_info(int64_t consumed, int64_t T, int64_t up, int64_t down, int64_t nh, int dtype, int64_t *out_begin,
                               int64_t *out_end, int64_t *hist_len, int64_t *pre_remove, int64_t *Lp, int *kernel,
                               int64_t *lds_bytes)
{
    const int one = 1;
    const ResampleStreamPlan pl = resample_stream_check(&one, &one, dtype, 0, T, up, down, &one, nh, consumed, nullptr, nullptr);
    *out_begin = pl.g.m_begin;
    *out_end = pl.g.m_end;
    *hist_len = pl.g.H;
    *pre_remove = pl.g.pre_remove;
    *Lp = pl.g.Lp;
    *kernel = pl.t.kernel;
    *lds_bytes = pl.t.lds;
}

constexpr int64_t RS_STREAM_MIN_WG = 256;                // one workgroup per CU

// A chunk can be short next to a whole signal (2 x 512 in real time is a tile or two): halve the outputs per thread until the
// launch has RS_STREAM_MIN_WG workgroups (or E = 1).  Not further: below ~8 outputs per thread the register taps are loaded for
// too few outputs (a 1536-workgroup target made 64 x 65536-sample chunks at 160/147 1.6x slower).  The sum each output gets
// does not depend on the tiling.
static ResampleTiling stream_tiling(ResampleTiling t, int64_t rows, int64_t up, int64_t down, int64_t pre, int64_t n_tile_out,
                                    int esz)
{
    while (t.E > 1 && rows * ceil_div(n_tile_out, t.tile_out) < RS_STREAM_MIN_WG) {
        t.E = (t.E + 1) / 2;
        t.tile_out = up * t.G * t.E;
        if (t.kernel != RS_GATHER) {
            t.span = window_span(up, down, pre, t.LP, t.G, t.E);
            t.lds = t.span * esz;
        }
    }
    return t;
}

template <typename T>
static void resample_stream_launch(const void *x, void *y, int64_t rows, int64_t T_, int64_t up, int64_t down,
                                   const void *taps_host, int64_t nh, int64_t N, const void *hist_in, void *hist_out,
                                   const ResampleStreamGeom &g, const ResampleTiling &t0, hipStream_t stream)
{
    const int64_t m_base = g.m_begin / up * up;
    const ResampleTiling t = stream_tiling(t0, rows, up, down, g.pre_remove, g.m_end - m_base, (int)sizeof(T));
    std::shared_ptr<DeviceBuffer> table;
    ResampleArgs<T> p{};
    p.x = (const T *)x; p.y = (T *)y; p.hp = resample_table<T>(taps_host, nh, up, down, g.pre_pad, g.Lp, stream, &table);
    p.T_ = T_; p.n_out = g.m_end; p.up = up; p.down = down; p.pre = g.pre_remove; p.pre_div = g.pre_remove * down / up; p.Lp = g.Lp;
    p.G = t.G; p.E = t.E; p.span = t.span; p.tile_out = t.tile_out; p.halo = t.LP - 1;
    p.hist = (const T *)hist_in; p.hist_out = (T *)hist_out; p.N = N; p.H = g.H;
    p.m_begin = g.m_begin; p.m_base = m_base;
    // at least one tile per row: tile 0 writes the new history even when the chunk completes no output
    p.tiles = std::max<int64_t>(1, ceil_div(g.m_end - p.m_base, t.tile_out));
    resample_dispatch<T, true>(p, rows, t, stream);
}

void resample_stream_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t up, int64_t down,
                             const void *taps_host, int64_t nh, int64_t consumed, const void *hist_in, void *hist_out,
                             hipStream_t stream)
{
    const ResampleStreamPlan pl = resample_stream_check(x, y, dtype, rows, T, up, down, taps_host, nh, consumed, hist_in, hist_out);
    const int esz = dtype == TFX_F32 ? 4 : 8;
    const ResampleStreamGeom &g = pl.g;
    const ResampleTiling &t = pl.t;
    up = pl.up;
    down = pl.down;
    if (rows == 0) return;
    if (t.kernel == RS_COPY) {                                  // up == down: y = x, no history
        if (T) TFX_HIP(hipMemcpyAsync(y, x, (size_t)(rows * T * esz), hipMemcpyDeviceToDevice, stream));
        return;
    }
    if (g.m_end == g.m_begin && g.H == 0) return;               // nothing to emit and nothing to carry
    if (dtype == TFX_F32) resample_stream_launch<float>(x, y, rows, T, up, down, taps_host, nh, consumed, hist_in, hist_out, g, t, stream);
    else resample_stream_launch<double>(x, y, rows, T, up, down, taps_host, nh, consumed, hist_in, hist_out, g, t, stream);
}

// ---- true peak: max |y| over a row's up-sampled outputs, the up-sampled signal never stored --------------------------------
// BS.1770-4 Annex 2 reading (tfx_true_peak_forward): peak[row] = max_m |y[m]| with y = resample_forward(x, up, 1), every y[m]
// the same descending-j fma chain from +0 over hp[phase][j], so a finite row gives the bits of the composition.  With down = 1
// the `up` outputs n = i*up + phase of one input position i read the same Lp inputs x[i - j]: a thread takes TP_R consecutive
// positions, holds their TP_R + LP - 1 inputs in registers and runs phase after phase over them.  The taps of a phase are the
// same for every lane (scalar loads, one move each into a vector register per phase), so a term costs one fma and nothing
// else; the LDS window is read once per thread, (TP_R + LP - 1) / TP_R reads per position instead of up * Lp.
//   tile      TP_THREADS * TP_R positions of one row; its window (LP - 1 inputs of halo in front) is staged in LDS transposed
//             (tp_stage, polyphase.h); the chain is tp_phase, this kernel's part is what it does with a phase's sums
//   edges     only the row's first and last positions have phases that are no output (n outside [pre, pre + T*up)); the two
//             threads that own them take tp_phase_at over the window with the bounds test, everyone else the unrolled chain
//   reduce    running NaN-propagating max per thread, lane shuffles, LDS across the four waves, ONE writer of work[row, tile];
//             true_peak_fold_kernel (one workgroup per row) folds work[row, :] into peak[row].  No atomics.
//   non-finite  a tile whose window holds a NaN or an Inf writes NaN (the row's reading is NaN; other rows are untouched)
// The tiling is fixed (it does not depend on rows), so a row's bits do not depend on the batch.
template <typename T> struct TruePeakArgs {
    const T *x;                 // [rows, T_]
    T *work;                    // [rows, tiles]
    const T *hp;                // [up, LP]: resample_table's layout with LP >= Lp taps per phase, zeros past Lp
    int64_t T_, tiles, up;
    int64_t i_lo;               // pre / up: the input position of the row's first output
    int64_t n_lo, n_hi;         // n = i*up + phase is an output for n in [pre, pre + T_*up)
};

template <typename T> __device__ __forceinline__ T tp_block_max(T m, T *part)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) m = tp_max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < TP_THREADS / 64; ++w) m = tp_max(m, part[w]);
    return m;                                                   // thread 0 holds the workgroup's
}

template <typename T, int LP>
__global__ void __launch_bounds__(TP_THREADS) true_peak_kernel(const TruePeakArgs<T> p)
{
    constexpr int S = tp_stride<T>(), NW = TP_R + LP - 1, SPAN = (int)TP_TILE + LP - 1;
    static_assert(TP_THREADS + (LP - 2) / TP_R + 1 <= S, "the halo columns must fit the line");
    extern __shared__ unsigned char rs_lds_raw[];
    __shared__ T part[TP_THREADS / 64];
    T *win = (T *)rs_lds_raw;
    const int64_t row = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const StreamRow<T, false> xr(p.x, p.T_, nullptr, 0, 0, p.T_, row);
    const int64_t P0 = tile * TP_TILE;                           // the tile's first position, counted from i_lo
    const int64_t s0 = p.i_lo + P0 - (LP - 1);                   // first input of the window
    const int t = (int)threadIdx.x;
    if (__syncthreads_or(tp_stage<TP_R, S, TP_THREADS>(win, xr, s0, SPAN, t))) {
        if (t == 0) p.work[blockIdx.x] = (T)NAN;
        return;
    }
    const int64_t nf = (p.i_lo + P0 + (int64_t)t * TP_R) * p.up;    // n of the thread's first position, phase 0
    const int up = (int)p.up;
    T m = (T)0;
    if (nf >= p.n_lo && nf + (int64_t)TP_R * up <= p.n_hi) {
        T xw[NW];
        tp_window<TP_R, S>(xw, win, t);
        unsigned mb = 0;                                         // f32: |acc| compared as bits, NaN above Inf
#pragma unroll 1
        for (int ph = 0; ph < up; ++ph) {
            T acc[TP_R];
            tp_phase<LP>(acc, p.hp + ph * LP, xw);
#pragma unroll
            for (int r = 0; r < TP_R; ++r) {
                if constexpr (sizeof(T) == 4) {
                    const unsigned a = __float_as_uint(acc[r]) & 0x7fffffffu;
                    mb = a > mb ? a : mb;
                } else {
                    m = tp_max(m, fabs(acc[r]));
                }
            }
        }
        if constexpr (sizeof(T) == 4) m = __uint_as_float(mb);
    } else if (nf < p.n_hi) {
        for (int r = 0; r < TP_R; ++r)
            for (int ph = 0; ph < up; ++ph) {
                const int64_t n = nf + (int64_t)r * up + ph;
                if (n < p.n_lo || n >= p.n_hi) continue;
                m = tp_max(m, (T)fabs(tp_phase_at<TP_R, S>(p.hp + ph * LP, LP, LP, win, t, r)));
            }
    }
    m = tp_block_max(m, part);
    if (t == 0) p.work[blockIdx.x] = m;
}

template <typename T> __global__ void __launch_bounds__(TP_THREADS) true_peak_fold_kernel(const T *work, T *peak, int64_t tiles)
{
    __shared__ T part[TP_THREADS / 64];
    const T *w = work + (int64_t)blockIdx.x * tiles;
    T m = (T)0;
    for (int64_t k = threadIdx.x; k < tiles; k += TP_THREADS) m = tp_max(m, w[k]);
    m = tp_block_max(m, part);
    if (threadIdx.x == 0) peak[blockIdx.x] = m;
}

struct TruePeakPlan : InterpPlan {
    int64_t tiles;
};

// everything but the pointers (host-only)
static TruePeakPlan true_peak_plan(int dtype, int64_t rows, int64_t T, int64_t up, int64_t nh)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "true_peak_forward: bad dtype %d", dtype);
    TFX_CHECK(up == 2 || up == 4 || up == 8, "true_peak_forward: up must be 2, 4 or 8, got %lld", (long long)up);
    TFX_CHECK(rows >= 0 && T >= 0, "true_peak_forward: negative size");
    TruePeakPlan pl{interp_plan("true_peak_forward", up, nh, T), 0};
    pl.tiles = T ? ceil_div((pl.g.pre_remove + T * up - 1) / up - pl.i_lo + 1, TP_TILE) : 0;
    TFX_CHECK(rows == 0 || (T <= INT64_MAX / 16 / rows && pl.tiles < (1ll << 31) / rows), "true_peak_forward: size overflows");
    return pl;
}

// every refusal of true_peak_forward (host-only); hands back the plan it built on the way
static TruePeakPlan true_peak_check(const void *x, int dtype, const void *peak, int64_t rows, int64_t T, int64_t up,
                                    const void *taps_host, int64_t nh, const void *work)
{
    const TruePeakPlan pl = true_peak_plan(dtype, rows, T, up, nh);
    TFX_CHECK(taps_host, "true_peak_forward: no taps");
    TFX_CHECK(rows * T == 0 || (x && peak && work), "true_peak_forward: null pointer");
    return pl;
}

void true_peak_plan_info(int64_t rows, int64_t T, int64_t up, int64_t nh, int dtype, int64_t *Lp, int64_t *tile_in, int64_t *tiles,
                         int64_t *work_elems)
{
    const TruePeakPlan pl = true_peak_plan(dtype, rows, T, up, nh);
    *Lp = pl.g.Lp;
    *tile_in = TP_TILE;
    *tiles = pl.tiles;
    *work_elems = rows * pl.tiles;
}

template <typename T>
static void true_peak_launch(const void *x, void *peak, int64_t rows, int64_t T_, int64_t up, const void *taps_host, int64_t nh,
                             void *work, const TruePeakPlan &pl, hipStream_t stream)
{
    std::shared_ptr<DeviceBuffer> table;
    TruePeakArgs<T> p{};
    p.x = (const T *)x; p.work = (T *)work; p.hp = resample_table<T>(taps_host, nh, up, 1, pl.g.pre_pad, pl.LP, stream, &table);
    p.T_ = T_; p.tiles = pl.tiles; p.up = up; p.i_lo = pl.i_lo;
    p.n_lo = pl.g.pre_remove; p.n_hi = pl.g.pre_remove + T_ * up;
    const dim3 grid((unsigned)(rows * pl.tiles)), block(TP_THREADS);
    const size_t lds = (size_t)TP_R * tp_stride<T>() * sizeof(T);
    {
        ProfScope ps("true_peak_kernel", stream);
        tp_dispatch(pl.LP, [&](auto lp) { hipLaunchKernelGGL((true_peak_kernel<T, lp()>), grid, block, lds, stream, p); });
        TFX_HIP(hipGetLastError());
    }
    ProfScope ps("true_peak_fold_kernel", stream);
    hipLaunchKernelGGL((true_peak_fold_kernel<T>), dim3((unsigned)rows), block, 0, stream, (const T *)work, (T *)peak, pl.tiles);
    TFX_HIP(hipGetLastError());
}

void true_peak_forward(const void *x, int dtype, void *peak, int64_t rows, int64_t T, int64_t up, const void *taps_host, int64_t nh,
                       void *work, hipStream_t stream)
{
    const TruePeakPlan pl = true_peak_check(x, dtype, peak, rows, T, up, taps_host, nh, work);
    if (rows * T == 0) return;                                  // a row of no samples has peak 0: nothing is written
    if (dtype == TFX_F32) true_peak_launch<float>(x, peak, rows, T, up, taps_host, nh, work, pl, stream);
    else true_peak_launch<double>(x, peak, rows, T, up, taps_host, nh, work, pl, stream);
}

void resample_clear() { g_tables.clear(); }

}  // namespace tfx
