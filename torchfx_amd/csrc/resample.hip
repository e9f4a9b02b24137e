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
#include "../../include/torchfx_hip.h"

#include <vector>

namespace tfx {

constexpr int RS_THREADS = 512;
constexpr int64_t RS_LDS_BYTES = 49152;                  // three workgroups of 8 waves per CU
constexpr int64_t RS_EMAX = 64;                           // outputs per thread and tile
enum { RS_REG = 0, RS_LDS = 1, RS_GATHER = 2, RS_COPY = 3 };

// scipy.signal.resample_poly's arithmetic for a filter of nh taps (up, down already reduced)
struct ResampleGeom {
    int64_t n_out, pre_pad, post_pad, pre_remove, padded, Lp;
};

static int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

static ResampleGeom resample_geometry(int64_t T, int64_t up, int64_t down, int64_t nh)
{
    ResampleGeom g{};
    g.n_out = ceil_div(T * up, down);
    const int64_t half_len = (nh - 1) / 2;
    g.pre_pad = down - half_len % down;
    g.pre_remove = (half_len + g.pre_pad) / down;
    // SciPy increments n_post_pad while _output_len(len, T, up, down) = ((T-1)*up + len - 1) // down + 1 < n_out + pre_remove;
    // the least such pad in closed form (floor division: T = 0 gives a negative numerator)
    const int64_t len0 = nh + g.pre_pad, need = g.n_out + g.pre_remove;
    const int64_t have = floor_div((T - 1) * up + len0 - 1, down) + 1;
    g.post_pad = have >= need ? 0 : down * (need - 1) - (T - 1) * up - len0 + 1;
    g.padded = len0 + g.post_pad;
    g.Lp = ceil_div(g.padded, up);
    return g;
}

// workgroup geometry: G phase groups of `up` threads, E outputs per thread, `span` inputs in the tile's window
struct ResampleTiling {
    int kernel;
    int64_t G, E, span, tile_out, lds;
    int64_t LP;                 // REG: taps held in registers (Lp rounded up to a bucket), else Lp
};

// register-tap buckets: each is one instantiation of the kernel
static int64_t reg_bucket(int64_t Lp)
{
    for (int64_t b : {8, 16, 24, 32, 48, 64})
        if (Lp <= b) return b;
    return 0;
}

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
    t.G = up >= RS_THREADS ? 1 : RS_THREADS / up;
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
    T *y;                       // [rows, n_out]
    const T *hp;                // [up, Lp]
    int64_t T_, n_out, tiles;
    int64_t up, down, pre, pre_div, Lp;
    int64_t halo;               // window inputs behind x[n / up] of the tile's first output: LP - 1 (>= Lp - 1)
    int64_t G, E, span, tile_out;
};

constexpr int RS_STAGE_BATCH = 8;                         // staging loads in flight per thread

// LP > 0: taps in registers, zero past Lp (LP >= Lp);  LP == 0: taps through the cache.  STAGE: inputs from the LDS window.
// Register taps run LP terms per output: the extra ones are 0 * x[n / up - j] for j >= Lp, exact (+0 or -0 added) while the
// window is finite.  A workgroup whose window holds a NaN or an Inf sums exactly the Lp terms SciPy sums instead, so the
// non-finite samples poison the same outputs.
template <typename T, int LP, bool STAGE>
__global__ void __launch_bounds__(RS_THREADS) resample_kernel(const ResampleArgs<T> p)
{
    extern __shared__ unsigned char rs_lds_raw[];
    T *win = (T *)rs_lds_raw;
    const int64_t row = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const T *xr = p.x + row * p.T_;
    T *yr = p.y + row * p.n_out;
    const int64_t m0 = tile * p.tile_out;                          // a multiple of up
    const int64_t s0 = (m0 / p.up) * p.down + p.pre_div - p.halo;    // first input of the window
    bool finite = true;
    if (STAGE) {
        const int span = (int)p.span;
        bool bad = false;
        for (int j0 = 0; j0 < span; j0 += RS_THREADS * RS_STAGE_BATCH) {
            T v[RS_STAGE_BATCH];
#pragma unroll
            for (int u = 0; u < RS_STAGE_BATCH; ++u) {
                const int j = j0 + u * RS_THREADS + (int)threadIdx.x;
                const int64_t i = s0 + j;
                v[u] = (j < span && i >= 0 && i < p.T_) ? xr[i] : (T)0;
            }
#pragma unroll
            for (int u = 0; u < RS_STAGE_BATCH; ++u) {
                const int j = j0 + u * RS_THREADS + (int)threadIdx.x;
                if (j < span) win[j] = v[u];
                bad |= !isfinite(v[u]);
            }
        }
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
                const T *w = win + ((int)last + wstep * (int)e);
                T acc = (T)0;
#pragma unroll
                for (int j = (LP > 0 ? LP : 1) - 1; j >= 0; --j) acc = fma(tap[j], w[-j], acc);
                yr[m] = acc;
            }
            continue;
        }
        for (int64_t e = 0; e < p.E; ++e) {
            const int64_t m = m0 + q + step * e;
            if (m >= p.n_out) break;
            const int64_t li = last + (int64_t)wstep * e;
            T acc = (T)0;
            if (STAGE) {
                const T *w = win + li;
                for (int64_t j = p.Lp - 1; j >= 0; --j) acc = fma(h[j], w[-j], acc);
            } else {
                const int64_t i = s0 + li;                          // x[i - j], j < Lp, inside [0, T)
                const int64_t j_lo = i - p.T_ + 1 > 0 ? i - p.T_ + 1 : 0, j_hi = i < p.Lp - 1 ? i : p.Lp - 1;
                for (int64_t j = j_hi; j >= j_lo; --j) acc = fma(h[j], xr[i - j], acc);
            }
            yr[m] = acc;
        }
    }
}

void resample_check(const void *x, const void *y, int dtype, int64_t rows, int64_t T, int64_t up, int64_t down,
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

// polyphase tables by content: the taps' bytes plus (up, down, dtype, n_pre_pad, Lp)
static PlanCache<DeviceBuffer, 5> g_tables(32, "resample_forward");

template <typename T>
static void resample_launch(const void *x, void *y, int64_t rows, int64_t T_, int64_t up, int64_t down, const void *taps_host,
                            int64_t nh, const ResampleGeom &g, const ResampleTiling &t, hipStream_t stream)
{
    const int64_t tail[5] = {up, down, (int64_t)sizeof(T), g.pre_pad, g.Lp};
    std::shared_ptr<DeviceBuffer> table = g_tables.get(taps_host, (size_t)nh * sizeof(T), tail, stream, [&] {
        std::vector<T> hp((size_t)(up * g.Lp), (T)0);
        const T *h = (const T *)taps_host;
        for (int64_t k = 0; k < nh; ++k) {                       // h_padded[g.pre_pad + k] = h[k] -> hp[p][j], p + j*up
            const int64_t s = g.pre_pad + k;
            hp[(size_t)((s % up) * g.Lp + s / up)] = h[k];
        }
        return std::make_shared<DeviceBuffer>(hp);
    });
    ResampleArgs<T> p{};
    p.x = (const T *)x; p.y = (T *)y; p.hp = (const T *)table->p;
    p.T_ = T_; p.n_out = g.n_out; p.up = up; p.down = down; p.pre = g.pre_remove; p.pre_div = g.pre_remove * down / up; p.Lp = g.Lp;
    p.G = t.G; p.E = t.E; p.span = t.span; p.tile_out = t.tile_out; p.halo = t.LP - 1;
    p.tiles = ceil_div(g.n_out, t.tile_out);
    const int64_t nwg = rows * p.tiles;
    TFX_CHECK(nwg < (1ll << 31), "resample_forward: grid too large");
    const dim3 grid((unsigned)nwg), block(RS_THREADS);
    if (t.kernel == RS_REG) {
        ProfScope ps("resample_reg_kernel", stream);
        switch (t.LP) {
        case 8: hipLaunchKernelGGL((resample_kernel<T, 8, true>), grid, block, (size_t)t.lds, stream, p); break;
        case 16: hipLaunchKernelGGL((resample_kernel<T, 16, true>), grid, block, (size_t)t.lds, stream, p); break;
        case 24: hipLaunchKernelGGL((resample_kernel<T, 24, true>), grid, block, (size_t)t.lds, stream, p); break;
        case 32: hipLaunchKernelGGL((resample_kernel<T, 32, true>), grid, block, (size_t)t.lds, stream, p); break;
        case 48: hipLaunchKernelGGL((resample_kernel<T, 48, true>), grid, block, (size_t)t.lds, stream, p); break;
        default: hipLaunchKernelGGL((resample_kernel<T, 64, true>), grid, block, (size_t)t.lds, stream, p); break;
        }
    } else if (t.kernel == RS_LDS) {
        ProfScope ps("resample_lds_kernel", stream);
        hipLaunchKernelGGL((resample_kernel<T, 0, true>), grid, block, (size_t)t.lds, stream, p);
    } else {
        ProfScope ps("resample_gather_kernel", stream);
        hipLaunchKernelGGL((resample_kernel<T, 0, false>), grid, block, 0, stream, p);
    }
    TFX_HIP(hipGetLastError());
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

void resample_clear() { g_tables.clear(); }

}  // namespace tfx
