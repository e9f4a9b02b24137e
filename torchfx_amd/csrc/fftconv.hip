// fftconv.hip -- overlap-save FFT convolution: rocFFT transforms + hand-written HIP
// frame / spectrum / un-frame kernels.
//
// Replaces fft_conv1d (src/torchfx/filter/_fftconv.py:70-141) -- F.pad, unfold (as_strided),
// torch.fft.rfft, `* kernel_z.conj()`, torch.fft.irfft, slice [:S], reshape, trim -- which in
// the reference materialises four full-size temporaries and recomputes the kernel spectrum on
// every call.  Same semantics (causal correlation with the stored flipped kernel, output length
// T+l+r-K+1); different framing: the block is a power of two chosen for rocFFT on MI355X instead
// of int(5*K), the kernel spectrum (pre-conjugated, pre-scaled by 1/N) is cached per filter, and
// the frames are processed in channel slabs so the workspace stays bounded.
//
//   frame f of row c :  fr[i] = xp[c, f*S + i],  xp = x padded (l, r),   i < N,  S = N-K+1
//   Z = rfft(fr) ;  Z *= conj(rfft(kf_pad)) / N ;  o = irfft(Z) ;  y[c, f*S + i] = o[i], i < S
#include "common.h"
#include "epilogue.h"
#include "ols_route.h"
#include "plan_cache.h"
#include "sos.h"
#include "../../include/torchfx_hip.h"

#include <rocfft/rocfft.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <map>
#include <mutex>
#include <vector>

namespace tfx {

#define TFX_ROCFFT(expr)                                                                     \
    do {                                                                                     \
        rocfft_status _s = (expr);                                                           \
        TFX_CHECK(_s == rocfft_status_success, "rocFFT error %d at %s:%d (%s)", (int)_s,     \
                  __FILE__, __LINE__, #expr);                                                \
    } while (0)

// ---- frame: zero-padded gather of overlapping blocks ---------------------------------------
// one thread = 4 consecutive samples of one frame; N % 4 == 0
template <typename T>
__global__ void __launch_bounds__(256)
ols_frame_kernel(const T *__restrict__ x, T *__restrict__ fr, int64_t Tn, int64_t c0, int64_t F,
                 int64_t N, int64_t S, int64_t pad_left, int64_t total4, const T *__restrict__ hist, int64_t H)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total4) return;
    const int64_t n4 = N / 4;
    const int64_t b = g / n4;            // frame index within the slab
    const int64_t i = (g - b * n4) * 4;
    const int64_t c = c0 + b / F, f = b % F;
    const int64_t m = f * S + i - pad_left;     // index into x[c, :]
    const T *xr = x + c * Tn;
    T v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t mm = m + e;
        v[e] = (mm >= 0 && mm < Tn) ? xr[mm] : ((hist && mm < 0 && mm >= -H) ? hist[c * H + H + mm] : (T)0);
    }
    T *dst = fr + b * N + i;
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e] = v[e];
}

// ---- spectrum multiply: Z[b,k] *= H[k]  (H already conjugated and scaled) -------------------
template <typename T2>
__global__ void __launch_bounds__(256)
ols_cmul_kernel(T2 *__restrict__ z, const T2 *__restrict__ h, int64_t bins, int64_t total)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int64_t k = g % bins;
    const T2 a = z[g], w = h[k];
    T2 o;
    o.x = a.x * w.x - a.y * w.y;
    o.y = a.x * w.y + a.y * w.x;
    z[g] = o;
}

// ---- un-frame: keep the first S samples of every block ---------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
ols_unframe_kernel(const T *__restrict__ fr, T *__restrict__ y, int64_t Tout, int64_t c0, int64_t F,
                   int64_t N, int64_t S, int64_t total)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;                      // total = nb * S
    const int64_t b = g / S, i = g - b * S;
    const int64_t c = c0 + b / F, f = b % F;
    const int64_t n = f * S + i;
    if (n < Tout) y[c * Tout + n] = fr[b * N + i];
}

// ---- plans -------------------------------------------------------------------------------------
struct FftKey {
    int dev, dtype;
    int64_t N, batch;
    bool operator<(const FftKey &o) const
    {
        if (dev != o.dev) return dev < o.dev;
        if (dtype != o.dtype) return dtype < o.dtype;
        if (N != o.N) return N < o.N;
        return batch < o.batch;
    }
};
struct FftPlan {
    rocfft_plan fwd = nullptr, inv = nullptr;
    size_t work_bytes = 0;
};

static std::mutex g_fft_mu;
static bool g_rocfft_up = false;
static std::map<FftKey, FftPlan> g_fft_plans;
static PlanCache<DeviceBuffer, 2> g_specs(64);                   // tail: dtype, N
static PlanCache<int64_t, 1> g_warmups(256);                     // fused_warmup; tail: bits

static FftPlan &get_fft_plan(int dtype, int64_t N, int64_t batch)
{
    if (!g_rocfft_up) {
        TFX_ROCFFT(rocfft_setup());
        g_rocfft_up = true;
    }
    FftKey key{current_device(), dtype, N, batch};
    auto it = g_fft_plans.find(key);
    if (it != g_fft_plans.end()) return it->second;
    FftPlan pl;
    const size_t len[1] = {(size_t)N};
    const rocfft_precision pr = dtype == TFX_F32 ? rocfft_precision_single : rocfft_precision_double;
    TFX_ROCFFT(rocfft_plan_create(&pl.fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                                  pr, 1, len, (size_t)batch, nullptr));
    TFX_ROCFFT(rocfft_plan_create(&pl.inv, rocfft_placement_notinplace, rocfft_transform_type_real_inverse,
                                  pr, 1, len, (size_t)batch, nullptr));
    size_t w1 = 0, w2 = 0;
    TFX_ROCFFT(rocfft_plan_get_work_buffer_size(pl.fwd, &w1));
    TFX_ROCFFT(rocfft_plan_get_work_buffer_size(pl.inv, &w2));
    pl.work_bytes = w1 > w2 ? w1 : w2;
    return g_fft_plans.emplace(key, pl).first->second;
}

static void exec_fft(rocfft_plan plan, void *in, void *out, void *work, size_t work_bytes, hipStream_t stream)
{
    rocfft_execution_info info = nullptr;
    TFX_ROCFFT(rocfft_execution_info_create(&info));
    TFX_ROCFFT(rocfft_execution_info_set_stream(info, stream));
    if (work_bytes) TFX_ROCFFT(rocfft_execution_info_set_work_buffer(info, work, work_bytes));
    void *ib[1] = {in}, *ob[1] = {out};
    rocfft_status st = rocfft_execute(plan, ib, ob, info);
    rocfft_execution_info_destroy(info);
    TFX_CHECK(st == rocfft_status_success, "rocfft_execute failed (%d)", (int)st);
}

template <typename T, typename T2>
static std::shared_ptr<DeviceBuffer> get_spectrum(int dtype, const void *kernel_host, int64_t K, int64_t N, hipStream_t stream)
{
    return g_specs.get(kernel_host, (size_t)K * sizeof(T), {dtype, N}, stream, [&] {
        // one-time per (filter, N): pad taps, forward transform, conjugate + scale.  Blocking.
        const int64_t bins = N / 2 + 1;
        std::vector<T> hp((size_t)N, (T)0);
        memcpy(hp.data(), kernel_host, (size_t)K * sizeof(T));
        const DeviceBuffer dpad(hp);
        auto dspec = std::make_shared<DeviceBuffer>(nullptr, (size_t)bins * sizeof(T2));
        FftPlan &p1 = get_fft_plan(dtype, N, 1);
        const DeviceBuffer work(nullptr, p1.work_bytes);
        exec_fft(p1.fwd, dpad.p, dspec->p, work.p, p1.work_bytes, stream);
        TFX_HIP(hipStreamSynchronize(stream));
        std::vector<T2> hs((size_t)bins);
        TFX_HIP(hipMemcpy(hs.data(), dspec->p, (size_t)bins * sizeof(T2), hipMemcpyDeviceToHost));
        const T sc = (T)1 / (T)N;
        for (auto &v : hs) { v.x = v.x * sc; v.y = -v.y * sc; }        // conj(.)/N  (_fftconv.py:131)
        TFX_HIP(hipMemcpy(dspec->p, hs.data(), (size_t)bins * sizeof(T2), hipMemcpyHostToDevice));
        return dspec;
    });
}

void fftconv_clear()
{
    g_specs.clear();
    g_warmups.clear();
    std::lock_guard<std::mutex> lk(g_fft_mu);
    for (auto &kv : g_fft_plans) {
        if (kv.second.fwd) rocfft_plan_destroy(kv.second.fwd);
        if (kv.second.inv) rocfft_plan_destroy(kv.second.inv);
    }
    g_fft_plans.clear();
}


int64_t fftconv_block_size(int64_t K, int64_t L)
{
    // power of two >= 4K (>= 75 % of each block is valid output), at least 4096, but no larger
    // than needed for the whole (padded) signal in one block
    int64_t n = 4096;
    while (n < 4 * K) n <<= 1;
    const int64_t lg = env_i64("TFX_FFT_LOG2N", 0);
    if (lg > 0) { n = (int64_t)1 << lg; while (n < 2 * K) n <<= 1; }
    int64_t cap = 8;
    while (cap < L) cap <<= 1;            // one block covers everything
    if (n > cap) n = cap;
    while (n < K) n <<= 1;
    return n;
}

template <typename T, typename T2>
static void fft_conv_typed(const T *x, T *y, int dtype, int64_t C, int64_t Tn, const void *kernel_host,
                           int64_t K, int64_t pl, int64_t pr, const OlsRoute &r, hipStream_t stream, const T *hist, int64_t Hlen)
{
    const int64_t Tout = Tn + pl + pr - K + 1;
    const int64_t N = r.N, S = r.S, F = r.F;
    const int64_t bins = N / 2 + 1;

    std::lock_guard<std::mutex> lk(g_fft_mu);
    const std::shared_ptr<DeviceBuffer> spec = get_spectrum<T, T2>(dtype, kernel_host, K, N, stream);
    const T2 *H = (const T2 *)spec->p;

    // channel slab so that frames + spectra stay within the workspace budget
    const int64_t ws_mb = env_i64("TFX_FFT_WS_MB", 2048);
    const int64_t per_ch = F * (N * (int64_t)sizeof(T) + bins * (int64_t)sizeof(T2));
    int64_t cps = (ws_mb << 20) / per_ch;
    if (cps < 1) cps = 1;
    if (cps > C) cps = C;

    T *fr = (T *)scratch(dtype == TFX_F32 ? "ols_frames32" : "ols_frames64", (size_t)(cps * F * N) * sizeof(T), stream);
    T2 *zs = (T2 *)scratch(dtype == TFX_F32 ? "ols_spec32" : "ols_spec64", (size_t)(cps * F * bins) * sizeof(T2), stream);

    for (int64_t c0 = 0; c0 < C; c0 += cps) {
        const int64_t nc = (C - c0 < cps) ? (C - c0) : cps;
        const int64_t nb = nc * F;
        FftPlan &plan = get_fft_plan(dtype, N, nb);
        void *work = plan.work_bytes ? scratch("ols_work", plan.work_bytes, stream) : nullptr;
        {
            const int64_t total4 = nb * (N / 4);
            ProfScope ps("ols_frame_kernel", stream);
            hipLaunchKernelGGL(ols_frame_kernel<T>, dim3((unsigned)ceil_div(total4, 256)), dim3(256), 0, stream,
                               x, fr, Tn, c0, F, N, S, pl, total4, hist, Hlen);
            TFX_HIP(hipGetLastError());
        }
        {
            ProfScope ps("rocfft_r2c", stream);
            exec_fft(plan.fwd, fr, zs, work, plan.work_bytes, stream);
        }
        {
            const int64_t total = nb * bins;
            ProfScope ps("ols_cmul_kernel", stream);
            hipLaunchKernelGGL(ols_cmul_kernel<T2>, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, stream,
                               zs, H, bins, total);
            TFX_HIP(hipGetLastError());
        }
        {
            ProfScope ps("rocfft_c2r", stream);
            exec_fft(plan.inv, zs, fr, work, plan.work_bytes, stream);
        }
        {
            const int64_t total = nb * S;
            ProfScope ps("ols_unframe_kernel", stream);
            hipLaunchKernelGGL(ols_unframe_kernel<T>, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, stream,
                               fr, y, Tout, c0, F, N, S, total);
            TFX_HIP(hipGetLastError());
        }
    }
}

// hist (streaming): [C, H] samples that precede each row, x[-H .. -1], H <= pad_left: they replace the zeros of
// the left padding
void fft_conv_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, const void *kernel_host,
                      int64_t K, int64_t pad_left, int64_t pad_right, hipStream_t stream, const void *hist, int64_t H,
                      const Epilogue *ep)
{
    TFX_CHECK(!ep || ep->stat_mode < 0 || ep->stat_out, "fft_conv_forward: statistic requested without an output buffer");
    TFX_CHECK(H >= 0 && H <= pad_left && (H == 0 || hist), "fft_conv_forward: bad history");
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "fft_conv_forward: bad dtype %d", dtype);
    TFX_CHECK(K >= 1 && pad_left >= 0 && pad_right >= 0, "fft_conv_forward: bad sizes");
    const int64_t L = T + pad_left + pad_right;
    // same condition and wording as _fftconv.py:111-115
    TFX_CHECK(L >= K, "Input should be at least as large as the kernel size %lld, but it is only %lld samples long.",
              (long long)K, (long long)L);
    if (C == 0) return;
    TFX_CHECK(C > 0 && T >= 0, "fft_conv_forward: negative size");
    TFX_CHECK(y && kernel_host && (x || T == 0), "fft_conv_forward: null pointer");
    olsnative_wait_warm();               // a set-up helper started by tfx_prewarm finishes before anything here is enqueued
    const OlsRoute r = ols_route(K, T, pad_left, pad_right, dtype, hist != nullptr, ols_sh_base(x, dtype == TFX_F32 ? 4 : 8));
    const Epilogue *fused_ep = (ep && ep->any()) ? ep : nullptr;
    if (r.path == OLS_PATH_LDS)          // kernels that fit on chip: no workspace, epilogue in the store of the inverse transform
        return olslds_forward(x, y, dtype, C, T, kernel_host, K, pad_left, pad_right, r, stream, hist, H, fused_ep);
    if (r.path == OLS_PATH_PASSES && dtype == TFX_F32)     // the epilogue in the last pass (the store of the inverse column FFT)
        return olsnative_forward((const float *)x, (float *)y, C, T, (const float *)kernel_host, K, pad_left, pad_right, r, stream,
                                 (const float *)hist, H, fused_ep);
    if (r.path == OLS_PATH_PASSES)       // float64 beyond the one-launch kernels' 4096 taps (olsnative64.hip)
        olsnative64_forward((const double *)x, (double *)y, C, T, (const double *)kernel_host, K, pad_left, pad_right, r, stream);
    else if (dtype == TFX_F32)
        fft_conv_typed<float, float2>((const float *)x, (float *)y, dtype, C, T, kernel_host, K, pad_left, pad_right, r, stream,
                                      (const float *)hist, H);
    else
        fft_conv_typed<double, double2>((const double *)x, (double *)y, dtype, C, T, kernel_host, K, pad_left, pad_right, r, stream,
                                        (const double *)hist, H);
    if (fused_ep) epilogue_as_passes(y, dtype, C, L - K + 1, *ep, stream);     // float64 three-pass and rocFFT: separate passes
}

OlsRoute ols_route(int64_t K, int64_t Tn, int64_t pl, int64_t pr, int dtype, bool has_hist, int sh_base)
{
    const int64_t L = Tn + pl + pr;
    OlsRoute r;
    if (olslds_supported(K, dtype, L, &r.N, &r.lds_kind)) {
        r.path = OLS_PATH_LDS;
        olslds_geometry(K, Tn, pl, pr, dtype, r);
    } else if (dtype == TFX_F32 && olsnative_supported(K, L, &r.N)) {
        r.path = OLS_PATH_PASSES;
        olsnative_geometry(K, Tn, pl, pr, sh_base, r);
    } else if (dtype == TFX_F64 && olsnative64_supported(K, L, has_hist, &r.N)) {
        r.path = OLS_PATH_PASSES;
        olsnative64_geometry(K, Tn, pl, pr, sh_base, r);
    } else {
        r.N = fftconv_block_size(K, L);
        r.S = r.N - K + 1;
        r.F = ceil_div(L - K + 1, r.S);
    }
    return r;
}

// `iir-cascade | FIR` as ONE overlap-save pipeline in the reference's arithmetic: the zero-state float64 cascade
// (_ops.py:119-176 with state None -> iir_cpu.cpp:64-159), its result rounded to float32 (iir.py:84-184, the downcast), then
// fft_conv1d (_fftconv.py:70-141) -- the cascade runs inside the forward column pass (olsnative.hip), no pass of its own.
// Warm-up of a row's recursion inside the column pass: the state a row starts from is the true one to 2^-bits of the
// state's scale (40 bits = 9e-13: 1/20 of the 2e-11 the section-by-section parity tests state
// (tests/gpu_common.py TOL_IIR_F64OUT) and 5 orders below the float32 rounding the samples get next; round 5 ran 48, 3.6e-15:
// +0.15 ms per chain step for digits no test can read, profiles/r05_experiments.txt section 6; the stand-alone cascade kernel
// uses 60).  Cached by coefficient content: the analysis is a few dozen
// long-double matrix products.
static int64_t fused_warmup(const double *sos_host, int64_t Ksos)
{
    constexpr int bits = 40;
    return *g_warmups.get(sos_host, (size_t)(6 * Ksos) * sizeof(double), {bits}, nullptr,
                          [&] { return std::make_shared<int64_t>(sos_warmup_bits(sos_host, Ksos, bits)); });
}

int64_t sos_fft_conv_warmup(const double *sos_host, int64_t Ksos) { return (Ksos >= 1 && Ksos <= OLS_SOS_MAXK) ? fused_warmup(sos_host, Ksos) : -1; }

// The cascade-in-pass-A route: 4096- or 8192-point rows of the three-pass pipeline, a cascade of at most OLS_SOS_MAXK
// sections whose warm-up fits a row.  `force`: 1 / 2 = the 2^20 / 2^21-point block even for rows shorter than one block
// (tests at fixture size; a one-frame launch).  False when this form does not serve the call, else its route and warm-up.
// At 2^21 points the route carries a tail geometry where a row's last frame fits a 2^20-point block (olsnative_tail_geometry).
static bool sos_fft_conv_route(int64_t T, const double *sos_host, int64_t Ksos, int64_t K, int64_t pl, int64_t pr, int force,
                               int sh_base, OlsRoute &r, int64_t &warm)
{
    if (Ksos < 1 || Ksos > OLS_SOS_MAXK || T <= 0 || K < 1) return false;
    warm = fused_warmup(sos_host, Ksos);
    const int64_t L = T + pl + pr;
    if (warm < 0 || warm > 4096 || L < K) return false;
    r.N = (int64_t)1 << (force == 2 ? 21 : 20);
    if (force) { if (r.N < 2 * (K + 32)) return false; }
    else {
        if (!olsnative_supported(K, L, &r.N) || (r.N != ((int64_t)1 << 20) && r.N != ((int64_t)1 << 21))) return false;
        // rows of 8192 samples (N = 2^21) halve the warm-up share of the recursion pass: 9.7 against 10.1 ms on the cfg-5 chain
        // (the plain pipeline is 5 % slower at 2^21 and stays at 2^20; profiles/r05_experiments.txt section 8)
        if (r.N == ((int64_t)1 << 20) && L >= ((int64_t)1 << 23) && 2 * (K + 32) <= ((int64_t)1 << 21))
            r.N = (int64_t)1 << 21;
    }
    r.path = OLS_PATH_PASSES;
    olsnative_geometry(K, T, pl, pr, sh_base, r);
    olsnative_tail_geometry(K, T, pl, pr, r);
    return true;
}

// block length, hop, frames per row, warm-up samples and the tail geometry's block and hop (0: none) the fused pipeline would
// use for x on a 128-byte line; false when it does not serve the geometry
bool sos_fft_conv_plan(int64_t T, const double *sos_host, int64_t Ksos, int64_t K, int64_t pad_left, int64_t pad_right, int force,
                       int64_t *N_out, int64_t *S_out, int64_t *F_out, int64_t *warm_out, int64_t *tail_N_out, int64_t *tail_S_out)
{
    OlsRoute r;
    int64_t warm = 0;
    if (!sos_fft_conv_route(T, sos_host, Ksos, K, pad_left, pad_right, force, 0, r, warm)) return false;
    if (N_out) *N_out = r.N;
    if (S_out) *S_out = r.S;
    if (F_out) *F_out = r.F;
    if (warm_out) *warm_out = warm;
    if (tail_N_out) *tail_N_out = r.tail_N;
    if (tail_S_out) *tail_S_out = r.tail_S;
    return true;
}

void sos_fft_conv_forward(const float *x, float *y, int64_t C, int64_t T, const double *sos_host, int64_t Ksos,
                          const float *kernel_host, int64_t K, int64_t pad_left, int64_t pad_right, double *sections, int force,
                          const Epilogue *ep, hipStream_t stream)
{
    TFX_CHECK(!ep || ep->stat_mode < 0 || ep->stat_out, "sos_fft_conv_forward: statistic requested without an output buffer");
    TFX_CHECK(K >= 1 && pad_left >= 0 && pad_right >= 0 && Ksos >= 1, "sos_fft_conv_forward: bad sizes");
    const int64_t L = T + pad_left + pad_right;
    TFX_CHECK(L >= K, "Input should be at least as large as the kernel size %lld, but it is only %lld samples long.",
              (long long)K, (long long)L);
    if (C == 0) return;
    TFX_CHECK(C > 0 && T > 0, "sos_fft_conv_forward: bad shape");
    TFX_CHECK(x && y && kernel_host && sos_host, "sos_fft_conv_forward: null pointer");
    TFX_CHECK(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0, "sos_fft_conv_forward: x and y must be float-aligned");
    olsnative_wait_warm();               // a set-up helper started by tfx_prewarm finishes before anything here is enqueued
    OlsRoute r;
    int64_t warm = -1;
    TFX_CHECK(sos_fft_conv_route(T, sos_host, Ksos, K, pad_left, pad_right, force, ols_sh_base(x, 4), r, warm),
              "sos_fft_conv_forward: unsupported here (at most 8 sections whose memory fades within 4096 samples, taps that take "
              "the 2^20-point block) -- ask tfx_sos_fft_conv_supported first");
    const SosFuseHost sf{sos_host, Ksos, warm, sections};
    olsnative_forward(x, y, C, T, kernel_host, K, pad_left, pad_right, r, stream, nullptr, 0, (ep && ep->any()) ? ep : nullptr, &sf);
}

}  // namespace tfx
