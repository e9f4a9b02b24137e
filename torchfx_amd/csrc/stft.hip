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
// The stages, the exchange and the tables are stft_frame.h's, shared with the inverse (istft.hip); so are the kernel's front
// (stft_frames: loads, staged span, window product, transform), the bin and power expressions and the plan, which the mel
// spectrogram (mel.hip) runs too, so that its power spectrum has this kernel's bits.
#include "stft_frame.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <cmath>

namespace tfx {

PlanCache<DeviceBuffer, 2> g_stft_tables(16, "stft_forward");

namespace {

template <typename R, int M, int THREADS>
__global__ __launch_bounds__(THREADS, sizeof(R) == 4 ? 2 : 1) void stft_kernel(const StftArgs<R> p)
{
    constexpr int TPF = M / 16, G = THREADS / TPF, FS = M + M / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char stft_smem[];
    const int tid = (int)threadIdx.x;
    const int64_t grp = blockIdx.x, row = grp / p.groups_per_row, f0 = (grp - row * p.groups_per_row) * G;
    stft_frames<R, M, THREADS>(p, stft_smem, row, f0, [] {}, [] {});

    const cx<R> *post = (const cx<R> *)stft_smem;                      // W_n^k by now
    const cx<R> *work = post + M + M;                                   // behind W and the window's n_fft reals
    const int64_t left = p.frames - f0;
    const int total = (int)(left < G ? left : G) * (M + 1);
    const int64_t o0 = (row * p.frames + f0) * (M + 1);
    for (int idx = tid; idx < total; idx += THREADS) {
        const int f = idx / (M + 1), k = idx - f * (M + 1);
        const cx<R> X = stft_bin<R, M>(work + f * FS, post, k, p);
        if (p.power == STFT_POWER_COMPLEX) ((cx<R> *)p.out)[o0 + idx] = X;
        else ((R *)p.out)[o0 + idx] = stft_power(X, p.power);
    }
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
    const StftArgs<R> p = stft_args<R>(x, window, (const cx<R> *)tab->p, out, T, n_fft, hop, win_length, pad, pad_mode, power, normalized, pl);
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
