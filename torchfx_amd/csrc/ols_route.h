// ols_route.h -- host-only: which overlap-save pipeline serves an FFT-mode FIR call, its block N and its frame geometry (lead
// zero taps in front of the flipped kernel, hop S, frames per row F).  fft_conv_forward acts on ols_route(); tfx_ols_plan_info(2)
// report it for no history and sh_base = 0; the cascade form resolves its own in one helper (fftconv.hip).  Nothing else calls
// the pipelines' supported / geometry functions.  F of a query is the frame count for a base pointer on a 128-byte line: the
// three-pass pipelines shift a row's frame grid onto lines of memory (sh_on), so a view that starts inside a line can take one more.
#pragma once
#include "common.h"
#include "epilogue.h"

#include <vector>

namespace tfx {

enum { OLS_PATH_ROCFFT = 0, OLS_PATH_PASSES = 1, OLS_PATH_LDS = 2 };      // tfx_ols_plan_info2's *path codes

struct OlsRoute {
    int path = OLS_PATH_ROCFFT;
    int lds_kind = -1;          // one-launch kernel: 0 = 4096 points, 1 = 8192, 2 = 16 384 (1024-thread), 3 = 16 384 (w8)
    int64_t N = 0, lead = 0, S = 0, F = 0;
    int sh_base = 0, sh_on = 0; // three-pass: element offset of x in its 128-byte line; row frame grids shifted
    int64_t tail_N = 0, tail_S = 0;   // cascade route: block and hop of the tail geometry (the last of a row's F frames runs at this
                                      // smaller block, the F - 1 before it at N), or 0: all F frames at N  (olsnative_tail_geometry)
};

inline int ols_sh_base(const void *x, int elem_bytes) { return (int)(((uintptr_t)x & 127) / elem_bytes); }

// fftconv.hip
OlsRoute ols_route(int64_t K, int64_t Tn, int64_t pl, int64_t pr, int dtype, bool has_hist, int sh_base);
int64_t fftconv_block_size(int64_t K, int64_t L);           // the rocFFT path's block
void fft_conv_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, const void *kernel_host,
                      int64_t K, int64_t pad_left, int64_t pad_right, hipStream_t stream, const void *hist = nullptr,
                      int64_t H = 0, const Epilogue *ep = nullptr);
void fftconv_clear();
constexpr int OLS_SOS_MAXK = 8;                              // cascade sections the column pass holds (SOSF_MAXK)
int64_t sos_fft_conv_warmup(const double *sos_host, int64_t Ksos);
bool sos_fft_conv_plan(int64_t T, const double *sos_host, int64_t Ksos, int64_t K, int64_t pad_left, int64_t pad_right, int force,
                       int64_t *N_out, int64_t *S_out, int64_t *F_out, int64_t *warm_out, int64_t *tail_N_out = nullptr,
                       int64_t *tail_S_out = nullptr);
void sos_fft_conv_forward(const float *x, float *y, int64_t C, int64_t T, const double *sos_host, int64_t Ksos,
                          const float *kernel_host, int64_t K, int64_t pad_left, int64_t pad_right, double *sections, int force,
                          const Epilogue *ep, hipStream_t stream);

// olslds.hip: one launch, the whole transform of a block in LDS; the geometry functions below fill lead, S, F (and sh_*)
bool olslds_supported(int64_t K, int dtype, int64_t L, int64_t *N_out, int *kind_out);
void olslds_geometry(int64_t K, int64_t Tn, int64_t pl, int64_t pr, int dtype, OlsRoute &r);
void olslds_forward(const void *x, void *y, int dtype, int64_t C, int64_t Tn, const void *kf_host, int64_t K,
                    int64_t pl, int64_t pr, const OlsRoute &r, hipStream_t stream, const void *hist, int64_t H, const Epilogue *ep);
void olslds_clear();

// olsnative.hip: the three-pass pipeline in float32
bool olsnative_supported(int64_t K, int64_t L, int64_t *N_out);
void olsnative_geometry(int64_t K, int64_t Tn, int64_t pl, int64_t pr, int sh_base, OlsRoute &r);
void olsnative_tail_geometry(int64_t K, int64_t Tn, int64_t pl, int64_t pr, OlsRoute &r);   // after olsnative_geometry: fills tail_N, tail_S
void olsnative_forward(const float *x, float *y, int64_t C, int64_t Tn, const float *kf_host, int64_t K, int64_t pl, int64_t pr,
                       const OlsRoute &r, hipStream_t stream, const float *hist, int64_t H, const Epilogue *ep,
                       const SosFuseHost *sosf = nullptr);
void olsnative_prewarm();
void olsnative_wait_warm();
void olsnative_clear();
void host_fft_f64(std::vector<double> &re, std::vector<double> &im);      // in-place host FFT: the spectra olslds.hip and olsnative64.hip upload

// olsnative64.hip: the three-pass pipeline in float64
bool olsnative64_supported(int64_t K, int64_t L, bool has_hist, int64_t *N_out);
void olsnative64_geometry(int64_t K, int64_t Tn, int64_t pl, int64_t pr, int sh_base, OlsRoute &r);
void olsnative64_forward(const double *x, double *y, int64_t C, int64_t Tn, const double *kf_host, int64_t K, int64_t pl, int64_t pr,
                         const OlsRoute &r, hipStream_t stream);
void olsnative64_clear();

}  // namespace tfx
