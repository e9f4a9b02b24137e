// sos.h -- what sos.hip exports to the library's other translation units (capi.hip, fftconv.hip, olsnative.hip).
// sos.hip includes it too, so every prototype here is compiled against its definition.
#pragma once

#include "common.h"
#include "epilogue.h"

namespace tfx {

// the fused K-section cascade; NB > 1 = filter bank, sum_bands = its `+` mode
void sos_forward(const void *x, int x_dtype, void *y, int y_dtype, int64_t C, int64_t T,
                 const double *sos_host, int64_t K, const double *sx_in, const double *sy_in,
                 double *sx_out, double *sy_out, void *y_sections, int precision, hipStream_t stream, int64_t NB = 1,
                 bool sum_bands = false, const Epilogue *ep = nullptr);
void sos_plan_info(const double *sos_host, int64_t K, int *precision, int64_t *warmup, double *err_bound);
void sos_refine_info(const double *sos_host, int64_t K, int *unit_form, int *refine_f32, int *refine_f64, double *errs);
void sos_route_info(int64_t C, int64_t T, const double *sos_host, int64_t K, int x_dtype, int y_dtype, int precision, int sections,
                    int64_t wave_slots, int *route, int64_t *nseg, int64_t *seg_len, int64_t *warm, int *passes, double *bytes_per_sample);
void sos_clear_plans();

// zero-phase filtering (scipy.signal.sosfiltfilt along each row)
int64_t sos_filtfilt_default_padlen(const double *sos_host, int64_t K);
void sos_filtfilt_forward(const void *x, int x_dtype, void *y, int y_dtype, int64_t C, int64_t T, const double *sos_host, int64_t K,
                          int padtype, int64_t padlen, double *work, hipStream_t stream);
void sos_filtfilt_plan_info(int64_t C, int64_t T, const double *sos_host, int64_t K, int padtype, int64_t padlen,
                            int64_t *default_padlen, int64_t *padlen_used, int64_t *work_elems, int64_t *warmup,
                            int *nseg_forward, int *nseg_reverse);

// block energies of the cascade's output (BS.1770 measuring pass)
void sos_block_energy_forward(const void *x, int x_dtype, double *s, int64_t C, int64_t T, const double *sos_host, int64_t K,
                              int64_t num, int64_t den, hipStream_t stream);
void sos_block_energy_plan_info(int64_t C, int64_t T, const double *sos_host, int64_t K, int64_t num, int64_t den,
                                int64_t *nblk, int *nseg, int64_t *warm);

// one launch per small streaming chunk: cascade -> direct FIR with carried history -> gain / clip
bool chunk_supported(int64_t C, int64_t T, int64_t K, int64_t Kf);
void chunk_forward(const float *x, int64_t x_pitch, float *y, int64_t C, int64_t T, const double *sos_host, int64_t K,
                   const double *sx_in, const double *sy_in, double *sx_out, double *sy_out,
                   const float *taps_host, int64_t Kf, const float *hist_in, float *hist_out,
                   double gain, int scale, int clamp, int precision, hipStream_t stream);

// for the cascade inside the overlap-save passes: the warm-up for max|A^W| < 2^-bits (-1: none), and the unit-b0 form of a
// cascade -- rows [G_s = b0_0 ... b0_s, b1 / b0, b2 / b0, -a1, -a2] -- or false when the cascade has no such form
int64_t sos_warmup_bits(const double *sos_host, int64_t K, int bits);
bool sos_unit_rows(const double *sos_host, int64_t K, double (*rows)[5]);

}  // namespace tfx
