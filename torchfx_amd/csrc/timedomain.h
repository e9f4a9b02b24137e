// timedomain.h -- the host entry points of the time-domain and elementwise ops, one prototype per exported function of fir.hip,
// effects.hip, select.hip, delay.hip, resample.hip, limiter.hip, compressor.hip, modulation.hip, reverb.hip, waveshaper.hip, phaser.hip, gate.hip, stft.hip, istft.hip and layout.hip (the cascade's: sos.h; the
// overlap-save pipelines': ols_route.h).  Included by the file that defines each function and by capi.hip, so a prototype that drifts from
// its definition does not compile; default arguments live here and nowhere else.  Every *_forward checks its arguments before
// anything touches the device; a *_plan_info takes the same checking path without the pointers.
#pragma once
#include "common.h"

namespace tfx {

struct Epilogue;                 // epilogue.h

// ---- fir.hip ----
void fir_direct_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, const void *kernel_host, int64_t K,
                        hipStream_t stream, const void *hist = nullptr, int64_t H = 0);
void fir_hist_update(const void *x, const void *hist_in, void *hist_out, int dtype, int64_t C, int64_t T, int64_t H,
                     hipStream_t stream);
// one chunk of a stateful FIR (tfx_fir_stream_forward): direct form or overlap-save (ols_route.h), then the new history
void fir_stream_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, const void *kernel_host, int64_t K, int direct,
                        const void *hist_in, void *hist_out, hipStream_t stream);
void fir_clear();

// ---- effects.hip ----
void gain_forward(const void *x, void *y, int dtype, int64_t n, double gain, int clamp, hipStream_t stream);
void stat_forward(const void *x, int dtype, int64_t C, int64_t T, int mode, int per_row, double *out_dev, hipStream_t stream);
void normalize_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, int mode, int per_row, double peak,
                       hipStream_t stream);
void normalize_apply_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, int mode, int per_row, double peak,
                             const double *stat, hipStream_t stream);
void sum_forward(const void *const *xs_host, int n, void *y, int dtype, int64_t numel, hipStream_t stream);
void delay_line_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, int64_t delay, double coeff,
                        hipStream_t stream);
void delay_line_stream_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, int64_t delay, double coeff,
                               const void *hist_in, void *hist_out, hipStream_t stream);
void effects_plan_info(int64_t T, int dtype, int64_t *vec, int64_t *tile, int64_t *group, int64_t *groups, int64_t *finish_threads,
                       int64_t *stream_tile);

// ---- select.hip ----
void quantile_abs_forward(const float *x, int64_t n, double q, double *out_dev, hipStream_t stream);

// ---- delay.hip ----
void delay_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t delay, int64_t taps,
                   const double *amps_host, double mix, int pingpong, const Epilogue *ep, hipStream_t stream);
void delay_stream_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t delay, int64_t taps,
                          const double *amps_host, double mix, int pingpong, const void *hist_in, void *hist_out, hipStream_t stream);
int delay_regime(int64_t D, int64_t taps, int esz, int pingpong);
// the geometry of one delay_forward launch (host-only; delay_launch fills its kernel arguments from it)
struct DelayPlan {
    int regime;
    int64_t units;              // rows (GATHER) or rows / pairs (SPAN, LATTICE)
    int64_t tiles;              // SPAN / GATHER: output tiles per row;  LATTICE: residue blocks per row
    int64_t kc, nchunks;        // LATTICE: k steps per chunk, chunks per residue block;  0 otherwise
    int64_t groups;             // workgroups per unit
    int64_t nwg;                // workgroups in the grid (0: nothing is launched)
    int64_t lds_bytes;          // SPAN: dynamic LDS per workgroup;  0 otherwise
};
DelayPlan delay_plan(int64_t rows, int64_t T, int64_t D, int64_t taps, int esz, int pingpong);
void delay_tiling_info(int64_t rows, int64_t T, int64_t delay, int64_t taps, int dtype, int pingpong, int *regime, int64_t *units,
                       int64_t *tiles, int64_t *kc, int64_t *nchunks, int64_t *groups, int64_t *nwg, int64_t *lds_bytes);
void delay_clear();

// ---- resample.hip (the polyphase table its users share: polyphase.h) ----
void resample_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t up, int64_t down, const void *taps_host,
                      int64_t nh, hipStream_t stream);
void resample_plan_info(int64_t T, int64_t up, int64_t down, int64_t nh, int dtype, int64_t *n_out, int64_t *pre_remove,
                        int64_t *padded, int64_t *Lp, int *kernel, int64_t *lds_bytes);
void resample_tiling_info(int64_t T, int64_t up, int64_t down, int64_t nh, int dtype, int *kernel, int64_t *G, int64_t *G_initial,
                          int64_t *E, int64_t *tile_out, int64_t *span, int64_t *LP, int64_t *tiles);
void resample_stream_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t up, int64_t down,
                             const void *taps_host, int64_t nh, int64_t consumed, const void *hist_in, void *hist_out,
                             hipStream_t stream);
void resample_stream_plan_info(int64_t consumed, int64_t T, int64_t up, int64_t down, int64_t nh, int dtype, int64_t *out_begin,
                               int64_t *out_end, int64_t *hist_len, int64_t *pre_remove, int64_t *Lp, int *kernel,
                               int64_t *lds_bytes);
void true_peak_forward(const void *x, int dtype, void *peak, int64_t rows, int64_t T, int64_t up, const void *taps_host, int64_t nh,
                       void *work, hipStream_t stream);
void true_peak_plan_info(int64_t rows, int64_t T, int64_t up, int64_t nh, int dtype, int64_t *Lp, int64_t *tile_in, int64_t *tiles,
                         int64_t *work_elems);
void resample_clear();

// ---- limiter.hip ----
void limiter_forward(const void *x, void *y, void *gain, int dtype, int64_t groups, int64_t channels, int64_t T, double c,
                     int64_t A, int64_t H, const void *window_host, int64_t up, const void *taps_host, int64_t nh,
                     hipStream_t stream);
void limiter_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t A, int64_t H, int64_t up, int64_t nh, int dtype,
                       int64_t *tile, int64_t *tiles, int64_t *halo_left, int64_t *halo_right, int64_t *Lp, int64_t *lds_bytes);
void limiter_stream_forward(const void *x, void *y, void *gain, int dtype, int64_t groups, int64_t channels, int64_t T, int64_t n_in,
                            int64_t consumed, double c, int64_t A, int64_t H, const void *window_host, int64_t up,
                            const void *taps_host, int64_t nh, const void *hist_in, void *hist_out, hipStream_t stream);
void limiter_stream_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t A, int64_t H, int64_t up, int64_t nh, int dtype,
                              int64_t *latency, int64_t *history, int64_t *tile, int64_t *tiles, int64_t *positions,
                              int64_t *lds_bytes);
void limiter_clear();

// ---- compressor.hip ----
void compressor_forward(const void *x, void *y, void *gain, int dtype, int64_t groups, int64_t channels, int64_t T, double th,
                        double s, double w, double alpha_a, double alpha_r, double makeup_db, const double *state_in,
                        double *state_out, int64_t segments, void *scratch, hipStream_t stream);
void compressor_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t segments, int64_t *tile, int64_t *tiles,
                          int64_t *segments_out, int64_t *seg_tiles, int64_t *scratch_bytes);

// ---- modulation.hip ----
void modulated_delay_forward(const void *x, void *y, int dtype, int64_t batch, int64_t channels, int64_t T, const double *voices_host,
                             int64_t V, double spread, double dry, int shape, int interp, int64_t position, hipStream_t stream);
void modulated_delay_stream_forward(const void *x, void *y, int dtype, int64_t batch, int64_t channels, int64_t T,
                                    const double *voices_host, int64_t V, double spread, double dry, int shape, int interp,
                                    const void *hist_in, void *hist_out, const int64_t *pos_in, int64_t *pos_out, hipStream_t stream);
void modulated_delay_plan_info(int64_t batch, int64_t channels, int64_t T, const double *voices_host, int64_t V, int interp,
                               int64_t *tile, int64_t *tiles, int64_t *history, int64_t *batch_items, int64_t *batch_groups);
void modulation_clear();

// ---- reverb.hip ----
void freeverb_forward(const void *x, void *y, int dtype, int64_t batch, int64_t channels, int64_t T, int64_t tail,
                      const int64_t *comb_delays_host, int64_t NC, const int64_t *allpass_delays_host, int64_t NA, double feedback,
                      double damp, double allpass_gain, double input_gain, double dry_gain, double wet1, double wet2,
                      const double *state_in, double *state_out, void *workspace, hipStream_t stream);
void freeverb_plan_info(int64_t batch, int64_t channels, int64_t T, int64_t tail, const int64_t *comb_delays_host, int64_t NC,
                        const int64_t *allpass_delays_host, int64_t NA, double wet2, int64_t *block, int *placement,
                        int64_t *state_len, int64_t *launches, int64_t *workspace_bytes);

// ---- waveshaper.hip ----
void waveshaper_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t oversample, int shape,
                        const void *curve_host, int64_t curve_n, double drive, double bias, double dry, double wet,
                        const void *taps_up_host, int64_t nh_up, const void *taps_dn_host, int64_t nh_dn, hipStream_t stream);
void waveshaper_plan_info(int64_t rows, int64_t T, int64_t oversample, int64_t nh_up, int64_t nh_dn, int64_t curve_n, int dtype,
                          int64_t *tile, int64_t *tiles, int64_t *reach_before, int64_t *reach_after, int64_t *lds_bytes,
                          int64_t *taps_up, int64_t *taps_dn);
void waveshaper_stream_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t n_in, int64_t consumed,
                               int64_t oversample, int shape, const void *curve_host, int64_t curve_n, double drive, double bias,
                               double dry, double wet, const void *taps_up_host, int64_t nh_up, const void *taps_dn_host,
                               int64_t nh_dn, const void *hist_in, void *hist_out, hipStream_t stream);
void waveshaper_stream_plan_info(int64_t rows, int64_t T, int64_t oversample, int64_t nh_up, int64_t nh_dn, int64_t curve_n, int dtype,
                                 int64_t *latency, int64_t *history, int64_t *tile, int64_t *tiles, int64_t *positions,
                                 int64_t *lds_bytes);
void waveshaper_clear();

// ---- phaser.hip ----
void phaser_forward(const void *x, void *y, double *coef, int dtype, int64_t rows, int64_t channels, int64_t T, int64_t stages, double fs,
                    double rate, double min_freq, double max_freq, double phase, double spread, double dry, double wet, int shape,
                    int64_t position, const int64_t *pos_in, int64_t *pos_out, const double *state_in, double *state_out,
                    int64_t segments, void *scratch, hipStream_t stream);
void phaser_plan_info(int64_t rows, int64_t channels, int64_t T, int64_t stages, int64_t segments, int64_t *tile, int64_t *tiles,
                      int64_t *segments_out, int64_t *seg_tiles, int64_t *scratch_bytes);

// ---- gate.hip ----
void gate_forward(const void *x, void *y, void *gain, unsigned char *open, int dtype, int64_t groups, int64_t channels, int64_t T,
                  double p_open, double p_close, double range, int64_t hold, double alpha_a, double alpha_r, const double *state_in,
                  double *state_out, int64_t segments, void *scratch, hipStream_t stream);
void gate_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t segments, int64_t *tile, int64_t *tiles,
                    int64_t *segments_out, int64_t *seg_tiles, int64_t *scratch_bytes);

// ---- stft.hip ----
void stft_forward(const void *x, const void *window, void *out, int dtype, int64_t rows, int64_t T, int64_t n_fft, int64_t hop,
                  int64_t win_length, int64_t pad, int pad_mode, int power, int normalized, hipStream_t stream);
void stft_plan_info(int64_t n_fft, int64_t hop, int64_t win_length, int64_t T, int64_t rows, int dtype, int center, int pad_mode,
                    int onesided, int *route, int64_t *frames, int64_t *frames_per_workgroup, int64_t *threads_per_frame,
                    int64_t *lds_bytes, int64_t *workgroups);
void stft_clear();

// ---- istft.hip ----
void istft_forward(const void *spec, const void *window, void *out, int *flag, int dtype, int64_t rows, int64_t frames, int64_t n_fft,
                   int64_t hop, int64_t win_length, int64_t pad, int64_t length, int normalized, hipStream_t stream);
void istft_plan_info(int64_t n_fft, int64_t hop, int64_t win_length, int64_t frames, int64_t rows, int dtype, int center, int64_t length,
                     int onesided, int *route, int64_t *out_length, int64_t *tile, int64_t *frames_per_batch, int64_t *threads_per_frame,
                     int64_t *lds_bytes, int64_t *workgroups, double *redundant_share);

// ---- layout.hip ----
void deinterleave_forward(const void *in, int in_kind, float *out, int64_t F, int64_t C, int64_t ld_out, int64_t f_base,
                          double scale, hipStream_t stream);
void interleave_forward(const float *in, float *out, int64_t F, int64_t C, int64_t ld_in, int64_t f_base,
                        hipStream_t stream);

}  // namespace tfx
