/*
 * torchfx_hip.h -- C ABI of libtorchfx_hip.so: the MI355X (gfx950) backend for
 * the torchfx.filter hot path.
 *
 * This is the drop-in boundary.  Every entry point takes plain device pointers,
 * sizes and a hipStream_t (as void*); no torch types.  Each one cites the
 * reference interface it replaces (paths relative to the reference repo,
 * matteospanio/torchfx v0.5.3).  The Python host side (torchfx_amd/torchfx_ext.py)
 * binds these with ctypes and re-exposes the reference's own names and
 * signatures (torchfx_ext.biquad_forward / sos_forward / delay_line_forward,
 * FIR.forward, fft_conv1d); INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - all signal buffers are DEVICE memory, row-major [C, T], time-minor,
 *     contiguous (row stride == T);
 *   - coefficient arrays marked HOST are read on the host during the call
 *     (they are O(K), like the reference's `sos_cpu` argument);
 *   - state buffers are DEVICE float64, layout identical to the reference
 *     ([K, C, 2] = {v[n-1], v[n-2]} per section and channel);
 *   - calls are asynchronous on `stream` (no host sync inside), outputs never
 *     alias inputs, inputs are never written;
 *   - return value: 0 = ok, non-zero = error; tfx_last_error() gives the text
 *     (thread-local).  The Python layer turns it into RuntimeError, as
 *     TORCH_CHECK does in the reference (binding.cpp:47,63,78).
 */
#ifndef TORCHFX_HIP_H
#define TORCHFX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *tfx_stream_t; /* hipStream_t */

enum tfx_dtype { TFX_F32 = 0, TFX_F64 = 1 };

/* Arithmetic used INSIDE the IIR kernel (I/O dtypes are independent of it).
 *   TFX_PREC_F64  : float64 recurrences -- what the reference does
 *                   (_ops.py:95,149; iir_cpu.cpp is all double).  Default.
 *   TFX_PREC_F32  : float32 recurrences, float64 only on the host tables.
 *   TFX_PREC_AUTO : F32 when a host-side worst-case error bound derived from
 *                   the SOS is below `TFX_AUTO_F32_BOUND`, else F64.
 */
enum tfx_precision { TFX_PREC_AUTO = 0, TFX_PREC_F32 = 1, TFX_PREC_F64 = 2 };

int tfx_version(void);
const char *tfx_last_error(void);

/* Device / build facts for reports: fills name[len] with the gfx arch string,
 * returns #CUs in *cus (either pointer may be NULL). */
int tfx_device_info(char *name, int len, int *cus);

/* ---------------------------------------------------------------------------
 * tfx_sos_forward -- fused K-section DF1 SOS cascade.
 *
 * Replaces  torchfx_ext.sos_forward(x, sos, sos_cpu, state_x, state_y)
 *           src/torchfx/_csrc/binding.cpp:52-66,88-91
 *           -> sos_forward_cpu  src/torchfx/_csrc/cpu/iir_cpu.cpp:64-159
 *           -> sos_forward_cuda src/torchfx/_csrc/cuda/biquad_forward.cu:49-92
 * and, with in/out dtype f32, also the casts around it
 *           x.to(float64)       src/torchfx/_ops.py:149
 *           out.to(x.dtype)     src/torchfx/filter/iir.py:176
 *
 *   x        DEVICE [C,T] of x_dtype
 *   y        DEVICE [C,T] of y_dtype (written)
 *   sos_host HOST   [K,6] float64 rows [b0,b1,b2,a0,a1,a2]; a0 ignored
 *            (iir_cpu.cpp:86) -- this is the reference's `sos_cpu` argument
 *   state_x_in / state_y_in   DEVICE [K,C,2] float64, or NULL for zeros
 *            (_ops.py:144-147)
 *   state_x_out / state_y_out DEVICE [K,C,2] float64 (written), may be NULL
 *   y_sections  optional DEVICE [K,C,T] of y_dtype: output of every section
 *            (section-by-section parity checks); NULL in production
 *   precision  enum tfx_precision
 * ------------------------------------------------------------------------- */
int tfx_sos_forward(const void *x, int x_dtype, void *y, int y_dtype,
                    int64_t C, int64_t T,
                    const double *sos_host, int64_t K,
                    const double *state_x_in, const double *state_y_in,
                    double *state_x_out, double *state_y_out,
                    void *y_sections, int precision, tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * tfx_sos_bank_forward -- filter bank: n_bands independent K-section cascades applied to the SAME
 * input rows in one launch (x is read from HBM once, the bands' re-reads hit cache).
 * Replaces the loop of LogFilterBank.forward (src/torchfx/filter/filterbank.py:157-185:
 * `torch.stack([f(x) for f in self.filters])`) -- SURVEY.md 8(f) rank 2.
 *   x DEVICE [C,T];  y DEVICE [n_bands, C, T];  sos_host HOST [n_bands, K, 6];
 *   states DEVICE [K, n_bands*C, 2] float64 (band-major rows), NULL = zeros.
 * ------------------------------------------------------------------------- */
int tfx_sos_bank_forward(const void *x, int x_dtype, void *y, int y_dtype,
                         int64_t C, int64_t T,
                         const double *sos_host, int64_t n_bands, int64_t K,
                         const double *state_x_in, const double *state_y_in,
                         double *state_x_out, double *state_y_out,
                         int precision, tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * tfx_sos_bank_sum_forward -- `f1 + f2 + ...` of IIR branches in ONE launch: n_bands independent
 * K-section cascades applied to the same input rows and their outputs accumulated,
 *   y[C,T] = sum_b cascade_b(x[C,T]),
 * each branch rounded to the output dtype and added in branch order, exactly like
 * ParallelFilterCombination.forward (src/torchfx/filter/__base.py:1019-1026: zeros_like + in-place
 * adds of the branch outputs) -- 8 B/sample instead of n x 8 + (n + 1) x 4.  Shorter branches are
 * padded by the caller with identity sections [1,0,0,1,0,0].  x and y must have the same dtype.
 *   sos_host HOST [n_bands, K, 6];  states DEVICE [K, n_bands*C, 2] float64 (band-major rows).
 * ------------------------------------------------------------------------- */
int tfx_sos_bank_sum_forward(const void *x, int x_dtype, void *y, int y_dtype,
                             int64_t C, int64_t T,
                             const double *sos_host, int64_t n_bands, int64_t K,
                             const double *state_x_in, const double *state_y_in,
                             double *state_x_out, double *state_y_out,
                             int precision, tfx_stream_t stream);

/* What AUTO would pick for this SOS, and the plan facts (for DESIGN/bench
 * reporting and tests): *precision (TFX_PREC_F32/F64), *warmup (samples of
 * warm-up halo per time segment; -1 = filter memory too long, sequential
 * segments), *err_bound (worst-case |error| of the f32 path for |x|<=1). */
int tfx_sos_plan_info(const double *sos_host, int64_t K,
                      int *precision, int64_t *warmup, double *err_bound);

/* The float64-arithmetic facts of a cascade (host only, any output may be NULL): *unit_form = 1 when float32 signals on
 * aligned rows run it in the unit-b0 form (K >= 2, sane b0); *refine_f32 / *refine_f64 = 1 when launches with a float32 /
 * float64 result take the kernels that refine the lane scan's start states once per section and tile.  The rule is
 * measured per cascade: the unrefined kernel's float64 arithmetic and the sequential float64 recursion are replayed on the
 * host against a long double recursion; errs[4] = {blocked, sequential} error as shares of the output scale at 64 samples
 * per lane (float32 signals), then at 16 (float64 results).  A float32 result refines when blocked > 1e-10, a float64
 * result when blocked > 2 max(sequential, 2^-50).  Cascades with poles next to z = 1 under a rough output (20 Hz
 * high-pass, notch, low peaking EQ) refine; ordinary ones run the kernels they always did. */
int tfx_sos_refine_info(const double *sos_host, int64_t K,
                        int *unit_form, int *refine_f32, int *refine_f64, double *errs);

/* How tfx_sos_forward cuts [C,T] rows into time segments for this cascade, dtypes and precision (host only when wave_slots
 * > 0; same argument checks and the same code path as the call; any output may be NULL).  *route:
 *   TFX_SOS_ROUTE_SEQUENTIAL  one wavefront per row;
 *   TFX_SOS_ROUTE_HALO        segments after the first start *warmup samples early from zero state (short-memory cascades);
 *   TFX_SOS_ROUTE_HANDOFF     every segment starts at its own first sample from the exact state, for any pole radius: end-state
 *                             passes over the segments, a scan of the end states with the segment's transition matrix, one
 *                             refinement of both where the cascade's lane scan is refined too, then the ordinary kernel.
 * *nseg segments per row, *seg_len samples between the starts of consecutive segments (segment g stores from
 * g * seg_len + warmup), *warmup the halo in force (0 unless HALO), *passes reads of the signal (1; hand-off: 2, or 3 with
 * the refinement), *bytes_per_sample the signal traffic that makes.  sections != 0: section taps are asked for.
 * wave_slots: wavefronts the device is taken to hold at once (MI355X: 2048 for the float64 kernels); 0 = ask the current
 * device as the launch does.  The environment (TFX_SOS_NSEG, TFX_SOS_HANDOFF) acts on the query as on the call. */
enum tfx_sos_route { TFX_SOS_ROUTE_SEQUENTIAL = 0, TFX_SOS_ROUTE_HALO = 1, TFX_SOS_ROUTE_HANDOFF = 2 };
int tfx_sos_route_info(int64_t C, int64_t T, const double *sos_host, int64_t K, int x_dtype, int y_dtype, int precision,
                       int sections, int64_t wave_slots, int *route, int64_t *nseg, int64_t *seg_len, int64_t *warmup,
                       int *passes, double *bytes_per_sample);

/* ---------------------------------------------------------------------------
 * tfx_sos_filtfilt_forward -- zero-phase (forward-backward) filtering along each row with the semantics of
 * scipy.signal.sosfiltfilt(sos, x, axis=-1, padtype, padlen) (SciPy 1.15); the reference has no counterpart.
 * The cascade runs over the row extended by `padlen` samples at each end, then backward over its own output, each
 * pass started from the cascade's steady state for its first sample (sosfilt_zi), in float64 DF1 arithmetic.  Two
 * cascade launches around one float64 intermediate: the extension and the time reversal are index arithmetic, the
 * signal is read once and written once (24 B per float32 sample).  A row with a NaN comes back all NaN, a row
 * with an Inf all non-finite.
 *   x        DEVICE [C,T] of x_dtype;  y DEVICE [C,T] of y_dtype (written)
 *   sos_host HOST   [K,6] float64, a0 = 1; a section with a pole at z = 1 (a0 + a1 + a2 = 0) is an error
 *   padtype  enum tfx_padtype;  padlen >= 0, or -1 for SciPy's default (tfx_sos_filtfilt_plan_info reports it);
 *            T <= padlen is an error
 *   work     DEVICE float64 [C * (T + 2 * padlen)], provided by the caller (the intermediate); contents on
 *            return are unspecified
 * ------------------------------------------------------------------------- */
enum tfx_padtype { TFX_PAD_ODD = 0, TFX_PAD_EVEN = 1, TFX_PAD_CONSTANT = 2, TFX_PAD_NONE = 3 };
int tfx_sos_filtfilt_forward(const void *x, int x_dtype, void *y, int y_dtype,
                             int64_t C, int64_t T,
                             const double *sos_host, int64_t K,
                             int padtype, int64_t padlen, double *work, tfx_stream_t stream);
/* What tfx_sos_filtfilt_forward does for [C,T] rows (host-only; same argument checks): SciPy's default padlen for
 * this cascade, the padlen in force, the elements of `work`, the warm-up halo of a time segment (-1 = one segment
 * per row) and the segments per row of the forward and of the reverse pass.  Any output may be NULL. */
int tfx_sos_filtfilt_plan_info(int64_t C, int64_t T, const double *sos_host, int64_t K, int padtype, int64_t padlen,
                               int64_t *default_padlen, int64_t *padlen_used, int64_t *work_elems, int64_t *warmup,
                               int *nseg_forward, int *nseg_reverse);

/* ---------------------------------------------------------------------------
 * tfx_sos_block_energy_forward -- the cascade and the energy of its output per block of samples in ONE launch; the
 * filtered signal is never stored.  With y = the float64 DF1 cascade of row r from zero state,
 *   s[r, i] = sum of y[r, n]^2 over n in [e_i, e_(i+1)),   e_i = (i * num) / den (integer division),
 * for i < nblk = (T * den) / num; samples from e_nblk on belong to no block.  The measurement under a BS.1770 loudness
 * meter (K-weighting, num / den = fs / 10); the reference has no counterpart.  Deterministic: every s[r, i] has one
 * writer, and how a row is cut into time segments depends on T, the cascade and num / den alone, so a row's result
 * does not depend on the other rows.  A NaN / Inf sample makes its block and every later block of its row non-finite.
 *   x        DEVICE [C,T] of x_dtype (float32 or float64);  s DEVICE float64 [C, nblk] (written)
 *   sos_host HOST   [K,6] float64, a0 = 1
 *   num, den >= 1 with num >= 64 * den (blocks of at least 64 samples)
 * ------------------------------------------------------------------------- */
int tfx_sos_block_energy_forward(const void *x, int x_dtype, double *s,
                                 int64_t C, int64_t T,
                                 const double *sos_host, int64_t K,
                                 int64_t num, int64_t den, tfx_stream_t stream);
/* What tfx_sos_block_energy_forward does for [C,T] rows (host-only; same argument checks): the blocks per row, the time
 * segments per row and the warm-up halo of a segment (0 with one segment).  A cascade that does not decay
 * (tfx_sos_plan_info: warmup -1) runs one segment per row and is refused for rows above 2^24 samples.  Any output may
 * be NULL. */
int tfx_sos_block_energy_plan_info(int64_t C, int64_t T, const double *sos_host, int64_t K, int64_t num, int64_t den,
                                   int64_t *nblk, int *nseg, int64_t *warm);

/* ---------------------------------------------------------------------------
 * tfx_biquad_forward -- single DF1 biquad.
 * Replaces  torchfx_ext.biquad_forward(x, b, a1, a2, state_x, state_y)
 *           binding.cpp:30-50,84-87 -> biquad_forward_cpu iir_cpu.cpp:10-62 /
 *           biquad_forward_cuda cuda/biquad_forward.cu:7-47.
 * b_host = HOST [3]; states DEVICE [C,2] float64 (NULL = zeros).
 * ------------------------------------------------------------------------- */
int tfx_biquad_forward(const void *x, int x_dtype, void *y, int y_dtype,
                       int64_t C, int64_t T,
                       const double *b_host, double a1, double a2,
                       const double *state_x_in, const double *state_y_in,
                       double *state_x_out, double *state_y_out,
                       int precision, tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * tfx_fir_direct_forward -- causal depthwise FIR, direct form.
 * Replaces the conv_mode="direct" branch of FIR.forward
 *           src/torchfx/filter/fir.py:556-568  (F.pad + F.conv1d(groups=C)):
 *   y[c,n] = sum_{j<K} kernel[j] * xpad[c,n+j],  xpad = x left-padded by K-1,
 * with `kernel` the FLIPPED taps exactly as FIR stores them (fir.py:516-518).
 * kernel_host: HOST [K] of `dtype`.  x, y: DEVICE [C,T] of `dtype`.
 * ------------------------------------------------------------------------- */
int tfx_fir_direct_forward(const void *x, void *y, int dtype,
                           int64_t C, int64_t T,
                           const void *kernel_host, int64_t K,
                           tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * tfx_fft_conv_forward -- overlap-save FFT convolution (rocFFT + HIP kernels).
 * Replaces  fft_conv1d(x, kernel, padding=(l,r))
 *           src/torchfx/filter/_fftconv.py:70-141
 * and through it the default conv_mode="fft" branch of FIR.forward
 *           src/torchfx/filter/fir.py:552-555.
 *   x  DEVICE [C,T];  kernel_host HOST [K] FLIPPED taps (the reference's
 *   [1,1,K] buffer);  y DEVICE [C, T+pad_left+pad_right-K+1] (written).
 * Errors like the reference: rc != 0 with "kernel size" in the message when
 * T+l+r < K (_fftconv.py:111-115).
 * The FFT block size is chosen for MI355X (power of two), not the
 * reference's int(5*K); results agree to float rounding.
 * ------------------------------------------------------------------------- */
int tfx_fft_conv_forward(const void *x, void *y, int dtype,
                         int64_t C, int64_t T,
                         const void *kernel_host, int64_t K,
                         int64_t pad_left, int64_t pad_right,
                         tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Epilogues: `filter | Gain | Normalize` without a streaming pass per effect.
 * Replaces, when it follows a filter in a pipeline,
 *   Gain.forward                      src/torchfx/effect.py:361-383   y = x * gain, optional clip to [-1, 1]
 *   the reduction half of Normalize   src/torchfx/effect.py:696-698 (peak), 719-721 (RMS), 775-786 (per channel)
 * The producing kernel (the SOS cascade; the last pass of the overlap-save convolution) multiplies and
 * clips every sample it stores -- in the output dtype, on the rounded value a standalone Gain pass would
 * have read: bit-identical -- and gathers max|y| or sum y^2 on the fly; `stat_out` receives that raw
 * statistic (float64, DEVICE, [C] when stat_per_row else [1]) and tfx_normalize_apply turns it into
 *   y = s > 0 ? x / s * peak : x,   s = max|x|  (mode 0)  or  sqrt(sum x^2 / n)  (mode 1)
 * in one pass.  Producers without a fused epilogue (direct FIR, the rocFFT path) run the same arithmetic
 * as separate passes inside the call.
 * ------------------------------------------------------------------------- */
typedef struct tfx_epilogue {
    double gain;          /* linear factor; 1.0 = none */
    int clamp;            /* != 0: clip to [-1, 1] after the gain */
    int stat_mode;        /* -1 none, 0 max|y|, 1 sum of y^2 */
    int stat_per_row;     /* != 0: one statistic per output row, else one for the whole tensor */
    double *stat_out;     /* DEVICE float64 [C] or [1]; required when stat_mode >= 0 */
} tfx_epilogue;

/* tfx_sos_forward (no section taps) + epilogue */
int tfx_sos_forward_ep(const void *x, int x_dtype, void *y, int y_dtype, int64_t C, int64_t T,
                       const double *sos_host, int64_t K,
                       const double *state_x_in, const double *state_y_in,
                       double *state_x_out, double *state_y_out,
                       int precision, const tfx_epilogue *epilogue, tfx_stream_t stream);

/* tfx_fft_conv_forward + epilogue */
int tfx_fft_conv_forward_ep(const void *x, void *y, int dtype, int64_t C, int64_t T,
                            const void *kernel_host, int64_t K, int64_t pad_left, int64_t pad_right,
                            const tfx_epilogue *epilogue, tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * tfx_sos_fft_conv_forward -- a zero-state SOS cascade followed by an FFT-mode FIR as ONE overlap-save
 * pipeline, in the reference's own arithmetic.  Replaces two consecutive steps of Wave._materialize
 *           src/torchfx/wave.py:207-239
 * namely  parallel_iir_forward(x, sos, None, None)   src/torchfx/_ops.py:119-176  (float64 DF1 recursion,
 *           src/torchfx/_csrc/cpu/iir_cpu.cpp:132-147; fresh FusedSOSCascade: zero state, src/torchfx/filter/fused.py:62-64),
 * the downcast to the signal's float32             src/torchfx/filter/iir.py:84-184,
 * and    fft_conv1d(., kernel, padding=(l, r))      src/torchfx/filter/_fftconv.py:70-141.
 * The recursion runs in float64 registers inside the forward column pass of the three-pass transform (one
 * thread per 4096-sample row, exact warm-up from zero state), so it costs no pass over the signal of its own.
 *   x DEVICE float32 [C,T]; sos_host HOST float64 [K,6]; kernel_host HOST float32 [taps] FLIPPED;
 *   y DEVICE float32 [C, T+pad_left+pad_right-taps+1];  y_sections: optional DEVICE float64 [K,C,T], every
 *   section's output ("IIR compared section-by-section"), or NULL;  force_block 1 / 2: take the 2^20 / 2^21-point
 *   block even when the row is shorter than one block (fixture-sized parity tests).
 * tfx_sos_fft_conv_supported answers 1 when the geometry is served (T and T+l+r-taps+1 multiples of 32,
 * K <= 8 sections whose memory fades within 4096 samples, taps that select the 2^20-point block), else 0:
 * callers stage the two steps (tfx_sos_forward, tfx_fft_conv_forward) then.
 * ------------------------------------------------------------------------- */
int tfx_sos_fft_conv_supported(int64_t T, const double *sos_host, int64_t K, int64_t taps,
                               int64_t pad_left, int64_t pad_right, int force_block);
/* 1 + the geometry the fused pipeline would use (*N block length: 2^20, or 2^21 = 256 rows of 8192 samples on rows of at
 * least 2^23 samples; *S hop; *F frames per row for x on a 128-byte line -- a view that starts inside one can take one
 * frame more; *warmup samples), 0 when tfx_sos_fft_conv_supported would say no.  Host-only. */
int tfx_sos_fft_conv_plan_info(int64_t T, const double *sos_host, int64_t K, int64_t taps,
                               int64_t pad_left, int64_t pad_right, int force_block,
                               int64_t *N, int64_t *S, int64_t *F, int64_t *warmup);
/* The same, plus the tail geometry: at N = 2^21, where what a row's last frame has to deliver fits the hop of a 2^20-point
 * frame, that frame runs at *tail_N = 2^20 points with hop *tail_S, from sample (*F - 1) * *S of the output row on; the
 * *F - 1 frames before it run at *N.  *tail_N = *tail_S = 0: all *F frames run at *N.  Any output may be NULL. */
int tfx_sos_fft_conv_plan_info2(int64_t T, const double *sos_host, int64_t K, int64_t taps,
                                int64_t pad_left, int64_t pad_right, int force_block,
                                int64_t *N, int64_t *S, int64_t *F, int64_t *warmup, int64_t *tail_N, int64_t *tail_S);
/* samples a row's recursion starts early from zero state inside the column pass (-1: more than 8 sections / no decay) */
int64_t tfx_sos_fft_conv_warmup(const double *sos_host, int64_t K);
int tfx_sos_fft_conv_forward(const float *x, float *y, int64_t C, int64_t T,
                             const double *sos_host, int64_t K,
                             const float *kernel_host, int64_t taps,
                             int64_t pad_left, int64_t pad_right,
                             double *y_sections, int force_block,
                             const tfx_epilogue *epilogue, tfx_stream_t stream);

/* the apply half of Normalize on a statistic left by an epilogue (or by tfx_stat_forward's raw form) */
int tfx_normalize_apply(const void *x, void *y, int dtype, int64_t C, int64_t T, int mode, int per_row,
                        double peak, const double *stat_dev, tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Stream history -- the contract of every streaming entry point (tfx_fir_stream_forward, tfx_chunk_forward,
 * tfx_delay_stream_forward, tfx_delay_line_stream_forward, tfx_resample_stream_forward, tfx_limiter_stream_forward,
 * tfx_modulated_delay_stream_forward, tfx_waveshaper_stream_forward).  A chunk
 * continues the last H input samples of each of its rows (H is the entry's: K-1, Kf-1, taps*delay, delay, Lp_s-1, Hs, the
 * modulated delay's reach, the waveshaper's Hs):
 *   hist_in  DEVICE [rows, H] of the entry's dtype: the H samples before the chunk, oldest first; NULL = silence (the first
 *            chunk of a stream).
 *   hist_out DEVICE [rows, H]: receives the newest H samples of [hist_in | x] (x: what the entry filters, the cascade output
 *            for tfx_chunk_forward), the next chunk's hist_in.  NULL only where the entry allows it, or when rows*H = 0.
 * hist_out needs its own buffer, and neither y nor hist_out may overlap x, hist_in or each other.  The entries check this
 * rule and their other arguments before they touch the device; a refused call returns non-zero.
 * ------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------
 * tfx_fir_stream_forward -- one chunk of a stateful FIR (streaming).
 * The reference's FIR is stateless (src/torchfx/filter/fir.py:526-579: every call left-pads with K-1
 * zeros), so StreamProcessor (src/torchfx/realtime/stream.py:164-347) is only seamless for FIR stages
 * with overlap >= K-1.  Here the chunk is filtered as the continuation of what came before:
 *   y[c,n] = sum_{j<K} kernel[j] * xv[c, n+j],   xv = [hist_in[c, 0..K-2] | x[c, 0..T-1]],
 * the kernels read the K-1 history samples and the chunk from their two buffers (no concatenated copy),
 * and hist_out receives the last K-1 samples of xv for the next call.
 *   History as in "Stream history" with H = K-1; hist_out NULL: no history out.  direct != 0: time-domain kernels, else
 *   overlap-save.
 * ------------------------------------------------------------------------- */
int tfx_fir_stream_forward(const void *x, void *y, int dtype, int64_t C, int64_t T,
                           const void *kernel_host, int64_t K, int direct,
                           const void *hist_in, void *hist_out, tfx_stream_t stream);

/* tfx_quantile_abs -- out_dev[0] (DEVICE float64) = the q-quantile (0 <= q <= 1, linear interpolation) of |x| over all n float32
 * elements: the threshold of PercentileNormalizationStrategy (src/torchfx/effect.py:723-755,
 * `torch.quantile(torch.abs(waveform), p / 100, interpolation="linear")`) as a three-pass radix SELECT instead of a sort -- same
 * value as torch.quantile wherever that runs (float32 rank arithmetic and lerp of ATen), no 16 M element limit, no host sync.
 * Feed out_dev to tfx_normalize_apply (mode 0) for the scaling.  NaN anywhere in x -> NaN. */
int tfx_quantile_abs(const float *x, int64_t n, double q, double *out_dev, tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * tfx_chunk_forward -- ONE launch for one small streaming chunk: SOS cascade -> stateful direct FIR -> gain / clip.
 * Replaces, for the reference's small-block caller (RealtimeProcessor._audio_callback,
 * src/torchfx/realtime/processor.py:253-292, and StreamProcessor's chunk loop, realtime/stream.py:234-273), the
 * per-effect launches of   IIR ... | FIR | Gain   on a [C, T] float32 block:
 *   u = cascade(x) with carried DF1 state (layout and rounding of tfx_sos_forward, float32 output),
 *   y[c,n] = clip(gain * sum_{j<Kf} taps[j] * [hist_in[c] | u[c]][n+j]),  hist_out[c] = last Kf-1 samples of [hist_in[c] | u[c]].
 * Same arithmetic as tfx_sos_forward -> tfx_fir_stream_forward(direct) -> tfx_gain_forward (the cascade walks 16-sample lane
 * chunks instead of 64: results agree to float64 round-off of the recursion, i.e. to the last float32 bit in all but rare samples).
 *   K = 0: no cascade (u = x);  Kf = 1 with taps {1}: no FIR;  scale / clamp = 0: no gain stage.
 *   Limits (tfx_chunk_supported): T <= 4096, K <= 64, Kf <= 4096, T * Kf <= 2^22 -- a latency path, not a throughput one.
 *   x_pitch: elements between consecutive rows of x (a chunk is usually a column window of a longer [C, T_total] buffer:
 *   no contiguous copy needed); 0 = T.  y is contiguous [C, T].
 *   state pointers: DEVICE float64 [K, C, 2] (in: NULL = zeros);  history as in "Stream history", float32 with H = Kf-1 (its
 *   overlap rule takes x as (C-1)*x_pitch + T floats); hist_out NULL: no history out;
 *   sos_host [K, 6] HOST float64;  taps_host HOST float32 (flipped, like the module's kernel buffer).
 * ------------------------------------------------------------------------- */
int tfx_chunk_supported(int64_t C, int64_t T, int64_t K, int64_t Kf);
int tfx_chunk_forward(const float *x, int64_t x_pitch, float *y, int64_t C, int64_t T,
                      const double *sos_host, int64_t K,
                      const double *state_x_in, const double *state_y_in, double *state_x_out, double *state_y_out,
                      const float *taps_host, int64_t Kf, const float *hist_in, float *hist_out,
                      double gain, int scale, int clamp, int precision, tfx_stream_t stream);

/* Block geometry the overlap-save op would use for a [*, T] signal and a K-tap kernel with
 * padding (l, r): *N = FFT block length, *S = hop (valid outputs per block), *F = blocks per row,
 * *native = 1 when a hand-written LDS-FFT path runs -- the three-pass pipeline OR (since round 4) a one-launch kernel --
 * and 0 for the rocFFT path: callers that price traffic must use tfx_ols_plan_info2's *path (the 20 N/S + 4 model
 * holds for path 1 only).  No GPU needed. */
int tfx_ols_plan_info(int64_t K, int64_t T, int64_t pad_left, int64_t pad_right,
                      int64_t *N, int64_t *S, int64_t *F, int *native);
/* The same for a signal of `dtype` (tfx_ols_plan_info answers for float32).  *path = 2: one launch, the
 * whole transform of a block in LDS and registers (*N = 4096, 8192 or 16384: K <= 8192 in float32, K <= 4096 in
 * float64; e N/S + e bytes of HBM traffic per output sample, e = element size); 1: the three-pass four-step
 * pipeline (float32, 20 N/S + 4); 0: rocFFT (~95, float64 ~190).  The answer is what tfx_fft_conv_forward does for a
 * signal whose base pointer sits on a 128-byte line: *F is that signal's frame count, and on path 1 a view that starts
 * inside a line can take one frame more. */
int tfx_ols_plan_info2(int64_t K, int64_t T, int64_t pad_left, int64_t pad_right, int dtype,
                       int64_t *N, int64_t *S, int64_t *F, int *path);

/* Start, on a helper thread, the one-time per-device set-up of the overlap-save path (kernel attributes = load of the
 * library's code object, internal streams and events: 20-35 ms of driver time in the first call of a process) for the
 * device current at the call; returns at once, the first overlap-save call waits for it.  Optional: a caller that has
 * host work of its own before its first call (the Python planner merges taps, src/torchfx/wave.py:207-239 is the
 * reference's counterpart) overlaps the two.  No reference counterpart; needs a device. */
int tfx_prewarm(void);
/* TFX_* tuning knobs are read from the environment ONCE per process (a dispatch asks for about ten of them); a process
 * that changes them at run time calls this afterwards -- or sets TFX_ENV_DYNAMIC=1 before the first call, which makes
 * every lookup a fresh getenv (the test suite does). */
int tfx_env_reload(void);

/* ---------------------------------------------------------------------------
 * tfx_delay_line_forward -- kept because the reference extension exports it
 * (binding.cpp:68-81,92-95; tests/test_ops_dispatch.py:29-35); out of the
 * hot-path scope.  y = x + (mix*decay) * x[n-delay]  (delay_cpu.cpp:17-41).
 * ------------------------------------------------------------------------- */
int tfx_delay_line_forward(const void *x, void *y, int dtype, int64_t C, int64_t T,
                           int64_t delay, double decay, double mix, tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * tfx_delay_forward -- the BPM-synced multi-tap Delay (src/torchfx/effect.py:934-1538: MonoDelayStrategy,
 * PingPongDelayStrategy and the torch.lerp dry/wet mix of Delay.forward) in ONE launch:
 *   wet[n] = sum_{i=1..taps} amps[i-1] * src[n - i*delay]   (positions outside [0, T) skipped, tap order, +0.0 start)
 *   y[n]   = lerp(n < T ? x[n] : 0, wet[n], mix)            n in [0, T + taps*delay)
 * x DEVICE [rows, T] of dtype; y DEVICE [rows, T + taps*delay]; amps_host HOST float64 [taps] (the reference's
 * feedback ** (i-1), amps[0] = 1).  pingpong != 0: rows are consecutive (left, right) pairs (rows even); odd taps of the
 * left row feed the right one, even taps of the right row the left one; else every row delays itself.  Same arithmetic
 * as the composition on the device (bit-identical).  The epilogue works as for the filters above.  Arguments are
 * checked before the device is touched (null pointers, taps < 1, delay < 0, odd rows with ping-pong, bad dtype).
 * ------------------------------------------------------------------------- */
int tfx_delay_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t delay, int64_t taps,
                      const double *amps_host, double mix, int pingpong, const tfx_epilogue *epilogue,
                      tfx_stream_t stream);
/* ---------------------------------------------------------------------------
 * tfx_delay_stream_forward -- one chunk of a stateful (streaming) Delay, StatefulDelay in torchfx_amd/realtime.py.
 * Each row's chunk continues the last H = taps*delay input samples of that row (hist_in):
 *   v = [hist_in[r] | x[r]],  wet[n] = sum_{i=1..taps} amps[i-1] * src_v[H + n - i*delay]   (tap order, +0.0 start)
 *   y[n] = lerp(x[n], wet[n], mix)   n in [0, T);   hist_out[r] = the newest H samples of v
 * x DEVICE [rows, T] of dtype; y DEVICE [rows, T]; history as in "Stream history" (the kernel reads the inputs and
 * writes the outputs from different workgroups); amps and pingpong as for tfx_delay_forward (ping-pong rows read the partner row's
 * history).  The outputs of consecutive chunks,
 * followed by those of H zero samples (the ring-out), are bit-identical to tfx_delay_forward on the whole signal.
 * T = 0 leaves y empty and copies the history.  One launch.  Refused: null pointers, taps < 1, delay < 0, negative sizes,
 * odd rows with ping-pong, bad dtype, overflow of taps*delay.
 * ------------------------------------------------------------------------- */
int tfx_delay_stream_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t delay, int64_t taps,
                             const double *amps_host, double mix, int pingpong, const void *hist_in, void *hist_out,
                             tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * tfx_delay_line_stream_forward -- one chunk of tfx_delay_line_forward over a continuous stream (StatefulReverb):
 *   v = [hist_in[c] | x[c]],  y[c,n] = x[c,n] + (mix*decay) * v[c, n]   (v indexed from the start of hist_in),
 *   hist_out[c] = the newest `delay` samples of v.
 * x, y DEVICE [C, T]; history as in "Stream history" with H = delay (silence: the first `delay` outputs copy x, as the
 * one-shot call leaves them).  Same arithmetic as tfx_delay_line_forward.  One launch.
 * ------------------------------------------------------------------------- */
int tfx_delay_line_stream_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, int64_t delay, double decay,
                                  double mix, const void *hist_in, void *hist_out, tfx_stream_t stream);

/* the kernel tfx_delay_forward picks (host-only): 0 = span (taps*delay + tile staged in LDS), 1 = lattice (long delay,
 * taps <= 8, residue classes with a register ring), 2 = gather (anything else, every tap a global load) */
int tfx_delay_plan_info(int64_t delay, int64_t taps, int dtype, int pingpong, int *regime);
/* the workgroup geometry of tfx_delay_forward on [rows, T] (host-only; the size checks of tfx_delay_forward; the launch fills
 * its kernel arguments from the same plan): the regime (as above); units = rows (gather) or rows / pairs (span, lattice; a
 * ping-pong pair is one unit); tiles = ceil(L / 1024) output tiles per row, L = T + taps*delay (span, gather), or
 * ceil(delay / 256) residue blocks of 256 lanes (lattice); kc and nchunks, lattice only (else 0): the ceil(L / delay) steps of a
 * row are cut into nchunks chunks of kc steps (128, halved down to 16 while the grid has fewer than 4096 workgroups), chunk c
 * owning outputs [c*kc*delay, (c+1)*kc*delay); groups = workgroups per unit (tiles, or tiles*nchunks) = the first-level
 * partials of an epilogue statistic per unit; nwg = units*groups (0: nothing to launch); lds_bytes per workgroup (span). */
int tfx_delay_tiling_info(int64_t rows, int64_t T, int64_t delay, int64_t taps, int dtype, int pingpong, int *regime, int64_t *units,
                          int64_t *tiles, int64_t *kc, int64_t *nchunks, int64_t *groups, int64_t *nwg, int64_t *lds_bytes);

/* ---------------------------------------------------------------------------
 * tfx_resample_forward -- polyphase rational resampling along each row, scipy.signal.resample_poly(x, up, down, axis=-1,
 * padtype="constant") with the caller's filter, in ONE launch:
 *   up, down reduced by their gcd; up == down: y = x (a copy);  n_out = ceil(T * up / down);
 *   h_padded = [0 * n_pre_pad | taps | 0 * n_post_pad] with SciPy's n_pre_pad, n_post_pad and n_pre_remove (worked out here
 *   from nh, up and down, half_len = (nh - 1) / 2), zero padded to Lp * up taps;
 *   y[m] = sum_{j < Lp} h_padded[n mod up + j*up] * x[n / up - j],  n = (m + n_pre_remove) * down,  x = 0 outside [0, T).
 * x DEVICE [rows, T] of dtype (float32 / float64); y DEVICE [rows, n_out] of dtype; taps_host HOST [nh] of dtype, already
 * scaled by up (resample_poly's `h *= up`).  The polyphase table is cached by the taps' bytes, up, down and dtype, so once a
 * filter has run the call can be captured into a HIP graph.  Arguments are checked before the device is touched.
 * ------------------------------------------------------------------------- */
int tfx_resample_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t up, int64_t down,
                         const void *taps_host, int64_t nh, tfx_stream_t stream);
/* what tfx_resample_forward does for rows of T samples (host-only): n_out, n_pre_remove, the padded filter length
 * (nh + n_pre_pad + n_post_pad), taps per phase Lp, the kernel (0 = window in LDS and taps in registers, 1 = window in LDS and
 * taps through the cache, 2 = gather: the window does not fit in LDS, 3 = copy: up == down) and its LDS bytes per workgroup */
int tfx_resample_plan_info(int64_t T, int64_t up, int64_t down, int64_t nh, int dtype, int64_t *n_out, int64_t *n_pre_remove,
                           int64_t *padded, int64_t *Lp, int *kernel, int64_t *lds_bytes);
/* the workgroup geometry of that launch (host-only, same arguments and checks): the kernel (as above), G phase groups of `up`
 * threads per workgroup and G_initial, the count before it was halved until the tile's window fit in LDS; E outputs per thread;
 * tile_out = up * G * E outputs per workgroup (tile k starts at output k * tile_out); span, the input samples of a tile's
 * window (0 for the gather kernel, which stages none); LP, the taps per phase a thread runs (Lp rounded up to 8, 16, 24, 32,
 * 48 or 64 with zero taps for kernel 0, else Lp) and tiles = ceil(n_out / tile_out) workgroups per row.  All 0 for the copy. */
int tfx_resample_tiling_info(int64_t T, int64_t up, int64_t down, int64_t nh, int dtype, int *kernel, int64_t *G, int64_t *G_initial,
                             int64_t *E, int64_t *tile_out, int64_t *span, int64_t *LP, int64_t *tiles);
/* ---------------------------------------------------------------------------
 * tfx_resample_stream_forward -- one chunk of tfx_resample_forward over a continuous stream, in ONE launch.  The stream fixes
 * (up, down reduced by their gcd) n_pre_pad and n_pre_remove as above and Lp_s = ceil((nh + n_pre_pad) / up) taps per phase.
 * After `consumed` = N input samples per row it has emitted M(N) = max(0, ceil(N*up/down) - n_pre_remove) outputs; a chunk of
 * T samples emits outputs [M(N), M(N + T)) of the whole signal's, each final (it reads no input past N + T - 1).  Every row
 * carries the last H = Lp_s - 1 input samples ("Stream history"): hist_in holds inputs [N - H, N) (zeros before 0), hist_out
 * receives [N + T - H, N + T).  The remaining ceil(N*up/down) - M(N) outputs come from
 * feeding zeros.  For finite inputs, the chunks' outputs equal tfx_resample_forward on the whole signal bit for bit (up to the
 * sign of a zero): each output is the same fma chain.  up == down: y = x and H = 0.
 * x DEVICE [rows, T], y DEVICE [rows, M(N + T) - M(N)], taps_host as for tfx_resample_forward.
 * ------------------------------------------------------------------------- */
int tfx_resample_stream_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t up, int64_t down,
                                const void *taps_host, int64_t nh, int64_t consumed, const void *hist_in, void *hist_out,
                                tfx_stream_t stream);
/* what tfx_resample_stream_forward does with a chunk of T samples after `consumed` (host-only): the outputs [out_begin, out_end)
 * it emits, the history length H, n_pre_remove (the outputs a stream holds back), Lp_s, the kernel (as tfx_resample_plan_info)
 * and its largest LDS bytes per workgroup (a chunk with few tiles per launch takes smaller tiles, to fill the device) */
int tfx_resample_stream_plan_info(int64_t consumed, int64_t T, int64_t up, int64_t down, int64_t nh, int dtype, int64_t *out_begin,
                                  int64_t *out_end, int64_t *hist_len, int64_t *n_pre_remove, int64_t *Lp, int *kernel,
                                  int64_t *lds_bytes);

/* ---------------------------------------------------------------------------
 * tfx_true_peak_forward -- the true-peak reading of ITU-R BS.1770-4 Annex 2 per row: peak[r] = max_m |y[r, m]| over the
 * T * up outputs y = tfx_resample_forward(x, up, down = 1) with the caller's interpolation filter, the up-sampled signal never
 * stored.  Every y[m] is tfx_resample_forward's fma chain, so a finite row gives the bits of max |.| over that call's output.
 * A row with a NaN sample reads NaN, a row with an Inf sample NaN or +Inf; other rows are unaffected.
 * x DEVICE [rows, T] of dtype (float32 / float64); peak DEVICE [rows] of dtype (linear, not dB); up 2, 4 or 8; taps_host HOST
 * [nh] of dtype, already scaled by up, nh <= 64 * up (the taps of a phase are held in registers); work DEVICE [work_elems] of
 * dtype (tfx_true_peak_plan_info), the per-tile maxima, the caller's to reuse once the call has run.  Two launches, no atomics;
 * the tiling depends on T, up and nh alone, so a row's bits do not depend on the batch.  The polyphase table is the one
 * tfx_resample_forward caches.  Arguments are checked before the device is touched.  rows * T == 0 writes nothing (a row of no
 * samples has peak 0: the caller's to set).
 * ------------------------------------------------------------------------- */
int tfx_true_peak_forward(const void *x, int dtype, void *peak, int64_t rows, int64_t T, int64_t up,
                          const void *taps_host, int64_t nh, void *work, tfx_stream_t stream);
/* what tfx_true_peak_forward does for rows of T samples (host-only, same checks): taps per phase Lp, the input positions per
 * workgroup tile_in, the tiles per row and the elements of `work` (rows * tiles) */
int tfx_true_peak_plan_info(int64_t rows, int64_t T, int64_t up, int64_t nh, int dtype,
                            int64_t *Lp, int64_t *tile_in, int64_t *tiles, int64_t *work_elems);

/* ---------------------------------------------------------------------------
 * tfx_limiter_forward -- look-ahead true-peak limiter in ONE launch.  x is [groups, channels, T]; the `channels` rows of a
 * group share one gain curve.  All arithmetic in dtype, for a group and sample positions n, i, k:
 *   1. q[ch,i] = max_{ph<up} |v[ch, i*up + ph]|, v = tfx_resample_forward(x[ch], up, down = 1) with taps_host (that call's fma
 *      chain, as tfx_true_peak_forward); q[ch,-1] = 0
 *   2. p[i] = max_ch max(|x[ch,i]|, q[ch,i], q[ch,i-1]);  up == 1 (the sample peak, taps ignored): p[i] = max_ch |x[ch,i]|
 *   3. r[i] = p[i] > c ? c / p[i] : 1 (correctly rounded), r = 1 outside [0, T)
 *   4. m[k] = min r[k-H+1 .. k+A-1]
 *   5. s[n]: acc = +0, then for j = A-1 down to 0: acc = fma(w[j], 1 - m[n-j], acc)
 *   6. g[n] = min(max(1 - s[n], 0), r[n])
 *   7. y[ch,n] = g[n] * x[ch,n]
 * x, y DEVICE [groups, channels, T] of dtype (y may not alias x: tiles read their neighbours' inputs); gain DEVICE [groups, T]
 * of dtype or null (g, the gain-reduction meter); c the linear ceiling (> 0, already rounded to dtype); A in [1, 512] and H in
 * [1, 4096] samples; window_host HOST [A] of dtype, non-negative and finite (the caller normalises it to sum 1); up 1, 2, 4 or 8;
 * taps_host HOST [nh] of dtype as for tfx_true_peak_forward (nh <= 64 * up; ignored for up == 1).
 * No recursion: a workgroup computes `tile` consecutive outputs of one group from a bounded window, so a group's bits do not
 * depend on the batch.  A tile whose staged window holds a NaN or an Inf in any channel writes NaN to all its outputs in every
 * channel of the group (and to gain); other tiles and other groups are unaffected.  No atomics, no workspace.  The tap table
 * and the padded window are cached by content, so once they have run the call can be captured into a HIP graph.  Arguments are
 * checked before the device is touched.  groups * T == 0 writes nothing.
 * ------------------------------------------------------------------------- */
int tfx_limiter_forward(const void *x, void *y, void *gain_or_null, int dtype, int64_t groups, int64_t channels, int64_t T,
                        double c, int64_t A, int64_t H, const void *window_host, int64_t up, const void *taps_host, int64_t nh,
                        tfx_stream_t stream);
/* what tfx_limiter_forward does (host-only, same checks on the sizes): outputs per workgroup `tile` (8193 - 2A - H), tiles per
 * group, the input samples a tile reads behind its first and past its last output (halo_left, halo_right), taps per phase Lp
 * (0 for up == 1) and the LDS bytes per workgroup.  The tiling depends on T, A, H, up, nh and dtype alone. */
int tfx_limiter_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t A, int64_t H, int64_t up, int64_t nh, int dtype,
                          int64_t *tile, int64_t *tiles, int64_t *halo_left, int64_t *halo_right, int64_t *Lp,
                          int64_t *lds_bytes);

/* ---------------------------------------------------------------------------
 * tfx_limiter_stream_forward -- one chunk of tfx_limiter_forward over a continuous stream, in ONE launch.  With Y the one-shot
 * result of the whole stream (past and to come), the chunk of T samples that follows `consumed` = N inputs per row writes
 *   y[., t] = Y[N - D + t], 0 where N - D + t < 0        (gain[., t] = g[N - D + t], 1 there)
 * and each sample is final.  (A, H, up, nh) fix the stream's geometry, with n_pre_remove and Lp as tfx_resample_plan_info gives
 * them for (up, down = 1, nh), i_lo = n_pre_remove / up and rem = n_pre_remove mod up:
 *   latency D  = A - 1 + i_lo (+ 1 when rem >= 2; an odd-length filter has rem = 1): output n needs input n + D and no later one;
 *                up == 1: A - 1
 *   history Hs = D + A + H - 2 + max(1, Lp - i_lo) (up == 1: D + A + H - 2): the inputs before the chunk its outputs read
 * History as in "Stream history" with H = Hs: hist_in holds inputs [N - Hs, N) (zeros before 0).  The kernel reads [hist_in | x]
 * from the two buffers and knows where the stream began: positions before 0 have r = 1 and q[-1] = 0 although the interpolator
 * rings into them.  n_in <= T is the number of real inputs in x: n_in < T says that the stream ends after them -- x[., n_in:] is
 * never read, r = 1 from N + n_in on and the interpolated signal is cut there, exactly as tfx_limiter_forward treats its end --
 * and hist_out then receives the newest Hs samples of [hist_in | x[., :n_in]].  The last min(N, D) outputs of a stream of N
 * inputs are the end of a chunk with T = D, n_in = 0.  `consumed` matters only up to Hs + D and is clamped there.
 * Every output is tfx_limiter_forward's arithmetic (the same fma chains, rounded division and exact minimum), so the chunks'
 * outputs equal the one-shot call on the whole signal bit for bit, whatever the chunk sizes.  A workgroup computes up to `tile`
 * outputs and sweeps only the T' + 2A + H - 2 positions of p / r they depend on.  A tile whose [hist_in | x] window holds a NaN
 * or an Inf in any channel writes NaN to all its outputs (at positions >= 0) in every channel of the group; once the sample has
 * left the history the outputs are the clean stream's again.
 * x, y DEVICE [groups, channels, T], gain DEVICE [groups, T] or null, hist_out DEVICE [groups, channels, Hs] or null (no history
 * out); gain may not overlap x, y, hist_in or hist_out either; the other arguments as for tfx_limiter_forward.  T == 0 copies
 * hist_in to hist_out.
 * ------------------------------------------------------------------------- */
int tfx_limiter_stream_forward(const void *x, void *y, void *gain_or_null, int dtype, int64_t groups, int64_t channels, int64_t T,
                               int64_t n_in, int64_t consumed, double c, int64_t A, int64_t H, const void *window_host, int64_t up,
                               const void *taps_host, int64_t nh, const void *hist_in, void *hist_out, tfx_stream_t stream);
/* what tfx_limiter_stream_forward does with a chunk of T samples (host-only, same checks on the sizes): the stream's latency D
 * and history length Hs, outputs per workgroup `tile` (8193 - 2A - H), tiles per group, the positions of p / r the first
 * workgroup sweeps (min(T, tile) + 2A + H - 2, of 8192) and the LDS bytes per workgroup */
int tfx_limiter_stream_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t A, int64_t H, int64_t up, int64_t nh,
                                 int dtype, int64_t *latency, int64_t *history, int64_t *tile, int64_t *tiles, int64_t *positions,
                                 int64_t *lds_bytes);

/* ---------------------------------------------------------------------------
 * tfx_compressor_forward -- feed-forward compressor: log-domain static curve with a soft knee and the smooth decoupled peak
 * detector of Giannoulis, Massberg & Reiss (JAES 2012).  x is [groups, channels, T]; the `channels` rows of a group share one
 * gain curve.  The detector runs in float64 for both signal dtypes, for a group and a sample n:
 *   1. p[n]  = max_ch |x[ch,n]|
 *   2. o = 20 log10 p[n] - th (p = 0: -inf);  v[n] = 0 where 2o <= -w, s o where 2o >= w, else s (o + w/2)^2 / (2w);
 *      a non-finite p[n] gives v[n] = NaN
 *   3. y1[n] = max(v[n], alpha_r y1[n-1] + (1 - alpha_r) v[n]);  yL[n] = alpha_a yL[n-1] + (1 - alpha_a) y1[n];
 *      (y1[-1], yL[-1]) = state_in[group] or 0; max propagates NaN
 *   4. g[n] = 10^((makeup_db - yL[n]) / 20);  y[ch,n] = dtype(g[n] x[ch,n]);  gain[n] = dtype(g[n])
 * th the threshold in dB, s = 1 - 1/ratio in [0, 1], w the knee width in dB (>= 0), alpha_a / alpha_r = exp(-1 / (time * fs)) in
 * [0, 1] (0 for a time of 0).  x, y DEVICE [groups, channels, T] of dtype (y may alias x); gain DEVICE [groups, T] of dtype or
 * null; state_in / state_out DEVICE [groups, 2] float64 (y1, yL) or null (silence in / no state out; state_out is the pair at
 * T - 1 and needs its own buffer).
 * Both recursions are associative scans, so a group's row is cut into tiles of 2048 samples and the tiles into `segments` runs
 * (tfx_compressor_plan_info; 0 = chosen from groups and T, any other value is clamped to the tile count).  segments == 1 is
 * one launch that reads x once and writes y once; otherwise three launches (release summaries, attack summaries, result):
 * x is read three times and `scratch` -- DEVICE, scratch_bytes of the plan, may be null for one segment -- carries the
 * summaries across the launch boundaries.  No workgroup waits for another, no atomics.  The association of the scans follows
 * the tiling: results for different `segments` agree to float64 round-off of the detector (about 1e-13 dB), not bit for bit; a
 * group whose level never passes th - w/2 comes back bit-identical from a zero state with makeup_db = 0, whatever the tiling.
 * From the first non-finite sample of a group to the end of its rows every output, the gain and the end state are NaN; earlier
 * samples and other groups are unaffected.  A group's bits depend on (T, segments) and its own samples alone.  Arguments are
 * checked before the device is touched.  T == 0 copies state_in to state_out.
 * ------------------------------------------------------------------------- */
int tfx_compressor_forward(const void *x, void *y, void *gain_or_null, int dtype, int64_t groups, int64_t channels, int64_t T,
                           double th, double s, double w, double alpha_a, double alpha_r, double makeup_db, const double *state_in,
                           double *state_out, int64_t segments, void *scratch, tfx_stream_t stream);
/* what tfx_compressor_forward does (host-only, same checks on the sizes): samples per tile (2048), tiles per group, the segments
 * it takes for the request `segments`, the tiles of the longest segment (the first tiles mod segments hold one more than the
 * rest) and the bytes of `scratch` (0 for one segment) */
int tfx_compressor_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t segments, int64_t *tile, int64_t *tiles,
                             int64_t *segments_out, int64_t *seg_tiles, int64_t *scratch_bytes);

/* ---------------------------------------------------------------------------
 * tfx_modulated_delay_forward -- the time-varying delay line behind Chorus, Flanger and Vibrato:
 *   y[n] = dry x[n] + sum_v g_v x(n - d_v[n]),   the delay d_v moved by a low-frequency oscillator (LFO).
 * x is [batch, channels, T]; the channel index of a row is c = row mod channels.  voices_host is HOST float64 [V, 5], 1 <= V <= 8,
 * one row (base, depth, inc, phase, gain) per voice: base and depth in samples, inc = rate / fs in cycles per sample, phase in
 * cycles.  For the absolute sample n = position + j, voice v and channel c, every intermediate in float64 for both dtypes:
 *   1. off = frac(phase_v + c * spread), computed on the host
 *   2. t = double(n) * inc_v -- one IEEE multiplication, never contracted into an FMA;  a = (t - floor(t)) + off
 *   3. l = sinpi(2 a) (TFX_LFO_SINE) or 1 - 4 |frac(a + 0.25) - 0.5| (TFX_LFO_TRIANGLE)
 *   4. d = base_v + depth_v * l;  i = floor(d);  f = d - i
 *   5. TFX_INTERP_LINEAR: xd = x[n-i] + f (x[n-i-1] - x[n-i]);  TFX_INTERP_CUBIC: the 4-point third-order Lagrange interpolant
 *      through x[n-i+1], x[n-i], x[n-i-1], x[n-i-2] at f, weights -f(f-1)(f-2)/6, (f+1)(f-1)(f-2)/2, -(f+1)f(f-2)/2, (f+1)f(f-1)/6;
 *      reads before the first sample of the stream give 0 (or the carried history)
 *   6. y[n] = dtype(dry x[n] + sum_v g_v xd_v), summed in voice order and rounded once
 * Rules: base_v - depth_v >= 0 (linear) or >= 1 (cubic); floor(base_v + depth_v) + 3 <= 2^24; 0 < inc_v < 0.5; every value
 * finite; 0 <= position <= 2^52.  x, y DEVICE [batch, channels, T] of dtype, y may not overlap x; the delayed tail past T is
 * dropped.  One launch: a workgroup owns a tile of 1024 samples of one channel index and applies each (i, f) to up to 4 batch
 * items (tfx_modulated_delay_plan_info).  Feed-forward: a row's bits depend on its own samples, its channel index and the
 * position alone -- not on the tiling or the other rows.  At f = 0 both interpolants return x[n-i] exactly.  A non-finite
 * x[m] reaches no output outside [m, m + floor(max_v(base_v + depth_v)) + 2] of its row.  Arguments are checked before the
 * device is touched.
 * ------------------------------------------------------------------------- */
enum tfx_lfo_shape { TFX_LFO_SINE = 0, TFX_LFO_TRIANGLE = 1 };
enum tfx_interp { TFX_INTERP_LINEAR = 0, TFX_INTERP_CUBIC = 1 };
int tfx_modulated_delay_forward(const void *x, void *y, int dtype, int64_t batch, int64_t channels, int64_t T,
                                const double *voices_host, int64_t V, double spread, double dry, int shape, int interp,
                                int64_t position, tfx_stream_t stream);
/* ---------------------------------------------------------------------------
 * tfx_modulated_delay_stream_forward -- one chunk of tfx_modulated_delay_forward over a continuous stream (StatefulChorus,
 * StatefulFlanger, StatefulVibrato), one launch: the chunks' outputs are bit-identical to the one-shot call on the whole
 * signal, whatever the chunk sizes.  History as in "Stream history" with H = max_v floor(base_v + depth_v) + 2 (the plan's
 * `history`); the kernel reads [hist_in | x] from their two buffers and writes hist_out (chunks shorter than H included).
 * The position of the chunk's first sample is read on the device: pos_in DEVICE int64 [1] (NULL = 0), and one lane stores
 * pos_in + T to pos_out (DEVICE int64 [1], its own buffer; NULL = not stored) -- a replayed HIP graph bakes host scalars in,
 * a device counter moves on with every replay.  T = 0 carries history and position over.
 * ------------------------------------------------------------------------- */
int tfx_modulated_delay_stream_forward(const void *x, void *y, int dtype, int64_t batch, int64_t channels, int64_t T,
                                       const double *voices_host, int64_t V, double spread, double dry, int shape, int interp,
                                       const void *hist_in, void *hist_out, const int64_t *pos_in, int64_t *pos_out,
                                       tfx_stream_t stream);
/* what the two entries above do (host-only, same checks on the sizes and the voice table): samples per tile (1024), tiles per
 * row, the history H of a stream, the batch items a workgroup applies one (i, f) to (4) and the batch groups of the grid
 * (ceil(batch / 4)); the grid is tiles * channels * batch_groups workgroups */
int tfx_modulated_delay_plan_info(int64_t batch, int64_t channels, int64_t T, const double *voices_host, int64_t V, int interp,
                                  int64_t *tile, int64_t *tiles, int64_t *history, int64_t *batch_items, int64_t *batch_groups);

/* ---------------------------------------------------------------------------
 * tfx_freeverb_forward -- Freeverb (Jezar at Dreampoint, public domain), the Schroeder-Moorer room reverb: per *bank* (one
 * channel of one batch item) NC parallel feedback combs with a one-pole low-pass in the loop, summed, then NA all-passes in
 * series.  x is [batch, channels, T], channels 1 or 2; y is [batch, channels, T + tail] (x counts as zero from T on).
 * comb_delays_host HOST int64 [channels, NC], 1 <= NC <= 8; allpass_delays_host HOST int64 [channels, NA], 0 <= NA <= 4 (may be
 * null for NA = 0); every delay in [1, 65536] samples.  Everything is float64 for both signal dtypes.  For an item and a sample n:
 *   feed       u[n] = input_gain (2 / channels) sum_c x_c[n]          ((L + R) gain for stereo, L = R for mono)
 *   comb k     o_k[n] = w_k[n - D];  f_k[n] = d2 o_k[n] + d1 f_k[n-1];  w_k[n] = u[n] + feedback f_k[n];  d1 = damp, d2 = 1 - d1
 *   comb sum   s_0[n] = ((o_0[n] + o_1[n]) + o_2[n]) + ...            in this order
 *   all-pass j b[n] = v_j[n - D];  s_{j+1}[n] = b[n] - s_j[n];  v_j[n] = s_j[n] + allpass_gain b[n]
 *   mix        y_c[n] = dtype(dry_gain x_c[n] + wet1 r_c[n] + wet2 r_{1-c}[n]),  r_c = s_NA of bank c; for one channel
 *              dtype(dry_gain x[n] + (wet1 + wet2) r_0[n]); summed left to right, rounded once
 * |feedback| < 1, 0 <= damp < 1, |allpass_gain| < 1, the four gains finite.  w, f and v are zero before sample 0 unless
 * state_in is given.
 * State: DEVICE float64 [batch * channels, state_len], one row per bank: for each comb the last D values of w, oldest first,
 * then f; then for each all-pass the last D values of v, oldest first; state_len is the longest bank's length and a shorter
 * bank's row ends in zeros.  Time order, not ring order: the state does not depend on how the stream was cut, and chunks
 * shorter than a delay work.  state_in null = silence, state_out null = not stored; state_out needs its own buffer.
 * One workgroup per bank and one wave per comb: blocks of B = min(shortest comb delay, 1024) samples; within a block the
 * low-pass is an affine scan over the 64 lanes, the all-passes run in parallel over sub-blocks of up to their delay.  The
 * lines are float64 rings in LDS (TFX_FREEVERB_LINES_LDS) when 8 (line words + 2 B) <= 159 KB, else in `workspace`
 * (TFX_FREEVERB_LINES_GLOBAL).  One launch when channels == 1 or wet2 == 0; else the banks write r to `workspace` and a
 * second, elementwise launch mixes.  workspace: DEVICE, workspace_bytes of the plan, may be null when that is 0.  No
 * workgroup waits for another, no atomics.  The scan's association follows the blocks, and the blocks the start of the call:
 * chunked calls agree with the one-shot call to float64 round-off, not bit for bit.  A bank's bits depend on its item's
 * samples, T, tail and the arguments alone -- not on the other items or their number.  Samples before an item's first
 * non-finite input sample are unaffected by it; other items never are.  x, y DEVICE of dtype, y may not overlap x.  Arguments
 * are checked before the device is touched.  T + tail == 0 copies state_in to state_out.
 * ------------------------------------------------------------------------- */
enum tfx_freeverb_lines { TFX_FREEVERB_LINES_LDS = 0, TFX_FREEVERB_LINES_GLOBAL = 1 };
int tfx_freeverb_forward(const void *x, void *y, int dtype, int64_t batch, int64_t channels, int64_t T, int64_t tail,
                         const int64_t *comb_delays_host, int64_t NC, const int64_t *allpass_delays_host, int64_t NA, double feedback,
                         double damp, double allpass_gain, double input_gain, double dry_gain, double wet1, double wet2,
                         const double *state_in, double *state_out, void *workspace, tfx_stream_t stream);
/* what tfx_freeverb_forward does (host-only, same checks on the sizes and the delays): the block size B, where the lines live
 * (tfx_freeverb_lines), the length of a state row, the launches (1 or 2) and the bytes of `workspace` (the lines of every bank
 * for the global placement, then [batch * channels, T + tail] float64 for two launches) */
int tfx_freeverb_plan_info(int64_t batch, int64_t channels, int64_t T, int64_t tail, const int64_t *comb_delays_host, int64_t NC,
                           const int64_t *allpass_delays_host, int64_t NA, double wet2, int64_t *block, int *placement,
                           int64_t *state_len, int64_t *launches, int64_t *workspace_bytes);

/* ---------------------------------------------------------------------------
 * tfx_waveshaper_forward -- an oversampled memoryless nonlinearity (Waveshaper, Distortion) in ONE launch.  With
 * L = oversample in {1, 2, 4, 8}, h_up the taps of tfx_resample_forward(x, L, 1) and h_dn those of (1, L):
 *   u = resample(x, L, 1)            length T*L, zeros outside [0, T)
 *   v = drive * u + bias             a multiplication, then an addition: two roundings
 *   w = f(v) - c0                    c0 = f(bias) evaluated in float64 on the host and rounded to dtype
 *   z = resample(w, 1, L)            length T; w counts as zero outside [0, T*L)
 *   y = dry * x + wet * z            two multiplications and an addition
 * all in dtype; L = 1 has no filters (z = w).  f: TFX_SHAPE_HARD min(max(v, -1), 1); TFX_SHAPE_CUBIC 1.5 v - 0.5 v^3 inside
 * [-1, 1], sign(v) outside; TFX_SHAPE_TANH; TFX_SHAPE_CURVE a table c of curve_n in [2, 4096] points over [-1, 1] read
 * with WebAudio's rule: pos = (v + 1)(N - 1)/2 clamped to [0, N - 1], i = min(floor(pos), N - 2),
 * f = c[i] + (pos - i)(c[i+1] - c[i]).  x, y DEVICE [rows, T] of dtype (y may not overlap x); curve_host HOST [curve_n] of
 * dtype (NULL unless TFX_SHAPE_CURVE); taps_up_host / taps_dn_host HOST arrays of dtype with at most 64 * L taps each (both
 * ignored when L = 1).  Both stages sum as tfx_resample_forward does (a descending-j fma chain from +0), so a finite signal
 * through TFX_SHAPE_HARD gives the bits of resample -> multiply -> clamp -> resample.  The oversampled signal lives in LDS only.
 * A workgroup owns a tile of `tile` outputs of one row (tfx_waveshaper_plan_info); the tiling does not depend on `rows`, and
 * a row's bits depend on its own samples alone.  Non-finite input: y[m] is NaN exactly when x[m - reach_after .. m +
 * reach_before] holds a NaN or an Inf (every tap of both zero-padded filters counted; an up-sampled value that is not finite
 * shapes to NaN); every other output has the bits it has with a zero in that sample's place.  drive, bias, dry and wet must be
 * finite after rounding to dtype, which is how the kernel holds them: 1e39 is refused for TFX_F32 (it would arrive as Inf, and
 * silence would shape to 0 * Inf = NaN) and accepted for TFX_F64; tfx_waveshaper_stream_forward refuses the same.  Arguments are
 * checked before the device is touched; the first call with a new filter or curve uploads it with a blocking copy and caches it by content.
 * ------------------------------------------------------------------------- */
enum tfx_shape { TFX_SHAPE_HARD = 0, TFX_SHAPE_CUBIC = 1, TFX_SHAPE_TANH = 2, TFX_SHAPE_CURVE = 3 };
int tfx_waveshaper_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t oversample, int shape,
                           const void *curve_host, int64_t curve_n, double drive, double bias, double dry, double wet,
                           const void *taps_up_host, int64_t nh_up, const void *taps_dn_host, int64_t nh_dn, tfx_stream_t stream);
/* what tfx_waveshaper_forward does (host-only, same checks on the sizes): outputs per tile, tiles per row, the future and past
 * input samples an output depends on (reach_before, reach_after; 0 for L = 1), the LDS bytes of a workgroup and the taps per
 * phase of the up-sampler and of the (single-phase, zero-padded) decimator; the grid is rows * tiles workgroups */
int tfx_waveshaper_plan_info(int64_t rows, int64_t T, int64_t oversample, int64_t nh_up, int64_t nh_dn, int64_t curve_n, int dtype,
                             int64_t *tile, int64_t *tiles, int64_t *reach_before, int64_t *reach_after, int64_t *lds_bytes,
                             int64_t *taps_up, int64_t *taps_dn);

/* ---------------------------------------------------------------------------
 * tfx_waveshaper_stream_forward -- one chunk of tfx_waveshaper_forward over a continuous stream, in ONE launch.  With Y the
 * one-shot result of the whole stream (past and to come), the chunk of T samples that follows `consumed` = N inputs per row
 * writes
 *   y[., t] = Y[N - D + t], 0 where N - D + t < 0
 * and each sample is final.  (oversample, nh_up, nh_dn) fix the stream's geometry, with reach_before and reach_after as
 * tfx_waveshaper_plan_info gives them (they do not depend on T):
 *   latency D  = reach_before: output n needs input n + D and no later one
 *   history Hs = reach_before + reach_after: the inputs before the chunk its outputs read
 * and D = Hs = 0 for oversample = 1.  History as in "Stream history" with H = Hs: hist_in holds inputs [N - Hs, N) (zeros
 * before 0).  The kernel reads [hist_in | x] from the two buffers -- the dry term x[N - D + t] too -- and knows where the stream
 * began: the shaped signal w is zero before up-sampled index 0 although the up-sampler rings into it.  n_in <= T is the number
 * of real inputs in x: n_in < T says that the stream ends after them -- x[., n_in:] is never read, the inputs from N + n_in on
 * are zeros and w counts as zero from up-sampled index (N + n_in) * oversample on, exactly as tfx_waveshaper_forward treats its
 * end -- and hist_out then receives the newest Hs samples of [hist_in | x[., :n_in]].  The last min(N, D) outputs of a stream
 * of N inputs are the end of a chunk with T = D, n_in = 0.  `consumed` matters only up to Hs + D and is clamped there.
 * Every output is tfx_waveshaper_forward's arithmetic (the same source: both fma chains, the transfer function, the mix), so
 * the chunks' outputs equal the one-shot call on the whole signal bit for bit, whatever the chunk sizes, a NaN's or an Inf's
 * reach included.  A workgroup computes up to `tile` outputs (the one-shot tiling), and whole waves whose positions no output
 * of the chunk depends on skip the up-sampler and the transfer function.
 * x, y DEVICE [rows, T], hist_out DEVICE [rows, Hs] or null (no history out); the other arguments as for
 * tfx_waveshaper_forward.  T == 0 copies hist_in to hist_out.
 * ------------------------------------------------------------------------- */
int tfx_waveshaper_stream_forward(const void *x, void *y, int dtype, int64_t rows, int64_t T, int64_t n_in, int64_t consumed,
                                  int64_t oversample, int shape, const void *curve_host, int64_t curve_n, double drive, double bias,
                                  double dry, double wet, const void *taps_up_host, int64_t nh_up, const void *taps_dn_host,
                                  int64_t nh_dn, const void *hist_in, void *hist_out, tfx_stream_t stream);
/* what tfx_waveshaper_stream_forward does with a chunk of T samples (host-only, same checks on the sizes): the stream's latency
 * D and history length Hs, outputs per workgroup `tile`, tiles per row, the positions whose up-sampled samples the first
 * workgroup computes and shapes (those its min(T, tile) outputs read, rounded up to whole waves of 512 / 256 positions, of
 * 2048 for float32 / 1024 for float64; min(T, tile) for oversample = 1) and the LDS bytes per workgroup */
int tfx_waveshaper_stream_plan_info(int64_t rows, int64_t T, int64_t oversample, int64_t nh_up, int64_t nh_dn, int64_t curve_n,
                                    int dtype, int64_t *latency, int64_t *history, int64_t *tile, int64_t *tiles,
                                    int64_t *positions, int64_t *lds_bytes);

/* ---------------------------------------------------------------------------
 * tfx_phaser_forward -- the phaser: `stages` = N first-order all-pass sections in series whose one coefficient an LFO sweeps
 * every sample.  x is [rows, T] with rows = batch * channels; the channel index of a row is c = row mod channels.  For the
 * absolute sample n = position + j (position: the host scalar, or *pos_in when pos_in is given), every intermediate in float64
 * for both dtypes:
 *   1. off = frac(phase + c * spread)
 *   2. t = double(n) * (rate / fs) -- one IEEE multiplication, never contracted into an FMA;  a_ = (t - floor(t)) + off
 *   3. l = sinpi(2 a_) (TFX_LFO_SINE) or 1 - 4 |frac(a_ + 0.25) - 0.5| (TFX_LFO_TRIANGLE)   [1 to 3: tfx_modulated_delay_forward's]
 *   4. fc = min_freq * exp(Lg * (0.5 + 0.5 l)),  Lg = ln(max_freq / min_freq) computed on the host as a double (an exponential
 *      sweep; min_freq == max_freq gives a constant filter)
 *   5. g = tan(w * fc),  w = pi / fs computed on the host as a double;  a[n] = (g - 1) / (g + 1): |a| < 1 under the rules, negative below fs / 4
 *   6. x_0 = double(x);  for k = 1..N:  x_k[n] = a[n] x_{k-1}[n] + x_{k-1}[n-1] - a[n] x_k[n-1]   (every section uses a[n])
 *   7. y[n] = dtype(dry x_0[n] + wet x_N[n]), rounded once
 * State: DEVICE float64 [rows, N + 1] = (x_0[-1], x_1[-1], .., x_N[-1]); state_in NULL = silence; state_out (its own buffer, or
 * NULL) receives the state after the last sample.  pos_out (DEVICE int64 [1], its own buffer, or NULL) receives the position + T:
 * a replayed HIP graph bakes host scalars in, a device counter moves on with every replay.  coef_or_null: DEVICE float64
 * [channels, T] -- [1, T] when spread == 0 or channels == 1 -- receives a[n] as the kernel computed it.
 * Rules: 1 <= stages <= 12; 10 Hz <= min_freq <= max_freq <= 0.45 fs; 0 < rate < fs / 2; 0 <= position <= 2^52; dry, wet,
 * phase and spread finite.  x, y DEVICE [rows, T] of dtype, y may not overlap x.
 * Launches: a row is cut into tiles of 2048 samples and the tiles into `segments` runs of whole tiles (0 = the plan's choice: 1
 * when the rows alone fill the chip; clamped to the tile count).  One segment is one launch; otherwise two, the first storing
 * per segment how it maps the incoming state (s -> M s + v, M lower-triangular Toeplitz: 2 N doubles) into `scratch`
 * (scratch_bytes of tfx_phaser_plan_info; may be NULL for one segment).  The coefficient track does not depend on the cut, the
 * segments or the other rows, bit for bit; the outputs depend on the cut only through the association of the scan (float64
 * round-off).  A sample's bits do not depend on values after it.  From a NaN / Inf x[m] on, every output of that row is
 * non-finite.  T == 0 hands the state and the position on.  Arguments are checked before the device is touched.
 * ------------------------------------------------------------------------- */
int tfx_phaser_forward(const void *x, void *y, double *coef_or_null, int dtype, int64_t rows, int64_t channels, int64_t T,
                       int64_t stages, double fs, double rate, double min_freq, double max_freq, double phase, double spread, double dry,
                       double wet, int shape, int64_t position, const int64_t *pos_in, int64_t *pos_out, const double *state_in,
                       double *state_out, int64_t segments, void *scratch, tfx_stream_t stream);
/* what tfx_phaser_forward does (host-only, same checks on the sizes): samples per tile (2048), tiles per row, the segments it
 * takes for the request, the tiles of the longest segment and the bytes of `scratch` (0 for one segment) */
int tfx_phaser_plan_info(int64_t rows, int64_t channels, int64_t T, int64_t stages, int64_t segments, int64_t *tile, int64_t *tiles,
                         int64_t *segments_out, int64_t *seg_tiles, int64_t *scratch_bytes);

/* ---------------------------------------------------------------------------
 * tfx_gate_forward -- noise gate with hysteresis, hold and range.  x is [groups, channels, T]; the `channels` rows of a group
 * share one gain curve.  All levels are linear and come from the caller, so that every implementation compares against the
 * same doubles: p_open = 10^(threshold_db / 20), p_close = 10^((threshold_db - hysteresis_db) / 20) <= p_open, range = r =
 * 10^(-range_db / 20) in [0, 1] (0 for an infinite range), hold = H = floor(hold_seconds * fs + 0.5) samples in [0, 2^31),
 * alpha_a / alpha_r = exp(-1 / (time * fs)) in [0, 1] (0 for a time of 0); the kernel takes bA = 1 - alpha_a and
 * bR = (1 - alpha_r) * r.  The detector runs in float64 for both signal dtypes, for a group and a sample n:
 *   1. p[n] = max_ch |x[ch,n]|; the max propagates NaN
 *   2. the state (open, c) starts from state_in[group] or (closed, 0):
 *        if p >= p_open: open = 1, c = 0;  else if open and p >= p_close: c = 0;
 *        else if open: c += 1, and if c > H then open = 0, c = 0;  else: stays closed.   open[n] is the value after sample n
 *   3. g[n] = alpha_a g[n-1] + bA where open[n], else alpha_r g[n-1] + bR;  g[-1] = state_in[group][0] or r
 *   4. y[ch,n] = dtype(g[n] x[ch,n]);  gain[n] = dtype(g[n])
 *   5. a non-finite p[n] (NaN or Inf) poisons its group: from that sample to the end of its rows y, gain and the end state are
 *      NaN and open is 0; earlier samples and other groups are untouched.  A non-finite state_in poisons from sample 0.
 * x, y DEVICE [groups, channels, T] of dtype (y may alias x); gain DEVICE [groups, T] of dtype or null; open DEVICE [groups, T]
 * bytes (0 / 1) or null; state_in / state_out DEVICE [groups, 3] float64 (g, open, c) or null (start state in / no state out);
 * state_out is the triple at T - 1, with c = 0 whenever closed, and needs its own buffer.
 * Both recursions are associative scans (the decision over summaries (S0, S1, L, allquiet) of a run, the gain over affine maps
 * with the coefficient product carried), so a group's row is cut into tiles of 2048 samples and the tiles into `segments` runs
 * (tfx_gate_plan_info; 0 = chosen from groups and T, any other value is clamped to the tile count).  segments == 1 is one
 * launch that reads x once and writes y once; otherwise three launches (decision summaries, gain summaries, result): x is read
 * three times and `scratch` -- DEVICE, scratch_bytes of the plan, may be null for one segment -- carries the summaries across
 * the launch boundaries.  No workgroup waits for another, no atomics.  The open track and the (open, c) of the end state are
 * the per-sample loop's bit for bit under any tiling and any `segments`; the gain follows the association of the scan: results
 * for different `segments` agree to float64 round-off, within 8 * 2^-53 * min(T, 1 / (1 - max(alpha_a, alpha_r))) of the
 * exact recursion.  With alpha_a = alpha_r = 0 the gain is exactly 1 or r.  A group's bits depend on (T, segments) and its own
 * samples alone.  Arguments are checked before the device is touched.  T == 0 copies state_in (or the start state) to state_out.
 * ------------------------------------------------------------------------- */
int tfx_gate_forward(const void *x, void *y, void *gain_or_null, unsigned char *open_or_null, int dtype, int64_t groups,
                     int64_t channels, int64_t T, double p_open, double p_close, double range, int64_t hold, double alpha_a,
                     double alpha_r, const double *state_in, double *state_out, int64_t segments, void *scratch, tfx_stream_t stream);
/* what tfx_gate_forward does (host-only, same checks on the sizes): samples per tile (2048), tiles per group, the segments it
 * takes for the request `segments`, the tiles of the longest segment (the first tiles mod segments hold one more than the rest)
 * and the bytes of `scratch` (0 for one segment) */
int tfx_gate_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t segments, int64_t *tile, int64_t *tiles,
                       int64_t *segments_out, int64_t *seg_tiles, int64_t *scratch_bytes);

/* ---------------------------------------------------------------------------
 * tfx_stft_forward -- short-time Fourier transform of every row of x [rows, T] (torch.stft's onesided result).  With
 * M = n_fft / 2, frames = 1 + (T + 2 pad - n_fft) / hop and xp the row extended by `pad` samples at each end (reflected:
 * xp[-i] = x[i], xp[T - 1 + i] = x[T - 1 - i], needs pad < T; or zeros), frame f and bin k <= M:
 *   1. s[i] = dtype(w[i] * xp[f hop + i - pad]), i < n_fft: ONE rounded product per sample, in the signal's dtype; w is `window`
 *      [win_length] centred in zeros ((n_fft - win_length) / 2 on the left), ones when window is null.  The product is always
 *      formed, so a non-finite sample under a zero of the window is NaN, as in torch.
 *   2. X[f, k] = sum_i s[i] exp(-2 pi i k i / n_fft), times n_fft^-1/2 when `normalized` (one more rounding per component)
 *   3. out[row, f, k] = X (power 0: complex, interleaved re / im of dtype), |X| (power 1) or |X|^2 (power 2), of dtype, formed
 *      in registers from the complex value: re * re + im * im, and its correctly rounded square root.
 * x, window DEVICE; out DEVICE [rows, frames, M + 1], contiguous (torch.stft returns the transpose of the last two axes as a
 * view of just this buffer).  One launch, x read once, nothing but out written: a workgroup stages the span of its
 * frames_per_workgroup consecutive frames in LDS, the padding being part of that load's addressing.  Each frame is transformed
 * on its own by threads_per_frame threads (an M-point complex transform of the even / odd samples and the real-input
 * post-twiddle; all twiddles are tables computed in double and rounded once), so a frame's bits depend on its n_fft samples and
 * the window alone: not on its index, its row, hop, its place in the workgroup or the batch.  A NaN sample makes exactly the
 * frames that hold it (through the reflected edge too) non-finite in every bin; so does an Inf, and it turns into NaN on the way
 * (Inf - Inf, Inf * 0).  Error: ||Xhat - X||_2 over a frame's bins <= 8 u (log2 n_fft + 2) sqrt(n_fft) ||s||_2, u = 2^-24 /
 * 2^-53, X being the exact transform of the rounded s.
 * Served: n_fft in {256, 512, 1024, 2048, 4096}, pad_mode constant or reflect (any pad_mode when pad == 0), 0 <= pad <= n_fft,
 * hop >= 1, 1 <= win_length <= n_fft; anything else is refused (tfx_stft_plan_info says route 0: the caller takes torch.stft).
 * Arguments are checked before the device is touched.
 * ------------------------------------------------------------------------- */
enum tfx_stft_pad { TFX_STFT_PAD_CONSTANT = 0, TFX_STFT_PAD_REFLECT = 1, TFX_STFT_PAD_REPLICATE = 2, TFX_STFT_PAD_CIRCULAR = 3 };
int tfx_stft_forward(const void *x, const void *window_or_null, void *out, int dtype, int64_t rows, int64_t T, int64_t n_fft,
                     int64_t hop, int64_t win_length, int64_t pad, int pad_mode, int power, int normalized, tfx_stream_t stream);
/* what an STFT of this geometry does (host-only, same checks on the sizes; pad = n_fft / 2 when `center`): route (1: the LDS
 * kernel, 0: not served -- another n_fft, a two-sided result, another pad_mode), frames per row and, for route 1, the frames
 * and threads per frame of a workgroup, its LDS bytes and the workgroups of the launch (rows * ceil(frames / frames per
 * workgroup); 0 for route 0) */
int tfx_stft_plan_info(int64_t n_fft, int64_t hop, int64_t win_length, int64_t T, int64_t rows, int dtype, int center, int pad_mode,
                       int onesided, int *route, int64_t *frames, int64_t *frames_per_workgroup, int64_t *threads_per_frame,
                       int64_t *lds_bytes, int64_t *workgroups);

/* ---------------------------------------------------------------------------
 * tfx_istft_forward -- inverse short-time Fourier transform of every row of spec [rows, frames, M + 1] (M = n_fft / 2; complex,
 * interleaved re / im of dtype; the buffer tfx_stft_forward writes), torch.istft's onesided semantics:
 *   1. s_f = irfft(spec[row, f, :], n_fft), scaled once by 1 / n_fft (n_fft^-1/2 when `normalized`); the imaginary parts of
 *      bins 0 and M are not read.
 *   2. num[t] = sum_f dtype(w[t - f hop] * s_f[t - f hop]),  env[t] = sum_f dtype(w[t - f hop]^2): over the frames that cover t,
 *      in ascending frame order, starting from zero, in dtype; w is `window` [win_length] centred in n_fft zeros, ones when
 *      window is null.  Both products are always formed, so a non-finite frame reaches every sample it covers, also under a
 *      zero of the window.
 *   3. out[row, t - pad] = num[t] / env[t] for 0 <= t - pad < length; positions past the last frame ((frames - 1) hop + n_fft)
 *      read 0.  length = -1 is the natural length (frames - 1) hop + n_fft - 2 pad.
 * spec, window, out [rows, length] and flag (one int) DEVICE.  *flag is cleared on the stream, then set to 1 by every thread
 * that meets !(|env[t]| > 1e-11) on a returned position under a frame (torch's "window overlap add min" condition): the caller
 * reads it when it may synchronise.  One launch: a workgroup owns `tile` consecutive output samples of one row, transforms the
 * frames that cover them (frames_per_batch at a time, threads_per_frame threads each, the forward transform's stages and
 * tables run on the conjugate) and adds them in frame order in registers: no atomics, nothing but out and flag written.  A
 * frame that straddles two tiles is transformed by both, to the same bits, so a sample's bits depend on the frames that cover
 * it and the window alone -- not on the tile, the row, the batch or the frame count.
 * Served: n_fft in {256, 512, 1024, 2048, 4096}, 1 <= hop <= win_length <= n_fft, 0 <= pad <= n_fft; anything else is refused
 * (tfx_istft_plan_info says route 0: the caller takes torch.istft).  Arguments are checked before the device is touched.
 * ------------------------------------------------------------------------- */
int tfx_istft_forward(const void *spec, const void *window_or_null, void *out, int *flag, int dtype, int64_t rows, int64_t frames,
                      int64_t n_fft, int64_t hop, int64_t win_length, int64_t pad, int64_t length, int normalized, tfx_stream_t stream);
/* what an ISTFT of this geometry does (host-only, same checks on the sizes; pad = n_fft / 2 when `center`, length -1 = natural):
 * route (1: the LDS kernel, 0: not served -- another n_fft, a two-sided spectrum), the output length and, for route 1, the
 * samples of a tile, the frames of a batch, the threads per frame, the LDS bytes of a workgroup, the workgroups of the launch
 * (rows * ceil(length / tile); 0 for route 0) and the share of the transforms that a neighbouring tile runs too:
 * e / (tile / hop + e), e = ceil(n_fft / hop) - 1 */
int tfx_istft_plan_info(int64_t n_fft, int64_t hop, int64_t win_length, int64_t frames, int64_t rows, int dtype, int center,
                        int64_t length, int onesided, int *route, int64_t *out_length, int64_t *tile, int64_t *frames_per_batch,
                        int64_t *threads_per_frame, int64_t *lds_bytes, int64_t *workgroups, double *redundant_share);

/* ---------------------------------------------------------------------------
 * tfx_sum_forward -- y = sum_i xs[i]  (the accumulate of
 * ParallelFilterCombination.forward, src/torchfx/filter/__base.py:1019-1026).
 * xs_host: HOST array of n DEVICE pointers, each [numel] of dtype.
 * ------------------------------------------------------------------------- */
int tfx_sum_forward(const void *const *xs_host, int n, void *y, int dtype,
                    int64_t numel, tfx_stream_t stream);

/* ---------------------------------------------------------------------------
 * Elementwise effects that sit between filters in a pipeline.
 *
 * tfx_gain_forward -- Gain.forward, src/torchfx/effect.py:361-383:  y = x * gain, then (clamp != 0)
 *   clip to [-1, 1].  `gain` is the LINEAR factor (the host layer maps "db" / "power" through
 *   10^(g/20), effect.py:132-136,372-378) and is rounded to the signal dtype like torch does for
 *   tensor * python_float.  y may alias x (pure elementwise).
 *
 * tfx_stat_forward -- the reductions behind the normalization strategies (effect.py:678-790):
 *   mode TFX_STAT_ABSMAX: max|x| ;  TFX_STAT_RMS: sqrt(mean(x^2)) (float64 accumulation, deterministic).
 *   per_row != 0: one value per row -> out_dev[C];  else one value over all C*T -> out_dev[1].
 *   out_dev: DEVICE float64.  NaN anywhere gives NaN (torch.max semantics).
 *
 * tfx_normalize_forward -- Normalize.forward with PeakNormalizationStrategy (mode ABSMAX, per_row 0,
 *   effect.py:696-698), PerChannelNormalizationStrategy (ABSMAX, per_row 1, :775-786) or
 *   RMSNormalizationStrategy (RMS, per_row 0, :719-721):  y = s > 0 ? (x / s) * peak : x, evaluated in
 *   the signal dtype in that order.  The statistic never leaves the device (the reference's
 *   `if max_val > 0` is a blocking host read).  y may alias x.
 * ------------------------------------------------------------------------- */
enum tfx_stat { TFX_STAT_ABSMAX = 0, TFX_STAT_RMS = 1 };
int tfx_gain_forward(const void *x, void *y, int dtype, int64_t numel, double gain, int clamp,
                     tfx_stream_t stream);
int tfx_stat_forward(const void *x, int dtype, int64_t C, int64_t T, int mode, int per_row,
                     double *out_dev, tfx_stream_t stream);
int tfx_normalize_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, int mode, int per_row,
                          double peak, tfx_stream_t stream);
/* the geometry of the launches above, of tfx_normalize_apply, tfx_sum_forward and the two tfx_delay_line entries for rows of T
 * samples of `dtype` (host-only, from the launches' own constants): vec = samples per 16-byte vector (4 / 2); tile = samples
 * one workgroup of an elementwise pass covers (1024 / 512); group = samples one workgroup of the statistics' first stage
 * reduces to one partial (8 tiles); groups = partials per row of T samples; finish_threads = threads of the second stage's one
 * workgroup per row (1024: a row with more partials takes strided trips); stream_tile = samples per workgroup of
 * tfx_delay_line_stream_forward (1024 for both dtypes) */
int tfx_effects_plan_info(int64_t T, int dtype, int64_t *vec, int64_t *tile, int64_t *group, int64_t *groups,
                          int64_t *finish_threads, int64_t *stream_tile);

/* ---------------------------------------------------------------------------
 * The data-format edge: decoded audio is INTERLEAVED frames [F, C]; the filter
 * path works on PLANAR rows [C, F].  The reference transposes on the host (`data_np.T.copy()`,
 * src/torchfx/wave.py:448-452, and `.numpy().T` before writing, :566-573); these do it on the device so
 * the host buffer can be uploaded as it is, in chunks, and 16-bit PCM can cross PCIe as 2-byte samples.
 *
 * tfx_deinterleave_forward: in DEVICE [F, C] of float32 (in_kind TFX_PCM_F32) or int16 (TFX_PCM_S16,
 *   converted as v * scale; scale = 1/32768 is libsndfile's normalisation);
 *   out DEVICE float32 rows of pitch ld_out: out[c * ld_out + f_base + f] = in[f * C + c].
 *   f_base / ld_out let a file be uploaded chunk by chunk into one [C, F_total] tensor.
 * tfx_interleave_forward: the inverse, out[f * C + c] = in[c * ld_in + f_base + f], float32.
 * ------------------------------------------------------------------------- */
enum tfx_pcm { TFX_PCM_F32 = 0, TFX_PCM_S16 = 1 };
int tfx_deinterleave_forward(const void *in, int in_kind, void *out, int64_t F, int64_t C, int64_t ld_out,
                             int64_t f_base, double scale, tfx_stream_t stream);
int tfx_interleave_forward(const void *in, void *out, int64_t F, int64_t C, int64_t ld_in, int64_t f_base,
                           tfx_stream_t stream);

/* Timing hooks for bench.py: HIP events recorded on the SAME stream the
 * kernels are launched on (torch.cuda.Event only sees torch's current stream).
 * tfx_prof_enable(1) makes every kernel launch inside the library bracket
 * itself with events; tfx_prof_collect() synchronises and returns, per kernel
 * name, call count and total milliseconds as a JSON string (static buffer). */
int tfx_prof_enable(int on);
const char *tfx_prof_collect(void);

/* Drop all cached plans / device workspaces (tests, memory pressure). */
int tfx_clear_caches(void);

/* Workspace under the caller's control.  The overlap-save pipelines keep device workspaces between calls (the default chain
 * step: three lanes x up to 3.75 GB); by default they come from hipMalloc / hipFree.  A host that runs its own device allocator
 * installs it here -- the torch module (csrc/ext/torchfx_ext.cpp) routes the workspaces through PyTorch's caching allocator, so
 * torch.cuda.memory_allocated(), its free-cached-blocks-and-retry and its OutOfMemoryError cover them (the reference allocates
 * every temporary as a torch tensor: src/torchfx/filter/_fftconv.py:119-140).
 *   alloc_fn(bytes, device, stream, ctx) -> device pointer, or NULL when it cannot (the pipeline then asks for a smaller slab:
 *       fewer frame pairs per launch, down to 8; below that the call fails with "out of device memory")
 *   free_fn(ptr, device, ctx)               called after a device synchronise
 * Both NULL restores hipMalloc / hipFree.  Buffers held at the time of the call keep the allocator they came from.
 * tfx_workspace_bytes(): bytes of workspace held right now (all streams and devices); tfx_clear_caches() releases them. */
typedef void *(*tfx_alloc_fn)(size_t bytes, int device, void *stream, void *ctx);
typedef void (*tfx_free_fn)(void *ptr, int device, void *ctx);
int tfx_set_workspace_allocator(tfx_alloc_fn alloc_fn, tfx_free_fn free_fn, void *ctx);
int64_t tfx_workspace_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* TORCHFX_HIP_H */
