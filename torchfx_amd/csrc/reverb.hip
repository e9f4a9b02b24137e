// reverb.hip -- Freeverb (Jezar at Dreampoint, public domain): per bank (one channel of one batch item) NC parallel feedback
// combs with a one-pole low-pass in the loop, summed, then NA Schroeder all-passes in series (tfx_freeverb_forward;
// include/torchfx_hip.h has the full contract).  All arithmetic in float64:
//   u[n]   = gin (x_0[n] + ... + x_{C-1}[n]),  gin = input_gain 2 / C
//   comb k:      o[n] = w[n - D];  f[n] = d2 o[n] + d1 f[n-1];  w[n] = u[n] + fb f[n]
//   s_0[n] = ((o_0[n] + o_1[n]) + o_2[n]) + ...
//   all-pass j:  b[n] = v[n - D];  s_{j+1}[n] = b[n] - s_j[n];  v[n] = s_j[n] + g b[n]
//   y_c[n] = dtype(dry x_c[n] + wet1 r_c[n] + wet2 r_{1-c}[n]),  r = s_NA
//
// Work unit.  One workgroup of FV_THREADS = 512 threads (8 waves) owns a bank from its first sample to its last; no workgroup
// waits for another, no atomics.  A delay line of D samples is a ring of D float64 words: sample n lives in slot n mod D, so the
// word a step reads (n - D) is the word it overwrites (n).  A comb reads only samples at least D old, hence a block of
// B = min(min_k D_k, FV_BLOCK) samples has every comb output o_k at hand when it starts:
//   1  all threads:   u[i] (coalesced signal reads) and the comb sum s_0[i] for the block, into two LDS slots of B words
//   2  wave k:        comb k.  Lane l owns E consecutive samples (E odd: the lanes' LDS words fall on different banks), folds
//                     them into the affine map f -> a f + s, the maps are scanned over the 64 lanes (Kogge-Stone, shuffles),
//                     the lane runs its samples again from its true f and writes w in place; lane 63's f is the next block's
//   3  all threads:   all-pass j over the block: the samples i, i + D_j, i + 2 D_j, ... share one word of the ring, a thread walks
//                     them with that word in a register, the min(D_j, B) walks run in parallel
//   4  all threads:   the mix (one launch: C = 1 or wet2 = 0) or r to a float64 workspace for freeverb_mix_kernel
// with a barrier after phases 1 and 2 and after every all-pass.  The signal is fetched one block ahead.  D = 1 gives blocks (or
// walks) of one sample: correct, not fast.
//
// The rings live in LDS when the bank's lines fit beside the two slots (LINES_LDS; the default tunings up to 48 kHz), else in a
// workgroup-private stretch of the caller's workspace (96 / 192 kHz, long delays): the same code over another pointer.
// The state is in time order (oldest first), not ring order: the rings are loaded at slot 0 and written back rotated.
#include "common.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <algorithm>
#include <cmath>

namespace tfx {

constexpr int FV_THREADS = 512, FV_WAVES = FV_THREADS / 64;
constexpr int FV_MAX_COMBS = 8, FV_MAX_ALLPASS = 4, FV_LINES = FV_MAX_COMBS + FV_MAX_ALLPASS;
constexpr int FV_BLOCK = 1024;                     // the longest block: two slots of 8 KB
constexpr int64_t FV_MAX_DELAY = 65536;
constexpr int64_t FV_LDS_BUDGET = 159 * 1024;      // of the 160 KB of a CU; the rest holds the small tables

constexpr int FV_Q = FV_BLOCK / FV_THREADS;        // samples of a block per thread
constexpr int FV_E = (FV_BLOCK / 64) | 1;          // samples of a block per lane of a comb's wave, odd

static_assert(FV_WAVES == FV_MAX_COMBS, "one wave per comb");
static_assert(FV_Q * FV_THREADS == FV_BLOCK, "every thread owns FV_Q samples of a full block");

template <typename T> struct FvArgs {
    const T *x;                 // [batch, C, T_]
    T *y;                       // [batch, C, Tn]
    double *r;                  // [batch * C, Tn]: the wet signal for the mix launch, or null (this launch mixes)
    double *lines;              // [batch * C, line_words] (global placement) or null
    const double *state_in;     // [batch * C, S] or null (silence)
    double *state_out;          // [batch * C, S] or null
    int64_t T_, Tn, S, line_words;
    int C, NC, NA, B;
    int Dc[2][FV_MAX_COMBS], Da[2][FV_MAX_ALLPASS];
    double fb, d1, d2, g, gin, dry, wet;
};

// D[c][k] without a dynamically indexed copy of the argument block
template <typename T> __device__ __forceinline__ int fv_delay(const FvArgs<T> &p, int c, int i)
{
    int v = 0;
#pragma unroll
    for (int k = 0; k < FV_MAX_COMBS; ++k)
        if (i == k) v = c ? p.Dc[1][k] : p.Dc[0][k];
#pragma unroll
    for (int j = 0; j < FV_MAX_ALLPASS; ++j)
        if (i == FV_MAX_COMBS + j) v = c ? p.Da[1][j] : p.Da[0][j];
    return v;
}

template <typename T, bool LINES_LDS>
__global__ void __launch_bounds__(FV_THREADS) freeverb_kernel(const FvArgs<T> p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fv_lds_raw[];
    __shared__ int sD[FV_LINES], sOff[FV_LINES], sPos[FV_LINES];
    double *ub = (double *)fv_lds_raw, *sb = ub + p.B;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t bank = blockIdx.x, item = bank / p.C;
    const int c = (int)(bank % p.C);
    const int NC = p.NC, NA = p.NA, NL = FV_MAX_COMBS + NA;
    double *line = LINES_LDS ? sb + p.B : p.lines + bank * p.line_words;

    // the tables: delay, ring offset and position (n mod D) of every line; combs at 0 .. NC-1, all-passes at 8 .. 8+NA-1
    if (t == 0) {
        int off = 0;
        for (int i = 0; i < NL; ++i) {
            const int D = (i < NC || i >= FV_MAX_COMBS) ? fv_delay(p, c, i) : 0;
            sD[i] = D, sOff[i] = off, sPos[i] = 0;
            off += D;
        }
    }
    __syncthreads();

    // the rings at slot 0 from the state (time order), or silence; a comb's state is its D words of w, then f
    const double *sin = p.state_in ? p.state_in + bank * p.S : nullptr;
    double f = 0.0;                                                   // wave k < NC: comb k's low-pass state
    {
        int soff = 0;
        for (int i = 0; i < NL; ++i) {
            const int D = sD[i];
            if (D == 0) continue;
            double *ln = line + sOff[i];
            for (int j = t; j < D; j += FV_THREADS) ln[j] = sin ? sin[soff + j] : 0.0;
            if (i < NC) {
                if (sin && i == wave) f = sin[soff + D];
                soff += D + 1;
            } else {
                soff += D;
            }
        }
    }
    __syncthreads();

    // This thread's samples of a block (i = t and t + 512), fetched one block ahead and left as they came until the next block
    // converts them, so that the memory round trip runs under the block before: x0 / x1 the item's channels.
    const T *xr = p.x + item * p.C * p.T_;
    T nx0[FV_Q], nx1[FV_Q];
    const auto fetch = [&](int64_t n0) {
#pragma unroll
        for (int q = 0; q < FV_Q; ++q) {
            const int i = t + q * FV_THREADS;
            const int64_t n = n0 + i;
            nx0[q] = nx1[q] = (T)0;
            if (i < p.B && n < p.T_) {
                nx0[q] = xr[n];
                if (p.C == 2) nx1[q] = xr[p.T_ + n];
            }
        }
    };
    fetch(0);
    for (int64_t n0 = 0; n0 < p.Tn; n0 += p.B) {
        const int nb = (int)(p.Tn - n0 < p.B ? p.Tn - n0 : p.B);
        double own[FV_Q], sum[FV_Q];                                  // its own channel's for the mix, the channel sum for the feed
#pragma unroll
        for (int q = 0; q < FV_Q; ++q) {
            const double x0 = (double)nx0[q], x1 = (double)nx1[q];
            own[q] = c ? x1 : x0;
            sum[q] = p.C == 2 ? x0 + x1 : x0;
        }
        if (n0 + p.B < p.Tn) fetch(n0 + p.B);

        // ---- 1: the feed and the comb sum
#pragma unroll
        for (int q = 0; q < FV_Q; ++q) {
            const int i = t + q * FV_THREADS;
            if (i < nb) {
                ub[i] = p.gin * sum[q];
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < FV_MAX_COMBS; ++k) {
                    if (k < NC) {
                        const int D = sD[k];
                        int slot = sPos[k] + i;
                        if (slot >= D) slot -= D;
                        const double o = line[sOff[k] + slot];
                        s = k == 0 ? o : s + o;
                    }
                }
                sb[i] = s;
            }
        }
        __syncthreads();

        // ---- 2: comb `wave`; the lane's words of the line and of the feed sit in registers for both runs
        if (wave < NC) {
            const int D = sD[wave], pos = sPos[wave];
            double *ln = line + sOff[wave];
            const int E = ((nb + 63) >> 6) | 1;
            const int i0 = min(lane * E, nb), cnt = min(E, nb - i0);
            int slot0 = pos + i0;
            if (slot0 >= D) slot0 -= D;
            double o[FV_E], uu[FV_E];
#pragma unroll
            for (int e = 0; e < FV_E; ++e) {
                int slot = slot0 + e;
                if (slot >= D) slot -= D;
                o[e] = e < cnt ? ln[slot] : 0.0;
                uu[e] = e < cnt ? ub[i0 + e] : 0.0;
            }
            double a = 1.0, s = 0.0;
#pragma unroll
            for (int e = 0; e < FV_E; ++e) {
                if (e < cnt) {
                    s = p.d1 * s + p.d2 * o[e];
                    a *= p.d1;
                }
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double ap = __shfl_up(a, 1 << j), sp = __shfl_up(s, 1 << j);
                if (lane >= (1 << j)) {
                    s = a * sp + s;
                    a = a * ap;
                }
            }
            const double aex = __shfl_up(a, 1), sex = __shfl_up(s, 1);       // the lanes in front of this one
            double fl = lane > 0 ? aex * f + sex : f;
#pragma unroll
            for (int e = 0; e < FV_E; ++e) {
                if (e < cnt) {
                    int slot = slot0 + e;
                    if (slot >= D) slot -= D;
                    fl = p.d2 * o[e] + p.d1 * fl;
                    ln[slot] = uu[e] + p.fb * fl;
                }
            }
            f = __shfl(fl, 63);
            if (lane == 0) {                                         // nobody else reads this comb's position before the barrier
                int np = pos + nb;
                sPos[wave] = np >= D ? np - D : np;
            }
        }
        __syncthreads();

        // ---- 3: the all-passes, in place on the block's slot.  The samples i, i + D, i + 2D, ... of a block share one word of
        // the ring, so a thread walks them with that word in a register and a stage needs no barrier but the one at its end.
        for (int j = 0; j < NA; ++j) {
            const int D = sD[FV_MAX_COMBS + j], pos = sPos[FV_MAX_COMBS + j];
            double *ln = line + sOff[FV_MAX_COMBS + j];
            const int m = min(D, nb);
            for (int r = t; r < m; r += FV_THREADS) {
                int slot = pos + r;
                if (slot >= D) slot -= D;
                double b = ln[slot];
                for (int i = r; i < nb; i += D) {
                    const double s = sb[i];
                    sb[i] = b - s;
                    b = s + p.g * b;
                }
                ln[slot] = b;
            }
            __syncthreads();
            if (t == 0) sPos[FV_MAX_COMBS + j] = (pos + nb) % D;
        }

        // ---- 4: out.  A thread reads the words of the slot it overwrites in the next block's phase 1: no barrier in between.
#pragma unroll
        for (int q = 0; q < FV_Q; ++q) {
            const int i = t + q * FV_THREADS;
            if (i < nb) {
                if (p.r) p.r[bank * p.Tn + n0 + i] = sb[i];
                else p.y[bank * p.Tn + n0 + i] = (T)(p.dry * own[q] + p.wet * sb[i]);
            }
        }
    }
    __syncthreads();

    // the state, oldest first: the ring from its position on
    if (p.state_out) {
        double *so = p.state_out + bank * p.S;
        int soff = 0;
        for (int i = 0; i < NL; ++i) {
            const int D = sD[i];
            if (D == 0) continue;
            const double *ln = line + sOff[i];
            const int pos = sPos[i];
            for (int j = t; j < D; j += FV_THREADS) {
                int slot = pos + j;
                if (slot >= D) slot -= D;
                so[soff + j] = ln[slot];
            }
            if (i < NC) {
                if (i == wave && lane == 0) so[soff + D] = f;
                soff += D + 1;
            } else {
                soff += D;
            }
        }
        for (int64_t j = soff + t; j < p.S; j += FV_THREADS) so[j] = 0.0;     // a shorter bank's row ends in zeros
    }
}

// y_c = dtype(dry x_c + wet1 r_c + wet2 r_{1-c}) for C = 2; one thread per sample of an item, `tiles` workgroups per item
template <typename T>
__global__ void __launch_bounds__(256) freeverb_mix_kernel(const T *x, T *y, const double *r, int64_t T_, int64_t Tn, int64_t tiles,
                                                           double dry, double wet1, double wet2)
{
    const int64_t item = blockIdx.x / tiles;
    const int64_t n = (int64_t)(blockIdx.x % tiles) * 256 + threadIdx.x;
    if (n >= Tn) return;
    const double r0 = r[(item * 2) * Tn + n], r1 = r[(item * 2 + 1) * Tn + n];
    const double x0 = n < T_ ? (double)x[(item * 2) * T_ + n] : 0.0, x1 = n < T_ ? (double)x[(item * 2 + 1) * T_ + n] : 0.0;
    y[(item * 2) * Tn + n] = (T)(dry * x0 + wet1 * r0 + wet2 * r1);
    y[(item * 2 + 1) * Tn + n] = (T)(dry * x1 + wet1 * r1 + wet2 * r0);
}

struct FvPlan {
    int64_t banks, Tn, B, state_len, line_words, lds_bytes, launches, lines_bytes, r_bytes;
    int placement;              // TFX_FREEVERB_LINES_LDS / _GLOBAL
};

// sizes and delays alone (host-only)
static FvPlan freeverb_plan(const char *what, int64_t batch, int64_t channels, int64_t T, int64_t tail, const int64_t *comb_delays,
                            int64_t NC, const int64_t *allpass_delays, int64_t NA, double wet2)
{
    TFX_CHECK(batch >= 0 && T >= 0 && tail >= 0, "%s: negative size", what);
    TFX_CHECK(channels == 1 || channels == 2, "%s: channels must be 1 or 2, got %lld", what, (long long)channels);
    TFX_CHECK(NC >= 1 && NC <= FV_MAX_COMBS, "%s: the number of combs must be in [1, %d], got %lld", what, FV_MAX_COMBS, (long long)NC);
    TFX_CHECK(NA >= 0 && NA <= FV_MAX_ALLPASS, "%s: the number of all-passes must be in [0, %d], got %lld", what, FV_MAX_ALLPASS,
              (long long)NA);
    TFX_CHECK(comb_delays && (NA == 0 || allpass_delays), "%s: null delay table", what);
    TFX_CHECK(T <= INT64_MAX / 64 - tail && (batch == 0 || T + tail <= INT64_MAX / 64 / batch), "%s: size overflows", what);
    TFX_CHECK(batch * channels < (1ll << 31), "%s: size overflows", what);
    FvPlan pl{};
    pl.banks = batch * channels;
    pl.Tn = T + tail;
    int64_t minD = FV_MAX_DELAY;
    for (int64_t c = 0; c < channels; ++c) {
        int64_t words = 0, st = 0;
        for (int64_t k = 0; k < NC; ++k) {
            const int64_t D = comb_delays[c * NC + k];
            TFX_CHECK(D >= 1 && D <= FV_MAX_DELAY, "%s: comb delays must be in [1, %lld] samples, got %lld", what, (long long)FV_MAX_DELAY,
                      (long long)D);
            words += D, st += D + 1;
            minD = std::min(minD, D);
        }
        for (int64_t j = 0; j < NA; ++j) {
            const int64_t D = allpass_delays[c * NA + j];
            TFX_CHECK(D >= 1 && D <= FV_MAX_DELAY, "%s: all-pass delays must be in [1, %lld] samples, got %lld", what,
                      (long long)FV_MAX_DELAY, (long long)D);
            words += D, st += D;
        }
        pl.line_words = std::max(pl.line_words, words);
        pl.state_len = std::max(pl.state_len, st);
    }
    pl.B = std::min<int64_t>(minD, FV_BLOCK);
    const int64_t slots = 2 * pl.B * (int64_t)sizeof(double), in_lds = slots + pl.line_words * (int64_t)sizeof(double);
    pl.placement = in_lds <= FV_LDS_BUDGET ? TFX_FREEVERB_LINES_LDS : TFX_FREEVERB_LINES_GLOBAL;
    pl.lds_bytes = pl.placement == TFX_FREEVERB_LINES_LDS ? in_lds : slots;
    pl.launches = (channels == 2 && wet2 != 0.0) ? 2 : 1;
    pl.lines_bytes = pl.placement == TFX_FREEVERB_LINES_GLOBAL ? pl.banks * pl.line_words * (int64_t)sizeof(double) : 0;
    pl.r_bytes = pl.launches == 2 ? pl.banks * pl.Tn * (int64_t)sizeof(double) : 0;
    return pl;
}

void freeverb_plan_info(int64_t batch, int64_t channels, int64_t T, int64_t tail, const int64_t *comb_delays_host, int64_t NC,
                        const int64_t *allpass_delays_host, int64_t NA, double wet2, int64_t *block, int *placement,
                        int64_t *state_len, int64_t *launches, int64_t *workspace_bytes)
{
    const FvPlan pl = freeverb_plan("freeverb_plan_info", batch, channels, T, tail, comb_delays_host, NC, allpass_delays_host, NA, wet2);
    *block = pl.B;
    *placement = pl.placement;
    *state_len = pl.state_len;
    *launches = pl.launches;
    *workspace_bytes = pl.lines_bytes + pl.r_bytes;
}

template <typename T, bool LINES_LDS> static void freeverb_launch_at(const FvArgs<T> &p, const FvPlan &pl, hipStream_t stream)
{
    static bool attr_done[TFX_MAX_DEVICES] = {};
    bool &done = attr_done[current_device()];
    if (!done) {
        TFX_HIP(hipFuncSetAttribute((const void *)freeverb_kernel<T, LINES_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)FV_LDS_BUDGET));
        done = true;
    }
    ProfScope ps(LINES_LDS ? "freeverb_kernel_lds" : "freeverb_kernel_global", stream);
    hipLaunchKernelGGL((freeverb_kernel<T, LINES_LDS>), dim3((unsigned)pl.banks), dim3(FV_THREADS), (size_t)pl.lds_bytes, stream, p);
    TFX_HIP(hipGetLastError());
}

template <typename T>
static void freeverb_launch(FvArgs<T> p, const void *x, void *y, int64_t batch, double dry, double wet1, double wet2, void *workspace,
                            const FvPlan &pl, hipStream_t stream)
{
    p.x = (const T *)x;
    p.y = (T *)y;
    p.lines = pl.lines_bytes ? (double *)workspace : nullptr;
    p.r = pl.r_bytes ? (double *)((char *)workspace + pl.lines_bytes) : nullptr;
    p.dry = dry;
    p.wet = p.C == 1 ? wet1 + wet2 : wet1;
    if (pl.placement == TFX_FREEVERB_LINES_LDS) freeverb_launch_at<T, true>(p, pl, stream);
    else freeverb_launch_at<T, false>(p, pl, stream);
    if (pl.launches == 2) {
        ProfScope ps("freeverb_mix_kernel", stream);
        const int64_t tiles = ceil_div(pl.Tn, 256);
        hipLaunchKernelGGL((freeverb_mix_kernel<T>), dim3((unsigned)(batch * tiles)), dim3(256), 0, stream, p.x, p.y, p.r, p.T_, pl.Tn,
                           tiles, dry, wet1, wet2);
        TFX_HIP(hipGetLastError());
    }
}

void freeverb_forward(const void *x, void *y, int dtype, int64_t batch, int64_t channels, int64_t T, int64_t tail,
                      const int64_t *comb_delays_host, int64_t NC, const int64_t *allpass_delays_host, int64_t NA, double feedback,
                      double damp, double allpass_gain, double input_gain, double dry_gain, double wet1, double wet2,
                      const double *state_in, double *state_out, void *workspace, hipStream_t stream)
{
    const char *what = "freeverb_forward";
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: bad dtype %d", what, dtype);
    const FvPlan pl = freeverb_plan(what, batch, channels, T, tail, comb_delays_host, NC, allpass_delays_host, NA, wet2);
    TFX_CHECK(std::fabs(feedback) < 1.0, "%s: |feedback| must be < 1, got %g", what, feedback);
    TFX_CHECK(damp >= 0.0 && damp < 1.0, "%s: damp must be in [0, 1), got %g", what, damp);
    TFX_CHECK(std::fabs(allpass_gain) < 1.0, "%s: |allpass_gain| must be < 1, got %g", what, allpass_gain);
    TFX_CHECK(std::isfinite(input_gain) && std::isfinite(dry_gain) && std::isfinite(wet1) && std::isfinite(wet2),
              "%s: the gains must be finite", what);
    TFX_CHECK(pl.launches == 1 || batch * ceil_div(pl.Tn, 256) < (1ll << 24), "%s: the mix launch takes at most 2^32 samples per call",
              what);
    TFX_CHECK(pl.banks * pl.Tn == 0 || (y && (T == 0 || x)), "%s: null pointer", what);
    TFX_CHECK(pl.banks * pl.Tn == 0 || pl.lines_bytes + pl.r_bytes == 0 || workspace, "%s: this call needs a workspace of %lld bytes",
              what, (long long)(pl.lines_bytes + pl.r_bytes));
    TFX_CHECK(!state_out || state_out != state_in, "%s: the new state needs its own buffer", what);
    if (pl.banks == 0) return;
    if (pl.Tn == 0) {                            // nothing in, nothing out: the state moves on unchanged
        const size_t bytes = (size_t)(pl.banks * pl.state_len) * sizeof(double);
        if (state_out) {
            if (state_in) TFX_HIP(hipMemcpyAsync(state_out, state_in, bytes, hipMemcpyDeviceToDevice, stream));
            else TFX_HIP(hipMemsetAsync(state_out, 0, bytes, stream));
        }
        return;
    }
    const auto fill = [&](auto &p) {
        p.state_in = state_in; p.state_out = state_out;
        p.T_ = T; p.Tn = pl.Tn; p.S = pl.state_len; p.line_words = pl.line_words;
        p.C = (int)channels; p.NC = (int)NC; p.NA = (int)NA; p.B = (int)pl.B;
        for (int64_t c = 0; c < channels; ++c) {
            for (int64_t k = 0; k < NC; ++k) p.Dc[c][k] = (int)comb_delays_host[c * NC + k];
            for (int64_t j = 0; j < NA; ++j) p.Da[c][j] = (int)allpass_delays_host[c * NA + j];
        }
        p.fb = feedback; p.d1 = damp; p.d2 = 1.0 - damp; p.g = allpass_gain; p.gin = input_gain * (2.0 / (double)channels);
    };
    if (dtype == TFX_F32) {
        FvArgs<float> p{};
        fill(p);
        freeverb_launch<float>(p, x, y, batch, dry_gain, wet1, wet2, workspace, pl, stream);
    } else {
        FvArgs<double> p{};
        fill(p);
        freeverb_launch<double>(p, x, y, batch, dry_gain, wet1, wet2, workspace, pl, stream);
    }
}

}  // namespace tfx
