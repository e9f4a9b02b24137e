// compressor.hip -- feed-forward compressor with a log-domain smooth decoupled peak detector (tfx_compressor_forward;
// include/torchfx_hip.h has the full contract).  For a group of `channels` rows that share one gain curve, detector in float64:
//   p[n]  = max_ch |x[ch,n]|
//   v[n]  = the static curve's gain reduction in dB at level 20 log10 p[n] (0 under the knee; NaN for a non-finite p)
//   y1[n] = max(v[n], aR y1[n-1] + (1 - aR) v[n])                 (release)
//   yL[n] = aA yL[n-1] + (1 - aA) y1[n]                           (attack)
//   g[n]  = 10^((makeup - yL[n]) / 20);   y[ch,n] = dtype(g[n] x[ch,n])
// Both recursions are scans over a monoid.  A run of k samples acts on the incoming y1 as y -> max(M, aR^k y + B); two runs
// compose as (M1, B1) then (M2, B2; k2 samples) = (max(M2, aR^k2 M1 + B2), aR^k2 B1 + B2).  The attack stage is the affine
// y -> aA^k y + S.  No identity element is ever used (0 * -inf with aR = 0): every combine has a left operand.
//
// Work unit: scan_tile.h's, a unit being a group; both carries stay in registers, and the powers a^(8 * 2^j) the scan strides need
// come from the host (long double).  segments == 1: one launch (pass C).  Otherwise three:
//   A  every segment but the last: its release summary (M, B)                                         reads x
//   B  every segment but the last: composes the release summaries in front of it (a short loop), runs the release stage for
//      real and stores its attack summary S                                                          reads x
//   C  every segment: composes both carries, runs both stages, applies the gain                      reads x, writes y
// The three passes compute v with the same code, so the carries B and C compose are the same numbers.
// The two wave scans are written out here, not through scan_tile.h's scan_wave: through it pass C gave the same bits and
// measured 0.7 % slower on an MI355X.
#include "common.h"
#include "scan_tile.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <algorithm>
#include <cmath>

namespace tfx {

constexpr int CP_NPW = 9;                                 // a^(8 * 2^j): j < 6 the lane strides, 6 a wave, 8 a tile
constexpr int64_t CP_AUTO_BLOCKS = 1024, CP_AUTO_GROUPS = 512;

struct CpStage {
    double a, b;                // the coefficient and 1 - a
    double pw[CP_NPW];          // a^(ST_E * 2^j)
    double seg[2];              // a^(samples of a short segment), a^(samples of a long one)
};

template <typename T> struct CompArgs {
    ScanGainIO<T> io;
    const double *state_in;     // [groups, 2] (y1, yL) or null (silence)
    double *state_out;          // [groups, 2] or null
    double *scratch;            // [groups, segments, 3] (M, B, S); unused for segments == 1
    ScanCut cut;
    double th, s, w, makeup, lin_lo;
    CpStage R, A;
};

template <typename T> __device__ __forceinline__ double cp_curve(double pv, const CompArgs<T> &p)
{
    if (!(pv <= 1.7976931348623157e308)) return (double)NAN;          // NaN or Inf
    if (pv <= p.lin_lo) return 0.0;                                    // under the knee: no logarithm (lin_lo sits just below it)
    const double o = 20.0 * log10(pv) - p.th;
    if (2.0 * o <= -p.w) return 0.0;
    if (2.0 * o >= p.w) return p.s * o;
    const double u = o + 0.5 * p.w;
    return p.s * u * u / (2.0 * p.w);
}

__device__ __forceinline__ double cp_lane_power(const CpStage &st, int lane)
{
    double a = 1.0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
        if ((lane >> j) & 1) a *= st.pw[j];
    return a;
}

// PASS 0 = A, 1 = B, 2 = C
template <typename T, int PASS>
__global__ void __launch_bounds__(ST_THREADS) compressor_kernel(const CompArgs<T> p)
{
    __shared__ double slot[ST_PAD];
    __shared__ double wM[ST_WAVES], wB[ST_WAVES], wS[ST_WAVES];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const ScanSeg sg = scan_segment(p.cut, PASS == 2 ? p.cut.segments : p.cut.segments - 1);
    const int64_t grp = sg.unit, T_ = p.cut.T_;
    const int seg = sg.seg;
    const double laneR = cp_lane_power(p.R, lane), laneA = cp_lane_power(p.A, lane);

    // the carries at the segment's start: the state, then the summaries of the segments in front
    double c1 = 0.0, c2 = 0.0;
    if constexpr (PASS >= 1) {
        if (p.state_in) c1 = p.state_in[grp * 2], c2 = p.state_in[grp * 2 + 1];
        const double *sc = p.scratch + grp * p.cut.segments * 3;
        for (int k = 0; k < seg; ++k) {
            const int lg = k < p.cut.r ? 1 : 0;
            c1 = st_max(sc[k * 3], p.R.seg[lg] * c1 + sc[k * 3 + 1]);
            if constexpr (PASS == 2) c2 = p.A.seg[lg] * c2 + sc[k * 3 + 2];
        }
    }
    double sM = 0.0, sB = 0.0, sS = 0.0;                             // the segment's summaries (passes A and B)

    for (int64_t it = 0; it < sg.ntile; ++it) {
        const int64_t n0 = (sg.tile0 + it) * ST_TILE;
        scan_stage_peak(slot, p.io, T_, grp, n0);
        __syncthreads();
        double v[ST_E];
#pragma unroll
        for (int e = 0; e < ST_E; ++e) v[e] = cp_curve(slot[st_own(t, e)], p);

        // ---- release stage: lane summary, wave scan, wave totals
        double M = v[0], B = p.R.b * v[0];
#pragma unroll
        for (int e = 1; e < ST_E; ++e) {
            const double bv = p.R.b * v[e];
            M = st_max(v[e], p.R.a * M + bv);
            B = p.R.a * B + bv;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double Mp = __shfl_up(M, 1 << j), Bp = __shfl_up(B, 1 << j);
            if (lane >= (1 << j)) {
                M = st_max(M, p.R.pw[j] * Mp + B);
                B = p.R.pw[j] * Bp + B;
            }
        }
        const double Mex = __shfl_up(M, 1), Bex = __shfl_up(B, 1);   // the lanes in front of this one (lane 0: unused)
        if (lane == 63) wM[wave] = M, wB[wave] = B;
        __syncthreads();

        if constexpr (PASS == 0) {
            double Mt = wM[0], Bt = wB[0];
#pragma unroll
            for (int k = 1; k < ST_WAVES; ++k) {
                Mt = st_max(wM[k], p.R.pw[6] * Mt + wB[k]);
                Bt = p.R.pw[6] * Bt + wB[k];
            }
            if (it == 0) {
                sM = Mt, sB = Bt;
            } else {
                sM = st_max(Mt, p.R.pw[8] * sM + Bt);
                sB = p.R.pw[8] * sB + Bt;
            }
            __syncthreads();                                         // wM / wB and the slots are free again
            continue;
        } else {
            // second run from the true start
            double y1 = c1;
#pragma unroll
            for (int k = 0; k < ST_WAVES - 1; ++k)
                if (k < wave) y1 = st_max(wM[k], p.R.pw[6] * y1 + wB[k]);
            if (lane > 0) y1 = st_max(Mex, laneR * y1 + Bex);
#pragma unroll
            for (int e = 0; e < ST_E; ++e) {
                y1 = st_max(v[e], p.R.a * y1 + p.R.b * v[e]);
                v[e] = y1;
            }
#pragma unroll
            for (int k = 0; k < ST_WAVES; ++k) c1 = st_max(wM[k], p.R.pw[6] * c1 + wB[k]);

            // ---- attack stage on y1 (now in v)
            double S = p.A.b * v[0];
#pragma unroll
            for (int e = 1; e < ST_E; ++e) S = p.A.a * S + p.A.b * v[e];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double Sp = __shfl_up(S, 1 << j);
                if (lane >= (1 << j)) S = p.A.pw[j] * Sp + S;
            }
            const double Sex = __shfl_up(S, 1);
            if (lane == 63) wS[wave] = S;
            __syncthreads();

            if constexpr (PASS == 1) {
                double St = wS[0];
#pragma unroll
                for (int k = 1; k < ST_WAVES; ++k) St = p.A.pw[6] * St + wS[k];
                sS = it == 0 ? St : p.A.pw[8] * sS + St;
                __syncthreads();
                continue;
            } else {
                double yl = c2;
#pragma unroll
                for (int k = 0; k < ST_WAVES - 1; ++k)
                    if (k < wave) yl = p.A.pw[6] * yl + wS[k];
                if (lane > 0) yl = laneA * yl + Sex;
                const int64_t nl = n0 + (int64_t)t * ST_E;           // the lane's first sample
#pragma unroll
                for (int e = 0; e < ST_E; ++e) {
                    yl = p.A.a * yl + p.A.b * v[e];
                    slot[st_own(t, e)] = exp10((p.makeup - yl) * 0.05);
                    if (p.state_out && nl + e == T_ - 1) {
                        p.state_out[grp * 2] = v[e];
                        p.state_out[grp * 2 + 1] = yl;
                    }
                }
#pragma unroll
                for (int k = 0; k < ST_WAVES; ++k) c2 = p.A.pw[6] * c2 + wS[k];
                __syncthreads();
                scan_apply_gain(slot, p.io, T_, grp, n0);
                __syncthreads();                                     // the slots are free again
            }
        }
    }
    if constexpr (PASS == 0) {
        if (t == 0) {
            double *sc = p.scratch + (grp * p.cut.segments + seg) * 3;
            sc[0] = sM, sc[1] = sB;
        }
    }
    if constexpr (PASS == 1) {
        if (t == 0) p.scratch[(grp * p.cut.segments + seg) * 3 + 2] = sS;
    }
}

// sizes alone (host-only)
static ScanPlan compressor_plan(const char *what, int64_t groups, int64_t channels, int64_t T, int64_t segments)
{
    return scan_plan(what, groups, channels, T, segments, CP_AUTO_BLOCKS, CP_AUTO_GROUPS, 3 * (int64_t)sizeof(double));
}

void compressor_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t segments, int64_t *tile, int64_t *tiles,
                          int64_t *segments_out, int64_t *seg_tiles, int64_t *scratch_bytes)
{
    scan_plan_info(compressor_plan("compressor_plan_info", groups, channels, T, segments), tile, tiles, segments_out, seg_tiles,
                   scratch_bytes);
}

static void stage_constants(CpStage &st, double a, const ScanPlan &pl)
{
    st.a = a;
    st.b = 1.0 - a;
    for (int j = 0; j < CP_NPW; ++j) st.pw[j] = (double)powl((long double)a, (long double)((int64_t)ST_E << j));
    for (int k = 0; k < 2; ++k) st.seg[k] = (double)powl((long double)a, (long double)((pl.q + k) * ST_TILE));
}

void compressor_forward(const void *x, void *y, void *gain, int dtype, int64_t groups, int64_t channels, int64_t T, double th,
                        double s, double w, double alpha_a, double alpha_r, double makeup_db, const double *state_in,
                        double *state_out, int64_t segments, void *scratch, hipStream_t stream)
{
    const char *what = "compressor_forward";
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: bad dtype %d", what, dtype);
    const ScanPlan pl = compressor_plan(what, groups, channels, T, segments);
    TFX_CHECK(std::isfinite(th), "%s: the threshold must be a finite level in dB, got %g", what, th);
    TFX_CHECK(s >= 0.0 && s <= 1.0, "%s: the slope 1 - 1/ratio must be in [0, 1], got %g", what, s);
    TFX_CHECK(std::isfinite(w) && w >= 0.0, "%s: the knee must be a finite width >= 0 in dB, got %g", what, w);
    TFX_CHECK(alpha_a >= 0.0 && alpha_a <= 1.0, "%s: alpha_a must be in [0, 1], got %g", what, alpha_a);
    TFX_CHECK(alpha_r >= 0.0 && alpha_r <= 1.0, "%s: alpha_r must be in [0, 1], got %g", what, alpha_r);
    TFX_CHECK(std::isfinite(makeup_db), "%s: the make-up gain must be finite, got %g", what, makeup_db);
    scan_check_buffers(what, pl, T, x, y, scratch, state_in, state_out);
    if (groups * T == 0) return scan_empty_chunk(groups, 2, state_in, state_out, stream);
    auto run = [&](auto tag) {
        using E = decltype(tag);
        CompArgs<E> p{};
        p.io = {(const E *)x, (E *)y, (E *)gain, (int)channels};
        p.state_in = state_in; p.state_out = state_out; p.scratch = (double *)scratch;
        p.cut = scan_cut(pl, T);
        p.th = th; p.s = s; p.w = w; p.makeup = makeup_db;
        p.lin_lo = pow(10.0, (th - 0.5 * w) / 20.0) * (1.0 - 0x1p-40);
        stage_constants(p.R, alpha_r, pl);
        stage_constants(p.A, alpha_a, pl);
        const ScanPass<CompArgs<E>> ladder[] = {{compressor_kernel<E, 0>, "compressor_pass_a"},
                                                {compressor_kernel<E, 1>, "compressor_pass_b"},
                                                {compressor_kernel<E, 2>, "compressor_pass_c"}};
        scan_launch(ladder, p, pl, stream);
    };
    if (dtype == TFX_F32) run(float{});
    else run(double{});
}

}  // namespace tfx
