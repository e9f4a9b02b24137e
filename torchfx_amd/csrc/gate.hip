// gate.hip -- noise gate with hysteresis, hold and range (tfx_gate_forward; include/torchfx_hip.h has the full contract).  For a
// group of `channels` rows that share one gain curve, detector in float64:
//   p[n]    = max_ch |x[ch,n]|
//   open[n] : p >= P_open opens and clears the hold counter c; an open gate with p >= P_close clears c; an open gate below
//             P_close counts c += 1 and closes (c = 0) once c > H; a closed gate below P_open stays closed
//   g[n]    = aA g[n-1] + bA where open[n], else aR g[n-1] + bR       (bA = 1 - aA, bR = (1 - aR) r)
//   y[ch,n] = dtype(g[n] x[ch,n])
// Both recursions are scans over a monoid.
//   Decision.  A run of samples acts on the incoming (open, c) through four values: S0, the end state when entered closed; S1,
//   the end state when entered open with c = 0; L, the length of the run's leading stretch of samples below P_close; and
//   allquiet.  A closed state goes to S0; an open one to S0 if c + L > H (it closes inside the leading stretch, and a closed
//   gate does not see the rest of that stretch), else to (open, c + L) if the run is all quiet, else to S1 (the first sample
//   at or above P_close clears c, as it does for the gate entered with c = 0).  Two runs X then Y compose as S0 = Y(S0_X),
//   S1 = Y(S1_X), L = L_X + L_Y if X is all quiet else L_X, allquiet = both.  L saturates at H + 1: beyond that it only ever
//   answers "c + L > H".  A state is one 32-bit word (GT_CLOSED, or c of the open gate); a summary is two 64-bit words.
//   Gain.  g -> A g + S with a per-sample coefficient; the product A is carried explicitly.
// Non-finite input: a NaN or Inf p[n] puts NaN in the gain scan's addend, and a NaN g is the mark of a poisoned group from then
// on (0 * NaN is NaN, so aA = aR = 0 carries it too): the open track is forced to 0 wherever g is NaN and the end state is NaN.
// The decision scan itself runs over such samples as the comparisons fall; its result there is masked.
//
// Work unit: scan_tile.h's, a unit being a group; both carries stay in registers.  The decision's lane summary runs the lane's 8
// samples from both start states; the gain's scan follows it, its coefficients fixed by the decision just made.
// segments == 1: one launch (pass C).  Otherwise three:
//   A  every segment but the last: its decision summary                                               reads x
//   B  every segment but the last: composes the decision summaries in front of it (a short loop), runs the decision for real
//      and stores its gain summary (A, S)                                                             reads x
//   C  every segment: composes both carries, runs both scans, applies the gain                        reads x, writes y
// The three passes compute p and the decision with the same code, so the carries B and C compose are the same words.
#include "common.h"
#include "scan_tile.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <algorithm>
#include <cmath>

namespace tfx {

constexpr int64_t GT_AUTO_BLOCKS = 1024, GT_AUTO_GROUPS = 512;
constexpr int GT_SCRATCH_WORDS = 4;                       // per (group, segment): the decision summary's two words, then A and S
constexpr unsigned GT_CLOSED = 0x80000000u;               // the closed state; an open one is its hold counter c <= H < 2^31

typedef unsigned long long gt_u64;

// what a run of samples does to the decision state
struct GtSum {
    gt_u64 s;                   // S0 (low word) and S1 (high word)
    gt_u64 l;                   // min(L, H + 1) (low word) and allquiet (bit 32)
};

template <typename T> struct GateArgs {
    ScanGainIO<T> io;
    unsigned char *open;        // [groups, T_] or null
    const double *state_in;     // [groups, 3] (g, open, c) or null (closed, g = r)
    double *state_out;          // [groups, 3] or null
    gt_u64 *scratch;            // [groups, segments, GT_SCRATCH_WORDS]; unused for segments == 1
    ScanCut cut;
    unsigned H;
    double p_open, p_close, range;
    double aA, bA, aR, bR;
};

// a run of samples of the gain stage: g -> A g + S
struct GtGain {
    double A, S;
};

// one sample of the automaton: cls 2 = at or above P_open, 1 = at or above P_close, 0 = below both (NaN falls here)
__device__ __forceinline__ unsigned gt_step(unsigned s, unsigned cls, unsigned H)
{
    if (cls == 2u) return 0u;
    if (s == GT_CLOSED) return s;
    if (cls == 1u) return 0u;
    return s + 1u > H ? GT_CLOSED : s + 1u;               // H + 1 <= 2^31 = GT_CLOSED: no wrap
}

// the run `m` applied to the state `s`
__device__ __forceinline__ unsigned gt_apply(const GtSum &m, unsigned s, unsigned H)
{
    const unsigned s0 = (unsigned)m.s, s1 = (unsigned)(m.s >> 32), L = (unsigned)m.l;
    if (s == GT_CLOSED) return s0;
    const gt_u64 c = (gt_u64)s + L;
    if (c > H) return s0;
    return (m.l >> 32) ? (unsigned)c : s1;
}

// the run `x`, then the run `y`
__device__ __forceinline__ GtSum gt_compose(const GtSum &x, const GtSum &y, unsigned H)
{
    GtSum o;
    o.s = (gt_u64)gt_apply(y, (unsigned)x.s, H) | ((gt_u64)gt_apply(y, (unsigned)(x.s >> 32), H) << 32);
    if (x.l >> 32) {
        const gt_u64 L = (gt_u64)(unsigned)x.l + (unsigned)y.l;
        o.l = (L > (gt_u64)H + 1 ? (gt_u64)H + 1 : L) | (y.l & (1ull << 32));
    } else {
        o.l = x.l;
    }
    return o;
}

// (g, open, c) -> the state word; anything that is not a clean state is closed (the gain's NaN marks the poisoned group)
__device__ __forceinline__ unsigned gt_state_word(double op, double c, unsigned H)
{
    if (!(op > 0.0)) return GT_CLOSED;
    if (!(c >= 0.0)) return 0u;
    return c > (double)H ? H : (unsigned)c;
}

// PASS 0 = A, 1 = B, 2 = C
template <typename T, int PASS>
__global__ void __launch_bounds__(ST_THREADS, 4) gate_kernel(const GateArgs<T> p)      // 4 waves per SIMD: pass C fits 128 VGPRs
{
    __shared__ double slot[ST_PAD];
    __shared__ gt_u64 wDs[ST_WAVES], wDl[ST_WAVES];
    __shared__ double wA[ST_WAVES], wS[ST_WAVES];
    __shared__ gt_u64 obits[ST_THREADS];                               // the open track, a lane's 8 samples as 8 bytes
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const ScanSeg sg = scan_segment(p.cut, PASS == 2 ? p.cut.segments : p.cut.segments - 1);
    const int64_t grp = sg.unit, T_ = p.cut.T_;
    const int seg = sg.seg;
    const unsigned H = p.H;

    // the carries at the segment's start: the state, then the summaries of the segments in front
    unsigned cs = GT_CLOSED;
    double cg = p.range;
    if constexpr (PASS >= 1) {
        if (p.state_in) {
            const double g0 = p.state_in[grp * 3], o0 = p.state_in[grp * 3 + 1], c0 = p.state_in[grp * 3 + 2];
            cs = gt_state_word(o0, c0, H);
            cg = (fabs(g0) <= 1.7976931348623157e308 && o0 == o0 && c0 == c0) ? g0 : (double)NAN;
        }
        const gt_u64 *sc = p.scratch + grp * p.cut.segments * GT_SCRATCH_WORDS;
        for (int k = 0; k < seg; ++k) {
            GtSum m;
            m.s = sc[k * GT_SCRATCH_WORDS], m.l = sc[k * GT_SCRATCH_WORDS + 1];
            cs = gt_apply(m, cs, H);
            if constexpr (PASS == 2)
                cg = __longlong_as_double((long long)sc[k * GT_SCRATCH_WORDS + 2]) * cg +
                     __longlong_as_double((long long)sc[k * GT_SCRATCH_WORDS + 3]);
        }
    }
    GtSum sD{};                                                        // the segment's summaries (passes A and B)
    double sA = 1.0, sS = 0.0;

    for (int64_t it = 0; it < sg.ntile; ++it) {
        const int64_t n0 = (sg.tile0 + it) * ST_TILE;
        scan_stage_peak(slot, p.io, T_, grp, n0);
        __syncthreads();
        // the lane's 8 samples: class (2 bits each) and non-finite mark (1 bit each)
        unsigned cls = 0u, bad = 0u;
#pragma unroll
        for (int e = 0; e < ST_E; ++e) {
            const double pv = slot[st_own(t, e)];
            cls |= (pv >= p.p_open ? 2u : pv >= p.p_close ? 1u : 0u) << (2 * e);
            bad |= (pv <= 1.7976931348623157e308 ? 0u : 1u) << e;
        }

        // ---- decision: lane summary, wave scan, wave totals
        GtSum D;
        {
            unsigned s0 = GT_CLOSED, s1 = 0u, L = 0u;
            bool quiet = true;
#pragma unroll
            for (int e = 0; e < ST_E; ++e) {
                const unsigned c = (cls >> (2 * e)) & 3u;
                s0 = gt_step(s0, c, H);
                s1 = gt_step(s1, c, H);
                quiet = quiet && c == 0u;
                L += quiet ? 1u : 0u;
            }
            if (L > H) L = H + 1u;
            D.s = (gt_u64)s0 | ((gt_u64)s1 << 32);
            D.l = (gt_u64)L | ((gt_u64)(quiet ? 1u : 0u) << 32);
        }
        scan_wave(D, lane, [&](const GtSum &Dp, const GtSum &Dc, int) { return gt_compose(Dp, Dc, H); });
        const GtSum Dex = scan_shfl_up(D, 1);                          // the lanes in front of this one (lane 0: unused)
        if (lane == 63) wDs[wave] = D.s, wDl[wave] = D.l;
        __syncthreads();

        if constexpr (PASS == 0) {
            GtSum Dt;
            Dt.s = wDs[0], Dt.l = wDl[0];
#pragma unroll
            for (int k = 1; k < ST_WAVES; ++k) {
                GtSum w;
                w.s = wDs[k], w.l = wDl[k];
                Dt = gt_compose(Dt, w, H);
            }
            sD = it == 0 ? Dt : gt_compose(sD, Dt, H);
            __syncthreads();                                         // wD and the slots are free again
            continue;
        } else {
            // second run from the true start
            unsigned s = cs;
#pragma unroll
            for (int k = 0; k < ST_WAVES; ++k) {
                GtSum w;
                w.s = wDs[k], w.l = wDl[k];
                if (k < wave) s = gt_apply(w, s, H);
                cs = gt_apply(w, cs, H);
            }
            if (lane > 0) s = gt_apply(Dex, s, H);
            const int64_t nl = n0 + (int64_t)t * ST_E;               // the lane's first sample
            unsigned op = 0u, slast = GT_CLOSED;                     // open[e] at bit e; the state after sample T - 1
#pragma unroll
            for (int e = 0; e < ST_E; ++e) {
                s = gt_step(s, (cls >> (2 * e)) & 3u, H);
                op |= (s != GT_CLOSED ? 1u : 0u) << e;
                if (nl + e == T_ - 1) slast = s;
            }

            // ---- gain: the coefficients follow the decision; a non-finite sample's addend is NaN
            GtGain G{1.0, 0.0};
#pragma unroll
            for (int e = 0; e < ST_E; ++e) {
                const bool o = (op >> e) & 1u;
                const double a = o ? p.aA : p.aR;
                const double b = ((bad >> e) & 1u) ? (double)NAN : (o ? p.bA : p.bR);
                G.S = a * G.S + b;
                G.A = a * G.A;
            }
            scan_wave(G, lane, [](const GtGain &f, GtGain c, int) {
                c.S = c.A * f.S + c.S;
                c.A = c.A * f.A;
                return c;
            });
            const GtGain Gex = scan_shfl_up(G, 1);
            if (lane == 63) wA[wave] = G.A, wS[wave] = G.S;
            __syncthreads();

            if constexpr (PASS == 1) {
                double At = wA[0], St = wS[0];
#pragma unroll
                for (int k = 1; k < ST_WAVES; ++k) {
                    St = wA[k] * St + wS[k];
                    At = wA[k] * At;
                }
                if (it == 0) {
                    sA = At, sS = St;
                } else {
                    sS = At * sS + St;
                    sA = At * sA;
                }
                __syncthreads();
                continue;
            } else {
                double g = cg;
#pragma unroll
                for (int k = 0; k < ST_WAVES; ++k) {
                    if (k < wave) g = wA[k] * g + wS[k];
                    cg = wA[k] * cg + wS[k];
                }
                if (lane > 0) g = Gex.A * g + Gex.S;
                gt_u64 ob = 0ull;
#pragma unroll
                for (int e = 0; e < ST_E; ++e) {
                    const bool o = (op >> e) & 1u;
                    g = (o ? p.aA : p.aR) * g + (((bad >> e) & 1u) ? (double)NAN : (o ? p.bA : p.bR));
                    slot[st_own(t, e)] = g;
                    ob |= (gt_u64)((o && g == g) ? 1u : 0u) << (8 * e);
                    if (p.state_out && nl + e == T_ - 1) {
                        const bool ok = g == g, so = slast != GT_CLOSED;
                        p.state_out[grp * 3] = g;
                        p.state_out[grp * 3 + 1] = ok ? (so ? 1.0 : 0.0) : (double)NAN;
                        p.state_out[grp * 3 + 2] = ok ? (so ? (double)slast : 0.0) : (double)NAN;
                    }
                }
                if (p.open) obits[t] = ob;
                __syncthreads();
                scan_apply_gain(slot, p.io, T_, grp, n0);
                if (p.open) {
                    const unsigned char *ob8 = (const unsigned char *)obits;
#pragma unroll
                    for (int k = 0; k < ST_E; ++k) {
                        const int a = k * ST_THREADS + t;
                        const int64_t n = n0 + a;
                        if (n < T_) p.open[grp * T_ + n] = ob8[a];
                    }
                }
                __syncthreads();                                     // the slots are free again
            }
        }
    }
    if constexpr (PASS == 0) {
        if (t == 0) {
            gt_u64 *sc = p.scratch + (grp * p.cut.segments + seg) * GT_SCRATCH_WORDS;
            sc[0] = sD.s, sc[1] = sD.l;
        }
    }
    if constexpr (PASS == 1) {
        if (t == 0) {
            gt_u64 *sc = p.scratch + (grp * p.cut.segments + seg) * GT_SCRATCH_WORDS;
            sc[2] = (gt_u64)__double_as_longlong(sA), sc[3] = (gt_u64)__double_as_longlong(sS);
        }
    }
}

// T == 0 without a state: the start state (r, closed, 0) of every group
__global__ void gate_start_state_kernel(double *state_out, int64_t groups, double range)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < groups) state_out[i * 3] = range, state_out[i * 3 + 1] = 0.0, state_out[i * 3 + 2] = 0.0;
}

// sizes alone (host-only)
static ScanPlan gate_plan(const char *what, int64_t groups, int64_t channels, int64_t T, int64_t segments)
{
    return scan_plan(what, groups, channels, T, segments, GT_AUTO_BLOCKS, GT_AUTO_GROUPS, GT_SCRATCH_WORDS * (int64_t)sizeof(gt_u64));
}

void gate_plan_info(int64_t groups, int64_t channels, int64_t T, int64_t segments, int64_t *tile, int64_t *tiles,
                    int64_t *segments_out, int64_t *seg_tiles, int64_t *scratch_bytes)
{
    scan_plan_info(gate_plan("gate_plan_info", groups, channels, T, segments), tile, tiles, segments_out, seg_tiles, scratch_bytes);
}

void gate_forward(const void *x, void *y, void *gain, unsigned char *open, int dtype, int64_t groups, int64_t channels, int64_t T,
                  double p_open, double p_close, double range, int64_t hold, double alpha_a, double alpha_r, const double *state_in,
                  double *state_out, int64_t segments, void *scratch, hipStream_t stream)
{
    const char *what = "gate_forward";
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "%s: bad dtype %d", what, dtype);
    const ScanPlan pl = gate_plan(what, groups, channels, T, segments);
    TFX_CHECK(std::isfinite(p_open) && p_open > 0.0, "%s: the opening level must be a finite linear level > 0, got %g", what, p_open);
    TFX_CHECK(p_close >= 0.0 && p_close <= p_open, "%s: the closing level must be in [0, the opening level %g], got %g", what, p_open,
              p_close);
    TFX_CHECK(range >= 0.0 && range <= 1.0, "%s: the range must be a linear gain in [0, 1], got %g", what, range);
    TFX_CHECK(hold >= 0 && hold < (1ll << 31), "%s: the hold must be in [0, 2^31) samples, got %lld", what, (long long)hold);
    TFX_CHECK(alpha_a >= 0.0 && alpha_a <= 1.0, "%s: alpha_a must be in [0, 1], got %g", what, alpha_a);
    TFX_CHECK(alpha_r >= 0.0 && alpha_r <= 1.0, "%s: alpha_r must be in [0, 1], got %g", what, alpha_r);
    scan_check_buffers(what, pl, T, x, y, scratch, state_in, state_out);
    if (groups * T == 0)
        return scan_empty_chunk(groups, 3, state_in, state_out, stream, [&](size_t) {
            hipLaunchKernelGGL(gate_start_state_kernel, dim3((unsigned)ceil_div(groups, 256)), dim3(256), 0, stream, state_out, groups,
                               range);
            TFX_HIP(hipGetLastError());
        });
    auto run = [&](auto tag) {
        using E = decltype(tag);
        GateArgs<E> p{};
        p.io = {(const E *)x, (E *)y, (E *)gain, (int)channels};
        p.open = open; p.state_in = state_in; p.state_out = state_out; p.scratch = (gt_u64 *)scratch;
        p.cut = scan_cut(pl, T);
        p.H = (unsigned)hold; p.p_open = p_open; p.p_close = p_close; p.range = range;
        p.aA = alpha_a; p.bA = 1.0 - alpha_a;
        p.aR = alpha_r; p.bR = (1.0 - alpha_r) * range;
        const ScanPass<GateArgs<E>> ladder[] = {{gate_kernel<E, 0>, "gate_pass_a"}, {gate_kernel<E, 1>, "gate_pass_b"},
                                                {gate_kernel<E, 2>, "gate_pass_c"}};
        scan_launch(ladder, p, pl, stream);
    };
    if (dtype == TFX_F32) run(float{});
    else run(double{});
}

}  // namespace tfx
