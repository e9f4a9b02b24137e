// sos.hip -- fused K-section DF1 SOS cascade for gfx950 (MI355X).
//
// Replaces the reference's CPU loop (src/torchfx/_csrc/cpu/iir_cpu.cpp:64-159) and its
// CUDA path (cuda/biquad_forward.cu:49-92 + cuda/parallel_scan.cu: one forcing kernel and a
// 3-phase Blelloch scan PER SECTION, ~40 B/sample/section of HBM traffic) with ONE launch that
// reads x once and writes y once (8 B/sample for f32 I/O).  Not a port of either.
//
// Decomposition (DESIGN.md "IIR kernel"):
//   * a STREAM = (channel, time segment) is owned by one 64-lane wavefront; a workgroup is four
//     independent streams (no __syncthreads anywhere).  Segments other than the first start
//     `warm` samples early from zero state (the halo is part of the stream's tile grid: every
//     stream walks the same number of full tiles); `warm` is chosen on the host so that the cascade's
//     zero-input transition matrix A^warm is below 2^-60, i.e. the halo reproduces the true
//     state to float64 round-off.  Filters whose memory is too long get nseg = 1 (exact,
//     sequential tiles per channel).
//   * a TILE = 64 lanes x LC consecutive samples.  Coalesced 16-byte global loads are
//     transposed through a padded (bank-conflict-free) LDS stage so that lane j owns samples
//     [j*LC, (j+1)*LC) in registers.  The next tile's loads are issued before computing.
//   * per section, entirely in registers (7 flop per sample):  (1a) the feed-forward part
//     f[n] = b0 v[n] + b1 v[n-1] + b2 v[n-2] overwrites v in place, walking n downwards;  (1b) the
//     recursion runs over f from zero state (lane 0: from the carried true state) only to get the
//     lane's 2-vector end state;  (2) the end states are combined across lanes by a DPP-only scan
//     (row_shr Kogge-Stone inside 16-lane rows, row_bcast:15 / row_bcast:31 across rows, wave_shr:1)
//     with constant 2x2 matrices C^(LC*m) computed on the host in long double;  (3) the recursion
//     runs once more over f from the true start state and leaves the section output in place.
//     Section s+1 then consumes the exact output of s.
//   * arithmetic type TC is float64 by default -- the reference computes in float64
//     (_ops.py:149) -- or float32 (TFX_PREC_F32).
#include "common.h"
#include "epilogue.h"
#include "plan_cache.h"
#include "sos.h"
#include "sos_route.h"
#include "../../include/torchfx_hip.h"

#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <type_traits>
#include <vector>

namespace tfx {

// ------------------------------------------------------------------------------------------
// Table layout per section (TC elements):
//   [0..4]  b0 b1 b2 -a1 -a2      [5..7] pad
//   [8 + 4k + {0..3}]             Cmp^(LC * 2^k) row-major, k < 6   (Cmp = [[-a1,-a2],[1,0]])
//   [32 + 4p + {0..3}]            Cmp^(LC * (p+1)), p < 32: per-lane matrices of the scan's two
//                                 cross-row steps (p = lane % 16 and p = lane % 32)
//   [160..163]                    1/Gin, 1/Gout, Gin, Gout: the scale of the section's input / output in the unit-b0 form (else 1)
// Unit-b0 form (UNIT kernels, float64, K >= 2): every b0 is pulled out of its section, section s computes
//   y' = v' + (b1/b0) v'[n-1] + (b2/b0) v'[n-2] - a1 y'[n-1] - a2 y'[n-2]
// on v' = v / Gin, y' = y / Gout (Gin = product of the b0 before it, Gout = Gin b0): step (1a) loses its multiply, the product
// of all b0 comes back in ONE multiply where the output is rounded and stored -- K - 1 vector instructions per sample less.
// The carried states enter and leave through the same factors.  Same recursion, same poles; the numerator arithmetic
// differs from the reference's by float64 round-off (parity at 2e-11 of the output scale like the plain form).
// Cascades with a zero / tiny / huge b0 keep the plain form (unit_form_ok).
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr int tab_stride(int) { return 32 + 128 + 8; }

struct SosParams {
    const void *x;
    void *y;
    void *taps;          // optional [K,C,T] of TOut
    const void *tab;     // device table, TC
    const double *sx_in, *sy_in;
    double *sx_out, *sy_out;
    int64_t C, T;        // C = output rows (= bands x input rows in filter-bank mode)
    int64_t x_pitch;     // elements between consecutive input rows (= T for a contiguous [C_in, T] signal)
    int64_t C_in;        // input rows: output row c reads input row c % C_in with the tables of band c / C_in
    int64_t seg_len;     // distance between the starts of consecutive streams of a row = seg_tiles * TILE - warm
    int64_t warm;        // halo of the streams g > 0; multiple of 32 samples (streams start on 128-byte lines)
    int K, nseg, nsteps;
    int nt;              // nontemporal global loads / stores of the signal (aligned 16-byte path)
    int nsum;            // > 0: sum mode -- every stream runs `nsum` bands over its input row and accumulates them
    // epilogue on the stored samples (epilogue.h): y *= gain, clip, partial of max|y| / sum y^2 per stream
    double ep_gain;
    int ep_scale, ep_clamp, ep_stat;
    double *ep_partial;  // [C * nseg], one per stream (row-major over (row, segment)), pre-zeroed
    int *nf_flag;        // [C * nseg]: stream ended with a non-finite carried state (nseg > 1 only; every stream writes its slot)
    int fair;            // > 0: waves that share a SIMD alternate their issue priority every 2^fair clocks
    int fair_nw;         // waves per SIMD of this launch (the priority levels that rotate): 2 ... 4
    // zero-phase passes (FF kernels, sos_filtfilt_forward): T above is the length of the edge-extended row, ff_T + 2 * ff_pad
    int ff;              // 1 = forward pass over the virtual extension of x, 2 = reverse-time pass over the intermediate
    int ff_padtype;      // TFX_PAD_ODD / EVEN / CONSTANT (NONE arrives as ff_pad = 0)
    int64_t ff_T;        // samples per row of the signal itself
    int64_t ff_pad;      // samples the row is extended by at each end
    const double *ff_gain;   // device [K + 1]: G_(s-1) at [s], the DC gain of the sections in front of section s (G_(-1) = 1)
    // measuring pass (MEAS kernels, sos_block_energy_forward): y is the float64 [C, ms_nblk] array of block energies; block i
    // holds the samples [e_i, e_(i+1)), e_i = (i * ms_num) / ms_den, and segment g owns the blocks [g * ms_bps, (g + 1) * ms_bps)
    int64_t ms_num, ms_den, ms_nblk, ms_bps;
    // hand-off route (sos_route.h): D = 2 K + 2 doubles per stream, [x1 x2 | y1 y2 of section 0 | ... of section K - 1] in the
    // true scale (cascade_step's vector; a section's input history is the output history of the one before it)
    const double *ho_state;  // [C * nseg, D] or null: the streams g > 0 start from their slot instead of zeros
    double *ho_end;          // ENDS kernels: [C * nseg, D], stream (row, g) leaves its end state in its slot
};

// Sample i of the row x[0 .. T) extended by `pad` samples at each end (scipy.signal's odd_ext / even_ext / const_ext), i counted
// from the start of the extension; pad < T.
template <typename TIn>
__device__ __forceinline__ double ff_ext_sample(const TIn *__restrict__ x, int64_t T, int64_t pad, int padtype, int64_t i)
{
    const int64_t j = i - pad;
    if (j >= 0 && j < T) return (double)x[j];
    const int64_t edge = j < 0 ? 0 : T - 1;
    const int64_t mirror = j < 0 ? -j : 2 * (T - 1) - j;
    if (padtype == TFX_PAD_CONSTANT) return (double)x[edge];
    if (padtype == TFX_PAD_EVEN) return (double)x[mirror];
    return 2.0 * (double)x[edge] - (double)x[mirror];
}

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// DPP shift of a value across lanes; lanes with no source lane receive 0 (bound_ctrl).
template <int CTRL> __device__ __forceinline__ float dpp_shift(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL> __device__ __forceinline__ double dpp_shift(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// DPP row broadcast (row_bcast:15 = 0x142, row_bcast:31 = 0x143) into the rows of ROWMASK; all
// other lanes receive 0.
template <int CTRL, int ROWMASK> __device__ __forceinline__ float dpp_bcast(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWMASK, 0xF, false));
}
template <int CTRL, int ROWMASK> __device__ __forceinline__ double dpp_bcast(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWMASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWMASK, 0xF, false);
    return __hiloint2double(hi, lo);
}
// streaming (nontemporal) 16-byte global accesses: the signal is read once and written once, and a plain streaming copy
// gains 3-8 % from them on this part (tools/ubench/stream_copy2.hip: linear sweep 6.29 -> 6.80 TB/s, persistent streams
// 5.06 -> 5.20 / 5.86 -> 6.12)
typedef unsigned uintx4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld16(const uint4 *p, bool nt)
{
    if (nt) { const uintx4_t v = __builtin_nontemporal_load((const uintx4_t *)p); return make_uint4(v.x, v.y, v.z, v.w); }
    return *p;
}
__device__ __forceinline__ void st16(uint4 *p, uint4 v, bool nt)
{
    if (nt) __builtin_nontemporal_store((uintx4_t){v.x, v.y, v.z, v.w}, (uintx4_t *)p);
    else *p = v;
}
template <typename T> struct U16 {               // 16 bytes of T
    static constexpr int N = 16 / sizeof(T);
    union { uint4 u; T e[N]; };
};

// LC   samples per lane per tile          VEC  16-byte global accesses (aligned rows)
// TAPS also store every section's output  PF   keep the next tile's loads in flight in registers
// MINW waves per SIMD the register allocator must leave room for
// SUMB sum mode (`+` of IIR branches, __base.py:1019-1026): the stream applies p.nsum independent
//      cascades ("bands") to its input tile, which stays in the LDS stage, and accumulates their
//      outputs -- rounded to TOut per band and added in branch order, exactly like the reference's
//      zeros_like + in-place adds -- so N branches cost 8 B/sample instead of N x 8 + (N + 1) x 4
// EPI  epilogue on the stored samples (epilogue.h); a separate instantiation so that the plain kernel keeps
//      its register budget (the statistic accumulator and the extra selects cost ~30 VGPRs = one wave per SIMD)
// FF   zero-phase pass (SosParams::ff): 1 reads the virtual edge extension of x, 2 walks the float64 intermediate from its
//      end and stores the signal's own samples at their reversed places; both start from the cascade's steady state for
//      the row's first sample (scipy.signal.sosfilt_zi * x[0]).  Scalar (!VEC) path only; FF = 0 compiles to the code
//      it was before
// FFR  refine the scan's start states once (see the scan below): the zero-phase passes of a float64 result, and the forward
//      cascade and the measuring pass for the cascades whose plan asks for it (plan_refine)
// MEAS measuring pass (SosParams::ms_*): the cascade's output is not stored; the stream keeps the sum of its squares over each
//      block of samples it owns.  Segments start on block edges (their halo in front), so every block has one writer.  Scalar
//      (!VEC) path only, TOut = TIn (the stage holds the input alone); MEAS = false compiles to the code it was before
// ENDS end-state pass of the hand-off route (SosParams::ho_*): the streams g < nseg - 1 walk their whole-tile segments with the
//      same arithmetic and store nothing but the cascade's state after their last sample.  Scalar (!VEC) path only, TOut = TIn,
//      float64 arithmetic; ENDS = false compiles to the code it was before
// One compiled instance of the kernel = one value of this struct and a type triple; written with designated initialisers.
struct SosKernel { int LC = 32; bool VEC = false, TAPS = false, PF = false; int MINW = 2;
                   bool SUMB = false, EPI = false, UNIT = false; int FF = 0; bool FFR = false, MEAS = false, ENDS = false;
                   bool operator==(const SosKernel &) const = default; };

// The stream body: one wavefront walks stream `sid` = (row, segment) with `stage` as its private LDS (transposition
// stage + carry).  Shared by the cascade kernel below and by the fused per-chunk kernel (chunk_iir_fir_kernel), whose
// output pointer is an LDS buffer.
template <typename TIn, typename TOut, typename TC, SosKernel G>
__device__ __forceinline__ void sos_stream_body(const SosParams &p, const int64_t sid, char *const stage, const int lane)
{
    constexpr int LC = G.LC, FF = G.FF;
    constexpr bool VEC = G.VEC, TAPS = G.TAPS, PF = G.PF, SUMB = G.SUMB, EPI = G.EPI, UNIT = G.UNIT, FFR = G.FFR, MEAS = G.MEAS, ENDS = G.ENDS;
    static_assert(!(TAPS && SUMB), "section taps are not available in sum mode");
    static_assert(!(UNIT && (TAPS || SUMB)), "the unit-b0 form serves the plain cascade only");
    static_assert(FF == 0 || !(VEC || TAPS || PF || SUMB || EPI || UNIT), "the zero-phase passes run the plain scalar path");
    static_assert(!MEAS || !(VEC || TAPS || PF || SUMB || EPI || UNIT || FF != 0), "the measuring pass runs the plain scalar path");
    static_assert(!MEAS || (std::is_same<TC, double>::value && LC <= 64), "block energies: float64 sums, at most one block edge per lane");
    static_assert(!ENDS || !(VEC || TAPS || PF || SUMB || EPI || UNIT || FF != 0 || MEAS), "the end-state pass runs the plain scalar path");
    static_assert(!ENDS || std::is_same<TC, double>::value, "end states are float64");
    // what the LDS stage holds on the way in: the odd extension 2 x[0] - x[i] of a float32 row is not a float32 value
    typedef typename std::conditional<FF == 1, TC, TIn>::type TSt;
    constexpr int IOB = sizeof(TIn) > sizeof(TOut) ? sizeof(TIn) : sizeof(TOut);
    constexpr int CHUNK_B = LC * IOB + 16;   // per-lane chunk, padded: conflict-free b128 access
    constexpr int STAGE_B = 64 * CHUNK_B;
    constexpr int TILE = 64 * LC;
    constexpr int TS = tab_stride(LC);
    constexpr int SB = 4;               // scheduling-barrier period (samples)
    constexpr int EI = 16 / sizeof(TSt), NUI = LC / EI;   // elems per 16 B, units per lane (in)
    constexpr int EO = 16 / sizeof(TOut), NUO = LC / EO;  // (out)

    const int K = p.K;
    if (sid >= p.C * p.nseg) return;                       // wave-uniform
    unsigned wave_slot = 0;
    if (p.fair) {
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        wave_slot = hw & 15u;                              // wave slot within the SIMD
    }
    const int64_t c = sid / p.nseg;
    const int g = (int)(sid - c * p.nseg);
    const int nbl = SUMB ? p.nsum : 1;                     // bands handled inside this stream
    TC *carry = (TC *)(stage + STAGE_B);                   // [nbl][K][4] = vin1 vin2 y1 y2
    TC *cap = carry + nbl * K * 4;                         // [2][LC] final-state capture scratch

    const int64_t T = p.T;
    const int64_t band = SUMB ? 0 : c / p.C_in;
    const int64_t st_rows = SUMB ? p.C_in * nbl : p.C;     // rows of the [K, rows, 2] state tensors
    const TIn *__restrict__ xrow = (const TIn *)p.x + (c - band * p.C_in) * p.x_pitch;
    TOut *__restrict__ yrow = (TOut *)p.y + c * (FF == 2 ? p.ff_T : T);
    // Coefficient tables live in the CONSTANT address space: wave-uniform indices then lower to
    // s_load (scalar cache, SGPR operands) instead of per-lane vector loads.
    typedef const TC __attribute__((address_space(4))) *ctab_t;
    const ctab_t tab = (ctab_t)(uintptr_t)p.tab + band * (int64_t)K * TS;

    // stream g reads [g * seg_len, (g + 1) * seg_len + warm): exactly seg_tiles full tiles for every stream, the
    // first `warm` samples of a stream g > 0 being its halo (plan_segments)
    int64_t start = (int64_t)g * p.seg_len;
    int64_t out_begin = g ? start + p.warm : 0;
    int64_t ms_kb = 0, ms_ke = 0;                          // measuring pass: this stream owns the blocks [ms_kb, ms_ke)
    if constexpr (MEAS) {
        ms_kb = (int64_t)g * p.ms_bps;
        ms_ke = ms_kb + p.ms_bps < p.ms_nblk ? ms_kb + p.ms_bps : p.ms_nblk;
        out_begin = ms_kb * p.ms_num / p.ms_den;           // e_kb >= warm for g > 0 (block_energy_plan)
        start = g ? out_begin - p.warm : 0;
    }
    if constexpr (ENDS) { if (g == p.nseg - 1) return; }      // the last segment hands nothing on
    if (out_begin >= T) {
        if (p.nf_flag && lane == 0) p.nf_flag[sid] = 0;
        return;
    }
    int64_t out_end = start + p.seg_len + p.warm;
    if (out_end > T || g == p.nseg - 1) out_end = T;
    if constexpr (MEAS) out_end = ms_ke * p.ms_num / p.ms_den;      // e_ke <= T: samples from e_nblk on belong to no block
    const bool last_seg = !MEAS && !ENDS && (out_end == T);     // (the measuring and end-state passes return no state)

    // ---- initial carry: the caller's state for the stream that starts at n = 0, zeros for a
    //      warm-up start.  Layout of state tensors: [K, C, 2] (iir_cpu.cpp:125-130).
    for (int i = lane; i < nbl * K * 4; i += 64) {
        const int b = i / (K * 4), rem = i - b * K * 4;
        const int s = rem >> 2, f = rem & 3;
        TC v = (TC)0;
        if (FF == 0 && !MEAS && g > 0 && p.ho_state) {
            // hand-off: the exact state at the segment's first sample (the scan's), into the section's scale like the caller's
            v = (TC)p.ho_state[sid * (2 * K + 2) + (f < 2 ? 2 * s + f : 2 + 2 * s + (f & 1))];
            if (UNIT) v *= ((const TC *)p.tab)[(band * K + s) * TS + (f < 2 ? 160 : 161)];
        } else if (start == 0) {
            if constexpr (FF != 0) {
                // steady state of the cascade for a constant input v0 = the first sample of the pass: section s has seen
                // v0 G_(s-1) for ever and answered v0 G_s
                const double v0 = FF == 1 ? ff_ext_sample(xrow, p.ff_T, p.ff_pad, p.ff_padtype, 0) : (double)xrow[T - 1];
                v = (TC)(v0 * p.ff_gain[s + (f >> 1)]);
            } else {
                const double *src = (f < 2) ? p.sx_in : p.sy_in;
                if (src) v = (TC)src[((int64_t)s * st_rows + (SUMB ? b * p.C_in + c : c)) * 2 + (f & 1)];
                if (UNIT) v *= ((const TC *)p.tab)[(band * K + s) * TS + (f < 2 ? 160 : 161)];      // into the section's scale
            }
        }
        carry[i] = v;
    }
    wave_sync();

    // ---- global -> registers (coalesced).  Per-lane pointer + immediate offsets; the common
    //      full-tile case is branch-free, a partial tile (signal tail) is predicated.
    uint4 rawv[VEC ? NUI : 1];
    TSt raws[VEC ? 1 : LC];
    auto load_tile = [&](int64_t ts) {
        const int64_t left = T - ts;
        if constexpr (VEC) {
            const uint4 *__restrict__ xl = (const uint4 *)(xrow + ts) + lane;
            if (left >= TILE) {
#pragma unroll
                for (int i = 0; i < NUI; ++i) rawv[i] = ld16(xl + i * 64, p.nt);
            } else {
                const int nv = (int)(left / EI);   // valid 16-byte units
#pragma unroll
                for (int i = 0; i < NUI; ++i)
                    rawv[i] = (i * 64 + lane < nv) ? xl[i * 64] : make_uint4(0, 0, 0, 0);
            }
        } else if constexpr (FF == 1) {
            // element e of the tile is sample ts + e of the extended row; tiles inside the signal load it as it lies
            const int64_t j0 = ts - p.ff_pad;
            if (j0 >= 0 && j0 + TILE <= p.ff_T) {
                const TIn *__restrict__ xl = xrow + j0 + lane;
#pragma unroll
                for (int i = 0; i < LC; ++i) raws[i] = (TSt)xl[i * 64];
            } else {
#pragma unroll
                for (int i = 0; i < LC; ++i) {
                    const int64_t n = ts + i * 64 + lane;
                    raws[i] = n < T ? (TSt)ff_ext_sample(xrow, p.ff_T, p.ff_pad, p.ff_padtype, n) : (TSt)0;
                }
            }
        } else if constexpr (FF == 2) {
            // element e of the tile is sample T - 1 - (ts + e) of the intermediate: the row is walked from its end
            const TIn *__restrict__ xl = xrow + (T - 1 - ts - lane);
            if (left >= TILE) {
#pragma unroll
                for (int i = 0; i < LC; ++i) raws[i] = xl[-(i * 64)];
            } else {
                const int nv = (int)left;
#pragma unroll
                for (int i = 0; i < LC; ++i) raws[i] = (i * 64 + lane < nv) ? xl[-(i * 64)] : (TIn)0;
            }
        } else {
            const TIn *__restrict__ xl = xrow + ts + lane;
            if (left >= TILE) {
#pragma unroll
                for (int i = 0; i < LC; ++i) raws[i] = xl[i * 64];
            } else {
                const int nv = (int)left;
#pragma unroll
                for (int i = 0; i < LC; ++i) raws[i] = (i * 64 + lane < nv) ? xl[i * 64] : (TIn)0;
            }
        }
    };
    // LDS stage addresses: unit q = i*64 + lane lives at chunk q/NU, slot q%NU; 64 % NU == 0
    char *const st_in_v = stage + (lane / NUI) * CHUNK_B + (lane % NUI) * 16;
    char *const st_out_v = stage + (lane / NUO) * CHUNK_B + (lane % NUO) * 16;
    char *const st_in_s = stage + (lane / LC) * CHUNK_B + (lane % LC) * (int)sizeof(TSt);     // LC | 64
    char *const st_out_s = stage + (lane / LC) * CHUNK_B + (lane % LC) * (int)sizeof(TOut);
    char *const st_own = stage + lane * CHUNK_B;

    if constexpr (PF) load_tile(start);
    double ep_acc = 0.0;                   // this lane's share of the stream's statistic (0 is neutral for both modes)
    double ms_carry = 0.0;                 // measuring pass: the sum so far of the block that is open at the tile's first sample
    int ms_bad = 0;                        // ... and whether this lane has written a non-finite block

    for (int64_t ts = start; ts < out_end; ts += TILE) {
        TC d[LC];
        if constexpr (!PF) load_tile(ts);
        // ---- stage: coalesced order -> LDS -> blocked (lane j owns [j*LC,(j+1)*LC))
        if constexpr (VEC) {
#pragma unroll
            for (int i = 0; i < NUI; ++i) *(uint4 *)(st_in_v + i * (64 / NUI) * CHUNK_B) = rawv[i];
        } else {
#pragma unroll
            for (int i = 0; i < LC; ++i) *(TSt *)(st_in_s + i * (64 / LC) * CHUNK_B) = raws[i];
        }
        wave_sync();
        auto read_own = [&]() {
#pragma unroll
            for (int i = 0; i < NUI; ++i) {
                U16<TSt> v;
                v.u = *(const uint4 *)(st_own + i * 16);
#pragma unroll
                for (int e = 0; e < EI; ++e) d[i * EI + e] = (TC)v.e[e];
            }
        };
        if constexpr (!SUMB) {
            read_own();
            wave_sync();
        }

        // ---- prefetch the next tile while this one is computed
        if constexpr (PF) { if (ts + TILE < out_end) load_tile(ts + TILE); }

        const bool final_tile = last_seg && (ts + TILE >= T);
        const int r = (int)(T - ts);   // valid samples in the final tile (1..TILE)

        TOut acc[SUMB ? LC : 1];
        for (int bnd = 0; bnd < nbl; ++bnd) {
        if constexpr (SUMB) read_own();          // the input tile is still in this lane's LDS chunk
        const int64_t tband = SUMB ? bnd : band;
        TC *const carry_s = carry + bnd * K * 4;
        for (int s = 0; s < K; ++s) {
            if (p.fair) {
                // Fair share of the SIMD.  The waves of two workgroups share each SIMD for the whole launch, and the issue arbiter
                // serves them by priority, then AGE: the older wave runs almost unimpeded, the younger one on the leftover slots
                // (per-stream time stamps, round 4: the first wave of every SIMD finished after 251 us, the second after 347 us,
                // the last 96 us with one wave per SIMD and half the issue rate).  Both waves read the same clock, and each takes
                // the high priority in alternate epochs according to its slot, so they advance together and finish together.
                // (more than two waves per SIMD: the priority levels 0 ... nw - 1 rotate over the slots, s_setprio has four)
                const unsigned e = (unsigned)(__builtin_readcyclecounter() >> p.fair);
                const unsigned lvl = (e + wave_slot) % (unsigned)p.fair_nw;
                if (lvl == 0) __builtin_amdgcn_s_setprio(0);
                else if (lvl == 1) __builtin_amdgcn_s_setprio(1);
                else if (lvl == 2) __builtin_amdgcn_s_setprio(2);
                else __builtin_amdgcn_s_setprio(3);
            }
            const ctab_t tb = tab + (SUMB ? (int64_t)bnd * K * TS : 0) + s * TS;
            const TC b0 = tb[0], b1 = tb[1], b2 = tb[2], na1 = tb[3], na2 = tb[4];
            TC mqa[4], mqb[4];                  // P^(lane%16 + 1), P^(lane%32 + 1)
            {
                const TC *mp = (const TC *)p.tab + (tband * K + s) * TS + 32;
#pragma unroll
                for (int i = 0; i < 4; ++i) mqa[i] = mp[4 * (lane & 15) + i];
#pragma unroll
                for (int i = 0; i < 4; ++i) mqb[i] = mp[4 * (lane & 31) + i];
            }
            const TC cv1 = carry_s[s * 4 + 0], cv2 = carry_s[s * 4 + 1];
            const TC cy1 = carry_s[s * 4 + 2], cy2 = carry_s[s * 4 + 3];

            // final tile only: read the section's sequence at tile-local index idx (-1/-2 = the
            // carried history) through a 2 x LC scratch in LDS
            auto capture2 = [&](int i1, int i2, TC h1, TC h2, TC &o1, TC &o2) {
                const int w1 = i1 >= 0 ? i1 / LC : -1, w2 = i2 >= 0 ? i2 / LC : -1;
                if (lane == w1) {
#pragma unroll
                    for (int n = 0; n < LC; ++n) cap[n] = d[n];
                }
                if (lane == w2) {
#pragma unroll
                    for (int n = 0; n < LC; ++n) cap[LC + n] = d[n];
                }
                wave_sync();
                o1 = i1 >= 0 ? cap[i1 - w1 * LC] : (i1 == -1 ? h1 : h2);
                o2 = i2 >= 0 ? cap[LC + i2 - w2 * LC] : (i2 == -1 ? h1 : h2);
                wave_sync();
            };

            // input history of this lane's chunk: previous lane's last two inputs
            TC pv1 = dpp_shift<0x138>(d[LC - 1]);     // wave_shr:1
            TC pv2 = dpp_shift<0x138>(d[LC - 2]);
            if (lane == 0) { pv1 = cv1; pv2 = cv2; }
            TC sx1 = (TC)0, sx2 = (TC)0;
            if (final_tile) capture2(r - 1, r - 2, cv1, cv2, sx1, sx2);
            if (lane == 63) { carry_s[s * 4 + 0] = d[LC - 1]; carry_s[s * 4 + 1] = d[LC - 2]; }

            // (1a) feed-forward part f[n] = b0 v[n] + b1 v[n-1] + b2 v[n-2], written IN PLACE by
            //      walking n downwards (f[n] never needs v[m] for m > n): 3 flop/sample, no second
            //      register set and no copies
#pragma unroll
            for (int n = LC - 1; n >= 0; --n) {
                const TC x1 = n >= 1 ? d[n - 1] : pv1;
                const TC x2 = n >= 2 ? d[n - 2] : (n == 1 ? pv1 : pv2);
                d[n] = UNIT ? fma(b2, x2, fma(b1, x1, d[n])) : fma(b2, x2, fma(b1, x1, b0 * d[n]));
            }
            // (1b) the recursion over f from zero start state (lane 0: from the carried true
            //      state), only to get this chunk's END STATE -- 2 flop/sample, nothing stored
            TC u1 = (lane == 0) ? cy1 : (TC)0;
            TC u2 = (lane == 0) ? cy2 : (TC)0;
#pragma unroll
            for (int n = 0; n < LC; ++n) {
                const TC u = fma(na1, u1, fma(na2, u2, d[n]));
                u2 = u1;   u1 = u;
            }

            // (2) inclusive scan of chunk end-states over lanes:  S_j = sum_i P^(j-i) z_i, then the
            //     exclusive shift (h1,h2) = S_{j-1}.  All cross-lane traffic is DPP -- a few cycles of
            //     latency per step instead of an LDS round trip per ds_bpermute:
            //       a. intra-row Kogge-Stone with P^1, P^2, P^4, P^8 (row_shr; lanes without a
            //          source add 0)
            //       b. row_bcast:15 into rows 1,3 and row_bcast:31 into rows 2,3, each applied with
            //          the lane's own matrix P^(lane%16+1) / P^(lane%32+1) from the table
            //       c. wave_shr:1 turns the inclusive scan into every lane's start state
            const ctab_t pm = tb + 8;
            TC s0 = u1, s1 = u2;
#define TFX_KS_STEP(K_, CTRL_)                                                            \
            {                                                                             \
                const TC t0 = dpp_shift<CTRL_>(s0), t1 = dpp_shift<CTRL_>(s1);            \
                s0 += fma(pm[4 * K_ + 0], t0, pm[4 * K_ + 1] * t1);                       \
                s1 += fma(pm[4 * K_ + 2], t0, pm[4 * K_ + 3] * t1);                       \
            }
            // b. rows 1 and 3 take in the aggregate of the row before them (row_bcast:15),
            //    then rows 2 and 3 the inclusive value of lane 31 (row_bcast:31): two DPP
            //    steps with per-lane matrices instead of readlanes + a select tree
#define TFX_LANE_SCAN()                                                                   \
            TFX_KS_STEP(0, 0x111)   /* row_shr:1 */                                       \
            TFX_KS_STEP(1, 0x112)   /* row_shr:2 */                                       \
            TFX_KS_STEP(2, 0x114)   /* row_shr:4 */                                       \
            TFX_KS_STEP(3, 0x118)   /* row_shr:8 */                                       \
            {                                                                             \
                const TC a0 = dpp_bcast<0x142, 0xA>(s0), a1 = dpp_bcast<0x142, 0xA>(s1);  \
                s0 += fma(mqa[0], a0, mqa[1] * a1);                                       \
                s1 += fma(mqa[2], a0, mqa[3] * a1);                                       \
                const TC c0 = dpp_bcast<0x143, 0xC>(s0), c1 = dpp_bcast<0x143, 0xC>(s1);  \
                s0 += fma(mqb[0], c0, mqb[1] * c1);                                       \
                s1 += fma(mqb[2], c0, mqb[3] * c1);                                       \
            }
            TFX_LANE_SCAN()
            TC h1 = dpp_shift<0x138>(s0), h2 = dpp_shift<0x138>(s1);     // wave_shr:1: state at chunk start
            if (lane == 0) { h1 = cy1; h2 = cy2; }                       // lane 0: the carried true state
            if constexpr (FFR) {
                // One step of iterative refinement of the start states.  The scan adds zero-state chunk responses that are
                // hundreds of times larger than the state they cancel to when the poles lie next to z = 1 and the output
                // is rough (high-pass, notch): 2e-9 of the output scale on HiButterworth(20) at 48 kHz in float64, and 1e-7
                // at 192 kHz.  So: run the recursion once more from the start states just found; where chunk j - 1 ends and where chunk j was told to start differ
                // by a residual of that size, and the same scan over the residuals (e_j = r_j + P e_(j-1), e_0 = 0) gives
                // the correction with a relative error of its own.  What is left is the rounding of a sequential recursion.
                TC w1 = h1, w2 = h2;
#pragma unroll
                for (int n = 0; n < LC; ++n) {
                    const TC w = fma(na1, w1, fma(na2, w2, d[n]));
                    w2 = w1;   w1 = w;
                }
                s0 = dpp_shift<0x138>(w1) - h1;
                s1 = dpp_shift<0x138>(w2) - h2;
                if (lane == 0) { s0 = (TC)0; s1 = (TC)0; }
                TFX_LANE_SCAN()
                h1 += s0;   h2 += s1;
            }
#undef TFX_LANE_SCAN
#undef TFX_KS_STEP

            // (3) the recursion proper from the TRUE start state over the stored f[n]: 2 flop/sample,
            //     writes the section output in place.  (Cheaper than correcting the zero-state output
            //     with its homogeneous response, 3 flop/sample, and no table.)
#pragma unroll
            for (int n = 0; n < LC; ++n) {
                const TC t = fma(na2, h2, d[n]);
                const TC yv = fma(na1, h1, t);
                d[n] = yv;
                h2 = h1; h1 = yv;
                if ((n & (SB - 1)) == SB - 1) __builtin_amdgcn_sched_barrier(0);
            }

            if (lane == 63) { carry_s[s * 4 + 2] = d[LC - 1]; carry_s[s * 4 + 3] = d[LC - 2]; }

            if (final_tile) {
                TC sy1, sy2;
                capture2(r - 1, r - 2, cy1, cy2, sy1, sy2);
                if (lane == 0) {
                    const int64_t o = ((int64_t)s * st_rows + (SUMB ? bnd * p.C_in + c : c)) * 2;
                    const TC g_in = UNIT ? tb[162] : (TC)1, g_out = UNIT ? tb[163] : (TC)1;      // back to the true scale
                    if (p.sx_out) { p.sx_out[o] = (double)(sx1 * g_in); p.sx_out[o + 1] = (double)(sx2 * g_in); }
                    if (p.sy_out) { p.sy_out[o] = (double)(sy1 * g_out); p.sy_out[o + 1] = (double)(sy2 * g_out); }
                }
            }
            if constexpr (TAPS) {   // debug / section-by-section parity only
                TOut *trow = (TOut *)p.taps + ((int64_t)s * p.C + c) * T + ts;
                const int64_t lo64 = out_begin - ts, hi64 = out_end - ts;
                const int lo = lo64 > 0 ? (int)lo64 : 0, hi = hi64 < TILE ? (int)hi64 : TILE;
#pragma unroll
                for (int n = 0; n < LC; ++n) {
                    const int rel = lane * LC + n;
                    if (rel >= lo && rel < hi) trow[rel] = (TOut)d[n];
                }
            }
            wave_sync();   // carry[] written by lane 63 is read by all lanes next tile/section
        }
        if constexpr (SUMB) {
#pragma unroll
            for (int n = 0; n < LC; ++n) acc[n] = (bnd == 0 ? (TOut)0 : acc[n]) + (TOut)d[n];
        }
        }   // bands
        if constexpr (SUMB) {
#pragma unroll
            for (int n = 0; n < LC; ++n) d[n] = (TC)acc[n];
        }


        // ---- measuring pass: nothing is stored but the energy of the blocks that end in this tile
        if constexpr (MEAS) {
            if (ts + TILE > out_begin) {
                // Sample n lies in block floor(((n + 1) den - 1) / num).  For this lane's chunk [a, a + LC): qm = the block of
                // sample a - 1 (-1 in front of the row), rm the remainder of that division; sample a + k is in block
                // qm + floor((rm + (k + 1) den) / num), so the chunk's only edge (blocks are at least 64 >= LC samples long) is
                // at k = ke = floor((num - rm - 1) / den), if that is below LC.  The two quotients come from a float64
                // estimate corrected by one step of integer arithmetic (T den < 2^61: the estimate is off by at most one).
                const int64_t w = (ts + (int64_t)lane * LC) * p.ms_den - 1;
                int64_t qm = (int64_t)floor((double)w / (double)p.ms_num);
                int64_t rm = w - qm * p.ms_num;
                if (rm < 0) { qm -= 1; rm += p.ms_num; }
                else if (rm >= p.ms_num) { qm += 1; rm -= p.ms_num; }
                const int64_t gap = p.ms_num - rm - 1;
                int ke = LC;
                if (gap < (int64_t)LC * p.ms_den) {
                    ke = (int)((double)gap / (double)p.ms_den);
                    if ((int64_t)ke * p.ms_den > gap) --ke;
                    else if ((int64_t)(ke + 1) * p.ms_den <= gap) ++ke;
                }
                const bool edge = ke < LC;
                // this lane's samples in sequence: sa belongs to the block open at its first sample, sb to the one that starts at ke
                TC sa = (TC)0, sb = (TC)0;
#pragma unroll
                for (int n = 0; n < LC; ++n) sa = fma(d[n], d[n], sa);
                if (edge) {                        // rare: one lane in num / den / LC
                    sa = (TC)0;
#pragma unroll
                    for (int n = 0; n < LC; ++n) {
                        const TC t = d[n] * d[n];
                        if (n < ke) sa += t; else sb += t;
                    }
                }
                // segmented inclusive scan over the lanes (Kogge-Stone, fixed tree): v = the open block's sum at the END of the
                // lane's chunk, counted from the last edge at or before it -- or, with no edge yet (f = 0), from the tile's start
                TC v = edge ? sb : sa;
                int f = edge ? 1 : 0;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const TC vp = __shfl_up(v, off);
                    const int fp = __shfl_up(f, off);
                    if (lane >= off) {
                        if (!f) v = vp + v;
                        f |= fp;
                    }
                }
                if (!f) v = ms_carry + v;
                TC before = __shfl_up(v, 1);       // the open block's sum in front of this lane's chunk
                if (lane == 0) before = ms_carry;
                if (edge && qm >= ms_kb && qm < ms_ke) {       // block qm ends inside this chunk: its one writer
                    const TC tot = before + sa;
                    ((double *)p.y)[c * p.ms_nblk + qm] = tot;
                    ms_bad |= !(fabs(tot) <= 1.79e308);
                }
                ms_carry = __shfl(v, 63);
            }
        }

        // ---- store (skipped entirely while still inside the warm-up halo)
        if (!MEAS && !ENDS && ts + TILE > out_begin) {
            const int64_t lo64 = out_begin - ts, hi64 = out_end - ts;
            const bool full = (lo64 <= 0) && (hi64 >= TILE);
            if constexpr (UNIT) {                       // the product of all b0, once, on the way out
                const TC gt = tab[(K - 1) * TS + 163];
#pragma unroll
                for (int n = 0; n < LC; ++n) d[n] *= gt;
            }
            if constexpr (!EPI) {
#pragma unroll
                for (int i = 0; i < NUO; ++i) {
                    U16<TOut> v;
#pragma unroll
                    for (int e = 0; e < EO; ++e) v.e[e] = (TOut)d[i * EO + e];
                    *(uint4 *)(st_own + i * 16) = v.u;
                }
            } else {
                // Gain / clamp on the rounded output value, in the output dtype (what a standalone Gain pass
                // would compute from the stored sample), and this lane's share of the statistic over the
                // samples that are really stored
                const TOut g_ = (TOut)p.ep_gain;
                const int lo_s = lo64 > 0 ? (int)lo64 : 0, hi_s = hi64 < TILE ? (int)hi64 : TILE;
#pragma unroll
                for (int i = 0; i < NUO; ++i) {
                    U16<TOut> v;
#pragma unroll
                    for (int e = 0; e < EO; ++e) {
                        TOut o = (TOut)d[i * EO + e];
                        if (p.ep_scale) o = o * g_;
                        if (p.ep_clamp) o = clamp_unit(o);
                        v.e[e] = o;
                        if (p.ep_stat >= 0) {
                            const int rel = lane * LC + i * EO + e;
                            if (full || (rel >= lo_s && rel < hi_s)) ep_acc = red_comb_rt(p.ep_stat, ep_acc, red_elem_rt(p.ep_stat, (double)o));
                        }
                    }
                    *(uint4 *)(st_own + i * 16) = v.u;
                }
            }
            wave_sync();
            if constexpr (VEC) {
                uint4 *__restrict__ yl = (uint4 *)(yrow + ts) + lane;
                if (full) {
#pragma unroll
                    for (int i = 0; i < NUO; ++i)
                        st16(yl + i * 64, *(const uint4 *)(st_out_v + i * (64 / NUO) * CHUNK_B), p.nt);
                } else {
                    const int lo = lo64 > 0 ? (int)(lo64 / EO) : 0;
                    const int hi = hi64 < TILE ? (int)(hi64 / EO) : TILE / EO;
#pragma unroll
                    for (int i = 0; i < NUO; ++i) {
                        const int q = i * 64 + lane;
                        const uint4 v = *(const uint4 *)(st_out_v + i * (64 / NUO) * CHUNK_B);
                        if (q >= lo && q < hi) yl[i * 64] = v;
                    }
                }
            } else if constexpr (FF == 2) {
                // sample n of this pass is sample T - 1 - ff_pad - n of the result; the extension's samples are not stored
                const int64_t lo_s = p.ff_pad - ts, hi_s = p.ff_pad + p.ff_T - ts;
                const int64_t lo2 = lo64 > lo_s ? lo64 : lo_s, hi2 = hi64 < hi_s ? hi64 : hi_s;
                const int lo = lo2 > 0 ? (int)(lo2 < TILE ? lo2 : TILE) : 0;
                const int hi = hi2 < TILE ? (int)(hi2 > 0 ? hi2 : 0) : TILE;
                TOut *__restrict__ yl = yrow + (T - 1 - p.ff_pad - ts - lane);
#pragma unroll
                for (int i = 0; i < LC; ++i) {
                    const int e = i * 64 + lane;
                    const TOut v = *(const TOut *)(st_out_s + i * (64 / LC) * CHUNK_B);
                    if (e >= lo && e < hi) yl[-(i * 64)] = v;
                }
            } else {
                TOut *__restrict__ yl = yrow + ts + lane;
                const int lo = lo64 > 0 ? (int)lo64 : 0;
                const int hi = hi64 < TILE ? (int)hi64 : TILE;
#pragma unroll
                for (int i = 0; i < LC; ++i) {
                    const int e = i * 64 + lane;
                    const TOut v = *(const TOut *)(st_out_s + i * (64 / LC) * CHUNK_B);
                    if (e >= lo && e < hi) yl[i * 64] = v;
                }
            }
            wave_sync();
        }
    }
    if constexpr (MEAS) {
        // the stream's last block ends with its last tile when e_ke is a multiple of the tile away from `start`: no lane saw that edge
        if (lane == 0 && (out_end - start) % TILE == 0) {
            ((double *)p.y)[c * p.ms_nblk + ms_ke - 1] = ms_carry;
            ms_bad |= !(fabs(ms_carry) <= 1.79e308);
        }
        // a non-finite block = a non-finite output sample of the cascade among the stream's own: the recursion keeps it to the end
        // of the row, which the segments after this one cannot know (sos_block_energy_fix_kernel).  Not the carried state: the last
        // tile runs on into the next segment's samples.
        const int anyb = __any(ms_bad) ? 1 : 0;
        if (p.nf_flag && lane == 0) p.nf_flag[sid] = anyb;
        return;
    }
    if constexpr (ENDS) {
        // the carry after a whole number of full tiles is the cascade's state after the segment's last sample
        for (int i = lane; i < 2 * K + 2; i += 64) p.ho_end[sid * (2 * K + 2) + i] = (double)carry[i < 2 ? i : 4 * ((i - 2) >> 1) + 2 + (i & 1)];
        return;
    }
    if (p.nf_flag) {
        // the carried state at the end of the stream (every band, every section: last two inputs and outputs);
        // non-finite there = non-finite from some sample of this stream to the end of the row (iir_cpu.cpp:132-147),
        // whatever an epilogue (clamp) made of the stored samples
        int badc = 0;
        for (int i = lane; i < nbl * K * 4; i += 64) badc |= !(fabs((double)carry[i]) <= 1.79e308);
        const int anyb = __any(badc) ? 1 : 0;
        if (lane == 0) p.nf_flag[sid] = anyb;
    }
    if (EPI && p.ep_stat >= 0) {           // one partial per stream, lanes combined in a fixed order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) ep_acc = red_comb_rt(p.ep_stat, ep_acc, __shfl_xor(ep_acc, off));
        if (lane == 0) p.ep_partial[sid] = ep_acc;
    }
}

// Bytes of LDS one stream (wavefront) needs, as sos_stream_body lays them out: the transposition stage (64 padded per-lane chunks
// of the wider of the two signal types) plus the carry (4 values per band and section, 2 x LC capture scratch), rounded to 16.
// Every launch sizes its dynamic LDS with this and the kernels place wave w at w times it: if the two disagreed, the carry of
// one wave would overwrite the stage of the next.
template <typename TIn, typename TOut, typename TC, int LC>
__host__ __device__ constexpr int sos_wave_lds_bytes(int nbl, int K)
{
    return 64 * (LC * (int)(sizeof(TIn) > sizeof(TOut) ? sizeof(TIn) : sizeof(TOut)) + 16) +
           ((((nbl * K * 4 + 2 * LC) * (int)sizeof(TC)) + 15) & ~15);
}

template <typename TIn, typename TOut, typename TC, SosKernel G>
__global__ void __launch_bounds__(256, G.MINW) sos_stream_kernel(const SosParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // provably wave-uniform -> SGPR addressing
    const int per_wave = sos_wave_lds_bytes<TIn, TOut, TC, G.LC>(G.SUMB ? p.nsum : 1, p.K);
    sos_stream_body<TIn, TOut, TC, G>(p, (int64_t)blockIdx.x * 4 + wave, smem + wave * per_wave, lane);
}

// Non-finite samples and time segmentation.  In the sequential recursion a NaN / Inf never leaves: once the
// state is non-finite every later output of the row is (iir_cpu.cpp:132-147).  A segment that starts from its
// warm-up halo does not see what happened before the halo, so every stream leaves a flag "my carried state ended
// non-finite" (every slot is written: no memset in front of the launch) and a second, tiny launch -- one workgroup
// per row; the kernel boundary is what makes the flags and samples of the eight XCDs' L2s visible -- finds the first
// flagged segment g0 of its row and overwrites the segments after it with NaN: their samples (and section taps),
// their statistic partials (so a following Normalize sees NaN like the standalone reduction would) and the returned
// states: "non-finite from the first bad sample to the end of the row", independent of how many segments the launch
// used and of what an epilogue (clamp) did to the stored samples.  Finite signals: C workgroups read nseg flags each
// and exit.  (Folding this into the main launch -- last workgroup to finish, device-scope fences -- was measured:
// the per-workgroup release fence writes back the XCD's L2 and the cfg-2 kernel went from 0.29-0.33 to 0.46-0.52 ms.)
//   y rows = C (output rows); state rows = st_rows with row c owning {b * C_in + c} for b < nbl in sum mode.
// The first segment of `row` whose stream left its flag set, p.nseg if none did.  Called by every thread of the workgroup.
__device__ __forceinline__ int first_flagged_segment(const SosParams &p, int64_t row)
{
    __shared__ int sh_first;
    if (threadIdx.x == 0) sh_first = p.nseg;
    __syncthreads();
    for (int q = threadIdx.x; q < p.nseg; q += blockDim.x)
        if (p.nf_flag[row * p.nseg + q]) atomicMin(&sh_first, q);
    __syncthreads();
    return sh_first;
}

template <typename TOut>
__global__ void __launch_bounds__(256) sos_nonfinite_fix_kernel(const SosParams p, int nbl, int64_t st_rows)
{
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int64_t T = p.T, row = blockIdx.x;
    const int g0 = first_flagged_segment(p, row);
    if (g0 >= p.nseg - 1) return;                                // clean row, or only the last segment is bad (it poisons itself)
    const int64_t begin = (int64_t)(g0 + 1) * p.seg_len + p.warm;   // first sample segment g0 + 1 stores
    if (begin >= T) return;
    TOut *y = (TOut *)p.y, *taps = (TOut *)p.taps;
    const TOut nanv = (TOut)__builtin_nan("");
    if (p.ff == 2) {      // reverse-time pass: sample n of the pass lies at T - 1 - ff_pad - n of the result row (sos_stream_body)
        const int64_t lo = begin > p.ff_pad ? begin : p.ff_pad, hi = p.ff_pad + p.ff_T;
        for (int64_t n = lo + tid; n < hi; n += nthr) y[row * p.ff_T + (T - 1 - p.ff_pad - n)] = nanv;
        return;
    }
    for (int64_t n = begin + tid; n < T; n += nthr) y[row * T + n] = nanv;
    if (taps)
        for (int sct = 0; sct < p.K; ++sct)
            for (int64_t n = begin + tid; n < T; n += nthr) taps[((int64_t)sct * p.C + row) * T + n] = nanv;
    if (p.ep_stat >= 0 && p.ep_partial)
        for (int g = g0 + 1 + tid; g < p.nseg; g += nthr) p.ep_partial[row * p.nseg + g] = __builtin_nan("");
    for (int i = tid; i < nbl * p.K * 2; i += nthr) {
        const int b = i / (p.K * 2), sct = (i >> 1) % p.K, f = i & 1;
        const int64_t o = ((int64_t)sct * st_rows + (nbl > 1 ? b * p.C_in + row : row)) * 2 + f;
        if (p.sx_out && sct > 0) p.sx_out[o] = __builtin_nan("");   // section 0's input history is the signal itself: already exact
        if (p.sy_out) p.sy_out[o] = __builtin_nan("");
    }
}

// The same repair for the measuring pass: the blocks of the segments after the row's first flagged one become NaN.
__global__ void __launch_bounds__(256) sos_block_energy_fix_kernel(const SosParams p)
{
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int64_t row = blockIdx.x;
    const int g0 = first_flagged_segment(p, row);
    if (g0 >= p.nseg - 1) return;
    double *s = (double *)p.y + row * p.ms_nblk;
    for (int64_t b = (int64_t)(g0 + 1) * p.ms_bps + tid; b < p.ms_nblk; b += nthr) s[b] = __builtin_nan("");
}

// Hand-off scan: the start states of a row's segments from the end states the ENDS pass left.  With v_j the input of segment
// boundary j = 1 ... nseg - 1 and P the transition over a segment, S_j = v_j + P S_(j-1) (S_0 = 0) -- a Kogge-Stone scan over the
// boundaries with the host's powers P^(2^k) (pw [nlev][D][D]), like the lane scan of the stream kernel one level up:
// ceil(log2(nseg - 1)) levels of independent D x D mat-vecs instead of nseg - 1 dependent ones.  One workgroup per row; the
// two buffers of a row (work [C][2][nseg][D]) and the barrier between levels stay inside the workgroup.
//   refine == 0:  v_j = ends[j - 1]                  state[j] = S_j        (ends[0] is the TRUE end of segment 0: it ran from the
//                                                                           caller's state, so the states are the true ones)
//   refine == 1:  v_j = ends[j - 1] - state[j]       state[j] += S_j       (ends = where the segments really end when started
//                 from `state`: the residual of the first scan, scanned the same way -- the FFR step of the lane scan)
// A non-finite end state makes every later state of its row non-finite in every component (each mat-vec adds all D products).
// state[0] is never read or written: segment 0 starts from the caller's state.
constexpr int SOS_HANDOFF_MAXD = 2 * SOS_HANDOFF_MAXK + 2;
__global__ void __launch_bounds__(256) sos_handoff_scan_kernel(const double *__restrict__ ends, double *__restrict__ state,
                                                               const double *__restrict__ pw, double *__restrict__ work,
                                                               int nseg, int D, int nlev, int refine)
{
    __shared__ double Pk[SOS_HANDOFF_MAXD * SOS_HANDOFF_MAXD];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int64_t row = blockIdx.x;
    const int n = (nseg - 1) * D;                              // element (j, i) of the boundaries 1 ... nseg - 1 at (j - 1) * D + i
    const double *e = ends + row * (int64_t)nseg * D;
    double *st = state + row * (int64_t)nseg * D + D;          // boundary 1 first
    double *a = work + row * 2 * (int64_t)nseg * D, *b = a + (int64_t)nseg * D;
    for (int q = tid; q < n; q += nthr) a[q] = refine ? e[q] - st[q] : e[q];
    for (int k = 0; k < nlev; ++k) {
        __syncthreads();
        for (int q = tid; q < D * D; q += nthr) Pk[q] = pw[(int64_t)k * D * D + q];
        __syncthreads();
        const int off = (1 << k) * D;
        for (int q = tid; q < n; q += nthr) {
            double v = a[q];
            if (q >= off) {
                const int i = q % D;
                const double *src = a + (q - i - off), *pr = Pk + i * D;
                double acc = 0.0;
                for (int m = 0; m < D; ++m) acc = fma(pr[m], src[m], acc);
                v += acc;
            }
            b[q] = v;
        }
        double *t = a; a = b; b = t;
    }
    __syncthreads();
    for (int q = tid; q < n; q += nthr) st[q] = refine ? st[q] + a[q] : a[q];
}

// ------------------------------------------------------------------------------------------
// Host side: tables and plan cache
// ------------------------------------------------------------------------------------------
typedef long double ld;

struct SosPlan {
    int K = 0;          // sections per band
    int NB = 1;         // bands (filter-bank mode: independent SOS sets sharing the input)
    int64_t warm = -1;            // samples; -1 = too long / not decaying
    double err_bound_f32 = -1.0;  // worst-case |err| of f32 arithmetic for |x| <= 1 (lazy)
    struct Table { std::unique_ptr<DeviceBuffer> buf; int nsteps = 6; };
    Table tab[2][3][2];           // [float32 / float64][LC = 16 / 32 / 64][plain / unit-b0 form (fill_tables)], lazy: table_for
    std::unique_ptr<DeviceBuffer> ff_gain;               // zero-phase passes: the K + 1 cumulative DC gains (filtfilt_gains), lazy
    int unit_ok = -1;                    // the cascade has a unit-b0 form (lazy)
    int blocked_known[3] = {0, 0, 0};    // per LC = 16 / 32 / 64: the measured error of the unrefined float64 kernel and of the
    double blocked[3][3] = {};           // sequential float64 recursion, shares of the output scale (plan_blocked_error, lazy)
    // hand-off route: P^(2^k), k < nlev, for P = A^L, the zero-input transition of the cascade over a segment of L samples --
    // computed in long double, rounded to float64, [nlev][D][D] row-major; ok = every entry finite and below SOS_HANDOFF_PMAX.
    // The device copy is made by the first launch that needs it (the route query needs none).  Lazy, per L (handoff_powers).
    struct Handoff {
        int nlev = 0; bool ok = false; std::vector<double> pw; std::unique_ptr<DeviceBuffer> buf;
        int nlev_for(int64_t nseg) const { int n = 0; while (((int64_t)1 << n) < nseg - 1) ++n; return n; }      // <= nlev (handoff_powers)
    };
    std::map<int64_t, std::shared_ptr<Handoff>> handoff;
    std::vector<double> sos;
};

static PlanCache<SosPlan, 1> g_plans(256);     // tail: the number of bands (a bank of NB x K sections is not a cascade of NB*K)
static std::mutex g_plan_mu;                   // the lazy members of a plan

// one zero-input step of the whole cascade on state w = [x1,x2, y1_1,y1_2, ..., yK_1,yK_2]
static void cascade_step(const std::vector<double> &sos, int K, std::vector<ld> &w)
{
    std::vector<ld> nw(w.size());
    ld v = 0.0L;                     // current input sample = 0
    ld p1 = w[0], p2 = w[1];         // input history of section 0
    nw[0] = 0.0L; nw[1] = w[0];
    for (int s = 0; s < K; ++s) {
        const double *co = &sos[s * 6];
        const ld y1 = w[2 + 2 * s], y2 = w[3 + 2 * s];
        const ld yn = (ld)co[0] * v + (ld)co[1] * p1 + (ld)co[2] * p2 - (ld)co[4] * y1 - (ld)co[5] * y2;
        nw[2 + 2 * s] = yn; nw[3 + 2 * s] = y1;
        p1 = y1; p2 = y2;            // next section's input history = this section's old outputs
        v = yn;
    }
    w.swap(nw);
}

static std::vector<ld> matmul(const std::vector<ld> &a, const std::vector<ld> &b, int D)
{
    std::vector<ld> c((size_t)D * D, 0.0L);
    for (int i = 0; i < D; ++i)
        for (int k = 0; k < D; ++k) {
            const ld aik = a[(size_t)i * D + k];
            if (aik == 0.0L) continue;
            for (int j = 0; j < D; ++j) c[(size_t)i * D + j] += aik * b[(size_t)k * D + j];
        }
    return c;
}
static ld maxabs(const std::vector<ld> &a)
{
    ld m = 0;
    for (ld v : a) { ld t = fabsl(v); if (!(t <= m)) m = t; }   // NaN-propagating
    return m;
}

// smallest W (with margin) such that max|A^W| < tol; -1 if not reached within 2^26 samples
static int64_t warmup_length(const std::vector<double> &sos, int K, int bits = 60)
{
    // O(K^3) long-double matrix squarings: beyond ~100 sections the analysis would cost seconds of host
    // time, so such cascades run as one sequential segment per row (exact, just less parallel)
    if (K > 96) return -1;
    const int D = 2 * K + 2;
    std::vector<ld> A((size_t)D * D, 0.0L);
    for (int j = 0; j < D; ++j) {
        std::vector<ld> w(D, 0.0L);
        w[j] = 1.0L;
        cascade_step(sos, K, w);
        for (int i = 0; i < D; ++i) A[(size_t)i * D + j] = w[i];
    }
    const ld tol = ldexpl(1.0L, -bits);
    std::vector<std::vector<ld>> pw;   // A^(2^i)
    pw.push_back(A);
    int m = 0;
    for (; m < 26; ++m) {
        ld nrm = maxabs(pw.back());
        if (!(nrm == nrm) || nrm > 1e300L) return -1;
        if (nrm < tol) break;
        pw.push_back(matmul(pw.back(), pw.back(), D));
    }
    if (m == 26) return -1;
    // greedy: largest n with max|A^n| >= tol
    std::vector<ld> cur;
    int64_t n = 0;
    for (int i = m - 1; i >= 0; --i) {
        std::vector<ld> cand = cur.empty() ? pw[i] : matmul(cur, pw[i], D);
        if (maxabs(cand) >= tol) { cur.swap(cand); n += (int64_t)1 << i; }
    }
    int64_t W = n + 1;
    W += W / 8 + 8;                    // margin: the norm is not strictly monotone
    return W;
}

// Hand-off route: the powers P^(2^k), k < nlev, of P = A^L (L samples of zero input), in long double, rounded to float64 at
// the end.  `ok` is false when an entry of any of them is not finite or reaches SOS_HANDOFF_PMAX: a cascade that is truly
// unstable keeps today's plan.  Poles ON the unit circle are fine (an integrator's P is bounded, a double one's grows like L).
static void handoff_power_table(const std::vector<double> &sos, int K, int64_t L, int nlev, std::vector<double> &out, bool &ok)
{
    const int D = 2 * K + 2;
    std::vector<ld> A((size_t)D * D, 0.0L);
    for (int j = 0; j < D; ++j) {
        std::vector<ld> w(D, 0.0L);
        w[j] = 1.0L;
        cascade_step(sos, K, w);
        for (int i = 0; i < D; ++i) A[(size_t)i * D + j] = w[i];
    }
    std::vector<ld> P;                       // A^L by squaring
    for (std::vector<ld> sq = A; L > 0; L >>= 1) {
        if (L & 1) P = P.empty() ? sq : matmul(P, sq, D);
        if (L > 1) sq = matmul(sq, sq, D);
    }
    out.assign((size_t)nlev * D * D, 0.0);
    ok = !P.empty();
    for (int k = 0; k < nlev && ok; ++k) {
        if (!(maxabs(P) < (ld)SOS_HANDOFF_PMAX)) { ok = false; break; }      // NaN-propagating
        for (size_t i = 0; i < (size_t)D * D; ++i) out[(size_t)k * D * D + i] = (double)P[i];
        if (k + 1 < nlev) P = matmul(P, P, D);
    }
}

// Whether the cascade can run in the unit-b0 form: every b0 non-zero, not dwarfed by its section's other numerator
// coefficients (b1 / b0 must stay a sane number) and every partial product of them far inside the float64 range.
static bool unit_form_ok(const std::vector<double> &sos, int K)
{
    if (K < 2) return false;
    ld g = 1.0L;
    for (int s = 0; s < K; ++s) {
        const ld b0 = sos[s * 6], b1 = sos[s * 6 + 1], b2 = sos[s * 6 + 2];
        g *= b0;
        if (!(fabsl(b0) > 0) || !(fabsl(b0) * 1e9L >= fmaxl(fabsl(b1), fabsl(b2))) || !(fabsl(g) > 1e-100L && fabsl(g) < 1e100L)) return false;
    }
    return true;
}

template <typename TC>
static void fill_tables(const std::vector<double> &sos, int K, int LC, std::vector<TC> &out, int &nsteps, bool unit = false)
{
    const int TS = tab_stride(LC);
    out.assign((size_t)K * TS, (TC)0);
    nsteps = 0;
    ld gin = 1.0L;
    for (int s = 0; s < K; ++s) {
        const double *co = &sos[s * 6];
        TC *tb = &out[(size_t)s * TS];
        if (unit) {
            tb[0] = (TC)1; tb[1] = (TC)((ld)co[1] / (ld)co[0]); tb[2] = (TC)((ld)co[2] / (ld)co[0]);
            const ld gout = gin * (ld)co[0];
            tb[160] = (TC)(1.0L / gin); tb[161] = (TC)(1.0L / gout); tb[162] = (TC)gin; tb[163] = (TC)gout;
            gin = gout;
        } else {
            tb[0] = (TC)co[0]; tb[1] = (TC)co[1]; tb[2] = (TC)co[2];
            tb[160] = tb[161] = tb[162] = tb[163] = (TC)1;
        }
        tb[3] = (TC)(-co[4]); tb[4] = (TC)(-co[5]);
        const ld a1 = co[4], a2 = co[5];
        // alpha: response to state (1,0); beta: to (0,1)
        ld al1 = 1, al2 = 0, be1 = 0, be2 = 1;
        ld P[4] = {1, 0, 0, 1};
        for (int n = 0; n < LC; ++n) {
            const ld al = -a1 * al1 - a2 * al2, be = -a1 * be1 - a2 * be2;
            al2 = al1; al1 = al; be2 = be1; be1 = be;
        }
        P[0] = al1; P[1] = be1; P[2] = al2; P[3] = be2;          // Cmp^LC
        {
            ld Q[4] = {P[0], P[1], P[2], P[3]};                   // Cmp^(LC (p+1))
            for (int pp = 0; pp < 32; ++pp) {
                for (int i = 0; i < 4; ++i) tb[32 + 4 * pp + i] = (TC)Q[i];
                const ld q0 = Q[0] * P[0] + Q[1] * P[2], q1 = Q[0] * P[1] + Q[1] * P[3];
                const ld q2 = Q[2] * P[0] + Q[3] * P[2], q3 = Q[2] * P[1] + Q[3] * P[3];
                Q[0] = q0; Q[1] = q1; Q[2] = q2; Q[3] = q3;
            }
        }
        int need = 0;
        for (int k = 0; k < 6; ++k) {
            for (int i = 0; i < 4; ++i) tb[8 + 4 * k + i] = (TC)P[i];
            ld m = 0;
            for (int i = 0; i < 4; ++i) m = fmaxl(m, fabsl(P[i]));
            if (!(m < 1e-22L)) need = k + 1;    // this step still contributes (or is NaN/inf)
            const ld q0 = P[0] * P[0] + P[1] * P[2], q1 = P[0] * P[1] + P[1] * P[3];
            const ld q2 = P[2] * P[0] + P[3] * P[2], q3 = P[2] * P[1] + P[3] * P[3];
            P[0] = q0; P[1] = q1; P[2] = q2; P[3] = q3;
        }
        if (need > nsteps) nsteps = need;
    }
}

// Estimate of the largest error of the float32 recursion against the float64 one for |x| <= 1 (what
// precision = "auto" decides on).  A rounding-noise model (noise variance x energy gain) is off by orders of
// magnitude exactly where it matters: with poles near z = 1 the chunked formulation adds zero-state
// responses that are 10^3..10^5 times larger than the output, which float64 shrugs off and float32 does not
// (HiButterworth-2 @ 20 Hz: error 3.0 on a signal of amplitude 1; profiles/r02_iir_f32_calibration.txt).  So
// the estimate is MEASURED: the kernel's float32 arithmetic -- same tile / lane structure (LC = 32), same
// operation order, same float32 tables and scan tree -- is replayed on the host for 2^16 pseudo-random
// samples per cascade (a millisecond, once per plan) against the sequential float64 recursion, and the
// largest difference is scaled by 2.5 (device runs of 4.6e7 samples per cascade measure 0.54 .. 1.02 of twice the
// replayed error over five orders of magnitude of it, tools/iir_f32_calibrate.py).
static double f32_error_bound(const std::vector<double> &sos, int K)
{
    constexpr int LC = 32, TILE = 64 * LC;
    const int TS = tab_stride(LC);
    const int64_t N = 1 << 16;
    std::vector<float> tab;
    int nsteps = 0;
    fill_tables<float>(sos, K, LC, tab, nsteps, false);
    for (float v : tab) if (!std::isfinite(v)) return INFINITY;
    // input: uniform in [-1, 1], fixed LCG
    std::vector<float> x((size_t)N);
    uint64_t st = 0x9E3779B97F4A7C15ull;
    for (auto &v : x) { st = st * 6364136223846793005ull + 1442695040888963407ull; v = (float)((double)(st >> 11) / 9007199254740992.0 * 2.0 - 1.0); }
    // float64 reference, sequential DF1
    std::vector<double> ref(x.begin(), x.end());
    for (int s = 0; s < K; ++s) {
        const double *co = &sos[s * 6];
        double x1 = 0, x2 = 0, y1 = 0, y2 = 0;
        for (int64_t n = 0; n < N; ++n) {
            const double v = ref[(size_t)n];
            const double y = co[0] * v + co[1] * x1 + co[2] * x2 - co[4] * y1 - co[5] * y2;
            x2 = x1; x1 = v; y2 = y1; y1 = y;
            ref[(size_t)n] = y;
        }
    }
    // float32 replay of sos_stream_kernel (one stream, no time segmentation)
    std::vector<float> cur(x);
    std::vector<float> carry((size_t)K * 4, 0.0f);        // vin1 vin2 y1 y2 per section
    double worst = 0.0, scale = 1.0;
    for (int64_t ts = 0; ts < N; ts += TILE) {
        float *d = &cur[(size_t)ts];                        // d[lane * LC + n]
        for (int s = 0; s < K; ++s) {
            const float *tb = &tab[(size_t)s * TS];
            const float b0 = tb[0], b1 = tb[1], b2 = tb[2], na1 = tb[3], na2 = tb[4];
            float *cs = &carry[(size_t)s * 4];
            float pv1[64], pv2[64];
            for (int l = 0; l < 64; ++l) {
                pv1[l] = l ? d[(l - 1) * LC + LC - 1] : cs[0];
                pv2[l] = l ? d[(l - 1) * LC + LC - 2] : cs[1];
            }
            cs[0] = d[63 * LC + LC - 1]; cs[1] = d[63 * LC + LC - 2];
            float s0[64], s1[64];
            for (int l = 0; l < 64; ++l) {
                float *c = d + l * LC;
                for (int n = LC - 1; n >= 0; --n) {          // (1a) in place, descending
                    const float x1 = n >= 1 ? c[n - 1] : pv1[l];
                    const float x2 = n >= 2 ? c[n - 2] : (n == 1 ? pv1[l] : pv2[l]);
                    c[n] = fmaf(b2, x2, fmaf(b1, x1, b0 * c[n]));
                }
                float u1 = l ? 0.0f : cs[2], u2 = l ? 0.0f : cs[3];   // (1b) end state from zero (lane 0: carried) state
                for (int n = 0; n < LC; ++n) { const float u = fmaf(na1, u1, fmaf(na2, u2, c[n])); u2 = u1; u1 = u; }
                s0[l] = u1; s1[l] = u2;
            }
            const float *pm = tb + 8;                        // (2) the scan tree of the kernel
            for (int k = 0; k < 4; ++k) {
                float t0[64], t1[64];
                for (int l = 0; l < 64; ++l) { const bool src = (l & 15) >= (1 << k); t0[l] = src ? s0[l - (1 << k)] : 0.0f; t1[l] = src ? s1[l - (1 << k)] : 0.0f; }
                for (int l = 0; l < 64; ++l) {
                    s0[l] += fmaf(pm[4 * k + 0], t0[l], pm[4 * k + 1] * t1[l]);
                    s1[l] += fmaf(pm[4 * k + 2], t0[l], pm[4 * k + 3] * t1[l]);
                }
            }
            {
                const float *mp = tb + 32;
                float a0[64], a1[64];
                for (int l = 0; l < 64; ++l) { const bool on = (l >> 4) & 1; a0[l] = on ? s0[(l & ~15) - 1] : 0.0f; a1[l] = on ? s1[(l & ~15) - 1] : 0.0f; }
                for (int l = 0; l < 64; ++l) {
                    const float *m = mp + 4 * (l & 15);
                    s0[l] += fmaf(m[0], a0[l], m[1] * a1[l]);
                    s1[l] += fmaf(m[2], a0[l], m[3] * a1[l]);
                }
                const float c0 = s0[31], c1 = s1[31];
                for (int l = 32; l < 64; ++l) {
                    const float *m = mp + 4 * (l & 31);
                    const float n0 = s0[l] + fmaf(m[0], c0, m[1] * c1), n1 = s1[l] + fmaf(m[2], c0, m[3] * c1);
                    s0[l] = n0; s1[l] = n1;
                }
            }
            const float cy1 = cs[2], cy2 = cs[3];
            for (int l = 0; l < 64; ++l) {                   // (3) the recursion from the true start state
                float h1 = l ? s0[l - 1] : cy1, h2 = l ? s1[l - 1] : cy2;
                float *c = d + l * LC;
                for (int n = 0; n < LC; ++n) {
                    const float yv = fmaf(na1, h1, fmaf(na2, h2, c[n]));
                    c[n] = yv; h2 = h1; h1 = yv;
                }
            }
            cs[2] = d[63 * LC + LC - 1]; cs[3] = d[63 * LC + LC - 2];
        }
        for (int i = 0; i < TILE; ++i) {
            const double e = fabs((double)d[i] - ref[(size_t)ts + i]);
            if (!(e <= worst)) worst = e;                     // NaN-propagating
            scale = fmax(scale, fabs(ref[(size_t)ts + i]));
        }
    }
    return 2.5 * worst / scale;
}

// Whether a cascade needs the refined start states (FFR kernels).  The lane scan rebuilds every lane's start state from
// zero-state pieces that are far larger than the state they cancel to when the poles sit next to z = 1 and the section's
// output is rough (20 Hz high-pass, notch, low peaking EQ, the K-weighting high-pass): the float64 kernel then loses
// 5e-9 of the output scale at 48 kHz and 1e-7 at 192 kHz on a plain DC-blocking high-pass, where a sequential float64
// recursion loses 2e-12 and 2e-11.  No closed form of the pole positions predicts that across numerators
// (a low-pass with the same poles is fine), so -- like the float32 estimate above -- it is MEASURED, once per plan and
// tile size: the kernel's float64 arithmetic without the refinement (same tile / lane structure, same tables, same scan
// tree) and the sequential float64 recursion are both replayed on 2^16 pseudo-random samples against a long double
// recursion.  `blocked` and `seq` are the two largest errors as shares of max(1, max|y|).  The rule:
//   float64 result (and the block energies):  refine when blocked > 2 max(seq, 2^-50) -- the blocking costs more than the
//                                             float64 recursion itself does;
//   float32 result:                           refine when blocked > 1e-10.  An error e flips the float32 rounding of about
//                                             (e / 2^-23) log2(2^-23 / e) of the outputs (one binade after the other, each
//                                             with its own ulp); at a typical error of a third of the largest that is
//                                             0.3 % at 1e-10, and 6 % at the 5e-9 of the 48 kHz high-pass.
template <typename TR>
static std::vector<TR> replay_sequential(const std::vector<double> &sos, int K, const std::vector<float> &x)
{
    std::vector<TR> ref(x.begin(), x.end());
    for (int s = 0; s < K; ++s) {
        const double *co = &sos[s * 6];
        const TR b0 = co[0], b1 = co[1], b2 = co[2], a1 = co[4], a2 = co[5];
        TR x1 = 0, x2 = 0, y1 = 0, y2 = 0;
        for (size_t n = 0; n < ref.size(); ++n) {
            const TR v = ref[n];
            const TR y = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2;
            x2 = x1; x1 = v; y2 = y1; y1 = y;
            ref[n] = y;
        }
    }
    return ref;
}

struct BlockedError { double blocked = 0.0, seq = 0.0, blocked_max = 0.0; };      // blocked_max: over the bands of a bank

static BlockedError f64_blocked_error(const std::vector<double> &sos, int K, int LC)
{
    const int TILE = 64 * LC, TS = tab_stride(LC);
    const int64_t N = 1 << 16;
    BlockedError out;
    std::vector<double> tab;
    int nsteps = 0;
    fill_tables<double>(sos, K, LC, tab, nsteps, false);
    for (double v : tab) if (!std::isfinite(v)) { out.blocked = out.seq = INFINITY; return out; }
    std::vector<float> x((size_t)N);
    uint64_t st = 0x9E3779B97F4A7C15ull;
    for (auto &v : x) { st = st * 6364136223846793005ull + 1442695040888963407ull; v = (float)((double)(st >> 11) / 9007199254740992.0 * 2.0 - 1.0); }
    const std::vector<ld> ref = replay_sequential<ld>(sos, K, x);
    const std::vector<double> seq = replay_sequential<double>(sos, K, x);
    // float64 replay of sos_stream_kernel without FFR (one stream, no time segmentation): the float32 replay above in double
    std::vector<double> cur(x.begin(), x.end());
    std::vector<double> carry((size_t)K * 4, 0.0);
    std::vector<double> pv1(64), pv2(64), s0(64), s1(64), t0(64), t1(64);
    for (int64_t ts = 0; ts < N; ts += TILE) {
        double *d = &cur[(size_t)ts];
        for (int s = 0; s < K; ++s) {
            const double *tb = &tab[(size_t)s * TS];
            const double b0 = tb[0], b1 = tb[1], b2 = tb[2], na1 = tb[3], na2 = tb[4];
            double *cs = &carry[(size_t)s * 4];
            for (int l = 0; l < 64; ++l) {
                pv1[l] = l ? d[(l - 1) * LC + LC - 1] : cs[0];
                pv2[l] = l ? d[(l - 1) * LC + LC - 2] : cs[1];
            }
            cs[0] = d[63 * LC + LC - 1]; cs[1] = d[63 * LC + LC - 2];
            for (int l = 0; l < 64; ++l) {
                double *c = d + l * LC;
                for (int n = LC - 1; n >= 0; --n) {
                    const double x1 = n >= 1 ? c[n - 1] : pv1[l];
                    const double x2 = n >= 2 ? c[n - 2] : (n == 1 ? pv1[l] : pv2[l]);
                    c[n] = fma(b2, x2, fma(b1, x1, b0 * c[n]));
                }
                double u1 = l ? 0.0 : cs[2], u2 = l ? 0.0 : cs[3];
                for (int n = 0; n < LC; ++n) { const double u = fma(na1, u1, fma(na2, u2, c[n])); u2 = u1; u1 = u; }
                s0[l] = u1; s1[l] = u2;
            }
            const double *pm = tb + 8;
            for (int k = 0; k < 4; ++k) {
                for (int l = 0; l < 64; ++l) { const bool src = (l & 15) >= (1 << k); t0[l] = src ? s0[l - (1 << k)] : 0.0; t1[l] = src ? s1[l - (1 << k)] : 0.0; }
                for (int l = 0; l < 64; ++l) {
                    s0[l] += fma(pm[4 * k + 0], t0[l], pm[4 * k + 1] * t1[l]);
                    s1[l] += fma(pm[4 * k + 2], t0[l], pm[4 * k + 3] * t1[l]);
                }
            }
            {
                const double *mp = tb + 32;
                for (int l = 0; l < 64; ++l) { const bool on = (l >> 4) & 1; t0[l] = on ? s0[(l & ~15) - 1] : 0.0; t1[l] = on ? s1[(l & ~15) - 1] : 0.0; }
                for (int l = 0; l < 64; ++l) {
                    const double *m = mp + 4 * (l & 15);
                    s0[l] += fma(m[0], t0[l], m[1] * t1[l]);
                    s1[l] += fma(m[2], t0[l], m[3] * t1[l]);
                }
                const double c0 = s0[31], c1 = s1[31];
                for (int l = 32; l < 64; ++l) {
                    const double *m = mp + 4 * (l & 31);
                    const double n0 = s0[l] + fma(m[0], c0, m[1] * c1), n1 = s1[l] + fma(m[2], c0, m[3] * c1);
                    s0[l] = n0; s1[l] = n1;
                }
            }
            const double cy1 = cs[2], cy2 = cs[3];
            for (int l = 0; l < 64; ++l) {
                double h1 = l ? s0[l - 1] : cy1, h2 = l ? s1[l - 1] : cy2;
                double *c = d + l * LC;
                for (int n = 0; n < LC; ++n) {
                    const double yv = fma(na1, h1, fma(na2, h2, c[n]));
                    c[n] = yv; h2 = h1; h1 = yv;
                }
            }
            cs[2] = d[63 * LC + LC - 1]; cs[3] = d[63 * LC + LC - 2];
        }
    }
    ld scale = 1.0L, wb = 0.0L, wq = 0.0L;
    for (size_t i = 0; i < (size_t)N; ++i) {
        const ld eb = fabsl((ld)cur[i] - ref[i]), eq = fabsl((ld)seq[i] - ref[i]);
        if (!(eb <= wb)) wb = eb;                             // NaN-propagating
        if (!(eq <= wq)) wq = eq;
        scale = fmaxl(scale, fabsl(ref[i]));
    }
    out.blocked = (double)(wb / scale);
    out.seq = (double)(wq / scale);
    return out;
}

constexpr double REFINE_F32_RESULT = 1e-10;       // largest blocked error a float32 result is left with
constexpr double REFINE_F64_FACTOR = 2.0;         // ... and a float64 result, as a multiple of the sequential recursion's own
constexpr double REFINE_F64_FLOOR = 0x1p-50;

static int lc_index(int LC) { return LC == 16 ? 0 : (LC == 32 ? 1 : 2); }

// the measured errors of the plan's worst band at tile size LC (lazy)
static BlockedError plan_blocked_error(SosPlan *pl, int LC)
{
    const int i = lc_index(LC);
    bool known;
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        known = pl->blocked_known[i] != 0;
    }
    if (!known) {
        // The replay runs OUTSIDE the lock (about 10 ms for four sections, a second for 512): the plan's coefficients never
        // change, two threads that race here compute the same numbers, and nobody else's plan lookup waits for them.
        BlockedError worst;
        double bmax = 0.0;
        for (int b = 0; b < pl->NB; ++b) {
            std::vector<double> one(pl->sos.begin() + (size_t)b * pl->K * 6, pl->sos.begin() + (size_t)(b + 1) * pl->K * 6);
            const BlockedError e = f64_blocked_error(one, pl->K, LC);
            // a float64 result: the band furthest past its own bar decides; a float32 result: the largest error of any band
            if (b == 0 || !(e.blocked / fmax(e.seq, REFINE_F64_FLOOR) <= worst.blocked / fmax(worst.seq, REFINE_F64_FLOOR))) worst = e;
            if (!(e.blocked <= bmax)) bmax = e.blocked;
        }
        std::lock_guard<std::mutex> lk(g_plan_mu);
        pl->blocked[i][0] = worst.blocked; pl->blocked[i][1] = worst.seq; pl->blocked[i][2] = bmax;
        pl->blocked_known[i] = 1;
    }
    std::lock_guard<std::mutex> lk(g_plan_mu);
    BlockedError e;
    e.blocked = pl->blocked[i][0]; e.seq = pl->blocked[i][1]; e.blocked_max = pl->blocked[i][2];
    return e;
}
// The decision, per cascade, tile size and result dtype (float64 arithmetic only).  Non-finite estimates (an unstable
// cascade) refine nothing: there is no accuracy to keep.
static bool plan_refine(SosPlan *pl, int LC, bool f64_result)
{
    const BlockedError e = plan_blocked_error(pl, LC);
    if (!std::isfinite(e.blocked) || !std::isfinite(e.seq) || !std::isfinite(e.blocked_max)) return false;
    return f64_result ? e.blocked > REFINE_F64_FACTOR * fmax(e.seq, REFINE_F64_FLOOR) : e.blocked_max > REFINE_F32_RESULT;
}

static double plan_err_bound(SosPlan *pl)
{
    std::lock_guard<std::mutex> lk(g_plan_mu);
    if (pl->err_bound_f32 < 0) {
        double worst = 0.0;
        for (int b = 0; b < pl->NB; ++b) {
            std::vector<double> one(pl->sos.begin() + (size_t)b * pl->K * 6, pl->sos.begin() + (size_t)(b + 1) * pl->K * 6);
            worst = fmax(worst, f32_error_bound(one, pl->K));
        }
        pl->err_bound_f32 = worst;
    }
    return pl->err_bound_f32;
}
static double auto_bound()
{
    const char *e = getenv("TFX_AUTO_F32_BOUND");
    // precision = "auto": float32 when the estimated largest error (relative to max(1, max|y|)) stays below this --
    // a fifth of the tolerance of the reference's own CUDA path (1e-4, tests/test_cuda_kernels.py:23-24)
    return (e && *e) ? atof(e) : 2e-5;
}

static std::shared_ptr<SosPlan> get_plan(const double *sos_host, int64_t K, hipStream_t stream, int64_t NB = 1)
{
    return g_plans.get(sos_host, (size_t)(NB * K * 6) * sizeof(double), {NB}, stream, [&] {
        auto pl = std::make_shared<SosPlan>();
        pl->K = (int)K;
        pl->NB = (int)NB;
        pl->sos.assign(sos_host, sos_host + NB * K * 6);
        pl->warm = 0;
        for (int64_t b = 0; b < NB; ++b) {     // every band must have forgotten its start state
            std::vector<double> one(sos_host + b * K * 6, sos_host + (b + 1) * K * 6);
            const int64_t w = warmup_length(one, (int)K);
            if (w < 0) { pl->warm = -1; break; }
            if (w > pl->warm) pl->warm = w;
        }
        return pl;
    });
}

static bool plan_unit_ok(SosPlan *pl)
{
    std::lock_guard<std::mutex> lk(g_plan_mu);
    if (pl->unit_ok < 0) {
        bool ok = true;
        for (int b = 0; b < pl->NB && ok; ++b)
            ok = unit_form_ok(std::vector<double>(pl->sos.begin() + (size_t)b * pl->K * 6, pl->sos.begin() + (size_t)(b + 1) * pl->K * 6), pl->K);
        pl->unit_ok = ok ? 1 : 0;
    }
    return pl->unit_ok != 0;
}

template <typename TC> static void build_table(SosPlan *pl, int LC, bool unit, SosPlan::Table &t)
{
    std::vector<TC> h;
    for (int b = 0; b < pl->NB; ++b) {
        std::vector<double> one(pl->sos.begin() + (size_t)b * pl->K * 6, pl->sos.begin() + (size_t)(b + 1) * pl->K * 6);
        std::vector<TC> hb;
        fill_tables<TC>(one, pl->K, LC, hb, t.nsteps, unit);
        h.insert(h.end(), hb.begin(), hb.end());
    }
    t.buf = std::make_unique<DeviceBuffer>(h);          // synchronous copy from a temporary: once per distinct filter
}
// The one way to a plan's device tables: sets p.tab / p.nsteps for the arithmetic type and for the kernel that will read them
// -- its tile size G.LC (16, 32, 64) and its form G.UNIT -- building the table on first use.  Every (type, LC, form) has a
// table of its own.
static void table_for(SosParams &p, SosPlan *pl, bool f32, const SosKernel &G)
{
    std::lock_guard<std::mutex> lk(g_plan_mu);
    SosPlan::Table &t = pl->tab[f32 ? 0 : 1][lc_index(G.LC)][G.UNIT ? 1 : 0];
    if (!t.buf) {
        if (f32) build_table<float>(pl, G.LC, G.UNIT, t);
        else build_table<double>(pl, G.LC, G.UNIT, t);
    }
    p.tab = t.buf->p; p.nsteps = t.nsteps;
}

void sos_clear_plans() { g_plans.clear(); }

static int g_cus[TFX_MAX_DEVICES] = {0};
static int device_cus()
{
    const int dev = current_device();
    if (!g_cus[dev]) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, dev) == hipSuccess) g_cus[dev] = pr.multiProcessorCount;
        if (g_cus[dev] <= 0) g_cus[dev] = 256;
    }
    return g_cus[dev];
}

// Time segmentation.  Streams are persistent (one wavefront walks its whole segment), so the
// launch should be exactly ONE resident round: nstreams <= CUs x resident waves, otherwise the
// second round doubles the time.  `resident_waves_per_cu` comes from the occupancy query of the
// kernel actually launched.  Segments shorter than 8 x warm-up are not worth their halo.
static void plan_segments(SosParams &p, int64_t plan_warm, int TILE, int resident_waves_per_cu)
{
    const int64_t capacity = plan_warm >= 0 ? (int64_t)device_cus() * resident_waves_per_cu : 0;
    const SosRoute r = sos_halo_plan(p.C, p.T, plan_warm, TILE, capacity, env_i64("TFX_SOS_NSEG", 0));      // the formula: sos_route.h
    p.nseg = (int)r.nseg; p.seg_len = r.seg_len; p.warm = r.warm;
}

// Zero-phase passes: the segmentation must not depend on an occupancy query, because tfx_sos_filtfilt_plan_info reports it
// without a device.  The FF kernels run LC = 32 at two workgroups per CU (launch bounds; 72 KB of LDS each at K = 4) unless
// the carry of a long cascade leaves room for one only.
constexpr int FF_LC = 32;
// the kernel of a pass (1 = forward, 2 = reverse): a float64 result takes the refined start states in both passes; a float32
// result is 20 times inside its bar without
constexpr SosKernel ff_kernel(int pass, bool f64_result) { return {.LC = FF_LC, .FF = pass, .FFR = f64_result}; }
static size_t ff_shmem(int K)
{
    return 4 * (size_t)sos_wave_lds_bytes<double, double, double, FF_LC>(1, K);      // float32 at either end: the same, the stage holds the wider type
}
static int ff_blocks_per_cu(int K) { return 2 * ff_shmem(K) <= 160 * 1024 ? 2 : 1; }

// ------------------------------------------------------------------------------------------
// Hand-off route (sos_route.h): what runs in front of the result launch.
// ------------------------------------------------------------------------------------------
constexpr int HO_LC = 32;
static_assert(64 * HO_LC == SOS_HANDOFF_QUANTUM, "hand-off segments are whole tiles of the end-state kernel");
// the end-state kernel: refined lane scan exactly where the result kernel's is (an end state is a float64 result of the cascade)
constexpr SosKernel ends_kernel(bool refine) { return {.LC = HO_LC, .FFR = refine, .ENDS = true}; }

// what a forward call hands to launch_one for the route decision, and what it gets back
struct SosRouting {
    SosPlan *pl = nullptr;
    bool eligible = false;        // the call may take the hand-off route (sos_forward_impl)
    bool refine = false;          // plan_refine for the call's kernel geometry and result dtype
    int64_t wave_slots = 0;       // > 0: given (the route query); 0: the device's, from the occupancy of the kernel launched
    bool query = false;           // decide only: nothing is allocated or launched
    SosRoute route;               // out
};

// P^(2^k) of the plan for segments of L samples, enough levels for nseg segments (lazy, a few L per plan)
static std::shared_ptr<SosPlan::Handoff> handoff_powers(SosPlan *pl, int64_t L, int64_t nseg)
{
    int nlev = 0;
    while (((int64_t)1 << nlev) < nseg - 1) ++nlev;
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        auto it = pl->handoff.find(L);
        if (it != pl->handoff.end() && (it->second->nlev >= nlev || !it->second->ok)) return it->second;
    }
    // outside the lock, like the replays of plan_blocked_error: the coefficients never change, racing threads compute the same
    auto h = std::make_shared<SosPlan::Handoff>();
    h->nlev = nlev;
    handoff_power_table(pl->sos, pl->K, L, nlev, h->pw, h->ok);
    std::lock_guard<std::mutex> lk(g_plan_mu);
    if (pl->handoff.size() >= 8) pl->handoff.clear();
    pl->handoff[L] = h;
    return h;
}

// The launches in front of the result pass; returns the per-stream start states [C * nseg, D] (slot 0 of a row is unused).
// Everything goes to the caller's stream with scratch() buffers: no host synchronisation.
template <typename TIn>
static const double *handoff_states(const SosParams &p, SosPlan *pl, SosPlan::Handoff *ho, bool refine, hipStream_t stream)
{
    const int D = 2 * p.K + 2;
    const int64_t nstreams = p.C * p.nseg;
    TFX_CHECK(nstreams * D < ((int64_t)1 << 30) && p.C <= INT32_MAX, "sos_forward: %lld segments are too many for the hand-off route", (long long)nstreams);
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        if (!ho->buf && !ho->pw.empty()) ho->buf = std::make_unique<DeviceBuffer>(ho->pw);
    }
    const double *pw = ho->buf ? (const double *)ho->buf->p : nullptr;
    const size_t bytes = (size_t)nstreams * D * sizeof(double);
    double *ends = (double *)scratch("sos_ho_end", bytes, stream);
    double *state = (double *)scratch("sos_ho_state", bytes, stream);
    double *work = (double *)scratch("sos_ho_work", 2 * bytes, stream);
    SosParams e = p;
    e.y = nullptr; e.taps = nullptr; e.sx_out = nullptr; e.sy_out = nullptr;
    e.ep_stat = -1; e.ep_partial = nullptr; e.nf_flag = nullptr; e.fair = 0; e.nt = 0;
    e.ho_end = ends; e.ho_state = nullptr;
    const size_t shmem = 4 * (size_t)sos_wave_lds_bytes<TIn, TIn, double, HO_LC>(1, p.K);
    TFX_CHECK(shmem <= 160 * 1024, "sos_forward: K=%d needs %zu B of LDS on the hand-off route (max 163840)", p.K, shmem);
    const auto ends_pass = [&](const char *name) {
        const auto go = [&](auto kern) {
            if (shmem > 64 * 1024) TFX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
            ProfScope ps(name, stream);
            hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(nstreams, 4)), dim3(256), shmem, stream, e);
            TFX_HIP(hipGetLastError());
        };
        table_for(e, pl, false, ends_kernel(refine));
        if (refine) go(sos_stream_kernel<TIn, TIn, double, ends_kernel(true)>);
        else go(sos_stream_kernel<TIn, TIn, double, ends_kernel(false)>);
    };
    const auto scan = [&](const char *name, int second) {
        ProfScope ps(name, stream);
        hipLaunchKernelGGL(sos_handoff_scan_kernel, dim3((unsigned)p.C), dim3(256), 0, stream, ends, state, pw, work, p.nseg, D, ho->nlev_for(p.nseg), second);
        TFX_HIP(hipGetLastError());
    };
    ends_pass("sos_handoff_ends_kernel");
    scan("sos_handoff_scan_kernel", 0);
    if (refine) {
        e.ho_state = state;
        ends_pass("sos_handoff_refine_ends_kernel");
        scan("sos_handoff_refine_scan_kernel", 1);
    }
    return state;
}

// The one launch of the cascade kernel: LDS size, segmentation, flag scratch, the launch and the repair launch behind it.
// MEAS: the measuring pass arrives with its segmentation decided (block_energy_plan: nseg, warm, ms_bps; fair_nw = 2), so the
// occupancy query and plan_segments are not for it.  `ep`: the Epilogue an EPI kernel serves (where its statistic goes).
// `rt`: a forward call's routing (sos_route): the zero-phase passes have none and keep the halo plan.
template <typename TIn, typename TOut, typename TC, SosKernel G>
static void launch_one(SosParams p, const Epilogue *ep, int64_t plan_warm, hipStream_t stream, SosRouting *rt = nullptr)
{
    constexpr int LC = G.LC, FF = G.FF;
    constexpr bool SUMB = G.SUMB, EPI = G.EPI, MEAS = G.MEAS;
    const int nbl = SUMB ? p.nsum : 1;
    const size_t shmem = 4 * (size_t)sos_wave_lds_bytes<TIn, TOut, TC, LC>(nbl, p.K);
    if constexpr (MEAS) TFX_CHECK(shmem <= 160 * 1024, "sos_block_energy: K=%d needs %zu B of LDS (max 163840)", p.K, shmem);
    else TFX_CHECK(shmem <= 160 * 1024, "sos_forward: %d band(s) x K=%d need %zu B of LDS (max 163840)", nbl, p.K, shmem);
    auto kern = sos_stream_kernel<TIn, TOut, TC, G>;
    if (!EPI) p.ep_stat = -1;                      // the plain instantiation has no epilogue code
    const bool query = rt && rt->query;
    if (shmem > 64 * 1024 && !query)
        TFX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    if constexpr (!MEAS) {
        static int blocks_per_cu_tab[TFX_MAX_DEVICES] = {0};     // per template instance and device
        static size_t blocks_shmem_tab[TFX_MAX_DEVICES] = {0};
        const int dev = current_device();
        int &blocks_per_cu = blocks_per_cu_tab[dev];
        size_t &blocks_shmem = blocks_shmem_tab[dev];
        if constexpr (FF != 0) {
            // the plan query's assumption, checked once per instance, device and LDS size against what the runtime can hold
            if (!blocks_per_cu || blocks_shmem != shmem) {
                int nb = 0;
                TFX_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kern, 256, shmem) == hipSuccess &&
                          nb >= ff_blocks_per_cu(p.K), "sos_filtfilt: %d workgroup(s) per CU fit, the segment plan counts on %d", nb,
                          ff_blocks_per_cu(p.K));
                blocks_shmem = shmem;
            }
            blocks_per_cu = ff_blocks_per_cu(p.K);
        } else if (!(rt && rt->wave_slots > 0) && (!blocks_per_cu || blocks_shmem != shmem)) {
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kern, 256, shmem) != hipSuccess || nb < 1) nb = 1;
            blocks_per_cu = nb;
            blocks_shmem = shmem;
        }
        if constexpr (FF != 0) plan_segments(p, plan_warm, 64 * LC, blocks_per_cu * 4);
        else {
            SosRouteQuery q;
            q.C = p.C; q.T = p.T; q.plan_warm = plan_warm; q.K = p.K; q.tile = 64 * LC;
            q.wave_slots = rt && rt->wave_slots > 0 ? rt->wave_slots : (int64_t)device_cus() * blocks_per_cu * 4;
            q.force_nseg = env_i64("TFX_SOS_NSEG", 0);
            q.handoff = (int)env_i64("TFX_SOS_HANDOFF", -1);
            q.eligible = rt && rt->eligible; q.refine = rt && rt->refine;
            SosRoute r = sos_route(q);
            std::shared_ptr<SosPlan::Handoff> ho;
            if (r.route == SOS_ROUTE_HANDOFF) {
                ho = handoff_powers(rt->pl, r.seg_len, r.nseg);
                if (!ho->ok) { q.eligible = false; r = sos_route(q); }      // P overflows: a truly unstable cascade keeps today's plan
            }
            p.nseg = (int)r.nseg; p.seg_len = r.seg_len; p.warm = r.warm;
            if (rt) rt->route = r;
            if (query) return;
            if (r.route == SOS_ROUTE_HANDOFF) p.ho_state = handoff_states<TIn>(p, rt->pl, ho.get(), rt->refine, stream);
        }
        p.fair_nw = blocks_per_cu < 2 ? 1 : (blocks_per_cu > 4 ? 4 : blocks_per_cu);      // one wave of every resident workgroup per SIMD
        if (p.fair_nw < 2) p.fair = 0;
    }
    const int64_t nstreams = p.C * p.nseg;
    if constexpr (MEAS) TFX_CHECK(nstreams <= INT32_MAX, "sos_block_energy: %lld streams are too many for one launch", (long long)nstreams);
    const unsigned grid = (unsigned)ceil_div(nstreams, 4);
    if (p.ep_stat >= 0) {                  // streams that have nothing to store leave their (zeroed) slot alone
        p.ep_partial = (double *)scratch("sos_ep_partial", (size_t)nstreams * sizeof(double), stream);
        TFX_HIP(hipMemsetAsync(p.ep_partial, 0, (size_t)nstreams * sizeof(double), stream));
    }
    p.nf_flag = nullptr;
    if (p.nseg > 1)                        // see sos_nonfinite_fix_kernel: every stream writes its slot, no memset needed
        p.nf_flag = (int *)scratch("sos_nf_flag", (size_t)nstreams * sizeof(int), stream);
    {
        ProfScope ps(MEAS ? "sos_block_energy_kernel" : FF == 1 ? "sos_filtfilt_forward_kernel" : FF == 2 ? "sos_filtfilt_reverse_kernel"
                     : sizeof(TC) == 8 ? "sos_stream_kernel<f64>" : "sos_stream_kernel<f32>", stream);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), shmem, stream, p);
        TFX_HIP(hipGetLastError());
    }
    if (p.nseg > 1) {                      // ~2 us on cfg 2 (measured by leaving it out)
        const auto fix = [&] {
            if constexpr (MEAS) hipLaunchKernelGGL(sos_block_energy_fix_kernel, dim3((unsigned)p.C), dim3(256), 0, stream, p);
            else hipLaunchKernelGGL(sos_nonfinite_fix_kernel<TOut>, dim3((unsigned)p.C), dim3(256), 0, stream, p, nbl, SUMB ? p.C_in * nbl : p.C);
            TFX_HIP(hipGetLastError());
        };
        if constexpr (MEAS || FF != 0) {   // the zero-phase and measuring profiles name every launch of the call
            ProfScope ps(MEAS ? "sos_block_energy_fix_kernel" : "sos_nonfinite_fix_kernel", stream);
            fix();
        } else fix();
    }
    if (p.ep_stat >= 0)
        stat_finish(p.ep_partial, ep->per_row ? p.C : 1, ep->per_row ? p.nseg : nstreams, p.ep_stat, ep->stat_out, stream);
}

// Which kernel a forward call runs: sos_choose decides it, the lists behind it compile it, a static_assert holds the two together.
// The type family of a call: float32 signals with float32 / float64 arithmetic (main), the other dtype mixes (rare), and the
// sum mode with float32 / float64 arithmetic.
enum class SosFamily { MainF32, MainF64, Rare, SumF32, SumF64 };

// Cascades whose lane scan costs the result accuracy (poles next to z = 1 under a rough output; plan_refine, decided per
// cascade and for the dtype of the result) take the refined kernels.  Those exist for the shipping geometry only: LC = 64
// on aligned rows, LC = 32 on the dword path; LC = 16 for the rare dtype mixes and the sum mode as before.  The decision
// is made at the tile size of that geometry -- the one the refined launch runs -- whatever TFX_SOS_VARIANT asks for: a
// variant with fewer samples per lane is never left unrefined where the shipping one is refined.  Every other cascade runs the kernel, and computes the bits, it did without this rule.
constexpr int sos_refine_lc(SosFamily fam, bool vec) { return fam == SosFamily::MainF32 || fam == SosFamily::MainF64 ? (vec ? 64 : 32) : 16; }

// The kernel of a call.  `vec`: aligned rows (16-byte path); `taps`: section taps asked for; `ep`: an epilogue asked for --
// the chosen kernel applies it where G.EPI says so, separate passes over y otherwise; `refine`: plan_refine at sos_refine_lc
// (float64 arithmetic only); `unit_ok`: the plan has a unit-b0 form; `knob`: TFX_SOS_VARIANT, negative = unset.
// Variants: 0 = LC32, 1 = LC16, 2 = LC32 + register prefetch, 3 = LC16 + prefetch, 4 = LC64, 5 = LC64 + prefetch.
// Register budgets (MINW, waves/SIMD) were chosen from -Rpass-analysis so that nothing spills.
constexpr SosKernel sos_choose(SosFamily fam, bool vec, bool taps, bool ep, bool refine, bool unit_ok, int knob)
{
    const bool F32 = fam == SosFamily::MainF32;
    const bool ffr = refine && !F32 && fam != SosFamily::SumF32;
    // rarely used dtype mixes and the sum mode: one configuration each (LC = 16: the sum's accumulator costs registers)
    if (fam == SosFamily::Rare) return {.LC = 16, .VEC = vec && !taps, .TAPS = taps, .MINW = vec && !taps ? 4 : 3, .FFR = ffr};
    if (fam == SosFamily::SumF32 || fam == SosFamily::SumF64) return {.LC = 16, .VEC = vec, .MINW = 3, .SUMB = true, .FFR = ffr};
    // the epilogue is fused on aligned rows without section taps, into kernels that exist for LC = 32 + prefetch and LC = 64
    const bool fuse = ep && vec && !taps;
    // float32 arithmetic: LC = 32 + register prefetch (4 waves per SIMD); float64: LC = 64 -- the kernel is bound by VALU
    // issue (1440 instructions per 2048-sample tile, ~100 % busy at 3 waves per SIMD), and 64 samples per lane halve the
    // scan's share per sample (0.352 vs 0.38-0.42 ms at cfg 2 on the same box)
    int variant = knob >= 0 ? knob : (F32 ? 2 : 4);
    if (variant >= 4 && !vec) variant = 2;         // LC = 64 exists for the aligned (16-byte) path only
    if (fuse) variant = variant >= 4 ? 4 : 2;
    if (ffr) variant = vec ? 4 : 0;                // refined start states: the shipping geometry only (sos_refine_lc)
    const int LC = variant >= 4 ? 64 : ((variant & 1) ? 16 : 32);
    if (taps || !vec)                              // debug taps / unaligned rows: plain dword path, but LC = 64 taps its aligned rows
        return {.LC = LC, .VEC = LC == 64, .TAPS = taps, .MINW = LC == 16 ? (F32 ? 5 : 3) : (F32 ? 3 : 2), .FFR = ffr};
    // the shipping float32-in / float32-out geometry (float64 arithmetic, LC = 64, aligned rows, no section taps) runs the
    // unit-b0 form when the cascade has one (unit_form_ok), plain and with the epilogue: same cascade arithmetic in both
    if (!F32 && variant == 4 && unit_ok) return {.LC = 64, .VEC = true, .MINW = 2, .EPI = fuse, .UNIT = true, .FFR = ffr};
    if (fuse && LC == 32) return {.LC = 32, .VEC = true, .PF = true, .MINW = 2, .EPI = true};
    if (fuse) return {.LC = 64, .VEC = true, .MINW = F32 ? 3 : 2, .EPI = true, .FFR = ffr};
    switch (variant) {
    case 0: return {.LC = 32, .VEC = true, .MINW = F32 ? 5 : 3};
    case 1: return {.LC = 16, .VEC = true, .MINW = F32 ? 8 : 5};
    case 2: return {.LC = 32, .VEC = true, .PF = true, .MINW = F32 ? 4 : 2};
    case 3: return {.LC = 16, .VEC = true, .PF = true, .MINW = F32 ? 6 : 4};
    case 4: return {.LC = 64, .VEC = true, .MINW = F32 ? 3 : 2, .FFR = ffr};      // 64 samples per lane: half the scan per sample
    case 5: return {.LC = 64, .VEC = true, .PF = true, .MINW = F32 ? 3 : 1};
    default: return {.LC = 0};                     // no such variant (sos_forward rejects the knob): in no list
    }
}

// does `f` hold for the kernel of any input of sos_choose in this family (the knob: unset and 0 ... 5)
template <typename F> constexpr bool sos_any_choice(SosFamily fam, F f)
{
    for (int in = 0; in < 32; ++in)
        for (int knob = -1; knob <= 5; ++knob)
            if (f(sos_choose(fam, in & 1, in & 2, in & 4, in & 8, in & 16, knob))) return true;
    return false;
}

// A list of compiled instances: `launch` takes a runtime SosKernel to the instance equal to it.  `matches`: every kernel
// sos_choose picks in `fam` is in the list, and every kernel of the list is picked (this file's compile time is its instances).
template <SosKernel... Gs> struct SosKernels {
    static constexpr bool has(SosKernel g) { return ((g == Gs) || ...); }
    static constexpr bool matches(SosFamily fam)
    {
        return !sos_any_choice(fam, [](SosKernel g) { return !has(g); }) && (sos_any_choice(fam, [](SosKernel g) { return g == Gs; }) && ...);
    }
    template <typename TIn, typename TOut, typename TC>
    static void launch(SosKernel g, const SosParams &p, const Epilogue *ep, int64_t plan_warm, hipStream_t stream, SosRouting *rt = nullptr)
    {
        const bool found = ((g == Gs && (launch_one<TIn, TOut, TC, Gs>(p, ep, plan_warm, stream, rt), true)) || ...);
        TFX_CHECK(found, "sos: no kernel instance LC=%d VEC=%d TAPS=%d PF=%d EPI=%d UNIT=%d FFR=%d", g.LC, g.VEC, g.TAPS, g.PF, g.EPI, g.UNIT, g.FFR);
    }
};

template <bool F32, SosKernel... More> using SosMainKernels = SosKernels<
    SosKernel{.LC = 32, .VEC = true, .MINW = F32 ? 5 : 3},                     // aligned rows: variants 0 ... 5
    SosKernel{.LC = 16, .VEC = true, .MINW = F32 ? 8 : 5},
    SosKernel{.LC = 32, .VEC = true, .PF = true, .MINW = F32 ? 4 : 2},
    SosKernel{.LC = 16, .VEC = true, .PF = true, .MINW = F32 ? 6 : 4},
    SosKernel{.LC = 64, .VEC = true, .MINW = F32 ? 3 : 2},
    SosKernel{.LC = 64, .VEC = true, .PF = true, .MINW = F32 ? 3 : 1},
    SosKernel{.LC = 32, .VEC = true, .PF = true, .MINW = 2, .EPI = true},       // ... with the epilogue: same tile geometry as
    SosKernel{.LC = 64, .VEC = true, .MINW = F32 ? 3 : 2, .EPI = true},         //     the plain kernel (bit-identical cascade output)
    SosKernel{.LC = 16, .MINW = F32 ? 5 : 3},                                   // unaligned rows
    SosKernel{.LC = 32, .MINW = F32 ? 3 : 2},
    SosKernel{.LC = 16, .TAPS = true, .MINW = F32 ? 5 : 3},                     // section taps (parity tests)
    SosKernel{.LC = 32, .TAPS = true, .MINW = F32 ? 3 : 2},
    SosKernel{.LC = 64, .VEC = true, .TAPS = true, .MINW = F32 ? 3 : 2},
    More...>;
using SosMainF64Kernels = SosMainKernels<false,
    SosKernel{.LC = 64, .VEC = true, .MINW = 2, .UNIT = true},                  // unit-b0 form
    SosKernel{.LC = 64, .VEC = true, .MINW = 2, .EPI = true, .UNIT = true},
    SosKernel{.LC = 64, .VEC = true, .MINW = 2, .FFR = true},                   // refined start states
    SosKernel{.LC = 64, .VEC = true, .MINW = 2, .EPI = true, .FFR = true},
    SosKernel{.LC = 64, .VEC = true, .MINW = 2, .UNIT = true, .FFR = true},
    SosKernel{.LC = 64, .VEC = true, .MINW = 2, .EPI = true, .UNIT = true, .FFR = true},
    SosKernel{.LC = 32, .MINW = 2, .FFR = true},
    SosKernel{.LC = 32, .TAPS = true, .MINW = 2, .FFR = true},
    SosKernel{.LC = 64, .VEC = true, .TAPS = true, .MINW = 2, .FFR = true}>;
using SosRareKernels = SosKernels<                                              // one list for the three type triples
    SosKernel{.LC = 16, .VEC = true, .MINW = 4}, SosKernel{.LC = 16, .VEC = true, .MINW = 4, .FFR = true},
    SosKernel{.LC = 16, .MINW = 3}, SosKernel{.LC = 16, .MINW = 3, .FFR = true},
    SosKernel{.LC = 16, .TAPS = true, .MINW = 3}, SosKernel{.LC = 16, .TAPS = true, .MINW = 3, .FFR = true}>;
template <SosKernel... More> using SosSumKernels = SosKernels<
    SosKernel{.LC = 16, .VEC = true, .MINW = 3, .SUMB = true}, SosKernel{.LC = 16, .MINW = 3, .SUMB = true}, More...>;
using SosSumF64Kernels = SosSumKernels<
    SosKernel{.LC = 16, .VEC = true, .MINW = 3, .SUMB = true, .FFR = true}, SosKernel{.LC = 16, .MINW = 3, .SUMB = true, .FFR = true}>;

static_assert(SosMainKernels<true>::matches(SosFamily::MainF32) && SosMainF64Kernels::matches(SosFamily::MainF64) &&
              SosRareKernels::matches(SosFamily::Rare) && SosSumKernels<>::matches(SosFamily::SumF32) &&
              SosSumF64Kernels::matches(SosFamily::SumF64), "sos_choose and a kernel list disagree: a chosen kernel is not compiled, or a compiled one is never chosen");

// The coefficient checks every entry point shares: K sections per band in 1 ... 512 (the per-wave carry, 4 values per section,
// lives in LDS next to the transposition stage), finite values, and -- where the caller's contract says so -- a0 = 1.
static void check_sos(const char *op, const double *sos_host, int64_t K, bool require_a0_one, int64_t NB = 1)
{
    TFX_CHECK(sos_host && K >= 1 && K <= 512, "%s: null coefficients or bad section count %lld (1 ... 512)", op, (long long)K);
    for (int64_t i = 0; i < NB * K * 6; ++i) TFX_CHECK(std::isfinite(sos_host[i]), "%s: non-finite SOS coefficient", op);
    if (require_a0_one)
        for (int64_t s = 0; s < NB * K; ++s) TFX_CHECK(sos_host[s * 6 + 3] == 1.0, "%s: sos[%lld, 3] (a0) must be 1", op, (long long)s);
}

// NB > 1 = filter-bank mode: NB independent K-section cascades applied to the same C_in input
// rows; output rows (and state rows) are band-major: row = band * C_in + c.  C is the number of
// INPUT rows.  sum_bands: the bands' outputs are accumulated into C_in output rows (`+`); the state
// tensors keep the band-major [K, NB * C_in, 2] layout.
// `rq`: the route query (sos_route_info) -- the same checks and decisions, then launch_one decides the route and returns
// before anything is allocated or launched; x and y are not looked at beyond their alignment (null = aligned).
static void sos_forward_impl(const void *x, int x_dtype, void *y, int y_dtype, int64_t C_in, int64_t T,
                             const double *sos_host, int64_t K,
                             const double *sx_in, const double *sy_in, double *sx_out, double *sy_out,
                             void *y_sections, int precision, hipStream_t stream, int64_t NB, bool sum_bands, const Epilogue *ep,
                             SosRouting *rq)
{
    Epilogue none;
    if (!ep) ep = &none;
    TFX_CHECK(!(ep->any() && y_sections), "sos_forward: no epilogue together with section taps");
    TFX_CHECK(ep->stat_mode < 0 || ep->stat_out, "sos_forward: statistic requested without an output buffer");
    TFX_CHECK(NB >= 1, "sos_forward: need at least one band");
    TFX_CHECK(!(sum_bands && y_sections), "sos_forward: no section taps in sum mode");
    const int64_t C = sum_bands ? C_in : C_in * NB;
    TFX_CHECK(C >= 0 && T >= 0 && K >= 0, "sos_forward: negative size");
    // the per-wave carry (4 values per section) lives in LDS next to the transposition stage
    TFX_CHECK(K <= 512, "sos_forward: at most 512 sections per cascade (got %lld); split the cascade", (long long)K);
    TFX_CHECK(x_dtype == TFX_F32 || x_dtype == TFX_F64, "sos_forward: bad x dtype %d", x_dtype);
    TFX_CHECK(y_dtype == TFX_F32 || y_dtype == TFX_F64, "sos_forward: bad y dtype %d", y_dtype);
    if (C == 0) return;
    if (rq && (T == 0 || K == 0)) return;          // nothing to segment: the query's default, one sequential pass
    TFX_CHECK((T == 0 || (x && y) || rq) && (K == 0 || sos_host), "sos_forward: null signal or coefficient pointer");   // an empty tensor has no storage
    const size_t st_bytes = (size_t)K * C_in * NB * 2 * sizeof(double);   // [K, NB * C_in, 2] in every mode
    TFX_CHECK(!(sum_bands && K == 0), "sos_forward: sum mode needs at least one section");
    if (T == 0 || K == 0) {
        // no samples: state passes through (iir_cpu.cpp writes back what it loaded);
        // no sections: y = x
        if (sx_out && K) { if (sx_in) TFX_HIP(hipMemcpyAsync(sx_out, sx_in, st_bytes, hipMemcpyDeviceToDevice, stream));
                           else TFX_HIP(hipMemsetAsync(sx_out, 0, st_bytes, stream)); }
        if (sy_out && K) { if (sy_in) TFX_HIP(hipMemcpyAsync(sy_out, sy_in, st_bytes, hipMemcpyDeviceToDevice, stream));
                           else TFX_HIP(hipMemsetAsync(sy_out, 0, st_bytes, stream)); }
        if (K == 0 && T > 0) {
            TFX_CHECK(x_dtype == y_dtype && NB == 1, "sos_forward: K=0 needs equal dtypes and a single band");
            TFX_HIP(hipMemcpyAsync(y, x, (size_t)C * T * (x_dtype == TFX_F32 ? 4 : 8), hipMemcpyDeviceToDevice, stream));
        }
        if (ep->any()) epilogue_as_passes(y, y_dtype, C, K == 0 ? T : 0, *ep, stream);
        return;
    }
    check_sos("sos_forward", sos_host, K, false, NB);

    const std::shared_ptr<SosPlan> plan = get_plan(sos_host, K, stream, NB);     // held until the launches are enqueued
    SosPlan *pl = plan.get();
    int prec = precision;
    if (prec == TFX_PREC_AUTO) prec = (plan_err_bound(pl) <= auto_bound()) ? TFX_PREC_F32 : TFX_PREC_F64;
    if (x_dtype == TFX_F64 || y_dtype == TFX_F64) prec = TFX_PREC_F64;   // f64 signals: always f64 math
    const bool f32 = prec == TFX_PREC_F32;
    const bool rare = !(x_dtype == TFX_F32 && y_dtype == TFX_F32);
    const int xsz = x_dtype == TFX_F32 ? 4 : 8, ysz = y_dtype == TFX_F32 ? 4 : 8;
    const bool vec = (((uintptr_t)x & 15) == 0) && (((uintptr_t)y & 15) == 0) && ((T * xsz) % 16 == 0) && ((T * ysz) % 16 == 0);
    TFX_CHECK(!sum_bands || x_dtype == y_dtype, "sos_forward: sum mode needs equal input and output dtypes");
    const int64_t knob = env_i64("TFX_SOS_VARIANT", -1);
    TFX_CHECK(knob <= 5, "sos_forward: TFX_SOS_VARIANT=%lld is outside 0 ... 5 (negative = unset)", (long long)knob);
    const SosFamily fam = sum_bands ? (f32 ? SosFamily::SumF32 : SosFamily::SumF64)
                        : rare ? SosFamily::Rare : (f32 ? SosFamily::MainF32 : SosFamily::MainF64);
    const bool refine = !f32 && plan_refine(pl, sos_refine_lc(fam, vec), y_dtype == TFX_F64);
    SosKernel G = sos_choose(fam, vec, y_sections != nullptr, ep->any(), refine, true, (int)knob);
    if (G.UNIT && !plan_unit_ok(pl)) G = sos_choose(fam, vec, y_sections != nullptr, ep->any(), refine, false, (int)knob);

    SosParams p{};
    p.x = x; p.y = y; p.taps = y_sections;
    p.sx_in = sx_in; p.sy_in = sy_in; p.sx_out = sx_out; p.sy_out = sy_out;
    p.C = C; p.C_in = C_in; p.T = T; p.K = (int)K; p.x_pitch = T;
    p.nt = 1;
    p.fair = 15;
    p.nsum = sum_bands ? (int)NB : 0;
    p.ep_stat = -1;
    // the epilogue runs in the kernels that have it; everything else runs the plain kernel and the same arithmetic as
    // separate passes over y
    if (G.EPI) { p.ep_gain = ep->gain; p.ep_scale = ep->scale; p.ep_clamp = ep->clamp; p.ep_stat = ep->stat_mode; }
    if (!rq) table_for(p, pl, f32, G);

    // The route (sos_route.h) is decided per kernel instance, in launch_one.  Hand-off serves the float64 arithmetic of one
    // cascade of up to SOS_HANDOFF_MAXK sections, main and rare dtype families; float32 arithmetic, banks and the sum mode keep
    // the halo plan (DESIGN.md 4.1.1 names them as follow-ups).
    SosRouting own;
    SosRouting *rt = rq ? rq : &own;
    rt->pl = pl;
    rt->eligible = !f32 && NB == 1 && !sum_bands && K <= SOS_HANDOFF_MAXK && (fam == SosFamily::MainF64 || fam == SosFamily::Rare);
    rt->refine = refine;
    const int64_t warm = pl->warm;
    if (fam == SosFamily::MainF32) SosMainKernels<true>::launch<float, float, float>(G, p, ep, warm, stream, rt);
    else if (fam == SosFamily::MainF64) SosMainF64Kernels::launch<float, float, double>(G, p, ep, warm, stream, rt);
    else if (fam == SosFamily::SumF32) SosSumKernels<>::launch<float, float, float>(G, p, ep, warm, stream, rt);
    else if (fam == SosFamily::SumF64 && x_dtype == TFX_F32) SosSumF64Kernels::launch<float, float, double>(G, p, ep, warm, stream, rt);
    else if (fam == SosFamily::SumF64) SosSumF64Kernels::launch<double, double, double>(G, p, ep, warm, stream, rt);
    else if (x_dtype == TFX_F32) SosRareKernels::launch<float, double, double>(G, p, ep, warm, stream, rt);
    else if (y_dtype == TFX_F32) SosRareKernels::launch<double, float, double>(G, p, ep, warm, stream, rt);
    else SosRareKernels::launch<double, double, double>(G, p, ep, warm, stream, rt);
    if (rq) return;
    if (ep->any() && !G.EPI) epilogue_as_passes(y, y_dtype, C, T, *ep, stream);
}

void sos_forward(const void *x, int x_dtype, void *y, int y_dtype, int64_t C_in, int64_t T,
                 const double *sos_host, int64_t K,
                 const double *sx_in, const double *sy_in, double *sx_out, double *sy_out,
                 void *y_sections, int precision, hipStream_t stream, int64_t NB, bool sum_bands, const Epilogue *ep)
{
    sos_forward_impl(x, x_dtype, y, y_dtype, C_in, T, sos_host, K, sx_in, sy_in, sx_out, sy_out, y_sections, precision, stream, NB,
                     sum_bands, ep, nullptr);
}

// The route a forward call of [C, T] takes (sos_route.h), decided by the call's own code path.  `sections`: section taps are
// asked for (they change the kernel, and with it the tile).  wave_slots > 0: the wavefronts the device is taken to hold -- no
// device is asked anything; 0: the current device's, as the launch counts them.  Rows are taken as 16-byte aligned.
// bytes_per_sample: signal traffic, one read per pass and one store (plus the section taps).
void sos_route_info(int64_t C, int64_t T, const double *sos_host, int64_t K, int x_dtype, int y_dtype, int precision, int sections,
                    int64_t wave_slots, int *route, int64_t *nseg, int64_t *seg_len, int64_t *warm, int *passes, double *bytes_per_sample)
{
    TFX_CHECK(wave_slots >= 0, "sos_route_info: negative wave_slots");
    SosRouting rq;
    rq.query = true;
    rq.wave_slots = wave_slots;
    rq.route.seg_len = T;
    sos_forward_impl(nullptr, x_dtype, nullptr, y_dtype, C, T, sos_host, K, nullptr, nullptr, nullptr, nullptr,
                     sections ? (void *)(uintptr_t)16 : nullptr /* asked for or not: never dereferenced */, precision, nullptr, 1, false, nullptr, &rq);
    const SosRoute &r = rq.route;
    if (route) *route = r.route;
    if (nseg) *nseg = r.nseg;
    if (seg_len) *seg_len = r.seg_len;
    if (warm) *warm = r.warm;
    if (passes) *passes = r.passes;
    const int xsz = x_dtype == TFX_F64 ? 8 : 4, ysz = y_dtype == TFX_F64 ? 8 : 4;
    if (bytes_per_sample) *bytes_per_sample = (double)r.passes * xsz + (double)ysz * (1 + (sections ? K : 0));
}

// ------------------------------------------------------------------------------------------
// Zero-phase filtering, scipy.signal.sosfiltfilt along each row: the cascade runs forward over the edge-extended row and then
// backward over its own output, each pass from the cascade's steady state for the first sample it sees, and the extension is
// dropped.  Two launches of the cascade kernel (FF = 1, 2) around ONE float64 intermediate [C, T + 2 padlen]: the extension is
// index arithmetic in the first pass's loads, the time reversal is the second pass's load and store addressing -- no padded,
// flipped or widened copy of the signal exists.  24 B per sample of float32 signal (4 + 8 + 8 + 4).  Both passes are cut into
// time segments exactly like the forward cascade (same warm-up bound, same repair of non-finite rows); in the reverse pass a
// segment's halo lies at LATER samples of the row.
// ------------------------------------------------------------------------------------------
int64_t sos_filtfilt_default_padlen(const double *sos_host, int64_t K)
{
    int64_t zb = 0, za = 0;
    for (int64_t s = 0; s < K; ++s) { zb += sos_host[s * 6 + 2] == 0.0; za += sos_host[s * 6 + 5] == 0.0; }
    return 3 * (2 * K + 1 - (zb < za ? zb : za));
}

// G_(s-1) at [s], s = 0 ... K: the DC gain of the first s sections, prod sum(b_j) / sum(a_j).  A pole at z = 1 has none.
static std::vector<double> filtfilt_gains(const double *sos_host, int64_t K)
{
    std::vector<double> g((size_t)K + 1);
    ld acc = 1.0L;
    g[0] = 1.0;
    for (int64_t s = 0; s < K; ++s) {
        const double *co = sos_host + s * 6;
        const ld den = (ld)co[3] + (ld)co[4] + (ld)co[5];
        TFX_CHECK(den != 0.0L, "sos_filtfilt: section %lld has a pole at z = 1: the cascade has no steady state to start from", (long long)s);
        acc *= ((ld)co[0] + (ld)co[1] + (ld)co[2]) / den;
        g[(size_t)s + 1] = (double)acc;
    }
    return g;
}

// the checks shared by the call and its plan query; returns the padlen in force
static int64_t filtfilt_check(int64_t C, int64_t T, const double *sos_host, int64_t K, int padtype, int64_t padlen)
{
    TFX_CHECK(C >= 0 && T >= 0, "sos_filtfilt: negative size");
    check_sos("sos_filtfilt", sos_host, K, true);
    TFX_CHECK(padtype >= TFX_PAD_ODD && padtype <= TFX_PAD_NONE, "sos_filtfilt: bad padtype %d", padtype);
    TFX_CHECK(padlen >= -1, "sos_filtfilt: negative padlen %lld (-1 = the default)", (long long)padlen);
    int64_t pad = padlen < 0 ? sos_filtfilt_default_padlen(sos_host, K) : padlen;
    if (padtype == TFX_PAD_NONE) pad = 0;
    TFX_CHECK(T > pad, "The length of the input vector x must be greater than padlen, which is %lld.", (long long)pad);
    TFX_CHECK(T <= (INT64_MAX / 64 - 2 * pad) / (C > 0 ? C : 1), "sos_filtfilt: size overflows");
    return pad;
}

static SosParams filtfilt_params(int pass, int64_t C, int64_t T, int64_t K, int padtype, int64_t pad)
{
    SosParams p{};
    p.C = C; p.C_in = C; p.T = T + 2 * pad; p.K = (int)K;
    p.x_pitch = pass == 1 ? T : p.T;
    p.fair = 15;
    p.ep_stat = -1;
    p.ff = pass; p.ff_padtype = padtype; p.ff_T = T; p.ff_pad = pad;
    return p;
}

void sos_filtfilt_plan_info(int64_t C, int64_t T, const double *sos_host, int64_t K, int padtype, int64_t padlen,
                            int64_t *default_padlen, int64_t *padlen_used, int64_t *work_elems, int64_t *warmup,
                            int *nseg_forward, int *nseg_reverse)
{
    const int64_t pad = filtfilt_check(C, T, sos_host, K, padtype, padlen);
    (void)filtfilt_gains(sos_host, K);
    const std::shared_ptr<SosPlan> plan = get_plan(sos_host, K, nullptr, 1);
    SosParams p = filtfilt_params(1, C > 0 ? C : 1, T, K, padtype, pad);
    plan_segments(p, plan->warm, 64 * FF_LC, ff_blocks_per_cu((int)K) * 4);      // both passes walk rows of T + 2 pad samples
    if (default_padlen) *default_padlen = sos_filtfilt_default_padlen(sos_host, K);
    if (padlen_used) *padlen_used = pad;
    if (work_elems) *work_elems = C * (T + 2 * pad);
    if (warmup) *warmup = plan->warm;
    if (nseg_forward) *nseg_forward = p.nseg;
    if (nseg_reverse) *nseg_reverse = p.nseg;
}

void sos_filtfilt_forward(const void *x, int x_dtype, void *y, int y_dtype, int64_t C, int64_t T, const double *sos_host, int64_t K,
                          int padtype, int64_t padlen, double *work, hipStream_t stream)
{
    TFX_CHECK(x_dtype == TFX_F32 || x_dtype == TFX_F64, "sos_filtfilt: bad x dtype %d", x_dtype);
    TFX_CHECK(y_dtype == TFX_F32 || y_dtype == TFX_F64, "sos_filtfilt: bad y dtype %d", y_dtype);
    const int64_t pad = filtfilt_check(C, T, sos_host, K, padtype, padlen);
    const std::vector<double> gains = filtfilt_gains(sos_host, K);
    if (C == 0) return;
    TFX_CHECK(x && y && work, "sos_filtfilt: null signal, result or workspace pointer");

    const std::shared_ptr<SosPlan> plan = get_plan(sos_host, K, stream, 1);      // held until the launches are enqueued
    SosPlan *pl = plan.get();
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        if (!pl->ff_gain) pl->ff_gain = std::make_unique<DeviceBuffer>(gains);
    }
    SosParams p = filtfilt_params(1, C, T, K, padtype, pad);
    const bool f64_result = y_dtype == TFX_F64;
    table_for(p, pl, false, ff_kernel(1, f64_result));     // (the two passes read the same table: same LC, same form)
    p.ff_gain = (const double *)pl->ff_gain->p;
    p.x = x; p.y = work;
    using Forward = SosKernels<ff_kernel(1, false), ff_kernel(1, true)>;
    if (x_dtype == TFX_F32) Forward::launch<float, double, double>(ff_kernel(1, f64_result), p, nullptr, pl->warm, stream);
    else Forward::launch<double, double, double>(ff_kernel(1, f64_result), p, nullptr, pl->warm, stream);
    p.ff = 2; p.x = work; p.y = y; p.x_pitch = p.T;
    if (f64_result) launch_one<double, double, double, ff_kernel(2, true)>(p, nullptr, pl->warm, stream);
    else launch_one<double, float, double, ff_kernel(2, false)>(p, nullptr, pl->warm, stream);
}

// ------------------------------------------------------------------------------------------
// Block energies: S[r, i] = sum of y[r, n]^2 over n in [e_i, e_(i+1)), e_i = (i num) / den, y = the float64 cascade of row r from
// zero state -- the measurement under a loudness meter (K-weighting, 100 ms blocks).  One launch of the cascade kernel (MEAS)
// that reads the signal once and writes nblk values per row; the filtered signal exists in registers only.
//
// Rows are cut into time segments like the forward cascade (same warm-up bound, same TFX_SOS_NSEG), with two differences.
// A segment owns whole blocks: it starts `warm` samples in front of a block edge, so every S[r, i] has one writer and no
// partial sums cross streams.  And the cut depends on the row length, the cascade and num / den alone -- not on the number of
// rows, not on the device: a row's bits are the same in every batch, and the plan query needs no GPU.  The target is one
// segment per wave slot of the part (256 CUs x 2 workgroups x 4 waves), and segments of at least 4 x warm-up: 2 rows x 28.8 M
// samples ran 0.191 / 0.140 / 0.119 ms with segments of 8 / 4 / 2 x warm-up, 8 x 2.88 M 0.181 / 0.106 / 0.071, but 64 x 2.88 M,
// which fills the part either way, 0.258 / 0.242 / 0.28: 4 x is the shortest that costs the full part nothing.
// ------------------------------------------------------------------------------------------
constexpr int MS_LC = 32;
constexpr SosKernel ms_kernel(bool refine) { return {.LC = MS_LC, .FFR = refine, .MEAS = true}; }
constexpr int64_t MS_STREAMS = 2048;
constexpr int64_t MS_SEQ_MAX = (int64_t)1 << 24;       // longest row one wavefront is asked to walk alone

struct BlockEnergyPlan { int64_t nblk, bps, warm; int nseg; };

static BlockEnergyPlan block_energy_plan(int64_t C, int64_t T, const double *sos_host, int64_t K, int64_t num, int64_t den)
{
    TFX_CHECK(C >= 0 && T >= 0, "sos_block_energy: negative size");
    check_sos("sos_block_energy", sos_host, K, true);
    TFX_CHECK(num >= 1 && den >= 1, "sos_block_energy: block length num / den needs num >= 1 and den >= 1");
    TFX_CHECK(num / 64 >= den, "sos_block_energy: blocks of num / den = %lld / %lld samples are shorter than 64", (long long)num, (long long)den);
    TFX_CHECK(T <= ((int64_t)1 << 61) / den && C <= INT32_MAX, "sos_block_energy: size overflows");
    const std::shared_ptr<SosPlan> plan = get_plan(sos_host, K, nullptr, 1);
    BlockEnergyPlan bp;
    bp.nblk = T * den / num;
    bp.bps = bp.nblk; bp.warm = 0; bp.nseg = 1;
    TFX_CHECK(plan->warm >= 0 || T <= MS_SEQ_MAX, "sos_block_energy: the cascade does not decay (no warm-up length), so rows cannot be cut into "
              "segments, and %lld samples are too many for one wavefront per row (max %lld)", (long long)T, (long long)MS_SEQ_MAX);
    if (plan->warm >= 0 && bp.nblk > 1) {
        const int64_t warm = (plan->warm + 255) & ~(int64_t)255;
        const int64_t force_nseg = env_i64("TFX_SOS_NSEG", 0);
        const int64_t covered = bp.nblk * num / den;                       // e_nblk
        int64_t len = ceil_div(covered, force_nseg > 0 ? force_nseg : MS_STREAMS);
        if (force_nseg <= 0 && len < 4 * warm) len = 4 * warm;
        if (len < warm) len = warm;
        if (len < 1) len = 1;
        const int64_t b = ceil_div(len * den, num);                        // e_b >= len >= warm: the halo of segment 1 starts inside the row
        if (b >= 1 && b < bp.nblk) { bp.bps = b; bp.nseg = (int)ceil_div(bp.nblk, b); bp.warm = warm; }
    }
    return bp;
}

void sos_block_energy_plan_info(int64_t C, int64_t T, const double *sos_host, int64_t K, int64_t num, int64_t den,
                                int64_t *nblk, int *nseg, int64_t *warm)
{
    const BlockEnergyPlan bp = block_energy_plan(C, T, sos_host, K, num, den);
    if (nblk) *nblk = bp.nblk;
    if (nseg) *nseg = bp.nseg;
    if (warm) *warm = bp.warm;
}

void sos_block_energy_forward(const void *x, int x_dtype, double *s, int64_t C, int64_t T, const double *sos_host, int64_t K,
                              int64_t num, int64_t den, hipStream_t stream)
{
    TFX_CHECK(x_dtype == TFX_F32 || x_dtype == TFX_F64, "sos_block_energy: bad x dtype %d", x_dtype);
    const BlockEnergyPlan bp = block_energy_plan(C, T, sos_host, K, num, den);
    if (C == 0 || bp.nblk == 0) return;
    TFX_CHECK(x && s, "sos_block_energy: null signal or result pointer");
    const std::shared_ptr<SosPlan> plan = get_plan(sos_host, K, stream, 1);      // held until the launches are enqueued
    SosPlan *pl = plan.get();
    // the energies are float64 results: a cascade whose lane scan costs more than the float64 recursion itself refines it
    const SosKernel G = ms_kernel(plan_refine(pl, MS_LC, true));
    SosParams p{};
    table_for(p, pl, false, G);
    p.x = x; p.y = s;
    p.C = C; p.C_in = C; p.T = T; p.K = (int)K; p.x_pitch = T;
    p.nseg = bp.nseg; p.warm = bp.warm;
    p.fair = 15; p.fair_nw = 2;
    p.ep_stat = -1;
    p.ms_num = num; p.ms_den = den; p.ms_nblk = bp.nblk; p.ms_bps = bp.bps;
    // the segmentation above is final (block_energy_plan): launch_one takes it as it is
    using Measuring = SosKernels<ms_kernel(false), ms_kernel(true)>;
    if (x_dtype == TFX_F32) Measuring::launch<float, float, double>(G, p, nullptr, pl->warm, stream);
    else Measuring::launch<double, double, double>(G, p, nullptr, pl->warm, stream);
}

// ------------------------------------------------------------------------------------------
// One launch per small streaming chunk:  SOS cascade -> direct FIR with carried history -> gain / clip
// (the reference's small-block caller is RealtimeProcessor._audio_callback, realtime/processor.py:253-292, over
// StreamProcessor's chunk loop, realtime/stream.py:234-273: a 2 x 512 block is launch-bound -- four to five kernels
// for a few microseconds of arithmetic).  One workgroup per channel: wave 0 runs the cascade stream body on the chunk
// (carried DF1 state in / out, float64 or float32 arithmetic, output rounded to float32 exactly like the IIR module's)
// straight into an LDS buffer that sits behind the channel's FIR history, then all four waves convolve [history |
// cascade output] with the taps from LDS, apply the gain / clip to what they store and write the next history.
// Same arithmetic as the staged passes (same cascade code with LC = 16, same float32 FMA order as fir_direct_simple_kernel).
// ------------------------------------------------------------------------------------------
struct ChunkParams {
    SosParams sos;           // x = the chunk [C, T] with row pitch sos.x_pitch; y is replaced by the LDS buffer inside the kernel
    const float *taps;       // device: [Hpad - H zeros | flipped taps (Kf) | zeros up to Hpad + 4]   (cached_taps)
                             // (the zeros only fill the float4 groups: the kernel never multiplies them)
    const float *hist_in;    // [C, Kf - 1] or null (= silence)
    float *hist_out;         // [C, Kf - 1] or null
    float *y;                // [C, T]
    int Kf;
    int Tpad;                // T rounded up to a multiple of 4
    float gain;
    int scale, clamp;
};

constexpr SosKernel chunk_kernel(bool vec) { return {.LC = 16, .VEC = vec}; }     // the cascade inside the chunk kernel (body alone)
template <typename TC, bool VEC>
__global__ void __launch_bounds__(1024) chunk_iir_fir_kernel(const ChunkParams q)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t c = blockIdx.x;
    const int T = (int)q.sos.T, H = q.Kf - 1;
    const int Hpad = (H + 3) & ~3;                         // the cascade output starts on a 16-byte boundary
    const int Kp = Hpad + 4;                               // padded tap count: leading zeros align the history, trailing ones fill the float4
    // ubuf = [Hpad - H zeros | history (H) | cascade output (T) | zeros]: every float4 the FIR phase touches is aligned
    float *ubuf = (float *)smem;                           // [Hpad + Tpad + 8]
    float *kp = ubuf + Hpad + q.Tpad + 8;                  // [Kp]
    char *stage = (char *)(kp + Kp);                       // cascade stage + carry (wave 0)
    float *u = ubuf + Hpad;
    for (int i = tid; i < Hpad; i += nthr) {
        const int j = i - (Hpad - H);
        ubuf[i] = (j >= 0 && q.hist_in) ? q.hist_in[c * H + j] : 0.0f;
    }
    for (int i = T + tid; i < q.Tpad + 8; i += nthr) u[i] = 0.0f;
    for (int i = tid; i < Kp; i += nthr) kp[i] = q.taps[i];
    if (q.sos.K == 0) {
        const float *xr = (const float *)q.sos.x + c * q.sos.x_pitch;
        for (int i = tid; i < T; i += nthr) u[i] = xr[i];
    } else if (wave == 0) {
        SosParams p = q.sos;
        p.y = (void *)(u - c * (int64_t)T);                // the body stores row c at y + c * T
        p.C_in = p.C;
        sos_stream_body<float, float, TC, chunk_kernel(VEC)>(p, c, stage, lane);
    }
    __syncthreads();
    // direct form, float32 FMA in tap order (as fir_direct_simple_kernel): y[n] = sum_k kp[k] * ubuf[n + k].  A thread owns
    // four consecutive outputs and slides an 8-sample register window over the taps: one ds_read_b128 of samples and one
    // (broadcast) of taps per 16 FMAs.
    const float4 *ub4 = (const float4 *)ubuf, *kp4 = (const float4 *)kp;
    for (int n0 = 4 * tid; n0 < T; n0 += 4 * nthr) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        float4 a = ub4[n0 >> 2];
        // taps [jlo, jhi) of the group at k; the sample window slides on by four either way
        const auto group = [&](int k, int jlo, int jhi) {
            const float4 b = ub4[((n0 + k) >> 2) + 1];
            const float4 h = kp4[k >> 2];
            const float win[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (jlo <= 0 && 0 < jhi) acc[r] = fmaf(h.x, win[r], acc[r]);
                if (jlo <= 1 && 1 < jhi) acc[r] = fmaf(h.y, win[r + 1], acc[r]);
                if (jlo <= 2 && 2 < jhi) acc[r] = fmaf(h.z, win[r + 2], acc[r]);
                if (jlo <= 3 && 3 < jhi) acc[r] = fmaf(h.w, win[r + 3], acc[r]);
            }
            a = b;
        };
        // The padding taps are never multiplied: 0 * NaN = 0 * Inf = NaN would carry a non-finite sample to outputs outside
        // its K-sample reach (the trailing zeros meet the three samples AFTER the output, the leading ones older history).
        // First group: its Hpad - H leading zeros are skipped; last group: the last real tap and three zeros.  Real taps are
        // multiplied whatever their value, in the same order as before: finite data keeps its bits.
        group(0, Hpad - H, Kp == 4 ? 1 : 4);
        for (int k = 4; k < Kp - 4; k += 4) group(k, 0, 4);
        if (Kp > 4) group(Kp - 4, 0, 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + r;
            if (n < T) {
                float o = acc[r];
                if (q.scale) o *= q.gain;
                if (q.clamp) o = clamp_unit(o);
                q.y[c * T + n] = o;
            }
        }
    }
    if (q.hist_out)
        for (int i = tid; i < H; i += nthr) q.hist_out[c * H + i] = ubuf[(Hpad - H) + T + i];      // the last H samples of [hist | u]
}

bool chunk_supported(int64_t C, int64_t T, int64_t K, int64_t Kf)
{
    // one workgroup per channel, everything in LDS; the FIR phase costs T * Kf / 1024 FMAs per thread
    return C >= 1 && T >= 1 && T <= 4096 && K >= 0 && K <= 64 && Kf >= 1 && Kf <= 4096 && T * Kf <= ((int64_t)1 << 22);
}

void chunk_forward(const float *x, int64_t x_pitch, float *y, int64_t C, int64_t T, const double *sos_host, int64_t K,
                   const double *sx_in, const double *sy_in, double *sx_out, double *sy_out,
                   const float *taps_host, int64_t Kf, const float *hist_in, float *hist_out,
                   double gain, int scale, int clamp, int precision, hipStream_t stream)
{
    TFX_CHECK(chunk_supported(C, T, K, Kf), "chunk_forward: unsupported geometry C=%lld T=%lld K=%lld taps=%lld "
              "(T <= 4096, K <= 64, T * taps <= 2^22)", (long long)C, (long long)T, (long long)K, (long long)Kf);
    TFX_CHECK(x && y && taps_host && (K == 0 || sos_host), "chunk_forward: null pointer");
    if (x_pitch <= 0) x_pitch = T;
    TFX_CHECK(x_pitch >= T, "chunk_forward: row pitch %lld smaller than the row length %lld", (long long)x_pitch, (long long)T);
    TFX_CHECK(x_pitch <= INT64_MAX / 8 / C, "chunk_forward: row pitch %lld overflows", (long long)x_pitch);
    check_stream_buffers("chunk_forward", 4, x, (C - 1) * x_pitch + T, y, C * T, hist_in, hist_out, C * (Kf - 1));
    ChunkParams q{};
    SosParams &p = q.sos;
    p.x = x; p.y = nullptr; p.taps = nullptr;
    p.sx_in = sx_in; p.sy_in = sy_in; p.sx_out = sx_out; p.sy_out = sy_out;
    p.C = C; p.C_in = C; p.T = T; p.K = (int)K; p.x_pitch = x_pitch;
    p.nseg = 1; p.warm = 0; p.seg_len = ceil_div(T, 1024) * 1024; p.nsum = 0;
    p.ep_stat = -1; p.nf_flag = nullptr;
    int prec = precision;
    std::shared_ptr<SosPlan> plan;                 // the plan and the taps are held until the launch is enqueued
    std::shared_ptr<DeviceBuffer> taps;
    if (K > 0) {
        check_sos("chunk_forward", sos_host, K, false);
        plan = get_plan(sos_host, K, stream, 1);
        SosPlan *pl = plan.get();
        if (prec == TFX_PREC_AUTO) prec = (plan_err_bound(pl) <= auto_bound()) ? TFX_PREC_F32 : TFX_PREC_F64;
        table_for(p, pl, prec == TFX_PREC_F32, chunk_kernel(false));     // (the table does not depend on VEC)
    }
    const int H = (int)Kf - 1, Hpad = (H + 3) & ~3, Kp = Hpad + 4;
    {   // device taps in the kernel's layout: Hpad - H leading zeros (they meet the zero-filled front of the LDS buffer),
        // the flipped taps, zeros up to Kp; cached by content like every other tap vector
        std::vector<float> lay((size_t)Kp, 0.0f);
        memcpy(lay.data() + (Hpad - H), taps_host, (size_t)Kf * 4);
        taps = cached_taps(lay.data(), (size_t)Kp * 4, (size_t)Kp * 4);
        q.taps = (const float *)taps->p;
    }
    q.hist_in = Kf > 1 ? hist_in : nullptr; q.hist_out = Kf > 1 ? hist_out : nullptr; q.y = y; q.Kf = (int)Kf;
    q.Tpad = (int)((T + 3) & ~3);
    q.gain = (float)gain; q.scale = scale; q.clamp = clamp;
    const bool vec = (((uintptr_t)x & 15) == 0) && (T % 4 == 0) && (x_pitch % 4 == 0);
    const bool f32 = prec == TFX_PREC_F32;
    constexpr int LC = chunk_kernel(false).LC;
    const size_t stage_b = K == 0 ? 0 : (size_t)(f32 ? sos_wave_lds_bytes<float, float, float, LC>(1, (int)K) : sos_wave_lds_bytes<float, float, double, LC>(1, (int)K));
    const size_t shmem = (size_t)(Hpad + q.Tpad + 8 + Kp) * 4 + stage_b;
    TFX_CHECK(shmem <= 64 * 1024, "chunk_forward: needs %zu B of LDS", shmem);
    // the cascade is one wavefront's work; the FIR phase scales with the threads: 4 outputs each
    const int threads = T * Kf <= (1 << 14) ? 256 : 1024;
    ProfScope ps("chunk_iir_fir_kernel", stream);
    if (f32) {
        if (vec) hipLaunchKernelGGL((chunk_iir_fir_kernel<float, true>), dim3((unsigned)C), dim3(threads), shmem, stream, q);
        else hipLaunchKernelGGL((chunk_iir_fir_kernel<float, false>), dim3((unsigned)C), dim3(threads), shmem, stream, q);
    } else {
        if (vec) hipLaunchKernelGGL((chunk_iir_fir_kernel<double, true>), dim3((unsigned)C), dim3(threads), shmem, stream, q);
        else hipLaunchKernelGGL((chunk_iir_fir_kernel<double, false>), dim3((unsigned)C), dim3(threads), shmem, stream, q);
    }
    TFX_HIP(hipGetLastError());
}

// olsnative.hip (cascade inside the forward column pass): the warm-up for max|A^W| < 2^-bits and the unit-b0 form of a
// cascade -- rows [G_s = b0_0 ... b0_s, b1 / b0, b2 / b0, -a1, -a2] (quotients in long double) -- or false when the cascade
// has no such form (unit_form_ok)
int64_t sos_warmup_bits(const double *sos_host, int64_t K, int bits)
{
    const std::vector<double> sos(sos_host, sos_host + 6 * K);
    return warmup_length(sos, (int)K, bits);
}
bool sos_unit_rows(const double *sos_host, int64_t K, double (*rows)[5])
{
    const std::vector<double> sos(sos_host, sos_host + 6 * K);
    if (!unit_form_ok(sos, (int)K)) return false;
    ld g = 1.0L;
    for (int64_t s = 0; s < K; ++s) {
        const ld b0 = sos[s * 6];
        g *= b0;
        rows[s][0] = (double)g;
        rows[s][1] = (double)((ld)sos[s * 6 + 1] / b0);
        rows[s][2] = (double)((ld)sos[s * 6 + 2] / b0);
        rows[s][3] = -sos[s * 6 + 4];
        rows[s][4] = -sos[s * 6 + 5];
    }
    return true;
}

void sos_plan_info(const double *sos_host, int64_t K, int *precision, int64_t *warmup, double *err_bound)
{
    const std::shared_ptr<SosPlan> plan = get_plan(sos_host, K, nullptr, 1);
    SosPlan *pl = plan.get();
    const double eb = plan_err_bound(pl);
    if (precision) *precision = (eb <= auto_bound()) ? TFX_PREC_F32 : TFX_PREC_F64;
    if (warmup) *warmup = pl->warm;
    if (err_bound) *err_bound = eb;
}

// The float64-arithmetic facts of a cascade: whether it runs the unit-b0 form on the shipping geometry, and the refinement
// rule (plan_refine) with what it was decided on, at the two tile sizes that matter: LC = 64 (float32 signals, aligned rows)
// and LC = 16 (float64 results: the other dtype mixes, banks, the sum mode).  errs = {blocked, seq} at LC = 64, then at LC = 16.
void sos_refine_info(const double *sos_host, int64_t K, int *unit_form, int *refine_f32, int *refine_f64, double *errs)
{
    const std::shared_ptr<SosPlan> plan = get_plan(sos_host, K, nullptr, 1);
    SosPlan *pl = plan.get();
    if (unit_form) *unit_form = plan_unit_ok(pl) ? 1 : 0;
    if (refine_f32) *refine_f32 = plan_refine(pl, 64, false) ? 1 : 0;
    if (refine_f64) *refine_f64 = plan_refine(pl, 16, true) ? 1 : 0;
    if (errs) {
        const BlockedError a = plan_blocked_error(pl, 64), b = plan_blocked_error(pl, 16);
        errs[0] = a.blocked; errs[1] = a.seq; errs[2] = b.blocked; errs[3] = b.seq;
    }
}

}  // namespace tfx
