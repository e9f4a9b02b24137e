// sos_route.h -- host-only: how a forward call of the SOS cascade cuts its rows into time segments.  The launch (sos.hip,
// launch_one) acts on sos_route(); tfx_sos_route_info reports it.  Nothing else decides a segmentation of the forward cascade
// (the zero-phase passes keep sos_halo_plan alone, the measuring pass its own block-aligned plan).
//
//   sequential  one stream per row.
//   halo        segments after the first start `warm` samples early from zero state (the plan of every cascade whose memory is
//               short against the row).
//   handoff     every segment starts at its own first sample from the exact state: end-state passes over the segments, a scan
//               of the end states over each row with the segment's transition matrix, then the ordinary kernel from those
//               states.  Works for any pole radius, costs 2 or 3 reads of the signal instead of 1.
#pragma once
#include <cstdint>

namespace tfx {

enum { SOS_ROUTE_SEQUENTIAL = 0, SOS_ROUTE_HALO = 1, SOS_ROUTE_HANDOFF = 2 };      // tfx_sos_route_info's *route codes

// Hand-off constants, from profiles/sos_hard_bench.txt (DESIGN.md 4.1.1 has the table):
// segments are multiples of the end-state kernel's tile and of the result kernel's;
constexpr int SOS_HANDOFF_QUANTUM = 2048;
// the shortest segment the automatic rule cuts (two tiles of the shipping kernel);
constexpr int64_t SOS_HANDOFF_MIN_SEG = 8192;
// an end-state pass over a segment, in units of the result pass over it: it reads the signal and stores nothing
// (0.218 / 0.279 ms on two sections, 0.296 / 0.318 on four, 0.143 / 0.266 on one);
constexpr double SOS_HANDOFF_END_COST = 0.78;
// a wavefront that has its SIMD to itself walks its samples in this share of the time it takes next to a second one: a plan
// that fills at most half of the wave slots runs that much faster per sample (halo plans of 4, 5 and 8 segments on 64 rows:
// 1.54, 2.06 and 1.70 ns per sample against 3.1, 3.5 and 3.1 of the same cascades with every slot taken);
constexpr double SOS_HANDOFF_LONE_WAVE = 0.55;
// one scan launch, in samples of a result pass (2.9 ns each): 3000 for the launch, and per level, 256-thread trip and row of
// P a unit that grows with the matrix (D = 10: 12 samples, D = 26: 56 -- the states of a long row no longer sit in the L1);
constexpr double SOS_HANDOFF_SCAN_LAUNCH = 3000.0;
inline double sos_handoff_scan_unit(int D) { const double u = (double)D * D / 12.0; return u > 12.0 ? u : 12.0; }
// and how much shorter than today's the modelled critical path must be (box noise is +-4 %, the model is good to 5 %).
constexpr double SOS_HANDOFF_MARGIN = 1.1;
constexpr int SOS_HANDOFF_MAXK = 32;             // sections: the scan multiplies (2K + 2)^2 matrices
constexpr double SOS_HANDOFF_PMAX = 1e100;       // largest entry of a transition matrix the route accepts

struct SosRouteQuery {
    int64_t C = 0, T = 0;            // rows, samples per row
    int64_t plan_warm = -1;          // the cascade's warm-up length, -1 = none (SosPlan::warm)
    int K = 1;                       // sections of the cascade
    int tile = 4096;                 // samples per tile of the kernel that stores the result
    int64_t wave_slots = 0;          // wavefronts of that kernel the device holds at once
    int64_t force_nseg = 0;          // TFX_SOS_NSEG, <= 0 = unset
    int handoff = -1;                // TFX_SOS_HANDOFF: -1 = unset (automatic), 0 = never, 1 = whenever the call is eligible
    bool eligible = false;           // the call can take the hand-off route (float64 arithmetic, one cascade, K and P in range)
    bool refine = false;             // ... and needs its refinement pass (plan_refine)
};

struct SosRoute {
    int route = SOS_ROUTE_SEQUENTIAL;
    int64_t nseg = 1, seg_len = 0, warm = 0;     // seg_len: distance between the starts of consecutive segments; warm: halo in force
    int passes = 1;                              // reads of the signal: 1, or 2 / 3 on the hand-off route
    bool floored = false;                        // halo plan: the 8 x warm floor cut nseg below its target
};

// The halo plan.  Streams are persistent (one wavefront walks its whole segment), so the launch should be exactly ONE resident
// round: nstreams <= wave_slots, otherwise the second round doubles the time.  Segments shorter than 8 x warm-up are not worth
// their halo.
inline SosRoute sos_halo_plan(int64_t C, int64_t T, int64_t plan_warm, int TILE, int64_t wave_slots, int64_t force_nseg)
{
    const auto cdiv = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    const int64_t tiles_total = cdiv(T, TILE);
    SosRoute r;
    int64_t nseg = 1, seg_len = tiles_total * TILE, warm = 0;
    if (plan_warm >= 0) {
        // halo rounded to 1 KB of float32: streams start on cache-line boundaries; 256 measured 1.5-4 % faster
        // than 32 on the float64 kernel (64 x 2.88 M / 10 M / 28.8 M), no difference beyond
        warm = (plan_warm + 255) & ~(int64_t)255;
        int64_t nseg_target = force_nseg > 0 ? force_nseg : wave_slots / (C > 0 ? C : 1);      // floor: one round
        if (nseg_target < 1) nseg_target = 1;
        if (nseg_target > 1 && T > warm) {
            // Every stream walks seg_tiles FULL tiles: stream g starts at g * stride, stride = seg_tiles * TILE - warm,
            // and its first `warm` samples (g > 0) are the halo -- the halo is absorbed into the tile grid instead of
            // costing every stream an extra, mostly discarded tile (+4 % at 64 x 2.88 M with 4096-sample tiles).
            int64_t seg_tiles = cdiv(cdiv(T - warm, nseg_target) + warm, TILE);
            if (force_nseg <= 0) {
                const int64_t min_tiles = cdiv(8 * warm, TILE);
                if (seg_tiles < min_tiles) { seg_tiles = min_tiles; r.floored = true; }
            }
            if (seg_tiles < 1) seg_tiles = 1;
            const int64_t stride = seg_tiles * TILE - warm;
            if (stride > 0) {
                nseg = cdiv(T - warm, stride);
                seg_len = stride;
            }
        }
        if (nseg <= 1) { nseg = 1; warm = 0; seg_len = tiles_total * TILE; }
    }
    r.route = nseg > 1 ? SOS_ROUTE_HALO : SOS_ROUTE_SEQUENTIAL;
    r.nseg = nseg; r.seg_len = seg_len; r.warm = warm;
    return r;
}

// The route of a call.  The halo plan is never displaced where it works: when it reaches its target without the 8 x warm
// floor, or TFX_SOS_NSEG is set alone, the answer is sos_halo_plan's, bit for bit.  Hand-off is a candidate when the cascade
// has no warm-up length, the row is not longer than it, or the floor cut the segment count; it is taken when its critical
// path -- the segment times the cost of its passes, plus its scans -- is shorter than the halo plan's (seg_tiles x TILE
// samples) by SOS_HANDOFF_MARGIN, each path weighted by how full its plan leaves the SIMDs.
inline SosRoute sos_route(const SosRouteQuery &q)
{
    const auto cdiv = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    const SosRoute today = sos_halo_plan(q.C, q.T, q.plan_warm, q.tile, q.wave_slots, q.force_nseg);
    if (!q.eligible || q.handoff == 0 || q.T <= 0) return today;
    const bool forced = q.handoff == 1;
    if (!forced && (q.force_nseg > 0 || !(q.plan_warm < 0 || q.T <= q.plan_warm || today.floored))) return today;
    const int64_t Q = q.tile > SOS_HANDOFF_QUANTUM ? q.tile : SOS_HANDOFF_QUANTUM;      // both are powers of two
    const int64_t quanta = cdiv(q.T, Q);
    int64_t target = q.force_nseg > 0 ? q.force_nseg : q.wave_slots / (q.C > 0 ? q.C : 1);
    if (target < 1) target = 1;
    int64_t seg_q = cdiv(quanta, target);
    if (q.force_nseg <= 0 && seg_q * Q < SOS_HANDOFF_MIN_SEG) seg_q = cdiv(SOS_HANDOFF_MIN_SEG, Q);
    SosRoute r;
    r.route = SOS_ROUTE_HANDOFF;
    r.seg_len = seg_q * Q;
    r.nseg = cdiv(quanta, seg_q);
    r.warm = 0;
    r.passes = q.refine ? 3 : 2;
    if (r.nseg < 2) return today;
    if (!forced) {
        const auto load = [&](int64_t nseg) { return 2 * q.C * nseg <= q.wave_slots ? SOS_HANDOFF_LONE_WAVE : 1.0; };
        const int D = 2 * q.K + 2;
        int nlev = 0;
        while (((int64_t)1 << nlev) < r.nseg - 1) ++nlev;
        const double scan = SOS_HANDOFF_SCAN_LAUNCH + (double)nlev * (double)cdiv((r.nseg - 1) * D, 256) * D * sos_handoff_scan_unit(D);
        const double ours = (double)r.seg_len * (1.0 + (r.passes - 1) * SOS_HANDOFF_END_COST) * load(r.nseg) + (r.passes - 1) * scan;
        const double theirs = (double)(today.seg_len + today.warm) * load(today.nseg);      // seg_tiles x TILE (one segment: the whole row)
        if (!(ours * SOS_HANDOFF_MARGIN < theirs)) return today;
    }
    return r;
}

}  // namespace tfx
