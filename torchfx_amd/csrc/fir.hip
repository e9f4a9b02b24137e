// fir.hip -- direct-form causal depthwise FIR for gfx950.
//
// Replaces the conv_mode="direct" branch of FIR.forward (src/torchfx/filter/fir.py:556-568:
// F.pad(x,(K-1,0)) + F.conv1d(groups=C) with one shared flipped kernel):
//     y[c,n] = sum_{t<K} kf[t] * xp[c, n+t],   xp[m] = x[m-(K-1)]  (zero for m < K-1)
//
// float32: 2K flop/sample (2048 at K=1024) makes this FP32-rate bound, not HBM bound.  gfx950 has
// an exact-f32 matrix instruction, v_mfma_f32_32x32x2_f32 (on finite data bitwise an fmaf chain, same
// peak as the vector ALU but one instruction per 4096 flop), so the convolution is phrased as a
// Toeplitz product on the matrix pipe -- NOT to "reach MFMA" with reduced precision, the
// arithmetic is plain f32 FMA:
//     out(i,j) = y[nb + 32 i + j] = sum_s  A[i][s] * B[s][j]
//     A[i][s] = xw[32 i + s]          (signal window, LDS, rows padded 32->33 floats)
//     B[s][j] = kpad[s - j + 31]      (taps, Toeplitz, LDS, 31 zeros in front)
// Each wave owns NJ output tiles of 32x32 = 1024 consecutive samples and re-uses every B fragment
// across them; a workgroup (4 waves) covers 4 x NJ x 1024 outputs of one channel per pass and walks
// the taps in chunks of <= 1024 so the LDS window stays bounded for any K.
//
// Non-finite samples.  The Toeplitz array multiplies its zero padding (31 in front, 33 behind, K rounded up to
// the chunk) with real samples, and 0 * NaN = 0 * Inf = NaN: left alone, a bad sample at p would reach outputs
// before p and after p + K - 1, and an Inf inside its reach would come out as NaN.  But the padded sum touches a
// superset of the reference's samples and NaN / Inf never leave an accumulator, so a FINITE result has met no
// bad sample and stands; a thread forms each of its non-finite results again after the tap loop as a plain
// fmaf chain over the K real taps -- the terms of the reference, no others; zero-VALUED taps are multiplied
// like any other.  A bad sample at p reaches exactly y[p .. p + K - 1] of its row ("Non-finite
// samples in the direct FIR"; tests/test_gpu_fir_edges.py); finite data never takes the branch and keeps its bits.
//
// float64 signals (the reference computes conv1d in the input dtype) use a plain LDS-tiled
// vector kernel: rare path, correctness first.
#include "common.h"
#include "ols_route.h"
#include "plan_cache.h"
#include "timedomain.h"
#include "../../include/torchfx_hip.h"

#include <cstdlib>
#include <cstring>
#include <vector>

namespace tfx {

// device copies of tap vectors, keyed by content and padded size: uploaded (blocking) the first time a filter is seen, then
// reused -- no host sync on the steady-state path
static PlanCache<DeviceBuffer, 1> g_taps(128);
std::shared_ptr<DeviceBuffer> cached_taps(const void *host, size_t bytes, size_t padded)
{
    return g_taps.get(host, bytes, {(int64_t)padded}, nullptr, [&] {
        std::vector<char> h(padded, 0);
        memcpy(h.data(), host, bytes);
        return std::make_shared<DeviceBuffer>(h);
    });
}
void fir_clear() { g_taps.clear(); }

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int FIR_NJ = 1;                       // 32x32 tiles per wave
constexpr int FIR_NOUT = 4 * FIR_NJ * 1024;     // outputs per workgroup
constexpr int FIR_KC_MAX = 1024;                // largest tap chunk (taps are zero-padded to it)
constexpr int64_t FIR_MFMA_MIN_T = 4096;        // float32 rows shorter than this run the plain kernel

constexpr int FIR_CLASS_NONFINITE = 0x207;      // v_cmp_class mask: signalling NaN | quiet NaN | -Inf | +Inf

__device__ __forceinline__ int xpad33(int m) { return m + (m >> 5); }

// kf_dev: [Kpad] flipped taps on device, zero-padded to a multiple of FIR_KC_MAX
// FIR_KC: taps per chunk (128 / 512 / 1024 -- short filters do not pay for 1024-tap chunks).
// DBG (tools/ubench/fir_probe.hip only): bit 0 drops the output stores, bit 1 the global loads.
// NJ = 32x32 output tiles per wave; the library launches NJ = FIR_NJ = 1: 4096 outputs and a 26 KB window per workgroup,
// five per CU.  NJ = 4 (16384 outputs, 76 KB, two per CU; rounds 1-2) and NJ = 2 (8192 outputs, 43 KB, three per CU) were
// slower: with two workgroups per CU, both fill their window, multiply and store in lockstep, so the matrix pipe idles
// during every fill and store; more, smaller workgroups interleave those phases: cfg 3 2.86 / 2.77 / 2.73 ms for
// NJ = 4 / 2 / 1 on one box (profiles/r03_fir.txt; NJ = 1 at six waves per SIMD spills 36 B and is back to 2.78).
template <int FIR_KC, int DBG = 0, int NJ = FIR_NJ>
__global__ void __launch_bounds__(256, NJ == 4 ? 2 : (NJ == 2 ? 3 : 5))
fir_direct_mfma_kernel(const float *__restrict__ x, float *__restrict__ y,
                       const float *__restrict__ kf_dev, int64_t C, int64_t T, int K, int nchunks,
                       int64_t tiles_per_row, const float *__restrict__ hist, int H)
{
    // hist (streaming, StatefulFIR): [C, H] samples that precede the row, x[-H .. -1]; null = zeros
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int WOUT = NJ * 1024, NOUT = 4 * WOUT;
    constexpr int XW = NOUT + FIR_KC + 32;              // window length (floats)
    constexpr int XW_PAD = XW + (XW >> 5) + 1;
    float *xw = (float *)smem;                              // [XW_PAD]
    float *kp = xw + ((XW_PAD + 3) & ~3);                   // [31 + FIR_KC + 33]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Tile -> workgroup: workgroups are dealt to the eight XCDs round robin (observed; only speed and traffic depend on it), so
    // XCD b % 8 takes the tiles [xcd * per_xcd, (xcd + 1) * per_xcd) in order: neighbouring tiles of a row, whose windows share
    // K - 1 + 32 samples, are worked on by ONE XCD and the overlap is an L2 hit instead of a second fetch (round 4: PMC read
    // traffic of cfg 3 1.2 x -> see profiles/r04_traffic.json).
    const int64_t ntiles = C * tiles_per_row, per_xcd = (ntiles + 7) / 8;
    const int64_t bid = (int64_t)(blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if ((int64_t)(blockIdx.x >> 3) >= per_xcd || bid >= ntiles) return;
    // (64-bit divisions run on the vector unit: the wave-uniform quotient goes back to scalar registers, or row bases and tile
    // offsets sit in VGPR pairs for the whole tile -- the kernel spilled one register at its 96-VGPR budget: 46 MB of scratch
    // writes per cfg-3 call in the PMC write traffic)
    const auto uni64 = [](int64_t v) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uint64_t)v);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((uint64_t)v >> 32));
        return (int64_t)(((uint64_t)hi << 32) | lo);
    };
    const int64_t c = uni64(bid / tiles_per_row);
    const int64_t n0 = (bid - c * tiles_per_row) * (int64_t)NOUT;
    const float *xrow = x + c * T;
    float *yrow = y + c * T;

    floatx16 acc[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int li = lane & 31, kk = lane >> 5;

    // Per-lane LDS bases.  With s = 32*blk + 2*q + kk the padded window index of A[i=li][s] for
    // tile t is  (xb + xb/32 + 33*li + kk) + 1056*t + 33*blk + 2*q  and the Toeplitz tap index is
    // (31 - li + kk) + 32*blk + 2*q : everything but `blk` is an immediate ds_read offset.
    const int xb = wave * WOUT;
    const float *pa0 = xw + xb + (xb >> 5) + 33 * li + kk;
    const float *pb0 = kp + 31 - li + kk;
    constexpr int XV = (XW + 255) / 256;                    // window loads per thread
    constexpr int KV = (31 + FIR_KC + 33 + 255) / 256;      // tap loads per thread

    for (int ch = 0; ch < nchunks; ++ch) {
        const int t0 = ch * FIR_KC;
        // window: xw[m] = xp[n0 + t0 + m] = x[n0 + t0 + m - (K-1)].  All loads are issued before
        // the first LDS write (branch-free: clamped address + select), so the fill costs one
        // memory latency instead of XV of them.
        const int64_t base = n0 + t0 - (int64_t)(K - 1);
        float xv[XV], kv[KV];
        // Buffer descriptor over the part of the window that lies inside the row: reads past
        // its end return 0 in hardware; elements before the row start are clamped to offset 0
        // here and zeroed at the LDS write.  32-bit offsets, no per-load address pairs.
        const int64_t gstart = base < 0 ? 0 : (base > T ? T : base);
        const int64_t gend0 = base + (int64_t)XV * 256;
        const int64_t gend = gend0 < gstart ? gstart : (gend0 > T ? T : gend0);
        const int shift = (int)(base - gstart);             // <= 0; 0 for every interior tile
        // (the 64-bit divide that produced `c` ran on the vector ALU: tell the compiler the
        // descriptor words are wave-uniform, or every load becomes a waterfall loop)
        const uint64_t pw = (uint64_t)(xrow + gstart);
        const uint64_t pu = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(pw >> 32)) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)pw);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)pu, 0, __builtin_amdgcn_readfirstlane((int)((gend - gstart) * 4)), 0x00020000);
        // Interior tiles (window entirely inside the row: all but the first and last tile or two of a row): ONE
        // per-lane offset and a scalar offset per load -- no 68 address registers (the per-load clamped offsets of
        // the general form made this kernel spill 292 VGPRs = 4.6 x the output bytes of scratch traffic).  The scalar
        // offset is not part of the hardware range check, so tiles that touch either end of the row take the
        // partially unrolled loop below, where the range check and the clamp do their work.
        const bool interior = (shift == 0) && (gend0 <= T);  // workgroup-uniform
        if (interior) {
#pragma unroll
            for (int r = 0; r < XV; ++r)
                xv[r] = (DBG & 2) ? 1.0f : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, tid * 4, r * 1024, 0));
        }
#pragma unroll
        for (int r = 0; r < KV; ++r) {
            const int v = tid + 256 * r - 31;               // kf_dev is zero-padded to a multiple of KC
            const int vc = v < 0 ? 0 : (v >= FIR_KC ? FIR_KC - 1 : v);
            kv[r] = kf_dev[t0 + vc];
        }
        __builtin_amdgcn_sched_barrier(0);   // keep every load above, every use below
        __syncthreads();    // previous chunk's readers are done
        if (interior) {
#pragma unroll
            for (int r = 0; r < XV; ++r) {
                const int m = tid + 256 * r;
                if (m < XW) xw[xpad33(m)] = xv[r];
            }
        } else {
#pragma unroll 2
            for (int r = 0; r < XV; ++r) {
                const int m = tid + 256 * r;
                const int e = shift + m;
                float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (e < 0 ? 0 : e) * 4, 0, 0));
                if (e < 0) {                                 // before the row start (first tiles only)
                    const int64_t g = base + m;              // < 0
                    v = (hist && g >= -(int64_t)H) ? hist[c * H + H + g] : 0.0f;
                }
                if (m < XW) xw[xpad33(m)] = v;
            }
        }
#pragma unroll
        for (int r = 0; r < KV; ++r) {
            const int u = tid + 256 * r;
            if (u < 31 + FIR_KC + 33) kp[u] = (u >= 31 && u < 31 + FIR_KC) ? kv[r] : 0.0f;
        }
        __syncthreads();

        // contraction over s in [0, KC+32) in blocks of 32 (16 k-steps of 2)
        for (int blk = 0; blk < (FIR_KC + 32) / 32; ++blk) {
            const float *pa = pa0 + 33 * blk;
            const float *pb = pb0 + 32 * blk;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float b = pb[2 * q];
#pragma unroll
                for (int t = 0; t < NJ; ++t) {
                    const float a = pa[1056 * t + 2 * q];
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
                }
            }
        }
    }

    // D layout: lane holds column j = lane&31, rows i = 8*(r/4) + 4*(lane>>5) + (r&3).  The lane id is taken afresh (mbcnt):
    // keeping `li` / `kk` alive through the contraction cost the 96-VGPR kernel its one spilled register.
    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int li_e = lane_e & 31, kk_e = lane_e >> 5;
    static_assert(NJ * 16 <= 32, "one bit of `redo` per accumulator");
    unsigned redo = 0;                                      // accumulators that came out NaN / Inf
#pragma unroll
    for (int t = 0; t < NJ; ++t) {
        const int64_t nb = n0 + wave * WOUT + t * 1024;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 8 * (r >> 2) + 4 * kk_e + (r & 3);
            const int64_t n = nb + 32 * i + li_e;
            if ((DBG & 1) ? (acc[t][r] == 1234.5f) : (n < T)) yrow[n] = acc[t][r];
            redo |= (unsigned)__builtin_amdgcn_classf(acc[t][r], FIR_CLASS_NONFINITE) << (16 * t + r);
        }
    }
    // rare: non-finite results (see the header).  Each again from the definition: the K real taps in tap order, the sum
    // fir_direct_simple_kernel forms, samples straight from memory.  Here, after the stores, the accumulators are dead: the
    // branch costs the steady-state kernel no register (inside the tap loop it cost 13 and a wave of occupancy).
    if (DBG == 0 && redo) {
        const int nl0 = wave * WOUT + 128 * kk_e + li_e;
#pragma unroll 1
        for (int q = 0; q < NJ * 16; ++q) {
            const int64_t n = n0 + nl0 + (q >> 4) * 1024 + 32 * (8 * ((q & 15) >> 2) + (q & 3));
            if (!((redo >> q) & 1u) || n >= T) continue;
            float a = 0.0f;
#pragma unroll 1
            for (int u = 0; u < K; ++u) {
                const int64_t g = n + u - (int64_t)(K - 1);          // <= n < T
                const float v = g >= 0 ? xrow[g] : ((hist && g >= -(int64_t)H) ? hist[c * H + H + g] : 0.0f);
                a = fmaf(kf_dev[u], v, a);
            }
            yrow[n] = a;
        }
    }
}

// generic (float64, or any dtype) LDS-tiled vector kernel: 256 threads x 4 outputs
template <typename T>
__global__ void __launch_bounds__(256)
fir_direct_simple_kernel(const T *__restrict__ x, T *__restrict__ y, const T *__restrict__ kf_dev,
                         int64_t C, int64_t Tn, int K, int64_t tiles_per_row, const T *__restrict__ hist, int H)
{
    constexpr int NO = 1024, KC = 512;
    __shared__ T xw[NO + KC];
    __shared__ T kp[KC];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x / tiles_per_row;
    const int64_t n0 = (blockIdx.x % tiles_per_row) * (int64_t)NO;
    const T *xrow = x + c * Tn;
    T acc[4] = {0, 0, 0, 0};
    for (int t0 = 0; t0 < K; t0 += KC) {
        __syncthreads();
        const int64_t base = n0 + t0 - (int64_t)(K - 1);
        for (int m = tid; m < NO + KC; m += 256) {
            const int64_t g = base + m;
            xw[m] = (g >= 0 && g < Tn) ? xrow[g] : ((hist && g < 0 && g >= -(int64_t)H) ? hist[c * H + H + g] : (T)0);
        }
        for (int u = tid; u < KC; u += 256) kp[u] = (t0 + u < K) ? kf_dev[t0 + u] : (T)0;
        __syncthreads();
        const int kc = (K - t0 < KC) ? (K - t0) : KC;
        for (int u = 0; u < kc; ++u) {
            const T k = kp[u];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = fma(k, xw[tid + 256 * r + u], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t n = n0 + tid + 256 * r;
        if (n < Tn) y[c * Tn + n] = acc[r];
    }
}

// The last H samples of the logical signal [hist | x] (what the next chunk needs as its history).
template <typename T>
__global__ void __launch_bounds__(256)
fir_hist_update_kernel(const T *__restrict__ x, const T *__restrict__ hist_in, T *__restrict__ hist_out,
                       int64_t C, int64_t Tn, int64_t H)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= C * H) return;
    const int64_t c = g / H;
    hist_out[g] = stream_hist_at(x + c * Tn, hist_in ? hist_in + c * H : nullptr, Tn, H, g - c * H);
}

void fir_hist_update(const void *x, const void *hist_in, void *hist_out, int dtype, int64_t C, int64_t T, int64_t H,
                     hipStream_t stream)
{
    if (C * H == 0) return;
    const unsigned grid = (unsigned)ceil_div(C * H, 256);
    if (dtype == TFX_F32)
        hipLaunchKernelGGL(fir_hist_update_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float *)x,
                           (const float *)hist_in, (float *)hist_out, C, T, H);
    else
        hipLaunchKernelGGL(fir_hist_update_kernel<double>, dim3(grid), dim3(256), 0, stream, (const double *)x,
                           (const double *)hist_in, (double *)hist_out, C, T, H);
    TFX_HIP(hipGetLastError());
}

void fir_direct_forward(const void *x, void *y, int dtype, int64_t C, int64_t T,
                        const void *kernel_host, int64_t K, hipStream_t stream, const void *hist, int64_t H)
{
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "fir_direct_forward: bad dtype %d", dtype);
    TFX_CHECK(K >= 1, "fir_direct_forward: empty kernel");
    TFX_CHECK(K < (1 << 30), "fir_direct_forward: kernel too long");
    TFX_CHECK(H >= 0 && H < (1 << 30) && (H == 0 || hist), "fir_direct_forward: bad history");
    if (C == 0 || T == 0) return;
    TFX_CHECK(x && y && kernel_host, "fir_direct_forward: null pointer");
    TFX_CHECK(C > 0 && T > 0, "fir_direct_forward: negative size");
    const size_t esz = dtype == TFX_F32 ? 4 : 8;
    const int64_t Kpad = ceil_div(K, FIR_KC_MAX) * FIR_KC_MAX;
    const std::shared_ptr<DeviceBuffer> taps = cached_taps(kernel_host, (size_t)K * esz, (size_t)Kpad * esz);   // held until launched
    const void *kdev = taps->p;
    // rows shorter than FIR_MFMA_MIN_T (streaming chunks; measured when an MFMA tile was 16384 samples, NJ = 4): the plain
    // LDS-tiled kernel has 1024-sample tiles and finishes in a few microseconds instead of a full tile's ~60
    // ... and so does any job whose 1024-sample tiles are all resident at once (8 workgroups per CU): one round of
    // the plain kernel costs ~40 clocks per tap, one NJ = 4 MFMA workgroup walked its 16384-sample tile for ~128 clocks per
    // tap -- the MFMA kernel wins on throughput (2.5 x), not on latency (streaming chunks, 64 x 4096 and the like)
    const bool few_tiles = C * ceil_div(T, (int64_t)1024) <= env_i64("TFX_FIR_ONE_ROUND_TILES", 2048);   // 0: MFMA whenever T allows (tests)
    const bool short_rows = dtype == TFX_F32 && (T < env_i64("TFX_FIR_MFMA_MIN_T", FIR_MFMA_MIN_T) || few_tiles);
    if (dtype == TFX_F32 && !short_rows) {
        const int64_t tiles = ceil_div(T, FIR_NOUT);
        TFX_CHECK(C * tiles < (1ll << 31), "fir_direct_forward: grid too large");
        // chunk size: cost per chunk ~ (KC+32)/32 contraction blocks + ~4 blocks' worth of refill
        int kc = 1024;
        int64_t best = -1;
        for (int cand : {128, 512, 1024}) {
            const int64_t cost = ceil_div(K, cand) * ((cand + 32) / 32 + 4);
            if (best < 0 || cost < best) best = cost, kc = cand;
        }
        {
            const int v = (int)env_i64("TFX_FIR_KC", 0);
            if (v == 128 || v == 512 || v == 1024) kc = v;
        }
        const int nchunks = (int)ceil_div(K, kc);
        auto launch = [&](auto kern, int KC) {
            const int XW = FIR_NOUT + KC + 32;
            const int XW_PAD = XW + (XW >> 5) + 1;
            const size_t shmem = (((XW_PAD + 3) & ~3) + 31 + KC + 33) * sizeof(float);
            static bool attr_done[TFX_MAX_DEVICES][3] = {};
            bool &done = attr_done[current_device()][KC == 128 ? 0 : (KC == 512 ? 1 : 2)];
            if (!done) {
                TFX_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
                done = true;
            }
            ProfScope ps("fir_direct_mfma_kernel", stream);
            hipLaunchKernelGGL(kern, dim3((unsigned)(ceil_div(C * tiles, 8) * 8)), dim3(256), shmem, stream, (const float *)x,
                               (float *)y, (const float *)kdev, C, T, (int)K, nchunks, tiles, (const float *)hist, (int)H);
            TFX_HIP(hipGetLastError());
        };
        if (kc == 128) launch(fir_direct_mfma_kernel<128>, 128);
        else if (kc == 512) launch(fir_direct_mfma_kernel<512>, 512);
        else launch(fir_direct_mfma_kernel<1024>, 1024);
    } else {
        const int64_t tiles = ceil_div(T, 1024);
        TFX_CHECK(C * tiles < (1ll << 31), "fir_direct_forward: grid too large");
        if (dtype == TFX_F32) {
            ProfScope ps("fir_direct_simple_kernel<f32>", stream);
            hipLaunchKernelGGL(fir_direct_simple_kernel<float>, dim3((unsigned)(C * tiles)), dim3(256), 0, stream,
                               (const float *)x, (float *)y, (const float *)kdev, C, T, (int)K, tiles, (const float *)hist, (int)H);
        } else {
            ProfScope ps("fir_direct_simple_kernel<f64>", stream);
            hipLaunchKernelGGL(fir_direct_simple_kernel<double>, dim3((unsigned)(C * tiles)), dim3(256), 0, stream,
                               (const double *)x, (double *)y, (const double *)kdev, C, T, (int)K, tiles, (const double *)hist, (int)H);
        }
        TFX_HIP(hipGetLastError());
    }
}

// one chunk of a stateful FIR: history and chunk are read from their two buffers (direct form here, overlap-save through
// ols_route.h), then the new history is written
void fir_stream_forward(const void *x, void *y, int dtype, int64_t C, int64_t T, const void *kernel_host, int64_t K, int direct,
                        const void *hist_in, void *hist_out, hipStream_t stream)
{
    TFX_CHECK(K >= 1, "fir_stream_forward: empty kernel");
    TFX_CHECK(dtype == TFX_F32 || dtype == TFX_F64, "fir_stream_forward: bad dtype %d", dtype);
    TFX_CHECK(C >= 0 && T >= 0 && (C == 0 || (T <= INT64_MAX / 16 / C && K <= INT64_MAX / 16 / C)),
              "fir_stream_forward: negative size or size overflows");
    TFX_CHECK(C == 0 || T == 0 || x, "fir_stream_forward: null signal");
    const int64_t H = K - 1;
    check_stream_buffers("fir_stream_forward", dtype == TFX_F32 ? 4 : 8, x, C * T, y, C * T, hist_in, hist_out, C * H);
    if (C > 0 && T > 0) {
        if (direct) fir_direct_forward(x, y, dtype, C, T, kernel_host, K, stream, H ? hist_in : nullptr, hist_in ? H : 0);
        else fft_conv_forward(x, y, dtype, C, T, kernel_host, K, H, 0, stream, H ? hist_in : nullptr, hist_in ? H : 0);
    }
    if (hist_out && C > 0) fir_hist_update(x, hist_in, hist_out, dtype, C, T, H, stream);
}

}  // namespace tfx
