// Micro-benchmark: what scalar (not packed) float32 vector instructions sustain on gfx950, in plain C++ compiled with packed fp32
// instructions disabled -- the instruction mix of yin.hip's sweep.  Every lane runs 18 independent chains; a step is either one
// fused multiply-add per chain (FMA) or a subtraction and a fused multiply-add per chain (PAIR: d = a - w, acc = fma(d, d, acc)).
// Workgroups of 256 threads, 8 per CU (8 waves per SIMD).  Prints lane-instructions per second and, for 256 CUs x 4 SIMDs at
// 2.4 GHz, the clocks one wave-instruction takes on its SIMD.
//   hipcc --offload-arch=gfx950 -O3 -Xclang -target-feature -Xclang -packed-fp32-ops tools/ubench/valu_rate.hip -o valu_rate
#include <hip/hip_runtime.h>

#include <cstdio>

constexpr int CHAINS = 18, STEPS = 4096;

template <bool PAIR> __global__ __launch_bounds__(256) void valu_kernel(float *out, float a, float b)
{
    float acc[CHAINS], w[CHAINS];
#pragma unroll
    for (int i = 0; i < CHAINS; ++i) acc[i] = (float)threadIdx.x + i, w[i] = b * i;
    for (int s = 0; s < STEPS; ++s) {
#pragma unroll
        for (int i = 0; i < CHAINS; ++i) {
            if constexpr (PAIR) {
                const float d = a - w[i];
                acc[i] = fmaf(d, d, acc[i]);
                w[i] = acc[i];                                          // keeps the subtraction inside the loop
            } else {
                acc[i] = fmaf(acc[i], a, b);
            }
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CHAINS; ++i) sum += acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = sum;
}

template <bool PAIR> void run(const char *what, float *out, int blocks)
{
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    float best = 1e30f;
    for (int rep = 0; rep < 6; ++rep) {
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(valu_kernel<PAIR>, dim3(blocks), dim3(256), 0, 0, out, 0.999f, 1e-3f);
        (void)hipEventRecord(e1);
        (void)hipEventSynchronize(e1);
        float ms;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (rep && ms < best) best = ms;
    }
    const double lane_ops = (double)blocks * 256 * STEPS * CHAINS * (PAIR ? 2 : 1);
    const double rate = lane_ops / (best * 1e-3);
    printf("%-46s %8.3f ms  %.2fe12 lane-instructions/s  %.2f clocks per wave-instruction per SIMD at 2.4 GHz\n", what, best, rate * 1e-12,
           2.4e9 * 1024 * 64 / rate);
}

int main()
{
    const int blocks = 256 * 8 * 16;
    float *out;
    if (hipMalloc(&out, (size_t)blocks * 256 * sizeof(float)) != hipSuccess) return 1;
    run<false>("v_fma_f32, 18 independent chains", out, blocks);
    run<true>("v_sub_f32 + v_fma_f32, 18 chains", out, blocks);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
