// shape_sweep.cpp -- the largest error, in float32 ulps, of the waveshaper's float32 tanh and cubic (torchfx_amd/csrc/shape_fn.h)
// against the float64 math library, over every float32 in [-20, 20] or a sample of them.  Host only:
//   g++ -O2 -std=c++17 -ffp-contract=off -pthread tools/shape_sweep.cpp -o shape_sweep && ./shape_sweep [stride]
// stride 1 (the default) visits every float; a larger one visits every stride-th bit pattern plus 256 floats on each side of
// every breakpoint of the two functions (0, +-1, +-9, +-20).  One line per function:
//   <name> max_ulp=<e> at=<x> max_rel_u=<E> at=<x> n=<count>
// max_ulp counts spacings of float32 at the true value; max_rel_u is the error over u |true value| with u = 2^-24 (at most twice
// max_ulp; u |value| is floored at half the denormal spacing) -- the unit in which E_SHAPE enters the tests' error bound.
#include "../torchfx_amd/csrc/shape_fn.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

static float from_bits(uint32_t b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static uint32_t to_bits(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

// spacing of float32 at |r| (the denormal spacing below the smallest normal)
static double ulp_at(double r)
{
    r = std::fabs(r);
    if (r < 1.17549435e-38) return std::ldexp(1.0, -149);
    return std::ldexp(1.0, std::ilogb(r) - 23);
}

static double rel_unit(double r) { return std::max(std::ldexp(std::fabs(r), -24), std::ldexp(1.0, -150)); }

static double cubic_ref(double v) { return v >= 1 ? 1.0 : (v <= -1 ? -1.0 : 1.5 * v - 0.5 * v * v * v); }

struct Worst {
    double tanh_ulp = 0, cubic_ulp = 0, tanh_rel = 0, cubic_rel = 0;
    float tanh_at = 0, cubic_at = 0, tanh_rel_at = 0, cubic_rel_at = 0;
    uint64_t n = 0;
    void visit(float x)
    {
        const double rt = std::tanh((double)x), rc = cubic_ref((double)x);
        const double dt = std::fabs((double)shape_fn::tanh_f32(x) - rt), dc = std::fabs((double)shape_fn::cubic(x) - rc);
        const double et = dt / ulp_at(rt), ec = dc / ulp_at(rc), ft = dt / rel_unit(rt), fc = dc / rel_unit(rc);
        if (et > tanh_ulp) tanh_ulp = et, tanh_at = x;
        if (ec > cubic_ulp) cubic_ulp = ec, cubic_at = x;
        if (ft > tanh_rel) tanh_rel = ft, tanh_rel_at = x;
        if (fc > cubic_rel) cubic_rel = fc, cubic_rel_at = x;
        ++n;
    }
    void merge(const Worst &o)
    {
        if (o.tanh_ulp > tanh_ulp) tanh_ulp = o.tanh_ulp, tanh_at = o.tanh_at;
        if (o.cubic_ulp > cubic_ulp) cubic_ulp = o.cubic_ulp, cubic_at = o.cubic_at;
        if (o.tanh_rel > tanh_rel) tanh_rel = o.tanh_rel, tanh_rel_at = o.tanh_rel_at;
        if (o.cubic_rel > cubic_rel) cubic_rel = o.cubic_rel, cubic_rel_at = o.cubic_rel_at;
        n += o.n;
    }
};

int main(int argc, char **argv)
{
    const uint32_t stride = argc > 1 ? (uint32_t)std::max(1l, atol(argv[1])) : 1;
    const uint32_t top = to_bits(20.0f);                                 // positive floats are ordered like their bits
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<Worst> part(nt);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            const uint64_t steps = (uint64_t)top / stride + 1;
            for (uint64_t k = t; k < steps; k += nt) {
                const float x = from_bits((uint32_t)(k * stride));
                part[t].visit(x);
                part[t].visit(-x);
            }
        });
    for (auto &th : pool) th.join();
    Worst w;
    for (const Worst &p : part) w.merge(p);
    if (stride > 1)
        for (float b : {0.0f, 1.0f, 9.0f, 20.0f}) {
            const uint32_t c = to_bits(b);
            for (uint32_t k = c > 256 ? c - 256 : 0; k <= std::min(top, c + 256); ++k) {
                w.visit(from_bits(k));
                w.visit(-from_bits(k));
            }
        }
    printf("tanh max_ulp=%.4f at=%.9g max_rel_u=%.4f at=%.9g n=%llu\n", w.tanh_ulp, (double)w.tanh_at, w.tanh_rel, (double)w.tanh_rel_at,
           (unsigned long long)w.n);
    printf("cubic max_ulp=%.4f at=%.9g max_rel_u=%.4f at=%.9g n=%llu\n", w.cubic_ulp, (double)w.cubic_at, w.cubic_rel,
           (double)w.cubic_rel_at, (unsigned long long)w.n);
    return 0;
}
