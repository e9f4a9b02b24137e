// torchfx_ext -- the compiled boundary module of the HIP backend.
//
// The reference binds its native kernels through a pybind11 torch extension named `torchfx_ext`
// (src/torchfx/_csrc/binding.cpp:83-96, imported as `from torchfx import torchfx_ext`).  This file is
// that module for MI355X: the same three entry points with the same signatures on at::Tensor
// (biquad_forward, sos_forward, delay_line_forward), launched on PyTorch's current HIP stream, plus a
// TORCH_LIBRARY(torchfx_hip) registration of every op of the backend so that Python reaches the kernels
// through the dispatcher (torch.ops.torchfx_hip.*) -- no ctypes on the tensor path.  It is a thin,
// host-only translation unit (compiled with g++): tensors are checked, outputs allocated, and the
// extern "C" ABI of libtorchfx_hip.so (include/torchfx_hip.h) is called -- the C ABI stays the one
// boundary non-torch hosts and this module share.
//
// Host tensors: the reference's module dispatches on x.is_cuda() (binding.cpp:30-81), so the three pybind entry points
// at the bottom do too -- their host branch is host_branch.h (this module's own Direct Form I loop).  Everything else is
// device-only: the dispatcher ops are registered for the CUDA key (= ROCm device tensors in a ROCm build of PyTorch) and
// for Meta (shape inference), and a CPU tensor gets an explicit error there.
#include <torch/extension.h>
#include <torch/library.h>

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <cstdlib>
#include <exception>
#include <optional>
#include <string>
#include <tuple>
#include <vector>

#include "../../../include/torchfx_hip.h"
#include "host_branch.h"

namespace {

using at::Tensor;
using OptTensor = std::optional<Tensor>;

// ---- workspaces through PyTorch's caching allocator (tfx_set_workspace_allocator, include/torchfx_hip.h) -------------------------
// The overlap-save pipelines keep multi-GB workspaces between calls.  Allocated here they show up in torch.cuda.memory_allocated(),
// an allocation under memory pressure first frees torch's cached blocks and retries, and when it still fails the library asks
// for a smaller slab; only if even 8 frame pairs do not fit does the op fail -- with torch's own OutOfMemoryError (kept in
// `pending_oom` by the hook, rethrown by check_rc), not a raw hipErrorOutOfMemory.  TORCHFX_AMD_WORKSPACE=hip keeps hipMalloc.
thread_local std::exception_ptr pending_oom;

void *torch_ws_alloc(size_t bytes, int device, void *stream, void *)
{
    try {
        c10::hip::HIPGuard guard((c10::DeviceIndex)device);
        return c10::hip::HIPCachingAllocator::raw_alloc_with_stream(bytes, (hipStream_t)stream);
    } catch (...) {
        pending_oom = std::current_exception();
        return nullptr;
    }
}

void torch_ws_free(void *ptr, int device, void *)
{
    try {
        c10::hip::HIPGuard guard((c10::DeviceIndex)device);
        c10::hip::HIPCachingAllocator::raw_delete(ptr);
    } catch (...) {            // interpreter shutdown: the allocator may be gone
    }
}

struct WorkspaceHook {
    WorkspaceHook()
    {
        const char *e = std::getenv("TORCHFX_AMD_WORKSPACE");
        if (!(e && std::string(e) == "hip")) tfx_set_workspace_allocator(torch_ws_alloc, torch_ws_free, nullptr);
    }
} workspace_hook;

void check_rc(int rc, const char *what)
{
    std::exception_ptr oom;
    std::swap(oom, pending_oom);           // an allocation that failed on the way to a smaller slab is not an error of a call that succeeded
    if (rc != 0 && oom) std::rethrow_exception(oom);
    TORCH_CHECK(rc == 0, what, ": ", tfx_last_error());
}

int dtype_code(const Tensor &t, const char *what)
{
    if (t.scalar_type() == at::kFloat) return TFX_F32;
    if (t.scalar_type() == at::kDouble) return TFX_F64;
    TORCH_CHECK(false, what, ": expected a float32 or float64 tensor, got ", t.scalar_type());
}

void need_device(const Tensor &t, const char *what)
{
    TORCH_CHECK(t.is_cuda(), "torchfx_amd: ", what, " must live on a ROCm device (got ", t.device(),
                "); this backend has no CPU path -- move the tensor with .to('cuda').");
}

tfx_stream_t stream_of(const Tensor &t)
{
    return (tfx_stream_t)c10::hip::getCurrentHIPStream(t.get_device()).stream();
}

// small coefficient tensor -> contiguous host float64 (O(K) bytes; the C ABI takes coefficients on the host)
Tensor host_f64(const Tensor &t, int64_t last, const char *what)
{
    Tensor h = t.detach().to(at::kCPU, at::kDouble).contiguous();
    TORCH_CHECK(h.dim() >= 1 && h.size(-1) == last, what, ": expected last dimension ", last, ", got shape ", h.sizes());
    return h;
}

const double *state_ptr(const OptTensor &s, at::IntArrayRef shape, const Tensor &x, const char *what, Tensor &keep)
{
    if (!s.has_value() || !s->defined()) return nullptr;
    TORCH_CHECK(s->sizes() == shape, what, " must have shape ", shape, ", got ", s->sizes());
    keep = s->to(x.device(), at::kDouble).contiguous();
    return keep.data_ptr<double>();
}

// a filter or window handed over as it is: a 1-D host tensor in x's dtype, non-empty (or of exactly `numel` values), made contiguous
Tensor host_vector(const Tensor &t, const Tensor &x, const char *what, const char *name, int64_t numel = -1)
{
    if (numel < 0) {
        TORCH_CHECK(!t.is_cuda() && t.dim() == 1 && t.numel() >= 1, what, ": ", name, " must be a non-empty 1-D host tensor");
    } else {
        TORCH_CHECK(!t.is_cuda() && t.dim() == 1 && t.numel() == numel, what, ": ", name, " must be a 1-D host tensor of ", numel, " values");
    }
    TORCH_CHECK(t.scalar_type() == x.scalar_type(), what, ": ", name, " must have x's dtype (", x.scalar_type(), "), got ",
                t.scalar_type());
    return t.contiguous();
}

int precision_or_default(int64_t precision)
{
    if (precision >= 0) return (int)precision;
    const char *e = getenv("TORCHFX_AMD_IIR_PRECISION");
    if (!e || !*e) return TFX_PREC_F64;
    const std::string s(e);
    if (s == "f64" || s == "float64") return TFX_PREC_F64;
    if (s == "f32" || s == "float32") return TFX_PREC_F32;
    if (s == "auto") return TFX_PREC_AUTO;
    TORCH_CHECK(false, "TORCHFX_AMD_IIR_PRECISION=", s, ": expected f64, f32 or auto");
}

at::ScalarType out_type(const Tensor &x, const std::optional<at::ScalarType> &out_dtype)
{
    return out_dtype.has_value() ? *out_dtype : x.scalar_type();
}

// ---------------------------------------------------------------------------------------------------
// SOS cascade (binding.cpp:52-66) and its filter-bank / sum forms
// ---------------------------------------------------------------------------------------------------
// the epilogue arguments of the *_ep ops; absent = the plain op and its C entry
struct EpilogueArgs {
    double gain;
    bool clamp;
    int64_t stat_mode;
    bool per_row;
};

// cascade + epilogue (Gain / clamp / statistic for Normalize applied by the producing kernel, include/torchfx_hip.h)
tfx_epilogue make_epilogue(const EpilogueArgs &a, Tensor &stat, const Tensor &like, int64_t rows)
{
    TORCH_CHECK(a.stat_mode >= -1 && a.stat_mode <= 1, "epilogue: stat_mode must be -1 (none), 0 (max|y|) or 1 (sum y^2)");
    stat = at::empty({a.stat_mode >= 0 ? (a.per_row ? rows : 1) : 0}, like.options().dtype(at::kDouble));
    tfx_epilogue ep;
    ep.gain = a.gain; ep.clamp = a.clamp ? 1 : 0; ep.stat_mode = (int)a.stat_mode; ep.stat_per_row = a.per_row ? 1 : 0;
    ep.stat_out = a.stat_mode >= 0 ? stat.data_ptr<double>() : nullptr;
    return ep;
}

// sos_forward / sos_forward_sections (tfx_sos_forward) and, with `epa`, sos_forward_ep (tfx_sos_forward_ep): the fourth tensor is
// every section's output (empty without `sections`) or the epilogue's statistic
std::tuple<Tensor, Tensor, Tensor, Tensor> sos_impl(const Tensor &x_in, const Tensor &sos_cpu, const OptTensor &state_x,
                                                    const OptTensor &state_y, std::optional<at::ScalarType> out_dtype,
                                                    int64_t precision, bool sections, const EpilogueArgs *epa = nullptr)
{
    const char *what = epa ? "sos_forward_ep" : "sos_forward";
    TORCH_CHECK(x_in.dim() == 2, what, ": x must be [C, T], got ", x_in.sizes());
    need_device(x_in, "x");
    const Tensor x = x_in.contiguous();
    const Tensor sos = host_f64(sos_cpu, 6, what);
    TORCH_CHECK(sos.dim() == 2, what, ": sos must be [K, 6]");
    const int64_t C = x.size(0), T = x.size(1), K = sos.size(0);
    Tensor kx, ky, fourth;
    const double *sx = state_ptr(state_x, {K, C, 2}, x, "state_x", kx);
    const double *sy = state_ptr(state_y, {K, C, 2}, x, "state_y", ky);
    const auto odt = out_type(x, out_dtype);
    Tensor y = at::empty({C, T}, x.options().dtype(odt));
    Tensor nsx = at::empty({K, C, 2}, x.options().dtype(at::kDouble));
    Tensor nsy = at::empty({K, C, 2}, x.options().dtype(at::kDouble));
    tfx_epilogue ep{};
    if (epa) ep = make_epilogue(*epa, fourth, x, C);
    else fourth = sections ? at::empty({K, C, T}, x.options().dtype(odt)) : at::empty({0}, x.options().dtype(odt));
    const int xdt = dtype_code(x, what), ydt = dtype_code(y, what), prec = precision_or_default(precision);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(epa ? tfx_sos_forward_ep(x.data_ptr(), xdt, y.data_ptr(), ydt, C, T, sos.data_ptr<double>(), K, sx, sy, nsx.data_ptr<double>(),
                                      nsy.data_ptr<double>(), prec, &ep, stream_of(x))
                 : tfx_sos_forward(x.data_ptr(), xdt, y.data_ptr(), ydt, C, T, sos.data_ptr<double>(), K, sx, sy, nsx.data_ptr<double>(),
                                   nsy.data_ptr<double>(), sections ? fourth.data_ptr() : nullptr, prec, stream_of(x)),
             what);
    return {y, nsx, nsy, fourth};
}

std::tuple<Tensor, Tensor, Tensor> sos_op(const Tensor &x, const Tensor &sos_cpu, const OptTensor &sx, const OptTensor &sy,
                                          std::optional<at::ScalarType> out_dtype, int64_t precision)
{
    auto r = sos_impl(x, sos_cpu, sx, sy, out_dtype, precision, false);
    return {std::get<0>(r), std::get<1>(r), std::get<2>(r)};
}

std::tuple<Tensor, Tensor, Tensor, Tensor> sos_sections_op(const Tensor &x, const Tensor &sos_cpu, const OptTensor &sx,
                                                           const OptTensor &sy, std::optional<at::ScalarType> out_dtype,
                                                           int64_t precision)
{
    return sos_impl(x, sos_cpu, sx, sy, out_dtype, precision, true);
}

std::tuple<Tensor, Tensor, Tensor, Tensor> sos_ep_op(const Tensor &x, const Tensor &sos_cpu, const OptTensor &sx, const OptTensor &sy,
                                                     double gain, bool clamp, int64_t stat_mode, bool per_row,
                                                     std::optional<at::ScalarType> out_dtype, int64_t precision)
{
    const EpilogueArgs epa{gain, clamp, stat_mode, per_row};
    return sos_impl(x, sos_cpu, sx, sy, out_dtype, precision, false, &epa);
}

std::tuple<Tensor, Tensor, Tensor> bank_impl(const Tensor &x_in, const Tensor &banks_cpu, const OptTensor &state_x,
                                             const OptTensor &state_y, std::optional<at::ScalarType> out_dtype,
                                             int64_t precision, bool sum)
{
    const char *what = sum ? "sos_bank_sum_forward" : "sos_bank_forward";
    TORCH_CHECK(x_in.dim() == 2, what, ": x must be [C, T], got ", x_in.sizes());
    need_device(x_in, "x");
    const Tensor x = x_in.contiguous();
    const Tensor banks = host_f64(banks_cpu, 6, what);
    TORCH_CHECK(banks.dim() == 3, what, ": sos_banks must be [NB, K, 6]");
    const int64_t C = x.size(0), T = x.size(1), NB = banks.size(0), K = banks.size(1);
    Tensor kx, ky;
    const double *sx = state_ptr(state_x, {K, NB * C, 2}, x, "state_x", kx);
    const double *sy = state_ptr(state_y, {K, NB * C, 2}, x, "state_y", ky);
    const auto odt = sum ? x.scalar_type() : out_type(x, out_dtype);
    Tensor y = sum ? at::empty({C, T}, x.options()) : at::empty({NB, C, T}, x.options().dtype(odt));
    Tensor nsx = at::empty({K, NB * C, 2}, x.options().dtype(at::kDouble));
    Tensor nsy = at::empty({K, NB * C, 2}, x.options().dtype(at::kDouble));
    c10::hip::HIPGuard guard(x.get_device());
    auto fn = sum ? tfx_sos_bank_sum_forward : tfx_sos_bank_forward;
    check_rc(fn(x.data_ptr(), dtype_code(x, what), y.data_ptr(), dtype_code(y, what), C, T, banks.data_ptr<double>(), NB, K,
                sx, sy, nsx.data_ptr<double>(), nsy.data_ptr<double>(), precision_or_default(precision), stream_of(x)),
             what);
    return {y, nsx, nsy};
}

std::tuple<Tensor, Tensor, Tensor> bank_op(const Tensor &x, const Tensor &banks, const OptTensor &sx, const OptTensor &sy,
                                           std::optional<at::ScalarType> out_dtype, int64_t precision)
{
    return bank_impl(x, banks, sx, sy, out_dtype, precision, false);
}
std::tuple<Tensor, Tensor, Tensor> bank_sum_op(const Tensor &x, const Tensor &banks, const OptTensor &sx, const OptTensor &sy,
                                               int64_t precision)
{
    return bank_impl(x, banks, sx, sy, std::nullopt, precision, true);
}

// single biquad (binding.cpp:30-50): b [3] tensor, a1 / a2 scalars, states [C, 2]
std::tuple<Tensor, Tensor, Tensor> biquad_op(const Tensor &x_in, const Tensor &b, double a1, double a2, const OptTensor &state_x,
                                             const OptTensor &state_y, std::optional<at::ScalarType> out_dtype, int64_t precision)
{
    TORCH_CHECK(x_in.dim() == 2, "biquad_forward: x must be [C, T], got ", x_in.sizes());
    need_device(x_in, "x");
    const Tensor x = x_in.contiguous();
    const Tensor bh = host_f64(b.reshape({-1}), 3, "biquad_forward");
    const int64_t C = x.size(0), T = x.size(1);
    Tensor kx, ky;
    const double *sx = state_ptr(state_x, {C, 2}, x, "state_x", kx);
    const double *sy = state_ptr(state_y, {C, 2}, x, "state_y", ky);
    Tensor y = at::empty({C, T}, x.options().dtype(out_type(x, out_dtype)));
    Tensor nsx = at::empty({C, 2}, x.options().dtype(at::kDouble));
    Tensor nsy = at::empty({C, 2}, x.options().dtype(at::kDouble));
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_biquad_forward(x.data_ptr(), dtype_code(x, "biquad_forward"), y.data_ptr(), dtype_code(y, "biquad_forward"), C, T,
                                bh.data_ptr<double>(), a1, a2, sx, sy, nsx.data_ptr<double>(), nsy.data_ptr<double>(),
                                precision_or_default(precision), stream_of(x)),
             "biquad_forward");
    return {y, nsx, nsy};
}

// delay line (binding.cpp:68-81 / delay_cpu.cpp:43-85): the input itself when the signal is not longer than the delay
Tensor delay_line_op(const Tensor &x, int64_t delay_samples, double decay, double mix)
{
    need_device(x, "x");
    const int64_t T = x.dim() ? x.size(-1) : 1;
    if (T <= delay_samples) return x;
    const Tensor xc = x.contiguous();
    const int64_t rows = xc.numel() / T;
    Tensor y = at::empty_like(xc);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_delay_line_forward(xc.data_ptr(), y.data_ptr(), dtype_code(xc, "delay_line_forward"), rows, T, delay_samples,
                                    decay, mix, stream_of(x)),
             "delay_line_forward");
    return y;
}

// The streaming ops' history (include/torchfx_hip.h, "Stream history"): the previous chunk's [rows, H] on x's device and in
// x's dtype, or undefined (= silence: None, or nothing to carry)
Tensor stream_hist_in(const OptTensor &hist, const Tensor &x, int64_t rows, int64_t H, const char *what)
{
    if (!hist.has_value() || !hist->defined() || rows * H == 0) return Tensor();
    TORCH_CHECK(hist->dim() == 2 && hist->size(0) == rows && hist->size(1) == H, what, ": history must be [rows, H] = [", rows, ", ", H,
                "], got ", hist->sizes());
    return hist->to(x.device(), x.scalar_type()).contiguous();
}

// rows of x [..., T]: the leading dimensions flattened (also for T = 0)
int64_t stream_rows(const Tensor &x)
{
    TORCH_CHECK(x.dim() >= 1, "stream: x must have a time dimension");
    return c10::multiply_integers(x.sizes().begin(), x.sizes().end() - 1);
}

// BPM-synced multi-tap Delay (effect.py:934-1538): x [..., T] -> [..., T + taps*D], leading dimensions flattened into rows;
// ping-pong when the second-to-last dimension holds a stereo pair, as PingPongDelayStrategy decides
std::vector<int64_t> delay_shape(const Tensor &x, int64_t delay_samples, int64_t taps)
{
    TORCH_CHECK(x.dim() >= 1, "delay_forward: x must have a time dimension");
    TORCH_CHECK(taps >= 1, "delay_forward: at least one tap");
    TORCH_CHECK(delay_samples >= 0, "delay_forward: negative delay");
    std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
    shape.back() += taps * delay_samples;
    return shape;
}

std::tuple<Tensor, Tensor> delay_impl(const Tensor &x_in, int64_t delay_samples, at::ArrayRef<double> amps, double mix, bool pingpong,
                                      const EpilogueArgs &epa)
{
    need_device(x_in, "x");
    const int64_t taps = (int64_t)amps.size();
    const std::vector<int64_t> shape = delay_shape(x_in, delay_samples, taps);
    const Tensor x = x_in.contiguous();
    const int64_t T = x.size(-1), rows = stream_rows(x);
    const bool pp = pingpong && x.dim() >= 2 && x.size(-2) == 2;
    Tensor y = at::empty(shape, x.options()), stat;
    const tfx_epilogue ep = make_epilogue(epa, stat, x, rows);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_delay_forward(x.data_ptr(), y.data_ptr(), dtype_code(x, "delay_forward"), rows, T, delay_samples, taps, amps.data(), mix,
                               pp ? 1 : 0, &ep, stream_of(x)),
             "delay_forward");
    return {y, stat};
}

std::tuple<Tensor, Tensor> delay_ep_op(const Tensor &x, int64_t delay_samples, at::ArrayRef<double> amps, double mix, bool pingpong,
                                       double gain, bool clamp, int64_t stat_mode, bool per_row)
{
    return delay_impl(x, delay_samples, amps, mix, pingpong, {gain, clamp, stat_mode, per_row});
}

Tensor delay_op(const Tensor &x, int64_t delay_samples, at::ArrayRef<double> amps, double mix, bool pingpong)
{
    return std::get<0>(delay_impl(x, delay_samples, amps, mix, pingpong, {1.0, false, -1, false}));      // the neutral epilogue
}

// one chunk of a streaming Delay / delay line (StatefulDelay, StatefulReverb): x [..., T] -> (y [..., T], new history [rows, H]).
// The history of the previous chunk (None = silence) and the chunk are read from their two buffers; the new history is a fresh
// tensor every call (the graph replay of realtime.py copies it into its persistent home).
std::tuple<Tensor, Tensor> delay_stream_op(const Tensor &x_in, const OptTensor &hist, int64_t delay_samples, at::ArrayRef<double> amps,
                                           double mix, bool pingpong)
{
    need_device(x_in, "x");
    const int64_t taps = (int64_t)amps.size();
    TORCH_CHECK(taps >= 1, "delay_stream_forward: at least one tap");
    TORCH_CHECK(delay_samples >= 0, "delay_stream_forward: negative delay");
    const Tensor x = x_in.contiguous();
    const int64_t T = x.size(-1), rows = stream_rows(x), H = taps * delay_samples;
    const bool pp = pingpong && x.dim() >= 2 && x.size(-2) == 2;
    const Tensor hin = stream_hist_in(hist, x, rows, H, "delay_stream_forward");
    Tensor y = at::empty_like(x), hout = at::empty({rows, H}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_delay_stream_forward(x.data_ptr(), y.data_ptr(), dtype_code(x, "delay_stream_forward"), rows, T, delay_samples, taps,
                                      amps.data(), mix, pp ? 1 : 0, hin.defined() ? hin.data_ptr() : nullptr, hout.data_ptr(),
                                      stream_of(x)),
             "delay_stream_forward");
    return {y, hout};
}

std::tuple<Tensor, Tensor> delay_line_stream_op(const Tensor &x_in, const OptTensor &hist, int64_t delay_samples, double decay, double mix)
{
    need_device(x_in, "x");
    TORCH_CHECK(delay_samples >= 0, "delay_line_stream_forward: negative delay");
    const Tensor x = x_in.contiguous();
    const int64_t T = x.size(-1), rows = stream_rows(x);
    const Tensor hin = stream_hist_in(hist, x, rows, delay_samples, "delay_line_stream_forward");
    Tensor y = at::empty_like(x), hout = at::empty({rows, delay_samples}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_delay_line_stream_forward(x.data_ptr(), y.data_ptr(), dtype_code(x, "delay_line_stream_forward"), rows, T, delay_samples,
                                           decay, mix, hin.defined() ? hin.data_ptr() : nullptr, hout.data_ptr(), stream_of(x)),
             "delay_line_stream_forward");
    return {y, hout};
}

// Polyphase resampling (scipy.signal.resample_poly, padtype "constant"): x [..., T] -> [..., ceil(T * up / down)], leading
// dimensions flattened into rows; h HOST [nh] in x's dtype, the designed filter already scaled by up
std::vector<int64_t> resample_shape(const Tensor &x, int64_t up, int64_t down)
{
    TORCH_CHECK(x.dim() >= 1, "resample_forward: x must have a time dimension");
    TORCH_CHECK(up >= 1 && down >= 1, "resample_forward: up and down must be >= 1");
    std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
    TORCH_CHECK(shape.back() <= INT64_MAX / up, "resample_forward: T * up overflows");
    shape.back() = (shape.back() * up + down - 1) / down;
    return shape;
}

Tensor resample_op(const Tensor &x_in, int64_t up, int64_t down, const Tensor &h)
{
    need_device(x_in, "x");
    const std::vector<int64_t> shape = resample_shape(x_in, up, down);
    const Tensor hc = host_vector(h, x_in, "resample_forward", "h"), x = x_in.contiguous();
    const int64_t T = x.size(-1), rows = stream_rows(x);
    Tensor y = at::empty(shape, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_resample_forward(x.data_ptr(), y.data_ptr(), dtype_code(x, "resample_forward"), rows, T, up, down, hc.data_ptr(),
                                  hc.numel(), stream_of(x)),
             "resample_forward");
    return y;
}

// Zero-phase filtering (scipy.signal.sosfiltfilt along the last axis): x [..., T] -> [..., T] of x's dtype, leading dimensions
// flattened into rows; sos HOST [K, 6]; padtype as enum tfx_padtype, padlen -1 = SciPy's default.  The float64 intermediate
// [rows, T + 2 padlen] is a temporary tensor of PyTorch's allocator, released when the op returns (stream-ordered reuse).
Tensor sos_filtfilt_op(const Tensor &x_in, const Tensor &sos_cpu, int64_t padtype, int64_t padlen)
{
    need_device(x_in, "x");
    TORCH_CHECK(x_in.dim() >= 1, "sos_filtfilt: x must have a time dimension");
    const Tensor sos = host_f64(sos_cpu, 6, "sos_filtfilt");
    TORCH_CHECK(sos.dim() == 2, "sos_filtfilt: sos must be [K, 6]");
    const Tensor x = x_in.contiguous();
    const int64_t T = x.size(-1), rows = stream_rows(x), K = sos.size(0);
    const int dt = dtype_code(x, "sos_filtfilt");
    int64_t work_elems = 0;
    check_rc(tfx_sos_filtfilt_plan_info(rows, T, sos.data_ptr<double>(), K, (int)padtype, padlen, nullptr, nullptr, &work_elems,
                                        nullptr, nullptr, nullptr),
             "sos_filtfilt");
    Tensor y = at::empty_like(x);
    if (rows == 0) return y;
    Tensor work = at::empty({work_elems}, x.options().dtype(at::kDouble));
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_sos_filtfilt_forward(x.data_ptr(), dt, y.data_ptr(), dt, rows, T, sos.data_ptr<double>(), K, (int)padtype, padlen,
                                      work.data_ptr<double>(), stream_of(x)),
             "sos_filtfilt");
    return y;
}

// The cascade and the energy of its output per block of samples (tfx_sos_block_energy_forward): x [..., T] -> float64 [..., nblk],
// leading dimensions flattened into rows; sos HOST [K, 6]; blocks [(i num) / den, ((i + 1) num) / den), nblk = (T den) / num
std::vector<int64_t> sos_block_energy_shape(const Tensor &x, const Tensor &sos, int64_t num, int64_t den)
{
    TORCH_CHECK(x.dim() >= 1, "sos_block_energy: x must have a time dimension");
    TORCH_CHECK(sos.dim() == 2 && sos.size(1) == 6, "sos_block_energy: sos must be [K, 6]");
    TORCH_CHECK(num >= 1 && den >= 1 && num / 64 >= den, "sos_block_energy: blocks of num / den = ", num, " / ", den,
                " samples are shorter than 64");
    std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
    TORCH_CHECK(shape.back() <= (int64_t(1) << 61) / den, "sos_block_energy: T * den overflows");
    shape.back() = shape.back() * den / num;
    return shape;
}

Tensor sos_block_energy_op(const Tensor &x_in, const Tensor &sos_cpu, int64_t num, int64_t den)
{
    need_device(x_in, "x");
    const Tensor sos = host_f64(sos_cpu, 6, "sos_block_energy");
    const std::vector<int64_t> shape = sos_block_energy_shape(x_in, sos, num, den);
    const Tensor x = x_in.contiguous();
    const int64_t T = x.size(-1), rows = stream_rows(x), K = sos.size(0);
    const int dt = dtype_code(x, "sos_block_energy");
    int64_t nblk = 0;
    check_rc(tfx_sos_block_energy_plan_info(rows, T, sos.data_ptr<double>(), K, num, den, &nblk, nullptr, nullptr), "sos_block_energy");
    TORCH_CHECK(nblk == shape.back(), "sos_block_energy: the library plans ", nblk, " blocks, the shape has ", shape.back());
    Tensor s = at::empty(shape, x.options().dtype(at::kDouble));
    if (s.numel() == 0) return s;
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_sos_block_energy_forward(x.data_ptr(), dt, s.data_ptr<double>(), rows, T, sos.data_ptr<double>(), K, num, den,
                                          stream_of(x)),
             "sos_block_energy");
    return s;
}

// True peak per row (tfx_true_peak_forward): x [..., T] -> [...] of x's dtype, the linear max |.| over the T * up outputs of
// resample_forward(x, up, 1, taps); taps HOST [nh] in x's dtype, already scaled by up.  The per-tile maxima are a temporary
// tensor of PyTorch's allocator.  A row of no samples has peak 0.
std::vector<int64_t> true_peak_shape(const Tensor &x)
{
    TORCH_CHECK(x.dim() >= 1, "true_peak: x must have a time dimension");
    return std::vector<int64_t>(x.sizes().begin(), x.sizes().end() - 1);
}

Tensor true_peak_op(const Tensor &x_in, const Tensor &taps, int64_t up)
{
    need_device(x_in, "x");
    const std::vector<int64_t> shape = true_peak_shape(x_in);
    const Tensor hc = host_vector(taps, x_in, "true_peak", "taps"), x = x_in.contiguous();
    const int64_t T = x.size(-1), rows = stream_rows(x);
    const int dt = dtype_code(x, "true_peak");
    int64_t Lp = 0, tile_in = 0, tiles = 0, work_elems = 0;
    check_rc(tfx_true_peak_plan_info(rows, T, up, hc.numel(), dt, &Lp, &tile_in, &tiles, &work_elems), "true_peak");
    if (rows * T == 0) return at::zeros(shape, x.options());
    Tensor peak = at::empty(shape, x.options()), work = at::empty({work_elems}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_true_peak_forward(x.data_ptr(), dt, peak.data_ptr(), rows, T, up, hc.data_ptr(), hc.numel(), work.data_ptr(),
                                   stream_of(x)),
             "true_peak");
    return peak;
}

// Look-ahead limiter (tfx_limiter_forward): x [..., T], its rows in groups of `channels` consecutive rows that share one gain
// curve -> (y like x, gain [groups, T] or an empty tensor).  c the linear ceiling already rounded to x's dtype, A / H in samples,
// window HOST [A] and taps HOST [nh] (None for up == 1) in x's dtype.
// what both limiter ops do between the device check and the plan query: the checks, the contiguous tensors and the sizes the C entries take
struct LimiterInputs {
    Tensor x, window, taps;              // contiguous; taps undefined without an interpolator
    int64_t T, rows, groups, nh;         // nh = 0 for up == 1
    int dt;
    const void *taps_ptr() const { return nh ? taps.data_ptr() : nullptr; }
};

LimiterInputs limiter_inputs(const char *what, const Tensor &x_in, int64_t A, const Tensor &window, int64_t up, const OptTensor &taps,
                             int64_t channels)
{
    TORCH_CHECK(x_in.dim() >= 1, what, ": x must have a time dimension");
    LimiterInputs in;
    in.window = host_vector(window, x_in, what, "window", A);
    const bool has_taps = taps.has_value() && taps->defined();
    TORCH_CHECK(up == 1 || has_taps, what, ": up > 1 needs taps");
    if (has_taps) in.taps = host_vector(*taps, x_in, what, "taps");
    in.x = x_in.contiguous();
    in.T = in.x.size(-1);
    in.rows = stream_rows(in.x);
    TORCH_CHECK(channels >= 1 && in.rows % channels == 0, what, ": ", in.rows, " rows do not split into groups of ", channels);
    in.groups = in.rows / channels;
    in.nh = has_taps && up > 1 ? in.taps.numel() : 0;
    in.dt = dtype_code(in.x, what);
    return in;
}

std::tuple<Tensor, Tensor> limiter_op(const Tensor &x_in, double c, int64_t A, int64_t H, const Tensor &window, int64_t up,
                                      const OptTensor &taps, int64_t channels, bool return_gain)
{
    const char *what = "limiter_forward";
    need_device(x_in, "x");
    const LimiterInputs in = limiter_inputs(what, x_in, A, window, up, taps, channels);
    const Tensor &x = in.x;
    int64_t info[6];
    check_rc(tfx_limiter_plan_info(in.groups, channels, in.T, A, H, up, in.nh, in.dt, info, info + 1, info + 2, info + 3, info + 4,
                                   info + 5),
             what);
    Tensor y = at::empty_like(x);
    Tensor gain = return_gain ? at::empty({in.groups, in.T}, x.options()) : at::empty({0}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_limiter_forward(x.data_ptr(), y.data_ptr(), return_gain ? gain.data_ptr() : nullptr, in.dt, in.groups, channels, in.T, c,
                                 A, H, in.window.data_ptr(), up, in.taps_ptr(), in.nh, stream_of(x)),
             what);
    return std::make_tuple(y, gain);
}

// One chunk of a limiter stream (tfx_limiter_stream_forward): x [..., T] after `consumed` samples per row, hist [rows, Hs] (None =
// silence), n_in real inputs in x (-1: all T; fewer: the stream ends after them) -> (y like x: the one-shot result from position
// consumed - D on, gain [groups, T] or an empty tensor, new history [rows, Hs]).  The other arguments as limiter_op's.
std::tuple<Tensor, Tensor, Tensor> limiter_stream_op(const Tensor &x_in, const OptTensor &hist, int64_t consumed, double c, int64_t A,
                                                     int64_t H, const Tensor &window, int64_t up, const OptTensor &taps,
                                                     int64_t channels, bool return_gain, int64_t n_in)
{
    const char *what = "limiter_stream_forward";
    need_device(x_in, "x");
    const LimiterInputs in = limiter_inputs(what, x_in, A, window, up, taps, channels);
    const Tensor &x = in.x;
    int64_t info[6];
    check_rc(tfx_limiter_stream_plan_info(in.groups, channels, in.T, A, H, up, in.nh, in.dt, info, info + 1, info + 2, info + 3, info + 4,
                                          info + 5),
             what);
    const int64_t Hs = info[1];
    const Tensor hin = stream_hist_in(hist, x, in.rows, Hs, what);
    Tensor y = at::empty_like(x), hout = at::empty({in.rows, Hs}, x.options());
    Tensor gain = return_gain ? at::empty({in.groups, in.T}, x.options()) : at::empty({0}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_limiter_stream_forward(x.data_ptr(), y.data_ptr(), return_gain ? gain.data_ptr() : nullptr, in.dt, in.groups, channels,
                                        in.T, n_in < 0 ? in.T : n_in, consumed, c, A, H, in.window.data_ptr(), up, in.taps_ptr(), in.nh,
                                        hin.defined() ? hin.data_ptr() : nullptr, hout.data_ptr(), stream_of(x)),
             what);
    return std::make_tuple(y, gain, hout);
}

// What the scan-parallel ops (compressor, gate, phaser) do between their shape checks and the C entry: the contiguous x and its
// dtype code, the rows split into units of `per_unit` rows, the plan query (plan_info(units, T, info) -> rc; info[4] the scratch
// bytes), the state [units, width] float64 or None, and the tensors for the new state and for the summaries between the launches.
struct ScanInputs {
    Tensor x, state, sout, scratch;      // x contiguous; state the given one on x's device, or undefined
    int64_t T, units;
    int dt;
    const double *sin;                   // null without a state
    void *scratch_ptr;                   // null when the plan needs none
};

template <typename PlanInfo>
ScanInputs scan_inputs(const char *what, const Tensor &x_in, int64_t per_unit, int64_t width, const OptTensor &state, PlanInfo plan_info)
{
    ScanInputs in;
    in.x = x_in.contiguous();
    in.dt = dtype_code(in.x, what);
    in.T = in.x.size(-1);
    const int64_t rows = stream_rows(in.x);
    TORCH_CHECK(per_unit >= 1 && rows % per_unit == 0, what, ": ", rows, " rows do not split into groups of ", per_unit);
    in.units = rows / per_unit;             // the phaser's units are its rows (per_unit 1): the check above is the dynamics effects'
    int64_t info[5];
    check_rc(plan_info(in.units, in.T, info), what);
    in.sin = state_ptr(state, {in.units, width}, in.x, (std::string(what) + ": state").c_str(), in.state);
    const auto f64 = in.x.options().dtype(at::kDouble);
    in.sout = at::empty({in.units, width}, f64);
    in.scratch = at::empty({info[4] / 8}, f64);
    in.scratch_ptr = info[4] ? in.scratch.data_ptr() : nullptr;
    return in;
}

// Feed-forward compressor (tfx_compressor_forward): x [..., T], its rows in groups of `channels` consecutive rows that share one
// gain curve; th, s, w, alpha_a, alpha_r, makeup_db as the C entry takes them; state [groups, 2] float64 (y1, yL) or None
// (silence); segments 0 = the plan's choice -> (y like x, gain [groups, T] or an empty tensor, new state [groups, 2] float64).
// The summaries between the launches live in a tensor from torch's allocator.
std::tuple<Tensor, Tensor, Tensor> compressor_op(const Tensor &x_in, double th, double s, double w, double alpha_a, double alpha_r,
                                                 double makeup_db, int64_t channels, const OptTensor &state, bool return_gain,
                                                 int64_t segments)
{
    const char *what = "compressor_forward";
    need_device(x_in, "x");
    TORCH_CHECK(x_in.dim() >= 1, what, ": x must have a time dimension");
    const ScanInputs in = scan_inputs(what, x_in, channels, 2, state, [&](int64_t groups, int64_t T, int64_t *info) {
        return tfx_compressor_plan_info(groups, channels, T, segments, info, info + 1, info + 2, info + 3, info + 4);
    });
    const Tensor &x = in.x;
    Tensor y = at::empty_like(x);
    Tensor gain = return_gain ? at::empty({in.units, in.T}, x.options()) : at::empty({0}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_compressor_forward(x.data_ptr(), y.data_ptr(), return_gain ? gain.data_ptr() : nullptr, in.dt, in.units, channels, in.T,
                                    th, s, w, alpha_a, alpha_r, makeup_db, in.sin, in.sout.data_ptr<double>(), segments, in.scratch_ptr,
                                    stream_of(x)),
             what);
    return std::make_tuple(y, gain, in.sout);
}

// Noise gate (tfx_gate_forward): x [..., T], its rows in groups of `channels` consecutive rows that share one gain curve; p_open,
// p_close, range (linear), hold (samples), alpha_a, alpha_r as the C entry takes them; state [groups, 3] float64 (g, open, c) or
// None (closed, g = range); segments 0 = the plan's choice -> (y like x, gain [groups, T] or an empty tensor, open [groups, T]
// uint8 or an empty tensor, new state [groups, 3] float64).  The summaries between the launches live in a tensor from torch's
// allocator.
std::tuple<Tensor, Tensor, Tensor, Tensor> gate_op(const Tensor &x_in, double p_open, double p_close, double range, int64_t hold,
                                                   double alpha_a, double alpha_r, int64_t channels, const OptTensor &state,
                                                   bool return_gain, bool return_open, int64_t segments)
{
    const char *what = "gate_forward";
    need_device(x_in, "x");
    TORCH_CHECK(x_in.dim() >= 1, what, ": x must have a time dimension");
    const ScanInputs in = scan_inputs(what, x_in, channels, 3, state, [&](int64_t groups, int64_t T, int64_t *info) {
        return tfx_gate_plan_info(groups, channels, T, segments, info, info + 1, info + 2, info + 3, info + 4);
    });
    const Tensor &x = in.x;
    const auto u8 = x.options().dtype(at::kByte);
    Tensor y = at::empty_like(x);
    Tensor gain = return_gain ? at::empty({in.units, in.T}, x.options()) : at::empty({0}, x.options());
    Tensor open = return_open ? at::empty({in.units, in.T}, u8) : at::empty({0}, u8);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_gate_forward(x.data_ptr(), y.data_ptr(), return_gain ? gain.data_ptr() : nullptr,
                              return_open ? open.data_ptr<uint8_t>() : nullptr, in.dt, in.units, channels, in.T, p_open, p_close, range,
                              hold, alpha_a, alpha_r, in.sin, in.sout.data_ptr<double>(), segments, in.scratch_ptr, stream_of(x)),
             what);
    return std::make_tuple(y, gain, open, in.sout);
}

// Short-time Fourier transform (tfx_stft_forward): x [..., T]; window a 1-D device tensor of x's dtype with 1 <= numel <= n_fft
// (centred in zeros) or None (ones over n_fft); pad samples at each end, pad_mode a tfx_stft_pad; power 0 (complex), 1 or 2 ->
// [..., n_fft / 2 + 1, frames], the transposed view of a contiguous [..., frames, n_fft / 2 + 1] buffer, as torch.stft returns it.
struct StftShape {
    std::vector<int64_t> sizes;     // [..., frames, bins]
    at::ScalarType dtype;
    int64_t win_length;
};

StftShape stft_shape(const Tensor &x, const OptTensor &window, int64_t n_fft, int64_t hop, int64_t pad, int64_t power, const char *what)
{
    TORCH_CHECK(x.dim() >= 1 && x.size(-1) >= 1, what, ": x must have a non-empty time dimension");
    TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble, what, ": expected a float32 or float64 tensor, got ",
                x.scalar_type());
    TORCH_CHECK(n_fft >= 2 && hop >= 1 && pad >= 0 && x.size(-1) + 2 * pad >= n_fft, what, ": bad geometry (n_fft ", n_fft, ", hop ", hop,
                ", pad ", pad, ", T ", x.size(-1), ")");
    TORCH_CHECK(power >= 0 && power <= 2, what, ": power must be 0 (complex), 1 or 2");
    StftShape s;
    s.win_length = n_fft;
    if (window.has_value() && window->defined()) {
        TORCH_CHECK(window->dim() == 1 && window->numel() >= 1 && window->numel() <= n_fft, what, ": window must be 1-D with 1 to n_fft values");
        TORCH_CHECK(window->scalar_type() == x.scalar_type() && window->device() == x.device(), what, ": window must have x's dtype and device");
        s.win_length = window->numel();
    }
    s.sizes.assign(x.sizes().begin(), x.sizes().end() - 1);
    s.sizes.push_back(1 + (x.size(-1) + 2 * pad - n_fft) / hop);
    s.sizes.push_back(n_fft / 2 + 1);
    s.dtype = power != 0 ? x.scalar_type() : (x.scalar_type() == at::kFloat ? at::kComplexFloat : at::kComplexDouble);
    return s;
}

Tensor stft_op(const Tensor &x_in, const OptTensor &window, int64_t n_fft, int64_t hop, int64_t pad, int64_t pad_mode, int64_t power,
               bool normalized)
{
    const char *what = "stft_forward";
    need_device(x_in, "x");
    const StftShape s = stft_shape(x_in, window, n_fft, hop, pad, power, what);
    const Tensor x = x_in.contiguous();
    Tensor w;
    if (window.has_value() && window->defined()) w = window->contiguous();
    const int64_t T = x.size(-1), rows = stream_rows(x);
    Tensor out = at::empty(s.sizes, x.options().dtype(s.dtype));
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_stft_forward(x.data_ptr(), w.defined() ? w.data_ptr() : nullptr, out.data_ptr(), dtype_code(x, what), rows, T, n_fft, hop,
                              s.win_length, pad, (int)pad_mode, (int)power, normalized ? 1 : 0, stream_of(x)),
             what);
    return out.transpose(-1, -2);
}

// Inverse short-time Fourier transform (tfx_istft_forward): spec [bins, frames], [C, bins, frames] or [B, C, bins, frames],
// complex64 / complex128 with bins = n_fft / 2 + 1; window a 1-D device tensor of the matching real dtype with hop <= numel <=
// n_fft (centred in zeros) or None (ones over n_fft); pad samples cut from each end; length -1 = natural -> (y [..., T] of the
// real dtype, flag [1] int32: 1 where the window envelope vanishes, which the caller reads when it may synchronise).  The kernel
// reads the buffer stft_forward writes -- the transpose of a contiguous [..., frames, bins] -- in place; any other layout is
// copied into it first.
struct IstftShape {
    std::vector<int64_t> sizes;     // [..., T]
    at::ScalarType dtype;
    int64_t win_length, frames;
};

IstftShape istft_shape(const Tensor &spec, const OptTensor &window, int64_t n_fft, int64_t hop, int64_t pad, int64_t length, const char *what)
{
    TORCH_CHECK(spec.dim() >= 2 && spec.dim() <= 4, what, ": spec must be [bins, frames], [C, bins, frames] or [B, C, bins, frames], got ",
                spec.dim(), " dimensions");
    TORCH_CHECK(spec.scalar_type() == at::kComplexFloat || spec.scalar_type() == at::kComplexDouble, what,
                ": expected a complex64 or complex128 tensor, got ", spec.scalar_type());
    TORCH_CHECK(n_fft >= 2 && spec.size(-2) == n_fft / 2 + 1, what, ": expected the frequency dimension (2nd to the last) to be n_fft / 2 + 1 = ",
                n_fft / 2 + 1, ", got ", spec.size(-2));
    TORCH_CHECK(spec.size(-1) >= 1 && hop >= 1 && pad >= 0 && (length == -1 || length >= 1), what, ": bad geometry (frames ", spec.size(-1),
                ", hop ", hop, ", pad ", pad, ", length ", length, ")");
    IstftShape s;
    s.dtype = spec.scalar_type() == at::kComplexFloat ? at::kFloat : at::kDouble;
    s.win_length = n_fft;
    s.frames = spec.size(-1);
    if (window.has_value() && window->defined()) {
        TORCH_CHECK(window->dim() == 1 && window->numel() >= 1 && window->numel() <= n_fft, what, ": window must be 1-D with 1 to n_fft values");
        TORCH_CHECK(window->scalar_type() == s.dtype && window->device() == spec.device(), what,
                    ": window must have spec's real dtype and device");
        s.win_length = window->numel();
    }
    TORCH_CHECK(hop <= s.win_length, what, ": expected 0 < hop <= win_length, got hop ", hop, " and win_length ", s.win_length);
    const int64_t T = length == -1 ? (s.frames - 1) * hop + n_fft - 2 * pad : length;
    TORCH_CHECK(T >= 1, what, ": ", s.frames, " frames leave no sample after ", pad, " are cut from each end");
    s.sizes.assign(spec.sizes().begin(), spec.sizes().end() - 2);
    s.sizes.push_back(T);
    return s;
}

std::tuple<Tensor, Tensor> istft_op(const Tensor &spec_in, const OptTensor &window, int64_t n_fft, int64_t hop, int64_t pad, int64_t length,
                                    bool normalized)
{
    const char *what = "istft_forward";
    need_device(spec_in, "spec");
    const IstftShape s = istft_shape(spec_in, window, n_fft, hop, pad, length, what);
    const Tensor spec = spec_in.transpose(-1, -2).contiguous();         // [..., frames, bins]: no copy for stft_forward's layout
    Tensor w;
    if (window.has_value() && window->defined()) w = window->contiguous();
    const int64_t rows = c10::multiply_integers(s.sizes.begin(), s.sizes.end() - 1);
    Tensor out = at::empty(s.sizes, spec.options().dtype(s.dtype));
    Tensor flag = at::empty({1}, spec.options().dtype(at::kInt));
    c10::hip::HIPGuard guard(spec.get_device());
    check_rc(tfx_istft_forward(spec.data_ptr(), w.defined() ? w.data_ptr() : nullptr, out.data_ptr(), flag.data_ptr<int>(),
                               s.dtype == at::kFloat ? TFX_F32 : TFX_F64, rows, s.frames, n_fft, hop, s.win_length, pad, length,
                               normalized ? 1 : 0, stream_of(spec)),
             what);
    return std::make_tuple(out, flag);
}

// Freeverb (tfx_freeverb_forward): x [T], [C, T] or [B, C, T] with C 1 or 2; comb_delays / allpass_delays the flattened
// [C, NC] / [C, NA] tables in samples; state [B * C, state_len] float64 or None (silence) -> (y [..., T + tail], new state).
// The shape and the tables are checked here and by the plan, before anything touches the device; the workspace (global lines,
// the wet signal between two launches) is a tensor from torch's allocator.
struct FreeverbInputs {
    Tensor x;
    std::vector<int64_t> comb, allpass, yshape;
    int dt, placement;
    int64_t batch, channels, T, NC, NA, block, state_len, launches, workspace_bytes;
};

FreeverbInputs freeverb_inputs(const Tensor &x, at::IntArrayRef comb_delays, at::IntArrayRef allpass_delays, double wet2, int64_t tail,
                               const char *what)
{
    TORCH_CHECK(x.dim() >= 1 && x.dim() <= 3, what, ": x must be [T], [C, T] or [B, C, T], got ", x.dim(), " dimensions");
    TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble, what, ": float32 or float64 only, got ", x.scalar_type());
    FreeverbInputs in;
    in.dt = x.scalar_type() == at::kFloat ? TFX_F32 : TFX_F64;
    in.T = x.size(-1);
    in.channels = x.dim() >= 2 ? x.size(-2) : 1;
    in.batch = x.dim() == 3 ? x.size(0) : 1;
    TORCH_CHECK(in.channels == 1 || in.channels == 2, what, ": channels must be 1 or 2, got ", in.channels);
    TORCH_CHECK(comb_delays.size() % in.channels == 0 && allpass_delays.size() % in.channels == 0, what,
                ": the delay tables must hold one row per channel");
    in.comb.assign(comb_delays.begin(), comb_delays.end());
    in.allpass.assign(allpass_delays.begin(), allpass_delays.end());
    in.NC = (int64_t)in.comb.size() / in.channels;
    in.NA = (int64_t)in.allpass.size() / in.channels;
    check_rc(tfx_freeverb_plan_info(in.batch, in.channels, in.T, tail, in.comb.data(), in.NC, in.NA ? in.allpass.data() : nullptr, in.NA,
                                    wet2, &in.block, &in.placement, &in.state_len, &in.launches, &in.workspace_bytes),
             what);
    in.yshape.assign(x.sizes().begin(), x.sizes().end());
    in.yshape.back() = in.T + tail;
    return in;
}

std::tuple<Tensor, Tensor> freeverb_op(const Tensor &x_in, at::IntArrayRef comb_delays, at::IntArrayRef allpass_delays, double feedback,
                                       double damp, double allpass_gain, double input_gain, double dry_gain, double wet1, double wet2,
                                       int64_t tail, const OptTensor &state)
{
    const char *what = "freeverb_forward";
    need_device(x_in, "x");
    FreeverbInputs in = freeverb_inputs(x_in, comb_delays, allpass_delays, wet2, tail, what);
    const Tensor x = x_in.contiguous();
    const int64_t banks = in.batch * in.channels;
    Tensor keep;
    const double *sin = state_ptr(state, {banks, in.state_len}, x, "freeverb_forward: state", keep);
    const auto f64 = x.options().dtype(at::kDouble);
    Tensor y = at::empty(in.yshape, x.options()), sout = at::empty({banks, in.state_len}, f64),
           work = at::empty({in.workspace_bytes / 8}, f64);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_freeverb_forward(x.data_ptr(), y.data_ptr(), in.dt, in.batch, in.channels, in.T, tail, in.comb.data(), in.NC,
                                  in.NA ? in.allpass.data() : nullptr, in.NA, feedback, damp, allpass_gain, input_gain, dry_gain, wet1,
                                  wet2, sin, sout.data_ptr<double>(), in.workspace_bytes ? work.data_ptr() : nullptr, stream_of(x)),
             what);
    return std::make_tuple(y, sout);
}

// The modulated delay line (tfx_modulated_delay_forward): x [T], [C, T] or [B, C, T]; voices a host float64 [V, 5] table of
// (base, depth, inc, phase, gain) rows; shape 0 sine / 1 triangle, interp 0 linear / 1 cubic.  V, the shape of x and the
// interpolation are checked here, before anything touches the device.
struct ModInputs {
    Tensor x, voices;
    int dt;
    int64_t batch, channels, T, V, H;
};

ModInputs mod_inputs(const Tensor &x_in, const Tensor &voices, int64_t shape, int64_t interp, const char *what)
{
    need_device(x_in, "x");
    TORCH_CHECK(x_in.dim() >= 1 && x_in.dim() <= 3, what, ": x must be [T], [C, T] or [B, C, T], got ", x_in.dim(), " dimensions");
    TORCH_CHECK(!voices.is_cuda() && voices.dim() == 2 && voices.size(1) == 5 && voices.scalar_type() == at::kDouble, what,
                ": voices must be a host float64 [V, 5] tensor");
    TORCH_CHECK(voices.size(0) >= 1 && voices.size(0) <= 8, what, ": the number of voices must be in [1, 8], got ", voices.size(0));
    TORCH_CHECK(shape == TFX_LFO_SINE || shape == TFX_LFO_TRIANGLE, what, ": bad LFO shape ", shape);
    TORCH_CHECK(interp == TFX_INTERP_LINEAR || interp == TFX_INTERP_CUBIC, what, ": bad interpolation ", interp);
    ModInputs in;
    in.x = x_in.contiguous();
    in.voices = voices.contiguous();
    in.dt = dtype_code(in.x, what);
    in.T = in.x.size(-1);
    in.channels = in.x.dim() >= 2 ? in.x.size(-2) : 1;
    in.batch = in.x.dim() == 3 ? in.x.size(0) : 1;
    in.V = in.voices.size(0);
    TORCH_CHECK(in.channels >= 1, what, ": x has no channels");
    int64_t info[5];
    check_rc(tfx_modulated_delay_plan_info(in.batch, in.channels, in.T, in.voices.data_ptr<double>(), in.V, (int)interp, info, info + 1,
                                           info + 2, info + 3, info + 4),
             what);
    in.H = info[2];
    return in;
}

Tensor modulated_delay_op(const Tensor &x_in, const Tensor &voices, double spread, double dry, int64_t shape, int64_t interp,
                          int64_t position)
{
    const char *what = "modulated_delay_forward";
    const ModInputs in = mod_inputs(x_in, voices, shape, interp, what);
    Tensor y = at::empty_like(in.x);
    c10::hip::HIPGuard guard(in.x.get_device());
    check_rc(tfx_modulated_delay_forward(in.x.data_ptr(), y.data_ptr(), in.dt, in.batch, in.channels, in.T, in.voices.data_ptr<double>(),
                                         in.V, spread, dry, (int)shape, (int)interp, position, stream_of(in.x)),
             what);
    return y;
}

// one chunk of a modulated-delay stream: hist [rows, H] or None (silence), pos a device int64 [1] or None (0)
// -> (y like x, new history [rows, H], new position int64 [1]), both fresh tensors (the graph replay of realtime.py copies them
// into their persistent homes)
std::tuple<Tensor, Tensor, Tensor> modulated_delay_stream_op(const Tensor &x_in, const OptTensor &hist, const OptTensor &pos,
                                                             const Tensor &voices, double spread, double dry, int64_t shape,
                                                             int64_t interp)
{
    const char *what = "modulated_delay_stream_forward";
    const ModInputs in = mod_inputs(x_in, voices, shape, interp, what);
    const int64_t rows = in.batch * in.channels;
    const Tensor hin = stream_hist_in(hist, in.x, rows, in.H, what);
    Tensor pin;
    if (pos.has_value() && pos->defined()) {
        TORCH_CHECK(pos->numel() == 1 && pos->scalar_type() == at::kLong, what, ": the position must be an int64 tensor of one element");
        pin = pos->to(in.x.device()).contiguous();
    }
    Tensor y = at::empty_like(in.x), hout = at::empty({rows, in.H}, in.x.options()),
           pout = at::empty({1}, in.x.options().dtype(at::kLong));
    c10::hip::HIPGuard guard(in.x.get_device());
    check_rc(tfx_modulated_delay_stream_forward(in.x.data_ptr(), y.data_ptr(), in.dt, in.batch, in.channels, in.T,
                                                in.voices.data_ptr<double>(), in.V, spread, dry, (int)shape, (int)interp,
                                                hin.defined() ? hin.data_ptr() : nullptr, hout.data_ptr(),
                                                pin.defined() ? pin.data_ptr<int64_t>() : nullptr, pout.data_ptr<int64_t>(),
                                                stream_of(in.x)),
             what);
    return std::make_tuple(y, hout, pout);
}

// The phaser (tfx_phaser_forward): x [T], [C, T] or [B, C, T]; the parameters as the C entry takes them; pos a device int64 [1]
// (a stream's position; None = the host scalar `position`), state [rows, stages + 1] float64 or None (silence); segments 0 = the
// plan's choice -> (y like x, coef [C or 1, T] float64 or an empty tensor, new state [rows, stages + 1] float64, pos + T as a
// fresh int64 [1] or an empty tensor without pos).  The summaries between the launches live in a tensor from torch's allocator.
int64_t phaser_coef_rows(int64_t channels, double spread) { return (spread == 0.0 || channels == 1) ? 1 : channels; }

std::tuple<Tensor, Tensor, Tensor, Tensor> phaser_op(const Tensor &x_in, int64_t stages, double fs, double rate, double min_freq,
                                                     double max_freq, double phase, double spread, double dry, double wet, int64_t shape,
                                                     int64_t position, const OptTensor &pos, const OptTensor &state, bool return_coef,
                                                     int64_t segments)
{
    const char *what = "phaser_forward";
    need_device(x_in, "x");
    TORCH_CHECK(x_in.dim() >= 1 && x_in.dim() <= 3, what, ": x must be [T], [C, T] or [B, C, T], got ", x_in.dim(), " dimensions");
    TORCH_CHECK(shape == TFX_LFO_SINE || shape == TFX_LFO_TRIANGLE, what, ": bad LFO shape ", shape);
    const int64_t channels = x_in.dim() >= 2 ? x_in.size(-2) : 1;
    const ScanInputs in = scan_inputs(what, x_in, 1, stages + 1, state, [&](int64_t rows, int64_t T, int64_t *info) {
        TORCH_CHECK(channels >= 1, what, ": x has no channels");    // here, not in front: callers meet it after the dtype check, as ever
        return tfx_phaser_plan_info(rows, channels, T, stages, segments, info, info + 1, info + 2, info + 3, info + 4);
    });
    const Tensor &x = in.x;
    const int64_t T = in.T;
    Tensor pin;
    if (pos.has_value() && pos->defined()) {
        TORCH_CHECK(pos->numel() == 1 && pos->scalar_type() == at::kLong, what, ": the position must be an int64 tensor of one element");
        pin = pos->to(x.device()).contiguous();
    }
    const auto f64 = x.options().dtype(at::kDouble), i64 = x.options().dtype(at::kLong);
    Tensor y = at::empty_like(x);
    Tensor coef = return_coef ? at::empty({phaser_coef_rows(channels, spread), T}, f64) : at::empty({0}, f64);
    Tensor pout = at::empty({pin.defined() ? 1 : 0}, i64);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_phaser_forward(x.data_ptr(), y.data_ptr(), return_coef ? coef.data_ptr<double>() : nullptr, in.dt, in.units, channels, T, stages,
                                fs, rate, min_freq, max_freq, phase, spread, dry, wet, (int)shape, position,
                                pin.defined() ? pin.data_ptr<int64_t>() : nullptr, pin.defined() ? pout.data_ptr<int64_t>() : nullptr, in.sin,
                                in.sout.data_ptr<double>(), segments, in.scratch_ptr, stream_of(x)),
             what);
    return std::make_tuple(y, coef, in.sout, pout);
}

std::tuple<Tensor, Tensor, Tensor, Tensor> phaser_meta(const Tensor &x, int64_t stages, double, double, double, double, double,
                                                       double spread, double, double, int64_t, int64_t, const OptTensor &pos,
                                                       const OptTensor &, bool return_coef, int64_t)
{
    TORCH_CHECK(x.dim() >= 1 && x.dim() <= 3 && stages >= 1, "phaser_forward: bad shape");
    const int64_t T = x.size(-1), channels = x.dim() >= 2 ? x.size(-2) : 1;
    const auto f64 = x.options().dtype(at::kDouble);
    return {at::empty_like(x), return_coef ? at::empty({phaser_coef_rows(channels, spread), T}, f64) : at::empty({0}, f64),
            at::empty({stream_rows(x), stages + 1}, f64),
            at::empty({pos.has_value() && pos->defined() ? 1 : 0}, x.options().dtype(at::kLong))};
}

// What the waveshaper's two ops take: x [..., T] contiguous, rows independent; curve (shape 3 only) and the two tap vectors
// (oversample > 1 only) host tensors of x's dtype
struct ShaperInputs {
    Tensor x, cv, hu, hd;
    int64_t T = 0, rows = 0;
    int dt = 0;
    int64_t n_curve() const { return cv.defined() ? cv.numel() : 0; }
    int64_t n_up() const { return hu.defined() ? hu.numel() : 0; }
    int64_t n_dn() const { return hd.defined() ? hd.numel() : 0; }
    const void *curve_ptr() const { return cv.defined() ? cv.data_ptr() : nullptr; }
    const void *up_ptr() const { return hu.defined() ? hu.data_ptr() : nullptr; }
    const void *dn_ptr() const { return hd.defined() ? hd.data_ptr() : nullptr; }
};

ShaperInputs shaper_inputs(const char *what, const Tensor &x_in, int64_t oversample, int64_t shape, const OptTensor &curve,
                           const OptTensor &taps_up, const OptTensor &taps_dn)
{
    need_device(x_in, "x");
    TORCH_CHECK(x_in.dim() >= 1, what, ": x must have a time dimension");
    ShaperInputs in;
    in.x = x_in.contiguous();
    in.dt = dtype_code(in.x, what);
    const bool has_curve = curve.has_value() && curve->defined();
    TORCH_CHECK(has_curve == (shape == TFX_SHAPE_CURVE), what, ": a curve goes with shape ", (int)TFX_SHAPE_CURVE, " and with no other");
    if (has_curve) in.cv = host_vector(*curve, in.x, what, "curve");
    if (oversample != 1) {
        TORCH_CHECK(taps_up.has_value() && taps_up->defined() && taps_dn.has_value() && taps_dn->defined(), what,
                    ": oversample > 1 needs the taps of both stages");
        in.hu = host_vector(*taps_up, in.x, what, "taps_up");
        in.hd = host_vector(*taps_dn, in.x, what, "taps_dn");
    }
    in.T = in.x.size(-1);
    in.rows = stream_rows(in.x);
    return in;
}

// The oversampled waveshaper (tfx_waveshaper_forward).  Everything is checked by the plan query before anything touches the device.
Tensor waveshaper_op(const Tensor &x_in, int64_t oversample, int64_t shape, const OptTensor &curve, double drive, double bias, double dry,
                     double wet, const OptTensor &taps_up, const OptTensor &taps_dn)
{
    const char *what = "waveshaper_forward";
    const ShaperInputs in = shaper_inputs(what, x_in, oversample, shape, curve, taps_up, taps_dn);
    const Tensor &x = in.x;
    int64_t info[7];
    check_rc(tfx_waveshaper_plan_info(in.rows, in.T, oversample, in.n_up(), in.n_dn(), in.n_curve(), in.dt, info, info + 1, info + 2,
                                      info + 3, info + 4, info + 5, info + 6),
             what);
    Tensor y = at::empty_like(x);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_waveshaper_forward(x.data_ptr(), y.data_ptr(), in.dt, in.rows, in.T, oversample, (int)shape, in.curve_ptr(), in.n_curve(),
                                    drive, bias, dry, wet, in.up_ptr(), in.n_up(), in.dn_ptr(), in.n_dn(), stream_of(x)),
             what);
    return y;
}

// One chunk of a waveshaper stream (tfx_waveshaper_stream_forward): x [..., T] after `consumed` samples per row, hist [rows, Hs]
// (None = silence), n_in real inputs in x (-1: all T; fewer: the stream ends after them) -> (y like x: the one-shot result from
// position consumed - D on, new history [rows, Hs]).  The other arguments as waveshaper_op's.
std::tuple<Tensor, Tensor> waveshaper_stream_op(const Tensor &x_in, const OptTensor &hist, int64_t consumed, int64_t oversample,
                                                int64_t shape, const OptTensor &curve, double drive, double bias, double dry, double wet,
                                                const OptTensor &taps_up, const OptTensor &taps_dn, int64_t n_in)
{
    const char *what = "waveshaper_stream_forward";
    const ShaperInputs in = shaper_inputs(what, x_in, oversample, shape, curve, taps_up, taps_dn);
    const Tensor &x = in.x;
    int64_t info[6];
    check_rc(tfx_waveshaper_stream_plan_info(in.rows, in.T, oversample, in.n_up(), in.n_dn(), in.n_curve(), in.dt, info, info + 1,
                                             info + 2, info + 3, info + 4, info + 5),
             what);
    const int64_t Hs = info[1];
    const Tensor hin = stream_hist_in(hist, x, in.rows, Hs, what);
    Tensor y = at::empty_like(x), hout = at::empty({in.rows, Hs}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_waveshaper_stream_forward(x.data_ptr(), y.data_ptr(), in.dt, in.rows, in.T, n_in < 0 ? in.T : n_in, consumed, oversample,
                                           (int)shape, in.curve_ptr(), in.n_curve(), drive, bias, dry, wet, in.up_ptr(), in.n_up(),
                                           in.dn_ptr(), in.n_dn(), hin.defined() ? hin.data_ptr() : nullptr,
                                           Hs ? hout.data_ptr() : nullptr, stream_of(x)),
             what);
    return std::make_tuple(y, hout);
}

// One chunk of a resampling stream (tfx_resample_stream_forward): x [..., T] after `consumed` samples per row, h as for
// resample_forward, hist [rows, H] (None = silence) -> (y [..., M(consumed + T) - M(consumed)], new history [rows, H])
struct ResampleStreamPlan {
    int64_t begin, end, H, pre, Lp, lds;
    int kernel;
};

ResampleStreamPlan resample_stream_plan(const Tensor &x, const Tensor &h, int64_t up, int64_t down, int64_t consumed)
{
    TORCH_CHECK(x.dim() >= 1, "resample_stream_forward: x must have a time dimension");
    TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble, "resample_stream_forward: float32 or float64 only, got ",
                x.scalar_type());
    ResampleStreamPlan p{};
    check_rc(tfx_resample_stream_plan_info(consumed, x.size(-1), up, down, h.numel(), x.scalar_type() == at::kFloat ? TFX_F32 : TFX_F64,
                                           &p.begin, &p.end, &p.H, &p.pre, &p.Lp, &p.kernel, &p.lds),
             "resample_stream_forward");
    return p;
}

std::tuple<Tensor, Tensor> resample_stream_op(const Tensor &x_in, const Tensor &h, const OptTensor &hist, int64_t up, int64_t down,
                                              int64_t consumed)
{
    need_device(x_in, "x");
    const Tensor hc = host_vector(h, x_in, "resample_stream_forward", "h");
    const ResampleStreamPlan pl = resample_stream_plan(x_in, hc, up, down, consumed);
    const Tensor x = x_in.contiguous();
    const int64_t T = x.size(-1), rows = stream_rows(x);
    const Tensor hin = stream_hist_in(hist, x, rows, pl.H, "resample_stream_forward");
    std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
    shape.back() = pl.end - pl.begin;
    Tensor y = at::empty(shape, x.options()), hout = at::empty({rows, pl.H}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_resample_stream_forward(x.data_ptr(), y.data_ptr(), dtype_code(x, "resample_stream_forward"), rows, T, up, down,
                                         hc.data_ptr(), hc.numel(), consumed, hin.defined() ? hin.data_ptr() : nullptr,
                                         hout.data_ptr(), stream_of(x)),
             "resample_stream_forward");
    return {y, hout};
}

// ---------------------------------------------------------------------------------------------------
// FIR (fir.py:556-568) and overlap-save FFT convolution (_fftconv.py:70-141)
// ---------------------------------------------------------------------------------------------------
Tensor taps_host(const Tensor &kernel, const Tensor &x)
{
    return kernel.detach().reshape({-1}).to(at::kCPU, x.scalar_type()).contiguous();
}

Tensor fir_direct_op(const Tensor &x_in, const Tensor &kernel)
{
    TORCH_CHECK(x_in.dim() == 2, "fir_direct_forward: x must be [C, T], got ", x_in.sizes());
    need_device(x_in, "x");
    const Tensor x = x_in.contiguous();
    const Tensor k = taps_host(kernel, x);
    Tensor y = at::empty_like(x);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_fir_direct_forward(x.data_ptr(), y.data_ptr(), dtype_code(x, "fir_direct_forward"), x.size(0), x.size(1),
                                    k.data_ptr(), k.numel(), stream_of(x)),
             "fir_direct_forward");
    return y;
}

// fft_conv_forward (tfx_fft_conv_forward) and, with `epa`, fft_conv_forward_ep (tfx_fft_conv_forward_ep): y and the epilogue's
// statistic (undefined without one)
std::tuple<Tensor, Tensor> fft_conv_impl(const Tensor &x_in, const Tensor &kernel, int64_t pad_left, int64_t pad_right,
                                         const EpilogueArgs *epa)
{
    const char *what = epa ? "fft_conv_forward_ep" : "fft_conv_forward";
    TORCH_CHECK(x_in.dim() == 2, what, ": x must be [C, T], got ", x_in.sizes());
    need_device(x_in, "x");
    const Tensor x = x_in.contiguous();
    const Tensor k = taps_host(kernel, x);
    const int64_t C = x.size(0), T = x.size(1), K = k.numel();
    const int64_t tout = T + pad_left + pad_right - K + 1;
    Tensor y = at::empty({C, tout > 0 ? tout : 0}, x.options()), stat;
    tfx_epilogue ep{};
    if (epa) ep = make_epilogue(*epa, stat, x, C);
    const int dt = dtype_code(x, what);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(epa ? tfx_fft_conv_forward_ep(x.data_ptr(), y.data_ptr(), dt, C, T, k.data_ptr(), K, pad_left, pad_right, &ep, stream_of(x))
                 : tfx_fft_conv_forward(x.data_ptr(), y.data_ptr(), dt, C, T, k.data_ptr(), K, pad_left, pad_right, stream_of(x)),
             what);
    return {y, stat};
}

Tensor fft_conv_op(const Tensor &x, const Tensor &kernel, int64_t pad_left, int64_t pad_right)
{
    return std::get<0>(fft_conv_impl(x, kernel, pad_left, pad_right, nullptr));
}

std::tuple<Tensor, Tensor> fft_conv_ep_op(const Tensor &x, const Tensor &kernel, int64_t pad_left, int64_t pad_right, double gain,
                                          bool clamp, int64_t stat_mode, bool per_row)
{
    const EpilogueArgs epa{gain, clamp, stat_mode, per_row};
    return fft_conv_impl(x, kernel, pad_left, pad_right, &epa);
}

// zero-state SOS cascade | FFT-mode FIR as one overlap-save pipeline (tfx_sos_fft_conv_forward): y, the statistic of the
// epilogue and -- on request -- every section's float64 output [K, C, T]
std::tuple<Tensor, Tensor, Tensor> sos_fft_conv_op(const Tensor &x_in, const Tensor &sos_cpu, const Tensor &kernel, int64_t pad_left,
                                                   int64_t pad_right, bool sections, int64_t force_block, double gain, bool clamp,
                                                   int64_t stat_mode, bool per_row)
{
    TORCH_CHECK(x_in.dim() == 2, "sos_fft_conv_forward: x must be [C, T], got ", x_in.sizes());
    need_device(x_in, "x");
    TORCH_CHECK(x_in.scalar_type() == at::kFloat, "sos_fft_conv_forward: float32 signals only, got ", x_in.scalar_type());
    const Tensor x = x_in.contiguous();
    const Tensor sos = host_f64(sos_cpu, 6, "sos_fft_conv_forward");
    TORCH_CHECK(sos.dim() == 2, "sos_fft_conv_forward: sos must be [K, 6]");
    const Tensor k = taps_host(kernel, x);
    const int64_t C = x.size(0), T = x.size(1), K = sos.size(0), taps = k.numel();
    const int64_t tout = T + pad_left + pad_right - taps + 1;
    Tensor y = at::empty({C, tout > 0 ? tout : 0}, x.options()), stat;
    Tensor sec = sections ? at::empty({K, C, T}, x.options().dtype(at::kDouble)) : at::empty({0}, x.options().dtype(at::kDouble));
    const tfx_epilogue ep = make_epilogue({gain, clamp, stat_mode, per_row}, stat, x, C);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_sos_fft_conv_forward(x.data_ptr<float>(), y.data_ptr<float>(), C, T, sos.data_ptr<double>(), K, k.data_ptr<float>(), taps,
                                      pad_left, pad_right, sections ? sec.data_ptr<double>() : nullptr, (int)force_block, &ep,
                                      stream_of(x)),
             "sos_fft_conv_forward");
    return {y, stat, sec};
}

// the apply half of Normalize on a statistic an epilogue left on the device
Tensor normalize_apply_op(const Tensor &x, const Tensor &stat, double peak, int64_t mode, bool per_row)
{
    need_device(x, "x");
    need_device(stat, "stat");
    const Tensor xc = x.contiguous();
    const int64_t T = xc.dim() ? xc.size(-1) : 1, rows = T ? xc.numel() / T : 0;
    TORCH_CHECK(stat.scalar_type() == at::kDouble && stat.numel() == (per_row ? rows : 1), "normalize_apply: stat must be float64 [",
                per_row ? rows : 1, "], got ", stat.sizes(), " ", stat.scalar_type());
    const Tensor st = stat.contiguous();
    Tensor y = at::empty_like(xc);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_normalize_apply(xc.data_ptr(), y.data_ptr(), dtype_code(xc, "normalize_apply"), rows, T, (int)mode, per_row ? 1 : 0,
                                 peak, st.data_ptr<double>(), stream_of(x)),
             "normalize_apply");
    return y;
}

// one chunk of a stateful FIR: history and chunk are read from their two buffers, the new history is returned
std::tuple<Tensor, Tensor> fir_stream_op(const Tensor &x_in, const Tensor &kernel, const OptTensor &hist, bool direct)
{
    TORCH_CHECK(x_in.dim() == 2, "fir_stream_forward: x must be [C, T], got ", x_in.sizes());
    need_device(x_in, "x");
    const Tensor x = x_in.contiguous();
    const Tensor k = taps_host(kernel, x);
    const int64_t C = x.size(0), T = x.size(1), K = k.numel();
    TORCH_CHECK(K >= 1, "fir_stream_forward: empty kernel");
    const Tensor hin = stream_hist_in(hist, x, C, K - 1, "fir_stream_forward");
    Tensor y = at::empty_like(x);
    Tensor hout = at::empty({C, K - 1}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_fir_stream_forward(x.data_ptr(), y.data_ptr(), dtype_code(x, "fir_stream_forward"), C, T, k.data_ptr(), K,
                                    direct ? 1 : 0, hin.defined() ? hin.data_ptr() : nullptr, K > 1 ? hout.data_ptr() : nullptr,
                                    stream_of(x)),
             "fir_stream_forward");
    return {y, hout};
}

// one small streaming chunk through cascade -> stateful direct FIR -> gain / clip in ONE launch (tfx_chunk_forward).
// Returns (y, new_state_x, new_state_y, new_hist); sos_cpu [K, 6] may have K = 0, kernel one tap.
std::tuple<Tensor, Tensor, Tensor, Tensor> chunk_op(const Tensor &x_in, const Tensor &sos_cpu, const OptTensor &state_x,
                                                    const OptTensor &state_y, const Tensor &kernel, const OptTensor &hist,
                                                    double gain, bool scale, bool clamp, int64_t precision)
{
    TORCH_CHECK(x_in.dim() == 2 && x_in.scalar_type() == at::kFloat, "chunk_forward: x must be float32 [C, T], got ", x_in.sizes());
    need_device(x_in, "x");
    // a chunk is usually a column window of a longer buffer: rows with unit stride are taken as they are (row pitch)
    const Tensor x = (x_in.stride(1) == 1 && x_in.stride(0) >= x_in.size(1)) ? x_in : x_in.contiguous();
    const Tensor sos = host_f64(sos_cpu, 6, "chunk_forward");
    TORCH_CHECK(sos.dim() == 2, "chunk_forward: sos must be [K, 6]");
    const Tensor k = taps_host(kernel, x);
    const int64_t C = x.size(0), T = x.size(1), K = sos.size(0), Kf = k.numel();
    TORCH_CHECK(tfx_chunk_supported(C, T, K, Kf), "chunk_forward: unsupported geometry C=", C, " T=", T, " K=", K, " taps=", Kf);
    Tensor kx, ky;
    const double *sx = K ? state_ptr(state_x, {K, C, 2}, x, "state_x", kx) : nullptr;
    const double *sy = K ? state_ptr(state_y, {K, C, 2}, x, "state_y", ky) : nullptr;
    const Tensor hin = stream_hist_in(hist, x, C, Kf - 1, "chunk_forward");
    Tensor y = at::empty({C, T}, x.options());
    Tensor nsx = at::empty({K, C, 2}, x.options().dtype(at::kDouble));
    Tensor nsy = at::empty({K, C, 2}, x.options().dtype(at::kDouble));
    Tensor hout = at::empty({C, Kf - 1}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_chunk_forward(x.data_ptr<float>(), C > 1 ? x.stride(0) : T, y.data_ptr<float>(), C, T, K ? sos.data_ptr<double>() : nullptr, K, sx, sy,
                               K ? nsx.data_ptr<double>() : nullptr, K ? nsy.data_ptr<double>() : nullptr, k.data_ptr<float>(), Kf,
                               hin.defined() ? hin.data_ptr<float>() : nullptr, Kf > 1 ? hout.data_ptr<float>() : nullptr, gain,
                               scale ? 1 : 0, clamp ? 1 : 0, precision_or_default(precision), stream_of(x)),
             "chunk_forward");
    return {y, nsx, nsy, hout};
}

// ---------------------------------------------------------------------------------------------------
// `+` of branch outputs, Gain / Normalize passes, layout kernels
// ---------------------------------------------------------------------------------------------------
Tensor sum_op(at::TensorList tensors)
{
    TORCH_CHECK(!tensors.empty(), "sum_forward: need at least one tensor");
    std::vector<Tensor> ts;
    for (const Tensor &t : tensors) {
        need_device(t, "branch output");
        TORCH_CHECK(t.sizes() == tensors[0].sizes() && t.scalar_type() == tensors[0].scalar_type(),
                    "sum_forward: branch outputs differ in shape or dtype");
        ts.push_back(t.contiguous());
    }
    Tensor out = at::empty_like(ts[0]);
    c10::hip::HIPGuard guard(out.get_device());
    for (size_t i = 0; i < ts.size(); i += 15) {            // the kernel takes up to 16 inputs per launch
        std::vector<const void *> grp;
        if (i > 0) grp.push_back(out.data_ptr());
        for (size_t j = i; j < ts.size() && j < i + 15; ++j) grp.push_back(ts[j].data_ptr());
        check_rc(tfx_sum_forward(grp.data(), (int)grp.size(), out.data_ptr(), dtype_code(out, "sum_forward"), out.numel(),
                                 stream_of(out)),
                 "sum_forward");
    }
    return out;
}

// q-quantile (linear interpolation) of |x| over all elements, float64 [1] on the device: the percentile threshold as a radix select
Tensor quantile_abs_op(const Tensor &x, double q)
{
    need_device(x, "x");
    TORCH_CHECK(x.scalar_type() == at::kFloat, "quantile_abs: float32 signals only (got ", x.scalar_type(), ")");
    TORCH_CHECK(x.numel() >= 1, "quantile_abs: empty input");
    const Tensor xc = x.contiguous();
    Tensor out = at::empty({1}, xc.options().dtype(at::kDouble));
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_quantile_abs(xc.data_ptr<float>(), xc.numel(), q, out.data_ptr<double>(), stream_of(x)), "quantile_abs");
    return out;
}

Tensor gain_op(const Tensor &x, double gain, bool clamp)
{
    need_device(x, "x");
    const Tensor xc = x.contiguous();
    Tensor y = at::empty_like(xc);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_gain_forward(xc.data_ptr(), y.data_ptr(), dtype_code(xc, "gain_forward"), xc.numel(), gain, clamp ? 1 : 0,
                              stream_of(x)),
             "gain_forward");
    return y;
}

Tensor stat_op(const Tensor &x, int64_t mode, bool per_row)
{
    need_device(x, "x");
    const Tensor xc = x.contiguous();
    const int64_t T = xc.dim() ? xc.size(-1) : 1, rows = T ? xc.numel() / T : 0;
    Tensor out = at::empty({per_row ? rows : 1}, x.options().dtype(at::kDouble));
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_stat_forward(xc.data_ptr(), dtype_code(xc, "stat_forward"), rows, T, (int)mode, per_row ? 1 : 0,
                              out.data_ptr<double>(), stream_of(x)),
             "stat_forward");
    return out;
}

Tensor normalize_op(const Tensor &x, double peak, int64_t mode, bool per_row)
{
    need_device(x, "x");
    const Tensor xc = x.contiguous();
    const int64_t T = xc.dim() ? xc.size(-1) : 1, rows = T ? xc.numel() / T : 0;
    Tensor y = at::empty_like(xc);
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_normalize_forward(xc.data_ptr(), y.data_ptr(), dtype_code(xc, "normalize_forward"), rows, T, (int)mode,
                                   per_row ? 1 : 0, peak, stream_of(x)),
             "normalize_forward");
    return y;
}

void deinterleave_into_op(const Tensor &frames, Tensor out, int64_t frame_base, double scale)
{
    need_device(frames, "frames");
    TORCH_CHECK(frames.dim() == 2 && (frames.scalar_type() == at::kFloat || frames.scalar_type() == at::kShort),
                "deinterleave_forward: expected [F, C] float32 or int16, got ", frames.sizes(), " ", frames.scalar_type());
    const Tensor fr = frames.contiguous();
    const int64_t F = fr.size(0), C = fr.size(1);
    TORCH_CHECK(out.dim() == 2 && out.size(0) == C && out.scalar_type() == at::kFloat && out.is_contiguous() &&
                    out.device() == fr.device(),
                "deinterleave_forward: out must be a contiguous float32 [C, F_total] tensor on the same device");
    c10::hip::HIPGuard guard(fr.get_device());
    check_rc(tfx_deinterleave_forward(fr.data_ptr(), fr.scalar_type() == at::kFloat ? 0 : 1, out.data_ptr(), F, C, out.size(1),
                                      frame_base, scale, stream_of(fr)),
             "deinterleave_forward");
}

Tensor deinterleave_op(const Tensor &frames, double scale)
{
    TORCH_CHECK(frames.dim() == 2, "deinterleave_forward: expected [F, C], got ", frames.sizes());
    Tensor out = at::empty({frames.size(1), frames.size(0)}, frames.options().dtype(at::kFloat));
    deinterleave_into_op(frames, out, 0, scale);
    return out;
}

Tensor interleave_op(const Tensor &x, int64_t frame_base, int64_t frames)
{
    need_device(x, "x");
    TORCH_CHECK(x.dim() == 2 && x.scalar_type() == at::kFloat, "interleave_forward: expected float32 [C, F], got ", x.sizes(), " ",
                x.scalar_type());
    const Tensor xc = x.contiguous();
    const int64_t C = xc.size(0), Ft = xc.size(1);
    const int64_t F = frames < 0 ? Ft - frame_base : frames;
    Tensor out = at::empty({F > 0 ? F : 0, C}, x.options());
    c10::hip::HIPGuard guard(x.get_device());
    check_rc(tfx_interleave_forward(xc.data_ptr(), out.data_ptr(), F, C, Ft, frame_base, stream_of(x)), "interleave_forward");
    return out;
}

// ---------------------------------------------------------------------------------------------------
// Meta kernels (shape / dtype inference: torch.compile, fake tensors)
// ---------------------------------------------------------------------------------------------------
std::tuple<Tensor, Tensor, Tensor> sos_meta(const Tensor &x, const Tensor &sos_cpu, const OptTensor &, const OptTensor &,
                                            std::optional<at::ScalarType> out_dtype, int64_t)
{
    const int64_t K = sos_cpu.size(0), C = x.size(0);
    Tensor st = at::empty({K, C, 2}, x.options().dtype(at::kDouble));
    return {at::empty(x.sizes(), x.options().dtype(out_type(x, out_dtype))), st, at::empty_like(st)};
}
std::tuple<Tensor, Tensor, Tensor, Tensor> sos_sections_meta(const Tensor &x, const Tensor &sos_cpu, const OptTensor &a,
                                                             const OptTensor &b, std::optional<at::ScalarType> out_dtype, int64_t p)
{
    auto r = sos_meta(x, sos_cpu, a, b, out_dtype, p);
    return {std::get<0>(r), std::get<1>(r), std::get<2>(r),
            at::empty({sos_cpu.size(0), x.size(0), x.size(1)}, x.options().dtype(out_type(x, out_dtype)))};
}
std::tuple<Tensor, Tensor, Tensor> bank_meta(const Tensor &x, const Tensor &banks, const OptTensor &, const OptTensor &,
                                             std::optional<at::ScalarType> out_dtype, int64_t)
{
    const int64_t NB = banks.size(0), K = banks.size(1), C = x.size(0);
    Tensor st = at::empty({K, NB * C, 2}, x.options().dtype(at::kDouble));
    return {at::empty({NB, C, x.size(1)}, x.options().dtype(out_type(x, out_dtype))), st, at::empty_like(st)};
}
std::tuple<Tensor, Tensor, Tensor> bank_sum_meta(const Tensor &x, const Tensor &banks, const OptTensor &, const OptTensor &, int64_t)
{
    const int64_t NB = banks.size(0), K = banks.size(1), C = x.size(0);
    Tensor st = at::empty({K, NB * C, 2}, x.options().dtype(at::kDouble));
    return {at::empty_like(x), st, at::empty_like(st)};
}
std::tuple<Tensor, Tensor, Tensor> biquad_meta(const Tensor &x, const Tensor &, double, double, const OptTensor &, const OptTensor &,
                                               std::optional<at::ScalarType> out_dtype, int64_t)
{
    Tensor st = at::empty({x.size(0), 2}, x.options().dtype(at::kDouble));
    return {at::empty(x.sizes(), x.options().dtype(out_type(x, out_dtype))), st, at::empty_like(st)};
}
Tensor resample_meta(const Tensor &x, int64_t up, int64_t down, const Tensor &)
{
    return at::empty(resample_shape(x, up, down), x.options());
}
std::tuple<Tensor, Tensor> resample_stream_meta(const Tensor &x, const Tensor &h, const OptTensor &, int64_t up, int64_t down,
                                                int64_t consumed)
{
    const ResampleStreamPlan pl = resample_stream_plan(x, h, up, down, consumed);
    std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
    shape.back() = pl.end - pl.begin;
    return {at::empty(shape, x.options()), at::empty({stream_rows(x), pl.H}, x.options())};
}
Tensor delay_meta(const Tensor &x, int64_t delay_samples, at::ArrayRef<double> amps, double, bool)
{
    return at::empty(delay_shape(x, delay_samples, (int64_t)amps.size()), x.options());
}
std::tuple<Tensor, Tensor> delay_ep_meta(const Tensor &x, int64_t delay_samples, at::ArrayRef<double> amps, double, bool, double, bool,
                                         int64_t stat_mode, bool per_row)
{
    const int64_t T = x.dim() ? x.size(-1) : 1, rows = T > 0 ? x.numel() / T : 0;
    return {at::empty(delay_shape(x, delay_samples, (int64_t)amps.size()), x.options()),
            at::empty({stat_mode >= 0 ? (per_row ? rows : 1) : 0}, x.options().dtype(at::kDouble))};
}
std::tuple<Tensor, Tensor> delay_stream_meta(const Tensor &x, const OptTensor &, int64_t delay_samples, at::ArrayRef<double> amps,
                                             double, bool)
{
    TORCH_CHECK(!amps.empty() && delay_samples >= 0, "delay_stream_forward: bad delay or taps");
    return {at::empty_like(x), at::empty({stream_rows(x), (int64_t)amps.size() * delay_samples}, x.options())};
}
std::tuple<Tensor, Tensor> delay_line_stream_meta(const Tensor &x, const OptTensor &, int64_t delay_samples, double, double)
{
    TORCH_CHECK(delay_samples >= 0, "delay_line_stream_forward: negative delay");
    return {at::empty_like(x), at::empty({stream_rows(x), delay_samples}, x.options())};
}
Tensor fft_conv_meta(const Tensor &x, const Tensor &kernel, int64_t pad_left, int64_t pad_right)
{
    const int64_t tout = x.size(1) + pad_left + pad_right - kernel.numel() + 1;
    return at::empty({x.size(0), tout > 0 ? tout : 0}, x.options());
}

std::tuple<Tensor, Tensor, Tensor> compressor_meta(const Tensor &x, double, double, double, double, double, double, int64_t channels,
                                                   const OptTensor &, bool return_gain, int64_t)
{
    TORCH_CHECK(x.dim() >= 1 && channels >= 1, "compressor_forward: bad shape");
    const int64_t T = x.size(-1), groups = stream_rows(x) / channels;
    return {at::empty_like(x), return_gain ? at::empty({groups, T}, x.options()) : at::empty({0}, x.options()),
            at::empty({groups, 2}, x.options().dtype(at::kDouble))};
}

std::tuple<Tensor, Tensor, Tensor, Tensor> gate_meta(const Tensor &x, double, double, double, int64_t, double, double, int64_t channels,
                                                     const OptTensor &, bool return_gain, bool return_open, int64_t)
{
    TORCH_CHECK(x.dim() >= 1 && channels >= 1, "gate_forward: bad shape");
    const int64_t T = x.size(-1), groups = stream_rows(x) / channels;
    const auto u8 = x.options().dtype(at::kByte);
    return {at::empty_like(x), return_gain ? at::empty({groups, T}, x.options()) : at::empty({0}, x.options()),
            return_open ? at::empty({groups, T}, u8) : at::empty({0}, u8), at::empty({groups, 3}, x.options().dtype(at::kDouble))};
}

Tensor stft_meta(const Tensor &x, const OptTensor &window, int64_t n_fft, int64_t hop, int64_t pad, int64_t, int64_t power, bool)
{
    const StftShape s = stft_shape(x, window, n_fft, hop, pad, power, "stft_forward");
    return at::empty(s.sizes, x.options().dtype(s.dtype)).transpose(-1, -2);
}

std::tuple<Tensor, Tensor> istft_meta(const Tensor &spec, const OptTensor &window, int64_t n_fft, int64_t hop, int64_t pad, int64_t length, bool)
{
    const IstftShape s = istft_shape(spec, window, n_fft, hop, pad, length, "istft_forward");
    return {at::empty(s.sizes, spec.options().dtype(s.dtype)), at::empty({1}, spec.options().dtype(at::kInt))};
}

std::tuple<Tensor, Tensor, Tensor> modulated_delay_stream_meta(const Tensor &x, const OptTensor &, const OptTensor &, const Tensor &voices,
                                                               double, double, int64_t, int64_t)
{
    TORCH_CHECK(x.dim() >= 1 && x.dim() <= 3 && voices.dim() == 2 && voices.size(1) == 5 && voices.size(0) >= 1,
                "modulated_delay_stream_forward: bad shape");
    // the history's length comes from the table's values: H = max_v floor(base_v + depth_v) + 2 (a host tensor holds them even
    // when x is a meta tensor)
    int64_t H = 2;
    if (!voices.is_meta()) {
        const Tensor v = voices.to(at::kCPU, at::kDouble).contiguous();
        for (int64_t i = 0; i < v.size(0); ++i)
            H = std::max<int64_t>(H, (int64_t)std::floor(v.data_ptr<double>()[5 * i] + v.data_ptr<double>()[5 * i + 1]) + 2);
    }
    return {at::empty_like(x), at::empty({stream_rows(x), H}, x.options()), at::empty({1}, x.options().dtype(at::kLong))};
}

std::tuple<Tensor, Tensor> freeverb_meta(const Tensor &x, at::IntArrayRef comb_delays, at::IntArrayRef allpass_delays, double, double,
                                         double, double, double, double, double wet2, int64_t tail, const OptTensor &)
{
    const FreeverbInputs in = freeverb_inputs(x, comb_delays, allpass_delays, wet2, tail, "freeverb_forward");
    return {at::empty(in.yshape, x.options()), at::empty({in.batch * in.channels, in.state_len}, x.options().dtype(at::kDouble))};
}

// No CPU branch, by design: every op of the namespace answers a host tensor with the same error instead of the dispatcher's
// "no kernel for backend CPU" (one boxed function registered for the CPU key of each op; per-namespace fallbacks are not
// supported by the dispatcher).
void no_cpu_boxed(const c10::OperatorHandle &op, c10::DispatchKeySet, torch::jit::Stack *)
{
    TORCH_CHECK(false, "torchfx_amd: ", op.schema().name(),
                ": tensors must live on a ROCm device; this backend has no CPU path -- move them with .to('cuda').");
}

// One line per op: its schema, `fn` for the CUDA key ("CUDA" is the dispatch key of ROCm device tensors) and the refusal above
// for the CPU key.  The op's name is the schema up to its "(".
template <typename F> void reg_op(torch::Library &m, const char *schema, F *fn)
{
    const std::string s(schema), name = s.substr(0, s.find('('));
    m.def(schema);
    m.impl(name.c_str(), torch::dispatch(c10::DispatchKey::CUDA, fn));
    m.impl(name.c_str(), torch::dispatch(c10::DispatchKey::CPU, torch::CppFunction::makeFromBoxedFunction<&no_cpu_boxed>()));
}

}  // namespace

TORCH_LIBRARY(torchfx_hip, m)
{
    reg_op(m, "sos_forward(Tensor x, Tensor sos_cpu, Tensor? state_x=None, Tensor? state_y=None, *, ScalarType? out_dtype=None, "
              "int precision=-1) -> (Tensor, Tensor, Tensor)", sos_op);
    reg_op(m, "sos_forward_sections(Tensor x, Tensor sos_cpu, Tensor? state_x=None, Tensor? state_y=None, *, ScalarType? out_dtype=None, "
              "int precision=-1) -> (Tensor, Tensor, Tensor, Tensor)", sos_sections_op);
    reg_op(m, "sos_bank_forward(Tensor x, Tensor sos_banks_cpu, Tensor? state_x=None, Tensor? state_y=None, *, ScalarType? out_dtype=None, "
              "int precision=-1) -> (Tensor, Tensor, Tensor)", bank_op);
    reg_op(m, "sos_bank_sum_forward(Tensor x, Tensor sos_banks_cpu, Tensor? state_x=None, Tensor? state_y=None, *, int precision=-1) "
              "-> (Tensor, Tensor, Tensor)", bank_sum_op);
    reg_op(m, "biquad_forward(Tensor x, Tensor b, float a1, float a2, Tensor? state_x=None, Tensor? state_y=None, *, "
              "ScalarType? out_dtype=None, int precision=-1) -> (Tensor, Tensor, Tensor)", biquad_op);
    reg_op(m, "delay_line_forward(Tensor(a) x, int delay_samples, float decay, float mix) -> Tensor(a)", delay_line_op);
    reg_op(m, "delay_forward(Tensor x, int delay_samples, float[] amps, float mix, bool pingpong) -> Tensor", delay_op);
    reg_op(m, "resample_forward(Tensor x, int up, int down, Tensor h) -> Tensor", resample_op);
    reg_op(m, "sos_filtfilt(Tensor x, Tensor sos_cpu, int padtype=0, int padlen=-1) -> Tensor", sos_filtfilt_op);
    reg_op(m, "sos_block_energy(Tensor x, Tensor sos_cpu, int num, int den=1) -> Tensor", sos_block_energy_op);
    reg_op(m, "true_peak(Tensor x, Tensor taps_cpu, int up) -> Tensor", true_peak_op);
    reg_op(m, "limiter_forward(Tensor x, float c, int A, int H, Tensor window_cpu, int up, Tensor? taps_cpu, int channels, "
              "bool return_gain) -> (Tensor, Tensor)", limiter_op);
    reg_op(m, "limiter_stream_forward(Tensor x, Tensor? hist, int consumed, float c, int A, int H, Tensor window_cpu, int up, "
              "Tensor? taps_cpu, int channels, bool return_gain, int n_in=-1) -> (Tensor, Tensor, Tensor)", limiter_stream_op);
    reg_op(m, "resample_stream_forward(Tensor x, Tensor h, Tensor? hist, int up, int down, int consumed) -> (Tensor, Tensor)",
           resample_stream_op);
    reg_op(m, "delay_forward_ep(Tensor x, int delay_samples, float[] amps, float mix, bool pingpong, float gain, bool clamp, int stat_mode, "
              "bool per_row) -> (Tensor, Tensor)", delay_ep_op);
    reg_op(m, "delay_stream_forward(Tensor x, Tensor? hist, int delay_samples, float[] amps, float mix, bool pingpong) -> (Tensor, Tensor)",
           delay_stream_op);
    reg_op(m, "delay_line_stream_forward(Tensor x, Tensor? hist, int delay_samples, float decay, float mix) -> (Tensor, Tensor)",
           delay_line_stream_op);
    reg_op(m, "fir_direct_forward(Tensor x, Tensor kernel) -> Tensor", fir_direct_op);
    reg_op(m, "fft_conv_forward(Tensor x, Tensor kernel, int pad_left, int pad_right) -> Tensor", fft_conv_op);
    reg_op(m, "fir_stream_forward(Tensor x, Tensor kernel, Tensor? hist, bool direct) -> (Tensor, Tensor)", fir_stream_op);
    reg_op(m, "chunk_forward(Tensor x, Tensor sos_cpu, Tensor? state_x, Tensor? state_y, Tensor kernel, Tensor? hist, float gain, "
              "bool scale, bool clamp, int precision=-1) -> (Tensor, Tensor, Tensor, Tensor)", chunk_op);
    reg_op(m, "sos_forward_ep(Tensor x, Tensor sos_cpu, Tensor? state_x, Tensor? state_y, float gain, bool clamp, int stat_mode, "
              "bool per_row, *, ScalarType? out_dtype=None, int precision=-1) -> (Tensor, Tensor, Tensor, Tensor)", sos_ep_op);
    reg_op(m, "fft_conv_forward_ep(Tensor x, Tensor kernel, int pad_left, int pad_right, float gain, bool clamp, int stat_mode, "
              "bool per_row) -> (Tensor, Tensor)", fft_conv_ep_op);
    reg_op(m, "sos_fft_conv_forward(Tensor x, Tensor sos_cpu, Tensor kernel, int pad_left, int pad_right, bool sections=False, "
              "int force_block=0, float gain=1.0, bool clamp=False, int stat_mode=-1, bool per_row=False) -> (Tensor, Tensor, Tensor)",
           sos_fft_conv_op);
    reg_op(m, "normalize_apply(Tensor x, Tensor stat, float peak, int mode, bool per_row) -> Tensor", normalize_apply_op);
    reg_op(m, "sum_forward(Tensor[] tensors) -> Tensor", sum_op);
    reg_op(m, "gain_forward(Tensor x, float gain, bool clamp) -> Tensor", gain_op);
    reg_op(m, "quantile_abs(Tensor x, float q) -> Tensor", quantile_abs_op);
    reg_op(m, "stat_forward(Tensor x, int mode, bool per_row) -> Tensor", stat_op);
    reg_op(m, "normalize_forward(Tensor x, float peak, int mode, bool per_row) -> Tensor", normalize_op);
    reg_op(m, "deinterleave_forward(Tensor frames, float scale=3.0517578125e-05) -> Tensor", deinterleave_op);
    reg_op(m, "deinterleave_into(Tensor frames, Tensor(a!) out, int frame_base=0, float scale=3.0517578125e-05) -> ()", deinterleave_into_op);
    reg_op(m, "interleave_forward(Tensor x, int frame_base=0, int frames=-1) -> Tensor", interleave_op);
}

TORCH_LIBRARY_IMPL(torchfx_hip, Meta, m)
{
    m.impl("sos_forward", sos_meta);
    m.impl("sos_forward_sections", sos_sections_meta);
    m.impl("sos_bank_forward", bank_meta);
    m.impl("sos_bank_sum_forward", bank_sum_meta);
    m.impl("biquad_forward", biquad_meta);
    m.impl("fir_direct_forward", [](const Tensor &x, const Tensor &) { return at::empty_like(x); });
    m.impl("fft_conv_forward", fft_conv_meta);
    m.impl("delay_forward", delay_meta);
    m.impl("resample_forward", resample_meta);
    m.impl("sos_filtfilt", [](const Tensor &x, const Tensor &, int64_t, int64_t) { return at::empty_like(x); });
    m.impl("sos_block_energy", [](const Tensor &x, const Tensor &sos, int64_t num, int64_t den) {
        return at::empty(sos_block_energy_shape(x, sos, num, den), x.options().dtype(at::kDouble));
    });
    m.impl("true_peak", [](const Tensor &x, const Tensor &, int64_t) { return at::empty(true_peak_shape(x), x.options()); });
    m.impl("resample_stream_forward", resample_stream_meta);
    m.impl("delay_forward_ep", delay_ep_meta);
    m.impl("delay_stream_forward", delay_stream_meta);
    m.impl("delay_line_stream_forward", delay_line_stream_meta);
    m.impl("fir_stream_forward", [](const Tensor &x, const Tensor &kernel, const OptTensor &, bool) {
        return std::make_tuple(at::empty_like(x), at::empty({x.size(0), kernel.numel() - 1}, x.options()));
    });
    m.impl("gain_forward", [](const Tensor &x, double, bool) { return at::empty_like(x); });
    m.impl("normalize_forward", [](const Tensor &x, double, int64_t, bool) { return at::empty_like(x); });
}

// The dynamics processors live in a namespace of their own (torch.ops.torchfx_dynamics), registered the same way: the device
// kernel for the CUDA key, the "no CPU path" refusal for the CPU key, shape inference for Meta.
TORCH_LIBRARY(torchfx_dynamics, m)
{
    reg_op(m, "compressor_forward(Tensor x, float th, float s, float w, float alpha_a, float alpha_r, float makeup_db, int channels, "
              "Tensor? state, bool return_gain, int segments=0) -> (Tensor, Tensor, Tensor)", compressor_op);
}

TORCH_LIBRARY_IMPL(torchfx_dynamics, Meta, m)
{
    m.impl("compressor_forward", compressor_meta);
}

// The modulation effects (Chorus, Flanger, Vibrato) likewise: torch.ops.torchfx_modulation.
TORCH_LIBRARY(torchfx_modulation, m)
{
    reg_op(m, "modulated_delay_forward(Tensor x, Tensor voices_cpu, float spread, float dry, int shape, int interp, int position=0) "
              "-> Tensor", modulated_delay_op);
    reg_op(m, "modulated_delay_stream_forward(Tensor x, Tensor? hist, Tensor? pos, Tensor voices_cpu, float spread, float dry, "
              "int shape, int interp) -> (Tensor, Tensor, Tensor)", modulated_delay_stream_op);
}

TORCH_LIBRARY_IMPL(torchfx_modulation, Meta, m)
{
    m.impl("modulated_delay_forward", [](const Tensor &x, const Tensor &, double, double, int64_t, int64_t, int64_t) {
        return at::empty_like(x);
    });
    m.impl("modulated_delay_stream_forward", modulated_delay_stream_meta);
}

// Freeverb likewise: torch.ops.torchfx_reverb.
TORCH_LIBRARY(torchfx_reverb, m)
{
    reg_op(m, "freeverb_forward(Tensor x, int[] comb_delays, int[] allpass_delays, float feedback, float damp, float allpass_gain, "
              "float input_gain, float dry_gain, float wet1, float wet2, int tail=0, Tensor? state=None) -> (Tensor, Tensor)",
           freeverb_op);
}

TORCH_LIBRARY_IMPL(torchfx_reverb, Meta, m)
{
    m.impl("freeverb_forward", freeverb_meta);
}

// The phaser likewise: torch.ops.torchfx_phaser.
TORCH_LIBRARY(torchfx_phaser, m)
{
    reg_op(m, "phaser_forward(Tensor x, int stages, float fs, float rate, float min_freq, float max_freq, float phase, float spread, "
              "float dry, float wet, int shape, int position=0, Tensor? pos=None, Tensor? state=None, bool return_coef=False, "
              "int segments=0) -> (Tensor, Tensor, Tensor, Tensor)", phaser_op);
}

TORCH_LIBRARY_IMPL(torchfx_phaser, Meta, m)
{
    m.impl("phaser_forward", phaser_meta);
}

// The gate likewise: torch.ops.torchfx_gate.
TORCH_LIBRARY(torchfx_gate, m)
{
    reg_op(m, "gate_forward(Tensor x, float p_open, float p_close, float range, int hold, float alpha_a, float alpha_r, int channels, "
              "Tensor? state, bool return_gain, bool return_open, int segments=0) -> (Tensor, Tensor, Tensor, Tensor)", gate_op);
}

TORCH_LIBRARY_IMPL(torchfx_gate, Meta, m)
{
    m.impl("gate_forward", gate_meta);
}

// The short-time Fourier transform likewise: torch.ops.torchfx_spectral.
TORCH_LIBRARY(torchfx_spectral, m)
{
    reg_op(m, "stft_forward(Tensor x, Tensor? window, int n_fft, int hop, int pad, int pad_mode, int power, bool normalized) -> Tensor",
           stft_op);
}

TORCH_LIBRARY_IMPL(torchfx_spectral, Meta, m)
{
    m.impl("stft_forward", stft_meta);
}

// Its inverse in a namespace of its own: torch.ops.torchfx_spectral_inverse.
TORCH_LIBRARY(torchfx_spectral_inverse, m)
{
    reg_op(m, "istft_forward(Tensor spec, Tensor? window, int n_fft, int hop, int pad, int length, bool normalized) -> (Tensor, Tensor)",
           istft_op);
}

TORCH_LIBRARY_IMPL(torchfx_spectral_inverse, Meta, m)
{
    m.impl("istft_forward", istft_meta);
}

// The waveshaper likewise: torch.ops.torchfx_shaper.
TORCH_LIBRARY(torchfx_shaper, m)
{
    reg_op(m, "waveshaper_forward(Tensor x, int oversample, int shape, Tensor? curve_cpu, float drive, float bias, float dry, float wet, "
              "Tensor? taps_up_cpu, Tensor? taps_dn_cpu) -> Tensor", waveshaper_op);
}

TORCH_LIBRARY_IMPL(torchfx_shaper, Meta, m)
{
    m.impl("waveshaper_forward", [](const Tensor &x, int64_t, int64_t, const OptTensor &, double, double, double, double, const OptTensor &,
                                    const OptTensor &) { return at::empty_like(x); });
}

// Its stream form in a namespace of its own: torch.ops.torchfx_shaper_stream.
TORCH_LIBRARY(torchfx_shaper_stream, m)
{
    reg_op(m, "waveshaper_stream_forward(Tensor x, Tensor? hist, int consumed, int oversample, int shape, Tensor? curve_cpu, float drive, "
              "float bias, float dry, float wet, Tensor? taps_up_cpu, Tensor? taps_dn_cpu, int n_in=-1) -> (Tensor, Tensor)",
           waveshaper_stream_op);
}

TORCH_LIBRARY_IMPL(torchfx_shaper_stream, Meta, m)
{
    // the history's length is the plan's (host-only: it reads the sizes alone)
    m.impl("waveshaper_stream_forward", [](const Tensor &x, const OptTensor &, int64_t, int64_t oversample, int64_t, const OptTensor &curve,
                                           double, double, double, double, const OptTensor &taps_up, const OptTensor &taps_dn, int64_t) {
        const char *what = "waveshaper_stream_forward";
        const auto count = [](const OptTensor &t) { return t.has_value() && t->defined() ? t->numel() : (int64_t)0; };
        const int64_t rows = stream_rows(x);
        int64_t info[6];
        check_rc(tfx_waveshaper_stream_plan_info(rows, x.size(-1), oversample, oversample == 1 ? 0 : count(taps_up),
                                                 oversample == 1 ? 0 : count(taps_dn), count(curve), dtype_code(x, what), info,
                                                 info + 1, info + 2, info + 3, info + 4, info + 5),
                 what);
        return std::make_tuple(at::empty_like(x), at::empty({rows, info[1]}, x.options()));
    });
}

// The reference's module surface (binding.cpp:83-96): exactly these three names and argument lists.
PYBIND11_MODULE(torchfx_ext, m)
{
    m.doc() = "torchfx native extension for MI355X (HIP kernels behind the reference's torchfx_ext interface)";
    m.def("biquad_forward",
          [](const Tensor &x, const Tensor &b, double a1, double a2, const OptTensor &state_x, const OptTensor &state_y) {
              if (!x.is_cuda()) return host::biquad_forward(x, b, a1, a2, state_x, state_y);      // binding.cpp:30-50 dispatches the same way
              return biquad_op(x, b, a1, a2, state_x, state_y, std::nullopt, -1);
          },
          "Biquad forward pass (x, b, a1, a2, state_x, state_y) -> (y, new_state_x, new_state_y)", py::arg("x"), py::arg("b"),
          py::arg("a1"), py::arg("a2"), py::arg("state_x"), py::arg("state_y"));
    m.def("sos_forward",
          [](const Tensor &x, const OptTensor &sos, const Tensor &sos_cpu, const OptTensor &state_x, const OptTensor &state_y) {
              // host tensors: binding.cpp:52-66 hands `sos` (the 2nd argument) to sos_forward_cpu; `sos_cpu` only when it is absent
              if (!x.is_cuda()) return host::sos_forward(x, (sos.has_value() && sos->defined() && !sos->is_cuda()) ? *sos : sos_cpu, state_x, state_y);
              // device tensors: `sos` is the reference's device copy of the coefficients (its sync-avoidance argument), unused here
              return sos_op(x, sos_cpu, state_x, state_y, std::nullopt, -1);
          },
          "SOS cascade forward pass (x, sos, sos_cpu, state_x, state_y) -> (y, new_state_x, new_state_y)", py::arg("x"),
          py::arg("sos"), py::arg("sos_cpu"), py::arg("state_x"), py::arg("state_y"));
    m.def("delay_line_forward",
          [](const Tensor &x, int64_t delay_samples, double decay, double mix) {
              if (!x.is_cuda()) return host::delay_line_forward(x, delay_samples, decay, mix);    // binding.cpp:68-81
              return delay_line_op(x, delay_samples, decay, mix);
          },
          "Delay line forward pass (x, delay_samples, decay, mix) -> y", py::arg("x"), py::arg("delay_samples"), py::arg("decay"),
          py::arg("mix"));
}
