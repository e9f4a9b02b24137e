"""The C-ABI library loads on a machine without a GPU and exports exactly what
include/torchfx_hip.h declares (no compute calls here)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "torchfx_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tfx_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_hot_path():
    syms = declared_symbols()
    for need in ("tfx_sos_forward", "tfx_biquad_forward", "tfx_fir_direct_forward",
                 "tfx_fft_conv_forward", "tfx_delay_line_forward", "tfx_sum_forward", "tfx_effects_plan_info"):
        assert need in syms


def test_library_exports_every_declared_symbol():
    from torchfx_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(lib, s), f"{s} declared in the header but not exported"
    assert lib.tfx_version() >= 100


def test_python_binding_table_matches_header():
    from torchfx_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    _lib.load()     # sets restype/argtypes for all of them; raises on any mismatch


def test_only_extern_c_tfx_symbols_are_public_entry_points():
    from torchfx_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported_c = sorted({ln.split()[-1] for ln in out.splitlines() if " T tfx_" in ln})
    assert exported_c == declared_symbols()


def test_plan_info_runs_without_gpu():
    import numpy as np
    from scipy.signal import butter
    from torchfx_amd import torchfx_ext as E
    info = E.sos_plan_info(butter(4, 0.1, output="sos"))
    assert 100 < info["warmup"] < 2000 and info["f32_error_bound"] > 0
    # pure delay-free FIR section: memory of exactly two samples
    assert E.sos_plan_info(np.array([[1.0, 0.5, 0.25, 1, 0, 0]]))["warmup"] < 32
    # marginally stable integrator never decays
    assert E.sos_plan_info(np.array([[1.0, 0, 0, 1, -1.0, 0]]))["warmup"] == -1
    # the elementwise effects' geometry: 16-byte vectors, 256 threads, 8 tiles per reduce workgroup
    assert E.effects_plan_info(3 * 8192 + 1) == dict(vec=4, tile=1024, group=8192, groups=4, finish_threads=1024, stream_tile=1024)


def test_errors_without_device_are_loud():
    import pytest
    import torch
    from torchfx_amd import torchfx_ext as E
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.sos_forward(torch.zeros(1, 8), None, torch.tensor([[1., 0, 0, 1, 0, 0]]), None, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.fir_direct_forward(torch.zeros(1, 8), torch.ones(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.fft_conv_forward(torch.zeros(1, 8), torch.ones(3), (2, 0))


def test_custom_ops_registered_with_meta_and_no_cpu_kernel():
    import pytest
    import torch
    import torchfx_amd.ops  # noqa: F401
    x = torch.empty(3, 100, device="meta")
    y, sx, sy = torch.ops.torchfx_hip.sos_forward(x, torch.empty(2, 6, dtype=torch.float64), None, None)
    assert y.shape == (3, 100) and sx.shape == (2, 3, 2) and sx.dtype == torch.float64
    assert torch.ops.torchfx_hip.fft_conv_forward(x, torch.empty(8), 7, 0).shape == (3, 100)
    with pytest.raises(RuntimeError, match="no CPU path"):          # there is deliberately no CPU implementation
        torch.ops.torchfx_hip.fir_direct_forward(torch.zeros(1, 8), torch.ones(3))


TORCH_OPS = {
    "sos_forward", "sos_forward_sections", "sos_bank_forward", "sos_bank_sum_forward", "biquad_forward", "delay_line_forward",
    "delay_forward", "resample_forward", "sos_filtfilt", "sos_block_energy", "true_peak", "limiter_forward",
    "limiter_stream_forward", "resample_stream_forward", "delay_forward_ep", "delay_stream_forward", "delay_line_stream_forward",
    "fir_direct_forward", "fft_conv_forward", "fir_stream_forward", "chunk_forward", "sos_forward_ep", "fft_conv_forward_ep",
    "sos_fft_conv_forward", "normalize_apply", "sum_forward", "gain_forward", "quantile_abs", "stat_forward", "normalize_forward",
    "deinterleave_forward", "deinterleave_into", "interleave_forward",
}


def test_every_op_of_the_namespace_has_a_device_kernel_and_a_cpu_refusal():
    """The 33 ops of ``torchfx_hip`` and nothing else; each one is registered for the CUDA key (its kernel) and for the CPU key
    (the "no CPU path" error), so no op can be defined without either."""
    import torch
    import torchfx_amd.ops  # noqa: F401
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_hip::")}
    assert len(TORCH_OPS) == 33
    assert names == {"torchfx_hip::" + n for n in TORCH_OPS}
    for name in sorted(names):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA"), name
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CPU"), name
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.torchfx_hip.interleave_forward(torch.zeros(2, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.torchfx_hip.resample_forward(torch.zeros(1, 8), 2, 1, torch.ones(5))


def test_compiled_module_has_the_reference_surface():
    """`torchfx_ext` (pybind) exposes exactly the names of src/torchfx/_csrc/binding.cpp:83-96 with the same
    argument lists (tests/test_ops_dispatch.py:29-35 of the reference asserts the three attributes)."""
    import inspect

    from torchfx_amd import native
    m = native.load()
    assert sorted(n for n in dir(m) if not n.startswith("_")) == ["biquad_forward", "delay_line_forward", "sos_forward"]
    import re

    def argnames(fn):          # pybind11 puts the signature on the first line of the docstring
        return re.findall(r"(\w+): ", fn.__doc__.splitlines()[0])
    assert argnames(m.biquad_forward) == ["x", "b", "a1", "a2", "state_x", "state_y"]            # binding.cpp:84-87
    assert argnames(m.sos_forward) == ["x", "sos", "sos_cpu", "state_x", "state_y"]              # binding.cpp:88-91
    assert argnames(m.delay_line_forward) == ["x", "delay_samples", "decay", "mix"]              # binding.cpp:92-95
    import torch
    names = set(dir(torch.ops.torchfx_hip)) | {n for n in ("sos_forward", "biquad_forward", "delay_line_forward", "fir_direct_forward",
                                                           "fft_conv_forward", "sos_bank_forward", "sos_bank_sum_forward", "sum_forward",
                                                           "gain_forward", "stat_forward", "normalize_forward", "deinterleave_forward",
                                                           "interleave_forward") if hasattr(torch.ops.torchfx_hip, n)}
    assert {"sos_forward", "biquad_forward", "delay_line_forward", "fir_direct_forward", "fft_conv_forward", "sum_forward",
            "gain_forward", "normalize_forward"} <= names
    assert inspect.ismodule(m)


def test_bad_arguments_are_errors_not_crashes():
    """Null pointers / negative sizes come back as rc != 0 with a message (host-side checks, no GPU
    needed: every entry point validates before it touches the device)."""
    import ctypes

    from torchfx_amd import _lib
    lib = _lib.load()
    sos = (ctypes.c_double * 6)(1, 0, 0, 1, 0, 0)
    cases = [
        lib.tfx_sos_forward(None, 0, None, 0, 2, 100, sos, 1, None, None, None, None, None, 2, None),
        lib.tfx_sos_forward(None, 0, None, 0, -1, 100, sos, 1, None, None, None, None, None, 2, None),
        lib.tfx_sos_forward(None, 7, None, 0, 2, 100, sos, 1, None, None, None, None, None, 2, None),
        lib.tfx_fir_direct_forward(None, None, 0, 2, 100, None, 5, None),
        lib.tfx_fft_conv_forward(None, None, 0, 2, 100, None, 5, 4, 0, None),
        lib.tfx_fft_conv_forward(None, None, 0, 2, 3, None, 50, 0, 0, None),
        lib.tfx_gain_forward(None, None, 0, 10, 1.0, 0, None),
        lib.tfx_stat_forward(None, 0, 2, 10, 0, 0, None, None),
        lib.tfx_normalize_forward(None, None, 0, 2, 10, 3, 0, 1.0, None),
        lib.tfx_delay_line_forward(None, None, 0, 2, 10, 3, 0.5, 0.5, None),
        lib.tfx_deinterleave_forward(None, 0, None, 10, 2, 10, 0, 1.0, None),
        lib.tfx_deinterleave_forward(None, 5, None, 10, 2, 10, 0, 1.0, None),
        lib.tfx_interleave_forward(None, None, 10, 0, 10, 0, None),
        lib.tfx_sum_forward(None, 2, None, 0, 10, None),
    ]
    assert all(rc != 0 for rc in cases), cases
    assert lib.tfx_fft_conv_forward(None, None, 0, 2, 3, None, 50, 0, 0, None) != 0
    assert "kernel size" in lib.tfx_last_error().decode()                 # the reference's wording, _fftconv.py:111-115
    # empty work is fine and touches nothing
    assert lib.tfx_gain_forward(None, None, 0, 0, 1.0, 0, None) == 0
    assert lib.tfx_sos_forward(None, 0, None, 0, 0, 100, sos, 1, None, None, None, None, None, 2, None) == 0


def _build_c_host(tmp_path, with_hip=False):
    """examples/c_host.c: a plain-C99 host of the C ABI, compiled with gcc against include/torchfx_hip.h."""
    from torchfx_amd import _lib
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "c_host")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    if with_hip:
        cmd += ["-DWITH_HIP", "-I", "/opt/rocm/include"]
    cmd += [os.path.join(ROOT, "examples", "c_host.c"), "-L", libdir, "-ltorchfx_hip", f"-Wl,-rpath,{libdir}"]
    if with_hip:
        cmd += ["-L", "/opt/rocm/lib", "-lamdhip64"]
    cmd += ["-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_fir_and_chunk_streams_refuse_overlapping_buffers_before_the_device():
    """The stream-history buffer rule (torchfx_hip.h, "Stream history") holds for tfx_fir_stream_forward and
    tfx_chunk_forward as for the other streams: refused before any launch, so no device is needed to see it."""
    from torchfx_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 512)()
    at = lambda k: ctypes.c_void_p(ctypes.addressof(buf) + 4 * k)    # noqa: E731
    taps = (ctypes.c_float * 33)(*([1.0 / 33] * 33))
    # C = 2 rows; (T, taps, x, y, hist_in, hist_out, x_pitch), offsets in floats; H = taps - 1
    cases = {
        "aliased histories": (8, 5, 0, 16, 32, 32, 0),                   # x [0, 16), y [16, 32), hist_in [32, 40)
        "overlapping histories": (8, 5, 0, 16, 32, 36, 0),
        "hist_out inside y": (8, 5, 0, 16, 32, 20, 0),
        "y inside hist_in": (8, 33, 0, 20, 16, 100, 0),                  # hist_in [16, 80), y [20, 36)
        "y = x": (8, 5, 0, 0, 32, 40, 0),
        "hist_out overlaps x": (8, 5, 0, 16, 32, 8, 0),
        "y overlaps the pitched x": (8, 5, 0, 20, 40, 50, 20),          # x rows [0, 8) and [20, 28)
    }
    for what, (T, K, x, y, hin, hout, pitch) in cases.items():
        own = "own buffer" if "histories" in what else "may not overlap"
        if not pitch:
            assert lib.tfx_fir_stream_forward(at(x), at(y), 0, 2, T, taps, K, 1, at(hin), at(hout), None) != 0, what
            err = lib.tfx_last_error()
            assert b"fir_stream_forward" in err and own.encode() in err, (what, err)
        assert lib.tfx_chunk_forward(at(x), pitch, at(y), 2, T, None, 0, None, None, None, None, taps, K, at(hin), at(hout),
                                     1.0, 0, 0, 0, None) != 0, what
        err = lib.tfx_last_error()
        assert b"chunk_forward" in err and own.encode() in err, (what, err)


def test_plain_c_host_builds_and_runs_without_a_gpu(tmp_path):
    exe = _build_c_host(tmp_path)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "tfx_version" in out and "overlap-save plan: N 1048576" in out
    assert "workspace allocator installed; held now 0 bytes (0 calls" in out
    assert "fused cascade|FIR plan: served 1 block 2097152" in out and "28800001-sample rows served 1" in out      # any row length since round 6 (row_shift)
    assert "null pointer ->" in out            # error code + message instead of a crash


def test_reference_package_binds_to_our_compiled_module():
    """Build container only (skipped where /root/reference is absent, i.e. on the GPU box): the REAL reference package is
    imported with our compiled module installed as `torchfx.torchfx_ext`; `torchfx._ops` binds to it and the reference's own
    call paths (`_ops.*`, `IIR.forward`, `Wave | iir | iir`) COMPUTE through our C++ on host tensors and reproduce the
    reference's fixtures -- cfg 1 of BASELINE.json bit for bit (oracle/check_reference_binding.py)."""
    import os
    import subprocess
    import sys
    if not os.path.isdir("/root/reference/src"):
        pytest.skip("needs /root/reference (build container)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "oracle", "check_reference_binding.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "check_reference_binding: ok" in r.stdout and r.stdout.count("bit-identical to the reference fixture") == 2


def test_no_kernel_spills_registers_to_scratch():
    """Spilled registers are HBM traffic no bandwidth model shows (round 4: PMC found 138 MB each way per call under the 8192-point
    overlap-save kernel and 46 MB of writes under the direct FIR).  The build keeps the compiler's per-kernel resource report
    (`torchfx_amd/csrc/build/<file>.rpass`, Makefile); every kernel must report ScratchSize 0 except the ones listed here."""
    import glob
    import re
    allowed = {"ols_lds16k_kernel"}           # 1024-thread 16 384-point transform: rows shorter than 65 536 samples only (22 us calls)
    reports = sorted(glob.glob(os.path.join(ROOT, "torchfx_amd", "csrc", "build", "*.rpass")))
    if not reports:
        pytest.skip("no compiler resource reports (library not built by this Makefile)")
    seen, bad = 0, []
    for path in reports:
        name = None
        for line in open(path, encoding="utf-8", errors="replace"):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and name:
                seen += 1
                if int(m.group(1)) > 0 and not any(a in name for a in allowed):
                    bad.append((os.path.basename(path), name[:90], int(m.group(1))))
    assert seen > 50, f"only {seen} kernels in the reports"
    assert not bad, f"kernels with scratch memory: {bad}"


def test_tuning_knobs_are_read_once_per_process_and_reloadable():
    """the library reads its TFX_* knobs ONCE per process (a dispatch asks for about ten of them); a host that
    changes one at run time calls `tfx_env_reload()` -- or sets TFX_ENV_DYNAMIC=1 before the first call, which this test
    suite does (tests/conftest.py).  Checked in a fresh process without that switch, on a host-only planning query."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import os, sys\n"
        "sys.path.insert(0, %r)\n"
        "os.environ.pop('TFX_ENV_DYNAMIC', None); os.environ.pop('TFX_FFT_LOG2N', None)\n"
        "from torchfx_amd import _lib, torchfx_ext as E\n"
        "lib = _lib.load()\n"
        "n = lambda: E.ols_plan_info(66559, 28_800_000, (66558, 0))['N']\n"
        "a = n()\n"
        "os.environ['TFX_FFT_LOG2N'] = '18'\n"
        "b = n()\n"
        "lib.tfx_env_reload()\n"
        "c = n()\n"
        "os.environ['TFX_ENV_DYNAMIC'] = '1'; os.environ['TFX_FFT_LOG2N'] = '20'\n"
        "d0 = n()\n"
        "lib.tfx_env_reload()\n"
        "os.environ['TFX_FFT_LOG2N'] = '18'\n"
        "d1 = n()\n"
        "print(a, b, c, d0, d1)\n" % root)
    env = {k: v for k, v in os.environ.items() if k not in ("TFX_ENV_DYNAMIC", "TFX_FFT_LOG2N")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b, c, d0, d1 = (int(v) for v in r.stdout.split()[-5:])
    assert a == 1 << 20 and b == 1 << 20          # the second lookup comes from the table, not from the environment
    assert c == 1 << 18                           # ... until the host asks for a reload
    assert d0 == 1 << 18 and d1 == 1 << 18        # the dynamic switch itself is read at reload; then every lookup is fresh


# switches retired in favour of the constant they defaulted to: no source may read or offer them again
RETIRED_KNOBS = (
    "TFX_SOS_NT", "TFX_SOS_FAIR", "TFX_SOS_WAVES_PER_CU", "TFX_SOS_WARM_ROUND", "TFX_SOS_MIN_SEG_OVER_WARM", "TFX_SOS_UNIT_B0",
    "TFX_FIR_NJ", "TFX_OLS_NT", "TFX_OLS_LDS_NT", "TFX_OLS_ROWMAP", "TFX_OLS_ALIGN", "TFX_OLS_NATIVE_MIN_K",
    "TFX_OLS_N18_MINK", "TFX_OLS_N20_MINK", "TFX_OLS_N21", "TFX_OLS_SOS", "TFX_OLS_SOS_MAXWARM", "TFX_OLS_SOS_N21",
    "TFX_OLS_SOS_HALO_BITS", "TFX_OLS_SOS_UNIT_B0", "TFX_OLS_GPU_SPECTRUM", "TFX_OLS_TRACE", "TFX_OLS_LDS16K_MINK",
    "TFX_OLS_LDS16K_GRID",
)


def test_every_environment_knob_the_library_reads_is_documented():
    """The TFX_* variables the native library reads (env_i64 / getenv under torchfx_amd/csrc) are exactly the ones
    INTEGRATION.md section 5 names, and no retired switch is left anywhere in the library's sources or header."""
    read = set()
    for dirpath, _, files in os.walk(os.path.join(ROOT, "torchfx_amd", "csrc")):
        for f in files:
            if f.endswith((".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                read |= set(re.findall(r'\b(?:env_i64|getenv)\s*\(\s*"(TFX_[A-Z0-9_]+)"', src))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = re.search(r"^## 5\..*?(?=^## |\Z)", doc, flags=re.M | re.S).group(0)
    documented = set(re.findall(r"\b(TFX_[A-Z0-9_]+)", section))
    assert len(read) > 10, sorted(read)
    assert read == documented, f"read, not documented: {sorted(read - documented)}; documented, not read: {sorted(documented - read)}"
    pattern = re.compile(r"\b(%s)\b" % "|".join(RETIRED_KNOBS))
    left = []
    for top in ("torchfx_amd", "include"):
        for dirpath, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [d for d in dirs if d not in ("build", "__pycache__")]
            for f in files:
                if f.endswith((".hip", ".h", ".cpp", ".py", ".md", ".txt")):
                    path = os.path.join(dirpath, f)
                    left += ["%s: %s" % (os.path.relpath(path, ROOT), m) for m in pattern.findall(open(path).read())]
    assert not left, left


def _plan_info(lib, sos):
    a = np.ascontiguousarray(sos, dtype=np.float64)
    prec, warm, bound = ctypes.c_int(), ctypes.c_int64(), ctypes.c_double()
    assert lib.tfx_sos_plan_info(a.ctypes.data, a.shape[0], ctypes.byref(prec), ctypes.byref(warm), ctypes.byref(bound)) == 0
    return prec.value, warm.value, bound.value


def _fused_warmup(lib, sos):
    a = np.ascontiguousarray(sos, dtype=np.float64)
    return lib.tfx_sos_fft_conv_warmup(a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a.shape[0])


def test_nan_coefficient_does_not_share_a_cache_entry_with_the_valid_cascade():
    """The host caches key on the coefficients' bytes: a cascade queried after its NaN twin (same coefficients but one
    NaN) keeps its own answers, and the NaN twin gets its own, whichever of the two comes first."""
    from torchfx_amd import _lib
    lib = _lib.load()
    good = np.array([[0.2, 0.4, 0.2, 1, -0.5, 0.2]])
    nan = good.copy()
    nan[0, 4] = np.nan
    assert lib.tfx_clear_caches() == 0
    alone = _plan_info(lib, good)
    assert alone[0] == 1 and alone[1] > 0 and np.isfinite(alone[2])      # TFX_PREC_F32, decays, finite bound
    assert lib.tfx_clear_caches() == 0
    assert _plan_info(lib, nan)[1] == -1
    assert _plan_info(lib, good) == alone

    good = np.array([[0.3, 0.1, 0.3, 1, -0.6, 0.25]])
    nan = good.copy()
    nan[0, 4] = np.nan
    assert lib.tfx_clear_caches() == 0
    w = _fused_warmup(lib, good)
    assert w > 0
    assert _fused_warmup(lib, nan) == -1
    assert lib.tfx_clear_caches() == 0
    assert _fused_warmup(lib, nan) == -1
    assert _fused_warmup(lib, good) == w


def test_plan_info_is_the_same_when_more_cascades_than_the_cache_holds_come_in_another_order():
    """300 distinct cascades (the SOS plan cache holds 256) queried forwards, then backwards: evicted plans are rebuilt with
    the same answers."""
    from torchfx_amd import _lib
    lib = _lib.load()
    g = np.random.default_rng(7)
    cascades = []
    for _ in range(300):
        r, th = g.uniform(0.3, 0.95), g.uniform(0.05, 3.0)
        cascades.append(np.array([[*g.uniform(-1, 1, 3), 1.0, -2 * r * np.cos(th), r * r]]))
    first = [_plan_info(lib, s) for s in cascades]
    second = [_plan_info(lib, s) for s in reversed(cascades)][::-1]
    assert first == second
