"""The inverse short-time Fourier transform without a GPU: the CPU route is torch.istft itself, the device route's own argument
check raises what torch raises, the plan's geometry, the Meta op, Wave.from_stft and the C entry points' refusals."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

from tests import istft_reference as R


def sp():
    import torchfx_amd.spectral as S
    return S


def ext():
    from torchfx_amd import torchfx_ext
    return torchfx_ext


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # torch's "a window was not provided", "the length is longer"
        yield


def spectrum(shape, seed=0, dtype=torch.complex64):
    g = np.random.default_rng(seed)
    return torch.from_numpy(g.standard_normal(shape) + 1j * g.standard_normal(shape)).to(dtype)


X3 = spectrum((3, 129, 12))

GOOD = [
    dict(n_fft=256), dict(n_fft=256, hop_length=100, window=torch.hann_window(256)), dict(n_fft=256, win_length=200, hop_length=50),
    dict(n_fft=256, win_length=201, window=torch.hamming_window(201)), dict(n_fft=256, center=False), dict(n_fft=256, normalized=True),
    dict(n_fft=256, window=torch.hann_window(256), length=300), dict(n_fft=256, length=1500), dict(n_fft=256, hop_length=256),
]


@pytest.mark.parametrize("kw", GOOD, ids=lambda k: "-".join(f"{a}={b if not isinstance(b, torch.Tensor) else 'w'}" for a, b in k.items()))
def test_cpu_tensors_get_torch_istft_itself(kw):
    for X in (X3[0], X3, X3.to(torch.complex128)):
        k = dict(kw)
        if "window" in k:
            k["window"] = k["window"].to(X.real.dtype)
        got, exp = sp().istft(X, **k), torch.istft(X, **k)
        assert got.dtype == exp.dtype and torch.equal(got, exp)
    X4 = torch.stack([X3, X3.flip(0)])               # [B, C, bins, frames]: the leading axes are rows
    got = sp().istft(X4, **kw)
    exp = torch.istft(X4.reshape(6, 129, 12), **kw)
    assert got.shape == (2, 3) + exp.shape[1:] and torch.equal(got.reshape(exp.shape), exp)


def test_cpu_two_sided_and_complex_results_are_torchs():
    X = spectrum((2, 256, 9), 3)
    w = torch.hann_window(256)
    assert torch.equal(sp().istft(X, 256, window=w, onesided=False), torch.istft(X, 256, window=w, onesided=False))
    got = sp().istft(X, 256, window=w, onesided=False, return_complex=True)
    assert got.dtype == torch.complex64 and torch.equal(got, torch.istft(X, 256, window=w, onesided=False, return_complex=True))
    assert torch.equal(sp().istft(X, 256, window=w), torch.istft(X, 256, window=w))         # onesided=None: 256 bins mean two-sided


BAD = [
    (dict(n_fft=512), "expected the frequency dimension"), (dict(n_fft=256, onesided=False), "expected the frequency dimension"),
    (dict(n_fft=0), "expected the frequency dimension"), (dict(n_fft=256, hop_length=0), "expected 0 < hop_length <= win_length"),
    (dict(n_fft=256, hop_length=200, win_length=100), "expected 0 < hop_length <= win_length"),
    (dict(n_fft=256, win_length=0), "expected 0 < hop_length <= win_length"), (dict(n_fft=256, win_length=300), "expected 0 < win_length <= n_fft"),
    (dict(n_fft=256, window=torch.ones(100)), "Invalid window shape"), (dict(n_fft=256, window=torch.ones(2, 256)), "Invalid window shape"),
    (dict(n_fft=256, window=torch.ones(256, dtype=torch.complex64)), "Complex windows are incompatible"),
    (dict(n_fft=256, return_complex=True), "Cannot have onesided output"),
    (dict(n_fft=256, window=torch.zeros(256)), "window overlap add min"), (dict(n_fft=256, window=torch.hann_window(256), center=False), "window overlap add min"),
]


@pytest.mark.parametrize("kw,fragment", BAD, ids=lambda k: "-".join(f"{a}={b if not isinstance(b, torch.Tensor) else tuple(b.shape)}" for a, b in k.items()) if isinstance(k, dict) else "")
def test_argument_errors_are_torchs_type_with_its_fragment(kw, fragment):
    """Through the public function (a CPU tensor: torch itself) and through the check the device route runs first."""
    k = dict(n_fft=None, hop_length=None, win_length=None, window=None, center=True, normalized=False, onesided=None, length=None,
             return_complex=False)
    k.update(kw)
    with pytest.raises(Exception) as want:
        torch.istft(X3, **k)
    assert fragment in str(want.value)
    with pytest.raises(type(want.value)) as got:
        sp().istft(X3, **k)
    assert fragment in str(got.value)
    if fragment == "window overlap add min":
        return                                       # a property of the window's values: the kernel's flag (tests/test_gpu_istft.py)
    with pytest.raises(type(want.value)) as got:
        sp()._check_istft(X3, *[k[n] for n in ("n_fft", "hop_length", "win_length", "window", "center", "normalized", "onesided", "length",
                                               "return_complex")])
    assert fragment in str(got.value)


def test_input_errors_are_torchs_type_with_its_fragment():
    for X, fragment in ((X3.real, "requires a complex-valued input"), (X3[:0], "input tensor cannot be empty"),
                        (X3[0, 0], "Dimension out of range"), (X3[None, None], "expected a tensor with 3 or 4 dimensions"),
                        (X3[..., :1], "Expected reduction dim")):
        with pytest.raises(Exception) as want:
            torch.istft(X, 256)
        assert fragment in str(want.value)
        with pytest.raises(type(want.value)) as got:
            sp()._check_istft(X, 256, None, None, None, True, False, None, None, False)
        assert fragment in str(got.value)
    with pytest.raises(TypeError, match="expected a tensor"):
        sp().istft([1.0], 256)
    assert sp()._check_istft(X3, 256, None, None, None, True, False, None, None, False) == (64, 256, True, 11 * 64)
    assert sp()._check_istft(X3, 256, 100, 200, None, False, False, None, 77, False) == (100, 200, True, 77)


@pytest.mark.parametrize("n_fft", [256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_plan_geometry(n_fft, dtype):
    E = ext()
    threads, acc_max, esz = (256, 32, 4) if dtype == torch.float32 else (128, 32, 8)
    tile_max = min(8 * n_fft, threads * acc_max)
    M = n_fft // 2
    for hop, frames, rows, center, length in ((n_fft // 4, 100, 3, True, None), (1, 700, 1, False, None), (n_fft, 9, 2, True, None),
                                              (100, 50, 4, True, 3000), (n_fft // 2, 7, 2, True, 40 * n_fft)):
        p = E.istft_plan_info(n_fft, hop, n_fft, frames, rows, dtype, center, length)
        pad = n_fft // 2 if center else 0
        T = R.natural_length(frames, n_fft, hop, pad) if length is None else length
        tile = min(tile_max, max(4 * n_fft, -(-8 * (n_fft - hop) // threads) * threads))
        G = threads // (n_fft // 32)
        extra = -(-n_fft // hop) - 1
        assert p["route"] == "lds" and p["length"] == T and p["tile"] == tile and tile % threads == 0
        assert p["frames_per_batch"] == G and p["threads_per_frame"] == n_fft // 32
        assert p["workgroups"] == rows * -(-T // tile)
        assert p["lds_bytes"] == esz * (2 * M + n_fft + G * (M + M // 16) * 2)
        assert p["redundant_share"] == pytest.approx(extra / (tile / hop + extra), rel=1e-12)
    assert E.istft_plan_info(n_fft, n_fft // 4, n_fft, 10, 1, torch.complex64 if dtype == torch.float32 else torch.complex128) == \
        E.istft_plan_info(n_fft, n_fft // 4, n_fft, 10, 1, dtype)
    if dtype == torch.float32:                       # two workgroups fit a CU's 160 KiB at every size
        assert 2 * p["lds_bytes"] <= 160 * 1024


def test_geometries_off_the_route_say_torch_and_bad_sizes_are_errors():
    E = ext()
    for kw in (dict(n_fft=400, hop=100, win_length=400), dict(n_fft=8192, hop=100, win_length=8192), dict(n_fft=256, hop=64, win_length=256, onesided=False)):
        p = E.istft_plan_info(frames=50, rows=2, **kw)
        assert p["route"] == "torch" and p["workgroups"] == 0 and p["tile"] == 0
        assert p["length"] == 49 * kw["hop"] + kw["n_fft"] - 2 * (kw["n_fft"] // 2)
    for kw, msg in ((dict(n_fft=0, hop=1, win_length=1), "n_fft"), (dict(n_fft=256, hop=0, win_length=256), "hop"),
                    (dict(n_fft=256, hop=201, win_length=200), "hop"), (dict(n_fft=256, hop=64, win_length=257), "win_length"),
                    (dict(n_fft=256, hop=64, win_length=0), "win_length"), (dict(n_fft=256, hop=64, win_length=256, frames=0), "bad shape"),
                    (dict(n_fft=256, hop=64, win_length=256, rows=-1), "bad shape"), (dict(n_fft=256, hop=64, win_length=256, length=0), "length"),
                    (dict(n_fft=256, hop=64, win_length=256, length=-7), "length"), (dict(n_fft=256, hop=64, win_length=256, frames=1), "no sample")):
        kw.setdefault("frames", 50)
        with pytest.raises(RuntimeError, match=msg):
            E.istft_plan_info(**kw)


def test_meta_op_has_the_result_shapes_dtypes_and_the_flag():
    from torchfx_amd import native
    native.load()
    op = torch.ops.torchfx_spectral_inverse.istft_forward
    for lead in ((), (3,), (2, 3)):
        for cdt, dt in ((torch.complex64, torch.float32), (torch.complex128, torch.float64)):
            X = torch.empty(lead + (513, 20), dtype=cdt, device="meta")
            y, flag = op(X, None, 1024, 256, 512, -1, False)
            assert y.shape == lead + (19 * 256,) and y.dtype == dt and y.device.type == "meta"
            assert flag.shape == (1,) and flag.dtype == torch.int32
            assert op(X, None, 1024, 256, 0, 777, True)[0].shape == lead + (777,)
            assert op(X, torch.empty(300, dtype=dt, device="meta"), 1024, 300, 0, -1, False)[0].shape == lead + (19 * 300 + 1024,)
    X = torch.empty(3, 513, 20, dtype=torch.complex64, device="meta")
    for args, msg in (((X, None, 512, 128, 256, -1, False), "expected the frequency dimension"), ((X, None, 1024, 0, 512, -1, False), "bad geometry"),
                      ((X, None, 1024, 256, 512, 0, False), "bad geometry"), ((X, None, 1024, 256, -1, -1, False), "bad geometry"),
                      ((X, torch.empty(2000, device="meta"), 1024, 256, 512, -1, False), "window"),
                      ((X, torch.empty(1024, dtype=torch.float64, device="meta"), 1024, 256, 512, -1, False), "real dtype"),
                      ((X, torch.empty(100, device="meta"), 1024, 256, 512, -1, False), "0 < hop <= win_length"),
                      ((X.real, None, 1024, 256, 512, -1, False), "complex64 or complex128"), ((X[0, :, 0], None, 1024, 256, 512, -1, False), "dimensions"),
                      ((X[..., :1], None, 1024, 256, 512, -1, False), "no sample")):
        with pytest.raises(RuntimeError, match=msg):
            op(*args)


def test_the_namespace_holds_the_one_op_with_a_device_kernel_and_a_cpu_refusal():
    import torchfx_amd
    from torchfx_amd import native
    native.load()
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_spectral_inverse::")}
    assert names == {"torchfx_spectral_inverse::istft_forward"}
    assert native.spectral_inverse_ops() is torch.ops.torchfx_spectral_inverse
    assert torch._C._dispatch_has_kernel_for_dispatch_key("torchfx_spectral_inverse::istft_forward", "CUDA")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext().istft_forward(X3, None, 256, 64, 128)
    assert {"istft_forward", "istft_plan_info"} <= set(ext().__all__) and "istft" in torchfx_amd.__all__ and "istft" in sp().__all__
    assert torchfx_amd.istft is sp().istft


def test_wave_from_stft_round_trips_on_the_cpu():
    from torchfx_amd import Wave
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 4096)).astype(np.float32))
    w = torch.hann_window(512)
    wave = Wave(x, 44100)
    back = Wave.from_stft(wave.stft(512, 128, window=w), 44100, 512, 128, window=w)
    assert isinstance(back, Wave) and back.fs == 44100 and back.ys.shape == x.shape and back.ys.dtype == torch.float32
    assert torch.equal(back.ys, torch.istft(torch.stft(x, 512, 128, window=w, return_complex=True), 512, 128, window=w))
    assert float((back.ys - x).abs().max()) < 1e-5
    assert Wave.from_stft(wave.stft(512, 128, window=w), 44100, 512, 128, window=w, length=1000).ys.shape == (2, 1000)


def test_c_entry_points_refuse_null_and_negative_arguments_without_a_device():
    from torchfx_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                        # never dereferenced: every check comes before the device is touched
    flag = ctypes.cast(one, ctypes.POINTER(ctypes.c_int))

    def fwd(spec=one, w=None, out=one, flag=flag, dtype=0, rows=2, frames=20, n_fft=1024, hop=256, wl=1024, pad=512, length=-1, norm=0):
        rc = lib.tfx_istft_forward(spec, w, out, flag, dtype, rows, frames, n_fft, hop, wl, pad, length, norm, None)
        return rc, (lib.tfx_last_error() or b"").decode()

    for kw, msg in ((dict(spec=None), "null"), (dict(out=None), "null"), (dict(flag=None), "null"), (dict(dtype=2), "dtype"), (dict(rows=-1), "bad shape"),
                    (dict(frames=0), "bad shape"), (dict(frames=-5), "bad shape"), (dict(n_fft=-1024), "n_fft"), (dict(hop=0), "hop"), (dict(hop=-3), "hop"),
                    (dict(hop=600, wl=512), "hop"), (dict(wl=0), "win_length"), (dict(wl=1025), "win_length"), (dict(pad=-1), "pad"), (dict(pad=2000), "pad"),
                    (dict(length=0), "length"), (dict(length=-2), "length"), (dict(frames=1), "no sample"),
                    (dict(n_fft=400, wl=400, hop=100, pad=200), "not on the LDS route")):
        rc, err = fwd(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    outs = [ctypes.c_int()] + [ctypes.c_int64() for _ in range(6)] + [ctypes.c_double()]
    refs = [ctypes.byref(o) for o in outs]
    assert lib.tfx_istft_plan_info(1024, 256, 1024, 20, 2, 0, 1, -1, 1, *refs) == 0
    assert outs[0].value == 1 and outs[1].value == 19 * 256 and outs[2].value == 6144 and outs[6].value == 2
    for i in range(8):
        broken = list(refs)
        broken[i] = None
        assert lib.tfx_istft_plan_info(1024, 256, 1024, 20, 2, 0, 1, -1, 1, *broken) != 0
        assert b"null output" in lib.tfx_last_error()
    assert lib.tfx_istft_plan_info(1024, -256, 1024, 20, 2, 0, 1, -1, 1, *refs) != 0
    assert lib.tfx_istft_plan_info(1024, 256, 1024, -20, 2, 0, 1, -1, 1, *refs) != 0


def masked_spectrum(n, hop, rows=2, frames_worth=6, seed=0, dtype=np.float32):
    """Gaussian rows, Hann window, the spectrum times a uniform(0.5, 1.5) mask: no longer a consistent STFT."""
    g = np.random.default_rng(seed)
    x = torch.from_numpy(g.standard_normal((rows, frames_worth * n + 5)).astype(dtype))
    w = torch.hann_window(n, dtype=torch.float64).to(x.dtype)
    X = torch.stft(x, n, hop, window=w, return_complex=True)
    return X * torch.from_numpy(g.uniform(0.5, 1.5, tuple(X.shape)).astype(dtype)), w


def test_reference_bound_holds_for_the_cpu_transform_with_the_headroom_the_device_test_relies_on():
    """CPU float32 torch.istft on masked spectra of Gaussian rows sits far inside the bound, so the device tests have room."""
    worst = 0.0
    for n in (256, 1024, 4096):
        for hop in (n // 4, n // 2, 100):
            X, w = masked_spectrum(n, hop, seed=n + hop)
            y, b = R.reference(X.numpy(), n, hop, n // 2, w.numpy())
            frac, _ = R.within(torch.istft(X, n, hop, window=w).numpy(), y, b, f"cpu {n}/{hop}")
            worst = max(worst, frac)
    assert worst < 0.1
    X, w = masked_spectrum(256, 64, rows=1, frames_worth=3, dtype=np.float64)
    y, b = R.reference(X.numpy(), 256, 64, 128, w.numpy(), frames_exact=R.exact_frames_longdouble(X.numpy(), 256))
    R.within(torch.istft(X, 256, 64, window=w).numpy(), y, b, "cpu float64 against the long-double inverse DFT")
    y64, _ = R.reference(X.numpy(), 256, 64, 128, w.numpy())
    assert float(np.abs(y64 - y).max()) < 1e-13
    assert math.isclose(R.natural_length(7, 256, 64, 128), 6 * 64)
