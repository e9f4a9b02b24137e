"""The short-time Fourier transform without a GPU: the CPU route is torch.stft itself, torch's argument errors come in its
wording, the plan's geometry, the Meta op, the Wave methods and the C entry points' refusals."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tests import stft_reference as R


def sp():
    import torchfx_amd.spectral as S
    return S


def ext():
    from torchfx_amd import torchfx_ext
    return torchfx_ext


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # torch's "a window was not provided"
        yield


X3 = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 3, 3001)).astype(np.float32))


@pytest.mark.parametrize("kw", [
    dict(n_fft=512), dict(n_fft=400, hop_length=100), dict(n_fft=256, win_length=201), dict(n_fft=256, center=False),
    dict(n_fft=256, pad_mode="constant"), dict(n_fft=256, pad_mode="replicate"), dict(n_fft=256, normalized=True),
    dict(n_fft=256, onesided=False), dict(n_fft=1024, hop_length=1000, window=torch.hann_window(1024)),
    dict(n_fft=256, win_length=1, window=torch.tensor([2.0])),
], ids=lambda k: "-".join(f"{a}={b if not isinstance(b, torch.Tensor) else 'w'}" for a, b in k.items()))
def test_cpu_tensors_get_torch_stft_itself(kw):
    for x in (X3[0, 0], X3[0], X3[0].double()):
        k = dict(kw)
        if "window" in k:
            k["window"] = k["window"].to(x.dtype)
        got, exp = sp().stft(x, **k), torch.stft(x, return_complex=True, **k)
        assert got.dtype == exp.dtype and got.stride() == exp.stride() and torch.equal(got, exp)
    got = sp().stft(X3, **kw)                        # [B, C, T]: the leading axes are rows
    exp = torch.stft(X3.reshape(6, -1), return_complex=True, **kw)
    assert got.shape == (2, 3) + exp.shape[1:] and torch.equal(got.reshape(exp.shape), exp)


def test_spectrogram_on_the_cpu_is_the_power_of_torch_stft_with_the_named_window():
    S = sp()
    x = X3[0]
    for name, make in (("hann", torch.hann_window), ("hamming", torch.hamming_window)):
        w = make(300, periodic=True, dtype=torch.float64).to(torch.float32)
        assert torch.equal(S.named_window(name, 300), w)
        ref = torch.stft(x, 512, 128, 300, w, return_complex=True)
        assert torch.equal(S.spectrogram(x, 512, 128, 300, name, power=None), ref)
        assert torch.equal(S.spectrogram(x, 512, 128, 300, name, power=1.0), ref.abs())
        assert torch.equal(S.spectrogram(x, 512, 128, 300, name), ref.real.square() + ref.imag.square())
    assert torch.equal(S.named_window("rect", 7, torch.float64), torch.ones(7, dtype=torch.float64))
    assert S.named_window("hann", 16, torch.float64).dtype == torch.float64
    assert S.spectrogram(x).shape == (3, 513, 1 + 3001 // 256)
    with pytest.raises(ValueError, match="power must be None, 1.0 or 2.0"):
        S.spectrogram(x, power=3.0)
    with pytest.raises(ValueError, match="window must be a tensor or one of"):
        S.spectrogram(x, window="kaiser")


BAD = [
    dict(n_fft=0), dict(n_fft=6000), dict(n_fft=256, hop_length=0), dict(n_fft=256, win_length=0), dict(n_fft=256, win_length=300),
    dict(n_fft=256, window=torch.ones(100)), dict(n_fft=256, window=torch.ones(2, 256)), dict(n_fft=256, win_length=100, window=torch.ones(256)),
    dict(n_fft=8192), dict(n_fft=8192, center=False), dict(n_fft=256, pad_mode="nonsense"),
]


@pytest.mark.parametrize("kw", BAD, ids=lambda k: "-".join(f"{a}={b if not isinstance(b, torch.Tensor) else tuple(b.shape)}" for a, b in k.items()))
def test_every_argument_error_of_torch_stft_comes_in_its_wording(kw):
    """Both through the public function (a CPU tensor) and through the check the device route runs first, which asks torch.stft
    itself on tensors without storage."""
    x = X3[0, :, :3000]                              # n_fft 8192: reflect padding 4096 exceeds the row, and so does n_fft
    k = dict(n_fft=None, hop_length=None, win_length=None, window=None, center=True, pad_mode="reflect", normalized=False, onesided=True)
    k.update(kw)
    with pytest.raises(Exception) as want:
        torch.stft(x, return_complex=True, **k)
    with pytest.raises(type(want.value)) as got:
        sp().stft(x, **k)
    assert str(got.value) == str(want.value)
    with pytest.raises(type(want.value)) as got:
        sp()._check_as_torch(x, *[k[n] for n in ("n_fft", "hop_length", "win_length", "window", "center", "pad_mode", "normalized", "onesided")])
    assert str(got.value) == str(want.value)


def test_shortest_rows_torch_accepts_pass_the_check_and_one_sample_less_does_not():
    for n in (256, 4096):
        ok, short = torch.zeros(n // 2 + 1), torch.zeros(n // 2)
        sp()._check_as_torch(ok, n, None, None, None, True, "reflect", False, True)
        with pytest.raises(RuntimeError, match="Padding size should be less than"):
            sp()._check_as_torch(short, n, None, None, None, True, "reflect", False, True)
        sp()._check_as_torch(torch.zeros(n), n, None, None, None, False, "reflect", False, True)
        with pytest.raises(RuntimeError, match="expected 0 < n_fft"):
            sp()._check_as_torch(torch.zeros(n - 1), n, None, None, None, False, "reflect", False, True)


@pytest.mark.parametrize("n_fft", [256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_plan_geometry(n_fft, dtype):
    E = ext()
    threads = 256 if dtype == torch.float32 else 128
    esz = 4 if dtype == torch.float32 else 8
    for hop, T, rows, center in ((n_fft // 4, 10 * n_fft + 5, 3, True), (1, n_fft + 300, 1, False), (2 * n_fft, 9 * n_fft, 2, True),
                                 (100, 5000, 4, True)):
        p = E.stft_plan_info(n_fft, hop, n_fft, T, rows, dtype, center)
        pad = n_fft // 2 if center else 0
        G = threads // (n_fft // 32)
        assert p["route"] == "lds" and p["frames"] == 1 + (T + 2 * pad - n_fft) // hop == R.n_frames(T, n_fft, hop, pad)
        assert p["frames_per_workgroup"] == G and p["threads_per_frame"] == n_fft // 32
        assert p["workgroups"] == rows * -(-p["frames"] // G)
        M = n_fft // 2
        span, work = (G - 1) * min(hop, n_fft) + n_fft, G * (M + M // 16) * 2
        assert p["lds_bytes"] == esz * (2 * M + n_fft + max(span, work))
    # two workgroups of the largest float32 transform fit a CU's 160 KiB
    assert 2 * E.stft_plan_info(4096, 4096, 4096, 1 << 20)["lds_bytes"] <= 160 * 1024


def test_geometries_off_the_route_say_torch_and_bad_sizes_are_errors():
    E = ext()
    for kw in (dict(n_fft=400, hop=100, win_length=400), dict(n_fft=8192, hop=100, win_length=8192), dict(n_fft=256, hop=64, win_length=256, onesided=False),
               dict(n_fft=256, hop=64, win_length=256, pad_mode="replicate"), dict(n_fft=256, hop=64, win_length=256, pad_mode="circular")):
        p = E.stft_plan_info(length=20000, rows=2, **kw)
        assert p["route"] == "torch" and p["workgroups"] == 0 and p["frames"] == 1 + 20000 // kw["hop"]
    assert E.stft_plan_info(256, 64, 256, 5000, pad_mode="replicate", center=False)["route"] == "lds"     # nothing to pad
    for kw, msg in ((dict(n_fft=0, hop=1, win_length=1), "n_fft"), (dict(n_fft=256, hop=0, win_length=256), "hop"),
                    (dict(n_fft=256, hop=64, win_length=257), "win_length"), (dict(n_fft=256, hop=64, win_length=0), "win_length"),
                    (dict(n_fft=256, hop=64, win_length=256, length=128), "padding"),
                    (dict(n_fft=256, hop=64, win_length=256, length=255, center=False), "fewer than n_fft"),
                    (dict(n_fft=256, hop=64, win_length=256, rows=-1), "bad shape")):
        kw.setdefault("length", 5000)
        with pytest.raises(RuntimeError, match=msg):
            E.stft_plan_info(**kw)
    with pytest.raises(ValueError, match="pad_mode"):
        E.stft_plan_info(256, 64, 256, 5000, pad_mode="wrap")


def test_meta_op_has_torch_stfts_shape_dtype_and_strides():
    from torchfx_amd import native
    native.load()
    op = torch.ops.torchfx_spectral.stft_forward
    for shape in ((5001,), (3, 5001), (2, 3, 5001)):
        for dt, cdt in ((torch.float32, torch.complex64), (torch.float64, torch.complex128)):
            x = torch.empty(shape, dtype=dt, device="meta")
            y = op(x, None, 1024, 256, 512, 1, 0, False)
            ref = torch.stft(torch.empty((max(1, int(np.prod(shape[:-1]))), 5001), dtype=dt), 1024, 256, return_complex=True)
            assert y.shape == shape[:-1] + (513, 20) and y.dtype == cdt
            assert y.stride()[-2:] == ref.stride()[-2:] == (1, 513) and y.transpose(-1, -2).is_contiguous()
            for power in (1, 2):
                assert op(x, None, 1024, 256, 0, 0, power, True).dtype == dt
            assert op(x, torch.empty(201, dtype=dt, device="meta"), 256, 1, 0, 0, 0, False).shape == shape[:-1] + (129, 5001 - 255)
    x = torch.empty(3, 5001, device="meta")
    for args, msg in (((x, None, 1024, 0, 512, 1, 0, False), "bad geometry"), ((x, None, 8192, 64, 0, 1, 0, False), "bad geometry"),
                      ((x, None, 1024, 256, 512, 1, 3, False), "power"), ((x, torch.empty(2000, device="meta"), 1024, 256, 512, 1, 0, False), "window"),
                      ((x.to(torch.float16), None, 1024, 256, 512, 1, 0, False), "float32 or float64")):
        with pytest.raises(RuntimeError, match=msg):
            op(*args)


def test_the_namespace_holds_the_one_op_with_a_device_kernel_and_a_cpu_refusal():
    import torchfx_amd
    from torchfx_amd import native
    native.load()
    names = {s.name for s in torch._C._jit_get_all_schemas() if s.name.startswith("torchfx_spectral::")}
    assert names == {"torchfx_spectral::stft_forward"}
    assert torch._C._dispatch_has_kernel_for_dispatch_key("torchfx_spectral::stft_forward", "CUDA")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext().stft_forward(torch.zeros(2, 4096), None, 1024, 256, 512)
    assert {"stft_forward", "stft_plan_info"} <= set(ext().__all__) and {"stft", "spectrogram"} <= set(torchfx_amd.__all__)
    assert torchfx_amd.stft is sp().stft and torchfx_amd.spectrogram is sp().spectrogram
    from torchfx_amd import effect, realtime
    assert not any("stft" in n.lower() or "spectro" in n.lower() for n in dir(effect) + dir(realtime))      # an analysis, not an effect


def test_wave_methods_return_tensors():
    from torchfx_amd import Wave
    x = X3[0]
    w = Wave(x, 48000)
    assert torch.equal(w.stft(512, 128), torch.stft(x, 512, 128, return_complex=True))
    assert torch.equal(w.stft(256, win_length=201, window=torch.hamming_window(201), center=False, normalized=True),
                       torch.stft(x, 256, win_length=201, window=torch.hamming_window(201), center=False, normalized=True, return_complex=True))
    assert torch.equal(w.spectrogram(), sp().spectrogram(x)) and w.spectrogram().dtype == torch.float32
    assert torch.equal(w.spectrogram(512, power=1.0, window="hamming", pad_mode="constant"),
                       sp().spectrogram(x, 512, power=1.0, window="hamming", pad_mode="constant"))
    assert w.spectrogram(256, power=None).dtype == torch.complex64


def test_c_entry_points_refuse_null_and_negative_arguments_without_a_device():
    from torchfx_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                        # never dereferenced: every check comes before the device is touched

    def fwd(x=one, w=None, out=one, dtype=0, rows=2, T=5000, n_fft=1024, hop=256, wl=1024, pad=512, mode=1, power=0, norm=0):
        rc = lib.tfx_stft_forward(x, w, out, dtype, rows, T, n_fft, hop, wl, pad, mode, power, norm, None)
        return rc, (lib.tfx_last_error() or b"").decode()

    for kw, msg in ((dict(x=None), "null"), (dict(out=None), "null"), (dict(dtype=2), "dtype"), (dict(rows=-1), "bad shape"), (dict(T=0), "bad shape"),
                    (dict(T=-5), "bad shape"), (dict(n_fft=-1024), "n_fft"), (dict(hop=0), "hop"), (dict(hop=-3), "hop"), (dict(wl=0), "win_length"),
                    (dict(wl=1025), "win_length"), (dict(pad=-1), "pad"), (dict(pad=2000), "pad"), (dict(mode=7), "pad_mode"), (dict(mode=-1), "pad_mode"),
                    (dict(power=3), "power"), (dict(power=-1), "power"), (dict(T=512), "padding"), (dict(T=100, pad=0), "fewer than n_fft"),
                    (dict(n_fft=400, wl=400, pad=200), "not on the LDS route"), (dict(mode=2), "not on the LDS route")):
        rc, err = fwd(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    outs = [ctypes.c_int()] + [ctypes.c_int64() for _ in range(5)]
    refs = [ctypes.byref(o) for o in outs]
    assert lib.tfx_stft_plan_info(1024, 256, 1024, 5000, 2, 0, 1, 1, 1, *refs) == 0 and outs[0].value == 1 and outs[1].value == 20
    for i in range(6):
        broken = list(refs)
        broken[i] = None
        assert lib.tfx_stft_plan_info(1024, 256, 1024, 5000, 2, 0, 1, 1, 1, *broken) != 0
        assert b"null output" in lib.tfx_last_error()
    assert lib.tfx_stft_plan_info(1024, -256, 1024, 5000, 2, 0, 1, 1, 1, *refs) != 0
    assert lib.tfx_stft_plan_info(1024, 256, 1024, -5000, 2, 0, 1, 1, 1, *refs) != 0


def test_reference_bound_holds_for_the_cpu_transform_with_the_headroom_the_device_test_relies_on():
    """CPU float32 torch.stft on Gaussian rows sits far inside the bound, so the inputs of the device tests leave room."""
    for n in (256, 1024, 4096):
        x = np.random.default_rng(n).standard_normal((2, 3 * n + 5)).astype(np.float32)
        w = torch.hann_window(n, dtype=torch.float64).to(torch.float32)
        got = torch.stft(torch.from_numpy(x), n, n // 4, window=w, return_complex=True).numpy()
        assert R.within(got, R.windowed(x, n, n // 4, n // 2, "reflect", w.numpy()), f"cpu {n}") < 0.1
    x = np.random.default_rng(1).standard_normal((1, 700))
    s = R.windowed(x, 256, 64, 128)
    R.within(np.swapaxes(R.exact(s), -1, -2), s, "rfft against the long-double DFT", X=R.exact_longdouble(s))
