"""Mel spectrogram, host side (no GPU): the filterbank against the float64 formulas, the band table, every argument error and
the CPU composition."""
import math

import numpy as np
import pytest
import torch

from tests import mel_reference as R


def S():
    import torchfx_amd.spectral as sp
    return sp


# the last row has all-zero columns; at 129 bins and 40 htk mels the narrowest triangle (89 Hz) still holds a bin (62.5 Hz apart)
@pytest.mark.parametrize("n_freqs, rate, n_mels", [(129, 16000, 40), (513, 48000, 80), (2049, 44100, 128), (129, 16000, 128)])
@pytest.mark.parametrize("norm", [None, "slaney"])
@pytest.mark.parametrize("scale", ["htk", "slaney"])
def test_filterbank_is_the_float64_formula_rounded_once(n_freqs, rate, n_mels, norm, scale):
    want = R.fbanks(n_freqs, rate, n_mels, norm=norm, mel_scale=scale)
    for dtype, u in ((torch.float64, 2.0 ** -53), (torch.float32, 2.0 ** -24)):
        fb = S().mel_filterbank(n_freqs, rate, n_mels, norm=norm, mel_scale=scale, dtype=dtype)
        assert fb.shape == (n_freqs, n_mels) and fb.dtype == dtype
        # one rounding of dtype; the float64 design itself may differ from the reference's by a few float64 roundings
        assert (np.abs(fb.numpy().astype(np.float64) - want) <= u * np.abs(want) + 64 * 2.0 ** -53 * np.abs(want).max()).all()
    zero_columns = int((want == 0).all(0).sum())
    assert (zero_columns > 0) == (n_mels == 128 and n_freqs == 129) and int((fb == 0).all(0).sum()) == zero_columns
    if norm is None:
        assert float(fb.max()) <= 1.0
    table, total = __import__("torchfx_amd").torchfx_ext.mel_band_table(fb.numpy())
    head = np.frombuffer(table.numpy().tobytes()[:12 * n_mels], np.int32).reshape(3, n_mels)
    assert (head[1] == R.band_lengths(fb.numpy())).all() and total == head[1].sum() and (head[2] == np.cumsum(head[1]) - head[1]).all()
    assert table.numel() == (12 * n_mels + 7) // 8 * 8 + 4 * total


def test_known_points_of_the_scales():
    """htk: 1000 Hz is 2595 log10(17 / 7) = 999.9855... mel (the 2595 of the formula makes it 1000 to two parts in 10^5, not
    exactly); slaney: exactly 15."""
    sp = S()
    for hz_to_mel in (R.hz_to_mel, sp._hz_to_mel):
        htk = float(hz_to_mel(1000.0, "htk"))
        assert abs(htk - 2595.0 * math.log10(17.0 / 7.0)) < 1e-9 and abs(htk - 1000.0) < 0.02 and float(hz_to_mel(1000.0, "slaney")) == 15.0


@pytest.mark.parametrize("kw, name", [
    (dict(n_mels=0), "n_mels"), (dict(f_min=-1.0), "f_min"), (dict(f_min=4000.0, f_max=4000.0), "f_min"), (dict(f_max=9000.0), "f_max"),
    (dict(power=3.0), "power"), (dict(norm="l2"), "norm"), (dict(mel_scale="bark"), "mel_scale"), (dict(log="dB"), "log"),
    (dict(amin=0.0), "amin"), (dict(top_db=-1.0), "top_db"), (dict(filterbank=torch.ones(128, 4)), "filterbank")])
def test_every_argument_error_names_its_argument(kw, name):
    with pytest.raises(ValueError, match=name):
        S().mel_spectrogram(torch.zeros(2, 2048), 16000, 256, **kw)


@pytest.mark.parametrize("log, power, top_db", [(None, 2.0, None), ("db", 2.0, 80.0), ("db", 1.0, 30.0), ("log10", 1.0, None), ("ln", 2.0, None)])
def test_cpu_result_is_the_composition(log, power, top_db):
    sp = S()
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 3, 5000))).to(torch.float32)
    x[1] *= 1e-3
    x[0, :, :600] = 0                                                    # silent frames: the floor
    got = sp.mel_spectrogram(x, 16000, 400, 160, n_mels=40, power=power, log=log, top_db=top_db, norm="slaney", mel_scale="slaney")
    P = sp.spectrogram(x, 400, 160, power=power)
    fb = sp.mel_filterbank(201, 16000, 40, norm="slaney", mel_scale="slaney")
    want = torch.matmul(P.transpose(-1, -2), fb).transpose(-1, -2)
    if log is not None:
        v = torch.where(want < 1e-10, torch.full_like(want, 1e-10), want)
        want = v.log() if log == "ln" else v.log10() * ({2.0: 10.0, 1.0: 20.0}[power] if log == "db" else 1.0)
    if top_db is not None:
        want = torch.maximum(want, want.amax(dim=(1, 2, 3), keepdim=True) - top_db)
        assert float(want[1].min()) < float(want[0].min())                # each batch item has a floor of its own
    assert got.shape == (2, 3, 40, 32) and got.stride()[-2:] == (1, 40) and torch.equal(got, want)
    assert torch.equal(sp.MelSpectrogram(16000, 400, 160, n_mels=40, power=power, log=log, top_db=top_db, norm="slaney", mel_scale="slaney")(x), got)
    if top_db is None:                                                   # a caller's bank, and a [C, T] signal
        assert torch.equal(sp.mel_spectrogram(x[0], 16000, 400, 160, power=power, log=log, filterbank=fb), got[0])
