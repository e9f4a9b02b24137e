"""Test signals of the true-peak and loudness-range tests (tests/test_truepeak_host.py, tests/test_gpu_truepeak.py): the
EBU Tech 3341 true-peak tones and the Tech 3342 loudness-range tones, built the way the two documents describe them."""
import numpy as np

# (samples per period, phase in degrees) of the Tech 3341 true-peak tones: fs/4 at 45 and 0, fs/6 at 60, fs/8 at 67.5
TONES = [(4, 45.0), (4, 0.0), (6, 60.0), (8, 67.5)]
TP_TOL_ABOVE, TP_TOL_BELOW = 0.2, 0.4           # dB, Tech 3341: the reading lies within +0.2 / -0.4 of the tone's peak


def tone(div, phase_deg, amp=0.5, length=4800, fade=480, dtype=np.float32):
    """``amp * sin(2 pi n / div + phase)`` with a raised-cosine fade of ``fade`` samples at each end (0 = none).  An abrupt
    onset overshoots in any band-limited reconstruction, so only the faded tone has the true peak ``amp``."""
    n = np.arange(length)
    x = amp * np.sin(2.0 * np.pi * n / div + np.deg2rad(phase_deg))
    if fade:
        w = 0.5 - 0.5 * np.cos(np.pi * np.arange(fade) / fade)
        x[:fade] *= w
        x[-fade:] *= w[::-1]
    return x.astype(dtype)


def accent_tone(length=96000, base=0.02, accent=0.5, accent_len=480, dtype=np.float32):
    """The faded (4, 45 deg) tone at ``base`` with ONE raised-cosine accent of ``accent_len`` samples up to ``accent`` in the
    middle.  A steady tone's true peak sits a fixed ~0.3 dB under its loudness figure at fs/4 whatever its level, so no gain
    to -14 LUFS can bring it near -1 dBTP; 10 ms at 28 dB over the rest carry the peak and a fortieth of a gating block's
    energy."""
    x = tone(4, 45.0, 1.0, length, 480, np.float64)
    env = np.full(length, base)
    c = length // 2
    env[c:c + accent_len] += (accent - base) * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(accent_len) / accent_len))
    return (x * env).astype(dtype)


def stereo_sine(fs, f, seconds):
    s = np.sin(2.0 * np.pi * f * np.arange(int(round(fs * seconds))) / fs)
    return np.stack([s, s])


# Tech 3342 cases: (levels in LUFS of consecutive segments, seconds per segment, expected LRA in LU)
LRA_CASES = [((-20.0, -30.0), 20, 10.0), ((-20.0, -15.0), 20, 5.0), ((-40.0, -20.0), 20, 20.0),
             ((-50.0, -35.0, -20.0, -35.0, -50.0), 20, 15.0), ((-20.0, -30.0), 8, 10.0)]
LRA_TONE = {8000: 500.0, 48000: 1000.0}          # the sine's frequency per sample rate
LRA_TOL = 0.05                                    # LU; Tech 3342 allows +-1


def lra_signal(levels, seconds, fs, unit_lufs):
    """Stereo sine segments at ``levels`` LUFS; ``unit_lufs`` is the integrated loudness of the same sine at amplitude 1."""
    s = stereo_sine(fs, LRA_TONE[fs], seconds)
    return np.concatenate([s * 10.0 ** ((lv - unit_lufs) / 20.0) for lv in levels], axis=-1)
