"""The overlap-save route -- which pipeline serves a call, its block length N, hop S and frames per row F -- pinned
for float32 and float64 signals and for the cascade-in-pass-A form, under the default knobs and under each forced
setting.  The expected values were recorded from the library before its route was gathered into one resolver
(csrc/ols_route.h); the answers are host-only, so no device is needed."""
import json
import os
import subprocess
import sys

from tests.conftest import ROOT

# (K, T, pad_left, pad_right, dtype)
CASES = [
    (257, 60000, 0, 0, "f32"),                # one-launch, 4096 points, short row
    (257, 2_880_000, 256, 0, "f32"),          # ... long row
    (639, 2_880_000, 638, 0, "f32"),
    (640, 2_880_000, 639, 0, "f32"),          # 8192 points from 640 taps on long rows
    (1500, 44100, 1499, 0, "f32"),            # short rows keep 4096 points up to 2048 taps
    (3000, 44100, 1500, 1499, "f32"),         # 8192 points
    (3000, 2_880_000, 2999, 0, "f32"),
    (3400, 2_880_000, 3399, 0, "f32"),        # 16 384 points, four 4096-point transforms (w8)
    (4096, 2_880_000, 0, 0, "f32"),
    (5000, 44100, 4999, 0, "f32"),            # 16 384 points, 1024-thread workgroup
    (8192, 2_880_000, 8191, 0, "f32"),
    (8192, 50000, 8191, 0, "f32"),
    (8193, 1_000_000, 8192, 0, "f32"),        # three-pass 2^16
    (12288, 2_880_000, 12287, 0, "f32"),      # three-pass 2^18
    (8193, 28_800_000, 8192, 0, "f32"),       # three-pass 2^20
    (20000, 1_000_000, 19999, 0, "f32"),
    (23000, 2_880_000, 22999, 0, "f32"),
    (66559, 28_800_000, 66558, 0, "f32"),
    (20000, 100_000, 19999, 0, "f32"),        # row shorter than the block: smaller block
    (100_000, 150_000, 0, 0, "f32"),          # ... none fits: rocFFT
    (600_000, 2_000_000, 0, 0, "f32"),        # rocFFT
    (10000, 1_000_003, 9999, 0, "f32"),       # rows that are not whole 128-byte lines
    (10000, 1_000_003, 4999, 5000, "f32"),
    (10000, 4_194_311, 9999, 0, "f32"),
    (257, 60001, 128, 128, "f32"),
    (12, 1000, 11, 0, "f32"),
    (257, 2_880_000, 256, 0, "f64"),          # float64: one-launch 4096 / 8192
    (1000, 2_880_000, 999, 0, "f64"),
    (4096, 44100, 4095, 0, "f64"),
    (5000, 2_880_000, 4999, 0, "f64"),        # float64 three-pass
    (5000, 2_880_003, 2500, 2499, "f64"),
    (100_000, 4_000_000, 99999, 0, "f64"),
    (5000, 500_000, 4999, 0, "f64"),          # float64 rocFFT
    (600_000, 2_000_000, 0, 0, "f64"),
]

SOS = {
    "a": [[0.2, 0.4, 0.2, 1.0, -0.5, 0.2]],
    "b": [[0.2, 0.4, 0.2, 1.0, -0.5, 0.2], [1.0, -1.2, 0.5, 1.0, -1.6, 0.7]],
    "slow": [[1e-4, 0.0, 0.0, 1.0, -0.9999, 0.0]],         # memory longer than a row: not served
    "nine": [[0.2, 0.4, 0.2, 1.0, -0.5, 0.2]] * 9,           # more sections than the column pass holds
}

# (T, taps, pad_left, pad_right, force_block, sos)
SOS_CASES = [
    (4_194_304, 10000, 9999, 0, 0, "a"),
    (8_388_608, 10000, 9999, 0, 0, "a"),
    (2_880_000, 10000, 9999, 0, 0, "a"),
    (28_800_000, 66559, 66558, 0, 0, "b"),
    (100_000, 257, 256, 0, 1, "a"),
    (100_000, 257, 256, 0, 2, "b"),
    (100_003, 257, 128, 128, 1, "a"),
    (4_194_307, 10000, 5000, 4999, 0, "b"),
    (100_000, 600_000, 0, 600_000, 1, "a"),
    (4_194_304, 10000, 9999, 0, 0, "slow"),
    (4_194_304, 10000, 9999, 0, 0, "nine"),
]

KNOBS = ("TFX_FFT_LOG2N", "TFX_OLS_LDS", "TFX_OLS_LDS16K", "TFX_OLS_LDS16K_R4", "TFX_OLS_LDS8K_MINK", "TFX_OLS_NATIVE",
         "TFX_OLS_NATIVE64")
SETTINGS = {"default": {}}
SETTINGS.update({"TFX_FFT_LOG2N=%d" % n: {"TFX_FFT_LOG2N": str(n)} for n in (12, 13, 14, 16, 17, 18, 20, 21)})
SETTINGS.update({"%s=%s" % kv: dict([kv]) for kv in (
    ("TFX_OLS_LDS", "0"), ("TFX_OLS_LDS16K", "0"), ("TFX_OLS_LDS16K", "2"), ("TFX_OLS_LDS16K_R4", "0"),
    ("TFX_OLS_LDS16K_R4", "2"), ("TFX_OLS_LDS8K_MINK", "0"), ("TFX_OLS_LDS8K_MINK", "2000"), ("TFX_OLS_NATIVE", "0"),
    ("TFX_OLS_NATIVE64", "0"))})

_CODE = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import torch
from torchfx_amd import torchfx_ext as E
cases, sos_cases, sos, knobs, settings = json.loads(sys.stdin.read())
out = {}
for name, env in settings.items():
    for k in knobs:
        os.environ.pop(k, None)
    os.environ.update(env)
    E.env_reload()
    plans = []
    for K, T, l, r, dt in cases:
        p = E.ols_plan_info(K, T, (l, r), torch.float64 if dt == "f64" else torch.float32)
        plans.append([p["path"], p["N"], p["S"], p["F"]])
    fused = []
    for T, taps, l, r, force, s in sos_cases:
        ok = E.sos_fft_conv_supported(T, sos[s], taps, (l, r), force)
        p = E.sos_fft_conv_plan_info(T, sos[s], taps, (l, r), force)
        fused.append([ok, None if p is None else [p["N"], p["S"], p["F"], p["warmup"]]])
    out[name] = {"plans": plans, "fused": fused, "warmup": {s: E.sos_fft_conv_warmup(c) for s, c in sorted(sos.items())}}
print(json.dumps(out))
"""


def route_answers(root):
    """Every answer of the grid under every setting, computed by the library built in `root` (a fresh process: the
    knobs are set in its own environment and reloaded between settings)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("TFX_")}
    r = subprocess.run([sys.executable, "-c", _CODE, root], input=json.dumps([CASES, SOS_CASES, SOS, KNOBS, SETTINGS]),
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


# answers under the default knobs: (path, N, S, F) per CASES entry
PLANS = [
    ("lds", 4096, 3840, 16),
    ("lds", 4096, 3840, 750),
    ("lds", 4096, 3456, 834),
    ("lds", 8192, 7552, 382),
    ("lds", 4096, 2597, 17),
    ("lds", 8192, 5193, 9),
    ("lds", 8192, 5184, 556),
    ("lds", 16384, 12960, 223),
    ("lds", 16384, 12289, 235),
    ("lds", 16384, 11385, 4),
    ("lds", 16384, 8192, 352),
    ("lds", 16384, 8193, 7),
    ("passes", 65536, 57344, 18),
    ("passes", 262144, 249856, 12),
    ("passes", 1048576, 1040384, 28),
    ("passes", 262144, 242144, 5),
    ("passes", 1048576, 1025568, 3),
    ("passes", 1048576, 982016, 30),
    ("passes", 65536, 45536, 3),
    ("rocfft", 262144, 162145, 1),
    ("rocfft", 2097152, 1497153, 1),
    ("passes", 65536, 55520, 19),
    ("passes", 65536, 55488, 19),
    ("passes", 1048576, 1038560, 5),
    ("lds", 4096, 3840, 16),
    ("lds", 4096, 4085, 1),
    ("lds", 4096, 3840, 750),
    ("lds", 8192, 7184, 401),
    ("lds", 8192, 4097, 11),
    ("passes", 1048576, 1043568, 3),
    ("passes", 1048576, 1043552, 3),
    ("passes", 1048576, 948576, 5),
    ("rocfft", 32768, 27769, 19),
    ("rocfft", 2097152, 1497153, 1),
]
# (N, S, F, warm-up) per SOS_CASES entry, None where the fused form does not serve
FUSED = [
    (1048576, 1038560, 5, 48), (2097152, 2087136, 5, 48), None, (2097152, 2030592, 15, 185), (1048576, 1048320, 1, 48),
    (2097152, 2096896, 1, 185), (1048576, 1048320, 1, 48), (1048576, 1038528, 5, 185), None, None, None,
]
WARMUP = {"a": 48, "b": 185, "nine": -1, "slow": 311910}
# forced settings: the entries that differ from the defaults, by index
FORCED = {
    "TFX_FFT_LOG2N=12": (
        {3: ("lds", 4096, 3456, 834), 5: ("rocfft", 8192, 5193, 9), 6: ("rocfft", 8192, 5193, 555),
         7: ("rocfft", 8192, 4793, 601), 8: ("rocfft", 8192, 4097, 702), 9: ("rocfft", 16384, 11385, 4),
         10: ("rocfft", 16384, 8193, 352), 11: ("rocfft", 16384, 8193, 7), 12: ("rocfft", 32768, 24576, 41),
         13: ("rocfft", 32768, 20481, 141), 14: ("rocfft", 32768, 24576, 1172), 15: ("rocfft", 65536, 45537, 22),
         16: ("rocfft", 65536, 42537, 68), 17: ("rocfft", 262144, 195586, 148), 18: ("rocfft", 65536, 45537, 3),
         21: ("rocfft", 32768, 22769, 44), 22: ("rocfft", 32768, 22769, 44), 23: ("rocfft", 32768, 22769, 185),
         27: ("lds", 4096, 3088, 933), 28: ("rocfft", 8192, 4097, 11), 29: ("rocfft", 16384, 11385, 253),
         30: ("rocfft", 16384, 11385, 253), 31: ("rocfft", 262144, 162145, 25), 32: ("rocfft", 16384, 11385, 44)},
        {0: None, 1: None, 3: None, 7: None}),
    "TFX_FFT_LOG2N=13": (
        {0: ("lds", 8192, 7936, 8), 1: ("lds", 8192, 7936, 363), 2: ("lds", 8192, 7552, 382),
         4: ("lds", 8192, 6693, 7), 7: ("lds", 8192, 4768, 605), 8: ("lds", 8192, 4097, 702),
         9: ("rocfft", 16384, 11385, 4), 10: ("rocfft", 16384, 8193, 352), 11: ("rocfft", 16384, 8193, 7),
         12: ("rocfft", 32768, 24576, 41), 13: ("rocfft", 32768, 20481, 141), 14: ("rocfft", 32768, 24576, 1172),
         15: ("rocfft", 65536, 45537, 22), 16: ("rocfft", 65536, 42537, 68), 17: ("rocfft", 262144, 195586, 148),
         18: ("rocfft", 65536, 45537, 3), 21: ("rocfft", 32768, 22769, 44), 22: ("rocfft", 32768, 22769, 44),
         23: ("rocfft", 32768, 22769, 185), 24: ("lds", 8192, 7936, 8), 25: ("lds", 8192, 8181, 1),
         26: ("lds", 8192, 7936, 363), 29: ("rocfft", 16384, 11385, 253), 30: ("rocfft", 16384, 11385, 253),
         31: ("rocfft", 262144, 162145, 25), 32: ("rocfft", 16384, 11385, 44)},
        {0: None, 1: None, 3: None, 7: None}),
    "TFX_FFT_LOG2N=14": (
        {0: ("lds", 16384, 16128, 4), 1: ("lds", 16384, 16128, 179), 2: ("lds", 16384, 15744, 183),
         3: ("lds", 16384, 15744, 183), 4: ("lds", 16384, 14885, 3), 5: ("lds", 16384, 13385, 4),
         6: ("lds", 16384, 13376, 216), 12: ("rocfft", 32768, 24576, 41), 13: ("rocfft", 32768, 20481, 141),
         14: ("rocfft", 32768, 24576, 1172), 15: ("rocfft", 65536, 45537, 22), 16: ("rocfft", 65536, 42537, 68),
         17: ("rocfft", 262144, 195586, 148), 18: ("rocfft", 65536, 45537, 3), 21: ("rocfft", 32768, 22769, 44),
         22: ("rocfft", 32768, 22769, 44), 23: ("rocfft", 32768, 22769, 185), 24: ("lds", 16384, 16128, 4),
         25: ("lds", 16384, 16373, 1), 26: ("rocfft", 16384, 16128, 179), 27: ("rocfft", 16384, 15385, 188),
         28: ("rocfft", 16384, 12289, 4), 29: ("rocfft", 16384, 11385, 253), 30: ("rocfft", 16384, 11385, 253),
         31: ("rocfft", 262144, 162145, 25), 32: ("rocfft", 16384, 11385, 44)},
        {0: None, 1: None, 3: None, 7: None}),
    "TFX_FFT_LOG2N=16": (
        {0: ("rocfft", 65536, 65280, 1), 1: ("passes", 65536, 65280, 45), 2: ("passes", 65536, 64896, 45),
         3: ("passes", 65536, 64896, 45), 4: ("rocfft", 65536, 64037, 1), 5: ("rocfft", 65536, 62537, 1),
         6: ("passes", 65536, 62528, 47), 7: ("passes", 65536, 62112, 47), 8: ("passes", 65536, 61440, 47),
         9: ("rocfft", 65536, 60537, 1), 10: ("passes", 65536, 57344, 51), 11: ("rocfft", 65536, 57345, 1),
         13: ("passes", 65536, 53248, 55), 14: ("passes", 65536, 57344, 503), 15: ("passes", 65536, 45536, 22),
         16: ("passes", 65536, 42528, 68), 17: ("rocfft", 262144, 195586, 148), 23: ("passes", 65536, 55520, 76),
         24: ("rocfft", 65536, 65280, 1), 25: ("rocfft", 1024, 1013, 1), 26: ("rocfft", 65536, 65280, 45),
         27: ("rocfft", 65536, 64537, 45), 28: ("rocfft", 65536, 61441, 1), 29: ("rocfft", 65536, 60537, 48),
         30: ("rocfft", 65536, 60537, 48), 31: ("rocfft", 262144, 162145, 25), 32: ("rocfft", 65536, 60537, 9)},
        {0: None, 1: None, 3: None, 7: None}),
    "TFX_FFT_LOG2N=17": (
        {0: ("rocfft", 65536, 65280, 1), 1: ("rocfft", 131072, 130816, 23), 2: ("rocfft", 131072, 130434, 23),
         3: ("rocfft", 131072, 130433, 23), 4: ("rocfft", 65536, 64037, 1), 5: ("rocfft", 65536, 62537, 1),
         6: ("rocfft", 131072, 128073, 23), 7: ("rocfft", 131072, 127673, 23), 8: ("rocfft", 131072, 126977, 23),
         9: ("rocfft", 65536, 60537, 1), 10: ("rocfft", 131072, 122881, 24), 11: ("rocfft", 65536, 57345, 1),
         12: ("rocfft", 131072, 122880, 9), 13: ("rocfft", 131072, 118785, 25), 14: ("rocfft", 131072, 122880, 235),
         15: ("rocfft", 131072, 111073, 10), 16: ("rocfft", 131072, 108073, 27), 17: ("rocfft", 262144, 195586, 148),
         18: ("rocfft", 131072, 111073, 1), 21: ("rocfft", 131072, 121073, 9), 22: ("rocfft", 131072, 121073, 9),
         23: ("rocfft", 131072, 121073, 35), 24: ("rocfft", 65536, 65280, 1), 25: ("rocfft", 1024, 1013, 1),
         26: ("rocfft", 131072, 130816, 23), 27: ("rocfft", 131072, 130073, 23), 28: ("rocfft", 65536, 61441, 1),
         29: ("rocfft", 131072, 126073, 23), 30: ("rocfft", 131072, 126073, 23), 31: ("rocfft", 262144, 162145, 25),
         32: ("rocfft", 131072, 126073, 4)},
        {0: None, 1: None, 3: None, 7: None}),
    "TFX_FFT_LOG2N=18": (
        {0: ("rocfft", 65536, 65280, 1), 1: ("passes", 262144, 261888, 11), 2: ("passes", 262144, 261504, 12),
         3: ("passes", 262144, 261504, 12), 4: ("rocfft", 65536, 64037, 1), 5: ("rocfft", 65536, 62537, 1),
         6: ("passes", 262144, 259136, 12), 7: ("passes", 262144, 258720, 12), 8: ("passes", 262144, 258048, 12),
         9: ("rocfft", 65536, 60537, 1), 10: ("passes", 262144, 253952, 12), 11: ("rocfft", 65536, 57345, 1),
         12: ("passes", 262144, 253952, 4), 14: ("passes", 262144, 253952, 114), 16: ("passes", 262144, 239136, 13),
         17: ("passes", 262144, 195584, 148), 18: ("rocfft", 131072, 111073, 1), 21: ("passes", 262144, 252128, 4),
         22: ("passes", 262144, 252096, 4), 23: ("passes", 262144, 252128, 17), 24: ("rocfft", 65536, 65280, 1),
         25: ("rocfft", 1024, 1013, 1), 26: ("rocfft", 262144, 261888, 11), 27: ("rocfft", 262144, 261145, 12),
         28: ("rocfft", 65536, 61441, 1), 29: ("rocfft", 262144, 257145, 12), 30: ("rocfft", 262144, 257145, 12),
         31: ("rocfft", 262144, 162145, 25), 32: ("rocfft", 262144, 257145, 2)},
        {0: None, 1: None, 3: None, 7: None}),
    "TFX_FFT_LOG2N=20": (
        {0: ("rocfft", 65536, 65280, 1), 1: ("passes", 1048576, 1048320, 3), 2: ("passes", 1048576, 1047936, 3),
         3: ("passes", 1048576, 1047936, 3), 4: ("rocfft", 65536, 64037, 1), 5: ("rocfft", 65536, 62537, 1),
         6: ("passes", 1048576, 1045568, 3), 7: ("passes", 1048576, 1045152, 3), 8: ("passes", 1048576, 1044480, 3),
         9: ("rocfft", 65536, 60537, 1), 10: ("passes", 1048576, 1040384, 3), 11: ("rocfft", 65536, 57345, 1),
         12: ("rocfft", 1048576, 1040384, 1), 13: ("passes", 1048576, 1036288, 3),
         15: ("rocfft", 1048576, 1028577, 1), 18: ("rocfft", 131072, 111073, 1), 21: ("rocfft", 1048576, 1038577, 1),
         22: ("rocfft", 1048576, 1038577, 1), 24: ("rocfft", 65536, 65280, 1), 25: ("rocfft", 1024, 1013, 1),
         26: ("rocfft", 1048576, 1048320, 3), 27: ("rocfft", 1048576, 1047577, 3), 28: ("rocfft", 65536, 61441, 1),
         29: ("rocfft", 1048576, 1043577, 3), 30: ("rocfft", 1048576, 1043577, 3),
         31: ("rocfft", 1048576, 948577, 5), 32: ("rocfft", 524288, 519289, 1)},
        {2: (1048576, 1038560, 3, 48)}),
    "TFX_FFT_LOG2N=21": (
        {0: ("rocfft", 65536, 65280, 1), 1: ("passes", 2097152, 2096896, 2), 2: ("passes", 2097152, 2096512, 2),
         3: ("passes", 2097152, 2096512, 2), 4: ("rocfft", 65536, 64037, 1), 5: ("rocfft", 65536, 62537, 1),
         6: ("passes", 2097152, 2094144, 2), 7: ("passes", 2097152, 2093728, 2), 8: ("passes", 2097152, 2093056, 2),
         9: ("rocfft", 65536, 60537, 1), 10: ("passes", 2097152, 2088960, 2), 11: ("rocfft", 65536, 57345, 1),
         12: ("rocfft", 1048576, 1040384, 1), 13: ("passes", 2097152, 2084864, 2),
         14: ("passes", 2097152, 2088960, 14), 15: ("rocfft", 1048576, 1028577, 1),
         16: ("passes", 2097152, 2074144, 2), 17: ("passes", 2097152, 2030592, 15),
         18: ("rocfft", 131072, 111073, 1), 21: ("rocfft", 1048576, 1038577, 1), 22: ("rocfft", 1048576, 1038577, 1),
         23: ("passes", 2097152, 2087136, 3), 24: ("rocfft", 65536, 65280, 1), 25: ("rocfft", 1024, 1013, 1),
         26: ("rocfft", 2097152, 2096896, 2), 27: ("rocfft", 2097152, 2096153, 2), 28: ("rocfft", 65536, 61441, 1),
         29: ("rocfft", 2097152, 2092153, 2), 30: ("rocfft", 2097152, 2092153, 2),
         31: ("rocfft", 2097152, 1997153, 3), 32: ("rocfft", 524288, 519289, 1)},
        {0: (2097152, 2087136, 3, 48), 2: (2097152, 2087136, 2, 48), 7: (2097152, 2087104, 3, 185)}),
    "TFX_OLS_LDS=0": (
        {0: ("rocfft", 4096, 3840, 16), 1: ("passes", 65536, 65280, 45), 2: ("passes", 65536, 64896, 45),
         3: ("passes", 65536, 64896, 45), 4: ("rocfft", 8192, 6693, 7), 5: ("rocfft", 16384, 13385, 4),
         6: ("passes", 65536, 62528, 47), 7: ("passes", 65536, 62112, 47), 8: ("passes", 65536, 61440, 47),
         9: ("rocfft", 32768, 27769, 2), 10: ("passes", 65536, 57344, 51), 11: ("rocfft", 32768, 24577, 3),
         24: ("rocfft", 4096, 3840, 16), 25: ("rocfft", 1024, 1013, 1), 26: ("rocfft", 4096, 3840, 750),
         27: ("rocfft", 4096, 3097, 930), 28: ("rocfft", 16384, 12289, 4)},
        {}),
    "TFX_OLS_LDS16K=0": (
        {7: ("lds", 8192, 4768, 605), 8: ("lds", 8192, 4097, 702), 9: ("rocfft", 32768, 27769, 2),
         10: ("passes", 65536, 57344, 51), 11: ("rocfft", 32768, 24577, 3)},
        {}),
    "TFX_OLS_LDS16K=2": (
        {7: ("lds", 8192, 4768, 605), 8: ("lds", 8192, 4097, 702)},
        {}),
    "TFX_OLS_LDS16K_R4=0": (
        {7: ("lds", 8192, 4768, 605), 8: ("lds", 8192, 4097, 702), 10: ("passes", 65536, 57344, 51)},
        {}),
    "TFX_OLS_LDS16K_R4=2": (
        {},
        {}),
    "TFX_OLS_LDS8K_MINK=0": (
        {3: ("lds", 4096, 3456, 834), 5: ("lds", 16384, 13385, 4), 6: ("lds", 16384, 13376, 216),
         27: ("lds", 4096, 3088, 933), 28: ("rocfft", 16384, 12289, 4)},
        {}),
    "TFX_OLS_LDS8K_MINK=2000": (
        {3: ("lds", 4096, 3456, 834), 27: ("lds", 4096, 3088, 933)},
        {}),
    "TFX_OLS_NATIVE=0": (
        {0: ("rocfft", 4096, 3840, 16), 1: ("rocfft", 4096, 3840, 750), 2: ("rocfft", 4096, 3458, 833),
         3: ("rocfft", 4096, 3457, 834), 4: ("rocfft", 8192, 6693, 7), 5: ("rocfft", 16384, 13385, 4),
         6: ("rocfft", 16384, 13385, 216), 7: ("rocfft", 16384, 12985, 222), 8: ("rocfft", 16384, 12289, 235),
         9: ("rocfft", 32768, 27769, 2), 10: ("rocfft", 32768, 24577, 118), 11: ("rocfft", 32768, 24577, 3),
         12: ("rocfft", 65536, 57344, 18), 13: ("rocfft", 65536, 53249, 55), 14: ("rocfft", 65536, 57344, 503),
         15: ("rocfft", 131072, 111073, 10), 16: ("rocfft", 131072, 108073, 27), 17: ("rocfft", 524288, 457730, 63),
         18: ("rocfft", 131072, 111073, 1), 21: ("rocfft", 65536, 55537, 19), 22: ("rocfft", 65536, 55537, 19),
         23: ("rocfft", 65536, 55537, 76), 24: ("rocfft", 4096, 3840, 16), 25: ("rocfft", 1024, 1013, 1),
         26: ("rocfft", 4096, 3840, 750), 27: ("rocfft", 4096, 3097, 930), 28: ("rocfft", 16384, 12289, 4),
         29: ("rocfft", 32768, 27769, 104), 30: ("rocfft", 32768, 27769, 104), 31: ("rocfft", 524288, 424289, 10)},
        {0: None, 1: None, 3: None, 7: None}),
    "TFX_OLS_NATIVE64=0": (
        {29: ("rocfft", 32768, 27769, 104), 30: ("rocfft", 32768, 27769, 104), 31: ("rocfft", 524288, 424289, 10)},
        {}),
}


def test_route_answers_match_the_recorded_ones():
    got = route_answers(ROOT)
    assert sorted(got) == sorted(SETTINGS)
    for name, (plans, fused) in [("default", ({}, {}))] + sorted(FORCED.items()):
        want_plans = [plans.get(i, p) for i, p in enumerate(PLANS)]
        want_fused = [fused.get(i, f) for i, f in enumerate(FUSED)]
        have = got[name]
        for case, want, (path, n, s, f) in zip(CASES, want_plans, have["plans"]):
            assert (path, n, s, f) == want, (name, "ols_plan_info", case)
        for case, want, (ok, plan) in zip(SOS_CASES, want_fused, have["fused"]):
            assert ok == (want is not None), (name, "sos_fft_conv_supported", case)
            assert (None if plan is None else tuple(plan)) == want, (name, "sos_fft_conv_plan_info", case)
        assert have["warmup"] == WARMUP, name
