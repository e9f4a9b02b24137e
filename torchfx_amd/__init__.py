"""torchfx_amd -- MI355X-native backend for the ``torchfx.filter`` hot path.

Top-level names follow the reference (``src/torchfx/__init__.py:12-23``): ``Wave``, ``FX``,
``FilterChain``, ``filter``, ``is_native_available``.
"""
from torchfx_amd import filter  # noqa: A004
from torchfx_amd._ops import is_native_available
from torchfx_amd.chain import FilterChain
from torchfx_amd.dynamics import compress
from torchfx_amd.effect import (FX, Chorus, Compressor, Delay, Distortion, Flanger, Freeverb, Gain, Gate, Limiter, LoudnessNormalize, ModulatedDelay, Normalize, Phaser, Reverb,
                                Vibrato, Waveshaper)
from torchfx_amd.filtfilt import sosfiltfilt
from torchfx_amd.gate import gate
from torchfx_amd.limiter import limit
from torchfx_amd.loudness import (block_energy, integrated_loudness, kweighting_sos, loudness_range, momentary_loudness,
                                  short_term_loudness, true_peak, true_peak_linear)
from torchfx_amd.modulation import modulated_delay
from torchfx_amd.phaser import phase_shift
from torchfx_amd.resample import Resample, resample_poly
from torchfx_amd.reverb import freeverb, freeverb_bank
from torchfx_amd.spectral import istft, spectrogram, stft
from torchfx_amd.wave import Wave
from torchfx_amd.waveshaper import waveshape

__all__ = ["FX", "Chorus", "Compressor", "Delay", "Distortion", "FilterChain", "Flanger", "Freeverb", "Gain", "Gate", "Limiter", "LoudnessNormalize", "ModulatedDelay", "Normalize", "Phaser", "Resample", "Reverb", "Wave", "block_energy",
           "compress", "filter", "freeverb", "freeverb_bank", "gate", "integrated_loudness", "is_native_available", "istft", "kweighting_sos", "limit", "loudness_range", "modulated_delay", "momentary_loudness",
           "phase_shift", "resample_poly", "short_term_loudness", "sosfiltfilt", "spectrogram", "stft", "true_peak", "true_peak_linear", "Vibrato", "Waveshaper", "waveshape"]
__version__ = "0.1.0"
