"""Plumbing of the audio-rate links on the sources and the segment Envelope (tests/test_ar_params_sources_abi.py,
tests/test_gpu_ar_params_sources.py): the voices of each case, shared so that the signatures the CPU test compiles are the
ones the GPU test runs.  Every voice is `driver -> linked node -> gain`, the driver SinWt(slow) * depth + offset."""
from __future__ import annotations

import numpy as np

from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

SIN_WAVEFORMS = (1, 2, 9, 10)  # Sine, Cosine, Half/FullWaveRectifiedSine: the PolyBlep waveforms that call sin
READER_BUFFER = (700, 44100.0)  # frames, sample rate of the reader bank's Buffer
ENV_SEGMENTS = ((0.003, 1.0), (0.004, 0.0))
LINKS = ["polyblep_freq", "polyblep_pulse_width", "random_lin_freq", "reader_rate", "envelope_time_scale"]


def lfo(n, p, depth, offset, rate_scale=0.01):
    """three stages: SinWt(slow) * depth + offset -- the driving signal; returns (stages, ctor entries by relative index)"""
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST)]
    ctor = {0: (p["freq"] * rate_scale).reshape(n, 1), 1: np.broadcast_to(np.asarray(depth, dtype=np.float64), (n,)).reshape(n, 1).copy(),
            2: np.broadcast_to(np.asarray(offset, dtype=np.float64), (n,)).reshape(n, 1).copy()}
    return st, ctor


def reader_buffer():
    n, sr = READER_BUFFER
    t = np.arange(n) / sr
    return 0.6 * np.sin(2 * np.pi * 331.0 * t) + 0.3 * np.sin(2 * np.pi * 1777.0 * t + 0.5)


def envelope_ctor(n, looping):
    """Envelope::new(0, segments).looping(looping): start_value, time_scale, looping, n_segments, then (duration, value) pairs"""
    row = [0.0, 1.0, 1.0 if looping else 0.0, float(len(ENV_SEGMENTS))] + [x for seg in ENV_SEGMENTS for x in seg]
    return np.tile(row, (n, 1))


def workload(case, n, sample_type, block_size=None, looping=False):
    """The bank of `case` with n voices: stage 3 is the linked node everywhere except the envelope bank, where it is stage 4
    (stage 3 the sine it shapes).  -> Workload (.linked = the linked stage's index)"""
    p = configs.voice_parameters(n)
    v = np.arange(n)
    gain = np.full((n, 1), 1.0 / n)
    wf = np.stack([(v % 14).astype(np.float64), p["freq"]], axis=1)  # PolyBlep::new(waveform, freq)
    bs = block_size or (64 if case == "envelope_time_scale" else 96)
    buffer = None
    linked = 3
    if case == "polyblep_freq":  # vibrato / FM on a band-limited oscillator
        drv, c = lfo(n, p, 0.3 * p["freq"], p["freq"], rate_scale=0.2)
        st = drv + [Stage(L.STAGE_POLYBLEP, ar_param=1, input2=3), Stage(L.STAGE_MUL_CONST)]
        c.update({3: wf, 4: np.ones((n, 1))})
    elif case == "polyblep_across_quarter_rate":  # both sides of sample_rate / 4, where every waveform turns into a sine
        drv, c = lfo(n, p, 2000.0, 12000.0, rate_scale=1.0)
        st = drv + [Stage(L.STAGE_POLYBLEP, ar_param=1, input2=3), Stage(L.STAGE_MUL_CONST)]
        c.update({3: wf, 4: np.ones((n, 1))})
    elif case == "polyblep_pulse_width":  # pulse-width modulation
        drv, c = lfo(n, p, 0.45, 0.5, rate_scale=0.05)
        st = drv + [Stage(L.STAGE_POLYBLEP, ar_param=2, input2=3), Stage(L.STAGE_MUL_CONST)]
        c.update({3: wf, 4: np.ones((n, 1))})
    elif case == "random_lin_freq":  # a rate-modulated random LFO
        drv, c = lfo(n, p, 900.0, 1000.0, rate_scale=0.2)
        st = drv + [Stage(L.STAGE_RANDOM_LIN, ar_param=1, input2=3), Stage(L.STAGE_MUL_CONST)]
        c.update({3: np.stack([v + 1.0, np.full(n, 500.0)], axis=1), 4: gain})
    elif case == "reader_rate":  # varispeed on a sampler voice; odd voices loop, even ones play once
        drv, c = lfo(n, p, 0.8, 1.0, rate_scale=0.05)
        st = drv + [Stage(L.STAGE_BUFFER_READER, ar_param=1, input2=3), Stage(L.STAGE_MUL_CONST)]
        c.update({3: np.stack([np.ones(n), (v % 2).astype(np.float64), np.zeros(n)], axis=1), 4: gain})
        buffer = (3, reader_buffer(), READER_BUFFER[1])
    elif case == "envelope_time_scale":  # an envelope whose speed follows a signal
        drv, c = lfo(n, p, 0.5, 1.0, rate_scale=0.5)
        st = drv + [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_ENVELOPE, ar_param=1, input2=3), Stage(L.STAGE_MUL_CONST)]
        c.update({3: p["freq"].reshape(n, 1), 4: envelope_ctor(n, looping), 5: gain})
        linked = 4
    else:
        raise KeyError(case)
    w = configs.Workload("ars_" + case, st, n, bs, sample_type, 1)
    w.ctor = c
    w.buffer = buffer
    w.linked = linked
    return w
