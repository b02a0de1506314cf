"""Voices with several delay stages: the workloads, rings and parameter traffic of tests/test_multi_delay_abi.py and
tests/test_gpu_multi_delay.py, and an independent numpy model of the delay nodes (delay.rs:14-50, 93-306).

Sizes are the smallest at which a ring per (delay stage, voice) can go wrong: 130 voices (two full wavefronts and a ragged
third), rings of 150 to 260 samples, a different length per stage and per 64-voice group, odd ones among them (a 16-byte piece
straddles the end), delays of 70 to 200 samples (whole lines, and every ring wraps at least three times in 10 to 14 blocks)."""
from __future__ import annotations

import functools

import numpy as np

from helpers import make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

N = 130
SR = configs.SAMPLE_RATE
KF = L.VALUE_FLOAT
DELAY_KINDS = (L.STAGE_SAMPLE_DELAY, L.STAGE_ALLPASS_DELAY, L.STAGE_ALLPASS_FB_DELAY)


def ring_seconds(samples):
    """max_delay for a ring of exactly `samples` samples, in SampleDelay (`as usize` of seconds * rate) and in the allpass
    delays (Seconds::to_samples) alike."""
    return (np.asarray(samples, dtype=np.float64) + 0.5) / SR


def per_group(lengths, n=N):
    return np.array([lengths[(v // 64) % len(lengths)] for v in range(n)], dtype=np.int64)


# ---- 1. three delays in series ---------------------------------------------------------------------------------------------
SERIES_STAGES = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SAMPLE_DELAY, delayed_changes_per_block=2),
                 Stage(L.STAGE_ALLPASS_FB_DELAY, delayed_changes_per_block=2), Stage(L.STAGE_ALLPASS_DELAY, delayed_changes_per_block=2),
                 Stage(L.STAGE_MUL_CONST)]
SERIES_RINGS = {2: per_group([192, 251, 160]), 3: per_group([256, 150, 201]), 4: per_group([177, 260, 237])}


def series_workload(sample_type, bs, n=N):
    p = configs.voice_parameters(n)
    w = configs.Workload("series", SERIES_STAGES, n, bs, sample_type, 2)
    w.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 0.5), 5: np.full((n, 1), 1.0 / n)}
    for s, rings in SERIES_RINGS.items():
        w.ctor[s] = ring_seconds(rings[:n]).reshape(n, 1)
    return w


def series_delays(stage, salt, n=N):
    """70 .. ring - 3 samples (and at most 200), a different one per voice; the allpass delays with a fraction."""
    v = np.arange(n, dtype=np.int64)
    ring = SERIES_RINGS[stage][:n]
    d = 70 + (v * 7 + salt * 13) % (np.minimum(ring - 3, 200) - 70 + 1)
    return (d + (0.0 if stage == 2 else 0.37)) / SR


def series_events(block, bank, bs, n=N):
    v = np.arange(n, dtype=np.uint32)
    if block == 0:
        for s in (2, 3, 4):
            bank.param_apply_many(v, s, 0, KF, series_delays(s, 0, n))
        bank.param_apply_many(v, 3, 1, KF, 0.5 + 0.001 * v)
    if block == 2:  # stage 2 only
        bank.param_apply_many(v, 2, 0, KF, series_delays(2, 1, n))
    if block == 3:  # stage 3 only
        bank.param_apply_many(v, 3, 0, KF, series_delays(3, 2, n))
    if block == 4:
        bank.param_apply_many(v, 3, 1, KF, -0.6 + 0.002 * v)
    if block == 5:  # sample-accurate: every voice at a frame of its own, one of its three delays; the others keep theirs
        for s in (2, 3, 4):
            sel = v[v % 3 == s - 2]
            bank.param_apply_many(sel, s, 0, KF, series_delays(s, 3, n)[sel], delays=((sel * 3 + 1) % bs).astype(np.uint16))
    if block == 6:  # voices 64 .. 127: shorter than a tile (0, 1 and the odd ones among them), on every delay
        sel = v[64:128]
        short = np.array([[0, 1, 5, 17, 31, 40, 63][i % 7] for i in range(len(sel))], dtype=np.float64)
        for s in (2, 3, 4):
            bank.param_apply_many(sel, s, 0, KF, (short + (0.0 if s == 2 else 0.25)) / SR)
    if block == 8:  # ... and long again
        sel = v[64:128]
        for s in (2, 3, 4):
            bank.param_apply_many(sel, s, 0, KF, series_delays(s, 4, n)[sel])


def series_blocks(bs):
    return 14 if bs == 64 else 10  # 896 / 1 000 samples: the longest ring (260) wraps three times


@functools.lru_cache(maxsize=None)
def series_expected(oracle, sample_type, bs):
    """The oracle's per-voice blocks, computed once and shared, read-only."""
    o = make_oracle(oracle, series_workload(sample_type, bs), want_mix=False)
    blocks = []
    for b in range(series_blocks(bs)):
        series_events(b, o, bs)
        voices = o.process_block()[1].copy()
        voices.setflags(write=False)
        blocks.append(voices)
    o.close()
    return blocks


# ---- 2. two SampleDelays against one -------------------------------------------------------------------------------------
def identity_workloads(sample_type, bs=64, n=N):
    """SampleDelay(d1) -> SampleDelay(d2) and the one-delay bank with d1 + d2; d = 0, d = the ring length and rings of one
    sample among the voices.  -> (two-delay workload, one-delay workload, d1, d2) with the delays in samples."""
    p = configs.voice_parameters(n)
    v = np.arange(n, dtype=np.int64)
    r1 = 150 + (v * 11) % 111           # 150 .. 260, odd ones among them
    r2 = 260 - (v * 7) % 111
    d1 = 70 + (v * 5) % (r1 - 70)
    d2 = 70 + (v * 3) % (r2 - 70)
    d1[3], d2[3] = 0, 90                # no delay in front
    d1[4], d2[4] = 100, 0               # ... behind
    d1[5], d2[5] = 0, 0
    d1[64], d2[65] = r1[64], r2[65]     # the whole ring
    d1[66], d2[66] = r1[66], r2[66]
    r1[67], d1[67] = 1, 1               # a ring of one sample
    r2[68], d2[68] = 1, 0
    r1[129], r2[129], d1[129], d2[129] = 1, 1, 1, 1
    two = configs.Workload("two_delays", [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SAMPLE_DELAY), Stage(L.STAGE_SAMPLE_DELAY),
                                          Stage(L.STAGE_MUL_CONST)], n, bs, sample_type, 2)
    two.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 0.5), 2: ring_seconds(r1).reshape(n, 1), 3: ring_seconds(r2).reshape(n, 1),
                4: np.full((n, 1), 1.0 / n)}
    one = configs.Workload("one_delay", [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SAMPLE_DELAY), Stage(L.STAGE_MUL_CONST)],
                           n, bs, sample_type, 2)
    one.ctor = {0: two.ctor[0], 1: two.ctor[1], 2: ring_seconds(r1 + r2).reshape(n, 1), 3: two.ctor[4]}
    return two, one, d1, d2


def delay_seconds(samples):
    """A delay_time that `(seconds * sample_rate) as usize` turns into exactly `samples`."""
    return (np.asarray(samples, dtype=np.float64) + 0.25) / SR


# ---- 3. graph voices --------------------------------------------------------------------------------------------------------
def parallel_workload(sample_type, bs, n=N, connected=False):
    """One source into two AllpassFeedbackDelays in parallel: joined by MATH_ADD, or (connected) the two delays are the voice's
    left and right signals."""
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_ALLPASS_FB_DELAY, input=2), Stage(L.STAGE_ALLPASS_FB_DELAY, input=2)]
    if not connected:
        st += [Stage(L.STAGE_MATH_ADD, input=3, input2=4), Stage(L.STAGE_MUL_CONST)]
    w = configs.Workload("parallel", st, n, bs, sample_type, 2)
    w.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 0.5), 2: ring_seconds(SERIES_RINGS[3][:n]).reshape(n, 1),
              3: ring_seconds(SERIES_RINGS[4][:n]).reshape(n, 1)}
    if not connected:
        w.ctor[5] = np.full((n, 1), 1.0 / n)
    return w


def parallel_events(block, bank, n=N):
    v = np.arange(n, dtype=np.uint32)
    if block == 0:
        bank.param_apply_many(v, 2, 0, KF, series_delays(3, 0, n))
        bank.param_apply_many(v, 3, 0, KF, series_delays(4, 0, n))
        bank.param_apply_many(v, 2, 1, KF, 0.5 + 0.001 * v)
        bank.param_apply_many(v, 3, 1, KF, 0.7 - 0.001 * v)
    if block == 3:  # the second delay only
        bank.param_apply_many(v, 3, 0, KF, series_delays(4, 2, n))


TWELVE_COMBS, TWELVE_SERIES = 8, 4


def twelve_workload(sample_type, bs, n):
    """Freeverb's mono topology: a source into eight feedback delays in parallel, summed, then four allpass delays in series."""
    p = configs.voice_parameters(n)
    v = np.arange(n, dtype=np.int64)
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL)]
    ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 0.25)}
    delays = {}
    for k in range(TWELVE_COMBS):
        st.append(Stage(L.STAGE_ALLPASS_FB_DELAY, input=2))
        ring = 150 + (v * (k + 3) + 17 * k) % 111
        ctor[len(st) - 1] = ring_seconds(ring).reshape(n, 1)
        delays[len(st) - 1] = (70 + (v * 3 + 11 * k) % (ring - 72) + 0.37) / SR
    acc = 3  # 1 + index of the first comb
    for k in range(1, TWELVE_COMBS):
        st.append(Stage(L.STAGE_MATH_ADD, input=acc, input2=3 + k))
        acc = len(st)
    for k in range(TWELVE_SERIES):
        st.append(Stage(L.STAGE_ALLPASS_DELAY) if k else Stage(L.STAGE_ALLPASS_DELAY, input=acc))
        ring = 260 - (v * (k + 5) + 7 * k) % 111
        ctor[len(st) - 1] = ring_seconds(ring).reshape(n, 1)
        delays[len(st) - 1] = (70 + (v * 5 + 13 * k) % (ring - 72) + 0.61) / SR
    st.append(Stage(L.STAGE_MUL_CONST))
    ctor[len(st) - 1] = np.full((n, 1), 1.0 / n)
    w = configs.Workload("twelve", st, n, bs, sample_type, 2)
    w.ctor = ctor
    return w, delays


def twelve_events(block, bank, w, delays):
    v = np.arange(w.n_voices, dtype=np.uint32)
    if block == 0:
        for s, d in delays.items():
            bank.param_apply_many(v, s, 0, KF, d)
            if w.stages[s].kind == L.STAGE_ALLPASS_FB_DELAY:
                bank.param_apply_many(v, s, 1, KF, np.full(w.n_voices, 0.5 + 0.02 * (s % 8)))
    if block == 2:  # one comb and one of the series delays, no other
        for s in (4, len(w.stages) - 3):
            bank.param_apply_many(v, s, 0, KF, delays[s] * 0.9)


# ---- the nodes restated (delay.rs), one voice, in the bank's sample type ----------------------------------------------------
class SampleDelayModel:
    def __init__(self, ring, dtype):
        self.buf = np.zeros(ring, dtype=dtype)
        self.wp = 0
        self.delay = 0

    def delay_time(self, seconds):
        self.delay = int(seconds * SR)

    def tick(self, x):
        self.buf[self.wp] = x
        out = self.buf[(self.wp + len(self.buf) - self.delay) % len(self.buf)]
        self.wp = (self.wp + 1) % len(self.buf)
        return out


class AllpassFeedbackDelayModel:
    """AllpassDelay with its AllpassInterpolator (delay.rs:53-206) inside the Schroeder allpass of :210-306."""

    def __init__(self, ring, dtype):
        self.F = dtype
        self.buf = np.zeros(ring, dtype=dtype)
        self.wf = self.rf = 0
        self.coeff = self.pin = self.pout = dtype(1)
        self.fb = dtype(0)

    def delay_time(self, seconds):
        F = self.F
        num = F(seconds * SR)
        fl = np.floor(num)
        frames = int(fl)
        delta = F(num - fl)
        if num > F(0.5) and delta < F(0.5):
            delta = F(delta + F(1))
            frames -= 1
        self.rf = self.wf - frames if self.wf >= frames else len(self.buf) - frames + self.wf
        self.coeff = F(F(F(1) - delta) / F(F(1) + delta))

    def feedback(self, value):
        self.fb = self.F(value)

    def tick(self, x):
        F = self.F
        v = self.buf[self.rf]
        d = F(F(self.coeff * F(v - self.pout)) + self.pin)
        self.pout, self.pin = d, v
        self.rf = (self.rf + 1) % len(self.buf)
        w = F(F(d * self.fb) + x)
        self.buf[self.wf] = w
        self.wf = (self.wf + 1) % len(self.buf)
        return F(d - F(self.fb * w))
