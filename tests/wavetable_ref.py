"""OscWt on a Wavetable, restated in numpy from the reference's own lines (knaster_core_dsp/src/ugens/osc.rs:28-87,
dsp/wavetable.rs:327-610) -- not from the library under test.  u32 wrap-around phase arithmetic, the f32 threshold count
and a table look-up: no floating-point arithmetic lies between a table and the output, so every comparison against this
module is bit for bit.

  init:             phase = 0, freq_to_phase_inc = 16384 * 65536 * (1 / sample_rate)            (f64)
  freq(v):          self.freq = F::new(v); step = (self.freq as f64 * freq_to_phase_inc) as u32  (saturating cast)
  phase_offset(v):  (v * 65536.0) as u32
  next_sample:      out = wavetable.get(phase + phase_offset, self.freq); phase = phase.wrapping_add(step)
  Wavetable::get:   partial_tables[freq_to_table_index(freq as f32)][(phase >> 16) & 16383]
The stage's one constructor argument is applied as freq() right after init (include/knaster_hip.h, the decision at
KNH_STAGE_FLAG_WAVETABLE)."""
import math

import numpy as np

TABLE_SIZE = 16384
N_TABLES = 17
# 32 * 1.5^k, k = 0..15: every one exact in f32
THRESHOLDS = np.array([32.0, 48.0, 72.0, 108.0, 162.0, 243.0, 364.5, 546.75, 820.125, 1230.1875, 1845.28125, 2767.921875,
                       4151.8828125, 6227.82421875, 9341.736328125, 14012.6044921875], dtype=np.float32)
assert all(float(t) == 32.0 * 1.5 ** k for k, t in enumerate(THRESHOLDS))
# (20000 / (32 * 1.5^i)) as usize in f32: the highest harmonic partial table i takes (wavetable.rs:378-386)
HARMONIC_LIMITS = [625, 416, 277, 185, 123, 82, 54, 36, 24, 16, 10, 7, 4, 3, 2, 1, 0]
assert HARMONIC_LIMITS == [int(np.float32(20000.0) / (np.float32(32.0) * np.float32(1.5) ** np.float32(i))) for i in range(N_TABLES)]


def table_index(freq) -> np.ndarray:
    """freq_to_table_index(freq as f32), wavetable.rs:329-377: `if f <= 32.0 {0} else if f <= 48.0 {1} ... else {16}`."""
    f = np.asarray(freq).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.sum(~(f[..., None] <= THRESHOLDS), axis=-1).astype(np.uint32)


def sat_u32(x) -> np.ndarray:
    """Rust's `as u32` from f64: NaN -> 0, negative -> 0, too large -> u32::MAX, else truncation."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        y = np.where(x > 0.0, np.minimum(x, 4294967295.0), 0.0)
    return np.trunc(y).astype(np.uint64).astype(np.uint32)


def freq_to_phase_inc(sample_rate: int) -> float:
    return 16384.0 * 65536.0 * (1.0 / float(sample_rate))


def sine_table(dtype) -> np.ndarray:
    """NonAaWavetable::sine() (wavetable.rs:130-139) as the library's own SinWt table is made: f64 sin of the host libm,
    rounded to f32 -- the f32 values, widened for an f64 bank."""
    t = np.array([np.float32(math.sin((i / 16384.0) * math.pi * 2.0)) for i in range(TABLE_SIZE)], dtype=np.float32)
    return t.astype(dtype)


def ramp_tables(dtype) -> np.ndarray:
    """[17, 16384] with T[k][i] = k + i / 16384: exact and distinct in f32, so a wrong table or a wrong index shows in the value."""
    k = np.arange(N_TABLES, dtype=np.float64)[:, None]
    i = np.arange(TABLE_SIZE, dtype=np.float64)[None, :]
    t = (k + i / TABLE_SIZE).astype(dtype)
    assert np.array_equal(t.astype(np.float64), k + i / TABLE_SIZE)
    return t


def single_table(dtype) -> np.ndarray:
    """[1, 16384] with T[i] = -(1 + i / 16384): never a value of ramp_tables."""
    i = np.arange(TABLE_SIZE, dtype=np.float64)[None, :]
    return (-(1.0 + i / TABLE_SIZE)).astype(dtype)


class OscWtBank:
    """n voices, each an OscWt on one of `entries` ([n_tables, 16384] arrays, n_tables 17 or 1: one table that serves as
    all seventeen, Wavetable::from_buffer)."""

    def __init__(self, entries, entry_of_voice, freq, sample_rate, dtype):
        self.entries = [np.asarray(e, dtype=dtype).reshape(-1, TABLE_SIZE) for e in entries]
        self.dtype = np.dtype(dtype)
        self.n = len(entry_of_voice)
        self.f2p = freq_to_phase_inc(sample_rate)
        self.entry = np.array(entry_of_voice, dtype=np.int64)
        self.ctor = np.array(np.broadcast_to(np.asarray(freq, dtype=np.float64), (self.n,)))
        self.phase = np.zeros(self.n, dtype=np.uint32)
        self.offset = np.zeros(self.n, dtype=np.uint32)
        self.freq = np.zeros(self.n, dtype=self.dtype)
        self.step = np.zeros(self.n, dtype=np.uint32)
        self.set_freq(np.arange(self.n), self.ctor)

    # -- the setters --
    def set_freq(self, voices, values):
        voices = np.asarray(voices, dtype=np.int64)
        f = np.broadcast_to(np.asarray(values, dtype=np.float64), voices.shape).astype(self.dtype)  # F::new(v)
        self.freq[voices] = f
        self.step[voices] = sat_u32(f.astype(np.float64) * self.f2p)

    def set_phase_offset(self, voices, values):
        voices = np.asarray(voices, dtype=np.int64)
        self.offset[voices] = sat_u32(np.broadcast_to(np.asarray(values, dtype=np.float64), voices.shape) * 65536.0)

    def reset_phase(self, voices):
        self.phase[np.asarray(voices, dtype=np.int64)] = 0

    def construct(self, voices, entries=None, freq=None):
        """A new node for these voices: on `entries` (or the entry each has), with `freq` (or its constructor argument)."""
        voices = np.asarray(voices, dtype=np.int64)
        if entries is not None:
            self.entry[voices] = np.broadcast_to(np.asarray(entries, dtype=np.int64), voices.shape)
        if freq is not None:
            self.ctor[voices] = np.broadcast_to(np.asarray(freq, dtype=np.float64), voices.shape)
        self.phase[voices] = 0
        self.offset[voices] = 0
        self.set_freq(voices, self.ctor[voices])

    # -- the samples --
    def _get(self, phase, freq):
        out = np.zeros(self.n, dtype=self.dtype)
        idx = table_index(freq)
        pos = ((phase >> np.uint32(16)) & np.uint32(16383)).astype(np.int64)
        for e, tables in enumerate(self.entries):
            m = self.entry == e
            t = idx[m] if tables.shape[0] == N_TABLES else np.zeros(int(m.sum()), dtype=np.uint32)
            out[m] = tables[t, pos[m]]
        return out

    def render(self, n_frames, at_frame=None, ar_freq=None):
        """[n, n_frames].  at_frame: {frame: callable(self)} run in front of that frame (sample-accurate changes).
        ar_freq: [n, n_frames] (or [n_frames]) -- the signal on "freq" under .ar_params(): freq(x) in front of every sample."""
        out = np.zeros((self.n, n_frames), dtype=self.dtype)
        every = np.arange(self.n)
        for j in range(n_frames):
            if at_frame and j in at_frame:
                at_frame[j](self)
            if ar_freq is not None:
                a = np.asarray(ar_freq)
                self.set_freq(every, a[..., j].astype(np.float64))
            out[:, j] = self._get(self.phase + self.offset, self.freq)
            self.phase = self.phase + self.step  # u32: wraps
        return out


def smoothed_block_values(end_value, duration_s, sample_rate, block_size, n_blocks, start_value=0.0):
    """WrSmoothParams, block-rate linear smoothing (smooth_params.rs:188-197, 263-300): the value the wrapped node's setter
    gets at the start of each of the next n_blocks blocks after `end_value` was sent -- (end - start) * elapsed / duration
    + start with elapsed = 0, B, 2B, ... up to duration (f64) -- and None from the block after the one that reached it.
    start_value 0.0: what a parameter that never went through the wrapper's ramp starts from."""
    duration = int(float(np.float32(duration_s)) * float(sample_rate))
    vals, elapsed, done = [], 0, False
    for _ in range(n_blocks):
        if done:
            vals.append(None)
            continue
        vals.append((end_value - start_value) * (float(elapsed) / float(duration)) + start_value)
        if elapsed == duration:
            done = True
        else:
            elapsed = min(elapsed + block_size, duration)
    return vals
