"""The Galactic reverb restated in numpy from reading knaster_airwindows/src/galactic.rs:14-400 and StaticSampleDelay
(knaster_core_dsp/src/ugens/delay.rs:308-416): the checker of KNH_STAGE_GALACTIC.  Test infrastructure like the oracle --
nothing under knaster_amd/ imports it.  Citations are file:line in the knaster repo.

Two implementations written separately, so that a slip in one shows against the other (tests/test_galactic_ref.py):
  * StaticSampleDelay / Galactic: vectorised over voices (arrays of shape [n_voices]), a Python loop over samples; every F
    operation in np.float32 / np.float64 according to `dtype`, the f64 parts (vib_m, oldfpd, the dither products) in
    np.float64, casts where the Rust has F::new / to_f64;
  * ScalarGalactic: one voice in plain Python floats, f32 by rounding every result through struct (for + - * / a double
    rounded to f32 equals the f32 operation: 53 >= 2 * 24 + 2 bits).

sin() is math.sin (the C library's) in both: it is what the host side of the engine calls for the phase that never moves.
The seeds of the two xorshift32 streams (fpd_l, fpd_r) are arguments: the reference draws them from
fastrand::Rng::with_seed(next_randomness_seed()).u32(16386..u32::MAX) (galactic.rs:147-154), which is not restated.
The reference's 2_u64.pow(exp + 62) (galactic.rs:372) overflows for exp >= 2; the release build's wrap to 0 is restated."""
from __future__ import annotations

import math
import struct

import numpy as np

GALACTIC_DELAY_TIMES = [6480, 3660, 1720, 680, 9700, 6000, 2320, 940, 15220, 8460, 4540, 3200]  # galactic.rs:39-41


def ring_lengths(sample_rate: int):
    """galactic.rs:52-60: ((time as f64 / 44100.) * sample_rate as f64) as usize"""
    return [int((float(t) / 44100.0) * float(sample_rate)) for t in GALACTIC_DELAY_TIMES]


class StaticSampleDelay:
    """delay.rs:308-416, one ring per voice: buffer [n_voices][len], position and delay_length per voice."""

    def __init__(self, delay_length_in_samples: int, n_voices: int = 1, dtype=np.float64):
        assert delay_length_in_samples != 0  # delay.rs:321
        self.dtype = np.dtype(dtype).type
        self.n = n_voices
        self.buffer = np.zeros((n_voices, delay_length_in_samples), dtype=dtype)
        self.position = np.zeros(n_voices, dtype=np.int64)
        self.delay_length = np.full(n_voices, delay_length_in_samples, dtype=np.int64)
        self._v = np.arange(n_voices)

    def buffer_len(self) -> int:
        return self.buffer.shape[1]

    def set_delay_length_fraction(self, fraction):  # delay.rs:337-342: (F(buffer.len()) * fraction).to_usize()
        f = np.asarray(fraction, dtype=self.dtype)
        self.delay_length = np.broadcast_to((self.dtype(self.buffer_len()) * f).astype(np.int64), (self.n,)).copy()

    def read(self):  # delay.rs:370-372
        return self.buffer[self._v, self.position]

    def write_and_advance(self, x):  # delay.rs:395-398: the wrap uses delay_length, after the write
        self.buffer[self._v, self.position] = x
        self.position = (self.position + 1) % self.delay_length

    def read_at_lin(self, index):  # delay.rs:378-392
        index = np.asarray(index, dtype=self.dtype)
        low = np.floor(index).astype(np.int64)
        high = np.ceil(index).astype(np.int64)
        n = self.buffer_len()
        k = low // n  # `while low >= len { low -= len; high -= len }`
        low = low - k * n
        high = high - k * n
        high = np.where(high >= n, high - n, high)
        low_sample = self.buffer[self._v, low]
        high_sample = self.buffer[self._v, high]
        fract = index - np.trunc(index)
        return low_sample + (high_sample - low_sample) * fract

    # the block half (delay.rs:344-368), voice by voice
    def read_block(self, block_size: int):
        out = np.zeros((self.n, block_size), dtype=self.dtype)
        n = self.buffer_len()
        assert n >= block_size
        for v in range(self.n):
            pos = int(self.position[v])
            end = pos + block_size
            if end <= n:
                out[v] = self.buffer[v, pos:end]
            else:
                end = end % int(self.delay_length[v])
                out[v, :block_size - end] = self.buffer[v, pos:]
                out[v, block_size - end:] = self.buffer[v, :end]
        return out

    def write_block_and_advance(self, block):
        block = np.asarray(block, dtype=self.dtype).reshape(self.n, -1)
        block_size = block.shape[1]
        n = self.buffer_len()
        assert n >= block_size
        for v in range(self.n):
            pos = int(self.position[v])
            end = pos + block_size
            if end <= n:
                self.buffer[v, pos:end] = block[v]
            else:
                end = end % int(self.delay_length[v])
                self.buffer[v, pos:] = block[v, :block_size - end]
                self.buffer[v, :end] = block[v, block_size - end:]
            self.position[v] = (pos + block_size) % n


def _powi(x, n: int):
    """f32::powi / f64::powi: multiply by squaring (compiler-builtins __powisf2 / __powidf2), n > 0."""
    r = np.ones_like(x)
    a = x.copy()
    while True:
        if n & 1:
            r = r * a
        n //= 2
        if n == 0:
            break
        a = a * a
    return r


def _sin_all(x: np.ndarray) -> np.ndarray:
    return np.array([math.sin(float(t)) for t in x], dtype=np.float64)


class Galactic:
    """galactic.rs:14-400 for n_voices independent reverbs.  Parameters are arrays [n_voices] (or scalars)."""

    REPLACE, DETUNE, BRIGHTNESS, BIGNESS, WET = range(5)

    def __init__(self, n_voices, dtype, replace, detune, brightness, bigness, wet, fpd_l, fpd_r):
        self.n = n_voices
        self.F = np.dtype(dtype).type
        arr = lambda x: np.broadcast_to(np.asarray(x, dtype=np.float64), (n_voices,)).astype(self.F)  # noqa: E731
        self.param = [arr(replace), arr(detune), arr(brightness), arr(bigness), arr(wet)]
        self.fpd_l = np.broadcast_to(np.asarray(fpd_l, dtype=np.uint32), (n_voices,)).copy()
        self.fpd_r = np.broadcast_to(np.asarray(fpd_r, dtype=np.uint32), (n_voices,)).copy()
        assert (self.fpd_l != 0).all() and (self.fpd_r != 0).all()
        self.vib_m = np.full(n_voices, 3.0)           # galactic.rs:160
        self.oldfpd = np.full(n_voices, 429496.7295)  # :162
        z = lambda: np.zeros(n_voices, dtype=self.F)  # noqa: E731
        self.feedback = [[z() for _ in range(4)] for _ in range(2)]
        self.iir_al, self.iir_ar, self.iir_bl, self.iir_br = z(), z(), z(), z()
        self._sin_key = None

    def set_param(self, index: int, value, voices=None):
        """param_apply (galactic.rs:124-136): value.f() as F."""
        if voices is None:
            self.param[index] = np.broadcast_to(np.asarray(value, dtype=np.float64), (self.n,)).astype(self.F)
        else:
            self.param[index] = self.param[index].copy()
            self.param[index][voices] = np.asarray(value, dtype=np.float64).astype(self.F)

    def init(self, sample_rate: int):  # galactic.rs:51-74
        lens = ring_lengths(sample_rate)
        self.delays_left = [StaticSampleDelay(n, self.n, self.F) for n in lens]
        self.delays_right = [StaticSampleDelay(n, self.n, self.F) for n in lens]
        self.detune_delay_left = StaticSampleDelay(256, self.n, self.F)
        self.detune_delay_right = StaticSampleDelay(256, self.n, self.F)
        overallscale = 1.0
        overallscale /= 44100.0
        overallscale *= float(sample_rate)
        self.overallscale = self.F(overallscale)

    def _sines(self):
        key = self.vib_m.tobytes()
        if key != self._sin_key:
            self._sin_key = key
            self._sin = (_sin_all(self.vib_m), _sin_all(self.vib_m + (math.pi / 2.0)))
        return self._sin

    @staticmethod
    def _mix(b, i):  # galactic.rs:285-289
        return b[i] - (b[(1 + i) % 4] + b[(2 + i) % 4] + b[(3 + i) % 4])

    def _dither(self, sample, fpd):
        """galactic.rs:364-373 with frexp (:390-400); fpd is the stream's state AFTER this sample's xorshift."""
        s = sample.astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = np.log2(np.abs(s))
            e = np.floor(lg) + np.float32(1.0)
        e = np.where(np.isnan(e), 0.0, e.astype(np.float64))
        exp = np.clip(e, 0.0, 4294967295.0).astype(np.uint64)  # `as u32` saturates
        exp = np.where(s == 0, np.uint64(0), exp)
        shift = (exp + np.uint64(62)) & np.uint64(0xFFFFFFFF)   # u32 addition (wraps in a release build)
        pw = np.where(shift < 64, np.uint64(1) << np.minimum(shift, np.uint64(63)), np.uint64(0))  # 2_u64.pow wraps to 0
        return self.F(0) + ((fpd.astype(np.float64) - float(0x7FFFFFFF)) * 5.5e-36 * pw.astype(np.float64)).astype(self.F)

    def process(self, left, right):
        """galactic.rs:172-388.  left, right: [n_voices][n] of F.  Returns (left_out, right_out)."""
        F = self.F
        left = np.asarray(left, dtype=F)
        right = np.asarray(right, dtype=F)
        n = left.shape[1]
        out_l = np.zeros((self.n, n), dtype=F)
        out_r = np.zeros((self.n, n), dtype=F)
        one = F(1)
        p_replace, p_detune, p_brightness, p_bigness, p_wet = self.param
        regen = F(0.0625) + ((one - p_replace) * F(0.0625))
        attenuate = (one - (regen / F(0.125))) * F(1.333)
        lowpass = _powi(F(1.00001) - (one - p_brightness), 2) / np.sqrt(self.overallscale)
        drift = _powi(p_detune, 3) * F(0.001)
        size = (p_bigness * F(0.9)) + F(0.1)
        wet = one - _powi(one - p_wet, 3)
        for d in self.delays_left + self.delays_right:
            d.set_delay_length_fraction(size)
        drift64 = drift.astype(np.float64)
        dl, dr = self.delays_left, self.delays_right
        for k in range(n):
            in_l, in_r = left[:, k], right[:, k]
            in_l = np.where(np.abs(in_l).astype(np.float64) < 1.18e-23, (self.fpd_l.astype(np.float64) * 1.18e-17).astype(F), in_l)
            in_r = np.where(np.abs(in_r).astype(np.float64) < 1.18e-23, (self.fpd_r.astype(np.float64) * 1.18e-17).astype(F), in_r)
            dry_l, dry_r = in_l, in_r
            self.vib_m = self.vib_m + self.oldfpd * drift64
            over = self.vib_m > math.tau
            if over.any():
                self.vib_m = np.where(over, 0.0, self.vib_m)
                self.oldfpd = np.where(over, 0.4294967295 + (self.fpd_l.astype(np.float64) * 0.0000000000618), self.oldfpd)
            self.detune_delay_left.write_and_advance(in_l * attenuate)
            self.detune_delay_right.write_and_advance(in_r * attenuate)
            sin_l, sin_r = self._sines()
            offset_ml = (sin_l + 1.0) * 127.0
            offset_mr = (sin_r + 1.0) * 127.0
            working_ml = self.detune_delay_left.position.astype(np.float64) + offset_ml
            working_mr = self.detune_delay_right.position.astype(np.float64) + offset_mr
            in_l = self.detune_delay_left.read_at_lin(working_ml.astype(F))
            in_r = self.detune_delay_right.read_at_lin(working_mr.astype(F))
            self.iir_al = (self.iir_al * (one - lowpass)) + (in_l * lowpass)
            in_l = self.iir_al
            self.iir_ar = (self.iir_ar * (one - lowpass)) + (in_r * lowpass)
            in_r = self.iir_ar
            # block 0: left rings take the right channel's feedback and the other way round (galactic.rs:259-265)
            for i in range(4):
                dl[i].write_and_advance((self.feedback[1][i] * regen) + in_l)
            for i in range(4):
                dr[i].write_and_advance((self.feedback[0][i] * regen) + in_r)
            b0l = [dl[i].read() for i in range(4)]
            b0r = [dr[i].read() for i in range(4)]
            for i in range(4):
                dl[i + 4].write_and_advance(self._mix(b0l, i))
            for i in range(4):
                dr[i + 4].write_and_advance(self._mix(b0r, i))
            b1l = [dl[i + 4].read() for i in range(4)]
            b1r = [dr[i + 4].read() for i in range(4)]
            for i in range(4):
                dl[i + 8].write_and_advance(self._mix(b1l, i))
            for i in range(4):
                dr[i + 8].write_and_advance(self._mix(b1r, i))
            b2l = [dl[i + 8].read() for i in range(4)]
            b2r = [dr[i + 8].read() for i in range(4)]
            for i in range(4):
                self.feedback[0][i] = self._mix(b2l, i)
            for i in range(4):
                self.feedback[1][i] = self._mix(b2r, i)
            s_l = ((((F(0) + b2l[0]) + b2l[1]) + b2l[2]) + b2l[3]) * F(0.125)  # iter().sum() folds from zero
            s_r = ((((F(0) + b2r[0]) + b2r[1]) + b2r[2]) + b2r[3]) * F(0.125)
            self.iir_bl = (self.iir_bl * (one - lowpass)) + s_l * lowpass
            s_l = self.iir_bl
            self.iir_br = (self.iir_br * (one - lowpass)) + (s_r * lowpass)
            s_r = self.iir_br
            mixed_l = (s_l * wet) + (dry_l * (one - wet))
            mixed_r = (s_r * wet) + (dry_r * (one - wet))
            s_l = np.where(wet < one, mixed_l, s_l)
            s_r = np.where(wet < one, mixed_r, s_r)
            f = self.fpd_l.copy()
            f ^= f << np.uint32(13)
            f ^= f >> np.uint32(17)
            f ^= f << np.uint32(5)
            s_l = s_l + self._dither(s_l, f)
            self.fpd_l = f
            f = self.fpd_r.copy()
            f ^= f << np.uint32(13)
            f ^= f >> np.uint32(17)
            f ^= f << np.uint32(5)
            s_r = s_r + self._dither(s_r, f)
            self.fpd_r = f
            out_l[:, k] = s_l
            out_r[:, k] = s_r
        return out_l, out_r


# ------------------------------------------------------------------------------------------------------------------
# the second implementation: one voice, plain Python numbers
# ------------------------------------------------------------------------------------------------------------------
def _r32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


class ScalarDelay:
    def __init__(self, n):
        self.buf = [0.0] * n
        self.pos = 0
        self.length = n


class ScalarGalactic:
    def __init__(self, f32: bool, sample_rate: int, replace, detune, brightness, bigness, wet, fpd_l: int, fpd_r: int):
        self.r = _r32 if f32 else float
        r = self.r
        self.p = [r(replace), r(detune), r(brightness), r(bigness), r(wet)]
        self.fl, self.fr = fpd_l, fpd_r
        self.vib, self.old = 3.0, 429496.7295
        self.fb = [[0.0] * 4, [0.0] * 4]
        self.ia = [0.0, 0.0]
        self.ib = [0.0, 0.0]
        lens = [int((t / 44100.0) * sample_rate) for t in GALACTIC_DELAY_TIMES]
        self.d = [[ScalarDelay(n) for n in lens], [ScalarDelay(n) for n in lens]]
        self.m = [ScalarDelay(256), ScalarDelay(256)]
        self.scale = r((1.0 / 44100.0) * sample_rate)

    @staticmethod
    def _xs(x):
        x ^= (x << 13) & 0xFFFFFFFF
        x ^= x >> 17
        x ^= (x << 5) & 0xFFFFFFFF
        return x

    def _wr(self, d, x):
        d.buf[d.pos] = x
        d.pos = (d.pos + 1) % d.length

    def _lin(self, d, idx):
        lo, hi = math.floor(idx), math.ceil(idx)
        n = len(d.buf)
        while lo >= n:
            lo -= n
            hi -= n
        if hi >= n:
            hi -= n
        r = self.r
        a, b = d.buf[lo], d.buf[hi]
        return r(a + r(r(b - a) * r(idx - math.trunc(idx))))

    def _dither(self, s, fpd):
        s32 = _r32(s)
        if s32 == 0.0 or math.isnan(s32):
            e = 0
        elif math.isinf(s32):
            e = 0xFFFFFFFF
        else:
            e = min(max(int(math.floor(_r32(math.log2(abs(s32)))) + 1), 0), 0xFFFFFFFF)
        sh = (e + 62) & 0xFFFFFFFF
        pw = (1 << sh) if sh < 64 else 0
        return self.r((float(fpd) - 2147483647.0) * 5.5e-36 * float(pw))

    def process(self, xs):
        """xs: the mono input (both channels), a sequence of numbers.  Returns ([left], [right])."""
        r = self.r
        rep, det, bri, big, wetp = self.p
        regen = r(r(0.0625) + r(r(1.0 - rep) * r(0.0625)))
        att = r(r(1.0 - r(regen / r(0.125))) * r(1.333))
        t = r(r(1.00001) - r(1.0 - bri))
        lowpass = r(r(t * t) / r(math.sqrt(self.scale)))
        drift = r(r(det * r(det * det)) * r(0.001))
        size = r(r(big * r(0.9)) + r(0.1))
        u = r(1.0 - wetp)
        wet = r(1.0 - r(u * r(u * u)))
        oml, omw = r(1.0 - lowpass), r(1.0 - wet)
        for ch in self.d:
            for d in ch:
                d.length = int(r(r(float(len(d.buf))) * size))
        outs = ([], [])
        for x in xs:
            x = r(x)
            ins = [r(self.fl * 1.18e-17) if abs(x) < 1.18e-23 else x, r(self.fr * 1.18e-17) if abs(x) < 1.18e-23 else x]
            dry = list(ins)
            self.vib += self.old * drift
            if self.vib > math.tau:
                self.vib = 0.0
                self.old = 0.4294967295 + (self.fl * 0.0000000000618)
            for c in range(2):
                self._wr(self.m[c], r(ins[c] * att))
            offs = [(math.sin(self.vib) + 1.0) * 127.0, (math.sin(self.vib + (math.pi / 2.0)) + 1.0) * 127.0]
            y = [0.0, 0.0]
            for c in range(2):
                v = self._lin(self.m[c], r(self.m[c].pos + offs[c]))
                self.ia[c] = r(r(self.ia[c] * oml) + r(v * lowpass))
                y[c] = self.ia[c]
            mix = lambda b, i: r(b[i] - r(r(b[(1 + i) % 4] + b[(2 + i) % 4]) + b[(3 + i) % 4]))  # noqa: E731
            b2 = [None, None]
            for c in range(2):
                for i in range(4):
                    self._wr(self.d[c][i], r(r(self.fb[1 - c][i] * regen) + y[c]))
            b0 = [[self.d[c][i].buf[self.d[c][i].pos] for i in range(4)] for c in range(2)]
            for c in range(2):
                for i in range(4):
                    self._wr(self.d[c][4 + i], mix(b0[c], i))
            b1 = [[self.d[c][4 + i].buf[self.d[c][4 + i].pos] for i in range(4)] for c in range(2)]
            for c in range(2):
                for i in range(4):
                    self._wr(self.d[c][8 + i], mix(b1[c], i))
            b2 = [[self.d[c][8 + i].buf[self.d[c][8 + i].pos] for i in range(4)] for c in range(2)]
            self.fb = [[mix(b2[c], i) for i in range(4)] for c in range(2)]
            nf = [self._xs(self.fl), self._xs(self.fr)]
            for c in range(2):
                s = r(r(r(r(r(0.0 + b2[c][0]) + b2[c][1]) + b2[c][2]) + b2[c][3]) * 0.125)
                self.ib[c] = r(r(self.ib[c] * oml) + r(s * lowpass))
                s = self.ib[c]
                if wet < 1.0:
                    s = r(r(s * wet) + r(dry[c] * omw))
                s = r(s + self._dither(s, nf[c]))
                outs[c].append(s)
            self.fl, self.fr = nf
        return outs
