"""BufferReader<F, U2> on interleaved two-channel Buffers: an independent numpy restatement of the node, and the plumbing the
stereo reader tests share (tests/test_stereo_reader_ref.py, tests/test_stereo_reader_abi.py, tests/test_gpu_stereo_reader.py).

THE PREMISE.  The oracle has a single-channel Buffer and BufferReader<F, U1> only.  It does not need more: the read pointer,
`finished`, the done mark and every setter of a two-channel reader do not depend on the channel, and channel c of its output
is  buf[2i + c] * (1 - mix) + buf[(2i + c + 2) mod 2n] * mix  -- which is what a one-channel reader with the same arguments
and parameter traffic renders on the de-interleaved plane c (same number of frames, same sample rate, same wrap to frame 0).
So the expected planes of a stereo bank are TWO oracle banks, one per plane, assembled as tests/sampler_pool.py assembles
pooled banks (`Planes` below).  `InterleavedReader` is what pins that premise: written from the description of the node
(one f64 read pointer, linear interpolation between frame i and frame i + 1 wrapping to 0, loop or stop at end_frame), on the
INTERLEAVED samples, and compared bit for bit with the two oracle banks on a machine without a GPU.

Past the end of a Buffer the reference is undefined (it indexes out of bounds): the restatement asserts that its integer
index stays below the Buffer's frame count, and the traffic below keeps end_frame <= n_frames (`check_in_range`)."""
from __future__ import annotations

import numpy as np

import sampler_pool as sp
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

NOT_DONE = 0xFFFFFFFF
TESIMALS = 282240000.0  # subsample units per second of the reference's Seconds type

# two-channel Buffers whose loops, `i + 1 == n` wraps and one-shot ends all fall inside the first few blocks of a 48 kHz bank
SPEC = [(37, 44100.0), (64, 48000.0), (200, 44100.0)]
SIZES = [3, 65, 130]      # a partial wavefront, one past a wavefront, two and a bit
BLOCKS = 12


def ch1(reader_index: int) -> Stage:
    """The stage that stands for output channel 1 of the BufferReader stage `reader_index`."""
    return Stage(L.STAGE_BUFFER_READER, flags=L.STAGE_FLAG_READER_CH1, input=reader_index + 1)


READER = Stage(L.STAGE_BUFFER_READER)
# the reference's buffer_player.rs voice: the stereo reader, `* amp.out([0, 0])` (a MUL_CONST per channel), both to graph out
STEREO = [READER, ch1(0), Stage(L.STAGE_MUL_CONST, input=1), Stage(L.STAGE_MUL_CONST, input=2)]
STEREO_OUTS = (2, 3)


def make_stereo_buffers(spec=SPEC, seed=11):
    """[(n_frames, sample_rate)] -> [(interleaved [n_frames, 2] f64, sample_rate)]: tones plus seeded noise, different content
    in every entry AND in the two channels of an entry."""
    left = sp.make_buffers(spec, seed)
    right = sp.make_buffers([(n, sr * 1.37) for n, sr in spec], seed + 101)  # other tones, other noise
    return [(np.stack([l, 0.8 * r], axis=1), sr) for (l, sr), (r, _) in zip(left, right)]


def plane(buffers, c):
    """The de-interleaved plane c of every entry: [(samples, sample_rate)] as the one-channel pool calls take them."""
    return [(np.ascontiguousarray(s[:, c]), sr) for s, sr in buffers]


def stereo_ctor(n, shift=0):
    """rate, looping, start_s per voice: a rate of its own, every third voice looping, every reader from frame 0 (a start
    further in would put end_frame = start + the whole Buffer past the end)."""
    u = np.arange(n) + shift
    return np.stack([0.25 + 0.03 * (u % 40), (u % 3 == 0).astype(np.float64), np.zeros(n)], axis=1)


def stereo_traffic(n, length_s):
    """sampler_pool.sampler_traffic's kinds of change (rate, duration_s, start_s, t_restart, end_s, looping) with times that are
    fractions of each voice's own Buffer length `length_s[v]`, chosen so that end_frame never passes the Buffer's end:
    duration <= 0.5 of it before any start > 0, start <= 0.4, end_s <= 0.95."""
    v = np.arange(n, dtype=np.uint32)
    rate = stereo_ctor(n)[:, 0]
    length_s = np.asarray(length_s, dtype=np.float64)

    def ev(block, bank, **kw):
        if block == 3:
            bank.param_apply_many(v, 0, 0, L.VALUE_FLOAT, rate * 2.5, **kw)                                   # rate
            bank.param_apply_many(v, 0, 3, L.VALUE_FLOAT, (0.3 + 0.2 * (v % 5) / 4.0) * length_s, **kw)       # duration_s
        if block == 5:
            bank.param_apply_many(v, 0, 2, L.VALUE_FLOAT, (0.05 + 0.35 * (v % 7) / 6.0) * length_s, **kw)     # start_s
            bank.param_apply_many(v, 0, 5, L.VALUE_TRIGGER, **kw)                                             # t_restart
        if block == 8:
            bank.param_apply_many(v[1::2], 0, 4, L.VALUE_FLOAT, (0.6 + 0.35 * (v[1::2] % 4) / 3.0) * length_s[1::2], **kw)  # end_s
            bank.param_apply_many(v, 0, 1, L.VALUE_BOOL, ivalues=(v % 2).astype(np.int64), **kw)              # looping
        if block == 10:
            bank.param_apply_many(v, 0, 5, L.VALUE_TRIGGER, **kw)
    return ev


def lengths(buffers, ids):
    """Each voice's Buffer length in seconds."""
    return np.array([buffers[e][0].shape[0] / buffers[e][1] for e in ids], dtype=np.float64)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _sat_u32(x):
    x = np.where(np.isnan(x), 0.0, x)
    return np.trunc(np.clip(x, 0.0, 4294967295.0))


def secs_to_frames(secs, sr):
    """Seconds (whole seconds + subsample units, both u32) to frames at `sr`, in f64."""
    secs = np.asarray(secs, dtype=np.float64)
    whole = _sat_u32(np.floor(secs))
    sub = _sat_u32((secs - np.trunc(secs)) * TESIMALS)
    return whole * sr + (sub * sr) / TESIMALS


class InterleavedReader:
    """n two-channel readers, voice v on the interleaved Buffer buffers[ids[v]], rendered in `dtype` at `sample_rate`.
    linked: the rate is driven per sample by a signal (the per-sample `process` path: done is marked at frame 0)."""

    def __init__(self, dtype, sample_rate, buffers, ids, ctor, linked=False):
        self.dtype, self.sr, self.linked = dtype, float(sample_rate), linked
        self.buffers = [(np.ascontiguousarray(s, dtype=np.float64).astype(dtype).reshape(-1), float(sr)) for s, sr in buffers]  # INTERLEAVED, flat
        n = len(ids)
        self.n = n
        self.entry = np.zeros(n, dtype=np.int64)
        self.nf = np.zeros(n, dtype=np.int64)
        self.bsr = np.zeros(n)
        z = np.zeros(n)
        self.rp, self.step, self.start, self.dur, self.end, self.rate = z.copy(), z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
        self.finished = np.zeros(n, dtype=bool)
        self.looping = np.zeros(n, dtype=bool)
        self.construct(np.arange(n), ids, ctor)

    def construct(self, voices, ids, ctor):
        """BufferReader::new(buffer, rate, looping).start_at(start_s) and init, for the listed voices (a FRESH reader)."""
        voices = np.asarray(voices, dtype=np.int64)
        ctor = np.asarray(ctor, dtype=np.float64).reshape(len(voices), 3)
        ids = np.broadcast_to(np.asarray(ids, dtype=np.int64), voices.shape)
        self.entry[voices] = ids
        self.nf[voices] = [self.buffers[e][0].shape[0] // 2 for e in ids]
        self.bsr[voices] = [self.buffers[e][1] for e in ids]
        self.rate[voices] = ctor[:, 0]
        self.looping[voices] = ctor[:, 1] != 0.0
        self.start[voices] = secs_to_frames(ctor[:, 2], self.bsr[voices])
        self.dur[voices] = secs_to_frames(self.nf[voices] / self.bsr[voices], self.bsr[voices])
        self.end[voices] = self.start[voices] + self.dur[voices]
        self.rp[voices] = self.start[voices]
        self.step[voices] = (self.bsr[voices] / self.sr) * self.rate[voices]
        self.finished[voices] = False

    def check_in_range(self):
        assert (self.end <= self.nf).all(), "end_frame past the Buffer's end: the reference is undefined there"

    def param_apply_many(self, voices, stages, params, kinds, fvalues=None, ivalues=None):
        v = np.asarray(voices, dtype=np.int64)
        assert np.all(np.asarray(stages) == 0)
        param = int(np.asarray(params).reshape(-1)[0])
        assert np.all(np.asarray(params) == param)
        f = None if fvalues is None else np.broadcast_to(np.asarray(fvalues, dtype=np.float64), v.shape)
        if param == 0:
            if not self.linked:  # (an ordinary change of a linked parameter is ignored while the link stands)
                self.rate[v] = f
                self.step[v] = (self.bsr[v] / self.sr) * f
        elif param == 1:
            self.looping[v] = np.broadcast_to(np.asarray(ivalues), v.shape) != 0
        elif param == 2:
            self.start[v] = secs_to_frames(f, self.bsr[v])
            self.end[v] = self.start[v] + self.dur[v]
        elif param == 3:
            self.dur[v] = secs_to_frames(f, self.bsr[v])
            self.end[v] = self.start[v] + self.dur[v]
        elif param == 4:
            self.end[v] = secs_to_frames(f, self.bsr[v])
        else:  # t_restart
            self.rp[v] = self.start[v]
            self.finished[v] = False
        self.check_in_range()

    def process_block(self, bs, driver=None):
        """-> (planes [2, n, bs] of dtype, done frames [n]).  driver [n, bs]: the signal the rate is linked to."""
        dt = self.dtype
        out = np.zeros((2, self.n, bs), dtype=dt)
        done = np.full(self.n, NOT_DONE, dtype=np.uint32)
        one = dt(1)
        width = max(b.shape[0] for b, _ in self.buffers)
        table = np.zeros((len(self.buffers), width), dtype=dt)  # the interleaved samples of every entry, a row each
        for e, (b, _) in enumerate(self.buffers):
            table[e, :b.shape[0]] = b
        two_n = np.maximum(2 * self.nf, 1)
        for f in range(bs):
            if self.linked:
                self.step = (self.bsr / self.sr) * driver[:, f].astype(np.float64)
            live = ~self.finished & (self.nf > 0)
            ip = np.trunc(self.rp)
            mix = (self.rp - ip).astype(dt)
            i = np.where(self.rp > 0.0, ip, 0.0).astype(np.int64)
            assert (i[live] < self.nf[live]).all(), "read index at or past the Buffer's last frame"
            i = np.minimum(i, np.maximum(self.nf - 1, 0))
            for c in range(2):
                # channel c of frame i is sample 2i + c; its right neighbour is sample (2i + c + 2) mod 2n
                a = table[self.entry, 2 * i + c]
                b = table[self.entry, (2 * i + c + 2) % two_n]
                y = a * (one - mix) + b * mix
                out[c, :, f] = np.where(live, y, dt(0))
            self.rp = np.where(live, self.rp + self.step, self.rp)
            hit = live & (self.rp >= self.end)
            self.rp = np.where(hit & self.looping, self.start, self.rp)
            ended = hit & ~self.looping
            self.finished |= ended
            done[ended] = 0 if self.linked else f + 1
        return out, done


# ---- the expected planes: two oracle banks per pool entry --------------------------------------------------------------------
def oracle_on(oracle, n, bs, sample_type, buffer, ctor, gain, flags=0):
    """An oracle bank (one-channel reader, `* gain`) with every voice on `buffer` = (samples of ONE plane, sample rate)."""
    o = oracle.OracleBank([Stage(L.STAGE_BUFFER_READER, flags=flags), Stage(L.STAGE_MUL_CONST)], n, sample_type, 2, False, True)
    o.set_ctor_args(0, ctor)
    o.set_ctor_args(1, np.full((n, 1), gain))
    o.set_buffer(0, buffer[0], buffer[1])
    o.init(configs.SAMPLE_RATE, bs)
    return o


class Planes:
    """sampler_pool.Expected for both planes of a pool of two-channel Buffers.  step(block) -> (planes [2, n, bs], done [n]);
    reassign(block, voices, ids, ctor_rows) before step(block): fresh readers (a swap to another entry, or a restart)."""

    def __init__(self, oracle, n, bs, sample_type, buffers, ids, ctor, traffic, gain=1.0, flags=0):
        self.oracle, self.n, self.bs, self.st, self.traffic, self.gain, self.flags = oracle, n, bs, sample_type, traffic, gain, flags
        self.planes = [plane(buffers, 0), plane(buffers, 1)]
        self.ids = np.array(ids, dtype=np.int64)
        self.gen = np.zeros(n, dtype=np.int64)
        self.ctors = {0: np.array(ctor, dtype=np.float64)}
        self.banks = {}  # (generation, entry) -> the two oracle banks
        for e in sorted(set(self.ids.tolist())):
            self.banks[(0, e)] = self._pair(e, self.ctors[0])
        self._pending = None

    def _pair(self, entry, ctor):
        return [oracle_on(self.oracle, self.n, self.bs, self.st, self.planes[c][entry], ctor, self.gain, self.flags) for c in range(2)]

    def reassign(self, block, voices, ids, ctor_rows):
        c = self.ctors.setdefault(block, np.tile([1.0, 0.0, 0.0], (self.n, 1)))
        c[voices] = ctor_rows
        self.ids[voices] = ids
        self.gen[voices] = block
        self._pending = block

    def step(self, block):
        if self._pending == block:
            for e in sorted(set(self.ids[self.gen == block].tolist())):
                self.banks[(block, e)] = self._pair(e, self.ctors[block])
            self._pending = None
            live = set(zip(self.gen.tolist(), self.ids.tolist()))
            for key in [k for k in self.banks if k not in live]:
                for b in self.banks.pop(key):
                    b.close()
        dtype = np.float64 if self.st == L.F64 else np.float32
        out = np.zeros((2, self.n, self.bs), dtype=dtype)
        done = np.full(self.n, NOT_DONE, dtype=np.uint32)
        for (g, e), pair in self.banks.items():
            mine = (self.gen == g) & (self.ids == e)
            for c, bank in enumerate(pair):
                self.traffic(block, bank)
                _, rows, _, d = bank.process_block()
                out[c][mine] = rows[mine]
                if c == 0:
                    done[mine] = d[mine]
                else:  # one node, one done mark: the two planes' readers agree
                    np.testing.assert_array_equal(d[mine], done[mine])
        return out, done

    def close(self):
        for pair in self.banks.values():
            for b in pair:
                b.close()
        self.banks = {}


def stereo_bank(knh, n, bs, sample_type, buffers, ids, ctor, mix_mode=L.MIX_TREE, stages=STEREO, outs=STEREO_OUTS, gain=1.0,
                out_channels=2, init=True, **kw):
    """A bank on a pool of two-channel Buffers: voice v on entry ids[v]; every MUL_CONST stage gets `gain`."""
    b = knh.VoiceBank(stages, n, sample_type, out_channels, mix_mode, -1, False, **kw)
    for s, st in enumerate(stages):
        if st.kind == L.STAGE_BUFFER_READER and not st.flags & L.STAGE_FLAG_READER_CH1:
            b.set_ctor_args(s, ctor)
        elif st.kind == L.STAGE_MUL_CONST:
            b.set_ctor_args(s, np.full((n, 1), gain))
    reader = next(s for s, st in enumerate(stages) if st.kind == L.STAGE_BUFFER_READER)
    for k, (s, sr) in enumerate(buffers):
        assert b.add_buffer(reader, s, sr, channels=2) == k
    b.assign_buffers(reader, np.arange(n, dtype=np.uint32), ids)
    if outs is not None:
        b.connect_outputs(*outs)
    if init:
        b.init(configs.SAMPLE_RATE, bs)
    return b


def spread_ids(n, entries=len(SPEC)):
    return (np.arange(n) % entries).astype(np.uint32)
