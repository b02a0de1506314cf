"""Plumbing of the BufferReader pool tests: the pooled sampler bank, and its expected signal assembled from oracle banks.

The oracle takes one Buffer per bank.  The expected signal of a pooled bank is therefore made of one oracle bank per pool
entry -- all voices on that entry, same constructor arguments and parameter traffic -- of whose per-voice output only the
rows of the voices assigned to that entry are kept.  A voice that is given another entry while the bank runs continues, from
that block on, as its row of a FRESH oracle bank on the new entry (the reference frees the old node and pushes a new one)."""
from __future__ import annotations

import functools

import numpy as np

from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

STAGES = [Stage(L.STAGE_BUFFER_READER), Stage(L.STAGE_MUL_CONST)]
NOT_DONE = 0xFFFFFFFF


def make_buffers(spec, seed=11):
    """[(n_frames, sample_rate)] -> [(samples f64, sample_rate)]: tones and noise, different in every entry."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (n, sr) in enumerate(spec):
        t = np.arange(n) / sr
        s = 0.5 * np.sin(2 * np.pi * (200.0 + 170.0 * k) * t + k) + 0.3 * np.sin(2 * np.pi * (1234.5 + 99.0 * k) * t) + 0.15 * rng.uniform(-1, 1, n)
        out.append((s, float(sr)))
    return out


def sampler_ctor(n, shift=0):
    """rate, looping, start_s per voice as tests/test_gpu_parity.py::test_buffer_reader_sampler_bank has them (`shift` moves
    the pattern along the voices: the constructor arguments of a reassignment)."""
    v = np.arange(n, dtype=np.uint32)
    u = v + shift
    rate = 0.25 + 0.03 * u
    looping = (u % 3 == 0).astype(np.float64)
    start = np.where(u % 4 == 0, 0.011 + 0.0001 * u, 0.0)
    return np.stack([rate, looping, start], axis=1)


def sampler_traffic(n):
    """The parameter traffic of the existing sampler test: events(block, bank)."""
    v = np.arange(n, dtype=np.uint32)
    rate = sampler_ctor(n)[:, 0]

    def ev(block, bank, **kw):
        if block == 3:
            bank.param_apply_many(v, 0, 0, L.VALUE_FLOAT, rate * 2.5, **kw)                   # rate
            bank.param_apply_many(v[::2], 0, 3, L.VALUE_FLOAT, 0.004 + 0.0002 * v[::2], **kw)  # duration_s
        if block == 5:
            bank.param_apply_many(v, 0, 2, L.VALUE_FLOAT, 0.02 + 0.0001 * v, **kw)           # start_s
            bank.param_apply_many(v, 0, 5, L.VALUE_TRIGGER, **kw)                             # t_restart
        if block == 8:
            bank.param_apply_many(v[1::2], 0, 4, L.VALUE_FLOAT, 0.05 + 0.0001 * v[1::2], **kw)  # end_s
            bank.param_apply_many(v, 0, 1, L.VALUE_BOOL, ivalues=(v % 2).astype(np.int64), **kw)  # looping
        if block == 10:
            bank.param_apply_many(v, 0, 5, L.VALUE_TRIGGER, **kw)
    return ev


def pooled_bank(knh, n, bs, sample_type, buffers, ids, ctor, mix_mode=L.MIX_TREE, stages=STAGES, gain=None, **kw):
    """A sampler bank on a pool: every buffer added in order, voice v on entry ids[v]."""
    b = knh.VoiceBank(stages, n, sample_type, 2, mix_mode, -1, False, **kw)
    b.set_ctor_args(0, ctor)
    b.set_ctor_args(1, np.full((n, 1), (1.0 / n) if gain is None else gain))
    for k, (s, sr) in enumerate(buffers):
        assert b.add_buffer(0, s, sr) == k
    b.assign_buffers(0, np.arange(n, dtype=np.uint32), ids)
    b.init(configs.SAMPLE_RATE, bs)
    return b


def oracle_on(oracle, n, bs, sample_type, buffer, ctor, stages=STAGES):
    """An oracle bank with every voice on `buffer` (per-voice output only)."""
    o = oracle.OracleBank(stages, n, sample_type, 2, False, True)
    o.set_ctor_args(0, ctor)
    o.set_ctor_args(1, np.full((n, 1), 1.0 / n))
    o.set_buffer(0, buffer[0], buffer[1])
    o.init(configs.SAMPLE_RATE, bs)
    return o


def left_fold(rows):
    """KNH_MIX_LEFT_FOLD: the voices added one after the other in voice order, in the rows' own precision."""
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = acc + r
    return acc


class Expected:
    """The assembled oracle: per block, the per-voice rows and done frames of a pooled bank whose voices may be given other
    entries at block boundaries.  step(block) -> (voices [n, bs], done [n])."""

    def __init__(self, oracle, n, bs, sample_type, buffers, ids, ctor, traffic):
        self.oracle, self.n, self.bs, self.st, self.buffers, self.traffic = oracle, n, bs, sample_type, buffers, traffic
        self.ids = np.array(ids, dtype=np.int64)
        self.gen = np.zeros(n, dtype=np.int64)  # the block at which the voice's current reader was made
        self.banks = {}                          # (generation, entry) -> oracle bank
        self.ctors = {0: np.array(ctor)}
        for e in sorted(set(self.ids.tolist())):
            self.banks[(0, e)] = oracle_on(oracle, n, bs, sample_type, buffers[e], ctor)

    def reassign(self, block, voices, ids, ctor_rows):
        """Before step(block): these voices get fresh readers on entries `ids`, constructor arguments `ctor_rows`."""
        c = self.ctors.setdefault(block, np.tile([1.0, 0.0, 0.0], (self.n, 1)))
        c[voices] = ctor_rows
        self.ids[voices] = ids
        self.gen[voices] = block
        self._pending = block

    def step(self, block):
        if getattr(self, "_pending", None) == block:  # the fresh banks of this block's reassignments, started now
            for e in sorted(set(self.ids[self.gen == block].tolist())):
                self.banks[(block, e)] = oracle_on(self.oracle, self.n, self.bs, self.st, self.buffers[e], self.ctors[block])
            self._pending = None
            live = set(zip(self.gen.tolist(), self.ids.tolist()))
            for key in [k for k in self.banks if k not in live]:
                self.banks.pop(key).close()
        dtype = np.float64 if self.st == L.F64 else np.float32
        voices = np.zeros((self.n, self.bs), dtype=dtype)
        done = np.full(self.n, NOT_DONE, dtype=np.uint32)
        for (g, e), bank in self.banks.items():
            self.traffic(block, bank)
            _, rows, _, d = bank.process_block()
            mine = (self.gen == g) & (self.ids == e)
            voices[mine] = rows[mine]
            done[mine] = d[mine]
        return voices, done

    def close(self):
        for b in self.banks.values():
            b.close()
        self.banks = {}


# ---- test 1's scenario, computed once per sample type and shared (read-only) --------------------------------------------
POOL_SPEC = [(2, 8000.0), (3, 22050.0), (64, 44100.0), (3000, 48000.0), (4099, 96000.0)]
POOL_N, POOL_BS, POOL_BLOCKS = 130, 64, 14


def pool_ids(n=POOL_N):
    return (np.arange(n) % len(POOL_SPEC)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def pool_reference(oracle, sample_type):
    """[(voices, done)] per block of the pool parity scenario."""
    buffers = make_buffers(POOL_SPEC)
    x = Expected(oracle, POOL_N, POOL_BS, sample_type, buffers, pool_ids(), sampler_ctor(POOL_N), sampler_traffic(POOL_N))
    blocks = []
    for b in range(POOL_BLOCKS):
        voices, done = x.step(b)
        voices.setflags(write=False)
        done.setflags(write=False)
        blocks.append((voices, done))
    x.close()
    return tuple(blocks)
