"""knh_bank_restart_voices: the case table and the expected-value builder (tests/test_restart_cases.py proves each case's
premise on the CPU oracle alone, tests/test_gpu_restart.py runs the cases on the device).

The expected signal is built from two reference runs.  Bank A is built with constructor arguments A and runs blocks
0 .. k - 1; at the boundary the voices R restart with arguments B.  For a voice outside R the expected signal is bank A
continuing; for a voice in R it is a FRESH bank with arguments B, whose block j is the device's block k + j.  Parameter
traffic after the boundary goes to both.  A case's hooks are called with the role of the bank they address:
    "gpu"    the bank under test
    "cont"   reference bank A (before and after the boundary)
    "fresh"  the reference bank made at the boundary
`stale` holds the calls made after block k - 1 but BEFORE the restart call: the bank under test must drop them for R, the
continuing reference keeps them, the fresh one never sees them."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np

import sampler_pool as sp
from helpers import make_gpu, make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

N = 130  # two full wavefronts and a ragged third
NOT_DONE = 0xFFFFFFFF
R_SETS = {
    "first": [0],
    "straddle": [63, 64],            # the last voice of one wavefront (and of range 0 of a two-range bank) and the first of the next
    "last": [129],
    "all": list(range(N)),
    "dup": [5, 64, 5, 129, 64],      # a voice listed twice is restarted once
    "ring": [63, 64, 129],           # 62, 65 and 128 beside them; 129's ring lies in front of the spare ring
    "range": [63, 64, 127, 128],     # ... and the last voice of range 0 of a two-range bank (128 + 2 voices) and the first of range 1
}
V = np.arange(N, dtype=np.uint32)
KF, KT, KS = L.VALUE_FLOAT, L.VALUE_TRIGGER, L.VALUE_SMOOTHING


def _none(*_a, **_k):
    return None


@dataclass
class Case:
    name: str
    stages: List[Stage]
    sample_type: int
    bs: int
    ctor_a: Dict[int, np.ndarray]
    ctor_b: Dict[int, np.ndarray]           # [n, n_args] per stage; the rows of R are used
    k: int                                   # blocks before the boundary
    n_after: int                             # blocks compared after it
    pre: Callable = _none                    # pre(bank, block, **kw): traffic before block `block` < k
    stale: Callable = _none                  # stale(bank, role): calls between block k - 1 and the restart call
    post: Callable = _none                   # post(bank, j, role, **kw): traffic before block k + j, made after the restart call
    n: int = N
    r_sets: Dict[str, List[int]] = field(default_factory=lambda: R_SETS)
    buffers: Optional[list] = None           # BufferReader pool [(samples, sr)]; every voice on entry `entry`
    entry: int = 0
    reader_stage: int = 0

    def workload(self, ctor):
        w = configs.Workload(self.name, self.stages, self.n, self.bs, self.sample_type, 2)
        w.ctor = {s: np.asarray(a, dtype=np.float64).reshape(self.n, -1) for s, a in ctor.items()}
        if self.buffers is not None:  # (the oracle takes one Buffer per bank: the entry every voice is on)
            w.buffer = (self.reader_stage, self.buffers[self.entry][0], self.buffers[self.entry][1])
        return w

    def mixed_ctor(self, rname):
        r = sorted(set(self.r_sets[rname]))
        out = {s: np.array(a, dtype=np.float64).reshape(self.n, -1) for s, a in self.ctor_a.items()}
        for s, b in self.ctor_b.items():
            out[s][r] = np.asarray(b, dtype=np.float64).reshape(self.n, -1)[r]
        return out

    def make_gpu(self, knh, ctor, mix_mode=L.MIX_LEFT_FOLD, **kw):
        w = self.workload(ctor)
        if self.buffers is None:
            return make_gpu(knh, w, mix_mode, **kw)
        b = knh.VoiceBank(w.stages, w.n_voices, w.sample_type, 2, mix_mode, -1, False, **kw)
        for s, a in w.ctor.items():
            b.set_ctor_args(s, a)
        for i, (samples, sr) in enumerate(self.buffers):
            assert b.add_buffer(self.reader_stage, samples, sr) == i
        b.assign_buffers(self.reader_stage, np.arange(self.n, dtype=np.uint32), self.entry)  # before init; the restart keeps the entry
        b.init(configs.SAMPLE_RATE, self.bs)
        return b

    def restart(self, bank, rname):
        """The two calls under test: arguments B for the voices of R, then the restart (R as listed, duplicates and all)."""
        r = np.array(sorted(set(self.r_sets[rname])), dtype=np.uint32)
        for s, b in self.ctor_b.items():
            bank.set_voice_ctor_args(s, r, np.asarray(b, dtype=np.float64).reshape(self.n, -1)[r])
        bank.restart_voices(np.array(self.r_sets[rname], dtype=np.uint32))


@dataclass
class Expected:
    before: list   # [(voices, done)] blocks 0 .. k - 1
    after: list    # [(voices, done)] blocks k .. : R from the fresh bank, the rest from A continuing
    cont: list     # [voices] bank A continuing, all voices (the premise: differs from `fresh` on R)
    fresh: list    # [voices] the fresh bank, all voices


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def build_expected(case: Case, rname: str, make_bank, step) -> Expected:
    """make_bank(workload) -> a reference bank; step(bank) -> (voices [n, bs], done [n]) of its next block."""
    r = sorted(set(case.r_sets[rname]))
    a = make_bank(case.workload(case.ctor_a))
    before = []
    for b in range(case.k):
        case.pre(a, b)
        before.append(_freeze(*step(a)))
    case.stale(a, "cont")
    f = make_bank(case.workload(case.mixed_ctor(rname)))
    after, cont, fresh = [], [], []
    for j in range(case.n_after):
        case.post(a, j, "cont")
        case.post(f, j, "fresh")
        va, da = step(a)
        vf, df = step(f)
        v, d = va.copy(), da.copy()
        v[r], d[r] = vf[r], df[r]
        after.append(_freeze(v, d))
        cont.append(_freeze(va)[0])
        fresh.append(_freeze(vf)[0])
    a.close()
    f.close()
    return Expected(before, after, cont, fresh)


def oracle_step(bank):
    _, voices, _, done = bank.process_block()
    return voices, done


def gpu_step(bank):
    _, voices, _ = bank.process_block_voices()
    return voices, bank.read_done_frames()


@functools.lru_cache(maxsize=None)
def oracle_expected(oracle, case_name: str, rname: str) -> Expected:
    """Computed once per (case, R) and shared, read-only, among the tests that need it."""
    case = CASES[case_name]
    return build_expected(case, rname, lambda w: make_oracle(oracle, w, want_mix=False), oracle_step)


# ---- the cases -------------------------------------------------------------------------------------------------------------
P = configs.voice_parameters(N)
U = (V % 7) / 7.0


def _svf(cutoff, q):
    return np.stack([np.full(N, float(L.SVF_LOW)), cutoff, q, np.zeros(N)], axis=1)


def _c3(sample_type, bs, name):
    """C3's voice, SinWt.wr_mul -> SvfFilter -> * EnvAsr, with envelopes short enough to finish before the boundary: every
    restarted voice had reported done (the pattern of free_node_when_done), then plays its next note as a new node."""
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)]
    a = {0: P["freq"], 1: np.full(N, 1.0 / N), 2: _svf(P["cutoff"], P["q"]),
         3: np.stack([0.0005 + 0.0005 * U, 0.001 + 0.0012 * U], axis=1)}           # release <= 106 frames
    b = {0: P["freq"] * 1.37 + 11.0, 1: np.full(N, 0.5 / N), 2: _svf(P["cutoff"] * 0.8 + 100.0, P["q"] + 0.3),
         3: np.stack([0.001 + 0.0005 * U, 0.002 + 0.001 * U], axis=1)}

    def pre(bank, block, **kw):
        if block == 0:
            bank.param_apply_many(V, 3, 3, KT, **kw)      # t_restart: note on
        if block == 1:
            bank.param_apply_many(V, 3, 2, KT, **kw)      # t_release: done within two blocks

    def post(bank, j, role, **kw):
        if j == 0:
            bank.param_apply_many(V, 3, 3, KT, **kw)      # the next note, on every voice
        if j == 1:
            bank.param_apply_many(V[::3], 0, 0, KF, 300.0 + V[::3], **kw)
        if j == 2:
            bank.param_apply_many(V, 3, 2, KT, **kw)
    return Case(name, st, sample_type, bs, a, b, 4, 4, pre, _none, post)


def _rings(kind, sample_type, name):
    """SinWt -> a delay with a 192-sample ring, delay of 100 samples; restarted after the rings have wrapped.  The new nodes get
    a shorter ring (0.003 s: 144 samples within the stride of 192)."""
    st = [Stage(L.STAGE_SIN_WT), Stage(kind)]
    a = {0: P["freq"], 1: np.full(N, 0.004)}
    b = {0: P["freq"] * 0.61 + 40.0, 1: np.full(N, 0.003)}
    delay = np.full(N, 100.5 / configs.SAMPLE_RATE)

    def setup(bank, **kw):
        bank.param_apply_many(V, 1, 0, KF, delay, **kw)
        if kind == L.STAGE_ALLPASS_FB_DELAY:
            bank.param_apply_many(V, 1, 1, KF, np.full(N, 0.5), **kw)

    def pre(bank, block, **kw):
        if block == 0:
            setup(bank, **kw)

    def post(bank, j, role, **kw):
        if j == 0:
            setup(bank, **kw)  # (a new node's delay is 0)
    return Case(name, st, sample_type, 64, a, b, 4, 3, pre, _none, post, r_sets={"ring": R_SETS["ring"], "all": R_SETS["all"]})


def _graph(name):
    """A graph voice of eight stages, fused at init: RandomLin drives SinWt's freq at audio rate; WhiteNoise and a BufferReader
    on a pooled buffer are added; a segment Envelope shapes the sum.  The restart changes both seeds, the reader's arguments
    and the envelope's segment count, and keeps the reader's pool entry."""
    st = [Stage(L.STAGE_RANDOM_LIN), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_SIN_WT, ar_param=1, input2=2), Stage(L.STAGE_WHITE_NOISE),
          Stage(L.STAGE_MATH_ADD, input=3, input2=4), Stage(L.STAGE_BUFFER_READER), Stage(L.STAGE_MATH_ADD, input=5, input2=6),
          Stage(L.STAGE_MUL_ENVELOPE)]

    def env(n_seg, scale):
        e = np.zeros((N, 4 + 2 * 3))
        e[:, 0], e[:, 1], e[:, 2], e[:, 3] = 0.1 * scale, 1.0, 0.0, n_seg
        e[:, 4::2] = (0.0008 + 0.0001 * (V % 5))[:, None] * np.array([1.0, 1.5, 2.0]) * scale
        e[:, 5::2] = np.array([1.0, 0.4, 0.0]) * scale
        return e
    a = {0: np.stack([V + 7.0, 300.0 + 5.0 * V], axis=1), 1: np.full(N, 800.0), 2: np.full(N, 440.0), 3: V + 1000.0,
         5: np.stack([0.5 + 0.01 * V, np.ones(N), np.zeros(N)], axis=1), 7: env(2, 1.0)}
    b = {0: np.stack([V + 5000.0, 450.0 + 3.0 * V], axis=1), 1: np.full(N, 600.0), 3: V + 90000.0,
         5: np.stack([1.0 + 0.01 * V, np.ones(N), np.full(N, 0.001)], axis=1), 7: env(3, 0.9)}

    def pre(bank, block, **kw):
        if block == 0:
            bank.param_apply_many(V, 7, 2, KT, **kw)

    def post(bank, j, role, **kw):
        if j == 0:
            bank.param_apply_many(V, 7, 2, KT, **kw)
    return Case(name, st, L.F32, 64, a, b, 3, 3, pre, _none, post, r_sets={"dup": R_SETS["dup"]},
                buffers=sp.make_buffers([(700, 22050.0), (3000, 48000.0)]), entry=1, reader_stage=5)


def _queues(name):
    """WrPreciseTiming on SinWt (its queue is resolved on the device by default) and on SvfFilter (always on the host), both
    with two delayed changes per block and a delay of 7 armed.  A change addressed to the block after next is waiting when
    the voices restart: it never appears on R.  A change made after the restart applies at frame 0 there (a new node has no
    delay armed) and at frame 7 on the continuing voices."""
    st = [Stage(L.STAGE_SIN_WT, delayed_changes_per_block=2), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF, delayed_changes_per_block=2),
          Stage(L.STAGE_MUL_ENV_ASR)]
    a = {0: P["freq"], 1: np.full(N, 1.0 / N), 2: _svf(P["cutoff"], P["q"]), 3: np.tile([0.001, 0.5], (N, 1))}
    b = {0: P["freq"] * 1.2 + 30.0, 2: _svf(P["cutoff"] * 0.7 + 50.0, P["q"])}
    seven = np.full(N, 7, dtype=np.uint16)

    def later(bank, **kw):
        bank.param_apply_many(V, 0, 0, KF, 1234.0 + V, **kw)
        bank.param_apply_many(V, 2, 0, KF, 2222.0 + V, **kw)

    def pre(bank, block, **kw):
        if block == 0:
            bank.param_apply_many(V, 3, 3, KT, **kw)
        if block == 2:  # arms the delays; they stay armed
            bank.param_apply_many(V, 0, 0, KF, 500.0 + V, None, seven, **kw)
            bank.param_apply_many(V, 2, 0, KF, 900.0 + V, None, seven, **kw)

    def stale(bank, role):
        if role == "gpu":
            later(bank, block_offset=1)  # waits for block k + 1

    def post(bank, j, role, **kw):
        if j == 0:
            bank.param_apply_many(V, 3, 3, KT, **kw)
            bank.param_apply_many(V, 0, 0, KF, 777.0 + V, **kw)
            bank.param_apply_many(V, 2, 0, KF, 1500.0 + V, **kw)
        if j == 1 and role == "cont":
            later(bank)  # what the waiting change does to a voice that goes on: at frame 7 of block k + 1
    return Case(name, st, L.F32, 64, a, b, 3, 3, pre, stale, post, r_sets={"straddle": R_SETS["straddle"], "all": R_SETS["all"]})


def _ordering(name):
    """Calls before the restart call are dropped (here: a phase offset and a frequency), the same frequency call after it is
    honoured; a WrSmoothParams ramp on the filter's cutoff is in flight at the boundary and does not continue: the new
    node has no smoothing selected, its next cutoff goes straight through."""
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF, flags=L.STAGE_FLAG_SMOOTH_PARAMS), Stage(L.STAGE_MUL_ENV_ASR)]
    a = {0: P["freq"], 1: np.full(N, 1.0 / N), 2: _svf(P["cutoff"], P["q"]), 3: np.tile([0.001, 0.5], (N, 1))}
    b = {0: P["freq"] * 0.9 + 17.0, 3: np.tile([0.002, 0.4], (N, 1))}

    def pre(bank, block, **kw):
        if block == 0:
            bank.param_apply_many(V, 3, 3, KT, **kw)
            bank.param_apply_many(V, 2, 0, KS, np.full(N, 0.01), np.ones(N, dtype=np.int64), **kw)  # cutoff: 10 ms linear, 7.5 blocks
            bank.param_apply_many(V, 2, 0, KF, P["cutoff"], **kw)
        if block == 2:
            bank.param_apply_many(V, 2, 0, KF, P["cutoff"] * 0.5, **kw)                               # in flight at the boundary

    def stale(bank, role):
        bank.param_apply_many(V, 0, 1, KF, np.full(N, 0.25))
        bank.param_apply_many(V, 0, 0, KF, 999.0 + V)

    def post(bank, j, role, **kw):
        if j == 0:
            bank.param_apply_many(V, 3, 3, KT, **kw)
            bank.param_apply_many(V, 0, 0, KF, 999.0 + V, **kw)
            bank.param_apply_many(V, 2, 0, KF, P["cutoff"] * 0.75, **kw)
    return Case(name, st, L.F32, 64, a, b, 3, 3, pre, stale, post, r_sets={"straddle": R_SETS["straddle"]})


def _frame(name):
    """SinWt and arithmetic only: the lane-per-frame forms, whose oscillators advance in closed form after each block."""
    n = 3
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MATH_MUL, input=2, input2=3)]
    v = np.arange(n)
    a = {0: 220.0 + 50.0 * v, 1: np.full(n, 0.5), 2: 3.0 + v}
    b = {0: 333.0 + 20.0 * v, 1: np.full(n, 0.25), 2: 5.0 + 2.0 * v}

    def post(bank, j, role, **kw):
        if j == 1:
            bank.param_apply_many(np.arange(n, dtype=np.uint32), 2, 0, KF, 7.0 + v, **kw)
    return Case(name, st, L.F32, 128, a, b, 3, 3, _none, _none, post, n=n, r_sets={"one": [1], "every": [0, 1, 2, 1]})


def _numeric(name):
    """Stage kinds held to a tolerance against the CPU reference elsewhere (SinNumeric's sin and powf run in the device library):
    on the device the references are device banks -- bank A continuing and a freshly initialised bank -- bit for bit."""
    st = [Stage(L.STAGE_SIN_NUMERIC), Stage(L.STAGE_ADD_CONST), Stage(L.STAGE_WR_POWF), Stage(L.STAGE_MUL_CONST)]
    a = {0: P["freq"], 1: np.full(N, 1.25), 2: 1.5 + 0.01 * V, 3: np.full(N, 1.0 / N)}
    b = {0: P["freq"] * 1.21 + 9.0, 1: np.full(N, 1.5), 2: 0.7 + 0.01 * V, 3: np.full(N, 0.5 / N)}

    def post(bank, j, role, **kw):
        if j == 1:
            bank.param_apply_many(V[::2], 0, 0, KF, 400.0 + V[::2], **kw)
    return Case(name, st, L.F32, 100, a, b, 2, 3, _none, _none, post, r_sets={"dup": R_SETS["dup"], "all": R_SETS["all"]})


CASES = {c.name: c for c in [
    _c3(L.F32, 64, "c3_f32_64"), _c3(L.F32, 100, "c3_f32_100"), _c3(L.F64, 64, "c3_f64_64"), _c3(L.F64, 100, "c3_f64_100"),
    _rings(L.STAGE_SAMPLE_DELAY, L.F32, "sample_delay_f32"), _rings(L.STAGE_SAMPLE_DELAY, L.F64, "sample_delay_f64"),
    _rings(L.STAGE_ALLPASS_DELAY, L.F32, "allpass_f32"), _rings(L.STAGE_ALLPASS_FB_DELAY, L.F32, "allpass_fb_f32"),
    _rings(L.STAGE_ALLPASS_FB_DELAY, L.F64, "allpass_fb_f64"),
    _graph("graph"), _queues("queues"), _ordering("ordering"), _frame("frame"), _numeric("numeric"),
]}
PAIRS = [(name, r) for name, c in CASES.items() for r in c.r_sets]
