"""KNH_STAGE_FLAG_ENV_SOURCE -- EnvAsr, EnvAr and Envelope as source stages: the oracle twin and the case table
(tests/test_env_source_twin.py pins the twin on the CPU, tests/test_gpu_env_source.py runs the cases on the device).

The oracle does not know the flag.  The TWIN of a descriptor spells the same voice the way it could be spelled before the
flag existed: every ENV_SOURCE stage becomes KNH_STAGE_INPUT (channel 0 of a one-channel bank input that is all ones)
followed by the same stage without the flag -- `1.0 * env`, which is `env` exactly -- and every `input` / `input2` index is
shifted for the inserted stages.  An index that named the source names the MUL_ENV_* stage of the twin (never the INPUT
stage: the oracle refuses links from a graph input); wrapper stages behind it follow it as they did.  A case's traffic is
written once, against the stage indices of the descriptor under test; TwinBank maps them."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np

from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

SR = configs.SAMPLE_RATE
ES = L.STAGE_FLAG_ENV_SOURCE
NOT_DONE = 0xFFFFFFFF
KF, KT, KI = L.VALUE_FLOAT, L.VALUE_TRIGGER, L.VALUE_INTEGER
ENV_KINDS = (L.STAGE_MUL_ENV_ASR, L.STAGE_MUL_ENV_AR, L.STAGE_MUL_ENVELOPE)


def is_source(s: Stage) -> bool:
    return s.kind in ENV_KINDS and bool(s.flags & ES)


def twin(stages):
    """-> (the twin's stages, smap): smap[i] = the twin's index of stage i (of the MUL_ENV_* stage for a source)."""
    out, smap = [], []
    for s in stages:
        if is_source(s):
            out.append(Stage(L.STAGE_INPUT))
        smap.append(len(out))
        out.append(s)
    shift = lambda k: 0 if k == 0 else 1 + smap[k - 1]
    for i, s in zip(smap, stages):
        out[i] = Stage(s.kind, s.flags & ~ES, s.delayed_changes_per_block, shift(s.input), shift(s.input2), s.ar_param)
    return out, smap


class TwinBank:
    """The oracle bank of a descriptor's twin with the call surface the cases' traffic uses, stage indices mapped."""

    def __init__(self, oracle, stages, n, sample_type, ctor, bs, sr=SR, want_mix=True):
        self.stages, self.smap = twin(stages)
        self.n, self.bs = n, bs
        self.o = oracle.OracleBank(self.stages, n, sample_type, 1, want_mix, True)
        self.has_input = len(self.stages) != len(stages)
        if self.has_input:
            self.o.set_in_channels(1)
        for i, s in enumerate(self.stages):
            if s.kind == L.STAGE_INPUT:
                self.o.set_ctor_args(i, np.zeros((n, 1)))  # channel 0
        for s, a in ctor.items():
            self.o.set_ctor_args(self.smap[s], a)
        self.o.init(sr, bs)
        self.ones = np.ones((1, bs), dtype=self.o.dtype)

    def param_apply_many(self, voices, stage, param, kinds, fvalues=None, ivalues=None, delays=None):
        self.o.param_apply_many(voices, self.smap[stage], param, kinds, fvalues, ivalues, delays)

    def param_apply(self, voice, stage, param, value):
        self.o.param_apply(voice, self.smap[stage], param, value)

    def process_block(self):
        """-> (mix [1, bs], voices [n, bs], flags, done [n])"""
        if self.has_input:
            self.o.set_input(self.ones)
        return self.o.process_block()

    def close(self):
        self.o.close()


# ---- the cases -------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    stages: List[Stage]
    ctor: Callable                      # ctor(n) -> {stage: [n, n_args]}
    traffic: Callable                   # traffic(bank, block, n): the parameter calls made before `block`
    silencers: tuple = ()               # (stage, restart param) of the multiplying envelopes: what ALL_DONE follows
    bs: int = 96
    blocks: int = 8
    outs: Optional[tuple] = None        # the two connected outputs (knh_bank_connect_outputs)
    tol: float = 0.0                    # 0: bit for bit


def spread(n, lo, hi, mul=1):
    """n values from lo to hi, dealt to the voices so that neighbours differ (mul is odd and prime to n's usual factors)"""
    k = (np.arange(n) * mul) % n
    return lo + (hi - lo) * k / max(1, n - 1)


def env_times(n, mul=37, release_hi=0.006):
    """attack 0.1 .. 4 ms, release 0.2 .. 6 ms, spread so that state changes land on every tile position and Attacking,
    Sustaining, Releasing and Stopped lanes share wavefronts"""
    return np.stack([spread(n, 0.0001, 0.004, mul), spread(n, 0.0002, release_hi, mul + 22)], axis=1)


def _v(n):
    return np.arange(n, dtype=np.uint32)


def note_traffic(src, src_restart, asr=None, src_release=None):
    """The timing every case shares.  src: the source stage (src_restart its t_restart parameter, src_release its t_release
    if it is an EnvAsr); asr: a multiplying EnvAsr (the amplitude envelope), or None.
    block 0: every envelope starts.  block 2: t_release for a third of the voices, half of them at an offset inside the block
    (the stage has delayed_changes_per_block = 2).  block 4: t_restart for some of the released voices (their long releases
    are still running) and for every fifth source.  block 5: every EnvAsr is released, so that most voices report done inside the run."""
    def traffic(bank, block, n):
        v = _v(n)
        third = v[v % 3 == 0]
        delays = ((third * 7) % 90 + 1).astype(np.uint16) * (third % 2 == 0)
        if block == 0:
            bank.param_apply_many(v, src, src_restart, KT)
            if asr is not None:
                bank.param_apply_many(v, asr, 3, KT)
        if block == 2:
            for stage in (asr, src if src_release is not None else None):
                if stage is not None:
                    bank.param_apply_many(third, stage, 2, KT, delays=delays)
        if block == 4:
            some = v[v % 6 == 0]
            if asr is not None:
                bank.param_apply_many(some, asr, 3, KT)
            if src_release is not None:
                bank.param_apply_many(some, src, src_restart, KT)
            else:
                bank.param_apply_many(v[v % 5 == 0], src, src_restart, KT)
        if block == 5:
            if asr is not None:
                bank.param_apply_many(v, asr, 2, KT)
            if src_release is not None:
                bank.param_apply_many(v, src, src_release, KT)
    return traffic


# 1. the pitch envelope: EnvAr.wr-less -> * 300 -> + 110 -> SinWt.ar_params(freq) -> * EnvAsr
PITCH = [Stage(L.STAGE_MUL_ENV_AR, flags=ES), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST),
         Stage(L.STAGE_SIN_WT, flags=L.STAGE_FLAG_AR_FREQ), Stage(L.STAGE_MUL_ENV_ASR, delayed_changes_per_block=2)]


def pitch_ctor(n):
    # the amplitude envelopes' releases end at 4 ms: released in block 5 -- at the offset of up to 90 frames that stays set
    # from block 2 -- they have all run out by the end of block 7 (90 + 192 of the 288 frames left), so ALL_DONE comes on
    # inside the run; the sources keep the full 0.2 .. 6 ms
    return {0: env_times(n), 1: np.full((n, 1), 300.0), 2: (110.0 + 3.0 * np.arange(n)).reshape(n, 1), 3: np.full((n, 1), 110.0),
            4: env_times(n, 41, 0.004)}


# 2. an envelope alone with wrappers: EnvAsr.wr_mul(3000).wr_add(200); wr_mul changes mid-run
WRAPPED = [Stage(L.STAGE_MUL_ENV_ASR, flags=ES, delayed_changes_per_block=2), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_WR_ADD)]


def wrapped_ctor(n):
    return {0: env_times(n), 1: np.full((n, 1), 3000.0), 2: np.full((n, 1), 200.0)}


def wrapped_traffic(bank, block, n):
    note_traffic(0, 3, None, src_release=2)(bank, block, n)
    if block == 3:
        bank.param_apply_many(_v(n)[::2], 1, 0, KF, 1000.0 + 10.0 * _v(n)[::2])


# 3. a graph voice: the sound (SinWt * EnvAsr), then EnvAr -> * 0.5 -> + 0.25 driving the value of a gain on the sound
GAIN = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_ENV_ASR, delayed_changes_per_block=2),
        Stage(L.STAGE_MUL_ENV_AR, flags=ES), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST),
        Stage(L.STAGE_MUL_CONST, input=2, ar_param=1, input2=5)]


def gain_ctor(n):
    return {0: (220.0 + 5.0 * np.arange(n)).reshape(n, 1), 1: env_times(n, 41, 0.004), 2: env_times(n), 3: np.full((n, 1), 0.5),
            4: np.full((n, 1), 0.25), 5: np.full((n, 1), 1.0)}


# 4. the filter envelope: the same, the envelope on SvfFilter's cutoff_freq (200 .. 3200 Hz)
FILTER = GAIN[:5] + [Stage(L.STAGE_SVF, input=2, ar_param=1, input2=5)]


def filter_ctor(n):
    c = gain_ctor(n)
    c[3], c[4] = np.full((n, 1), 3000.0), np.full((n, 1), 200.0)
    c[5] = np.tile([float(L.SVF_LOW), 1000.0, 0.9, 0.0], (n, 1))
    return c


# 5. one envelope read twice: EnvAsr; sine * env; and env * 400 onto the freq of a second oscillator
TWICE = [Stage(L.STAGE_MUL_ENV_ASR, flags=ES, delayed_changes_per_block=2), Stage(L.STAGE_SIN_WT),
         Stage(L.STAGE_MATH_MUL, input=2, input2=1), Stage(L.STAGE_MUL_CONST, input=1),
         Stage(L.STAGE_SIN_WT, ar_param=1, input2=4), Stage(L.STAGE_MATH_ADD, input=3, input2=5)]


def twice_ctor(n):
    return {0: env_times(n), 1: (330.0 + 2.0 * np.arange(n)).reshape(n, 1), 3: np.full((n, 1), 400.0), 4: np.full((n, 1), 55.0)}


# 6. the segment Envelope as a source, on SinWt's freq: 3 segments, looping on half the voices
SEG = [Stage(L.STAGE_MUL_ENVELOPE, flags=ES), Stage(L.STAGE_SIN_WT, flags=L.STAGE_FLAG_AR_FREQ)]


def seg_ctor(n):
    # Envelope: start_value, time_scale, looping, n_segments, then (duration, value) per segment
    v = np.arange(n)
    a = np.zeros((n, 4 + 2 * 3))
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = 100.0, 1.0, v % 2, 3
    a[:, 4], a[:, 5] = 0.0005 + 0.00003 * (v % 31), 900.0 + 4.0 * v
    a[:, 6], a[:, 7] = 0.0011 + 0.00007 * (v % 17), 300.0
    a[:, 8], a[:, 9] = 0.0023 + 0.00005 * (v % 23), 150.0 + v
    return {0: a, 1: np.full((n, 1), 100.0)}


def seg_traffic(bank, block, n):
    v = _v(n)
    if block == 0:
        bank.param_apply_many(v, 0, 2, KT)              # t_restart
    if block == 2:
        bank.param_apply_many(v[::3], 0, 0, KF, 0.5 + 0.01 * (v[::3] % 50))  # time_scale
    if block == 3:
        bank.param_apply_many(v[1::4], 0, 3, KT)        # t_stop
    if block == 5:
        bank.param_apply_many(v[::5], 0, 2, KT)


# 7. the source's own attack_time at audio rate, driven by a Phasor (0 .. 1 -> 0.2 .. 2.2 ms)
AR_ATTACK = [Stage(L.STAGE_PHASOR), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST),
             Stage(L.STAGE_MUL_ENV_ASR, flags=ES, ar_param=1, input2=3)]


def ar_attack_ctor(n):
    return {0: (200.0 + 13.0 * np.arange(n)).reshape(n, 1), 1: np.full((n, 1), 0.002), 2: np.full((n, 1), 0.0002), 3: env_times(n)}


CASES: Dict[str, Case] = {c.name: c for c in [
    Case("pitch", PITCH, pitch_ctor, note_traffic(0, 2, 4), silencers=((4, 3),)),
    Case("pitch64", PITCH, pitch_ctor, note_traffic(0, 2, 4), silencers=((4, 3),), bs=64, blocks=12),
    Case("wrapped", WRAPPED, wrapped_ctor, wrapped_traffic),
    Case("gain", GAIN, gain_ctor, note_traffic(2, 2, 1), silencers=((1, 3),)),
    Case("filter", FILTER, filter_ctor, note_traffic(2, 2, 1), silencers=((1, 3),), tol=2e-4),
    Case("twice", TWICE, twice_ctor, note_traffic(0, 3, None, src_release=2)),
    Case("segments", SEG, seg_ctor, seg_traffic),
    Case("ar_attack", AR_ATTACK, ar_attack_ctor, note_traffic(3, 3, None, src_release=2)),
    Case("stereo", GAIN, gain_ctor, note_traffic(2, 2, 1), silencers=((1, 3),), outs=(2, 5)),
]}


class SilenceTracker:
    """THE RULE (knaster_hip.h, KNH_STAGE_FLAG_ENV_SOURCE): ALL_DONE describes silence.  A voice runs from a t_restart of a
    multiplying envelope until that envelope reports done; the oracle does not compute ALL_DONE, so the rule is kept here, on
    a bank that holds nothing but the voice's multiplying envelopes (INPUT on ones, then each of them), driven by the same
    traffic.  A voice whose only finishing stages are envelope sources never reports ALL_DONE."""

    def __init__(self, oracle, case: Case, n, sample_type):
        self.case, self.n = case, n
        self.stage_of = {}
        st = [Stage(L.STAGE_INPUT)]
        for s, _ in case.silencers:
            self.stage_of[s] = len(st)
            st.append(Stage(case.stages[s].kind, 0, case.stages[s].delayed_changes_per_block))
        self.running = np.zeros(n, dtype=bool)
        self.o = None
        if case.silencers:
            self.o = oracle.OracleBank(st, n, sample_type, 1, False, True)
            self.o.set_in_channels(1)
            self.o.set_ctor_args(0, np.zeros((n, 1)))
            c = case.ctor(n)
            for s, k in self.stage_of.items():
                self.o.set_ctor_args(k, c[s])
            self.o.init(SR, case.bs)

    def param_apply_many(self, voices, stage, param, kinds, fvalues=None, ivalues=None, delays=None):
        if stage not in self.stage_of:
            return
        self.o.param_apply_many(voices, self.stage_of[stage], param, kinds, fvalues, ivalues, delays)
        if (stage, param) in self.case.silencers:
            self.running[np.asarray(voices)] = True

    def all_done_after_block(self, block) -> bool:
        if self.o is None:
            return False
        self.case.traffic(self, block, self.n)
        self.o.set_input(np.ones((1, self.case.bs), dtype=self.o.dtype))
        _, _, _, done = self.o.process_block()
        self.running &= done == NOT_DONE
        return not self.running.any()

    def close(self):
        if self.o is not None:
            self.o.close()


@dataclass
class Run:
    voices: np.ndarray   # [blocks, n, bs] ([blocks, 2, n, bs] with connected outputs)
    mix: np.ndarray      # [blocks, planes, bs] left fold
    any_done: list       # per block
    done: np.ndarray     # [blocks, n]
    all_done: list       # per block, by the rule


def _left_fold(rows):
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = acc + r
    return acc


@functools.lru_cache(maxsize=None)
def twin_run(oracle, name: str, n: int, sample_type: int) -> Run:
    """The oracle twin's run of a case, computed once and shared read-only.  A voice with two connected outputs is two twins:
    the descriptor up to each output's node (a voice's signal is its last stage's)."""
    case = CASES[name]
    ctor = case.ctor(n)
    if case.outs is None:
        ends = [len(case.stages)]
    else:
        ends = []
        for o in case.outs:
            e = o + 1
            while e < len(case.stages) and case.stages[e].kind in WRAPPERS:
                e += 1
            ends.append(e)
    banks = [TwinBank(oracle, case.stages[:e], n, sample_type, {s: a for s, a in ctor.items() if s < e}, case.bs, want_mix=False) for e in ends]
    full = banks[ends.index(max(ends))]  # the twin that holds every envelope: its done frames are the voice's
    rule = SilenceTracker(oracle, case, n, sample_type)
    voices, mix, any_done, done, all_done = [], [], [], [], []
    for b in range(case.blocks):
        planes = []
        for bank, e in zip(banks, ends):
            case.traffic(_Upto(bank, e), b, n)
            _, v, f, d = bank.process_block()
            planes.append(np.array(v))
            if bank is full:
                any_done.append(bool(f & L.FLAG_ANY_DONE))
                done.append(np.array(d))
        voices.append(planes[0] if case.outs is None else np.stack(planes))
        mix.append(np.stack([_left_fold(p) for p in planes]))
        all_done.append(rule.all_done_after_block(b))
    for bank in banks:
        bank.close()
    rule.close()
    run = Run(np.stack(voices), np.stack(mix), any_done, np.stack(done), all_done)
    for a in (run.voices, run.mix, run.done):
        a.setflags(write=False)
    return run


WRAPPERS = (L.STAGE_WR_MUL, L.STAGE_WR_ADD, L.STAGE_WR_SUB, L.STAGE_WR_VSUB, L.STAGE_WR_DIV, L.STAGE_WR_VDIV, L.STAGE_WR_POWF, L.STAGE_WR_POWI)


class _Upto:
    """a bank that holds the stages before `end` only: calls to later stages are not for it"""

    def __init__(self, bank, end):
        self.bank, self.end = bank, end

    def param_apply_many(self, voices, stage, *a, **kw):
        if stage < self.end:
            self.bank.param_apply_many(voices, stage, *a, **kw)


def make_gpu(knh, case: Case, n, sample_type, mix_mode=L.MIX_LEFT_FOLD, stages=None, ctor=None):
    stages = case.stages if stages is None else stages
    b = knh.VoiceBank(stages, n, sample_type, 2 if case.outs else 1, mix_mode)
    for s, a in (case.ctor(n) if ctor is None else ctor).items():
        b.set_ctor_args(s, a)
    if case.outs:
        b.connect_outputs(*case.outs)
    b.init(SR, case.bs)
    return b
