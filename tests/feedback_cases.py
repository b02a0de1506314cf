"""Voices with feedback edges (KNH_STAGE_FLAG_FEEDBACK): the test voices of tests/test_feedback_abi.py and
tests/test_gpu_feedback.py, and their expected signals from the CPU oracle with the loop closed OUTSIDE it.

The oracle has no feedback edge.  For a voice list S with m feedback sources, the twin list S' has a plain KNH_STAGE_INPUT in
the place of source k, on a bank input channel of its own.  Per voice there is one one-voice OracleBank on S' (and on every
prefix S'[0 .. p] whose last stage's signal is wanted: the tapped node outputs, a connected output); prefixes are
self-contained because the stages are in dependency order.  Block b's input on edge k's channel is the tap's block b - 1, zeros
for b = 0: the contract of graph.rs:153-155 and graph_tests.rs:185-254, a delay of exactly one block."""
from __future__ import annotations

import numpy as np

from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

SR = configs.SAMPLE_RATE
KF = L.VALUE_FLOAT
FB = L.STAGE_FLAG_FEEDBACK
WRAPPERS = (L.STAGE_WR_MUL, L.STAGE_WR_ADD, L.STAGE_WR_SUB, L.STAGE_WR_VSUB, L.STAGE_WR_DIV, L.STAGE_WR_VDIV, L.STAGE_WR_POWF, L.STAGE_WR_POWI)


def fb(tap):
    """The source of a feedback edge from stage `tap` (its index in the list)."""
    return Stage(L.STAGE_INPUT, flags=FB, input=tap + 1)


def is_fb(s):
    return s.kind == L.STAGE_INPUT and bool(s.flags & FB)


def node_output(stages, k):
    while k + 1 < len(stages) and stages[k + 1].kind in WRAPPERS:
        k += 1
    return k


class Case:
    """stages, ctor {stage: [n, args]}, the bank inputs the voice reads beside its edges, what is fired before block 0."""

    def __init__(self, name, stages, ctor, n, in_channels=0, outs=None):
        self.name, self.stages, self.ctor, self.n, self.in_channels, self.outs = name, list(stages), ctor, n, in_channels, outs
        self.silencers = ()  # (stage, restart parameter) of the multiplying envelopes: what KNH_FLAG_ALL_DONE follows
        self.edges = [i for i, s in enumerate(self.stages) if is_fb(s)]
        self.taps = [node_output(self.stages, self.stages[i].input - 1) for i in self.edges]

    def workload(self, sample_type, bs):
        w = configs.Workload(self.name, self.stages, self.n, bs, sample_type, 2)
        w.ctor = dict(self.ctor)
        w.in_channels = self.in_channels
        return w

    def start(self, bank):
        """Calls before block 0, on the device bank and on the closed-loop oracle alike (voice indices are the bank's)."""


# ---- the reference's two vectors (graph_tests.rs:185-254), TestInPlusParamUGen as ADD_CONST ------------------------------------
def vector_later(n=1):
    st = [fb(2), Stage(L.STAGE_ADD_CONST), Stage(L.STAGE_ADD_CONST)]
    return Case("feedback_nodes", st, {1: np.full((n, 1), 1.25), 2: np.full((n, 1), 0.125)}, n)


def vector_earlier(n=1):
    st = [Stage(L.STAGE_INPUT), Stage(L.STAGE_ADD_CONST), fb(1), Stage(L.STAGE_ADD_CONST)]
    return Case("feedback_nodes2", st, {0: np.zeros((n, 1)), 1: np.full((n, 1), 1.25), 3: np.full((n, 1), 0.125)}, n, in_channels=1)


VECTOR_LATER = (1.375, 2.75, 4.125)
VECTOR_EARLIER = (0.125, 1.375, 1.375)


# ---- the comb: SinWt * EnvAsr + 0.6 * fb -> SampleDelay(d) -> tap ------------------------------------------------------------
class Comb(Case):
    GAIN_STAGE, DELAY_STAGE, ENV_STAGE = 3, 5, 1

    def __init__(self, n, attack=0.001, release=0.002):
        w = configs.feedback_comb(n, 64)
        ctor = dict(w.ctor)
        ctor[1] = np.tile([attack, release], (n, 1))  # short enough to finish inside a test
        ctor[6] = np.full((n, 1), 0.5)
        super().__init__("comb", w.stages, ctor, n)
        self.silencers = ((self.ENV_STAGE, 3),)
        self.delays = w.param_sets[0][2]

    def start(self, bank, voices=None):
        v = np.arange(self.n, dtype=np.uint32) if voices is None else np.asarray(voices, dtype=np.uint32)
        bank.param_apply_many(v, self.DELAY_STAGE, 0, KF, self.delays[v])
        bank.param_apply_many(v, self.ENV_STAGE, 3, L.VALUE_TRIGGER)  # t_restart


# ---- feedback FM: the operator's own output, one block late, on its phase_offset ------------------------------------------------
def fm(n):
    p = configs.voice_parameters(n)
    st = [fb(3), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_SIN_WT, ar_param=2, input2=2), Stage(L.STAGE_MUL_CONST)]
    # (phase_offset counts entries of the 16 384-entry table: an index of some hundreds is a tenth of a cycle at full swing)
    ctor = {1: (300.0 + 250.0 * (np.arange(n) % 7)).reshape(n, 1), 2: p["freq"].reshape(n, 1), 3: np.full((n, 1), 0.9)}
    return Case("fm", st, ctor, n)


# ---- two crossed edges: two one-pole branches, each fed from the other --------------------------------------------------------
def crossed(n, connected=False):
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT),
          fb(8), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_MATH_ADD, input=1, input2=3), Stage(L.STAGE_ONEPOLE_LPF),   # branch A: 4
          fb(4), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_MATH_ADD, input=1, input2=7), Stage(L.STAGE_ONEPOLE_LPF),   # branch B: 8
          Stage(L.STAGE_MATH_ADD, input=5, input2=9), Stage(L.STAGE_MUL_CONST)]
    ctor = {0: p["freq"].reshape(n, 1), 2: np.full((n, 1), 0.5), 4: p["cutoff"].reshape(n, 1), 6: np.full((n, 1), -0.4),
            8: (p["cutoff"] * 0.5).reshape(n, 1), 10: np.full((n, 1), 0.5)}
    return Case("crossed", st, ctor, n, outs=(4, 8) if connected else None)


# ---- a voice whose signal IS an edge's source, behind its tap: the device list ends in the edge's write, not in the voice's signal ----
def tail(n):
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), fb(1)]
    return Case("tail", st, {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 0.5)}, n)


# ---- a loop in a voice of more than sixteen device ops: the kernel visits eight samples at a time, every tile as 16-byte pieces ----
def long_loop(n):
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT), fb(18), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_MATH_ADD, input=1, input2=3)]
    ctor = {0: p["freq"].reshape(n, 1), 2: np.full((n, 1), 0.5)}
    for k in range(14):  # gains that cancel in pairs: the loop gain stays 0.5
        ctor[len(st)] = np.full((n, 1), 1.25 if k % 2 == 0 else 0.8)
        st.append(Stage(L.STAGE_MUL_CONST))
    ctor[len(st)] = p["cutoff"].reshape(n, 1)
    st.append(Stage(L.STAGE_ONEPOLE_LPF))  # stage 18: the tap
    ctor[len(st)] = np.full((n, 1), 0.5)
    st.append(Stage(L.STAGE_MUL_CONST))
    assert len(st) == 20 and st[18].kind == L.STAGE_ONEPOLE_LPF
    return Case("long", st, ctor, n)


# ---- the closed loop ---------------------------------------------------------------------------------------------------------
class _VoiceLoop:
    """One voice: a one-voice OracleBank on S' and on each prefix of it that a tap or a view ends."""

    def __init__(self, oracle, case, v, sample_type, bs, views, cut_edges):
        self.case, self.bs = case, bs
        self.dtype = np.float64 if sample_type == L.F64 else np.float32
        m = len(case.edges)
        self.in_channels = case.in_channels + m
        twin = list(case.stages)
        for k, i in enumerate(case.edges):
            twin[i] = Stage(L.STAGE_INPUT)
        self.ends = sorted(set(case.taps) | set(views))
        self.banks = {}
        # (a wanted signal that IS an edge's source -- the voice's last stage, as a rule -- is the input block itself: the oracle
        # builds no voice that ends in a bank input)
        self.straight = {end: case.edges.index(end) for end in self.ends if end in case.edges}
        for end in self.ends:
            if end in self.straight:
                continue
            b = oracle.OracleBank(twin[:end + 1], 1, sample_type, 2, False, True)
            b.set_in_channels(self.in_channels)
            for s, a in case.ctor.items():
                if s <= end:
                    b.set_ctor_args(s, np.asarray(a, dtype=np.float64)[v:v + 1])
            for k, i in enumerate(case.edges):
                if i <= end:
                    b.set_ctor_args(i, np.array([[float(case.in_channels + k)]]))
            b.init(SR, bs)
            self.banks[end] = b
        self.cut = set(cut_edges)
        self.prev = np.zeros((m, bs), dtype=self.dtype)  # the taps' last block: FeedbackSink's buffer, zero at first

    def each(self, stage):
        return [b for end, b in self.banks.items() if stage <= end]

    def block(self, bank_input=None):
        """-> {end: the block of stage `end`'s signal}, done frame and flags of the whole voice (the longest bank)."""
        x = np.zeros((self.in_channels, self.bs), dtype=self.dtype)
        if self.case.in_channels:
            x[:self.case.in_channels] = bank_input
        for k in range(len(self.case.edges)):
            if k not in self.cut:
                x[self.case.in_channels + k] = self.prev[k]
        got, done, flags = {}, 0xFFFFFFFF, 0
        for end, k in self.straight.items():
            got[end] = x[self.case.in_channels + k].copy()
        for end, b in self.banks.items():
            b.set_input(x)
            _, voices, fl, dn = b.process_block()
            got[end] = voices[0].copy()
            if end == self.ends[-1]:
                done, flags = int(dn[0]), fl
        for k, t in enumerate(self.case.taps):
            self.prev[k] = got[t]
        return got, done, flags

    def close(self):
        for b in self.banks.values():
            b.close()


class ClosedLoop:
    """The expected signals of a bank of `case` voices.  It takes the device bank's parameter calls (param_apply,
    set_delay_within_block_for_param, by voice, stage, param) and hands each to every oracle bank of that voice that holds the
    stage.  views: the stages whose node outputs are wanted (the voice's last stage always is).  cut_edges: edges whose
    source reads zeros for ever -- the same voice with the edge removed."""

    def __init__(self, oracle, case, sample_type, bs, views=(), cut_edges=()):
        self.case, self.bs = case, bs
        self.last = node_output(case.stages, len(case.stages) - 1)
        self.views = sorted(set(views) | {self.last})
        self.loops = [_VoiceLoop(oracle, case, v, sample_type, bs, self.views, cut_edges) for v in range(case.n)]
        # KNH_FLAG_ALL_DONE describes silence and the oracle does not compute it: a voice runs from a t_restart of a multiplying
        # envelope until that envelope reports done; a voice without one never finishes (knaster_hip.h)
        self.running = np.zeros(case.n, dtype=bool)

    def param_apply(self, voice, stage, param, value):
        for b in self.loops[voice].each(stage):
            b.param_apply(0, stage, param, value)

    def set_delay_within_block_for_param(self, voice, stage, param, delay):
        for b in self.loops[voice].each(stage):
            b.set_delay_within_block_for_param(0, stage, param, delay)

    def param_apply_many(self, voices, stage, param, kind, fvalues=None, ivalues=None, delays=None):
        """One stage and parameter for the listed voices, as VoiceBank.param_apply_many takes them."""
        voices = np.asarray(voices, dtype=np.uint32)
        if kind == L.VALUE_TRIGGER and (stage, param) in self.case.silencers:
            self.running[voices] = True
        pick = lambda a, k: None if a is None else [np.broadcast_to(np.asarray(a), voices.shape)[k]]
        for k, v in enumerate(voices):
            for b in self.loops[int(v)].each(stage):
                b.param_apply_many([0], stage, param, kind, pick(fvalues, k), pick(ivalues, k), pick(delays, k))

    def restart(self, oracle, voices, sample_type):
        """Fresh nodes and zero feedback buffers for the listed voices."""
        for v in voices:
            self.loops[v].close()
            self.loops[v] = _VoiceLoop(oracle, self.case, v, sample_type, self.bs, self.views, ())
            self.running[v] = False

    def block(self, bank_input=None):
        """-> ({view stage: [n, bs]}, done frames [n], flags of the bank)"""
        rows = {s: [] for s in self.views}
        done, any_done = [], False
        for v, loop in enumerate(self.loops):
            got, dn, fl = loop.block(bank_input)
            for s in self.views:
                rows[s].append(got[s])
            done.append(dn)
            any_done = any_done or bool(fl & L.FLAG_ANY_DONE)
            if dn != 0xFFFFFFFF:
                self.running[v] = False
        flags = (L.FLAG_ANY_DONE if any_done else 0) | (L.FLAG_ALL_DONE if self.case.silencers and not self.running.any() else 0)
        return {s: np.stack(r) for s, r in rows.items()}, np.array(done, dtype=np.uint32), flags

    def close(self):
        for loop in self.loops:
            loop.close()


def expected_blocks(oracle, case, sample_type, bs, n_blocks, views=(), cut_edges=(), events=None, bank_input=None):
    """n_blocks of the closed loop -> ([block]{view: [n, bs]}, [block] done frames, [block] flags); events(block, target)
    makes the block's parameter calls."""
    loop = ClosedLoop(oracle, case, sample_type, bs, views, cut_edges)
    case.start(loop)
    rows, done, flags = [], [], []
    for b in range(n_blocks):
        if events:
            events(b, loop)
        r, d, f = loop.block(bank_input)
        rows.append(r)
        done.append(d)
        flags.append(f)
    loop.close()
    return rows, done, flags


def left_fold(rows):
    acc = rows[0].copy()
    for k in range(1, rows.shape[0]):
        acc = acc + rows[k]
    return acc
