"""Graph voices built from every stage kind (tests/test_graph_voices.py, tests/test_gpu_graph_voices.py): the seeded generator,
the directed voices, and a restatement in Python of what the library derives from a stage list -- the signal-slot plan of
build_signature and the envelopes' task order -- shared so that what the CPU test accepts and compiles is what the GPU test
runs.  random_dag of tests/test_gpu_dag.py draws from a small pool (SinWt, arithmetic, two filters, EnvAr); this one draws
from every kind and setting that another test already holds bit for bit."""
from __future__ import annotations

import functools
import itertools
import os
import re
import types

import numpy as np

import ar_sources
import env_source_cases as esc
import wavetable_ref
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

NOT_DONE = 0xFFFFFFFF
N_SEEDS = max(32, int(os.environ.get("KNH_TEST_SEEDS", "32")))
VOICE_COUNTS = (1, 3, 64, 65, 130)
BLOCK_SIZES = (16, 48, 64, 100)

SOURCES = (L.STAGE_SIN_WT, L.STAGE_PHASOR, L.STAGE_WHITE_NOISE, L.STAGE_PINK_NOISE, L.STAGE_BROWN_NOISE, L.STAGE_RANDOM_LIN,
           L.STAGE_POLYBLEP, L.STAGE_BUFFER_READER)
NOISES = (L.STAGE_WHITE_NOISE, L.STAGE_PINK_NOISE, L.STAGE_BROWN_NOISE)
DELAYS = (L.STAGE_SAMPLE_DELAY, L.STAGE_ALLPASS_DELAY, L.STAGE_ALLPASS_FB_DELAY)
ENVELOPES = (L.STAGE_MUL_ENV_ASR, L.STAGE_MUL_ENV_AR, L.STAGE_MUL_ENVELOPE)
CONSTANTS = (L.STAGE_MUL_CONST, L.STAGE_ADD_CONST, L.STAGE_SUB_CONST, L.STAGE_DIV_CONST)
PROCESSORS = (L.STAGE_SVF, L.STAGE_ONEPOLE_LPF, L.STAGE_ONEPOLE_HPF, L.STAGE_MUL_ENV_ASR, L.STAGE_MUL_ENV_AR, L.STAGE_SAFETY_LIMITER,
              L.STAGE_MUL_ENVELOPE) + CONSTANTS + DELAYS
MATH2 = (L.STAGE_MATH_ADD, L.STAGE_MATH_SUB, L.STAGE_MATH_MUL, L.STAGE_MATH_DIV)
WRAPPERS = (L.STAGE_WR_MUL, L.STAGE_WR_ADD, L.STAGE_WR_SUB, L.STAGE_WR_VSUB, L.STAGE_WR_DIV, L.STAGE_WR_POWI)
ALL_WRAPPERS = WRAPPERS + (L.STAGE_WR_VDIV, L.STAGE_WR_POWF)
POOL = SOURCES + PROCESSORS + MATH2 + WRAPPERS + (L.STAGE_PAN2,)
PLAIN_WAVEFORMS = tuple(w for w in range(14) if w not in ar_sources.SIN_WAVEFORMS)
PRECISE = (L.STAGE_SIN_WT, L.STAGE_SVF, L.STAGE_ONEPOLE_LPF, L.STAGE_ONEPOLE_HPF, L.STAGE_ADD_CONST, L.STAGE_SUB_CONST,
           L.STAGE_DIV_CONST) + ENVELOPES + DELAYS  # the nodes the generator wraps in WrPreciseTiming
# link kind -> (stage kinds, parameter, the driver's depth and offset as multiples of (1, the node's own frequency))
LINKS = {
    "constant_value": ((L.STAGE_MUL_CONST, L.STAGE_ADD_CONST, L.STAGE_SUB_CONST), 0),
    "wr_mul": ((L.STAGE_WR_MUL,), 0),
    "sin_freq": ((L.STAGE_SIN_WT,), 0),
    "sin_phase_offset": ((L.STAGE_SIN_WT,), 1),
    "polyblep_freq": ((L.STAGE_POLYBLEP,), 0),
    "polyblep_pulse_width": ((L.STAGE_POLYBLEP,), 1),
    "random_lin_freq": ((L.STAGE_RANDOM_LIN,), 0),
    "reader_rate": ((L.STAGE_BUFFER_READER,), 0),
    "envelope_time_scale": ((L.STAGE_MUL_ENVELOPE,), 0),
}
# the float parameters a change may go to: kind -> [(parameter, low, high)]
CHANGEABLE = {
    L.STAGE_SIN_WT: [(0, 50.0, 3000.0)], L.STAGE_SVF: [(0, 200.0, 6000.0), (1, 0.5, 4.0)], L.STAGE_ONEPOLE_LPF: [(0, 100.0, 8000.0)],
    L.STAGE_ONEPOLE_HPF: [(0, 100.0, 8000.0)], L.STAGE_MUL_CONST: [(0, 0.3, 1.0)], L.STAGE_ADD_CONST: [(0, -0.5, 0.5)],
    L.STAGE_SUB_CONST: [(0, -0.5, 0.5)], L.STAGE_DIV_CONST: [(0, 1.0, 3.0)], L.STAGE_WR_MUL: [(0, 0.3, 1.0)],
    L.STAGE_MUL_ENVELOPE: [(0, 0.5, 2.0)], L.STAGE_ALLPASS_FB_DELAY: [(1, -0.8, 0.8)], L.STAGE_BUFFER_READER: [(0, 0.25, 2.0)],
}


def is_env_source(s):
    return s.kind in ENVELOPES and bool(s.flags & L.STAGE_FLAG_ENV_SOURCE)


def is_source(s):
    """Reads no signal: the sources, an envelope source (KNH_STAGE_FLAG_ENV_SOURCE); not a SinWt / OscWt under AR_FREQ, which
    reads its frequency"""
    if s.kind == L.STAGE_SIN_WT and s.flags & L.STAGE_FLAG_AR_FREQ:
        return False
    return s.kind in SOURCES or s.kind in (L.STAGE_SIN_NUMERIC, L.STAGE_INPUT) or is_env_source(s)


def is_math2(s):
    return L.STAGE_MATH_ADD <= s.kind <= L.STAGE_MATH_POW


def is_wrapper(s):
    return s.kind in ALL_WRAPPERS


# ---- what the library derives from a stage list, restated ----------------------------------------------------------------
def node_output(st, k):
    """The stage whose output a reader of stage k gets: the last of the wrapper stages that follow it."""
    while k + 1 < len(st) and is_wrapper(st[k + 1]):
        k += 1
    return k


def operands(st):
    """-> (a, b): per stage, the stage whose signal it reads (-1: none) and the second one (a MATH_* operand, a link's driver)"""
    a, b = [-1] * len(st), [-1] * len(st)
    for i, s in enumerate(st):
        if is_math2(s):
            a[i], b[i] = node_output(st, s.input - 1), node_output(st, s.input2 - 1)
        elif i > 0 and not is_source(s):
            a[i] = node_output(st, s.input - 1) if s.input else i - 1
        if s.ar_param:
            b[i] = node_output(st, s.input2 - 1)
    return a, b


def readers(st):
    """-> per stage, the stages that read its output"""
    a, b = operands(st)
    out = [[] for _ in st]
    for i in range(len(st)):
        for k in {a[i], b[i]} - {-1}:
            out[k].append(i)
    return out


def connected(st, outs):
    """outs: None, or the two node-output stages of connect_outputs(l, r); the last stage twice is the default voice"""
    return outs is not None and not (outs[0] == len(st) - 1 and outs[1] == len(st) - 1)


def slot_plan(st, outs=None):
    """The signal slots of a graph voice: -> ([(slot of a, slot of b, slot written)] per stage, number of slots).  A stage
    takes the first free slot; a signal's slot is free again at its last reader; a stage that is not a MATH_* writes in place
    when its first operand dies at it.  A signal nobody reads holds its slot only while it is written; the last stage's
    signal is the voice's output -- or, with two connected outputs, theirs are: neither slot is given to a later stage, and
    the last stage's is held only if it is one of them."""
    a, b = operands(st)
    n = len(st)
    last = [max(r) if r else -1 for r in readers(st)]
    last[n - 1] = n
    if connected(st, outs):
        last[n - 1] = -1
        last[outs[0]] = last[outs[1]] = n
    slot, busy, plan = [-1] * n, [], []
    for i in range(n):
        sa = slot[a[i]] if a[i] >= 0 else -1
        sb = slot[b[i]] if b[i] >= 0 else -1
        for k, s in ((a[i], sa), (b[i], sb)):
            if k >= 0 and last[k] == i:
                busy[s] = False
        free = [k for k, x in enumerate(busy) if not x]
        if sa >= 0 and not busy[sa] and not is_math2(st[i]):
            o = sa
        elif free:
            o = free[0]
        else:
            o = len(busy)
            busy.append(False)
        busy[o] = last[i] >= 0
        slot[i] = o
        plan.append((sa, sb, o))
    return plan, len(busy)


def parse_signature(sig):
    """"W@_,_,0m%0@0,1,0...#3" -> ([(character, linked parameter or None, a, b, o)], slots); a, b: -1 for "_" """
    body, _, count = sig.partition("#")
    count = count.partition(":")[0]  # "#R:l,r": the slots of two connected outputs (signature_outputs)
    num = lambda t: -1 if t == "_" else int(t)
    out = [(m.group(1), None if m.group(2) is None else int(m.group(2)), num(m.group(3)), num(m.group(4)), num(m.group(5)))
           for m in re.finditer(r"(.)(?:%(\d+))?@(_|\d+),(_|\d+),(_|\d+)", body)]
    return out, int(count)


def signature_outputs(sig):
    """"...#3:0,2" -> (0, 2), the slots of the two connected outputs; None without the suffix"""
    tail = sig.partition("#")[2].partition(":")[2]
    return tuple(int(t) for t in tail.split(",")) if tail else None


# the signature character of every stage kind, in the order of the kinds (stage_table.hpp kKinds)
KIND_CHARS = "WNSLHAEmasdmasVvdqpipDPXBYZFUKOGJ+-*/^IQcrftwe"
assert len(KIND_CHARS) == L.STAGE_MATH1_EXP + 1 and KIND_CHARS[L.STAGE_MATH1_CEIL] == "c" and KIND_CHARS[L.STAGE_PAN2] == "J"


def stage_char(s):
    """'M' / 'k': OscWt (WAVETABLE), plain and under AR_FREQ; 'R': SinWt under AR_FREQ; 'b' 'j' 'l': EnvAsr, EnvAr, Envelope as
    sources.  (A bank that stages its one Wavetable to LDS shows 'g' / 'h' for 'M' / 'k' once it is initialised.)"""
    if is_env_source(s):
        return "bjl"[ENVELOPES.index(s.kind)]
    if s.kind == L.STAGE_SIN_WT:
        ar, wt = bool(s.flags & L.STAGE_FLAG_AR_FREQ), bool(s.flags & L.STAGE_FLAG_WAVETABLE)
        return ("k" if ar else "M") if wt else ("R" if ar else "W")
    return KIND_CHARS[s.kind]


def is_graph(st, outs=None):
    """What build_signature takes for a graph: connected outputs, a MATH_* of two signals, a named operand that is not the
    stage in front, an audio-rate link, a second source"""
    if connected(st, outs):
        return True
    named = any(is_math2(s) or (s.input != 0 and s.input != i) or s.ar_param for i, s in enumerate(st))
    return named or sum(is_source(s) for s in st) > 1


def expected_signature(st, outs=None):
    """debug_signature() of an uninitialised bank of these stages, restated (chain_signature.hpp build_signature)"""
    chars = [stage_char(s) for s in st]
    if not is_graph(st, outs):
        return "".join(chars)
    num = lambda v: "_" if v < 0 else str(v)
    plan, n_slots = slot_plan(st, outs)
    body = "".join(c + (f"%{s.ar_param - 1}" if s.ar_param else "") + f"@{num(sa)},{num(sb)},{num(o)}"
                   for c, s, (sa, sb, o) in zip(chars, st, plan))
    tail = f":{plan[outs[0]][2]},{plan[outs[1]][2]}" if connected(st, outs) else ""
    return f"{body}#{n_slots}{tail}"


def overwritten_live_signals(st, written):
    """`written`: the slot every stage writes.  -> [(stage, the earlier stage whose signal it destroys)] for signals that
    still have a reader after the write (a reader AT the writing stage has read the sample already: in place is allowed)"""
    rd = readers(st)
    bad, holder = [], {}
    for i in range(len(st)):
        k = holder.get(written[i])
        if k is not None and any(r > i for r in rd[k]):
            bad.append((i, k))
        holder[written[i]] = i
    return bad


def task_order(st):
    """The order the reference's graph runs the nodes in (Graph::calculate_node_order): depth first from the output, a node's
    signal input before a parameter edge, each node after what it reads; nodes the output does not depend on last."""
    a, b = operands(st)
    order, seen = [], set()

    def visit(k):
        if k < 0 or k in seen:
            return
        seen.add(k)
        visit(a[k])
        visit(b[k])
        order.append(k)
    visit(len(st) - 1)
    return order + [i for i in range(len(st)) if i not in seen]


def envelope_orders(st):
    """-> (the envelope stages in list order, the same in task order); BufferReader is not among them"""
    envs = [i for i, s in enumerate(st) if s.kind in ENVELOPES]
    rank = {k: r for r, k in enumerate(task_order(st))}
    return envs, sorted(envs, key=lambda i: rank[i])


# ---- the generator ---------------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, rng, n, seed):
        self.rng, self.n, self.seed = rng, n, seed
        self.st, self.ctor = [], {}
        self.buffer = None
        self.links = {}  # stage -> link kind
        self.v = np.arange(n, dtype=np.float64)

    def push(self, stage, args=None):
        self.st.append(stage)
        if args is not None:
            self.ctor[len(self.st) - 1] = np.asarray(args, dtype=np.float64).reshape(self.n, -1)
        return len(self.st)  # the value `input` takes to name this stage

    def pick(self):
        return int(self.rng.integers(1, len(self.st) + 1))

    def col(self, lo, hi):
        return np.full(self.n, float(self.rng.uniform(lo, hi)))

    def gain(self):  # a factor that is not near zero
        return np.full(self.n, float(self.rng.uniform(0.3, 1.2)) * (1.0 if self.rng.random() < 0.7 else -1.0))

    def driver(self, depth, offset):
        """limiter(an earlier signal) * depth + offset -> the stage to name in input2"""
        self.push(Stage(L.STAGE_SAFETY_LIMITER, input=self.pick()))
        self.push(Stage(L.STAGE_MUL_CONST), np.broadcast_to(depth, (self.n,)))
        return self.push(Stage(L.STAGE_ADD_CONST), np.broadcast_to(offset, (self.n,)))

    def precise(self, kind):
        return int(self.rng.integers(0, 3)) if kind in PRECISE else 0

    def ctor_for(self, kind):
        rng, n, v = self.rng, self.n, self.v
        if kind in (L.STAGE_SIN_WT, L.STAGE_PHASOR):
            return float(rng.uniform(50.0, 3000.0)) * (1.0 + 0.01 * v)
        if kind in NOISES:
            return 1000.0 * self.seed + 17.0 * len(self.st) + v  # a seed per voice
        if kind == L.STAGE_RANDOM_LIN:
            return np.stack([v + 1.0 + len(self.st), self.col(100.0, 2000.0)], axis=1)
        if kind == L.STAGE_POLYBLEP:
            return np.stack([rng.choice(PLAIN_WAVEFORMS, n).astype(np.float64), float(rng.uniform(50.0, 3000.0)) * (1.0 + 0.01 * v)], axis=1)
        if kind == L.STAGE_BUFFER_READER:
            looping = (v % 2) if rng.random() < 0.5 else np.full(n, float(rng.integers(0, 2)))
            return np.stack([0.5 + 0.03 * (v % 40), looping, np.zeros(n)], axis=1)
        if kind == L.STAGE_SVF:
            return np.stack([rng.integers(0, 9, n).astype(np.float64), rng.uniform(200.0, 6000.0, n), rng.uniform(0.5, 3.0, n), rng.uniform(-6.0, 6.0, n)], axis=1)
        if kind == L.STAGE_ONEPOLE_LPF:
            return rng.uniform(200.0, 6000.0, n)
        if kind in (L.STAGE_MUL_ENV_ASR, L.STAGE_MUL_ENV_AR):
            return np.stack([rng.uniform(0.0003, 0.002, n), rng.uniform(0.0005, 0.004, n)], axis=1)
        if kind == L.STAGE_MUL_ENVELOPE:  # start, time_scale, looping, n_segments, (duration, value) * 4
            a = np.zeros((n, 12))
            a[:, 0] = rng.uniform(-0.5, 0.5, n)
            a[:, 1] = rng.uniform(0.5, 2.0, n)
            a[:, 2] = rng.integers(0, 2, n)
            a[:, 3] = rng.integers(1, 5, n)
            a[:, 4::2] = rng.uniform(0.0003, 0.002, (n, 4))
            a[:, 5::2] = rng.uniform(0.3, 1.0, (n, 4)) * rng.choice([-1.0, 1.0], (n, 4))
            return a
        if kind in DELAYS:
            return rng.uniform(0.0045, 0.006, n)  # the ring: the longest delay
        if kind == L.STAGE_PAN2:
            return rng.uniform(-1.0, 1.0, n)
        if kind in (L.STAGE_DIV_CONST, L.STAGE_WR_DIV):
            return rng.uniform(1.0, 3.0, n)
        if kind == L.STAGE_WR_POWI:
            return rng.integers(0, 4, n).astype(np.float64)
        if kind in (L.STAGE_MUL_CONST, L.STAGE_WR_MUL):
            return self.gain()
        if kind in (L.STAGE_ADD_CONST, L.STAGE_SUB_CONST, L.STAGE_WR_ADD, L.STAGE_WR_SUB, L.STAGE_WR_VSUB):
            return rng.uniform(-1.0, 1.0, n)
        return None

    def node(self, kind, input=0, link=None, wrap=()):
        """One node, the driver of its link in front of it, its wrapper stages behind it.  link: a LINKS key that fits `kind`,
        or "wr_mul" (the first wrapper is then a linked WrMul)."""
        args = self.ctor_for(kind)
        drv, ar = 0, 0
        if link is not None and self.st:
            if link == "sin_freq":
                drv = self.driver(0.3 * args, args)
            elif link == "polyblep_freq":
                drv = self.driver(0.3 * args[:, 1], args[:, 1])
            elif link == "random_lin_freq":
                drv = self.driver(900.0, 1000.0)
            elif link == "reader_rate":
                drv = self.driver(0.8, 1.0)
            elif link == "envelope_time_scale":
                drv = self.driver(0.5, 1.0)
            elif link == "polyblep_pulse_width":
                drv = self.driver(0.45, 0.5)
            else:  # constant_value, wr_mul, sin_phase_offset
                drv = self.driver(0.4, 0.6)
            if link != "wr_mul":
                ar = LINKS[link][1] + 1
        if input == 0 and drv and not is_source(Stage(kind)):
            input = len(self.st) - 3  # the signal in front of the driver: what "the stage before it" was
        me = self.push(Stage(kind, 0, 0 if ar else self.precise(kind), input, drv if ar else 0, ar), args)
        if ar:
            self.links[me - 1] = link
        if kind == L.STAGE_BUFFER_READER:
            self.buffer = (me - 1, ar_sources.reader_buffer(), ar_sources.READER_BUFFER[1])
        if link == "wr_mul" and drv:
            self.push(Stage(L.STAGE_WR_MUL, input2=drv, ar_param=1), self.ctor_for(L.STAGE_WR_MUL))
            self.links[len(self.st) - 1] = "wr_mul"
        for k in wrap:
            self.push(Stage(k), self.ctor_for(k))
        return me


def _count(st, kinds):
    return sum(s.kind in kinds for s in st)


def random_graph_voice(seed):
    """-> Workload of a seeded random graph voice of 5 .. 14 stages, with .events(block, bank), the parameter traffic of the
    six blocks the tests run (the same calls go to the device bank and to the oracle), and .links {stage: link kind}."""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice(VOICE_COUNTS))
    bs = int(rng.choice(BLOCK_SIZES))
    sample_type = L.F64 if seed % 3 == 0 else L.F32
    pan = rng.random() < 0.3
    target = int(rng.integers(6, 15))
    b = _Builder(rng, n, seed)
    # what the seed is given for certain (the rest is drawn): two sources, and every other seed a link, a delay, two envelopes
    first, second = SOURCES[seed % 8], SOURCES[(seed // 8 + 3 * (seed % 8) + 1) % 8]
    if first == second == L.STAGE_BUFFER_READER:
        second = L.STAGE_SIN_WT
    link_kind = list(LINKS)[(seed // 2) % len(LINKS)] if seed % 2 else None
    if seed % 8 == 4:  # (sixteen odd seeds go round the nine link kinds once and seven ninths: the last two once more)
        link_kind = list(LINKS)[7 + (seed // 8) % 2]
    delay_kind = DELAYS[(seed // 2) % 3] if seed % 4 in (0, 3) else None
    two_envelopes = seed % 4 == 2

    def wrappers(p=0.3):
        out = []
        while rng.random() < p and len(out) < 2 and len(b.st) < 8:
            out.append(WRAPPERS[int(rng.integers(0, len(WRAPPERS)))])
        return tuple(out)

    def source(kind, link=None):
        if kind == L.STAGE_BUFFER_READER and b.buffer is not None:
            kind = L.STAGE_SIN_WT
        return b.node(kind, link=link if link in LINKS and kind in LINKS[link][0] else None, wrap=wrappers())

    def processor(kind, link=None, named=None):
        if kind in DELAYS and _count(b.st, DELAYS) or kind == L.STAGE_MUL_ENVELOPE and _count(b.st, (L.STAGE_MUL_ENVELOPE,)):
            kind = L.STAGE_SVF
        inp = named if named is not None else (0 if rng.random() < 0.5 else b.pick())
        fits = link == "wr_mul" or (link in LINKS and kind in LINKS[link][0])
        return b.node(kind, input=inp, link=link if fits else None, wrap=wrappers())

    source(first)
    if link_kind in ("sin_freq", "sin_phase_offset", "polyblep_freq", "polyblep_pulse_width", "random_lin_freq", "reader_rate"):
        want = LINKS[link_kind][0][0]
        if want == L.STAGE_BUFFER_READER and b.buffer is not None:
            b.st[:], b.ctor, b.buffer = [], {}, None  # (one reader per random voice: the linked one)
            source(L.STAGE_SIN_WT)
        source(want, link_kind)
    else:
        source(second)
    if link_kind == "constant_value":
        processor([L.STAGE_MUL_CONST, L.STAGE_ADD_CONST, L.STAGE_SUB_CONST][int(rng.integers(0, 3))], link_kind)
    elif link_kind == "envelope_time_scale":
        processor(L.STAGE_MUL_ENVELOPE, link_kind)
    elif link_kind == "wr_mul":
        processor([L.STAGE_SVF, L.STAGE_ONEPOLE_HPF, L.STAGE_MUL_ENV_ASR][int(rng.integers(0, 3))], link_kind)
    if delay_kind is not None:  # every other one reads a signal that is named and not the one in front of it
        far = [k + 1 for k in range(len(b.st) - 1) if node_output(b.st, k) != len(b.st) - 1]
        processor(delay_kind, named=int(rng.choice(far)) if far and seed % 8 in (0, 3) else None)
    if two_envelopes:  # the one listed first hangs on the second operand of the sum: it runs last
        kinds = [ENVELOPES[k] for k in rng.permutation(3)[:2]]
        e1 = processor(kinds[0], named=1)
        e1 = node_output(b.st, e1 - 1) + 1
        e2 = processor(kinds[1], named=int(rng.integers(1, e1)))
        b.push(Stage(L.STAGE_MATH_ADD, input=e2, input2=e1))
    body = target - (2 if pan else 1)
    while len(b.st) < body:
        room = body - len(b.st)
        r = rng.random()
        if r < 0.15:
            source(SOURCES[int(rng.integers(0, len(SOURCES)))])
        elif r < 0.45:
            kind = MATH2[int(rng.integers(0, 4))]
            if kind == L.STAGE_MATH_DIV:
                if room < 4:
                    continue
                num = b.pick()
                b.push(Stage(L.STAGE_SAFETY_LIMITER, input=b.pick()))  # the denominator: signal * 0.25 + 2, never near zero
                b.push(Stage(L.STAGE_MUL_CONST), np.full(n, 0.25))
                den = b.push(Stage(L.STAGE_ADD_CONST), np.full(n, 2.0))
                b.st[b.node(kind, wrap=wrappers()) - 1] = Stage(kind, input=num, input2=den)
            else:
                x, y = b.pick(), b.pick()
                b.st[b.node(kind, wrap=wrappers()) - 1] = Stage(kind, input=x, input2=y)
        else:
            processor(PROCESSORS[int(rng.integers(0, len(PROCESSORS)))])
    # the end: Pan2, or the limiter that keeps a runaway product finite
    if pan:
        b.push(Stage(L.STAGE_SAFETY_LIMITER))
        b.push(Stage(L.STAGE_PAN2), b.ctor_for(L.STAGE_PAN2))
    else:
        b.push(Stage(L.STAGE_SAFETY_LIMITER))
    st = b.st
    w = configs.Workload(f"graph{seed}", st, n, bs, sample_type, 2 if pan else 1)
    w.ctor = b.ctor
    w.buffer = b.buffer
    w.links = dict(b.links)
    w.events = _random_events(seed, st, n, bs, w.links)
    return w


def _random_events(seed, st, n, bs, links):
    """The six blocks' parameter traffic, drawn once: {block: [(voices, stage, param, kind, fvalues, delays)]}"""
    rng = np.random.default_rng(9000 + seed)
    v = np.arange(n, dtype=np.uint32)
    script = {k: [] for k in range(6)}
    half = v[rng.random(n) < 0.5] if n > 1 else v
    for i, s in enumerate(st):
        if s.kind == L.STAGE_MUL_ENV_ASR:
            script[0].append((v, i, 3, L.VALUE_TRIGGER, None, None))
            script[2].append((half, i, 2, L.VALUE_TRIGGER, None, None))
        if s.kind == L.STAGE_MUL_ENV_AR:
            script[0].append((v, i, 2, L.VALUE_TRIGGER, None, None))
        if s.kind == L.STAGE_MUL_ENVELOPE:
            script[0].append((v, i, 2, L.VALUE_TRIGGER, None, None))
            script[2].append((half, i, 3, L.VALUE_TRIGGER, None, None))
        if s.kind in DELAYS:  # no longer than a quarter of the six blocks, so that the delayed signal is heard in them
            longest = min(0.004, 1.5 * bs / configs.SAMPLE_RATE)
            script[0].append((v, i, 0, L.VALUE_FLOAT, rng.uniform(0.0001, longest, n), None))
            delays = rng.integers(0, bs, n).astype(np.uint16) if s.delayed_changes_per_block else None
            script[3].append((v, i, 0, L.VALUE_FLOAT, rng.uniform(0.0001, longest, n), delays))
    free = [(i, p, lo, hi) for i, s in enumerate(st) for (p, lo, hi) in CHANGEABLE.get(s.kind, []) if not (s.ar_param == p + 1)]
    for block in (1, 4):
        if free:
            i, p, lo, hi = free[int(rng.integers(0, len(free)))]
            sel = v[rng.random(n) < 0.5] if n > 1 else v
            if len(sel):
                delays = rng.integers(0, bs, len(sel)).astype(np.uint16) if st[i].delayed_changes_per_block else None
                script[block].append((sel, i, p, L.VALUE_FLOAT, rng.uniform(lo, hi, len(sel)), delays))
    for i in links:  # a change of a linked parameter: ignored while the link stands
        script[2].append((v, i, st[i].ar_param - 1, L.VALUE_FLOAT, np.full(n, 0.37), None))

    def events(block, bank):
        for (sel, i, p, kind, f, d) in script.get(block, []):
            bank.param_apply_many(sel, i, p, kind, f, None, d)
    events.script = script
    return events


# ---- the directed voices ---------------------------------------------------------------------------------------------------
S = Stage
DIRECTED = ["comb_asr_pan", "wrapped_noise", "three_envs", "nineteen", "reader_mix", "wrapped_fanout"]
READER_POOL = ((700, 44100.0), (450, 22050.0))  # reader_mix: the two entries of the bank's pool


def _trigger_events(n, script):
    """script: {block: [(stage, param, every k-th voice)]}"""
    v = np.arange(n, dtype=np.uint32)

    def events(block, bank):
        for (stage, param, step) in script.get(block, []):
            bank.param_apply_many(v[::step], stage, param, L.VALUE_TRIGGER)
    events.script = script
    return events


def directed_voice(name, n, sample_type, block_size=64):
    """-> Workload with .events(block, bank) for the 12 blocks the tests run; reader_mix has .pool (stage, buffers, ids)
    instead of a bank buffer (the oracle, which takes one Buffer per bank, is assembled per pool entry)."""
    p = configs.voice_parameters(n)
    v = np.arange(n, dtype=np.float64)
    col = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)).reshape(n, 1).copy()
    svf = lambda ty: np.stack([np.full(n, float(ty)), p["cutoff"], p["q"], np.zeros(n)], axis=1)
    out_channels, pool, buffer = 1, None, None
    if name == "comb_asr_pan":  # W m D(in=2) +(2,3) A J: dry + delay(dry), an ASR, Pan2
        st = [S(L.STAGE_SIN_WT), S(L.STAGE_MUL_CONST), S(L.STAGE_SAMPLE_DELAY, input=2), S(L.STAGE_MATH_ADD, input=2, input2=3),
              S(L.STAGE_MUL_ENV_ASR), S(L.STAGE_PAN2)]
        ctor = {0: col(p["freq"]), 1: col(0.5), 2: col(0.006), 4: np.stack([p["attack"] * 0.1, p["release"] * 0.02], axis=1),
                5: col(-1.0 + 2.0 * (p["fm_ratio"] - 1.0) / 3.0)}
        script = {0: [(4, 3, 1)], 5: [(4, 2, 2)], 8: [(4, 2, 1)]}
        out_channels = 2
        floats = {0: [(2, 0, 0.0002 + 0.00003 * v)], 3: [(2, 0, 0.004 - 0.00002 * v)]}
    elif name == "wrapped_noise":  # K B wr_mul wr_add *(1,2) Z -(6,4) H X
        st = [S(L.STAGE_PINK_NOISE), S(L.STAGE_POLYBLEP), S(L.STAGE_WR_MUL), S(L.STAGE_WR_ADD), S(L.STAGE_MATH_MUL, input=1, input2=2),
              S(L.STAGE_ALLPASS_FB_DELAY), S(L.STAGE_MATH_SUB, input=6, input2=4), S(L.STAGE_ONEPOLE_HPF), S(L.STAGE_SAFETY_LIMITER)]
        wf = np.asarray(PLAIN_WAVEFORMS, dtype=np.float64)[np.arange(n) % len(PLAIN_WAVEFORMS)]
        ctor = {0: col(100.0 + v), 1: np.stack([wf, p["freq"]], axis=1), 2: col(0.7), 3: col(0.25), 5: col(0.006)}
        script = {}
        floats = {0: [(5, 0, 0.0005 + 0.00002 * v), (5, 1, np.full(n, 0.5)), (7, 0, 300.0 + v)], 6: [(5, 0, 0.003 - 0.00001 * v)]}
    elif name == "three_envs":  # W E P V G A +(6,2) +(7,4): task order A, E, V; list order E, V, A
        st = [S(L.STAGE_SIN_WT), S(L.STAGE_MUL_ENV_AR), S(L.STAGE_PHASOR), S(L.STAGE_MUL_ENVELOPE), S(L.STAGE_RANDOM_LIN), S(L.STAGE_MUL_ENV_ASR),
              S(L.STAGE_MATH_ADD, input=6, input2=2), S(L.STAGE_MATH_ADD, input=7, input2=4)]
        k = 1.0 + 0.001 * (v % 7)
        # EnvAr ends 6 ms after its restart, in block 4; the ASR, released at block 4 (5.33 ms), 0.5 ms later; the Envelope is
        # stopped at block 4 on the even voices and ends after 7 ms, in block 5, on the odd ones
        ctor = {0: col(p["freq"]), 1: np.stack([0.002 * k, 0.004 * k], axis=1), 2: col(p["freq"] * 0.5), 3: ar_sources.envelope_ctor(n, False),
                4: np.stack([v + 1.0, np.full(n, 700.0)], axis=1), 5: np.stack([0.001 * k, 0.0005 * k], axis=1)}
        script = {0: [(1, 2, 1), (3, 2, 1), (5, 3, 1)], 4: [(5, 2, 1), (3, 3, 2)], 8: [(1, 2, 2), (3, 2, 3)], 9: [(3, 3, 3)]}
        floats = {}
    elif name == "nineteen":  # W O * then seven L m pairs, then Y(in=3) +: more than sixteen stages
        st = [S(L.STAGE_SIN_WT), S(L.STAGE_BROWN_NOISE), S(L.STAGE_MATH_MUL, input=1, input2=2)]
        ctor = {0: col(p["freq"]), 1: col(500.0 + v)}
        for k in range(7):
            st += [S(L.STAGE_ONEPOLE_LPF), S(L.STAGE_MUL_CONST)]
            ctor[len(st) - 2] = col(p["cutoff"] * (1.0 + 0.1 * k))
            ctor[len(st) - 1] = col(1.3)
        st += [S(L.STAGE_ALLPASS_DELAY, input=3), S(L.STAGE_MATH_ADD, input=17, input2=18)]
        ctor[17] = col(0.006)
        script = {}
        floats = {0: [(17, 0, 0.0003 + 0.00002 * v)], 5: [(17, 0, 0.002 + 0.00001 * v)]}
    elif name == "reader_mix":  # F F +(1,2) A: a looping and a one-shot reader on pooled buffers, summed, behind an ASR
        st = [S(L.STAGE_BUFFER_READER), S(L.STAGE_BUFFER_READER), S(L.STAGE_MATH_ADD, input=1, input2=2), S(L.STAGE_MUL_ENV_ASR)]
        ctor = {0: np.stack([0.5 + 0.01 * (v % 50), np.ones(n), np.zeros(n)], axis=1),
                1: np.stack([1.5 + 0.02 * (v % 30), np.zeros(n), 0.002 + 0.00001 * v], axis=1),
                3: np.stack([np.full(n, 0.001), 0.001 + 0.00001 * v], axis=1)}
        # (the two readers start at different frames and are restarted apart: each has a start, a length and a rate of its own)
        script = {0: [(3, 3, 1)], 7: [(3, 2, 2)], 9: [(0, 5, 1)], 10: [(1, 5, 2)]}
        floats = {5: [(0, 3, 0.004 + 0.00002 * v)], 6: [(1, 0, 1.0 + 0.01 * (v % 20))]}
        t = [np.arange(k) / sr for (k, sr) in READER_POOL]
        buffers = [(ar_sources.reader_buffer(), READER_POOL[0][1]),
                   (0.5 * np.sin(2 * np.pi * 523.0 * t[1]) + 0.25 * np.sin(2 * np.pi * 2111.0 * t[1] + 1.0), READER_POOL[1][1])]
        ids = (np.arange(n) % 3 == 1).astype(np.uint32)
        pool = (0, buffers, ids)  # (a bank has one pool: both readers of voice v play entry ids[v])
    elif name == "wrapped_fanout":  # SinWt wr_mul wr_add read by an Svf, a OnePoleHpf and (through them) a MATH_MUL
        st = [S(L.STAGE_SIN_WT), S(L.STAGE_WR_MUL), S(L.STAGE_WR_ADD), S(L.STAGE_SVF), S(L.STAGE_ONEPOLE_HPF, input=1),
              S(L.STAGE_MATH_MUL, input=4, input2=5)]
        ctor = {0: col(p["freq"]), 1: col(0.8), 2: col(0.1), 3: svf(L.SVF_BAND)}
        script = {}
        floats = {0: [(4, 0, 200.0 + 3.0 * v)], 3: [(1, 0, 0.5 + 0.001 * v)]}
    else:
        raise KeyError(name)
    w = configs.Workload("gv_" + name, st, n, block_size, sample_type, out_channels)
    w.ctor = ctor
    w.buffer = buffer
    w.pool = pool
    w.links = {}
    triggers = _trigger_events(n, script)
    vi = np.arange(n, dtype=np.uint32)

    def events(block, bank):
        triggers(block, bank)
        for (stage, param, values) in floats.get(block, []):
            bank.param_apply_many(vi, stage, param, L.VALUE_FLOAT, values)
    w.events = events
    w.triggers = script
    return w


def three_envs_alone(n, sample_type, block_size=64):
    """three_envs' envelopes each in a chain of its own (source -> envelope), same constructor arguments and triggers: the
    oracle's done frames of these say which envelopes finish in which block.  -> [Workload] in TASK order: EnvAsr, EnvAr,
    Envelope"""
    full = directed_voice("three_envs", n, sample_type, block_size)
    out = []
    for env in (5, 1, 3):
        w = configs.Workload(f"gv_three_envs_{env}", full.stages[env - 1:env + 1], n, block_size, sample_type, 1)
        w.ctor = {0: full.ctor[env - 1], 1: full.ctor[env]}
        w.buffer = w.pool = None
        w.events = _trigger_events(n, {b: [(1, p, step) for (s, p, step) in ev if s == env] for b, ev in full.triggers.items()})
        out.append(w)
    return out


# ---- banks -----------------------------------------------------------------------------------------------------------------
def gpu_bank(knh, w, mix_mode=L.MIX_LEFT_FOLD, **kw):
    """The device bank of a voice of this module (helpers.make_gpu, plus the buffer pools of reader_mix)."""
    b = knh.VoiceBank(w.stages, w.n_voices, w.sample_type, w.out_channels, mix_mode, -1, False, **kw)
    for s, a in w.ctor.items():
        b.set_ctor_args(s, a)
    if w.buffer is not None:
        b.set_buffer(*w.buffer)
    if getattr(w, "pool", None):
        stage, buffers, ids = w.pool
        for k, (samples, sr) in enumerate(buffers):
            assert b.add_buffer(stage, samples, sr) == k
        b.assign_buffers(stage, np.arange(w.n_voices, dtype=np.uint32), ids)
    b.init(configs.SAMPLE_RATE, w.block_size)
    return b


class OracleVoices:
    """The oracle of a voice of this module, with the call surface the events use.  A pooled voice is one oracle bank per
    pool entry, every voice on that entry, of which the rows of the voices assigned to it are kept (tests/sampler_pool.py);
    its left-fold mix is folded here from the rows."""

    def __init__(self, oracle, w):
        self.w = w
        pool = getattr(w, "pool", None)
        self.banks = []
        if not pool:
            o = oracle.OracleBank(w.stages, w.n_voices, w.sample_type, w.out_channels, True, True)
            self._start(o, w.buffer)
            self.banks.append((o, None))
        else:
            _, buffers, ids = pool
            for e, (samples, sr) in enumerate(buffers):
                o = oracle.OracleBank(w.stages, w.n_voices, w.sample_type, w.out_channels, False, True)
                self._start(o, (0, samples, sr))
                self.banks.append((o, ids == e))

    def _start(self, o, buffer):
        for s, a in self.w.ctor.items():
            o.set_ctor_args(s, a)
        if buffer is not None:
            o.set_buffer(*buffer)
        o.init(configs.SAMPLE_RATE, self.w.block_size)

    def param_apply_many(self, *a, **kw):
        for o, _ in self.banks:
            o.param_apply_many(*a, **kw)

    def process_block(self):
        """-> (mix, voices, flags, done frames), as OracleBank.process_block"""
        if self.banks[0][1] is None:
            return self.banks[0][0].process_block()
        voices = done = None
        for o, mine in self.banks:
            _, rows, _, d = o.process_block()
            if voices is None:
                voices, done = np.zeros_like(rows), np.full_like(d, NOT_DONE)
            voices[..., mine, :] = rows[..., mine, :]
            done[mine] = d[mine]
        planes = voices if voices.ndim == 3 else voices[None]
        mix = np.stack([_left_fold(pl) for pl in planes])
        if self.w.out_channels == 2 and mix.shape[0] == 1:
            mix = np.concatenate([mix, mix])
        flags = L.FLAG_ANY_DONE if (done != NOT_DONE).any() else 0
        return mix, voices, flags, done

    def close(self):
        for o, _ in self.banks:
            o.close()


def _left_fold(rows):
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = acc + r
    return acc


def oracle_run(oracle, w, blocks):
    """-> (voices [blocks, ...], mixes [blocks, ch, bs], flags [blocks], done [blocks, n]) of the oracle alone, read-only"""
    o = OracleVoices(oracle, w)
    out = [[], [], [], []]
    for b in range(blocks):
        w.events(b, o)
        mix, voices, flags, done = o.process_block()
        for k, x in enumerate((voices, mix, flags, done)):
            out[k].append(np.copy(x))
    o.close()
    res = tuple(np.stack(x) for x in out)
    for x in res:
        x.setflags(write=False)
    return res


# ---- the second generator path: voices that combine the newer stage kinds, flags and calls --------------------------------
# random_graph_voice draws what it drew when it was written.  random_voice_head draws, on top of that pool: OscWt sources
# (SIN_WT | WAVETABLE) on pools of sine Wavetables, envelope sources (ENV_SOURCE), two to twelve delay stages, the exact Math1
# functions, two connected outputs, a reader on a pool of two mono Buffers that is reassigned while the bank runs, and a
# restart of every third voice.  What a seed is GIVEN is a function of the seed (HEAD_SUBSETS: every three of the six
# features that the library allows together), so that coverage is a condition on the seed list and not a matter of chance.
# Not drawn:
#   * READER_CH1 and two-channel pools -- their reference is numpy, not the oracle (tests/test_gpu_stereo_reader.py);
#   * SIN_NUMERIC and PolyBlep's sine waveforms -- compared with a tolerance elsewhere;
#   * Galactic, and Pan2 (which cannot end a voice with connected outputs);
#   * MATH1_EXP -- not exact;
#   * anything that makes NaN: the limiter at the end, the `x * x + c` under sqrt and the denominator guards stay;
#   * an envelope of any kind in a voice whose reader is reassigned: knh_bank_assign_buffers refuses it after init (the
#     voice's one done frame could not be attributed), so "env_source" and "reassign" never share a seed;
#   * a reader wrapped in WrPreciseTiming (delayed_changes_per_block), as in the first path: the reference's
#     BufferReader::process_block writes ctx.block_size() frames into the partial block a delayed change makes (buffer.rs:161);
#   * more delay stages than sixteen stages hold beside the seed's other two features (KNH_MAX_DELAY_STAGES is sixteen too).
HEAD_FEATURES = ("oscwt", "env_source", "delays", "math1", "connected", "reassign")
HEAD_SUBSETS = [c for c in itertools.combinations(HEAD_FEATURES, 3) if not {"env_source", "reassign"} <= set(c)]
HEAD_VOICE_COUNTS = (3, 65, 130)  # a partial wavefront, one lane over, a third wavefront
HEAD_BLOCK_SIZES = (48, 64, 100)  # partial tiles only, whole tiles, a ragged end
HEAD_BLOCKS, HEAD_RESTART_BLOCK = 9, 6
HEAD_ATTEMPTS = 8
HEAD_MAX_STAGES = 16
MATH1_EXACT = (L.STAGE_MATH1_CEIL, L.STAGE_MATH1_SQRT, L.STAGE_MATH1_FLOOR, L.STAGE_MATH1_TRUNC, L.STAGE_MATH1_FRACT)
OSCWT_SETTINGS = ("plain", "ar_freq", "ar_param", "smooth", "delayed")
ENV_SOURCE_USES = ("math", "link", "wrapper")
HEAD_MANY_DELAYS = (2, 3)  # the places, modulo 8, among the seeds with delays that take as many delays as fit
HEAD_POOL = ((300, 44100.0), (120, 22050.0))  # the two mono Buffers of a pooled reader: short enough to run out in the nine blocks
WT, ES = L.STAGE_FLAG_WAVETABLE, L.STAGE_FLAG_ENV_SOURCE
HEAD_FILL = (L.STAGE_SVF, L.STAGE_ONEPOLE_LPF, L.STAGE_ONEPOLE_HPF, L.STAGE_SAFETY_LIMITER) + CONSTANTS


def head_features(seed):
    return frozenset(HEAD_SUBSETS[seed % len(HEAD_SUBSETS)])


def _rank(seed, feature):
    """the seed's place among the seeds of 0..31 that are given `feature` (seeds past 31 go round again)"""
    return [s for s in range(32) if feature in head_features(s)].index(seed % 32)


def head_pool_buffers():
    out = []
    for k, (frames, sr) in enumerate(HEAD_POOL):
        t = np.arange(frames) / sr
        out.append((0.5 * np.sin(2 * np.pi * (331.0 + 192.0 * k) * t + k) + 0.3 * np.sin(2 * np.pi * (1777.0 + 334.0 * k) * t), sr))
    return out


def _head_attempt(seed, attempt):
    """One draw of the seed's voice -> Workload, or None if the draw does not fit the sixteen stages."""
    rng = np.random.default_rng([11000, seed, attempt])
    feats = head_features(seed)
    n = HEAD_VOICE_COUNTS[(seed + seed // 3) % 3]
    if seed % 6 in (2, 3) and n < 65:  # the seeds tests/test_gpu_graph_voices.py cuts into two voice ranges: a range is whole wavefronts
        n = 65
    bs = HEAD_BLOCK_SIZES[(seed // 2 + seed // 6) % 3]
    f64 = seed % 3 == 0
    b = _Builder(rng, n, seed)
    v = b.v
    info = types.SimpleNamespace(features=feats, oscwt=None, wt_variant=None, env_use=None, math1=None, delays=0, chain=False)
    wavetables = pool = outs = None
    reassign = {}
    mains = []  # the node outputs the voice's main signal went through (1-based, as `input` names them)
    # what the features still to come need at the least, so that an earlier one leaves them room
    need = {"env_source": 3, "delays": 2, "math1": 2, "reassign": 2}
    todo = [f for f in ("reassign", "env_source", "delays", "math1") if f in feats]
    room = lambda: HEAD_MAX_STAGES - 1 - len(b.st) - sum(need[f] for f in todo)
    # a plain chain (one source, nothing named): the fused pipeline's form, where several delays' tiles share the LDS
    chain = feats == {"oscwt", "delays", "math1"}

    def to(me):
        mains.append(node_output(b.st, me - 1) + 1)
        return mains[-1]

    def mix(x, y):  # the two signals into one: + - or *
        return to(b.push(Stage(MATH2[int(rng.integers(0, 3))], input=x, input2=y)))

    # ---- the first source ----
    lds_wanted = False
    if "oscwt" in feats:
        k = _rank(seed, "oscwt")
        setting = OSCWT_SETTINGS[k % len(OSCWT_SETTINGS)]
        if chain and setting == "ar_param":
            setting = "plain"
        f32_rank = [s for s in range(32) if "oscwt" in head_features(s) and s % 3 != 0]
        variant = "tables17" if f64 else ("lds", "sinwt")[f32_rank.index(seed % 32) % 2] if seed % 32 in f32_rank else "tables17"
        if chain and variant == "sinwt":
            variant = "lds"
        lds_wanted = variant == "lds"
        freq = float(rng.uniform(80.0, 2500.0)) * (1.0 + 0.01 * v)
        if setting == "ar_freq":  # Phasor * depth + freq, read as the frequency by the stage behind it
            b.push(Stage(L.STAGE_PHASOR), float(rng.uniform(3.0, 40.0)) * (1.0 + 0.02 * v))
            b.push(Stage(L.STAGE_MUL_CONST), 0.3 * freq)
            b.push(Stage(L.STAGE_ADD_CONST), freq)
            osc = b.push(Stage(L.STAGE_SIN_WT, WT | L.STAGE_FLAG_AR_FREQ), freq)
        elif setting == "ar_param":
            to(b.node(L.STAGE_PHASOR))
            drv = b.driver(0.3 * freq, freq)
            osc = b.push(Stage(L.STAGE_SIN_WT, WT, 0, 0, drv, 1), freq)
            b.links[osc - 1] = "sin_freq"
        elif setting == "smooth":
            osc = b.push(Stage(L.STAGE_SIN_WT, WT | L.STAGE_FLAG_SMOOTH_PARAMS), freq)
        else:
            osc = b.push(Stage(L.STAGE_SIN_WT, WT, 2 if setting == "delayed" else 0), freq)
        # the pool: sine Wavetables only (the oracle's SinWt is the reference), as one table or as seventeen equal ones
        entries = ["one"] if variant in ("lds", "sinwt") else ["seventeen", "one"]
        wavetables = (osc - 1, entries, (np.arange(n) % len(entries)).astype(np.uint32))
        if mains:
            mix(mains[-1], osc)
        else:
            to(osc)
        if variant == "sinwt":  # a plain SinWt beside it: the sine table keeps its place in the LDS
            mix(mains[-1], b.node(L.STAGE_SIN_WT))
        info.oscwt, info.wt_variant = setting, variant
    else:
        first = (L.STAGE_PHASOR, L.STAGE_WHITE_NOISE, L.STAGE_POLYBLEP, L.STAGE_SIN_WT, L.STAGE_PINK_NOISE, L.STAGE_RANDOM_LIN,
                 L.STAGE_BROWN_NOISE, L.STAGE_BUFFER_READER)[(seed // 2) % 8]
        if first == L.STAGE_BUFFER_READER and "reassign" in feats:
            first = L.STAGE_SIN_WT
        to(b.node(first))
    sources = [k for k in SOURCES if not (lds_wanted and k == L.STAGE_SIN_WT) and not (k == L.STAGE_BUFFER_READER and (b.buffer is not None or "reassign" in feats))]

    # ---- a reader on a pool of two mono Buffers, reassigned while the bank runs ----
    if "reassign" in feats:
        todo.remove("reassign")
        reader = b.push(Stage(L.STAGE_BUFFER_READER), np.stack([1.0 + 0.03 * (v % 30), v % 2, np.zeros(n)], axis=1))
        ids = (np.arange(n) % 3 == 1).astype(np.uint32)
        pool = (reader - 1, head_pool_buffers(), ids)
        vi = np.arange(n, dtype=np.uint32)
        half, some = vi[::2], vi[1::4]
        reassign[3] = (half, 1 - ids[half], np.stack([1.6 + 0.02 * (half % 20), (half % 4 == 0).astype(np.float64), np.full(len(half), 0.001)], axis=1))
        if len(some):
            reassign[7] = (some, np.zeros(len(some), dtype=np.uint32), np.stack([1.5 + 0.01 * (some % 10), np.zeros(len(some)), np.zeros(len(some))], axis=1))
        mix(mains[-1], reader)
    elif not chain and room() >= 2:  # a second source
        mix(mains[-1], b.node(sources[int(rng.integers(0, len(sources)))]))

    # ---- an envelope source, beside a multiplying envelope of another kind ----
    if "env_source" in feats:
        todo.remove("env_source")
        k = _rank(seed, "env_source")
        kind, beside = ENVELOPES[k % 3], ENVELOPES[(k + 1 + k // 3) % 3 if (k + 1 + k // 3) % 3 != k % 3 else (k + 2) % 3]
        use = ENV_SOURCE_USES[(k // 3 + k) % 3]
        cost = {"math": 3, "link": 6, "wrapper": 5}
        if room() + need["env_source"] < cost[use]:
            use = "math"
        env = b.push(Stage(kind, ES), b.ctor_for(kind))
        main = mains[-1]
        if use == "math":
            to(b.push(Stage(L.STAGE_MATH_MUL if k % 2 else L.STAGE_MATH_ADD, input=main, input2=env)))
        elif use == "wrapper":
            b.push(Stage(L.STAGE_WR_MUL), b.gain())
            b.push(Stage(L.STAGE_WR_ADD), rng.uniform(-0.5, 0.5, n))
            to(b.push(Stage(L.STAGE_MATH_MUL, input=main, input2=env)))
        else:
            link = [x for x in ("constant_value", "sin_freq", "wr_mul") if not (lds_wanted and x == "sin_freq")][k % (2 if lds_wanted else 3)]
            if link == "sin_freq":
                f = float(rng.uniform(100.0, 1500.0))
                b.push(Stage(L.STAGE_MUL_CONST), np.full(n, 0.5 * f))
                drv = b.push(Stage(L.STAGE_ADD_CONST), f * (1.0 + 0.01 * v))
                osc2 = b.push(Stage(L.STAGE_SIN_WT, 0, 0, 0, drv, 1), np.full(n, f))
                b.links[osc2 - 1] = link
                mix(main, osc2)
            else:
                b.push(Stage(L.STAGE_MUL_CONST), np.full(n, 0.5))
                drv = b.push(Stage(L.STAGE_ADD_CONST), np.full(n, 0.4))
                if link == "constant_value":
                    me = b.push(Stage(L.STAGE_MUL_CONST, 0, 0, main, drv, 1), np.ones(n))
                    b.links[me - 1] = link
                else:
                    me = b.push(Stage(L.STAGE_ONEPOLE_HPF, input=main))
                    b.push(Stage(L.STAGE_WR_MUL, input2=drv, ar_param=1), b.gain())
                    b.links[len(b.st) - 1] = link
                to(me)
            use = "link:" + link
        to(b.push(Stage(beside, 0, b.precise(beside), mains[-1]), b.ctor_for(beside)))
        info.env_use = use

    # ---- two to KNH_MAX_DELAY_STAGES delay stages of mixed kinds: in series, and reading a named earlier signal ----
    # two, three or four; a quarter of these seeds (HEAD_MANY_DELAYS) takes as many as the sixteen stages hold beside the
    # seed's other features -- twelve in a plain chain, where every delay's tile shares the fused pipeline's LDS, eight or so
    # in a graph -- and is restarted like every seed, so the restart kernel sees that many live rings
    if "delays" in feats:
        todo.remove("delays")
        k = _rank(seed, "delays")
        many = k % 8 in HEAD_MANY_DELAYS
        for j in range(L.KNH_MAX_DELAY_STAGES if many else 2 + k % 3):
            kind = DELAYS[(k + j) % 3]
            far = [m for m in mains[:-1] if m != len(b.st)]
            named = j % 2 == 1 and not chain and far
            if named and many and room() < 2:
                named = False
            if room() + need["delays"] < (2 if named else 1) or (j >= 2 and room() < (2 if named else 1)):
                break
            if named:  # beside the main signal, on an earlier one; summed in
                d = b.push(Stage(kind, 0, b.precise(kind), int(far[int(rng.integers(0, len(far)))])), b.ctor_for(kind))
                to(b.push(Stage(L.STAGE_MATH_ADD, input=mains[-1], input2=d)))
            else:
                to(b.push(Stage(kind, 0, b.precise(kind), 0 if chain or mains[-1] == len(b.st) else mains[-1]), b.ctor_for(kind)))
            info.delays += 1
            need["delays"] = 0
        if info.delays < 2:
            return None

    # ---- a Math1 function behind the signal ----
    if "math1" in feats:
        todo.remove("math1")
        kind = MATH1_EXACT[_rank(seed, "math1") % 5]
        if kind == L.STAGE_MATH1_SQRT and chain:
            kind = L.STAGE_MATH1_FRACT
        if kind == L.STAGE_MATH1_SQRT:  # sqrt(x * x + c), c > 0
            if room() + need["math1"] < 3:
                return None
            main = mains[-1]
            b.push(Stage(L.STAGE_MATH_MUL, input=main, input2=main))
            b.push(Stage(L.STAGE_ADD_CONST), rng.uniform(0.05, 1.0, n))
        else:  # scaled up first, so that the integers it lands on are not all 0 and -1
            b.push(Stage(L.STAGE_MUL_CONST, input=0 if chain or mains[-1] == len(b.st) else mains[-1]), np.full(n, float(rng.uniform(2.5, 6.0))))
        to(b.push(Stage(kind)))
        info.math1 = kind

    # ---- the rest, from the first path's pool; the limiter that keeps a runaway product finite ends the voice ----
    target = max(6, int(rng.integers(6, HEAD_MAX_STAGES + 1)))
    while len(b.st) < target - 1:
        kind = HEAD_FILL[int(rng.integers(0, len(HEAD_FILL)))]
        inp = 0 if chain or mains[-1] == len(b.st) else mains[-1]
        wrap = (WRAPPERS[int(rng.integers(0, len(WRAPPERS)))],) if rng.random() < 0.25 and len(b.st) < target - 2 else ()
        to(b.node(kind, input=inp, wrap=wrap))
    if len(b.st) > HEAD_MAX_STAGES - 1:
        return None
    last = b.push(Stage(L.STAGE_SAFETY_LIMITER, input=0 if chain or mains[-1] == len(b.st) else mains[-1]))
    if "connected" in feats:  # the last stage and an earlier node output, either way round
        earlier = sorted({m for m in mains if m != last})
        other = int(earlier[int(rng.integers(0, len(earlier)))])
        outs = (other - 1, last - 1) if seed % 2 else (last - 1, other - 1)
        before = node_output(b.st, mains[-1] - 1)
        if _rank(seed, "connected") % 6 == 4 and before != other - 1:
            # ... and in a sixth of these seeds neither is the last stage: the signal in front of the limiter instead, so that
            # the last stage's signal is one nobody reads and its slot is not held (no stage that can finish lies behind it)
            outs = tuple(before if o == last - 1 else o for o in outs)
    st = b.st
    info.chain = not is_graph(st, outs)
    w = configs.Workload(f"head{seed}", st, n, bs, L.F64 if f64 else L.F32, 2 if outs else 1)
    w.ctor, w.buffer, w.links = b.ctor, b.buffer, dict(b.links)
    w.pool, w.wavetables, w.outs, w.reassign = pool, wavetables, outs, reassign
    w.restart_block, w.restart_voices = HEAD_RESTART_BLOCK, np.arange(0, n, 3, dtype=np.uint32)
    w.info, w.seed, w.attempt = info, seed, attempt
    w.events = _head_events(seed, w)
    return w


def _head_events(seed, w):
    """The nine blocks' parameter traffic: the first path's six blocks of it, then -- in front of block 6, where every third
    voice starts again as fresh nodes -- every envelope triggered and every delay time set once more, so that the restarted
    voices sound; and the OscWt's frequency moved in block 1 (through WrSmoothParams or at an offset inside the block where
    the stage has them)."""
    st, n, bs = w.stages, w.n_voices, w.block_size
    base = _random_events(seed, st, n, bs, w.links)
    script = {k: [e + (None,) for e in ev] for k, ev in base.script.items()}
    rng = np.random.default_rng([13000, seed])
    v = np.arange(n, dtype=np.uint32)
    again = script.setdefault(HEAD_RESTART_BLOCK, [])
    for i, s in enumerate(st):
        if s.kind in ENVELOPES:
            again.append((v, i, 3 if s.kind == L.STAGE_MUL_ENV_ASR else 2, L.VALUE_TRIGGER, None, None, None))
        if s.kind == L.STAGE_MUL_ENV_ASR:
            script.setdefault(7, []).append((v[::2], i, 2, L.VALUE_TRIGGER, None, None, None))
        if s.kind in DELAYS:
            again.append((v, i, 0, L.VALUE_FLOAT, rng.uniform(0.0001, min(0.004, 1.5 * bs / configs.SAMPLE_RATE), n), None, None))
        if s.kind == L.STAGE_SIN_WT and s.flags & WT and not s.ar_param and not s.flags & L.STAGE_FLAG_AR_FREQ:
            if s.flags & L.STAGE_FLAG_SMOOTH_PARAMS:  # Linear(1.5 blocks) at Rate::BlockRate, then the new value
                script[1].append((v, i, 0, L.VALUE_SMOOTHING, np.full(n, 1.5 * bs / configs.SAMPLE_RATE), None, np.ones(n, dtype=np.int64)))
            delays = rng.integers(0, bs, n).astype(np.uint16) if s.delayed_changes_per_block else None
            script[1].append((v, i, 0, L.VALUE_FLOAT, rng.uniform(80.0, 2500.0, n), delays, None))

    if seed % 6 == 0:
        # The seeds tests/test_gpu_graph_voices.py renders as two calls per block: every offset inside the block lies in the
        # first part.  A change that is due behind the point where a call ends is forgotten by WrPreciseTiming, in the
        # reference (precise_timing.rs:65-114: the queue's count goes back to 0 at the end of every process_block) as on
        # the device (voice_bank.hpp: "behind a change that is not due in this block: never reached"), so a block in two
        # calls and the block in one are not the same voice then.
        first = head_split_point(bs)
        script = {k: [(sel, i, p, kind, f, None if d is None else (np.asarray(d) % first).astype(np.uint16), iv) for (sel, i, p, kind, f, d, iv) in ev]
                  for k, ev in script.items()}

    def events(block, bank):
        for (sel, i, p, kind, f, d, iv) in script.get(block, []):
            bank.param_apply_many(sel, i, p, kind, f, iv, d)
    events.script = script
    return events


def head_split_point(block_size):
    """where the "split" way cuts a block: 40 + rest frames, 17 + rest at block size 48"""
    return 17 if block_size == 48 else 40


@functools.lru_cache(maxsize=None)
def random_voice_head(seed):
    """-> Workload of the seed's voice of 6 .. 16 stages, as random_graph_voice's, plus .pool (a reader's pool: stage, Buffers,
    entry per voice), .reassign {block: (voices, entries, ctor rows)}, .wavetables (stage, entries, entry per voice), .outs
    (the two connected outputs' stages, or None), .restart_block and .restart_voices, and .reference: the lowered oracle's
    run of the nine blocks (head_reference).  No seed is without a voice: a draw that does not fit, or whose oracle run is
    silent or not finite, is drawn again -- HEAD_ATTEMPTS deterministic attempts, then an error."""
    why = []
    for attempt in range(HEAD_ATTEMPTS):
        w = _head_attempt(seed, attempt)
        if w is None:
            why.append("does not fit")
            continue
        ref = head_reference(w)
        planes = ref.voices if w.outs else ref.voices[:, None]
        peak = np.abs(planes).max(axis=(0, -1))  # [plane, voice]
        if not (np.isfinite(ref.voices).all() and np.isfinite(ref.mix).all()):
            why.append("not finite")
        elif not (peak > 1e-4).all():
            why.append("silent")
        elif not (np.abs(planes[HEAD_RESTART_BLOCK:, :, w.restart_voices]).max(axis=(0, -1)) > 1e-4).all():
            why.append("silent after the restart")
        else:
            w.reference = ref
            return w
    raise AssertionError(f"seed {seed}: no voice in {HEAD_ATTEMPTS} attempts ({why})")


# ---- the reference of such a voice: the oracle, through lowerings that are themselves pinned ----------------------------
def lower_for_oracle(w):
    """The voice spelled the way the oracle knows -> one plane per output: namespace(stages, smap, ctor, end, in_channels,
    ones_channel, reader).  smap[i]: the lowered index of stage i (parameter calls go there).
      * WAVETABLE on a pool of sine Wavetables is the same stage without the flag: SinWt (tests/test_gpu_wavetable.py holds
        OscWt on a sine table to SinWt bit for bit);
      * ENV_SOURCE is env_source_cases.twin(): an all-ones bank input in front of the same stage without the flag
        (tests/test_env_source_twin.py pins it);
      * two connected outputs are two planes: the stage list cut behind each output's node (env_source_cases.twin_run);
      * a reader whose voices are given other Buffers while the bank runs is a bank input in front of `* 1.0`, one input
        channel per voice: the readers themselves are oracle banks of their own, one per pool entry and generation, as
        tests/sampler_pool.py's Expected builds them (PoolReaders), and their rows are that input."""
    st, n = list(w.stages), w.n_voices
    outs = w.outs if connected(st, w.outs) else None
    ends = [len(st)] if outs is None else [node_output(st, o) + 1 for o in outs]
    lowered_reader = w.pool[0] if w.pool and w.reassign else None
    planes = []
    for end in ends:
        first, smap1, ctor1 = [], [], {}
        for i, s in enumerate(st[:end]):
            if i == lowered_reader:
                ctor1[len(first)] = np.arange(n, dtype=np.float64).reshape(n, 1)  # voice v reads input channel v
                first.append(Stage(L.STAGE_INPUT))
                ctor1[len(first)] = np.ones((n, 1))
                smap1.append(len(first))
                first.append(Stage(L.STAGE_MUL_CONST))
                continue
            smap1.append(len(first))
            if i in w.ctor:
                ctor1[len(first)] = w.ctor[i]
            first.append(s)
        shift = lambda k: 0 if k == 0 else 1 + smap1[k - 1]
        for i, s in enumerate(st[:end]):
            if i != lowered_reader:
                first[smap1[i]] = Stage(s.kind, s.flags & ~WT, s.delayed_changes_per_block, shift(s.input), shift(s.input2), s.ar_param)
        stages, smap2 = esc.twin(first)
        has_ones = len(stages) != len(first)
        ones_channel = n if lowered_reader is not None and lowered_reader < end else 0
        ctor = {smap2[k]: a for k, a in ctor1.items()}
        for k, s in enumerate(stages):
            if s.kind == L.STAGE_INPUT and k not in ctor:
                ctor[k] = np.full((n, 1), float(ones_channel))
        reader_here = lowered_reader is not None and lowered_reader < end
        planes.append(types.SimpleNamespace(stages=stages, smap=[smap2[k] for k in smap1], ctor=ctor, end=end,
                                            in_channels=(n if reader_here else 0) + (1 if has_ones else 0),
                                            ones_channel=ones_channel if has_ones else None, reader=reader_here))
    return planes


class PoolReaders:
    """The readers of a pooled, reassigned voice alone: one oracle bank [BufferReader, * 1.0] per (generation, pool entry),
    every voice on that entry, of which the rows of the voices that are on it are kept -- tests/sampler_pool.py's Expected,
    for this module's readers.  A reassigned or restarted voice continues as its row of a fresh bank."""

    def __init__(self, oracle, w):
        self.oracle, self.w = oracle, w
        stage, self.buffers, ids = w.pool
        self.stage = stage
        self.desc = [Stage(L.STAGE_BUFFER_READER, 0, w.stages[stage].delayed_changes_per_block), Stage(L.STAGE_MUL_CONST)]
        self.ids = np.array(ids, dtype=np.int64)
        self.gen = np.zeros(w.n_voices, dtype=np.int64)
        self.ctor = np.array(w.ctor[stage], dtype=np.float64)  # the constructor arguments each voice holds now
        self.banks = {}
        self._open(0)

    def _open(self, gen):
        w = self.w
        for e in sorted(set(self.ids[self.gen == gen].tolist())):
            o = self.oracle.OracleBank(self.desc, w.n_voices, w.sample_type, 1, False, True)
            o.set_ctor_args(0, self.ctor)
            o.set_ctor_args(1, np.ones((w.n_voices, 1)))
            o.set_buffer(0, *self.buffers[e])
            o.init(configs.SAMPLE_RATE, w.block_size)
            self.banks[(gen, e)] = o
        live = set(zip(self.gen.tolist(), self.ids.tolist()))
        for key in [k for k in self.banks if k not in live]:
            self.banks.pop(key).close()

    def renew(self, block, voices, ids=None, ctor_rows=None):
        """In front of `block`: these voices get fresh readers (on other entries, with other constructor arguments)."""
        voices = np.asarray(voices, dtype=np.int64)
        if ids is not None:
            self.ids[voices] = ids
        if ctor_rows is not None:
            self.ctor[voices] = ctor_rows
        self.gen[voices] = block
        self._open(block)

    def param_apply_many(self, voices, stage, param, kinds, fvalues=None, ivalues=None, delays=None):
        for o in self.banks.values():
            o.param_apply_many(voices, 0, param, kinds, fvalues, ivalues, delays)

    def process_block(self):
        """-> (rows [n, bs], done [n])"""
        w = self.w
        rows = np.zeros((w.n_voices, w.block_size), dtype=np.float64 if w.sample_type == L.F64 else np.float32)
        done = np.full(w.n_voices, NOT_DONE, dtype=np.uint32)
        for (g, e), o in self.banks.items():
            _, r, _, d = o.process_block()
            mine = (self.gen == g) & (self.ids == e)
            rows[mine], done[mine] = r[mine], d[mine]
        return rows, done

    def close(self):
        for o in self.banks.values():
            o.close()
        self.banks = {}


class HeadOracle:
    """The lowered oracle of a voice of random_voice_head, with the call surface head_edits uses on the device bank:
    param_apply_many, assign_buffers, restart_voices, process_block.  Restarted voices continue as their rows of freshly built
    banks that run from their own block 0 (constructor arguments as the voices hold them then) and get the same calls as
    the device from there on; the other voices continue on the first banks."""

    def __init__(self, oracle, w):
        self.oracle, self.w = oracle, w
        self.planes = lower_for_oracle(w)
        self.readers = PoolReaders(oracle, w) if any(p.reader for p in self.planes) else None
        self.full = max(range(len(self.planes)), key=lambda k: self.planes[k].end)  # holds every finishing stage
        self.gen = np.zeros(w.n_voices, dtype=np.int64)
        self.block = 0
        self.banks = {0: self._build()}
        self.dtype = np.float64 if w.sample_type == L.F64 else np.float32

    def _build(self):
        w, out = self.w, []
        for p in self.planes:
            o = self.oracle.OracleBank(p.stages, w.n_voices, w.sample_type, 1, self.readers is None, True)
            if p.in_channels:
                o.set_in_channels(p.in_channels)
            for s, a in p.ctor.items():
                o.set_ctor_args(s, a)
            if w.buffer is not None and w.buffer[0] < p.end:
                o.set_buffer(p.smap[w.buffer[0]], w.buffer[1], w.buffer[2])
            if w.pool and not p.reader and w.pool[0] < p.end:
                raise AssertionError("a pooled reader that is never reassigned is not drawn")
            o.init(configs.SAMPLE_RATE, w.block_size)
            out.append(o)
        return out

    def param_apply_many(self, voices, stage, param, kinds, fvalues=None, ivalues=None, delays=None):
        if self.readers is not None and stage == self.readers.stage:
            return self.readers.param_apply_many(voices, stage, param, kinds, fvalues, ivalues, delays)
        for banks in self.banks.values():
            for p, o in zip(self.planes, banks):
                if stage < p.end:
                    o.param_apply_many(voices, p.smap[stage], param, kinds, fvalues, ivalues, delays)

    def assign_buffers(self, stage, voices, ids, ctor=None):
        assert self.readers is not None and stage == self.readers.stage and ctor is not None
        self.readers.renew(self.block, voices, ids, ctor)

    def restart_voices(self, voices):
        voices = np.asarray(voices, dtype=np.int64)
        self.gen[voices] = self.block
        self.banks[self.block] = self._build()
        if self.readers is not None:
            self.readers.renew(self.block, voices)

    def process_block(self):
        """-> (mix [planes, bs], voices [n, bs] ([2, n, bs] with connected outputs), flags, done [n])"""
        w = self.w
        rows = reader_done = None
        if self.readers is not None:
            rows, reader_done = self.readers.process_block()
        planes, mixes = [], []
        done = np.full(w.n_voices, NOT_DONE, dtype=np.uint32)
        own_flags = 0
        for k, p in enumerate(self.planes):
            voices = np.zeros((w.n_voices, w.block_size), dtype=self.dtype)
            mix = None
            for g, banks in self.banks.items():
                o = banks[k]
                if p.in_channels:
                    ins = ([rows] if p.reader else []) + ([np.ones((1, w.block_size), dtype=self.dtype)] if p.ones_channel is not None else [])
                    o.set_input(np.concatenate(ins))
                mix, r, f, d = o.process_block()
                mine = self.gen == g
                voices[mine] = r[mine]
                if k == self.full:
                    done[mine] = d[mine]
                    own_flags = f
            planes.append(voices)
            # the oracle's own Add chain while the bank is one graph; the same fold over the assembled rows afterwards
            mixes.append(mix[0] if len(self.banks) == 1 and self.readers is None else _left_fold(voices))
        if reader_done is not None:
            done = np.where(done != NOT_DONE, done, reader_done)
        self.block += 1
        # ANY_DONE: the oracle's own flag while one bank (the plane that holds every finishing stage) is the reference;
        # read off the assembled done frames once voices continue on banks of their own
        flags = own_flags if len(self.banks) == 1 and self.readers is None else (L.FLAG_ANY_DONE if (done != NOT_DONE).any() else 0)
        return np.stack(mixes), (np.stack(planes) if len(planes) == 2 else planes[0]), flags, done

    def close(self):
        for banks in self.banks.values():
            for o in banks:
                o.close()
        if self.readers is not None:
            self.readers.close()


def head_edits(w, block, bank, restart=True):
    """What happens in front of `block`, on the device bank and on HeadOracle alike: the reassignments, the restart, then the
    block's parameter calls (calls made before a restart are dropped for the restarted voices, so they come after it)."""
    if block in w.reassign:
        voices, ids, rows = w.reassign[block]
        bank.assign_buffers(w.pool[0], voices, ids, ctor=rows)
    if restart and block == w.restart_block:
        bank.restart_voices(w.restart_voices)
    w.events(block, bank)


def head_reference(w, blocks=HEAD_BLOCKS):
    """-> namespace(voices [blocks, ...], mix [blocks, planes, bs], flags [blocks], done [blocks, n]) of the lowered oracle
    through the whole scenario, read-only"""
    from oracle import oracle_py
    oracle_py.load()
    o = HeadOracle(oracle_py, w)
    out = [[], [], [], []]
    for b in range(blocks):
        head_edits(w, b, o)
        mix, voices, flags, done = o.process_block()
        for k, x in enumerate((voices, mix, flags, done)):
            out[k].append(np.copy(x))
    o.close()
    res = [np.stack(x) for x in out]
    for x in res:
        x.setflags(write=False)
    return types.SimpleNamespace(voices=res[0], mix=res[1], flags=res[2], done=res[3])


def head_gpu_bank(knh, w, mix_mode=L.MIX_LEFT_FOLD, **kw):
    """The device bank of a voice of random_voice_head: gpu_bank, plus the Wavetable pool and the connected outputs."""
    b = knh.VoiceBank(w.stages, w.n_voices, w.sample_type, w.out_channels, mix_mode, -1, False, **kw)
    for s, a in w.ctor.items():
        b.set_ctor_args(s, a)
    if w.buffer is not None:
        b.set_buffer(*w.buffer)
    if w.pool:
        stage, buffers, ids = w.pool
        for k, (samples, sr) in enumerate(buffers):
            index = b.add_buffer(stage, samples, sr)
            assert index == k
        b.assign_buffers(stage, np.arange(w.n_voices, dtype=np.uint32), ids)
    if w.wavetables:
        stage, entries, of_voice = w.wavetables
        sine = wavetable_ref.sine_table(b.dtype)
        for k, e in enumerate(entries):
            index = b.add_wavetable(stage, np.tile(sine, (wavetable_ref.N_TABLES, 1)) if e == "seventeen" else sine)
            assert index == k
        b.assign_wavetables(stage, np.arange(w.n_voices, dtype=np.uint32), of_voice)
    if w.outs:
        b.connect_outputs(*w.outs)
    b.init(configs.SAMPLE_RATE, w.block_size)
    return b
