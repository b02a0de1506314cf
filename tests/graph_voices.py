"""Graph voices built from every stage kind (tests/test_graph_voices.py, tests/test_gpu_graph_voices.py): the seeded generator,
the directed voices, and a restatement in Python of what the library derives from a stage list -- the signal-slot plan of
build_signature and the envelopes' task order -- shared so that what the CPU test accepts and compiles is what the GPU test
runs.  random_dag of tests/test_gpu_dag.py draws from a small pool (SinWt, arithmetic, two filters, EnvAr); this one draws
from every kind and setting that another test already holds bit for bit."""
from __future__ import annotations

import os
import re

import numpy as np

import ar_sources
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


def is_source(s):
    return s.kind in SOURCES or s.kind in (L.STAGE_SIN_NUMERIC, L.STAGE_INPUT)


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


def slot_plan(st):
    """The signal slots of a graph voice: -> ([(slot of a, slot of b, slot written)] per stage, number of slots).  A stage
    takes the first free slot; a signal's slot is free again at its last reader; a stage that is not a MATH_* writes in place
    when its first operand dies at it.  A signal nobody reads holds its slot only while it is written; the last stage's
    signal is the voice's output."""
    a, b = operands(st)
    n = len(st)
    last = [max(r) if r else -1 for r in readers(st)]
    last[n - 1] = n
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
    num = lambda t: -1 if t == "_" else int(t)
    out = [(m.group(1), None if m.group(2) is None else int(m.group(2)), num(m.group(3)), num(m.group(4)), num(m.group(5)))
           for m in re.finditer(r"(.)(?:%(\d+))?@(_|\d+),(_|\d+),(_|\d+)", body)]
    return out, int(count)


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
