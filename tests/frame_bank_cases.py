"""Lane-per-frame banks of 512 voices and more: the voices, the case tables and the references of
tests/test_gpu_frame_banks.py.

The voices per workgroup (`vpw`) in the tables are literal numbers, worked out by hand from the rule the library applies
(voice_bank.hpp init for the kernel built at init, kernels_interp.hip interp_voices_per_workgroup for the interpreter):
    tpv = block_size rounded up to a multiple of 64 threads
    vpw = min(max(1, n_voices // 256), 1024 // tpv), then lowered until the LDS fits
      built kernel:  64 KiB table + vpw * (state words rounded up to 4) * word size            <= 156 KiB
      interpreter:   64 KiB table + 16 B per stage + vpw * (state words, padded to 16 B, + n_sig * frames * word size) <= 158 KiB
They are NOT computed from that rule here: a change of the rule has to show as an edit of these tables.

References come from the CPU oracle (one node per stage), computed once per case and shared read-only by the two forms."""
from __future__ import annotations

import functools

import numpy as np

from helpers import make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

KF = L.VALUE_FLOAT

# the two lane-per-frame forms: environment, the form the bank must report in debug word 2
FORM_ENVS = ("KNH_INTERP", "KNH_FRAME_JIT", "KNH_JIT", "KNH_JIT_PIPE", "KNH_JIT_WAVES", "KNH_PIPELINE", "KNH_WIDE", "KNH_RESIDENT",
             "KNH_HOST_THREADS", "KNH_DEV_EVENTS")
FORMS = {"built": ({}, L.DEBUG_FORM_FRAME_JIT), "interp": ({"KNH_FRAME_JIT": "0"}, L.DEBUG_FORM_FRAME_INTERP)}


def freeze(a):
    a.setflags(write=False)
    return a


def cascade(depth, n, bs, sample_type):
    """configs.fm_cascade with add = 19: `depth` SinWt, 3 state words each, and 2 * depth - 2 constants of one word:
    5 * depth - 2 state words, 4 signal rows (debug_signature ends in "#4"); voice v's oscillators are detuned by 1 + v / 1000."""
    return configs.fm_cascade(depth, n, bs, sample_type, add=19.0)


@functools.lru_cache(maxsize=None)
def cascade_reference(oracle, depth, n, bs, sample_type, blocks):
    """-> [blocks] per-voice signals [n, bs] of the oracle"""
    o = make_oracle(oracle, cascade(depth, n, bs, sample_type), want_mix=False)
    out = tuple(freeze(o.process_block()[1]) for _ in range(blocks))
    o.close()
    return out


# ---- a. several voices per workgroup, with and without spare threads --------------------------------------------------------
# (n_voices, block_size, vpw, what the last workgroup holds)
#   bs 64: tpv 64, the threads allow 16.  512 // 256 = 513 // 256 = 2;  4096 // 256 = 4113 // 256 = 16.
#   bs 100: tpv 128, the threads allow 8 = 2057 // 256.   bs 16: tpv 64, 16 live lanes of 64.
SEVERAL = [
    (512, 64, 2, "full"),
    (513, 64, 2, "one voice, one shadow"),
    (4096, 64, 16, "full, 1 024 threads"),
    (4113, 64, 16, "one voice, fifteen shadows"),
    (2057, 100, 8, "one voice, seven shadows; 100 live lanes of 128"),
    (513, 16, 2, "one voice, one shadow; 16 live lanes of 64"),
]
SEVERAL_DEPTH, SEVERAL_BLOCKS = 8, 3


# ---- b. parameter changes that differ per voice within a workgroup ----------------------------------------------------------
# The voice: (0.5 * SinWt(f1) + 0.3 * SinWt(f2) + fract(1.7 * SinWt(f3))) * c.  The oracle has no Math1UGen, so the expected
# signal is composed as tests/test_gpu_math1.py composes it: the oracle renders x = 0.5 s1 + 0.3 s2 and y = 1.7 s3 (the same
# stages, the same parameter calls), numpy does (x + (y - trunc(y))) * c -- one IEEE operation per stage in the sample type,
# which rounds the same on both sides.
TRAFFIC_STAGES = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST),                 # 1, 2
                  Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST),                 # 3, 4
                  Stage(L.STAGE_MATH_ADD, input=2, input2=4),                      # 5: x
                  Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST),                 # 6, 7: y
                  Stage(L.STAGE_MATH1_FRACT, input=7),                             # 8
                  Stage(L.STAGE_MATH_ADD, input=5, input2=8),                      # 9
                  Stage(L.STAGE_MUL_CONST)]                                        # 10: * c
TRAFFIC_BLOCKS = 5
TRAFFIC = [(513, 2), (4113, 16)]  # (n_voices, vpw) at bs 64: 513 // 256, 4113 // 256


def traffic_ctor(n):
    v = np.arange(n, dtype=np.float64)
    return {0: 110.0 + 0.37 * v, 1: np.full(n, 0.5), 2: 171.0 + 0.53 * v, 3: np.full(n, 0.3), 5: 63.0 + 0.29 * v, 6: np.full(n, 1.7),
            9: np.full(n, 0.25)}


def traffic_workload(n, bs=64, sample_type=L.F32):
    w = configs.Workload("frame_traffic", TRAFFIC_STAGES, n, bs, sample_type, 1)
    w.ctor = {s: a.reshape(n, 1) for s, a in traffic_ctor(n).items()}
    return w


def traffic_calls(n, block):
    """The parameter calls made before `block`: [(stage of the device voice, voices, values)], in call order."""
    v = np.arange(n, dtype=np.uint32)
    if block == 1:  # a new frequency on every third voice
        return [(0, v[::3], 300.0 + 0.41 * v[::3])]
    if block == 2:  # a new constant on every voice
        return [(9, v, 0.05 + 0.9 * ((v * 37) % 101) / 101.0)]
    if block == 3:  # three changes of the same frequency on the last voice only: the last one wins
        last = np.array([n - 1] * 3, dtype=np.uint32)
        return [(5, last, np.array([500.0, 90.0, 222.0]))]
    if block == 4:  # the last two voices
        return [(2, v[n - 2:], np.array([640.0, 77.0]))]
    return []


@functools.lru_cache(maxsize=None)
def traffic_reference(oracle, n, without=None):
    """-> [TRAFFIC_BLOCKS] expected per-voice signals [n, 64], f32; without: a block whose calls are left out (the tests'
    premise: those calls are heard)"""
    x_w = configs.Workload("frame_traffic_x", TRAFFIC_STAGES[:5], n, 64, L.F32, 1)
    y_w = configs.Workload("frame_traffic_y", TRAFFIC_STAGES[5:7], n, 64, L.F32, 1)
    ctor = traffic_ctor(n)
    x_w.ctor = {s: ctor[s].reshape(n, 1) for s in (0, 1, 2, 3)}
    y_w.ctor = {s - 5: ctor[s].reshape(n, 1) for s in (5, 6)}
    ox, oy = make_oracle(oracle, x_w, want_mix=False), make_oracle(oracle, y_w, want_mix=False)
    c = ctor[9].astype(np.float32)
    out = []
    for b in range(TRAFFIC_BLOCKS):
        for stage, voices, values in ([] if b == without else traffic_calls(n, b)):
            if stage < 5:
                ox.param_apply_many(voices, stage, 0, KF, values)
            elif stage < 7:
                oy.param_apply_many(voices, stage - 5, 0, KF, values)
            else:
                c = c.copy()
                c[voices] = values.astype(np.float32)  # Constant::param_apply: F::new(value)
        x, y = ox.process_block()[1], oy.process_block()[1]
        out.append(freeze((x + (y - np.trunc(y))) * c.reshape(n, 1)))
    ox.close()
    oy.close()
    return tuple(out)


# ---- c. a block in two calls --------------------------------------------------------------------------------------------------
# bs 100 (tpv 128) as frames 0 .. 40 and 40 .. 100.  The built kernel keeps its shape; the interpreter chooses per call: the
# 40-frame call runs on tpv 64.  (n_voices, vpw of a whole block, the interpreter's vpw for the 40-frame call -- for the record,
# no diagnostic reports it):  1025 // 256 = 4 in both;  4113 // 256 = 16, the 128 threads per voice of a whole block allow 8.
SPLIT = [(1025, 4, 4), (4113, 8, 16)]
SPLIT_DEPTH, SPLIT_BS, SPLIT_AT, SPLIT_BLOCKS = 8, 100, 40, 2


def split_calls(n, block):
    """the frequency change made between the two calls of `block`: (stage, voices, values)"""
    v = np.arange(n, dtype=np.uint32)
    if block == 0:
        return 0, v[::2], 150.0 + 0.31 * v[::2]
    return 3, v[1::3], 95.0 + 0.17 * v[1::3]  # (stage 3: the cascade's second SinWt)


@functools.lru_cache(maxsize=None)
def split_reference(oracle, n, sample_type):
    """The oracle takes whole blocks only.  Every stage of the voice is a function of the oscillators' phases alone, so a bank
    of block size 20 (the common measure of 40, 60 and 100) renders the same samples -- asserted here, without changes, against
    the oracle at block size 100 -- and takes the change after its second block of each five, where the device gets it.
    -> [SPLIT_BLOCKS] per-voice signals [n, 100]"""
    assert cascade(SPLIT_DEPTH, n, 20, sample_type).stages[3].kind == L.STAGE_SIN_WT
    plain = make_oracle(oracle, cascade(SPLIT_DEPTH, n, 20, sample_type), want_mix=False)
    small = np.concatenate([plain.process_block()[1] for _ in range(5)], axis=1)
    plain.close()
    assert np.array_equal(small, cascade_reference(oracle, SPLIT_DEPTH, n, SPLIT_BS, sample_type, 1)[0])
    o = make_oracle(oracle, cascade(SPLIT_DEPTH, n, 20, sample_type), want_mix=False)
    out = []
    for b in range(SPLIT_BLOCKS):
        parts = [o.process_block()[1] for _ in range(2)]
        stage, voices, values = split_calls(n, b)
        o.param_apply_many(voices, stage, 0, KF, values)
        parts += [o.process_block()[1] for _ in range(3)]
        out.append(freeze(np.concatenate(parts, axis=1)))
    o.close()
    return tuple(out)


# ---- d. vpw limited by the LDS ------------------------------------------------------------------------------------------------
# Interpreter, f64, bs 128, 1 301 voices.  Twenty oscillators first, then 1.25 * s1 (s1 is read again at the end, so the
# product takes a 21st signal row), then the sum: 21 rows of 128 doubles = 21 504 B, 61 state words = 488 B padded to 496:
# 22 000 B per voice.  158 KiB - 64 KiB table - 41 stages * 16 B = 95 600 B: four voices (88 000 B), not five.  The voice count
# allows 1301 // 256 = 5, the threads 1024 // 128 = 8.  The built kernel keeps signals in registers: 5.
ROWS_N, ROWS_BS, ROWS_SIG = 1301, 128, 21
ROWS_VPW = {"interp": 4, "built": 5}
ROWS_VPW_BY_COUNT, ROWS_VPW_BY_THREADS = 5, 8


def rows_workload(n=ROWS_N, bs=ROWS_BS, sample_type=L.F64):
    st = [Stage(L.STAGE_SIN_WT) for _ in range(20)]
    st.append(Stage(L.STAGE_MUL_CONST, input=1))           # 21
    acc = 21
    for k in list(range(2, 21)) + [1]:
        st.append(Stage(L.STAGE_MATH_ADD, input=acc, input2=k))
        acc = len(st)
    w = configs.Workload("frame_rows", st, n, bs, sample_type, 1)
    scale = 1.0 + 0.001 * np.arange(n)
    w.ctor = {k: ((97.0 + 41.0 * k) * scale).reshape(n, 1) for k in range(20)}
    w.ctor[20] = np.full((n, 1), 1.25)
    return w


# Built kernel, f64, bs 64, 4 097 voices, fm_cascade of 150 oscillators: 5 * 150 - 2 = 748 state words (a multiple of 4) of
# 8 B = 5 984 B per voice beside the 64 KiB table; 156 KiB - 64 KiB = 94 208 B: fifteen voices (89 760 B), not sixteen
# (95 744 B).  The voice count (4097 // 256) and the threads (1024 // 64) allow 16.
# The interpreter on the same voice: 5 984 B of words + 4 rows * 64 * 8 B = 8 032 B per voice, the program 895 * 16 B =
# 14 320 B: 158 KiB - 64 KiB - 14 320 B = 81 936 B: ten voices.
DEEP_DEPTH, DEEP_N, DEEP_BS, DEEP_WORDS = 150, 4097, 64, 748
DEEP_VPW = {"built": 15, "interp": 10}
DEEP_VPW_BY_COUNT, DEEP_VPW_BY_THREADS = 16, 16


@functools.lru_cache(maxsize=None)
def workload_reference(oracle, which, blocks):
    w = rows_workload() if which == "rows" else cascade(DEEP_DEPTH, DEEP_N, DEEP_BS, L.F64)
    o = make_oracle(oracle, w, want_mix=False)
    out = tuple(freeze(o.process_block()[1]) for _ in range(blocks))
    o.close()
    return out


# ---- e. long blocks ---------------------------------------------------------------------------------------------------------------
# (n_voices, block_size, sample types, vpw): 513 // 256 = 2 = 1024 // 512;  three voices: one per workgroup, tpv 1 024
LONG = [(513, 512, (L.F32,), 2), (3, 1000, (L.F32, L.F64), 1), (3, 1024, (L.F32, L.F64), 1)]
LONG_DEPTH, LONG_BLOCKS = 8, 2

# ---- f. the tree fold beyond two passes: the rows are the voices, 256 to a pass ------------------------------------------------
# (n_voices, vpw at bs 48 = n_voices // 256 up to 16, passes of fold_tree_kernel = ceil(n_voices / 256), what they exercise)
TREE = [
    (769, 3, 4, "three whole passes and one row: the one-row pass carries over two levels"),
    (1297, 5, 6, "five whole passes and 17 rows (a chunk of 16, a chunk of one): two nodes left for the closing walk"),
    (1553, 6, 7, "six whole passes and 17 rows: three nodes of falling level left for the closing walk"),
    (1793, 7, 8, "seven whole passes and one row: the one-row pass carries over three levels"),
    (2048, 8, 8, "eight whole passes: every carry, one node left"),
    (4113, 16, 17, "sixteen whole passes (a carry over four levels) and 17 rows: two nodes left"),
]
TREE_DEPTH, TREE_BS, TREE_BLOCKS = 6, 48, 2

# ---- g. restart ---------------------------------------------------------------------------------------------------------------------
RESTART_N, RESTART_VPW, RESTART_R = 513, 2, [0, 255, 256, 512]  # the first voice, both sides of a workgroup pair, the lone last voice

# ---- h. voice ranges -----------------------------------------------------------------------------------------------------------------
# 1 301 voices at bs 64: one range 1301 // 256 = 5.  Two ranges of whole 64-voice groups: 704 and 597 voices, 2 each.
RANGES_N, RANGES_VPW_ONE, RANGES_VPW_FIRST = 1301, 5, 2


def restart_case():
    """tests/restart_cases.py's Case on the cascade voice: arguments B move every oscillator of the restarted voices"""
    import restart_cases as rc
    w = cascade(SEVERAL_DEPTH, RESTART_N, 64, L.F32)
    a = {s: c[:, 0] for s, c in w.ctor.items()}
    b = {s: c * 1.5 + 7.0 for s, c in a.items() if w.stages[s].kind == L.STAGE_SIN_WT}
    return rc.Case("frame_bank", w.stages, L.F32, 64, a, b, 2, 2, n=RESTART_N, r_sets={"edges": RESTART_R})


@functools.lru_cache(maxsize=None)
def restart_expected(oracle):
    import restart_cases as rc
    return rc.build_expected(restart_case(), "edges", lambda w: make_oracle(oracle, w, want_mix=False), rc.oracle_step)
