"""The connected voices of tests/test_stereo_out_abi.py and tests/test_gpu_stereo_out.py: stage lists, constructor arguments,
which two stages go to graph outputs 0 and 1, and the parameter calls of each block.  Only stages whose parity with the
oracle is bit-exact (no SinNumeric, powf, exp, no setter that runs on the device)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Tuple

import numpy as np

from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

S = Stage


def node_output(st, k):
    """The stage whose output a connection to stage k carries: the last of the wrapper stages that follow it."""
    wrappers = (L.STAGE_WR_MUL, L.STAGE_WR_ADD, L.STAGE_WR_SUB, L.STAGE_WR_VSUB, L.STAGE_WR_DIV, L.STAGE_WR_VDIV, L.STAGE_WR_POWF, L.STAGE_WR_POWI)
    while k + 1 < len(st) and st[k + 1].kind in wrappers:
        k += 1
    return k


@dataclass
class Case:
    stages: List[Stage]
    ctor: Dict[int, np.ndarray]
    connect: Tuple[int, int]
    # events(block, rig): the calls in front of block `block`; `rig` takes param_apply_many / param_apply /
    # set_delay_within_block_for_param and passes each on to the GPU bank and to the oracle views that hold the stage
    events: Callable = field(default=lambda block, rig: None)
    envelopes: Tuple[int, ...] = ()  # envelope stages (every voice gets a t_restart in front of block 0)


def _col(x, n):
    return np.asarray(x, dtype=np.float64).reshape(n, -1)


def _svf(p, n, scale=1.0):
    return np.stack([np.zeros(n), p["cutoff"] * scale, p["q"], np.zeros(n)], axis=1)


def case_a(n, precise=0):
    p = configs.voice_parameters(n)
    st = [S(L.STAGE_SIN_WT, delayed_changes_per_block=precise), S(L.STAGE_MUL_CONST), S(L.STAGE_SIN_WT), S(L.STAGE_MUL_CONST)]
    ctor = {0: _col(p["freq"], n), 1: _col(np.full(n, 0.5), n), 2: _col(p["freq"] * p["fm_ratio"], n), 3: _col(np.full(n, 0.25), n)}
    v = np.arange(n, dtype=np.uint32)

    def events(block, rig):
        if block == 1:  # changes at the start of a block, on either side
            rig.param_apply_many(v[::2], 0, 0, L.VALUE_FLOAT, 200.0 + v[::2])
            rig.param_apply_many(v, 3, 0, L.VALUE_FLOAT, np.full(n, 0.125))
    return Case(st, ctor, (1, 3), events)


def case_b(n):
    """A plain chain: the left signal (the raw oscillator) must survive the in-place filter."""
    p = configs.voice_parameters(n)
    st = [S(L.STAGE_SIN_WT), S(L.STAGE_SVF), S(L.STAGE_MUL_ENV_ASR)]
    ctor = {0: _col(p["freq"], n), 1: _svf(p, n), 2: np.tile([0.0005, 0.002], (n, 1))}
    v = np.arange(n, dtype=np.uint32)

    def events(block, rig):
        if block == 1:
            rig.param_apply_many(v[::3], 0, 0, L.VALUE_FLOAT, 300.0 + v[::3])
            rig.param_apply_many(v, 2, 2, L.VALUE_TRIGGER)  # t_release
    return Case(st, ctor, (0, 2), events, envelopes=(2,))


def case_c(n):
    """One oscillator into two filters, each with its own EnvAsr, one side each.  Released in front of block 1, both
    envelopes end in that block (19 and 38 frames later: also inside a 64-frame block), at different frames."""
    p = configs.voice_parameters(n)
    st = [S(L.STAGE_SIN_WT), S(L.STAGE_SVF), S(L.STAGE_MUL_ENV_ASR), S(L.STAGE_SVF, input=1), S(L.STAGE_MUL_ENV_ASR)]
    ctor = {0: _col(p["freq"], n), 1: _svf(p, n), 2: np.tile([0.0005, 0.0004], (n, 1)), 3: _svf(p, n, 0.5), 4: np.tile([0.0005, 0.0008], (n, 1))}
    v = np.arange(n, dtype=np.uint32)

    def events(block, rig):
        if block == 1:
            rig.param_apply_many(v, 2, 2, L.VALUE_TRIGGER)
            rig.param_apply_many(v, 4, 2, L.VALUE_TRIGGER)
    return Case(st, ctor, (2, 4), events, envelopes=(2, 4))


def case_d(n):
    """Dry left, a delayed copy right: the ring stage beside a held slot."""
    p = configs.voice_parameters(n)
    wf = np.asarray([3.0, 4.0, 5.0, 6.0])[np.arange(n) % 4]  # waveforms without sin
    st = [S(L.STAGE_POLYBLEP), S(L.STAGE_SAMPLE_DELAY)]
    ctor = {0: np.stack([wf, p["freq"]], axis=1), 1: _col(np.full(n, 0.003), n)}
    v = np.arange(n, dtype=np.uint32)

    def events(block, rig):
        if block == 0:
            rig.param_apply_many(v, 1, 0, L.VALUE_FLOAT, 0.0005 + 0.002 * (v % 7) / 7.0)  # delay_time, within the 0.003 s ring
    return Case(st, ctor, (0, 1), events)


def case_e(n):
    """An oscillator whose frequency another signal drives on the left, a free oscillator on the right."""
    p = configs.voice_parameters(n)
    st = [S(L.STAGE_SIN_WT), S(L.STAGE_MUL_CONST), S(L.STAGE_SIN_WT, ar_param=1, input2=2), S(L.STAGE_SIN_WT)]
    ctor = {0: _col(p["freq"] * 0.25, n), 1: _col(p["fm_index"] + 50.0, n), 2: _col(p["freq"], n), 3: _col(p["freq"] * p["fm_ratio"], n)}
    return Case(st, ctor, (2, 3))


def case_h(n):
    """Oscillators and arithmetic only: unconnected, the lane-per-frame class."""
    p = configs.voice_parameters(n)
    st = [S(L.STAGE_SIN_WT), S(L.STAGE_MUL_CONST), S(L.STAGE_SIN_WT), S(L.STAGE_MATH_MUL, input=2, input2=3)]
    ctor = {0: _col(p["freq"], n), 1: _col(np.full(n, 0.5), n), 2: _col(p["freq"] * p["fm_ratio"], n)}
    return Case(st, ctor, (1, 3))


def case_i(n):
    """Case A with the left oscillator in WrPreciseTiming<4, _>: freq changes at frames 5 and 37 of the second block."""
    c = case_a(n, precise=4)

    def events(block, rig):
        if block == 1:
            for voice in range(0, n, 3):
                rig.set_delay_within_block_for_param(voice, 0, 0, 5)
                rig.param_apply(voice, 0, 0, 150.0 + 7.0 * voice)
                rig.set_delay_within_block_for_param(voice, 0, 0, 37)
                rig.param_apply(voice, 0, 0, 900.0 - 5.0 * voice)
    return Case(c.stages, c.ctor, c.connect, events)


def case_m(n):
    """The right output feeds the left one through a join, an envelope on each side of it: left = E3(osc2) + E1(osc0),
    right = E1(osc0).  Released in front of block 1, E3 ends 19 frames later and E1 38.  The reference starts its search at
    the deepest output node only (the sum): E3's side is ordered first, E1 last."""
    p = configs.voice_parameters(n)
    st = [S(L.STAGE_SIN_WT), S(L.STAGE_MUL_ENV_ASR), S(L.STAGE_SIN_WT), S(L.STAGE_MUL_ENV_ASR), S(L.STAGE_MATH_ADD, input=4, input2=2)]
    ctor = {0: _col(p["freq"], n), 1: np.tile([0.0005, 0.0008], (n, 1)), 2: _col(p["freq"] * p["fm_ratio"], n), 3: np.tile([0.0005, 0.0004], (n, 1))}
    v = np.arange(n, dtype=np.uint32)

    def events(block, rig):
        if block == 1:
            rig.param_apply_many(v, 1, 2, L.VALUE_TRIGGER)
            rig.param_apply_many(v, 3, 2, L.VALUE_TRIGGER)
    return Case(st, ctor, (4, 1), events, envelopes=(1, 3))


CASES = {"M": case_m, "A": case_a, "B": case_b, "C": case_c, "D": case_d, "E": case_e, "H": case_h, "I": case_i}
