"""The six Math1UGen stages (ceil sqrt floor trunc fract exp: knaster_core_dsp/src/ugens/math.rs:167-305) at the C-ABI
boundary, on a machine without a GPU: the kind values in the header, the ctypes layer and the Rust bindings agree, a chain
with such a stage is accepted and counted, what cannot apply to a stage without parameters is refused, and a chain, a graph
voice and a lane-per-frame voice holding all six compile for gfx950 (the compile is host work: tests/test_jit_compile.py)."""
import os
import re
import subprocess

import pytest

from knaster_amd import _lib as L
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "bin", "jit_compile_check")

# the reference's declaration order (math.rs:167-305)
MATH1 = {"CEIL": 40, "SQRT": 41, "FLOOR": 42, "TRUNC": 43, "FRACT": 44, "EXP": 45}


def test_kind_values_agree_between_header_ctypes_and_rust():
    header = open(os.path.join(ROOT, "include", "knaster_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "ffi.rs")).read()
    for name, value in MATH1.items():
        assert re.search(rf"\bKNH_STAGE_MATH1_{name} = {value},", header), name
        assert re.search(rf"pub const KNH_STAGE_MATH1_{name}: u16 = {value};", ffi), name
        assert getattr(L, "STAGE_MATH1_" + name) == value
        assert L.STAGE_CTOR_ARGS[value] == 0
    assert re.search(r"\bKNH_STAGE_KIND_COUNT = 46\b", header)
    assert re.search(r"pub const KNH_STAGE_KIND_COUNT: u16 = 46;", ffi)
    assert re.search(r"#define KNH_ABI_VERSION 4\b", header) and L.KNH_ABI_VERSION == 4  # new enum values only


@pytest.mark.parametrize("name", list(MATH1))
def test_a_chain_with_the_stage_is_accepted_and_counted(knh, name):
    kind = MATH1[name]
    assert knh.chain_ugen_count([Stage(kind)]) == 1                       # one reference node per stage
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(kind)]
    assert knh.chain_ugen_count(st) == 1 + 2 + 1
    b = knh.VoiceBank(st, 5, L.F32, 1)
    assert b.stage_parameters(2) == 0 and b.stage_param_descriptions(2) == []
    plain = knh.VoiceBank(st[:2], 5, L.F32, 1)
    assert b.algorithmic_bytes_per_voice_block() == plain.algorithmic_bytes_per_voice_block()  # no state: nothing moves
    assert b.debug_signature() == "Wm" + "crftwe"[kind - 40]
    plain.close()
    b.close()
    # it reads `input` like any other stage: a graph voice
    g = knh.VoiceBank([Stage(L.STAGE_SIN_WT), Stage(L.STAGE_SIN_WT), Stage(kind, input=1), Stage(L.STAGE_MATH_ADD, input=3, input2=2)], 3, L.F64, 1)
    assert "@" in g.debug_signature()
    g.close()


@pytest.mark.parametrize("name", list(MATH1))
def test_what_needs_a_parameter_is_refused(knh, name):
    kind = MATH1[name]
    src = Stage(L.STAGE_SIN_WT)
    for bad in ([Stage(kind)],                                                         # stage 0: no signal to read
                [src, src, Stage(kind, ar_param=1, input2=1)],                         # an audio-rate parameter it does not have
                [src, Stage(kind, delayed_changes_per_block=2)],                       # WrPreciseTiming around no parameters
                [src, Stage(kind, flags=L.STAGE_FLAG_SMOOTH_PARAMS)],                  # WrSmoothParams around no parameters
                [src, src, Stage(kind, input2=1)]):                                    # a second operand
        with pytest.raises(L.KnasterHipError) as e:
            knh.VoiceBank(bad, 4, L.F32, 1)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        message = str(e.value).split(":", 1)[1].strip()
        assert message and "unknown stage kind" not in message  # refused for what it asks, with a message that says so
    b = knh.VoiceBank([src, Stage(kind)], 4, L.F32, 1)
    for call in (lambda: b.param_apply(0, 1, 0, 1.0), lambda: b.set_delay_within_block_for_param(0, 1, 0, 3),
                 lambda: b.param_apply_range(0, 4, 1, 0, L.VALUE_FLOAT, 1.0),
                 lambda: b.param_apply_many([0, 1, 2, 3], 1, 0, L.VALUE_FLOAT, [1.0] * 4)):
        with pytest.raises(L.KnasterHipError) as e:
            call()
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "no parameters" in str(e.value)
    b.close()


def _all_six_graph(knh):
    """Two oscillators, every Math1 stage, a fan-out (stage 3 is read twice) and a MathUGen: a voice that is a graph."""
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST, input=1),
          Stage(L.STAGE_MATH1_TRUNC), Stage(L.STAGE_MATH1_FRACT, input=3), Stage(L.STAGE_MATH_ADD, input=4, input2=5),
          Stage(L.STAGE_MATH1_CEIL), Stage(L.STAGE_MATH1_FLOOR, input=2), Stage(L.STAGE_MATH1_EXP),
          Stage(L.STAGE_MATH_MUL, input=7, input2=9), Stage(L.STAGE_MATH1_SQRT)]
    b = knh.VoiceBank(st, 3, L.F32, 1)
    sig = b.debug_signature()
    b.close()
    assert "@" in sig and all(c in sig for c in "crftwe")
    return sig


@pytest.fixture(scope="module")
def jit_compile_check(knh):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/jit_compile_check"], check=True, capture_output=True)
    assert os.path.exists(CHECK)


@pytest.mark.parametrize("what,args", [("chain", []), ("chain", ["f64", "pipe"]), ("graph", []), ("graph", ["f64", "frame"]), ("chain", ["frame"])])
def test_voices_holding_all_six_compile_for_gfx950(knh, jit_compile_check, what, args):
    signature = "Wmcrftwe" if what == "chain" else _all_six_graph(knh)
    p = subprocess.run([CHECK, signature] + args, cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, f"{signature} {args}: rc {p.returncode}: {p.stdout.decode(errors='replace')[-800:]}"
