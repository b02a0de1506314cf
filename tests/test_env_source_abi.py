"""KNH_STAGE_FLAG_ENV_SOURCE at the C-ABI boundary, on a machine without a GPU: the flag's value in the header, the ctypes
layer and the Rust bindings agree; a chain with an envelope source is accepted and counted as ONE node; its parameters are
those of the multiplying form; what the flag cannot mean is refused with a message; no existing chain changes its
signature; and voices with each of the three sources compile for gfx950 (the compile is host work)."""
import os
import re
import subprocess

import pytest

import env_source_cases as ec
import graph_voices as gv
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "bin", "jit_compile_check")
ES = L.STAGE_FLAG_ENV_SOURCE
ENVS = {"ASR": L.STAGE_MUL_ENV_ASR, "AR": L.STAGE_MUL_ENV_AR, "ENVELOPE": L.STAGE_MUL_ENVELOPE}


def test_flag_value_agrees_between_header_ctypes_and_rust():
    header = open(os.path.join(ROOT, "include", "knaster_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "ffi.rs")).read()
    assert re.search(r"\bKNH_STAGE_FLAG_ENV_SOURCE = 1u << 4\b", header)
    assert re.search(r"pub const KNH_STAGE_FLAG_ENV_SOURCE: u16 = 1 << 4;", ffi)
    assert ES == 1 << 4
    assert re.search(r"#define KNH_ABI_VERSION 4\b", header) and L.KNH_ABI_VERSION == 4  # a new enum value only


def test_a_chain_with_a_source_is_accepted_and_counted_as_one_node(knh):
    src = [Stage(L.STAGE_MUL_ENV_ASR, flags=ES), Stage(L.STAGE_MUL_CONST)]
    assert knh.chain_ugen_count(src) == 1 + 2
    mul = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_ENV_ASR), Stage(L.STAGE_MUL_CONST)]
    assert knh.chain_ugen_count(mul) == 1 + 2 + 2          # `x * env` is the envelope and a Mul
    assert knh.chain_ugen_count(mul[1:]) == knh.chain_ugen_count(src) + 1
    b = knh.VoiceBank(src, 5, L.F32, 1)
    assert b.debug_signature() == "bm"
    b.close()
    for kind, c in ((L.STAGE_MUL_ENV_AR, "j"), (L.STAGE_MUL_ENVELOPE, "l")):
        b = knh.VoiceBank([Stage(kind, flags=ES)], 3, L.F64, 1)  # it may be stage 0, and the voice's only stage
        assert b.debug_signature() == c
        b.close()
    # a source after stage 0 makes the voice a graph, as every other source does
    g = knh.VoiceBank(ec.CASES["gain"].stages, 3, L.F32, 1)
    assert g.debug_signature() == "W@_,_,0A@0,_,0j@_,_,1m@1,_,1a@1,_,1m%0@0,1,0#2"
    g.close()
    # wrappers behind it wrap the envelope node: whoever names the source reads the last wrapper's output
    w = knh.VoiceBank([Stage(L.STAGE_MUL_ENV_ASR, flags=ES), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_WR_ADD), Stage(L.STAGE_SIN_WT),
                       Stage(L.STAGE_MATH_MUL, input=4, input2=1)], 3, L.F32, 1)
    assert w.debug_signature() == "b@_,_,0m@0,_,0a@0,_,0W@_,_,1*@1,0,0#2"
    w.close()


@pytest.mark.parametrize("name", list(ENVS))
def test_parameters_are_those_of_the_multiplying_form(knh, name):
    kind = ENVS[name]
    for flags in (0, L.STAGE_FLAG_SMOOTH_PARAMS):
        s = knh.VoiceBank([Stage(kind, flags=ES | flags, delayed_changes_per_block=0 if flags else 2)], 4, L.F32, 1)
        m = knh.VoiceBank([Stage(L.STAGE_SIN_WT), Stage(kind, flags=flags, delayed_changes_per_block=0 if flags else 2)], 4, L.F32, 1)
        assert s.stage_parameters(0) == m.stage_parameters(1) > 0
        assert s.stage_param_descriptions(0) == m.stage_param_descriptions(1)
        s.close()
        m.close()
    # the audio-rate parameters too: attack_time and release_time, or time_scale, driven by input2
    src = [Stage(L.STAGE_PHASOR), Stage(L.STAGE_MUL_CONST)]
    n_ar = 1 if kind == L.STAGE_MUL_ENVELOPE else 2
    for p in range(4):
        if p < n_ar:
            knh.VoiceBank(src + [Stage(kind, flags=ES, ar_param=p + 1, input2=2)], 4, L.F32, 1).close()
        else:
            with pytest.raises(L.KnasterHipError):
                knh.VoiceBank(src + [Stage(kind, flags=ES, ar_param=p + 1, input2=2)], 4, L.F32, 1)


def test_what_the_flag_cannot_mean_is_refused(knh):
    osc = Stage(L.STAGE_SIN_WT)
    bad = {
        "another kind": [osc, Stage(L.STAGE_MUL_CONST, flags=ES)],
        "a source kind": [Stage(L.STAGE_SIN_WT, flags=ES)],
        "with AR_FREQ": [osc, Stage(L.STAGE_MUL_ENV_ASR, flags=ES | L.STAGE_FLAG_AR_FREQ)],
        "with READER_CH1": [osc, Stage(L.STAGE_MUL_ENV_AR, flags=ES | L.STAGE_FLAG_READER_CH1)],
        "with WAVETABLE": [osc, Stage(L.STAGE_MUL_ENVELOPE, flags=ES | L.STAGE_FLAG_WAVETABLE)],
        "input": [osc, Stage(L.STAGE_MUL_ENV_ASR, flags=ES, input=1)],
        "input2 without ar_param": [osc, Stage(L.STAGE_MUL_ENV_ASR, flags=ES, input2=1)],
        "a second Envelope": [Stage(L.STAGE_MUL_ENVELOPE, flags=ES), Stage(L.STAGE_MUL_ENVELOPE)],
        "a second Envelope source": [osc, Stage(L.STAGE_MUL_ENVELOPE), Stage(L.STAGE_MUL_ENVELOPE, flags=ES)],
    }
    for what, stages in bad.items():
        with pytest.raises(L.KnasterHipError) as e:
            knh.VoiceBank(stages, 4, L.F32, 1)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, what
        message = str(e.value).split(":", 1)[1].strip()
        assert message and "unknown stage" not in message, what  # refused for what it asks, with a message that says so


def test_no_existing_chain_changes_its_signature(knh):
    """the strings of the commit before the flag"""
    want = {"C1": "Wm", "C2": "Nm", "C3": "WmSA", "C4": "WmSA", "C5": "WmaRm"}
    for name, sig in want.items():
        w = configs.config(name, n_voices=8, block_size=64)
        b = knh.VoiceBank(w.stages, w.n_voices, w.sample_type, w.out_channels)
        assert b.debug_signature() == sig, name
        b.close()
    w = gv.directed_voice("comb_asr_pan", 1, L.F32, 64)
    b = knh.VoiceBank(w.stages, w.n_voices, w.sample_type, w.out_channels)
    assert b.debug_signature() == "W@_,_,0m@0,_,0D@0,_,1+@0,1,0A@0,_,0J@0,_,0#2"
    b.close()


@pytest.fixture(scope="module")
def jit_compile_check(knh):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/jit_compile_check"], check=True, capture_output=True)
    assert os.path.exists(CHECK)


def _signature(knh, name):
    b = knh.VoiceBank(ec.CASES[name].stages, 3, L.F32, 1)
    sig = b.debug_signature()
    b.close()
    return sig


@pytest.mark.parametrize("case,args", [("pitch", []), ("pitch", ["f64", "pipe"]), ("filter", []), ("segments", [])])
def test_voices_with_a_source_compile_for_gfx950(knh, jit_compile_check, case, args):
    signature = _signature(knh, case)
    assert any(c in signature for c in "bjl")
    p = subprocess.run([CHECK, signature] + args, cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, f"{signature} {args}: rc {p.returncode}: {p.stdout.decode(errors='replace')[-800:]}"
