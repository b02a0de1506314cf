"""Two of a voice's signals connected to graph outputs 0 and 1 (knh_bank_connect_outputs / knh_bank_output_stage; the
reference's to_graph_out_channels, graph_edit.rs:363-394) at the C-ABI boundary, on a machine without a GPU: the header, the
Rust bindings and ctypes declare both functions; before init a connected bank is accepted, every refusal returns its status
and changes nothing; the signature names the two slots and stays what it was for an unconnected bank; the connected voices
of tests/test_gpu_stereo_out.py compile for gfx950 (the compile is host work: tests/test_jit_compile.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import stereo_cases as sc
from knaster_amd import _lib as L
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "bin", "jit_compile_check")
NONE = 0xFFFFFFFF

SIN, MUL, SVF, ASR = Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)
FOUR = [SIN, MUL, SIN, MUL]


def test_header_rust_and_ctypes_declare_both_functions():
    header = open(os.path.join(ROOT, "include", "knaster_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "ffi.rs")).read()
    assert re.search(r"int32_t\s+knh_bank_connect_outputs\(knh_bank\* bank, uint32_t n_channels, const uint32_t\* stages\);", header)
    assert re.search(r"uint32_t\s+knh_bank_output_stage\(const knh_bank\* bank, uint32_t channel\);", header)
    assert re.search(r"pub fn knh_bank_connect_outputs\(bank: \*mut knh_bank, n_channels: u32, stages: \*const u32\) -> i32;", ffi)
    assert re.search(r"pub fn knh_bank_output_stage\(bank: \*const knh_bank, channel: u32\) -> u32;", ffi)
    assert L.PROTOTYPES["knh_bank_connect_outputs"] == (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)])
    assert L.PROTOTYPES["knh_bank_output_stage"] == (C.c_uint32, [C.c_void_p, C.c_uint32])
    assert re.search(r"#define KNH_ABI_VERSION 4\b", header)  # a new entry point, not a new ABI


@pytest.mark.parametrize("kw", [{}, {"host_threads": 2}, {"devices": [0]}, {"rank": 0, "world": 1}])
def test_a_connected_bank_is_accepted_by_every_kind_of_bank(knh, kw):
    b = knh.VoiceBank(FOUR, 200, L.F32, 2, **kw)
    assert (b.output_stage(0), b.output_stage(1)) == (3, 3)
    b.connect_outputs(1, 3)
    assert (b.output_stage(0), b.output_stage(1)) == (1, 3)
    b.connect_outputs(3, 0)  # the last accepted call holds
    assert (b.output_stage(0), b.output_stage(1)) == (3, 0)
    assert b.output_stage(2) == NONE
    b.close()
    assert knh._lib.load().knh_bank_output_stage(None, 0) == NONE


def test_output_stage_is_the_node_output_when_a_wrapper_follows(knh):
    st = [SIN, Stage(L.STAGE_WR_MUL), Stage(L.STAGE_WR_ADD), SIN, MUL]
    b = knh.VoiceBank(st, 3, L.F32, 2)
    b.connect_outputs(0, 4)
    assert (b.output_stage(0), b.output_stage(1)) == (2, 4)
    same = b.debug_signature()
    b.connect_outputs(2, 4)  # naming the node or the last of its wrappers: the same connection
    assert b.debug_signature() == same
    b.connect_outputs(1, 4)
    assert b.output_stage(0) == 2 and b.debug_signature() == same
    b.close()


def _refused(b, call, status):
    before = (b.debug_signature(), b.output_stage(0), b.output_stage(1))
    with pytest.raises(L.KnasterHipError) as e:
        call()
    assert e.value.status == status, str(e.value)
    assert str(e.value).split(":", 1)[1].strip()  # a knh_last_error text
    assert (b.debug_signature(), b.output_stage(0), b.output_stage(1)) == before


def test_every_refusal_returns_its_status_and_changes_nothing(knh):
    lib = L.load()
    two = (C.c_uint32 * 2)(1, 3)
    assert lib.knh_bank_connect_outputs(None, 2, two) == L.ERR_INVALID_ARGUMENT
    b = knh.VoiceBank(FOUR, 70, L.F32, 2)
    b.connect_outputs(1, 3)
    _refused(b, lambda: b._check(lib.knh_bank_connect_outputs(b._h, 2, None)), L.ERR_INVALID_ARGUMENT)
    three = (C.c_uint32 * 3)(0, 1, 2)
    for n in (0, 1, 3):
        _refused(b, lambda: b._check(lib.knh_bank_connect_outputs(b._h, n, three)), L.ERR_INVALID_ARGUMENT)
    _refused(b, lambda: b.connect_outputs(4, 0), L.ERR_OUT_OF_RANGE)
    _refused(b, lambda: b.connect_outputs(0, 4), L.ERR_OUT_OF_RANGE)
    _refused(b, lambda: b.connect_outputs(0, NONE), L.ERR_OUT_OF_RANGE)
    b.close()
    mono = knh.VoiceBank(FOUR, 70, L.F32, 1)
    _refused(mono, lambda: mono.connect_outputs(1, 3), L.ERR_INVALID_ARGUMENT)
    mono.close()
    pan = knh.VoiceBank([SIN, MUL, Stage(L.STAGE_PAN2)], 70, L.F32, 2)
    _refused(pan, lambda: pan.connect_outputs(0, 1), L.ERR_INVALID_ARGUMENT)
    pan.close()
    gal = knh.VoiceBank([SIN, MUL, Stage(L.STAGE_GALACTIC)], 4, L.F32, 2)
    _refused(gal, lambda: gal.connect_outputs(0, 1), L.ERR_INVALID_ARGUMENT)
    gal.close()
    inp = knh.VoiceBank([Stage(L.STAGE_INPUT), MUL, SIN], 8, L.F32, 2, in_channels=1)
    _refused(inp, lambda: inp.connect_outputs(0, 2), L.ERR_INVALID_ARGUMENT)
    _refused(inp, lambda: inp.connect_outputs(2, 0), L.ERR_INVALID_ARGUMENT)
    inp.connect_outputs(1, 2)  # the input through `* value`: a node
    inp.close()


def test_more_than_512_stages_are_refused_also_for_oscillators_and_arithmetic(knh):
    """An unconnected voice of this class runs a lane per frame (up to 4 096 stages); connected it is fused like any graph."""
    st = [SIN, SIN] + [Stage(L.STAGE_MATH_ADD, input=i + 1, input2=i + 2) for i in range(600)]
    b = knh.VoiceBank(st, 2, L.F32, 2)
    _refused(b, lambda: b.connect_outputs(0, len(st) - 1), L.ERR_UNSUPPORTED_CHAIN)
    b.connect_outputs(len(st) - 1, len(st) - 1)  # the default is no connection
    b.close()
    chain = knh.VoiceBank([SIN] + [MUL] * 520, 2, L.F32, 2)  # a plain chain of any length -- until it is connected
    _refused(chain, lambda: chain.connect_outputs(0, 520), L.ERR_UNSUPPORTED_CHAIN)
    chain.close()


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_signatures(knh, sample_type):
    plain = knh.VoiceBank(FOUR, 70, sample_type, 2)
    mono_sig = plain.debug_signature()
    assert mono_sig == "W@_,_,0m@0,_,0W@_,_,0m@0,_,0#1"  # (two sources: a graph; nobody reads the first) not a character moved
    chain = knh.VoiceBank([SIN, SVF, ASR], 70, sample_type, 2)
    assert chain.debug_signature() == "WSA"
    chain.connect_outputs(2, 2)
    assert chain.debug_signature() == "WSA"  # the default, restored or never left: the plain chain, its pre-built kernel
    chain.connect_outputs(0, 2)
    assert chain.debug_signature() == "W@_,_,0S@0,_,1A@1,_,1#2:0,1"  # the left signal survives the in-place filter
    chain.connect_outputs(2, 2)
    assert chain.debug_signature() == "WSA"
    chain.close()

    sigs = {}
    for lr in ((3, 3), (0, 2), (2, 0), (1, 3), (1, 1)):
        b = knh.VoiceBank(FOUR, 70, sample_type, 2)
        b.connect_outputs(*lr)
        twin = knh.VoiceBank(FOUR, 70, sample_type, 2)
        twin.connect_outputs(*lr)
        assert b.debug_signature() == twin.debug_signature()  # connected alike: one kernel, one cache entry
        sigs[lr] = b.debug_signature()
        assert knh.chain_ugen_count(FOUR) == 6  # an edge is not a node
        assert b.algorithmic_bytes_per_voice_block() == plain.algorithmic_bytes_per_voice_block()
        b.close()
        twin.close()
    assert sigs[(3, 3)] == mono_sig
    assert len(set(sigs.values())) == len(sigs)  # (0, 2), (2, 0), (1, 3), (1, 1) and mono: five kernels
    for lr, s in sigs.items():
        if lr != (3, 3):
            assert re.fullmatch(r".*#\d+:\d+,\d+", s) and s.split("#")[0] != "" and s != mono_sig
    plain.close()


def test_held_slots_are_never_overwritten(knh):
    """Both connected signals keep their slot to the end: no later stage writes it (graph_voices.overwritten_live_signals'
    rule with the two outputs as readers behind the last stage)."""
    for name in sc.CASES:
        case = sc.CASES[name](3)
        b = knh.VoiceBank(case.stages, 3, L.F32, 2)
        b.connect_outputs(*case.connect)
        sig = b.debug_signature()
        l, r = b.output_stage(0), b.output_stage(1)
        b.close()
        body, _, tail = sig.partition("#")
        count, _, outs = tail.partition(":")
        written = [int(m.group(1)) for m in re.finditer(r"@(?:_|\d+),(?:_|\d+),(\d+)", body)]
        assert len(written) == len(case.stages), sig
        sl, sr = (int(x) for x in outs.split(","))
        assert (written[l], written[r]) == (sl, sr) and max(written) < int(count), sig
        for out in {l, r}:
            assert all(w != written[out] for w in written[out + 1:]), f"{name}: {sig}: slot of stage {out} is written again"


@pytest.fixture(scope="module")
def jit_compile_check(knh):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/jit_compile_check"], check=True, capture_output=True)
    assert os.path.exists(CHECK)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_connected_voices_compile_for_gfx950(knh, jit_compile_check, name, f64):
    case = sc.CASES[name](3)
    b = knh.VoiceBank(case.stages, 3, L.F64 if f64 else L.F32, 2)
    b.connect_outputs(*case.connect)
    signature = b.debug_signature()
    b.close()
    assert ":" in signature
    p = subprocess.run([CHECK, signature] + (["f64"] if f64 else []), cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, f"{signature}: rc {p.returncode}: {p.stdout.decode(errors='replace')[-800:]}"
