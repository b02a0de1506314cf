"""BufferReader<F, U2> at the C-ABI boundary, on a machine without a GPU: interleaved two-channel Buffers in the pool
(knh_bank_add_buffer_interleaved) and the stage that stands for the reader's second output (KNH_STAGE_FLAG_READER_CH1).
The header, the Rust bindings and ctypes agree; every kind of bank accepts a reader + CH1 voice; every refusal returns its
status with a text and changes nothing; the second output is no node (no UGen counted, no parameters); mono reader chains
keep their signatures to the character; the slot plan never overwrites a live signal; and the fused kernels the GPU tests
run compile for gfx950 (the compile is host work: tests/test_jit_compile.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import graph_voices as gv
import stereo_reader_ref as sr
from knaster_amd import _lib as L
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "bin", "jit_compile_check")

R, M = sr.READER, Stage(L.STAGE_MUL_CONST)
CH1 = L.STAGE_FLAG_READER_CH1
LFO = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST)]
LINKED = LFO + [Stage(L.STAGE_BUFFER_READER, ar_param=1, input2=3), sr.ch1(3)]

# the voices of tests/test_gpu_stereo_reader.py: name -> (stages, connected outputs or None)
VOICES = {
    "player": (sr.STEREO, sr.STEREO_OUTS),
    "swapped": (sr.STEREO, (3, 2)),
    "raw": ([R, sr.ch1(0)], (0, 1)),
    "ch1_alone": ([R, sr.ch1(0)], None),
    "fold_down": ([R, sr.ch1(0), Stage(L.STAGE_MATH_ADD, input=1, input2=2)], None),
    "linked": (LINKED, (3, 4)),
    "smooth": ([Stage(L.STAGE_BUFFER_READER, flags=L.STAGE_FLAG_SMOOTH_PARAMS), sr.ch1(0)], (0, 1)),
}


def signature_of(knh, stages, outs, sample_type=L.F32):
    b = knh.VoiceBank(stages, 3, sample_type, 2)
    if outs is not None:
        b.connect_outputs(*outs)
    s = b.debug_signature()
    b.close()
    return s


def test_header_rust_and_ctypes_declare_the_entry_point_and_the_flag():
    header = open(os.path.join(ROOT, "include", "knaster_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "ffi.rs")).read()
    assert re.search(r"int32_t\s+knh_bank_add_buffer_interleaved\(knh_bank\* bank, uint32_t stage, const void\* samples, size_t n_frames,\s*"
                     r"uint32_t n_channels, double buffer_sample_rate, uint32_t\* out_index\);", header)
    assert re.search(r"pub fn knh_bank_add_buffer_interleaved\(bank: \*mut knh_bank, stage: u32, samples: \*const c_void, n_frames: usize, "
                     r"n_channels: u32, buffer_sample_rate: f64, out_index: \*mut u32\) -> i32;", ffi)
    assert L.PROTOTYPES["knh_bank_add_buffer_interleaved"] == (
        C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_double, C.POINTER(C.c_uint32)])
    assert hasattr(C.CDLL(L.LIB_PATH), "knh_bank_add_buffer_interleaved")
    assert re.search(r"\bKNH_STAGE_FLAG_READER_CH1 = 1u << 2\b", header)
    assert re.search(r"pub const KNH_STAGE_FLAG_READER_CH1: u16 = 1 << 2;", ffi)
    assert L.STAGE_FLAG_READER_CH1 == 1 << 2
    # a new entry point and a new flag, not a new ABI and not a new stage kind
    assert re.search(r"#define KNH_ABI_VERSION 4\b", header) and L.KNH_ABI_VERSION == 4
    assert re.search(r"\bKNH_STAGE_KIND_COUNT = 46\b", header) and re.search(r"pub const KNH_STAGE_KIND_COUNT: u16 = 46;", ffi)
    assert re.search(r"\bKNH_STAGE_BUFFER_READER = 27,", header) and L.STAGE_BUFFER_READER == 27


@pytest.mark.parametrize("kw", [{}, {"host_threads": 2}, {"devices": [0]}, {"rank": 0, "world": 1}])
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_a_reader_with_a_second_output_is_accepted_by_every_kind_of_bank(knh, kw, sample_type):
    n = 200
    buffers = sr.make_stereo_buffers()
    b = sr.stereo_bank(knh, n, 64, sample_type, buffers, sr.spread_ids(n), sr.stereo_ctor(n), init=False, **kw)
    assert b.buffer_count(0) == 3 and b.buffer_count(1) == 0  # the second output has no pool of its own
    assert (b.output_stage(0), b.output_stage(1)) == sr.STEREO_OUTS
    assert b.stage_parameters(0) == 6 and b.stage_parameters(1) == 0 and b.stage_param_descriptions(1) == []
    b.close()


def test_the_second_output_is_no_node(knh):
    two_mul = [R, Stage(L.STAGE_MUL_CONST, input=1), Stage(L.STAGE_MUL_CONST, input=1)]
    assert knh.chain_ugen_count(sr.STEREO) == knh.chain_ugen_count(two_mul) == 5  # BufferReader + 2 x (Constant + MathUGen)
    assert knh.chain_ugen_count([R, sr.ch1(0)]) == knh.chain_ugen_count([R]) == 1
    a = knh.VoiceBank(sr.STEREO, 4, L.F32, 2)
    b = knh.VoiceBank(two_mul, 4, L.F32, 2)
    assert a.algorithmic_bytes_per_voice_block() == b.algorithmic_bytes_per_voice_block()  # no state of its own
    a.close()
    b.close()


def test_parameter_calls_that_name_the_second_output_are_refused_before_init_too(knh):
    for kw in ({}, {"host_threads": 2}, {"rank": 0, "world": 1}):
        b = knh.VoiceBank(sr.STEREO, 130, L.F32, 2, **kw)
        v = np.arange(4, dtype=np.uint32)
        for call in (lambda: b.param_apply(0, 1, 0, 1.0), lambda: b.set_delay_within_block_for_param(0, 1, 0, 3),
                     lambda: b.param_apply_range(0, 4, 1, 0, L.VALUE_FLOAT, 1.0),
                     lambda: b.param_apply_many(v, 1, 0, L.VALUE_FLOAT, [1.0] * 4),
                     lambda: b.param_apply_many(v, 1, 5, L.VALUE_TRIGGER)):
            with pytest.raises(L.KnasterHipError) as e:
                call()
            assert e.value.status == L.ERR_INVALID_ARGUMENT and "no parameters" in str(e.value), (kw, str(e.value))
        with pytest.raises(L.KnasterHipError) as e:  # ... while the reader stage answers as any node does before init
            b.param_apply(0, 0, 0, 1.0)
        assert e.value.status == L.ERR_NOT_INITIALISED
        with pytest.raises(L.KnasterHipError) as e:
            b.set_ctor_args(1, np.zeros((130, 3)))  # no constructor arguments either
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        b.close()


@pytest.mark.parametrize("what,bad,status", [
    ("flag on another kind", [R, Stage(L.STAGE_MUL_CONST, flags=CH1, input=1)], L.ERR_INVALID_ARGUMENT),
    ("no reader named", [R, Stage(L.STAGE_BUFFER_READER, flags=CH1)], L.ERR_INVALID_ARGUMENT),
    ("names a stage that is no reader", [R, M, Stage(L.STAGE_BUFFER_READER, flags=CH1, input=2)], L.ERR_INVALID_ARGUMENT),
    ("names a later stage", [R, Stage(L.STAGE_BUFFER_READER, flags=CH1, input=3), R], L.ERR_INVALID_ARGUMENT),
    ("names a second output", [R, sr.ch1(0), Stage(L.STAGE_BUFFER_READER, flags=CH1, input=2)], L.ERR_INVALID_ARGUMENT),
    ("two for one reader", [R, sr.ch1(0), sr.ch1(0)], L.ERR_INVALID_ARGUMENT),
    ("ar_param on it", LFO + [R, Stage(L.STAGE_BUFFER_READER, flags=CH1, input=4, ar_param=1, input2=3)], L.ERR_INVALID_ARGUMENT),
    ("input2 on it", [R, Stage(L.STAGE_BUFFER_READER, flags=CH1, input=1, input2=1)], L.ERR_INVALID_ARGUMENT),
    ("WrPreciseTiming on it", [R, Stage(L.STAGE_BUFFER_READER, flags=CH1, input=1, delayed_changes_per_block=2)], L.ERR_INVALID_ARGUMENT),
    ("WrSmoothParams on it", [R, Stage(L.STAGE_BUFFER_READER, flags=CH1 | L.STAGE_FLAG_SMOOTH_PARAMS, input=1)], L.ERR_INVALID_ARGUMENT),
    ("first stage", [Stage(L.STAGE_BUFFER_READER, flags=CH1)], L.ERR_INVALID_ARGUMENT),
    ("a wrapper on the reader", [R, Stage(L.STAGE_WR_MUL), sr.ch1(0)], L.ERR_UNSUPPORTED_CHAIN),
    ("a wrapper behind the second output", [R, sr.ch1(0), Stage(L.STAGE_WR_ADD)], L.ERR_UNSUPPORTED_CHAIN),
    ("two wrappers on the reader", [R, Stage(L.STAGE_WR_MUL), Stage(L.STAGE_WR_ADD), sr.ch1(0)], L.ERR_UNSUPPORTED_CHAIN),
])
def test_malformed_chains_are_refused_with_a_text(knh, what, bad, status):
    with pytest.raises(L.KnasterHipError) as e:
        knh.VoiceBank(bad, 4, L.F32, 2)
    assert e.value.status == status, f"{what}: {e.value}"
    message = str(e.value).split(":", 1)[1].strip()
    assert message and "unknown stage" not in message, what
    # the same wrapper on a reader WITHOUT a second output stays what it was
    knh.VoiceBank([R, Stage(L.STAGE_WR_MUL)], 4, L.F32, 2).close()


def _state(b):
    return (b.debug_signature(), b.buffer_count(0), b.output_stage(0), b.output_stage(1))


def _refused(b, call, status):
    before = _state(b)
    with pytest.raises(L.KnasterHipError) as e:
        call()
    assert e.value.status == status, str(e.value)
    assert str(e.value).split(":", 1)[1].strip()  # a knh_last_error text
    assert _state(b) == before


@pytest.mark.parametrize("kw", [{}, {"host_threads": 2}, {"rank": 0, "world": 1}])
def test_the_channel_count_is_the_pools(knh, kw):
    """The first entry fixes it; an entry with another count is refused and changes nothing."""
    lib = L.load()
    (stereo, rate), = sr.make_stereo_buffers([(37, 44100.0)])
    mono = np.ascontiguousarray(stereo[:, 0])
    assert lib.knh_bank_add_buffer_interleaved(None, 0, None, 1, 2, 44100.0, None) == L.ERR_INVALID_ARGUMENT

    b = knh.VoiceBank(sr.STEREO, 130, L.F32, 2, **kw)
    b.connect_outputs(*sr.STEREO_OUTS)
    for ch in (0, 3, 4):  # one or two channels
        _refused(b, lambda: b.add_buffer(0, stereo, rate, channels=ch), L.ERR_INVALID_ARGUMENT)
    _refused(b, lambda: b.add_buffer(1, stereo, rate, channels=2), L.ERR_INVALID_ARGUMENT)  # the second output is no reader
    _refused(b, lambda: b.add_buffer(2, stereo, rate, channels=2), L.ERR_INVALID_ARGUMENT)
    _refused(b, lambda: b.assign_buffers(1, [0], [0]), L.ERR_INVALID_ARGUMENT)
    assert b.add_buffer(0, stereo, rate, channels=2) == 0
    assert b.add_buffer(0, stereo[:20], 48000.0, channels=2) == 1
    _refused(b, lambda: b.add_buffer(0, mono, rate), L.ERR_INVALID_ARGUMENT)               # knh_bank_add_buffer: one channel
    _refused(b, lambda: b.add_buffer(0, mono, rate, channels=1), L.ERR_INVALID_ARGUMENT)
    _refused(b, lambda: b.set_buffer(0, mono, rate), L.ERR_INVALID_ARGUMENT)               # knh_bank_set_buffer: one channel
    _refused(b, lambda: b.add_buffer(0, stereo[:0], rate, channels=2), L.ERR_INVALID_ARGUMENT)  # empty
    _refused(b, lambda: b.add_buffer(0, stereo, 0.0, channels=2), L.ERR_INVALID_ARGUMENT)
    before = _state(b)
    with pytest.raises(ValueError):  # an odd number of samples is not whole stereo frames: refused, not cut short
        b.add_buffer(0, stereo.reshape(-1)[:21], rate, channels=2)
    assert _state(b) == before
    _refused(b, lambda: b.assign_buffers(0, [0], [2]), L.ERR_OUT_OF_RANGE)
    assert b.buffer_count(0) == 2
    b.close()

    m = knh.VoiceBank([R, M], 130, L.F32, 2, **kw)  # ... and a pool that began with one channel stays a one-channel pool
    assert m.add_buffer(0, mono, rate, channels=1) == 0  # n_channels = 1 is knh_bank_add_buffer
    assert m.add_buffer(0, mono, rate) == 1
    _refused(m, lambda: m.add_buffer(0, stereo, rate, channels=2), L.ERR_INVALID_ARGUMENT)
    m.set_buffer(0, mono[:10], rate)  # entry 0 replaced, as before
    assert m.buffer_count(0) == 2
    m.close()


def test_mono_reader_signatures_are_what_they_were(knh):
    """The literals are those of the parent commit: a chain, a linked rate, two readers summed, two readers connected."""
    assert signature_of(knh, [R, M], None) == "Fm"
    assert signature_of(knh, [R, M], None, L.F64) == "Fm"
    assert signature_of(knh, [R], None) == "F"
    assert signature_of(knh, LFO + [Stage(L.STAGE_BUFFER_READER, ar_param=1, input2=3), M], None) == "W@_,_,0m@0,_,0a@0,_,0F%0@_,0,0m@0,_,0#1"
    assert signature_of(knh, [R, R, Stage(L.STAGE_MATH_ADD, input=1, input2=2), Stage(L.STAGE_MUL_ENV_ASR)], None) == "F@_,_,0F@_,_,1+@0,1,0A@0,_,0#2"
    assert signature_of(knh, [R, M, R, M], (1, 3)) == "F@_,_,0m@0,_,0F@_,_,1m@1,_,1#2:0,1"
    # ... and the stereo reader's own: one device stage with two output slots, the second output not a stage
    assert signature_of(knh, *VOICES["player"]) == "T@_,_,0,1m@0,_,0m@1,_,1#2:0,1"
    assert signature_of(knh, *VOICES["ch1_alone"]) == "T@_,_,0,1#2=1"
    assert signature_of(knh, *VOICES["linked"]) == "W@_,_,0m@0,_,0a@0,_,0T%0@_,0,0,1#2:0,1"


def written_slots(stages, signature):
    """The slot every descriptor stage writes, from the signature: a reader with a second output names two, and its
    second-output stage (which is no device stage) writes the second of them -- at the reader's position in time."""
    body = signature.partition("#")[0]
    nodes = re.findall(r"@(?:_|\d+),(?:_|\d+),(\d+)(?:,(\d+))?", body)
    written, second = [None] * len(stages), {}
    it = iter(nodes)
    for i, s in enumerate(stages):
        if s.kind == L.STAGE_BUFFER_READER and s.flags & CH1:
            written[i] = second[s.input - 1]
            continue
        o, o2 = next(it)
        written[i] = int(o)
        if o2:
            second[i] = int(o2)
    assert next(it, None) is None, signature
    return written


def _graphs():
    rng = np.random.default_rng(3)
    yield "player", sr.STEREO, sr.STEREO_OUTS
    yield "linked", LINKED, (3, 4)
    yield "both read late", [R, sr.ch1(0), Stage(L.STAGE_SIN_WT), M, Stage(L.STAGE_MATH_MUL, input=4, input2=1), Stage(L.STAGE_MATH_ADD, input=5, input2=2)], None
    yield "ch0 unread", [R, sr.ch1(0), Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MATH_ADD, input=3, input2=2)], None
    yield "ch1 last", [Stage(L.STAGE_SIN_WT), R, Stage(L.STAGE_MATH_ADD, input=1, input2=2), sr.ch1(1)], None
    yield "two stereo readers", [R, sr.ch1(0), R, sr.ch1(2), Stage(L.STAGE_MATH_ADD, input=1, input2=3), Stage(L.STAGE_MATH_ADD, input=2, input2=4)], (4, 5)
    for k in range(12):  # random feed-forward graphs around a stereo reader
        st = [R, sr.ch1(0)]
        for _ in range(int(rng.integers(2, 9))):
            m = len(st)
            kind = int(rng.integers(0, 3))
            if kind == 0:
                st.append(Stage(L.STAGE_SIN_WT))
            elif kind == 1:
                st.append(Stage(L.STAGE_MUL_CONST, input=int(rng.integers(1, m + 1))))
            else:
                st.append(Stage(L.STAGE_MATH_ADD, input=int(rng.integers(1, m + 1)), input2=int(rng.integers(1, m + 1))))
        outs = (int(rng.integers(0, len(st))), int(rng.integers(0, len(st)))) if k % 2 else None
        yield f"random {k}", st, outs


def test_the_slot_plan_never_overwrites_a_live_signal(knh):
    """graph_voices.overwritten_live_signals' rule: no stage writes a slot whose signal still has a reader; both outputs of a
    stereo reader are held until their last reader, connected outputs to the end; the two outputs are two slots."""
    for name, st, outs in _graphs():
        b = knh.VoiceBank(st, 3, L.F32, 2)
        if outs is not None:
            b.connect_outputs(*outs)
        sig = b.debug_signature()
        held = {b.output_stage(0), b.output_stage(1)} if outs is not None else {len(st) - 1}
        b.close()
        written = written_slots(st, sig)
        count = int(re.match(r"\d+", sig.partition("#")[2]).group(0))
        assert max(written) < count, (name, sig)
        # the second output is written WHEN THE READER RUNS: for the liveness rule it sits at the reader's place in the list
        order = sorted(range(len(st)), key=lambda i: (st[i].input - 1 + 0.5) if st[i].flags & CH1 and st[i].kind == L.STAGE_BUFFER_READER else i)
        place = {stage: k for k, stage in enumerate(order)}
        rd = gv.readers(st)
        holder = {}
        for i in order:
            k = holder.get(written[i])
            if k is not None:
                last = max([place[r] for r in rd[k]] + ([len(st)] if k in held else []), default=-1)
                assert last <= place[i], f"{name}: {sig}: stage {i} writes slot {written[i]} while stage {k}'s signal is still read"
            holder[written[i]] = i
        for i, s in enumerate(st):
            if s.kind == L.STAGE_BUFFER_READER and s.flags & CH1:
                assert written[i] != written[s.input - 1], (name, sig)
        tail = sig.partition("#")[2]
        if outs is not None and ":" in tail:
            l, r = (int(x) for x in tail.partition(":")[2].split(","))
            o0, o1 = sorted(held) if len(held) == 2 else (list(held)[0], list(held)[0])
            assert {l, r} == {written[o0], written[o1]}, (name, sig)
        if outs is None and st[-1].flags & CH1:
            assert tail.endswith("=" + str(written[-1])), (name, sig)


@pytest.fixture(scope="module")
def jit_compile_check(knh):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/jit_compile_check"], check=True, capture_output=True)
    assert os.path.exists(CHECK)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("name", sorted(VOICES) + ["mono_on_stereo_pool", "mono_linked_on_stereo_pool"])
def test_the_fused_kernels_of_the_gpu_cases_compile_for_gfx950(knh, jit_compile_check, name, f64):
    if name == "mono_on_stereo_pool":      # what knh_bank_init turns "Fm" into on a pool of two-channel Buffers
        signature, args = "Cm", ["pipe"]
    elif name == "mono_linked_on_stereo_pool":
        signature, args = "W@_,_,0m@0,_,0a@0,_,0C%0@_,0,0m@0,_,0#1", []
    else:
        signature, args = signature_of(knh, *VOICES[name], L.F64 if f64 else L.F32), []
        assert "T" in signature
    p = subprocess.run([CHECK, signature] + args + (["f64"] if f64 else []), cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, f"{signature}: rc {p.returncode}: {p.stdout.decode(errors='replace')[-800:]}"
