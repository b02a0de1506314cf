"""OscWt on a pool of Wavetables (KNH_STAGE_FLAG_WAVETABLE on KNH_STAGE_SIN_WT, knh_bank_add_wavetable /
knh_bank_wavetable_count / knh_bank_assign_wavetables; osc.rs:28-87, wavetable.rs:327-610) at the C-ABI boundary, on a
machine without a GPU: header, ctypes layer and Rust bindings agree, no kind was added and the ABI version stands, a flagged
stage is one node with SinWt's three parameters, every refusal the header lists returns its status and leaves the pool as
it was, and flagged voices compile for gfx950 (the compile is host work: tests/test_jit_compile.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import wavetable_ref as wr
from knaster_amd import _lib as L
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "bin", "jit_compile_check")
WT = L.STAGE_FLAG_WAVETABLE


def osc(flags=WT, **kw):
    return Stage(L.STAGE_SIN_WT, flags=flags, **kw)


def test_flag_and_entry_points_agree_between_header_ctypes_and_rust():
    header = open(os.path.join(ROOT, "include", "knaster_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "ffi.rs")).read()
    assert re.search(r"\bKNH_STAGE_FLAG_WAVETABLE = 1u << 3\b", header)
    assert re.search(r"pub const KNH_STAGE_FLAG_WAVETABLE: u16 = 1 << 3;", ffi)
    assert L.STAGE_FLAG_WAVETABLE == 1 << 3
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    h, r = squeeze(header), squeeze(ffi)
    assert "int32_t knh_bank_add_wavetable(knh_bank* bank, uint32_t stage, const void* samples, uint32_t n_tables, uint32_t* out_index);" in h
    assert "uint32_t knh_bank_wavetable_count(const knh_bank* bank, uint32_t stage);" in h
    assert ("int32_t knh_bank_assign_wavetables(knh_bank* bank, uint32_t stage, size_t count, const uint32_t* voices, "
            "const uint32_t* entries, const double* ctor);") in h
    assert "pub fn knh_bank_add_wavetable(bank: *mut knh_bank, stage: u32, samples: *const c_void, n_tables: u32, out_index: *mut u32) -> i32;" in r
    assert "pub fn knh_bank_wavetable_count(bank: *const knh_bank, stage: u32) -> u32;" in r
    assert "pub fn knh_bank_assign_wavetables(bank: *mut knh_bank, stage: u32, count: usize, voices: *const u32, entries: *const u32, ctor: *const f64) -> i32;" in r
    import ctypes as C
    assert L.PROTOTYPES["knh_bank_add_wavetable"] == (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)])
    assert L.PROTOTYPES["knh_bank_wavetable_count"] == (C.c_uint32, [C.c_void_p, C.c_uint32])
    assert L.PROTOTYPES["knh_bank_assign_wavetables"] == (C.c_int32, [C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p])
    # a flag and entry points only: no new kind, no version bump
    assert re.search(r"\bKNH_STAGE_KIND_COUNT = 46\b", header) and re.search(r"pub const KNH_STAGE_KIND_COUNT: u16 = 46;", ffi)
    assert re.search(r"#define KNH_ABI_VERSION 4\b", header) and L.KNH_ABI_VERSION == 4


def test_a_flagged_stage_is_one_node_with_sin_wts_parameters(knh):
    assert knh.chain_ugen_count([osc()]) == 1
    st = [osc(), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)]
    plain = [Stage(L.STAGE_SIN_WT)] + st[1:]
    assert knh.chain_ugen_count(st) == knh.chain_ugen_count(plain) == 1 + 0 + 1 + 2
    b, p = knh.VoiceBank(st, 5, L.F32, 1), knh.VoiceBank(plain, 5, L.F32, 1)
    assert b.stage_param_descriptions(0) == p.stage_param_descriptions(0) == ["freq", "phase_offset", "reset_phase"]
    assert b.debug_signature() == "MmSA" and p.debug_signature() == "WmSA"  # a stage of its own: never a pre-built kernel
    # the table in use and the pool entry: two more state words read per block (no table sample yet: block_size is init's)
    assert b.algorithmic_bytes_per_voice_block() == (p.algorithmic_bytes_per_voice_block()[0] + 8, p.algorithmic_bytes_per_voice_block()[1])
    b.set_ctor_args(0, np.full((5, 1), 220.0))  # one constructor argument, freq
    with pytest.raises(L.KnasterHipError) as e:
        b.set_ctor_args(0, np.zeros((5, 2)))
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    b.close()
    p.close()
    # with the running signal on "freq", with an audio-rate parameter, twice in one voice
    assert knh.VoiceBank([Stage(L.STAGE_SIN_WT), osc(WT | L.STAGE_FLAG_AR_FREQ)], 3, L.F32, 1).debug_signature() == "Wk"
    g = knh.VoiceBank([Stage(L.STAGE_SIN_WT), osc(ar_param=1, input2=1), osc(), Stage(L.STAGE_MATH_MUL, input=2, input2=3)], 3, L.F64, 1)
    assert "M%0@" in g.debug_signature() and g.debug_signature().count("M") == 2
    g.close()


def test_a_galactic_wrapped_bank_forwards_the_pool_calls(knh):
    """A chain that ends in Galactic is a bank around a bank: the pool calls reach the inner one, the reverb stage has none."""
    st = [osc(), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_MUL_ENV_AR), Stage(L.STAGE_GALACTIC)]
    b = knh.VoiceBank(st, 6, L.F32, 2)
    assert b.add_wavetable(0, wr.ramp_tables(np.float32)) == 0 and b.add_wavetable(0, wr.single_table(np.float32)) == 1
    b.assign_wavetables(0, [0, 5], [1, 1], ctor=[100.0, 200.0])
    assert b.wavetable_count(0) == 2 and b.wavetable_count(3) == 0
    for call, status in ((lambda: b.add_wavetable(3, wr.single_table(np.float32)), L.ERR_INVALID_ARGUMENT),
                         (lambda: b.assign_wavetables(3, [0], [0]), L.ERR_INVALID_ARGUMENT),
                         (lambda: b.assign_wavetables(0, [6], [0]), L.ERR_OUT_OF_RANGE)):
        with pytest.raises(L.KnasterHipError) as e:
            call()
        assert e.value.status == status
    b.close()


def test_the_flag_on_any_other_kind_is_refused(knh):
    for kind in (L.STAGE_SIN_NUMERIC, L.STAGE_PHASOR, L.STAGE_POLYBLEP, L.STAGE_BUFFER_READER, L.STAGE_MUL_CONST):
        with pytest.raises(L.KnasterHipError) as e:
            knh.VoiceBank([Stage(L.STAGE_SIN_WT), Stage(kind, flags=WT)], 4, L.F32, 1)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "WAVETABLE" in str(e.value)


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
@pytest.mark.parametrize("host_threads", [0, 2])
def test_refusals_leave_the_pool_as_it_was(knh, sample_type, host_threads):
    dtype = np.float64 if sample_type == L.F64 else np.float32
    b = knh.VoiceBank([osc(), Stage(L.STAGE_MUL_CONST), osc()], 130, sample_type, 1, host_threads=host_threads)
    assert b.wavetable_count(0) == b.wavetable_count(1) == b.wavetable_count(2) == b.wavetable_count(7) == 0
    assert b.add_wavetable(0, wr.ramp_tables(dtype)) == 0
    assert b.add_wavetable(0, wr.single_table(dtype)) == 1
    assert b.add_wavetable(2, wr.single_table(dtype)[0]) == 0  # every flagged stage has a pool of its own
    assert (b.wavetable_count(0), b.wavetable_count(2)) == (2, 1)

    def refused(call, status):
        with pytest.raises(L.KnasterHipError) as e:
            call()
        assert e.value.status == status, str(e.value)
        assert str(e.value).split(":", 1)[1].strip()
        assert (b.wavetable_count(0), b.wavetable_count(1), b.wavetable_count(2)) == (2, 0, 1)

    for n_tables in (0, 2, 16, 18):  # 17 or 1, nothing else
        t = np.zeros((max(n_tables, 1), wr.TABLE_SIZE), dtype=dtype)
        refused(lambda: b._check(b._lib.knh_bank_add_wavetable(b._h, 0, t.ctypes.data, n_tables, None)), L.ERR_INVALID_ARGUMENT)
    refused(lambda: b._check(b._lib.knh_bank_add_wavetable(b._h, 0, None, 17, None)), L.ERR_INVALID_ARGUMENT)  # a null pointer
    refused(lambda: b.add_wavetable(1, wr.single_table(dtype)), L.ERR_INVALID_ARGUMENT)   # a stage without the flag
    refused(lambda: b.add_wavetable(9, wr.single_table(dtype)), L.ERR_INVALID_ARGUMENT)   # no such stage
    refused(lambda: b.assign_wavetables(1, [0], [0]), L.ERR_INVALID_ARGUMENT)
    refused(lambda: b.assign_wavetables(0, [0, 1], [0, 2]), L.ERR_OUT_OF_RANGE)           # an entry that does not exist
    refused(lambda: b.assign_wavetables(2, [0], [1]), L.ERR_OUT_OF_RANGE)                 # (stage 0 has two, stage 2 one)
    refused(lambda: b.assign_wavetables(0, [130], [0]), L.ERR_OUT_OF_RANGE)               # a voice that does not exist
    refused(lambda: b._check(b._lib.knh_bank_assign_wavetables(b._h, 0, 1, None, None, None)), L.ERR_INVALID_ARGUMENT)
    b.assign_wavetables(0, [0, 64, 129], [1, 1, 0])               # before init: no constructor argument needed ...
    b.assign_wavetables(0, [3, 70], [1, 0], ctor=[110.0, 55.0])  # ... or with one
    b.close()
    # (a null handle has no pool)
    assert knh.lib.load().knh_bank_wavetable_count(None, 0) == 0


@pytest.fixture(scope="module")
def jit_compile_check(knh):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/jit_compile_check"], check=True, capture_output=True)
    assert os.path.exists(CHECK)


def _signature(knh, what):
    if what == "chain":
        st = [osc(), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)]
    elif what == "ar graph":  # a plain SinWt drives the flagged stage's freq at audio rate
        st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), osc(ar_param=1, input2=2), Stage(L.STAGE_MUL_ENV_ASR)]
    else:  # two flagged stages in one voice
        st = [osc(), osc(), Stage(L.STAGE_MATH_MUL, input=1, input2=2)]
    b = knh.VoiceBank(st, 3, L.F32, 1)
    sig = b.debug_signature()
    b.close()
    return sig


@pytest.mark.parametrize("what,args", [("chain", []), ("chain", ["pipe"]), ("chain", ["f64"]), ("chain", ["f64", "pipe"]), ("chain", ["fma"]),
                                       ("ar graph", []), ("ar graph", ["f64"]), ("two stages", []), ("two stages", ["f64", "fma"]),
                                       # a bank whose one f32 table is staged to LDS: 'g' for 'M', 'h' for 'k' (knh_bank_init decides)
                                       ("gmSA", []), ("gmSA", ["pipe"]), ("Imh", ["fma"])])
def test_flagged_voices_compile_for_gfx950(knh, jit_compile_check, what, args):
    signature = what if what in ("gmSA", "Imh") else _signature(knh, what)
    assert any(c in signature for c in "Mgh")
    p = subprocess.run([CHECK, signature] + args, cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, f"{signature} {args}: rc {p.returncode}: {p.stdout.decode(errors='replace')[-800:]}"


def test_host_table_index_agrees_with_the_restatement(knh):
    """wt_table_index of knaster_amd/csrc/stage_table.hpp (what the host writes into a voice's table word) over the threshold
    list, its f32 neighbours on both sides and the odd values: tests/cpp/wavetable_index_test.cpp prints, wavetable_ref counts."""
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "wavetable_index_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    # (stage_table.hpp has no HIP in it: CPU only, no library)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unused-variable",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "wavetable_index_test.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    th = wr.THRESHOLDS
    f = np.concatenate([th, np.nextafter(th, np.float32(np.inf)), np.nextafter(th, np.float32(-np.inf)),
                        np.array([0.0, -0.0, -440.0, 1e-30, 20000.0, 30000.0, np.inf, -np.inf, np.nan, 3.4e38], dtype=np.float32)]).astype(np.float32)
    res = subprocess.run([exe] + ["%08x" % b for b in f.view(np.uint32)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.array([int(x) for x in res.stdout.split()], dtype=np.uint32)
    want = wr.table_index(f)
    np.testing.assert_array_equal(got, want)
    assert list(want[:16]) == list(range(16)) and list(want[16:32]) == list(range(1, 17))  # on a threshold: below it
    assert want[32 + 16 + 2] == 0 and want[32 + 16 + 4] == 16 and want[32 + 16 + 8] == 16  # negative: 0; 20 000: 16; NaN: 16
