"""knh_bank_set_voice_ctor_args / knh_bank_restart_voices at the C ABI on a machine without a GPU (knh_bank_create needs no
device): both refuse before init, in every form of bank; a Galactic chain is accepted by knh_bank_create (its refusal comes
at the call, tests/test_gpu_restart.py); header, exports, ctypes prototypes and the Rust declarations agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from knaster_amd import _lib as L
from knaster_amd import configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"knh_bank_set_voice_ctor_args": 6, "knh_bank_restart_voices": 3}


def status_of(fn, *a, **kw):
    with pytest.raises(L.KnasterHipError) as e:
        fn(*a, **kw)
    assert str(e.value)  # knh_last_error says why
    return e.value.status


def _no_reduce(_user, buf, count, sample_type, root, stream):
    return 0


@pytest.mark.parametrize("kw", [{}, {"host_threads": 2}, {"rank": 1, "world": 2, "reduce_fn": _no_reduce}, {"rank": 3, "world": 256, "reduce_fn": _no_reduce}],
                         ids=["one_range", "host_sharded", "rank_1_of_2", "rank_without_voices"])
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_both_calls_refuse_before_init(knh, sample_type, kw):
    w = configs.config("C3", n_voices=130, block_size=64, sample_type=sample_type)
    b = knh.VoiceBank(w.stages, 130, sample_type, 2, L.MIX_TREE, -1, False, **kw)
    assert status_of(b.restart_voices, [0, 64]) == L.ERR_NOT_INITIALISED
    assert status_of(b.restart_voices, []) == L.ERR_NOT_INITIALISED
    assert status_of(b.set_voice_ctor_args, 0, [0, 64], np.array([[440.0], [441.0]])) == L.ERR_NOT_INITIALISED
    assert status_of(b.set_voice_ctor_args, 9, [500], np.zeros((1, 3))) == L.ERR_NOT_INITIALISED  # (before anything else is looked at)
    b.set_ctor_args(0, w.ctor[0])  # knh_bank_set_ctor_args is what it was: before init, by voice range
    b.close()


def test_null_handle(knh):
    lib = L.load()
    assert lib.knh_bank_restart_voices(None, 0, None) == L.ERR_INVALID_ARGUMENT
    assert lib.knh_bank_set_voice_ctor_args(None, 0, 0, None, None, 0) == L.ERR_INVALID_ARGUMENT


def test_a_galactic_chain_is_accepted_at_create(knh):
    w = configs.config("G1", n_voices=4, block_size=64)
    b = knh.VoiceBank(w.stages, 4, L.F32, 2)
    for s, a in w.ctor.items():
        b.set_ctor_args(s, a)
    assert status_of(b.restart_voices, [0]) == L.ERR_NOT_INITIALISED
    b.close()


def test_header_exports_prototypes_and_rust_agree(knh):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "knaster_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "ffi.rs")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "lib.rs")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, n_args in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m and m.group(1).count(",") + 1 == n_args, name
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = L.PROTOTYPES[name]
        assert restype is C.c_int32 and len(argtypes) == n_args
        r = re.search(r"pub fn %s\(([^)]*)\) -> i32;" % name, rust)
        assert r and r.group(1).count(":") == n_args, name
        assert name + "(self.h" in shim, f"GpuVoiceBank does not call {name}"
    assert "pub fn restart_voices(&mut self, voices: &[u32])" in shim
    # nothing else moved: the version and the number of stage kinds are what tests/test_math1_abi.py pins
    assert L.KNH_ABI_VERSION == 4 and int(re.search(r"#define KNH_ABI_VERSION (\d+)", text).group(1)) == 4
