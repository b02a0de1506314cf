"""Which kernel form a bank takes (knaster_amd/csrc/kernel_form.hpp), asked through the real kernel registry: each row
creates and initialises a bank, renders one block of 64 frames and reads the form back from debug word 2 (and, in the
lane-per-frame forms, the voices per workgroup from word 3).  The voice counts are the group thresholds of DESIGN.md
section 4: 1, 2, 256, 257, 512, 513, 1 024 and 1 025 groups of 64 voices.  The expected forms are written out by hand;
the decision table itself, variants included, is tests/cpp/kernel_form_test.cpp (CPU)."""
import numpy as np
import pytest

import frame_bank_cases as fc
import graph_voices as gv
import sampler_pool as sp
from helpers import make_gpu
from knaster_amd import _lib as L
from knaster_amd import configs

pytestmark = pytest.mark.gpu

BS = 64
SWITCHES = ("KNH_JIT", "KNH_PIPELINE", "KNH_PIPE_BIG", "KNH_PAIR", "KNH_WIDE", "KNH_INTERP", "KNH_FRAME_JIT", "KNH_JIT_PIPE", "KNH_JIT_WAVES",
            "KNH_HOST_THREADS")
PIPE, MANY, ONE = L.DEBUG_FORM_PIPELINE, L.DEBUG_FORM_MANY_WAVE, L.DEBUG_FORM_WHOLE_CHAIN
PIPE_FUSED, ONE_FUSED = L.DEBUG_FORM_PIPELINE_FUSED, L.DEBUG_FORM_WHOLE_CHAIN_FUSED


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def words_after_a_block(g):
    g.process_block()
    w = g.debug_words()
    return int(w[2]), int(w[3])


# ---- pre-built chains at the group thresholds -------------------------------------------------------------------------------
# (the pair of 257-512 groups in f32 is a pipeline too: word 2 does not tell the variants apart)
C3_F32 = {64: PIPE, 128: PIPE, 16384: PIPE, 16448: PIPE, 32768: PIPE, 32832: MANY, 65536: MANY, 65600: MANY}
C3_F64 = {64: PIPE, 128: PIPE, 16384: PIPE, 16448: MANY, 32768: MANY, 32832: MANY, 65536: MANY, 65600: MANY}
PREBUILT = [("C3", L.F32, n, f) for n, f in C3_F32.items()] + [("C3", L.F64, n, f) for n, f in C3_F64.items()] + \
           [("D3", L.F32, 16384, PIPE), ("D3", L.F32, 16448, MANY)]


@pytest.mark.parametrize("name,sample_type,n,want", PREBUILT, ids=[f"{c[0]}-{'f64' if c[1] == L.F64 else 'f32'}-{c[2]}" for c in PREBUILT])
def test_prebuilt_chain_at_the_group_thresholds(knh, monkeypatch, name, sample_type, n, want):
    set_env(monkeypatch, {})
    g = make_gpu(knh, configs.config(name, n_voices=n, block_size=BS, sample_type=sample_type))
    assert words_after_a_block(g) == (want, 0)
    g.close()


# ---- the switches, 130 voices of C3 ------------------------------------------------------------------------------------------
SWITCH_ROWS = [({"KNH_PIPELINE": "0"}, ONE), ({"KNH_WIDE": "4"}, MANY), ({"KNH_JIT": "1"}, PIPE_FUSED),
               ({"KNH_JIT": "1", "KNH_JIT_PIPE": "0"}, ONE_FUSED)]


@pytest.mark.parametrize("env,want", SWITCH_ROWS, ids=["-".join(f"{k[4:]}={v}" for k, v in r[0].items()) for r in SWITCH_ROWS])
def test_switches(knh, monkeypatch, env, want):
    set_env(monkeypatch, env)
    g = make_gpu(knh, configs.config("C3", n_voices=130, block_size=BS))
    assert words_after_a_block(g) == (want, 0)
    g.close()


# ---- voices without a pre-built kernel --------------------------------------------------------------------------------------
def test_one_graph_voice(knh, monkeypatch):
    """a graph with a delay and an envelope: the fused one-wavefront kernel"""
    set_env(monkeypatch, {})
    g = gv.gpu_bank(knh, gv.directed_voice("comb_asr_pan", 1, L.F32, BS))
    assert words_after_a_block(g) == (ONE_FUSED, 0)
    g.close()


OSC_ROWS = [({}, L.DEBUG_FORM_FRAME_JIT, 1), ({"KNH_FRAME_JIT": "0"}, L.DEBUG_FORM_FRAME_INTERP, 1), ({"KNH_INTERP": "0"}, ONE_FUSED, 0)]


@pytest.mark.parametrize("env,want,vpw", OSC_ROWS, ids=["default", "FRAME_JIT=0", "INTERP=0"])
def test_one_voice_of_oscillators_and_arithmetic(knh, monkeypatch, env, want, vpw):
    """a lane per frame, one voice per workgroup (1 // 256 voices, at least one); KNH_INTERP=0: a lane per voice, fused"""
    set_env(monkeypatch, env)
    g = make_gpu(knh, fc.cascade(4, 1, BS, L.F32))
    assert words_after_a_block(g) == (want, vpw)
    g.close()


# ---- the order of the calls before init ---------------------------------------------------------------------------------------
def test_outputs_connected_and_restored_before_init(knh, monkeypatch):
    """knh_bank_connect_outputs changes the voice's signature; naming the last stage twice restores it, and the bank takes
    the form of one whose outputs were never connected."""
    set_env(monkeypatch, {})
    w = configs.config("C3", n_voices=130, block_size=BS)
    plain = make_gpu(knh, w)
    want, sig = words_after_a_block(plain), plain.debug_signature()
    plain.close()
    assert want == (PIPE, 0)
    g = knh.VoiceBank(w.stages, w.n_voices, w.sample_type, 2)
    for s, a in w.ctor.items():
        g.set_ctor_args(s, a)
    g.connect_outputs(1, 3)
    assert g.debug_signature() != sig
    last = len(w.stages) - 1
    g.connect_outputs(last, last)
    g.init(configs.SAMPLE_RATE, BS)
    assert g.debug_signature() == sig
    assert words_after_a_block(g) == want
    g.close()


def test_refused_init_of_a_two_channel_pool_changes_nothing(knh, monkeypatch):
    """A mono reader on a pool of two-channel Buffers is a stage of its own ('C' for 'F'), decided at init.  An init that is
    refused leaves the bank as it was: the next one gives the signature and the form of a bank initialised once."""
    set_env(monkeypatch, {})
    n = 130
    rng = np.random.default_rng(5)
    frames = rng.uniform(-1.0, 1.0, (700, 2))

    def bank():
        b = knh.VoiceBank(sp.STAGES, n, L.F32, 2)
        b.set_ctor_args(0, sp.sampler_ctor(n))
        b.set_ctor_args(1, np.full((n, 1), 1.0 / n))
        assert b.add_buffer(0, frames, 44100.0, channels=2) == 0
        return b
    once = bank()
    before = once.debug_signature()
    once.init(configs.SAMPLE_RATE, BS)
    want, sig = words_after_a_block(once), once.debug_signature()
    once.close()
    assert "F" in before and "F" not in sig and "C" in sig
    assert want == (PIPE_FUSED, 0)  # (three voice groups, nothing pre-built: a fused pipeline)
    g = bank()
    with pytest.raises(L.KnasterHipError):
        g.init(configs.SAMPLE_RATE, 0)
    with pytest.raises(L.KnasterHipError):
        g.init(configs.SAMPLE_RATE, 65536)
    assert g.debug_signature() == before
    g.init(configs.SAMPLE_RATE, BS)
    assert g.debug_signature() == sig
    assert words_after_a_block(g) == want
    g.close()
