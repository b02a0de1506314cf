"""Graph voices built from every stage kind, without a GPU: the library accepts every committed seed of
tests/graph_voices.py and every directed voice, hands out the signal slots as the rule says (restated in Python), their
kernels compile for gfx950, the oracle renders them finite and audible, and the committed seeds cover what the generator
is there to cover.  tests/test_gpu_graph_voices.py runs the same voices on the device."""
import collections
import functools
import os
import subprocess

import numpy as np
import pytest

import graph_voices as gv
from knaster_amd import _lib as L
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "bin", "jit_compile_check")
SEEDS = list(range(gv.N_SEEDS))
VOICES = [f"seed{s}" for s in SEEDS] + gv.DIRECTED


@functools.lru_cache(maxsize=None)
def voice(name, sample_type=None):
    if name.startswith("seed"):
        return gv.random_graph_voice(int(name[4:]))
    return gv.directed_voice(name, 3, L.F32 if sample_type is None else sample_type)


def signature_of(knh, st):
    b = knh.VoiceBank(st, 3, L.F32, 2 if st[-1].kind == L.STAGE_PAN2 else 1, L.MIX_LEFT_FOLD)
    sig = b.debug_signature()
    b.close()
    return sig


@pytest.mark.parametrize("name", VOICES)
def test_voice_is_accepted_and_its_slots_follow_the_rule(knh, name):
    """knh_bank_create takes the voice as a graph ("@" operands, "#R" slots); the slots in its signature are the ones the
    rule gives -- first free slot, freed at the last reader, in place if the first operand dies here -- and no stage writes
    a slot whose signal still has a later reader."""
    w = voice(name)
    st = w.stages
    if name.startswith("seed"):
        assert 5 <= len(st) <= 14
        assert sum(gv.is_source(s) for s in st) >= 2
    sig = signature_of(knh, st)
    assert "@" in sig and "#" in sig, sig
    parsed, n_slots = gv.parse_signature(sig)
    assert len(parsed) == len(st), sig
    plan, want_slots = gv.slot_plan(st)
    assert [(a, b, o) for (_, _, a, b, o) in parsed] == plan, sig
    assert n_slots == want_slots
    assert [p for (_, p, _, _, _) in parsed] == [s.ar_param - 1 if s.ar_param else None for s in st]
    a, b = gv.operands(st)
    written = [o for (_, _, _, _, o) in parsed]
    for i, (_, _, sa, sb, _) in enumerate(parsed):  # every operand slot is the slot its signal was written to
        assert sa == (written[a[i]] if a[i] >= 0 else -1) and sb == (written[b[i]] if b[i] >= 0 else -1), (sig, i)
    assert gv.overwritten_live_signals(st, written) == [], sig


def test_the_slot_check_sees_a_signal_destroyed_before_its_last_reader():
    """The checker itself: a + b written over a while a later stage still reads a is reported; in place at the last reader
    is not."""
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_PHASOR), Stage(L.STAGE_MATH_ADD, input=1, input2=2), Stage(L.STAGE_MATH_MUL, input=3, input2=1)]
    assert gv.overwritten_live_signals(st, [0, 1, 0, 0]) == [(2, 0)]
    assert gv.overwritten_live_signals(st, [0, 1, 1, 0]) == []
    plan, n_slots = gv.slot_plan(st)
    assert [o for (_, _, o) in plan] == [0, 1, 1, 0] and n_slots == 2


def test_a_reader_of_a_wrapped_stage_gets_the_wrappers_output(knh):
    """wrapped_fanout: the Svf, the OnePoleHpf (which names the SinWt, stage 1) and, through them, the product all read the
    slot the last wrapper wrote -- the signature says so, not only the restatement."""
    st = voice("wrapped_fanout").stages
    parsed, _ = gv.parse_signature(signature_of(knh, st))
    wrapped = parsed[2][4]
    assert parsed[3][2] == wrapped and parsed[4][2] == wrapped
    assert gv.operands(st)[0][4] == 2 and len(gv.readers(st)[2]) == 2 and gv.readers(st)[0] == [1]


@pytest.fixture(scope="module")
def jit_compile_check(knh):
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/jit_compile_check"], check=True, capture_output=True)
    assert os.path.exists(CHECK)


@pytest.mark.parametrize("sample_type", ["f32", "f64"])
@pytest.mark.parametrize("name", gv.DIRECTED + [f"seed{s}" for s in range(4)])
def test_kernel_compiles_for_gfx950(knh, jit_compile_check, name, sample_type):
    """The fused kernel of the voice, built by hiprtc in a process of its own (tests/test_jit_compile.py)."""
    sig = signature_of(knh, voice(name).stages)
    p = subprocess.run([CHECK, sig] + (["f64"] if sample_type == "f64" else []), cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=900)
    assert p.returncode == 0, f"{name} {sig} ({sample_type}): rc {p.returncode}: {p.stdout.decode(errors='replace')[-600:]}"


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_renders_the_seed_finite_and_audible(oracle, seed):
    w = voice(f"seed{seed}")
    voices, mixes, _, _ = gv.oracle_run(oracle, w, 6)
    for b in range(6):
        assert np.isfinite(voices[b]).all() and np.isfinite(mixes[b]).all(), f"seed {seed} block {b}"
    peak = np.abs(voices).max(axis=(0, -1))  # per voice (per plane under Pan2), over the blocks
    assert (peak > 1e-4).all(), f"seed {seed}: silent voices {np.argwhere(peak <= 1e-4)[:5].tolist()}"


@pytest.mark.parametrize("name", gv.DIRECTED)
def test_oracle_renders_the_directed_voice_finite_and_audible(oracle, name):
    w = gv.directed_voice(name, 65, L.F32)
    voices, _, _, _ = gv.oracle_run(oracle, w, 12)
    assert np.isfinite(voices).all()
    assert (np.abs(voices).max(axis=(0, -1)) > 1e-4).all()


def coverage(voices):
    """What a list of voices holds -> Counter of items, each counted once per voice."""
    c = collections.Counter()
    for w in voices:
        st = w.stages
        a, _ = gv.operands(st)
        rd = gv.readers(st)
        have = set()
        for i, s in enumerate(st):
            have.add(("kind", s.kind))
            if s.kind in gv.DELAYS and s.input and a[i] != i - 1:
                have.add("delay reads a named signal that is not adjacent")
            if gv.is_wrapper(s) and not (i + 1 < len(st) and gv.is_wrapper(st[i + 1])) and len(rd[i]) >= 2:
                have.add("wrapper on a node with two readers")
        for s, (sa, _, o) in zip(st, gv.slot_plan(st)[0]):
            if sa >= 0 and sa != o and not gv.is_math2(s) and not s.ar_param:
                have.add("a stage's input is copied into another slot in front of its tile code")
        for kind in w.links.values():
            have.add(("link", kind))
        if st[-1].kind == L.STAGE_PAN2:
            have.add("Pan2 ends the voice")
        in_list, in_task = gv.envelope_orders(st)
        if len({st[i].kind for i in in_list}) >= 2 and in_list != in_task:
            have.add("envelopes of different kinds, task order is not list order")
        c.update(have)
    return c


def test_the_committed_seeds_cover_the_pool():
    """A condition on the seed list, not a measurement: every kind of the pool, every link kind and every structure the
    generator is for occurs in at least two of the committed seeds."""
    c = coverage([voice(f"seed{s}") for s in SEEDS])
    want = [("kind", k) for k in gv.POOL] + [("link", k) for k in gv.LINKS] + [
        "delay reads a named signal that is not adjacent", "wrapper on a node with two readers", "Pan2 ends the voice",
        "a stage's input is copied into another slot in front of its tile code",
        "envelopes of different kinds, task order is not list order"]
    short = {str(k): c[k] for k in want if c[k] < 2}
    assert not short, short
    sizes = {(voice(f"seed{s}").n_voices) for s in SEEDS}
    blocks = {(voice(f"seed{s}").block_size) for s in SEEDS}
    assert sizes == set(gv.VOICE_COUNTS) and blocks == set(gv.BLOCK_SIZES)
    assert {voice(f"seed{s}").sample_type for s in SEEDS} == {L.F32, L.F64}


def test_directed_voices_are_what_they_are_for():
    st = voice("three_envs").stages
    in_list, in_task = gv.envelope_orders(st)
    assert [st[i].kind for i in in_list] == [L.STAGE_MUL_ENV_AR, L.STAGE_MUL_ENVELOPE, L.STAGE_MUL_ENV_ASR]
    assert [st[i].kind for i in in_task] == [L.STAGE_MUL_ENV_ASR, L.STAGE_MUL_ENV_AR, L.STAGE_MUL_ENVELOPE]
    assert len(voice("nineteen").stages) == 19
    st = voice("comb_asr_pan").stages
    assert st[2].kind == L.STAGE_SAMPLE_DELAY and st[-1].kind == L.STAGE_PAN2
