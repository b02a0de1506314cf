"""KNH_STAGE_FLAG_ENV_SOURCE on the device: EnvAsr, EnvAr and the segment Envelope as source stages, every case of
tests/env_source_cases.py against its oracle twin (INPUT on a plane of ones, then the multiplying form: `1.0 * e` is `e`),
bit for bit in per-voice samples, left-fold mix, done frames and ANY_DONE unless the case says otherwise.  ALL_DONE is held
to the rule written down at the flag (knaster_hip.h): only a stage that can silence the voice takes part.

Shapes: 70 voices (a full wavefront and a partial one), 300 for the forms with several wavefronts per workgroup (two
workgroups at four), blocks of 96 frames (f32 pipeline tiles of 32; a 64-frame tile and a partial one in the whole-chain
forms), 8 blocks at 48 kHz.  Attack 0.1 .. 4 ms and release 0.2 .. 6 ms spread over the voices put state changes on every
tile position and all four envelope states into every wavefront."""
import numpy as np
import pytest

import env_source_cases as ec
import galactic_ref as gr
from helpers import assert_bit_equal, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd.bank import Stage

pytestmark = pytest.mark.gpu

SWITCHES = ("KNH_JIT", "KNH_PIPELINE", "KNH_PIPE_BIG", "KNH_PAIR", "KNH_WIDE", "KNH_INTERP", "KNH_FRAME_JIT", "KNH_JIT_PIPE", "KNH_JIT_WAVES",
            "KNH_HOST_THREADS")
PIPE_FUSED, ONE_FUSED = L.DEBUG_FORM_PIPELINE_FUSED, L.DEBUG_FORM_WHOLE_CHAIN_FUSED


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def half_report_done(run):
    """a property of the inputs: at least half the voices report a done frame inside the run"""
    assert (run.done != ec.NOT_DONE).any(axis=0).mean() >= 0.5


def check_case(knh, oracle, name, n, st, form=None):
    case = ec.CASES[name]
    want = ec.twin_run(oracle, name, n, st)
    half_report_done(want)
    g = ec.make_gpu(knh, case, n, st)
    for b in range(case.blocks):
        case.traffic(g, b, n)
        out, voices, flags = g.process_block_voices()
        done = g.read_done_frames()
        what = f"{name} block {b}"
        if case.tol == 0.0:
            assert_bit_equal(voices, want.voices[b], what + ": per-voice")
            assert_bit_equal(out[:want.mix.shape[1]], want.mix[b], what + ": left-fold mix")
        else:
            err = float(np.abs(voices.astype(np.float64) - want.voices[b]).max())
            print(f"{what}: max |gpu - twin| = {err:.3e}")
            assert err <= case.tol, what
        np.testing.assert_array_equal(done, want.done[b], what + ": done frames")
        assert bool(flags & L.FLAG_ANY_DONE) == want.any_done[b], what
        assert bool(flags & L.FLAG_ALL_DONE) == want.all_done[b], what + ": ALL_DONE follows the multiplying envelopes only"
    if form is not None:
        assert int(g.debug_words()[2]) == form
    g.close()
    return want


# ---- 1. the pitch envelope in every lane-per-voice form -----------------------------------------------------------------
FORMS = [("pipeline", {}, 70, PIPE_FUSED, L.F32), ("pipeline", {}, 70, PIPE_FUSED, L.F64),
         ("waves1", {"KNH_PIPELINE": "0", "KNH_JIT_WAVES": "1"}, 70, ONE_FUSED, L.F32),
         ("waves1", {"KNH_PIPELINE": "0", "KNH_JIT_WAVES": "1"}, 70, ONE_FUSED, L.F64),
         ("waves4", {"KNH_PIPELINE": "0", "KNH_JIT_WAVES": "4"}, 300, ONE_FUSED, L.F32),
         ("waves8", {"KNH_PIPELINE": "0", "KNH_JIT_WAVES": "8"}, 300, ONE_FUSED, L.F32),
         ("waves16", {"KNH_PIPELINE": "0", "KNH_JIT_WAVES": "16"}, 300, ONE_FUSED, L.F32)]


@pytest.mark.parametrize("form,env,n,want_form,st", FORMS, ids=[f"{f[0]}-{'f64' if f[4] == L.F64 else 'f32'}" for f in FORMS])
def test_pitch_envelope_in_every_form(knh, oracle, monkeypatch, form, env, n, want_form, st):
    set_env(monkeypatch, env)
    want = check_case(knh, oracle, "pitch", n, st, want_form)
    # every source has stopped while amplitude envelopes still sound: the voice is running, ALL_DONE is off ...
    assert not want.all_done[6] and want.all_done[7]  # ... and comes on when the last amplitude envelope has run out


def test_pitch_envelope_with_64_frame_blocks(knh, oracle, monkeypatch):
    """whole tiles only, in the one-wavefront form: 12 blocks of 64 frames, the same 768 frames"""
    set_env(monkeypatch, {"KNH_PIPELINE": "0", "KNH_JIT_WAVES": "1"})
    check_case(knh, oracle, "pitch64", 70, L.F32, ONE_FUSED)


# ---- 2 - 7, 9 -------------------------------------------------------------------------------------------------------------
def test_envelope_alone_with_wrappers(knh, oracle, monkeypatch):
    """[ENV_ASR src, WR_MUL, WR_ADD]; a wr_mul change in block 3 is applied; envelope sources alone never report ALL_DONE"""
    set_env(monkeypatch, {})
    want = check_case(knh, oracle, "wrapped", 70, L.F32)
    assert not any(want.all_done) and any(want.any_done)
    assert not np.array_equal(want.voices[2], want.voices[3])


@pytest.mark.parametrize("st", [L.F32, L.F64], ids=["f32", "f64"])
def test_graph_voice_envelope_drives_a_gain(knh, oracle, monkeypatch, st):
    set_env(monkeypatch, {})
    want = check_case(knh, oracle, "gain", 70, st, ONE_FUSED)
    assert not want.all_done[4]  # the amplitude envelopes run


def test_filter_envelope(knh, oracle, monkeypatch):
    """the envelope on SvfFilter's cutoff_freq: the device's tan, within the tolerance of tests/test_gpu_ar_params.py"""
    set_env(monkeypatch, {})
    check_case(knh, oracle, "filter", 70, L.F32, ONE_FUSED)


def test_one_envelope_read_twice(knh, oracle, monkeypatch):
    set_env(monkeypatch, {})
    check_case(knh, oracle, "twice", 70, L.F32, ONE_FUSED)


@pytest.mark.parametrize("st", [L.F32, L.F64], ids=["f32", "f64"])
def test_segment_envelope_as_a_source(knh, oracle, monkeypatch, st):
    set_env(monkeypatch, {})
    check_case(knh, oracle, "segments", 70, st)


def test_attack_time_at_audio_rate(knh, oracle, monkeypatch):
    set_env(monkeypatch, {})
    check_case(knh, oracle, "ar_attack", 70, L.F32, ONE_FUSED)


@pytest.mark.parametrize("mix_mode", [L.MIX_LEFT_FOLD, L.MIX_TREE], ids=["left_fold", "tree"])
def test_connected_outputs(knh, oracle, monkeypatch, mix_mode):
    """the envelope source on output 0, the sound on output 1"""
    set_env(monkeypatch, {})
    name, n, st = "stereo", 70, L.F32
    case, want = ec.CASES[name], ec.twin_run(oracle, name, n, st)
    g = ec.make_gpu(knh, case, n, st, mix_mode)
    for b in range(case.blocks):
        case.traffic(g, b, n)
        out, voices, flags = g.process_block_voices()
        assert_bit_equal(voices, want.voices[b], f"block {b}: per-voice, both outputs")
        mix = want.mix[b] if mix_mode == L.MIX_LEFT_FOLD else np.stack([pairwise_sum(want.voices[b][c]) for c in range(2)])
        assert_bit_equal(out, mix, f"block {b}: mix")
        np.testing.assert_array_equal(g.read_done_frames(), want.done[b])
        assert bool(flags & L.FLAG_ALL_DONE) == want.all_done[b]
    g.close()


# ---- 8. restart -----------------------------------------------------------------------------------------------------------
def test_restart_of_voices_whose_source_reported_done(knh, oracle, monkeypatch):
    """Voices whose envelope source reported done in blocks 0 .. 4 are restarted before block 5 with new attack and release
    times, then started: they equal a twin whose voices were built at that block (tests/restart_cases.py's scheme), the
    others the continuing twin.  The continuing twin's wr_mul change of block 3 is what a restarted voice must have lost."""
    set_env(monkeypatch, {})
    case, n, st, k = ec.CASES["wrapped"], 70, L.F32, 5
    ctor_a = case.ctor(n)
    ctor_b = dict(ctor_a)
    ctor_b[0] = ctor_a[0] * 1.5
    cont = ec.TwinBank(oracle, case.stages, n, st, ctor_a, case.bs, want_mix=False)
    g = ec.make_gpu(knh, case, n, st)
    reported = np.zeros(n, dtype=bool)
    for b in range(k):
        for bank in (cont, g):
            case.traffic(bank, b, n)
        _, want, _, done = cont.process_block()
        _, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, want, f"block {b}")
        reported |= done != ec.NOT_DONE
    r = np.flatnonzero(reported).astype(np.uint32)
    assert 0 < len(r) < n
    fresh = ec.TwinBank(oracle, case.stages, n, st, ctor_b, case.bs, want_mix=False)
    g.set_voice_ctor_args(0, r, ctor_b[0][r])
    g.restart_voices(r)
    differs = False
    for j in range(case.blocks - k):
        for bank in (cont, fresh, g):
            case.traffic(bank, k + j, n)
            if j == 0:
                bank.param_apply_many(r, 0, 3, ec.KT)  # the new notes start
        _, va, _, da = cont.process_block()
        _, vf, _, df = fresh.process_block()
        want, want_done = np.array(va), np.array(da)
        want[r], want_done[r] = vf[r], df[r]
        differs = differs or not np.array_equal(va[r], vf[r])
        _, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, want, f"block {k + j}")
        np.testing.assert_array_equal(g.read_done_frames(), want_done)
    assert differs  # the premise: a restarted voice is not the continuing one
    for bank in (cont, fresh, g):
        bank.close()


# ---- 10. in front of Galactic ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", [L.F32, L.F64], ids=["f32", "f64"])
def test_pitch_envelope_in_front_of_galactic(knh, oracle, monkeypatch, st):
    """4 voices, 3 blocks of 64 frames: the chain in front of the reverb holds the pitch envelope.  Compared as
    tests/test_gpu_galactic.py compares: the dry signal from the oracle (here: the twin), the reverb from the numpy restatement
    (detune 0: bit for bit), its output kept below 1.0."""
    set_env(monkeypatch, {})
    case, nv, bs = ec.CASES["pitch"], 4, 64
    stages = case.stages + [Stage(L.STAGE_MUL_CONST)]  # (* 0.25: the restatement's output stays below 1.0)
    rng = np.random.default_rng(3)
    p = {k: rng.random(nv) for k in ("replace", "brightness", "bigness", "wet")}
    p["replace"] = 0.3 + 0.7 * p["replace"]
    p["detune"] = np.zeros(nv)
    fpd = [(16386 + rng.integers(0, 2 ** 32 - 20000, nv)).astype(np.float64) for _ in range(2)]
    ctor = case.ctor(nv)
    ctor[len(case.stages)] = np.full((nv, 1), 0.25)
    g = knh.VoiceBank(stages + [Stage(L.STAGE_GALACTIC)], nv, st, 2, L.MIX_LEFT_FOLD)
    for s, a in ctor.items():
        g.set_ctor_args(s, a)
    g.set_ctor_args(len(stages), np.stack([p["replace"], p["detune"], p["brightness"], p["bigness"], p["wet"], fpd[0], fpd[1]], axis=1))
    g.init(ec.SR, bs)
    dry = ec.TwinBank(oracle, stages, nv, st, ctor, bs, want_mix=False)
    ref = gr.Galactic(nv, dry.o.dtype, p["replace"], p["detune"], p["brightness"], p["bigness"], p["wet"], fpd[0].astype(np.uint32), fpd[1].astype(np.uint32))
    ref.init(ec.SR)
    for b in range(3):
        for bank in (g, dry):
            case.traffic(bank, b, nv)
        _, d, _, _ = dry.process_block()
        d = np.asarray(d).reshape(nv, bs)
        assert np.abs(d).max() > 0 or b == 0
        out_l, out_r = ref.process(d, d)
        want = np.stack([out_l, out_r])
        assert float(np.abs(want).max()) < 1.0
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, want, f"block {b}: per-voice left/right")
        mix = want[:, 0].copy()
        for v in range(1, nv):
            mix = mix + want[:, v]
        assert_bit_equal(out, mix, f"block {b}: mix")
    g.close()
    dry.close()


# ---- 11. the resident per-block call ---------------------------------------------------------------------------------------
def test_resident_calls_equal_a_launch_per_call(knh, monkeypatch):
    set_env(monkeypatch, {})
    case, n = ec.CASES["pitch"], 70

    def render(resident):
        monkeypatch.setenv("KNH_RESIDENT", "1" if resident else "0")
        g = ec.make_gpu(knh, case, n, L.F32, L.MIX_TREE)
        outs, flags = [], []
        for b in range(case.blocks):
            case.traffic(g, b, n)
            out, f = g.process_block()
            outs.append(out.copy())
            flags.append(f)
        last_done = g.read_done_frames()
        stats = g.resident_stats()
        g.close()
        return outs, flags, last_done, stats

    a, b = render(True), render(False)
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        assert_bit_equal(x, y, f"block {k}")
    assert a[1] == b[1]
    np.testing.assert_array_equal(a[2], b[2])
    assert np.abs(np.stack(b[0])).max() > 1e-3
    assert b[3] == (0, 0) and a[3][0] > 0, (a[3], b[3])  # a resident kernel did serve calls
