"""The paths of KNH_STAGE_GALACTIC (voice_galactic.hpp, galactic_bank.hpp) that tests/test_gpu_galactic.py never enters: runs
shorter than 64 samples (sample rates below 44.1 kHz, down to the lowest knh_bank_init accepts), other rates above it, blocks
shorter than a run and one sample longer, banks of 1 / 64 / 65 voices, the phase vib_m resetting inside a run and again and
again, detune moved after init, output at and beyond 1.0 (the other branches of gal_dither_scale), and other chains in front
of the reverb.  The reference is tests/galactic_ref.py fed with the oracle's per-voice source signal, as there; with detune 0
everywhere the comparison is bit for bit on the per-voice planes and on both mixes.

Every case proves its own premise on the restatement before it trusts a pass: the runs that occurred (from the restatement's
delay_length), the resets (oldfpd changing), the share of loud samples.

Observed shares of samples not bit-identical with detune > 0 (the tests print them): DESIGN.md, "Galactic"."""
import numpy as np
import pytest

import galactic_ref as gr
from helpers import assert_bit_equal
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage
from test_gpu_galactic import SRC, Rig, check_block, gal_ctor, settings, src_ctor
from test_gpu_pan2 import FORMS

pytestmark = pytest.mark.gpu

BOTH = (L.MIX_LEFT_FOLD, L.MIX_TREE)
REPLACE, DETUNE, BRIGHTNESS, BIGNESS, WET = range(5)


def brightness_below(sr):
    """lowpass = (brightness + 1e-5)^2 / sqrt(sr / 44100), and y = y * (1 - lowpass) + x * lowpass is stable for lowpass < 2:
    brightness < sqrt(2 * sqrt(sr / 44100)) - 1e-5 (0.92 at 8 kHz, 0.60 at 1.5 kHz).  The cases stay 5 % inside."""
    return min(1.0, 0.95 * (np.sqrt(2.0 * np.sqrt(sr / 44100.0)) - 1e-5))


def settings_at(nv, sr, seed):
    p = settings(nv, seed=seed)
    p["brightness"] = p["brightness"] * brightness_below(sr)
    p["bigness"] = p["bigness"] ** 3              # most voices on short rings: several runs below 64 in one launch
    p["bigness"][0], p["bigness"][1] = 0.0, 1.0  # (settings() pins them from 8 voices up only)
    return p


def runs_of(ref):
    """GalParams::run as the restatement's rings say it must be, per voice: max(1, min(64, min(delay_length) - 1))."""
    shortest = np.min([d.delay_length for d in ref.delays_left + ref.delays_right], axis=0)
    return np.maximum(1, np.minimum(64, shortest - 1))


# rate -> (shortest delay_length at bigness 0, its run, the run at bigness 1, block size)
RATES = {44100: (68, 64, 64, 512), 96000: (148, 64, 64, 512), 22050: (34, 33, 64, 200), 8000: (12, 11, 64, 100),
         2000: (3, 2, 29, 50), 1500: (2, 1, 22, 50)}


@pytest.mark.parametrize("st", [L.F32, L.F64])
@pytest.mark.parametrize("sr", sorted(RATES))
def test_sample_rates_and_short_runs_bit_exact(knh, oracle, st, sr):
    """Ten voices, bigness 0 on voice 0 and 1 on voice 1, the rest between: below 44.1 kHz one launch holds voices with
    different runs.  As many blocks as the longest ring of the rate (15 220 / 44 100 s, bigness 1) needs to wrap."""
    shortest, run0, run1, bs = RATES[sr]
    nv = 10
    rig = Rig(knh, oracle, nv, st, bs, settings_at(nv, sr, seed=20), mixes=BOTH, sr=sr)
    longest = max(gr.ring_lengths(sr))
    n_blocks = longest // bs + 2
    loud = 0.0
    for k in range(n_blocks):
        if k % 29 == 0:
            rig.fire()
        loud = max(loud, float(np.abs(check_block(rig, f"{sr} Hz block {k}")).max()))
        if k == 0:
            assert min(int(d.delay_length[0]) for d in rig.ref.delays_left) == shortest
            runs = runs_of(rig.ref)
            assert runs[0] == run0 and runs[1] == run1
            assert set(runs.tolist()) == {64} if sr >= 44100 else len(set(runs.tolist())) >= 3, runs
    assert n_blocks * bs > int(rig.ref.delays_left[8].delay_length[1]) == longest
    assert loud > 1e-3
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
@pytest.mark.parametrize("sr", [8000, 2000])
def test_bigness_traffic_with_short_runs(knh, oracle, st, sr):
    """test_parameter_traffic_between_blocks' bigness moves where the runs are short: every voice down to the shortest rings
    (`position` of the long ones stranded beyond the new length), spread out again, 0.3, 1.0, 0.05."""
    nv, bs = 12, 64
    rig = Rig(knh, oracle, nv, st, bs, settings_at(nv, sr, seed=21), sr=sr)
    rig.fire()
    seen = set()
    stranded = False
    for k in range(28):
        if k == 3:
            before = [d.position.copy() for d in rig.ref.delays_left]
            rig.set_param(BIGNESS, 0.0)
        if k == 5:
            rig.set_param(BIGNESS, np.linspace(0.0, 1.0, nv))
        if k == 11:
            rig.set_param(BIGNESS, 0.3)
            rig.fire()
        if k == 12:
            rig.set_param(BIGNESS, 1.0)
            rig.set_param(BRIGHTNESS, np.linspace(1.0, 0.0, nv) * brightness_below(sr))
        if k == 20:
            rig.set_param(BIGNESS, 0.05)
        check_block(rig, f"{sr} Hz block {k}")
        seen |= set(runs_of(rig.ref).tolist())
        if k == 3:
            stranded = any(bool((pos >= d.delay_length).any()) for pos, d in zip(before, rig.ref.delays_left))
    assert stranded, "no ring's position lay beyond its new length at the shrink"
    assert RATES[sr][1] in seen and RATES[sr][2] in seen and len(seen) >= 4, seen
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_partial_blocks_with_short_runs(knh, oracle, st):
    """8 kHz, runs of 11 .. 64: a block of 100 as 37 + 63 frames (37 is prime: the first call ends inside a run of every voice)."""
    sr, nv, bs = 8000, 10, 100
    rig = Rig(knh, oracle, nv, st, bs, settings_at(nv, sr, seed=22), sr=sr)
    g = rig.gpu[0]
    rig.fire()
    for k in range(12):
        want = rig.ref_block()
        if k == 0:
            runs = runs_of(rig.ref)
            assert runs[0] == 11 and 37 % 11 != 0 and len(set(runs.tolist())) >= 3, runs
        out_a, _, _ = g.process_block_voices(37, 0)
        out_b, voices, _ = g.process_block_voices(63, 37)
        assert_bit_equal(voices, want, f"block {k} in two calls: per-voice left/right")
        mix = want[:, 0].copy()
        for v in range(1, nv):
            mix = mix + want[:, v]
        assert_bit_equal(np.concatenate([out_a[:, :37], out_b[:, 37:]], axis=1), mix, f"block {k} in two calls: left fold")
    assert rig.peak > 1e-3
    rig.close()


def test_lowest_sample_rate(knh, oracle):
    """knh_bank_init refuses a rate whose shortest ring would hold fewer than 2 samples at bigness 0 (read() after
    write_and_advance() would return the sample just written), as an ordinary error; the lowest rate it takes runs sample by
    sample."""
    assert gr.ring_lengths(1297)[3] == 19 and gr.ring_lengths(1298)[3] == 20  # x 0.1: 1 sample, 2 samples
    nv, bs = 6, 48
    p = settings_at(nv, 1298, seed=23)
    for st in (L.F32, L.F64):
        z = knh.VoiceBank(SRC + [Stage(L.STAGE_GALACTIC)], nv, st, 2)
        for s, c in src_ctor(nv, sr=1297).items():
            z.set_ctor_args(s, c)
        z.set_ctor_args(3, gal_ctor(p))
        with pytest.raises(L.KnasterHipError) as e:
            z.init(1297, bs)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "shortest delay line" in str(e.value)
        z.close()
        rig = Rig(knh, oracle, nv, st, bs, p, mixes=BOTH, sr=1298)
        rig.fire()
        for k in range(12):  # 576 samples: the longest ring (447) wraps
            check_block(rig, f"1298 Hz block {k}")
            if k == 0:
                runs = runs_of(rig.ref)
                assert runs[0] == 1 and int(rig.ref.delays_left[3].delay_length[0]) == 2
        assert rig.peak > 1e-3
        rig.close()


@pytest.mark.parametrize("bs,nv,st", [
    (1, 65, L.F32), (16, 64, L.F32), (63, 65, L.F32), (63, 1, L.F64), (65, 64, L.F32), (65, 65, L.F64), (65, 1, L.F32),
    (512, 1, L.F64), (512, 65, L.F32)])
def test_block_shapes_and_bank_sizes(knh, oracle, bs, nv, st):
    """48 kHz (runs of 64): a block shorter than a run, one sample short of it, one sample over (a one-sample tail run), eight
    runs; one voice, a full wavefront of voices for the fold kernels, one more.  bigness at most 0.05 (rings at most 1.45
    times their shortest): the burst first leaves the three banks after 870 samples at the latest and, fed back, a second
    time after 1 630; every case runs 2 600, so the feedback a run hands to the next is in the output."""
    p = settings(nv, seed=24 + nv)
    p["bigness"] = 0.05 * p["bigness"]
    rig = Rig(knh, oracle, nv, st, bs, p, mixes=BOTH)
    # the first arrival of the feedback at its latest: 110 samples in the short ring, then twice through each bank's shortest ring
    lens = [min(int(d.buffer_len() * 0.145) for d in rig.ref.delays_left[4 * b:4 * b + 4]) for b in range(3)]
    assert 110 + 2 * sum(lens) < 2600 - 800
    loud = 0.0
    for k in range(-(-2600 // bs)):
        if k == 0:
            rig.fire()
        loud = max(loud, float(np.abs(check_block(rig, f"block {k} of {bs}")).max()))
    assert loud > 1e-3
    rig.close()


def run_within_tolerance(rig, n_blocks, what, fire_every=0, between=None):
    """test_detune_within_tolerance's comparison: worst absolute error over the per-voice planes, the count of samples not
    bit-identical.  Returns per-voice counts [nv]."""
    differ = np.zeros(rig.nv, dtype=np.int64)
    total = 0
    worst = 0.0
    for k in range(n_blocks):
        if between is not None:
            between(k)
        if fire_every and k % fire_every == 0:
            rig.fire()
        want = rig.ref_block()
        _, voices, _ = rig.gpu[0].process_block_voices()
        worst = max(worst, float(np.abs(voices.astype(np.float64) - want).max()))
        differ += np.count_nonzero(voices != want, axis=(0, 2))
        total += want.size
    print(f"galactic {what} {'f64' if rig.dtype == np.float64 else 'f32'}: {int(differ.sum())} of {total} samples not bit-identical "
          f"({differ.sum() / total:.3e}), worst |error| {worst:.3e}")
    assert rig.peak > 1e-3
    assert worst <= 1e-4
    return differ


@pytest.mark.parametrize("st", [L.F32, L.F64])
@pytest.mark.parametrize("detune,first_reset", [(0.05, 61), (0.15, 2)])
def test_first_reset_inside_a_run(knh, oracle, st, detune, first_reset):
    """The phase leaves 3.0 in steps of 429496.7295 * detune^3 * 0.001 (0.054, 1.45) and passes 2 pi at sample `first_reset` of
    the first run: the lanes before it read the ring with one phase, the lanes from it on with another, and the voice's next
    step comes from its own fpd_l at that sample.  Tolerance as in test_detune_within_tolerance (replace >= 0.5)."""
    nv, bs = 16, 256
    rig = Rig(knh, oracle, nv, st, bs, settings(nv, seed=40, detune=detune, replace_lo=0.5))
    # the restatement's phase, stepped here in the same f64 arithmetic, resets where the docstring says
    drift = float(gr._powi(rig.ref.param[DETUNE][:1], 3)[0] * rig.dtype(0.001))
    vib, at = 3.0, 0
    while True:
        vib += 429496.7295 * drift
        if vib > 2.0 * np.pi:
            break
        at += 1
    assert at == first_reset and 0 < at < 63
    run_within_tolerance(rig, 8, f"detune={detune}", fire_every=4)
    assert len(set(rig.ref.oldfpd.tolist())) == nv and np.all(rig.ref.oldfpd < 1.0)
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_many_resets(knh, oracle, st):
    """detune 3.0 (nothing clamps it to the 0 .. 1 of its hint): after the first reset a step is oldfpd * 0.027 = 0.012 .. 0.019,
    a reset every 340 .. 540 samples, each inside some run, each drawing a new oldfpd from the voice's own stream.  A burst
    every block of 256 keeps signal in the 256-sample ring at every reset."""
    nv, bs, n_blocks = 16, 256, 17
    rig = Rig(knh, oracle, nv, st, bs, settings(nv, seed=41, detune=3.0, replace_lo=0.5))
    resets = np.zeros(nv, dtype=np.int64)
    last = [rig.ref.oldfpd.copy()]

    def between(k):  # (a block is shorter than the shortest interval: at most one reset per voice and block)
        resets[:] += rig.ref.oldfpd != last[0]
        last[0] = rig.ref.oldfpd.copy()

    run_within_tolerance(rig, n_blocks, "detune=3.0", fire_every=1, between=between)
    between(n_blocks)
    assert n_blocks * bs >= 4000 and resets.min() >= 5, resets
    assert len(set(rig.ref.oldfpd.tolist())) == nv
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_detune_traffic(knh, oracle, st):
    """Every voice starts with detune 0: the host's offsets for vib_m = 3.0 are in use.  Then 0.6 (the device's sin takes
    over), 0 (the phase frozen somewhere else than 3.0: the device's sin still), 0.05, 0 -- by param_apply_many for some of the
    voices that move and by param_apply_range for a stretch of them.  Voice 0 and the last six stay at 0 throughout and must
    stay bit-identical."""
    nv, bs = 24, 128
    rig = Rig(knh, oracle, nv, st, bs, settings(nv, seed=42, detune=0.0, replace_lo=0.5))
    g = rig.gpu[0]
    still = np.array([0, 18, 19, 20, 21, 22, 23])
    moving = np.arange(1, 18)
    many = np.concatenate([np.arange(1, 6), np.arange(12, 18)])

    def detune(value):
        rig.set_param(DETUNE, value, voices=many)                          # param_apply_many
        g.param_apply_range(6, 12, rig.G, DETUNE, L.VALUE_FLOAT, value)    # param_apply_range
        rig.ref.set_param(DETUNE, value, voices=np.arange(6, 12))

    frozen = {}

    def between(k):
        if k in (2, 5, 8, 11):
            detune({2: 0.6, 5: 0.0, 8: 0.05, 11: 0.0}[k])
        if k in (2, 5, 8, 14):
            frozen[k] = rig.ref.vib_m.copy()

    differ = run_within_tolerance(rig, 14, "detune 0 -> 0.6 -> 0 -> 0.05 -> 0", fire_every=3, between=between)
    between(14)
    assert np.all(frozen[2] == 3.0)                                  # blocks 0, 1: the host's offsets
    assert np.all(frozen[5][moving] != 3.0) and np.array_equal(frozen[8], frozen[5])  # blocks 5 .. 7: frozen off 3.0
    assert np.all(frozen[14][moving] != frozen[8][moving])            # blocks 8 .. 10 moved it again
    assert np.all(frozen[14][still] == 3.0)
    assert not differ[still].any(), f"voices whose detune stayed 0 are not bit-identical: {differ[still]}"
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_loud_output_bit_exact(knh, oracle, st):
    """A source of amplitude 3 (40 on every fourth voice), wet 0 / 0.3 / 1 by voice, detune 0: output samples in all three
    classes of gal_dither_scale -- |s| < 1 (2^62), 1 <= |s| < 2 (2^63), |s| >= 2 (the reference's 2_u64.pow wraps to 0: no
    dither).  The kernel reads the exponent from the f32's bits where the reference takes floor(log2f(|s|)) + 1; a sample a hair
    below a power of two, where the two could differ, would be a difference of definition: the case asserts it holds none."""
    nv, bs, n_blocks = 12, 250, 24
    p = settings(nv, seed=43)
    p["wet"] = np.array([0.0, 0.3, 1.0])[np.arange(nv) % 3]
    p["replace"] = 0.5 + 0.5 * p["replace"]
    amp = np.where(np.arange(nv) % 4 == 3, 40.0, 3.0)
    ctor = src_ctor(nv)
    ctor[1] = amp.reshape(nv, 1)
    ctor[2] = np.tile([0.002, 0.03], (nv, 1))  # 96 + 1 440 samples: the decay passes slowly through 2 and 1
    rig = Rig(knh, oracle, nv, st, bs, p, mixes=BOTH, src=(SRC, ctor, (2, 2)), peak_limit=None)
    everything = []
    for k in range(n_blocks):
        if k % 8 == 0:
            rig.fire()
        everything.append(check_block(rig, f"block {k}"))
    s = np.concatenate(everything, axis=2).astype(np.float32)
    assert np.isfinite(s).all()
    mag = np.abs(s)
    shares = [float(np.mean(mag < 1.0)), float(np.mean((mag >= 1.0) & (mag < 2.0))), float(np.mean(mag >= 2.0))]
    print(f"galactic loud {'f64' if st else 'f32'}: shares of |s| < 1, [1, 2), >= 2: {shares}")
    assert min(shares) >= 0.05, shares
    nz = mag[mag != 0]
    assert np.array_equal(np.floor(np.log2(nz)) + np.float32(1.0), np.frexp(nz)[1].astype(np.float32))
    rig.close()


def c3_source(nv, bs, st, precise=0):
    """C3's voice, SinWt.wr_mul -> SvfFilter(Low) -> * EnvAsr, at a gain the reverb's output can be told from silence with."""
    w = configs.config("C3", n_voices=nv, block_size=bs, sample_type=st, precise=precise)
    w.ctor[1] = np.full((nv, 1), 0.1)
    return w


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_filter_chain_in_front_in_every_kernel_form(knh, oracle, monkeypatch, form, st):
    """The chain in front of the reverb in the forms the environment switches of tests/test_gpu_pan2.py select, 70 voices (one
    full voice group and six lanes of another): whatever kernel renders the voices into the staging buffer, the reverb's
    output is the restatement's of the oracle's voices."""
    for k, val in FORMS[form].items():
        monkeypatch.setenv(k, val)
    nv, bs = 70, 128
    w = c3_source(nv, bs, st)
    rig = Rig(knh, oracle, nv, st, bs, settings(nv, seed=50), mixes=BOTH, src=(w.stages, w.ctor, w.restart))
    v = np.arange(nv, dtype=np.uint32)
    for k in range(8):
        if k == 0:
            rig.fire()
        if k == 2:
            rig.inner(lambda b: b.param_apply_many(v, w.release[0], w.release[1], L.VALUE_TRIGGER))
        if k == 3:
            rig.inner(lambda b: b.param_apply_many(v[1::4], 0, 0, L.VALUE_FLOAT, 220.0 + 3.0 * v[1::4]))
            rig.fire()
        check_block(rig, f"{form} block {k}")
    assert rig.peak > 1e-3
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_sample_accurate_change_in_front(knh, oracle, st):
    """WrPreciseTiming on the envelope in front of the reverb: releases and restarts that land mid-block, at a different
    frame per voice, and a block rendered in two calls around them."""
    nv, bs = 70, 96
    w = c3_source(nv, bs, st, precise=2)
    assert w.stages[3].delayed_changes_per_block == 2
    rig = Rig(knh, oracle, nv, st, bs, settings(nv, seed=51), mixes=BOTH, src=(w.stages, w.ctor, w.restart))
    v = np.arange(nv, dtype=np.uint32)
    delays = ((17 * v) % bs).astype(np.uint16)
    rig.fire()
    for k in range(10):
        if k in (2, 6):
            rig.inner(lambda b: b.param_apply_many(v, 3, 2, L.VALUE_TRIGGER, delays=delays))
        if k == 4:
            rig.inner(lambda b: b.param_apply_many(v, 3, 3, L.VALUE_TRIGGER, delays=delays[::-1].copy()))
        if k == 6:
            rig.inner(lambda b: b.param_apply_many(v[::2], 3, 3, L.VALUE_TRIGGER, delays=np.full(len(v[::2]), bs - 1, dtype=np.uint16)))
        check_block(rig, f"block {k}")
    assert rig.peak > 1e-3
    rig.close()


def arithmetic_voice(nv):
    """Two oscillators ring-modulated, scaled: SinWt oscillators and arithmetic alone, no pre-built kernel -- the voice
    takes the frame-parallel form (voice_bank.hpp), whose rows are copied into the reverb's staging buffer."""
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MATH_MUL, input=1, input2=2), Stage(L.STAGE_MUL_CONST)]
    f = 110.0 + 7.0 * np.arange(nv)
    return st, {0: f.reshape(nv, 1), 1: np.full((nv, 1), 3.0), 3: np.full((nv, 1), 0.25)}, None


@pytest.mark.parametrize("frame_jit", ["1", "0"])
@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_frame_parallel_voice_in_front(knh, oracle, monkeypatch, frame_jit, st):
    """A voice of oscillators and arithmetic in front of the reverb, as the kernel built at init (KNH_FRAME_JIT=1, the default)
    and as the interpreter (0); whole blocks, a block in two calls, and a frequency moved between blocks."""
    monkeypatch.setenv("KNH_FRAME_JIT", frame_jit)
    nv, bs = 70, 96
    stages, ctor, _ = arithmetic_voice(nv)
    p = settings(nv, seed=52)
    p["wet"] = 0.5 * p["wet"]              # (a steady tone at 0.25: keep the sum of dry and tail below 1.0)
    p["replace"] = 0.5 + 0.5 * p["replace"]
    rig = Rig(knh, oracle, nv, st, bs, p, mixes=BOTH, src=(stages, ctor, None))
    v = np.arange(nv, dtype=np.uint32)
    for k in range(12):
        if k == 5:
            rig.inner(lambda b: b.param_apply_many(v[::3], 1, 0, L.VALUE_FLOAT, 2.0 + 0.25 * v[::3]))
        if k in (3, 7):  # a block in two calls
            want = rig.ref_block()
            for b in rig.gpu:
                b.process_block_voices(40, 0)
                _, voices, _ = b.process_block_voices(56, 40)
                assert_bit_equal(voices, want, f"block {k} in two calls")
        else:
            check_block(rig, f"block {k}")
    assert rig.peak > 1e-3
    rig.close()
