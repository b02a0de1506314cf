"""Pins tests/galactic_ref.py -- the numpy restatement of the Galactic reverb that judges KNH_STAGE_GALACTIC on the GPU
(tests/test_gpu_galactic.py) -- before it judges anything, and checks what knh_bank_create accepts and refuses for a chain
that ends in the reverb (creation needs no device).  Citations are file:line in the knaster repo."""
import numpy as np
import pytest

import galactic_ref as gr
from knaster_amd import _lib as L
from knaster_amd.bank import Stage


@pytest.mark.parametrize("n_voices", [1, 3])
def test_static_sample_delay_doctest(n_voices):
    """delay.rs:273-307, value for value: the only reference-held vector on this path."""
    d = gr.StaticSampleDelay(4, n_voices, np.float64)
    eq = lambda a, b: np.testing.assert_array_equal(a, np.broadcast_to(np.asarray(b, dtype=np.float64), np.shape(a)))  # noqa: E731
    eq(d.read(), 0.0)
    for w, r in [(1.0, 0.0), (2.0, 0.0), (3.0, 0.0), (4.0, 1.0), (0.0, 2.0), (0.0, 3.0), (0.0, 4.0), (0.0, 0.0)]:
        d.write_and_advance(w)
        eq(d.read(), r)
    d.write_and_advance(0.0)
    blk = lambda a, b: np.tile(np.array([a, b]), (n_voices, 1))  # noqa: E731
    d.write_block_and_advance(blk(1.0, 2.0))
    d.read_block(2)
    d.write_block_and_advance(blk(3.0, 4.0))
    eq(d.read_block(2), blk(1.0, 2.0))
    d.write_block_and_advance(blk(5.0, 6.0))
    eq(d.read_block(2), blk(3.0, 4.0))
    d.write_block_and_advance(blk(0.0, 0.0))
    eq(d.read_block(2), blk(5.0, 6.0))


def test_ring_lengths():
    """((t / 44100) * sample_rate) as usize for GALACTIC_DELAY_TIMES (galactic.rs:39-41, :52-60)."""
    assert gr.ring_lengths(44100) == [6480, 3660, 1720, 680, 9700, 6000, 2320, 940, 15220, 8460, 4540, 3200]
    assert gr.ring_lengths(48000) == [7053, 3983, 1872, 740, 10557, 6530, 2525, 1023, 16565, 9208, 4941, 3482]
    assert gr.ring_lengths(96000) == [14106, 7967, 3744, 1480, 21115, 13061, 5050, 2046, 33131, 18416, 9882, 6965]
    # the state of one f32 voice: 2 x 12 long rings + 2 x 256, about 550 KB at 48 kHz
    assert 2 * sum(gr.ring_lengths(48000)) + 512 == 137470
    # shortest delay_length at bigness 0 (size 0.1): a 64-sample run fits from 44.1 kHz up
    for sr, want in [(44100, 68), (48000, 74), (96000, 148)]:
        d = gr.StaticSampleDelay(min(gr.ring_lengths(sr)), 1, np.float32)
        d.set_delay_length_fraction((np.float32(0.0) * np.float32(0.9)) + np.float32(0.1))
        assert int(d.delay_length[0]) == want


def test_set_delay_length_keeps_position():
    """delay.rs:337-342 does not touch `position`; write_and_advance wraps with % delay_length only after the write."""
    d = gr.StaticSampleDelay(10, 1, np.float32)
    for k in range(7):
        d.write_and_advance(np.float32(k + 1))
    d.set_delay_length_fraction(np.float32(0.5))
    assert int(d.position[0]) == 7 and int(d.delay_length[0]) == 5
    d.write_and_advance(np.float32(99.0))  # lands at 7, beyond the new length
    assert d.buffer[0, 7] == 99.0 and int(d.position[0]) == 3


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dry_path_is_input_plus_dither(dtype):
    """wet = 0: the output is the dry input plus the dither term, exactly."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 300)) * 0.2).astype(dtype)
    g = gr.Galactic(2, dtype, 0.5, 0.0, 0.5, 0.5, 0.0, [77777, 123456789], [99999, 3000000001])
    g.init(48000)
    fl = np.array([77777, 123456789], dtype=np.uint32)
    out_l, out_r = g.process(x, x)
    for k in range(x.shape[1]):
        fl ^= fl << np.uint32(13)
        fl ^= fl >> np.uint32(17)
        fl ^= fl << np.uint32(5)
        # |x| < 1 here: exponent 0, 2^62
        want = x[:, k] + ((fl.astype(np.float64) - 2147483647.0) * 5.5e-36 * float(2 ** 62)).astype(dtype)
        np.testing.assert_array_equal(out_l[:, k], want)
    assert np.abs(out_r - x).max() < 1e-6 and not np.array_equal(out_l, out_r)


def test_impulse_arrives_when_the_rings_say():
    """wet = 1, detune = 0: nothing but dither-sized samples before the first arrival the ring lengths predict."""
    sr = 48000
    lens = gr.ring_lengths(sr)
    bigness = 0.0
    size = np.float32(np.float32(bigness) * np.float32(0.9)) + np.float32(0.1)
    dl = [int(np.float32(n) * size) for n in lens]
    # the 256-sample ring is read (sin(3) + 1) * 127 = 144.9 slots ahead of `position`, which is one past the write: the
    # interpolation's upper sample (slot position + 145) is the impulse 256 - 145 - 1 = 110 samples after it was written;
    # then the shortest ring of each of the three banks, each delay_length - 1 (read() after write_and_advance())
    first = (256 - int(np.ceil((np.sin(3.0) + 1.0) * 127.0)) - 1) + sum(min(dl[4 * b:4 * b + 4]) - 1 for b in range(3))
    x = np.zeros((1, first + 200), dtype=np.float32)
    x[0, 0] = 0.25
    g = gr.Galactic(1, np.float32, 1.0, 0.0, 1.0, bigness, 1.0, 1234567, 7654321)
    g.init(sr)
    out_l, out_r = g.process(x, x)
    assert np.abs(out_l[0, :first]).max() < 1e-6 and np.abs(out_r[0, :first]).max() < 1e-6
    assert np.abs(out_l[0, first:]).max() > 1e-4 and np.abs(out_r[0, first:]).max() > 1e-4


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("detune", [0.0, 0.8])
def test_scalar_and_vectorised_agree_bit_for_bit(f32, detune):
    dtype = np.float32 if f32 else np.float64
    n = 3000
    rng = np.random.default_rng(11)
    x = np.zeros(n)
    x[:400] = rng.standard_normal(400) * 0.1 * np.linspace(1, 0, 400)
    x[1500:1520] = 0.2
    x = x.astype(dtype)
    args = (0.3, detune, 0.7, 0.05, 0.6)
    v = gr.Galactic(2, dtype, *args, [424242, 5], [31337, 6])
    v.init(44100)
    s = gr.ScalarGalactic(f32, 44100, *args, 424242, 31337)
    outs_v = [np.zeros((2, 0), dtype=dtype), np.zeros((2, 0), dtype=dtype)]
    outs_s = [[], []]
    for b in range(3):  # three process calls; bigness moves between them (a shrink that strands `position`, then growth)
        seg = x[b * 1000:(b + 1) * 1000]
        ol, orr = v.process(np.tile(seg, (2, 1)), np.tile(seg, (2, 1)))
        outs_v = [np.concatenate([outs_v[0], ol], axis=1), np.concatenate([outs_v[1], orr], axis=1)]
        sl, sr_ = s.process([float(t) for t in seg])
        outs_s[0] += sl
        outs_s[1] += sr_
        new_big = [0.0, 0.9][b % 2]
        v.set_param(gr.Galactic.BIGNESS, new_big)
        s.p[3] = s.r(new_big)
    for c in range(2):
        a = outs_v[c][0]
        b_ = np.array(outs_s[c], dtype=dtype)
        assert np.array_equal(a.view(np.uint32 if f32 else np.uint64), b_.view(np.uint32 if f32 else np.uint64)), f"channel {c}"
        assert np.abs(a).max() > 1e-3


def _both(f32, sr, args, x, between=None, n_calls=3, seeds=((424242, 31337), (5, 6))):
    """`x` through Galactic (two voices, the second with other seeds) and through one ScalarGalactic per voice, in `n_calls`
    process calls; between(k, set_param) moves parameters after call k.  Asserts every sample of both channels of both voices
    bit-identical; returns (left, right) of voice 0 and the vectorised object."""
    dtype = np.float32 if f32 else np.float64
    x = np.asarray(x).astype(dtype)
    v = gr.Galactic(2, dtype, *args, [s[0] for s in seeds], [s[1] for s in seeds])
    v.init(sr)
    ss = [gr.ScalarGalactic(f32, sr, *args, *s) for s in seeds]

    def set_param(index, value):
        v.set_param(index, value)
        for s in ss:
            s.p[index] = s.r(value)

    n = len(x) // n_calls
    got = [[], []]
    want = [[[], []], [[], []]]
    for k in range(n_calls):
        seg = x[k * n:(k + 1) * n]
        ol, orr = v.process(np.tile(seg, (2, 1)), np.tile(seg, (2, 1)))
        got[0].append(ol)
        got[1].append(orr)
        for i, s in enumerate(ss):
            sl, sr_ = s.process([float(t) for t in seg])
            want[i][0] += sl
            want[i][1] += sr_
        if between is not None:
            between(k, set_param)
    u = np.uint32 if f32 else np.uint64
    got = [np.concatenate(g, axis=1) for g in got]
    for i in range(2):
        for c in range(2):
            w = np.array(want[i][c], dtype=dtype)
            assert np.isfinite(w).all()
            differ = np.flatnonzero(got[c][i].view(u) != w.view(u))
            assert differ.size == 0, f"voice {i} channel {c}: {differ.size} samples differ, first at {differ[0]}"
    for s, want_vib, want_old in zip(ss, v.vib_m, v.oldfpd):
        assert s.vib == want_vib and s.old == want_old
    return got[0][0], got[1][0], v


def _burst(n, amp=0.1, seed=11):
    rng = np.random.default_rng(seed)
    x = np.zeros(n)
    m = min(400, n // 4)
    x[:m] = rng.standard_normal(m) * amp * np.linspace(1, 0, m)
    x[n // 2:n // 2 + 20] = 2.0 * amp
    return x


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("sr,min_len", [(1500, 2), (2000, 3), (8000, 12), (22050, 34), (96000, 148)])
def test_scalar_and_vectorised_agree_at_other_sample_rates(f32, sr, min_len):
    """Rings of 2 .. 33 131 samples: the short ones wrap many times per call.  bigness starts at 0 (the shortest rings the rate
    has), then moves as in the 44.1 kHz case: growth, then the shrink that strands `position`.  brightness 0.5 keeps the
    one-pole's coefficient (brightness + 1e-5)^2 / sqrt(sr / 44100) below 2 down to 1 500 Hz (1.36 there)."""
    n = 2400 if sr < 44100 else 1500

    def between(k, set_param):
        set_param(gr.Galactic.BIGNESS, [0.9, 0.0][k % 2])

    dtype = np.float32 if f32 else np.float64
    probe = gr.Galactic(1, dtype, 0.3, 0.0, 0.5, 0.0, 0.6, 1, 1)
    probe.init(sr)
    probe.process(np.zeros((1, 1), dtype=dtype), np.zeros((1, 1), dtype=dtype))
    seen = min(int(d.delay_length[0]) for d in probe.delays_left)
    assert seen == min_len
    left, right, _ = _both(f32, sr, (0.3, 0.0, 0.5, 0.0, 0.6), _burst(n), between)
    assert np.abs(left).max() > 1e-3 and np.abs(right).max() > 1e-3


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("detune,least_resets", [(0.05, 1), (3.0, 5)])
def test_scalar_and_vectorised_agree_through_phase_resets(f32, detune, least_resets):
    """detune 0.05: the phase leaves 3.0 in steps of 429496.7 * 1.25e-7 = 0.054 and first passes 2 pi some 60 samples in;
    detune 3.0 (the 0 .. 1 of the parameter is a hint: nothing clamps it): after the first reset a step is
    oldfpd * 0.027 = 0.012 .. 0.019, a reset every 340 .. 540 samples."""
    n = 3000
    resets = [0, 0]
    old = [429496.7295, 429496.7295]

    dtype = np.float32 if f32 else np.float64
    # count the resets on the vectorised object, call by call of 100 samples (oldfpd changes at a reset: the seeds' streams
    # do not repeat a value within 2^32 - 1 steps)
    x = _burst(n).astype(dtype)
    v = gr.Galactic(2, dtype, 0.6, detune, 0.7, 0.05, 0.6, [424242, 5], [31337, 6])
    v.init(44100)
    for k in range(0, n, 100):
        seg = np.tile(x[k:k + 100], (2, 1))
        v.process(seg, seg)
        for i in range(2):
            if v.oldfpd[i] != old[i]:
                resets[i] += 1
                old[i] = v.oldfpd[i]
    assert min(resets) >= least_resets, resets
    assert v.oldfpd[0] != v.oldfpd[1]
    left, right, v3 = _both(f32, 44100, (0.6, detune, 0.7, 0.05, 0.6), x)
    assert np.array_equal(v3.oldfpd, v.oldfpd) and np.array_equal(v3.vib_m, v.vib_m)  # (100-sample calls or 1 000: the same)
    assert np.abs(left).max() > 1e-3 and np.abs(right).max() > 1e-3


@pytest.mark.parametrize("f32", [True, False])
def test_scalar_and_vectorised_agree_when_detune_moves(f32):
    """0 -> 0.6 -> 0 -> 0.05: the phase is still at its initial 3.0 in the first call, moves, is frozen at some other value
    (its sine is no longer the constant of the first call), and moves again, slowly."""
    seq = [0.6, 0.0, 0.05]
    frozen = []

    def between(k, set_param):
        if k < len(seq):
            set_param(gr.Galactic.DETUNE, seq[k])

    n = 3200
    x = np.concatenate([_burst(n // 4, seed=s) for s in range(4)])
    left, right, v = _both(f32, 44100, (0.6, 0.0, 0.7, 0.05, 0.6), x, between, n_calls=4)
    assert np.all(v.vib_m != 3.0)
    # the call with detune back at 0 must have run with the phase off 3.0: replay the first two calls and look
    dtype = np.float32 if f32 else np.float64
    w = gr.Galactic(1, dtype, 0.6, 0.0, 0.7, 0.05, 0.6, 424242, 31337)
    w.init(44100)
    for k in range(3):
        seg = x[k * 800:(k + 1) * 800].astype(dtype).reshape(1, -1)
        w.process(seg, seg)
        frozen.append(float(w.vib_m[0]))
        if k < 2:
            w.set_param(gr.Galactic.DETUNE, seq[k])
    assert frozen[0] == 3.0 and frozen[1] != 3.0 and frozen[2] == frozen[1]
    assert np.abs(left).max() > 1e-3 and np.abs(right).max() > 1e-3


@pytest.mark.parametrize("f32", [True, False])
def test_scalar_and_vectorised_agree_on_loud_output(f32):
    """Output samples in all three classes of the dither's exponent: |s| < 1 (2^62), 1 <= |s| < 2 (2^63), |s| >= 2 (2_u64.pow
    wraps to 0 in a release build: no dither).  The input is a decaying sine of amplitude 3 or 40, dry (wet 0), mixed (0.3)
    and reverb alone (1); over the six runs each class must hold at least 5 % of the samples."""
    n = 1500
    t = np.arange(n)
    mags = []
    for amp in (3.0, 40.0):
        for wet in (0.0, 0.3, 1.0):
            x = amp * np.sin(t * 0.31) * np.exp(-t / 500.0)
            left, right, _ = _both(f32, 44100, (0.8, 0.0, 0.7, 0.05, wet), x)
            mags.append(np.abs(np.concatenate([left, right])))
    mag = np.concatenate(mags)
    for lo, hi in [(0.0, 1.0), (1.0, 2.0), (2.0, np.inf)]:
        share = np.count_nonzero((mag >= lo) & (mag < hi)) / mag.size
        assert share >= 0.05, (lo, hi, share)


def _chain(*extra, galactic=Stage(L.STAGE_GALACTIC)):
    return [Stage(L.STAGE_SIN_WT), *extra, galactic]


def test_galactic_bank_creation_without_device(knh):
    """knh_bank_create is device-free: a chain that ends in the reverb is accepted, and each refusal has its status."""
    b = knh.VoiceBank(_chain(), 4, L.F32, 2)
    assert b.outputs() == 2
    assert b.stage_param_descriptions(1) == ["replace", "detune", "brightness", "bigness", "wet"]
    b.close()
    knh.VoiceBank(_chain(Stage(L.STAGE_WR_MUL), Stage(L.STAGE_MUL_ENV_AR)), 4, L.F64, 2, L.MIX_LEFT_FOLD).close()
    assert L.STAGE_CTOR_ARGS[L.STAGE_GALACTIC] == 7

    def refused(stages, out_channels=2, **kw):
        with pytest.raises(L.KnasterHipError) as e:
            knh.VoiceBank(stages, 4, L.F32, out_channels, **kw)
        return e.value

    assert refused(_chain(), out_channels=1).status == L.ERR_INVALID_ARGUMENT            # two channels come out of it
    assert refused([Stage(L.STAGE_SIN_WT), Stage(L.STAGE_GALACTIC), Stage(L.STAGE_MUL_CONST)]).status == L.ERR_INVALID_ARGUMENT  # last
    assert refused([Stage(L.STAGE_GALACTIC)]).status == L.ERR_INVALID_ARGUMENT           # needs a signal
    assert refused(_chain(galactic=Stage(L.STAGE_GALACTIC, delayed_changes_per_block=2))).status == L.ERR_INVALID_ARGUMENT
    assert refused(_chain(Stage(L.STAGE_MUL_CONST), galactic=Stage(L.STAGE_GALACTIC, ar_param=1, input2=1))).status == L.ERR_INVALID_ARGUMENT
    assert refused(_chain(Stage(L.STAGE_SAMPLE_DELAY))).status == L.ERR_INVALID_ARGUMENT  # no other delay-ring stage
    assert refused(_chain(Stage(L.STAGE_ALLPASS_FB_DELAY))).status == L.ERR_INVALID_ARGUMENT
    assert refused(_chain(Stage(L.STAGE_PAN2))).status == L.ERR_INVALID_ARGUMENT          # Pan2 must itself be last
    # both inputs of the reverb are the voice's running signal
    assert refused([Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_GALACTIC, input=1)]).status == L.ERR_INVALID_ARGUMENT
