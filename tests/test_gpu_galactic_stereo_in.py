"""`(l | r) >> Galactic` on the device: KNH_STAGE_GALACTIC with `input` / `input2` (knh_stage_desc) against
galactic_ref.Galactic.process(left, right), the numpy restatement tests/test_galactic_ref.py pins.  The left and right source
signals come from the CPU oracle, never from a GPU bank: one OracleBank over the stage-list prefix that ends at the node
output `input` names, one over the prefix that ends at `input2`'s (the sampler case: the per-plane oracle banks of
tests/stereo_reader_ref.py).  Source stages are SinWt, wr_mul, EnvAr and the BufferReader with `* value`: their oracle parity is
bit-exact.  Every case asserts max |want| < 1.0 on the restatement before it compares, as tests/test_gpu_galactic.py does.

Three source chains, each one run-time fusion per sample type: the two oscillators (TWO), the stereo sampler, and the mono
chain of test_gpu_galactic.py (`input == input2` naming the last stage IS the mono form).

Observed share of samples that are not bit-identical with detune = 0.7 (test_detune_within_tolerance prints it): see DESIGN.md,
"Galactic"."""
import numpy as np
import pytest

import galactic_ref as gr
import stereo_reader_ref as srr
from helpers import assert_bit_equal, fire_all, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage
from test_gpu_galactic import SRC, gal_ctor, settings, src_ctor
from test_gpu_galactic_paths import RATES, runs_of, settings_at

pytestmark = pytest.mark.gpu

SR = configs.SAMPLE_RATE
BOTH = (L.MIX_LEFT_FOLD, L.MIX_TREE)
# SinWt.wr_mul(amp) * EnvAr on the left, another one on the right
TWO = SRC + SRC
G = len(TWO)          # the Galactic stage
LEFT, RIGHT = 3, 6    # the prefixes that end at the node outputs `input = 3` and `input2 = 6` name
GAL = Stage(L.STAGE_GALACTIC, input=LEFT, input2=RIGHT)


def two_ctor(nv, amp_l=0.25, amp_r=0.25, sr=SR):
    """The burst of test_gpu_galactic.src_ctor on the left; on the right another oscillator, a third of a semitone up and
    more per voice, with a longer envelope."""
    c = src_ctor(nv, amp_l, sr)
    freq_r = c[0] * 2.0 ** (1.0 / 36.0) + 0.5 * np.arange(nv).reshape(nv, 1) * (sr / SR)
    return {0: c[0], 1: c[1], 2: c[2], 3: freq_r, 4: np.full((nv, 1), amp_r), 5: np.tile([40.0 / sr, 150.0 / sr], (nv, 1))}


def mix_of(want, mix_mode):
    if mix_mode == L.MIX_LEFT_FOLD:
        mix = want[:, 0].copy()
        for v in range(1, want.shape[1]):
            mix = mix + want[:, v]
        return mix
    return np.stack([pairwise_sum(want[0]), pairwise_sum(want[1])])


class StereoRig:
    """The GPU bank(s) on TWO + Galactic(input, input2), the oracle's two prefixes and the restatement, driven alike."""

    def __init__(self, knh, oracle, nv, st, bs, p, mixes=(L.MIX_LEFT_FOLD,), sr=SR, amp_l=0.25, amp_r=0.25):
        self.nv, self.bs, self.st = nv, bs, st
        self.dtype = np.float64 if st == L.F64 else np.float32
        ctor = two_ctor(nv, amp_l, amp_r, sr)
        self.gpu, self.mixes = [], list(mixes)
        for mix in mixes:
            b = knh.VoiceBank(TWO + [GAL], nv, st, 2, mix)
            for s, a in ctor.items():
                b.set_ctor_args(s, a)
            b.set_ctor_args(G, gal_ctor(p))
            b.init(sr, bs)
            self.gpu.append(b)
        self.left = oracle.OracleBank(TWO[:LEFT], nv, st, 1)
        self.right = oracle.OracleBank(TWO[:RIGHT], nv, st, 1)  # (a voice of two sources: its signal is the last stage's)
        for o, n in ((self.left, LEFT), (self.right, RIGHT)):
            for s in range(n):
                o.set_ctor_args(s, ctor[s])
            o.init(sr, bs)
        self.ref = self.new_ref(p, sr)
        self.peak = 0.0

    def new_ref(self, p, sr=SR):
        ref = gr.Galactic(self.nv, self.dtype, p["replace"], p["detune"], p["brightness"], p["bigness"], p["wet"],
                          p["fpd_l"].astype(np.uint32), p["fpd_r"].astype(np.uint32))
        ref.init(sr)
        return ref

    def source_call(self, stage, call):
        """call(bank) on every bank that holds `stage` of the source chain."""
        for b in self.gpu + ([self.left] if stage < LEFT else []) + [self.right]:
            call(b)

    def fire(self):
        for stage in (2, 5):
            self.source_call(stage, lambda b: fire_all(b, self.nv, stage, 2))

    def set_param(self, param, values, voices=None):
        v = np.arange(self.nv, dtype=np.uint32) if voices is None else np.asarray(voices, dtype=np.uint32)
        values = np.broadcast_to(np.asarray(values, dtype=np.float64), v.shape)
        for b in self.gpu:
            b.param_apply_many(v, G, param, L.VALUE_FLOAT, values)
        self.ref.set_param(param, values, voices=v)

    def sources(self):
        _, l, _, _ = self.left.process_block()
        _, r, _, _ = self.right.process_block()
        return np.asarray(l).reshape(self.nv, self.bs), np.asarray(r).reshape(self.nv, self.bs)

    def restate(self, l, r, ref=None):
        out_l, out_r = (ref or self.ref).process(l, r)
        want = np.stack([out_l, out_r])
        self.peak = max(self.peak, float(np.abs(want).max()))
        assert self.peak < 1.0, "the restatement's output must stay below 1.0: change the input, not the bound"
        return want

    def ref_block(self):
        return self.restate(*self.sources())

    def close(self):
        for b in self.gpu + [self.left, self.right]:
            b.close()


def check_block(rig, what, want=None):
    want = rig.ref_block() if want is None else want
    for b, mix_mode in zip(rig.gpu, rig.mixes):
        out, voices, _ = b.process_block_voices()
        assert voices.shape == (2, rig.nv, rig.bs)
        assert_bit_equal(voices, want, f"{what}: per-voice left/right")
        assert_bit_equal(out, mix_of(want, mix_mode), f"{what}: mix mode {mix_mode}")
    return want


@pytest.mark.parametrize("st", [L.F32, L.F64])
@pytest.mark.parametrize("bs,n_blocks", [(64, 24), (100, 16), (256, 12)])
def test_bit_exact_without_detune(knh, oracle, st, bs, n_blocks):
    """130 voices (two full wavefronts of the source kernel and a partial one), L != R, a re-trigger part-way through, both
    mix modes; settings() has the corners among its first voices: bigness 0 and 1, wet 1 and below, replace 1."""
    nv = 130
    p = settings(nv)
    assert p["bigness"][0] == 0.0 and p["bigness"][1] == 1.0 and p["wet"][2] == 1.0 and p["wet"][5] < 1.0 and p["replace"][4] == 1.0
    rig = StereoRig(knh, oracle, nv, st, bs, p, mixes=BOTH)
    loud, sides = 0.0, 0
    for k in range(n_blocks):
        if k % (n_blocks // 2) == 0:
            rig.fire()
        want = check_block(rig, f"block {k}")
        loud = max(loud, float(np.abs(want).max()))
        sides += int(np.count_nonzero(want[0] != want[1]))
    assert loud > 1e-3 and sides > want[0].size  # audible, and a left that is not the right
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
@pytest.mark.parametrize("silent", ["right", "left"])
def test_one_side_silent(knh, oracle, st, silent):
    """One input is an oscillator times 0.0: that side alone is below 1.18e-23 and takes its own dither floor.  A restatement
    fed the sounding signal on BOTH inputs (one test for both sides) renders something else -- asserted before the GPU is
    compared -- and the silent side's output is not zero."""
    nv, bs = 66, 96
    p = settings(nv, seed=4)
    amp = {"amp_l": 0.25, "amp_r": 0.0} if silent == "right" else {"amp_l": 0.0, "amp_r": 0.25}
    rig = StereoRig(knh, oracle, nv, st, bs, p, **amp)
    twin = rig.new_ref(p)  # the same reverbs, fed the sounding side twice
    rig.fire()
    side = 1 if silent == "right" else 0
    differs = nonzero = False
    for k in range(12):
        l, r = rig.sources()
        assert not np.any((r if silent == "right" else l) != 0)
        want = rig.restate(l, r)
        both = rig.restate(*((l, l) if silent == "right" else (r, r)), ref=twin)
        differs = differs or bool(np.any(want != both))
        nonzero = nonzero or bool(np.any(want[side] != 0))
        if k == 0:  # before any feedback has crossed over: the silent side's first samples are its own dither floor
            assert np.any(want[side][:, :8] != 0)
        check_block(rig, f"{silent} silent, block {k}", want)
    assert differs and nonzero
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_input_equals_input2_naming_the_last_stage(knh, oracle, st):
    """Bit-identical to the restatement fed the one signal twice, and to the mono spelling of the same chain."""
    nv, bs = 66, 96
    p = settings(nv, seed=9)
    banks = []
    for gal in (Stage(L.STAGE_GALACTIC, input=3, input2=3), Stage(L.STAGE_GALACTIC)):
        b = knh.VoiceBank(SRC + [gal], nv, st, 2, L.MIX_LEFT_FOLD)
        for s, a in src_ctor(nv).items():
            b.set_ctor_args(s, a)
        b.set_ctor_args(3, gal_ctor(p))
        b.init(SR, bs)
        fire_all(b, nv, 2, 2)
        banks.append(b)
    assert banks[0].debug_signature() == banks[1].debug_signature()
    src = oracle.OracleBank(SRC, nv, st, 1)
    for s, a in src_ctor(nv).items():
        src.set_ctor_args(s, a)
    src.init(SR, bs)
    fire_all(src, nv, 2, 2)
    ref = gr.Galactic(nv, np.float64 if st == L.F64 else np.float32, p["replace"], p["detune"], p["brightness"], p["bigness"], p["wet"],
                      p["fpd_l"].astype(np.uint32), p["fpd_r"].astype(np.uint32))
    ref.init(SR)
    for k in range(8):
        _, dry, _, _ = src.process_block()
        dry = np.asarray(dry).reshape(nv, bs)
        want = np.stack(ref.process(dry, dry))
        assert np.abs(want).max() < 1.0
        outs = [b.process_block_voices() for b in banks]
        assert_bit_equal(outs[0][1], want, f"block {k}: input == input2 against the restatement")
        assert_bit_equal(outs[0][1], outs[1][1], f"block {k}: input == input2 against the mono spelling")
        assert_bit_equal(outs[0][0], outs[1][0], f"block {k}: the mix")
    for b in banks + [src]:
        b.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_parameter_traffic_between_blocks(knh, oracle, st):
    """Calls to stages on the left only, on the right only, and to the reverb, between blocks."""
    nv, bs = 70, 128
    rig = StereoRig(knh, oracle, nv, st, bs, settings(nv, seed=2))
    v = np.arange(nv, dtype=np.uint32)
    freq = two_ctor(nv)
    rig.fire()
    for k in range(14):
        if k == 2:   # the left oscillator alone
            rig.source_call(0, lambda b: b.param_apply_many(v, 0, 0, L.VALUE_FLOAT, freq[0][:, 0] * 1.5))
        if k == 4:   # the right oscillator and its gain alone
            rig.source_call(3, lambda b: b.param_apply_many(v, 3, 0, L.VALUE_FLOAT, freq[3][:, 0] * 0.75))
            rig.source_call(4, lambda b: b.param_apply_many(v, 4, 0, L.VALUE_FLOAT, np.linspace(0.05, 0.3, nv)))
        if k == 5:   # the reverb: shrink (`position` of the long rings is left beyond the new length), wet across 1
            rig.set_param(3, 0.0)
            for vv, val in [(0, 0.5), (2, 0.999), (5, 1.0), (6, 0.0)]:
                rig.set_param(4, val, voices=[vv])
        if k == 7:
            rig.set_param(3, np.linspace(0.0, 1.0, nv))
            rig.set_param(0, 0.75, voices=np.arange(10, 40))
            rig.source_call(5, lambda b: fire_all(b, nv, 5, 2))  # the right envelope alone
        if k == 9:
            rig.set_param(2, np.linspace(1.0, 0.0, nv))
            rig.source_call(2, lambda b: fire_all(b, nv, 2, 2))  # the left envelope alone
        if k == 11:
            rig.set_param(3, 0.05)
        check_block(rig, f"block {k}")
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_a_launch_of_three_blocks_with_a_reverb_parameter_addressed_to_block_2(knh, oracle, st):
    nv, bs = 70, 128
    rig = StereoRig(knh, oracle, nv, st, bs, settings(nv, seed=5), mixes=(L.MIX_TREE,))
    g = rig.gpu[0]
    v = np.arange(nv, dtype=np.uint32)
    big = np.linspace(1.0, 0.0, nv)
    rig.fire()
    loud = 0.0
    for launch in range(2):
        g.param_apply_many(v, G, 3, L.VALUE_FLOAT, big, block_offset=2)   # param_apply_many_at: the reverb, block 2 of the launch
        g.param_apply_many(v, 5, 2, L.VALUE_TRIGGER, block_offset=1)      # ... and the right envelope at block 1
        many, _ = g.process_blocks(3)
        for k in range(3):
            if k == 1:
                fire_all(rig.right, nv, 5, 2)
            if k == 2:
                rig.ref.set_param(3, big)
            want = rig.ref_block()  # the restatement, block by block
            assert_bit_equal(many[k], mix_of(want, L.MIX_TREE), f"launch {launch} block {k}")
            loud = max(loud, float(np.abs(want).max()))
        big = big[::-1].copy()
    assert loud > 1e-3
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_a_block_rendered_as_two_partial_calls(knh, oracle, st):
    """frames_to_process / block_start_offset: 50 + 78 frames, compared with the restatement driven slice by slice."""
    nv, bs, cut = 70, 128, 50
    rig = StereoRig(knh, oracle, nv, st, bs, settings(nv, seed=6))
    g = rig.gpu[0]
    rig.fire()
    for k in range(4):
        l, r = rig.sources()
        want = np.concatenate([rig.restate(l[:, :cut], r[:, :cut]), rig.restate(l[:, cut:], r[:, cut:])], axis=2)
        part = np.zeros((2, bs), dtype=rig.dtype)
        g.process_block(cut, 0, out=part)
        assert_bit_equal(part[:, :cut], mix_of(want[:, :, :cut], L.MIX_LEFT_FOLD), f"block {k}: the first slice")
        out, voices, _ = g.process_block_voices(bs - cut, cut)
        assert_bit_equal(out[:, cut:], mix_of(want[:, :, cut:], L.MIX_LEFT_FOLD), f"block {k}: the second slice")
        assert_bit_equal(voices, want, f"block {k}: per-voice, both slices")
    assert rig.peak > 1e-3
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_stereo_sampler_through_the_reverb(knh, oracle, st):
    """stereo_reader_ref.STEREO (the two-channel reader, a MUL_CONST per channel) with Galactic behind its two MUL_CONSTs:
    the operands name stages whose inputs are the reader and its KNH_STAGE_FLAG_READER_CH1 companion."""
    nv, bs, gain = 65, 64, 0.25
    buffers = srr.make_stereo_buffers()
    ids = srr.spread_ids(nv)
    ctor = srr.stereo_ctor(nv)
    traffic = srr.stereo_traffic(nv, srr.lengths(buffers, ids))
    p = settings(nv, seed=7)
    stages = srr.STEREO + [Stage(L.STAGE_GALACTIC, input=3, input2=4)]
    banks = []
    for mix in BOTH:
        b = srr.stereo_bank(knh, nv, bs, st, buffers, ids, ctor, mix, stages=stages, outs=None, gain=gain, init=False)
        b.set_ctor_args(4, gal_ctor(p))
        b.init(SR, bs)
        banks.append(b)
    planes = srr.Planes(oracle, nv, bs, st, buffers, ids, ctor, traffic, gain=gain)
    ref = gr.Galactic(nv, np.float64 if st == L.F64 else np.float32, p["replace"], p["detune"], p["brightness"], p["bigness"], p["wet"],
                      p["fpd_l"].astype(np.uint32), p["fpd_r"].astype(np.uint32))
    ref.init(SR)
    loud, sides = 0.0, 0
    for k in range(srr.BLOCKS):
        dry, done = planes.step(k)
        want = np.stack(ref.process(dry[0], dry[1]))
        assert np.abs(want).max() < 1.0
        loud = max(loud, float(np.abs(want).max()))
        sides += int(np.count_nonzero(dry[0] != dry[1]))
        for b, mix in zip(banks, BOTH):
            traffic(k, b)
            out, voices, _ = b.process_block_voices()
            assert_bit_equal(voices, want, f"block {k}: per-voice left/right")
            assert_bit_equal(out, mix_of(want, mix), f"block {k}: mix mode {mix}")
            np.testing.assert_array_equal(b.read_done_frames(), done)  # done frames: the chain's in front of the reverb
    assert loud > 1e-3 and sides > 0
    planes.close()
    for b in banks:
        b.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_detune_within_tolerance(knh, oracle, st):
    """detune = 0.7, replace >= 0.5.  The absolute tolerance is the 1e-4 test_gpu_galactic.test_detune_within_tolerance derives
    for the mono form -- the device's f64 sin and the C library's may differ in the last place, which through
    F::new(position + offset) can only flip a rounding, <= 2^-15 * 0.5 on the interpolated sample, decaying under a loop gain
    <= 0.75 -- and it holds per side: each side has its own detune ring and interpolated read."""
    nv, bs = 66, 256
    rig = StereoRig(knh, oracle, nv, st, bs, settings(nv, seed=3, detune=0.7, replace_lo=0.5))
    rig.fire()
    differ = total = 0
    worst = 0.0
    for k in range(24):
        want = rig.ref_block()
        _, voices, _ = rig.gpu[0].process_block_voices()
        worst = max(worst, float(np.abs(voices.astype(np.float64) - want).max()))
        differ += int(np.count_nonzero(voices != want))
        total += want.size
    print(f"galactic stereo input detune=0.7 {'f64' if st else 'f32'}: {differ} of {total} samples not bit-identical "
          f"({differ / total:.3e}), worst |error| {worst:.3e}")
    assert worst <= 1e-4
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_algorithmic_bytes_count_the_second_staging_plane(knh, st):
    """One more plane of block_size samples written by the source chain and read by the reverb, beside what the mono form
    counts (before knh_bank_init the block size is not known: the count is the mono form's, tests/test_galactic_stereo_in_abi.py)."""
    nv, bs, word = 8, 64, 8 if st == L.F64 else 4
    b = knh.VoiceBank(TWO + [GAL], nv, st, 2)
    for s, a in two_ctor(nv).items():
        b.set_ctor_args(s, a)
    b.set_ctor_args(G, gal_ctor(settings(nv)))
    before = b.algorithmic_bytes_per_voice_block()
    b.init(SR, bs)
    after = b.algorithmic_bytes_per_voice_block()
    b.close()
    assert (after[0] - before[0], after[1] - before[1]) == (word * bs, word * bs)


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_short_runs(knh, oracle, st):
    """8 kHz: the shortest ring at bigness 0 is 12 samples, GalParams::run = 11 (tests/test_gpu_galactic_paths.py RATES)."""
    sr = 8000
    shortest, run0, run1, _ = RATES[sr]
    nv, bs = 8, 64
    rig = StereoRig(knh, oracle, nv, st, bs, settings_at(nv, sr, seed=22), mixes=BOTH, sr=sr)
    rig.fire()
    for k in range(8):
        check_block(rig, f"{sr} Hz block {k}")
        if k == 0:
            runs = runs_of(rig.ref)
            assert runs[0] == run0 < 64 and runs[1] == run1 and int(rig.ref.delays_left[3].delay_length[0]) == shortest
    assert rig.peak > 1e-3
    rig.close()
