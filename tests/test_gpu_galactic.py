"""KNH_STAGE_GALACTIC on the device (knaster_airwindows/src/galactic.rs:14-400) against tests/galactic_ref.py, the numpy
restatement pinned by tests/test_galactic_ref.py.  The chain is SinWt.wr_mul(amp) -> * EnvAr -> Galactic: a short burst (the
loop gain of the reverb is 1 - replace / 2: exactly 1, an endless tail, at replace = 0), the source's per-voice signal taken
from the CPU oracle and fed to the restatement.  Every case first asserts max |out| < 1.0 on the restatement's output: that
keeps the output dither's exponent at 0 and out of the reference's log2 corner.

Observed share of samples that are not bit-identical with detune > 0 (test_detune_within_tolerance prints it): see
DESIGN.md, "Galactic"."""
import numpy as np
import pytest

import galactic_ref as gr
from helpers import assert_bit_equal, fire_all, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

pytestmark = pytest.mark.gpu

SR = configs.SAMPLE_RATE
SRC = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_MUL_ENV_AR)]
G = 3  # the Galactic stage


def settings(nv, seed=1, detune=0.0, replace_lo=0.0):
    """Per-voice reverb settings spread over 0..1, the corners the issue names among the first voices; distinct seeds."""
    rng = np.random.default_rng(seed)
    p = {"replace": replace_lo + (1.0 - replace_lo) * rng.random(nv), "detune": np.full(nv, float(detune)), "brightness": rng.random(nv),
         "bigness": rng.random(nv), "wet": rng.random(nv)}
    if nv >= 8:
        p["bigness"][0], p["bigness"][1] = 0.0, 1.0
        p["wet"][2], p["wet"][0] = 1.0, 1.0
        p["replace"][3], p["replace"][4] = max(0.0, replace_lo), 1.0
        p["replace"][1] = 1.0
    p["fpd_l"] = (16386 + rng.integers(0, 2 ** 32 - 20000, nv)).astype(np.float64)
    p["fpd_r"] = (16386 + rng.integers(0, 2 ** 32 - 20000, nv)).astype(np.float64)
    assert len(set(p["fpd_l"])) == nv
    return p


def src_ctor(nv, amp=0.25, sr=SR):
    """The burst has the same shape in samples at every rate: 110 + 7 v Hz and 0.5 ms + 2 ms at 48 kHz."""
    freq = (110.0 + 7.0 * np.arange(nv)) * (sr / SR)
    return {0: freq.reshape(nv, 1), 1: np.full((nv, 1), amp), 2: np.tile([24.0 / sr, 96.0 / sr], (nv, 1))}  # 24 + 96 samples of burst


def gal_ctor(p):
    return np.stack([p[k] for k in ("replace", "detune", "brightness", "bigness", "wet", "fpd_l", "fpd_r")], axis=1)


class Rig:
    """The GPU bank(s), the oracle's source chain and the restatement, driven with identical calls.
    sr: the sample rate of all three.  src: another chain in front of the reverb, as (stages, {stage: ctor args}, (stage, param)
    of the trigger fire() sends); the default is SRC with src_ctor.  peak_limit: the bound ref_block asserts on the
    restatement's output (None: the case is about loud output)."""

    def __init__(self, knh, oracle, nv, st, bs, p, mixes=(L.MIX_LEFT_FOLD,), amp=0.25, sr=SR, src=None, peak_limit=1.0):
        self.nv, self.bs, self.sr = nv, bs, sr
        self.dtype = np.float64 if st == L.F64 else np.float32
        stages, ctor, self.trigger = src if src is not None else (SRC, src_ctor(nv, amp, sr), (2, 2))
        stages = list(stages)
        self.G = len(stages)  # the Galactic stage
        self.gpu, self.mixes = [], list(mixes)
        for mix in mixes:
            b = knh.VoiceBank(stages + [Stage(L.STAGE_GALACTIC)], nv, st, 2, mix)
            for s, a in ctor.items():
                b.set_ctor_args(s, a)
            b.set_ctor_args(self.G, gal_ctor(p))
            b.init(sr, bs)
            self.gpu.append(b)
        self.src = oracle.OracleBank(stages, nv, st, 1)
        for s, a in ctor.items():
            self.src.set_ctor_args(s, a)
        self.src.init(sr, bs)
        self.ref = gr.Galactic(nv, self.dtype, p["replace"], p["detune"], p["brightness"], p["bigness"], p["wet"],
                               p["fpd_l"].astype(np.uint32), p["fpd_r"].astype(np.uint32))
        self.ref.init(sr)
        self.peak, self.peak_limit = 0.0, peak_limit

    def fire(self):
        for b in self.gpu + [self.src]:
            fire_all(b, self.nv, *self.trigger)

    def inner(self, call):
        """call(bank) on every bank that holds the chain in front of the reverb: the GPU banks and the oracle's."""
        for b in self.gpu + [self.src]:
            call(b)

    def set_param(self, param, values, voices=None):
        """One of the reverb's parameters on the GPU banks (param_apply_many) and on the restatement."""
        v = np.arange(self.nv, dtype=np.uint32) if voices is None else np.asarray(voices, dtype=np.uint32)
        values = np.broadcast_to(np.asarray(values, dtype=np.float64), v.shape)
        for b in self.gpu:
            b.param_apply_many(v, self.G, param, L.VALUE_FLOAT, values)
        self.ref.set_param(param, values, voices=v)

    def ref_block(self):
        _, dry, _, _ = self.src.process_block()
        dry = np.asarray(dry).reshape(self.nv, self.bs)
        out_l, out_r = self.ref.process(dry, dry)
        want = np.stack([out_l, out_r])
        self.peak = max(self.peak, float(np.abs(want).max()))
        if self.peak_limit is not None:
            assert self.peak < self.peak_limit, "the restatement's output must stay below 1.0: change the input, not the bound"
        return want

    def close(self):
        for b in self.gpu + [self.src]:
            b.close()


def check_block(rig, what):
    want = rig.ref_block()
    for b, mix_mode in zip(rig.gpu, rig.mixes):
        out, voices, _ = b.process_block_voices()
        assert voices.shape == (2, rig.nv, rig.bs)
        assert_bit_equal(voices, want, f"{what}: per-voice left/right")
        if mix_mode == L.MIX_LEFT_FOLD:
            mix = want[:, 0].copy()
            for v in range(1, rig.nv):
                mix = mix + want[:, v]
        else:
            mix = np.stack([pairwise_sum(want[0]), pairwise_sum(want[1])])
        assert_bit_equal(out, mix, f"{what}: mix mode {mix_mode}")
    return want


@pytest.mark.parametrize("st", [L.F32, L.F64])
@pytest.mark.parametrize("bs,n_blocks", [(256, 70), (64, 24), (100, 16)])
def test_bit_exact_without_detune(knh, oracle, st, bs, n_blocks):
    """130 voices, every ring of every voice wraps at block 256 (70 * 256 = 17 920 > 16 565)."""
    nv = 130
    rig = Rig(knh, oracle, nv, st, bs, settings(nv), mixes=(L.MIX_LEFT_FOLD, L.MIX_TREE))
    loud = 0.0
    for k in range(n_blocks):
        if k % 29 == 0:
            rig.fire()
        loud = max(loud, float(np.abs(check_block(rig, f"block {k}")).max()))
    assert loud > 1e-3
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_parameter_traffic_between_blocks(knh, oracle, st):
    nv, bs = 70, 128
    p = settings(nv, seed=2)
    rig = Rig(knh, oracle, nv, st, bs, p, mixes=(L.MIX_LEFT_FOLD,))
    g = rig.gpu[0]
    v = np.arange(nv, dtype=np.uint32)
    rig.fire()

    def everywhere(param, values):
        values = np.broadcast_to(np.asarray(values, dtype=np.float64), (nv,))
        g.param_apply_many(v, G, param, L.VALUE_FLOAT, values)
        rig.ref.set_param(param, values)

    for k in range(40):
        if k == 3:   # shrink: `position` of the long rings is left beyond the new length
            everywhere(3, 0.0)
        if k == 5:
            everywhere(3, np.linspace(0.0, 1.0, nv))
        if k == 7:   # wet across 1, one voice at a time (param_apply)
            for vv, val in [(0, 0.5), (2, 0.999), (5, 1.0), (6, 0.0)]:
                g.param_apply(vv, G, 4, val)
                rig.ref.set_param(4, val, voices=[vv])
        if k == 9:   # one value for a range of voices
            g.param_apply_range(10, 40, G, 0, L.VALUE_FLOAT, 0.75)
            rig.ref.set_param(0, 0.75, voices=np.arange(10, 40))
            g.param_apply_range(20, 60, G, 2, L.VALUE_FLOAT, 0.125)
            rig.ref.set_param(2, 0.125, voices=np.arange(20, 60))
        if k == 11:
            everywhere(3, 0.3)
            rig.fire()
        if k == 12:
            everywhere(3, 1.0)
            everywhere(2, np.linspace(1.0, 0.0, nv))
        if k == 20:
            everywhere(3, 0.05)
        check_block(rig, f"block {k}")
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
@pytest.mark.parametrize("detune", [0.3, 0.7, 1.0])
def test_detune_within_tolerance(knh, oracle, st, detune):
    """The device's f64 sin and the C library's may differ in the last place; through F::new(position + offset) (<= 511, f32
    spacing 2^-15) that can only flip a rounding: <= 2^-15 * 0.5 = 1.5e-5 on the interpolated sample.  replace >= 0.5 (loop
    gain <= 0.75) lets such an error decay.  Tolerance 1e-4 absolute; the share of samples not bit-identical is printed."""
    nv, bs = 66, 256
    rig = Rig(knh, oracle, nv, st, bs, settings(nv, seed=3, detune=detune, replace_lo=0.5))
    rig.fire()
    differ = total = 0
    worst = 0.0
    for k in range(24):
        want = rig.ref_block()
        _, voices, _ = rig.gpu[0].process_block_voices()
        worst = max(worst, float(np.abs(voices.astype(np.float64) - want).max()))
        differ += int(np.count_nonzero(voices != want))
        total += want.size
    print(f"galactic detune={detune} {'f64' if st else 'f32'}: {differ} of {total} samples not bit-identical "
          f"({differ / total:.3e}), worst |error| {worst:.3e}")
    assert worst <= 1e-4
    rig.close()


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_silence_in(knh, oracle, st):
    """A source times 0.0: the input-dither branch; the output is the reverb of the fpd * 1.18e-17 floor."""
    nv, bs = 66, 96
    rig = Rig(knh, oracle, nv, st, bs, settings(nv, seed=4), amp=0.0)
    rig.fire()
    nonzero = False
    for k in range(12):
        nonzero = nonzero or bool(np.any(check_block(rig, f"block {k}") != 0))
    assert nonzero
    rig.close()


def gpu_only(knh, nv, st, bs, p, mix=L.MIX_TREE):
    b = knh.VoiceBank(SRC + [Stage(L.STAGE_GALACTIC)], nv, st, 2, mix)
    for s, a in src_ctor(nv).items():
        b.set_ctor_args(s, a)
    b.set_ctor_args(G, gal_ctor(p))
    b.init(SR, bs)
    fire_all(b, nv, 2, 2)
    return b


@pytest.mark.parametrize("st", [L.F32, L.F64])
def test_partial_blocks_and_many_blocks_per_launch(knh, st):
    nv, bs = 130, 256
    p = settings(nv, seed=5)
    a, b = gpu_only(knh, nv, st, bs, p), gpu_only(knh, nv, st, bs, p)
    for k in range(3):  # one block as 100 + 156 frames
        whole, _ = a.process_block()
        part = np.zeros_like(whole)
        b.process_block(100, 0, out=part)
        b.process_block(156, 100, out=part)
        assert_bit_equal(part, whole, f"partial calls, block {k}")
    a.close()
    b.close()
    a, b = gpu_only(knh, nv, st, bs, p), gpu_only(knh, nv, st, bs, p)
    v = np.arange(nv, dtype=np.uint32)
    big = np.linspace(1.0, 0.0, nv)
    for rounds in range(2):
        a.param_apply_many(v, G, 3, L.VALUE_FLOAT, big, block_offset=2)  # the reverb's parameters move at block 2 of the launch
        a.param_apply_many(v, 2, 2, L.VALUE_TRIGGER, block_offset=3)
        many, _ = a.process_blocks(4)
        for k in range(4):
            if k == 2:
                b.param_apply_many(v, G, 3, L.VALUE_FLOAT, big)
            if k == 3:
                b.param_apply_many(v, 2, 2, L.VALUE_TRIGGER)
            one, _ = b.process_block()
            assert_bit_equal(many[k], one, f"launch {rounds} block {k}")
        big = big[::-1].copy()
    assert np.abs(many).max() > 1e-4
    a.close()
    b.close()


def test_independence_at_size(knh, oracle):
    """2 048 voices x 512 frames x 8 blocks, f32 (1.1 GB of rings); 16 voices restated alone on the CPU."""
    nv, bs, n_blocks = 2048, 512, 8
    p = settings(nv, seed=6)
    try:
        g = gpu_only(knh, nv, L.F32, bs, p, L.MIX_LEFT_FOLD)
    except L.KnasterHipError as e:  # knh_bank_init asks hipMemGetInfo before it allocates the rings
        if "do not fit in device memory" not in str(e):
            raise
        pytest.skip(f"the rings of {nv} voices (1.1 GB) do not fit in the free device memory: {e}")
    pick = np.sort(np.random.default_rng(7).choice(nv, 16, replace=False))
    src = oracle.OracleBank(SRC, 16, L.F32, 1)
    for s, a in src_ctor(nv).items():
        src.set_ctor_args(s, a[pick])
    src.init(SR, bs)
    fire_all(src, 16, 2, 2)
    ref = gr.Galactic(16, np.float32, *(p[k][pick] for k in ("replace", "detune", "brightness", "bigness", "wet")),
                      p["fpd_l"][pick].astype(np.uint32), p["fpd_r"][pick].astype(np.uint32))
    ref.init(SR)
    for k in range(n_blocks):
        _, voices, _ = g.process_block_voices()
        _, dry, _, _ = src.process_block()
        dry = np.asarray(dry).reshape(16, bs)
        out_l, out_r = ref.process(dry, dry)
        want = np.stack([out_l, out_r])
        assert np.abs(want).max() < 1.0
        assert_bit_equal(voices[:, pick], want, f"block {k}: the picked voices")
    g.close()
    src.close()


def test_refusals_on_the_device_path(knh):
    nv, bs = 8, 64
    p = settings(nv, seed=8)
    a, b = gpu_only(knh, nv, L.F32, bs, p), gpu_only(knh, nv, L.F32, bs, p)
    a.process_block()
    b.process_block()
    for bad in (1.5, -0.01, float("nan")):
        with pytest.raises(L.KnasterHipError) as e:
            a.param_apply(1, G, 3, bad)
        assert e.value.status == L.ERR_OUT_OF_RANGE
    x, _ = a.process_block()
    y, _ = b.process_block()
    assert_bit_equal(x, y, "the block after a refused bigness")
    a.close()
    b.close()
    p["fpd_r"][3] = 0.0
    z = knh.VoiceBank(SRC + [Stage(L.STAGE_GALACTIC)], nv, L.F32, 2)
    for s, c in src_ctor(nv).items():
        z.set_ctor_args(s, c)
    z.set_ctor_args(G, gal_ctor(p))
    with pytest.raises(L.KnasterHipError) as e:
        z.init(SR, bs)
    assert "fpd" in str(e.value)
    z.close()
