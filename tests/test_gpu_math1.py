"""The six Math1UGen stages (ceil sqrt floor trunc fract exp: knaster_core_dsp/src/ugens/math.rs:167-305) in every voice form.

The oracle does not know these kinds, so expected values are composed: the oracle's output for the part of the voice in front
of the Math1 stage, the op itself in numpy at the bank's dtype (np.ceil, np.floor, np.trunc, x - np.trunc(x), np.sqrt: all
correctly rounded IEEE operations, like Rust's std), and -- for anything stateful behind it -- an oracle bank of ONE voice
[INPUT, ...rest] fed that signal block by block.  Five ops are compared bit for bit, the sign of a zero included; where the
expectation is a NaN the result must be a NaN (x86 and gfx950 make different default NaNs: sign and payload are not compared).
exp runs the device library: tolerance (test_exp_accuracy).

Everywhere: f32 and f64, blocks of 64 frames, 3 or 4 blocks, banks of 3, 64, 65 and 130 voices (a partial wavefront, a full
one, one lane over, a third wavefront)."""
import numpy as np
import pytest

from helpers import assert_bit_equal, bits, make_gpu, make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

pytestmark = pytest.mark.gpu

BS = 64
VOICE_COUNTS = (3, 64, 65, 130)
TYPES = [L.F32, L.F64]
MATH1 = {"ceil": 40, "sqrt": 41, "floor": 42, "trunc": 43, "fract": 44, "exp": 45}
EXACT = ["ceil", "sqrt", "floor", "trunc", "fract"]
# Largest distance, in units in the last place, between the device library's exp and the correctly rounded value, as
# test_exp_accuracy measured it on an MI355X (ROCm 7.2) over its 33 280 inputs per type: 1 ulp in f32 (2 144 of the inputs
# are not correctly rounded) and 1 ulp in f64 (2 792).  The test's bound is this plus one ulp (a point release of the device
# library may round the last place differently).
EXP_MEASURED_MAX_ULP = {L.F32: 1, L.F64: 1}


def dtype_of(sample_type):
    return np.float64 if sample_type == L.F64 else np.float32


def numpy_op(name, x):
    with np.errstate(all="ignore"):
        if name == "fract":
            return x - np.trunc(x)  # f32::fract: self - self.trunc()
        return getattr(np, name)(x)


def assert_bits_or_nan(got, want, what):
    """Bit for bit, the sign of zero included; a NaN where a NaN is expected (sign and payload not compared)."""
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{what}: a NaN is expected at {np.argwhere(nan & ~np.isnan(got))[:3].tolist()}"
    g, w = got.copy(), want.copy()
    g[nan] = 0
    w[nan] = 0
    assert_bit_equal(g, w, what, strict_zero=True)


def ulp_distance(got, want):
    """Units in the last place between finite values of one sign (consecutive floats have consecutive bit patterns)."""
    assert np.isfinite(got).all() and np.isfinite(want).all() and (np.signbit(got) == np.signbit(want)).all()
    return np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64))


def workload(name, stages, n, sample_type, ctor, in_channels=0):
    w = configs.Workload(name, stages, n, BS, sample_type, 1)
    w.ctor = {s: np.asarray(a, dtype=np.float64).reshape(n, -1) for s, a in ctor.items()}
    w.in_channels = in_channels
    return w


def run_voices(bank, blocks, inputs=None, before=None):
    """Per-voice signals of `blocks` consecutive blocks: [blocks, n_voices, BS].  bank: a VoiceBank or an OracleBank."""
    out = []
    for b in range(blocks):
        if before:
            before(b, bank)
        if inputs is not None:
            bank.set_input(inputs[b].reshape(1, BS))
        out.append(bank.process_block_voices()[1] if hasattr(bank, "process_block_voices") else bank.process_block()[1])
    return np.stack(out)


def through_oracle(oracle, rest, ctor_of_rest, signal, sample_type, before=None):
    """`signal` [blocks, BS] through the one-voice oracle bank [INPUT, *rest]: what a stateful tail makes of it."""
    w = workload("tail", [Stage(L.STAGE_INPUT)] + list(rest), 1, sample_type, {0: [0.0], **{s + 1: a for s, a in ctor_of_rest.items()}}, 1)
    o = make_oracle(oracle, w)
    out = run_voices(o, signal.shape[0], signal, before)[:, 0, :]
    o.close()
    return out


def special_inputs(sample_type):
    """One block of 64 inputs: signed zeros, halves on both sides of the rounding modes, the last odd half below 2^23 / 2^52 and
    that power itself, the ends of the subnormal range, the largest finite values, infinities, a NaN, arguments beyond exp's
    range, and ordinary values."""
    dt = dtype_of(sample_type)
    fi = np.finfo(dt)
    big = dt(2.0) ** (23 if dt == np.float32 else 52)
    v = [0.0, -0.0, 0.25, -0.25, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 1e6 + 0.5, -(1e6 + 0.5), big - dt(0.5), -(big - dt(0.5)), big, -big,
         fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny - fi.smallest_subnormal, -(fi.tiny - fi.smallest_subnormal), fi.tiny, -fi.tiny,
         fi.max, -fi.max, np.inf, -np.inf, np.nan, 89.5 if dt == np.float32 else 710.5, 7000.0, -7000.0]
    rng = np.random.default_rng(7)
    v += list(rng.uniform(-4.0, 4.0, 64 - len(v)))
    x = np.array(v, dtype=dt)
    assert x.shape == (64,) and x[10] == dt(1000000.5) and x[12] == big - dt(0.5) and x[12] != big and x[18] == np.nextafter(fi.tiny, dt(0))
    return x


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("name", list(MATH1))
def test_special_values(knh, oracle, monkeypatch, name, sample_type):
    """[INPUT, MUL_CONST c_v, MATH1_x] with c_v = 1, -1, 0.5, 3 by voice, in the whole-chain kernel (one wavefront runs the
    chain; KNH_JIT_PIPE=0): expected op(oracle [INPUT, MUL_CONST]).  exp: only what is exact about it -- exp(-inf) = 0,
    exp(+inf) = inf, NaN -> NaN, overflow -> inf, exp(+-0) = 1."""
    monkeypatch.setenv("KNH_JIT_PIPE", "0")
    dt = dtype_of(sample_type)
    x = special_inputs(sample_type)
    inputs = np.stack([np.roll(x, 5 * b) for b in range(3)])
    for n in VOICE_COUNTS:
        c = np.array([1.0, -1.0, 0.5, 3.0])[np.arange(n) % 4]
        head = [Stage(L.STAGE_INPUT), Stage(L.STAGE_MUL_CONST)]
        o = make_oracle(oracle, workload("head", head, n, sample_type, {0: np.zeros(n), 1: c}, 1))
        arg = run_voices(o, 3, inputs)
        o.close()
        g = make_gpu(knh, workload(name, head + [Stage(MATH1[name])], n, sample_type, {0: np.zeros(n), 1: c}, 1), L.MIX_LEFT_FOLD)
        got = run_voices(g, 3, inputs)
        assert g.debug_words()[2] == L.DEBUG_FORM_WHOLE_CHAIN_FUSED
        g.close()
        assert got.dtype == dt and arg.dtype == dt
        if name != "exp":
            assert_bits_or_nan(got, numpy_op(name, arg), f"{name} {dt.__name__} {n} voices")
            continue
        assert (got[arg == -np.inf] == 0).all() and (got[arg == np.inf] == np.inf).all() and np.isnan(got[np.isnan(arg)]).all()
        assert (got[arg > (89 if dt == np.float32 else 710)] == np.inf).all()
        assert_bit_equal(got[arg == 0], np.ones(np.count_nonzero(arg == 0), dtype=dt), "exp(+-0) = 1", strict_zero=True)
        assert np.count_nonzero(arg == 0) >= 6 and np.count_nonzero(arg > 700) >= 6 and np.isnan(arg).any()


@pytest.mark.parametrize("sample_type", TYPES)
def test_sqrt_is_correctly_rounded_from_the_smallest_subnormal_to_the_largest_finite(knh, sample_type):
    """[INPUT, MATH1_SQRT] over 64 x 4 log-spaced inputs, bit for bit against np.sqrt: the kernels hiprtc builds at init (this
    chain has no pre-built one; the pipelined form) keep the correctly rounded sequence, subnormal inputs included."""
    dt = dtype_of(sample_type)
    fi = np.finfo(dt)
    lo, hi = np.log2(float(fi.smallest_subnormal)), np.log2(float(fi.max))
    with np.errstate(over="ignore"):  # (f64: the last point, 2^1024, is replaced by the largest finite value below)
        x = np.exp2(np.linspace(lo, hi, 4 * BS)).astype(dt)
    x[0], x[-1] = fi.smallest_subnormal, fi.max
    assert (x > 0).all() and np.isfinite(x).all() and np.count_nonzero(x < fi.tiny) >= 5
    inputs = x.reshape(4, BS)
    for n in VOICE_COUNTS:
        g = make_gpu(knh, workload("sqrt", [Stage(L.STAGE_INPUT), Stage(L.STAGE_MATH1_SQRT)], n, sample_type, {0: np.zeros(n)}, 1), L.MIX_LEFT_FOLD)
        got = run_voices(g, 4, inputs)
        assert g.debug_words()[2] == L.DEBUG_FORM_PIPELINE_FUSED
        g.close()
        want = np.broadcast_to(np.sqrt(inputs)[:, None, :], got.shape)
        assert_bit_equal(got, want, f"sqrt {dt.__name__} {n} voices", strict_zero=True)


@pytest.mark.parametrize("n", VOICE_COUNTS)
@pytest.mark.parametrize("sample_type", TYPES)
def test_sqrt_of_subnormals_in_the_lane_per_frame_forms(knh, oracle, monkeypatch, sample_type, n):
    """The other build path: the interpreter (kernels_interp.hip) is compiled ahead of time with the library, the frame kernel at
    init.  SIN_WT -> MUL_CONST tiny -> MATH1_SQRT -> MUL_CONST huge is frame-eligible and hands sqrt nothing but subnormal
    inputs (and negative ones: NaN): both forms bit for bit against np.sqrt of the oracle's [SIN_WT, MUL_CONST]."""
    dt = dtype_of(sample_type)
    tiny, huge = (1e-40, 1e19) if dt == np.float32 else (1e-310, 1e150)
    p = configs.voice_parameters(n)
    head = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST)]
    o = make_oracle(oracle, workload("head", head, n, sample_type, {0: p["freq"], 1: np.full(n, tiny)}))
    arg = run_voices(o, 3)
    o.close()
    assert np.abs(arg).max() < np.finfo(dt).tiny and np.count_nonzero(arg > 0) > arg.size // 3  # subnormal, every one of them
    want = numpy_op("sqrt", arg) * dt(huge)
    for env, form in (("0", L.DEBUG_FORM_FRAME_INTERP), ("1", L.DEBUG_FORM_FRAME_JIT)):
        monkeypatch.setenv("KNH_FRAME_JIT", env)
        g = make_gpu(knh, workload("sub", head + [Stage(L.STAGE_MATH1_SQRT), Stage(L.STAGE_MUL_CONST)], n, sample_type,
                                   {0: p["freq"], 1: np.full(n, tiny), 3: np.full(n, huge)}), L.MIX_LEFT_FOLD)
        got = run_voices(g, 3)
        assert g.debug_words()[2] == form
        g.close()
        assert_bits_or_nan(got, want, f"sqrt of subnormals, KNH_FRAME_JIT={env}, {dt.__name__} {n} voices")


@pytest.mark.parametrize("sample_type", TYPES)
def test_exp_accuracy(knh, oracle, sample_type, capsys):
    """[INPUT, ADD_CONST d_v, MATH1_EXP]: the inputs are 256 points over [-87, 88] (f32) / [-700, 700] (f64) -- no true result
    is subnormal there -- shifted by a fraction of their spacing per voice, so that the 130 voices cover 33 280 points.
    Truth: np.exp in f64 (rounded to f32 for an f32 bank) of the oracle's [INPUT, ADD_CONST] signal.
    Measured on an MI355X (ROCm 7.2): the largest distance is 1 ulp in f32 and 1 ulp in f64 (with 130 voices, 2 144 and 2 792
    of the 33 280 results are one ulp off, the others correctly rounded); the bound is that plus one ulp.  The test prints what
    it measures per bank.  (The bound the project accepts for WR_POWF, 2e-6 absolute on values up to 2, is about 8 ulp.)"""
    dt = dtype_of(sample_type)
    lo, hi = (-87.0, 88.0) if dt == np.float32 else (-700.0, 700.0)
    grid = np.linspace(lo, hi, 4 * BS + 1)[:-1]
    step = grid[1] - grid[0]
    inputs = grid.astype(dt).reshape(4, BS)
    worst = 0
    for n in VOICE_COUNTS:
        head = [Stage(L.STAGE_INPUT), Stage(L.STAGE_ADD_CONST)]
        ctor = {0: np.zeros(n), 1: step * np.arange(n) / n}  # voice v renders the points v / n of the way to the next grid point
        o = make_oracle(oracle, workload("head", head, n, sample_type, ctor, 1))
        arg = run_voices(o, 4, inputs)
        o.close()
        g = make_gpu(knh, workload("exp", head + [Stage(L.STAGE_MATH1_EXP)], n, sample_type, ctor, 1), L.MIX_LEFT_FOLD)
        got = run_voices(g, 4, inputs)
        g.close()
        assert arg.min() >= lo and arg.max() <= hi  # no input is excluded
        truth = np.exp(arg.astype(np.float64)).astype(dt)
        assert (truth >= np.finfo(dt).tiny).all() and np.isfinite(truth).all()
        ulps = ulp_distance(got, truth)
        worst = max(worst, int(ulps.max()))
        with capsys.disabled():
            print(f"\n[exp accuracy] {dt.__name__} {n} voices: max {int(ulps.max())} ulp over {ulps.size} inputs, {np.count_nonzero(ulps)} not correctly rounded")
    assert worst <= EXP_MEASURED_MAX_ULP[sample_type] + 1, f"exp {dt.__name__}: {worst} ulp"


SUBSET = (0, 63, 64)


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("name,tail", [("floor", L.STAGE_SVF), ("fract", L.STAGE_ONEPOLE_LPF)])
def test_a_stateful_stage_behind_the_op(knh, oracle, name, tail, sample_type):
    """SIN_WT -> MUL_CONST 3 -> MATH1_FLOOR -> SVF(low), and the same with MATH1_FRACT and ONEPOLE_LPF, 65 voices with their
    own freq / cutoff / q: voices 0, 63 and 64 against an oracle bank [INPUT, filter] fed op(oracle [SIN_WT, MUL_CONST])."""
    n = 65
    p = configs.voice_parameters(n)
    svf = np.stack([np.full(n, float(L.SVF_LOW)), p["cutoff"], p["q"], np.zeros(n)], axis=1)
    tail_ctor = svf if tail == L.STAGE_SVF else p["cutoff"].reshape(n, 1)
    head = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST)]
    o = make_oracle(oracle, workload("head", head, n, sample_type, {0: p["freq"], 1: np.full(n, 3.0)}))
    mid = numpy_op(name, run_voices(o, 3))
    o.close()
    g = make_gpu(knh, workload(name, head + [Stage(MATH1[name]), Stage(tail)], n, sample_type, {0: p["freq"], 1: np.full(n, 3.0), 3: tail_ctor}), L.MIX_LEFT_FOLD)
    got = run_voices(g, 3)
    g.close()
    assert np.abs(got).max() > 1e-3
    for v in SUBSET:
        want = through_oracle(oracle, [Stage(tail)], {0: tail_ctor[v]}, mid[:, v, :], sample_type)
        assert_bit_equal(got[:, v, :], want, f"{name} -> filter, voice {v}", strict_zero=True)


def checked_voices(n):
    return sorted({0, 1, 62, 63, 64, 65, n // 2, n - 1} & set(range(n)))


@pytest.mark.parametrize("n", VOICE_COUNTS)
@pytest.mark.parametrize("sample_type", TYPES)
def test_graph_voice(knh, oracle, monkeypatch, sample_type, n):
    """A voice that is a graph: trunc of 4 a, plus b, shifted above zero, its square root read by two later stages --
    sqrt(trunc(4 a) + b + 5.5) * (0.5 * the same) -- fused into the lane-per-voice kernel (every stage of it could also run a
    lane per frame, test_lane_per_frame: KNH_INTERP=0 keeps it here).  Expected: numpy over the oracle's per-voice a * 4 and b."""
    monkeypatch.setenv("KNH_INTERP", "0")
    dt = dtype_of(sample_type)
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_SIN_WT),                       # 1 a, 2 b
          Stage(L.STAGE_MUL_CONST, input=1), Stage(L.STAGE_MATH1_TRUNC),       # 3 a * 4, 4 trunc
          Stage(L.STAGE_MATH_ADD, input=4, input2=2), Stage(L.STAGE_ADD_CONST),  # 5 trunc + b, 6 + 5.5
          Stage(L.STAGE_MATH1_SQRT),                                           # 7: read by 8 and 9
          Stage(L.STAGE_MUL_CONST, input=7), Stage(L.STAGE_MATH_MUL, input=7, input2=8)]
    fb = p["freq"] * p["fm_ratio"]
    g = make_gpu(knh, workload("graph", st, n, sample_type, {0: p["freq"], 1: fb, 2: np.full(n, 4.0), 5: np.full(n, 5.5), 7: np.full(n, 0.5)}), L.MIX_LEFT_FOLD)
    assert "@" in g.debug_signature() and "t@" in g.debug_signature() and "r@" in g.debug_signature()
    got = run_voices(g, 3)
    assert g.debug_words()[2] == L.DEBUG_FORM_WHOLE_CHAIN_FUSED
    g.close()
    oa = make_oracle(oracle, workload("a4", [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST)], n, sample_type, {0: p["freq"], 1: np.full(n, 4.0)}))
    ob = make_oracle(oracle, workload("b", [Stage(L.STAGE_SIN_WT)], n, sample_type, {0: fb}))
    a4, b = run_voices(oa, 3), run_voices(ob, 3)
    oa.close()
    ob.close()
    s6 = (np.trunc(a4) + b) + dt(5.5)
    r = np.sqrt(s6)
    want = r * (r * dt(0.5))
    assert want.dtype == dt and (s6 > 0).all() and len(np.unique(np.trunc(a4))) >= 7
    assert_bit_equal(got, want, f"graph voice {dt.__name__} {n} voices", strict_zero=True)


@pytest.mark.parametrize("n", VOICE_COUNTS)
@pytest.mark.parametrize("sample_type", TYPES)
def test_pipeline_form(knh, oracle, sample_type, n):
    """SIN_WT -> MATH1_FRACT -> SVF -> MUL_ENV_ASR -> MATH1_CEIL -> MUL_CONST: no pre-built kernel, long enough to be cut into
    stage groups -- the wave pipeline built at init.  Expected: oracle [SIN_WT], fract, a one-voice oracle [INPUT, SVF, MUL_ENV_ASR]
    (restarted before block 0, released before block 2), ceil, times the voice's constant."""
    dt = dtype_of(sample_type)
    p = configs.voice_parameters(n)
    svf = np.stack([np.full(n, float(L.SVF_LOW)), p["cutoff"], p["q"], np.zeros(n)], axis=1)
    env = np.stack([np.full(n, 0.001), np.full(n, 0.002)], axis=1)
    gain = 0.25 + np.arange(n) / 256.0
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MATH1_FRACT), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR), Stage(L.STAGE_MATH1_CEIL), Stage(L.STAGE_MUL_CONST)]

    def triggers(stage):
        def before(block, bank):
            if block == 0:
                bank.param_apply_many(np.arange(bank.n_voices, dtype=np.uint32), stage, 3, L.VALUE_TRIGGER)
            if block == 2:
                bank.param_apply_many(np.arange(bank.n_voices, dtype=np.uint32), stage, 2, L.VALUE_TRIGGER)
        return before
    g = make_gpu(knh, workload("pipe", st, n, sample_type, {0: p["freq"] * 8.0, 2: svf, 3: env, 5: gain}), L.MIX_LEFT_FOLD)
    assert g.debug_signature() == "WwSAcm"
    got = run_voices(g, 4, before=triggers(3))
    assert g.debug_words()[2] == L.DEBUG_FORM_PIPELINE_FUSED
    g.close()
    o = make_oracle(oracle, workload("osc", [Stage(L.STAGE_SIN_WT)], n, sample_type, {0: p["freq"] * 8.0}))
    osc = run_voices(o, 4)
    o.close()
    assert len(np.unique(got)) > 3 and np.abs(got).max() > 0.2
    for v in checked_voices(n):
        filtered = through_oracle(oracle, [Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)], {0: svf[v], 1: env[v]}, numpy_op("fract", osc[:, v, :]), sample_type,
                                  before=triggers(2))
        want = np.ceil(filtered) * dt(gain[v])
        assert_bit_equal(got[:, v, :], want, f"pipeline {dt.__name__} voice {v} of {n}", strict_zero=True)


@pytest.mark.parametrize("n", VOICE_COUNTS)
@pytest.mark.parametrize("sample_type", TYPES)
def test_lane_per_frame(knh, oracle, monkeypatch, sample_type, n):
    """sqrt(fract(4 a) + 1) * b, b = a second SinWt scaled to 0.7 so that the product stays within [-1, 1]: a lane per frame as
    the kernel built at init and as the interpreter (KNH_FRAME_JIT=0), and a lane per voice (a SAFETY_LIMITER behind it: not
    frame-eligible, and it changes nothing within [-1, 1]).  Three blocks -- the phases carry -- bit-identical to each other and
    to the composed expectation.  A second voice, exp(4 a): the two frame forms bit-identical, and within exp's bound."""
    dt = dtype_of(sample_type)
    p = configs.voice_parameters(n)
    fb = p["freq"] * p["fm_ratio"]
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_MATH1_FRACT), Stage(L.STAGE_ADD_CONST), Stage(L.STAGE_MATH1_SQRT),
          Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_MATH_MUL, input=5, input2=6)]
    ctor = {0: p["freq"], 1: np.full(n, 4.0), 3: np.full(n, 1.0), 5: fb, 6: np.full(n, 0.7)}
    got = {}
    for form, env, stages, want_form in (("frame", "1", st, L.DEBUG_FORM_FRAME_JIT), ("interp", "0", st, L.DEBUG_FORM_FRAME_INTERP),
                                         ("voice", "1", st + [Stage(L.STAGE_SAFETY_LIMITER)], L.DEBUG_FORM_WHOLE_CHAIN_FUSED)):
        monkeypatch.setenv("KNH_FRAME_JIT", env)
        g = make_gpu(knh, workload(form, stages, n, sample_type, ctor), L.MIX_LEFT_FOLD)
        got[form] = run_voices(g, 3)
        assert g.debug_words()[2] == want_form, form
        g.close()
    oa = make_oracle(oracle, workload("a4", [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST)], n, sample_type, {0: p["freq"], 1: np.full(n, 4.0)}))
    ob = make_oracle(oracle, workload("b", [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL)], n, sample_type, {0: fb, 1: np.full(n, 0.7)}))
    a4, b = run_voices(oa, 3), run_voices(ob, 3)
    oa.close()
    ob.close()
    want = np.sqrt(numpy_op("fract", a4) + dt(1.0)) * b
    assert np.abs(want).max() <= 1.0 and np.abs(want).max() > 0.5 and not np.isnan(want).any()
    for form in ("frame", "interp", "voice"):
        assert_bit_equal(got[form], want, f"lane per frame, {form}, {dt.__name__} {n} voices", strict_zero=True)
    # exp in a lane-per-frame voice
    ste = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_MATH1_EXP)]
    e = {}
    for form, env, want_form in (("frame", "1", L.DEBUG_FORM_FRAME_JIT), ("interp", "0", L.DEBUG_FORM_FRAME_INTERP)):
        monkeypatch.setenv("KNH_FRAME_JIT", env)
        g = make_gpu(knh, workload("exp" + form, ste, n, sample_type, {0: p["freq"], 1: np.full(n, 4.0)}), L.MIX_LEFT_FOLD)
        e[form] = run_voices(g, 3)
        assert g.debug_words()[2] == want_form, form
        g.close()
    assert_bit_equal(e["frame"], e["interp"], "exp: frame kernel against interpreter", strict_zero=True)
    truth = np.exp(a4.astype(np.float64)).astype(dt)
    assert int(ulp_distance(e["frame"], truth).max()) <= EXP_MEASURED_MAX_ULP[sample_type] + 1


@pytest.mark.parametrize("n", VOICE_COUNTS)
@pytest.mark.parametrize("sample_type", TYPES)
def test_exp_of_a_ramp_drives_an_oscillator_at_audio_rate(knh, oracle, sample_type, n):
    """PHASOR(2 Hz) -> MUL_CONST 1 -> MATH1_EXP -> MUL_CONST 220 .. drives SIN_WT freq (ar_param = 1, input2): a pitch envelope.
    The oscillator is bit-exact given its driver: an oracle voice [INPUT, SIN_WT | AR_FREQ] fed the GPU's own driver signal, read
    from a second bank that ends at the MUL_CONST (the driver itself: test_exp_accuracy).  (The oracle's voice has a `* 1.0`
    between the two, as the reference needs one: a parameter edge starts at a node, not at a graph input; it changes no bit.)"""
    drv = [Stage(L.STAGE_PHASOR), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_MATH1_EXP), Stage(L.STAGE_MUL_CONST)]
    scale = 220.0 * (1.0 + np.arange(n) / 64.0)
    ctor = {0: np.full(n, 2.0) + 40.0 * (np.arange(n) % 3), 1: np.full(n, 1.0), 3: scale}
    d = make_gpu(knh, workload("driver", drv, n, sample_type, ctor), L.MIX_LEFT_FOLD)
    driver = run_voices(d, 3)
    d.close()
    assert driver.min() >= 219.0 and driver.max() < 220.0 * 4.2 * np.e and len(np.unique(driver[:, 0, :])) > 100
    g = make_gpu(knh, workload("pitch", drv + [Stage(L.STAGE_SIN_WT, input2=4, ar_param=1)], n, sample_type, {**ctor, 4: np.full(n, 440.0)}), L.MIX_LEFT_FOLD)
    assert "%0" in g.debug_signature()
    got = run_voices(g, 3)
    g.close()
    assert np.abs(got).max() > 0.9
    for v in checked_voices(n):
        want = through_oracle(oracle, [Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_SIN_WT, flags=L.STAGE_FLAG_AR_FREQ)], {0: [1.0], 1: [440.0]}, driver[:, v, :], sample_type)
        assert_bit_equal(got[:, v, :], want, f"voice {v} of {n}", strict_zero=True)


@pytest.mark.parametrize("name", list(MATH1))
def test_refusals(knh, name):
    """What a stage without parameters cannot take is KNH_ERR_INVALID_ARGUMENT with a message, and launches nothing."""
    kind = MATH1[name]
    src = Stage(L.STAGE_SIN_WT)
    for bad in ([Stage(kind)], [src, src, Stage(kind, ar_param=1, input2=1)], [src, Stage(kind, delayed_changes_per_block=1)],
                [src, Stage(kind, flags=L.STAGE_FLAG_SMOOTH_PARAMS)]):
        with pytest.raises(L.KnasterHipError) as e:
            knh.VoiceBank(bad, 65, L.F32, 1)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and str(e.value).split(":", 1)[1].strip() not in ("", "unknown stage kind")
    g = make_gpu(knh, workload("ok", [src, Stage(L.STAGE_MUL_CONST), Stage(kind)], 65, L.F32, {0: np.full(65, 440.0), 1: np.full(65, 2.0)}))
    g.timing_reset(True)
    v = np.arange(65, dtype=np.uint32)
    for call in (lambda: g.param_apply(64, 2, 0, 1.0), lambda: g.param_apply(0, 2, 0, L.VALUE_TRIGGER),
                 lambda: g.param_apply_many(v, 2, 0, L.VALUE_FLOAT, np.ones(65)), lambda: g.param_apply_many(v[:3], 2, 0, L.VALUE_FLOAT, np.ones(3)),
                 lambda: g.param_apply_many(v, 2, 0, L.VALUE_FLOAT, np.ones(65), block_offset=1), lambda: g.param_apply_range(0, 65, 2, 0, L.VALUE_FLOAT, 1.0)):
        with pytest.raises(L.KnasterHipError) as e:
            call()
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "no parameters" in str(e.value)
    assert g.timing_read()[1] == 0  # nothing was launched
    g.process_block()                # and the bank is as it was: the next block renders
    assert g.timing_read()[1] == 1
    g.close()
    # the same answer from a bank cut into host shards and from a rank bank
    st = [src, Stage(L.STAGE_MUL_CONST), Stage(kind)]
    v = np.arange(130, dtype=np.uint32)
    for kw in ({"host_threads": 2}, {"rank": 0, "world": 1}):
        b = knh.VoiceBank(st, 130, L.F32, 1, L.MIX_TREE, -1, False, **kw)
        b.set_ctor_args(0, np.full((130, 1), 440.0))
        b.set_ctor_args(1, np.full((130, 1), 2.0))
        b.init(configs.SAMPLE_RATE, BS)
        for call in (lambda: b.param_apply(129, 2, 0, 1.0), lambda: b.param_apply_many(v, 2, 0, L.VALUE_FLOAT, np.ones(130)),
                     lambda: b.set_delay_within_block_for_param(1, 2, 0, 5)):
            with pytest.raises(L.KnasterHipError) as e:
                call()
            assert e.value.status == L.ERR_INVALID_ARGUMENT and "no parameters" in str(e.value), kw
        b.close()
