"""OscWt on a pool of Wavetables (KNH_STAGE_FLAG_WAVETABLE on KNH_STAGE_SIN_WT; osc.rs:28-87, wavetable.rs:327-610) on the
device, against two references neither of which is the code under test:

  * tests/wavetable_ref.py, the reference's lines restated in numpy -- u32 phase arithmetic, the f32 threshold count, a
    table look-up; no floating-point arithmetic in the output path, so every comparison is bit for bit;
  * the plain SIN_WT path, which the oracle pins: a flagged stage on a Wavetable whose tables all equal
    NonAaWavetable::sine() is bit-identical to the unflagged stage in the same voice, in every kernel form a flagged voice
    takes (debug word 2 says which one ran)."""
from dataclasses import replace

import numpy as np
import pytest

import wavetable_ref as wr
from helpers import assert_bit_equal, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage
from test_gpu_kernel_form import ONE_FUSED, PIPE_FUSED, set_env

pytestmark = pytest.mark.gpu

WT = L.STAGE_FLAG_WAVETABLE
BS = 64
CASES = [(L.F32, 48000), (L.F64, 44100), (L.F32, 44100), (L.F64, 48000)]
IDS = ["f32-48000", "f64-44100", "f32-44100", "f64-48000"]


def np_type(sample_type):
    return np.float64 if sample_type == L.F64 else np.float32


def osc(flags=WT, **kw):
    return Stage(L.STAGE_SIN_WT, flags=flags, **kw)


# ---- against the numpy restatement ---------------------------------------------------------------------------------------------
def frequencies(dtype):
    """Every threshold, the next f32 above each, 0, a negative one, 20 000, 30 000 -- and, in an f64 bank, a double just
    above 32.0 that rounds to 32.0f (table 0).  An odd count, so that voice v on entry v % 2 meets every one on both entries."""
    up = np.nextafter(wr.THRESHOLDS, np.float32(np.inf))
    f = [float(t) for t in wr.THRESHOLDS] + [float(t) for t in up] + [0.0, -440.0, 20000.0, 30000.0]
    if dtype == np.float64:
        f.append(float(np.nextafter(np.float64(32.0), np.float64(64.0))))
        assert f[-1] > 32.0 and np.float32(f[-1]) == np.float32(32.0)
    if len(f) % 2 == 0:
        f.append(441.0)
    return np.array(f, dtype=np.float64)


def ramp_bank(knh, stages, n, sample_type, sample_rate, freq, stage=0, entry_of_voice=None, **kw):
    """A bank whose flagged stage `stage` has the two test entries -- 0: seventeen tables T[k][i] = k + i / 16384,
    1: one table -- voice v on entry v % 2, and the numpy bank that says what it must render."""
    dtype = np_type(sample_type)
    entries = [wr.ramp_tables(dtype), wr.single_table(dtype)]
    ids = (np.arange(n) % 2).astype(np.uint32) if entry_of_voice is None else entry_of_voice
    g = knh.VoiceBank(stages, n, sample_type, 1, L.MIX_TREE, **kw)
    assert g.add_wavetable(stage, entries[0]) == 0 and g.add_wavetable(stage, entries[1]) == 1
    assert g.wavetable_count(stage) == 2
    g.set_ctor_args(stage, np.asarray(freq, dtype=np.float64).reshape(n, 1))
    g.assign_wavetables(stage, np.arange(n, dtype=np.uint32), ids)
    return g, wr.OscWtBank(entries, ids, freq, sample_rate, dtype)


def check_block(g, want, what):
    out, voices, _ = g.process_block_voices()
    print(f"{what}: voices differing {int(np.count_nonzero(voices != want))} of {want.size}")
    assert_bit_equal(voices, want, f"{what} per-voice", strict_zero=True)
    assert_bit_equal(out[0], pairwise_sum(want), f"{what} tree mix")


@pytest.mark.parametrize("sample_type,sample_rate", CASES, ids=IDS)
def test_thresholds_parameters_reassignment_and_restart(knh, monkeypatch, sample_type, sample_rate):
    set_env(monkeypatch, {})
    set_read_path(monkeypatch, None)
    n = 197
    dtype = np_type(sample_type)
    fl = frequencies(dtype)
    v = np.arange(n, dtype=np.uint32)
    f0 = fl[v % len(fl)]
    g, ref = ramp_bank(knh, [osc()], n, sample_type, sample_rate, f0)
    g.init(sample_rate, BS)
    assert g.algorithmic_bytes_per_voice_block()[0] == (5 + BS) * dtype().itemsize  # five state words, one table sample per frame
    check_block(g, ref.render(BS), "block 0, every threshold")
    assert len(np.unique(wr.table_index(ref.freq))) == 17
    # a freq change across thresholds at a block boundary
    f1 = fl[(v + 5) % len(fl)]
    g.param_apply_many(v, 0, 0, L.VALUE_FLOAT, f1)
    ref.set_freq(v, f1)
    check_block(g, ref.render(BS), "block 1, new frequencies")
    # phase_offset (the cast saturates: a negative one is 0) and reset_phase
    a, r = v[v % 3 == 0], v[v % 5 == 0]
    po = np.array([0.25, -0.5, 1.5, 0.999])[np.arange(len(a)) % 4]
    g.param_apply_many(a, 0, 1, L.VALUE_FLOAT, po)
    g.param_apply_many(r, 0, 2, L.VALUE_TRIGGER)
    ref.set_phase_offset(a, po)
    ref.reset_phase(r)
    check_block(g, ref.render(BS), "block 2, phase_offset and reset_phase")
    # after init: the pool is closed, a new oscillator needs its constructor argument, the entries are the pool's
    for call, status in ((lambda: g.add_wavetable(0, wr.single_table(dtype)), L.ERR_INVALID_ARGUMENT),
                         (lambda: g.assign_wavetables(0, a, 1), L.ERR_INVALID_ARGUMENT),
                         (lambda: g.assign_wavetables(0, a, 2, ctor=100.0), L.ERR_OUT_OF_RANGE)):
        with pytest.raises(L.KnasterHipError) as e:
            call()
        assert e.value.status == status and g.wavetable_count(0) == 2
    check_block(g, ref.render(BS), "block 3, after refused calls")
    # assign_wavetables after init: a new OscWt on the other entry, phase 0, phase_offset 0, freq from ctor
    f3 = fl[(a + 11) % len(fl)]
    g.assign_wavetables(0, a, (1 - ref.entry[a]).astype(np.uint32), ctor=f3)
    ref.construct(a, 1 - ref.entry[a], f3)
    check_block(g, ref.render(BS), "block 4, reassigned")
    # restart_voices: a new node on the entry the voice has, from its constructor argument
    rs = v[v % 4 == 1]
    g.restart_voices(rs)
    ref.construct(rs)
    check_block(g, ref.render(BS), "block 5, restarted")
    g.param_apply_many(rs, 0, 0, L.VALUE_FLOAT, f1[rs])  # ... and the new nodes take parameters on their entry
    ref.set_freq(rs, f1[rs])
    check_block(g, ref.render(BS), "block 6")
    g.close()


@pytest.mark.parametrize("sample_type,lds,signature", [(L.F32, None, "g"), (L.F32, "0", "M"), (L.F64, None, "M")],
                         ids=["f32-lds", "f32-gather", "f64-gather"])
def test_a_bank_on_one_single_table_in_both_read_paths(knh, monkeypatch, sample_type, lds, signature):
    """One entry of one table for the whole bank: an f32 bank stages it to LDS (an f64 table is 128 KiB: gathered),
    KNH_WT_LDS=0 forces the gather.  Every frequency reads the one table; a reassignment to the same entry is a new node."""
    set_env(monkeypatch, {})
    set_read_path(monkeypatch, lds)
    n = 197
    dtype = np_type(sample_type)
    fl = frequencies(dtype)
    v = np.arange(n, dtype=np.uint32)
    table = wr.single_table(dtype)
    g = knh.VoiceBank([osc(delayed_changes_per_block=2)], n, sample_type, 1, L.MIX_TREE)
    assert g.add_wavetable(0, table) == 0
    g.set_ctor_args(0, fl[v % len(fl)].reshape(n, 1))
    g.init(44100, BS)
    assert g.debug_signature() == signature
    ref = wr.OscWtBank([table], np.zeros(n, dtype=np.uint32), fl[v % len(fl)], 44100, dtype)
    check_block(g, ref.render(BS), "block 0")
    f1 = fl[(v + 7) % len(fl)]
    g.param_apply_many(v, 0, 0, L.VALUE_FLOAT, f1, delays=17)
    g.param_apply_many(v[::3], 0, 1, L.VALUE_FLOAT, 0.3)
    ref.set_phase_offset(v[::3], 0.3)
    check_block(g, ref.render(BS, at_frame={17: lambda r: r.set_freq(v, f1)}), "block 1, freq at frame 17")
    a = v[1::4]
    g.assign_wavetables(0, a, 0, ctor=777.0 + a)
    ref.construct(a, 0, 777.0 + a)
    check_block(g, ref.render(BS), "block 2, new nodes on the same entry")
    g.restart_voices(v[::5])
    ref.construct(v[::5])
    check_block(g, ref.render(BS), "block 3, restarted")
    g.close()


def test_init_without_a_wavetable_is_refused(knh, monkeypatch):
    set_env(monkeypatch, {})
    set_read_path(monkeypatch, None)
    g = knh.VoiceBank([osc()], 70, L.F32, 1)
    with pytest.raises(L.KnasterHipError) as e:
        g.init(48000, BS)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "wavetable" in str(e.value).lower()
    g.add_wavetable(0, wr.single_table(np.float32))  # a refused init changes nothing: the bank can still be completed
    g.init(48000, BS)
    out, voices, _ = g.process_block_voices()
    assert_bit_equal(voices, np.full((70, BS), -1.0, dtype=np.float32), "freq 0: the table's first sample, held")
    g.close()


@pytest.mark.parametrize("sample_type,sample_rate", CASES[:2], ids=IDS[:2])
def test_sample_accurate_freq_change(knh, monkeypatch, sample_type, sample_rate):
    """WrPreciseTiming around the oscillator (delayed_changes_per_block = 2): a freq change across a threshold at frame 17 --
    table and increment change at that frame and not before -- and a phase_offset at frame 40 of the same block."""
    set_env(monkeypatch, {})
    n = 70
    v = np.arange(n, dtype=np.uint32)
    f0 = 20.0 + 45.0 * v  # tables 0 .. 10
    g, ref = ramp_bank(knh, [osc(delayed_changes_per_block=2)], n, sample_type, sample_rate, f0)
    g.init(sample_rate, BS)
    check_block(g, ref.render(BS), "block 0")
    f1 = f0 * 1.5 + 13.0
    assert np.count_nonzero(wr.table_index(f1.astype(np_type(sample_type))) != wr.table_index(f0.astype(np_type(sample_type)))) > n // 2
    g.param_apply_many(v, 0, 0, L.VALUE_FLOAT, f1, delays=17)
    g.param_apply_many(v[::2], 0, 1, L.VALUE_FLOAT, 0.375, delays=40)
    want = ref.render(BS, at_frame={17: lambda r: r.set_freq(v, f1), 40: lambda r: r.set_phase_offset(v[::2], 0.375)})
    check_block(g, want, "block 1, changes at frames 17 and 40")
    check_block(g, ref.render(BS), "block 2")
    g.close()


@pytest.mark.parametrize("sample_type,sample_rate", CASES[:2], ids=IDS[:2])
def test_smoothed_freq_ramp_across_thresholds(knh, monkeypatch, sample_type, sample_rate):
    """WrSmoothParams around the oscillator: a block-rate linear ramp of freq from 0 to 100 + v Hz over three blocks crosses
    32, 48, 72 (and 108): increment and table follow the ramp's value block by block."""
    set_env(monkeypatch, {})
    n = 70
    v = np.arange(n, dtype=np.uint32)
    g, ref = ramp_bank(knh, [osc(WT | L.STAGE_FLAG_SMOOTH_PARAMS)], n, sample_type, sample_rate, np.full(n, 500.0))
    g.init(sample_rate, BS)
    check_block(g, ref.render(BS), "block 0")
    seconds = 3.0 * BS / sample_rate
    end = 100.0 + v.astype(np.float64)
    g.param_apply_many(v, 0, 0, L.VALUE_SMOOTHING, seconds, 1)  # Linear(seconds) at Rate::BlockRate
    g.param_apply_many(v, 0, 0, L.VALUE_FLOAT, end)
    values = wr.smoothed_block_values(end, seconds, sample_rate, BS, 6)
    assert values[0].max() == 0.0 and values[5] is None
    seen = set()
    for k, val in enumerate(values):
        if val is not None:
            ref.set_freq(v, val)
        seen |= set(int(i) for i in wr.table_index(ref.freq))
        check_block(g, ref.render(BS), f"ramp block {k}")
    assert {0, 1, 2, 3} <= seen
    g.close()


@pytest.mark.parametrize("sample_type,sample_rate", CASES[:2], ids=IDS[:2])
def test_audio_rate_freq_from_a_bank_input(knh, monkeypatch, sample_type, sample_rate):
    """OscWt.ar_params() with the running signal on "freq" (KNH_STAGE_FLAG_AR_FREQ): a bank input ramp put through `* 1.0`
    sweeps 40 .. 120 Hz inside one block -- across 48, 72 and 108 -- then 100 .. 4 500: increment and table index per sample."""
    set_env(monkeypatch, {})
    n = 70
    dtype = np_type(sample_type)
    stages = [Stage(L.STAGE_INPUT), Stage(L.STAGE_MUL_CONST), osc(WT | L.STAGE_FLAG_AR_FREQ)]
    g, ref = ramp_bank(knh, stages, n, sample_type, sample_rate, np.zeros(n), stage=2, in_channels=1)
    g.set_ctor_args(0, np.zeros((n, 1)))
    g.set_ctor_args(1, np.ones((n, 1)))
    g.init(sample_rate, BS)
    assert g.debug_signature() == "Imk"
    for k, (lo, hi) in enumerate([(40.0, 120.0), (100.0, 4500.0), (-10.0, 33.0)]):
        ramp = np.linspace(lo, hi, BS).astype(dtype)
        if k == 0:
            assert len(np.unique(wr.table_index(ramp))) == 4
        g.set_input(ramp.reshape(1, BS))
        check_block(g, ref.render(BS, ar_freq=ramp), f"audio-rate block {k}")
    g.close()


# ---- against plain SIN_WT -------------------------------------------------------------------------------------------------------
def sine_pair(knh, stages, n, sample_type, ctor, sample_rate, n_tables, out_channels=2, connect=None, **kw):
    """[the bank with every KNH_STAGE_FLAG_WAVETABLE taken off, the bank as given with a sine Wavetable per flagged stage]:
    n_tables(stage) = 17 (seventeen equal tables) or 1."""
    dtype = np_type(sample_type)
    sine = wr.sine_table(dtype)
    banks = []
    for flagged in (False, True):
        st = list(stages) if flagged else [replace(s, flags=s.flags & ~WT) for s in stages]
        b = knh.VoiceBank(st, n, sample_type, out_channels, L.MIX_TREE, **kw)
        for s, a in ctor.items():
            b.set_ctor_args(s, a)
        for i, s in enumerate(stages):
            if flagged and s.flags & WT:
                assert b.add_wavetable(i, np.tile(sine, (17, 1)) if n_tables(i) == 17 else sine) == 0
        if connect:
            b.connect_outputs(*connect)
        b.init(sample_rate, BS)
        banks.append(b)
    return banks


def same_blocks(banks, traffic, n_blocks, want_form, what, per_voice=True):
    """Each bank in turn (two banks called alternately would ask each other's resident kernel to leave), then block by block."""
    res = []
    for b in banks:
        blocks = []
        for k in range(n_blocks):
            traffic(k, b)
            r = b.process_block_voices() if per_voice else b.process_block()
            blocks.append([np.array(x) for x in r[:2 if per_voice else 1]])
        res.append(blocks)
        forms = want_form if isinstance(want_form, tuple) else (want_form,)
        assert int(b.debug_words()[2]) in forms, (what, b.debug_signature(), b.debug_words()[:4])
    loud = 0.0
    for k in range(n_blocks):
        if per_voice:
            assert_bit_equal(res[1][k][1], res[0][k][1], f"{what} block {k} per-voice", strict_zero=True)
        assert_bit_equal(res[1][k][0], res[0][k][0], f"{what} block {k} mix", strict_zero=True)
        loud = max(loud, float(np.abs(res[0][k][0]).max()))
    assert loud > 1e-4, "a silent comparison shows nothing"
    assert int(banks[0].debug_words()[2]) == int(banks[1].debug_words()[2])


def c3_chain(n):
    w = configs.config("C3", n_voices=n, block_size=BS)
    st = list(w.stages)
    st[0] = osc(delayed_changes_per_block=2)
    st[3] = replace(st[3], delayed_changes_per_block=2)
    return st, w.ctor


def c3_traffic(n):
    v = np.arange(n, dtype=np.uint32)

    def traffic(k, b):
        if k == 0:
            b.param_apply_many(v, 3, 3, L.VALUE_TRIGGER)                                   # note on
        if k == 1:
            b.param_apply_many(v[::2], 0, 0, L.VALUE_FLOAT, 30.0 + 41.5 * v[::2], delays=17)  # freq, sample-accurate
            b.param_apply_many(v[1::3], 2, 0, L.VALUE_FLOAT, 900.0 + 5.0 * v[1::3])          # cutoff
        if k == 2:
            b.param_apply_many(v[::3], 0, 1, L.VALUE_FLOAT, 0.25)                           # phase_offset
            b.param_apply_many(v[::4], 3, 2, L.VALUE_TRIGGER, delays=5)                     # release at frame 5
            b.param_apply_many(v, 1, 0, L.VALUE_FLOAT, 0.01 + 0.0001 * v)                   # wr_mul
        if k == 3:
            b.param_apply_many(v[::5], 0, 2, L.VALUE_TRIGGER, delays=33)                    # reset_phase at frame 33
            b.param_apply_many(v[1::2], 0, 0, L.VALUE_FLOAT, 14012.6044921875)
    return traffic


W1 = {"KNH_JIT": "1", "KNH_PIPELINE": "0", "KNH_JIT_WAVES": "1"}
W4 = {"KNH_JIT": "1", "KNH_PIPELINE": "0", "KNH_JIT_WAVES": "4"}
PIPE = {"KNH_JIT": "1"}
# (switches, the form meant, tables of the sine Wavetable, KNH_WT_LDS): a bank whose one flagged stage plays a single f32 table
# stages it to LDS ('g' for 'M' in the signature) unless KNH_WT_LDS=0; seventeen tables are always gathered
FORM_ROWS = [(W1, ONE_FUSED, 17, None), (W1, ONE_FUSED, 1, None), (W4, ONE_FUSED, 1, None), (W4, ONE_FUSED, 1, "0"),
             (PIPE, PIPE_FUSED, 17, None), (PIPE, PIPE_FUSED, 1, None), (PIPE, PIPE_FUSED, 1, "0")]
FORM_IDS = ["one-wave-17", "one-wave-1-lds", "four-waves-1-lds", "four-waves-1-gather", "pipeline-17", "pipeline-1-lds", "pipeline-1-gather"]


def set_read_path(monkeypatch, lds):
    monkeypatch.delenv("KNH_WT_LDS", raising=False)
    if lds is not None:
        monkeypatch.setenv("KNH_WT_LDS", lds)


@pytest.mark.parametrize("env,form,n_tables,lds", FORM_ROWS, ids=FORM_IDS)
def test_c3_chain_equals_plain_sin_wt_in_every_fused_form(knh, monkeypatch, env, form, n_tables, lds):
    """[SIN_WT, WR_MUL, SVF, MUL_ENV_ASR] with parameter traffic and sample-accurate changes, KNH_JIT=1 so that both banks are
    fused: one wavefront per workgroup, four, the fused pipeline; both read paths."""
    set_env(monkeypatch, env)
    set_read_path(monkeypatch, lds)
    n = 197
    st, ctor = c3_chain(n)
    banks = sine_pair(knh, st, n, L.F32, ctor, 48000, lambda i: n_tables)
    assert [b.debug_signature() for b in banks] == ["WmSA", "gmSA" if n_tables == 1 and lds is None else "MmSA"]
    same_blocks(banks, c3_traffic(n), 4, form, f"C3 {env}")
    for b in banks:
        b.close()


@pytest.mark.parametrize("env,form,n_tables", [(PIPE, PIPE_FUSED, 17), (W1, ONE_FUSED, 17), (PIPE, PIPE_FUSED, 1)],
                         ids=["pipeline-gather", "one-wave-gather", "pipeline-lds"])
def test_c3_chain_on_a_resident_launch(knh, monkeypatch, env, form, n_tables):
    """The call the reference makes, knh_bank_process_block once per block: served by a resident kernel, the mixes equal."""
    set_env(monkeypatch, env)
    set_read_path(monkeypatch, None)
    monkeypatch.setenv("KNH_RESIDENT", "1")
    n = 197
    st, ctor = c3_chain(n)
    banks = sine_pair(knh, st, n, L.F32, ctor, 48000, lambda i: n_tables)
    assert banks[1].debug_signature() == ("gmSA" if n_tables == 1 else "MmSA")
    same_blocks(banks, c3_traffic(n), 6, form, f"resident {env}", per_voice=False)
    for b in banks:
        print("resident calls, launches:", b.resident_stats())
        assert b.resident_stats()[0] >= 1, b.resident_stats()
        b.close()


def freq_traffic(n, stages_with_freq):
    v = np.arange(n, dtype=np.uint32)

    def traffic(k, b):
        if k == 1:
            for s in stages_with_freq:
                b.param_apply_many(v[s % 2::2], s, 0, L.VALUE_FLOAT, 25.0 + 97.0 * v[s % 2::2])
        if k == 2:
            b.param_apply_many(v[::3], stages_with_freq[0], 1, L.VALUE_FLOAT, 0.6)
    return traffic


GRAPHS = {
    # two oscillators multiplied: each flagged stage has a pool of its own (seventeen equal tables / one)
    "product": ([osc(), osc(), Stage(L.STAGE_MATH_MUL, input=1, input2=2)], L.F64, None, [0, 1]),
    # an FM pair: the flagged stage is the carrier, its freq (ar_param = 1) is modulator * index + base, per sample
    "fm": ([Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST), osc(ar_param=1, input2=3)], L.F32, None, [0]),
    # two connected outputs: a flagged oscillator on each
    "stereo": ([osc(), Stage(L.STAGE_WR_MUL), osc(), Stage(L.STAGE_WR_MUL)], L.F64, (1, 3), [0, 2]),
}


def graph_ctor(name, n):
    v = np.arange(n, dtype=np.float64).reshape(n, 1)
    if name == "product":
        return {0: 110.0 + 13.0 * v, 1: 3.0 + 0.25 * v}
    if name == "fm":
        return {0: 50.0 + 7.0 * v, 1: 200.0 + 3.0 * v, 2: 300.0 + 40.0 * v, 3: np.zeros((n, 1))}
    return {0: 220.0 + 9.0 * v, 1: np.full((n, 1), 0.5), 2: 55.0 + 31.0 * v, 3: np.full((n, 1), 0.25)}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_graph_voices_equal_plain_sin_wt(knh, monkeypatch, name):
    # (KNH_INTERP=0: the plain twin of the product is oscillators and arithmetic alone and would run a lane per frame)
    set_env(monkeypatch, {"KNH_JIT": "1", "KNH_INTERP": "0"})
    n = 70
    stages, sample_type, connect, with_freq = GRAPHS[name]
    banks = sine_pair(knh, stages, n, sample_type, graph_ctor(name, n), 44100, lambda i: 17 if i == 0 else 1, connect=connect)
    assert "M" in banks[1].debug_signature() and "M" not in banks[0].debug_signature()
    same_blocks(banks, freq_traffic(n, with_freq), 3, ONE_FUSED, name)
    for b in banks:
        b.close()


def test_pan2_chain_equals_plain_sin_wt(knh, monkeypatch):
    """many_sines.rs' voice, (EnvAr * osc.wr_mul(amp)) >> Pan2, with the oscillator on a Wavetable: left and right per voice."""
    set_env(monkeypatch, {"KNH_JIT": "1"})
    n = 70
    w = configs.config("M1", n_voices=n, block_size=BS)
    st = [osc()] + list(w.stages[1:])
    banks = sine_pair(knh, st, n, L.F32, w.ctor, 48000, lambda i: 1)
    v = np.arange(n, dtype=np.uint32)

    def traffic(k, b):
        if k == 0:
            b.param_apply_many(v, *w.restart, L.VALUE_TRIGGER)
        if k == 1:
            b.param_apply_many(v[::2], 0, 0, L.VALUE_FLOAT, 60.0 + 101.0 * v[::2])
            b.param_apply_many(v[::3], 3, 0, L.VALUE_FLOAT, -0.5)
    same_blocks(banks, traffic, 3, (PIPE_FUSED, ONE_FUSED), "Pan2")
    for b in banks:
        b.close()


def test_host_sharded_bank_equals_plain_sin_wt(knh, monkeypatch):
    """knh_bank_create_sharded: two voice ranges, each with the whole pool; voices reassigned across the range boundary."""
    set_env(monkeypatch, {"KNH_JIT": "1"})
    n = 197
    st, ctor = c3_chain(n)
    banks = sine_pair(knh, st, n, L.F32, ctor, 48000, lambda i: 17, host_threads=2)
    assert banks[1].ranks() == 2 and banks[1].wavetable_count(0) == 1
    traffic = c3_traffic(n)
    v = np.arange(n, dtype=np.uint32)

    # odd voices on both sides of the range boundary (128) on which no delay is armed (c3_traffic arms them on even voices
    # and on every fifth): a new OscWt on entry 0 is, for plain SinWt, freq + phase_offset 0 + reset_phase
    sw = v[121:140:2]
    sw = sw[sw % 5 != 0]
    f = 333.0 + sw

    def with_swap(k, b):
        traffic(k, b)
        if k == 4 and b is banks[1]:
            b.assign_wavetables(0, sw, 0, ctor=f)
        elif k == 4:
            b.param_apply_many(sw, 0, 0, L.VALUE_FLOAT, f)
            b.param_apply_many(sw, 0, 1, L.VALUE_FLOAT, 0.0)
            b.param_apply_many(sw, 0, 2, L.VALUE_TRIGGER)
    same_blocks(banks, with_swap, 6, PIPE_FUSED, "sharded")
    for b in banks:
        b.close()
