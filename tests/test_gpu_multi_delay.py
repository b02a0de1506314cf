"""Several delay stages per voice on the device: a ring per (delay stage, voice), the stages of a voice one after the other on
the wavefront's one RingLines tile.  Per voice bit for bit against the oracle (one node per stage: oracle/oracle_bank.hpp;
tests/test_multi_delay_abi.py pins it to an independent model), in f32 and f64, in every kernel form a delay chain takes.
The cases and their sizes: tests/multi_delay_cases.py."""
import numpy as np
import pytest

import multi_delay_cases as mc
import restart_cases as rc
from helpers import assert_bit_equal, make_gpu, make_oracle, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage
from test_gpu_ring_lines import FORMS as RING_FORMS

pytestmark = pytest.mark.gpu

FORM_ENVS = ("KNH_PIPELINE", "KNH_WIDE", "KNH_JIT", "KNH_JIT_PIPE", "KNH_JIT_WAVES", "KNH_RESIDENT", "KNH_HOST_THREADS")
# the pre-built forms of tests/test_gpu_ring_lines.py and the two fused at init, each with the form the bank must report
FORMS = {name: (env, {"one": L.DEBUG_FORM_WHOLE_CHAIN, "four": L.DEBUG_FORM_MANY_WAVE, "eight": L.DEBUG_FORM_MANY_WAVE,
                      "pipeline": L.DEBUG_FORM_PIPELINE}[name]) for name, env in RING_FORMS.items()}
FORMS["fused_pipeline"] = ({"KNH_JIT": "1"}, L.DEBUG_FORM_PIPELINE_FUSED)
FORMS["fused_one_wavefront"] = ({"KNH_JIT": "1", "KNH_JIT_PIPE": "0"}, L.DEBUG_FORM_WHOLE_CHAIN_FUSED)
V = np.arange(mc.N, dtype=np.uint32)
KF = L.VALUE_FLOAT


def set_env(monkeypatch, env):
    for k in FORM_ENVS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def left_fold(rows):
    acc = rows[0].copy()
    for k in range(1, rows.shape[0]):
        acc = acc + rows[k]
    return acc


# ---- 1. three delays in series, every form ----------------------------------------------------------------------------------
def _series(knh, oracle, monkeypatch, form, sample_type, bs):
    env, want_form = FORMS[form]
    set_env(monkeypatch, env)
    exp = mc.series_expected(oracle, sample_type, bs)
    g = make_gpu(knh, mc.series_workload(sample_type, bs), L.MIX_LEFT_FOLD)
    assert g.debug_words()[2] == want_form, (g.debug_words()[2], want_form, g.debug_signature())
    for b in range(mc.series_blocks(bs)):
        mc.series_events(b, g, bs)
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, exp[b], f"series {form} bs={bs} block {b} per voice")
        assert_bit_equal(out[0], left_fold(exp[b]), f"series {form} bs={bs} block {b} left-fold mix")
    assert max(np.abs(e).max() for e in exp[-3:]) > 1e-3
    g.close()


@pytest.mark.parametrize("sample_type,bs", [(L.F32, 64), (L.F32, 100), (L.F64, 64), (L.F64, 100)])
@pytest.mark.parametrize("form", list(RING_FORMS))
def test_three_delays_in_series_in_every_prebuilt_form(knh, oracle, monkeypatch, form, sample_type, bs):
    """SinWt.wr_mul -> SampleDelay -> AllpassFeedbackDelay -> AllpassDelay -> x const, ring lengths different per stage and
    per voice group; a delay_time change to one stage at a time, a feedback change, a sample-accurate change per voice to one of
    its delays, one voice group with delays shorter than a tile."""
    _series(knh, oracle, monkeypatch, form, sample_type, bs)


@pytest.mark.parametrize("sample_type,bs", [(L.F32, 64), (L.F64, 100)])
@pytest.mark.parametrize("form", ["fused_pipeline", "fused_one_wavefront"])
def test_three_delays_in_series_fused_at_init(knh, oracle, monkeypatch, form, sample_type, bs):
    _series(knh, oracle, monkeypatch, form, sample_type, bs)


# ---- 2. identity without the oracle, 4. neighbours ----------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_two_sample_delays_equal_one_of_the_sum(knh, oracle, monkeypatch, sample_type):
    """SampleDelay(d1) -> SampleDelay(d2) is, bit for bit, the one-delay bank with d1 + d2 -- d = 0, d = the ring length and
    rings of one sample included.  A delay of the whole ring reads the sample just written (delay.rs:38-40 takes the index
    modulo the length): in the sum it counts as the delay it is, none.
    Every voice has a frequency and two ring lengths of its own, and is held to the oracle per voice as well: a ring that
    overlapped a neighbour's -- another voice's or the other stage's -- would show in one of them.  (The ring allocation
    itself is not reachable from outside the library: no entry point hands out its address, and this work adds none.)"""
    set_env(monkeypatch, {"KNH_PIPELINE": "0"})
    bs, blocks = 64, 12
    two, one, d1, d2 = mc.identity_workloads(sample_type, bs)
    ring1 = np.floor(two.ctor[2][:, 0] * mc.SR).astype(np.int64)
    ring2 = np.floor(two.ctor[3][:, 0] * mc.SR).astype(np.int64)
    a, b, o = make_gpu(knh, two, L.MIX_LEFT_FOLD), make_gpu(knh, one, L.MIX_LEFT_FOLD), make_oracle(oracle, two, want_mix=False)
    for bank in (a, o):
        bank.param_apply_many(V, 2, 0, KF, mc.delay_seconds(d1))
        bank.param_apply_many(V, 3, 0, KF, mc.delay_seconds(d2))
    b.param_apply_many(V, 2, 0, KF, mc.delay_seconds(d1 % ring1 + d2 % ring2))
    peak = 0.0
    for k in range(blocks):
        va, vb, vo = a.process_block_voices()[1], b.process_block_voices()[1], o.process_block()[1]
        assert_bit_equal(va, vb, f"block {k}: two delays against one of the sum")
        assert_bit_equal(va, vo, f"block {k}: two delays against the oracle, per voice")
        peak = max(peak, float(np.abs(va).max()))
    assert peak > 1e-4
    for bank in (a, b, o):
        bank.close()


# ---- 3. graph voices ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type,bs", [(L.F32, 64), (L.F64, 100)])
def test_two_delays_in_parallel_joined_by_an_add(knh, oracle, monkeypatch, sample_type, bs):
    set_env(monkeypatch, {})
    w = mc.parallel_workload(sample_type, bs)
    g, o = make_gpu(knh, w, L.MIX_LEFT_FOLD), make_oracle(oracle, w, want_mix=False)
    assert g.debug_words()[2] == L.DEBUG_FORM_WHOLE_CHAIN_FUSED
    for b in range(10):
        for bank in (g, o):
            mc.parallel_events(b, bank)
        assert_bit_equal(g.process_block_voices()[1], o.process_block()[1], f"parallel bs={bs} block {b} per voice")
    g.close()
    o.close()


@pytest.mark.parametrize("sample_type,bs", [(L.F32, 64), (L.F64, 100)])
def test_two_delays_connected_to_outputs_0_and_1(knh, oracle, monkeypatch, sample_type, bs):
    """The same two delays as the voice's left and right signals (knh_bank_connect_outputs): each plane against the oracle's
    voice cut after that delay."""
    set_env(monkeypatch, {})
    w = mc.parallel_workload(sample_type, bs, connected=True)
    g = knh.VoiceBank(w.stages, mc.N, sample_type, 2, L.MIX_TREE)
    for s, a in w.ctor.items():
        g.set_ctor_args(s, a)
    g.connect_outputs(2, 3)
    g.init(configs.SAMPLE_RATE, bs)
    views = []
    for cut in (3, 4):
        o = oracle.OracleBank(w.stages[:cut], mc.N, sample_type, 1, False, True)
        for s, a in w.ctor.items():
            if s < cut:
                o.set_ctor_args(s, a)
        o.init(configs.SAMPLE_RATE, bs)
        views.append(o)

    class Both:  # a call goes to the bank and to each view that holds its stage
        def param_apply_many(self, voices, stage, param, kind, fvalues=None):
            for t in [g] + [o for o in views if stage < len(o.stages)]:
                t.param_apply_many(voices, stage, param, kind, fvalues)
    for b in range(10):
        mc.parallel_events(b, Both())
        want = np.stack([o.process_block()[1] for o in views])
        out, planes, _ = g.process_block_voices()
        assert_bit_equal(planes, want, f"connected bs={bs} block {b}: per-voice planes (left, right)")
        assert_bit_equal(out, np.stack([pairwise_sum(p) for p in want]), f"connected bs={bs} block {b}: the mix of each plane")
    g.close()
    for o in views:
        o.close()


@pytest.mark.parametrize("sample_type,n", [(L.F32, 130), (L.F64, 66)])
def test_a_voice_of_twelve_delays(knh, oracle, monkeypatch, sample_type, n):
    """Freeverb's mono topology: eight feedback delays in parallel, summed, four allpass delays in series."""
    set_env(monkeypatch, {})
    bs = 64
    w, delays = mc.twelve_workload(sample_type, bs, n)
    g, o = make_gpu(knh, w, L.MIX_LEFT_FOLD), make_oracle(oracle, w, want_mix=False)
    for b in range(10):
        for bank in (g, o):
            mc.twelve_events(b, bank, w, delays)
        vg, vo = g.process_block_voices()[1], o.process_block()[1]
        assert_bit_equal(vg, vo, f"twelve delays, block {b} per voice")
    assert np.abs(vo).max() > 1e-4
    g.close()
    o.close()


# ---- 5. restart ---------------------------------------------------------------------------------------------------------------
def _two_rings(sample_type, name):
    """SinWt -> SampleDelay -> AllpassFeedbackDelay, rings of 259 and 192 samples (strides of 288 and 192), delays of 100 and
    90.5; restarted after both rings have wrapped, the new nodes with shorter rings (240 and 144 samples)."""
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_SAMPLE_DELAY), Stage(L.STAGE_ALLPASS_FB_DELAY)]
    a = {0: rc.P["freq"], 1: np.full(rc.N, 0.0054), 2: np.full(rc.N, 0.004)}
    b = {0: rc.P["freq"] * 0.61 + 40.0, 1: np.full(rc.N, 0.005), 2: np.full(rc.N, 0.003)}

    def setup(bank, **kw):
        bank.param_apply_many(rc.V, 1, 0, KF, np.full(rc.N, 100.25 / mc.SR), **kw)
        bank.param_apply_many(rc.V, 2, 0, KF, np.full(rc.N, 90.5 / mc.SR), **kw)
        bank.param_apply_many(rc.V, 2, 1, KF, np.full(rc.N, 0.5), **kw)

    def pre(bank, block, **kw):
        if block == 0:
            setup(bank, **kw)

    def post(bank, j, role, **kw):
        if j == 0:
            setup(bank, **kw)  # (a new node's delay is 0, its feedback too)
    return rc.Case(name, st, sample_type, 64, a, b, 6, 3, pre, rc._none, post,
                   r_sets={"straddle": rc.R_SETS["straddle"], "last": rc.R_SETS["last"], "all": rc.R_SETS["all"]})


TWO_RINGS = {L.F32: _two_rings(L.F32, "two_rings_f32"), L.F64: _two_rings(L.F64, "two_rings_f64")}


@pytest.mark.parametrize("rname", ["straddle", "last", "all"])
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_restarted_voices_get_both_rings_zeroed_and_nothing_else(knh, oracle, monkeypatch, sample_type, rname):
    """After the rings have wrapped the restarted voices equal a fresh bank (both rings zero); voices 62, 65 and 128 beside
    them -- and every other -- equal the continuing bank."""
    set_env(monkeypatch, {})
    case = TWO_RINGS[sample_type]
    exp = rc.build_expected(case, rname, lambda w: make_oracle(oracle, w, want_mix=False), rc.oracle_step)
    r = sorted(set(case.r_sets[rname]))
    assert any(not np.array_equal(c[r], f[r]) for c, f in zip(exp.cont, exp.fresh))  # the premise: a restart shows on R
    g = case.make_gpu(knh, case.ctor_a, L.MIX_LEFT_FOLD)
    for b in range(case.k):
        case.pre(g, b)
        assert_bit_equal(g.process_block_voices()[1], exp.before[b][0], f"{case.name}/{rname} block {b}")
    case.restart(g, rname)
    for j in range(case.n_after):
        case.post(g, j, "gpu")
        assert_bit_equal(g.process_block_voices()[1], exp.after[j][0], f"{case.name}/{rname} block k+{j}")
    g.close()


def test_a_ring_longer_than_its_own_stages_stride_is_refused(knh, monkeypatch):
    """The second delay's rings were allocated 192 samples apart: a new max_delay of 216 samples for it is KNH_ERR_OUT_OF_RANGE
    and changes nothing, although the first delay's rings (288 apart) would hold it; for the first delay it is accepted."""
    set_env(monkeypatch, {})
    case = TWO_RINGS[L.F32]
    g, twin = case.make_gpu(knh, case.ctor_a), case.make_gpu(knh, case.ctor_a)
    for b in range(3):
        for bank in (g, twin):
            case.pre(bank, b)
            bank.process_block()
    r = np.array([63, 64], dtype=np.uint32)
    with pytest.raises(L.KnasterHipError) as e:
        g.set_voice_ctor_args(2, r, [[0.004], [0.0045]])
    assert e.value.status == L.ERR_OUT_OF_RANGE
    g.restart_voices(r)  # nothing of the refused call was kept: both banks restart with arguments A
    twin.restart_voices(r)
    for bank in (g, twin):
        case.post(bank, 0, "gpu")
    for k in range(3):
        x, y = g.process_block_voices(), twin.process_block_voices()
        assert_bit_equal(x[1], y[1], f"block {k} after the refusal, per voice")
    g.set_voice_ctor_args(1, r, [[0.0045], [0.0045]])  # 216 samples: within the first delay's 288
    g.close()
    twin.close()


# ---- 6. launch shapes ------------------------------------------------------------------------------------------------------------
def test_two_launches_of_four_blocks_equal_eight_single_blocks(knh, monkeypatch):
    set_env(monkeypatch, {})
    bs = 64
    runs = []
    for many in (False, True):
        g = make_gpu(knh, mc.series_workload(L.F32, bs))
        blocks = []
        for launch in range(2):
            if many:
                for i in range(4):
                    mc.series_events(4 * launch + i, _AtOffset(g, i), bs)
                blocks += list(g.process_blocks(4)[0])
            else:
                for i in range(4):
                    mc.series_events(4 * launch + i, g, bs)
                    blocks.append(g.process_block()[0].copy())
        runs.append(np.stack(blocks))
        g.close()
    assert np.abs(runs[0]).max() > 1e-4
    assert_bit_equal(runs[1], runs[0], "process_blocks(4) twice against eight single blocks")


class _AtOffset:
    """The calls of block `offset` of the coming launch."""

    def __init__(self, bank, offset):
        self.bank, self.offset = bank, offset

    def param_apply_many(self, voices, stage, param, kind, fvalues=None, delays=None):
        self.bank.param_apply_many(voices, stage, param, kind, fvalues, None, delays, block_offset=self.offset)


def test_the_per_block_call_on_a_resident_kernel(knh, monkeypatch):
    bs = 64
    runs = {}
    for resident in ("1", "0"):
        set_env(monkeypatch, {"KNH_RESIDENT": resident})
        g = make_gpu(knh, mc.series_workload(L.F32, bs))
        blocks = []
        for b in range(8):
            mc.series_events(b, g, bs)
            blocks.append(g.process_block()[0].copy())
        runs[resident] = (np.stack(blocks), g.resident_stats())
        g.close()
    assert_bit_equal(runs["1"][0], runs["0"][0], "resident against a launch per call")
    assert runs["0"][1] == (0, 0) and runs["1"][1][0] > 0, (runs["0"][1], runs["1"][1])


# ---- 7. ranges -------------------------------------------------------------------------------------------------------------------
def _no_reduce(_user, buf, count, sample_type, root, stream):
    return 0


@pytest.mark.parametrize("kw", [{"host_threads": 2}, {"devices": [0, 0]}, {"rank": 0, "world": 1, "reduce_fn": _no_reduce}],
                         ids=["host_threads_2", "two_ranges_one_device", "rank_0_of_1"])
def test_banks_of_several_ranges_allocate_their_own_rings(knh, oracle, monkeypatch, kw):
    """128 + 2 voices: the range boundary lies inside the third wavefront.  The same blocks as the one-range bank (and, where
    the bank hands out per-voice rows, the oracle's voices)."""
    set_env(monkeypatch, {})
    bs, sample_type = 64, L.F32
    exp = mc.series_expected(oracle, sample_type, bs)
    outs = []
    for bank_kw in ({}, kw):
        g = make_gpu(knh, mc.series_workload(sample_type, bs), L.MIX_TREE, **bank_kw)
        if "host_threads" in bank_kw or "devices" in bank_kw:
            assert g.ranks() == 2
        blocks = []
        for b in range(8):
            mc.series_events(b, g, bs)
            if "rank" in bank_kw:  # (a rank bank hands out no per-voice rows)
                blocks.append(g.process_block()[0].copy())
            else:
                out, voices, _ = g.process_block_voices()
                assert_bit_equal(voices, exp[b], f"{bank_kw} block {b} per voice")
                blocks.append(out.copy())
        outs.append(np.stack(blocks))
        g.close()
    assert_bit_equal(outs[1], outs[0], f"{kw} against one range")
