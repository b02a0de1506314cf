"""Several delay stages per voice, on a machine without a GPU.

The C ABI: knh_bank_create (which needs no device) accepts chains and graph voices of up to KNH_MAX_DELAY_STAGES delay stages
and refuses one more with KNH_ERR_UNSUPPORTED_CHAIN; what stays refused stays refused; no kind, flag or version moved.

The oracle against an independent model: the expected values tests/test_gpu_multi_delay.py leans on come from the oracle's
one node per stage (oracle/oracle_bank.hpp); here two of its delay nodes in series are held to numpy restatements of
delay.rs that do not pass through it."""
import os
import re

import numpy as np
import pytest

import multi_delay_cases as mc
from helpers import assert_bit_equal, make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def status_of(fn, *a, **kw):
    with pytest.raises(L.KnasterHipError) as e:
        fn(*a, **kw)
    assert str(e.value)
    return e.value.status


def _no_reduce(_user, buf, count, sample_type, root, stream):
    return 0


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"host_threads": 2}, {"rank": 0, "world": 1, "reduce_fn": _no_reduce}], ids=["one_range", "host_sharded", "rank_0_of_1"])
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_a_chain_of_several_delays_is_created(knh, sample_type, kw):
    for stages in (mc.SERIES_STAGES, mc.identity_workloads(sample_type)[0].stages, configs.config("D4", n_voices=mc.N).stages):
        b = knh.VoiceBank(stages, mc.N, sample_type, 2, L.MIX_TREE, -1, False, **kw)
        assert status_of(b.restart_voices, [0]) == L.ERR_NOT_INITIALISED  # created, and no more than that: no device was touched
        b.close()


def test_a_graph_voice_of_twelve_delays_is_created(knh):
    w, _ = mc.twelve_workload(L.F32, 64, mc.N)
    assert sum(s.kind in mc.DELAY_KINDS for s in w.stages) == 12
    b = knh.VoiceBank(w.stages, mc.N, L.F32, 2)
    assert b.debug_signature().count("Z") == 8 and b.debug_signature().count("Y") == 4
    b.close()
    w2 = mc.parallel_workload(L.F64, 64, connected=True)
    b = knh.VoiceBank(w2.stages, mc.N, L.F64, 2)
    b.connect_outputs(2, 3)
    b.close()


@pytest.mark.parametrize("kind", mc.DELAY_KINDS)
def test_the_cap_is_documented_and_one_more_is_unsupported(knh, kind):
    text = open(os.path.join(ROOT, "include", "knaster_hip.h")).read()
    cap = int(re.search(r"#define KNH_MAX_DELAY_STAGES (\d+)", text).group(1))
    assert cap >= 12 and cap == L.KNH_MAX_DELAY_STAGES
    head = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL)]
    knh.VoiceBank(head + [Stage(kind)] * cap, 4, L.F32, 2).close()
    assert status_of(knh.VoiceBank, head + [Stage(kind)] * (cap + 1), 4, L.F32, 2) == L.ERR_UNSUPPORTED_CHAIN
    # ... in a graph voice too: the delays in parallel
    par = head + [Stage(kind, input=2)] * (cap + 1) + [Stage(L.STAGE_MATH_ADD, input=3, input2=4)]
    assert status_of(knh.VoiceBank, par, 4, L.F32, 2) == L.ERR_UNSUPPORTED_CHAIN


def test_what_stays_refused(knh):
    gal = configs.config("G1", n_voices=4, block_size=64).stages
    for kind in mc.DELAY_KINDS:  # a chain that ends in Galactic holds no delay stage
        assert status_of(knh.VoiceBank, gal[:3] + [Stage(kind)] + gal[3:], 4, L.F32, 2) == L.ERR_INVALID_ARGUMENT
        # delay_time cannot be driven at audio rate
        st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_SIN_WT), Stage(kind, input=1, input2=2, ar_param=1)]
        assert status_of(knh.VoiceBank, st, 4, L.F32, 2) == L.ERR_UNSUPPORTED_CHAIN


def test_no_kind_flag_or_version_moved(knh):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "knaster_hip.h")).read(), flags=re.S)
    assert int(re.search(r"KNH_STAGE_KIND_COUNT = (\d+)", text).group(1)) == 46
    assert int(re.search(r"#define KNH_ABI_VERSION (\d+)", text).group(1)) == 4 == L.KNH_ABI_VERSION
    assert L.load().knh_abi_version() == 4
    full = open(os.path.join(ROOT, "include", "knaster_hip.h")).read()
    assert "At most one delay stage" not in full and "KNH_MAX_DELAY_STAGES" in full
    sample_delay = full[full.index("KNH_STAGE_SAMPLE_DELAY    x >>"):full.index("KNH_STAGE_ALLPASS_DELAY   x >>")]
    assert "At most one" not in sample_delay


def test_the_d4_workload(knh):
    w = configs.config("D4", n_voices=200)
    assert [s.kind for s in w.stages] == [L.STAGE_SIN_WT, L.STAGE_WR_MUL, L.STAGE_SAMPLE_DELAY] + [L.STAGE_ALLPASS_FB_DELAY] * 4 + [L.STAGE_MUL_ENV_ASR]
    rings = configs.D4_ALLPASS_SAMPLES
    assert all(np.gcd(a, b) == 1 for i, a in enumerate(rings) for b in rings[i + 1:])
    for stage, param, values in w.param_sets:
        if w.stages[stage].kind == L.STAGE_ALLPASS_FB_DELAY and param == 1:
            assert ((values >= 0.5) & (values <= 0.7)).all()
        if w.stages[stage].kind == L.STAGE_ALLPASS_FB_DELAY and param == 0:  # inside the ring, a tile or more
            assert ((values * mc.SR >= 64) & (values * mc.SR < rings[stage - 3])).all()
    assert configs.config("D3").delay_times is not None and configs.config("D3").param_sets == ()  # the existing configs as they were


# ---- the oracle against an independent model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_two_sample_delays_in_series_shift_by_the_sum(oracle, sample_type):
    """x[n - d1 - d2] exactly, x the one-stage bank's signal; a delay of the whole ring reads the sample just written
    (delay.rs:38-40: the ring index is taken modulo the length), so it shifts by nothing."""
    bs, blocks = 64, 12
    two, _, d1, d2 = mc.identity_workloads(sample_type, bs)
    n = two.n_voices
    v = np.arange(n, dtype=np.uint32)
    src = configs.Workload("source", two.stages[:2], n, bs, sample_type, 2)
    src.ctor = {0: two.ctor[0], 1: two.ctor[1]}
    o, s = make_oracle(oracle, two, want_mix=False), make_oracle(oracle, src, want_mix=False)
    o.param_apply_many(v, 2, 0, L.VALUE_FLOAT, mc.delay_seconds(d1))
    o.param_apply_many(v, 3, 0, L.VALUE_FLOAT, mc.delay_seconds(d2))
    got = np.concatenate([o.process_block()[1] for _ in range(blocks)], axis=1)
    x = np.concatenate([s.process_block()[1] for _ in range(blocks)], axis=1)
    o.close()
    s.close()
    gain = two.ctor[4][0, 0]
    ring1 = np.floor(two.ctor[2][:, 0] * mc.SR).astype(np.int64)
    ring2 = np.floor(two.ctor[3][:, 0] * mc.SR).astype(np.int64)
    assert (ring1 == 1).any() and (d1 == ring1).any() and (d1 == 0).any() and (ring1 % 2 == 1).any()
    want = np.zeros_like(x)
    for k in range(n):
        shift = int(d1[k] % ring1[k] + d2[k] % ring2[k])
        want[k, shift:] = x[k, :x.shape[1] - shift]
    want = (want * x.dtype.type(gain)).astype(x.dtype)
    assert np.abs(want).max() > 1e-4
    assert_bit_equal(got, want, "SampleDelay(d1) -> SampleDelay(d2) against the shifted source")


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_an_allpass_feedback_delay_behind_a_sample_delay(oracle, sample_type):
    """SampleDelay -> AllpassFeedbackDelay in the oracle against the numpy restatement of delay.rs:93-306 fed the shifted
    signal, with a delay_time and a feedback change on the second node while the first keeps its delay."""
    n, bs, blocks = 6, 64, 10
    dtype = np.float64 if sample_type == L.F64 else np.float32
    p = configs.voice_parameters(n)
    v = np.arange(n, dtype=np.uint32)
    rings_d, rings_z = np.array([192, 251, 160, 1, 177, 150]), np.array([256, 150, 201, 237, 151, 260])
    d, z1, z2 = np.array([70, 130, 160, 0, 0, 99]), np.array([100.37, 77.5, 140.25, 70.61, 149.9, 200.0]), np.array([71.0, 120.37, 90.5, 180.25, 3.61, 0.3])
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SAMPLE_DELAY), Stage(L.STAGE_ALLPASS_FB_DELAY)]
    w = configs.Workload("dz", st, n, bs, sample_type, 2)
    w.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 0.5), 2: mc.ring_seconds(rings_d).reshape(n, 1), 3: mc.ring_seconds(rings_z).reshape(n, 1)}
    src = configs.Workload("source", st[:2], n, bs, sample_type, 2)
    src.ctor = {0: w.ctor[0], 1: w.ctor[1]}
    o, s = make_oracle(oracle, w, want_mix=False), make_oracle(oracle, src, want_mix=False)
    fb = 0.5 + 0.03 * v
    got = []
    for b in range(blocks):
        if b == 0:
            o.param_apply_many(v, 2, 0, L.VALUE_FLOAT, mc.delay_seconds(d))
            o.param_apply_many(v, 3, 0, L.VALUE_FLOAT, z1 / mc.SR)
            o.param_apply_many(v, 3, 1, L.VALUE_FLOAT, fb)
        if b == 4:
            o.param_apply_many(v, 3, 0, L.VALUE_FLOAT, z2 / mc.SR)
        if b == 6:
            o.param_apply_many(v, 3, 1, L.VALUE_FLOAT, -fb)
        got.append(o.process_block()[1])
    got = np.concatenate(got, axis=1)
    x = np.concatenate([s.process_block()[1] for _ in range(blocks)], axis=1)
    o.close()
    s.close()
    want = np.zeros_like(x)
    for k in range(n):
        first, second = mc.SampleDelayModel(int(rings_d[k]), dtype), mc.AllpassFeedbackDelayModel(int(rings_z[k]), dtype)
        first.delay_time(float(mc.delay_seconds(d[k])))
        second.delay_time(z1[k] / mc.SR)
        second.feedback(fb[k])
        for i in range(x.shape[1]):
            if i == 4 * bs:
                second.delay_time(z2[k] / mc.SR)
            if i == 6 * bs:
                second.feedback(-fb[k])
            want[k, i] = second.tick(first.tick(x[k, i]))
    assert np.abs(want).max() > 1e-3
    assert_bit_equal(got, want, "SampleDelay -> AllpassFeedbackDelay against the numpy model")
