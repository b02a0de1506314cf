"""knh_bank_restart_voices on the device: the voices named become freshly constructed nodes at a block boundary, every other
voice goes on untouched -- bit for bit against the expected signal tests/restart_cases.py assembles from two reference
runs (bank A continuing, and a fresh bank with arguments B).  Sizes are the smallest at which the mechanism can go wrong:
130 voices (two full wavefronts and a ragged third), blocks of 64 frames (one whole f32 tile) and 100 (ragged)."""
import numpy as np
import pytest

import restart_cases as rc
from helpers import assert_bit_equal, make_gpu, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from sampler_pool import left_fold

pytestmark = pytest.mark.gpu

FORM_ENVS = ("KNH_PIPELINE", "KNH_WIDE", "KNH_JIT", "KNH_JIT_PIPE", "KNH_FRAME_JIT", "KNH_DEV_EVENTS", "KNH_RESIDENT", "KNH_HOST_THREADS")
FORMS = {
    "pipeline": ({}, L.DEBUG_FORM_PIPELINE),
    "one_wavefront": ({"KNH_PIPELINE": "0"}, L.DEBUG_FORM_WHOLE_CHAIN),
    "four_per_workgroup": ({"KNH_WIDE": "4"}, L.DEBUG_FORM_MANY_WAVE),
    "fused_pipeline": ({"KNH_JIT": "1"}, L.DEBUG_FORM_PIPELINE_FUSED),
    "fused_one_wavefront": ({"KNH_JIT": "1", "KNH_JIT_PIPE": "0"}, L.DEBUG_FORM_WHOLE_CHAIN_FUSED),
}


def set_env(monkeypatch, env):
    for k in FORM_ENVS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def mix_of(rows, mix_mode):
    return left_fold(rows) if mix_mode == L.MIX_LEFT_FOLD else pairwise_sum(rows)


def check_block(g, exp_block, mix_mode, what):
    """One block of the bank under test against (voices, done): per-voice signals, the mix, done frames, ANY_DONE."""
    voices, done = exp_block
    out, got, flags = g.process_block_voices()
    assert_bit_equal(got, voices, f"{what} per-voice")
    want = mix_of(voices, mix_mode)
    for c in range(out.shape[0]):
        assert_bit_equal(out[c], want, f"{what} mix ch{c}")
    np.testing.assert_array_equal(g.read_done_frames(), done, err_msg=what)
    assert bool(flags & L.FLAG_ANY_DONE) == bool((done != rc.NOT_DONE).any()), what
    return flags


def run_case(knh, case, rname, exp, mix_mode=L.MIX_LEFT_FOLD, form=None, **gpu_kw):
    g = case.make_gpu(knh, case.ctor_a, mix_mode, **gpu_kw)
    if form is not None:
        assert g.debug_words()[2] == form, (g.debug_words()[2], form)
    flags = []
    for b in range(case.k):
        case.pre(g, b)
        flags.append(check_block(g, exp.before[b], mix_mode, f"{case.name}/{rname} block {b}"))
    case.stale(g, "gpu")
    case.restart(g, rname)
    for j in range(case.n_after):
        case.post(g, j, "gpu")
        flags.append(check_block(g, exp.after[j], mix_mode, f"{case.name}/{rname} block k+{j}"))
    g.close()
    return flags


# ---- 1. kernel forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rname", ["first", "straddle", "last", "all", "dup"])
@pytest.mark.parametrize("name", ["c3_f32_64", "c3_f32_100", "c3_f64_64", "c3_f64_100"])
def test_c3_restart_between_single_blocks_left_fold(knh, oracle, monkeypatch, name, rname):
    """The default form, the reference's mix order: per-voice signals, the left-fold mix, done frames and ANY_DONE, every R."""
    set_env(monkeypatch, {})
    run_case(knh, rc.CASES[name], rname, rc.oracle_expected(oracle, name, rname), L.MIX_LEFT_FOLD)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["c3_f32_64", "c3_f32_100", "c3_f64_64"])
def test_c3_restart_in_every_kernel_form(knh, oracle, monkeypatch, name, form):
    """Every kernel form the environment switches select, tree mix; all voices had finished their note before the boundary
    (ALL_DONE), are restarted (new nodes at rest: still ALL_DONE until triggered) and play the next one."""
    env, want_form = FORMS[form]
    set_env(monkeypatch, env)
    case = rc.CASES[name]
    for rname in ("dup", "all"):
        flags = run_case(knh, case, rname, rc.oracle_expected(oracle, name, rname), L.MIX_TREE, form=want_form)
        assert flags[case.k - 1] & L.FLAG_ALL_DONE, "every envelope had finished before the boundary"
        assert not (flags[case.k] & L.FLAG_ALL_DONE), "the restarted voices were triggered again"


@pytest.mark.parametrize("form", ["pipeline", "fused_one_wavefront"])
@pytest.mark.parametrize("name", ["c3_f32_64", "c3_f64_100"])
def test_c3_restart_between_two_four_block_launches(knh, oracle, monkeypatch, name, form):
    """knh_bank_process_blocks: the traffic addressed to the blocks of the launch, the restart between two launches -- and
    between two launches in flight (knh_bank_process_blocks_begin / _end)."""
    env, want_form = FORMS[form]
    set_env(monkeypatch, env)
    case = rc.CASES[name]
    assert case.k == 4 and case.n_after == 4
    for rname in ("straddle", "all"):
        exp = rc.oracle_expected(oracle, name, rname)
        for in_flight in (False, True):
            g = case.make_gpu(knh, case.ctor_a, L.MIX_TREE)
            assert g.debug_words()[2] == want_form
            for b in range(4):
                case.pre(g, b, **({"block_offset": b} if b else {}))
            if in_flight:
                g.process_blocks_begin(4)
            else:
                first, _ = g.process_blocks(4)
            case.stale(g, "gpu")
            case.restart(g, rname)
            for j in range(4):
                case.post(g, j, "gpu", **({"block_offset": j} if j else {}))
            if in_flight:
                g.process_blocks_begin(4)
                first, second = g.process_blocks_end(), g.process_blocks_end()
            else:
                second, _ = g.process_blocks(4)
            for b in range(4):
                for c in range(2):
                    assert_bit_equal(first[b, c], pairwise_sum(exp.before[b][0]), f"{name}/{rname} launch 1 block {b}")
                    assert_bit_equal(second[b, c], pairwise_sum(exp.after[b][0]), f"{name}/{rname} launch 2 block {b}")
            g.close()


# ---- 2. rings -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sample_delay_f32", "sample_delay_f64", "allpass_f32", "allpass_fb_f32", "allpass_fb_f64"])
def test_restarted_delay_rings_are_zero_and_the_neighbours_untouched(knh, oracle, monkeypatch, name):
    """Restarted after the rings have wrapped: the new nodes' first samples are the fresh bank's (a ring of zeros), and
    voices 62, 65 and 128 beside them -- and every other -- are the continuing bank's to the bit: the clear stays inside
    the voice's ring on both sides and in front of the spare ring."""
    set_env(monkeypatch, {})
    case = rc.CASES[name]
    for rname in case.r_sets:
        run_case(knh, case, rname, rc.oracle_expected(oracle, name, rname), L.MIX_LEFT_FOLD)
    set_env(monkeypatch, {"KNH_PIPELINE": "0"})
    run_case(knh, case, "ring", rc.oracle_expected(oracle, name, "ring"), L.MIX_TREE)


# ---- 3. a graph voice -----------------------------------------------------------------------------------------------------
def test_graph_voice_fused_at_init(knh, oracle, monkeypatch):
    set_env(monkeypatch, {})
    run_case(knh, rc.CASES["graph"], "dup", rc.oracle_expected(oracle, "graph", "dup"), L.MIX_LEFT_FOLD, form=L.DEBUG_FORM_WHOLE_CHAIN_FUSED)


def test_kinds_held_to_a_tolerance_elsewhere_against_device_references(knh, monkeypatch):
    """SinNumeric's sin and powf run in the device library: bank A continuing and the fresh bank are device banks here."""
    set_env(monkeypatch, {})
    case = rc.CASES["numeric"]
    for rname in case.r_sets:
        exp = rc.build_expected(case, rname, lambda w: make_gpu(knh, w, L.MIX_LEFT_FOLD), rc.gpu_step)
        assert all((c[sorted(set(case.r_sets[rname]))] != f[sorted(set(case.r_sets[rname]))]).any() for c, f in zip(exp.cont, exp.fresh))
        run_case(knh, case, rname, exp, L.MIX_LEFT_FOLD)


# ---- 4. queues, 5. ordering ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev_events", ["0", None])
@pytest.mark.parametrize("rname", ["straddle", "all"])
def test_armed_delays_and_waiting_changes_do_not_survive(knh, oracle, monkeypatch, rname, dev_events):
    set_env(monkeypatch, {} if dev_events is None else {"KNH_DEV_EVENTS": dev_events})
    run_case(knh, rc.CASES["queues"], rname, rc.oracle_expected(oracle, "queues", rname), L.MIX_LEFT_FOLD)
    run_case(knh, rc.CASES["queues"], rname, rc.oracle_expected(oracle, "queues", rname), L.MIX_TREE)


def test_calls_before_the_restart_are_dropped_and_ramps_end(knh, oracle, monkeypatch):
    set_env(monkeypatch, {})
    run_case(knh, rc.CASES["ordering"], "straddle", rc.oracle_expected(oracle, "ordering", "straddle"), L.MIX_LEFT_FOLD)


# ---- 6. lane-per-frame forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_jit,form", [("0", L.DEBUG_FORM_FRAME_INTERP), (None, L.DEBUG_FORM_FRAME_JIT)])
def test_lane_per_frame_forms(knh, oracle, monkeypatch, frame_jit, form):
    set_env(monkeypatch, {} if frame_jit is None else {"KNH_FRAME_JIT": frame_jit})
    for rname in ("one", "every"):
        run_case(knh, rc.CASES["frame"], rname, rc.oracle_expected(oracle, "frame", rname), L.MIX_LEFT_FOLD, form=form)


# ---- 7. the per-block call on a resident kernel ---------------------------------------------------------------------------
def test_restart_between_calls_on_a_resident_kernel(knh, oracle, monkeypatch):
    case, rname = rc.CASES["c3_f32_64"], "straddle"
    exp = rc.oracle_expected(oracle, case.name, rname)
    runs = {}
    for resident in ("1", "0"):
        set_env(monkeypatch, {"KNH_RESIDENT": resident})
        g = case.make_gpu(knh, case.ctor_a, L.MIX_TREE)
        outs = []
        for b in range(case.k):
            case.pre(g, b)
            outs.append(g.process_block()[0].copy())
        case.stale(g, "gpu")
        case.restart(g, rname)
        for j in range(case.n_after):
            case.post(g, j, "gpu")
            outs.append(g.process_block()[0].copy())
        runs[resident] = (outs, g.resident_stats())
        g.close()
    for b, (x, y) in enumerate(zip(runs["1"][0], runs["0"][0])):
        assert_bit_equal(x, y, f"block {b}: resident against a launch per call")
        want = pairwise_sum((exp.before + exp.after)[b][0])
        assert_bit_equal(y[0], want, f"block {b} mix")
    assert runs["0"][1] == (0, 0)
    assert runs["1"][1] == (case.k + case.n_after, 2), runs["1"][1]  # every call served resident; the kernel left for the restart and was launched again


# ---- 8. voice ranges ------------------------------------------------------------------------------------------------------
def _no_reduce(_user, buf, count, sample_type, root, stream):
    return 0


@pytest.mark.parametrize("kw", [{"host_threads": 2}, {"devices": [0, 0]}, {"rank": 0, "world": 1, "reduce_fn": _no_reduce}],
                         ids=["host_threads_2", "two_ranges_one_device", "rank_0_of_1"])
@pytest.mark.parametrize("name", ["c3_f32_64", "c3_f64_100"])
def test_banks_of_several_ranges_route_by_global_voice(knh, oracle, monkeypatch, name, kw):
    """R straddles a wavefront boundary (63, 64) and the boundary between the two ranges (127, 128: a two-range bank of 130 voices
    is 128 + 2): same blocks as the one-range bank."""
    set_env(monkeypatch, {})
    case = rc.CASES[name]
    for rname in ("range", "dup"):
        exp = rc.oracle_expected(oracle, name, rname)
        outs = []
        for bank_kw in ({}, kw):
            g = case.make_gpu(knh, case.ctor_a, L.MIX_TREE, **bank_kw)
            if "host_threads" in bank_kw or "devices" in bank_kw:
                assert g.ranks() == 2
            blocks = []
            for b in range(case.k):
                case.pre(g, b)
                blocks.append(g.process_block()[0].copy())
            case.stale(g, "gpu")
            case.restart(g, rname)
            for j in range(case.n_after):
                case.post(g, j, "gpu")
                if "rank" in bank_kw:
                    blocks.append(g.process_block()[0].copy())
                else:  # (a rank bank hands out no per-voice rows)
                    out, voices, _ = g.process_block_voices()
                    assert_bit_equal(voices, exp.after[j][0], f"{name}/{rname} block k+{j} per-voice")
                    blocks.append(out.copy())
            if "rank" not in bank_kw:
                np.testing.assert_array_equal(g.read_done_frames(), exp.after[-1][1])
            outs.append(blocks)
            g.close()
        for b, (x, y) in enumerate(zip(*outs)):
            assert_bit_equal(y, x, f"{name}/{rname} block {b}: {kw} against one range")


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------
def status_of(fn, *a, **kw):
    with pytest.raises(L.KnasterHipError) as e:
        fn(*a, **kw)
    assert str(e.value)
    return e.value.status


def _twins(knh, case, mix_mode=L.MIX_LEFT_FOLD):
    g, twin = case.make_gpu(knh, case.ctor_a, mix_mode), case.make_gpu(knh, case.ctor_a, mix_mode)
    for b in range(2):
        for bank in (g, twin):
            case.pre(bank, b)
            bank.process_block()
    return g, twin


def _same_next_blocks(g, twin, what, first_call=()):
    for k in range(2):
        a = g.process_block_voices(*(first_call if k == 0 else ()))
        b = twin.process_block_voices(*(first_call if k == 0 else ()))
        assert_bit_equal(a[1], b[1], f"{what}: per-voice, block {k} after the refusal")
        assert_bit_equal(a[0], b[0], f"{what}: mix, block {k} after the refusal")


def test_refusals_change_nothing(knh, monkeypatch):
    set_env(monkeypatch, {})
    case = rc.CASES["c3_f32_64"]
    r = np.array([63, 64], dtype=np.uint32)
    freq_b = np.asarray(case.ctor_b[0]).reshape(rc.N, -1)[r]
    # a voice index of n_voices, a stage out of range, a wrong n_args, null arrays
    g, twin = _twins(knh, case)
    assert status_of(g.restart_voices, [5, rc.N]) == L.ERR_OUT_OF_RANGE
    assert status_of(g.set_voice_ctor_args, 0, [5, rc.N], [[100.0], [200.0]]) == L.ERR_OUT_OF_RANGE
    assert status_of(g.set_voice_ctor_args, 4, [5], [[100.0]]) == L.ERR_OUT_OF_RANGE
    assert status_of(g.set_voice_ctor_args, 2, [5], [[100.0]]) == L.ERR_INVALID_ARGUMENT   # SvfFilter::new takes four
    lib = L.load()
    assert lib.knh_bank_restart_voices(g._h, 2, None) == L.ERR_INVALID_ARGUMENT
    assert lib.knh_bank_set_voice_ctor_args(g._h, 0, 2, None, None, 1) == L.ERR_INVALID_ARGUMENT
    g.restart_voices([])  # count == 0 is KNH_OK
    _same_next_blocks(g, twin, "index and argument refusals")
    # (the refused ctor calls kept nothing: a restart now constructs voice 5 from arguments A, as a bank does that never got them)
    g.restart_voices([5])
    twin.restart_voices([5])
    _same_next_blocks(g, twin, "a restart after refused ctor calls")
    g.close(); twin.close()
    # while a block is partly processed
    g, twin = _twins(knh, case)
    g.process_block(40, 0)
    twin.process_block(40, 0)
    assert status_of(g.restart_voices, r) == L.ERR_INVALID_ARGUMENT
    assert status_of(g.set_voice_ctor_args, 0, r, freq_b) == L.ERR_INVALID_ARGUMENT
    _same_next_blocks(g, twin, "mid-block", first_call=(24, 40))
    g.set_voice_ctor_args(0, r, freq_b)  # the block is complete: both calls are taken again
    g.restart_voices(r)
    g.close(); twin.close()
    # a ring longer than the stride (the allocation was made at init: 0.004 s = 192 samples)
    ring = rc.CASES["sample_delay_f32"]
    g, twin = _twins(knh, ring)
    assert status_of(g.set_voice_ctor_args, 1, r, [[0.004], [0.0041]]) == L.ERR_OUT_OF_RANGE
    g.restart_voices(r)  # nothing of the refused call was kept, not its first row either: both banks restart with arguments A
    twin.restart_voices(r)
    _same_next_blocks(g, twin, "ring longer than the stride")
    g.close(); twin.close()
    # a chain that ends in Galactic: accepted at create and init, refused at the call
    w = configs.config("G1", n_voices=4, block_size=64)
    g, twin = make_gpu(knh, w), make_gpu(knh, w)
    for bank in (g, twin):
        bank.param_apply_many(np.arange(4, dtype=np.uint32), 2, 2, L.VALUE_TRIGGER)
        bank.process_block()
    assert status_of(g.restart_voices, [0]) == L.ERR_UNSUPPORTED_CHAIN
    assert status_of(g.set_voice_ctor_args, 0, [0], [[100.0]]) == L.ERR_UNSUPPORTED_CHAIN
    _same_next_blocks(g, twin, "Galactic")
    g.close(); twin.close()
