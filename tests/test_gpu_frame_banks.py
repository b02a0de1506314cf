"""Lane-per-frame banks (the interpreter, kernels_interp.hip, and the kernel built at init, voice_frame.hpp) at the sizes where
a workgroup holds SEVERAL voices -- 512 voices and more -- and the tree fold beyond two passes of 256 rows, which the same
banks reach cheaply: in these forms fold_tree_kernel gets one row per voice.

Every bank asserts the form it runs in (debug word 2) and its voices per workgroup (debug word 3) against the literal
numbers of tests/frame_bank_cases.py.  Per-voice signals: bit for bit, signs of zeros included, against the CPU oracle.  The
tree mix: bit for bit helpers.pairwise_sum of the per-voice rows.  The left fold: numpy's sequential sum."""
import numpy as np
import pytest

import frame_bank_cases as fc
from helpers import assert_bit_equal, fire_all, make_gpu, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs

pytestmark = pytest.mark.gpu

KF = L.VALUE_FLOAT
TYPES = [L.F32, L.F64]
TYPE_IDS = ["f32", "f64"]
FORM_NAMES = list(fc.FORMS)


def set_env(monkeypatch, env):
    for k in fc.FORM_ENVS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def open_bank(knh, monkeypatch, w, form, vpw, mix_mode=L.MIX_TREE, **kw):
    """The bank of `w` in lane-per-frame form `form`; it must report that form and `vpw` voices per workgroup."""
    env, want_form = fc.FORMS[form]
    set_env(monkeypatch, env)
    g = make_gpu(knh, w, mix_mode, **kw)
    words = g.debug_words()
    assert int(words[2]) == want_form, (int(words[2]), want_form, form)
    assert int(words[3]) == vpw, f"{w.n_voices} voices, block of {w.block_size}, {form}: {int(words[3])} voices per workgroup, not {vpw}"
    return g


def left_fold(rows):
    acc = rows[0].copy()
    for k in range(1, rows.shape[0]):
        acc = acc + rows[k]
    return acc


def check_blocks(g, want, what, mix=pairwise_sum):
    """Whole blocks of `g`: every voice against want[b], the mix against `mix` of those rows."""
    for b, exp in enumerate(want):
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, exp, f"{what} block {b} per voice", strict_zero=True)
        assert_bit_equal(out[0], mix(exp), f"{what} block {b} mix", strict_zero=True)
    assert min(float(np.abs(exp).max()) for exp in want) > 1e-3, f"{what}: silent"


# ---- a. several voices per workgroup ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("sample_type", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("n,bs,vpw,last", fc.SEVERAL, ids=[f"{c[0]}x{c[1]}" for c in fc.SEVERAL])
def test_several_voices_per_workgroup(knh, oracle, monkeypatch, n, bs, vpw, last, sample_type, form):
    """`vi = threadIdx.x / threads_per_voice` picks the voice's state words (and, interpreted, its signal rows); the spare
    threads of the last workgroup shadow voice n - 1 and write nothing.  Three blocks: the phases carry."""
    want = fc.cascade_reference(oracle, fc.SEVERAL_DEPTH, n, bs, sample_type, fc.SEVERAL_BLOCKS)
    g = open_bank(knh, monkeypatch, fc.cascade(fc.SEVERAL_DEPTH, n, bs, sample_type), form, vpw)
    check_blocks(g, want, f"{n} voices ({last}), {form}")
    g.close()


def test_a_lane_per_voice_bank_reports_no_voices_per_workgroup(knh, monkeypatch):
    set_env(monkeypatch, {})
    w = configs.config("C3", n_voices=256, block_size=64)
    g = make_gpu(knh, w)
    fire_all(g, w.n_voices, *w.restart)
    g.process_block()
    words = g.debug_words()
    assert int(words[2]) not in (L.DEBUG_FORM_FRAME_JIT, L.DEBUG_FORM_FRAME_INTERP) and int(words[3]) == 0, words[:4]
    g.close()


# ---- b. parameter changes that differ per voice within a workgroup --------------------------------------------------------------
def send(bank, calls, **kw):
    for stage, voices, values in calls:
        bank.param_apply_many(voices, stage, 0, KF, values, **kw)


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("n,vpw", fc.TRAFFIC, ids=[str(c[0]) for c in fc.TRAFFIC])
def test_parameter_changes_differ_within_a_workgroup(knh, oracle, monkeypatch, n, vpw, form):
    """Voices that share a workgroup's barriers walk event lists of different lengths (none, one, two, and three on the last
    voice, whose shadows walk the same list and must write nothing).  Then the same traffic scheduled ahead, five blocks in one
    launch: the same mixes."""
    want = fc.traffic_reference(oracle, n)
    w = fc.traffic_workload(n)
    g = open_bank(knh, monkeypatch, w, form, vpw)
    mixes = []
    for b in range(fc.TRAFFIC_BLOCKS):
        send(g, fc.traffic_calls(n, b))
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, want[b], f"{n} voices, {form}, block {b} per voice", strict_zero=True)
        assert_bit_equal(out[0], pairwise_sum(want[b]), f"{n} voices, {form}, block {b} mix", strict_zero=True)
        assert float(np.abs(want[b]).max()) > 1e-3
        mixes.append(out)
    g.close()
    for b, touched, untouched in ((1, 0, 1), (2, n - 1, None), (3, n - 1, n - 2), (4, n - 2, n - 3)):  # (the premise: each block's calls are heard)
        silent = fc.traffic_reference(oracle, n, without=b)[b]
        assert not np.array_equal(want[b][touched], silent[touched])
        assert untouched is None or np.array_equal(want[b][untouched], silent[untouched])
    ahead = open_bank(knh, monkeypatch, w, form, vpw)
    for b in range(1, fc.TRAFFIC_BLOCKS):
        send(ahead, fc.traffic_calls(n, b), block_offset=b)
    many = ahead.process_blocks(fc.TRAFFIC_BLOCKS)[0]
    ahead.close()
    assert_bit_equal(many, np.stack(mixes), f"{n} voices, {form}: five blocks in one launch", strict_zero=True)


# ---- c. a block in two calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("sample_type", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("n,vpw,vpw_short", fc.SPLIT, ids=[str(c[0]) for c in fc.SPLIT])
def test_a_block_in_two_calls(knh, oracle, monkeypatch, n, vpw, vpw_short, sample_type, form):
    """Frames 0 .. 40, a frequency change, frames 40 .. 100.  The interpreter picks its workgroup shape per call (the 40-frame
    call: 64 threads per voice, `vpw_short` voices per workgroup), so the second call finds the words the first one left in
    another arrangement of threads.  A call on a node takes effect at once in the reference (UGen::param_apply): the change is
    heard from frame 40 on, which is what the oracle at block size 20 renders (frame_bank_cases.split_reference) -- not what a
    whole-block call at the next block start would give, so that comparison has no place here."""
    want = fc.split_reference(oracle, n, sample_type)
    plain = fc.cascade_reference(oracle, fc.SPLIT_DEPTH, n, fc.SPLIT_BS, sample_type, 1)[0]
    assert not np.array_equal(want[0][0, fc.SPLIT_AT:], plain[0, fc.SPLIT_AT:]) and np.array_equal(want[0][:, :fc.SPLIT_AT], plain[:, :fc.SPLIT_AT])
    g = open_bank(knh, monkeypatch, fc.cascade(fc.SPLIT_DEPTH, n, fc.SPLIT_BS, sample_type), form, vpw)
    at, bs = fc.SPLIT_AT, fc.SPLIT_BS
    for b in range(fc.SPLIT_BLOCKS):
        o1, v1, _ = g.process_block_voices(at, 0)
        stage, voices, values = fc.split_calls(n, b)
        g.param_apply_many(voices, stage, 0, KF, values)
        o2, v2, _ = g.process_block_voices(bs - at, at)
        got = np.concatenate([v1[:, :at], v2[:, at:]], axis=1)
        assert_bit_equal(got, want[b], f"{n} voices, {form}, block {b} as {at} + {bs - at} frames, per voice", strict_zero=True)
        assert_bit_equal(np.concatenate([o1[0, :at], o2[0, at:]]), pairwise_sum(want[b]), f"{n} voices, {form}, block {b} mix", strict_zero=True)
        assert float(np.abs(want[b]).max()) > 1e-3
    g.close()


# ---- d. voices per workgroup limited by the LDS -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
def test_the_lds_limits_the_interpreters_voices_per_workgroup(knh, oracle, monkeypatch, form):
    """launch_interp's loop that shrinks vpw until the signal rows fit: four voices on 512 threads where the voice count allows
    five and the threads eight.  (The kernel built at init keeps the signals in registers: five, not a power of two either.)"""
    vpw = fc.ROWS_VPW[form]
    if form == "interp":
        assert 1 < vpw < min(fc.ROWS_VPW_BY_COUNT, fc.ROWS_VPW_BY_THREADS)
    w = fc.rows_workload()
    g = open_bank(knh, monkeypatch, w, form, vpw)
    assert g.debug_signature().endswith(f"#{fc.ROWS_SIG}"), g.debug_signature()[-8:]
    check_blocks(g, fc.workload_reference(oracle, "rows", 2), f"21 signal rows, {form}")
    g.close()


@pytest.mark.parametrize("form", FORM_NAMES)
def test_the_lds_limits_the_built_kernels_voices_per_workgroup(knh, oracle, monkeypatch, form):
    """voice_bank.hpp's loop for the kernel built at init: 748 state words per voice in f64 leave room for fifteen voices where
    the voice count and the threads allow sixteen.  The interpreter on the same voice: ten."""
    vpw = fc.DEEP_VPW[form]
    assert 1 < vpw < min(fc.DEEP_VPW_BY_COUNT, fc.DEEP_VPW_BY_THREADS)
    w = fc.cascade(fc.DEEP_DEPTH, fc.DEEP_N, fc.DEEP_BS, L.F64)
    g = open_bank(knh, monkeypatch, w, form, vpw)
    assert sum(g.stage_parameters(s) for s in range(len(w.stages))) == fc.DEEP_WORDS  # (a state word per parameter in this voice)
    check_blocks(g, fc.workload_reference(oracle, "deep", 2), f"{fc.DEEP_DEPTH} oscillators, {form}")
    g.close()


# ---- e. long blocks ----------------------------------------------------------------------------------------------------------------------
LONG_CASES = [(n, bs, t, vpw) for n, bs, types, vpw in fc.LONG for t in types]


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("n,bs,sample_type,vpw", LONG_CASES, ids=[f"{c[0]}x{c[1]}-{TYPE_IDS[TYPES.index(c[2])]}" for c in LONG_CASES])
def test_long_blocks(knh, oracle, monkeypatch, n, bs, sample_type, vpw, form):
    """512 frames: two voices on 1 024 threads.  1 000 and 1 024 frames: a voice on 1 024 threads, the limit of these forms."""
    want = fc.cascade_reference(oracle, fc.LONG_DEPTH, n, bs, sample_type, fc.LONG_BLOCKS)
    g = open_bank(knh, monkeypatch, fc.cascade(fc.LONG_DEPTH, n, bs, sample_type), form, vpw)
    check_blocks(g, want, f"{n} voices, blocks of {bs}, {form}")
    g.close()


@pytest.mark.parametrize("sample_type", TYPES, ids=TYPE_IDS)
def test_a_block_of_1025_frames_leaves_the_lane_per_frame_forms(knh, oracle, monkeypatch, sample_type):
    set_env(monkeypatch, {})
    want = fc.cascade_reference(oracle, fc.LONG_DEPTH, 3, 1025, sample_type, fc.LONG_BLOCKS)
    g = make_gpu(knh, fc.cascade(fc.LONG_DEPTH, 3, 1025, sample_type))
    words = g.debug_words()
    assert int(words[2]) == L.DEBUG_FORM_WHOLE_CHAIN_FUSED and int(words[3]) == 0, words[:4]
    check_blocks(g, want, "blocks of 1 025 frames, a lane per voice")
    g.close()


# ---- f. the tree fold beyond two passes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("sample_type", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("n,vpw,passes,what", fc.TREE, ids=[str(c[0]) for c in fc.TREE])
def test_tree_fold_of_many_passes(knh, oracle, monkeypatch, n, vpw, passes, what, sample_type, form):
    """fold_tree_kernel's binary-counter stack (voice_chain.hpp): passes of 256 rows meet as a counter carries, a ragged last
    pass, the closing walk over nodes of falling level.  out[0] is pairwise_sum of the bank's own per-voice rows, and those
    rows are the oracle's."""
    assert passes == -(-n // 256) and passes > 2
    want = fc.cascade_reference(oracle, fc.TREE_DEPTH, n, fc.TREE_BS, sample_type, fc.TREE_BLOCKS)
    g = open_bank(knh, monkeypatch, fc.cascade(fc.TREE_DEPTH, n, fc.TREE_BS, sample_type), form, vpw)
    for b in range(fc.TREE_BLOCKS):
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(out[0], pairwise_sum(voices), f"{n} rows, {passes} passes ({what}), {form}, block {b}", strict_zero=True)
        assert_bit_equal(voices, want[b], f"{n} voices, {form}, block {b} per voice", strict_zero=True)
        assert float(np.abs(out).max()) > 1e-3
    g.close()


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("sample_type", TYPES, ids=TYPE_IDS)
def test_tree_fold_of_several_blocks_and_of_part_of_a_block(knh, oracle, monkeypatch, sample_type, form):
    """1 297 rows: three blocks in one launch (the fold's blockIdx.y) against three single blocks, and a block as 20 + 28
    frames (the fold's frame_begin is no multiple of its 16 frames per workgroup)."""
    n, vpw = fc.TREE[1][:2]
    assert n == 1297
    want = fc.cascade_reference(oracle, fc.TREE_DEPTH, n, fc.TREE_BS, sample_type, 3)
    mixes = np.stack([pairwise_sum(v) for v in want]).reshape(3, 1, fc.TREE_BS)
    assert float(np.abs(mixes).max()) > 1e-3
    w = fc.cascade(fc.TREE_DEPTH, n, fc.TREE_BS, sample_type)
    g = open_bank(knh, monkeypatch, w, form, vpw)
    assert_bit_equal(g.process_blocks(3)[0], mixes, f"{form}: three blocks in one launch", strict_zero=True)
    g.close()
    g = open_bank(knh, monkeypatch, w, form, vpw)
    for b in range(3):
        out = np.zeros((1, fc.TREE_BS), dtype=mixes.dtype)
        g.process_block(20, 0, out=out)
        g.process_block(28, 20, out=out)
        assert_bit_equal(out, mixes[b], f"{form}: block {b} as 20 + 28 frames", strict_zero=True)
    g.close()


@pytest.mark.parametrize("form", FORM_NAMES)
def test_left_fold_of_1297_rows(knh, oracle, monkeypatch, form):
    """fold_rows_kernel: 81 rounds of its 16-rows-ahead loop and a tail of one row, against numpy's sum in voice order."""
    n, vpw = fc.TREE[1][:2]
    want = fc.cascade_reference(oracle, fc.TREE_DEPTH, n, fc.TREE_BS, L.F32, fc.TREE_BLOCKS)
    g = open_bank(knh, monkeypatch, fc.cascade(fc.TREE_DEPTH, n, fc.TREE_BS, L.F32), form, vpw, L.MIX_LEFT_FOLD)
    check_blocks(g, want, f"left fold of {n} rows, {form}", mix=left_fold)
    g.close()


# ---- g. restart ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
def test_restart_in_a_bank_of_several_voices_per_workgroup(knh, oracle, monkeypatch, form):
    """Voices 0, 255 | 256 and the lone voice 512 of the last workgroup become fresh nodes after two blocks (driven as
    tests/test_gpu_restart.py drives its cases): they equal a fresh bank's, every other voice the continuing bank's."""
    case, exp = fc.restart_case(), fc.restart_expected(oracle)
    r = sorted(case.r_sets["edges"])
    assert all(not np.array_equal(c[r], f[r]) for c, f in zip(exp.cont, exp.fresh))
    env, want_form = fc.FORMS[form]
    set_env(monkeypatch, env)
    g = case.make_gpu(knh, case.ctor_a, L.MIX_TREE)
    words = g.debug_words()
    assert int(words[2]) == want_form and int(words[3]) == fc.RESTART_VPW, words[:4]
    for b in range(case.k):
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, exp.before[b][0], f"{form} block {b} per voice", strict_zero=True)
    case.restart(g, "edges")
    for j in range(case.n_after):
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, exp.after[j][0], f"{form} block {case.k + j} per voice", strict_zero=True)
        assert_bit_equal(out[0], pairwise_sum(exp.after[j][0]), f"{form} block {case.k + j} mix", strict_zero=True)
        assert float(np.abs(voices[r]).max()) > 1e-3
    g.close()


# ---- h. voice ranges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("kw", [{"host_threads": 2}, {"devices": [0, 0]}], ids=["host_threads_2", "two_ranges_one_device"])
def test_voice_ranges_pick_their_own_voices_per_workgroup(knh, oracle, monkeypatch, kw, form):
    """1 301 voices as ranges of 704 and 597: two voices per workgroup in each, five in the one-range bank.  The same rows, bit
    for bit; the mix within the bound tests/test_gpu_dag.py holds such banks to (the ranges' trees are joined differently)."""
    n = fc.RANGES_N
    want = fc.cascade_reference(oracle, fc.SEVERAL_DEPTH, n, 64, L.F32, 3)
    w = fc.cascade(fc.SEVERAL_DEPTH, n, 64, L.F32)
    one = open_bank(knh, monkeypatch, w, form, fc.RANGES_VPW_ONE)
    cut = open_bank(knh, monkeypatch, w, form, fc.RANGES_VPW_FIRST, **kw)
    assert cut.ranks() == 2
    for b in range(3):
        o_out, o_voices, _ = one.process_block_voices()
        c_out, c_voices, _ = cut.process_block_voices()
        assert_bit_equal(o_voices, want[b], f"one range, {form}, block {b}", strict_zero=True)
        assert_bit_equal(c_voices, o_voices, f"{kw}, {form}, block {b} per voice", strict_zero=True)
        ref = pairwise_sum(want[b])
        assert_bit_equal(o_out[0], ref, f"one range, {form}, block {b} mix", strict_zero=True)
        assert np.max(np.abs(c_out[0] - ref)) <= 1e-5 * max(1.0, float(np.abs(ref).max())), (kw, form, b)
        assert float(np.abs(ref).max()) > 1e-3
    one.close()
    cut.close()
