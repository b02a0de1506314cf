"""Quiet runs of the pipeline kernel (voice_pipe.hpp, pipe_run_group): consecutive whole tiles of a block with no event of
any lane inside them run in a tight loop -- LDS reads, the stages, LDS stores, the step barrier, the advance -- with the tile
buffers carried forward and the filter's choice of step made once per run.  What can go wrong is the run logic: where a run
starts and ends, the barrier count, the buffer a tile lands in, a choice made per run that an event should have changed.
So: the smallest banks with more than one voice group and a ragged last one, blocks of one tile, of whole tiles and with a
partial last tile, and events on some lanes placed on the frames around the tile edges.  Every pipeline form (32-sample tiles
with a mixer wavefront, 64-sample tiles folding in the last group, 64-sample tiles in place; f64: half of each) is held, bit
for bit, to the single-wavefront kernel (KNH_PIPELINE=0) and to the CPU oracle.

The filter's ic2 = -0.0 is the one state in which the run's choice of step must come out "general".  No call of the reference
produces it (no entry point writes a filter's state; SET events reach coefficients only), so the library has a test-only
switch for it: KNH_DEBUG_SVF_IC2_NEG0=1 starts every third voice's filter with ic2eq = -0.0 (voice_bank.hpp)."""
import numpy as np
import pytest

from helpers import assert_bit_equal, make_gpu, make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

pytestmark = pytest.mark.gpu

SINGLE = {"KNH_PIPELINE": "0"}
FORMS = {"mixer": {"KNH_PIPELINE": "1", "KNH_PIPE_BIG": "0"}, "fold": {"KNH_PIPELINE": "1", "KNH_PIPE_BIG": "1"},
         "inplace": {"KNH_PIPELINE": "1", "KNH_PIPE_BIG": "2"}}
PAIR = {"pair": {"KNH_PIPELINE": "1", "KNH_PAIR": "1"}}  # two voice groups per workgroup (an odd number of groups: one of them dead)


def _bank(knh, monkeypatch, w, env, mix=L.MIX_TREE):
    with monkeypatch.context() as m:  # (the switches are read when a bank is created and initialised)
        for k, v in env.items():
            m.setenv(k, v)
        return make_gpu(knh, w, mix)


def _c3_timed(n, bs, sample_type):
    """the C3 chain with the filter and the envelope behind WrPreciseTiming: their changes land on a frame of the block"""
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF, delayed_changes_per_block=2),
          Stage(L.STAGE_MUL_ENV_ASR, delayed_changes_per_block=2)]
    w = configs.Workload("quiet", st, n, bs, sample_type, 2)
    w.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 1.0 / n),
              2: np.stack([np.full(n, float(L.SVF_LOW)), p["cutoff"], p["q"], np.zeros(n)], axis=1), 3: np.stack([p["attack"], p["release"]], axis=1)}
    return w


def _edge_frames(bs):
    """frames around the tile edges of every tile length in use (16, 32, 64): the last frame of a tile, frame 0 of the next;
    the block's last frame, and the block's end itself (a change due at frame == block_size)"""
    f = set()
    for t in (16, 32, 64):
        for k in (1, 2):
            if k * t < bs:
                f.update((k * t - 1, k * t))
    f.update((bs - 1, bs))
    return sorted(f)


def _plan(w, n_blocks):
    """{block: batches}: the note on for every voice in front of block 0; in blocks 0 and 2 one change on two voices of three,
    neighbours on different frames: a release or a restart of the envelope, a new cutoff (SETs of the filter's coefficients),
    the filter's type away from low-pass (block 0) and back (block 2)."""
    n, bs = w.n_voices, w.block_size
    v = np.arange(n, dtype=np.uint32)
    frames = _edge_frames(bs)
    p = configs.voice_parameters(n)
    plan = {0: [(v, 3, 3, L.VALUE_TRIGGER, None, None, None)]}
    for blk in (0, 2):
        if blk >= n_blocks:
            continue
        some = v[v % 3 != 1]
        d = np.array([frames[(int(x) * 5 + blk) % len(frames)] for x in some], dtype=np.uint16)
        kind = (some // 2) % 4
        b = plan.setdefault(blk, [])
        m = kind == 0
        b.append((some[m], 3, 2, L.VALUE_TRIGGER, None, None, d[m]))                       # t_release
        m = kind == 1
        b.append((some[m], 3, 3, L.VALUE_TRIGGER, None, None, d[m]))                       # t_restart
        m = kind == 2
        b.append((some[m], 2, 0, L.VALUE_FLOAT, p["cutoff"][some[m]] * (0.5 + 0.25 * blk), None, d[m]))  # cutoff_freq
        m = kind == 3
        ty = (L.SVF_LOW + 1 + (some[m] % 8)) % 9 if blk == 0 else np.full(int(m.sum()), L.SVF_LOW)
        b.append((some[m], 2, 3, L.VALUE_INTEGER, None, np.asarray(ty, dtype=np.int64), d[m]))         # filter type
    return plan


def _took(bank, env):
    """the kernel form the bank's launches took (word 2 of knh_bank_debug_words): a wave pipeline, or whole-chain wavefronts"""
    form = int(bank.debug_words()[2])
    if env.get("KNH_PIPELINE") == "0":
        assert form in (L.DEBUG_FORM_WHOLE_CHAIN, L.DEBUG_FORM_WHOLE_CHAIN_FUSED), form
    else:
        assert form in (L.DEBUG_FORM_PIPELINE, L.DEBUG_FORM_PIPELINE_FUSED), form


def _apply(bank, batches, offset=0):
    for (v, s, p, kind, f, i, d) in batches:
        if len(v):
            if offset:
                bank.param_apply_many(v, s, p, kind, f, i, d, block_offset=offset)
            else:
                bank.param_apply_many(v, s, p, kind, f, i, d)


_ORACLE = {}  # (n, bs, sample type, blocks) -> the oracle's per-voice signals and done frames, rendered once


def _oracle_voices(oracle, w, n_blocks):
    key = (w.n_voices, w.block_size, w.sample_type, n_blocks)
    if key not in _ORACLE:
        o = make_oracle(oracle, w)
        plan = _plan(w, n_blocks)
        res = []
        for blk in range(n_blocks):
            _apply(o, plan.get(blk, []))
            _, ov, _, od = o.process_block()
            res.append((ov.copy(), od.copy()))
        o.close()
        for ov, _ in res:
            ov.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


def _launch(knh, monkeypatch, w, env, n_blocks):
    """all blocks in one launch, the changes scheduled ahead -> the mix [blocks, ch, B]"""
    g = _bank(knh, monkeypatch, w, env)
    for blk, batches in _plan(w, n_blocks).items():
        _apply(g, batches, blk)
    out, _ = g.process_blocks(n_blocks)
    _took(g, env)
    g.close()
    return out


def _check_forms(knh, oracle, monkeypatch, w, n_blocks, forms):
    want = _oracle_voices(oracle, w, n_blocks)
    single = _launch(knh, monkeypatch, w, SINGLE, n_blocks)
    assert np.abs(single).max() > 1e-6
    plan = _plan(w, n_blocks)
    for form, env in forms.items():
        assert_bit_equal(_launch(knh, monkeypatch, w, env, n_blocks), single, f"{form}: {n_blocks} blocks in one launch against the single-wavefront kernel")
        g = _bank(knh, monkeypatch, w, env)  # block by block: the per-voice signals
        for blk in range(n_blocks):
            _apply(g, plan.get(blk, []))
            out, voices, _ = g.process_block_voices()
            assert_bit_equal(voices, want[blk][0], f"{form}: block {blk} per-voice against the oracle")
            assert_bit_equal(out, single[blk], f"{form}: block {blk} mix")
            np.testing.assert_array_equal(g.read_done_frames(), want[blk][1])
        _took(g, env)
        g.close()


# one tile (f32, 64-sample form: a run of one), whole tiles, a partial last tile that ends every run; f64: tiles of 32 / 16
@pytest.mark.parametrize("sample_type,bs,n_blocks", [(L.F32, 64, 3), (L.F32, 128, 3), (L.F32, 192, 3), (L.F32, 96, 3), (L.F32, 160, 3), (L.F32, 128, 1),
                                                     (L.F64, 64, 3), (L.F64, 128, 3), (L.F64, 96, 3), (L.F64, 160, 3)])
def test_runs_end_at_events_on_the_tile_edges(knh, oracle, monkeypatch, sample_type, bs, n_blocks):
    """130 voices (three groups, the last with two live lanes)."""
    _check_forms(knh, oracle, monkeypatch, _c3_timed(130, bs, sample_type), n_blocks, FORMS)


@pytest.mark.parametrize("n,bs", [(200, 96), (130, 128)])
def test_runs_in_the_two_groups_per_workgroup_form(knh, oracle, monkeypatch, n, bs):
    """Four groups in two workgroups; three groups, the second workgroup's other group only keeping the barriers company."""
    _check_forms(knh, oracle, monkeypatch, _c3_timed(n, bs, L.F32), 3, PAIR)


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_a_call_over_frames_that_are_not_tile_aligned(knh, oracle, monkeypatch, sample_type):
    """Block 1 of three in two calls, frames [0, 37) and [37, 160): the second call's tiles start on frame 37."""
    w = _c3_timed(130, 160, sample_type)
    want = _oracle_voices(oracle, w, 3)
    plan = _plan(w, 3)
    cut = 37
    for form, env in {"single": SINGLE, **FORMS}.items():
        g = _bank(knh, monkeypatch, w, env)
        for blk in range(3):
            _apply(g, plan.get(blk, []))
            if blk == 1:
                _, v1, _ = g.process_block_voices(cut, 0)
                _, v2, _ = g.process_block_voices(w.block_size - cut, cut)
                voices = np.concatenate([v1[:, :cut], v2[:, cut:]], axis=1)
            else:
                _, voices, _ = g.process_block_voices()
            assert_bit_equal(voices, want[blk][0], f"{form}: block {blk} per-voice against the oracle")
        g.close()


@pytest.mark.parametrize("form", ["mixer", "inplace"])  # (the form that folds in its last group has no mixer wavefront and is never resident)
def test_one_block_calls_on_a_resident_kernel(knh, monkeypatch, form):
    """Six calls of one block, with single changes, a range trigger and nothing at all between them: a resident kernel (the
    run loop once per call) gives what a launch per call gives."""
    w = configs.config("C3", n_voices=130, block_size=128)
    v = np.arange(w.n_voices, dtype=np.uint32)

    def render(resident):
        monkeypatch.setenv("KNH_RESIDENT", "1" if resident else "0")
        g = _bank(knh, monkeypatch, w, FORMS[form])
        outs = []
        for b in range(6):
            if b == 0:
                g.param_apply_many(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
            if b == 2:
                g.param_apply_range(10, 100, w.release[0], w.release[1], L.VALUE_TRIGGER)  # one range event
            if b == 3:
                g.param_apply_many(v[::7], 2, 0, L.VALUE_FLOAT, 400.0 + (v[::7] % 900))
            if b == 4:
                g.param_apply_range(60, 130, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
            outs.append(g.process_block()[0].copy())
        done, stats = g.read_done_frames(), g.resident_stats()
        g.close()
        return outs, done, stats
    a, b = render(True), render(False)
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        assert_bit_equal(x, y, f"call {k}")
    np.testing.assert_array_equal(a[1], b[1])
    assert np.abs(np.stack(b[0])).max() > 1e-6
    assert b[2] == (0, 0)
    assert a[2] == (6, 1), a[2]  # the six calls on one launch


# a Fan group (C2: SinNumeric's sin on eight wavefronts, each a window of every tile), a Pan2 behind the envelope (its gains
# ride in the tile rows), a delay line in the envelope's group (its ring tiles are prefetched from tile to tile)
@pytest.mark.parametrize("name,bs,voice_tol", [("C2", 256, 1e-5 / 130), ("P3", 128, 0.0), ("D3", 128, 0.0), ("D3", 96, 0.0)])
def test_other_kinds_of_stage_group(knh, oracle, monkeypatch, name, bs, voice_tol):
    """voice_tol: C2's device sine is within the north star's 1e-5 of full scale of the oracle's by design (the voices' gain is
    1 / 130; tests/test_gpu_parity.py::test_c2_sin_numeric_within_tolerance); the forms among themselves are bit-identical."""
    w = configs.config(name, n_voices=130, block_size=bs)
    v = np.arange(w.n_voices, dtype=np.uint32)
    n_blocks = 4

    def script(bank, blk):
        if blk == 0:
            if w.restart:
                bank.param_apply_many(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
            if w.delay_times is not None:  # 24 .. 190 samples, different per voice: the delayed signal arrives within these blocks
                bank.param_apply_many(v, 3, 0, L.VALUE_FLOAT, 0.0005 + 0.0005 * (v % 8))
        if blk == 2 and w.release:
            bank.param_apply_many(v[::3], w.release[0], w.release[1], L.VALUE_TRIGGER)
        if blk == 2 and name == "C2":
            bank.param_apply_many(v[::4], 0, 0, L.VALUE_FLOAT, 300.0 + v[::4])
    o = make_oracle(oracle, w)
    want = []
    for blk in range(n_blocks):
        script(o, blk)
        want.append(o.process_block()[1].copy())
    o.close()
    res = {}
    for form, env in {"single": SINGLE, **FORMS}.items():
        g = _bank(knh, monkeypatch, w, env)
        res[form] = []
        for blk in range(n_blocks):
            script(g, blk)
            out, voices, _ = g.process_block_voices()
            res[form].append((out, voices))
            if voice_tol:
                err = float(np.max(np.abs(voices.astype(np.float64) - want[blk].astype(np.float64))))
                assert err <= voice_tol, (form, blk, err)
            else:
                assert_bit_equal(voices, want[blk], f"{name} {form}: block {blk} per-voice against the oracle")
        g.close()
    assert max(float(np.abs(o_).max()) for o_, _ in res["single"]) > 1e-6
    for form in FORMS:
        for blk in range(n_blocks):
            assert_bit_equal(res[form][blk][1], res["single"][blk][1], f"{name} {form}: block {blk} per-voice against the single-wavefront kernel")
            assert_bit_equal(res[form][blk][0], res["single"][blk][0], f"{name} {form}: block {blk} mix")


@pytest.mark.parametrize("sample_type,bs", [(L.F32, 128), (L.F32, 96), (L.F64, 96)])
def test_a_run_that_starts_with_ic2_minus_zero(knh, oracle, monkeypatch, sample_type, bs):
    """Every third voice's filter starts with ic2eq = -0.0 (KNH_DEBUG_SVF_IC2_NEG0=1): the first run of every group evaluates
    "not the low-pass step" and keeps the general step to its end, the later runs (the state is an ordinary one after one
    sample) the low-pass one.  Same samples as the single-wavefront kernel, the signs of zeros included; and the oracle's
    (which starts from +0.0: the two starts differ in the sign of a zero at most, which assert_bit_equal lets pass).
    This walks the branch; it cannot tell a wrong choice from a right one: with ic1 = +0 the term ic2 + a2 * ic1 is
    -0 + +0 = +0, so v2 is never -0 and the two steps give the same bits -- as they do from every state a bank can be in
    (the comment above Svf::low_pass).  What it does catch is a run that mishandles the choice itself: a stale flag, the wrong
    branch's registers."""
    monkeypatch.setenv("KNH_DEBUG_SVF_IC2_NEG0", "1")
    w = configs.config("C3", n_voices=130, block_size=bs, sample_type=sample_type)
    v = np.arange(w.n_voices, dtype=np.uint32)
    res = {}
    for form, env in {"single": SINGLE, **FORMS}.items():
        g = _bank(knh, monkeypatch, w, env, L.MIX_LEFT_FOLD)
        res[form] = []
        for blk in range(3):
            if blk == 1:  # (the envelope is at rest in block 0: the voices are zeros with the sign the filter's output gives them)
                g.param_apply_many(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
            res[form].append(g.process_block_voices()[1])
        _took(g, env)
        g.close()
    monkeypatch.delenv("KNH_DEBUG_SVF_IC2_NEG0")
    o = make_oracle(oracle, w)
    for blk in range(3):
        if blk == 1:
            o.param_apply_many(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
        want = o.process_block()[1]
        assert_bit_equal(res["single"][blk], want, f"single: block {blk} against the oracle")
        for form in FORMS:
            assert_bit_equal(res[form][blk], res["single"][blk], f"{form}: block {blk} against the single-wavefront kernel", strict_zero=True)
    o.close()
    assert np.abs(res["single"][2]).max() > 1e-6


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_a_filter_behind_a_gain_in_its_group(knh, oracle, monkeypatch, sample_type):
    """A noise source in front of gain, filter and envelope is cut into Group<WhiteNoise> | Group<MulVal, Svf> | Group<MulAsr> by
    the run-time fusion (stage_table.hpp, partition_chain).  With a stage in front of the filter in its group, the f32 filter
    steps' state once failed to leave their fixed registers inside the run loop -- ic2 stood still from tile to tile (the
    comment at the end of Svf::tick_tile_low).  Three whole 32-sample tiles per block: a run of three."""
    n, bs = 130, 96
    v = np.arange(n, dtype=np.uint32)
    p = configs.voice_parameters(n)
    w = configs.Workload("noise", [Stage(L.STAGE_WHITE_NOISE), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)], n, bs, sample_type, 2)
    w.ctor = {0: v.astype(np.float64).reshape(n, 1), 1: np.full((n, 1), 1.0 / n),
              2: np.stack([np.zeros(n), p["cutoff"], p["q"], np.zeros(n)], axis=1), 3: np.stack([p["attack"], p["release"]], axis=1)}
    o = make_oracle(oracle, w)
    banks = {form: _bank(knh, monkeypatch, w, env, L.MIX_LEFT_FOLD) for form, env in {"single": SINGLE, "pipe": {"KNH_PIPELINE": "1"}}.items()}
    for blk in range(3):
        for bank in (o, *banks.values()):
            if blk == 0:
                bank.param_apply_many(v, 3, 3, L.VALUE_TRIGGER)
        want = o.process_block()[1]
        for form, g in banks.items():
            assert_bit_equal(g.process_block_voices()[1], want, f"{form}: block {blk} per-voice against the oracle")
    assert int(banks["pipe"].debug_words()[2]) == L.DEBUG_FORM_PIPELINE_FUSED
    assert np.abs(want).max() > 1e-6
    for bank in (o, *banks.values()):
        bank.close()
