"""Feedback edges on the device (KNH_STAGE_FLAG_FEEDBACK): every voice of tests/feedback_cases.py against the CPU oracle with
the loop closed outside it -- every sample of every voice bit for bit, the mixes as left fold / pairwise tree of those rows --
and the ways of running a bank against each other: one launch of n blocks, single calls (resident or not), partial calls,
restarted voices, banks in several ranges."""
import functools
import os

import numpy as np
import pytest

import feedback_cases as fc
from helpers import assert_bit_equal, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs

pytestmark = pytest.mark.gpu

TYPES = [L.F32, L.F64]
# every block size (8, 16: shorter than any tile; 64; 100: a tile and a 36-frame tail; 128) and every bank size (1, 64, 65, 130) once
SHAPES = [(1, 8), (64, 16), (65, 64), (130, 100), (130, 128)]
FORM_ENVS = ("KNH_PIPELINE", "KNH_WIDE", "KNH_JIT", "KNH_JIT_PIPE", "KNH_JIT_WAVES", "KNH_RESIDENT", "KNH_HOST_THREADS")


def blocks_for(bs):
    """At least four blocks, and long enough for the longest loop (a block and a delay of 100 samples) to come round twice."""
    return max(5, (208 + bs) // bs + 1)


NOT_DONE = 0xFFFFFFFF


def set_env(monkeypatch, env):
    for k in FORM_ENVS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def make_case(name, n):
    return {"comb": fc.Comb, "fm": fc.fm, "crossed": fc.crossed, "stereo": lambda k: fc.crossed(k, True), "tail": fc.tail, "long": fc.long_loop}[name](n)


def gpu_bank(knh, case, sample_type, bs, mix_mode=L.MIX_TREE, **kw):
    b = knh.VoiceBank(case.stages, case.n, sample_type, 2, mix_mode, in_channels=case.in_channels, **kw)
    for s, a in case.ctor.items():
        b.set_ctor_args(s, a)
    if case.outs:
        b.connect_outputs(*case.outs)
    b.init(configs.SAMPLE_RATE, bs)
    case.start(b)
    return b


def comb_events(block, bank, n, bs, **at):
    """Parameter traffic on the loop's other stages: a sample-accurate change of the feedback gain (the stage is wrapped for two
    changes per block), every voice at a frame of its own; the note's release for the even voices (2 ms)."""
    v = np.arange(n, dtype=np.uint32)
    if block == 2:
        bank.param_apply_many(v, fc.Comb.GAIN_STAGE, 0, L.VALUE_FLOAT, 0.3 + 0.004 * (v % 50), None, ((v * 3 + 1) % bs).astype(np.uint16), **at)
    if block == 3:
        bank.param_apply_many(v[0::2], fc.Comb.ENV_STAGE, 2, L.VALUE_TRIGGER, **at)


def events_of(name, n, bs):
    return (lambda b, bank: comb_events(b, bank, n, bs)) if name == "comb" else None


@functools.lru_cache(maxsize=None)
def expected(oracle, name, n, bs, sample_type):
    """The closed-loop oracle's blocks, computed once and shared, read-only: ([block]{stage: [n, bs]}, done frames, flags)."""
    case = make_case(name, n)
    rows, done, flags = fc.expected_blocks(oracle, case, sample_type, bs, blocks_for(bs), views=case.outs or (), events=events_of(name, n, bs))
    for r in rows:
        for a in r.values():
            a.setflags(write=False)
    return rows, done, flags


def planes_of(case, rows_b):
    """The voice's signal(s) of one block as process_block_voices hands them out."""
    if case.outs:
        return np.stack([rows_b[case.outs[0]], rows_b[case.outs[1]]])
    return rows_b[len(case.stages) - 1]


def mix_of(case, planes, mix_mode):
    fold = pairwise_sum if mix_mode == L.MIX_TREE else fc.left_fold
    if case.outs:
        return np.stack([fold(planes[0]), fold(planes[1])])
    m = fold(planes)
    return np.stack([m, m])


def assert_alive(oracle, name, n, bs, sample_type, rows):
    case = make_case(name, n)
    whole = np.concatenate([planes_of(case, r) for r in rows], axis=-1)
    last = planes_of(case, rows[-1])
    assert np.isfinite(whole).all(), "the expected signal is finite"
    assert np.abs(last).reshape(-1, last.shape[-1]).max(axis=1).min() > 0.0, "no voice is silent in the last block"
    cut, _, _ = fc.expected_blocks(oracle, case, sample_type, bs, len(rows), views=case.outs or (), cut_edges=range(len(case.edges)),
                                   events=events_of(name, n, bs))
    without = np.concatenate([planes_of(case, r) for r in cut], axis=-1)
    assert (np.abs(whole - without).reshape(-1, whole.shape[-1]).max(axis=1) > 0.0).all(), "every voice differs from itself with the edges removed"


# ---- 1. the reference's vectors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", TYPES)
def test_reference_vectors(knh, monkeypatch, sample_type):
    """graph_tests.rs:185-254 through the C ABI, 16-frame blocks: n0(+1.25) -> n1(+0.125) -> feedback -> n0 gives 1.375, 2.75,
    4.125; an edge that needed no feedback is delayed all the same: 0.125, 1.375, 1.375."""
    set_env(monkeypatch, {})
    bs = 16
    dtype = np.float64 if sample_type == L.F64 else np.float32
    g = gpu_bank(knh, fc.vector_later(3), sample_type, bs)
    word = dtype().itemsize  # the two constants' words; the edge: a block read from its ring and a block written to it
    assert g.algorithmic_bytes_per_voice_block() == (2 * word + word * bs, word * bs)
    for want in fc.VECTOR_LATER:
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, np.full((3, bs), want, dtype=dtype), "feedback_nodes")
    g.close()
    g = gpu_bank(knh, fc.vector_earlier(3), sample_type, bs)
    for want in fc.VECTOR_EARLIER:
        g.set_input(np.zeros((1, bs)))
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, np.full((3, bs), want, dtype=dtype), "feedback_nodes2")
    g.close()


# ---- 2. the voices against the closed loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", TYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,bs", SHAPES)
@pytest.mark.parametrize("name", ["comb", "fm", "crossed"])
def test_voices_equal_the_closed_loop_oracle(knh, oracle, monkeypatch, name, n, bs, sample_type):
    set_env(monkeypatch, {})
    case = make_case(name, n)
    rows, done, flags = expected(oracle, name, n, bs, sample_type)
    assert_alive(oracle, name, n, bs, sample_type, rows)
    tree = gpu_bank(knh, case, sample_type, bs, L.MIX_TREE)
    fold = gpu_bank(knh, case, sample_type, bs, L.MIX_LEFT_FOLD)
    ev = events_of(name, n, bs)
    for b in range(blocks_for(bs)):
        want = planes_of(case, rows[b])
        for bank, mode in ((tree, L.MIX_TREE), (fold, L.MIX_LEFT_FOLD)):
            if ev:
                ev(b, bank)
            out, voices, fl = bank.process_block_voices()
            assert_bit_equal(voices, want, f"{name} block {b}: per-voice rows")
            assert_bit_equal(out, mix_of(case, want, mode), f"{name} block {b}: mix {mode}")
            assert fl == flags[b], (b, fl, flags[b])
            np.testing.assert_array_equal(bank.read_done_frames(), done[b], err_msg=f"{name} block {b}: done frames")
    if name == "comb" and n > 1:  # the released voices have finished, the others sound on
        seen = np.stack(done)
        assert (seen[:, 0::2] != NOT_DONE).any(axis=0).all() and (seen[:, 1::2] == NOT_DONE).all()
        assert any(f & L.FLAG_ANY_DONE for f in flags) and not any(f & L.FLAG_ALL_DONE for f in flags)
    if name == "comb" and n == 1:  # the one voice is released and finishes: silence
        assert flags[-1] & L.FLAG_ALL_DONE and not flags[0] & L.FLAG_ALL_DONE
    tree.close()
    fold.close()


@pytest.mark.parametrize("sample_type", TYPES, ids=["f32", "f64"])
def test_stereo_connected_outputs(knh, oracle, monkeypatch, sample_type):
    """The two branches of the crossed voice as graph outputs 0 and 1: the tap of one edge and the tap of the other."""
    set_env(monkeypatch, {})
    n, bs = 65, 100
    case = make_case("stereo", n)
    rows, _, _ = expected(oracle, "stereo", n, bs, sample_type)
    assert_alive(oracle, "stereo", n, bs, sample_type, rows)
    for mode in (L.MIX_TREE, L.MIX_LEFT_FOLD):
        g = gpu_bank(knh, case, sample_type, bs, mode)
        for b in range(blocks_for(bs)):
            want = planes_of(case, rows[b])
            out, voices, _ = g.process_block_voices()
            assert_bit_equal(voices, want, f"block {b}: planes")
            assert_bit_equal(out, mix_of(case, want, mode), f"block {b}: mix")
        g.close()


@pytest.mark.parametrize("sample_type", TYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["tail", "long"])
def test_the_other_device_paths(knh, oracle, monkeypatch, name, sample_type):
    """tail: the voice's signal is an edge's source that stands behind its tap, so the device list ends in the edge's write and
    the signature says which slot the voice's signal is in ("#R=k").  long: a loop in a voice of more than sixteen device ops,
    which the kernel visits eight samples at a time -- every tile of the ring as 16-byte pieces of the lane's own ring."""
    set_env(monkeypatch, {})
    n, bs = 65, 100
    case = make_case(name, n)
    rows, _, _ = expected(oracle, name, n, bs, sample_type)
    assert_alive(oracle, name, n, bs, sample_type, rows)
    g = gpu_bank(knh, case, sample_type, bs)
    sig = g.debug_signature()
    if name == "tail":
        assert "=" in sig.rsplit("#", 1)[1] and sig.rsplit("#", 1)[0].endswith("y$0@0,_,0"), sig
    else:
        assert sig.count("@") > 16, sig
    for b in range(blocks_for(bs)):
        want = planes_of(case, rows[b])
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, want, f"{name} block {b}: per-voice rows")
        assert_bit_equal(out, mix_of(case, want, L.MIX_TREE), f"{name} block {b}: mix")
    g.close()


# ---- 3. the same blocks by three call patterns ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", TYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["comb", "crossed"])
def test_call_patterns_give_the_same_bits(knh, oracle, monkeypatch, name, sample_type):
    n, bs = 130, 100
    blocks = blocks_for(bs)
    case = make_case(name, n)
    rows, _, _ = expected(oracle, name, n, bs, sample_type)
    want = np.stack([mix_of(case, planes_of(case, r), L.MIX_TREE) for r in rows])
    ev = events_of(name, n, bs)

    # one launch of n blocks
    set_env(monkeypatch, {})
    g = gpu_bank(knh, case, sample_type, bs)
    for b in range(blocks):
        if name == "comb":  # the calls of block b of the coming launch
            comb_events(b, g, n, bs, block_offset=b)
    many, _ = g.process_blocks(blocks)
    assert_bit_equal(many, want, "one launch of n blocks")
    g.close()
    # single calls: on a resident kernel, and a launch per call
    for resident in ("1", "0"):
        set_env(monkeypatch, {"KNH_RESIDENT": resident})
        g = gpu_bank(knh, case, sample_type, bs)
        for b in range(blocks):
            if ev:
                ev(b, g)
            assert_bit_equal(g.process_block()[0], want[b], f"single calls (KNH_RESIDENT={resident}), block {b}")
        stats = g.resident_stats()
        assert (stats[0] > 0) if resident == "1" else (stats == (0, 0)), (resident, stats)
        g.close()
    # a block as two partial calls (40, 0) and (60, 40)
    set_env(monkeypatch, {})
    g = gpu_bank(knh, case, sample_type, bs)
    for b in range(blocks):
        if ev:
            ev(b, g)
        if name == "comb" and b == 2:
            # (the block with the sample-accurate changes stays one call: at the end of a call WrPreciseTiming forgets the queued
            # changes the call did not reach, precise_timing.rs:110-113 -- split, the block would not be the same block)
            assert_bit_equal(g.process_block()[0], want[b], f"block {b}")
            continue
        out = np.zeros((2, bs), dtype=g.dtype)
        g.process_block(40, 0, out=out)
        g.process_block(60, 40, out=out)
        assert_bit_equal(out, want[b], f"two partial calls, block {b}")
    g.close()


# ---- 4. restart ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", TYPES, ids=["f32", "f64"])
def test_restarted_voices_start_with_an_empty_loop(knh, oracle, monkeypatch, sample_type):
    """restart_voices([1, 64]) of a 65-voice comb bank after two blocks: from that block on the two voices are those of a fresh
    bank (first block: nothing comes round the loop), the others those of an undisturbed twin."""
    set_env(monkeypatch, {})
    n, bs = 65, 64
    case = make_case("comb", n)
    r = np.array([1, 64], dtype=np.uint32)
    others = np.setdiff1d(np.arange(n), r)
    running, twin = gpu_bank(knh, case, sample_type, bs), gpu_bank(knh, case, sample_type, bs)
    before = []
    for b in range(2):
        before.append(running.process_block_voices()[1])
        twin.process_block_voices()
    running.restart_voices(r)
    case.start(running, r)
    fresh = gpu_bank(knh, case, sample_type, bs)
    rows, _, _ = fc.expected_blocks(oracle, case, sample_type, bs, 3)
    for b in range(3):
        _, got, _ = running.process_block_voices()
        _, new, _ = fresh.process_block_voices()
        _, old, _ = twin.process_block_voices()
        assert_bit_equal(new, rows[b][len(case.stages) - 1], f"block {b}: the fresh bank against the closed loop")
        assert_bit_equal(got[r], new[r], f"block {b}: restarted voices against the fresh bank")
        assert_bit_equal(got[others], old[others], f"block {b}: the other voices")
        assert np.abs(got[r]).max(axis=1).min() > 0.0
    assert_bit_equal(before[0][r], rows[0][len(case.stages) - 1][r], "(the first note began the same way)")
    for bank in (running, twin, fresh):
        bank.close()


# ---- 5. banks in several ranges ---------------------------------------------------------------------------------------------------
def _no_reduce(_user, buf, count, sample_type, root, stream):
    return 0


@pytest.mark.parametrize("kw", [{"host_threads": 2}, {"devices": [0, 0]}, {"rank": 0, "world": 1, "reduce_fn": _no_reduce}],
                         ids=["host_threads_2", "two_ranges_one_device", "rank_0_of_1"])
def test_banks_of_several_ranges_equal_the_plain_bank(knh, oracle, monkeypatch, kw):
    """Each voice range is an ordinary bank with feedback rings of its own.  The host-sharded bank and the multi-device form (both
    ranges on one device) hold the 130 voices in ranges of 128 and 2: per-voice rows and mix are the plain bank's.  The rank form
    is rank 0 of a world of 1 here -- one range behind the rank bank's own entry points, which hand out no per-voice rows: its
    mix is the plain bank's."""
    set_env(monkeypatch, {})
    n, bs, sample_type = 130, 64, L.F32
    case = make_case("comb", n)
    ev = events_of("comb", n, bs)
    plain, ranges = gpu_bank(knh, case, sample_type, bs), gpu_bank(knh, case, sample_type, bs, **kw)
    if "rank" not in kw:
        assert ranges.ranks() == 2 and plain.ranks() == 1
    for b in range(blocks_for(bs)):
        ev(b, plain)
        ev(b, ranges)
        if "rank" in kw:  # (a rank bank hands out no per-voice rows)
            o0, f0 = plain.process_block()
            o1, f1 = ranges.process_block()
        else:
            o0, v0, f0 = plain.process_block_voices()
            o1, v1, f1 = ranges.process_block_voices()
            assert_bit_equal(v1, v0, f"block {b}: per-voice rows")
        assert_bit_equal(o1, o0, f"block {b}: mix")
        assert f1 == f0
        assert np.abs(o0).max() > 0.0
    plain.close()
    ranges.close()
