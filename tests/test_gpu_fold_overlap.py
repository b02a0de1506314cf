"""A launch's tree fold beside the next launch's voice kernel (voice_bank.hpp process): back-to-back
knh_bank_process_blocks_device calls put their voice kernels on a stream of the bank's, their folds -- in the form that needs
no LDS, fold_tree_wave_kernel -- on another, and make the caller's stream wait for each fold.  What can go wrong: a fold reading
rows the launch after the next already rewrites (two sets of partial rows), a fold clearing flag words a running kernel
accumulates into (three sets of flag words), the caller's stream running ahead of a fold, the realloc of the row sets, the
return to the caller's stream for a blocking call, and the new fold's own tree.

Small banks that still have a tree above the wavefront level and a partial group: the C3 chain at 130 voices (3 rows) and at
64 * 5 + 1 voices (6 rows), blocks of 64 frames (one tile) and 96 (one and a half), f32 and f64, launches of 1..3 blocks.
Every comparison is bit for bit against the same bank with KNH_FOLD_OVERLAP=0 (every launch on the caller's stream, the
fold fold_tree_kernel) driven one launch at a time with synchronize() after each; the one-launch-per-block path is pinned to
the oracle by the other suites.  Debug word 9 says how many launches took the overlapped path, word 10 how many tree folds
took the form without LDS."""
import numpy as np
import pytest

import frame_bank_cases as fc
from device_buffers import Hip
from helpers import assert_bit_equal, make_gpu, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.configs import Stage

pytestmark = pytest.mark.gpu

SERIAL = {"KNH_FOLD_OVERLAP": "0"}
SHAPES = [(n, bs, st) for n in (130, 64 * 5 + 1) for bs in (64, 96) for st in (L.F32, L.F64)]
SHAPE_IDS = [f"{n}x{bs}-{'f64' if st == L.F64 else 'f32'}" for n, bs, st in SHAPES]
PLAN = [1, 2, 3, 1, 3, 2]  # blocks per launch: the row sets are reallocated in front of launches 1 and 2
MAX_BLOCKS = 3


def workload(name, n, bs, st):
    """The C3 chain (P3: with a Pan2 behind it), its envelopes short enough to finish inside the few hundred frames of a run:
    attack 24 frames, release 30 .. 170 frames, rising with the voice index."""
    if name == "IN":  # the bank node's input channel times a constant per voice: the input's upload travels on the caller's stream
        w = configs.Workload(name, [Stage(L.STAGE_INPUT), Stage(L.STAGE_MUL_CONST)], n, bs, st, 1)
        w.ctor = {0: np.zeros((n, 1)), 1: (0.25 + np.arange(n) % 7).reshape(n, 1).astype(np.float64)}
        w.in_channels = 1
        return w
    w = configs.config("C3" if name == "RESTART" else name, n_voices=n, block_size=bs, sample_type=st)
    w.name = name
    w.ctor = dict(w.ctor)
    w.ctor[3] = np.stack([np.full(n, 0.0005), 0.000625 + 0.003 * np.arange(n) / n], axis=1)
    return w


def bank(knh, monkeypatch, w, env, **kw):
    with monkeypatch.context() as m:  # (the switches are read when a bank is created)
        for k, v in env.items():
            m.setenv(k, v)
        g = make_gpu(knh, w, **kw)
    assert int(g.debug_words()[2]) not in (L.DEBUG_FORM_FRAME_JIT, L.DEBUG_FORM_FRAME_INTERP)
    return g


def events(g, w, k, nb):
    """The range events in front of launch k: envelopes start, are released half a bank at a time and finish in different launches."""
    n = w.n_voices
    if w.name == "IN":  # this launch's input blocks, different in every launch
        g.set_input(np.random.default_rng(100 + k).uniform(-1.0, 1.0, (nb, 1, w.block_size)).astype(np_dtype(w)))
        return
    if w.name == "RESTART" and k in (2, 3):  # voices of both halves and the lone last one become fresh nodes in front of launches 2 and 3
        g.restart_voices(np.array([0, 63, 64, n - 1], dtype=np.uint32))
    def trig(v0, v1, what, off=0):
        g.param_apply_many(np.arange(v0, v1, dtype=np.uint32), what[0], what[1], L.VALUE_TRIGGER, block_offset=off)
    if k % 3 == 0:
        trig(0, n, w.restart)
    elif k == 1:
        trig(0, n // 2, w.release[:2])
    elif k == 2:
        trig(n // 2, n, w.release[:2])
    elif k == 4:
        trig(0, n, w.release[:2], nb - 1)


def np_dtype(w):
    return np.float64 if w.sample_type == L.F64 else np.float32


def block_bytes(w):
    return w.out_channels * w.block_size * np.dtype(np_dtype(w)).itemsize


_SERIAL = {}


def serial_run(knh, monkeypatch, name, shape, plan=tuple(PLAN)):
    """Launch by launch on the caller's stream, synchronize() after each: per launch (blocks, done_frames, flag words 0 and 1)."""
    key = (name, shape, plan)
    if key not in _SERIAL:
        w = workload(name, *shape)
        g = bank(knh, monkeypatch, w, SERIAL)
        hip = Hip()
        buf = hip.zeros(MAX_BLOCKS * block_bytes(w))
        res = []
        for k, nb in enumerate(plan):
            events(g, w, k, nb)
            g.process_blocks_device(nb, buf)
            g.synchronize()
            words = g.debug_words()
            assert int(words[9]) == 0
            res.append((hip.to_host(buf, (nb, w.out_channels, w.block_size), np_dtype(w)), g.read_done_frames().copy(), (int(words[0]), int(words[1]))))
        g.close()
        hip.close()
        assert max(float(np.abs(r[0]).max()) for r in res) > 1e-4, "silent"
        if name != "IN":
            assert len({r[2] for r in res}) >= 2 and any(r[2][0] for r in res), "the flag words never change: the envelopes do not finish"
        _SERIAL[key] = res
    return _SERIAL[key]


def overlapped_run(knh, monkeypatch, name, shape, launches, n_bufs=3, plan=tuple(PLAN), timing=False):
    """`launches` back-to-back calls on a stream of the caller's with no host sync; each launch's blocks are copied, device to
    device, on that stream right behind the call (hipMemcpyAsync: what a framework's copy or clone on its current stream
    enqueues).  -> (blocks per launch, done_frames, flag words, debug word 9, timing_read) after the last."""
    w = workload(name, *shape)
    g = bank(knh, monkeypatch, w, {})
    hip = Hip()
    s = hip.stream()
    bufs = [hip.zeros(MAX_BLOCKS * block_bytes(w)) for _ in range(n_bufs)]
    snaps = [hip.zeros(nb * block_bytes(w)) for nb in plan[:launches]]
    if timing:
        g.timing_reset(True)
    for k, nb in enumerate(plan[:launches]):
        events(g, w, k, nb)
        g.process_blocks_device(nb, bufs[k % n_bufs], s)
        hip.copy_on(s, snaps[k], bufs[k % n_bufs], nb * block_bytes(w))
    g.synchronize()
    timed = g.timing_read() if timing else None
    words = g.debug_words()
    done = g.read_done_frames().copy()
    outs = [hip.to_host(snaps[k], (nb, w.out_channels, w.block_size), np_dtype(w)) for k, nb in enumerate(plan[:launches])]
    g.close()
    hip.close()
    return outs, done, (int(words[0]), int(words[1])), int(words[9]), timed


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_six_launches_back_to_back(knh, monkeypatch, shape):
    """Three output buffers in turn, both sets of partial rows and all three sets of flag words: every launch's blocks, and
    after 1 .. 6 launches the done frames, the any-done word and the running count, as launch by launch."""
    ref = serial_run(knh, monkeypatch, "C3", shape)
    for launches in range(1, len(PLAN) + 1):
        outs, done, flags, overlapped, timed = overlapped_run(knh, monkeypatch, "C3", shape, launches, timing=launches == len(PLAN))
        print(f"{launches} launches: flags {flags} (serial {ref[launches - 1][2]}), {overlapped} overlapped, timing {timed}")
        assert overlapped == launches
        for k in range(launches):
            assert_bit_equal(outs[k], ref[k][0], f"launch {k} of {launches}", strict_zero=True)
        assert np.array_equal(done, ref[launches - 1][1]), f"done frames after {launches} launches"
        assert flags == ref[launches - 1][2], f"flag words after {launches} launches"
        if timed is not None:
            assert timed[1] == launches and timed[0] > 0.0, timed


def test_a_copy_on_the_caller_s_stream_sees_the_launch(knh, monkeypatch):
    """Stream order alone: the clone enqueued on the caller's stream behind one call, no host sync in between."""
    shape = SHAPES[0]
    ref = serial_run(knh, monkeypatch, "C3", shape)
    outs, _, _, overlapped, _ = overlapped_run(knh, monkeypatch, "C3", shape, 1)
    assert overlapped == 1
    assert_bit_equal(outs[0], ref[0][0], "the launch's blocks", strict_zero=True)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[6]], ids=[SHAPE_IDS[1], SHAPE_IDS[6]])
def test_one_output_buffer_for_every_launch(knh, monkeypatch, shape):
    """The fold of launch k + 1 writes the buffer the clone behind launch k reads: it waits for what the caller's stream held."""
    ref = serial_run(knh, monkeypatch, "C3", shape)
    outs, _, flags, overlapped, _ = overlapped_run(knh, monkeypatch, "C3", shape, len(PLAN), n_bufs=1)
    assert overlapped == len(PLAN)
    for k in range(len(PLAN)):
        assert_bit_equal(outs[k], ref[k][0], f"launch {k}", strict_zero=True)
    assert flags == ref[-1][2]


def test_launches_that_grow(knh, monkeypatch):
    """n_blocks 1, 1, 2, 3: both sets of rows exist and are in use when they are reallocated, twice."""
    shape, plan = SHAPES[2], (1, 1, 2, 3)
    ref = serial_run(knh, monkeypatch, "C3", shape, plan)
    outs, done, flags, overlapped, _ = overlapped_run(knh, monkeypatch, "C3", shape, len(plan), plan=plan)
    assert overlapped == len(plan)
    for k in range(len(plan)):
        assert_bit_equal(outs[k], ref[k][0], f"launch {k}", strict_zero=True)
    assert np.array_equal(done, ref[-1][1]) and flags == ref[-1][2]


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[7]], ids=[SHAPE_IDS[0], SHAPE_IDS[7]])
def test_a_blocking_host_call_right_behind_an_overlapped_launch(knh, monkeypatch, shape):
    """knh_bank_process_blocks keeps to one stream and fold_tree_kernel: it meets the bank's streams first."""
    def run(env):
        w = workload("C3", *shape)
        g = bank(knh, monkeypatch, w, env)
        hip = Hip()
        buf = hip.zeros(MAX_BLOCKS * block_bytes(w))
        res = []
        for k in range(2):
            events(g, w, 2 * k, 2)
            g.process_blocks_device(2, buf)
            if env:
                g.synchronize()
            events(g, w, 2 * k + 1, 3)
            res.append(g.process_blocks(3))
        overlapped = int(g.debug_words()[9])
        g.close()
        hip.close()
        return res, overlapped
    got, overlapped = run({})
    want, _ = run(SERIAL)
    assert overlapped == 2
    for k in range(2):
        assert_bit_equal(got[k][0], want[k][0], f"host blocks of call {k}", strict_zero=True)
        assert got[k][1] == want[k][1], f"flags of call {k}"
    assert float(np.abs(want[0][0]).max()) > 1e-4


@pytest.mark.parametrize("st", [L.F32, L.F64], ids=["f32", "f64"])
def test_a_pan2_chain(knh, monkeypatch, st):
    """Two planes of rows per block: the fold sees twice as many blocks of one channel each."""
    shape = (130, 96, st)
    ref = serial_run(knh, monkeypatch, "P3", shape)
    outs, done, flags, overlapped, _ = overlapped_run(knh, monkeypatch, "P3", shape, len(PLAN))
    assert overlapped == len(PLAN) and outs[0].shape[1] == 2
    for k in range(len(PLAN)):
        assert_bit_equal(outs[k], ref[k][0], f"launch {k}", strict_zero=True)
        assert not np.array_equal(outs[k][:, 0], outs[k][:, 1]), "left equals right"
    assert np.array_equal(done, ref[-1][1]) and flags == ref[-1][2]


@pytest.mark.parametrize("st", [L.F32, L.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_rows", [1, 2, 3, 5, 16, 17, 255, 256])
def test_the_fold_without_lds_alone(knh, monkeypatch, n_rows, st):
    """fold_tree_wave_kernel against fold_tree_kernel on the same rows, the way the fold tests of test_gpu_frame_banks.py
    reach the fold: a lane-per-frame bank hands it one row per voice (KNH_FOLD_WAVE=1 gives such a bank's single-stream fold the
    new form).  The rows are the signals of n_rows detuned FM voices; blocks of 80 frames: a full wavefront and a partial one,
    then a block in two calls (frame_begin inside a wavefront's 64 frames).  Bit for bit, and bit for bit the pairwise tree."""
    w = fc.cascade(fc.TREE_DEPTH, n_rows, 80, st)
    banks = []
    for env in ({"KNH_FOLD_WAVE": "1"}, {}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            banks.append(make_gpu(knh, w))
        assert int(banks[-1].debug_words()[2]) in (L.DEBUG_FORM_FRAME_JIT, L.DEBUG_FORM_FRAME_INTERP)
    new, old = banks
    calls = 0
    for b in range(2):
        o_new, v_new, _ = new.process_block_voices()
        o_old, v_old, _ = old.process_block_voices()
        assert_bit_equal(v_new, v_old, f"{n_rows} rows, block {b}: the rows themselves", strict_zero=True)
        assert_bit_equal(o_new, o_old, f"{n_rows} rows, block {b}: the two folds", strict_zero=True)
        assert_bit_equal(o_new[0], pairwise_sum(v_new), f"{n_rows} rows, block {b}: the pairwise tree", strict_zero=True)
        assert float(np.abs(o_new).max()) > 1e-3
        calls += 1
    for ftp, off in ((30, 0), (50, 30)):  # the block after, in two calls
        o_new, v_new, _ = new.process_block_voices(ftp, off)
        o_old, v_old, _ = old.process_block_voices(ftp, off)
        assert_bit_equal(o_new, o_old, f"{n_rows} rows: frames {off} .. {off + ftp}", strict_zero=True)
        assert_bit_equal(o_new[0, off:off + ftp], pairwise_sum(v_new)[off:off + ftp], f"{n_rows} rows: frames {off} .. {off + ftp}, the tree", strict_zero=True)
        calls += 1
    # debug word 10: the folds that took the form without LDS -- every one of the first bank's, none of the second's
    assert int(new.debug_words()[10]) == calls == 4 and int(old.debug_words()[10]) == 0, (new.debug_words()[:11], old.debug_words()[:11])
    new.close()
    old.close()


@pytest.mark.parametrize("st", [L.F32, L.F64], ids=["f32", "f64"])
def test_the_bank_s_input_uploaded_on_the_caller_s_stream(knh, monkeypatch, st):
    """A voice kernel on the bank's stream that reads the bank node's input waits for the caller's stream, where the input's
    upload was enqueued in this very call -- also when the launch before it was overlapped (the case in which it otherwise
    does not wait).  Every launch has input blocks of its own.  (A pipeline fused at init: its events are recorded around the
    kernel, not carried in its dispatch.)"""
    shape = (130, 96, st)
    ref = serial_run(knh, monkeypatch, "IN", shape)
    outs, _, _, overlapped, _ = overlapped_run(knh, monkeypatch, "IN", shape, len(PLAN))
    assert overlapped == len(PLAN)
    for k in range(len(PLAN)):
        assert_bit_equal(outs[k], ref[k][0], f"launch {k}", strict_zero=True)
        assert k == 0 or not np.array_equal(outs[k][0], outs[k - 1][0])


def test_voices_restarted_between_overlapped_launches(knh, monkeypatch):
    """knh_bank_restart_voices between two overlapped launches: the restart kernel goes to the caller's stream, and the voice
    kernel behind it waits for that stream."""
    shape = SHAPES[1]
    ref = serial_run(knh, monkeypatch, "RESTART", shape)
    plain = serial_run(knh, monkeypatch, "C3", shape)
    assert not np.array_equal(ref[2][0], plain[2][0]), "the restart is not heard"
    outs, done, flags, overlapped, _ = overlapped_run(knh, monkeypatch, "RESTART", shape, len(PLAN))
    assert overlapped == len(PLAN)
    for k in range(len(PLAN)):
        assert_bit_equal(outs[k], ref[k][0], f"launch {k}", strict_zero=True)
    assert np.array_equal(done, ref[-1][1]) and flags == ref[-1][2]
