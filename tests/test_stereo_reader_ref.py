"""The premise of the stereo reader tests, pinned without a GPU: an independent numpy restatement of BufferReader<F, U2> on
INTERLEAVED two-channel Buffers (stereo_reader_ref.InterleavedReader) renders, bit for bit, what two oracle banks of
one-channel readers render on the two de-interleaved planes -- samples, done frames, under the whole parameter traffic,
across swaps to other pool entries, in f32 and f64; and the same for a reader whose rate is linked to a signal (the
per-sample `process` path, which marks done at frame 0).  tests/test_gpu_stereo_reader.py compares the device with those two
oracle banks."""
import numpy as np
import pytest

import stereo_reader_ref as sr
from helpers import assert_bit_equal, make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

BOTH = [L.F32, L.F64]


def dtype_of(sample_type):
    return np.float64 if sample_type == L.F64 else np.float32


def test_traffic_stays_inside_the_buffers():
    """Every start_s / duration_s / end_s of the shared traffic leaves end_frame <= n_frames for every voice on every entry
    (the restatement asserts it after each call), and the restatement's index never reaches n_frames while it renders."""
    n = 130
    buffers = sr.make_stereo_buffers()
    ids = sr.spread_ids(n)
    r = sr.InterleavedReader(np.float64, configs.SAMPLE_RATE, buffers, ids, sr.stereo_ctor(n))
    r.check_in_range()
    ev = sr.stereo_traffic(n, sr.lengths(buffers, ids))
    wrapped = False
    for b in range(sr.BLOCKS):
        ev(b, r)
        before = r.rp.copy()
        r.process_block(40)
        wrapped = wrapped or bool(((before >= r.nf - 1) & (before < r.nf)).any())
    assert wrapped, "some block starts with a read pointer in the last frame: the i + 1 == n wrap is exercised"
    with pytest.raises(AssertionError):
        r.param_apply_many(np.arange(n), 0, 4, L.VALUE_FLOAT, sr.lengths(buffers, ids) * 1.5)  # an end_s past the end is caught


@pytest.mark.parametrize("sample_type", BOTH)
@pytest.mark.parametrize("n,bs", [(3, 64), (65, 40), (130, 64)])
def test_interleaved_restatement_equals_two_oracle_planes(oracle, n, bs, sample_type):
    """process_block: twelve blocks of the shared traffic on three two-channel Buffers of 37, 64 and 200 frames; at block 1 a
    third of the voices move to the next entry (fresh readers), at block 7 every fifth voice is restarted on its own entry."""
    buffers = sr.make_stereo_buffers()
    ids = sr.spread_ids(n)
    ctor = sr.stereo_ctor(n)
    ev = sr.stereo_traffic(n, sr.lengths(buffers, ids))
    # (the traffic's times are fractions of the length of the Buffer each voice STARTED on: moved voices go to a longer or
    # equal one -- 37 -> 64 -> 200 frames -- or, from the 200-frame entry, stay; end_frame <= n_frames still holds, asserted)
    v = np.arange(n)
    moved = v[(v % 3 != 2) & (v % 2 == 0)]
    again = v[::5]
    ref = sr.InterleavedReader(dtype_of(sample_type), configs.SAMPLE_RATE, buffers, ids, ctor)
    x = sr.Planes(oracle, n, bs, sample_type, buffers, ids, ctor, ev)
    any_done = loud = differ = False
    for b in range(sr.BLOCKS):
        if b == 1 and len(moved):
            new_ids = (ids[moved] + 1).astype(np.uint32)
            ref.construct(moved, new_ids, sr.stereo_ctor(n, 5)[moved])
            x.reassign(b, moved, new_ids, sr.stereo_ctor(n, 5)[moved])
        if b == 7:
            ref.construct(again, x.ids[again], sr.stereo_ctor(n, 9)[again])
            x.reassign(b, again, x.ids[again], sr.stereo_ctor(n, 9)[again])
        ev(b, ref)
        got, got_done = ref.process_block(bs)
        want, want_done = x.step(b)
        for c in range(2):
            assert_bit_equal(got[c], want[c], f"block {b} plane {c}")
        np.testing.assert_array_equal(got_done, want_done, err_msg=f"block {b} done frames")
        any_done = any_done or bool((want_done != sr.NOT_DONE).any())
        loud = loud or float(np.abs(want).max()) > 1e-3
        differ = differ or not np.array_equal(want[0], want[1])
    x.close()
    assert any_done and loud and differ  # (the two planes carry different signals)


@pytest.mark.parametrize("sample_type", BOTH)
def test_linked_rate_restatement_equals_two_oracle_planes(oracle, sample_type):
    """A reader pushed as .ar_params() with its rate linked to SinWt(slow) * depth + offset: the per-sample path.  The driver
    comes from an oracle bank of the three driver stages; a one-shot voice marks done at frame 0."""
    n, bs, blocks = 65, 40, 10
    dtype = dtype_of(sample_type)
    (samples, rate), = sr.make_stereo_buffers([(200, 44100.0)])
    p = configs.voice_parameters(n)
    v = np.arange(n)
    drv = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST)]
    dctor = {0: (p["freq"] * 0.05).reshape(n, 1), 1: np.full((n, 1), 0.8), 2: np.ones((n, 1))}
    reader_ctor = np.stack([np.ones(n), (v % 2).astype(np.float64), np.zeros(n)], axis=1)

    w = configs.Workload("drv", drv, n, bs, sample_type, 1)
    w.ctor, w.buffer = dctor, None
    driver = make_oracle(oracle, w, want_mix=False)
    planes = []
    for c in range(2):
        w = configs.Workload("linked", drv + [Stage(L.STAGE_BUFFER_READER, ar_param=1, input2=3), Stage(L.STAGE_MUL_CONST)], n, bs, sample_type, 1)
        w.ctor = dict(dctor)
        w.ctor.update({3: reader_ctor, 4: np.ones((n, 1))})
        w.buffer = (3, np.ascontiguousarray(samples[:, c]), rate)
        planes.append(make_oracle(oracle, w, want_mix=False))
    ref = sr.InterleavedReader(dtype, configs.SAMPLE_RATE, [(samples, rate)], np.zeros(n, dtype=np.int64), reader_ctor, linked=True)
    seen = set()
    for b in range(blocks):
        if b == 6:  # t_restart on every voice: the one-shots play (and end) again
            ref.param_apply_many(v, 0, 5, L.VALUE_TRIGGER)
            for o in planes:
                o.param_apply_many(v.astype(np.uint32), 3, 5, L.VALUE_TRIGGER)
        _, d_rows, _, _ = driver.process_block()
        got, got_done = ref.process_block(bs, d_rows)
        for c in range(2):
            _, rows, _, done = planes[c].process_block()
            assert_bit_equal(got[c], rows, f"block {b} plane {c}")
            np.testing.assert_array_equal(got_done, done, err_msg=f"block {b} done frames")
        seen |= set(np.unique(got_done).tolist())
    assert seen == {0, sr.NOT_DONE}
    driver.close()
    for o in planes:
        o.close()
