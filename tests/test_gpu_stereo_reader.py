"""BufferReader<F, U2> on the device: one reader node, two output signals, interleaved two-channel Buffers in the pool
(knh_bank_add_buffer_interleaved, KNH_STAGE_FLAG_READER_CH1).  The expected planes are two oracle banks of one-channel
readers, one per de-interleaved plane (stereo_reader_ref.Planes; the premise is pinned in tests/test_stereo_reader_ref.py).
Everything is compared bit for bit, in exact mode (allow_fma = 0)."""
import numpy as np
import pytest

import sampler_pool as sp
import stereo_reader_ref as sr
from helpers import assert_bit_equal, make_oracle, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage
from test_stereo_reader_abi import LFO, LINKED, VOICES

pytestmark = pytest.mark.gpu

BOTH = [L.F32, L.F64]
SHAPES = [(3, 64), (65, 40), (130, 64)]  # voices (a partial wavefront, one past one, two and a bit), block size


def dtype_of(sample_type):
    return np.float64 if sample_type == L.F64 else np.float32


def scenario(n):
    """Three two-channel entries of 37, 64 and 200 frames, the voices spread over them; at block 1 a third of the voices move
    to the next entry (knh_bank_assign_buffers), at block 7 every fifth voice is restarted with other constructor arguments."""
    buffers = sr.make_stereo_buffers()
    ids = sr.spread_ids(n)
    v = np.arange(n)
    moved = v[(v % 3 != 2) & (v % 2 == 0)]
    return buffers, ids, moved, v[::5], sr.stereo_traffic(n, sr.lengths(buffers, ids))


_REFERENCE = {}


def reference(oracle, n, bs, sample_type, gain):
    """[(planes [2, n, bs], done [n], every reader finished)] per block of the scenario: computed once, shared, read-only."""
    key = (n, bs, sample_type, gain)
    if key not in _REFERENCE:
        buffers, ids, moved, again, ev = scenario(n)
        x = sr.Planes(oracle, n, bs, sample_type, buffers, ids, sr.stereo_ctor(n), ev, gain=gain)
        finished = np.zeros(n, dtype=bool)
        blocks = []
        for b in range(sr.BLOCKS):
            if b == 1 and len(moved):
                x.reassign(b, moved, (ids[moved] + 1).astype(np.uint32), sr.stereo_ctor(n, 5)[moved])
                finished[moved] = False
            if b == 7:
                x.reassign(b, again, x.ids[again], sr.stereo_ctor(n, 9)[again])
                finished[again] = False
            if b in (5, 10):  # t_restart on every voice
                finished[:] = False
            planes, done = x.step(b)
            finished |= done != sr.NOT_DONE
            planes.setflags(write=False)
            done.setflags(write=False)
            blocks.append((planes, done, bool(finished.all())))
        x.close()
        _REFERENCE[key] = tuple(blocks)
    return _REFERENCE[key]


def drive(g, n, b, ids, moved, again, ev, **kw):
    """The scenario's calls of block b on a device bank (reader stage 0)."""
    if b == 1 and len(moved):
        g.assign_buffers(0, moved.astype(np.uint32), (ids[moved] + 1).astype(np.uint32), sr.stereo_ctor(n, 5)[moved])
    if b == 7:
        g.set_voice_ctor_args(0, again.astype(np.uint32), sr.stereo_ctor(n, 9)[again])
        g.restart_voices(again.astype(np.uint32))
    ev(b, g, **kw)


@pytest.mark.parametrize("sample_type", BOTH)
@pytest.mark.parametrize("n,bs", SHAPES)
def test_planes_done_frames_flags_and_both_mixes(knh, oracle, n, bs, sample_type):
    """reader -> CH1 -> a MUL_CONST per channel -> connected outputs, twelve blocks of rate / duration_s / start_s / t_restart /
    end_s / looping traffic, a swap of voices to another entry and a restart: the per-voice planes [2][n][bs], the done
    frames, ANY_DONE / ALL_DONE, the left-fold mix (numpy's sequential sum per channel) and the tree mix (pairwise)."""
    gain = 1.0 / n
    ref = reference(oracle, n, bs, sample_type, gain)
    assert any((d != sr.NOT_DONE).any() for _, d, _ in ref) and max(float(np.abs(p).max()) for p, _, _ in ref) > 1e-4
    buffers, ids, moved, again, ev = scenario(n)
    fold = sr.stereo_bank(knh, n, bs, sample_type, buffers, ids, sr.stereo_ctor(n), L.MIX_LEFT_FOLD, gain=gain)
    tree = sr.stereo_bank(knh, n, bs, sample_type, buffers, ids, sr.stereo_ctor(n), L.MIX_TREE, gain=gain)
    assert fold.debug_signature() == "T@_,_,0,1m@0,_,0m@1,_,1#2:0,1"
    for b, (planes, done, all_done) in enumerate(ref):
        drive(fold, n, b, ids, moved, again, ev)
        drive(tree, n, b, ids, moved, again, ev)
        out, voices, flags = fold.process_block_voices()
        print(f"block {b}: samples differing {int(np.count_nonzero(voices != planes))}, done {int(np.count_nonzero(done != sr.NOT_DONE))}, flags {flags}")
        assert voices.shape == (2, n, bs)
        for c in range(2):
            assert_bit_equal(voices[c], planes[c], f"block {b} plane {c}")
            assert_bit_equal(out[c], sp.left_fold(planes[c]), f"block {b} left-fold mix, channel {c}")
        np.testing.assert_array_equal(fold.read_done_frames(), done, err_msg=f"block {b} done frames")
        assert bool(flags & L.FLAG_ANY_DONE) == bool((done != sr.NOT_DONE).any()), f"block {b} ANY_DONE"
        assert bool(flags & L.FLAG_ALL_DONE) == all_done, f"block {b} ALL_DONE"
        t_out, t_flags = tree.process_block()  # (the call the reference makes, once per block)
        for c in range(2):
            assert_bit_equal(t_out[c], pairwise_sum(planes[c]), f"block {b} tree mix, channel {c}")
        assert t_flags == flags
    fold.close()
    tree.close()


@pytest.mark.parametrize("sample_type", BOTH)
def test_every_reader_finished_is_all_done(knh, oracle, sample_type):
    """One-shot voices only: ALL_DONE from the block in which the last reader ends (one done mark per node, not per channel)."""
    n, bs = 65, 40
    buffers = sr.make_stereo_buffers()
    ids = sr.spread_ids(n)
    ctor = sr.stereo_ctor(n)
    ctor[:, 1] = 0.0
    x = sr.Planes(oracle, n, bs, sample_type, buffers, ids, ctor, lambda block, bank: None)
    g = sr.stereo_bank(knh, n, bs, sample_type, buffers, ids, ctor, L.MIX_LEFT_FOLD, stages=VOICES["raw"][0], outs=VOICES["raw"][1])
    finished = np.zeros(n, dtype=bool)
    seen_all = False
    for b in range(24):
        planes, done = x.step(b)
        finished |= done != sr.NOT_DONE
        _, voices, flags = g.process_block_voices()
        for c in range(2):
            assert_bit_equal(voices[c], planes[c], f"block {b} plane {c}")
        np.testing.assert_array_equal(g.read_done_frames(), done)
        assert bool(flags & L.FLAG_ALL_DONE) == bool(finished.all()), f"block {b}"
        seen_all = seen_all or bool(finished.all())
    assert seen_all
    x.close()
    g.close()


@pytest.mark.parametrize("sample_type", BOTH)
@pytest.mark.parametrize("name", ["swapped", "ch1_alone", "fold_down"])
def test_the_second_output_is_a_signal_like_any_other(knh, oracle, name, sample_type):
    """connect_outputs(ch1, ch0): the planes change places.  CH1 as the last stage of an unconnected voice: the voice's one
    signal is plane 1.  MATH_ADD of both channels: plane 0 + plane 1 in the bank's precision."""
    n, bs = 65, 40
    ref = reference(oracle, n, bs, sample_type, 1.0)
    buffers, ids, moved, again, ev = scenario(n)
    stages, outs = VOICES[name]
    g = sr.stereo_bank(knh, n, bs, sample_type, buffers, ids, sr.stereo_ctor(n), L.MIX_LEFT_FOLD, stages=stages, outs=outs)
    for b, (planes, done, _) in enumerate(ref):
        drive(g, n, b, ids, moved, again, ev)
        out, voices, _ = g.process_block_voices()
        if name == "swapped":
            assert_bit_equal(voices[0], planes[1], f"block {b} left = plane 1")
            assert_bit_equal(voices[1], planes[0], f"block {b} right = plane 0")
            assert_bit_equal(out[0], sp.left_fold(planes[1]), f"block {b} mix")
        else:
            want = planes[1] if name == "ch1_alone" else planes[0] + planes[1]
            assert voices.shape == (n, bs)
            assert_bit_equal(voices, want, f"block {b} per-voice")
            assert_bit_equal(out[0], sp.left_fold(want), f"block {b} mix")
            assert_bit_equal(out[1], out[0], "L == R")
        np.testing.assert_array_equal(g.read_done_frames(), done, err_msg=f"block {b} done frames")
    g.close()


@pytest.mark.parametrize("sample_type", BOTH)
@pytest.mark.parametrize("n,bs", [(3, 40), (130, 64)])
def test_a_mono_reader_on_a_two_channel_pool_plays_channel_0(knh, oracle, n, bs, sample_type):
    """BufferReader<F, U1> on a stereo Buffer (index * num_channels + 0): reader -> MUL_CONST without a CH1 stage equals the
    oracle on plane 0 -- the chain forms (130 voices: a fused pipeline) as well as a single group."""
    gain = 1.0 / n
    ref = reference(oracle, n, bs, sample_type, gain)
    buffers, ids, moved, again, ev = scenario(n)
    g = sr.stereo_bank(knh, n, bs, sample_type, buffers, ids, sr.stereo_ctor(n), L.MIX_LEFT_FOLD, stages=sp.STAGES, outs=None, gain=gain)
    for b, (planes, done, _) in enumerate(ref):
        drive(g, n, b, ids, moved, again, ev)
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, planes[0], f"block {b} per-voice")
        assert_bit_equal(out[0], sp.left_fold(planes[0]), f"block {b} mix")
        np.testing.assert_array_equal(g.read_done_frames(), done, err_msg=f"block {b} done frames")
    assert "C" in g.debug_signature() and "F" not in g.debug_signature()
    g.close()


@pytest.mark.parametrize("sample_type", BOTH)
@pytest.mark.parametrize("n", [3, 65])
def test_linked_rate(knh, oracle, n, sample_type):
    """ar_param = 1: the stereo reader's rate driven by SinWt(slow) * depth + offset.  Both planes against two oracle
    WrArParams readers driven by the same signal; a one-shot voice marks done at frame 0."""
    bs, blocks = 40, 10
    (samples, rate), = sr.make_stereo_buffers([(200, 44100.0)])
    p = configs.voice_parameters(n)
    v = np.arange(n, dtype=np.uint32)
    dctor = {0: (p["freq"] * 0.05).reshape(n, 1), 1: np.full((n, 1), 0.8), 2: np.ones((n, 1))}
    reader_ctor = np.stack([np.ones(n), (v % 2).astype(np.float64), np.zeros(n)], axis=1)
    planes = []
    for c in range(2):
        w = configs.Workload("linked", LFO + [Stage(L.STAGE_BUFFER_READER, ar_param=1, input2=3), Stage(L.STAGE_MUL_CONST)], n, bs, sample_type, 1)
        w.ctor = dict(dctor)
        w.ctor.update({3: reader_ctor, 4: np.ones((n, 1))})
        w.buffer = (3, np.ascontiguousarray(samples[:, c]), rate)
        planes.append(make_oracle(oracle, w, want_mix=False))
    g = knh.VoiceBank(LINKED, n, sample_type, 2, L.MIX_LEFT_FOLD)
    for s, a in dctor.items():
        g.set_ctor_args(s, a)
    g.set_ctor_args(3, reader_ctor)
    assert g.add_buffer(3, samples, rate, channels=2) == 0
    g.connect_outputs(3, 4)
    g.init(configs.SAMPLE_RATE, bs)
    seen = set()
    for b in range(blocks):
        if b == 6:
            g.param_apply_many(v, 3, 5, L.VALUE_TRIGGER)
            for o in planes:
                o.param_apply_many(v, 3, 5, L.VALUE_TRIGGER)
        _, voices, _ = g.process_block_voices()
        for c in range(2):
            _, rows, _, done = planes[c].process_block()
            assert_bit_equal(voices[c], rows, f"block {b} plane {c}")
            np.testing.assert_array_equal(g.read_done_frames(), done, err_msg=f"block {b} done frames")
        seen |= set(np.unique(done).tolist())
    assert seen == {0, sr.NOT_DONE}
    g.close()
    for o in planes:
        o.close()


@pytest.mark.parametrize("sample_type", BOTH)
def test_smoothed_rate(knh, oracle, sample_type):
    """KNH_STAGE_FLAG_SMOOTH_PARAMS on the stereo reader: one block-rate ramp of the rate (the host's), retargeted mid-ramp."""
    n, bs = 65, 40
    buffers = sr.make_stereo_buffers()
    ids = sr.spread_ids(n)
    ctor = sr.stereo_ctor(n)
    ctor[:, 1] = 1.0  # looping: the ramp is heard to its end
    v = np.arange(n, dtype=np.uint32)

    def ev(block, bank):
        if block == 1:
            bank.param_apply_many(v, 0, 0, L.VALUE_SMOOTHING, np.full(n, 0.004), np.ones(n, dtype=np.int64))  # rate: 4 ms, linear
            bank.param_apply_many(v, 0, 0, L.VALUE_FLOAT, 0.5 + 0.02 * v)
        if block == 4:
            bank.param_apply_many(v[::2], 0, 0, L.VALUE_FLOAT, 1.5 - 0.01 * v[::2])
    stages, outs = VOICES["smooth"]
    x = sr.Planes(oracle, n, bs, sample_type, buffers, ids, ctor, ev, flags=L.STAGE_FLAG_SMOOTH_PARAMS)
    g = sr.stereo_bank(knh, n, bs, sample_type, buffers, ids, ctor, L.MIX_LEFT_FOLD, stages=stages, outs=outs)
    for b in range(10):
        planes, done = x.step(b)
        ev(b, g)
        _, voices, _ = g.process_block_voices()
        for c in range(2):
            assert_bit_equal(voices[c], planes[c], f"block {b} plane {c}")
        np.testing.assert_array_equal(g.read_done_frames(), done)
    x.close()
    g.close()


@pytest.mark.parametrize("sample_type", BOTH)
def test_launches_cut_differently_render_the_same(knh, oracle, sample_type):
    """One launch of three blocks against block by block; 64-frame blocks cut 40 + 24 against single calls; the per-block
    call (knh_bank_process_block) against the launch (knh_bank_process_blocks).  The tree mix, per channel."""
    n, bs = 130, 64
    gain = 1.0 / n
    ref = reference(oracle, n, bs, sample_type, gain)
    buffers, ids, moved, again, ev = scenario(n)
    make = lambda mix: sr.stereo_bank(knh, n, bs, sample_type, buffers, ids, sr.stereo_ctor(n), mix, gain=gain)
    per_block, launches, cut = make(L.MIX_TREE), make(L.MIX_TREE), make(L.MIX_LEFT_FOLD)
    # (a swap or a restart lands between launches: blocks 1 and 7 begin launches of their own)
    for group in ([0], [1, 2], [3, 4, 5], [6], [7, 8], [9, 10, 11]):
        drive(launches, n, group[0], ids, moved, again, ev)
        for j, b in enumerate(group[1:], start=1):
            ev(b, launches, block_offset=j)
        outs, _ = launches.process_blocks(len(group))
        for j, b in enumerate(group):
            planes = ref[b][0]
            drive(per_block, n, b, ids, moved, again, ev)
            out, _ = per_block.process_block()
            for c in range(2):
                assert_bit_equal(out[c], pairwise_sum(planes[c]), f"per-block call, block {b} channel {c}")
                assert_bit_equal(outs[j][c], out[c], f"launch of {len(group)}, block {b} channel {c}")
            drive(cut, n, b, ids, moved, again, ev)
            o1, v1, _ = cut.process_block_voices(40, 0)
            o2, v2, _ = cut.process_block_voices(24, 40)
            whole = np.concatenate([v1[:, :, :40], v2[:, :, 40:]], axis=2)
            for c in range(2):
                assert_bit_equal(whole[c], planes[c], f"40 + 24, block {b} plane {c}")
                assert_bit_equal(np.concatenate([o1[c, :40], o2[c, 40:]]), sp.left_fold(planes[c]), f"40 + 24, block {b} mix {c}")
    for g in (per_block, launches, cut):
        g.close()


@pytest.mark.parametrize("how", ["host_threads", "two_devices"])
def test_two_voice_ranges_render_the_plain_banks_voices(knh, oracle, how):
    """host_threads = 2, and two "devices" on device 0: every range holds the whole two-channel pool; the per-voice planes are
    the plain bank's (the oracle's) bit for bit, the mix is the ranges' tree mixes added in range order."""
    n, bs, sample_type = 130, 64, L.F32
    gain = 1.0 / n
    ref = reference(oracle, n, bs, sample_type, gain)
    buffers, ids, moved, again, ev = scenario(n)
    kw = {"host_threads": 2} if how == "host_threads" else {"devices": [0, 0]}
    g = sr.stereo_bank(knh, n, bs, sample_type, buffers, ids, sr.stereo_ctor(n), L.MIX_TREE, gain=gain, **kw)
    assert g.ranks() == 2 and g.buffer_count(0) == 3
    for b, (planes, done, _) in enumerate(ref):
        drive(g, n, b, ids, moved, again, ev)
        out, voices, _ = g.process_block_voices()
        for c in range(2):
            assert_bit_equal(voices[c], planes[c], f"{how} block {b} plane {c}")
            # ranges of whole 64-voice groups: 128 + 2 voices
            assert_bit_equal(out[c], pairwise_sum(planes[c][:128]) + pairwise_sum(planes[c][128:]), f"{how} block {b} mix {c}")
        np.testing.assert_array_equal(g.read_done_frames(), done)
    g.close()


@pytest.mark.parametrize("kw", [{}, {"host_threads": 2}])
def test_a_second_output_on_a_one_channel_pool_fails_init(knh, kw):
    (stereo, rate), = sr.make_stereo_buffers([(37, 44100.0)])
    b = knh.VoiceBank(sr.STEREO, 130, L.F32, 2, **kw)
    b.connect_outputs(*sr.STEREO_OUTS)
    b.add_buffer(0, np.ascontiguousarray(stereo[:, 0]), rate)
    with pytest.raises(L.KnasterHipError) as e:
        b.init(configs.SAMPLE_RATE, 64)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "two-channel" in str(e.value)
    b.close()


def test_a_refused_init_leaves_the_signature_and_the_forms_as_they_were(knh):
    """On a two-channel pool knh_bank_init turns a mono reader's 'F' into 'C' -- only if it gets to its end: an init refused
    later (here: a reader wrapped in WrPreciseTiming) leaves debug_signature() what it was."""
    (stereo, rate), = sr.make_stereo_buffers([(37, 44100.0)])
    b = knh.VoiceBank([Stage(L.STAGE_BUFFER_READER, delayed_changes_per_block=2), Stage(L.STAGE_MUL_CONST)], 130, L.F32, 2)
    b.add_buffer(0, stereo, rate, channels=2)
    before = (b.debug_signature(), b.buffer_count(0))
    assert before[0] == "Fm"
    with pytest.raises(L.KnasterHipError) as e:
        b.init(configs.SAMPLE_RATE, 64)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "WrPreciseTiming" in str(e.value)
    assert (b.debug_signature(), b.buffer_count(0)) == before
    b.close()
