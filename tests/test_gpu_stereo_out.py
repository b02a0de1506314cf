"""Stereo voices on the device: two of a voice's signals connected to graph outputs 0 and 1 (knh_bank_connect_outputs).
The left plane of a connected bank is what the oracle renders for the descriptor cut after the left node
(stages[:node_output(l) + 1]), the right plane the same with r; every parameter call goes to the GPU bank and to the views
that hold its stage.  Every sample of every voice is compared, bit for bit; the tree mix is helpers.pairwise_sum of each
plane, the left-fold mix numpy's sequential sum.  Sizes: 70 voices (a full wavefront and one with 6 live lanes) and 1;
blocks of 100 frames (whole visits, an 8-sample visit and a sample-by-sample tail) and 64; three blocks; f32 and f64."""
import numpy as np
import pytest

import stereo_cases as sc
from helpers import assert_bit_equal, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

pytestmark = pytest.mark.gpu

NOT_DONE = 0xFFFFFFFF
SHAPES = [(70, 100), (1, 100), (70, 64), (1, 64)]
TYPES = [L.F32, L.F64]
MIXES = [L.MIX_TREE, L.MIX_LEFT_FOLD]


def left_fold(plane):
    acc = plane[0].copy()
    for k in range(1, plane.shape[0]):
        acc = acc + plane[k]
    return acc


def expected_mix(planes, mix_mode):
    return np.stack([pairwise_sum(p) if mix_mode == L.MIX_TREE else left_fold(p) for p in planes])


def gpu_bank(knh, case, n, bs, sample_type, mix_mode, connect="case", ctor=None, **kw):
    b = knh.VoiceBank(case.stages, n, sample_type, 2, mix_mode, **kw)
    for s, a in (ctor or case.ctor).items():
        b.set_ctor_args(s, a)
    if connect == "case":
        connect = case.connect
    if connect is not None:
        b.connect_outputs(*connect)
    b.init(configs.SAMPLE_RATE, bs)
    return b


def oracle_view(oracle, case, n, bs, sample_type, stage, ctor=None):
    """The oracle's voices for the descriptor cut after the node of `stage`."""
    k = sc.node_output(case.stages, stage) + 1
    o = oracle.OracleBank(case.stages[:k], n, sample_type, 1, False, True)
    for s, a in (ctor or case.ctor).items():
        if s < k:
            o.set_ctor_args(s, a)
    o.init(configs.SAMPLE_RATE, bs)
    return o


class Rig:
    """A connected GPU bank and the two oracle views; a call goes to the bank and to each view that holds its stage."""

    def __init__(self, knh, oracle, case, n, bs, sample_type, mix_mode, connect=None, **kw):
        self.case, self.n, self.bs, self.mix_mode = case, n, bs, mix_mode
        self.connect = case.connect if connect is None else connect
        self.g = gpu_bank(knh, case, n, bs, sample_type, mix_mode, self.connect, **kw)
        self.views = [oracle_view(oracle, case, n, bs, sample_type, s) for s in self.connect]
        self.done = [np.full(n, NOT_DONE, dtype=np.uint32)] * 2

    def _targets(self, stage):
        return [self.g] + [o for o in self.views if stage < len(o.stages)]

    def param_apply_many(self, voices, stage, param, kind, fvalues=None):
        for t in self._targets(stage):
            t.param_apply_many(voices, stage, param, kind, fvalues)

    def param_apply(self, voice, stage, param, value):
        for t in self._targets(stage):
            t.param_apply(voice, stage, param, value)

    def set_delay_within_block_for_param(self, voice, stage, param, delay):
        for t in self._targets(stage):
            t.set_delay_within_block_for_param(voice, stage, param, delay)

    def events(self, block):
        if block == 0:
            v = np.arange(self.n, dtype=np.uint32)
            for e in self.case.envelopes:
                self.param_apply_many(v, e, 3, L.VALUE_TRIGGER)  # t_restart
        self.case.events(block, self)

    def oracle_planes(self):
        planes = []
        for k, o in enumerate(self.views):
            _, voices, _, done = o.process_block()
            planes.append(voices)
            self.done[k] = done
        return np.stack(planes)

    def step(self, block, what):
        """One block: the calls in front of it, then planes and mix against the views.  -> (planes, flags)"""
        self.events(block)
        want = self.oracle_planes()
        out, planes, flags = self.g.process_block_voices()
        assert_bit_equal(planes, want, f"{what} block {block}: per-voice planes (left, right)")
        assert_bit_equal(out, expected_mix(want, self.mix_mode), f"{what} block {block}: the mix of each plane")
        return want, flags

    def close(self):
        self.g.close()
        for o in self.views:
            o.close()


def run_case(knh, oracle, name, n, bs, sample_type, check=None, blocks=3):
    peak = np.zeros(2)
    for mix_mode in MIXES:
        rig = Rig(knh, oracle, sc.CASES[name](n), n, bs, sample_type, mix_mode)
        for b in range(blocks):
            planes, flags = rig.step(b, f"case {name} n={n} bs={bs} mix {mix_mode}")
            peak = np.maximum(peak, np.abs(planes).max(axis=(1, 2)))
            if check:
                check(rig, b, flags)
        rig.close()
    assert (peak > 1e-3).all(), f"a silent plane proves nothing: {peak}"
    return peak


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n,bs", SHAPES)
@pytest.mark.parametrize("name", ["A", "B", "D", "E", "H", "I"])
def test_planes_and_mixes_equal_the_two_oracle_views(knh, oracle, name, n, bs, sample_type):
    """A: two oscillators, one per side.  B: a plain chain whose left signal must survive the in-place filter.  D: dry left,
    delayed right (the ring stage beside a held slot).  E: an audio-rate link on the left.  H: oscillators and arithmetic
    only -- connected, the voice is fused like any graph.  I: WrPreciseTiming changes at frames 5 and 37 of block 1."""
    run_case(knh, oracle, name, n, bs, sample_type)


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n,bs", SHAPES)
def test_two_envelopes_done_frame_is_the_left_views(knh, oracle, n, bs, sample_type):
    """C: both envelopes end in block 1, at different frames.  The reference's task order for two connected outputs runs the
    right output's subtree first, then what only the left reads: the last mark_done of the block is the left envelope's.
    (The right VIEW holds the left envelope too, as a node nothing reads, so its done frame says nothing about the right
    envelope: that one is taken from the right side rendered alone -- oscillator, its filter, its envelope, as a chain.)"""
    case = sc.case_c(n)
    v = np.arange(n, dtype=np.uint32)
    right_done = []
    for mix_mode in MIXES:
        alone = oracle.OracleBank([case.stages[0], Stage(L.STAGE_SVF), case.stages[4]], n, sample_type, 1, False, True)
        for k, s in enumerate((0, 3, 4)):
            alone.set_ctor_args(k, case.ctor[s])
        alone.init(configs.SAMPLE_RATE, bs)
        rig = Rig(knh, oracle, case, n, bs, sample_type, mix_mode)
        for b in range(3):
            if b < 2:
                alone.param_apply_many(v, 2, 3 if b == 0 else 2, L.VALUE_TRIGGER)  # t_restart, then t_release
            _, alone_voices, _, dr = alone.process_block()
            planes, flags = rig.step(b, f"case C n={n} bs={bs} mix {mix_mode}")
            assert_bit_equal(planes[1], alone_voices, f"block {b}: the right plane is the right side rendered alone")
            dl = rig.done[0]
            got = rig.g.read_done_frames()
            if b == 1:
                assert (dl != NOT_DONE).all() and (dr != NOT_DONE).all() and (dl != dr).all(), "both end in block 1, at different frames"
                np.testing.assert_array_equal(got, dl)
                assert flags & L.FLAG_ANY_DONE
                right_done.append(dr)
            else:
                assert (dl == NOT_DONE).all() and (dr == NOT_DONE).all()
                np.testing.assert_array_equal(got, dl)
            if b == 2:
                assert flags & L.FLAG_ALL_DONE
        rig.close()
        alone.close()
    assert len(right_done) == len(MIXES)


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n,bs", SHAPES)
def test_an_output_that_feeds_the_other_is_not_a_root_of_the_search(knh, oracle, n, bs, sample_type):
    """M: left = E3(osc2) + E1(osc0), right = E1(osc0), both envelopes ending in block 1 (E3 first).  The reference pushes the
    deepest output node each output edge leads to (get_deepest_output_node, graph.rs:1984-2040): E1's walk forward ends at
    the sum, which is pushed already, so the search starts from the sum alone -- E3's side first, then E1's -- and the
    block's last mark_done is E1's.  That is the order of the left view (the whole graph, one output): its done frame."""
    case = sc.case_m(n)
    v = np.arange(n, dtype=np.uint32)
    for mix_mode in MIXES:
        e3 = oracle.OracleBank([case.stages[2], case.stages[3]], n, sample_type, 1, False, True)  # E3's side alone: its done frame
        e3.set_ctor_args(0, case.ctor[2])
        e3.set_ctor_args(1, case.ctor[3])
        e3.init(configs.SAMPLE_RATE, bs)
        rig = Rig(knh, oracle, case, n, bs, sample_type, mix_mode)
        peak = np.zeros(2)
        for b in range(3):
            if b < 2:
                e3.param_apply_many(v, 1, 3 if b == 0 else 2, L.VALUE_TRIGGER)
            d3 = e3.process_block()[3]
            planes, flags = rig.step(b, f"case M n={n} bs={bs} mix {mix_mode}")
            peak = np.maximum(peak, np.abs(planes).max(axis=(1, 2)))
            dl, d1 = rig.done  # the whole graph's; E1's (the right view is osc0 and E1)
            got = rig.g.read_done_frames()
            if b == 1:
                assert (d1 != NOT_DONE).all() and (d3 != NOT_DONE).all() and (d3 < d1).all(), "both end in block 1, E3 first"
                np.testing.assert_array_equal(dl, d1)
                assert flags & L.FLAG_ANY_DONE
            else:
                assert (dl == NOT_DONE).all() and (d3 == NOT_DONE).all()
            np.testing.assert_array_equal(got, dl)
            if b == 2:
                assert flags & L.FLAG_ALL_DONE
        assert peak.min() > 1e-3
        rig.close()
        e3.close()


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n,bs", SHAPES)
def test_one_stage_twice_and_the_default(knh, oracle, n, bs, sample_type):
    """F: connect(k, k) for an inner k: both planes equal view k.  connect(last, last): bit-equal, in shape too, to a bank
    never connected."""
    case = sc.case_a(n)
    for mix_mode in MIXES:
        rig = Rig(knh, oracle, case, n, bs, sample_type, mix_mode, connect=(1, 1))
        for b in range(3):
            planes, _ = rig.step(b, f"connect(1, 1) mix {mix_mode}")
            assert_bit_equal(planes[0], planes[1], "both planes are view 1")
        rig.close()
        never = gpu_bank(knh, case, n, bs, sample_type, mix_mode, connect=None)
        again = gpu_bank(knh, case, n, bs, sample_type, mix_mode, connect=(3, 3))
        back = knh.VoiceBank(case.stages, n, sample_type, 2, mix_mode)  # connected, then restored
        for s, a in case.ctor.items():
            back.set_ctor_args(s, a)
        back.connect_outputs(1, 3)
        back.connect_outputs(3, 3)
        back.init(configs.SAMPLE_RATE, bs)
        assert never.debug_signature() == again.debug_signature() == back.debug_signature()
        for b in range(3):
            o0, v0, f0 = never.process_block_voices()
            for other in (again, back):
                o1, v1, f1 = other.process_block_voices()
                assert v0.shape == (n, bs) and v1.shape == v0.shape
                assert_bit_equal(v1, v0, f"connect(last, last) block {b}: voices")
                assert_bit_equal(o1, o0, f"connect(last, last) block {b}: mix")
                assert f1 == f0
        for bank in (never, again, back):
            bank.close()


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n,bs", SHAPES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_swapped_connection_swaps_the_planes(knh, name, n, bs, sample_type):
    """G: connect(r, l) equals the planes of connect(l, r) swapped."""
    case = sc.CASES[name](n)
    l, r = case.connect
    for mix_mode in MIXES:
        a = gpu_bank(knh, case, n, bs, sample_type, mix_mode, connect=(l, r))
        b = gpu_bank(knh, case, n, bs, sample_type, mix_mode, connect=(r, l))
        v = np.arange(n, dtype=np.uint32)
        peak = np.zeros(2)
        for blk in range(3):
            for bank in (a, b):
                if blk == 0:
                    for e in case.envelopes:
                        bank.param_apply_many(v, e, 3, L.VALUE_TRIGGER)
                case.events(blk, bank)
            oa, va, _ = a.process_block_voices()
            ob, vb, _ = b.process_block_voices()
            assert_bit_equal(vb, va[::-1], f"{name} block {blk}: planes swapped")
            assert_bit_equal(ob, oa[::-1], f"{name} block {blk}: channels swapped")
            peak = np.maximum(peak, np.abs(va).max(axis=(1, 2)))
        assert peak.min() > 1e-3
        a.close()
        b.close()


def _script_b(case, n, block, bank):
    v = np.arange(n, dtype=np.uint32)
    if block == 0:
        bank.param_apply_many(v, 2, 3, L.VALUE_TRIGGER)
    case.events(block, bank)


@pytest.mark.parametrize("mix_mode", MIXES)
@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n,bs", SHAPES)
def test_every_way_of_calling_gives_the_same_samples(knh, n, bs, sample_type, mix_mode):
    """J, on the bank of case B: three single calls; one process_blocks(3); process_blocks_begin / _end; each block split
    into two calls (40 + 60 frames, 24 + 40).  KNH_MIX_LEFT_FOLD processes one block per call: there the launches of
    several blocks are refused, and the single and the split calls are compared."""
    case = sc.case_b(n)
    make = lambda: gpu_bank(knh, case, n, bs, sample_type, mix_mode)
    single = make()
    want = []
    for b in range(3):
        _script_b(case, n, b, single)
        want.append(single.process_block()[0])
    want = np.stack(want)
    assert np.abs(want).max(axis=(0, 2)).min() > 1e-3
    single.close()

    def at_offsets(bank):  # the calls of blocks 1 and 2 known up front: queued for their block of the launch
        v = np.arange(n, dtype=np.uint32)
        bank.param_apply_many(v, 2, 3, L.VALUE_TRIGGER)
        bank.param_apply_many(v[::3], 0, 0, L.VALUE_FLOAT, 300.0 + v[::3], block_offset=1)
        bank.param_apply_many(v, 2, 2, L.VALUE_TRIGGER, block_offset=1)

    many = make()
    if mix_mode == L.MIX_TREE:
        at_offsets(many)
        got, _ = many.process_blocks(3)
        assert_bit_equal(got, want, "process_blocks(3)")
        piped = make()
        at_offsets(piped)
        piped.process_blocks_begin(3)
        assert_bit_equal(piped.process_blocks_end(), want, "process_blocks_begin / _end")
        piped.close()
    else:
        with pytest.raises(L.KnasterHipError) as e:
            many.process_blocks(3)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
    many.close()
    first = 40 if bs == 100 else 24
    split = make()
    for b in range(3):
        _script_b(case, n, b, split)
        out = np.zeros((2, bs), dtype=want.dtype)
        split.process_block(first, 0, out=out)
        split.process_block(bs - first, first, out=out)
        assert_bit_equal(out, want[b], f"block {b} in calls of {first} and {bs - first} frames")
    split.close()


@pytest.mark.parametrize("mix_mode", MIXES)
@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n,bs", SHAPES)
def test_restarted_voices_equal_a_fresh_bank(knh, oracle, n, bs, sample_type, mix_mode):
    """K: restart_voices([0, 5, 69]) (one voice: [0]) with new constructor arguments equals a fresh bank built with them (and
    the oracle's views of it), per voice and in the mix; the other voices go on untouched."""
    case = sc.case_b(n)
    r = np.array([0, 5, 69] if n == 70 else [0], dtype=np.uint32)
    freq_b = np.array([[333.0], [1234.5], [87.0]])[:len(r)]
    ctor_b = {s: a.copy() for s, a in case.ctor.items()}
    ctor_b[0][r] = freq_b
    running = gpu_bank(knh, case, n, bs, sample_type, mix_mode)
    twin = gpu_bank(knh, case, n, bs, sample_type, mix_mode)  # never restarted: what the other voices go on as
    v = np.arange(n, dtype=np.uint32)
    for bank in (running, twin):
        bank.param_apply_many(v, 2, 3, L.VALUE_TRIGGER)
        bank.process_block()
    running.set_voice_ctor_args(0, r, freq_b)
    running.restart_voices(r)
    running.param_apply_many(r, 2, 3, L.VALUE_TRIGGER)
    fresh = gpu_bank(knh, case, n, bs, sample_type, mix_mode, ctor=ctor_b)
    fresh.param_apply_many(v, 2, 3, L.VALUE_TRIGGER)
    views = [oracle_view(oracle, case, n, bs, sample_type, s, ctor=ctor_b) for s in case.connect]
    views[1].param_apply_many(v, 2, 3, L.VALUE_TRIGGER)
    others = np.setdiff1d(v, r)
    for b in range(2):
        mix, got, _ = running.process_block_voices()
        _, new, _ = fresh.process_block_voices()
        _, old, _ = twin.process_block_voices()
        want = np.stack([o.process_block()[1] for o in views])
        assert_bit_equal(new, want, f"block {b}: the fresh bank against the oracle views")
        assert_bit_equal(got[:, r], new[:, r], f"block {b}: restarted voices against the fresh bank")
        assert_bit_equal(got[:, others], old[:, others], f"block {b}: the other voices")
        assert_bit_equal(mix, expected_mix(got, mix_mode), f"block {b}: the mix of the running bank's planes")
        assert np.abs(got[:, r]).max(axis=(1, 2)).min() > 1e-3
    for bank in (running, twin, fresh):
        bank.close()
    for o in views:
        o.close()


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("bs", [100, 64])
@pytest.mark.parametrize("kw", [{"host_threads": 2}, {"devices": [0, 0]}], ids=["host_threads", "multi_device"])
def test_banks_of_several_ranges_equal_the_plain_bank(knh, kw, bs, sample_type):
    """L: host_threads = 2, and the multi-device form on one GPU, both bit-equal to the plain connected bank (70 voices in
    ranges of 64 and 6: the ranges' sums are the two children of the plain bank's tree root).  A bank in ranges mixes with
    KNH_MIX_TREE: with KNH_MIX_LEFT_FOLD host_threads keeps one range (compared all the same) and the multi-device form is
    refused at creation."""
    n = 70
    case = sc.case_b(n)
    for mix_mode in MIXES:
        if mix_mode == L.MIX_LEFT_FOLD and "devices" in kw:
            with pytest.raises(L.KnasterHipError):
                knh.VoiceBank(case.stages, n, sample_type, 2, mix_mode, **kw)
            continue
        plain = gpu_bank(knh, case, n, bs, sample_type, mix_mode)
        ranges = gpu_bank(knh, case, n, bs, sample_type, mix_mode, **kw)
        assert ranges.ranks() == (2 if mix_mode == L.MIX_TREE else 1) and plain.ranks() == 1
        assert (ranges.output_stage(0), ranges.output_stage(1)) == (0, 2)
        peak = np.zeros(2)
        for b in range(3):
            for bank in (plain, ranges):
                _script_b(case, n, b, bank)
            o0, v0, f0 = plain.process_block_voices()
            o1, v1, f1 = ranges.process_block_voices()
            assert v0.shape == (2, n, bs)
            assert_bit_equal(v1, v0, f"block {b}: per-voice planes")
            assert_bit_equal(o1, o0, f"block {b}: mix")
            assert f1 == f0
            peak = np.maximum(peak, np.abs(v0).max(axis=(1, 2)))
        assert peak.min() > 1e-3
        np.testing.assert_array_equal(ranges.read_done_frames(), plain.read_done_frames())
        plain.close()
        ranges.close()
