"""Banks that share a device buffer (knh_bank_process_blocks_device_add: a host with voices of several shapes has one bank
per shape, and every bank after the first adds its mix into the buffer the first one wrote) and banks that read their input
where another bank left it (knh_bank_set_input_device) -- on ONE stream of the caller's, launch behind launch, with no host
sync in between.  What can go wrong: an additive fold that ignores `accumulate` or adds twice (five folds take the argument:
fold_rows_kernel, fold_tree_kernel, fold_tree_wave_kernel, sum_shards_kernel, the Galactic bank's), a fold on a bank's own
stream that runs ahead of the bank that wrote the buffer or behind the one that reads it, a voice kernel on a bank's own
stream that reads an input the caller's stream has not written yet, a copy that overtakes the kernel still reading.

The expected value.  An additive launch does one IEEE add per sample (`*o + total`, nothing to contract), so a bank B added
to a buffer that holds X leaves X + mix_B, numpy's add in the sample type.  mix_B comes from a twin of B -- the same bank, the
same events, built under KNH_FOLD_OVERLAP=0 (one stream, fold_tree_kernel), driven one plain launch at a time with
synchronize() after each; that path is pinned to the oracle by the other suites, and test_the_shared_buffer_against_the_oracle
ties one case of this file to it directly.  Every comparison is bit for bit, the sign of a zero included.  Each case runs
once: the orderings show in the result of an unsynchronised sequence, not in repetition.

Shapes as in test_gpu_fold_overlap.py: the C3 chain at 130 voices (3 rows, a partial group) and 64 * 5 + 1 (6 rows), blocks of
64 frames (one tile) and 96 (one and a half), 2 and 3 blocks per launch, f32 and f64, envelopes that finish inside the run.
Debug word 2 is the kernel form, word 9 the launches that took the two-stream path, word 10 the folds without LDS."""
import dataclasses

import numpy as np
import pytest

import frame_bank_cases as fc
from device_buffers import Hip
from helpers import assert_bit_equal, make_gpu, make_oracle, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from test_gpu_fold_overlap import workload
from test_gpu_multi import _script

pytestmark = pytest.mark.gpu

SWITCHES = ("KNH_JIT", "KNH_PIPELINE", "KNH_PIPE_BIG", "KNH_PAIR", "KNH_WIDE", "KNH_INTERP", "KNH_FRAME_JIT", "KNH_JIT_PIPE", "KNH_JIT_WAVES",
            "KNH_FOLD_OVERLAP", "KNH_FOLD_WAVE", "KNH_HOST_THREADS", "KNH_RESIDENT", "KNH_DEV_EVENTS", "KNH_RANGE_LAUNCHES")
PLAN = (2, 3, 2, 3, 3, 2)  # blocks per launch: the row sets are reallocated in front of launch 1
PIPELINED = (L.DEBUG_FORM_PIPELINE, L.DEBUG_FORM_PIPELINE_FUSED)
TYPES = [(bs, st) for bs in (64, 96) for st in (L.F32, L.F64)]
TYPE_IDS = [f"{bs}-{'f64' if st == L.F64 else 'f32'}" for bs, st in TYPES]
BY_TYPE = pytest.mark.parametrize("st", [L.F32, L.F64], ids=["f32", "f64"])


@dataclasses.dataclass(frozen=True)
class Src:
    """One bank of a test: the voice, the shape, the switches it is created under and the kind of bank."""
    name: str              # C3, P3, IN: test_gpu_fold_overlap.workload; SCRIPT: C3 as test_gpu_multi drives it; G1; FMC: frame_bank_cases.cascade
    n: int
    bs: int
    st: int
    detuned: bool = False  # other oscillator frequencies than the bank of the same chain beside it
    channels: int = 0      # output channels, where not the workload's own
    env: tuple = ()        # ((switch, value), ..)
    mix_mode: int = L.MIX_TREE
    kw: tuple = ()         # ((argument of VoiceBank, value), ..): host_threads, devices, rank, world

    @property
    def dtype(self):
        return np.float64 if self.st == L.F64 else np.float32


def workload_of(src):
    if src.name == "SCRIPT":
        w = configs.config("C3", n_voices=src.n, block_size=src.bs, sample_type=src.st)
    elif src.name == "G1":
        w = configs.config("G1", n_voices=src.n, block_size=src.bs, sample_type=src.st)
    elif src.name == "FMC":
        w = fc.cascade(fc.TREE_DEPTH, src.n, src.bs, src.st)
    else:
        w = workload(src.name, src.n, src.bs, src.st)
    if src.detuned:
        w.ctor = dict(w.ctor)
        w.ctor[0] = np.ascontiguousarray(w.ctor[0][::-1] * 1.25)
    if src.channels:
        w.out_channels = src.channels
    return w


def note_events(w, k, nb):
    """The range events in front of launch k as (first voice, end voice, (stage, param), block of the launch): envelopes start,
    are released half a bank at a time and finish in different launches (test_gpu_fold_overlap.events)."""
    n = w.n_voices
    if not w.restart:
        return []
    if k % 3 == 0 or not w.release:  # (a voice without a release, G1's plucked sine: a new note in every launch)
        return [(0, n, w.restart, 0)]
    if k == 1:
        return [(0, n // 2, w.release[:2], 0)]
    if k == 2:
        return [(n // 2, n, w.release[:2], 0)]
    if k == 4:
        return [(0, n, w.release[:2], nb - 1)]
    return []


def drive(src, w, k, nb, g):
    """the parameter calls in front of launch k"""
    if src.name == "SCRIPT":
        _script(w, k, g)
        return
    for v0, v1, what, off in note_events(w, k, nb):
        g.param_apply_many(np.arange(v0, v1, dtype=np.uint32), what[0], what[1], L.VALUE_TRIGGER, block_offset=off)


def build(knh, monkeypatch, src, serial=False):
    w = workload_of(src)
    with monkeypatch.context() as m:  # (the switches are read when a bank is created)
        for k in SWITCHES:
            m.delenv(k, raising=False)
        for k, v in src.env:
            m.setenv(k, v)
        if serial:
            m.setenv("KNH_FOLD_OVERLAP", "0")
        g = make_gpu(knh, w, src.mix_mode, **dict(src.kw))
    return w, g


def block_bytes(w):
    return w.out_channels * w.block_size * (8 if w.sample_type == L.F64 else 4)


def freeze(a):
    a.setflags(write=False)
    return a


_TWINS = {}


def twin(knh, monkeypatch, src, plan=PLAN):
    """mix_B: the bank alone, every launch on one stream with fold_tree_kernel, plain calls, synchronize() after each.
    -> per launch (blocks, done frames, flag words 0 and 1); computed once, shared, read-only."""
    key = (src, plan)
    if key not in _TWINS:
        w, g = build(knh, monkeypatch, src, serial=True)
        hip = Hip()
        try:
            buf = hip.zeros(max(plan) * block_bytes(w))
            res = []
            for k, nb in enumerate(plan):
                drive(src, w, k, nb, g)
                g.process_blocks_device(nb, buf)
                g.synchronize()
                words = g.debug_words()
                assert int(words[9]) == 0, "the twin took the two-stream path"
                res.append((freeze(hip.to_host(buf, (nb, w.out_channels, w.block_size), src.dtype)), freeze(g.read_done_frames().copy()),
                            (int(words[0]), int(words[1]))))
        finally:
            g.close()
            hip.close()
        assert max(float(np.abs(r[0]).max()) for r in res) > 1e-4, "silent"
        _TWINS[key] = res
    return _TWINS[key]


class Rig:
    """The caller: a device, buffers and one non-blocking stream of its own, and the banks it drives."""

    def __init__(self, knh, monkeypatch):
        self.knh, self.monkeypatch = knh, monkeypatch
        self.hip = Hip()
        self.banks = []
        self.s = self.hip.stream()

    def bank(self, src):
        w, g = build(self.knh, self.monkeypatch, src)
        self.banks.append(g)
        return w, g

    def twin(self, src, plan=PLAN):
        return twin(self.knh, self.monkeypatch, src, plan)

    def synchronize(self):
        for g in self.banks:
            g.synchronize()

    def close(self):
        for g in self.banks:
            try:
                g.synchronize()
            finally:
                g.close()
        self.hip.close()


@pytest.fixture
def rig(knh, monkeypatch):
    r = Rig(knh, monkeypatch)
    yield r
    r.close()


def play(rig, srcs, plan=PLAN, n_bufs=1, prefill=None):
    """Launch k of every bank of `srcs` in turn on the caller's stream, all into the same buffer, a snapshot of the buffer
    (hipMemcpyAsync on that stream) behind the last bank's call; no host sync until every launch is enqueued.  The first
    bank writes and the others add; with `prefill` (one array per launch, each in a buffer of its own) every bank adds.
    -> (the snapshots, [(workload, bank)])"""
    banks = [rig.bank(src) for src in srcs]
    w0 = banks[0][0]
    bb = block_bytes(w0)
    assert all(block_bytes(w) == bb for w, _ in banks)
    hip, s = rig.hip, rig.s
    bufs = [hip.upload(x) for x in prefill] if prefill is not None else [hip.zeros(max(plan) * bb) for _ in range(n_bufs)]
    snaps = [hip.zeros(nb * bb) for nb in plan]
    for k, nb in enumerate(plan):
        buf = bufs[k % len(bufs)]
        for i, (src, (w, g)) in enumerate(zip(srcs, banks)):
            drive(src, w, k, nb, g)
            g.process_blocks_device(nb, buf, s, add=prefill is not None or i > 0)
        hip.copy_on(s, snaps[k], buf, nb * bb)
    rig.synchronize()
    outs = [hip.to_host(snaps[k], (nb, w0.out_channels, w0.block_size), srcs[0].dtype) for k, nb in enumerate(plan)]
    return outs, banks


def summed(twins, k):
    """X + mix_B (+ mix_C): numpy's add in the sample type, in the order of the launches"""
    total = twins[0][k][0]
    for t in twins[1:]:
        total = total + t[k][0]
    return total


def words_of(g):
    w = g.debug_words()
    return int(w[2]), int(w[9]), int(w[10]), (int(w[0]), int(w[1]))


# ---- a. two pipelined banks, one stream, no host sync ------------------------------------------------------------------------
@pytest.mark.parametrize("n_bufs", [1, 3], ids=["one_buffer", "three_buffers"])
@pytest.mark.parametrize("bs,st", TYPES, ids=TYPE_IDS)
def test_a_second_bank_adds_into_the_first_one_s_buffer(rig, bs, st, n_bufs):
    """A (130 voices) writes, B (321 voices, other frequencies) adds, six launches each in turn.  B's fold, on B's fold
    stream, follows A's, on A's; A's next fold follows the snapshot that reads what B added (one buffer reused)."""
    a, b = Src("C3", 130, bs, st), Src("C3", 64 * 5 + 1, bs, st, detuned=True)
    ta, tb = rig.twin(a), rig.twin(b)
    outs, banks = play(rig, [a, b], n_bufs=n_bufs)
    for k in range(len(PLAN)):
        assert not np.array_equal(ta[k][0], tb[k][0])
        assert_bit_equal(outs[k], summed([ta, tb], k), f"launch {k}: A + B", strict_zero=True)
    assert max(float(np.abs(o).max()) for o in outs) > 1e-4
    for (w, g), t, name in zip(banks, (ta, tb), "AB"):
        form, overlapped, wave_folds, flags = words_of(g)
        assert form == L.DEBUG_FORM_PIPELINE and overlapped == wave_folds == len(PLAN), (name, form, overlapped, wave_folds)
        assert np.array_equal(g.read_done_frames(), t[-1][1]), f"{name}: done frames"
        assert flags == t[-1][2], f"{name}: flag words"
    assert len({t[2] for t in tb}) >= 2 and any(t[2][0] for t in tb), "the flag words never change: the envelopes do not finish"


# ---- b. three banks, one of them with two planes ---------------------------------------------------------------------------------
@BY_TYPE
def test_three_banks_the_third_a_pan2_chain(rig, st):
    """A writes, B and C add.  C's rows are two planes, its fold sees twice as many blocks of one channel each
    (fold_channels == 1), while A and B write one mono signal into both channels."""
    a, b, c = Src("C3", 130, 96, st), Src("C3", 64 * 5 + 1, 96, st, detuned=True), Src("P3", 130, 96, st)
    twins = [rig.twin(x) for x in (a, b, c)]
    outs, banks = play(rig, [a, b, c])
    for k in range(len(PLAN)):
        assert np.array_equal(twins[0][k][0][:, 0], twins[0][k][0][:, 1]) and np.array_equal(twins[1][k][0][:, 0], twins[1][k][0][:, 1])
        assert not np.array_equal(twins[2][k][0][:, 0], twins[2][k][0][:, 1]), "C: left equals right"
        assert_bit_equal(outs[k], summed(twins, k), f"launch {k}: A + B + C", strict_zero=True)
        assert not np.array_equal(outs[k][:, 0], outs[k][:, 1]), "left equals right"
    assert max(float(np.abs(o).max()) for o in outs) > 1e-4
    for _, g in banks:
        form, overlapped, _, _ = words_of(g)
        assert form == L.DEBUG_FORM_PIPELINE and overlapped == len(PLAN), (form, overlapped)


# ---- c. every fold that takes `accumulate` ------------------------------------------------------------------------------------------
def _c3(**kw):
    return Src("C3", 130, 96, kw.pop("st", L.F32), **kw)


SHORT = (2, 3, 2)
FRAMES = (L.DEBUG_FORM_FRAME_JIT, L.DEBUG_FORM_FRAME_INTERP)
# id: (the adding bank, blocks per launch, the forms debug word 2 may name (None: any), launches on the two-stream path, ranks())
ADDERS = {
    "default": (_c3(), SHORT, (L.DEBUG_FORM_PIPELINE,), 3, 1),                                  # fold_tree_wave_kernel, beside the next launch
    "default_f64": (_c3(st=L.F64), SHORT, (L.DEBUG_FORM_PIPELINE,), 3, 1),
    "one_stream": (_c3(env=(("KNH_FOLD_OVERLAP", "0"),)), SHORT, (L.DEBUG_FORM_PIPELINE,), 0, 1),  # fold_tree_kernel
    "one_wavefront": (_c3(env=(("KNH_PIPELINE", "0"),)), SHORT, (L.DEBUG_FORM_WHOLE_CHAIN,), 0, 1),
    "four_per_workgroup": (_c3(env=(("KNH_WIDE", "4"),)), SHORT, (L.DEBUG_FORM_MANY_WAVE,), 0, 1),
    "fused_pipeline": (_c3(env=(("KNH_JIT", "1"),)), SHORT, (L.DEBUG_FORM_PIPELINE_FUSED,), 3, 1),  # events recorded around the kernel
    "fused_one_wavefront": (_c3(env=(("KNH_JIT", "1"), ("KNH_JIT_PIPE", "0"))), SHORT, (L.DEBUG_FORM_WHOLE_CHAIN_FUSED,), 0, 1),
    "pair": (_c3(env=(("KNH_PAIR", "1"),)), SHORT, (L.DEBUG_FORM_PIPELINE,), 3, 1),
    # a lane per frame: the rows are the voices', 300 of them in two passes of fold_tree_kernel, 80 frames: a partial wavefront
    "lane_per_frame": (Src("FMC", 300, 80, L.F32), SHORT, FRAMES, 0, 1),
    "left_fold": (_c3(mix_mode=L.MIX_LEFT_FOLD), (1, 1, 1), None, 0, 1),                         # fold_rows_kernel
    "galactic": (Src("G1", 4, 64, L.F32), SHORT, None, 0, 1),
    # voice ranges are whole 64-voice groups, as many per range as it takes: 200 voices are 4 groups, 2 per range for three
    # threads or devices -- two ranges, 128 and 72 voices; 321 voices are 6 groups -- three ranges, 128, 128 and 65
    "host_sharded": (Src("C3", 200, 96, L.F32, kw=(("host_threads", 3),)), SHORT, (L.DEBUG_FORM_PIPELINE,), 3, 2),  # sum_shards_kernel
    "host_sharded_three_ranges": (Src("C3", 64 * 5 + 1, 96, L.F64, kw=(("host_threads", 3),)), SHORT, (L.DEBUG_FORM_PIPELINE,), 3, 3),
    "multi_device": (Src("C3", 200, 96, L.F32, kw=(("devices", (0, 0, 0)),)), SHORT, (L.DEBUG_FORM_PIPELINE,), 3, 2),
}


@pytest.mark.parametrize("adder", list(ADDERS))
def test_every_fold_adds_once(rig, adder):
    """Each launch adds into a buffer that holds a pseudo-random X, nowhere zero, left unlike right: a fold that ignores
    `accumulate` leaves mix_B, one that adds twice X + 2 mix_B (or 2 X + mix_B)."""
    src, plan, forms, overlapped, ranks = ADDERS[adder]
    t = rig.twin(src, plan)
    ch = t[0][0].shape[1]
    rng = np.random.default_rng(7)
    xs = [(rng.uniform(0.25, 1.0, (nb, ch, src.bs)) * rng.choice([-1.0, 1.0], (nb, ch, src.bs))).astype(src.dtype) for nb in plan]
    outs, banks = play(rig, [src], plan, prefill=xs)
    g = banks[0][1]
    for k in range(len(plan)):
        mix = t[k][0]
        assert float(np.abs(mix).max()) > 1e-4 and not np.array_equal(xs[k] + mix, xs[k]), f"launch {k}: nothing to hear"
        assert_bit_equal(outs[k], xs[k] + mix, f"{adder}, launch {k}: X + mix", strict_zero=True)
    form, took, _, _ = words_of(g)
    assert (forms is None or form in forms) and took == overlapped and g.ranks() == ranks, (form, took, g.ranks())
    if src.mix_mode == L.MIX_LEFT_FOLD:  # (what tells a left-fold bank from the outside: it takes one block per call)
        with pytest.raises(L.KnasterHipError):
            g.process_blocks_device(2, rig.hip.zeros(2 * block_bytes(banks[0][0])), rig.s, add=True)
    if src.name == "G1":
        assert g.stages[-1].kind == L.STAGE_GALACTIC and g.outputs() == 2
        assert not np.array_equal(t[0][0][:, 0], t[0][0][:, 1]), "the reverb's left equals its right"


# ---- d. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["rank_bank", "null_output"])
def test_a_refused_additive_launch_leaves_the_bank_as_it_was(rig, what):
    """A rank's share of a sharded bank cannot add into a mix the other ranks do not see, and no bank can add into a buffer of
    its own.  The refused call takes nothing with it: the events queued in front of it belong to the next launch."""
    src = Src("C3", 130, 96, L.F32, kw=(("rank", 0), ("world", 1)) if what == "rank_bank" else ())
    (w, g), (_, fresh) = rig.bank(src), rig.bank(src)
    buf = rig.hip.upload(np.full((3, w.out_channels, w.block_size), 0.5, dtype=src.dtype))
    outs = []
    for bank, refuse in ((g, True), (fresh, False)):
        res = []
        for k, nb in enumerate(SHORT):
            drive(src, w, k, nb, bank)
            if refuse and k in (0, 2):
                with pytest.raises(L.KnasterHipError) as e:
                    bank.process_blocks_device(nb, buf if what == "rank_bank" else 0, rig.s, add=True)
                assert e.value.status == L.ERR_INVALID_ARGUMENT, e.value
            bank.process_blocks_device(nb, buf, rig.s)
            bank.synchronize()
            res.append(rig.hip.to_host(buf, (nb, w.out_channels, w.block_size), src.dtype))
        outs.append(res)
    for k in range(len(SHORT)):
        assert_bit_equal(outs[0][k], outs[1][k], f"{what}: launch {k} behind a refusal", strict_zero=True)
    assert max(float(np.abs(o).max()) for o in outs[1]) > 1e-4
    assert np.array_equal(g.read_done_frames(), fresh.read_done_frames())


# ---- e. voice ranges with device output -------------------------------------------------------------------------------------------------
KINDS = {"multi_device": (("devices", (0, 0, 0)),), "host_sharded": (("host_threads", 3),), "rank": (("rank", 0), ("world", 1))}


@pytest.mark.parametrize("kind", list(KINDS))
def test_voice_ranges_with_device_output(rig, kind):
    """The banks made of voice ranges hand the caller's `sync == false` on to the ranges' own banks, whose launches then take
    the two-stream path, each range on a stream of its own: three launches back to back against the same kind of bank
    rendering to host memory, where every launch is waited for."""
    src = Src("SCRIPT", 200, 64, L.F32, kw=KINDS[kind])  # (200 voices: two ranges of 128 and 72, see ADDERS)
    plan = (3, 3, 3)
    w, ref = rig.bank(src)
    want = []
    for k, nb in enumerate(plan):
        drive(src, w, k, nb, ref)
        want.append(ref.process_blocks(nb)[0])
    assert int(ref.debug_words()[9]) == 0
    outs, banks = play(rig, [src], plan)
    g = banks[0][1]
    for k in range(len(plan)):
        assert_bit_equal(outs[k], want[k], f"{kind}: launch {k}", strict_zero=True)
        assert k == 0 or not np.array_equal(want[k], want[k - 1])
    assert float(np.abs(want[0]).max()) > 1e-4
    form, overlapped, _, _ = words_of(g)
    assert form == L.DEBUG_FORM_PIPELINE and overlapped == len(plan) and g.ranks() == (1 if kind == "rank" else 2), (form, overlapped, g.ranks())
    assert np.array_equal(g.read_done_frames(), ref.read_done_frames())


# ---- f. the input read where it lies -------------------------------------------------------------------------------------------------------
def closed_form(w, blocks):
    """pairwise_sum(const[v] * input): [n_blocks, 1, block_size] from this launch's input blocks [n_blocks, 1, block_size]"""
    c = w.ctor[1][:, 0].astype(blocks.dtype).reshape(-1, 1)
    return np.stack([pairwise_sum(c * b[0].reshape(1, -1)).reshape(1, -1) for b in blocks])


INPUT_FORMS = {"default": ((), PIPELINED, len(PLAN)), "one_wavefront": ((("KNH_PIPELINE", "0"),), (L.DEBUG_FORM_WHOLE_CHAIN, L.DEBUG_FORM_WHOLE_CHAIN_FUSED), 0)}


@pytest.mark.parametrize("form", list(INPUT_FORMS))
@BY_TYPE
def test_the_input_read_where_it_lies(rig, st, form):
    """Input * const per voice, fed two ways: blocks uploaded by set_input, and the same blocks copied into ONE device buffer
    by a hipMemcpyAsync on the caller's stream right in front of each process call, then set_input_device.  The voice kernel of
    launch k + 1 (on the bank's own stream in the default form) must not start before that copy, and the copy must not
    overtake launch k's reads."""
    env, forms, overlapped = INPUT_FORMS[form]
    src = Src("IN", 130, 96, st, env=env)
    (w, by_host), (_, by_device) = rig.bank(src), rig.bank(src)
    hip, s, bb = rig.hip, rig.s, block_bytes(w)
    inputs = [np.random.default_rng(100 + k).uniform(-1.0, 1.0, (nb, 1, w.block_size)).astype(src.dtype) for k, nb in enumerate(PLAN)]
    staged = [hip.upload(x) for x in inputs]
    d_in = hip.zeros(max(PLAN) * bb)
    d_out = [hip.zeros(max(PLAN) * bb) for _ in range(2)]
    snaps = [[hip.zeros(nb * bb) for nb in PLAN] for _ in range(2)]
    for k, nb in enumerate(PLAN):
        by_host.set_input(inputs[k])
        by_host.process_blocks_device(nb, d_out[0], s)
        hip.copy_on(s, snaps[0][k], d_out[0], nb * bb)
        hip.copy_on(s, d_in, staged[k], nb * bb)
        by_device.set_input_device(d_in, nb)
        by_device.process_blocks_device(nb, d_out[1], s)
        hip.copy_on(s, snaps[1][k], d_out[1], nb * bb)
    rig.synchronize()
    for k, nb in enumerate(PLAN):
        got_host, got_device = (hip.to_host(snaps[i][k], (nb, 1, w.block_size), src.dtype) for i in range(2))
        want = closed_form(w, inputs[k])
        assert float(np.abs(want).max()) > 1e-4
        assert_bit_equal(got_device, got_host, f"launch {k}: set_input_device against set_input", strict_zero=True)
        assert_bit_equal(got_device, want, f"launch {k}: against pairwise_sum(const * input)", strict_zero=True)
    for g in (by_host, by_device):
        took, n_overlapped, _, _ = words_of(g)
        assert took in forms and n_overlapped == overlapped, (took, n_overlapped)


# ---- g. banks in series and in parallel on the device ------------------------------------------------------------------------------------
@BY_TYPE
def test_banks_in_series_and_in_parallel(rig, st):
    """A renders into U; C renders into V; B reads U where it lies, multiplies it per voice and ADDS its mix into V.  Four
    rounds on one stream: B's voice kernel waits for A's fold, A's next fold for B's reads, B's fold for C's."""
    plan = (2, 3, 2, 3)
    a, b, c = Src("C3", 130, 96, st, channels=1), Src("IN", 130, 96, st), Src("C3", 64 * 5 + 1, 96, st, detuned=True, channels=1)
    ta, tc = rig.twin(a, plan), rig.twin(c, plan)
    (wa, ga), (wb, gb), (wc, gc) = rig.bank(a), rig.bank(b), rig.bank(c)
    hip, s, bb = rig.hip, rig.s, block_bytes(wa)
    assert bb == block_bytes(wb) == block_bytes(wc) and wb.in_channels == 1
    u, v = hip.zeros(max(plan) * bb), hip.zeros(max(plan) * bb)
    snaps = [hip.zeros(nb * bb) for nb in plan]
    for k, nb in enumerate(plan):
        drive(a, wa, k, nb, ga)
        ga.process_blocks_device(nb, u, s)
        drive(c, wc, k, nb, gc)
        gc.process_blocks_device(nb, v, s)
        gb.set_input_device(u, nb)
        gb.process_blocks_device(nb, v, s, add=True)
        hip.copy_on(s, snaps[k], v, nb * bb)
    rig.synchronize()
    for k, nb in enumerate(plan):
        series = closed_form(wb, ta[k][0])
        assert k > 0 or (float(np.abs(series).max()) > 1e-4 and float(np.abs(tc[k][0]).max()) > 1e-4), "silent"
        assert_bit_equal(hip.to_host(snaps[k], (nb, 1, wa.block_size), a.dtype), tc[k][0] + series, f"round {k}: C + B(A)", strict_zero=True)
    for g, forms in ((ga, (L.DEBUG_FORM_PIPELINE,)), (gb, PIPELINED), (gc, (L.DEBUG_FORM_PIPELINE,))):
        form, overlapped, _, _ = words_of(g)
        assert form in forms and overlapped == len(plan), (form, overlapped)


# ---- h. one direct tie to the oracle ---------------------------------------------------------------------------------------------------------
def test_the_shared_buffer_against_the_oracle(rig, oracle):
    """Case (a) at 130 + 321 voices, f32, blocks of 64, two launches: pairwise_sum(the oracle's voices of A) +
    pairwise_sum(those of B), the oracle driven block by block with each block's events in front of it.  C3's voices are
    bit-exact against the oracle (test_gpu_properties.py) and the tree mix is defined as that sum."""
    plan = (2, 3)
    a, b = Src("C3", 130, 64, L.F32), Src("C3", 64 * 5 + 1, 64, L.F32, detuned=True)
    outs, banks = play(rig, [a, b], plan)
    mixes = []
    for src in (a, b):
        w = workload_of(src)
        o = make_oracle(oracle, w, want_mix=False)
        per_launch = []
        for k, nb in enumerate(plan):
            ev = note_events(w, k, nb)
            blocks = []
            for blk in range(nb):
                for v0, v1, what, off in ev:
                    if off == blk:
                        o.param_apply_many(np.arange(v0, v1, dtype=np.uint32), what[0], what[1], L.VALUE_TRIGGER)
                blocks.append(pairwise_sum(o.process_block()[1]))
            per_launch.append(np.stack(blocks))
        o.close()
        mixes.append(per_launch)
    for k, nb in enumerate(plan):
        want = mixes[0][k] + mixes[1][k]  # [nb, bs]: the one mono signal of both channels
        assert want.dtype == np.float32 and float(np.abs(want).max()) > 1e-4
        assert_bit_equal(outs[k], np.stack([want, want], axis=1), f"launch {k}: against the oracle's voices", strict_zero=True)
    for _, g in banks:
        assert words_of(g)[:2] == (L.DEBUG_FORM_PIPELINE, len(plan))
