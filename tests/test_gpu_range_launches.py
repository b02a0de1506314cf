"""Range events in ordinary launches (voice_bank.hpp upload_events, voice_pipe.hpp voice_pipe_kernel): a launch of a
pipelined kernel whose events are nothing but a few changes for runs of neighbouring voices, all due inside the launch,
takes them as range events in its kernel arguments instead of per-voice lists in pinned host memory.  What can go wrong:
which voices a record covers (group boundaries, the ragged last group, the dead group of the pair form), the order of
records on one frame, the decision to fall back (per-voice events in the same launch, a range beyond the launch, more
ranges than the kernel arguments hold), and the staging itself.

Common shape: the C3 chain, 130 voices (two full groups and a ragged one of two voices), blocks of 64 and of 96 frames (a
partial last tile), two launches of four blocks, f32 and f64, every pipeline form.  Each case is held bit for bit to the
same bank with KNH_RANGE_LAUNCHES=0 (per-voice lists), to the single-wavefront kernel (KNH_PIPELINE=0, which always takes
lists) and -- block by block, per voice -- to the CPU oracle; knh_bank_event_stats says which path ran.  Beside the C3
chain: a Pan2 and a delay line behind it, and a chain whose pipeline is fused at run time.

(A run of fewer than 16 voices never becomes a range event on the host -- knh_bank_param_apply_range's own threshold -- so
the case of a single voice of the ragged group, [129, 130), reaches the kernel as a per-voice list; the ragged group is
reached by range records through [100, 130) and the bank-wide ranges.)"""
import numpy as np
import pytest

from helpers import assert_bit_equal, make_gpu, make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs

pytestmark = pytest.mark.gpu

N, BLOCKS, LAUNCHES = 130, 4, 2
CAP = 16  # knh_dev::LAUNCH_RANGES_MAX (voice_chain.hpp)
SINGLE = {"KNH_PIPELINE": "0"}
LISTS = {"KNH_RANGE_LAUNCHES": "0"}
FORMS = {"mixer": {"KNH_PIPELINE": "1", "KNH_PIPE_BIG": "0"}, "fold": {"KNH_PIPELINE": "1", "KNH_PIPE_BIG": "1"},
         "inplace": {"KNH_PIPELINE": "1", "KNH_PIPE_BIG": "2"}, "pair": {"KNH_PIPELINE": "1", "KNH_PAIR": "1"}}
SHAPES = [(L.F32, 64), (L.F32, 96), (L.F64, 64), (L.F64, 96)]
RESTART, RELEASE = (3, 3), (3, 2)  # C3's envelope: t_restart, t_release

shapes = pytest.mark.parametrize("sample_type,bs", SHAPES)
forms = pytest.mark.parametrize("form", list(FORMS))


def _bank(knh, monkeypatch, w, env, mix=L.MIX_TREE, **kw):
    with monkeypatch.context() as m:  # (the switches are read when a bank is created and initialised)
        for k, v in env.items():
            m.setenv(k, v)
        return make_gpu(knh, w, mix, **kw)


def trig(v0, v1, what):
    return (np.arange(v0, v1, dtype=np.uint32), what[0], what[1], L.VALUE_TRIGGER, None)


def cutoff(voices, hz):
    v = np.asarray(voices, dtype=np.uint32)
    return (v, 2, 0, L.VALUE_FLOAT, np.full(len(v), float(hz)))


# A script: [(launch the call is made in front of, block_offset, call)], in the order the calls are made.
def _due(entry):
    return entry[0] * BLOCKS + entry[1]


def _send(bank, call, offset=0):
    v, s, p, kind, f = call
    if offset:
        bank.param_apply_many(v, s, p, kind, f, block_offset=offset)
    else:
        bank.param_apply_many(v, s, p, kind, f)


_ORACLE = {}  # (script name, sample type, block size) -> per block (voices, done frames), rendered once


def _oracle_blocks(oracle, w, name, script):
    key = (name, w.sample_type, w.block_size)
    if key not in _ORACLE:
        o = make_oracle(oracle, w)
        res = []
        for blk in range(BLOCKS * LAUNCHES):
            for e in script:
                if _due(e) == blk:
                    _send(o, e[2])
            _, ov, _, od = o.process_block()
            res.append((ov.copy(), od.copy()))
        o.close()
        for ov, od in res:
            ov.setflags(write=False)
            od.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


def _launches(knh, monkeypatch, w, env, script):
    """two launches of four blocks, the calls made in front of their launch -> (mix [8, ch, B], flags, done frames, stats per launch)"""
    g = _bank(knh, monkeypatch, w, env)
    outs, flags, dones, stats = [], [], [], []
    for launch in range(LAUNCHES):
        for e in script:
            if e[0] == launch:
                _send(g, e[2], e[1])
        out, fl = g.process_blocks(BLOCKS)
        outs.append(out)
        flags.append(fl)
        dones.append(g.read_done_frames())
        stats.append(g.event_stats())
    form = int(g.debug_words()[2])
    if env.get("KNH_PIPELINE") == "0":
        assert form in (L.DEBUG_FORM_WHOLE_CHAIN, L.DEBUG_FORM_WHOLE_CHAIN_FUSED), form
    else:
        assert form in (L.DEBUG_FORM_PIPELINE, L.DEBUG_FORM_PIPELINE_FUSED), form
    g.close()
    return np.concatenate(outs), flags, dones, stats


_SINGLE = {}  # the single-wavefront kernel's launches do not depend on the pipeline form


def _check(knh, oracle, monkeypatch, name, script, sample_type, bs, form, want_stats, w=None):
    """want_stats: per launch, 'range' or 'list' -- the path the launch must have taken with range launches on"""
    if w is None:
        w = configs.config("C3", n_voices=N, block_size=bs, sample_type=sample_type)
    env = FORMS[form]
    got = _launches(knh, monkeypatch, w, env, script)
    lists = _launches(knh, monkeypatch, w, {**env, **LISTS}, script)
    key = (name, sample_type, bs)
    if key not in _SINGLE:
        _SINGLE[key] = _launches(knh, monkeypatch, w, SINGLE, script)
    single = _SINGLE[key]
    assert np.abs(got[0]).max() > 1e-6
    for other, what in ((lists, "KNH_RANGE_LAUNCHES=0"), (single, "the single-wavefront kernel")):
        assert_bit_equal(got[0], other[0], f"{name} {form}: mix against {what}")
        assert got[1] == other[1], (name, form, what, got[1], other[1])
        for launch in range(LAUNCHES):
            np.testing.assert_array_equal(got[2][launch], other[2][launch], err_msg=f"{name} {form}: done frames of launch {launch} against {what}")
    # which path ran: the counters after each launch
    n_range = n_list = 0
    for launch, kind in enumerate(want_stats):
        n_range += kind == "range"
        n_list += kind == "list"
        r, l, b = got[3][launch]
        assert (r, l) == (n_range, n_list), (name, form, launch, got[3])
        assert (b > 0) == (n_list > 0), (name, form, launch, got[3])
    assert [s[0] for s in lists[3]] == [0] * LAUNCHES and [s[0] for s in single[3]] == [0] * LAUNCHES  # the references took lists
    assert lists[3][-1][1] == len([k for k in want_stats if k]) and lists[3][-1][2] > 0
    # ... and the oracle, block by block and voice by voice (one-block launches: the calls in front of their block)
    want = _oracle_blocks(oracle, w, name, script)
    g = _bank(knh, monkeypatch, w, env)
    for blk in range(BLOCKS * LAUNCHES):
        for e in script:
            if _due(e) == blk:
                _send(g, e[2])
        out, voices, _ = g.process_block_voices()
        assert_bit_equal(voices, want[blk][0], f"{name} {form}: block {blk} per-voice against the oracle")
        assert_bit_equal(out, got[0][blk], f"{name} {form}: block {blk} mix, a launch per block against four blocks per launch")
        np.testing.assert_array_equal(g.read_done_frames(), want[blk][1])
    g.close()


@forms
@shapes
def test_bank_wide_and_partial_ranges(knh, oracle, monkeypatch, sample_type, bs, form):
    """The bench's note cycle (restart on every voice at block 0, release at block 2), then ranges that cross a group
    boundary, cover exactly one group, end in the ragged group, and the whole bank again."""
    script = [(0, 0, trig(0, N, RESTART)), (0, 2, trig(0, N, RELEASE)),
              (1, 0, trig(3, 67, RESTART)), (1, 1, trig(64, 128, RELEASE)), (1, 2, trig(100, 130, RESTART)), (1, 3, trig(0, N, RELEASE))]
    _check(knh, oracle, monkeypatch, "ranges", script, sample_type, bs, form, ["range", "range"])


@forms
@shapes
def test_one_voice_of_the_ragged_group(knh, oracle, monkeypatch, sample_type, bs, form):
    """[129, 130): a run of one voice is a per-voice event on the host, so the launch that carries it takes lists."""
    script = [(0, 0, trig(0, N, RESTART)), (1, 1, trig(129, 130, RELEASE))]
    _check(knh, oracle, monkeypatch, "one_voice", script, sample_type, bs, form, ["range", "list"])


@forms
@shapes
def test_two_ranges_on_one_frame_keep_their_order(knh, oracle, monkeypatch, sample_type, bs, form):
    """Restart then release, and release then restart, of the same voices on the same frame; and a call for an earlier
    block made after one for a later block (the records are walked in frame order)."""
    script = [(0, 0, trig(0, N, RESTART)), (0, 0, trig(0, N, RELEASE)), (0, 3, trig(3, 67, RESTART)), (0, 2, trig(0, N, RESTART)),
              (1, 1, trig(0, N, RELEASE)), (1, 1, trig(0, N, RESTART)), (1, 1, trig(64, 128, RELEASE))]
    _check(knh, oracle, monkeypatch, "order", script, sample_type, bs, form, ["range", "range"])


@forms
@shapes
def test_a_per_voice_event_in_the_launch_falls_back(knh, oracle, monkeypatch, sample_type, bs, form):
    """A range together with a new cutoff on one voice: the launch takes per-voice lists, and says so."""
    script = [(0, 0, trig(0, N, RESTART)), (0, 1, cutoff([70], 1234.5)), (1, 0, trig(0, N, RELEASE)), (1, 2, trig(0, N, RESTART))]
    _check(knh, oracle, monkeypatch, "mixed", script, sample_type, bs, form, ["list", "range"])


@forms
@shapes
def test_a_range_beyond_the_launch(knh, oracle, monkeypatch, sample_type, bs, form):
    """A release addressed to block 5 of a four-block launch: it is applied in block 1 of the next launch."""
    script = [(0, 0, trig(0, N, RESTART)), (0, BLOCKS + 1, trig(0, N, RELEASE))]
    _check(knh, oracle, monkeypatch, "beyond", script, sample_type, bs, form, ["list", "list"])


@forms
@shapes
def test_one_range_more_than_the_cap(knh, oracle, monkeypatch, sample_type, bs, form):
    """As many ranges as the kernel arguments hold (16) go as ranges; one more and the launch takes lists."""
    def many(launch, n):
        return [(launch, k % BLOCKS, trig(k, N - k, RESTART if k % 2 == 0 else RELEASE)) for k in range(n)]
    script = many(0, CAP) + many(1, CAP + 1)
    _check(knh, oracle, monkeypatch, "cap", script, sample_type, bs, form, ["range", "list"])


@pytest.mark.parametrize("form", ["mixer", "inplace"])
@pytest.mark.parametrize("name,bs", [("P3", 64), ("P3", 96), ("D3", 96)])
def test_other_kinds_of_stage_group(knh, oracle, monkeypatch, name, bs, form):
    """A Pan2 behind the envelope (P3: two planes of rows) and a delay line in the envelope's group (D3: its per-voice delay
    times are per-voice events, so the first launch takes lists and the second ranges).  (The Fan forms exist for chains
    without an envelope only: no range event can reach them.)"""
    w = configs.config(name, n_voices=N, block_size=bs)
    v = np.arange(N, dtype=np.uint32)
    restart, release = w.restart, w.release[:2]
    script = [(0, 0, trig(0, N, restart)), (0, 2, trig(3, 67, release)), (1, 0, trig(64, 128, release)), (1, 1, trig(0, N, restart)), (1, 3, trig(100, N, release))]
    first = "range"
    if w.delay_times is not None:  # 24 .. 190 samples, different per voice: the delayed signal arrives within these blocks
        script.insert(0, (0, 0, (v, 3, 0, L.VALUE_FLOAT, 0.0005 + 0.0005 * (v % 8))))
        first = "list"
    _check(knh, oracle, monkeypatch, name, script, w.sample_type, bs, form, [first, "range"], w=w)


def test_a_pipeline_fused_at_run_time(knh, oracle, monkeypatch):
    """A chain without a pre-built kernel (noise -> gain -> filter -> envelope): hiprtc builds voice_pipe_kernel from the same
    headers, and its launches take range events too."""
    from knaster_amd.bank import Stage

    bs = 96
    p = configs.voice_parameters(N)
    w = configs.Workload("noise", [Stage(L.STAGE_WHITE_NOISE), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)], N, bs, L.F32, 2)
    w.ctor = {0: np.arange(N, dtype=np.float64).reshape(N, 1), 1: np.full((N, 1), 1.0 / N),
              2: np.stack([np.zeros(N), p["cutoff"], p["q"], np.zeros(N)], axis=1), 3: np.stack([p["attack"], p["release"]], axis=1)}
    script = [(0, 0, trig(0, N, RESTART)), (0, 2, trig(3, 67, RELEASE)), (1, 1, trig(100, N, RELEASE)), (1, 1, trig(0, N, RESTART))]
    FORMS["fused"] = {"KNH_PIPELINE": "1"}
    try:
        _check(knh, oracle, monkeypatch, "noise", script, L.F32, bs, "fused", ["range", "range"], w=w)
    finally:
        del FORMS["fused"]


@pytest.mark.parametrize("on", [True, False])
def test_the_bench_s_calls_on_a_rank_bank(knh, monkeypatch, on):
    """bench.py's own calls, small: a rank bank (world 1) of 256 voices, prepared batches for all voices at offsets 0 and
    n / 2, knh_bank_process_blocks_device.  Range launches only, no byte of per-voice lists; same blocks as with lists."""
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    w = configs.config("C3", n_voices=256, block_size=128)
    n_blocks = 4

    def run(env):
        g = _bank(knh, monkeypatch, w, env, rank=0, world=1)
        mine = np.arange(w.n_voices, dtype=np.uint32)
        restart = g.prepare_many(mine, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
        release = g.prepare_many(mine, w.release[0], w.release[1], L.VALUE_TRIGGER)
        out = np.zeros((LAUNCHES, n_blocks, w.out_channels, w.block_size), dtype=np.float32)
        rings = [C.c_void_p() for _ in range(LAUNCHES)]  # a launch's blocks in device memory, as the bench's rings
        for ring in rings:
            assert hip.hipMalloc(C.byref(ring), out[0].nbytes) == 0
        for ring in rings:
            g.param_apply_prepared(restart, 0)
            g.param_apply_prepared(release, n_blocks // 2)
            g.process_blocks_device(n_blocks, ring.value)
        g.synchronize()
        stats = g.event_stats()
        for k, ring in enumerate(rings):
            assert hip.hipMemcpy(out[k].ctypes.data, ring, out[k].nbytes, 2) == 0  # device to host
            hip.hipFree(ring)
        g.close()
        return out, stats
    out, stats = run({} if on else LISTS)
    ref, _ = run(SINGLE)
    assert np.abs(out).max() > 1e-6
    assert_bit_equal(out, ref, "against the single-wavefront kernel")
    if on:
        assert stats == (LAUNCHES, 0, 0), stats
    else:
        assert stats[0] == 0 and stats[1] == LAUNCHES and stats[2] == LAUNCHES * (2 * w.n_voices * 16 + (w.n_voices + 1) * 4), stats


def test_resident_calls_keep_their_path(knh, monkeypatch):
    """One-block calls served by a resident kernel are no ordinary launches: their range events ride with the command."""
    monkeypatch.setenv("KNH_RESIDENT", "1")
    w = configs.config("C3", n_voices=N, block_size=128)
    g = _bank(knh, monkeypatch, w, FORMS["inplace"])
    v = np.arange(N, dtype=np.uint32)
    for b in range(4):
        if b == 0:
            g.param_apply_many(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER)
        if b == 2:
            g.param_apply_range(10, 100, w.release[0], w.release[1], L.VALUE_TRIGGER)
        g.process_block()
    assert g.resident_stats() == (4, 1)
    assert g.event_stats() == (0, 0, 0)
    g.close()
