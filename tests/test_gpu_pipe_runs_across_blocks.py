"""Quiet runs of the pipeline kernel that carry on over the end of a block (voice_pipe.hpp, pipe_run_group): in a launch of
several blocks a run of whole, event-free tiles no longer ends with its block -- the frame goes back to the launch's first,
the block index and the absolute frame move on, and the next block's tile 0 is the run's next tile.  What can go wrong is where
such a run must NOT carry on (an event due at the block's end, at frame 0 of the next block or inside its first tile; a block
that is no whole number of tiles; the launch's last block; a stage with work at the block's end; an envelope whose partial-block
origin a queued change has moved), and what it carries with it when it does (the frame the envelope's done mark counts from,
the block a folding group writes to, the filter's choice of step, the tile buffers).

So: the smallest banks (a full group, a group with one live lane, three groups with a ragged last one), block sizes of one tile
(every tile ends a block), of a few tiles, of the headline's eight, and one that is no multiple of the tile; 8 to 16 blocks
to a launch, and one block.  Every case compares the launch of all blocks, bit for bit, with one launch per block of a bank of
the same shape; its flags and done frames with the single-wavefront kernel's (KNH_PIPELINE=0: no pipeline, no runs); and the
per-block launches' per-voice signals, done frames and done flag with the CPU oracle for the C3-shaped chains."""
import numpy as np
import pytest

from helpers import assert_bit_equal, make_gpu, make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

pytestmark = pytest.mark.gpu

SINGLE = {"KNH_PIPELINE": "0"}
# f32: 32-sample tiles and a mixer wavefront / 64-sample tiles, the last group folding / 64-sample tiles, the last group in place
# (f64: half of each).  These are what the switches ASK for: the library reports the kind of kernel a bank took (a wave pipeline
# or whole-chain wavefronts: _took), not the layout, and it gives a block that is no whole number of long tiles the mixer layout
# whatever was asked (kernel_form.hpp, plan_forms) -- for such a block the three entries run the same kernel three times.
FORMS = {"mixer": {"KNH_PIPELINE": "1", "KNH_PIPE_BIG": "0"}, "fold": {"KNH_PIPELINE": "1", "KNH_PIPE_BIG": "1"},
         "inplace": {"KNH_PIPELINE": "1", "KNH_PIPE_BIG": "2"}}
NONE = 0xFFFFFFFF


def _bank(knh, monkeypatch, w, env, mix=L.MIX_TREE):
    with monkeypatch.context() as m:  # (the switches are read when a bank is created and initialised)
        for k, v in env.items():
            m.setenv(k, v)
        return make_gpu(knh, w, mix)


def _took(bank, env):
    form = int(bank.debug_words()[2])
    if env.get("KNH_PIPELINE") == "0":
        assert form in (L.DEBUG_FORM_WHOLE_CHAIN, L.DEBUG_FORM_WHOLE_CHAIN_FUSED), form
    else:
        assert form in (L.DEBUG_FORM_PIPELINE, L.DEBUG_FORM_PIPELINE_FUSED), form


def _c3_timed(n, bs, sample_type, env_times=None):
    """the C3 chain with the filter and the envelope behind WrPreciseTiming: their changes land on a frame of the block"""
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF, delayed_changes_per_block=2),
          Stage(L.STAGE_MUL_ENV_ASR, delayed_changes_per_block=2)]
    w = configs.Workload("across", st, n, bs, sample_type, 2)
    times = np.stack([p["attack"], p["release"]], axis=1) if env_times is None else env_times
    w.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 1.0 / n),
              2: np.stack([np.full(n, float(L.SVF_LOW)), p["cutoff"], p["q"], np.zeros(n)], axis=1), 3: times}
    w.restart = (3, 3)
    w.release = (3, 2, 0)
    return w


def _tile(sample_type):
    return 64 if sample_type == L.F32 else 32  # the long tiles (fold, in place); the mixer form's are half as long


# ---- where the events go.  A batch: (voices, stage, param, kind, floats, ints, delays-within-the-block) ----
def _plan(w, n_blocks, placement, env_stage=3, svf_stage=2):
    """{block: batches}.  Every plan starts the note in front of block 0 (the envelope is at rest before it: silence).
    "edges": one kind of placement per block, blocks without any between them --
       block 2  a new cutoff for every voice at frame 0: the same frame in all lanes, frame 0 of a middle block
       block 3  a release on every third voice at the block's last frame
       block 5  a new cutoff on another third, due exactly at the block's end (frame == block_size)
       block 7  a restart of ONE voice, the last live lane of the (partial) last group, in the first tile behind the boundary
    "first_tile": block 1: a cutoff change per voice on a frame of its own inside the first tile behind the boundary; block 4: a
       release of every voice at frame 0; block 6: a new cutoff for the last voice alone at the block's last frame.
    "none": nothing after the note on."""
    n, bs = w.n_voices, w.block_size
    v = np.arange(n, dtype=np.uint32)
    p = configs.voice_parameters(n)
    t = min(_tile(w.sample_type), bs)
    plan = {0: [(v, env_stage, 3, L.VALUE_TRIGGER, None, None, None)]}
    u16 = lambda a: np.asarray(a, dtype=np.uint16)
    if placement == "edges":
        plan[2] = [(v, svf_stage, 0, L.VALUE_FLOAT, p["cutoff"] * 0.5, None, None)]
        a = v[v % 3 == 0]
        plan[3] = [(a, env_stage, 2, L.VALUE_TRIGGER, None, None, u16(np.full(len(a), bs - 1)))]
        b = v[v % 3 == 1]
        plan[5] = [(b, svf_stage, 0, L.VALUE_FLOAT, p["cutoff"][b] * 1.5, None, u16(np.full(len(b), bs)))]
        plan[7] = [(v[-1:], env_stage, 3, L.VALUE_TRIGGER, None, None, u16([min(3, bs - 1)]))]
    elif placement == "first_tile":
        plan[1] = [(v, svf_stage, 0, L.VALUE_FLOAT, p["cutoff"] * 0.75, None, u16((v * 5 + 1) % t))]
        plan[4] = [(v, env_stage, 2, L.VALUE_TRIGGER, None, None, None)]
        plan[6] = [(v[-1:], svf_stage, 0, L.VALUE_FLOAT, p["cutoff"][-1:] * 1.25, None, u16([bs - 1]))]
    else:
        assert placement == "none"
    return {blk: b for blk, b in plan.items() if blk < n_blocks}


def _apply(bank, batches, offset=0):
    for (v, s, p, kind, f, i, d) in batches:
        if offset:
            bank.param_apply_prepared(bank.prepare_many(v, s, p, kind, f, i, d), offset)  # scheduled ahead, for block `offset` of the launch
        else:
            bank.param_apply_many(v, s, p, kind, f, i, d)


def _oracle(oracle, w, plan, n_blocks):
    """-> per block (voices, done frames, flags), rendered once and left unchanged"""
    o = make_oracle(oracle, w)
    res = []
    for blk in range(n_blocks):
        _apply(o, plan.get(blk, []))
        _, ov, of, od = o.process_block()
        ov.setflags(write=False)
        res.append((ov, od.copy(), of))
    o.close()
    return res


def _launch(knh, monkeypatch, w, env, plan, n_blocks, took=True):
    """all blocks in one launch, the changes scheduled ahead -> (mix [blocks, ch, B], flags, done frames)"""
    g = _bank(knh, monkeypatch, w, env)
    for blk, batches in plan.items():
        _apply(g, batches, blk)
    out, flags = g.process_blocks(n_blocks)
    done = g.read_done_frames()
    if took:
        _took(g, env)
    g.close()
    return out, flags, done


def _last_marks(per_block_done):
    """the done frame a launch of all the blocks ends up with: each voice's mark of the last block that set one"""
    acc = np.full_like(per_block_done[0], NONE)
    for d in per_block_done:
        acc = np.where(d != NONE, d, acc)
    return acc


def _check(knh, oracle, monkeypatch, w, plan, n_blocks, forms, want, voice_tol=0.0, took=True):
    """want: the oracle's blocks.  voice_tol: the per-voice signals are the oracle's within this, not bit for bit (and the chain
    has no envelope: no done frames).  took: assert the kernel form each bank took (a wave pipeline; whole-chain wavefronts for
    KNH_PIPELINE=0)."""
    single = _launch(knh, monkeypatch, w, SINGLE, plan, n_blocks, took)
    assert np.abs(single[0]).max() > 1e-6
    if not voice_tol:
        np.testing.assert_array_equal(single[2], _last_marks([d for _, d, _ in want]))
    for form, env in forms.items():
        out, flags, done = _launch(knh, monkeypatch, w, env, plan, n_blocks, took)
        assert_bit_equal(out, single[0], f"{form}: {n_blocks} blocks in one launch against the single-wavefront kernel")
        assert flags == single[1], (form, flags, single[1])
        np.testing.assert_array_equal(done, single[2])
        g = _bank(knh, monkeypatch, w, env)  # one launch per block
        for blk in range(n_blocks):
            _apply(g, plan.get(blk, []))
            o, voices, f = g.process_block_voices()
            assert_bit_equal(o, out[blk], f"{form}: block {blk} of the launch against a launch of its own")
            if voice_tol:
                err = float(np.max(np.abs(voices.astype(np.float64) - want[blk][0].astype(np.float64))))
                assert err <= voice_tol, (form, blk, err)
            else:
                assert_bit_equal(voices, want[blk][0], f"{form}: block {blk} per-voice against the oracle")
                np.testing.assert_array_equal(g.read_done_frames(), want[blk][1])
                assert (f & L.FLAG_ANY_DONE) == (want[blk][2] & L.FLAG_ANY_DONE), (form, blk)
        if took:
            _took(g, env)
        g.close()


# The tile a bank's kernel has follows from its block (kernel_form.hpp, plan_forms): the 64-sample-tile layouts (fold, in place;
# f64: 32) are taken only where the block is a whole number of those tiles, every other block goes to the mixer layout's
# 32-sample tiles (f64: 16), whatever KNH_PIPE_BIG says.
# f32, 64-sample tiles: blocks of one tile (every tile ends a block), two, and the headline's eight; f64, 32-sample tiles: one
# tile and two.  (In the mixer form these are two, four and sixteen tiles.)  Block 96 is the mixer layout's in all three forms,
# three whole 32-sample tiles: its runs carry on.  A full group, a group with one live lane, three groups with two live lanes in
# the last.
SHAPES = [(64, 64, L.F32, 16), (65, 128, L.F32, 8), (130, 512, L.F32, 8), (130, 96, L.F32, 8), (130, 64, L.F32, 9),
          (130, 32, L.F64, 16), (65, 64, L.F64, 8), (130, 128, L.F32, 1)]
# Blocks that are a whole number of tiles in NO form -- one and a half and two and a half of the shortest tile a pipeline has
# (f32 32, f64 16), so of the mixer layout every one of these banks takes: the last tile of every block is a partial one, no run
# may carry on over it (cross_ok's "whole tiles" term), and every block ends on the path it always had.  A run that wrapped at
# the last WHOLE tile would skip the partial one.
SHORTEST_TILE = {L.F32: 32, L.F64: 16}
RAGGED = [(130, 48, L.F32, 9), (65, 80, L.F32, 8), (130, 24, L.F64, 9), (65, 40, L.F64, 8)]


@pytest.mark.parametrize("placement", ["edges", "first_tile", "none"])
@pytest.mark.parametrize("n,bs,sample_type,n_blocks", SHAPES)
def test_c3_launch_of_many_blocks(knh, oracle, monkeypatch, n, bs, sample_type, n_blocks, placement):
    w = _c3_timed(n, bs, sample_type)
    plan = _plan(w, n_blocks, placement)
    _check(knh, oracle, monkeypatch, w, plan, n_blocks, FORMS, _oracle(oracle, w, plan, n_blocks))


@pytest.mark.parametrize("placement", ["edges", "first_tile", "none"])
@pytest.mark.parametrize("n,bs,sample_type,n_blocks", RAGGED)
def test_blocks_with_a_partial_last_tile_end_every_run(knh, oracle, monkeypatch, n, bs, sample_type, n_blocks, placement):
    """(_check asserts that every bank ran a wave pipeline; that its tile does not divide the block follows from the block:
    no pipeline has a tile shorter than SHORTEST_TILE, and the longer ones are its double.)"""
    assert bs % SHORTEST_TILE[sample_type] != 0 and bs > SHORTEST_TILE[sample_type]
    w = _c3_timed(n, bs, sample_type)
    plan = _plan(w, n_blocks, placement)
    _check(knh, oracle, monkeypatch, w, plan, n_blocks, FORMS, _oracle(oracle, w, plan, n_blocks))


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_envelope_arrives_and_runs_out_next_to_a_block_end(knh, oracle, monkeypatch, sample_type):
    """Blocks of two long tiles.  Voice v's attack takes 2 T + 2 + (v mod 2 T - 8) samples and its release as long: started at
    frame 0 of a block, the attack arrives -- and the release, triggered at frame 0 of block 4, runs out -- in the NEXT block,
    for some voices in its first tile (the first tile behind a block end a run has carried on over), for the others in its
    second (the last tile in front of one).  The done frame counts from the start of the block the release ran out in, and
    "no envelope is running any more" is what the launch reports: two launches of four blocks, the first ending with every
    voice sustaining, the second with every voice stopped."""
    n, t = 130, _tile(sample_type)
    bs = 2 * t
    v = np.arange(n, dtype=np.uint32)
    samples = bs + 2 + (v % (bs - 8))
    w = _c3_timed(n, bs, sample_type, np.stack([samples / 48000.0, samples / 48000.0], axis=1))
    plan = {0: [(v, 3, 3, L.VALUE_TRIGGER, None, None, None)], 4: [(v, 3, 2, L.VALUE_TRIGGER, None, None, None)]}
    want = _oracle(oracle, w, plan, 8)
    out_in = {u for u in np.unique(want[5][1]) if u != NONE}
    assert any(u < t for u in out_in) and any(u >= t for u in out_in), "releases run out in both tiles of block 5"
    assert all((d == NONE).all() for k, (_, d, _) in enumerate(want) if k != 5)
    flags_of = {}
    for form, env in {"single": SINGLE, **FORMS}.items():
        g = _bank(knh, monkeypatch, w, env)  # one launch per block
        ref = []
        for blk in range(8):
            _apply(g, plan.get(blk, []))
            o, voices, f = g.process_block_voices()
            assert_bit_equal(voices, want[blk][0], f"{form}: block {blk} per-voice against the oracle")
            np.testing.assert_array_equal(g.read_done_frames(), want[blk][1])
            ref.append((o, f))
        g.close()
        g = _bank(knh, monkeypatch, w, env)  # two launches of four blocks
        _apply(g, plan[0])
        first, f1 = g.process_blocks(4)
        assert (g.read_done_frames() == NONE).all()
        _apply(g, plan[4])
        second, f2 = g.process_blocks(4)
        np.testing.assert_array_equal(g.read_done_frames(), want[5][1])
        _took(g, env)
        g.close()
        for blk in range(8):
            assert_bit_equal((first if blk < 4 else second)[blk % 4], ref[blk][0], f"{form}: block {blk} of its launch against a launch of its own")
        assert not (f1 & L.FLAG_ALL_DONE) and (f2 & L.FLAG_ALL_DONE), (form, f1, f2)
        flags_of.setdefault("single", (f1, f2))
        assert (f1, f2) == flags_of["single"], (form, f1, f2, flags_of["single"])
        assert (ref[7][1] & L.FLAG_ALL_DONE) and not (ref[3][1] & L.FLAG_ALL_DONE), form


def test_a_queued_change_moves_the_envelopes_origin(knh, oracle, monkeypatch):
    """A queued (WrPreciseTiming) change of the envelope starts a new partial block at its frame, and the done mark of a release
    that runs out later IN THAT BLOCK counts from there; from the next block on it counts from frame 0 again.  A run that
    starts behind such a change stays in its block (Chain::block_begun), so the mark of a release that runs out one block
    later is the oracle's.  Blocks of four tiles; the release is triggered at frame 70 of block 2 and lasts 100 samples on the
    even voices (out in block 2, counted from frame 70) and 300 on the odd ones (out in block 3, counted from its frame 0)."""
    n, bs = 130, 256
    v = np.arange(n, dtype=np.uint32)
    rel = np.where(v % 2 == 0, 100.0, 300.0) + (v % 7)
    w = _c3_timed(n, bs, L.F32, np.stack([np.full(n, 40.0 / 48000.0), rel / 48000.0], axis=1))
    plan = {0: [(v, 3, 3, L.VALUE_TRIGGER, None, None, None)],
            2: [(v, 3, 2, L.VALUE_TRIGGER, None, None, np.full(n, 70, dtype=np.uint16))]}
    want = _oracle(oracle, w, plan, 6)
    assert (want[2][1][0::2] != NONE).all() and (want[3][1][1::2] != NONE).all() and (want[3][1][1::2] > 70).all()
    _check(knh, oracle, monkeypatch, w, plan, 6, FORMS, want)


# Other kinds of stage group, eight blocks of two long tiles, a release in block 4 and nothing else after the note on:
#   P3  a Pan2 behind the envelope: its gains ride in the padding of every tile's rows, a carried-on run's tiles included
#   D3  a delay line in the envelope's group: the group has work at every block's end (its ring is bound there) and its runs
#       end with their block, as they always did -- while the oscillator's and the filter's groups beside it carry on
#   C2  SinNumeric's phase | its sine over eight wavefronts (a Fan group), and no event at all: the phase and the sine stages
#       have not declared themselves free of block work, so every wavefront of this pipeline ends its runs with the block
@pytest.mark.parametrize("name,voice_tol", [("P3", 0.0), ("D3", 0.0), ("C2", 1e-5 / 130)])
def test_other_kinds_of_stage_group(knh, oracle, monkeypatch, name, voice_tol):
    """voice_tol: C2's device sine is within 1e-5 of full scale of the oracle's by design (the voices' gain is 1 / 130;
    tests/test_gpu_parity.py::test_c2_sin_numeric_within_tolerance); the launches among themselves are bit-identical.
    All three chains have pre-built pipelines (kernels_pipe.hip: WmSAJ, WmSDA, Nm); _check asserts that they were taken."""
    w = configs.config(name, n_voices=130, block_size=128)
    v = np.arange(w.n_voices, dtype=np.uint32)
    plan = {}
    if w.restart:
        plan[0] = [(v, w.restart[0], w.restart[1], L.VALUE_TRIGGER, None, None, None)]
        plan[4] = [(v[::3], w.release[0], w.release[1], L.VALUE_TRIGGER, None, None, None)]
    if w.delay_times is not None:  # 24 .. 190 samples, different per voice: the delayed signal arrives within these blocks
        plan[0].append((v, 3, 0, L.VALUE_FLOAT, 0.0005 + 0.0005 * (v % 8), None, None))
    _check(knh, oracle, monkeypatch, w, plan, 8, FORMS, _oracle(oracle, w, plan, 8), voice_tol)


def test_a_filter_behind_a_gain_in_its_group(knh, oracle, monkeypatch):
    """Group<WhiteNoise> | Group<MulVal, Svf> | Group<MulAsr> (the run-time fusion's cut: tests/test_gpu_pipe_quiet_runs.py):
    the filter's state leaves its fixed registers through the stage in front of it, tile after tile of a run -- now also from
    a block's last tile to the next block's first.  (The noise source has not declared itself free of block work: group 0
    ends its runs with the block beside two groups that carry on.)"""
    n, bs = 130, 64
    v = np.arange(n, dtype=np.uint32)
    p = configs.voice_parameters(n)
    w = configs.Workload("noise", [Stage(L.STAGE_WHITE_NOISE), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)], n, bs, L.F32, 2)
    w.ctor = {0: v.astype(np.float64).reshape(n, 1), 1: np.full((n, 1), 1.0 / n),
              2: np.stack([np.zeros(n), p["cutoff"], p["q"], np.zeros(n)], axis=1), 3: np.stack([p["attack"], p["release"]], axis=1)}
    plan = {0: [(v, 3, 3, L.VALUE_TRIGGER, None, None, None)], 5: [(v[1::2], 2, 0, L.VALUE_FLOAT, p["cutoff"][1::2] * 0.5, None, None)]}
    forms = {"pipe": {"KNH_PIPELINE": "1"}}
    _check(knh, oracle, monkeypatch, w, plan, 8, forms, _oracle(oracle, w, plan, 8))
    g = _bank(knh, monkeypatch, w, forms["pipe"])
    assert int(g.debug_words()[2]) == L.DEBUG_FORM_PIPELINE_FUSED
    g.close()


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_frames_strictly_inside_the_block(knh, oracle, monkeypatch, sample_type):
    """A call over frames [T, 3 T) of a block of four long tiles, between a call over [0, T) and one over [3 T, 4 T): launches of
    one block whose tiles are whole and whose frames end short of the block -- nothing to carry on into, today's path."""
    t = _tile(sample_type)
    w = _c3_timed(130, 4 * t, sample_type)
    plan = _plan(w, 3, "edges")
    want = _oracle(oracle, w, plan, 3)
    for form, env in {"single": SINGLE, **FORMS}.items():
        g = _bank(knh, monkeypatch, w, env)
        for blk in range(3):
            _apply(g, plan.get(blk, []))
            if blk == 1:
                parts = [g.process_block_voices(n, at)[1] for at, n in ((0, t), (t, 2 * t), (3 * t, t))]
                voices = np.concatenate([parts[0][:, :t], parts[1][:, t:3 * t], parts[2][:, 3 * t:]], axis=1)
            else:
                voices = g.process_block_voices()[1]
            assert_bit_equal(voices, want[blk][0], f"{form}: block {blk} per-voice against the oracle")
        g.close()
