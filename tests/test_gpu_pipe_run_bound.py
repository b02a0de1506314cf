"""The quiet run's event bound as a scalar, the filter's registers resident for a run, the tile addresses carried from tile to
tile (voice_pipe.hpp, pipe_run_group; voice_stages.hpp, Svf::run_enter / tick_tile_fixed / run_leave).  A run that goes on to a
second tile takes the minimum of its 64 lanes' next event frames once and from then on compares a scalar; a run of a group that
carries on over block ends folds "no whole tile left in the block" into the same compare; a filter alone in its stage group
keeps ic1, ic2 and its coefficients in the fixed registers of its step from the run's first tile to its last.  What can go
wrong: the minimum (a lane left out, the dead lanes of a partial group, the 0xFFFFFFFF of a lane without an event, an off-by-one
at a tile's or a block's end), the bound after a block end (last_due, the wrap), a run of one tile (no minimum taken), registers
that are stale when the next run begins (coefficients a SET has changed, a state a trigger's tile has moved on).

The cases are banks of 65 or 130 voices (two or three voice groups, the last with one or two live lanes), each with a lead-in launch of
one block that starts the note (so that the launch under test can be without any event at all), and then ONE launch of 1 to 8
blocks of 128 or 192 frames (and of one and a half short tiles) with the case's events scheduled ahead.  Each is compared, bit for bit, with the single-wavefront
kernel (KNH_PIPELINE=0: no pipeline, no runs) and with one launch per block of a bank of the same shape, in every pipeline
form: 32-sample tiles and a mixer wavefront (KNH_PIPE_BIG=0), 64-sample tiles with the last group folding or in place, two
voice groups per workgroup (f32); f64 with half those tiles.  The per-block launches' per-voice signals and done frames are the
CPU oracle's where a case says so (one placement per form, and the cases about the filter's registers)."""
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
PAIR = {"pair": {"KNH_PIPELINE": "1", "KNH_PAIR": "1"}}  # two voice groups per workgroup; three groups: one of the four is dead
ENV, SVF = 3, 2  # the C3 chain's envelope and filter stages


def _bank(knh, monkeypatch, w, env):
    with monkeypatch.context() as m:  # (the switches are read when a bank is created and initialised)
        for k, v in env.items():
            m.setenv(k, v)
        return make_gpu(knh, w, L.MIX_TREE)


def _took(bank, env):
    form = int(bank.debug_words()[2])
    if env.get("KNH_PIPELINE") == "0":
        assert form in (L.DEBUG_FORM_WHOLE_CHAIN, L.DEBUG_FORM_WHOLE_CHAIN_FUSED), form
    else:
        assert form in (L.DEBUG_FORM_PIPELINE, L.DEBUG_FORM_PIPELINE_FUSED), form


def _c3_timed(n, bs, sample_type):
    """the C3 chain with the filter and the envelope behind WrPreciseTiming: their changes land on a frame of the block"""
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF, delayed_changes_per_block=2),
          Stage(L.STAGE_MUL_ENV_ASR, delayed_changes_per_block=2)]
    w = configs.Workload("bound", st, n, bs, sample_type, 2)
    w.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 1.0 / n),
              2: np.stack([np.full(n, float(L.SVF_LOW)), p["cutoff"], p["q"], np.zeros(n)], axis=1),
              3: np.stack([p["attack"], p["release"]], axis=1)}
    return w


def _tile(sample_type):
    return 64 if sample_type == L.F32 else 32  # the long tiles (fold, in place); the mixer form's are half as long


def _note_on(n):
    return [(np.arange(n, dtype=np.uint32), ENV, 3, L.VALUE_TRIGGER, None, None, None)]


def _cutoffs(v, frames, scale=0.5):
    """a new cutoff for each of the voices v, each at its own frame of the block (a SET of the filter's six coefficients)"""
    p = configs.voice_parameters(int(v.max()) + 1)
    return (v, SVF, 0, L.VALUE_FLOAT, p["cutoff"][v] * scale, None, np.asarray(frames, dtype=np.uint16))


# ---- where the events go: {block of the launch under test: batches}.  The launch's block b is the bank's block b + 1. ----
def _plan(n, bs, t, placement):
    """Every voice group has ONE lane whose event is the group's earliest, a different lane in each (in the last, partial group
    of a 130-voice bank one of its two live lanes, in that of a 65-voice bank its only one), exactly at the placement's frame;
    every other even lane has one 3, 6, 9 or 12 frames later (in the next block where the block is over by then) and the odd
    lanes have none (0xFFFFFFFF):
       behind_1 / behind_2   the first frame behind exactly one / two whole tiles of block 1
       behind_block          ... behind all the tiles of block 1: frame 0 of block 2, scheduled there
       tile_last             the last frame of block 1's first tile
       block_last            block 1's last frame
       block_end             the end of block 1 itself (frame == block size: due before block 2 begins)
       next_first_tile       inside the first tile of block 2
    "none": no event in the whole launch.  "one_lane": the last live lane of the last group, alone, in the second tile of block
    1.  "first_tile_only": events in the first and in the third tile of block 1 and nowhere else -- the quiet tile between them
    is a run of one tile, which ends without the minimum taken; the tiles behind them a run that takes it with every lane at
    0xFFFFFFFF."""
    v = np.arange(n, dtype=np.uint32)
    if placement == "none":
        return {}
    if placement == "one_lane":
        return {1: [_cutoffs(v[-1:], [t + 5])]}
    if placement == "first_tile_only":
        a, b = v[v % 3 == 0], v[v % 3 == 1]
        return {1: [_cutoffs(a, np.full(len(a), 5)), _cutoffs(b, np.full(len(b), 2 * t + 5), 0.75)]}
    blk, f0 = {"behind_1": (1, t), "behind_2": (1, 2 * t), "behind_block": (2, 0), "tile_last": (1, t - 1), "block_last": (1, bs - 1),
               "block_end": (1, bs), "next_first_tile": (2, 3)}[placement]
    plan = {}
    for g0 in range(0, n, 64):
        lanes = np.arange(min(64, n - g0))
        first = (7 * (g0 // 64) + 5) % len(lanes)  # the lane whose event is the group's earliest
        for lane in lanes[(lanes % 2 == 0) | (lanes == first)]:
            at = f0 + 3 * ((int(lane) - first) % 5)
            where = (blk, bs) if at == bs and placement == "block_end" else (blk + at // bs, at % bs)
            plan.setdefault(where[0], {}).setdefault("v", []).append(g0 + int(lane))
            plan[where[0]].setdefault("f", []).append(where[1])
    return {b: [_cutoffs(np.asarray(d["v"], dtype=np.uint32), d["f"])] for b, d in plan.items()}


PLACEMENTS = ["none", "one_lane", "behind_1", "behind_2", "behind_block", "tile_last", "block_last", "block_end", "next_first_tile",
              "first_tile_only"]


def _apply(bank, batches, offset=0):
    for (v, s, p, kind, f, i, d) in batches:
        if offset:
            bank.param_apply_prepared(bank.prepare_many(v, s, p, kind, f, i, d), offset)  # scheduled ahead, for block `offset` of the launch
        else:
            bank.param_apply_many(v, s, p, kind, f, i, d)


def _oracle(oracle, w, lead, plan, n_blocks):
    """-> per block of the launch under test (voices, done frames, flags), rendered once and left unchanged"""
    o = make_oracle(oracle, w)
    _apply(o, lead)
    o.process_block()
    res = []
    for blk in range(n_blocks):
        _apply(o, plan.get(blk, []))
        _, ov, of, od = o.process_block()
        ov.setflags(write=False)
        res.append((ov, od.copy(), of))
    o.close()
    return res


def _launch(knh, monkeypatch, w, env, lead, plan, n_blocks):
    """the lead-in block, then all blocks in one launch with the changes scheduled ahead -> (mix [blocks, ch, B], flags, done frames)"""
    g = _bank(knh, monkeypatch, w, env)
    _apply(g, lead)
    g.process_blocks(1)
    for blk, batches in plan.items():
        _apply(g, batches, blk)
    out, flags = g.process_blocks(n_blocks)
    done = g.read_done_frames()
    _took(g, env)
    g.close()
    return out, flags, done


def _check(knh, oracle, monkeypatch, w, plan, n_blocks, forms, with_oracle, lead=None):
    lead = _note_on(w.n_voices) if lead is None else lead
    assert all(blk < n_blocks for blk in plan)
    want = _oracle(oracle, w, lead, plan, n_blocks) if with_oracle else None
    single = _launch(knh, monkeypatch, w, SINGLE, lead, plan, n_blocks)
    assert np.abs(single[0]).max() > 1e-6
    for form, env in forms.items():
        out, flags, done = _launch(knh, monkeypatch, w, env, lead, plan, n_blocks)
        assert_bit_equal(out, single[0], f"{form}: {n_blocks} blocks in one launch against the single-wavefront kernel")
        assert flags == single[1], (form, flags, single[1])
        np.testing.assert_array_equal(done, single[2])
        g = _bank(knh, monkeypatch, w, env)  # one launch per block
        _apply(g, lead)
        g.process_block_voices()
        for blk in range(n_blocks):
            _apply(g, plan.get(blk, []))
            o, voices, f = g.process_block_voices()
            assert_bit_equal(o, out[blk], f"{form}: block {blk} of the launch against a launch of its own")
            if want is not None:
                assert_bit_equal(voices, want[blk][0], f"{form}: block {blk} per-voice against the oracle")
                np.testing.assert_array_equal(g.read_done_frames(), want[blk][1])
                assert (f & L.FLAG_ANY_DONE) == (want[blk][2] & L.FLAG_ANY_DONE), (form, blk)
        _took(g, env)
        g.close()


# f32: blocks of three 64-sample tiles (six of the mixer form's), f64: of six 32-sample tiles, three voice groups with two live
# lanes in the last: every placement.  Blocks of two tiles (f64: four), two groups with one live lane in the last, eight and four
# blocks to a launch: the placements at the block's end (two whole tiles are the whole block there) and the two without a
# minimum to find.  The oracle joins in for one placement per shape -- a lane's event exactly where a block ends -- in every form.
CASES = [(130, 192, st, 4, pl) for st in (L.F32, L.F64) for pl in PLACEMENTS]
CASES += [(65, 128, st, nb, pl) for st, nb in ((L.F32, 8), (L.F64, 4)) for pl in ("none", "one_lane", "block_last", "block_end", "behind_block")]


@pytest.mark.parametrize("n,bs,sample_type,n_blocks,placement", CASES)
def test_where_the_earliest_event_of_a_wavefront_sits(knh, oracle, monkeypatch, n, bs, sample_type, n_blocks, placement):
    w = _c3_timed(n, bs, sample_type)
    forms = {**FORMS, **PAIR} if sample_type == L.F32 else FORMS
    plan = _plan(n, bs, _tile(sample_type), placement)
    _check(knh, oracle, monkeypatch, w, plan, n_blocks, forms, with_oracle=placement == "block_end")


@pytest.mark.parametrize("n_blocks", [1, 2])
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_short_launches(knh, oracle, monkeypatch, sample_type, n_blocks):
    """One block: nothing to carry on into, the bound still ends the run with the block.  Two: one block end, the launch's last
    behind it.  An event of one lane in the last tile of the launch."""
    t = _tile(sample_type)
    w = _c3_timed(130, 2 * t, sample_type)
    plan = {n_blocks - 1: [_cutoffs(np.array([64], dtype=np.uint32), [t + 1])]}
    _check(knh, oracle, monkeypatch, w, plan, n_blocks, FORMS, with_oracle=False)


@pytest.mark.parametrize("n,bs,sample_type", [(130, 48, L.F32), (65, 24, L.F64)])
def test_blocks_of_one_and_a_half_tiles(knh, oracle, monkeypatch, n, bs, sample_type):
    """One and a half of the shortest tile a pipeline has (f32 32, f64 16), which every form then takes: the block's second tile
    is a partial one, no run carries on over it, and the run of its one whole tile ends with the block's whole tiles whatever
    the lanes' events say -- none at all (block 0), one lane's far ahead (its event is in block 3), every lane's in the partial
    tile (block 2)."""
    w = _c3_timed(n, bs, sample_type)
    v = np.arange(n, dtype=np.uint32)
    plan = {2: [_cutoffs(v, np.full(n, bs - 2))], 3: [_cutoffs(v[-1:], [3], 0.75)]}
    _check(knh, oracle, monkeypatch, w, plan, 5, FORMS, with_oracle=True)


@pytest.mark.parametrize("sample_type,bs", [(L.F32, 128), (L.F32, 192), (L.F64, 128)])
def test_a_run_that_starts_with_ic2_minus_zero(knh, oracle, monkeypatch, sample_type, bs):
    """Every third voice's filter starts with ic2eq = -0.0 (KNH_DEBUG_SVF_IC2_NEG0=1, a test-only switch of the library): the
    first run of every wavefront -- here the whole launch, three blocks without an event behind the note-on at its frame 0 --
    takes the general step, with the filter's state resident in the step's registers from tile to tile and over two block ends.
    A state that did not advance, or came out of the wrong registers at the run's end, shows against the single-wavefront kernel
    here and in the launch behind it, whose runs take the low-pass step from the state this one left.  (The oracle starts from
    +0.0: the two starts differ in the sign of a zero at most, which assert_bit_equal lets pass.)"""
    monkeypatch.setenv("KNH_DEBUG_SVF_IC2_NEG0", "1")
    w = _c3_timed(130, bs, sample_type)
    res = {}
    for form, env in {"single": SINGLE, **FORMS}.items():
        g = _bank(knh, monkeypatch, w, env)
        _apply(g, _note_on(130))
        first, _ = g.process_blocks(3)
        second, _ = g.process_blocks(2)
        _took(g, env)
        g.close()
        res[form] = np.concatenate([first, second])
    monkeypatch.delenv("KNH_DEBUG_SVF_IC2_NEG0")
    assert np.abs(res["single"]).max() > 1e-6
    for form in FORMS:
        assert_bit_equal(res[form], res["single"], f"{form}: five blocks in two launches against the single-wavefront kernel")
    o = make_oracle(oracle, w)
    _apply(o, _note_on(130))
    g = _bank(knh, monkeypatch, w, FORMS["inplace"])  # (from +0.0, block by block: the oracle's samples)
    _apply(g, _note_on(130))
    for blk in range(5):
        assert_bit_equal(g.process_block_voices()[1], o.process_block()[1], f"block {blk} per-voice against the oracle")
    g.close()
    o.close()


def test_a_filter_behind_a_gain_in_its_group(knh, oracle, monkeypatch):
    """Group<WhiteNoise> | Group<MulVal, Svf> | Group<MulAsr> (the run-time fusion's cut): the filter is not alone in its group,
    so its state goes to and from the step's registers tile by tile, through the stage in front of it -- the shape in which the
    compiler once lost the copy out of them -- now inside the run loop with the scalar bound and the carried addresses.  Three
    blocks in one launch, a new cutoff for every other voice in the second."""
    n, bs = 130, 128
    v = np.arange(n, dtype=np.uint32)
    p = configs.voice_parameters(n)
    w = configs.Workload("noise", [Stage(L.STAGE_WHITE_NOISE), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF), Stage(L.STAGE_MUL_ENV_ASR)], n, bs, L.F32, 2)
    w.ctor = {0: v.astype(np.float64).reshape(n, 1), 1: np.full((n, 1), 1.0 / n),
              2: np.stack([np.zeros(n), p["cutoff"], p["q"], np.zeros(n)], axis=1), 3: np.stack([p["attack"], p["release"]], axis=1)}
    plan = {1: [(v[1::2], SVF, 0, L.VALUE_FLOAT, p["cutoff"][1::2] * 0.5, None, None)]}
    forms = {"pipe": {"KNH_PIPELINE": "1"}}
    _check(knh, oracle, monkeypatch, w, plan, 3, forms, with_oracle=True)
    g = _bank(knh, monkeypatch, w, forms["pipe"])
    assert int(g.debug_words()[2]) == L.DEBUG_FORM_PIPELINE_FUSED
    g.close()


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_coefficients_and_state_change_between_two_runs_of_a_launch(knh, oracle, monkeypatch, sample_type):
    """In the second tile of block 1 every voice gets a new cutoff (six SETs of the filter's coefficients) and every other voice
    a restart of its envelope, each at a frame of its own; block 2 ends with a release on every third voice at its last frame.
    The runs in front of these tiles have the old coefficients in the step's registers, the runs behind them must have the new
    ones and the state the tiles between have left: the registers are loaded where a run begins, not where the launch does."""
    t = _tile(sample_type)
    n, bs = 130, 3 * t
    w = _c3_timed(n, bs, sample_type)
    v = np.arange(n, dtype=np.uint32)
    u16 = lambda a: np.asarray(a, dtype=np.uint16)
    plan = {1: [_cutoffs(v, t + 1 + (v * 5) % (t - 2), 0.4), (v[::2], ENV, 3, L.VALUE_TRIGGER, None, None, u16(t + (v[::2] * 3) % t))],
            2: [(v[::3], ENV, 2, L.VALUE_TRIGGER, None, None, u16(np.full(len(v[::3]), bs - 1)))]}
    forms = {**FORMS, **PAIR} if sample_type == L.F32 else FORMS
    _check(knh, oracle, monkeypatch, w, plan, 4, forms, with_oracle=True)
