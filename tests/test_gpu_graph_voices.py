"""Graph voices built from every stage kind, on the device (tests/graph_voices.py; tests/test_graph_voices.py is the part that
needs no GPU).  A voice that is a graph takes a kernel path no chain takes: signal slots handed out like registers, a copy
into the output slot in front of a stage's tile code, linked stages run sample by sample, the envelopes' task order naming
the done frame, eight-sample visits past sixteen stages.  Seeded random voices and six directed ones against the oracle,
bit for bit; a comb against numpy; one launch against block by block; the bank cut into voice ranges; ALL_DONE."""
import functools
import re

import numpy as np
import pytest

import graph_voices as gv
from helpers import assert_bit_equal, make_gpu
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

pytestmark = pytest.mark.gpu

NOT_DONE = gv.NOT_DONE
TYPES = [L.F32, L.F64]


def dtype_of(sample_type):
    return np.float64 if sample_type == L.F64 else np.float32


def against_the_oracle(knh, w, want, blocks, what):
    """The device bank of `w` block by block against oracle_run's `want`: every voice's signal (both planes under Pan2), the
    left-fold mix, the done frames, ANY_DONE.  -> the bank, still open"""
    voices, mixes, flags, done = want
    g = gv.gpu_bank(knh, w, L.MIX_LEFT_FOLD)
    for b in range(blocks):
        w.events(b, g)
        g_out, g_voices, g_flags = g.process_block_voices()
        assert_bit_equal(g_voices, voices[b], f"{what} block {b} per-voice")
        assert_bit_equal(g_out, mixes[b], f"{what} block {b} left-fold mix")
        np.testing.assert_array_equal(g.read_done_frames(), done[b], err_msg=f"{what} block {b} done frames")
        assert g_flags & L.FLAG_ANY_DONE == int(flags[b]) & L.FLAG_ANY_DONE, f"{what} block {b} ANY_DONE"
    return g


@pytest.mark.parametrize("seed", range(gv.N_SEEDS))
def test_random_graph_voice_matches_the_oracle(knh, oracle, seed):
    w = gv.random_graph_voice(seed)
    want = gv.oracle_run(oracle, w, 6)
    assert np.isfinite(want[0]).all() and np.abs(want[0]).max() > 1e-4
    g = against_the_oracle(knh, w, want, 6, f"seed {seed} {g_signature(knh, w)}")
    assert g.debug_words()[2] == L.DEBUG_FORM_WHOLE_CHAIN_FUSED  # (a silent change of form would empty the test)
    g.close()


def g_signature(knh, w):
    b = knh.VoiceBank(w.stages, 1, w.sample_type, w.out_channels, L.MIX_LEFT_FOLD)
    sig = b.debug_signature()
    b.close()
    return sig


@functools.lru_cache(maxsize=None)
def directed_reference(oracle, name, n, sample_type):
    return gv.oracle_run(oracle, gv.directed_voice(name, n, sample_type), 12)


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n", [3, 65, 130])
@pytest.mark.parametrize("name", gv.DIRECTED)
def test_directed_voice_matches_the_oracle(knh, oracle, name, n, sample_type):
    """Twelve blocks with the triggers that end the envelopes and the delay times moved: a partial wavefront, one lane over,
    a third wavefront."""
    w = gv.directed_voice(name, n, sample_type)
    want = directed_reference(oracle, name, n, sample_type)
    assert np.isfinite(want[0]).all() and (np.abs(want[0]).max(axis=(0, -1)) > 1e-4).all()
    if name == "nineteen":
        assert len(w.stages) > 16  # the eight-sample visits, where a delay's ring no longer moves through the LDS tile
    if name in ("comb_asr_pan", "three_envs", "reader_mix"):
        assert (want[3] != NOT_DONE).any(), "voices finish inside the run"
    if name == "three_envs":
        # the envelopes alone, in task order (EnvAsr, EnvAr, Envelope): where several finish in one block the voice's done
        # frame is the one of the last of them in that order -- list order would name the EnvAsr's
        alone = np.stack([gv.oracle_run(oracle, x, 12)[3] for x in gv.three_envs_alone(n, sample_type)])  # [3, blocks, n]
        together = (alone != NOT_DONE).sum(axis=0) >= 2
        assert together.any(), "two envelopes finish in one block"
        last = np.where(alone[2] != NOT_DONE, alone[2], np.where(alone[1] != NOT_DONE, alone[1], alone[0]))
        np.testing.assert_array_equal(want[3], last)
        in_list_order = np.where(alone[0] != NOT_DONE, alone[0], np.where(alone[2] != NOT_DONE, alone[2], alone[1]))
        assert (in_list_order[together] != last[together]).any(), "the two orders name different frames"
    against_the_oracle(knh, w, want, 12, f"{name} n={n}").close()


def comb_banks(n, bs, sample_type):
    p = configs.voice_parameters(n)
    dry = configs.Workload("gv_dry", [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST)], n, bs, sample_type, 1)
    dry.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 0.5)}
    comb = configs.Workload("gv_comb", dry.stages + [Stage(L.STAGE_SAMPLE_DELAY, input=2), Stage(L.STAGE_MATH_ADD, input=2, input2=3)],
                            n, bs, sample_type, 1)
    comb.ctor = dict(dry.ctor)
    comb.ctor[2] = np.full((n, 1), 0.006)  # a ring of 288 samples
    return dry, comb


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("sample_type", TYPES)
def test_comb_against_numpy(knh, sample_type, moved):
    """x + SampleDelay(x) with delay_time 0.001 s -- at 48 kHz exactly 48 samples -- is x[n] + x[n - 48], zeros before the
    start: numpy's from the per-voice output of a bank that is x alone, in the sample type.  One IEEE addition rounds the
    same on both sides: bit for bit, without the oracle.  moved: from block 3 on the odd voices' delay is 17 samples (17.5
    sample periods: delay_time * sample_rate is truncated)."""
    n, bs, blocks = 65, 64, 6
    dry, comb = comb_banks(n, bs, sample_type)
    v = np.arange(n, dtype=np.uint32)
    a, b = make_gpu(knh, dry, L.MIX_LEFT_FOLD), make_gpu(knh, comb, L.MIX_LEFT_FOLD)
    assert "D@" in b.debug_signature() and "@" not in a.debug_signature()
    b.param_apply_many(v, 2, 0, L.VALUE_FLOAT, np.full(n, 0.001))
    x, y = [], []
    for k in range(blocks):
        if moved and k == 3:
            b.param_apply_many(v[1::2], 2, 0, L.VALUE_FLOAT, np.full(len(v[1::2]), 17.5 / configs.SAMPLE_RATE))
        x.append(a.process_block_voices()[1])
        y.append(b.process_block_voices()[1])
    a.close()
    b.close()
    x, y = np.concatenate(x, axis=1), np.concatenate(y, axis=1)  # [n, blocks * bs]
    assert x.dtype == dtype_of(sample_type) and np.abs(x).max() > 0.4

    def delayed(d):
        out = np.zeros_like(x)
        out[:, d:] = x[:, :x.shape[1] - d]
        return out
    want = x + delayed(48)
    if moved:
        want[1::2, 3 * bs:] = (x + delayed(17))[1::2, 3 * bs:]
    assert_bit_equal(y, want, "x[n] + x[n - delay]")


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("name", ["comb_asr_pan", "reader_mix"])
def test_one_launch_equals_block_by_block(knh, name, sample_type):
    """Six blocks in one launch, the same six block by block, and each 64-frame block as 40 + 24 frames: identical bits,
    signs of zeros included (tree mix: the left fold takes one block per call)."""
    w = gv.directed_voice(name, 65, sample_type)
    whole, single, parts = (gv.gpu_bank(knh, w, L.MIX_TREE) for _ in range(3))
    for bank in (whole, single, parts):
        w.events(0, bank)
    many, _ = whole.process_blocks(6)
    assert np.abs(many).max() > 1e-4
    for k in range(6):
        out, _ = single.process_block()
        assert_bit_equal(out, many[k], f"{name} block {k}: block by block", strict_zero=True)
        split = np.zeros_like(out)
        parts.process_block(40, 0, out=split)
        parts.process_block(24, 40, out=split)
        assert_bit_equal(split, many[k], f"{name} block {k}: 40 + 24 frames", strict_zero=True)
    for bank in (whole, single, parts):
        bank.close()


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("form", ["host_threads", "devices", "rank"])
def test_bank_cut_into_voice_ranges(knh, form, sample_type):
    """The comb-ASR-Pan2 voice at 130 voices on two host threads, as two voice ranges of a multi-device bank (both on device
    0) and as one rank's share: the plain bank's voices bit for bit where the form hands them out (a rank bank gives the mix
    only), the mix within the 1e-5 tests/test_gpu_multi.py holds re-associated tree mixes to, the same done frames."""
    n = 130
    w = gv.directed_voice("comb_asr_pan", n, sample_type)
    kw = {"host_threads": dict(host_threads=2), "devices": dict(devices=[0, 0]), "rank": dict(rank=0, world=1)}[form]
    plain, other = gv.gpu_bank(knh, w, L.MIX_TREE), gv.gpu_bank(knh, w, L.MIX_TREE, **kw)
    peak, finished = 0.0, 0
    for b in range(12):
        w.events(b, plain)
        w.events(b, other)
        if form == "rank":
            p_out, _ = plain.process_block()
            o_out, _ = other.process_block()
        else:
            p_out, p_voices, _ = plain.process_block_voices()
            o_out, o_voices, _ = other.process_block_voices()
            assert_bit_equal(o_voices, p_voices, f"{form} block {b} per-voice", strict_zero=True)
        assert np.max(np.abs(o_out.astype(np.float64) - p_out.astype(np.float64))) <= 1e-5 * max(1.0, float(np.abs(p_out).max()))
        done = plain.read_done_frames()
        np.testing.assert_array_equal(other.read_done_frames(), done, err_msg=f"{form} block {b} done frames")
        finished += int((done != NOT_DONE).sum())
        peak = max(peak, float(np.abs(p_out).max()))
    assert peak > 1e-4 and finished > 0
    plain.close()
    other.close()


@pytest.mark.parametrize("held_last_in_list", [False, True])
def test_all_done_follows_the_envelope_listed_last(knh, held_last_in_list):
    """KNH_FLAG_ALL_DONE on a graph voice with two envelopes whose list order and task order differ (the sum names the one
    listed second as its first operand): the flag follows the envelope LISTED last, as on a chain, whichever runs last.
    An EnvAr that ends after 1.5 ms and an EnvAsr that is held: listed EnvAr, EnvAsr the bank never reports ALL_DONE;
    listed EnvAsr, EnvAr it does once the EnvAr has stopped, the held EnvAsr still sounding."""
    n, bs = 65, 64
    p = configs.voice_parameters(n)
    ar, asr = Stage(L.STAGE_MUL_ENV_AR, input=1), Stage(L.STAGE_MUL_ENV_ASR, input=1)
    envs = [ar, asr] if held_last_in_list else [asr, ar]
    st = [Stage(L.STAGE_SIN_WT)] + envs + [Stage(L.STAGE_MATH_ADD, input=3, input2=2)]
    in_list, in_task = gv.envelope_orders(st)
    assert in_list == [1, 2] and in_task == [2, 1]
    w = configs.Workload("gv_all_done", st, n, bs, L.F32, 1)
    w.ctor = {0: p["freq"].reshape(n, 1), 1: np.tile([0.0005, 0.001], (n, 1)), 2: np.tile([0.0005, 0.001], (n, 1))}
    g = make_gpu(knh, w, L.MIX_LEFT_FOLD)
    v = np.arange(n, dtype=np.uint32)
    for stage in (1, 2):
        g.param_apply_many(v, stage, 3 if st[stage].kind == L.STAGE_MUL_ENV_ASR else 2, L.VALUE_TRIGGER)
    flags, peaks = [], []
    for b in range(4):  # the EnvAr ends at sample 72, in block 1
        _, voices, f = g.process_block_voices()
        flags.append(f)
        peaks.append(float(np.abs(voices).max(axis=1).min()))
    g.close()
    assert not flags[0] & L.FLAG_ALL_DONE and flags[1] & L.FLAG_ANY_DONE
    assert min(peaks) > 0.1, "the held EnvAsr keeps every voice sounding"
    if held_last_in_list:
        assert not any(f & L.FLAG_ALL_DONE for f in flags)
    else:
        assert all(f & L.FLAG_ALL_DONE for f in flags[2:])


# ---- the second generator path: voices that combine the newer stage kinds, flags and calls ----------------------------------
def expected_form(w):
    """A graph takes the one-wavefront fused form, a plain chain the fused pipeline (kernel_form.hpp plan_forms)."""
    return L.DEBUG_FORM_PIPELINE_FUSED if w.info.chain else L.DEBUG_FORM_WHOLE_CHAIN_FUSED


def check_wavetable_place(w, sig):
    """'g' / 'h' in the initialised bank's signature: its one f32 Wavetable is staged to LDS in the sine table's place -- one
    flagged stage, a one-table entry, f32, no 'W' / 'R' in the voice; 'M' / 'k': gathered from device memory."""
    if not w.wavetables:
        assert not set("gMhk") & set(sig.split("#")[0].replace("@", " ")), sig
        return
    chars = [gv.stage_char(s) for s in w.stages]
    staged = w.wavetables[1] == ["one"] and w.sample_type == L.F32 and not set("WR") & set(chars) and sum(c in "Mk" for c in chars) == 1
    assert staged == (w.info.wt_variant == "lds")
    body = [m.group(1) for m in re.finditer(r"(.)(?:%\d+)?@", sig)] if "@" in sig else list(sig)
    assert (("g" in body) or ("h" in body)) == staged, sig
    assert (("M" in body) or ("k" in body)) == (not staged), sig


@pytest.mark.parametrize("seed", range(gv.N_SEEDS))
def test_random_head_voice_matches_the_oracle(knh, seed):
    """Nine blocks in KNH_MIX_LEFT_FOLD against the lowered oracle (gv.lower_for_oracle), bit for bit: every voice's signal
    (both planes with connected outputs), the left-fold mix, the done frames, ANY_DONE.  Readers are given other Buffers in
    front of blocks 3 and 7; in front of block 6 every third voice is restarted and continues against a freshly built oracle
    bank, the others against the first one."""
    w = gv.random_voice_head(seed)
    ref = w.reference
    g = gv.head_gpu_bank(knh, w, L.MIX_LEFT_FOLD)
    sig = g.debug_signature()
    what = f"head seed {seed} {sig}"
    check_wavetable_place(w, sig)
    form = int(g.debug_words()[2])
    print(f"head seed {seed}: form {form} n {w.n_voices} bs {w.block_size} {'f64' if w.sample_type == L.F64 else 'f32'} {sorted(w.info.features)}")
    assert form == expected_form(w), what  # (a silent change of form would empty the test)
    for b in range(gv.HEAD_BLOCKS):
        gv.head_edits(w, b, g)
        g_out, g_voices, g_flags = g.process_block_voices()
        assert_bit_equal(g_voices, ref.voices[b], f"{what} block {b} per-voice")
        assert_bit_equal(g_out, ref.mix[b], f"{what} block {b} left-fold mix")
        np.testing.assert_array_equal(g.read_done_frames(), ref.done[b], err_msg=f"{what} block {b} done frames")
        assert g_flags & L.FLAG_ANY_DONE == int(ref.flags[b]) & L.FLAG_ANY_DONE, f"{what} block {b} ANY_DONE"
    g.close()


WAYS = ("split", "one_launch", "host_threads", "devices", "rank", "resident")
WAY_BLOCKS = 6  # (the restart, in front of block 6, is the first test's)


class _AtBlock:
    """parameter calls for block `offset` of the coming launch (knh_bank_param_apply_many_at)"""

    def __init__(self, bank, offset):
        self.bank, self.offset = bank, offset

    def param_apply_many(self, voices, stages, params, kinds, fvalues=None, ivalues=None, delays=None):
        self.bank.param_apply_many(voices, stages, params, kinds, fvalues, ivalues, delays, block_offset=self.offset)


@pytest.mark.parametrize("seed", range(gv.N_SEEDS))
def test_head_voice_runs_the_same_every_way(knh, monkeypatch, seed):
    """The seed's voice in KNH_MIX_TREE, run one other way (seed % 6) beside a plain bank, six blocks with the reassignment in
    front of block 3: each block as 40 + rest frames (17 + rest at block size 48); the blocks in one process_blocks per
    stretch between graph edits; on two host threads; as two voice ranges on one device; as one rank's share; resident.
    Per-voice rows bit for bit, signs of zero included, where the way hands them out; the mix bit for bit for the split, the
    single launch and the resident call, and within 1e-5 * max(1, peak) -- what tests/test_gpu_multi.py holds re-associated
    tree mixes to -- for the three forms that cut the bank into voice ranges."""
    w = gv.random_voice_head(seed)
    way = WAYS[seed % len(WAYS)]
    bs = w.block_size
    monkeypatch.setenv("KNH_RESIDENT", "0")
    plain = gv.head_gpu_bank(knh, w, L.MIX_TREE)
    monkeypatch.setenv("KNH_RESIDENT", "1" if way == "resident" else "0")
    kw = {"host_threads": dict(host_threads=2), "devices": dict(devices=[0, 0]), "rank": dict(rank=0, world=1)}.get(way, {})
    other = gv.head_gpu_bank(knh, w, L.MIX_TREE, **kw)
    what = f"head seed {seed} {way}"
    want_mix, want_voices, want_done = [], [], []
    for b in range(WAY_BLOCKS):
        gv.head_edits(w, b, plain, restart=False)
        out, voices, _ = plain.process_block_voices()
        want_mix.append(out)
        want_voices.append(voices)
        want_done.append(plain.read_done_frames())
    assert max(float(np.abs(m).max()) for m in want_mix) > 1e-4
    if way == "one_launch":
        cuts = sorted({0, WAY_BLOCKS} | {b for b in w.reassign if b < WAY_BLOCKS})
        for lo, hi in zip(cuts, cuts[1:]):
            if lo in w.reassign:
                voices, ids, rows = w.reassign[lo]
                other.assign_buffers(w.pool[0], voices, ids, ctor=rows)
            for b in range(lo, hi):
                w.events(b, _AtBlock(other, b - lo))
            many, _ = other.process_blocks(hi - lo)
            for b in range(lo, hi):
                assert_bit_equal(many[b - lo], want_mix[b], f"{what} block {b} mix", strict_zero=True)
    else:
        for b in range(WAY_BLOCKS):
            gv.head_edits(w, b, other, restart=False)
            if way == "split":
                first = gv.head_split_point(bs)
                out = np.zeros_like(want_mix[b])
                other.process_block(first, 0, out=out)
                other.process_block(bs - first, first, out=out)
                assert_bit_equal(out, want_mix[b], f"{what} block {b} mix", strict_zero=True)
            elif way == "resident":
                out, _ = other.process_block()
                assert_bit_equal(out, want_mix[b], f"{what} block {b} mix", strict_zero=True)
            else:
                if way == "rank":  # (a rank bank gives the mix only)
                    out, _ = other.process_block()
                else:
                    out, voices, _ = other.process_block_voices()
                    assert_bit_equal(voices, want_voices[b], f"{what} block {b} per-voice", strict_zero=True)
                bound = 1e-5 * max(1.0, float(np.abs(want_mix[b]).max()))
                assert np.max(np.abs(out.astype(np.float64) - want_mix[b].astype(np.float64))) <= bound, f"{what} block {b} mix"
            if way != "split":  # (a call that ends inside a block reports frames of its own part)
                np.testing.assert_array_equal(other.read_done_frames(), want_done[b], err_msg=f"{what} block {b} done frames")
    # the way meant is the way run
    if way in ("host_threads", "devices"):
        assert other.ranks() == 2
    elif way == "rank":  # one rank of a world of one: what tells it from a plain bank is that it hands out no per-voice rows
        assert other.ranks() == 1 and plain.ranks() == 1
        with pytest.raises(L.KnasterHipError, match="per-voice output is not available from a sharded bank"):
            other.process_block_voices()
    elif way == "resident":
        assert other.resident_stats()[0] >= 1 and plain.resident_stats()[0] == 0
    plain.close()
    other.close()
