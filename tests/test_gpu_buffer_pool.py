"""BufferReader on a pool of Buffers (knh_bank_add_buffer / knh_bank_assign_buffers): every voice plays the entry it was
given, with that entry's length and sample rate, and can be given another one -- a new reader -- while the bank runs.
The expected signal is assembled from one oracle bank per pool entry (sampler_pool.py); per-voice output, both mixes and
the done frames are bit-identical to it in every kernel form a BufferReader chain can take."""
import numpy as np
import pytest

import sampler_pool as sp
from helpers import assert_bit_equal, pairwise_sum
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage
from test_gpu_pan2 import FORMS

pytestmark = pytest.mark.gpu

BOTH = [L.F32, L.F64]


def check_pool_parity(knh, oracle, sample_type, what, **kw):
    """Test 1's scenario on a bank made with **kw: per-voice bit-equal; returns the mixes for the caller to judge."""
    ref = sp.pool_reference(oracle, sample_type)
    buffers = sp.make_buffers(sp.POOL_SPEC)
    g = sp.pooled_bank(knh, sp.POOL_N, sp.POOL_BS, sample_type, buffers, sp.pool_ids(), sp.sampler_ctor(sp.POOL_N), **kw)
    ev = sp.sampler_traffic(sp.POOL_N)
    outs = []
    for b, (voices, done) in enumerate(ref):
        ev(b, g)
        out, g_voices, flags = g.process_block_voices()
        print(f"{what} block {b}: voices differing {int(np.count_nonzero(g_voices != voices))}, done {int(np.count_nonzero(done != sp.NOT_DONE))}")
        assert_bit_equal(g_voices, voices, f"{what} block {b} per-voice")
        np.testing.assert_array_equal(g.read_done_frames(), done)
        assert bool(flags & L.FLAG_ANY_DONE) == bool((done != sp.NOT_DONE).any())
        assert_bit_equal(out[0], out[1], "L == R")
        outs.append(out[0])
    g.close()
    return outs


@pytest.mark.parametrize("sample_type", BOTH)
def test_pool_parity(knh, oracle, sample_type):
    """130 voices on five Buffers of 2 .. 4 099 frames at five sample rates, voice v on entry v % 5, the existing sampler
    test's constructor arguments and parameter traffic: per-voice output, the left-fold mix, the tree mix (served by the
    per-block call, resident where the device allows) and the done frames equal the assembled oracle's."""
    ref = sp.pool_reference(oracle, sample_type)
    assert any((d != sp.NOT_DONE).any() for _, d in ref) and max(float(np.abs(v).max()) for v, _ in ref) > 1e-4
    fold = check_pool_parity(knh, oracle, sample_type, "left fold", mix_mode=L.MIX_LEFT_FOLD)
    tree = check_pool_parity(knh, oracle, sample_type, "tree", mix_mode=L.MIX_TREE)
    for b, (voices, _) in enumerate(ref):
        assert_bit_equal(fold[b], sp.left_fold(voices), f"block {b} left-fold mix")
        assert_bit_equal(tree[b], pairwise_sum(voices), f"block {b} tree mix")
    # ... and the call the reference makes, one knh_bank_process_block per block
    t = sp.pooled_bank(knh, sp.POOL_N, sp.POOL_BS, sample_type, sp.make_buffers(sp.POOL_SPEC), sp.pool_ids(), sp.sampler_ctor(sp.POOL_N))
    ev = sp.sampler_traffic(sp.POOL_N)
    for b, (voices, done) in enumerate(ref):
        ev(b, t)
        out, flags = t.process_block()
        assert_bit_equal(out[0], pairwise_sum(voices), f"per-block call, block {b} tree mix")
        assert bool(flags & L.FLAG_ANY_DONE) == bool((done != sp.NOT_DONE).any())
    np.testing.assert_array_equal(t.read_done_frames(), ref[-1][1])
    t.close()


@pytest.mark.parametrize("sample_type", BOTH)
def test_add_buffer_once_equals_set_buffer(knh, sample_type):
    """A pool of one entry and no assignment call at all: the same bits as knh_bank_set_buffer."""
    n, bs = 100, 64
    (samples, sr), = sp.make_buffers([(3000, 44100.0)])
    banks = []
    for how in ("set", "add"):
        b = knh.VoiceBank(sp.STAGES, n, sample_type, 2, L.MIX_LEFT_FOLD)
        b.set_ctor_args(0, sp.sampler_ctor(n))
        b.set_ctor_args(1, np.full((n, 1), 1.0 / n))
        if how == "set":
            b.set_buffer(0, samples, sr)
        else:
            assert b.add_buffer(0, samples, sr) == 0
        assert b.buffer_count(0) == 1
        b.init(configs.SAMPLE_RATE, bs)
        banks.append(b)
    ev = sp.sampler_traffic(n)
    for blk in range(14):
        res = []
        for b in banks:
            ev(blk, b)
            out, voices, flags = b.process_block_voices()
            res.append((out, voices, flags, b.read_done_frames()))
        assert_bit_equal(res[0][1], res[1][1], f"block {blk} per-voice")
        assert_bit_equal(res[0][0], res[1][0], f"block {blk} mix")
        assert res[0][2] == res[1][2]
        np.testing.assert_array_equal(res[0][3], res[1][3])
    assert np.abs(res[0][1]).max() > 1e-4
    for b in banks:
        b.close()


# ---- reassignment ---------------------------------------------------------------------------------------------------
RE_SPEC = [(3, 22050.0), (64, 44100.0), (3000, 48000.0), (4099, 96000.0)]
RE_N, RE_BS, RE_BLOCKS = 70, 32, 12


def re_ctor0():
    """One-shots on the short entries have finished by block 3, the voices on the long ones are in mid-play, every third loops."""
    return sp.sampler_ctor(RE_N)


def re_swaps():
    """block -> (voices, entries, constructor rows): at block 3 every voice v with v % 3 != 1 (finished one-shots on the 3- and
    64-frame entries, voices in mid-play on the long ones, looping voices), at block 7 every voice with v % 4 < 2."""
    v = np.arange(RE_N, dtype=np.uint32)
    a, b = v[v % 3 != 1], v[v % 4 < 2]
    return {3: (a, ((a + 1) % 4).astype(np.uint32), sp.sampler_ctor(RE_N, 5)[a]),
            7: (b, ((b + 2) % 4).astype(np.uint32), sp.sampler_ctor(RE_N, 9)[b])}


def re_traffic(block, bank, **kw):
    v = np.arange(RE_N, dtype=np.uint32)
    if block == 1:
        bank.param_apply_many(v[::2], 0, 3, L.VALUE_FLOAT, 0.003 + 0.0001 * v[::2], **kw)  # duration_s: forgotten by a swap
    if block == 5:  # on reassigned voices (and others): converts with each voice's own Buffer's rate
        bank.param_apply_many(v, 0, 3, L.VALUE_FLOAT, 0.002 + 0.00015 * v, **kw)
    if block == 6:
        bank.param_apply_many(v[::5], 0, 5, L.VALUE_TRIGGER, **kw)
    if block == 9:
        bank.param_apply_many(v[1::2], 0, 2, L.VALUE_FLOAT, 0.001 + 0.0001 * v[1::2], **kw)  # start_s
        bank.param_apply_many(v, 0, 0, L.VALUE_FLOAT, 0.5 + 0.02 * v, **kw)                   # rate
        bank.param_apply_many(v[1::2], 0, 5, L.VALUE_TRIGGER, **kw)


def re_expected(oracle, sample_type):
    buffers = sp.make_buffers(RE_SPEC, seed=5)
    ids0 = (np.arange(RE_N) % 4).astype(np.uint32)
    x = sp.Expected(oracle, RE_N, RE_BS, sample_type, buffers, ids0, re_ctor0(), re_traffic)
    swaps = re_swaps()
    blocks = []
    for k in range(RE_BLOCKS):
        if k in swaps:
            x.reassign(k, *swaps[k])
        blocks.append(x.step(k))
    x.close()
    return buffers, ids0, blocks


@pytest.mark.parametrize("sample_type", BOTH)
def test_reassignment_is_a_fresh_reader(knh, oracle, sample_type):
    """70 voices, 32-frame blocks, twelve single-block calls: the voices given another entry at blocks 3 and 7 continue as a
    FRESH oracle bank on that entry started at that block; a later duration_s converts with the new Buffer's rate; done
    frames are cleared by the swap and set again when the new reader ends.  Then the same traffic in front of 4-block launches."""
    buffers, ids0, blocks = re_expected(oracle, sample_type)
    swaps = re_swaps()
    before = blocks[2][0]
    a = swaps[3][0]
    # what the swap at block 3 meets: silent (finished) one-shots and sounding voices, among them looping ones
    assert (np.abs(before[a]).max(axis=1) == 0).any() and (np.abs(before[a]).max(axis=1) > 0).any()
    g = sp.pooled_bank(knh, RE_N, RE_BS, sample_type, buffers, ids0, re_ctor0(), mix_mode=L.MIX_LEFT_FOLD)
    seen_done_again = False
    for k, (voices, done) in enumerate(blocks):
        if k in swaps:
            g.assign_buffers(0, *swaps[k])
        re_traffic(k, g)
        out, g_voices, flags = g.process_block_voices()
        print(f"reassign block {k}: voices differing {int(np.count_nonzero(g_voices != voices))}, done {int(np.count_nonzero(done != sp.NOT_DONE))}")
        assert_bit_equal(g_voices, voices, f"block {k} per-voice")
        assert_bit_equal(out[0], sp.left_fold(voices), f"block {k} left-fold mix")
        g_done = g.read_done_frames()
        np.testing.assert_array_equal(g_done, done)
        assert bool(flags & L.FLAG_ANY_DONE) == bool((done != sp.NOT_DONE).any())
        if k > 3:
            seen_done_again = seen_done_again or bool((done[a] != sp.NOT_DONE).any())
    assert seen_done_again
    g.close()

    # the same traffic in front of 4-block launches: blocks 0 .. 2 singly, [3, 7) and [7, 11) as one launch each, block 11
    m = sp.pooled_bank(knh, RE_N, RE_BS, sample_type, buffers, ids0, re_ctor0(), mix_mode=L.MIX_TREE)
    k = 0
    while k < RE_BLOCKS:
        span = 4 if k in swaps else 1
        if k in swaps:
            m.assign_buffers(0, *swaps[k])
        for j in range(span):
            re_traffic(k + j, m, block_offset=j)
        if span == 1:
            out, _ = m.process_block()
            outs = out[None]
        else:
            outs, _ = m.process_blocks(span)
        for j in range(span):
            assert_bit_equal(outs[j][0], pairwise_sum(blocks[k + j][0]), f"launch at block {k}, block {k + j} tree mix")
        # a launch reports, per voice, the last frame marked in it
        want = np.full(RE_N, sp.NOT_DONE, dtype=np.uint32)
        for j in range(span):
            d = blocks[k + j][1]
            want = np.where(d != sp.NOT_DONE, d, want)
        np.testing.assert_array_equal(m.read_done_frames(), want)
        k += span
    m.close()


@pytest.mark.parametrize("sample_type", BOTH)
def test_a_restart_constructs_the_reader_the_voice_has(knh, oracle, sample_type):
    """knh_bank_restart_voices behind a reassignment: the constructor arguments given with knh_bank_assign_buffers are the
    voice's from then on, so every other voice restarted in front of block 5 -- reassigned at block 3 or not -- is a fresh
    reader on the entry it has with the rate, looping and start it has, the oracle bank Expected starts at that block.
    (Found by the graph-voice fuzz, tests/test_gpu_graph_voices.py: the restart built the FIRST reader's rate, looping and
    start on the new Buffer.)"""
    buffers = sp.make_buffers(RE_SPEC, seed=5)
    ids0 = (np.arange(RE_N) % 4).astype(np.uint32)
    x = sp.Expected(oracle, RE_N, RE_BS, sample_type, buffers, ids0, re_ctor0(), re_traffic)
    g = sp.pooled_bank(knh, RE_N, RE_BS, sample_type, buffers, ids0, re_ctor0(), mix_mode=L.MIX_LEFT_FOLD)
    voices3, ids3, rows3 = re_swaps()[3]
    held = re_ctor0().copy()
    again = np.arange(0, RE_N, 2, dtype=np.uint32)
    assert np.isin(again, voices3).any() and (~np.isin(again, voices3)).any()
    for k in range(8):
        if k == 3:
            x.reassign(k, voices3, ids3, rows3)
            g.assign_buffers(0, voices3, ids3, rows3)
            held[voices3] = rows3
        if k == 5:
            assert (held[again] != re_ctor0()[again]).any()
            x.reassign(k, again, x.ids[again].astype(np.uint32), held[again])
            g.restart_voices(again)
        re_traffic(k, g)
        voices, done = x.step(k)
        out, g_voices, _ = g.process_block_voices()
        assert_bit_equal(g_voices, voices, f"block {k} per-voice")
        assert_bit_equal(out[0], sp.left_fold(voices), f"block {k} left-fold mix")
        np.testing.assert_array_equal(g.read_done_frames(), done)
        if k == 5:
            assert (np.abs(voices[again]).max(axis=1) > 0).any()
    x.close()
    g.close()


# ---- every kernel form -------------------------------------------------------------------------------------------------
POOL_FORMS = dict(FORMS)
POOL_FORMS["jitwide4"] = {"KNH_JIT_PIPE": "0", "KNH_JIT_WAVES": "4"}  # whole-chain wavefronts, four to a workgroup


@pytest.mark.parametrize("form", sorted(POOL_FORMS))
def test_pool_parity_in_every_kernel_form(knh, oracle, monkeypatch, form):
    """Test 1's f32 case under each set of environment switches tests/test_gpu_pan2.py selects kernel forms with (a
    BufferReader chain is always fused at run time: what the switches can change is the fused kernel's form), and with the
    fused chain as whole-chain wavefronts sharing a workgroup."""
    for k, val in POOL_FORMS[form].items():
        monkeypatch.setenv(k, val)
    ref = sp.pool_reference(oracle, L.F32)
    fold = check_pool_parity(knh, oracle, L.F32, f"{form} left fold", mix_mode=L.MIX_LEFT_FOLD)
    tree = check_pool_parity(knh, oracle, L.F32, f"{form} tree", mix_mode=L.MIX_TREE)
    for b, (voices, _) in enumerate(ref):
        assert_bit_equal(fold[b], sp.left_fold(voices), f"{form} block {b} left-fold mix")
        assert_bit_equal(tree[b], pairwise_sum(voices), f"{form} block {b} tree mix")


@pytest.mark.parametrize("how", ["host_sharded", "multi_device"])
def test_pool_parity_in_sharded_banks(knh, oracle, how):
    """A 2-thread host-sharded bank and a two-range multi-device bank on device 0 twice: every range holds the whole pool, voice
    numbers are translated to the ranges.  Per-voice output bit-equal; the mix (a sum of per-range tree mixes) within the
    1e-5 of the f64 sum that the sharded banks' own tests hold it to (tests/test_gpu_multi.py)."""
    kw = {"host_threads": 2} if how == "host_sharded" else {"devices": [0, 0]}
    ref = sp.pool_reference(oracle, L.F32)
    outs = check_pool_parity(knh, oracle, L.F32, how, mix_mode=L.MIX_TREE, **kw)
    for b, (voices, _) in enumerate(ref):
        assert np.max(np.abs(outs[b].astype(np.float64) - voices.astype(np.float64).sum(axis=0))) <= 1e-5, f"{how} block {b}"


def test_reassignment_in_sharded_banks(knh, oracle):
    """The reassignment traffic through a host-sharded bank: voice numbers of the whole bank reach the right range."""
    buffers, ids0, blocks = re_expected(oracle, L.F32)
    swaps = re_swaps()
    g = sp.pooled_bank(knh, RE_N, RE_BS, L.F32, buffers, ids0, re_ctor0(), mix_mode=L.MIX_TREE, host_threads=2)
    assert g.ranks() == 2 and g.buffer_count(0) == 4
    for k, (voices, done) in enumerate(blocks):
        if k in swaps:
            g.assign_buffers(0, *swaps[k])
        re_traffic(k, g)
        _, g_voices, _ = g.process_block_voices()
        assert_bit_equal(g_voices, voices, f"block {k} per-voice")
        np.testing.assert_array_equal(g.read_done_frames(), done)
    g.close()


# ---- refusals after init -------------------------------------------------------------------------------------------------
ENV_STAGES = [Stage(L.STAGE_BUFFER_READER), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_MUL_ENV_ASR)]


SMOOTH_STAGES = [Stage(L.STAGE_BUFFER_READER, flags=L.STAGE_FLAG_SMOOTH_PARAMS), Stage(L.STAGE_MUL_CONST)]


@pytest.mark.parametrize("case", ["null_ctor", "bad_buffer", "bad_voice", "add_after_init", "envelope_behind", "smooth_reader"])
def test_refused_calls_after_init_change_nothing(knh, case):
    """A refused call leaves the bank as it was: its output afterwards is bit-equal to a bank that never saw the call."""
    n, bs = 70, 32
    buffers = sp.make_buffers(RE_SPEC, seed=5)
    ids = (np.arange(n) % 4).astype(np.uint32)
    # (smooth_reader: a reader wrapped in WrSmoothParams keeps ramp state on the host that a new node would not have)
    stages = ENV_STAGES if case == "envelope_behind" else SMOOTH_STAGES if case == "smooth_reader" else sp.STAGES
    v = np.arange(n, dtype=np.uint32)
    banks = []
    for _ in range(2):
        b = sp.pooled_bank(knh, n, bs, L.F32, buffers, ids, sp.sampler_ctor(n), mix_mode=L.MIX_LEFT_FOLD, stages=stages)
        if case == "envelope_behind":
            b.param_apply_many(v, 2, 3, L.VALUE_TRIGGER)  # t_restart
        banks.append(b)
    seen, clean = banks
    ctor = sp.sampler_ctor(n, 5)
    for blk in range(6):
        if blk == 2:
            with pytest.raises(L.KnasterHipError) as e:
                if case == "null_ctor":
                    seen.assign_buffers(0, v, (ids + 1) % 4)
                elif case == "bad_buffer":
                    seen.assign_buffers(0, v, np.where(v == n - 1, 4, (ids + 1) % 4), ctor)
                elif case == "bad_voice":
                    seen.assign_buffers(0, np.where(v == n - 1, n, v), (ids + 1) % 4, ctor)
                elif case == "add_after_init":
                    seen.add_buffer(0, buffers[0][0], buffers[0][1])
                else:
                    seen.assign_buffers(0, v, (ids + 1) % 4, ctor)
            want = {"null_ctor": L.ERR_INVALID_ARGUMENT, "bad_buffer": L.ERR_OUT_OF_RANGE, "bad_voice": L.ERR_OUT_OF_RANGE,
                    "add_after_init": L.ERR_INVALID_ARGUMENT, "envelope_behind": L.ERR_UNSUPPORTED_CHAIN,
                    "smooth_reader": L.ERR_UNSUPPORTED_CHAIN}[case]
            assert e.value.status == want and str(e.value)
            assert seen.buffer_count(0) == 4
        if blk == 3:  # a seconds-valued parameter still converts with the rates the voices had
            for b in banks:
                b.param_apply_many(v, 0, 3, L.VALUE_FLOAT, 0.002 + 0.0001 * v)
                b.param_apply_many(v, 0, 5, L.VALUE_TRIGGER)
        a_out, a_voices, a_flags = seen.process_block_voices()
        b_out, b_voices, b_flags = clean.process_block_voices()
        assert_bit_equal(a_voices, b_voices, f"{case} block {blk} per-voice")
        assert_bit_equal(a_out, b_out, f"{case} block {blk} mix")
        assert a_flags == b_flags
        np.testing.assert_array_equal(seen.read_done_frames(), clean.read_done_frames())
    assert np.abs(a_voices).max() > 0
    for b in banks:
        b.close()


def test_init_without_a_pool_is_refused_as_before(knh):
    b = knh.VoiceBank(sp.STAGES, 4)
    with pytest.raises(L.KnasterHipError) as e:
        b.init(configs.SAMPLE_RATE, 32)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "BufferReader" in str(e.value)
    b.close()


def test_reassignment_in_a_two_rank_bank(knh, oracle):
    """Rank 0 and rank 1 of a two-rank bank in this process (a reduce function that leaves the buffers alone): every rank is
    handed the whole pool and the whole bank's voice numbers, renders its own range, and reports its own done frames."""
    buffers, ids0, blocks = re_expected(oracle, L.F32)
    swaps = re_swaps()

    def no_reduce(_user, buf, count, sample_type, root, stream):
        return 0
    ranks = [sp.pooled_bank(knh, RE_N, RE_BS, L.F32, buffers, ids0, re_ctor0(), mix_mode=L.MIX_TREE, rank=r, world=2, reduce_fn=no_reduce)
             for r in range(2)]
    ranges = [knh.shard_voice_range(RE_N, r, 2) for r in range(2)]
    assert all(cnt > 0 for _, cnt in ranges) and all(b.buffer_count(0) == 4 for b in ranks)
    for k, (voices, done) in enumerate(blocks):
        outs = []
        for r, b in enumerate(ranks):
            if k in swaps:
                b.assign_buffers(0, *swaps[k])
            re_traffic(k, b)
            out, _ = b.process_block()
            outs.append(out[0].astype(np.float64))
            lo, cnt = ranges[r]
            want = np.full(RE_N, sp.NOT_DONE, dtype=np.uint32)
            want[lo:lo + cnt] = done[lo:lo + cnt]
            np.testing.assert_array_equal(b.read_done_frames(), want)
            assert np.max(np.abs(outs[r] - voices[lo:lo + cnt].astype(np.float64).sum(axis=0))) <= 1e-5, f"rank {r} block {k}"
    with pytest.raises(L.KnasterHipError) as e:
        ranks[0].assign_buffers(0, [RE_N], [0], [[1.0, 0.0, 0.0]])
    assert e.value.status == L.ERR_OUT_OF_RANGE
    for b in ranks:
        b.close()
