"""Feedback edges at the C ABI without a device: the flag in the header and its mirrors, what knh_bank_create accepts and
refuses (status and a message that names the reason), the node count, and the closed-loop oracle of tests/feedback_cases.py
against the reference's own two vectors (graph_tests.rs:185-254)."""
import os
import re

import numpy as np
import pytest

import feedback_cases as fc
from knaster_amd import _lib as L
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = L.STAGE_FLAG_FEEDBACK
SIN, MULC, ADDC = Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST)


def test_flag_in_header_and_mirrors():
    header = open(os.path.join(ROOT, "include", "knaster_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bKNH_STAGE_FLAG_FEEDBACK\s*=\s*1u\s*<<\s*5\b", code)
    assert L.STAGE_FLAG_FEEDBACK == 1 << 5
    ffi = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "ffi.rs")).read()
    assert re.search(r"pub const KNH_STAGE_FLAG_FEEDBACK: u16 = 1 << 5;", ffi)
    shim = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "lib.rs")).read()
    assert "KNH_STAGE_FLAG_FEEDBACK" in shim
    assert int(re.search(r"#define KNH_ABI_VERSION (\d+)", header).group(1)) == 4 == L.KNH_ABI_VERSION
    kinds = re.search(r"KNH_STAGE_KIND_COUNT\s*=\s*(\d+)", code)
    assert kinds is None or int(kinds.group(1)) == 46
    assert L.STAGE_MATH1_EXP == 45  # the last kind: 46 of them


def test_abi_version_and_kind_count(knh):
    assert knh.lib.load().knh_abi_version() == 4
    with pytest.raises(L.KnasterHipError) as e:  # kind 46 does not exist
        knh.VoiceBank([Stage(46)], 1)
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    knh.VoiceBank([SIN, Stage(45)], 1).close()  # kind 45 does


def refused(knh, stages, status, words, **kw):
    with pytest.raises(L.KnasterHipError) as e:
        knh.VoiceBank(stages, 4, **kw)
    assert e.value.status == status, str(e.value)
    text = str(e.value).split(":", 1)[1].strip()
    assert text, "an empty message"
    assert any(w in text for w in words), text
    return text


def test_refusals(knh):
    INV, UNS = L.ERR_INVALID_ARGUMENT, L.ERR_UNSUPPORTED_CHAIN
    # the flag on any other kind, or combined with any other flag
    refused(knh, [SIN, Stage(L.STAGE_MUL_CONST, flags=FB, input=1)], INV, ["only defined for KNH_STAGE_INPUT"])
    refused(knh, [SIN, Stage(L.STAGE_SIN_WT, flags=FB, input=1), Stage(L.STAGE_MATH_ADD, input=1, input2=2)], INV, ["only defined for KNH_STAGE_INPUT"])
    for other in (L.STAGE_FLAG_AR_FREQ, L.STAGE_FLAG_SMOOTH_PARAMS, L.STAGE_FLAG_READER_CH1, L.STAGE_FLAG_WAVETABLE, L.STAGE_FLAG_ENV_SOURCE):
        with pytest.raises(L.KnasterHipError) as e:
            knh.VoiceBank([SIN, MULC, Stage(L.STAGE_INPUT, flags=FB | other, input=2)], 4)
        assert e.value.status == INV and str(e.value).split(":", 1)[1].strip()
    refused(knh, [SIN, MULC, Stage(L.STAGE_INPUT, flags=FB | L.STAGE_FLAG_SMOOTH_PARAMS, input=2)], INV, ["no other stage flag"])
    # input
    refused(knh, [Stage(L.STAGE_INPUT, flags=FB), ADDC], INV, ["input = 1 + its index"])
    refused(knh, [Stage(L.STAGE_INPUT, flags=FB, input=3), ADDC], INV, ["beyond the last stage"])
    refused(knh, [Stage(L.STAGE_INPUT), Stage(L.STAGE_INPUT, flags=FB, input=1), Stage(L.STAGE_MATH_ADD, input=1, input2=2)], INV, ["* 1.0"], in_channels=1)
    refused(knh, [Stage(L.STAGE_INPUT, flags=FB, input=1), ADDC], INV, ["* 1.0"])                       # itself
    refused(knh, [Stage(L.STAGE_INPUT, flags=FB, input=3), ADDC, Stage(L.STAGE_INPUT, flags=FB, input=2)], INV, ["* 1.0"])  # another edge's source
    reader = [Stage(L.STAGE_BUFFER_READER), Stage(L.STAGE_BUFFER_READER, flags=L.STAGE_FLAG_READER_CH1, input=1)]
    refused(knh, reader + [Stage(L.STAGE_INPUT, flags=FB, input=2), Stage(L.STAGE_MATH_ADD, input=1, input2=3)], INV, ["READER_CH1"])
    refused(knh, reader + [Stage(L.STAGE_WR_MUL), Stage(L.STAGE_INPUT, flags=FB, input=3)], UNS, ["wrapper stage on a BufferReader"])  # (refused before: stays refused)
    refused(knh, [Stage(L.STAGE_INPUT, flags=FB, input=3), SIN, Stage(L.STAGE_PAN2)], INV, ["Pan2 or Galactic"])
    refused(knh, [Stage(L.STAGE_INPUT, flags=FB, input=3), SIN, Stage(L.STAGE_GALACTIC)], INV, ["Pan2 or Galactic"])
    # no parameters: ar_param, input2, delayed_changes_per_block
    for bad in (Stage(L.STAGE_INPUT, flags=FB, input=2, ar_param=1, input2=1), Stage(L.STAGE_INPUT, flags=FB, input=2, input2=1),
                Stage(L.STAGE_INPUT, flags=FB, input=2, delayed_changes_per_block=2)):
        refused(knh, [SIN, MULC, bad, Stage(L.STAGE_MATH_ADD, input=2, input2=3)], INV, ["must be 0"])
    # a chain that ends in Galactic
    refused(knh, [SIN, Stage(L.STAGE_INPUT, flags=FB, input=3), Stage(L.STAGE_MATH_ADD, input=1, input2=2), Stage(L.STAGE_GALACTIC)], UNS,
            ["ends in Galactic"])
    # delay stages plus feedback edges above KNH_MAX_DELAY_STAGES
    delays = [SIN] + [Stage(L.STAGE_SAMPLE_DELAY)] * (L.KNH_MAX_DELAY_STAGES - 1)
    two_edges = [Stage(L.STAGE_INPUT, flags=FB, input=2), Stage(L.STAGE_INPUT, flags=FB, input=2)]
    refused(knh, delays + two_edges + [Stage(L.STAGE_MATH_ADD, input=len(delays) + 1, input2=len(delays) + 2)], UNS, ["KNH_MAX_DELAY_STAGES"])
    knh.VoiceBank(delays + two_edges[:1] + [Stage(L.STAGE_MATH_ADD, input=len(delays), input2=len(delays) + 1)], 4).close()  # sixteen in all: fine
    # more than one envelope beside an edge (the header says why)
    refused(knh, [SIN, Stage(L.STAGE_MUL_ENV_ASR), Stage(L.STAGE_MUL_ENV_AR), Stage(L.STAGE_INPUT, flags=FB, input=3),
                  Stage(L.STAGE_MATH_ADD, input=3, input2=4)], UNS, ["at most one envelope"])


def test_what_was_refused_stays_refused(knh):
    INV = L.ERR_INVALID_ARGUMENT
    refused(knh, [SIN, Stage(L.STAGE_MUL_CONST, input=3), MULC], INV, ["earlier stage"])                    # an unflagged stage naming a later one
    refused(knh, [SIN, Stage(L.STAGE_INPUT, input=1), Stage(L.STAGE_MATH_ADD, input=1, input2=2)], INV, ["source stage reads no signal"], in_channels=1)
    refused(knh, [SIN, Stage(L.STAGE_INPUT), Stage(L.STAGE_MUL_CONST, input=1, ar_param=1, input2=2)], INV, ["* 1.0"], in_channels=1)
    refused(knh, [SIN, Stage(L.STAGE_MUL_CONST, flags=1 << 6)], INV, ["unknown stage flag"])


def test_parameter_calls_name_the_chain_before_the_state(knh):
    case = fc.vector_later(4)
    b = knh.VoiceBank(case.stages, 4)
    for call in (lambda: b.param_apply(0, 0, 0, 1.0), lambda: b.set_delay_within_block_for_param(0, 0, 0, 3),
                 lambda: b.param_apply_many([0, 1], 0, 0, L.VALUE_FLOAT, [1.0, 2.0]), lambda: b.param_apply_range(0, 4, 0, 0, L.VALUE_FLOAT, 1.0)):
        with pytest.raises(L.KnasterHipError) as e:
            call()
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "no parameters" in str(e.value), str(e.value)
    with pytest.raises(L.KnasterHipError) as e:  # any other stage: the state comes first
        b.param_apply(0, 1, 0, 1.0)
    assert e.value.status == L.ERR_NOT_INITIALISED
    assert b.stage_parameters(0) == 0 and b.inputs() == 0
    with pytest.raises(L.KnasterHipError):  # no constructor arguments (no channel)
        b.set_ctor_args(0, np.zeros((4, 1)))
    b.close()
    sharded = knh.VoiceBank(fc.Comb(130).stages, 130, host_threads=2)
    with pytest.raises(L.KnasterHipError) as e:
        sharded.param_apply(0, 2, 0, 1.0)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "no parameters" in str(e.value)
    sharded.close()


def test_accepted_shapes_and_node_count(knh):
    later, earlier = fc.vector_later(4), fc.vector_earlier(4)
    comb, fm, crossed = fc.Comb(4), fc.fm(4), fc.crossed(4)
    behind = [Stage(L.STAGE_INPUT, flags=FB, input=2), ADDC]  # the stage right behind it
    for stages, in_ch, nodes in ((later.stages, 0, 6), (earlier.stages, 1, 6), (behind, 0, 4), (comb.stages, 0, 11), (fm.stages, 0, 7),
                                 (crossed.stages, 0, 16)):
        b = knh.VoiceBank(stages, 4, in_channels=in_ch)
        sig = b.debug_signature()
        edges = sum(fc.is_fb(s) for s in stages)
        assert sig.count("x$") == edges and sig.count("y$") == edges, sig  # a read and a write per edge
        for k in range(edges):  # ... the read in front of the write
            assert sig.index(f"x${k}@") < sig.index(f"y${k}@"), sig
        b.close()
        assert knh.chain_ugen_count(stages) == nodes
        assert knh.chain_ugen_count([s for s in stages if not fc.is_fb(s)]) == nodes - 2 * edges  # FeedbackSink + FeedbackSource
    # an edge's source is a node: it may be a connected output, and drive an ar_param directly
    b = knh.VoiceBank(crossed.stages, 4)
    b.connect_outputs(1, 5)
    b.close()
    knh.VoiceBank([Stage(L.STAGE_INPUT, flags=FB, input=2), Stage(L.STAGE_SIN_WT, ar_param=2, input2=1)], 4).close()
    # a 100-stage voice with one loop holds a few live signals, not a hundred
    long = [Stage(L.STAGE_INPUT, flags=FB, input=100), SIN, Stage(L.STAGE_MATH_ADD, input=1, input2=2)] + [MULC] * 97
    b = knh.VoiceBank(long, 4)
    assert int(b.debug_signature().rsplit("#", 1)[1]) <= 3, b.debug_signature()
    b.close()
    # ring traffic: block_size samples read and written per edge, once the block size is known
    b = knh.VoiceBank(later.stages, 4)
    assert b.algorithmic_bytes_per_voice_block() == (8, 0)  # the two constants' words
    b.close()


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_closed_loop_oracle_reproduces_the_reference_vectors(oracle, sample_type):
    bs = 16
    rows, _, _ = fc.expected_blocks(oracle, fc.vector_later(), sample_type, bs, 3)
    for b, want in enumerate(fc.VECTOR_LATER):
        assert np.array_equal(rows[b][2], np.full((1, bs), want)), (b, rows[b][2])
    rows, _, _ = fc.expected_blocks(oracle, fc.vector_earlier(), sample_type, bs, 3, bank_input=np.zeros((1, bs)))
    for b, want in enumerate(fc.VECTOR_EARLIER):
        assert np.array_equal(rows[b][3], np.full((1, bs), want)), (b, rows[b][3])
    # ... and with the edge removed the loop does nothing
    rows, _, _ = fc.expected_blocks(oracle, fc.vector_later(), sample_type, bs, 3, cut_edges=(0,))
    assert all(np.array_equal(r[2], np.full((1, bs), 1.375)) for r in rows)


def test_test_voices_are_alive(oracle):
    """Every voice of the device tests: finite, not silent in its last block, and not what it is with the edges removed."""
    for case, blocks in ((fc.Comb(3), 5), (fc.fm(3), 4), (fc.crossed(3), 4)):
        views = case.outs or ()
        with_edges, _, _ = fc.expected_blocks(oracle, case, L.F32, 64, blocks, views=views)
        without, _, _ = fc.expected_blocks(oracle, case, L.F32, 64, blocks, views=views, cut_edges=range(len(case.edges)))
        last = len(case.stages) - 1
        a = with_edges[-1][last]
        assert np.isfinite(a).all() and np.abs(a).max(axis=1).min() > 0.0, case.name
        # (over the whole run: SinWt's phase_offset saturates at 0, so a block that follows a negative one has no offset)
        whole, cut = (np.concatenate([r[last] for r in rows], axis=1) for rows in (with_edges, without))
        assert (np.abs(whole - cut).max(axis=1) > 0.0).all(), case.name
