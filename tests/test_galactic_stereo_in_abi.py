"""`(l | r) >> Galactic` at the C-ABI boundary, on a machine without a GPU (knh_bank_create touches no device):
KNH_STAGE_GALACTIC with `input = l + 1` and `input2 = r + 1` is accepted -- two oscillators, one stage on both inputs, the stereo
sampler -- and reports the reverb's outputs, parameters and constructor arguments; every refusal keeps its status; no stage
kind, flag value or ABI version moved; G2, the workload with a stereo input, is G1's reverb behind two voices' worth of
source."""
import os
import re

import numpy as np
import pytest

import stereo_reader_ref as srr
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIN, MUL = Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST)
GAL_PARAMS = ["replace", "detune", "brightness", "bigness", "wet"]


def gal(**kw):
    return Stage(L.STAGE_GALACTIC, **kw)


TWO_OSC = [SIN, MUL, SIN, MUL, gal(input=2, input2=4)]
SAME = [SIN, MUL, SIN, MUL, gal(input=2, input2=2)]
SAMPLER = srr.STEREO + [gal(input=3, input2=4)]
ACCEPTED = {"two oscillators": TWO_OSC, "input == input2": SAME, "stereo sampler": SAMPLER}


def refused(knh, stages, status, out_channels=2, **kw):
    with pytest.raises(L.KnasterHipError) as e:
        knh.VoiceBank(stages, 4, L.F32, out_channels, **kw)
    assert e.value.status == status, str(e.value)
    text = str(e.value).split(":", 1)[1].strip()
    assert text  # a knh_last_error text
    return text


@pytest.mark.parametrize("mix", [L.MIX_TREE, L.MIX_LEFT_FOLD])
@pytest.mark.parametrize("st", [L.F32, L.F64])
@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_accepted(knh, name, st, mix):
    stages = ACCEPTED[name]
    g = len(stages) - 1
    b = knh.VoiceBank(stages, 5, st, 2, mix)
    assert b.outputs() == 2
    assert b.stage_param_descriptions(g) == GAL_PARAMS
    b.set_ctor_args(g, np.tile([0.5, 0.0, 0.5, 0.5, 0.5, 17.0, 19.0], (5, 1)))  # Galactic::new's five and the two seeds
    with pytest.raises(L.KnasterHipError) as e:
        b.set_ctor_args(g, np.zeros((5, 6)))
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    # the stages in front keep their own: parameters, constructor arguments
    assert b.stage_param_descriptions(0)[0] == ("rate" if name == "stereo sampler" else "freq")
    assert (b.output_stage(0), b.output_stage(1)) == (g, g)  # the reverb makes both outputs
    b.close()


def test_the_signature_is_that_of_the_stage_list_connected_by_hand(knh):
    """The chain before the reverb is the voice knh_bank_connect_outputs makes of it: the same signature, so the same
    fused kernel and the same JIT cache entry; naming the last stage twice is the mono form."""
    for stages, outs in ((TWO_OSC, (1, 3)), (SAME, (1, 1)), (SAMPLER, (2, 3)),
                         ([SIN, Stage(L.STAGE_WR_MUL), SIN, MUL, gal(input=1, input2=3)], (0, 2))):  # the node's output: behind its wrapper
        b = knh.VoiceBank(stages, 70, L.F32, 2)
        hand = knh.VoiceBank(stages[:-1], 70, L.F32, 2)
        hand.connect_outputs(*outs)
        assert re.fullmatch(r".*#\d+:\d+,\d+", hand.debug_signature())
        assert b.debug_signature() == hand.debug_signature()
        b.close()
        hand.close()
    mono = knh.VoiceBank([SIN, MUL, SIN, MUL, gal()], 70, L.F32, 2)
    for same in (gal(input=4, input2=4), gal(input=4)):  # the stage before the reverb, named
        b = knh.VoiceBank([SIN, MUL, SIN, MUL, same], 70, L.F32, 2)
        assert b.debug_signature() == mono.debug_signature()
        b.close()
    wrapped = knh.VoiceBank([SIN, MUL, SIN, Stage(L.STAGE_WR_MUL), gal(input=3, input2=4)], 70, L.F32, 2)  # both name the last node
    wmono = knh.VoiceBank([SIN, MUL, SIN, Stage(L.STAGE_WR_MUL), gal()], 70, L.F32, 2)
    assert wrapped.debug_signature() == wmono.debug_signature()
    wrapped.close()
    wmono.close()
    mono.close()


def test_what_was_refused_stays_refused_with_its_status(knh):
    inv = L.ERR_INVALID_ARGUMENT
    refused(knh, [SIN, MUL, SIN, MUL, gal(input=2)], inv)                          # input alone, not the stage before
    refused(knh, [SIN, MUL, SIN, MUL, gal(input=2, input2=4, ar_param=1)], inv)    # ar_param
    refused(knh, [SIN, MUL, SIN, MUL, gal(ar_param=1)], inv)
    for flag in (L.STAGE_FLAG_AR_FREQ, L.STAGE_FLAG_SMOOTH_PARAMS, L.STAGE_FLAG_READER_CH1):
        refused(knh, [SIN, MUL, SIN, MUL, gal(input=2, input2=4, flags=flag)], inv)
    refused(knh, [SIN, MUL, SIN, MUL, gal(input=2, input2=4, delayed_changes_per_block=2)], inv)
    refused(knh, [SIN, MUL, SIN, gal(input=2, input2=3), MUL], inv)                # not last
    refused(knh, TWO_OSC, inv, out_channels=1)
    for delay in (L.STAGE_SAMPLE_DELAY, L.STAGE_ALLPASS_DELAY, L.STAGE_ALLPASS_FB_DELAY):
        refused(knh, [SIN, Stage(delay), SIN, MUL, gal(input=2, input2=4)], inv)   # a delay stage anywhere in the chain
        refused(knh, [SIN, MUL, SIN, Stage(delay), gal(input=2, input2=4)], inv)
    refused(knh, [SIN, MUL, SIN, MUL, gal(input=6, input2=2)], inv)                # a forward reference
    refused(knh, [SIN, MUL, SIN, MUL, gal(input=2, input2=5)], inv)                # ... to itself
    # one voice range on one device
    for kw in ({"devices": [0]}, {"rank": 0, "world": 1}):
        refused(knh, TWO_OSC, L.ERR_UNSUPPORTED_CHAIN, **kw)


def test_new_refusals(knh):
    inv = L.ERR_INVALID_ARGUMENT
    assert "input2" in refused(knh, [SIN, MUL, SIN, MUL, gal(input2=4)], inv)      # input2 alone
    inp = Stage(L.STAGE_INPUT)
    for stages in ([inp, MUL, SIN, MUL, gal(input=1, input2=4)], [SIN, MUL, inp, MUL, gal(input=2, input2=3)],
                   [SIN, inp, gal(input=2, input2=2)]):
        assert "* 1.0" in refused(knh, stages, inv, in_channels=1)                  # the text output connections use
    ok = knh.VoiceBank([inp, MUL, SIN, MUL, gal(input=2, input2=4)], 4, L.F32, 2, in_channels=1)  # through `* value`: a node
    ok.close()
    # the rule for input2 names its three cases
    assert "Galactic" in refused(knh, [SIN, MUL, Stage(L.STAGE_SVF, input2=1)], inv)


def test_connect_outputs_is_refused(knh):
    for stages in ACCEPTED.values():
        b = knh.VoiceBank(stages, 4, L.F32, 2)
        sig = b.debug_signature()
        with pytest.raises(L.KnasterHipError) as e:
            b.connect_outputs(0, 1)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "Galactic" in str(e.value)
        assert b.debug_signature() == sig
        b.close()


def test_restart_stays_refused(knh):
    b = knh.VoiceBank(TWO_OSC, 4, L.F32, 2)
    with pytest.raises(L.KnasterHipError) as e:
        b.restart_voices(np.arange(2, dtype=np.uint32))
    assert e.value.status in (L.ERR_NOT_INITIALISED, L.ERR_UNSUPPORTED_CHAIN)
    b.close()


def test_ugen_count_and_algorithmic_bytes(knh):
    import knaster_amd
    assert knaster_amd.chain_ugen_count(TWO_OSC) == knaster_amd.chain_ugen_count(TWO_OSC[:-1]) + 1
    stereo = knh.VoiceBank(TWO_OSC, 4, L.F32, 2)
    mono = knh.VoiceBank(TWO_OSC[:-1] + [gal()], 4, L.F32, 2)
    # before init the block size is not known: the second staging plane counts block_size samples written and read after it
    assert stereo.algorithmic_bytes_per_voice_block() == mono.algorithmic_bytes_per_voice_block()
    stereo.close()
    mono.close()


def test_header_and_rust_bindings():
    header = open(os.path.join(ROOT, "include", "knaster_hip.h")).read()
    assert re.search(r"KNH_STAGE_KIND_COUNT = 46\b", header)
    assert re.search(r"#define KNH_ABI_VERSION 4\b", header)
    assert re.search(r"KNH_STAGE_GALACTIC = 39,", header)
    assert re.search(r"KNH_STAGE_FLAG_READER_CH1 = 1u << 2\b", header)
    entry = header[header.index(" * KNH_STAGE_GALACTIC "):header.index(" * KNH_STAGE_PAN2 ")]
    for words in ("input = l + 1", "input2 = r + 1", "(l | r) >>", "KNH_STAGE_FLAG_READER_CH1", "KNH_STAGE_INPUT", "l == r"):
        assert words in entry, words
    desc = header[header.index("Which signal the stage reads."):header.index("} knh_stage_desc;")]
    assert "KNH_STAGE_GALACTIC" in desc
    ffi = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "ffi.rs")).read()
    assert re.search(r"pub const KNH_ABI_VERSION: u32 = 4;", ffi)
    assert re.search(r"pub const KNH_STAGE_KIND_COUNT: u16 = 46;", ffi)
    assert re.search(r"pub const KNH_STAGE_GALACTIC: u16 = 39;", ffi)
    lib = open(os.path.join(ROOT, "bindings", "rust", "knaster_hip", "src", "lib.rs")).read()
    m = re.search(r"pub fn galactic_stereo\(l: u16, r: u16, [^)]*\) -> \(Stage, \[f64; 7\]\) \{(.*?)\n\}", lib, re.S)
    assert m and "s.input = l + 1;" in m.group(1) and "s.input2 = r + 1;" in m.group(1)
    assert L.KNH_ABI_VERSION == 4


def test_workload_g2(knh):
    """G2: two SinWt.wr_mul(0.25), 7 cents apart, each through an EnvAr, on Galactic's left and right; G1's reverb."""
    g1, g2 = configs.config("G1", n_voices=64), configs.config("G2", n_voices=64)
    assert (g2.n_voices, g2.block_size, g2.sample_type) == (g1.n_voices, g1.block_size, g1.sample_type)
    assert configs.config("G2").n_voices == configs.config("G1").n_voices == 4096
    kinds = [s.kind for s in g2.stages]
    assert kinds == [L.STAGE_SIN_WT, L.STAGE_WR_MUL, L.STAGE_MUL_ENV_AR] * 2 + [L.STAGE_GALACTIC]
    assert (g2.stages[6].input, g2.stages[6].input2) == (3, 6)
    np.testing.assert_array_equal(g2.ctor[6], g1.ctor[3])  # the reverb's settings and seeds
    np.testing.assert_array_equal(g2.ctor[0], g1.ctor[0])
    cents = 1200.0 * np.log2(g2.ctor[3] / g2.ctor[0])
    assert np.all(cents > 1.0) and np.all(cents < 20.0)
    assert np.all(g2.ctor[1] == 0.25) and np.all(g2.ctor[4] == 0.25)
    assert g2.restart == (2, 2) and g2.restart_more == ((5, 2),)
    b = knh.VoiceBank(g2.stages, g2.n_voices, g2.sample_type, g2.out_channels)
    for s, a in g2.ctor.items():
        b.set_ctor_args(s, a)
    hand = knh.VoiceBank(g2.stages[:-1], g2.n_voices, g2.sample_type, 2)
    hand.connect_outputs(2, 5)
    assert b.debug_signature() == hand.debug_signature()
    b.close()
    hand.close()
