"""Audio-rate links on PolyBlep, RandomLin, BufferReader and the segment Envelope, as far as they go without a
device: the descriptor is accepted, the signature names the linked stage ("%P"), and the kernel that knh_bank_init would fuse
compiles for gfx950 -- each compile in a process of its own (tests/cpp/bin/jit_compile_check, as tests/test_jit_compile.py).
What stays refused is refused with the status and a message that says why."""
import os
import subprocess

import pytest

import ar_sources
from knaster_amd import _lib as L
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "bin", "jit_compile_check")

# the linked stage as the signature spells it: kind character, "%" + the parameter's index
LINKED = {"polyblep_freq": "B%0", "polyblep_pulse_width": "B%1", "random_lin_freq": "G%0",
          "reader_rate": "F%0", "envelope_time_scale": "V%0"}


@pytest.fixture(scope="module")
def jit_compile_check(knh):
    """built by __graft_entry__.build(); a tree without it (the library built alone) gets it here, as in tests/test_jit_compile.py"""
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/jit_compile_check"], check=True, capture_output=True)
    assert os.path.exists(CHECK)


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
@pytest.mark.parametrize("case", ar_sources.LINKS)
def test_link_is_accepted_named_and_compiles(knh, jit_compile_check, case, sample_type):
    w = ar_sources.workload(case, 3, sample_type)
    b = knh.VoiceBank(w.stages, w.n_voices, w.sample_type, w.out_channels, L.MIX_LEFT_FOLD)
    sig = b.debug_signature()
    b.close()
    assert sig.count("%") == 1 and LINKED[case] + "@" in sig, sig
    p = subprocess.run([CHECK, sig] + (["f64"] if sample_type == L.F64 else []), cwd="/tmp", stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, f"{sig}: rc {p.returncode}: {p.stdout.decode(errors='replace')[-600:]}"


def refused(knh, stages):
    with pytest.raises(L.KnasterHipError) as e:
        knh.VoiceBank(stages, 4, L.F32, 1)
    assert str(e.value).strip(), "a refusal says why"
    return e.value.status


DRV = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST)]  # the driver: stage 2's output


@pytest.mark.parametrize("kind,param,what", [(L.STAGE_POLYBLEP, 2, "waveform"), (L.STAGE_BUFFER_READER, 1, "looping"),
                                             (L.STAGE_BUFFER_READER, 5, "t_restart"), (L.STAGE_MUL_ENVELOPE, 1, "jump_to_segment"),
                                             (L.STAGE_MUL_ENVELOPE, 2, "t_restart")])
def test_only_float_parameters_can_be_linked(knh, kind, param, what):
    src = [Stage(L.STAGE_SIN_WT)] if kind == L.STAGE_MUL_ENVELOPE else []
    assert refused(knh, DRV + src + [Stage(kind, ar_param=param + 1, input2=2)]) == L.ERR_INVALID_ARGUMENT, what


@pytest.mark.parametrize("kind", [L.STAGE_SAMPLE_DELAY, L.STAGE_ALLPASS_DELAY, L.STAGE_ALLPASS_FB_DELAY])
def test_delay_time_is_still_refused(knh, kind):
    assert refused(knh, DRV + [Stage(L.STAGE_SIN_WT), Stage(kind, ar_param=1, input2=2)]) == L.ERR_UNSUPPORTED_CHAIN


def test_phasor_freq_is_still_refused(knh):
    """(tests/test_gpu_ar_params.py::test_audio_rate_parameter_rules holds Phasor.freq to a refusal)"""
    assert refused(knh, DRV + [Stage(L.STAGE_PHASOR, ar_param=1, input2=2)]) == L.ERR_UNSUPPORTED_CHAIN


@pytest.mark.parametrize("case", ar_sources.LINKS)
def test_link_and_smooth_params_exclude_each_other(knh, case):
    w = ar_sources.workload(case, 4, L.F32)
    x = w.stages[w.linked]
    st = list(w.stages)
    st[w.linked] = Stage(x.kind, L.STAGE_FLAG_SMOOTH_PARAMS, 0, x.input, x.input2, x.ar_param)
    assert refused(knh, st) == L.ERR_INVALID_ARGUMENT
