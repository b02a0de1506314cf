"""The Galactic reverb in the C++ host mirror (knaster_amd/host/knaster_host.hpp: `voice.out({0, 0}) >> g.push(Galactic(..))`
and `(l | r) >> g.push(Galactic(..))`): tests/cpp/host_mirror_galactic_test.cpp, compiled here with the flags of
tests/cpp/Makefile."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "bin", "host_mirror_galactic_test")


@pytest.fixture(scope="module")
def binary(knh):
    os.makedirs(os.path.join(CPP, "bin"), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", BIN,
           os.path.join(CPP, "host_mirror_galactic_test.cpp"), "-L" + os.path.join(ROOT, "knaster_amd", "csrc"), "-lknaster_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "knaster_amd", "csrc")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return BIN


def test_both_spellings_are_traced_and_what_is_no_such_voice_is_refused(binary):
    res = subprocess.run([binary, "--plan"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("plan_the_mono_spelling_is_the_mono_chain", "plan_stacked_signals_are_input_and_input2",
                 "plan_a_shared_node_is_traced_once", "plan_the_reverb_has_its_parameters",
                 "plan_what_is_not_such_a_voice_is_refused"):
        assert f"ok   {name}" in res.stdout


@pytest.mark.gpu
def test_traced_reverb_banks_render_what_the_descriptors_render(binary):
    res = subprocess.run([binary, "--gpu"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("gpu_mono_equals_descriptor", "gpu_stereo_equals_descriptor"):
        assert f"ok   {name}" in res.stdout
