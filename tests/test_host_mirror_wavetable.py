"""The Wavetable value type and the OscWt node of the C++ host mirror (knaster_amd/host/knaster_host.hpp; the reference's
builders, dsp/wavetable.rs:396-610): tests/cpp/host_mirror_wavetable_test.cpp, compiled here with the flags of tests/cpp/Makefile."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "bin", "host_mirror_wavetable_test")


@pytest.fixture(scope="module")
def binary(knh):
    os.makedirs(os.path.join(CPP, "bin"), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", BIN,
           os.path.join(CPP, "host_mirror_wavetable_test.cpp"), "-L" + os.path.join(ROOT, "knaster_amd", "csrc"), "-lknaster_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "knaster_amd", "csrc")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return BIN


def test_wavetable_builders_and_the_traced_node(binary):
    res = subprocess.run([binary, "--plan"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("cpu_add_sine_fills_the_tables_within_the_harmonic_limit", "cpu_from_buffer_gives_seventeen_equal_tables",
                 "cpu_saw_multiply_normalize", "plan_an_osc_wt_is_a_flagged_sin_wt"):
        assert f"ok   {name}" in res.stdout


@pytest.mark.gpu
def test_osc_wt_through_the_mirror_renders_the_c_abi_banks_blocks(binary):
    res = subprocess.run([binary, "--gpu"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ok   gpu_osc_wt_equals_the_c_abi_bank" in res.stdout
