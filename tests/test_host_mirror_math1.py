"""The Math1UGen factories of the C++ host mirror (knaster_amd/host/knaster_host.hpp: fract ceil exp trunc floor sqrt, as
knaster/src/math_ugens.rs names them): tests/cpp/host_mirror_math1_test.cpp, compiled here with the flags of tests/cpp/Makefile."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "bin", "host_mirror_math1_test")


@pytest.fixture(scope="module")
def binary(knh):
    os.makedirs(os.path.join(CPP, "bin"), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", BIN,
           os.path.join(CPP, "host_mirror_math1_test.cpp"), "-L" + os.path.join(ROOT, "knaster_amd", "csrc"), "-lknaster_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "knaster_amd", "csrc")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return BIN


def test_math1_nodes_are_traced_into_stages(binary):
    res = subprocess.run([binary, "--plan"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("plan_chain_stays_a_chain", "plan_fan_out_names_its_operands", "plan_a_math1_node_has_no_parameters"):
        assert f"ok   {name}" in res.stdout


@pytest.mark.gpu
def test_traced_banks_render_what_hand_written_descriptors_render(binary):
    res = subprocess.run([binary, "--gpu"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("gpu_chain_equals_descriptor", "gpu_fan_out_equals_descriptor"):
        assert f"ok   {name}" in res.stdout
