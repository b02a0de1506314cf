"""Envelopes as signals in the C++ host mirror (knaster_amd/host/knaster_host.hpp): an envelope node that is not just the
operand of a `*` is traced into an ENV_SOURCE stage with its wrappers behind it, and a plain `signal * env` is still one
MUL_ENV_* stage.  tests/cpp/host_mirror_env_source_test.cpp, compiled here with the flags of tests/cpp/Makefile."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "bin", "host_mirror_env_source_test")


@pytest.fixture(scope="module")
def binary(knh):
    os.makedirs(os.path.join(CPP, "bin"), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", BIN,
           os.path.join(CPP, "host_mirror_env_source_test.cpp"), "-L" + os.path.join(ROOT, "knaster_amd", "csrc"), "-lknaster_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "knaster_amd", "csrc")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return BIN


def test_envelope_nodes_are_traced_into_stages(binary):
    res = subprocess.run([binary, "--plan"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("plan_filter_envelope_is_a_source_with_its_wrappers", "plan_wrapped_envelope_inside_a_product",
                 "plan_envelope_read_by_a_product_and_a_link", "plan_envelope_on_the_graph_output_and_under_plus",
                 "plan_signal_times_envelope_is_still_one_stage"):
        assert f"ok   {name}" in res.stdout


@pytest.mark.gpu
def test_traced_filter_envelope_bank_renders_what_the_descriptor_renders(binary):
    res = subprocess.run([binary, "--gpu"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ok   gpu_filter_envelope_equals_descriptor" in res.stdout
