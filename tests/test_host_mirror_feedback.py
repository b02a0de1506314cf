"""Feedback edges in the C++ host mirror (knaster_amd/host/knaster_host.hpp): to_feedback / to_feedback_replace are traced into
the KNH_STAGE_FLAG_FEEDBACK stage (plus the MATH_ADD of the additive form), and the reference's two vectors come out of the
mirror.  tests/cpp/host_mirror_feedback_test.cpp, compiled here with the flags of tests/cpp/Makefile."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "bin", "host_mirror_feedback_test")


@pytest.fixture(scope="module")
def binary(knh):
    os.makedirs(os.path.join(CPP, "bin"), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", BIN,
           os.path.join(CPP, "host_mirror_feedback_test.cpp"), "-L" + os.path.join(ROOT, "knaster_amd", "csrc"), "-lknaster_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "knaster_amd", "csrc")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return BIN


def test_feedback_edges_are_traced_into_stages(binary):
    res = subprocess.run([binary, "--plan"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("plan_replace_is_the_flagged_stage", "plan_additive_is_a_math_add_of_the_two",
                 "plan_additive_onto_an_empty_input_is_the_edge_alone", "plan_a_node_only_the_edge_reads_comes_behind_the_output",
                 "plan_refusals"):
        assert f"ok   {name}" in res.stdout


@pytest.mark.gpu
def test_reference_vectors_through_the_mirror(binary):
    res = subprocess.run([binary, "--gpu"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ok   gpu_reference_vectors" in res.stdout
