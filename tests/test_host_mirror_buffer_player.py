"""knaster/examples/buffer_player.rs through the C++ host mirror (knaster_amd/host/knaster_host.hpp): a two-channel Buffer, a
BufferReader whose handle has two channels, `play * amp.out({0, 0})`, `.to_graph_out()`, parameters on `play`:
tests/cpp/host_mirror_buffer_player_test.cpp, compiled here with the flags of tests/cpp/Makefile."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "bin", "host_mirror_buffer_player_test")


@pytest.fixture(scope="module")
def binary(knh):
    os.makedirs(os.path.join(CPP, "bin"), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", BIN,
           os.path.join(CPP, "host_mirror_buffer_player_test.cpp"), "-L" + os.path.join(ROOT, "knaster_amd", "csrc"), "-lknaster_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "knaster_amd", "csrc")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return BIN


def test_the_examples_graph_calls_trace_into_one_connected_voice(binary):
    res = subprocess.run([binary, "--plan"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("plan_the_example_is_one_connected_voice", "plan_parameter_names_are_the_readers",
                 "plan_a_one_channel_buffer_stays_the_mono_reader"):
        assert f"ok   {name}" in res.stdout


@pytest.mark.gpu
def test_the_traced_bank_renders_what_the_descriptor_bank_renders(binary):
    res = subprocess.run([binary, "--gpu"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ok   gpu_the_example_renders_what_the_descriptor_renders" in res.stdout
