"""Reader voices through the C++ host mirror (knaster_amd/host/knaster_host.hpp): `BufferReader(buffer, rate, looping)` voices
made on different Buffers share a bank, whose pool holds every distinct Buffer once (tests/cpp/host_sampler_test.cpp, built
here with the flags of tests/cpp/Makefile)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CPP, "bin", "host_sampler_test")


@pytest.fixture(scope="module")
def binary(knh):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", BIN,
                    os.path.join(CPP, "host_sampler_test.cpp"), "-L" + os.path.join(ROOT, "knaster_amd", "csrc"), "-lknaster_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "knaster_amd", "csrc")], check=True, capture_output=True)
    return BIN


def test_reader_voices_pool_their_buffers(binary):
    res = subprocess.run([binary, "--create"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "ok   pool accepted" in res.stdout, res.stdout + res.stderr


@pytest.mark.gpu
def test_reader_voices_read_their_own_buffers_on_gpu(binary):
    res = subprocess.run([binary, "--gpu"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "ok   reader voices on their own Buffers" in res.stdout, res.stdout + res.stderr
