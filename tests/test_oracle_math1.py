"""The oracle's Math1UGen (oracle/knaster_oracle.hpp, restated from knaster_core_dsp/src/ugens/math.rs:167-305) against numpy,
without a GPU: ceil, sqrt, floor, trunc and fract are correctly rounded IEEE operations on both sides, so [INPUT, MATH1_x] is
numpy's function of the input bit for bit, the sign of a zero included, in f32 and f64 -- on the edge list the device test
uses (tests/test_gpu_math1.py::special_inputs: zeros of both signs, the ends of the subnormal range, the last odd half below
2^23 / 2^52, infinities, a NaN).  exp is refused: it is not the same bits in every math library."""
import numpy as np
import pytest

from helpers import make_oracle
from knaster_amd import _lib as L
from knaster_amd.bank import Stage
from test_gpu_math1 import EXACT, MATH1, assert_bits_or_nan, dtype_of, numpy_op, special_inputs, workload


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
@pytest.mark.parametrize("name", EXACT)
def test_oracle_math1_is_numpys_function(oracle, name, sample_type):
    x = special_inputs(sample_type)
    inputs = np.stack([np.roll(x, 5 * b) for b in range(3)])
    n = 3
    o = make_oracle(oracle, workload(name, [Stage(L.STAGE_INPUT), Stage(MATH1[name])], n, sample_type, {0: np.zeros(n)}, 1))
    for b in range(3):
        o.set_input(inputs[b].reshape(1, -1))
        mix, voices, _, _ = o.process_block()
        assert voices.dtype == dtype_of(sample_type)
        want = numpy_op(name, inputs[b])
        for v in range(n):
            assert_bits_or_nan(voices[v], want, f"{name} block {b} voice {v}")
    o.close()


def test_oracle_math1_behind_a_node(oracle):
    """SinWt -> * 3 -> floor: the Math1 node reads another node's output, not a graph input."""
    n = 2
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_MATH1_FLOOR)]
    ctor = {0: np.array([440.0, 1234.5]), 1: np.full(n, 3.0)}
    head = make_oracle(oracle, workload("head", st[:2], n, L.F32, ctor))
    full = make_oracle(oracle, workload("full", st, n, L.F32, ctor))
    for _ in range(2):
        arg, got = head.process_block()[1], full.process_block()[1]
        assert_bits_or_nan(got, np.floor(arg), "floor(3 sin)")
        assert len(np.unique(got)) >= 4
    head.close()
    full.close()


def test_oracle_refuses_exp(oracle):
    o = oracle.OracleBank([Stage(L.STAGE_INPUT), Stage(L.STAGE_MATH1_EXP)], 1, L.F32, 1, True, True)
    o.set_in_channels(1)
    with pytest.raises(RuntimeError, match="MATH1_EXP"):
        o.init(48000, 64)
    o.close()
