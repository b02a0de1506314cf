"""The BufferReader pool at the C ABI on a machine without a GPU (knh_bank_create needs no device): what is refused before
init, the pool indices, knh_bank_buffer_count, the Python wrappers -- and that the oracle, of which the GPU tests assemble
their expected signal, accepts the shortest Buffers they use."""
import ctypes as C

import numpy as np
import pytest

import sampler_pool as sp
from knaster_amd import _lib as L
from knaster_amd.bank import Stage


def status_of(fn, *a, **kw):
    with pytest.raises(L.KnasterHipError) as e:
        fn(*a, **kw)
    assert str(e.value)  # knh_last_error says why
    return e.value.status


def _no_reduce(_user, buf, count, sample_type, root, stream):
    return 0


@pytest.mark.parametrize("kw", [{}, {"host_threads": 2}, {"rank": 1, "world": 2, "reduce_fn": _no_reduce}, {"rank": 3, "world": 256, "reduce_fn": _no_reduce}],
                         ids=["one_range", "host_sharded", "rank_1_of_2", "rank_without_voices"])
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_pool_indices_count_and_refusals_before_init(knh, sample_type, kw):
    n = 130
    b = knh.VoiceBank(sp.STAGES, n, sample_type, 2, L.MIX_TREE, -1, False, **kw)
    assert b.buffer_count(0) == 0 and b.buffer_count(1) == 0 and b.buffer_count(7) == 0
    buffers = sp.make_buffers(sp.POOL_SPEC)
    # nothing to assign to yet
    assert status_of(b.assign_buffers, 0, [0], [0]) == L.ERR_OUT_OF_RANGE
    for k, (s, sr) in enumerate(buffers):
        assert b.add_buffer(0, s, sr) == k  # indices in call order
        assert b.buffer_count(0) == k + 1
    # refused, and nothing changes
    assert status_of(b.add_buffer, 1, buffers[0][0], 48000.0) == L.ERR_INVALID_ARGUMENT      # not a BufferReader stage
    assert status_of(b.add_buffer, 9, buffers[0][0], 48000.0) == L.ERR_INVALID_ARGUMENT      # no such stage
    assert status_of(b.add_buffer, 0, np.zeros(0), 48000.0) == L.ERR_INVALID_ARGUMENT        # empty
    for bad_rate in (0.0, -44100.0, float("nan"), float("inf")):
        assert status_of(b.add_buffer, 0, buffers[0][0], bad_rate) == L.ERR_INVALID_ARGUMENT
    assert status_of(b.assign_buffers, 1, [0], [0]) == L.ERR_INVALID_ARGUMENT                # not a BufferReader stage
    assert status_of(b.assign_buffers, 0, [0, n], [0, 1]) == L.ERR_OUT_OF_RANGE              # voice
    assert status_of(b.assign_buffers, 0, [0, 1], [0, 5]) == L.ERR_OUT_OF_RANGE              # entry
    assert status_of(b.assign_buffers, 0, [0, 1], [0, 5], np.ones((2, 3))) == L.ERR_OUT_OF_RANGE
    assert b.buffer_count(0) == 5
    # accepted: with and without constructor arguments, in any voice order, the same voice twice
    v = np.arange(n, dtype=np.uint32)
    b.assign_buffers(0, v, v % 5)
    b.assign_buffers(0, v[::-1], (v[::-1] + 1) % 5, sp.sampler_ctor(n)[::-1])
    b.assign_buffers(0, [3, 3], [0, 4])
    b.assign_buffers(0, [], [])
    # knh_bank_set_buffer stays, and means entry 0: replaces it, adds nothing
    b.set_buffer(0, buffers[1][0], 32000.0)
    assert b.buffer_count(0) == 5
    b.close()
    # ... or makes it; what it refuses it refuses on every kind of bank (ranks without voices too: the ranks must agree on the indices)
    b = knh.VoiceBank(sp.STAGES, n, sample_type, 2, L.MIX_TREE, -1, False, **kw)
    assert status_of(b.set_buffer, 1, buffers[1][0], 32000.0) == L.ERR_INVALID_ARGUMENT
    assert status_of(b.set_buffer, 0, np.zeros(0), 32000.0) == L.ERR_INVALID_ARGUMENT
    assert status_of(b.set_buffer, 0, buffers[1][0], float("nan")) == L.ERR_INVALID_ARGUMENT
    assert b.buffer_count(0) == 0
    b.set_buffer(0, buffers[1][0], 32000.0)
    assert b.buffer_count(0) == 1
    assert b.add_buffer(0, buffers[2][0], 44100.0) == 1
    b.close()


def test_null_arguments_at_the_c_abi(knh):
    lib = L.load()
    b = knh.VoiceBank(sp.STAGES, 4)
    s = np.ones(8, dtype=np.float32)
    assert lib.knh_bank_add_buffer(b._h, 0, None, 8, 48000.0, None) == L.ERR_INVALID_ARGUMENT  # null samples
    assert lib.knh_bank_add_buffer(b._h, 0, s.ctypes.data_as(C.c_void_p), 8, 48000.0, None) == L.OK  # out_index may be NULL
    assert lib.knh_bank_assign_buffers(b._h, 0, 2, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.knh_bank_assign_buffers(None, 0, 0, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.knh_bank_add_buffer(None, 0, s.ctypes.data_as(C.c_void_p), 8, 48000.0, None) == L.ERR_INVALID_ARGUMENT
    assert lib.knh_bank_buffer_count(None, 0) == 0
    assert lib.knh_bank_buffer_count(b._h, 0) == 1
    b.close()


def test_python_wrapper_checks_the_constructor_rows(knh):
    b = knh.VoiceBank(sp.STAGES, 4)
    b.add_buffer(0, np.ones(8), 48000.0)
    with pytest.raises(ValueError):
        b.assign_buffers(0, [0, 1], [0, 0], np.ones((2, 2)))
    b.assign_buffers(0, [0, 1], 0, np.ones((2, 3)))  # one entry for all the voices named
    b.close()


def test_a_reader_stage_behind_galactic_forwards_the_pool(knh):
    """A chain that ends in the reverb wraps the bank that holds the reader: the pool calls reach it."""
    st = [Stage(L.STAGE_BUFFER_READER), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_GALACTIC)]
    b = knh.VoiceBank(st, 4, L.F32, 2)
    assert b.add_buffer(0, np.ones(8), 48000.0) == 0 and b.add_buffer(0, np.ones(3), 8000.0) == 1
    assert b.buffer_count(0) == 2 and b.buffer_count(2) == 0
    b.assign_buffers(0, [0, 3], [1, 1])
    assert status_of(b.add_buffer, 2, np.ones(8), 48000.0) == L.ERR_INVALID_ARGUMENT
    assert status_of(b.assign_buffers, 2, [0], [0]) == L.ERR_INVALID_ARGUMENT
    b.close()


@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_the_oracle_takes_the_shortest_buffers(oracle, sample_type):
    """Buffers of 2 and 3 frames, looping and one-shot, starts inside and past the end: the oracle renders finite samples
    and, for the one-shots, a done frame."""
    n, bs = 12, 64
    for (samples, sr) in sp.make_buffers(sp.POOL_SPEC[:2]):
        o = sp.oracle_on(oracle, n, bs, sample_type, (samples, sr), sp.sampler_ctor(n))
        ev = sp.sampler_traffic(n)
        peak, any_done = 0.0, False
        for blk in range(6):
            ev(blk, o)
            _, voices, _, done = o.process_block()
            assert np.isfinite(voices).all()
            peak = max(peak, float(np.abs(voices).max()))
            any_done = any_done or bool((done != sp.NOT_DONE).any())
        assert peak > 0 and any_done
        o.close()
