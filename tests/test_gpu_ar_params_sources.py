"""Audio-rate links (WrArParams, audio_rate.rs:11-85; `link`, graph_edit.rs:735-754) on the nodes a synthesiser bank is used
for first: PolyBlep freq and pulse_width, RandomLin freq, BufferReader rate, the segment Envelope's time_scale.
Against the oracle, whose voices hold the reference's own wrapper and parameter edge.  All five setters are + - x / and
stores: bit for bit wherever the node itself is (the four PolyBlep waveforms that call sin, and every waveform at or above
sample_rate / 4, stay within 4e-6 of a unit-range signal, the bound tests/test_gpu_parity.py holds PolyBlep to).  Under the
wrapper a node runs through UGen::process: a one-shot reader (buffer.rs:143) and the Envelope (envelopes.rs:457) mark done
at frame 0.  Banks of 3, 65 and 130 voices: a partial wavefront, one lane over, a third wavefront."""
import numpy as np
import pytest

import ar_sources
import sampler_pool as sp
from helpers import assert_bit_equal, fire_all, make_gpu, make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import Stage

pytestmark = pytest.mark.gpu

SIZES = [3, 65, 130]
TYPES = [L.F32, L.F64]
SIN_TOL = 4e-6
NOT_DONE = sp.NOT_DONE


def dtype_of(sample_type):
    return np.float64 if sample_type == L.F64 else np.float32


def run(knh, oracle, w, blocks, events=None, exact=None, check_mix=True):
    """Both banks block by block.  exact: None -- every sample bit for bit, the left-fold mix too; or a [n_voices] mask of the
    voices that are (the others within SIN_TOL; the mix then within what n voices off by SIN_TOL and the rounding of the n
    additions of the fold can come to).  -> (oracle voices [blocks, n, bs], oracle done frames [blocks, n])"""
    g = make_gpu(knh, w, L.MIX_LEFT_FOLD)
    o = make_oracle(oracle, w)
    all_voices, all_done = [], []
    for b in range(blocks):
        if events:
            events(b, g)
            events(b, o)
        g_out, g_voices, _ = g.process_block_voices()
        o_out, o_voices, _, o_done = o.process_block()
        assert np.isfinite(o_voices).all() and np.isfinite(g_voices).all(), f"{w.name} block {b}"
        if exact is None:
            assert_bit_equal(g_voices, o_voices, f"{w.name} block {b} per-voice")
            if check_mix:
                assert_bit_equal(g_out, o_out, f"{w.name} block {b} left-fold mix")
        else:
            if exact.any():
                assert_bit_equal(g_voices[exact], o_voices[exact], f"{w.name} block {b} per-voice (waveforms without sin)")
            err = np.max(np.abs(g_voices.astype(np.float64) - o_voices.astype(np.float64)))
            print(f"{w.name} block {b}: largest per-voice error {err:.3e}")
            assert err <= SIN_TOL, f"{w.name} block {b}: {err} > {SIN_TOL}"
            n = w.n_voices
            partial = np.abs(o_voices.astype(np.float64)).sum(axis=0).max() + n * SIN_TOL  # no partial sum of the fold is larger
            mix_tol = n * SIN_TOL + n * 0.5 * np.finfo(o_voices.dtype).eps * partial
            mix_err = np.max(np.abs(g_out.astype(np.float64) - o_out.astype(np.float64)))
            print(f"{w.name} block {b}: mix error {mix_err:.3e} (bound {mix_tol:.3e})")
            assert mix_err <= mix_tol, f"{w.name} block {b} mix: {mix_err} > {mix_tol}"
        np.testing.assert_array_equal(g.read_done_frames(), o_done, err_msg=f"{w.name} block {b} done frames")
        all_voices.append(o_voices.copy())
        all_done.append(o_done.copy())
    g.close()
    o.close()
    all_voices = np.stack(all_voices)
    assert np.abs(all_voices).max() > 1e-4
    return all_voices, np.stack(all_done)


def without_sin(n):
    return ~np.isin(np.arange(n) % 14, ar_sources.SIN_WAVEFORMS)


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_polyblep_freq(knh, oracle, n, sample_type):
    """osc.link("freq", lfo): dt = F(v) / F(sample_rate) every sample.  An ordinary change of the linked parameter is ignored
    while the link stands (audio_rate.rs:70-74); the driver's own parameters change as ever."""
    w = ar_sources.workload("polyblep_freq", n, sample_type)

    def ev(block, bank):
        if block == 2:
            bank.param_apply(5 % n, 3, 0, 0.123)
            bank.param_apply(7 % n, 1, 0, 17.0)
    run(knh, oracle, w, 6, ev, exact=without_sin(n))


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_polyblep_across_quarter_rate(knh, oracle, n, sample_type):
    """The driver crosses sample_rate / 4 = 12 kHz, where next_sample renders a sine whatever the waveform (polyblep.rs:210):
    decided per sample from the new dt.  Every sample within 4e-6; where the driver is below 12 kHz and the waveform calls
    no sin, bit for bit."""
    w = ar_sources.workload("polyblep_across_quarter_rate", n, sample_type)
    blocks = 6
    d = configs.Workload("ars_driver", w.stages[:3], n, w.block_size, sample_type, 1)
    d.ctor = {k: a for k, a in w.ctor.items() if k < 3}
    od = make_oracle(oracle, d)
    driver = np.stack([od.process_block()[1] for _ in range(blocks)])  # [blocks, n, bs]
    od.close()
    assert ((driver < 12000.0).any(axis=(0, 2)) & (driver >= 12000.0).any(axis=(0, 2))).all(), "every voice sees both sides"
    g = make_gpu(knh, w, L.MIX_LEFT_FOLD)
    o = make_oracle(oracle, w)
    plain = without_sin(n)[:, None]
    compared = 0
    for b in range(blocks):
        _, g_voices, _ = g.process_block_voices()
        _, o_voices, _, o_done = o.process_block()
        err = np.max(np.abs(g_voices.astype(np.float64) - o_voices.astype(np.float64)))
        print(f"{w.name} block {b}: largest per-voice error {err:.3e}")
        assert err <= SIN_TOL, f"block {b}: {err} > {SIN_TOL}"
        below = (driver[b] < 12000.0) & plain
        compared += int(below.sum())
        assert_bit_equal(g_voices[below], o_voices[below], f"block {b}: below sample_rate / 4, waveforms without sin")
        np.testing.assert_array_equal(g.read_done_frames(), o_done)
    assert compared > 0
    g.close()
    o.close()


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_polyblep_pulse_width(knh, oracle, n, sample_type):
    w = ar_sources.workload("polyblep_pulse_width", n, sample_type)
    run(knh, oracle, w, 6, exact=without_sin(n))


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_random_lin_freq(knh, oracle, n, sample_type):
    """phase_step = F(v) * (F(1) / F(sample_rate)); at 100 .. 1 900 Hz several new values are drawn in a 96-frame block."""
    w = ar_sources.workload("random_lin_freq", n, sample_type)
    run(knh, oracle, w, 6)


def reader_events(n):
    def ev(block, bank):
        if block == 2:  # ignored while the link stands
            bank.param_apply_many(np.arange(n, dtype=np.uint32), 3, 0, L.VALUE_FLOAT, np.full(n, 0.31))
        if block == 9:
            fire_all(bank, n, 3, 5)  # t_restart
    return ev


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n", SIZES + [67])
def test_reader_rate(knh, oracle, n, sample_type):
    """reader.link("rate", lfo): the per-sample step is base_rate * rate with the driver's sample as the rate.  Odd voices
    loop; the one-shot voices end inside the run and report done frame 0, as the reference's process does under the wrapper
    (buffer.rs:143), not the frame after the last one (process_block, :172)."""
    w = ar_sources.workload("reader_rate", n, sample_type)
    _, done = run(knh, oracle, w, 12, reader_events(n))
    one_shot = np.arange(n) % 2 == 0
    assert set(np.unique(done).tolist()) == {0, NOT_DONE}
    assert (done[:9, one_shot] == 0).any(axis=0).all(), "every one-shot voice ends before the restart"
    assert (done[:, ~one_shot] == NOT_DONE).all()


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("n", SIZES)
def test_reader_rate_across_a_buffer_swap(knh, oracle, n, sample_type):
    """Three pool entries with sample rates of their own.  At block 4 the voices v % 3 == 1 move to the next entry: the new
    reader takes that entry's base_rate (the slot pair the linked form adds) and stands linked to the same signal.  The
    driver is INPUT * c_v + 1, stateless, so an oracle bank made fresh for the new entry sees the same driver; the expected
    signal is assembled as tests/sampler_pool.py describes."""
    bs, blocks, swap_at = 96, 8, 4
    dtype = dtype_of(sample_type)
    buffers = sp.make_buffers([(700, 22050.0), (900, 44100.0), (1100, 48000.0)])
    v = np.arange(n)
    st = [Stage(L.STAGE_INPUT), Stage(L.STAGE_MUL_CONST), Stage(L.STAGE_ADD_CONST),
          Stage(L.STAGE_BUFFER_READER, ar_param=1, input2=3), Stage(L.STAGE_MUL_CONST)]
    reader_ctor = np.stack([np.ones(n), (v % 2).astype(np.float64), np.zeros(n)], axis=1)
    ctor = {0: np.zeros((n, 1)), 1: (0.1 + 0.005 * v).reshape(n, 1), 2: np.ones((n, 1)), 3: reader_ctor, 4: np.full((n, 1), 1.0 / n)}
    t = np.arange(blocks * bs) / configs.SAMPLE_RATE
    ins = np.sin(2 * np.pi * 90.0 * t).astype(dtype).reshape(blocks, 1, bs)
    ids = (v % 3).astype(np.uint32)
    moved = v % 3 == 1

    def oracle_on(entry):
        w = configs.Workload("ars_swap", st, n, bs, sample_type, 1, in_channels=1)
        w.ctor = ctor
        w.buffer = (3, buffers[entry][0], buffers[entry][1])
        return make_oracle(oracle, w, want_mix=False)

    g = knh.VoiceBank(st, n, sample_type, 1, L.MIX_LEFT_FOLD, in_channels=1)
    for s, a in ctor.items():
        g.set_ctor_args(s, a)
    for k, (samples, sr) in enumerate(buffers):
        assert g.add_buffer(3, samples, sr) == k
    g.assign_buffers(3, v.astype(np.uint32), ids)
    g.init(configs.SAMPLE_RATE, bs)
    banks = {(0, e): oracle_on(e) for e in range(3)}  # (the block its readers were made at, entry)
    gen = np.zeros(n, dtype=np.int64)
    for b in range(blocks):
        if b == swap_at:
            ids[moved] = (ids[moved] + 1) % 3
            gen[moved] = b
            g.assign_buffers(3, v[moved].astype(np.uint32), ids[moved], reader_ctor[moved])
            for e in sorted(set(ids[moved].tolist())):
                banks[(b, e)] = oracle_on(e)
        expect = np.zeros((n, bs), dtype=dtype)
        done = np.full(n, NOT_DONE, dtype=np.uint32)
        for (made, e), bank in banks.items():
            bank.set_input(ins[b])
            _, rows, _, d = bank.process_block()
            mine = (gen == made) & (ids == e)
            expect[mine] = rows[mine]
            done[mine] = d[mine]
        g.set_input(ins[b])
        g_out, g_voices, _ = g.process_block_voices()
        assert_bit_equal(g_voices, expect, f"block {b} per-voice")
        assert_bit_equal(g_out[0], sp.left_fold(expect), f"block {b} left-fold mix")
        np.testing.assert_array_equal(g.read_done_frames(), done, err_msg=f"block {b} done frames")
    assert np.abs(expect).max() > 1e-4
    g.close()
    for bank in banks.values():
        bank.close()


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("looping", [False, True])
@pytest.mark.parametrize("n", SIZES + [67])
def test_envelope_time_scale(knh, oracle, n, looping, sample_type):
    """env.link("time_scale", lfo): time_scale = (double)F(v), a sample's increment time_scale * base_scale.  Not looping,
    every voice ends once and reports frame 0 (envelopes.rs:457)."""
    w = ar_sources.workload("envelope_time_scale", n, sample_type, looping=looping)

    def ev(block, bank):
        if block == 0:
            fire_all(bank, n, 4, 2)  # t_restart
    _, done = run(knh, oracle, w, 12, ev)
    if looping:
        assert (done == NOT_DONE).all()
    else:
        assert ((done == 0).sum(axis=0) == 1).all() and set(np.unique(done).tolist()) == {0, NOT_DONE}


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("case", ["polyblep_freq", "reader_rate"])
def test_one_launch_equals_block_by_block(knh, case, sample_type):
    """Whatever a linked stage stores back between launches: six blocks in one launch and the same six block by block give
    identical bits.  (The tree mix: the left fold takes one block per call.)"""
    w = ar_sources.workload(case, 65, sample_type)
    a = make_gpu(knh, w, L.MIX_TREE)
    b = make_gpu(knh, w, L.MIX_TREE)
    whole, _ = a.process_blocks(6)
    for k in range(6):
        out, _ = b.process_block()
        assert_bit_equal(out, whole[k], f"{case} block {k}", strict_zero=True)
    assert np.abs(whole).max() > 1e-4
    a.close()
    b.close()


@pytest.mark.parametrize("sample_type", TYPES)
@pytest.mark.parametrize("form", ["host_threads", "rank"])
def test_other_bank_forms(knh, form, sample_type):
    """The linked reader's slot layout differs from the plain one's: the bank cut into voice ranges for two host threads, and
    as one rank's share, renders the same bits as the plain bank, events and done frames included.  (A rank bank hands out
    the mix only, and with one rank it is the plain bank's; the host-sharded bank's mix is a sum of per-range tree mixes,
    held to the 1e-5 tests/test_gpu_multi.py holds it to -- its per-voice output is compared bit for bit.)"""
    n = 130
    w = ar_sources.workload("reader_rate", n, sample_type)
    ev = reader_events(n)
    plain = make_gpu(knh, w, L.MIX_TREE)
    other = make_gpu(knh, w, L.MIX_TREE, **(dict(host_threads=2) if form == "host_threads" else dict(rank=0, world=1)))
    peak = 0.0
    for b in range(12):
        ev(b, plain)
        ev(b, other)
        if form == "rank":
            p_out, _ = plain.process_block()
            o_out, _ = other.process_block()
            assert_bit_equal(o_out, p_out, f"rank block {b} mix", strict_zero=True)
        else:
            p_out, p_voices, _ = plain.process_block_voices()
            o_out, o_voices, _ = other.process_block_voices()
            assert_bit_equal(o_voices, p_voices, f"host_threads block {b} per-voice", strict_zero=True)
            assert np.max(np.abs(o_out.astype(np.float64) - p_out.astype(np.float64))) <= 1e-5
        np.testing.assert_array_equal(other.read_done_frames(), plain.read_done_frames())
        peak = max(peak, float(np.abs(p_out).max()))
    assert peak > 1e-4
    plain.close()
    other.close()
