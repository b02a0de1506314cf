"""The device event resolver (kernels_events.hip, event_resolver.hpp) at the sizes where its code branches: more voices than
the scan has threads, more records on a voice than its LDS sort holds, launches that outgrow every buffer, a ninth wrapped
node per voice, partial blocks with armed delays.  Every case first proves, in plain Python and from the planned traffic
alone, that it reaches its branch; then per-voice signals are compared bit for bit with the CPU oracle (single-block launches),
and the mixes of multi-block launches with those of a block-by-block bank that was itself checked per voice."""
import numpy as np
import pytest

from helpers import assert_bit_equal, make_gpu, make_oracle
from knaster_amd import _lib as L
from knaster_amd import configs
from knaster_amd.bank import TRIGGER, Stage

gpu = pytest.mark.gpu
BS = 64
FLOAT, TRIG = L.VALUE_FLOAT, L.VALUE_TRIGGER
# resolver constants the premises are stated against (kernels_events.hip, event_resolver.hpp, Bank::init)
SCAN_THREADS, SORT_LDS, MIN_CAP, MAX_DEV_WRAPPED = 1024, 32, 16384, 8


def c3_chain(name, n, sample_type, sin_q, svf_q, env_q):
    """SinWt.wr_mul -> SvfFilter -> * EnvAsr (the C3 / C4 voice), its nodes wrapped in WrPreciseTiming as asked: the
    oscillator's and the envelope's queues are the device's, the filter's is the host's."""
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT, delayed_changes_per_block=sin_q), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_SVF, delayed_changes_per_block=svf_q),
          Stage(L.STAGE_MUL_ENV_ASR, delayed_changes_per_block=env_q)]
    w = configs.Workload(name, st, n, BS, sample_type, 2)
    w.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 0.5), 2: np.stack([np.zeros(n), p["cutoff"], p["q"], np.zeros(n)], axis=1),
              3: np.stack([p["attack"], p["release"]], axis=1)}
    return w


def send(bank, batch, **kw):
    v, s, p, kind, f, d = batch
    bank.param_apply_many(v, s, p, kind, f, None, d, **kw)


def check_voices(g, o, what):
    """One block on both; the per-voice signals bit for bit.  -> the bank's mix."""
    mix, gv, _ = g.process_block_voices()
    ov = o.process_block()[1]
    assert not np.isnan(ov).any(), what
    assert_bit_equal(gv, ov, what)
    return mix


# ---- 1. the scan's chunk loop ------------------------------------------------------------------------------------------------

SCAN_TARGETS = [(0, 0), (0, 1), (3, 0), (3, 1)]  # SinWt freq, phase_offset; EnvAsr attack_time, release_time: device-resolved


def scan_plan(n, block):
    """Voice v gets (7 v + block) % 5 records for its device-resolved nodes, as batches of "the j-th record of every voice
    that has one"; every third voice a filter cutoff as well (the host's list).  -> (batches, device records per voice)."""
    v = np.arange(n, dtype=np.int64)
    count = (7 * v + block) % 5
    batches = []
    for j in range(4):
        who = v[count > j]
        t = (who + j + block) % 4
        s = np.array([SCAN_TARGETS[i][0] for i in t], dtype=np.uint32)
        p = np.array([SCAN_TARGETS[i][1] for i in t], dtype=np.uint32)
        f = np.choose(t, [110.0 + (who % 997) * 2.0 + j, ((who * 7 + j) % 64) / 64.0, 0.001 + ((who + j) % 50) * 0.0004, 0.01 + ((who + j) % 40) * 0.002])
        d = ((13 * who + 17 * j + 5 * block) % BS).astype(np.uint16)  # spread over the block; 0 leaves the armed delay as it is
        batches.append((who.astype(np.uint32), s, p, FLOAT, f, d))
    third = v[v % 3 == 0]
    batches.append((third.astype(np.uint32), 2, 0, FLOAT, 300.0 + ((third + block) % 400) * 10.0, ((5 * third + block) % BS).astype(np.uint16)))
    return batches, count


@gpu
@pytest.mark.parametrize("n,sample_type", [(1024, L.F32), (1025, L.F32), (2047, L.F32), (2049, L.F32), (3100, L.F32), (1025, L.F64)])
def test_scan_over_more_voices_than_threads(knh, oracle, monkeypatch, n, sample_type):
    """ev_scan_kernel: 1 024 threads, each sums a chunk of ceil(n / 1024) voices -- whole chunks, a ragged last one, threads
    with nothing -- over record counts and host-list counts that differ from voice to voice (zeros among them)."""
    monkeypatch.delenv("KNH_DEV_EVENTS", raising=False)
    n_blocks = 4
    plans = [scan_plan(n, b) for b in range(n_blocks)]
    # the premise, from the traffic alone
    chunk = -(-n // SCAN_THREADS)
    assert (chunk >= 2 and (n % chunk != 0 or n // chunk < SCAN_THREADS)) or n == SCAN_THREADS  # (1 024: the last size with one voice per thread)
    for b, (batches, count) in enumerate(plans):
        got = np.zeros(n, dtype=np.int64)
        host = np.zeros(n, dtype=np.int64)
        for (v, s, _p, _k, _f, _d) in batches:
            stage = np.broadcast_to(np.asarray(s), v.shape)
            np.add.at(got, v[stage != 2], 1)
            np.add.at(host, v[stage == 2], 1)
        assert np.array_equal(got, count) and set(np.unique(got)) == {0, 1, 2, 3, 4}
        starts = np.concatenate([[0], np.cumsum(got)])
        assert len(np.unique(starts[:-1][got > 0])) == np.count_nonzero(got)  # every voice with records starts somewhere else
        assert host.max() == 1 and host.min() == 0 and host.sum() == (n + 2) // 3  # a host list that is not uniform either
    w = c3_chain(f"scan{n}", n, sample_type, 4, 1, 2)
    g, o = make_gpu(knh, w, L.MIX_LEFT_FOLD), make_oracle(oracle, w, want_mix=False)
    for bank in (g, o):
        bank.param_apply_many(np.arange(n, dtype=np.uint32), 3, 3, TRIG)
    check_voices(g, o, f"{n} voices: the note-on block")
    loud = 0.0
    for b, (batches, _count) in enumerate(plans):
        for batch in batches:
            send(g, batch)
            send(o, batch)
        mix = check_voices(g, o, f"{n} voices, block {b}")
        loud = max(loud, float(np.abs(mix).max()))
    assert loud > 1e-3
    g.close()
    o.close()


# ---- 2. the sort: LDS columns and the Shell sort in one workgroup ------------------------------------------------------------

SORT_COUNTS = [0, 1, 31, 32, 33, 34, 64, 100, 200]
SORT_VOICES = [3, 10, 17, 24, 31, 38, 45, 52, 59]  # all in the first workgroup of 64
SORT_TARGETS = [(0, 0, FLOAT), (3, 0, FLOAT), (0, 1, FLOAT), (0, 0, FLOAT), (3, 1, FLOAT), (0, 2, TRIG), (0, 0, FLOAT), (3, 3, TRIG), (0, 1, FLOAT)]


def sort_plan(n, block):
    """-> (batches, records per voice).  Batch r holds the r-th record of every voice that has one, so no voice's records are
    neighbours on arrival; the calls arm delays all over the block (bs - 1, bs, bs + 5 among them) or none: then the delay
    armed before stays, and where none ever was the change goes straight through."""
    count = np.arange(n, dtype=np.int64) % 4
    for i, v in enumerate(SORT_VOICES):
        count[v] = SORT_COUNTS[(i + block) % len(SORT_COUNTS)]
    batches = []
    recs = np.zeros(n, dtype=np.int64)
    for r in range(int(count.max())):
        who = np.nonzero(count > r)[0]
        t = (who + r) % len(SORT_TARGETS)
        s = np.array([SORT_TARGETS[i][0] for i in t], dtype=np.uint32)
        p = np.array([SORT_TARGETS[i][1] for i in t], dtype=np.uint32)
        kind = np.array([SORT_TARGETS[i][2] for i in t], dtype=np.uint32)
        f = np.where(s == 0, np.where(p == 0, 150.0 + 9.0 * who + r, ((who * 5 + r) % 97) / 97.0), 0.002 + ((who + 3 * r) % 30) * 0.001)
        d = 1 + (5 * r + who) % 40
        d = np.where(r % 11 == 10, np.array([BS - 1, BS, BS + 5])[(r // 11 + who + block) % 3], d)
        d = np.where(r % 6 == 5, 0, d).astype(np.uint16)
        recs[who] += 1
        batches.append((who.astype(np.uint32), s, p, kind, f, d))
    return batches, recs


@gpu
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_sort_in_lds_and_in_place_side_by_side(knh, oracle, monkeypatch, sample_type):
    """ev_resolve_kernel sorts a voice's keys in LDS up to 32 of them and in place beyond: 0, 1, 31, 32, 33, 34, 64, 100 and
    200 records on voices of one 64-thread workgroup, delivered interleaved; a queue that holds 48 changes beside one that
    holds 2.  Then the same traffic scheduled ahead, later blocks first, some of it beyond the launch."""
    monkeypatch.delenv("KNH_DEV_EVENTS", raising=False)
    n, n_blocks = 130, 6
    plans = [sort_plan(n, b) for b in range(n_blocks)]
    for items, recs in plans:  # the premise: both sort paths, and both sides of the threshold, inside workgroup 0
        assert max(SORT_VOICES) < 64 and {int(recs[v]) for v in SORT_VOICES} == {0, 1, SORT_LDS - 1, SORT_LDS, SORT_LDS + 1, 34, 64, 100, 200}
        assert recs[64:].max() <= 3
        for batch in items:
            assert np.all(np.diff(batch[0].astype(np.int64)) > 0)  # one record per voice and batch: a voice's records never arrive side by side
    delays = np.concatenate([batch[5] for items, _ in plans for batch in items])
    assert {0, BS - 1, BS, BS + 5} <= set(delays.tolist())
    w = c3_chain("sort", n, sample_type, 48, 0, 2)
    a, c, o = make_gpu(knh, w, L.MIX_LEFT_FOLD), make_gpu(knh, w), make_oracle(oracle, w, want_mix=False)
    for bank in (a, c, o):
        bank.param_apply_many(np.arange(n, dtype=np.uint32), 3, 3, TRIG)
    mixes = []
    for b, (items, _recs) in enumerate(plans):
        for batch in items:
            for bank in (a, c, o):
                send(bank, batch)
        mix, cv, _ = c.process_block_voices()  # the tree-mix bank block by block: its voices are checked too, its mix is the yardstick below
        ov = o.process_block()[1]
        assert not np.isnan(ov).any()
        assert_bit_equal(a.process_block_voices()[1], ov, f"block {b} per voice")
        assert_bit_equal(cv, ov, f"block {b} per voice (tree-mix bank)")
        mixes.append(mix)
    assert max(float(np.abs(m).max()) for m in mixes) > 1e-3
    # scheduled ahead: one 4-block launch, the batches of the later blocks first (arrival index and block order disagree),
    # blocks 4 and 5 addressed beyond it
    b_ = make_gpu(knh, w)
    b_.param_apply_many(np.arange(n, dtype=np.uint32), 3, 3, TRIG)
    for off in range(n_blocks - 1, -1, -1):
        for batch in plans[off][0]:
            send(b_, batch, block_offset=off)
    out = np.concatenate([b_.process_blocks(4)[0], b_.process_blocks(2)[0]])
    for b in range(n_blocks):
        assert_bit_equal(out[b], mixes[b], f"scheduled ahead: block {b}")
    for bank in (a, b_, c, o):
        bank.close()


# ---- 3. buffer growth ------------------------------------------------------------------------------------------------------

class GrowthModel:
    """DevEventResolver's buffer policy restated (reserve(), resolve()): every buffer starts empty and grows to
    max(2 x need, 16 384); pinned record buffers and output sets alternate from launch to launch.  Replays planned traffic
    and notes which of the growth paths it takes."""

    def __init__(self):
        self.pinned, self.parity, self.n, self.keys, self.out, self.out_parity, self.hit = [0, 0], 0, 0, 0, [0, 0], 0, set()

    def batch(self, m):
        if self.n + m > self.pinned[self.parity]:
            if self.n:
                self.hit.add("pinned buffer grows while it holds records")
            self.pinned[self.parity] = max(2 * (self.n + m), MIN_CAP)
        self.n += m

    def launch(self, n_later):
        n_now, other = self.n - n_later, self.parity ^ 1
        if n_later > self.pinned[other]:
            if self.pinned[other]:
                self.hit.add("carry-over buffer grows")
            self.pinned[other] = max(2 * n_later, MIN_CAP)
        if n_now > self.keys:
            if self.keys:
                self.hit.add("device keys and records reallocated after use")
            self.keys = max(2 * n_now, MIN_CAP)
        if n_now > self.out[self.out_parity]:
            if self.out[self.out_parity]:
                self.hit.add("device output events reallocated after use")
            self.out[self.out_parity] = max(2 * n_now, MIN_CAP)
        self.out_parity ^= 1
        self.parity, self.n = other, n_later


def growth_batch(n, per_voice, salt, lo=0):
    """`per_voice` records for each voice, record-major (voices interleaved), every one with a value of its voice's own at a
    frame of its own: C5's modulator freq and phase_offset and the carrier's phase_offset in turn, delays rising with the
    record so that each takes hold for some frames before the next."""
    v = np.tile(np.arange(n, dtype=np.int64), per_voice)
    r = np.repeat(np.arange(per_voice, dtype=np.int64), n) + lo
    t = (v + r) % 3
    s = np.where(t == 2, 3, 0).astype(np.uint32)
    p = np.where(t == 0, 0, 1).astype(np.uint32)
    f = np.where(t == 0, 120.0 + 0.37 * v + 11.0 * r + salt, ((v * 7 + r * 13 + salt) % 1000) / 1000.0)
    d = np.minimum(BS - 1, 8 + v % 3 + 3 * r).astype(np.uint16)
    return v.astype(np.uint32), s, p, FLOAT, f, d


def split(batch, at):
    return tuple(x[:at] if isinstance(x, np.ndarray) else x for x in batch), tuple(x[at:] if isinstance(x, np.ndarray) else x for x in batch)


@gpu
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_launches_that_outgrow_every_buffer(knh, oracle, monkeypatch, sample_type):
    """Three launches on one bank, each with more records than the buffers of the launches before can take: the pinned
    record buffer grows while it holds records, the device buffers are freed and allocated anew after kernels have used
    them, and a scheduled-ahead launch carries more records over to the next than the other pinned buffer holds."""
    monkeypatch.delenv("KNH_DEV_EVENTS", raising=False)
    n = 2100
    v100 = np.arange(100, dtype=np.uint32)
    first = (v100, 0, 0, FLOAT, 3000.0 + 7.0 * v100, (1 + v100 % 5).astype(np.uint16))  # (frames 1-5: before the first of the big batch, frame 8)
    l1 = [first, growth_batch(n, 8, 1)]
    l2 = list(split(growth_batch(n, 17, 2), n * 17 // 2))
    l3 = {off: [growth_batch(n, 9, 3 + off)] for off in range(4)}  # blocks 0, 1 of a 2-block launch; 2, 3 beyond it
    # the premise: every growth path, by the policy and the planned record counts alone
    m = GrowthModel()
    for batch in l1:
        m.batch(len(batch[0]))
    assert m.n > MIN_CAP
    m.launch(0)
    for batch in l2:
        m.batch(len(batch[0]))
    m.launch(0)
    later = sum(len(bt[0]) for off in (2, 3) for bt in l3[off])
    for off in range(4):
        for batch in l3[off]:
            m.batch(len(batch[0]))
    assert later > MIN_CAP
    m.launch(later)
    assert m.hit == {"pinned buffer grows while it holds records", "device keys and records reallocated after use",
                     "device output events reallocated after use", "carry-over buffer grows"}, m.hit
    w = configs.config("C5", n_voices=n, block_size=BS, sample_type=sample_type, precise=16)
    g, c, o = make_gpu(knh, w), make_gpu(knh, w), make_oracle(oracle, w, want_mix=False)
    loud = 0.0
    for k, launch in enumerate((l1, l2)):  # single blocks: per voice against the oracle, on the bank under test itself
        for batch in launch:
            for bank in (g, c, o):
                send(bank, batch)
        mix, gv, _ = g.process_block_voices()
        ov = o.process_block()[1]
        assert_bit_equal(gv, ov, f"launch {k + 1} per voice")
        assert_bit_equal(c.process_block_voices()[1], ov, f"launch {k + 1} per voice (block-by-block bank)")
        loud = max(loud, float(np.abs(mix).max()))
    for off in range(4):
        for batch in l3[off]:
            send(g, batch, block_offset=off)
    out = np.concatenate([g.process_blocks(2)[0], g.process_blocks(2)[0]])
    for off in range(4):
        for batch in l3[off]:
            send(c, batch)
            send(o, batch)
        mix, cv, _ = c.process_block_voices()
        assert_bit_equal(cv, o.process_block()[1], f"block {off} of the scheduled launches, per voice (block-by-block bank)")
        assert_bit_equal(out[off], mix, f"block {off} of the scheduled launches")
    assert loud > 1e-4
    for bank in (g, c, o):
        bank.close()


# ---- 4. the ninth wrapped node ----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("sample_type", [L.F32, L.F64])
def test_ninth_and_tenth_wrapped_nodes_are_the_hosts(knh, oracle, monkeypatch, sample_type):
    """Ten oscillators, each times a constant gain wrapped in WrPreciseTiming, summed: ten device-resolvable queues per voice,
    of which the device takes eight.  Equal delays on the 8th (device), 9th and 10th (host, merged on the device) of the same
    voices in the same block; the 1st also queues a later change, so that a queue shared between two nodes would show."""
    monkeypatch.delenv("KNH_DEV_EVENTS", raising=False)
    n, n_osc = 70, 10
    st = []
    for i in range(n_osc):
        st += [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_MUL_CONST, delayed_changes_per_block=2)]
    for i in range(n_osc - 1):
        st.append(Stage(L.STAGE_MATH_ADD, input=len(st), input2=2 * i + 2))  # (the stage before: the last gain, then the sum so far) + gain stage i
    gains = [2 * i + 1 for i in range(n_osc)]
    wrapped = [i for i, s in enumerate(st) if s.delayed_changes_per_block > 0]
    assert wrapped == gains and len(wrapped) > MAX_DEV_WRAPPED + 1  # the premise: a ninth and a tenth queue the device could take
    w = configs.Workload("ten", st, n, BS, sample_type, 1)
    vs = np.arange(n)
    w.ctor = {}
    for i in range(n_osc):
        w.ctor[2 * i] = (110.0 * (i + 1) * (1.0 + 0.01 * vs)).reshape(n, 1)
        w.ctor[2 * i + 1] = np.full((n, 1), 0.05)
    g, o = make_gpu(knh, w, L.MIX_LEFT_FOLD), make_oracle(oracle, w, want_mix=False)
    v = vs.astype(np.uint32)
    loud = 0.0
    for b in range(4):
        d = (1 + (5 * vs + 11 * b) % (BS - 2)).astype(np.uint16)
        late = np.minimum(BS - 1, d.astype(np.int64) + 9).astype(np.uint16)
        batches = [(v, gains[0], 0, FLOAT, 0.02 + 0.001 * vs + 0.01 * b, late)]  # the 1st wrapped node queues a change behind the 8th's frame
        for i in (7, 8, 9):
            batches.append((v, gains[i], 0, FLOAT, 0.03 + 0.002 * vs + 0.01 * i + 0.005 * b, d))  # equal delays, device and host side
        for i in (1, 2, 3):  # never armed: straight through
            batches.append((v[i::4], gains[i], 0, FLOAT, 0.04 + 0.001 * vs[i::4] + 0.003 * b, None))
        batches.append((v[::2], gains[8], 0, FLOAT, 0.09 - 0.001 * vs[::2], np.minimum(BS, d[::2] + 20).astype(np.uint16)))  # a second change on the 9th
        for batch in batches:
            send(g, batch)
            send(o, batch)
        loud = max(loud, float(np.abs(check_voices(g, o, f"block {b}")).max()))
    assert loud > 1e-3
    g.close()
    o.close()


# ---- 5. partial blocks with armed delays ---------------------------------------------------------------------------------------

def whole_block_script(parts, armed):
    """WrPreciseTiming's queue (precise_timing.rs:75-114, 126-148) for a block processed in parts.
    parts: [(block_start_offset, frames_to_process, calls)], calls made before that part is processed, in order, each
    (node, param, delay or None, value): the delay is armed first unless None.  armed: {(node, param): delay}, persists
    (updated in place).  -> [(node, param, value, frame)] in the order the changes are applied: the in-block frame at which
    each takes hold (block size: applied behind the block's last frame); changes that are lost do not appear."""
    out = []
    for offset, frames, calls in parts:
        queues = {}
        for node, param, delay, value in calls:
            if delay is not None:
                armed[(node, param)] = delay
            d = armed.get((node, param), 0)
            if d == 0:
                out.append((node, param, value, offset))  # applied when called: from the first frame processed next
            else:
                queues.setdefault(node, []).append((d, param, value))
        for node, queue in queues.items():
            block_i = 0
            for d, param, value in queue:
                due = max(d, offset + block_i)
                if due > offset + frames:
                    break  # not due inside this call: lost, and so is everything queued behind it
                out.append((node, param, value, due))
                block_i = due - offset
    return out


def test_translator_change_due_exactly_at_the_split():
    assert whole_block_script([(0, 17, [(0, 0, 17, "a")]), (17, 47, [])], {}) == [(0, 0, "a", 17)]


def test_translator_late_change_blocks_its_follower_only_on_its_node():
    parts = [(0, 17, [(0, 0, 30, "a"), (0, 1, 5, "b"), (3, 0, 5, "c")]), (17, 47, [(0, 1, 20, "d")])]
    assert whole_block_script(parts, {}) == [(3, 0, "c", 5), (0, 1, "d", 20)]


def test_translator_early_delay_between_the_parts_takes_hold_at_the_split():
    assert whole_block_script([(0, 17, []), (17, 47, [(0, 0, 5, "a"), (0, 1, 17, "b"), (0, 0, 40, "c")])], {}) == \
        [(0, 0, "a", 17), (0, 1, "b", 17), (0, 0, "c", 40)]


def test_translator_block_size_is_still_due_and_one_more_is_not():
    assert whole_block_script([(0, 17, []), (17, 47, [(0, 0, 64, "a"), (3, 0, 65, "b"), (3, 0, 20, "c")])], {}) == [(0, 0, "a", 64)]


def test_translator_fifo_never_goes_back_and_armed_delays_persist():
    armed = {}
    parts = [(0, 17, [(0, 0, 12, "a"), (0, 1, 3, "b")]), (17, 47, [(0, 0, None, "c"), (0, 1, None, "d")])]
    assert whole_block_script(parts, armed) == [(0, 0, "a", 12), (0, 1, "b", 12), (0, 0, "c", 17), (0, 1, "d", 17)]
    assert armed == {(0, 0): 12, (0, 1): 3}
    # the next block, whole, nothing re-armed; then a delay disarmed between two parts: applied when called
    assert whole_block_script([(0, 64, [(0, 1, None, "e"), (0, 0, None, "f")])], armed) == [(0, 1, "e", 3), (0, 0, "f", 12)]
    assert whole_block_script([(0, 1, []), (1, 63, [(0, 0, 0, "g"), (0, 1, None, "h")])], armed) == [(0, 0, "g", 1), (0, 1, "h", 3)]


PARTIAL_NODES = [0, 2, 3]  # SinWt, EnvAsr, the constant gain


def partial_plan(n, k, block):
    """Per voice: two changes per node before part [0, k) and two between the parts, their delays on both sides of k and of
    the block size.  -> {voice: (calls before part 1, calls before part 2)}, and the kinds of delay it used."""
    lt = k - 1                       # d < k (k = 1: zero -- disarmed, straight through)
    mid = k + (BS - k) // 2          # k < d2 < B where there is such a frame
    p1 = [(lt, k), (k, k + 3), (k + 3, lt), (k, k), (lt, lt)]
    p2 = [(lt, k), (k, mid), (mid, BS), (BS, BS + 5), (BS + 5, lt), (lt, BS)]
    plan, kinds = {}, set()
    for v in range(n):
        before, between = [], []
        for ni, node in enumerate(PARTIAL_NODES):
            for part, (calls, menu) in enumerate(((before, p1), (between, p2))):
                pair = menu[(v + block * (1 + part) + ni) % len(menu)]
                for idx, d in enumerate(pair):
                    if node == 0:
                        param, value = idx, (180.0 + 3.0 * v + 17.0 * block + 5.0 * part) if idx == 0 else ((v * 3 + block * 7 + part) % 31) / 31.0
                    elif node == 2:
                        param, value = (2 + (v + block + part) % 2, TRIGGER) if idx == 0 else (part, 0.002 + 0.001 * ((v + block) % 9) + 0.01 * part)
                    else:
                        param, value = 0, 0.1 + 0.01 * ((v + 3 * block + 2 * part + idx) % 50)
                    calls.append((node, param, d, value))
                    if part == 0:
                        kinds.add("d<k" if d < k else "d==k" if d == k else "d>k")
                    else:
                        kinds.add("d2<k" if d < k else "d2==k" if d == k else "k<d2<B" if d < BS else "d2==B" if d == BS else "d2>B")
        plan[v] = (before, between)
    return plan, kinds


def apply_calls(bank, voice, calls):
    for node, param, delay, value in calls:
        if delay is not None:
            bank.set_delay_within_block_for_param(voice, node, param, delay)
        bank.param_apply(voice, node, param, value)


@gpu
@pytest.mark.parametrize("k,sample_type,dev_events", [(k, L.F32, m) for k in (1, 17, 63) for m in (None, "0")] + [(17, L.F64, None), (17, L.F64, "0")])
def test_armed_delays_across_partial_blocks(knh, oracle, monkeypatch, k, sample_type, dev_events):
    """Every block as [0, k) then [k, B), delays armed before and between the parts on both sides of k and B, two changes per
    node and part (a late one blocks its follower): frame_begin > 0 and frame_end < block_size in the resolver kernel and,
    with KNH_DEV_EVENTS=0, in the host's resolve_qrecs.  The oracle renders whole blocks: it is driven by whole_block_script's
    translation -- arm the frame at which the change takes hold, then the value."""
    if dev_events is None:
        monkeypatch.delenv("KNH_DEV_EVENTS", raising=False)
    else:
        monkeypatch.setenv("KNH_DEV_EVENTS", dev_events)
    n, n_blocks = 70, 4
    plans = [partial_plan(n, k, b) for b in range(n_blocks)]
    want = {"d<k", "d==k", "d>k", "d2<k", "d2==k", "d2==B", "d2>B"} | ({"k<d2<B"} if k + 1 < BS - 1 else set())
    armed = [dict() for _ in range(n)]
    scripts, lost = [], 0
    for plan, kinds in plans:
        assert kinds >= want, (k, want - kinds)  # the premise: every relation of a delay to the split and to the block's end
        script = {}
        for v, (before, between) in plan.items():
            script[v] = whole_block_script([(0, k, before), (k, BS - k, between)], armed[v])
            lost += len(before) + len(between) - len(script[v])
            per_node = {}
            for node, _p, _val, frame in script[v]:
                assert per_node.get(node, 0) <= frame <= BS  # (what the oracle's whole block can be told: frames that never decrease on a node)
                per_node[node] = frame
            assert max(sum(1 for c in before + between if c[0] == node) for node in PARTIAL_NODES) <= 8  # the capacity is never the difference
        scripts.append(script)
    assert lost > 0  # head-of-line blocking happened
    p = configs.voice_parameters(n)
    st = [Stage(L.STAGE_SIN_WT, delayed_changes_per_block=8), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_MUL_ENV_ASR, delayed_changes_per_block=8),
          Stage(L.STAGE_MUL_CONST, delayed_changes_per_block=8)]
    w = configs.Workload(f"parts{k}", st, n, BS, sample_type, 2)
    w.ctor = {0: p["freq"].reshape(n, 1), 1: np.full((n, 1), 0.5), 2: np.stack([p["attack"], p["release"]], axis=1), 3: np.full((n, 1), 0.25)}
    g, o = make_gpu(knh, w, L.MIX_LEFT_FOLD), make_oracle(oracle, w, want_mix=False)
    for bank in (g, o):
        bank.param_apply_many(np.arange(n, dtype=np.uint32), 2, 3, TRIG)
    loud = 0.0
    for b, (plan, _kinds) in enumerate(plans):
        for v in range(n):
            apply_calls(g, v, plan[v][0])
        part1 = g.process_block_voices(frames_to_process=k, block_start_offset=0)[1]
        for v in range(n):
            apply_calls(g, v, plan[v][1])
        part2 = g.process_block_voices(frames_to_process=BS - k, block_start_offset=k)[1]
        for v in range(n):
            apply_calls(o, v, [(node, param, frame, value) for node, param, value, frame in scripts[b][v]])
        ov = o.process_block()[1]
        assert not np.isnan(ov).any()
        assert_bit_equal(np.concatenate([part1[:, :k], part2[:, k:]], axis=1), ov, f"split at {k}, block {b}")
        loud = max(loud, float(np.abs(ov).max()))
    assert loud > 1e-3
    g.close()
    o.close()
