"""Graph voices built from every stage kind, without a GPU: the library accepts every committed seed of
tests/graph_voices.py and every directed voice, hands out the signal slots as the rule says (restated in Python), their
kernels compile for gfx950, the oracle renders them finite and audible, and the committed seeds cover what the generator
is there to cover.  tests/test_gpu_graph_voices.py runs the same voices on the device."""
import collections
import functools
import hashlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import graph_voices as gv
from helpers import assert_bit_equal
from knaster_amd import _lib as L
from knaster_amd.bank import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "bin", "jit_compile_check")
SEEDS = list(range(gv.N_SEEDS))
VOICES = [f"seed{s}" for s in SEEDS] + gv.DIRECTED


@functools.lru_cache(maxsize=None)
def voice(name, sample_type=None):
    if name.startswith("seed"):
        return gv.random_graph_voice(int(name[4:]))
    return gv.directed_voice(name, 3, L.F32 if sample_type is None else sample_type)


def signature_of(knh, st):
    b = knh.VoiceBank(st, 3, L.F32, 2 if st[-1].kind == L.STAGE_PAN2 else 1, L.MIX_LEFT_FOLD)
    sig = b.debug_signature()
    b.close()
    return sig


@pytest.mark.parametrize("name", VOICES)
def test_voice_is_accepted_and_its_slots_follow_the_rule(knh, name):
    """knh_bank_create takes the voice as a graph ("@" operands, "#R" slots); the slots in its signature are the ones the
    rule gives -- first free slot, freed at the last reader, in place if the first operand dies here -- and no stage writes
    a slot whose signal still has a later reader."""
    w = voice(name)
    st = w.stages
    if name.startswith("seed"):
        assert 5 <= len(st) <= 14
        assert sum(gv.is_source(s) for s in st) >= 2
    sig = signature_of(knh, st)
    assert "@" in sig and "#" in sig, sig
    parsed, n_slots = gv.parse_signature(sig)
    assert len(parsed) == len(st), sig
    plan, want_slots = gv.slot_plan(st)
    assert [(a, b, o) for (_, _, a, b, o) in parsed] == plan, sig
    assert n_slots == want_slots
    assert [p for (_, p, _, _, _) in parsed] == [s.ar_param - 1 if s.ar_param else None for s in st]
    a, b = gv.operands(st)
    written = [o for (_, _, _, _, o) in parsed]
    for i, (_, _, sa, sb, _) in enumerate(parsed):  # every operand slot is the slot its signal was written to
        assert sa == (written[a[i]] if a[i] >= 0 else -1) and sb == (written[b[i]] if b[i] >= 0 else -1), (sig, i)
    assert gv.overwritten_live_signals(st, written) == [], sig


def test_the_slot_check_sees_a_signal_destroyed_before_its_last_reader():
    """The checker itself: a + b written over a while a later stage still reads a is reported; in place at the last reader
    is not."""
    st = [Stage(L.STAGE_SIN_WT), Stage(L.STAGE_PHASOR), Stage(L.STAGE_MATH_ADD, input=1, input2=2), Stage(L.STAGE_MATH_MUL, input=3, input2=1)]
    assert gv.overwritten_live_signals(st, [0, 1, 0, 0]) == [(2, 0)]
    assert gv.overwritten_live_signals(st, [0, 1, 1, 0]) == []
    plan, n_slots = gv.slot_plan(st)
    assert [o for (_, _, o) in plan] == [0, 1, 1, 0] and n_slots == 2


def test_a_reader_of_a_wrapped_stage_gets_the_wrappers_output(knh):
    """wrapped_fanout: the Svf, the OnePoleHpf (which names the SinWt, stage 1) and, through them, the product all read the
    slot the last wrapper wrote -- the signature says so, not only the restatement."""
    st = voice("wrapped_fanout").stages
    parsed, _ = gv.parse_signature(signature_of(knh, st))
    wrapped = parsed[2][4]
    assert parsed[3][2] == wrapped and parsed[4][2] == wrapped
    assert gv.operands(st)[0][4] == 2 and len(gv.readers(st)[2]) == 2 and gv.readers(st)[0] == [1]


@pytest.fixture(scope="module")
def jit_compile_check(knh):
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "bin/jit_compile_check"], check=True, capture_output=True)
    assert os.path.exists(CHECK)


@pytest.mark.parametrize("sample_type", ["f32", "f64"])
@pytest.mark.parametrize("name", gv.DIRECTED + [f"seed{s}" for s in range(4)])
def test_kernel_compiles_for_gfx950(knh, jit_compile_check, name, sample_type):
    """The fused kernel of the voice, built by hiprtc in a process of its own (tests/test_jit_compile.py)."""
    sig = signature_of(knh, voice(name).stages)
    p = subprocess.run([CHECK, sig] + (["f64"] if sample_type == "f64" else []), cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=900)
    assert p.returncode == 0, f"{name} {sig} ({sample_type}): rc {p.returncode}: {p.stdout.decode(errors='replace')[-600:]}"


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_renders_the_seed_finite_and_audible(oracle, seed):
    w = voice(f"seed{seed}")
    voices, mixes, _, _ = gv.oracle_run(oracle, w, 6)
    for b in range(6):
        assert np.isfinite(voices[b]).all() and np.isfinite(mixes[b]).all(), f"seed {seed} block {b}"
    peak = np.abs(voices).max(axis=(0, -1))  # per voice (per plane under Pan2), over the blocks
    assert (peak > 1e-4).all(), f"seed {seed}: silent voices {np.argwhere(peak <= 1e-4)[:5].tolist()}"


@pytest.mark.parametrize("name", gv.DIRECTED)
def test_oracle_renders_the_directed_voice_finite_and_audible(oracle, name):
    w = gv.directed_voice(name, 65, L.F32)
    voices, _, _, _ = gv.oracle_run(oracle, w, 12)
    assert np.isfinite(voices).all()
    assert (np.abs(voices).max(axis=(0, -1)) > 1e-4).all()


def coverage(voices):
    """What a list of voices holds -> Counter of items, each counted once per voice."""
    c = collections.Counter()
    for w in voices:
        st = w.stages
        a, _ = gv.operands(st)
        rd = gv.readers(st)
        have = set()
        for i, s in enumerate(st):
            have.add(("kind", s.kind))
            if s.kind in gv.DELAYS and s.input and a[i] != i - 1:
                have.add("delay reads a named signal that is not adjacent")
            if gv.is_wrapper(s) and not (i + 1 < len(st) and gv.is_wrapper(st[i + 1])) and len(rd[i]) >= 2:
                have.add("wrapper on a node with two readers")
        for s, (sa, _, o) in zip(st, gv.slot_plan(st)[0]):
            if sa >= 0 and sa != o and not gv.is_math2(s) and not s.ar_param:
                have.add("a stage's input is copied into another slot in front of its tile code")
        for kind in w.links.values():
            have.add(("link", kind))
        if st[-1].kind == L.STAGE_PAN2:
            have.add("Pan2 ends the voice")
        in_list, in_task = gv.envelope_orders(st)
        if len({st[i].kind for i in in_list}) >= 2 and in_list != in_task:
            have.add("envelopes of different kinds, task order is not list order")
        c.update(have)
    return c


def test_the_committed_seeds_cover_the_pool():
    """A condition on the seed list, not a measurement: every kind of the pool, every link kind and every structure the
    generator is for occurs in at least two of the committed seeds."""
    c = coverage([voice(f"seed{s}") for s in SEEDS])
    want = [("kind", k) for k in gv.POOL] + [("link", k) for k in gv.LINKS] + [
        "delay reads a named signal that is not adjacent", "wrapper on a node with two readers", "Pan2 ends the voice",
        "a stage's input is copied into another slot in front of its tile code",
        "envelopes of different kinds, task order is not list order"]
    short = {str(k): c[k] for k in want if c[k] < 2}
    assert not short, short
    sizes = {(voice(f"seed{s}").n_voices) for s in SEEDS}
    blocks = {(voice(f"seed{s}").block_size) for s in SEEDS}
    assert sizes == set(gv.VOICE_COUNTS) and blocks == set(gv.BLOCK_SIZES)
    assert {voice(f"seed{s}").sample_type for s in SEEDS} == {L.F32, L.F64}


def test_directed_voices_are_what_they_are_for():
    st = voice("three_envs").stages
    in_list, in_task = gv.envelope_orders(st)
    assert [st[i].kind for i in in_list] == [L.STAGE_MUL_ENV_AR, L.STAGE_MUL_ENVELOPE, L.STAGE_MUL_ENV_ASR]
    assert [st[i].kind for i in in_task] == [L.STAGE_MUL_ENV_ASR, L.STAGE_MUL_ENV_AR, L.STAGE_MUL_ENVELOPE]
    assert len(voice("nineteen").stages) == 19
    st = voice("comb_asr_pan").stages
    assert st[2].kind == L.STAGE_SAMPLE_DELAY and st[-1].kind == L.STAGE_PAN2


# ---- the first path draws what it drew ------------------------------------------------------------------------------------
# workload_digest of random_graph_voice(seed), seeds 0..31, as the module of the commit before random_voice_head was added
# gives them: that commit's tests/graph_voices.py (`git show <parent>:tests/graph_voices.py`) loaded as a module of its own
# and run through this same function.
PARENT_DIGESTS = [
    "bc4adde648bd25c9", "997a2c6f72cd5fc4", "7af7d51b26f9c85e", "3bd72530914da6e2",
    "02f50ee45ca09420", "f55b51b257076e9c", "05976b4e3e07cd8d", "7512477fdef16ffc",
    "6b7fb914926e79d0", "0c26ce33638e7f21", "a237f63e167bc2a1", "b3cdbc8ef4fc670f",
    "3fb35e4a44f6a2f9", "c055d70ef2f3fd4b", "58492b477f731569", "dc4a9c7f26f6439d",
    "f903c2cdeb079541", "1774aa6702a95946", "f69bedbd6d2cb6be", "b43d7fc3c3011951",
    "d2a7204aff5acb8e", "a9803cf39e96acef", "ff6b240183db2a44", "4c278d9447734a39",
    "6189f2cf65d44b24", "766778d0e0dae285", "2e320b4c9a77ac2a", "0bd88758b8f57ef8",
    "3083fcabc56dbe4c", "8bed29c57b45dabe", "d2ba17880092d2d0", "a069587c3e842dc9",
]


def workload_digest(w):
    """sha256 over the sizes, the stage descriptors, the constructor arrays and events.script (first 16 hex digits)"""
    h = hashlib.sha256()
    h.update(repr((w.n_voices, w.block_size, w.sample_type, w.out_channels)).encode())
    for s in w.stages:
        h.update(repr((s.kind, s.flags, s.delayed_changes_per_block, s.input, s.input2, s.ar_param)).encode())
    for k in sorted(w.ctor):
        a = np.ascontiguousarray(w.ctor[k], dtype=np.float64)
        h.update(repr((k, a.shape)).encode())
        h.update(a.tobytes())
    for block in sorted(w.events.script):
        for (sel, i, p, kind, f, d) in w.events.script[block]:
            h.update(repr((block, i, p, kind)).encode())
            h.update(np.ascontiguousarray(sel, dtype=np.uint32).tobytes())
            h.update(b"-" if f is None else np.ascontiguousarray(f, dtype=np.float64).tobytes())
            h.update(b"-" if d is None else np.ascontiguousarray(d, dtype=np.uint16).tobytes())
    return h.hexdigest()[:16]


def test_the_first_path_draws_what_it_drew():
    assert [workload_digest(gv.random_graph_voice(s)) for s in range(32)] == PARENT_DIGESTS


# ---- the second path: voices that combine the newer kinds, flags and calls ----------------------------------------------------
HEAD_SEEDS = list(range(gv.N_SEEDS))


def head_signature(knh, w, n=3):
    b = knh.VoiceBank(w.stages, n, w.sample_type, w.out_channels, L.MIX_LEFT_FOLD)
    if w.outs:
        b.connect_outputs(*w.outs)
    sig = b.debug_signature()
    b.close()
    return sig


def test_every_seed_has_a_head_voice():
    """No seed is skipped: a draw that is silent, not finite or too long is drawn again inside the generator."""
    for s in HEAD_SEEDS:
        w = gv.random_voice_head(s)
        assert 6 <= len(w.stages) <= gv.HEAD_MAX_STAGES and w.attempt < gv.HEAD_ATTEMPTS
        assert w.n_voices in gv.HEAD_VOICE_COUNTS and w.block_size in gv.HEAD_BLOCK_SIZES
        assert (w.sample_type == L.F64) == (s % 3 == 0)
        assert w.reference.voices.shape[0] == gv.HEAD_BLOCKS


@pytest.mark.parametrize("seed", HEAD_SEEDS)
def test_head_voice_is_accepted_and_its_signature_is_the_restatement(knh, seed):
    """debug_signature() of an uninitialised bank is what the Python restatement spells: the characters ('M' 'k' for OscWt,
    'b' 'j' 'l' for the envelope sources among them), the slots, the ":l,r" of two connected outputs."""
    w = gv.random_voice_head(seed)
    st = w.stages
    sig = head_signature(knh, w)
    assert sig == gv.expected_signature(st, w.outs)
    assert ("@" in sig) == (not w.info.chain)
    if w.info.chain:
        return
    parsed, n_slots = gv.parse_signature(sig)
    plan, want_slots = gv.slot_plan(st, w.outs)
    assert [(a, b, o) for (_, _, a, b, o) in parsed] == plan and n_slots == want_slots
    assert [c for (c, _, _, _, _) in parsed] == [gv.stage_char(s) for s in st]
    written = [o for (_, _, _, _, o) in parsed]
    assert gv.overwritten_live_signals(st, written) == [], sig
    if w.outs:  # neither output's slot is written again behind its node
        l, r = gv.signature_outputs(sig)
        assert (l, r) == (written[w.outs[0]], written[w.outs[1]])
        for o in w.outs:
            assert written[o] not in written[o + 1:] or o == len(st) - 1, sig
    else:
        assert gv.signature_outputs(sig) is None
    for i, s in enumerate(st):  # an envelope source reads nothing
        if gv.is_env_source(s):
            assert parsed[i][2] == -1 and (parsed[i][3] == -1 or s.ar_param)


@pytest.mark.parametrize("seed", HEAD_SEEDS)
def test_lowered_oracle_renders_the_head_voice(seed):
    """All nine blocks, reassignments and restart included: finite, every output plane of every voice above 1e-4, and voices
    that finish where the seed has an envelope or a one-shot reader."""
    w = gv.random_voice_head(seed)
    ref = w.reference
    assert np.isfinite(ref.voices).all() and np.isfinite(ref.mix).all()
    planes = ref.voices if w.outs else ref.voices[:, None]
    assert planes.shape[1] == (2 if w.outs else 1)
    assert (np.abs(planes).max(axis=(0, -1)) > 1e-4).all()
    after = planes[gv.HEAD_RESTART_BLOCK:, :, w.restart_voices]
    assert (np.abs(after).max(axis=(0, -1)) > 1e-4).all(), "the restarted voices sound again"
    if any(s.kind in gv.ENVELOPES for s in w.stages) or any(s.kind == L.STAGE_BUFFER_READER for s in w.stages):
        assert (ref.done != gv.NOT_DONE).any(), f"seed {seed}: no voice finishes"
        assert ref.flags.any()


def head_coverage(seeds):
    """-> {seed: the set of what the seed's voice holds}, read off the voice itself and not off what the seed was given"""
    out = {}
    for s in seeds:
        w = gv.random_voice_head(s)
        st = w.stages
        have = set()
        if any(x.kind == L.STAGE_SIN_WT and x.flags & gv.WT for x in st):
            have.add("oscwt")
            flagged = sum(bool(x.flags & gv.WT) for x in st)
            one_table = w.wavetables[1] == ["one"]
            others = any(gv.stage_char(x) in "WR" for x in st)
            if flagged == 1 and one_table and w.sample_type == L.F32:
                have.add("wt_lds missed for a W" if others else "wt_lds")
            have.add("oscwt " + w.info.oscwt)
        if any(gv.is_env_source(x) for x in st):
            kinds = {x.kind for x in st if gv.is_env_source(x)}
            beside = {x.kind for x in st if x.kind in gv.ENVELOPES and not gv.is_env_source(x)}
            assert beside and not (beside & kinds), "a multiplying envelope of another kind beside the source"
            have.add("env_source")
            have.add(("env_source", min(kinds)))
            have.add("env_source feeds " + w.info.env_use.split(":")[0])
        if gv._count(st, gv.DELAYS) >= 2:
            have.add("delays")
            have.add(("delays", "chain" if w.info.chain else "graph", gv._count(st, gv.DELAYS)))
            assert len(w.restart_voices) > 0 and w.restart_block < gv.HEAD_BLOCKS
            a, _ = gv.operands(st)
            if any(x.kind in gv.DELAYS and x.input and a[i] != i - 1 for i, x in enumerate(st)):
                have.add("a delay reads a named signal")
            if any(x.kind in gv.DELAYS and a[i] >= 0 and st[a[i]].kind in gv.DELAYS for i, x in enumerate(st)):
                have.add("delays in series")
        for x in st:
            if x.kind in gv.MATH1_EXACT:
                have.add("math1")
                have.add(("math1", x.kind))
        if w.outs:
            assert min(w.outs) < len(st) - 1 and w.outs[0] != w.outs[1]
            have.add("connected")
            if max(w.outs) < len(st) - 1:  # the last stage's signal is read by nobody and no output: its slot is not held
                assert not any(s.kind in gv.ENVELOPES or s.kind == L.STAGE_BUFFER_READER for s in st[max(w.outs) + 1:])
                have.add("neither output is the last stage")
        if w.reassign:
            have.add("reassign")
        if w.info.chain:
            have.add("a plain chain")
        out[s] = have
    return out


def test_the_head_seeds_cover_the_combinations():
    """A condition on the default 32 seeds: each of the six features in at least 6 of them, each pair in at least 2 -- but
    for the one pair the library refuses: knh_bank_assign_buffers after init refuses a chain in which an envelope can mark a
    voice done, with or without ENV_SOURCE (include/knaster_hip.h; held on the device by
    tests/test_gpu_buffer_pool.py::test_refused_calls_after_init_change_nothing[envelope_behind]) --, wt_lds taken in at least 3 and missed for a 'W' in at
    least 3, and every variant the generator has at least once."""
    cov = head_coverage(range(32))
    count = lambda *items: sum(all(i in have for i in items) for have in cov.values())
    table = {f: count(f) for f in gv.HEAD_FEATURES}
    assert all(k >= 6 for k in table.values()), table
    pairs = {(f, g): count(f, g) for f, g in itertools.combinations(gv.HEAD_FEATURES, 2)}
    assert pairs.pop(("env_source", "reassign")) == 0
    assert all(not (w.reassign and any(s.kind in gv.ENVELOPES for s in w.stages)) for w in map(gv.random_voice_head, range(32)))
    assert all(k >= 2 for k in pairs.values()), pairs
    assert count("wt_lds") >= 3 and count("wt_lds missed for a W") >= 3
    once = ["oscwt " + x for x in gv.OSCWT_SETTINGS] + ["env_source feeds " + x for x in gv.ENV_SOURCE_USES] + \
           [("env_source", k) for k in gv.ENVELOPES] + [("math1", k) for k in gv.MATH1_EXACT] + \
           ["a delay reads a named signal", "delays in series", "a plain chain", "neither output is the last stage"]
    assert not [x for x in once if count(x) < 1]
    # two to KNH_MAX_DELAY_STAGES delays: the small counts, and as many as sixteen stages hold -- a plain chain of an OscWt,
    # twelve delays, a Math1 function and the limiter, and graphs of seven or more (every seed is restarted)
    drawn = {x[1:] for have in cov.values() for x in have if isinstance(x, tuple) and x[0] == "delays"}
    assert {2, 3, 4} <= {k for _, k in drawn}
    assert max(k for shape, k in drawn if shape == "chain") == 12 and max(k for shape, k in drawn if shape == "graph") >= 8
    assert sum(k >= 7 for _, k in drawn) >= 3 and max(k for _, k in drawn) <= L.KNH_MAX_DELAY_STAGES
    ws = [gv.random_voice_head(s) for s in range(32)]
    assert {w.n_voices for w in ws} == set(gv.HEAD_VOICE_COUNTS) and {w.block_size for w in ws} == set(gv.HEAD_BLOCK_SIZES)
    assert {w.sample_type for w in ws} == {L.F32, L.F64}


def test_the_lowering_of_a_reassigned_reader_is_the_reader(oracle):
    """lower_for_oracle's own step, pinned against the oracle's BufferReader: Phasor + reader -> Svf with the reader lowered to
    a per-voice bank input fed by PoolReaders (forced by a reassignment that is never reached) is, bit for bit, the voice the
    oracle renders with the reader in it."""
    n, bs = 5, 48
    st = [Stage(L.STAGE_PHASOR), Stage(L.STAGE_BUFFER_READER), Stage(L.STAGE_WR_MUL), Stage(L.STAGE_MATH_ADD, input=1, input2=2), Stage(L.STAGE_SVF)]
    v = np.arange(n, dtype=np.float64)
    w = gv.configs.Workload("lowered_reader", st, n, bs, L.F32, 1)
    w.ctor = {0: (200.0 + 10.0 * v).reshape(n, 1), 1: np.stack([2.0 + 0.1 * v, v % 2, np.zeros(n)], axis=1), 2: np.full((n, 1), 0.7),
              4: np.tile([0.0, 900.0, 1.0, 0.0], (n, 1))}
    buf = gv.head_pool_buffers()[0]
    w.buffer, w.pool, w.links, w.outs, w.wavetables, w.reassign = (1, buf[0], buf[1]), None, {}, None, None, {}
    u = np.arange(n, dtype=np.uint32)

    def events(block, bank):
        if block == 1:
            bank.param_apply_many(u, 1, 0, L.VALUE_FLOAT, 1.5 + 0.05 * v)
            bank.param_apply_many(u, 2, 0, L.VALUE_FLOAT, np.full(n, 0.4))
        if block == 5:  # (the one-shot readers have run out in block 4)
            bank.param_apply_many(u, 1, 5, L.VALUE_TRIGGER)
    w.events = events
    direct = gv.oracle_run(oracle, w, 6)
    w.buffer, w.pool, w.reassign = None, (1, [buf], np.zeros(n, dtype=np.uint32)), {99: None}
    planes = gv.lower_for_oracle(w)
    assert [s.kind for s in planes[0].stages[1:3]] == [L.STAGE_INPUT, L.STAGE_MUL_CONST] and planes[0].in_channels == n
    assert planes[0].smap == [0, 2, 3, 4, 5] and planes[0].stages[4].input2 == 3
    o = gv.HeadOracle(oracle, w)
    for b in range(6):
        events(b, o)
        mix, voices, flags, done = o.process_block()
        assert_bit_equal(voices, direct[0][b], f"block {b} per-voice")
        assert_bit_equal(mix, direct[1][b], f"block {b} mix")
        np.testing.assert_array_equal(done, direct[3][b])
    o.close()
    assert (direct[3] != gv.NOT_DONE).any()


def test_the_lowering_maps_flags_indices_and_outputs():
    """WAVETABLE dropped, ENV_SOURCE as env_source_cases.twin() spells it, one plane per connected output cut behind its node."""
    w = gv.random_voice_head(2)  # OscWt under an audio-rate freq, an Envelope source with wrappers, connected outputs
    planes = gv.lower_for_oracle(w)
    assert len(planes) == 2 and sorted(p.end for p in planes)[1] == len(w.stages)
    for p in planes:
        assert not any(s.flags & (gv.WT | gv.ES) for s in p.stages)
        assert sum(s.kind == L.STAGE_INPUT for s in p.stages) == sum(gv.is_env_source(s) for s in w.stages[:p.end])
        for i, s in enumerate(w.stages[:p.end]):
            t = p.stages[p.smap[i]]
            assert t.kind == s.kind and t.ar_param == s.ar_param and t.delayed_changes_per_block == s.delayed_changes_per_block
            for mine, theirs in ((s.input, t.input), (s.input2, t.input2)):
                assert (theirs == 0) == (mine == 0) and (mine == 0 or theirs - 1 == p.smap[mine - 1])
            if gv.is_env_source(s):
                assert p.stages[p.smap[i] - 1].kind == L.STAGE_INPUT and t.input == 0


@pytest.mark.parametrize("seed", [1, 2, 4, 10, 14, 19])
def test_head_kernel_compiles_for_gfx950(knh, jit_compile_check, seed):
    """The fused kernel of a head voice in its own sample type: an OscWt under AR_FREQ beside an envelope source, connected
    outputs, eight delays in a graph, four delays, a pooled reader, a plain chain with twelve delays."""
    w = gv.random_voice_head(seed)
    sig = head_signature(knh, w)
    p = subprocess.run([CHECK, sig] + (["f64"] if w.sample_type == L.F64 else []), cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=900)
    assert p.returncode == 0, f"seed {seed} {sig}: rc {p.returncode}: {p.stdout.decode(errors='replace')[-600:]}"
