"""The oracle twin of an envelope source (tests/env_source_cases.py: INPUT on a plane of ones, then the multiplying form)
pinned against arithmetic that does not pass through the oracle: a numpy restatement of EnvAsr::next_sample and
EnvAr::next_sample (envelopes.rs:52-81 / :205-233), their setters' rates (:135-151) and triggers (:113-133), in f32 and f64.
8 voices, 4 blocks of 64 frames.  `1.0 * e` is `e`: the twin's per-voice output equals the restatement bit for bit, and its
done frames are the frames at which the restated machine stops.

It also asserts what the twin construction relies on: the twin's Mul node depends on no node but the envelope, so the envelope
keeps its place in the reference's task order -- seen through the one thing the order decides, whose mark_done a voice
reports when two envelopes finish in one block (the last in task order, graph_gen.rs:196-200)."""
import numpy as np
import pytest

import env_source_cases as ec
from helpers import assert_bit_equal
from knaster_amd import _lib as L
from knaster_amd.bank import Stage

N, BS, BLOCKS = 8, 64, 4
STOPPED, ATTACKING, SUSTAINING, RELEASING = range(4)


class Env:
    """EnvAsr (ar=False) or EnvAr (ar=True) of one voice, every operation a scalar operation of dtype F in source order"""

    def __init__(self, F, attack, release, ar, sr=ec.SR):
        self.F, self.ar = F, ar
        one = F(1)
        atk, rel = F(attack), F(release)
        self.attack_rate = one if atk == F(0) else one / (atk * F(sr))    # init, envelopes.rs:135-151 / :268-284
        self.release_rate = one if rel == F(0) else one / (rel * F(sr))
        self.state, self.t, self.scale = STOPPED, F(0), one

    def t_restart(self):
        self.state = ATTACKING                                            # trig_start: from the current t

    def t_release(self):                                                  # EnvAsr only, :113-128
        if self.state == ATTACKING:
            self.scale, self.state, self.t = self.t, RELEASING, self.F(1)
        elif self.state == SUSTAINING:
            self.scale, self.state, self.t = self.F(1), RELEASING, self.F(1)

    def next_sample(self):
        """-> (sample, stopped at this sample)"""
        F = self.F
        if self.state == ATTACKING:
            out = self.t                                                  # linear attack
            self.t = F(self.t + self.attack_rate)
            if self.t >= F(1):
                if self.ar:
                    self.scale, self.state, self.t = F(1), RELEASING, F(1)
                else:
                    self.state = SUSTAINING
            return out, False
        if self.state == SUSTAINING:
            return F(1), False
        if self.state == RELEASING:
            t = self.t
            out = F(F(t * F(t * t)) * self.scale)                          # powi(3) by squaring, then * release_scale
            self.t = F(t - self.release_rate)
            if self.t <= F(0):
                self.state, self.t = STOPPED, F(0)
                return out, True
            return out, False
        return F(0), False


def times(n):
    """attack 5 .. 40 samples, release 12 .. 110 samples: the long releases still run at the restart of block 2"""
    v = np.arange(n)
    return np.stack([(5.0 + 5.0 * v) / ec.SR, (12.0 + 14.0 * v) / ec.SR], axis=1)


class Machines:
    """the call surface of the traffic, on N restated envelopes"""

    def __init__(self, envs, stage, restart, release):
        self.envs, self.stage, self.restart, self.release = envs, stage, restart, release

    def param_apply_many(self, voices, stage, param, kinds, fvalues=None, ivalues=None, delays=None):
        if stage != self.stage:
            return
        for v in voices:
            if param == self.restart:
                self.envs[v].t_restart()
            elif param == self.release:
                self.envs[v].t_release()

    def block(self, F):
        out = np.zeros((len(self.envs), BS), dtype=F)
        done = np.full(len(self.envs), ec.NOT_DONE, dtype=np.uint32)
        for v, e in enumerate(self.envs):
            for i in range(BS):
                out[v, i], stopped = e.next_sample()
                if stopped:
                    done[v] = i
        return out, done


@pytest.mark.parametrize("st,F", [(L.F32, np.float32), (L.F64, np.float64)], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["asr", "ar"])
def test_twin_of_a_lone_source_equals_the_restated_envelope(oracle, st, F, kind):
    ar = kind == "ar"
    stages = [Stage(L.STAGE_MUL_ENV_AR if ar else L.STAGE_MUL_ENV_ASR, flags=ec.ES)]
    tw, smap = ec.twin(stages)
    assert [s.kind for s in tw] == [L.STAGE_INPUT, stages[0].kind] and tw[1].flags == 0 and smap == [1]
    t = times(N)
    if ar:
        t[:, 0] = (30.0 + 9.0 * np.arange(N)) / ec.SR  # (an EnvAr releases by itself: longer attacks keep some attacking in block 1)

    def traffic(bank, block, n):
        v = np.arange(n, dtype=np.uint32)
        if ar:
            if block == 0:
                bank.param_apply_many(v, 0, 2, ec.KT)
            if block == 2:
                bank.param_apply_many(v[3:], 0, 2, ec.KT)   # t_restart while Releasing (long releases) and after the stop
        else:
            if block == 0:
                bank.param_apply_many(v, 0, 3, ec.KT)
                bank.param_apply_many(v[6:], 0, 2, ec.KT)   # t_release right behind the start: from Attacking at t = 0
            if block == 1:
                bank.param_apply_many(v[:6], 0, 2, ec.KT)   # t_release from Sustaining (attacks of up to 30 samples are over)
            if block == 2:
                bank.param_apply_many(v[3:], 0, 3, ec.KT)   # t_restart while Releasing, and after the stop
            if block == 3:
                bank.param_apply_many(v[4:], 0, 2, ec.KT)   # t_release from Attacking (attacks of 25+ samples from t > 0) and Sustaining

    bank = ec.TwinBank(oracle, stages, N, st, {0: t}, BS, want_mix=False)
    ref = Machines([Env(F, a, r, ar) for a, r in t], 0, 2 if ar else 3, None if ar else 2)
    stops = 0
    for b in range(BLOCKS):
        traffic(bank, b, N)
        traffic(ref, b, N)
        _, voices, flags, done = bank.process_block()
        want, want_done = ref.block(F)
        assert_bit_equal(np.asarray(voices), want, f"block {b}", strict_zero=True)
        np.testing.assert_array_equal(done, want_done, f"block {b}: done frames")
        assert bool(flags & L.FLAG_ANY_DONE) == bool((want_done != ec.NOT_DONE).any())
        stops += int((want_done != ec.NOT_DONE).sum())
    bank.close()
    assert stops >= N // 2


@pytest.mark.parametrize("st,F", [(L.F32, np.float32), (L.F64, np.float64)], ids=["f32", "f64"])
@pytest.mark.parametrize("name,src,amp,last", [("pitch", 0, 4, "amp"), ("gain", 2, 1, "src")])
def test_the_envelope_keeps_its_place_in_the_task_order(oracle, st, F, name, src, amp, last):
    """An EnvAr source and a multiplying EnvAsr that stop in the same block, at different frames.  In the pitch chain the
    source comes first in the reference's task order (the chain hangs on it) and the voice reports the amplitude envelope's
    frame; in the gain graph the source's subgraph hangs on a parameter edge, is ordered after the sound, and the voice reports
    the source's frame.  The twin must agree with both."""
    case = ec.CASES[name]
    ctor = case.ctor(N)
    v = np.arange(N)
    ctor[src] = np.stack([np.full(N, 20.0 / ec.SR), (120.0 + v) / ec.SR], axis=1)        # stops near frame 140 + v
    ctor[amp] = np.stack([np.full(N, 10.0 / ec.SR), (20.0 + 3.0 * v) / ec.SR], axis=1)   # released at frame 128: stops near 148 + 3 v

    def traffic(bank, block, n):
        vv = np.arange(n, dtype=np.uint32)
        if block == 0:
            bank.param_apply_many(vv, src, 2, ec.KT)
            bank.param_apply_many(vv, amp, 3, ec.KT)
        if block == 2:
            bank.param_apply_many(vv, amp, 2, ec.KT)

    bank = ec.TwinBank(oracle, case.stages, N, st, ctor, BS, want_mix=False)
    m_src = Machines([Env(F, a, r, True) for a, r in ctor[src]], src, 2, None)
    m_amp = Machines([Env(F, a, r, False) for a, r in ctor[amp]], amp, 3, 2)
    for b in range(3):
        for x in (bank, m_src, m_amp):
            traffic(x, b, N)
        _, _, _, done = bank.process_block()
        _, d_src = m_src.block(F)
        _, d_amp = m_amp.block(F)
    assert (d_src != ec.NOT_DONE).all() and (d_amp != ec.NOT_DONE).all() and (d_src != d_amp).sum() >= N - 1
    np.testing.assert_array_equal(done, d_amp if last == "amp" else d_src)
    bank.close()
