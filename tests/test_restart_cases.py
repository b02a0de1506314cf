"""The premise of every case of tests/restart_cases.py, on the CPU oracle alone: for EVERY restarted voice the voice that
goes on and the freshly constructed voice differ in the compared blocks -- otherwise a bank that ignored the restart would pass
tests/test_gpu_restart.py.  No restarted voice is exempt (arguments B differ from A for every voice)."""
import numpy as np
import pytest

import restart_cases as rc


@pytest.mark.parametrize("name,rname", rc.PAIRS)
def test_continuing_and_fresh_voice_differ_for_every_restarted_voice(oracle, name, rname):
    case = rc.CASES[name]
    exp = rc.oracle_expected(oracle, name, rname)
    r = sorted(set(case.r_sets[rname]))
    cont, fresh = np.stack(exp.cont), np.stack(exp.fresh)        # [block, voice, frame]
    differs = (cont != fresh).any(axis=(0, 2))
    assert differs[r].all(), f"{name}/{rname}: voices {[v for v in r if not differs[v]]} show nothing"
    assert np.isfinite(fresh).all() and np.isfinite(cont).all()
    assert np.abs(fresh[:, r]).max() > 1e-6, "the restarted voices are silent"
    # the expected rows are the fresh bank's on R and bank A's everywhere else
    for j, (v, _d) in enumerate(exp.after):
        np.testing.assert_array_equal(v[r], exp.fresh[j][r])
        rest = np.setdiff1d(np.arange(case.n), r)
        np.testing.assert_array_equal(v[rest], exp.cont[j][rest])


@pytest.mark.parametrize("name", [n for n in rc.CASES if n.startswith("c3_")])
def test_c3_voices_had_reported_done_before_the_boundary(oracle, name):
    """The pattern the restart serves: the envelope reports done, the host starts the next note on a new node."""
    exp = rc.oracle_expected(oracle, name, "all")
    done = np.stack([d for _v, d in exp.before])
    assert (done != rc.NOT_DONE).any(axis=0).all()
    assert (np.stack([d for _v, d in exp.after]) != rc.NOT_DONE).any(), "no voice finishes its next note in the compared blocks"


@pytest.mark.parametrize("name", ["sample_delay_f32", "sample_delay_f64"])
def test_a_restarted_delay_is_silent_for_its_first_100_samples(oracle, name):
    """A new SampleDelay's ring is zeros: silence for the 100 samples of the delay, then the new oscillator; the voice that goes
    on reads what its ring held."""
    exp = rc.oracle_expected(oracle, name, "ring")
    r = rc.R_SETS["ring"]
    fresh = np.concatenate(exp.fresh, axis=1)[r]
    cont = np.concatenate(exp.cont, axis=1)[r]
    assert (fresh[:, :100] == 0).all() and (fresh[:, 101:164] != 0).any(axis=1).all()
    assert (cont[:, :100] != 0).any(axis=1).all()


def test_case_table_shapes():
    assert rc.N == 130 and sorted(set(rc.R_SETS["dup"])) != rc.R_SETS["dup"]
    assert {c.bs for c in rc.CASES.values() if c.name.startswith("c3_")} == {64, 100}
    for c in rc.CASES.values():
        assert c.k * c.bs >= 192 or not c.name.startswith(("sample", "allpass")), "restart after the rings have wrapped"
        for s, b in c.ctor_b.items():
            a = np.asarray(c.ctor_a[s], dtype=np.float64).reshape(c.n, -1)
            assert (a != np.asarray(b, dtype=np.float64).reshape(c.n, -1)).any(axis=1).all(), f"{c.name} stage {s}: B equals A for some voice"
