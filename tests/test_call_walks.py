"""CPU: the scripts of tests/call_walks.py before any engine sees them -- make_script is
deterministic and stays inside its mode's alphabet and bookkeeping; the census that keeps the walks
from hiding a gap holds over exactly the seeds tests/test_gpu_call_walks.py runs; and every
single-engine script leaves the oracle in one state with and without its observe ops.
tests/CALL_WALKS.md holds the numbers."""
import numpy as np
import pytest

from tests import call_walks as cw

ALL_MODES = list(cw.MODES)
PURITY_MODES = [m for m, s in cw.MODES.items() if s["kind"] == "single" and s.get("purity", True)]
# ops that change no state of the model: an observe after them reads what the op before them left
STATELESS = ("observe", "execute", "m_execute", "set_timing", "refuse", "g_run_refused")


def scripts(mode, seeds=None):
    return [cw.make_script(mode, s) for s in range(cw.SEEDS[mode] if seeds is None else seeds)]


def pairs_of(script_list):
    return {(a[0], b[0]) for s in script_list for a, b in zip(s, s[1:])}


def census(mode, seeds=None):
    """(missing ordered pairs, state-changing kinds never followed by another state-changing op
    without an observe between, kinds observe never follows), from the scripts alone."""
    ss = scripts(mode, seeds)
    kinds = cw.kinds_of(mode)
    changing = [k for k in kinds if k not in STATELESS]
    want = {(a, b) for a in kinds for b in kinds} - set(cw.impossible_pairs(mode))
    unobserved = set()
    for s in ss:
        for i, op in enumerate(s):
            if op[0] not in changing:
                continue
            for nxt in s[i + 1:]:
                if nxt[0] == "observe":
                    break
                if nxt[0] in changing:
                    unobserved.add(op[0])
                    break
    seen = pairs_of(ss)
    return (want - seen, set(changing) - unobserved, {k for k in kinds if (k, "observe") not in seen})


@pytest.mark.parametrize("mode", ALL_MODES)
def test_make_script_is_deterministic_and_valid(mode):
    kinds = set(cw.kinds_of(mode))
    for seed in (0, 1, cw.SEEDS[mode] - 1):
        a, b = cw.make_script(mode, seed), cw.make_script(mode, seed)
        assert a == b and len(a) == cw.length_of(mode)
        assert {op[0] for op in a} <= kinds, sorted({op[0] for op in a} - kinds)
        book = cw.new_book(mode)
        for op in a:
            book.apply(op)          # asserts the op against the bookkeeping
        for op in cw.final_ops(mode, a):
            book.apply(op)
    assert cw.make_script(mode, 0) != cw.make_script(mode, 1)
    assert len(cw.make_script(mode, 0, 7)) == 7


@pytest.mark.parametrize("mode", ALL_MODES)
def test_census(mode):
    missing, never_unobserved, never_observed = census(mode)
    assert not missing, sorted(missing)
    assert not never_unobserved, sorted(never_unobserved)
    assert not never_observed, sorted(never_observed)
    # exactly the listed pairs are missing: none of them occurs
    listed = set(cw.impossible_pairs(mode))
    assert not (listed & pairs_of(scripts(mode))), sorted(listed & pairs_of(scripts(mode)))
    # and the count of seeds is the smallest that closes the census
    assert any(census(mode, cw.SEEDS[mode] - 1)), "one seed fewer closes the census too: lower call_walks.SEEDS"


def run_on_oracle(mode, script):
    pair = cw.Pair(cw.MODES[mode]["make"](), engine=None, threads=cw.MODES[mode].get("threads", 1))
    cw.replay(mode, script, pair)
    return pair.full_state()


@pytest.mark.parametrize("mode", PURITY_MODES)
def test_observe_is_pure_on_the_oracle(mode):
    # the oracle held to itself: as written, and with the observe ops removed (no script may raise
    # the binding's non-finite ValueError: replay would turn it into a failure)
    for seed in range(cw.SEEDS[mode]):
        script = cw.make_script(mode, seed)
        a = run_on_oracle(mode, script)
        b = run_on_oracle(mode, [op for op in script if op[0] != "observe"])
        assert set(a) == set(b)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{mode} seed {seed} {k}")
            assert np.isfinite(a[k]).all(), (mode, seed, k)
