"""CPU: the scripts of tests/call_walks.py before any engine sees them -- make_script is
deterministic and stays inside its mode's alphabet and bookkeeping; the census that keeps the walks
from hiding a gap holds over exactly the seeds tests/test_gpu_call_walks.py runs; and every
single-engine script leaves the oracle in one state with and without its observe ops (an ask mode's
with and without its asks too).  The ask modes' census counts the ordered pairs with at least one ask,
and their conditions on the references ("the asks matter") are checked here before any GPU sees them.
tests/CALL_WALKS.md holds the numbers."""
import hashlib

import numpy as np
import pytest

from tests import call_walks as cw

ALL_MODES = list(cw.MODES)
ASK_MODES = [m for m, s in cw.MODES.items() if s.get("ask")]
PURITY_MODES = [m for m, s in cw.MODES.items() if s["kind"] == "single" and s.get("purity", True)]
# ops that change no state of the model: an observe after them reads what the op before them left
STATELESS = ("observe", "execute", "m_execute", "set_timing", "refuse", "g_run_refused") + cw.ASKS


# sha256 over repr(make_script(mode, s)) for s in range(SEEDS[mode]), first 16 hex digits: of the 16
# modes that existed before IDENTS was frozen, taken from the module as it stood then, and of the 8
# modes of the second round, taken from the module as it stood before the ask modes were added
FROZEN = {
    "reuse_fused": (12, "551ed103eb57069c"), "reuse_no_spec": (14, "f72724523517a58b"),
    "reuse_no_pick_fuse": (12, "ca78c028a041468c"), "pregen": (13, "3d7ccbc5272ae295"), "unfused": (13, "709b0847a262bc79"),
    "slot_loop": (28, "8e86eba3f0bbe99a"), "slot_loop_lean": (25, "96775fc24c2ccc39"), "phased": (18, "80c970bb6c9bd8a3"),
    "terms_cum": (15, "18cae7079647691b"), "device_brick": (16, "bf08661dfbc87845"), "group_reuse": (5, "93118209f64a2177"),
    "group_pregen": (4, "46c1002411977521"), "group_mixed": (18, "d678ad55031ad205"),
    "group_mixed_compact": (8, "668f442d07b844f8"), "ranks_partials": (4, "f250a29a5c3c51d4"),
    "ranks_gather": (4, "9ba975cd67205712"),
    "request_reuse": (16, "89c9ad6100992805"), "request_pregen_cum": (25, "2a5120ce2933363e"),
    "scene_linear": (20, "d411d0c74c429add"), "scene_brick": (16, "a4046441faad04e5"),
    "group_request": (20, "b8698f79b725b6a0"), "group_serve_reuse": (12, "c1d1b3739aa60c81"),
    "group_serve_pregen": (21, "5d6ff670105ca5eb"), "group_serve_shelf": (22, "b93f86905583d098"),
}
FIRST_ROUND = list(FROZEN)[:16]


@pytest.mark.parametrize("mode", list(FROZEN))
def test_existing_scripts_have_not_moved(mode):
    seeds, digest = FROZEN[mode]
    # the first round's idents were the modes' indices in sorted order, the second round's 16 .. 23 as listed
    ident = sorted(FIRST_ROUND).index(mode) if mode in FIRST_ROUND else list(FROZEN).index(mode)
    assert cw.SEEDS[mode] == seeds and cw.IDENTS[mode] == ident
    h = hashlib.sha256()
    for s in range(seeds):
        h.update(repr(cw.make_script(mode, s)).encode())
    assert h.hexdigest()[:16] == digest
    new = {k for m in cw.MODES if m not in FROZEN for k in cw.kinds_of(m)} - {k for m in FROZEN for k in cw.kinds_of(m)}
    assert not (new & set(cw.kinds_of(mode))), sorted(new & set(cw.kinds_of(mode)))


def test_new_modes_have_idents_from_16_up():
    new = [m for m in cw.MODES if m not in FIRST_ROUND]
    assert set(cw.IDENTS) == set(cw.MODES) and all(cw.IDENTS[m] >= 16 for m in new)
    assert len(set(cw.IDENTS.values())) == len(cw.IDENTS)


def test_ask_modes_have_idents_from_24_up():
    new = [m for m in cw.MODES if m not in FROZEN]
    assert new == ASK_MODES and list(cw.MODES)[:24] == list(FROZEN)
    assert set(cw.IDENTS) == set(cw.MODES) and all(cw.IDENTS[m] >= 24 for m in new)
    assert len(set(cw.IDENTS.values())) == len(cw.IDENTS)


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
    if mode in ASK_MODES:
        return ask_census(mode, ss, kinds, changing, want)
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


def ask_census(mode, ss, kinds, changing, want):
    """An ask mode's census.  Pairs of two old kinds are the old modes' business: (the ordered pairs
    with at least one ask that are missing; the state-changing old kinds that no ask follows before
    an observe, and the asks that no state-changing old kind follows before one; what else the mode
    must show: every chomp_refused reason its book can reach, in ask_ranks the refused
    stomp_chomp_create, and in ask_group a serve that leaves the live descent's member unturned and
    one that turns it)."""
    asks = [k for k in kinds if k in cw.ASKS]
    want = {(a, b) for a, b in want if a in asks or b in asks}
    followed = set()
    for s in ss:
        for i, op in enumerate(s):
            then = asks if op[0] in changing else changing if op[0] in asks else ()
            for nxt in s[i + 1:]:
                if nxt[0] == "observe":
                    break
                if nxt[0] in then:
                    followed.add(op[0])
                    break
    lacking = set()
    if "chomp_refused" in kinds:
        reasons = set(cw.CHOMP_REFUSALS) - (set() if cw.MODES[mode].get("request") else {"stale_model"})
        lacking |= reasons - {op[1] for s in ss for op in s if op[0] == "chomp_refused"}
    if cw.MODES[mode]["kind"] == "ranks":      # the refusal the mode adds: stomp_chomp_create on a sharded engine
        if not any(op[:2] == ("refuse", "chomp_create") for s in ss for op in s):
            lacking.add("refuse(chomp_create)")
    if cw.MODES[mode]["kind"] == "group":
        served = set()
        for s in ss:
            book = cw.new_book(mode)
            for op in s:
                if op[0] == "g_serve" and cw.descent_allows(book.descent, "chomp_get"):
                    served.add("short" if op[2] <= cw.DESCENT_MEMBER else "turning")
                book.apply(op)
        lacking |= {"a short g_serve under a live descent", "a turning g_serve under a live descent"} - {
            f"a {k} g_serve under a live descent" for k in served}
    return (want - pairs_of(ss), (set(changing) | set(asks)) - followed, lacking)


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


@pytest.mark.parametrize("mode", ASK_MODES)
def test_the_asks_matter(mode):
    # the conditions every ask mode asserts before it touches a device, on the references alone
    cw.assert_asks_matter(mode)


def run_on_oracle(mode, script):
    made = cw.MODES[mode]["make"]()
    if cw.MODES[mode].get("request"):
        cw.assert_attach_matters(made)
    if cw.MODES[mode].get("scene"):      # the field the scene's static layer gives
        made.sdf = cw.po.sdf_build_objects(made.grid, cw.scene_static_layer(made, 0))[0]
    pair = cw.Pair(made, engine=None, threads=cw.MODES[mode].get("threads", 1))
    cw.replay(mode, script, pair)
    return pair.full_state()


@pytest.mark.parametrize("mode", PURITY_MODES)
def test_observe_is_pure_on_the_oracle(mode):
    # the oracle held to itself: as written, and with the observe ops removed (no script may raise
    # the binding's non-finite ValueError: replay would turn it into a failure)
    for seed in range(cw.SEEDS[mode]):
        script = cw.make_script(mode, seed)
        a = run_on_oracle(mode, script)
        others = [run_on_oracle(mode, [op for op in script if op[0] != "observe"])]
        if mode in ASK_MODES:     # and with the asks removed as well: the script stays valid without them
            others.append(run_on_oracle(mode, [op for op in script if op[0] not in ("observe",) + cw.ASKS]))
        for b in others:
            assert set(a) == set(b)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{mode} seed {seed} {k}")
                assert np.isfinite(a[k]).all(), (mode, seed, k)
