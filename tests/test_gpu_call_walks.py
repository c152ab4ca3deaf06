"""GPU: seeded walks over the public API (tests/call_walks.py) -- one script drives an engine, an
engine group with its single-engine twins, or two in-process ranks, and the CPU oracle.  Only what a
call returns is compared as the walk goes; state is read where the walk put an `observe`, not after
every call, so a stale pregen iteration, a dropped pending rollout or an unswapped row set that a
read would have repaired stays visible to the next call.  Every comparison is bitwise.  Each case
ends with a full observe of everything both sides define (groups and ranks: after a synchronize).

The ask modes put state queries, gradient queries and a CHOMP descent among those calls: each is
compared with its own CPU reference on the pair's current problem and field, and the oracle side never
hears of them, so an ask that touched the engine shows in what the next calls return.

tests/CALL_WALKS.md holds the alphabet, the modes, the census and what the walks found; the scripts
that showed a bug stand below the walks as named regression tests, and after them the literal scripts:
the padding-collision flag turned through a serve call, and a descent on a group member that a short
serve leaves alone and a full one makes stale.
"""
import numpy as np
import pytest

from stomp_motion_planner_icra2011_amd import engine as eng
from tests import call_walks as cw
from tests import rank_util as ru

pytestmark = pytest.mark.gpu

CASES = [(mode, seed) for mode in cw.MODES for seed in range(cw.SEEDS[mode])]


def lines(capfd, prefix):
    err = capfd.readouterr().err
    out = [l for l in err.splitlines() if l.startswith(prefix)]
    assert out, err
    return out


def make_pair(mode, monkeypatch, capfd):
    """The mode's pair, created under its environment; the path it names asserted from the
    engine's own STOMP_DEBUG_LEAN_PRINT lines."""
    spec = cw.MODES[mode]
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    for k, v in spec["env"].items():
        monkeypatch.setenv(k, v)
    threads = spec.get("threads", 1)
    if spec.get("ask"):     # on the references alone, before any device is touched
        cw.assert_asks_matter(mode)
    made = spec["make"]()
    capfd.readouterr()
    if spec["kind"] == "single":
        buf = None
        if spec.get("device_field"):
            buf = eng.DeviceBuffer(2 * made.grid.cells)
            eng.sdf_build_objects_device(made.grid, cw.scene_objects(made, False), buf.ptr)
            made.sdf = buf.to_numpy(np.uint16, tuple(made.grid.dims))
        if spec.get("request"):     # on the oracle alone, before any engine exists
            cw.assert_attach_matters(made)
        scene = stream = None
        if spec.get("scene"):
            # the field belongs to a scene on a stream it shares with the engine
            stream = eng.Stream()
            buf = eng.DeviceBuffer(2 * made.grid.cells)
            scene = eng.Scene(made.grid, buf.ptr, stream=stream.ptr)
            scene.set_static(cw.scene_static_layer(made, 0))
            assert scene.info()["stray"] == 0
            made.sdf = buf.to_numpy(np.uint16, tuple(made.grid.dims))
        e = eng.Engine(made, sdf_device_ptr=buf.ptr if buf else None, stream=stream.ptr if stream else None)
        got = lines(capfd, "stomp: model ")[-1:]
        pair = cw.Pair(made, e, threads=threads, field=buf, scene=scene, stream=stream,
                       brick=spec["env"].get("STOMP_SDF_LAYOUT") == "brick")
        if scene is not None:
            np.testing.assert_array_equal(made.sdf, pair.scene_field(0, 0), err_msg="the static layer against the oracle's build")
    elif spec["kind"] == "group":
        targets = spec["targets"]() if "targets" in spec else None
        pair = cw.GroupPair(made, threads=threads, targets=targets, **spec.get("group", {}))
        got = lines(capfd, "stomp: group ")
    else:
        ranks = ru.make_ranks(made, 2, spec["shard"], monkeypatch)
        got = lines(capfd, "stomp: model ")
        pair = cw.RankPair(made, ranks, threads=threads)
        assert [e.shard_mode for e in ranks] == [spec["shard"]] * 2 and [e.K_loc for e in ranks] == [64, 64]
    for piece in spec["expect"]:
        assert any(piece in l for l in got), (piece, got)
    if "chomp" in spec:     # the parameters of the mode's one CHOMP object
        pair.chomp_params = spec["chomp"]
    return pair


def walk(mode, script, monkeypatch, capfd, seed=None, after=None):
    """after(pair, i, op): called behind every op of the script (a literal test's own assertions)"""
    pair = make_pair(mode, monkeypatch, capfd)
    try:
        if after is None:
            cw.replay(mode, script, pair, seed)
        else:
            for i, op in enumerate(script):
                cw.replay(mode, [op], pair, seed, start=i)
                after(pair, i, op)
        cw.replay(mode, cw.final_ops(mode, script), pair, seed, start=len(script))
    finally:
        pair.close()


@pytest.mark.parametrize("mode,seed", CASES, ids=[f"{m}-{s}" for m, s in CASES])
def test_walk(monkeypatch, capfd, mode, seed):
    walk(mode, cw.make_script(mode, seed), monkeypatch, capfd, seed)


# ---------------------------------------------------------------------------- what the walks found
# The shortest scripts that show each bug (tests/CALL_WALKS.md, "What the walks found").

@pytest.mark.parametrize("mode", ["reuse_fused", "reuse_no_pick_fuse"])
def test_set_theta_before_a_reusing_iteration(monkeypatch, capfd, mode):
    # the extra rollout keeps the parameters it was added with (policy_improvement.cpp:446-449): after
    # set_theta they are not theta, and the reuse step must rank and re-base that row, not theta + 0.
    # The rollout launch that prices the candidates ahead took theta for it.  The first ranking of this
    # script keeps the extra rollout (the oracle's reuse_log: [7, 3, -1, 1, 6]).
    script = [("iterate", 1), ("set_theta", 503634), ("iterate", 2), ("observe", ("theta", "params", "noise")),
              ("run", 3, 2), ("set_theta", 96949), ("run", 5, 1)]
    walk(mode, script, monkeypatch, capfd)


@pytest.mark.parametrize("mode", ["pregen", "reuse_fused", "unfused"])
@pytest.mark.parametrize("fused", [("iterate", 2), ("run", 2, 2), ("optimize",)], ids=lambda op: op[0])
def test_extra_rollout_after_a_fused_iteration_is_priced_with_its_weight(monkeypatch, capfd, mode, fused):
    # runSingleIteration calls setRolloutCosts with the loop's weight (policy_improvement_loop.cpp:173),
    # so an addExtraRollouts after it prices with that weight, not with the 2 w of the step round before
    script = [("pi_get_rollouts", 1), ("pi_set_rollout_costs", 2), ("pi_improve_policy",), fused,
              ("pi_add_extra_rollout", None), ("observe", ("x_control",))]
    walk(mode, script, monkeypatch, capfd)


# ---------------------------------------------------------------------------- the padding flag through a serve
def test_serve_turns_the_padding_flag_both_ways(monkeypatch, capfd):
    # A queue alternating flag_pair's A (only its padding poses collide) and B (free): the slots'
    # padding-collision flags change at the turnovers (k_serve_flags) and the call's end brings the
    # last ones back to the three host copies.  flag_pair asserts on the oracle that the flag alone
    # decides A's result, so a flag that stayed behind shows: in the requests' results, in the
    # execute(member 0) of every slot straight after the serve (the engine's own copy), and in the
    # grouped run after them (the group's copy and the model's).
    A, B = 1, 2
    # A B A B, B A B A, ...: the slots of this group turn together, so the order flips every P requests
    which = tuple(A if (r + r // 4) % 2 == 0 else B for r in range(16))
    script = [("g_serve", 77, len(which), which)]
    script += [("m_execute", m, 300 + m, 2, 0) for m in range(4)]
    script += [("g_run", 7, 2)]

    def after(pair, i, op):
        if op[0] != "g_serve":
            return
        reqs, results = pair.served
        by_slot = {}
        for r, res in enumerate(results):
            by_slot.setdefault(res[0], []).append(which[r])
        turns = {(a, b) for seq in by_slot.values() for a, b in zip(seq, seq[1:])}
        print("requests per slot:", by_slot)
        assert (A, B) in turns and (B, A) in turns, by_slot
        assert all(A in seq and B in seq for seq in by_slot.values()) and len(by_slot) == 4, by_slot

    walk("group_serve_shelf", script, monkeypatch, capfd, after=after)


# ---------------------------------------------------------------------------- a descent under a serve
def test_descent_survives_a_short_serve(monkeypatch, capfd):
    # The descent borrows member 1's engine.  A serve of one request turns slot 0 alone: the descent
    # stays live and goes on bit for bit, its steps enqueued behind the serve with no wait.  A serve of
    # P requests turns every slot: step, optimize and get are each refused for the retarget, get writes
    # nothing, and a reset from member 1's theta (the oracle's, after the slot's last request) brings
    # the descent back.
    P = 4
    script = [("chomp_reset", 2, 41), ("g_serve", 5, 1), ("chomp_step", 2),
              ("chomp_get", ("trajectory", "collision_increments", "potentials", "cost")),
              ("g_serve", 6, P), ("chomp_refused", "stale_target"), ("chomp_reset", 1, None),
              ("chomp_get", ("trajectory", "distances", "costs", "collision_free"))]
    book = cw.new_book("ask_group")
    states = []
    for op in script:
        book.apply(op)
        states.append(book.descent)
    assert states == ["fresh", "fresh", "stepped", "stepped", "stale_target", "stale_target", "fresh", "fresh"], states
    walk("ask_group", script, monkeypatch, capfd)
