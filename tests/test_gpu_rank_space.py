"""The K-sharded iteration beyond the PR2 fixture (tests/SHARDED_RANKS.md): odd worlds, several
64-rollout blocks per rank, every row-tile kernel in its sharded phases, N at both ends of the
engine's range, J from 1 to 32, reuse at the shard edges, the cost options, fields, the calls between
iterations and the refusals -- the model zoo (tests/model_zoo.py) against the CPU oracle, bit for bit.

The ranks are W engines of one process on device 0, one host thread each (tests/rank_util.py); every
rank must reproduce its slice of the one oracle of the whole K.  Every case asserts what creation
chose (the engine's `stomp: model` line, shard_mode, K_loc, first) and what its inputs reach (the
censuses, on the oracle's arrays alone) before it compares; every comparison is assert_array_equal.
"""
import numpy as np
import pytest

from oracle import pyoracle as po
from stomp_motion_planner_icra2011_amd import engine as eng
from stomp_motion_planner_icra2011_amd import problem as pb
from tests import model_zoo as mz
from tests import rank_util as ru
from tests.pi_steps_util import zoo_problem
from tests.test_model_space import N_EXTREME_MODELS, N_EXTREMES

pytestmark = pytest.mark.gpu

MODES = ru.MODES


def assert_ragged_columns(p, tail=3):
    # the flat-column tiles are four wide: J N = 3 (mod 4) ends in a tile of three columns, and
    # N % 4 != 0 makes tiles cross joint boundaries
    assert (p.J * p.N) % 4 == tail and p.N % 4 != 0, (p.J, p.N)


# ---------------------------------------------------------------------------- 1. worlds and blocks
WORLDS = [(2, 128), (3, 192), (5, 320), (3, 576), (6, 384), (2, 512), (2, 640)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("world,K", WORLDS)
def test_worlds_and_blocks_bitwise(monkeypatch, capfd, world, K, mode):
    # chain5, N = 39: J N = 195 columns.  The block partials of rank r are blocks r nb_loc .. of
    # d_psum_all / d_u_all; (3, 576) has nine of them, three per rank
    p = zoo_problem("chain5", K, 0)
    assert_ragged_columns(p)
    body = "slot loop" if (world, K) == (2, 512) else None    # 257 rollouts: more than compute units
    recs, orecs = ru.run_case(p, world, mode, monkeypatch, capfd, body=body, key=("worlds", K))
    # the probabilities compared were the rank's K_loc rows, not all K
    assert all(rec[-1]["probabilities"].shape == (K // world, p.J, p.N) for rec in recs)


# ---------------------------------------------------------------------------- 2. the row tiles' phases
TILE_K = [64, 256, 320, 1024, 1088, 2048, 2112, 4096]
TILE_CASES = [(n, K, False) for n in ("chain5", "hand9") for K in TILE_K] + [("chain5", 320, True), ("chain5", 1088, True)]


@pytest.mark.parametrize("name,K,cumulative", TILE_CASES)
def test_row_tile_kernels_in_their_sharded_phases_bitwise(monkeypatch, capfd, name, K, cumulative):
    # one device running the MINMAX / PSUM / USUM phases (STOMP_DEBUG_SHARDED_MODES): both sides of
    # every K at which weights_kernel takes another instantiation.  At K = 64 the name itself shows
    # the phases ran (the fused launch would be the wave kernel)
    monkeypatch.setenv("STOMP_DEBUG_SHARDED_MODES", "1")
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = zoo_problem(name, K, 0, cumulative=cumulative)
    assert_ragged_columns(p)
    assert bool(p.params.use_cumulative_costs) == cumulative
    orecs = ru.oracle_records(p, (1, 2), ru.ROW_FIELDS)
    e = eng.Engine(p)
    try:
        line, = ru.model_lines(capfd)
        assert line.endswith("weights " + ru.rows_kernel(K)), line
        recs = ru.iterate_records(e, (1, 2))
    finally:
        e.close()
    ru.compare_records([recs], orecs, K, tag=f"{name} K {K}")


# ---------------------------------------------------------------------------- 3. N on ranks
N_RANK_CASES = [(m, n) for m in sorted(N_EXTREME_MODELS) for n in sorted(N_EXTREMES)] + [("chain5", n) for n in (64, 65, 129)]
N_REUSE_CASES = [("chain5", 9), ("pr2", 9), ("chain5", 65), ("chain5", 256), ("pr2", 256)]


def n_problem(model, N, Kr):
    p = N_EXTREME_MODELS[model](N + 1, K=128, Kr=Kr)
    assert p.N == N
    return p


def run_n_case(p, world, mode, monkeypatch, capfd, key):
    """ru.run_case without the default trajectory's census (at the short N it need not touch the
    scene): the census is that of the oracle's own rollout rows."""
    ru.run_case(p, world, mode, monkeypatch, capfd, key=key, default_census=False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model,N", N_RANK_CASES)
def test_n_edges_on_ranks_bitwise(monkeypatch, capfd, model, N, mode):
    run_n_case(n_problem(model, N, 0), 2, mode, monkeypatch, capfd, ("n", model, N, 0))


@pytest.mark.parametrize("model,N", N_REUSE_CASES)
def test_n_edges_on_ranks_with_reuse_bitwise(monkeypatch, capfd, model, N):
    run_n_case(n_problem(model, N, 40), 2, "partials", monkeypatch, capfd, ("n", model, N, 40))


# ---------------------------------------------------------------------------- 4. J and the robots
FUSED_ROBOTS = ["stick1", "hand9", "fork12", "fork13"]       # J <= 16: the noise in the rollout launch
UNFUSED_ROBOTS = ["chain17", "fork24", "chain32"]            # J > 16: k_noise makes every row, no pregen


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FUSED_ROBOTS)
def test_robots_on_ranks_bitwise(monkeypatch, capfd, name, mode):
    p = zoo_problem(name, 128, 0)
    ru.run_case(p, 2, mode, monkeypatch, capfd, key=("robot", name, 0), expect=("pregen 1 fused_noise 1",))


@pytest.mark.parametrize("name", FUSED_ROBOTS)
def test_robots_on_ranks_with_reuse_bitwise(monkeypatch, capfd, name):
    # J <= 16 with reuse on ranks: the rollout launch first, run_reuse after it, no pregen rows
    p = zoo_problem(name, 128, 40)
    ru.run_case(p, 2, "partials", monkeypatch, capfd, census=reuse_census_of(128, 40, 64, cross=True, extra=False),
                expect=("pregen 0 fused_noise 1",))


@pytest.mark.parametrize("Kr", [0, 40])
@pytest.mark.parametrize("name", UNFUSED_ROBOTS)
def test_unfused_robots_on_ranks_bitwise(monkeypatch, capfd, name, Kr):
    # K_r = 40: the only way to run_reuse before launch_noise on ranks (reuse && !reuse_late); four
    # iterations, so that rows reused once are ranked again
    p = zoo_problem(name, 128, Kr)
    assert p.J > 16
    census = reuse_census_of(128, 40, 64, cross=True, extra=False) if Kr else None
    ru.run_case(p, 2, "partials", monkeypatch, capfd, iterations=(1, 2, 3, 4) if Kr else (1, 2, 3), census=census,
                expect=("pregen 0 fused_noise 0",))


@pytest.mark.parametrize("name", UNFUSED_ROBOTS)
def test_gather_is_refused_past_16_joints(monkeypatch, name):
    p = zoo_problem(name, 128, 0)
    monkeypatch.setenv("STOMP_SHARD_MODE", "gather")
    with pytest.raises(RuntimeError) as ei:
        eng.Engine(p, rank=0, world_size=2, comm_id=eng.comm_local_id(2))
    msg = str(ei.value)
    assert "error -3" in msg and "STOMP_SHARD_MODE=gather needs the pregen rows" in msg and f"J = {p.J})" in msg, msg


# ---------------------------------------------------------------------------- 5. reuse at the shard edges

def reuse_census_of(K, Kr, K_loc, cross, extra=True, again=False):
    """The census of a reuse case as a function of the oracle's records (rank_util.reuse_census).
    again: a row reused in one iteration is a source of the next (rows are kept twice in a row)."""
    def census(orecs):
        c = ru.reuse_census(orecs, [r["x_state_costs"] for r in orecs], K, Kr, K_loc)
        assert len(c["sources"]) == len(orecs) - 1
        if cross:
            assert c["crossed"] >= 1, c["sources"]
        if extra:
            assert c["extra_kept"] >= 1, c["sources"]
        if Kr >= K - K_loc:
            assert c["foreign_generated"] == 0, c
        else:
            assert c["foreign_generated"] >= 1, c
        if again:
            kept = sum(1 for a, b in zip(c["sources"], c["sources"][1:]) for _, s in b if s in {d for d, _ in a})
            assert kept >= 1, c["sources"]
    return census


def edge_krs(K):
    return sorted({1, 63, 64, 65, K - 65, K - 64, K - 1})


REUSE_EDGES = [(W, K, Kr) for W, K in ((2, 128), (3, 192)) for Kr in edge_krs(K)]
# K_r = 1 keeps one row, the best of the K + 1 candidates: the extra rollout is kept only if it beats
# every noisy row, which the shape cannot arrange (in these runs it never does: SHARDED_RANKS.md).
# Every other K_r keeps it at least once; every K_r, 1 included, moves a row to another rank
REUSE_EXTRA = {(W, K, Kr): Kr > 1 for W, K, Kr in REUSE_EDGES}


@pytest.mark.parametrize("world,K,Kr", REUSE_EDGES)
def test_reuse_at_the_shard_edges_bitwise(monkeypatch, capfd, world, K, Kr):
    # six iterations: reused rows are reused again, the extra rollout is ranked five times
    p = zoo_problem("chain5", K, Kr)
    census = reuse_census_of(K, Kr, K // world, cross=True, extra=REUSE_EXTRA[world, K, Kr], again=True)
    ru.run_case(p, world, "partials", monkeypatch, capfd, iterations=range(1, 7), census=census)


# ---------------------------------------------------------------------------- 6. cost options on ranks

@pytest.mark.parametrize("mode", MODES)
def test_cumulative_costs_on_ranks_bitwise(monkeypatch, capfd, mode):
    # gather mode: launch_cumulative over all K rows on every rank
    p = zoo_problem("chain5", 128, 0, cumulative=True)
    assert p.params.use_cumulative_costs
    ru.run_case(p, 2, mode, monkeypatch, capfd, key="cumulative")


@pytest.mark.parametrize("mode", MODES)
def test_per_joint_noise_schedule_on_ranks_bitwise(monkeypatch, capfd, mode):
    p = mz.chain5(K=128, Kr=0, noise_stddev=[2.0, 1.5, 3.0, 0.5, 2.5], noise_decay=[0.999, 0.995, 1.0, 0.99, 0.98])

    def census(orecs):      # the joints' noise differs in scale
        spread = [np.abs(orecs[-1]["noise"][:, j]).mean() for j in range(p.J)]
        assert len({round(s, 6) for s in spread}) == p.J, spread

    ru.run_case(p, 2, mode, monkeypatch, capfd, key="schedule", census=census)


@pytest.mark.parametrize("mode", MODES)
def test_alternative_smoothness_parameters_on_ranks_bitwise(monkeypatch, capfd, mode):
    # chain5 carries ALT_PARAMS already (every chain5 case runs them); hand9 does not by default
    p = mz.hand9(K=128, Kr=0, **mz.ALT_PARAMS)
    assert p.params.smoothness_cost_velocity == 0.3 and p.params.smoothness_cost_jerk == 0.05
    assert zoo_problem("chain5", 128, 0).params.ridge_factor == mz.ALT_PARAMS["ridge_factor"]
    ru.run_case(p, 2, mode, monkeypatch, capfd, key="alt")


@pytest.mark.parametrize("mode", MODES)
def test_degenerate_weights_on_ranks_bitwise(monkeypatch, capfd, mode):
    # noise_stddev = 0: min == max arrive through the all-reduce and W_PSUM floors the range at 1e-8
    K = 128
    p = mz.chain5(K=K, Kr=0, noise_stddev=0.0)
    theta0 = po.Oracle(p).theta()

    def census(orecs):
        assert not any(orec["noise"].any() for orec in orecs)

    recs, _ = ru.run_case(p, 2, mode, monkeypatch, capfd, iterations=(1, 2), key="degenerate", census=census)
    for r, rank_recs in enumerate(recs):
        for rec in rank_recs:
            np.testing.assert_array_equal(rec["probabilities"], np.full((K // 2, p.J, p.N), 1.0 / K), err_msg=f"rank {r}")
            np.testing.assert_array_equal(rec["theta"], theta0, err_msg=f"rank {r}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["chain5", "fork12_base"])
def test_state_terms_on_ranks_bitwise(monkeypatch, capfd, name, mode):
    p = zoo_problem(name, 128, 0, terms=True)
    assert p.params.torque_cost_weight > 0 and p.orientation_constraints

    def census(orecs):      # the terms are in the costs: the same row costs less without them
        plain = po.Oracle(mz.TERMS_ZOO[name](K=128, Kr=0, torque=0.0, constrained=False))
        without = plain.execute(orecs[0]["params"][0], 0)[0]
        assert np.all(orecs[0]["state_costs"][0] >= without) and np.any(orecs[0]["state_costs"][0] > without)

    ru.run_case(p, 2, mode, monkeypatch, capfd, key=("terms", name), census=census)


@pytest.mark.parametrize("mode", MODES)
def test_optimize_and_best_torques_on_ranks_bitwise(monkeypatch, capfd, mode):
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = zoo_problem("chain5", 128, 0, terms=True, max_iterations=10)
    o = po.Oracle(p, threads=ru.THREADS)
    ru.assert_default_census(p, o.theta())
    ost, ocosts = o.optimize()
    assert ost.iterations == 10
    ru.assert_rollout_census(p, [dict(params=o.rollouts("params"))])
    engines = ru.make_ranks(p, 2, mode, monkeypatch)

    def drive(r, e):
        st, costs = e.optimize()
        return np.array([st.iterations, st.success, st.success_iteration, st.last_improvement_iteration]), \
            np.array([st.best_cost]), costs, e.best_trajectory(), e.best_torques(), e.theta()

    try:
        ru.assert_creation(engines, ru.model_lines(capfd), 128, mode)
        res = ru.on_threads(engines, drive)
    finally:
        ru.close_all(engines)
    want = (np.array([ost.iterations, ost.success, ost.success_iteration, ost.last_improvement_iteration]),
            np.array([ost.best_cost]), ocosts, o.best_trajectory(), o.best_torques(), o.theta())
    assert want[4].any()
    for r, got in enumerate(res):
        for k, (a, b) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(a, b, err_msg=f"rank {r} item {k}")
        np.testing.assert_array_equal(got[4], res[0][4])


# ---------------------------------------------------------------------------- 7. fields

def _with_cylinder(p):
    """The second scene: the problem's boxes and a pole through the middle sphere's place at the
    middle of the default trajectory, so that the rows' costs change."""
    mid = 0.5 * (np.asarray(p.start) + np.asarray(p.goal))
    c = pb.sphere_positions(p.robot, p.spheres, mid)[len(p.spheres) // 2]
    p.cylinders = [pb.Cylinder((float(c[0]) + 0.06, float(c[1]), float(c[2])), 0.05, 0.3)]
    return pb.build_sdf(p.grid, p.boxes, p.cylinders)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["linear", "brick"])
@pytest.mark.parametrize("shape", [mz.NONCUBIC, mz.NONCUBIC_PERM])
def test_shared_device_field_refreshed_on_ranks_bitwise(monkeypatch, capfd, shape, layout, mode):
    monkeypatch.setenv("STOMP_SDF_LAYOUT", layout)
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    K = 128
    p = mz.chain5(K=K, Kr=0, shape=shape)
    first = p.sdf.copy()
    assert first.shape == tuple(shape)
    o = po.Oracle(p, threads=ru.THREADS)
    ru.assert_default_census(p, o.theta())
    buf = eng.DeviceBuffer(2 * p.grid.cells)
    engines = []
    try:
        eng.sdf_build_device(p, buf.ptr)
        np.testing.assert_array_equal(buf.to_numpy(np.uint16, tuple(shape)), first)
        engines = ru.make_ranks(p, 2, mode, monkeypatch, sdf_device_ptr=buf.ptr)
        lines = ru.model_lines(capfd)
        ru.assert_creation(engines, lines, K, mode)
        assert all(f"brick {int(layout == 'brick')}," in l for l in lines), lines
        orecs = ru.iterate_records(o, (1, 2))
        ru.assert_rollout_census(p, orecs)
        recs = ru.on_threads(engines, lambda r, e: ru.iterate_records(e, (1, 2)))
        # every rank is idle (iterate returned): the caller rebuilds its buffer in place
        second = _with_cylinder(p)
        assert (second != first).sum() > 100
        eng.sdf_build_device(p, buf.ptr)
        np.testing.assert_array_equal(buf.to_numpy(np.uint16, tuple(shape)), second)
        o.refresh_field(second)
        p.sdf = second
        c = mz.census(p, o.theta()[None])
        assert c["collision"] >= 1 and c["hinge"] >= 1, c
        orecs += ru.iterate_records(o, (3, 4))
        ru.assert_rollout_census(p, orecs[2:])

        def drive(r, e):
            e.refresh_field()
            return ru.iterate_records(e, (3, 4))

        more = ru.on_threads(engines, drive)
    finally:
        ru.close_all(engines)
        buf.free()
    # the new field changed what the rows cost: an engine still on the old one would differ
    old = ru.iterate_records(po.Oracle(mz.chain5(K=K, Kr=0, shape=shape), threads=ru.THREADS), (1, 2, 3))
    np.testing.assert_array_equal(old[1]["state_costs"], orecs[1]["state_costs"])
    assert (old[2]["state_costs"] != orecs[2]["state_costs"]).sum() > 100
    ru.compare_records([a + b for a, b in zip(recs, more)], orecs, K // 2, tag=f"{shape} {layout} {mode}")


# ---------------------------------------------------------------------------- 8. calls between iterations

@pytest.mark.parametrize("mode,Kr", [("partials", 40), ("gather", 0)])
@pytest.mark.parametrize("world", [2, 3])
def test_calls_between_iterations_on_ranks_bitwise(monkeypatch, capfd, world, mode, Kr):
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    K = 64 * world * 2
    K_loc = K // world
    p = zoo_problem("chain5", K, Kr)
    fields = ru.ROW_FIELDS + (ru.X_FIELDS if Kr else ())
    offset = 0.01 * np.sin(np.arange(p.J * p.N, dtype=np.float64)).reshape(p.J, p.N)

    def script(x, rows, theta_set):
        """The one sequence of calls, for the oracle and for every rank; returns (records, execute's
        outputs).  rows / theta_set None: the oracle's pass, which makes them."""
        oracle = rows is None
        if oracle:
            for it in (1, 2, 3):
                x.iterate(it)
        else:
            x.run(1, 3)
            x.synchronize()
        recs = [ru.snapshot(x, None, fields)]
        recs.append(ru.snapshot(x, x.iterate(4), fields))
        if oracle:
            rows = mz.execute_rows(p, recs[-1]["theta"], rows=2 * K_loc + 3)
            theta_set = recs[-1]["theta"] + offset
            out = [x.execute(r, 1) for r in rows]
            ex = (np.stack([c for c, _, _ in out]), np.array([f for _, f, _ in out]), np.stack([t for _, _, t in out]))
        else:
            ex = x.execute(rows, iteration_member=1)
        recs.append(ru.snapshot(x, None, fields))             # eval left every row where it was
        x.set_theta(theta_set)
        recs.append(ru.snapshot(x, x.iterate(9), fields))     # an out-of-order iteration number
        if oracle:
            x.iterate(10)
            x.iterate(11)
        else:
            x.run(10, 2)
        recs.append(ru.snapshot(x, x.iterate(12), fields))
        return recs, ex, rows, theta_set

    o = po.Oracle(p, threads=ru.THREADS)
    ru.assert_default_census(p, o.theta())
    orecs, oex, rows, theta_set = script(o, None, None)
    assert len(rows) == 2 * K_loc + 3 > K_loc
    ru.assert_rollout_census(p, orecs)
    # (of theta's own row, three walks and the shifted last row: what they reach, all the rows reach)
    c = mz.census(p, rows[[0, 1, 2, 3, len(rows) - 1]])
    assert c["rows_limited"] >= 1 and c["collision"] >= 1 and c["hinge"] >= 1 and c["free"] >= 1, c
    engines = ru.make_ranks(p, world, mode, monkeypatch)
    try:
        ru.assert_creation(engines, ru.model_lines(capfd), K, mode)
        res = ru.on_threads(engines, lambda r, e: script(e, rows, theta_set)[:2])
    finally:
        ru.close_all(engines)
    # the records without a cost (after run + synchronize, after execute) carry none on either side
    ru.compare_records([rr for rr, _ in res], orecs, K_loc, tag=f"W {world} {mode}")
    for r, (_, ex) in enumerate(res):
        for k, name in enumerate(("costs", "collision free", "trajectories")):
            np.testing.assert_array_equal(ex[k], oex[k], err_msg=f"rank {r} execute {name}")


# ---------------------------------------------------------------------------- 9. refusals, the default rule

@pytest.mark.parametrize("mode,Kr", [("partials", 40), ("gather", 0)])
def test_step_api_is_refused_on_ranks(monkeypatch, capfd, mode, Kr):
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    K = 128
    p = zoo_problem("chain5", K, Kr)
    fields = ru.ROW_FIELDS + (ru.X_FIELDS if Kr else ())
    orecs = ru.oracle_records(p, (1, 2, 3, 4), fields)
    engines = ru.make_ranks(p, 2, mode, monkeypatch)
    try:
        ru.assert_creation(engines, ru.model_lines(capfd), K, mode)
        recs = ru.on_threads(engines, lambda r, e: ru.iterate_records(e, (1,), fields))
        sig, zeros = np.full(p.J, 2.0), np.zeros((K, p.N))
        for e in engines:      # on this thread, one rank after the other: a refusal posts no collective
            for call in (lambda: e.pi_get_rollouts(2, sig), lambda: e.pi_set_rollout_costs(zeros, 1.0),
                         lambda: e.pi_improve_policy(), lambda: e.pi_add_extra_rollout(orecs[0]["theta"], zeros[0]),
                         lambda: e.pi_reset()):
                with pytest.raises(RuntimeError) as ei:
                    call()
                assert "error -3" in str(ei.value) and "single-rank" in str(ei.value), str(ei.value)
        more = ru.on_threads(engines, lambda r, e: ru.iterate_records(e, (2, 3, 4), fields))
    finally:
        ru.close_all(engines)
    ru.compare_records([a + b for a, b in zip(recs, more)], orecs, K // 2, tag=mode)


def test_group_of_rank_engines_is_refused(monkeypatch, capfd):
    # two ranks on one stream, one shape: the only reason left to refuse the group is that they are ranks
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = zoo_problem("chain5", 128, 0)
    orecs = ru.oracle_records(p, (1,), ru.ROW_FIELDS)
    stream = eng.Stream()
    engines = ru.make_ranks(p, 2, "partials", monkeypatch, stream=stream.ptr)
    try:
        ru.assert_creation(engines, ru.model_lines(capfd), 128, "partials")
        with pytest.raises(RuntimeError) as ei:
            eng.EngineGroup(engines)
        assert "error -3" in str(ei.value) and "groups run single-device engines" in str(ei.value), str(ei.value)
    finally:
        ru.close_all(engines)
        stream.close()
    # the library works afterwards
    engines = ru.make_ranks(p, 2, "partials", monkeypatch)
    try:
        ru.assert_creation(engines, ru.model_lines(capfd), 128, "partials")
        recs = ru.on_threads(engines, lambda r, e: ru.iterate_records(e, (1,)))
    finally:
        ru.close_all(engines)
    ru.compare_records(recs, orecs, 64)


def test_half_a_block_per_rank_is_refused(monkeypatch):
    # K = 64 W + 64 at W = 2: a multiple of 64 but not of 64 W, K_loc would be one and a half blocks
    # (tests/test_abi.py has K = 96, which is no multiple of 64 at all, and rank = W)
    monkeypatch.setenv("STOMP_SHARD_MODE", "partials")
    p = zoo_problem("chain5", 192, 0)
    assert p.params.num_rollouts % 64 == 0 and p.params.num_rollouts % 128 == 64
    for rank in (0, 1):
        with pytest.raises(RuntimeError) as ei:
            eng.Engine(p, rank=rank, world_size=2, comm_id=eng.comm_local_id(2))
        assert "error -1" in str(ei.value) and "num_rollouts must be a multiple of 64 * world_size" in str(ei.value), \
            str(ei.value)
    # the same K on three ranks is whole blocks: accepted (test_worlds_and_blocks_bitwise[3-192] runs it)
    engines = ru.make_ranks(p, 3, "partials", monkeypatch)
    try:
        assert [(e.first, e.K_loc) for e in engines] == [(0, 64), (64, 64), (128, 64)]
    finally:
        ru.close_all(engines)


def test_joining_a_local_group_wrongly_is_refused(monkeypatch, capfd):
    monkeypatch.setenv("STOMP_SHARD_MODE", "partials")
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = zoo_problem("chain5", 128, 0)
    orecs = ru.oracle_records(p, (1,), ru.ROW_FIELDS)
    with pytest.raises(RuntimeError) as ei:
        eng.Engine(p, rank=0, world_size=2, comm_id=eng.comm_local_id(3))
    assert "error -4" in str(ei.value) and "local group of 3 ranks, engine world_size 2" in str(ei.value), str(ei.value)
    gid = eng.comm_local_id(2)
    ru.model_lines(capfd)      # a refused rank printed its line too: the join comes after the model
    e0 = eng.Engine(p, rank=0, world_size=2, comm_id=gid)
    lines = ru.model_lines(capfd)
    try:
        with pytest.raises(RuntimeError) as ei:
            eng.Engine(p, rank=0, world_size=2, comm_id=gid)
        assert "error -4" in str(ei.value) and "rank 0 joined the local group twice" in str(ei.value), str(ei.value)
        ru.model_lines(capfd)
        # the group is still whole for the rank that was missing
        e1 = eng.Engine(p, rank=1, world_size=2, comm_id=gid)
        try:
            ru.assert_creation([e0, e1], lines + ru.model_lines(capfd), 128, "partials")
            recs = ru.on_threads([e0, e1], lambda r, e: ru.iterate_records(e, (1,)))
        finally:
            e1.close()
    finally:
        e0.close()
    ru.compare_records(recs, orecs, 64)


@pytest.mark.parametrize("K,waypoints,nbytes,want", [(512, 257, 1 << 20, "gather"), (640, 205, 1044480, "gather"),
                                                     (640, 206, 1049600, "partials")])
def test_default_decomposition_at_its_boundary_bitwise(monkeypatch, capfd, K, waypoints, nbytes, want):
    # no STOMP_SHARD_MODE, an in-process group without calibration: gather while the K N state rows
    # are at most 1 MiB (choose_decomposition)
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    p = zoo_problem("chain5", K, 0, waypoints=waypoints)
    assert K * p.N * 8 == nbytes and (nbytes <= 1 << 20) == (want == "gather")
    orecs = ru.oracle_records(p, (1,), ru.ROW_FIELDS, default_census=False)
    engines = ru.make_ranks(p, 2, None, monkeypatch)
    try:
        ru.assert_creation(engines, ru.model_lines(capfd), K, want)
        assert all(e.shard_info is None for e in engines)     # nothing was measured
        recs = ru.on_threads(engines, lambda r, e: ru.iterate_records(e, (1,)))
    finally:
        ru.close_all(engines)
    ru.compare_records(recs, orecs, K // 2, tag=want)
