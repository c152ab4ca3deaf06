"""CPU tests of the C oracle's state-cost terms over the terms robots of tests/model_zoo.py
(tests/STATE_TERMS.md): torque chains with a fixed first, inner or last segment, a chain of one
segment, a torque root that is not the tree's, constraints on other branches than the torque tip,
and the crafted constraint rows that reach KDL GetQuaternion's single-precision branches and
bullet getRPY's gimbal branch.

The oracle is held to the independent numpy restatements at the tolerances tests/test_torque.py and
tests/test_constraints.py use on the PR2 fixture: rtol = atol = 1e-11 for the inverse dynamics,
rel 1e-10 / abs 1e-12 for the weighted torque sum in the cost, rel 1e-6 / abs 1e-7 once an
orientation constraint is in the cost (the scipy restatement, away from the gimbal branch).  The GPU
twin (tests/test_gpu_terms_space.py) then holds the engine to the oracle bit for bit.
"""
import math

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from oracle import numpy_oracle as npo
from oracle import pyoracle as po
from stomp_motion_planner_icra2011_amd import problem as pb
from tests import model_zoo as mz

TERMS = list(mz.TERMS_ZOO)


def test_terms_robots_have_their_chain_shapes():
    def chain(name):
        p = mz.TERMS_ZOO[name]()
        return p, [p.robot.segments[i] for i in p.torque_chain()]

    for name in TERMS:      # the LDS rows the GPU tests' byte counts are computed from
        p, c = chain(name)
        assert 3 * p.J + 6 * len(c) == mz.TERMS_LDS_ROWS[name], name
        assert [s.q_index for s in c if s.q_index >= 0] == list(range(p.J)), name
        assert all(s.inertia is not None for s in p.robot.segments[1:]), name
    p, c = chain("stick1_one")
    assert len(c) == 1 and c[0].q_index == 0                                  # first segment == last segment
    p, c = chain("stick1_pedestal")
    assert [s.q_index for s in c] == [-1, 0, -1]                              # fixed first and last segment
    p, c = chain("fork12_base")
    assert c[0].q_index < 0 and p.robot.index(p.torque_root) == 0             # fixed first segment
    assert [s.name for s in c if s.q_index < 0] == ["pedestal", "brace", "palm", "prong_b"]
    assert 0 < c.index(p.robot.segments[p.robot.index("brace")]) < len(c) - 2   # a fixed segment between joints
    p, c = chain("fork12_pedestal")
    assert p.robot.index(p.torque_root) != 0 and c[0].q_index == 0            # a root that is not the tree's
    assert [s.q_index for s in c[-2:]] == [-1, -1]                            # a fixed tail of two segments
    on_chain = {s.name for s in c}
    links = [oc.link_name for oc in p.orientation_constraints]
    assert len(links) == 3 and "prong_a" in links and "prong_a" not in on_chain and "palm" in on_chain
    p, c = chain("chain17")
    assert p.J == 17 and len(c) == 17
    h = mz.hand9_constrained()
    assert h.torque_segments() == (-1, -1) and [oc.link_name for oc in h.orientation_constraints] == ["a2", "b2"]
    tols = [t for oc in mz.fork12_constraints() for t in
            (oc.absolute_roll_tolerance, oc.absolute_pitch_tolerance, oc.absolute_yaw_tolerance)]
    assert any(t >= math.pi for t in tols) and any(t < math.pi for t in tols)


@pytest.mark.parametrize("name", TERMS)
def test_inverse_dynamics_matches_world_frame_newton_euler(name):
    p = mz.TERMS_ZOO[name]()
    o = po.Oracle(p)
    rng = np.random.default_rng(1)
    for _ in range(20):
        q, qd, qdd = rng.uniform(-2, 2, (3, p.J))
        np.testing.assert_allclose(o.inverse_dynamics(q, qd, qdd), npo.inverse_dynamics(p, q, qd, qdd), rtol=1e-11,
                                   atol=1e-11)


def _numpy_terms(p, traj, t):
    """(sum_j |tau_j|, summed constraint cost, all satisfied, near the gimbal branch) at free
    waypoint t of the joint-limited trajectory `traj` (J x N), by the numpy restatements."""
    disc = p.params.trajectory_discretization
    full = np.concatenate([np.repeat(p.start[None], 6, 0), traj.T, np.repeat(p.goal[None], 6, 0)])
    i = t + 6
    tq = 0.0
    if p.torque_segments() != (-1, -1):
        qd = sum(npo.DIFF_RULES[0][k + 3] / disc * full[i + k] for k in range(-3, 4))
        qdd = sum(npo.DIFF_RULES[1][k + 3] / disc ** 2 * full[i + k] for k in range(-3, 4))
        tq = np.abs(npo.inverse_dynamics(p, full[i], qd, qdd)).sum()
    con, ok, near = 0.0, True, False
    frames = pb.fk_frames(p.robot, traj[:, t])
    for c in p.orientation_constraints:
        R = frames[p.robot.index(c.link_name)][0]
        N = Rotation.from_quat(np.asarray(c.orientation, np.float64)).as_matrix()
        E = R @ N.T if c.header_frame else N.T @ R
        near = near or abs(E[2, 0]) > 0.999
        cc, sat = npo.orientation_constraint_cost(c, R)
        con += cc
        ok = ok and sat
    return tq, con, ok, near


@pytest.mark.parametrize("name", TERMS + ["hand9"])
def test_execute_adds_the_weighted_terms(name):
    # the oracle with the terms on against the oracle without them plus the numpy restatements
    if name == "hand9":
        p, p0 = mz.hand9_constrained(), mz.hand9()
    else:
        p, p0 = mz.TERMS_ZOO[name](), mz.TERMS_ZOO[name](torque=0.0, constrained=False)
    o, o0 = po.Oracle(p), po.Oracle(p0)
    w_tq, w_con = p.params.torque_cost_weight, p.params.constraint_cost_weight
    tol = dict(rel=1e-6, abs=1e-7) if p.orientation_constraints else dict(rel=1e-10, abs=1e-12)
    rows = mz.execute_rows(p, o.theta(), rows=3, seed=9)
    checked = 0
    for r in rows:
        c1, cf1, traj = o.execute(r, 1)
        sat1 = o.last_constraints_satisfied
        c0, cf0, traj0 = o0.execute(r, 1)
        np.testing.assert_array_equal(traj, traj0)
        assert cf1 == cf0
        oks = []
        for t in sorted({0, 1, 2, 3, p.N // 2, p.N - 4, p.N - 3, p.N - 2, p.N - 1}):   # the padded taps and the middle
            tq, con, ok, near = _numpy_terms(p, traj, t)
            assert not near
            assert c1[t] == pytest.approx(c0[t] + w_con * con + w_tq * tq, **tol), (name, t)
            checked += 1
        for t in range(p.N):
            oks.append(_numpy_terms(p, traj, t)[2])
        assert sat1 == all(oks)
    assert checked == 3 * 9


# ---------------------------------------------------------------------------- crafted constraint rows

def crafted_census_all():
    """The census of every crafted case on the oracle alone: {case: (problem, rows, census)}."""
    out = {}
    for case in mz.CRAFTED_CASES:
        p = mz.crafted_problem(case)
        o = po.Oracle(p)
        rows = mz.crafted_rows(p)
        sat = []
        for r in rows:
            o.execute(r, 1)
            sat.append(o.last_constraints_satisfied)
        out[case] = (p, rows, mz.crafted_census(p, o, rows), sat)
    return out


def assert_crafted_census(cases):
    """What the crafted rows must reach on the oracle (its own kdl_get_quaternion / bt_get_rpy,
    through Oracle.orientation_probe) before anything is compared with them."""
    seen = set()
    for case, (p, rows, census, sat) in cases.items():
        for c, body_fixed, branch, gimbal, exact in census:
            if exact:      # only the waypoints with every joint exactly 0 count
                seen.add((body_fixed, branch, gimbal))
    for body_fixed in (0, 1):
        for branch in (0, 1, 2, 3):
            assert any(s[0] == body_fixed and s[1] == branch for s in seen), (body_fixed, branch, seen)
        for gimbal in (-1, 1):
            assert any(s[0] == body_fixed and s[2] == gimbal for s in seen), (body_fixed, gimbal, seen)
    assert any(s[2] == 0 for s in seen)
    ocs = [oc for p, _, _, _ in cases.values() for oc in p.orientation_constraints]
    assert any(tuple(oc.orientation) != mz.Q_IDENT for oc in ocs)             # a non-identity nominal orientation
    gimbal_constraints = {(case, c) for case, (_, _, census, _) in cases.items() for c, _, _, g, ex in census if ex and g}
    assert any(tuple(cases[case][0].orientation_constraints[c].orientation) != mz.Q_IDENT
               for case, c in gimbal_constraints)                            # ... also in the gimbal branch
    assert any(oc.absolute_roll_tolerance >= math.pi for oc in ocs)           # the zeroed weights
    assert any(oc.absolute_pitch_tolerance >= math.pi for oc in ocs)
    assert any(oc.absolute_yaw_tolerance >= math.pi for oc in ocs)
    sats = [s for _, _, _, sat in cases.values() for s in sat]
    assert any(sats) and not all(sats)                                        # constraints_satisfied 1 and 0
    assert any(len(p.orientation_constraints) >= 3 for p, _, _, _ in cases.values())
    # the nanoradian waypoints fall on both sides of |E[6]| >= 1
    near = [(g != 0) for case, (p, rows, census, _) in cases.items() if case.startswith("gimbal")
            for (c, _, _, g, ex), t in zip(census, np.repeat(np.tile(np.arange(p.N), len(rows)),
                                                             len(p.orientation_constraints)))
            if t in mz.NEAR_T and not ex]
    assert any(near) and not all(near)


@pytest.fixture(scope="module")
def crafted():
    return crafted_census_all()


def test_crafted_rows_reach_every_branch(crafted):
    assert_crafted_census(crafted)


def _ypr_matrix(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    Ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    Rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    return Rz @ Ry @ Rx


C_DOUBLE, C_SINGLE = 16.0, 1.0


def test_crafted_rows_angles_rebuild_the_error_matrix(crafted):
    """On the crafted rows scipy's Euler angles are ill-conditioned (half turns, quarter turns of
    pitch), so the oracle's signed angles are checked through the matrix they stand for:
    Rz(yaw) Ry(pitch) Rx(roll) against the orientation error E computed in numpy from the numpy FK.

    Bound, per entry: C_DOUBLE eps64 / cos(pitch) + (C_SINGLE eps32 in the three single-precision
    quaternion branches).  The first term is double rounding through asin / atan2 of entries divided by
    cos(pitch) (the nanoradian waypoints have cos(pitch) near 1.5e-8); the second is the rounding of
    `float s` in KDL GetQuaternion.  Measured on these cases: 10.7 eps64 / cos(pitch) in the trace branch
    (1.7 away from the quarter turns) and 0.83 eps32 in the single-precision branches; the constants
    16 and 1 are those with a margin of 1.5 and 1.2.

    bullet's gimbal branch (|E[6]| >= 1) is not a decomposition of E: it returns yaw 0, pitch +-pi/2
    and roll = +-pitch + atan2(E[0], E[2]) (the reference's bullet reads E[0][0] and E[0][2] there, and
    calls E[6] > 0 "locked up"), and the rebuilt matrix is off by up to 2.0 on these cases.  There the
    angles are held to that published formula on the numpy E instead, to 4 eps64."""
    eps64, eps32 = np.finfo(np.float64).eps, float(np.finfo(np.float32).eps)
    counts = dict(trace=0, single=0, gimbal=0, gimbal_roll=0)
    worst = dict(trace=0.0, single=0.0)
    for case, (p, rows, census, _) in crafted.items():
        o = po.Oracle(p)
        for r in rows:
            for t in range(p.N):
                frames = pb.fk_frames(p.robot, r[:, t])
                for c, oc in enumerate(p.orientation_constraints):
                    R = frames[p.robot.index(oc.link_name)][0]
                    N = Rotation.from_quat(np.asarray(oc.orientation, np.float64)).as_matrix()
                    E = R @ N.T if oc.header_frame else N.T @ R
                    branch, gimbal, (roll, pitch, yaw) = o.orientation_probe(r[:, t], c)
                    if gimbal:
                        assert gimbal == (1 if E[2, 0] > 0 else -1) and abs(abs(E[2, 0]) - 1.0) <= 4 * eps64
                        assert yaw == 0.0 and pitch == gimbal * (math.pi / 2)
                        if math.hypot(E[0, 0], E[0, 2]) > 0.5:      # else atan2 of two zeros: any angle
                            delta = math.atan2(E[0, 0], E[0, 2])
                            assert abs(roll - (math.pi / 2 + delta)) <= 4 * eps64 * 2 * math.pi, (case, t, c)
                            counts["gimbal_roll"] += 1
                        assert -math.pi / 2 <= roll <= 3 * math.pi / 2
                        counts["gimbal"] += 1
                        continue
                    err = np.abs(_ypr_matrix(roll, pitch, yaw) - E).max()
                    bound = C_DOUBLE * eps64 / abs(math.cos(pitch)) + (C_SINGLE * eps32 if branch else 0.0)
                    assert err <= bound, (case, t, c, branch, err, bound)
                    kind = "single" if branch else "trace"
                    counts[kind] += 1
                    worst[kind] = max(worst[kind], err / bound)
    assert min(counts.values()) >= 100, counts
    # the bound is not slack: the worst case uses more than half of it in both classes
    assert worst["trace"] > 0.5 and worst["single"] > 0.5, worst


def test_crafted_rows_costs_match_numpy(crafted):
    # the cost the oracle adds at the exact waypoints: weight * (rw |roll| + pw |pitch| + yw |yaw|) with
    # the probe's angles, which the test above ties to E; the weights of tolerances >= pi are zero
    for case, (p, rows, census, _) in crafted.items():
        o = po.Oracle(p)
        p0 = mz.crafted_problem(case)
        p0.orientation_constraints = []
        o0 = po.Oracle(p0)
        w = p.params.constraint_cost_weight
        for r in rows[:2]:
            c1, c0 = o.execute(r, 1)[0], o0.execute(r, 1)[0]
            for t in mz.CRAFTED_T + mz.NEAR_T:
                want = 0.0
                for c, oc in enumerate(p.orientation_constraints):
                    _, _, rpy = o.orientation_probe(r[:, t], c)
                    tols = (oc.absolute_roll_tolerance, oc.absolute_pitch_tolerance, oc.absolute_yaw_tolerance)
                    want += oc.weight * sum(abs(a) for a, tol in zip(rpy, tols) if tol < math.pi)
                assert c1[t] == pytest.approx(c0[t] + w * want, rel=1e-12, abs=1e-12), (case, t)
