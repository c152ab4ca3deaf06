"""The oracle's PolicyImprovement steps (so_pi_*, oracle/stomp_oracle.c) on the CPU.

so_iterate is the composition of the five steps, so the golden files of the iteration pin them
already; here the steps driven from outside, as a host planner drives them, are held to a second
oracle that calls iterate (assert_array_equal), the probabilities and the update to a plain numpy
restatement (the tolerances tests/test_model_space.py uses for the same quantities), and the
censuses the GPU cases of tests/test_gpu_pi_steps.py rely on are asserted on the oracle alone.
tests/PI_STEPS.md lists what each case reaches.
"""
import numpy as np
import pytest

from oracle import numpy_oracle as npo
from oracle import pyoracle as po
from tests import pi_steps_util as su

FIELDS = ("params", "noise", "noise_projected", "control_costs", "state_costs", "probabilities") + su.X_FIELDS


def loop_sigma(p, it):
    """policy_improvement_loop.cpp:155-160, the arithmetic of so_iterate."""
    sd, dc = p.params.per_joint("noise_stddev", p.J), p.params.per_joint("noise_decay", p.J)
    return np.array([float(sd[d]) * float(dc[d]) ** (it - 1) for d in range(p.J)])


@pytest.mark.parametrize("name", ["stick1", "chain5", "chain17"])
def test_steps_equal_iterate(name):
    # driven exactly as runSingleIteration drives PolicyImprovement: the oracle's own execute for the
    # generated rows, theta + update through set_theta, theta as the extra rollout
    p = su.zoo_problem(name, 12, 5)
    d, ref = su.Driver(p), po.Oracle(p)
    for it in range(1, 6):
        out = d.step_iteration(it, costs="oracle", extra="theta", sig=loop_sigma(p, it))
        cost, cf = ref.iterate(it)
        assert float(out["x_costs"].sum()) == pytest.approx(cost, rel=1e-12)
        assert len(out["rollouts"]) == (12 if it == 1 else 7)
        np.testing.assert_array_equal(d.o.theta(), ref.theta(), err_msg=f"it {it} theta")
        for f in FIELDS:
            np.testing.assert_array_equal(d.o.rollouts(f), ref.rollouts(f), err_msg=f"it {it} {f}")
        np.testing.assert_array_equal(out["totals"], su.totals_in_reference_order(
            ref.rollouts("state_costs"), ref.rollouts("control_costs")))
    np.testing.assert_array_equal(d.o.reuse_log(), ref.reuse_log())
    assert d.o.reuse_log().shape == (4, 5)


def test_steps_against_numpy():
    # chain5, N = 39, synthetic state costs, another weight in the second iteration and an extra
    # rollout that is not theta: control costs, probabilities and update against numpy, the
    # ranking exactly
    p = su.zoo_problem("chain5", 12, 5)
    assert p.N == 39
    d, n = su.Driver(p), npo.NumpyStomp(p)
    rng = np.random.default_rng(5)
    K, Kr = d.K, d.Kr
    prev = None
    for it in (1, 2, 3):
        wgt = d.w * (3.0 if it == 2 else 1.0)
        theta0 = d.o.theta()
        out = d.step_iteration(it, costs=lambda it, ro: su.synthetic_costs(rng, len(ro), p.N),
                               extra=lambda it, th: (su.walk(rng, th), su.synthetic_costs(rng, 1, p.N)[0]),
                               weights=(wgt,))
        if prev is not None:
            # generateRollouts' ranking (policy_improvement.cpp:178-212): (total, index), the extra at -1
            cand = sorted(zip(list(prev["totals"]) + [prev["x_total"]], list(range(K)) + [-1]))
            assert [i for _, i in cand[:Kr]] == list(d.o.reuse_log()[-1])
            for slot, (_, src) in enumerate(cand[:Kr]):
                want = prev["x_params"] if src < 0 else prev["params"][src]
                np.testing.assert_array_equal(d.o.rollouts("params")[K - Kr + slot], want)
        params, noise, state = d.o.rollouts("params"), d.o.rollouts("noise"), d.o.rollouts("state_costs")
        np.testing.assert_array_equal(noise[d.K_gen:], params[d.K_gen:] - theta0[None])
        np.testing.assert_array_equal(state[:d.K_gen], out["costs"])
        nproj = np.einsum("ik,rdk->rdi", n.M, noise)
        ctrl = np.stack([n.control_costs(params[r], nproj[r]) for r in range(K)]) * (wgt / d.w)
        np.testing.assert_allclose(d.o.rollouts("control_costs"), ctrl, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(out["totals"], state.sum(axis=1) + ctrl.sum(axis=(1, 2)), rtol=1e-6, atol=1e-9)
        S = state[:, None, :] + ctrl
        mn, mx = S.min(axis=0), S.max(axis=0)
        P = np.exp(-10.0 * (S - mn) / np.maximum(mx - mn, 1e-8))
        P = P / P.sum(axis=0)
        np.testing.assert_allclose(d.o.rollouts("probabilities"), P, rtol=1e-5, atol=1e-10)
        np.testing.assert_allclose(out["update"], (noise * P).sum(axis=0) @ n.M.T, rtol=0, atol=1e-7)
        assert np.abs(out["update"]).max() > 1e-4      # the bound above says something
        # the extra rollout: noise against the theta addExtraRollouts saw, priced under the kept weight
        xn = out["x_params"] - out["theta"]
        np.testing.assert_array_equal(d.o.rollouts("x_noise"), xn)
        assert xn.any()
        xc = n.control_costs(out["x_params"], np.einsum("ik,dk->di", n.M, xn)) * (wgt / d.w)
        np.testing.assert_allclose(d.o.rollouts("x_control_costs"), xc, rtol=1e-6, atol=1e-9)
        prev = dict(totals=out["totals"], params=params, x_params=out["x_params"],
                    x_total=su.totals_in_reference_order(out["x_costs"][None],
                                                         d.o.rollouts("x_control_costs")[None])[0])


@pytest.mark.parametrize("case", list(su.CRAFTED))
def test_crafted_census(case):
    # the conditions the GPU cases rely on, on the oracle alone (the assertions are in the case)
    problem, run = su.CRAFTED[case]
    run(su.Driver(problem()))


def test_reset_and_weight_memory():
    # setNumRollouts (policy_improvement.cpp:139-143): the next getRollouts generates all K and a
    # pending extra rollout is dropped; addExtraRollouts prices under the last setRolloutCosts' weight
    p = su.zoo_problem("chain5", 12, 5)
    d = su.Driver(p)
    rng = np.random.default_rng(9)
    mk = lambda it, ro: su.synthetic_costs(rng, len(ro), p.N)
    d.step_iteration(1, costs=mk, extra="theta", weights=(d.w, 2.0 * d.w))
    x2 = d.o.rollouts("x_control_costs")
    d.o.pi_set_rollout_costs(d.o.rollouts("state_costs"), d.w)
    d.o.pi_add_extra_rollout(d.o.theta(), np.zeros(p.N))
    np.testing.assert_allclose(x2, 2.0 * d.o.rollouts("x_control_costs"), rtol=1e-14, atol=0)
    assert len(d.get_rollouts(2)) == 7 and list(d.o.reuse_log()[0]).count(-1) <= 1
    d.set_costs(mk(2, range(7)))
    d.improve()
    d.add_extra(d.o.theta(), np.zeros(p.N))     # would rank first
    d.reset()
    assert len(d.get_rollouts(3)) == 12
    assert len(d.o.reuse_log()) == 1            # no ranking ran
    d.set_costs(mk(3, range(12)))
    d.improve()
    assert len(d.get_rollouts(4)) == 7
    assert -1 not in d.o.reuse_log()[-1]        # the extra rollout of iteration 2 was dropped


def test_non_finite_costs_are_refused_by_the_binding():
    p = su.zoo_problem("chain5", 12, 5)
    o = po.Oracle(p)
    o.pi_get_rollouts(1, su.sigma(p, 1))
    bad = np.zeros((12, p.N))
    bad[3, 4] = np.nan
    with pytest.raises(ValueError):
        o.pi_set_rollout_costs(bad, 1.0)
    with pytest.raises(ValueError):
        o.pi_add_extra_rollout(o.theta(), np.full(p.N, np.inf))
    with pytest.raises(ValueError):
        o.pi_get_rollouts(1, np.zeros(p.J + 1))
