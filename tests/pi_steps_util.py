"""Shared by tests/test_pi_steps.py (CPU) and tests/test_gpu_pi_steps.py (GPU): one driver that gives
the step oracle and, when there is one, an engine the same PolicyImprovement calls and compares
them after every step, and the crafted cost cases with their censuses.

Every census is asserted on an oracle alone, before anything is compared with it: the CPU file
asserts them as tests of their own, the GPU file again in front of each comparison.
"""
import functools

import numpy as np

from oracle import pyoracle as po
from tests import model_zoo as mz

X_FIELDS = ("x_params", "x_noise", "x_control_costs", "x_state_costs")


@functools.lru_cache(maxsize=None)
def zoo_problem(name, K, Kr, waypoints=40, terms=False, cumulative=False, max_iterations=None):
    """A zoo problem, built once per process (the tests only read it)."""
    kw = {}
    if cumulative:
        kw["use_cumulative_costs"] = True
    if max_iterations is not None:
        kw.update(max_iterations=max_iterations, max_iterations_after_collision_free=1000)
    if terms:
        return mz.TERMS_ZOO[name](K=K, Kr=Kr, waypoints=waypoints, **kw)
    return mz.ZOO[name](K=K, Kr=Kr, waypoints=waypoints, **kw)


def sigma(problem, it):
    """noise_stddev of iteration it, distinct in every joint and decaying at a distinct rate:
    base (1 + 0.25 d) (0.98^(d + 1))^(it - 1)."""
    d = np.arange(problem.J, dtype=np.float64)
    return problem.params.noise_stddev * (1.0 + 0.25 * d) * (0.98 ** (d + 1.0)) ** (it - 1)


def synthetic_costs(rng, rows, N, low=0.0, high=1.0):
    """State-cost rows that no execute made: finite, non-negative, rows and waypoints all distinct."""
    return rng.uniform(low, high, (rows, N)) ** 2


def walk(rng, theta, scale=0.01):
    """An extra rollout that is not theta: theta + scale * cumsum(standard normal)."""
    return theta + scale * np.cumsum(rng.standard_normal(theta.shape), axis=1)


def totals_in_reference_order(state, control):
    """Rollout::getCost (policy_improvement.cpp:149-156): the state sum, then each joint's control
    sum, every sum in index order."""
    out = []
    for k in range(state.shape[0]):
        v = float(state[k][0])
        for x in state[k][1:]:
            v += float(x)
        for row in control[k]:
            sd = float(row[0])
            for x in row[1:]:
                sd += float(x)
            v += sd
        out.append(v)
    return np.array(out)


class Driver:
    """The oracle and (optionally) an engine side by side.  Every step goes to both with the same
    inputs; what exists after the step is compared with assert_array_equal."""

    def __init__(self, problem, oracle=None, engine=None):
        self.p = problem
        self.o = oracle if oracle is not None else po.Oracle(problem)
        self.e = engine
        self.w = problem.params.smoothness_cost_weight
        self.K, self.Kr = problem.params.num_rollouts, problem.params.num_reused_rollouts
        self.K_gen = None
        self.it = 0
        self.tag = ""

    # ------------------------------------------------------------------ comparisons
    def _same(self, what, a, b):
        np.testing.assert_array_equal(b, a, err_msg=f"{self.tag} {what}")

    def compare(self, fields):
        if self.e is None:
            return
        for f in fields:
            self._same(f, self.o.rollouts(f), self.e.rollouts(f))

    def compare_theta(self):
        if self.e is not None:
            self._same("theta", self.o.theta(), self.e.theta())

    def compare_all(self, x_rows=True):
        """Everything a finished iteration leaves."""
        self.compare_theta()
        self.compare(("params", "noise", "control_costs", "state_costs", "probabilities"))
        if x_rows:
            self.compare(X_FIELDS)

    # ------------------------------------------------------------------ the five steps
    def get_rollouts(self, it, sig=None):
        self.it = it
        self.tag = f"it {it} get_rollouts"
        sig = sigma(self.p, it) if sig is None else np.asarray(sig, np.float64)
        ro = self.o.pi_get_rollouts(it, sig)
        if self.e is not None:
            re = self.e.pi_get_rollouts(it, sig)
            assert len(re) == len(ro), f"{self.tag}: K_gen {len(re)} != {len(ro)}"
            self._same("rollouts", ro, re)
        self.K_gen = len(ro)
        self.compare(("params", "noise"))
        self.compare_theta()
        return ro

    def execute(self, rows, member, source="engine"):
        """State costs of parameter rows from one source for both sides: the engine's execute (its
        parity with the oracle's is other files' job), or the oracle's."""
        rows = np.asarray(rows, np.float64).reshape(-1, self.p.J, self.p.N)
        if source == "engine" and self.e is not None:
            return self.e.execute(rows, iteration_member=member)[0]
        return np.stack([self.o.execute(r, iteration_member=member)[0] for r in rows])

    def set_costs(self, costs, weight=None):
        weight = self.w if weight is None else weight
        self.tag = f"it {self.it} set_rollout_costs({weight:g})"
        to = self.o.pi_set_rollout_costs(costs, weight)
        if self.e is not None:
            self._same("totals", to, self.e.pi_set_rollout_costs(costs, weight))
        self.compare(("params", "noise", "control_costs", "state_costs"))
        return to

    def improve(self):
        self.tag = f"it {self.it} improve_policy"
        uo = self.o.pi_improve_policy()
        if self.e is not None:
            self._same("update", uo, self.e.pi_improve_policy())
        self.compare(("probabilities",))
        self.compare_theta()   # untouched by improvePolicy
        return uo

    def set_theta(self, theta):
        self.o.set_theta(theta)
        if self.e is not None:
            self.e.set_theta(theta)
        self.compare_theta()

    def add_extra(self, params, costs):
        self.tag = f"it {self.it} add_extra_rollout"
        self.o.pi_add_extra_rollout(params, costs)
        if self.e is not None:
            self.e.pi_add_extra_rollout(params, costs)
        self.compare(X_FIELDS)

    def reset(self):
        self.o.pi_reset()
        if self.e is not None:
            self.e.pi_reset()

    # ------------------------------------------------------------------ fused calls
    def iterate(self, it):
        self.it = it
        self.tag = f"it {it} iterate"
        ro = self.o.iterate(it)
        if self.e is not None:
            assert self.e.iterate(it) == ro, self.tag
        self.compare_all(x_rows=self.Kr > 0)   # the fused iteration writes the x rows only with reuse
        return ro

    # ------------------------------------------------------------------ one iteration in steps
    def step_iteration(self, it, costs="engine", extra="theta", weights=None, rng=None, sig=None, theta=None):
        """runSingleIteration (policy_improvement_loop.cpp:143-202) in steps.
        costs: "engine" / "oracle" (that side's execute), or a function (it, rollouts) -> K_gen x N rows;
        extra: "theta", "walk" (theta + 0.01 cumsum(normal), executed), None (no addExtraRollouts), or a
        function (it, theta) -> (params, costs); weights: the control cost weights of successive
        setRolloutCosts calls (default: the problem's, once); theta: the parameters set after
        improvePolicy instead of theta + update.  Returns what the iteration was given and gave."""
        member = it - 1
        ro = self.get_rollouts(it, sig)
        c = costs(it, ro) if callable(costs) else self.execute(ro, member, costs)
        totals = None
        for wgt in (weights or (self.w,)):
            totals = self.set_costs(c, wgt)
        upd = self.improve()
        th = self.o.theta() + 1.0 * upd if theta is None else theta   # updateParameters
        self.set_theta(th)
        xp = xc = None
        if extra is not None:
            if callable(extra):
                xp, xc = extra(it, th)
            else:
                xp = th if extra == "theta" else walk(rng, th)
                xc = self.execute(xp, member, "oracle" if costs == "oracle" else "engine")[0]
            self.add_extra(xp, xc)
        return dict(rollouts=ro, costs=c, totals=totals, update=upd, theta=th, x_params=xp, x_costs=xc)


# ---------------------------------------------------------------------------- crafted costs
# Every crafted case is chain5 at N = 39 with synthetic state rows.  A case is a function
# run(driver) that drives the steps and asserts its census on driver.o; with an engine in the driver
# the same calls go to both sides, and the census assertions still read the oracle alone.

def _perm_rows(rng, base, rows):
    out = np.stack([rng.permutation(base) for _ in range(rows)])
    assert len({tuple(r) for r in out}) == rows, "the permuted rows must differ"
    return out


def ties_problem():
    return zoo_problem("chain5", 12, 5)


def run_exact_ties(d, groups=1):
    """noise_stddev 0: every row is theta and every control cost row the same; the state rows are
    permutations of small integers, so equal sums are exactly equal.  groups = 1: all 13 candidates
    tie, the kept rows are the extra rollout (index -1) then rows 0 .. 3.  groups = 2: rows 1, 3, 5
    tie below the other nine, and the extra rollout ties with the nine: kept 1, 3, 5, -1, 0."""
    p = d.p
    rng = np.random.default_rng(71)
    K, N, Kr = d.K, p.N, d.Kr
    assert (K, Kr) == (12, 5)
    base = np.arange(N, dtype=np.float64) % 7          # small integers: every partial sum exact
    worse = base + 1.0
    zero = np.zeros(p.J)
    good = (1, 3, 5) if groups == 2 else ()
    for it in (1, 2, 3):
        ro = d.get_rollouts(it, zero)
        theta = d.o.theta()
        assert all(np.array_equal(r, theta) for r in ro), "sigma 0: every generated row is theta"
        if it > 1:
            log = d.o.reuse_log()[-1]
            want = [1, 3, 5, -1, 0] if (groups == 2 and it == 2) else [-1, 0, 1, 2, 3]
            if groups == 2 and it == 3:
                # the second ranking: the three good rows now sit at 7, 8, 9; the extra ties the rest
                want = [7, 8, 9, -1, 0]
            assert list(log) == want, (it, log)
            st = d.o.rollouts("state_costs")
            for slot, src in enumerate(want):
                row = x_state if src == -1 else prev_state[src]
                assert np.array_equal(st[d.K_gen + slot], row), (it, slot, src)
        kg = d.K_gen
        rows = _perm_rows(rng, worse if groups == 2 else base, kg + 1)
        costs, x_state = rows[:kg].copy(), rows[kg].copy()
        if groups == 2 and it == 1:
            for r in good:
                costs[r] = rng.permutation(base)
        totals = d.set_costs(costs)
        if groups == 1:
            assert np.all(totals == totals[0]), totals
        else:
            best = totals.min()
            lo = np.flatnonzero(totals == best)
            assert list(lo) == ([1, 3, 5] if it == 1 else [7, 8, 9]), (it, totals)
            assert np.all(np.delete(totals, lo) == totals.max()), totals
        prev_state = d.o.rollouts("state_costs")
        upd = d.improve()
        assert not upd.any(), "zero noise: zero update"
        d.set_theta(theta + 1.0 * upd)
        d.add_extra(theta, x_state)
        # the extra rollout ties with the (worse) group: its total is that group's
        xt = totals_in_reference_order(x_state[None], d.o.rollouts("x_control_costs")[None])[0]
        assert xt == totals.max(), (xt, totals)


def rank_problem():
    return zoo_problem("chain5", 20, 10)


def run_extra_rank(d, where):
    """K + 1 = 21 candidates, K_r = 10: the extra rollout's total is made the best, the 9th, or
    worse than every kept row; reuse_log has -1 at position 0, at position 8, or nowhere."""
    p = d.p
    rng = np.random.default_rng(73)
    assert (d.K, d.Kr) == (20, 10)
    expect = {"best": 0, "ninth": 8, "worst": None}[where]

    def extra(it, theta):
        xp = walk(rng, theta)
        # its control costs under the kept weight: the oracle alone prices it once with zero state
        # costs (addExtraRollouts again below, on both sides, replaces that rollout)
        d.o.pi_add_extra_rollout(xp, np.zeros(p.N))
        cx = totals_in_reference_order(np.zeros((1, p.N)), d.o.rollouts("x_control_costs")[None])[0]
        t = np.sort(extra.totals)
        target = {"best": t[0] - 1.0, "ninth": 0.5 * (t[7] + t[8]), "worst": t[-1] + 1.0}[where]
        return xp, np.full(p.N, (target - cx) / p.N)

    for it in (1, 2, 3):
        out = d.step_iteration(it, costs=lambda it, ro: synthetic_costs(rng, len(ro), p.N, 0.5, 2.0), extra=None)
        extra.totals = out["totals"]
        assert len(set(out["totals"])) == d.K, "distinct totals"
        d.add_extra(*extra(it, out["theta"]))
        if it > 1:
            log = list(d.o.reuse_log()[-1])
            if expect is None:
                assert -1 not in log, log
            else:
                assert log.index(-1) == expect, log
    assert len(d.o.reuse_log()) == 2


def run_no_extra(d):
    """Three iterations without addExtraRollouts: the ranking has n = K candidates and no -1."""
    rng = np.random.default_rng(75)
    for it in (1, 2, 3):
        d.step_iteration(it, costs=lambda it, ro: synthetic_costs(rng, len(ro), d.p.N), extra=None)
    log = d.o.reuse_log()
    assert log.shape == (2, d.Kr) and (log >= 0).all(), log


def run_survivor(d):
    """Row 2 of iteration 1 costs nothing and everything else a lot: it is kept by three rankings
    in a row (source chain 2 -> 7 -> 7 with K_gen = 7), its parameters never change and its noise is
    re-based on the theta of each iteration."""
    p = d.p
    rng = np.random.default_rng(77)
    assert (d.K, d.Kr) == (12, 5)
    kept = None
    for it in (1, 2, 3, 4):
        def costs(it, ro):
            c = synthetic_costs(rng, len(ro), p.N, 3.0, 4.0)
            if it == 1:
                c[2] = 0.0
            return c
        out = d.step_iteration(it, costs=costs,
                               extra=lambda it, th: (th, synthetic_costs(rng, 1, p.N, 3.0, 4.0)[0]))
        prm, nz = d.o.rollouts("params"), d.o.rollouts("noise")
        if it == 1:
            kept = prm[2].copy()
        else:
            assert d.o.reuse_log()[-1][0] == (2 if it == 2 else 7), d.o.reuse_log()
            assert np.array_equal(prm[7], kept), "the survivor's parameters are copied, never changed"
            # re-based on the theta generateRollouts saw: the one the previous iteration left
            assert np.array_equal(nz[7], kept - theta_before), it
            assert nz[7].any()
        theta_before = out["theta"]
    assert [int(r[0]) for r in d.o.reuse_log()] == [2, 7, 7]


CRAFTED = {
    "ties_all": (ties_problem, lambda d: run_exact_ties(d, 1)),
    "ties_two_groups": (ties_problem, lambda d: run_exact_ties(d, 2)),
    "extra_best": (rank_problem, lambda d: run_extra_rank(d, "best")),
    "extra_ninth": (rank_problem, lambda d: run_extra_rank(d, "ninth")),
    "extra_worst": (rank_problem, lambda d: run_extra_rank(d, "worst")),
    "no_extra": (ties_problem, run_no_extra),
    "survivor": (ties_problem, run_survivor),
}
