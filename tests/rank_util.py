"""Shared by tests/test_gpu_rank_space.py: W ranks of one K-sharded problem as W engines of one
process, one host thread each, beside one oracle of the whole K (tests/SHARDED_RANKS.md).

Every rank's drive function makes the same engine calls and asserts nothing: a rank that stopped
early would leave the others in the exchange group's barrier.  It returns records (dicts of
arrays), and compare_records holds every rank's record to the oracle's after the threads joined.
The censuses read the oracle's records alone.
"""
import concurrent.futures as cf
import os

import numpy as np

from oracle import pyoracle as po
from stomp_motion_planner_icra2011_amd import engine as eng
from tests import model_zoo as mz

THREADS = int(os.environ.get("OMP_NUM_THREADS") or 8)
MODES = ["partials", "gather"]
ROW_FIELDS = ("params", "noise", "control_costs", "state_costs", "probabilities")
X_FIELDS = ("x_params", "x_noise", "x_control_costs", "x_state_costs")

# weights_kernel (k_weights.hip) for the row tiles: the instantiation by the rows of the launch.
# The sharded phases (fused = false) take it at every K_loc, the fused launch above 64 rows.
ROWS_KERNELS = [(256, "rows<256,4,4>"), (512, "rows<512,4,4>"), (1024, "rows<512,4,8>"), (2048, "rows<256,4,32>"),
                (4096, "rows<256,2,32>")]


def rows_kernel(rows):
    return next(name for top, name in ROWS_KERNELS if rows <= top)


def make_ranks(p, world, mode, monkeypatch, **kw):
    """The W engines of one in-process exchange group (mode None: the engine's default rule)."""
    if mode is None:
        monkeypatch.delenv("STOMP_SHARD_MODE", raising=False)
        monkeypatch.delenv("STOMP_DEBUG_CALIBRATE_LOCAL", raising=False)
    else:
        monkeypatch.setenv("STOMP_SHARD_MODE", mode)
    gid = eng.comm_local_id(world)
    engines = []
    try:
        for r in range(world):
            engines.append(eng.Engine(p, rank=r, world_size=world, comm_id=gid, **kw))
    except Exception:
        close_all(engines)
        raise
    return engines


def close_all(engines):
    for e in engines:
        e.close()


def on_threads(engines, fn):
    with cf.ThreadPoolExecutor(len(engines)) as ex:
        futs = [ex.submit(fn, r, e) for r, e in enumerate(engines)]
        return [f.result(timeout=300) for f in futs]


def model_lines(capfd):
    """The engines' own accounts of what creation chose (STOMP_DEBUG_LEAN_PRINT), one per engine
    created since the last call."""
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("stomp: model ")]
    assert lines, err
    return lines


def assert_creation(engines, lines, K, mode, weights=None, body=None):
    """What every rank's creation chose, before anything is compared: its shard, the decomposition,
    the weights kernel of its launch (partials: the K_loc rows of the phases; gather: all K rows,
    fused) and, where the case depends on it, the rollout body."""
    W = len(engines)
    K_loc = K // W
    assert len(lines) == W, lines
    for r, (e, line) in enumerate(zip(engines, lines)):
        assert (e.first, e.K_loc, e.shard_mode) == (r * K_loc, K_loc, mode), (r, e.first, e.K_loc, e.shard_mode)
        want = weights or rows_kernel(K_loc if mode == "partials" else K)
        assert line.endswith("weights " + want), (r, line)
        assert f"launch of {K_loc + 1} rollouts: " in line, line
        if body is not None:
            assert f"launch of {K_loc + 1} rollouts: {body}," in line, line


def snapshot(x, cost=None, fields=ROW_FIELDS):
    """Everything an iteration leaves, of an engine (its K_loc rows) or the oracle (all K)."""
    rec = dict(theta=x.theta(), last=x.last_trajectory())
    if cost is not None:
        rec["cost"] = np.array([cost[0], float(cost[1])])
    for f in fields:
        rec[f] = x.rollouts(f)
    return rec


def iterate_records(x, iterations, fields=ROW_FIELDS):
    return [snapshot(x, x.iterate(it), fields) for it in iterations]


def freeze(recs):
    """Records that several cases share: their arrays refuse writes."""
    for rec in recs:
        for v in rec.values():
            v.setflags(write=False)
    return recs


def compare_records(recs, orecs, K_loc, tag=""):
    """recs[rank][step] against orecs[step]: replicated values whole, row fields on the rank's
    slice [r K_loc, (r + 1) K_loc) of the oracle's."""
    for r, rank_recs in enumerate(recs):
        assert len(rank_recs) == len(orecs), (r, len(rank_recs), len(orecs))
        for k, (rec, orec) in enumerate(zip(rank_recs, orecs)):
            assert sorted(rec) == sorted(orec), (sorted(rec), sorted(orec))
            for f, v in orec.items():
                want = v[r * K_loc:(r + 1) * K_loc] if f in ROW_FIELDS else v
                np.testing.assert_array_equal(rec[f], want, err_msg=f"{tag} step {k} rank {r} {f}")


_ORACLE_RECORDS = {}


def oracle_records(p, iterations, fields, key=None, default_census=True):
    """The oracle's records of a case, made once per process for the cases that name the same key
    (the two decompositions of one problem); their arrays are read-only.  The censuses of the inputs
    are asserted as they are made: the default trajectory's (unless default_census is False: the
    short and long N, whose default trajectory need not touch the scene) and the rollouts' own."""
    if key is None or key not in _ORACLE_RECORDS:
        o = po.Oracle(p, threads=THREADS)
        if default_census:
            assert_default_census(p, o.theta())
        recs = freeze(iterate_records(o, iterations, fields))
        assert_rollout_census(p, recs)
        if key is None:
            return recs
        _ORACLE_RECORDS[key] = recs
    return _ORACLE_RECORDS[key]


def run_case(p, world, mode, monkeypatch, capfd, iterations=(1, 2, 3), census=None, weights=None, body=None,
             key=None, expect=(), default_census=True, **engine_kw):
    """The common case: creation choices asserted (expect: further pieces of every rank's model
    line), the censuses asserted on the problem and on the oracle's records, then every rank's
    records compared.  Returns (rank records, oracle records)."""
    monkeypatch.setenv("STOMP_DEBUG_LEAN_PRINT", "1")
    K = p.params.num_rollouts
    # with reuse the extra rollout's rows exist too: replicated, every rank evaluates it
    fields = ROW_FIELDS + (X_FIELDS if p.params.num_reused_rollouts > 0 else ())
    orecs = oracle_records(p, iterations, fields, key, default_census)
    if census is not None:
        census(orecs)
    engines = make_ranks(p, world, mode, monkeypatch, **engine_kw)
    try:
        lines = model_lines(capfd)
        assert_creation(engines, lines, K, mode, weights, body)
        for piece in expect:
            assert all(piece in l for l in lines), (piece, lines)
        recs = on_threads(engines, lambda r, e: iterate_records(e, iterations, fields))
    finally:
        close_all(engines)
    compare_records(recs, orecs, K // world, tag=f"W {world} {mode}")
    return recs, orecs


def assert_default_census(p, theta):
    """The default trajectory touches the scene: lookups in collision and in the hinge zone."""
    c = mz.census(p, theta[None])
    assert c["collision"] >= 1 and c["hinge"] >= 1, c


def assert_rollout_census(p, orecs, rows=(0, 1, 2, -2, -1)):
    """What the compared rollouts themselves reach, on the oracle's own parameter rows of the first
    iteration (the first rows of rank 0 and the last of the last rank): lookups in collision, in
    the hinge zone and in free space."""
    c = mz.census(p, orecs[0]["params"][list(rows)])
    assert c["collision"] >= 1 and c["hinge"] >= 1 and c["free"] >= 1, c


# ---------------------------------------------------------------------------- the reuse census

def reuse_census(orecs, x_states, K, K_r, K_loc):
    """From the oracle's rows alone.  orecs[i]: the records of successive iterations; x_states[i]:
    the extra rollout's state row after iteration i (the noiseless rollout of the updated theta).
    Rows K_gen.. of an iteration after the first are reused: each is recognised among the previous
    iteration's rows, or as the previous extra rollout, by its state row.  Returns
    dict(sources=[[(destination row, source row or -1)]], crossed, extra_kept, foreign_generated):
    crossed counts reused rows whose source row another rank owned, foreign_generated rows of ranks
    other than 0 that match no previous row."""
    K_gen = K - K_r
    out = dict(sources=[], crossed=0, extra_kept=0, foreign_generated=0)
    for i in range(1, len(orecs)):
        prev, cur = orecs[i - 1]["state_costs"], orecs[i]["state_costs"]
        index = {}
        for k in range(K):
            key = prev[k].tobytes()
            assert key not in index, f"iteration {i}: previous rows {index[key]} and {k} have one state row"
            index[key] = k
        xkey = x_states[i - 1].tobytes()
        assert xkey not in index, f"iteration {i}: the extra rollout's state row is also row {index[xkey]}'s"
        index[xkey] = -1
        src = []
        for d in range(K):
            s = index.get(cur[d].tobytes())
            if s is None and d >= K_loc:
                out["foreign_generated"] += 1
            if d < K_gen:
                assert s is None, f"iteration {i}: generated row {d} repeats previous row {s}"
                continue
            assert s is not None, f"iteration {i}: reused row {d} matches no previous row"
            src.append((d, s))
            if s == -1:
                out["extra_kept"] += 1
            elif s // K_loc != d // K_loc:
                out["crossed"] += 1
        assert len({s for _, s in src}) == K_r, "every candidate is kept at most once"
        out["sources"].append(src)
    return out
