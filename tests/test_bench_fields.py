"""bench.py's roofline fields (host logic only): the bound the evidence names and the rocprof-based
fraction beside the event-based one; what a plain run leaves out and how --dump-outputs writes."""
import numpy as np

import bench


def test_bound_from_evidence():
    # cfg2 round 4: 34.4 MB per 47.5 us launch (0.09 of 8 TB/s), VALU issue 0.39 -> latency
    assert bench.roofline_bound(34.4e6, 47.5e-6, {"frac_valu_issue": 0.39})[0] == "latency"
    assert bench.roofline_bound(350e6, 47.5e-6, {"frac_valu_issue": 0.39})[0] == "hbm"
    assert bench.roofline_bound(34.4e6, 47.5e-6, {"frac_valu_issue": 0.8})[0] == "valu"
    # no PMC summary of this build: priced against HBM, no claim
    assert bench.roofline_bound(None, 47.5e-6, {"frac_valu_issue": None}) == ("hbm", None)


def test_rocprof_fraction():
    f = bench.rocprof_fields({"rocprof_avg_ns": 45680.0}, 16.05e6)
    assert f["rocprof_avg_launch_us"] == 45.68
    assert abs(f["frac_rocprof"] - 16.05e6 / 45.68e-6 / 8e12) < 1e-5
    assert bench.rocprof_fields({}, 1.0) == {"rocprof_avg_launch_us": None, "frac_rocprof": None}


def test_plain_run_is_lean(monkeypatch):
    # without --full nothing runs beside the timed steps, whatever the other options say
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.no_timing and a.cpu_seconds == 0 and a.optimize_steps == 0
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and not a.no_timing and a.cpu_seconds == 12.0 and a.optimize_steps == 200
    assert a.dump_outputs == "d"


def test_dump_outputs(tmp_path):
    # float64 .npy per name; an array over the cap is the same seeded sample of its elements in
    # every run (ascending flat index), so two builds' dumps compare element for element
    small = np.arange(12, dtype=np.float32).reshape(3, 4)
    big = np.arange(bench.DUMP_ARRAY_BYTES // 8 + 1000, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, {"theta": small, "state_costs": big})
    got = np.load(tmp_path / "a" / "theta.npy")
    assert got.dtype == np.float64 and np.array_equal(got, small)
    s = np.load(tmp_path / "a" / "state_costs.npy")
    assert s.nbytes == bench.DUMP_ARRAY_BYTES and np.all(np.diff(s) > 0) and s[-1] < big.size
    assert np.array_equal(s, np.load(tmp_path / "b" / "state_costs.npy"))
    bench.dump_outputs(str(tmp_path / "a"), 1, {"theta": small})
    assert (tmp_path / "a" / "theta.rank1.npy").exists()


def test_shard_choice_explained(monkeypatch):
    # config.parallelism says why the ranks run their decomposition: the measured sums, the
    # environment's request, or the shape's only option
    class E:
        shard_info = {"t_gather": 51.4, "t_partials": 42.7, "l_allreduce": 20.0, "l_allgather_state": 22.0,
                      "l_allgather_partials": 21.0}
    why = bench.shard_why(E())
    assert "gather 51.4 + all-gather 22.0 = 73.4 us" in why and "= 104.7 us" in why
    E.shard_info = None
    monkeypatch.delenv("STOMP_SHARD_MODE", raising=False)
    assert "only decomposition" in bench.shard_why(E())
    monkeypatch.setenv("STOMP_SHARD_MODE", "partials")
    assert "STOMP_SHARD_MODE" in bench.shard_why(E())
