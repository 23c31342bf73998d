"""Host logic of bench.py that shapes the driver's line (no GPU): the clock
settling loop's stopping rules, the algorithmic work model, and the output dump."""
import numpy as np

import bench


def _fake_chunks(durations):
    it = iter(durations)
    clock = [0.0]

    def now():
        return clock[0]

    def run_chunk():
        clock[0] += next(it)
    return now, run_chunk


def test_settle_stops_when_two_chunks_agree(monkeypatch):
    # a ramp 170 -> 147 us per iteration in 20-iteration chunks: stops at the
    # first pair within 1% once 50 ms have passed
    per_it = [170, 165, 160, 156, 152, 149, 147.5, 147.2, 147.1, 147.0] + [147.0] * 40
    now, run_chunk = _fake_chunks([x * 20e-6 for x in per_it])
    monkeypatch.setattr(bench.time, "perf_counter", now)
    r = bench.settle_clocks(run_chunk, 20)
    assert r["first_chunk_us_per_it"] == 170
    assert abs(r["last_chunk_us_per_it"] - 147.0) < 1e-9
    assert r["seconds"] >= 0.05
    n = r["iterations"] // 20
    assert abs(per_it[n - 1] - per_it[n - 2]) <= 0.01 * per_it[n - 2]


def test_settle_respects_the_time_cap(monkeypatch):
    # never agreeing chunks end at max_s
    per_it = [100 + (i % 2) * 50 for i in range(1000)]
    now, run_chunk = _fake_chunks([x * 20e-3 for x in per_it])
    monkeypatch.setattr(bench.time, "perf_counter", now)
    r = bench.settle_clocks(run_chunk, 20, max_s=1.0)
    assert r["seconds"] >= 1.0 and r["seconds"] < 1.0 + 150 * 20e-3


def test_settle_fixed_chunks_is_exact(monkeypatch):
    # strips that exchange every iteration: the same count on every rank
    now, run_chunk = _fake_chunks([1e-3] * 20)
    monkeypatch.setattr(bench.time, "perf_counter", now)
    assert bench.settle_clocks(run_chunk, 20, fixed_chunks=8)["iterations"] == 160


def test_c2_algorithmic_work_model():
    # 292 L K^2 flops and (18 L + 2) S bytes per node and iteration
    assert bench.algorithmic_flops_per_node("mixture", 1, 9) == 292 * 81
    assert bench.algorithmic_bytes_per_node("mixture", 1, 8) == 160


def test_dump_outputs_writes_every_array(tmp_path):
    # under the limit: every array whole, float64 (float32 kept), layout preserved
    outs = {"map": np.asfortranarray(np.arange(24.0).reshape(2, 3, 4)), "trace": np.ones((5, 3), np.float32),
            "its": np.array([3, 4])}
    rec = bench.dump_outputs(str(tmp_path / "d"), outs)
    assert not rec["sampled"] and sorted(rec["arrays"]) == ["its", "map", "trace"]
    for k, a in outs.items():
        b = np.load(tmp_path / "d" / f"{k}.npy")
        assert b.dtype == (np.float32 if k == "trace" else np.float64)
        np.testing.assert_array_equal(b, a)


def test_dump_outputs_samples_past_the_limit(tmp_path):
    # past the limit: a fixed seeded sample, the same from run to run, within the limit
    # (arrays under limit/1024 bytes stay whole)
    rng = np.random.default_rng(1)
    outs = {"a": rng.standard_normal((100, 70)), "b": rng.standard_normal(3000), "t": np.array([[7.0]])}
    r1 = bench.dump_outputs(str(tmp_path / "x"), outs, limit=16000)
    r2 = bench.dump_outputs(str(tmp_path / "y"), outs, limit=16000)
    assert r1["sampled"] and r1["arrays"] == r2["arrays"]
    total = 0
    for k, a in outs.items():
        x, y = np.load(tmp_path / "x" / f"{k}.npy"), np.load(tmp_path / "y" / f"{k}.npy")
        np.testing.assert_array_equal(x, y)
        if k == "t":
            np.testing.assert_array_equal(x, a)
        else:
            assert x.ndim == 1 and 0 < x.size < a.size and np.isin(x, a).all()
        total += x.nbytes
    assert total <= 16000
