"""bench.py's stdout line stays small enough for the driver to parse it whole (round 4's 20.5 KB
line was cut to its last 8 KB and left unparsed): the headline keys plus one summary per leg,
every leg's full record in a side file referenced by path and sha256."""
import hashlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_line_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _canned():
    # the full round-4 default line (every leg, 20.5 KB) as the canned result set
    with open(os.path.join(ROOT, "profiles", "r04_bench_default.json")) as f:
        return json.load(f)


def test_compact_line_fits_and_keeps_the_headline(tmp_path):
    bench = _bench()
    full = _canned()
    full["facade_call"] = {"cfg2": {"ms_per_call": 1.234, "calls_per_s": 810.4},
                           "robotcar_n295": {"ms_per_call": 2.5, "calls_per_s": 400.0}}
    ref = bench.write_detail(full, str(tmp_path / "d" / "bench_detail.json"))
    line = bench.compact_line(full, ref)
    text = json.dumps(line)
    assert len(text) <= bench.LINE_MAX_BYTES, len(text)
    assert len(text) <= 12000
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config",
              "roofline", "cpu_baseline", "gn_iters_per_s", "statuses"):
        assert k in line, k
    assert line["value"] == full["value"] and line["metric"] == full["metric"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    assert "legs_dropped" not in line
    legs = line["legs"]
    for k in ("single_query", "hard_init", "hard_init_ratio08", "ratio08", "layout_f", "end_to_end",
              "end_to_end.full_pack", "end_to_end.robotcar_1664", "pyramid_robotcar_1664",
              "pyramid_robotcar_1664.median_query_n295", "fixed_total_1024", "no_memo", "pack",
              "facade_call.cfg2", "facade_call.robotcar_n295"):
        assert k in legs, k
        assert "ms" in legs[k] or "rate" in legs[k], (k, legs[k])
    assert legs["hard_init"]["frac"] == full["hard_init"]["roofline"]["frac"]
    assert legs["facade_call.cfg2"]["ms"] == 1.234
    # the side file is what the line names
    with open(ref["path"], "rb") as f:
        blob = f.read()
    assert hashlib.sha256(blob).hexdigest() == ref["sha256"] and len(blob) == ref["bytes"]
    assert json.loads(blob)["pyramid_robotcar_1664"] == full["pyramid_robotcar_1664"]


def test_compact_line_drops_legs_before_the_headline():
    bench = _bench()
    full = _canned()
    for i in range(400):  # far more legs than fit
        full[f"extra_leg_{i}"] = {"ms_per_launch": 1.0, "pose_refinements_per_s": 2.0, "roofline": {"frac": 0.5}}
    line = bench.compact_line(full, {"path": None})
    assert len(json.dumps(line)) <= bench.LINE_MAX_BYTES
    assert line["legs_dropped"] > 0 and line["roofline"]["frac"] == full["roofline"]["frac"]
    assert "cpu_baseline" in line and "single_query" in line["legs"]


def test_plain_run_has_no_legs_and_full_has_them():
    """A plain run times the headline only; the legs (CPU baselines, other configurations, the
    pipeline, ...) run with --full, all of them unless --legs names some."""
    bench = _bench()
    plain = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not plain.full and plain.legs == set() and plain.dump_outputs is None
    assert (plain.steps, plain.warmup) == (7, 2)
    assert bench.parse(["--legs", "pack,cpu"]).legs == set()  # --legs alone selects nothing
    full = bench.parse(["--full"])
    assert full.full and full.legs == set(bench.LEGS) and "cpu" in full.legs
    assert bench.parse(["--full", "--legs", "pack,cpu"]).legs == {"pack", "cpu"}
    assert bench.parse(["--full", "--legs", "none"]).legs == set()
    assert bench.parse(["--dump-outputs", "somewhere"]).dump_outputs == "somewhere"


def test_dump_outputs_writes_one_float64_array_per_field(tmp_path):
    import numpy as np
    bench = _bench()
    rng = np.random.default_rng(0)
    res = [dict(R=rng.standard_normal((3, 3)), t=rng.standard_normal(3), initial_cost=1.5 + q, best_cost=0.25 * q,
                final_lambda=1e-3, final_lr=1.0, best_num_inliers=500 + q, n_evals=51, n_steps=50, n_accepted=40 + q,
                status=0, has_best=True, texel_gathers=12345 + q) for q in range(5)]
    d = tmp_path / "out" / "dump"
    paths = bench.dump_outputs(res, str(d))
    assert sorted(os.path.basename(p) for p in paths) == sorted(os.listdir(d)) == \
        sorted(k + ".npy" for k in bench.DUMP_FIELDS)
    got = {k: np.load(d / (k + ".npy")) for k in bench.DUMP_FIELDS}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["R"].shape == (5, 3, 3) and got["t"].shape == (5, 3) and got["best_cost"].shape == (5,)
    for q, r in enumerate(res):
        assert np.array_equal(got["R"][q], r["R"]) and np.array_equal(got["t"][q], r["t"])
        assert got["initial_cost"][q] == r["initial_cost"] and got["n_accepted"][q] == r["n_accepted"]
    assert got["has_best"].tolist() == [1.0] * 5
    # several ranks: one set of files per rank
    paths = bench.dump_outputs(res[:2], str(d), rank=1, world=2)
    assert all(p.endswith("_rank1.npy") for p in paths) and np.load(d / "t_rank1.npy").shape == (2, 3)
