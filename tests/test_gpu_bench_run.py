"""A plain `bench.py --gpus 1 --steps K --warmup W` run on the GPU: it times the headline only
(no legs, no CPU baseline, no side file), its line carries the headline keys, and --dump-outputs
writes what the last timed launch returned -- the same arrays, bit for bit, as the same queries
refined in this process through the same AsyncBatch path (the inputs are seeded by the global query
index)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fmpnp import _lib, refine as rf, synth  # noqa: E402  (no skip: a missing HIP library must fail)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS, WARMUP = 3, 4, 1


def test_plain_run_line_and_dumped_outputs(tmp_path):
    dump = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--batch", str(B), "--dump-outputs", str(dump)],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"].startswith("pose-refinements/sec") and line["unit"] == "pose-refinements/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (STEPS, WARMUP, 1)
    assert line["ms_per_step"] > 0
    # value = queries per step / seconds per step (both rounded in the line)
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3), rel=1e-2)
    assert line["legs"] == {} and "cpu_baseline" not in line and line["detail"]["path"] is None
    assert line["statuses"] == [0]
    assert os.listdir(tmp_path) == ["dump"]  # nothing else written where it ran

    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_run_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert sorted(os.listdir(dump)) == sorted(k + ".npy" for k in bench.DUMP_FIELDS)
    got = {k: np.load(dump / (k + ".npy")) for k in bench.DUMP_FIELDS}
    assert all(a.dtype == np.float64 and a.shape[0] == B for a in got.values())

    probs = []
    for q in range(B):
        inp = synth.problem_inputs(bench.N_PTS, bench.C, bench.HF, bench.WF, seed=q, device="cuda:0")
        f = rf.pack_features(inp["fmap"], storage=torch.float32, device="cuda:0")
        probs.append(rf.make_problem(f, inp["fref"], inp["pts3d"], inp["K"], inp["im_width"], inp["im_height"],
                                     inp["R0"], inp["t0"]))
        del inp
    ab = rf.AsyncBatch(probs, rf.make_options(bench.ITERS, 0.01, _lib.GEMAN_MCCLURE, dtype=_lib.F32))
    ab.launch()
    res = ab.results()
    for k in bench.DUMP_FIELDS:
        want = np.stack([np.asarray(x[k], dtype=np.float64) for x in res])
        np.testing.assert_array_equal(got[k], want, err_msg=k)
    assert all(x["status"] == 0 for x in res)
    # poses are rotations and the refinement moved them off the start
    for q in range(B):
        np.testing.assert_allclose(got["R"][q] @ got["R"][q].T, np.eye(3), atol=1e-12)
        assert got["best_cost"][q] < got["initial_cost"][q]
