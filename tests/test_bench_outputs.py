"""`bench.py --dump-outputs DIR`: what the last timed step of each region returned, as float32 / float64 .npy files that two
builds can be compared with (the inputs are seeded); and `--steps` is the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sfm_danpipeline_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
NAMES = {"match_counts", "match_query_idx", "match_train_idx", "match_distance", "ba_cameras", "ba_points", "ba_focal", "ba_cost"}


def test_fewer_than_one_step_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_dumped_outputs_are_the_timed_steps_results(tmp_path, orc):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--lean", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3
    assert line["config"]["ba_timed_iterations"] == [16, 18]          # 15 untimed LM iterations, then exactly --steps timed ones
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == NAMES
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    # matching: the 1225 pairs of the cfg2 sweep, lists concatenated pair by pair; spot pairs against the oracle
    cnt = got["match_counts"]
    assert cnt.shape == (1225,) and int(cnt.sum()) == line["config"]["matches_found"]
    assert len(got["match_query_idx"]) == len(got["match_train_idx"]) == len(got["match_distance"]) == int(cnt.sum())
    imgs = synth.sift_image_set(50, 2000, 128, seed=1234)
    pairs = synth.all_pairs(50)
    off = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    for p in (0, 611, 1224):
        q, t, d = orc.match_knn2(imgs[pairs[p, 0]], imgs[pairs[p, 1]])
        sl = slice(off[p], off[p + 1])
        assert np.array_equal(got["match_query_idx"][sl], q) and np.array_equal(got["match_train_idx"][sl], t)
        assert np.array_equal(got["match_distance"][sl], d)
    # BA: the parameters after the timed LM iterations of cfg4, and the cost the line reports for them
    assert got["ba_cameras"].shape == (200, 6) and got["ba_points"].shape == (100000, 3) and got["ba_focal"].shape == (1,)
    assert np.all(np.isfinite(got["ba_points"])) and got["ba_focal"][0] > 0
    assert got["ba_cost"].tolist() == line["config"]["ba_cost"]


@pytest.mark.gpu
def test_a_plain_run_measures_the_headline_only():
    """Without --full the line carries the two timed regions and leaves every other leg out (null)."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["value"] > 0 and line["ba_iterations_per_s"] > 0 and line["ms_per_step"] > 0
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"] == "i8"
    assert line["config"]["ba_timed_iterations"] == [16, 17] and line["config"]["matches_found"] > 0
    full_only = ("sustained", "value_host_visible", "roofline", "roofline_ba", "ba_amdahl", "ba_batch", "cfg5_strong",
                 "find_best_pair_scoring", "sift_front_end", "adjust_bundle_call", "cpu_baseline")
    assert all(line[k] is None for k in full_only), {k: line[k] is None for k in full_only}
