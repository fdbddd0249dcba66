"""bench.py --gpus N without a launcher starts its N rank processes itself
(one per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, never exec),
relays rank 0's JSON line and fails when a rank fails.  CPU dry run over
gloo: the launch and timing contract without a device."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, timeout=180):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "2",
                           "--warmup", "1", *extra], capture_output=True, text=True, timeout=timeout, env=env)


def test_launcher_starts_n_ranks():
    p = _run("--gpus", "2")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2
    assert line["ranks_seen"] == 2
    assert line["ranks"] == [0, 1]
    assert line["steps"] == 2 and line["ms_per_step"] > 0


def test_launcher_single_rank_runs_inline():
    p = _run("--gpus", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["ranks"] == [0]


def test_launcher_fails_when_a_rank_fails():
    p = _run("--gpus", "2", "--dry-fail-rank", "1")
    assert p.returncode != 0


def test_dump_outputs_repeatable(tmp_path):
    """A plain run: --steps sets the timed steps, the line holds the headline
    keys and no other config; --dump-outputs DIR: float32 / float64 .npy
    files, the same from run to run with the same arguments."""
    import numpy as np
    dumps = []
    for k in range(2):
        d = tmp_path / ("dump%d" % k)
        p = _run("--gpus", "1", "--steps", "3", "--dump-outputs", str(d))
        assert p.returncode == 0, p.stderr[-2000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["warmup"] == 1 and "configs" not in line
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert line[key] is not None, key
        files = sorted(os.listdir(d))
        assert files and all(f.endswith(".npy") for f in files)
        dumps.append({f: np.load(d / f) for f in files})
    assert dumps[0].keys() == dumps[1].keys()
    for f, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64) and a.nbytes <= 64e6
        assert np.array_equal(a, dumps[1][f]), f
    assert (dumps[0]["dry_run.npy"] == 4.0).all()   # 1 warm-up + 3 timed adds


def test_other_configs_need_full():
    p = _run("--gpus", "1", "--only", "c1")
    assert p.returncode == 2 and "--full" in p.stderr


def test_sample_rgba_is_seeded():
    """The RGBA sample of --dump-outputs: the same pixels on every draw, each
    read back from the batch, and exact per-tile channel sums."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    rng = np.random.default_rng(7)
    rgba = rng.integers(0, 256, (5, 8, 6, 4), dtype=np.uint8)
    a = bench.sample_rgba(torch.from_numpy(rgba), n_pixels=64)
    b = bench.sample_rgba(torch.from_numpy(rgba.copy()), n_pixels=64)
    assert sorted(a) == ["rgba_sample", "rgba_sample_pixel", "rgba_tile_sums"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    idx = a["rgba_sample_pixel"].astype(np.int64)
    assert idx.shape == (64,) and (idx >= 0).all() and (idx < 5 * 8 * 6).all()
    assert np.array_equal(a["rgba_sample"], rgba.reshape(-1, 4)[idx].astype(np.float32))
    assert np.array_equal(a["rgba_tile_sums"], rgba.reshape(5, -1, 4).sum(axis=1).astype(np.float64))
    whole = bench.sample_rgba(torch.from_numpy(rgba), n_pixels=1 << 20)
    assert np.array_equal(whole["rgba_sample"], rgba.reshape(-1, 4).astype(np.float32))
