"""bench.py's multi-rank launcher on the CPU (gloo): `bench.py --gpus 2` starts two ranks itself, shards each
step's global batch, gathers the controls (uint16 level ranks) and Φ* to rank 0 and reports n_gpus = 2, with
results identical to one rank solving the whole batch.  The per-rank solver here is the CPU oracle (test double);
on GPUs the same launcher / shard / gather code drives libmioc over RCCL."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(gpus, batch, total=0, steps=2, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--solver", "oracle", "--backend",
           "gloo", "--config", "C5", "--nt", "10", "--batch", str(batch), "--steps", str(steps), "--warmup", "1",
           "--no-cpu-baseline", "--total", str(total), *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_launcher_world2_matches_world1():
    two = _bench(2, 2)
    one = _bench(1, 4)
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["scaling"] == "weak"
    # the same global batch per step (world x batch = 4 restarts): identical controls and Φ*
    assert two["checksum"] == one["checksum"]
    assert two["value"] > 0 and one["value"] > 0


def test_launcher_strong_scaling_world2_matches_world1():
    """Strong scaling (`--total`, the mode of bench.py's batch_strong line): a fixed global batch per step split
    over the ranks -- 5 restarts as 3 + 2 on two ranks -- gives the same controls and Φ* as one rank solving all 5."""
    two = _bench(2, 1, total=5)
    one = _bench(1, 1, total=5)
    assert two["scaling"] == "strong" and one["scaling"] == "strong"
    assert two["checksum"] == one["checksum"]
    weak = _bench(1, 5)
    assert weak["checksum"] == one["checksum"] and weak["scaling"] == "weak"


def test_dump_outputs_repeatable(tmp_path):
    """`--dump-outputs DIR` writes the last timed step's results (here the test double's level ranks and Φ*) as
    float32 / float64 .npy files; the inputs are seeded, so a second run with the same arguments writes the same
    arrays.  `--steps` sets the number of timed steps and the line carries ms_per_step; a plain run carries none of
    the `--full` lines."""
    import numpy as np
    outs = []
    for d in ("a", "b"):
        line = _bench(1, 3, steps=3, extra=("--dump-outputs", str(tmp_path / d)))
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert abs(line["value"] * line["ms_per_step"] / 1e3 - 3) <= 1e-3 * 3  # 3 subproblems per step
        assert not [k for k in line if k.startswith(("batch", "single_", "variant", "cpu_baseline", "roofline"))]
        outs.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
        assert sorted(outs[-1]) == ["phi.npy", "ranks.npy"]
        assert outs[-1]["ranks.npy"].dtype == np.float32 and outs[-1]["ranks.npy"].shape == (3, 10)
        assert outs[-1]["phi.npy"].dtype == np.float64 and outs[-1]["phi.npy"].shape == (3,)
        assert float(outs[-1]["phi.npy"].sum()) + float(outs[-1]["ranks.npy"].sum()) == line["checksum"]
    for f in outs[0]:
        assert np.array_equal(outs[0][f], outs[1][f])


def test_dump_outputs_size_cap(tmp_path, monkeypatch):
    """An output over its share of the size limit is cut to a fixed sample: the same elements every time."""
    import numpy as np

    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 400)
    big = np.arange(1000, dtype=np.float64).reshape(10, 100) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"u": big, "status": np.zeros(4, dtype=np.int32)})
    a, b = np.load(tmp_path / "a" / "u.npy"), np.load(tmp_path / "b" / "u.npy")
    assert a.dtype == np.float64 and a.shape == (50,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and np.all(np.isin(a, big))
    st = np.load(tmp_path / "a" / "status.npy")
    assert st.dtype == np.float64 and st.shape == (4,)
