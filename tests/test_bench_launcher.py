"""bench.py's own multi-rank launcher: `bench.py --gpus 2`
without WORLD_SIZE starts two ranks through torch.distributed.run, shards the global batch on
whole states, and selects the global minimum with ONE all-gather of the selection records.
Run on CPU over gloo with --selection-dry-run (seeded synthetic costs replace the GPU solve),
so the launcher, the sharding and the selection are exactly the code the GPU run executes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _run(world, G, seed=11, extra=()):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env["OMP_NUM_THREADS"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world),
           "--selection-dry-run", "--steps", "2", "--warmup", "1", "--global-batch", str(G),
           "--seed", str(seed), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout  # ONE JSON line, from rank 0
    return json.loads(lines[0])


@pytest.mark.parametrize("world,G", [(1, 4096), (2, 4096), (3, 4097 * 16)])
def test_bench_launcher_global_argmin(world, G):
    """(3, 4097 x 16): an uneven state split, 1366 / 1366 / 1365 states over three ranks"""
    sys.path.insert(0, ROOT)
    import bench
    from mpcqp.dist import host_select

    seed = 11
    r = _run(world, G, seed)
    assert r["n_gpus"] == world
    assert r["scaling"] == "strong" and r["config"]["global_batch"] == G
    assert r["config"]["parallelism"] == f"dp{world}"
    # host reference over the whole batch: the synthetic costs are a function of the index
    cost, status, _ = bench.synthetic_shard(G, 60, seed, 0, 0)
    c0, i0 = host_select(cost, status)
    assert r["config"]["selected"]["index"] == i0
    assert r["config"]["selected"]["cost"] == pytest.approx(c0)


def test_shards_cover_whole_states():
    sys.path.insert(0, ROOT)
    import bench
    for S, w in ((4096, 8), (4097, 8), (10, 3)):
        cover = []
        for r in range(w):
            s0, n = bench.shard(S, w, r)
            cover.extend(range(s0, s0 + n))
        assert cover == list(range(S))


def test_bench_line_records_the_formed_group():
    """the line names the world size the process group formed, each rank's
    device and shard, and both the pipelined and the serial-selection step times (the serial
    pass is one of the `--full` measurements)"""
    r = _run(2, 4096, extra=("--full",))
    cfg = r["config"]
    pg = cfg["process_group"]
    assert pg["world_size"] == 2 and pg["backend"] == "gloo"
    ranks = sorted(pg["ranks"], key=lambda x: x["rank"])
    assert [x["rank"] for x in ranks] == [0, 1]
    assert [x["local_rank"] for x in ranks] == [0, 1]
    assert all(x["device"] == "cpu" for x in ranks)  # dry run; cuda:<local_rank> on the GPU box
    assert ranks[0]["shard"] == [0, 2048] and ranks[1]["shard"] == [2048, 4096]
    assert cfg["shards_cover_global_batch"] is True
    assert cfg["pipelined_ms_per_step"] == pytest.approx(r["ms_per_step"])
    assert cfg["serial_select_ms_per_step"] > 0


def _load_dump(path):
    out = {f[:-4]: np.load(os.path.join(path, f), allow_pickle=False) for f in os.listdir(path)}
    assert all(a.dtype == np.float64 for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64e6
    return out


def test_plain_line_and_dump_outputs_dry_run(tmp_path):
    """a plain run prints the headline fields and none of the `--full` measurements, and
    `--dump-outputs` writes the shard's arrays and the decoded selection, the same on a rerun"""
    sys.path.insert(0, ROOT)
    import bench
    from mpcqp.dist import host_select

    G, seed = 4096, 11
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _run(2, G, seed, extra=("--dump-outputs", a))
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["unit"] == "QP/s"
    assert r["value"] == pytest.approx(G / (r["ms_per_step"] * 1e-3))
    assert "serial_select_ms_per_step" not in r["config"] or \
        r["config"]["serial_select_ms_per_step"] is None
    assert not {"roofline", "cpu_baseline"} & set(r) and "per_config" not in r["config"]
    _run(2, G, seed, extra=("--dump-outputs", b))
    da, db = _load_dump(a), _load_dump(b)
    assert sorted(da) == sorted(f"{k}_rank{i}" for k in ("U", "cost", "selected", "status")
                                for i in (0, 1))
    assert all(np.array_equal(da[k], db[k]) for k in da)
    cost, status, U = bench.synthetic_shard(G, 60, seed, 0, 0)
    assert np.array_equal(np.concatenate([da["U_rank0"], da["U_rank1"]]), U)
    assert np.array_equal(np.concatenate([da["cost_rank0"], da["cost_rank1"]]), cost)
    c0, i0 = host_select(cost, status)
    for k in ("selected_rank0", "selected_rank1"):  # every rank holds the global selection
        assert da[k][0] == i0 and da[k][1] == pytest.approx(c0)
        assert np.array_equal(da[k][2:], U[i0])


def test_dump_outputs_samples_rows_above_the_limit(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    assert bench.DUMP_LIMIT_BYTES <= 64e6
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)  # the same code at a small limit
    B = 3 * bench.DUMP_LIMIT_BYTES // (8 * 8)
    arrays = dict(U=np.arange(B * 6, dtype=np.float64).reshape(B, 6), cost=np.arange(B) * 0.5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, np.zeros(8))
    da, db = _load_dump(str(tmp_path / "a")), _load_dump(str(tmp_path / "b"))
    rows = da["rows"].astype(np.int64)
    assert 0 < len(rows) < B and np.all(np.diff(rows) > 0)
    assert np.array_equal(da["U"], arrays["U"][rows]) and np.array_equal(da["cost"], rows * 0.5)
    assert all(np.array_equal(da[k], db[k]) for k in da)


@pytest.mark.gpu
def test_plain_bench_dumps_what_the_timed_path_computed(gpu, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` on the device: the dumped
    arrays are, bit for bit, what mpcqp_batch_solve_select leaves for the same seeded batch"""
    import mpcqp
    from mpcqp.dist import decode_record
    from mpcqp.engine import BatchEngine

    G, seed = 1040, 20250404  # 65 states: an odd number of paired workgroups' worth
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--global-batch", str(G), "--seed", str(seed),
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["dtype"] == "f64" and r["n_gpus"] == 1
    assert r["value"] == pytest.approx(G / (r["ms_per_step"] * 1e-3))
    assert not {"roofline", "cpu_baseline"} & set(r)
    assert not {"per_config", "kernel_ms", "per_tick_latency"} & set(r["config"])
    assert r["config"]["solved_frac"] == 1.0
    p = mpcqp.model_params("B")
    eng = BatchEngine(p, device=0)
    d = eng.upload(mpcqp.make_batch(p, G, seed=seed))
    rec = gpu.zeros(1 + eng.nV, dtype=gpu.int64, device="cuda:0")
    eng.solve_select(d, rec)
    eng.sync()
    got = _load_dump(str(tmp_path))
    assert sorted(got) == ["U", "cost", "iters", "selected", "status"]
    for k in ("U", "cost", "status", "iters"):
        assert np.array_equal(got[k], d[k].cpu().numpy().astype(np.float64)), k
    c, i, U = decode_record(rec.cpu().numpy())
    eng.close()
    assert got["selected"][0] == i == r["config"]["selected"]["index"]
    assert got["selected"][1] == c and np.array_equal(got["selected"][2:], U)
