"""bench.py driver contract: one JSON line on stdout with the required
schema (the round driver parses exactly this)."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {"metric": str, "value": float, "unit": str, "n_gpus": int,
            "steps": int, "warmup": int, "ms_per_step": float,
            "higher_is_better": bool, "scaling": str, "dtype": str,
            "data": str, "config": dict}


def _run(args):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py")] + args,
        capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_json_contract_acco():
    d = _run(["--steps", "2", "--warmup", "1"])
    for k, t in REQUIRED.items():
        assert k in d, f"missing {k}"
        assert isinstance(d[k], t), (k, type(d[k]))
    assert "vs_baseline" in d            # null allowed (no published baseline)
    assert d["metric"] == "tokens/s"
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["data"] == "synthetic"
    cfg = d["config"]
    for k in ("model", "method", "global_batch", "seq_len", "parallelism"):
        assert k in cfg


def test_bench_json_contract_ddp():
    d = _run(["--method", "ddp", "--steps", "2", "--warmup", "1"])
    assert d["config"]["method"] == "ddp"
    assert d["value"] > 0


def test_bench_json_contract_dpu():
    d = _run(["--method", "dpu", "--steps", "2", "--warmup", "1"])
    assert d["config"]["method"] == "dpu"
    assert d["value"] > 0


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs saves the last timed step's loss / params / grads as
    float32 .npy, and two runs with the same arguments produce the same
    arrays. (dpu is the sequential method: ACCO's micro-batch count per
    round depends on thread timing on the CPU.) The second run also passes
    --full, which must leave the result line and the outputs as they are."""
    import numpy as np
    base = ["--method", "dpu", "--model", "tiny", "--steps", "2", "--warmup", "1"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    da = _run(base + ["--dump-outputs", a])
    db = _run(base + ["--full", "--dump-outputs", b])
    assert set(da) == set(db) and da["config"].keys() == db["config"].keys()
    assert sorted(os.listdir(a)) == ["grads.npy", "loss.npy", "params.npy"]
    assert sorted(os.listdir(b)) == sorted(os.listdir(a))
    total = 0
    for name in os.listdir(a):
        xa, xb = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        assert xa.dtype == np.float32 and xa.size > 0
        assert np.isfinite(xa).all()
        if da["dtype"] == "fp32":
            assert np.array_equal(xa, xb), name
        else:
            # bf16 on a GPU: atomic reductions change the summation order
            # (float32-level noise), which can flip the bf16 rounding of a
            # few elements by one ulp each; the whole array stays well
            # within one bf16 epsilon (2^-8) in relative l2 norm
            err = np.linalg.norm(xa.astype(np.float64) - xb)
            assert err <= 2.0 ** -8 * np.linalg.norm(xa.astype(np.float64)), name
        total += xa.nbytes
    assert total <= 64 * 2**20
    assert np.load(os.path.join(a, "loss.npy")).shape == (1,)
    assert np.load(os.path.join(a, "params.npy")).size == da["config"]["params"]
    assert np.abs(np.load(os.path.join(a, "grads.npy"))).max() > 0


def test_bench_dump_sample_is_fixed():
    """An array longer than the sample size is reduced to the same sorted
    indices on every call."""
    import importlib.util
    import tempfile

    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location(
        "bench", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.DUMP_SAMPLE + 12345
    x = torch.arange(n, dtype=torch.float32)
    with tempfile.TemporaryDirectory() as d:
        bench.dump_outputs(d, {"x": x})
        s1 = np.load(os.path.join(d, "x.npy"))
        bench.dump_outputs(d, {"x": x * 2})
        s2 = np.load(os.path.join(d, "x.npy"))
    assert s1.dtype == np.float32 and s1.shape == (bench.DUMP_SAMPLE,)
    assert (np.diff(s1) >= 0).all() and s1.max() < n
    assert np.array_equal(s2, 2 * s1)


def test_bench_multirank_launch_contract():
    """The driver's N>1 launch shape: torch.distributed.run --nnodes=1
    --nproc-per-node 2 bench.py --gpus 2 ... (gloo on CPU here; RCCL on a
    GPU node). Rank 0 must emit exactly one whole-job JSON line with
    n_gpus=2 and the SUM-over-ranks token throughput."""
    env = dict(os.environ)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29611", os.path.join(REPO, "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=600, cwd=REPO, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["config"]["global_batch"] == 2 * 8
    assert d["value"] > 0


def test_bench_refuses_mislabeled_gpus_flag():
    """--gpus that contradicts WORLD_SIZE must refuse (exit 2), not emit a
    mislabeled record."""
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "4",
         "--steps", "1", "--warmup", "1"],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 2
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_bench_json_contract_ckpt_flag():
    """--ckpt (activation checkpointing) runs and is recorded in config."""
    d = _run(["--steps", "2", "--warmup", "1", "--ckpt"])
    assert d["config"]["ckpt"] is True
    assert d["value"] > 0
