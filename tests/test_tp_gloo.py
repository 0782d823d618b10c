"""Multi-process (gloo, world_size 2 and 4, CPU) test of the tensor-parallel sharding logic
(paroquant_amd/tp.py; reference vllm/plugin.py:33-50,196-198).  The per-rank linear is evaluated by
the CPU oracle here (the HIP path needs a GPU); what is under test is the sharding of the
checkpoint tensors, the narrowing of the rotation parameters and the all-reduce placement."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import paro_oracle as po


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _apply_oracle(layer, x):
    y = po.paro_linear_merged(x.numpy(), layer["qweight"].numpy(), layer["qzeros"].numpy(), layer["scales"].numpy(),
                              layer["theta"].numpy(), layer["pairs"].numpy(), layer["channel_scales"].numpy(),
                              layer["sizes"], None if layer.get("bias") is None else layer["bias"].numpy(), ideal=True)
    return torch.from_numpy(np.ascontiguousarray(y))


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from paroquant_amd import tp
        from paroquant_amd.vllm_plugin import _maybe_shard_input
        K, sizes = 512, [128, 64, 64]
        L = po.make_layer(5, K, sizes, bias=True)
        layer = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in L.items()}
        x = torch.from_numpy(np.random.default_rng(1).standard_normal((3, K)))
        full = _apply_oracle(layer, x)

        # column parallel: each rank holds N/world columns of every merged partition, full rotation
        col = tp.shard_column_parallel(layer, sizes, rank, world)
        y_local = _apply_oracle(col, x)
        gathered = [torch.empty_like(y_local) for _ in range(world)]
        dist.all_gather(gathered, y_local)
        pieces, off = [], 0
        for n in sizes:           # re-interleave [rank][partition] -> [partition][rank]
            per = n // world
            pieces += [g[:, off:off + per] for g in gathered]
            off += per
        ok_col = torch.allclose(torch.cat(pieces, dim=-1), full, rtol=1e-9, atol=1e-9)

        # row parallel: K sharded in multiples of 128, rotation params narrowed by rank, all-reduce(SUM)
        one = dict(layer)
        one["sizes"] = [sum(sizes)]
        one["theta"], one["pairs"], one["channel_scales"] = layer["theta"][:1], layer["pairs"][:1], layer["channel_scales"][:1]
        full_row = _apply_oracle(one, x)
        row = tp.shard_row_parallel(one, rank, world)
        y = tp.row_parallel_forward(lambda xs: _apply_oracle(row, xs), x, rank, world)
        ok_row = torch.allclose(y, full_row, rtol=1e-9, atol=1e-9)

        # the plug-in's loader slices by the process rank exactly like plugin.py:47-50
        tgt = torch.zeros(8, K // world, dtype=torch.int16)
        sl = _maybe_shard_input(tgt, layer["pairs"][0])
        ok_loader = torch.equal(sl, layer["pairs"][0][:, rank * (K // world):(rank + 1) * (K // world)])
        # the collective a TP decode step asks for: without a GPU the one-shot buffers cannot be set up -- on EVERY rank
        # alike (no rank is left waiting in a collective the others skipped) -- and the backend's all-reduce takes over,
        # with the residual added after the sum
        fn, name = tp.make_allreduce(torch.device("cuda", 0), 256)
        part = torch.full((256,), float(rank + 1))
        out = fn(part.clone(), residual=torch.ones(256))
        ok_fallback = name == "gloo" and torch.equal(out, torch.full((256,), float(world * (world + 1) // 2 + 1)))
        q.put((rank, bool(ok_col), bool(ok_row), bool(ok_loader and ok_fallback)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_tp_sharding(world):
    """World 2 and world 4 (BASELINE config 5 is TP = 4): K = 512 shards into 128-channel slices, every merged
    partition of [128, 64, 64] columns into 16-column multiples."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(r, True, True, True) for r in range(world)]


def _bench_line(cmd, env=None):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None); e.pop("RANK", None); e.pop("LOCAL_RANK", None)
    e.update(env or {})
    out = subprocess.run([sys.executable] + cmd, cwd=root, env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout      # rank 0 prints exactly ONE JSON line
    return json.loads(lines[0])


def test_bench_spawns_its_ranks():
    """`python bench.py --gpus N` (the driver's command shape without torchrun) must start N ranks itself and
    report n_gpus = N; the default workload at N > 1 is the tensor-parallel one (strong scaling), a single-GPU
    workload named explicitly runs N replicas (weak scaling).  --dry-run swaps the GPU step for a CPU matmul and
    nccl for gloo; everything else (spawn, rendezvous, barrier, max-over-ranks clock, JSON) is the real path."""
    r = _bench_line(["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"])
    assert r["n_gpus"] == 2 and r["scaling"] == "strong" and r["config"]["parallelism"] == "tp2"
    assert r["config"]["workload"] == "llama3-70b-tp" and r["steps"] == 3 and r["warmup"] == 1
    r = _bench_line(["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run", "--workload", "qwen3-4b"])
    assert r["n_gpus"] == 2 and r["scaling"] == "weak" and r["config"]["parallelism"] == "dp2"
    r = _bench_line(["bench.py", "--steps", "2", "--warmup", "1", "--dry-run"])
    assert r["n_gpus"] == 1 and r["config"]["workload"] == "qwen3-4b"


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: the last timed step's output as DIR/<name>.npy in float32, the same in two runs with the same arguments
    (seeded inputs); --steps sets the number of timed steps and ms_per_step is reported."""
    import numpy as np
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        r = _bench_line(["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "0", "--dry-run", "--dump-outputs", str(d)])
        assert r["steps"] == 3 and r["ms_per_step"] > 0
    ya, yb = np.load(a / "step_output.npy"), np.load(b / "step_output.npy")
    assert ya.dtype == np.float32 and ya.shape == (1, 256) and np.array_equal(ya, yb)


def test_bench_dump_outputs_budget(tmp_path):
    """Past the 64 MB budget an output is replaced by a fixed seeded sample of its elements, the same in every run; float64 stays
    float64, everything else is written as float32; --steps below 1 is refused."""
    import subprocess
    import sys
    import numpy as np
    import bench
    big = np.arange(1 << 16, dtype=np.int32).reshape(256, 256)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"f64": np.ones(3), "big": big}, limit=4096 * 2 + 24 + 1000)
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and s.shape == (250,) and np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))
    assert np.all(np.diff(s) > 0) and np.all(np.isin(s, big.astype(np.float32)))
    assert np.load(tmp_path / "a" / "f64.npy").dtype == np.float64
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = subprocess.run([sys.executable, "bench.py", "--steps", "0", "--dry-run"], cwd=root, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--steps" in bad.stderr


def test_bench_under_torchrun():
    """The driver's launch line for N > 1: torch.distributed.run, one rank per process, rendezvous on 127.0.0.1."""
    port = _free_port()
    r = _bench_line(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                     "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"])
    assert r["n_gpus"] == 2 and r["scaling"] == "strong"
