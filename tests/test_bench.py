"""bench.py's command line: a plain run is lean, --full adds the side measurements, --dump-outputs
writes what the last timed call computed, reproducibly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what only --full measures (each a run of its own)
FULL_ONLY = ("siblings", "reference_config", "quantize_int8", "uniform_inputs", "torch_ext", "solve_calls",
             "cpu_baseline", "clock_probe", "device", "isa", "allgather")


def _bench(*args, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_dry_run_reproducible(tmp_path):
    """--dump-outputs on the CPU plumbing path: one float32 O.npy of the step's [B, N, H*d] output, the
    same from run to run; --steps sets the number of timed steps the line reports."""
    outs = []
    for i in (1, 2):
        j = _bench("--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / f"d{i}"))
        assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] >= 0
        assert not [k for k in FULL_ONLY if k in j]
        assert sorted(os.listdir(tmp_path / f"d{i}")) == ["O.npy"]
        outs.append(np.load(tmp_path / f"d{i}" / "O.npy"))
    c = j["config"]
    assert outs[0].dtype == np.float32 and outs[0].shape == (c["B_per_gpu"], c["N"], c["d_model"])
    assert np.isfinite(outs[0]).all() and outs[0].std() > 0.1  # the dry-run step copies Q ~ N(0, 0.5^2)
    assert np.array_equal(outs[0], outs[1])


def test_dump_outputs_samples_large_output(tmp_path):
    """An output above the 64 MB bound is written as a fixed sample of whole rows: sorted distinct rows
    drawn by the documented seed, the same on every call, within the bound for all ranks together."""
    import bench
    rows, width = 20000, 1024  # 78 MiB of fp32
    O = (torch.arange(rows, dtype=torch.float32)[:, None] + torch.arange(width, dtype=torch.float32)[None, :] / 2048
         ).reshape(4, rows // 4, width)
    assert O.numel() * 4 > bench.DUMP_MAX_BYTES
    bench.dump_outputs(str(tmp_path / "a"), O, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), O, 0, 1)
    a, b = np.load(tmp_path / "a" / "O.npy"), np.load(tmp_path / "b" / "O.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE_BYTES // (4 * width), width)
    assert a.nbytes <= bench.DUMP_MAX_BYTES and np.array_equal(a, b)
    picked = a[:, 0].astype(np.int64)  # column 0 holds the row number
    want = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(rows, size=a.shape[0], replace=False))
    assert np.array_equal(picked, want) and np.all(np.diff(picked) > 0)
    assert np.array_equal(a, O.reshape(rows, width).numpy()[picked])
    # several ranks: one file each, the bound shared between them
    bench.dump_outputs(str(tmp_path / "w"), O, 1, 4)
    w = np.load(tmp_path / "w" / "O_rank1.npy")
    assert w.nbytes * 4 <= bench.DUMP_MAX_BYTES and os.listdir(tmp_path / "w") == ["O_rank1.npy"]
    # a small output is written whole, in its own shape
    bench.dump_outputs(str(tmp_path / "s"), O[:, :8], 0, 1)
    assert np.array_equal(np.load(tmp_path / "s" / "O.npy"), O[:, :8].numpy())


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_kernel_output(tmp_path):
    """A plain `--gpus 1 --steps K --warmup W` run on the GPU: the headline fields and the roofline of the
    timed calls, none of the --full measurements, and O.npy equal bit for bit to what the same kernel
    returns through torch_ext.flash_solve for the bench's own inputs (seed 1234, N(0, 0.5^2))."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    B, H, N, d = 2, 4, 512, 64
    j = _bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--B", str(B), "--H", str(H), "--N", str(N),
               "--dump-outputs", str(tmp_path / "d"))
    assert not [k for k in FULL_ONLY if k in j]
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "TFLOPS"
    assert j["higher_is_better"] is True and j["dtype"] == "int8"
    assert j["roofline"]["main_kernel_ms"] > 0
    got = np.load(tmp_path / "d" / "O.npy")
    assert got.dtype == np.float32 and got.shape == (B, N, H * d)
    from quantizedmha_amd import torch_ext
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1234)
    Q, K, V = (torch.randn(B, N, H * d, device=dev, generator=g) * 0.5 for _ in range(3))
    ref = torch_ext.flash_solve(Q, K, V, H * d, H, kernel="fa_tc_int8_b").cpu().numpy()
    assert np.array_equal(got, ref)
