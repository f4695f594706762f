"""A plain bench.py run on the GPU: the K timed steps and nothing else, the
result line's fixed fields, and --dump-outputs' file against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_crcs(cuda, tmp_path):
    """configs[0] (1,000 x 4 KiB of synthetic stream 0xB1A2E5), 3 timed steps:
    DIR/crc32c.npy holds every message's CRC as the oracle computes it (so it
    is the same from run to run), the line says steps 3 and carries
    ms_per_step, and nothing that belongs to --full was run."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--config", "1k_x_4KiB",
                        "--settle-seconds", "0", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["value"] == pytest.approx(1000 * 4096 / 2**30 / (d["ms_per_step"] / 1e3), rel=1e-2)
    assert d["full"] is False
    for key in ("parity", "cpu_baseline", "planned_ms_per_step", "strong_scaling"):
        assert key not in d
    assert "kernel_avg_us" not in d["roofline"]
    n, size, seed = 1000, 4096, 0xB1A2E5
    host = oracle.fill_payload(0, n * size, seed)
    exp = oracle.batch(host, np.arange(n, dtype=np.uint64) * size, np.full(n, size, np.uint32))
    assert os.listdir(tmp_path) == ["crc32c.npy"]
    got = np.load(tmp_path / "crc32c.npy")
    assert got.dtype == np.float64 and got.shape == (n,)
    assert np.array_equal(got.astype(np.uint32), exp)
