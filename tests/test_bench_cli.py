"""bench.py's command line: a plain run is the headline alone, `--full` is behind its option,
and `--dump-outputs DIR` writes what the last timed step computed as .npy files.

* CPU: dump_outputs on stub batches (file names, dtypes, the seeded sample, the size cap, the
  same files for the same inputs), and `--full` accepted next to `--dry-run`.
* GPU: one plain run of two steps with `--dump-outputs`: the result line holds the headline
  fields and none of the lines that take runs of their own; every tile answered OK; the
  sampled bodies are PNG files that decode to the oracle's pixels of their grid tile and
  carry the length and CRC-32 the dump states for them.
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FILES = ("status", "nbytes", "crc32", "sample_index", "sample_body")


def _env():
    return {k: v for k, v in os.environ.items()
            if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}


def _load(d):
    assert sorted(os.listdir(d)) == sorted(f + ".npy" for f in FILES)
    arrs = {f: np.load(os.path.join(d, f + ".npy")) for f in FILES}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(os.path.getsize(os.path.join(d, f + ".npy")) for f in FILES) <= 64 << 20
    return arrs


class _StubBatch:
    def __init__(self, res):
        self.res = res

    def fetch(self):
        return self.res


def test_dump_outputs_files(tmp_path):
    import bench
    rng = np.random.RandomState(1)
    bodies = [rng.bytes(int(n)) for n in rng.randint(1, 3000, 100)]
    res = [(0, b) for b in bodies]
    res[7] = (404, None)
    bodies[7] = b""
    halves = [_StubBatch(res[:60]), _StubBatch(res[60:])]  # a step of two sub-batches
    bench.dump_outputs(str(tmp_path / "a"), halves)
    bench.dump_outputs(str(tmp_path / "b"), halves)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[f], b[f]) for f in FILES)
    assert a["status"].tolist() == [s for s, _ in res]
    assert a["nbytes"].tolist() == [len(x) for x in bodies]
    assert a["crc32"].tolist() == [zlib.crc32(x) for x in bodies]
    idx = a["sample_index"].astype(int)
    assert len(idx) == bench.DUMP_TILES and len(set(idx)) == len(idx) and idx.max() < 100
    for row, i in zip(a["sample_body"], idx):
        assert row[:len(bodies[i])].astype(np.uint8).tobytes() == bodies[i]
        assert not row[len(bodies[i]):].any()


def test_dump_outputs_stays_under_the_size_cap(tmp_path, monkeypatch):
    """Bodies too long for DUMP_TILES of them: fewer are stored, never more than the cap."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BODY_BYTES", 40000)
    bench.dump_outputs(str(tmp_path), [_StubBatch([(0, bytes(2500))] * 50)])
    a = _load(tmp_path)
    assert a["sample_body"].shape == (4, 2500) and a["sample_body"].nbytes <= 40000
    assert len(a["nbytes"]) == 50


def test_full_is_an_option():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dry-run", "--full", "--steps", "2",
                          "--warmup", "0"], env=_env(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout.splitlines()[-1])["steps"] == 2


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_its_outputs(tmp_path, oracle):
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], env=_env(), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "tiles/s" and rec["higher_is_better"] is True and rec["dtype"] == "u8"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 4096 / (rec["ms_per_step"] * 1e-3)) <= 1e-3 * rec["value"]
    for moved in ("roofline", "kernels", "kernel_streams", "cpu_baseline", "e2e_with_d2h",
                  "raw_4096x512x512_u16", "c5_mixed_16384_requests"):
        assert moved not in rec
    a = _load(tmp_path)
    assert len(a["status"]) == 4096 and not a["status"].any()
    assert a["nbytes"].sum() / 4096 == pytest.approx(rec["compressed_bytes_per_tile"], abs=0.1)
    idx = a["sample_index"].astype(int)
    assert len(idx) >= 16
    for row, i in zip(a["sample_body"], idx):
        body = row[:int(a["nbytes"][i])].astype(np.uint8).tobytes()
        assert zlib.crc32(body) == a["crc32"][i] and not row[len(body):].any()
        r, px, _ = oracle.png_decode(body)
        want = oracle.gen_region(oracle.GEN_NOISE, oracle.UINT16, (i % 64) * 512, (i // 64) * 512, 512, 512)
        assert r == 0 and px == want.tobytes(), i
