"""bench.py keeps the driver's contract: one JSON line with the metric, the whole-job value and the
roofline object; with --full also the cpu_baseline object and a bit-exact oracle comparison of the
sampled outputs (run here at a reduced batch so it takes seconds; the round-end bench runs the full 4096).
A plain run times its steps only, and --dump-outputs writes the last timed step's ciphertexts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("preset", ["gate_fft", "fhevm_fft"])
def test_bench_json_contract(preset):
    r = subprocess.run([sys.executable, "bench.py", "--preset", preset, "--steps", "2", "--warmup", "1",
                        "--batch", "512", "--full", "--cpu-sample", "32"], cwd=ROOT, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert d["dtype"] == "f64" and d["config"]["batch_per_gpu"] == 512
    rf = d["roofline"]
    # VALU-issue bound; at B = 512 no same-build counter profile exists, so the f64 FLOP figure is reported
    assert rf["bound"] == "valu" and rf["kernel_ms"] > 0
    assert rf["unit"] == "TFLOP/s" and rf["peak"] == 78.6 and rf["traffic"] is None
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0 < rf["frac"] <= 1
    assert rf["hbm_model_r1"]["bytes_per_launch"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
    assert d["decrypt_ok"] is True and d["sample_bitexact"] is True
    bx = d["bitexact_check"]
    assert bx["bitexact_pbs"] == 32 and bx["gpu_sha256"] == bx["oracle_sha256"]


def test_bench_strong_scaling_mode():
    """--global-batch: one global batch, this rank's contiguous slice, scaling "strong"."""
    r = subprocess.run([sys.executable, "bench.py", "--steps", "1", "--warmup", "1", "--global-batch", "1024",
                        "--no-cpu"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.strip().startswith("{")][0])
    assert d["scaling"] == "strong" and d["config"]["global_batch"] == 1024 and d["config"]["batch_per_gpu"] == 1024
    assert d["decrypt_ok"] is True


def test_bench_c3_config():
    """--config c3 (BASELINE.json configs[2]): FheUint8 values x 8 per-bit LUTs in one multi-LUT launch; every byte
    decrypted, the CPU sample (whole FheUint8 values, lut_index included) bit-exact against the oracle."""
    r = subprocess.run([sys.executable, "bench.py", "--config", "c3", "--steps", "2", "--warmup", "1", "--batch", "128",
                        "--full", "--cpu-sample", "64"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.strip().startswith("{")][0])
    assert d["unit"] == "FheUint8/s" and d["config"]["batch_per_gpu"] == 128 and d["config"]["pbs_per_gpu"] == 1024
    assert abs(d["pbs_per_s"] - 8 * d["value"]) < 1e-6 * d["pbs_per_s"] + 1
    assert d["decrypt_ok"] is True and d["sample_bitexact"] is True
    assert d["roofline"]["launches"] == 2 and d["roofline"]["kernel_ms"] > 0
    bx = d["bitexact_check"]
    assert bx["bitexact_pbs"] == 64 and bx["gpu_sha256"] == bx["oracle_sha256"]


def test_bench_plain_run_dumps_outputs(tmp_path, gate_fft_keys):
    """A plain run (no --full) carries no CPU leg; --steps sets the timed launches; --dump-outputs writes the last
    step's output ciphertexts as exact float64 halves, identical from run to run (fixed seeds): rebuilt to u64 they
    decrypt, under the bench's key set, to the bench's input bits."""
    import bench
    from tfhe_amd.dist import rank_batch_seed
    B = 96
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert "cpu_baseline" not in d and "sample_bitexact" not in d
    assert d["metric"] == bench.METRIC and d["unit"] == "PBS/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 3 and d["roofline"]["launches"] == 3 and d["ms_per_step"] > 0 and d["decrypt_ok"] is True
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]   # ms_per_step is rounded to 1 us
    assert sorted(os.listdir(tmp_path)) == ["pbs_out_hi32.npy", "pbs_out_lo32.npy", "pbs_out_rows.npy"]
    hi, lo, rows = (np.load(tmp_path / f"pbs_out_{n}.npy") for n in ("hi32", "lo32", "rows"))
    assert hi.dtype == lo.dtype == rows.dtype == np.float64 and hi.shape == lo.shape == (B, 631)
    assert np.array_equal(rows, np.arange(B))
    assert hi.min() >= 0 and hi.max() < 2.0 ** 32 and lo.min() >= 0 and lo.max() < 2.0 ** 32
    out = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    ck, _ = gate_fft_keys
    bits = np.random.default_rng(rank_batch_seed(bench.INPUT_SEED, 0)).integers(0, 2, B).astype(bool)
    assert np.array_equal(ck.decrypt_bool(out), bits)
    assert np.array_equal(out, _pbs_of_bench_inputs(ck, gate_fft_keys[1], bits))


def _pbs_of_bench_inputs(ck, sk, bits):
    """The bench's batch through the library in this process: same keys, same encryption streams."""
    import bench
    import tfhe_amd
    cts = ck.encrypt_bool(bits, seed=bench.INPUT_SEED + 1, stream0=0)
    with tfhe_amd.Engine(ck.params, 0) as eng:
        eng.load_keys(sk)
        return eng.pbs(cts, eng.gate_lut())

