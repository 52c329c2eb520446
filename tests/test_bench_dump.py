"""bench.py --dump-outputs, the writer alone (no GPU): exact float64 halves of the u64 words, and a fixed,
ascending row sample once the output exceeds the budget."""
import numpy as np


def _rebuilt(d):
    hi, lo, rows = (np.load(d / f"pbs_out_{n}.npy") for n in ("hi32", "lo32", "rows"))
    assert hi.dtype == lo.dtype == rows.dtype == np.float64 and hi.shape == lo.shape and len(rows) == len(hi)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64), rows, hi.nbytes + lo.nbytes + rows.nbytes


def test_dump_outputs_small_output_is_written_whole(tmp_path):
    import bench
    out = np.arange(7 * 631, dtype=np.uint64).reshape(7, 631) * np.uint64(0x9E3779B97F4A7C15)
    out[0, 0], out[0, 1] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)
    bench.dump_outputs(str(tmp_path), out)
    got, rows, _ = _rebuilt(tmp_path)
    assert np.array_equal(rows, np.arange(7)) and np.array_equal(got, out)


def test_dump_outputs_samples_within_budget(tmp_path):
    import bench
    n = bench.DUMP_BUDGET // (16 * 2049) + 100                       # 100 rows past the budget at P-FHEVM's width
    out = np.arange(n * 2049, dtype=np.uint64).reshape(n, 2049) * np.uint64(0x9E3779B97F4A7C15)
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out)
    got, rows, nbytes = _rebuilt(tmp_path / "a")
    assert nbytes <= 64 * 10 ** 6 and len(rows) == n - 100
    assert np.all(np.diff(rows) > 0) and np.array_equal(rows, np.load(tmp_path / "b" / "pbs_out_rows.npy"))
    assert np.array_equal(got, out[rows.astype(np.int64)])
