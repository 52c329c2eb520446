"""Encrypted matrix x clear matrix on one MI355X at the reference test's own shape (ml/extensions/tests/
test_matmul.py:64-72): (4 x 2048) . (2048 x 2048) at the ML2048 presets, values and weights 0 .. 255, bits_reserved =
bit width of max |X.W| + 1.

After --warmup rounds, --reps rounds of expand -> dot -> packing keyswitch on torch's current stream, each stage between
a pair of HIP events, then the download of the packed GLWEs and their compression on the host by wall clock; the
median of each stage is reported, with the dot kernels' u64 multiply-add rate (R x Kb N x N x C multiply-adds of the
mask GEMM over the dot stage's time, which also holds the small body kernel).  One MatMul.multiply call is timed end
to end as well, and its result must decrypt to X.W under the reference's criterion (12 most significant bits, at most
1 % of the entries off) or nothing is reported.
Writes one JSON document (source_id, hostname) to --out and prints it.
  python tools/matmul_bench.py [--reps 5] [--warmup 1] [--out profiles/matmul_bench.json]"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_amd  # noqa: E402
from tfhe_amd import compression as C  # noqa: E402
from tfhe_amd import matmul as MM  # noqa: E402

SEED = 0x7F4E0001
R, K, COLS = 4, 2048, 2048


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "matmul_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    X = rng.integers(0, 256, size=(R, K), dtype=np.int64)
    W = rng.integers(0, 256, size=(K, COLS), dtype=np.int64)
    expected = X @ W
    width = int(np.ceil(np.log2(np.abs(expected).max() + 1)))
    mp = MM.MatmulParams.preset()
    mp.bits_reserved = width + 1
    pp = C.PksParams.preset(C.PKS_PRESET_ML2048)
    t = time.perf_counter()
    pkey = MM.PrivateKey(mp, pp, SEED)
    keygen_s = time.perf_counter() - t
    t = time.perf_counter()
    enc = MM.encrypt_matrix(pkey, X, seed=SEED + 1)
    encrypt_s = time.perf_counter() - t
    N, Kb, lpg = mp.N, enc.blocks, pp.lwe_per_glwe
    groups = -(-COLS // lpg)
    col_stride = groups * lpg
    dev = torch.device("cuda", 0)
    packer = C.Packer(pp, 0).load_key(pkey.compression_key)
    stage_ms = {"expand": [], "dot": [], "pack": [], "download_compress": []}
    try:
        with MM.MatMul(mp, packer, 0) as mm:
            clear = mm.clear_matrix(W)
            d_seeds = torch.from_numpy(enc.seeds.view(np.int64)).to(dev)
            d_packed = torch.from_numpy(enc.packed.view(np.int64)).to(dev)
            d_glwes = torch.empty((R * Kb, 2, N), dtype=torch.int64, device=dev)
            d_lwes = torch.zeros((R, col_stride, N + 1), dtype=torch.int64, device=dev)
            d_out = torch.empty((R * groups, pp.glwe_len), dtype=torch.int64, device=dev)
            for rep in range(a.warmup + a.reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record()
                mm.expand_async(d_seeds, d_packed, R * Kb, d_glwes)
                ev[1].record()
                mm.dot_async(clear, d_glwes, R, col_stride, d_lwes)
                ev[2].record()
                packer.pack_async(d_lwes, R * col_stride, d_out)
                ev[3].record()
                ev[3].synchronize()
                t = time.perf_counter()
                out = d_out.cpu().numpy().view(np.uint64).reshape(R, groups, pp.glwe_len)
                staged = [[C.compress_glwe(pp, out[r, g], min(lpg, COLS - g * lpg)) for g in range(groups)]
                          for r in range(R)]
                host_ms = (time.perf_counter() - t) * 1e3
                if rep >= a.warmup:
                    for i, name in enumerate(("expand", "dot", "pack")):
                        stage_ms[name].append(ev[i].elapsed_time(ev[i + 1]))
                    stage_ms["download_compress"].append(host_ms)
            whole_ms = []
            for rep in range(a.warmup + a.reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                result = mm.multiply(enc, clear)
                if rep >= a.warmup:
                    whole_ms.append((time.perf_counter() - t) * 1e3)
    finally:
        packer.close()
    for r in range(R):
        for g in range(groups):
            if not np.array_equal(staged[r][g].packed, result[r][g].packed):
                raise RuntimeError("the staged run and multiply() differ")
    got = MM.decrypt_matrix(result, pkey, COLS)
    shift = 12 if width <= 12 else width - 12
    bad = int(np.count_nonzero((got >> shift) != (expected >> shift)))
    if bad > got.size // 100:
        raise RuntimeError(f"{bad} of {got.size} entries differ from X.W on the 12 most significant bits")
    macs = R * Kb * N * N * COLS
    dot_med = statistics.median(stage_ms["dot"])
    doc = {"what": "encrypted (4 x 2048) . clear (2048 x 2048) at the ML2048 presets: expand -> dot -> packing "
                   "keyswitch on the device, download + host compression",
           "source_id": tfhe_amd.source_id(), "hostname": socket.gethostname(), "reps": a.reps, "warmup": a.warmup,
           "shape": {"R": R, "K": K, "C": COLS, "N": N, "bits_reserved": mp.bits_reserved, "bit_width": width},
           "stages": {k: stats(v) for k, v in stage_ms.items()},
           "multiply_wall": stats(whole_ms),
           "dot_u64_macs": macs, "dot_tmac_per_s": round(macs / (dot_med * 1e-3) / 1e12, 3),
           "msb_mismatches": bad, "max_abs_error": int(np.abs(got - expected).max()),
           "input_bytes": int(enc.nbytes), "output_bytes": int(sum(cg.nbytes for row in result for cg in row)),
           "keygen_s": round(keygen_s, 2), "encrypt_s": round(encrypt_s, 3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
