"""Throughput of the 128-bit packing keyswitch on one MI355X at the fhEVM preset (in_dim 4096, 2^61 x 1, out k = 6,
N = 1024, 128 LWEs per GLWE; 470 MB key): valid squashed-LWE encryptions resident in HBM are packed in batches of
128, 1024 and 4096; every packed message must decrypt from the stored form; times are HIP events on torch's stream
after a warm-up, the median of several runs.  Writes one JSON file and prints it as one line.
  python tools/sns_pack_bench.py [--batches 128,1024,4096] [--steps K] [--runs R] [--out profiles/NAME.json]
      [--squash-json FILE]   (the line tools/sns_bench.py printed on the same machine: adds both rates' ratio)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_amd  # noqa: E402
from tfhe_amd import sns_compression as SC  # noqa: E402

# sns_pks_gemm_kernel as compiled for gfx950 (hipcc -Rpass-analysis=kernel-resource-usage), kept with the numbers
GEMM_RESOURCES = {"vgprs": 132, "scratch_bytes": 0, "lds_bytes": 24832, "waves_per_simd": 3}


def log(msg):  # progress on stderr, flushed: a run that stalls shows how far it got
    print(f"[sns_pack_bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def encrypt(pp, in_key, msgs, seed):
    """Noiseless encryptions over Z_2^128: mask uniform, b = <a, s> + m 2^127 / 16; (count, in_dim + 1, 2) u64."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2 ** 64, size=(len(msgs), pp.in_dim + 1, 2), dtype=np.uint64)
    sel = np.asarray(in_key, dtype=bool)
    lo, hi = x[:, :pp.in_dim, 0][:, sel], x[:, :pp.in_dim, 1][:, sel]
    lo_l = (lo & np.uint64(0xFFFFFFFF)).sum(1, dtype=np.uint64)       # exact: < 2^44
    lo_h = (lo >> np.uint64(32)).sum(1, dtype=np.uint64)
    hi_s = hi.sum(1, dtype=np.uint64)                                 # mod 2^64, as wanted
    delta = (1 << 127) // 16
    for q, m in enumerate(msgs):
        b = (int(lo_l[q]) + (int(lo_h[q]) << 32) + (int(hi_s[q]) << 64) + delta * int(m)) & ((1 << 128) - 1)
        x[q, pp.in_dim] = (b & ((1 << 64) - 1), b >> 64)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,1024,4096")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "sns_pack_bench.json"))
    ap.add_argument("--squash-json", default=None)
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("sns_pack_bench: no GPU (a rate is measured on the device or not at all)")
    pp = SC.SnsPksParams.preset()
    log(f"start: batches {batches}, steps {a.steps}, runs {a.runs}")
    in_key = np.random.default_rng(0x7F4E0001).integers(0, 2, pp.in_dim).astype(np.uint64)
    t = time.time()
    key = SC.SquashedCompressionKey(pp, 0x7F4E0001, in_key)
    keygen_s = time.time() - t
    log(f"packing key generated in {keygen_s:.1f}s ({key.pksk.nbytes / 1e6:.0f} MB)")
    packer = SC.SquashedPacker(pp, 0).load_key(key)
    log("packing key loaded")
    top = max(batches)
    msgs = (np.arange(top) * 5 + 1) % 16
    pool = encrypt(pp, in_key, msgs, 5)
    dev = torch.device("cuda:0")
    d_pool = torch.from_numpy(pool.view(np.int64)).to(dev)
    s = torch.cuda.current_stream(dev)
    log("inputs ready")
    macs = pp.in_dim * pp.level * (pp.out_k + 1) * pp.out_N            # u64 x u128 MACs per ciphertext
    results = []
    for B in batches:
        groups = -(-B // pp.lwe_per_glwe)
        d_out = torch.zeros((groups,) + pp.glwe_shape, dtype=torch.int64, device=dev)
        packer.pack_async(d_pool, B, d_out, s)                         # warm-up: workspaces, code objects
        torch.cuda.synchronize()
        times = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.steps):
                packer.pack_async(d_pool, B, d_out, s)
            e1.record(s)
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / a.steps)
        ms = statistics.median(times)
        glwes = d_out.cpu().numpy().view(np.uint64)
        comp = [SC.compress_glwe(pp, glwes[g], min(pp.lwe_per_glwe, B - g * pp.lwe_per_glwe)) for g in range(groups)]
        ok = bool(np.array_equal(SC.decrypt_list(key, comp, 16), msgs[:B]))
        log(f"batch {B}: {ms:.3f} ms median of {a.runs} (min {min(times):.3f}, max {max(times):.3f}), decrypt_ok {ok}")
        results.append({"batch": B, "ms_per_batch": round(ms, 3), "ms_min": round(min(times), 3),
                        "ms_max": round(max(times), 3), "ciphertexts_per_s": round(B / (ms * 1e-3), 1),
                        "gmacs_per_s": round(B * macs / (ms * 1e-3) / 1e9, 1), "decrypt_ok": ok,
                        "stored_bytes": sum(c.nbytes for c in comp), "squashed_bytes": B * (pp.in_dim + 1) * 16})
    best = max(results, key=lambda r: r["ciphertexts_per_s"])
    out = {"metric": "squashed ciphertexts packed/s (128-bit packing keyswitch, in 4096, 2^61x1, k=6 N=1024, 128/GLWE)",
           "value": best["ciphertexts_per_s"], "batch": best["batch"], "results": results,
           "macs_per_ciphertext": macs, "pksk_mb": round(key.pksk.nbytes / 1e6, 1), "keygen_s": round(keygen_s, 1),
           "steps": a.steps, "runs": a.runs, "timing": "HIP events, median of runs, after one warm-up call per batch",
           "gemm_kernel": GEMM_RESOURCES, "source_id": tfhe_amd.source_id(),
           "decrypt_ok": all(r["decrypt_ok"] for r in results)}
    if a.squash_json:
        with open(a.squash_json) as f:
            sq = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
        out["squashes_per_s"] = sq["value"]
        out["squash_batch"] = sq["batch"]
        out["pack_over_squash_rate"] = round(best["ciphertexts_per_s"] / sq["value"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    packer.close()
    if not out["decrypt_ok"]:
        raise SystemExit("sns_pack_bench: a packed message did not decrypt")


if __name__ == "__main__":
    main()
