"""Oblivious pseudo-random ciphertexts (fhEVM rand) on one MI355X: Engine.oprf against the route that existed before
it, same box, same process.

--rows rows (default 4096) at P-FHEVM-FFT (staircase LUT of 2 random bits in the radix block, rotation only) and at
P-GATE-FFT (gate LUT, rotation + keyswitch), keys from a fixed seed.  After warm-up, --reps rounds alternate
  (a) host route: tfhe_hip_csprng_words per row on the host (software AES), the (mask, 0) rows through
      Engine.bootstrap (P-FHEVM) / Engine.pbs (P-GATE) from host buffers, the post-add on the host;
  (b) Engine.oprf: 16 bytes per row up, the masks from csprng.hip on the device, rotation, post-add kernel.
Both are wall clock around calls that end in a stream synchronise.  The two routes must give the same words, or
nothing is reported.  Leg (b) also records the engine's event timing: slot 3 (mask kernel), 0 (rotation + sample
extraction), 1 (keyswitch).  The bar: (b) is not slower than (a) beyond the spread of (a).
Writes one JSON document (source_id, hostname) to --out and prints it.
  python tools/oprf_bench.py [--rows 4096] [--reps 7] [--out profiles/oprf_bench.json]"""
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

SEED = 0x7F4E0001
PARENT = (0x0F2F0002, 0)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs_ms": [round(x, 3) for x in ms]}


def host_route(eng, seeds, lut, post):
    p = eng.params
    L = tfhe_amd.lib()
    cts = np.zeros((seeds.shape[0], p.n + 1), dtype=np.uint64)
    t0 = time.perf_counter()
    for r in range(seeds.shape[0]):
        tfhe_amd._check(L.tfhe_hip_csprng_words(tfhe_amd._u64(seeds[r]), 0, p.n, tfhe_amd._u64(cts[r])))
    t1 = time.perf_counter()
    out = eng.bootstrap(cts, lut) if p.order == 1 else eng.pbs(cts, lut)
    with np.errstate(over="ignore"):
        out[:, -1] += np.uint64(post)
    return out, (t1 - t0) * 1e3


def one_preset(preset, name, rows, reps, warmup):
    params = tfhe_amd.Params.preset(preset)
    ck, sk = tfhe_amd.gen_keys(params, SEED)
    seeds = tfhe_amd.oprf_block_seeds(PARENT, rows)
    lut, post = tfhe_amd.lut_oprf(params.N, 2, 5) if params.order == 1 else (tfhe_amd.lut_constant(params.N, tfhe_amd.MU), 0)
    a_ms, a_masks_ms, b_ms = [], [], []
    with tfhe_amd.Engine(params, 0) as eng:
        eng.load_keys(sk)
        eng.timing_reset()
        for r in range(warmup + reps):
            t = time.perf_counter()
            ref, masks_ms = host_route(eng, seeds, lut, post)
            ta = (time.perf_counter() - t) * 1e3
            eng.timing(r >= warmup)
            t = time.perf_counter()
            out = eng.oprf(seeds, lut, [post])
            tb = (time.perf_counter() - t) * 1e3
            eng.timing(False)
            if not np.array_equal(out, ref):
                raise RuntimeError(f"{name}: Engine.oprf and the host route differ")
            if r >= warmup:
                a_ms.append(ta)
                a_masks_ms.append(masks_ms)
                b_ms.append(tb)
        slots = {}
        for slot, what in ((3, "mask_kernel_ms"), (0, "rotation_ms"), (1, "keyswitch_ms")):
            ms, n = eng.timing_stats(slot)
            slots[what] = round(ms / n, 4) if n else None
        kernel = eng.br_kernel(rows)
    res = {"rows": rows, "host_route": stats(a_ms), "host_route_masks_on_host": stats(a_masks_ms), "oprf": stats(b_ms),
           **slots, "rotation_kernel": kernel}
    res["speedup_over_host_route"] = round(res["host_route"]["median_ms"] / res["oprf"]["median_ms"], 2)
    res["host_route_spread_ms"] = round(max(a_ms) - min(a_ms), 3)
    res["oprf_not_slower_beyond_spread"] = bool(
        res["oprf"]["median_ms"] <= res["host_route"]["median_ms"] + res["host_route_spread_ms"])
    res["mask_kernel_share_of_rotation"] = round(slots["mask_kernel_ms"] / slots["rotation_ms"], 5)
    res["upload_bytes"] = {"host_route": int(rows * (params.n + 1) * 8), "oprf": int(rows * 16)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "oprf_bench.json"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps: at least five repetitions")
    doc = {"what": "Engine.oprf (masks generated on the device from 16-byte seeds) vs masks from the host CSPRNG + "
                   "Engine.bootstrap / Engine.pbs through host buffers + host post-add",
           "source_id": tfhe_amd.source_id(), "hostname": socket.gethostname(), "reps": a.reps, "warmup": a.warmup}
    for preset, name in ((tfhe_amd.PRESET_FHEVM_FFT, "P-FHEVM-FFT"), (tfhe_amd.PRESET_GATE_FFT, "P-GATE-FFT")):
        doc[name] = one_preset(preset, name, a.rows, a.reps, a.warmup)
        print(f"{name}: done", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
