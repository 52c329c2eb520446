#!/usr/bin/env python3
"""Key-load time from a CompressedServerKey container: host decompression against expansion on the device.

One process, one GPU, two key sets: classic PRESET_FHEVM_FFT with its 1449 modulus-switch zeros, and
PRESET_FHEVM_MB_FFT at grouping factor 3.  After WARMUP loads of each route the two routes alternate for ROUNDS
rounds on one engine:

  host route    loads_compressed_server_key -> decompress_server_key -> Engine.load_keys / load_ms_key
  device route  loads_compressed_server_key -> Engine.load_compressed_keys

Each load ends in a device synchronise and is followed by one fixed PBS batch (not timed); the two routes' outputs
must be equal.  Reported: median, minimum, maximum and interquartile range of both routes, the bytes each uploads,
and the device route split by device events into upload, expansion kernels and conversion (shard 0,
tfhe_hip_seeded_load_stats).  Writes profiles/seeded_load_bench.json.

    python tools/seeded_load_bench.py [--rounds 10] [--warmup 3] [--out profiles/seeded_load_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tfhe_amd  # noqa: E402
from tfhe_amd import keyio  # noqa: E402

MM = 16
DELTA = (1 << 63) // MM


def stats(ms):
    a = np.sort(np.asarray(ms, dtype=float))
    q1, q3 = np.percentile(a, [25, 75])
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "iqr_ms": float(q3 - q1),
            "samples_ms": [round(float(x), 3) for x in ms]}


def host_route(eng, blob):
    csk = keyio.loads_compressed_server_key(blob)
    _, sk = keyio.decompress_server_key(csk)
    zeros, sk.ms_zeros = sk.ms_zeros, None
    eng.load_keys(sk)
    up = sk.bsk.nbytes + sk.ksk.nbytes
    if zeros is not None:
        eng.load_ms_key(zeros, **csk.ms)
        up += zeros.nbytes                       # the rows; their transpose is built on the device
    eng.sync()
    return up


def device_route(eng, blob):
    csk = keyio.loads_compressed_server_key(blob)
    eng.load_compressed_keys(csk)
    eng.sync()
    return csk.bsk_bodies.nbytes + csk.ksk_bodies.nbytes + (csk.ms_bodies.nbytes if csk.ms_bodies is not None else 0)


def run_set(name, preset, grouping, ms_count, rounds, warmup):
    p = tfhe_amd.Params.preset(preset)
    ck, _ = tfhe_amd.gen_keys(p, 0x5EEDBE7C, with_server_key=False)
    blob = keyio.dumps_compressed_server_key(keyio.compress_server_key(ck, seed=0x5EEDBE7D, ms_count=ms_count,
                                                                       grouping=grouping))
    msgs = np.arange(32, dtype=np.uint64) % MM
    cts = ck.encrypt(msgs, MM, seed=0xC0FFEE7C)
    lut = tfhe_amd.lut_from_table(p.N, MM, [(5 * m + 3) % MM for m in range(MM)], DELTA)[None]
    t = {"host": [], "device": []}
    split = {"upload_ms": [], "expand_ms": [], "convert_ms": []}
    up = {}
    with tfhe_amd.Engine(p, 0) as eng:
        routes = (("host", host_route), ("device", device_route))
        ref = None
        for r in range(warmup + rounds):
            for which, fn in routes:
                t0 = time.perf_counter()
                up[which] = fn(eng, blob)
                dt = (time.perf_counter() - t0) * 1e3
                out = eng.pbs(cts, lut)
                if ref is None:
                    ref = out
                    if not np.array_equal(ck.decrypt(out, MM), (5 * msgs + 3) % MM):
                        raise RuntimeError(f"{name}: the batch does not decrypt")
                elif not np.array_equal(out, ref):
                    raise RuntimeError(f"{name}: round {r}, {which} route: outputs differ from the first load's")
                if r >= warmup:
                    t[which].append(dt)
                    if which == "device":
                        for k, v in eng.seeded_load_stats().items():
                            split[k].append(v)
        kernel = eng.br_kernel(32)
    res = {"preset": int(preset), "n": int(p.n), "grouping": grouping, "ms_zeros": ms_count, "container_bytes": len(blob),
           "br_kernel": kernel, "host_route": {**stats(t["host"]), "uploaded_bytes": int(up["host"])},
           "device_route": {**stats(t["device"]), "uploaded_bytes": int(up["device"]),
                            "device_events_median_ms": {k: float(np.median(v)) for k, v in split.items()}}}
    res["host_over_device"] = res["host_route"]["median_ms"] / res["device_route"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_load_bench.json"))
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds must be at least 10")
    res = {"tool": "tools/seeded_load_bench.py", "source": tfhe_amd.source_id(), "rounds": a.rounds, "warmup": a.warmup,
           "sets": {
               "fhevm_classic": run_set("fhevm_classic", tfhe_amd.PRESET_FHEVM_FFT, 1, tfhe_amd.MS_FHEVM["count"],
                                        a.rounds, a.warmup),
               "fhevm_multibit_g3": run_set("fhevm_multibit_g3", tfhe_amd.PRESET_FHEVM_MB_FFT, 3, 0, a.rounds, a.warmup)}}
    try:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
    except Exception:  # noqa: BLE001 - the name is informative only
        pass
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for k, s in res["sets"].items():
        print(f"{k}: host {s['host_route']['median_ms']:.1f} ms (iqr {s['host_route']['iqr_ms']:.1f}), device "
              f"{s['device_route']['median_ms']:.1f} ms (iqr {s['device_route']['iqr_ms']:.1f}), "
              f"x{s['host_over_device']:.2f}; device events {s['device_route']['device_events_median_ms']}")


if __name__ == "__main__":
    main()
