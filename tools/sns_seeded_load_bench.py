#!/usr/bin/env python3
"""Load time of the two 128-bit keys of the sns-worker path from a CompressedServerKey container: host decompression
against expansion on the device, with today's standard-domain load beside them.

One process, one GPU, the two presets: the noise-squashing key (n = 918, k = 2, N = 2048, 2^24 x 3) and the ct128
packing key (in_dim 4096, level 1, k = 6, N = 1024).  Each key is measured from a container of its own: the squashing
set carries the squashing key alone; the packing key travels inside a squashing key, so its set carries one at n = 1
(295 KB) beside it.  After WARMUP loads of every route the three routes alternate for ROUNDS rounds on one context:

  (a) standard   the standard-domain key words, already in host memory -> load_key (the loader as it was)
  (b) host       container bytes -> loads_compressed_server_key -> decompress() on the host -> load_key
  (c) device     container bytes -> loads_compressed_server_key -> load_compressed_key

Each load ends in a device synchronise and is followed by one fixed squash or pack (not timed), whose output must be
equal between the routes.  Reported: median, minimum, maximum and interquartile range of every route, the bytes each
uploads, route (c) split by device events into upload, expansion and conversion / correction, and the acceptance
criterion: the median of (c) lies below the median of (b) by more than the IQR of (b).
Writes profiles/sns_seeded_load_bench.json.

    python tools/sns_seeded_load_bench.py [--rounds 10] [--warmup 3] [--out profiles/sns_seeded_load_bench.json]
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
from tfhe_amd import sns as S  # noqa: E402
from tfhe_amd import sns_compression as SC  # noqa: E402

RNG_SEED, SEED = 0x5EEDBE80, 0x5EEDBE81


def stats(ms):
    a = np.sort(np.asarray(ms, dtype=float))
    q1, q3 = np.percentile(a, [25, 75])
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "iqr_ms": float(q3 - q1),
            "samples_ms": [round(float(x), 3) for x in ms]}


def client_key(n):
    p = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_FFT)
    p.n = n
    return tfhe_amd.gen_keys(p, RNG_SEED, with_server_key=False)[0]


def alternate(name, routes, check, rounds, warmup):
    """routes: [(label, fn() -> uploaded bytes)]; check() -> the fixed call's output.  Returns label -> result."""
    t = {k: [] for k, _ in routes}
    split = {}
    up = {}
    ref = None
    for r in range(warmup + rounds):
        for which, fn in routes:
            t0 = time.perf_counter()
            got = fn()
            dt = (time.perf_counter() - t0) * 1e3
            up[which], ev = got if isinstance(got, tuple) else (got, None)
            out = check()
            if ref is None:
                ref = out
            elif not np.array_equal(out, ref):
                raise RuntimeError(f"{name}: round {r}, route {which}: outputs differ from the first load's")
            if r >= warmup:
                t[which].append(dt)
                if ev:
                    for k, v in ev.items():
                        split.setdefault(k, []).append(v)
    res = {k: {**stats(v), "uploaded_bytes": int(up[k])} for k, v in t.items()}
    res["device"]["device_events_median_ms"] = {k: float(np.median(v)) for k, v in split.items()}
    b, c = res["host"], res["device"]
    res["host_over_device"] = b["median_ms"] / c["median_ms"]
    res["criterion"] = {"device_median_ms": c["median_ms"], "host_median_minus_iqr_ms": b["median_ms"] - b["iqr_ms"],
                        "holds": bool(c["median_ms"] < b["median_ms"] - b["iqr_ms"])}
    return res, ref


def run_squashing(rounds, warmup):
    ck = client_key(918)
    key = S.SquashedKey(S.SnsParams.preset(0), RNG_SEED, ck.lwe_key, with_bsk=False)
    blob = keyio.dumps_compressed_server_key(keyio.compress_server_key(ck, seed=SEED, squashing=key))
    std = keyio.loads_compressed_server_key(blob).squashing.decompress()      # route (a)'s words
    msgs = np.arange(8, dtype=np.uint64) % 16
    rng = np.random.default_rng(5)
    small = rng.integers(0, 2 ** 64, size=(8, 919), dtype=np.uint64)
    with np.errstate(over="ignore"):
        small[:, 918] = (small[:, :918] * ck.lwe_key).sum(axis=1, dtype=np.uint64) + (msgs << np.uint64(59))
    sq = S.Squasher(key.params, 0)
    try:
        def standard():
            sq.load_key(std)
            return std.bsk.nbytes

        def host():
            d = keyio.loads_compressed_server_key(blob).squashing.decompress()
            sq.load_key(d)
            return d.bsk.nbytes

        def device():
            c = keyio.loads_compressed_server_key(blob).squashing
            sq.load_compressed_key(c)
            return c.bodies.nbytes, sq.seeded_load_stats()

        res, out = alternate("squashing", (("standard", standard), ("host", host), ("device", device)),
                             lambda: sq.squash(small), rounds, warmup)
    finally:
        sq.close()
    if not np.array_equal(key.decrypt(out), msgs):
        raise RuntimeError("squashing: the fixed batch does not decrypt")
    return {"n": 918, "container_bytes": len(blob), **res}


def run_packing(rounds, warmup):
    ck = client_key(1)
    sq_key = S.SquashedKey(_squash_params(1), RNG_SEED, ck.lwe_key, with_bsk=False)
    pp = SC.SnsPksParams.preset(0)
    key = SC.SquashedCompressionKey(pp, RNG_SEED, sq_key.glwe_key, with_key=False)
    blob = keyio.dumps_compressed_server_key(
        keyio.compress_server_key(ck, seed=SEED, squashing=sq_key, squashed_compression=key))
    std = keyio.loads_compressed_server_key(blob).squashed_compression.decompress()
    msgs = np.arange(8, dtype=np.uint64) % 16
    rng = np.random.default_rng(6)
    lwes = rng.integers(0, 2 ** 64, size=(8, pp.in_dim + 1, 2), dtype=np.uint64)
    a = lwes[:, :pp.in_dim, 0].astype(object) | (lwes[:, :pp.in_dim, 1].astype(object) << 64)
    sel = key.in_key.astype(bool)
    for q, m in enumerate(msgs):
        b = (int(a[q][sel].sum()) + ((1 << 127) // 16) * int(m)) & ((1 << 128) - 1)
        lwes[q, pp.in_dim] = (b & ((1 << 64) - 1), b >> 64)
    packer = SC.SquashedPacker(pp, 0)
    try:
        def standard():
            packer.load_key(std)
            return std.pksk.nbytes

        def host():
            d = keyio.loads_compressed_server_key(blob).squashed_compression.decompress()
            packer.load_key(d)
            return d.pksk.nbytes

        def device():
            c = keyio.loads_compressed_server_key(blob).squashed_compression
            packer.load_compressed_key(c)
            return c.bodies.nbytes, packer.seeded_load_stats()

        res, out = alternate("packing", (("standard", standard), ("host", host), ("device", device)),
                             lambda: packer.pack(lwes), rounds, warmup)
    finally:
        packer.close()
    if not np.array_equal(SC.decrypt_list(key, SC._compress_groups(pp, out, 8)), msgs):
        raise RuntimeError("packing: the fixed batch does not decrypt")
    return {"in_dim": int(pp.in_dim), "out_k": int(pp.out_k), "out_N": int(pp.out_N), "level": int(pp.level),
            "container_bytes": len(blob), **res}


def _squash_params(n):
    sp = S.SnsParams.preset(0)
    sp.n = n
    return sp


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sns_seeded_load_bench.json"))
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds must be at least 10")
    res = {"tool": "tools/sns_seeded_load_bench.py", "source": tfhe_amd.source_id(), "rounds": a.rounds,
           "warmup": a.warmup, "sets": {"squashing_key": run_squashing(a.rounds, a.warmup),
                                        "ct128_packing_key": run_packing(a.rounds, a.warmup)}}
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
        print(f"{k}: standard {s['standard']['median_ms']:.1f} ms (iqr {s['standard']['iqr_ms']:.1f}), host "
              f"{s['host']['median_ms']:.1f} ms (iqr {s['host']['iqr_ms']:.1f}), device {s['device']['median_ms']:.1f} ms "
              f"(iqr {s['device']['iqr_ms']:.1f}), x{s['host_over_device']:.2f}; criterion holds: "
              f"{s['criterion']['holds']}; device events {s['device']['device_events_median_ms']}")


if __name__ == "__main__":
    main()
