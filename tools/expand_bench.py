"""Ingest of compact ciphertext lists on one MI355X: ctlist.cast_list_to_blocks_device against the route that existed
before it, same box, same run.

P-FHEVM on the FFT64 transform with casting keys (keyswitch key: compact-PKE key -> small key; MS noise reduction on).
For each --counts entry, a packed compact list of that many LWEs (two radix blocks each, rep = 2) is encrypted under
a fresh compact public key; then, after warm-up, --reps rounds of
  (a) device: cast_list_to_blocks_device on the resident list words (expansion kernel + casting PBS), timed by a pair
      of HIP events on the launch stream, with the engine's own event timing splitting the call into slot 3
      (expansion), 1 (keyswitch), 2 (MS noise reduction) and 0 (rotation + sample extraction);
  (b) host route: ctlist.expand (numpy) + ctlist.cast_to_blocks (every packed LWE gathered twice on the host, then
      Engine.pbs through host buffers); wall clock around calls that end in a stream synchronise (--host-reps
      rounds: the leg is slow),
interleaved in that order.  The two legs must give the same words and every block must decrypt, or nothing is
reported.  Bytes of the expansion kernel are derived from the shapes (stores: rows x (N + 1) words; loads: one mask
polynomial per workgroup and one body word per row).
Writes one JSON document (source_id, hostname) to --out and prints it.
  python tools/expand_bench.py [--counts 2048,8192] [--reps 10] [--host-reps 3] [--out profiles/expand_bench.json]"""
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
from tfhe_amd import ctlist  # noqa: E402

SEED = 0x7F4E0001
EXPAND_ROWS_PER_WG = 8  # expand.hip EX_ROWS
REP = 2


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs_ms": [round(x, 3) for x in ms]}


def host_route(cast, cl):
    return ctlist.cast_to_blocks(cast, ctlist.expand(cl), cl.blocks)


def one_count(cast, ck, cpk, count, reps, host_reps, warmup):
    import torch
    dev = torch.device("cuda", cast.device)
    rng = np.random.default_rng(count)
    packed = rng.integers(0, ctlist.PACKED_MM, count)
    blocks = np.stack([packed % 4, packed // 4], axis=1).reshape(-1).astype(np.uint64)
    cl = ctlist.encrypt_compact(cpk, packed.tolist(), [(ctlist.KIND_UNSIGNED, 2 * count)], rng)
    rows = cl.blocks
    words = ctlist.list_words(cl)
    d_words = torch.from_numpy(words.view(np.int64)).to(dev)
    dev_ms, host_ms, host_out, d_out = [], [], None, None
    cast.timing_reset()
    for r in range(warmup + reps):
        cast.timing(r >= warmup)  # the engine's slots record the timed device legs only
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d_out = ctlist.cast_list_to_blocks_device(cast, cl, d_words=d_words)
        e1.record()
        e1.synchronize()
        cast.timing(False)
        if r >= warmup:
            dev_ms.append(e0.elapsed_time(e1))
        if r < warmup or len(host_ms) < host_reps:
            t = time.perf_counter()
            host_out = host_route(cast, cl)
            if r >= warmup:
                host_ms.append((time.perf_counter() - t) * 1e3)
    slot_ms = {}
    for slot in (3, 1, 2, 0):
        ms, n = cast.timing_stats(slot)
        assert n == reps, (slot, n)
        slot_ms[slot] = ms / reps
    out = d_out.cpu().numpy().view(np.uint64)
    if not np.array_equal(out, host_out):
        raise RuntimeError(f"count {count}: the device and the host route differ")
    if not np.array_equal(ck.decrypt(out, ctlist.PACKED_MM), blocks):
        raise RuntimeError(f"count {count}: cast blocks do not decrypt to the messages")
    res = {"rows": int(rows), "device": stats(dev_ms), "host_route": stats(host_ms)}
    med = res["device"]["median_ms"]
    res["blocks_per_s"] = round(rows / (med * 1e-3))
    res["host_route_blocks_per_s"] = round(rows / (res["host_route"]["median_ms"] * 1e-3))
    res["speedup_over_host_route"] = round(res["host_route"]["median_ms"] / med, 2)
    res["expansion_ms"] = round(slot_ms[3], 4)
    res["keyswitch_ms"] = round(slot_ms[1], 3)
    res["ms_reduce_ms"] = round(slot_ms[2], 3)
    res["rotation_ms"] = round(slot_ms[0], 3)
    res["expansion_share_of_kernel_time"] = round(slot_ms[3] / sum(slot_ms.values()), 5)
    N = cl.lwe_dim
    wgs = -(-rows // EXPAND_ROWS_PER_WG)
    stored, loaded = rows * (N + 1) * 8, wgs * N * 8 + rows * 8
    res["expansion_derived_bytes"] = {"stored": stored, "loaded": loaded}
    res["expansion_derived_GBps"] = round((stored + loaded) / (slot_ms[3] * 1e-3) / 1e9, 1)
    res["rotation_kernel"] = cast.br_kernel(rows)
    res["list_bytes"] = int(words.nbytes)
    res["host_route_upload_bytes"] = int(rows * (N + 1) * 8)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="2048,8192")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "expand_bench.json"))
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]
    params = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_FFT)
    ck, _ = tfhe_amd.gen_keys(params, SEED, with_server_key=False)
    rng = np.random.default_rng(SEED)
    pke_key = rng.integers(0, 2, params.k * params.N).astype(np.uint64)
    cpk = ctlist.gen_compact_public_key(pke_key, rng)
    doc = {"what": "cast_list_to_blocks_device (expansion kernel + casting PBS on resident list words) vs ctlist.expand "
                   "+ cast_to_blocks through host buffers; packed compact lists into P-FHEVM-FFT, rep = 2",
           "source_id": tfhe_amd.source_id(), "hostname": socket.gethostname(), "reps": a.reps,
           "host_reps": a.host_reps, "warmup": a.warmup, "n": params.n, "N": params.N, "rep": REP}
    with tfhe_amd.Engine(params, 0) as cast:
        cast.load_keys(ctlist.casting_keys(ck, pke_key, seed=SEED + 1))
        for count in counts:
            doc[f"count_{count}"] = one_count(cast, ck, cpk, count, a.reps, a.host_reps, a.warmup)
            print(f"count {count}: done", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
