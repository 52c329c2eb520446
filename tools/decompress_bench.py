"""Decompression of compressed ciphertext lists on one MI355X: Decompressor.decompress_device against the route that
existed before it, same box, same run.

ML2048 packing parameters (1 x 2048, 2048 LWEs per GLWE, 26 stored bits) into P-FHEVM on the FFT64 transform: the
decompression context rotates ciphertexts of dimension n = 2048.  For each --counts entry, a list of that many 4-bit
messages is encrypted, packed on the device and compressed on the host; then, after warm-up, --reps rounds of
  (a) device: decompress_device on the resident packed words (unpack / extract kernel + blind rotation), timed by a
      pair of HIP events on the launch stream, with the engine's own event timing splitting the call into slot 3
      (unpack / extract) and slot 0 (rotation + sample extraction);
  (b) host route: tfhe_hip_pks_extract and numpy extract_lwe per ciphertext on the host, then tfhe_hip_blind_rotate and
      tfhe_hip_sample_extract through host buffers; wall clock around calls that end in a stream synchronise
      (--host-reps rounds: the leg is slow),
interleaved in that order.  The two legs must give the same words and every output must decrypt, or nothing is
reported.  Bytes of the unpack kernel are derived from the shapes (stores: count x (kN + 1) words; loads: one packed
polynomial per workgroup).
Writes one JSON document (source_id, hostname) to --out and prints it.
  python tools/decompress_bench.py [--counts 2048,8192] [--reps 10] [--host-reps 3] [--out profiles/decompress_bench.json]"""
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

SEED = 0x7F4E0001
UNPACK_ROWS_PER_WG = 8  # decompress.hip DX_ROWS


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs_ms": [round(x, 3) for x in ms]}


def host_route(dec, comp):
    """Extract on the host, rotate and sample-extract through host buffers."""
    pp = dec.key.pks_params
    lwes = np.stack([C.extract_lwe(pp, glwe, i) for glwe, bodies in ((c.extract(), c.bodies) for c in comp)
                     for i in range(bodies)])
    return dec.engine.sample_extract(dec.engine.blind_rotate(lwes, dec.identity_lut()))


def one_count(dec, packer, ck, count, reps, host_reps, warmup):
    import torch
    p, pp = dec.key.params, dec.key.pks_params
    dev = torch.device("cuda", dec.device)
    msgs = np.random.default_rng(count).integers(0, 16, count).astype(np.uint64)
    comp = packer.compress_ciphertexts_into_list(ck.encrypt(msgs, 16, seed=0xDEC0))
    packed, n = C.concat_list(pp, comp)
    assert n == count
    d_packed = torch.from_numpy(packed.view(np.int64)).to(dev)
    d_lut = torch.from_numpy(dec.identity_lut().view(np.int64)).to(dev)
    d_out = torch.empty((count, p.k * p.N + 1), dtype=torch.int64, device=dev)
    eng = dec.engine
    dev_ms, host_ms, host_out = [], [], None
    eng.timing_reset()
    for r in range(warmup + reps):
        eng.timing(r >= warmup)  # the engine's slots record the timed device legs only
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.decompress_async(d_packed, count, d_lut, d_out)
        e1.record()
        e1.synchronize()
        eng.timing(False)
        if r >= warmup:
            dev_ms.append(e0.elapsed_time(e1))
        if r < warmup or len(host_ms) < host_reps:
            t = time.perf_counter()
            host_out = host_route(dec, comp)
            if r >= warmup:
                host_ms.append((time.perf_counter() - t) * 1e3)
    unpack_ms, unpack_n = eng.timing_stats(3)
    rot_ms, rot_n = eng.timing_stats(0)
    assert unpack_n == reps and rot_n == reps, (unpack_n, rot_n)
    out = d_out.cpu().numpy().view(np.uint64)
    if not np.array_equal(out, host_out):
        raise RuntimeError(f"count {count}: the device and the host route differ")
    if not np.array_equal(ck.decrypt(out, 16), msgs):
        raise RuntimeError(f"count {count}: decompressed ciphertexts do not decrypt to the messages")
    res = {"device": stats(dev_ms), "host_route": stats(host_ms)}
    med = res["device"]["median_ms"]
    res["lwes_per_s"] = round(count / (med * 1e-3))
    res["host_route_lwes_per_s"] = round(count / (res["host_route"]["median_ms"] * 1e-3))
    res["speedup_over_host_route"] = round(res["host_route"]["median_ms"] / med, 2)
    res["unpack_extract_ms"] = round(unpack_ms / reps, 4)
    res["rotation_ms"] = round(rot_ms / reps, 3)
    res["unpack_share_of_kernel_time"] = round(unpack_ms / (unpack_ms + rot_ms), 5)
    kN = pp.out_k * pp.out_N
    groups = -(-count // pp.lwe_per_glwe)
    wgs = groups * -(-pp.lwe_per_glwe // UNPACK_ROWS_PER_WG) * pp.out_k
    stored, loaded = count * (kN + 1) * 8, wgs * pp.out_N * pp.storage_log // 8
    res["unpack_derived_bytes"] = {"stored": stored, "loaded": loaded}
    res["unpack_derived_GBps"] = round((stored + loaded) / (unpack_ms / reps * 1e-3) / 1e9, 1)
    res["rotation_kernel"] = eng.br_kernel(count)
    res["packed_bytes"] = int(packed.nbytes)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="2048,8192")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "decompress_bench.json"))
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]
    params = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_FFT)
    pp = C.PksParams.preset(C.PKS_PRESET_ML2048)
    ck, _ = tfhe_amd.gen_keys(params, SEED, with_server_key=False)
    key = C.CompressionKey(pp, SEED, ck.glwe_key)
    dk = C.DecompressionKey(params, pp, key.post_packing_key, ck.glwe_key, SEED + 1)
    doc = {"what": "decompress_device (unpack/extract kernel + blind rotation) vs host extract + blind_rotate + "
                   "sample_extract through host buffers; ML2048 lists into P-FHEVM-FFT, n = 2048",
           "source_id": tfhe_amd.source_id(), "hostname": socket.gethostname(), "reps": a.reps,
           "host_reps": a.host_reps, "warmup": a.warmup, "n": dk.params.n, "N": params.N,
           "pks": {f: getattr(pp, f) for f, _ in pp._fields_}}
    packer = C.Packer(pp, 0).load_key(key)
    try:
        with C.Decompressor(dk, 0) as dec:
            for count in counts:
                doc[f"count_{count}"] = one_count(dec, packer, ck, count, a.reps, a.host_reps, a.warmup)
    finally:
        packer.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
