"""Many-LUT PBS against the single-table PBS on one MI355X, device-resident, one process.

For P-FHEVM and P-GATE on the FFT64 transform, B ciphertexts in HBM: after warm-up, --reps rounds of
  (a) one pbs call, (b) pbs_many with n_fn = 2, (c) two pbs calls
interleaved in that order, each timed by a pair of HIP events on the launch stream; median and min of each.  (a) is
the path the many-LUT work does not touch, so it is the baseline: (b) should cost one blind rotation plus the
accumulator round trip of the extraction kernel, (c) two rotations.
Then a euint64 add over --add-batch values on P-FHEVM FFT64 (host-array radix circuit), with and without
RadixCircuit(many_lut=True): wall time and blind rotations.
Writes one JSON document (source_id, hostname) to --out and prints it.
  python tools/many_lut_bench.py [--batch 4096] [--reps 10] [--add-batch 256] [--out profiles/many_lut_bench.json]"""
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
from tfhe_amd import radix as R  # noqa: E402


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs_ms": [round(x, 3) for x in ms]}


def pbs_legs(eng, ck, B, reps, warmup, mm):
    import torch
    p = eng.params
    dev = torch.device("cuda", eng.device)
    rng = np.random.default_rng(B)
    half, delta = mm // 2, (1 << 63) // mm
    t0, t1 = [int(v) for v in rng.integers(0, mm, half)], [int(v) for v in rng.integers(0, mm, half)]
    many, stride = tfhe_amd.lut_many(p.N, mm, [t0, t1], delta)
    single = [tfhe_amd.lut_from_table(p.N, mm, t + [0] * half, delta) for t in (t0, t1)]
    m = rng.integers(0, half, B)
    d_in = torch.from_numpy(ck.encrypt(m, mm, seed=0xBE7C).view(np.int64)).to(dev)
    d_many = torch.from_numpy(many.view(np.int64)).to(dev)
    d_single = [torch.from_numpy(s.view(np.int64)).to(dev) for s in single]
    d_one = torch.empty_like(d_in)
    d_two = torch.empty_like(d_in)
    d_out = torch.empty((B, 2, d_in.shape[1]), dtype=d_in.dtype, device=dev)
    legs = {
        "pbs": lambda: eng.pbs_async(d_in, d_single[0], d_one),
        "pbs_many_2": lambda: eng.pbs_many_async(d_in, d_many, d_out, 2, stride),
        "two_pbs": lambda: (eng.pbs_async(d_in, d_single[0], d_one), eng.pbs_async(d_in, d_single[1], d_two)),
    }
    ms = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            t = timed(fn)
            if r >= warmup:
                ms[k].append(t)
    # the three legs computed the same functions: a wrong many-LUT result is not a measurement
    two = np.stack([d_one.cpu().numpy(), d_two.cpu().numpy()], axis=1).view(np.uint64)
    out = d_out.cpu().numpy().view(np.uint64)
    want = [[t0[x] for x in m], [t1[x] for x in m]]
    ok = all([int(v) for v in ck.decrypt(a[:, f], mm)] == want[f] for a in (two, out) for f in range(2))
    res = {k: stats(v) for k, v in ms.items()}
    res["many_over_single"] = round(res["pbs_many_2"]["median_ms"] / res["pbs"]["median_ms"], 4)
    res["many_over_two"] = round(res["pbs_many_2"]["median_ms"] / res["two_pbs"]["median_ms"], 4)
    res["decrypt_ok"] = bool(ok)
    res["kernel"] = eng.br_kernel(B)
    acc_bytes = (p.k + 1) * p.N * 8
    # over a plain pbs: the accumulator written and read back, and one more output row
    res["derived_extra_bytes_per_pbs"] = 2 * acc_bytes + (p.k * p.N + 1) * 8
    res["msg_modulus"] = mm
    return res


def add_legs(eng, ck, B, reps):
    rng = np.random.default_rng(64)
    a = rng.integers(0, 1 << 63, B, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    b = rng.integers(0, 1 << 63, B, dtype=np.uint64) * np.uint64(2)
    res = {}
    walls = {False: [], True: []}
    for r in range(reps + 1):
        for many in (False, True):
            c = R.RadixCircuit(eng, many_lut=many)
            A = R.RadixUint.encrypt(c, ck, a, 64, seed=0xADD, stream0=0)
            Bv = R.RadixUint.encrypt(c, ck, b, 64, seed=0xADD, stream0=32 * B)
            t = time.perf_counter()
            s = c.run(R.fhevm_op(c, "add", A, Bv))
            wall = time.perf_counter() - t
            if r:
                walls[many].append(wall * 1e3)
            res["many_lut" if many else "default"] = {
                "rotations": c.pbs_count, "launches": c.launches,
                "ok": bool(np.array_equal(s.decrypt(ck), a + b))}
    for many, key in ((False, "default"), (True, "many_lut")):
        res[key].update(stats(walls[many]))
    res["wall_ratio"] = round(res["many_lut"]["median_ms"] / res["default"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--add-batch", type=int, default=256)
    ap.add_argument("--add-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "many_lut_bench.json"))
    a = ap.parse_args()
    doc = {"what": "pbs vs pbs_many(n_fn=2) vs two pbs, device-resident, HIP events; euint64 add with/without many_lut",
           "source_id": tfhe_amd.source_id(), "hostname": socket.gethostname(), "batch": a.batch, "reps": a.reps,
           "warmup": a.warmup}
    # message spaces the parameter sets decrypt reliably: 4 bits on P-FHEVM, 2 bits on P-GATE
    for name, preset, mm in (("fhevm_fft", tfhe_amd.PRESET_FHEVM_FFT, 16), ("gate_fft", tfhe_amd.PRESET_GATE_FFT, 4)):
        params = tfhe_amd.Params.preset(preset)
        ck, sk = tfhe_amd.gen_keys(params, 0x7F4E0001)
        with tfhe_amd.Engine(params, 0) as eng:
            eng.load_keys(sk)
            doc[name] = pbs_legs(eng, ck, a.batch, a.reps, a.warmup, mm)
            if name == "fhevm_fft":
                doc["euint64_add"] = dict(add_legs(eng, ck, a.add_batch, a.add_reps), batch=a.add_batch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
