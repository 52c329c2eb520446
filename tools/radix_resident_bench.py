"""Radix circuits on one MI355X: the host mode (every block a host array, each level through Engine.pbs) against the
device-resident mode (RadixCircuit(engine, device=...): blocks stay in HBM, each level is one term description
through Engine.lincomb_pbs_device), same box, same process, same encrypted inputs.

Workloads, at P-FHEVM on the FFT64 transform, keys from a fixed seed:
  add / lt / mul   euint64, --batch values (default 256), one operator per run
  kats             the reference's fhEVM operator KATs up to euint64 in one run_many (tests/golden/fhevm_kats.json)
After one warm-up run per mode, --reps runs alternate host and device mode.  A run is wall clock from the first
coroutine step to the end of a device synchronise: host mode ends with its results in host arrays, device mode with
its results in device buffers (to_host() is timed apart, once).  The inputs are encrypted before the clock starts and,
in device mode, already uploaded.  The two modes must give the same words, or nothing is reported.
  kernel           tfhe_hip_lwe_lincomb_async alone on --rows rows (default 4096) x 2 terms at dim 2049, next to
                   tfhe_hip_pbs_async of the same rows: the engine's own HIP event pairs (slot 3 for the assembly;
                   slots 1, 2, 0 for keyswitch, noise reduction and rotation), median of --reps launches each.  The
                   bar: the assembly takes under 1 % of the PBS.
Writes one JSON document (source_id, hostname) to --out and prints it.
  python tools/radix_resident_bench.py [--batch 256] [--rows 4096] [--reps 5] [--out profiles/radix_resident_bench.json]"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tfhe_amd  # noqa: E402
from tfhe_amd import radix as R  # noqa: E402

SEED = 0x7F4E0001
DEVICE = "cuda:0"


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs_ms": [round(x, 3) for x in ms]}


def width(t):
    return 1 if t == "ebool" else int(t.lstrip("e").replace("uint", ""))


def load_kats(max_width):
    with open(os.path.join(ROOT, "tests", "golden", "fhevm_kats.json")) as f:
        kats = json.load(f)
    keep = [k for k in kats if k["op"] in R.RADIX_OPS and max(width(t) for t in k["types"] + [k["result_type"]]) <= max_width]
    return [dict(k, args=[int(a) for a in k["args"]], expect=int(k["expect"])) for k in keep]


def words(r):
    return r.to_host() if isinstance(r, R.RadixUint) else np.asarray(r)


def timed(c, make_ops):
    import torch
    ops = make_ops()
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = c.run_many(ops)
    torch.cuda.synchronize()
    return res, (time.perf_counter() - t) * 1e3


def compare(name, eng, prepare, reps):
    """prepare(circuit) -> make_ops; host and device mode alternate, reps timed runs each after one warm-up."""
    import torch
    modes = {"host": R.RadixCircuit(eng), "device": R.RadixCircuit(eng, device=DEVICE)}
    make = {m: prepare(c) for m, c in modes.items()}
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    ref = None
    for r in range(reps + 1):
        for m, c in modes.items():
            res, t = timed(c, make[m])
            if r:
                ms[m].append(t)
                continue
            t0 = time.perf_counter()
            w = [words(x) for x in res]
            if m == "device":
                download_ms = (time.perf_counter() - t0) * 1e3
                if not all(np.array_equal(a, b) for a, b in zip(ref, w)):
                    raise RuntimeError(f"{name}: host and device mode differ")
            ref = w
        print(f"{name}: run {r} done", file=sys.stderr, flush=True)
    out = {m: stats(v) for m, v in ms.items()}
    c = modes["device"]
    out.update(pbs=c.pbs_count // (reps + 1), launches=c.launches // (reps + 1), max_terms=c.max_terms,
               device_to_host_once_ms=round(download_ms, 3),
               host_over_device=round(out["host"]["median_ms"] / out["device"]["median_ms"], 3),
               device_not_slower=bool(out["device"]["median_ms"] <= out["host"]["median_ms"]))
    return out


def operator_workload(ck, op, batch):
    rng = np.random.default_rng(64)
    a = rng.integers(0, 1 << 63, batch, dtype=np.uint64)
    b = rng.integers(0, 1 << 63, batch, dtype=np.uint64)

    def prepare(c):
        A = R.RadixUint.encrypt(c, ck, a, 64, seed=1, stream0=0)
        Bv = R.RadixUint.encrypt(c, ck, b, 64, seed=1, stream0=batch * 32)
        return lambda: [R.fhevm_op(c, op, A, Bv)]
    return prepare


def kat_workload(ck, kats):
    def prepare(c):
        argv, stream = [], 0
        for k in kats:
            args = []
            for t, v in zip(k["types"], k["args"]):
                if t.startswith("e"):
                    args.append(R.RadixUint.encrypt(c, ck, [v], width(t), seed=0x5AD1, stream0=stream))
                    stream += width(t) // 2
                else:
                    args.append(int(v))
            argv.append(args)
        return lambda: [R.fhevm_op(c, k["op"], *args) for k, args in zip(kats, argv)]
    return prepare


def kernel_alone(eng, ck, rows, reps):
    import torch
    dim = eng.params.io_dim + 1
    rng = np.random.default_rng(7)
    src = torch.from_numpy(ck.encrypt(rng.integers(0, 4, 2 * rows), R.SPACE, seed=3).view(np.int64)).to(DEVICE)
    row_start = np.arange(0, 2 * rows + 1, 2, dtype=np.uint32)
    term_row = rng.permutation(2 * rows).astype(np.uint32)          # every source row once: no reuse from a cache
    term_coef = np.tile(np.array([R.MSG, 1], dtype=np.uint64), rows)
    desc = (row_start, np.zeros(2 * rows, dtype=np.uint32), term_row, term_coef, None)
    luts = torch.from_numpy(np.stack([eng_lut(eng, R.T_AND)]).view(np.int64)).to(DEVICE)
    lin_ms, pbs_ms = [], []
    for r in range(reps + 2):
        eng.timing_reset()
        eng.timing(True)
        lin = eng.lincomb_device([src], *desc)
        torch.cuda.synchronize()
        t_lin = eng.timing_stats(3)[0]
        eng.timing_reset()
        out = eng.pbs_device(lin, luts)
        torch.cuda.synchronize()
        t_pbs = sum(eng.timing_stats(s)[0] for s in (0, 1, 2))
        eng.timing(False)
        if r >= 2:
            lin_ms.append(t_lin)
            pbs_ms.append(t_pbs)
    del out
    moved = rows * dim * 8 * 3
    res = {"rows": rows, "terms_per_row": 2, "dim": dim, "lincomb": stats(lin_ms), "pbs": stats(pbs_ms),
           "bytes_moved": moved, "rotation_kernel": eng.br_kernel(rows)}
    res["lincomb_gb_per_s"] = round(moved / (res["lincomb"]["median_ms"] * 1e-3) / 1e9, 1)
    res["lincomb_share_of_pbs"] = round(res["lincomb"]["median_ms"] / res["pbs"]["median_ms"], 5)
    res["under_one_percent_of_pbs"] = bool(res["lincomb_share_of_pbs"] < 0.01)
    return res


def eng_lut(eng, table):
    return tfhe_amd.lut_from_table(eng.params.N, R.SPACE, list(table), R.DELTA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kat-width", type=int, default=64)
    ap.add_argument("--only", default="", help="comma-separated subset of add,lt,mul,kats,kernel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radix_resident_bench.json"))
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    params = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_FFT)
    ck, sk = tfhe_amd.gen_keys(params, SEED)
    doc = {"what": "RadixCircuit host mode (host arrays, Engine.pbs per level) vs device mode (LinBlocks over device "
                   "buffers, Engine.lincomb_pbs_device per level); and the lincomb kernel next to the PBS of its rows",
           "preset": "P-FHEVM-FFT", "source_id": tfhe_amd.source_id(), "hostname": socket.gethostname(), "reps": a.reps,
           "batch": a.batch}
    with tfhe_amd.Engine(params, 0) as eng:
        eng.load_keys(sk)
        if not only or "kernel" in only:
            doc["kernel"] = kernel_alone(eng, ck, a.rows, max(a.reps, 5))
            print("kernel: done", file=sys.stderr, flush=True)
        for op in ("add", "lt", "mul"):
            if not only or op in only:
                doc[f"euint64 {op}"] = compare(f"euint64 {op}", eng, operator_workload(ck, op, a.batch), a.reps)
        if not only or "kats" in only:
            kats = load_kats(a.kat_width)
            doc["kats"] = dict(compare("kats", eng, kat_workload(ck, kats), a.reps), count=len(kats),
                               max_width=a.kat_width)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
