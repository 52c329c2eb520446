"""Multi-bit PBS against the classic kernels at n = 924 (preset 4), one secret key set, one process, one box:
    python tools/mb_sweep.py [--out profiles/multibit_sweep.txt] [--reps 20] [--batches 2,32,256,4096]
Configurations: classic keys (the parent's kernels: latency kernel up to 512, batch kernel above) and multi-bit keys
g = 2, 3, 4.  Per batch size every configuration is warmed up (3 calls), then `reps` rounds run the configurations
interleaved, one synchronous Engine.pbs (host arrays in and out: upload, keyswitch, blind rotation, download) each;
reported: the median and the min .. max of the host clock around the call, and the median of the blind rotation's
own device time (HIP events, timing slot 0).  Every output is checked by decryption.  No GPU: the tool fails."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_amd  # noqa: E402

SEED = 0x7F4E0001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "multibit_sweep.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="2,32,256,4096")
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    p = tfhe_amd.Params.preset(tfhe_amd.PRESET_FHEVM_MB_FFT)
    ck, sk = tfhe_amd.gen_keys(p, SEED)
    sk.ms_zeros = None                       # the same pipeline on every side: no modulus-switch noise reduction
    engines = {"classic": tfhe_amd.Engine(p, 0).load_keys(sk)}
    del sk
    for g in (2, 3, 4):
        skg = tfhe_amd.server_keygen(ck, SEED, grouping=g)
        engines[f"mb g={g}"] = tfhe_amd.Engine(p, 0).load_keys(skg)
        del skg
    table = [(3 * v + 1) % 16 for v in range(16)]
    lut = tfhe_amd.lut_from_table(p.N, 16, table, (1 << 63) // 16)
    lines = [f"# tools/mb_sweep.py  source_id {tfhe_amd.source_id()}  n = {p.n}, N = {p.N}, reps = {a.reps}, interleaved",
             "# Engine.pbs wall time per call, ms: median (min .. max) | blind rotation device time, ms: median",
             f"# {'B':>5} {'config':<9} {'kernel':<30} {'pbs ms':>9} {'min':>9} {'max':>9} {'br ms':>9} {'vs classic':>10}"]
    for B in batches:
        msgs = np.arange(B) % 16
        cts = ck.encrypt(msgs, 16, seed=0x5EE0 + B)
        want = [table[m] for m in msgs]
        wall = {k: [] for k in engines}
        dev = {k: [] for k in engines}
        for k, e in engines.items():
            for _ in range(3):
                out = e.pbs(cts, lut)
            assert list(ck.decrypt(out, 16)) == want, (B, k)
            e.timing(True)
        for _ in range(a.reps):
            for k, e in engines.items():
                e.timing_reset()
                t0 = time.perf_counter()
                e.pbs(cts, lut)
                wall[k].append((time.perf_counter() - t0) * 1e3)
                ms, cnt = e.timing_stats(0)
                dev[k].append(ms / max(cnt, 1))
        for e in engines.values():
            e.timing(False)
        base = statistics.median(dev["classic"])
        for k, e in engines.items():
            w, d = statistics.median(wall[k]), statistics.median(dev[k])
            lines.append(f"  {B:>5} {k:<9} {e.br_kernel(B):<30} {w:>9.3f} {min(wall[k]):>9.3f} {max(wall[k]):>9.3f} "
                         f"{d:>9.3f} {d / base:>9.2f}x")
        print("\n".join(lines[-len(engines):]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
