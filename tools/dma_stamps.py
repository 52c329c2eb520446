"""Issue cost of the pair kernel's LDS-DMA bursts (diagnostic build only: make -C tfhe_amd B=../build_diag/ds/obj
LIB=../build_diag/ds/libtfhe_hip.so EXTRA=-DFFT_DMASTAMP=1; run with TFHE_HIP_LIB=build_diag/ds/libtfhe_hip.so).
Per wave of workgroups 0..63 of a full batch, the shader-clock cycles (s_memtime) between the instruction before and
the instruction after the eight 1 KB pieces of a level step, as the mean over the CMUXes, per site q = 0, 1, 2, and
the three sites together as a fraction of the wave's time per CMUX.
  python tools/dma_stamps.py [--batch 4096]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    params = tfhe_amd.Params.preset(tfhe_amd.PRESET_GATE_FFT)
    ck, sk = tfhe_amd.gen_keys(params, 0x7F4E0001)
    eng = tfhe_amd.Engine(params, 0).load_keys(sk)
    eng.set_latency_batch(0)
    cts = ck.encrypt_bool(np.random.default_rng(1).integers(0, 2, a.batch).astype(bool), seed=0xC0FFEE01)
    for _ in range(3):
        eng.pbs(cts, eng.gate_lut())
    buf = np.zeros(64 * 4 * 4, dtype=np.uint64)
    f = tfhe_amd.lib().tfhe_hip_debug_dmastamps
    f.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    assert f(buf.ctypes.data, buf.size) == 0
    wgs = min(64, (a.batch + 1) // 2)
    t = buf.reshape(64, 4, 4)[:wgs].astype(np.float64) / params.n   # cycles per CMUX: q = 0, 1, 2, whole CMUX
    per_wave = t.reshape(-1, 4)
    site = per_wave[:, :3]
    res = {"batch": a.batch, "workgroups": wgs, "clock": "s_memtime",
           "burst_cycles_mean": [round(x, 1) for x in site.mean(axis=0)],
           "burst_cycles_min": [round(x, 1) for x in site.min(axis=0)],
           "burst_cycles_max": [round(x, 1) for x in site.max(axis=0)],
           "cmux_cycles_mean": round(per_wave[:, 3].mean(), 1),
           "bursts_share_of_cmux": round(float((site.sum(axis=1) / per_wave[:, 3]).mean()), 4),
           "per_wave_of_wg0": [[round(x, 1) for x in row] for row in t[0]]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
