"""Every kernel that takes the LWE dimension n as a run-time argument, on the MI355X away from the preset n: both
keyswitch kernels (ks_mfma.hip, pbs_kernels.hip keyswitch_kernel), the modulus-switch noise reduction (ms_reduce.hip)
and both blind-rotation kernels of all four engines, then the whole PBS.  Inputs and references come from
tests/offpreset_cases.py (tests/test_offpreset_n.py shows on the CPU that they test what they claim); every comparison
of ciphertext words is an integer equality with the oracle.  Every engine is opened at the modified parameters and
takes the full key set through load_keys, so the keyswitch planes are built for n as well."""
import functools
import os

import numpy as np
import pytest

import tfhe_amd
import offpreset_cases as C

pytestmark = pytest.mark.gpu

KERNELS = ("mfma", "valu")
BR_NAMES = {0: ("blind_rotate_lat_kernel", "blind_rotate_kernel"),
            1: ("blind_rotate2048_lat_kernel", "blind_rotate2048_kernel"),
            2: ("blind_rotate_fft_lat_kernel", "blind_rotate_fft_pair_kernel"),
            3: ("blind_rotate_fft2k_kernel", "blind_rotate_fft2k_kernel")}


def _p(preset):
    return f"p{preset}"


def open_engine(ks, kernel="mfma"):
    """An engine at the key set's parameters with the full key set loaded; "valu": the VALU keyswitch kernel, chosen
    by the environment around the constructor only."""
    if kernel == "valu":
        os.environ["TFHE_HIP_KS_VALU"] = "1"
    try:
        eng = tfhe_amd.Engine(ks.params, 0)
    finally:
        os.environ.pop("TFHE_HIP_KS_VALU", None)
    try:
        eng.load_keys(ks.sk)
    except BaseException:
        eng.close()
        raise
    return eng


def both_rotation_kernels(eng, preset, B):
    """Yields the kernel's name with the engine forced onto the latency kernel, then onto the batch kernel."""
    for lat, name in zip((1 << 20, 0), BR_NAMES[preset]):
        eng.set_latency_batch(lat)
        assert eng.br_kernel(B) == name
        yield name


def bad_rows(got, ref):
    return np.nonzero((got != ref).reshape(got.shape[0], -1).any(1))[0][:8].tolist()


# ---- a. keyswitch ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ks_outputs(preset, n, kernel):
    """-> {1: the five rows of the B = 5 input as five batches of one, 5: ..., 257: ...} from one engine."""
    ks = C.keyset_big() if (preset, n) == C.KS_BIG else C.keyset(preset, n)
    case = C.ks_case(preset, n)
    with open_engine(ks, kernel) as eng:
        out = {B: eng.keyswitch(case[B][0]) for B in (5, 257)}
        out[1] = np.concatenate([eng.keyswitch(case[5][0][r:r + 1]) for r in range(5)])
    return out


def check_keyswitch(preset, n, kernel):
    case, out = C.ks_case(preset, n), ks_outputs(preset, n, kernel)
    assert set(out) == set(C.KS_BATCHES)
    ref5 = np.stack([case[5][1][r] for r in range(5)])
    assert out[1].shape == out[5].shape == (5, n + 1) and out[257].shape == (257, n + 1)
    assert np.array_equal(out[1], ref5), f"B = 1, {kernel}: rows {bad_rows(out[1], ref5)}"
    assert np.array_equal(out[5], ref5), f"B = 5, {kernel}: rows {bad_rows(out[5], ref5)}"
    for r, ref in case[257][1].items():
        assert np.array_equal(out[257][r], ref), f"B = 257, {kernel}: row {r}, columns {np.nonzero(out[257][r] != ref)[0][:8]}"
    other = ks_outputs(preset, n, KERNELS[1 - KERNELS.index(kernel)])
    assert np.array_equal(out[257], other[257]), f"the two kernels differ in rows {bad_rows(out[257], other[257])}"


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", C.NS, ids=str)
@pytest.mark.parametrize("preset", C.PRESETS, ids=_p)
def test_keyswitch_off_preset_n(preset, n, kernel):
    check_keyswitch(preset, n, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_keyswitch_above_the_preset_n(kernel):
    """n + 1 = 1040: every 16-column tile full, the body in the last lane of the last one; 16 full 64-column tiles
    and a ragged one on the VALU kernel."""
    check_keyswitch(*C.KS_BIG, kernel)


# ---- b. rotation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.ROT_NS, ids=str)
@pytest.mark.parametrize("preset", C.PRESETS, ids=_p)
def test_rotation_off_preset_n(preset, n):
    cts, lut, ref_acc, ref_out = C.rot_case(preset, n)
    ks = C.keyset(preset, n)
    with open_engine(ks) as eng:
        try:
            for kernel in both_rotation_kernels(eng, preset, C.ROT_B):
                acc = eng.blind_rotate(cts, lut)
                assert acc.shape == ref_acc.shape
                for q in range(C.ROT_B):
                    for c in range(ks.prm.k + 1):
                        got, want = acc[q].reshape(-1, ks.prm.N)[c], ref_acc[q].reshape(-1, ks.prm.N)[c]
                        assert np.array_equal(got, want), \
                            f"blind_rotate on {kernel}: row {q} component {c}, words {np.nonzero(got != want)[0][:8]}"
                out = eng.bootstrap(cts, lut)
                assert np.array_equal(out, ref_out), f"bootstrap on {kernel}: rows {bad_rows(out, ref_out)}"
        finally:
            eng.set_latency_batch(C.LAT_DEFAULT[preset])


# ---- c. noise reduction ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.NS, ids=str)
@pytest.mark.parametrize("preset", C.MS_PRESETS, ids=_p)
def test_ms_reduce_off_preset_n(preset, n):
    cs = C.ms_case(preset, n)
    with open_engine(cs.ks) as eng:
        for name, bound in (("half-minimum", cs.bound_half), ("2 % quantile", cs.bound_q)):
            ref, rpicks = cs.reference(bound)
            eng.load_ms_key(cs.zeros, bound=bound)
            out, picks = eng.ms_reduce(cs.cts)
            assert np.array_equal(picks, rpicks), f"{name}: device {picks.tolist()} oracle {rpicks.tolist()}"
            assert np.array_equal(out, ref), f"{name}: rows {bad_rows(out, ref)}"


@pytest.mark.parametrize("preset", C.MS_PRESETS, ids=_p)
def test_ms_reduce_default_bound_is_an_early_out(preset):
    """With the bound of load_keys (2^58) every row at this n is within the bound before any zero is read."""
    cs = C.ms_case(preset, C.MS_DEFAULT_N)
    with open_engine(cs.ks) as eng:
        out, picks = eng.ms_reduce(cs.cts)
    assert (picks == -1).all() and np.array_equal(out, cs.cts)


# ---- d. the whole PBS ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.PBS_NS, ids=str)
@pytest.mark.parametrize("preset", C.PRESETS, ids=_p)
def test_pbs_off_preset_n(preset, n):
    cs = C.pbs_case(preset, n)
    ks = cs.ks
    ref, _ = cs.reference()
    with open_engine(ks) as eng:
        try:
            if ks.prm.order == 1:
                eng.load_ms_key(ks.sk.ms_zeros, bound=cs.bound)
            for kernel in both_rotation_kernels(eng, preset, C.PBS_B):
                out = eng.pbs(cs.cts, cs.luts, cs.lut_index)
                assert np.array_equal(out, ref), f"pbs on {kernel}: rows {bad_rows(out, ref)}"
                assert np.array_equal(cs.decode(out), cs.want)
            if ks.prm.order == 1:
                plain, _ = cs.reference(reduce=False)
                eng.load_ms_key(None)
                for kernel in both_rotation_kernels(eng, preset, C.PBS_B):
                    out = eng.pbs(cs.cts, cs.luts, cs.lut_index)
                    assert np.array_equal(out, plain), f"pbs without the reduction on {kernel}: rows {bad_rows(out, plain)}"
                    assert np.array_equal(cs.decode(out), cs.want)
        finally:
            eng.set_latency_batch(C.LAT_DEFAULT[preset])
