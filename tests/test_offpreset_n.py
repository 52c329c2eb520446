"""The off-preset-n cases of tests/offpreset_cases.py, checked on the CPU from the oracle alone: the product's key
generation equals the oracle's at every (preset, n), the crafted rotation rows switch to the intended amounts, the
explicit noise-reduction bounds make the oracle scan (so the device test cannot pass by never scanning), and the
whole-PBS references decrypt.  tests/test_gpu_offpreset_n.py runs the same inputs on the device."""
import numpy as np
import pytest

import offpreset_cases as C

KEY_NS = sorted(set(C.NS) | set(C.ROT_NS))


def _id(v):
    return str(v)


@pytest.mark.parametrize("n", KEY_NS, ids=_id)
@pytest.mark.parametrize("preset", C.PRESETS, ids=lambda p: f"p{p}")
def test_product_keys_equal_oracle_keys(preset, n):
    ks = C.keyset(preset, n)
    assert (ks.params.n, ks.prm.n) == (n, n) and ks.params.as_dict() == {f: getattr(ks.prm, f) for f, _ in ks.prm._fields_}
    assert np.array_equal(ks.ck.lwe_key, ks.okeys.lwe_key) and np.array_equal(ks.ck.glwe_key, ks.okeys.glwe_key)
    assert ks.sk.bsk.size and np.array_equal(ks.sk.bsk, ks.okeys.bsk)
    assert ks.sk.ksk.size == ks.big_dim * ks.prm.ks_level * (n + 1) and np.array_equal(ks.sk.ksk, ks.okeys.ksk)
    if ks.prm.order == 1:
        assert ks.sk.ms_zeros.shape == (1449, n + 1) and np.array_equal(ks.sk.ms_zeros, ks.okeys.ms_zeros)
    else:
        assert ks.sk.ms_zeros is None and ks.okeys.ms_zeros is None


def test_keyswitch_key_above_the_preset_equals_oracle():
    ks = C.keyset_big()
    assert ks.prm.n == C.KS_BIG[1] > C.oracle().params(C.KS_BIG[0]).n and (ks.prm.n + 1) % 16 == 0
    assert np.array_equal(ks.sk.ksk, ks.okeys.ksk)


def test_keyswitch_rows_hold_the_edges():
    """Rows 0 - 4 of every keyswitch input: 0, all ones, 2^63, ties of the closest-representable step, one below."""
    for B, (big, ref) in C.ks_case(2, 16).items():
        assert big.shape == (B, 1025) and set(ref) == set(range(5) if B == 5 else C.KS_ROWS_257)
        assert not big[0].any() and (big[1] == 2 ** 64 - 1).all() and (big[2] == 2 ** 63).all()
        low = np.uint64((1 << (64 - C.KS_PREC_BITS)) - 1)
        assert ((big[3] & low) == 1 << (63 - C.KS_PREC_BITS)).all()
        assert ((big[4] & low) == (1 << (63 - C.KS_PREC_BITS)) - 1).all()
        assert ref[0].shape == (17,) and not ref[0].any() and ref[3].any()


@pytest.mark.parametrize("N", (1024, 2048))
def test_crafted_rows_switch_to_the_intended_amounts(N):
    O = C.oracle()
    want = C.amounts(N)
    assert {0, 1, 63, 64, 65, N - 1, N, N + 1, 2 * N - 64, 2 * N - 1} <= set(want) and max(want) < 2 * N
    assert any(a == b for a, b in zip(want, want[1:])) and want[0] == want[-1] == 0
    for n in (16, 64):
        (row0, row1), (a0, a1) = C.crafted_masks(N, n)
        assert O.mod_switch(row0, 2 * N).tolist() == a0.tolist() == np.resize(want, n).tolist()
        assert O.mod_switch(row1, 2 * N).tolist() == a1.tolist() == np.resize(want, n)[::-1].tolist()
        assert set(want) <= set(a0.tolist())  # n = 16 already holds every amount


@pytest.mark.parametrize("n", C.ROT_NS, ids=_id)
@pytest.mark.parametrize("preset", C.PRESETS, ids=lambda p: f"p{p}")
def test_rotation_case_inputs(preset, n):
    """The rows the device test sends are the crafted ones, and the LUT has full-width words of its ring."""
    O = C.oracle()
    cts, lut, acc, out = C.rot_case(preset, n)
    ks = C.keyset(preset, n)
    N = ks.prm.N
    assert cts.shape == (C.ROT_B, n + 1) and acc.shape == (C.ROT_B, 2 * N) and out.shape == (C.ROT_B, N + 1)
    assert not cts[2, :n].any()
    if n >= 16:
        assert O.mod_switch(cts[0, :n], 2 * N).tolist() == np.resize(C.amounts(N), n).tolist()
        assert O.mod_switch(cts[1, :n], 2 * N).tolist() == np.resize(C.amounts(N), n)[::-1].tolist()
    if ks.fft:
        assert (lut >> np.uint64(63)).any() and (lut & np.uint64(0xFFFFFFFF)).any()
    else:
        assert lut.max() == C.GOLDILOCKS - 1 and lut.min() == 0
    # row 2 rotates by the body alone: the accumulator's mask polynomial stays 0 on both rings
    assert not acc[2, :N].any() and acc[:, :N].any()


@pytest.mark.parametrize("n", C.NS, ids=_id)
@pytest.mark.parametrize("preset", C.MS_PRESETS, ids=lambda p: f"p{p}")
def test_explicit_bounds_make_the_oracle_scan(preset, n):
    cs = C.ms_case(preset, n)
    assert cs.cts.shape == (C.MS_B, n + 1) and cs.measures.shape == (4, 1449)
    # half the smallest measure: no zero is within the bound, every row scans the whole key and takes a minimiser
    red, picks = cs.reference(cs.bound_half)
    print("half-minimum bound 2^%.2f: picks %s" % (np.log2(cs.bound_half), picks.tolist()))
    assert (picks >= 0).all()
    # the 2 % quantile: early exits, and at least one of them past the first 64-zero tile
    red_q, picks_q = cs.reference(cs.bound_q)
    print("2 %% quantile bound 2^%.2f: picks %s" % (np.log2(cs.bound_q), picks_q.tolist()))
    assert (picks_q >= 0).sum() * 2 >= C.MS_B and picks_q.max() >= 64
    for r, p in ((red, picks), (red_q, picks_q)):
        with np.errstate(over="ignore"):
            want = np.where((p >= 0)[:, None], cs.cts + cs.zeros[np.maximum(p, 0)], cs.cts)
        assert np.array_equal(r, want)


@pytest.mark.parametrize("n", C.NS, ids=_id)
@pytest.mark.parametrize("preset", C.MS_PRESETS, ids=lambda p: f"p{p}")
def test_default_bound_never_scans_at_small_n(preset, n):
    """The trap the explicit bounds are there for: every row's own measure is already under 2^58."""
    cs = C.ms_case(preset, n)
    assert (cs.own < 2.0 ** 58).all()
    if n == C.MS_DEFAULT_N:
        O = C.oracle()
        red, picks = O.ms_reduce(cs.ks.prm, cs.ks.okeys, cs.cts)
        assert (picks == -1).all() and np.array_equal(red, cs.cts)


@pytest.mark.parametrize("n", C.PBS_NS, ids=_id)
@pytest.mark.parametrize("preset", C.PRESETS, ids=lambda p: f"p{p}")
def test_pbs_references_decrypt(preset, n):
    cs = C.pbs_case(preset, n)
    out, picks = cs.reference()
    assert np.array_equal(cs.decode(out), cs.want)
    if cs.ks.prm.order == 1:
        plain, _ = cs.reference(reduce=False)
        print("picks", picks.tolist())
        assert np.array_equal(cs.decode(plain), cs.want)
        assert (picks >= 0).any() and not np.array_equal(out, plain)  # the reduction is live in the reference
        O = C.oracle()  # and or_pbs_batch, with the default bound, is the composition without it
        assert np.array_equal(O.pbs_batch(cs.ks.prm, cs.ks.okeys, cs.cts, cs.luts, cs.lut_index), plain)
