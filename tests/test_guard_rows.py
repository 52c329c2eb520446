"""The guard-row checker of tests/guard_rows.py on numpy arrays: it stands in for a mutation test of
tests/test_gpu_device_buffers.py, which never runs a kernel that is broken on purpose.  A write is planted where a
kernel with a missing row or column guard would put one, and the checker has to name it."""
import numpy as np
import pytest

import guard_rows as G

ROWS, ROW_LEN = 5, 17   # an odd row length, as n + 1 = 17 and kN + 1 = 1025 are


def fresh(front=2, back=2):
    return G.guarded(ROWS, ROW_LEN, front, back, device=None)


def test_layout_and_alignment():
    whole, view = fresh()
    assert whole.shape == (2 + ROWS + 2, ROW_LEN) and whole.dtype == np.int64
    assert view.shape == (ROWS, ROW_LEN) and view.flags["C_CONTIGUOUS"] and np.shares_memory(view, whole)
    assert (view.ctypes.data - whole.ctypes.data) == 2 * ROW_LEN * 8 and (2 * ROW_LEN * 8) % 16 == 0
    assert (whole == G.SENTINEL).all()
    for front, back in ((1, 2), (2, 3), (-2, 2)):
        with pytest.raises(ValueError):
            G.guarded(ROWS, ROW_LEN, front, back, device=None)


def test_untouched_buffer_passes():
    whole, view = fresh()
    G.assert_guards(whole, ROWS, "untouched")
    view[:] = np.arange(ROWS * ROW_LEN, dtype=np.int64).reshape(ROWS, ROW_LEN)   # any payload, both edges included
    view[0, 0] = view[-1, -1] = 0
    G.assert_guards(whole, ROWS, "payload written")
    assert G.guard_damage(whole, ROWS) == []
    wide, _ = fresh(4, 6)
    G.assert_guards(wide, ROWS, "other guard counts", front=4)


# (name, flat index into the whole buffer, guard row, side, word, what the message says about the distance)
PLANTED = [
    ("the first guard word", 0, 0, "front", 0, "2 before the first payload row"),
    ("the last guard word", (2 + ROWS + 2) * ROW_LEN - 1, 2 + ROWS + 1, "back", ROW_LEN - 1, "2 past the last payload row"),
    ("the word just past the last payload row", (2 + ROWS) * ROW_LEN, 2 + ROWS, "back", 0, "1 past the last payload row"),
    ("the word just before the first payload row", 2 * ROW_LEN - 1, 1, "front", ROW_LEN - 1, "1 before the first payload row"),
]


@pytest.mark.parametrize("name,flat,row,side,word,distance", PLANTED, ids=[p[0] for p in PLANTED])
def test_a_planted_write_is_reported(name, flat, row, side, word, distance):
    whole, view = fresh()
    view[:] = 7
    whole.reshape(-1)[flat] = 0                    # what a stray store leaves: any word but the sentinel
    damage = G.guard_damage(whole, ROWS)
    assert [(r, s, b.tolist()) for r, s, b in damage] == [(row, side, [word])]
    with pytest.raises(AssertionError) as e:
        G.assert_guards(whole, ROWS, f"planted: {name}")
    msg = str(e.value)
    assert f"planted: {name}" in msg and "1 guard words written" in msg
    assert f"{side} guard row {row} ({distance})" in msg and f"words [{word}]" in msg and "1 of 17 words" in msg


def test_a_whole_stray_row_is_counted():
    """A missing b < B guard writes a whole row B: every word of the first back guard row, none of the second."""
    whole, _ = fresh()
    whole[2 + ROWS] = np.arange(ROW_LEN)
    whole[2 + ROWS, 3] = G.SENTINEL               # one word happens to store the sentinel: 16 of 17 are seen
    with pytest.raises(AssertionError) as e:
        G.assert_guards(whole, ROWS, "row B")
    assert "16 guard words written" in str(e.value) and "16 of 17 words" in str(e.value) and "..." in str(e.value)
    assert f"back guard row {2 + ROWS + 1}" not in str(e.value)


def test_a_wrong_row_count_is_refused():
    whole, _ = fresh()
    with pytest.raises(ValueError):
        G.assert_guards(whole, ROWS + 3, "too many rows")


def test_embedded_holds_the_rows_between_seeded_neighbours():
    rows = np.arange(ROWS * ROW_LEN, dtype=np.uint64).reshape(ROWS, ROW_LEN) << np.uint64(40)
    w1, v1 = G.embedded(rows, fill_seed=1, device=None)
    w2, v2 = G.embedded(rows, fill_seed=2, device=None)
    again, _ = G.embedded(rows, fill_seed=1, device=None)
    assert w1.shape == (2 + ROWS + 2, ROW_LEN) and w1.dtype == np.int64 and v1.flags["C_CONTIGUOUS"]
    assert np.array_equal(v1.view(np.uint64), rows) and np.array_equal(v2.view(np.uint64), rows)
    assert np.array_equal(w1, again)
    for r in (0, 1, 2 + ROWS, 2 + ROWS + 1):        # every neighbour row differs between the two seeds
        assert not np.array_equal(w1[r], w2[r])
    assert (v1.ctypes.data - w1.ctypes.data) % 16 == 0
    with pytest.raises(ValueError):
        G.embedded(rows, front=1, device=None)
