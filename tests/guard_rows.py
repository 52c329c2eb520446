"""Guard rows around the buffers of the device-buffer (``*_async``) entry points.  A plain module, no fixtures.

A host-buffer call cannot show a stray write: the library stages the output itself and copies back exactly the rows
asked for.  A device-buffer call writes into the caller's tensor, so a test can put memory around it: ``guarded``
hands out the middle rows of one sentinel-filled tensor and ``assert_guards`` checks afterwards that the rows in front
and behind still hold the sentinel; ``embedded`` does the same for an input, with random neighbours.

Guards are whole rows in an even count: the view's base then keeps the 16-byte alignment of a fresh allocation's
first row even when ``row_len`` is odd (17, 1025, 2049), the condition every buffer of a resident circuit meets.

Every function works the same on numpy arrays (``device=None``): tests/test_guard_rows.py plants writes there and
shows that the checker reports them.
"""
import numpy as np

SENTINEL = 0x5EA71E555EA71E55      # fits int64; a stray write goes unseen only if it stores exactly this word
DEVICE = "cuda:0"


def _check_counts(front, back):
    if front < 0 or back < 0 or front % 2 or back % 2:
        raise ValueError(f"guards are whole rows in an even count, not {front} and {back}")


def guarded(rows, row_len, front=2, back=2, device=DEVICE):
    """-> (whole, view): one sentinel-filled int64 tensor of front + rows + back rows of row_len words on ``device``
    (a numpy array for device=None) and its middle ``rows`` rows, contiguous and sharing its memory."""
    _check_counts(front, back)
    shape = (front + int(rows) + back, int(row_len))
    if device is None:
        whole = np.full(shape, SENTINEL, dtype=np.int64)
    else:
        import torch
        whole = torch.full(shape, SENTINEL, dtype=torch.int64, device=device)
    view = whole[front:front + int(rows)]
    if int(rows) > 0:  # an empty torch view reports no address
        assert _base(view) - _base(whole) == front * int(row_len) * 8 and (_base(view) - _base(whole)) % 16 == 0
    return whole, view


def _base(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def guard_damage(whole, rows, front=2):
    """-> [(guard row of ``whole``, "front" or "back", the written word indices)] of every guard row that no longer
    holds the sentinel in every word; [] for an untouched buffer."""
    w = _host(whole)
    total = w.shape[0]
    if w.ndim != 2 or front < 0 or front + rows > total:
        raise ValueError(f"{front} + {rows} rows do not fit a buffer of shape {w.shape}")
    out = []
    for r in list(range(front)) + list(range(front + rows, total)):
        bad = np.nonzero(w[r] != np.int64(SENTINEL))[0]
        if bad.size:
            out.append((r, "front" if r < front else "back", bad))
    return out


def assert_guards(whole, rows, what, front=2):
    """Every word of the front and back guard rows of ``whole`` (``front`` rows, ``rows`` payload rows, the rest
    behind) still holds the sentinel; otherwise an AssertionError that names each guard row written, its distance
    from the payload, the first words and how many."""
    damage = guard_damage(whole, rows, front)
    if not damage:
        return
    lines = []
    for r, side, bad in damage:
        where = f"{front - r} before the first payload row" if side == "front" else f"{r - front - rows + 1} past the last payload row"
        lines.append(f"{side} guard row {r} ({where}): {bad.size} of {_host(whole).shape[1]} words written, "
                     f"words {bad[:8].tolist()}{' ...' if bad.size > 8 else ''}")
    total = sum(bad.size for _, _, bad in damage)
    raise AssertionError(f"{what}: {total} guard words written outside the {rows} payload rows\n  " + "\n  ".join(lines))


def embedded(array, front=2, back=2, fill_seed=0, device=DEVICE):
    """-> (whole, view): the rows of ``array`` (2-D uint64) uploaded as the middle of a tensor of front + rows + back
    rows whose other rows hold random words from ``fill_seed``; ``view`` is those middle rows, contiguous.  An entry
    point that reads past its B input rows, or in front of them, computes something else for another seed."""
    _check_counts(front, back)
    a = np.ascontiguousarray(array, dtype=np.uint64)
    if a.ndim != 2:
        raise ValueError("embedded: a 2-D array of rows")
    rng = np.random.default_rng(fill_seed)
    host = rng.integers(0, 2 ** 64, size=(front + a.shape[0] + back, a.shape[1]), dtype=np.uint64)
    host[front:front + a.shape[0]] = a
    host = host.view(np.int64)
    if device is None:
        whole = host
    else:
        import torch
        whole = torch.from_numpy(host).to(device)
    view = whole[front:front + a.shape[0]]
    if a.shape[0] > 0:
        assert (_base(view) - _base(whole)) % 16 == 0
    return whole, view
