"""What the gate circuits (integer.Circuit) and the radix circuits (radix.RadixCircuit) share: stepping operator
coroutines in lockstep, cutting a level into engine calls, and cutting the joined output back into the entries'
shapes.  The arrays are numpy arrays, torch tensors or ``radix.LinBlocks``: all three slice and reshape alike, and
``cat`` joins them."""
import numpy as np


def is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def cat(seq, axis: int = 0):
    seq = list(seq)
    if seq and is_torch(seq[0]):
        import torch
        return torch.cat(seq, dim=axis)
    return np.concatenate(seq, axis=axis)       # LinBlocks answer this themselves


def chunks(n: int, step: int, run):
    """run(o, o + step) for o = 0, step, 2 * step, ... below n, the outputs joined along axis 0.  One level is one
    launch, but levels of wide operators (euint128 mul: ~10^5 to ~10^6 PBS) go in chunks so that host and device
    staging stay bounded.  A single chunk's output is returned as it is, not copied."""
    outs = [run(o, o + step) for o in range(0, n, step)]
    return outs[0] if len(outs) == 1 else cat(outs)


def n_rows(lead) -> int:
    return int(np.prod(lead, dtype=np.int64))


def split(out, leads):
    """The joined output of a level -> per entry (its leading shape, its rows of ``out``)."""
    off = 0
    for lead in leads:
        cnt = n_rows(lead)
        yield lead, out[off:off + cnt]
        off += cnt


def run_many(bootstrap, ops) -> list:
    """Steps the coroutines ``ops`` together: each yields one level (a list of entries) at a time and is sent the
    list of its bootstrapped entries; the levels that the pending coroutines yield at one step go through one
    ``bootstrap`` call, so the set costs max(depth) calls, not sum(depth).  -> their return values, in order."""
    results = [None] * len(ops)
    pending = {}
    for i, g in enumerate(ops):
        try:
            pending[i] = (g, next(g))
        except StopIteration as e:
            results[i] = e.value
    while pending:
        order = list(pending)
        reqs, counts = [], []
        for i in order:
            reqs.extend(pending[i][1])
            counts.append(len(pending[i][1]))
        outs = bootstrap(reqs)
        off = 0
        for i, cnt in zip(order, counts):
            g = pending[i][0]
            try:
                pending[i] = (g, g.send(outs[off:off + cnt]))
            except StopIteration as e:
                results[i] = e.value
                del pending[i]
            off += cnt
    return results
