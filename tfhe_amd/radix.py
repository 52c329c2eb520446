"""Radix integers on the production fhEVM parameters (the representation tfhe-rs /
fhEVM use: PARAM_MESSAGE_2_CARRY_2_KS_PBS, sdk/relayer/src/tfhe.ts:14-19).

A w-bit encrypted integer is w/2 blocks (LSB first); each block is a big LWE (dim 2048) of a value
v in [0, 16) = 2-bit message + 2-bit carry space, encoded v * 2^63 / 16 (one padding bit).  A
"clean" block holds v < 4.  Every programmable bootstrap evaluates a 16-entry table on one block;
two clean blocks x, y combine into one PBS input 4x + y ("bivariate" LUT, tfhe-rs
`apply_bivariate_lookup_table`).  All PBS of one circuit level — across every value, block and
independent operation — run as ONE `Engine.pbs` launch with a per-ciphertext LUT index.

Operators (fhEVM semantics, as tfhe_amd.integer): add/sub/neg with parallel-prefix carry
propagation over block states {0: none, 1: propagate, 2: generate} (log2(blocks) levels),
bitwise and/or/xor (1 level), not (free: 3 - v), eq/ne (per-block equality + AND tree),
lt/le/gt/ge (per-block {<, =, >} + MSB-first merge tree), min/max (compare + 2-PBS select),
shl/shr/rotl/rotr by a plaintext amount (block moves + one bivariate level for odd shifts) or an
encrypted one (barrel shifter over the amount's bits), mul (block products by bivariate low/high
digit tables, carry-save reduction rounds of up to 5 blocks, final prefix add; plaintext factors by
univariate tables), div/rem by a plaintext divisor (multiply-high by a (w+1)-bit reciprocal),
plaintext right operands, mixed widths zero-extended.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .lockstep import chunks, n_rows, run_many, split

MSG = 4                     # message modulus
SPACE = 16                  # message x carry
DELTA = (1 << 63) // SPACE  # one padding bit
FULL_BITS = 5               # padding bit + carry + message: DELTA = 2^(64 - FULL_BITS)
_M64 = 1 << 64


def _table(f: Callable[[int], int]) -> Tuple[int, ...]:
    return tuple(int(f(v)) % SPACE for v in range(SPACE))


def _biv(f: Callable[[int, int], int]) -> Tuple[int, ...]:
    """bivariate table on 4x + y (x, y < 4)."""
    return _table(lambda v: f(v // MSG, v % MSG))


MAX_LAUNCH = 1 << 18  # ciphertexts per engine call (P-FHEVM: 2 x 2049 x 8 B x 256 Ki = 8.6 GB of I/O)


class RadixCircuit:
    """Lockstep executor: each level is a list of (lin array (..., dim+1), table) pairs; every
    distinct table becomes one LUT of the launch and each ciphertext indexes its own.

    A level entry whose second member is a tuple of n_fn tables of SPACE / n_fn entries is a many-LUT
    request (tfhe-rs ``apply_many_lookup_table``): one blind rotation per ciphertext, n_fn results, and the
    caller guarantees every value of ``lin`` is < SPACE / n_fn.  ``many_lut=True`` lets the circuits that
    know such a bound (``g_propagate``) use it; the default keeps every circuit on one table per rotation.
    ``pbs_count`` counts blind rotations, ``launches`` levels.

    ``device`` (a torch device of the engine's one shard, or "cpu") makes the circuit resident: every block array
    is a ``LinBlocks`` (host-side terms over buffers that stay where they are), the linear work between two levels
    is never executed on its own, and ``bootstrap`` turns a level into one term description that
    ``Engine.lincomb_pbs_device`` assembles and bootstraps on torch's current stream; the outputs are new device
    buffers and nothing synchronises before ``RadixUint.decrypt`` / ``to_host``.  ``device="cpu"`` is the same
    executor over numpy buffers: it assembles with ``lincomb_ref`` and calls the overridable ``_pbs`` /
    ``_pbs_many`` / ``_oprf``.  Both give the bits of the default host mode (the maps are exact mod 2^64).
    ``max_terms`` records the most terms any assembled row had.

    All three modes run one level routine, ``_level`` (``oprf`` has the same shape): join the entries' rows, then
    chunk by chunk  rows -> ``_assemble`` -> ``_run_pbs`` / ``_run_pbs_many`` / ``_run_oprf`` -> ``_wrapped``, and cut
    the joined output back into the entries' shapes (``tfhe_amd.lockstep``, shared with ``integer.Circuit``).  The
    constructor binds those steps, ``_const`` (``trivial``) and ``_from_host`` (``_ingest``) once; nothing else asks
    which mode the circuit is in.  Host mode's steps are identities around the seams, on plain uint64 arrays."""

    def __init__(self, engine, many_lut: bool = False, device=None):
        self.engine = engine
        self.many_lut = bool(many_lut)
        p = engine.params
        self.dim = p.k * p.N + 1 if p.order == 1 else p.n + 1
        self.N = p.N
        self._luts: Dict[Tuple[int, ...], np.ndarray] = {}
        self.pbs_count = 0
        self.launches = 0
        self.lazy = device is not None
        self.device = None
        self.max_terms = 0
        # The mode is chosen here and nowhere else.  Every chunk of a level (and of an oprf call) takes one way,
        #   rows -> _assemble -> _run_pbs / _run_pbs_many / _run_oprf -> _wrapped,
        # and what enters a circuit comes from _const (trivial) or _from_host (_ingest).
        self._run_pbs, self._run_pbs_many, self._run_oprf = self._pbs, self._pbs_many, self._oprf
        if not self.lazy:
            # host: block arrays are plain uint64 arrays, and the seams take a level's rows as they are
            self._const, self._from_host, self._assemble, self._wrapped = self._host_const, _same, _same, _same
            return
        self._const = lambda bodies: LinBlocks.const(bodies, self.dim, self._lincomb)
        self._from_host = lambda host: self.wrap(self._buffer(np.ascontiguousarray(host, dtype=np.uint64)))
        if str(device) == "cpu":
            # resident over numpy buffers: lincomb_ref assembles a chunk's rows, then the same seams
            self._lincomb, self._buffer = lincomb_ref, _same
            self._assemble = lambda chunk: lincomb_ref(*self._terms(chunk), self.dim)
            self._wrapped = lambda out: LinBlocks.wrap(np.ascontiguousarray(out, dtype=np.uint64), lincomb_ref)
            return
        # resident in HBM: a chunk stays a term description, and the engine assembles and bootstraps it
        import torch
        if len(getattr(engine, "devices", (0,))) > 1:
            raise ValueError("a device-resident RadixCircuit takes an engine with one shard")
        self.device = torch.device(device)
        self._d_cache: Dict = {}
        self._lincomb = engine.lincomb_device
        self._buffer = lambda host: self._upload(host.view(np.int64))
        self._assemble = self._terms
        self._wrapped = lambda out: LinBlocks.wrap(out, self._lincomb)
        self._run_pbs, self._run_pbs_many, self._run_oprf = self._pbs_device, self._pbs_many_device, self._oprf_device

    def _host_const(self, bodies: np.ndarray) -> np.ndarray:
        out = np.zeros(bodies.shape + (self.dim,), dtype=np.uint64)
        out[..., -1] = bodies
        return out

    def _terms(self, chunk: "LinBlocks"):
        """The term description of a chunk's rows (``LinBlocks.terms``); ``max_terms`` keeps the widest row."""
        desc = chunk.terms()
        self.max_terms = max(self.max_terms, int(np.diff(desc[1]).max(initial=0)))
        return desc

    def wrap(self, buf) -> "LinBlocks":
        """A (..., dim) buffer of ciphertext words (an int64 torch tensor on the circuit's device; a uint64 numpy
        array for device="cpu") as a block array of this circuit.  The buffer is referenced, not copied."""
        if not self.lazy:
            raise ValueError("wrap: the circuit is not resident (RadixCircuit(engine, device=...))")
        if isinstance(buf, np.ndarray) != (self.device is None):
            raise TypeError("wrap: a numpy array for device=\"cpu\", a torch tensor on the device otherwise")
        if tuple(buf.shape[-1:]) != (self.dim,):
            raise ValueError(f"wrap: rows of {self.dim} words expected, got shape {tuple(buf.shape)}")
        return LinBlocks.wrap(buf, self._lincomb)

    def _ingest(self, host: np.ndarray):
        """Host ciphertexts (..., dim) as a block array of this circuit: one upload in device mode."""
        return self._from_host(host)

    # ---- a torch device: uploads, cached LUT stacks, and the level calls that take a term description ----------
    def _upload(self, host: np.ndarray):
        """numpy -> a tensor on the circuit's device through pinned memory, queued on the current stream."""
        import torch
        return torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)

    def _d_luts(self, key, build):
        """Device copy of a level's LUT stack, cached by its tables."""
        if key not in self._d_cache:
            self._d_cache[key] = self._upload(np.ascontiguousarray(build()).view(np.int64))
        return self._d_cache[key]

    def _pbs_device(self, desc, tables, idx):
        """``_pbs`` in HBM: the rows of the term description ``desc`` assembled and bootstrapped in one call."""
        d_luts = self._d_luts(tuple(tables), lambda: np.stack([self.lut(t) for t in tables]))
        return self.engine.lincomb_pbs_device(*desc, d_luts, self._upload(idx.view(np.int32)))

    def _pbs_many_device(self, desc, table_groups, idx, n_fn: int):
        """``_pbs_many`` in HBM: the assembly is its own launch here (``lincomb_device``), then ``pbs_many_device``."""
        d_luts = self._d_luts(tuple(table_groups), lambda: np.stack([self.many_lut_of(g) for g in table_groups]))
        lin = self.engine.lincomb_device(*desc, self.dim)
        return self.engine.pbs_many_device(lin, d_luts, n_fn, self.N // n_fn, self._upload(idx.view(np.int32)))

    def _oprf_device(self, seeds, bit_kinds, idx):
        """``_oprf`` in HBM: the seeds go up (16 bytes a row), the blocks stay on the device."""
        tabs = [self.oprf_lut(b) for b in bit_kinds]
        d_luts = self._d_luts(("oprf",) + tuple(bit_kinds), lambda: np.stack([t[0] for t in tabs]))
        d_post = self._d_luts(("oprf post",) + tuple(bit_kinds),
                              lambda: np.array([int(t[1]) % _M64 for t in tabs], dtype=np.uint64))
        return self.engine.oprf_device(self._upload(seeds.view(np.int64)), d_luts, d_post, self._upload(idx.view(np.int32)))

    # ---- the seams: how a level reaches the engine in host and device="cpu" mode (tests override them) ----------
    def _pbs(self, flat, tables, idx):
        """(cnt, dim) -> (cnt, dim): ciphertext q through tables[idx[q]]."""
        luts = np.stack([self.lut(t) for t in tables])
        return self.engine.pbs(flat, luts, idx)

    def _pbs_many(self, flat, table_groups, idx, n_fn: int):
        """(cnt, dim) -> (cnt, n_fn, dim): ciphertext q through the many-LUT of table_groups[idx[q]]."""
        luts = np.stack([self.many_lut_of(g) for g in table_groups])
        return self.engine.pbs_many(flat, luts, n_fn, self.N // n_fn, idx)

    def _oprf(self, seeds, bit_kinds, idx):
        """(cnt, 2) -> (cnt, dim): row q gets ``bit_kinds[idx[q]]`` random bits."""
        tabs = [self.oprf_lut(b) for b in bit_kinds]
        return self.engine.oprf(seeds, np.stack([t[0] for t in tabs]), [t[1] for t in tabs], idx)

    def lut(self, table: Tuple[int, ...]) -> np.ndarray:
        if table not in self._luts:
            from . import lut_from_table
            self._luts[table] = lut_from_table(self.N, SPACE, list(table), DELTA)
        return self._luts[table]

    def many_lut_of(self, group: Tuple[Tuple[int, ...], ...]) -> np.ndarray:
        if group not in self._luts:
            from . import lut_many
            self._luts[group] = lut_many(self.N, SPACE, [list(t) for t in group], DELTA)[0]
        return self._luts[group]

    def oprf_lut(self, random_bits: int):
        """(lut, post_add) of ``random_bits`` uniform bits in a block of this encoding (``lut_oprf``), cached."""
        key = ("oprf", int(random_bits))
        if key not in self._luts:
            from . import lut_oprf
            self._luts[key] = lut_oprf(self.N, int(random_bits), FULL_BITS)
        return self._luts[key]

    # encodings
    def trivial(self, vals) -> np.ndarray:
        v = np.asarray(vals, dtype=np.uint64)
        return self._const((v % np.uint64(SPACE)) * np.uint64(DELTA))

    # ---- levels ---------------------------------------------------------------------------------------------------
    def bootstrap(self, reqs: Sequence[Tuple[np.ndarray, Tuple[int, ...]]]) -> list:
        """One level: the ordinary entries first, then the many-LUT entries grouped by ascending n_fn, each group
        one ``_level``; the results in request order."""
        if not reqs:
            return []
        kinds = [len(t) if isinstance(t[0], tuple) else 0 for _, t in reqs]
        if not any(kinds):
            res = self._level(reqs)
        else:
            res = [None] * len(reqs)
            for n_fn in sorted(set(kinds)):
                grp = [i for i, k in enumerate(kinds) if k == n_fn]
                for i, r in zip(grp, self._level([reqs[i] for i in grp], n_fn or None)):
                    res[i] = r
        self.launches += 1
        return res

    def _level(self, reqs, n_fn: Optional[int] = None) -> list:
        """The entries of one level that take ``n_fn`` tables each (None: ordinary entries, one table each): every
        distinct table (group) becomes one LUT and each row indexes its own, the rows go through ``_pbs`` in chunks
        of MAX_LAUNCH (``_pbs_many`` in chunks of MAX_LAUNCH outputs), and every entry gets its leading shape back:
        an array, or for a many-LUT entry a tuple of n_fn arrays."""
        tables, index, idx_parts, flat_parts = [], {}, [], []
        for a, t in reqs:
            if n_fn and any(len(f) * n_fn != SPACE for f in t):
                raise ValueError(f"a many-LUT entry of {n_fn} tables takes tables of {SPACE // n_fn} entries")
            if t not in index:
                index[t] = len(tables)
                tables.append(t)
            cnt = n_rows(a.shape[:-1])
            flat_parts.append(a.reshape(cnt, self.dim))
            idx_parts.append(np.full(cnt, index[t], dtype=np.uint32))
        flat = np.concatenate(flat_parts, axis=0)
        idx = np.concatenate(idx_parts)
        if n_fn:
            step, run = max(1, MAX_LAUNCH // n_fn), lambda lin, i: self._run_pbs_many(lin, tables, i, n_fn)
        else:
            step, run = MAX_LAUNCH, lambda lin, i: self._run_pbs(lin, tables, i)
        out = chunks(flat.shape[0], step, lambda o, e: self._wrapped(run(self._assemble(flat[o:e]), idx[o:e])))
        self.pbs_count += flat.shape[0]
        parts = split(out, [a.shape[:-1] for a, _ in reqs])
        if n_fn:
            return [tuple(part[:, f].reshape(s + (self.dim,)) for f in range(n_fn)) for s, part in parts]
        return [part.reshape(s + (self.dim,)) for s, part in parts]

    def oprf(self, row_seeds, random_bits) -> np.ndarray:
        """Oblivious pseudo-random blocks (tfhe-rs ``generate_oblivious_pseudo_random*``): (R, 2) row seeds -> (R, dim)
        clean blocks of ``random_bits`` uniform bits each (one number, or one per row).  One ``Engine.oprf`` launch
        (in chunks of MAX_LAUNCH rows): the masks come from the seeds on the device, one blind rotation per row."""
        seeds = np.ascontiguousarray(np.asarray(row_seeds, dtype=np.uint64)).reshape(-1, 2)
        rb = np.broadcast_to(np.asarray(random_bits, dtype=np.int64), (seeds.shape[0],))
        if seeds.shape[0] == 0:
            return self.trivial(np.zeros((0,), dtype=np.uint64))
        kinds = sorted({int(b) for b in rb})
        idx = np.searchsorted(np.array(kinds), rb).astype(np.uint32)
        out = chunks(seeds.shape[0], MAX_LAUNCH, lambda o, e: self._wrapped(self._run_oprf(seeds[o:e], kinds, idx[o:e])))
        self.pbs_count += seeds.shape[0]
        self.launches += 1
        return out

    def run(self, op):
        return self.run_many([op])[0]

    def run_many(self, ops) -> list:
        return run_many(self.bootstrap, ops)


def _same(x):
    return x


# --------------------------------------------------------------------------------------------
# linear operations on block arrays (mod 2^64, any leading shape)
# --------------------------------------------------------------------------------------------
def lincomb_ref(bufs, row_start, term_buf, term_row, term_coef, bias, dim: int) -> np.ndarray:
    """The numpy statement of the lincomb map (tfhe_amd/csrc/lincomb.hip; ``Engine.lincomb*`` take the same
    arguments), all arithmetic mod 2^64:

        out[r] = sum over t in row_start[r] .. row_start[r + 1] - 1 of term_coef[t] * bufs[term_buf[t]][term_row[t]]
        out[r][dim - 1] += bias[r]            (bias may be None)

    ``bufs``: arrays of (rows_b, dim) words; a row without terms is a trivial ciphertext.  -> (rows, dim) uint64."""
    rs = np.asarray(row_start, dtype=np.int64)
    rows = rs.shape[0] - 1
    T = int(rs[-1]) if rows >= 0 else 0
    out = np.zeros((max(rows, 0), dim), dtype=np.uint64)
    if T:
        tb = np.asarray(term_buf, dtype=np.int64)[:T]
        tr = np.asarray(term_row, dtype=np.int64)[:T]
        src = np.empty((T, dim), dtype=np.uint64)
        for b in np.unique(tb):
            sel = tb == b
            src[sel] = np.asarray(bufs[b], dtype=np.uint64).reshape(-1, dim)[tr[sel]]
        src *= np.asarray(term_coef, dtype=np.uint64)[:T, None]
        counts = np.diff(rs)
        for k in range(int(counts.max())):  # term k of every row that has one
            sel = np.nonzero(counts > k)[0]
            out[sel] += src[rs[sel] + k]
    if bias is not None and rows > 0:
        out[:, -1] += np.asarray(bias, dtype=np.uint64)
    return out


_BUF_IDS = __import__("itertools").count()


class LinBlocks:
    """A lazy block array of a resident ``RadixCircuit``: host-side metadata only.  Element e of the leading shape
    stands for the ciphertext  sum over its terms of coef * (row ``row`` of buffer ``buf``)  + bias[e] on the body,
    mod 2^64.  The terms of an element are slots along the last axis of ``buf`` / ``row`` / ``coef`` (``buf`` < 0:
    empty slot); ``bufs`` maps the ids the array names to the buffers themselves (torch tensors on the device, or
    numpy arrays), which keeps them alive.  ``shape`` is leading + (dim,), as of the eager array it replaces, and
    the array supports what the circuits do to block arrays: basic and strided slicing and ``None`` on leading axes
    (a full slice on the last), ``copy``, ``reshape`` of the leading axes, item assignment of another LinBlocks,
    ``np.concatenate`` / ``np.stack`` / ``np.roll`` / ``np.broadcast_to`` along leading axes, and the linear
    helpers ``_add`` / ``_scale`` / ``_sub`` / ``_not``.  None of these touches ciphertext words: ``materialize``
    does, in one call of ``apply`` (``Engine.lincomb_device`` or ``lincomb_ref``)."""

    def __init__(self, buf, row, coef, bias, bufs, dim, apply):
        # bufs may name more buffers than the terms still use (a slice keeps its parent's): every bootstrap output
        # starts from its one buffer again, so the surplus lives no longer than the linear work between two levels
        self.buf, self.row, self.coef, self.bias, self.bufs, self.dim, self.apply = buf, row, coef, bias, bufs, int(dim), apply

    @classmethod
    def wrap(cls, buffer, apply) -> "LinBlocks":
        """Every row of a (..., dim) buffer as one term of coefficient 1."""
        if isinstance(buffer, LinBlocks) or buffer.ndim < 1:
            raise TypeError("LinBlocks.wrap takes a (..., dim) buffer of ciphertext words")
        lead, dim = tuple(buffer.shape[:-1]), int(buffer.shape[-1])
        if isinstance(buffer, np.ndarray):
            buffer = np.ascontiguousarray(buffer, dtype=np.uint64)
        elif not buffer.is_contiguous():
            buffer = buffer.contiguous()
        i = next(_BUF_IDS)
        n = int(np.prod(lead, dtype=np.int64))
        return cls(np.full(lead + (1,), i, dtype=np.int64), np.arange(n, dtype=np.int64).reshape(lead + (1,)),
                   np.ones(lead + (1,), dtype=np.uint64), np.zeros(lead, dtype=np.uint64), {i: buffer.reshape(n, dim)},
                   dim, apply)

    @classmethod
    def const(cls, bodies, dim, apply) -> "LinBlocks":
        """Trivial ciphertexts: no terms, body ``bodies``."""
        b = np.array(bodies, dtype=np.uint64)
        z = b.shape + (0,)
        return cls(np.zeros(z, dtype=np.int64), np.zeros(z, dtype=np.int64), np.zeros(z, dtype=np.uint64), b, {}, dim, apply)

    # ---- shape ------------------------------------------------------------------------------------------------
    @property
    def shape(self):
        return self.bias.shape + (self.dim,)

    @property
    def ndim(self):
        return self.bias.ndim + 1

    def __len__(self):
        return self.shape[0]

    def _like(self, buf, row, coef, bias, bufs=None) -> "LinBlocks":
        return LinBlocks(buf, row, coef, bias, self.bufs if bufs is None else bufs, self.dim, self.apply)

    def _lead_key(self, key):
        """An index of the block array -> the index of its leading axes (the last axis takes a full slice only)."""
        key = key if isinstance(key, tuple) else (key,)
        if any(k is Ellipsis for k in key):
            i = next(j for j, k in enumerate(key) if k is Ellipsis)
            fill = self.ndim - sum(k is not None and k is not Ellipsis for k in key)
            key = key[:i] + (slice(None),) * fill + key[i + 1:]
        if not all(k is None or isinstance(k, (int, np.integer, slice)) for k in key):
            raise IndexError("LinBlocks: basic indexing only (integers, slices, None)")
        if sum(k is not None for k in key) == self.ndim:
            if key[-1] != slice(None):
                raise IndexError("LinBlocks: the last axis (ciphertext words) takes a full slice only")
            key = key[:-1]
        return key

    def __getitem__(self, key) -> "LinBlocks":
        key = self._lead_key(key)
        kk = key + (slice(None),)
        return self._like(self.buf[kk], self.row[kk], self.coef[kk], self.bias[key])

    def _slots(self, K: int):
        """(buf, row, coef) padded with empty slots to K terms per element."""
        pad = K - self.buf.shape[-1]
        if pad == 0:
            return self.buf, self.row, self.coef
        tail = self.bias.shape + (pad,)
        return (np.concatenate([self.buf, np.full(tail, -1, dtype=np.int64)], axis=-1),
                np.concatenate([self.row, np.zeros(tail, dtype=np.int64)], axis=-1),
                np.concatenate([self.coef, np.zeros(tail, dtype=np.uint64)], axis=-1))

    def __setitem__(self, key, value: "LinBlocks") -> None:
        if not isinstance(value, LinBlocks):
            raise TypeError("LinBlocks: only another LinBlocks can be assigned")
        key = self._lead_key(key)
        K = max(self.buf.shape[-1], value.buf.shape[-1])
        kk = key + (slice(None),)
        mine, theirs = self._slots(K), value._slots(K)
        for dst, src in zip(mine, theirs):
            dst[kk] = src
        self.bias[key] = value.bias
        self.buf, self.row, self.coef = mine
        self.bufs = {**self.bufs, **value.bufs}

    def copy(self) -> "LinBlocks":
        return self._like(self.buf.copy(), self.row.copy(), self.coef.copy(), self.bias.copy())

    def reshape(self, *shape) -> "LinBlocks":
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else tuple(shape)
        if not shape or shape[-1] not in (-1, self.dim):
            raise ValueError(f"LinBlocks.reshape: the last axis stays {self.dim} words")
        bias = self.bias.reshape(shape[:-1])
        K = (self.buf.shape[-1],)
        return self._like(self.buf.reshape(bias.shape + K), self.row.reshape(bias.shape + K),
                          self.coef.reshape(bias.shape + K), bias)

    # ---- numpy functions along leading axes ---------------------------------------------------------------------
    def _lead_axis(self, axis, ndim=None) -> int:
        ndim = self.ndim if ndim is None else ndim
        a = int(axis) % ndim
        if a == ndim - 1:
            raise ValueError("LinBlocks: the last axis (ciphertext words) cannot be moved or joined")
        return a

    @staticmethod
    def _joined(fn, arrs, axis) -> "LinBlocks":
        arrs = list(arrs)
        if not arrs or not all(isinstance(a, LinBlocks) for a in arrs):
            raise TypeError("LinBlocks joins with LinBlocks only")
        K = max(a.buf.shape[-1] for a in arrs)
        slots = [a._slots(K) for a in arrs]
        bufs = {}
        for a in arrs:
            bufs.update(a.bufs)
        return arrs[0]._like(*[fn([s[i] for s in slots], axis=axis) for i in range(3)],
                             fn([a.bias for a in arrs], axis=axis), bufs)

    def __array_function__(self, func, types, args, kwargs):
        if func is np.concatenate:
            arrs = args[0]
            axis = args[1] if len(args) > 1 else kwargs.get("axis", 0)
            return LinBlocks._joined(np.concatenate, arrs, arrs[0]._lead_axis(axis))
        if func is np.stack:
            arrs = args[0]
            axis = args[1] if len(args) > 1 else kwargs.get("axis", 0)
            return LinBlocks._joined(np.stack, arrs, arrs[0]._lead_axis(axis, arrs[0].ndim + 1))
        if func is np.roll:
            a, shift = args[0], args[1] if len(args) > 1 else kwargs["shift"]
            axis = args[2] if len(args) > 2 else kwargs.get("axis")
            if axis is None:
                raise ValueError("LinBlocks: np.roll needs a leading axis")
            ax = a._lead_axis(axis)
            return a._like(np.roll(a.buf, shift, ax), np.roll(a.row, shift, ax), np.roll(a.coef, shift, ax),
                           np.roll(a.bias, shift, ax))
        if func is np.broadcast_to:
            a, shape = args[0], tuple(args[1] if len(args) > 1 else kwargs["shape"])
            if not shape or shape[-1] != a.dim:
                raise ValueError(f"LinBlocks: broadcast keeps the last axis at {a.dim} words")
            K = (a.buf.shape[-1],)
            return a._like(np.broadcast_to(a.buf, shape[:-1] + K), np.broadcast_to(a.row, shape[:-1] + K),
                           np.broadcast_to(a.coef, shape[:-1] + K), np.broadcast_to(a.bias, shape[:-1]))
        return NotImplemented

    # ---- linear maps -------------------------------------------------------------------------------------------
    def scaled(self, k: int) -> "LinBlocks":
        k = np.uint64(int(k) % _M64)
        with np.errstate(over="ignore"):
            return self._like(self.buf, self.row, self.coef * k, np.asarray(self.bias * k, dtype=np.uint64))

    @staticmethod
    def sum(xs) -> "LinBlocks":
        """Elementwise sum (leading shapes broadcast): the operands' terms side by side, empty slots squeezed out."""
        xs = list(xs)
        lead = xs[0].bias.shape
        if any(x.bias.shape != lead for x in xs):
            lead = np.broadcast_shapes(*[x.bias.shape for x in xs])
            xs = [x if x.bias.shape == lead else np.broadcast_to(x, lead + (x.dim,)) for x in xs]
        buf, row, coef = [np.concatenate([getattr(x, f) for x in xs], axis=-1) for f in ("buf", "row", "coef")]
        bias = np.zeros(lead, dtype=np.uint64)
        bufs = {}
        for x in xs:
            with np.errstate(over="ignore"):
                bias = np.asarray(bias + x.bias, dtype=np.uint64)
            bufs.update(x.bufs)
        valid = buf >= 0
        if not valid.all():
            order = np.argsort(~valid, axis=-1, kind="stable")
            K = int(valid.sum(axis=-1).max(initial=0))
            buf, row, coef = [np.take_along_axis(a, order, axis=-1)[..., :K] for a in (buf, row, coef)]
        return xs[0]._like(buf, row, coef, bias, bufs)

    # ---- ciphertext words ----------------------------------------------------------------------------------------
    def terms(self):
        """The term description of the flattened array, the arguments of ``lincomb_ref`` / ``Engine.lincomb*``:
        (bufs, row_start, term_buf, term_row, term_coef, bias), one output row per element in C order."""
        flat = (self.bias.size, self.buf.shape[-1])
        buf = self.buf.reshape(flat)
        valid = buf >= 0
        row_start = np.zeros(flat[0] + 1, dtype=np.uint32)
        row_start[1:] = np.cumsum(valid.sum(axis=1))
        ids, term_buf = np.unique(buf[valid], return_inverse=True)
        return ([self.bufs[int(i)] for i in ids], row_start, term_buf.astype(np.uint32).reshape(-1),
                self.row.reshape(flat)[valid].astype(np.uint32), np.ascontiguousarray(self.coef.reshape(flat)[valid]),
                np.ascontiguousarray(self.bias.reshape(-1)))

    def materialize(self):
        """The array's ciphertext words as one (leading..., dim) buffer where the buffers live: one ``apply`` call,
        or no work at all for an untouched run of rows of one buffer."""
        lead = self.bias.shape
        bufs, row_start, term_buf, term_row, term_coef, bias = desc = self.terms()
        n = row_start.shape[0] - 1
        if (len(bufs) == 1 and term_row.shape[0] == n and self.buf.shape[-1] == 1 and n and not bias.any()
                and np.all(term_coef == 1) and np.array_equal(term_row, term_row[0] + np.arange(n, dtype=np.uint32))):
            return bufs[0][int(term_row[0]):int(term_row[0]) + n].reshape(lead + (self.dim,))
        return self.apply(*desc, self.dim).reshape(lead + (self.dim,))

    def to_host(self) -> np.ndarray:
        """Materialised and downloaded: the eager uint64 array this one stands for."""
        m = self.materialize()
        if isinstance(m, np.ndarray):
            return m
        return m.cpu().numpy().view(np.uint64)

    def __array__(self, dtype=None, copy=None):
        h = self.to_host()
        return h if dtype is None else h.astype(dtype, copy=False)


def _host(blocks) -> np.ndarray:
    return blocks.to_host() if isinstance(blocks, LinBlocks) else blocks


def _add(*xs):
    if isinstance(xs[0], LinBlocks):
        return LinBlocks.sum(xs)
    with np.errstate(over="ignore"):
        out = xs[0].copy()
        for x in xs[1:]:
            out += x
    return out


def _scale(x, k: int):
    if isinstance(x, LinBlocks):
        return x.scaled(k)
    with np.errstate(over="ignore"):
        return (x * np.uint64(k % _M64)).astype(np.uint64)


def _sub(x, y):
    if isinstance(x, LinBlocks):
        return LinBlocks.sum([x, y.scaled(-1)])
    with np.errstate(over="ignore"):
        return (x - y).astype(np.uint64)


def _const(c: "RadixCircuit", shape, v: int):
    return c.trivial(np.full(shape, v, dtype=np.uint64))


def _pack(x, y):
    """4x + y for clean blocks (the bivariate PBS input)."""
    return _add(_scale(x, MSG), y)


def _not(c, a):
    """3 - a for clean blocks (bitwise NOT of the 2-bit message), no PBS."""
    return _sub(_const(c, a.shape[:-1], MSG - 1), a)


class RadixUint:
    """A batch of B encrypted w-bit integers: blocks (B, w/2, dim), LSB block first, all clean."""

    def __init__(self, c: RadixCircuit, blocks: np.ndarray):
        self.c, self.blocks = c, blocks

    @property
    def width(self) -> int:
        return 2 * self.blocks.shape[1]

    @property
    def batch(self) -> int:
        return self.blocks.shape[0]

    @staticmethod
    def _digits(values, w):
        """(B, w/2) base-4 digits, least significant first; values are ints of any size."""
        if w <= 64:
            v = np.atleast_1d(np.asarray(values, dtype=np.uint64))
            return (v[:, None] >> (2 * np.arange(w // 2, dtype=np.uint64))[None, :]) & np.uint64(3)
        vs = [int(x) for x in np.atleast_1d(np.asarray(values, dtype=object))]
        return np.array([[(x >> (2 * j)) & 3 for j in range(w // 2)] for x in vs], dtype=np.uint64).reshape(len(vs), w // 2)

    @classmethod
    def encrypt(cls, c: RadixCircuit, ck, values, w: int, seed: Optional[int] = None, stream0: int = 0) -> "RadixUint":
        d = cls._digits(values, w)
        ct = ck.encrypt(d.reshape(-1), SPACE, seed, stream0).reshape(d.shape + (-1,))
        return cls(c, c._ingest(ct))

    @classmethod
    def trivial(cls, c: RadixCircuit, values, w: int) -> "RadixUint":
        return cls(c, c.trivial(cls._digits(values, w)))

    def tensor(self):
        """The blocks as one (B, w/2, dim) buffer where the circuit keeps them: for a resident circuit the
        materialised device tensor (int64, queued on torch's current stream, not synchronised; a numpy array for
        device="cpu"), otherwise the host array itself."""
        return self.blocks.materialize() if isinstance(self.blocks, LinBlocks) else self.blocks

    def to_host(self) -> np.ndarray:
        """The blocks as a host (B, w/2, dim) uint64 array (a resident circuit materialises and downloads)."""
        return _host(self.blocks)

    def decrypt(self, ck) -> np.ndarray:
        B, nb = self.blocks.shape[:2]
        d = ck.decrypt(self.to_host().reshape(B * nb, -1), SPACE).reshape(B, nb).astype(object)
        w = self.width
        vals = [sum(int(d[i, j]) << (2 * j) for j in range(nb)) % (1 << w) for i in range(B)]
        return np.array(vals, dtype=np.uint64 if w <= 64 else object)

    def cast(self, w: int) -> "RadixUint":
        nb = w // 2
        if nb == self.blocks.shape[1]:
            return self
        if nb < self.blocks.shape[1]:
            return RadixUint(self.c, self.blocks[:, :nb])
        pad = _const(self.c, (self.batch, nb - self.blocks.shape[1]), 0)
        return RadixUint(self.c, np.concatenate([self.blocks, pad], axis=1))

    @classmethod
    def rand(cls, c: RadixCircuit, seeds, w: int) -> "RadixUint":
        """fhEVM ``rand``: one uniform w-bit value per (lo, hi) seed of ``seeds`` (``g_rand``)."""
        return c.run(g_rand(c, seeds, w))

    @classmethod
    def rand_bounded(cls, c: RadixCircuit, seeds, w: int, bound: int) -> "RadixUint":
        """fhEVM ``randBounded``: uniform in [0, bound), bound a power of two <= 2^w (``g_rand_bounded``)."""
        return c.run(g_rand_bounded(c, seeds, w, bound))


# --------------------------------------------------------------------------------------------
# circuits (coroutines yielding levels of (lin, table))
# --------------------------------------------------------------------------------------------
T_MSG = _table(lambda v: v % MSG)
T_STATE = _table(lambda v: 2 if v >= MSG else (1 if v == MSG - 1 else 0))   # of a block sum <= 7
T_MERGE = _biv(lambda hi, lo: lo if hi == 1 else hi)                       # prefix op on states
T_APPLY = _biv(lambda st, m: (m + (1 if st == 2 else 0)) % MSG)            # carry-in from the prefix
# both tables of a block sum <= 7 from one blind rotation (a 2-function many-LUT: the sum leaves the top bit free)
T_MSG_STATE = (T_MSG[:SPACE // 2], T_STATE[:SPACE // 2])


def g_propagate(c: RadixCircuit, s: np.ndarray, carry_in: bool):
    """Carry propagation of block sums s (B, nb, dim) with values <= 7: clean result blocks."""
    B, nb = s.shape[:2]
    if carry_in:
        s = s.copy()
        s[:, 0] = _add(s[:, 0], _const(c, (B,), 1))
    if not c.many_lut:
        msg, st = yield [(s, T_MSG), (s, T_STATE)]
    elif not carry_in:
        ((msg, st),) = yield [(s, T_MSG_STATE)]
    elif nb == 1:
        msg, st = yield [(s, T_MSG), (s, T_STATE)]
    else:
        # block 0 holds up to 8 with the carry-in: all 16 values, so it stays on one table per rotation
        (msg_hi, st_hi), msg0, st0 = yield [(s[:, 1:], T_MSG_STATE), (s[:, :1], T_MSG), (s[:, :1], T_STATE)]
        msg = np.concatenate([msg0, msg_hi], axis=1)
        st = np.concatenate([st0, st_hi], axis=1)
    # Kogge-Stone over block states: prefix[j] = state of blocks 0..j
    d = 1
    while d < nb:
        (merged,) = yield [(_pack(st[:, d:], st[:, :-d]), T_MERGE)]
        st = np.concatenate([st[:, :d], merged], axis=1)
        d *= 2
    if nb == 1:
        return msg
    (hi,) = yield [(_pack(st[:, :-1], msg[:, 1:]), T_APPLY)]
    return np.concatenate([msg[:, :1], hi], axis=1)


def g_add(c, a, b, carry_in=False):
    return (yield from g_propagate(c, _add(a, b), carry_in))


def g_sub(c, a, b):
    return (yield from g_propagate(c, _add(a, _not(c, b)), True))


T_AND = _biv(lambda x, y: x & y)
T_OR = _biv(lambda x, y: x | y)
T_XOR = _biv(lambda x, y: x ^ y)
T_EQ = _biv(lambda x, y: int(x == y))
T_AND1 = _biv(lambda x, y: x & y & 1)
T_CMP = _biv(lambda x, y: 0 if x < y else (1 if x == y else 2))           # {<, =, >}
T_SEL_T = _biv(lambda cond, x: x if cond == 1 else 0)
T_SEL_F = _biv(lambda cond, x: 0 if cond == 1 else x)


def g_bitwise(c, kind, a, b):
    t = {"and": T_AND, "or": T_OR, "xor": T_XOR}[kind]
    (r,) = yield [(_pack(a, b), t)]
    return r


def g_eq(c, a, b):
    """encrypted bool block (B, dim), value 0/1."""
    (e,) = yield [(_pack(a, b), T_EQ)]
    while e.shape[1] > 1:
        if e.shape[1] % 2:
            e = np.concatenate([e, _const(c, (e.shape[0], 1), 1)], axis=1)
        (e,) = yield [(_pack(e[:, 0::2], e[:, 1::2]), T_AND1)]
    return e[:, 0]


def g_cmp(c, a, b):
    """comparison state of a vs b per value: block (B, dim) with 0 (<), 1 (=), 2 (>)."""
    (st,) = yield [(_pack(a, b), T_CMP)]
    # merge MSB-first: result = hi if hi != '=' else lo  (blocks are LSB first: hi = odd index)
    while st.shape[1] > 1:
        if st.shape[1] % 2:
            st = np.concatenate([st, _const(c, (st.shape[0], 1), 1)], axis=1)
        (st,) = yield [(_pack(st[:, 1::2], st[:, 0::2]), T_MERGE_CMP)]
    return st[:, 0]


T_MERGE_CMP = _biv(lambda hi, lo: lo if hi == 1 else hi)
T_IS = {"lt": _table(lambda v: int(v == 0)), "le": _table(lambda v: int(v <= 1)),
        "gt": _table(lambda v: int(v == 2)), "ge": _table(lambda v: int(v >= 1))}


def g_compare(c, kind, a, b):
    st = yield from g_cmp(c, a, b)
    (r,) = yield [(st, T_IS[kind])]
    return r


def g_select(c, cond, x, y):
    """cond (B, dim) in {0,1} ? x : y, blockwise: two bivariate PBS per block, then one message
    PBS of their sum, so the result is a fresh block again (noise level 1; a bivariate input 4x + y
    has level 5 = max_noise_level of the parameter set, so levels never stack)."""
    cw = np.broadcast_to(cond[:, None, :], x.shape)
    t, f = yield [(_pack(cw, x), T_SEL_T), (_pack(cw, y), T_SEL_F)]
    (r,) = yield [(_add(t, f), T_MSG)]
    return r


def g_minmax(c, kind, a, b):
    st = yield from g_cmp(c, a, b)
    (take_a,) = yield [(st, T_IS["lt"] if kind == "min" else T_IS["gt"])]
    return (yield from g_select(c, take_a, a, b))


T_SHL_LO = _biv(lambda cur, prev: ((cur << 1) | (prev >> 1)) & 3)   # one-bit left shift across blocks
T_SHR_LO = _biv(lambda nxt, cur: ((cur >> 1) | (nxt << 1)) & 3)     # one-bit right shift


def g_shift(c, a, k: int, kind: str):
    B, nb = a.shape[:2]
    w = 2 * nb
    k %= w
    q, r = divmod(k, 2)
    zero = _const(c, (B, q), 0)
    rot = kind in ("rotl", "rotr")
    if kind in ("shl", "rotl"):
        moved = np.roll(a, q, axis=1) if rot else np.concatenate([zero, a[:, :nb - q]], axis=1)
        if not r:
            return moved
        prev = np.roll(moved, 1, axis=1) if rot else np.concatenate([_const(c, (B, 1), 0), moved[:, :-1]], axis=1)
        (out,) = yield [(_pack(moved, prev), T_SHL_LO)]
        return out
    moved = np.roll(a, -q, axis=1) if rot else np.concatenate([a[:, q:], zero], axis=1)
    if not r:
        return moved
    nxt = np.roll(moved, -1, axis=1) if rot else np.concatenate([moved[:, 1:], _const(c, (B, 1), 0)], axis=1)
    (out,) = yield [(_pack(nxt, moved), T_SHR_LO)]
    return out


T_MUL_LO = _biv(lambda x, y: (x * y) % MSG)
T_MUL_HI = _biv(lambda x, y: (x * y) // MSG)
T_CARRY = _table(lambda v: v // MSG)


def g_sum_columns(c, cols: List[List[np.ndarray]], B: int):
    """Sum per-position lists of clean blocks (position k has weight 4^k, positions >= nb dropped)
    into one clean radix value: carry-save rounds add up to 5 blocks (<= 15, the block capacity) and
    split each sum into message (stays) and carry (moves up) in one PBS level, until every position
    holds at most two blocks; then one carry-propagating add."""
    nb = len(cols)
    while max(len(col) for col in cols) > 2:
        reqs, plan = [], []
        new_cols: List[List[np.ndarray]] = [[] for _ in range(nb)]
        for k, col in enumerate(cols):
            if len(col) <= 2:
                new_cols[k].extend(col)
                continue
            for g in range(0, len(col), 5):
                grp = col[g:g + 5]
                if len(grp) == 1:
                    new_cols[k].append(grp[0])
                    continue
                ssum = _add(*grp)
                reqs += [(ssum, T_MSG), (ssum, T_CARRY)]
                plan.append(k)
        outs = yield reqs
        for t, k in enumerate(plan):
            new_cols[k].append(outs[2 * t])
            if k + 1 < nb:
                new_cols[k + 1].append(outs[2 * t + 1])
        cols = new_cols
    zero = _const(c, (B,), 0)
    a = np.stack([col[0] if len(col) > 0 else zero for col in cols], axis=1)
    b = np.stack([col[1] if len(col) > 1 else zero for col in cols], axis=1)
    return (yield from g_add(c, a, b))


def g_mul(c, a, b):
    """a * b mod 2^w.  b: blocks (B, nb, dim) or a plaintext int.  Block products: two bivariate
    PBS (low / high digit of x*y) per pair i + j < nb (plaintext: univariate per a-block and digit)."""
    B, nb = a.shape[:2]
    reqs, pos = [], []
    if isinstance(b, (int, np.integer)):
        digs = [(int(b) >> (2 * j)) & 3 for j in range(nb)]
        for i in range(nb):
            for j in range(nb - i):
                d = digs[j]
                if d == 0:
                    continue
                reqs.append((a[:, i], _table(lambda v, d=d: (v * d) % MSG)))
                pos.append(i + j)
                if i + j + 1 < nb:
                    reqs.append((a[:, i], _table(lambda v, d=d: (v * d) // MSG)))
                    pos.append(i + j + 1)
    else:
        for i in range(nb):
            for j in range(nb - i):
                packed = _pack(a[:, i], b[:, j])
                reqs.append((packed, T_MUL_LO))
                pos.append(i + j)
                if i + j + 1 < nb:
                    reqs.append((packed, T_MUL_HI))
                    pos.append(i + j + 1)
    cols: List[List[np.ndarray]] = [[] for _ in range(nb)]
    if reqs:
        outs = yield reqs
        for o, k in zip(outs, pos):
            cols[k].append(o)
    return (yield from g_sum_columns(c, cols, B))


T_BIT = {k: _table(lambda v, k=k: (v >> k) & 1) for k in (0, 1)}


def g_shift_enc(c, a, amount, kind: str):
    """Shift / rotate by an encrypted amount (mod w): barrel shifter, one select per amount bit."""
    B, nb = a.shape[:2]
    w = 2 * nb
    nbits = max(1, (w - 1).bit_length())
    reqs = [(amount[:, k // 2], T_BIT[k % 2]) for k in range(nbits)]
    bits = yield reqs
    cur = a
    for k in range(nbits):
        moved = yield from g_shift(c, cur, 1 << k, kind)
        cur = yield from g_select(c, bits[k], moved, cur)
    return cur


T_LOW_BIT = _table(lambda v: v & 1)


def g_div_rem_scalar(c, a, d: int):
    """(a // d, a % d) for a plaintext divisor by multiply-high: with l = ceil(log2 d) and
    m = ceil(2^(w+l) / d) (w + 1 bits), floor(a * m / 2^(w+l)) = floor(a / d) for every a < 2^w
    (m*d - 2^(w+l) < d, so the error term a*(m*d - 2^(w+l)) / d < 2^(w+l) never crosses an integer).
    One constant multiply at width 2w + 2, a block shift, one constant multiply and one subtract.
    d = 0 follows tfhe-rs / fhEVM: quotient all ones, remainder = numerator.  Powers of two are a
    block shift and a mask."""
    B, nb = a.shape[:2]
    w = 2 * nb
    d = int(d) % (1 << w)
    if d == 0:
        return _const(c, (B, nb), MSG - 1), a
    if d & (d - 1) == 0:
        s = d.bit_length() - 1
        q = (yield from g_shift(c, a, s, "shr")) if s else a
        keep = s // 2
        parts = [a[:, :keep]]
        if s % 2:
            (lowbit,) = yield [(a[:, keep], T_LOW_BIT)]
            parts.append(lowbit[:, None])
        done = keep + s % 2
        parts.append(_const(c, (B, nb - done), 0))
        return q, np.concatenate(parts, axis=1)
    l = (d - 1).bit_length()
    m = -(-(1 << (w + l)) // d)
    nbw = w + 1                                             # width 2w + 2 holds a * m < 2^(2w+1)
    a_ext = np.concatenate([a, _const(c, (B, nbw - nb), 0)], axis=1)
    prod = yield from g_mul(c, a_ext, m)
    k = w + l
    sub = prod[:, k // 2:k // 2 + nb + 1]
    if sub.shape[1] < nb + 1:
        sub = np.concatenate([sub, _const(c, (B, nb + 1 - sub.shape[1]), 0)], axis=1)
    q = (yield from g_shift(c, sub, k % 2, "shr"))[:, :nb] if k % 2 else sub[:, :nb]
    qd = yield from g_mul(c, q, d)
    r = yield from g_sub(c, a, qd)
    return q, r


def _request_seeds(seeds) -> np.ndarray:
    """One (lo, hi) seed, or a (B, 2) array of them -> (B, 2) uint64."""
    s = np.asarray([[int(v) % _M64 for v in row] for row in np.asarray(seeds, dtype=object).reshape(-1, 2)],
                   dtype=np.uint64)
    return s.reshape(-1, 2)


def _rand_bits(bound) -> int:
    b = int(bound)
    if b < 2 or b & (b - 1):
        raise ValueError(f"randBounded: the bound must be a power of two >= 2 (fhEVM), got {bound}")
    return b.bit_length() - 1


def g_rand_bounded(c: RadixCircuit, seeds, w: int, bound: int):
    """fhEVM ``randBounded``: per request seed one value uniform in [0, bound), bound = 2^t with 1 <= t <= w.  The
    value is t // 2 two-bit blocks, a one-bit block if t is odd, then trivial zeros up to w / 2 blocks.  Request b
    draws the row seeds of its random blocks, in block order, from its seed (``oprf_block_seeds``: words (2j, 2j + 1)
    of the seed's stream).  No level of the lockstep executor: the blocks are one ``RadixCircuit.oprf`` launch."""
    from . import oprf_block_seeds
    yield from ()
    t = _rand_bits(bound)
    if w < 2 or w % 2:
        raise ValueError(f"radix rand: width {w} is not a positive multiple of the 2-bit block (ebool: g_rand_bool)")
    if t > w:
        raise ValueError(f"randBounded: bound 2^{t} exceeds the type's 2^{w}")
    parents = _request_seeds(seeds)
    B, nb, nr = parents.shape[0], w // 2, (t + 1) // 2
    bits = np.array([2] * (t // 2) + [1] * (t % 2), dtype=np.int64)
    rows = np.concatenate([oprf_block_seeds(s, nr) for s in parents], axis=0)
    rnd = c.oprf(rows, np.tile(bits, B)).reshape(B, nr, c.dim)
    if nr == nb:
        return RadixUint(c, rnd)
    return RadixUint(c, np.concatenate([rnd, _const(c, (B, nb - nr), 0)], axis=1))


def g_rand(c: RadixCircuit, seeds, w: int):
    """fhEVM ``rand``: per request seed one uniform w-bit value (every block random)."""
    return (yield from g_rand_bounded(c, seeds, w, 1 << w))


def g_rand_bool(c: RadixCircuit, seeds):
    """fhEVM ``rand`` on ebool: an encrypted bool block (B, dim) holding a uniform 0 / 1, from block seed 0 of each
    request seed."""
    from . import oprf_block_seeds
    yield from ()
    rows = np.concatenate([oprf_block_seeds(s, 1) for s in _request_seeds(seeds)], axis=0)
    return c.oprf(rows, 1)


RADIX_RAND_OPS = ("rand", "randBounded")


def fhevm_rand(c: RadixCircuit, op: str, seeds, w: int, bound=None):
    """The two random fhEVM operators (coroutine, as ``fhevm_op``): ``rand`` gives a RadixUint of width w, or for
    w == 1 (ebool) an encrypted bool block; ``randBounded`` takes a power-of-two ``bound``."""
    if op not in RADIX_RAND_OPS:
        raise ValueError(f"radix random operator {op!r} not supported")
    if op == "rand":
        if bound is not None:
            raise ValueError("rand takes no bound (randBounded does)")
        if w == 1:
            return (yield from g_rand_bool(c, seeds))
        return (yield from g_rand(c, seeds, w))
    if bound is None:
        raise ValueError("randBounded needs a bound")
    return (yield from g_rand_bounded(c, seeds, w, bound))


RADIX_OPS = ("add", "sub", "mul", "div", "rem", "and", "or", "xor", "eq", "ne", "lt", "le", "gt", "ge", "min", "max",
             "neg", "not", "shl", "shr", "rotl", "rotr")


def fhevm_op(c: RadixCircuit, op: str, lhs, rhs=None):
    """One fhEVM operator on radix integers (coroutine).  Comparisons return an encrypted bool block
    (B, dim) holding 0/1; other operators a RadixUint."""
    if op not in RADIX_OPS:
        raise ValueError(f"radix operator {op!r} not supported")
    if op == "not":
        return RadixUint(c, _not(c, lhs.blocks))
    if op == "neg":
        z = _const(c, lhs.blocks.shape[:-1], 0)
        return RadixUint(c, (yield from g_sub(c, z, lhs.blocks)))
    lenc, renc = isinstance(lhs, RadixUint), isinstance(rhs, RadixUint)
    if not (lenc or renc):
        raise ValueError("at least one operand must be encrypted")
    if op in ("shl", "shr", "rotl", "rotr"):
        if not lenc:
            raise ValueError("shift of a plaintext by an encrypted amount is not an fhEVM overload")
        if renc:
            return RadixUint(c, (yield from g_shift_enc(c, lhs.blocks, rhs.blocks, op)))
        return RadixUint(c, (yield from g_shift(c, lhs.blocks, int(rhs), op)))
    w = max(x.width for x in (lhs, rhs) if isinstance(x, RadixUint))
    B = (lhs if lenc else rhs).batch

    def blocks(x):
        if isinstance(x, RadixUint):
            return x.cast(w).blocks
        return c.trivial(np.broadcast_to(RadixUint._digits([int(x) % (1 << w)], w), (B, w // 2)))

    if op in ("div", "rem"):
        if not lenc or renc:
            raise ValueError("fhEVM div / rem take an encrypted numerator and a plaintext divisor")
        q, r = yield from g_div_rem_scalar(c, lhs.blocks, int(rhs))
        return RadixUint(c, q if op == "div" else r)
    if op == "mul":
        if not lenc:
            return RadixUint(c, (yield from g_mul(c, rhs.cast(w).blocks, int(lhs) % (1 << w))))
        if not renc:
            return RadixUint(c, (yield from g_mul(c, lhs.cast(w).blocks, int(rhs) % (1 << w))))
        return RadixUint(c, (yield from g_mul(c, blocks(lhs), blocks(rhs))))
    a, b = blocks(lhs), blocks(rhs)
    if op == "add":
        return RadixUint(c, (yield from g_add(c, a, b)))
    if op == "sub":
        return RadixUint(c, (yield from g_sub(c, a, b)))
    if op in ("and", "or", "xor"):
        return RadixUint(c, (yield from g_bitwise(c, op, a, b)))
    if op in ("eq", "ne"):
        e = yield from g_eq(c, a, b)
        if op == "eq":
            return e
        return _sub(_const(c, e.shape[:-1], 1), e)
    if op in ("lt", "le", "gt", "ge"):
        return (yield from g_compare(c, op, a, b))
    return RadixUint(c, (yield from g_minmax(c, op, a, b)))
