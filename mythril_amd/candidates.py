"""Candidate-model generator: candidates BEYOND the 100-entry LRU.

The reference tries only the models z3 returned earlier (``ModelCache``, support_utils.py:56-67,
filled at model.py:125), at most 100 of them, so every path the cached models miss costs a z3
``Optimize.check`` (model.py:104-130).  A fork (svm.py:351-358) usually differs from a path the
cache already satisfies in one or a few branch conditions — a selector, ``require(x == c)``,
``x < c`` — so mutating a cached model's inputs towards the constants those conditions compare
against often yields a satisfying assignment without a solver call.  That is what this module
generates, for the GPU to evaluate in bulk (M up to 10^5 per launch):

* **directed** candidates: for a conjunction, each cached model with ALL the conjunct's
  invertible branch conditions patched to a satisfying value (polarity from ``Not``);
* **single mutations**: one condition patched to ``c``, ``c - 1`` or ``c + 1``;
* **boundary** values of single variables (0, 1, 2^w - 1, 2^(w-1), 2^(w-1) - 1) and
  **random fills**.

A branch condition is *invertible* when it compares a constant with an expression that maps
bits of model inputs one to one: variables, calldata bytes at constant offsets (derived
variables), ``Extract``, ``Concat``, ``ZeroExt`` and the calldata-byte shape ``If(i < size,
byte, 0)`` (calldata.py:234-246).  Patching a derived variable (the interpretation of
``<tx>_calldata`` at a constant index) also adds that entry to the candidate's table, so every
candidate is a consistent model: evaluating it is exactly ``model.eval(expr, model_completion=
True)`` of the model :meth:`CandidateSet.materialize` returns.  With ``keccak_sites`` (opt-in) a
patch that changes the input of a ``keccak256_<n>`` application also enters the new input's image
in that function's table and its inverse's (:class:`KeccakSites`), so the keccak manager's axioms
hold on the candidate and forks over a mapping key can be answered.

Generated candidates sit strictly AFTER the LRU models in global candidate order (index >= the
LRU size), so an LRU hit is never pre-empted and the reference's first-hit / bump semantics are
untouched.  They are only used behind ``Args.quick_sat_candidates`` and only for verdict
callers (``Constraints.is_possible``), never for callers that read model contents
(arbitrary_jump.py:29-32, instructions.py:1742-1746).
"""
from __future__ import annotations

import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .models import ModelBatch
from .smt_model import Model, as_record
from .tape import NONE, Op, Tape, limbs, to_words

_EQ, _ULT, _ULE, _SLT, _SLE = 20, 21, 22, 23, 24
_PREDS = (_EQ, _ULT, _ULE, _SLT, _SLE)

# a bit map: tuple of segments from the low bit up: (var, var_lo_bit, n_bits) or (-1, const, n_bits);
# a floor (var, minimum) says a mapped calldata byte is only read when that size variable exceeds
# its offset (If(i < size, byte, 0), calldata.py:234-246).  A patch is a tuple of assignments
# (var, lo, n_bits, bits), floors written as (var, -1, 0, minimum).
Segment = Tuple[int, int, int]


class _BitMaps:
    """Which DAG nodes are one-to-one maps of model-input bits (memoised per node)."""

    def __init__(self, nodes: np.ndarray, consts: np.ndarray, opaque=frozenset()):
        self.opaque = opaque   # variables that are not free model inputs (never patched)
        self.op = nodes["op"].astype(np.int64)
        self.w = nodes["width"].astype(np.int64)
        self.a = nodes["a"].astype(np.int64)
        self.b = nodes["b"].astype(np.int64)
        self.c = nodes["c"].astype(np.int64)
        self.consts = consts
        self.memo: Dict[int, Optional[Tuple[Segment, ...]]] = {}
        self.cvals: Dict[int, int] = {}
        self.floors: Dict[int, Tuple[Tuple[int, int], ...]] = {}

    def const_value(self, n: int) -> Optional[int]:
        if self.op[n] != 1:
            return None
        v = self.cvals.get(n)
        if v is not None:
            return v
        nl = limbs(int(self.w[n]))
        off = int(self.a[n])
        v = 0
        for i in range(nl):
            v |= int(self.consts[off + i]) << (32 * i)
        v &= (1 << int(self.w[n])) - 1
        self.cvals[n] = v
        return v

    def map(self, n: int) -> Optional[Tuple[Segment, ...]]:
        if n in self.memo:
            return self.memo[n]
        op, w = int(self.op[n]), int(self.w[n])
        r: Optional[Tuple[Segment, ...]] = None
        fl: Tuple[Tuple[int, int], ...] = ()
        if op == 2 and w > 0 and int(self.a[n]) not in self.opaque:   # VAR
            r = ((int(self.a[n]), 0, w),)
        elif op == 1:                                          # CONST
            r = ((-1, self.const_value(n), w),)
        elif op == 50:                                         # EXTRACT(x, hi, lo)
            x = self.map(int(self.a[n]))
            if x is not None:
                r, fl = _slice(x, int(self.c[n]), w), self.floors[int(self.a[n])]
        elif op == 51:                                         # CONCAT(hi, lo)
            hi, lo = self.map(int(self.a[n])), self.map(int(self.b[n]))
            if hi is not None and lo is not None:
                r = lo + hi
                fl = self.floors[int(self.a[n])] + self.floors[int(self.b[n])]
        elif op == 52:                                         # ZEXT(x, k)
            x = self.map(int(self.a[n]))
            if x is not None:
                r, fl = x + ((-1, 0, w - int(self.w[int(self.a[n])])),), self.floors[int(self.a[n])]
        elif op == 54:                                         # ITE(c, x, 0): calldata byte shape
            x = self.map(int(self.b[n]))
            e = self.const_value(int(self.c[n]))
            if x is not None and e == 0:
                r = x
                fl = self.floors[int(self.b[n])]
                c = int(self.a[n])                              # i < size (signed, calldata.py:243)
                if int(self.op[c]) in (_SLT, _ULT) and int(self.op[int(self.b[c])]) == 2:
                    i = self.const_value(int(self.a[c]))
                    if i is not None and i < (1 << 31):
                        fl = fl + ((int(self.a[int(self.b[c])]), i + 1),)
        self.memo[n] = r
        self.floors[n] = tuple(sorted(set(fl)))
        return r


def _slice(segs: Tuple[Segment, ...], lo: int, n: int) -> Tuple[Segment, ...]:
    out, pos = [], 0
    for v, s, k in segs:
        a, b = max(lo, pos), min(lo + n, pos + k)
        if a < b:
            if v < 0:
                out.append((-1, (s >> (a - pos)) & ((1 << (b - a)) - 1), b - a))
            else:
                out.append((v, s + a - pos, b - a))
        pos += k
    return tuple(out)


def _patch_for(segs: Tuple[Segment, ...], value: int) -> Optional[Tuple[Tuple[int, int, int, int], ...]]:
    """Variable bit assignments (var, lo, n_bits, bits) that make the mapped expression equal
    ``value``; None if a constant segment disagrees."""
    out, pos = [], 0
    for v, s, k in segs:
        bits = (value >> pos) & ((1 << k) - 1)
        if v < 0:
            if bits != s:
                return None
        else:
            out.append((v, s, k, bits))
        pos += k
    return tuple(out)


def _wanted(op: int, const_left: bool, c: int, w: int, positive: Optional[bool]) -> List[int]:
    """Values of the mapped side that satisfy (positive) / falsify (negative) the predicate."""
    m = (1 << w) - 1
    if positive is None:
        return sorted({c, (c - 1) & m, (c + 1) & m})
    if op == _EQ:
        return [c] if positive else [(c + 1) & m, (c - 1) & m]
    strict = op in (_ULT, _SLT)
    # X < c / X <= c  (const on the right) or c < X / c <= X (const on the left)
    if not const_left:
        lo_side = (c - 1) & m if strict else c
        return [lo_side, 0] if positive else [c if strict else (c + 1) & m]
    hi_side = (c + 1) & m if strict else c
    return [hi_side, m >> (1 if op in (_SLT, _SLE) else 0)] if positive else [c if strict else (c - 1) & m]


def _candidate_rows(lru: ModelBatch, src: np.ndarray, starts: np.ndarray, sizes: np.ndarray,
                    blocks: List[Tuple[Tuple, np.ndarray]], syms, off: np.ndarray, K: int) -> np.ndarray:
    """The whole batch's variable rows [rows, n_lru + K]: the LRU's, then each generated
    candidate's base LRU row with its block's patch applied — value assignments in patch order
    (the last assignment of a bit wins), then the size floors.  The host extension's loop
    (csrc/lowerwalk.cpp candidate_rows, writing the candidates' columns in place); the numpy form
    below where it is not built (the tests compare the two)."""
    from .lower import _walker
    n_lru = lru.n_models
    walker = _walker()
    if walker is not None and n_lru and K and os.environ.get("MQ_PY_CANDIDATES") != "1":
        words = np.empty((int(off[-1]), n_lru + K), np.uint32)
        words[:, :n_lru] = lru.var_words
        gen = words[:, n_lru:]
        widths = syms.var_widths
        walker.candidate_rows(gen, np.ascontiguousarray(lru.var_words, np.uint32), np.ascontiguousarray(src, np.int64),
                              np.ascontiguousarray(starts, np.int64), [p for p, _ in blocks],
                              np.ascontiguousarray(off[:-1], np.int64),
                              np.asarray([limbs(w) for w in widths], np.int64))
        return words
    gen = lru.var_words[:, src].copy() if n_lru else np.zeros((int(off[-1]), K), np.uint32)
    # each block's patch over its candidate range.  Per (limb row, block) the composed update
    # (mask, bits) of the block's value assignments, in patch order (the last assignment of a
    # bit wins); the limb updates of a patch element are computed once (elements recur in many
    # blocks: the random mixes reuse the directed singles).  Then ONE vectorised update per
    # row over every block that patches it, and the size floors (applied after the values of
    # their block) per variable
    widths = syms.var_widths
    cache: Dict[Tuple, List[Tuple[int, int, int]]] = {}
    row_ops: Dict[int, Dict[int, List[int]]] = {}
    floor_ops: Dict[int, Dict[int, int]] = {}
    for j, (patch, _) in enumerate(blocks):
        for el in patch:
            v, lo, n, bits = el
            if lo < 0:   # size >= minimum (values < 2^32 in their low limb)
                fj = floor_ops.setdefault(v, {})
                fj[j] = max(fj.get(j, 0), bits)
                continue
            ups = cache.get(el)
            if ups is None:
                ups = []
                o = int(off[v])
                for i in range(lo // 32, (lo + n - 1) // 32 + 1):
                    blo = 32 * i
                    a, b2 = max(lo, blo), min(lo + n, blo + 32)
                    mask = ((1 << (b2 - a)) - 1) << (a - blo)
                    ups.append((o + i, mask, ((bits >> (a - lo)) << (a - blo)) & mask))
                cache[el] = ups
            for row, mask, val in ups:
                d = row_ops.get(row)
                if d is None:
                    d = row_ops[row] = {}
                c = d.get(j)
                if c is None:
                    d[j] = [mask, val]
                else:
                    c[1] = (c[1] & ~mask) | val
                    c[0] |= mask
    nb = int(sizes.max()) if len(sizes) else 0
    ar = np.arange(nb, dtype=np.int64)

    def cols_of(js: np.ndarray):
        """(block columns [k, nb] of the full-size blocks among js, their positions in js, the others)."""
        full = sizes[js] == nb
        return starts[js[full]][:, None] + ar[None, :], np.flatnonzero(full), np.flatnonzero(~full)

    for row, d in row_ops.items():
        js = np.fromiter(d.keys(), np.int64, len(d))
        mv = np.asarray(list(d.values()), np.uint64).astype(np.uint32).reshape(-1, 2)
        keep, val = ~mv[:, 0], mv[:, 1]
        cols, fi, pi = cols_of(js)
        if len(fi):
            gen[row, cols] = (gen[row, cols] & keep[fi][:, None]) | val[fi][:, None]
        for k in pi:   # (a partial block: the budget's last random block)
            sl = slice(int(starts[js[k]]), int(starts[js[k] + 1]))
            gen[row, sl] = (gen[row, sl] & keep[k]) | val[k]
    for v, fj in floor_ops.items():
        r0, nl = int(off[v]), limbs(widths[v])
        js = np.fromiter(fj.keys(), np.int64, len(fj))
        mins = np.fromiter(fj.values(), np.int64, len(fj)).astype(np.uint32)
        cols, fi, pi = cols_of(js)
        groups = [(cols, mins[fi][:, None])] + [(np.arange(int(starts[js[k]]), int(starts[js[k] + 1]))[None, :],
                                                 mins[k:k + 1][:, None]) for k in pi]
        for cc, mn in groups:
            if not cc.size:
                continue
            x = gen[r0, cc]
            small = ~gen[r0 + 1:r0 + nl][:, cc].any(axis=0) if nl > 1 else np.ones(x.shape, bool)
            gen[r0, cc] = np.where(small & (x < mn), mn, x)
    return np.concatenate([lru.var_words, gen], axis=1)


class Derivation:
    """The generated candidates' rows as "the LRU rows, patched" — the arrays of ``mq_derivation``
    (include/mq.h): the device expands them (``Evaluator.upload_models_derived``), so the
    ``[rows, n_lru + K]`` matrix is neither built on the host nor sent over the bus.

    ``base_words`` [rows, n_base]; ``src`` int32[K] (-1: all-zero rows); ``block_start`` /
    ``patch_ptr`` / ``floor_ptr`` int64[n_blocks + 1]; ``patches`` uint32[n, 3] of (row, keep, bits):
    ``w = (w & keep) | bits``, at most one per (block, row); ``floors`` uint32[n, 3] of (row0,
    n_limbs, minimum), applied after the block's patches."""

    def __init__(self, base_words, src, block_start, patch_ptr, patches, floor_ptr, floors):
        self.base_words = np.ascontiguousarray(base_words, np.uint32)
        self.n_base = int(self.base_words.shape[1])
        self.src = np.ascontiguousarray(src, np.int32)
        self.block_start = np.ascontiguousarray(block_start, np.int64)
        self.patch_ptr = np.ascontiguousarray(patch_ptr, np.int64)
        self.patches = np.ascontiguousarray(patches, np.uint32).reshape(-1, 3)
        self.floor_ptr = np.ascontiguousarray(floor_ptr, np.int64)
        self.floors = np.ascontiguousarray(floors, np.uint32).reshape(-1, 3)

    @property
    def n_derived(self) -> int:
        return len(self.src)

    @property
    def n_blocks(self) -> int:
        return len(self.block_start) - 1

    def upload_bytes(self) -> int:
        """Host-to-device bytes of the variable rows' description."""
        return 4 * self.base_words.size + 12 * len(self.patches) + 12 * len(self.floors) + 4 * len(self.src)


def _compose_blocks(blocks: List[Tuple[Tuple, np.ndarray]], off: np.ndarray, syms):
    """Per block: ({limb row: [mask, bits]} of its value assignments composed in patch order — the
    last assignment of a bit wins — and {variable: minimum} of its floors).  The composition the
    numpy form of :func:`_candidate_rows` does in ``row_ops`` / ``floor_ops``."""
    cache: Dict[Tuple, List[Tuple[int, int, int]]] = {}
    out = []
    for patch, _ in blocks:
        rows: Dict[int, List[int]] = {}
        floors: Dict[int, int] = {}
        for el in patch:
            if el[1] < 0:   # size >= minimum (values < 2^32 in their low limb)
                if floors.get(el[0], 0) < el[3]:
                    floors[el[0]] = el[3]
                continue
            ups = cache.get(el)
            if ups is None:
                v, lo, n, bits = el
                ups = []
                o = int(off[v])
                for i in range(lo // 32, (lo + n - 1) // 32 + 1):
                    blo = 32 * i
                    a, b2 = max(lo, blo), min(lo + n, blo + 32)
                    mask = ((1 << (b2 - a)) - 1) << (a - blo)
                    ups.append((o + i, mask, ((bits >> (a - lo)) << (a - blo)) & mask))
                cache[el] = ups
            for row, mask, val in ups:
                c = rows.get(row)
                if c is None:
                    rows[row] = [mask, val]
                else:
                    c[1] = (c[1] & ~mask) | val
                    c[0] |= mask
        out.append((rows, floors))
    return out


def derivation_arrays(lru: ModelBatch, base: np.ndarray, blocks: List[Tuple[Tuple, np.ndarray]], starts: np.ndarray,
                      sizes: np.ndarray, off: np.ndarray, syms, composed=None) -> Derivation:
    """``(blocks, starts, sizes, off, syms)`` as a :class:`Derivation` over the LRU batch ``lru``:
    each block's value assignments composed per limb row into one ``(keep, bits)``, its floors as
    ``(row0, n_limbs, minimum)``.  ``base`` is the LRU index of every candidate (-1: none)."""
    if composed is None:
        composed = _compose_blocks(blocks, off, syms)
    widths = syms.var_widths
    pptr = np.zeros(len(blocks) + 1, np.int64)
    fptr = np.zeros(len(blocks) + 1, np.int64)
    patches: List[Tuple[int, int, int]] = []
    floors: List[Tuple[int, int, int]] = []
    for j, (rows, fl) in enumerate(composed):
        for row in sorted(rows):
            mask, val = rows[row]
            patches.append((row, ~mask & 0xFFFFFFFF, val))
        for v in sorted(fl):
            floors.append((int(off[v]), limbs(widths[v]), fl[v]))
        pptr[j + 1] = len(patches)
        fptr[j + 1] = len(floors)
    src = np.asarray(base, np.int64) if lru.n_models else np.full(len(base), -1, np.int64)
    return Derivation(lru.var_words, src, np.asarray(starts, np.int64), pptr,
                      np.asarray(patches, np.uint64).reshape(-1, 3), fptr, np.asarray(floors, np.uint64).reshape(-1, 3))


class TableDerivation:
    """The generated candidates' function tables as "the LRU's tables, plus a few entries per
    block" — the arrays of ``mq_table_derivation`` (include/mq.h), expanded on the device next to a
    :class:`Derivation` (``Evaluator.upload_models_derived(..., tables=)``), so no table of
    ``n_lru + K`` models is built on the host or sent over the bus.

    ``base``: the LRU batch (its function CSR and else values are read); ``add_ptr``
    int64[n_blocks + 1] into the additions; per addition ``add_func``, ``add_var`` (the entry's
    value is the candidate's own limbs of that variable) and ``add_key_off`` into ``key_words``,
    the constant key words.  A block's additions are listed per function by ascending variable,
    which is their order in the resulting table, in front of the base model's entries."""

    def __init__(self, base: ModelBatch, add_ptr, add_func, add_var, add_key_off, key_words):
        self.base = base
        self.add_ptr = np.ascontiguousarray(add_ptr, np.int64)
        self.add_func = np.ascontiguousarray(add_func, np.int32)
        self.add_var = np.ascontiguousarray(add_var, np.int32)
        self.add_key_off = np.ascontiguousarray(add_key_off, np.int64)
        self.key_words = np.ascontiguousarray(key_words, np.uint32)

    @property
    def n_blocks(self) -> int:
        return len(self.add_ptr) - 1

    def upload_bytes(self) -> int:
        """Host-to-device bytes of the function tables' description."""
        b = self.base
        return (8 * b.entry_ptr.size + 4 * b.entry_words.size + 4 * b.else_words.size + 8 * self.add_ptr.size
                + 16 * len(self.add_func) + 4 * self.key_words.size)


def table_derivation_arrays(lru: ModelBatch, n_blocks: int, per_f, syms) -> TableDerivation:
    """The triples of :func:`_table_triples` as a :class:`TableDerivation` over the LRU batch:
    per block its additions ordered by (function, variable), each derived variable's constant
    arguments once in the key pool."""
    adds = sorted((j, f, v) for f, (tj, _, tv) in per_f.items() for j, v in zip(tj, tv))
    key_off: Dict[int, int] = {}
    keys: List[int] = []
    for _, f, v in adds:
        if v not in key_off:
            key_off[v] = len(keys)
            for aw, av in zip(lru.funcs[f].arg_widths, syms.derived[v][1]):
                keys.extend(to_words(int(av), aw))
    ptr = np.zeros(n_blocks + 1, np.int64)
    if adds:
        ptr[1:] = np.cumsum(np.bincount([j for j, _, _ in adds], minlength=n_blocks))
    return TableDerivation(lru, ptr, [f for _, f, _ in adds], [v for _, _, v in adds],
                           [key_off[v] for _, _, v in adds], np.asarray(keys, np.uint32))


# ---------------------------------------------------------------------------------------------
# Keccak sites (opt-in, CandidateGenerator(keccak_sites=True)): a patch that changes a variable
# feeding keccak256_<n>(x) moves x to an input the base model's tables do not hold, so the
# manager's axiom keccak256_<n>-1(keccak256_<n>(x)) == x (function_managers.py _create_condition)
# fails on the else values.  For such an application the candidate gets x -> v appended to
# keccak256_<n> and v -> x to keccak256_<n>-1 (and its @@lo:hi slice functions), v being the
# digest of x folded into the manager's interval: base + ((keccak256(x) mod 2^b) << 6).
_KECCAK_NAME = re.compile(r"keccak256_(\d+)$")
_UF, _UF_CHUNK, _UF_WIDE, _KECCAK_OP, _OR = (int(o) for o in (Op.UF, Op.UF_CHUNK, Op.UF_WIDE, Op.KECCAK, Op.OR))
_REFS = {int(o): Tape.operand_slots(o) for o in Op}   # which of (a, b, c) are node references, per op
MAX_SITES = 64
MAX_SITE_BITS = 2048
MAX_COLLISIONS = 8


def image_params(lo: int, hi: int) -> Optional[Tuple[int, int]]:
    """``(base, b)`` of the interval ``[lo, hi)``: base = lo rounded up to a multiple of 64, b the
    largest integer <= 192 with base + 64 * 2^b <= hi (None: the interval holds no such image)."""
    base = (lo + 63) & ~63
    q = (hi - base) // 64
    if q < 1:
        return None
    return base, min(192, q.bit_length() - 1)


def keccak_images(xs: Sequence[int], n_bits: int, base: int, b: int) -> List[int]:
    """The image of each ``n_bits``-wide input: base + ((D mod 2^b) << 6), D the keccak256 (Ethereum
    padding) of the input's big-endian bytes read big-endian (mq.h MQ_OP_KECCAK)."""
    from .evaluator import keccak256_host
    digs = keccak256_host([int(x).to_bytes(n_bits // 8, "big") for x in xs])
    m = (1 << b) - 1
    return [base + ((int.from_bytes(d, "big") & m) << 6) for d in digs]


class KeccakSite:
    """One ``keccak256_<n>(x)`` application whose input is a word-aligned map of model variables."""

    def __init__(self, node, func, n_bits, inverses, segs, words, base, b, collisions):
        self.node = node               # the UF node (sites are ordered by it)
        self.func = func               # f
        self.n_bits = n_bits
        self.inverses = inverses       # [(function id, lo, hi)]: f^-1 (0, n) and its slices, bits [lo, hi) of x
        self.segs = segs               # the input's bit map (_BitMaps.map)
        self.words = words             # per 32-bit word of x, low first: (row, 0) or (-1, constant)
        self.base, self.b = base, b    # image_params of the interval in the DAG
        self.collisions = collisions   # [(constant key, derived variable of f at that key, its first row)]
        self.vars = frozenset(v for v, _, _ in segs if v >= 0)


class KeccakSites:
    """The batch's keccak sites and, per block, the 64-bit mask of the sites its patch activates —
    the arrays of ``mq_keccak_derivation`` (include/mq.h); rides on the CandidateSet next to
    Derivation / TableDerivation."""

    def __init__(self, sites: List[KeccakSite], active: np.ndarray, skipped: Dict[str, int]):
        self.sites = sites
        self.active = np.ascontiguousarray(active, np.uint64)
        self.skipped = skipped

    def contributions(self, f: int) -> List[Tuple[int, Optional[Tuple[int, int]]]]:
        """Sites that append an entry to function ``f``, in site order: (site, None) for the site's
        own function, (site, (lo, hi)) for its inverse or a slice of it."""
        out = []
        for i, s in enumerate(self.sites):
            if s.func == f:
                out.append((i, None))
            for g, lo, hi in s.inverses:
                if g == f:
                    out.append((i, (lo, hi)))
        return out

    def site_counts(self, n_funcs: int) -> np.ndarray:
        """int64[n_funcs, n_blocks]: entries the active sites of block j append to function f."""
        cnt = np.zeros((n_funcs, len(self.active)), np.int64)
        for f in range(n_funcs):
            for i, _ in self.contributions(f):
                cnt[f] += ((self.active >> np.uint64(i)) & np.uint64(1)).astype(np.int64)
        return cnt


def _reachable(db) -> np.ndarray:
    """Nodes of the DAG reachable from the batch's roots (ascending)."""
    op, a, b, c = (db.nodes[k] for k in ("op", "a", "b", "c"))
    seen = set()
    stack = [int(r) for r in db.roots[:int(db.root_offsets[-1])]]
    while stack:
        n = stack.pop()
        if n in seen:
            continue
        seen.add(n)
        args = (int(a[n]), int(b[n]), int(c[n]))
        for i in _REFS[int(op[n])]:
            if args[i] != NONE and args[i] not in seen:
                stack.append(args[i])
    return np.asarray(sorted(seen), np.int64)


def find_keccak_sites(db, syms, off: np.ndarray, bm: Optional[_BitMaps] = None):
    """``(sites, skipped)``: the keccak sites of the batch (at most MAX_SITES, by ascending UF node)
    and how many applications were left out, by reason."""
    from .lower import SLICE, split_slice
    if bm is None:
        opaque = frozenset(v for v, (f, _) in syms.derived.items() if SLICE in f)
        bm = _BitMaps(db.nodes, db.consts, opaque)
    op, a, b = bm.op, bm.a, bm.b
    reach = _reachable(db)
    skipped: Dict[str, int] = {}

    def skip(why: str) -> None:
        skipped[why] = skipped.get(why, 0) + 1
    # the intervals: Or(ULT(lo, u), EQ(lo, u)) / ULE(lo, u) and ULT(u, hi), lo and hi constant
    los: Dict[int, int] = {}
    his: Dict[int, int] = {}
    for n in reach:
        n = int(n)
        o = int(op[n])
        if o == _ULT and int(op[int(a[n])]) == _UF:
            hi = bm.const_value(int(b[n]))
            if hi is not None:
                u = int(a[n])
                his[u] = min(his.get(u, hi), hi)
        elif o == _ULE and int(op[int(b[n])]) == _UF:
            lo = bm.const_value(int(a[n]))
            if lo is not None:
                u = int(b[n])
                los[u] = max(los.get(u, lo), lo)
        elif o == _OR:
            p, q = int(a[n]), int(b[n])
            if int(op[p]) == _EQ:
                p, q = q, p
            if int(op[p]) == _ULT and int(op[q]) == _EQ and int(op[int(b[p])]) == _UF:
                u, cn = int(b[p]), int(a[p])
                lo = bm.const_value(cn)
                if lo is not None and {int(a[q]), int(b[q])} == {u, cn}:
                    los[u] = max(los.get(u, lo), lo)
    derived_of: Dict[str, List[int]] = {}
    for v, (fn, _) in syms.derived.items():
        derived_of.setdefault(fn, []).append(v)
    sites: List[KeccakSite] = []
    for n in reach:
        n = int(n)
        o = int(op[n])
        if o == _KECCAK_OP:
            skip("interpreted")
            continue
        if o == _UF_WIDE and _KECCAK_NAME.match(syms.func_names[int(a[n])]):
            skip("wide")
            continue
        if o != _UF or int(bm.c[n]) != NONE:
            continue
        f = int(a[n])
        name = syms.func_names[f]
        mt = _KECCAK_NAME.match(name)
        if mt is None:
            continue
        nb = int(mt.group(1))
        if nb % 32 or nb > MAX_SITE_BITS or nb != int(bm.w[int(b[n])]) or int(bm.w[n]) != 256:
            skip("wide" if nb > MAX_SITE_BITS else "misaligned")
            continue
        inv = syms.funcs.get(name + "-1")
        if inv is None:
            skip("no_inverse")
            continue
        x = int(b[n])
        segs = bm.map(x)
        if segs is None:
            under = _reachable(_OneRoot(db, x))
            nested = any(int(op[int(m)]) in (_UF, _UF_CHUNK, _UF_WIDE, _KECCAK_OP) for m in under)
            skip("nested" if nested else "unmapped")
            continue
        if bm.floors[x]:
            skip("floor")
            continue
        pos, aligned = 0, True
        for v, s, k in segs:
            if pos % 32 or k % 32 or (v >= 0 and s % 32):
                aligned = False
            pos += k
        if not aligned:
            skip("misaligned")
            continue
        if n not in los or n not in his:
            skip("no_interval")
            continue
        par = image_params(los[n], his[n])
        if par is None:
            skip("no_interval")
            continue
        inverses = [(inv, 0, nb)]
        bad = False
        for g, gname in enumerate(syms.func_names):
            base_name, sl = split_slice(gname)
            if sl is not None and base_name == name + "-1":
                if sl[0] % 32 or (sl[1] - sl[0]) % 32 or sl[1] > nb:
                    bad = True
                inverses.append((g, sl[0], sl[1]))
        if bad:
            skip("misaligned")
            continue
        if any(derived_of.get(syms.func_names[g]) for g, _, _ in inverses):
            skip("inverse_derived")
            continue
        dvs = sorted(derived_of.get(name, []))
        if len(dvs) > MAX_COLLISIONS:
            skip("too_many_derived")
            continue
        if len(sites) >= MAX_SITES:
            skip("too_many_sites")
            continue
        words: List[Tuple[int, int]] = []
        for v, s, k in segs:
            for i in range(k // 32):
                words.append((int(off[v]) + s // 32 + i, 0) if v >= 0 else (-1, (s >> (32 * i)) & 0xFFFFFFFF))
        coll = [(int(syms.derived[v][1][0]), v, int(off[v])) for v in dvs]
        sites.append(KeccakSite(n, f, nb, inverses, segs, words, par[0], par[1], coll))
    return sites, skipped


class _OneRoot:
    """A one-root view of a DAG batch (:func:`_reachable` under a single node)."""

    def __init__(self, db, root: int):
        self.nodes = db.nodes
        self.roots = np.asarray([root], np.uint32)
        self.root_offsets = np.asarray([0, 1], np.int64)


def keccak_sites_of(db, syms, off: np.ndarray, blocks: List[Tuple[Tuple, np.ndarray]]) -> KeccakSites:
    """The batch's sites with each block's active mask: site i is active in block j iff the
    block's patch assigns (a value or a floor of) a variable of the site's map."""
    sites, skipped = find_keccak_sites(db, syms, off)
    active = np.zeros(len(blocks), np.uint64)
    for j, (patch, _) in enumerate(blocks):
        vs = {el[0] for el in patch}
        m = 0
        for i, s in enumerate(sites):
            if vs & s.vars:
                m |= 1 << i
        active[j] = m
    return KeccakSites(sites, active, skipped)


def _site_values(ks: KeccakSites, words: np.ndarray, n_lru: int, starts: np.ndarray):
    """Per site ``(candidates k, x words [n, n/32], v words [n, 8])`` over the candidates of the
    blocks the site is active in; ``words`` is the batch's row matrix (patched and floored)."""
    out = []
    for i, s in enumerate(ks.sites):
        js = np.flatnonzero((ks.active >> np.uint64(i)) & np.uint64(1))
        cols = np.concatenate([np.arange(int(starts[j]), int(starts[j + 1]), dtype=np.int64) for j in js]) \
            if len(js) else np.zeros(0, np.int64)
        nw = s.n_bits // 32
        xw = np.zeros((len(cols), nw), np.uint32)
        for l, (row, cv) in enumerate(s.words):
            xw[:, l] = words[row, n_lru + cols] if row >= 0 else cv
        raw = np.ascontiguousarray(xw[:, ::-1]).astype(">u4").tobytes()
        xs = [int.from_bytes(raw[4 * nw * t:4 * nw * (t + 1)], "big") for t in range(len(cols))]
        vs = keccak_images(xs, s.n_bits, s.base, s.b)
        vw = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vs), "<u4").reshape(len(cols), 8).copy()
        for key, _, r0 in s.collisions:
            hit = np.flatnonzero((xw == np.asarray(to_words(key, s.n_bits), np.uint32)[None, :]).all(axis=1))
            if len(hit):
                vw[hit] = words[r0:r0 + 8, n_lru + cols[hit]].T
        out.append((cols, xw, vw))
    return out


def _table_triples(lru: ModelBatch, blocks: List[Tuple[Tuple, np.ndarray]], syms):
    """Per function: (block, position among the block's changed derived vars of it, var) triples:
    the entries a block's patch adds in front of the base model's (per function by ascending
    variable index)."""
    func_index = {name: f for f, name in enumerate(syms.func_names)}
    dfunc = {v: func_index[fn] for v, (fn, _) in syms.derived.items() if fn in func_index}
    per_f: Dict[int, Tuple[List[int], List[int], List[int]]] = {}
    for j, (patch, _) in enumerate(blocks):
        vs = {el[0] for el in patch if el[0] in dfunc and el[1] >= 0}
        if not vs:
            continue
        pos: Dict[int, int] = {}
        for v in sorted(vs):
            f = dfunc[v]
            t = per_f.setdefault(f, ([], [], []))
            t[0].append(j)
            t[1].append(pos.get(f, 0))
            t[2].append(v)
            pos[f] = pos.get(f, 0) + 1
    return per_f


def _function_tables(lru: ModelBatch, blocks, syms, per_f, src, starts, sizes, off, K, words, composed, sites=None,
                     site_words=None):
    """The fully materialised function tables of the LRU models followed by the K candidates:
    ``(entry_ptr, entry_words, entry_base, else_words, else_base)``.  A candidate's table is its
    base model's entries, preceded by an entry for every derived variable of that function its
    block's patch changed (so table and derived column agree; first match wins).  ``words`` is the
    batch's row matrix, or None with ``composed`` (:func:`_compose_blocks`) to compute the added
    values from the LRU rows and the blocks' composed patches.  ``sites`` (:class:`KeccakSites`):
    each active site's entries follow the base model's, read from ``site_words`` (default ``words``)."""
    n_lru = lru.n_models
    site_cnt = site_vals = None
    if sites is not None and sites.active.any() and K:   # (no active block: no entry, and no rows needed)
        site_cnt = sites.site_counts(len(lru.funcs))
        site_vals = _site_values(sites, words if site_words is None else site_words, n_lru, starts)
    M = n_lru + K
    F = len(lru.funcs)
    eptr = np.zeros((F, M + 1), np.int64)
    ew_chunks, el_chunks = [], []
    ebase = np.zeros(F, np.int64)
    elb = np.zeros(F, np.int64)
    wpos = epos = 0
    for f, spec in enumerate(lru.funcs):
        s = spec.stride
        base_ptr = lru.entry_ptr[f]
        base_cnt = np.diff(base_ptr)                                   # [n_lru]
        cnt_gen = base_cnt[src] if n_lru else np.zeros(K, np.int64)
        trip = per_f.get(f)
        if trip is not None:
            tj, ti, tv = (np.asarray(x, np.int64) for x in trip)
            add_cnt = np.repeat(np.bincount(tj, minlength=len(blocks)), sizes)
        else:
            add_cnt = np.zeros(K, np.int64)
        site_add = np.repeat(site_cnt[f], sizes) if site_cnt is not None else np.zeros(K, np.int64)
        counts = np.concatenate([base_cnt, cnt_gen + add_cnt + site_add])
        eptr[f, 1:] = np.cumsum(counts)
        ent = lru.entry_words[int(lru.entry_base[f]):int(lru.entry_base[f]) + int(base_ptr[-1]) * s].reshape(-1, s)
        out = np.zeros((int(eptr[f, -1]), s), np.uint32)
        out[:int(base_ptr[-1])] = ent
        gstarts = eptr[f, n_lru:n_lru + K]
        if trip is not None:
            # the changed derived vars' entries (key = their constant arguments, value = the
            # candidate's patched column), one row per (triple, candidate of its block)
            lens = sizes[tj]
            rep = np.repeat(np.arange(len(tj)), lens)
            within = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
            cols = starts[tj][rep] + within
            rows = gstarts[cols] + ti[rep]
            uv, vinv = np.unique(tv, return_inverse=True)
            keys = np.asarray([[w for aw, av in zip(spec.arg_widths, syms.derived[int(v)][1])
                                for w in to_words(int(av), aw)] for v in uv], np.uint32)
            klen = keys.shape[1]
            nl = limbs(syms.var_widths[int(uv[0])])
            out[rows, :klen] = keys[vinv[rep]]
            vrow = off[uv][vinv[rep]]
            if words is not None:
                out[rows, klen:klen + nl] = words[vrow[:, None] + np.arange(nl)[None, :], (n_lru + cols)[:, None]]
            else:
                # the same values without the matrix: the base model's limbs of that variable
                # under the block's composed (keep, bits), then its floor
                keep_t = np.full((len(tj), nl), 0xFFFFFFFF, np.uint32)
                bits_t = np.zeros((len(tj), nl), np.uint32)
                mins_t = np.zeros(len(tj), np.uint32)
                for t, (j, v) in enumerate(zip(trip[0], trip[2])):
                    prow, pfl = composed[j]
                    for i in range(nl):
                        c = prow.get(int(off[v]) + i)
                        if c is not None:
                            keep_t[t, i], bits_t[t, i] = ~c[0] & 0xFFFFFFFF, c[1]
                    mins_t[t] = pfl.get(v, 0)
                if n_lru:
                    vals = lru.var_words[vrow[:, None] + np.arange(nl)[None, :], src[cols][:, None]]
                else:
                    vals = np.zeros((len(cols), nl), np.uint32)
                vals = (vals & keep_t[rep]) | bits_t[rep]
                mn = mins_t[rep]
                if mn.any():
                    small = ~vals[:, 1:].any(axis=1)
                    vals[:, 0] = np.where(small & (vals[:, 0] < mn), mn, vals[:, 0])
                out[rows, klen:klen + nl] = vals
        if n_lru and K:
            gstart = gstarts + add_cnt
            rep = cnt_gen
            tot = int(rep.sum())
            if tot:
                cand = np.repeat(np.arange(K), rep)
                within = np.arange(tot) - np.repeat(np.cumsum(rep) - rep, rep)
                dst = gstart[cand] + within
                srcrow = base_ptr[src[cand]] + within
                out[dst] = ent[srcrow]
        if site_cnt is not None and site_add.any():
            # the active sites' entries behind the base model's, in site order: x -> v in the
            # site's own function, v -> bits [lo, hi) of x in its inverse and the inverse's slices
            at = gstarts + add_cnt + cnt_gen
            for i, sl in sites.contributions(f):
                cols, xw, vw = site_vals[i]
                if not len(cols):
                    continue
                rows = at[cols]
                if sl is None:
                    out[rows] = np.concatenate([xw, vw], axis=1)
                else:
                    out[rows] = np.concatenate([vw, xw[:, sl[0] // 32:sl[1] // 32]], axis=1)
                at[cols] += 1
        ebase[f] = wpos
        ew_chunks.append(out.reshape(-1))
        wpos += out.size
        nr = limbs(spec.result_width)
        lel = lru.else_words[int(lru.else_base[f]):int(lru.else_base[f]) + n_lru * nr].reshape(-1, nr) \
            if n_lru else np.zeros((0, nr), np.uint32)
        gel = lel[src] if n_lru else np.zeros((K, nr), np.uint32)
        elb[f] = epos
        el = np.concatenate([lel, gel]).reshape(-1)
        el_chunks.append(el)
        epos += el.size
    return eptr, np.concatenate(ew_chunks), ebase, np.concatenate(el_chunks), elb


class CandidateSet:
    """The LRU models followed by the generated candidates, serialized (``batch``), plus what is
    needed to turn a generated candidate back into a model (:meth:`materialize`).  Candidates
    come in blocks: one patch applied to a range of base models.

    From a generator with ``device_rows`` the set carries a :class:`Derivation` instead of the
    variable rows: ``batch.var_words`` is absent (the device expands the rows), and :meth:`rows`
    materialises the matrix on demand."""

    derivation: Optional[Derivation] = None
    table_derivation: Optional[TableDerivation] = None   # (a generator with ``device_tables``)
    keccak_sites: Optional[KeccakSites] = None           # (a generator with ``keccak_sites``)
    _row_args = None

    @property
    def keccak_skips(self) -> Dict[str, int]:
        """keccak applications that are no site, counted by reason (empty without ``keccak_sites``)."""
        return dict(self.keccak_sites.skipped) if self.keccak_sites is not None else {}

    def rows(self) -> np.ndarray:
        """The whole batch's variable rows [rows, n_lru + K] (:func:`_candidate_rows`; as
        uploaded, before the device masks them to the variables' widths)."""
        if self.batch.var_words is not None:
            return self.batch.var_words
        lru, src, starts, sizes, blocks, off, K = self._row_args
        return _candidate_rows(lru, src, starts, sizes, blocks, self.syms, off, K)

    def host_batch(self) -> ModelBatch:
        """``batch`` with its variable rows on the host (oracle re-checks)."""
        b = self.batch
        if b.var_words is not None:
            return b
        if b.entry_ptr is None:
            # device_tables: the tables were not built either
            lru, src, starts, sizes, blocks, off, K = self._row_args
            words = self.rows()
            if not lru.funcs:
                return ModelBatch(b.var_widths, words)
            per_f = _table_triples(lru, blocks, self.syms)
            return ModelBatch(b.var_widths, words, b.funcs, *_function_tables(
                lru, blocks, self.syms, per_f, src, starts, sizes, off, K, words, None, self.keccak_sites), b.index_base)
        return ModelBatch(b.var_widths, self.rows(), b.funcs, b.entry_ptr, b.entry_words, b.entry_base,
                          b.else_words, b.else_base, b.index_base)

    def __init__(self, batch: ModelBatch, n_lru: int, base: np.ndarray, block_of: np.ndarray,
                 block_patches: List[Tuple], syms, lru_models):
        self.batch = batch
        self.n_lru = n_lru
        self.base = base                  # [K] LRU index each candidate derives from (-1: none)
        self.block_of = block_of          # [K] its block
        self.block_patches = block_patches   # per block: tuple of (var, lo, n_bits, bits)
        self.syms = syms
        self.lru_models = list(lru_models)

    @property
    def n_generated(self) -> int:
        return self.batch.n_models - self.n_lru

    def patch(self, k: int) -> Tuple:
        return self.block_patches[int(self.block_of[k])]

    def materialize(self, index: int) -> Model:
        """Global candidate ``index`` (>= n_lru) as a model: the base model with the patched
        variables assigned and the patched derived variables entered in their tables."""
        k = index - self.n_lru
        b = int(self.base[k])
        rec = as_record(self.lru_models[b]) if b >= 0 else Model()
        asg = dict(rec.assignment)
        funcs = {name: (dict(e), els) for name, (e, els) in rec.functions.items()}
        names = {i: key for key, i in self.syms.vars.items()}
        vals: Dict[int, int] = {}
        for v, lo, n, bits in sorted(self.patch(k), key=lambda p: p[1] < 0):   # floors last
            if v not in vals:
                name, w = names[v]
                if v in self.syms.derived:
                    fname, fargs = self.syms.derived[v]
                    interp = funcs.get(fname)
                    vals[v] = 0 if interp is None else int(interp[0].get(fargs, interp[1]))
                else:
                    vals[v] = int(asg.get(name, 0) or 0)
            if lo < 0:
                if vals[v] < (1 << 32) and vals[v] < bits:
                    vals[v] = bits
                continue
            vals[v] = (vals[v] & ~(((1 << n) - 1) << lo)) | (bits << lo)
        for v, val in vals.items():
            name, w = names[v]
            if v in self.syms.derived:
                fname, fargs = self.syms.derived[v]
                e, els = funcs.get(fname, ({}, 0))
                e = dict(e)
                e[tuple(fargs)] = val
                funcs[fname] = (e, els)
            else:
                asg[name] = val
        ks = self.keccak_sites
        if ks is not None and ks.sites:
            self._materialize_sites(ks, int(ks.active[int(self.block_of[k])]), asg, funcs, names)
        return Model(asg, funcs)

    def _materialize_sites(self, ks: KeccakSites, mask: int, asg, funcs, names) -> None:
        """The active sites' entries of one candidate, in site order, behind what the model holds
        (``setdefault``: an entry for the same key keeps its value)."""
        def value(v: int) -> int:
            name, w = names[v]
            if v in self.syms.derived:
                fname, fargs = self.syms.derived[v]
                interp = funcs.get(fname)
                val = 0 if interp is None else int(interp[0].get(tuple(fargs), interp[1]))
            else:
                val = int(asg.get(name, 0) or 0)
            return val & ((1 << max(w, 1)) - 1)
        fnames = self.syms.func_names
        for i, s in enumerate(ks.sites):
            if not (mask >> i) & 1:
                continue
            x, pos = 0, 0
            for v, lo, n in s.segs:
                bits = lo if v < 0 else (value(v) >> lo) & ((1 << n) - 1)
                x |= bits << pos
                pos += n
            hit = [var for key, var, _ in s.collisions if key == x]
            img = value(hit[0]) if hit else keccak_images([x], s.n_bits, s.base, s.b)[0]
            for fname, key, val in ((fnames[s.func], x, img), (fnames[s.inverses[0][0]], img, x)):
                e, els = funcs.get(fname, ({}, 0))
                e = dict(e)
                e.setdefault((key,), val)
                funcs[fname] = (e, els)


class CandidateGenerator:
    """Generates up to ``max_candidates`` candidates for a batch of conjunctions (seeded)."""

    def __init__(self, max_candidates: int = 100_000, seed: int = 0, random_frac: float = 0.05, per_query: int = 16,
                 fill: bool = False, device_rows: bool = False, device_tables: bool = False,
                 keccak_sites: bool = False):
        if device_tables and not device_rows:
            raise ValueError("device_tables needs device_rows: the derived tables read the derived rows")
        # candidates whose patch changes the input of a keccak256_<n> application get that input's
        # image entered in keccak256_<n> and its inverse (KeccakSites; meant for device_tables: the
        # host modes hash every (candidate, site) on the CPU)
        self.keccak_sites = bool(keccak_sites)
        # the candidates' function tables are not materialised either: the set carries a
        # TableDerivation next to the Derivation (needs device_rows)
        self.device_tables = bool(device_tables)
        self.max_candidates = int(max_candidates)
        # the candidates' variable rows are not materialised: the set carries a Derivation for
        # Evaluator.upload_models_derived (VerdictEngine.candidate_first_hits, one device)
        self.device_rows = bool(device_rows)
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.random_frac = random_frac
        self.per_query = int(per_query)   # patches per query (each over every base model)
        self.fill = fill                  # fill max_candidates with random mixes (throughput runs)

    # ------------------------------------------------------------ targets
    def _targets(self, db, syms):
        """Per query: list of (patch-option lists) of its invertible branch conditions."""
        # a derived variable of a value slice (lower.py _wide_eq) shares its bits with the other
        # slices of the same function value: patching one alone would split them
        from .lower import SLICE
        opaque = frozenset(v for v, (f, _) in syms.derived.items() if SLICE in f)
        bm = _BitMaps(db.nodes, db.consts, opaque)
        op, a, b = bm.op, bm.a, bm.b
        per_query = []
        for q in range(db.n_tapes):
            roots = db.roots[db.root_offsets[q]:db.root_offsets[q + 1]]
            opts = []
            for r in roots:
                r = int(r)
                positive: Optional[bool] = True
                if op[r] == 10:                        # NOT(pred): the branch not taken
                    r, positive = int(a[r]), False
                # a conjunct that is itself an OR / deeper: look one level for a predicate
                if op[r] not in _PREDS:
                    continue
                x, y = int(a[r]), int(b[r])
                cx, cy = bm.const_value(x), bm.const_value(y)
                if cx is not None and cy is None:
                    segs, c, const_left, fl = bm.map(y), cx, True, None
                elif cy is not None and cx is None:
                    segs, c, const_left, fl = bm.map(x), cy, False, None
                else:
                    continue
                if segs is None or all(v < 0 for v, _, _ in segs):
                    continue
                floors = bm.floors[y if const_left else x]
                w = int(bm.w[x])
                o = []
                for val in _wanted(int(op[r]), const_left, c, w, positive):
                    p = _patch_for(segs, val)
                    if p is not None:
                        o.append(p + tuple((v, -1, 0, mn) for v, mn in floors))
                if o:
                    opts.append(o)
            per_query.append(opts)
        return per_query

    # ------------------------------------------------------------ generation
    def generate(self, db, syms, lru_batch: ModelBatch, lru_models: Sequence) -> CandidateSet:
        """``lru_batch`` (the serialized LRU, MRU first, index_base 0) followed by generated
        candidates; their model rows are patched copies of LRU rows (random fills: fresh).

        Blocks of one patch over every base model, in order: per query all its invertible
        conditions patched at once (two rounds of options), then single conditions newest first,
        at most ``per_query`` patches per query; random multi-condition mixes and boundary /
        random values of plain variables add ``random_frac`` of that.  The budget adapts to the
        batch: ``per_query`` x bases per query, capped by ``max_candidates``."""
        rng = self.rng
        n_lru = lru_batch.n_models
        per_query = self._targets(db, syms)
        base_ids = np.arange(n_lru, dtype=np.int64) if n_lru else np.full(1, -1, np.int64)
        nb = len(base_ids)
        n_q = sum(1 for o in per_query if o)
        budget = max(0, self.max_candidates - n_lru)
        if not self.fill:
            budget = min(budget, self.per_query * nb * max(n_q, 1))
        blocks: List[Tuple[Tuple, np.ndarray]] = []
        total = [0]
        seen = set()

        def add(patch: Tuple, bases: np.ndarray = base_ids, dedupe: bool = True) -> bool:
            if total[0] + len(bases) > budget:
                return False
            if dedupe:
                if patch in seen:
                    return True
                seen.add(patch)
            blocks.append((patch, bases))
            total[0] += len(bases)
            return True

        used = [0] * len(per_query)
        for rnd in range(2):
            for q, opts in enumerate(per_query):
                if not opts:
                    continue
                patch = tuple(p for o in opts for p in (o[0] if rnd == 0 else o[int(rng.integers(len(o)))]))
                if add(patch):
                    used[q] += 1
        depth = max((len(o) for o in per_query), default=0)
        for back in range(1, depth + 1):
            for q, opts in enumerate(per_query):
                if back > len(opts):
                    continue
                for p in opts[-back]:
                    if used[q] >= self.per_query:
                        break
                    if add(p):
                        used[q] += 1
        singles = [p for opts in per_query for o in opts for p in o]
        plain = [v for v, w in enumerate(syms.var_widths) if w > 0 and v not in syms.derived
                 and v not in syms.hoisted_vars]
        # (each random patch over every base model, like the directed ones)
        n_rand = budget - total[0] if self.fill else int(total[0] * self.random_frac)
        for _ in range(-(-n_rand // nb)):
            bases = base_ids if total[0] + nb <= budget else base_ids[:budget - total[0]]
            if not len(bases):
                break
            if singles and rng.random() < 0.7:
                k = int(rng.integers(1, 4))
                patch = tuple(q for i in rng.integers(0, len(singles), k) for q in singles[int(i)])
            elif plain:
                v = plain[int(rng.integers(len(plain)))]
                w = syms.var_widths[v]
                val = int(rng.choice([0, 1, (1 << w) - 1, 1 << (w - 1), (1 << (w - 1)) - 1,
                                      int.from_bytes(rng.bytes((w + 7) // 8), "little")])) & ((1 << w) - 1)
                patch = ((v, 0, w, val),)
            else:
                break
            if not add(patch, bases, dedupe=False):
                break
        if self.keccak_sites:   # (the batch _serialize looks for keccak sites in; off: the call as it always was)
            return self._serialize(lru_batch, blocks, syms, lru_models, db)
        return self._serialize(lru_batch, blocks, syms, lru_models)

    # ------------------------------------------------------------ serialization
    def _serialize(self, lru: ModelBatch, blocks: List[Tuple[Tuple, np.ndarray]], syms, lru_models,
                   db=None) -> CandidateSet:
        n_lru = lru.n_models
        sizes = np.asarray([len(b) for _, b in blocks], np.int64)
        K = int(sizes.sum())
        base = np.concatenate([b for _, b in blocks]) if blocks else np.zeros(0, np.int64)
        block_of = np.repeat(np.arange(len(blocks), dtype=np.int64), sizes)
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        off = lru.var_word_offsets()
        src = np.where(base >= 0, base, 0)
        M = n_lru + K
        composed = deriv = None
        if self.device_rows:
            # the rows stay a description (Derivation) the device expands; only the patched derived
            # variables' values, which enter the function tables below, are computed here
            composed = _compose_blocks(blocks, off, syms)
            deriv = derivation_arrays(lru, base, blocks, starts, sizes, off, syms, composed)
            words = None
        else:
            words = _candidate_rows(lru, src, starts, sizes, blocks, syms, off, K)
        # the batch's keccak sites (found once per batch) and the blocks' active masks
        sites = None
        if self.keccak_sites and db is not None and lru.funcs:
            sites = keccak_sites_of(db, syms, off, blocks)

        def done(mb: ModelBatch) -> CandidateSet:
            cs = CandidateSet(mb, n_lru, base, block_of, [p for p, _ in blocks], syms, lru_models)
            cs.keccak_sites = sites
            if deriv is not None:
                cs.derivation = deriv
                cs._row_args = (lru, src, starts, sizes, blocks, off, K)
            return cs
        if not lru.funcs:
            return done(ModelBatch(lru.var_widths, words, n_models=M, tables=not self.device_tables))
        per_f = _table_triples(lru, blocks, syms)
        if self.device_tables:
            # the tables stay a description too (TableDerivation): the LRU's own tables, and per
            # block the (function, variable, key) of each entry its patch adds
            cs = done(ModelBatch(lru.var_widths, None, lru.funcs, n_models=M, tables=False))
            cs.table_derivation = table_derivation_arrays(lru, len(blocks), per_f, syms)
            return cs
        site_words = words
        if sites is not None and sites.active.any() and words is None:
            # (device_rows with host tables: the sites' inputs are read from the rows, built here for that)
            site_words = _candidate_rows(lru, src, starts, sizes, blocks, syms, off, K)
        eptr, ew, ebase, el, elb = _function_tables(lru, blocks, syms, per_f, src, starts, sizes, off, K, words, composed,
                                                    sites, site_words)
        return done(ModelBatch(lru.var_widths, words, lru.funcs, eptr, ew, ebase, el, elb, 0, n_models=M))
