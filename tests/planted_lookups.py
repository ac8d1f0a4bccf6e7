"""Planted-result workload for table lookups, arrays, keccak and the Bool connectives (test helper).

The companion of planted_ops.py for the rest of the vocabulary of include/mq.h: ``UF`` of one and two
arguments, ``SELECT`` over ``ARRAY_VAR`` / ``CONST_ARRAY`` / ``STORE`` chains, wide-key lookups
(``UF_CHUNK`` / ``UF_WIDE``), ``KECCAK`` and NOT / AND / OR / XOR / IMPLIES / IFF / BITE.  Every case
is ONE such operation:

* a value result goes into the tape ``EQ(op(...), R)``; model variable R holds the reference result
  of that model in even models and the same with exactly one bit flipped in odd ones (the flipped
  bit walks over the result as in planted_ops.flip_positions);
* a Bool result is the root itself, and ``NOT(root)`` a second tape.

The reference (:func:`ref_lookup`, :func:`ref_select`, the truth tables of :func:`ref_bool`) is plain
Python over ORDERED entry lists - the first entry whose key equals the query wins (mq.h) - and
shares no code with the oracles.  The model batches are built from those ordered lists directly
(:func:`tables_arrays`), so duplicate keys and entry order are expressible, which
``ModelBatch.from_python`` (a dict per table) cannot do.

Per-model table classes cycle with the model index: an entry-count cycle of 11 and a scenario cycle
of 13 (hit slot, absent key, near-miss entries before the hit, duplicates), both coprime to 2 and to
each other, so every (count, scenario) pair meets flipped and unflipped models within 286 models.
The classes a table really holds are read back from its content (:func:`table_labels`), and
test_planted_lookups.py asserts them per signature.

M = 577 models (nine full waves and a ragged one); the keccak groups use 150 (two full waves and a
ragged one of 22 lanes: the pure-Python hash costs a millisecond a block).
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

import keccak_ref
from mythril_amd.models import FuncSpec, ModelBatch
from mythril_amd.tape import Tape, TapeBatch, limbs
from planted_ops import M, N_PRELOADED, _rows, flip_positions, mask, xor_const

M_KECCAK = 150
COUNTS_CSR = (0, 1, 2, 7, 8, 9, 15, 16, 17, 24, 40)        # both sides of kDenseMaxE = 16, up to five scan rounds
COUNTS_DENSE = (0, 1, 2, 7, 8, 9, 15, 16, 16, 15, 16)      # mean 9.5: the memory bound of mq_models_upload holds
COUNTS_WIDE = (0, 1, 2, 32, 33, 64, 1)                     # wide-key sets hold at most 64 entries
N_SCEN = 13
N_SCEN_WIDE = 9
M32 = 0xFFFFFFFF
GROUPS = ("uf1", "uf2", "array", "widekey", "keccak", "keccak_columns", "bool")
LOOKUP_GROUPS = ("uf1", "uf2", "array", "widekey")


# ---------------------------------------------------------------- reference semantics
def ref_lookup(entries: Sequence[Tuple[Tuple[int, ...], int]], else_value: int, key: Tuple[int, ...]) -> int:
    """The value of the first entry whose key tuple equals ``key``, else the else value."""
    for k, v in entries:
        if k == key:
            return v
    return else_value


def ref_select(term, idx: int, lookup=ref_lookup) -> int:
    """``term``: ("store", inner, index, value) | ("const", value) | ("var", entries, else_value).
    The outermost store whose index equals ``idx`` wins, otherwise the base decides."""
    while term[0] == "store":
        if term[2] == idx:
            return term[3]
        term = term[1]
    if term[0] == "const":
        return term[1]
    return lookup(term[1], term[2], (idx,))


def ref_bool(op: str, a: int, b: int = 0, c: int = 0) -> int:
    return {"NOT": 1 - a, "AND": a & b, "OR": a | b, "XOR": a ^ b, "IMPLIES": (1 - a) | b, "IFF": int(a == b),
            "BITE": b if a else c}[op]


def ref_keccak(value: int, width: int) -> int:
    """MQ_OP_KECCAK: keccak256 of the value's width / 8 big-endian bytes, read big-endian."""
    return _keccak_cached(value.to_bytes(width // 8, "big"))


@functools.lru_cache(maxsize=None)
def _keccak_cached(data: bytes) -> int:
    return int.from_bytes(keccak_ref.keccak256(data), "big")


# ---------------------------------------------------------------- tables
@dataclass
class Table:
    """One model function: per model an ordered entry list and an else value."""
    name: str
    spec: FuncSpec
    entries: List[List[Tuple[Tuple[int, ...], int]]]
    elses: List[int]
    dense: bool = False            # meant for the dense slot layout (mq_models_upload)
    counts: Tuple[int, ...] = ()   # the entry counts its models hold

    def get(self, m: int, key: Tuple[int, ...]) -> int:
        return ref_lookup(self.entries[m], self.elses[m], key)


def _limb(v: int, k: int) -> int:
    return (v >> (32 * k)) & M32


def differ(rng: random.Random, rw: int, *avoid: int) -> int:
    """A value of ``rw`` bits (Bool: 1) each of whose limbs differs from the same limb of every
    ``avoid`` value, as far as the limb has room (earlier ``avoid`` values take precedence)."""
    rw = max(rw, 1)
    out = 0
    for l in range(limbs(rw)):
        lw = min(32, rw - 32 * l)
        bad = []
        for a in avoid:
            if len(bad) + 1 < (1 << lw) and _limb(a, l) not in bad:
                bad.append(_limb(a, l))
        x = rng.getrandbits(lw)
        while x in bad or (lw >= 8 and x == 0):
            x = rng.getrandbits(lw)
        out |= x << (32 * l)
    return out


def _other_key(rng, widths, q):
    for _ in range(6):
        k = tuple(rng.getrandbits(w) for w in widths)
        if k != q and (_limb(k[0], 0) != _limb(q[0], 0) or widths[0] < 8):
            return k
    return k


def _model_entries(rng, spec: FuncSpec, n: int, scen: int, j: int, q: Tuple[int, ...], hv: int, dv: int, fck: int = 0, els: int = 0):
    """The ordered entries of one model for query ``q``: scenario ``scen`` (module docstring) as far
    as ``n`` entries allow.  hv: the value of the true match, dv: that of a later duplicate, fck: which
    higher key limb a false candidate differs in."""
    ws = spec.arg_widths
    rw = spec.result_width
    ent = [(_other_key(rng, ws, q), differ(rng, rw)) for _ in range(n)]
    if n == 0:
        return ent
    L0 = limbs(ws[0])

    def put(slot, key, val=None):
        if 0 <= slot < n:
            ent[slot] = (tuple(key), differ(rng, rw, *((hv, els) if rng.random() < 0.5 else (els, hv))) if val is None else val)

    def false_cand(k):      # limb 0 of argument 0 equal, one bit of a higher limb (or of argument 1) differs
        higher = [(0, l) for l in range(1, L0)] + ([(1, l) for l in range(limbs(ws[1]))] if len(q) > 1 else [])
        if not higher:
            return lo_only()
        a, lim = higher[(fck + k) % len(higher)]
        bit = 1 << (32 * lim + rng.randrange(min(32, ws[a] - 32 * lim)))
        return (q[0] ^ bit,) + q[1:] if a == 0 else (q[0], q[1] ^ bit)

    def lo_only():          # differs in limb 0 of argument 0 only
        return (q[0] ^ (1 << rng.randrange(min(32, ws[0]))),) + q[1:]

    def top_only():
        return (q[0] ^ (1 << (ws[0] - 1)),) + q[1:]

    def arg_only(i):        # arity 2: argument i equal, the other not
        o = _other_key(rng, ws, q)
        return (q[0], o[1] if o[1] != q[1] else q[1] ^ 1) if i == 0 else (o[0] if o[0] != q[0] else q[0] ^ 1, q[1])

    def swapped():
        return (q[1] & mask(ws[0]), q[0] & mask(ws[1]))

    if scen <= 4:
        h = min((0, 6, 7, 8, n - 1)[scen], n - 1)
        if len(q) > 1 and h > 0:
            put(h - 1, (arg_only(0), arg_only(1), swapped())[j % 3])
        put(h, q, hv)
    elif scen == 5:
        if len(q) == 1:
            put(n // 2, false_cand(0))
        else:
            for s, k in enumerate((arg_only(0), arg_only(1), swapped())):
                put((j + s) % n if n >= 3 else s, k)
    elif scen == 6:
        put(n - 1, top_only())
        if n > 1:
            put(0, lo_only())
    elif scen == 7:         # a false candidate right before the match: same scan round unless h % 8 == 0
        h = n - 1 if j % 2 or n <= 8 else 7
        put(h - 1, false_cand(0))
        put(h, q, hv)
    elif scen == 8:         # a false candidate in slot 0, the match in the last slot (a later round for n > 8)
        put(0, false_cand(0))
        put(n - 1, q, hv)
    elif scen == 9:
        put(0, top_only())
        put(n - 2, lo_only())
        put(n - 1, q, hv)
    elif scen == 10:        # the same key twice in one round
        h = min((0, 5)[j % 2], max(n - 2, 0))
        put(h + 1, q, dv)
        put(h, q, hv)
    elif scen == 11:        # the same key in the first and in the last slot
        put(n - 1, q, dv)
        put(0, q, hv)
    else:                   # false candidate, true match, duplicate
        put(0, false_cand(0))
        put(n - 1, q, dv)
        put(min(1, n - 1), q, hv)
    return ent


def make_table(name: str, spec: FuncSpec, counts: Sequence[int], queries: Sequence[Tuple[int, ...]], dense: bool = False,
               scen_of: Optional[Callable[[int], int]] = None, count_of: Optional[Callable[[int], int]] = None) -> Table:
    """Count class m % len(counts), scenario m % 13 (or ``scen_of(m)`` / ``count_of(m)``); the
    else value differs in every limb from the hit's value and the previous model's else value."""
    rng = random.Random("table/" + name)
    rw = spec.result_width
    entries, elses = [], []
    prev = 0
    fck = [0, 0]        # false candidates so far in even / odd models: their limbs advance one by one
    for m, q in enumerate(queries):
        n = count_of(m) if count_of else counts[m % len(counts)]
        scen = scen_of(m) if scen_of else m % N_SCEN
        j = m // (max(len(counts), 1) * N_SCEN)
        els = differ(rng, rw, prev)
        hv = differ(rng, rw, els, prev)
        dv = differ(rng, rw, hv, els)
        q = tuple(q)
        entries.append(_model_entries(rng, spec, n, scen, m // 2 + j, q, hv, dv, fck[m % 2], els))
        fck[m % 2] += scen in (5, 7, 8, 12) and any(k != q and _limb(k[0], 0) == _limb(q[0], 0) for k, _ in entries[-1])
        elses.append(els)
        prev = els
    return Table(name, spec, entries, elses, dense, tuple(sorted({len(e) for e in entries})))


def table_labels(tab: Table, m: int, q: Tuple[int, ...]) -> set:
    """The classes model m's table holds for query q, read from its content."""
    ent = tab.entries[m]
    ws = tab.spec.arg_widths
    hits = [i for i, (k, _) in enumerate(ent) if k == q]
    out = {f"n={len(ent)}"}
    h = hits[0] if hits else len(ent)
    out.add(f"hit@{h}" if hits else "absent")
    if hits and h == len(ent) - 1:
        out.add("hit@last")
    if len(hits) > 1 and ent[hits[1]][1] != ent[h][1]:
        out.add("dup-same-round" if hits[1] // 8 == h // 8 else "dup-later-round")
    for i, (k, _) in enumerate(ent[:h]):
        if k == q:
            continue
        d0 = k[0] ^ q[0]
        rest = k[1:] == q[1:]
        if _limb(d0, 0) == 0 and limbs(ws[0]) > 1:
            out.add(("false-cand-same-round" if i // 8 == h // 8 else "false-cand-earlier-round") if hits else "false-cand-absent")
            if rest and bin(d0).count("1") == 1:
                out.add(f"near-limb{(d0.bit_length() - 1) // 32}")
        if rest and d0 and d0 >> 32 == 0:
            out.add("near-limb0-only")
        if rest and d0 == 1 << (ws[0] - 1):
            out.add("near-top-bit")
        if len(q) > 1:
            if k[0] == q[0]:
                out.add("arg0-only")
            elif k[1] == q[1]:
                out.add("arg1-only")
            if k == (q[1] & mask(ws[0]), q[0] & mask(ws[1])):
                out.add("swapped")
    return out


def tables_arrays(tables: Sequence[Table], n_models: int):
    """(funcs, entry_ptr, entry_words, entry_base, else_words, else_base) of mq_model_batch from the
    ordered entry lists: entry e of model m of function f is ``stride`` words (argument limbs, then
    result limbs) at entry_base[f] + (entry_ptr[f, m] + e) * stride."""
    F = len(tables)
    ptr = np.zeros((max(F, 1), n_models + 1), np.int64)
    ebase, lbase = np.zeros(max(F, 1), np.int64), np.zeros(max(F, 1), np.int64)
    ew, lw = [], []
    epos = lpos = 0
    for f, tab in enumerate(tables):
        spec = tab.spec
        nls = [limbs(w) for w in spec.arg_widths] + [limbs(spec.result_width)]
        ebase[f], lbase[f] = epos, lpos
        raw = bytearray()
        n = 0
        for m in range(n_models):
            ptr[f, m] = n
            for key, val in tab.entries[m]:
                for x, nl in zip(key + (val,), nls):
                    raw += int(x).to_bytes(4 * nl, "little")
            n += len(tab.entries[m])
        ptr[f, n_models] = n
        words = np.frombuffer(bytes(raw), np.uint32)
        assert len(words) == n * spec.stride
        ew.append(words)
        epos += len(words)
        lw.append(_rows(max(spec.result_width, 1), tab.elses).T.reshape(-1))
        lpos += n_models * nls[-1]
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(1, np.uint32)      # noqa: E731
    return [t.spec for t in tables], ptr, cat(ew), ebase, cat(lw), lbase


def dense_expected(tab: Table) -> int:
    """The dense condition of mq_models_upload restated: the slots per model, 0 for the CSR layout."""
    s = tab.spec
    nl_a0, nl_res = limbs(s.arg_widths[0]), limbs(s.result_width)
    counts = [len(e) for e in tab.entries]
    emax, total, n = max(counts), sum(counts), len(counts)
    if s.arity != 1 or nl_a0 > 8 or nl_res > 8:
        return 0
    if emax == 0 or emax > 16 or emax * (nl_a0 + nl_res) * n > 2 * total * s.stride + 16 * n:
        return 0
    return emax


# ---------------------------------------------------------------- semantics (reference and faults)
class Sem:
    """What a case computes its value with; a fault model overrides one method."""
    name = "ref"

    def lookup(self, tab: Table, m: int, key: Tuple[int, ...], raw: Optional[Tuple[int, ...]] = None) -> int:
        """``raw``: the query before it is masked to the key width (the "a" operand form)."""
        return ref_lookup(tab.entries[m], tab.elses[m], key)

    def select(self, term, idx: int, tab: Optional[Table], m: int) -> int:
        return ref_select(term, idx, lambda e, d, k: self.lookup(tab, m, k))

    def wide(self, tab: Table, m: int, key: Tuple[int, ...]) -> int:
        return self.lookup(tab, m, key)

    def keccak(self, value: int, width: int) -> int:
        return ref_keccak(value, width)

    def boolean(self, op: str, a: int, b: int = 0, c: int = 0) -> int:
        return ref_bool(op, a, b, c)

    def can(self, case: "LCase") -> bool:
        return True


REF = Sem()


def _first(tab, m, pred):
    for i, (k, v) in enumerate(tab.entries[m]):
        if pred(i, k):
            return i
    return None


class LookupFault(Sem):
    """``match(tab, i, entry key, query)`` picks the entry, ``value(tab, m, i)`` what it returns."""
    groups = LOOKUP_GROUPS

    def __init__(self, name, match=None, value=None, can=None, last=False, groups=None):
        self.name, self._match, self._value, self._can, self._last = name, match, value, can, last
        if groups:
            self.groups = groups

    def lookup(self, tab, m, key, raw=None):
        ent = tab.entries[m]
        match = self._match or (lambda t, i, k, q, r: k == q)
        idx = [i for i, (k, _) in enumerate(ent) if match(tab, i, k, key, raw)]
        i = (idx[-1] if self._last else idx[0]) if idx else None
        if self._value:
            return self._value(tab, m, i)
        return ent[i][1] if i is not None else tab.elses[m]

    def can(self, case):
        return case.group in self.groups and bool(case.tables) and (self._can is None or self._can(case))


def _key_limbs(spec):
    return sum(limbs(w) for w in spec.arg_widths)


def _flat(key, ws):
    """The key tuple as one integer of its limbs, argument 0 lowest."""
    out = sh = 0
    for k, w in zip(key, ws):
        out |= k << sh
        sh += 32 * limbs(w)
    return out


def lookup_faults() -> List[Sem]:
    F: List[Sem] = []
    val = lambda t, m, i: t.entries[m][i][1] if i is not None else t.elses[m]      # noqa: E731
    F.append(LookupFault("last match wins", last=True))
    F.append(LookupFault("only key limb 0 compared", lambda t, i, k, q, r: _limb(k[0], 0) == _limb(q[0], 0),
                         can=lambda c: _key_limbs(c.tables[0].spec) > 1))
    for kk in range(64):
        F.append(LookupFault(f"key limb {kk} ignored",
                             lambda t, i, k, q, r, kk=kk: (_flat(k, t.spec.arg_widths) ^ _flat(q, t.spec.arg_widths)) & ~(M32 << (32 * kk)) == 0,
                             can=lambda c, kk=kk: kk < _key_limbs(c.tables[0].spec), groups=("uf1", "uf2", "array")))
    F.append(LookupFault("top key bits above the width compared", lambda t, i, k, q, r: k == (r if r is not None else q),
                         can=lambda c: c.form == "a"))
    F.append(LookupFault("argument 1 ignored", lambda t, i, k, q, r: k[0] == q[0], can=lambda c: c.tables[0].spec.arity == 2))
    F.append(LookupFault("arguments swapped", lambda t, i, k, q, r: k == (q[1] & mask(t.spec.arg_widths[0]), q[0] & mask(t.spec.arg_widths[1])),
                         can=lambda c: c.tables[0].spec.arity == 2))
    for s in (8, 16):
        F.append(LookupFault(f"a match in slot >= {s} missed", lambda t, i, k, q, r, s=s: k == q and i < s,
                             can=lambda c, s=s: max(c.tables[0].counts) > s))
    F.append(LookupFault("the slot after the match returned",
                         value=lambda t, m, i: t.elses[m] if i is None or i + 1 >= len(t.entries[m]) else t.entries[m][i + 1][1]))
    F.append(LookupFault("a matched lane returns the else value", value=lambda t, m, i: t.elses[m]))
    for d in (1, -1):
        F.append(LookupFault(f"else value of model m{d:+d}",
                             value=lambda t, m, i, d=d: val(t, m, i) if i is not None else t.elses[min(max(m + d, 0), len(t.elses) - 1)]))
    for kk in range(64):
        lm = M32 << (32 * kk)
        F.append(LookupFault(f"value limb {kk} dropped", value=lambda t, m, i, lm=lm: val(t, m, i) & ~lm,
                             can=lambda c, kk=kk: kk < limbs(c.tables[0].spec.result_width)))
        F.append(LookupFault(f"value limb {kk} taken from the else value",
                             value=lambda t, m, i, lm=lm: (val(t, m, i) & ~lm) | (t.elses[m] & lm),
                             can=lambda c, kk=kk: kk < limbs(c.tables[0].spec.result_width)))
    # (tables are canonical - a value above its width is no supported input - so nothing can tell
    # an unmasked result from a masked one: applicable nowhere, listed for the record)
    F.append(LookupFault("result not masked to its width", can=lambda c: False))
    F.append(LookupFault("Bool result taken from bit 1", value=lambda t, m, i: (val(t, m, i) >> 1) & 1,
                         can=lambda c: c.tables[0].spec.result_width == 0))
    return F


class SelectFault(Sem):
    def __init__(self, name, fn):
        self.name, self._fn = name, fn

    def select(self, term, idx, tab, m):
        return self._fn(term, idx, lambda t: ref_select(t, idx))

    def can(self, case):
        return case.group == "array" and case.depth >= 2


def _innermost(term, idx, rest):
    hit = None
    t = term
    while t[0] == "store":
        if t[2] == idx:
            hit = t[3]
        t = t[1]
    return hit if hit is not None else rest(t)


def _one_level(term, idx, rest):
    if term[0] != "store" or term[2] == idx:
        return rest(term)
    t = term
    while t[0] == "store":
        t = t[1]
    return rest(t)


class WideFault(Sem):
    """Wide-key lookups: the key is matched 256 bits a chunk into a 64-bit entry set."""

    def __init__(self, name, match, can=None):
        self.name, self._match, self._can = name, match, can

    def wide(self, tab, m, key):
        i = _first(tab, m, lambda i, k: self._match(tab, m, i, k[0], key[0]))
        return tab.entries[m][i][1] if i is not None else tab.elses[m]

    def can(self, case):
        return case.group == "widekey" and (self._can is None or self._can(case))


def _short_chunk_as_full(tab, m, i, k, q):
    """The last chunk of an entry read as 8 limbs: the entry's value limbs follow its key."""
    w = tab.spec.arg_widths[0]
    short = limbs(w) % 8
    spill = tab.entries[m][i][1] & mask(32 * (8 - short))
    return k == q and spill == 0


def wide_faults() -> List[Sem]:
    F: List[Sem] = [WideFault("wide-key set limited to 32 entries", lambda t, m, i, k, q: k == q and i < 32),
                    WideFault("last short chunk compared as a full chunk", _short_chunk_as_full,
                              can=lambda c: limbs(c.tables[0].spec.arg_widths[0]) % 8 != 0)]
    for kk in range(16):
        F.append(WideFault(f"chunk {kk} skipped", lambda t, m, i, k, q, kk=kk: (k ^ q) & ~(mask(256) << (256 * kk)) == 0,
                           can=lambda c, kk=kk: 256 * kk < c.tables[0].spec.arg_widths[0]))
    return F


class KeccakFault(Sem):
    def __init__(self, name, fn, can):
        self.name, self._fn, self._can = name, fn, can

    def keccak(self, value, width):
        return self._fn(value.to_bytes(width // 8, "big"))

    def can(self, case):
        return case.group in ("keccak", "keccak_columns") and self._can(case.kw // 8)


def _sponge(data: bytes, pad_at: Optional[int] = None, blocks: Optional[int] = None) -> int:
    msg = bytearray(data)
    if pad_at is None:
        msg.append(1)
    else:
        msg += bytes(pad_at - len(msg)) + b"\x01"
    msg += bytes(-len(msg) % 136)
    msg[-1] |= 0x80
    state = [0] * 25
    for off in range(0, len(msg), 136)[:blocks]:
        for i in range(17):
            state[i] ^= int.from_bytes(msg[off + 8 * i:off + 8 * i + 8], "little")
        state = keccak_ref.keccak_f1600(state)
    return int.from_bytes(b"".join(s.to_bytes(8, "little") for s in state)[:32], "big")


def _swap_limbs(d: int) -> int:
    b = d.to_bytes(32, "big")
    return int.from_bytes(b"".join(b[i:i + 4][::-1] for i in range(0, 32, 4)), "big")


def keccak_faults() -> List[Sem]:
    return [KeccakFault("keccak pad byte misplaced by one at the 135 / 136-byte boundary",
                        lambda d: _sponge(d, pad_at=len(d) + 1) if len(d) in (135, 136) else _keccak_cached(d), lambda n: n in (135, 136)),
            KeccakFault("second block dropped", lambda d: _sponge(d, blocks=1) if len(d) >= 136 else _keccak_cached(d), lambda n: n >= 136),
            KeccakFault("digest byte order reversed per limb", lambda d: _swap_limbs(_keccak_cached(d)), lambda n: True)]


class BoolFault(Sem):
    def __init__(self, op, name, fn):
        self.op, self.name, self._fn = op, f"{op}: {name}", fn

    def boolean(self, op, a, b=0, c=0):
        return self._fn(a, b, c) if op == self.op else ref_bool(op, a, b, c)

    def can(self, case):
        return case.group == "bool" and case.sig == self.op


def bool_faults() -> List[Sem]:
    return [BoolFault("NOT", "identity", lambda a, b, c: a), BoolFault("AND", "computed as OR", lambda a, b, c: a | b),
            BoolFault("OR", "computed as XOR", lambda a, b, c: a ^ b), BoolFault("XOR", "computed as OR", lambda a, b, c: a | b),
            BoolFault("IMPLIES", "operands reversed", lambda a, b, c: (1 - b) | a), BoolFault("IFF", "computed as XOR", lambda a, b, c: a ^ b),
            BoolFault("IFF", "computed as IMPLIES", lambda a, b, c: (1 - a) | b), BoolFault("BITE", "branches swapped", lambda a, b, c: c if a else b),
            BoolFault("BITE", "condition ignored", lambda a, b, c: b)]


@functools.lru_cache(maxsize=None)
def all_faults() -> Tuple[Sem, ...]:
    return tuple(lookup_faults() + [SelectFault("innermost store wins", _innermost), SelectFault("store chain stops after one level", _one_level)]
                 + wide_faults() + keccak_faults() + bool_faults())


# ---------------------------------------------------------------- a case
@dataclass
class LCase:
    group: str
    sig: str                      # signature / op / width: the cell the sensitivity test counts per
    form: str
    place: str                    # "lo": variables below index 8; "hi": from index 8 up
    negate: bool
    rw: int                       # result width, 0: Bool
    value: Callable[[int, Sem], int]                 # (model, semantics) -> the operation's result
    var_specs: List[Tuple[int, List[int]]]           # without R
    tables: List[Table]
    term: Callable[[Tape, Sequence[int], Sequence[int]], int]     # (tape, variable indices, function ids) -> node
    info: Callable[[int], str]
    n_models: int = M
    depth: int = 0                # array: stores in the chain
    kw: int = 0                   # keccak: message bits
    queries: Optional[List[Tuple[int, ...]]] = None      # lookups: the query key tuple of every model
    kernel: str = ""              # the kernel class the GPU test asserts (test_gpu_planted_lookups.expected_kernel)
    rs: Optional[List[int]] = None
    expect: np.ndarray = field(default=None, repr=False)

    def __post_init__(self):
        n = self.n_models
        vals = [self.value(m, REF) for m in range(n)]
        if self.rw:
            pos = flip_positions(self.rw)
            self.rs = [v ^ (1 << pos[(m // 2 + self.flip_shift) * self.flip_step % len(pos)]) if m % 2 else v for m, v in enumerate(vals)]
            self.var_specs = self.var_specs + [(self.rw, self.rs)]
            self.expect = np.arange(n) % 2 == 0
        else:
            self.expect = np.array([bool(v) != self.negate for v in vals])

    flip_shift = 0                # odd model m flips bit flip_positions[(m // 2 + flip_shift) * flip_step]
    flip_step = 1

    def name(self) -> str:
        return f"{'NOT ' if self.negate else ''}{self.group} {self.sig} form={self.form} place={self.place}"

    def build(self, vi: Sequence[int], fi: Sequence[int]) -> Tape:
        t = Tape()
        v = self.term(t, vi, fi)
        if self.rw:
            return t.finish(t.eq(v, t.var(vi[-1], self.rw)))
        return t.finish(t.not_(v) if self.negate else v)

    def describe(self, m: int) -> str:
        s = f"{self.name()} model {m}: {self.info(m)}; reference result {self.value(m, REF):#x}"
        if self.rs is not None:
            s += f" planted R={self.rs[m]:#x}"
        return s + f" expected verdict {bool(self.expect[m])}"

    def killed_by(self, fault: Sem) -> bool:
        for m in range(self.n_models):
            got = self.value(m, fault)
            if self.rs is not None:
                if ((got == self.rs[m]) != getattr(self, "negate_eq", False)) != bool(self.expect[m]):
                    return True
            elif (bool(got) != self.negate) != bool(self.expect[m]):
                return True
        return False


def _with_not(**kw) -> List[LCase]:
    """Value results: one case; Bool results: the tape and its negation."""
    if kw["rw"]:
        return [LCase(negate=False, **kw)]
    return [LCase(negate=False, **kw), LCase(negate=True, **kw)]


def _leaf(t: Tape, kind: str, width: int, var_index: Optional[int], const: Optional[int]) -> int:
    """Operand forms: "v" variable, "k" / "K" constant, "c" BXOR(var, const), "a" ADD(var, const)."""
    if kind == "v":
        return t.var(var_index, width)
    if kind == "c":
        return t.bxor(t.var(var_index, width), t.const(xor_const(width), width))
    if kind == "a":
        return t.add(t.var(var_index, width), t.const(xor_const(width), width))
    return t.const(const, width)


def _planted(kind: str, width: int, vals: Sequence[int]) -> List[int]:
    """The variable values that make an operand of form ``kind`` take ``vals``."""
    if kind == "c":
        return [v ^ xor_const(width) for v in vals]
    if kind == "a":
        return [(v - xor_const(width)) & mask(width) for v in vals]
    return list(vals)


def _queries(name: str, widths: Sequence[int], n: int, fixed: Optional[Tuple[int, ...]] = None) -> List[Tuple[int, ...]]:
    rng = random.Random("query/" + name)
    out = []
    for m in range(n):
        if fixed is not None:
            out.append(fixed)
        elif len(widths) == 2 and m % N_SCEN == 5:       # (arity 2, absent: small arguments, so a swapped entry fits both widths)
            out.append(tuple(rng.getrandbits(min(widths)) for _ in widths))
        else:
            out.append(tuple(rng.getrandbits(w) | (1 << (w - 1) if m % 3 == 0 else 0) for w in widths))
    return out


# ---------------------------------------------------------------- group 1: uf1
UF1_SIGS = ((1, 8), (8, 256), (8, 0), (32, 1), (33, 33), (64, 32), (160, 256), (160, 64), (256, 256), (256, 8), (256, 0), (256, 160))
UF1_WIDE_SIGS = ((257, 256), (512, 256), (1088, 256), (2048, 256), (256, 512), (256, 1088), (256, 2048))
UF1_FULL_FORMS = ((256, 256), (256, 8), (256, 0), (33, 33))     # these signatures take every key operand form


def _uf1_cases(kw: int, rw: int, tab: Table, queries, form: str, place: str, fixed=None) -> List[LCase]:
    keys = [q[0] for q in queries]
    if form == "a":     # the sum before it is masked to the key width, for the fault that compares those bits
        c = xor_const(kw)
        raws = [((k - c) & mask(kw)) + c for k in keys]
    specs = [] if form in "kK" else [(kw, _planted(form, kw, keys))]

    def value(m, sem):
        return sem.lookup(tab, m, queries[m], (raws[m],) if form == "a" else None)

    def term(t, vi, fi):
        return t.uf(fi[0], rw, _leaf(t, form, kw, vi[0] if specs else None, fixed))

    def info(m):
        return f"key={keys[m]:#x} table {sorted(table_labels(tab, m, queries[m]))} of {tab.name} else={tab.elses[m]:#x}"

    return _with_not(group="uf1", sig=f"{kw}->{rw}", form=form, place=place, rw=rw, value=value, var_specs=specs, tables=[tab],
                     term=term, info=info, queries=list(queries))


def _small_const(kw: int) -> int:
    return 0xA5C3 & mask(min(kw, 16)) or 1


def _wide_const(kw: int) -> int:
    return xor_const(kw) | (1 << (kw - 1))


@functools.lru_cache(maxsize=None)
def uf1_cases() -> Tuple[LCase, ...]:
    out: List[LCase] = []
    for kw, rw in UF1_SIGS + UF1_WIDE_SIGS:
        narrow = kw <= 256 and rw <= 256
        sig = f"{kw}->{rw}"
        q = _queries(sig, (kw,), M)
        spec = FuncSpec(1, rw, (kw,))
        tabs = [make_table(f"uf1 {sig} csr", spec, COUNTS_CSR, q)]
        if narrow:
            tabs.append(make_table(f"uf1 {sig} dense", spec, COUNTS_DENSE, q, dense=True))
        for tab in tabs:
            out += _uf1_cases(kw, rw, tab, q, "v", "hi")
            if (kw, rw) in UF1_FULL_FORMS:
                out += _uf1_cases(kw, rw, tab, q, "c", "hi")
                out += _uf1_cases(kw, rw, tab, q, "v", "lo")
                if kw % 32:
                    out += _uf1_cases(kw, rw, tab, q, "a", "hi")
        if (kw, rw) in UF1_FULL_FORMS:
            for form, const, dense in (("k", _small_const(kw), True), ("K", _wide_const(kw), False)):
                if form == "K" and kw <= 16:
                    continue
                qc = _queries(sig, (kw,), M, (const,))
                tab = make_table(f"uf1 {sig} key {form}", spec, COUNTS_DENSE if dense else COUNTS_CSR, qc, dense=dense)
                out += _uf1_cases(kw, rw, tab, qc, form, "hi", const)
    # entry counts across the wave: all 64 lanes different (0 .. 63), and all equal
    q = _queries("ragged", (256,), M)
    spec = FuncSpec(1, 256, (256,))
    for name, count_of, dense in (("all counts differ", lambda m: (m * 27 + m // 64) % 64, False), ("all counts 9", lambda m: 9, True)):
        tab = make_table("uf1 256->256 " + name, spec, (), q, dense=dense, count_of=count_of)
        for c in _uf1_cases(256, 256, tab, q, "v", "hi"):
            c.sig = "256->256 " + name
            out.append(c)
    return tuple(out)


# ---------------------------------------------------------------- group 2: uf2
UF2_SIGS = ((256, 256, 256), (160, 8, 72), (8, 256, 0), (33, 64, 160))
COUNTS_UF2 = (0, 1, 2, 7, 8, 9, 17)


@functools.lru_cache(maxsize=None)
def uf2_cases() -> Tuple[LCase, ...]:
    out: List[LCase] = []
    for w0, w1, rw in UF2_SIGS:
        sig = f"({w0},{w1})->{rw}"
        q = _queries(sig, (w0, w1), M)
        tab = make_table("uf2 " + sig, FuncSpec(2, rw, (w0, w1)), COUNTS_UF2, q)
        for form, place in (("vv", "hi"), ("cv", "hi"), ("vc", "hi"), ("vv", "lo")):
            specs = [(w, _planted(f, w, [k[i] for k in q])) for i, (f, w) in enumerate(zip(form, (w0, w1)))]

            def value(m, sem, tab=tab, q=q):
                return sem.lookup(tab, m, q[m])

            def term(t, vi, fi, form=form, w0=w0, w1=w1, rw=rw):
                return t.uf(fi[0], rw, _leaf(t, form[0], w0, vi[0], None), _leaf(t, form[1], w1, vi[1], None))

            def info(m, tab=tab, q=q):
                return f"args=({q[m][0]:#x}, {q[m][1]:#x}) table {sorted(table_labels(tab, m, q[m]))} else={tab.elses[m]:#x}"

            out += _with_not(group="uf2", sig=sig, form=form, place=place, rw=rw, value=value, var_specs=specs, tables=[tab],
                             term=term, info=info, queries=q)
    return tuple(out)


# ---------------------------------------------------------------- group 3: array
ARRAY_SIGS = ((256, 8), (256, 256), (160, 256), (8, 33), (256, 0))
ARRAY_DEPTHS = (0, 1, 2, 5)
N_ARRAY_CLASS = 7
ARRAY_CLASSES = ("outermost", "inner-only", "two-or-more", "none-base-hit", "none-base-else", "near-miss", "all")


def _array_case(iw: int, rw: int, base: str, depth: int, rot: int) -> List[LCase]:
    """SELECT(chain, idx): ``depth`` stores over ARRAY_VAR ("var") or CONST_ARRAY ("const").  Level i
    (0 = outermost) takes its index and value as variable / constant / computed term by (i + rot) % 3."""
    sig = f"{iw}->{rw} {base} depth {depth}"
    rng = random.Random("array/" + sig)
    L = limbs(iw)
    iform = ["vkc"[(i + rot) % 3] for i in range(depth)]
    vform = ["vck"[(i + rot) % 3] for i in range(depth)]
    vw = max(rw, 1)
    ic = [rng.getrandbits(iw) | 1 for _ in range(depth)]            # the constants of "k" index levels
    kval = differ(rng, rw)                                          # CONST_ARRAY's value; the stored constants differ from
    vc = [kval] * (depth + 1)                                       # it (innermost) and from the level below
    for i in reversed(range(depth)):
        vc[i] = differ(rng, rw, vc[i + 1])
    idxs, sidx, sval, cls = [], [], [], []
    for m in range(M):
        c, j = m % N_ARRAY_CLASS, m // (2 * N_ARRAY_CLASS)
        want = {0: {0}, 1: {depth - 1 if j % 2 == 0 else max(1, depth // 2)}, 2: {0, depth - 1} | ({2} if j % 2 else set()),
                6: set(range(depth))}.get(c, set())
        want = {i for i in want if 0 <= i < depth}
        if c == 1 and depth < 2:
            want = set()
        consts = [i for i in sorted(want) if iform[i] == "k"]
        idx = ic[consts[0]] if consts else rng.getrandbits(iw) | (1 << (iw - 1) if m % 3 == 0 else 0)
        row_i, row_v = [], []
        prev_vals: List[int] = []
        for i in range(depth):
            if iform[i] == "k":
                si = ic[i]
            elif i in want:
                si = idx
            elif c == 5:        # one bit of limb (j + i) % L differs
                lim = (j + i) % L
                si = idx ^ (1 << (32 * lim + rng.randrange(min(32, iw - 32 * lim))))
            else:
                si = rng.getrandbits(iw)
                si ^= 1 if si == idx else 0
            sv = vc[i] if vform[i] == "k" else differ(rng, rw, *prev_vals[-2:]) if rw > 1 else rng.getrandbits(1)
            prev_vals.append(sv)
            row_i.append(si)
            row_v.append(sv)
        idxs.append(idx)
        sidx.append(row_i)
        sval.append(row_v)
        hit = [i for i in range(depth) if row_i[i] == idx]
        cls.append(ARRAY_CLASSES[c] + f" (levels {hit})")
    tab = None
    kvals = [differ(rng, rw, kval) if rw > 1 else rng.getrandbits(1) for _ in range(M)]      # CONST_ARRAY of a variable, every other tape
    kvar = base == "const" and depth % 2 == 0
    if base == "var":
        scen = lambda m: (4, 5, 0, 10, 7, 6, 8)[(m // N_ARRAY_CLASS) % 7] if m % N_ARRAY_CLASS not in (3, 4) else (  # noqa: E731
            (4, 2, 7, 11, 12)[(m // N_ARRAY_CLASS) % 5] if m % N_ARRAY_CLASS == 3 else (5, 6)[(m // N_ARRAY_CLASS) % 2])
        dense = depth in (0, 2)
        tab = make_table("array " + sig, FuncSpec(1, rw, (iw,)), COUNTS_DENSE if dense else COUNTS_CSR, [(i,) for i in idxs],
                         dense=dense, scen_of=scen)
    specs: List[Tuple[int, List[int]]] = [(iw, idxs)]
    slot: Dict[Tuple[str, int], int] = {}
    for i in range(depth):
        if iform[i] != "k":
            slot[("i", i)] = len(specs)
            specs.append((iw, _planted(iform[i], iw, [r[i] for r in sidx])))
        if vform[i] != "k":
            slot[("v", i)] = len(specs)
            vals = [r[i] for r in sval]
            # a Bool value has no BXOR: its computed form is NOT(var)
            specs.append((rw, [1 - v for v in vals] if rw == 0 and vform[i] == "c" else _planted(vform[i], vw, vals) if rw else vals))
    if kvar:
        slot[("k", 0)] = len(specs)
        specs.append((rw, kvals))

    def chain(m):
        t = ("var", tab.entries[m], tab.elses[m]) if tab is not None else ("const", kvals[m] if kvar else kval)
        for i in reversed(range(depth)):
            t = ("store", t, sidx[m][i], sval[m][i])
        return t

    def value(m, sem):
        return sem.select(chain(m), idxs[m], tab, m)

    def term(t, vi, fi):
        def val_leaf(kind, s, const):
            if rw:
                return _leaf(t, kind, rw, vi[s] if s is not None else None, const)
            if kind == "k":
                return t.true() if const else t.false()
            return t.not_(t.var(vi[s], 0)) if kind == "c" else t.var(vi[s], 0)
        if tab is not None:
            a = t.array_var(fi[0], rw)
        else:
            a = t.const_array(val_leaf("v" if kvar else "k", slot.get(("k", 0)), kval))
        for i in reversed(range(depth)):
            a = t.store(a, _leaf(t, iform[i], iw, vi[slot[("i", i)]] if ("i", i) in slot else None, ic[i]),
                        val_leaf(vform[i], slot.get(("v", i)), vc[i]))
        return t.select(a, t.var(vi[0], iw))

    def info(m):
        s = f"idx={idxs[m]:#x} class {cls[m]} stores (outermost first) " + ", ".join(f"[{i:#x}]={v:#x}" for i, v in zip(sidx[m], sval[m]))
        if tab is not None:
            s += f" base table {sorted(table_labels(tab, m, (idxs[m],)))} else={tab.elses[m]:#x}"
        return s

    cases = _with_not(group="array", sig=sig, form="".join(iform) + "/" + "".join(vform), place="hi", rw=rw, value=value, var_specs=specs,
                      tables=[tab] if tab is not None else [], term=term, info=info, depth=depth, queries=[(i,) for i in idxs])
    for c in cases:
        c.classes = cls
    return cases


@functools.lru_cache(maxsize=None)
def array_cases() -> Tuple[LCase, ...]:
    out: List[LCase] = []
    for s, (iw, rw) in enumerate(ARRAY_SIGS):
        for b, base in enumerate(("var", "const")):
            for depth in ARRAY_DEPTHS:
                out += _array_case(iw, rw, base, depth, s + b)
    return tuple(out)


# ---------------------------------------------------------------- group 4: widekey
WIDE_SIGS = ((2080, 256), (2304, 256), (2560, 256), (4096, 256), (2080, 64), (4096, 64))


def _wide_entries(rng, kw: int, rw: int, n: int, scen: int, j: int, q: int, hv: int, dv: int):
    nch = (kw + 255) // 256
    last_bits = kw - 256 * (nch - 1)

    def near(kind):     # differs from the key in chunk 0 / a middle chunk / one bit of the last chunk only
        if kind == 0:
            return q ^ (rng.getrandbits(256) | 1)
        if kind == 1:
            ch = 1 + rng.randrange(nch - 2)
            return q ^ ((rng.getrandbits(256) | 1) << (256 * ch))
        return q ^ (1 << (256 * (nch - 1) + rng.randrange(last_bits)))

    ent = [((rng.getrandbits(kw) | 1 << 5,), differ(rng, rw, hv)) for _ in range(n)]
    ent = [(k if k != (q,) else (q ^ 2,), v) for k, v in ent]

    def put(slot, key, val=None):
        if 0 <= slot < n:
            ent[slot] = ((key,), differ(rng, rw, hv) if val is None else val)

    if n == 0:
        return ent
    if scen <= 3:
        put(min((0, 31, 32, 63)[scen], n - 1), q, hv)
    elif scen == 4:
        for s in range(n):
            put(s, near((s + j) % 3))
    elif scen == 5:
        for s in range(max(0, n - 4), n - 1):
            put(s, near((s + j) % 3))
        put(n - 1, q, hv)
    elif scen == 6:         # entries that survive every chunk but the last, then the match
        for s in range(n - 1):
            if s % 2 == 0 or s >= n - 4:
                put(s, near(2))
        put(n - 1, q, hv)
    elif scen == 7:
        put(n - 1, q, dv)
        put((0, n // 2)[j % 2] if n > 1 else 0, q, hv)
    return ent


def wide_labels(tab: Table, m: int, q: int) -> set:
    kw = tab.spec.arg_widths[0]
    nch = (kw + 255) // 256
    ent = tab.entries[m]
    hits = [i for i, (k, _) in enumerate(ent) if k[0] == q]
    h = hits[0] if hits else len(ent)
    out = {f"n={len(ent)}", f"hit@{h}" if hits else "absent"}
    if len(hits) > 1 and ent[hits[1]][1] != ent[h][1]:
        out.add("dup")
    last = 0
    for k, _ in ent[:h]:
        d = k[0] ^ q
        chunks = [c for c in range(nch) if (d >> (256 * c)) & mask(256)]
        if chunks == [0]:
            out.add("chunk0-only")
        elif len(chunks) == 1 and chunks[0] < nch - 1:
            out.add("middle-chunk-only")
        elif chunks == [nch - 1]:
            last += 1
            if bin(d).count("1") == 1:
                out.add("last-chunk-one-bit")
    if last >= 2:
        out.add("several-survive-to-last")
    return out


@functools.lru_cache(maxsize=None)
def widekey_cases() -> Tuple[LCase, ...]:
    out: List[LCase] = []
    for kw, rw in WIDE_SIGS:
        sig = f"{kw}->{rw}"
        rng = random.Random("wide/" + sig)
        nch = (kw + 255) // 256
        cw = [min(256, kw - 256 * c) for c in range(nch)]
        keys = [rng.getrandbits(kw) | (1 << (kw - 1)) for _ in range(M)]
        entries, elses = [], []
        prev = 0
        for m in range(M):
            els = differ(rng, rw, prev)
            hv = differ(rng, rw, els, prev)
            dv = differ(rng, rw, hv, els)
            entries.append(_wide_entries(rng, kw, rw, COUNTS_WIDE[m % len(COUNTS_WIDE)], m % N_SCEN_WIDE, m // 2, keys[m], hv, dv))
            elses.append(els)
            prev = els
        tab = Table("widekey " + sig, FuncSpec(1, rw, (kw,)), entries, elses, False, tuple(sorted(set(COUNTS_WIDE))))
        # chunk c as a variable, or (every third) a computed term
        forms = ["c" if c % 3 == 1 else "v" for c in range(nch)]
        specs = [(cw[c], _planted(forms[c], cw[c], [(k >> (256 * c)) & mask(cw[c]) for k in keys])) for c in range(nch)]

        def value(m, sem, tab=tab, keys=keys):
            return sem.wide(tab, m, (keys[m],))

        def term(t, vi, fi, forms=forms, cw=cw, rw=rw):
            return t.uf_wide(fi[0], rw, [_leaf(t, forms[c], cw[c], vi[c], None) for c in range(len(cw))])

        def info(m, tab=tab, keys=keys):
            return f"key={keys[m]:#x} table {sorted(wide_labels(tab, m, keys[m]))} else={tab.elses[m]:#x}"

        out += _with_not(group="widekey", sig=sig, form="".join(forms), place="hi", rw=rw, value=value, var_specs=specs, tables=[tab],
                         term=term, info=info, queries=[(k,) for k in keys])
    return tuple(out)


# ---------------------------------------------------------------- group 5: keccak
KECCAK_BYTES = tuple(range(1, 65)) + (65, 96, 127, 128, 135, 136, 137, 200, 255, 256)
KECCAK_INPUTS = ("zero", "ones", "bit-in-first-byte", "bit-in-last-byte", "random")


def keccak_inputs(width: int, n: int, seed: str) -> Tuple[List[int], List[str]]:
    rng = random.Random("keccak/" + seed)
    vals, cls = [], []
    for m in range(n):
        c, j = m % 5, m // 10
        v = (0, mask(width), 1 << (width - 8 + j % 8), 1 << (j % 8), rng.getrandbits(width))[c]
        vals.append(v)
        cls.append(KECCAK_INPUTS[c])
    return vals, cls


@functools.lru_cache(maxsize=None)
def keccak_cases() -> Tuple[LCase, ...]:
    out = []
    for wi, nb in enumerate(KECCAK_BYTES):
        w = 8 * nb
        vals, cls = keccak_inputs(w, M_KECCAK, str(nb))

        def value(m, sem, vals=vals, w=w):
            return sem.keccak(vals[m], w)

        c = LCase.__new__(LCase)
        # (set before __post_init__ runs) stride 37: a width's 75 flips touch every limb; width i goes on where
        # width i - 1 stopped, so the group flips every digest bit
        c.flip_shift, c.flip_step = 75 * wi, 37
        LCase.__init__(c, group="keccak", sig=f"{nb} bytes", form="v", place="hi", negate=False, rw=256, value=value,
                       var_specs=[(w, vals)], tables=[], term=lambda t, vi, fi, w=w: t.keccak(t.var(vi[0], w)),
                       info=lambda m, vals=vals, cls=cls: f"input ({cls[m]}) {vals[m]:#x}", n_models=M_KECCAK, kw=w)
        out.append(c)
    return tuple(out)


# ---------------------------------------------------------------- group 6: keccak columns
KECCAK_COLUMN_BITS = (256, 512, 544, 768, 1056, 1088, 2048)


@dataclass
class ColumnWorkload:
    """Hoisted ``Keccak256(Concat(...)) == R`` roots: three roots a message (R, R2 planted with
    different flips, and a negation), so that each message is shared and hoists."""
    roots: list
    models: list                  # smt_model.Model per model
    expect: np.ndarray            # bool[n_roots, M_KECCAK]
    cases: List[LCase]            # one per root, for the fault models and failure messages
    n_messages: int


@functools.lru_cache(maxsize=None)
def keccak_column_workload() -> ColumnWorkload:
    from mythril_amd import smt as S
    from mythril_amd.smt_model import Model
    n = M_KECCAK
    assign: List[Dict[str, int]] = [{} for _ in range(n)]
    roots, cases = [], []
    for mi, bits in enumerate(KECCAK_COLUMN_BITS):
        # the message: 256-bit words (variables, every third a constant), a 32-bit selector where the width asks for one
        parts, widths, names = [], [], []
        rest, k = bits, 0
        while rest:
            w = 32 if rest % 256 else 256
            nm = f"m{mi}p{k}"
            const = k % 3 == 2 and rest != bits
            parts.append(S.BitVecVal(xor_const(w) >> 3, w) if const else S.BitVecSym(nm, w))
            widths.append(w)
            names.append(None if const else nm)
            rest -= w
            k += 1
        msg = S.Concat(*parts) if len(parts) > 1 else parts[0]
        vals, cls = keccak_inputs(bits, n, f"col{bits}")
        # constant parts overwrite the class value at their position
        full = []
        for m in range(n):
            v, sh = 0, bits
            for p, w, nm in zip(parts, widths, names):
                sh -= w
                piece = (vals[m] >> sh) & mask(w) if nm else xor_const(w) >> 3
                if nm:
                    assign[m][nm] = piece
                v |= piece << sh
            full.append(v)
        h = S.Keccak256(msg)
        for r, (shift, neg) in enumerate(((0, False), (101, False), (53, True))):
            rn = f"r{mi}_{r}"

            def value(m, sem, full=full, bits=bits):
                return sem.keccak(full[m], bits)

            c = LCase.__new__(LCase)
            c.flip_shift, c.flip_step = shift + 29 * mi, 37
            LCase.__init__(c, group="keccak_columns", sig=f"{bits} bits", form="concat", place="hi", negate=False, rw=256, value=value,
                           var_specs=[], tables=[], term=None, info=lambda m, full=full, cls=cls: f"message ({cls[m]}) {full[m]:#x}",
                           n_models=n, kw=bits)
            if neg:     # NOT(h == R): the expectation and the fault verdicts invert
                c.expect = ~c.expect
                c.negate_eq = True
            for m in range(n):
                assign[m][rn] = c.rs[m]
            e = h == S.BitVecSym(rn, 256)
            roots.append(S.Not(e) if neg else e)
            cases.append(c)
    models = [Model(a) for a in assign]
    return ColumnWorkload(roots, models, np.array([c.expect for c in cases]), cases, len(KECCAK_COLUMN_BITS))


# ---------------------------------------------------------------- group 7: bool
BOOL_OPS = ("NOT", "AND", "OR", "XOR", "IMPLIES", "IFF", "BITE")
BOOL_FORMS = ("vvv", "vTv", "Fvv", "ccc", "cvv", "vcT")       # per operand: variable, TRUE, FALSE, computed ULT(x, y)


@functools.lru_cache(maxsize=None)
def bool_cases() -> Tuple[LCase, ...]:
    out: List[LCase] = []
    rng = random.Random("bool")
    for op in BOOL_OPS:
        arity = {"NOT": 1, "BITE": 3}.get(op, 2)
        for form in sorted({f[:arity] for f in BOOL_FORMS}):
            for place in ("hi", "lo"):
                if place == "lo" and "c" in form and arity == 3 and form.count("c") > 1:
                    continue        # (more than 8 variables)
                bits = [[(m >> i) & 1 if f in "vc" else int(f == "T") for m in range(M)] for i, f in enumerate(form)]
                specs: List[Tuple[int, List[int]]] = []
                slots = []
                for i, f in enumerate(form):
                    slots.append(len(specs))
                    if f == "v":
                        specs.append((0, bits[i]))
                    elif f == "c":      # ULT(x, y): x, y differ in one random bit, ordered by the wanted truth value
                        xs, ys = [], []
                        for m in range(M):
                            a = rng.getrandbits(256)
                            b = a ^ (1 << rng.randrange(256)) if m % 5 else a
                            lo, hi = min(a, b), max(a, b)
                            if bits[i][m]:
                                lo, hi = (lo, hi) if lo != hi else (lo & ~1, lo | 1)
                                xs.append(lo), ys.append(hi)
                            else:
                                xs.append(hi), ys.append(lo)
                        specs += [(256, xs), (256, ys)]

                def value(m, sem, op=op, bits=bits):
                    return sem.boolean(op, *(b[m] for b in bits))

                def term(t, vi, fi, op=op, form=form, slots=slots):
                    xs = []
                    for f, s in zip(form, slots):
                        xs.append(t.var(vi[s], 0) if f == "v" else t.true() if f == "T" else t.false() if f == "F"
                                  else t.ult(t.var(vi[s], 256), t.var(vi[s + 1], 256)))
                    return {"NOT": t.not_, "AND": t.and_, "OR": t.or_, "XOR": t.xor, "IMPLIES": t.implies, "IFF": t.iff, "BITE": t.bite}[op](*xs)

                out += _with_not(group="bool", sig=op, form=form, place=place, rw=0, value=value, var_specs=specs, tables=[],
                                 term=term, info=lambda m, bits=bits: "operands " + ", ".join(str(b[m]) for b in bits))
    return tuple(out)


# ---------------------------------------------------------------- groups and packs
def group_cases(group: str) -> Tuple[LCase, ...]:
    return {"uf1": uf1_cases, "uf2": uf2_cases, "array": array_cases, "widekey": widekey_cases, "keccak": keccak_cases,
            "bool": bool_cases}[group]()


def constant_tapes(group: str) -> List[str]:
    """Bool tapes that have one outcome in every model by construction: connectives whose operands
    are all TRUE / FALSE do not exist in the grid, but some with one constant operand are constant."""
    out = []
    for c in group_cases(group) if group == "bool" else ():
        vals = {ref_bool(c.sig, *(((a >> i) & 1) if f in "vc" else int(f == "T") for i, f in enumerate(c.form))) for a in range(8)}
        if len(vals) == 1:
            out.append(c.name())
    return out


@dataclass
class Pack:
    """Cases that share one model batch and one tape batch (tape i = cases[i])."""
    cases: List[LCase]
    tapes: TapeBatch
    models: ModelBatch
    tables: List[Table]

    @property
    def expect(self) -> np.ndarray:
        return np.array([c.expect for c in self.cases])


def _make_pack(cases: List[LCase], first_index: int) -> Pack:
    n = cases[0].n_models
    order = []      # variables of at most 256 bits first (G addresses rows with 16 bits)
    for ci, c in enumerate(cases):
        order += [(c.var_specs[k][0] > 256, ci, k) for k in range(len(c.var_specs))]
    order.sort()
    widths = [256] * first_index
    rows = [np.zeros((8 * first_index, n), np.uint32)] if first_index else []
    index: Dict[Tuple[int, int], int] = {}
    for _, ci, k in order:
        width, vals = cases[ci].var_specs[k]
        index[(ci, k)] = len(widths)
        widths.append(width)
        rows.append(_rows(max(width, 1), vals))
    tables: List[Table] = []
    for c in cases:
        for tab in c.tables:
            if not any(tab is t for t in tables):
                tables.append(tab)
    fid = {id(t): f for f, t in enumerate(tables)}
    tapes = [c.build([index[(ci, k)] for k in range(len(c.var_specs))], [fid[id(t)] for t in c.tables]) for ci, c in enumerate(cases)]
    funcs, ptr, ew, eb, lw, lb = tables_arrays(tables, n)
    return Pack(cases, TapeBatch(tapes), ModelBatch(widths, np.vstack(rows), funcs, ptr, ew, eb, lw, lb), tables)


def packs_of(cases: Sequence[LCase]) -> List[Pack]:
    """One pack of the "hi" cases (variables from index 8 up) and packs of at most 8 variables of
    the "lo" ones."""
    out = []
    hi = [c for c in cases if c.place == "hi"]
    if hi:
        out.append(_make_pack(hi, N_PRELOADED))
    cur: List[LCase] = []
    n = 0
    for c in (c for c in cases if c.place == "lo"):
        if cur and n + len(c.var_specs) > N_PRELOADED:
            out.append(_make_pack(cur, 0))
            cur, n = [], 0
        cur.append(c)
        n += len(c.var_specs)
    if cur:
        out.append(_make_pack(cur, 0))
    return out


@functools.lru_cache(maxsize=None)
def group_packs(group: str) -> Tuple[Pack, ...]:
    return tuple(packs_of(group_cases(group)))
