"""Planted-result workload: value-exact parity cases per op, width and operand form (test helper).

Every GPU parity test compares Bool verdicts, and a verdict shows a wrong value inside a tape
only when the root flips because of it.  Here every case is ONE operation whose per-model result
is planted into the model batch, so that any wrong result bit in any model flips a verdict:

* value ops: the tape is ``EQ(op(A, B), R)``; model variable R holds :func:`ref` of that model's
  operands in even models and the same with exactly one bit flipped in odd ones (expected
  verdict: true / false).  The flipped bit cycles with the model index over every bit of the
  result (results wider than 256 bits: bits 32k-1 and 32k of every limb, bit 0 and the top bit);
* predicates: ``pred(A, B)`` and ``NOT(pred(A, B))`` as roots, expected verdict from :func:`ref`.

:func:`ref` is the ground truth: plain Python integers, written from the SMT-LIB
FixedSizeBitVectors definitions (plus the three multiplication-overflow predicates of mq.h); it
shares no code with the oracles, which the grid therefore checks as well.

An operand is a model variable ("v"), a constant of at most 16 bits ("k"), a wider constant
("K") or a computed sub-term ("c": ``BXOR(var, const)`` with the variable planted so that the
sub-term has the wanted value) - the operand forms the assembly translator (qsa_translate.cpp
qsa_translate) picks different handlers for.  Every case whose widest value has 256 bits, and
every narrower case at operand widths 33 and 160, exists twice: with its variables at indices below
8 (the P kernel's preloaded set, ``place == "lo"``; 8 variables a batch, so these come in many small
batches) and from index 8 up (``"hi"``: the G kernel).

M = 577 models: nine full waves and a ragged one; 2 x 256 models are needed to flip every bit of a
256-bit result once.  Operand classes cycle with the model index, 7 classes (coprime to 2) so that
every class meets flipped and unflipped models; the class parameter (limb index, sign
combination, ...) advances every 14 models, i.e. once per (unflipped, flipped) pair.
"""
from __future__ import annotations

import functools
import hashlib
import random
from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from mythril_amd.models import ModelBatch
from mythril_amd.tape import Op, Tape, TapeBatch, limbs

M = 577
NCLASS = 7
M32 = 0xFFFFFFFF

WIDTHS = (1, 8, 31, 32, 33, 64, 160, 255, 256, 257, 512)
WIDE_WIDTHS = (544, 1088, 2048)          # not for multiplication, division, overflow predicates (mq.h)
LO_WIDTHS = (33, 160, 256)               # widths whose cases also exist on preloaded variables
MAX_WIDTH = 2048

MULDIV = frozenset({Op.MUL, Op.UDIV, Op.UREM, Op.SDIV, Op.SREM, Op.SMOD,
                    Op.UMUL_NOOVFL, Op.SMUL_NOOVFL, Op.SMUL_NOUDFL})
PREDICATES = (Op.EQ, Op.ULT, Op.ULE, Op.SLT, Op.SLE, Op.UMUL_NOOVFL, Op.SMUL_NOOVFL, Op.SMUL_NOUDFL)
UNARY = (Op.NEG, Op.BNOT, Op.EXTRACT, Op.ZEXT, Op.SEXT)
SHIFTS = (Op.SHL, Op.LSHR, Op.ASHR)
DIVS = (Op.UDIV, Op.UREM, Op.SDIV, Op.SREM, Op.SMOD)
SIGNED_DIVS = (Op.SDIV, Op.SREM, Op.SMOD)
OVERFLOW = (Op.UMUL_NOOVFL, Op.SMUL_NOOVFL, Op.SMUL_NOUDFL)

GROUPS: Dict[str, Tuple[Op, ...]] = {
    "addsub": (Op.ADD, Op.SUB, Op.NEG, Op.BAND, Op.BOR, Op.BXOR, Op.BNOT),
    "mul": (Op.MUL,) + OVERFLOW,
    "udiv": (Op.UDIV, Op.UREM),
    "sdiv": SIGNED_DIVS,
    "shift": SHIFTS,
    "width": (Op.EXTRACT, Op.CONCAT, Op.ZEXT, Op.SEXT, Op.ITE),
    "cmp": (Op.EQ, Op.ULT, Op.ULE, Op.SLT, Op.SLE),
}
# ("cK": the only form in which P runs a commutative op's constant handler - ADDC, MULC, ... - since
# the tape compiler moves a constant next to a variable to the left, which is ADDCV's shape)
BINARY_FORMS = ("vv", "vk", "vK", "kv", "Kv", "cc", "cv", "cK")
UNARY_FORMS = ("v", "c")


# ---------------------------------------------------------------- reference semantics
def mask(w: int) -> int:
    return (1 << w) - 1


def to_signed(x: int, w: int) -> int:
    """The two's-complement integer bv2int of SMT-LIB's signed operators."""
    return x - (1 << w) if x >> (w - 1) else x


def result_width(op: Op, w: int, imm=None) -> int:
    if op in PREDICATES:
        return 0
    if op == Op.EXTRACT:
        return imm[0] - imm[1] + 1
    if op in (Op.CONCAT, Op.ZEXT, Op.SEXT):
        return w + imm
    return w


def ref(op: Op, w: int, x: int, y: Optional[int] = None, imm=None) -> int:
    """SMT-LIB FixedSizeBitVectors value of ``op`` on operands of ``w`` bits (predicates: 0 / 1).

    imm: EXTRACT (hi, lo); ZEXT / SEXT the k added bits; CONCAT the width of the low operand y
    (x is the high one, w bits); ITE the condition (x if imm else y)."""
    m = mask(w)
    if op == Op.ADD:
        return (x + y) & m
    if op == Op.SUB:
        return (x - y) & m
    if op == Op.MUL:
        return (x * y) & m
    if op == Op.NEG:
        return (-x) & m
    if op == Op.UDIV:                       # bvudiv s 0 = all ones
        return m if y == 0 else x // y
    if op == Op.UREM:                       # bvurem s 0 = s
        return x if y == 0 else x % y
    if op in SIGNED_DIVS:
        sx, sy = to_signed(x, w), to_signed(y, w)
        if op == Op.SDIV:                   # truncated quotient; by 0: -1 for s >= 0, else 1
            if sy == 0:
                return 1 if sx < 0 else m
            q = abs(sx) // abs(sy)
            return (-q if (sx < 0) != (sy < 0) else q) & m
        if op == Op.SREM:                   # sign follows the dividend; by 0: s
            if sy == 0:
                return x
            r = abs(sx) % abs(sy)
            return (-r if sx < 0 else r) & m
        if sy == 0:                         # bvsmod: sign follows the divisor; by 0: s
            return x
        return (sx % sy) & m                # Python's % is the floored modulo
    if op == Op.BAND:
        return x & y
    if op == Op.BOR:
        return x | y
    if op == Op.BXOR:
        return x ^ y
    if op == Op.BNOT:
        return ~x & m
    if op == Op.SHL:
        return 0 if y >= w else (x << y) & m
    if op == Op.LSHR:
        return 0 if y >= w else x >> y
    if op == Op.ASHR:
        return (to_signed(x, w) >> min(y, w)) & m
    if op == Op.EXTRACT:
        hi, lo = imm
        return (x >> lo) & mask(hi - lo + 1)
    if op == Op.CONCAT:
        return (x << imm) | y
    if op == Op.ZEXT:
        return x
    if op == Op.SEXT:
        return to_signed(x, w) & mask(w + imm)
    if op == Op.ITE:
        return x if imm else y
    if op == Op.EQ:
        return int(x == y)
    if op == Op.ULT:
        return int(x < y)
    if op == Op.ULE:
        return int(x <= y)
    if op == Op.SLT:
        return int(to_signed(x, w) < to_signed(y, w))
    if op == Op.SLE:
        return int(to_signed(x, w) <= to_signed(y, w))
    if op == Op.UMUL_NOOVFL:
        return int(x * y < (1 << w))
    p = to_signed(x, w) * to_signed(y, w)
    if op == Op.SMUL_NOOVFL:
        return int(p <= (1 << (w - 1)) - 1)
    if op == Op.SMUL_NOUDFL:
        return int(p >= -(1 << (w - 1)))
    raise ValueError(f"not a value op: {op!r}")


# ---------------------------------------------------------------- a case
@dataclass
class Case:
    op: Op
    w: int                        # operand width (CONCAT: of the high operand)
    form: str
    place: str                    # "lo": variables below index 8; "hi": from index 8 up
    imm: object
    negate: bool                  # predicates: the NOT(pred) tape
    xs: List[int]
    ys: Optional[List[int]]
    conds: Optional[List[int]]    # ITE
    rs: Optional[List[int]]       # planted R (value ops)
    expect: np.ndarray            # bool[M]
    fx: Optional[int]             # the constant operand of a "k" / "K" side
    fy: Optional[int]
    var_specs: List[Tuple[int, List[int]]]            # (width, per-model values) of the case's variables
    build: Callable[[Sequence[int]], Tape]            # variable indices -> tape

    @property
    def wy(self) -> int:
        return self.imm if self.op == Op.CONCAT else self.w

    @property
    def max_width(self) -> int:
        return max(self.w, self.wy, result_width(self.op, self.w, self.imm))

    @property
    def cell(self) -> Tuple[str, str, str]:
        return (self.op.name, self.form, self.place)

    def name(self) -> str:
        imm = "" if self.imm is None or self.op == Op.ITE else f" imm={self.imm}"
        return f"{'NOT ' if self.negate else ''}{self.op.name} w={self.w}{imm} form={self.form} place={self.place}"

    def operands(self, m: int) -> Tuple:
        return (self.xs[m], self.ys[m] if self.ys is not None else None,
                self.conds[m] if self.conds is not None else self.imm)

    def describe(self, m: int) -> str:
        """Operands and expectation of model m in hex (what a failure message carries)."""
        x, y, imm = self.operands(m)
        s = f"{self.name()} model {m}: x={x:#x}"
        if y is not None:
            s += f" y={y:#x}"
        if self.op == Op.ITE:
            s += f" cond={imm}"
        if self.rs is not None:
            s += f" op(x,y)={ref(self.op, self.w, x, y, imm):#x} planted R={self.rs[m]:#x}"
        return s + f" expected verdict {bool(self.expect[m])}"


def xor_const(w: int) -> int:
    """The constant of the computed operand form BXOR(var, const): multi-limb, no limb zero."""
    raw = b"".join(hashlib.sha256(b"planted-%d" % i).digest() for i in range((w + 255) // 256))
    return (int.from_bytes(raw, "little") | int.from_bytes(b"\x01\x00\x00\x00" * (len(raw) // 4), "little")) & mask(w)


def flip_positions(rw: int) -> List[int]:
    if rw <= 256:
        return list(range(rw))
    pos = {0, rw - 1}
    for k in range(1, limbs(rw)):
        pos.update((32 * k - 1, 32 * k))
    return sorted(pos)


# ---------------------------------------------------------------- operands per model
def _rnd_len(rng: random.Random, w: int, lo: int = 1) -> int:
    """A value of uniformly random bit length in [lo, w]."""
    n = rng.randint(min(lo, w), w)
    return rng.getrandbits(n) | (1 << (n - 1))


def _cj(m: int) -> Tuple[int, int]:
    return m % NCLASS, (m // NCLASS) // 2


def generic_pair(op, w, m, rng, fx, fy):
    """0 specials (0, 1, all ones, 2^(w-1), 2^(w-1)-1); 1 one-limb values / low limbs zero;
    2 (2^k - 1, 1): carries across every limb boundary; 3 (2^k, 1): borrows; 4, 6 equal or
    differing only in one bit of limb k, for every limb; 5 uniform / random bit lengths."""
    L, mk, MIN = limbs(w), mask(w), 1 << (w - 1)
    c, j = _cj(m)
    r = m // NCLASS
    if c == 0:
        sp = [(0, 0), (0, 1), (1, 0), (mk, mk), (mk, 1), (1, mk), (MIN, MIN - 1), (MIN - 1, MIN), (MIN, mk), (0, mk),
              (mk, 0), (MIN, MIN), (MIN - 1, MIN - 1), (MIN, 1), (MIN - 1, 1), (0, MIN), (mk, MIN), (mk, MIN - 1)]
        x, y = sp[j % len(sp)]
    elif c == 1:
        x = ((rng.getrandbits(32) | 1) << (32 * (r % L))) & mk or 1
        y = ((rng.getrandbits(32) | 1) << (32 * ((r if fx is not None else j) % L))) & mk or 1
    elif c in (2, 3):
        k = 32 * (j % L + 1)
        x = (1 << min(k, w)) - 1 if c == 2 else (1 << k) & mk
        y = 1
        if (j // L) % 2:
            x, y = y, x
    elif c in (4, 6):
        k = (j + (41 if c == 6 else 0)) % (L + 1)
        # the pair's two models (r even / odd) order the operands both ways
        base = fy if fy is not None else fx if fx is not None else rng.getrandbits(w)
        bits = [b for b in range(32 * k, min(w, 32 * k + 32))]
        want = [b for b in bits if (base >> b & 1) == r % 2] if (fx is not None or fy is not None) else []
        if k == L:
            other = base
        else:
            other = base ^ (1 << rng.choice(want or bits))
            if fx is None and fy is None:
                base, other = min(base, other), max(base, other)
        x, y = (base, other) if (fx is not None or (fy is None and r % 2)) else (other, base)
    else:
        x = rng.getrandbits(w) if j % 3 != 1 else _rnd_len(rng, w)
        y = rng.getrandbits(w) if j % 3 == 0 else _rnd_len(rng, w)
    return (x if fx is None else fx), (y if fy is None else fy)


def _with_signs(x: int, y: int, s: int, w: int) -> Tuple[int, int]:
    mk = mask(w)
    return (-x & mk if s & 1 else x), (-y & mk if s & 2 else y)


def div_pair(op, w, m, rng, fx, fy):
    """0 divisor 0 / 1 / -1, equal, one above, greater, MIN / -1; 1 power-of-two divisors;
    2 divisors of every limb count; 3 every sign combination at random lengths; 4 exact multiples
    and multiples minus one; 5 uniform; 6 divisor = dividend + {0, 1, -1, small}."""
    L, mk, MIN = limbs(w), mask(w), 1 << (w - 1)
    signed = op in SIGNED_DIVS
    c, j = _cj(m)
    R = rng.getrandbits(w)
    s = j % 4 if signed else 0
    mw = w - 1 if signed and w > 1 else w       # magnitudes that survive a sign change
    if c == 0:
        sp = [(R, 0), (R, 1), (R, mk), (MIN, mk), (R, R), (R, (R + 1) & mk), (R >> 1, R | 1), (0, 0), (MIN, 1), (mk, MIN),
              (0, R), (MIN, 0), (mk, 0), (MIN, MIN), (mk, mk), (1, mk), (MIN | 1, mk), (MIN - 1, mk), (R | MIN, 1), (R | MIN, 0)]
        x, y = sp[j % len(sp)]
    elif c == 1:
        x, y = R, 1 << ((j * 5 + j // 8) % w)
        if signed and j % 2:
            y = -y & mk
    elif c == 2:
        n = j % L + 1
        top = min(32 * n, mw)
        if top - 1 >= 32 * (n - 1):
            y = rng.getrandbits(top) | (1 << (32 * (n - 1) + rng.randrange(top - 32 * (n - 1))))
            x, y = _with_signs(rng.getrandbits(mw), y, (j // L) % 4 if signed else 0, w)
        else:                                   # only -2^(w-1) has a magnitude of n limbs
            x, y = R, MIN
    elif c == 3:
        x, y = _with_signs(_rnd_len(rng, mw), _rnd_len(rng, max(1, mw // 2)), s, w)
    elif c == 4:
        d = abs(to_signed(fy, w)) if (signed and fy is not None) else fy if fy is not None else _rnd_len(rng, max(1, mw // 2))
        d = d or 1
        q = rng.getrandbits(max(1, mw - d.bit_length()))
        x = min(q * d + (0, d - 1, 1)[j % 3], mask(mw))
        x, y = _with_signs(x, d, s, w)
    elif c == 5:
        x, y = R, rng.getrandbits(w)
    else:
        d = (0, 1, -1, rng.randrange(2, 1000))[j % 4]
        if fx is not None:
            x, y = fx, (fx + d) & mk
        else:
            y = fy if fy is not None else R
            x = (y - d) & mk
    return (x if fx is None else fx), (y if fy is None else fy)


def overflow_targets(w: int) -> List[int]:
    return [(1 << w) - 1, 1 << w, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << (w - 1)) + 1]


def overflow_pair(op, w, m, rng, fx, fy):
    """Factor pairs whose product is exactly 2^w - 1, 2^w, 2^(w-1) - 1, +-2^(w-1), -2^(w-1) - 1 and
    their neighbours (1 - 4, 6), specials (0) and random lengths adding up to about w (5)."""
    mk, MIN = mask(w), 1 << (w - 1)
    signed = op != Op.UMUL_NOOVFL
    c, j = _cj(m)
    s = j % 4 if signed else 0
    if c == 0:
        R = rng.getrandbits(w)
        sp = [(0, R), (1, mk), (mk, mk), (MIN, mk), (MIN, MIN), (1, MIN), (mk, 1), (MIN, 1), (MIN - 1, 1), (MIN - 1, 2),
              (MIN, 2), (2, MIN), (mk, 2), (MIN - 1, MIN - 1), (0, 0), (R, 1), (mk, MIN), (MIN + 1 & mk, mk), (MIN - 1, mk)]
        x, y = sp[j % len(sp)]
    elif c in (1, 2):       # 2^a * 2^(t-a) = 2^t, t = w (1) or w - 1 (2)
        t = w if c == 1 else w - 1
        a = (j * 7) % (t + 1)
        x, y = _with_signs((1 << a) & mk, (1 << (t - a)) & mk, s, w)
    elif c == 3:            # neighbours of the above
        t = w - (j // 4) % 2
        a = (j * 5) % (t + 1)
        x, y = _with_signs((1 << a) & mk, ((1 << (t - a)) + (1, -1)[j % 2]) & mk, s, w)
    elif c == 4:            # floor(target / y) and its neighbours
        d = fy if fy is not None else fx if fx is not None else _rnd_len(rng, max(1, w - 1))
        dm = abs(to_signed(d, w)) if signed else d
        t = overflow_targets(w)[j % 5]
        q = (t // dm + (0, 1, -1)[(j // 5) % 3]) & mk if dm else rng.getrandbits(w)
        if signed and fy is None and fx is None:
            q, d = _with_signs(q, d, s, w)
        elif signed and s & 1:
            q = -q & mk
        x, y = (q, d) if fx is None else (d, q)
    elif c == 5:
        a = rng.randint(1, w)
        x, y = _with_signs(_rnd_len(rng, a, a), _rnd_len(rng, max(1, w - a + (j % 3 - 1)), max(1, w - a + (j % 3 - 1))), s, w)
        x, y = x & mk, y & mk
    else:                   # (2^h - 1)(2^h + 1) = 2^(2h) - 1; 3 * ((2^t + 1) / 3); -1 * MIN; 1 * max
        h = (w - j % 2) // 2
        sp = [((1 << h) - 1, (1 << h) + 1), (1, mk), (1, MIN - 1), (mk, MIN), (mk, MIN + 1 & mk), (mk, MIN - 1)]
        for t in (w, w - 1):
            if ((1 << t) + 1) % 3 == 0:
                sp += [(3, ((1 << t) + 1) // 3), (-3 & mk, ((1 << t) + 1) // 3)]
        x, y = sp[(j // 2) % len(sp)]
        x, y = x & mk, y & mk
        if j % 4 >= 2:
            x, y = y, x
    return (x if fx is None else fx), (y if fy is None else fy)


def shift_edge_amounts(w: int) -> List[int]:
    """The edge amounts of the variable-shift parity test (tests/test_gpu_parity.py
    ``_shift_amounts``: its first models take them in order), reduced mod 2^w as there.
    test_planted_ops.py holds the two lists equal."""
    edge = [0, 1, 31, 32, 33, 63, 64, 255, 256, 257, w - 1, w, w + 1, 1 << 32, (1 << 32) + 1, 1 << 64, 1 << 255]
    return [a & mask(w) for a in edge]


def shift_pair(op, w, m, rng, fx, fy, edges):
    """0, 2, 4 the edge amounts; 1 multiples of 32; 3 uniform below w + 10; 5 high limbs set;
    6 uniform below w.  The shifted value cycles over random, all ones, MIN, 1, negative, MIN - 1."""
    L, mk, MIN = limbs(w), mask(w), 1 << (w - 1)
    c, j = _cj(m)
    xsrc = [rng.getrandbits(w), mk, MIN, 1, rng.getrandbits(w) | MIN, MIN - 1, rng.getrandbits(w) | MIN | 1]
    x = xsrc[(j + c) % len(xsrc)]
    if c in (0, 2, 4):
        y = edges[(3 * j + c // 2) % len(edges)]
    elif c == 1:
        y = 32 * (j % (L + 2))
        x = rng.getrandbits(w) | MIN | 1
    elif c == 3:
        y = rng.randrange(0, w + 10)
    elif c == 5:
        y = ((rng.getrandbits(max(1, w - 32)) | 1) << 32 | rng.randrange(w)) if w > 32 else rng.getrandbits(w)
        x = rng.getrandbits(w) | MIN | 1
    else:
        y = rng.randrange(w)
        x = rng.getrandbits(w) | MIN | 1
    return (x if fx is None else fx), (y & mk if fy is None else fy)


def unary_value(op, w, m, rng):
    """0 specials; 1 one bit set; 2 one bit clear; 3, 6 uniform; 4 random bit length; 5 low k
    limbs zero (a carry of NEG ripples through them)."""
    L, mk, MIN = limbs(w), mask(w), 1 << (w - 1)
    c, j = _cj(m)
    if c == 0:
        sp = [0, 1, mk, MIN, MIN - 1, mk // 3, mk - mk // 3, MIN | 1, mk - 1, 2 & mk]
        return sp[j % len(sp)]
    if c in (1, 2):
        bit = 1 << ((j * 37 + 31) % w)
        return bit if c == 1 else mk ^ bit
    if c == 4:
        return _rnd_len(rng, w)
    if c == 5:
        return ((rng.getrandbits(w) | 1) << (32 * (j % L))) & mk or MIN
    return rng.getrandbits(w) | (MIN if j % 2 else 0)


# ---------------------------------------------------------------- the grid
def _constants(op: Op, w: int, side: str, wide: bool) -> List[int]:
    """The constants of a "k" (at most 16 bits) or "K" (wider) operand on side "x" / "y"."""
    mk, MIN = mask(w), 1 << (w - 1)
    pat = xor_const(w) | (MIN if w > 16 else 0)
    if op in SHIFTS and side == "y":
        vals = [2 ** 32 + 1, MIN, 2 ** 64] if wide else [0, 1, 31, 32, 33, w - 1, w, w + 1, 64]
    elif op in SHIFTS:
        vals = [mk, pat] if wide else [1, 0xFFFF]
    elif op in DIVS:
        if side == "y":   # wide: two limbs, all limbs, -1, -(two limbs); small: 3, a power of two, 0, 1, 0xFFFF
            vals = [pat, pat & mask(min(w, 64)) | 1 << min(w - 1, 40), mk, -(pat & mask(min(w, 48)) | 1 << 33) & mk,
                    MIN, mk - 2] if wide else [3, 16, 0, 1, 0xFFFF]
        else:
            vals = [pat, mk, MIN] if wide else [1, 0xFFFF, 0]
    elif op in OVERFLOW:
        vals = [MIN + 1, 1 << (w // 2), pat] if wide else [2, 3, 0x100]
    elif op in (Op.SLT, Op.SLE, Op.ULT, Op.ULE, Op.EQ):
        vals = [MIN + 1, pat] if wide else [1, 0xFFFF]
    else:
        vals = [mk, pat, MIN] if wide else [1, 0xFFFF]
    out = []
    for v in vals:
        v &= mk
        if (v > 0xFFFF) == wide and v not in out:
            out.append(v)
    return out


def _extract_fields(w: int) -> List[Tuple[int, int]]:
    """(hi, lo): fields that start and end inside, at and across limb boundaries, one spanning two
    boundaries, single bits and the whole value."""
    f = [(w - 1, 0), (0, 0), (w - 1, w - 1), (w - 1, 1), (w - 2, 0), (31, 0), (32, 0), (63, 32), (40, 8), (70, 5), (95, 33),
         (64, 31), (w - 1, 32), (w - 1, 31), (w - 2, w - 34), (w - 1, w - 70), (256, 1), (w - 1, w - 256), (w - 3, w - 258)]
    return sorted({(hi, lo) for hi, lo in f if 0 <= lo <= hi < w})


def _ext_amounts(w: int) -> List[int]:
    ks = {1, 32, 33, 256 - w, 257 - w, 2048 - w, 32 * limbs(w) - w, 32 * limbs(w) - w + 1}
    return sorted(k for k in ks if k >= 1 and w + k <= MAX_WIDTH)


def _concat_low_widths(w: int) -> List[int]:
    ks = {1, 31, 32, 33, 256 - w, 2048 - w}
    return sorted(k for k in ks if k >= 1 and w + k <= MAX_WIDTH)


def _leaf(t: Tape, kind: str, width: int, var_index: Optional[int], const: Optional[int]) -> int:
    if kind == "v":
        return t.var(var_index, width)
    if kind == "c":
        return t.bxor(t.var(var_index, width), t.const(xor_const(width), width))
    return t.const(const, width)


def make_case(op: Op, w: int, form: str, place: str, imm=None, fx=None, fy=None, negate=False) -> Case:
    rng = random.Random(f"{op.name}/{w}/{form}/{imm}/{fx}/{fy}")
    unary = op in UNARY
    wy = imm if op == Op.CONCAT else w
    xs, ys, conds = [], (None if unary else []), ([] if op == Op.ITE else None)
    edges = shift_edge_amounts(w) if op in SHIFTS else None
    for m in range(M):
        if unary:
            xs.append(unary_value(op, w, m, rng))
            continue
        if op in DIVS:
            x, y = div_pair(op, w, m, rng, fx, fy)
        elif op in OVERFLOW:
            x, y = overflow_pair(op, w, m, rng, fx, fy)
        elif op in SHIFTS:
            x, y = shift_pair(op, w, m, rng, fx, fy, edges)
        elif op == Op.CONCAT:
            x, y = (fx if fx is not None else unary_value(op, w, m, rng)), (fy if fy is not None else unary_value(op, wy, m, rng))
        else:
            x, y = generic_pair(op, w, m, rng, fx, fy)
        xs.append(x & mask(w))
        ys.append(y & mask(wy))
        if conds is not None:
            conds.append((m // 2 + m // 14) % 2)
    rw = result_width(op, w, imm)
    rs = None
    if op in PREDICATES:
        expect = np.array([bool(ref(op, w, xs[m], ys[m])) != negate for m in range(M)])
    else:
        pos = flip_positions(rw)
        rs = []
        for m in range(M):
            r = ref(op, w, xs[m], None if unary else ys[m], conds[m] if conds is not None else imm)
            rs.append(r ^ (1 << pos[(m // 2) % len(pos)]) if m % 2 else r)
        expect = np.arange(M) % 2 == 0
    # variables of the tape, in order: x, y, (cond), (R)
    kx, ky = (form, None) if unary else (form[0], form[1])
    specs: List[Tuple[int, List[int]]] = []
    slot: Dict[str, int] = {}
    for side, kind, width, vals in (("x", kx, w, xs), ("y", ky, wy, ys)):
        if kind in ("v", "c"):
            slot[side] = len(specs)
            specs.append((width, vals if kind == "v" else [v ^ xor_const(width) for v in vals]))
    if conds is not None:
        slot["c"] = len(specs)
        # the computed forms test the condition as NOT(var): the variable holds its complement
        specs.append((0, conds if kx != "c" else [1 - v for v in conds]))
    if rs is not None:
        slot["r"] = len(specs)
        specs.append((rw, rs))

    def build(vi: Sequence[int]) -> Tape:
        t = Tape()
        a = _leaf(t, kx, w, vi[slot["x"]] if "x" in slot else None, fx)
        b = None if unary else _leaf(t, ky, wy, vi[slot["y"]] if "y" in slot else None, fy)
        if op in PREDICATES:
            root = t._pred(op, a, b)
            return t.finish(t.not_(root) if negate else root)
        if op == Op.NEG:
            v = t.neg(a)
        elif op == Op.BNOT:
            v = t.bnot(a)
        elif op == Op.EXTRACT:
            v = t.extract(imm[0], imm[1], a)
        elif op == Op.ZEXT:
            v = t.zext(imm, a)
        elif op == Op.SEXT:
            v = t.sext(imm, a)
        elif op == Op.CONCAT:
            v = t.concat(a, b)
        elif op == Op.ITE:
            cv = t.var(vi[slot["c"]], 0)
            v = t.ite(t.not_(cv) if kx == "c" else cv, a, b)
        else:
            v = t._bin(op, a, b)
        return t.finish(t.eq(v, t.var(vi[slot["r"]], rw)))

    return Case(op, w, form, place, imm, negate, xs, ys, conds, rs, expect, fx, fy, specs, build)


def op_widths(op: Op) -> Tuple[int, ...]:
    return WIDTHS if op in MULDIV else WIDTHS + WIDE_WIDTHS


def _case_params(op: Op, w: int) -> List[Tuple[str, object, Optional[int], Optional[int]]]:
    """(form, imm, fx, fy) of every case of ``op`` at operand width ``w``."""
    if op in UNARY:
        imms = {Op.EXTRACT: _extract_fields(w), Op.ZEXT: _ext_amounts(w), Op.SEXT: _ext_amounts(w)}.get(op, [None])
        return [(f, imm, None, None) for imm in imms for f in UNARY_FORMS]
    out = []
    for imm in (_concat_low_widths(w) if op == Op.CONCAT else [None]):
        wy = imm if op == Op.CONCAT else w
        for form in BINARY_FORMS:
            cxs = [None] if form[0] in "vc" else _constants(op, w, "x", form[0] == "K")
            cys = [None] if form[1] in "vc" else _constants(op, wy, "y", form[1] == "K")
            out += [(form, imm, cx, cy) for cx in cxs for cy in cys]
    return out


@functools.lru_cache(maxsize=None)
def group_cases(group: str) -> Tuple[Case, ...]:
    cases: List[Case] = []
    for op in GROUPS[group]:
        for w in op_widths(op):
            for form, imm, fx, fy in _case_params(op, w):
                for negate in ((False, True) if op in PREDICATES else (False,)):
                    base = make_case(op, w, form, "hi", imm, fx, fy, negate)
                    cases.append(base)
                    if base.max_width == 256 or (w in LO_WIDTHS and base.max_width < 256):
                        cases.append(replace(base, place="lo"))
    return tuple(cases)


def all_cases() -> List[Case]:
    return [c for g in GROUPS for c in group_cases(g)]


# ---------------------------------------------------------------- batches
N_PRELOADED = 8


@dataclass
class Pack:
    """Cases that share one model batch and one tape batch (tape i = cases[i])."""
    cases: List[Case]
    tapes: TapeBatch
    models: ModelBatch

    @property
    def expect(self) -> np.ndarray:
        return np.array([c.expect for c in self.cases])


def _rows(width: int, vals: Sequence[int]) -> np.ndarray:
    nl = limbs(width)
    raw = b"".join(int(v).to_bytes(4 * nl, "little") for v in vals)
    return np.frombuffer(raw, np.uint32).reshape(len(vals), nl).T


def _make_pack(cases: List[Case], first_index: int) -> Pack:
    order = []    # (case, local variable): variables of at most 256 bits first (G addresses rows with 16 bits)
    for ci, c in enumerate(cases):
        order += [(c.var_specs[k][0] > 256, ci, k) for k in range(len(c.var_specs))]
    order.sort()
    widths = [256] * first_index
    rows = [np.zeros((8 * first_index, M), np.uint32)] if first_index else []
    index: Dict[Tuple[int, int], int] = {}
    for _, ci, k in order:
        width, vals = cases[ci].var_specs[k]
        index[(ci, k)] = len(widths)
        widths.append(width)
        rows.append(_rows(width, vals))
    tapes = [c.build([index[(ci, k)] for k in range(len(c.var_specs))]) for ci, c in enumerate(cases)]
    return Pack(cases, TapeBatch(tapes), ModelBatch(widths, np.vstack(rows)))


def packs_of(cases: Sequence[Case], key: Optional[Callable[[Case], object]] = None) -> List[Pack]:
    """One pack of all the "hi" cases (variables from index 8 up, behind 8 unused ones) and packs
    of at most 8 variables for the "lo" ones; with ``key``, no "lo" pack mixes two key values."""
    out = []
    hi = [c for c in cases if c.place == "hi"]
    if hi:
        out.append(_make_pack(hi, N_PRELOADED))
    lo = [c for c in cases if c.place == "lo"]
    if key is not None:
        lo.sort(key=lambda c: str(key(c)))      # (stable: cases of a key stay in grid order)
    cur: List[Case] = []
    n = 0
    for c in lo:
        if cur and (n + len(c.var_specs) > N_PRELOADED or (key is not None and key(c) != key(cur[0]))):
            out.append(_make_pack(cur, 0))
            cur, n = [], 0
        cur.append(c)
        n += len(c.var_specs)
    if cur:
        out.append(_make_pack(cur, 0))
    return out


# ---------------------------------------------------------------- fault models (sensitivity)
@dataclass
class Fault:
    """A subtly wrong implementation ``fn(op, w, x, y, imm)`` of ``ops``.  ``can(op, w, imm, fx, fy)``:
    whether some operand pair of a case with those constant operands makes it differ from ``ref``
    at all (a fault that needs a multi-limb right operand is the identity mutation of a case whose
    right operand is the constant 3: such a case cannot, and need not, tell them apart)."""
    name: str
    ops: Tuple[Op, ...]
    fn: Callable
    can: Callable = lambda op, w, imm, fx, fy: True


def nlimbs(v: int) -> int:
    return max(1, (v.bit_length() + 31) // 32)


def _limb(v: int, k: int) -> int:
    return (v >> (32 * k)) & M32


def _split_add(x, y, k, sub):
    """x + y (x - y) with the carry (borrow) into limb k dropped."""
    lo = mask(32 * k)
    low = (x - y if sub else x + y) & lo
    high = ((x >> (32 * k)) - (y >> (32 * k)) if sub else (x >> (32 * k)) + (y >> (32 * k))) << (32 * k)
    return high | low


def _mag(v: int, w: int) -> int:
    return abs(to_signed(v, w))


def _signed_factor(f: int, w: int, negative: bool) -> bool:
    """Whether the w-bit signed f times some w-bit signed value is exactly 2^(w-1) (-2^(w-1))."""
    sf, t = to_signed(f, w), 1 << (w - 1)
    if sf == 0 or t % abs(sf):
        return False
    q = (-t if negative else t) // sf
    return -t <= q < t


def faults_for(op: Op, w: int, imm=None) -> List[Fault]:
    """The fault models applicable to ``op`` at operand width ``w`` (and immediate)."""
    L, mk, MIN = limbs(w), mask(w), 1 << (w - 1)
    F: List[Fault] = []

    def add(name, fn, can=None):
        F.append(Fault(name, (op,), fn, can or (lambda *a: True)))

    if op in (Op.ADD, Op.SUB):
        sub = op == Op.SUB
        for k in range(1, L):       # (the issue's table: ADD into bits 32 and 160, SUB into bit 32)
            add(f"{'borrow' if sub else 'carry'} into bit {32 * k} dropped",
                lambda o, w_, x, y, i, k=k: _split_add(x, y, k, sub) & mk,
                # a carry needs non-zero low limbs on both sides; a borrow a non-zero subtrahend
                (lambda o, w_, i, fx, fy, k=k: (fy is None or fy & mask(32 * k)) and (sub or fx is None or fx & mask(32 * k))))
    if op == Op.NEG:
        add("bit 1 wrong when the low limb is 0", lambda o, w_, x, y, i: ref(o, w_, x) ^ (2 & mk if x & M32 == 0 else 0),
            lambda *a: w >= 2)
        for k in range(1, L):
            add(f"carry into bit {32 * k} dropped", lambda o, w_, x, y, i, k=k: _split_add(~x & mk, 1, k, False) & mk)
    if op == Op.MUL:
        add("bit 64 of the product cleared when both operands >= 2^32",
            lambda o, w_, x, y, i: ref(o, w_, x, y) & ~((1 << 64) if x >> 32 and y >> 32 else 0),
            lambda o, w_, i, fx, fy: w > 64 and (fx is None or fx >> 32) and (fy is None or fy >> 32))
        for a in range(L):
            for b in range(L - a):
                add(f"partial product ({a}, {b}) dropped",
                    lambda o, w_, x, y, i, a=a, b=b: (x * y - (_limb(x, a) * _limb(y, b) << (32 * (a + b)))) & mk,
                    lambda o, w_, i, fx, fy, a=a, b=b: (fx is None or _limb(fx, a)) and (fy is None or _limb(fy, b)))
    if op in (Op.EQ, Op.ULT, Op.ULE, Op.SLT, Op.SLE):
        for k in range(L):
            hole = mk & ~(M32 << (32 * k))
            if L == 1:      # one limb: the compare ignores its top bit instead
                hole = mk >> 1
            add(f"compare ignores limb {k}", lambda o, w_, x, y, i, hole=hole: ref(o, w_, x & hole, y & hole) if w_ > 1 else ref(o, w_, 0, 0))
    if op in (Op.BAND, Op.BOR, Op.BXOR, Op.ITE):
        for k in range(L):
            lm = (M32 << (32 * k)) & mk
            add(f"limb {k} of the result is the left operand's",
                lambda o, w_, x, y, i, lm=lm: (ref(o, w_, x, y, i) & ~lm) | (x & lm),
                {Op.BAND: lambda o, w_, i, fx, fy, lm=lm: (fx is None or fx & lm) and (fy is None or ~fy & lm),
                 Op.BOR: lambda o, w_, i, fx, fy, lm=lm: (fy is None or fy & lm) and (fx is None or ~fx & lm),
                 Op.BXOR: lambda o, w_, i, fx, fy, lm=lm: fy is None or fy & lm,
                 Op.ITE: lambda o, w_, i, fx, fy, lm=lm: fx is None or fy is None or (fx ^ fy) & lm}[op])
    if w % 32 and op in (Op.ADD, Op.SUB, Op.MUL, Op.NEG, Op.BNOT, Op.SHL):
        top = mask(32 * L)

        def unmasked(o, w_, x, y, i):
            if o == Op.ADD:
                return (x + y) & top
            if o == Op.SUB:
                return (x - y) & top
            if o == Op.MUL:
                return (x * y) & top
            if o == Op.NEG:
                return -x & top
            if o == Op.BNOT:
                return ~x & top
            return 0 if y >= w_ else (x << y) & top
        add(f"result not re-masked above bit {w}", unmasked,
            # something must leave the width: a shift by 1..w-1, a product of factors >= 2, a
            # difference whose minuend is not all ones
            lambda o, w_, i, fx, fy: not ((o == Op.SHL and fy is not None and (fy == 0 or fy >= w)) or
                                          (o == Op.MUL and (fx in (0, 1) or fy in (0, 1))) or (o == Op.SUB and fx == mk)))
    if op == Op.UDIV and w % 32:
        add("x / 0 not re-masked", lambda o, w_, x, y, i: mask(32 * L) if y == 0 else x // y, lambda o, w_, i, fx, fy: fy in (None, 0))
    if op in SHIFTS:
        if w > 32:
            add("shift amount's high limbs ignored", lambda o, w_, x, y, i: ref(o, w_, x, y & M32),
                lambda o, w_, i, fx, fy: fy is None or (fy >> 32 and fy & M32 < w))
            add("shift amount = 0 mod 32 mishandled",
                lambda o, w_, x, y, i: ref(o, w_, x, y) ^ (1 if y % 32 == 0 and 0 < y < w_ else 0),
                lambda o, w_, i, fx, fy: fy is None or (fy % 32 == 0 and 0 < fy < w))
        if 32 * L < 2 ** w:
            add("shift amounts >= w not saturated",
                lambda o, w_, x, y, i: ref(o, w_, x, y % (32 * L) if y >= w_ else y),
                lambda o, w_, i, fx, fy: fy is None or (fy >= w and fy % (32 * L) < w))
        if op == Op.ASHR and w > 32:
            def short_fill(o, w_, x, y, i):
                if not x >> (w_ - 1) or y == 0 or y >= w_:
                    return ref(o, w_, x, y)
                lo_fill = w_ - y
                hi_fill = min(w_, (lo_fill + 31) // 32 * 32) if lo_fill % 32 else min(w_, lo_fill + 32)
                return (x >> y) | (mask(hi_fill) & ~mask(lo_fill))
            add("sign fill stops at the next limb boundary", short_fill,
                lambda o, w_, i, fx, fy: (fx is None or fx >> (w - 1)) and (fy is None or (0 < fy < w and w - fy + 32 < w + (w - fy) % 32)))
    if op == Op.SEXT:
        rw = w + imm
        nxt = (w + 31) // 32 * 32 if w % 32 else w + 32
        if nxt < rw:
            add("sign fill stops at the next limb boundary",
                lambda o, w_, x, y, i: x | (mask(nxt) & ~mask(w_) if x >> (w_ - 1) else 0))
        if rw % 32:
            add(f"result not re-masked above bit {rw}", lambda o, w_, x, y, i: to_signed(x, w_) & mask(32 * limbs(rw)))
    if op == Op.ZEXT:
        add("zero extension fills with the sign", lambda o, w_, x, y, i: to_signed(x, w_) & mask(w_ + i))
    if op == Op.EXTRACT:
        hi, lo = imm
        if hi // 32 - lo // 32 >= 2:
            bit = 32 * (lo // 32 + 2) - lo      # the first bit that comes from the third limb
            add("one bit lost when the field crosses two limb boundaries", lambda o, w_, x, y, i: ref(o, w_, x, y, i) & ~(1 << bit))
        rw = hi - lo + 1
        if rw % 32 and hi < w - 1:
            add(f"result not re-masked above bit {rw}", lambda o, w_, x, y, i: (x >> i[1]) & mask(min(32 * limbs(rw), w_ - i[1])))
    if op == Op.CONCAT:
        add("lowest bit of the high part lost", lambda o, w_, x, y, i: ((x & ~1) << i) | y, lambda o, w_, i, fx, fy: fx is None or fx & 1)
        add("low part not masked to its width", lambda o, w_, x, y, i: ((x << i) | y) ^ (((y >> (i - 1)) & 1) << i))
    if op in DIVS:
        signed = op in SIGNED_DIVS
        for n in range(1, L + 1):
            add(f"off by one when the divisor has {n} limbs",
                lambda o, w_, x, y, i, n=n: (ref(o, w_, x, y) + 1) & mk if y and nlimbs(_mag(y, w_) if signed else y) == n else ref(o, w_, x, y),
                lambda o, w_, i, fx, fy, n=n: fy is None or (fy != 0 and nlimbs(_mag(fy, w) if signed else fy) == n))
        add("division by 0 wrong", lambda o, w_, x, y, i: 0 if y == 0 else ref(o, w_, x, y), lambda o, w_, i, fx, fy: fy in (None, 0))
        if op == Op.UDIV:
            add("low quotient bit wrong when divisor and quotient >= 2^32",
                lambda o, w_, x, y, i: ref(o, w_, x, y) ^ (1 if y >> 32 and (x // y) >> 32 else 0),
                lambda o, w_, i, fx, fy: w > 64 and (fy is None or (fy >> 32 and (mk // fy) >> 32)) and (fx is None or fx >> 64))
        if op == Op.UREM:
            add("low bit wrong when the divisor >= 2^64", lambda o, w_, x, y, i: ref(o, w_, x, y) ^ (1 if y >> 64 else 0),
                lambda o, w_, i, fx, fy: w > 64 and (fy is None or fy >> 64))
        if signed:
            add("MIN / -1 wrong", lambda o, w_, x, y, i: ref(o, w_, x, y) ^ (1 if x == MIN and y == mk else 0),
                lambda o, w_, i, fx, fy: fx in (None, MIN) and fy in (None, mk))
        if op == Op.SMOD:
            add("SMOD computed as SREM", lambda o, w_, x, y, i: ref(Op.SREM, w_, x, y), lambda *a: w >= 2)
    if op == Op.UMUL_NOOVFL:
        add("<= instead of < at exactly 2^w", lambda o, w_, x, y, i: int(x * y <= 1 << w_),
            lambda o, w_, i, fx, fy: all(f is None or (f and (1 << w) % f == 0) for f in (fx, fy)))
    if op == Op.SMUL_NOOVFL:
        add("off by one at 2^(w-1)", lambda o, w_, x, y, i: int(to_signed(x, w_) * to_signed(y, w_) <= 1 << (w_ - 1)),
            lambda o, w_, i, fx, fy: all(f is None or _signed_factor(f, w, False) for f in (fx, fy)))
    if op == Op.SMUL_NOUDFL:
        add("off by one at -2^(w-1)", lambda o, w_, x, y, i: int(to_signed(x, w_) * to_signed(y, w_) > -(1 << (w_ - 1))),
            lambda o, w_, i, fx, fy: all(f is None or _signed_factor(f, w, True) for f in (fx, fy)))
    return F


def applicable(fault: Fault, case: Case) -> bool:
    """Whether the fault can differ from ``ref`` on some operands the case's form admits: by
    exhaustive enumeration up to 4 bits (at 1 bit most faults are the identity), else ``can``."""
    if case.max_width > 4:
        return bool(fault.can(case.op, case.w, case.imm, case.fx, case.fy))
    xs = range(1 << case.w) if case.fx is None else [case.fx]
    ys = [None] if case.ys is None else range(1 << case.wy) if case.fy is None else [case.fy]
    imms = (0, 1) if case.op == Op.ITE else (case.imm,)
    return any(fault.fn(case.op, case.w, x, y, i) != ref(case.op, case.w, x, y, i) for x in xs for y in ys for i in imms)


def constant_predicate(case: Case) -> bool:
    """Whether a predicate case of at most 8 bits has one value on every operand pair its form
    admits (UMUL_NOOVFL at 1 bit, ULT(1, y) at 1 bit, ...): such a tape cannot show both outcomes."""
    if case.rs is not None or case.w > 8:
        return False
    xs = range(1 << case.w) if case.fx is None else [case.fx]
    ys = range(1 << case.w) if case.fy is None else [case.fy]
    return len({ref(case.op, case.w, x, y) for x in xs for y in ys}) == 1


def killed_by(case: Case, fault: Fault) -> bool:
    """Whether the faulty implementation changes a verdict of the case: ``mut == R[m]`` is the
    verdict of a value case, ``mut`` itself that of a predicate (no tape evaluation needed)."""
    for m in range(M):
        x, y, imm = case.operands(m)
        got = fault.fn(case.op, case.w, x, y, imm)
        if case.rs is not None:
            if (got == case.rs[m]) != bool(case.expect[m]):
                return True
        elif bool(got) != (bool(case.expect[m]) != case.negate):
            return True
    return False
