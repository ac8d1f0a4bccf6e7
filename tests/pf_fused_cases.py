"""Hand-built conjunction tapes for the fused narrow handlers of the low-limb prefilter
(gen_qsa.py ADD32V .. MUL32VV, qsa_translate.cpp qsa_translate_pf), shared by the host and the GPU
tests.  Every tape is And(<a dear ULE>, EQ(expr, R)) with R planted at one model.

Placement: the tape compiler evaluates the deeper operand of a binary op first and the left one
on a tie, so a subtree X lands at stack slot s when it is the right operand of s nested SUBs
whose left operands are complete SUB trees over variables at least as deep as what they face
(`at_slot`).  SUB keeps the operand order visible in the value."""
import numpy as np

from mythril_amd.models import ModelBatch
from mythril_amd.synth import random_words
from mythril_amd.tape import Tape, TapeBatch

W = 256
M256 = (1 << W) - 1
PY = {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "band": lambda a, b: a & b,
      "bor": lambda a, b: a | b, "bxor": lambda a, b: a ^ b, "neg": lambda a: -a, "bnot": lambda a: ~a}
BINOPS = ("add", "sub", "mul", "band", "bor", "bxor")
KOPS = ("add", "mul", "band", "bor", "bxor")       # ADDK, MULK, ANDK, ORK, XORK
LOW_CONSTS = (0, 1, 0x80000000, 0xFFFFFFFF)
# handler kinds of the prefilter mode: the fused narrow ones, the unfused narrow ones a program
# over variables reaches (PUSH_K32 needs a constant conjunct), and P's own that serve the mode
FUSED = {"ADD32V", "SUB32V", "MUL32V", "EQ32V", "ADD32VV", "SUB32VV", "MUL32VV", "ADDK32V", "MULK32V", "ANDK32V", "ORK32V",
         "XORK32V", "EQK32V"}
UNFUSED = {"ADD32", "SUB32", "MUL32", "NEG32", "ADDK32", "MULK32", "ANDK32", "ORK32", "XORK32", "EQ32", "EQK32"}
SHARED = {"PUSH_VAR", "BNOT", "BAND", "BOR", "BXOR", "BANDV", "BORV", "BXORV", "BANDVV", "BORVV", "BXORVV"}
MAX_SLOT = 4            # gen_qsa.py DF: the deepest slot a 48-instruction narrow program reaches


def var(i):
    return ("var", i % 8)


def const(c):
    return ("const", c & M256)


def op(name, *args):
    return (name,) + args


def label(e):
    """Stack slots the compiled expression needs (constants fold into their reader)."""
    if e[0] in ("var", "const"):
        return 1
    if len(e) == 2:
        return label(e[1])
    a, b = label(e[1]), label(e[2])
    if e[2][0] == "const" or e[1][0] == "const":
        return max(a, b) if e[1][0] != e[2][0] else 1
    return a + 1 if a == b else max(a, b)


def value(e, vals):
    if e[0] == "var":
        return vals[e[1]]
    if e[0] == "const":
        return e[1]
    return PY[e[0]](*(value(x, vals) for x in e[1:])) & M256


def build(t, e):
    if e[0] == "var":
        return t.var(e[1], W)
    if e[0] == "const":
        return t.const(e[1], W)
    return getattr(t, e[0])(*(build(t, x) for x in e[1:]))


def complete(n, k):
    """A complete SUB tree over variables needing n slots; k rotates the variables."""
    if n == 1:
        return var(k)
    return op("sub", complete(n - 1, k), complete(n - 1, k + 3))


def at_slot(x, s, k=0):
    """x evaluated with s values below it."""
    e = x
    for i in range(s):
        e = op("sub", complete(label(e), k + i), e)
    return e


def wide(rng, low):
    """A 256-bit constant with the given low limb (random above: nothing folds)."""
    return const((int.from_bytes(rng.bytes(28), "little") << 32) | low)


def cases(rng):
    """[(name, expr, rhs)]: rhs None = a planted constant R, else the variable compared against
    (the expression then ends in + c, c planted)."""
    out = []
    for v in range(8):
        # right operand a variable: S[d - 1] = S[d - 1] op V[v]
        for d in range(1, MAX_SLOT + 1):
            for o in BINOPS:
                out.append((f"{o}V d{d} v{v}", at_slot(op(o, op("bnot", var(v + d)), var(v)), d - 1, v), None))
        out.append((f"eqV v{v}", op("bnot", var(v + 1)), v))
        # variable with constant: S[d] = V[v] op k
        for d in range(MAX_SLOT + 1):
            for o in KOPS:
                out.append((f"{o}KV d{d} v{v}", at_slot(op(o, var(v), wide(rng, int(rng.integers(2, 1 << 32)))), d, v + 1), None))
        out.append((f"eqKV v{v}", var(v), None))
        # both operands variables: S[x] = V[v] op V[v2]
        for x in range(MAX_SLOT):
            for o in BINOPS:
                out.append((f"{o}VV x{x} v{v}", at_slot(op(o, var(v), var(v + 1 + (x + BINOPS.index(o)) % 7)), x, v + 1), None))
    for v1 in range(8):
        for v2 in range(8):
            for o in BINOPS:
                # (x - x and x ^ x hold at every model: another variable on top)
                e = op(o, var(v1), var(v2))
                out.append((f"{o}VV v{v1} v{v2}", op("sub", e, var(v1 + 1)) if v1 == v2 else e, None))
    for o in KOPS:
        for k in LOW_CONSTS:
            if k == 0 and o in ("mul", "band"):     # (the low limb is 0 whatever the variable: it folds)
                continue
            for d in (0, 2):
                out.append((f"{o}KV k{k:#x} d{d}", at_slot(op(o, var(3), wide(rng, k)), d, 1), None))
    for o in BINOPS:        # the unfused binary forms: both operands computed
        out.append((f"{o}", op(o, op("bnot", var(1)), op("neg", var(6))), None))
    for o in KOPS:          # the unfused constant forms, on a computed value
        out.append((f"{o}K", op(o, op("bnot", var(2)), wide(rng, int(rng.integers(2, 1 << 32)))), None))
    # an M0-indexed handler (kindVV) right before and right after the other classes of handler
    vv = lambda i: op(("add", "sub", "mul")[i % 3], var(i), var(i + 5))   # noqa: E731
    k = wide(rng, 0x1234567)
    for name, left in (("neg", op("neg", vv(0))), ("bnot", op("bnot", vv(1))), ("addk", op("add", vv(2), k)),
                       ("mulk", op("mul", vv(3), k)), ("addv", op("add", vv(4), var(6))), ("bandv", op("band", vv(5), var(7))),
                       ("add32", op("add", vv(6), vv(7))), ("band", op("band", vv(6), vv(7)))):
        out.append((f"m0 {name}", op("sub", left, vv(len(name))), None))
    out.append(("m0 kv", op("sub", vv(1), op("mul", var(2), k)), None))
    out.append(("m0 pushvar", op("sub", vv(2), op("bnot", var(3))), None))
    out.append(("m0 eq32", op("bnot", vv(3)), "expr"))
    return out


def spots(m):
    """Planted models spread over the 64-model blocks, lanes 0 and 63, and the last model."""
    out = [64 * b + lane for b in range((m + 63) // 64) for lane in (0, 63) if 64 * b + lane < m]
    return out + [m - 1]


def fused_batch(m, seed=71, only=""):
    """(TapeBatch, ModelBatch, planted model per tape, names); only: the cases whose name starts so."""
    rng = np.random.Generator(np.random.PCG64(seed))
    words = random_words(rng, 64, m)
    mb = ModelBatch([W] * 8, words)
    sp = spots(m)
    tapes, planted, names = [], [], []
    for i, (name, e, rhs) in enumerate(c for c in cases(rng) if c[0].startswith(only)):
        p = sp[i % len(sp)]
        vals = [mb.var_value(v, p) for v in range(8)]
        t = Tape()
        if rhs is None:
            eq = t.eq(build(t, e), t.const(value(e, vals), W))
        elif rhs == "expr":     # both sides computed: EQ32 behind an M0-indexed handler
            r = op("mul", var(4), var(6))
            c = (value(r, vals) - value(e, vals)) & M256
            eq = t.eq(build(t, op("add", e, const(c))), build(t, r))
        else:
            c = (vals[rhs] - value(e, vals)) & M256
            eq = t.eq(t.add(build(t, e), t.const(c, W)), t.var(rhs, W))
        tapes.append(t.finish(t.and_(t.ule(t.mul(t.var(4, W), t.var(5, W)), t.const(M256, W)), eq)))
        planted.append(p)
        names.append(name)
    return TapeBatch(tapes), mb, np.asarray(planted), names
