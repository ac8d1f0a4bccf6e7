"""MQ_G_BAIL=1 in the tape compiler (tape_compiler.cpp g_bail_enabled): tapes that read a variable
outside the P interpreter's eight get the conjunction spine and its bail points under the
unchanged rules, for both programs an upload builds (``tape_program``, and ``tape_program_g``: the
variant spilled to G's four slots where the plain one is deeper).  With the flag unset they keep
the programs MQ_NO_BAIL=1 gives, word for word.  Host only."""
import pytest

from mythril_amd import evaluator as ev
from mythril_amd.tape import Tape, TapeBatch

G_END, G_NOT, G_AND, G_EQ, G_BAIL = 0, 10, 11, 20, 35
G_CMP = (21, 22, 23, 24)          # ULT ULE UGT UGE
HAS_IMM2 = (56, 57, 58, 60, 61, 32, 33, 34, 35)
W = 256


def decode(prog):
    """[(op, d, imm, second word or None)] of a gprog.h program."""
    out, i = [], 0
    while i < len(prog):
        w = int(prog[i])
        i += 1
        op = w & 0xFF
        imm2 = None
        if op in HAS_IMM2:
            imm2 = int(prog[i])
            i += 1
        out.append((op, (w >> 8) & 0xF, w >> 12, imm2))
    return out


def bails(prog):
    return [ins[3] for ins in prog if ins[0] == G_BAIL]


def spine(prog):
    """The predicate that closes each conjunct of a spine program: 'eq', 'cmp' or 'ne'."""
    kinds, last = [], None
    for op, d, imm, imm2 in prog:
        if op == G_EQ:
            last = "eq"
        elif op in G_CMP:
            last = "cmp"
        elif op == G_NOT:
            last = "ne"
        elif (op == G_AND and d == 1) or (op == G_BAIL and not kinds) or (op == G_END and not kinds):
            if last is not None:
                kinds.append(last)
            last = None
    return kinds


def v(t, i):
    return t.var(i, W)


# conjuncts over the 256-bit variables 0..8; no two share a non-leaf node, so a conjunction costs
# the sum of its conjuncts + one per AND.  ult_b9 reads the ninth variable: the tape is G's
CONJ = {
    # EQ, 88 ops: MUL 72 + ADD 8 + EQ 8
    "eq_small": lambda t: t.eq(t.add(t.mul(v(t, 0), v(t, 1)), v(t, 2)), t.const(0x1234, W)),
    # EQ, 168 ops: MUL 72 + MUL 72 + ADD 8 + BAND 8 + EQ 8
    "eq_big": lambda t: t.eq(t.mul(t.mul(v(t, 3), v(t, 4)), t.add(v(t, 5), v(t, 6))), t.band(v(t, 7), t.const(0xFF00FF, W))),
    # ULT, 88 ops
    "ult_a": lambda t: t.ult(t.mul(v(t, 1), v(t, 5)), t.add(v(t, 2), t.const(77, W))),
    # ULT, 168 ops: MUL 72 + MUL 72 + ADD 8 + SUB 8 + ULT 8
    "ult_b9": lambda t: t.ult(t.add(t.mul(t.mul(v(t, 6), v(t, 2)), v(t, 0)), v(t, 8)), t.sub(v(t, 4), v(t, 3))),
}
COST = {"eq_small": 88, "eq_big": 168, "ult_a": 88, "ult_b9": 168}


def conj_tape(names, balanced=False):
    t = Tape()
    n = [CONJ[x](t) for x in names]
    if balanced:
        return t.finish(t.and_(t.and_(n[0], n[1]), t.and_(n[2], n[3])))
    return t.finish(t.and_(*n))


def ops_of(names):
    return sum(COST[n] for n in names) + len(names) - 1


WRITTEN = ["ult_a", "eq_big", "eq_small", "ult_b9"]
ORDER = ["eq_small", "eq_big", "ult_a", "ult_b9"]         # EQ first, cheapest first, the rest as written
TAPES = {
    "flat": lambda: conj_tape(WRITTEN),
    "balanced": lambda: conj_tape(WRITTEN, balanced=True),
    "eq_last": lambda: conj_tape(["ult_a", "ult_b9", "eq_big", "eq_small"]),
}


def _programs(tape):
    tb = TapeBatch([tape])
    pg, dg, tg, spilled = ev.tape_program_g(tb, 0)
    return decode(ev.tape_program(tb, 0)), decode(pg), (dg, tg, spilled)


def _env(monkeypatch, g_bail, no_bail=False):
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)
    for name, on in (("MQ_G_BAIL", g_bail), ("MQ_NO_BAIL", no_bail)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("shape", list(TAPES))
def test_flag_unset_keeps_the_programs(monkeypatch, shape):
    """A tape reading a ninth variable, flag unset: both programs are MQ_NO_BAIL=1's."""
    tape = TAPES[shape]()
    assert ev.tape_alg_ops(TapeBatch([tape]), 0) == ops_of(WRITTEN)
    _env(monkeypatch, g_bail=False)
    p, pg, info = _programs(tape)
    _env(monkeypatch, g_bail=False, no_bail=True)
    p0, pg0, info0 = _programs(tape)
    assert p == p0 and pg == pg0 and info == info0
    assert not bails(p) and not bails(pg)


@pytest.mark.parametrize("shape", list(TAPES))
def test_flag_places_bail_points_on_nine_variable_tapes(monkeypatch, shape):
    """MQ_G_BAIL=1: the same tapes carry G_BAIL in both programs, cheapest EQ first, every second
    word the cost of the rest of the program; MQ_NO_BAIL=1 still removes everything."""
    tape = TAPES[shape]()
    _env(monkeypatch, g_bail=True)
    p, pg, info = _programs(tape)
    want = [ops_of(ORDER[i + 1:]) + 1 for i in range(3)]
    total = ops_of(WRITTEN)
    assert want == [total - 88, total - 88 - 168 - 1, 168 + 1]
    for prog in (p, pg):
        assert bails(prog) == want
        assert spine(prog) == ["eq", "eq", "cmp", "cmp"]
        marks = [(op, d) for op, d, _, _ in prog if op in (G_AND, G_BAIL, G_END)]
        assert marks == [(G_BAIL, 0), (G_AND, 1), (G_BAIL, 0), (G_AND, 1), (G_BAIL, 0), (G_AND, 1), (G_END, 0)]
    _env(monkeypatch, g_bail=True, no_bail=True)
    p0, pg0, info0 = _programs(tape)
    assert not bails(p0) and not bails(pg0)
    # the spine costs no slot and no temp, and only adds the two-word bail points
    assert info == info0
    assert sum(1 for i in p if i[0] != G_BAIL) == len(p0) and sum(1 for i in pg if i[0] != G_BAIL) == len(pg0)
    _env(monkeypatch, g_bail=False)
    assert _programs(tape) == (p0, pg0, info0)


def test_spilled_g_variant_carries_its_own_second_words(monkeypatch):
    """Conjuncts needing five slots, one reading a ninth variable: the variant spilled to G's four
    slots has more of the tape in temps (computed before the root unit), so its bail points skip
    less than the plain program's; neither needs more slots or temps than without the flag."""

    def deep(t, k, o):     # right-nested subtractions (no operand swap): k + 2 slots
        x = t.mul(v(t, (k + o) % 9), v(t, (k + 1 + o) % 9))
        for j in range(k):
            x = t.sub(t.mul(v(t, (j + o) % 9), v(t, (j + 3 + o) % 9)), x)
        return x

    t = Tape()
    tape = t.finish(t.and_(t.ult(deep(t, 3, 0), v(t, 8)), t.eq(deep(t, 3, 1), t.const(9, W)), t.eq(v(t, 2), deep(t, 3, 2))))
    tb = TapeBatch([tape])
    _env(monkeypatch, g_bail=False)
    ci0, (p0, pg0, (dg0, tg0, sp0)) = ev.compile_info(tb, 0), _programs(tape)
    _env(monkeypatch, g_bail=True)
    ci, (p, pg, (dg, tg, sp)) = ev.compile_info(tb, 0), _programs(tape)
    assert ci.supported and 4 < ci0.depth <= 6 and (ci.depth, ci.n_temps) == (ci0.depth, ci0.n_temps)
    assert sp and sp0 and (dg, tg) == (dg0, tg0) and dg <= 4
    assert not bails(p0) and not bails(pg0)
    assert len(bails(p)) == 2 and bails(pg)
    assert bails(pg)[0] >= 64 and bails(pg)[0] < bails(p)[0]
    assert spine(pg) == ["eq", "eq", "cmp"]
    assert max(d for _, d, _, _ in pg) < 4
    assert sum(1 for i in pg if i[0] != G_BAIL) == len(pg0)


_C3 = {}


def _c3(hoist):
    from mythril_amd.synth_evm import c3_workload
    if hoist not in _C3:
        _C3[hoist] = c3_workload(40, 128, seed=3, hoist=hoist)[0]
    return _C3[hoist]


def _c3_rows(tb):
    rows = []
    for t in range(tb.n_tapes):
        ci = ev.compile_info(tb, t)
        assert ci.supported
        pg, dg, tg, sp = ev.tape_program_g(tb, t)
        rows.append(((ci.depth, ci.n_temps), ev.compile_info_g(tb, t), (dg, tg, sp), decode(ev.tape_program(tb, t)), decode(pg)))
    return rows


@pytest.mark.parametrize("hoist", [False, True], ids=["unhoisted", "hoisted"])
def test_c3_depth_temps_coverage_and_columns(monkeypatch, hoist):
    """synth_evm.c3_workload(40, 128, seed=3): every tape reads a variable >= 8 and has a
    bit-vector EQ conjunct, so with the flag every tape gets a bail point; depth and temps -- of
    the plain compile, of the G compile and of the value-root (column) compile -- are those
    without the flag, and the column compile has the same number of words: no bail point."""
    tb = _c3(hoist)
    _env(monkeypatch, g_bail=False)
    off = _c3_rows(tb)
    _env(monkeypatch, g_bail=True)
    on = _c3_rows(tb)
    _env(monkeypatch, g_bail=True, no_bail=True)
    none = _c3_rows(tb)
    n_g = 0
    for t, (a, b, c) in enumerate(zip(on, off, none)):
        assert a[0] == b[0] and a[2] == b[2], (t, a[:3], b[:3])
        assert a[1] == b[1] == c[1], t                 # value root: (depth, temps, words) unchanged
        assert not bails(b[3]) and not bails(b[4])     # flag unset: word for word MQ_NO_BAIL's
        assert b[3] == c[3] and b[4] == c[4], t
        ws = bails(a[3])
        assert ws, t                                   # coverage: 40 of 40
        total = ev.tape_alg_ops(tb, t)
        for w2 in (ws, bails(a[4])):
            assert all(x > y for x, y in zip(w2, w2[1:])) and all(64 <= x < total for x in w2), (t, w2, total)
        n_g += bool(bails(a[4]))
    print(f"hoist={hoist}: {n_g} of {tb.n_tapes} G programs carry a bail point")
    # (a spilled G variant keeps less in its root unit: a few unhoisted tapes have nothing left to skip)
    assert n_g == tb.n_tapes if hoist else n_g > tb.n_tapes // 2
