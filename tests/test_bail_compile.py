"""The tape compiler's conjunction spine (tape_compiler.cpp, gprog.h G_BAIL): where bail points
go, what their second word says, the EQ-first conjunct order, and that the spine never costs a
stack slot or a temp.  Host only: programs are read back through ``evaluator.tape_program``."""
import pytest

from mythril_amd import evaluator as ev
from mythril_amd.synth import c2_workload, fuzz_workload
from mythril_amd.tape import Tape, TapeBatch

G_END, G_STORE_TMP_B, G_NOT, G_AND, G_EQ, G_BAIL = 0, 8, 10, 11, 20, 35
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


def program(tape_or_batch, t=0):
    tb = tape_or_batch if isinstance(tape_or_batch, TapeBatch) else TapeBatch([tape_or_batch])
    return decode(ev.tape_program(tb, t))


def bails(prog):
    return [ins[3] for ins in prog if ins[0] == G_BAIL]


# conjunct builders over the 256-bit variables 0..7: (name, fn(tape) -> Bool node); no two share
# a non-leaf node, so a conjunction's cost is the sum of its conjuncts' + one per AND
def v(t, i):
    return t.var(i, W)


CONJ = {
    # EQ, 88 ops: MUL 72 + ADD 8 + EQ 8
    "eq_small": lambda t: t.eq(t.add(t.mul(v(t, 0), v(t, 1)), v(t, 2)), t.const(0x1234, W)),
    # EQ, 168 ops: MUL 72 + MUL 72 + ADD 8 + BAND 8 + EQ 8
    "eq_big": lambda t: t.eq(t.mul(t.mul(v(t, 3), v(t, 4)), t.add(v(t, 5), v(t, 6))), t.band(v(t, 7), t.const(0xFF00FF, W))),
    # ULT, 88 ops
    "ult_a": lambda t: t.ult(t.mul(v(t, 1), v(t, 5)), t.add(v(t, 2), t.const(77, W))),
    # ULT, 160 ops
    "ult_b": lambda t: t.ult(t.mul(t.mul(v(t, 6), v(t, 2)), v(t, 0)), t.sub(v(t, 4), v(t, 3))),
    # NOT(EQ), 89 ops
    "ne": lambda t: t.not_(t.eq(t.add(t.mul(v(t, 7), v(t, 7)), v(t, 1)), t.const(5, W))),
}


def conj_tape(names):
    t = Tape()
    nodes = [CONJ[n](t) for n in names]
    return t.finish(t.and_(*nodes) if len(nodes) > 1 else nodes[0])


def ops_of(names):
    return ev.tape_alg_ops(TapeBatch([conj_tape(names)]), 0)


def spine(prog):
    """The conjunct order a spine program shows: the predicate that closes each conjunct (the
    last compare before the conjunct's AND / bail), as 'eq', 'cmp' or 'ne'."""
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


def test_bail_points_and_their_second_word(monkeypatch):
    """Four conjuncts written ULT, EQ(168), EQ(88), ULT: emitted cheapest EQ first, the others in
    their order, every conjunct after the first at slot 1 followed by AND d = 1, and a bail
    after each but the last whose second word is the cost of the rest of the program."""
    monkeypatch.delenv("MQ_NO_BAIL", raising=False)
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)
    written = ["ult_a", "eq_big", "eq_small", "ult_b"]
    order = ["eq_small", "eq_big", "ult_a", "ult_b"]
    assert ops_of(["eq_small"]) == 88 and ops_of(["eq_big"]) == 168 and ops_of(["ult_a"]) == 88 and ops_of(["ult_b"]) == 160
    prog = program(conj_tape(written))
    total = ops_of(written)
    assert total == 88 + 168 + 88 + 160 + 3
    # the rest after bail i: the conjuncts behind it as a tape of their own, + the AND joining them
    want = [ops_of(order[i + 1:]) + 1 for i in range(3)]
    assert want == [total - 88, total - 88 - 168 - 1, 160 + 1]
    assert bails(prog) == want
    assert spine(prog) == ["eq", "eq", "cmp", "cmp"]
    # shape: [c0 @0] BAIL [c1 @1] AND(d=1) BAIL [c2 @1] AND BAIL [c3 @1] AND END
    marks = [(op, d) for op, d, _, _ in prog if op in (G_AND, G_BAIL, G_END)]
    assert marks == [(G_BAIL, 0), (G_AND, 1), (G_BAIL, 0), (G_AND, 1), (G_BAIL, 0), (G_AND, 1), (G_END, 0)]
    first_bail = next(i for i, ins in enumerate(prog) if ins[0] == G_BAIL)
    assert max(d for _, d, _, _ in prog[:first_bail]) >= 1 and prog[first_bail - 1][0] == G_EQ and prog[first_bail - 1][1] == 1
    # the threshold: a bail only where at least MQ_BAIL_MIN_OPS ops follow
    monkeypatch.setenv("MQ_BAIL_MIN_OPS", "200")
    assert bails(program(conj_tape(written))) == [w for w in want if w >= 200]
    monkeypatch.setenv("MQ_BAIL_MIN_OPS", "100000")
    assert program(conj_tape(written)) == _no_bail_program(monkeypatch, conj_tape(written))


def _no_bail_program(monkeypatch, tape):
    monkeypatch.setenv("MQ_NO_BAIL", "1")
    try:
        return program(tape)
    finally:
        monkeypatch.delenv("MQ_NO_BAIL")


def test_eq_first_order_and_not_eq_stays_put(monkeypatch):
    """EQ conjuncts go first by ascending cost; a NOT above the EQ disqualifies it (it keeps its
    place among the others, and alone it earns no bail point); an EQ written last is still first."""
    monkeypatch.delenv("MQ_NO_BAIL", raising=False)
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)
    prog = program(conj_tape(["ne", "ult_a", "eq_big"]))
    assert spine(prog) == ["eq", "ne", "cmp"]
    assert bails(prog) == [ops_of(["ne", "ult_a"]) + 1, ops_of(["ult_a"]) + 1]
    prog = program(conj_tape(["ult_b", "ult_a", "ne", "eq_small"]))
    assert spine(prog) == ["eq", "cmp", "cmp", "ne"]
    assert bails(prog)[0] == ops_of(["ult_b", "ult_a", "ne"]) + 1
    # MQ_NO_BAIL=1: nothing emitted, nothing reordered
    off = _no_bail_program(monkeypatch, conj_tape(["ult_b", "ult_a", "ne", "eq_small"]))
    assert not bails(off) and spine(off)[-1] == "eq"


def _balanced():
    t = Tape()
    a, b, c, d = (CONJ[n](t) for n in ("ult_a", "eq_big", "ult_b", "eq_small"))
    return t.finish(t.and_(t.and_(a, b), t.and_(c, d)))


def test_any_nesting_of_single_use_ands_is_flattened(monkeypatch):
    monkeypatch.delenv("MQ_NO_BAIL", raising=False)
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)
    prog = program(_balanced())
    assert spine(prog) == ["eq", "eq", "cmp", "cmp"]
    assert bails(prog) == bails(program(conj_tape(["ult_a", "eq_big", "ult_b", "eq_small"])))
    t = Tape()
    a, b, c = (CONJ[n](t) for n in ("ult_a", "eq_small", "ult_b"))
    prog = program(t.finish(t.and_(a, t.and_(b, c))))     # right-nested
    assert spine(prog) == ["eq", "cmp", "cmp"] and len(bails(prog)) == 2


def _multi_use_and():
    t = Tape()
    x = t.and_(CONJ["eq_small"](t), CONJ["ult_a"](t))      # two users: a Bool temp
    return t.finish(t.and_(x, t.iff(x, CONJ["ult_b"](t))))


def _or_root():
    t = Tape()
    return t.finish(t.or_(CONJ["eq_small"](t), CONJ["eq_big"](t), CONJ["ult_b"](t)))


def _not_eq_only():
    return conj_tape(["ne", "ult_b", "ult_a"])


@pytest.mark.parametrize("make", [lambda: conj_tape(["eq_big"]), _or_root, _not_eq_only, _multi_use_and],
                         ids=["single_conjunct", "or_root", "not_eq_conjuncts", "multi_use_and"])
def test_tapes_that_carry_no_bail(monkeypatch, make):
    """No bail point, and the very program MQ_NO_BAIL=1 gives: a single conjunct, an OR root,
    conjuncts none of which is a plain EQ (NOT(EQ) is not one), an AND node with two users (it is a
    Bool temp, computed in a unit of its own that ends in STORE_TMP at slot 0)."""
    monkeypatch.delenv("MQ_NO_BAIL", raising=False)
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)
    tape = make()
    prog = program(tape)
    assert not bails(prog)
    assert prog == _no_bail_program(monkeypatch, tape)
    if make is _multi_use_and:
        assert any(op == G_STORE_TMP_B for op, _, _, _ in prog)


def test_column_programs_carry_no_bail(monkeypatch):
    """A value-root (column) compile of a tape that gets bail points as a verdict tape has the
    words of the MQ_NO_BAIL=1 program: column programs are never given one."""
    monkeypatch.delenv("MQ_NO_BAIL", raising=False)
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)
    tape = conj_tape(["ult_a", "eq_big", "eq_small", "ult_b"])
    tb = TapeBatch([tape])
    on = ev.compile_info_g(tb, 0)          # (mq_tape_compile_info_g compiles with value_root)
    n_on = ev.compile_info(tb, 0).prog_words
    monkeypatch.setenv("MQ_NO_BAIL", "1")
    off = ev.compile_info_g(tb, 0)
    n_off = ev.compile_info(tb, 0).prog_words
    assert on == off
    assert n_on == n_off + 2 * 3           # the verdict compile: three two-word bail points


def _workloads():
    yield "c2", c2_workload(50, 100)[0]
    for seed in range(4):
        yield f"fuzz{seed}", fuzz_workload(seed, 60, 4)[0]
    # (8-variable fuzz: the seed and depth at which a few random roots are conjunctions with a spine)
    yield "fuzz_asm", fuzz_workload(9, 120, 4, asm_only=True, depth=5)[0]


@pytest.mark.parametrize("name,tb", list(_workloads()), ids=[n for n, _ in _workloads()])
def test_depth_and_temps_never_grow(monkeypatch, name, tb):
    """depth, the temp count, and depth_g / its temp count -- of the verdict compile for the G
    interpreter's four slots (``tape_program_g``: what an upload builds, the spilled variant
    where the plain program is deeper) -- with bail points are those without (a deeper program
    would move a tape off P, or off G); second words fall along a program and stay below the
    tape's cost; every C2 tape (an EQ first conjunct, conjuncts of hundreds of ops) has one and
    some of their spilled G programs carry the spine; the 8-variable fuzz batch has spines too."""
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)
    info = {}
    for mode in ("on", "off"):
        if mode == "off":
            monkeypatch.setenv("MQ_NO_BAIL", "1")
        else:
            monkeypatch.delenv("MQ_NO_BAIL", raising=False)
        rows = []
        for t in range(tb.n_tapes):
            ci = ev.compile_info(tb, t)
            if not ci.supported:
                rows.append(None)
                continue
            pg, dg, tg, spilled = ev.tape_program_g(tb, t)
            rows.append((ci.depth, ci.n_temps, (dg, tg, spilled, decode(pg)), decode(ev.tape_program(tb, t))))
        info[mode] = rows
    n_bail = n_spine_g = 0
    for t, (a, b) in enumerate(zip(info["on"], info["off"])):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert a[0] <= b[0] and a[1] <= b[1], (name, t, a[:2], b[:2])
        (dg, tg, sp, pg), (dg0, tg0, sp0, pg0) = a[2], b[2]
        # (the spine can be the shallower program: then it fits G unspilled where today's does not)
        assert dg <= dg0 and tg <= tg0 and sp <= sp0, (name, t, a[2][:3], b[2][:3])
        assert max(d for _, d, _, _ in pg) < dg and (not sp or dg <= 4), (name, t, dg)
        assert not bails(b[3]) and not bails(pg0)
        for on, off in ((a[3], b[3]), (pg, pg0)):
            ws = bails(on)
            if not ws:
                assert on == off, (name, t)       # no bail point: the program is untouched
                continue
            total = ev.tape_alg_ops(tb, t)
            assert all(x > y for x, y in zip(ws, ws[1:])) and ws[0] < total and ws[-1] >= 64, (name, t, ws, total)
            if on is a[3] or sp == sp0:
                assert sum(1 for i in on if i[0] != G_BAIL) == len(off), (name, t)
        n_bail += bool(bails(a[3]))
        n_spine_g += sp and bool(bails(pg))
    if name == "c2":
        assert n_bail == tb.n_tapes
        assert n_spine_g > 0, n_spine_g
    if name == "fuzz_asm":
        assert n_bail > 0


def test_deep_conjunction_spilled_for_g(monkeypatch):
    """An AND-root tape over variables 0-7 whose conjuncts need five slots under the spine's six:
    P's program has the spine, and the variant spilled to G's four slots (more of the tape in
    temps, computed before the root unit, so fewer ops are left to skip) has one too -- within
    four slots, with no more slots or temps than without bail points."""
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)

    def deep(t, k, o):     # right-nested subtractions (not commutative: no operand swap): k + 2 slots
        x = t.mul(v(t, (k + o) % 8), v(t, (k + 1 + o) % 8))
        for j in range(k):
            x = t.sub(t.mul(v(t, (j + o) % 8), v(t, (j + 3 + o) % 8)), x)
        return x

    t = Tape()
    tape = t.finish(t.and_(t.ult(deep(t, 3, 0), v(t, 1)), t.eq(deep(t, 3, 1), t.const(9, W)), t.eq(v(t, 2), deep(t, 3, 2))))
    tb = TapeBatch([tape])
    monkeypatch.delenv("MQ_NO_BAIL", raising=False)
    ci, (pg, dg, tg, sp) = ev.compile_info(tb, 0), ev.tape_program_g(tb, 0)
    monkeypatch.setenv("MQ_NO_BAIL", "1")
    ci0, (pg0, dg0, tg0, sp0) = ev.compile_info(tb, 0), ev.tape_program_g(tb, 0)
    monkeypatch.delenv("MQ_NO_BAIL")
    assert ci.supported and 4 < ci0.depth <= 6 and ci.depth <= ci0.depth and ci.n_temps <= ci0.n_temps
    assert sp and sp0 and dg <= dg0 <= 4 and tg <= tg0
    pg, pg0 = decode(pg), decode(pg0)
    assert len(bails(program(tape))) == 2
    assert bails(pg) and not bails(pg0) and bails(pg)[0] >= 64
    assert spine(pg) == ["eq", "eq", "cmp"]
    assert max(d for _, d, _, _ in pg) < 4
    assert sum(1 for i in pg if i[0] != G_BAIL) == len(pg0)
