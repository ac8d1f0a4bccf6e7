"""The planted-result grid (planted_ops.py) on the CPU: both oracles agree with its by-construction
expectations, every fault model changes a verdict in every form it applies to, every predicate
tape has both outcomes, nothing is unsupported - and the seeded fuzz workload kills fewer of the
same faults."""
import random

import numpy as np
import pytest

import cref
import planted_ops as po
import pyoracle
from mythril_amd.evaluator import compile_info
from mythril_amd.synth import fuzz_workload
from mythril_amd.tape import NONE, Op, from_words, limbs

GROUPS = list(po.GROUPS)


@pytest.fixture(scope="module")
def packs():
    cache = {}

    def get(group):
        if group not in cache:
            cache[group] = po.packs_of(po.group_cases(group))
        return cache[group]
    return get


def test_reference_semantics_spot_values():
    """SMT-LIB's corner definitions, written out: division by zero, MIN / -1, the sign of
    bvsrem / bvsmod, shifts by the width and more."""
    r, m8 = po.ref, 0xFF
    assert r(Op.UDIV, 8, 7, 0) == m8 and r(Op.UREM, 8, 7, 0) == 7
    assert r(Op.SDIV, 8, 7, 0) == m8 and r(Op.SDIV, 8, 0xF9, 0) == 1 and r(Op.SDIV, 8, 0, 0) == m8
    assert r(Op.SREM, 8, 0xF9, 0) == 0xF9 and r(Op.SMOD, 8, 0xF9, 0) == 0xF9
    assert r(Op.SDIV, 8, 0x80, m8) == 0x80 and r(Op.SREM, 8, 0x80, m8) == 0 and r(Op.SMOD, 8, 0x80, m8) == 0
    assert r(Op.SDIV, 8, 0xF9, 2) == 0xFD and r(Op.SREM, 8, 0xF9, 2) == m8 and r(Op.SMOD, 8, 0xF9, 2) == 1    # -7 / 2
    assert r(Op.SDIV, 8, 7, 0xFE) == 0xFD and r(Op.SREM, 8, 7, 0xFE) == 1 and r(Op.SMOD, 8, 7, 0xFE) == m8    # 7 / -2
    assert r(Op.SREM, 8, 0xF9, 0xFE) == m8 and r(Op.SMOD, 8, 0xF9, 0xFE) == m8                               # -7 / -2
    assert r(Op.SHL, 8, 0x81, 8) == 0 and r(Op.LSHR, 8, 0x81, 8) == 0 and r(Op.ASHR, 8, 0x81, 8) == m8
    assert r(Op.ASHR, 8, 0x81, 1) == 0xC0 and r(Op.ASHR, 8, 0x41, 200) == 0 and r(Op.SHL, 8, 0x81, 1) == 2
    assert r(Op.EXTRACT, 16, 0xABCD, imm=(11, 4)) == 0xBC and r(Op.CONCAT, 8, 0xAB, 0xC, imm=4) == 0xABC
    assert r(Op.SEXT, 4, 0x8, imm=4) == 0xF8 and r(Op.ZEXT, 4, 0x8, imm=4) == 0x08 and r(Op.SEXT, 4, 0x7, imm=4) == 7
    assert r(Op.SLT, 8, 0x80, 0x7F) == 1 and r(Op.ULT, 8, 0x80, 0x7F) == 0 and r(Op.SLE, 8, 0x7F, 0x7F) == 1
    assert r(Op.UMUL_NOOVFL, 8, 16, 16) == 0 and r(Op.UMUL_NOOVFL, 8, 15, 17) == 1
    assert r(Op.SMUL_NOOVFL, 8, 8, 16) == 0 and r(Op.SMUL_NOOVFL, 8, 0xF8, 16) == 1                            # 128, -128
    assert r(Op.SMUL_NOUDFL, 8, 0xF8, 16) == 1 and r(Op.SMUL_NOUDFL, 8, 0xF7, 16) == 0 and r(Op.SMUL_NOUDFL, 8, 0x80, 0x80) == 1
    assert r(Op.NEG, 8, 0x80) == 0x80 and r(Op.BNOT, 3, 5) == 2 and r(Op.ITE, 8, 1, 2, imm=0) == 2


def test_shift_amounts_are_the_variable_shift_tests():
    from test_gpu_parity import _shift_amounts
    for w in po.WIDTHS + po.WIDE_WIDTHS:
        assert po.shift_edge_amounts(w) == _shift_amounts(np.random.default_rng(0), w, 17)


def test_grid_shape():
    """What the grid has to span: every value op, the widths, forms and placements, M = 577."""
    cases = po.all_cases()
    assert po.M == 577 and po.NCLASS % 2 == 1
    vocab = {Op.ADD, Op.SUB, Op.MUL, Op.NEG, Op.UDIV, Op.UREM, Op.SDIV, Op.SREM, Op.SMOD, Op.BAND, Op.BOR, Op.BXOR, Op.BNOT,
             Op.SHL, Op.LSHR, Op.ASHR, Op.EXTRACT, Op.CONCAT, Op.ZEXT, Op.SEXT, Op.ITE, Op.EQ, Op.ULT, Op.ULE, Op.SLT, Op.SLE,
             Op.UMUL_NOOVFL, Op.SMUL_NOOVFL, Op.SMUL_NOUDFL}
    assert {c.op for c in cases} == vocab
    for op in vocab:
        mine = [c for c in cases if c.op == op]
        want = (1, 8, 31, 32, 33, 64, 160, 255, 256, 257, 512) + (() if op in po.MULDIV else (544, 1088, 2048))
        # (CONCAT / ZEXT / SEXT widen: their 2048-bit cases are results, no operand can be that wide)
        assert {c.w for c in mine} | {c.max_width for c in mine} >= set(want) and {c.w for c in mine} <= set(want), op
        forms = po.UNARY_FORMS if op in po.UNARY else ("vv", "vk", "vK", "kv", "cc", "cv")
        for w in sorted({c.w for c in mine}):
            have = {c.form for c in mine if c.w == w}
            assert set(forms) - have <= ({"vK"} if w <= 16 else set()), (op, w, have)
        # every 256-bit case twice: on the preloaded variables and past them
        at256 = [c for c in mine if c.max_width == 256]
        assert at256 and sum(c.place == "lo" for c in at256) == sum(c.place == "hi" for c in at256)
        if op in po.PREDICATES:
            assert sum(c.negate for c in mine) * 2 == len(mine)
    # shifts by a constant and by a variable; the width changes' immediates
    assert all({c.form for c in cases if c.op == op} >= {"vk", "vv"} for op in po.SHIFTS)
    ext = {c.imm for c in cases if c.op == Op.EXTRACT and c.w == 256}
    assert any(hi // 32 - lo // 32 >= 2 for hi, lo in ext) and any(lo % 32 == 0 and hi % 32 == 31 for hi, lo in ext)
    assert any(lo % 32 and hi % 32 != 31 and hi // 32 == lo // 32 + 1 for hi, lo in ext)
    assert {(c.w, c.imm) for c in cases if c.op == Op.SEXT} >= {(31, 225), (33, 223), (255, 1)}
    for c in cases:     # value cases: every bit of a result of at most 256 bits is flipped in some odd model
        if c.rs is not None and c.w in (8, 256) and c.form in ("vv", "v"):
            rw = po.result_width(c.op, c.w, c.imm)
            flipped = {(c.rs[m] ^ po.ref(c.op, c.w, *c.operands(m))).bit_length() - 1 for m in range(1, po.M, 2)}
            assert flipped == (set(range(rw)) if rw <= 256 else set(po.flip_positions(rw))), c.name()


@pytest.mark.parametrize("group", GROUPS)
def test_oracles_agree_with_the_planted_expectations(packs, group):
    """cref over the whole grid, pyoracle on a strided sample of models; no case unsupported."""
    stride = 24
    for p in packs(group):
        v = cref.verdicts(p.tapes, p.models)
        bad = np.argwhere(v != p.expect)
        assert len(bad) == 0, f"cref disagrees with ref on {len(bad)} pairs, first: " + p.cases[bad[0][0]].describe(int(bad[0][1]))
        fh, _ = cref.first_hit(p.tapes, p.models)
        assert (fh == np.where(p.expect.any(axis=1), p.expect.argmax(axis=1), -1)).all()
        for t, c in enumerate(p.cases):
            info = compile_info(p.tapes, t)
            assert info.supported, (c.name(), info.why)
    rnd = random.Random(group)
    p = packs(group)[0]
    for t in rnd.sample(range(p.tapes.n_tapes), 60):
        for m in range(t % stride, po.M, stride):
            assert pyoracle.eval_tape(p.tapes, t, p.models, m) == p.expect[t, m], p.cases[t].describe(m)


@pytest.mark.parametrize("group", GROUPS)
def test_every_predicate_tape_has_both_outcomes(group):
    n = 0
    for c in po.group_cases(group):
        if c.rs is None and not po.constant_predicate(c):
            # (constant_predicate: by exhaustive enumeration, e.g. UMUL_NOOVFL at 1 bit is always true)
            assert c.expect.any() and not c.expect.all(), c.name()
            n += 1
    assert n or group not in ("mul", "cmp")


def _survivors(cases):
    """{(op, width, form, fault)}: applicable in some case of the form, killed by none of them."""
    applicable, killed = set(), set()
    for c in cases:
        if c.place != "hi" or c.negate:
            continue    # (placement and the NOT tape share operands and expectations with their twins)
        for f in po.faults_for(c.op, c.w, c.imm):
            key = (c.op.name, c.w, c.form, f.name)
            if po.applicable(f, c):
                applicable.add(key)
                if key not in killed and po.killed_by(c, f):
                    killed.add(key)
    return applicable, killed


@pytest.mark.parametrize("group", GROUPS)
def test_no_fault_model_survives_the_grid(group):
    applicable, killed = _survivors(po.group_cases(group))
    assert applicable and not applicable - killed, sorted(applicable - killed)[:20]


def test_fault_list_covers_the_required_families():
    names = {f.name for op in po.PREDICATES + tuple(o for ops in po.GROUPS.values() for o in ops)
             for w in (33, 160, 256) for f in po.faults_for(op, w, {Op.EXTRACT: (100, 5), Op.CONCAT: 33, Op.ZEXT: 70, Op.SEXT: 70}.get(op))}
    for needle in ("carry into bit 32 dropped", "carry into bit 160 dropped", "borrow into bit 32 dropped", "partial product (1, 2) dropped",
                   "bit 64 of the product cleared", "bit 1 wrong when the low limb is 0", "compare ignores limb 3",
                   "result not re-masked above bit 33", "sign fill stops at the next limb boundary", "shift amount's high limbs ignored",
                   "shift amount = 0 mod 32 mishandled", "shift amounts >= w not saturated", "off by one when the divisor has 5 limbs",
                   "SMOD computed as SREM", "division by 0 wrong", "MIN / -1 wrong", "<= instead of < at exactly 2^w", "off by one at 2^(w-1)",
                   "one bit lost when the field crosses two limb boundaries", "low quotient bit wrong when divisor and quotient >= 2^32",
                   "low bit wrong when the divisor >= 2^64"):
        assert any(needle in n for n in names), needle


# ---------------------------------------------------------------- baseline: the seeded fuzz workload
def _eval_tape_with(fn, nodes, consts, models, m):
    """Verdict of a tape under model m with every value op computed by ``fn(op, w, x, y, imm)``
    (``po.ref`` or a fault model); Bool connectives, arrays and lookups as in pyoracle."""
    V = []
    for nd in nodes:
        op, w, a, b, c = Op(int(nd["op"])), int(nd["width"]), int(nd["a"]), int(nd["b"]), int(nd["c"])
        if op == Op.CONST:
            r = from_words(consts[a:a + limbs(w)]) & po.mask(w)
        elif op == Op.VAR:
            r = (models.var_value(a, m) if a < models.n_vars else 0) & po.mask(max(w, 1))
        elif op in (Op.TRUE, Op.FALSE):
            r = int(op == Op.TRUE)
        elif op == Op.NOT:
            r = 1 - V[a]
        elif op in (Op.AND, Op.OR, Op.XOR, Op.IMPLIES, Op.IFF):
            r = {Op.AND: V[a] & V[b], Op.OR: V[a] | V[b], Op.XOR: V[a] ^ V[b], Op.IMPLIES: (1 - V[a]) | V[b], Op.IFF: int(V[a] == V[b])}[op]
        elif op == Op.BITE:
            r = V[b] if V[a] else V[c]
        elif op in (Op.NEG, Op.BNOT):
            r = fn(op, w, V[a], None, None)
        elif op == Op.EXTRACT:
            r = fn(op, int(nodes[a]["width"]), V[a], None, (b, c))
        elif op in (Op.ZEXT, Op.SEXT):
            r = fn(op, w - b, V[a], None, b)
        elif op == Op.CONCAT:
            r = fn(op, int(nodes[a]["width"]), V[a], V[b], int(nodes[b]["width"]))
        elif op == Op.ITE:
            r = fn(op, w, V[b], V[c], V[a])
        elif op == Op.ARRAY_VAR:
            r = ("F", a)
        elif op == Op.CONST_ARRAY:
            r = ("K", V[a])
        elif op == Op.STORE:
            r = ("S", V[a], V[b], V[c])
        elif op == Op.SELECT:
            arr = V[a]
            while arr[0] == "S" and arr[2] != V[b]:
                arr = arr[1]
            if arr[0] == "F":
                table, els = models.func_table(arr[1], m)
                r = table.get((V[b],), els)
            else:
                r = arr[3] if arr[0] == "S" else arr[1]
        elif op == Op.UF:
            table, els = models.func_table(a, m)
            r = table.get((V[b],) if c == NONE else (V[b], V[c]), els)
        else:
            r = fn(op, int(nodes[a]["width"]), V[a], V[b], None)
        V.append(r)
    return V[-1] == 1


def test_planted_grid_kills_more_faults_than_the_seeded_fuzz():
    """The fault list against ``fuzz_workload(100, ...)`` (the first GPU parity seed) on its first 32
    models, through verdict changes of a patched evaluator, next to the planted grid's cases of the
    same (op, width) pairs.  (EXTRACT / CONCAT / ZEXT / SEXT faults are per immediate: left out.)"""
    tb, mb = fuzz_workload(100, 60, 150, max_width=256, depth=4)
    tapes = [tb.tape_nodes(t) for t in range(tb.n_tapes)]
    models = range(32)
    base = [[_eval_tape_with(po.ref, nodes, tb.consts, mb, m) for m in models] for nodes in tapes]
    assert (np.array(base) == cref.verdicts(tb, mb)[:, :32]).all()      # the evaluator itself is right
    plain = {op for ops in po.GROUPS.values() for op in ops} - {Op.EXTRACT, Op.CONCAT, Op.ZEXT, Op.SEXT}
    uses = [{(Op(int(nd["op"])), int(nodes[int(nd["a"])]["width"]) if int(nd["op"]) in po.PREDICATES else int(nd["width"]))
             for nd in nodes if int(nd["op"]) in plain} for nodes in tapes]
    fuzz_killed = grid_killed = total = 0
    for op, w in sorted(set().union(*uses)):
        cases = [c for g, ops in po.GROUPS.items() if op in ops for c in po.group_cases(g)
                 if c.op == op and c.w == w and c.place == "hi" and not c.negate]
        if not cases:
            continue    # (a width only the fuzz's extracts and concats make, e.g. 27 bits)
        for f in po.faults_for(op, w):
            def mut(o, w_, x, y, i):
                return f.fn(o, w_, x, y, i) if (o, w_) == (op, w) else po.ref(o, w_, x, y, i)
            total += 1
            fuzz_killed += any(_eval_tape_with(mut, nodes, tb.consts, mb, m) != base[t][m]
                               for t, nodes in enumerate(tapes) if (op, w) in uses[t] for m in models)
            grid_killed += any(po.applicable(f, c) and po.killed_by(c, f) for c in cases)
    # (the rest of `total` cannot differ from the reference at their width: 1-bit products, ...)
    print(f"{total} fault models; killed by fuzz_workload(100) on 32 models: {fuzz_killed}, by the planted grid: {grid_killed}")
    assert fuzz_killed < grid_killed
