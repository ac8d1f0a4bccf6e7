"""The low-limb prefilter program of a conjunction tape (tape_compiler.cpp build_prefilter; gprog.h
PfOp), on the host: it never rejects a (tape, model) pair the oracle accepts, it is built only from
an eligible EQ conjunct (the cheapest one), the switches remove it without touching the full
programs, and its cost is the one-limb cost table's."""
import hashlib

import numpy as np
import pytest

import cref
from mythril_amd import evaluator as evmod
from mythril_amd.models import ModelBatch
from mythril_amd.synth import c2_tape, c2_workload, fuzz_workload, random_words
from mythril_amd.tape import Tape, TapeBatch

W = 256
M256 = (1 << W) - 1
N_MODELS = 257
(PF_END, PF_PUSH_VAR, PF_PUSH_K, PF_ADD, PF_SUB, PF_MUL, PF_NEG, PF_BAND, PF_BOR, PF_BXOR, PF_BNOT, PF_ADDK, PF_MULK,
 PF_ANDK, PF_ORK, PF_XORK, PF_EQ, PF_EQK) = range(18)
# SURVEY §8(d) at L = 1: a multiplication L (L + 1) = 2, every other operation L = 1, pushes 0
COST = {PF_ADD: 1, PF_SUB: 1, PF_MUL: 2, PF_NEG: 1, PF_BAND: 1, PF_BOR: 1, PF_BXOR: 1, PF_BNOT: 1, PF_ADDK: 1,
        PF_MULK: 2, PF_ANDK: 1, PF_ORK: 1, PF_XORK: 1, PF_EQ: 1, PF_EQK: 1, PF_END: 0, PF_PUSH_VAR: 0, PF_PUSH_K: 0}
MAX_INSTR, MAX_DEPTH = 48, 6   # gprog.h kPfMaxInstr, kPfMaxDepth


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in ("MQ_PREFILTER", "MQ_NO_BAIL", "MQ_G_BAIL", "MQ_BAIL_MIN_OPS"):
        monkeypatch.delenv(k, raising=False)


def run_pf(prog, mb):
    """prog_pf over uint32, all models at once: (mask of models that pass, value compared)."""
    off = mb.var_word_offsets()
    n = mb.n_models
    st = {}
    assert len(prog) % 2 == 0 and len(prog) // 2 - 1 <= MAX_INSTR
    assert int(prog[-2]) & 0xFF == PF_END
    res = left = None
    with np.errstate(over="ignore"):
        for i in range(0, len(prog) - 2, 2):
            op, d, imm = int(prog[i]) & 0xFF, (int(prog[i]) >> 8) & 0xF, np.uint32(prog[i + 1])
            assert d < MAX_DEPTH and res is None, "an instruction after the final EQ"
            if op == PF_PUSH_VAR:
                st[d] = mb.var_words[off[int(imm)]].copy()
            elif op == PF_PUSH_K:
                st[d] = np.full(n, imm, np.uint32)
            elif op == PF_ADD:
                st[d - 1] = st[d - 1] + st[d]
            elif op == PF_SUB:
                st[d - 1] = st[d - 1] - st[d]
            elif op == PF_MUL:
                st[d - 1] = st[d - 1] * st[d]
            elif op == PF_NEG:
                st[d] = np.uint32(0) - st[d]
            elif op == PF_BAND:
                st[d - 1] = st[d - 1] & st[d]
            elif op == PF_BOR:
                st[d - 1] = st[d - 1] | st[d]
            elif op == PF_BXOR:
                st[d - 1] = st[d - 1] ^ st[d]
            elif op == PF_BNOT:
                st[d] = ~st[d]
            elif op == PF_ADDK:
                st[d] = st[d] + imm
            elif op == PF_MULK:
                st[d] = st[d] * imm
            elif op == PF_ANDK:
                st[d] = st[d] & imm
            elif op == PF_ORK:
                st[d] = st[d] | imm
            elif op == PF_XORK:
                st[d] = st[d] ^ imm
            elif op == PF_EQ:
                left, res = st[d - 1], st[d - 1] == st[d]
            elif op == PF_EQK:
                left, res = st[d], st[d] == imm
            else:
                raise AssertionError(f"unknown prefilter op {op}")
    assert res is not None
    return res, left


def check_sound(tb, mb):
    """No false negatives; returns how many tapes have a prefilter."""
    v = cref.verdicts(tb, mb).astype(bool)
    n_pf = 0
    for t in range(tb.n_tapes):
        prog, ops, depth = evmod.tape_prefilter_program(tb, t)
        if len(prog) == 0:
            continue
        n_pf += 1
        assert 1 <= depth <= MAX_DEPTH
        assert ops == sum(COST[int(w) & 0xFF] for w in prog[0::2])
        passes, _ = run_pf(prog, mb)
        lost = v[t] & ~passes
        assert not lost.any(), (t, np.flatnonzero(lost)[:5])
    return n_pf


# ---------------------------------------------------------------- 1. soundness
def test_c2_tapes_planted_and_not():
    rng = np.random.Generator(np.random.PCG64(5))
    words = random_words(rng, 64, N_MODELS)
    mb = ModelBatch([W] * 8, words)
    tapes = []
    for i in range(300):
        if i % 2:
            p = int(rng.integers(N_MODELS))
            tapes.append(c2_tape(rng, [mb.var_value(v, p) for v in range(8)]))
        else:
            tapes.append(c2_tape(rng, None))
    tb = TapeBatch(tapes)
    assert cref.verdicts(tb, mb).any(axis=1).sum() >= 150
    # every C2 tape's first conjunct is EQ(a, b + c) over ADD / MUL / AND: all of them are eligible
    assert check_sound(tb, mb) == 300


@pytest.mark.parametrize("seed", [3, 4])
def test_fuzz_tapes(seed):
    tb, mb = fuzz_workload(seed, 150, N_MODELS, asm_only=True)
    check_sound(tb, mb)
    tb, mb = fuzz_workload(seed + 10, 150, N_MODELS, max_width=256, with_funcs=False)
    check_sound(tb, mb)


BIN = {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "band": lambda a, b: a & b,
       "bor": lambda a, b: a | b, "bxor": lambda a, b: a ^ b}
UN = {"neg": lambda a: -a, "bnot": lambda a: ~a}


def _operand(t, form, rng, k):
    """(node, its Python-integer value given the variables' values) of a var / const / computed operand."""
    if form == "var":
        return t.var(k, W), lambda v: v[k]
    if form == "const":
        c = int.from_bytes(rng.bytes(32), "little")
        return t.const(c, W), lambda v: c
    return t.bxor(t.var(k, W), t.var(k + 2, W)), lambda v: v[k] ^ v[k + 2]


def _one_op_cases():
    out = []
    for op in BIN:
        for fa in ("var", "const", "computed"):
            for fb in ("var", "const", "computed"):
                if fa == fb == "const":
                    continue
                out.append((op, fa, fb))
    out += [(op, f, None) for op in UN for f in ("var", "computed")]
    return out


def test_one_op_tapes_are_value_exact():
    """And(EQ(op(A, B), R), ULT(x, y)): the narrow value is lo32 of the Python-integer result."""
    rng = np.random.Generator(np.random.PCG64(9))
    words = random_words(rng, 64, N_MODELS)
    mb = ModelBatch([W] * 8, words)
    p = 200
    vals = [mb.var_value(v, p) for v in range(8)]
    tapes, expect = [], []
    for op, fa, fb in _one_op_cases():
        t = Tape()
        a, va = _operand(t, fa, rng, 0)
        if fb is None:
            node, fn = getattr(t, op)(a), (lambda v, va=va, op=op: UN[op](va(v)) & M256)
        else:
            b, vb = _operand(t, fb, rng, 1)
            node, fn = getattr(t, op)(a, b), (lambda v, va=va, vb=vb, op=op: BIN[op](va(v), vb(v)) & M256)
        tapes.append(t.finish(t.and_(t.eq(node, t.const(fn(vals), W)), t.ule(t.var(4, W), t.const(M256, W)))))
        expect.append((op, fa, fb, fn))
    tb = TapeBatch(tapes)
    assert check_sound(tb, mb) == len(tapes)
    assert cref.verdicts(tb, mb)[:, p].all()
    for t, (op, fa, fb, fn) in enumerate(expect):
        prog, _, _ = evmod.tape_prefilter_program(tb, t)
        passes, left = run_pf(prog, mb)
        assert passes[p]
        for m in (0, 1, p, N_MODELS - 1):
            want = fn([mb.var_value(k, m) for k in range(8)])
            assert int(left[m]) == want & 0xFFFFFFFF, (op, fa, fb, m)


# ---------------------------------------------------------------- 2. eligibility
def _has_pf(tape):
    return len(evmod.tape_prefilter_program(TapeBatch([tape]), 0)[0]) > 0


def _conj(build):
    t = Tape()
    return t.finish(build(t))


def test_ineligible_cones_get_no_prefilter():
    x = lambda t, k=0, w=W: t.var(k, w)   # noqa: E731
    k = lambda t, v=12345, w=W: t.const(v, w)   # noqa: E731
    ult = lambda t: t.ult(x(t, 3), x(t, 4))   # noqa: E731
    assert _has_pf(_conj(lambda t: t.and_(t.eq(t.add(x(t), x(t, 1)), k(t)), ult(t))))
    cases = {
        "sub-32-bit cone": lambda t: t.and_(t.eq(t.add(x(t, 0, 16), x(t, 1, 16)), k(t, 7, 16)), ult(t)),
        "sub-32-bit operand": lambda t: t.and_(t.eq(t.zext(W - 8, x(t, 0, 8)), k(t)), ult(t)),
        "udiv": lambda t: t.and_(t.eq(t.udiv(x(t), x(t, 1)), k(t)), ult(t)),
        "lshr": lambda t: t.and_(t.eq(t.lshr(x(t), k(t, 3)), k(t)), ult(t)),
        "ite": lambda t: t.and_(t.eq(t.ite(ult(t), x(t), x(t, 1)), k(t)), ult(t)),
        "lookup": lambda t: t.and_(t.eq(t.uf(0, W, x(t)), k(t)), ult(t)),
        "extract / concat": lambda t: t.and_(t.eq(t.concat(t.extract(127, 0, x(t)), t.extract(127, 0, x(t, 1))), k(t)), ult(t)),
        "variable index 8": lambda t: t.and_(t.eq(t.add(x(t, 8), x(t, 1)), k(t)), ult(t)),
        "root not a conjunction": lambda t: t.or_(t.eq(t.add(x(t), x(t, 1)), k(t)), ult(t)),
        "lone EQ root": lambda t: t.eq(t.add(x(t), x(t, 1)), k(t)),
        "conjunction without an EQ": lambda t: t.and_(ult(t), t.ule(x(t), x(t, 1))),
        "folds to true": lambda t: t.and_(t.eq(t.mul(x(t), k(t, 1 << 32)), k(t, 5 << 64)), ult(t)),
    }
    for name, build in cases.items():
        assert not _has_pf(_conj(build)), name


def test_cheapest_eligible_eq_is_chosen():
    def build(t):
        dear = t.eq(t.mul(t.mul(t.var(0, W), t.var(1, W)), t.var(2, W)), t.const(77, W))
        bad = t.eq(t.udiv(t.var(0, W), t.var(1, W)), t.const(3, W))
        cheap = t.eq(t.add(t.var(5, W), t.var(6, W)), t.const(99, W))
        return t.and_(dear, bad, t.ult(t.var(3, W), t.var(4, W)), cheap)
    prog, ops, depth = evmod.tape_prefilter_program(TapeBatch([_conj(build)]), 0)
    assert [int(w) & 0xFF for w in prog[0::2]] == [PF_PUSH_VAR, PF_PUSH_VAR, PF_ADD, PF_EQK, PF_END]
    assert [int(w) for w in prog[1::2]] == [5, 6, 0, 99, 0]
    assert ops == 2 and depth == 2


def test_depth_and_length_caps():
    def chain(n):
        def build(t):
            e = t.var(0, W)
            for i in range(n):
                e = t.add(t.mul(e, t.var(1 + i % 7, W)), t.var(i % 8, W))
            return t.and_(t.eq(e, t.const(1, W)), t.ult(t.var(3, W), t.var(4, W)))
        return build
    assert _has_pf(_conj(chain(10)))          # 1 + 4 * 10 + 1 = 42 instructions
    assert not _has_pf(_conj(chain(12)))      # 50 > kPfMaxInstr

    def deep(t):   # a balanced tree of 128 leaves needs 8 slots
        level = [t.var(i % 8, W) for i in range(128)]
        while len(level) > 1:
            level = [t.add(level[i], level[i + 1]) for i in range(0, len(level), 2)]
        return t.and_(t.eq(level[0], t.const(1, W)), t.ult(t.var(3, W), t.var(4, W)))
    assert not _has_pf(_conj(deep))


# ---------------------------------------------------------------- 3. switches
def _digest(tb):
    h = hashlib.sha256()
    for t in range(tb.n_tapes):
        h.update(evmod.tape_program(tb, t).tobytes())
        h.update(evmod.tape_program_g(tb, t)[0].tobytes())
    return h.hexdigest()


def test_switches(monkeypatch):
    tb, _, _ = c2_workload(40, 8, seed=7, planted_frac=0.5)
    ftb, _ = fuzz_workload(21, 40, 8, asm_only=True)
    with_pf = sum(len(evmod.tape_prefilter_program(tb, t)[0]) > 0 for t in range(tb.n_tapes))
    assert with_pf == tb.n_tapes
    on = (_digest(tb), _digest(ftb))
    monkeypatch.setenv("MQ_PREFILTER", "0")
    assert all(len(evmod.tape_prefilter_program(tb, t)[0]) == 0 for t in range(tb.n_tapes))
    assert (_digest(tb), _digest(ftb)) == on
    monkeypatch.setenv("MQ_PREFILTER", "force")
    assert all(len(evmod.tape_prefilter_program(tb, t)[0]) > 0 for t in range(tb.n_tapes))
    assert (_digest(tb), _digest(ftb)) == on
    monkeypatch.delenv("MQ_PREFILTER")
    monkeypatch.setenv("MQ_NO_BAIL", "1")
    assert all(len(evmod.tape_prefilter_program(tb, t)[0]) == 0 for t in range(tb.n_tapes))
    no_bail = (_digest(tb), _digest(ftb))
    monkeypatch.setenv("MQ_PREFILTER", "0")
    assert (_digest(tb), _digest(ftb)) == no_bail


# ---------------------------------------------------------------- 4. cost
def test_cost_is_the_one_limb_table():
    tb, _, _ = c2_workload(200, 8, seed=2, planted_frac=0.1)
    total = muls = 0
    for t in range(tb.n_tapes):
        prog, ops, _ = evmod.tape_prefilter_program(tb, t)
        assert len(prog) > 0
        kinds = [int(w) & 0xFF for w in prog[0::2]]
        assert ops == sum(COST[k] for k in kinds)
        total += len([k for k in kinds if COST[k]])
        muls += len([k for k in kinds if k in (PF_MUL, PF_MULK)])
    # C2's narrow conjunct: about ten operations, two of them multiplications
    print(f"narrow ops per tape {total / tb.n_tapes:.2f}, multiplications {muls / tb.n_tapes:.2f}")
    assert 5 <= total / tb.n_tapes <= 12
