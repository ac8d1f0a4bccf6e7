"""Bail points on the GPU (gprog.h G_BAIL; gen_qsa.py BAIL handler of the P interpreter): a wave
that leaves a conjunction tape early decides what the oracle decides -- first hits and verdicts,
integer-exact against ``cref``, with bail points (the default) and without (MQ_NO_BAIL=1) -- and
the counters say what ran.  The G interpreter takes no bail points yet (a tape that reads a
ninth variable keeps its program; the G translator drops the word should it meet one): the same
tapes are checked there all the same."""
import numpy as np
import pytest

import cref
from mythril_amd import evaluator as evmod
from mythril_amd.models import ModelBatch
from mythril_amd.synth import c2_workload, random_words
from mythril_amd.tape import Tape, TapeBatch

pytestmark = pytest.mark.gpu

W = 256
M256 = (1 << 256) - 1
MODES = ["bail", "no_bail"]


def _bail_words(prog):
    """Second words of the program's bail points (gprog.h: G_BAIL = 35; ops with a second word)."""
    out, i = [], 0
    while i < len(prog):
        op = int(prog[i]) & 0xFF
        i += 1
        if op in (56, 57, 58, 60, 61, 32, 33, 34, 35):
            if op == 35:
                out.append(int(prog[i]))
            i += 1
    return out


def _model_value(words, v, m):
    return sum(int(x) << (32 * i) for i, x in enumerate(words[8 * v:8 * v + 8, m]))


def _set_mode(monkeypatch, mode):
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)
    if mode == "no_bail":
        monkeypatch.setenv("MQ_NO_BAIL", "1")
    else:
        monkeypatch.delenv("MQ_NO_BAIL", raising=False)


def _check(evaluator, tb, mb):
    """First hits and verdicts of tb against the oracle; returns the compiled tapes (caller frees)."""
    assert evaluator.asm_ready, "the assembly interpreters did not come up: nothing here would run a bail point"
    evaluator.upload_models(mb)
    ct = evaluator.compile(tb)
    assert ct.n_unsupported == 0
    fh_ref, _ = cref.first_hit(tb, mb)
    fh = evaluator.first_hit(ct)
    assert (fh == fh_ref).all(), np.flatnonzero(fh != fh_ref)[:10]
    v, fh2 = evaluator.verdicts(ct)
    assert (v == cref.verdicts(tb, mb)).all()
    assert (fh2 == fh_ref).all()
    return ct, fh_ref


# ---------------------------------------------------------------- C2: ragged tiles, clamped lanes
_C2 = {}


def _c2(m):
    if m not in _C2:
        _C2[m] = c2_workload(60, m, seed=11, planted_frac=0.5)
    return _C2[m]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 63, 64, 65, 256, 257, 700])
def test_c2_first_hits_and_verdicts(evaluator, monkeypatch, m, mode):
    _set_mode(monkeypatch, mode)
    tb, mb, exp = _c2(m)
    ct, fh_ref = _check(evaluator, tb, mb)
    try:
        assert (fh_ref == exp).all()
        # C2 runs on the P interpreter, through the BAIL handler exactly when it is on
        assert ct.asm_split()[0] == tb.n_tapes
        assert (ct.handler_histogram(0).get("BAIL", 0) > 0) == (mode == "bail")
    finally:
        ct.free()


# ---------------------------------------------------------------- hand-built conjunctions
class _Build:
    """Conjuncts over 256-bit variables with their value under one model tracked in Python, so a
    tape can be planted: every EQ holds exactly at that model (its constant is chosen there; at
    any other model it holds with probability 2^-256), every ULT at least there."""

    def __init__(self, t, vals, planted, rng):
        self.t, self.vals, self.planted, self.rng = t, vals, planted, rng

    def var(self, i):
        return self.t.var(i, W), self.vals[i]

    def mul(self, a, b):
        return self.t.mul(a[0], b[0]), (a[1] * b[1]) & M256

    def add(self, a, b):
        return self.t.add(a[0], b[0]), (a[1] + b[1]) & M256

    def eq(self, a):
        c = a[1] if self.planted else int.from_bytes(self.rng.bytes(32), "little")
        return self.t.eq(a[0], self.t.const(c, W))

    def ult(self, a, b):
        if a[1] >= b[1]:
            a, b = b, a
        if a[1] == b[1]:
            b = self.add(b, (self.t.const(1, W), 1))
        return self.t.ult(a[0], b[0])


def _four(b, extra_var=None):
    """ULT, EQ (dear), EQ (cheap), ULT; extra_var: a ninth variable in the last conjunct (a tape
    that reads one is not the P interpreter's: it runs on G)."""
    v = b.var
    last = b.mul(b.mul(v(6), v(2)), v(0))
    if extra_var is not None:
        last = b.add(last, v(extra_var))
    return [b.ult(b.mul(v(1), v(5)), b.add(v(2), v(3))),
            b.eq(b.mul(b.mul(v(3), v(4)), b.add(v(5), v(6)))),
            b.eq(b.add(b.mul(v(0), v(1)), v(2))),
            b.ult(last, b.add(v(4), v(7)))]


def _hand_built(n_vars, m, seed):
    """Tapes over n_vars variables and m models: the 4-conjunct tape satisfied only by model 0
    (lane 0), 63 (lane 63), m - 1 (the one lane of the last wave when m = 65) or none; the EQ
    written last; a balanced And(And(a, b), And(c, d)); conjuncts sharing a temp."""
    rng = np.random.Generator(np.random.PCG64(seed))
    words = random_words(rng, 8 * n_vars, m)
    mb = ModelBatch([W] * n_vars, words)
    extra = 8 if n_vars > 8 else None

    def vals(p):
        return [_model_value(words, i, 0 if p is None else p) for i in range(n_vars)]

    tapes, want = [], []
    for p in (0, 63, m - 1, None):
        t = Tape()
        tapes.append(t.finish(t.and_(*_four(_Build(t, vals(p), p is not None, rng), extra))))
        want.append(-1 if p is None else p)
    for p in (17, None):                     # the EQ conjunct written last
        t = Tape()
        b = _Build(t, vals(p), p is not None, rng)
        c = _four(b, extra)
        tapes.append(t.finish(t.and_(c[0], c[3], c[2])))
        want.append(-1 if p is None else p)
    for p in (64 if m > 64 else 1, None):    # balanced
        t = Tape()
        c = _four(_Build(t, vals(p), p is not None, rng), extra)
        tapes.append(t.finish(t.and_(t.and_(c[0], c[1]), t.and_(c[2], c[3]))))
        want.append(-1 if p is None else p)
    for p in (33, None):                     # two conjuncts share a product (an LDS temp)
        t = Tape()
        b = _Build(t, vals(p), p is not None, rng)
        sh = b.mul(b.mul(b.var(0), b.var(1)), b.var(2))
        tail = b.add(sh, b.var(extra)) if extra is not None else b.add(sh, b.var(7))
        tapes.append(t.finish(t.and_(b.ult(b.add(sh, b.var(3)), b.mul(b.var(4), b.var(5))),
                                     b.eq(b.add(b.mul(sh, b.var(6)), b.var(5))),
                                     b.ult(tail, b.mul(b.var(6), b.var(6))))))
        want.append(-1 if p is None else p)
    return TapeBatch(tapes), mb, np.array(want, np.int32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_vars", [8, 9], ids=["P", "G"])
def test_hand_built_conjunctions(evaluator, monkeypatch, n_vars, mode):
    """n_vars = 8: the P interpreter (BAIL handler); 9: the same tapes reading a ninth variable,
    which forces them onto G."""
    _set_mode(monkeypatch, mode)
    tb, mb, want = _hand_built(n_vars, 65, seed=5)
    if mode == "bail":   # (bail points only for tapes over the P interpreter's eight variables)
        assert all(bool(_bail_words(evmod.tape_program(tb, t))) == (n_vars == 8) for t in range(tb.n_tapes))
    ct, fh_ref = _check(evaluator, tb, mb)
    try:
        assert (fh_ref == want).all(), (fh_ref, want)
        on_p, on_g, live = ct.asm_split()
        assert live and (on_p, on_g) == ((tb.n_tapes, 0) if n_vars == 8 else (0, tb.n_tapes))
        if n_vars == 8:
            assert (ct.handler_histogram(0).get("BAIL", 0) > 0) == (mode == "bail")
    finally:
        ct.free()


# ---------------------------------------------------------------- counters
def test_counters_on_one_wave(evaluator, monkeypatch):
    """One 64-model wave, early exit off, tapes no model satisfies (every wave bails at the first
    bail point): pairs and node_evals count decided pairs x |tape| in both modes; alg_ops counts
    executed ops -- pairs x the tape's prefix (its cost less the first bail's second word) with
    bail points, pairs x the tape's cost without."""
    tb, mb, exp = c2_workload(40, 64, seed=23, planted_frac=0.0)
    assert (exp == -1).all()
    stats = {}
    assert evaluator.asm_ready, "the assembly interpreters did not come up: nothing here would run a bail point"
    evaluator.upload_models(mb)
    evaluator.set_option(evaluator.OPT_EARLY_EXIT, 0)
    try:
        for mode in MODES:
            _set_mode(monkeypatch, mode)
            fh, st = evaluator.first_hit(tb, with_stats=True)
            assert (fh == -1).all()
            stats[mode] = st
    finally:
        evaluator.set_option(evaluator.OPT_EARLY_EXIT, 1)
    _set_mode(monkeypatch, "bail")
    total = prefix = 0.0
    for t in range(tb.n_tapes):
        ops = evmod.tape_alg_ops(tb, t)
        total += ops
        prefix += ops - _bail_words(evmod.tape_program(tb, t))[0]
    a, b = stats["bail"], stats["no_bail"]
    print(f"pairs {a.pairs_evaluated} / {b.pairs_evaluated}, node_evals {a.node_evals} / {b.node_evals}, "
          f"alg_ops {a.alg_ops} / {b.alg_ops} (prefix x 64 = {64 * prefix}, total x 64 = {64 * total})")
    assert a.pairs_evaluated == b.pairs_evaluated == 64 * tb.n_tapes
    assert a.node_evals == b.node_evals == 64.0 * float(tb.sizes().sum())
    assert b.alg_ops == 64 * total
    assert a.alg_ops == 64 * prefix
    assert a.alg_ops <= b.alg_ops


# ---------------------------------------------------------------- G: EVM-shaped conjunctions
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hoist", [False, True], ids=["unhoisted", "hoisted"])
def test_c3_on_g(evaluator, monkeypatch, hoist, mode):
    """synth_evm.c3_workload(40, 700), as built and with batch-level hoisting, against the oracle
    on the unhoisted batch."""
    _set_mode(monkeypatch, mode)
    exp = _c3(False)[2]
    tb, mb, _, _ = _c3(hoist)
    ref_fh, ref_v = _c3_ref()
    evaluator.upload_models(mb)
    ct = evaluator.compile(tb)
    try:
        assert ct.n_unsupported == 0
        assert (evaluator.first_hit(ct) == ref_fh).all()
        v, fh = evaluator.verdicts(ct)
        assert (v == ref_v).all() and (fh == ref_fh).all()
        assert (ref_fh == exp).all()
    finally:
        ct.free()


_C3 = {}


def _c3(hoist):
    from mythril_amd.synth_evm import c3_workload
    if hoist not in _C3:
        _C3[hoist] = c3_workload(40, 700, seed=3, planted_frac=0.3, hoist=hoist)
    return _C3[hoist]


def _c3_ref():
    if "ref" not in _C3:
        ptb, pmb, _, _ = _c3(False)
        _C3["ref"] = (cref.first_hit(ptb, pmb)[0], cref.verdicts(ptb, pmb))
    return _C3["ref"]
