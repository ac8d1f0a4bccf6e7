"""Bail points on the general assembly interpreter (MQ_G_BAIL=1; gen_qsa.py G BAIL handler,
qsa_translate.cpp qsa_translate): a wave that leaves a tape mid-window decides what the oracle decides
and leaves the next tape of its group intact -- first hits and verdicts integer-exact against
``cref`` with the flag on and off -- and the counters say what ran.  (The skipped-ops count of a
bail word is a word of the tape's constants, not an inline data word: what must not straddle a
window is the bail word itself, and the sweep below puts it at every window position.)"""
import numpy as np
import pytest

import cref
from mythril_amd import evaluator as evmod
from mythril_amd import support as sp
from mythril_amd.models import FuncSpec, ModelBatch
from mythril_amd.synth import random_words
from mythril_amd.tape import Tape, TapeBatch
from test_gpu_bail import _Build, _bail_words, _c3, _c3_ref, _four, _model_value

pytestmark = pytest.mark.gpu

W = 256
M256 = (1 << 256) - 1
FLAG = ["g_bail", "unset"]


def _set_flag(monkeypatch, flag):
    monkeypatch.delenv("MQ_BAIL_MIN_OPS", raising=False)
    monkeypatch.delenv("MQ_NO_BAIL", raising=False)
    if flag == "g_bail":
        monkeypatch.setenv("MQ_G_BAIL", "1")
    else:
        monkeypatch.delenv("MQ_G_BAIL", raising=False)


def _check(evaluator, tb, mb, ref, flag, want_refill=False):
    """First hits and verdicts of tb (models uploaded) against ref = (first hits, verdict matrix);
    every tape on G, through the BAIL handler exactly when the flag is on."""
    assert evaluator.asm_ready, "the assembly interpreters did not come up: nothing here would run a bail point"
    ct = evaluator.compile(tb)
    try:
        assert ct.n_unsupported == 0
        fh = evaluator.first_hit(ct)
        assert (fh == ref[0]).all(), np.flatnonzero(fh != ref[0])[:10]
        v, fh2 = evaluator.verdicts(ct)
        bad = np.argwhere(v != ref[1])
        assert not len(bad), bad[:10]
        assert (fh2 == ref[0]).all()
        on_p, on_g, live = ct.asm_split()
        assert live and (on_p, on_g) == (0, tb.n_tapes)
        hist = ct.handler_histogram(1)
        assert (hist.get("BAIL", 0) > 0) == (flag == "g_bail"), hist.get("BAIL", 0)
        if want_refill:
            assert hist.get("REFILL", 0) > 0
    finally:
        ct.free()


# ---------------------------------------------------------------- hand-built 9-variable conjunctions
_NINE = {}


def _nine(m):
    """Tapes over nine 256-bit variables and m models (the ninth variable forces them onto G):
    the EQ conjunct written last, a balanced And(And, And), two conjuncts sharing an LDS temp --
    each satisfied only by model 0, 63, m - 1 (those that exist) or by none."""
    if m in _NINE:
        return _NINE[m]
    rng = np.random.Generator(np.random.PCG64(1000 + m))
    words = random_words(rng, 8 * 9, m)
    mb = ModelBatch([W] * 9, words)
    tapes, want = [], []
    for p in sorted({q for q in (0, 63, m - 1) if q < m}) + [None]:
        vals = [_model_value(words, i, 0 if p is None else p) for i in range(9)]
        for shape in ("eq_last", "balanced", "shared"):
            t = Tape()
            b = _Build(t, vals, p is not None, rng)
            if shape == "shared":
                sh = b.mul(b.mul(b.var(0), b.var(1)), b.var(2))
                root = t.and_(b.ult(b.add(sh, b.var(3)), b.mul(b.var(4), b.var(5))),
                              b.eq(b.add(b.mul(sh, b.var(6)), b.var(5))),
                              b.ult(b.add(sh, b.var(8)), b.mul(b.var(6), b.var(6))))
            else:
                c = _four(b, 8)
                root = t.and_(c[0], c[3], c[2]) if shape == "eq_last" else t.and_(t.and_(c[0], c[1]), t.and_(c[2], c[3]))
            tapes.append(t.finish(root))
            want.append(-1 if p is None else p)
    tb = TapeBatch(tapes)
    ref = (cref.first_hit(tb, mb)[0], cref.verdicts(tb, mb))
    assert (ref[0] == np.array(want, np.int32)).all(), (ref[0], want)
    _NINE[m] = (tb, mb, ref)
    return _NINE[m]


@pytest.mark.parametrize("flag", FLAG)
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_hand_built_nine_variable_conjunctions(evaluator, monkeypatch, m, flag):
    _set_flag(monkeypatch, flag)
    tb, mb, ref = _nine(m)
    if flag == "g_bail":
        assert all(_bail_words(evmod.tape_program_g(tb, t)[0]) for t in range(tb.n_tapes))
    evaluator.upload_models(mb)
    _check(evaluator, tb, mb, ref, flag)


# ---------------------------------------------------------------- leaving mid-window
class _B(_Build):
    """_Build with constants, XOR and a table lookup (select over an array variable)."""

    def const(self, c):
        return self.t.const(c, W), c

    def bxor(self, a, b):
        return self.t.bxor(a[0], b[0]), a[1] ^ b[1]

    def big(self, n):
        """A random constant of exactly n limbs (n = 0: a 16-bit immediate)."""
        if n == 0:
            return self.const(int(self.rng.integers(1, 1 << 16)))
        c = int.from_bytes(self.rng.bytes(4 * n), "little") | (1 << (32 * n - 1))
        return self.const(c)

    def pad(self, x, words):
        """x XOR constants whose pushes and XORs take `words` G program words: a constant of n
        limbs travels as 1 + n inline words (a 16-bit one in the immediate) + 1 for the XOR."""
        assert words == 0 or words >= 2
        while words:
            step = 10 if (words >= 12 or words == 10) else 5 if words == 11 else words
            x = self.bxor(x, self.big(step - 2))
            words -= step
        return x


_WIN = {}
N_SWEEP = 70


def _window_batch():
    """>= 40 G tapes for ONE tape group (MQ_G_TPG): a program shorter than a 64-word window; one
    over three and more windows with its first bail in window 0; one whose first bail lies past
    the first REFILL; a table lookup behind the bail; and a sweep whose first conjunct grows one
    program word at a time over more than a window, so the bail word meets every position of a
    window: the last one before a REFILL and the first one after it included."""
    if _WIN:
        return _WIN["b"]
    m, nv = 130, 10
    rng = np.random.Generator(np.random.PCG64(77))
    words = random_words(rng, 8 * nv, m)
    # one array (function 0, 256 -> 256 bits): every model maps its own value of variable 2 and a
    # decoy key; anything else reads the model's else-value
    keys = [_model_value(words, 2, j) for j in range(m)]
    tab = [int.from_bytes(rng.bytes(32), "little") for _ in range(m)]
    ew = np.zeros((m, 2, 16), np.uint32)
    for j in range(m):
        for e, (k, val) in enumerate(((keys[j] ^ 1, 7), (keys[j], tab[j]))):
            ew[j, e, :8] = [(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
            ew[j, e, 8:] = [(val >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    mb = ModelBatch([W] * nv, words, funcs=[FuncSpec(1, 256, (256,))],
                    entry_ptr=(2 * np.arange(m + 1, dtype=np.int64))[None, :], entry_words=ew.reshape(-1),
                    entry_base=np.zeros(1, np.int64), else_words=random_words(rng, 1, 8 * m).reshape(-1),
                    else_base=np.zeros(1, np.int64))
    tapes = []
    plant = [0, None, 63, None, 64, None, 129, None]

    def build(k, fn):
        p = plant[k % len(plant)]
        t = Tape()
        vals = [_model_value(words, i, 0 if p is None else p) for i in range(nv)]
        b = _B(t, vals, p is not None, rng)
        b.p = 0 if p is None else p
        tapes.append(t.finish(t.and_(*fn(b))))

    def tail(b, o=0):     # >= 64 ops behind a bail point, in two stack slots; reads the tenth variable
        return b.ult(b.mul(b.mul(b.var(1 + o), b.var(2 + o)), b.var(3 + o)), b.var(9))

    for k in range(4):      # shorter than one window
        build(k, lambda b: [b.eq(b.add(b.var(0), b.var(8))), tail(b)])
    for k in range(4):      # three and more windows, the first bail in window 0
        build(k, lambda b: [b.eq(b.add(b.var(0), b.var(8)))] +
              [b.ult(b.bxor(b.var(i % 8), b.big(8)), b.add(b.mul(b.var((i + 3) % 10), b.var((i + 5) % 10)), b.big(8)))
               for i in range(12)])
    for k in range(4):      # the first bail past the first REFILL
        build(k, lambda b: [b.eq(b.pad(b.var(8), 120)), tail(b), tail(b, 1)])
    for k in range(4):      # a table lookup behind the bail
        def lookup(b):
            arr = b.t.array_var(0, 256)
            sel = (b.t.select(arr, b.var(2)[0]), tab[b.p])
            # (one use, two slots: a shared lookup would be a temp, computed before the root unit and
            # its bail; a deeper conjunct would have to stay first)
            return [b.eq(b.add(b.mul(b.var(0), b.var(1)), b.var(8))), b.ult(sel, b.var(5)), tail(b)]
        build(k, lookup)
    for k in range(N_SWEEP):   # the bail word at every window position
        build(k, lambda b, k=k: [b.eq(b.pad(b.var(8), 20 + k)), tail(b)])
    tb = TapeBatch(tapes)
    ref = (cref.first_hit(tb, mb)[0], cref.verdicts(tb, mb))
    want = np.array([-1 if plant[k % len(plant)] is None else plant[k % len(plant)]
                     for n in (4, 4, 4, 4, N_SWEEP) for k in range(n)], np.int32)
    assert (ref[0] == want).all(), (ref[0], want)
    _WIN["b"] = (tb, mb, ref)
    return _WIN["b"]


@pytest.mark.parametrize("flag", FLAG)
@pytest.mark.parametrize("launch", ["early_exit", "no_early_exit", "latency"])
def test_leaving_mid_window(evaluator, monkeypatch, launch, flag):
    """The window batch as one tape group (every bailing tape is followed by a checked one), with
    early exit on and off, and one tape per wave (latency mode)."""
    _set_flag(monkeypatch, flag)
    monkeypatch.setenv("MQ_G_TPG", "128")
    tb, mb, ref = _window_batch()
    evaluator.upload_models(mb)
    if launch == "no_early_exit":
        evaluator.set_option(evaluator.OPT_EARLY_EXIT, 0)
    if launch == "latency":
        evaluator.set_option(evaluator.OPT_LATENCY_WAVES, 1 << 20)
    try:
        _check(evaluator, tb, mb, ref, flag, want_refill=True)
    finally:
        evaluator.set_option(evaluator.OPT_EARLY_EXIT, 1)
        evaluator.set_option(evaluator.OPT_LATENCY_WAVES, 0)


# ---------------------------------------------------------------- counters
def test_counters_on_one_wave(evaluator, monkeypatch):
    """One 64-model wave, early exit off, 40 nine-variable tapes no model satisfies (every wave
    leaves at the first bail point): pairs and node_evals count decided pairs x |tape| in both
    modes; alg_ops counts executed ops -- pairs x the tape's cost without the flag, pairs x (cost
    less the first bail word of the program G ran) with it."""
    rng = np.random.Generator(np.random.PCG64(41))
    words = random_words(rng, 8 * 9, 64)
    mb = ModelBatch([W] * 9, words)
    vals = [_model_value(words, i, 0) for i in range(9)]
    tapes = []
    for k in range(40):
        t = Tape()
        c = _four(_Build(t, vals, False, rng), 8)
        tapes.append(t.finish(t.and_(*(c[k % 4:] + c[:k % 4]))))
    tb = TapeBatch(tapes)
    assert evaluator.asm_ready
    evaluator.upload_models(mb)
    evaluator.set_option(evaluator.OPT_EARLY_EXIT, 0)
    stats = {}
    try:
        for flag in FLAG:
            _set_flag(monkeypatch, flag)
            ct = evaluator.compile(tb)
            try:
                fh, st = evaluator.first_hit(ct, with_stats=True)
                assert (fh == -1).all()
                assert ct.asm_split()[:2] == (0, tb.n_tapes)
                stats[flag] = st
            finally:
                ct.free()
    finally:
        evaluator.set_option(evaluator.OPT_EARLY_EXIT, 1)
    _set_flag(monkeypatch, "g_bail")
    total = prefix = 0.0
    for t in range(tb.n_tapes):
        ops = evmod.tape_alg_ops(tb, t)
        total += ops
        prefix += ops - _bail_words(evmod.tape_program_g(tb, t)[0])[0]
    a, b = stats["g_bail"], stats["unset"]
    print(f"pairs {a.pairs_evaluated} / {b.pairs_evaluated}, node_evals {a.node_evals} / {b.node_evals}, "
          f"alg_ops {a.alg_ops} / {b.alg_ops} (prefix x 64 = {64 * prefix}, total x 64 = {64 * total})")
    assert a.pairs_evaluated == b.pairs_evaluated == 64 * tb.n_tapes
    assert a.node_evals == b.node_evals == 64.0 * float(tb.sizes().sum())
    assert b.alg_ops == 64 * total
    assert a.alg_ops == 64 * prefix
    assert a.alg_ops < b.alg_ops


# ---------------------------------------------------------------- C3 on G
@pytest.mark.parametrize("hoist", [False, True], ids=["unhoisted", "hoisted"])
def test_c3_on_g_with_bail_points(evaluator, monkeypatch, hoist):
    """synth_evm.c3_workload(40, 700, seed=3, planted_frac=0.3), as built and with batch-level
    hoisting (its mode-3 column programs carry no bail point), against the oracle on the
    unhoisted batch."""
    _set_flag(monkeypatch, "g_bail")
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
        assert ct.handler_histogram(1).get("BAIL", 0) > 0
        assert ct.handler_histogram(2).get("BAIL", 0) == 0
    finally:
        ct.free()


# ---------------------------------------------------------------- engine paths
def test_engine_whole_query_path(evaluator, monkeypatch):
    """VerdictEngine, whole-query path (conj_tapes = 0), 8 EVM-shaped queries x 70 models: the
    rows with the flag are the rows without it."""
    from mythril_amd.synth_evm import dropin_workload
    exprs, recs, planted = dropin_workload(8, 70, seed=5, query_seed=3)
    rows = {}
    for flag in FLAG:
        _set_flag(monkeypatch, flag)
        eng = sp.VerdictEngine(evaluator)
        eng.conj_tapes = 0
        rows[flag] = eng.rows(exprs, recs)
        assert eng.stats["whole_query_batches"] == 1
    assert all(r is not None for r in rows["unset"])
    assert any(r.any() for r in rows["unset"])
    for a, b in zip(rows["g_bail"], rows["unset"]):
        assert a is not None and np.array_equal(a, b)


def test_engine_candidate_first_hits(evaluator, monkeypatch):
    """VerdictEngine.candidate_first_hits on fork-pruning queries: the first hits with the flag
    are those without it."""
    from mythril_amd.candidates import CandidateGenerator
    from mythril_amd.synth_evm import fork_workload
    exprs, recs, parents = fork_workload(16, 60, seed=12)
    out = {}
    for flag in FLAG:
        _set_flag(monkeypatch, flag)
        eng = sp.VerdictEngine(evaluator)
        fh, cs = eng.candidate_first_hits(exprs, recs, CandidateGenerator(2_000, seed=5))
        out[flag] = np.asarray(fh).copy()
    assert (out["unset"] >= 0).any()
    assert np.array_equal(out["g_bail"], out["unset"])
