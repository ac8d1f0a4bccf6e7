"""Derived function tables on the GPU (mq_models_upload_derived_tables; derive_table_ptr_kernel,
derive_table_entries_kernel, derive_table_else_kernel, derive_table_dense_kernel): the tables the
device builds from the base models' tables and the blocks' additions are, word for word, what a
plain upload of the materialised batch leaves resident, and every verdict read from them agrees.

Shapes (table_derivation_util.x_case): 3 (or 0) base models with 0, 1 and 3 entries of a dense
one-argument function and 0, 1 and 17 of a two-argument one, K = 130 derived models in blocks of 64,
65 and 1 that add two entries to one function, one to each, and none."""
from types import SimpleNamespace

import numpy as np
import pytest

import cref
import term_eval
from derivation_util import mask_rows
from mythril_amd import candidates as C
from mythril_amd import support as sp
from mythril_amd.evaluator import EvaluatorError
from mythril_amd.models import FuncSpec, ModelBatch
from mythril_amd.synth import fuzz_workload
from mythril_amd.synth_evm import fork_workload
from mythril_amd.tape import Tape, TapeBatch
from table_derivation_util import (X_ABSENT_KEY, X_BASE_KEY, X_FUNCS, X_KEY, X_KEY2, X_PABSENT_KEY, X_PKEY, X_SIZES, X_WIDTHS,
                                   dense_e, x_case)
from derivation_util import T_BIG

pytestmark = pytest.mark.gpu

_cases = {}


def case(n_base):
    """(materialised set, derived set, tapes, oracle verdicts), built once."""
    if n_base not in _cases:
        ref, _ = x_case(n_base)
        cs, _ = x_case(n_base, True, True)
        tb = _tapes(ref.batch, n_base)
        _cases[n_base] = (ref, cs, tb, cref.verdicts(tb, ref.batch))
    return _cases[n_base]


def _tapes(mb, n_base):
    """Selects on the one-argument table (added key, base-only key, absent key: the else value), UF
    lookups on the two-argument table (added pair, absent pair), table entry == derived column for
    every derived variable, and a tape true on the last candidate only.  Without base models
    nobody holds the base-only key, and every else value is 0."""
    tapes = []

    def cd(key):
        return t.select(t.array_var(0, 8), t.const(key, 256))

    def power(pair):
        return t.uf(1, 256, t.const(pair[0], 256), t.const(pair[1], 256))
    for key, want in ((X_KEY, 0xA7), (X_KEY, 0x40), (X_BASE_KEY, 0x77 if n_base else 0), (X_ABSENT_KEY, 2 if n_base else 0)):
        t = Tape()
        tapes.append(t.finish(t.eq(cd(key), t.const(want, 8))))
    for pair, want in ((X_PKEY, T_BIG), (X_PABSENT_KEY, (2 << 130) if n_base else 0)):
        t = Tape()
        tapes.append(t.finish(t.eq(power(pair), t.const(want, 256))))
    t = Tape()
    tapes.append(t.finish(t.eq(cd(X_KEY), t.var(1, 8))))
    t = Tape()
    tapes.append(t.finish(t.and_(t.eq(cd(X_KEY2), t.var(5, 8)), t.eq(t.band(t.var(5, 8), t.const(0x7E, 8)), t.const(0x2B << 1, 8)))))
    t = Tape()
    tapes.append(t.finish(t.and_(t.eq(power(X_PKEY), t.var(3, 256)), t.eq(t.var(3, 256), t.const(T_BIG, 256)))))
    t = Tape()
    last = mb.n_models - 1
    tapes.append(t.finish(t.eq(t.var(4, 512), t.const(mb.var_value(4, last), 512))))
    return TapeBatch(tapes)


@pytest.fixture
def asm_mode(evaluator, request):
    prev = evaluator.option(evaluator.OPT_USE_ASM, 1)
    evaluator.use_asm(bool(request.param))
    yield request.param
    evaluator.use_asm(bool(prev))


def _same_tables(a, b):
    for name in ("entry_ptr", "entry_words", "else_words", "dense_words", "info"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape, name
        bad = np.argwhere(x != y)
        assert len(bad) == 0, (name, bad[:8].tolist())


def _resident_tables_equal(evaluator, monkeypatch, n_base, no_dense):
    ref, cs, _, _ = case(n_base)
    if no_dense:
        monkeypatch.setenv("MQ_NO_DENSE_TABLES", "1")
    else:
        monkeypatch.delenv("MQ_NO_DENSE_TABLES", raising=False)
    evaluator.upload_models(ref.batch)
    plain, plain_vars = evaluator.download_funcs(), evaluator.download_vars()
    seq, n = evaluator.upload_seq, evaluator.table_uploads
    evaluator.upload_models_derived(cs.batch, cs.derivation, cs.table_derivation)
    assert evaluator.upload_seq == seq + 1 and evaluator.table_uploads == n + 1
    assert evaluator.n_models == n_base + sum(X_SIZES)
    derived = evaluator.download_funcs()
    # the plain upload holds what the host built ...
    a = ref.batch
    n_ew = len(a.entry_words)
    assert (plain.entry_ptr == a.entry_ptr).all() and (plain.else_words == a.else_words).all()
    assert (plain.entry_words[:n_ew] == a.entry_words).all() and not plain.entry_words[n_ew:].any()
    assert len(plain.entry_words) - n_ew >= 512
    M = a.n_models
    want_dense = [0 if no_dense else dense_e(X_FUNCS[f], a.entry_ptr[f], M) for f in range(2)]
    assert plain.info[:, 1].tolist() == want_dense and (want_dense[0] > 0) == (not no_dense) and want_dense[1] == 0
    assert plain.info[:, 3].tolist() == [int(np.diff(a.entry_ptr[f]).max()) for f in range(2)]
    assert (len(plain.dense_words) > 0) == (not no_dense)
    # ... and the derived upload holds the same
    _same_tables(derived, plain)
    assert (evaluator.download_vars() == plain_vars).all()
    assert (plain_vars == mask_rows(a.var_words, X_WIDTHS)).all()


@pytest.mark.parametrize("n_base", [3, 0])
def test_derived_tables_equal_the_plain_upload(evaluator, monkeypatch, n_base):
    _resident_tables_equal(evaluator, monkeypatch, n_base, False)


def test_derived_tables_equal_the_plain_upload_without_dense_tables(evaluator, monkeypatch):
    _resident_tables_equal(evaluator, monkeypatch, 3, True)


@pytest.mark.parametrize("asm_mode", [1, 0], indirect=True)
@pytest.mark.parametrize("n_base", [3, 0])
def test_verdicts_and_first_hits_equal_the_plain_upload(evaluator, n_base, asm_mode):
    ref, cs, tb, oracle = case(n_base)
    assert oracle.any(axis=1).all()                  # every tape is true somewhere ...
    assert oracle[:, n_base:].any(axis=1).all()      # ... also on a derived candidate
    assert np.flatnonzero(oracle[-1]).tolist() == [ref.batch.n_models - 1]   # the last tape: the last candidate only
    evaluator.upload_models(ref.batch)
    ct = evaluator.compile(tb)
    try:
        v_plain, fh_v_plain = evaluator.verdicts(ct)
        fh_plain = evaluator.first_hit(ct)
    finally:
        ct.free()
    evaluator.upload_models_derived(cs.batch, cs.derivation, cs.table_derivation)
    ct = evaluator.compile(tb)
    try:
        v_der, fh_v_der = evaluator.verdicts(ct)
        fh_der = evaluator.first_hit(ct)
    finally:
        ct.free()
    assert (v_plain == oracle).all()
    assert (v_der == v_plain).all()
    assert (fh_der == fh_plain).all() and (fh_v_der == fh_v_plain).all()
    assert (fh_der == cref.first_hit(tb, ref.batch)[0]).all()


def test_scan_boundaries(evaluator):
    """One function over M = 3 * (threads - 1) + 2 models: every thread of the scan owns a chunk of
    three models but the last, whose chunk is partial (two).  Per-model entry counts cycle through
    0..3 (5 base models with 0, 1, 2, 3 and 0 entries; blocks of 7, every other one adding an
    entry).  entry_ptr and the entry words only."""
    T = evaluator.lib.mq_table_scan_threads()
    M, n_base = 3 * (T - 1) + 2, 5
    assert -(-M // T) == 3 and M - 3 * (T - 1) == 2 and M < 10_000
    widths, funcs = [8, 8], [FuncSpec(1, 8, (256,))]
    models = [{"vars": {0: m, 1: 0x10 + m}, "funcs": {0: ({100 + i: (16 * m + i) & 0xFF for i in range(c)}, m)}}
              for m, c in enumerate([0, 1, 2, 3, 0])]
    lru = ModelBatch.from_python(widths, models, funcs)
    syms = SimpleNamespace(var_widths=widths, derived={1: ("f", (77,))}, func_names=["f"])
    K = M - n_base
    blocks, k = [], 0
    while k < K:
        n = min(7, K - k)
        ks = np.arange(k, k + n)
        if len(blocks) % 2:
            blocks.append((((1, 0, 8, len(blocks) & 0xFF),), ks % 3))        # 0..2 base entries + 1 added
        else:
            blocks.append((((0, 0, 4, len(blocks) & 0xF),), ks % 4))         # 0..3 base entries
        k += n
    ref = C.CandidateGenerator()._serialize(lru, blocks, syms, models)
    cs = C.CandidateGenerator(device_rows=True, device_tables=True)._serialize(lru, blocks, syms, models)
    counts = np.diff(ref.batch.entry_ptr[0])
    assert counts.min() == 0 and counts.max() == 3 and len(counts) == M
    evaluator.upload_models(ref.batch)
    plain = evaluator.download_funcs()
    evaluator.upload_models_derived(cs.batch, cs.derivation, cs.table_derivation)
    derived = evaluator.download_funcs()
    assert (plain.entry_ptr == ref.batch.entry_ptr).all()
    bad = np.argwhere(derived.entry_ptr != plain.entry_ptr)
    assert len(bad) == 0, bad[:8].tolist()
    bad = np.argwhere(derived.entry_words != plain.entry_words)
    assert len(bad) == 0, bad[:8].tolist()
    assert (derived.entry_words[:len(ref.batch.entry_words)] == ref.batch.entry_words).all()


def _same_answer(a, b):
    if a is False or b is False:
        return a is b
    if hasattr(a, "assignment") and hasattr(b, "assignment"):
        return a is b or (a.assignment == b.assignment and a.functions == b.functions)
    return a is b


def test_model_cache_takes_the_table_path_and_every_hit_rechecks(evaluator, monkeypatch):
    exprs, recs, _ = fork_workload(6, 10, seed=13)
    budget = sp.args.quick_sat_candidate_budget
    sp.args.quick_sat_candidate_budget = 2_000

    def run(mode):
        if mode is None:
            monkeypatch.delenv("MQ_DEVICE_CANDIDATES", raising=False)
        else:
            monkeypatch.setenv("MQ_DEVICE_CANDIDATES", mode)
        mc = sp.ModelCache(sp.VerdictEngine(evaluator))
        for m in reversed(recs):
            mc.put(m, 1)
        return mc.candidates(exprs)
    try:
        n = evaluator.table_uploads
        unset = run(None)
        assert evaluator.table_uploads == n
        rows_only = run("1")
        assert evaluator.table_uploads == n
        got = run("2")
        assert evaluator.table_uploads == n + 1      # the table path was taken
    finally:
        sp.args.quick_sat_candidate_budget = budget
    assert len(got) == len(unset) == len(exprs)
    assert all(_same_answer(a, b) for a, b in zip(got, unset))
    assert all(_same_answer(a, b) for a, b in zip(rows_only, unset))
    hits = [q for q, a in enumerate(got) if a is not False]
    assert len(hits) > 0 and any(all(got[q] is not r for r in recs) for q in hits)   # generated candidates among them
    for q in hits:
        assert term_eval.is_true(exprs[q], got[q])


def test_malformed_table_derivation_leaves_the_resident_models(evaluator):
    ref, cs, tb, oracle = case(3)
    evaluator.upload_models(ref.batch)
    before = evaluator.download_funcs()
    t = cs.table_derivation
    keep = int(t.add_func[1])
    t.add_func[1] = 2
    try:
        with pytest.raises(EvaluatorError):
            evaluator.upload_models_derived(cs.batch, cs.derivation, t)
    finally:
        t.add_func[1] = keep
    _same_tables(evaluator.download_funcs(), before)
    v, _ = evaluator.verdicts(tb)
    assert (v == oracle).all()
    with pytest.raises(EvaluatorError):        # a batch without tables is no plain or rows-only upload
        evaluator.upload_models_derived(cs.batch, cs.derivation)
    v, _ = evaluator.verdicts(tb)
    assert (v == oracle).all()


def test_plain_upload_after_a_table_derived_one(evaluator):
    _, cs, _, _ = case(3)
    tb, mb = fuzz_workload(5, 24, 40, max_width=512)
    evaluator.upload_models(mb)
    v_alone, fh_alone = evaluator.verdicts(tb)
    alone = evaluator.download_funcs()
    evaluator.upload_models_derived(cs.batch, cs.derivation, cs.table_derivation)
    evaluator.upload_models(mb)
    assert evaluator.n_models == mb.n_models == 40
    v, fh = evaluator.verdicts(tb)
    assert (v == v_alone).all() and (fh == fh_alone).all()
    assert (v == cref.verdicts(tb, mb)).all()
    _same_tables(evaluator.download_funcs(), alone)
    assert (evaluator.download_vars() == mask_rows(mb.var_words, mb.var_widths)).all()
