"""Derived model upload on the GPU (mq_models_upload_derived, derive_rows_kernel): the rows the
device expands from the base models and the patch tables are, bit for bit, the rows a plain upload
of the materialised batch leaves resident, and every verdict read from them agrees.

Shapes (derivation_util.table_case): 3 (or 0) base models and K = 130 derived ones in blocks of
64, 65 and 1, so one block boundary falls on a wave boundary, the other inside the last, partial
wave; Bool, 8, 33, 256 and 512-bit variables; a function entry that is a patched derived variable."""
import numpy as np
import pytest

import cref
import term_eval
from derivation_util import T_KEY, T_SIZES, T_WIDTHS, apply_derivation, mask_rows, table_case
from mythril_amd import support as sp
from mythril_amd.candidates import CandidateGenerator
from mythril_amd.evaluator import EvaluatorError
from mythril_amd.synth import fuzz_workload
from mythril_amd.synth_evm import fork_workload
from mythril_amd.tape import Tape, TapeBatch

pytestmark = pytest.mark.gpu

_cases = {}


def case(n_base):
    """(materialised set, derived set, masked expected rows, tapes, oracle verdicts), built once."""
    if n_base not in _cases:
        ref, _ = table_case(n_base, False)
        cs, _ = table_case(n_base, True)
        tb = _tapes(ref.batch, n_base)
        _cases[n_base] = (ref, cs, mask_rows(ref.batch.var_words, T_WIDTHS), tb, cref.verdicts(tb, ref.batch))
    return _cases[n_base]


def _tapes(mb, n_base):
    """Tapes that read every variable: ``var == const`` over all variables for chosen candidates
    (base models, both sides of each block boundary, the last one), the Bool variable alone, and
    selects on the patched table."""
    M = mb.n_models
    chosen = sorted({0, max(n_base - 1, 0), n_base, n_base + 63, n_base + 64, n_base + 128, n_base + 129, M - 1})
    tapes = []
    for m in chosen:
        t = Tape()
        parts = []
        for v, w in enumerate(T_WIDTHS):
            val = mb.var_value(v, m)
            if w == 0:
                parts.append(t.var(v, 0) if val & 1 else t.not_(t.var(v, 0)))
            else:
                parts.append(t.eq(t.var(v, w), t.const(val & ((1 << w) - 1), w)))
        tapes.append(t.finish(t.and_(*parts)))
    for v, w in enumerate(T_WIDTHS):      # one variable at a time (the preloaded-variable kernel's tapes)
        t = Tape()
        if w == 0:
            tapes.append(t.finish(t.var(v, 0)))
        else:
            m = n_base + 64
            tapes.append(t.finish(t.eq(t.var(v, w), t.const(mb.var_value(v, m) & ((1 << w) - 1), w))))
    for want in (0xA7, 0x40, 0x31):       # the table entry of the patched derived variable
        t = Tape()
        sel = t.select(t.array_var(0, 8), t.const(T_KEY, 256))
        tapes.append(t.finish(t.eq(sel, t.const(want, 8))))
    t = Tape()                             # table and derived column agree
    tapes.append(t.finish(t.eq(t.select(t.array_var(0, 8), t.const(T_KEY, 256)), t.var(1, 8))))
    t = Tape()
    tapes.append(t.finish(t.and_(t.var(0, 0), t.ult(t.var(2, 33), t.const(1 << 32, 33)))))
    return TapeBatch(tapes)


@pytest.fixture
def asm_mode(evaluator, request):
    prev = evaluator.option(evaluator.OPT_USE_ASM, 1)
    evaluator.use_asm(bool(request.param))
    yield request.param
    evaluator.use_asm(bool(prev))


@pytest.mark.parametrize("n_base", [3, 0])
def test_derived_rows_equal_the_plain_upload(evaluator, n_base):
    ref, cs, want, tb, _ = case(n_base)
    assert cs.derivation.n_base == n_base and cs.derivation.n_derived == sum(T_SIZES) == 130
    assert cs.derivation.block_start.tolist() == [0, 64, 129, 130]
    if n_base == 0:
        assert (cs.derivation.src == -1).all()
    assert (mask_rows(apply_derivation(cs.derivation, want.shape[0]), T_WIDTHS) == want).all()
    evaluator.upload_models(ref.batch)
    plain = evaluator.download_vars()
    seq = evaluator.upload_seq
    evaluator.upload_models_derived(cs.batch, cs.derivation)
    assert evaluator.upload_seq == seq + 1 and evaluator.n_models == n_base + 130
    derived = evaluator.download_vars()
    assert plain.shape == derived.shape == want.shape
    assert (plain == want).all()
    bad = np.argwhere(derived != want)
    assert len(bad) == 0, bad[:8].tolist()


@pytest.mark.parametrize("asm_mode", [1, 0], indirect=True)
@pytest.mark.parametrize("n_base", [3, 0])
def test_verdicts_and_first_hits_equal_the_plain_upload(evaluator, n_base, asm_mode):
    ref, cs, _, tb, oracle = case(n_base)
    assert oracle.any(axis=1).all()        # every tape is true somewhere ...
    assert oracle[:, n_base:].any()        # ... also on derived candidates
    evaluator.upload_models(ref.batch)
    ct = evaluator.compile(tb)
    try:
        v_plain, fh_v_plain = evaluator.verdicts(ct)
        fh_plain = evaluator.first_hit(ct)
    finally:
        ct.free()
    evaluator.upload_models_derived(cs.batch, cs.derivation)
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


def test_engine_takes_the_derived_upload_and_every_hit_rechecks(evaluator):
    exprs, recs, _ = fork_workload(6, 10, seed=13)
    eng = sp.VerdictEngine(evaluator)
    fh0, cs0 = eng.candidate_first_hits(exprs, recs, CandidateGenerator(2_000, seed=5))
    fh, cs = eng.candidate_first_hits(exprs, recs, CandidateGenerator(2_000, seed=5, device_rows=True))
    assert cs.derivation is not None and cs.batch.var_words is None and cs0.derivation is None
    assert (fh == fh0).all()
    gen = np.flatnonzero(fh >= cs.n_lru)
    assert len(gen) > 0
    # the rows the device derived are the rows the host would have sent
    assert (evaluator.download_vars() == mask_rows(cs.rows(), cs.batch.var_widths)).all()
    tb = eng.incremental.lower(exprs)[0].to_tapes()
    host = cs.host_batch()
    assert (host.var_words == cs0.batch.var_words).all()
    for q in gen:
        h = int(fh[q])
        assert cref.eval_tape(tb, int(q), host, h) == 1
        assert term_eval.is_true(exprs[q], cs.materialize(h))


def test_plain_upload_after_a_derived_one(evaluator):
    """Resident bookkeeping: a smaller plain batch uploaded after a derived one answers as it does
    alone (model count, rows, Bool masks, tables)."""
    _, cs, _, _, _ = case(3)
    tb, mb = fuzz_workload(5, 24, 40, max_width=512)
    evaluator.upload_models(mb)
    v_alone, fh_alone = evaluator.verdicts(tb)
    evaluator.upload_models_derived(cs.batch, cs.derivation)
    evaluator.upload_models(mb)
    assert evaluator.n_models == mb.n_models == 40
    v, fh = evaluator.verdicts(tb)
    assert (v == v_alone).all() and (fh == fh_alone).all()
    assert (v == cref.verdicts(tb, mb)).all()
    assert (evaluator.download_vars() == mask_rows(mb.var_words, mb.var_widths)).all()


def test_malformed_derivation_leaves_the_resident_models(evaluator):
    ref, cs, want, _, _ = case(3)
    evaluator.upload_models(ref.batch)
    d = cs.derivation
    keep = d.src[7]
    d.src[7] = 3
    try:
        with pytest.raises(EvaluatorError):
            evaluator.upload_models_derived(cs.batch, d)
    finally:
        d.src[7] = keep
    assert (evaluator.download_vars() == want).all()
    with pytest.raises(EvaluatorError):        # a batch without rows is no plain upload
        evaluator.upload_models(cs.batch)
    assert (evaluator.download_vars() == want).all()
