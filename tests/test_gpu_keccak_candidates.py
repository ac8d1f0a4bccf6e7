"""Keccak sites on the GPU (mq_models_upload_derived_keccak; derive_keccak_sites_kernel and the third
segment of derive_table_ptr_kernel / derive_table_entries_kernel / derive_table_dense_kernel): the
tables the device builds are, word for word, what a plain upload of the materialised batch leaves
resident; on forks over a mapping key every query hits a generated candidate with the sites and
none does without them; assembly on and off agree; the drop-in path keeps those forks alive.

Shapes (keccak_candidates_util.k_case): 37 base models (or none: src = -1), blocks of 37 candidates
so 64-wide waves straddle blocks, K = 259, 518 and 475 (M = 512: two full chunks per scan thread
boundary), inputs of 256, 512 and 1088 bits (the last exactly one rate block), two sites of one
function in a block, a block without an active site, a function that stays dense and one a site
pushes past the dense limit."""
import numpy as np
import pytest

import cref
import term_eval
from derivation_util import mask_rows
from mythril_amd import support as sp
from mythril_amd.candidates import CandidateGenerator
from mythril_amd.evaluator import EvaluatorError
from mythril_amd.synth_evm import token_fork_workload
from table_derivation_util import dense_e

from keccak_candidates_util import N_LRU, k_case, k_idle_case

pytestmark = pytest.mark.gpu


def _same_tables(a, b):
    for name in ("entry_ptr", "entry_words", "else_words", "dense_words", "info"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape, name
        bad = np.argwhere(x != y)
        assert len(bad) == 0, (name, bad[:8].tolist())


# ---------------------------------------------------------------- 1. resident tables
@pytest.mark.parametrize("n_lru,K", [(N_LRU, 259), (N_LRU, 518), (N_LRU, 475), (0, 130)])
def test_keccak_derived_tables_equal_the_plain_upload(evaluator, monkeypatch, n_lru, K):
    monkeypatch.delenv("MQ_NO_DENSE_TABLES", raising=False)
    sets, _, _, _ = k_case(n_lru, K)
    cs = sets[2]
    hb = sets[0].host_batch()
    M = n_lru + K
    if K == 475:
        assert M % evaluator.lib.mq_table_scan_threads() == 0      # every scan thread owns a full chunk
    evaluator.upload_models(hb)
    plain, plain_vars = evaluator.download_funcs(), evaluator.download_vars()
    n_t, n_k = evaluator.table_uploads, evaluator.keccak_uploads
    evaluator.upload_models_derived(cs.batch, cs.derivation, cs.table_derivation, cs.keccak_sites)
    assert (evaluator.table_uploads, evaluator.keccak_uploads) == (n_t + 1, n_k + 1) and evaluator.n_models == M
    derived = evaluator.download_funcs()
    # the plain upload holds what the host built ...
    n_ew = len(hb.entry_words)
    assert (plain.entry_ptr == hb.entry_ptr).all() and (plain.else_words == hb.else_words).all()
    assert (plain.entry_words[:n_ew] == hb.entry_words).all() and not plain.entry_words[n_ew:].any()
    # ... keccak256_256 and its inverse dense; with base models the slices of keccak256_512-1 are
    # dense without the sites (16 entries) and pushed past the limit by the 17th
    names = cs.syms.func_names
    want = [dense_e(hb.funcs[f], hb.entry_ptr[f], M) for f in range(len(names))]
    assert plain.info[:, 1].tolist() == want
    assert want[names.index("keccak256_256")] > 0 and want[names.index("keccak256_256-1")] > 0
    if n_lru:
        f = names.index("keccak256_512-1@@0:256")
        without = k_case(n_lru, K, False)[0][0].host_batch()
        assert dense_e(hb.funcs[f], without.entry_ptr[f], M) == 16 and want[f] == 0
        assert int(np.diff(hb.entry_ptr[f]).max()) == 17
    assert plain.info[:, 3].tolist() == [int(np.diff(hb.entry_ptr[f]).max()) for f in range(len(names))]
    # ... and the derived upload holds the same
    _same_tables(derived, plain)
    assert (evaluator.download_vars() == plain_vars).all()
    assert (plain_vars == mask_rows(hb.var_words, hb.var_widths)).all()


def test_sites_without_an_active_block_equal_the_plain_upload(evaluator):
    """Sites in the batch, none activated by any block: nothing is hashed, no entry appended."""
    sets, _, _, _ = k_idle_case()
    cs = sets[2]
    assert len(cs.keccak_sites.sites) == 4 and not cs.keccak_sites.active.any()
    evaluator.upload_models(sets[0].host_batch())
    plain, plain_vars = evaluator.download_funcs(), evaluator.download_vars()
    n_k = evaluator.keccak_uploads
    evaluator.upload_models_derived(cs.batch, cs.derivation, cs.table_derivation, cs.keccak_sites)
    assert evaluator.keccak_uploads == n_k + 1
    _same_tables(evaluator.download_funcs(), plain)
    assert (evaluator.download_vars() == plain_vars).all()


def test_malformed_keccak_derivation_leaves_the_resident_models(evaluator):
    sets, _, _, _ = k_case(N_LRU, 259)
    cs = sets[2]
    evaluator.upload_models(sets[0].host_batch())
    before = evaluator.download_funcs()
    site = cs.keccak_sites.sites[0]
    keep = site.b
    site.b = 193
    try:
        with pytest.raises(EvaluatorError):
            evaluator.upload_models_derived(cs.batch, cs.derivation, cs.table_derivation, cs.keccak_sites)
    finally:
        site.b = keep
    _same_tables(evaluator.download_funcs(), before)


# ---------------------------------------------------------------- 2. first hits
def test_token_forks_hit_generated_candidates_only_with_the_sites(evaluator):
    exprs, recs, _ = token_fork_workload(12, 20, seed=43)
    eng = sp.VerdictEngine(evaluator)
    n_k = evaluator.keccak_uploads
    fh, cs = eng.candidate_first_hits(exprs, recs, CandidateGenerator(5000, seed=3, device_rows=True, device_tables=True,
                                                                      keccak_sites=True))
    assert evaluator.keccak_uploads == n_k + 1
    tb = eng.incremental.lower(exprs)[0].to_tapes()
    hb = cs.host_batch()
    print("first hits with the sites:", fh.tolist())
    for q, h in enumerate(fh.tolist()):
        assert h >= cs.n_lru, (q, h)                          # every query hits at a generated index
        assert cref.eval_tape(tb, q, hb, h) == 1
        assert term_eval.is_true(exprs[q], cs.materialize(h))
        assert cref.first_hit(tb.subset([q]), hb.shard(0, h))[0][0] == -1    # nothing before it
    # the same call without the sites: no candidate answers these queries
    eng = sp.VerdictEngine(evaluator)
    fh0, cs0 = eng.candidate_first_hits(exprs, recs, CandidateGenerator(5000, seed=3, device_rows=True, device_tables=True))
    print("first hits without:", fh0.tolist())
    assert cs0.batch.n_models == cs.batch.n_models and (fh0 == -1).all()


# ---------------------------------------------------------------- 3. assembly on and off
def test_verdicts_agree_with_assembly_on_and_off(evaluator):
    sets, _, db, _ = k_case(N_LRU, 259)
    cs = sets[2]
    tb = db.to_tapes()
    oracle = cref.verdicts(tb, sets[0].host_batch())
    assert oracle[:, N_LRU:].any(axis=1).all()
    evaluator.upload_models_derived(cs.batch, cs.derivation, cs.table_derivation, cs.keccak_sites)
    prev = evaluator.option(evaluator.OPT_USE_ASM, 1)
    got = []
    try:
        for on in (True, False):
            evaluator.use_asm(on)
            ct = evaluator.compile(tb)
            try:
                got.append((evaluator.verdicts(ct), evaluator.first_hit(ct)))
            finally:
                ct.free()
    finally:
        evaluator.use_asm(bool(prev))
    (v_on, fhv_on), fh_on = got[0]
    (v_off, fhv_off), fh_off = got[1]
    assert (v_on == oracle).all() and (v_off == oracle).all()
    assert (fh_on == fh_off).all() and (fhv_on == fhv_off).all()
    assert (fh_on == cref.first_hit(tb, sets[0].host_batch())[0]).all()


# ---------------------------------------------------------------- 4. the drop-in path
def test_is_possible_batch_keeps_the_token_forks_alive_only_with_the_flag(monkeypatch):
    exprs, recs, _ = token_fork_workload(8, 10, seed=44)

    def run(flag):
        monkeypatch.setenv("MQ_DEVICE_CANDIDATES", "2")
        if flag:
            monkeypatch.setenv("MQ_CANDIDATE_KECCAK", "1")
        else:
            monkeypatch.delenv("MQ_CANDIDATE_KECCAK", raising=False)
        sp.reset_caches()
        sp.args.quick_sat_candidates = True
        try:
            for m in reversed(recs):
                sp.model_cache.put(m, 1)
            sp.set_solver_backend(sp.NoSolver())
            got = sp.is_possible_batch([sp.Constraints(list(e.args)) for e in exprs])
            return got, sp.counters["candidate_answers"]
        finally:
            sp.args.quick_sat_candidates = False
            sp.set_solver_backend(None)
            sp.reset_caches()
    got, answers = run(True)
    assert all(got) and answers > 0
    got, answers = run(False)
    assert not any(got) and answers == 0
