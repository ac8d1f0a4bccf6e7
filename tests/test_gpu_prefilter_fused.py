"""The fused narrow handlers of the low-limb prefilter on the GPU (gen_qsa.py ADD32V .. MUL32VV and
the tail NEXT_PF; qsa_translate.cpp qsa_translate_pf's peephole).  A fused handler that reads the
wrong register loses a hit, so every generated (kind, slot, variable) handler runs here on a tape
with a planted hit (pf_fused_cases; test_prefilter_translate checks on the host that those tapes
name every handler of the table): first hits are the oracle's and those of the MQ_PF_FUSE=0 and
MQ_PREFILTER=0 arms, and each tape's bitmap column is exactly the planted block."""
import re

import numpy as np
import pytest

import cref
import pf_fused_cases as fc
from test_prefilter_compile import run_pf
from mythril_amd import evaluator as evmod
from mythril_amd.models import ModelBatch
from mythril_amd.synth import c2_workload, random_words
from mythril_amd.tape import Tape, TapeBatch

pytestmark = pytest.mark.gpu

W = 256
M256 = (1 << W) - 1
FUSED_RE = re.compile(r"(ADD|SUB|MUL|EQ)32VV?|(ADD|MUL|AND|OR|XOR|EQ)K32V")


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    for k in ("MQ_NO_BAIL", "MQ_G_BAIL", "MQ_BAIL_MIN_OPS", "MQ_P_WG", "MQ_PF_WG", "MQ_PF_FUSE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MQ_PREFILTER", "force")


def _arm(evaluator, monkeypatch, tb, mb, prefilter="force", fuse=None):
    """(first hits, compiled tapes) of one arm; the caller frees."""
    monkeypatch.setenv("MQ_PREFILTER", prefilter)
    if fuse is None:
        monkeypatch.delenv("MQ_PF_FUSE", raising=False)
    else:
        monkeypatch.setenv("MQ_PF_FUSE", fuse)
    assert evaluator.asm_ready, "the assembly interpreters did not come up: no prefilter would run"
    evaluator.upload_models(mb)
    ct = evaluator.compile(tb)
    assert ct.n_unsupported == 0
    return evaluator.first_hit(ct), ct


def _three_arms(evaluator, monkeypatch, tb, mb, ref):
    """First hits of the fused, MQ_PF_FUSE=0 and MQ_PREFILTER=0 arms against the oracle; returns
    the fused arm's (compiled tapes, bitmap view, histogram) -- the caller frees -- and the
    unfused arm's (bitmap bits, histogram, entries)."""
    off, ct0 = _arm(evaluator, monkeypatch, tb, mb, "0")
    try:
        assert ct0.prefilter_split() == (0, False)
    finally:
        ct0.free()
    assert (off == ref).all(), np.flatnonzero(off != ref)[:10]
    un, ctu = _arm(evaluator, monkeypatch, tb, mb, "force", "0")
    try:
        assert ctu.prefilter_split()[1]
        unfused = (ctu.prefilter_alive()[0].copy(), ctu.handler_histogram(3), ctu.prefilter_entries())
    finally:
        ctu.free()
    assert (un == ref).all(), np.flatnonzero(un != ref)[:10]
    fh, ct = _arm(evaluator, monkeypatch, tb, mb, "force")
    assert (fh == ref).all(), np.flatnonzero(fh != ref)[:10]
    assert ct.prefilter_split()[1]
    return ct, ct.prefilter_alive(), ct.handler_histogram(3), unfused


def _check_columns(alive, tb, mb, planted, names):
    """Each tape's bitmap column: exactly the block of its planted model -- but for the tapes
    whose constant leaves limb 0 few values (x & 1, x | 0xFFFFFFFF, x * 0x80000000), where it is
    exactly the blocks in which the narrow program itself (run_pf) passes a model."""
    bits, tapes, has = alive
    assert has.all() and len(tapes) == tb.n_tapes
    for d, t in enumerate(tapes):
        got = [int(b) for b in np.flatnonzero(bits[:, d])]
        passes, _ = run_pf(evmod.tape_prefilter_program(tb, int(t))[0], mb)
        want = sorted({int(m) // 64 for m in np.flatnonzero(passes)})
        assert int(planted[t]) // 64 in want
        if " k0x" not in names[t]:
            assert want == [int(planted[t]) // 64], (names[t], want)
        assert got == want, (names[t], got, want, int(planted[t]))


_BATCH = {}


def _batch(m):
    if m not in _BATCH:
        tb, mb, planted, names = fc.fused_batch(m)
        _BATCH[m] = (tb, mb, planted, names, cref.first_hit(tb, mb)[0])
    return _BATCH[m]


@pytest.mark.parametrize("m", [130, 577])
def test_every_fused_handler_with_a_planted_hit(evaluator, monkeypatch, m):
    """m = 577: nine full blocks and one lane, so a wave's ninth block (a second wave) and a
    ragged tail both run; plants on lanes 0 and 63 of every block and on the last model."""
    tb, mb, planted, names, ref = _batch(m)
    assert (ref == planted).all(), [names[t] for t in np.flatnonzero(ref != planted)[:10]]
    assert {int(p) // 64 for p in planted} == set(range((m + 63) // 64)) and {int(p) % 64 for p in planted} >= {0, 63}
    ct, alive, hist, (ubits, uhist, uentries) = _three_arms(evaluator, monkeypatch, tb, mb, ref)
    try:
        assert ct.asm_split()[0] == tb.n_tapes and ct.prefilter_split() == (tb.n_tapes, True)
        _check_columns(alive, tb, mb, planted, names)
        assert (alive[0] == ubits).all()
        kinds, i = [], 0
        while evaluator.lib.mq_qsa_kind_name(i):
            kinds.append(evaluator.lib.mq_qsa_kind_name(i).decode())
            i += 1
        fused = {k for k in kinds if FUSED_RE.fullmatch(k)}
        assert fused == fc.FUSED, sorted(fused ^ fc.FUSED)      # (the library's kinds: none unnamed)
        assert fused | fc.UNFUSED | fc.SHARED <= set(hist), sorted((fused | fc.UNFUSED | fc.SHARED) - set(hist))
        assert not (fused & set(uhist)) and fc.UNFUSED | {"PUSH_VAR", "BNOT", "BAND", "BOR", "BXOR"} <= set(uhist)
        entries, instrs = ct.prefilter_entries()
        print(f"m {m}: {tb.n_tapes} tapes, entries {entries} of {instrs} instructions")
        assert uentries == (instrs, instrs) and entries < 0.7 * instrs
        assert sum(hist.values()) == entries + tb.n_tapes and sum(uhist.values()) == instrs + tb.n_tapes    # (+ END)
    finally:
        ct.free()


def test_m0_indexed_handlers_leave_index_mode_off(evaluator, monkeypatch):
    """The tapes that put a kindVV handler (operand addressed through M0) directly before and
    directly after every other class of handler, alone in a batch: were the index mode still on,
    the neighbour would read another variable's registers and the planted hit would be lost."""
    tb2, mb2, planted2, names2 = fc.fused_batch(577, only="m0 ")
    assert len(names2) >= 11
    ref2 = cref.first_hit(tb2, mb2)[0]
    assert (ref2 == planted2).all()
    ct, alive, hist, _ = _three_arms(evaluator, monkeypatch, tb2, mb2, ref2)
    try:
        _check_columns(alive, tb2, mb2, planted2, names2)
        assert {"ADD32VV", "SUB32VV", "MUL32VV", "NEG32", "BNOT", "ADDK32", "MULK32", "ADD32V", "BANDV", "ADD32", "BAND",
                "MULK32V", "PUSH_VAR", "SUB32", "EQ32", "EQK32"} <= set(hist), hist
    finally:
        ct.free()


def test_low_limb_collisions_on_fused_compares(evaluator, monkeypatch):
    """EQ32V and EQK32V tapes; at the fakes limb 0 of every variable is the planted model's and the
    limbs above are random: the prefilter keeps their blocks alive and P rejects them."""
    m, p = 700, 601
    rng = np.random.Generator(np.random.PCG64(73))
    words = random_words(rng, 64, m)
    fakes = [3, 64, 130, 600]
    for f in fakes:
        words[0::8, f] = words[0::8, p]
    mb = ModelBatch([W] * 8, words)
    vals = [mb.var_value(v, p) for v in range(8)]
    tapes = []
    for v in (0, 5):
        dear = lambda t: t.ule(t.mul(t.var(4, W), t.var(6, W)), t.const(M256, W))     # noqa: E731
        t = Tape()       # ... PUSH_VAR v; EQ  ->  EQ32V
        c = (vals[v] - (~vals[v + 1] & M256)) & M256
        tapes.append(t.finish(t.and_(dear(t), t.eq(t.add(t.bnot(t.var(v + 1, W)), t.const(c, W)), t.var(v, W)))))
        t = Tape()       # PUSH_VAR v; EQK  ->  EQK32V
        tapes.append(t.finish(t.and_(dear(t), t.eq(t.var(v, W), t.const(vals[v], W)))))
    tb = TapeBatch(tapes)
    ref = cref.first_hit(tb, mb)[0]
    assert list(ref) == [p] * 4
    ct, alive, hist, _ = _three_arms(evaluator, monkeypatch, tb, mb, ref)
    try:
        assert hist.get("EQ32V") == 2 and hist.get("EQK32V") == 2, hist
        bits, dtapes, has = alive
        assert has.all()
        for d in range(len(dtapes)):
            got = sorted(int(b) for b in np.flatnonzero(bits[:, d]))
            assert got == sorted({f // 64 for f in fakes} | {p // 64}), (d, got)
    finally:
        ct.free()


def test_counters_equal_the_unfused_arm(evaluator, monkeypatch):
    """Early exit off, nothing planted: pairs, node-evals and alg-ops do not depend on how the
    narrow program is cut into entries."""
    tb, mb, exp = c2_workload(40, 4096, seed=23, planted_frac=0.0)
    assert (exp == -1).all()
    stats = {}
    evaluator.set_option(evaluator.OPT_EARLY_EXIT, 0)
    try:
        for arm, fuse in (("fused", None), ("unfused", "0")):
            monkeypatch.delenv("MQ_PREFILTER", raising=False)
            fh, ct = _arm(evaluator, monkeypatch, tb, mb, "force", fuse)
            try:
                assert (fh == -1).all() and ct.prefilter_split() == (40, True)
                _, st = evaluator.first_hit(ct, with_stats=True)
                stats[arm] = (st.pairs_evaluated, st.node_evals, st.alg_ops, ct.prefilter_entries())
            finally:
                ct.free()
    finally:
        evaluator.set_option(evaluator.OPT_EARLY_EXIT, 1)
    print(stats)
    assert stats["fused"][:3] == stats["unfused"][:3]
    assert stats["fused"][0] == 4096 * tb.n_tapes
    assert stats["fused"][3][0] < stats["unfused"][3][0] == stats["unfused"][3][1]
