"""The planted lookup / array / keccak / Bool grid (planted_lookups.py) on the CPU: the reference hash
is pinned first, both oracles agree with the by-construction expectations, nothing is unsupported,
every tape has both outcomes, the table classes the grid claims are really in its tables, and no
fault model - a subtly wrong Python lookup, select, hash or connective - survives a signature it can
differ from the reference in."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import cref
import keccak_ref
import planted_lookups as pl
import pyoracle
from mythril_amd.evaluator import compile_info
from mythril_amd.tape import limbs
from planted_ops import flip_positions, mask

TAPE_GROUPS = [g for g in pl.GROUPS if g != "keccak_columns"]


# ---------------------------------------------------------------- the reference itself
def test_reference_hash_is_pinned():
    """keccak_ref's sha3_256 shares sponge and permutation with keccak256 (only the domain byte
    differs): it equals hashlib's for every length 0..300, and keccak256 reproduces the KATs."""
    for n in range(301):
        msg = bytes((i * 13 + n) & 0xFF for i in range(n))
        assert keccak_ref.sha3_256(msg) == hashlib.sha3_256(msg).digest(), n
    with open(os.path.join(os.path.dirname(__file__), "golden", "keccak_kats.json")) as f:
        kats = json.load(f)
    assert len(kats) >= 12
    for k in kats:
        assert keccak_ref.keccak256(bytes.fromhex(k["data"])).hex() == k["digest"], k["name"]
    # the helper's own sponge (the fault models' base) is the same function when nothing is wrong
    for n in (0, 1, 135, 136, 137, 256):
        d = bytes((7 * i) & 0xFF for i in range(n))
        assert pl._sponge(d) == int.from_bytes(keccak_ref.keccak256(d), "big")


def test_reference_lookup_and_select_spot_values():
    e = [((5,), 1), ((6,), 2), ((5,), 3)]
    assert pl.ref_lookup(e, 9, (5,)) == 1 and pl.ref_lookup(e, 9, (6,)) == 2 and pl.ref_lookup(e, 9, (7,)) == 9
    assert pl.ref_lookup([], 9, (0,)) == 9 and pl.ref_lookup([((1, 2), 4)], 9, (2, 1)) == 9
    base = ("var", e, 9)
    chain = ("store", ("store", base, 5, 20), 6, 10)        # store(store(a, 5, 20), 6, 10)
    assert pl.ref_select(chain, 6) == 10 and pl.ref_select(chain, 5) == 20 and pl.ref_select(chain, 7) == 9
    assert pl.ref_select(("store", ("store", base, 5, 20), 5, 10), 5) == 10        # the outermost store wins
    assert pl.ref_select(("store", ("const", 4), 1, 2), 3) == 4 and pl.ref_select(base, 5) == 1
    tt = {op: [pl.ref_bool(op, a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)] for op in pl.BOOL_OPS}
    assert tt == {"NOT": [1, 1, 1, 1, 0, 0, 0, 0], "AND": [0, 0, 0, 0, 0, 0, 1, 1], "OR": [0, 0, 1, 1, 1, 1, 1, 1],
                  "XOR": [0, 0, 1, 1, 1, 1, 0, 0], "IMPLIES": [1, 1, 1, 1, 0, 0, 1, 1], "IFF": [1, 1, 0, 0, 0, 0, 1, 1],
                  "BITE": [0, 1, 0, 1, 0, 0, 1, 1]}


def test_model_batch_builder_keeps_order_and_duplicates():
    """tables_arrays against ModelBatch.func_table (first entry of a key wins there too) and the raw
    words: duplicates stay, in order."""
    from mythril_amd.models import FuncSpec, ModelBatch
    spec = FuncSpec(2, 72, (160, 8))
    tab = pl.Table("t", spec, [[((3, 1), 7), ((3, 1), 8), ((1 << 159, 255), (1 << 72) - 1)], [], [((0, 0), 5)]], [11, 12, 1 << 71])
    funcs, ptr, ew, eb, lw, lb = pl.tables_arrays([tab], 3)
    assert ptr.tolist() == [[0, 3, 3, 4]] and len(ew) == 4 * spec.stride == 4 * 9
    assert ew[:9].tolist() == [3, 0, 0, 0, 0, 1, 7, 0, 0] and ew[9:18].tolist() == [3, 0, 0, 0, 0, 1, 8, 0, 0]
    assert lw.tolist() == [11, 0, 0, 12, 0, 0, 0, 0, 1 << 7]
    mb = ModelBatch([8], np.zeros((1, 3), np.uint32), funcs, ptr, ew, eb, lw, lb)
    assert mb.func_table(0, 0) == ({(3, 1): 7, (1 << 159, 255): (1 << 72) - 1}, 11) and mb.func_table(0, 2) == ({(0, 0): 5}, 1 << 71)


# ---------------------------------------------------------------- oracles
@pytest.mark.parametrize("group", TAPE_GROUPS)
def test_oracles_agree_with_the_planted_expectations(group):
    """cref over the whole grid, pyoracle on a sample of (tape, model) pairs; no tape unsupported."""
    rnd = random.Random(group)
    for p in pl.group_packs(group):
        v = cref.verdicts(p.tapes, p.models)
        bad = np.argwhere(v != p.expect)
        assert len(bad) == 0, f"cref disagrees with ref on {len(bad)} pairs, first: " + p.cases[bad[0][0]].describe(int(bad[0][1]))
        fh, _ = cref.first_hit(p.tapes, p.models)
        assert (fh == np.where(p.expect.any(axis=1), p.expect.argmax(axis=1), -1)).all()
        for t, c in enumerate(p.cases):
            info = compile_info(p.tapes, t)
            assert info.supported, (c.name(), info.why)
    p = pl.group_packs(group)[0]
    n = p.cases[0].n_models
    for t in rnd.sample(range(p.tapes.n_tapes), min(12, p.tapes.n_tapes)):
        for m in rnd.sample(range(n), 6 if group == "keccak" else 12):
            assert pyoracle.eval_tape(p.tapes, t, p.models, m) == p.expect[t, m], p.cases[t].describe(m)


def test_keccak_column_workload_on_the_oracle():
    """The hoisted keccak-column roots, lowered WITHOUT hoisting: cref agrees with the expectation."""
    from mythril_amd.lower import SymbolTable, lower_batch, serialize_models
    w = pl.keccak_column_workload()
    tb, syms, ok = lower_batch(w.roots, SymbolTable(interpret_keccak=True))
    assert ok.all() and len(w.roots) == 3 * len(pl.KECCAK_COLUMN_BITS) == 3 * w.n_messages
    mb = serialize_models(w.models, syms)
    v = cref.verdicts(tb, mb)
    bad = np.argwhere(v != w.expect)
    assert len(bad) == 0, w.cases[bad[0][0]].describe(int(bad[0][1]))
    tb2, _, ok2 = lower_batch(w.roots, SymbolTable(interpret_keccak=True), hoist=True)
    assert ok2.all() and tb2.columns is not None and tb2.columns.n >= w.n_messages
    assert all(c.expect.any() and not c.expect.all() for c in w.cases)


# ---------------------------------------------------------------- both outcomes
CONSTANT_BOOL_TAPES = sorted(f"{neg}bool {op} form={form} place={place}" for neg in ("", "NOT ") for place in ("hi", "lo")
                             for op, form in (("NOT", "F"), ("AND", "Fv"), ("OR", "vT"), ("IMPLIES", "vT"), ("IMPLIES", "Fv")))


@pytest.mark.parametrize("group", TAPE_GROUPS)
def test_every_tape_has_both_outcomes(group):
    """Except the connectives that are constant by construction - NOT(FALSE), AND(FALSE, v), OR(v, TRUE),
    IMPLIES(v, TRUE), IMPLIES(FALSE, v) - enumerated by name."""
    const = pl.constant_tapes(group)
    if group == "bool":
        assert sorted(const) == CONSTANT_BOOL_TAPES
    else:
        assert const == []
    for c in pl.group_cases(group):
        if c.name() not in const:
            assert c.expect.any() and not c.expect.all(), c.name()
            assert c.expect[:64].any() and not c.expect[:64].all(), c.name()      # within the first wave already


# ---------------------------------------------------------------- grid preconditions
def _labels(tab, queries):
    labs = set()
    for m in range(len(queries)):
        labs |= pl.table_labels(tab, m, queries[m])
    return labs


def test_grid_shape():
    assert pl.M == 577 and pl.M_KECCAK == 150 and pl.M_KECCAK // 64 == 2 and pl.M_KECCAK % 64
    for n in (len(pl.COUNTS_CSR), len(pl.COUNTS_DENSE), len(pl.COUNTS_WIDE), len(pl.COUNTS_UF2), pl.N_SCEN, pl.N_SCEN_WIDE,
              pl.N_ARRAY_CLASS, len(pl.KECCAK_INPUTS)):
        assert n % 2 == 1       # coprime to 2: every class meets flipped and unflipped models
    uf1 = pl.uf1_cases()
    sigs = {tuple(int(x) for x in c.sig.split("->")) for c in uf1 if "counts" not in c.sig}
    assert {k for k, _ in sigs} >= {1, 8, 32, 33, 64, 160, 256, 257, 512, 1088, 2048}
    assert {r for _, r in sigs} >= {0, 1, 8, 32, 33, 64, 160, 256, 512, 1088, 2048}
    assert sigs >= {(256, 256), (256, 8), (160, 256), (256, 0), (33, 33), (8, 256), (257, 256), (512, 256), (1088, 256), (2048, 256),
                    (256, 512), (256, 1088), (256, 2048)}
    for sig in ("256->256", "256->8", "256->0", "33->33"):
        assert {(c.form, c.place) for c in uf1 if c.sig == sig} >= {("v", "hi"), ("v", "lo"), ("k", "hi"), ("K", "hi"), ("c", "hi")}
    assert {c.sig for c in pl.uf2_cases()} == {"(256,256)->256", "(160,8)->72", "(8,256)->0", "(33,64)->160"}
    assert {c.sig for c in pl.widekey_cases()} >= {"2080->256", "2304->256", "2560->256", "4096->256", "2080->64", "4096->64"}
    arr = pl.array_cases()
    for iw, rw in ((256, 8), (256, 256), (160, 256), (8, 33), (256, 0)):
        assert {c.sig for c in arr} >= {f"{iw}->{rw} {b} depth {d}" for b in ("var", "const") for d in (0, 1, 2, 5)}
    assert {f for c in arr for f in c.form} >= set("vkc")
    assert [c.kw // 8 for c in pl.keccak_cases()] == list(range(1, 65)) + [65, 96, 127, 128, 135, 136, 137, 200, 255, 256]
    assert {c.sig for c in pl.bool_cases()} == set(pl.BOOL_OPS) and {c.place for c in pl.bool_cases()} == {"lo", "hi"}
    assert {f for c in pl.bool_cases() for f in c.form} == set("vTFc")


def test_lookup_tables_hold_the_classes_the_grid_claims():
    """Per function: every entry count of its cycle, the hit slots 0 / 6 / 7 / 8 / last, absent keys,
    near-miss entries before the hit (limb 0 equal and one bit of EVERY higher limb in turn, in the
    hit's scan round and in an earlier one; limb 0 only; the top bit only), duplicates in one round and
    across rounds; canonical keys and values; else values that differ in every limb from the hit's
    value and from the neighbouring models'; the dense condition of mq_models_upload."""
    seen = set()
    for c in pl.uf1_cases() + pl.uf2_cases() + pl.array_cases():
        if not c.tables or c.tables[0].name in seen:
            continue
        tab = c.tables[0]
        seen.add(tab.name)
        spec = tab.spec
        L = limbs(spec.arg_widths[0])
        labs = _labels(tab, c.queries)
        want = {"hit@0", "absent", "dup-same-round"}
        if "counts" in tab.name:
            assert tab.counts == ((9,) if "all counts 9" in tab.name else tuple(range(64))), tab.name
        elif spec.arity == 2:
            assert tab.counts == tuple(sorted(set(pl.COUNTS_UF2)))
            want |= {"arg0-only", "arg1-only", "swapped", "dup-later-round", "hit@6", "hit@7", "hit@8", "hit@last"}
        else:
            assert tab.counts == tuple(sorted(set(pl.COUNTS_DENSE if tab.dense else pl.COUNTS_CSR))), tab.name
            want |= {"hit@6", "hit@7", "hit@8", "hit@last", "dup-later-round", "near-limb0-only"}
            if spec.arg_widths[0] > 1:
                want.add("near-top-bit")
            if L > 1:
                want |= {"false-cand-same-round", "false-cand-earlier-round", "false-cand-absent"} | {f"near-limb{k}" for k in range(1, L)}
        assert want <= labs, (tab.name, sorted(want - labs))
        assert bool(pl.dense_expected(tab)) == tab.dense, tab.name
        rw = max(spec.result_width, 1)
        for m in range(pl.M):
            for key, val in tab.entries[m]:
                assert all(0 <= k <= mask(w) for k, w in zip(key, spec.arg_widths)) and 0 <= val <= mask(rw)
            hit = pl.ref_lookup(tab.entries[m], None, c.queries[m])
            for l in range(limbs(rw)):
                lw = min(32, rw - 32 * l)
                e = pl._limb(tab.elses[m], l)
                if lw >= 8:
                    assert e != 0 and (m == 0 or e != pl._limb(tab.elses[m - 1], l)), (tab.name, m, l)
                if lw >= 2 and hit is not None:
                    assert e != pl._limb(hit, l), (tab.name, m, l)
    # one wave whose 64 lanes all hold different counts, one where all are equal
    rag = next(c.tables[0] for c in pl.uf1_cases() if "all counts differ" in c.sig)
    for w0 in range(0, pl.M - 63, 64):
        assert len({len(rag.entries[m]) for m in range(w0, w0 + 64)}) == 64
    # the wide-key sets
    for c in pl.widekey_cases():
        tab = c.tables[0]
        labs = set()
        for m in range(pl.M):
            labs |= pl.wide_labels(tab, m, c.queries[m][0])
        assert labs >= {"n=0", "n=1", "n=2", "n=32", "n=33", "n=64", "hit@0", "hit@31", "hit@32", "hit@63", "absent", "dup", "chunk0-only",
                        "middle-chunk-only", "last-chunk-one-bit", "several-survive-to-last"}, (tab.name, sorted(labs))
        assert max(len(e) for e in tab.entries) == 64      # (more is the documented -2: left out)
    # arrays: every class in every chain, in flipped and unflipped models
    for c in pl.array_cases():
        by = {}
        for m, s in enumerate(c.classes):
            by.setdefault(s.split(" (")[0], set()).add(m % 2)
        assert set(by) == set(pl.ARRAY_CLASSES) and all(v == {0, 1} for v in by.values()), c.name()
        if c.depth >= 2:
            assert any("two-or-more" in s and s.count(",") >= 1 for s in c.classes)
            assert any("inner-only" in s and "[0" not in s and "[]" not in s for s in c.classes)


def test_planted_results_flip_every_bit():
    """Value cases: the flipped bit walks over every result bit up to 256 bits and over both sides of
    every limb boundary above; keccak: every digest bit over the group, every limb within a width."""
    for g in ("uf1", "uf2", "array", "widekey"):
        for c in pl.group_cases(g):
            if c.rs is not None:
                flipped = {(c.rs[m] ^ c.value(m, pl.REF)).bit_length() - 1 for m in range(1, c.n_models, 2)}
                assert flipped == set(flip_positions(c.rw)) and all(c.rs[m] == c.value(m, pl.REF) for m in range(0, c.n_models, 2)), c.name()
    over_all = set()
    for c in pl.keccak_cases() + tuple(pl.keccak_column_workload().cases):
        flipped = {(c.rs[m] ^ c.value(m, pl.REF)).bit_length() - 1 for m in range(1, c.n_models, 2)}
        assert {b // 32 for b in flipped} == set(range(8)), c.name()
        if c.group == "keccak":
            over_all |= flipped
        assert {pl.KECCAK_INPUTS[m % 5] for m in range(c.n_models)} == set(pl.KECCAK_INPUTS)
    assert over_all == set(range(256))


# ---------------------------------------------------------------- sensitivity
def _cells(group):
    """{(signature, fault name)}: applicable in some case of the signature / killed by one of them."""
    cases = pl.keccak_column_workload().cases if group == "keccak_columns" else pl.group_cases(group)
    applicable, killed = set(), set()
    for c in cases:
        if c.negate:
            continue        # (the NOT tape shares operands and expectation with its twin)
        for f in pl.all_faults():
            key = (c.sig, f.name)
            if f.can(c):
                applicable.add(key)
                if key not in killed and c.killed_by(f):
                    killed.add(key)
    return applicable, killed


# (fault, signature) cells per group: what DESIGN.md records
FAULT_CELLS = {"uf1": 781, "uf2": 110, "array": 470, "widekey": 197, "keccak": 81, "keccak_columns": 10, "bool": 9}


@pytest.mark.parametrize("group", pl.GROUPS)
def test_no_fault_model_survives(group):
    applicable, killed = _cells(group)
    assert applicable and not applicable - killed, sorted(applicable - killed)[:20]
    print(f"{group}: {len(applicable)} (fault, signature) cells, all killed")
    assert len(applicable) == FAULT_CELLS[group]


def test_fault_list_covers_the_required_families():
    names = {f.name for f in pl.all_faults()}
    for needle in ("last match wins", "only key limb 0 compared", "key limb 7 ignored", "top key bits above the width compared",
                   "argument 1 ignored", "arguments swapped", "a match in slot >= 8 missed", "a match in slot >= 16 missed",
                   "the slot after the match returned", "a matched lane returns the else value", "else value of model m+1",
                   "else value of model m-1", "value limb 3 dropped", "value limb 3 taken from the else value",
                   "result not masked to its width", "Bool result taken from bit 1", "innermost store wins",
                   "store chain stops after one level", "wide-key set limited to 32 entries", "last short chunk compared as a full chunk",
                   "chunk 8 skipped", "keccak pad byte misplaced by one at the 135 / 136-byte boundary", "second block dropped",
                   "digest byte order reversed per limb"):
        assert needle in names, needle
