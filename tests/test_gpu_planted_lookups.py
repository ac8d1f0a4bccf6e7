"""GPU parity on planted results (planted_lookups.py): table lookups of one and two arguments, SELECT
over array terms and store chains, wide-key lookups, in-tape keccak, the keccak column kernel and
the Bool connectives - one operation a tape, its per-model result planted into the model batch, so
that a wrong result bit, a wrong entry or a neighbour's else value in any model flips a verdict - on
the default path and on the HIP C++ path, the lookups under both table layouts, with the kernel
that runs each cell and the layout of each function asserted."""
import numpy as np
import pytest

import cref
import planted_lookups as pl

pytestmark = pytest.mark.gpu

FLAT_BOOL = {("NOT", "v"), ("AND", "vT"), ("AND", "vv"), ("OR", "vv")}


def expected_kernel(c: pl.LCase) -> str:
    """Which kernel runs a case on the default path, read from the translator (qsa_translate.cpp
    qsa_translate, mq_api.cpp qsa_prepare, tape_compiler.cpp) and confirmed on the MI355X:

    WIDE  a key or result wider than 256 bits, and every in-tape KECCAK: the wider generic HIP C++
          kernels (L = 16 / 32 / 64);
    CPP   the 256-bit HIP C++ interpreter: lookups of two arguments and wide-key lookups
          (UF_CHUNK / UF_WIDE) - neither has an assembly handler;
    FLAT  NOT / AND / OR of Bool variables are flat conjunctions (fc.hip); so is SELECT of a
          CONST_ARRAY of a Bool variable, which the tape compiler folds to that variable;
    G     every lookup of one argument with key and result of at most 256 bits (UF1 / UF1B), also on
          variables below index 8: P has no lookup handler; store chains, which the tape compiler
          rewrites into ITE(EQ(idx, key), val, rest) over the base's UF1; Bool connectives of
          variables from index 8 up;
    P     Bool connectives of variables below index 8 (and of constants alone)."""
    if c.group == "keccak":
        return "WIDE"
    if c.group in ("uf2", "widekey"):
        return "CPP"
    if c.group == "uf1":
        spec = c.tables[0].spec
        return "WIDE" if max(spec.arg_widths[0], spec.result_width) > 256 else "G"
    if c.group == "array":
        return "FLAT" if c.sig == "256->0 const depth 0" else "G"
    if (c.sig, c.form) in FLAT_BOOL:
        return "FLAT"
    return "P" if c.place == "lo" or not set(c.form) & set("vc") else "G"


# handler kinds a group's cells must reach on the assembly kernels
KINDS = {
    ("uf1", "G"): ["UF1", "UF1B", "EQ", "MASKP", "NOT", "BXOR", "ADD"],
    ("array", "G"): ["UF1", "UF1B", "ITE", "ITE_EF", "BITE", "BITE_EF", "EQ", "EQK", "NOT"],
    ("bool", "G"): ["NOT", "OR", "XOR", "IMPLIES", "IFF", "BITE", "ULT", "PUSH_PKB_A"],
    ("bool", "P"): ["NOT", "OR", "XOR", "IMPLIES", "IFF", "BITE", "ULTV", "PUSH_VARB_A"],
}
KERNELS = {"uf1": {"G", "WIDE"}, "uf2": {"CPP"}, "array": {"G", "FLAT"}, "widekey": {"CPP"}, "keccak": {"WIDE"}, "bool": {"P", "G", "FLAT"}}


def _check(evaluator, pack, idx, kernel, path):
    """Verdicts, first hits and the kernel of tapes ``idx`` of ``pack`` (its models are resident)."""
    tb = pack.tapes.subset(idx)
    cases = [pack.cases[i] for i in idx]
    exp = np.array([c.expect for c in cases])
    ct = evaluator.compile(tb)
    try:
        v, fh = evaluator.verdicts(ct)
        fh1 = evaluator.first_hit(ct)
        n = len(idx)
        split, (n_p, n_g, live), n_flat = ct.split(), ct.asm_split(), ct.flat_split()[0]
        hist = {}
        if path.startswith("default") and kernel in ("P", "G"):
            hist = ct.handler_histogram(0 if kernel == "P" else 1)
    finally:
        ct.free()
    where = f"{kernel} cells on the {path} path"
    assert (fh != -2).all() and (fh1 != -2).all(), f"{where}: unsupported: " + cases[int(np.flatnonzero((fh == -2) | (fh1 == -2))[0])].name()
    bad = np.argwhere(v != exp)
    if len(bad):
        t, m = (int(x) for x in bad[0])
        ref_cpu = cref.verdicts(tb, pack.models)
        side = "the oracle agrees with the expectation" if ref_cpu[t, m] == exp[t, m] else "the ORACLE disagrees with the expectation too"
        raise AssertionError(f"{where}: {len(bad)} wrong verdicts in {len(set(bad[:, 0]))} tapes; first: {cases[t].describe(m)}, "
                             f"got {bool(v[t, m])} ({side})")
    want_fh = np.where(exp.any(axis=1), exp.argmax(axis=1), -1)
    for got in (fh, fh1):
        t = np.flatnonzero(got != want_fh)
        assert len(t) == 0, f"{where}: first hit {got[t[0]]} != {want_fh[t[0]]}: {cases[int(t[0])].name()}"
    # the intended kernel ran: a cell expected on an assembly kernel that falls back fails here
    got = {"asm": (n_p, n_g, live), "flat": n_flat, "split": split}
    if path.startswith("cpp"):
        assert not live and n_flat == 0, (where, got)
    elif kernel == "P":
        assert (n_p, n_g, live, n_flat) == (n, 0, True, 0), (where, got, [c.name() for c in cases][:8])
    elif kernel == "G":
        assert (n_p, n_g, live, n_flat) == (0, n, True, 0), (where, got, [c.name() for c in cases][:8])
    elif kernel == "FLAT":
        assert n_flat == n, (where, got)
    elif kernel == "CPP":
        assert split == (0, n, 0) and n_flat == 0, (where, got)
    else:
        assert split == (0, 0, n) and n_flat == 0, (where, got)
    return hist


def _keccak_columns(evaluator, monkeypatch):
    """``Keccak256(Concat(...)) == R`` with R planted, three roots a message so that it hoists: the
    keccak column kernel computes the digests, the tapes compare them (default path, use_asm(False),
    and MQ_NO_KECCAK_COLUMNS=1, where the interpreters hash)."""
    from mythril_amd.lower import SymbolTable, lower_batch, serialize_models
    w = pl.keccak_column_workload()
    tb, syms, ok = lower_batch(w.roots, SymbolTable(interpret_keccak=True), hoist=True)
    assert ok.all() and tb.columns is not None
    evaluator.upload_models(serialize_models(w.models, syms))
    want_fh = np.where(w.expect.any(axis=1), w.expect.argmax(axis=1), -1)
    for columns in (True, False):
        if not columns:
            monkeypatch.setenv("MQ_NO_KECCAK_COLUMNS", "1")
        for asm in (True, False):
            evaluator.use_asm(asm)
            try:
                ct = evaluator.compile(tb)
                try:
                    assert ct.keccak_columns() == (w.n_messages if columns else 0)
                    v, fh = evaluator.verdicts(ct)
                    fh1 = evaluator.first_hit(ct)
                finally:
                    ct.free()
            finally:
                evaluator.use_asm(True)
            where = f"keccak columns {'on' if columns else 'off'}, {'default' if asm else 'cpp'} path"
            bad = np.argwhere(v != w.expect)
            if len(bad):
                t, m = (int(x) for x in bad[0])
                tb0, syms0, _ = lower_batch(w.roots, SymbolTable(interpret_keccak=True))
                ref_cpu = cref.verdicts(tb0, serialize_models(w.models, syms0))
                side = "the oracle agrees with the expectation" if ref_cpu[t, m] == w.expect[t, m] else "the ORACLE disagrees too"
                raise AssertionError(f"{where}: {len(bad)} wrong verdicts; first: root {t} {w.cases[t].describe(m)}, got {bool(v[t, m])} ({side})")
            assert (fh == want_fh).all() and (fh1 == want_fh).all() and (fh != -2).all(), (where, fh, want_fh)
    print(f"keccak_columns: {len(w.roots)} roots over {w.n_messages} messages, {pl.M_KECCAK} models")


@pytest.mark.parametrize("group", pl.GROUPS)
def test_planted_results(evaluator, monkeypatch, group):
    """Default path and ``use_asm(False)``, the lookup groups under MQ_NO_DENSE_TABLES=1 as well:
    verdicts equal the by-construction expectation bit for bit, first hits are its argmax (-1 where
    none), no tape answers -2, every cell runs on the kernel expected_kernel names, and every function
    has the table layout it was built for (dense slots / CSR entry lists)."""
    if group == "keccak_columns":
        return _keccak_columns(evaluator, monkeypatch)
    hists = {"P": {}, "G": {}}
    seen = set()
    packs = pl.group_packs(group)
    for layout in (("dense", "csr") if group in pl.LOOKUP_GROUPS else ("",)):
        if layout == "csr":
            monkeypatch.setenv("MQ_NO_DENSE_TABLES", "1")       # (read at the upload)
        else:
            monkeypatch.delenv("MQ_NO_DENSE_TABLES", raising=False)
        for pack in packs:
            evaluator.upload_models(pack.models)
            if pack.tables:
                info = evaluator.download_funcs().info
                for f, tab in enumerate(pack.tables):
                    want = pl.dense_expected(tab) if layout == "dense" else 0
                    assert bool(want) == (tab.dense and layout == "dense") and int(info[f][1]) == want, (tab.name, layout, info[f].tolist())
            by_kernel = {}
            for t, c in enumerate(pack.cases):
                by_kernel.setdefault(expected_kernel(c), []).append(t)
            for kernel, idx in by_kernel.items():
                seen.add(kernel)
                hist = _check(evaluator, pack, idx, kernel, f"default {layout}".strip())
                for k, n in hist.items():
                    hists[kernel][k] = hists[kernel].get(k, 0) + n
                evaluator.use_asm(False)
                try:
                    _check(evaluator, pack, idx, kernel, f"cpp {layout}".strip())
                finally:
                    evaluator.use_asm(True)
    assert seen == KERNELS[group], (group, seen)
    n = {k: sum(expected_kernel(c) == k for c in pl.group_cases(group)) for k in sorted(seen)}
    print(f"{group}: {len(pl.group_cases(group))} tapes {n}; P handlers {sorted(hists['P'])}; G handlers {sorted(hists['G'])}")
    for kernel in ("P", "G"):
        h = hists[kernel]
        missing = [k for k in KINDS.get((group, kernel), []) if h.get(k, 0) == 0]
        assert not missing, (group, kernel, missing, sorted(h))
