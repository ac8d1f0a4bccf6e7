"""GPU parity on planted results (planted_ops.py): every value op at every width and operand form,
one operation a tape, its per-model result planted into the model batch - so that a wrong result
bit in any model flips a verdict - on the default path and on the HIP C++ path, with the kernel
that runs each (op, form, placement) cell asserted."""
import numpy as np
import pytest

import cref
import planted_ops as po
from mythril_amd.tape import Op

pytestmark = pytest.mark.gpu

CMP = (Op.EQ, Op.ULT, Op.ULE, Op.SLT, Op.SLE)


def expected_kernel(c: po.Case) -> str:
    """Which kernel runs a case on the default path, read from the translator (qsa_translate.cpp
    qsa_translate, mq_api.cpp qsa_prepare, tape_compiler.cpp) and confirmed on the MI355X:

    WIDE  a value wider than 256 bits: the wider generic HIP C++ kernels (L = 16 / 32 / 64);
    CPP   the 256-bit HIP C++ interpreter: the multiplication-overflow predicates (no assembly
          handler), and ASHR and the signed divisions below 256 bits (their handlers are 256-bit only);
    FLAT  a compare of a variable with a constant is a one-atom flat conjunction (fc.hip);
    P     variables below index 8 and handlers P has;
    G     everything else - also "lo" cases whose handler only G has: shifts by a variable amount,
          division by a variable, or by a constant that is 0 or has a magnitude of 2^32 or more."""
    if c.max_width > 256:
        return "WIDE"
    if c.op in po.OVERFLOW or (c.w != 256 and (c.op == Op.ASHR or c.op in po.SIGNED_DIVS)):
        return "CPP"
    if c.op in CMP and c.form in ("vk", "vK", "kv", "Kv"):
        return "FLAT"
    if c.place == "hi":
        return "G"
    if c.op in po.SHIFTS:
        return "P" if c.form[1] in "kK" else "G"
    if c.op in po.DIVS:
        if c.form[1] not in "kK":
            return "G"
        mag = abs(po.to_signed(c.fy, c.w)) if c.op in po.SIGNED_DIVS else c.fy
        return "P" if 0 < mag < 2 ** 32 else "G"
    return "P"


# handler kinds a group's cells must reach (a constant handler may run as its prefetched PF_ variant)
P_KINDS = {
    "addsub": [k + s for k in ("ADD", "SUB", "BAND", "BOR", "BXOR") for s in ("", "V", "C", "VV", "CV")] + ["NEG", "BNOT", "MASKP", "MASKZ"],
    "mul": ["MUL", "MULV", "MULC", "MULVV", "MULCV", "MASKP"],
    "udiv": ["UDIVC", "UREMC", "LSHRI", "MASKP"],
    "sdiv": ["SDIVCP", "SDIVCN", "SREMC", "SMODCP", "SMODCN"],
    "shift": ["SHLI", "SHLW", "LSHRI", "ASHRI", "MASKP"],
    "width": ["LSHRI", "MASKP", "MASKZ", "SHLI", "SHLW", "BOR", "SEXTA", "SEXTB", "ITE", "PUSH_VARB"],
    "cmp": ["EQ", "EQV", "EQC", "ULT", "ULTV", "ULTC", "ULE", "ULEV", "ULEC", "UGE", "UGT", "SLT", "SLE", "SGE", "SGT", "FLIP2"],
}
G_KINDS = {
    "addsub": ["ADD", "SUB", "BAND", "BOR", "BXOR", "NEG", "BNOT", "MASKP", "MASKZ", "PUSH_MEM", "PUSH_CONSTI", "PUSH_CONSTW"],
    "mul": ["MUL", "MASKP", "MASKZ"],
    "udiv": ["UDIVV", "UREMV", "UDIVC", "UREMC", "LSHRI", "MASKP"],
    "sdiv": ["SDIVV", "SREMV", "SMODV", "SDIVCP", "SDIVCN", "SREMC", "SMODCP", "SMODCN"],
    "shift": ["SHLV", "LSHRV", "ASHRV", "SHLI", "SHLW", "LSHRI", "ASHRI", "MASKP"],
    "width": ["LSHRI", "MASKP", "MASKZ", "SHLOR", "SHLW", "BOR", "SEXTA", "SEXTB", "ITE", "PUSH_PKB"],
    "cmp": ["EQ", "EQK", "ULT", "ULTK", "ULE", "ULEK", "UGE", "UGT", "SLT", "SLTK", "SLE", "SGE", "SGT", "FLIP2"],
}


def _check(evaluator, pack, idx, kernel, path, ref_cpu):
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
        if path == "default" and kernel in ("P", "G"):
            hist = ct.handler_histogram(0 if kernel == "P" else 1)
    finally:
        ct.free()
    where = f"{kernel} cells on the {path} path"
    assert (fh != -2).all() and (fh1 != -2).all(), f"{where}: unsupported: " + cases[int(np.flatnonzero((fh == -2) | (fh1 == -2))[0])].name()
    bad = np.argwhere(v != exp)
    if len(bad):
        t, m = (int(x) for x in bad[0])
        side = "the oracle agrees with the expectation" if ref_cpu[idx[t], m] == exp[t, m] else "the ORACLE disagrees with the expectation too"
        raise AssertionError(f"{where}: {len(bad)} wrong verdicts in {len(set(bad[:, 0]))} tapes; first: {cases[t].describe(m)}, "
                             f"got {bool(v[t, m])} ({side})")
    want_fh = np.where(exp.any(axis=1), exp.argmax(axis=1), -1)
    for got in (fh, fh1):
        t = np.flatnonzero(got != want_fh)
        assert len(t) == 0, f"{where}: first hit {got[t[0]]} != {want_fh[t[0]]}: {cases[int(t[0])].name()}"
    # the intended kernel ran: a cell expected on an assembly kernel that falls back fails here
    got = {"asm": (n_p, n_g, live), "flat": n_flat, "split": split}
    if path == "cpp":
        assert not live and n_flat == 0, (where, got)
    elif kernel == "P":
        assert (n_p, n_g, live, n_flat) == (n, 0, True, 0), (where, got, [c.name() for c in cases][:8])
    elif kernel == "G":
        assert (n_p, n_g, live, n_flat) == (0, n, True, 0), (where, got, [c.name() for c in cases][:8])
    elif kernel == "FLAT":
        assert n_flat == n, (where, got)
    elif kernel == "CPP":
        assert split == (0, n, 0), (where, got)
    else:
        assert split == (0, 0, n), (where, got)
    return hist


@pytest.mark.parametrize("group", list(po.GROUPS))
def test_planted_results(evaluator, group):
    """Default path and ``use_asm(False)`` (the HIP C++ interpreter at 256 bits, the wider generic
    kernels above): verdicts equal the by-construction expectation bit for bit, first hits are its
    argmax (-1 where none), no tape answers -2, and every cell runs on the kernel expected_kernel names."""
    cases = po.group_cases(group)
    hists = {"P": {}, "G": {}}
    seen = set()
    for pack in po.packs_of(cases, key=expected_kernel):
        evaluator.upload_models(pack.models)        # (one batch of all "hi" cases; 8 variables a "lo" batch)
        ref_cpu = cref.verdicts(pack.tapes, pack.models)
        by_kernel = {}
        for t, c in enumerate(pack.cases):
            by_kernel.setdefault(expected_kernel(c), []).append(t)
        for kernel, idx in by_kernel.items():
            seen.add(kernel)
            hist = _check(evaluator, pack, idx, kernel, "default", ref_cpu)
            for k, n in hist.items():
                hists[kernel][k] = hists[kernel].get(k, 0) + n
            evaluator.use_asm(False)
            try:
                _check(evaluator, pack, idx, kernel, "cpp", ref_cpu)
            finally:
                evaluator.use_asm(True)
    assert seen >= {"P", "G", "WIDE"} and (group not in ("mul", "sdiv", "shift") or "CPP" in seen) and (group != "cmp" or "FLAT" in seen)
    print(f"{group}: {len(cases)} tapes; P handlers {sorted(hists['P'])}; G handlers {sorted(hists['G'])}")
    for kernel, kinds in (("P", P_KINDS[group]), ("G", G_KINDS[group])):
        h = hists[kernel]
        missing = [k for k in kinds if h.get(k, 0) + h.get("PF_" + k, 0) == 0]
        assert not missing, (group, kernel, missing, sorted(h))
    if group in ("addsub", "mul"):
        assert sum(n for k, n in hists["P"].items() if k.startswith("PF_")) > 0, hists["P"]
