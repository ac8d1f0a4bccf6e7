"""The low-limb prefilter translation on a CPU (qsa_translate.cpp qsa_translate_pf, its peephole
over PUSH_VAR and the instruction that reads it): tests/host/pf_translate_check.cpp is compiled with
the host compiler alone, AddressSanitizer and UBSan on, and writes every translated narrow program
as (kind, slot, variable, immediate, third word).  A numpy uint32 model of those entries must agree
with the model of the compiled program itself (test_prefilter_compile.run_pf) on every model; the
handlers named are compared against the generated table (qsa_table.h), never against a recording."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pf_fused_cases as fc
from test_host_planners import _dump
from test_prefilter_compile import N_MODELS, run_pf
from mythril_amd import build as mq_build
from mythril_amd import evaluator as evmod
from mythril_amd.models import ModelBatch
from mythril_amd.synth import c2_tape, c2_workload, fuzz_workload, random_words
from mythril_amd.tape import Tape, TapeBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mythril_amd", "csrc")
W = 256
# gprog.h PfOp -> the handler kind of the unfused translation
(PF_END, PF_PUSH_VAR, PF_PUSH_K, PF_ADD, PF_SUB, PF_MUL, PF_NEG, PF_BAND, PF_BOR, PF_BXOR, PF_BNOT, PF_ADDK, PF_MULK,
 PF_ANDK, PF_ORK, PF_XORK, PF_EQ, PF_EQK) = range(18)
UNFUSED = {PF_END: "END", PF_PUSH_VAR: "PUSH_VAR", PF_PUSH_K: "PUSH_K32", PF_ADD: "ADD32", PF_SUB: "SUB32", PF_MUL: "MUL32",
           PF_NEG: "NEG32", PF_BAND: "BAND", PF_BOR: "BOR", PF_BXOR: "BXOR", PF_BNOT: "BNOT", PF_ADDK: "ADDK32",
           PF_MULK: "MULK32", PF_ANDK: "ANDK32", PF_ORK: "ORK32", PF_XORK: "XORK32", PF_EQ: "EQ32", PF_EQK: "EQK32"}
BIN = {"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "BAND": np.bitwise_and, "BOR": np.bitwise_or,
       "BXOR": np.bitwise_xor, "AND": np.bitwise_and, "OR": np.bitwise_or, "XOR": np.bitwise_xor}
FUSED = re.compile(r"(ADD|SUB|MUL|EQ)32VV?|(ADD|MUL|AND|OR|XOR|EQ)K32V")
DROPPED = ("MUL32VV", "ADDK32V", "EQ32V", "BANDV")


def run_entries(entries, mb):
    """The translated entries over uint32, all models at once: (pass mask, value compared)."""
    off = mb.var_word_offsets()
    V = lambda v: mb.var_words[off[v]]      # noqa: E731
    st, res, left = {}, None, None
    assert entries[-1][0] == "END"
    with np.errstate(over="ignore"):
        for kind, d, v, imm, w3 in entries[:-1]:
            assert res is None and w3 == 0, (kind, "an entry after the final compare, or a third word")
            k = np.uint32(imm)
            m = re.fullmatch(r"(ADD|SUB|MUL|BAND|BOR|BXOR)(32)?(VV|V)?", kind)
            mk = re.fullmatch(r"(ADD|MUL|AND|OR|XOR)K32(V)?", kind)
            if kind == "PUSH_VAR":
                st[d] = V(v).copy()
            elif kind == "PUSH_K32":
                st[d] = np.full(mb.n_models, k, np.uint32)
            elif kind == "NEG32":
                st[d] = np.uint32(0) - st[d]
            elif kind == "BNOT":
                st[d] = ~st[d]
            elif m and m.group(3) == "VV":
                assert imm % 8 == 0 and imm // 8 < 8
                st[d] = BIN[m.group(1)](V(v), V(imm // 8))
            elif m and m.group(3) == "V":
                st[d - 1] = BIN[m.group(1)](st[d - 1], V(v))
            elif m:
                st[d - 1] = BIN[m.group(1)](st[d - 1], st[d])
            elif mk:
                st[d] = BIN[mk.group(1)](V(v) if mk.group(2) else st[d], k)
            elif kind == "EQ32":
                left, res = st[d - 1], st[d - 1] == st[d]
            elif kind == "EQ32V":
                left, res = st[d - 1], st[d - 1] == V(v)
            elif kind == "EQK32":
                left, res = st[d], st[d] == k
            elif kind == "EQK32V":
                left, res = V(v), V(v) == k
            else:
                raise AssertionError(f"unknown narrow handler kind {kind}")
    assert res is not None
    return res, left


def _batches():
    """{name: (TapeBatch, ModelBatch)}"""
    rng = np.random.Generator(np.random.PCG64(5))
    mb = ModelBatch([W] * 8, random_words(rng, 64, N_MODELS))
    tapes = []
    for i in range(300):
        tapes.append(c2_tape(rng, [mb.var_value(v, int(rng.integers(N_MODELS))) for v in range(8)] if i % 2 else None))
    out = {"c2": (TapeBatch(tapes), mb)}
    for seed in (3, 4):
        out[f"fuzz{seed}"] = fuzz_workload(seed, 150, N_MODELS, asm_only=True)
        out[f"fuzz{seed + 10}"] = fuzz_workload(seed + 10, 150, N_MODELS, max_width=256, with_funcs=False)
    tb, mb, _, _ = fc.fused_batch(N_MODELS)
    out["hand"] = (tb, mb)
    tb, mb, _ = c2_workload(400, 8, seed=2, planted_frac=0.1)
    out["yield"] = (tb, mb)
    t = Tape()      # two constants that differ in limb 0: PUSH_K32, EQK32
    tape = t.finish(t.and_(t.ule(t.var(1, W), t.const((1 << W) - 1, W)),
                           t.eq(t.add(t.const(3, W), t.const(4, W)), t.bxor(t.const(9, W), t.const(1, W)))))
    out["konst"] = (TapeBatch([tape]), mb)
    return out


def _parse(text):
    """({(kind, d, v)} of the table, {batch: [{"prog": [...], "pf": [(kind, d, v, imm, w3)] or None}]})"""
    keys, batches, tape = set(), {}, None
    for line in text.splitlines():
        tag, *rest = line.split(" ")
        if tag == "key":
            keys.add((rest[0], int(rest[1]), int(rest[2])))
        elif tag == "batch":
            cur = batches.setdefault(rest[0], [])
        elif tag == "tape":
            tape = {"prog": [], "pf": None}
            cur.append(tape)
        elif tag == "prog":
            tape["prog"] = [int(x, 16) for x in rest]
        elif tag == "pf":
            tape["pf"] = [] if int(rest[0]) else None
        elif tag == "e":
            tape["pf"].append((rest[0], int(rest[1]), int(rest[2]), int(rest[3]), int(rest[4])))
        else:
            raise AssertionError(f"unexpected line {line!r}")
    return keys, batches


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{"batches": ..., arm: (exit status, stderr, table keys, parsed batches)}; arms: "fused",
    "unfused" (MQ_PF_FUSE=0) and one per kind of DROPPED taken out of the table."""
    if not mq_build._generated_current():      # qsa_table.h is generated, not tracked
        subprocess.check_call([sys.executable, os.path.join(CSRC, "gen_qsa.py")])
    d = tmp_path_factory.mktemp("pf_translate_check")
    exe, corpus = str(d / "pf_translate_check"), str(d / "corpus.txt")
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "the host compiler is needed"
    cmd = [cxx, "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", os.path.join(ROOT, "tests", "host", "pf_translate_check.cpp")] + \
          [os.path.join(CSRC, s) for s in ("tape_compiler.cpp", "qsa_translate.cpp")] + ["-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    batches = _batches()
    _dump(corpus, [(name, tb, list(mb.var_widths), list(mb.funcs)) for name, (tb, mb) in batches.items()])
    out = {"batches": batches}
    env = {k: v for k, v in os.environ.items() if not k.startswith("MQ_")}
    for arm, extra, args in [("fused", {}, []), ("unfused", {"MQ_PF_FUSE": "0"}, [])] + [(k, {}, [k]) for k in DROPPED]:
        res = subprocess.run([exe, corpus] + args, capture_output=True, text=True, env={**env, **extra})
        out[arm] = (res.returncode, res.stderr) + _parse(res.stdout)
    return out


def _decode(prog):
    return [(int(w) & 0xFF, (int(w) >> 8) & 0xF, int(i)) for w, i in zip(prog[0::2], prog[1::2])]


def _check_semantics(run, batches):
    n = 0
    for name, (tb, mb) in batches.items():
        tapes = run[name]
        assert len(tapes) == tb.n_tapes
        for t, tape in enumerate(tapes):
            assert (tape["pf"] is None) == (len(tape["prog"]) == 0), (name, t)
            if tape["pf"] is None:
                continue
            assert tape["prog"] == [int(w) for w in evmod.tape_prefilter_program(tb, t)[0]], (name, t)
            want, want_left = run_pf(np.asarray(tape["prog"], np.uint32), mb)
            got, got_left = run_entries(tape["pf"], mb)
            assert (got == want).all() and (got_left == want_left).all(), (name, t, tape["pf"])
            n += 1
    return n


def test_fused_entries_compute_what_the_program_computes(runs):
    """Every model of every batch: pass mask and compared value of the entries equal run_pf's."""
    rc, err, _, run = runs["fused"]
    assert rc == 0, err[-4000:]
    n = _check_semantics(run, runs["batches"])
    print(f"{n} narrow programs")
    assert n >= 300 + 400 + len(runs["batches"]["hand"][0].offsets) - 1


def test_unfused_is_one_entry_per_instruction(runs):
    """MQ_PF_FUSE=0: the translation before the peephole, word for word -- one entry per
    instruction, the kind by UNFUSED, the variable as the handler's key, the immediate as it is."""
    rc, err, _, run = runs["unfused"]
    assert rc == 0, err[-4000:]
    n = 0
    for name, tapes in run.items():
        for t, tape in enumerate(tapes):
            if tape["pf"] is None:
                continue
            want = []
            for op, d, imm in _decode(tape["prog"]):
                if op == PF_PUSH_VAR:
                    want.append(("PUSH_VAR", d, imm, 0, 0))
                elif op == PF_END:
                    want.append(("END", -1, -1, 0, 0))
                else:
                    want.append((UNFUSED[op], d, -1, imm, 0))
            assert tape["pf"] == want, (name, t)
            n += 1
    assert n > 700
    _check_semantics(run, {"hand": runs["batches"]["hand"]})


def test_every_generated_fused_handler_is_named(runs):
    """The union of the programs names every fused narrow handler of qsa_table.h by (kind, slot,
    variable), and every unfused narrow kind; the hand-built batch alone does."""
    _, _, keys, run = runs["fused"]
    narrow = {k for k in keys if "32" in k[0]}
    fused = {k for k in narrow if FUSED.fullmatch(k[0])}
    assert len(fused) >= 8 * (3 * 4 + 1 + 5 * 5 + 1 + 3 * 4) and {k[0] for k in narrow - fused} == set(UNFUSED.values()) - {
        "END", "PUSH_VAR", "BAND", "BOR", "BXOR", "BNOT"}
    seen = {e[:3] for tape in run["hand"] if tape["pf"] for e in tape["pf"]}
    assert not (fused - seen), sorted(fused - seen)[:20]
    # P's own limb-wise handlers serve the fused bitwise forms at the same slots
    for d in range(1, fc.MAX_SLOT + 1):
        for v in range(8):
            assert {("BANDV", d, v), ("BORV", d, v), ("BXORV", d, v)} <= seen and \
                {("BANDVV", d - 1, v), ("BORVV", d - 1, v), ("BXORVV", d - 1, v)} <= seen, (d, v)
    everything = {e[0] for tapes in run.values() for tape in tapes if tape["pf"] for e in tape["pf"]}
    assert {k[0] for k in narrow} <= everything, sorted({k[0] for k in narrow} - everything)
    # every v2 behind every v1, v1 == v2 among them, and the four edge constants
    vv = {(e[0], e[2], e[3] // 8) for tape in run["hand"] if tape["pf"] for e in tape["pf"] if e[0].endswith("VV")}
    for kind in ("ADD32VV", "SUB32VV", "MUL32VV", "BANDVV", "BORVV", "BXORVV"):
        assert {(kind, a, b) for a in range(8) for b in range(8)} <= vv, kind
    for kind in ("ADDK32V", "MULK32V", "ANDK32V", "ORK32V", "XORK32V"):
        ks = {e[3] for tape in run["hand"] if tape["pf"] for e in tape["pf"] if e[0] == kind}
        # (a product or an AND with a constant whose low limb is 0 is no narrow instruction: it folds)
        assert set(fc.LOW_CONSTS) - ({0} if kind in ("MULK32V", "ANDK32V") else set()) <= ks, (kind, sorted(ks)[:8])


def test_hand_built_batch_is_what_the_gpu_test_expects(runs):
    """test_gpu_prefilter_fused reads these from the launch's histogram and entry counts."""
    _, _, keys, run = runs["fused"]
    assert {k[0] for k in keys if FUSED.fullmatch(k[0])} == fc.FUSED
    hist = {e[0] for tape in run["hand"] for e in tape["pf"]}
    uhist = {e[0] for tape in runs["unfused"][3]["hand"] for e in tape["pf"]}
    assert fc.FUSED | fc.UNFUSED | fc.SHARED <= hist, sorted((fc.FUSED | fc.UNFUSED | fc.SHARED) - hist)
    assert not (fc.FUSED & uhist) and fc.UNFUSED | {"PUSH_VAR", "BNOT", "BAND", "BOR", "BXOR"} <= uhist
    entries = sum(len(tape["pf"]) - 1 for tape in run["hand"])
    instrs = sum(len(tape["prog"]) // 2 - 1 for tape in run["hand"])
    assert entries < 0.7 * instrs
    m0 = {e[0] for tape, name in zip(run["hand"], fc.fused_batch(N_MODELS)[3]) if name.startswith("m0 ") for e in tape["pf"]}
    assert {"ADD32VV", "SUB32VV", "MUL32VV", "NEG32", "BNOT", "ADDK32", "MULK32", "ADD32V", "BANDV", "ADD32", "BAND",
            "MULK32V", "PUSH_VAR", "SUB32", "EQ32", "EQK32"} <= m0


def test_m0_indexed_handlers_next_to_every_class(runs):
    """A kindVV handler (index mode through M0) directly before and directly after a handler of
    every class that can stand there: P's own (NEXT_P), unfused narrow, fused by variable, fused
    with a constant, and the final compares.  (The deeper operand comes first, so a lone variable
    or a variable with a constant is never pushed right before the two-variable form.)"""
    _, _, _, run = runs["fused"]
    before, after = set(), set()
    for tape in run["hand"]:
        ks = [e[0] for e in tape["pf"] or []]
        for a, b in zip(ks, ks[1:]):
            if a.endswith("VV"):
                after.add(b)
            if b.endswith("VV"):
                before.add(a)
    print(sorted(before), sorted(after))
    assert {"NEG32", "BNOT", "ADDK32", "MULK32", "ADD32V", "BANDV", "SUB32"} <= before
    assert {"NEG32", "BNOT", "ADDK32", "MULK32", "ADD32V", "BANDV", "SUB32", "ADD32", "BAND", "MULK32V", "PUSH_VAR", "EQ32",
            "EQK32"} <= after
    assert any(k.endswith("VV") for k in before & after)       # two in a row


def test_yield_on_c2(runs):
    """c2_workload(400, 8, seed=2, planted_frac=0.1): entries per program (END left out) at most
    0.65 of the compiled instructions (the adjacent-pattern peephole reaches 0.603: 16.17 -> 9.75)."""
    tapes = runs["fused"][3]["yield"]
    assert len(tapes) == 400 and all(t["pf"] for t in tapes)
    entries = np.mean([len(t["pf"]) - 1 for t in tapes])
    instrs = np.mean([len(t["prog"]) // 2 - 1 for t in tapes])
    print(f"entries {entries:.3f} of {instrs:.3f} instructions: {entries / instrs:.4f}")
    assert entries <= 0.65 * instrs


@pytest.mark.parametrize("kind", DROPPED)
def test_missing_handler_falls_back_unfused(runs, kind):
    """A table without one fused kind still translates every program: the kind does not occur,
    the spot is the unfused entries, the values are the program's."""
    rc, err, keys, run = runs[kind]
    assert rc == 0, err[-4000:]
    full = runs["fused"][3]
    assert any(e[0] == kind for tape in full["hand"] if tape["pf"] for e in tape["pf"])
    more = 0
    for name, tapes in run.items():
        for t, tape in enumerate(tapes):
            assert (tape["pf"] is None) == (full[name][t]["pf"] is None), (name, t)
            if tape["pf"]:
                assert all(e[0] != kind for e in tape["pf"]), (name, t)
                assert len(tape["pf"]) >= len(full[name][t]["pf"])
                more += len(tape["pf"]) - len(full[name][t]["pf"])
    assert more > 0
    _check_semantics(run, {"hand": runs["batches"]["hand"], "c2": runs["batches"]["c2"]})
