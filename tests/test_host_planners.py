"""The host planners on a CPU (csrc/qsa_translate.cpp, csrc/fc_plan.cpp): tests/host/planner_check.cpp
is compiled with the host compiler alone -- no ROCm include path, AddressSanitizer and UBSan on --
and run on a corpus dumped from the Python tape builders.  The program checks the structure of
every translation itself (its exit status); the text it writes is checked here against the rules
the translator documents and the generated form tables (qsa_table.h), never against a recording."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import planted_ops as po
import test_g_bail_compile as gb
import test_gpu_parity as gp
from mythril_amd import build as mq_build
from mythril_amd.synth import c2_tape
from mythril_amd.synth_evm import c3_workload
from mythril_amd.tape import Tape, TapeBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mythril_amd", "csrc")
G_BAIL = 35
G_FINAL = {"not": 10, "and": 11, "or": 12}           # gprog.h G_NOT, G_AND, G_OR
G_COMPARE = {20: "EQ", 21: "ULT", 22: "ULE", 23: "UGT", 24: "UGE", 25: "SLT", 26: "SLE", 27: "SGT", 28: "SGE"}


def _fusion_tapes():
    """Bool results consumed right where they are made; both operands of every compare are
    computed values, so no leaf fusion renames the compare."""
    def cmp(t, k, kind):
        a = t.mul(t.var(k % 8, 256), t.var((k + 1) % 8, 256))
        b = t.add(t.var((k + 2) % 8, 256), t.var((k + 3) % 8, 256))
        return getattr(t, kind)(a, b)

    out = {}
    for kind in ("ult", "slt"):      # (an ordering compare has a complement; EQ has none)
        t = Tape()
        out[f"not_{kind}"] = t.finish(t.not_(cmp(t, 0, kind)))
    for kind in ("eq", "ult"):
        t = Tape()
        out[f"and_{kind}"] = t.finish(t.and_(cmp(t, 0, "ult"), cmp(t, 4, kind)))
        t = Tape()
        out[f"or_{kind}"] = t.finish(t.or_(cmp(t, 0, "ult"), cmp(t, 4, kind)))
    return out


FUSION = _fusion_tapes()


def _planted_packs():
    """One case per op, form and place of planted_ops at the largest width whose values fit 256 bits."""
    cases = []
    for ops in po.GROUPS.values():
        for op in ops:
            seen = set()
            for w in sorted((w for w in po.op_widths(op) if w <= 256), reverse=True):
                for form, imm, fx, fy in po._case_params(op, w):
                    if form in seen or po.result_width(op, w, imm) > 256:
                        continue
                    base = po.make_case(op, w, form, "hi", imm, fx, fy)
                    if base.max_width > 256:
                        continue
                    seen.add(form)
                    cases.append(base)
                    if base.max_width == 256 or (w in po.LO_WIDTHS and base.max_width < 256):
                        cases.append(po.replace(base, place="lo"))
    return po.packs_of(cases)


def _corpus():
    """[(name, TapeBatch, variable widths, function signatures)]"""
    rng = np.random.Generator(np.random.PCG64(5))
    out = [("c2", TapeBatch([c2_tape(rng, None) for _ in range(6)]), [256] * 8, [])]
    tb, mb = c3_workload(40, 128, seed=3)[:2]
    out.append(("c3", tb, list(mb.var_widths), list(mb.funcs)))
    out.append(("conj", TapeBatch([gb.TAPES[s]() for s in gb.TAPES]), [256] * 9, []))
    out.append(("fusion", TapeBatch(list(FUSION.values())), [256] * 8, []))
    out.append(("leafpair", gp._leaf_pair_tapes(np.random.default_rng(100), 300), [256] * 8, []))
    tb, mb = gp._bool_heavy_workload(120, 1000, seed=1000)
    out.append(("boolheavy", tb, list(mb.var_widths), []))
    for i, p in enumerate(_planted_packs()):
        out.append((f"planted{i}", p.tapes, list(p.models.var_widths), list(p.models.funcs)))
    return out


def _dump(path, corpus):
    with open(path, "w") as f:
        for name, tb, widths, funcs in corpus:
            consts = np.asarray(tb.consts, np.uint32)
            f.write(f"batch {name} {len(widths)} {len(funcs)} 0 {tb.n_tapes} {len(tb.nodes)} {len(consts)}\n")
            f.write(" ".join(str(int(w)) for w in widths) + "\n")
            for fn in funcs:
                aw = list(fn.arg_widths) + [0, 0]
                f.write(f"{fn.arity} {fn.result_width} {aw[0]} {aw[1]}\n")
            f.write(" ".join(str(int(o)) for o in tb.offsets) + "\n")
            for n in tb.nodes:
                f.write(f"{int(n['op'])} {int(n['width'])} {int(n['a'])} {int(n['b'])} {int(n['c'])}\n")
            f.write(" ".join(str(int(c)) for c in consts) + "\n")


def _parse(text):
    """{"kinds": [...], "andform": [...], ..., "batches": {name: {"tapes": [dict], "fca": dict}}}"""
    out = {"batches": {}}
    batch = tape = None
    for line in text.splitlines():
        tag, *rest = line.split(" ")
        if tag == "kinds":
            out["kinds"] = rest
        elif tag in ("andform", "orform", "notform", "lform"):
            out[tag] = [int(x) for x in rest]
        elif tag == "batch":
            batch = out["batches"].setdefault(rest[0], {"tapes": []})
        elif tag == "tape":
            tape = dict(zip(rest[1::2], (int(x) for x in rest[2::2])))
            batch["tapes"].append(tape)
        elif tag in ("prog", "prog_g") or tag.endswith("x"):
            tape[tag] = [int(x, 16) for x in rest]
        elif tag in ("P", "Gs", "G0", "G1", "G1s", "PF"):
            tape[tag] = rest[1:] if rest[0] == "1" else None
        elif tag == "fc":
            tape["fc"] = {"fc": int(rest[0]), **dict(zip(rest[1::2], (int(x) for x in rest[2::2])))}
        elif tag == "fca":
            batch["fca"] = dict(zip(rest[0::2], (int(x) for x in rest[1::2])))
        else:
            raise AssertionError(f"unexpected line {line!r}")
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The program's parsed output with MQ_G_BAIL unset (False) and set (True)."""
    if not mq_build._generated_current():      # qsa_table.h is generated, not tracked
        subprocess.check_call([sys.executable, os.path.join(CSRC, "gen_qsa.py")])
    d = tmp_path_factory.mktemp("planner_check")
    exe, corpus = str(d / "planner_check"), str(d / "corpus.txt")
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "the host compiler is needed"
    # (no ROCm include path: that the planners need none is part of the check.  The sanitizer
    # runtimes are linked into the program: the test hands its caller's environment on untouched,
    # and ASan's shared runtime refuses to start unless it is the first library loaded)
    cmd = [cxx, "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan",
           os.path.join(ROOT, "tests", "host", "planner_check.cpp")] + \
          [os.path.join(CSRC, s) for s in ("tape_compiler.cpp", "qsa_translate.cpp", "fc_plan.cpp")] + ["-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    _dump(corpus, _corpus())
    out = {}
    for g_bail in (False, True):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MQ_")}
        if g_bail:
            env["MQ_G_BAIL"] = "1"
        res = subprocess.run([exe, corpus], capture_output=True, text=True, env=env)
        out[g_bail] = (res.returncode, res.stderr, _parse(res.stdout))
    return out


def _tapes(run):
    for name, b in run["batches"].items():
        for i, t in enumerate(b["tapes"]):
            yield name, i, t


@pytest.mark.parametrize("g_bail", [False, True])
def test_every_translation_is_well_formed(runs, g_bail):
    """The program's own checks: every translation walks handler by handler onto END / END_V at
    its last word, also after the window layout (no handler group across a 64-word block), and a
    second translation repeats the words and the derived constants; no sanitizer report."""
    rc, err, run = runs[g_bail]
    assert rc == 0, err[-4000:]
    n = {k: sum(1 for _, _, t in _tapes(run) if t.get(k)) for k in ("P", "Gs", "G0", "G1", "G1s", "PF")}
    print(n)
    assert all(v > 0 for v in n.values()), n
    # the structural translation promises what the translation for a layout then gives
    for name, i, t in _tapes(run):
        if t.get("G0") is not None:
            assert t["Gs"] is not None, (name, i)


def test_bail_points_on_g(runs):
    """A G_BAIL of a verdict tape becomes a BAIL word only with g_bail, and only where no PUSH_MEM
    load can be outstanding: behind it every PUSH_MEM was followed by a stack reader (a kind with
    an _L form, in either form) or by a handler that waits for vector memory itself.  With g_bail,
    `extra` ends with the second words of all the program's bail points, kept and dropped."""
    kept = dropped = 0
    for g_bail in (False, True):
        run = runs[g_bail][2]
        kinds, lform = run["kinds"], run["lform"]
        drains = {k for i, k in enumerate(kinds) if lform[i] >= 0} | {kinds[f] for f in lform if f >= 0} | \
                 {k for k in kinds if k == "PUSH_MEMB" or k.startswith("MEQK") or k.startswith("UF1")}
        for name, i, t in _tapes(run):
            if "prog" not in t:
                continue
            seconds = [imm2 for op, _, _, imm2 in gb.decode(t["prog_g"] or t["prog"]) if op == G_BAIL]
            for k in ("Gs", "G0"):
                assert t[k] is None or "BAIL" not in t[k], (name, i, k)
            if t["P"] is not None:
                assert t["P"].count("BAIL") == sum(1 for op, _, _, _ in gb.decode(t["prog"]) if op == G_BAIL), (name, i)
            for k in ("G1", "G1s"):
                if t[k] is None:
                    continue
                assert t[k + "x"][len(t[k + "x"]) - len(seconds):] == seconds, (name, i, k)
                if k == "G1":
                    assert t["G1x"][:len(t["G0x"])] == t["G0x"] and len(t["G1x"]) == len(t["G0x"]) + len(seconds), (name, i)
                assert t[k].count("BAIL") <= len(seconds), (name, i, k)
                pending = False
                for q in t[k]:
                    if q == "PUSH_MEM":
                        pending = True
                    elif q == "BAIL":
                        assert not pending, (name, i, k, t[k])
                    elif q in drains:
                        pending = False
                if k == "G1":
                    kept += t[k].count("BAIL")
                    dropped += len(seconds) - t[k].count("BAIL")
    print(f"G bail points kept {kept}, dropped {dropped}")
    # MQ_G_BAIL=1: at every spine point of the nine-variable conjunctions the pushes have been
    # consumed by the compare that made B(0), so all three bail points stay
    for t in runs[True][2]["batches"]["conj"]["tapes"]:
        assert t["G1"].count("BAIL") == 3, t["G1"]
    for t in runs[False][2]["batches"]["conj"]["tapes"]:
        assert "BAIL" not in t["G1"] and t["G1x"] == t["G0x"]     # (compiled without: nothing to keep)
    # the hand-built program (planner_check.cpp bail_behind_push): bail points right behind the
    # pushes of variables 8 and 9, 10, and one behind the compare that read variable 8.  Read from
    # memory, the first and the third find a load nothing waited for and go; all three second
    # words stay in `extra`.  Without g_bail none is a word and `extra` is empty.
    for g_bail in (False, True):
        (t,) = runs[g_bail][2]["batches"]["handbuilt"]["tapes"]
        assert [imm2 for op, _, _, imm2 in gb.decode(t["prog"]) if op == G_BAIL] == [300, 200, 100]
        assert t["G0"] == ["PUSH_MEM", "EQK", "PUSH_MEM", "PUSH_MEM", "EQ_A", "END"] and t["G0x"] == []
        assert t["G1"] == ["PUSH_MEM", "EQK", "BAIL", "PUSH_MEM", "PUSH_MEM", "EQ_A", "END"], t["G1"]
        assert t["G1x"] == [300, 200, 100]
    assert kept > 0 and dropped == 4        # (the two dropped ones, in both runs)


def test_p_never_prefetches_twice_in_a_row(runs):
    """P's constant prefetch: a PF_ handler's predecessor is never one itself."""
    n_pf = 0
    for name, i, t in _tapes(runs[False][2]):
        for k in ("P", "PF"):
            ks = t.get(k) or []
            n_pf += sum(q.startswith("PF_") for q in ks)
            assert not any(a.startswith("PF_") and b.startswith("PF_") for a, b in zip(ks, ks[1:])), (name, i, ks)
    assert n_pf > 0


def test_bool_fusions_leave_one_word(runs):
    """NOT of a compare is the complementary compare, AND / OR of a Bool the previous word just
    made is that word's accumulating form (qsa_table.h kQsaKindNot / AndForm / OrForm): no
    separate NOT, AND or OR word; G may then run the word's _L form."""
    run = runs[False][2]
    kinds = run["kinds"]
    form = {"not": run["notform"], "and": run["andform"], "or": run["orform"]}
    tapes = run["batches"]["fusion"]["tapes"]
    for (name, _), t in zip(FUSION.items(), tapes):
        how = name.split("_")[0]
        for k in ("P", "G0", "G1"):
            # the compare the stack program ends on (the compiler orders a conjunction's compares)
            prog = gb.decode(t["prog"] if k == "P" or not t["prog_g"] else t["prog_g"])
            assert [op for op, _, _, _ in prog[-2:]] == [G_FINAL[how], 0], (name, prog)
            fused = form[how][kinds.index(G_COMPARE[prog[-3][0]])]
            assert fused >= 0, (name, "the generator has a fused form")
            want = {kinds[fused]}
            ks = t[k]
            assert ks is not None, (name, k)
            assert how.upper() not in ks, (name, k, ks)
            ok = want | ({kinds[run["lform"][fused]]} if k != "P" and run["lform"][fused] >= 0 else set())
            assert ks[-1] in ("END", "END_V") and ks[-2] in ok, (name, k, ks, ok)


def test_p_candidate(runs):
    """P preloads variables 0-7: a tape reading variable 8 is no candidate; one over 0-7 is."""
    run = runs[False][2]
    assert [t["p_candidate"] for t in run["batches"]["conj"]["tapes"]] == [0, 0, 0]
    assert all(t["p_candidate"] == 1 and t["P"] is not None for t in run["batches"]["c2"]["tapes"])
    assert all(t["p_candidate"] == 1 for t in run["batches"]["fusion"]["tapes"])


def test_leaf_pair_and_bool_mask_handlers(runs):
    """What test_p_leaf_pair_fusions_match_oracle and
    test_g_kernel_bool_masks_and_fused_handlers_match_oracle read from the GPU histograms: every
    leaf-pair tape is P's and the twelve both-leaf kinds occur (plain or prefetched); the
    Bool-heavy tapes left to G read packed masks and use accumulating (_A) handlers."""
    run = runs[False][2]
    tapes = run["batches"]["leafpair"]["tapes"]
    assert all(t["p_candidate"] and t["P"] is not None and not t["fc"]["fc"] for t in tapes)
    hist = {}
    for t in tapes:
        for q in t["P"]:
            hist[q] = hist.get(q, 0) + 1
    for kind in ("ADDVV", "SUBVV", "BANDVV", "BORVV", "BXORVV", "MULVV", "ADDCV", "SUBCV", "BANDCV", "BORCV",
                 "BXORCV", "MULCV"):
        assert hist.get(kind, 0) + hist.get("PF_" + kind, 0) > 0, (kind, hist)
    assert sum(v for k, v in hist.items() if k.startswith("PF_")) > 0, hist
    on_g = [t for t in run["batches"]["boolheavy"]["tapes"] if not t["fc"]["fc"]]
    assert on_g and all(t["G0"] is not None and not t["p_candidate"] for t in on_g)
    hist = {}
    for t in on_g:
        for q in t["G0"]:
            hist[q] = hist.get(q, 0) + 1
    assert hist.get("PUSH_PKB", 0) + hist.get("PUSH_PKB_A", 0) + hist.get("PUSH_PKB_O", 0) > 0, hist
    assert any(k.endswith("_A") for k in hist), hist
    assert 0 < run["batches"]["boolheavy"]["fca"]["tapes"] <= sum(t["fc"]["fc"] for t in run["batches"]["boolheavy"]["tapes"])
