"""The candidates' rows as a derivation (mythril_amd/candidates.py Derivation, include/mq.h
mq_derivation) on CPU: a literal numpy applier of the derivation reproduces _candidate_rows word
for word, hand-built patches hit the edges, the function tables of a ``device_rows`` generator
equal the default's, the C-ABI mirrors match the header, and malformed derivations are refused
by the host-side check (no device)."""
import ctypes
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from mythril_amd import candidates as C
from mythril_amd import evaluator
from mythril_amd._abi import MqDerivation, MqRowFloor, MqRowPatch, as_derivation, as_model_batch
from mythril_amd.lower import IncrementalLowering
from mythril_amd.models import ModelBatch
from mythril_amd.synth_evm import fork_workload
from mythril_amd.tape import limbs, to_words

from derivation_util import T_KEY, T_PATCHES, T_SIZES, apply_derivation, table_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MQ_ERR_ARG = -1


def _generate(n_models, seed, **kw):
    exprs, recs, _ = fork_workload(8, 12, seed=seed)
    recs = recs[:n_models]
    inc = IncrementalLowering()
    db, ok = inc.lower(exprs)
    return C.CandidateGenerator(3000, seed=2, **kw).generate(db, inc.syms, inc.serialize(recs), recs)


@pytest.mark.parametrize("py_rows", [False, True])
@pytest.mark.parametrize("n_models,seed", [(12, 3), (12, 7), (0, 3)])
def test_applied_derivation_is_candidate_rows(monkeypatch, n_models, seed, py_rows):
    if py_rows:
        monkeypatch.setenv("MQ_PY_CANDIDATES", "1")
    else:
        monkeypatch.delenv("MQ_PY_CANDIDATES", raising=False)
    ref = _generate(n_models, seed)
    cs = _generate(n_models, seed, device_rows=True)
    d = cs.derivation
    assert cs.batch.var_words is None and d.n_base == n_models == cs.n_lru
    assert d.n_derived == ref.n_generated > 50 and len(d.patches) > 0 and len(d.floors) > 0
    assert (d.src == (-1 if n_models == 0 else cs.base)).all()
    want = ref.batch.var_words
    assert (apply_derivation(d, want.shape[0]) == want).all()
    assert (cs.rows() == want).all()
    assert (cs.host_batch().var_words == want).all()
    # nothing of size rows x K is described: base rows + tables
    assert d.upload_bytes() == 4 * d.base_words.size + 12 * len(d.patches) + 12 * len(d.floors) + 4 * d.n_derived
    assert d.upload_bytes() < 4 * want.size // 2


# ---------------------------------------------------------------- hand-built patches
WIDTHS = [0, 8, 33, 256, 512, 64]


def _hand_lru(n):
    rng = np.random.default_rng(5)
    models = []
    for m in range(n):
        vs = {v: int.from_bytes(rng.bytes(64), "little") & ((1 << max(w, 1)) - 1) for v, w in enumerate(WIDTHS)}
        models.append({"vars": vs})
    # the size variable (5): high limb nonzero / low limb small / low limb large
    sizes = [(7 << 32) | 3, 5, 100]
    for m in range(n):
        models[m]["vars"][5] = sizes[m % 3]
    return ModelBatch.from_python(WIDTHS, models), models


HAND_BLOCKS = [
    (((3, 28, 10, 0x2AB),), np.asarray([0, 1, 2], np.int64)),                       # crosses a limb boundary
    (((1, 0, 8, 0xFF), (1, 4, 4, 0x0), (4, 500, 12, 0xABC), (4, 504, 4, 0x5)),      # overlapping bits: last wins
     np.asarray([2, 0, 1], np.int64)),
    (((5, -1, 0, 37), (2, 30, 3, 0b101)), np.asarray([0, 1, 2], np.int64)),          # a floor (+ a 33-bit variable)
    (((0, 0, 1, 1), (5, 0, 64, 9), (5, -1, 0, 37)), np.asarray([1, 2], np.int64)),   # a partial last block; floor after a patch
]


def _literal(models, blocks):
    """Expected rows from Python integers (a base of -1: the all-zero model)."""
    off = np.concatenate([[0], np.cumsum([limbs(w) for w in WIDTHS])])
    cols = []
    for patch, bases in blocks:
        for b in bases:
            vals = dict(models[b]["vars"]) if b >= 0 else {v: 0 for v in range(len(WIDTHS))}
            for v, lo, n, bits in [p for p in patch if p[1] >= 0]:
                vals[v] = (vals[v] & ~(((1 << n) - 1) << lo)) | (bits << lo)
            for v, lo, n, mn in [p for p in patch if p[1] < 0]:
                if vals[v] < (1 << 32) and vals[v] < mn:
                    vals[v] = mn
            col = np.zeros(int(off[-1]), np.uint32)
            for v, w in enumerate(WIDTHS):
                col[off[v]:off[v + 1]] = to_words(vals[v], w)
            cols.append(col)
    return np.stack(cols, axis=1)


def _hand_derivation(lru, blocks):
    syms = SimpleNamespace(var_widths=WIDTHS)
    sizes = np.asarray([len(b) for _, b in blocks], np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    base = np.concatenate([b for _, b in blocks])
    off = lru.var_word_offsets()
    return C.derivation_arrays(lru, base, blocks, starts, sizes, off, syms), (syms, sizes, starts, base, off)


@pytest.mark.parametrize("py_rows", [False, True])
def test_hand_built_patches(monkeypatch, py_rows):
    if py_rows:
        monkeypatch.setenv("MQ_PY_CANDIDATES", "1")
    else:
        monkeypatch.delenv("MQ_PY_CANDIDATES", raising=False)
    lru, models = _hand_lru(3)
    d, (syms, sizes, starts, base, off) = _hand_derivation(lru, HAND_BLOCKS)
    rows = int(off[-1])
    got = apply_derivation(d, rows)
    want = _literal(models, HAND_BLOCKS)
    assert (got[:, :3] == lru.var_words).all() and (got[:, 3:] == want).all()
    assert (C._candidate_rows(lru, base, starts, sizes, HAND_BLOCKS, syms, off, len(base)) == got).all()
    # the composed words themselves
    p0 = d.patches[d.patch_ptr[0]:d.patch_ptr[1]]
    r3 = int(off[3])
    assert p0.tolist() == [[r3, 0x0FFFFFFF, 0xB0000000], [r3 + 1, 0xFFFFFFC0, 0x2A]]
    p1 = d.patches[d.patch_ptr[1]:d.patch_ptr[2]]
    assert p1.tolist() == [[int(off[1]), 0xFFFFFF00, 0x0F], [int(off[4]) + 15, 0x000FFFFF, 0xA5C00000]]
    assert d.floors.tolist() == [[int(off[5]), 2, 37], [int(off[5]), 2, 37]]
    assert d.floor_ptr.tolist() == [0, 0, 0, 1, 2] and d.block_start.tolist() == [0, 3, 6, 9, 11]
    # the floor: not applied (high limb nonzero), applied (5 -> 37), not applied (100)
    r5 = int(off[5])
    assert got[r5:r5 + 2, 3 + 6:3 + 9].T.tolist() == [[3, 7], [37, 0], [100, 0]]
    assert got[r5:r5 + 2, 3 + 9:].T.tolist() == [[37, 0], [37, 0]]   # patched to 9 first, then floored


def test_hand_built_zero_source():
    """src = -1: the candidate starts from all-zero rows (no base model)."""
    lru, models = _hand_lru(3)
    blocks = [(HAND_BLOCKS[0][0], np.asarray([-1, 1, -1], np.int64)), (HAND_BLOCKS[3][0], np.asarray([-1], np.int64))]
    d, (_, _, _, _, off) = _hand_derivation(lru, blocks)
    assert d.src.tolist() == [-1, 1, -1, -1]
    got = apply_derivation(d, int(off[-1]))
    assert (got[:, 3:] == _literal(models, blocks)).all()
    # and with no base models at all
    empty = ModelBatch.from_python(WIDTHS, [])
    blocks0 = [(p, np.full(len(b), -1, np.int64)) for p, b in HAND_BLOCKS]
    d0, (syms, sizes, starts, base, off) = _hand_derivation(empty, blocks0)
    assert d0.n_base == 0 and (d0.src == -1).all()
    got0 = apply_derivation(d0, int(off[-1]))
    assert (got0 == _literal(models, blocks0)).all()
    assert (C._candidate_rows(empty, np.zeros(len(base), np.int64), starts, sizes, blocks0, syms, off, len(base)) == got0).all()


# ---------------------------------------------------------------- function tables
@pytest.mark.parametrize("n_models", [12, 0])
def test_device_rows_function_tables_equal_the_default(n_models):
    ref = _generate(n_models, 3)
    cs = _generate(n_models, 3, device_rows=True)
    a, b = ref.batch, cs.batch
    assert a.funcs and b.n_models == a.n_models and (b.var_widths == a.var_widths).all()
    for name in ("entry_ptr", "entry_words", "entry_base", "else_words", "else_base", "func_arr"):
        assert (getattr(a, name) == getattr(b, name)).all(), name
    assert (cs.base == ref.base).all() and (cs.block_of == ref.block_of).all() and cs.block_patches == ref.block_patches
    k = ref.n_lru + ref.n_generated // 2
    assert cs.materialize(k).assignment == ref.materialize(k).assignment


@pytest.mark.parametrize("n_base", [3, 0])
def test_patched_derived_entries_without_the_matrix(n_base):
    """A candidate whose patch changes a derived variable (the function's value at a constant key)
    gets that entry in its table, holding the patched and floored value: computed from the composed
    (keep, bits) and floors alone under ``device_rows``, equal to the default's."""
    ref, models = table_case(n_base, False)
    cs, _ = table_case(n_base, True)
    a, b = ref.batch, cs.batch
    assert b.var_words is None and b.n_models == a.n_models == n_base + sum(T_SIZES)
    for name in ("entry_ptr", "entry_words", "entry_base", "else_words", "else_base"):
        assert (getattr(a, name) == getattr(b, name)).all(), name
    assert (apply_derivation(cs.derivation, a.var_words.shape[0]) == a.var_words).all()
    host = cs.host_batch()
    k = 0
    for j, n in enumerate(T_SIZES):
        for _ in range(n):
            m = n_base + k
            table, els = host.func_table(0, m)
            base = int(cs.base[k])
            want = models[base]["vars"][1] if base >= 0 else 0
            for v, lo, nb, bits in [p for p in T_PATCHES[j] if p[0] == 1 and p[1] >= 0]:
                want = (want & ~(((1 << nb) - 1) << lo)) | (bits << lo)
            for v, lo, nb, mn in [p for p in T_PATCHES[j] if p[0] == 1 and p[1] < 0]:
                want = max(want, mn)
            assert table[(T_KEY,)] == want == host.var_value(1, m), (j, k)
            assert els == (base + 1 if base >= 0 else 0)
            k += 1
    assert {host.var_value(1, n_base + 64 + i) for i in range(3)} == ({0x40, 0x98, 0x59} if n_base else {0x40})


# ---------------------------------------------------------------- C-ABI
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "mq.h")).read()
    lib = evaluator.load_library()
    for name in ("mq_models_upload_derived", "mq_models_download_vars", "mq_derivation_check"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name
        assert hasattr(lib, name), name
    for name in ("mq_row_patch", "mq_row_floor", "mq_derivation"):
        assert re.search(r"typedef struct %s\b" % name, header), name


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mq.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mq_row_patch), sizeof(mq_row_floor),'
                   ' sizeof(mq_derivation), offsetof(mq_derivation, src), offsetof(mq_derivation, block_start),'
                   ' offsetof(mq_derivation, floors)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(MqRowPatch), ctypes.sizeof(MqRowFloor), ctypes.sizeof(MqDerivation),
                   MqDerivation.src.offset, MqDerivation.block_start.offset, MqDerivation.floors.offset]
    assert got[:3] == [12, 12, 80]


# ---------------------------------------------------------------- argument errors (host check, no device)
def _check(mb, d):
    lib = evaluator.load_library()
    s, keep = as_model_batch(mb)
    ds, keep_d = as_derivation(d)
    rc = lib.mq_derivation_check(ctypes.byref(s), ctypes.byref(ds))
    # the upload runs the same check before it looks at the context or the device
    assert lib.mq_models_upload_derived(None, ctypes.byref(s), ctypes.byref(ds)) == MQ_ERR_ARG
    return rc


def _valid():
    lru, _ = _hand_lru(3)
    d, (_, _, _, base, off) = _hand_derivation(lru, HAND_BLOCKS)
    mb = ModelBatch(WIDTHS, None, n_models=3 + len(base))
    return mb, d, int(off[-1])


def test_well_formed_derivation_passes_the_check():
    mb, d, rows = _valid()
    assert _check(mb, d) == 0
    empty = ModelBatch.from_python(WIDTHS, [])
    d0, _ = _hand_derivation(empty, [(p, np.full(len(b), -1, np.int64)) for p, b in HAND_BLOCKS])
    assert _check(ModelBatch(WIDTHS, None, n_models=d0.n_derived), d0) == 0


def _break(name):
    mb, d, rows = _valid()
    if name == "src_past_base":
        d.src[4] = 3
    elif name == "src_below_minus_one":
        d.src[0] = -2
    elif name == "patch_row_past_rows":
        d.patches[1, 0] = rows
    elif name == "floor_past_rows":
        d.floors[0, 0] = rows - 1
    elif name == "floor_without_limbs":
        d.floors[1, 1] = 0
    elif name == "block_start_not_monotone":
        d.block_start[2] = 2
    elif name == "block_start_not_ending_at_k":
        d.block_start[-1] -= 1
    elif name == "patch_ptr_not_monotone":
        d.patch_ptr[2] = d.patch_ptr[1] - 1
    elif name == "floor_ptr_not_monotone":
        d.floor_ptr[2] = 2
    elif name == "counts_do_not_add_up":
        mb = ModelBatch(WIDTHS, None, n_models=mb.n_models + 1)
    elif name == "base_plus_derived_short":
        mb = ModelBatch(WIDTHS, None, n_models=mb.n_models - 3)
    else:
        raise AssertionError(name)
    return mb, d


@pytest.mark.parametrize("name", ["src_past_base", "src_below_minus_one", "patch_row_past_rows", "floor_past_rows",
                                  "floor_without_limbs", "block_start_not_monotone", "block_start_not_ending_at_k",
                                  "patch_ptr_not_monotone", "floor_ptr_not_monotone", "counts_do_not_add_up",
                                  "base_plus_derived_short"])
def test_malformed_derivation_is_an_argument_error(name):
    mb, d = _break(name)
    assert _check(mb, d) == MQ_ERR_ARG
