"""The candidates' function tables as a derivation (mythril_amd/candidates.py TableDerivation,
include/mq.h mq_table_derivation) on CPU: a literal applier of the table derivation reproduces the
tables CandidateGenerator._serialize materialises, array for array; the host-side check accepts the
hand-built case and refuses one malformed variant per rule (no device); the generator's arguments;
the C-ABI mirrors match the header.

The hand-built case is table_derivation_util's (see its docstring for which function is dense)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mythril_amd import candidates as C
from mythril_amd import evaluator
from mythril_amd._abi import MqTableAdd, MqTableDerivation, as_derivation, as_model_batch, as_table_derivation
from mythril_amd.lower import IncrementalLowering
from mythril_amd.models import ModelBatch
from mythril_amd.synth_evm import fork_workload
from mythril_amd.tape import limbs, to_words

from table_derivation_util import (X_FUNCS, X_KEY, X_KEY2, X_PKEY, X_SIZES, X_WIDTHS, apply_table_derivation, dense_e,
                                   x_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MQ_OK, MQ_ERR_ARG = 0, -1
TABLES = ("entry_ptr", "entry_words", "entry_base", "else_words", "else_base")


def _generate(n_models, seed, **kw):
    exprs, recs, _ = fork_workload(8, 12, seed=seed)
    recs = recs[:n_models]
    inc = IncrementalLowering()
    db, ok = inc.lower(exprs)
    return C.CandidateGenerator(3000, seed=2, **kw).generate(db, inc.syms, inc.serialize(recs), recs)


# ---------------------------------------------------------------- the literal applier
@pytest.mark.parametrize("n_base", [3, 0])
def test_applied_table_derivation_is_the_materialised_tables(n_base):
    ref, _ = x_case(n_base)
    cs, _ = x_case(n_base, True, True)
    t, d = cs.table_derivation, cs.derivation
    K = sum(X_SIZES)
    assert d.n_base == n_base and d.n_derived == K == 130 and d.block_start.tolist() == [0, 64, 129, 130]
    # block 0 adds two entries to function 0, block 1 one to each function, block 2 none;
    # per function by ascending variable
    assert t.add_ptr.tolist() == [0, 2, 4, 4]
    assert list(zip(t.add_func.tolist(), t.add_var.tolist())) == [(0, 1), (0, 5), (0, 1), (1, 3)]
    pool = {1: to_words(X_KEY, 256), 5: to_words(X_KEY2, 256), 3: to_words(X_PKEY[0], 256) + to_words(X_PKEY[1], 256)}
    for v, ko in zip(t.add_var.tolist(), t.add_key_off.tolist()):
        assert t.key_words[ko:ko + len(pool[v])].tolist() == list(pool[v])
    if n_base:
        assert np.diff(t.base.entry_ptr[0]).tolist() == [0, 1, 3]       # base models with 0, 1 and 3 entries
        assert np.diff(t.base.entry_ptr[1]).tolist() == [0, 1, 17]
    else:
        assert (d.src == -1).all()
    got = apply_table_derivation(t, d, X_FUNCS, X_WIDTHS)
    for name, g in zip(TABLES, got):
        want = getattr(ref.batch, name)
        assert g.shape == want.shape and (g == want).all(), name
    if n_base == 0:
        # only the additions, else value 0
        assert np.diff(got[0][0]).tolist() == [2] * 64 + [1] * 65 + [0]
        assert np.diff(got[0][1]).tolist() == [0] * 64 + [1] * 65 + [0]
        assert not got[3].any()
    # function 0 is dense, function 1 is not (upload_one's rule, restated in dense_e)
    M = n_base + K
    assert dense_e(X_FUNCS[0], got[0][0], M) == (5 if n_base else 2)
    assert dense_e(X_FUNCS[1], got[0][1], M) == 0
    if n_base:
        assert np.diff(got[0][1]).max() == 18 > 16


@pytest.mark.parametrize("n_models", [12, 0])
def test_generated_table_derivation_is_the_materialised_tables(n_models):
    ref = _generate(n_models, 3)
    cs = _generate(n_models, 3, device_rows=True, device_tables=True)
    assert ref.batch.funcs and cs.table_derivation is not None
    got = apply_table_derivation(cs.table_derivation, cs.derivation, ref.batch.funcs, ref.batch.var_widths)
    for name, g in zip(TABLES, got):
        assert (g == getattr(ref.batch, name)).all(), name
    # the description is O(n_lru + blocks): far below the materialised tables
    a = ref.batch
    assert cs.table_derivation.upload_bytes() < (8 * a.entry_ptr.size + 4 * a.entry_words.size + 4 * a.else_words.size) // 2


# ---------------------------------------------------------------- generator arguments
def test_device_tables_needs_device_rows():
    with pytest.raises(ValueError):
        C.CandidateGenerator(device_tables=True)
    with pytest.raises(ValueError):
        C.CandidateGenerator(device_rows=False, device_tables=True)


@pytest.mark.parametrize("n_models", [12, 0])
def test_device_tables_batch_carries_no_per_model_arrays(n_models):
    ref = _generate(n_models, 3)
    rows_only = _generate(n_models, 3, device_rows=True)
    cs = _generate(n_models, 3, device_rows=True, device_tables=True)
    b = cs.batch
    assert b.var_words is None and all(getattr(b, name) is None for name in TABLES)
    assert b.n_models == ref.batch.n_models and (b.func_arr == ref.batch.func_arr).all()
    assert rows_only.table_derivation is None and ref.table_derivation is None
    host = cs.host_batch()
    for name in ("var_words",) + TABLES:
        assert (getattr(host, name) == getattr(ref.batch, name)).all(), name
    k = ref.n_lru + ref.n_generated // 2
    assert cs.materialize(k).assignment == ref.materialize(k).assignment


@pytest.mark.parametrize("n_base", [3, 0])
def test_hand_built_host_batch_equals_the_default(n_base):
    ref, _ = x_case(n_base)
    cs, _ = x_case(n_base, True, True)
    host = cs.host_batch()
    for name in ("var_words",) + TABLES:
        assert (getattr(host, name) == getattr(ref.batch, name)).all(), name


# ---------------------------------------------------------------- C-ABI
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "mq.h")).read()
    lib = evaluator.load_library()
    for name in ("mq_models_upload_derived_tables", "mq_table_derivation_check", "mq_models_download_funcs",
                 "mq_models_funcs_sizes", "mq_table_scan_threads"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name
        assert hasattr(lib, name), name
    for name in ("mq_table_add", "mq_table_derivation"):
        assert re.search(r"typedef struct %s\b" % name, header), name
    assert lib.mq_table_scan_threads() >= 64


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mq.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mq_table_add), offsetof(mq_table_add, key_off),'
                   ' sizeof(mq_table_derivation), offsetof(mq_table_derivation, adds),'
                   ' offsetof(mq_table_derivation, n_key_words)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(MqTableAdd), MqTableAdd.key_off.offset, ctypes.sizeof(MqTableDerivation),
                   MqTableDerivation.adds.offset, MqTableDerivation.n_key_words.offset]
    assert got[0] == 16


# ---------------------------------------------------------------- argument errors (host check, no device)
def _check(mb, d, t):
    lib = evaluator.load_library()
    s, keep = as_model_batch(mb)
    ds, keep_d = as_derivation(d)
    ts, keep_t = as_table_derivation(t)
    rc = lib.mq_table_derivation_check(ctypes.byref(s), ctypes.byref(ds), ctypes.byref(ts))
    # the upload runs the same checks before it looks at the context or the device
    assert lib.mq_models_upload_derived_tables(None, ctypes.byref(s), ctypes.byref(ds), ctypes.byref(ts)) == MQ_ERR_ARG
    return rc


@pytest.mark.parametrize("n_base", [3, 0])
def test_well_formed_table_derivation_passes_the_check(n_base):
    cs, _ = x_case(n_base, True, True)
    assert _check(cs.batch, cs.derivation, cs.table_derivation) == MQ_OK


def _break(name):
    cs, models = x_case(3, True, True)
    mb, d, t = cs.batch, cs.derivation, cs.table_derivation
    if name == "add_ptr_not_from_zero":
        t.add_ptr[0] = 1
    elif name == "add_ptr_not_monotone":
        t.add_ptr[1] = 5
    elif name == "func_past_n_funcs":
        t.add_func[1] = 2
    elif name == "func_negative":
        t.add_func[0] = -1
    elif name == "var_past_n_vars":
        t.add_var[2] = len(X_WIDTHS)
    elif name == "var_limbs_differ_from_result":
        t.add_var[1] = 3              # a 256-bit variable as the value of an 8-bit function
    elif name == "key_past_pool":
        t.add_key_off[3] = len(t.key_words) - 15      # (16 key words needed)
    elif name == "key_negative":
        t.add_key_off[0] = -1
    elif name == "base_models_not_n_base":
        t.base = ModelBatch.from_python(X_WIDTHS, models[:2], X_FUNCS)
    elif name == "base_csr_not_monotone":
        t.base = ModelBatch.from_python(X_WIDTHS, models, X_FUNCS)
        t.base.entry_ptr[0, 2] = 5
    elif name == "base_entries_past_the_words":
        t.base = ModelBatch.from_python(X_WIDTHS, models, X_FUNCS)
        t.base.entry_ptr[1, 3] += 1
    elif name == "base_functions_differ":
        t.base = ModelBatch.from_python(X_WIDTHS, models, X_FUNCS[:1])
    elif name == "two_additions_of_one_variable":
        t.add_var[1] = 1              # block 0: (function 0, variable 1) twice
    elif name == "row_derivation_malformed":
        d.src[7] = 3
    else:
        raise AssertionError(name)
    return mb, d, t


@pytest.mark.parametrize("name", ["add_ptr_not_from_zero", "add_ptr_not_monotone", "func_past_n_funcs", "func_negative",
                                  "var_past_n_vars", "var_limbs_differ_from_result", "key_past_pool", "key_negative",
                                  "base_models_not_n_base", "base_csr_not_monotone", "base_entries_past_the_words",
                                  "base_functions_differ", "two_additions_of_one_variable", "row_derivation_malformed"])
def test_malformed_table_derivation_is_an_argument_error(name):
    assert _check(*_break(name)) == MQ_ERR_ARG
