"""Shared by the table-derivation tests: a literal applier of a TableDerivation, and a hand-built
candidate set that extends derivation_util.table_case — three blocks of 64, 65 and 1 candidates over
3 or 0 base models, two functions:

* function 0 ("cd"): one 256-bit key, 8-bit result.  Base models 0, 1, 2 hold 0, 1 and 3 entries.
  Variables 1 and 5 are its values at keys X_KEY and X_KEY2.  Block 0 patches both (two entries
  added to one function), block 1 patches variable 1 (one entry).  Its counts make it DENSE.
* function 1 ("Power"): two 256-bit keys, 256-bit result.  Base model 2 holds 17 entries, base
  model 1 one, base model 0 none.  Variable 3 is its value at X_PKEY; block 1 patches it (so block 1
  adds one entry to each function).  NOT dense: two arguments, and 17 entries are past the limit.

Block 2 patches no derived variable: it adds nothing."""
from types import SimpleNamespace

import numpy as np

from mythril_amd import candidates as C
from mythril_amd.models import FuncSpec, ModelBatch
from mythril_amd.tape import limbs

from derivation_util import T_BIG, apply_derivation, mask_rows

X_WIDTHS = [0, 8, 33, 256, 512, 8]
X_FUNCS = [FuncSpec(1, 8, (256,)), FuncSpec(2, 256, (256, 256))]
X_KEY, X_KEY2 = 5, (1 << 255) | 6
X_BASE_KEY, X_ABSENT_KEY = 9, 1234            # held by base model 2 only / by nobody
X_PKEY = (3, 1 << 200)
X_PBASE_KEY, X_PABSENT_KEY = (2, 7), (8, 8)
X_SIZES = (64, 65, 1)
X_PATCHES = [
    ((1, 0, 8, 0xA7), (5, 1, 6, 0x2B), (2, 3, 10, 0x2AB), (0, 0, 1, 1)),
    ((4, 500, 12, 0xABC), (3, 0, 256, T_BIG), (2, 30, 3, 0b101), (1, 2, 3, 0b110), (1, -1, 0, 0x40)),
    ((4, 3, 40, 0x9876543210), (2, 0, 33, 0x1_2345_6789)),
]
X_DERIVED = {1: ("cd", (X_KEY,)), 5: ("cd", (X_KEY2,)), 3: ("Power", X_PKEY)}


def x_models(n):
    rng = np.random.default_rng(11)
    out = []
    for m in range(n):
        vs = {v: int.from_bytes(rng.bytes(64), "little") & ((1 << max(w, 1)) - 1) for v, w in enumerate(X_WIDTHS)}
        vs[1] = [0x03, 0x9C, 0x41][m % 3]
        vs[0] = m & 1
        cd = [{}, {X_KEY: vs[1]}, {X_KEY: vs[1], X_BASE_KEY: 0x77, X_KEY2: vs[5]}][m % 3]
        pw = [{}, {X_PKEY: vs[3]}, {X_PBASE_KEY: 49, X_PKEY: vs[3], **{(2, 100 + i): i for i in range(15)}}][m % 3]
        out.append({"vars": vs, "funcs": {0: (cd, m + 1), 1: (pw, (m + 1) << 130)}})
    return out


def x_syms():
    return SimpleNamespace(var_widths=X_WIDTHS, derived=dict(X_DERIVED), func_names=["cd", "Power"])


def x_blocks(n_base, sizes=X_SIZES, patches=X_PATCHES):
    if n_base:
        bases = [(np.arange(n) + j) % n_base for j, n in enumerate(sizes)]
    else:
        bases = [np.full(n, -1, np.int64) for n in sizes]
    return [(p, np.asarray(b, np.int64)) for p, b in zip(patches, bases)]


def x_case(n_base, device_rows=False, device_tables=False):
    """The hand-built set through CandidateGenerator._serialize."""
    models = x_models(n_base)
    lru = ModelBatch.from_python(X_WIDTHS, models, X_FUNCS)
    gen = C.CandidateGenerator(device_rows=device_rows, device_tables=device_tables)
    return gen._serialize(lru, x_blocks(n_base), x_syms(), models), models


def apply_table_derivation(t, d, funcs, widths):
    """What mq_models_upload_derived_tables leaves resident, literally, in the host layout of
    mq_model_batch with the functions packed in order: (entry_ptr, entry_words, entry_base,
    else_words, else_base)."""
    off = np.concatenate([[0], np.cumsum([limbs(int(w)) for w in widths])])
    rows = mask_rows(apply_derivation(d, int(off[-1])), widths)
    b, nb, K = t.base, d.n_base, d.n_derived
    M = nb + K
    eptr = np.zeros((len(funcs), M + 1), np.int64)
    ebase, elb = np.zeros(len(funcs), np.int64), np.zeros(len(funcs), np.int64)
    ew, el = [], []
    for f, spec in enumerate(funcs):
        s, nr = spec.stride, limbs(spec.result_width)
        ebase[f], elb[f] = len(ew), len(el)

        def base_entries(m):
            lo, hi = int(b.entry_ptr[f, m]), int(b.entry_ptr[f, m + 1])
            return b.entry_words[int(b.entry_base[f]) + lo * s:int(b.entry_base[f]) + hi * s].tolist()

        def base_else(m):
            return b.else_words[int(b.else_base[f]) + m * nr:int(b.else_base[f]) + (m + 1) * nr].tolist()
        n = 0
        for m in range(M):
            eptr[f, m] = n
            if m < nb:
                words, els = base_entries(m), base_else(m)
            else:
                k = m - nb
                j = int(np.searchsorted(d.block_start, k, side="right")) - 1
                words = []
                for q in range(int(t.add_ptr[j]), int(t.add_ptr[j + 1])):
                    if t.add_func[q] != f:
                        continue
                    klen = s - nr
                    assert limbs(int(widths[t.add_var[q]])) == nr
                    words += t.key_words[int(t.add_key_off[q]):int(t.add_key_off[q]) + klen].tolist()
                    r0 = int(off[t.add_var[q]])
                    words += rows[r0:r0 + nr, m].tolist()
                src = int(d.src[k])
                words += base_entries(src) if src >= 0 else []
                els = base_else(src) if src >= 0 else [0] * nr
            ew += words
            el += els
            n += len(words) // s
        eptr[f, M] = n
    return eptr, np.asarray(ew, np.uint32), ebase, np.asarray(el, np.uint32), elb


def dense_e(spec, entry_ptr_row, M):
    """upload_one's rule restated: the dense slots per model of a function (0: not dense)."""
    nl_a0, nl_res = limbs(spec.arg_widths[0]), limbs(spec.result_width)
    counts = np.diff(entry_ptr_row)
    emax, total = int(counts.max(initial=0)), int(counts.sum())
    if spec.arity != 1 or nl_a0 > 8 or nl_res > 8 or M == 0:
        return 0
    words = emax * (nl_a0 + nl_res) * M
    if emax == 0 or emax > 16 or words > 2 * total * spec.stride + 16 * M:
        return 0
    return emax
