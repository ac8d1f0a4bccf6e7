"""ctypes mirror of the structs in ``include/mq.h`` (the C-ABI boundary).

``as_tape_batch`` / ``as_model_batch`` build the C structs over numpy buffers owned by
the returned keep-alive tuple; the library copies everything it needs.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .tape import TapeBatch
from .models import ModelBatch


class MqNode(C.Structure):
    _fields_ = [("op", C.c_uint16), ("width", C.c_uint16), ("a", C.c_uint32), ("b", C.c_uint32), ("c", C.c_uint32)]


class MqTapeBatch(C.Structure):
    _fields_ = [
        ("n_tapes", C.c_int32),
        ("tape_offsets", C.POINTER(C.c_int64)),
        ("nodes", C.c_void_p),
        ("const_words", C.POINTER(C.c_uint32)),
        ("n_const_words", C.c_int64),
    ]


class MqFuncDesc(C.Structure):
    _fields_ = [("arity", C.c_uint16), ("result_width", C.c_uint16), ("arg_width", C.c_uint16 * 2)]


class MqModelBatch(C.Structure):
    _fields_ = [
        ("n_models", C.c_int64),
        ("index_base", C.c_int64),
        ("n_vars", C.c_int32),
        ("var_width", C.POINTER(C.c_uint16)),
        ("var_words", C.POINTER(C.c_uint32)),
        ("n_funcs", C.c_int32),
        ("funcs", C.c_void_p),
        ("entry_ptr", C.POINTER(C.c_int64)),
        ("entry_base", C.POINTER(C.c_int64)),
        ("entry_words", C.POINTER(C.c_uint32)),
        ("n_entry_words", C.c_int64),
        ("else_base", C.POINTER(C.c_int64)),
        ("else_words", C.POINTER(C.c_uint32)),
        ("n_else_words", C.c_int64),
    ]


class MqRowPatch(C.Structure):
    _fields_ = [("row", C.c_uint32), ("keep", C.c_uint32), ("bits", C.c_uint32)]


class MqRowFloor(C.Structure):
    _fields_ = [("row0", C.c_uint32), ("n_limbs", C.c_uint32), ("minimum", C.c_uint32)]


class MqDerivation(C.Structure):
    _fields_ = [
        ("n_base", C.c_int64),
        ("base_words", C.POINTER(C.c_uint32)),
        ("n_derived", C.c_int64),
        ("src", C.POINTER(C.c_int32)),
        ("n_blocks", C.c_int32),
        ("block_start", C.POINTER(C.c_int64)),
        ("patch_ptr", C.POINTER(C.c_int64)),
        ("patches", C.POINTER(MqRowPatch)),
        ("floor_ptr", C.POINTER(C.c_int64)),
        ("floors", C.POINTER(MqRowFloor)),
    ]


class MqTableAdd(C.Structure):
    _fields_ = [("func", C.c_int32), ("var", C.c_int32), ("key_off", C.c_int64)]


class MqTableDerivation(C.Structure):
    _fields_ = [
        ("base", C.POINTER(MqModelBatch)),
        ("add_ptr", C.POINTER(C.c_int64)),
        ("adds", C.POINTER(MqTableAdd)),
        ("key_words", C.POINTER(C.c_uint32)),
        ("n_key_words", C.c_int64),
    ]


class MqKeccakWord(C.Structure):
    _fields_ = [("row", C.c_uint32), ("value", C.c_uint32)]


class MqKeccakInverse(C.Structure):
    _fields_ = [("func", C.c_int32), ("lo_word", C.c_uint32)]


class MqKeccakCollision(C.Structure):
    _fields_ = [("var", C.c_int32), ("pad", C.c_int32), ("key_off", C.c_int64)]


class MqKeccakSite(C.Structure):
    _fields_ = [
        ("func", C.c_int32),
        ("n_words", C.c_uint32),
        ("map_off", C.c_int64),
        ("inv_off", C.c_int32),
        ("n_inv", C.c_int32),
        ("coll_off", C.c_int32),
        ("n_coll", C.c_int32),
        ("b", C.c_uint32),
        ("pad", C.c_uint32),
        ("base", C.c_uint32 * 8),
    ]


class MqKeccakDerivation(C.Structure):
    _fields_ = [
        ("n_sites", C.c_int32),
        ("sites", C.POINTER(MqKeccakSite)),
        ("words", C.POINTER(MqKeccakWord)),
        ("n_words", C.c_int64),
        ("inverses", C.POINTER(MqKeccakInverse)),
        ("n_inverses", C.c_int64),
        ("collisions", C.POINTER(MqKeccakCollision)),
        ("n_collisions", C.c_int64),
        ("key_words", C.POINTER(C.c_uint32)),
        ("n_key_words", C.c_int64),
        ("active", C.POINTER(C.c_uint64)),
    ]


class MqStats(C.Structure):
    _fields_ = [
        ("kernel_ms", C.c_double),
        ("node_evals", C.c_double),
        ("alg_ops", C.c_double),
        ("pairs_evaluated", C.c_int64),
        ("n_hits", C.c_int32),
        ("n_unsupported", C.c_int32),
    ]


class MqDagBatch(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int64),
        ("nodes", C.c_void_p),
        ("const_words", C.POINTER(C.c_uint32)),
        ("n_const_words", C.c_int64),
        ("n_tapes", C.c_int32),
        ("root_offsets", C.POINTER(C.c_int64)),
        ("roots", C.POINTER(C.c_uint32)),
    ]


def _ptr(arr: np.ndarray, ctype):
    return arr.ctypes.data_as(C.POINTER(ctype))


def as_tape_batch(tb: TapeBatch):
    nodes = np.ascontiguousarray(tb.nodes)
    offs = np.ascontiguousarray(tb.offsets, dtype=np.int64)
    consts = np.ascontiguousarray(tb.consts, dtype=np.uint32)
    s = MqTapeBatch(tb.n_tapes, _ptr(offs, C.c_int64), nodes.ctypes.data, _ptr(consts, C.c_uint32), consts.size)
    return s, (nodes, offs, consts)


def as_model_batch(mb: ModelBatch):
    vw = np.ascontiguousarray(mb.var_widths, dtype=np.uint16)
    if vw.size == 0:
        vw = np.zeros(1, np.uint16)
    # (a derived batch carries no rows: mq_models_upload_derived ignores var_words)
    words = np.ascontiguousarray(mb.var_words, dtype=np.uint32) if mb.var_words is not None else np.zeros(1, np.uint32)
    if words.size == 0:
        words = np.zeros(1, np.uint32)
    funcs = np.ascontiguousarray(mb.func_arr)
    if mb.entry_ptr is None:
        # (a batch whose tables are derived too: mq_models_upload_derived_tables reads the widths,
        # the function signatures and index_base only)
        null32, null64 = C.POINTER(C.c_uint32)(), C.POINTER(C.c_int64)()
        s = MqModelBatch(mb.n_models, mb.index_base, mb.n_vars, _ptr(vw, C.c_uint16), null32, len(mb.funcs),
                         funcs.ctypes.data, null64, null64, null32, 0, null64, null32, 0)
        return s, (vw, funcs)
    eptr = np.ascontiguousarray(mb.entry_ptr, dtype=np.int64)
    ebase = np.ascontiguousarray(mb.entry_base, dtype=np.int64)
    ew = np.ascontiguousarray(mb.entry_words, dtype=np.uint32)
    elb = np.ascontiguousarray(mb.else_base, dtype=np.int64)
    elw = np.ascontiguousarray(mb.else_words, dtype=np.uint32)
    s = MqModelBatch(
        mb.n_models, mb.index_base, mb.n_vars, _ptr(vw, C.c_uint16),
        _ptr(words, C.c_uint32) if mb.var_words is not None else C.POINTER(C.c_uint32)(),
        len(mb.funcs), funcs.ctypes.data, _ptr(eptr, C.c_int64), _ptr(ebase, C.c_int64),
        _ptr(ew, C.c_uint32), ew.size, _ptr(elb, C.c_int64), _ptr(elw, C.c_uint32), elw.size)
    return s, (vw, words, funcs, eptr, ebase, ew, elb, elw)


def as_derivation(d):
    """``mq_derivation`` over the arrays of a :class:`mythril_amd.candidates.Derivation`."""
    base = np.ascontiguousarray(d.base_words, dtype=np.uint32)
    n_base = int(d.n_base)
    src = np.ascontiguousarray(d.src, dtype=np.int32)
    bs = np.ascontiguousarray(d.block_start, dtype=np.int64)
    pp = np.ascontiguousarray(d.patch_ptr, dtype=np.int64)
    fp = np.ascontiguousarray(d.floor_ptr, dtype=np.int64)
    pa = np.ascontiguousarray(d.patches, dtype=np.uint32).reshape(-1, 3)
    fl = np.ascontiguousarray(d.floors, dtype=np.uint32).reshape(-1, 3)

    def ptr(a, ctype):
        return C.cast(a.ctypes.data, C.POINTER(ctype)) if a.size else C.POINTER(ctype)()
    s = MqDerivation(n_base, ptr(base, C.c_uint32), len(src), ptr(src, C.c_int32), len(bs) - 1,
                     ptr(bs, C.c_int64), ptr(pp, C.c_int64), ptr(pa, MqRowPatch), ptr(fp, C.c_int64), ptr(fl, MqRowFloor))
    return s, (base, src, bs, pp, fp, pa, fl)


def as_table_derivation(t):
    """``mq_table_derivation`` over a :class:`mythril_amd.candidates.TableDerivation`."""
    base, keep_b = as_model_batch(t.base)
    ap = np.ascontiguousarray(t.add_ptr, dtype=np.int64)
    adds = np.zeros(len(t.add_func), dtype=np.dtype([("func", "<i4"), ("var", "<i4"), ("key_off", "<i8")]))
    adds["func"], adds["var"], adds["key_off"] = t.add_func, t.add_var, t.add_key_off
    keys = np.ascontiguousarray(t.key_words, dtype=np.uint32)

    def ptr(a, ctype):
        return C.cast(a.ctypes.data, C.POINTER(ctype)) if a.size else C.POINTER(ctype)()
    s = MqTableDerivation(C.pointer(base), ptr(ap, C.c_int64), ptr(adds, MqTableAdd), ptr(keys, C.c_uint32), keys.size)
    return s, (base, keep_b, ap, adds, keys)


def keccak_derivation_arrays(ks):
    """The arrays of ``mq_keccak_derivation`` for a :class:`mythril_amd.candidates.KeccakSites`:
    ``(sites, words, inverses, collisions, key_words, active)`` (structured numpy arrays)."""
    from .tape import to_words
    sites = np.zeros(len(ks.sites), np.dtype([("func", "<i4"), ("n_words", "<u4"), ("map_off", "<i8"), ("inv_off", "<i4"),
                                              ("n_inv", "<i4"), ("coll_off", "<i4"), ("n_coll", "<i4"), ("b", "<u4"),
                                              ("pad", "<u4"), ("base", "<u4", (8,))]))
    words, invs, colls, keys = [], [], [], []
    for i, s in enumerate(ks.sites):
        sites[i] = (s.func, s.n_bits // 32, len(words), len(invs), len(s.inverses), len(colls), len(s.collisions), s.b, 0,
                    to_words(s.base, 256))
        words += [(0xFFFFFFFF, cv) if row < 0 else (row, 0) for row, cv in s.words]
        invs += [(g, lo // 32) for g, lo, _ in s.inverses]
        for key, var, _ in s.collisions:
            colls.append((var, 0, len(keys)))
            keys += to_words(key, s.n_bits)
    return (sites, np.asarray(words, np.dtype([("row", "<u4"), ("value", "<u4")])),
            np.asarray(invs, np.dtype([("func", "<i4"), ("lo_word", "<u4")])),
            np.asarray(colls, np.dtype([("var", "<i4"), ("pad", "<i4"), ("key_off", "<i8")])),
            np.asarray(keys, np.uint32), np.ascontiguousarray(ks.active, np.uint64))


def as_keccak_derivation(ks, arrays=None):
    """``mq_keccak_derivation`` over a :class:`mythril_amd.candidates.KeccakSites` (``arrays``: the
    tuple of :func:`keccak_derivation_arrays`, to pass altered ones)."""
    sites, words, invs, colls, keys, active = arrays if arrays is not None else keccak_derivation_arrays(ks)

    def ptr(a, ctype):
        return C.cast(a.ctypes.data, C.POINTER(ctype)) if a.size else C.POINTER(ctype)()
    s = MqKeccakDerivation(len(sites), ptr(sites, MqKeccakSite), ptr(words, MqKeccakWord), len(words),
                           ptr(invs, MqKeccakInverse), len(invs), ptr(colls, MqKeccakCollision), len(colls),
                           ptr(keys, C.c_uint32), keys.size, ptr(active, C.c_uint64))
    return s, (sites, words, invs, colls, keys, active)


def as_dag_batch(db):
    nodes = np.ascontiguousarray(db.nodes)
    consts = np.ascontiguousarray(db.consts, dtype=np.uint32)
    offs = np.ascontiguousarray(db.root_offsets, dtype=np.int64)
    roots = np.ascontiguousarray(db.roots, dtype=np.uint32)
    if roots.size == 0:
        roots = np.zeros(1, np.uint32)
    s = MqDagBatch(len(nodes), nodes.ctypes.data if len(nodes) else None, _ptr(consts, C.c_uint32), consts.size,
                   db.n_tapes, _ptr(offs, C.c_int64), _ptr(roots, C.c_uint32))
    return s, (nodes, consts, offs, roots)
