"""Shared by the keccak-candidate tests: a hand-built candidate set over four keccak sites.

Terms: 256-bit ``a``, ``p``, ``s``, ``z`` and a 1088-bit ``w`` (exactly one rate block: the pad
falls in the second block); the applications keccak256_256(a), keccak256_256(p) (two sites of one
function), keccak256_512(Concat(s, 1)) and keccak256_1088(w) under one KeccakFunctionManager's
axioms, plus keccak256_256(77): a lookup at a CONSTANT key, the collision rule's derived variable.

Base models (``n_lru`` of them, or none: every candidate then has ``src = -1``) hold consistent
tables.  keccak256_512-1 carries 15 more entries per model, 16 in all, so its 256-bit slices are
dense (16 slots) until a site adds a 17th entry; keccak256_256 and its inverse stay dense.

Blocks cycle through seven patches, each over every base model (37 candidates per block, so 64-wide
waves straddle blocks): one activating the 512-bit site, one both 256-bit sites, the 1088-bit site,
NO site (z only), the collision (a := 77), partial words of s and w, and three sites at once."""
import numpy as np

from mythril_amd import candidates as C
from mythril_amd import smt as S
from mythril_amd.function_managers import KeccakFunctionManager
from mythril_amd.lower import IncrementalLowering
from mythril_amd.smt_model import Model

K_COLLIDE = 77
N_LRU = 37
MODES = ({}, {"device_rows": True}, {"device_rows": True, "device_tables": True})
TABLES = ("entry_ptr", "entry_words", "entry_base", "else_words", "else_base")

_built = {}


def k_terms():
    """(variables, the four applications, axioms, manager), built once."""
    if "terms" not in _built:
        kfm = KeccakFunctionManager()
        v = {n: S.BitVecSym(n, 256) for n in ("a", "p", "s", "z")}
        v["w"] = S.BitVecSym("w", 1088)
        x512 = S.Concat(v["s"], S.BitVecVal(1, 256))
        apps = {"a": kfm.create_keccak(v["a"]), "p": kfm.create_keccak(v["p"]), "s": kfm.create_keccak(x512),
                "w": kfm.create_keccak(v["w"])}
        axioms = kfm.create_conditions()
        f256, _ = kfm.get_function(256)
        _built["terms"] = (v, apps, axioms, kfm, f256(S.BitVecVal(K_COLLIDE, 256)))
    return _built["terms"]


def k_consts(j: int):
    """The constants block j's patch writes."""
    rng = np.random.default_rng(1000 + j)
    return [int.from_bytes(rng.bytes(136), "big") for _ in range(4)]


def k_exprs():
    """Queries the candidates of blocks 0, 1, 2, 3 and 4 satisfy (block j of the first cycle)."""
    v, apps, axioms, kfm, at77 = k_terms()
    m256 = (1 << 256) - 1
    c = [k_consts(j) for j in range(5)]
    return [S.And(v["s"] == S.BitVecVal(c[0][0] & m256, 256), axioms),
            S.And(v["a"] == S.BitVecVal(c[1][0] & m256, 256), v["p"] == S.BitVecVal(c[1][1] & m256, 256), axioms),
            S.And(v["w"] == S.BitVecVal(c[2][0] & ((1 << 1088) - 1), 1088), axioms),
            S.And(v["z"] == S.BitVecVal(3, 256), axioms),
            S.And(v["a"] == S.BitVecVal(K_COLLIDE, 256), at77 == apps["a"]),
            S.And(S.Not(at77 == apps["a"]), v["z"] == S.BitVecVal(3, 256))]


def k_models(n):
    v, apps, axioms, kfm, _ = k_terms()
    rng = np.random.default_rng(5)
    par = {w: C.image_params(*kfm.interval(w)) for w in (256, 512, 1088)}

    def r(nbytes):
        return int.from_bytes(rng.bytes(nbytes), "big")
    out = []
    for m in range(n):
        a, p, s, z, w = r(32), r(32), r(20), r(32), r(136)
        at77 = {(K_COLLIDE,): r(32)} if m % 2 else {}    # every other model holds the constant key
        x512 = (s << 256) | 1
        va, vp = C.keccak_images([a, p], 256, *par[256])
        vs = C.keccak_images([x512], 512, *par[512])[0]
        vw = C.keccak_images([w], 1088, *par[1088])[0]
        junk = {(r(32),): r(64) for _ in range(15)}
        out.append(Model({"a": a, "p": p, "s": s, "z": z, "w": w},
                         {"keccak256_256": ({(a,): va, (p,): vp, **at77}, 0), "keccak256_256-1": ({(va,): a, (vp,): p}, 0),
                          "keccak256_512": ({(x512,): vs}, 0), "keccak256_512-1": ({(vs,): x512, **junk}, 0),
                          "keccak256_1088": ({(w,): vw}, 0), "keccak256_1088-1": ({(vw,): w}, 0)}))
    return out


def k_patches(syms, n_blocks):
    var = {name: syms.vars[(name, 1088 if name == "w" else 256)] for name in ("a", "p", "s", "z", "w")}
    m256 = (1 << 256) - 1
    out = []
    for j in range(n_blocks):
        c = k_consts(j)
        out.append([
            ((var["s"], 0, 256, c[0] & m256),),
            ((var["a"], 0, 256, c[0] & m256), (var["p"], 0, 256, c[1] & m256)),
            ((var["w"], 0, 1088, c[0] & ((1 << 1088) - 1)),),
            ((var["z"], 0, 256, 3),),
            ((var["a"], 0, 256, K_COLLIDE),),
            ((var["s"], 32, 64, c[0] & ((1 << 64) - 1)), (var["w"], 64, 32, c[1] & 0xFFFFFFFF)),
            ((var["p"], 0, 256, c[0] & m256), (var["s"], 0, 256, c[1] & m256), (var["w"], 1056, 32, c[2] & 0xFFFFFFFF)),
        ][j % 7])
    return out


def array_digests(cs):
    """sha256 of every array a candidate set carries (``batch``: absent arrays as None; the row and
    table derivations where present) and of ``host_batch()``'s."""
    import hashlib

    def dig(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return f"{a.dtype.str}{list(a.shape)}:{hashlib.sha256(a.tobytes()).hexdigest()}"
    out = {}
    for part, mb in (("batch", cs.batch), ("host_batch", cs.host_batch())):
        for name in ("var_words",) + TABLES:
            out[f"{part}.{name}"] = dig(getattr(mb, name))
    for part, obj, names in (("derivation", cs.derivation, ("base_words", "src", "block_start", "patch_ptr", "patches",
                                                            "floor_ptr", "floors")),
                             ("table_derivation", cs.table_derivation, ("add_ptr", "add_func", "add_var", "add_key_off",
                                                                        "key_words"))):
        for name in names:
            out[f"{part}.{name}"] = None if obj is None else dig(getattr(obj, name))
    return out


def k_idle_case(n_lru=N_LRU):
    """The three build modes over ONE block of 37 candidates that patches only ``z``: the batch
    has its four sites, and no block activates any of them."""
    key = ("idle", n_lru)
    if key not in _built:
        exprs = k_exprs()
        recs = k_models(n_lru)
        sets = []
        for kw in MODES:
            inc = IncrementalLowering()
            db, ok = inc.lower(exprs)
            assert ok.all()
            z = inc.syms.vars[("z", 256)]
            bases = np.arange(37) % n_lru if n_lru else np.full(37, -1, np.int64)
            blocks = [(((z, 0, 256, 3),), np.asarray(bases, np.int64))]
            sets.append(C.CandidateGenerator(keccak_sites=True, **kw)._serialize(inc.serialize(recs), blocks, inc.syms, recs, db))
        _built[key] = (sets, exprs, db, inc)
    return _built[key]


def k_case(n_lru, K, keccak_sites=True):
    """``[host-table set, device_rows set, device_tables set]`` of K candidates over ``n_lru`` base
    models (blocks of 37, the last one partial), plus ``(exprs, DagBatch, lowering)``; built once."""
    key = (n_lru, K, keccak_sites)
    if key not in _built:
        exprs = k_exprs()
        recs = k_models(n_lru)
        sets = []
        for kw in MODES:
            inc = IncrementalLowering()
            db, ok = inc.lower(exprs)
            assert ok.all()
            lru = inc.serialize(recs)
            sizes = [37] * (K // 37) + ([K % 37] if K % 37 else [])
            bases = [np.arange(n) % n_lru if n_lru else np.full(n, -1, np.int64) for n in sizes]
            blocks = [(p, np.asarray(b, np.int64)) for p, b in zip(k_patches(inc.syms, len(sizes)), bases)]
            gen = C.CandidateGenerator(keccak_sites=keccak_sites, **kw)
            sets.append(gen._serialize(lru, blocks, inc.syms, recs, db))
        _built[key] = (sets, exprs, db, inc)
    return _built[key]
