"""Shared by the candidate-derivation tests: a literal applier of a Derivation, and a small
hand-built candidate set (three blocks of 64, 65 and 1 candidates over 3 or 0 base models, Bool /
8 / 33 / 256 / 512-bit variables, one function whose entry at a constant key is a patched derived
variable)."""
from types import SimpleNamespace

import numpy as np

from mythril_amd import candidates as C
from mythril_amd.models import FuncSpec, ModelBatch
from mythril_amd.tape import limbs


def apply_derivation(d, rows):
    """What mq_models_upload_derived leaves resident (before masking), literally."""
    gen = np.zeros((rows, d.n_derived), np.uint32)
    for k in range(d.n_derived):
        if d.src[k] >= 0:
            gen[:, k] = d.base_words[:, d.src[k]]
    for j in range(d.n_blocks):
        sl = slice(int(d.block_start[j]), int(d.block_start[j + 1]))
        ps = d.patches[int(d.patch_ptr[j]):int(d.patch_ptr[j + 1])]
        assert len(set(ps[:, 0].tolist())) == len(ps)        # at most one patch per (block, row)
        for row, keep, bits in ps:
            gen[row, sl] = (gen[row, sl] & keep) | bits
        for row0, nl, mn in d.floors[int(d.floor_ptr[j]):int(d.floor_ptr[j + 1])]:
            small = ~gen[row0 + 1:row0 + nl, sl].any(axis=0)
            x = gen[row0, sl]
            gen[row0, sl] = np.where(small & (x < mn), mn, x)
    return np.concatenate([d.base_words.reshape(rows, d.n_base), gen], axis=1)


def mask_rows(words, widths):
    """Rows as the device keeps them: bits above a variable's width cleared (Bool: bit 0)."""
    out = words.copy()
    r = 0
    for w in widths:
        w = int(w)
        r += limbs(w)
        top = 1 if w == 0 else ((1 << (w % 32)) - 1 if w % 32 else 0xFFFFFFFF)
        out[r - 1] &= np.uint32(top)
    return out


T_WIDTHS = [0, 8, 33, 256, 512]
T_FUNCS = [FuncSpec(1, 8, (256,))]
T_KEY = 5                     # variable 1 is the function's value at this key
T_SIZES = (64, 65, 1)         # K = 130: the last wave is partial and straddles the block boundary at 129
T_BIG = int.from_bytes(bytes(range(1, 33)), "little")
T_PATCHES = [
    ((1, 0, 8, 0xA7), (3, 28, 10, 0x2AB), (0, 0, 1, 1)),
    ((4, 500, 12, 0xABC), (2, 30, 3, 0b101), (1, 2, 3, 0b110), (1, -1, 0, 0x40)),
    ((3, 0, 256, T_BIG), (0, 0, 1, 0), (1, 0, 8, 0x11), (1, 4, 4, 0x3)),
]


def table_models(n):
    rng = np.random.default_rng(11)
    out = []
    for m in range(n):
        vs = {v: int.from_bytes(rng.bytes(64), "little") & ((1 << max(w, 1)) - 1) for v, w in enumerate(T_WIDTHS)}
        vs[1] = [0x03, 0x9C, 0x41][m % 3]   # (floor 0x40 with bits 2..4 = 110: applied / not / not)
        vs[0] = m & 1
        out.append({"vars": vs, "funcs": {0: ({T_KEY: vs[1], 9 + m: 0x77}, m + 1)}})
    return out


def table_case(n_base, device_rows):
    """The hand-built set through CandidateGenerator._serialize (host-built function tables)."""
    models = table_models(n_base)
    lru = ModelBatch.from_python(T_WIDTHS, models, T_FUNCS)
    syms = SimpleNamespace(var_widths=T_WIDTHS, derived={1: ("cd", (T_KEY,))}, func_names=["cd"])
    if n_base:
        bases = [(np.arange(n) + j) % n_base for j, n in enumerate(T_SIZES)]
    else:
        bases = [np.full(n, -1, np.int64) for n in T_SIZES]
    blocks = [(p, np.asarray(b, np.int64)) for p, b in zip(T_PATCHES, bases)]
    cs = C.CandidateGenerator(device_rows=device_rows)._serialize(lru, blocks, syms, models)
    return cs, models
