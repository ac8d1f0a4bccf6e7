"""Keccak-consistent generated candidates on the CPU (mythril_amd/candidates.py KeccakSites,
include/mq.h mq_keccak_derivation): which applications are sites and why the others are not; the
image lies in the manager's interval; on forks over a mapping key no generated candidate satisfies
its query without the feature and every query has one with it; the tables read like the
materialized model; the collision rule; the three build modes agree; the flag off changes nothing;
the host-side check refuses one malformed variant per rule (no device)."""
import ctypes

import numpy as np
import pytest

import cref
import term_eval
from mythril_amd import candidates as C
from mythril_amd import evaluator
from mythril_amd import smt as S
from mythril_amd._abi import as_derivation, as_keccak_derivation, as_model_batch, as_table_derivation, keccak_derivation_arrays
from mythril_amd.function_managers import KeccakFunctionManager
from mythril_amd.lower import IncrementalLowering
from mythril_amd.synth_evm import _Tx, fork_workload, token_fork_workload
from mythril_amd.tape import limbs

from keccak_candidates_util import K_COLLIDE, MODES, TABLES, array_digests, k_case, k_idle_case

MQ_OK, MQ_ERR_ARG = 0, -1


def _sites(expr):
    inc = IncrementalLowering()
    db, ok = inc.lower([expr])
    assert ok.all()
    off = np.concatenate([[0], np.cumsum([limbs(w) for w in inc.syms.var_widths])])
    return C.find_keccak_sites(db, inc.syms, off)


# ---------------------------------------------------------------- 1. site discovery
def test_sites_found_on_the_token_forks():
    exprs, recs, kfm = token_fork_workload(2, 2, seed=1)
    sites, skipped = _sites(exprs[0])
    assert sorted(s.n_bits for s in sites) == [256, 512] and skipped == {}
    s512 = [s for s in sites if s.n_bits == 512][0]
    # Concat(sender, 1): the low eight words constant, the high eight the sender's rows
    assert s512.words[0] == (-1, 1) and all(w == (-1, 0) for w in s512.words[1:8])
    assert [r for r, _ in s512.words[8:]] == list(range(s512.words[8][0], s512.words[8][0] + 8))
    assert [(lo, hi) for _, lo, hi in s512.inverses] == [(0, 512), (0, 256), (256, 512)]
    assert (s512.base, s512.b) == C.image_params(*kfm.interval(512)) and s512.b == 117
    s256 = [s for s in sites if s.n_bits == 256][0]
    assert [(lo, hi) for _, lo, hi in s256.inverses] == [(0, 256)] and len(s256.words) == 8


def _skip_case(name):
    kfm = KeccakFunctionManager()
    x = S.BitVecSym("x", 256)
    if name == "misaligned":          # the variable's bits start 8 bits into the input
        kfm.create_keccak(S.Concat(S.Extract(247, 0, x), S.BitVecVal(1, 8)))
        return kfm.create_conditions(), 0
    if name == "nested":              # keccak of a keccak: the inner one is a site
        kfm.create_keccak(kfm.create_keccak(x))
        return kfm.create_conditions(), 1
    f, inv = kfm.get_function(256)
    lo, hi = kfm.interval(256)
    if name == "no_inverse":
        g = S.Function("keccak256_288", [288], 256)   # (no keccak256_288-1 anywhere)
        gx = g(S.Concat(x, S.BitVecVal(7, 32)))
        return S.And(S.ULE(S.BitVecVal(lo, 256), gx), S.ULT(gx, S.BitVecVal(hi, 256))), 0
    if name == "no_interval":
        return S.And(inv(f(x)) == x, S.URem(f(x), S.BitVecVal(64, 256)) == 0), 0
    if name == "floor":               # a calldata word: bytes read under i < calldatasize
        kfm.create_keccak(_Tx(1).word(4))
        return kfm.create_conditions(), 0
    if name == "inverse_derived":     # the inverse is also looked up at a constant key
        kfm.create_keccak(x)
        return S.And(kfm.create_conditions(), inv(S.BitVecVal(5, 256)) == 9), 0
    if name == "too_many_derived":    # nine constant-key lookups of f: one more than the collision rule takes
        kfm.create_keccak(x)
        return S.And(kfm.create_conditions(), *[f(S.BitVecVal(k, 256)) == k for k in range(9)]), 0
    if name == "too_many_sites":      # 65 applications: the first 64 are sites
        for i in range(65):
            kfm.create_keccak(S.BitVecSym(f"x{i}", 256))
        return kfm.create_conditions(), 64
    raise AssertionError(name)


@pytest.mark.parametrize("name", ["misaligned", "nested", "no_inverse", "no_interval", "floor", "inverse_derived",
                                  "too_many_derived", "too_many_sites"])
def test_skipped_applications_are_counted_by_reason(name):
    expr, n_sites = _skip_case(name)
    sites, skipped = _sites(expr)
    assert len(sites) == n_sites and skipped == {name: 1}
    assert [s.node for s in sites] == sorted(s.node for s in sites)       # site order: ascending UF node


# ---------------------------------------------------------------- 2. the image
def test_image_lies_in_the_interval_and_is_injective_in_practice():
    kfm = KeccakFunctionManager()
    rng = np.random.default_rng(3)
    for rnd in range(2):
        for n in (256, 512, 1088):
            lo, hi = kfm.interval(n)
            base, b = C.image_params(lo, hi)
            assert base % 64 == 0 and lo <= base and b <= 192 and base + 64 * 2 ** b <= hi < base + 64 * 2 ** (b + 1) + 64
            xs = [int.from_bytes(rng.bytes(n // 8), "big") for _ in range(10_000 if (rnd, n) == (0, 512) else 50)] + [0]
            vs = C.keccak_images(xs, n, base, b)
            assert all(lo <= v < hi and v % 64 == 0 for v in vs)
            assert len(set(vs)) == len(set(xs))
        kfm.reset()
    # the definition, spelled out on one input
    d = int.from_bytes(evaluator.keccak256_host([(5).to_bytes(32, "big")])[0], "big")
    assert C.keccak_images([5], 256, 128, 10) == [128 + ((d % 1024) << 6)]
    assert C.image_params(1, 64) is None and C.image_params(1, 128) == (64, 0) and C.image_params(0, 1 << 256)[1] == 192


# ---------------------------------------------------------------- 3. the premise and the feature
def _token(flag, **kw):
    exprs, recs, _ = token_fork_workload(8, 6, seed=41)
    inc = IncrementalLowering()
    db, ok = inc.lower(exprs)
    assert ok.all()
    cs = C.CandidateGenerator(3000, seed=2, keccak_sites=flag, **kw).generate(db, inc.syms, inc.serialize(recs), recs)
    return exprs, db, cs


def test_without_the_sites_no_generated_candidate_satisfies_its_query():
    exprs, db, cs = _token(False)
    assert cs.n_generated >= 8 * 6 and cs.keccak_sites is None and cs.keccak_skips == {}
    fh, _ = cref.first_hit(db.to_tapes(), cs.host_batch())
    assert (fh == -1).all()
    for k in range(cs.n_lru, cs.batch.n_models):
        m = cs.materialize(k)
        assert not any(term_eval.is_true(e, m) for e in exprs)


def test_with_the_sites_every_query_has_a_generated_candidate():
    exprs, db, cs = _token(True)
    assert len(cs.keccak_sites.sites) == 2 and cs.keccak_skips == {}
    fh, _ = cref.first_hit(db.to_tapes(), cs.host_batch())
    hits = 0
    for q, h in enumerate(fh):
        assert h >= cs.n_lru, (q, h)
        assert term_eval.is_true(exprs[q], cs.materialize(int(h)))
        hits += 1
    assert hits == len(exprs) == 8


# ---------------------------------------------------------------- 4. tables read like the materialized model
def test_tables_read_like_the_materialized_model():
    (cs, _, _), exprs, db, inc = k_case(37, 259)
    tb = db.to_tapes()
    hb = cs.host_batch()
    whole = cref.verdicts(tb, hb)
    assert whole[:, cs.n_lru:].any(axis=1).all()        # every query is true on some candidate
    rng = np.random.default_rng(9)
    edges = [0, 36, 37, 4 * 37, 5 * 37 - 1, 6 * 37, 258]      # block boundaries, the collision block, the last one
    rest = [k for k in rng.permutation(259).tolist() if k not in edges]
    sample = sorted(edges + rest[:60 - len(edges)])
    assert len(set(sample)) == 60
    for k in sample:
        i = cs.n_lru + k
        shard = cref.verdicts(tb, hb.shard(i, i + 1))[:, 0]
        model = cref.verdicts(tb, inc.serialize([cs.materialize(i)]))[:, 0]
        assert (shard == model).all() and (shard == whole[:, i]).all(), k


# ---------------------------------------------------------------- 5. the collision rule
def test_collision_with_a_constant_key_keeps_table_and_column_equal():
    (cs, _, _), exprs, db, inc = k_case(37, 259)
    tb = db.to_tapes().subset([4])                      # a == 77 and f(77) == f(a)
    hb = cs.host_batch()
    site = [s for s in cs.keccak_sites.sites if s.collisions]
    assert site and all(key == K_COLLIDE for s in site for key, _, _ in s.collisions)
    for k in range(4 * 37, 5 * 37):                     # block 4 patches a := 77
        i = cs.n_lru + k
        shard = int(cref.verdicts(tb, hb.shard(i, i + 1))[0, 0])
        m = cs.materialize(i)
        assert shard == int(term_eval.is_true(exprs[4], m)) == 1, k
        assert shard == int(cref.verdicts(tb, inc.serialize([m]))[0, 0])


# ---------------------------------------------------------------- 6. three build modes
@pytest.mark.parametrize("n_lru,K", [(37, 259), (0, 130)])
def test_host_batch_is_identical_across_the_build_modes(n_lru, K):
    sets, _, _, _ = k_case(n_lru, K)
    ref = sets[0].host_batch()
    assert sets[0].batch.var_words is not None and sets[1].derivation is not None and sets[2].table_derivation is not None
    assert sets[2].batch.entry_ptr is None
    for cs in sets[1:]:
        hb = cs.host_batch()
        for name in ("var_words",) + TABLES:
            assert (np.asarray(getattr(hb, name)) == np.asarray(getattr(ref, name))).all(), name
    # the sites add entries: more than the same set without them
    plain = k_case(n_lru, K, False)[0][0].host_batch()
    assert (ref.entry_ptr[:, -1] >= plain.entry_ptr[:, -1]).all() and ref.entry_ptr[:, -1].sum() > plain.entry_ptr[:, -1].sum()
    assert (ref.var_words == plain.var_words).all()


@pytest.mark.parametrize("n_lru", [37, 0])
def test_sites_present_but_no_block_active_builds_in_every_mode(n_lru):
    """The keccak axioms ride on every path, and most forks compare something else than the mapping
    key: a batch with sites whose blocks activate none of them appends nothing, in all three modes."""
    sets, _, _, _ = k_idle_case(n_lru)
    for cs in sets:
        assert len(cs.keccak_sites.sites) == 4 and not cs.keccak_sites.active.any()
        assert not cs.keccak_sites.site_counts(len(cs.batch.funcs)).any()
    ref = sets[0].host_batch()
    for cs in sets[1:]:
        hb = cs.host_batch()
        for name in ("var_words",) + TABLES:
            assert (np.asarray(getattr(hb, name)) == np.asarray(getattr(ref, name))).all(), name
    # every candidate's tables are its base model's
    counts = np.diff(ref.entry_ptr, axis=1)
    want = counts[:, np.arange(37) % n_lru] if n_lru else np.zeros((len(ref.funcs), 37), np.int64)
    assert (counts[:, n_lru:] == want).all()
    assert sets[0].materialize(n_lru + 5).functions == (sets[0].lru_models[5].functions if n_lru else {})


# ---------------------------------------------------------------- 7. flag off
@pytest.mark.parametrize("mode,kw", list(zip(("host_tables", "device_rows", "device_tables"), MODES)))
def test_flag_off_every_array_is_the_parent_code_paths(mode, kw):
    """tests/golden/keccak_flag_off.json holds the sha256 of every array (the batch's, host_batch()'s,
    the row and table derivations') that the code BEFORE this feature generated on the token
    workload, per build mode: with the flag off, and with the argument left out, this code
    generates the same.  (On batches without keccak applications the older candidate tests, which
    this feature leaves untouched, carry the same guarantee.)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keccak_flag_off.json")) as f:
        want = json.load(f)["sha256"][mode]
    exprs, recs, _ = token_fork_workload(6, 5, seed=41)
    for opts in ({}, {"keccak_sites": False}):
        inc = IncrementalLowering()
        db, ok = inc.lower(exprs)
        cs = C.CandidateGenerator(3000, seed=2, **kw, **opts).generate(db, inc.syms, inc.serialize(recs), recs)
        assert cs.keccak_sites is None
        got = array_digests(cs)
        assert got.keys() == want.keys()
        for name in want:
            assert got[name] == want[name], name
    # the flag on does change these tables (the recorded digests are not trivially matched) ...
    inc = IncrementalLowering()
    db, ok = inc.lower(exprs)
    on = array_digests(C.CandidateGenerator(3000, seed=2, keccak_sites=True, **kw).generate(db, inc.syms, inc.serialize(recs), recs))
    assert on["host_batch.entry_words"] != want["host_batch.entry_words"] and on["host_batch.var_words"] == want["host_batch.var_words"]
    # ... and on a batch without keccak applications it finds no site and changes no array
    exprs, recs, _ = fork_workload(8, 12, seed=3)
    got = []
    for opts in ({}, {"keccak_sites": True}):
        inc = IncrementalLowering()
        db, ok = inc.lower(exprs)
        got.append(C.CandidateGenerator(3000, seed=2, **kw, **opts).generate(db, inc.syms, inc.serialize(recs), recs))
    assert got[1].keccak_sites.sites == [] and not got[1].keccak_sites.active.any()
    assert array_digests(got[1]) == array_digests(got[0])


# ---------------------------------------------------------------- 8. mq_keccak_derivation_check
def _check(cs, arrays):
    lib = evaluator.load_library()
    s, keep = as_model_batch(cs.batch)
    d, keep_d = as_derivation(cs.derivation)
    t, keep_t = as_table_derivation(cs.table_derivation)
    k, keep_k = as_keccak_derivation(cs.keccak_sites, arrays)
    rc = lib.mq_keccak_derivation_check(ctypes.byref(s), ctypes.byref(d), ctypes.byref(k))
    # the upload runs the same checks before it looks at the context or the device
    assert lib.mq_models_upload_derived_keccak(None, ctypes.byref(s), ctypes.byref(d), ctypes.byref(t), ctypes.byref(k)) == MQ_ERR_ARG
    return rc


def test_struct_sizes_match_the_header(tmp_path):
    import os
    import subprocess
    from mythril_amd._abi import MqKeccakCollision, MqKeccakDerivation, MqKeccakInverse, MqKeccakSite, MqKeccakWord
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mq.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mq_keccak_word),'
                   ' sizeof(mq_keccak_inverse), sizeof(mq_keccak_collision), sizeof(mq_keccak_site),'
                   ' offsetof(mq_keccak_site, base), offsetof(mq_keccak_site, map_off), sizeof(mq_keccak_derivation),'
                   ' offsetof(mq_keccak_derivation, active)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(MqKeccakWord), ctypes.sizeof(MqKeccakInverse), ctypes.sizeof(MqKeccakCollision),
                   ctypes.sizeof(MqKeccakSite), MqKeccakSite.base.offset, MqKeccakSite.map_off.offset,
                   ctypes.sizeof(MqKeccakDerivation), MqKeccakDerivation.active.offset]
    assert got[:4] == [8, 8, 16, 72]
    sites = keccak_derivation_arrays(k_case(37, 259)[0][2].keccak_sites)[0]
    assert sites.dtype.itemsize == 72


def test_well_formed_keccak_derivation_passes_the_check():
    for n_lru, K in ((37, 259), (0, 130)):
        cs = k_case(n_lru, K)[0][2]
        assert _check(cs, None) == MQ_OK


@pytest.mark.parametrize("name", ["func_past_n_funcs", "func_width_differs", "inverse_is_the_function", "inverse_key_not_256",
                                  "inverse_slice_past_the_input", "map_row_past_rows", "map_past_words", "b_past_192",
                                  "base_not_a_multiple_of_64", "image_past_2_256", "mask_names_a_missing_site",
                                  "collision_var_past_n_vars", "collision_key_past_pool", "too_many_sites"])
def test_malformed_keccak_derivation_is_an_argument_error(name):
    cs = k_case(37, 259)[0][2]
    sites, words, invs, colls, keys, active = (a.copy() for a in keccak_derivation_arrays(cs.keccak_sites))
    funcs = cs.batch.funcs
    i512 = [i for i in range(len(sites)) if sites["n_words"][i] == 16][0]
    i256 = [i for i in range(len(sites)) if sites["n_words"][i] == 8][0]
    if name == "func_past_n_funcs":
        sites["func"][0] = len(funcs)
    elif name == "func_width_differs":
        sites["func"][i512] = sites["func"][i256]            # a 256-bit function for a 16-word input
    elif name == "inverse_is_the_function":
        invs["func"][sites["inv_off"][0]] = sites["func"][0]
    elif name == "inverse_key_not_256":
        invs["func"][sites["inv_off"][i256]] = sites["func"][i512]   # keccak256_512: a 512-bit key
    elif name == "inverse_slice_past_the_input":
        invs["lo_word"][sites["inv_off"][i256]] = 1
    elif name == "map_row_past_rows":
        words["row"][sites["map_off"][i256]] = int(sum(limbs(int(w)) for w in cs.batch.var_widths))
    elif name == "map_past_words":
        sites["map_off"][i512] = len(words) - 15
    elif name == "b_past_192":
        sites["b"][0] = 193
    elif name == "base_not_a_multiple_of_64":
        sites["base"][0][0] |= 32
    elif name == "image_past_2_256":
        sites["base"][0][:] = 0xFFFFFFFF                     # 2^256 - 64: any b carries out of limb 7
        sites["base"][0][0] = 0xFFFFFFC0
    elif name == "mask_names_a_missing_site":
        active[3] |= np.uint64(1) << np.uint64(len(sites))
    elif name == "collision_var_past_n_vars":
        colls["var"][0] = len(cs.batch.var_widths)
    elif name == "collision_key_past_pool":
        colls["key_off"][0] = len(keys) - 7
    elif name == "too_many_sites":
        sites = np.concatenate([sites] * 17)[:65]
    assert len(colls) >= 1
    assert _check(cs, (sites, words, invs, colls, keys, active)) == MQ_ERR_ARG
