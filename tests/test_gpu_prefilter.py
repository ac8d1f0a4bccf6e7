"""The low-limb prefilter on the GPU (gen_qsa.py pf_frame: P frame mode 4, the narrow handlers;
alive_scan: P reading the bitmap): first hits are bit for bit the oracle's and those of the same
call under MQ_PREFILTER=0, the bitmap keeps every (tape, block) pair that holds a hit and clears
the rest but for low-limb collisions, and the counters say what ran.  MQ_PREFILTER=force lifts the
launch's model-count gate unless a test says otherwise."""
import numpy as np
import pytest

import cref
from mythril_amd import evaluator as evmod
from mythril_amd.models import ModelBatch
from mythril_amd.synth import c2_workload, random_words
from mythril_amd.tape import Tape, TapeBatch

pytestmark = pytest.mark.gpu

W = 256
M256 = (1 << W) - 1


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    for k in ("MQ_NO_BAIL", "MQ_G_BAIL", "MQ_BAIL_MIN_OPS", "MQ_P_WG", "MQ_PF_WG"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MQ_PREFILTER", "force")


def _launch(evaluator, monkeypatch, tb, mb, switch="force"):
    """(first hits, compiled tapes) of one arm; the caller frees."""
    if switch is None:
        monkeypatch.delenv("MQ_PREFILTER", raising=False)
    else:
        monkeypatch.setenv("MQ_PREFILTER", switch)
    assert evaluator.asm_ready, "the assembly interpreters did not come up: no prefilter would run"
    evaluator.upload_models(mb)
    ct = evaluator.compile(tb)
    assert ct.n_unsupported == 0
    return evaluator.first_hit(ct), ct


def _both(evaluator, monkeypatch, tb, mb, ref=None):
    """First hits with the prefilter forced, checked against the oracle and the MQ_PREFILTER=0
    arm; returns (first hits, the forced arm's compiled tapes, its bitmap view)."""
    ref = cref.first_hit(tb, mb)[0] if ref is None else ref
    off, ct0 = _launch(evaluator, monkeypatch, tb, mb, "0")
    try:
        assert ct0.prefilter_split() == (0, False) and ct0.prefilter_alive() is None
    finally:
        ct0.free()
    fh, ct = _launch(evaluator, monkeypatch, tb, mb, "force")
    assert (fh == ref).all(), np.flatnonzero(fh != ref)[:10]
    assert (off == ref).all(), np.flatnonzero(off != ref)[:10]
    n_pf, ran = ct.prefilter_split()
    assert ran == (n_pf > 0)
    return fh, ct, ct.prefilter_alive()


def _bit(alive, tape, model, base=0):
    bits, tapes, has = alive
    d = int(np.flatnonzero(tapes == tape)[0])
    assert has[d]
    return bool(bits[(model - base) // 64, d])


# ---------------------------------------------------------------- 1. ragged edges
_C2 = {}


def _c2(m):
    if m not in _C2:
        tb, mb, exp = c2_workload(70, m, seed=31, planted_frac=0.5)
        _C2[m] = (tb, mb, exp, cref.first_hit(tb, mb)[0])
    return _C2[m]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2113])
def test_c2_ragged_edges(evaluator, monkeypatch, m):
    tb, mb, exp, ref = _c2(m)
    assert (ref == exp).all()
    fh, ct, alive = _both(evaluator, monkeypatch, tb, mb, ref)
    try:
        assert ct.asm_split()[0] == tb.n_tapes and ct.prefilter_split() == (tb.n_tapes, True)
        bits, tapes, has = alive
        assert bits.shape == ((m + 63) // 64, tb.n_tapes) and has.all()
        for t in np.flatnonzero(exp >= 0):
            assert _bit(alive, t, int(exp[t])), (t, int(exp[t]))
        if m == 2113:
            # the reference data (seed 2, 1 500 tapes x 10^5 models): planted pairs and low-limb
            # collisions are 194 of 2.3 M pairs; here at most the planted ones and a few more
            frac = bits.sum() / bits.size
            print(f"alive pairs {int(bits.sum())} of {bits.size} ({100 * frac:.2f} %), planted {(exp >= 0).sum()}")
            assert frac <= 0.05
    finally:
        ct.free()


# ---------------------------------------------------------------- hand-built tapes
def _models(rng, m):
    return random_words(rng, 64, m)


def _value(words, v, m):
    return sum(int(x) << (32 * i) for i, x in enumerate(words[8 * v:8 * v + 8, m]))


def _tape_at(words, p, dear=True):
    """And(EQ(x0 * x1 + (x2 & x3), R), ULT over a product) holding at model p (and, at random
    models, with probability 2^-256)."""
    t = Tape()
    x = [t.var(i, W) for i in range(8)]
    v = [_value(words, i, p) for i in range(8)]
    r = (v[0] * v[1] + (v[2] & v[3])) & M256
    eq = t.eq(t.add(t.mul(x[0], x[1]), t.band(x[2], x[3])), t.const(r, W))
    a, b = (v[4] * v[5]) & M256, (v[6] * v[7]) & M256
    lt = t.ule(t.mul(x[4], x[5]), t.mul(x[6], x[7])) if a <= b else t.ule(t.mul(x[6], x[7]), t.mul(x[4], x[5]))
    return t.finish(t.and_(lt, eq) if dear else t.and_(eq, lt))


# ---------------------------------------------------------------- 2. placement
def test_placement_in_wave_and_tile(evaluator, monkeypatch):
    m = 2048 + 64 + 7
    words = _models(np.random.Generator(np.random.PCG64(41)), m)
    spots = [64 * l + k for l in range(8) for k in (0, 63)] + [m - 1, 2048, 512 + 63, 1536]
    tb = TapeBatch([_tape_at(words, p) for p in spots])
    mb = ModelBatch([W] * 8, words)
    fh, ct, alive = _both(evaluator, monkeypatch, tb, mb)
    try:
        assert list(fh) == spots
        bits = alive[0]
        for t, p in enumerate(spots):
            assert _bit(alive, t, p)
        assert bits.sum() == len(spots)       # nothing else survives (no collisions planted)
    finally:
        ct.free()


# ---------------------------------------------------------------- 3. low-limb collisions
def test_low_limb_collisions_stay_alive_and_are_rejected(evaluator, monkeypatch):
    m, p = 700, 601
    rng = np.random.Generator(np.random.PCG64(43))
    words = _models(rng, m)
    fakes = [3, 64, 130, 600]
    for f in fakes:
        words[0::8, f] = words[0::8, p]       # limb 0 of every variable; the limbs above stay random
    tb = TapeBatch([_tape_at(words, p), _tape_at(words, p, dear=False)])
    mb = ModelBatch([W] * 8, words)
    fh, ct, alive = _both(evaluator, monkeypatch, tb, mb)
    try:
        assert list(fh) == [p, p]
        for t in range(2):
            got = sorted(int(b) for b in np.flatnonzero(alive[0][:, int(np.flatnonzero(alive[1] == t)[0])]))
            assert got == sorted({f // 64 for f in fakes} | {p // 64})
    finally:
        ct.free()


# ---------------------------------------------------------------- 4. many satisfiers
@pytest.mark.parametrize("early_exit", [1, 0])
@pytest.mark.parametrize("k", [0, 1, 70, 600])
def test_every_model_from_k_on_satisfies(evaluator, monkeypatch, k, early_exit):
    m = 777
    rng = np.random.Generator(np.random.PCG64(47))
    words = _models(rng, m)
    c = int.from_bytes(rng.bytes(32), "little")
    for l in range(8):
        words[l, k:] = (c >> (32 * l)) & 0xFFFFFFFF
    t = Tape()
    tape = t.finish(t.and_(t.eq(t.bxor(t.var(0, W), t.const(5, W)), t.const(c ^ 5, W)), t.ule(t.var(1, W), t.const(M256, W))))
    tb, mb = TapeBatch([tape] * 3), ModelBatch([W] * 8, words)
    evaluator.set_option(evaluator.OPT_EARLY_EXIT, early_exit)
    try:
        fh, ct, alive = _both(evaluator, monkeypatch, tb, mb)
        try:
            assert list(fh) == [k] * 3
            assert alive[0][k // 64:].all() and not alive[0][:k // 64].any()
        finally:
            ct.free()
    finally:
        evaluator.set_option(evaluator.OPT_EARLY_EXIT, 1)


def test_constant_false_conjunct(evaluator, monkeypatch):
    """EQ of two constants that differ in limb 0 (PUSH_K32, EQK32): every block is cleared."""
    m = 130
    words = _models(np.random.Generator(np.random.PCG64(49)), m)
    t = Tape()
    tape = t.finish(t.and_(t.ule(t.var(1, W), t.const(M256, W)),
                           t.eq(t.add(t.const(3, W), t.const(4, W)), t.bxor(t.const(9, W), t.const(1, W)))))
    tb, mb = TapeBatch([tape]), ModelBatch([W] * 8, words)
    assert [int(w) & 0xFF for w in evmod.tape_prefilter_program(tb, 0)[0][0::2]] == [2, 17, 0]   # PUSH_K, EQK, END
    fh, ct, alive = _both(evaluator, monkeypatch, tb, mb)
    try:
        assert list(fh) == [-1] and ct.prefilter_split() == (1, True) and not alive[0].any()
    finally:
        ct.free()


# ---------------------------------------------------------------- 5. mixed batch
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_mixed_batch(evaluator, monkeypatch, n):
    """Eligible tapes, P tapes without a prefilter (no EQ conjunct), nine-variable tapes (G) and
    flat conjunctions in one batch; tape groups of one tape and groups that start off a
    32-descriptor boundary."""
    m = 2600
    rng = np.random.Generator(np.random.PCG64(53 + n))
    words = random_words(rng, 72, m)
    mb = ModelBatch([W] * 9, words)
    tapes, want_pf = [], 0
    for i in range(n):
        p = int(rng.integers(m))
        kind = i % 4
        if kind in (0, 1):
            tapes.append(_tape_at(words, p, dear=bool(kind)))
            want_pf += 1
        elif kind == 2:      # P, no EQ conjunct: every block is P's
            t = Tape()
            a, b = _value(words, 0, p), _value(words, 1, p)
            lo, hi = (0, 1) if a <= b else (1, 0)
            tapes.append(t.finish(t.and_(t.ule(t.var(lo, W), t.var(hi, W)),
                                         t.ule(t.mul(t.var(2, W), t.var(3, W)), t.const(M256, W)))))
        else:                # a ninth variable: G
            t = Tape()
            tapes.append(t.finish(t.and_(t.eq(t.add(t.var(8, W), t.var(0, W)),
                                              t.const((_value(words, 8, p) + _value(words, 0, p)) & M256, W)),
                                         t.ule(t.var(1, W), t.const(M256, W)))))
    t = Tape()   # a flat conjunction
    tapes.append(t.finish(t.and_(t.ult(t.var(0, W), t.const(1 << 255, W)), t.ult(t.var(1, W), t.const(1 << 255, W)))))
    tb = TapeBatch(tapes)
    ref = cref.first_hit(tb, mb)[0]
    # single-tape groups; then P groups of 3 and prefilter groups of ~33 descriptors at n = 65
    for wg in (None, ("1000000", "1000000"), ("256", "3")):
        if wg:
            monkeypatch.setenv("MQ_P_WG", wg[0])
            monkeypatch.setenv("MQ_PF_WG", wg[1])
        fh, ct, alive = _both(evaluator, monkeypatch, tb, mb, ref)
        try:
            assert ct.prefilter_split() == (want_pf, want_pf > 0)
            if want_pf:
                assert int(alive[2].sum()) == want_pf
                assert not alive[0][:, ~alive[2]].any()
        finally:
            ct.free()


# ---------------------------------------------------------------- 6. shard
def test_shard_hits_are_global(evaluator, monkeypatch):
    tb, mb, exp = c2_workload(60, 4000, seed=37, planted_frac=0.6)
    sh = mb.shard(1000, 3113)
    ref = cref.first_hit(tb, sh)[0]
    inside = (exp >= 1000) & (exp < 3113)
    assert (ref[inside] == exp[inside]).all() and (ref[~inside] == -1).all() and inside.sum() >= 10
    fh, ct, alive = _both(evaluator, monkeypatch, tb, sh, ref)
    try:
        for t in np.flatnonzero(inside):
            assert _bit(alive, t, int(exp[t]), base=1000)
        assert alive[0].shape[0] == (2113 + 63) // 64
    finally:
        ct.free()


# ---------------------------------------------------------------- 7. value-exactness per handler
def _flip_cases():
    ops = ["add", "sub", "mul", "band", "bor", "bxor"]
    out = [(op, form) for op in ops for form in ("var", "const", "computed", "const_left")]
    return out + [("neg", "var"), ("bnot", "var"), ("neg", "computed"), ("bnot", "computed")]


PY = {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "band": lambda a, b: a & b,
      "bor": lambda a, b: a | b, "bxor": lambda a, b: a ^ b, "neg": lambda a, b: -a, "bnot": lambda a, b: ~a}


@pytest.mark.parametrize("rconst", [False, True], ids=["EQ32", "EQK32"])
def test_narrow_handlers_value_exact(evaluator, monkeypatch, rconst):
    """And(<a dear ULE conjunct>, EQ(op(A, B), R)) over 130 models, one tape per op and operand
    form.  R (a variable, EQ32) or A (R a constant, EQK32) is planted per block: block 0 one bit
    of limb 0 off (the prefilter clears it), block 1 one bit of limb 5 off (alive, rejected by the
    full tape), block 2 correct (the hit, model 128)."""
    m = 130
    rng = np.random.Generator(np.random.PCG64(59))
    tapes, batches = [], []
    for op, form in _flip_cases():
        words = _models(rng, m)
        kc = int.from_bytes(rng.bytes(32), "little") | 1
        t = Tape()
        x = [t.var(i, W) for i in range(8)]

        def operand(vals):
            if form == "var":
                return vals[1]
            if form == "computed":
                return (vals[1] + vals[2]) & M256
            return kc
        bn = x[1] if form == "var" else t.add(x[1], x[2]) if form == "computed" else t.const(kc, W)
        if op in ("neg", "bnot"):
            an = x[0] if form == "var" else t.bxor(x[0], x[2])
            node = getattr(t, op)(an)
            val = lambda vals: PY[op](vals[0] if form == "var" else vals[0] ^ vals[2], 0) & M256   # noqa: E731
        elif form == "const_left":
            node = getattr(t, op)(bn, x[0])
            val = lambda vals: PY[op](kc, vals[0]) & M256   # noqa: E731
        else:
            node = getattr(t, op)(x[0], bn)
            val = lambda vals: PY[op](vals[0], operand(vals)) & M256   # noqa: E731
        if rconst:
            # one model's values everywhere in variables 0-2, then variable 0 disturbed per block
            # (an odd multiplier / XOR / ADD / NOT / NEG keep a flipped bit of limb 0 in limb 0;
            # AND / OR with a random constant may not: those ops are planted through R only)
            if op in ("band", "bor", "mul", "sub") or form == "computed":
                continue
            for v in range(3):
                words[8 * v:8 * v + 8, :] = words[8 * v:8 * v + 8, 129:130]
            words[0, :64] ^= 1 << 7
            words[5, 64:128] ^= 1 << 9
            r = t.const(val([_value(words, v, 129) for v in range(8)]), W)
        else:
            for mm in range(m):
                rv = val([_value(words, v, mm) for v in range(8)])
                rv ^= (1 << 7) if mm < 64 else (1 << (160 + 9)) if mm < 128 else 0
                for l in range(8):
                    words[56 + l, mm] = (rv >> (32 * l)) & 0xFFFFFFFF
            r = x[7]
        dear = t.ule(t.mul(x[4], x[5]), t.const(M256, W))
        tapes.append(t.finish(t.and_(dear, t.eq(node, r))))
        batches.append(words)
    for tape, words in zip(tapes, batches):
        tb, mb = TapeBatch([tape]), ModelBatch([W] * 8, words)
        fh, ct, alive = _both(evaluator, monkeypatch, tb, mb)
        try:
            assert list(fh) == [128]
            assert ct.prefilter_split() == (1, True)
            assert [bool(b) for b in alive[0][:, 0]] == [False, True, True]
        finally:
            ct.free()


# ---------------------------------------------------------------- 8. counters
def test_counters_early_exit_off(evaluator, monkeypatch):
    tb, mb, exp = c2_workload(40, 4096, seed=23, planted_frac=0.0)
    assert (exp == -1).all()
    stats = {}
    evaluator.upload_models(mb)
    evaluator.set_option(evaluator.OPT_EARLY_EXIT, 0)
    try:
        for arm, switch in (("on", None), ("off", "0")):
            fh, ct = _launch(evaluator, monkeypatch, tb, mb, switch)
            try:
                assert (fh == -1).all()
                assert ct.prefilter_split() == ((40, True) if arm == "on" else (0, False))
                if arm == "on":
                    assert not ct.prefilter_alive()[0].any()   # no collision in this draw: P ran nothing
                _, stats[arm] = evaluator.first_hit(ct, with_stats=True)
            finally:
                ct.free()
    finally:
        evaluator.set_option(evaluator.OPT_EARLY_EXIT, 1)
    monkeypatch.delenv("MQ_PREFILTER", raising=False)
    pf_ops = sum(evmod.tape_prefilter_program(tb, t)[1] for t in range(tb.n_tapes))
    a, b = stats["on"], stats["off"]
    print(f"pairs {a.pairs_evaluated} / {b.pairs_evaluated}, node_evals {a.node_evals} / {b.node_evals}, "
          f"alg_ops {a.alg_ops} / {b.alg_ops} (narrow x 4096 = {4096 * pf_ops})")
    assert a.pairs_evaluated == b.pairs_evaluated == 4096 * tb.n_tapes
    assert a.node_evals == b.node_evals == 4096.0 * float(tb.sizes().sum())
    assert a.alg_ops == 4096 * pf_ops


# ---------------------------------------------------------------- 9. gate
def test_gate_below_4096_models(evaluator, monkeypatch):
    tb, mb, exp = c2_workload(40, 700, seed=29, planted_frac=0.5)
    res = {}
    for arm, switch in (("default", None), ("off", "0")):
        fh, ct = _launch(evaluator, monkeypatch, tb, mb, switch)
        try:
            _, st = evaluator.first_hit(ct, with_stats=True)
            res[arm] = (fh, ct.handler_histogram(0), st.pairs_evaluated, st.node_evals, st.alg_ops)
            assert ct.prefilter_split()[1] is False and ct.prefilter_alive() is None
            if arm == "default":
                assert ct.prefilter_split()[0] == tb.n_tapes
        finally:
            ct.free()
    assert (res["default"][0] == exp).all() and (res["off"][0] == exp).all()
    assert res["default"][1:] == res["off"][1:]
    # verdict mode never runs it, whatever the switch says
    fh, ct = _launch(evaluator, monkeypatch, tb, mb, "force")
    try:
        v, fh2 = evaluator.verdicts(ct)
        assert ct.prefilter_split() == (tb.n_tapes, False)
        assert (v == cref.verdicts(tb, mb)).all() and (fh2 == exp).all()
    finally:
        ct.free()
