#!/usr/bin/env python3
"""The mapping-key fork stream (synth_evm.token_fork_workload) with MQ_CANDIDATE_KECCAK off and on:
   python tools/keccak_candidates.py [n_forks] [--models N] [--budget B] [--mode 0|1|2] [--generate K]

Every state goes through ``is_possible_batch`` with ``Args.quick_sat_candidates`` on and no solver
behind it (support.NoSolver: a state nothing answers counts as a solver call and is pruned), so
the fraction of get_model calls answered without the solver and the ms per state are the candidate
generator's alone.  ``--mode`` is MQ_DEVICE_CANDIDATES (default 2: rows and tables derived on the
device, what the flag is meant for).  ``--generate K`` (CPU only, no device) instead times
CandidateGenerator.generate filled to K candidates in the three build modes, flag off and on: the
host modes hash every (candidate, site) on the CPU."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mythril_amd import support as sp  # noqa: E402
from mythril_amd.synth_evm import token_fork_workload  # noqa: E402


def _opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def stream(n, n_models, budget, mode):
    from mythril_amd.evaluator import Evaluator
    ev = Evaluator(0)
    exprs, recs, _ = token_fork_workload(n, n_models, seed=41)
    out = {"stream": f"token_fork_workload({n}, {n_models}, seed 41): forks comparing a mapping key over "
                     f"KeccakFunctionManager axioms; no solver (unanswered states are solver calls)",
           "MQ_DEVICE_CANDIDATES": mode, "candidate_budget": budget}
    saved = (sp.model_cache, sp.args.quick_sat_candidates, sp.args.quick_sat_candidate_budget)
    env = {k: os.environ.get(k) for k in ("MQ_DEVICE_CANDIDATES", "MQ_CANDIDATE_KECCAK")}
    try:
        for flag in (False, True, False, True):      # (the first pair warms the runtime up)
            os.environ["MQ_DEVICE_CANDIDATES"] = str(mode)
            os.environ.pop("MQ_CANDIDATE_KECCAK", None)
            if flag:
                os.environ["MQ_CANDIDATE_KECCAK"] = "1"
            sp.reset_caches()
            sp.model_cache = sp.ModelCache(sp.VerdictEngine(ev))
            sp.set_solver_backend(sp.NoSolver())
            sp.args.quick_sat_candidates, sp.args.quick_sat_candidate_budget = True, budget
            for m in reversed(recs):
                sp.model_cache.put(m, 1)
            cs = [sp.Constraints(list(e.args)) for e in exprs]
            eng = sp.model_cache.engine
            t_stage0, l0, k0 = dict(eng.timing), eng.launches, ev.keccak_uploads
            t0 = time.perf_counter()
            alive = sp.is_possible_batch(cs)
            dt = time.perf_counter() - t0
            c = dict(sp.counters)
            avoided = c["get_model_calls"] - c["solver_calls"]
            out["keccak_on" if flag else "keccak_off"] = {
                **c, "states_alive": int(sum(alive)), "fraction_avoided": avoided / max(c["get_model_calls"], 1),
                "ms_per_state": dt * 1e3 / len(cs), "engine_launches": eng.launches - l0,
                "keccak_uploads": ev.keccak_uploads - k0,
                "engine_stage_ms_per_state": {k: (eng.timing[k] - t_stage0[k]) * 1e3 / len(cs) for k in eng.timing}}
    finally:
        sp.model_cache, sp.args.quick_sat_candidates, sp.args.quick_sat_candidate_budget = saved
        sp.set_solver_backend(None)
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ev.close()
    return out


def generate(K, n_models):
    from mythril_amd.candidates import CandidateGenerator
    from mythril_amd.lower import IncrementalLowering
    exprs, recs, _ = token_fork_workload(16, n_models, seed=41)
    out = {"generate": f"CandidateGenerator({K}, fill=True).generate over token_fork_workload(16, {n_models}), seconds"}
    for name, kw in (("host_tables", {}), ("device_rows", {"device_rows": True}),
                     ("device_tables", {"device_rows": True, "device_tables": True})):
        for flag in (False, True):
            inc = IncrementalLowering()
            db, ok = inc.lower(exprs)
            lru = inc.serialize(recs)
            t0 = time.perf_counter()
            cs = CandidateGenerator(K, seed=3, fill=True, keccak_sites=flag, **kw).generate(db, inc.syms, lru, recs)
            out[f"{name}_{'on' if flag else 'off'}"] = {"seconds": time.perf_counter() - t0, "models": cs.batch.n_models}
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 64
    if "--generate" in sys.argv:
        res = generate(_opt("--generate", 100_000), _opt("--models", 100))
    else:
        res = stream(n, _opt("--models", 100), _opt("--budget", 100_000), _opt("--mode", 2))
    print(json.dumps(res, indent=1))
