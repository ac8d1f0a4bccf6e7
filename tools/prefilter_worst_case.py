#!/usr/bin/env python3
"""What the low-limb prefilter costs when it cannot help (DESIGN §3, next to its gate).

C2-shaped tapes, all planted on one model p; every model agrees with p in limb 0 of every variable
and is random above it.  The narrow test then passes for every (tape, model) pair: nothing is
filtered, every block stays alive, and P runs what it would have run anyway -- after a prefilter
launch that decided nothing.  Prints one JSON line with the step time (first_hit over compiled
tapes, wall clock, early exit as given) with the prefilter on and with MQ_PREFILTER=0.

    python tools/prefilter_worst_case.py [--tapes 1000] [--models 100000] [--steps 20] [--no-early-exit]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mythril_amd.evaluator import Evaluator  # noqa: E402
from mythril_amd.models import ModelBatch  # noqa: E402
from mythril_amd.synth import c2_tape, random_words  # noqa: E402
from mythril_amd.tape import TapeBatch  # noqa: E402


def workload(n_tapes, n_models, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    words = random_words(rng, 64, n_models)
    p = n_models - 1
    words[0::8, :] = words[0::8, p:p + 1]          # limb 0 of every variable as at model p
    mb = ModelBatch([256] * 8, words)
    vals = [mb.var_value(v, p) for v in range(8)]
    return TapeBatch([c2_tape(rng, vals) for _ in range(n_tapes)]), mb, p


def step_ms(ev, tb, mb, switch, steps, expect):
    if switch is None:
        os.environ.pop("MQ_PREFILTER", None)
    else:
        os.environ["MQ_PREFILTER"] = switch
    ev.upload_models(mb)
    ct = ev.compile(tb)
    try:
        fh = ev.first_hit(ct)
        assert (fh == expect).all(), "first hits differ from the planted model"
        n_pf, ran = ct.prefilter_split()
        alive = ct.prefilter_alive()
        t0 = time.perf_counter()
        for _ in range(steps):
            ev.first_hit(ct)
        ms = (time.perf_counter() - t0) * 1e3 / steps
        frac = float(alive[0][:, alive[2]].mean()) if alive is not None else None
        return {"ms_per_step": ms, "prefiltered_tapes": n_pf, "prefilter_ran": ran, "alive_fraction": frac}
    finally:
        ct.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tapes", type=int, default=1000)
    ap.add_argument("--models", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--no-early-exit", action="store_true")
    a = ap.parse_args()
    tb, mb, p = workload(a.tapes, a.models, a.seed)
    ev = Evaluator(0)
    try:
        if a.no_early_exit:
            ev.set_option(ev.OPT_EARLY_EXIT, 0)
        # every model whose upper limbs differ fails the full tape: the first hit is p itself
        expect = np.full(a.tapes, p, np.int32)
        res = {"tapes": a.tapes, "models": a.models, "early_exit": not a.no_early_exit,
               "on": step_ms(ev, tb, mb, None, a.steps, expect), "off": step_ms(ev, tb, mb, "0", a.steps, expect)}
    finally:
        ev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
