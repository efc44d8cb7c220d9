#!/usr/bin/env python3
"""Cost of contaminating field stars (wayne_exposure_set_sources): microseconds per exposure on a synthetic visit with
0 contaminants, 1 faint (flux_ratio 0.01) and 1 bright (1.0) -- GPU only; not part of bench.py.

    python scripts/bench_contaminants.py [cfg4] [exposures per case] [repeats] [case: none | faint_0.01 | bright_1.0]

Each case: the same descriptor uploaded into alternating slots and run, n exposures between two synchronisations
(the throughput loop of bench.py's plain run, without the host's descriptor building); the best of `repeats`.
Run one case under `rocprofv3 --kernel-trace --stats` to see its kernels: the difference of two cases is the marginal cost.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import _lib, calibration, detector, engine, grism, synthetic  # noqa: E402
from wayne_amd.exposure_generator import ExposureGenerator  # noqa: E402
from wayne_amd.sources import Contaminant, scale_to_ratio  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    cal = calibration.CalibrationSet.synthetic(11)
    det = detector.WFC3_IR()
    gr = grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=1)
    eng = engine.get_engine(0, gr, det, cal, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    ctx = eng.ctx
    eg = ExposureGenerator(det, gr, v.NSAMP, v.SAMPSEQ, v.SUBARRAY, calibration=cal, seed=v.seed)
    desc = eg.build_descriptor(eng, rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, **v.frame_kwargs(0))
    wl, flux = desc._keep[0], desc._keep[1]

    def companion(ratio):
        # a cooler star on the target's grid, 14 px right of and 40 px below the target
        from wayne_amd import tools
        f = scale_to_ratio(gr, wl, tools.blackbody_lambda(wl, 4800.0), wl, flux, ratio)
        return [Contaminant(14.0, -40.0, wl, f, 1, flux_ratio=ratio)]

    cases = [("none", []), ("faint_0.01", companion(0.01)), ("bright_1.0", companion(1.0))]
    if len(sys.argv) > 4:                              # one case only (a kernel trace of it)
        cases = [c for c in cases if c[0] == sys.argv[4]]
    out = {"config": name, "exposures": n, "repeats": repeats, "us_per_exposure": {}}
    for label, srcs in cases:
        best = None
        for rep in range(repeats + 1):                 # (the first pass warms up: allocations, code objects)
            ctx.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                slot = i % 4
                ctx.upload(slot, desc)
                if srcs:
                    ctx.set_sources(slot, srcs)
                ctx.run(slot)
            ctx.synchronize()
            dt = (time.perf_counter() - t0) / n * 1e6
            if rep > 0 or repeats == 0:                  # (repeats 0: the one pass, e.g. under a kernel trace)
                best = dt if best is None else min(best, dt)
        out["us_per_exposure"][label] = round(best, 2)
        print("%-12s %8.2f us / exposure" % (label, best), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
