#!/usr/bin/env python3
"""The cost of the noise-free expected image (k_expect) beside an exposure, on the metric's configuration: the kernel's
HIP-event time per rendering in both modes (every source's launch and the clearing of the plane), its fp64 FMA rate
against the chip's vector peak, the exposure's own kernels in the same runs, and the copy of the planes to the host.
GPU only.  No test asserts any of it.

The FMA count is the law's own: for every sub-sample, bin and component that holds electrons, the pixels of its 8 sigma
square -- what a gather that culls exactly at 8 sigma has to add; the kernel adds whole 32-bin batches per tile, so it
executes more.

    python scripts/bench_expected.py [config=cfg4] [runs=20] [out=profiles/expected.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
from wayne_amd import _lib, visit as wv  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_json = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "expected.json")
FP64_FMA_PEAK = 78.6e12 / 2      # fp64 vector FMAs per second of an MI355X: half its FP32 vector rate (157.3 TFLOPS)

v = helpers.make_visit(name)
S, R = v.detector.full_size(v.SUBARRAY), v.NSAMP - 1
eng = wv.VisitRunner(v, 0).engine()
ctx = eng.ctx
result = {"config": name, "S": S, "read_intervals": R, "sub_samples": v.K, "runs": runs,
          "library": _lib.library_info()[0].replace(ROOT + os.sep, ""), "fp64_fma_peak_per_s": FP64_FMA_PEAK, "modes": {}}

for mode in ("counts", "mean"):
    gen = helpers.product_generator(v, 0)
    desc = gen.build_descriptor(eng, expected=mode, **v.frame_kwargs(0))
    ctx.upload(0, desc)
    ctx.run_checked(0)
    counts, x, y, _ = ctx.debug_fetch(0)
    wl = desc._keep[0]
    sig = np.stack([v.grism.psf_sigmah_poly(wl), v.grism.psf_sigmal_poly(wl)]).astype(np.float32).astype(np.float64)
    nw = np.clip(np.trunc(counts * v.grism.psf_ratio_poly(wl)[None, :]), 0, counts)
    fmas = 0.0
    for c, n in enumerate((nw, counts - nw)):
        side = 2.0 * np.floor(8.0 * sig[c]) + 2.0
        fmas += float(((n > 0) * (side * side)[None, :]).sum())
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(runs):
        ctx.run(0)
    ctx.synchronize()
    prof, kernels = ctx.expected_profile(), ctx.profile_get()
    ctx.profile_enable(False)
    ms = prof["ms"] / max(prof["launches"], 1)
    t_copy = []
    for _ in range(5):
        t = time.perf_counter()
        planes = ctx.expected(0)
        t_copy.append(time.perf_counter() - t)
    row = {"renderings": prof["launches"], "ms_per_rendering": ms, "law_fmas": fmas,
           "law_fmas_per_s": fmas / (ms * 1e-3) if ms > 0 else None,
           "fraction_of_fp64_vector_peak": fmas / (ms * 1e-3) / FP64_FMA_PEAK if ms > 0 else None,
           "exposure_kernels_ms": {k: kernels[k]["ms"] / max(kernels[k]["launches"], 1) for k in kernels
                                   if k != "electrons" and kernels[k]["launches"]},
           "plane_bytes": int(planes.nbytes), "copy_s_to_pageable_memory": float(np.median(t_copy)),
           "electrons_in_E": float(planes.sum())}
    result["modes"][mode] = row
    print(mode, json.dumps(row), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
with open(out_json, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out_json)
