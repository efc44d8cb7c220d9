#!/usr/bin/env python3
"""Cost of limb darkening per wavelength bin (wayne_exposure_set_limb_darkening, k_lightcurve_ld) on the metric's
configuration (cfg4: K = 128 sub-samples, W = 4494 bins) -- GPU only; not part of bench.py.

    python scripts/bench_ld_table.py [cfg4] [exposures per pass] [passes] > profiles/ld_table.json

In one process, for four exposures -- mid-transit, mid-ingress (the planet's centre on the limb at mid-exposure), first
contact (z = 1 + rp at mid-exposure) and out of transit -- with ONE coefficient set (k_lightcurve) and with a table
(k_lightcurve_ld):
  * the light-curve launch by HIP events (the "k_lightcurve" profile slot counts both kernels), median of `passes`
    passes of `exposures` runs each;
  * how many of the K sub-samples took the per-wavelength path (a regime change inside [p_lo, p_hi]: the kernels'
    own decision, restated on the host);
  * device-complete exposures/s: the same descriptor uploaded into four slots in rotation and run, n exposures between
    two synchronisations (the throughput loop of bench.py's plain run, light curves on the device), median of `passes`.
The table is the one of tests/test_ld_table.py.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import _lib, calibration, detector, engine, grism, lightcurve, synthetic, tools  # noqa: E402
from wayne_amd.exposure_generator import ExposureGenerator  # noqa: E402


def table_at(wl):
    s = np.clip((np.asarray(wl, dtype=float) - 1.1) / 0.6, 0.0, 1.0)
    return np.stack([0.55 + 0.25 * s, -0.2 - 0.55 * s, 0.5 + 0.4 * s, -0.25 - 0.13 * s], axis=1)


def direct_sub_samples(z, rp):
    """Sub-samples the kernels integrate wavelength by wavelength (k_lightcurve.h: `direct`)."""
    p_lo, p_hi = float(rp.min()), float(rp.max())
    guard = 1e-9 + 0.08 * (p_hi - p_lo)        # lc_guard

    def inside(v):
        return (v > p_lo - guard) & (v < p_hi + guard)
    no_transit = ~(z < 1 + p_lo) & ~(z < 1 + p_hi)
    return int((~no_transit & (inside(np.abs(1 - z)) | inside(z) | inside(z - 1))).sum())


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    passes = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    cal = calibration.CalibrationSet.synthetic(11)
    det = detector.WFC3_IR()
    gr = grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=1)
    eng = engine.get_engine(0, gr, det, cal, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    ctx = eng.ctx
    i0, i1 = tools.crop_spectrum_ind(gr.wl_limits[0], gr.wl_limits[1], v.wl)
    # the exposure whose middle sub-sample has the planet's centre on the limb
    mid = 0.5 * float(v.read_times[-1]) / 86400.0
    t = np.linspace(-0.09, 0.0, 9001)
    o = v.ORBIT
    z, _ = lightcurve.planet_orbit(o["period"], o["sma_over_rs"], o["eccentricity"], o["inclination"], o["periastron"],
                                   0.0, t + mid)
    rp0 = float(np.sqrt(v.depth0[i0:i1].mean()))
    starts = {"mid_transit": -mid, "mid_ingress": float(t[np.argmin(np.abs(z - 1.0))]),
              "first_contact": float(t[np.argmin(np.abs(z - 1.0 - rp0))]), "out_of_transit": -0.2}
    table = lightcurve.LimbDarkening(v.wl, table_at(v.wl))
    out = {"config": name, "sub_samples": int(v.K), "wavelength_bins": int(i1 - i0), "exposures_per_pass": n,
           "passes": passes, "library": os.path.relpath(_lib.library_info()[0], ROOT), "exposures": {}}
    for label, start in starts.items():
        v.exp_start_days = np.array([start])
        rec = {}
        for case in ("one_set", "table"):
            v.ld_table = table if case == "table" else None
            dd = v.device_depths(0)
            eg = ExposureGenerator(det, gr, v.NSAMP, v.SAMPSEQ, v.SUBARRAY, calibration=cal, seed=v.seed)
            desc = eg.build_descriptor(eng, rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32,
                                       **v.frame_kwargs(0, planet_signal=dd))
            assert (desc._ld_table is not None) == (case == "table")
            rec["per_wavelength_sub_samples"] = direct_sub_samples(dd.z_tr, np.sqrt(dd.planet_spectrum[i0:i1]))
            rec["z_range"] = [float(dd.z_tr.min()), float(dd.z_tr.max())]
            # the light-curve launch alone
            ctx.profile_enable(True)
            ctx.profile_select(["k_lightcurve"])
            us = []
            for rep in range(passes + 1):                  # (the first pass warms up)
                ctx.profile_reset()
                for i in range(n):
                    ctx.upload(0, desc)
                    ctx.run(0)
                ctx.synchronize()
                p = ctx.profile_get()["k_lightcurve"]
                assert p["launches"] == n
                if rep:
                    us.append(p["ms"] / p["launches"] * 1e3)
            ctx.profile_enable(False)
            ctx.profile_select(None)
            # device-complete exposures per second
            rate = []
            for rep in range(passes + 1):
                ctx.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    ctx.upload(i % 4, desc)
                    ctx.run(i % 4)
                ctx.synchronize()
                if rep:
                    rate.append(n / (time.perf_counter() - t0))
            rec[case] = {"lightcurve_launch_us": round(float(np.median(us)), 2),
                         "lightcurve_launch_us_passes": [round(x, 2) for x in us],
                         "device_complete_exposures_per_s": round(float(np.median(rate)), 1),
                         "device_complete_passes": [round(x, 1) for x in rate]}
            print("%-15s %-8s light-curve launch %7.2f us   %7.1f exposures/s   (%d of %d sub-samples per wavelength)" % (
                label, case, rec[case]["lightcurve_launch_us"], rec[case]["device_complete_exposures_per_s"],
                rec["per_wavelength_sub_samples"], v.K), file=sys.stderr, flush=True)
        out["exposures"][label] = rec
    engine.close_all()                                 # (the context goes before the interpreter's teardown)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
