#!/usr/bin/env python3
"""Exposures/s of a visit written to _raw files on the host path (reads copied out of the pinned buffer, formatted into
big-endian FITS words by the writer threads) and with device_fits (k_fits_words forms the words, every file is written
straight from the slot's pinned mirror), on the metric's configuration -- the two paths taking turns in one process,
medians of five passes -- and the parts: host seconds per file outside os.writev, k_fits_words by HIP events against its
algorithmic bytes, the payload's copy against the reads'.  GPU only.  No test asserts any of it.

    python scripts/bench_device_fits.py [config=cfg4] [exposures per pass=16] [out=profiles/device_fits.json]
"""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
from wayne_amd import _lib, fitsio, visit as wv  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 16
out_json = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "device_fits.json")
PASSES = 5
COPY_CEILING = 6.29e12      # bytes/s: the measured float4 copy rate of an MI355X's HBM

v = helpers.make_visit(name, n_exposures=n)
S, R = v.detector.full_size(v.SUBARRAY), v.NSAMP - 1
dirs = {"tmp": tempfile.gettempdir()}
if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK):
    dirs["memory"] = "/dev/shm"
result = {"config": name, "S": S, "reads": R + 1, "exposures_per_pass": n, "passes": PASSES,
          "directories": dirs, "library": _lib.library_info()[0].replace(ROOT + os.sep, ""), "files_per_s": {}, "parts": {}}


def one_pass(dtype, device_fits, where):
    out = tempfile.mkdtemp(prefix="wayne_fits_", dir=where)
    try:
        r = wv.VisitRunner(v, 0, out_dir=out, out_dtype=dtype, device_fits=device_fits)
        t = time.perf_counter()
        r.run(range(n))
        dt = time.perf_counter() - t
        assert len(os.listdir(out)) == n
        return n / dt
    finally:
        shutil.rmtree(out, ignore_errors=True)


for dtype in (np.float32, np.uint16):
    key = np.dtype(dtype).name
    result["files_per_s"][key] = {}
    wv.VisitRunner(v, 0, out_dtype=dtype).run([0, 1])          # context, calibration, first-use allocations
    for where_name, where in dirs.items():
        for threads in (1, 2, 4, 16):
            os.environ["WAYNE_FITS_THREADS"] = str(threads)
            one_pass(dtype, True, where)                        # the slots' pinned mirrors of this type
            rates = {"host": [], "device_fits": []}
            for _ in range(PASSES):                             # taking turns
                rates["host"].append(one_pass(dtype, False, where))
                rates["device_fits"].append(one_pass(dtype, True, where))
            row = {k: {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))} for k, x in rates.items()}
            result["files_per_s"][key]["%s, %d writer threads" % (where_name, threads)] = row
            print("%s reads, %s, %2d writer threads: host %.1f /s, device_fits %.1f /s" % (
                key, where_name, threads, row["host"]["median"], row["device_fits"]["median"]), flush=True)

    # the parts, on one thread: a file's host time outside os.writev, the kernel, the two copies
    eng = wv.VisitRunner(v, 0, out_dtype=dtype).engine()
    ctx = eng.ctx
    gen = helpers.product_generator(v, 0)
    desc = gen.build_descriptor(eng, out_dtype=dtype, device_fits=True, **v.frame_kwargs(0))
    ctx.upload(0, desc)
    ctx.run_checked(0)
    plane_bytes, stride, bitpix = ctx.fits_layout_of(0)
    t_reads, t_payload = [], []
    for _ in range(PASSES):
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.fetch_async(0)
        reads = ctx.wait(0)
        t1 = time.perf_counter()
        ctx.fetch_fits_async(0)
        payload = ctx.wait_fits(0)
        t2 = time.perf_counter()
        t_reads.append(t1 - t0)
        t_payload.append(t2 - t1)
    in_writev = [0.0]
    real = fitsio._write_all

    def timed(fd, pieces):
        t = time.perf_counter()
        real(fd, pieces)
        in_writev[0] += time.perf_counter() - t

    fitsio._write_all = timed
    where = dirs.get("memory", dirs["tmp"])
    out = tempfile.mkdtemp(prefix="wayne_fits_", dir=where)
    outside = {"host": [], "device_fits": []}
    inside = {"host": [], "device_fits": []}
    try:
        for k in range(PASSES + 1):
            for path in ("host", "device_fits"):
                g = helpers.product_generator(v, 0)
                g.build_descriptor(None, out_dtype=dtype, **v.frame_kwargs(0))
                in_writev[0] = 0.0
                probe = "probe_%d_%s.fits" % (k, path)          # (a new file each time: no old pages to free)
                t = time.perf_counter()
                if path == "host":
                    exp = g._fill_exposure(reads.copy())        # (the copy out of the pinned buffer is the path's)
                else:
                    exp = g._fill_stored(payload, (plane_bytes, stride, bitpix))
                exp.generate_fits(out, probe)
                if k:                                           # (the first pass renders the cached header blocks)
                    outside[path].append(time.perf_counter() - t - in_writev[0])
                    inside[path].append(in_writev[0])
                os.remove(os.path.join(out, probe))
    finally:
        fitsio._write_all = real
        shutil.rmtree(out, ignore_errors=True)
    ctx.profile_enable(True)
    ctx.profile_select(["k_fits_words"])
    ctx.profile_reset()
    for _ in range(20):
        ctx.run(0)
    prof = ctx.fits_profile()
    ctx.profile_select(None)
    ctx.profile_enable(False)
    ms = prof["ms"] / max(prof["launches"], 1)
    B_in = np.dtype(dtype).itemsize
    algo = (R + 1) * S * S * B_in + (R + 1) * stride         # samples read once, every byte of the payload written once
    result["parts"][key] = {
        "host_s_per_file_outside_writev": {k: float(np.median(x)) for k, x in outside.items()},
        "host_s_per_file_in_writev": {k: float(np.median(x)) for k, x in inside.items()},
        "k_fits_words": {"launches": prof["launches"], "ms_per_launch": ms, "algorithmic_bytes": int(algo),
                         "bytes_per_s": algo / (ms * 1e-3) if ms > 0 else None,
                         "fraction_of_copy_ceiling": algo / (ms * 1e-3) / COPY_CEILING if ms > 0 else None},
        "copy_s": {"reads": float(np.median(t_reads)), "payload": float(np.median(t_payload)),
                   "reads_bytes": int(reads.nbytes), "payload_bytes": int(payload.nbytes)},
    }
    print(key, json.dumps(result["parts"][key]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
with open(out_json, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out_json)
