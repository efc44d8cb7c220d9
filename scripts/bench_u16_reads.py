#!/usr/bin/env python3
"""float32 reads against 16-bit unsigned reads (WAYNE_F_OUT_U16, out_dtype=np.uint16), side by side in one process:
device-complete exposures/s and the ramp kernel's own time (HIP events), reads delivered to pinned host memory, end to
end, and FITS files on disk with the per-exposure parts of a file -- GPU only; not part of bench.py.

    python scripts/bench_u16_reads.py [cfg4] [exposures per pass] [repeats] [--out FILE]

Every figure is the median of `repeats` passes with their spread (max - min), the two read types taking turns pass by
pass so that a drift of the box falls on both.  The legs are bench.py's: `device_complete` runs resident descriptors in
four slots between two synchronisations, `delivered` is VisitRunner.run_resident (reads copied to pinned host memory),
`end_to_end` VisitRunner.run with device light curves, `files` VisitRunner.run with an output directory (the FITS
writer pool).  Registers of the two production kernels come from the library's gfx950 code object.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import bench_traps  # noqa: E402
from wayne_amd import calibration, detector, engine, fitsio, grism, synthetic, visit as wvisit  # noqa: E402

TYPES = (("float32", np.float32), ("uint16", np.uint16))
SYMS = {"_ZN5wayne6k_rampIfLb1ELi1ELb0ELb1EEEvNS_8RampArgsE": "k_ramp<float, true, 1, false, true>",
        "_ZN5wayne6k_rampItLb1ELi1ELb0ELb1EEEvNS_8RampArgsE": "k_ramp<unsigned short, true, 1, false, true>",
        "_ZN5wayne6k_rampIfLb1ELi1ELb0ELb0EEEvNS_8RampArgsE": "k_ramp<float, true, 1, false, false>",
        "_ZN5wayne6k_rampItLb1ELi1ELb0ELb0EEEvNS_8RampArgsE": "k_ramp<unsigned short, true, 1, false, false>"}


def stat(vals, digits=2):
    return {"median": round(float(np.median(vals)), digits), "spread": round(float(max(vals) - min(vals)), digits),
            "repetitions": [round(float(x), digits) for x in vals]}


def main():
    argv = list(sys.argv[1:])
    out_path = None
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    name = argv[0] if len(argv) > 0 else "cfg4"
    n = int(argv[1]) if len(argv) > 1 else 200
    repeats = int(argv[2]) if len(argv) > 2 else 5
    n_host = max(8, n // 4)                                # exposures per pass of the legs that cross PCIe
    n_files = 24
    # (read from the code object before this process touches the GPU: no child process is started after that)
    resources = {SYMS[k]: r for k, r in bench_traps.kernel_resources(set(SYMS)).items()} if shutil.which("objcopy") else None

    cal = calibration.CalibrationSet.synthetic(11)
    det, gr = detector.WFC3_IR(), grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=max(n_files + 2, 32))
    runners = {label: wvisit.VisitRunner(v, 0, out_dtype=dt) for label, dt in TYPES}
    runners_lc = {label: wvisit.VisitRunner(v, 0, out_dtype=dt, device_lc=True) for label, dt in TYPES}
    eng = runners["float32"].engine()
    ctx = eng.ctx
    S, N, R = v.detector.full_size(v.SUBARRAY), v.detector.light_sensitive_size(v.SUBARRAY), v.NSAMP - 1
    descs = {label: [runners[label].descriptor(i, eng) for i in range(4)] for label, _ in TYPES}

    def make_resident(label):
        for slot in range(4):
            ctx.upload(slot, descs[label][slot])

    out = {"config": name, "S": S, "NSAMP": v.NSAMP, "exposures_per_pass": n, "exposures_per_host_pass": n_host,
           "files_per_pass": n_files, "repeats": repeats, "writer_threads": min(16, os.cpu_count() or 4)}
    rate = {leg: {label: [] for label, _ in TYPES} for leg in ("device_complete", "delivered", "end_to_end")}
    ramp_us = {label: [] for label, _ in TYPES}
    variant = {}
    for rep in range(repeats + 1):                         # (the first pass warms up: allocations, pinned buffers, code objects)
        for label, _ in TYPES:
            make_resident(label)
            for j in range(8):
                ctx.run(j % 4)
            ctx.synchronize()
            t0 = time.perf_counter()
            for j in range(n):
                ctx.run(j % 4)
            ctx.synchronize()
            dc = n / (time.perf_counter() - t0)
            variant[label] = ctx.ramp_variant(0)
            # the ramp kernel alone: HIP events around each launch
            ctx.profile_enable(True)
            ctx.profile_select(["k_ramp"])
            ctx.profile_reset()
            for j in range(min(n, 48)):
                ctx.run(j % 4)
            ctx.synchronize()
            p = ctx.profile_get()["k_ramp"]
            ctx.profile_enable(False)
            ctx.profile_select(None)
            us = p["ms"] / max(p["launches"], 1) * 1e3
            runners[label].run_resident(8)
            ctx.synchronize()
            t0 = time.perf_counter()
            runners[label].run_resident(n_host)
            dl = n_host / (time.perf_counter() - t0)
            idx = [j % v.n_exposures for j in range(n_host)]
            runners_lc[label].run(idx[:8])
            t0 = time.perf_counter()
            runners_lc[label].run(idx)
            ee = n_host / (time.perf_counter() - t0)
            if rep > 0:
                rate["device_complete"][label].append(dc)
                rate["delivered"][label].append(dl)
                rate["end_to_end"][label].append(ee)
                ramp_us[label].append(us)
    for leg in rate:
        out[leg] = {label: dict(stat(rate[leg][label], 1), unit="exposures/s") for label, _ in TYPES}
    out["ramp_kernel_us"] = {label: stat(ramp_us[label]) for label, _ in TYPES}
    out["variant"] = variant
    use_box, _, segs = ctx.debug_boxes(0)
    out["ramp_bytes"] = {}
    for label, dt in TYPES:
        b = bench.ramp_bytes(N, S, R, np.dtype(dt).itemsize, int(segs.sum()) if use_box else None)
        us = out["ramp_kernel_us"][label]["median"]
        out["ramp_bytes"][label] = {"B_out": np.dtype(dt).itemsize, "bytes_per_launch": int(b),
                                    "GB_per_s": round(b / (us * 1e-6) / 1e9, 1),
                                    "frac_of_8_TB_s": round(b / (us * 1e-6) / 1e9 / bench.HBM_PEAK_GBS, 4)}
    for leg in ("delivered", "end_to_end"):
        for label, dt in TYPES:
            mb = (R + 1) * S * S * np.dtype(dt).itemsize / 1e6
            out[leg][label]["MB_per_exposure"] = round(mb, 2)
            out[leg][label]["PCIe_GB_per_s"] = round(out[leg][label]["median"] * mb / 1e3, 2)

    # files on disk: the visit loop with the writer pool, and the parts of one file on one thread
    files = {label: [] for label, _ in TYPES}
    size = {}
    tmp = tempfile.mkdtemp(prefix="wayne_u16_")
    try:
        for rep in range(repeats + 1):
            for label, dt in TYPES:
                d = os.path.join(tmp, label)
                r = wvisit.VisitRunner(v, 0, out_dir=d, out_dtype=dt)
                t0 = time.perf_counter()
                r.run(range(2, n_files + 2))
                dt_s = time.perf_counter() - t0
                size[label] = os.path.getsize(os.path.join(d, "0003_raw.fits"))
                shutil.rmtree(d, ignore_errors=True)
                if rep > 0:
                    files[label].append(n_files / dt_s)
        out["files"] = {label: dict(stat(files[label], 1), unit="exposures/s", file_MB=round(size[label] / 1e6, 2))
                        for label, _ in TYPES}
        parts = {}
        for label, dt in TYPES:
            reads = runners[label].run([0], keep=True)[0]
            t_fmt, t_wr = [], []
            for rep in range(5):
                t0 = time.perf_counter()
                if dt == np.uint16:
                    cube = np.empty(reads.shape, dtype=">i2")
                    for i in range(reads.shape[0]):
                        fitsio.u16_to_stored(reads[i], out=cube[i])
                else:
                    cube = np.empty(reads.shape, dtype=">f8")
                    for i in range(reads.shape[0]):
                        cube[i] = reads[i]
                t1 = time.perf_counter()
                fitsio.write_pieces(os.path.join(tmp, "probe.fits"), [memoryview(cube.reshape(-1)).cast("B")])
                t2 = time.perf_counter()
                t_fmt.append((t1 - t0) * 1e3)
                t_wr.append((t2 - t1) * 1e3)
            parts[label] = {"device_to_host_ms": round(1e3 / out["delivered"][label]["median"], 2),
                            "format_ms_one_thread": stat(t_fmt), "write_ms_one_thread": stat(t_wr),
                            "format": "flip top bit + byte swap -> >i2" if dt == np.uint16 else "float32 -> big-endian float64",
                            "payload_MB": round(cube.nbytes / 1e6, 2)}
        out["file_parts_per_exposure"] = parts
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if resources is not None:
        out["resources"] = resources
    engine.close_all()                                     # (the context goes before the interpreter's teardown)
    text = json.dumps(out, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
