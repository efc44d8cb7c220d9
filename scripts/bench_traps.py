#!/usr/bin/env python3
"""Cost of per-pixel charge trapping (wayne_exposure_set_traps, k_ramp_trap): microseconds per exposure on a synthetic
visit with traps off and on, the ramp kernel's own time (HIP events), and the registers / occupancy of the kernels from
the library's gfx950 code object -- GPU only; not part of bench.py.

    python scripts/bench_traps.py [cfg4] [exposures per case] [repeats] [case: off | on]

Each case: the same descriptor uploaded into alternating slots and run, n exposures between two synchronisations
(the throughput loop of bench.py's plain run, without the host's descriptor building); the best of `repeats`.  The
trapped case uses the default model with the start tables of the 6th exposure of a two-orbit scanned visit.
Run one case under `rocprofv3 --kernel-trace --stats` to see its kernels.
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wayne_amd import _lib, build, calibration, detector, engine, grism, synthetic, traps  # noqa: E402
from wayne_amd.exposure_generator import ExposureGenerator  # noqa: E402


RAMP_THREADS = 1024          # threads of a ramp workgroup (k_ramp.h kRampThreads): 16 waves, 4 on each of a CU's SIMDs
LDS_PER_CU = 160 * 1024      # gfx950


def occupancy(vgpr, lds_bytes, threads=RAMP_THREADS):
    """(workgroups per CU, waves per SIMD) of a kernel launched with `threads`-thread workgroups.  Registers allow
    min(8, 512 // alloc) waves per SIMD (alloc: the VGPR count rounded up to 8), but a workgroup's waves are resident
    together -- threads / 256 of them on each SIMD -- so the waves per SIMD are whole workgroups' worth: k T / 256."""
    alloc = ((vgpr + 7) // 8) * 8
    per_simd = -(-threads // 64) // 4
    by_regs = min(8, 512 // alloc) // per_simd
    by_lds = LDS_PER_CU // lds_bytes if lds_bytes else by_regs
    k = min(by_regs, by_lds)
    return k, k * per_simd


def kernel_resources(names):
    """{kernel name: VGPRs, VGPR spills, LDS bytes, workgroups per CU and waves per SIMD at RAMP_THREADS threads per
    workgroup} from the library's code object metadata."""
    llvm = "/opt/rocm/llvm/bin"
    out = {}
    try:
        with tempfile.TemporaryDirectory() as d:
            fat = os.path.join(d, "fatbin")
            subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=" + fat, build.LIB], check=True, capture_output=True)
            targets = subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--list", "--type=o", "--input=" + fat],
                                     check=True, capture_output=True, text=True).stdout.split()
            t = [x for x in targets if "gfx950" in x][0]
            co = os.path.join(d, "co")
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + t,
                            "--input=" + fat, "--output=" + co], check=True, capture_output=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
    except (OSError, subprocess.CalledProcessError, IndexError):
        return out
    for blk in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(\S+)", blk)
        if not m or m.group(1) not in names:
            continue
        v = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        wgs, waves = occupancy(v, lds)
        out[m.group(1)] = {"vgpr": v, "vgpr_spill": spill, "lds_bytes": lds, "workgroups_per_cu": wgs,
                           "waves_per_simd": waves}
    return out


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    syms = {"_ZN5wayne6k_rampIfLb1ELi1ELb0ELb1EEEvNS_8RampArgsE": "k_ramp<float, true, 1, false, true>",
            "_ZN5wayne11k_ramp_trapIfLb1ELi1ELb0ELb1EEEvNS_8RampArgsENS_8TrapArgsE": "k_ramp_trap<float, true, 1, false, true>",
            "_ZN5wayne6k_rampIfLb1ELi1ELb0ELb0EEEvNS_8RampArgsE": "k_ramp<float, true, 1, false, false>",
            "_ZN5wayne11k_ramp_trapIfLb1ELi1ELb0ELb0EEEvNS_8RampArgsENS_8TrapArgsE": "k_ramp_trap<float, true, 1, false, false>"}
    # (read from the code object before this process touches the GPU: no child process is started after that)
    resources = None
    if shutil.which("objcopy"):
        resources = {syms[k]: r for k, r in kernel_resources(set(syms)).items()}
    cal = calibration.CalibrationSet.synthetic(11)
    det = detector.WFC3_IR()
    gr = grism.G141(cal)
    v = synthetic.Visit(name, det, gr, cal, n_exposures=1)
    eng = engine.get_engine(0, gr, det, cal, v.NSAMP, v.SAMPSEQ, v.SUBARRAY)
    ctx = eng.ctx
    eg = ExposureGenerator(det, gr, v.NSAMP, v.SAMPSEQ, v.SUBARRAY, calibration=cal, seed=v.seed)
    desc = eg.build_descriptor(eng, rng_mode=_lib.RNG_SPLIT, out_dtype=np.float32, **v.frame_kwargs(0))
    model = traps.ChargeTraps()
    exptime = float(v.read_times[-1])
    t = [o * 96.0 / 1440.0 + k * (exptime + 60.0) / 86400.0 for o in range(2) for k in range(4)]
    plan = {"exp_start_times": np.array(t), "orbit_start_index": [0, 4]}
    et = traps.ExposureTraps(model, model.start_tables(plan, exptime, staring=False)[5])

    cases = [("off", None), ("on", et)]
    if len(sys.argv) > 4:                              # one case only (a kernel trace of it)
        cases = [c for c in cases if c[0] == sys.argv[4]]
    out = {"config": name, "exposures": n, "repeats": repeats, "us_per_exposure": {}, "ramp_kernel_us": {}, "variant": {}}
    for label, tr in cases:
        best = None
        for rep in range(repeats + 1):                 # (the first pass warms up: allocations, code objects)
            ctx.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                slot = i % 4
                ctx.upload(slot, desc)
                if tr is not None:
                    ctx.set_traps(slot, tr)
                ctx.run(slot)
            ctx.synchronize()
            dt = (time.perf_counter() - t0) / n * 1e6
            if rep > 0 or repeats == 0:                  # (repeats 0: the one pass, e.g. under a kernel trace)
                best = dt if best is None else min(best, dt)
        out["us_per_exposure"][label] = round(best, 2)
        out["variant"][label] = ctx.ramp_variant(0)
        # the ramp kernel alone: HIP events around each launch, one exposure at a time
        ctx.profile_enable(True)
        ctx.profile_select(["k_ramp"])
        ctx.profile_reset()
        for i in range(min(n, 100)):
            ctx.upload(0, desc)
            if tr is not None:
                ctx.set_traps(0, tr)
            ctx.run(0)
        p = ctx.profile_get()["k_ramp"]
        ctx.profile_enable(False)
        ctx.profile_select(None)
        out["ramp_kernel_us"][label] = round(p["ms"] / max(p["launches"], 1) * 1e3, 2)
        print("%-4s %8.2f us / exposure   ramp kernel %7.2f us   %s" % (
            label, best, out["ramp_kernel_us"][label], out["variant"][label]), flush=True)
    if resources is not None:
        out["resources"] = resources
    engine.close_all()                                 # (the context goes before the interpreter's teardown)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
