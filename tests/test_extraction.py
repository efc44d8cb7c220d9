"""CPU: the host side of the device-side spectral extraction (wayne_amd/extraction.py, wayne_exposure_set_extraction).

The ABI (header, binding, struct layout), the default plan against the observer's geometry of tests/visit_science.py,
the channel weights, the law restated in numpy (tests/extraction_law.py) against the observer's extraction, and the
HIP-free argument check of wayne_amd/csrc/host_plan.h compiled with g++.  The device: tests/test_extraction_gpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import extraction_law as law
import helpers
import visit_science as vs
from wayne_amd import _lib, extraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wayne_exposure_set_extraction", "wayne_exposure_fetch_spectra_async", "wayne_exposure_wait_spectra",
       "wayne_exposure_download_spectra"]


def test_the_header_declares_the_extraction_calls_and_the_binding_mirrors_them(tmp_path):
    text = open(os.path.join(ROOT, "include", "wayne_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(wayne_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS, name
    assert declared == set(_lib.SYMBOLS)
    assert "#define WAYNE_ABI_VERSION 7" in text and _lib.ABI_VERSION == 7
    for name, bit in (("LINEARISE", 0), ("DARK", 1), ("GAIN", 2), ("SKY", 3), ("LAST_READ", 4)):
        assert re.search(r"#define WAYNE_X_%s \(1u << %d\)" % (name, bit), text) and getattr(_lib, "X_" + name) == 1 << bit
    assert _lib.X_ALL == 31 and extraction.ALL == 31
    # the ctypes mirror of wayne_extract_desc against the compiler's layout (the method of tests/test_abi.py)
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "wayne_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(wayne_extract_desc));']
    for f in _lib.ExtractDesc._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(wayne_extract_desc, %s));' % (f[0], f[0]))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True)
    out = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(_lib.ExtractDesc)
    for f in _lib.ExtractDesc._fields_:
        assert int(out[f[0]]) == getattr(_lib.ExtractDesc, f[0]).offset, f[0]
    d = extraction.Extraction([(5, 9), (6, 10), (5, 10)], bg_cols=(2, 4), steps=extraction.ALL & ~extraction.SKY).desc()
    assert (list(d.row_lo[:4]), list(d.row_hi[:4])) == ([5, 6, 5, 0], [9, 10, 10, 0])
    assert (d.bg_col_lo, d.bg_col_hi, d.steps) == (2, 4, 23)


@pytest.fixture(scope="module")
def sv():
    return vs.ScienceVisit("cfg3", 8)


def planned(sv_like, v, i, sub_scale, S):
    return extraction.row_windows(v.grism, v.wl, v.x_refs[i], v.y_refs[i], v.scan_speed, v.read_times, sub_scale, S)


def oracle_windows(sv, i):
    t = np.concatenate([[0.0], sv.read_times])
    return np.array([sv.row_window(i, t[r], t[r + 1]) for r in range(sv.R)] + [sv.row_window(i, 0.0, t[-1])])


def test_the_default_plan_is_the_observers_row_windows(sv):
    # the oracle evaluates the trace once per visit (at the nominal star position), the planner once per exposure (at the
    # exposure's own): a window's end may differ by one row, and by none without the sub-pixel phases
    assert extraction.ROW_MARGIN == vs.ROW_MARGIN and extraction.BG_COLS == vs.BG_COLS
    for i in range(sv.v.n_exposures):
        got, want = planned(sv, sv.v, i, sv.sub_scale, sv.S), oracle_windows(sv, i)
        assert got.shape == want.shape == (sv.R + 1, 2)
        assert np.abs(got - want).max() <= 1, (i, got, want)
        assert (got[:, 0] >= 5).all() and (got[:, 1] <= sv.S - 5).all() and (got[:, 0] < got[:, 1]).all()
    flat = vs.ScienceVisit("cfg3", 8)
    flat.v.x_refs = np.full(8, flat.v.cfg["x_ref"])
    flat.v.y_refs = np.full(8, flat.v.cfg["y_ref"])
    for i in range(8):
        np.testing.assert_array_equal(planned(flat, flat.v, i, flat.sub_scale, flat.S), oracle_windows(flat, i))


def test_a_staring_exposure_gets_one_window_for_every_product():
    v = helpers.make_visit("stare256", n_exposures=2)
    S, sub_scale = 266, 507 - 128
    tr = v.grism.get_trace(v.cfg["x_ref"] + 0.5, v.cfg["y_ref"] + 0.5)
    from wayne_amd import tools
    i0, i1 = tools.crop_spectrum_ind(v.grism.wl_limits[0], v.grism.wl_limits[1], v.wl)
    dy = np.asarray(tr.wl_to_y(v.wl[i0:i1]), dtype=float) - (v.cfg["y_ref"] + 0.5)
    for i in range(2):
        got = planned(None, v, i, sub_scale, S)
        assert got.shape == (v.NSAMP, 2) and (got == got[0]).all()
        # the oracle's rule (visit_science.ScienceVisit.row_window at speed 0), with the visit's one trace
        y = v.y_refs[i] - sub_scale + 5.0
        want = (max(int(np.floor(y + dy.min())) - 14, 5), min(int(np.ceil(y + dy.max())) + 14 + 1, S - 5))
        assert np.abs(got[0] - np.array(want)).max() <= 1


def test_channel_weights_are_the_observers_column_weights(sv):
    for i in range(sv.v.n_exposures):
        got = extraction.channel_weights(sv.v.x_refs[i], sv.edges, sv.sub_scale, sv.S)
        want = sv.column_weights(i)
        assert got.shape == want.shape == (vs.N_CHANNELS, sv.S)
        assert np.abs(got - want).max() <= 1e-12
        assert abs(got.sum() - (sv.edges[-1] - sv.edges[0])) <= 1e-9          # every channel's columns, counted once


def test_the_law_restated_per_column_is_the_observers_extraction(sv):
    rng = np.random.default_rng(5)
    R, S = sv.R, sv.S
    # a synthetic read cube: a bias, a ramp of random slope per pixel, read noise
    bias = rng.uniform(9000.0, 12000.0, (S, S))
    slope = rng.uniform(0.0, 1500.0, (S, S))
    reads = bias[None] + slope[None] * np.arange(R + 1)[:, None, None] + rng.normal(0.0, 20.0, (R + 1, S, S))
    pl = law.Planes(sv.v)
    for a, b in zip(pl.lin + [pl.dark, pl.gain, pl.sky], sv.lin + [sv.dark, sv.gain, sv.sky_template]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(pl.dt, sv.dt)
    for i in (0, 5):
        windows = oracle_windows(sv, i)
        spectra, sky, M, _ = law.restate(reads, pl, windows, vs.BG_COLS)
        ramp, last = sv.extract(i, reads)
        cw = extraction.channel_weights(sv.v.x_refs[i], sv.edges, sv.sub_scale, sv.S)
        got_ramp, got_last = cw @ spectra[:R].sum(axis=0), cw @ spectra[R]
        assert np.abs(got_ramp / ramp - 1.0).max() <= 1e-10 and np.abs(got_last / last - 1.0).max() <= 1e-10
        assert (sky != 0.0).all() and (M > 0.0).all()
    # a step that is off: the sky level is zero and the spectra are the plain sums
    spectra, sky, _, _ = law.restate(reads, pl, windows, vs.BG_COLS, law.ALL & ~law.SKY)
    assert (sky == 0.0).all() and spectra[R].sum() > 0.0
    spectra, sky, _, _ = law.restate(reads, pl, windows, vs.BG_COLS, law.ALL & ~law.LAST_READ)
    assert (spectra[R] == 0.0).all() and sky[R] == 0.0 and (sky[:R] != 0.0).all()


VALIDATOR = r"""
#include "host_plan.h"
extern "C" int check(int S, int R, unsigned steps, const int* lo, const int* hi, int b0, int b1, int* chunks) {
  return wayne::plan::extract_desc_error(S, R, steps, lo, hi, b0, b1, chunks) == nullptr ? 0 : -1;
}
"""


def test_the_descriptor_check_refuses_what_would_leave_the_frame(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    (tmp_path / "v.cpp").write_text(VALIDATOR)
    lib = str(tmp_path / "libv.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, "wayne_amd", "csrc"), str(tmp_path / "v.cpp"), "-o", lib], check=True)
    L = C.CDLL(lib)
    S, R = 74, 3

    def check(windows, bg=(6, 26), steps=31, S=S, R=R):
        lo = (C.c_int * 17)(*([w[0] for w in windows] + [0] * (17 - len(windows))))
        hi = (C.c_int * 17)(*([w[1] for w in windows] + [0] * (17 - len(windows))))
        n = C.c_int(-1)
        return L.check(S, R, steps, lo, hi, bg[0], bg[1], C.byref(n)), n.value

    good = [(5, 40), (10, 50), (20, 69), (5, 69)]
    assert check(good) == (0, 2)                                        # 64 rows: two chunks of 32
    assert check([(0, 74)] * 4) == (0, 3)                               # the whole frame: 74 rows, a remainder
    assert check([(7, 8)] * 4) == (0, 1)                                # one row
    assert check([(5, 40), (50, 50), (20, 69), (5, 69)])[0] != 0        # an empty window
    assert check([(5, 40), (60, 50), (20, 69), (5, 69)])[0] != 0        # ... or a reversed one
    assert check([(5, 40), (10, 75), (20, 69), (5, 69)])[0] != 0        # hi > S
    assert check([(-1, 40), (10, 50), (20, 69), (5, 69)])[0] != 0       # lo < 0
    assert check(good, steps=32 | 31)[0] != 0 and check(good, steps=1 << 31)[0] != 0       # unknown step bits
    assert check(good, bg=(26, 26))[0] != 0 and check(good, bg=(6, 75))[0] != 0 and check(good, bg=(-1, 5))[0] != 0
    # the last-read window is looked at only when the product is formed
    assert check(good[:3] + [(0, 0)])[0] != 0
    assert check(good[:3] + [(0, 0)], steps=31 & ~16) == (0, 2)
    assert check(good[:3] + [(0, 900)], steps=15) == (0, 2)
    assert check(good, R=16)[0] != 0 and check(good, S=1025)[0] != 0


def test_extraction_options_are_planned_per_exposure():
    v = helpers.make_visit("small256", n_exposures=2)
    assert extraction.for_exposure(None, v.grism, v.wl, 1.0, 1.0, 0.0, v.read_times, 379, 266) is None
    one = extraction.Extraction([(5, 9)] * 4)
    assert extraction.for_exposure(one, v.grism, v.wl, 1.0, 1.0, 0.0, v.read_times, 379, 266) is one
    a = extraction.for_exposure(True, v.grism, v.wl, v.x_refs[0], v.y_refs[0], v.scan_speed, v.read_times, 379, 266)
    b = extraction.for_exposure(extraction.ExtractionOptions(margin=3, bg_cols=(7, 9), steps=7), v.grism, v.wl,
                                v.x_refs[0], v.y_refs[0], v.scan_speed, v.read_times, 379, 266)
    np.testing.assert_array_equal(a.row_windows, planned(None, v, 0, 379, 266))
    assert (a.bg_cols, a.steps) == ((6, 26), 31) and (b.bg_cols, b.steps) == ((7, 9), 7)
    inner = (a.row_windows[:, 0] > 5) & (a.row_windows[:, 1] < 261)
    assert inner.any()
    np.testing.assert_array_equal((a.row_windows - b.row_windows)[inner], np.array([[-11, 11]] * int(inner.sum())))
    with pytest.raises(TypeError):
        extraction.for_exposure("yes", v.grism, v.wl, 1.0, 1.0, 0.0, v.read_times, 379, 266)
    with pytest.raises(ValueError):
        extraction.Extraction([(5, 9)])
