"""Wavelength-binned channels of the device-side extraction, host side: the per-row wavelength planner against the
simulator's own bin positions, the law (tests/channel_law.py) against the column spectra and against flux conservation,
the Python and C++ validators, the ctypes struct, the .npz keys, the CLI's usage errors, and what the product buys on
CPU-oracle reads: a line that stays put through a scan and a flat that is taken out again.  Device side:
tests/test_channels_gpu.py."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import channel_law
import extraction_law as law
import helpers
from oracle import wayne_oracle as wo
from wayne_amd import _lib, extraction, grism, run_visit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the planner ----

@pytest.mark.parametrize("name", ["G141", "G102"])
def test_row_solution_against_the_simulators_bin_positions(name):
    # Bound 1 A: ~0.3 A from the term quadratic in x that a linear row solution omits plus ~0.26 A (G102 0.15 A) for
    # planning at the row's centre while the bin sits anywhere in the row
    G = grism.G141() if name == "G141" else grism.G102()
    x_ref, y0, sub_scale, S = 420.3, 500.0, 0, 1024
    wl_a, wl_b = extraction.row_solution(G, x_ref, y0, sub_scale, S)
    assert wl_a.shape == wl_b.shape == (S,) and (wl_b > 0).all()
    wl = np.linspace(G.min_lambda, G.max_lambda, 400)
    mid = int(np.floor(G.get_trace(x_ref, y0).wl_to_y(wl.mean()))) - sub_scale + 5
    worst = one_200 = one_100 = 0.0
    for y_s in np.linspace(y0 - 200.0, y0 + 200.0, 81):
        tr = G.get_trace(x_ref, y_s)
        x, y = tr.wl_to_x(wl) - sub_scale, tr.wl_to_y(wl) - sub_scale         # frame positions, as the device forms them
        row = np.floor(y).astype(int) + 5
        worst = max(worst, float(np.abs(wl_a[row] + wl_b[row] * (x + 5.0) - wl).max()) * 1e4)
        one = float(np.abs(wl_a[mid] + wl_b[mid] * (x + 5.0) - wl).max()) * 1e4
        one_200 = max(one_200, one)
        if abs(y_s - y0) <= 100.0:
            one_100 = max(one_100, one)
    print("%s: a solution per row errs by %.3f A over +-200 px; one solution for all rows by %.1f A (+-100 px: %.1f A)" % (
        name, worst, one_200, one_100))
    assert worst <= 1.0
    assert one_100 > 20.0                                            # the defect the feature removes
    # a sub-array: the same wavelengths at the same detector pixels
    a2, b2 = extraction.row_solution(G, x_ref, y0, 379, 266)
    rows = np.arange(266)
    np.testing.assert_allclose(a2 + b2 * 100.0, wl_a[rows + 379] + wl_b[rows + 379] * (100.0 + 379), rtol=0, atol=1e-12)


# ---- the law ----

def synthetic_reads(S, R=3):
    y, x = np.mgrid[0:S, 0:S]
    ramp = 200.0 * np.exp(-0.5 * ((y - 130.0) / 30.0) ** 2) * (1.0 + 0.3 * np.sin(x / 7.0)) + 0.01 * x
    return np.stack([1000.0 + r * ramp for r in range(R + 1)]).astype(np.float32)


WINDOWS = [(100, 140), (110, 150), (120, 167), (20, 246)]


def test_integer_edges_restate_the_column_spectra():
    v = helpers.make_visit("small256")
    pl = law.Planes(v)
    S = pl.S
    reads = synthetic_reads(S)
    cols = [30, 31, 40, 100, 180, 250]
    edges = 0.5 + 0.0078125 * np.array(cols, dtype=float)            # (e - a) / b is exact
    wl_a, wl_b = np.full(S, 0.5), np.full(S, 0.0078125)
    for steps in (law.ALL, law.ALL & ~law.SKY, law.ALL & ~law.LAST_READ):
        spectra, sky, M, _ = law.restate(reads, pl, WINDOWS, (6, 26), steps)
        got = channel_law.restate(reads, pl, WINDOWS, (6, 26), edges, wl_a, wl_b, steps)
        assert got.sky.tobytes() == sky.tobytes()
        for b in range(len(cols) - 1):
            want = spectra[:, cols[b]:cols[b + 1]].sum(axis=1)
            bound = law.REL * M[:, cols[b]:cols[b + 1]].sum(axis=1)
            assert (np.abs(got.channels[:, b] - want) <= bound).all(), (steps, b)
            np.testing.assert_allclose(got.M[:, b], M[:, cols[b]:cols[b + 1]].sum(axis=1), rtol=1e-12)
        if not steps & law.LAST_READ:
            assert (got.channels[-1] == 0.0).all()
    assert np.abs(got.channels[:-1]).max() > 1000.0


def test_flux_is_conserved():
    v = helpers.make_visit("small256")
    pl = law.Planes(v)
    S = pl.S
    reads = synthetic_reads(S)
    rows = np.arange(S, dtype=float)
    wl_a, wl_b = 1.0 + 2e-4 * (rows - 130.0), np.full(S, 0.005) * (1.0 + 1e-4 * rows)     # slanted, and inside the frame
    edges = np.sort(np.concatenate([[1.31, 1.9], 1.31 + 0.59 * np.random.RandomState(5).uniform(size=30)]))
    steps = law.ALL & ~law.SKY
    got = channel_law.restate(reads, pl, WINDOWS, (6, 26), edges, wl_a, wl_b, steps)
    whole = channel_law.restate(reads, pl, WINDOWS, (6, 26), edges[[0, -1]], wl_a, wl_b, steps)
    ua0, uaC = (edges[0] - wl_a) / wl_b, (edges[-1] - wl_a) / wl_b
    assert ua0[20:246].min() > 5.0 and uaC[20:246].max() < S - 5.0
    for p, term in enumerate(channel_law.pixel_terms(reads, pl, WINDOWS, steps)):
        sl, val, Mv = term
        x = np.arange(S, dtype=float)[None, :]
        w = np.clip(np.minimum(x + 1.0, uaC[sl, None]) - np.maximum(x, ua0[sl, None]), 0.0, 1.0)
        want = (w * val).sum()
        bound = 1e-12 * (w * Mv).sum()
        assert abs(got.P[p].sum() - want) <= bound and abs(whole.P[p, 0] - want) <= bound, p
    assert (got.P > 0).all()


# ---- plans and validation ----

def test_channels_are_validated():
    ch = extraction.Channels([1.1, 1.2, 1.4])
    assert ch.n == 2 and ch.flat and not ch.with_flat(False).flat
    lin = extraction.Channels.linear(1.1, 1.7, 20)
    assert lin.n == 20 and lin.edges_um.tobytes() == np.linspace(1.1, 1.7, 21).tobytes()
    assert extraction.Channels.linear(1.0, 2.0, 256).n == 256
    nan, inf = float("nan"), float("inf")
    for bad in ([1.1], [], [1.1, nan], [1.1, inf], [1.2, 1.1], [1.1, 1.1], [1.1, 1.2, 1.2], np.linspace(1, 2, 258), [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            extraction.Channels(bad)
    for n in (0, -1, 257):
        with pytest.raises(ValueError):
            extraction.Channels.linear(1.1, 1.7, n)
    with pytest.raises(ValueError):
        extraction.Channels.linear(1.7, 1.1, 5)
    with pytest.raises(TypeError):
        extraction.Extraction(WINDOWS, channels=[1.1, 1.2], row_solution=(np.zeros(266), np.ones(266)))


def test_plans_carry_the_channels_and_mirror_every_refusal():
    S = 266
    ch = extraction.Channels.linear(1.1, 1.7, 20)
    sol = (np.full(S, 0.9), np.full(S, 0.0046))
    plain = extraction.Extraction(WINDOWS)
    assert plain.channels is None and plain.row_solution is None and plain.hull is None
    plan = extraction.Extraction(WINDOWS, channels=ch, row_solution=sol)
    assert plan.channels is ch and plan.hull == (int(np.floor(0.2 / 0.0046)), int(np.ceil(0.8 / 0.0046)))
    assert bytes(plan.desc()) == bytes(plain.desc())                 # the extract descriptor does not change
    kept = plan.with_crrej(True)
    assert kept.channels is ch and kept.crrej.k == 8.0 and kept.row_solution[0].tobytes() == sol[0].tobytes()
    assert plan.with_channels(None).channels is None and plan.with_channels(None).row_solution is None
    with pytest.raises(ValueError):
        extraction.Extraction(WINDOWS, channels=ch)                  # no row solution
    nan, inf = float("nan"), float("inf")

    def changed(arr, y, value):
        out = arr.copy()
        out[y] = value
        return out

    for a, b in ((changed(sol[0], 20, nan), sol[1]), (changed(sol[0], 245, inf), sol[1]), (sol[0], changed(sol[1], 100, 0.0)),
                 (sol[0], changed(sol[1], 100, -1.0)), (sol[0], changed(sol[1], 30, nan)), (sol[0], changed(sol[1], 30, inf)),
                 (sol[0], sol[1][:-1])):
        with pytest.raises(ValueError):
            extraction.Extraction(WINDOWS, channels=ch, row_solution=(a, b))
    # rows outside every formed window are not looked at; the last-read window counts only when it is formed
    extraction.Extraction(WINDOWS, channels=ch, row_solution=(changed(sol[0], 19, nan), changed(sol[1], 246, -1.0)))
    no_last = extraction.ALL & ~extraction.LAST_READ
    extraction.Extraction(WINDOWS, steps=no_last, channels=ch, row_solution=(changed(sol[0], 50, nan), sol[1]))
    # the hull: clamped to the frame, empty when no channel touches it, refused one column beyond the cap
    assert extraction.Extraction(WINDOWS, channels=extraction.Channels([0.1, 0.2]), row_solution=sol).hull == (0, 0)
    assert extraction.Extraction(WINDOWS, channels=extraction.Channels([3.0, 4.0]), row_solution=sol).hull == (S, S)
    assert extraction.Extraction(WINDOWS, channels=extraction.Channels([0.1, 4.0]), row_solution=sol).hull == (0, S)
    px = 2.0 ** -10                                                  # (exact: an edge falls on a pixel boundary)
    wide = (np.full(1024, 1.0), np.full(1024, px))
    w16 = [(300, 320)] * 15 + [(290, 331)]
    assert extraction.Extraction(w16, channels=extraction.Channels([1.0 + 300 * px, 1.0 + 684 * px]), row_solution=wide).hull == (300, 684)
    with pytest.raises(ValueError):
        extraction.Extraction(w16, channels=extraction.Channels([1.0 + 300 * px, 1.0 + 684.5 * px]), row_solution=wide)
    # options and frames
    opts = extraction.ExtractionOptions(channels=ch, crrej=True)
    assert opts.channels is ch and extraction.ExtractionOptions().channels is None
    G = grism.G141()
    args = (G, np.linspace(1.0, 1.8, 50), 404.5, 420.0, 3.0, [0.3, 7.6, 15.0, 22.3], 379, S)
    planned = extraction.for_exposure(opts, *args)
    want = extraction.row_solution(G, 404.5, 420.0, 379, S)
    assert planned.channels is ch and planned.crrej.k == 8.0
    assert planned.row_solution[0].tobytes() == want[0].tobytes() and planned.row_solution[1].tobytes() == want[1].tobytes()
    assert 120 <= planned.hull[1] - planned.hull[0] <= 150
    other = extraction.Channels.linear(1.2, 1.6, 8)
    assert extraction.for_exposure(opts, *args, channels=other).channels is other
    assert extraction.for_exposure(True, *args, channels=other).row_solution[0].tobytes() == want[0].tobytes()
    assert extraction.for_exposure(opts, *args, channels=False).channels is None
    assert extraction.for_exposure(True, *args).channels is None
    with pytest.raises(ValueError):
        extraction.for_exposure(None, *args, channels=other)


def test_algorithmic_bytes_count_the_bins_kernels():
    S, R = 266, 3
    ch = extraction.Channels.linear(1.1, 1.7, 20)
    sol = (np.full(S, 0.9), np.full(S, 0.0046))
    windows = [(100, 140), (110, 150), (120, 160), (100, 160)]
    plan = extraction.Extraction(windows, channels=ch, row_solution=sol)
    base = extraction.algorithmic_bytes(extraction.Extraction(windows), S, R)
    assert extraction.algorithmic_bytes(plan, S, R) == base and extraction.algorithmic_bytes(plan, S, R, channels=False) == base
    hull = plan.hull[1] - plan.hull[0]
    more = extraction.algorithmic_bytes(plan, S, R, channels=True) - base
    first, later = 2 * 4 + 16 + 4 + 4 + 4 + 16, 3 * 4 + 16 + 8 + 4 + 4 + 16
    pixels = hull * (40 * first + 40 * later + 40 * later + 60 * first)
    assert more == pixels + 180 * 16 + 2 * 8 * 2 * 20 * 8 + (R + 1) * 20 * 8
    assert extraction.algorithmic_bytes(plan.with_channels(ch.with_flat(False)), S, R, channels=True) - base == more - 180 * hull * 16
    cr = extraction.algorithmic_bytes(plan, S, R, crrej=True, channels=True) - extraction.algorithmic_bytes(plan, S, R, crrej=True)
    assert cr == more + 180 * hull * 2


def test_channels_struct_mirrors_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    fields = ("n_channels", "edges_um", "wl_a", "wl_b", "flags")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wayne_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(wayne_channels_desc));\n' +
                   "".join('  printf(" %%zu", offsetof(wayne_channels_desc, %s));\n' % f for f in fields) +
                   '  printf(" %u %d %d %d\\n", WAYNE_C_FLAT, WAYNE_MAX_CHANNELS, WAYNE_MAX_CHANNEL_HULL, WAYNE_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True)
    out = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.ChannelsDesc) == 40
    assert out[1:6] == [getattr(_lib.ChannelsDesc, f).offset for f in fields] == [0, 8, 16, 24, 32]
    assert out[6:] == [_lib.C_FLAT, _lib.MAX_CHANNELS, _lib.MAX_CHANNEL_HULL, _lib.ABI_VERSION] == [1, 256, 384, 7]
    for name in ("wayne_exposure_set_channels", "wayne_exposure_channels"):
        assert name in _lib.SYMBOLS


HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "host_plan.h"
using namespace wayne;
int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int S = 266, R = 3;
  int lo[17] = {100, 110, 120, 20}, hi[17] = {140, 150, 167, 246};
  std::vector<double> a(S, 0.9), b(S, 0.0046), e(21);
  for (int i = 0; i <= 20; ++i) e[i] = 1.1 + 0.03 * i;
  int bad = 0, u0 = -1, u1 = -1;
  auto expect = [&](bool ok, unsigned steps, int n, const std::vector<double>& ed, const std::vector<double>& wa,
                    const std::vector<double>& wb, unsigned flags, const char* what) {
    const char* why = plan::channels_desc_error(S, R, steps, lo, hi, n, ed.data(), wa.data(), wb.data(), flags, &u0, &u1);
    if ((why == nullptr) != ok) { std::printf("WRONG %s: %s\n", what, why ? why : "accepted"); ++bad; }
  };
  auto with = [](std::vector<double> v, int i, double x) { v[i] = x; return v; };
  expect(true, X_ALL, 20, e, a, b, C_FLAT, "a good plan");
  if (u0 != (int)std::floor(0.2 / 0.0046) || u1 != (int)std::ceil(0.8 / 0.0046)) { std::printf("WRONG hull %d %d\n", u0, u1); ++bad; }
  expect(true, X_ALL, 1, e, a, b, 0, "one channel");
  expect(false, X_ALL, 0, e, a, b, 0, "no channel");
  expect(false, X_ALL, 257, e, a, b, 0, "257 channels");
  expect(false, X_ALL, 20, with(e, 3, nan), a, b, 0, "nan edge");
  expect(false, X_ALL, 20, with(e, 20, inf), a, b, 0, "inf edge");
  expect(false, X_ALL, 20, with(e, 4, e[3]), a, b, 0, "equal edges");
  expect(false, X_ALL, 20, with(e, 4, e[2]), a, b, 0, "decreasing edges");
  expect(false, X_ALL, 20, e, with(a, 20, nan), b, 0, "nan wl_a on a window's first row");
  expect(false, X_ALL, 20, e, with(a, 245, inf), b, 0, "inf wl_a on a window's last row");
  expect(true, X_ALL, 20, e, with(a, 19, nan), with(b, 246, -1.0), 0, "bad values outside every window");
  expect(true, X_ALL & ~X_LAST_READ, 20, e, with(a, 50, nan), b, 0, "bad value in the last-read window alone, not formed");
  expect(false, X_ALL, 20, e, a, with(b, 100, 0.0), 0, "wl_b 0");
  expect(false, X_ALL, 20, e, a, with(b, 100, -0.0046), 0, "wl_b negative");
  expect(false, X_ALL, 20, e, a, with(b, 100, nan), 0, "wl_b nan");
  expect(false, X_ALL, 20, e, a, with(b, 100, inf), 0, "wl_b inf");
  expect(false, X_ALL, 20, e, a, b, 2u, "unknown flag");
  expect(false, X_ALL, 20, e, a, b, 0x80000001u, "unknown high flag");
  expect(true, X_ALL, 20, e, a, std::vector<double>(S, 0.001), 0, "600 columns, clamped to the frame's 266 before the cap");
  expect(true, X_ALL, 1, std::vector<double>{0.1, 0.2}, a, b, 0, "left of the frame");
  if (u0 != 0 || u1 != 0) { std::printf("WRONG left hull %d %d\n", u0, u1); ++bad; }
  expect(true, X_ALL, 1, std::vector<double>{3.0, 4.0}, a, b, 0, "right of the frame");
  if (u0 != S || u1 != S) { std::printf("WRONG right hull %d %d\n", u0, u1); ++bad; }
  expect(true, X_ALL, 1, std::vector<double>{-1e300, 1e300}, a, b, 0, "huge edges");
  if (u0 != 0 || u1 != S) { std::printf("WRONG whole hull %d %d\n", u0, u1); ++bad; }
  expect(false, X_ALL, 1, std::vector<double>{1.0, 1.5}, a, with(b, 100, 5e-324), 0, "an edge without a finite column");
  // the cap, on a frame wide enough to reach it
  {
    const int S2 = 1024;
    const double px = 0.0009765625;   // 2^-10: exact
    std::vector<double> a2(S2, 1.0), b2(S2, px);
    int lo2[17], hi2[17];
    for (int j = 0; j < 17; ++j) { lo2[j] = 300; hi2[j] = 320; }
    const double at[2] = {1.0 + 300 * px, 1.0 + 684 * px}, beyond[2] = {1.0 + 300 * px, 1.0 + 684.5 * px};
    const char* why = plan::channels_desc_error(S2, 15, X_ALL, lo2, hi2, 1, at, a2.data(), b2.data(), 0, &u0, &u1);
    if (why || u0 != 300 || u1 != 684) { std::printf("WRONG at the cap: %s %d %d\n", why ? why : "", u0, u1); ++bad; }
    if (!plan::channels_desc_error(S2, 15, X_ALL, lo2, hi2, 1, beyond, a2.data(), b2.data(), 0)) { std::printf("WRONG beyond the cap\n"); ++bad; }
  }
  std::printf("checked\n");
  return bad ? 1 : 0;
}
"""


def test_channels_desc_error_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "channels_plan.cpp"
    src.write_text(HARNESS)
    exe = str(tmp_path / "channels_plan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "wayne_amd", "csrc"), str(src), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checked" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr


def test_npz_keys_with_and_without_channels():
    S, R, n = 266, 3, 2
    ch = extraction.Channels.linear(1.1, 1.7, 20).with_flat(False)
    sol = (np.full(S, 0.9), np.full(S, 0.0046))
    base = ["spectra", "sky", "exposure_index", "row_lo", "row_hi", "bg_cols", "x_ref", "y_ref", "read_times", "exp_start"]
    args = (np.zeros((n, R + 1, S)), np.zeros((n, R + 1)), [0, 1])
    more = ([1.0, 2.0], [3.0, 4.0], [1.0, 2.0, 3.0], [0.0, 9.0])
    f = io.BytesIO()
    extraction.save_npz(f, *args, [extraction.Extraction(WINDOWS)] * n, *more)
    f.seek(0)
    assert sorted(np.load(f).files) == sorted(base)
    f = io.BytesIO()
    channels = np.arange(n * (R + 1) * 20, dtype=float).reshape(n, R + 1, 20)
    extraction.save_npz(f, *args, [extraction.Extraction(WINDOWS, channels=ch, row_solution=sol)] * n, *more, channels=channels)
    f.seek(0)
    z = np.load(f)
    assert sorted(z.files) == sorted(base + ["channels", "channel_edges_um", "channel_flat", "wl_a", "wl_b"])
    assert z["channels"].tobytes() == channels.tobytes() and z["channel_edges_um"].tobytes() == ch.edges_um.tobytes()
    assert not bool(z["channel_flat"]) and z["wl_a"].shape == (n, S) and z["wl_b"][1].tobytes() == sol[1].tobytes()


def test_cli_argument_errors():
    yml = os.path.join(ROOT, "tests", "fixtures", "mini_visit", "params.yml")
    for argv, word in ((["--channels", "1.1:1.7:20"], "--spectra"), (["--no-channel-flat"], "--channels"),
                       (["--spectra-only", "x.npz", "--no-channel-flat"], "--channels"),
                       (["--spectra-only", "x.npz", "--channels", "1.1:1.7"], "LO:HI:N"),
                       (["--spectra-only", "x.npz", "--channels", "1.1:1.7:0"], "LO:HI:N"),
                       (["--spectra-only", "x.npz", "--channels", "1.1:1.7:257"], "LO:HI:N"),
                       (["--spectra-only", "x.npz", "--channels", "1.7:1.1:20"], "LO:HI:N"),
                       (["--spectra-only", "x.npz", "--channels", "a:b:c"], "LO:HI:N"),
                       (["--spectra", "x.npz", "--channels", "nan:1.7:20"], "LO:HI:N")):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml] + argv)
        assert word in str(e.value), argv


# ---- what the product buys, on CPU-oracle reads ----

LINE_UM = 1.60
_science = {}


def science_case():
    """small256 without stellar, read and sky noise and without cosmic rays, on the same counters: (A) a continuum with one
    narrow emission line near the red end, the flat multiplied in; (B) the continuum alone; (C) as A without the flat."""
    if _science:
        return _science
    v = helpers.make_visit("small256")
    eo = helpers.oracle_generator(v)
    quiet = dict(add_stellar_noise=False, add_read_noise=False, sky_background=0.0, cosmic_rate=None)
    # (the line is strong: the oracle throws every electron at a random offset keyed by its index, so the continuum of
    # A and B lands differently and A - B carries its scatter -- ~400 e- in the 0.3 s of the first read interval, against
    # ~18 000 e- of line: ~1 A on the centroid)
    line = v.stellar_flux * (1.0 + 100.0 * np.exp(-0.5 * ((v.wl - LINE_UM) / 0.0015) ** 2))

    def reads(**over):
        kw = v.frame_kwargs(0, **dict(quiet, **over))
        draws = wo.PhiloxDraws(v.seed, 0, v.detector.light_sensitive_size(v.SUBARRAY))
        return np.stack(eo.scanning_frame(threads=2, draws=draws, thrower="oracle", **helpers.oracle_kwargs(kw)))

    _science.update(v=v, pl=law.Planes(v), flat=channel_law.Flat(v), A=reads(stellar_flux=line), B=reads(),
                    C=reads(stellar_flux=line, add_flat=False))
    gen = helpers.product_generator(v, 0)
    gen.build_descriptor(None, extraction=True, **v.frame_kwargs(0, **quiet))
    _science["plan"] = gen.extraction_plan
    _science["x_ref"], _science["y_ref"] = v.x_refs[0], v.y_refs[0]
    return _science


def test_a_line_keeps_its_wavelength_through_the_scan():
    s = science_case()
    v, pl, plan = s["v"], s["pl"], s["plan"]
    S, R = pl.S, v.NSAMP - 1
    wl_a, wl_b = extraction.row_solution(v.grism, s["x_ref"], s["y_ref"], 507 - 128, S)
    px = float(np.median(wl_b))
    edges = LINE_UM + px * (np.arange(16) - 7.5)                     # 1-pixel-wide channels about the line
    centres = 0.5 * (edges[1:] + edges[:-1])
    lo, hi = plan.row_windows[R]
    mid = (lo + hi) // 2

    def drift(a, b):
        on = channel_law.restate(s["A"], pl, plan.row_windows, plan.bg_cols, edges, a, b, flat=s["flat"]).channels
        off = channel_law.restate(s["B"], pl, plan.row_windows, plan.bg_cols, edges, a, b, flat=s["flat"]).channels
        d = on - off                                                 # the line alone
        c = (d * centres).sum(axis=1) / d.sum(axis=1)
        assert (d.sum(axis=1)[:R] > 1e4).all()
        return float(c[R - 1] - c[0]) * 1e4, c

    planned, c_planned = drift(wl_a, wl_b)
    single, c_single = drift(np.full(S, wl_a[mid]), np.full(S, wl_b[mid]))
    print("line centroid, last minus first read interval: %.3f A with the planned row solution, %.3f A with the mid-scan "
          "row's solution for every row (ratio %.1f); planned centroid %.5f um for a line at %.2f um" % (
              planned, single, abs(single) / max(abs(planned), 1e-12), c_planned[R - 1], LINE_UM))
    assert abs(single) > 5.0
    assert abs(planned) <= abs(single) / 5.0


def test_the_flat_is_taken_out_again():
    s = science_case()
    v, pl, plan = s["v"], s["pl"], s["plan"]
    S = pl.S
    wl_a, wl_b = extraction.row_solution(v.grism, s["x_ref"], s["y_ref"], 507 - 128, S)
    edges = np.linspace(1.1, 1.7, 21)

    def channels(reads, flat):
        return channel_law.restate(reads, pl, plan.row_windows, plan.bg_cols, edges, wl_a, wl_b, flat=flat).channels

    truth = channels(s["C"], None)                                   # no flat in, none taken out
    corrected, uncorrected = channels(s["A"], s["flat"]), channels(s["A"], None)
    big = truth > 1e5
    left, was = np.abs(corrected - truth)[big], np.abs(uncorrected - truth)[big]
    ratio = float(np.sqrt((left ** 2).mean()) / np.sqrt((was ** 2).mean()))
    print("flat: rms |corrected - flat-free| / rms |uncorrected - flat-free| = %.3g / %.3g = %.3g over %d (product, channel) "
          "pairs above 1e5 e-; worst pair %.3g" % (np.sqrt((left ** 2).mean()), np.sqrt((was ** 2).mean()), ratio, big.sum(),
                                                    float((left / was).max())))
    assert big.sum() >= 10                                           # (the last-read product's bright channels)
    assert (left < was).all()
    assert ratio <= 0.1
