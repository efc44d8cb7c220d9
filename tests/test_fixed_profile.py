"""CPU: the profile planes and the optimal extraction with a supplied profile -- properties of the laws
(tests/fixed_profile_law.py) on hand-made planes, the laws against an ensemble of CPU-oracle exposures, the Python binding
and the host-side argument checks.  Device side: tests/test_fixed_profile_gpu.py."""
import ctypes as C
import io
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import channel_law
import extraction_law as law
import fixed_profile_law as fpl
import helpers
import optimal_law
from oracle import wayne_oracle as wo
from wayne_amd import _lib, extraction, run_visit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [(100, 140), (110, 150), (120, 160), (100, 160)]


def hand_made_planes(S=64, R=3, seed=5):
    """Planes as extraction_law.Planes holds them, made by hand (as tests/test_optimal.py makes them): no non-linearity,
    no dark, a gain that varies from column to column and a sky template that is constant along y."""
    rs = np.random.RandomState(seed)
    pl = types.SimpleNamespace(S=S)
    pl.lin = [np.zeros((S, S)) for _ in range(4)]
    pl.dark = np.zeros((R + 1, S, S))
    pl.gain = np.full((S, S), 2.35)
    pl.gain[5:-5, 5:-5] = 2.35 / (1.0 + 0.05 * rs.standard_normal((1, S - 10)) * np.ones((S - 10, 1)))
    pl.sky = np.zeros((S, S))
    pl.sky[5:-5, 5:-5] = 1.0 + 0.1 * rs.random_sample((1, S - 10)) * np.ones((S - 10, 1))
    pl.dt = np.array([10.0, 12.0, 14.0])[:R]
    return pl


def top_hat(S, R, lit=(24, 31), cols=(20, 50), flux=4000.0):
    """Noise-free reads whose only light is a top-hat along y on the rows `lit`, a smooth spectrum on the columns `cols`
    (the background columns stay dark, so the sky level is exactly 0)."""
    F = np.zeros(S)
    F[cols[0]:cols[1]] = flux * (1.0 + 0.3 * np.sin(np.arange(cols[1] - cols[0]) / 5.0))
    hat = np.zeros(S)
    hat[lit[0]:lit[1]] = 1.0
    return np.stack([1000.0 + r * hat[:, None] * F[None, :] for r in range(R + 1)])


def test_a_noise_free_top_hat_with_its_true_profile_gives_the_box_sum():
    S, R, rn = 64, 3, 20.0
    pl = hand_made_planes(S, R)
    reads = top_hat(S, R)
    windows = [(14, 41)] * (R + 1)                                         # 7 lit rows and 2 x 10 margin rows
    box = optimal_law.box(reads, pl, windows, (6, 16), rn)
    true = np.zeros((27, S))
    true[10:17] = 1.0 / 7.0
    profile = np.concatenate([true] * (R + 1))
    for H in (1, 8, 16):
        got = fpl.restate(reads, pl, windows, H, rn, profile, *box)
        assert got.ok[:, 20:50].all() and not got.ok[:, :3].any() and (box[0][:, 20:50] > 1e4).all()
        assert np.abs(got.optimal - box[0]).max() <= 1e-12 * box[0].max(), H
    # the planes of the same exposure, normalised, are that profile on the lit columns
    pln = fpl.planes(reads, pl, windows, 8, box[1])
    own = fpl.normalise(pln, windows)
    assert np.abs(own[:, 20:50] - profile[:, 20:50]).max() <= 1e-12
    # sum_y S1 = S0: the window sums of the spectra, to rounding
    S0 = optimal_law.window_sum(box[0], 8)
    assert np.allclose(pln[:27].sum(axis=0), S0[0], rtol=1e-12, atol=1e-9 * S0.max())


def test_a_profile_of_zeros_falls_back_to_the_bit():
    S, R, rn = 64, 3, 20.0
    pl = hand_made_planes(S, R)
    reads = top_hat(S, R)
    windows = [(14, 41)] * (R + 1)
    box = optimal_law.box(reads, pl, windows, (6, 16), rn)
    profile = np.concatenate([np.full((27, S), 1.0 / 27.0)] * (R + 1))
    profile[:, 30:40] = 0.0
    profile[:27, 42] = -0.5                                               # clamped to 0 on every row: W = 0 as well
    got = fpl.restate(reads, pl, windows, 8, rn, profile, *box)
    assert not got.ok[:, 30:40].any() and not got.ok[0, 42] and got.ok[1:, 42].all() and got.ok[:, 25].all()
    assert got.optimal[~got.ok].tobytes() == box[0][~got.ok].tobytes()
    assert got.optimal_var[~got.ok].tobytes() == box[2][~got.ok].tobytes()
    assert np.isfinite(got.optimal).all() and np.isfinite(got.optimal_var).all()


def test_profile_sum_normalises_every_column_of_every_window():
    S = 64
    plan = extraction.Extraction([(10, 20), (15, 30), (25, 50), (8, 55)], variance=True, optimal=True)
    rows = extraction.window_heights(plan)
    assert rows == (10, 15, 25, 47) == fpl.heights(plan.row_windows)
    rs = np.random.RandomState(2)
    planes = rs.random_sample((sum(rows), S)) + 0.1
    planes[:10, 7] = -1.0                                                 # a column whose sum is not positive: zeros
    planes[10:25, 9] = 0.0
    prof = extraction.ProfileSum().add(plan, planes).profile()
    assert prof.rows == rows and prof.exposures == 1 and prof.planes.tobytes() == fpl.normalise(planes, plan.row_windows).tobytes()
    for p in range(4):
        tot = prof.window(p).sum(axis=0)
        dead = (p == 0) * (np.arange(S) == 7) + (p == 1) * (np.arange(S) == 9)
        assert np.abs(tot[~dead.astype(bool)] - 1.0).max() < 1e-14 and (tot[dead.astype(bool)] == 0.0).all()
    # a sum of several is the normalised sum, not the mean of normalised planes: a flux-weighted mean
    more = rs.random_sample(planes.shape) * 3.0
    both = extraction.ProfileSum().add(plan, planes).add(plan, more).profile()
    assert both.exposures == 2 and both.planes.tobytes() == fpl.normalise(planes + more, plan.row_windows).tobytes()
    # other window heights, or a plane of another shape, cannot be added
    acc = extraction.ProfileSum().add(plan, planes)
    with pytest.raises(ValueError):
        acc.add(extraction.Extraction([(10, 20), (15, 30), (25, 50), (8, 56)]), np.zeros((sum(rows) + 1, S)))
    with pytest.raises(ValueError):
        acc.add(plan, planes[:-1])
    with pytest.raises(ValueError):
        extraction.ProfileSum().profile()


def test_with_whole_column_channels_the_sky_term_is_taken_once():
    """channel_variance: sum 1 / W plus (sum G / W)^2 sky_var -- larger than the sum of optimal_var's own sky terms."""
    S, R, rn = 266, 3, 20.0
    rs = np.random.RandomState(1)
    res = optimal_law.Result(None, None, np.ones((R + 1, S), dtype=bool), None, 1.0 + rs.random_sample((R + 1, S)),
                             rs.random_sample((R + 1, S)), None)
    sky_var = np.array([0.5, 0.25, 1.0, 2.0])
    got = fpl.channel_variance(res, 2, np.zeros((R + 1, S)), sky_var)
    c0 = fpl.CHANNEL_COLS[0]
    k = (res.G[2] / res.W[2])[c0:c0 + 13]
    assert got.shape == (10,) and np.isclose(got[0], (1.0 / res.W[2][c0:c0 + 13]).sum() + k.sum() ** 2)
    summed = fpl.channel_sums(1.0 / res.W[2] + (res.G[2] / res.W[2]) ** 2 * sky_var[2])
    assert (got > summed).all()
    assert fpl.channel_sums(np.arange(S, dtype=float))[1] == sum(range(c0 + 13, c0 + 26))


_ensemble = {}


def oracle_ensemble(n=32, n_profile=16, H=8, rn=20.0):
    """n CPU-oracle exposures of small256 that differ in their draws alone, set up as tests/test_optimal.py's
    oracle_ensemble, and a profile summed from the planes of the n_profile exposures behind them (indices n .. n + n_profile
    - 1) -> dict: spectra [n, R + 1, S], optimal with the exposures' own profile and with the supplied one, and the
    predicted channel variances [n, R + 1, 10] of both."""
    key = (n, n_profile, H, rn)
    if key in _ensemble:
        return _ensemble[key]
    v = helpers.make_visit("small256")
    pl = law.Planes(v)
    S = pl.S
    eo = helpers.oracle_generator(v)
    kw = v.frame_kwargs(0, cosmic_rate=None, ssv_generator=None, add_flat=False)
    ch = extraction.Channels.linear(1.15, 1.65, 10).with_flat(False)
    plan = extraction.ExtractionOptions(channels=ch, variance=True, optimal=True).plan(v.grism, v.wl, kw["x_ref"], kw["y_ref"],
                                                                                       kw["scan_speed"], v.read_times, 507 - 128, S)
    sol = plan.row_solution
    windows = plan.row_windows

    def exposure(i):
        draws = wo.PhiloxDraws(v.seed, i, v.detector.light_sensitive_size(v.SUBARRAY))
        reads = np.stack(eo.scanning_frame(threads=2, draws=draws, thrower="oracle", **helpers.oracle_kwargs(kw)))
        return reads, optimal_law.box(reads, pl, windows, plan.bg_cols, rn)

    acc = extraction.ProfileSum()
    for i in range(n, n + n_profile):
        reads, box = exposure(i)
        acc.add(plan, fpl.planes(reads, pl, windows, H, box[1]))
    prof = acc.profile()
    out = {k: [] for k in ("spectra", "own", "fixed", "own_pred", "fixed_pred", "box_ch", "own_ch", "own_ch_var", "fixed_ch",
                           "fixed_ch_var")}
    R = len(windows) - 1
    for i in range(n):
        reads, box = exposure(i)
        own = optimal_law.restate(reads, pl, windows, H, rn, *box)
        fixed = fpl.restate(reads, pl, windows, H, rn, prof.planes, *box)
        out["spectra"].append(box[0])
        out["own"].append(own.optimal)
        out["fixed"].append(fixed.optimal)
        out["own_pred"].append([fpl.channel_variance(own, p, box[2], box[3]) for p in range(R + 1)])
        out["fixed_pred"].append([fpl.channel_variance(fixed, p, box[2], box[3]) for p in range(R + 1)])
        # the planned channels (fractional edges, the slanted row solution): the box channels and the optimal channels' law
        out["box_ch"].append(channel_law.restate(reads, pl, windows, plan.bg_cols, ch.edges_um, sol[0], sol[1], sky=box[1]).channels)
        for name, profile in (("own", None), ("fixed", prof.planes)):
            got = fpl.channels(reads, pl, windows, H, rn, profile, *box, ch.edges_um, sol[0], sol[1])
            out[name + "_ch"].append(got.channels_opt)
            out[name + "_ch_var"].append(got.channels_opt_var)
        if i == 0:
            c0, c1 = fpl.CHANNEL_COLS
            out["all_ok"] = bool(own.ok[R, c0:c1].all() and fixed.ok[R, c0:c1].all())
    _ensemble[key] = {k: np.array(a) for k, a in out.items()}
    _ensemble[key]["profile"] = prof
    return _ensemble[key]


def test_a_visits_profile_gives_trustworthy_channel_sums_on_cpu_oracle_reads():
    """32 exposures that differ in their draws alone, the profile from 16 further ones, H = 8, 10 channels of 13 whole
    columns (59 .. 188): with such edges a channel of the optimal extraction is the sum of its columns.  Asserted on the
    last-read product (fixed_profile_law.assert_ensemble; no tuned number): the supplied profile's variance ratio lies 4
    standard deviations below the own profile's, its ensemble variance within 1 +- 4 sqrt(2 / (10 x 31)) = 1 +- 0.32 of the
    prediction, its paired bias within 5 standard deviations of the paired mean -- and the exposures' own profile FAILS the
    prediction (its noise is common to the 13 columns of a channel).  Measured (the README's table): last read 0.41 / 0.87
    of the box, 0.86 / 1.80 of the prediction.  Every interval's figures are printed; interval 0 is nearly unlit, the stated
    limit."""
    n = 32
    e = oracle_ensemble(n)
    R = e["spectra"].shape[1] - 1
    assert e["all_ok"] and e["profile"].exposures == 16 and abs(4 * fpl.ensemble_sd(n) - 0.32) < 5e-3
    for p in list(range(R)) + [R]:
        fixed = fpl.channel_figures(e["fixed"][:, p], e["fixed_pred"][:, p], e["spectra"][:, p])
        own = fpl.channel_figures(e["own"][:, p], e["own_pred"][:, p], e["spectra"][:, p])
        print("CPU oracle, %d exposures, %s: channel variance / box: supplied profile %.3f, own profile %.3f; ensemble / "
              "predicted: %.3f, %.3f; bias %+.2e (5 sd: %.1e), %+.2e" % (n, "last read" if p == R else "interval %d" % p, fixed[0],
                                                                       own[0], fixed[1], own[1], fixed[2], fixed[3], own[2]))
    fpl.assert_ensemble(fixed, own, n, "CPU oracle")


def test_optimal_carries_the_profile_and_plans_pick_theirs():
    assert extraction.Optimal().profile is None and extraction.Optimal().deliver_profile is False
    rows = tuple(hi - lo for lo, hi in WINDOWS)
    prof = extraction.Profile(np.full((sum(rows), 266), 0.01), rows, exposures=3)
    assert prof.window(2).shape == (40, 266) and prof.planes.dtype == np.float64 and prof.exposures == 3
    for bad in (5, "x", np.zeros((3, 3))):
        with pytest.raises(TypeError):
            extraction.Optimal(8, profile=bad)
    with pytest.raises(TypeError):
        extraction.Optimal(8, profile={1: 5})
    for planes, r in ((np.zeros((sum(rows) + 1, 266)), rows), (np.zeros(sum(rows)), rows), (np.zeros((40, 266)), (40,)),
                      (np.zeros((sum(rows), 266)), (0,) + rows[1:]), (np.full((sum(rows), 266), np.nan), rows)):
        with pytest.raises(ValueError):
            extraction.Profile(planes, r)
    own = extraction.Optimal(5, profile=prof, deliver_profile=True)
    assert own.profile is prof and own.deliver_profile and own.desc().half_width == 5
    assert C.sizeof(own.desc()) == 4                                       # wayne_optimal_desc keeps its 4 bytes
    off = own.with_profile(None)
    assert off.profile is None and not off.deliver_profile and off.half_width == 5
    plan = extraction.Extraction(WINDOWS, variance=True, optimal=own)
    assert plan.optimal is own and plan.with_crrej(True).optimal is own and plan.with_variance(None).optimal is None
    assert extraction.window_heights(plan) == rows
    # the frame's optimal= replaces the plan's, profile and all
    args = (None, None, 0.0, 0.0, 0.0, [1.0], 0, 266)
    assert extraction.for_exposure(extraction.Extraction(WINDOWS, variance=True), *args, optimal=own).optimal is own
    # {profile_key: Profile}: a plan takes the profile of its window heights and scan direction, or says that none fits
    assert extraction.profile_key(plan, 1.5) == (rows, 1) and extraction.profile_key(plan, -0.2) == (rows, -1)
    assert extraction.profile_key(plan, None) == (rows, 0)
    both = extraction.Optimal(5, profile={(rows, 1): prof})
    picked = extraction.pick_profile(extraction.Extraction(WINDOWS, variance=True, optimal=both), 2.0)
    assert picked.optimal.profile is prof and picked.optimal.half_width == 5
    with pytest.raises(ValueError) as e:
        extraction.pick_profile(extraction.Extraction(WINDOWS, variance=True, optimal=both), -2.0)
    assert "no profile for window heights" in str(e.value)
    assert extraction.pick_profile(plan, 2.0) is plan and extraction.pick_profile(None, 2.0) is None


def test_the_new_symbols_are_declared_and_bound(tmp_path):
    names = ("wayne_exposure_deliver_profile", "wayne_exposure_set_optimal_profile", "wayne_exposure_fetch_profile",
             "wayne_exposure_profile", "wayne_ctx_profile_uploads", "wayne_exposure_set_optimal_profile_tagged")
    L = _lib.load()
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert _lib.ABI_VERSION == 7 and L.wayne_abi_version() == 7
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    # the header declares them with the argument types the binding passes: a C program that assigns each to a pointer
    # of the bound type compiles without a warning
    src = tmp_path / "symbols.c"
    src.write_text('#include <stdio.h>\n#include "wayne_hip.h"\n'
                   'int main(void) {\n'
                   '  int (*a)(wayne_ctx *, int, int) = wayne_exposure_deliver_profile;\n'
                   '  int (*b)(wayne_ctx *, int, const double *, const int *) = wayne_exposure_set_optimal_profile;\n'
                   '  int (*c)(wayne_ctx *, int) = wayne_exposure_fetch_profile;\n'
                   '  int (*d)(wayne_ctx *, int, const double **, size_t *) = wayne_exposure_profile;\n'
                   '  unsigned long long (*e)(const wayne_ctx *) = wayne_ctx_profile_uploads;\n'
                   '  int (*f)(wayne_ctx *, int, const double *, const int *, uint64_t) = wayne_exposure_set_optimal_profile_tagged;\n'
                   '  printf("%d %zu\\n", a && b && c && d && e && f, sizeof(wayne_optimal_desc));\n  return 0;\n}\n')
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(tmp_path / "symbols.o")], check=True)
    assert _lib.SYMBOLS["wayne_exposure_profile"][1][3] == C.POINTER(C.c_size_t)


HARNESS = r"""
#include <climits>
#include <cstdio>
#include <vector>
#include "host_plan.h"
using namespace wayne;
int main() {
  int bad = 0;
  auto expect = [&](bool ok, int S, int R, std::vector<int> rows, size_t want, const char* what) {
    size_t n = 12345;
    const char* why = plan::profile_rows_error(S, R, rows.empty() ? nullptr : rows.data(), &n);
    if ((why == nullptr) != ok) { std::printf("WRONG %s: %s\n", what, why ? why : "accepted"); ++bad; }
    if (ok && n != want) { std::printf("WRONG %s: count %zu\n", what, n); ++bad; }
    if (!ok && n != 12345) { std::printf("WRONG %s: count written on a refusal\n", what); ++bad; }
  };
  expect(true, 266, 3, {40, 40, 40, 60}, (size_t)180 * 266, "small256");
  expect(true, 266, 3, {1, 266, 1, 0}, (size_t)268 * 266, "extremes; no last read");
  expect(true, 1024, 15, std::vector<int>(16, 1024), (size_t)16 * 1024 * 1024, "the largest");
  expect(false, 266, 3, {0, 40, 40, 60}, 0, "an empty interval window");
  expect(false, 266, 3, {40, 40, 40, 267}, 0, "taller than the frame");
  expect(false, 266, 3, {40, -1, 40, 60}, 0, "negative");
  expect(false, 266, 3, {40, INT_MAX, 40, 60}, 0, "INT_MAX");
  expect(false, 266, 3, {INT_MIN, 40, 40, 60}, 0, "INT_MIN");
  expect(false, 266, 3, {}, 0, "null");
  expect(false, 266, 0, {40}, 0, "no reads");
  expect(false, 266, 16, std::vector<int>(17, 4), 0, "too many reads");
  expect(false, 0, 3, {1, 1, 1, 1}, 0, "no frame");
  expect(false, 1025, 3, {1, 1, 1, 1}, 0, "too wide a frame");
  // the heights of a plan's windows; the last read's window of a plan without it is not validated: any ints
  const int lo[4] = {100, 110, 120, 100}, hi[4] = {140, 150, 160, 160};
  const int rows[4] = {40, 40, 40, 60}, taller[4] = {40, 40, 41, 60};
  if (!plan::profile_rows_match(266, 3, X_ALL, lo, hi, rows) || plan::profile_rows_match(266, 3, X_ALL, lo, hi, taller)) {
    std::printf("WRONG match\n"); ++bad;
  }
  const int wild_lo[4] = {100, 110, 120, INT_MIN}, wild_hi[4] = {140, 150, 160, INT_MAX};
  const int back_lo[4] = {100, 110, 120, INT_MAX}, back_hi[4] = {140, 150, 160, INT_MIN};
  const unsigned no_last = X_ALL & ~X_LAST_READ;
  if (plan::profile_window_rows(266, 3, no_last, wild_lo, wild_hi, 3) != 266 || plan::profile_window_rows(266, 3, no_last, back_lo, back_hi, 3) != 0 ||
      plan::profile_window_rows(266, 3, no_last, lo, hi, 3) != 60 || plan::profile_window_rows(266, 3, no_last, lo, hi, 1) != 40) {
    std::printf("WRONG window rows of a plan without the last read\n"); ++bad;
  }
  const int none[4] = {40, 40, 40, 0};
  if (!plan::profile_rows_match(266, 3, no_last, back_lo, back_hi, none)) { std::printf("WRONG match without the last read\n"); ++bad; }
  std::printf("checked\n");
  return bad ? 1 : 0;
}
"""


def test_profile_row_checks_in_a_program_of_their_own(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "profile_rows.cpp"
    src.write_text(HARNESS)
    exe = str(tmp_path / "profile_rows")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "wayne_amd", "csrc"), str(src), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checked" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr


def test_algorithmic_bytes_count_the_profile_walks():
    S, R = 266, 3
    plan = extraction.Extraction(WINDOWS, variance=True, optimal=True)
    base = extraction.algorithmic_bytes(plan, S, R, variance=True, optimal=True)
    assert extraction.algorithmic_bytes(plan, S, R, variance=True, optimal=True, profile=False, deliver_profile=False) == base
    pixels = (3 * 40 + 60) * S
    # a supplied profile: one more float64 plane per window pixel, nothing else changes
    assert extraction.algorithmic_bytes(plan, S, R, variance=True, optimal=True, profile=True) - base == pixels * 8
    # delivery: the planes k_extract_rows reads once more (36 bytes for the first interval and the last read, 44 for the
    # others: tests/test_optimal.py) and a float64 written per window pixel
    walk = 40 * S * (36 + 44 + 44) + 60 * S * 36
    assert extraction.algorithmic_bytes(plan, S, R, variance=True, optimal=True, deliver_profile=True) - base == walk + pixels * 8
    cr = extraction.algorithmic_bytes(plan, S, R, crrej=True, variance=True, optimal=True)
    assert (extraction.algorithmic_bytes(plan, S, R, crrej=True, variance=True, optimal=True, profile=True, deliver_profile=True) - cr ==
            walk + pixels * 2 + 2 * pixels * 8)
    # without the last read its window still lies in the planes (zeros are written), but nothing is read for it
    no_last = extraction.Extraction(WINDOWS, steps=extraction.ALL & ~extraction.LAST_READ, variance=True, optimal=True)
    b = extraction.algorithmic_bytes(no_last, S, R, variance=True, optimal=True)
    assert (extraction.algorithmic_bytes(no_last, S, R, variance=True, optimal=True, deliver_profile=True) - b ==
            40 * S * (36 + 44 + 44) + pixels * 8)
    with pytest.raises(ValueError):
        extraction.algorithmic_bytes(plan, S, R, variance=True, profile=True)


def test_options_give_way_to_another_optimal():
    own = extraction.Optimal(5)
    opts = extraction.ExtractionOptions(margin=9, bg_cols=(6, 20), crrej=True, variance=extraction.Variances(7.0), optimal=own)
    other = opts.with_optimal(own.with_profile(None, deliver_profile=True))
    assert other.optimal.deliver_profile and other.optimal.half_width == 5 and opts.optimal is own
    assert (other.margin, other.bg_cols, other.steps, other.crrej, other.variance) == (9, (6, 20), opts.steps, opts.crrej, opts.variance)
    assert opts.with_optimal(None).optimal is None


def test_npz_key_with_and_without_a_visit_level_profile():
    S, R, n = 266, 3, 2
    base = ["spectra", "sky", "exposure_index", "row_lo", "row_hi", "bg_cols", "x_ref", "y_ref", "read_times", "exp_start",
            "spectra_var", "sky_var", "variance_read_noise", "optimal", "optimal_var", "optimal_half_width"]
    args = (np.zeros((n, R + 1, S)), np.zeros((n, R + 1)), [0, 1])
    more = ([1.0, 2.0], [3.0, 4.0], [1.0, 2.0, 3.0], [0.0, 9.0])
    sv, kv = np.ones((n, R + 1, S)), np.ones((n, R + 1))
    plan = extraction.Extraction(WINDOWS, variance=True, optimal=extraction.Optimal(5))

    def keys(**kw):
        f = io.BytesIO()
        extraction.save_npz(f, *args, [plan] * n, *more, variances=(sv, kv, None), optimal=(sv + 1, sv + 2), **kw)
        f.seek(0)
        return np.load(f)

    assert sorted(keys().files) == sorted(base) == sorted(keys(optimal_profile_exposures=None).files)
    assert sorted(keys(optimal_profile_exposures=0).files) == sorted(base)
    z = keys(optimal_profile_exposures=4)
    assert sorted(z.files) == sorted(base + ["optimal_profile_exposures"]) and int(z["optimal_profile_exposures"]) == 4


def test_cli_argument_errors():
    yml = os.path.join(ROOT, "tests", "fixtures", "mini_visit", "params.yml")
    for argv in (["--optimal-profile", "4"], ["--spectra-only", "x.npz", "--variances", "--optimal-profile", "4"]):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml] + argv)
        assert "--optimal-profile needs --optimal" in str(e.value)
    for n in ("0", "-3"):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml, "--spectra-only", "x.npz", "--variances", "--optimal", "--optimal-profile=" + n])
        assert "at least 1 exposure" in str(e.value)


def test_a_visits_profile_gives_trustworthy_planned_channels_on_cpu_oracle_reads():
    """The same ensemble on 10 channels over 1.15 - 1.65 um with the planned slanted row solution (fractional edges): the law
    of the optimal channels (fixed_profile_law.channels) with the visit's profile against the box channels, and against the
    same with the exposures' own profile; the assertions of fixed_profile_law.assert_ensemble on the last-read product."""
    n = 32
    e = oracle_ensemble(n)
    R = e["spectra"].shape[1] - 1
    for p in list(range(R)) + [R]:
        fixed = fpl.delivered_figures(e["fixed_ch"][:, p], e["fixed_ch_var"][:, p], e["box_ch"][:, p])
        own = fpl.delivered_figures(e["own_ch"][:, p], e["own_ch_var"][:, p], e["box_ch"][:, p])
        print("CPU oracle, %d exposures, %s: channels_opt variance / box: visit's profile %.3f, own profile %.3f; ensemble / "
              "predicted: %.3f, %.3f; bias %+.2e (5 sd: %.1e), %+.2e" % (n, "last read" if p == R else "interval %d" % p, fixed[0],
                                                                       own[0], fixed[1], own[1], fixed[2], fixed[3], own[2]))
    fpl.assert_ensemble(fixed, own, n, "CPU oracle, planned channels")


def test_optimal_channels_are_validated_carried_and_written():
    ch = extraction.Channels.linear(1.1, 1.7, 20)
    sol = (np.full(266, 0.9), np.full(266, 0.0046))
    assert extraction.Optimal().channels is False
    opt = extraction.Optimal(5, channels=True)
    assert opt.channels and opt.with_profile(None, deliver_profile=True).channels
    with pytest.raises(ValueError) as e:
        extraction.Extraction(WINDOWS, variance=True, optimal=opt)
    assert "optimal channels need channels" in str(e.value)
    plan = extraction.Extraction(WINDOWS, channels=ch, row_solution=sol, variance=True, optimal=opt)
    assert plan.optimal.channels and plan.with_crrej(True).optimal.channels
    with pytest.raises(ValueError):
        plan.with_channels(None)
    for name in ("wayne_exposure_set_optimal_channels", "wayne_exposure_optimal_channels"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    # the .npz: channels_opt and channels_opt_var only when they were delivered
    n, R, S = 2, 3, 266
    args = (np.zeros((n, R + 1, S)), np.zeros((n, R + 1)), [0, 1])
    more = ([1.0, 2.0], [3.0, 4.0], [1.0, 2.0, 3.0], [0.0, 9.0])
    sv, kv, cv = np.ones((n, R + 1, S)), np.ones((n, R + 1)), np.ones((n, R + 1, 20))

    def keys(**kw):
        f = io.BytesIO()
        extraction.save_npz(f, *args, [plan] * n, *more, channels=cv, variances=(sv, kv, cv), optimal=(sv, sv), **kw)
        f.seek(0)
        return np.load(f)

    without = keys()
    z = keys(channels_opt=(cv + 1, cv + 2))
    assert sorted(set(z.files) - set(without.files)) == ["channels_opt", "channels_opt_var"]
    assert z["channels_opt"].tobytes() == (cv + 1).tobytes() and z["channels_opt_var"].shape == (n, R + 1, 20)
    # the CLI
    yml = os.path.join(ROOT, "tests", "fixtures", "mini_visit", "params.yml")
    for argv in (["--spectra-only", "x.npz", "--variances", "--optimal", "--optimal-channels"],
                 ["--spectra-only", "x.npz", "--channels", "1.1:1.7:5", "--variances", "--optimal-channels"]):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml] + argv)
        assert "--optimal-channels needs --optimal and --channels" in str(e.value)
    # algorithmic bytes: the hull walked once more
    base = extraction.algorithmic_bytes(plan, S, R, channels=True, variance=True, optimal=True)
    more_b = extraction.algorithmic_bytes(plan, S, R, channels=True, variance=True, optimal=True, optimal_channels=True) - base
    hull = plan.hull[1] - plan.hull[0]
    chunks = 2 + 2 + 2 + 2
    walk = hull * (40 * (36 + 44 + 44) + 60 * 36 + 180 * 16) + 180 * 16
    assert more_b == walk + chunks * hull * 8 + 2 * chunks * 3 * 20 * 8 + 2 * (R + 1) * 20 * 8
    fixed_b = extraction.algorithmic_bytes(plan, S, R, channels=True, variance=True, optimal=True, profile=True, optimal_channels=True)
    assert fixed_b - base - more_b == 180 * S * 8 + 180 * hull * 8
    with pytest.raises(ValueError):
        extraction.algorithmic_bytes(plan, S, R, variance=True, optimal=True, optimal_channels=True)


def test_with_whole_column_edges_channels_opt_is_the_column_sums():
    """Hand-made planes, edges on whole columns, one solution for all rows, no flat: the law of the optimal channels gives the
    law of the optimal columns summed over a channel, and sum 1 / W plus the sky term once as its variance -- with the
    exposure's own profile and with a supplied one."""
    S, R, rn, H = 266, 3, 20.0, 8
    pl = hand_made_planes(S, R)
    rs = np.random.RandomState(4)
    y = np.arange(S, dtype=float)[:, None]
    F = 3000.0 * (1.0 + 0.3 * np.sin(np.arange(S) / 9.0))[None, :] * ((np.arange(S) > 40) & (np.arange(S) < 210))
    ramp = np.exp(-0.5 * ((y - 128.0) / 3.0) ** 2) * F
    reads = np.stack([1000.0 + r * ramp + 3.0 * rs.standard_normal((S, S)) for r in range(R + 1)])
    windows = [(110, 146)] * (R + 1)
    box = optimal_law.box(reads, pl, windows, (6, 16), rn)
    a, b = 1.0, 0.00390625                                                # 2^-8: a + b x and (e - a) / b are exact
    edges = a + b * np.array([fpl.CHANNEL_COLS[0] + fpl.CHANNEL_WIDTH * k for k in range(fpl.N_CHANNELS + 1)], dtype=np.float64)
    sol = (np.full(S, a), np.full(S, b))
    supplied = fpl.normalise(fpl.planes(reads, pl, windows, H, box[1]), windows)
    for profile in (None, supplied):
        got = fpl.channels(reads, pl, windows, H, rn, profile, *box, edges, sol[0], sol[1])
        res = (optimal_law.restate(reads, pl, windows, H, rn, *box) if profile is None
               else fpl.restate(reads, pl, windows, H, rn, profile, *box))
        c0, c1 = fpl.CHANNEL_COLS
        assert res.ok[:, c0:c1].all() and got.ok[:, c0:c1].all()
        assert (np.abs(got.channels_opt - fpl.channel_sums(res.optimal)) <= 1e-12 * got.M).all()
        for p in range(R + 1):
            once = fpl.channel_variance(res, p, box[2], box[3])
            assert np.allclose(got.channels_opt_var[p], once, rtol=1e-12, atol=0.0)
            assert (got.channels_opt_var[p] > fpl.channel_sums(res.optimal_var[p])).all()   # not the sum of optimal_var
    # a column that falls back: its box terms are binned -- d for e, bt for k, the pixel variance for ev
    dark = supplied.copy()
    dark[:, 100] = 0.0
    got = fpl.channels(reads, pl, windows, H, rn, dark, *box, edges, sol[0], sol[1])
    res = fpl.restate(reads, pl, windows, H, rn, dark, *box)
    assert not res.ok[:, 100].any() and (res.optimal[:, 100] == box[0][:, 100]).all()
    assert (np.abs(got.channels_opt - fpl.channel_sums(res.optimal)) <= 1e-12 * got.M).all()


def test_a_profile_is_read_only_and_its_tag_names_its_content():
    rows = (3, 4, 5, 6)
    rs = np.random.RandomState(9)
    planes = rs.random_sample((18, 74))
    a, b = extraction.Profile(planes, rows), extraction.Profile(planes.copy(), rows, exposures=7)
    assert a.tag == b.tag != 0 and 0 < a.tag < 2 ** 64               # the content, not the object or the count
    assert a.planes is not planes and not a.planes.flags.writeable
    with pytest.raises(ValueError):
        a.planes[0, 0] = 1.0
    planes[0, 0] += 1e-9                                              # the caller's array is the caller's: the Profile holds a copy
    assert extraction.Profile(planes, rows).tag != a.tag and a.planes[0, 0] == b.planes[0, 0]
    assert extraction.Profile(b.planes, (4, 3, 5, 6)).tag != a.tag    # other heights, the same values: another profile
    # the first pass of a visit forms no optimal channels, whatever the options say
    opt = extraction.Optimal(8, channels=True)
    first = opt.with_profile(None, deliver_profile=True, channels=False)
    assert first.deliver_profile and not first.channels and opt.with_profile(a).channels and opt.with_profile(a).profile is a
