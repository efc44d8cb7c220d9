"""CPU: the optimal (profile-weighted) extraction -- properties of the law (tests/optimal_law.py) on hand-made planes, the
law against an ensemble of CPU-oracle exposures, the Python binding and the host-side argument check.  Device side:
tests/test_optimal_gpu.py."""
import ctypes as C
import io
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import extraction_law as law
import helpers
import optimal_law
from oracle import wayne_oracle as wo
from wayne_amd import _lib, extraction, run_visit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [(100, 140), (110, 150), (120, 160), (100, 160)]


def hand_made_planes(S=64, R=3, seed=5):
    """Planes as extraction_law.Planes holds them, made by hand: no non-linearity, no dark, a gain that varies from
    column to column (2.35 on the border) and a sky template that is constant along y."""
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


def restated(reads, pl, windows, bg, H, rn, steps=law.ALL):
    spectra, sky, spectra_var, sky_var = optimal_law.box(reads, pl, windows, bg, rn, steps)
    return optimal_law.restate(reads, pl, windows, H, rn, spectra, sky, spectra_var, sky_var, steps), spectra, spectra_var


def test_window_sum_is_the_clamped_ascending_sum():
    a = np.arange(1.0, 11.0)
    got = optimal_law.window_sum(a, 2)
    want = [sum(a[max(x - 2, 0):min(x + 2, 9) + 1]) for x in range(10)]
    assert got.tolist() == want
    # left to right: 1e16 + 1 + 1 loses both ones, 1 + 1 + 1e16 keeps them
    assert optimal_law.window_sum(np.array([1e16, 1.0, 1.0]), 1)[1] == 1e16
    assert optimal_law.window_sum(np.array([1.0, 1.0, 1e16]), 1)[1] == 1e16 + 2.0


def test_pure_noise_falls_back_to_the_box_values():
    S, R, rn = 64, 3, 20.0
    pl = hand_made_planes(S, R)
    rs = np.random.RandomState(3)
    reads = (1000.0 + rn / np.sqrt(2.0) / 2.35 * rs.standard_normal((R + 1, S, S))).astype(np.float64)   # no source anywhere
    windows = [(10, 20), (15, 30), (25, 50), (8, 55)]
    # ok(x) is a one-sided 3 sigma test: 0.135 % of pure-noise columns pass it by chance, in runs (neighbours share 2H
    # of their 2H + 1 columns).  Allowed: one run of 2H + 1 columns among the 4 x 64 -- 50 times the expected rate.  (The
    # sky step is off: a fitted sky level's error is common to all columns, yet enters SV0 column by column as if it were
    # independent, so with it a window of noise alone passes more often than 3 sigma says -- and still only falls back or
    # not, column by column.)
    got, spectra, spectra_var = restated(reads, pl, windows, (6, 16), 8, rn, steps=law.ALL & ~law.SKY)
    print("pure noise, sky off: %d of %d columns pass ok(x)" % (got.ok.sum(), got.ok.size))
    assert got.ok.sum() <= 17
    assert got.optimal[~got.ok].tobytes() == spectra[~got.ok].tobytes()
    assert got.optimal_var[~got.ok].tobytes() == spectra_var[~got.ok].tobytes()
    got, spectra, spectra_var = restated(reads, pl, windows, (6, 16), 8, rn)
    print("pure noise, sky fitted: %d of %d columns pass ok(x)" % (got.ok.sum(), got.ok.size))
    assert got.optimal[~got.ok].tobytes() == spectra[~got.ok].tobytes()
    assert got.optimal_var[~got.ok].tobytes() == spectra_var[~got.ok].tobytes()
    # without the chance: noise whose column sums are negative is no source at any threshold
    down = np.sort(reads, axis=0)[::-1].copy()
    got, spectra, spectra_var = restated(down, pl, windows, (6, 16), 8, rn, steps=law.ALL & ~law.SKY)
    assert (spectra < 0.0).all() and not got.ok.any()
    assert got.optimal.tobytes() == spectra.tobytes() and got.optimal_var.tobytes() == spectra_var.tobytes()


def top_hat(S, R, pl, lit=(24, 31), cols=(20, 50), flux=4000.0):
    """Noise-free reads whose only light is a top-hat along y on the rows `lit`, a smooth spectrum on the columns `cols`
    (the background columns stay dark, so the sky level is exactly 0)."""
    F = np.zeros(S)
    F[cols[0]:cols[1]] = flux * (1.0 + 0.3 * np.sin(np.arange(cols[1] - cols[0]) / 5.0))
    hat = np.zeros(S)
    hat[lit[0]:lit[1]] = 1.0
    return np.stack([1000.0 + r * hat[:, None] * F[None, :] for r in range(R + 1)])


def test_a_noise_free_top_hat_gives_the_box_sum():
    S, R, rn = 64, 3, 20.0
    pl = hand_made_planes(S, R)
    reads = top_hat(S, R, pl)
    windows = [(14, 41)] * (R + 1)                                         # 7 lit rows and 2 x 10 margin rows
    for H in (1, 8, 16):
        got, spectra, _ = restated(reads, pl, windows, (6, 16), H, rn)
        assert got.ok[:, 20:50].all() and not got.ok[:, :3].any() and (spectra[:, 20:50] > 1e4).all()
        assert np.abs(got.optimal - spectra).max() <= 1e-12 * spectra.max(), H
        # and its variance is that of the lit rows alone -- the margin rows carry no weight -- with the sky level's share
        q2 = (pl.gain[30] / 2.35) ** 2
        sky_var = optimal_law.box(reads, pl, windows, (6, 16), rn)[3]
        scale = np.append(pl.dt, pl.dt.sum())
        bt_lit = 7 * scale[:, None] * pl.sky[30][None, 20:50]
        want = spectra[:, 20:50] + 7 * rn * rn * q2[20:50] + bt_lit * bt_lit * sky_var[:, None]
        assert (sky_var > 0.0).all()
        assert np.allclose(got.optimal_var[:, 20:50], want, rtol=1e-12, atol=0.0), H


def test_doubling_the_read_noise_never_lowers_the_variance():
    S, R = 64, 3
    pl = hand_made_planes(S, R)
    y = np.arange(S, dtype=float)[:, None]
    F = 3000.0 * (1.0 + 0.3 * np.sin(np.arange(S) / 5.0))[None, :] * (np.abs(np.arange(S) - 35) < 15)
    ramp = np.exp(-0.5 * ((y - 28.0) / 3.0) ** 2) * F                    # a Gaussian profile along y
    reads = np.stack([1000.0 + r * ramp for r in range(R + 1)])
    windows = [(10, 45)] * (R + 1)
    one, _, box_one = restated(reads, pl, windows, (6, 16), 8, 10.0)
    two, _, box_two = restated(reads, pl, windows, (6, 16), 8, 20.0)
    assert one.ok.any() and (~one.ok).any()
    assert (two.optimal_var >= one.optimal_var).all()
    assert (two.optimal_var[one.ok & two.ok] > one.optimal_var[one.ok & two.ok]).all()
    # the point of it all: the weighted sum is less noisy than the box sum
    assert (one.optimal_var[one.ok] < box_one[one.ok]).all() and (two.optimal_var[two.ok] < box_two[two.ok]).all()


def test_assert_parity_bounds_and_the_fallback_bytes():
    S, R, rn = 64, 3, 20.0
    pl = hand_made_planes(S, R)
    reads = top_hat(S, R, pl)
    want, spectra, spectra_var = restated(reads, pl, [(14, 41)] * (R + 1), (6, 16), 8, rn)
    ok = want.ok
    optimal_law.assert_parity(want.optimal, want.optimal_var, want, spectra, spectra_var, "itself")
    inside = want.optimal + np.where(ok, 1e-9 * want.M_U / np.where(ok, want.W, 1.0), 0.0)
    optimal_law.assert_parity(inside, want.optimal_var * np.where(ok, 1.0 + 3e-9, 1.0), want, spectra, spectra_var, "inside")
    outside = want.optimal + np.where(ok, 3e-9 * want.M_U / np.where(ok, want.W, 1.0), 0.0)
    with pytest.raises(AssertionError):
        optimal_law.assert_parity(outside, want.optimal_var, want, spectra, spectra_var, "outside")
    with pytest.raises(AssertionError):
        optimal_law.assert_parity(want.optimal, want.optimal_var * np.where(ok, 1.0 + 5e-9, 1.0), want, spectra, spectra_var, "var outside")
    with pytest.raises(AssertionError):                                   # a fallback column must be the box value to the bit
        optimal_law.assert_parity(want.optimal + np.where(ok, 0.0, 1e-300), want.optimal_var, want, spectra, spectra_var, "fallback")


_ensemble = {}


def oracle_ensemble(n, H=8, rn=20.0):
    """n CPU-oracle exposures of small256 that differ in their draws alone (no cosmic rays, no scan-speed variation, no
    flat; the set-up of tests/test_variance.py::oracle_ensemble) -> dict of [n, R + 1, S] arrays by the numpy laws: the
    box spectra and their variances, the optimal extraction, and its renormalised and data-variance variants."""
    if (n, H, rn) in _ensemble:
        return _ensemble[(n, H, rn)]
    v = helpers.make_visit("small256")
    pl = law.Planes(v)
    S = pl.S
    eo = helpers.oracle_generator(v)
    kw = v.frame_kwargs(0, cosmic_rate=None, ssv_generator=None, add_flat=False)
    plan = extraction.ExtractionOptions().plan(v.grism, v.wl, kw["x_ref"], kw["y_ref"], kw["scan_speed"], v.read_times,
                                               507 - 128, S)
    out = {k: [] for k in ("spectra", "spectra_var", "optimal", "optimal_var", "renormalised", "data_variance")}
    for i in range(n):
        draws = wo.PhiloxDraws(v.seed, i, v.detector.light_sensitive_size(v.SUBARRAY))
        reads = np.stack(eo.scanning_frame(threads=2, draws=draws, thrower="oracle", **helpers.oracle_kwargs(kw)))
        box = optimal_law.box(reads, pl, plan.row_windows, plan.bg_cols, rn)
        got = optimal_law.restate(reads, pl, plan.row_windows, H, rn, *box)
        out["spectra"].append(box[0])
        out["spectra_var"].append(box[2])
        out["optimal"].append(got.optimal)
        out["optimal_var"].append(got.optimal_var)
        out["renormalised"].append(optimal_law.restate(reads, pl, plan.row_windows, H, rn, *box, renormalise=True).optimal)
        out["data_variance"].append(optimal_law.restate(reads, pl, plan.row_windows, H, rn, *box, data_variance=True).optimal)
    _ensemble[(n, H, rn)] = {k: np.array(a) for k, a in out.items()}
    return _ensemble[(n, H, rn)]


COLS = (59, 189)                                                           # columns 59 .. 188: inside the first order


def test_the_optimal_extraction_beats_the_box_on_cpu_oracle_reads():
    # 32 exposures that differ in their draws alone, H = 8, sums over 130 columns, the last-read product asserted:
    # 1. ensemble variance of optimal / box <= 0.8 -- a prototype on 48 exposures gave 0.656; the ratio of two such sums over
    #    130 columns x 31 degrees of freedom has a standard deviation of about 0.03;
    # 2. paired mean |sum(optimal - spectra)| / sum(spectra) <= 1e-3 -- the prototype gave +5e-4; the paired mean's standard
    #    deviation is sqrt((7.2 - 4.7)e6 / 32) / 2.69e6 ~ 1e-4, so the bound lies 5 of them above it -- and Horne's
    #    renormalised weights (+1.6e-3 in the prototype) must fail it;
    # 3. ensemble / predicted variance within 1 +- 4 sqrt(2 / (130 x 31)) = 1 +- 0.089 -- the prototype gave 1.011.
    # Every read interval's figures are printed, not asserted: on the nearly unlit interval 0 the predicted variance is too
    # small (the profile's own noise is not in 1 / W) -- the stated limit.
    n = 32
    e = oracle_ensemble(n)
    R = e["spectra"].shape[1] - 1
    sd = np.sqrt(2.0 / ((COLS[1] - COLS[0]) * (n - 1)))
    for p in list(range(R)) + [R]:
        ratio, bias, predicted = optimal_law.ensemble_figures(e["optimal"][:, p], e["optimal_var"][:, p], e["spectra"][:, p], COLS)
        _, bias_r, _ = optimal_law.ensemble_figures(e["renormalised"][:, p], e["optimal_var"][:, p], e["spectra"][:, p], COLS)
        _, bias_d, _ = optimal_law.ensemble_figures(e["data_variance"][:, p], e["optimal_var"][:, p], e["spectra"][:, p], COLS)
        box_var = e["spectra"][:, p, COLS[0]:COLS[1]].var(axis=0, ddof=1).sum()
        print("CPU oracle, %d exposures, %s: ensemble variance box %.4g, optimal / box %.3f; bias %+.2e (renormalised %+.2e, "
              "data variance %+.2e); ensemble / predicted variance %.3f" % (
                  n, "last read" if p == R else "interval %d" % p, box_var, ratio, bias, bias_r, bias_d, predicted))
    assert ratio <= 0.8
    assert abs(bias) <= 1e-3
    assert abs(bias_r) > 1e-3
    assert abs(predicted - 1.0) <= 4 * sd and abs(4 * sd - 0.089) < 1e-3


def test_optimal_is_validated_and_plans_carry_it():
    assert extraction.Optimal().half_width == 8
    assert extraction.Optimal(1).half_width == 1 and extraction.Optimal(16).half_width == 16
    for bad in (0, 17, -1, 8.5, float("nan"), True):
        with pytest.raises(ValueError):
            extraction.Optimal(bad)
    assert extraction.Optimal.coerce(None) is None and extraction.Optimal.coerce(False) is None
    assert extraction.Optimal.coerce(True).half_width == 8
    own = extraction.Optimal(5)
    assert extraction.Optimal.coerce(own) is own
    with pytest.raises(TypeError):
        extraction.Optimal.coerce(5)
    d = own.desc()
    assert isinstance(d, _lib.OptimalDesc) and d.half_width == 5
    # without variances it is an error, wherever it is asked for
    with pytest.raises(ValueError):
        extraction.Extraction(WINDOWS, optimal=True)
    with pytest.raises(ValueError):
        extraction.ExtractionOptions(optimal=True)
    plain = extraction.Extraction(WINDOWS, variance=True)
    with_opt = extraction.Extraction(WINDOWS, variance=True, optimal=own)
    assert plain.optimal is None and extraction.Extraction(WINDOWS, variance=True, optimal=False).optimal is None
    assert with_opt.optimal is own and bytes(plain.desc()) == bytes(with_opt.desc())
    # the other options keep it, and it keeps them; without the variances it goes too
    S = 266
    ch = extraction.Channels.linear(1.1, 1.7, 20)
    sol = (np.full(S, 0.9), np.full(S, 0.0046))
    full = extraction.Extraction(WINDOWS, crrej=True, channels=ch, row_solution=sol, variance=True, optimal=own)
    assert full.with_crrej(None).optimal is own and full.with_channels(None).optimal is own
    assert full.with_variance(extraction.Variances(5.0)).optimal is own
    gone = full.with_variance(None)
    assert gone.optimal is None and gone.variance is None and gone.channels is ch
    off = full.with_optimal(None)
    assert off.optimal is None and off.variance is full.variance and off.crrej is full.crrej and off.hull == full.hull
    opts = extraction.ExtractionOptions(variance=True, optimal=own)
    assert opts.optimal is own and extraction.ExtractionOptions(variance=True).optimal is None
    # the frame's optimal= replaces the plan's; without an extraction or without variances it is an error
    args = (None, None, 0.0, 0.0, 0.0, [1.0], 0, 266)
    assert extraction.for_exposure(plain, *args, optimal=True).optimal.half_width == 8
    assert extraction.for_exposure(extraction.Extraction(WINDOWS), *args, variance=True, optimal=own).optimal is own
    assert extraction.for_exposure(with_opt, *args).optimal is own
    assert extraction.for_exposure(with_opt, *args, optimal=False).optimal is None
    assert extraction.for_exposure(with_opt, *args, crrej=True).optimal is own
    assert extraction.for_exposure(None, *args, optimal=False) is None
    with pytest.raises(ValueError):
        extraction.for_exposure(None, *args, optimal=True)
    with pytest.raises(ValueError):
        extraction.for_exposure(extraction.Extraction(WINDOWS), *args, optimal=True)
    dropped = extraction.for_exposure(with_opt, *args, variance=False)          # what clears the variances clears it too
    assert dropped.variance is None and dropped.optimal is None


def test_optimal_struct_mirrors_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wayne_hip.h"\n'
                   'int main(void) {\n  printf("%zu %zu %d\\n", sizeof(wayne_optimal_desc), offsetof(wayne_optimal_desc, half_width),\n'
                   '         WAYNE_MAX_OPTIMAL_HALF_WIDTH);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True)
    size, off, cap = (int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(_lib.OptimalDesc) == 4 and off == _lib.OptimalDesc.half_width.offset == 0
    assert cap == _lib.MAX_OPTIMAL_HALF_WIDTH == 16
    for name in ("wayne_exposure_set_optimal", "wayne_exposure_optimal"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 7


HARNESS = r"""
#include <climits>
#include <cstdio>
#include "host_plan.h"
using namespace wayne;
int main() {
  int bad = 0;
  auto expect = [&](bool ok, int H, const char* what) {
    const char* why = plan::optimal_desc_error(H);
    if ((why == nullptr) != ok) { std::printf("WRONG %s: %s\n", what, why ? why : "accepted"); ++bad; }
  };
  expect(true, 8, "default");
  expect(true, 1, "narrowest");
  expect(true, 16, "widest");
  expect(true, kOptMaxH, "kOptMaxH");
  expect(false, 0, "zero");
  expect(false, 17, "beyond the halo");
  expect(false, -1, "negative");
  expect(false, INT_MAX, "INT_MAX");
  expect(false, INT_MIN, "INT_MIN");
  std::printf("checked\n");
  return bad ? 1 : 0;
}
"""


def test_optimal_desc_error_in_a_program_of_its_own(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "optimal_plan.cpp"
    src.write_text(HARNESS)
    exe = str(tmp_path / "optimal_plan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "wayne_amd", "csrc"), str(src), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checked" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr


def test_npz_keys_with_and_without_the_optimal_extraction():
    S, R, n = 266, 3, 2
    base = ["spectra", "sky", "exposure_index", "row_lo", "row_hi", "bg_cols", "x_ref", "y_ref", "read_times", "exp_start"]
    var = ["spectra_var", "sky_var", "variance_read_noise"]
    args = (np.zeros((n, R + 1, S)), np.zeros((n, R + 1)), [0, 1])
    more = ([1.0, 2.0], [3.0, 4.0], [1.0, 2.0, 3.0], [0.0, 9.0])
    sv = np.arange(n * (R + 1) * S, dtype=float).reshape(n, R + 1, S)
    kv = np.arange(n * (R + 1), dtype=float).reshape(n, R + 1)
    op, ov = sv + 0.5, sv + 0.25

    def keys(plan, **kw):
        f = io.BytesIO()
        extraction.save_npz(f, *args, [plan] * n, *more, **kw)
        f.seek(0)
        return np.load(f)

    plan = extraction.Extraction(WINDOWS, variance=True, optimal=extraction.Optimal(5))
    assert sorted(keys(plan).files) == sorted(base)                        # on, but nothing was delivered
    assert sorted(keys(plan, variances=(sv, kv, None)).files) == sorted(base + var)
    z = keys(plan, variances=(sv, kv, None), optimal=(op, ov))
    assert sorted(z.files) == sorted(base + var + ["optimal", "optimal_var", "optimal_half_width"])
    assert z["optimal"].tobytes() == op.tobytes() and z["optimal_var"].tobytes() == ov.tobytes()
    assert z["optimal"].shape == (n, R + 1, S) and int(z["optimal_half_width"]) == 5
    assert sorted(keys(plan.with_optimal(None), variances=(sv, kv, None)).files) == sorted(base + var)


def test_cli_argument_errors():
    yml = os.path.join(ROOT, "tests", "fixtures", "mini_visit", "params.yml")
    for argv in (["--optimal"], ["--optimal", "4"], ["--spectra-only", "x.npz", "--optimal"]):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml] + argv)
        assert "--optimal needs --variances" in str(e.value)
    for H in ("0", "17", "-2"):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml, "--spectra-only", "x.npz", "--variances", "--optimal=" + H])
        assert "[H]" in str(e.value) and "half_width must lie in 1 .. 16" in str(e.value)


def test_algorithmic_bytes_count_the_second_walk():
    S, R = 266, 3
    plan = extraction.Extraction(WINDOWS, variance=True, optimal=True)
    base = extraction.algorithmic_bytes(plan, S, R, variance=True)
    assert extraction.algorithmic_bytes(plan, S, R, variance=True, optimal=False) == base
    chunks = 2 + 2 + 2 + 2
    # per window pixel the planes k_extract_rows reads, once more: float32 reads P_hi, (P_lo,) P_0, four coefficients, dark_hi
    # (, dark_lo), the pixel flat, the sky -- 36 bytes for the first interval and the last read, 44 for the others
    planes = 40 * S * (36 + 44 + 44) + 60 * S * 36
    sums = 2 * 3 * chunks * S * 8
    results = 2 * (R + 1) * S * 8
    assert extraction.algorithmic_bytes(plan, S, R, variance=True, optimal=True) - base == planes + sums + results
    # under rejection the flag word (2 bytes) of every window pixel is read again too
    cr = extraction.algorithmic_bytes(plan, S, R, crrej=True, variance=True)
    assert (extraction.algorithmic_bytes(plan, S, R, crrej=True, variance=True, optimal=True) - cr ==
            planes + (3 * 40 + 60) * S * 2 + sums + results)
    # 16-bit reads: 2 bytes a sample in place of 4
    assert (extraction.algorithmic_bytes(plan, S, R, read_bytes=2, variance=True, optimal=True) -
            extraction.algorithmic_bytes(plan, S, R, read_bytes=2, variance=True) ==
            planes - 40 * S * (2 * 2 + 3 * 2 + 3 * 2) - 60 * S * 2 * 2 + sums + results)
