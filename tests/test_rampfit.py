"""CPU: the ramp fit -- properties of the law (tests/rampfit_law.py) on hand-made ramps, the law against synthetic
ensembles and against CPU-oracle staring exposures (cosmic rays on against off, saturation, the noise of an ensemble), the
Python binding, the host-side argument check, the refusals and the FITS file.  Device side: tests/test_rampfit_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import extraction_law
import helpers
import rampfit_law as law
from oracle import wayne_oracle as wo
from wayne_amd import _lib, exposure, fitsio, rampfit, run_visit, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = np.array([2.9] + [7.35] * 14)
RN = 20.0


def ramps(rate, n, rs, dt=DT, rn=RN):
    """d [R, n]: Poisson electrons of every interval plus the noise of the R + 1 reads (rn: of a difference of two)."""
    e = np.concatenate([np.zeros((1, n)), np.cumsum(rs.poisson(rate * dt[:, None], (dt.size, n)), axis=0)])
    e = e + rs.standard_normal(e.shape) * (rn / np.sqrt(2.0))
    return np.diff(e, axis=0)


def hand_made_planes(S, dt):
    pl = types.SimpleNamespace(S=S)
    pl.lin = [np.zeros((S, S)) for _ in range(4)]
    pl.dark = np.zeros((len(dt) + 1, S, S))
    pl.gain = np.full((S, S), 2.35)
    pl.dt = np.asarray(dt, dtype=float)
    return pl


# ---- the law itself -------------------------------------------------------------------------------------------------
def test_the_recurrence_is_the_solution_of_the_sub_matrix():
    rs = np.random.RandomState(3)
    worst = 0.0
    for trial in range(200):
        R = rs.randint(1, 16)
        dt = rs.uniform(0.1, 10.0, R)
        G = rs.random_sample(R) < 0.7
        if not G.any():
            G[rs.randint(R)] = True
        d = rs.normal(50.0, 30.0, R)
        f0, rn = rs.uniform(0.0, 500.0), rs.uniform(5.0, 40.0)
        num, den, w = law.solve(d[:, None], dt, G[:, None], np.array([f0]), rn)
        idx = np.flatnonzero(G)
        Cm = np.diag(f0 * dt[idx] + rn * rn)
        for a in range(idx.size - 1):
            if idx[a + 1] == idx[a] + 1:
                Cm[a, a + 1] = Cm[a + 1, a] = -rn * rn / 2
        ww = np.linalg.solve(Cm, dt[idx])
        want_den, want_num = ww @ dt[idx], ww @ d[idx]
        assert abs(den[0] - want_den) <= 1e-12 * abs(want_den)
        scale = np.abs(ww * d[idx]).sum()
        assert abs(num[0] - want_num) <= 1e-12 * scale
        worst = max(worst, abs(den[0] - want_den) / abs(want_den), abs(num[0] - want_num) / scale)
        assert not w[~G, 0].any()
    print("recurrence against np.linalg.solve: worst relative difference %.3g" % worst)


def test_a_noiseless_linear_ramp_gives_its_rate_and_no_flag():
    rate = np.array([0.0, 0.3, 7.0, 1234.5])
    d = rate[None, :] * DT[:, None]
    f = law.fit(d, DT, np.full(rate.size, DT.size))
    assert np.allclose(f.rate, rate, rtol=1e-13, atol=1e-13) and not f.jump.any()
    assert (f.word == np.uint32(15 << 16)).all() and (f.var > 0).all()
    # the variance of a brighter pixel is larger, and that of the dark one is the read noise's alone
    assert (np.diff(f.var) > 0).all()


def test_one_jump_is_flagged_and_the_rate_restored():
    d = 40.0 * DT[:, None] * np.ones((1, 15))
    for j in range(15):
        d[j, j] += 3000.0
    f = law.fit(d, DT, np.full(15, 15))
    assert (f.jump == (np.uint32(1) << np.arange(15).astype(np.uint32))).all()
    assert np.allclose(f.rate, 40.0, rtol=1e-13)
    off = law.fit(d, DT, np.full(15, 15), k_jump=0.0)
    assert not off.jump.any() and (off.rate > 41.0).all() and np.isinf(off.margin).all()


def test_two_jumps_in_one_pixel():
    d = 40.0 * DT[:, None] * np.ones((1, 2))
    d[3, 0] += 5000.0; d[11, 0] += 900.0
    d[0, 1] += 700.0; d[1, 1] += 700.0                 # neighbours: both removed, the chain cut twice
    f = law.fit(d, DT, np.array([15, 15]))
    assert f.jump[0] == (1 << 3 | 1 << 11) and f.jump[1] == 3
    assert np.allclose(f.rate, 40.0, rtol=1e-13)
    dq, nsamp, time = law.derived(f.word, DT)
    assert (dq == 8192).all() and (nsamp == 13).all()
    assert np.isclose(time[0], DT.sum() - DT[3] - DT[11]) and np.isclose(time[1], DT.sum() - DT[0] - DT[1])


def test_fewer_than_three_intervals_are_never_tested():
    d = np.array([[10.0, 10.0, 10.0], [1e6, 1e6, 1e6], [10.0, 10.0, 10.0]]) * np.ones((3, 3))
    f = law.fit(d, DT[:3], np.array([1, 2, 3]))
    assert f.jump[0] == 0 and f.jump[1] == 0 and f.jump[2] == 2
    assert np.isinf(f.margin[:2]).all() and np.isfinite(f.margin[2])
    # ... and a pixel that is down to two intervals is not tested again
    d4 = np.array([10.0, 1e6, 2e4, 10.0])[:, None]
    f4 = law.fit(d4, DT[:4], np.array([4]))
    assert f4.jump[0] == 2 | 4                                            # 4 -> 3 -> 2 intervals: two passes, both hit
    d3 = np.array([10.0, 1e6, 2e4])[:, None]
    assert law.fit(d3, DT[:3], np.array([3])).jump[0] == 2                # 3 -> 2 intervals: the second jump stays


def test_saturation_cuts_the_ramp_and_a_nan_counts_as_saturated():
    S, R = 16, 6
    dt = DT[:R]
    pl = hand_made_planes(S, dt)
    t = np.concatenate([[0.0], np.cumsum(dt)])
    reads = (1000.0 + 100.0 * t[:, None, None] * np.ones((1, S, S))).astype(np.float64)
    reads[4, 6, 6] = 70000.0                       # K = 3
    reads[2, 7, 7] = np.nan                        # K = 1
    reads[0, 8, 8] = 66000.0                       # K = 0
    reads[1, 9, 9] = 65000.0                       # not < sat_dn: K = 0
    reads[6, 10, 10] = 64999.0                     # a jump, but no saturation
    reads[3, 5, 5] = 70000.0; reads[4:, 5, 5] = 100.0    # samples behind a saturated one are not used again
    f = law.restate(reads, pl)
    K = f.word >> 16
    assert K[6, 6] == 3 and K[7, 7] == 1 and K[8, 8] == 0 and K[9, 9] == 0 and K[10, 10] == R and K[5, 5] == 2
    assert K[6, 7] == R
    for y, x in ((6, 6), (7, 7), (5, 5), (6, 7)):
        assert np.isclose(f.rate[y, x], 235.0, rtol=1e-12), (y, x)
    assert f.rate[8, 8] == 0.0 and f.var[8, 8] == 0.0 and f.word[8, 8] == 0
    assert f.var[7, 7] > f.var[6, 6] > f.var[6, 7] > 0
    dq, nsamp, time = law.derived(f.word, dt)
    assert dq[6, 6] == 256 and dq[6, 7] == 0 and nsamp[6, 6] == 3 and np.isclose(time[6, 6], dt[:3].sum())
    assert dq[10, 10] == 8192 and nsamp[10, 10] == R - 1
    # the border is zero, whatever the reads hold
    border = np.ones((S, S), dtype=bool)
    border[5:-5, 5:-5] = False
    assert not f.rate[border].any() and not f.var[border].any() and not f.word[border].any()
    # the product's derivation is the law's
    got = rampfit.derive(f.word, dt)
    assert all((a == b).all() for a, b in zip(got, (dq, nsamp, time)))


def test_the_lower_median_is_taken():
    r = np.array([[4.0], [1.0], [3.0], [2.0]])
    G = np.ones((4, 1), dtype=bool)
    assert law.lower_median(r, G)[0] == 2.0                               # of 1 2 3 4: the lower of the middle two
    G[1] = False
    assert law.lower_median(r, G)[0] == 3.0                               # of 2 3 4
    G[:] = False
    assert law.lower_median(r, G)[0] == 0.0
    ties = np.array([[5.0], [5.0], [5.0], [7.0]])
    assert law.lower_median(ties, np.ones((4, 1), dtype=bool))[0] == 5.0
    # the upper median would fit another f0: the variance tells them apart
    d = np.array([10.0, 20.0, 3000.0, 4000.0])[:, None]
    dt = np.ones(4)
    f = law.fit(d, dt, np.array([4]), k_jump=0.0)
    _, den, _ = law.solve(d, dt, np.ones((4, 1), dtype=bool), np.array([20.0]), RN)
    _, den_upper, _ = law.solve(d, dt, np.ones((4, 1), dtype=bool), np.array([3000.0]), RN)
    assert f.var[0] == 1.0 / den[0] and f.var[0] != 1.0 / den_upper[0]


def test_the_variance_describes_a_synthetic_ensemble():
    # n ramps per rate: (n - 1) s^2 / sigma^2 is chi-square with n - 1 degrees of freedom, so the ratio of the ensemble's
    # variance to the mean predicted one has standard deviation sqrt(2 / (n - 1)) -- derived, not measured.  A prototype
    # with n = 2e5 gave 1.001, 0.999, 0.999, 1.000 at rates 5, 50, 500, 5000, 0.97 at 0.5 and 0.83 at 0: max(med, 0) of pure
    # noise is biased upward (the stated limit), so rate 0 is reported, not asserted.
    n = 20000
    rs = np.random.RandomState(11)
    bound = 4 * np.sqrt(2.0 / (n - 1))
    flagged = 0
    for rate in (0.0, 5.0, 50.0, 500.0, 5000.0):
        d = ramps(rate, n, rs)
        f = law.fit(d, DT, np.full(n, 15))
        ratio = f.rate.var(ddof=1) / f.var.mean()
        end_to_end = (d.sum(axis=0) / DT.sum()).var(ddof=1)
        flagged += int((f.jump != 0).sum())
        print("rate %6.1f e-/s: ensemble / predicted variance %.4f (allowed 1 +- %.4f), variance / end-to-end difference's %.3f, "
              "mean %.4f, %d of %d flagged" % (rate, ratio, bound, f.rate.var(ddof=1) / end_to_end, f.rate.mean(), int((f.jump != 0).sum()), n))
        if rate > 0:
            assert abs(ratio - 1.0) <= bound, rate
            assert abs(f.rate.mean() - rate) <= 5 * np.sqrt(f.var.mean() / n)
    assert flagged <= 1e-3 * 5 * n                 # (the prototype: 3e-5 of the pixels at k = 5)


def test_assert_parity_holds_what_it_says():
    rs = np.random.RandomState(2)
    S, R = 120, 8
    pl = hand_made_planes(S, DT[:R])
    e = np.concatenate([np.zeros((1, S, S)), np.cumsum(rs.poisson(40.0 * DT[:R, None, None] * np.ones((1, S, S))), axis=0)]) + rs.normal(0, 14.0, (R + 1, S, S))
    reads = (5000.0 + e / 2.35)
    reads[5:, 8, 8] += 2000.0                                             # a ray
    reads[6:, 9, 9] = 70000.0                                             # saturation
    want = law.restate(reads, pl)
    assert want.jump[8, 8] == 1 << 4 and want.word[9, 9] >> 16 == 5
    law.assert_parity(want.rate.copy(), want.var.copy(), want.word.copy(), want, "itself")
    law.assert_parity(want.rate + 5e-10 * want.M, want.var * (1 + 2e-9), want.word.copy(), want, "inside")
    for rate, var, word in ((want.rate + 2e-9 * want.M, want.var, want.word), (want.rate, want.var * (1 + 8e-9), want.word),
                            (want.rate, want.var, want.word ^ np.uint32(1 << 3)), (want.rate + 1e-30, want.var, want.word),
                            (want.rate.astype(np.float32).astype(np.float64), want.var, want.word)):
        with pytest.raises(AssertionError):
            law.assert_parity(rate.copy(), var.copy(), word.copy(), want, "outside")
    # a pixel whose deciding z lies at the threshold is left out, and counted
    near = want._replace(margin=np.where(np.arange(S * S).reshape(S, S) == 8 * S + 8, 1e-12, want.margin))
    flipped = want.word.copy()
    flipped[8, 8] = R << 16
    assert law.assert_parity(want.rate.copy(), want.var.copy(), flipped, near, "undecided")[0] == 1
    with pytest.raises(AssertionError):
        law.assert_parity(want.rate.copy(), want.var.copy(), flipped, want, "decided")


# ---- CPU-oracle reads ------------------------------------------------------------------------------------------------
_oracle = {}


def oracle_reads(E, cosmic, i=0, **over):
    key = (E, cosmic, i, tuple(sorted(over.items())))
    if key not in _oracle:
        v = helpers.make_visit("stare16_128", E=E)
        eo = helpers.oracle_generator(v)
        kw = v.frame_kwargs(0, cosmic_rate=11.0 if cosmic else None, ssv_generator=None, **over)
        draws = wo.PhiloxDraws(v.seed, i, v.detector.light_sensitive_size(v.SUBARRAY))
        reads = np.stack(eo.scanning_frame(threads=2, draws=draws, thrower="oracle", **helpers.oracle_kwargs(kw)))
        _oracle[key] = (v, reads)
    return _oracle[key]


def test_stare16_128_is_the_configuration_the_issue_names():
    assert synthetic.CONFIGS["stare16_128"] == dict(grism="G141", SUBARRAY=128, SAMPSEQ="SPARS10", NSAMP=16, K=15, E=2e7,
                                                    scan_speed=0.0, x_ref=400.0, y_ref=470.0, n_wl=900)
    v = helpers.make_visit("stare16_128")
    dt = np.diff(np.concatenate([[0.0], v.read_times]))
    assert dt.size == 15 and abs(dt[0] - 0.113) < 1e-3 and np.allclose(dt[1:], 7.18, atol=0.01)


def test_cosmic_rays_of_an_oracle_exposure_are_flagged():
    # The same draws with cosmic rays on and off (the oracle's streams are keyed by stage): the truth is the difference.
    v, on = oracle_reads(2e7, True)
    _, off = oracle_reads(2e7, False)
    pl = extraction_law.Planes(v)
    R = on.shape[0] - 1
    f_on, f_off = law.restate(on, pl), law.restate(off, pl)
    hit = np.diff(law.electrons(on, pl) - law.electrons(off, pl), axis=0)        # electrons a ray added per interval
    K = (f_on.word >> 16).astype(np.int64)
    usable = np.arange(R)[:, None, None] < K[None]
    inner = np.zeros(K.shape, dtype=bool)
    inner[5:-5, 5:-5] = True
    big = (hit > 150.0) & usable & inner[None]
    flagged = ((f_on.jump[None] >> np.arange(R, dtype=np.uint32)[:, None, None]) & 1).astype(bool)
    n_pix = int(inner.sum())
    false_off = int((f_off.jump != 0).sum())
    sigma = np.sqrt(f_off.var)
    ok = inner & (f_off.var > 0) & (K == R)
    with_rej = np.sqrt(np.mean(((f_on.rate - f_off.rate)[ok] / sigma[ok]) ** 2))
    no_rej = law.restate(on, pl, k_jump=0.0)
    without = np.sqrt(np.mean(((no_rej.rate - f_off.rate)[ok] / sigma[ok]) ** 2))
    print("stare16_128, E = 2e7: %d hits above 150 e- on usable intervals, %d flagged; %d of %d pixels flagged with rays off; "
          "rate with rays and rejection minus rate without rays: rms %.3f sigma (without the jump test %.1f sigma)" % (
              int(big.sum()), int((big & flagged).sum()), false_off, n_pix, with_rej, without))
    assert big.sum() >= 5                          # (the comparison is not one of nothing)
    assert (flagged[big]).all()
    assert false_off <= 1e-3 * n_pix               # a cap, not a measurement (the prototype saw 1.2e-4)
    assert with_rej < 1.0 < without


def test_a_bright_star_saturates_and_the_ramp_is_cut():
    v, reads = oracle_reads(1.2e8, False)
    f = law.restate(reads, extraction_law.Planes(v))
    K = (f.word >> 16)[5:-5, 5:-5]
    R = reads.shape[0] - 1
    cut = K < R
    print("stare16_128, E = 1.2e8: %d pixels with K < R, %d with K = 0, the brightest keeps %d intervals at %.0f e-/s" % (
        int(cut.sum()), int((K == 0).sum()), int(K[cut].min()) if cut.any() else R, float(f.rate.max())))
    assert cut.sum() >= 100
    assert np.isfinite(f.rate).all() and (f.var[5:-5, 5:-5][K > 0] > 0).all()


def oracle_ensemble_ratio(n, rn):
    """n CPU-oracle exposures of stare16_128 that differ in their draws alone (no cosmic rays): for every pixel whose
    ensemble mean rate is >= 5 e-/s the ensemble variance of the fitted rate over the pixel's mean predicted variance;
    -> (the mean of those ratios, the pixels)."""
    rates, variances = [], []
    for i in range(n):
        v, reads = oracle_reads(2e7, False, i)
        f = law.restate(reads, extraction_law.Planes(v), rn=rn)
        rates.append(f.rate); variances.append(f.var)
    return law.ensemble_ratio(np.array(rates), np.array(variances))


def test_the_variance_describes_the_cpu_oracles_noise():
    # The device test's ensemble (tests/test_rampfit_gpu.py) at half its size on CPU-oracle reads, every noise source on
    # (pointing jitter included).  A pixel's (n - 1) s^2 / sigma^2 is chi-square with n - 1 degrees of freedom, so the mean
    # of the pixels' ratios has standard deviation sqrt(2 / (n_pix (n - 1))) -- derived, not measured; the ratio is taken
    # pixel by pixel because that is what this bound holds for (a ratio of sums would be carried by the hundred brightest
    # pixels, whose variance is a thousand times the sky's, and have their few degrees of freedom).
    n = 16
    ratio, n_pix = oracle_ensemble_ratio(n, RN)
    control, _ = oracle_ensemble_ratio(n, 1e-3)
    bound = 4 * np.sqrt(2.0 / (n_pix * (n - 1)))
    print("CPU oracle, %d exposures of stare16_128, %d pixels at >= 5 e-/s: ensemble / predicted variance %.4f (allowed 1 +- %.4f); "
          "with read_noise = 0.001: %.3f" % (n, n_pix, ratio, bound, control))
    assert n_pix >= 100
    assert abs(ratio - 1.0) <= bound
    assert abs(control - 1.0) > bound


# ---- the binding, the validator, the refusals ------------------------------------------------------------------------
def test_rampfit_struct_mirrors_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    fields = [f[0] for f in _lib.RampFitDesc._fields_]
    assert fields == ["steps", "read_noise_e", "k_jump", "saturation_dn"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wayne_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(wayne_rampfit_desc));\n' +
                   "".join('  printf(" %%zu", offsetof(wayne_rampfit_desc, %s));\n' % f for f in fields) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True)
    got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.RampFitDesc) == 32
    assert got[1:] == [getattr(_lib.RampFitDesc, f).offset for f in fields] == [0, 8, 16, 24]
    header = open(os.path.join(ROOT, "include", "wayne_hip.h")).read()
    for name in ("wayne_exposure_set_rampfit", "wayne_exposure_download_rampfit", "wayne_rampfit_profile"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name) and ("int %s(" % name) in header
    assert _lib.ABI_VERSION == 7 and "#define WAYNE_ABI_VERSION 7" in header


HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include "host_plan.h"
using namespace wayne;
int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const unsigned three = X_LINEARISE | X_DARK | X_GAIN;
  int bad = 0;
  auto expect = [&](bool ok, unsigned steps, double rn, double k, double sat, const char* what) {
    const char* why = plan::rampfit_desc_error(steps, rn, k, sat);
    if ((why == nullptr) != ok) { std::printf("WRONG %s: %s\n", what, why ? why : "accepted"); ++bad; }
  };
  expect(true, three, 20.0, 5.0, 65000.0, "defaults");
  expect(true, X_GAIN, 1e-3, 0.0, 1.0, "gain alone, k 0");
  expect(true, X_GAIN | X_DARK, 20.0, 4.0, 1e9, "dark, no linearise");
  expect(false, X_LINEARISE | X_DARK, 20.0, 5.0, 65000.0, "gain off");
  expect(false, 0u, 20.0, 5.0, 65000.0, "no step");
  expect(false, three | X_SKY, 20.0, 5.0, 65000.0, "sky bit");
  expect(false, three | X_LAST_READ, 20.0, 5.0, 65000.0, "last-read bit");
  expect(false, three | (1u << 31), 20.0, 5.0, 65000.0, "high bit");
  expect(false, three, 0.0, 5.0, 65000.0, "rn 0");
  expect(false, three, -1.0, 5.0, 65000.0, "rn negative");
  expect(false, three, nan, 5.0, 65000.0, "rn nan");
  expect(false, three, inf, 5.0, 65000.0, "rn inf");
  expect(false, three, 20.0, -1.0, 65000.0, "k negative");
  expect(false, three, 20.0, nan, 65000.0, "k nan");
  expect(false, three, 20.0, inf, 65000.0, "k inf");
  expect(false, three, 20.0, 5.0, 0.0, "sat 0");
  expect(false, three, 20.0, 5.0, -5.0, "sat negative");
  expect(false, three, 20.0, 5.0, nan, "sat nan");
  expect(false, three, 20.0, 5.0, inf, "sat inf");
  expect(false, three, 20.0, 5.0, -inf, "sat -inf");
  std::printf("checked\n");
  return bad ? 1 : 0;
}
"""


def test_rampfit_desc_error_in_a_program_of_its_own(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "rampfit_plan.cpp"
    src.write_text(HARNESS)
    exe = str(tmp_path / "rampfit_plan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "wayne_amd", "csrc"), str(src), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checked" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr


def test_ramp_fits_are_validated_and_descriptors_carry_them():
    d = rampfit.RampFit()
    assert (d.read_noise, d.k, d.saturation_dn, d.linearise, d.dark) == (20.0, 5.0, 65000.0, True, True)
    assert d.steps == 7 and rampfit.RampFit(linearise=False).steps == 6 and rampfit.RampFit(dark=False).steps == 5
    c = rampfit.RampFit(13.0, 0.0, 3e4).desc()
    assert isinstance(c, _lib.RampFitDesc) and (c.steps, c.read_noise_e, c.k_jump, c.saturation_dn) == (7, 13.0, 0.0, 3e4)
    for bad in (dict(read_noise=0.0), dict(read_noise=-1.0), dict(read_noise=float("nan")), dict(read_noise=float("inf")),
                dict(k=-1.0), dict(k=float("nan")), dict(k=float("inf")), dict(saturation_dn=0.0),
                dict(saturation_dn=-3.0), dict(saturation_dn=float("nan")), dict(saturation_dn=float("inf"))):
        with pytest.raises(ValueError):
            rampfit.RampFit(**bad)
    assert rampfit.as_ramp_fit(None) is None and rampfit.as_ramp_fit(False) is None
    assert rampfit.as_ramp_fit(True).k == 5.0 and rampfit.as_ramp_fit(d) is d and rampfit.as_ramp_fit(4.0).k == 4.0
    with pytest.raises(TypeError):
        rampfit.as_ramp_fit("yes")
    # the descriptor carries it beside the C struct, whose bytes stay as they are
    v = helpers.make_visit("tiny")
    gen = helpers.product_generator(v, 0)
    plain = gen.build_descriptor(None, **v.frame_kwargs(0))
    asked = gen.build_descriptor(None, ramp_fit=True, **v.frame_kwargs(0))
    own = gen.build_descriptor(None, ramp_fit=d, **v.frame_kwargs(0))
    assert plain._ramp_fit is None and asked._ramp_fit.k == 5.0 and own._ramp_fit is d
    with pytest.raises(TypeError):
        gen.build_descriptor(None, ramp_fit="yes", **v.frame_kwargs(0))
    assert rampfit.rate_filename("0007_raw.fits") == "0007_rate.fits" and rampfit.rate_filename("x.fits") == "x_rate.fits"


def test_refusals():
    rampfit.refuse_combinations(None, resume=True, device_fits=True, spectra_only=True)      # nothing asked: nothing refused
    rampfit.refuse_combinations(True)
    for what in ("resume", "device_fits", "spectra_only"):
        with pytest.raises(ValueError) as e:
            rampfit.refuse_combinations(True, **{what: True})
        assert "ramp_fit: not together with " + what in str(e.value)


def test_cli_argument_errors():
    yml = os.path.join(ROOT, "tests", "fixtures", "mini_visit", "params.yml")
    for k in ("-3", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml, "--rate-images=" + k])
        assert "--rate-images [K]" in str(e.value) and "k must be" in str(e.value)
    with pytest.raises(SystemExit):
        run_visit.run(["-p", yml, "--rate-images", "many"])
    for other, what in ((["--resume"], "resume"), (["--device-fits"], "device_fits"), (["--spectra-only", "x.npz"], "spectra_only")):
        with pytest.raises(ValueError) as e:
            run_visit.run(["-p", yml, "--rate-images"] + other)
        assert "ramp_fit: not together with " + what in str(e.value)


def test_the_rate_file_reads_back(tmp_path):
    v = helpers.make_visit("tiny")
    gen = helpers.product_generator(v, 0)
    gen.build_descriptor(None, **v.frame_kwargs(0))
    frame = gen.exposure
    S, dt = 74, np.array([1.0, 2.0, 3.0])
    rs = np.random.RandomState(5)
    rate, var = rs.normal(50.0, 5.0, (S, S)), rs.uniform(1.0, 2.0, (S, S))
    word = np.full((S, S), 3 << 16, dtype=np.uint32)
    word[10, 10] = 2 << 16
    word[11, 11] = 3 << 16 | 2
    word[12, 12] = 1 << 16 | 1
    fit = rampfit.RampFit(read_noise=17.0, k=4.5, saturation_dn=6e4)
    with pytest.raises(ValueError):
        rampfit.write_fits(str(tmp_path / "none_rate.fits"), frame, fit)                # no planes on the exposure yet
    rampfit.fill_exposure(frame, (rate, var, word), dt)
    assert frame.rate is rate and frame.rate_var is var and frame.rate_word is word
    assert frame.rate_dq[10, 10] == 256 and frame.rate_dq[11, 11] == 8192 and frame.rate_dq[12, 12] == 256 | 8192 and frame.rate_dq[0, 0] == 0
    assert frame.rate_nsamp[10, 10] == 2 and frame.rate_nsamp[11, 11] == 2 and frame.rate_nsamp[12, 12] == 0 and frame.rate_nsamp[0, 0] == 3
    assert frame.rate_time[11, 11] == 4.0 and frame.rate_time[0, 0] == 6.0 and frame.rate_time[12, 12] == 0.0
    path = rampfit.write_fits(str(tmp_path / "0001_rate.fits"), frame, fit)
    hdus = fitsio.read(path)
    assert [h.header.get("EXTNAME") for h in hdus[1:]] == ["SCI", "ERR", "DQ", "SAMP", "TIME"]
    assert [h.header["BITPIX"] for h in hdus[1:]] == [-32, -32, 16, 16, -32]
    assert all(h.header["EXTVER"] == 1 for h in hdus[1:])
    p = hdus[0].header
    assert p["RFRN"] == 17.0 and p["RFK"] == 4.5 and p["RFSAT"] == 6e4
    raw = dict((k, val) for k, val, _ in frame.generate_science_header().cards if k)
    for key in ("TELESCOP", "INSTRUME", "FILTER", "SUBARRAY", "NSAMP"):
        if key in raw:
            assert p[key] == raw[key], key
    assert (hdus[1].data == rate.astype(np.float32)).all() and (hdus[2].data == np.sqrt(var).astype(np.float32)).all()
    assert (hdus[3].data == frame.rate_dq).all() and (hdus[4].data == frame.rate_nsamp).all()
    assert (hdus[5].data == frame.rate_time.astype(np.float32)).all()
    assert isinstance(frame, exposure.Exposure) and exposure.Exposure().rate is None
