"""CPU: variances of the device-side extraction -- properties of the law (tests/variance_law.py) on hand-made planes,
the law against an ensemble of CPU-oracle exposures, the Python binding and the host-side argument check.  Device side:
tests/test_variance_gpu.py."""
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
import helpers
import variance_law
from oracle import wayne_oracle as wo
from wayne_amd import _lib, extraction, run_visit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [(100, 140), (110, 150), (120, 160), (100, 160)]


def hand_made_planes(S=64, R=3, seed=5):
    """Planes as extraction_law.Planes holds them, made by hand: no non-linearity, no dark, a gain that varies from
    pixel to pixel (2.35 on the border) and a sky template that is constant along y."""
    rs = np.random.RandomState(seed)
    pl = types.SimpleNamespace(S=S)
    pl.lin = [np.zeros((S, S)) for _ in range(4)]
    pl.dark = np.zeros((R + 1, S, S))
    pl.gain = np.full((S, S), 2.35)
    pl.gain[5:-5, 5:-5] = 2.35 / (1.0 + 0.05 * rs.standard_normal((1, S - 10)) * np.ones((S - 10, 1)))   # constant along y
    pl.sky = np.zeros((S, S))
    pl.sky[5:-5, 5:-5] = 1.0 + 0.1 * rs.random_sample((1, S - 10)) * np.ones((S - 10, 1))
    pl.dt = np.array([10.0, 12.0, 14.0])[:R]
    return pl


def test_zero_flux_leaves_the_read_noise():
    S, R, rn = 64, 3, 20.0
    pl = hand_made_planes(S, R)
    reads = np.full((R + 1, S, S), 1234.0, dtype=np.float32)             # every difference is zero
    windows = [(10, 20), (15, 30), (25, 50), (3, 61)]
    got = variance_law.restate(reads, pl, windows, (6, 16), rn)
    q2 = (pl.gain / 2.35) ** 2
    for p, (lo, hi) in enumerate(windows):
        want = rn * rn * q2[lo:hi].sum(axis=0)
        assert np.allclose(got.VA[p], want, rtol=1e-13, atol=0.0), p
        assert got.VA[p, 0] == rn * rn * (hi - lo)                         # the border: q = 1
    # and without read noise nothing is left at all
    none = variance_law.restate(reads, pl, windows, (6, 16), 0.0)
    assert not none.spectra_var.any() and not none.sky_var.any()


def test_doubling_the_window_doubles_the_sums():
    S, R, rn = 64, 3, 20.0
    pl = hand_made_planes(S, R)
    rs = np.random.RandomState(7)
    ramp = 50.0 + 400.0 * rs.random_sample((1, S)) * np.ones((S, 1))     # constant along y, like the planes
    reads = np.stack([1000.0 + r * ramp for r in range(R + 1)]).astype(np.float64)
    one = variance_law.restate(reads, pl, [(10, 20), (10, 20), (10, 20), (10, 20)], (6, 16), rn)
    two = variance_law.restate(reads, pl, [(10, 30), (10, 30), (10, 30), (10, 30)], (6, 16), rn)
    assert (one.VA > 0.0).all()
    assert np.allclose(two.VA, 2.0 * one.VA, rtol=1e-13, atol=0.0)
    assert np.allclose(two.B, 2.0 * one.B, rtol=1e-13, atol=0.0)
    # the sky level is a mean: twice the pixels halve its variance, and B^2 sky_var doubles like VA
    assert np.allclose(two.sky_var, 0.5 * one.sky_var, rtol=1e-12, atol=0.0) and (one.sky_var > 0.0).all()
    assert np.allclose(two.spectra_var, 2.0 * one.spectra_var, rtol=1e-12, atol=0.0)
    # a pixel's variance is max(v, 0) + rn^2 q^2: product 0 of the ramp has v = ramp g
    v = (reads[1] - reads[0]) * pl.gain
    want = (np.maximum(v, 0.0) + rn * rn * (pl.gain / 2.35) ** 2)[10:20].sum(axis=0)
    assert np.allclose(one.VA[0], want, rtol=1e-13, atol=0.0)
    # a negative difference carries no Poisson term
    neg = variance_law.restate(reads[::-1].copy(), pl, [(10, 20)] * 4, (6, 16), rn)
    assert np.allclose(neg.VA[0], (rn * rn * (pl.gain / 2.35) ** 2)[10:20].sum(axis=0), rtol=1e-13, atol=0.0)


def test_integer_edges_sum_the_column_variances():
    S, R, rn = 64, 3, 20.0
    pl = hand_made_planes(S, R)
    rs = np.random.RandomState(9)
    reads = np.cumsum(100.0 * rs.random_sample((R + 1, S, S)), axis=0).astype(np.float32)
    windows = [(10, 20), (15, 30), (25, 50), (8, 55)]
    px = 2.0 ** -7                                                       # (exact: the edges fall on pixel boundaries)
    cols = [7, 8, 20, 33, 60]
    edges = 0.5 + px * np.array(cols, dtype=float)
    sol = (np.full(S, 0.5), np.full(S, px))
    for steps in (law.ALL, law.ALL & ~law.SKY):
        got = variance_law.restate(reads, pl, windows, (6, 16), rn, steps, edges=edges, wl_a=sol[0], wl_b=sol[1])
        for b in range(4):
            col = got.VA[:, cols[b]:cols[b + 1]].sum(axis=1)
            assert np.allclose(got.VP[:, b], col, rtol=1e-12, atol=0.0), (steps, b)
            if not steps & law.SKY:
                assert (got.sky_var == 0.0).all()
                assert np.allclose(got.channels_var[:, b], got.spectra_var[:, cols[b]:cols[b + 1]].sum(axis=1), rtol=1e-12, atol=0.0)
            else:
                # the sky level is one number for all the columns of a channel: its term adds as (sum B)^2, not sum B^2
                Bsum = got.B[:, cols[b]:cols[b + 1]].sum(axis=1)
                assert np.allclose(got.Q[:, b], Bsum, rtol=1e-12, atol=0.0)
                assert np.allclose(got.channels_var[:, b], col + Bsum * Bsum * got.sky_var, rtol=1e-12, atol=0.0)
    # a fractional edge weighs the shared pixel's variance by w^2: 0.25 + 0.25 of it, not all of it
    half = variance_law.restate(reads, pl, windows, (6, 16), rn, law.ALL & ~law.SKY,
                                edges=0.5 + px * np.array([20.0, 20.5, 21.0]), wl_a=sol[0], wl_b=sol[1])
    assert np.allclose(half.channels_var.sum(axis=1), 0.5 * half.VA[:, 20], rtol=1e-12, atol=0.0)
    # the last-read product off: zeros
    off = variance_law.restate(reads, pl, windows, (6, 16), rn, law.ALL & ~law.LAST_READ, edges=edges, wl_a=sol[0], wl_b=sol[1])
    assert not off.spectra_var[R].any() and not off.channels_var[R].any() and off.sky_var[R] == 0.0 and off.spectra_var[:R].all()


def test_assert_parity_is_relative_to_the_variance_itself():
    S, R = 64, 3
    pl = hand_made_planes(S, R)
    reads = np.cumsum(np.full((R + 1, S, S), 50.0), axis=0)
    want = variance_law.restate(reads, pl, [(10, 20)] * 4, (6, 16), 20.0)
    variance_law.assert_parity(want.spectra_var * (1.0 + 5e-10), want.sky_var, None, want, "inside")
    with pytest.raises(AssertionError):
        variance_law.assert_parity(want.spectra_var * (1.0 + 2e-9), want.sky_var, None, want, "outside")
    with pytest.raises(AssertionError):
        variance_law.assert_parity(want.spectra_var, want.sky_var * (1.0 - 2e-9), None, want, "sky outside")


def oracle_ensemble(n, rn=20.0):
    """n CPU-oracle exposures of small256 that differ in their draws alone (no cosmic rays, no scan-speed variation, no
    flat) -> (channels, channels_var, channels_var at read_noise 0) [n, R + 1, 10] by the numpy laws: 10 channels with
    edges on integer columns inside the trace."""
    v = helpers.make_visit("small256")
    pl = law.Planes(v)
    S = pl.S
    eo = helpers.oracle_generator(v)
    kw = v.frame_kwargs(0, cosmic_rate=None, ssv_generator=None, add_flat=False)
    plan = extraction.ExtractionOptions().plan(v.grism, v.wl, kw["x_ref"], kw["y_ref"], kw["scan_speed"], v.read_times,
                                               507 - 128, S)
    px = 2.0 ** -7
    sol = (np.full(S, 0.5), np.full(S, px))
    edges = 0.5 + px * np.arange(59.0, 190.0, 13.0)                      # columns 59, 72, ... 189: inside the first order
    assert edges.size == 11
    out = []
    for i in range(n):
        draws = wo.PhiloxDraws(v.seed, i, v.detector.light_sensitive_size(v.SUBARRAY))
        reads = np.stack(eo.scanning_frame(threads=2, draws=draws, thrower="oracle", **helpers.oracle_kwargs(kw)))
        ch = channel_law.restate(reads, pl, plan.row_windows, plan.bg_cols, edges, sol[0], sol[1])
        cv, cv0 = (variance_law.restate(reads, pl, plan.row_windows, plan.bg_cols, r, edges=edges, wl_a=sol[0],
                                        wl_b=sol[1]).channels_var for r in (rn, 0.0))
        out.append((ch.channels, cv, cv0))
    return tuple(np.array([o[k] for o in out]) for k in range(3))


def test_the_law_describes_the_cpu_oracles_noise():
    # The device test's ensemble (tests/test_variance_gpu.py) at a quarter of its size, on CPU-oracle reads and with the
    # numpy laws: 10 (n - 1) times the pooled ratio is chi-square with 10 (n - 1) degrees of freedom, so its standard
    # deviation is sqrt(2 / (10 (n - 1))) -- derived, not measured.  Measured with n = 64 (bound 4 x 0.056): 0.918 with the
    # read noise, 2.668 without; with n = 600: 0.952 and 2.773 (max(v, 0) of a pixel that holds noise alone averages 0.4 rn
    # above its mean, so the law overestimates by a few per cent where the read noise dominates).
    n = 16
    channels, cv, cv0 = oracle_ensemble(n)
    sd = np.sqrt(2.0 / (10 * (n - 1)))
    ratio, per_channel = variance_law.ensemble_ratio(channels, cv, cv0)
    ratio0, _ = variance_law.ensemble_ratio(channels, cv0, cv0)
    print("CPU oracle, %d exposures: ensemble / predicted variance %.3f (per channel %s), with read_noise = 0: %.3f; "
          "allowed |ratio - 1| <= %.3f" % (n, ratio, np.round(per_channel, 2), ratio0, 4 * sd))
    assert abs(ratio - 1.0) <= 4 * sd
    assert abs(ratio0 - 1.0) > 4 * sd                                     # the read noise is most of it


def test_variances_are_validated_and_plans_carry_them():
    assert extraction.Variances().read_noise == 20.0 == extraction.CosmicRejection().read_noise
    assert extraction.Variances(read_noise=0).read_noise == 0.0
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            extraction.Variances(bad)
    assert extraction.Variances.coerce(None) is None and extraction.Variances.coerce(False) is None
    assert extraction.Variances.coerce(True).read_noise == 20.0
    own = extraction.Variances(13.5)
    assert extraction.Variances.coerce(own) is own
    with pytest.raises(TypeError):
        extraction.Variances.coerce(13.5)
    d = own.desc()
    assert isinstance(d, _lib.VarianceDesc) and d.read_noise == 13.5
    plain, with_var = extraction.Extraction(WINDOWS), extraction.Extraction(WINDOWS, variance=True)
    assert plain.variance is None and extraction.Extraction(WINDOWS, variance=False).variance is None
    assert with_var.variance.read_noise == 20.0
    assert bytes(plain.desc()) == bytes(with_var.desc())                  # the extraction's own descriptor is untouched
    with pytest.raises(ValueError):
        extraction.Extraction(WINDOWS, steps=extraction.ALL & ~extraction.GAIN, variance=True)
    # the other options keep it, and it keeps them
    S = 266
    ch = extraction.Channels.linear(1.1, 1.7, 20)
    sol = (np.full(S, 0.9), np.full(S, 0.0046))
    full = extraction.Extraction(WINDOWS, crrej=True, channels=ch, row_solution=sol, variance=own)
    assert full.with_crrej(None).variance is own and full.with_channels(None).variance is own
    v2 = full.with_variance(None)
    assert v2.variance is None and v2.crrej is full.crrej and v2.channels is ch and v2.hull == full.hull
    opts = extraction.ExtractionOptions(variance=own)
    assert opts.variance is own and extraction.ExtractionOptions().variance is None
    # the frame's variance= replaces the plan's; without an extraction it is an error
    args = (None, None, 0.0, 0.0, 0.0, [1.0], 0, 266)
    assert extraction.for_exposure(plain, *args, variance=True).variance.read_noise == 20.0
    assert extraction.for_exposure(with_var, *args).variance is with_var.variance
    assert extraction.for_exposure(with_var, *args, variance=False).variance is None
    assert extraction.for_exposure(with_var, *args, crrej=True).variance is with_var.variance
    assert extraction.for_exposure(plain, *args, crrej=True, variance=own).crrej.k == 8.0
    assert extraction.for_exposure(None, *args, variance=False) is None
    with pytest.raises(ValueError):
        extraction.for_exposure(None, *args, variance=True)


def test_variance_struct_mirrors_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wayne_hip.h"\n'
                   'int main(void) {\n  printf("%zu %zu\\n", sizeof(wayne_variance_desc), offsetof(wayne_variance_desc, read_noise));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", exe], check=True)
    size, off = (int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(_lib.VarianceDesc) == 8 and off == _lib.VarianceDesc.read_noise.offset == 0
    for name in ("wayne_exposure_set_variance", "wayne_exposure_variances"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 7


HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include "host_plan.h"
using namespace wayne;
int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  int bad = 0;
  auto expect = [&](bool ok, unsigned steps, double rn, const char* what) {
    const char* why = plan::variance_desc_error(steps, rn);
    if ((why == nullptr) != ok) { std::printf("WRONG %s: %s\n", what, why ? why : "accepted"); ++bad; }
  };
  expect(true, X_ALL, 20.0, "defaults");
  expect(true, X_GAIN, 0.0, "gain alone, rn 0");
  expect(false, X_ALL, -1.0, "rn negative");
  expect(false, X_ALL, nan, "rn nan");
  expect(false, X_ALL, inf, "rn inf");
  expect(false, X_ALL, -inf, "rn -inf");
  expect(false, X_ALL & ~X_GAIN, 20.0, "gain off");
  std::printf("checked\n");
  return bad ? 1 : 0;
}
"""


def test_variance_desc_error_in_a_program_of_its_own(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "variance_plan.cpp"
    src.write_text(HARNESS)
    exe = str(tmp_path / "variance_plan")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "wayne_amd", "csrc"), str(src), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checked" in r.stdout and "WRONG" not in r.stdout, r.stdout + r.stderr


def test_npz_keys_with_and_without_variances():
    S, R, n, n_ch = 266, 3, 2, 20
    ch = extraction.Channels.linear(1.1, 1.7, n_ch).with_flat(False)
    sol = (np.full(S, 0.9), np.full(S, 0.0046))
    base = ["spectra", "sky", "exposure_index", "row_lo", "row_hi", "bg_cols", "x_ref", "y_ref", "read_times", "exp_start"]
    chan = ["channels", "channel_edges_um", "channel_flat", "wl_a", "wl_b"]
    args = (np.zeros((n, R + 1, S)), np.zeros((n, R + 1)), [0, 1])
    more = ([1.0, 2.0], [3.0, 4.0], [1.0, 2.0, 3.0], [0.0, 9.0])
    sv = np.arange(n * (R + 1) * S, dtype=float).reshape(n, R + 1, S)
    kv = np.arange(n * (R + 1), dtype=float).reshape(n, R + 1)
    cv = np.arange(n * (R + 1) * n_ch, dtype=float).reshape(n, R + 1, n_ch)

    def keys(plan, **kw):
        f = io.BytesIO()
        extraction.save_npz(f, *args, [plan] * n, *more, **kw)
        f.seek(0)
        return np.load(f)

    assert sorted(keys(extraction.Extraction(WINDOWS, variance=True)).files) == sorted(base)     # on, but nothing was delivered
    z = keys(extraction.Extraction(WINDOWS, variance=extraction.Variances(17.0)), variances=(sv, kv, None))
    assert sorted(z.files) == sorted(base + ["spectra_var", "sky_var", "variance_read_noise"])
    assert z["spectra_var"].tobytes() == sv.tobytes() and z["sky_var"].tobytes() == kv.tobytes()
    assert float(z["variance_read_noise"]) == 17.0
    with_ch = extraction.Extraction(WINDOWS, channels=ch, row_solution=sol, variance=True)
    channels = np.zeros((n, R + 1, n_ch))
    z = keys(with_ch, channels=channels, variances=(sv, kv, cv))
    assert sorted(z.files) == sorted(base + chan + ["spectra_var", "sky_var", "channels_var", "variance_read_noise"])
    assert z["channels_var"].tobytes() == cv.tobytes() and z["channels_var"].shape == (n, R + 1, n_ch)
    assert sorted(keys(with_ch.with_variance(None), channels=channels).files) == sorted(base + chan)


def test_cli_argument_errors():
    yml = os.path.join(ROOT, "tests", "fixtures", "mini_visit", "params.yml")
    for argv in (["--variances"], ["--variances", "15"]):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml] + argv)
        assert "--variances needs --spectra or --spectra-only" in str(e.value)
    for rn in ("-3", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            run_visit.run(["-p", yml, "--spectra-only", "x.npz", "--variances=" + rn])
        assert "RN" in str(e.value) and "read_noise must be" in str(e.value)


def test_algorithmic_bytes_count_the_variance_sums():
    S, R, n_ch = 266, 3, 20
    ch = extraction.Channels.linear(1.1, 1.7, n_ch)
    sol = (np.full(S, 0.9), np.full(S, 0.0046))
    plan = extraction.Extraction(WINDOWS, variance=True)
    base = extraction.algorithmic_bytes(plan, S, R)
    assert extraction.algorithmic_bytes(plan, S, R, variance=False) == base
    chunks = 2 + 2 + 2 + 2
    # no plane is read for the variances: the chunks' sums written and read, and the results written
    assert extraction.algorithmic_bytes(plan, S, R, variance=True) - base == 2 * chunks * S * 8 + (R + 1) * (S + 1) * 8
    for crrej in (False, True):
        assert (extraction.algorithmic_bytes(plan, S, R, crrej=crrej, variance=True) -
                extraction.algorithmic_bytes(plan, S, R, crrej=crrej)) == 2 * chunks * S * 8 + (R + 1) * (S + 1) * 8
    binned = extraction.Extraction(WINDOWS, channels=ch, row_solution=sol, variance=True)
    with_ch = extraction.algorithmic_bytes(binned, S, R, channels=True)
    assert (extraction.algorithmic_bytes(binned, S, R, channels=True, variance=True) - with_ch ==
            2 * chunks * S * 8 + (R + 1) * (S + 1) * 8 + 2 * chunks * n_ch * 8 + (R + 1) * n_ch * 8)
