"""The device light curves across the (z, rp, spread) plane, CPU side (tests/lightcurve_plane.py has the restatements):

  * the Chebyshev interpolation of k_lightcurve / k_lightcurve_ld in exact arithmetic against the law it interpolates,
    wherever the kernels' decision (`route`) takes it: 2e-9, a tenth of the 2e-8 the device is held to, so that the fit
    does not spend the float32 integrand's share;
  * the law (wayne_amd/lightcurve.py, 24 nodes) against the oracle's 2-D integral over the plane;
  * what the float32 integrand costs, per radius ratio: recorded in profiles/lightcurve_plane.json (`f32_emulation`),
    where the GPU test takes its bound beyond rp 0.2 from;
  * negative elements of the planet spectrum on the host: a column of zeros, nothing else moves.
GPU side: tests/test_lightcurve_plane_gpu.py."""
import numpy as np
import pytest

import lightcurve_plane as lp
from oracle import clib
from wayne_amd import lightcurve as lc

P0 = (0.03, 0.1208, 0.3)
SPREAD = (0.002, 0.02, 0.15, 0.3)
N_P = 4001
INTERP_TOL = 2e-9


def interpolation_errors(p0, spread, rel=None):
    """Worst |interpolant - law| over N_P radius ratios for every `families` separation the kernels interpolate at: per
    law, and for the five basis functions over pi.  {name: (error, label)}."""
    p_lo, p_hi = p0 * (1.0 - spread), p0 * (1.0 + spread)
    p = np.linspace(p_lo, p_hi, N_P)
    worst = {}
    n_cheb = 0
    for z, label in lp.families(p0, spread, rel):
        if lp.route(z, p_lo, p_hi, rel) != "cheb":
            continue
        n_cheb += 1
        errs = {name: np.abs(lp.cheb_of_law(z, p_lo, p_hi, ld, p) - (1.0 - lc.transit_flux(z, p, ld))).max()
                for name, ld in lp.LAWS.items()}
        B = lp.cheb_interp(lambda q: np.stack(lc.transit_basis(z, q), axis=1), p_lo, p_hi, p)
        D = np.stack(lc.transit_basis(z, p), axis=1)
        for n in range(5):
            errs["B_%d/pi" % n] = np.abs(B[:, n] - D[:, n]).max() / np.pi
        for name, e in errs.items():
            if e >= worst.get(name, (0.0, ""))[0]:
                worst[name] = (float(e), label)
    return worst, n_cheb


@pytest.mark.parametrize("spread", SPREAD)
@pytest.mark.parametrize("p0", P0)
def test_interpolation_in_exact_arithmetic(p0, spread):
    """With the band the kernels had before it scaled with the width (guard = 1e-9 + 1e-6 width; `rel=1e-6` here) the
    worst figures of this test were, first contact 1.01 guard outside the interval in every case:
        rp 0.1208:  +-2 % 2.9e-9   +-15 % 5.6e-8   +-30 % 1.4e-7
        rp 0.3:     +-2 % 2.0e-8   +-15 % 3.8e-7   +-30 % 9.4e-7         rp 0.03 +-30 %: 8.4e-9
    with 0.08 width: 1.2e-9 (rp 0.3 +-30 %), 5.0e-10 (0.3 +-15 %), 1.8e-10 (0.1208 +-30 %)."""
    worst, n_cheb = interpolation_errors(p0, spread)
    assert n_cheb >= 20                     # every contact from outside the band, and most of the uniform draws
    for name, (e, label) in sorted(worst.items()):
        print("rp %g +- %g %%  %-8s worst |interpolant - law| = %.2e  (%s)" % (p0, 100 * spread, name, e, label))
    bad = {k: v for k, v in worst.items() if not v[0] <= INTERP_TOL}
    assert not bad, bad


def test_a_band_blind_to_the_width_is_caught():
    # the same measurement with the former band: it must miss the criterion (or the test above says nothing)
    worst, _ = interpolation_errors(0.1208, 0.15, rel=1e-6)
    assert max(e for e, _ in worst.values()) > 10 * INTERP_TOL


def test_families_cover_every_route():
    for p0 in P0:
        for spread in SPREAD:
            p_lo, p_hi = p0 * (1.0 - spread), p0 * (1.0 + spread)
            fam = dict((label, z) for z, label in lp.families(p0, spread))
            routes = {label: lp.route(z, p_lo, p_hi) for label, z in fam.items()}
            assert set(routes.values()) == {"none", "direct", "cheb"}
            for name, _, _ in lp.contacts(p_lo, p_hi):
                # the band's edge is straddled from both sides, and so is the interval's end
                assert routes["%s outside 0.5 guard" % name] == "direct"
                assert routes["%s outside 1.01 guard" % name] == "cheb"
                assert routes["%s outside 2 guard" % name] == "cheb"
                assert routes["%s inside 2 guard" % name] == "direct"
            assert routes["1+p_hi - 2 guard"] == "direct" and routes["1+p_hi + 2 guard"] == "none"
            assert routes["z=1.5"] == "none"
    assert lp.route(0.5, 0.12, 0.12) == "flat" and lp.route(0.88, 0.12, 0.12) == "direct"
    assert lp.route(0.5, np.nan, np.nan) == "none"


LAWS6 = [("LD", lp.LD), ("uniform", lp.UNIFORM)] + [
    ("a%d=0.9" % (n + 1), [0.9 if i == n else 0.0 for i in range(4)]) for n in range(4)]
P_PLANE = np.array([0.01, 0.03, 0.0845, 0.1208, 0.2, 0.3, 0.5])


def plane_z():
    c = np.concatenate([1.0 - P_PLANE, 1.0 + P_PLANE, P_PLANE])
    return np.concatenate([np.linspace(0.0, 1.6, 161), c])


@pytest.mark.parametrize("name,ld", LAWS6)
def test_law_against_the_oracle(name, ld):
    """Worst |law - oracle| measured: 1.5e-9 (p = 0.5, a4 = 0.9); <= 2.5e-10 for p <= 0.3."""
    z = plane_z()
    got = 1.0 - lc.transit_flux(z[:, None], P_PLANE[None, :], ld)
    want = clib.lc_deficit(z, P_PLANE, ld)
    err = np.abs(got - want).max(axis=0)
    print("%s: worst |law - oracle| per p: %s" % (name, " ".join("%.1e" % e for e in err)))
    assert err[P_PLANE <= 0.3].max() <= 5e-10
    assert err[P_PLANE == 0.5].max() <= 3e-9
    # the oracle is converged on the same grid
    assert np.abs(want - clib.lc_deficit(z, P_PLANE, ld, nodes=257)).max() <= 1e-13


F32_P0 = (0.03, 0.1208, 0.16, 0.3, 0.5)
F32_SPREAD = 0.3


def f32_figure(p0):
    """Worst |float32-integrand law - oracle| over the `families` separations of p0 (1 +- 30 %), 129 radius ratios
    across the interval, the three laws."""
    p_lo, p_hi = p0 * (1.0 - F32_SPREAD), p0 * (1.0 + F32_SPREAD)
    z = np.array([v for v, _ in lp.families(p0, F32_SPREAD)])
    p = np.linspace(p_lo, p_hi, 129)
    return max(float(np.abs(lp.deficit_f32(z, p, ld) - clib.lc_deficit(z, p, ld)).max()) for ld in lp.LAWS.values())


def test_what_float32_costs():
    """Measured: 1.7e-9 (rp 0.03), 8.7e-9 (0.1208), 1.2e-8 (0.16), 3.5e-8 (0.3), 7.6e-8 (0.5), each +-30 %: the error grows
    with rp, and the project's flat 2e-8 holds up to rp ~ 0.2 only.  Asserted: 2e-8 where p_hi <= 0.21, and everywhere
    two float32 ulps of the largest radius ratio (2^-22 p_hi: the rounding of z, p and |z - p| to float32 alone moves
    the deficit by d(deficit)/dp ~ 2 p times 2^-24 p, and the 24 nodes' roundings add to it)."""
    figures = {}
    for p0 in F32_P0:
        e = f32_figure(p0)
        p_hi = p0 * (1.0 + F32_SPREAD)
        print("float32 integrand, rp %g +- 30 %%: worst |emulation - oracle| = %.2e" % (p0, e))
        figures["%g" % p0] = float("%.2g" % e)
        assert e <= 2.0 ** -22 * p_hi
        if p_hi <= 0.21:
            assert e <= 2e-8
    lp.record("f32_emulation", figures)
    assert figures["0.3"] > figures["0.1208"] > figures["0.03"]


HIDDEN = np.array([0.0, 0.0, 0.4, 1.0, 0.0])
Z_NEG = np.array([0.3, 1.05, 10.3, 11.0, 0.0])


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("hidden", [None, "zeros", "behind"])
def test_negative_spectrum_elements_on_the_host(hidden, table):
    W = 40
    spec = (0.1208 * (1.0 + 0.02 * np.sin(np.arange(W) / 3.0))) ** 2
    hid = {None: None, "zeros": np.zeros(5), "behind": HIDDEN}[hidden]
    ld = lp.LD
    if table:
        s = np.linspace(0.0, 1.0, W)
        ld = np.stack([0.55 + 0.25 * s, -0.2 - 0.55 * s, 0.5 + 0.4 * s, -0.25 - 0.13 * s], axis=1)
    clean = lc.DeviceDepths(Z_NEG, hid, spec, ld).host_matrix()
    assert np.isfinite(clean).all() and clean[0].min() > 0.01
    for planted in ([0], [W // 2], [0, W // 2], list(range(W))):
        bad = spec.copy()
        bad[planted] = [-1e-4, -0.3, -1e-4, -0.3][:len(planted)] if len(planted) <= 2 else -0.01
        got = lc.DeviceDepths(Z_NEG, hid, bad, ld).host_matrix()
        assert np.isfinite(got).all()
        assert not got[:, planted].any()
        keep = np.setdiff1d(np.arange(W), planted)
        assert got[:, keep].tobytes() == clean[:, keep].tobytes()
