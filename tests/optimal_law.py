"""TEST INFRASTRUCTURE: the law of the optimal (profile-weighted) extraction (include/wayne_hip.h, wayne_optimal_desc)
restated in numpy on top of tests/extraction_law.py, tests/channel_law.py (pixel_terms) and tests/variance_law.py.  Shared
by tests/test_optimal.py (properties of the law, the ensemble of CPU-oracle exposures) and tests/test_optimal_gpu.py (the
oracle of the device).

    d(y, x)  = v - sky_p bt,  bt = scale_p t            X(x) = [max(x - H, 0), min(x + H, S - 1)]
    S1(y, x) = sum_{x' in X(x), ascending} d(y, x')
    S0(x)    = sum_{x' in X(x), ascending} spectra_p[x']     SV0(x) = the same sum of spectra_var_p
    ok(x)   <=> S0 > 0 and S0 S0 > 9 SV0
    Pr = S1 / S0,  P = max(Pr, 0)
    V(y, x)  = max(spectra_p[x] Pr + sky_p bt, 0) + rn^2 (q q),  q = g / 2.35
    U_p[x] = sum_y (P d) / V,  W_p[x] = sum_y (P P) / V,  G_p[x] = sum_y (P bt) / V
    optimal_p[x]     = ok and W > 0 ? U / W                         : spectra_p[x]
    optimal_var_p[x] = ok and W > 0 ? 1 / W + (G/W)(G/W) sky_var_p  : spectra_var_p[x]

`restate` takes spectra, sky, spectra_var and sky_var as INPUTS: the device tests hand in the device's own delivered arrays
(verified against their laws in tests/test_extraction_gpu.py and tests/test_variance_gpu.py), so that d, S0, SV0, S1, ok, P
and V are formed from bit-identical numbers by the operations written here in this order (the library is compiled without
contraction) and no comparison -- ok, the clamps -- can fall the other way.  S1, S0 and SV0 are explicit loops over the
offset in ascending order: the device sums left to right too.

Tolerance (derived, not tuned): only the order of the row sums U, W and G differs -- at most 1024 terms each, so an exact
float64 summation in any order errs by at most 1024 x 2^-53 ~ 1e-13 of M_U = sum_y |P d / V| (W and G sum non-negative
terms when t >= 0: 1e-13 of themselves).  The project allows 1e-9 per sum (extraction_law.REL): optimal = U / W carries
the error of U and of W, hence 2e-9 M_U / W; optimal_var = 1 / W + (G/W)^2 sky_var carries W's once in the first term and
G's and W's twice each in the second, hence 4e-9 of itself.  On fallback columns the box values come back to the bit.
"""
import collections

import numpy as np

import channel_law
import extraction_law as law

REL = law.REL
Result = collections.namedtuple("Result", "optimal optimal_var ok U W G M_U")


def window_sum(a, H):
    """sum_{x' in X(x), ascending} a[..., x'] for every x -> the shape of `a`: a literal left-to-right sum."""
    a = np.asarray(a, dtype=np.float64)
    S = a.shape[-1]
    out = np.zeros_like(a)
    x = np.arange(S)
    for k in range(-H, H + 1):                                  # ascending offset = ascending x'
        src = x + k
        inside = (src >= 0) & (src <= S - 1)
        out[..., inside] = out[..., inside] + a[..., src[inside]]
    return out


def restate(reads, pl, windows, H, rn, spectra, sky, spectra_var, sky_var, steps=law.ALL, crrej=None, renormalise=False,
            data_variance=False):
    """reads [R + 1, S, S] of any type and the box extraction's spectra [R + 1, S], sky [R + 1], spectra_var [R + 1, S],
    sky_var [R + 1] -> Result(optimal, optimal_var [R + 1, S], ok [R + 1, S] (ok and W > 0: the optimal branch), U, W, G,
    M_U [R + 1, S]).  `crrej`: (k, rn) of the rejection or None.  `renormalise` (Horne's P / sum_y P after the clamp) and
    `data_variance` (V from the pixel's own v) are the two variants the law decided against: for the tests that show
    why."""
    R, S = reads.shape[0] - 1, reads.shape[-1]
    spectra, spectra_var = np.asarray(spectra, dtype=np.float64), np.asarray(spectra_var, dtype=np.float64)
    sky, sky_var = np.asarray(sky, dtype=np.float64), np.asarray(sky_var, dtype=np.float64)
    rn2 = float(rn) * float(rn)
    T = pl.sky if steps & law.SKY else np.zeros((S, S))
    out = Result(*(np.zeros((R + 1, S)) for _ in range(2)), np.zeros((R + 1, S), dtype=bool), *(np.zeros((R + 1, S)) for _ in range(4)))
    for p, term in enumerate(channel_law.pixel_terms(reads, pl, windows, steps, crrej)):
        if term is None:
            continue
        sl, v, _ = term
        rows = sl.stop - sl.start
        g = pl.gain[sl] if steps & law.GAIN else np.ones((rows, S))
        q = g / 2.35
        scale = pl.dt[p] if p < R else pl.dt.sum()
        bt = scale * T[sl]
        d = v - sky[p] * bt
        S1 = window_sum(d, H)
        S0, SV0 = window_sum(spectra[p], H), window_sum(spectra_var[p], H)
        detected = (S0 > 0.0) & (S0 * S0 > 9.0 * SV0)
        with np.errstate(all="ignore"):
            Pr = S1 / S0
            P = np.maximum(Pr, 0.0)
            if renormalise:
                P = P / P.sum(axis=0)
            V = np.maximum(v if data_variance else spectra[p] * Pr + sky[p] * bt, 0.0) + rn2 * (q * q)
            u, w, gg = (P * d) / V, (P * P) / V, (P * bt) / V
            U, W, G = u.sum(axis=0), w.sum(axis=0), gg.sum(axis=0)
            ok = detected & (W > 0.0)
            GW = G / W
            out.optimal[p] = np.where(ok, U / W, spectra[p])
            out.optimal_var[p] = np.where(ok, 1.0 / W + (GW * GW) * sky_var[p], spectra_var[p])
            out.M_U[p] = np.abs(u).sum(axis=0)
        out.ok[p], out.U[p], out.W[p], out.G[p] = ok, U, W, G
    return out


def box(reads, pl, windows, bg, rn, steps=law.ALL, crrej=None):
    """(spectra, sky, spectra_var, sky_var) of the box extraction by the numpy laws: the inputs of `restate` where no
    device delivered them (without rejection, or with the (k, rn) of `crrej`)."""
    import crrej_law
    import variance_law
    if crrej is None:
        spectra, sky = law.restate(reads, pl, windows, bg, steps)[:2]
    else:
        r = crrej_law.restate(reads, pl, windows, bg, steps, crrej[0], crrej[1])
        spectra, sky = r.spectra, r.sky
    var = variance_law.restate(reads, pl, windows, bg, rn, steps, crrej)
    return spectra, sky, var.spectra_var, var.sky_var


def assert_parity(got_optimal, got_optimal_var, want, spectra, spectra_var, what=""):
    """The device's (optimal, optimal_var) against a Result formed from the same delivered box arrays: 2e-9 M_U / W and
    4e-9 of the variance on the optimal columns, the box values to the bit on the others."""
    got, got_var = np.asarray(got_optimal), np.asarray(got_optimal_var)
    assert got.shape == want.optimal.shape and got_var.shape == want.optimal_var.shape, what
    ok = want.ok
    with np.errstate(all="ignore"):
        bound = np.where(ok, 2.0 * REL * want.M_U / want.W, 0.0)
    err = np.abs(got - want.optimal)
    err_var = np.abs(got_var - want.optimal_var)
    worst = float((err[ok] / np.maximum(bound[ok], 1e-300)).max()) * 2.0 * REL if ok.any() else 0.0
    worst_var = float((err_var[ok] / want.optimal_var[ok]).max()) if ok.any() else 0.0
    print("%s: %d optimal and %d fallback columns; worst |optimal - oracle| W / M_U = %.3g (allowed %.0e), worst relative "
          "|optimal_var - oracle| = %.3g (allowed %.0e)" % (what, int(ok.sum()), int((~ok).sum()), worst, 2.0 * REL, worst_var,
                                                              4.0 * REL))
    assert np.isfinite(got).all() and np.isfinite(got_var).all(), what
    assert (err[ok] <= bound[ok]).all(), (what, worst)
    assert (err_var[ok] <= 4.0 * REL * want.optimal_var[ok]).all(), (what, worst_var)
    assert (got_var[ok] > 0.0).all(), what
    assert got[~ok].tobytes() == np.asarray(spectra)[~ok].tobytes(), what + ": fallback columns are the box values"
    assert got_var[~ok].tobytes() == np.asarray(spectra_var)[~ok].tobytes(), what + ": fallback variances are the box values"


def ensemble_figures(optimal, optimal_var, spectra, cols):
    """The ensemble tests' three figures for one product.  optimal, optimal_var, spectra [N, S] of N exposures that differ
    in their random draws alone; `cols` = (c0, c1) -> (ensemble variance of optimal / of spectra, both summed over the
    columns; paired mean bias sum(optimal - spectra) / sum(spectra); ensemble variance / mean predicted variance of
    optimal, summed over the columns)."""
    c0, c1 = cols
    o, s, ov = (np.asarray(a, dtype=np.float64)[:, c0:c1] for a in (optimal, spectra, optimal_var))
    var_o, var_s = o.var(axis=0, ddof=1).sum(), s.var(axis=0, ddof=1).sum()
    bias = (o - s).mean(axis=0).sum() / s.mean(axis=0).sum()
    return float(var_o / var_s), float(bias), float(var_o / ov.mean(axis=0).sum())
