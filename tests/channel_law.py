"""TEST INFRASTRUCTURE: the law of the extraction's wavelength-binned channels (include/wayne_hip.h,
wayne_channels_desc) restated in numpy on top of tests/extraction_law.py and tests/crrej_law.py.  Shared by
tests/test_channels.py (the law against the column spectra, flux conservation, the science checks on CPU-oracle reads)
and tests/test_channels_gpu.py (the oracle of the device).

    ua_b(y)  = (e[b] - wl_a[y]) / wl_b[y]
    w_b(y,x) = min(max(min(x + 1, ua_{b+1}) - max(x, ua_b), 0), 1)
    F(y,x)   = float32(f0 + f1 tau + f2 tau^2 + f3 tau^3), tau = (1e4 (wl_a[y] + wl_b[y] x) - wmin) / (wmax - wmin), off the
               border and where > 0; else 1
    P_p[b] = sum w_b (v / F),  Q_p[b] = scale_p sum w_b (t / F),  channels_p[b] = P_p[b] - sky_p Q_p[b]

v is the term the column extraction sums for the pixel (extraction_law; under rejection crrej_law's cleaned value) and
sky_p the column extraction's level: `restate` takes it from the caller (the device's own, in the GPU tests -- the law
is a function of the level the column extraction formed) or forms it with extraction_law / crrej_law.

Tolerance (derived, not tuned): a channel sums at most 1024 rows x 384 columns ~ 4e5 terms, so an exact float64
summation in any order errs by at most 4e5 x 2^-53 ~ 4e-11 of
M_p[b] = sum w (|L_hi| + |L_lo| + |dark_hi| + |dark_lo|) g / F + |sky_p| Q_p[b]; the tests allow extraction_law.REL =
1e-9 of it.  A float32 accumulation anywhere misses that by orders of magnitude.
"""
import collections

import numpy as np

import crrej_law
import extraction_law as law

REL = law.REL
C_FLAT = 1
Result = collections.namedtuple("Result", "channels M P Q sky")


class Flat(object):
    """The flat cube of a synthetic.Visit's mode as the engine uploads it: four [N, N] float32 planes and the
    wavelength range (A) of the cubic's argument."""

    def __init__(self, v):
        read_times = np.asarray(v.read_times, dtype=float)
        planes = v.calibration.for_mode(v.grism.name, v.SUBARRAY, v.SAMPSEQ, read_times, detector=v.detector)
        self.cube = [np.asarray(p, dtype=np.float32) for p in planes["flat"]]
        self.wmin, self.wmax = (float(x) for x in v.calibration.flat_wl[v.grism.name])


def flat_factor(flat, wl_a, wl_b, S):
    """F [S, S] (float64) of the law; `flat` None: ones."""
    F = np.ones((S, S))
    if flat is None:
        return F
    x = np.arange(S, dtype=np.float64)[None, :]
    a, b = np.asarray(wl_a, dtype=np.float64)[:, None], np.asarray(wl_b, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        tau = ((1e4 * (a + b * x)) - flat.wmin) / (flat.wmax - flat.wmin)
        tau = tau[5:-5, 5:-5]
        t2 = tau * tau
        t3 = t2 * tau
        f0, f1, f2, f3 = (p.astype(np.float64) for p in flat.cube)
        f = f0 + (f1 * tau) + (f2 * t2) + (f3 * t3)
        f = f.astype(np.float32).astype(np.float64)
    F[5:-5, 5:-5] = np.where(f > 0.0, f, 1.0)
    return F


def pixel_terms(reads, pl, windows, steps=law.ALL, crrej=None):
    """Per product p (None where it is not formed): (rows slice, v [rows, S], Mv [rows, S]) -- the term the column
    extraction adds to A_p[x] for each pixel of the window, and the magnitude that bounds it.  `crrej`: (k, rn)."""
    R, S = reads.shape[0] - 1, reads.shape[-1]
    out = [None] * (R + 1)
    if crrej is None:
        c1, c2, c3, c4 = pl.lin

        def linear(r, sl):
            if r == 0:
                return 0.0, 0.0
            D = reads[r, sl].astype(np.float64) - reads[0, sl].astype(np.float64)
            L = D * (1.0 + c1[sl] + D * (c2[sl] + D * (c3[sl] + c4[sl] * D))) if steps & law.LINEARISE else D
            dk = pl.dark[r, sl] if steps & law.DARK else np.zeros_like(D)
            return L - dk, np.abs(dk)

        for p in range(R + 1):
            if p == R and not steps & law.LAST_READ:
                continue
            sl = slice(int(windows[p][0]), int(windows[p][1]))
            Lh, dh = linear(p + 1 if p < R else R, sl)
            Ll, dl = linear(p if p < R else 0, sl)
            g = pl.gain[sl] if steps & law.GAIN else 1.0
            out[p] = (sl, (Lh - Ll) * g, (np.abs(Lh) + np.abs(Ll) + dh + dl) * g * np.ones((sl.stop - sl.start, S)))
        return out
    k, rn = crrej
    m_lo, m_hi = crrej_law.mask_rows(windows, R, steps)
    slab = slice(max(m_lo - 2, 0), min(m_hi + 2, S))
    I, Mpix, LRg, MR = crrej_law.difference_images(reads, pl, steps, slab)
    in_rows = np.zeros((S, 1), dtype=bool)
    in_rows[m_lo:m_hi] = True
    clean, Mclean = I.copy(), Mpix.copy()
    corr, Mcorr = np.zeros((S, S)), np.zeros((S, S))
    for j in range(R):
        f, repl, _ = crrej_law.flags(I[j], k, rn)
        f &= in_rows
        nb = np.stack(crrej_law.row_neighbours(Mpix[j])).max(axis=0)
        clean[j][f], Mclean[j][f] = repl[f], nb[f]
        corr[f] += I[j][f] - repl[f]
        Mcorr[f] += Mpix[j][f] + nb[f]
    for p in range(R + 1):
        if p == R and not steps & law.LAST_READ:
            continue
        sl = slice(int(windows[p][0]), int(windows[p][1]))
        out[p] = (sl, clean[p][sl], Mclean[p][sl]) if p < R else (sl, LRg[sl] - corr[sl], MR[sl] + Mcorr[sl])
    return out


def bin_rows(values, rows, edges, wl_a, wl_b):
    """sum_y sum_x w_b(y, x) values_k[y - rows.start, x] for every channel b and every array of `values` (a list of
    [rows, S] arrays) -> [len(values), C].  Only the columns a channel can touch are looked at."""
    S = values[0].shape[1]
    a = np.asarray(wl_a, dtype=np.float64)[rows][:, None]
    b = np.asarray(wl_b, dtype=np.float64)[rows][:, None]
    e = np.asarray(edges, dtype=np.float64)
    C = e.size - 1
    out = np.zeros((len(values), C))
    ua = [(e[i] - a) / b for i in range(C + 1)]
    for c in range(C):
        x0 = int(min(max(np.floor(ua[c].min()), 0.0), float(S)))
        x1 = int(min(max(np.ceil(ua[c + 1].max()), 0.0), float(S)))
        if x1 <= x0:
            continue
        x = np.arange(x0, x1, dtype=np.float64)[None, :]
        w = np.minimum(np.maximum(np.minimum(x + 1.0, ua[c + 1]) - np.maximum(x, ua[c]), 0.0), 1.0)
        for k, val in enumerate(values):
            out[k, c] = (w * val[:, x0:x1]).sum()
    return out


def restate(reads, pl, windows, bg, edges, wl_a, wl_b, steps=law.ALL, flat=None, crrej=None, sky=None):
    """reads [R + 1, S, S] of any type -> Result(channels [R + 1, C], M [R + 1, C], P, Q [R + 1, C], sky [R + 1]).
    `flat`: a Flat when WAYNE_C_FLAT is set and the context holds a cube, else None; `crrej`: (k, rn) or None; `sky`:
    the column extraction's levels [R + 1] (None: formed here by extraction_law / crrej_law)."""
    R, S = reads.shape[0] - 1, reads.shape[-1]
    C = len(edges) - 1
    if sky is None:
        if crrej is None:
            sky = law.restate(reads, pl, windows, bg, steps)[1]
        else:
            sky = crrej_law.restate(reads, pl, windows, bg, steps, crrej[0], crrej[1]).sky
    sky = np.asarray(sky, dtype=np.float64)
    F = flat_factor(flat, wl_a, wl_b, S)
    T = pl.sky if steps & law.SKY else np.zeros((S, S))
    channels, M = np.zeros((R + 1, C)), np.zeros((R + 1, C))
    P, Q = np.zeros((R + 1, C)), np.zeros((R + 1, C))
    for p, term in enumerate(pixel_terms(reads, pl, windows, steps, crrej)):
        if term is None:
            continue
        sl, v, Mv = term
        scale = pl.dt[p] if p < R else pl.dt.sum()
        got = bin_rows([v / F[sl], T[sl] / F[sl], Mv / F[sl], np.abs(T[sl]) / F[sl]], sl, edges, wl_a, wl_b)
        P[p], Q[p] = got[0], scale * got[1]
        channels[p] = P[p] - sky[p] * Q[p]
        M[p] = got[2] + abs(sky[p]) * (scale * got[3])
    return Result(channels, M, P, Q, sky)


def assert_parity(got, want, what=""):
    """The device's channels against a Result, to REL of M per channel."""
    got = np.asarray(got)
    assert got.shape == want.channels.shape, (what, got.shape, want.channels.shape)
    err = np.abs(got - want.channels)
    worst = float((err / np.maximum(want.M, 1e-300)).max())
    print("%s: worst |channels - oracle| / M = %.3g (allowed %.0e)" % (what, worst, REL))
    assert np.isfinite(got).all(), what
    assert (err <= REL * want.M).all(), (what, worst)
