"""TEST INFRASTRUCTURE: the law of the extraction's cosmic-ray rejection (include/wayne_hip.h, wayne_crrej_desc) restated
in numpy on top of tests/extraction_law.py.  Shared by tests/test_crrej.py (the law against the truth of the CPU oracle)
and tests/test_crrej_gpu.py (the oracle of the device).

A flag is a comparison of two float64 numbers, d^2 and k^2 v with v = rn^2 + max(m8, 0): the device forms both with the
operations written here, in this order, so it decides as numpy does -- except that extraction_law's 1e-9 budget allows
for one contracted multiply-add in a pixel's chain.  Pixels with |d^2 - k^2 v| <= 1e-9 (d^2 + k^2 v) are therefore
reported as UNDECIDED: there the device may legitimately round the other way, and a test that compares masks exactly
first checks that its exposure has none.

Tolerance of the spectra: extraction_law's, 1e-9 M[x], where a flagged pixel enters M with the largest magnitude among
the four row neighbours its replacement is taken from (and, in the last-read product, with its own as well).
"""
import collections

import numpy as np

import extraction_law as law

MARGIN = 7            # pixels of the frame's edge that are never tested
UNDECIDED_REL = 1e-9

Result = collections.namedtuple("Result", "spectra sky n_rejected mask M M_sky undecided")


def _shift(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx] (0 where that lies outside the array)"""
    S0, S1 = a.shape
    b = np.zeros_like(a)
    ys = slice(max(-dy, 0), S0 - max(dy, 0))
    xs = slice(max(-dx, 0), S1 - max(dx, 0))
    yd = slice(max(dy, 0), S0 - max(-dy, 0))
    xd = slice(max(dx, 0), S1 - max(-dx, 0))
    b[ys, xs] = a[yd, xd]
    return b


def row_neighbours(a):
    return [_shift(a, 0, -2), _shift(a, 0, -1), _shift(a, 0, 1), _shift(a, 0, 2)]


def flags(I, k, rn):
    """One difference image I [S, S] (float64) -> (flag [S, S] bool, repl [S, S], undecided [S, S] bool) on every pixel
    at least MARGIN inside the frame (False / as computed elsewhere); the caller applies the mask rows."""
    S = I.shape[0]
    stencil = [_shift(I, -1, 0), _shift(I, 1, 0), _shift(I, -2, 0), _shift(I, 2, 0)] + row_neighbours(I)
    m8 = stencil[0]
    for s in stencil[1:]:
        m8 = np.maximum(m8, s)
    d = I - m8
    lhs = d * d
    rhs = (k * k) * ((rn * rn) + np.maximum(m8, 0.0))
    tested = np.zeros((S, S), dtype=bool)
    tested[MARGIN:S - MARGIN, MARGIN:S - MARGIN] = True
    flag = tested & (d > 0.0) & (lhs > rhs)
    undecided = tested & (d > 0.0) & (np.abs(lhs - rhs) <= UNDECIDED_REL * (lhs + rhs))
    srt = np.sort(np.stack(row_neighbours(I)), axis=0)
    repl = 0.5 * (srt[1] + srt[2])
    return flag, repl, undecided


def mask_rows(windows, R, steps=law.ALL):
    n = R + 1 if steps & law.LAST_READ else R
    return min(int(windows[p][0]) for p in range(n)), max(int(windows[p][1]) for p in range(n))


def difference_images(reads, pl, steps, rows):
    """The extraction law's per-pixel quantities on the row slab `rows` (a slice), embedded in full frames that are 0
    elsewhere: I [R, S, S] (I[j] = I_{j+1}), Mpix [R, S, S] (the magnitudes a pixel's I_{j+1} is bounded by),
    LRg [S, S] (L_R g) and its magnitude MR [S, S]."""
    R, S = reads.shape[0] - 1, reads.shape[-1]
    c1, c2, c3, c4 = [c[rows] for c in pl.lin]
    g = pl.gain[rows] if steps & law.GAIN else 1.0
    p0 = reads[0, rows].astype(np.float64)
    I, Mpix = np.zeros((R, S, S)), np.zeros((R, S, S))
    Lp, dp = 0.0, 0.0
    for r in range(1, R + 1):
        D = reads[r, rows].astype(np.float64) - p0
        L = D * (1.0 + c1 + D * (c2 + D * (c3 + c4 * D))) if steps & law.LINEARISE else D
        dk = pl.dark[r, rows] if steps & law.DARK else np.zeros_like(D)
        L = L - dk
        I[r - 1, rows] = (L - Lp) * g
        Mpix[r - 1, rows] = (np.abs(L) + np.abs(Lp) + np.abs(dk) + dp) * g
        Lp, dp = L, np.abs(dk)
    LRg, MR = np.zeros((S, S)), np.zeros((S, S))
    LRg[rows] = (Lp - 0.0) * g
    MR[rows] = (np.abs(Lp) + dp) * g
    return I, Mpix, LRg, MR


def restate(reads, pl, windows, bg, steps=law.ALL, k=8.0, rn=20.0):
    """reads [R + 1, S, S] of any type -> Result(spectra [R + 1, S], sky [R + 1], n_rejected [R + 1], mask [S, S] uint16,
    M [R + 1, S], M_sky [R + 1], undecided [S, S] bool): the extraction law with rejection, the flag plane (bit j =
    flag_j; 0 outside the mask rows), the magnitudes of extraction_law.restate, and the pixels of the mask rows whose
    flag the device may decide the other way in some interval."""
    assert steps & law.GAIN, "the rejection's noise model is in electrons"
    R, S = reads.shape[0] - 1, reads.shape[-1]
    b0, b1 = bg
    m_lo, m_hi = mask_rows(windows, R, steps)
    slab = slice(max(m_lo - 2, 0), min(m_hi + 2, S))
    I, Mpix, LRg, MR = difference_images(reads, pl, steps, slab)
    in_rows = np.zeros((S, 1), dtype=bool)
    in_rows[m_lo:m_hi] = True
    mask = np.zeros((S, S), dtype=np.uint16)
    undecided = np.zeros((S, S), dtype=bool)
    clean, Mclean = I.copy(), Mpix.copy()          # flag_j ? repl_j : I_{j+1}, and what bounds it
    corr, Mcorr = np.zeros((S, S)), np.zeros((S, S))   # sum_j flag_j (I_{j+1} - repl_j), ascending j
    count = np.zeros((R, S, S), dtype=bool)
    for j in range(R):
        f, repl, u = flags(I[j], k, rn)
        f &= in_rows
        undecided |= u & in_rows
        mask[f] |= np.uint16(1 << j)
        nb = np.stack(row_neighbours(Mpix[j])).max(axis=0)
        clean[j][f], Mclean[j][f] = repl[f], nb[f]
        corr[f] += I[j][f] - repl[f]
        Mcorr[f] += Mpix[j][f] + nb[f]
        count[j] = f
    spectra, sky = np.zeros((R + 1, S)), np.zeros(R + 1)
    M, M_sky = np.zeros((R + 1, S)), np.zeros(R + 1)
    n_rejected = np.zeros(R + 1, dtype=np.uint32)
    for p in range(R + 1):
        if p == R and not steps & law.LAST_READ:
            continue
        sl = slice(int(windows[p][0]), int(windows[p][1]))
        if p < R:
            A, Mp = clean[p][sl].sum(axis=0), Mclean[p][sl].sum(axis=0)
            n_rejected[p] = count[p][sl].sum()
        else:
            A, Mp = (LRg[sl] - corr[sl]).sum(axis=0), (MR[sl] + Mcorr[sl]).sum(axis=0)
            n_rejected[p] = count[:, sl].sum()
        scale = pl.dt[p] if p < R else pl.dt.sum()
        B = scale * (pl.sky[sl].sum(axis=0) if steps & law.SKY else np.zeros(S))
        sb = B[b0:b1].sum()
        s = A[b0:b1].sum() / sb if (steps & law.SKY and sb != 0.0) else 0.0
        spectra[p], sky[p] = A - s * B, s
        M[p] = Mp + abs(s) * B
        M_sky[p] = Mp[b0:b1].sum() / abs(sb) if sb != 0.0 else 0.0
    return Result(spectra, sky, n_rejected, mask, M, M_sky, undecided)


def assert_parity(got_spectra, got_sky, want, what=""):
    """The device's (spectra, sky) against a Result, to extraction_law.REL of M per column (and of M_sky)."""
    err = np.abs(np.asarray(got_spectra) - want.spectra)
    worst = float((err / np.maximum(want.M, 1e-300)).max())
    sky_err = np.abs(np.asarray(got_sky) - want.sky)
    worst_sky = float((sky_err / np.maximum(want.M_sky, 1e-300)).max())
    print("%s: worst |spectra - oracle| / M = %.3g, worst |sky - oracle| / M_sky = %.3g (allowed %.0e)" % (
        what, worst, worst_sky, law.REL))
    assert np.isfinite(np.asarray(got_spectra)).all() and np.isfinite(np.asarray(got_sky)).all(), what
    assert (err <= law.REL * want.M).all(), (what, worst)
    assert (sky_err <= law.REL * want.M_sky).all(), (what, worst_sky)
