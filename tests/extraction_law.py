"""TEST INFRASTRUCTURE: the law of the device-side spectral extraction (include/wayne_hip.h, wayne_extract_desc) restated
in numpy, per column, with the error budget of an exact float64 summation.  Shared by tests/test_extraction.py (against
the observer's extraction of tests/visit_science.py) and tests/test_extraction_gpu.py (the oracle of the device).

Tolerance (derived, not tuned): an exact float64 summation of n <= 1024 rows errs by at most ~n 2^-49 of
M[x] = sum_y (|L_r| + |L_{r-1}| + |dark_r| + |dark_{r-1}|) g (+ |sky_j| B_j[x]); the tests allow 1e-9 M[x] per column --
~2^10 above that bound, which covers a contracted multiply-add in the pixel's chain, while a float32 accumulation
anywhere misses it by a factor of ~60 -- and the same relative bound on the sky level.
"""
import numpy as np

LINEARISE, DARK, GAIN, SKY, LAST_READ, ALL = 1, 2, 4, 8, 16, 31
REL = 1e-9


class Planes(object):
    """The calibration planes of a synthetic.Visit's mode, bordered and in float64 (as tests/visit_science.py holds them)."""

    def __init__(self, v):
        N = 1014 if v.SUBARRAY == 1024 else v.SUBARRAY
        self.S = S = N + 10
        read_times = np.asarray(v.read_times, dtype=float)
        planes = v.calibration.for_mode(v.grism.name, v.SUBARRAY, v.SAMPSEQ, read_times, detector=v.detector)
        self.lin = [np.asarray(p, dtype=np.float64) for p in planes["lin"]]
        self.dark = np.concatenate([np.zeros((1, S, S)), np.asarray(planes["dark_sci"], dtype=np.float64)])
        self.gain = np.full((S, S), 2.35)
        self.gain[5:-5, 5:-5] = 2.35 / np.asarray(planes["pfl"], dtype=np.float64)
        self.sky = np.zeros((S, S))
        self.sky[5:-5, 5:-5] = np.asarray(planes["sky"], dtype=np.float64)
        self.dt = np.diff(np.concatenate([[0.0], read_times]))


def restate(reads, pl, windows, bg, steps=ALL):
    """reads [R + 1, S, S] of any type -> (spectra [R + 1, S], sky [R + 1], M [R + 1, S], M_sky [R + 1]): the law, and
    the magnitudes its float64 sums are bounded by (see the module's docstring)."""
    R, S = reads.shape[0] - 1, reads.shape[-1]
    b0, b1 = bg
    spectra, sky = np.zeros((R + 1, S)), np.zeros(R + 1)
    M, M_sky = np.zeros((R + 1, S)), np.zeros(R + 1)
    c1, c2, c3, c4 = pl.lin

    def linear(r, sl):
        """(L_r, |dark_r|) on the rows `sl`"""
        if r == 0:
            return 0.0, 0.0
        D = reads[r, sl].astype(np.float64) - reads[0, sl].astype(np.float64)
        L = D * (1.0 + c1[sl] + D * (c2[sl] + D * (c3[sl] + c4[sl] * D))) if steps & LINEARISE else D
        dk = pl.dark[r, sl] if steps & DARK else np.zeros_like(D)
        return L - dk, np.abs(dk)

    for p in range(R + 1):
        if p == R and not steps & LAST_READ:
            continue
        lo, hi = int(windows[p][0]), int(windows[p][1])
        sl = slice(lo, hi)
        Lh, dh = linear(p + 1 if p < R else R, sl)
        Ll, dl = linear(p if p < R else 0, sl)
        g = pl.gain[sl] if steps & GAIN else 1.0
        A = ((Lh - Ll) * g).sum(axis=0)
        scale = pl.dt[p] if p < R else pl.dt.sum()
        B = scale * (pl.sky[sl].sum(axis=0) if steps & SKY else np.zeros(S))
        sb = B[b0:b1].sum()
        s = A[b0:b1].sum() / sb if (steps & SKY and sb != 0.0) else 0.0
        spectra[p], sky[p] = A - s * B, s
        Mp = ((np.abs(Lh) + np.abs(Ll) + dh + dl) * g).sum(axis=0) * np.ones(S)
        M[p] = Mp + abs(s) * B
        M_sky[p] = Mp[b0:b1].sum() / abs(sb) if sb != 0.0 else 0.0
    return spectra, sky, M, M_sky


def assert_parity(got_spectra, got_sky, reads, pl, windows, bg, steps=ALL, what=""):
    """The device's (spectra, sky) against the restatement on the same reads, to REL of M per column (and of M_sky)."""
    want, want_sky, M, M_sky = restate(reads, pl, windows, bg, steps)
    err = np.abs(np.asarray(got_spectra) - want)
    worst = float((err / np.maximum(M, 1e-300)).max())
    sky_err = np.abs(np.asarray(got_sky) - want_sky)
    worst_sky = float((sky_err / np.maximum(M_sky, 1e-300)).max())
    print("%s: worst |spectra - oracle| / M = %.3g, worst |sky - oracle| / M_sky = %.3g (allowed %.0e)" % (
        what, worst, worst_sky, REL))
    assert np.isfinite(np.asarray(got_spectra)).all() and np.isfinite(np.asarray(got_sky)).all(), what
    assert (err <= REL * M).all(), (what, worst)
    assert (sky_err <= REL * M_sky).all(), (what, worst_sky)
    return want, want_sky, M
