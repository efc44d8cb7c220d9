"""TEST INFRASTRUCTURE: the law of the extraction's variances (include/wayne_hip.h, wayne_variance_desc) restated in
numpy on top of tests/extraction_law.py, tests/crrej_law.py and tests/channel_law.py.  Shared by tests/test_variance.py
(properties of the law, the ensemble of CPU-oracle exposures) and tests/test_variance_gpu.py (the oracle of the device).

    var_p(y, x)       = max(v, 0) + rn^2 (q q),   q = g / 2.35
    VA_p[x]           = sum_{y in window p} var_p(y, x)
    sky_var_p         = sum_{x in bg} VA_p[x] / (sum_{x in bg} B_p[x])^2     (0 where sky_p is 0 by its rule)
    spectra_var_p[x]  = VA_p[x] + (B_p[x] B_p[x]) sky_var_p
    VP_p[b]           = sum_y sum_x (w_b w_b) (var_p / (F F))
    channels_var_p[b] = VP_p[b] + (Q_p[b] Q_p[b]) sky_var_p

v is the term the column extraction sums for the pixel (channel_law.pixel_terms: under rejection the cleaned value), g
the gain factor (extraction_law.Planes.gain; 1 when the GAIN step is off -- which the library refuses), B_p, Q_p, w_b
and F those of extraction_law and channel_law.

Tolerance (derived, not tuned): every term of every sum is >= 0, and a pixel's var is formed on the device with the
operations written here in this order, from a v and a g that are bit-identical (the library is compiled without
contraction), so the two sides differ by the order of their float64 sums alone.  A sum of n non-negative terms in any
order errs by at most n 2^-53 of the sum itself: n <= 1024 rows x 384 columns ~ 4e5 gives 4e-11, and the few products
and quotients that combine such sums (B^2 sky_var, Q^2 sky_var, sky_var's quotient; B, Q and the background sums are
sums of non-negative terms too) add a few 2^-53 each.  The tests allow extraction_law.REL = 1e-9 of the variance itself
-- no magnitude beside it is needed, there is no cancellation.  A float32 accumulation anywhere misses that by orders of
magnitude; so does any missing or extra term of the law.
"""
import collections

import numpy as np

import channel_law
import extraction_law as law

REL = law.REL
Result = collections.namedtuple("Result", "spectra_var sky_var channels_var VA B VP Q")


def pixel_variances(reads, pl, windows, rn, steps=law.ALL, crrej=None):
    """Per product p (None where it is not formed): (rows slice, var [rows, S]).  `crrej`: (k, rn_of_the_rejection)."""
    S = reads.shape[-1]
    out = []
    rn2 = float(rn) * float(rn)
    for term in channel_law.pixel_terms(reads, pl, windows, steps, crrej):
        if term is None:
            out.append(None)
            continue
        sl, v, _ = term
        g = pl.gain[sl] if steps & law.GAIN else np.ones((sl.stop - sl.start, S))
        q = g / 2.35
        out.append((sl, np.maximum(v, 0.0) + rn2 * (q * q)))
    return out


def bin_rows_squared(values, rows, edges, wl_a, wl_b):
    """sum_y sum_x w_b(y, x)^2 values[y - rows.start, x] for every channel b -> [C] (channel_law.bin_rows with w w)."""
    S = values.shape[1]
    a = np.asarray(wl_a, dtype=np.float64)[rows][:, None]
    b = np.asarray(wl_b, dtype=np.float64)[rows][:, None]
    e = np.asarray(edges, dtype=np.float64)
    C = e.size - 1
    out = np.zeros(C)
    ua = [(e[i] - a) / b for i in range(C + 1)]
    for c in range(C):
        x0 = int(min(max(np.floor(ua[c].min()), 0.0), float(S)))
        x1 = int(min(max(np.ceil(ua[c + 1].max()), 0.0), float(S)))
        if x1 <= x0:
            continue
        x = np.arange(x0, x1, dtype=np.float64)[None, :]
        w = np.minimum(np.maximum(np.minimum(x + 1.0, ua[c + 1]) - np.maximum(x, ua[c]), 0.0), 1.0)
        out[c] = ((w * w) * values[:, x0:x1]).sum()
    return out


def restate(reads, pl, windows, bg, rn, steps=law.ALL, crrej=None, edges=None, wl_a=None, wl_b=None, flat=None):
    """reads [R + 1, S, S] of any type -> Result(spectra_var [R + 1, S], sky_var [R + 1], channels_var [R + 1, C] or None
    without `edges`, VA [R + 1, S], B [R + 1, S], VP, Q [R + 1, C] or None).  `rn`: the read noise of the variances;
    `crrej`: (k, rn) of the rejection or None; `flat`: a channel_law.Flat when the channels divide by the cube."""
    R, S = reads.shape[0] - 1, reads.shape[-1]
    b0, b1 = bg
    with_channels = edges is not None
    C = len(edges) - 1 if with_channels else 0
    spectra_var, sky_var = np.zeros((R + 1, S)), np.zeros(R + 1)
    VA, B = np.zeros((R + 1, S)), np.zeros((R + 1, S))
    channels_var, VP, Q = (np.zeros((R + 1, C)) for _ in range(3)) if with_channels else (None, None, None)
    F = channel_law.flat_factor(flat, wl_a, wl_b, S) if with_channels else None
    T = pl.sky if steps & law.SKY else np.zeros((S, S))
    for p, term in enumerate(pixel_variances(reads, pl, windows, rn, steps, crrej)):
        if term is None:
            continue
        sl, var = term
        scale = pl.dt[p] if p < R else pl.dt.sum()
        VA[p] = var.sum(axis=0)
        B[p] = scale * T[sl].sum(axis=0)
        sb = B[p, b0:b1].sum()
        sky_var[p] = VA[p, b0:b1].sum() / (sb * sb) if (steps & law.SKY and sb != 0.0) else 0.0
        spectra_var[p] = VA[p] + (B[p] * B[p]) * sky_var[p]
        if with_channels:
            VP[p] = bin_rows_squared(var / (F[sl] * F[sl]), sl, edges, wl_a, wl_b)
            Q[p] = scale * channel_law.bin_rows([T[sl] / F[sl]], sl, edges, wl_a, wl_b)[0]
            channels_var[p] = VP[p] + (Q[p] * Q[p]) * sky_var[p]
    return Result(spectra_var, sky_var, channels_var, VA, B, VP, Q)


def _worst(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    return err, float((err / np.maximum(want, 1e-300)).max()) if want.size else 0.0


def assert_parity(got_spectra_var, got_sky_var, got_channels_var, want, what=""):
    """The device's variances against a Result, to REL of each variance itself (a zero must be a zero)."""
    pairs = [("spectra_var", got_spectra_var, want.spectra_var), ("sky_var", got_sky_var, want.sky_var)]
    if want.channels_var is None:
        assert got_channels_var is None, what
    else:
        pairs.append(("channels_var", got_channels_var, want.channels_var))
    checked = [(name, np.asarray(g), np.asarray(w)) + _worst(g, w, what + ": " + name) for name, g, w in pairs]
    print("%s: worst relative |variance - oracle|: %s (allowed %.0e)" % (
        what, ", ".join("%s %.3g" % (name, worst) for name, _, _, _, worst in checked), REL))
    for name, g, w, err, worst in checked:
        assert np.isfinite(g).all() and (g >= 0.0).all(), (what, name)
        assert (err <= REL * w).all(), (what, name, worst)


def ensemble_ratio(channels, channels_var, channels_var_rn0):
    """The ensemble test's statistic.  channels, channels_var [N, R + 1, C] of N exposures that differ in their random
    draws alone, channels_var_rn0 the same exposures' variances at read_noise = 0 (their Poisson parts) ->
    (pooled ratio, per-channel ratios [C]) of the ensemble variance (N - 1 in the denominator) of X =
    channels[:R].sum(0) to the ensemble mean of its predicted variance

        channels_var_rn0[:R].sum(0) + (channels_var[R] - channels_var_rn0[R])

    -- the Poisson parts of the read intervals add; their read noise does not: consecutive intervals share a read, so
    in the sum every pixel keeps the noise of the first and the last read that cover it alone, which is the read-noise
    part of the last-read product, whose window is the union of the intervals' (include/wayne_hip.h, wayne_variance_desc:
    "Left out").  With independent channels (edges on integer columns) C (N - 1) times the pooled ratio follows a
    chi-square law with C (N - 1) degrees of freedom."""
    channels, cv, cv0 = (np.asarray(a, dtype=np.float64) for a in (channels, channels_var, channels_var_rn0))
    R = channels.shape[1] - 1
    X = channels[:, :R].sum(axis=1)
    predicted = (cv0[:, :R].sum(axis=1) + (cv[:, R] - cv0[:, R])).mean(axis=0)
    per_channel = X.var(axis=0, ddof=1) / predicted
    return float(per_channel.mean()), per_channel
