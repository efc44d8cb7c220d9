"""TEST INFRASTRUCTURE: the laws of the profile planes and of the optimal extraction with a supplied profile
(include/wayne_hip.h, wayne_exposure_deliver_profile / wayne_exposure_set_optimal_profile) restated in numpy on top of
tests/optimal_law.py (window_sum, Result, assert_parity), tests/channel_law.py (pixel_terms) and tests/extraction_law.py.
Shared by tests/test_fixed_profile.py (hand-made planes, the ensemble of CPU-oracle exposures) and
tests/test_fixed_profile_gpu.py (the oracle of the device).

Layout of planes and profile: the windows of all R + 1 products one behind the other, rows relative to the window --
[sum_p rows_p, S], product p's rows at offsets(windows)[p].

    planes:   S1(y, x) = sum_{x' in X(x), ascending} d(y, x'),  d = v - sky_p bt  (zeros for a product that is not formed)
    supplied: P = max(Pi, 0),  V = max(spectra_p[x] Pi + sky_p bt, 0) + rn^2 (q q)
              U = sum_y P d / V,  W = sum_y P P / V,  G = sum_y P bt / V
              ok(x) <=> S0 > 0 and S0 S0 > 9 SV0 and W > 0       (S0, SV0 over X(x): H enters here alone)
              optimal_p[x] = ok ? U / W : spectra_p[x],  optimal_var_p[x] = ok ? 1 / W + (G/W)^2 sky_var_p : spectra_var_p[x]

Like optimal_law.restate, both take the device's delivered box arrays as INPUTS, so that d is formed from bit-identical
numbers.  S1 is the same left-to-right sum of the same numbers as the device's: the planes are compared to the bit.  For
the supplied profile only the order of the row sums differs: optimal_law's derived bounds hold unchanged (2e-9 M_U / W,
4e-9 of the variance, fallback columns to the bit)."""
import collections

import numpy as np

import channel_law
import extraction_law as law
import optimal_law

Result = optimal_law.Result
REL = law.REL


def heights(windows):
    return tuple(int(hi) - int(lo) for lo, hi in np.asarray(windows))


def offsets(windows):
    """Row offset of every product's window in the planes, and the total."""
    h = heights(windows)
    return [sum(h[:p]) for p in range(len(h))], sum(h)


def terms(reads, pl, windows, sky, steps=law.ALL, crrej=None):
    """Per product (rows slice, d, bt, q q [rows, S], v) or None where it is not formed."""
    R, S = reads.shape[0] - 1, reads.shape[-1]
    T = pl.sky if steps & law.SKY else np.zeros((S, S))
    out = []
    for p, term in enumerate(channel_law.pixel_terms(reads, pl, windows, steps, crrej)):
        if term is None:
            out.append(None)
            continue
        sl, v, _ = term
        g = pl.gain[sl] if steps & law.GAIN else np.ones((sl.stop - sl.start, S))
        q = g / 2.35
        scale = pl.dt[p] if p < R else pl.dt.sum()
        bt = scale * T[sl]
        out.append((sl, v - sky[p] * bt, bt, q * q, v))
    return out


def planes(reads, pl, windows, H, sky, steps=law.ALL, crrej=None):
    """S1 of every window pixel -> [sum_p rows_p, S]."""
    off, total = offsets(windows)
    out = np.zeros((total, reads.shape[-1]))
    for p, t in enumerate(terms(reads, pl, windows, np.asarray(sky, dtype=np.float64), steps, crrej)):
        if t is not None:
            out[off[p]:off[p] + t[1].shape[0]] = optimal_law.window_sum(t[1], H)
    return out


def normalise(total, windows):
    """extraction.ProfileSum.profile restated: every column of every window over its sum; zeros where that is not > 0."""
    off, _ = offsets(windows)
    out = np.zeros_like(total)
    for o, h in zip(off, heights(windows)):
        w = total[o:o + h]
        tot = w.sum(axis=0)
        good = tot > 0.0
        out[o:o + h][:, good] = w[:, good] / tot[good]
    return out


def restate(reads, pl, windows, H, rn, profile, spectra, sky, spectra_var, sky_var, steps=law.ALL, crrej=None):
    """The optimal extraction with the supplied `profile` [sum_p rows_p, S] -> optimal_law.Result."""
    R, S = reads.shape[0] - 1, reads.shape[-1]
    spectra, spectra_var = np.asarray(spectra, dtype=np.float64), np.asarray(spectra_var, dtype=np.float64)
    sky, sky_var = np.asarray(sky, dtype=np.float64), np.asarray(sky_var, dtype=np.float64)
    rn2 = float(rn) * float(rn)
    off, _ = offsets(windows)
    out = Result(*(np.zeros((R + 1, S)) for _ in range(2)), np.zeros((R + 1, S), dtype=bool), *(np.zeros((R + 1, S)) for _ in range(4)))
    for p, t in enumerate(terms(reads, pl, windows, sky, steps, crrej)):
        if t is None:
            continue
        sl, d, bt, qq, _ = t
        Pr = profile[off[p]:off[p] + d.shape[0]]
        S0, SV0 = optimal_law.window_sum(spectra[p], H), optimal_law.window_sum(spectra_var[p], H)
        detected = (S0 > 0.0) & (S0 * S0 > 9.0 * SV0)
        with np.errstate(all="ignore"):
            P = np.maximum(Pr, 0.0)
            V = np.maximum(spectra[p] * Pr + sky[p] * bt, 0.0) + rn2 * qq
            u, w, gg = (P * d) / V, (P * P) / V, (P * bt) / V
            U, W, G = u.sum(axis=0), w.sum(axis=0), gg.sum(axis=0)
            ok = detected & (W > 0.0)
            GW = G / W
            out.optimal[p] = np.where(ok, U / W, spectra[p])
            out.optimal_var[p] = np.where(ok, 1.0 / W + (GW * GW) * sky_var[p], spectra_var[p])
            out.M_U[p] = np.abs(u).sum(axis=0)
        out.ok[p], out.U[p], out.W[p], out.G[p] = ok, U, W, G
    return out


# ---- the ensemble tests' channels: 10 channels of 13 whole columns over columns 59 .. 188 of small256 (inside the first
# order; optimal_law's COLS) -- with edges on whole columns, one solution for all rows and no flat, a channel of the optimal
# extraction is the sum of its columns of `optimal`, and its variance sum 1 / W plus the sky level's share taken ONCE for
# the channel: (sum G / W)^2 sky_var.  (A fallback column adds its box variance as if independent; the tests assert on
# the last-read product, where every column of the channels is on the optimal branch.)
CHANNEL_COLS, CHANNEL_WIDTH = (59, 189), 13
N_CHANNELS = (CHANNEL_COLS[1] - CHANNEL_COLS[0]) // CHANNEL_WIDTH


def channel_sums(a):
    """[..., S] -> [..., 10]: the columns of each channel added up."""
    a = np.asarray(a, dtype=np.float64)[..., CHANNEL_COLS[0]:CHANNEL_COLS[1]]
    return a.reshape(a.shape[:-1] + (N_CHANNELS, CHANNEL_WIDTH)).sum(axis=-1)


def channel_variance(res, p, spectra_var, sky_var):
    """The predicted variance [10] of product p's channels from a Result (W, G, ok) and the box arrays."""
    with np.errstate(all="ignore"):
        own = np.where(res.ok[p], 1.0 / res.W[p], spectra_var[p])
        k = np.where(res.ok[p], res.G[p] / res.W[p], 0.0)
    return channel_sums(own) + channel_sums(k) ** 2 * sky_var[p]


def ensemble_sd(n):
    """Relative standard deviation of a mean of 10 channels' variance estimates from n exposures: sqrt(2 / (10 (n - 1)))."""
    return float(np.sqrt(2.0 / (N_CHANNELS * (n - 1))))


def channel_figures(optimal, predicted_var, spectra):
    """optimal, spectra [n, S] and predicted_var [n, 10] of one product -> (ensemble variance of the optimal channels / of
    the box channels, ensemble / mean predicted variance, paired bias sum(opt - box) / sum(box), five standard deviations of
    that paired mean, formed from the ensemble's own scatter of the per-exposure differences)."""
    o, s = channel_sums(optimal), channel_sums(spectra)
    n = o.shape[0]
    ratio, bias, predicted = optimal_law.ensemble_figures(o, predicted_var, s, (0, N_CHANNELS))
    diff = (o - s).sum(axis=1)
    bound = 5.0 * diff.std(ddof=1) / np.sqrt(n) / s.mean(axis=0).sum()
    return ratio, predicted, bias, float(bound)


def assert_ensemble(fixed, own, n, what=""):
    """The ensemble assertions on the last-read product's figures (channel_figures of the supplied profile and of the
    exposures' own):
    1. the variance ratio with the supplied profile lies below the own-profile ratio by at least 4 standard deviations of
       their difference, each ratio r taken with the standard deviation r sqrt(2 / (10 (n - 1))) and the two as independent
       (they share the box variances and the reads, which only lowers the difference's scatter);
    2. ensemble / predicted variance within 1 +- 4 sqrt(2 / (10 (n - 1))) (0.32 at n = 32);
    3. |paired bias| within five standard deviations of the paired mean;
    and, as the negative control, the exposures' own profile must FAIL 2: its noise is common to a channel's columns."""
    sd = ensemble_sd(n)
    assert own[0] - fixed[0] >= 4.0 * sd * np.hypot(own[0], fixed[0]), (what, fixed, own)
    assert abs(fixed[1] - 1.0) <= 4.0 * sd, (what, fixed)
    assert abs(fixed[2]) <= fixed[3], (what, fixed)
    assert abs(own[1] - 1.0) > 4.0 * sd, (what, own)


# ---- the optimal channels (wayne_exposure_set_optimal_channels): w_b and F are the channels' law's (channel_law), d, bt, P,
# V those of the optimal law with either profile source, W_p[x] = sum_y P P / V and ok(x) as above:
#     e = ok ? ((P d) / V) / W : d,   k = ok ? ((P bt) / V) / W : bt,   ev = ok ? ((P P) / V) / (W W) : max(v, 0) + rn^2 q q
#     channels_opt_p[b] = sum w_b e / F,  K_p[b] = sum w_b k / F,  channels_opt_var_p[b] = sum w_b^2 ev / F^2 + K_p[b]^2 sky_var_p
# Tolerance (derived as channel_law's): only the order of the sums differs -- at most 4e5 terms, 4e-11 of the sum of absolute
# terms M_p[b] = sum w_b |e| / F; the tests allow extraction_law.REL = 1e-9 of it, and 4 REL of channels_opt_var itself (its
# terms are non-negative; W's own rounding enters e once and ev twice, K's square twice).
ChannelResult = collections.namedtuple("ChannelResult", "channels_opt channels_opt_var M K EV ok")


def bin_rows_pow(values, rows, edges, wl_a, wl_b, power):
    """channel_law.bin_rows with w_b^power."""
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
        w = w if power == 1 else w * w
        for k, val in enumerate(values):
            out[k, c] = (w * val[:, x0:x1]).sum()
    return out


def channels(reads, pl, windows, H, rn, profile, spectra, sky, spectra_var, sky_var, edges, wl_a, wl_b, steps=law.ALL, flat=None,
             crrej=None, mutate=None):
    """The optimal channels -> ChannelResult([R + 1, C] each).  `profile`: the supplied planes, or None for the exposure's
    own S1 / S0.  `mutate`: one of the hand mutations ("w", "no_sky") -- for the test that shows the parity test sees them."""
    R, S = reads.shape[0] - 1, reads.shape[-1]
    spectra, spectra_var = np.asarray(spectra, dtype=np.float64), np.asarray(spectra_var, dtype=np.float64)
    sky, sky_var = np.asarray(sky, dtype=np.float64), np.asarray(sky_var, dtype=np.float64)
    rn2 = float(rn) * float(rn)
    off, _ = offsets(windows)
    C = len(edges) - 1
    F = channel_law.flat_factor(flat, wl_a, wl_b, S)
    out = ChannelResult(*(np.zeros((R + 1, C)) for _ in range(5)), np.zeros((R + 1, S), dtype=bool))
    for p, t in enumerate(terms(reads, pl, windows, sky, steps, crrej)):
        if t is None:
            continue
        sl, d, bt, qq, v = t
        S0, SV0 = optimal_law.window_sum(spectra[p], H), optimal_law.window_sum(spectra_var[p], H)
        detected = (S0 > 0.0) & (S0 * S0 > 9.0 * SV0)
        with np.errstate(all="ignore"):
            Pr = profile[off[p]:off[p] + d.shape[0]] if profile is not None else optimal_law.window_sum(d, H) / S0
            P = np.maximum(Pr, 0.0)
            V = np.maximum(spectra[p] * Pr + sky[p] * bt, 0.0) + rn2 * qq
            u, w, gg = (P * d) / V, (P * P) / V, (P * bt) / V
            W = w.sum(axis=0)
            ok = detected & (W > 0.0)
            e = np.where(ok, u / W, d)
            k = np.where(ok, gg / W, bt)
            ev = np.where(ok, w / (W * W), np.maximum(v, 0.0) + rn2 * qq)
        Fs = F[sl]
        E, K, M = bin_rows_pow([e / Fs, k / Fs, np.abs(e) / Fs], sl, edges, wl_a, wl_b, 1)
        EV = bin_rows_pow([ev / (Fs * Fs)], sl, edges, wl_a, wl_b, 1 if mutate == "w" else 2)[0]
        out.channels_opt[p], out.M[p], out.K[p], out.EV[p], out.ok[p] = E, M, K, EV, ok
        out.channels_opt_var[p] = EV + (0.0 if mutate == "no_sky" else (K * K) * sky_var[p])
    return out


def assert_channel_parity(got, got_var, want, what=""):
    got, got_var = np.asarray(got), np.asarray(got_var)
    assert got.shape == want.channels_opt.shape == got_var.shape, what
    err, err_var = np.abs(got - want.channels_opt), np.abs(got_var - want.channels_opt_var)
    worst = float((err / np.maximum(want.M, 1e-300)).max())
    worst_var = float((err_var / np.maximum(want.channels_opt_var, 1e-300)).max())
    print("%s: worst |channels_opt - oracle| / M = %.3g (allowed %.0e), worst relative |channels_opt_var - oracle| = %.3g "
          "(allowed %.0e)" % (what, worst, REL, worst_var, 4 * REL))
    assert np.isfinite(got).all() and np.isfinite(got_var).all(), what
    assert (err <= REL * want.M).all(), (what, worst)
    assert (err_var <= 4.0 * REL * want.channels_opt_var).all(), (what, worst_var)


def delivered_figures(channels_opt, channels_opt_var, channels):
    """channels_opt, channels_opt_var and the box channels [n, C] of one product as delivered -> the tuple of
    channel_figures: (variance ratio, ensemble / predicted variance, paired bias, five standard deviations of it)."""
    o, s = np.asarray(channels_opt, dtype=np.float64), np.asarray(channels, dtype=np.float64)
    ratio, bias, predicted = optimal_law.ensemble_figures(o, channels_opt_var, s, (0, o.shape[1]))
    diff = (o - s).sum(axis=1)
    return ratio, predicted, bias, float(5.0 * diff.std(ddof=1) / np.sqrt(o.shape[0]) / s.mean(axis=0).sum())
