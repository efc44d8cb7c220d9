"""TEST INFRASTRUCTURE: the law of the device-side ramp fit (include/wayne_hip.h, wayne_rampfit_desc; k_ramp_fit) restated
in numpy, float64 throughout, vectorised over the pixels and looping over the (at most 15) read intervals.  Shared by
tests/test_rampfit.py (the law's own properties, on synthetic ramps and on CPU-oracle reads) and tests/test_rampfit_gpu.py
(the oracle of the device, applied to the slot's own downloaded reads).

For a pixel with reads P_k (k = 0 .. R), L_k / g the extraction's (extraction_law.Planes) and dt_j the read intervals:

    e_0 = 0, e_k = L_k g;   K = the largest K <= R with P_k < sat_dn for all 1 <= k <= K (0 if not P_0 < sat_dn)
    d_j = e_{j+1} - e_j,  r_j = d_j / dt_j,  j in G = {0 .. K-1}
    med(G) = the element of rank floor((|G| - 1) / 2) of {r_j} ascending, ties in order of j; 0 for empty G
    jump test (k_jump > 0), while |G| >= 3:  m = med(G), f0 = max(m, 0),
        z_j = (d_j - m dt_j) / sqrt(f0 dt_j + rn^2),  j* = the lowest j of the largest z_j,
        z_j* > k_jump ? G <- G \\ {j*}, bit j* of `jump` : stop
    fit: f0 = max(med(G), 0), a_j = f0 dt_j + rn^2, o = -rn^2 / 2: generalised least squares of d = f dt with
        cov(d_j, d_j) = a_j, cov(d_j, d_j+1) = o where both are in G, solved by the tridiagonal recurrence of solve()
    rate = den > 0 ? num / den : 0,  var = den > 0 ? 1 / den : 0,  word = K << 16 | jump

Parity bounds (tests/test_rampfit_gpu.py; derived, not tuned): a float64 chain of ~1e2 operations on a matrix whose
condition number is below ~1e3 errs by ~1e-12; the tests allow |rate - law| <= 1e-9 M with
M = (sum |w_j d_j| + |rate| sum |w_j| dt_j) / |den| and var to 4e-9 of itself -- room for contracted multiply-adds, while
a float32 step anywhere misses them by 1e2.  `word` must be equal except where the deciding z_j* lies within 1e-9
relative of k_jump (`margin`, returned by fit())."""
import collections

import numpy as np

LINEARISE, DARK, GAIN = 1, 2, 4
REL_RATE, REL_VAR, REL_DECIDE, MAX_UNDECIDED = 1e-9, 4e-9, 1e-9, 1e-4
DQ_SATURATED, DQ_JUMP = 256, 8192
BORDER = 5

Fit = collections.namedtuple("Fit", "rate var word K jump margin M")


def lower_median(r, G):
    """r, G [R, n] -> med [n]: the element of rank (|G| - 1) // 2 among the members, equal values in order of j; 0 for
    an empty G.  A rank count, as the kernel forms it."""
    R, n = r.shape
    target = (G.sum(axis=0) - 1) // 2
    med = np.zeros(n)
    for j in range(R):
        rank = np.zeros(n, dtype=np.int64)
        for i in range(R):
            if i != j:
                rank += G[i] & ((r[i] < r[j]) | ((r[i] == r[j]) & (i < j)))
        med = np.where(G[j] & (rank == target), r[j], med)
    return med


def solve(d, dt, G, f0, rn):
    """The generalised least squares of d = f dt over the members of G as the law writes it: (num, den, w)."""
    R, n = d.shape
    rn2 = rn * rn
    o = -rn2 / 2
    c, y, w = np.zeros((R, n)), np.zeros((R, n)), np.zeros((R + 1, n))
    no = np.zeros(n, dtype=bool)
    for j in range(R):
        a = f0 * dt[j] + rn2
        link = G[j - 1] if j > 0 else no
        nxt = G[j + 1] if j + 1 < R else no
        den = a - np.where(link, o * c[j - 1], 0.0) if j > 0 else a + np.zeros(n)
        with np.errstate(all="ignore"):
            cj = np.where(nxt, o / den, 0.0)
            yj = (dt[j] - (np.where(link, o * y[j - 1], 0.0) if j > 0 else 0.0)) / den
        c[j] = np.where(G[j], cj, 0.0)
        y[j] = np.where(G[j], yj, 0.0)
    for j in range(R - 1, -1, -1):
        w[j] = y[j] - c[j] * w[j + 1]
    num, den = np.zeros(n), np.zeros(n)
    for j in range(R):
        num = np.where(G[j], num + w[j] * d[j], num)
        den = np.where(G[j], den + w[j] * dt[j], den)
    return num, den, w[:R]


def fit(d, dt, K, rn=20.0, k_jump=5.0):
    """d [R, n] electrons of every interval, dt [R] seconds, K [n] usable intervals -> Fit of the n pixels (word without
    the border's rule; margin: the least |z_j* - k_jump| / k_jump over the pixel's jump passes, inf without one)."""
    d = np.asarray(d, dtype=np.float64)
    dt = np.asarray(dt, dtype=np.float64)
    R, n = d.shape
    K = np.asarray(K, dtype=np.int64)
    G = np.arange(R)[:, None] < K[None, :]
    rn2 = rn * rn
    r = d / dt[:, None]
    jump = np.zeros(n, dtype=np.uint32)
    margin = np.full(n, np.inf)
    idx = np.arange(n)
    if k_jump > 0:
        active = G.sum(axis=0) >= 3
        while active.any():
            m = lower_median(r, G)
            f0 = np.maximum(m, 0.0)
            with np.errstate(all="ignore"):
                z = (d - m[None, :] * dt[:, None]) / np.sqrt(f0[None, :] * dt[:, None] + rn2)
            z = np.where(G & (z == z), z, -np.inf)
            js = np.argmax(z, axis=0)                     # (the first of the largest: the lowest j)
            zmax = z[js, idx]
            with np.errstate(all="ignore"):
                margin = np.where(active, np.minimum(margin, np.abs(zmax - k_jump) / k_jump), margin)
            hit = active & (zmax > k_jump)
            G[js[hit], idx[hit]] = False
            jump[hit] |= (np.uint32(1) << js[hit].astype(np.uint32))
            active = hit & (G.sum(axis=0) >= 3)
    f0 = np.maximum(lower_median(r, G), 0.0)
    num, den, w = solve(d, dt, G, f0, rn)
    ok = den > 0
    with np.errstate(all="ignore"):
        rate = np.where(ok, num / den, 0.0)
        var = np.where(ok, 1.0 / den, 0.0)
        M = np.where(ok, ((np.abs(w * d) * G).sum(axis=0) + np.abs(rate) * (np.abs(w) * G * dt[:, None]).sum(axis=0)) / np.abs(den), 0.0)
    word = (K.astype(np.uint32) << np.uint32(16)) | jump
    return Fit(rate, var, word, K, jump, margin, M)


def electrons(reads, pl, steps=LINEARISE | DARK | GAIN):
    """reads [R + 1, S, S] of any type, pl an extraction_law.Planes -> e [R + 1, S, S]: e_0 = 0, e_k = L_k g."""
    reads = np.asarray(reads)
    P0 = reads[0].astype(np.float64)
    c1, c2, c3, c4 = pl.lin
    e = np.zeros(reads.shape, dtype=np.float64)
    for k in range(1, reads.shape[0]):
        D = reads[k].astype(np.float64) - P0
        L = D * (1.0 + c1 + D * (c2 + D * (c3 + c4 * D))) if steps & LINEARISE else D
        if steps & DARK:
            L = L - pl.dark[k]
        e[k] = L * pl.gain
    return e


def usable(reads, sat_dn):
    """K [S, S]: the samples in front of the first that is not < sat_dn (a NaN is not); 0 if read 0 is not."""
    with np.errstate(invalid="ignore"):
        good = np.asarray(reads).astype(np.float64) < sat_dn
    run = np.cumprod(good, axis=0)                 # 1 while every sample so far is good
    return np.maximum(run.sum(axis=0).astype(np.int64) - 1, 0)


def restate(reads, pl, rn=20.0, k_jump=5.0, sat_dn=65000.0, steps=LINEARISE | DARK | GAIN):
    """The law on a slot's reads [R + 1, S, S]: a Fit of [S, S] planes; the 5-pixel border zero (margin inf there)."""
    reads = np.asarray(reads)
    S = reads.shape[-1]
    e = electrons(reads, pl, steps)
    d = (e[1:] - e[:-1]).reshape(reads.shape[0] - 1, S * S)
    f = fit(d, pl.dt, usable(reads, sat_dn).reshape(S * S), rn, k_jump)
    inner = np.zeros((S, S), dtype=bool)
    inner[BORDER:-BORDER, BORDER:-BORDER] = True
    out = []
    for a, zero in zip(f, (0.0, 0.0, 0, 0, 0, np.inf, 0.0)):
        a = a.reshape(S, S)
        out.append(np.where(inner, a, np.asarray(zero, dtype=a.dtype)))
    return Fit(*out)


def derived(word, dt):
    """(dq uint16, nsamp uint16, time float64) planes of a word plane: what the host derives."""
    word = np.asarray(word, dtype=np.uint32)
    dt = np.asarray(dt, dtype=np.float64)
    R = dt.size
    K, jump = (word >> 16).astype(np.int64), word & np.uint32(0xFFFF)
    dq = np.where(K < R, DQ_SATURATED, 0) | np.where(jump != 0, DQ_JUMP, 0)
    nsamp, time = np.zeros(word.shape, dtype=np.int64), np.zeros(word.shape)
    for j in range(R):
        inG = (j < K) & (((jump >> np.uint32(j)) & 1) == 0)
        nsamp += inG
        time = time + np.where(inG, dt[j], 0.0)
    return dq.astype(np.uint16), nsamp.astype(np.uint16), time


def ensemble_ratio(rates, variances, floor=5.0):
    """rates, variances [n, S, S] of n exposures that differ in their draws alone -> (the mean over the pixels whose
    ensemble mean rate is >= floor of: ensemble variance of the rate / mean predicted variance, those pixels' number)."""
    sel = rates.mean(axis=0) >= floor
    per_pixel = rates[:, sel].var(axis=0, ddof=1) / variances[:, sel].mean(axis=0)
    return float(per_pixel.mean()), int(sel.sum())


def assert_parity(got_rate, got_var, got_word, want, what=""):
    """The device's planes against the law's Fit on the same reads; returns (pixels left out, worst rate error / M,
    worst relative variance error)."""
    got_rate, got_var, got_word = np.asarray(got_rate), np.asarray(got_var), np.asarray(got_word)
    assert got_rate.dtype == np.float64 and got_var.dtype == np.float64 and got_word.dtype == np.uint32, what
    assert got_rate.shape == want.rate.shape == got_var.shape == got_word.shape, what
    border = np.ones(got_rate.shape, dtype=bool)
    border[BORDER:-BORDER, BORDER:-BORDER] = False
    assert not got_rate[border].view(np.uint64).any() and not got_var[border].view(np.uint64).any() and not got_word[border].any(), \
        what + ": the border is not zero to the bit"
    undecided = want.margin <= REL_DECIDE
    differ = got_word != want.word
    agree = ~differ
    err = np.abs(got_rate - want.rate)
    worst = float((err[agree] / np.maximum(want.M[agree], 1e-300)).max())
    verr = np.abs(got_var - want.var)
    worst_v = float((verr[agree] / np.maximum(want.var[agree], 1e-300)).max())
    print("%s: %d of %d pixels left out (deciding z within %.0e of k), %d flagged, %d cut short; worst |rate - law| / M = %.3g "
          "(allowed %.0e), worst |var - law| / var = %.3g (allowed %.0e)" % (
              what, int(undecided.sum()), undecided.size, REL_DECIDE, int((want.jump != 0).sum()),
              int(((want.K > 0) & (want.K < (want.K.max() if want.K.size else 0))).sum()), worst, REL_RATE, worst_v, REL_VAR))
    assert undecided.sum() <= MAX_UNDECIDED * undecided.size, what
    assert not (differ & ~undecided).any(), (what, int((differ & ~undecided).sum()))
    assert np.isfinite(got_rate).all() and np.isfinite(got_var).all(), what
    assert (err[agree] <= REL_RATE * want.M[agree]).all(), (what, worst)
    assert (verr[agree] <= REL_VAR * want.var[agree]).all(), (what, worst_v)
    return int(undecided.sum()), worst, worst_v
