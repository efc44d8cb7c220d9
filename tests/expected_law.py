"""The law of the noise-free expected image (include/wayne_hip.h, "the noise-free expected image"), in numpy, float64.

A thrower keeps an electron of a bin at c iff 0 < floor(c + sigma z) < N on both axes, so with Phi the standard normal
CDF the chance that it lands in frame pixel (y, x) is a_x a_y,

    a(p; c, sigma) = Phi((p + 1 - c) / sigma) - Phi((p - c) / sigma)     for 1 <= p <= N - 1, else 0,

and for n independent electrons of a component the pixel's count has

    E = n a_x a_y        V = n a_x a_y (1 - a_x a_y)

(one cell of a multinomial).  expected_image adds the components, bins, sub-samples and sources up:

    E_r[y + 5, x + 5] = sum f_{s,k}(y, x)   sum_w ( n_h a(x; xs, sigma_h) a(y; ys, sigma_h) + n_l a(..sigma_l) a(..sigma_l) )
    V_r[y + 5, x + 5] = sum f_{s,k}(y, x)^2 sum_w ( n a_x a_y (1 - a_x a_y), both components )

V is the variance of the thrower's accumulators GIVEN the bins' counts (n_h, n_l): what a frame scatters by around the
E of mode "counts".  Per sub-sample and component the sums over the bins are matrix products over the bins' 8 sigma box
(the device's own cut is never wider: what lies outside is below 2 Phi(-8) of the electrons).
"""
import numpy as np
from scipy.special import erf, erfc

BORDER = 5
CULL = 8.0
PHI_M8 = 6.220960574271785e-16          # Phi(-8)
INT_MAX = 2147483647.0


def cell_mass(p, c, sigma, N):
    """a(p; c, sigma) for integer pixels p (broadcast against c and sigma), each difference formed on the tail side."""
    p = np.asarray(p)
    pf = p.astype(np.float64)
    s = 0.70710678118654752440
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t0 = ((pf - c) / sigma) * s
        t1 = ((pf + 1.0 - c) / sigma) * s
        right = 0.5 * (erfc(t0) - erfc(t1))               # the bin lies left of the pixel
        left = 0.5 * (erfc(-t1) - erfc(-t0))              # ... right of it
        mid = 0.5 * (erf(t1) + erf(-t0))                  # ... inside it
        a = np.where(t0 >= 0.0, right, np.where(t1 <= 0.0, left, mid))
    return np.where((p >= 1) & (p <= N - 1), a, 0.0)


def literal_image(N, xs, ys, n, sigma):
    """sum_w n_w a(x; xs_w, sigma_w) a(y; ys_w, sigma_w) over the whole N x N frame, bin by bin: the definition as it
    is written, for the toy tests."""
    img = np.zeros((N, N))
    p = np.arange(N)
    for x, y, k, s in zip(xs, ys, n, sigma):
        img += k * np.outer(cell_mass(p, y, s, N), cell_mass(p, x, s, N))
    return img


def split_counts(counts, ratio):
    """Mode "counts": (n_h, n_l) of bins holding `counts` electrons -- nwide = (int)(count ratio) (pyparallel_menu.c:89),
    n_h = min(max(nwide, 0), count), n_l = count - n_h.  counts [K, W] (or [W]), ratio [W]."""
    c = np.asarray(counts, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        nw = np.trunc(c * np.asarray(ratio, dtype=np.float64))
    nw = np.where(np.isfinite(nw), nw, 0.0)
    n_h = np.minimum(np.maximum(nw, 0.0), c)
    return n_h, c - n_h


def split_mean(lam, ratio):
    """Mode "mean": lambda+ = lambda finite and > 0 ? min(lambda, 2^31 - 1) : 0; n_h = min(max(ratio, 0), 1) lambda+."""
    lam = np.asarray(lam, dtype=np.float64)
    lp = np.where(np.isfinite(lam) & (lam > 0.0), np.minimum(lam, INT_MAX), 0.0)
    rho = np.minimum(np.maximum(np.nan_to_num(np.asarray(ratio, dtype=np.float64), nan=0.0), 0.0), 1.0)
    n_h = rho * lp
    return n_h, lp - n_h


def _component(N, xs, ys, n, sigma):
    """(x0, y0, E, V) of one component of one sub-sample: E, V on the box [y0, y0 + h) x [x0, x0 + w) of the bins that
    count (n > 0, a position inside +-1e6, a finite sigma > 0); None when there is none."""
    with np.errstate(invalid="ignore"):
        ok = (n > 0) & (np.abs(xs) < 1e6) & (np.abs(ys) < 1e6) & (sigma > 0) & np.isfinite(sigma)
    if not ok.any():
        return None
    xs, ys, n, sigma = xs[ok], ys[ok], n[ok], sigma[ok]
    reach = CULL * sigma.max() + 1.0
    x0, x1 = max(int(np.floor(xs.min() - reach)), 1), min(int(np.floor(xs.max() + reach)) + 1, N)
    y0, y1 = max(int(np.floor(ys.min() - reach)), 1), min(int(np.floor(ys.max() + reach)) + 1, N)
    if x0 >= x1 or y0 >= y1:
        return None
    ax = cell_mass(np.arange(x0, x1)[None, :], xs[:, None], sigma[:, None], N)     # [bins, w]
    ay = cell_mass(np.arange(y0, y1)[None, :], ys[:, None], sigma[:, None], N)     # [bins, h]
    nay = n[:, None] * ay
    E = nay.T @ ax
    V = E - (nay * ay).T @ (ax * ax)
    return x0, y0, E, V


def expected_image(N, R, sample_read, sources):
    """(E, V) [R, S, S], S = N + 10.  sample_read [K]: the read interval sub-sample k closes.  sources: one dict per
    source (the target first), with
        x, y           [K, W] bin positions in frame coordinates
        n_h, n_l       [K, W] electrons of the wide / the narrow component (split_counts or split_mean)
        sig_h, sig_l   [W]    the components' sigmas, AS THE THROWERS USE THEM: float32 values
        flat           None, or a function k -> [N, N] array: f of sub-sample k for this source"""
    S = N + 2 * BORDER
    E = np.zeros((R, S, S))
    V = np.zeros((R, S, S))
    for src in sources:
        sh = np.asarray(src["sig_h"], dtype=np.float32).astype(np.float64)
        sl = np.asarray(src["sig_l"], dtype=np.float32).astype(np.float64)
        for k, r in enumerate(np.asarray(sample_read)):
            f = None if src.get("flat") is None else np.asarray(src["flat"](k), dtype=np.float64)
            for n, sig in ((src["n_h"][k], sh), (src["n_l"][k], sl)):
                got = _component(N, np.asarray(src["x"][k], dtype=np.float64), np.asarray(src["y"][k], dtype=np.float64),
                                 np.asarray(n, dtype=np.float64), sig)
                if got is None:
                    continue
                x0, y0, e, v = got
                h, w = e.shape
                if f is not None:
                    fk = f[y0:y0 + h, x0:x0 + w]
                    e, v = fk * e, fk * fk * v
                E[r, y0 + BORDER:y0 + BORDER + h, x0 + BORDER:x0 + BORDER + w] += e
                V[r, y0 + BORDER:y0 + BORDER + h, x0 + BORDER:x0 + BORDER + w] += v
    return E, V


def culling_bound(electrons_r):
    """A_r: what the device's 8 sigma cut can take from any pixel of interval r, which holds `electrons_r` electrons."""
    return 2.0 * PHI_M8 * np.asarray(electrons_r, dtype=np.float64)


def chi2_per_pixel(frame, E, V, v_min=5.0):
    """(mean((frame - E)^2 / V) over the pixels with V >= v_min, their number)."""
    m = V >= v_min
    n = int(m.sum())
    return (float((((frame - E) ** 2)[m] / V[m]).mean()) if n else float("nan")), n


def flat_of(flat_cube, wmin, wmax, N, flat_off, grism_trace, x_ref, y_ref):
    """f of one sub-sample (flat_value of k_throw.h; grism.py:362-385): the float32-rounded cubic in the wavelength a
    pixel would see from a star at (x_ref, y_ref).  flat_cube: the four [N, N] float32 planes; grism_trace: (m_t, m_w,
    c_w) = the trace slope and the wavelength solution along the trace for that star position."""
    m_t, a_w, b_w = grism_trace
    a_t_i = 1.0 / m_t
    inv_norm = 1.0 / np.sqrt(a_t_i * a_t_i + 1.0)
    yy, xx = np.mgrid[0:N, 0:N]
    arr = y_ref - (yy + flat_off).astype(np.float64) + a_t_i * x_ref - a_t_i * (xx + flat_off).astype(np.float64)
    d = np.abs(arr) * inv_norm
    wl = a_w * d + b_w
    t = (wl - wmin) * (1.0 / (wmax - wmin))
    t2 = t * t
    t3 = t2 * t
    f = flat_cube[0].astype(np.float64) + flat_cube[1].astype(np.float64) * t + flat_cube[2].astype(np.float64) * t2 + \
        flat_cube[3].astype(np.float64) * t3
    return f.astype(np.float32).astype(np.float64)
