"""An independent float64 restatement of the charge-trapping model (wayne_amd/traps.py, k_ramp.h k_ramp_trap) for the
tests: the ODE, its exact step, a brute-force replay of a visit's schedule, the start-table interpolation and the
read-by-read trapping of whole frames.  It shares no code with the package."""
import math

import numpy as np

GAIN = 2.35          # e- per DN (detector.py:30)
BORDER = 5           # reference pixels on each side of a frame


def rhs(E, f, eta, N, tau):
    return eta * f * (1.0 - E / N) - E / tau


def rk4(E, f, dt, eta, N, tau, n):
    """n classical Runge-Kutta steps of the ODE over dt at constant f."""
    h = dt / n
    for _ in range(n):
        k1 = rhs(E, f, eta, N, tau)
        k2 = rhs(E + 0.5 * h * k1, f, eta, N, tau)
        k3 = rhs(E + 0.5 * h * k2, f, eta, N, tau)
        k4 = rhs(E + h * k3, f, eta, N, tau)
        E = E + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return E


def exact(E, f, dt, eta, N, tau):
    """The closed form: relaxation towards E_inf at rate c."""
    c = eta * f / N + 1.0 / tau
    e_inf = eta * f / c
    return e_inf + (E - e_inf) * np.exp(-c * dt)


def replay(schedule, E0, eta, N, tau, fill, step_s=None):
    """Brute-force replay of a visit: `schedule` is a list of ("lit", seconds, rate), ("dark", seconds) and ("orbit",)
    events; E0, eta, N, tau, fill per population (arrays broadcasting against the rates).  Integrated with RK4 in steps
    of at most step_s seconds (default: a tenth of the shortest time constant).  Returns the occupancy after each
    ("mark",) event."""
    E = np.array(E0, dtype=np.float64)
    marks = []
    for ev in schedule:
        if ev[0] == "mark":
            marks.append(E.copy())
        elif ev[0] == "orbit":
            E = np.minimum(E + fill, N)
        else:
            dt = ev[1]
            f = ev[2] if ev[0] == "lit" else 0.0
            c = np.max(eta * np.asarray(f) / N + 1.0 / tau)
            h = step_s or 0.1 / c
            E = rk4(E, f, dt, eta, N, tau, max(int(math.ceil(dt / h)), 1))
    return marks


def interp(table, f, rate_lo, rate_hi):
    """[2, G] table at rates f: point 0 at f = 0, points 1 .. G-1 log-spaced rate_lo .. rate_hi; linear in f below
    rate_lo, linear in ln f above, clamped."""
    G = table.shape[1]
    f = np.asarray(f, dtype=np.float64)
    out = np.empty((2,) + f.shape)
    step = math.log(rate_hi / rate_lo) / (G - 2) if G > 2 else 1.0
    flat = f.ravel()
    res = np.empty((2, flat.size))
    for j, x in enumerate(flat):
        for p in range(2):
            e = table[p]
            if not x > 0:
                res[p, j] = e[0]
            elif x < rate_lo:
                res[p, j] = e[0] + (e[1] - e[0]) * (x / rate_lo)
            else:
                u = (math.log(x) - math.log(rate_lo)) / step if G > 2 else 0.0
                if not u < G - 2:
                    res[p, j] = e[G - 1]
                else:
                    i = int(u)
                    res[p, j] = e[1 + i] + (e[2 + i] - e[1 + i]) * (u - i)
    out[:] = res.reshape((2,) + f.shape)
    return out


def interp_fast(table, f, rate_lo, rate_hi):
    """interp, vectorised (whole frames)."""
    G = table.shape[1]
    f = np.asarray(f, dtype=np.float64)
    step = math.log(rate_hi / rate_lo) / (G - 2) if G > 2 else 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (np.log(np.where(f > 0, f, rate_lo)) - math.log(rate_lo)) / step if G > 2 else np.zeros_like(f)
    i = np.clip(u.astype(np.int64), 0, max(G - 3, 0))
    out = np.empty((2,) + f.shape)
    for p in range(2):
        e = table[p]
        mid = e[np.minimum(1 + i, G - 1)] + (e[np.minimum(2 + i, G - 1)] - e[np.minimum(1 + i, G - 1)]) * (u - i)
        v = np.where(u < G - 2, mid, e[G - 1])
        v = np.where(f < rate_lo, e[0] + (e[1] - e[0]) * (f / rate_lo), v)
        out[p] = np.where(f > 0, v, e[0])
    return out


def trapped_reads(reads_off, acc, sky_plane, bg, read_dt, table, rate_lo, rate_hi, eta, N, tau):
    """The reads of a trapped exposure, from the float64 reads of the same exposure without traps (same draws).
    reads_off [R+1, S, S] DN, gain variations off; acc [R, S, S] the accumulator electrons (debug_fetch); sky_plane
    [S, S] the master sky as the device holds it (float32, zero border); bg [R] the per-read sky counts per unit master
    sky (float32); read_dt [R] s; table [2, G].  Returns (reads [R+1, S, S], trapped electrons [R, S, S] since the zero
    read, collected electrons [R, S, S] per interval)."""
    R, S = acc.shape[0], acc.shape[1]
    dN = np.diff(reads_off, axis=0) * GAIN                        # collected electrons per interval (sky draws included)
    sky_px = np.where(sky_plane > 0, sky_plane.astype(np.float64), 0.0)
    sum_bg = 0.0
    for b in bg:
        sum_bg += float(np.float32(b))
    sum_dt = 0.0
    for d in read_dt:
        sum_dt += float(d)
    fbar = (acc.sum(axis=0) + sky_px * sum_bg) / sum_dt
    E = interp_fast(table, fbar, rate_lo, rate_hi)
    E_start = E.sum(axis=0)
    eta, N, tau = (np.asarray(a, dtype=np.float64).reshape(2, 1, 1) for a in (eta, N, tau))
    out = reads_off.copy()
    trapped = np.zeros((R, S, S))
    cum = np.zeros((S, S))
    interior = np.zeros((S, S), dtype=bool)
    interior[BORDER:S - BORDER, BORDER:S - BORDER] = True
    prev = E_start
    for r in range(R):
        f = dN[r] / read_dt[r]
        c = eta * f / N + 1.0 / tau
        E = E + (eta * f / c - E) * -np.expm1(-c * read_dt[r])
        now = E.sum(axis=0)
        cum = cum + (dN[r] - (now - prev)) * (1.0 / GAIN)
        prev = now
        trapped[r] = now - E_start
        out[r + 1] = np.where(interior, reads_off[0] + cum, reads_off[r + 1])
    return out, trapped, dN
