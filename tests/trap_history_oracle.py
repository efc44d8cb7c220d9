"""A float64 restatement of the carried trap history (wayne_exposure_set_trap_history, k_ramp_hist) for the tests, on
whole frames: an exposure starts from the trap state the previous one left -- stepped over the gap, raised by the orbit's
fill, clipped to the capacity --, traps read by read as tests/trap_oracle.py states it, and leaves its state behind,
rounded to float32.  Built on trap_oracle (`exact`, and the body of `trapped_reads` with E at the zero read handed in);
it shares no code with the package."""
import numpy as np

import trap_oracle as to


def after_gap(E, f_gap, gap_s, fill, eta, N, tau):
    """E [2, ...] float64 after `gap_s` seconds at rate f_gap (0: a dark gap), then + fill, clipped to N.  eta, N, tau,
    fill: [2] per population, broadcast over the trailing axes of E."""
    E = np.asarray(E, dtype=np.float64)
    shape = (2,) + (1,) * (E.ndim - 1)
    eta, N, tau, fill = (np.asarray(a, dtype=np.float64).reshape(shape) for a in (eta, N, tau, fill))
    if gap_s > 0:
        E = to.exact(E, f_gap, gap_s, eta, N, tau)
    return np.minimum(E + fill, N)


def mean_rate(acc, sky_plane, bg, read_dt):
    """The pixel's mean rate over the exposure as the device forms it (trap_oracle.trapped_reads): its accumulators plus
    its expected sky, over the exposure's length."""
    sky_px = np.where(sky_plane > 0, sky_plane.astype(np.float64), 0.0)
    sum_bg = 0.0
    for b in bg:
        sum_bg += float(np.float32(b))
    sum_dt = 0.0
    for d in read_dt:
        sum_dt += float(d)
    return (acc.sum(axis=0) + sky_px * sum_bg) / sum_dt


def exposure(state, reads_off, acc, sky_plane, bg, read_dt, gap_s, lit, fill, eta, N, tau):
    """One exposure of a carried history.  state [S, S, 2] float32 (bordered; [..., 0] slow, [..., 1] fast);
    reads_off [R+1, S, S] the float64 reads of the same exposure without traps (same draws, gain variations off); acc
    [R, S, S] the accumulator electrons; sky_plane, bg, read_dt as trap_oracle.trapped_reads takes them; gap_s, lit,
    fill [2]: the exposure's history descriptor.  Returns (reads [R+1, S, S], the state it leaves [S, S, 2] float32 --
    reference pixels as they were --, E at the zero read [2, S, S], trapped electrons [R, S, S] since the zero read)."""
    R, S = acc.shape[0], acc.shape[1]
    assert state.shape == (S, S, 2) and state.dtype == np.float32
    dN = np.diff(reads_off, axis=0) * to.GAIN
    fbar = mean_rate(acc, sky_plane, bg, read_dt)
    E = np.moveaxis(state.astype(np.float64), 2, 0)
    E = after_gap(E, fbar if lit else 0.0, float(gap_s), fill, eta, N, tau)
    E_zero = E.copy()
    E_start = E.sum(axis=0)
    eta3, N3, tau3 = (np.asarray(a, dtype=np.float64).reshape(2, 1, 1) for a in (eta, N, tau))
    out = reads_off.copy()
    trapped = np.zeros((R, S, S))
    cum = np.zeros((S, S))
    interior = np.zeros((S, S), dtype=bool)
    interior[to.BORDER:S - to.BORDER, to.BORDER:S - to.BORDER] = True
    prev = E_start
    for r in range(R):
        f = dN[r] / read_dt[r]
        c = eta3 * f / N3 + 1.0 / tau3
        E = E + (eta3 * f / c - E) * -np.expm1(-c * read_dt[r])
        now = E.sum(axis=0)
        cum = cum + (dN[r] - (now - prev)) * (1.0 / to.GAIN)
        prev = now
        trapped[r] = now - E_start
        out[r + 1] = np.where(interior, reads_off[0] + cum, reads_off[r + 1])
    left = state.copy()
    left[interior] = np.moveaxis(E, 0, 2).astype(np.float32)[interior]
    return out, left, E_zero, trapped


def constant_rate_chain(plan, exptime_s, f, initial, eta, N, tau):
    """A pixel that collects at constant rate(s) f in every exposure, stepped through a history plan (gap_s, lit, fill
    per exposure) with one exact step of exptime_s per exposure, in float64 without the float32 rounding: its occupancy
    at every exposure's zero read, [n_exp, 2, *f.shape]."""
    f = np.asarray(f, dtype=np.float64)
    shape = (2,) + (1,) * f.ndim
    eta_, N_, tau_ = (np.asarray(a, dtype=np.float64).reshape(shape) for a in (eta, N, tau))
    E = np.broadcast_to(np.asarray(initial, dtype=np.float64).reshape(shape), (2,) + f.shape).copy()
    out = []
    for k in range(len(plan["gap_s"])):
        E = after_gap(E, f if plan["lit"][k] else 0.0, float(plan["gap_s"][k]), plan["fill"][k], eta, N, tau)
        out.append(E.copy())
        E = to.exact(E, f, float(exptime_s), eta_, N_, tau_)
    return np.array(out)
