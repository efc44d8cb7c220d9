"""Star spots in the device light curves: occulted and unocculted.

The star of `lightcurve` is a clean limb-darkened disc.  With spots the transit depths change in two ways: unocculted
spots bias every depth by F0 / (F0 - D) (the transit light source effect), and a spot the planet crosses puts a bump
into the light curve (the planet blocks less light there).  Both depend on wavelength through the spot's contrast.

All quantities are float64, lengths in stellar radii in the sky frame of `lightcurve.planet_position` (X, Y).  A spot is
a circle IN PROJECTION: centre C_i, radius r_i, contrast c_{i,w} >= 0 (spot intensity over photosphere intensity in bin
w; > 1: a facula); the limb-darkening law inside a spot is the photosphere's.  With the Claret profile
I(mu) = c0 + sum_n a_n mu^(n/2), c0 = 1 - sum a_n, and the disc flux F0_w = pi (1 - sum a_n n/(n+4)):

    Q_n(P, C, p, r) = int over (planet disc of radius p at P) n (spot disc of radius r at C) of mu^(n/2) dA   lens_basis
    S_{i,n} = Q_n(C_i, C_i, r_i, r_i)                                  the whole spot                          spot_basis
    D_w     = sum_i (1 - c_{i,w}) sum_n a'_n(w) S_{i,n}                a'_0 = c0, a'_n = a_n
    X_{k,w} = sum_i (1 - c_{i,w}) sum_n a'_n(w) Q_n(P_k, C_i, p_w, r_i)
    depth'[k][w] = (depth[k][w] F0_w - X_{k,w}) / (F0_w - D_w)         rows in transit (z_k < 10, hidden_k = 0),
                                                                       columns with a radius ratio
    depth'[k][w] = depth[k][w]                                         everywhere else

`lens_basis` is a FIXED quadrature rule (10 x 10 Gauss-Legendre nodes per panel, two panels, fixed order), stated here in
numpy and in wayne_amd/csrc/k_lightcurve_spots.h in C++ (host and device): the two agree to rounding, and the rule is
within 1e-6 of the lens area of the converged integral for spots wholly inside radius 0.98 (tests/test_spots.py).

Refused (ValueError): more than 8 spots, a radius that is not finite or <= 0, |C_i| + r_i > 0.98 (a lens never reaches
the limb, where mu^(1/2) has an infinite slope), two spots with |C_i - C_j| < r_i + r_j (their terms would not add), a
contrast that is not finite or < 0, F0_w - D_w <= 0.

Not covered: rotation or evolution within a visit, foreshortening (a spot is a circle on the sky, not on the sphere),
spots at or across the limb, overlapping spots, spots in the eclipse term, a changed stellar spectrum (the spectrum given
stays the out-of-transit spectrum; only the depths change), spotted contaminants, interpolation of Q_n in p.
"""
import hashlib

import numpy as np

from . import tools

MAX_SPOTS = 8
LIMB = 0.98          # |C| + r may not exceed this
GL_NODES = 10
_G, _OMEGA = np.polynomial.legendre.leggauss(GL_NODES)


def gauss_legendre():
    """The rule's nodes and weights on [-1, 1] (float64 arrays of GL_NODES): numpy.polynomial.legendre.leggauss(10).
    The kernel gets these very doubles in its argument struct."""
    return _G.copy(), _OMEGA.copy()


def _panels(d, p, r):
    """Per element of p: the two panels (cc, rad, sg, lo, hi) of the rule and `live` (d < p + r)."""
    p = np.asarray(p, dtype=float)
    d = np.broadcast_to(np.asarray(d, dtype=float), p.shape)
    r = np.broadcast_to(np.asarray(r, dtype=float), p.shape)
    live = d < p + r
    inside = d <= np.abs(p - r)
    rho = np.minimum(p, r)
    t_c = np.where(r <= p, d, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_star = (d * d + p * p - r * r) / (2.0 * d)
        phi1 = np.arccos(np.clip((d - t_star) / r, -1.0, 1.0))
        phi2 = np.arccos(np.clip(t_star / p, -1.0, 1.0))
    half_pi = 0.5 * np.pi
    zero = np.zeros(p.shape)
    one = np.ones(p.shape)
    pan1 = (np.where(inside, t_c, d), np.where(inside, rho, r), one, zero, np.where(inside, half_pi, phi1))
    pan2 = (np.where(inside, t_c, 0.0), np.where(inside, rho, p), np.where(inside, one, -one),
            np.where(inside, half_pi, 0.0), np.where(inside, np.pi, phi2))
    return live, (pan1, pan2)


def lens_basis(P, C, p, r, nodes=None):
    """Q_0 .. Q_4 = int mu^(n/2) dA over (disc of radius p at P) n (disc of radius r at C), mu = sqrt(max(1 - x^2 - y^2,
    0)): an array [5] + shape(p), vectorised over p (one (k, i), every wavelength).  The fixed rule: d = |C - P|,
    u = (C - P) / d (or (1, 0)), v = (-u_y, u_x); d >= p + r: zero; d <= |p - r|: the smaller circle in two panels of
    phi in [0, pi/2] and [pi/2, pi]; else the part bounded by the spot's circle, then the part bounded by the planet's,
    either side of the chord t* = (d^2 + p^2 - r^2) / (2 d).  A panel (cc, rad, sg, [lo, hi]): phi_a = mid + half g_a,
    t = cc - sg rad cos phi_a, h = rad sin phi_a, s_b = h g_b, (x, y) = P + t u + s_b v, Q_n += omega_a half rad
    sin phi_a h omega_b mu^(n/2); panels in that order, a outer, b inner, both ascending.  `nodes`: another Gauss-Legendre
    order (the tests' converged rule)."""
    g, om = (_G, _OMEGA) if nodes is None else np.polynomial.legendre.leggauss(int(nodes))
    px, py = float(P[0]), float(P[1])
    cx, cy = float(C[0]), float(C[1])
    p = np.asarray(p, dtype=float)
    r = float(r)
    dx, dy = cx - px, cy - py
    d = float(np.sqrt(dx * dx + dy * dy))
    ux, uy = (dx / d, dy / d) if d > 0.0 else (1.0, 0.0)
    vx, vy = -uy, ux
    Q = np.zeros((5,) + p.shape)
    live, panels = _panels(d, p, r)
    if not np.any(live):
        return Q
    for (cc, rad, sg, lo, hi) in panels:
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        for a in range(g.size):
            phi = mid + half * g[a]
            sn = np.sin(phi)
            t = cc - sg * rad * np.cos(phi)
            h = rad * sn
            wa = om[a] * half * rad * sn * h
            bx, by = px + t * ux, py + t * uy
            for b in range(g.size):
                s = h * g[b]
                x, y = bx + s * vx, by + s * vy
                mu = np.sqrt(np.maximum(1.0 - x * x - y * y, 0.0))
                sm = np.sqrt(mu)
                wab = wa * om[b]
                Q[0] += wab
                Q[1] += wab * sm
                Q[2] += wab * mu
                Q[3] += wab * (mu * sm)
                Q[4] += wab * (mu * mu)
    Q[:, ~live] = 0.0
    return Q


def spot_basis(cx, cy, radius):
    """S_{i,n} [n_spots, 5]: the whole spot's integrals, lens_basis(C_i, C_i, r_i, r_i)."""
    cx, cy, radius = (np.asarray(a, dtype=float).reshape(-1) for a in (cx, cy, radius))
    return np.array([lens_basis((cx[i], cy[i]), (cx[i], cy[i]), radius[i], radius[i]) for i in range(cx.size)]
                    ).reshape(cx.size, 5)


def claret_terms(ld, W):
    """(a'_0 .. a'_4) [5, W] and F0 [W] of coefficients `ld`, [4] or [W, 4] (the forms of lightcurve.deficit_from_basis)."""
    a = np.asarray(ld, dtype=float)
    if a.shape == (4,):
        a = np.broadcast_to(a, (W, 4))
    if a.shape != (W, 4):
        raise ValueError("spots: limb darkening must be 4 coefficients or an array [W, 4] with W = %d, got %s" % (W, a.shape))
    a1, a2, a3, a4 = (a[:, n] for n in range(4))
    c0 = 1.0 - a1 - a2 - a3 - a4
    f0 = np.pi * (1.0 - (a1 * (1.0 / 5.0) + a2 * (2.0 / 6.0) + a3 * (3.0 / 7.0) + a4 * (4.0 / 8.0)))
    return np.stack([c0, a1, a2, a3, a4]), f0


def _combine(terms, Q):
    """sum_n a'_n Q_n, n ascending (Q: [5] or [5, W])."""
    return (((terms[0] * Q[0] + terms[1] * Q[1]) + terms[2] * Q[2]) + terms[3] * Q[3]) + terms[4] * Q[4]


def check_geometry(cx, cy, radius, contrast=None):
    """ValueError for what the law refuses in the spots themselves."""
    cx, cy, radius = (np.asarray(a, dtype=float).reshape(-1) for a in (cx, cy, radius))
    n = radius.size
    if cx.size != n or cy.size != n:
        raise ValueError("spots: centres and radii differ in number")
    if n > MAX_SPOTS:
        raise ValueError("spots: at most %d spots, got %d" % (MAX_SPOTS, n))
    if not np.all(np.isfinite(radius)) or not np.all(radius > 0.0):
        raise ValueError("spots: a radius must be finite and > 0")
    if not np.all(np.isfinite(cx)) or not np.all(np.isfinite(cy)):
        raise ValueError("spots: a centre must be finite")
    if not np.all(np.sqrt(cx * cx + cy * cy) + radius <= LIMB):
        raise ValueError("spots: |centre| + radius must be <= %.2f (a spot may not reach the limb)" % LIMB)
    for i in range(n):
        for j in range(i + 1, n):
            if np.hypot(cx[i] - cx[j], cy[i] - cy[j]) < radius[i] + radius[j]:
                raise ValueError("spots: spots %d and %d overlap" % (i + 1, j + 1))
    if contrast is not None:
        c = np.asarray(contrast, dtype=float)
        if c.ndim != 2 or c.shape[0] != n:
            raise ValueError("spots: contrast must have shape [n_spots, W], got %s" % (c.shape,))
        if not np.all(np.isfinite(c)) or not np.all(c >= 0.0):
            raise ValueError("spots: a contrast must be finite and >= 0")


def unocculted_deficit(ld, cx, cy, radius, contrast):
    """(F0 [W], D [W]); ValueError when F0 - D <= 0 in some bin."""
    contrast = np.asarray(contrast, dtype=float)
    terms, f0 = claret_terms(ld, contrast.shape[1])
    S = spot_basis(cx, cy, radius)
    D = np.zeros(contrast.shape[1])
    for i in range(S.shape[0]):
        D = D + (1.0 - contrast[i]) * _combine(terms, S[i])
    if not np.all(f0 - D > 0.0):
        raise ValueError("spots: the spotted disc flux F0 - D must be > 0 in every bin")
    return f0, D


def apply_law(depth, X, Y, z_tr, hidden, planet_spectrum, ld, cx, cy, radius, contrast, parts=None):
    """The whole law in numpy: the spotted depth matrix [K, W] from the unspotted one.  `lens_basis` is evaluated only for
    (k, i) with d < p_max + r.  `parts` (a dict): filled with F0, D [W] and the bound's sum_i |1 - c| (Q_0 + S_0) [K, W]."""
    depth = np.asarray(depth, dtype=float)
    K, W = depth.shape
    X, Y, z_tr = (np.asarray(a, dtype=float).reshape(-1) for a in (X, Y, z_tr))
    hidden = np.zeros(K) if hidden is None else np.asarray(hidden, dtype=float).reshape(-1)
    cx, cy, radius = (np.asarray(a, dtype=float).reshape(-1) for a in (cx, cy, radius))
    contrast = np.asarray(contrast, dtype=float)
    spec = np.asarray(planet_spectrum, dtype=float).reshape(-1)
    if X.size != K or Y.size != K or z_tr.size != K or hidden.size != K:
        raise ValueError("spots: the planet track has %d points, the depth matrix %d rows" % (X.size, K))
    if spec.size != W or contrast.shape != (cx.size, W):
        raise ValueError("spots: contrast [n, W] and the planet spectrum [W] must match the depth matrix, W = %d" % W)
    check_geometry(cx, cy, radius, contrast)
    rows = (z_tr < 10.0) & (hidden == 0.0)
    if not np.all(np.isfinite(X[rows])) or not np.all(np.isfinite(Y[rows])):
        raise ValueError("spots: the planet track must be finite on every transit row")
    sized = spec >= 0.0
    p = np.sqrt(np.where(sized, spec, 0.0))
    terms, f0 = claret_terms(ld, W)
    f0, D = unocculted_deficit(ld, cx, cy, radius, contrast)
    S = spot_basis(cx, cy, radius)
    out = depth.copy()
    p_max = float(p[sized].max()) if sized.any() else 0.0
    mag = np.zeros((K, W))
    for k in np.nonzero(rows)[0]:
        Xk = np.zeros(W)
        for i in range(cx.size):
            mag[k] += np.abs(1.0 - contrast[i]) * S[i, 0]
            if not np.hypot(cx[i] - X[k], cy[i] - Y[k]) < p_max + radius[i]:
                continue
            Q = lens_basis((X[k], Y[k]), (cx[i], cy[i]), p, radius[i])
            Xk = Xk + (1.0 - contrast[i]) * _combine(terms, Q)
            mag[k] += np.abs(1.0 - contrast[i]) * Q[0]
        out[k, sized] = ((depth[k] * f0 - Xk) / (f0 - D))[sized]
    if parts is not None:
        parts.update(F0=f0, D=D, mag=mag, rows=rows, sized=sized)
    return out


class SpotGeometry(object):
    """What one exposure's device light curve needs of the spots: the planet's track X, Y [K] (stellar radii, the sky
    frame of lightcurve.planet_position), the centres and radii [n] and the contrast [n, W] on the exposure's wavelength
    grid.  Hand it to lightcurve.DeviceDepths as `spots`."""

    def __init__(self, X, Y, cx, cy, radius, contrast):
        self.X = np.ascontiguousarray(X, dtype=float).reshape(-1)
        self.Y = np.ascontiguousarray(Y, dtype=float).reshape(-1)
        self.cx, self.cy, self.radius = (np.ascontiguousarray(a, dtype=float).reshape(-1) for a in (cx, cy, radius))
        self.contrast = np.ascontiguousarray(contrast, dtype=float)
        if self.contrast.ndim != 2:
            raise ValueError("spots: contrast must have shape [n_spots, W]")
        if self.X.size != self.Y.size:
            raise ValueError("spots: the planet track's X and Y differ in length")
        check_geometry(self.cx, self.cy, self.radius, self.contrast)

    @property
    def n(self):
        return self.radius.size

    def crop(self, i0, i1):
        """The same geometry on the wavelength bins i0 .. i1 - 1."""
        return SpotGeometry(self.X, self.Y, self.cx, self.cy, self.radius, self.contrast[:, i0:i1])

    def apply(self, depth, z_tr, hidden, planet_spectrum, ld, parts=None):
        return apply_law(depth, self.X, self.Y, z_tr, hidden, planet_spectrum, ld, self.cx, self.cy, self.radius,
                         self.contrast, parts)

    def digest_bytes(self):
        return (b"spots" + self.X.tobytes() + self.Y.tobytes() + self.cx.tobytes() + self.cy.tobytes() +
                self.radius.tobytes() + self.contrast.tobytes())


class Spot(object):
    """One spot: centre (x, y) and radius in stellar radii on the sky, and either a `contrast` (one number for every
    wavelength) or a `temperature` (K; the contrast is then the Planck ratio against the photosphere's)."""

    def __init__(self, x, y, radius, contrast=None, temperature=None):
        if (contrast is None) == (temperature is None):
            raise ValueError("spot: give contrast or temperature, one of them")
        try:
            self.x, self.y, self.radius = float(x), float(y), float(radius)
            self.contrast = None if contrast is None else float(contrast)
            self.temperature = None if temperature is None else float(temperature)
        except (TypeError, ValueError):
            raise ValueError("spot: x, y, radius, contrast and temperature must be numbers")
        if self.contrast is not None and not (np.isfinite(self.contrast) and self.contrast >= 0.0):
            raise ValueError("spot: a contrast must be finite and >= 0")
        if self.temperature is not None and not (np.isfinite(self.temperature) and self.temperature > 0.0):
            raise ValueError("spot: a temperature must be finite and > 0")


class StarSpots(object):
    """The spots of a visit's star: at most 8 `Spot`s, none reaching beyond radius 0.98, no two overlapping;
    `photosphere_temperature` (K) is required if and only if some spot gives a temperature."""

    def __init__(self, spots, photosphere_temperature=None):
        self.spots = tuple(spots)
        if not self.spots:
            raise ValueError("spots: the list is empty")
        if not all(isinstance(s, Spot) for s in self.spots):
            raise ValueError("spots: every entry must be a spots.Spot")
        thermal = any(s.temperature is not None for s in self.spots)
        if thermal != (photosphere_temperature is not None):
            raise ValueError("spots: photosphere_temperature is required if and only if some spot gives a temperature")
        try:
            self.photosphere_temperature = None if photosphere_temperature is None else float(photosphere_temperature)
        except (TypeError, ValueError):
            raise ValueError("spots: photosphere_temperature must be a number")
        if thermal and not (np.isfinite(self.photosphere_temperature) and self.photosphere_temperature > 0.0):
            raise ValueError("spots: photosphere_temperature must be finite and > 0")
        self.cx = np.array([s.x for s in self.spots])
        self.cy = np.array([s.y for s in self.spots])
        self.radius = np.array([s.radius for s in self.spots])
        check_geometry(self.cx, self.cy, self.radius)

    def on_grid(self, wl):
        """The contrast [n, W] at the wavelengths `wl` (um): a scalar contrast as it is, a temperature as
        B_lambda(T_spot) / B_lambda(T_photosphere)."""
        wl = np.asarray(wl, dtype=float).reshape(-1)
        out = np.empty((len(self.spots), wl.size))
        for i, s in enumerate(self.spots):
            if s.contrast is not None:
                out[i] = s.contrast
            else:
                out[i] = tools.blackbody_lambda(wl, s.temperature) / tools.blackbody_lambda(wl, self.photosphere_temperature)
        if not np.all(np.isfinite(out)) or not np.all(out >= 0.0):
            raise ValueError("spots: a contrast must be finite and >= 0")
        return out

    def geometry(self, X, Y, wl):
        return SpotGeometry(X, Y, self.cx, self.cy, self.radius, self.on_grid(wl))

    def apply(self, depth, X, Y, z_tr, hidden, planet_spectrum, ld, contrast):
        """The numpy statement of the whole law for these spots (`contrast`: on_grid of the matrix's wavelengths)."""
        return apply_law(depth, X, Y, z_tr, hidden, planet_spectrum, ld, self.cx, self.cy, self.radius, contrast)

    def check_flux(self, ld, wl):
        """ValueError when the spotted disc flux F0 - D is not positive in some bin of `wl` (ld: [4] or [W, 4])."""
        unocculted_deficit(ld, self.cx, self.cy, self.radius, self.on_grid(wl))

    def hash(self, wl):
        h = hashlib.blake2b(self.cx.tobytes(), digest_size=8)
        for a in (self.cy, self.radius, self.on_grid(wl)):
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest().upper()

    def cards(self, wl):
        """Primary-header cards of an exposure of a spotted star: SPOTS = T, NSPOTS, per spot SPTXn / SPTYn / SPTRn and
        SPTCn (its contrast at the middle bin of `wl`), and SPTHASH, 64 bits of a blake2b over centres, radii and the
        contrast array on `wl`."""
        wl = np.asarray(wl, dtype=float).reshape(-1)
        contrast = self.on_grid(wl)
        cards = [("SPOTS", True, "star spots in the light curves on"), ("NSPOTS", len(self.spots), "number of spots")]
        for i in range(len(self.spots)):
            cards += [("SPTX%d" % (i + 1), float(self.cx[i]), "spot %d centre X (stellar radii)" % (i + 1)),
                      ("SPTY%d" % (i + 1), float(self.cy[i]), "spot %d centre Y (stellar radii)" % (i + 1)),
                      ("SPTR%d" % (i + 1), float(self.radius[i]), "spot %d radius (stellar radii)" % (i + 1)),
                      ("SPTC%d" % (i + 1), float(contrast[i, wl.size // 2]), "spot %d contrast, middle bin" % (i + 1))]
        cards.append(("SPTHASH", self.hash(wl), "blake2b-64 over centres, radii, contrast"))
        return cards

    def digest_bytes(self):
        temps = np.array([[-1.0 if s.contrast is None else s.contrast, -1.0 if s.temperature is None else s.temperature]
                          for s in self.spots])
        phot = np.array([-1.0 if self.photosphere_temperature is None else self.photosphere_temperature])
        return b"spots" + self.cx.tobytes() + self.cy.tobytes() + self.radius.tobytes() + temps.tobytes() + phot.tobytes()

    def __eq__(self, other):
        return isinstance(other, StarSpots) and self.digest_bytes() == other.digest_bytes()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self.digest_bytes())

    @classmethod
    def from_config(cls, section, position_at_phase=None):
        """The YAML's `target: spots:` section -> StarSpots: `photosphere_temperature` (K) and `list`, each entry
        {x, y, radius} or {at_phase, radius} -- centred where the planet's centre is at that orbital phase from
        mid-transit, in periods, through `position_at_phase(phase) -> (x, y)` -- with `contrast` or `temperature`.
        ValueError for every defect."""
        if not isinstance(section, dict):
            raise ValueError("spots must be a mapping with `list` and an optional photosphere_temperature")
        unknown = sorted(set(section) - {"photosphere_temperature", "list"})
        if unknown:
            raise ValueError("spots takes list and photosphere_temperature (unknown: %s)" % ", ".join(map(str, unknown)))
        entries = section.get("list")
        if not isinstance(entries, (list, tuple)) or not entries:
            raise ValueError("spots: list must be a non-empty list of spots")
        if len(entries) > MAX_SPOTS:
            raise ValueError("spots: at most %d spots, got %d" % (MAX_SPOTS, len(entries)))
        made = []
        for n, e in enumerate(entries, 1):
            if not isinstance(e, dict):
                raise ValueError("spots: entry %d must be a mapping" % n)
            unknown = sorted(set(e) - {"x", "y", "at_phase", "radius", "contrast", "temperature"})
            if unknown:
                raise ValueError("spots: entry %d: unknown key(s) %s" % (n, ", ".join(map(str, unknown))))
            if "radius" not in e:
                raise ValueError("spots: entry %d has no radius" % n)
            if "at_phase" in e:
                if "x" in e or "y" in e:
                    raise ValueError("spots: entry %d gives at_phase and a centre" % n)
                if position_at_phase is None:
                    raise ValueError("spots: entry %d: at_phase needs the planet's orbit" % n)
                try:
                    phase = float(e["at_phase"])
                except (TypeError, ValueError):
                    raise ValueError("spots: entry %d: at_phase must be a number" % n)
                if not np.isfinite(phase):
                    raise ValueError("spots: entry %d: at_phase must be finite" % n)
                x, y = position_at_phase(phase)
            elif "x" in e and "y" in e:
                x, y = e["x"], e["y"]
            else:
                raise ValueError("spots: entry %d needs x and y, or at_phase" % n)
            try:
                made.append(Spot(x, y, e["radius"], e.get("contrast"), e.get("temperature")))
            except ValueError as err:
                raise ValueError("spots: entry %d: %s" % (n, err))
        return cls(made, section.get("photosphere_temperature"))


def rule_check_lenses(seed=1, n=300):
    """The lenses on which the rule's error is stated (tests/test_spots.py, scripts/bench_spots.py): a list of
    (P, C, p, r) with p, r uniform in [0.03, 0.3], the spot wholly inside radius 0.98 -- every third pinned at
    |C| + r = 0.98 -- and d = |C - P| uniform in [0, p + r), every fifth scaled by 1e-3."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n):
        p, r = rng.uniform(0.03, 0.3, 2)
        rc = (LIMB - r) * (1.0 if j % 3 == 0 else rng.uniform())
        ang, ang_d = rng.uniform(0.0, 2.0 * np.pi, 2)
        d = rng.uniform() * (p + r) * (1e-3 if j % 5 == 0 else 1.0)
        C = (rc * np.cos(ang), rc * np.sin(ang))
        out.append(((C[0] + d * np.cos(ang_d), C[1] + d * np.sin(ang_d)), C, p, r))
    return out


def rule_error(lenses, converged=48):
    """Worst |Q_n - Q_n(converged nodes)| / lens area over `lenses` (the area: Q_0 of the converged rule)."""
    worst = 0.0
    for (P, C, p, r) in lenses:
        q, ref = lens_basis(P, C, p, r), lens_basis(P, C, p, r, nodes=converged)
        if ref[0] > 0.0:
            worst = max(worst, float(np.abs(q - ref).max() / ref[0]))
    return worst
