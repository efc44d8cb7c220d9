"""Charge trapping in the HgCdTe pixels: the WFC3-IR "ramp effect", per pixel (no reference counterpart).

The two-population model of Zhou et al. 2017, AJ 153, 243 ("RECTE"): a pixel has a slow and a fast trap population,
each with a capacity N (e-), a trapping efficiency eta and a lifetime tau (s).  Its occupancy E obeys

    dE/dt = eta f (1 - E / N) - E / tau        f = the pixel's collected-charge rate (e- / s)

and for constant f over an interval dt the step is exact (`step`).  Trapped charge is missing from the reads and
released charge comes back: read r shows what the pixel collected minus (E_s + E_f)(r) - (E_s + E_f)(zero read).
Nothing is drawn at random.

Within an exposure the device steps every pixel read by read (k_ramp.h, k_ramp_trap).  What the traps hold at an
exposure's zero read is planned here, so that exposure i stays a function of its descriptor and the visit seed alone:
the pixel is assumed to have seen its mean rate f_bar in every earlier exposure of the visit (the approximation the
published model makes for a visit).  `ChargeTraps.start_tables` tabulates each exposure's zero-read occupancy on a grid
of f_bar; the device interpolates its exposure's table once per pixel, by the rule of `interpolate`.

Default parameters: the paper's best fit (slow N = 1525.38, eta = 0.013318, tau = 1.63e4 s; fast N = 162.38,
eta = 0.008407, tau = 281.463 s; Zhou et al. 2017 and its public RECTE code), quoted without a copy of the paper at
hand -- check them against it before relying on them.  Nothing but the defaults depends on these numbers.
Known artefacts: cosmic-ray charge counts in f_bar (a hit pixel's history looks brighter, by an electron or two); the
history ignores the transit and the visit-trend scale (<= 2 % of f_bar); the direct image neither traps nor enters the
history.

Carried history (`history: carried`, opt-in): the device keeps each pixel's state (slow, fast) from one exposure to the
next instead (k_ramp_hist; wayne_exposure_set_trap_history).  An exposure starts from what the previous one left, stepped
over the gap between them and raised by `orbit_fill` at an orbit's start (`ChargeTraps.history_plan`: the schedule of
`start_tables`), and leaves its own state behind.  The history is then the charge each pixel really collected -- the
transit, the visit trend, every sky draw, and a cosmic ray in the pixel it hit -- and a state from an earlier visit can
be handed in (Observation.setup_charge_traps(initial_state=...)).  Exposures are no longer independent: no sharding over
ranks and no --resume in that mode.

Not modelled: replay mode; in the gaps of a carried history the rate is the exposure's own mean rate (staring) or zero
(a scan), as in the planned one.
"""
import math
import struct

import numpy as np

POPULATIONS = ("slow", "fast")
KEYS = ("n_traps", "efficiency", "lifetime_s", "initial", "orbit_fill")
DEFAULTS = {
    "slow": dict(n_traps=1525.38, efficiency=0.013318, lifetime_s=1.63e4, initial=0.0, orbit_fill=0.0),
    "fast": dict(n_traps=162.38, efficiency=0.008407, lifetime_s=281.463, initial=0.0, orbit_fill=0.0),
}
GRID = 1024                  # points of a start table (wayne_trap_desc.n_rate)
MAX_GRID = 4096              # WAYNE_MAX_TRAP_RATES
RATE_LO, RATE_HI = 1e-2, 1e6
SECONDS_PER_DAY = 86400.0
HISTORIES = ("planned", "carried")


class ChargeTrapConfigError(ValueError):
    pass


def step(E, f, dt, eta, n_traps, tau):
    """Occupancy after dt seconds at constant rate f, from E (float64, broadcasting):
    c = eta f / N + 1 / tau, E_inf = eta f / c, E(dt) = E + (E_inf - E)(1 - e^{-c dt})."""
    f = np.asarray(f, dtype=np.float64)
    c = eta * f / n_traps + 1.0 / tau
    return E + (eta * f / c - E) * -np.expm1(-c * dt)


def interpolate(table, f, rate_lo, rate_hi):
    """Start tables [2, G] at rates f (any shape) -> [2, *f.shape], the device's rule (k_ramp.h trap_start): point 0 is
    f = 0, points 1 .. G-1 are log-spaced from rate_lo to rate_hi; linear in f below rate_lo, linear in ln f above it,
    clamped at rate_hi."""
    table = np.asarray(table, dtype=np.float64)
    G = table.shape[-1]
    f = np.asarray(f, dtype=np.float64)
    u_scale = (G - 2) / math.log(rate_hi / rate_lo) if G > 2 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (np.log(np.where(f > 0, f, rate_lo)) - math.log(rate_lo)) * u_scale
    i = np.clip(np.trunc(u), 0, max(G - 3, 0)).astype(np.int64)
    w = u - i
    out = np.empty((2,) + f.shape)
    for p in range(2):
        e = table[p]
        v = np.where(u < G - 2, e[np.minimum(1 + i, G - 1)] + (e[np.minimum(2 + i, G - 1)] - e[np.minimum(1 + i, G - 1)]) * w,
                     e[G - 1])
        v = np.where(f < rate_lo, e[0] + (e[1] - e[0]) * (f / rate_lo), v)
        out[p] = np.where(f > 0, v, e[0])
    return out


class ChargeTraps(object):
    """The model's parameters.  `slow` / `fast`: mappings with n_traps, efficiency, lifetime_s, initial (occupancy at the
    visit's first exposure) and orbit_fill (added at every later orbit's start, clipped to n_traps); a key left out takes
    its default.  `grid`, `rate_lo`, `rate_hi`: the start tables' grid.  `history`: "planned" (start tables; exposures
    stay independent) or "carried" (the device carries each pixel's state from exposure to exposure: `history_plan`)."""

    def __init__(self, slow=None, fast=None, grid=GRID, rate_lo=RATE_LO, rate_hi=RATE_HI, history="planned"):
        if history not in HISTORIES:
            raise ChargeTrapConfigError("charge_traps.history: expected planned or carried, got %r" % (history,))
        self.history = history
        self.params = {}
        for name, given in (("slow", slow), ("fast", fast)):
            given = {} if given is None else given
            if not isinstance(given, dict):
                raise ChargeTrapConfigError("charge_traps.%s: expected a mapping" % name)
            unknown = sorted(set(given) - set(KEYS))
            if unknown:
                raise ChargeTrapConfigError("charge_traps.%s: unknown key(s) %s" % (name, ", ".join(map(str, unknown))))
            p = dict(DEFAULTS[name])
            for k, v in given.items():
                if v is None:
                    continue
                if isinstance(v, bool):
                    raise ChargeTrapConfigError("charge_traps.%s.%s must be a number" % (name, k))
                try:
                    p[k] = float(v)
                except (TypeError, ValueError):
                    raise ChargeTrapConfigError("charge_traps.%s.%s must be a number" % (name, k))
            self.params[name] = p
        self.grid, self.rate_lo, self.rate_hi = int(grid), float(rate_lo), float(rate_hi)
        self._validate()

    def _validate(self):
        for name in POPULATIONS:
            p = self.params[name]
            for k in KEYS:
                if not math.isfinite(p[k]):
                    raise ChargeTrapConfigError("charge_traps.%s.%s must be finite" % (name, k))
            if not p["n_traps"] > 0:
                raise ChargeTrapConfigError("charge_traps.%s.n_traps must be > 0" % name)
            if not 0.0 <= p["efficiency"] <= 1.0:
                raise ChargeTrapConfigError("charge_traps.%s.efficiency must lie in [0, 1]" % name)
            if not p["lifetime_s"] > 0:
                raise ChargeTrapConfigError("charge_traps.%s.lifetime_s must be > 0" % name)
            for k in ("initial", "orbit_fill"):
                if not 0.0 <= p[k] <= p["n_traps"]:
                    raise ChargeTrapConfigError("charge_traps.%s.%s must lie in [0, n_traps]" % (name, k))
        if not 2 <= self.grid <= MAX_GRID:
            raise ChargeTrapConfigError("charge_traps: the grid must have 2 .. %d points" % MAX_GRID)
        if not (math.isfinite(self.rate_lo) and math.isfinite(self.rate_hi) and self.rate_lo > 0
                and (self.rate_hi > self.rate_lo or (self.grid == 2 and self.rate_hi == self.rate_lo))):
            raise ChargeTrapConfigError("charge_traps: need finite 0 < rate_lo < rate_hi")

    @classmethod
    def from_config(cls, section):
        """The YAML's `charge_traps:` section -> ChargeTraps (`{}` or an empty section: every default)."""
        if section is None:
            section = {}
        if not isinstance(section, dict):
            raise ChargeTrapConfigError("`charge_traps` must be a mapping with optional `slow` and `fast` entries")
        unknown = sorted(set(section) - set(POPULATIONS) - {"history"})
        if unknown:
            raise ChargeTrapConfigError("charge_traps: unknown key(s) %s (expected slow, fast, history)" % ", ".join(map(str, unknown)))
        history = section.get("history")
        return cls(slow=section.get("slow"), fast=section.get("fast"), history="planned" if history is None else history)

    def with_history(self, history):
        """This model with another `history` setting (itself if it has that one already)."""
        if history == self.history:
            return self
        return ChargeTraps(slow=self.params["slow"], fast=self.params["fast"], grid=self.grid, rate_lo=self.rate_lo,
                           rate_hi=self.rate_hi, history=history)

    def __repr__(self):
        return "ChargeTraps(slow=%r, fast=%r)" % (self.params["slow"], self.params["fast"])

    def __eq__(self, other):
        return isinstance(other, ChargeTraps) and self.digest_bytes() == other.digest_bytes()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self.digest_bytes())

    def array(self, key):
        """[slow, fast] of one parameter."""
        return np.array([self.params[n][key] for n in POPULATIONS], dtype=np.float64)

    def cards(self):
        """Primary-header cards of a trapped exposure: CTRAPS = T, then per population (suffix S slow, F fast) capacity,
        efficiency, lifetime, initial occupancy and orbit fill, and the start tables' grid (CTGRID points from CTRATELO
        to CTRATEHI e- / s): everything the model's zero-read occupancies depend on besides the visit plan."""
        out = [("CTRAPS", True, "per-pixel charge trapping (ramp effect) on")]
        for n, suf in (("slow", "S"), ("fast", "F")):
            p = self.params[n]
            out += [("CTN" + suf, p["n_traps"], "%s traps: capacity (e-)" % n),
                    ("CTETA" + suf, p["efficiency"], "%s traps: trapping efficiency" % n),
                    ("CTTAU" + suf, p["lifetime_s"], "%s traps: lifetime (s)" % n),
                    ("CTE0" + suf, p["initial"], "%s traps: occupancy at the visit start (e-)" % n),
                    ("CTDE" + suf, p["orbit_fill"], "%s traps: added at each orbit start (e-)" % n)]
        out += [("CTGRID", self.grid, "trap start tables: points of the rate grid"),
                ("CTRATELO", self.rate_lo, "trap start tables: lowest non-zero rate (e-/s)"),
                ("CTRATEHI", self.rate_hi, "trap start tables: highest rate (e-/s)")]
        if self.history == "carried":
            out += [("CTHIST", "CARRIED", "trap state carried from exposure to exposure")]
        return out

    def digest_bytes(self):
        """What identifies the model in a descriptor digest (visit.descriptor_digest)."""
        vals = [self.params[n][k] for n in POPULATIONS for k in KEYS] + [self.rate_lo, self.rate_hi]
        tail = b"history=carried" if self.history == "carried" else b""
        return b"charge_traps" + struct.pack("<i", self.grid) + np.array(vals, dtype=np.float64).tobytes() + tail

    # -- start tables -----------------------------------------------------------------------------------------------
    def rates(self):
        """The grid (e- / s): point 0 = 0, points 1 .. G-1 log-spaced from rate_lo to rate_hi."""
        G = self.grid
        f = np.zeros(G)
        if G == 2:
            f[1] = self.rate_lo
            return f
        f[1:] = np.exp(math.log(self.rate_lo) + np.arange(G - 1) * (math.log(self.rate_hi / self.rate_lo) / (G - 2)))
        f[1], f[-1] = self.rate_lo, self.rate_hi
        return f

    def flat_table(self):
        """[2, G]: every pixel starts at `initial` whatever its rate (an exposure without a visit)."""
        return np.repeat(self.array("initial")[:, None], self.grid, axis=1)

    def start_tables(self, visit_plan, exptime_s, staring, n_exposures=None):
        """[n_exp, 2, G] float64: each exposure's zero-read occupancy per population, as a function of the pixel's mean
        rate f on the grid (`rates`), if the pixel saw f in every earlier exposure of the visit.  In visit order: the first
        exposure starts at `initial`; an exposure lasts exptime_s at f; the gap to the next exposure of the same orbit is
        dark for a spatial scan (the trace has moved on) and lit at f when staring; an orbit boundary
        (visit_plan["orbit_start_index"]) decays over its gap, then adds `orbit_fill`, clipped to n_traps.  Gaps are
        t[k+1] - t[k] - exptime_s, t = visit_plan["exp_start_times"] (days).  One pass: O(n_exp G)."""
        t = np.asarray(visit_plan["exp_start_times"], dtype=np.float64)
        n = len(t) if n_exposures is None else int(n_exposures)
        starts = set(int(i) for i in visit_plan.get("orbit_start_index", [0]))
        f = self.rates()[None, :]
        eta, N, tau = (self.array(k)[:, None] for k in ("efficiency", "n_traps", "lifetime_s"))
        fill = self.array("orbit_fill")[:, None]
        E = np.repeat(self.array("initial")[:, None], self.grid, axis=1)
        out = np.empty((n, 2, self.grid))
        for k in range(n):
            out[k] = E
            if k + 1 == n:
                break
            E = step(E, f, float(exptime_s), eta, N, tau)
            gap = max((t[k + 1] - t[k]) * SECONDS_PER_DAY - float(exptime_s), 0.0)
            if (k + 1) in starts:
                E = np.minimum(step(E, 0.0, gap, eta, N, tau) + fill, N)
            else:
                E = step(E, f if staring else 0.0, gap, eta, N, tau)
        return out

    def interpolate(self, table, f):
        return interpolate(table, f, self.rate_lo, self.rate_hi)

    def history_plan(self, visit_plan, exptime_s, staring, n_exposures=None):
        """What each exposure of a carried history hands the device beside the state (CarriedTraps), on the schedule of
        `start_tables`: a dict of gap_s [n_exp] (seconds since the previous exposure's last read), lit [n_exp] (bool: the
        pixel kept collecting at its mean rate during the gap) and fill [n_exp, 2] (added after the gap, clipped to
        n_traps).  Exposure 0: no gap, no fill (the state has been reset to `initial`); the same orbit: gap =
        max(t[k+1] - t[k] - exptime_s, 0), dark for a scan and lit for staring; an orbit's start: a dark gap, then
        `orbit_fill`."""
        t = np.asarray(visit_plan["exp_start_times"], dtype=np.float64)
        n = len(t) if n_exposures is None else int(n_exposures)
        starts = set(int(i) for i in visit_plan.get("orbit_start_index", [0]))
        gap, lit, fill = np.zeros(n), np.zeros(n, dtype=bool), np.zeros((n, 2))
        for k in range(1, n):
            gap[k] = max((t[k] - t[k - 1]) * SECONDS_PER_DAY - float(exptime_s), 0.0)
            if k in starts:
                fill[k] = self.array("orbit_fill")
            else:
                lit[k] = bool(staring)
        return {"gap_s": gap, "lit": lit, "fill": fill}

    def carried(self, plan, index):
        """Exposure `index` of a `history_plan` -> CarriedTraps."""
        return CarriedTraps(self, plan["gap_s"][index], plan["lit"][index], plan["fill"][index])


class ExposureTraps(object):
    """The model with one exposure's start tables [2, G]: what an exposure descriptor carries to the device
    (make_desc(traps=...) -> Context.upload -> wayne_exposure_set_traps)."""

    __slots__ = ("traps", "table")

    def __init__(self, traps, table=None):
        self.traps = traps
        table = traps.flat_table() if table is None else table
        self.table = np.ascontiguousarray(table, dtype=np.float64)
        if self.table.shape != (2, traps.grid):
            raise ValueError("a start table has shape (2, %d), got %s" % (traps.grid, self.table.shape))

    def digest_bytes(self):
        return self.traps.digest_bytes() + self.table.tobytes()


class CarriedTraps(ExposureTraps):
    """The model with one exposure's share of a carried history, accepted wherever ExposureTraps is: the exposure starts
    from the context's trap state -- stepped over `gap_s` seconds (lit: at the pixel's mean rate; else dark), then raised
    by `fill` [2] and clipped to n_traps -- and leaves its own state behind (Context.upload ->
    wayne_exposure_set_trap_history).  Its start table is the flat one and is not looked at."""

    __slots__ = ("gap_s", "lit", "fill")

    def __init__(self, traps, gap_s=0.0, lit=False, fill=(0.0, 0.0)):
        ExposureTraps.__init__(self, traps)
        self.gap_s, self.lit = float(gap_s), bool(lit)
        self.fill = np.array(fill, dtype=np.float64).reshape(2)

    def digest_bytes(self):
        return (self.traps.digest_bytes() + b"carried" + struct.pack("<d?", self.gap_s, self.lit) + self.fill.tobytes())


def for_exposure(charge_traps):
    """ChargeTraps (flat table at `initial`) or ExposureTraps / CarriedTraps -> itself; None -> None."""
    if charge_traps is None or isinstance(charge_traps, ExposureTraps):
        return charge_traps
    if isinstance(charge_traps, ChargeTraps):
        return ExposureTraps(charge_traps)
    raise TypeError("charge_traps: expected traps.ChargeTraps or traps.ExposureTraps, got %r" % (charge_traps,))
