"""Inter-pixel capacitance of the HgCdTe array: a pixel's reading holds a few per cent of each neighbour's charge (no
reference counterpart).

The law is integer arithmetic on the thrower's accumulators q_r (int64, 2^-28 e-, bordered S x S, read interval r):

    W[i][j] = rint(k[i][j] * 65536)   for the eight neighbours;   W[1][1] = 65536 - sum of them   (charge is conserved)
    q'_r[y, x] = floor((sum_{dy, dx in -1..1} W[dy+1][dx+1] q_r[y+dy, x+dx] + 32768) / 65536)

W[1][2] is the share a pixel receives from its right-hand neighbour; q is 0 beyond the frame; q' is 0 on the 5-pixel
reference border.  The device applies it to the electrons each read interval collected -- target, contaminants, cosmic
rays -- behind the throwers and in front of the ramp kernel (k_ipc.h; wayne_exposure_set_ipc), so every cumulative read is
coupled.  tests/ipc_law.py states the same law in numpy; the device is held to it bit for bit.

Limits.  The sky is drawn inside the ramp kernel: its Poisson noise stays uncorrelated (its mean is smooth and would not
change).  Non-linearity and charge traps act on the coupled charge instead of the pixel's own: an error of second order,
the coupling times the local contrast times those effects.  The direct image, reference pixels and the expected image
(`--expected`: the thrower's truth) are not coupled.

Default kernel: 0.025 to each edge neighbour, 0.0007 to each corner, the centre keeps the rest (0.8972) -- the values the
instrument's PSF modelling tool uses, quoted here without the document at hand.
"""
import struct

import numpy as np

UNIT = 65536
DEFAULT_EDGE = 0.025
DEFAULT_CORNER = 0.0007
CENTRE_TOLERANCE = 0.01      # a given centre further than this from 1 - sum(neighbours): an unnormalised kernel


class IpcConfigError(ValueError):
    pass


def _kernel(edge, corner):
    k = np.array([[corner, edge, corner], [edge, 0.0, edge], [corner, edge, corner]], dtype=np.float64)
    k[1, 1] = 1.0 - (4.0 * edge + 4.0 * corner)
    return k


class InterpixelCapacitance(object):
    """The coupling kernel.  `kernel`: 3 x 3 weights, kernel[1][2] the share a pixel receives from its right-hand
    neighbour; the centre may be given (it must then be 1 - sum of the neighbours to within 0.01) or be None / NaN.
    `alpha`: shorthand for `alpha` to each edge neighbour and nothing to the corners.  Neither: the default kernel."""

    def __init__(self, kernel=None, alpha=None):
        if kernel is not None and alpha is not None:
            raise IpcConfigError("interpixel_capacitance: give either kernel or alpha, not both")
        centre = None
        if alpha is not None:
            if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)):
                raise IpcConfigError("interpixel_capacitance.alpha must be a number")
            k = _kernel(float(alpha), 0.0)
        elif kernel is not None:
            try:
                rows = [[np.nan if v is None else v for v in row] for row in kernel]
                k = np.array(rows, dtype=np.float64)
            except (TypeError, ValueError):
                raise IpcConfigError("interpixel_capacitance.kernel must be a 3 x 3 array of numbers")
            if k.shape != (3, 3):
                raise IpcConfigError("interpixel_capacitance.kernel must be a 3 x 3 array, got shape %s" % (k.shape,))
            if not np.isnan(k[1, 1]):
                centre = float(k[1, 1])
        else:
            k = _kernel(DEFAULT_EDGE, DEFAULT_CORNER)
        nb = np.ones((3, 3), dtype=bool)
        nb[1, 1] = False
        if not np.isfinite(k[nb]).all():
            raise IpcConfigError("interpixel_capacitance: every neighbour weight must be finite")
        if (k[nb] < 0).any():
            raise IpcConfigError("interpixel_capacitance: every neighbour weight must be >= 0")
        if (k[nb] > 1).any():
            raise IpcConfigError("interpixel_capacitance: the neighbour weights sum to more than 1")
        w = np.zeros((3, 3), dtype=np.int64)
        w[nb] = np.rint(k[nb] * UNIT).astype(np.int64)
        total = int(w.sum())
        if total > UNIT:
            raise IpcConfigError("interpixel_capacitance: the neighbour weights sum to more than 1")
        if centre is not None and not abs(centre - (1.0 - float(k[nb].sum()))) <= CENTRE_TOLERANCE:
            raise IpcConfigError("interpixel_capacitance: the centre weight %g is not 1 - sum(neighbours) = %g: an "
                                 "unnormalised kernel" % (centre, 1.0 - float(k[nb].sum())))
        w[1, 1] = UNIT - total
        k = k.copy()
        k[1, 1] = 1.0 - float(k[nb].sum())
        self.kernel = k
        self._w = w.astype(np.int32)

    @staticmethod
    def from_config(section):
        """The YAML's `interpixel_capacitance:` section -> InterpixelCapacitance (`{}` or an empty section: the default
        kernel)."""
        if section is None:
            section = {}
        if not isinstance(section, dict):
            raise IpcConfigError("`interpixel_capacitance` must be a mapping with an optional `alpha` or `kernel` entry")
        unknown = sorted(set(map(str, section)) - {"alpha", "kernel"})
        if unknown:
            raise IpcConfigError("interpixel_capacitance: unknown key(s) %s (expected alpha or kernel)" % ", ".join(unknown))
        return InterpixelCapacitance(kernel=section.get("kernel"), alpha=section.get("alpha"))

    def weights(self):
        """The nine integer weights W [3, 3] int32, sum 65536 (what wayne_ipc_weights makes of `kernel`)."""
        return self._w.copy()

    def cards(self):
        """Primary-header cards of a coupled exposure: IPC = T, IPCUNIT = 65536 and the nine integer weights IPCWij."""
        out = [("IPC", True, "inter-pixel capacitance on"), ("IPCUNIT", UNIT, "IPC: the weights are in units of 1/IPCUNIT")]
        for i in range(3):
            for j in range(3):
                out.append(("IPCW%d%d" % (i, j), int(self._w[i, j]), "IPC: weight of the neighbour at (dy, dx) = (%d, %d)" % (i - 1, j - 1)))
        return out

    def digest_bytes(self):
        """What visit.descriptor_digest hashes: the law is a function of the integer weights alone."""
        return b"interpixel_capacitance" + struct.pack("<9i", *[int(v) for v in self._w.ravel()])

    def __eq__(self, other):
        return isinstance(other, InterpixelCapacitance) and self.digest_bytes() == other.digest_bytes()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self.digest_bytes())

    def __repr__(self):
        return "InterpixelCapacitance(kernel=%r)" % (self.kernel.tolist(),)


def as_ipc(ipc):
    """InterpixelCapacitance -> itself; True -> the default kernel; None / False -> None."""
    if ipc is None or ipc is False:
        return None
    if ipc is True:
        return InterpixelCapacitance()
    if isinstance(ipc, InterpixelCapacitance):
        return ipc
    raise TypeError("ipc: expected ipc.InterpixelCapacitance, True or None, got %r" % (ipc,))
