"""TEST INFRASTRUCTURE: the law of the device's calibrated reads (include/wayne_hip.h, wayne_ima_desc; k_ima) restated in
numpy, float64 throughout, payload included.  Shared by tests/test_ima.py (the law's own properties, on CPU-oracle reads)
and tests/test_ima_gpu.py (the oracle of the device, applied to the slot's own downloaded reads).

For a light-sensitive pixel with reads P_k (k = 0 .. R), L_k / g the extraction's (extraction_law.Planes; the electrons are
rampfit_law.electrons, K is rampfit_law.usable) and dt_j the read intervals:

    t_0 = 0, t_k = sum_{j<k} dt_j (ascending);   e_0 = 0, e_k = L_k g;   q = g / 2.35
    s_k = sqrt(max(e_k, 0) + rn^2 (q q))   (k >= 1; s_0 = 0)
    counts: SCI_k = float32(e_k), ERR_k = float32(s_k);   rate: SCI_k = float32(e_k / t_k), ERR_k = float32(s_k / t_k); read 0: 0
    DQ_k = (k > K or (k = 0 and K = 0 and not P_0 < sat) ? 256 : 0) | (some bit j < k of the ramp fit's jump ? 8192 : 0)
    the 5-pixel border: SCI = ERR = 0, DQ = 0

Tolerance: none.  Every float64 operation above is one correctly rounded operation, the kernel is compiled without
contraction, the float32 cast rounds to nearest even on both sides and the comparisons with sat are on the reads as
stored -- so the device's payload equals this one byte for byte (NaN samples compared as NaN, not by pattern)."""
import collections

import numpy as np

import rampfit_law

LINEARISE, DARK, GAIN = 1, 2, 4
DQ_SATURATED, DQ_JUMP = 256, 8192
BORDER = 5
BLOCK = 2880

Law = collections.namedtuple("Law", "sci err dq e K t")


def pad(b):
    return (b + BLOCK - 1) // BLOCK * BLOCK


def strides(S):
    """(sci_stride, dq_stride, imset_stride) of a frame of side S: the formula of the issue, nothing else."""
    n = S * S
    return pad(4 * n), pad(2 * n), 2 * pad(4 * n) + pad(2 * n)


def times(dt):
    """t_k, k = 0 .. R: the read intervals summed in ascending order."""
    t = [0.0]
    for d in np.asarray(dt, dtype=np.float64):
        t.append(t[-1] + float(d))
    return np.array(t)


def restate(reads, pl, units="rate", rn=20.0, sat_dn=65000.0, steps=LINEARISE | DARK | GAIN, jump=None):
    """The law on a slot's reads [R + 1, S, S]: Law of sci, err [R + 1, S, S] float32, dq [R + 1, S, S] int16, and the
    float64 electrons e, K and t_k it went through.  `jump`: the low 16 bits of the ramp fit's word [S, S], or None."""
    reads = np.asarray(reads)
    R, S = reads.shape[0] - 1, reads.shape[-1]
    e = rampfit_law.electrons(reads, pl, steps)
    K = rampfit_law.usable(reads, sat_dn)
    t = times(pl.dt)
    q = pl.gain / 2.35
    rq = (rn * rn) * (q * q)
    with np.errstate(invalid="ignore"):
        first_good = reads[0].astype(np.float64) < sat_dn
    inner = np.zeros((S, S), dtype=bool)
    inner[BORDER:-BORDER, BORDER:-BORDER] = True
    sci = np.zeros((R + 1, S, S), dtype=np.float32)
    err = np.zeros((R + 1, S, S), dtype=np.float32)
    dq = np.zeros((R + 1, S, S), dtype=np.int16)
    jump = np.zeros((S, S), dtype=np.uint32) if jump is None else (np.asarray(jump, dtype=np.uint32) & np.uint32(0xFFFF))
    for k in range(R + 1):
        if k == 0:
            flag = np.where((K == 0) & ~first_good, DQ_SATURATED, 0)
        else:
            with np.errstate(all="ignore"):
                s = np.sqrt(np.maximum(e[k], 0.0) + rq)
                a, b = (e[k] / t[k], s / t[k]) if units == "rate" else (e[k], s)
                sci[k] = np.where(inner, a, 0.0).astype(np.float32)
                err[k] = np.where(inner, b, 0.0).astype(np.float32)
            flag = np.where(k > K, DQ_SATURATED, 0) | np.where((jump & np.uint32((1 << k) - 1)) != 0, DQ_JUMP, 0)
        dq[k] = np.where(inner, flag, 0).astype(np.int16)
    return Law(sci, err, dq, e, K, t)


def payload(law):
    """The law's planes as the device lays them out: one uint8 array, the last read first, every section padded with
    zeros to its stride."""
    R, S = law.sci.shape[0] - 1, law.sci.shape[-1]
    sci_stride, dq_stride, imset = strides(S)
    n = S * S
    out = np.zeros((R + 1) * imset, dtype=np.uint8)
    for f in range(R + 1):
        k = R - f
        at = f * imset
        out[at:at + 4 * n] = law.sci[k].astype(">f4").reshape(-1).view(np.uint8)
        out[at + sci_stride:at + sci_stride + 4 * n] = law.err[k].astype(">f4").reshape(-1).view(np.uint8)
        out[at + 2 * sci_stride:at + 2 * sci_stride + 2 * n] = law.dq[k].astype(">i2").reshape(-1).view(np.uint8)
    return out


def sections(buf, S, R):
    """A payload -> (sci, err [R + 1, S, S] float32, dq [R + 1, S, S] int16, padding: every byte outside the data)."""
    sci_stride, dq_stride, imset = strides(S)
    n = S * S
    buf = np.asarray(buf, dtype=np.uint8)
    assert buf.size == (R + 1) * imset
    sci = np.empty((R + 1, S, S), dtype=np.float32)
    err = np.empty((R + 1, S, S), dtype=np.float32)
    dq = np.empty((R + 1, S, S), dtype=np.int16)
    rest = []
    for f in range(R + 1):
        k = R - f
        at = f * imset
        sci[k] = buf[at:at + 4 * n].view(">f4").reshape(S, S)
        rest.append(buf[at + 4 * n:at + sci_stride])
        err[k] = buf[at + sci_stride:at + sci_stride + 4 * n].view(">f4").reshape(S, S)
        rest.append(buf[at + sci_stride + 4 * n:at + 2 * sci_stride])
        dq[k] = buf[at + 2 * sci_stride:at + 2 * sci_stride + 2 * n].view(">i2").reshape(S, S)
        rest.append(buf[at + 2 * sci_stride + 2 * n:at + imset])
    return sci, err, dq, np.concatenate(rest)


def assert_parity(got, want, what=""):
    """The device's payload against the law's, byte for byte; a sample that is NaN in the law must be NaN on the device
    (its pattern is not specified).  Prints how many bytes, flags and NaNs were compared."""
    got = np.asarray(got)
    R, S = want.sci.shape[0] - 1, want.sci.shape[-1]
    assert got.dtype == np.uint8 and got.size == (R + 1) * strides(S)[2], what
    sci, err, dq, rest = sections(got, S, R)
    nan_s, nan_e = np.isnan(want.sci), np.isnan(want.err)
    print("%s: %d bytes; %d samples flagged 256, %d flagged 8192, %d NaN; %d bytes of padding" % (
        what, got.size, int(((want.dq & DQ_SATURATED) != 0).sum()), int(((want.dq & DQ_JUMP) != 0).sum()),
        int(nan_s.sum() + nan_e.sum()), rest.size))
    assert not rest.any(), what + ": the padding is not zero"
    assert (np.isnan(sci) == nan_s).all() and (np.isnan(err) == nan_e).all(), what + ": NaN samples differ"
    for name, a, b in (("SCI", sci, want.sci), ("ERR", err, want.err)):
        differ = (a.view(np.uint32) != b.view(np.uint32)) & ~np.isnan(b)
        assert not differ.any(), (what, name, int(differ.sum()), np.argwhere(differ)[:4].tolist(),
                                  a[differ][:4].tolist(), b[differ][:4].tolist())
    differ = dq != want.dq
    assert not differ.any(), (what, "DQ", int(differ.sum()), np.argwhere(differ)[:4].tolist())
    if not (nan_s.any() or nan_e.any()):
        np.testing.assert_array_equal(got, payload(want), err_msg=what)
