"""The inter-pixel capacitance law in numpy, on int64 (wayne_amd/ipc.py states it; k_ipc.h is held to it bit for bit).

    W[i][j] = rint(k[i][j] * 65536) for the eight neighbours, W[1][1] = 65536 - sum of them
    q'[y, x] = floor((sum_{dy, dx} W[dy+1][dx+1] q[y+dy, x+dx] + 32768) / 65536),  q = 0 beyond the frame,
    q' = 0 on the `border`-pixel reference border

The sum is formed without overflow for any int64 q: q = hi 2^32 + lo with hi the arithmetic high half and lo the unsigned
low 32 bits, S_hi = sum W hi, S_lo = sum W lo, q' = (S_hi << 16) + ((S_lo + 32768) >> 16).
"""
import numpy as np

UNIT = 65536
BORDER = 5


def weights(kernel):
    """The nine integer weights [3, 3] int64 of a kernel of doubles; ValueError for a neighbour that is not finite, is
    negative, or when the rounded neighbours sum to more than 65536.  kernel[1][1] is not looked at."""
    k = np.array(kernel, dtype=np.float64)
    if k.shape != (3, 3):
        raise ValueError("the kernel is 3 x 3")
    nb = np.ones((3, 3), dtype=bool)
    nb[1, 1] = False
    if not np.isfinite(k[nb]).all() or (k[nb] < 0).any() or (k[nb] > 1).any():
        raise ValueError("neighbour weights must be finite, >= 0 and sum to at most 1")
    w = np.zeros((3, 3), dtype=np.int64)
    w[nb] = np.rint(k[nb] * UNIT).astype(np.int64)
    if int(w.sum()) > UNIT:
        raise ValueError("the neighbour weights sum to more than 1")
    w[1, 1] = UNIT - int(w.sum())
    return w


def _shifted(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx], 0 beyond the frame."""
    out = np.zeros_like(a)
    H, Wd = a.shape[-2:]
    ys = slice(max(0, -dy), min(H, H - dy))
    xs = slice(max(0, -dx), min(Wd, Wd - dx))
    yd = slice(max(0, -dy) + dy, min(H, H - dy) + dy)
    xd = slice(max(0, -dx) + dx, min(Wd, Wd - dx) + dx)
    out[..., ys, xs] = a[..., yd, xd]
    return out


def couple(q, w, border=BORDER):
    """q [..., S, S] int64, w [3, 3] integer weights -> q' int64."""
    q = np.ascontiguousarray(q, dtype=np.int64)
    w = np.asarray(w, dtype=np.int64)
    hi = q >> 32                                    # arithmetic
    lo = (q & 0xFFFFFFFF).astype(np.uint64)
    s_hi = np.zeros(q.shape, dtype=np.int64)
    s_lo = np.zeros(q.shape, dtype=np.uint64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            wt = int(w[dy + 1, dx + 1])
            s_hi += np.int64(wt) * _shifted(hi, dy, dx)
            s_lo += np.uint64(wt) * _shifted(lo, dy, dx)
    low = ((s_lo + np.uint64(32768)) >> np.uint64(16)).astype(np.int64)
    with np.errstate(over="ignore"):
        out = (s_hi << 16) + low
    if border:
        out[..., :border, :] = 0
        out[..., -border:, :] = 0
        out[..., :, :border] = 0
        out[..., :, -border:] = 0
    return out


def couple_bigint(q, w, border=BORDER):
    """The same law on Python integers (one plane [S, S]): the statement `couple` is checked against."""
    q = np.asarray(q)
    H, Wd = q.shape
    rows = [[int(v) for v in row] for row in q.tolist()]
    wl = [[int(v) for v in row] for row in np.asarray(w).tolist()]
    out = np.zeros((H, Wd), dtype=object)
    for y in range(H):
        for x in range(Wd):
            if border and (y < border or y >= H - border or x < border or x >= Wd - border):
                continue
            s = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < Wd:
                        s += wl[dy + 1][dx + 1] * rows[yy][xx]
            out[y, x] = (s + 32768) // 65536
    return out
