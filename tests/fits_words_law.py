"""The law of the device-side FITS words (include/wayne_hip.h, "device-side FITS words"), in numpy.

For reads P_0 .. P_R (each S x S, bordered) of sample type T the payload is (R + 1) * stride bytes:

    words(v) = T float32 : the 8 bytes of (double)v, most significant first       np.asarray(P, '>f8')
               T float64 : the 8 bytes of v, most significant first               np.asarray(P, '>f8')
               T uint16  : the 2 bytes of (v XOR 0x8000), most significant first  fitsio.u16_to_stored(P)
    B        = 8, 8, 2                     plane_bytes = S * S * B
    stride   = plane_bytes rounded up to a multiple of 2880
    payload[f * stride + i * B ...]                      = words(P_{R - f} flat [i])      f = 0 .. R: the last read first
    payload[f * stride + plane_bytes .. (f + 1) * stride) = 0

Tolerance 0: widening float32 to float64 is exact and the rest is a permutation of bytes.  NaN payload bits are outside the
law (reads are clipped and finite)."""
import numpy as np

from wayne_amd import fitsio

BLOCK = 2880


def layout(S, R, dtype):
    """(plane_bytes, stride, bitpix) for bordered side S, R reads behind the zero read and the reads' dtype."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.uint16)):
        raise ValueError("no FITS words for reads of %s" % dtype)
    B = 2 if dtype == np.uint16 else 8
    plane_bytes = S * S * B
    stride = -(-plane_bytes // BLOCK) * BLOCK
    return plane_bytes, stride, 16 if dtype == np.uint16 else -64


def words(plane):
    """The stored bytes of one read (a uint8 array of plane_bytes)."""
    plane = np.ascontiguousarray(plane)
    if plane.dtype == np.uint16:
        stored = fitsio.u16_to_stored(plane)          # big-endian int16 of value - 32768
    else:
        stored = np.asarray(plane, dtype=">f8")
    return np.frombuffer(np.ascontiguousarray(stored).tobytes(), dtype=np.uint8)


def payload(reads):
    """The payload of reads [R + 1, S, S] (read 0 first): a uint8 array of (R + 1) * stride bytes."""
    reads = np.asarray(reads)
    n, S = reads.shape[0], reads.shape[1]
    assert reads.ndim == 3 and reads.shape[2] == S and n >= 2
    plane_bytes, stride, _ = layout(S, n - 1, reads.dtype)
    out = np.zeros(n * stride, dtype=np.uint8)
    for f in range(n):
        out[f * stride:f * stride + plane_bytes] = words(reads[n - 1 - f])
    return out


def clock_free(raw):
    """A file's bytes with the value of the primary header's clock-dependent cards (DATE, SIM-TIME) blanked: what two
    writes of the same exposure at different moments have in common."""
    raw = bytearray(raw)
    for at in range(0, len(raw), 80):
        card = bytes(raw[at:at + 80])
        if card.startswith(b"END     "):
            break
        if card[:8] in (b"DATE    ", b"SIM-TIME"):
            raw[at + 8:at + 80] = b" " * 72
    return bytes(raw)


def plane_of(payload_bytes, f, S, dtype):
    """Plane f of a payload back as an [S, S] array of the reads' values (float64 for float reads), and its padding."""
    plane_bytes, stride, _ = layout(S, 1, dtype)
    raw = np.asarray(payload_bytes)[f * stride:(f + 1) * stride]
    data, pad = raw[:plane_bytes], raw[plane_bytes:]
    if np.dtype(dtype) == np.uint16:
        vals = (np.frombuffer(data.tobytes(), dtype=">i2").astype(np.int32) + 32768).astype(np.uint16)
    else:
        vals = np.frombuffer(data.tobytes(), dtype=">f8").astype(np.float64)
    return vals.reshape(S, S), pad
