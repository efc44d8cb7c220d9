// Arithmetic of the tile flush (k_throw.h, flush_tile) that does not need the device: the walk of a thread over the
// cells of a tile, and the fixed-point conversion of a cell's charge.  No HIP header is included here: the file also
// compiles with plain g++ (tests/native/flush_check.cpp restates both against the division and llrint on the CPU).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "philox.h"   // WAYNE_HD

namespace wayne {

// ---- the walk ----
// Thread t of T visits the cells i = t, t + T, t + 2T, ... of a tile of width tw (row-major: i = ly tw + lx).  Cell i + T
// lies q = T / tw rows and rem = T % tw columns further on, and one more row further and tw columns back if that leaves
// the row: one division per thread for the start, one per workgroup for (q, rem), and additions from there on.  With
// the coordinates go two byte offsets, each linear in them: `fo` into a plane of pitch N with 4-byte cells (the flat
// planes, the int32 frame) and `ao` into a plane of pitch S with 8-byte cells (a read plane of the accumulator).
// All of it in 32 bits: offsets_fit_32() is the host's check that no cell of the frame lies beyond.
struct FlushWalk {
  int tw, x_end;            // tile width (>= 1); first frame column right of the tile
  int q, rem;               // T / tw, T % tw
  uint32_t fo_step, fo_wrap, ao_step, ao_wrap;
};
struct FlushCell {
  int x, y;                 // frame coordinates
  uint32_t fo, ao;
};

WAYNE_HD FlushWalk flush_walk(int T, int tw, int x0, int N, int S) {
  FlushWalk w;
  w.tw = tw; w.x_end = x0 + tw;
  w.q = T / tw; w.rem = T - w.q * tw;
  w.fo_step = ((uint32_t)w.q * (uint32_t)N + (uint32_t)w.rem) * 4u;
  w.ao_step = ((uint32_t)w.q * (uint32_t)S + (uint32_t)w.rem) * 8u;
  w.fo_wrap = (uint32_t)(N - tw) * 4u;
  w.ao_wrap = (uint32_t)(S - tw) * 8u;
  return w;
}
// the first cell of thread t.  (x0, y0): frame coordinates of the tile's corner; (ax, ay): what the 8-byte plane adds
// to a cell's coordinates (its border)
WAYNE_HD FlushCell flush_first(int t, int tw, int x0, int y0, int N, int S, int ax, int ay) {
  FlushCell c;
  const int ly = t / tw, lx = t - ly * tw;
  c.x = x0 + lx; c.y = y0 + ly;
  c.fo = ((uint32_t)c.y * (uint32_t)N + (uint32_t)c.x) * 4u;
  c.ao = ((uint32_t)(c.y + ay) * (uint32_t)S + (uint32_t)(c.x + ax)) * 8u;
  return c;
}
WAYNE_HD void flush_next(FlushCell& c, const FlushWalk& w) {
  c.x += w.rem; c.y += w.q; c.fo += w.fo_step; c.ao += w.ao_step;
  if (c.x >= w.x_end) { c.x -= w.tw; c.y += 1; c.fo += w.fo_wrap; c.ao += w.ao_wrap; }
}
// every byte offset of a cell of an S x S plane of 8-byte cells (hence of the N x N planes of 4-byte cells inside it)
// is below 2^32
WAYNE_HD bool offsets_fit_32(int N, int S) {
  return N >= 0 && S >= N && (uint64_t)S * (uint64_t)S * 8u <= 0xFFFFFFFFull;
}

// ---- the conversion ----
// q = rndne(v 2^28) as an int64.  For |v| < 2^23 the product is below 2^51 in magnitude, so v 2^28 + 1.5 x 2^52 lies in
// [2^52, 2^53), where doubles are the integers: the fma rounds the exact sum ONCE, to nearest-even -- the rounding that
// rndne applies to the (exact) product -- and the result's bit pattern is that of 1.5 x 2^52 plus q, in two's
// complement for either sign.  fixed_fast_ok is the guard: false for anything larger, for infinities and for NaN.
constexpr int kFixedBits = 28;
constexpr double kFixedScale = 268435456.0;        // 2^28 (common.h, kQ)
constexpr double kFixedGuard = 8388608.0;          // 2^23
constexpr double kFixedMagic = 6755399441055744.0; // 1.5 x 2^52 = 0x4338000000000000
WAYNE_HD bool fixed_fast_ok(double v) { return fabs(v) < kFixedGuard; }
WAYNE_HD long long fixed_fast(double v) {
  const double r = fma(v, kFixedScale, kFixedMagic);
  uint64_t b;
  memcpy(&b, &r, sizeof b);
  return (long long)(b - 0x4338000000000000ull);
}

}  // namespace wayne
