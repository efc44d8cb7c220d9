// CPU check of wayne_amd/csrc/flush_math.h, the arithmetic of the thrower's tile flush (k_throw.h, flush_tile), built
// with the sanitizer flags of tests/native/Makefile and run by tests/test_flush_math.py.
//   walk:     for every tile width tw = 1 ... 9216, T in {256, 512}, every thread and every step up to
//             tarea = min(tw th, 9216): the stepped cell is (i % tw, i / tw) and its two byte offsets are those of the
//             cell's frame coordinates
//   convert:  fixed_fast(v) == llrint(v 2^28) for every v the guard lets through; the guard refuses the rest
// One line per check: "<name> <cases> <failures>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>

#include "../../wayne_amd/csrc/flush_math.h"

using namespace wayne;

static long long walk_check(int T, long long* cases) {
  long long bad = 0;
  const int kTile = 9216;
  for (int tw = 1; tw <= kTile; ++tw) {
    // a tile height that leaves the last pass over the threads ragged wherever the width allows it
    const int th_full = kTile / tw, th = th_full > 3 ? th_full - (tw % 3) : th_full;
    const int tarea = tw * th < kTile ? tw * th : kTile;
    // the frame around the tile: its corner, and planes a little wider than the tile (N) and than that (S)
    const int x0 = 1 + tw % 7, y0 = 1 + tw % 5, border = 5;
    const int N = x0 + tw + tw % 11, S = N + 2 * border;
    const FlushWalk w = flush_walk(T, tw, x0, N, S);
    if (w.q != T / tw || w.rem != T % tw) ++bad;
    for (int t = 0; t < T && t < tarea; ++t) {
      FlushCell c = flush_first(t, tw, x0, y0, N, S, border, border);
      for (int i = t; i < tarea; i += T, flush_next(c, w)) {
        const int lx = i % tw, ly = i / tw;
        const uint32_t fo = (uint32_t)(((y0 + ly) * N + x0 + lx) * 4);
        const uint32_t ao = (uint32_t)(((y0 + ly + border) * S + x0 + lx + border) * 8);
        if (c.x != x0 + lx || c.y != y0 + ly || c.fo != fo || c.ao != ao) ++bad;
        ++*cases;
      }
    }
  }
  return bad;
}

static bool convert_ok(double v) { return fixed_fast_ok(v) && fixed_fast(v) == llrint(v * 268435456.0); }

int main() {
  for (int T : {256, 512}) {
    long long cases = 0;
    const long long bad = walk_check(T, &cases);
    std::printf("walk_T%d %lld %lld\n", T, cases, bad);
  }
  // offsets_fit_32: the largest plane whose last cell is still below 2^32 bytes
  {
    long long bad = 0;
    if (!offsets_fit_32(1014, 1024) || !offsets_fit_32(23160, 23170) || offsets_fit_32(23161, 23171) ||
        offsets_fit_32(40000, 40010) || offsets_fit_32(-1, 9) || offsets_fit_32(100, 90))
      ++bad;
    std::printf("offsets_fit_32 6 %lld\n", bad);
  }
  {
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> u(-8388608.0, 8388608.0);
    long long bad = 0, n = 0;
    while (n < 10000000) {
      const double v = u(rng);
      if (!(std::fabs(v) < 8388608.0)) continue;
      if (!convert_ok(v)) ++bad;
      ++n;
    }
    // ... and small magnitudes, where most of a double's bits lie below the grid
    std::uniform_real_distribution<double> e(-60.0, 23.0);
    for (int i = 0; i < 1000000; ++i, ++n) {
      const double v = std::ldexp(1.0 + u(rng) * 0x1p-24, (int)e(rng)) * (i & 1 ? -1.0 : 1.0);
      if (std::fabs(v) < 8388608.0 && !convert_ok(v)) ++bad;
    }
    std::printf("convert_random %lld %lld\n", n, bad);
  }
  {
    // every tie: (k + 1/2) 2^-28 for integers k around 0, around +-2^51 (the guard's edge) and spread between
    long long bad = 0, n = 0;
    auto tie = [&](long long k) {
      const double v = std::ldexp((double)k + 0.5, -28);       // exact: |k| < 2^51
      if (!fixed_fast_ok(v)) return;
      const long long want = (k & 1) ? k + 1 : k;               // to the even neighbour
      if (fixed_fast(v) != want || llrint(v * 268435456.0) != want) ++bad;
      ++n;
    };
    for (long long k = -2000000; k <= 2000000; ++k) tie(k);
    for (long long k = (1ll << 51) - 2000000; k < (1ll << 51); ++k) { tie(k); tie(-k - 1); }
    for (long long k = 1; k < (1ll << 51); k += 1099511627775ll) { tie(k); tie(-k); tie(k + 1); tie(-k - 1); }
    std::printf("convert_ties %lld %lld\n", n, bad);
  }
  {
    long long bad = 0;
    const double edge = std::nextafter(8388608.0, 0.0);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // through the fast path: zeros (either sign gives 0), the guard's edge values, the smallest and a plain number
    const double in[] = {0.0, -0.0, edge, -edge, 5e-324, -5e-324, 1.25 * 4238.0, -1.25 * 4238.0, 0x1p-29, -0x1p-29, 0x1.8p-29};
    for (double v : in)
      if (!convert_ok(v)) ++bad;
    if (fixed_fast(0.0) != 0 || fixed_fast(-0.0) != 0) ++bad;
    // refused by the guard
    const double out[] = {8388608.0, -8388608.0, std::nextafter(8388608.0, inf), 1e30, -1e30, nan, -nan, inf, -inf};
    for (double v : out)
      if (fixed_fast_ok(v)) ++bad;
    std::printf("convert_edges %d %lld\n", (int)(sizeof in / sizeof in[0] + sizeof out / sizeof out[0]) + 2, bad);
  }
  return 0;
}
