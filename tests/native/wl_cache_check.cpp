// Stand-alone check of plan::WlCache (wayne_amd/csrc/host_plan.h): when the per-wavelength arrays a source holds on the
// device are still the ones of an upload.  Built with g++ -fsanitize=address,undefined and run by tests/test_prep_cache.py.
// Prints one line per case ("<case> <holds: 0/1>") and exits 0; a wrong answer exits 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../wayne_amd/csrc/host_plan.h"

using wayne::plan::WlCache;

static int bad = 0;
static void expect(const char* what, bool got, bool want) {
  std::printf("%s %d\n", what, got ? 1 : 0);
  if (got != want) { std::printf("  WRONG: expected %d\n", want ? 1 : 0); bad = 1; }
}

int main() {
  const int W = 1201;
  std::vector<double> wl(W);
  for (int i = 0; i < W; ++i) wl[i] = 1.1 + 5e-4 * i;
  WlCache c;
  expect("empty_cache", c.holds(W, wl.data(), 1), false);
  c.adopt(W, wl.data(), 1);
  expect("same_bytes", c.holds(W, wl.data(), 1), true);
  std::vector<double> copy(wl);                       // another array with the same bytes
  expect("same_bytes_other_array", c.holds(W, copy.data(), 1), true);
  for (int i : {0, W / 2, W - 1}) {                   // one changed double, by one ulp, anywhere
    std::vector<double> v(wl);
    v[i] = std::nextafter(v[i], 2.0);
    expect("one_changed_double", c.holds(W, v.data(), 1), false);
  }
  {
    std::vector<double> v(wl);                        // the sign of a zero is a change of the bytes
    std::vector<double> z(wl);
    v[3] = 0.0; z[3] = -0.0;
    WlCache cz; cz.adopt(W, v.data(), 1);
    expect("negative_zero", cz.holds(W, z.data(), 1), false);
    v[3] = z[3] = std::numeric_limits<double>::quiet_NaN();   // ... and a NaN with the same bytes is the same grid
    cz.adopt(W, v.data(), 1);
    expect("same_nan", cz.holds(W, z.data(), 1), true);
  }
  expect("shorter_W", c.holds(W - 1, wl.data(), 1), false);         // a prefix of the grid is another grid
  {
    std::vector<double> v(wl);
    v.push_back(1.8);
    expect("longer_W", c.holds(W + 1, v.data(), 1), false);
  }
  expect("changed_generation", c.holds(W, wl.data(), 2), false);
  c.adopt(W, wl.data(), 2);
  expect("adopted_generation", c.holds(W, wl.data(), 2), true);
  expect("earlier_generation", c.holds(W, wl.data(), 1), false);
  c.drop();
  expect("dropped", c.holds(W, wl.data(), 2), false);
  // trace_table: kTrStride doubles per sub-sample, t[6] = 1 / t[4], t[7] = 0, the six of trace_coeffs in front
  wayne::GrismDev g{};
  for (int i = 0; i < 9; ++i) { g.trace[i] = 1e-3 * (i + 1); g.wlsol[i] = 40.0 + 1e-3 * i; }
  const double xr[3] = {400.5, 401.0, 402.25}, yr[3] = {500.0, 510.5, 521.75};
  std::vector<double> tr(3 * wayne::kTrStride, -1.0);
  wayne::plan::trace_table(g, 3, xr, yr, tr.data());
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    double t[6];
    wayne::trace_coeffs(g, xr[k], yr[k], t);
    const double* o = tr.data() + wayne::kTrStride * k;
    for (int i = 0; i < 6; ++i) ok = ok && o[i] == t[i];
    ok = ok && o[6] == 1. / t[4] && o[7] == 0.;
  }
  expect("trace_table", ok, true);
  return bad;
}
