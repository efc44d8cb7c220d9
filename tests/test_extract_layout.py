"""Host side of the spectra block's layout (host_plan.h: plan::spectra_layout) and of the profile planes' offsets
(plan::profile_offsets), in a program of their own under the sanitizers, against tests/spectra_layout_law.py -- the
header's documentation restated.  GPU: tests/test_fixed_profile_gpu.py, test_every_product_lies_where_the_layout_says."""
import os
import shutil
import subprocess

import pytest

import spectra_layout_law as sll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES, READS, CHANNELS = (74, 266, 1024), (1, 2, 3, 4, 15), (1, 5, 64)

HARNESS = r"""
#include <climits>
#include <cstdio>
#include "host_plan.h"
using namespace wayne;
static long long show(size_t v) { return v == plan::kNoRegion ? -1LL : (long long)v; }
int main() {
  const int sides[] = {74, 266, 1024}, reads[] = {1, 2, 3, 4, 15}, chans[] = {0, 1, 5, 64};
  for (int S : sides) for (int R : reads) for (int C : chans)
    for (int cr = 0; cr < 2; ++cr) for (int var = 0; var < 2; ++var) for (int opt = 0; opt <= var; ++opt)
      for (int oc = 0; oc <= (opt && C ? 1 : 0); ++oc) {
        const plan::SpectraLayout l = plan::spectra_layout(S, R, cr, C, var, opt, oc);
        std::printf("L %d %d %d %d %d %d %d : %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", S, R, cr, C, var, opt, oc,
                    show(l.spectra), show(l.sky), show(l.n_rejected), show(l.channels), show(l.spectra_var), show(l.sky_var),
                    show(l.channels_var), show(l.optimal), show(l.optimal_var), show(l.channels_opt), show(l.channels_opt_var),
                    show(l.bytes));
      }
  // a switch whose footing is off counts as off
  const plan::SpectraLayout a = plan::spectra_layout(74, 2, true, 0, false, true, true), b = plan::spectra_layout(74, 2, true, 0, false, false, false);
  const plan::SpectraLayout d = plan::spectra_layout(74, 2, true, 0, true, true, true), e = plan::spectra_layout(74, 2, true, 0, true, true, false);
  std::printf("F %d %d\n", a.bytes == b.bytes && a.optimal == plan::kNoRegion, d.bytes == e.bytes && d.channels_opt == plan::kNoRegion);
  // the profile planes' offsets: the windows of tests/test_fixed_profile.py at S = 266, R = 3
  const int lo[4] = {100, 110, 120, 100}, hi[4] = {140, 150, 160, 160};
  const int wild_lo[4] = {100, 110, 120, INT_MIN}, wild_hi[4] = {140, 150, 160, INT_MAX};
  const int back_lo[4] = {100, 110, 120, INT_MAX}, back_hi[4] = {140, 150, 160, INT_MIN};
  const unsigned no_last = X_ALL & ~X_LAST_READ;
  struct { const char* name; const int *lo, *hi; unsigned steps; } cases[] = {
      {"wild", wild_lo, wild_hi, no_last}, {"back", back_lo, back_hi, no_last}, {"plain", lo, hi, no_last}, {"formed", lo, hi, X_ALL}};
  for (const auto& c : cases) {
    size_t off[4] = {7, 7, 7, 7};
    const size_t n = plan::profile_offsets(266, 3, c.steps, c.lo, c.hi, off);
    std::printf("P %s %zu %zu %zu %zu %zu %d\n", c.name, off[0], off[1], off[2], off[3], n,
                n == plan::profile_offsets(266, 3, c.steps, c.lo, c.hi, nullptr));
  }
  std::printf("checked\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("extract_layout")
    src = tmp / "extract_layout.cpp"
    src.write_text(HARNESS)
    exe = str(tmp / "extract_layout")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "wayne_amd", "csrc"), str(src), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "checked" in r.stdout, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def layouts(printed):
    """{(S, R, crrej, C, variance, optimal, optimal_channels): ({region: offset} of the regions that are on, bytes)}"""
    out = {}
    for line in printed:
        if line.startswith("L "):
            key, values = line[2:].split(" : ")
            values = [int(x) for x in values.split()]
            off = {name: at for name, at in zip(sll.ORDER, values[:-1]) if at != -1}
            out[tuple(int(x) for x in key.split())] = (off, values[-1])
    return out


def test_spectra_layout_is_the_documented_one(printed):
    got = layouts(printed)
    want = {}
    for S in SIDES:
        for R in READS:
            for options, with_c in sll.combinations():
                for C in (CHANNELS if with_c else (0,)):
                    key = (S, R, int(options["crrej"]), C, int(options["variance"]), int(options["optimal"]), int(options["optimal_channels"]))
                    want[key] = sll.layout(S, R, C=C, **options)
    assert len(want) == 3 * 5 * 2 * (3 + 3 * 4) and sorted(got) == sorted(want)        # every legal combination, and no other
    for key in sorted(want):
        assert got[key] == want[key], key
    assert "F 1 1" in printed


def test_spectra_layout_properties(printed):
    got = layouts(printed)
    padded = 0
    for key, (off, total) in got.items():
        S, R, crrej, C, variance, optimal, optch = key
        size = sll.sizes(S, R, crrej=bool(crrej), C=C, variance=bool(variance), optimal=bool(optimal), optimal_channels=bool(optch))
        names = list(off)
        assert names == list(size) == [n for n in sll.ORDER if n in off], key          # the regions that are on, in the documented order
        assert off["spectra"] == 0
        for a, b in zip(names, names[1:]):
            assert off[a] + size[a] <= off[b], (key, a, b)                              # disjoint
            padded += off[a] + size[a] < off[b]
        assert all(off[n] % 8 == 0 for n in names if n != "n_rejected"), key            # float64 regions on 8 bytes
        assert off.get("n_rejected", 0) % 4 == 0
        assert total == off[names[-1]] + size[names[-1]], key                           # bytes: the end of the last region
        # the reservation rule: the block without rejection is never longer than with it
        with_cr = got[(S, R, 1, C, variance, optimal, optch)][1]
        assert got[(S, R, 0, C, variance, optimal, optch)][1] <= with_cr
    assert padded > 0                                                                   # (R + 1 odd: the padding rule was exercised)


def test_profile_offsets_of_the_three_windows(printed):
    S = 266
    want = {"wild": (40, 40, 40, 266), "back": (40, 40, 40, 0), "plain": (40, 40, 40, 60), "formed": (40, 40, 40, 60)}
    lines = {l.split()[1]: [int(x) for x in l.split()[2:]] for l in printed if l.startswith("P ")}
    assert sorted(lines) == sorted(want)
    for name, rows in want.items():
        starts = [sum(rows[:p]) * S for p in range(4)]
        assert lines[name] == starts + [sum(rows) * S, 1], name
