"""CPU: the arithmetic of the thrower's tile flush (wayne_amd/csrc/flush_math.h; k_throw.h, flush_tile) through a
stand-alone native program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/native/flush_check.cpp):

  * the walk of a thread over a tile's cells by additions -- one division for the start, then (q, rem) = (T / tw, T % tw)
    per step and a wrap -- gives (i % tw, i / tw) and the cell's two byte offsets for every tile width 1 ... 9216,
    T = 256 and 512, every thread and every step (tw > T, rem = 0, tw = 1 and ragged last passes are among them);
  * the one-rounding fixed-point conversion equals llrint(v 2^28) on 10^7 random v in (-2^23, 2^23), on every kind of
    tie, on +-0 and on the guard's edge values, and the guard refuses +-2^23, NaN and the infinities.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CXXFLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]     # (those of tests/native/Makefile)

_lines = {}


def check_lines():
    if not _lines:
        build = os.path.join(NATIVE, "_build")
        os.makedirs(build, exist_ok=True)
        exe = os.path.join(build, "flush_check")
        subprocess.check_call([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-o", exe, os.path.join(NATIVE, "flush_check.cpp")])
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        for line in p.stdout.splitlines():
            name, cases, bad = line.split()
            _lines[name] = (int(cases), int(bad))
        print(p.stdout)
    return _lines


def test_stepped_coordinates_equal_the_division():
    got = check_lines()
    for name in ("walk_T256", "walk_T512"):
        cases, bad = got[name]
        # every width's tile is visited cell by cell: 9216 widths of up to 9216 cells
        assert cases > 9216 * 9216 // 2, (name, cases)
        assert bad == 0, (name, bad)
    assert got["offsets_fit_32"] == (6, 0)


def test_one_rounding_conversion_equals_llrint():
    got = check_lines()
    assert set(got) == {"walk_T256", "walk_T512", "offsets_fit_32", "convert_random", "convert_ties", "convert_edges"}
    assert got["convert_random"][0] >= 10000000 and got["convert_random"][1] == 0
    assert got["convert_ties"][0] > 4000000 and got["convert_ties"][1] == 0
    assert got["convert_edges"] == (22, 0)
