"""CPU: the validity rule of the upload-time per-wavelength arrays (plan::WlCache, wayne_amd/csrc/host_plan.h) through a
stand-alone native program under AddressSanitizer + UndefinedBehaviorSanitizer: same bytes, one changed double, changed
W, changed grism generation."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CXXFLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]     # (those of tests/native/Makefile)


def test_validity_rule_of_the_per_wavelength_arrays():
    build = os.path.join(NATIVE, "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "wl_cache_check")
    subprocess.check_call([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-o", exe, os.path.join(NATIVE, "wl_cache_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    got = [line.split() for line in p.stdout.splitlines()]
    want = {"empty_cache": "0", "same_bytes": "1", "same_bytes_other_array": "1", "one_changed_double": "0", "negative_zero": "0",
            "same_nan": "1", "shorter_W": "0", "longer_W": "0", "changed_generation": "0", "adopted_generation": "1",
            "earlier_generation": "0", "dropped": "0", "trace_table": "1"}
    assert len(got) == 15 and {name for name, _ in got} == set(want)
    for name, holds in got:
        assert holds == want[name], (name, holds)
