#!/usr/bin/env python3
"""DESIGN.md is GENERATED: scripts/design_template.md + the round's measurement files -> DESIGN.md.

    python scripts/make_design.py [--round r06] [--check]

Every number in DESIGN.md is a placeholder `{{file.key.path|format}}` (optionally `{{file.key*1000|.1f}}`) in the
template, filled from ONE source file under profiles/<round>/:
    b   bench.json            the line `python bench.py --full` printed on the GPU box (scripts/collect_round.sh)
    s   visit_science.json    scripts/visit_science.py --cfg3 1024 --cfg4 480 --cfg2 100 --cfg5-g102 192
    k   kernel_stats.json     per-kernel averages of `rocprofv3 --kernel-trace --stats` of the same bench command
                              (scripts/summarize_kernel_stats.py writes it from kernel_stats.csv)
    t   k_ramp_traffic.json   HBM bytes of k_ramp from the PMC passes
    v   valu_issue.json       vector-pipe occupancy from the SQ counters
    a   ab_bin_local.json     the A/B of the bin-local coordinates on one box (scripts/ab_summary.py)
    e   kernel_stats_thrower_electron.json   kernel averages of `bench.py --thrower electron` under rocprofv3
    n   visit_science_test.json    what tests/test_visit_science_gpu.py measured (negative control, injected difference)
    x   ../extract.json       scripts/bench_extract.py (not a round's file)
    c   ../crrej.json         scripts/bench_crrej.py (nor this)
    h   ../channels.json      scripts/bench_channels.py (nor this)
    d   (derived)             computed here: d.traffic_over_algorithmic (t over b), and the fit lines of
                              thrower_vs_electrons.txt (d.lane_t0_us, d.lane_us_per_1e9, d.narrow_t0_us)
so the document cannot drift from the measurements: tests/test_design_doc.py renders the template again and compares
(`--check` does the same from the command line), and holds it to 400 lines.
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPLATE = os.path.join(ROOT, "scripts", "design_template.md")
OUT = os.path.join(ROOT, "DESIGN.md")
FILES = {"b": "bench.json", "s": "visit_science.json", "k": "kernel_stats.json", "t": "k_ramp_traffic.json",
         "v": "valu_issue.json", "a": "ab_bin_local.json", "e": "kernel_stats_thrower_electron.json",
         "n": "visit_science_test.json",
         "x": os.path.join("..", "extract.json"),        # (not a round's file: scripts/bench_extract.py)
         "c": os.path.join("..", "crrej.json"),          # (nor this: scripts/bench_crrej.py)
         "h": os.path.join("..", "channels.json")}       # (nor this: scripts/bench_channels.py)
PLACEHOLDER = re.compile(r"\{\{([a-z])\.([^|*}]+)(?:\*([0-9.eE+-]+))?\|([^}]*)\}\}")


def load(round_name):
    data = {}
    for key, name in FILES.items():
        p = os.path.join(ROOT, "profiles", round_name, name)
        data[key] = json.load(open(p)) if os.path.exists(p) else None
    data["d"] = derive_fits(round_name, derive(data))
    return data


def derive(data):
    d = {}
    try:
        t = [v for k, v in data["t"].items() if isinstance(v, dict) and "hbm_bytes_per_launch" in v][0]
        d["traffic_MB"] = t["hbm_bytes_per_launch"] / 1e6
        d["traffic_over_algorithmic"] = t["hbm_bytes_per_launch"] / data["b"]["roofline"]["bytes_per_launch"]
        nc = data["n"]["negative_control_dropped_fraction"]
        ratio = [abs(o) / s for o, s in zip(nc["offset_ppm"], nc["sigma_ppm"])]
        d["negctl_max_offset_ppm"] = max(abs(o) for o in nc["offset_ppm"])
        d["negctl_max_sigmas"] = max(ratio)
        sh = data["n"]["cfg3"]["paired"]["production_minus_per_electron"]["ramp"]
        d["shipped_max_offset_sigmas"] = max(abs(o) / s for o, s in zip(sh["channel_flux_offset_ppm"], sh["channel_flux_offset_sigma_ppm"]))
    except (TypeError, KeyError, IndexError):
        pass
    try:
        for name in ("cfg3", "cfg4"):
            sg = data["s"][name]["paired"]["production_minus_per_electron"]["ramp"]["sigma_ppm"]
            d["channel_sigma_" + name] = sum(sg) / len(sg)
    except (TypeError, KeyError):
        pass
    return d


def derive_fits(round_name, d):
    """`k_lane: t0 = 27.8 us per launch, 145.6 us per 1e9 electrons` lines of scripts/thrower_vs_electrons.py."""
    p = os.path.join(ROOT, "profiles", round_name, "thrower_vs_electrons.txt")
    if os.path.exists(p):
        for m in re.finditer(r"^(k_\w+): t0 = ([0-9.+-]+) us per launch, ([0-9.+-]+) us per 1e9 electrons", open(p).read(), re.M):
            d[m.group(1)[2:] + "_t0_us"] = float(m.group(2))
            d[m.group(1)[2:] + "_us_per_1e9"] = float(m.group(3))
    return d


def lookup(data, key, path):
    node = data[key]
    if node is None:
        raise KeyError("profiles file for '%s' (%s) is missing" % (key, FILES[key]))
    for part in path.strip(".").split("."):
        if isinstance(node, list):
            node = node[int(part)]
        else:
            node = node[part]
    return node


def render(round_name):
    data = load(round_name)
    text = open(TEMPLATE).read()

    def fill(m):
        key, path, factor, fmt = m.groups()
        v = lookup(data, key, path)
        if factor:
            v = v * float(factor)
        return format(v, fmt) if fmt else str(v)
    body = PLACEHOLDER.sub(fill, text.replace("{{round}}", round_name))
    head = ("<!-- GENERATED by scripts/make_design.py from scripts/design_template.md and profiles/%s/*.json -- edit the "
            "template, not this file -->\n" % round_name)
    return head + body


def main():
    rnd = "r06"
    if "--round" in sys.argv:
        rnd = sys.argv[sys.argv.index("--round") + 1]
    text = render(rnd)
    if "--check" in sys.argv:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("DESIGN.md is %s" % ("up to date" if same else "STALE: run scripts/make_design.py"))
        return 0 if same else 1
    open(OUT, "w").write(text)
    print("wrote %s (%d lines)" % (OUT, text.count("\n")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
