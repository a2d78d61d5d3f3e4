"""The pair kernels' launch planner (skellysim_amd/csrc/pair_plan.hpp) on the
host: a small stand-alone C++ program (tests/pair_plan_probe.cpp) is built
against the header with the host compiler, with AddressSanitizer and UBSan
where the compiler has them, and prints plans for a table of shapes.

Device constants used throughout are the MI355X's: 256 CUs, 3 workgroups a CU
(2 for the stresslet), fast path from 8192 sources a slice."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "skellysim_amd", "csrc")
PROBE = os.path.join(REPO, "tests", "pair_plan_probe.cpp")

N_CU, WG_PER_CU = 256, 3
FAST_MIN_SRC = 8192
MIN_SRC = 2048            # PAIR_PLAN_MIN_SRC
WS_CAP = 144 << 20        # PAIR_PLAN_WS_CAP


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pair_plan") / "pair_plan_probe")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, PROBE,
            "-o", exe]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # sanitizer runtime linked statically (gcc and clang spell the flag
    # differently), so the program starts whatever else the loader brings in
    for extra in (san + ["-static-libasan"], san + ["-static-libsan"], []):
        built = subprocess.run(base + extra, capture_output=True, text=True)
        if built.returncode == 0 and subprocess.run(
                [exe], input="", capture_output=True, text=True, env=env).returncode == 0:
            break
    else:
        pytest.fail("could not build the probe: " + built.stderr)

    def run(shapes):
        """shapes: dicts with n_src, n_trg and optional max_tpt, outdim,
        fast_mode, n_cu, wg_per_cu, forced. Returns one dict per shape."""
        lines = []
        for s in shapes:
            lines.append("%d %d %d %d %d %d %d %d %d" % (
                s["n_src"], s["n_trg"], s.get("max_tpt", 4), s.get("outdim", 3),
                s.get("fast_mode", 1), FAST_MIN_SRC, s.get("n_cu", N_CU),
                s.get("wg_per_cu", WG_PER_CU), s.get("forced", 0)))
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True,
                           text=True, timeout=60, env=env)
        assert r.returncode == 0, r.stderr
        out, cur = [], None
        for line in r.stdout.splitlines():
            w = line.split()
            if w[0] == "plan":
                cur = dict(tpt=int(w[1]), n_slices=int(w[2]), fast=int(w[3]), s_max=int(w[4]),
                           blocks=int(w[5]), time=float(w[6]), cand={})
            elif w[0] == "cand":
                cur["cand"][int(w[1])] = float(w[2])
            else:
                out.append(cur)
        assert len(out) == len(shapes)
        return out

    return run


def ceil_div(a, b):
    return -(-a // b)


def efficiency(plan, n_cu=N_CU):
    w = plan["blocks"] * plan["n_slices"]
    return (w / n_cu) / ceil_div(w, n_cu)


def test_constraints_on_a_grid_of_shapes(probe):
    """Slice-length floor, workspace cap and n_slices >= 1, velocity (3
    outputs, up to 4 targets a thread) and gradient (9, up to 2) kernels."""
    n_srcs = [1, 2047, 2048, 2049, 4096, 4097, 6000, 100_000, 1_000_000, 5_000_000]
    n_trgs = [1, 255, 256, 1023, 1024, 1025, 20_000, 125_000, 1_000_000, 4_000_000]
    shapes = [dict(n_src=s, n_trg=t, outdim=od, max_tpt=mt, wg_per_cu=wg, n_cu=cu)
              for s in n_srcs for t in n_trgs for od, mt, wg in ((3, 4, 3), (3, 4, 2), (9, 2, 3))
              for cu in (256, 304)]
    for s, p in zip(shapes, probe(shapes)):
        assert p["n_slices"] >= 1, s
        assert p["n_slices"] <= max(1, ceil_div(s["n_src"], MIN_SRC)), (s, p)
        if p["n_slices"] > 1:
            assert p["n_slices"] * s["outdim"] * s["n_trg"] * 8 <= WS_CAP, (s, p)
        assert p["tpt"] in (1, 2, 4) and p["tpt"] <= s["max_tpt"]
        assert p["blocks"] == ceil_div(s["n_trg"], 256 * p["tpt"])
        src_per_slice = ceil_div(s["n_src"], p["n_slices"])
        assert p["fast"] == int(src_per_slice >= FAST_MIN_SRC), (s, p)


def test_small_shapes_keep_their_slice_counts(probe):
    """The shapes the GPU tests rely on: 3000 sources give 2 slices for 1501
    targets and for its four shards alike; 6000 and 4099 sources give 3."""
    shapes = [dict(n_src=3000, n_trg=t) for t in (1501, 375, 376)]
    shapes += [dict(n_src=6000, n_trg=1500), dict(n_src=4099, n_trg=5)]
    shapes += [dict(n_src=2000, n_trg=1000), dict(n_src=20000, n_trg=20000),
               dict(n_src=5000, n_trg=5000)]
    got = [p["n_slices"] for p in probe(shapes)]
    assert got == [2, 2, 2, 3, 3, 1, 10, 3]
    # and for every kernel family (stresslet occupancy, gradient outputs)
    for kw in (dict(wg_per_cu=2), dict(outdim=9, max_tpt=2)):
        got = [p["n_slices"] for p in probe([dict(s, **kw) for s in shapes[:5]])]
        assert got == [2, 2, 2, 3, 3]


def test_underfilled_launches_keep_slicing(probe):
    """Where the old rule (at least 1024 workgroups, 2048 sources a slice)
    sliced a launch that underfills the chip (no more workgroups than CUs),
    the planner slices it as far as the floor allows."""
    shapes = [dict(n_src=s, n_trg=t) for s in (4096, 10_000, 50_000) for t in (1, 300, 1500, 5000)]
    for s, p in zip(shapes, probe(shapes)):
        if p["blocks"] * p["s_max"] <= N_CU:
            assert p["n_slices"] == p["s_max"], (s, p)


BIG = [dict(n_src=1_000_000, n_trg=1_000_000),
       dict(n_src=1_000_000, n_trg=125_000),
       dict(n_src=100_000, n_trg=100_000),
       dict(n_src=2_000_000, n_trg=2_000_000)]


def test_modelled_efficiency_of_the_big_shapes(probe):
    """(W/C)/ceil(W/C) >= 0.97 at the flagship, its 8-GPU target shard and
    2e6 x 2e6, each still on the fast path, and room for at least 6 slices
    at the flagship. 1e5 x 1e5 cannot reach 0.97 with the fast path on: its
    98 blocks give W/C = 0.3828 S, and S <= 12 (8192 sources a slice) tops
    out at 0.957 (S = 5 or 10); the first count above 0.97 is S = 13 (0.995),
    masked, which the model charges 7 %. The planner keeps the fast path
    there, so for that shape the modelled time against the best candidate is
    bounded instead (1.03), and the fast path is asserted."""
    plans = probe(BIG)
    for s, p in zip(BIG, plans):
        eff = efficiency(p)
        best = min(p["cand"].values())
        print(s, "slices", p["n_slices"], "fast", p["fast"], "efficiency %.4f" % eff,
              "time/best %.4f" % (p["time"] / best))
        assert p["fast"] == 1
        assert ceil_div(s["n_src"], p["n_slices"]) >= FAST_MIN_SRC
        assert p["time"] <= 1.03 * best
        if s["n_src"] != 100_000:
            assert eff >= 0.97, (s, p)
    assert plans[0]["s_max"] >= 6
    # the planner's choice is the smallest-time candidate, ties to the smaller S
    for p in plans:
        best = min(p["cand"].values())
        assert p["n_slices"] == min(S for S, t in p["cand"].items() if t == best)


def test_plan_is_a_pure_function(probe):
    """Same inputs, same plan, whatever was planned before; and the slice
    count does not follow the fast-path switch (only `fast` does)."""
    shapes = BIG + [dict(n_src=3000, n_trg=1501), dict(n_src=20000, n_trg=20000)]
    a = probe(shapes)
    b = probe(list(reversed(shapes)) + shapes)
    assert a == list(reversed(b[:len(shapes)])) == b[len(shapes):]
    for mode in (0, 2):
        c = probe([dict(s, fast_mode=mode) for s in shapes])
        assert [p["n_slices"] for p in c] == [p["n_slices"] for p in a]
        assert all(p["fast"] == (mode == 2) for p in c)


def test_forced_slice_count(probe):
    """The override gives exactly n slices, clamped only to the source count
    (and the grid limit), below the 2048-source floor too."""
    shapes = [dict(n_src=1303, n_trg=1100, forced=f) for f in (1, 2, 3, 7, 1303, 5000)]
    shapes += [dict(n_src=1_000_000, n_trg=1_000_000, forced=16),
               dict(n_src=1_000_000, n_trg=10, forced=100_000)]
    got = [p["n_slices"] for p in probe(shapes)]
    assert got == [1, 2, 3, 7, 1303, 1303, 16, 65535]
