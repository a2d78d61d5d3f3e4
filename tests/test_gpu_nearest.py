"""GPU tests of the nearest-source kernel (the Nearest functor through
pair_driver) and of what stands on it: skelly_nearest_device / _host, their
Python and C++ mirrors, and SystemFD's generic-periphery contact.

Reference: the numpy brute force of tests/nearest_reference.py. On
integer-lattice coordinates every d2 is exact, so d2 must be bit-equal and the
index equal, ties included (lowest index). On random fp64 inputs both sides sum
three non-negative products, each within 2u of the exact value (u = 2^-53;
the kernel's chain is fma-contracted, the reference's is not), so d2 agrees
to 4u relative, and the index may differ only between sources whose reference
d2 lie within 8u of the minimum.

Shapes: n_trg 1, 255, 257, 1027 cover 1, 2 and 4 targets a thread, each with a
remainder; n_src 1, 2, 3, 5, 129, 4099 cover the group remainders 0, 1 and
GROUP - 1 and the 2 GROUP loop boundary (GROUP = 2)."""

import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import nearest_reference as NR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
U = 2.0 ** -53
N_TRG = [1, 255, 257, 1027]
N_SRC = [1, 2, 3, 5, 129, 4099]
SLICES = [0, 1, 2, 3, 7]  # 0: the planner's choice


@pytest.fixture(scope="module")
def ska(hip_lib_path):
    import skellysim_amd
    return skellysim_amd


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def run(ska, src, trg, sg=None, tg=None, slices=0):
    """(d2, index) as numpy arrays of one device call with the slice knob at
    `slices`, the knob back at 0 afterwards."""
    import torch
    from skellysim_amd import _native
    groups = [None if g is None else _t(np.asarray(g, dtype=np.int64)) for g in (sg, tg)]
    try:
        _native.set_pair_slices(slices)
        d2, idx = ska.nearest_device(_t(src), _t(trg), *groups)
        torch.cuda.synchronize()
    finally:
        _native.set_pair_slices(0)
    return d2.cpu().numpy(), idx.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def lattice(n_src, n_trg, half):
    rng = np.random.default_rng(1000 * n_src + n_trg + half)
    src = rng.integers(-half, half + 1, (n_src, 3)).astype(float)
    trg = rng.integers(-half, half + 1, (n_trg, 3)).astype(float)
    return src, trg, NR.nearest(src, trg)


@functools.lru_cache(maxsize=None)
def cloud(n_src, n_trg):
    rng = np.random.default_rng(7000 * n_src + n_trg)
    src, trg = rng.uniform(-1, 1, (n_src, 3)), rng.uniform(-1, 1, (n_trg, 3))
    return src, trg, NR.nearest(src, trg)


def all_slices(ska, src, trg, sg=None, tg=None, slices=SLICES):
    """One result for every slice count, after checking that they are
    bit-identical to each other and to a second run."""
    first = run(ska, src, trg, sg, tg, slices[0])
    again = run(ska, src, trg, sg, tg, slices[0])
    assert same_bits(first[0], again[0]) and np.array_equal(first[1], again[1]), "two runs differ"
    for s in slices[1:]:
        d2, idx = run(ska, src, trg, sg, tg, s)
        assert same_bits(d2, first[0]), f"d2 differs at {s} slices"
        assert np.array_equal(idx, first[1]), f"index differs at {s} slices"
    return first


def check_random(src, trg, got, want):
    d2, idx = got
    d2_ref, idx_ref = want
    assert np.all(np.abs(d2 - d2_ref) <= 4 * U * d2_ref), \
        f"d2 off by {np.max(np.abs(d2 - d2_ref) / d2_ref) / U:.1f} u"
    other = idx != idx_ref
    assert np.all(idx[other] >= 0)
    d = trg[other] - src[idx[other]]
    d2_of_got = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    assert np.all(d2_of_got <= d2_ref[other] * (1 + 8 * U)), "an index that is no near-tie"


@pytest.mark.parametrize("n_src", N_SRC)
@pytest.mark.parametrize("n_trg", N_TRG)
def test_shapes(ska, n_trg, n_src):
    # exact arithmetic: a wide lattice and a tight one (ties, coincident points)
    for half in (64, 3):
        src, trg, (d2_ref, idx_ref) = lattice(n_src, n_trg, half)
        d2, idx = all_slices(ska, src, trg)
        assert same_bits(d2, d2_ref), f"lattice {half}: d2"
        assert np.array_equal(idx, idx_ref), \
            f"lattice {half}: {np.count_nonzero(idx != idx_ref)} indices differ"
        # every source twice: the first copy wins, whatever the slicing
        d2, idx = all_slices(ska, np.concatenate([src, src]), trg)
        assert same_bits(d2, d2_ref) and np.array_equal(idx, idx_ref), f"lattice {half}: doubled"
        assert np.all(idx < n_src)
    src, trg, want = cloud(n_src, n_trg)
    check_random(src, trg, all_slices(ska, src, trg), want)


@pytest.mark.parametrize("n_trg", N_TRG)
def test_empty_last_slice(ska, n_trg):
    """5 sources in 4 slices of 2: the fourth is empty and writes the neutral
    element."""
    for half in (64, 3):
        src, trg, (d2_ref, idx_ref) = lattice(5, n_trg, half)
        d2, idx = run(ska, src, trg, slices=4)
        assert same_bits(d2, d2_ref) and np.array_equal(idx, idx_ref)


def test_groups(ska):
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1, 1, (8 * 16, 3))
    group = np.repeat(np.arange(8), 16)
    want = NR.nearest(pts, pts, group, group)
    d2, idx = all_slices(ska, pts, pts, group, group, slices=[0, 1, 2, 3, 7])
    assert np.all(idx != np.arange(len(pts))) and np.all(group[idx] != group)
    check_random(pts, pts, (d2, idx), want)
    assert np.array_equal(idx, want[1])
    # exact coordinates: equal to the reference bit for bit, ties included
    lat = rng.integers(-3, 4, (8 * 16, 3)).astype(float)
    d2, idx = all_slices(ska, lat, lat, group, group)
    want = NR.nearest(lat, lat, group, group)
    assert same_bits(d2, want[0]) and np.array_equal(idx, want[1])
    # one group: nothing is eligible
    one = np.zeros(len(pts), dtype=np.int64)
    d2, idx = all_slices(ska, pts, pts, one, one)
    assert np.all(d2 == np.inf) and np.all(idx == -1)
    # coincident points of different groups are a hit at distance zero
    twice = np.concatenate([pts, pts])
    g2 = np.concatenate([one, one + 1])
    d2, idx = all_slices(ska, twice, twice, g2, g2)
    assert np.all(d2 == 0.0)
    assert np.array_equal(idx, (np.arange(len(twice)) + len(pts)) % len(twice))
    # ungrouped, a point is its own nearest source
    d2, idx = run(ska, pts, pts)
    assert np.all(d2 == 0.0) and np.array_equal(idx, np.arange(len(pts)))


@pytest.mark.parametrize("n_trg", [1, 257])
def test_no_sources(ska, n_trg):
    _, trg, _ = cloud(5, n_trg)
    for slices in (0, 3):
        d2, idx = run(ska, np.zeros((0, 3)), trg, slices=slices)
        assert d2.shape == (n_trg,) and np.all(d2 == np.inf) and np.all(idx == -1)


def test_nan_sources_and_targets(ska):
    src, trg, _ = cloud(129, 257)
    src, trg = src.copy(), trg.copy()
    _, nearest_clean = NR.nearest(src, trg)
    bad = np.unique(nearest_clean)[:20]  # sources that were somebody's nearest
    src[bad, np.arange(len(bad)) % 3] = np.nan
    trg[[0, 100, 256], [0, 1, 2]] = np.nan
    want = NR.nearest(src, trg)
    d2, idx = all_slices(ska, src, trg)
    assert not np.isin(idx, bad).any()
    for t in (0, 100, 256):
        assert d2[t] == np.inf and idx[t] == -1
    keep = np.ones(len(trg), dtype=bool)
    keep[[0, 100, 256]] = False
    check_random(src, trg[keep], (d2[keep], idx[keep]), (want[0][keep], want[1][keep]))
    d2, idx = run(ska, np.full((3, 3), np.nan), trg)
    assert np.all(d2 == np.inf) and np.all(idx == -1)


def block_bytes(stream):
    from skellysim_amd import _native
    n = ctypes.c_longlong(-1)
    assert _native.lib().skelly_persistent_ws_bytes(ctypes.c_void_p(stream.cuda_stream),
                                                    ctypes.byref(n)) == 0
    return n.value


def test_side_stream_and_workspace_does_not_grow(ska):
    import torch
    src, trg, want = lattice(4099, 1027, 64)
    rng = np.random.default_rng(9)
    sg, tg = rng.integers(0, 5, len(src)), rng.integers(0, 5, len(trg))
    want_g = NR.nearest(src, trg, sg, tg)
    d = [_t(a) for a in (src, trg, sg, tg)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d2, idx = ska.nearest_device(d[0], d[1])
        d2_g, idx_g = ska.nearest_device(*d)
    s.synchronize()
    assert same_bits(d2.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])
    assert same_bits(d2_g.cpu().numpy(), want_g[0])
    assert np.array_equal(idx_g.cpu().numpy(), want_g[1])
    before = block_bytes(s)
    assert before > 0, "the device form did not use the stream's persistent workspace"
    with torch.cuda.stream(s):
        for _ in range(3):
            d2, idx = ska.nearest_device(d[0], d[1])
            d2_g, idx_g = ska.nearest_device(*d)
    s.synchronize()
    assert block_bytes(s) == before
    assert same_bits(d2.cpu().numpy(), want[0]) and np.array_equal(idx_g.cpu().numpy(), want_g[1])


@pytest.mark.parametrize("forced", [0, 3])
def test_captured_call_replays(ska, forced):
    """The graph holds the staging, the packing, the pair kernel, the reduce
    and the unpack: new values in the static inputs come out as the eager call
    has them, with the slice knob back at 0."""
    import torch
    from skellysim_amd import _native
    first, second = lattice(4099, 1027, 64), lattice(4099, 1027, 3)
    rng = np.random.default_rng(11)
    groups = [(rng.integers(0, 4, 4099), rng.integers(0, 4, 1027)) for _ in range(2)]
    want = [NR.nearest(c[0], c[1], *g) for c, g in zip((first, second), groups)]
    static = [_t(a) for a in (first[0], first[1], *groups[0])]
    fresh = [_t(a) for a in (second[0], second[1], *groups[1])]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        _native.set_pair_slices(forced)
        with torch.cuda.stream(s):
            ska.nearest_device(*static)  # warm-up: the workspace is allocated here
            ska.nearest_device(*static)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            d2, idx = ska.nearest_device(*static)
    finally:
        _native.set_pair_slices(0)

    def replay():
        with torch.cuda.stream(s):
            d2.fill_(float("nan"))
            idx.fill_(-7)
            g.replay()
        torch.cuda.synchronize()
        return d2.cpu().numpy(), idx.cpu().numpy()

    got = replay()
    assert same_bits(got[0], want[0][0]) and np.array_equal(got[1], want[0][1])
    for a, b in zip(static, fresh):
        a.copy_(b)
    torch.cuda.synchronize()
    for _ in range(2):
        got = replay()
        assert same_bits(got[0], want[1][0]) and np.array_equal(got[1], want[1][1])


@pytest.mark.parametrize("grouped", [False, True])
def test_host_form_is_the_device_form(ska, grouped):
    src, trg, _ = cloud(4099, 1027)
    rng = np.random.default_rng(13)
    sg, tg = (rng.integers(0, 6, 4099), rng.integers(0, 6, 1027)) if grouped else (None, None)
    d2, idx = ska.nearest(src, trg, sg, tg)
    assert d2.dtype == np.float64 and idx.dtype == np.int64
    want = run(ska, src, trg, sg, tg)
    assert same_bits(d2, want[0]) and np.array_equal(idx, want[1])
    d2, idx = ska.Evaluator.nearest(src.T, trg.T, sg, tg)  # (3, n) is accepted
    assert same_bits(d2, want[0]) and np.array_equal(idx, want[1])
    d2, idx = ska.nearest(src, np.zeros((0, 3)), sg, None if sg is None else tg[:0])
    assert d2.shape == (0,) and idx.shape == (0,)


@pytest.mark.parametrize("grouped", [False, True])
def test_cpp_mirror_is_the_python_host_form(ska, tmp_path, grouped):
    from test_gpu_cpp_mirror import INCLUDE, LIBDIR
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe, case, out = (str(tmp_path / n) for n in ("nearest_probe", "case.bin", "out.bin"))
    built = subprocess.run(
        [cxx, "-O2", "-std=c++17", "-I", INCLUDE, os.path.join(REPO, "tests", "nearest_probe.cpp"),
         "-L", LIBDIR, "-lskellyhip", "-Wl,-rpath," + LIBDIR, "-o", exe],
        capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    src, trg, _ = cloud(129, 257)
    rng = np.random.default_rng(15)
    sg, tg = (rng.integers(0, 6, 129), rng.integers(0, 6, 257)) if grouped else (None, None)
    with open(case, "wb") as f:
        np.array([len(src), len(trg), int(grouped)], dtype=np.int64).tofile(f)
        src.tofile(f)
        trg.tofile(f)
        if grouped:
            sg.astype(np.int64).tofile(f)
            tg.astype(np.int64).tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"nearest_probe failed ({r.returncode}): {r.stdout} {r.stderr}"
    raw = np.fromfile(out, np.int64)
    assert raw.size == 2 * len(trg)
    d2, idx = raw[:len(trg)].view(np.float64), raw[len(trg):]
    want = ska.nearest(src, trg, sg, tg)
    assert same_bits(d2, want[0]) and np.array_equal(idx, want[1])


# ---- SystemFD on the oocyte shell -------------------------------------------------

def _system(nodes, normals, delta, interaction, clamp_first=False):
    from skellysim_amd.fiber_fd import FiberFD
    from skellysim_amd.system_fd import HipBackend, SystemFD
    fibers = []
    for i in range(4):
        k = np.arange(16 * i, 16 * (i + 1))
        fibers.append(FiberFD(nodes[k] + delta * normals[k], length=1.0, bending_rigidity=2.5e-3,
                              eta=1.0, minus_clamped=clamp_first and i == 0))
    return SystemFD(fibers, eta=1.0, dt=0.01, backend=HipBackend(),
                    periphery_interaction=interaction)


def test_system_on_the_oocyte_shell(ska):
    from skellysim_amd import contact
    fx = np.load(os.path.join(HERE, "golden", "oocyte_nodes.npz"))
    nodes, normals = np.ascontiguousarray(fx["nodes"]), np.ascontiguousarray(fx["normals"])
    generic = dict(kind="generic", nodes=nodes, normals=normals)
    law = dict(f_0=20.0, l_0=0.05)
    delta = 0.05
    s = _system(nodes, normals, delta, dict(generic, **law))
    assert not s.check_collision(generic)
    s.fibers[0].x[:, 0] = nodes[0] - 0.05 * normals[0]
    assert s.check_collision(generic)
    s.fibers[0].minus_clamped = True
    assert not s.check_collision(generic)
    s.fibers[0].minus_clamped = False
    s.fibers[0].x[:, 0] = nodes[0] + delta * normals[0]

    # min_fiber_gap against the brute force
    d, a, b = s.min_fiber_gap()
    pts = s.fiber_nodes()
    fid = np.repeat(np.arange(4), 16)
    m = np.sqrt(NR.distances(pts, pts))
    m[fid[:, None] == fid[None, :]] = np.inf
    bi, bj = np.unravel_index(np.argmin(m), m.shape)
    assert {a, b} == {(bi // 16, bi % 16), (bj // 16, bj % 16)}
    assert abs(d - m[bi, bj]) <= 4 * U * m[bi, bj]

    # the force of prep() against contact.py over the numpy reference
    clamped = _system(nodes, normals, delta, dict(generic, **law), clamp_first=True)
    rhs = clamped.prep_state_for_solver()
    want = contact.generic_periphery_force(pts, nodes, normals, law["f_0"], law["l_0"],
                                           NR.NumpyNearestBackend())
    assert np.linalg.norm(want, axis=1).min() > 0
    want[0] = 0.0  # node 0 of the minus-clamped fiber
    err = np.abs(clamped.periphery_force - want).max() / np.abs(want).max()
    print(f"prep() periphery force against the numpy reference: {err:.2e}")
    assert err <= 1e-13
    assert np.all(clamped.periphery_force[0] == 0.0)
    plain = _system(nodes, normals, delta, None, clamp_first=True)
    rhs_plain = plain.prep_state_for_solver()
    assert rhs.shape == rhs_plain.shape and np.all(np.isfinite(rhs))
    assert np.abs(rhs - rhs_plain).max() > 1e-6 * np.abs(rhs_plain).max()
