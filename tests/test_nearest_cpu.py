"""CPU tests of the nearest-source feature above the kernel: the two entry
points' bindings and the argument errors they find before any HIP call, the
contact layer (skellysim_amd/contact.py) and SystemFD's use of it over a
stand-in backend whose `nearest` is the numpy brute force of
tests/nearest_reference.py, and the config key that switches it on."""

import ctypes
import os
import threading

import numpy as np
import pytest

import nearest_reference as NR
from skellysim_amd import _native, contact
from skellysim_amd.fiber_fd import FiberFD
from skellysim_amd.system_fd import Shell, SystemFD

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY_POINTS = ["skelly_nearest_host", "skelly_nearest_device"]
SHELLS = ["sphere_6000_nodes", "oocyte_nodes", "periphery_sphere_192", "ellipsoid_8192_nodes"]
DELTAS = [0.01, 0.05, 0.1]


def shell(name):
    fx = np.load(os.path.join(HERE, "golden", name + ".npz"))
    return np.ascontiguousarray(fx["nodes"]), np.ascontiguousarray(fx["normals"])


@pytest.fixture(scope="module")
def backend():
    return NR.NumpyNearestBackend()


# ---- the bindings and the C boundary ------------------------------------------------

def test_native_declares_the_nearest_entry_points():
    N = _native.NearestCount
    assert issubclass(N, ctypes.c_longlong) and ctypes.sizeof(N) == 8
    assert N is not _native.PressureCount and N is not _native.TraceCount
    for name in ENTRY_POINTS:
        assert name in _native.SIGNATURES
        argtypes = _native.SIGNATURES[name][1]
        assert argtypes.count(N) == 2
        assert not any(t is ctypes.c_longlong for t in argtypes)
    assert len(_native.SIGNATURES["skelly_nearest_host"][1]) == 8
    assert len(_native.SIGNATURES["skelly_nearest_device"][1]) == 9
    assert sorted(ENTRY_POINTS) == sorted(
        n for n, (_, argtypes) in _native.SIGNATURES.items() if N in argtypes)


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    so = ctypes.CDLL(hip_lib_path)
    _native._bind(so)
    return so


def _call(lib, name, counts, src_group=None, trg_group=None):
    """(rc, message) of one call on a thread of its own (the message is per
    thread): null pointers but for the two group arguments, which are never
    read before the checks under test."""
    args = [None, src_group, counts[0], None, trg_group, counts[1], None, None]
    args += [None] * (len(_native.SIGNATURES[name][1]) - len(args))
    got = []

    def run():
        got.append(getattr(lib, name)(*args))
        got.append(lib.skelly_hip_last_error().decode())
    th = threading.Thread(target=run)
    th.start()
    th.join()
    return got


@pytest.mark.parametrize("counts", [(-1, 5), (5, -1), (-(1 << 40), 5)],
                         ids=["n_src", "n_trg", "far_negative_n_src"])
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_negative_count_is_an_error_before_any_launch(lib, name, counts):
    rc, msg = _call(lib, name, counts)
    assert rc != 0
    assert msg == name + ": negative size", msg


@pytest.mark.parametrize("which", ["src_group", "trg_group"])
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_one_group_without_the_other_is_an_error_before_any_launch(lib, name, which):
    ids = np.zeros(5, dtype=np.int64)
    rc, msg = _call(lib, name, (5, 5), **{which: ids.ctypes.data_as(ctypes.c_void_p)})
    assert rc != 0
    assert msg.startswith(name + ":") and "group" in msg, msg


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_zero_targets_is_no_error_and_touches_nothing(lib, name):
    rc, msg = _call(lib, name, (5, 0))
    assert rc == 0 and msg == ""


def test_python_forms_take_both_groups_or_neither():
    from skellysim_amd import evaluator as ev
    r = np.zeros((4, 3))
    with pytest.raises(ValueError, match="both or neither"):
        ev.nearest(r, r, src_group=np.zeros(4, dtype=np.int64))
    with pytest.raises(TypeError, match="integer"):
        ev.nearest(r, r, np.zeros(4), np.zeros(4))
    with pytest.raises(ValueError, match="rows"):
        ev.nearest(r, r, np.zeros(3, dtype=np.int64), np.zeros(4, dtype=np.int64))
    with pytest.raises(TypeError, match="CUDA"):
        import torch
        ev.nearest_device(torch.zeros((4, 3), dtype=torch.float64),
                          torch.zeros((4, 3), dtype=torch.float64))
    assert ev.Evaluator.nearest is ev.nearest


# ---- the reference itself --------------------------------------------------------

def test_reference_rules():
    src = np.array([[0., 0, 0], [2, 0, 0], [0, 0, 0], [np.nan, 0, 0]])
    trg = np.array([[1., 0, 0], [0, 0, 0], [np.nan, 0, 0]])
    d2, k = NR.nearest(src, trg)
    assert d2.tolist()[:2] == [1.0, 0.0] and k.tolist() == [0, 0, -1] and d2[2] == np.inf
    g = np.array([0, 1, 0, 1])
    d2, k = NR.nearest(src, trg, g, np.array([0, 0, 1]))
    assert k.tolist() == [1, 1, -1] and d2.tolist()[:2] == [1.0, 4.0]
    d2, k = NR.nearest(src[:0], trg)
    assert np.all(d2 == np.inf) and np.all(k == -1)


# ---- contact.py over the stand-in backend --------------------------------------------

@pytest.mark.parametrize("name", SHELLS)
def test_points_off_a_node_along_its_normal(backend, name):
    """x_k + delta n_k has nearest node k and gap delta; x_k - delta n_k
    collides."""
    nodes, normals = shell(name)
    own = np.arange(len(nodes))
    for delta in DELTAS:
        gap, k = contact.shell_gap(nodes + delta * normals, nodes, normals, backend)
        assert np.array_equal(k, own), f"{name} delta={delta}: {np.count_nonzero(k != own)} misses"
        err = np.abs(gap - delta).max()
        print(f"{name} delta={delta}: max |gap - delta| = {err:.2e}")
        assert err <= 1e-14
        gap_out, _ = contact.shell_gap(nodes - delta * normals, nodes, normals, backend)
        assert np.all(gap_out <= 0.0)
        assert contact.generic_points_collide((nodes - delta * normals)[:64], nodes, normals, 0.0,
                                              backend)


@pytest.fixture(scope="module")
def sphere_cloud(backend):
    """Random interior points of sphere_6000_nodes with their gap and node."""
    nodes, normals = shell("sphere_6000_nodes")
    R = float(np.load(os.path.join(HERE, "golden", "sphere_6000_nodes.npz"))["radius"])
    rng = np.random.default_rng(17)
    u = rng.normal(size=(2000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pts = u * rng.uniform(0.5 * R, 0.999 * R, (2000, 1))
    gap, k = contact.shell_gap(pts, nodes, normals, backend)
    return nodes, normals, R, pts, gap, k


def test_sphere_identity_and_one_sidedness(sphere_cloud):
    """gap = R - r cos(theta_k) with theta_k the angle to the nearest node:
    never below the true R - r."""
    nodes, normals, R, pts, gap, k = sphere_cloud
    r = np.linalg.norm(pts, axis=1)
    cos = np.einsum("ij,ij->i", pts, nodes[k]) / (r * np.linalg.norm(nodes[k], axis=1))
    err = np.abs(gap - (R - r * cos)).max()
    excess = gap - (R - r)
    print(f"identity {err:.2e}, excess of the gap {excess.min():.2e} .. {excess.max():.2e}")
    assert err <= 1e-13
    assert excess.min() >= -1e-13
    assert np.all(excess <= r * (1.0 - cos) + 1e-13)


def test_force_is_the_sphere_law_on_radial_lines_through_nodes(backend):
    nodes, normals = shell("sphere_6000_nodes")
    R = float(np.load(os.path.join(HERE, "golden", "sphere_6000_nodes.npz"))["radius"])
    ks = np.arange(0, 6000, 375)[:16]
    depth = np.linspace(0.01, 0.4, 16)
    pts = nodes[ks] * (1.0 - depth / R)[:, None]
    f = contact.generic_periphery_force(pts, nodes, normals, 20.0, 0.05, backend)
    fib = FiberFD(pts, length=1.0, bending_rigidity=2.5e-3, eta=1.0)
    want = fib.periphery_repulsion(kind="sphere", f_0=20.0, l_0=0.05, radius=R).T
    assert np.linalg.norm(want, axis=1).min() > 0
    err = np.abs(f - want).max() / np.abs(want).max()
    print(f"force against the sphere law: {err:.2e}")
    assert np.abs(f - want).max() <= 1e-12 * np.abs(want).max()


def test_collided_points_get_no_force_and_threshold_transition(backend):
    nodes, normals = shell("periphery_sphere_192")
    delta = np.array([-0.05, 0.0, 0.05])
    pts = nodes[[3, 50, 120]] + delta[:, None] * normals[[3, 50, 120]]
    gap, k = contact.shell_gap(pts, nodes, normals, backend)
    assert k.tolist() == [3, 50, 120]
    f = contact.generic_periphery_force(pts, nodes, normals, 20.0, 0.05, backend)
    assert np.all(f[gap <= 0] == 0.0) and np.all(np.linalg.norm(f[gap > 0], axis=1) > 0)
    inside = pts[2:]  # gap 0.05
    g = float(gap[2])
    assert not contact.generic_points_collide(inside, nodes, normals, 0.0, backend)
    assert not contact.generic_points_collide(inside, nodes, normals, np.nextafter(g, 0), backend)
    assert contact.generic_points_collide(inside, nodes, normals, g, backend)
    assert contact.generic_points_collide(inside, nodes, normals, 0.06, backend)


def test_min_group_gap_is_the_brute_force_pair_search(backend):
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1, 1, (8 * 16, 3))
    group = np.repeat(np.arange(8), 16)
    d, i, j = contact.min_group_gap(pts, group, backend)
    m = np.sqrt(NR.distances(pts, pts))
    m[group[:, None] == group[None, :]] = np.inf
    bi, bj = np.unravel_index(np.argmin(m), m.shape)
    assert (i, j) == (min(bi, bj), max(bi, bj)) and d == m[bi, bj]
    assert group[i] != group[j]
    assert contact.min_group_gap(pts, np.zeros(len(pts), dtype=np.int64), backend) == \
        (np.inf, -1, -1)


# ---- SystemFD over the stand-in backend --------------------------------------------

def shell_fibers(nodes, normals, delta, n_fibers=4, n=16, clamp_first=False):
    """Fibers whose node j lies at x_k + delta n_k, k = 16 i + j."""
    fibers = []
    for i in range(n_fibers):
        k = np.arange(n * i, n * (i + 1))
        fibers.append(FiberFD(nodes[k] + delta * normals[k], length=1.0, bending_rigidity=2.5e-3,
                              eta=1.0, minus_clamped=clamp_first and i == 0))
    return fibers


def test_system_collision_and_fiber_gap(backend):
    nodes, normals = shell("oocyte_nodes")
    sh = Shell(nodes, normals, None, None)
    generic = dict(kind="generic")  # the system's own shell
    s = SystemFD(shell_fibers(nodes, normals, 0.05), eta=1.0, dt=0.01, shell=sh, backend=backend)
    calls = backend.calls
    assert not s.check_collision(generic)
    assert backend.calls == calls + 1, "one launch over all fiber nodes"
    assert s.check_collision(generic, threshold=0.06)
    s.fibers[0].x[:, 0] = nodes[0] - 0.05 * normals[0]
    assert s.check_collision(generic)
    assert s.check_collision(dict(kind="generic", nodes=nodes, normals=normals))
    s.fibers[0].minus_clamped = True
    assert not s.check_collision(generic)

    d, a, b = s.min_fiber_gap()
    pts = s.fiber_nodes()
    fid = np.repeat(np.arange(4), 16)
    m = np.sqrt(NR.distances(pts, pts))
    m[fid[:, None] == fid[None, :]] = np.inf
    bi, bj = np.unravel_index(np.argmin(m), m.shape)
    assert d == m[bi, bj] and {a, b} == {(bi // 16, bi % 16), (bj // 16, bj % 16)}
    with pytest.raises(ValueError, match="generic"):
        SystemFD(s.fibers, eta=1.0, dt=0.01, backend=backend).check_collision(generic)


def test_system_body_against_a_generic_shell(backend):
    """A spherical body collides when gap(centre) - R_body <= threshold."""
    from types import SimpleNamespace
    nodes, normals = shell("periphery_sphere_192")
    centre = nodes[7] + 0.5 * normals[7]

    class Ball(SimpleNamespace):
        def check_collision(self, other, threshold):
            return False
    s = SystemFD([], eta=1.0, dt=0.01, backend=backend,
                 bodies=[Ball(position=centre, radius=0.4)])
    generic = dict(kind="generic", nodes=nodes, normals=normals)
    gap, _ = contact.shell_gap(centre[None], nodes, normals, backend)
    assert not s.check_collision(generic)
    assert s.check_collision(generic, threshold=float(gap[0]) - 0.4)
    s.bodies[0].radius = 0.6
    assert s.check_collision(generic)


# ---- the config key -------------------------------------------------------------------

def test_config_key_switches_generic_contact_on():
    from skellysim_amd.config import periphery_interaction_from, periphery_shape_from
    cfg = {"params": {"periphery_interaction_flag": True,
                      "fiber_periphery_interaction": {"f_0": 7.0, "l_0": 0.1}},
           "periphery": {"shape": "surface_of_revolution"}}
    assert periphery_shape_from(cfg) is None and periphery_interaction_from(cfg) is None
    cfg["params"]["generic_periphery_contact"] = True
    assert periphery_shape_from(cfg) == dict(kind="generic")
    assert periphery_interaction_from(cfg) == dict(kind="generic", f_0=7.0, l_0=0.1)
    cfg["params"]["periphery_interaction_flag"] = False
    assert periphery_interaction_from(cfg) is None
    # sphere and ellipsoid are not touched by the key
    cfg["periphery"] = {"shape": "sphere", "radius": 3.0}
    assert periphery_shape_from(cfg) == dict(kind="sphere", radius=3.0)
    del cfg["periphery"]
    assert periphery_shape_from(cfg) is None
