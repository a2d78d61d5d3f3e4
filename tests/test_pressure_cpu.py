"""CPU tests of the pressure and stress layers above the kernels: the closed
forms themselves, flows' stress composition and surface integrals, the
listener's pressure_field / stress_field and its two request keys, the
sources' flow_pressure, and the argument checks of the evaluator's new host
forms. The compute backend is test_gradient_cpu's numpy backend plus the three
pressure methods, built from (d = t - s, y = 1/sqrt(den), prefactor 1/(4 pi),
r == 0 dropped, no eta)

  Stokeslet / regularized Oseen   p = sum (f.d) y^3      den as the velocity's
  Stresslet                       p = sum [ tr(S) y^3 - 3 C y^5 ],  C = d^T S d
  Rotlet                          p = 0

The reference project has no pressure on its direct path, so the yardsticks
are the longdouble restatement (tests/pressure_reference.py) and identities
that no formula error survives: the momentum balance eta d_j G_ij = d_i p and
the force and torque that a closed surface around the sources carries.

tests/test_gpu_pressure.py imports the backend and the sphere from here."""

import io
import struct

import msgpack
import numpy as np
import pytest

import pair_reference as R
import pressure_reference as PR
from test_gradient_cpu import (NumpyBackend, _chunked, _sl_terms, _dl_terms, _ndencode,
                               np_stokeslet_grad, np_stresslet_grad, np_rotlet_grad,
                               np_oseen_grad, central_difference, far_probes, rel,
                               bent_fiber_frame, shell_fixture, body_fixture, fiber_nodes,
                               SEED, FIELD_X)

ETA = 1.3
FOUR_PI = 4 * np.pi


def np_stokeslet_pressure(r_src, f, r_trg, reg=0.0, eps=0.0):
    r_src, f = np.asarray(r_src, float), np.asarray(f, float)

    def block(t):
        d, y, fd = _sl_terms(r_src, f, t, reg, eps)
        return (y ** 3 * fd).sum(axis=1)

    return _chunked(block, r_trg, ()) / FOUR_PI


def np_oseen_pressure(r_src, r_trg, rho, reg=5e-3, eps=1e-5):
    return np_stokeslet_pressure(r_src, rho, r_trg, reg, eps)


def np_stresslet_pressure(r_src, f9, r_trg):
    r_src, f9 = np.asarray(r_src, float), np.asarray(f9, float)
    tr = f9[:, 0] + f9[:, 4] + f9[:, 8]

    def block(t):
        d, y, C, _ = _dl_terms(r_src, f9, t)
        return (y ** 3 * tr[None, :] - 3.0 * y ** 5 * C).sum(axis=1)

    return _chunked(block, r_trg, ()) / FOUR_PI


class NumpyPressureBackend(NumpyBackend):
    """test_gradient_cpu.NumpyBackend plus the pressure methods of the
    system_fd.HipBackend contract."""

    def stokeslet_pressure(self, r_src, f_src, r_trg):
        return np_stokeslet_pressure(r_src, f_src, r_trg)

    def stresslet_normal_density_pressure(self, r_src, normals, density, r_trg, eta):
        f_dl = 2.0 * eta * np.einsum("ni,nj->nij", normals, density).reshape(-1, 9)
        return np_stresslet_pressure(r_src, f_dl, r_trg)

    def oseen_contract_pressure(self, r_src, r_trg, density):
        return np_oseen_pressure(r_src, r_trg, density)


class NoPressureBackend(NumpyBackend):
    """A backend whose pressure methods must not be reached."""

    def _refuse(self, *a, **kw):
        raise AssertionError("a pressure method was called")

    stokeslet_pressure = stresslet_normal_density_pressure = oseen_contract_pressure = _refuse


def cloud37(seed=3):
    """37 sources in [-1, 1]^3 with forces, stresslet tensors and torques."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (37, 3)), rng.uniform(-1, 1, (37, 3)),
            rng.uniform(-1, 1, (37, 9)), rng.uniform(-1, 1, (37, 3)))


def sphere_quadrature(radius=3.0, n_theta=32, n_phi=64):
    """(points, outward normals, weights) of the sphere about the origin:
    Gauss-Legendre in cos(theta) x the midpoint rule in phi."""
    mu, w = np.polynomial.legendre.leggauss(n_theta)
    phi = (np.arange(n_phi) + 0.5) * (2 * np.pi / n_phi)
    s = np.sqrt(1.0 - mu * mu)
    n = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)),
                  np.outer(mu, np.ones(n_phi))], axis=-1).reshape(-1, 3)
    weights = np.repeat(w, n_phi) * (2 * np.pi / n_phi) * radius ** 2
    return radius * n, n, weights


# ---- the closed forms -----------------------------------------------------

def test_numpy_forms_match_the_longdouble_references():
    """The fp64 forms above against pressure_reference, per target, to a few
    hundred roundings of the condition sum (37 sources, unordered sums)."""
    src, f3, f9, _ = cloud37()
    trg = np.concatenate([far_probes(src, 16, seed=7), src[:3], src[5:8] + 3e-6])
    for got, (ref, A) in (
            (np_stokeslet_pressure(src, f3, trg), PR.stokeslet_pressure(src, f3, trg)),
            (np_oseen_pressure(src, trg, f3), PR.oseen_contract_pressure(src, trg, f3)),
            (np_stresslet_pressure(src, f9, trg), PR.stresslet_pressure(src, f9, trg))):
        assert got.shape == (len(trg),) and np.isfinite(got).all()
        assert (np.abs(got.astype(PR.LD) - ref) <= 400 * PR.U * A).all()
        assert (A > 0).all()
    # the regularized branch is not the plain one at 3e-6 from a source
    plain, reg = np_stokeslet_pressure(src, f3, trg[-3:]), np_oseen_pressure(src, trg[-3:], f3)
    assert rel(plain, reg) > 1.0


def test_pressure_reference_condition_sums():
    """A is the reference with absolute values inside: A >= |ref|, equality
    for a single source, and A == 0 exactly on a lone coincident pair."""
    src, f3, f9, _ = cloud37()
    trg = far_probes(src, 8, seed=8)
    for ref, A in (PR.stokeslet_pressure(src, f3, trg), PR.stresslet_pressure(src, f9, trg),
                   PR.oseen_contract_pressure(src, trg, f3)):
        assert (A >= np.abs(ref)).all() and (A > 0).all()
    one, f = src[:1], np.array([[0.0, 0.0, 2.0]])
    t = one + np.array([[0.0, 0.0, 0.5]])
    ref, A = PR.stokeslet_pressure(one, f, t)
    # (f.d) y^3 = (2 * 0.5) * 8
    assert abs(float(ref[0]) - 8.0 / FOUR_PI) < 1e-15 and A[0] == ref[0]
    for ref, A in (PR.stokeslet_pressure(one, f, one), PR.stresslet_pressure(one, f9[:1], one),
                   PR.oseen_contract_pressure(one, one, f)):
        assert ref[0] == 0 and A[0] == 0
    assert PR.P_RSQ == {"stokeslet_pressure": 3, "oseen_pressure": 3, "stresslet_pressure": 5}
    assert PR.E_RSQ is R.E_RSQ and PR.E_SEED is R.E_SEED  # imported, not re-measured


def _divergence_rows(grad_field, pts, h):
    """(d_j G_ij)[t, i] by central differences of the analytic G."""
    out = np.zeros((len(pts), 3))
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        out += (grad_field(pts + e)[:, :, j] - grad_field(pts - e)[:, :, j]) / (2 * h)
    return out


def _gradient_scalar(field, pts, h):
    out = np.zeros((len(pts), 3))
    for i in range(3):
        e = np.zeros(3)
        e[i] = h
        out[:, i] = (field(pts + e) - field(pts - e)) / (2 * h)
    return out


def test_momentum_balance():
    """eta d_j G_ij = d_i p by central differences (h = 1e-5) of the analytic
    gradient and of the pressure, 64 probes at least 0.5 from the 37 sources.
    Measured 8e-10 (Stokeslet) and 2e-9 (stresslet), all of it h^2 truncation;
    a wrong sign or prefactor gives O(1). The rotlet's eta d_j G_ij vanishes:
    its pressure is zero."""
    src, f3, f9, torque = cloud37()
    probes = far_probes(src, 64, seed=9)
    h = 1e-5
    cases = {
        "stokeslet": (lambda p: np_stokeslet_grad(src, f3, p, ETA),
                      lambda p: np_stokeslet_pressure(src, f3, p)),
        "stresslet": (lambda p: np_stresslet_grad(src, f9, p, ETA),
                      lambda p: np_stresslet_pressure(src, f9, p)),
    }
    for name, (G, p) in cases.items():
        lhs = ETA * _divergence_rows(G, probes, h)
        rhs = _gradient_scalar(p, probes, h)
        err = rel(lhs, rhs)
        print(f"momentum balance {name}: {err:.2e}")
        assert np.linalg.norm(rhs) > 1e-2
        assert err < 1e-7, (name, err)
    rot = ETA * _divergence_rows(lambda p: np_rotlet_grad(src, p, torque, ETA), probes, h)
    print(f"rotlet eta d_j G_ij: {np.abs(rot).max():.2e}")
    assert np.abs(rot).max() < 1e-7


def test_oseen_pressure_is_the_stokeslet_pressure_outside_eps():
    src, f3, _, _ = cloud37()
    probes = far_probes(src, 8, seed=10)
    assert np.array_equal(np_oseen_pressure(src, probes, f3),
                          np_stokeslet_pressure(src, f3, probes))


# ---- flows: stress, traction, surface integrals ---------------------------

def _empty_body_nodes():
    z = np.zeros((0, 3))
    return dict(node_pos=z, node_normals=z, densities=z)


def _surface_integrals(**terms):
    from skellysim_amd.flows import stress_at_targets, surface_force_torque
    pts, nrm, w = sphere_quadrature()
    sigma = stress_at_targets(pts, ETA, backend=NumpyPressureBackend(), **terms)
    assert sigma.shape == (len(pts), 3, 3)
    return surface_force_torque(pts, nrm, w, sigma, np.zeros(3))


def test_traction_integrals_stokeslets():
    """The sphere of radius 3 carries the force and torque applied inside:
    F = -sum f, T = -sum s x f about the origin."""
    src, f3, _, _ = cloud37()
    F, T = _surface_integrals(fiber=dict(r_src=src, forces=f3, weights=np.ones(len(src))))
    print("stokeslets", np.abs(F + f3.sum(0)).max(), np.abs(T + np.cross(src, f3).sum(0)).max())
    assert np.abs(F + f3.sum(axis=0)).max() < 1e-12
    assert np.abs(T + np.cross(src, f3).sum(axis=0)).max() < 1e-12


def test_traction_integrals_stresslets():
    """A double layer is force- and torque-free: F = T = 0."""
    src, nrm, _, rho = cloud37()
    F, T = _surface_integrals(shell=dict(node_pos=src, node_normal=nrm, density=rho))
    print("stresslets", np.abs(F).max(), np.abs(T).max())
    assert np.abs(F).max() < 1e-12 and np.abs(T).max() < 1e-12


def test_traction_integrals_rotlets():
    """Point torques: F = 0, T = -sum torque."""
    src, _, _, torque = cloud37()
    F, T = _surface_integrals(bodies=dict(_empty_body_nodes(), centers=src,
                                          forces=np.zeros_like(src), torques=torque))
    print("rotlets", np.abs(F).max(), np.abs(T + torque.sum(0)).max())
    assert np.abs(F).max() < 1e-12
    assert np.abs(T + torque.sum(axis=0)).max() < 1e-12


def test_surface_force_torque_origin_and_torch():
    """T about another origin is T0 - origin x F; torch tensors give the same
    numbers as numpy."""
    import torch
    from skellysim_amd.flows import stress_at_targets, surface_force_torque, traction
    src, f3, _, _ = cloud37()
    pts, nrm, w = sphere_quadrature(n_theta=8, n_phi=16)
    sigma = stress_at_targets(pts, ETA, backend=NumpyPressureBackend(),
                              fiber=dict(r_src=src, forces=f3, weights=np.ones(len(src))))
    F, T0 = surface_force_torque(pts, nrm, w, sigma, np.zeros(3))
    o = np.array([0.3, -0.2, 0.5])
    F1, T1 = surface_force_torque(pts, nrm, w, sigma, o)
    assert np.array_equal(F, F1) and np.allclose(T1, T0 - np.cross(o, F), rtol=0, atol=1e-13)
    t = torch.from_numpy
    Ft, Tt = surface_force_torque(t(pts), t(nrm), t(w), t(sigma), o)
    assert np.allclose(Ft.numpy(), F, rtol=0, atol=1e-14)
    assert np.allclose(Tt.numpy(), T1, rtol=0, atol=1e-14)
    # (another summation order of the three products: a few roundings of ~0.1)
    assert np.allclose(traction(t(sigma), t(nrm)).numpy(), traction(sigma, nrm), rtol=0,
                       atol=1e-15)
    assert np.array_equal(traction(sigma, nrm), np.einsum("nij,nj->ni", sigma, nrm))


def test_stress_from_fields_matches_closed_form_stokeslet_stress():
    """sigma_ij = -3/(4 pi) sum (f.d) d_i d_j y^5 for a Stokeslet cloud, from
    p and G of the separate closed forms: 1e-12 relative."""
    import torch
    from skellysim_amd.flows import stress_from_fields
    src, f3, _, _ = cloud37()
    probes = far_probes(src, 64, seed=11)
    p = np_stokeslet_pressure(src, f3, probes)
    G = np_stokeslet_grad(src, f3, probes, ETA)
    sigma = stress_from_fields(p, G, ETA)
    d = probes[:, None, :] - src[None, :, :]
    y5 = np.einsum("tsk,tsk->ts", d, d) ** -2.5
    want = -3.0 / FOUR_PI * np.einsum("ts,tsi,tsj->tij", y5 * np.einsum("sk,tsk->ts", f3, d),
                                      d, d)
    print("stress vs closed form", rel(sigma, want))
    assert sigma.shape == (64, 3, 3) and rel(sigma, want) < 1e-12
    assert np.array_equal(sigma, sigma.transpose(0, 2, 1))
    st = stress_from_fields(torch.from_numpy(p), torch.from_numpy(G), ETA)
    assert np.allclose(st.numpy(), sigma, rtol=0, atol=1e-15 * np.abs(sigma).max())


def test_pressure_at_targets_sums_the_terms():
    from skellysim_amd.flows import pressure_at_targets, stress_at_targets, stress_from_fields
    rng = np.random.default_rng(12)
    src, f3, _, torque = cloud37()
    wts = rng.uniform(0.1, 0.2, len(src))
    sh = dict(node_pos=rng.uniform(-1, 1, (20, 3)), node_normal=rng.uniform(-1, 1, (20, 3)),
              density=rng.uniform(-1, 1, (20, 3)))
    bd = dict(node_pos=rng.uniform(-1, 1, (15, 3)), node_normals=rng.uniform(-1, 1, (15, 3)),
              densities=rng.uniform(-1, 1, (15, 3)), centers=src[:2], forces=f3[:2],
              torques=torque[:2])
    fib = dict(r_src=src, forces=f3, weights=wts)
    trg = far_probes(np.concatenate([src, sh["node_pos"], bd["node_pos"]]), 9, seed=13)
    be = NumpyPressureBackend()
    dl = lambda n, d: 2.0 * ETA * np.einsum("ni,nj->nij", n, d).reshape(-1, 9)
    want = (np_stokeslet_pressure(src, f3 * wts[:, None], trg)
            + np_stresslet_pressure(sh["node_pos"], dl(sh["node_normal"], sh["density"]), trg)
            + np_stresslet_pressure(bd["node_pos"], dl(bd["node_normals"], bd["densities"]), trg)
            + np_stokeslet_pressure(src[:2], f3[:2], trg))
    p = pressure_at_targets(trg, ETA, fiber=fib, shell=sh, bodies=bd, backend=be)
    assert p.shape == (9,) and np.allclose(p, want, rtol=1e-13, atol=0)
    G = (np_stokeslet_grad(src, f3 * wts[:, None], trg, ETA)
         + np_stresslet_grad(sh["node_pos"], dl(sh["node_normal"], sh["density"]), trg, ETA)
         + np_stresslet_grad(bd["node_pos"], dl(bd["node_normals"], bd["densities"]), trg, ETA)
         + np_stokeslet_grad(src[:2], f3[:2], trg, ETA)
         + np_rotlet_grad(src[:2], trg, torque[:2], ETA))
    sigma = stress_at_targets(trg, ETA, fiber=fib, shell=sh, bodies=bd, backend=be)
    assert rel(sigma, stress_from_fields(want, G, ETA)) < 1e-13
    # nothing in, nothing out
    assert not pressure_at_targets(trg, ETA, backend=be).any()
    assert not stress_at_targets(trg, ETA, backend=be).any()


# ---- sources ----------------------------------------------------------------

def test_sources_flow_pressure():
    from skellysim_amd.sources import PointSource, PointSourceContainer, BackgroundSource
    always = PointSource(position=(0.1, 0.2, 0.3), force=(1.0, 0.0, -0.5),
                         torque=(0.0, 0.2, 0.0))
    mortal = PointSource(position=(-0.4, 0.0, 0.1), force=(0.0, 2.0, 0.0), time_to_live=1.0)
    torquer = PointSource(position=(0.5, 0.5, -0.2), torque=(0.3, 0.0, 0.1))
    psc = PointSourceContainer([always, mortal, torquer])
    be = NumpyPressureBackend()
    pts = far_probes(np.stack([p.position for p in psc.points]), 6, seed=5)

    def want(points):
        return sum(np_oseen_pressure(p.position[None], pts, p.force[None]) for p in points)

    early, late = psc.flow_pressure(pts, 0.5, be), psc.flow_pressure(pts, 1.0, be)
    assert early.shape == (6,)
    assert np.allclose(early, want([always, mortal]), rtol=1e-13, atol=0)
    assert np.allclose(late, want([always]), rtol=1e-13, atol=0)
    assert rel(early, late) > 1e-2
    # torques alone and no sources: zeros, and no backend call
    assert not PointSourceContainer([torquer]).flow_pressure(pts, 0.0, None).any()
    assert PointSourceContainer([]).flow_pressure(pts, 0.0, None).shape == (6,)
    bs = BackgroundSource(components=(1, 2, 0), scale_factor=(0.3, -0.2, 0.1),
                          uniform=(0.05, 0.0, -0.02))
    p = bs.flow_pressure(pts)
    assert p.shape == (6,) and not p.any()


# ---- listener ---------------------------------------------------------------

def _request(pressure_x=None, stress_x=None):
    cmd = {
        "frame_no": 1,
        "evaluator": "GPU",
        "streamlines": {"dt_init": 0.05, "t_final": 0.1, "abs_err": 1e-10,
                        "rel_err": 1e-8, "back_integrate": False, "x0": SEED},
        "vortexlines": {"dt_init": 0.05, "t_final": 0.1, "abs_err": 1e-10,
                        "rel_err": 1e-8, "back_integrate": False, "x0": np.zeros((0, 3))},
        "velocity_field": {"x": FIELD_X},
    }
    if pressure_x is not None:
        cmd["pressure"] = {"x": pressure_x}
    if stress_x is not None:
        cmd["stress"] = {"x": stress_x}
    msg = msgpack.packb(cmd, default=_ndencode)
    return struct.pack("<Q", len(msg)) + msg


def _serve(traj, request, compute, **kw):
    from skellysim_amd.listener import serve
    stdin = io.BytesIO(request + struct.pack("<Q", 0))
    stdout = io.BytesIO()
    serve(stdin, stdout, traj, compute, eta=1.0, **kw)
    raw = stdout.getvalue()
    (size,) = struct.unpack("<Q", raw[:8])
    assert len(raw) == 8 + size
    return raw, msgpack.unpackb(raw[8:], raw=False)


def test_serve_default_request_never_calls_a_pressure_method():
    """Without the two keys the response is, byte for byte, what a backend
    without pressure methods gives, and no pressure method is reached."""
    traj = bent_fiber_frame()
    raw_plain, res = _serve(traj, _request(), NumpyBackend())
    raw_guarded, _ = _serve(traj, _request(), NoPressureBackend())
    assert raw_guarded == raw_plain
    assert list(res.keys()) == ["time", "i_frame", "n_frames", "streamlines", "vortexlines",
                                "velocity_field"]
    # ... and the keys do need them
    with pytest.raises(AssertionError, match="pressure method"):
        _serve(traj, _request(pressure_x=FIELD_X), NoPressureBackend())
    with pytest.raises(AttributeError):
        _serve(traj, _request(stress_x=FIELD_X), NumpyBackend())


def test_serve_pressure_and_stress_blocks():
    from skellysim_amd.listener import eigen_decode, pressure_field, stress_field
    traj = bent_fiber_frame()
    be = NumpyPressureBackend()
    frame = traj.frames[1]
    _, base = _serve(traj, _request(), be)
    _, res = _serve(traj, _request(pressure_x=FIELD_X, stress_x=FIELD_X[:2]), be)
    assert list(res.keys()) == list(base.keys()) + ["pressure", "stress"]
    assert {k: res[k] for k in base} == base
    assert res["pressure"][:3] == ["__eigen__", 1, len(FIELD_X)]
    assert res["stress"][:3] == ["__eigen__", 9, 2]
    p = eigen_decode(res["pressure"])
    assert p.shape == (len(FIELD_X),)
    assert np.array_equal(p, pressure_field(frame, FIELD_X, 1.0, be))
    assert np.linalg.norm(p) > 0
    block = eigen_decode(res["stress"])
    assert block.shape == (9, 2)
    assert np.array_equal(block.T.reshape(-1, 3, 3), stress_field(frame, FIELD_X[:2], 1.0, be))
    # a key with no points gives an empty block
    _, res0 = _serve(traj, _request(pressure_x=np.zeros((0, 3))), be)
    assert res0["pressure"] == ["__eigen__", 1, 0]


def _stress_divergence(frame, probes, be, h=1e-5, **kw):
    from skellysim_amd.listener import stress_field
    div = np.zeros((len(probes), 3))
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        div += (stress_field(frame, probes + e, 1.0, be, **kw)[:, :, j]
                - stress_field(frame, probes - e, 1.0, be, **kw)[:, :, j]) / (2 * h)
    return div


def test_stress_field_is_divergence_free_with_shell():
    """d_j sigma_ij = 0 away from the sources, fibers + shell: differences at
    h = 1e-5 against the size of grad p (truncation ~ (h/r)^2, gate 1e-6)."""
    from skellysim_amd.listener import pressure_field, stress_field
    from skellysim_amd.flows import stress_from_fields
    from skellysim_amd.listener import velocity_gradient_field
    frame = bent_fiber_frame().frames[-1]
    fx, geom = shell_fixture()
    frame["shell"] = {"solution_vec_": np.asarray(fx["density"], float).reshape(-1)}
    probes = far_probes(np.concatenate([fiber_nodes(frame), fx["nodes"]]), 8, seed=2)
    be = NumpyPressureBackend()
    kw = dict(shell_geometry=geom)
    div = _stress_divergence(frame, probes, be, **kw)
    grad_p = _gradient_scalar(lambda x: pressure_field(frame, x, 1.0, be, **kw), probes, 1e-5)
    print("div sigma / grad p", np.linalg.norm(div) / np.linalg.norm(grad_p))
    assert np.linalg.norm(grad_p) > 0
    assert np.linalg.norm(div) < 1e-6 * np.linalg.norm(grad_p)
    # the shell takes part, and the stress is the composition of the two fields
    p, p_fib = pressure_field(frame, probes, 1.0, be, **kw), pressure_field(frame, probes, 1.0, be)
    assert rel(p, p_fib) > 1e-3
    sigma = stress_field(frame, probes, 1.0, be, **kw)
    assert np.array_equal(sigma, stress_from_fields(
        p, velocity_gradient_field(frame, probes, 1.0, be, **kw), 1.0))


def test_pressure_and_stress_inside_a_body():
    from skellysim_amd.listener import bodies_from_frame, pressure_field, stress_field
    frame, geom = body_fixture()
    (b,) = bodies_from_frame(frame, geom)
    outside = far_probes(b.nodes, 6, seed=3)
    inside = b.position + np.array([0.3, 0.1, 0.0])
    assert np.linalg.norm(inside - b.position) < b.radius
    probes = np.concatenate([outside, inside[None]])
    be = NumpyPressureBackend()
    p = pressure_field(frame, probes, 1.0, be, body_geometry=geom)
    sigma = stress_field(frame, probes, 1.0, be, body_geometry=geom)
    assert p[-1] == 0.0 and not sigma[-1].any()
    assert np.all(p[:-1] != 0.0) and np.linalg.norm(sigma[:-1]) > 0
    assert np.array_equal(p[:-1], pressure_field(frame, outside, 1.0, be, body_geometry=geom))
    div = _stress_divergence(frame, outside, be, body_geometry=geom)
    grad_p = _gradient_scalar(lambda x: pressure_field(frame, x, 1.0, be, body_geometry=geom),
                              outside, 1e-5)
    assert np.linalg.norm(div) < 1e-6 * np.linalg.norm(grad_p)


def test_pressure_and_stress_fields_with_sources():
    from skellysim_amd.sources import PointSource, PointSourceContainer, BackgroundSource
    from skellysim_amd.listener import pressure_field, stress_field
    from skellysim_amd.flows import stress_from_fields
    frame = bent_fiber_frame().frames[-1]
    psc = PointSourceContainer([
        PointSource(position=(0.4, -0.3, 0.2), force=(0.3, -0.1, 0.2)),
        PointSource(position=(-0.5, 0.2, 0.6), torque=(0.0, 0.4, -0.2)),
        PointSource(position=(0.0, 0.9, -0.4), force=(9.0, 9.0, 9.0), time_to_live=0.05),
    ])
    bs = BackgroundSource(components=(1, 2, 0), scale_factor=(0.3, -0.2, 0.1),
                          uniform=(0.05, 0.0, -0.02))
    pts = np.concatenate([fiber_nodes(frame)] + [p.position[None] for p in psc.points])
    probes = far_probes(pts, 8, seed=4)
    be = NumpyPressureBackend()
    p = pressure_field(frame, probes, 1.0, be, sources=(psc, bs))
    p_bare = pressure_field(frame, probes, 1.0, be)
    extra_p = psc.flow_pressure(probes, float(frame["time"]), be)
    assert np.allclose(p - p_bare, extra_p, rtol=0, atol=1e-14)
    assert np.linalg.norm(extra_p) > 1e-3
    sigma = stress_field(frame, probes, 1.0, be, sources=(psc, bs))
    extra_G = psc.flow_grad(probes, 1.0, float(frame["time"]), be) + bs.flow_grad(probes)
    assert np.allclose(sigma - stress_field(frame, probes, 1.0, be),
                       stress_from_fields(extra_p, extra_G, 1.0), rtol=0, atol=1e-13)


# ---- evaluator argument checks (no device) ------------------------------------

N = 10
RNG = np.random.default_rng(0)
R_SRC, R_TRG = RNG.uniform(-1, 1, (N, 3)), RNG.uniform(-1, 1, (4, 3))


def _host_forms():
    from skellysim_amd import evaluator as ev
    return {
        "stokeslet_pressure": (lambda f: ev.stokeslet_pressure(R_SRC, f, R_TRG), 3, "f_src"),
        "stresslet_pressure": (lambda f: ev.stresslet_pressure(R_SRC, f, R_TRG), 9, "f_src"),
        "oseen_contract_pressure": (lambda f: ev.oseen_contract_pressure(R_SRC, R_TRG, f), 3,
                                    "density"),
    }


FORMS = ["stokeslet_pressure", "stresslet_pressure", "oseen_contract_pressure"]


@pytest.fixture
def no_library(monkeypatch):
    from skellysim_amd import _native

    def lib():
        raise AssertionError("reached the library")
    monkeypatch.setattr(_native, "lib", lib)


@pytest.mark.parametrize("form", FORMS)
def test_pressure_host_form_rejects_bad_strengths(no_library, form):
    call, dim, name = _host_forms()[form]
    for n_f in (N - 1, N + 1):
        with pytest.raises(ValueError, match=name):
            call(RNG.uniform(-1, 1, (n_f, dim)))
        with pytest.raises(ValueError, match=name):
            call(RNG.uniform(-1, 1, (n_f, dim)).T)
    with pytest.raises(ValueError, match=name):
        call(None)
    with pytest.raises(ValueError, match=name):      # wrong trailing dimension
        call(RNG.uniform(-1, 1, (N, dim + 1)))
    with pytest.raises(ValueError, match=name):
        call(RNG.uniform(-1, 1, N * dim))            # not 2-D


@pytest.mark.parametrize("form", FORMS)
def test_pressure_host_form_reaches_its_entry_point(monkeypatch, form):
    """Matching lengths call skelly_<form>_host with (n_src, n_trg) and the
    trailing doubles only (no eta); the result is (n_trg,)."""
    from skellysim_amd import _native
    calls = []

    class Recorder:
        def __getattr__(self, name):
            def fn(*args):
                calls.append((name, [a for a in args if isinstance(a, int)],
                              [a for a in args if isinstance(a, float)]))
                return 0
            return fn

    monkeypatch.setattr(_native, "lib", lambda: Recorder())
    call, dim, _ = _host_forms()[form]
    out = call(RNG.uniform(-1, 1, (N, dim)))
    assert out.shape == (len(R_TRG),)
    scalars = [5e-3, 1e-5] if form == "oseen_contract_pressure" else []
    assert calls == [(f"skelly_{form}_host", [N, len(R_TRG)], scalars)]


def test_pressure_device_forms_refuse_host_arrays():
    from skellysim_amd import evaluator as ev
    import torch
    f = RNG.uniform(-1, 1, (N, 3))
    with pytest.raises(TypeError, match="CUDA"):
        ev.stokeslet_pressure_device(R_SRC, f, R_TRG)
    with pytest.raises(TypeError, match="CUDA"):
        ev.stresslet_pressure_device(torch.from_numpy(R_SRC), torch.zeros(N, 9), R_TRG)
    with pytest.raises(TypeError, match="CUDA"):
        ev.oseen_contract_pressure_device(torch.from_numpy(R_SRC), torch.from_numpy(R_TRG),
                                          torch.from_numpy(f))


def test_native_declares_the_pressure_entry_points():
    import ctypes
    from skellysim_amd import _native
    D, N = ctypes.c_double, _native.PressureCount
    assert issubclass(N, ctypes.c_longlong) and ctypes.sizeof(N) == 8
    for name in ("stokeslet_pressure", "stresslet_pressure"):
        _, argtypes = _native.SIGNATURES[f"skelly_{name}_host"]
        assert D not in argtypes and argtypes.count(N) == 2 and len(argtypes) == 6
        assert len(_native.SIGNATURES[f"skelly_{name}_device"][1]) == 7
    _, argtypes = _native.SIGNATURES["skelly_oseen_contract_pressure_host"]
    assert argtypes.count(D) == 2 and argtypes.count(N) == 2 and len(argtypes) == 8
    assert "skelly_rotlet_pressure_host" not in _native.SIGNATURES
    assert sorted(PRESSURE_ENTRY_POINTS) == sorted(
        n for n, (_, argtypes) in _native.SIGNATURES.items() if N in argtypes)


# ---- the C boundary: null pointers, a negative or a zero count ---------------------
# What tests/test_evaluator_arguments.py asks of the velocity and gradient entry
# points, asked of the six pressure entry points: an error before any HIP call
# (there is no GPU here, and the pointers are null).

PRESSURE_ENTRY_POINTS = [f"skelly_{k}_{form}" for k in FORMS for form in ("host", "device")]


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    import ctypes
    from skellysim_amd import _native
    so = ctypes.CDLL(hip_lib_path)
    _native._bind(so)
    return so


def _null_call(name, counts):
    """Arguments of one entry point: null pointers, scalars of the defaults'
    size, `counts` in the two count positions (n_src, n_trg)."""
    import ctypes
    from skellysim_amd import _native
    counts = iter(counts)
    return [next(counts) if t is _native.PressureCount else 1e-3 if t is ctypes.c_double
            else None for t in _native.SIGNATURES[name][1]]


def _call_and_message(lib, name, args):
    """(return value, skelly_hip_last_error()) on a thread of its own: the
    message is per thread, and the main thread's stays empty for test_abi.py."""
    import threading
    got = []

    def run():
        got.append(getattr(lib, name)(*args))
        got.append(lib.skelly_hip_last_error().decode())
    t = threading.Thread(target=run)
    t.start()
    t.join()
    return got


@pytest.mark.parametrize("counts", [(-1, 5), (5, -1), (-(1 << 40), 5)],
                         ids=["n_src", "n_trg", "far_negative_n_src"])
@pytest.mark.parametrize("name", PRESSURE_ENTRY_POINTS)
def test_pressure_negative_count_is_an_error_before_any_launch(lib, name, counts):
    rc, msg = _call_and_message(lib, name, _null_call(name, counts))
    assert rc != 0
    assert msg == name + ": negative size", msg


@pytest.mark.parametrize("name", PRESSURE_ENTRY_POINTS)
def test_pressure_zero_target_count_is_no_error(lib, name):
    rc, msg = _call_and_message(lib, name, _null_call(name, (5, 0)))
    assert rc == 0 and msg == ""


def test_sharded_evaluator_accepts_the_pressure_kernels(monkeypatch):
    from skellysim_amd import evaluator as ev
    from skellysim_amd.sharded import ShardedPairEvaluator
    seen = []
    monkeypatch.setattr(ev, "stokeslet_pressure_device",
                        lambda r, f, t: seen.append("sl") or "p_sl")
    monkeypatch.setattr(ev, "stresslet_pressure_device",
                        lambda r, f, t: seen.append("dl") or "p_dl")
    assert ShardedPairEvaluator(kernel="stokeslet_pressure")(R_SRC, R_SRC, R_TRG, eta=7.0) == "p_sl"
    assert ShardedPairEvaluator(kernel="stresslet_pressure")(R_SRC, R_SRC, R_TRG) == "p_dl"
    assert seen == ["sl", "dl"]
    with pytest.raises(ValueError):
        ShardedPairEvaluator(kernel="rotlet_pressure")
