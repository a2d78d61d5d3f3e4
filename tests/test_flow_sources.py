"""CPU tests of skellysim_amd/flow_sources.py, the one statement of which
sources make up a flow: the backend calls every field makes, in the documented
order (point forces, point torques, background, fibers, shell, body nodes,
body centre stokeslets, body centre rotlets); evaluate() against the sum
written out term by term; one frame build per listener request; one liveness
rule for the point sources. No library is needed."""

import io
import struct

import msgpack
import numpy as np

from test_gradient_cpu import (_ndencode, bent_fiber_frame, shell_fixture, body_fixture, EPS)
from test_pressure_cpu import NumpyPressureBackend

ETA = 1.3
SHAPES = {"": (3,), "_grad": (3, 3), "_pressure": ()}


class RecordingBackend:
    """Logs each call as (method, shapes of its array arguments, eta or None)
    and returns zeros of the method's shape; the targets are the arrays with
    `n_trg` rows."""

    def __init__(self, n_trg):
        self.n_trg = n_trg
        self.calls = []

    def __getattr__(self, name):
        suffix = next(s for s in ("_grad", "_pressure", "") if name.endswith(s))

        def method(*args):
            arrays = [a for a in args if isinstance(a, np.ndarray)]
            (eta,) = [a for a in args if not isinstance(a, np.ndarray)] or [None]
            self.calls.append((name, tuple(a.shape for a in arrays), eta))
            return np.zeros((self.n_trg,) + SHAPES[suffix])
        return method


def full_frame():
    """Two bent fibers (32 nodes), the 192-node shell, one 192-node body, a
    live and an expired point force, a point torque, an active background."""
    from skellysim_amd.sources import PointSource, PointSourceContainer, BackgroundSource
    frame, body_geometry = body_fixture()
    frame["fibers"] = bent_fiber_frame().frames[-1]["fibers"]
    fx, shell_geometry = shell_fixture()
    frame["shell"] = {"solution_vec_": np.asarray(fx["density"], float).reshape(-1)}
    frame["time"] = 0.2
    psc = PointSourceContainer([
        PointSource(position=(0.4, -0.3, 0.2), force=(0.3, -0.1, 0.2)),
        PointSource(position=(0.0, 0.9, -0.4), force=(9.0, 9.0, 9.0), time_to_live=0.05),
        PointSource(position=(-0.5, 0.2, 0.6), torque=(0.0, 0.4, -0.2))])
    bs = BackgroundSource(components=(1, 2, 0), scale_factor=(0.3, -0.2, 0.1),
                          uniform=(0.05, 0.0, -0.02))
    return frame, dict(shell_geometry=shell_geometry, body_geometry=body_geometry,
                       sources=(psc, bs))


def test_listener_fields_call_the_backend_in_the_documented_order():
    from skellysim_amd import listener
    frame, kw = full_frame()
    targets = np.random.default_rng(0).uniform(-3, 3, (5, 3))
    # read off the fields' code as it stood before flow_sources
    velocity = [
        ("oseen_contract", ((1, 3), (5, 3), (1, 3)), ETA),
        ("rotlet", ((1, 3), (1, 3), (5, 3)), ETA),
        ("stokeslet", ((32, 3), (32, 3), (5, 3)), ETA),
        ("stresslet_normal_density", ((192, 3), (192, 3), (192, 3), (5, 3)), ETA),
        ("stresslet_normal_density", ((192, 3), (192, 3), (192, 3), (5, 3)), ETA),
        ("stokeslet", ((1, 3), (1, 3), (5, 3)), ETA),
        ("rotlet", ((1, 3), (1, 3), (5, 3)), ETA),
    ]
    gradient = [(name + "_grad", shapes, eta) for name, shapes, eta in velocity]
    pressure = [
        ("oseen_contract_pressure", ((1, 3), (5, 3), (1, 3)), None),
        ("stokeslet_pressure", ((32, 3), (32, 3), (5, 3)), None),
        ("stresslet_normal_density_pressure", ((192, 3), (192, 3), (192, 3), (5, 3)), ETA),
        ("stresslet_normal_density_pressure", ((192, 3), (192, 3), (192, 3), (5, 3)), ETA),
        ("stokeslet_pressure", ((1, 3), (1, 3), (5, 3)), None),
    ]
    for field, want in ((listener.velocity_field, velocity),
                        (listener.velocity_gradient_field, gradient),
                        (listener.pressure_field, pressure),
                        (listener.stress_field, pressure + gradient)):
        be = RecordingBackend(5)
        field(frame, targets, ETA, be, **kw)
        assert be.calls == want, field.__name__
    # an already built flow gives the same calls, and builds nothing
    flow = listener.frame_flow(frame, ETA, **kw)
    be = RecordingBackend(5)
    listener.stress_field(None, targets, ETA, be, flow=flow)
    assert be.calls == pressure + gradient


def test_flows_at_targets_call_the_backend_in_the_documented_order(monkeypatch):
    from skellysim_amd import flows, flow_sources
    rng = np.random.default_rng(1)
    a = lambda n: rng.uniform(-1, 1, (n, 3))
    fiber = dict(r_src=a(37), forces=a(37), weights=rng.uniform(0.1, 0.2, 37))
    shell = dict(node_pos=a(20), node_normal=a(20), density=a(20))
    bodies = dict(node_pos=a(15), node_normals=a(15), densities=a(15), centers=a(1),
                  forces=a(1), torques=a(1))
    targets = a(4)
    be = RecordingBackend(4)
    monkeypatch.setattr(flow_sources, "default_backend", lambda targets: be)
    velocity = [
        ("stokeslet", ((37, 3), (37, 3), (4, 3)), ETA),
        ("stresslet_normal_density", ((20, 3), (20, 3), (20, 3), (4, 3)), ETA),
        ("stresslet_normal_density", ((15, 3), (15, 3), (15, 3), (4, 3)), ETA),
        ("stokeslet", ((1, 3), (1, 3), (4, 3)), ETA),
        ("rotlet", ((1, 3), (1, 3), (4, 3)), ETA),
    ]
    gradient = [(name + "_grad", shapes, eta) for name, shapes, eta in velocity]
    pressure = [
        ("stokeslet_pressure", ((37, 3), (37, 3), (4, 3)), None),
        ("stresslet_normal_density_pressure", ((20, 3), (20, 3), (20, 3), (4, 3)), ETA),
        ("stresslet_normal_density_pressure", ((15, 3), (15, 3), (15, 3), (4, 3)), ETA),
        ("stokeslet_pressure", ((1, 3), (1, 3), (4, 3)), None),
    ]
    kw = dict(fiber=fiber, shell=shell, bodies=bodies)
    # the stress takes the gradient first, then the pressure (as it always did)
    for call, want in ((lambda: flows.velocity_at_targets(targets, ETA, **kw), velocity),
                       (lambda: flows.velocity_gradient_at_targets(targets, ETA, **kw), gradient),
                       (lambda: flows.pressure_at_targets(targets, ETA, backend=be, **kw),
                        pressure),
                       (lambda: flows.stress_at_targets(targets, ETA, backend=be, **kw),
                        gradient + pressure)):
        be.calls.clear()
        call()
        assert be.calls == want
    # empty parts are no terms: no call, zeros out
    be.calls.clear()
    empty = dict(r_src=a(0), forces=a(0), weights=np.zeros(0))
    assert not flows.velocity_at_targets(targets, ETA, fiber=empty).any()
    assert not flows.pressure_at_targets(targets, ETA, fiber=empty, backend=None).any()
    assert be.calls == []


def test_evaluate_is_the_term_by_term_sum_in_the_documented_order():
    from skellysim_amd.flow_sources import evaluate, flow_sources
    from skellysim_amd.sources import BackgroundSource
    rng = np.random.default_rng(2)
    a = lambda n: rng.uniform(-1, 1, (n, 3))
    fiber = dict(r_src=a(37), forces=a(37), weights=rng.uniform(0.1, 0.2, 37))
    shell = dict(node_pos=a(37), node_normal=a(37), density=a(37))
    center, radius = np.array([2.0, 0.5, -1.0]), 0.8
    velocity, omega = np.array([0.3, -0.2, 0.1]), np.array([0.5, 0.0, -0.7])
    bodies = dict(node_pos=center + radius * a(37), node_normals=a(37), densities=a(37),
                  centers=center[None], forces=a(1), torques=a(1), radii=np.array([radius]),
                  velocities=velocity[None], angular_velocities=omega[None])
    bs = BackgroundSource(components=(1, 2, 0), scale_factor=(0.3, -0.2, 0.1),
                          uniform=(0.05, 0.0, -0.02))
    sources = dict(force_pos=a(37), forces=a(37), torque_pos=a(37), torques=a(37),
                   background=(bs.uniform, bs.scale_factor, bs.components))
    dx_in = np.array([0.3, 0.1, 0.0])
    targets = np.concatenate([3.0 + a(5), (center + dx_in)[None]])  # last one inside the body
    inside = np.linalg.norm(targets - center, axis=1) < radius
    assert inside.tolist() == [False] * 5 + [True]
    flow = flow_sources(fiber, shell, bodies, sources)
    assert [t[0] for t in flow.terms] == ["oseen", "rotlet", "background", "stokeslet",
                                          "double_layer", "double_layer", "stokeslet", "rotlet"]
    be = NumpyPressureBackend()
    wf = fiber["forces"] * fiber["weights"][:, None]
    sh = (shell["node_pos"], shell["node_normal"], shell["density"])
    bd = (bodies["node_pos"], bodies["node_normals"], bodies["densities"])

    u = np.zeros((6, 3))
    u = u + be.oseen_contract(sources["force_pos"], targets, sources["forces"], ETA)
    u = u + be.rotlet(sources["torque_pos"], sources["torques"], targets, ETA)
    u = u + bs.flow(targets)
    u = u + be.stokeslet(fiber["r_src"], wf, targets, ETA)
    u = u + be.stresslet_normal_density(*sh, targets, ETA)
    u = u + be.stresslet_normal_density(*bd, targets, ETA)
    u = u + be.stokeslet(bodies["centers"], bodies["forces"], targets, ETA)
    u = u + be.rotlet(bodies["centers"], bodies["torques"], targets, ETA)
    assert np.linalg.norm(u[-1] - (velocity + np.cross(omega, dx_in))) > 1e-3
    u[-1] = velocity + np.cross(omega, targets[-1] - center)
    assert np.array_equal(evaluate(flow, "velocity", targets, ETA, be), u)

    G = np.zeros((6, 3, 3))
    G = G + be.oseen_contract_grad(sources["force_pos"], targets, sources["forces"], ETA)
    G = G + be.rotlet_grad(sources["torque_pos"], sources["torques"], targets, ETA)
    G = G + bs.flow_grad(targets)
    G = G + be.stokeslet_grad(fiber["r_src"], wf, targets, ETA)
    G = G + be.stresslet_normal_density_grad(*sh, targets, ETA)
    G = G + be.stresslet_normal_density_grad(*bd, targets, ETA)
    G = G + be.stokeslet_grad(bodies["centers"], bodies["forces"], targets, ETA)
    G = G + be.rotlet_grad(bodies["centers"], bodies["torques"], targets, ETA)
    G[-1] = np.einsum("ikj,k->ij", EPS, omega)
    assert np.array_equal(evaluate(flow, "gradient", targets, ETA, be), G)

    p = np.zeros(6)
    p = p + be.oseen_contract_pressure(sources["force_pos"], targets, sources["forces"])
    p = p + be.stokeslet_pressure(fiber["r_src"], wf, targets)
    p = p + be.stresslet_normal_density_pressure(*sh, targets, ETA)
    p = p + be.stresslet_normal_density_pressure(*bd, targets, ETA)
    p = p + be.stokeslet_pressure(bodies["centers"], bodies["forces"], targets)
    assert p[-1] != 0.0
    p[-1] = 0.0
    assert np.array_equal(evaluate(flow, "pressure", targets, ETA, be), p)
    assert np.all(u[:-1] != 0) and np.all(p[:-1] != 0) and np.linalg.norm(G[:-1]) > 0


def test_serve_builds_the_frame_once_a_request(monkeypatch):
    from skellysim_amd import listener
    traj = bent_fiber_frame()
    x = np.array([[0.8, 0.6, 0.5], [-0.7, 0.9, 0.2]])
    seeds = np.array([[0.9, 0.5, 0.4], [-0.6, 0.7, 0.3]])
    line = {"dt_init": 0.05, "t_final": 0.1, "abs_err": 1e-10, "rel_err": 1e-8,
            "back_integrate": False}
    builds = []
    real = listener.fibers_from_frame
    monkeypatch.setattr(listener, "fibers_from_frame",
                        lambda *a, **k: builds.append(1) or real(*a, **k))

    def serve(cmd):
        msg = msgpack.packb(dict(cmd, frame_no=1), default=_ndencode)
        stdout = io.BytesIO()
        listener.serve(io.BytesIO(struct.pack("<Q", len(msg)) + msg + struct.pack("<Q", 0)),
                       stdout, traj, NumpyPressureBackend(), eta=1.0)
        return msgpack.unpackb(stdout.getvalue()[8:], raw=False)

    res = serve({"velocity_field": {"x": x}, "velocity_gradient": {"x": x}, "pressure": {"x": x},
                 "stress": {"x": x}, "streamlines": dict(line, x0=seeds)})
    assert len(builds) == 1
    assert len(res["streamlines"]) == 2 and all(len(s["time"]) > 2 for s in res["streamlines"])
    assert all(res[k][2] == 2 for k in ("velocity_field", "velocity_gradient", "pressure",
                                        "stress"))
    # no block with points: no build at all
    builds.clear()
    res = serve({"velocity_field": {"x": np.zeros((0, 3))}, "pressure": {"x": np.zeros((0, 3))}})
    assert builds == [] and res["velocity_field"] == ["__eigen__", 3, 0]


def test_point_sources_have_one_liveness_rule():
    from skellysim_amd.listener import streamline_terms
    from skellysim_amd.sources import PointSource, PointSourceContainer
    always = PointSource(position=(0.1, 0.2, 0.3), force=(1.0, 0.0, -0.5),
                         torque=(0.0, 0.2, 0.0))
    mortal = PointSource(position=(-0.4, 0.0, 0.1), force=(0.0, 2.0, 0.0), time_to_live=1.0)
    torquer = PointSource(position=(0.5, 0.5, -0.2), torque=(0.3, 0.0, 0.1), time_to_live=2.0)
    idle = PointSource(position=(0.7, 0.7, 0.7))  # no force, no torque: never a source
    psc = PointSourceContainer([always, mortal, torquer, idle])

    def want(forcers, torquers):
        return {"force_pos": np.stack([p.position for p in forcers]),
                "forces": np.stack([p.force for p in forcers]),
                "torque_pos": np.stack([p.position for p in torquers]),
                "torques": np.stack([p.torque for p in torquers])}

    def same(got, expected):
        return list(got) == list(expected) and \
            all(np.array_equal(got[k], expected[k]) for k in expected)

    assert same(psc.live(0.0), want([always, mortal], [always, torquer]))
    assert same(psc.live(0.999), want([always, mortal], [always, torquer]))
    assert same(psc.live(1.0), want([always], [always, torquer]))   # time >= ttl: dead
    assert same(psc.live(2.0), want([always], [always]))
    assert same(psc.live(1e9), want([always], [always]))           # ttl 0: always alive
    assert PointSourceContainer([idle]).live(0.0) == {}
    assert list(PointSourceContainer([mortal]).live(0.5)) == ["force_pos", "forces"]
    # the listener's frame -> dicts step hands the same arrays on
    frame = bent_fiber_frame().frames[-1]
    for time in (0.5, 1.0, 2.0):
        frame["time"] = time
        got = streamline_terms(frame, 1.0, sources=(psc, None))["sources"]
        assert same(got, psc.live(time))
