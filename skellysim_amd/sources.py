"""Point sources and background source flows — the reference's
PointSourceContainer (src/core/point_source.cpp) and BackgroundSource
(src/core/background_source.cpp): static point forces/torques with optional
lifetimes (regularized-Stokeslet + rotlet flow) and an affine background
velocity field. Both enter the solver RHS through prep
(system.cpp:445-446) and the post-processing velocity field
(system.cpp:357-359)."""

import numpy as np


class PointSource:
    """One point forcer/torquer (point_source.hpp:7-15); time_to_live 0
    means always alive (point_source.cpp:22-24)."""

    def __init__(self, position=(0.0, 0.0, 0.0), force=(0.0, 0.0, 0.0),
                 torque=(0.0, 0.0, 0.0), time_to_live=0.0):
        self.position = np.asarray(position, float)
        self.force = np.asarray(force, float)
        self.torque = np.asarray(torque, float)
        self.time_to_live = float(time_to_live)


class PointSourceContainer:
    """point_source.cpp:16-55: regularized-Stokeslet (oseen contract) flow
    of the live forces + rotlet flow of the live torques."""

    def __init__(self, points=()):
        self.points = list(points)

    @classmethod
    def from_config(cls, tables):
        return cls([PointSource(position=t.get("position", (0, 0, 0)),
                                force=t.get("force", (0, 0, 0)),
                                torque=t.get("torque", (0, 0, 0)),
                                time_to_live=t.get("time_to_live", 0.0))
                    for t in tables])

    def live(self, time):
        """The sources alive at `time` as flow_sources' `sources` dict:
        force_pos/forces of those with a force, torque_pos/torques of those
        with a torque. time_to_live 0 means always alive, else a source is
        dead from time >= time_to_live on (point_source.cpp:22-24)."""
        live = [p for p in self.points
                if not (p.time_to_live and time >= p.time_to_live)]
        out = {}
        for pos, strength, attr in (("force_pos", "forces", "force"),
                                    ("torque_pos", "torques", "torque")):
            active = [p for p in live if getattr(p, attr).any()]
            if active:
                out[pos] = np.stack([p.position for p in active])
                out[strength] = np.stack([getattr(p, attr) for p in active])
        return out

    def _field(self, quantity, r_trg, eta, time, backend):
        from .flow_sources import evaluate, flow_sources
        return evaluate(flow_sources(sources=self.live(time)), quantity,
                        np.asarray(r_trg, float), eta, backend)

    def flow(self, r_trg, eta, time, backend):
        return self._field("velocity", r_trg, eta, time, backend)

    def flow_grad(self, r_trg, eta, time, backend):
        """Velocity gradient (n_trg, 3, 3) of flow()."""
        return self._field("gradient", r_trg, eta, time, backend)

    def flow_pressure(self, r_trg, time, backend):
        """Pressure (n_trg,) of flow(); the torques add nothing (a rotlet's
        pressure is zero). No eta: no pressure of a point source reads it."""
        return self._field("pressure", r_trg, None, time, backend)


class BackgroundSource:
    """background_source.cpp:14-22: v_j(r) = uniform_j +
    r[components_j] * scale_factor_j."""

    def __init__(self, components=(0, 1, 2), scale_factor=(0.0, 0.0, 0.0),
                 uniform=(0.0, 0.0, 0.0)):
        self.components = np.asarray(components, int)
        self.scale_factor = np.asarray(scale_factor, float)
        self.uniform = np.asarray(uniform, float)

    @classmethod
    def from_config(cls, table):
        return cls(components=table.get("components", (0, 1, 2)),
                   scale_factor=table.get("scale_factor", (0.0, 0.0, 0.0)),
                   uniform=table.get("uniform", (0.0, 0.0, 0.0)))

    def is_active(self):
        return bool(np.linalg.norm(self.uniform)
                    + np.linalg.norm(self.scale_factor))

    def flow(self, r_trg, eta=None):
        r = np.asarray(r_trg, float)
        return self.uniform[None, :] + r[:, self.components] \
            * self.scale_factor[None, :]

    def flow_grad(self, r_trg):
        """Velocity gradient (n_trg, 3, 3) of flow(): the constant matrix
        G[j, components[j]] = scale_factor[j]."""
        G = np.zeros((3, 3))
        G[np.arange(3), self.components] = self.scale_factor
        return np.broadcast_to(G, (len(np.asarray(r_trg, float).reshape(-1, 3)), 3, 3)).copy()

    def flow_pressure(self, r_trg):
        """Pressure (n_trg,) of flow(): zeros. A linear velocity field has no
        Laplacian, so the Stokes pressure is constant, taken as 0."""
        return np.zeros(len(np.asarray(r_trg, float).reshape(-1, 3)))
