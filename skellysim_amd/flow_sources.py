"""The sources of a flow, stated once, and every field quantity from them.

A flow is a FlowSources: an ordered list of terms, each a tuple (kind, arrays):

  ("oseen", r, forces)                   regularized point forces
  ("rotlet", r, torques)                 point torques
  ("stokeslet", r, weighted forces)
  ("double_layer", r, normals, density)
  ("background", uniform, scale_factor, components)   at most once

plus the rigid bodies (centers, radii, velocities, angular_velocities) inside
which the fluid moves with the body. The terms stand in TERM_ORDER, the order
they are summed in; summation order decides the last bit of a result, so it is
part of the contract. flow_sources() is the only place that builds the list:
from the dicts flows.velocity_at_targets / streamlines_at_seeds take, which
listener.streamline_terms makes from a trajectory frame and
PointSourceContainer.live from the configured point sources.

evaluate() sums the terms through a system_fd backend's methods, chosen by the
tables below, and then applies the inside-a-body rule. numpy arrays in give
numpy out, device tensors in give tensors out with no synchronization
(HipBackend's contract).
"""

from dataclasses import dataclass, field

import numpy as np
import torch

from .sources import BackgroundSource

TERM_ORDER = ("point forces (oseen)", "point torques (rotlet)", "background",
              "fibers (stokeslet)", "shell (double_layer)", "body nodes (double_layer)",
              "body centres (stokeslet)", "body centres (rotlet)")

# kind -> (stem of the backend method, position of the targets among its
# arrays): oseen_contract(r, r_trg, forces), rotlet(r, torques, r_trg),
# stokeslet(r, forces, r_trg), stresslet_normal_density(r, normals, density, r_trg)
KINDS = {"oseen": ("oseen_contract", 1), "rotlet": ("rotlet", 2), "stokeslet": ("stokeslet", 2),
         "double_layer": ("stresslet_normal_density", 3)}


def _rigid_velocity(dx, velocity, omega, xp):
    """velocity + omega x dx (system.cpp:363-371)."""
    if xp is torch:
        return velocity[None, :] + torch.linalg.cross(omega.expand_as(dx), dx)
    return velocity[None, :] + np.cross(np.broadcast_to(omega, dx.shape), dx)


def _rigid_gradient(dx, velocity, omega, xp):
    """G_ij = eps_ikj omega_k, the gradient of omega x r."""
    zero = xp.zeros_like(omega[0])
    return xp.stack([xp.stack([zero, -omega[2], omega[1]]),
                     xp.stack([omega[2], zero, -omega[0]]),
                     xp.stack([-omega[1], omega[0], zero])])


# quantity -> (suffix of the backend method, per-target shape, kinds whose
# method takes eta, BackgroundSource's contribution or None for zero, value
# inside a body or None for zero). A kind that `takes eta` does not list has
# no eta argument there; a rotlet has no pressure and no pressure method.
# The stress is stress_from_fields(pressure, gradient): inside a body p = 0
# and G is antisymmetric, so it is exactly 0 there.
QUANTITIES = {
    "velocity": ("", (3,), tuple(KINDS), lambda bs, r: bs.flow(r), _rigid_velocity),
    "gradient": ("_grad", (3, 3), tuple(KINDS), lambda bs, r: bs.flow_grad(r), _rigid_gradient),
    "pressure": ("_pressure", (), ("double_layer",), None, None),
}
NO_TERM = {("pressure", "rotlet")}


@dataclass
class FlowSources:
    terms: list = field(default_factory=list)
    bodies: dict = None

    @property
    def background(self):
        """(uniform, scale_factor, components), or None."""
        return next((t[1:] for t in self.terms if t[0] == "background"), None)


def flow_sources(fiber=None, shell=None, bodies=None, sources=None):
    """FlowSources from the flows-level dicts; empty parts contribute no term.

    fiber  = dict(r_src, forces, weights): forces times weights are the
             Stokeslet strengths (fiber self terms are never subtracted here)
    shell  = dict(node_pos, node_normal, density)
    bodies = dict(node_pos, node_normals, densities, centers, forces, torques
             [, radii, velocities, angular_velocities]): with the last three,
             points inside a body move rigidly with it (system.cpp:363-371)
    sources = dict with any of force_pos/forces, torque_pos/torques
             (PointSourceContainer.live) and background = (uniform,
             scale_factor, components)"""
    fiber, shell, bodies, sources = fiber or {}, shell or {}, bodies or {}, sources or {}
    terms = []

    def add(kind, part, r, *strength):
        if part.get(r) is not None and len(part[r]):
            terms.append((kind, part[r]) + tuple(part[s] for s in strength))

    add("oseen", sources, "force_pos", "forces")
    add("rotlet", sources, "torque_pos", "torques")
    if sources.get("background") is not None:
        terms.append(("background",) + tuple(sources["background"]))
    if fiber and len(fiber["r_src"]):
        terms.append(("stokeslet", fiber["r_src"], fiber["forces"] * fiber["weights"][:, None]))
    add("double_layer", shell, "node_pos", "node_normal", "density")
    add("double_layer", bodies, "node_pos", "node_normals", "densities")
    add("stokeslet", bodies, "centers", "forces")
    add("rotlet", bodies, "centers", "torques")
    rigid = None
    if bodies and len(bodies["centers"]) and bodies.get("radii") is not None:
        rigid = {k: bodies[k] for k in ("centers", "radii", "velocities", "angular_velocities")}
    return FlowSources(terms, rigid)


def zero_rows(targets, *shape):
    if torch.is_tensor(targets):
        return torch.zeros((targets.shape[0],) + shape, dtype=targets.dtype,
                           device=targets.device)
    return np.zeros((targets.shape[0],) + shape)


def default_backend(targets):
    from .system_fd import HipBackend
    return HipBackend(targets.device) if torch.is_tensor(targets) else HipBackend()


def evaluate(sources, quantity, targets, eta, backend=None):
    """`quantity` ("velocity", "gradient" or "pressure") of the flow at
    targets (n, 3): the terms summed in list order, each through its backend
    method, looked up only when the term is there; then the value inside the
    bodies. backend=None: HipBackend on the targets' device."""
    suffix, shape, takes_eta, background, inside_value = QUANTITIES[quantity]
    out = zero_rows(targets, *shape)
    for kind, *arrays in sources.terms:
        if kind == "background":
            if background is not None:
                if torch.is_tensor(targets):
                    raise TypeError("a background flow is evaluated at numpy targets")
                out = out + background(BackgroundSource(arrays[2], arrays[1], arrays[0]), targets)
            continue
        if (quantity, kind) in NO_TERM:
            continue
        backend = backend if backend is not None else default_backend(targets)
        stem, at = KINDS[kind]
        arrays.insert(at, targets)
        out = out + getattr(backend, stem + suffix)(*arrays, *((eta,) if kind in takes_eta else ()))
    b = sources.bodies
    if b is not None:
        xp = torch if torch.is_tensor(targets) else np
        for k in range(len(b["centers"])):
            dx = targets - b["centers"][k][None, :]
            inside = xp.sqrt((dx * dx).sum(1)) < b["radii"][k]
            value = 0.0 if inside_value is None else \
                inside_value(dx, b["velocities"][k], b["angular_velocities"][k], xp)
            out = xp.where(inside.reshape((-1,) + (1,) * len(shape)), value, out)
    return out
