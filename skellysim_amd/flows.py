"""Container-level flow operators of the hot path
and the periphery dense operators (§8f next-row 1), on-device.

Mirrors:
  periphery_flow      — Periphery::flow (reference src/core/periphery.cpp:55-79):
                        f_dl(i*3+j) = 2*eta*normal_i*density_j per node, then
                        the stresslet evaluator (already /eta).
  fiber_flow          — FiberContainerFiniteDifference::flow
                        (src/core/fiber_container_finite_difference.cpp:172-214):
                        quadrature-weighted forces -> stokeslet evaluation ->
                        optional per-fiber self-interaction subtraction
                        vel_fib -= stokeslet_fib @ wf (lines 203-210).
  ShellOperator       — Periphery::apply_preconditioner / matvec
                        (src/core/periphery.cpp:21-47): the two dense
                        per-GMRES-iteration GEMVs (M_inv_ and
                        stresslet_plus_complementary_) with HBM-resident
                        matrices, rocBLAS dgemv via torch.mv; in a
                        distributed world the rows are block-sharded and the
                        solution all-gathered per apply (the reference's
                        MPI_Allgatherv, periphery.cpp:26,44 -> RCCL).

The `*_flow_grad` / velocity_gradient_at_targets forms return the analytic
velocity gradient G[t, i, j] = du_i/dx_j of the same fields (no reference
counterpart: the reference differences the velocity), with
vorticity_from_gradient / strain_rate_from_gradient on top. The
`*_flow_pressure` / pressure_at_targets forms return the pressure of the same
fields, stress_at_targets the stress sigma = -p I + eta (G + G^T), and
traction / surface_force_torque what a surface carries.

All tensors are torch fp64; the pair-kernel legs require CUDA tensors (the
product path; no CPU fallback).
"""

import torch

from .flow_sources import default_backend as _default_backend, evaluate, flow_sources
from .sharded import allgather_rows


def double_layer_strength(normals, density, eta):
    """Stresslet source strength of a double layer, (n, 9) contiguous:
    f_dl(node)[i*3+j] = 2*eta*normal_i*density_j (periphery.cpp:68-71)."""
    return (2.0 * eta * torch.einsum("ni,nj->nij", normals, density)
            ).reshape(-1, 9).contiguous()


# ---------------------------------------------------------------------------
# Every field below is flow_sources.evaluate over the FlowSources of its
# arguments: which sources make up a flow, in which order they are summed and
# which backend method gives which quantity is stated there, once. The pair
# kernels are reached through a system_fd backend's methods: `backend=None`
# is HipBackend on r_trg's device (tensors in, tensors out, no
# synchronization); any object with the same methods on numpy arrays serves
# numpy inputs (the tests' closed forms). The pressure p is the Stokes
# pressure of the same fields (prefactor 1/(4 pi), no eta dependence of its
# own; a rotlet's is zero), the stress sigma = -p I + eta (G + G^T).
# ---------------------------------------------------------------------------

def _field(quantity, r_trg, eta, backend=None, **parts):
    return evaluate(flow_sources(**parts), quantity, r_trg, eta, backend)


def _shell(node_pos, node_normal, density):
    return dict(node_pos=node_pos, node_normal=node_normal, density=density)


def _fiber(r_src, fib_forces, weights):
    return dict(r_src=r_src, forces=fib_forces, weights=weights)


def _bodies(node_pos, node_normals, densities, centers, forces, torques):
    return dict(node_pos=node_pos, node_normals=node_normals, densities=densities,
                centers=centers, forces=forces, torques=torques)


def periphery_flow(node_pos, node_normal, density, r_trg, eta):
    """Velocity at r_trg due to the shell's double-layer density
    (Periphery::flow, periphery.cpp:55-79).

    node_pos, node_normal, density: (n_nodes, 3); r_trg: (n_trg, 3).
    f_dl(node)[i*3+j] = 2*eta*normal_i*density_j (periphery.cpp:68-71);
    the stresslet evaluator divides by eta (periphery.cpp:74).
    """
    return _field("velocity", r_trg, eta, shell=_shell(node_pos, node_normal, density))


def periphery_flow_grad(node_pos, node_normal, density, r_trg, eta):
    """Velocity gradient (n_trg, 3, 3), G[t, i, j] = du_i/dx_j, of
    periphery_flow's field."""
    return _field("gradient", r_trg, eta, shell=_shell(node_pos, node_normal, density))


def periphery_flow_pressure(node_pos, node_normal, density, r_trg, eta, backend=None):
    """Pressure (n_trg,) of periphery_flow's field."""
    return _field("pressure", r_trg, eta, backend, shell=_shell(node_pos, node_normal, density))


def _subtract_fiber_self(vel, wf, fiber_sizes, self_stokeslets):
    """vel[fiber nodes] -= stokeslet_fib @ wf per fiber
    (fiber_container_finite_difference.cpp:203-210), in place."""
    if fiber_sizes is None:
        raise ValueError("fiber_sizes required with self_stokeslets")
    if all(n == fiber_sizes[0] for n in fiber_sizes):
        # uniform fibers: one batched GEMV (rocBLAS batched under torch.bmm)
        n = fiber_sizes[0]
        nf = len(fiber_sizes)
        S = self_stokeslets if torch.is_tensor(self_stokeslets) \
            else torch.stack(list(self_stokeslets))
        wf_flat = wf.reshape(nf, 3 * n, 1)
        corr = torch.bmm(S, wf_flat).reshape(nf * n, 3)
        vel[: nf * n] -= corr
    else:
        off = 0
        for S, n in zip(self_stokeslets, fiber_sizes):
            wf_flat = wf[off: off + n].reshape(-1)
            vel[off: off + n] -= (S @ wf_flat).reshape(n, 3)
            off += n
    return vel


def fiber_flow(r_src, fib_forces, weights, r_trg, eta, fiber_sizes=None,
               self_stokeslets=None):
    """Velocity at r_trg due to fiber forces
    (FiberContainerFiniteDifference::flow).

    r_src, fib_forces: (n_fib_nodes, 3); weights: (n_fib_nodes,) — the
    per-node quadrature weights 0.5 * length * weights_0
    (fiber_container_finite_difference.cpp:186). If self_stokeslets is given
    (list/stacked tensor of per-fiber (3n, 3n) matrices, with fiber_sizes the
    per-fiber node counts), the per-fiber self term stokeslet_ @ wf is
    subtracted from that fiber's slice of the result (lines 203-210) — this
    requires r_trg to start with the fiber nodes in order, as in the
    reference's matvec (system.cpp:298-299).
    """
    vel = _field("velocity", r_trg, eta, fiber=_fiber(r_src, fib_forces, weights))
    if self_stokeslets is not None and r_src.shape[0]:
        _subtract_fiber_self(vel, fib_forces * weights[:, None], fiber_sizes, self_stokeslets)
    return vel


def fiber_flow_grad(r_src, fib_forces, weights, r_trg, eta):
    """Velocity gradient of fiber_flow's field without the self term (the
    reference's subtract_self = false, the post-processing form)."""
    return _field("gradient", r_trg, eta, fiber=_fiber(r_src, fib_forces, weights))


def fiber_flow_pressure(r_src, fib_forces, weights, r_trg, backend=None):
    """Pressure of fiber_flow's field without the self term (as
    fiber_flow_grad)."""
    return _field("pressure", r_trg, None, backend, fiber=_fiber(r_src, fib_forces, weights))


def _body_backend(r_trg, reg, epsilon_distance):
    """HipBackend on r_trg's device; its rotlets take the caller's
    regularization where that is not the library's default."""
    backend = _default_backend(r_trg)
    if (reg, epsilon_distance) != (5e-3, 1e-5):
        def rotlet(name):
            return lambda centers, torques, trg, eta: backend._eval(
                name, (centers, trg, torques), eta, reg=reg, epsilon_distance=epsilon_distance)
        backend.rotlet, backend.rotlet_grad = rotlet("rotlet"), rotlet("rotlet_grad")
    return backend


def body_flow(node_pos, node_normals, densities, centers, forces, torques, r_trg, eta,
              reg=5e-3, epsilon_distance=1e-5):
    """Velocity at r_trg due to rigid bodies (BodyContainer::flow_spherical /
    _ellipsoidal, src/core/body_container.cpp:269-410): a stresslet from the
    body quadrature nodes with f_dl = 2*eta*n_i*d_j (lines 299-302), plus a
    stokeslet from the body centers with the link forces (line 327), plus a
    rotlet from the centers with the torques (line 335; always direct)."""
    return _field("velocity", r_trg, eta, _body_backend(r_trg, reg, epsilon_distance),
                  bodies=_bodies(node_pos, node_normals, densities, centers, forces, torques))


def body_flow_grad(node_pos, node_normals, densities, centers, forces, torques, r_trg, eta,
                   reg=5e-3, epsilon_distance=1e-5):
    """Velocity gradient of body_flow's field, term by term."""
    return _field("gradient", r_trg, eta, _body_backend(r_trg, reg, epsilon_distance),
                  bodies=_bodies(node_pos, node_normals, densities, centers, forces, torques))


def body_flow_pressure(node_pos, node_normals, densities, centers, forces, torques, r_trg, eta,
                       backend=None):
    """Pressure of body_flow's field, term by term; the rotlet of the
    torques has none."""
    return _field("pressure", r_trg, eta, backend,
                  bodies=_bodies(node_pos, node_normals, densities, centers, forces, torques))


def velocity_at_targets(r_trg, eta, fiber=None, shell=None, bodies=None):
    """Composite free-space velocity at arbitrary targets — the kernel
    portion of System::velocity_at_targets (src/core/system.cpp:330-384,
    lines 355-359: fiber flow + shell flow + body flow, summed in
    flow_sources.TERM_ORDER).

    fiber  = dict(r_src, forces, weights[, fiber_sizes, self_stokeslets]):
             with self_stokeslets, fiber_flow's self term is subtracted from
             the sum
    shell  = dict(node_pos, node_normal, density)
    bodies = dict(node_pos, node_normals, densities, centers, forces, torques
             [, radii, velocities, angular_velocities]): with the last three,
             points inside a body get its rigid motion (system.cpp:363-371)
    """
    u = _field("velocity", r_trg, eta, fiber=fiber, shell=shell, bodies=bodies)
    if fiber is not None and fiber.get("self_stokeslets") is not None and fiber["r_src"].shape[0]:
        _subtract_fiber_self(u, fiber["forces"] * fiber["weights"][:, None],
                             fiber.get("fiber_sizes"), fiber["self_stokeslets"])
    return u


def velocity_gradient_at_targets(r_trg, eta, fiber=None, shell=None, bodies=None):
    """Gradient (n_trg, 3, 3) of velocity_at_targets' field, same dict
    inputs; the fiber self term is never subtracted (fiber_flow_grad)."""
    return _field("gradient", r_trg, eta, fiber=fiber, shell=shell, bodies=bodies)


def vorticity_from_gradient(G):
    """Curl of the velocity from G[..., i, j] = du_i/dx_j (torch or numpy):
    (G21 - G12, G02 - G20, G10 - G01)."""
    w = (G[..., 2, 1] - G[..., 1, 2], G[..., 0, 2] - G[..., 2, 0],
         G[..., 1, 0] - G[..., 0, 1])
    if torch.is_tensor(G):
        return torch.stack(w, dim=-1)
    import numpy as np
    return np.stack(w, axis=-1)


def strain_rate_from_gradient(G):
    """Symmetric part of G: E = (G + G^T) / 2."""
    if torch.is_tensor(G):
        return 0.5 * (G + G.transpose(-1, -2))
    import numpy as np
    return 0.5 * (G + np.swapaxes(G, -1, -2))


def pressure_at_targets(r_trg, eta, fiber=None, shell=None, bodies=None, backend=None):
    """Pressure (n_trg,) of velocity_at_targets' field, same dict inputs; the
    fiber self term is never subtracted."""
    return _field("pressure", r_trg, eta, backend, fiber=fiber, shell=shell, bodies=bodies)


def stress_from_fields(p, G, eta):
    """sigma (n, 3, 3) = -p I + eta (G + G^T) from the pressure (n,) and the
    velocity gradient (n, 3, 3); torch or numpy."""
    if torch.is_tensor(G):
        eye = torch.eye(3, dtype=G.dtype, device=G.device)
        return eta * (G + G.transpose(-1, -2)) - p[..., None, None] * eye
    import numpy as np
    return eta * (G + np.swapaxes(G, -1, -2)) - np.asarray(p)[..., None, None] * np.eye(3)


def stress_at_targets(r_trg, eta, fiber=None, shell=None, bodies=None, backend=None):
    """Stress (n_trg, 3, 3) of velocity_at_targets' field: the velocity
    gradient and the pressure of the same sources through stress_from_fields."""
    sources = flow_sources(fiber, shell, bodies)
    backend = backend if backend is not None else _default_backend(r_trg)
    G = evaluate(sources, "gradient", r_trg, eta, backend)
    return stress_from_fields(evaluate(sources, "pressure", r_trg, eta, backend), G, eta)


def traction(stress, normals):
    """sigma . n (n, 3): the force per area that the fluid on the side the
    normal points to exerts across the surface element."""
    if torch.is_tensor(stress):
        return torch.einsum("nij,nj->ni", stress, normals)
    import numpy as np
    return np.einsum("nij,nj->ni", stress, normals)


def surface_force_torque(points, normals, weights, stress, origin):
    """(F, T): the quadrature sum_k w_k (sigma . n)_k and
    sum_k w_k (x_k - origin) x (sigma . n)_k over a surface given by its
    points (n, 3), normals (n, 3) and quadrature weights (n,)."""
    wt = traction(stress, normals) * weights[:, None]
    if torch.is_tensor(wt):
        arm = points - torch.as_tensor(origin, dtype=points.dtype, device=points.device)
        return wt.sum(dim=0), torch.linalg.cross(arm, wt).sum(dim=0)
    import numpy as np
    arm = points - np.asarray(origin, float)
    return wt.sum(axis=0), np.cross(arm, wt).sum(axis=0)


# ---------------------------------------------------------------------------
# Streamlines: dx/dt = u(x) with u the field of velocity_at_targets (plus
# point/background sources and the rigid motion inside bodies, as the
# listener's velocity_field has them), integrated on the device by one
# persistent kernel launch for all seeds (evaluator.trace_streamlines_device).
# ---------------------------------------------------------------------------

def streamline_source_sets(eta, fiber=None, shell=None, bodies=None, sources=None, to=None,
                           flow=None):
    """The tracer's inputs: the terms of flow_sources(fiber, shell, bodies,
    sources), or of an already built `flow`, concatenated per kind:
    dict(stokeslet, stresslet, rotlet, oseen = (r_src, strength) or None,
    background, bodies = rows of (centre, radius, velocity, angular velocity)
    or None). A double layer enters as its stresslet strength.
    `to` maps each array (numpy or tensor) to the tensor to concatenate."""
    to = to or (lambda a: a)
    flow = flow if flow is not None else flow_sources(fiber, shell, bodies, sources)

    def cat(kind, strength=lambda s: s):
        parts = [(to(t[1]), strength(*map(to, t[2:]))) for t in flow.terms if t[0] == kind]
        if kind == "rotlet":  # the tracer has the body centres before the point torques
            parts.reverse()
        if not parts:
            return None
        return (torch.cat([p[0] for p in parts]).contiguous(),
                torch.cat([p[1] for p in parts]).contiguous())

    rigid = flow.bodies
    if rigid is not None:
        rigid = torch.cat([to(rigid["centers"]), to(rigid["radii"]).reshape(-1, 1),
                           to(rigid["velocities"]), to(rigid["angular_velocities"])],
                          dim=1).contiguous()
    return dict(stokeslet=cat("stokeslet"),
                stresslet=cat("double_layer", lambda n, d: double_layer_strength(n, d, eta)),
                rotlet=cat("rotlet"), oseen=cat("oseen"), background=flow.background,
                bodies=rigid)


def streamlines_at_seeds(x0, eta, fiber=None, shell=None, bodies=None, sources=None,
                         dt_init=0.1, t_final=1.0, abs_err=1e-10, rel_err=1e-6,
                         back_integrate=True, max_points=4096, backend=None, flow=None):
    """Streamlines of velocity_at_targets' field through every row of x0
    (n, 3), as StreamLine::compute (streamline.cpp:67-113) integrates them:
    adaptive Cash-Karp 5(4) from t = 0 to t_final, and to -t_final when
    back_integrate, stopping where |u| > 1e3. All seeds are traced in one
    kernel launch with the sources uploaded and packed once; the terms
    (numpy arrays or tensors) are those of streamline_source_sets.

    Returns one dict per seed, {x (m, 3), val (m, 3), time (m,), status} as
    numpy arrays (this call waits for the kernel): the joined line of
    evaluator.join_streamlines, val the velocity at its points, status 0 when
    t_final was reached both ways (else the tracer's code: 1 singularity,
    2 max_points recorded, 3 step control gave up). backend: a HipBackend
    (default: one on x0's device, cuda:0 for numpy). flow: the already built
    flow_sources.FlowSources, in place of the four dicts."""
    return _lines_at_seeds("trace_streamlines", x0, eta, fiber, shell, bodies, sources, flow,
                           backend, dt_init=dt_init, t_final=t_final, abs_err=abs_err,
                           rel_err=rel_err, back_integrate=back_integrate, max_points=max_points)


def _lines_at_seeds(trace, x0, eta, fiber, shell, bodies, sources, flow, backend, **control):
    """streamlines_at_seeds and vortexlines_at_seeds: `trace` names the
    backend's method."""
    import numpy as np
    from .evaluator import join_streamlines
    if backend is None:
        backend = _default_backend(x0)

    def to(a):
        if not torch.is_tensor(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
        return backend._t(a)

    seeds = to(x0).reshape(-1, 3)
    n = seeds.shape[0]
    if n == 0:
        return []
    sets = streamline_source_sets(eta, fiber, shell, bodies, sources, to, flow)
    out = getattr(backend, trace)(seeds, eta, **sets, **control)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    return join_streamlines(host["x"], host["t"], host["val"], host["count"], host["status"], n)


def vortexlines_at_seeds(x0, eta, fiber=None, shell=None, bodies=None, sources=None,
                         dt_init=0.1, t_final=1.0, abs_err=1e-10, rel_err=1e-6,
                         back_integrate=True, max_points=4096, backend=None, flow=None):
    """Vortex lines of the same field through every row of x0, as
    VortexLine::compute (streamline.cpp:115-165) integrates them, with the
    analytic curl of the gradient kernels in place of its finite difference:
    dx/dt = curl u, still stopping where the VELOCITY has |u| > 1e3, as the
    reference's observer does. Arguments and return as streamlines_at_seeds,
    val the vorticity at the line's points (2 w inside a body)."""
    return _lines_at_seeds("trace_vortexlines", x0, eta, fiber, shell, bodies, sources, flow,
                           backend, dt_init=dt_init, t_final=t_final, abs_err=abs_err,
                           rel_err=rel_err, back_integrate=back_integrate, max_points=max_points)


class ShellOperator:
    """HBM-resident periphery dense operators (M_inv, stresslet+complementary).

    Single-GPU: matrices are the full (3N, 3N); distributed: each rank holds
    its contiguous row block (3n_local, 3N) — the reference's row
    distribution (periphery.cpp:422-442) — and x is all-gathered per apply.
    The matrices stay resident in HBM across GMRES iterations (4.6 GB at an
    8k-node shell — trivial in 288 GB).
    """

    def __init__(self, M_inv_rows, stresslet_plus_complementary_rows, distributed=False):
        self.M_inv = M_inv_rows.contiguous()
        self.SPC = stresslet_plus_complementary_rows.contiguous()
        self.distributed = distributed
        if self.M_inv.dtype != torch.float64:
            raise TypeError("ShellOperator expects fp64")

    def _gather(self, x_local):
        if self.distributed:
            return allgather_rows(x_local.reshape(-1, 1)).reshape(-1)
        return x_local

    def apply_preconditioner(self, x_local):
        """M_inv_ @ allgather(x) (periphery.cpp:21-29)."""
        x = self._gather(x_local)
        return torch.mv(self.M_inv, x)

    def matvec(self, x_local, v_local):
        """stresslet_plus_complementary_ @ allgather(x) + v (periphery.cpp:34-47)."""
        x = self._gather(x_local)
        return torch.addmv(v_local.reshape(-1), self.SPC, x)
