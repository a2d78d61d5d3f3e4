"""System orchestrator for fiber + periphery solves — the thin host harness
around the accelerated evaluators ("host control flow; kept as
thin harness around the accelerated evaluator for configs 4-5").

Mirrors the reference solve pipeline for finite-difference fibers, a
periphery and rigid bodies (src/core/system.cpp):
  prep_state_for_solver  (system.cpp:396-459)
  apply_matvec           (system.cpp:269-324)
  apply_preconditioner   (system.cpp:248-263)
  solve / step           (system.cpp:464-493) — backward-Euler via the
                         beta_tstep/dt terms inside the fiber operator.

There is one matvec and one preconditioner: torch, tensor in and tensor out,
on the backend's device, against operators that prep leaves resident there.
The pair kernels are reached only through the backend's methods
(SystemFD._kernel): HipBackend is the product (HIP kernels on the GPU, fails
loudly without one); any object with the same methods on numpy arrays and no
device is a host backend, served on CPU tensors — the tests inject the CPU
oracle that way and run the same pipeline off-GPU.
Fibers are held as runs — maximal blocks of consecutive fibers with equal
node counts, each one batch for the fiber operators — so a uniform
population is one run and a mixed one takes the same path.

The pipeline is written once, for a rank-local view of the system: the
solution vector is [own fibers | own shell rows | body block], targets are
the local nodes, and every place the reference communicates goes through
self.comm (sharded.Comm) — fiber sources and the shell density are gathered,
the body block is taken from rank 0, link forces are summed over ranks.
SystemFD holds the single-rank communicator, for which all of these are the
identity; system_dist.DistributedSystemFD is this class with a live
communicator and the rank-local layout accessors.
"""

import numpy as np

from .sharded import Comm


class HipBackend:
    """Product backend: the pair kernels on the MI355X, on the device `dev`.
    Every method takes numpy arrays or tensors and returns the same kind:
    resident tensors in give the tensor out with no synchronization (the
    solve pipeline), numpy in gives numpy out (prep-time and post-processing
    callers). Both go through _eval, the one seam to the kernels."""

    def __init__(self, device="cuda:0"):
        import torch
        self.dev = torch.device(device)

    def _t(self, a):
        import torch
        if torch.is_tensor(a):
            return a.to(self.dev)
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _eval(self, name, arrays, *scalars, **kw):
        """evaluator.<name>_device(*arrays on the device, *scalars, **kw):
        the tensor, asynchronous, when the arrays are tensors; else as numpy
        (the copy back waits for the kernel). The function is looked up on
        each call, so tests can replace it in the module."""
        import torch
        from . import evaluator
        out = getattr(evaluator, name + "_device")(
            *[self._t(a) for a in arrays], *scalars, **kw)
        return out if torch.is_tensor(arrays[0]) else out.cpu().numpy()

    @staticmethod
    def _f_dl(normals, density, eta):
        """Shell/body double layer: f_dl = 2*eta*n (x) d, then stresslet/eta
        (periphery.cpp:68-74)."""
        import torch
        if torch.is_tensor(normals):
            from .flows import double_layer_strength
            return double_layer_strength(normals, density, eta)
        return 2.0 * eta * np.einsum("ni,nj->nij", normals, density).reshape(-1, 9)

    def stokeslet(self, r_src, f_src, r_trg, eta):
        return self._eval("stokeslet", (r_src, f_src, r_trg), eta)

    def stresslet_normal_density(self, r_src, normals, density, r_trg, eta):
        return self._eval("stresslet",
                          (r_src, self._f_dl(normals, density, eta), r_trg), eta)

    def self_stokeslet_batch(self, pts, eta):
        """(nf, n, 3) -> (nf, 3n, 3n) oseen_tensor_direct per fiber."""
        return self._eval("oseen_tensor_batched", (pts,), eta=eta)

    def rotlet(self, centers, torques, r_trg, eta):
        return self._eval("rotlet", (centers, r_trg, torques), eta)

    def oseen_contract(self, r_src, r_trg, density, eta):
        return self._eval("oseen_contract", (r_src, r_trg, density), eta)

    # velocity gradients: (n_trg, 3, 3), G[t, i, j] = du_i/dx_j

    def stokeslet_grad(self, r_src, f_src, r_trg, eta):
        return self._eval("stokeslet_grad", (r_src, f_src, r_trg), eta)

    def stresslet_normal_density_grad(self, r_src, normals, density, r_trg, eta):
        """Gradient of stresslet_normal_density's field (same f_dl)."""
        return self._eval("stresslet_grad",
                          (r_src, self._f_dl(normals, density, eta), r_trg), eta)

    def rotlet_grad(self, centers, torques, r_trg, eta):
        return self._eval("rotlet_grad", (centers, r_trg, torques), eta)

    def oseen_contract_grad(self, r_src, r_trg, density, eta):
        return self._eval("oseen_contract_grad", (r_src, r_trg, density), eta)

    # pressures: (n_trg,), prefactor 1/(4 pi); the rotlet's is zero (no method)

    def stokeslet_pressure(self, r_src, f_src, r_trg):
        return self._eval("stokeslet_pressure", (r_src, f_src, r_trg))

    def stresslet_normal_density_pressure(self, r_src, normals, density, r_trg, eta):
        """Pressure of stresslet_normal_density's field (same f_dl, which is
        where eta comes in)."""
        return self._eval("stresslet_pressure",
                          (r_src, self._f_dl(normals, density, eta), r_trg))

    def oseen_contract_pressure(self, r_src, r_trg, density):
        return self._eval("oseen_contract_pressure", (r_src, r_trg, density))

    def nearest(self, r_src, r_trg, src_group=None, trg_group=None):
        """(d2, index) of evaluator.nearest_device on this device: per target
        the nearest source whose group differs from its own (every source
        without groups). Tensors (asynchronous) when r_src is one, else numpy."""
        import torch
        from . import evaluator
        groups = [None if g is None else
                  (g.to(self.dev) if torch.is_tensor(g) else
                   torch.from_numpy(np.ascontiguousarray(g, dtype=np.int64)).to(self.dev))
                  for g in (src_group, trg_group)]
        d2, index = evaluator.nearest_device(self._t(r_src), self._t(r_trg), *groups)
        if torch.is_tensor(r_src):
            return d2, index
        return d2.cpu().numpy(), index.cpu().numpy()

    def trace_streamlines(self, seeds, eta, stokeslet=None, stresslet=None, rotlet=None,
                          oseen=None, background=None, bodies=None, **control):
        """evaluator.trace_streamlines_device on this device: the source sets
        are (r_src, strength) pairs of numpy arrays or tensors (None or zero
        rows: an empty set), `control` its step-control keywords. Returns its
        dict of per-job arrays, tensors (asynchronous) when `seeds` is one,
        else numpy."""
        return self._trace("trace_streamlines_device", seeds, eta,
                           (stokeslet, stresslet, rotlet, oseen), background, bodies, control)

    def trace_vortexlines(self, seeds, eta, stokeslet=None, stresslet=None, rotlet=None,
                          oseen=None, background=None, bodies=None, **control):
        """evaluator.trace_vortexlines_device on this device; arguments and
        return as trace_streamlines, `val` the vorticity."""
        return self._trace("trace_vortexlines_device", seeds, eta,
                           (stokeslet, stresslet, rotlet, oseen), background, bodies, control)

    def _trace(self, entry, seeds, eta, pairs, background, bodies, control):
        import torch
        from . import evaluator
        sets = [None if p is None or len(p[0]) == 0 else (self._t(p[0]), self._t(p[1]))
                for p in pairs]
        if bodies is not None:
            bodies = self._t(bodies) if len(bodies) else None
        out = getattr(evaluator, entry)(
            self._t(seeds), eta, *sets, background=background, bodies=bodies, **control)
        if torch.is_tensor(seeds):
            return out
        return {k: v.cpu().numpy() for k, v in out.items()}

    def stresslet_times_normal(self, nodes, normals, eta):
        """Dense (3n, 3n) operator (kernels.cpp:264-287; eta-independent
        factor) — the M block of the body preconditioner."""
        return self._eval("stresslet_times_normal", (nodes, normals))


class Shell:
    """Periphery state: nodes/normals (N, 3) + the dense operators
    (stresslet_plus_complementary, M_inv)."""

    def __init__(self, nodes, normals, A, M_inv):
        self.nodes = np.asarray(nodes, float)
        self.normals = np.asarray(normals, float)
        self.A = A
        self.M_inv = M_inv
        self.n_nodes = len(self.nodes)


class SystemFD:
    # single rank: every collective in the pipeline below is the identity
    comm = Comm(single=True)

    def __init__(self, fibers, eta, dt, shell=None, background_flow=None, backend=None,
                 periphery_interaction=None, bodies=None, periphery_shape=None,
                 periphery_binding=None, dynamic_instability=None, seed=130319):
        self.fibers = list(fibers)
        self.eta = float(eta)
        self.dt = float(dt)
        self.shell = shell
        self.bodies = list(bodies) if bodies is not None else []
        # periphery_shape: dict(kind=, radius=|abc=) for collision/binding
        # geometry; periphery_binding: dict(active, polar_angle_start/_end,
        # threshold) (skelly_config.py:352-372); dynamic_instability: dict
        # with skellysim_amd.instability.DEFAULTS keys (0 n_nodes = off)
        self.periphery_shape = periphery_shape
        self.periphery_binding = periphery_binding
        self.dynamic_instability = dynamic_instability
        # fiber-fiber steric repulsion (ENGINE EXTENSION, default off):
        # dict(f_0=, l_0=, d_max=) — see _fiber_fiber_repulsion
        self.steric_interaction = None
        self.rng = np.random.default_rng(seed)  # params.seed default 130319
        # point/background sources (sources.py); simulation clock for their
        # lifetimes (properties.time — advanced by run())
        self.point_sources = None
        self.background_source = None
        self.time = 0.0
        # motor forces held at zero until the clock passes this
        # (params.implicit_motor_activation_delay, system.cpp:417-419)
        self.motor_activation_delay = 0.0
        self.background_flow = background_flow  # fn: (n,3) -> (n,3)
        # steric fiber-periphery repulsion (system.cpp:421, params.cpp:18):
        # dict(kind="sphere"|"ellipsoid", f_0=, l_0=, radius=|abc=) or None.
        # ENGINE EXTENSION: kind="generic" with nodes=, normals= (default:
        # this system's shell), for both dicts — contact.py
        self.periphery_interaction = periphery_interaction
        # (n_fiber_nodes, 3) periphery force of the last prep
        self.periphery_force = None
        self.backend = backend if backend is not None else HipBackend()
        self._uniform = self._fibers_uniform()

    # ---- the seam to the backend ----------------------------------------
    @property
    def dev(self):
        """Where the pipeline's tensors live: the backend's device, or the
        CPU for a host backend (numpy methods, no `dev`)."""
        import torch
        return getattr(self.backend, "dev", torch.device("cpu"))

    def _t(self, a):
        """numpy array or tensor -> tensor on self.dev."""
        import torch
        if not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(a))
        return a.to(self.dev)

    def _kernel(self, name, *args):
        """backend.<name>(*args) for the pipeline: tensors on self.dev in,
        tensor out. A backend with a device takes them as they are and does
        not synchronize; a host backend is called with numpy views."""
        import torch
        fn = getattr(self.backend, name)
        if hasattr(self.backend, "dev"):
            return fn(*args)
        return torch.from_numpy(fn(*[np.ascontiguousarray(a.numpy())
                                     if torch.is_tensor(a) else a for a in args]))

    # ---- layout helpers -------------------------------------------------
    @property
    def fiber_node_count(self):
        return sum(f.n_nodes for f in self.fibers)

    @property
    def fiber_sol_size(self):
        return sum(4 * f.n_nodes for f in self.fibers)

    # The solution vector and the node array are RANK-LOCAL: [own fibers |
    # own shell rows | body block]. The accessors below are the whole
    # layout; a multi-rank subclass overrides them and nothing else.
    def _own_shell_nodes(self):
        """The shell nodes whose rows this rank solves for."""
        return self.shell.nodes

    @property
    def shell_sol_size(self):
        return 3 * len(self._own_shell_nodes()) if self.shell else 0

    def _own_bodies(self):
        """The bodies whose solution block lives in this rank's vector.
        (self.bodies, the geometry, is the full set on every rank.)"""
        return self.bodies

    @property
    def global_body_sol_size(self):
        return sum(b.solution_size for b in self.bodies)

    @property
    def body_sol_size(self):
        return sum(b.solution_size for b in self._own_bodies())

    @property
    def body_node_count(self):
        return sum(b.n_nodes for b in self.bodies)

    def fiber_nodes(self):
        return np.concatenate([f.x.T for f in self.fibers], axis=0) \
            if self.fibers else np.zeros((0, 3))

    def body_nodes(self):
        return np.concatenate([b.nodes for b in self.bodies], axis=0) \
            if self.bodies else np.zeros((0, 3))

    def body_normals(self):
        return np.concatenate([b.normals for b in self.bodies], axis=0) \
            if self.bodies else np.zeros((0, 3))

    def all_nodes(self):
        """The local targets, in node order [fibers | shell | bodies]
        (system.cpp:408-418)."""
        parts = [self.fiber_nodes()]
        if self.shell:
            parts.append(self._own_shell_nodes())
        if self._own_bodies():
            parts.append(self.body_nodes())
        return np.concatenate(parts, axis=0)

    def _body_sol_slices(self):
        out, off = [], self.fiber_sol_size + self.shell_sol_size
        for b in self._own_bodies():
            out.append((b, off, off + b.solution_size))
            off += b.solution_size
        return out

    def _body_node_slices(self):
        """Slices into the [fibers | shell | bodies] node array."""
        out, off = [], self.fiber_node_count + self.shell_sol_size // 3
        for b in self._own_bodies():
            out.append((b, off, off + b.n_nodes))
            off += b.n_nodes
        return out

    def _global_body_solution(self, x):
        """The body block of the solution-layout vector x, from the rank
        that holds it (rank 0) on every rank (system.cpp:309)."""
        return self.comm.from_root(
            x[self.fiber_sol_size + self.shell_sol_size:],
            self.global_body_sol_size)

    def _fiber_slices(self):
        out, off = [], 0
        for f in self.fibers:
            out.append((f, off, off + 4 * f.n_nodes))
            off += 4 * f.n_nodes
        return out

    def _fiber_node_slices(self):
        out, off = [], 0
        for f in self.fibers:
            out.append((f, off, off + f.n_nodes))
            off += f.n_nodes
        return out

    def _fibers_uniform(self):
        """All fibers share one discretization (the batched paths apply)."""
        return all(f.n_nodes == self.fibers[0].n_nodes for f in self.fibers)

    def _fiber_runs(self):
        """[i0, i1) fiber index ranges of the runs: maximal blocks of
        consecutive fibers with equal n_nodes, each batched as one."""
        runs = []
        for i, f in enumerate(self.fibers):
            if runs and self.fibers[runs[-1][0]].n_nodes == f.n_nodes:
                runs[-1][1] = i + 1
            else:
                runs.append([i, i + 1])
        return runs

    # ---- resident state and the flow stages -----------------------------
    def _build_geometry(self):
        """Start the resident state self._ops with what the flow stages
        need. It depends on positions and eta only, so prep builds it first
        and runs its own flows through the same stages as the matvec."""
        T = self._t
        d = self._ops = dict(runs=[])
        a = na = 0
        for i0, i1 in self._fiber_runs():
            fibs = self.fibers[i0:i1]
            nf, n = len(fibs), fibs[0].n_nodes
            d["runs"].append(dict(
                fibers=fibs, nf=nf, n=n,
                sol=slice(a, a + 4 * nf * n), nodes=slice(na, na + nf * n),
                # self-stokeslets built directly on device (kernels.cpp:146-195)
                G=self._kernel("self_stokeslet_batch",
                               T(np.stack([f.x.T for f in fibs])), self.eta),
                w=T(np.concatenate([f.quadrature_weights() for f in fibs]))))
            a, na = a + 4 * nf * n, na + nf * n
        d["fib_size"], d["fib_nodes"], d["sh_size"] = a, na, self.shell_sol_size
        d["r_fib"] = T(self.fiber_nodes())
        # the one solve-static gather: fiber source positions of all ranks
        d["r_fib_all"] = self.comm.gather_rows(d["r_fib"])
        d["r_all"] = T(self.all_nodes())
        if self.shell:
            d["sh_nodes"] = T(self.shell.nodes)
            d["sh_normals"] = T(self.shell.normals)
        if self.bodies:
            d["body_nodes"] = T(self.body_nodes())
            d["body_normals"] = T(self.body_normals())
            d["centers"] = T(np.stack([b.position for b in self.bodies]))

    def _fiber_flow(self, forces):
        """FiberContainerFiniteDifference::flow (f_c_fd.cpp:172-214) at the
        local nodes: quadrature-weighted stokeslet of the fiber forces,
        minus the per-fiber self term on the fiber's own nodes. forces: per
        run, (nf*n, 3) node-major. The sources are ALL ranks' fibers (the
        weighted forces gathered per apply — the reference's
        MPI_Allgatherv); the self term is this rank's fibers against their
        own wf, and their nodes lead the targets."""
        import torch
        d = self._ops
        if not len(d["r_fib_all"]):
            return torch.zeros_like(d["r_all"])
        wf = [f * r["w"][:, None] for f, r in zip(forces, d["runs"])]
        wf_all = wf[0] if len(wf) == 1 else torch.cat(wf)
        vel = self._kernel("stokeslet", d["r_fib_all"],
                           self.comm.gather_rows(wf_all), d["r_all"], self.eta)
        for r, wf_r in zip(d["runs"], wf):
            # G and wf are point-major interleaved (xyz per node), matching
            # the reference's VectorMap flattening (f_c_fd.cpp:203-210)
            vel[r["nodes"]] -= torch.bmm(
                r["G"], wf_r.reshape(r["nf"], 3 * r["n"], 1)).reshape(-1, 3)
        return vel

    def _body_flow(self, densities, forces_torques):
        """BodyContainer::flow_spherical (body_container.cpp:269-337) at the
        local nodes: double layer of ALL bodies' surface densities (n, 3) +
        center Stokeslet of the forces + center rotlet of the torques.
        forces_torques: (n_bodies, 6) from the link conditions (matvec) or
        the external forces (prep)."""
        d, eta, kernel = self._ops, self.eta, self._kernel
        v = kernel("stresslet_normal_density", d["body_nodes"],
                   d["body_normals"], densities, d["r_all"], eta)
        v += kernel("stokeslet", d["centers"],
                    forces_torques[:, 0:3].contiguous(), d["r_all"], eta)
        v += kernel("rotlet", d["centers"],
                    forces_torques[:, 3:6].contiguous(), d["r_all"], eta)
        return v

    # ---- solver pipeline ------------------------------------------------
    def prep_state_for_solver(self):
        """system.cpp:396-459."""
        dt, eta = self.dt, self.eta
        # dynamic instability runs first (system.cpp:403) and can change
        # the fiber population
        if self.dynamic_instability:
            from .instability import dynamic_instability
            dynamic_instability(self, self.dynamic_instability, self.rng)
            self._uniform = self._fibers_uniform()
        for f in self.fibers:
            f.update_constants(eta)
            f.update_derivatives()
        # periphery binding re-evaluates the plus-end BCs every prep
        # (fc_->update_boundary_conditions, system.cpp:453)
        if self.periphery_binding and self.periphery_binding.get("active"):
            # a generic shell binds nothing, as the reference's stub
            # (GenericPeriphery::check_collision, periphery.cpp:264-335)
            shape = self.periphery_shape
            if shape is not None and shape["kind"] == "generic":
                shape = None
            for f in self.fibers:
                f.update_boundary_conditions(shape, self.periphery_binding)
        if not (self._uniform and self.fibers):
            for f in self.fibers:
                f.update_linear_operator(dt, eta)
                f.update_force_operator()

        # positions, self-stokeslets (fiber_finite_difference.cpp:56) and
        # quadrature weights, resident for the flows below and in the matvec
        self._build_geometry()
        T = self._t

        r_all = self.all_nodes()
        nf_nodes = self.fiber_node_count

        # motor force (generate_constant_force, f_c_fd.cpp:160-169); held
        # at zero until the activation delay passes (system.cpp:417-419)
        motor = np.zeros((nf_nodes, 3))
        if not (self.motor_activation_delay > self.time):
            for f, a, b in self._fiber_node_slices():
                motor[a:b] = (f.force_scale * f.xs).T

        # fiber-periphery steric repulsion (fc_->periphery_force,
        # system.cpp:421; per-fiber force periphery.cpp:140-162,232-263)
        ext = np.zeros((nf_nodes, 3))
        if self.periphery_interaction is not None:
            pi = self.periphery_interaction
            if pi["kind"] == "generic":
                # ENGINE EXTENSION: every fiber node against the shell's
                # nodes in one nearest-source launch (contact.py)
                if nf_nodes:
                    ext[:] = self._generic_periphery_force(pi)
            else:
                for f, a, b in self._fiber_node_slices():
                    ext[a:b] = f.periphery_repulsion(**pi).T
        # what the periphery alone exerts, for inspection
        self.periphery_force = ext.copy()
        # fiber-fiber steric repulsion (ENGINE EXTENSION, opt-in; see
        # _fiber_fiber_repulsion)
        if self.steric_interaction is not None and nf_nodes:
            ext += self._fiber_fiber_repulsion(**self.steric_interaction)

        # v_all: flow induced by the external (periphery) forces
        # (fc_->flow(r_all, external_force_fibers), system.cpp:425)
        # + background flow; motor forces enter only the RHS
        v_all = np.zeros_like(r_all)
        if nf_nodes and (self.periphery_interaction is not None
                         or self.steric_interaction is not None):
            ext_t = T(ext)
            v_all += self._fiber_flow(
                [ext_t[r["nodes"]] for r in self._ops["runs"]]).cpu().numpy()
        if self.background_flow is not None:
            v_all += self.background_flow(r_all)
        # point + background sources (psc_.flow / bs_.flow, system.cpp:445-446)
        if self.point_sources is not None:
            v_all += self.point_sources.flow(r_all, eta, self.time,
                                             self.backend)
        if self.background_source is not None and \
                self.background_source.is_active():
            v_all += self.background_source.flow(r_all, eta)

        # body caches + external body force/torque flow (system.cpp:427-443)
        if self.bodies:
            for b in self.bodies:
                b.update_cache(eta, self.backend)
            ext_ft = np.stack([np.concatenate([b.external_force_at(self.time),
                                               b.external_torque])
                               for b in self.bodies])
            if np.any(ext_ft):
                # zero densities on every body's nodes: the flow's sources
                # are all the bodies, whichever rank holds their block
                v_all += self._body_flow(
                    T(np.zeros((self.body_node_count, 3))),
                    T(ext_ft)).cpu().numpy()

        motor = motor + ext  # total_force_fibers (system.cpp:450)
        v_fib = v_all[:nf_nodes]
        assembled = None
        if self._uniform and self.fibers:
            # batched assembly (operator + RHS + BCs + force operator) —
            # numerically identical to the per-fiber loop (fiber_batch.py)
            from .fiber_batch import assemble_uniform, install_operators
            n = self.fibers[0].n_nodes
            nf = len(self.fibers)
            flow_b = v_fib.reshape(nf, n, 3).transpose(0, 2, 1)
            motor_b = motor.reshape(nf, n, 3).transpose(0, 2, 1)
            ext_b = ext.reshape(nf, n, 3).transpose(0, 2, 1) \
                if self.periphery_interaction is not None else None
            # assemble on the backend's device (the dominant prep cost) and
            # keep the resident tensors for _build_operators; the fibers
            # get host copies, as from the per-fiber methods
            A_t, RHS_t, F_t = assemble_uniform(
                self.fibers, dt, eta, flow=flow_b, f_external=motor_b,
                bc_force=ext_b, device=self.dev)
            install_operators(self.fibers, A_t.cpu().numpy(),
                              RHS_t.cpu().numpy(), F_t.cpu().numpy())
            assembled = (A_t, F_t)
        else:
            for f, a, b in self._fiber_node_slices():
                f.update_RHS(dt, v_fib[a:b].T, motor[a:b].T)
                f.apply_bc_rectangular(dt, v_fib[a:b].T, ext[a:b].T
                                       if self.periphery_interaction is not None
                                       else None)

        self._build_operators(assembled)

        rhs_parts = [f.RHS for f in self.fibers]
        sh_nodes = self.shell_sol_size // 3
        if self.shell:
            v_shell = v_all[nf_nodes: nf_nodes + sh_nodes]
            rhs_parts.append(-v_shell.reshape(-1))  # update_RHS, periphery.cpp:86
        for b, a, bb in self._body_node_slices():
            rhs_parts.append(b.update_RHS(v_all[a:bb]))
        self.RHS = np.concatenate(rhs_parts) if rhs_parts else np.zeros(0)
        return self.RHS

    def _build_operators(self, assembled=None):
        """Complete self._ops with the operators of the assembled state, so
        a whole GMRES iteration (matvec + preconditioner) runs on the
        backend's device with no host traffic. assembled: the (A, F)
        tensors of a uniform population's batched assembly, adopted as its
        one run; otherwise each run stacks its fibers' operators."""
        import torch
        from .batched import BatchedLU
        T, dev = self._t, self.dev
        d = self._ops
        for r in d["runs"]:
            fibs, m = r["fibers"], r["fibers"][0].mats
            r["A"], r["F"] = assembled if assembled is not None else (
                T(np.stack([f.A for f in fibs])),
                T(np.stack([f.force_operator for f in fibs])))
            r["lu"] = BatchedLU(r["A"])
            r["xs"] = T(np.stack([f.xs for f in fibs]))              # (nf, 3, n)
            # the tension row's D_1 is D_1_0 * 2/length_prev, each fiber's
            # own (fiber_fd.matvec); the factor rides on a copy of xs
            r["xs_D1"] = r["xs"] * T(np.array(
                [2.0 / f.length_prev for f in fibs]))[:, None, None]
            r["D1T"] = T(m["D_1_0"].T)
            r["P_ds"] = T(m["P_downsample_bc"])                      # (4n-14, 4n)
            r["plus_vel"] = T(np.array(
                [1.0 if f.bc_plus[0] == "Velocity" else 0.0 for f in fibs]))
            # fiber<->body link statics (body.py) of the attached fibers
            att = [i for i, f in enumerate(fibs) if f.binding_site[0] >= 0] \
                if self.bodies else []
            r["att"] = None
            if att:
                fa = [fibs[i] for i in att]
                site = np.stack(
                    [self.bodies[ib].nucleation_sites[js] - self.bodies[ib].position
                     for ib, js in (f.binding_site for f in fa)])
                col = lambda vals: T(np.array(vals))[:, None]
                r["att"] = dict(
                    idx=torch.tensor(att, dtype=torch.long, device=dev),
                    body=torch.tensor([f.binding_site[0] for f in fa],
                                      dtype=torch.long, device=dev),
                    site=T(site),
                    site_hat=T(site / np.linalg.norm(site, axis=1, keepdims=True)),
                    xs0=T(np.stack([f.xs[:, 0] for f in fa])),
                    d2c0=T(m["D_2_0"][:, 0]), d3c0=T(m["D_3_0"][:, 0]),
                    E=col([f.bending_rigidity for f in fa]),
                    s2=col([(2.0 / f.length) ** 2 for f in fa]),
                    s3=col([(2.0 / f.length) ** 3 for f in fa]))
        if self.shell:
            # transposed copies: rocBLAS dgemv's reduction (trans) path is
            # ~1.5x the axpy path on these square operators (measured
            # 0.96 vs 1.43 ms at 24576^2, tools/prof_iter.py), so store
            # X^T contiguous and apply as mv(X_T.t(), v). HBM cost is one
            # extra copy of each operator — trivial in 288 GB. A rank's
            # (3n_local, 3N) row block takes the same form. Kept on the
            # shell, per device, across preps.
            cache = self.shell.__dict__.setdefault("_transposed", {})
            if dev not in cache:
                cache[dev] = tuple(T(X).t().contiguous()
                                   for X in (self.shell.A, self.shell.M_inv))
            d["sh_A_T"], d["sh_Minv_T"] = cache[dev]
        if self.bodies:
            # [densities | U, w] offsets of every body in the global block
            d["body_offsets"] = np.cumsum(
                [0] + [b.solution_size for b in self.bodies])[:-1].tolist()
            # BatchedLU(batch of 1) so the per-iteration solves take the
            # trsm path — magma's lu_solve corrupts under deep stream
            # queues (profiles/cadence_matrix_r02.md) and the
            # preconditioner runs at sync cadence 8 by default
            d["bodies"] = [dict(n=b.n_nodes, e=T(np.stack(b.e_sub)),  # (3, n, 3)
                                w=T(b.weights), K=T(b.K),
                                lu=BatchedLU(T(b._A_dense)[None]))
                           for b in self._own_bodies()]

    def _link_conditions(self, r, x_run, body_vels, body_ft):
        """Fiber<->body link conditions of one run's attached fibers
        (body_container.cpp:171-268; body.calculate_link_conditions is the
        per-fiber statement). Adds the force and torque they exert on their
        bodies into body_ft (n_bodies, 6); returns the run's (nf, 7)
        v_boundary rows, zero for unattached fibers."""
        import torch
        at, n = r["att"], r["n"]
        xa = x_run[at["idx"]]
        x_new = xa[:, : 3 * n].reshape(-1, 3, n)
        T0 = xa[:, 3 * n, None]
        xss0 = torch.einsum("ain,n->ai", x_new, at["d2c0"]) * at["s2"]
        xsss0 = torch.einsum("ain,n->ai", x_new, at["d3c0"]) * at["s3"]
        xs0, E, site = at["xs0"], at["E"], at["site"]
        F_b = -E * xsss0 + xs0 * T0
        L_b = (-E * torch.cross(site, xsss0, dim=1)
               + torch.cross(site, xs0, dim=1) * T0
               + E * torch.cross(xs0, xss0, dim=1))
        body_ft.index_add_(0, at["body"], torch.cat([F_b, L_b], dim=1))
        U_att = body_vels[at["body"], 0:3]
        w_att = body_vels[at["body"], 3:6]
        v_f = -U_att - torch.cross(w_att, site, dim=1)
        tc = -(xs0 * U_att).sum(dim=1) \
            + (torch.cross(xs0, site, dim=1) * w_att).sum(dim=1)
        w_f = torch.cross(at["site_hat"], w_att, dim=1)
        vel7 = x_run.new_zeros((r["nf"], 7))
        vel7[at["idx"]] = torch.cat([v_f, tc[:, None], w_f], dim=1)
        return vel7

    def apply_matvec(self, x):
        """system.cpp:269-324 (fibers + shell + bodies), x and the result
        fp64 tensors on the backend's device in the solution layout: all
        ranks' sources, this rank's targets (node order [fib | shell |
        body]) and rows. Per apply, wf and the shell density are gathered
        (RCCL over xGMI on GPUs), the body block is taken from rank 0 and
        the link forces are summed."""
        import torch
        d, eta, kernel = self._ops, self.eta, self._kernel
        runs = d["runs"]
        nf_nodes = d["fib_nodes"]  # LOCAL fiber nodes (targets)
        sh = slice(d["fib_size"], d["fib_size"] + d["sh_size"])
        body_node0 = nf_nodes + d["sh_size"] // 3
        x_runs = [x[r["sol"]].reshape(r["nf"], 4 * r["n"]) for r in runs]

        # forces: F @ x (component-major) -> node-major (nf*n, 3)
        v_all = self._fiber_flow(
            [torch.bmm(r["F"], xr.unsqueeze(-1)).reshape(r["nf"], 3, r["n"])
             .permute(0, 2, 1).reshape(-1, 3) for r, xr in zip(runs, x_runs)])

        if self.shell:
            # the GLOBAL density (periphery.cpp:26,44 Allgatherv); its
            # double layer flows to fibers AND bodies, not to the shell
            # itself (system.cpp:302-305,314-316)
            dens = self.comm.gather_rows(x[sh].reshape(-1, 3))
            if nf_nodes:
                v_all[:nf_nodes] += kernel(
                    "stresslet_normal_density", d["sh_nodes"], d["sh_normals"],
                    dens, d["r_fib"], eta)
            if self._own_bodies():
                v_all[body_node0:] += kernel(
                    "stresslet_normal_density", d["sh_nodes"], d["sh_normals"],
                    dens, d["body_nodes"], eta)

        vel7 = [None] * len(runs)
        if self.bodies:
            # Bodies follow the reference's ownership model: the geometry
            # is replicated on every rank, the solution block lives in
            # rank 0's vector and is broadcast per apply
            # (body_container.hpp:99, system.cpp:309), and the link forces
            # each rank computes from its own fibers are summed
            # (body_container.cpp:131)
            x_bodies = self._global_body_solution(x)
            dens_b = torch.cat([x_bodies[o: o + 3 * b.n_nodes].reshape(-1, 3)
                                for o, b in zip(d["body_offsets"], self.bodies)])
            body_vels = torch.stack([x_bodies[o + 3 * b.n_nodes: o + b.solution_size]
                                     for o, b in zip(d["body_offsets"], self.bodies)])
            body_ft = torch.zeros_like(body_vels)
            for k, (r, xr) in enumerate(zip(runs, x_runs)):
                if r["att"] is not None:
                    vel7[k] = self._link_conditions(r, xr, body_vels, body_ft)
            v_all += self._body_flow(dens_b, self.comm.sum(body_ft))

        res = torch.empty_like(x)
        for r, xr, v7 in zip(runs, x_runs, vel7):
            res[r["sol"]] = self._fiber_block(r, xr, v_all[r["nodes"]],
                                              v7).reshape(-1)
        if self.shell:
            # own rows of the dense operator against the global density
            # (row-distributed dense ops, periphery.cpp:34-47)
            v_shell = v_all[nf_nodes: body_node0].reshape(-1)
            res[sh] = torch.addmv(v_shell, d["sh_A_T"].t(), dens.reshape(-1))
        off, node = sh.stop, body_node0
        for bd in d.get("bodies", ()):
            # body_spherical.cpp:39-62 (body.SphericalBody.matvec)
            nn = bd["n"]
            xb = x[off: off + 3 * nn + 6]
            dloc, U = xb[: 3 * nn].reshape(nn, 3), xb[3 * nn:]
            sub = (dloc[:, 0:1] * bd["e"][0] + dloc[:, 1:2] * bd["e"][1]
                   + dloc[:, 2:3] * bd["e"][2]) / bd["w"][:, None]
            res[off: off + 3 * nn] = \
                (-sub + v_all[node: node + nn]).reshape(-1) - bd["K"] @ U
            res[off + 3 * nn: off + 3 * nn + 6] = -bd["K"].T @ xb[: 3 * nn] + U
            off, node = off + 3 * nn + 6, node + nn
        return res

    def _fiber_block(self, r, x_run, v_nodes, vel7=None):
        """One run's fiber operator block: A x - vT_in + the two BC velocity
        corrections (fiber_fd.matvec, fiber_finite_difference.cpp:278-315),
        plus the y_BC link-condition rows when vel7 (nf, 7) is given
        (fiber matvec's v_boundary, f_c_fd.cpp:226).
        x_run (nf, 4n), v_nodes (nf*n, 3) node-major -> (nf, 4n)."""
        import torch
        nf, n = r["nf"], r["n"]
        v_fib = v_nodes.reshape(nf, n, 3).permute(0, 2, 1)           # (nf, 3, n)
        vT = torch.zeros((nf, 4 * n), dtype=x_run.dtype, device=x_run.device)
        vT[:, : 3 * n] = v_fib.reshape(nf, 3 * n)
        tens = torch.einsum("ts,fis->fit", r["D1T"],
                            r["xs_D1"] * v_fib).sum(dim=1)
        vT[:, 3 * n:] = tens
        vT_in = torch.zeros_like(vT)
        vT_in[:, : 4 * n - 14] = vT @ r["P_ds"].T
        res_fib = torch.bmm(r["A"], x_run.unsqueeze(-1)).squeeze(-1) - vT_in
        bc_start = 4 * n - 14
        res_fib[:, bc_start + 3] += (v_fib[:, :, 0] * r["xs"][:, :, 0]).sum(dim=1)
        res_fib[:, bc_start + 10] += r["plus_vel"] * \
            (v_fib[:, :, -1] * r["xs"][:, :, -1]).sum(dim=1)
        if vel7 is not None:
            res_fib[:, bc_start: bc_start + 7] += vel7
        return res_fib

    def apply_preconditioner(self, x):
        """system.cpp:248-263, tensor in and out like apply_matvec: one
        batched LU solve per run, own rows of M_inv against the global
        shell vector, one dense LU solve per body."""
        import torch
        d = self._ops
        res = torch.empty_like(x)
        for r in d["runs"]:
            res[r["sol"]] = r["lu"].solve(
                x[r["sol"]].reshape(r["nf"], 4 * r["n"])).reshape(-1)
        off = d["fib_size"] + d["sh_size"]
        if self.shell:
            res[d["fib_size"]: off] = torch.mv(
                d["sh_Minv_T"].t(),
                self.comm.gather_rows(x[d["fib_size"]: off].reshape(-1, 3)).reshape(-1))
        for bd in d.get("bodies", ()):
            m = 3 * bd["n"] + 6
            res[off: off + m] = bd["lu"].solve(x[off: off + m].unsqueeze(0)).squeeze(0)
            off += m
        return res

    def solve(self, tol=1e-10, maxiter=200, restart=None, warm_start=None):
        """system.cpp:464-478 via the engine GMRES (right-preconditioned,
        ICGS — solver_hydro.cpp:64-87). The whole iteration runs on the
        backend's device, body blocks included.

        warm_start=True seeds GMRES with the PREVIOUS timestep's solution
        (the state changes O(dt) per step, so the initial residual starts
        small) — an engine capability beyond the reference, which
        constructs a zero-initialized Tpetra X_ every solve
        (include/solver.hpp:25). Default off (reference semantics;
        SKELLY_WARM_START=1 flips it): the converged answer agrees to the
        GMRES tolerance either way, but iterate-level trajectories differ,
        so the reference-pinned regression tests keep cold starts."""
        import torch
        from .gmres import gmres

        rhs = self.prep_state_for_solver()
        if restart is None:
            restart = min(200, maxiter)
        if warm_start is None:
            import os
            warm_start = os.environ.get("SKELLY_WARM_START", "0") == "1"
        prev = getattr(self, "solution", None)
        x0 = self._t(prev) if (warm_start and prev is not None
                                       and prev.shape == rhs.shape) else None
        b = self._t(rhs)
        # rank-local slices of a block-row-distributed vector: the GMRES
        # dots and norms reduce over ranks (the Tpetra/Belos dots)
        x, info = gmres(self.apply_matvec, b, precond=self.apply_preconditioner,
                        tol=tol, maxiter=maxiter, restart=restart, x0=x0,
                        distributed=self.comm.world > 1)
        if b.is_cuda:
            torch.cuda.synchronize()
        self.solution = x.cpu().numpy()
        return info

    def step(self, tol=1e-10, maxiter=200, restart=None):
        """system.cpp:482-493: solve then adopt positions, then repin
        body-attached fibers to their (moved) nucleation sites
        (FiberContainerFiniteDifference::repin_to_bodies,
        fiber_container_finite_difference.cpp:308-316 via system.cpp:488).
        Fibers adopt locally; bodies adopt on EVERY rank from rank 0's
        solution block (bc step Bcast, body_container.cpp:49-60) so the
        replicated geometry stays consistent, and each rank repins its own
        fibers."""
        info = self.solve(tol=tol, maxiter=maxiter, restart=restart)
        for f, a, b in self._fiber_slices():
            f.step(self.solution[a:b])
        if self.bodies:
            x_bodies, off = self._global_body_solution(self.solution), 0
            for b in self.bodies:
                b.step(self.dt, x_bodies[off: off + b.solution_size])
                off += b.solution_size
        self.repin_to_bodies()
        return info

    def _fiber_fiber_repulsion(self, f_0=20.0, l_0=0.05, d_max=None,
                               fiber_radius=0.0125):
        """Pairwise fiber-fiber steric repulsion — an ENGINE EXTENSION,
        default OFF (set system.steric_interaction = dict(f_0=, l_0=,
        d_max=)). The reference implements steric interaction only
        against the periphery (periphery.cpp:140-162); at its own dense
        oocyte packing (examples/oocyte, ~0.1 fiber spacing) near-contact
        fiber pairs develop quadrature-singular velocities that reject
        timesteps at any dt (profiles/oocyte_r02.md). This applies the
        SAME exponential force law pairwise between nodes of different
        fibers: f = f_0 * exp(-gap/l_0) * unit(dx), equal and opposite,
        gap = center distance - 2*fiber_radius (clamped >= 0), cutoff
        d_max (default 5*l_0 + 2*fiber_radius)."""
        from scipy.spatial import cKDTree
        if self.comm.world > 1:
            raise NotImplementedError(
                "fiber-fiber steric repulsion needs a global neighbor "
                "search; not wired into the distributed prep yet")
        pts = self.fiber_nodes()
        out = np.zeros_like(pts)
        if d_max is None:
            d_max = 5.0 * l_0 + 2.0 * fiber_radius
        fid = np.concatenate([np.full(f.n_nodes, i)
                              for i, f in enumerate(self.fibers)])
        pairs = cKDTree(pts).query_pairs(r=d_max, output_type="ndarray")
        if len(pairs) == 0:
            return out
        i, j = pairs[:, 0], pairs[:, 1]
        keep = fid[i] != fid[j]
        i, j = i[keep], j[keep]
        if len(i) == 0:
            return out
        dx = pts[i] - pts[j]
        d = np.linalg.norm(dx, axis=1)
        pos = d > 0
        i, j, dx, d = i[pos], j[pos], dx[pos], d[pos]
        gap = np.maximum(d - 2.0 * fiber_radius, 0.0)
        mag = f_0 * np.exp(-gap / l_0) / d
        fvec = mag[:, None] * dx
        np.add.at(out, i, fvec)
        np.add.at(out, j, -fvec)
        return out

    # ---- generic-periphery contact (ENGINE EXTENSION, contact.py) --------
    def _generic_shell(self, spec):
        """(nodes, normals) of a kind="generic" periphery dict: its own
        nodes= / normals=, by default the system's shell."""
        nodes, normals = spec.get("nodes"), spec.get("normals")
        if nodes is None or normals is None:
            if self.shell is None:
                raise ValueError('periphery kind "generic" needs nodes= and '
                                 "normals=, or a system with a shell")
            nodes, normals = self.shell.nodes, self.shell.normals
        return nodes, normals

    def _free_fiber_nodes(self):
        """Mask over fiber_nodes() of the nodes that take part in periphery
        contact: all but node 0 of minus-clamped fibers (periphery.cpp:148,
        f_c_fd.cpp:39-55)."""
        free = np.ones(self.fiber_node_count, dtype=bool)
        for f, a, _ in self._fiber_node_slices():
            if f.minus_clamped:
                free[a] = False
        return free

    def _generic_periphery_force(self, pi):
        """(n_fiber_nodes, 3) force of a generic shell on all fiber nodes, one
        launch; node 0 of minus-clamped fibers gets none, as in the other
        kinds."""
        from .contact import generic_periphery_force
        nodes, normals = self._generic_shell(pi)
        f = generic_periphery_force(self.fiber_nodes(), nodes, normals,
                                    pi.get("f_0", 20.0), pi.get("l_0", 0.05),
                                    self.backend)
        f[~self._free_fiber_nodes()] = 0.0
        return f

    def _generic_collision(self, shape, threshold):
        """check_collision against a generic shell: the fiber nodes (without
        node 0 of minus-clamped fibers) and the centres of the spherical
        bodies in one launch. A node collides when gap <= threshold, a
        spherical body when gap(centre) - R_body <= threshold (the generic
        counterpart of periphery.cpp:94-97); ellipsoidal bodies are a no-op
        as in the other kinds."""
        from .contact import shell_gap
        from .body import EllipsoidalBody
        nodes, normals = self._generic_shell(shape)
        pts = self.fiber_nodes()[self._free_fiber_nodes()]
        spheres = [b for b in self.bodies if not isinstance(b, EllipsoidalBody)]
        margin = np.concatenate([np.zeros(len(pts)),
                                 np.array([b.radius for b in spheres], dtype=float)])
        if not len(margin):
            return False
        centres = np.array([b.position for b in spheres], dtype=float).reshape(-1, 3)
        gap, _ = shell_gap(np.concatenate([pts, centres]), nodes, normals, self.backend)
        return bool(np.any(gap - margin <= threshold))

    def min_fiber_gap(self):
        """(distance, (fiber_i, node_i), (fiber_j, node_j)): the closest pair
        of nodes on two different fibers, from one grouped nearest-source
        launch over all fiber nodes (group = fiber). A diagnostic: no force
        depends on it. (inf, None, None) with fewer than two fibers."""
        from .contact import min_group_gap
        fid = np.concatenate([np.full(f.n_nodes, i, dtype=np.int64)
                              for i, f in enumerate(self.fibers)]) \
            if self.fibers else np.zeros(0, dtype=np.int64)
        d, i, j = min_group_gap(self.fiber_nodes(), fid, self.backend)
        if i < 0:
            return d, None, None
        start = np.cumsum([0] + [f.n_nodes for f in self.fibers])
        where = lambda k: (int(fid[k]), int(k - start[fid[k]]))
        return d, where(i), where(j)

    def repin_to_bodies(self):
        """Translate every body-attached fiber so its minus end coincides
        with the body's nucleation site again — fiber and body do not move
        exactly together under finite dt
        (fiber_container_finite_difference.cpp:308-316)."""
        for f in self.fibers:
            ib, js = getattr(f, "binding_site", (-1, -1))
            if ib >= 0:
                delta = self.bodies[ib].nucleation_sites[js] - f.x[:, 0]
                f.x += delta[:, None]

    # ---- adaptive time-stepping driver (System::run, system.cpp:516-570) --
    def fiber_error(self):
        """max | |x_s| - 1 | over all fiber nodes
        (FiberContainerFiniteDifference::fiber_error_local, f_c_fd.cpp:79-89)."""
        err = 0.0
        for f in self.fibers:
            m = f.mats
            xs = (2.0 / f.length) * f.x @ m["D_1_0"]
            err = max(err, float(np.abs(np.linalg.norm(xs, axis=0) - 1.0).max()))
        return err

    def check_collision(self, periphery_shape=None, threshold=0.0):
        """System::check_collision (system.cpp:576-595): fiber-periphery
        (f_c_fd.cpp:39-55; minus-clamped fibers skip node 0),
        body-periphery (spherical shell only: |pos| + R > R_shell -
        threshold, periphery.cpp:94-97; ellipsoidal shells are stubbed in
        the reference) and body-body pairs. periphery_shape: dict like
        periphery_interaction."""
        from .fiber_fd import points_collide
        from .body import EllipsoidalBody
        if periphery_shape is not None and periphery_shape["kind"] == "generic":
            if self._generic_collision(periphery_shape, threshold):
                return True
        elif periphery_shape is not None:
            for f in self.fibers:
                pc = f.x[:, 1:] if f.minus_clamped else f.x
                if points_collide(pc, periphery_shape, threshold):
                    return True
            if periphery_shape["kind"] == "sphere":
                for b in self.bodies:
                    if np.linalg.norm(b.position) + b.radius > \
                            periphery_shape["radius"] - threshold:
                        return True
        for i, b1 in enumerate(self.bodies):
            for b2 in self.bodies[i + 1:]:
                # any ellipsoid pairing is stubbed False in the reference
                # (body_spherical.cpp:328-331, body_ellipsoidal.cpp)
                if isinstance(b1, EllipsoidalBody) or \
                        isinstance(b2, EllipsoidalBody):
                    continue
                if b1.check_collision(b2, threshold):
                    return True
        return False

    def backup(self):
        """System::backup (system.cpp:495-505)."""
        self._bak = [(f.x.copy(), f.tension.copy()) for f in self.fibers]
        self._bak_bodies = [(b.position.copy(), b.orientation.copy(),
                             b.solution_vec.copy()) for b in self.bodies]

    def restore(self):
        for f, (x, t) in zip(self.fibers, self._bak):
            f.x = x
            f.tension = t
        for b, (p, q, s) in zip(self.bodies, self._bak_bodies):
            b.place(p, q)
            b.solution_vec = s

    def run(self, t_final, adaptive=True, dt_min=1e-4, dt_max=None,
            beta_up=1.2, beta_down=0.5, fiber_error_tol=0.1,
            periphery_shape=None, tol=1e-10, maxiter=300, restart=None,
            on_accept=None):
        """The reference timestep loop, replicated EXACTLY
        (System::run, system.cpp:516-570): backup -> step -> accept if
        converged and fiber error within tolerance (grow dt when comfortably
        inside, params.cpp:9-10 defaults beta_up=1.2, beta_down=0.5),
        reject+restore+shrink otherwise; abort below dt_min; collision
        rejects with dt/2. Including the reference's time accounting quirk:
        properties.dt is updated to dt_new BEFORE time advances
        (system.cpp:554-558), so an accepted step advances the clock by the
        NEW dt although the state moved by the old one — kept verbatim so
        the reference's pinned end-to-end tests (e.g. the clamped-buckling
        peak values) reproduce. on_accept(system, time) is the
        trajectory-write hook (fires on every accepted step; callers apply
        the reference's dt_write crossing test, system.cpp:560-561)."""
        dt_max = dt_max if dt_max is not None else self.dt
        history = []
        while self.time < t_final:
            self.backup()
            info = self.step(tol=tol, maxiter=maxiter, restart=restart)
            err = self.fiber_error()
            dt_new = self.dt
            accept = not adaptive
            if adaptive:
                if info["converged"] and err <= fiber_error_tol:
                    accept = True
                    if err <= 0.9 * fiber_error_tol:
                        dt_new = min(dt_max, self.dt * beta_up)
                else:
                    dt_new = self.dt * beta_down
                    accept = False
                if info["converged"] and self.check_collision(periphery_shape):
                    dt_new = self.dt * 0.5
                    accept = False
                if dt_new < dt_min:
                    raise RuntimeError("Timestep smaller than dt_min")
                self.dt = dt_new  # BEFORE the clock advance (system.cpp:554)
            if accept:
                self.time += self.dt
                history.append(dict(time=self.time, dt=self.dt,
                                    iters=info["iters"], fiber_error=err))
                if on_accept is not None:
                    on_accept(self, self.time)
            else:
                self.restore()
        return history
