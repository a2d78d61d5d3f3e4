"""Batched (vectorized-over-fibers) assembly of the finite-difference fiber
operators for UNIFORM discretizations — the same formulas as the per-fiber
methods in fiber_fd.py (fiber_finite_difference.cpp citations there), but
each of the 16 operator blocks, the RHS, the force operator and the
boundary-condition rows is one broadcasted torch expression over the whole
fiber population, and the BC downsample is one batched GEMM. The one
assembly runs on whatever device it is given: the GPU in the product (the
per-timestep assembly is the dominant host cost of the solve prep), the CPU
under the oracle backends. The per-fiber path is its independent statement
and its oracle (tests/test_fiber_fd.py, tests/test_gpu_fiber_assembly.py).
"""

import numpy as np
import torch

from .fiber_fd import BC_VELOCITY


def assemble_uniform(fibers, dt, eta, flow=None, f_external=None,
                     bc_force=None, device=None):
    """update_linear_operator + update_RHS + update_force_operator +
    apply_bc_rectangular for a uniform-fiber population.
    flow/f_external/bc_force: (nf, 3, n) numpy arrays or None (bc_force is
    the f_on_fiber the reference passes to apply_bcs — the EXTERNAL forces
    only, system.cpp:453). Returns (A, RHS, F) fp64 tensors on `device`
    (None: the CPU); installs nothing on the fibers (install_operators)."""
    nf = len(fibers)
    f0 = fibers[0]
    n = f0.n_nodes
    m = f0.mats
    for f in fibers:
        if f.n_nodes != n:
            raise ValueError("assemble_uniform requires uniform n_nodes")
    dev = torch.device(device if device is not None else "cpu")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, float))).to(dev)
    ar = torch.arange(n, device=dev)

    # per-fiber scalars (broadcast shapes (nf, 1, 1) / (nf, 1))
    c0 = T([f.c0 for f in fibers])[:, None, None]
    c1 = T([f.c1 for f in fibers])[:, None, None]
    E = T([f.bending_rigidity for f in fibers])[:, None, None]
    beta_dt = T([f.beta_tstep for f in fibers])[:, None, None] / dt
    pen = T([f.penalty_param for f in fibers])[:, None, None]
    L = T([f.length for f in fibers])

    # shared derivative matrices scaled per fiber (uniform length in the
    # configs, but keep the general per-fiber scale)
    s = (2.0 / L)[:, None, None]
    D1 = s * T(m["D_1_0"].T)[None]
    D2 = s ** 2 * T(m["D_2_0"].T)[None]
    D3 = s ** 3 * T(m["D_3_0"].T)[None]
    D4 = s ** 4 * T(m["D_4_0"].T)[None]
    D1pre = D1.transpose(1, 2)

    xs = T(np.stack([f.xs for f in fibers]))       # (nf, 3, n)
    xss = T(np.stack([f.xss for f in fibers]))
    xsss = T(np.stack([f.xsss for f in fibers]))
    x = T(np.stack([f.x for f in fibers]))

    I = torch.eye(n, dtype=torch.float64, device=dev)[None]
    A = torch.zeros((nf, 4 * n, 4 * n), dtype=torch.float64, device=dev)

    def seg(i):
        return slice(i * n, (i + 1) * n)

    def blk(i, j):
        return (slice(None), seg(i), seg(j))

    for i in range(3):
        for j in range(3):
            if i == j:
                A[blk(i, i)] = (beta_dt * I
                                + E * c0 * ((1.0 + xs[:, i] ** 2)[:, :, None] * D4)
                                + E * c1 * ((1.0 - xs[:, i] ** 2)[:, :, None] * D4))
            elif j > i:
                A[blk(i, j)] = E * (c0 - c1) * ((xs[:, i] * xs[:, j])[:, :, None] * D4)
            else:
                A[blk(i, j)] = A[blk(j, i)]
        AiT = -(2.0 * c0) * (xs[:, i][:, :, None] * D1)
        AiT[:, ar, ar] -= (c0[:, :, 0] + c1[:, :, 0]) * xss[:, i]
        A[blk(i, 3)] = AiT
        A[blk(3, i)] = (-(c1 + 7.0 * c0) * E * (xss[:, i][:, :, None] * D4)
                        - 6.0 * c0 * E * (xsss[:, i][:, :, None] * D3)
                        - pen * (xs[:, i][:, :, None] * D1))
    ATT = -2.0 * c0 * D2
    ATT[:, ar, ar] += (c0[:, :, 0] + c1[:, :, 0]) * \
        (xss[:, 0] ** 2 + xss[:, 1] ** 2 + xss[:, 2] ** 2)
    A[blk(3, 3)] = ATT

    # ---- RHS (update_RHS) ----
    alpha = T(m["alpha"])
    vg = T([f.v_growth for f in fibers])[:, None]
    s_dot = (1.0 + alpha)[None] * (0.5 * vg)
    RHS = torch.zeros((nf, 4 * n), dtype=torch.float64, device=dev)
    von = T(flow) if flow is not None else None  # v_on_fiber (prep passes it)
    fe = T(f_external) if f_external is not None else None
    fon = T(bc_force) if bc_force is not None else None
    for i in range(3):
        RHS[:, seg(i)] = x[:, i] / dt + s_dot * xs[:, i]
    RHS[:, 3 * n:] = -pen[:, :, 0]
    if von is not None:
        fD = torch.einsum("fin,fnm->fim", von, D1pre)
        for i in range(3):
            RHS[:, seg(i)] += von[:, i]
        RHS[:, 3 * n:] += (xs * fD).sum(dim=1)
    if fe is not None:
        fs = torch.einsum("fin,fnm->fim", fe, D1pre)
        for i in range(3):
            acc = torch.zeros((nf, n), dtype=torch.float64, device=dev)
            for j in range(3):
                delta = 1.0 if i == j else 0.0
                acc += c0[:, :, 0] * ((delta + xs[:, i] * xs[:, j]) * fe[:, j])
                acc += c1[:, :, 0] * ((delta - xs[:, i] * xs[:, j]) * fe[:, j])
            RHS[:, seg(i)] += acc
        RHS[:, 3 * n:] += 2 * c0[:, :, 0] * (xs * fs).sum(dim=1)
        RHS[:, 3 * n:] += (c0[:, :, 0] - c1[:, :, 0]) * (xss * fe).sum(dim=1)

    # ---- force operator (update_force_operator) ----
    F = torch.zeros((nf, 3 * n, 4 * n), dtype=torch.float64, device=dev)
    D4preT = (s ** 4 * T(m["D_4_0"])[None]).transpose(1, 2)
    for i in range(3):
        F[:, seg(i), seg(i)] = -E * D4preT
        Tt = (D1pre * xs[:, i][:, None, :]).transpose(1, 2).clone()
        Tt[:, ar, ar] += xss[:, i]
        F[:, seg(i), seg(3)] = Tt

    # ---- boundary conditions (apply_bc_rectangular) ----
    P = T(m["P_downsample_bc"])
    A[:, : 4 * n - 14, :] = torch.matmul(P[None], A)
    RHS[:, : 4 * n - 14] = RHS @ P.T
    B = torch.zeros((nf, 14, 4 * n), dtype=torch.float64, device=dev)
    B_RHS = torch.zeros((nf, 14), dtype=torch.float64, device=dev)
    c0f = c0[:, 0, 0]
    Ef = E[:, 0, 0]
    bdtf = beta_dt[:, 0, 0]

    def end_rows(r0, node, sign, vel, angular):
        """The seven BC rows r0..r0+6 of one fiber end at `node`. The ends
        mirror each other: the Force leg's terms flip with `sign` (+1 minus
        end, -1 plus end). vel: per-fiber mask, first condition Velocity
        (else Force); fibers are grouped by it and each group is one
        vectorized write. The second condition is Torque, except
        AngularVelocity on the Velocity group where `angular`."""
        iv = torch.from_numpy(np.where(vel)[0]).to(dev)
        if len(iv):  # Velocity
            for i in range(3):
                B[iv, r0 + i, i * n + node] = bdtf[iv]
                B[iv, r0 + 3, seg(i)] = \
                    (6.0 * Ef[iv] * c0f[iv] * xss[iv, i, node])[:, None] * D3[iv, node]
            B[iv, r0 + 3, 3 * n:] = (2.0 * c0f[iv])[:, None] * D1[iv, node]
            B_RHS[iv, r0: r0 + 3] = x[iv, :, node] / dt
            if von is not None:
                B_RHS[iv, r0 + 3] -= (xs[iv, :, node] * von[iv, :, node]).sum(dim=1)
            if fon is not None:
                B_RHS[iv, r0 + 3] -= \
                    2 * c0f[iv] * (xs[iv, :, node] * fon[iv, :, node]).sum(dim=1)
        idx = torch.from_numpy(np.where(~vel)[0]).to(dev)
        if len(idx):  # Force
            for i in range(3):
                B[idx, r0 + i, seg(i)] = (sign * Ef[idx])[:, None] * D3[idx, node]
                B[idx, r0 + i, 3 * n + node] = -sign * xs[idx, i, node]
                B[idx, r0 + 3, seg(i)] = \
                    (-sign * Ef[idx] * xss[idx, i, node])[:, None] * D2[idx, node]
            B[idx, r0 + 3, 3 * n + node] = -sign
            if fon is not None:
                B_RHS[idx, r0: r0 + 3] = fon[idx, :, node]
                B_RHS[idx, r0 + 3] = (fon[idx, :, node] * xs[idx, :, node]).sum(dim=1)
        for i in range(3):  # Torque
            B[:, r0 + 4 + i, seg(i)] = D2[:, node]
        if angular and len(iv):  # AngularVelocity pairs with Velocity
            for i in range(3):
                B[iv, r0 + 4 + i, seg(i)] = bdtf[iv][:, None] * D1[iv, node]
            B_RHS[iv, r0 + 4: r0 + 7] = xs[iv, :, node] / dt

    end_rows(0, 0, 1.0, np.array([f.bc_minus[0] == BC_VELOCITY for f in fibers]),
             angular=True)
    # plus second BC: Torque for all supported configurations
    end_rows(7, n - 1, -1.0, np.array([f.bc_plus[0] == BC_VELOCITY for f in fibers]),
             angular=False)

    A[:, 4 * n - 14:, :] = B
    RHS[:, 4 * n - 14:] = B_RHS
    return A, RHS, F


def install_operators(fibers, A, RHS, F):
    """Install assembled operators on the fibers from host arrays
    (nf, 4n, 4n), (nf, 4n), (nf, 3n, 4n): what the per-fiber methods
    (FiberFD.matvec, the RHS) read."""
    for k, f in enumerate(fibers):
        f.adopt_operator(A[k], RHS[k])
        f.force_operator = F[k]
