"""CPU tests of SystemFD's one matvec / preconditioner on the layouts where
it can go wrong — per-fiber lengths inside a batch, and several runs of
different node counts — against the per-object host oracle
(tests/system_oracle.py), through the oracle backend."""

import os

import numpy as np
import pytest

from skellysim_amd.body import SphericalBody
from skellysim_amd.fiber_fd import FiberFD
from skellysim_amd.system_fd import SystemFD, Shell
from oracle_backend import OracleBackend
from system_oracle import pipeline_vs_host

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, "golden", "periphery_sphere_192.npz"))


def straight_fiber(n, length, x0, direction, **kw):
    d = np.asarray(direction, float) / np.linalg.norm(direction)
    x = np.asarray(x0, float)[None, :] + np.linspace(0, length, n)[:, None] * d[None, :]
    return FiberFD(x, length=length, bending_rigidity=2.5e-3, eta=1.0, **kw)


@pytest.mark.parametrize("with_shell", [False, True], ids=["free", "shell"])
def test_unequal_lengths_in_one_batch(with_shell):
    """Two 16-node fibers of lengths 0.5 and 1.0 are one run ("uniform"
    means equal node counts, not equal lengths): the tension row's D_1 must
    take each fiber's own 2/length_prev. A shared factor from the first
    fiber is off by 8.5e-3 here."""
    fibs = [straight_fiber(16, 0.5, (0.0, 0.0, -0.2), (0, 0, 1.0)),
            straight_fiber(16, 1.0, (0.2, 0.1, -0.3), (1.0, 1.0, 0.5))]
    shell = Shell(FX["nodes"] * 4.0, FX["normals"],
                  FX["stresslet_plus_complementary"], FX["M_inv"]) \
        if with_shell else None
    s = SystemFD(fibs, eta=1.0, dt=0.05, shell=shell, backend=OracleBackend())
    assert s._fiber_runs() == [[0, 2]]
    rel_mv, rel_pc = pipeline_vs_host(s)
    assert rel_mv < 1e-12, rel_mv
    # two LU implementations on ill-conditioned fiber operators: the bound
    # every CPU preconditioner comparison here uses
    assert rel_pc < 1e-9, rel_pc


def test_mixed_runs_with_shell_and_body():
    """Node counts [16, 16, 32, 16]: three runs with a repeated count; the
    first fiber is attached to a body (so minus-clamped by its BCs), the
    third is minus-clamped, all inside a 192-node shell."""
    R = float(FX["radius"])
    body = SphericalBody(FX["nodes"], -FX["normals"],
                         FX["quadrature_weights"].reshape(-1), R,
                         nucleation_sites_ref=np.array([[1.1 * R, 0.0, 0.0]]))
    site = body.nucleation_sites[0]
    fibs = [straight_fiber(16, 0.8, site, site, minus_clamped=True,
                           force_scale=-0.05),
            straight_fiber(16, 0.5, (0.0, 1.8, 0.3), (0, 0, 1.0)),
            straight_fiber(32, 0.7, (0.0, -1.9, 0.0), (0.2, -1.0, 0.1),
                           minus_clamped=True, force_scale=-0.02),
            straight_fiber(16, 0.6, (-1.7, 0.0, 0.0), (-1.0, 0.3, 0.0))]
    fibs[0].binding_site = (0, 0)
    shell = Shell(FX["nodes"] * 4.0, FX["normals"],
                  FX["stresslet_plus_complementary"], FX["M_inv"])
    s = SystemFD(fibs, eta=1.0, dt=0.05, shell=shell, bodies=[body],
                 backend=OracleBackend())
    assert s._fiber_runs() == [[0, 2], [2, 3], [3, 4]]
    rel_mv, rel_pc = pipeline_vs_host(s)
    assert rel_mv < 1e-12, rel_mv
    assert rel_pc < 1e-9, rel_pc
