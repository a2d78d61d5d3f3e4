"""Multi-rank (one process per GPU) fiber + periphery solves.

Decomposition mirrors the reference's MPI layout:
fibers block-distributed in contiguous chunks across ranks
(fiber_container_finite_difference.cpp:98-121), shell rows block-distributed
(periphery.cpp:388-406,422-442), and per apply the pair-kernel SOURCES are
all-gathered (the reference's per-iteration MPI_Allgatherv,
periphery.cpp:26,44 -> RCCL over xGMI) while every rank evaluates only its
own target block. GMRES runs with distributed inner products
(gmres distributed=True — the Tpetra/Belos dots).

The reference hard-forbids its direct evaluators under >1 rank
(system.cpp:618-623); this module is the new multi-GPU capability.

There is no second pipeline here: prep, the matvec, the preconditioner,
solve and step are SystemFD's, which is written against a rank-local layout
and a communicator (see system_fd.py). This module supplies the two things
that make a rank's view non-trivial — the layout (own shell rows; body block
on rank 0 only) and the live communicator — so at world size 1 it IS the
single-rank solve, bodies included. Covered by gloo world-2 CPU tests
(tests/test_dist_system.py, on CPU tensors over the oracle backend) and by
a world-1 HIP test (test_gpu_system.py); the same code drives RCCL + HIP
kernels on multi-GPU boxes.
"""

from .sharded import Comm, shard_range
from .system_fd import SystemFD


class DistributedSystemFD(SystemFD):
    """Rank-local view of the global system.

    Construct with this rank's OWN fibers and this rank's OWN shell row block
    (shell.A / shell.M_inv hold the (3n_local, 3N_global) row slices;
    shell.nodes/normals hold the GLOBAL shell geometry, shell_rows the
    [row0, row1) node range owned here). Requires >= 1 fiber per rank.
    """

    # follows the default process group; the identity without one
    comm = Comm()

    def __init__(self, fibers, eta, dt, shell=None, shell_rows=None,
                 background_flow=None, backend=None, bodies=None):
        # periphery_interaction is deliberately not accepted here: its
        # repulsion-induced flow in prep has not been validated against
        # the single-process solve under a world > 1 yet
        self.shell_rows = shell_rows  # (a, b) node indices owned by this rank
        super().__init__(fibers, eta, dt, shell=shell,
                         background_flow=background_flow, backend=backend,
                         bodies=bodies)

    # rank-local solution: [own fibers | own shell rows | bodies if rank 0]
    def _own_shell_nodes(self):
        a, b = self.shell_rows
        return self.shell.nodes[a:b]

    def _own_bodies(self):
        # the body objects are replicated on every rank; their solution
        # block lives only in rank 0's vector (body_container.hpp:99)
        return self.bodies if self.comm.rank == 0 else []


def distribute_fibers(fibers, world, rank):
    """Contiguous block distribution (f_c_fd.cpp:98-121)."""
    a, b = shard_range(len(fibers), world, rank)
    return fibers[a:b]
