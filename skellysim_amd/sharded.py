"""Multi-GPU target-sharded pair evaluation (RCCL over xGMI).

Decomposition (mirroring the reference's contiguous block
distribution of targets across MPI ranks — fibers:
fiber_container_finite_difference.cpp:102-121, shell nodes:
periphery.cpp:388-406): each rank owns a contiguous block of targets and a
contiguous block of sources; per evaluation the sources are all-gathered
(one collective over xGMI), then each rank computes its target block against
ALL sources with zero further communication. Velocities stay sharded.

The reference's own GPU path is strictly single-rank (system.cpp:618-623
hard-errors "CPU"/"GPU" with >1 MPI rank) — this module is the new capability
that lifts that restriction.

One process per GPU via torch.distributed; backend "nccl" IS RCCL on ROCm.
The collective logic is backend-agnostic so the world_size>1 path is covered
by gloo CPU tests (tests/test_sharding.py); compute on the product path is
the HIP extension (compute_fn defaults to the stokeslet device kernel and
fails loudly without a GPU).

Comm is the one place that asks torch.distributed whether there is a world:
the evaluator here and the solve pipeline (system_fd.py / system_dist.py)
reach their collectives through it.
"""

import numpy as np


def shard_sizes(n, world):
    """Contiguous block distribution: first n % world ranks get one extra
    (mirrors get_chunk_start_and_size, reference src/core/kernels.cpp:42-51)."""
    base = n // world
    rem = n % world
    return [base + 1 if r < rem else base for r in range(world)]


def shard_range(n, world, rank):
    sizes = shard_sizes(n, world)
    start = sum(sizes[:rank])
    return start, start + sizes[rank]


def allgather_rows(local, group=None):
    """All-gather a (n_local, d) fp64 tensor with per-rank-varying n_local,
    preserving rank order (rank 0's rows first). Returns a (n_total, d)
    tensor on the same device. Works over nccl (GPU) and gloo (CPU)."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    if world == 1:
        return local
    d = local.shape[1]
    n_local = torch.tensor([local.shape[0]], dtype=torch.int64, device=local.device)
    counts = torch.empty(world, dtype=torch.int64, device=local.device)
    dist.all_gather_into_tensor(counts, n_local, group=group)
    counts = counts.tolist()
    n_max = max(counts)
    padded = torch.zeros((n_max, d), dtype=local.dtype, device=local.device)
    padded[: local.shape[0]] = local
    gathered = torch.empty((world * n_max, d), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(gathered, padded, group=group)
    if all(c == n_max for c in counts):
        return gathered
    parts = [gathered[r * n_max: r * n_max + counts[r]] for r in range(world)]
    return torch.cat(parts, dim=0)


class Comm:
    """The questions the solve pipeline asks of torch.distributed — rank,
    world size, gather rows in rank order, take rank 0's vector, sum over
    ranks. Every one is the identity when no process group exists or the
    world is 1, and always for Comm(single=True) (a single-rank system
    inside somebody else's process group)."""

    def __init__(self, group=None, single=False):
        self.group = group
        self.single = single

    def _dist(self):
        """torch.distributed if there is a process group to talk to."""
        import torch.distributed as dist
        if not self.single and dist.is_available() and dist.is_initialized():
            return dist
        return None

    @property
    def world(self):
        dist = self._dist()
        return dist.get_world_size(self.group) if dist else 1

    @property
    def rank(self):
        dist = self._dist()
        return dist.get_rank(self.group) if dist else 0

    def gather_rows(self, a):
        """All ranks' (n_local, ...) rows, rank 0's first (allgather_rows);
        numpy array or tensor in, the same kind out."""
        import torch
        if self.world == 1:
            return a
        if torch.is_tensor(a):
            return allgather_rows(a, self.group)
        t = torch.from_numpy(np.ascontiguousarray(a).reshape(
            len(a), int(np.prod(a.shape[1:]))))
        return allgather_rows(t, self.group).numpy().reshape(-1, *a.shape[1:])

    def from_root(self, a, n):
        """Rank 0's length-n fp64 vector a on every rank (on the other
        ranks only a's kind and device matter); numpy array or tensor in,
        the same kind out."""
        import torch
        if self.world == 1:
            return a
        t = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, float))
        t = t.contiguous() if self.rank == 0 else t.new_zeros(n)
        self._dist().broadcast(t, src=0, group=self.group)
        return t if torch.is_tensor(a) else t.numpy()

    def sum(self, a):
        """Elementwise sum over ranks; numpy array or tensor in, the same
        kind out."""
        import torch
        if self.world == 1:
            return a
        t = a.clone() if torch.is_tensor(a) else torch.from_numpy(np.array(a))
        self._dist().all_reduce(t, group=self.group)
        return t if torch.is_tensor(a) else t.numpy()


class ShardedPairEvaluator:
    """Target-sharded pair evaluation over a torch.distributed world.

    compute_fn(r_src_all, f_src_all, r_trg_local, eta) -> u_local.
    The default is the HIP stokeslet device kernel (product path; requires a
    GPU and the in-tree extension — no CPU fallback). Tests may inject an
    oracle-backed compute_fn to exercise the collective logic on CPU.
    """

    def __init__(self, compute_fn=None, kernel="stokeslet", group=None):
        if compute_fn is None:
            from . import evaluator as ev

            if kernel == "stokeslet":
                compute_fn = lambda r, f, t, eta: ev.stokeslet_device(r, f, t, eta)
            elif kernel == "stresslet":
                compute_fn = lambda r, f, t, eta: ev.stresslet_device(r, f, t, eta)
            elif kernel == "oseen":
                compute_fn = lambda r, f, t, eta: ev.oseen_contract_device(r, t, f, eta)
            elif kernel == "rotlet":
                compute_fn = lambda r, f, t, eta: ev.rotlet_device(r, t, f, eta)
            elif kernel == "stokeslet_pressure":  # (n_trg,); no pressure reads eta
                compute_fn = lambda r, f, t, eta: ev.stokeslet_pressure_device(r, f, t)
            elif kernel == "stresslet_pressure":
                compute_fn = lambda r, f, t, eta: ev.stresslet_pressure_device(r, f, t)
            else:
                raise ValueError(f"unknown kernel {kernel!r}")

        self._compute = compute_fn
        self._comm = Comm(group)

    def __call__(self, r_src_local, f_src_local, r_trg_local, eta=1.0):
        r_all = self._comm.gather_rows(r_src_local)
        f_all = self._comm.gather_rows(f_src_local)
        return self._compute(r_all, f_all, r_trg_local, eta)


def local_shard(arr, world, rank):
    """numpy helper: this rank's contiguous block of rows."""
    a, b = shard_range(len(arr), world, rank)
    return np.asarray(arr)[a:b]
