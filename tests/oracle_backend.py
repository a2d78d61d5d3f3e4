"""Test-only backend over the CPU oracle for SystemFD orchestration tests.
Lives under tests/ (not the product package) so nothing on the product path
can import the oracle (oracle/ is test infrastructure; see oracle/__init__.py).
Method contract matches skellysim_amd.system_fd.HipBackend's, on numpy
arrays; having no device, it is a host backend, and SystemFD runs its one
pipeline over it on CPU tensors."""

import numpy as np


class OracleBackend:
    """TEST-ONLY backend over the CPU oracle (oracle/ is test infrastructure;
    this class exists so the orchestration logic is CPU-testable and must
    never be used outside tests)."""

    def __init__(self):
        import oracle
        self.oracle = oracle

    def stokeslet(self, r_src, f_src, r_trg, eta):
        return self.oracle.stokeslet(r_src, f_src, r_trg, eta)

    def stresslet_normal_density(self, r_src, normals, density, r_trg, eta):
        f_dl = 2.0 * eta * np.einsum("ni,nj->nij", normals, density).reshape(-1, 9)
        return self.oracle.stresslet(r_src, f_dl, r_trg, eta)

    def self_stokeslet_batch(self, pts, eta):
        return np.stack([self.oracle.oseen_tensor(p, eta) for p in pts])

    def rotlet(self, centers, torques, r_trg, eta):
        return self.oracle.rotlet(centers, r_trg, torques, eta)

    def oseen_contract(self, r_src, r_trg, density, eta):
        return self.oracle.oseen_contract(r_src, r_trg, density, eta)

    def stresslet_times_normal(self, nodes, normals, eta):
        return self.oracle.np_stresslet_times_normal(nodes, normals)
