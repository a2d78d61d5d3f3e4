"""The pair kernels' packed source records and scalar-operand pair loop: source
counts around the load group (1 or 2 records) and the buffer's padding,
slices that start and end at odd sources, every targets-a-thread
instantiation, coincident points on either side of a chunk (64) and group
boundary, inputs that are only 8-byte aligned, and a short launch after a long
one through the persistent workspace (stale records past the end).

Clouds, references, tolerance and the sliced() pattern (fast path forced on,
on again, off; both switches restored) are those of test_gpu_pair_slices.py:
sources are the first n of its 1300-source cloud against its 1100 targets.
Every check: two consecutive calls bit-identical, fast path on and off
bit-identical, finite, norm-relative error against the reference < REL_TOL."""

import numpy as np
import pytest

from test_gpu_pair_slices import ETA, REL_TOL, check, clouds, rel, ska, sliced  # noqa: F401
from test_gradient_cpu import np_rotlet_grad, np_stokeslet_grad, np_stresslet_grad

pytestmark = pytest.mark.gpu

KERNELS = ["stokeslet", "stresslet", "oseen", "rotlet", "normal_density",
           "stokeslet_grad", "stresslet_grad", "rotlet_grad"]
SRC_COUNTS = [1, 2, 3, 5, 63, 64, 65, 129]
SLICE_COUNTS = [1, 2, 3, 7]
TRG_COUNTS = [1, 255, 257, 513, 1025]  # 513: the 2-targets-a-thread build


def strengths(c, kernel, n):
    """The first n strengths of cloud c in the kernel's layout."""
    if kernel in ("stresslet", "stresslet_grad"):
        return c["f9"][:n]
    if kernel == "normal_density":
        # normals | densities, both (n, 3), cut from the 9 columns
        return c["f9"][:n, :6]
    return c["f3"][:n]


def evaluate(ska, kernel, r_src, r_trg, f):
    if kernel == "stokeslet":
        return ska.stokeslet_direct_gpu(r_src, None, r_trg, f, None, ETA)
    if kernel == "stresslet":
        return ska.stresslet_direct_gpu(None, r_src, r_trg, None, f, ETA)
    if kernel == "oseen":
        return ska.oseen_contract_direct_gpu(r_src, r_trg, f, ETA)
    if kernel == "rotlet":
        return ska.rotlet_gpu(r_src, r_trg, f, ETA)
    if kernel == "stokeslet_grad":
        return ska.stokeslet_grad(r_src, f, r_trg, ETA)
    if kernel == "stresslet_grad":
        return ska.stresslet_grad(r_src, f, r_trg, ETA)
    if kernel == "rotlet_grad":
        return ska.rotlet_grad(r_src, r_trg, f, ETA)
    assert kernel == "normal_density"
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    out = ska.stresslet_normal_density_device(T(r_src), T(f[:, :3]), T(f[:, 3:]), T(r_trg))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def reference(oracle_mod, kernel, r_src, r_trg, f):
    if kernel == "stokeslet":
        return oracle_mod.stokeslet(r_src, f, r_trg, ETA)
    if kernel == "stresslet":
        return oracle_mod.stresslet(r_src, f, r_trg, ETA)
    if kernel == "oseen":
        return oracle_mod.oseen_contract(r_src, r_trg, f, ETA)
    if kernel == "rotlet":
        return oracle_mod.rotlet(r_src, r_trg, f, ETA)
    if kernel == "stokeslet_grad":
        return np_stokeslet_grad(r_src, f, r_trg, ETA)
    if kernel == "stresslet_grad":
        return np_stresslet_grad(r_src, f, r_trg, ETA)
    if kernel == "rotlet_grad":
        return np_rotlet_grad(r_src, r_trg, f, ETA)
    # -3/(4 pi) (d.n)(d.rho)/r^5 d is the stresslet of S = 2 eta n rho^T
    # (tests/oracle_backend.py); coincident pairs are zero in both and no
    # pair here is closer than the regularization distance otherwise
    assert kernel == "normal_density"
    f_dl = 2.0 * ETA * np.einsum("ni,nj->nij", f[:, :3], f[:, 3:]).reshape(-1, 9)
    return oracle_mod.stresslet(r_src, f_dl, r_trg, ETA)


def run_case(ska, oracle_mod, kernel, r_src, r_trg, f, n_slices, ref=None):
    if ref is None:
        ref = reference(oracle_mod, kernel, r_src, r_trg, f)
    ref = np.asarray(ref).reshape(len(r_trg), -1)
    u = [np.asarray(x).reshape(len(r_trg), -1)
         for x in sliced(n_slices, lambda: evaluate(ska, kernel, r_src, r_trg, f))]
    check(*u, ref)
    return u[0]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n_src", SRC_COUNTS)
def test_source_counts_around_group_and_padding(ska, oracle_mod, clouds, kernel, n_src):
    """1 .. 129 sources in 1, 2, 3 and 7 forced slices: slices of 1 and 2
    sources, slices that start at odd sources, empty last slices (7 slices of
    5 sources: one source each, two empty), the last group read into the
    padding. The reference does not depend on the slice count."""
    c = clouds[1300]
    r_src, r_trg, f = c["r_src"][:n_src], c["r_trg"], strengths(c, kernel, n_src)
    ref = reference(oracle_mod, kernel, r_src, r_trg, f)
    for n_slices in SLICE_COUNTS:
        run_case(ska, oracle_mod, kernel, r_src, r_trg, f, n_slices, ref)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n_trg", TRG_COUNTS)
def test_target_counts(ska, oracle_mod, clouds, kernel, n_trg):
    """1, 2 and 4 targets a thread with a ragged last block, 131 sources (two
    chunks and three, an odd count) in 1 and 3 slices."""
    c = clouds[1300]
    r_src, r_trg, f = c["r_src"][:131], c["r_trg"][:n_trg], strengths(c, kernel, 131)
    ref = reference(oracle_mod, kernel, r_src, r_trg, f)
    for n_slices in (1, 3):
        run_case(ska, oracle_mod, kernel, r_src, r_trg, f, n_slices, ref)


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "oseen", "normal_density"])
@pytest.mark.parametrize("n", [65, 129, 257])
def test_coincident_points(ska, oracle_mod, clouds, kernel, n):
    """Targets are the sources: target i meets source i, so self pairs fall on
    both sides of every chunk boundary (63 | 64) and group boundary, in the
    main loop and in the one-source tail (n odd). sliced() forces the fast
    path on (mode 2) and off (0); check() wants them array_equal, finite and
    within tolerance of the oracle."""
    c = clouds[1300]
    r_src = c["r_src"][:n]
    f = strengths(c, kernel, n)
    for n_slices in (1, 2):
        run_case(ska, oracle_mod, kernel, r_src, r_src.copy(), f, n_slices)


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet"])
def test_offset_views(ska, oracle_mod, clouds, kernel):
    """Sources, strengths and targets that start one double into a larger
    device tensor: 8-byte aligned, not 16. Same result as the aligned call."""
    import torch
    c = clouds[1300]
    n = 129
    dim = 9 if kernel == "stresslet" else 3
    arrays = [c["r_src"][:n], strengths(c, kernel, n), c["r_trg"]]
    fn = ska.stresslet_device if kernel == "stresslet" else ska.stokeslet_device

    def shifted(a):
        big = torch.zeros(a.size + 1, dtype=torch.float64, device="cuda:0")
        view = big[1:].view(a.shape)
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        return view

    aligned = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    assert all(t.data_ptr() % 16 == 0 for t in aligned)

    def run(ts):
        out = fn(ts[0], ts[1], ts[2], ETA)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    assert arrays[1].shape[1] == dim
    u_aligned = run(aligned)
    u = sliced(2, lambda: run([shifted(a) for a in arrays]))
    ref = reference(oracle_mod, kernel, *[arrays[i] for i in (0, 2, 1)])
    check(*u, ref)
    u2 = sliced(2, lambda: run(aligned))[0]
    assert np.array_equal(u[0], u2)
    assert rel(u_aligned, ref) < REL_TOL


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "rotlet_grad"])
def test_short_launch_after_long_through_persistent_workspace(ska, oracle_mod, clouds, kernel):
    """With the persistent workspace a 129-source launch reuses the buffer a
    1300-source launch just filled: records 131 .. 1301 are stale. The result
    is the 129-source reference, and bit-identical to the same launch through
    a fresh workspace, for 1 and 7 slices."""
    from skellysim_amd import _native
    c = clouds[1300]
    f_all = strengths(c, kernel, 1300)
    short = (c["r_src"][:129], c["r_trg"], f_all[:129])
    ref = reference(oracle_mod, kernel, *short)
    fresh = {s: run_case(ska, oracle_mod, kernel, *short, s, ref) for s in (1, 7)}
    try:
        _native.lib().skelly_set_persistent_ws(1)
        for n_slices in (1, 7):
            long_u = sliced(n_slices, lambda: evaluate(ska, kernel, c["r_src"], c["r_trg"],
                                                       f_all))[0]
            assert np.all(np.isfinite(long_u))
            u = run_case(ska, oracle_mod, kernel, *short, n_slices, ref)
            assert np.array_equal(u, fresh[n_slices])
    finally:
        _native.lib().skelly_set_persistent_ws(-1)
