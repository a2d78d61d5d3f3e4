"""Forced source-slice counts of the pair kernels (set_pair_slices): the split
launch with slices shorter than a tile, slice starts that are no multiple of
a chunk, one-source slices and empty last slices.

Clouds as in test_gpu_fastpath.py: 1300 sources are 3 tiles of 512 with the
last one short, 1303 add a remainder after the unroll by 4; 1100 targets are
2 blocks at 4 targets a thread, the second ragged. Slices are ceil(n / S)
sources long: 7 slices of 1300 hold 186 each (two chunks and 58, starts at
186 k), 1303 slices hold one source each, 5000 is clamped to 1303.

Every case: norm-relative error against the reference under the parity bar of
test_gpu_parity.py, fast path forced on and off bit-identical, two
consecutive calls bit-identical."""

import numpy as np
import pytest

from test_gradient_cpu import np_stokeslet_grad

pytestmark = pytest.mark.gpu

REL_TOL = 1e-10
ETA = 1.3
N_TRG = 1100


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def ska(hip_lib_path):
    import skellysim_amd
    return skellysim_amd


@pytest.fixture(scope="module")
def clouds(oracle_mod):
    """Per source count: clouds, strengths and the references, computed once."""
    out = {}
    for n in (1300, 1303):
        rng = np.random.default_rng(7100 + n)
        c = dict(r_src=rng.uniform(-1, 1, (n, 3)), r_trg=rng.uniform(-1, 1, (N_TRG, 3)),
                 f3=rng.uniform(-1, 1, (n, 3)), f9=rng.uniform(-1, 1, (n, 9)))
        c["ref"] = dict(
            stokeslet=oracle_mod.stokeslet(c["r_src"], c["f3"], c["r_trg"], ETA),
            stresslet=oracle_mod.stresslet(c["r_src"], c["f9"], c["r_trg"], ETA),
            oseen=oracle_mod.oseen_contract(c["r_src"], c["r_trg"], c["f3"], ETA),
            rotlet=oracle_mod.rotlet(c["r_src"], c["r_trg"], c["f3"], ETA))
        out[n] = c
    return out


def evaluate(ska, kernel, r_src, r_trg, f):
    if kernel == "stokeslet":
        return ska.stokeslet_direct_gpu(r_src, None, r_trg, f, None, ETA)
    if kernel == "stresslet":
        return ska.stresslet_direct_gpu(None, r_src, r_trg, None, f, ETA)
    if kernel == "oseen":
        return ska.oseen_contract_direct_gpu(r_src, r_trg, f, ETA)
    if kernel == "rotlet":
        return ska.rotlet_gpu(r_src, r_trg, f, ETA)
    assert kernel == "stokeslet_grad"
    return ska.stokeslet_grad(r_src, f, r_trg, ETA)


def sliced(n_slices, fn):
    """(on, on again, off): fn() under n_slices forced slices with the fast
    path forced on, twice, and off; both switches back at their defaults."""
    from skellysim_amd import _native
    try:
        _native.set_pair_slices(n_slices)
        _native.set_pair_fastpath(2)
        u_on = fn()
        u_again = fn()
        _native.set_pair_fastpath(0)
        u_off = fn()
    finally:
        _native.set_pair_fastpath(1)
        _native.set_pair_slices(0)
    return u_on, u_again, u_off


def check(u_on, u_again, u_off, ref):
    assert np.array_equal(u_on, u_again), "two consecutive calls differ"
    assert np.array_equal(u_on, u_off), \
        f"fast path on/off differ in {np.count_nonzero(u_on != u_off)} entries"
    assert np.all(np.isfinite(u_on))
    r = rel(u_on, ref)
    print(f"rel vs reference = {r:.3e}")
    assert r < REL_TOL


CASES = [(1300, s) for s in (1, 2, 3, 7)] + [(1303, s) for s in (1, 2, 3, 7, 1303, 5000)]


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "oseen"])
@pytest.mark.parametrize("n_src,n_slices", CASES)
def test_forced_slices(ska, clouds, kernel, n_src, n_slices):
    c = clouds[n_src]
    f = c["f9"] if kernel == "stresslet" else c["f3"]
    check(*sliced(n_slices, lambda: evaluate(ska, kernel, c["r_src"], c["r_trg"], f)),
          c["ref"][kernel])


def test_forced_slices_rotlet(ska, clouds):
    c = clouds[1303]
    check(*sliced(7, lambda: evaluate(ska, "rotlet", c["r_src"], c["r_trg"], c["f3"])),
          c["ref"]["rotlet"])


def test_forced_slices_gradient_workspace(ska, clouds):
    """stokeslet_grad: 9 outputs a target through the partial workspace and
    the reduction, 2 targets a thread; reference is the numpy closed form of
    tests/test_gradient_cpu.py, as in test_gpu_gradient.py."""
    c = clouds[1303]
    ref = np_stokeslet_grad(c["r_src"], c["f3"], c["r_trg"], ETA)
    check(*sliced(7, lambda: evaluate(ska, "stokeslet_grad", c["r_src"], c["r_trg"], c["f3"])),
          ref)


def test_clamped_count_equals_one_source_slices(ska, clouds):
    """5000 slices on 1303 sources are clamped to 1303: the same launch."""
    c = clouds[1303]
    fn = lambda: evaluate(ska, "stokeslet", c["r_src"], c["r_trg"], c["f3"])
    assert np.array_equal(sliced(5000, fn)[0], sliced(1303, fn)[0])


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "oseen"])
def test_coincident_targets_in_three_slices(ska, oracle_mod, clouds, kernel):
    """Targets are the first 1100 sources, 3 slices of 434: every target
    meets its own source in slice 0, 1 or 2. Against 1 slice the result moves
    by rounding only (bound: 1300 terms summed in another order, 1300 eps of
    the norm, far above what two orders of a random sum differ by and far
    below one dropped or doubled pair, ~1e-3)."""
    c = clouds[1300]
    r_src = c["r_src"]
    r_trg = r_src[:N_TRG].copy()
    f = c["f9"] if kernel == "stresslet" else c["f3"]
    fn = lambda: evaluate(ska, kernel, r_src, r_trg, f)
    u3 = sliced(3, fn)
    ref = getattr(oracle_mod, {"oseen": "oseen_contract"}.get(kernel, kernel))
    ref = ref(r_src, r_trg, f, ETA) if kernel == "oseen" else ref(r_src, f, r_trg, ETA)
    check(*u3, ref)
    u1 = sliced(1, fn)[0]
    d = rel(u3[0], u1)
    print(f"3 slices vs 1 slice: {d:.3e}")
    assert d < 1300 * np.finfo(float).eps


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "oseen"])
def test_all_sources_on_one_target_sliced(ska, oracle_mod, kernel):
    """600 sources at one point that is also target 77 (the shape of
    test_gpu_fastpath.test_all_sources_on_one_target), in 3 slices of 200:
    each slice's partial for that target is exactly zero, and so is the sum."""
    rng = np.random.default_rng(4000)
    p = rng.uniform(-1, 1, 3)
    r_src = np.tile(p, (600, 1))
    r_trg = rng.uniform(-1, 1, (N_TRG, 3))
    r_trg[77] = p
    f = rng.uniform(-1, 1, (600, 9 if kernel == "stresslet" else 3))
    u = sliced(3, lambda: evaluate(ska, kernel, r_src, r_trg, f))
    ref = getattr(oracle_mod, {"oseen": "oseen_contract"}.get(kernel, kernel))
    ref = ref(r_src, r_trg, f, ETA) if kernel == "oseen" else ref(r_src, f, r_trg, ETA)
    check(*u, ref)
    assert np.all(u[0][77] == 0.0)


def test_shard_reassembly_under_equal_forced_counts(ska):
    """3 slices forced on 3000 sources: the full run (1501 targets) and its
    four shard_range pieces sum every target in the same order."""
    from skellysim_amd import _native
    from skellysim_amd.sharded import shard_range
    rng = np.random.default_rng(9)
    n_src, n_trg, world = 3000, 1501, 4
    r_src = rng.uniform(-1, 1, (n_src, 3))
    f_src = rng.uniform(-1, 1, (n_src, 3))
    r_trg = rng.uniform(-1, 1, (n_trg, 3))
    try:
        _native.set_pair_slices(3)
        u_full = ska.stokeslet_direct_gpu(r_src, None, r_trg, f_src, None, 1.0)
        parts = []
        for rank in range(world):
            a, b = shard_range(n_trg, world, rank)
            parts.append(ska.stokeslet_direct_gpu(r_src, None, r_trg[a:b], f_src, None, 1.0))
    finally:
        _native.set_pair_slices(0)
    assert np.array_equal(np.vstack(parts), u_full)
