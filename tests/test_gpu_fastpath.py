"""The pair kernels' unmasked fast path (pair_driver of csrc/pair_kernels.hip over
the pair<false> of the functors of csrc/pair_functors.hpp): each chunk of
sources runs without the r == 0 mask and is rerun masked only when a lane's
accumulator went NaN (oseen: when a tracked r^2 hit zero). Every case is
checked two ways: against the CPU oracle at the parity bar of
test_gpu_parity.py, and fast path on against fast path off in the same build,
which must agree bit for bit.

Sizes are a few thousand points: CHUNK = 64 sources per check, counted from
the slice start and read from the packed records in groups of 2 sources (1
for the stresslet), two groups in flight; 256-thread blocks with up to 4
targets a thread (target i sits in slot (i % 1024) // 256, wave
(i % 256) // 64). Where a case below speaks of tiles of 512 sources or of an
unroll by 4, those are the boundaries of the earlier LDS-staged loop; the
sizes are kept, they still leave a short last chunk and an odd last group."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-10  # the parity bar of tests/test_gpu_parity.py


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def ska(hip_lib_path):
    import skellysim_amd
    return skellysim_amd


def on_off(fn):
    """fn() with the fast path forced on (mode 2: the default, auto, keeps
    launches this small on the masked path), then off; the switch is left
    at its default."""
    from skellysim_amd import _native
    try:
        _native.set_pair_fastpath(2)
        u_on = fn()
        _native.set_pair_fastpath(0)
        u_off = fn()
    finally:
        _native.set_pair_fastpath(1)
    return u_on, u_off


ETA = 1.3


def run_kernel(ska, oracle_mod, kernel, r_src, r_trg, rng):
    """(u_on, u_off, oracle) of one kernel on the given clouds; strengths are
    drawn from rng."""
    n = len(r_src)
    if kernel == "stokeslet":
        f = rng.uniform(-1, 1, (n, 3))
        u_on, u_off = on_off(lambda: ska.stokeslet_direct_gpu(r_src, None, r_trg, f, None, ETA))
        ref = oracle_mod.stokeslet(r_src, f, r_trg, ETA)
    elif kernel == "stresslet":
        f = rng.uniform(-1, 1, (n, 9))
        u_on, u_off = on_off(lambda: ska.stresslet_direct_gpu(None, r_src, r_trg, None, f, ETA))
        ref = oracle_mod.stresslet(r_src, f, r_trg, ETA)
    elif kernel == "oseen":
        f = rng.uniform(-1, 1, (n, 3))
        u_on, u_off = on_off(lambda: ska.oseen_contract_direct_gpu(r_src, r_trg, f, ETA))
        ref = oracle_mod.oseen_contract(r_src, r_trg, f, ETA)
    elif kernel == "rotlet":
        f = rng.uniform(-1, 1, (n, 3))
        u_on, u_off = on_off(lambda: ska.rotlet_gpu(r_src, r_trg, f, ETA))
        ref = oracle_mod.rotlet(r_src, r_trg, f, ETA)
    else:  # stresslet-normal-density: one point set acts on itself
        assert r_trg is r_src
        nrm = rng.uniform(-1, 1, (n, 3))
        rho = rng.uniform(-1, 1, (n, 3))
        u_on, u_off = on_off(lambda: ska.stresslet_times_normal_times_density(r_src, nrm, rho))
        ref = oracle_mod.stresslet_times_normal_times_density(r_src, nrm, rho)
    return u_on, u_off, ref


def check(u_on, u_off, ref):
    assert np.array_equal(u_on, u_off), \
        f"fast path on/off differ in {np.count_nonzero(u_on != u_off)} entries"
    assert np.all(np.isfinite(u_on))
    r = rel(u_on, ref)
    print(f"rel vs oracle = {r:.3e}")
    assert r < REL_TOL


PAIR_KERNELS = ["stokeslet", "stresslet", "oseen"]


@pytest.mark.parametrize("n", [1300, 1303])
@pytest.mark.parametrize("kernel", PAIR_KERNELS + ["snd"])
def test_sources_equal_targets(ska, oracle_mod, kernel, n):
    """Every target coincides with one source: three tiles, the last one short
    (276 = 4 chunks + 20); 1303 adds a remainder after the unroll by 4."""
    rng = np.random.default_rng(1000 + n)
    r = rng.uniform(-1, 1, (n, 3))
    check(*run_kernel(ska, oracle_mod, kernel, r, r, rng))


@pytest.mark.parametrize("kernel", PAIR_KERNELS)
def test_split_path(ska, oracle_mod, kernel):
    """6000 sources go out as 3 source slices of 2000; the 1500 targets are
    the first 1500 sources, so only slice 0 holds coincidences."""
    rng = np.random.default_rng(2000)
    r_src = rng.uniform(-1, 1, (6000, 3))
    r_trg = r_src[:1500].copy()
    check(*run_kernel(ska, oracle_mod, kernel, r_src, r_trg, rng))


@pytest.mark.parametrize("kernel", PAIR_KERNELS)
def test_duplicates_on_boundaries(ska, oracle_mod, kernel):
    """Sources on both sides of a chunk boundary (63 | 64) and of a tile
    boundary (511 | 512) copied to targets in four different waves and
    target slots of block 0 and into block 1, plus one duplicated source
    pair that is also a target."""
    rng = np.random.default_rng(3000)
    r_src = rng.uniform(-1, 1, (1300, 3))
    r_trg = rng.uniform(-1, 1, (1100, 3))
    r_src[700] = r_src[300]
    r_trg[5] = r_src[63]                # slot 0, wave 0
    r_trg[256 + 70] = r_src[64]         # slot 1, wave 1
    r_trg[512 + 130] = r_src[511]       # slot 2, wave 2
    r_trg[768 + 200] = r_src[512]       # slot 3, wave 3
    r_trg[1050] = r_src[64]             # block 1
    r_trg[400] = r_src[300]             # hits both copies of the duplicate
    check(*run_kernel(ska, oracle_mod, kernel, r_src, r_trg, rng))


@pytest.mark.parametrize("kernel", PAIR_KERNELS)
def test_all_sources_on_one_target(ska, oracle_mod, kernel):
    """600 sources at one point that is also target 77: every chunk of that
    wave is rerun, and the target gets exactly zero."""
    rng = np.random.default_rng(4000)
    p = rng.uniform(-1, 1, 3)
    r_src = np.tile(p, (600, 1))
    r_trg = rng.uniform(-1, 1, (1100, 3))
    r_trg[77] = p
    u_on, u_off, ref = run_kernel(ska, oracle_mod, kernel, r_src, r_trg, rng)
    check(u_on, u_off, ref)
    assert np.all(u_on[77] == 0.0)


@pytest.mark.parametrize("kernel", PAIR_KERNELS)
def test_disjoint_clouds(ska, oracle_mod, kernel):
    """Targets shifted by (3, 0, 0): no coincidence, no rerun."""
    rng = np.random.default_rng(5000)
    r_src = rng.uniform(-1, 1, (1300, 3))
    r_trg = r_src[:1100] + np.array([3.0, 0.0, 0.0])
    check(*run_kernel(ska, oracle_mod, kernel, r_src, r_trg, rng))


def test_oseen_near_pairs_and_coincidences(ska, oracle_mod):
    """Targets ~3e-6 from their sources (below epsilon_distance = 1e-5, the
    regularized branch, as in test_oseen_near_branch), every third one moved
    back onto its source exactly."""
    rng = np.random.default_rng(6000)
    r_src = rng.uniform(-1, 1, (1300, 3))
    r_trg = r_src[:1100] + rng.uniform(-1, 1, (1100, 3)) * 3e-6
    r_trg[::3] = r_src[:1100:3]
    check(*run_kernel(ska, oracle_mod, "oseen", r_src, r_trg, rng))


def test_rotlet_folded_scale(ska, oracle_mod):
    """Rotlet has no mask; this covers the 3-op refinement with 1/8 folded
    into the scale, at the reference recipe's sizes."""
    rng = np.random.default_rng(7000)
    r_src = rng.uniform(-1, 1, (1229, 3))
    r_trg = rng.uniform(-1, 1, (743, 3))
    check(*run_kernel(ska, oracle_mod, "rotlet", r_src, r_trg, rng))


@pytest.mark.parametrize("kernel", PAIR_KERNELS)
def test_nan_source_coordinate(ska, kernel):
    """One NaN source coordinate: the call returns (each chunk is rerun once,
    no loop) and every output is NaN, fast path on or off."""
    rng = np.random.default_rng(8000)
    r_src = rng.uniform(-1, 1, (1300, 3))
    r_src[200, 1] = np.nan
    r_trg = rng.uniform(-1, 1, (1100, 3))
    if kernel == "stokeslet":
        f = rng.uniform(-1, 1, (1300, 3))
        fn = lambda: ska.stokeslet_direct_gpu(r_src, None, r_trg, f, None, ETA)
    elif kernel == "stresslet":
        f = rng.uniform(-1, 1, (1300, 9))
        fn = lambda: ska.stresslet_direct_gpu(None, r_src, r_trg, None, f, ETA)
    else:
        f = rng.uniform(-1, 1, (1300, 3))
        fn = lambda: ska.oseen_contract_direct_gpu(r_src, r_trg, f, ETA)
    u_on, u_off = on_off(fn)
    assert np.all(np.isnan(u_on))
    assert np.all(np.isnan(u_off))
