"""What the host forms of evaluator.py and the C entry points of
include/skelly_hip.h do with arguments that cannot be launched, checked where
nothing can be launched: the Python tests run against a library that raises
when it is touched, the C tests pass null pointers with a negative or a zero
count, which has to return before the first HIP call (there is no GPU here,
and on a machine that has one nothing may reach it).

A per-source array that is shorter than r_src would be read past its end (by
hipMemcpyAsync in the host forms), so a length mismatch is a ValueError that
names the argument, raised before the library is looked up."""

import ctypes
import threading

import numpy as np
import pytest

from skellysim_amd import _native, evaluator as ev

N = 10
RNG = np.random.default_rng(0)
R_SRC, R_TRG = RNG.uniform(-1, 1, (N, 3)), RNG.uniform(-1, 1, (4, 3))


def strength(n, dim=3):
    return RNG.uniform(-1, 1, (n, dim)) if n is not None else None


# name -> (call(f) with f the strength array, its width, the argument's name)
HOST_FORMS = {
    "stokeslet_direct_gpu": (lambda f: ev.stokeslet_direct_gpu(R_SRC, None, R_TRG, f, None, 1.3),
                             3, "f_sl"),
    "stresslet_direct_gpu": (lambda f: ev.stresslet_direct_gpu(None, R_SRC, R_TRG, None, f, 1.3),
                             9, "f_dl"),
    "oseen_contract_direct_gpu": (lambda f: ev.oseen_contract_direct_gpu(R_SRC, R_TRG, f, 1.3),
                                  3, "density"),
    "rotlet_gpu": (lambda f: ev.rotlet_gpu(R_SRC, R_TRG, f, 1.3), 3, "density"),
    "stokeslet_grad": (lambda f: ev.stokeslet_grad(R_SRC, f, R_TRG, 1.3), 3, "f_src"),
    "stresslet_grad": (lambda f: ev.stresslet_grad(R_SRC, f, R_TRG, 1.3), 9, "f_src"),
    "oseen_contract_grad": (lambda f: ev.oseen_contract_grad(R_SRC, R_TRG, f, 1.3), 3, "density"),
    "rotlet_grad": (lambda f: ev.rotlet_grad(R_SRC, R_TRG, f, 1.3), 3, "density"),
}


@pytest.fixture
def no_library(monkeypatch):
    """_native.lib raises: whatever the validation does, nothing is launched."""
    def lib():
        raise AssertionError("reached the library")
    monkeypatch.setattr(_native, "lib", lib)


class _Recorder:
    """Stands in for the library: every entry point returns 0 and is recorded
    with its integer arguments (the counts)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, [a for a in args if isinstance(a, int)]))
            return 0
        return fn


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_native, "lib", lambda: rec)
    return rec


@pytest.mark.parametrize("n_f", [N - 1, N + 1, None], ids=["short", "long", "none"])
@pytest.mark.parametrize("form", list(HOST_FORMS))
def test_host_form_rejects_strengths_of_another_length(no_library, form, n_f):
    call, dim, name = HOST_FORMS[form]
    with pytest.raises(ValueError, match=name):
        call(strength(n_f, dim))


@pytest.mark.parametrize("n_f", [N - 1, N + 1], ids=["short", "long"])
@pytest.mark.parametrize("form", list(HOST_FORMS))
def test_host_form_rejects_transposed_strengths_of_another_length(no_library, form, n_f):
    call, dim, name = HOST_FORMS[form]
    with pytest.raises(ValueError, match=name):
        call(strength(n_f, dim).T)


@pytest.mark.parametrize("which", ["normals", "density"])
@pytest.mark.parametrize("n_other", [N - 1, N + 1, None], ids=["short", "long", "none"])
def test_normal_density_host_form_rejects_another_length(no_library, which, n_other):
    args = dict(normals=strength(N), density=strength(N))
    args[which] = strength(n_other)
    with pytest.raises(ValueError, match=which):
        ev.stresslet_times_normal_times_density(R_SRC, **args)


@pytest.mark.parametrize("form", list(HOST_FORMS))
def test_matching_lengths_reach_the_library(recorder, form):
    """(n, dim), (dim, n) and empty sources are all valid calls."""
    call, dim, _ = HOST_FORMS[form]
    out = call(strength(N, dim))
    assert out.shape[0] == len(R_TRG)
    call(strength(N, dim).T)
    assert [c[1] for c in recorder.calls] == [[N, len(R_TRG)]] * 2
    assert recorder.calls[0][0] == f"skelly_{ev_symbol(form)}_host"


def ev_symbol(form):
    return {"stokeslet_direct_gpu": "stokeslet", "stresslet_direct_gpu": "stresslet",
            "oseen_contract_direct_gpu": "oseen_contract", "rotlet_gpu": "rotlet"}.get(form, form)


def test_transposed_sources_and_empty_sources_reach_the_library(recorder):
    ev.stokeslet_direct_gpu(R_SRC.T, None, R_TRG.T, strength(N).T, None, 1.3)
    ev.stokeslet_direct_gpu(None, None, R_TRG, None, None, 1.3)
    ev.stresslet_direct_gpu(None, np.empty((0, 3)), R_TRG, None, np.empty((0, 9)), 1.3)
    ev.rotlet_gpu(None, R_TRG, None)
    ev.stresslet_times_normal_times_density(R_SRC.T, strength(N), strength(N).T)
    ev.stresslet_times_normal_times_density(None, None, None)
    assert recorder.calls == [
        ("skelly_stokeslet_host", [N, 4]), ("skelly_stokeslet_host", [0, 4]),
        ("skelly_stresslet_host", [0, 4]), ("skelly_rotlet_host", [0, 4]),
        ("skelly_stresslet_normal_density_host", [N]),
        ("skelly_stresslet_normal_density_host", [0])]


# ---- the C boundary: null pointers, a negative or a zero count -------------------

@pytest.fixture(scope="module")
def lib(hip_lib_path):
    so = ctypes.CDLL(hip_lib_path)
    _native._bind(so)
    return so


def call_and_message(lib, name, args):
    """(return value, skelly_hip_last_error()) of one call, made on a thread of
    its own: the message is per thread, and this process's main thread keeps
    the empty one that tests/test_abi.py looks at."""
    got = []

    def run():
        got.append(getattr(lib, name)(*args))
        got.append(lib.skelly_hip_last_error().decode())
    t = threading.Thread(target=run)
    t.start()
    t.join()
    return got


def _counts(argtypes):
    return [i for i, t in enumerate(argtypes) if t is ctypes.c_longlong]


def _null_call(argtypes, counts):
    """Arguments of one entry point: null pointers, scalars of the defaults'
    size, `counts` in the count positions."""
    counts = iter(counts)
    return [next(counts) if t is ctypes.c_longlong else 1e-3 if t is ctypes.c_double else None
            for t in argtypes]


# every int-returning entry point that takes a count: the eight pair kernels'
# host and device forms, the normal-density pair, the two dense builders
COUNTED = sorted(n for n, (restype, argtypes) in _native.SIGNATURES.items()
                 if restype is ctypes.c_int and _counts(argtypes) and "probe" not in n)


def test_counted_entry_points_are_the_ones_the_header_has():
    pair = [f"skelly_{k}_{form}" for k in _native.PAIR_FAMILY for form in ("host", "device")]
    assert COUNTED == sorted(pair + [
        "skelly_stresslet_normal_density_host", "skelly_stresslet_normal_density_device",
        "skelly_stresslet_times_normal_device", "skelly_oseen_tensor_batched_device"])


def _negative_calls():
    for name in COUNTED:
        k = len(_counts(_native.SIGNATURES[name][1]))
        for bad in range(k):
            yield name, tuple(-1 if i == bad else 5 for i in range(k))


@pytest.mark.parametrize("name,counts", list(_negative_calls()))
def test_negative_count_is_an_error_before_any_launch(lib, name, counts):
    argtypes = _native.SIGNATURES[name][1]
    rc, msg = call_and_message(lib, name, _null_call(argtypes, counts))
    assert rc != 0
    assert msg.startswith(name + ":") and "negative" in msg, msg


@pytest.mark.parametrize("name", COUNTED)
def test_far_negative_source_count(lib, name):
    """A count under minus one record group, which once sized the workspace."""
    argtypes = _native.SIGNATURES[name][1]
    counts = [-(1 << 40)] + [5] * (len(_counts(argtypes)) - 1)
    rc, msg = call_and_message(lib, name, _null_call(argtypes, counts))
    assert rc != 0 and msg.startswith(name + ":") and "negative" in msg, msg


@pytest.mark.parametrize("name", COUNTED)
def test_zero_count_is_no_error(lib, name):
    """No targets (no points, no fibers): nothing to do, 0, and nothing is
    touched. The last count of every entry point is the one that empties the
    output."""
    argtypes = _native.SIGNATURES[name][1]
    k = len(_counts(argtypes))
    rc, msg = call_and_message(lib, name, _null_call(argtypes, [5] * (k - 1) + [0]))
    assert rc == 0 and msg == ""


@pytest.mark.parametrize("name", ["stokeslet_direct_gpu_impl", "stresslet_direct_gpu_impl"])
@pytest.mark.parametrize("n_src,n_trg", [(-1, 4), (5, -1)])
def test_void_wrapper_leaves_u_trg_untouched(lib, name, n_src, n_trg):
    sentinel = -12345.678
    u = np.full((4, 3), sentinel)
    before = u.copy()
    _, msg = call_and_message(lib, name,
                              (None, None, n_src, None, u.ctypes.data_as(_native._DP), n_trg))
    assert np.array_equal(u, before)
    assert msg.startswith(name + ":") and "negative" in msg, msg
