"""ctypes binding to the in-tree HIP extension (libskellyhip.so).

The extension is built in-tree by `make -C skellysim_amd/csrc` (driven by
__graft_entry__.build()) so the .so travels with the repo snapshot. If it is
missing, every entry point raises RuntimeError — the product path never falls
back to a CPU implementation.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libskellyhip.so")

_lib = None
_load_error = None

_I = ctypes.c_int
_D = ctypes.c_double
_DP = ctypes.POINTER(ctypes.c_double)
_LL = ctypes.c_longlong
_PV = ctypes.c_void_p

# The two argument orders of the pair entry points (include/skelly_hip.h); `p`
# is the pointer type: double* in the host forms, void* in the device forms,
# which end in one more void* for the stream.
STRENGTH = "strength"  # (r_src, f_src, n_src, r_trg, out, n_trg, eta)
DENSITY = "density"    # (r_src, r_trg, density, out, n_src, n_trg, eta, reg, eps)
_PAIR_ARGS = {
    STRENGTH: lambda p: [p, p, _LL, p, p, _LL, _D],
    DENSITY: lambda p: [p, p, p, p, _LL, _LL, _D, _D, _D],
}
# skelly_<name>_host and skelly_<name>_device exist for every key
PAIR_FAMILY = {
    "stokeslet": STRENGTH, "stresslet": STRENGTH,
    "stokeslet_grad": STRENGTH, "stresslet_grad": STRENGTH,
    "oseen_contract": DENSITY, "rotlet": DENSITY,
    "oseen_contract_grad": DENSITY, "rotlet_grad": DENSITY,
}


class PressureCount(ctypes.c_longlong):
    """The `long long` counts of the pressure entry points. A type of its own
    keeps those entry points apart from the ones above wherever entry points
    are enumerated by the type of their counts: tests/test_evaluator_arguments.py
    lists the velocity and gradient forms that way, in sorted order and with its
    cases numbered by position, and keeps exactly that list;
    tests/test_pressure_cpu.py makes the same checks on the pressure forms."""


# The pressures take the same two orders without eta (no pressure depends on it).
STRENGTH_NO_ETA = "strength_no_eta"  # (r_src, f_src, n_src, r_trg, out, n_trg)
DENSITY_NO_ETA = "density_no_eta"    # (r_src, r_trg, density, out, n_src, n_trg, reg, eps)
_N = PressureCount
_PRESSURE_ARGS = {
    STRENGTH_NO_ETA: lambda p: [p, p, _N, p, p, _N],
    DENSITY_NO_ETA: lambda p: [p, p, p, p, _N, _N, _D, _D],
}
# skelly_<name>_host and skelly_<name>_device exist for every key here too
PRESSURE_FAMILY = {
    "stokeslet_pressure": STRENGTH_NO_ETA, "stresslet_pressure": STRENGTH_NO_ETA,
    "oseen_contract_pressure": DENSITY_NO_ETA,
}


class TraceCount(ctypes.c_longlong):
    """The `long long` counts of the streamline and vortex-line entry points: a type of its
    own for the reason PressureCount is one (tests/test_streamlines_cpu.py
    checks these entry points' argument contract)."""


def _trace_args(p, ip):
    """skelly_trace_streamlines_* and skelly_trace_vortexlines_*: p the double pointers, ip the int pointers.
    `background` is a host pointer in both forms."""
    t = TraceCount
    return ([p, p, t] * 4                       # sl, dl, rot, os: r, f, n
            + [_DP, p, t]                       # background (host), bodies, n_bodies
            + [p, t, _I]                        # seeds, n_seeds, back_integrate
            + [_D] * 3                          # eta, reg, epsilon_distance
            + [_D] * 4 + [t]                    # dt_init, t_final, abs_err, rel_err, max_points
            + [p, p, p, ip, ip])                # x, t, val, count, status


class NearestCount(ctypes.c_longlong):
    """The `long long` counts of the nearest-source entry points: a type of its
    own for the reason PressureCount is one (tests/test_nearest_cpu.py checks
    these entry points' argument contract)."""


def _nearest_args(p):
    """skelly_nearest_*: (r_src, src_group, n_src, r_trg, trg_group, n_trg, d2, index)."""
    return [p, p, NearestCount, p, p, NearestCount, p, p]


def strength_first(symbol):
    """Whether skelly_<symbol>_* take (r_src, f_src, n_src, r_trg, ...), the
    strength orders, and not (r_src, r_trg, density, ...)."""
    family = PAIR_FAMILY.get(symbol) or PRESSURE_FAMILY[symbol]
    return family in (STRENGTH, STRENGTH_NO_ETA)


# every function of include/skelly_hip.h: name -> (restype, argtypes)
SIGNATURES = {
    "skelly_set_persistent_ws": (None, [_I]),
    "skelly_persistent_ws_bytes": (_I, [_PV, ctypes.POINTER(_LL)]),
    "skelly_set_pair_fastpath": (None, [_I]),
    "skelly_set_pair_slices": (None, [_I]),
    "skelly_hip_version": (ctypes.c_char_p, []),
    "skelly_hip_last_error": (ctypes.c_char_p, []),
    "skelly_hip_device_count": (_I, []),
    "skelly_hip_set_device": (_I, [_I]),
    "skelly_hip_shutdown": (_I, []),
    "stokeslet_direct_gpu_impl": (None, [_DP, _DP, _I, _DP, _DP, _I]),
    "stresslet_direct_gpu_impl": (None, [_DP, _DP, _I, _DP, _DP, _I]),
    "skelly_stresslet_normal_density_host": (_I, [_DP, _DP, _DP, _DP, _LL, _D, _D]),
    "skelly_stresslet_normal_density_device": (_I, [_PV, _PV, _PV, _PV, _LL, _LL, _D, _D, _PV]),
    "skelly_stresslet_times_normal_device": (_I, [_PV, _PV, _PV, _LL, _D, _D, _PV]),
    "skelly_oseen_tensor_batched_device": (_I, [_PV, _PV, _LL, _LL, _D, _D, _D, _PV]),
    "skelly_fp64_peak_tflops": (_I, [_DP]),
    "skelly_issue_cost_probe": (_I, [_DP]),
    "skelly_rsq_accuracy_probe": (_I, [_PV, _PV, _PV, _LL, _PV]),
    "skelly_trace_streamlines_host": (_I, _trace_args(_DP, ctypes.POINTER(_I))),
    "skelly_trace_streamlines_device": (_I, _trace_args(_PV, _PV) + [_PV]),
    "skelly_trace_vortexlines_host": (_I, _trace_args(_DP, ctypes.POINTER(_I))),
    "skelly_trace_vortexlines_device": (_I, _trace_args(_PV, _PV) + [_PV]),
    "skelly_trace_block_size": (_I, []),
    "skelly_nearest_host": (_I, _nearest_args(_PV)),
    "skelly_nearest_device": (_I, _nearest_args(_PV) + [_PV]),
}
for _name, _family in PAIR_FAMILY.items():
    SIGNATURES[f"skelly_{_name}_host"] = (_I, _PAIR_ARGS[_family](_DP))
    SIGNATURES[f"skelly_{_name}_device"] = (_I, _PAIR_ARGS[_family](_PV) + [_PV])
for _name, _family in PRESSURE_FAMILY.items():
    SIGNATURES[f"skelly_{_name}_host"] = (_I, _PRESSURE_ARGS[_family](_DP))
    SIGNATURES[f"skelly_{_name}_device"] = (_I, _PRESSURE_ARGS[_family](_PV) + [_PV])


def _bind(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes


def lib():
    """The loaded extension; raises loudly if it is missing/unloadable."""
    global _lib, _load_error
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"skellysim_amd HIP extension not found at {_LIB_PATH}. "
                "Build it with `make -C skellysim_amd/csrc` (or run "
                "__graft_entry__.build()). The product path has no CPU fallback.")
        try:
            _lib = ctypes.CDLL(_LIB_PATH)
        except OSError as e:
            _load_error = e
            raise RuntimeError(f"failed to load {_LIB_PATH}: {e}") from e
        _bind(_lib)
    return _lib


def set_pair_fastpath(mode):
    """Mode of the pair kernels' unmasked fast path: 0 off (every pair goes
    through the r == 0 mask), 1 auto (default: on for launches whose blocks
    each walk >= 8192 sources), 2 always on. Results are bit-identical in
    every mode."""
    lib().skelly_set_pair_fastpath(int(mode))


def set_pair_slices(n):
    """Source-slice count of the pair kernels' split launches: 0 (default)
    lets the launch planner choose, n >= 1 forces exactly n slices (clamped
    to the source count). The count fixes the summation order, so results
    are bit-identical for equal counts and equal to rounding otherwise."""
    lib().skelly_set_pair_slices(int(n))


def check(rc, what):
    if rc != 0:
        err = lib().skelly_hip_last_error().decode()
        raise RuntimeError(f"{what} failed (rc={rc}): {err}")
