"""Host-side mirror of SkellySim's evaluator interface.

Mirrors kernels::Evaluator (reference include/kernels.hpp:14-15):

    Evaluator(r_sl, r_dl, r_trg, f_sl, f_dl, eta) -> u [n_trg x 3]

Stokeslet consumers pass single-layer sources (r_sl, f_sl) with r_dl/f_dl
empty; stresslet consumers the reverse (see reference
tests/core/kernel_test.cpp:40,65). Results are divided by eta, exactly as the
reference host wrappers do (src/core/kernels.cpp:358,365).

Array convention: an (n, 3) C-order numpy array is byte-identical to the
reference's col-major 3 x n Eigen matrix (per-point xyz contiguous); (3, n)
inputs are accepted and transposed. Stresslet strengths are (n, 9).

Backend selection mirrors FiberContainerBase::set_evaluator
(src/core/fiber_container_base.cpp:20-33): set_evaluator("HIP") returns the
callables below; "CPU"/"GPU"/"FMM" raise — this engine IS the GPU backend and
ships no FMM or CPU compute path.
"""

import ctypes
import math

import numpy as np

from . import _native

_DP = ctypes.POINTER(ctypes.c_double)

class _Pair:
    """One pair kernel as this module sees it: the entry points
    skelly_<symbol>_host / skelly_<symbol>_device (argument order:
    _native.PAIR_FAMILY / PRESSURE_FAMILY), the doubles per source of its
    strength array and the per-target shape of its result. `symbol` is also the _native.check label.
    Everything a call needs is worked out here, once."""

    def __init__(self, symbol, srcdim, out):
        self.symbol, self.srcdim, self.out = symbol, srcdim, out
        self.host, self.device = f"skelly_{symbol}_host", f"skelly_{symbol}_device"
        self.strength_first = _native.strength_first(symbol)
        # argument names for error messages
        self.names = ("r_src", "f_src" if self.strength_first else "density")


_STOKESLET = _Pair("stokeslet", 3, (3,))
_STRESSLET = _Pair("stresslet", 9, (3,))
_OSEEN = _Pair("oseen_contract", 3, (3,))
_ROTLET = _Pair("rotlet", 3, (3,))
_STOKESLET_GRAD = _Pair("stokeslet_grad", 3, (3, 3))
_STRESSLET_GRAD = _Pair("stresslet_grad", 9, (3, 3))
_OSEEN_GRAD = _Pair("oseen_contract_grad", 3, (3, 3))
_ROTLET_GRAD = _Pair("rotlet_grad", 3, (3, 3))
_STOKESLET_PRESSURE = _Pair("stokeslet_pressure", 3, ())
_STRESSLET_PRESSURE = _Pair("stresslet_pressure", 9, ())
_OSEEN_PRESSURE = _Pair("oseen_contract_pressure", 3, ())


def _rows(a, dim, name):
    """Normalize to a C-contiguous (n, dim) fp64 array (accepts (dim, n))."""
    if a is None:
        return np.empty((0, dim))
    a = np.asarray(a, dtype=np.float64)
    if a.size == 0:
        return np.empty((0, dim))
    if a.ndim != 2:
        raise ValueError(f"{name}: expected 2-D array, got shape {a.shape}")
    if a.shape[1] != dim:
        if a.shape[0] == dim:
            a = a.T
        else:
            raise ValueError(f"{name}: expected (n, {dim}) or ({dim}, n), got {a.shape}")
    return np.ascontiguousarray(a)


def _ptr(a):
    return a.ctypes.data_as(_DP)


def _same_length(n, name, n_src, src_name):
    """A per-source array has one row per source: the library reads n_src rows
    of it, whatever it holds."""
    if n != n_src:
        raise ValueError(f"{name}: {n} rows for the {n_src} of {src_name}")


def _pair_args(k, r_src, f_src, n_src, r_trg, out, n_trg):
    """The leading arguments in the order k's entry points take them."""
    if k.strength_first:
        return r_src, f_src, n_src, r_trg, out, n_trg
    return r_src, r_trg, f_src, out, n_src, n_trg


def _host_pair(k, r_src, f_src, r_trg, scalars, names=None):
    """Kernel k on host arrays: normalize, call skelly_<symbol>_host, return
    (n_trg,) + k.out. `scalars` are the trailing doubles (eta[, reg, eps])."""
    names = names or k.names
    src = _rows(r_src, 3, names[0])
    f = _rows(f_src, k.srcdim, names[1])
    trg = _rows(r_trg, 3, "r_trg")
    _same_length(len(f), names[1], len(src), names[0])
    out = np.zeros((len(trg),) + k.out)
    fn = getattr(_native.lib(), k.host)
    rc = fn(*_pair_args(k, _ptr(src), _ptr(f), len(src), _ptr(trg), _ptr(out), len(trg)),
            *map(float, scalars))
    _native.check(rc, k.symbol)
    return out


def stokeslet_direct_gpu(r_sl, r_dl, r_trg, f_sl, f_dl, eta):
    """Evaluator-signature Stokeslet (mirrors kernels::stokeslet_direct_gpu,
    src/core/kernels.cpp:361-366): uses (r_sl, f_sl), returns u/eta."""
    return _host_pair(_STOKESLET, r_sl, f_sl, r_trg, (eta,), names=("r_sl", "f_sl"))


def stresslet_direct_gpu(r_sl, r_dl, r_trg, f_sl, f_dl, eta):
    """Evaluator-signature stresslet (mirrors kernels::stresslet_direct_gpu,
    src/core/kernels.cpp:354-359): uses (r_dl, f_dl), returns u/eta."""
    return _host_pair(_STRESSLET, r_dl, f_dl, r_trg, (eta,), names=("r_dl", "f_dl"))


def oseen_contract_direct_gpu(r_src, r_trg, density, eta=1.0, reg=5e-3, epsilon_distance=1e-5):
    """Mirrors kernels::oseen_tensor_contract_direct (kernels.cpp:85-131;
    defaults kernels.hpp:34-35)."""
    return _host_pair(_OSEEN, r_src, density, r_trg, (eta, reg, epsilon_distance))


def rotlet_gpu(r_src, r_trg, density, eta=1.0, reg=5e-3, epsilon_distance=1e-5):
    """Mirrors kernels::rotlet (kernels.cpp:206-242; defaults kernels.hpp:44-45)."""
    return _host_pair(_ROTLET, r_src, density, r_trg, (eta, reg, epsilon_distance))


# Velocity gradients, host arrays: (n_trg, 3, 3) with G[t, i, j] = du_i/dx_j at
# target t, from the analytic gradient kernels (one pass, no differencing).

def stokeslet_grad(r_src, f_src, r_trg, eta):
    """Gradient of the Stokeslet velocity (stokeslet_direct_gpu's field)."""
    return _host_pair(_STOKESLET_GRAD, r_src, f_src, r_trg, (eta,))


def stresslet_grad(r_src, f_src, r_trg, eta):
    """Gradient of the stresslet velocity (stresslet_direct_gpu's field)."""
    return _host_pair(_STRESSLET_GRAD, r_src, f_src, r_trg, (eta,))


def oseen_contract_grad(r_src, r_trg, density, eta=1.0, reg=5e-3, epsilon_distance=1e-5):
    """Gradient of oseen_contract_direct_gpu's field (exact inside each branch
    of the regularization)."""
    return _host_pair(_OSEEN_GRAD, r_src, density, r_trg, (eta, reg, epsilon_distance))


def rotlet_grad(r_src, r_trg, density, eta=1.0, reg=5e-3, epsilon_distance=1e-5):
    """Gradient of rotlet_gpu's field."""
    return _host_pair(_ROTLET_GRAD, r_src, density, r_trg, (eta, reg, epsilon_distance))


# Pressures, host arrays: (n_trg,), the Stokes pressure that goes with the
# velocity of the same sources (prefactor 1/(4 pi); no eta: no pressure depends
# on it). sigma = -p I + eta (G + G^T) with G from the gradient forms. The
# rotlet's pressure is identically zero, so it has no function here.

def stokeslet_pressure(r_src, f_src, r_trg):
    """p = 1/(4 pi) sum (f.d) / r^3 of stokeslet_direct_gpu's field, d = t - s."""
    return _host_pair(_STOKESLET_PRESSURE, r_src, f_src, r_trg, ())


def stresslet_pressure(r_src, f_src, r_trg):
    """p = 1/(4 pi) sum [tr(S) / r^3 - 3 (d^T S d) / r^5] of
    stresslet_direct_gpu's field, S_kl = f_src[:, 3k + l]."""
    return _host_pair(_STRESSLET_PRESSURE, r_src, f_src, r_trg, ())


def oseen_contract_pressure(r_src, r_trg, density, reg=5e-3, epsilon_distance=1e-5):
    """Pressure of oseen_contract_direct_gpu's field: the Stokeslet's
    expression with that kernel's regularized distance."""
    return _host_pair(_OSEEN_PRESSURE, r_src, density, r_trg, (reg, epsilon_distance))


# Nearest source, host arrays. Not a sum: per target the smallest squared
# distance to an eligible source and the index of that source (the lowest
# among equals); +inf and -1 where there is none. With groups a source is
# eligible when its group id differs from the target's.

def _groups(src_group, trg_group, n_src, n_trg, convert):
    """Both group arrays as `convert` makes them, or (None, None): the library
    takes both or neither."""
    if (src_group is None) != (trg_group is None):
        raise ValueError("src_group and trg_group: pass both or neither")
    if src_group is None:
        return None, None
    sg, tg = convert(src_group, "src_group"), convert(trg_group, "trg_group")
    _same_length(sg.shape[0], "src_group", n_src, "r_src")
    _same_length(tg.shape[0], "trg_group", n_trg, "r_trg")
    return sg, tg


def _host_group(g, name):
    g = np.ascontiguousarray(np.asarray(g).reshape(-1))
    if g.dtype.kind not in "iu":
        raise TypeError(f"{name}: expected integer group ids, got {g.dtype}")
    return g.astype(np.int64, copy=False)


def nearest(r_src, r_trg, src_group=None, trg_group=None):
    """(d2 float64 (n_trg,), index int64 (n_trg,)) of skelly_nearest_host
    (include/skelly_hip.h states the tie, +inf / -1 and NaN rules)."""
    src, trg = _rows(r_src, 3, "r_src"), _rows(r_trg, 3, "r_trg")
    sg, tg = _groups(src_group, trg_group, len(src), len(trg), _host_group)
    d2 = np.empty(len(trg))
    index = np.empty(len(trg), dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = _native.lib().skelly_nearest_host(ptr(src), ptr(sg), len(src), ptr(trg), ptr(tg),
                                           len(trg), ptr(d2), ptr(index))
    _native.check(rc, "nearest")
    return d2, index


class Evaluator:
    """Callable mirroring kernels::Evaluator for one kernel type."""

    def __init__(self, fn):
        self._fn = fn

    def __call__(self, r_sl, r_dl, r_trg, f_sl, f_dl, eta):
        return self._fn(r_sl, r_dl, r_trg, f_sl, f_dl, eta)

    # the nearest-source search is no kernel type of the reference's: every
    # evaluator offers the one host form
    nearest = staticmethod(nearest)


def set_evaluator(name):
    """Mirror of the reference's string-keyed backend selection
    (fiber_container_base.cpp:20-33, periphery.cpp:337-352). Returns
    (stokeslet_evaluator, stresslet_evaluator) for name == "HIP"."""
    if name == "HIP":
        return Evaluator(stokeslet_direct_gpu), Evaluator(stresslet_direct_gpu)
    if name in ("CPU", "GPU", "FMM"):
        raise NotImplementedError(
            f'evaluator "{name}": skellysim_amd is the MI355X-native GPU backend; '
            'use "HIP". The reference CPU/FMM paths are out of scope '
            "(SURVEY.md §8) and the CPU restatement under oracle/ is test "
            "infrastructure only.")
    raise ValueError(f"unknown evaluator {name!r}")


def stresslet_times_normal_times_density(r_src, normals, density, reg=5e-3,
                                         epsilon_distance=1e-5):
    """Mirrors kernels::stresslet_times_normal_times_density
    (kernels.cpp:307-334; defaults kernels.hpp:50-51). Returns (n, 3);
    no eta dependence (factor -3/(4 pi))."""
    src = _rows(r_src, 3, "r_src")
    nrm = _rows(normals, 3, "normals")
    rho = _rows(density, 3, "density")
    _same_length(len(nrm), "normals", len(src), "r_src")
    _same_length(len(rho), "density", len(src), "r_src")
    out = np.zeros((len(src), 3))
    rc = _native.lib().skelly_stresslet_normal_density_host(
        _ptr(src), _ptr(nrm), _ptr(rho), _ptr(out), len(src),
        float(reg), float(epsilon_distance))
    _native.check(rc, "stresslet_normal_density")
    return out


# ---------------------------------------------------------------------------
# torch device-tensor API (async on the current torch stream)
# ---------------------------------------------------------------------------

def _dev_rows(t, dim, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError(f"{name}: expected a CUDA torch tensor (no CPU fallback)")
    if t.dtype != torch.float64:
        raise TypeError(f"{name}: expected float64, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != dim:
        raise ValueError(f"{name}: expected (n, {dim}), got {tuple(t.shape)}")
    return t.contiguous()


def _dev_result(out, shape, like):
    """The result tensor of `shape`: a fresh one on `like`'s device, or the
    caller's `out` if a kernel can write it as is."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=like.device)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64
            and out.is_contiguous() and out.numel() == math.prod(shape)):
        raise ValueError("out: expected a contiguous float64 CUDA tensor of "
                         f"({', '.join(map(str, shape))})")
    return out


def _dev_out(out, r_trg, shape):
    """_dev_result for a pair kernel: (n_trg,) + shape."""
    # (shape[0] of a tensor: len() costs several times this)
    return _dev_result(out, (r_trg.shape[0],) + shape, r_trg)


def _dptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_pair(k, r_src, f_src, r_trg, out, scalars):
    """Kernel k on device tensors, async on torch's current stream: validate,
    call skelly_<symbol>_device, return `out` ((n_trg,) + k.out)."""
    r_src = _dev_rows(r_src, 3, "r_src")
    f_src = _dev_rows(f_src, k.srcdim, k.names[1])
    r_trg = _dev_rows(r_trg, 3, "r_trg")
    _same_length(f_src.shape[0], k.names[1], r_src.shape[0], "r_src")
    out = _dev_out(out, r_trg, k.out)
    fn = getattr(_native.lib(), k.device)
    rc = fn(*_pair_args(k, _dptr(r_src), _dptr(f_src), r_src.shape[0], _dptr(r_trg), _dptr(out),
                        r_trg.shape[0]),
            *map(float, scalars), _stream_ptr())
    _native.check(rc, k.symbol + "_device")
    return out


def stokeslet_device(r_src, f_src, r_trg, eta, out=None):
    """Stokeslet on device tensors (n,3); returns (n_trg,3) velocities
    (fully scaled 1/(8 pi eta)). Async on torch's current stream."""
    return _device_pair(_STOKESLET, r_src, f_src, r_trg, out, (eta,))


def stresslet_device(r_src, f_src, r_trg, eta, out=None):
    return _device_pair(_STRESSLET, r_src, f_src, r_trg, out, (eta,))


def oseen_contract_device(r_src, r_trg, density, eta=1.0, reg=5e-3, epsilon_distance=1e-5,
                          out=None):
    return _device_pair(_OSEEN, r_src, density, r_trg, out, (eta, reg, epsilon_distance))


def stresslet_normal_density_device(r_src, normals, density, r_trg=None, reg=5e-3,
                                    epsilon_distance=1e-5, out=None):
    """Device form of stresslet_times_normal_times_density; r_trg defaults to
    r_src (the reference's self form)."""
    import torch
    r_src = _dev_rows(r_src, 3, "r_src")
    normals = _dev_rows(normals, 3, "normals")
    density = _dev_rows(density, 3, "density")
    r_trg = r_src if r_trg is None else _dev_rows(r_trg, 3, "r_trg")
    _same_length(len(normals), "normals", len(r_src), "r_src")
    _same_length(len(density), "density", len(r_src), "r_src")
    nd = torch.cat([normals, density], dim=1).contiguous()
    out = _dev_out(out, r_trg, (3,))
    rc = _native.lib().skelly_stresslet_normal_density_device(
        _dptr(r_src), _dptr(nd), _dptr(r_trg), _dptr(out), len(r_src), len(r_trg),
        float(reg), float(epsilon_distance), _stream_ptr())
    _native.check(rc, "stresslet_normal_density_device")
    return out


def stresslet_times_normal_device(pts, normals, reg=5e-3, epsilon_distance=1e-5, out=None):
    """Dense stresslet_times_normal builder (kernels.cpp:264-287).
    pts, normals: (n, 3) CUDA fp64 -> (3n, 3n)."""
    import torch
    pts = _dev_rows(pts, 3, "pts")
    normals = _dev_rows(normals, 3, "normals")
    n = len(pts)
    _same_length(len(normals), "normals", n, "pts")
    out = _dev_result(out, (3 * n, 3 * n), pts)
    rc = _native.lib().skelly_stresslet_times_normal_device(
        _dptr(pts), _dptr(normals), _dptr(out), n, float(reg), float(epsilon_distance),
        _stream_ptr())
    _native.check(rc, "stresslet_times_normal_device")
    return out


def oseen_tensor_batched_device(pts, eta=1.0, reg=5e-3, epsilon_distance=1e-5, out=None):
    """Batched dense self-Oseen-tensor builder (kernels.cpp:146-195; the
    per-fiber self-stokeslet, fiber_finite_difference.cpp:56).
    pts: (nf, n, 3) CUDA fp64 -> G (nf, 3n, 3n)."""
    import torch
    if not (isinstance(pts, torch.Tensor) and pts.is_cuda and pts.dtype == torch.float64
            and pts.dim() == 3 and pts.shape[2] == 3):
        raise TypeError("pts: expected (nf, n, 3) fp64 CUDA tensor")
    pts = pts.contiguous()
    nf, n = pts.shape[0], pts.shape[1]
    out = _dev_result(out, (nf, 3 * n, 3 * n), pts)
    rc = _native.lib().skelly_oseen_tensor_batched_device(
        _dptr(pts), _dptr(out), nf, n, float(eta), float(reg), float(epsilon_distance),
        _stream_ptr())
    _native.check(rc, "oseen_tensor_batched_device")
    return out


def rotlet_device(r_src, r_trg, density, eta=1.0, reg=5e-3, epsilon_distance=1e-5, out=None):
    return _device_pair(_ROTLET, r_src, density, r_trg, out, (eta, reg, epsilon_distance))


# ---------------------------------------------------------------------------
# velocity gradients on device tensors: (n_trg, 3, 3), G[t, i, j] = du_i/dx_j
# ---------------------------------------------------------------------------

def stokeslet_grad_device(r_src, f_src, r_trg, eta, out=None):
    """Gradient of stokeslet_device's field. Async on torch's current stream."""
    return _device_pair(_STOKESLET_GRAD, r_src, f_src, r_trg, out, (eta,))


def stresslet_grad_device(r_src, f_src, r_trg, eta, out=None):
    """Gradient of stresslet_device's field."""
    return _device_pair(_STRESSLET_GRAD, r_src, f_src, r_trg, out, (eta,))


def oseen_contract_grad_device(r_src, r_trg, density, eta=1.0, reg=5e-3,
                               epsilon_distance=1e-5, out=None):
    """Gradient of oseen_contract_device's field."""
    return _device_pair(_OSEEN_GRAD, r_src, density, r_trg, out, (eta, reg, epsilon_distance))


def rotlet_grad_device(r_src, r_trg, density, eta=1.0, reg=5e-3, epsilon_distance=1e-5,
                       out=None):
    """Gradient of rotlet_device's field."""
    return _device_pair(_ROTLET_GRAD, r_src, density, r_trg, out, (eta, reg, epsilon_distance))


# ---------------------------------------------------------------------------
# pressures on device tensors: (n_trg,); no eta (see the host forms)
# ---------------------------------------------------------------------------

def stokeslet_pressure_device(r_src, f_src, r_trg, out=None):
    """Pressure of stokeslet_device's field. Async on torch's current stream."""
    return _device_pair(_STOKESLET_PRESSURE, r_src, f_src, r_trg, out, ())


def stresslet_pressure_device(r_src, f_src, r_trg, out=None):
    """Pressure of stresslet_device's field."""
    return _device_pair(_STRESSLET_PRESSURE, r_src, f_src, r_trg, out, ())


def oseen_contract_pressure_device(r_src, r_trg, density, reg=5e-3, epsilon_distance=1e-5,
                                   out=None):
    """Pressure of oseen_contract_device's field."""
    return _device_pair(_OSEEN_PRESSURE, r_src, density, r_trg, out, (reg, epsilon_distance))


# ---------------------------------------------------------------------------
# nearest source on device tensors
# ---------------------------------------------------------------------------

def _dev_group(g, name):
    import torch
    if not (isinstance(g, torch.Tensor) and g.is_cuda):
        raise TypeError(f"{name}: expected a CUDA torch tensor (no CPU fallback)")
    if g.dtype != torch.int64:
        raise TypeError(f"{name}: expected int64, got {g.dtype}")
    if g.dim() != 1:
        raise ValueError(f"{name}: expected (n,), got {tuple(g.shape)}")
    return g.contiguous()


def nearest_device(r_src, r_trg, src_group=None, trg_group=None):
    """nearest() on device tensors: (d2 float64 (n_trg,), index int64
    (n_trg,)), asynchronous on torch's current stream. Groups are int64
    tensors (n,), both or neither."""
    import torch
    r_src = _dev_rows(r_src, 3, "r_src")
    r_trg = _dev_rows(r_trg, 3, "r_trg")
    sg, tg = _groups(src_group, trg_group, r_src.shape[0], r_trg.shape[0], _dev_group)
    n_trg = r_trg.shape[0]
    d2 = torch.empty((n_trg,), dtype=torch.float64, device=r_trg.device)
    index = torch.empty((n_trg,), dtype=torch.int64, device=r_trg.device)
    ptr = lambda t: None if t is None else _dptr(t)
    rc = _native.lib().skelly_nearest_device(_dptr(r_src), ptr(sg), r_src.shape[0], _dptr(r_trg),
                                             ptr(tg), n_trg, _dptr(d2), _dptr(index),
                                             _stream_ptr())
    _native.check(rc, "nearest_device")
    return d2, index


# ---------------------------------------------------------------------------
# streamlines on device tensors: one launch, a workgroup per seed and direction
# ---------------------------------------------------------------------------

# the four source sets of the tracer, in the library's order: (name, doubles
# per source of the strength, label of the strength in error messages)
TRACE_SETS = (("stokeslet", 3, "forces"), ("stresslet", 9, "f_dl"),
              ("rotlet", 3, "torques"), ("oseen", 3, "forces"))
# status codes of a traced job (include/skelly_hip.h)
TRACE_DONE, TRACE_SINGULAR, TRACE_FULL, TRACE_GAVE_UP = 0, 1, 2, 3


def _background9(background):
    """(uniform, scale_factor, components) -> the 9 host doubles the library
    reads, or None."""
    if background is None:
        return None
    uniform, scale, components = background
    comp = np.asarray(components, dtype=np.int64).reshape(3)
    if ((comp < 0) | (comp > 2)).any():
        raise ValueError(f"background components: expected 0, 1 or 2, got {comp.tolist()}")
    return np.concatenate([np.asarray(uniform, np.float64).reshape(3),
                           np.asarray(scale, np.float64).reshape(3), comp.astype(np.float64)])


def _trace_lines_device(entry, seeds, eta, stokeslet, stresslet, rotlet, oseen, background,
                        bodies, dt_init, t_final, abs_err, rel_err, back_integrate, max_points,
                        reg, epsilon_distance):
    """The two tracers' one body: `entry` names the library function
    (skelly_<entry>), which decides the field."""
    import torch
    seeds = _dev_rows(seeds, 3, "seeds")
    args = []
    for (name, dim, label), pair in zip(TRACE_SETS, (stokeslet, stresslet, rotlet, oseen)):
        if pair is None:
            args += [None, None, 0]
            continue
        r = _dev_rows(pair[0], 3, f"{name} r_src")
        f = _dev_rows(pair[1], dim, f"{name} {label}")
        _same_length(f.shape[0], f"{name} {label}", r.shape[0], f"{name} r_src")
        args += [r, f, r.shape[0]]
    if bodies is not None:
        bodies = _dev_rows(bodies, 10, "bodies")
    bg = _background9(background)
    max_points = int(max_points)
    if max_points < 1:
        raise ValueError(f"max_points: expected at least 1, got {max_points}")
    n = seeds.shape[0]
    n_jobs = n * (2 if back_integrate else 1)
    out = {
        "x": torch.empty((n_jobs, max_points, 3), dtype=torch.float64, device=seeds.device),
        "t": torch.empty((n_jobs, max_points), dtype=torch.float64, device=seeds.device),
        "val": torch.empty((n_jobs, max_points, 3), dtype=torch.float64, device=seeds.device),
        "count": torch.empty((n_jobs,), dtype=torch.int32, device=seeds.device),
        "status": torch.empty((n_jobs,), dtype=torch.int32, device=seeds.device),
    }
    ptr = lambda t: None if t is None else _dptr(t)
    rc = getattr(_native.lib(), f"skelly_{entry}")(
        *[a if isinstance(a, int) else ptr(a) for a in args],
        None if bg is None else _ptr(bg), ptr(bodies), 0 if bodies is None else bodies.shape[0],
        _dptr(seeds), n, int(bool(back_integrate)),
        float(eta), float(reg), float(epsilon_distance),
        float(dt_init), float(t_final), float(abs_err), float(rel_err), max_points,
        *[_dptr(out[k]) for k in ("x", "t", "val", "count", "status")], _stream_ptr())
    _native.check(rc, entry)
    return out


def trace_streamlines_device(seeds, eta, stokeslet=None, stresslet=None, rotlet=None, oseen=None,
                             background=None, bodies=None, dt_init=0.1, t_final=1.0,
                             abs_err=1e-10, rel_err=1e-6, back_integrate=True, max_points=4096,
                             reg=5e-3, epsilon_distance=1e-5):
    """Streamlines of the summed field from every row of `seeds` (n, 3), in
    one kernel launch on torch's current stream (asynchronous, no
    synchronization; skelly_trace_streamlines_device, include/skelly_hip.h).

    stokeslet / stresslet / rotlet / oseen: (r_src (m, 3), strength (m, 3 or
    9)) device tensors or None, the fields of stokeslet_device,
    stresslet_device, rotlet_device and oseen_contract_device. background:
    (uniform, scale_factor, components) host values, u_j += uniform_j +
    x[components_j] * scale_factor_j. bodies: (n_b, 10) device tensor of rows
    {centre, radius, velocity, angular velocity}; a point inside one moves
    rigidly with it.

    Returns a dict of device tensors per job (job j < n runs seed j forward,
    job n + j backward when back_integrate): x (n_jobs, max_points, 3),
    t (n_jobs, max_points), val as x (the velocity at the points), count and
    status (n_jobs,) int32. Rows past count[job] are not written."""
    return _trace_lines_device("trace_streamlines_device", seeds, eta, stokeslet, stresslet,
                               rotlet, oseen, background, bodies, dt_init, t_final, abs_err,
                               rel_err, back_integrate, max_points, reg, epsilon_distance)


def trace_vortexlines_device(seeds, eta, stokeslet=None, stresslet=None, rotlet=None, oseen=None,
                             background=None, bodies=None, dt_init=0.1, t_final=1.0,
                             abs_err=1e-10, rel_err=1e-6, back_integrate=True, max_points=4096,
                             reg=5e-3, epsilon_distance=1e-5):
    """Vortex lines of the same field: trace_streamlines_device's arguments
    and dict, with dx/dt and `val` the vorticity curl u, summed analytically
    through the gradient kernels (skelly_trace_vortexlines_device). A point
    inside a body has twice its angular velocity. Status 1 remains a stop on
    the velocity, |u| > 1e3 at a recorded point."""
    return _trace_lines_device("trace_vortexlines_device", seeds, eta, stokeslet, stresslet,
                               rotlet, oseen, background, bodies, dt_init, t_final, abs_err,
                               rel_err, back_integrate, max_points, reg, epsilon_distance)


def join_streamlines(x, t, val, count, status, n_seeds):
    """The per-job arrays of a trace (host arrays, jobs as the library orders
    them) as one line per seed, joined as the reference's
    join_back_and_forward does (streamline.cpp:56-65): the backward path
    reversed and without the seed it shares with the forward path, then the
    forward path. Returns a list of dicts {x (m, 3), val (m, 3), time (m,),
    status}, status being the larger of the two jobs' codes (0 only when both
    directions reached t_final)."""
    x, t, val = np.asarray(x), np.asarray(t), np.asarray(val)
    count, status = np.asarray(count), np.asarray(status)
    back = len(count) == 2 * n_seeds
    lines = []
    for i in range(n_seeds):
        c = int(count[i])
        px, pt, pv, st = x[i, :c], t[i, :c], val[i, :c], int(status[i])
        if back:
            j, cb = n_seeds + i, int(count[n_seeds + i])
            px = np.concatenate([x[j, 1:cb][::-1], px])
            pt = np.concatenate([t[j, 1:cb][::-1], pt])
            pv = np.concatenate([val[j, 1:cb][::-1], pv])
            st = max(st, int(status[j]))
        lines.append({"x": px, "val": pv, "time": pt, "status": st})
    return lines
