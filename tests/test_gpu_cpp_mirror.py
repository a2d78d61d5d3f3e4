"""Every function of include/skelly_evaluator.hpp, called from C++ by
tests/evaluator_probe.cpp: the eight evaluator functions, both factories, and
a factory asked for "FMM", which has to throw.

The gradient wrappers take (r_src, r_trg, f_src) and forward to C functions
that take (r_src, f_src, n, r_trg); swapped arguments would compile. So each
result is held to the kernel's bound against the longdouble reference and to
bit-equality with the Python host form of the same call, which also asserts
that an (n, 3) C-order array is the header's 3 x n column-major matrix and
that column t of a 9 x n_trg gradient is G[t] in row-major order.

The case is the near cloud (coincident and regularized pairs) with reg and eps
off their defaults, so that a wrapper that dropped them would show. The probe
is built with the host compiler the way examples/Makefile links cpp_dropin and
run once.

The program is also what a host-form caller looks like at its barest: a fresh
process, ten calls of different kernels back to back. That found launches
returning a wrong result now and then while they took their workspace from the
stream-ordered mempool ("Launch workspace"); every launch now takes
it from a persistent block by default, and this test keeps watch on that
default."""

import os
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import pair_cases as PC
import pair_reference as R
from test_gpu_pair_accuracy import EVALUATE, judge

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(REPO, "tests", "evaluator_probe.cpp")
INCLUDE = os.path.join(REPO, "include")
LIBDIR = os.path.join(REPO, "skellysim_amd")

CASE_NAME = "near_reg2e-3_eps3e-5_probe"
CASE = replace(PC.CASES["near"][0], reg=2e-3, eps=3e-5)

# the probe's results in its order: (label, kernel of PC.KERNELS, doubles a target)
RESULTS = [
    ("stokeslet_direct_gpu", "stokeslet", 3), ("stresslet_direct_gpu", "stresslet", 3),
    ("oseen_tensor_contract_direct", "oseen", 3), ("rotlet", "rotlet", 3),
    ("stokeslet_grad", "stokeslet_grad", 9), ("stresslet_grad", "stresslet_grad", 9),
    ("oseen_tensor_contract_grad", "oseen_grad", 9), ("rotlet_grad", "rotlet_grad", 9),
    ("make_stokeslet_evaluator", "stokeslet", 3), ("make_stresslet_evaluator", "stresslet", 3),
]


def write_case(path, c):
    with open(path, "wb") as f:
        np.array([c.n_src, len(c.r_trg)], np.int64).tofile(f)
        np.array([c.eta, c.reg, c.eps], np.float64).tofile(f)
        for a in (c.r_src, c.r_trg, c.f3, c.f9):
            np.ascontiguousarray(a, np.float64).tofile(f)


@pytest.fixture(scope="module")
def probe_results(hip_lib_path, tmp_path_factory):
    """{label: array} of one run of the probe on CASE, and its stdout."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("evaluator_probe")
    exe, case, out = (str(tmp / n) for n in ("evaluator_probe", "case.bin", "out.bin"))
    built = subprocess.run(
        [cxx, "-O2", "-std=c++17", "-I", INCLUDE, PROBE, "-L", LIBDIR, "-lskellyhip",
         "-Wl,-rpath," + LIBDIR, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    write_case(case, CASE)
    r = subprocess.run([exe, case, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"evaluator_probe failed ({r.returncode}): {r.stdout} {r.stderr}"
    flat = np.fromfile(out, np.float64)
    n_trg = len(CASE.r_trg)
    assert flat.size == n_trg * sum(width for _, _, width in RESULTS)
    results, at = {}, 0
    for label, _, width in RESULTS:
        shape = (n_trg, 3) if width == 3 else (n_trg, 3, 3)
        results[label] = flat[at:at + n_trg * width].reshape(shape)
        at += n_trg * width
    return results, r.stdout


@pytest.fixture(scope="module")
def ska(hip_lib_path):
    import skellysim_amd
    return skellysim_amd


@pytest.mark.parametrize("label,kernel,width", RESULTS)
def test_cpp_result_is_the_kernel_and_the_python_host_form(ska, probe_results, label, kernel,
                                                           width):
    got = probe_results[0][label]
    ref, A = PC.reference(CASE_NAME, kernel, CASE)
    judge(f"{kernel} {CASE_NAME} C++ {label}", got, ref, A,
          R.bound(A, CASE.n_src, 1, kernel))
    want = EVALUATE[kernel](ska, CASE)
    assert np.array_equal(got, want), \
        f"{label}: {np.count_nonzero(got != want)} entries differ from the Python host form"


def test_factories_refuse_fmm(probe_results):
    stdout = probe_results[1]
    assert 'make_stokeslet_evaluator("FMM") threw' in stdout
    assert 'make_stresslet_evaluator("FMM") threw' in stdout
