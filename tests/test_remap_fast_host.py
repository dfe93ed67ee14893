"""CPU guard on the default remap arithmetic's branch stability (no GPU needed).

The default arithmetic (FV3_FAST_ARITH, csrc/mappm_core.h) may take the other side of a
limiter comparison that sits within an ulp of its switching point.  That is harmless
where the limiter is continuous there, and not where it is not: ppm_limiters lmt 2
replaces a whole parabola when its minimum dips below zero (`fmin < 0`), so a parabola
whose minimum touches zero (a tracer with exact zeros on a regular grid) moves by a
quarter of the level's scale.  ``fast_arith_serves(iv, kord)`` (mappm_core.h) keeps the
calls that reach lmt 2 on the reference's arithmetic; this file holds it to that.

tests/native/mappm_host.cpp is compiled under FV3_FAST_ARITH with ROCm's clang++ (-mfma:
the policy's `fp contract(on)` then gives FMAs as on the device) and the device's
reciprocal emulated: the correctly rounded 1 / b moved one ulp up or down for a quarter
of the denominators each, and div_refined by the device's own FMA refinement.  This is
an emulation of the device's rounding, not the device; tests/test_remap_default_matrix.py
runs the same pool on the GPU.

Pool ("lattice" columns, where exact ties are common): delp = 256 * choice([1, 2, 4]),
q = 0.25 * integers(0, 6), km 20, kn 16, pe2 sorted uniform over
[0.8 pe1(1), 1.1 pe1(km+1)], default_rng(3); and the same with q shifted by -0.5, which
puts the ties on both sides of zero.  Bound: 1e-5 of the level's largest |reference|
(tests/parity.py), the project's contract.
"""
import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle.mappm import oracle_mappm
from tests.parity import assert_per_level

HOST_SRC = os.path.join(ROOT, "tests", "native", "mappm_host.cpp")
BUILD_DIR = os.path.join(ROOT, "tests", "_build")

KORDS = list(range(0, 8))
IVS = [-1, 0, 1, 2]
N_ADMITTED = 25_000   # per (kord, iv) the predicate admits, both pools
N_REJECTED = 150_000  # per rejected pair: kord 7 / iv 0 flips in about 1 column of 50,000


def _rocm_clang():
    for c in [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")] + sorted(
            glob.glob("/opt/rocm*/llvm/bin/clang++")):
        if os.path.exists(c):
            return c
    hipcc = shutil.which("hipcc")
    if hipcc:
        c = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang++")
        if os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def fast_host_lib():
    cxx = _rocm_clang()
    if cxx is None:
        pytest.skip("ROCm's clang++ not present")
    os.makedirs(BUILD_DIR, exist_ok=True)
    own = os.path.join(BUILD_DIR, f"libmappm_host_fast.{os.getpid()}.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-DFV3_FAST_ARITH",
                    "-DFV3_EMULATE_DEVICE_RCP", "-o", own, HOST_SRC], check=True)
    lib = ctypes.CDLL(own)
    os.unlink(own)  # the mapping stays valid; nothing is left behind
    lib.host_mappm.restype = ctypes.c_int
    lib.host_mappm.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    lib.host_fast_arith_serves.restype = ctypes.c_int
    lib.host_fast_arith_serves.argtypes = [ctypes.c_int, ctypes.c_int]
    return lib


def lattice_pool(ncol, shift=0.0, km=20, kn=16, seed=3):
    """(pe1 [km+1, ncol], q [km, ncol], pe2 [kn+1, ncol]) float32."""
    rng = np.random.default_rng(seed)
    delp = (256.0 * rng.choice([1, 2, 4], (km, ncol))).astype(np.float32)
    q = (0.25 * rng.integers(0, 6, (km, ncol)) - shift).astype(np.float32)
    pe1 = np.concatenate([np.full((1, ncol), 256, np.float32), 256 + np.cumsum(delp, 0, dtype=np.float32)])
    pe2 = np.sort(rng.uniform(0.8 * pe1[0], 1.1 * pe1[-1], (kn + 1, ncol)), 0).astype(np.float32)
    return pe1, q, pe2


def exceedances(got, ref, rtol=1e-5):
    """[level, column] -> mask of the values beyond rtol of their level's largest |ref|."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return ~(np.abs(g - r) <= rtol * np.abs(r).max(axis=1, keepdims=True))  # a NaN counts


def _host(lib, pe1, q, pe2, iv, kord):
    out = np.empty((pe2.shape[0] - 1, q.shape[1]), np.float32)
    assert lib.host_mappm(q.shape[0], pe1.ctypes.data, q.ctypes.data, pe2.shape[0] - 1, pe2.ctypes.data,
                          out.ctypes.data, q.shape[1], iv, kord) == 0
    return out


def test_predicate_follows_the_interior_limiter(fast_host_lib):
    """fast_arith_serves is false exactly where ppm_profile's interior layers reach
    ppm_limiters lmt 2 -- lmt = min(max(kord - 3, 0), 2 if iv == 0) unless kord == 6, and
    after Huynh's constraint (kord >= 7) for iv 0 only -- and for kord > 7 (cs_profile)."""
    for kord in range(-3, 18):
        for iv in (-2, -1, 0, 1, 2):
            if kord >= 7:
                lmt = 2 if iv == 0 else None
            elif kord == 6:
                lmt = None
            else:
                lmt = max(kord - 3, 0)
                lmt = min(lmt, 2) if iv == 0 else lmt
            want = kord <= 7 and lmt != 2
            assert bool(fast_host_lib.host_fast_arith_serves(iv, kord)) == want, (iv, kord)
    rejected = [(k, i) for k in KORDS for i in IVS if not fast_host_lib.host_fast_arith_serves(i, k)]
    assert rejected == [(5, -1), (5, 0), (5, 1), (5, 2), (7, 0)]


@pytest.mark.parametrize("shift", [0.0, 0.5], ids=["lattice", "straddling_zero"])
def test_admitted_calls_hold_1e5_on_the_lattice_pool(fast_host_lib, shift):
    """Every (kord <= 7, iv) the predicate admits: no value beyond 1e-5 per level of
    oracle_mappm under the emulated device rounding (worst seen 1.2e-6)."""
    pe1, q, pe2 = lattice_pool(N_ADMITTED, shift)
    ran = 0
    for kord in KORDS:
        for iv in IVS:
            if not fast_host_lib.host_fast_arith_serves(iv, kord):
                continue
            ref = oracle_mappm(pe1, q, pe2, iv, kord)
            got = _host(fast_host_lib, pe1, q, pe2, iv, kord)
            bad = exceedances(got, ref)
            assert not bad.any(), (kord, iv, int(bad.sum()), np.nonzero(bad.any(0))[0][:8])
            assert_per_level(got.T, ref.T, 1e-5, f"kord {kord} iv {iv}")
            assert (got != ref).any(), (kord, iv)  # this is the fast policy, not the exact build
            ran += 1
    assert ran == len(KORDS) * len(IVS) - 5


def test_rejected_calls_do_flip_on_the_lattice_pool(fast_host_lib):
    """The pool is adversarial: each pair the predicate rejects shows values beyond 1e-5
    under the emulated rounding (kord 5: 59 columns of 150,000, worst 0.17 of the level's
    scale; kord 7 / iv 0: 4 columns, worst 0.086; of 500,000 columns 264 and 9, worst 0.24
    and 0.16).  Widening the predicate to admit one of
    them fails here, and then in the test above."""
    pe1, q, pe2 = lattice_pool(N_REJECTED)
    rejected = [(k, i) for k in KORDS for i in IVS if not fast_host_lib.host_fast_arith_serves(i, k)]
    assert (5, 1) in rejected and (7, 0) in rejected
    for kord, iv in rejected:
        bad = exceedances(_host(fast_host_lib, pe1, q, pe2, iv, kord), oracle_mappm(pe1, q, pe2, iv, kord))
        assert bad.any(), f"kord {kord} iv {iv}: no flip in the pool; it no longer probes this call"
