"""The default remap arithmetic (``exact=False``; FV3_FAST_ARITH, csrc/mappm_core.h)
against the oracle on every kernel the host can pick, and non-finite inputs.

Bound: 1e-5 of each output level's largest |reference| (tests/parity.py), the project's
contract; a level whose reference is all zero must come back exactly zero.  Wherever
``fast_arith_serves(iv, kord)`` admits the fast kernels the result must differ from the
``exact=True`` result somewhere (a silent reroute to the exact kernels would otherwise
pass as coverage); where it does not (kord 5; kord 7 with iv 0) the default must be the
exact result bit for bit.

Kernels are selected by size, as the product build does: the column counts 4,096 /
24,576 / 131,072 / 180,224 are one on each side of every threshold of ppm_kernel_choice
(csrc/mappm_choice.h; pinned on the CPU by tests/test_mappm_oracle.py) on a 256-CU device,
for one field and for pairs.  Nothing here depends on which kernel the device picks.

Field families: temperature-like 250 + N(0, 10); zero-mean N(0, 10); non-negative with
30 % exact zeros, max(0, N(0.524e-4, 1e-4)) (the mean puts 30 % of the draws below zero).
"""
import functools

import numpy as np
import pytest

from oracle import coarsen as OC
from oracle import restarts as OR
from oracle.mappm import oracle_mappm
from tests.parity import assert_per_level, per_level_errors
from tests.test_remap_fast_host import exceedances, lattice_pool

pytestmark = pytest.mark.gpu

NCOLS = (4096, 24576, 131072, 180224)
KM, KN = 24, 19
FAMILIES = ("temperature", "zero_mean", "non_negative")


def _family(rng, name, shape):
    if name == "temperature":
        return (250 + rng.normal(0, 10, shape)).astype(np.float32)
    if name == "zero_mean":
        return rng.normal(0, 10, shape).astype(np.float32)
    return np.maximum(0, rng.normal(0.524e-4, 1e-4, shape)).astype(np.float32)


def _rough_columns(rng, km, kn, ncol):
    """Rough thicknesses (1 .. 3000) and output edges that overhang both ends."""
    delp = rng.uniform(1, 3000, (km, ncol)).astype(np.float32)
    pe1 = np.concatenate([np.full((1, ncol), 300, np.float32), 300 + np.cumsum(delp, 0, dtype=np.float32)])
    pe2 = np.sort(rng.uniform(pe1[0] * 0.8, pe1[-1] * 1.1, (kn + 1, ncol)), 0).astype(np.float32)
    return pe1, pe2


@functools.lru_cache(maxsize=None)
def _columns(ncol, km=KM, kn=KN):
    """Shared inputs of one size (never written to): host arrays and their device copies."""
    import torch

    rng = np.random.default_rng(1000 + ncol + 7 * kn)
    pe1, pe2 = _rough_columns(rng, km, kn, ncol)
    q = {name: _family(rng, name, (km, ncol)) for name in FAMILIES}
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    return pe1, pe2, q, dev(pe1), dev(pe2), {k: dev(v) for k, v in q.items()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _worst(got, ref):
    rel, _ = per_level_errors(np.asarray(got).T, np.asarray(ref).T)
    return float(np.nanmax(rel)) if np.isfinite(rel).any() else 0.0


def _check_default(got, exact, ref, iv, kord, what):
    """[level, column] results of one call: the 1e-5 contract against the oracle, and
    the arithmetic that ran."""
    from fv3net_amd.mappm import runs_exact

    assert_per_level(got.T, ref.T, 1e-5, what)
    assert not exceedances(got, ref).any(), what
    if runs_exact(iv, kord):
        assert _same_bits(got, exact), f"{what}: rejected by fast_arith_serves but not the exact result"
    else:
        assert not _same_bits(got, exact), f"{what}: identical to exact=True (the fast kernels did not run)"


@pytest.mark.parametrize("iv", [-1, 0, 1, 2])
@pytest.mark.parametrize("kord", [1, 4, 6, 7])
@pytest.mark.parametrize("ncol", NCOLS)
def test_single_field_vs_oracle(gpu, ncol, kord, iv):
    """mappm_device, km 24 -> kn 19, kord x iv x the three field families, on the
    level-parallel / three-lane / two-lane / one-lane kernel (by ncol, see the module
    docstring)."""
    from fv3net_amd.mappm import mappm_device

    pe1, pe2, q, d1, d2, dq = _columns(ncol)
    for name in FAMILIES:
        got = mappm_device(d1, dq[name], d2, iv, kord).cpu().numpy()
        exact = mappm_device(d1, dq[name], d2, iv, kord, exact=True).cpu().numpy()
        ref = oracle_mappm(pe1, q[name], pe2, iv, kord)
        print(f"single ncol {ncol} kord {kord} iv {iv} {name}: worst {_worst(got, ref):.3e}")
        _check_default(got, exact, ref, iv, kord, f"ncol {ncol} kord {kord} iv {iv} {name}")


@pytest.mark.parametrize("kn", [3 * KM, 3])
@pytest.mark.parametrize("ncol", NCOLS[1:3])
def test_single_field_split_points(gpu, ncol, kn):
    """kn = 3 km (many outputs inside one input layer) and kn = 3 (each output spans many
    layers) on the two- and three-lane kernels, whose lanes start at output kn / 2 + 1 and
    kn / 3 + 1, 2 kn / 3 + 1."""
    from fv3net_amd.mappm import mappm_device

    pe1, pe2, q, d1, d2, dq = _columns(ncol, KM, kn)
    for iv, kord in ((1, 1), (0, 4), (-1, 7)):
        for name in FAMILIES:
            got = mappm_device(d1, dq[name], d2, iv, kord).cpu().numpy()
            exact = mappm_device(d1, dq[name], d2, iv, kord, exact=True).cpu().numpy()
            ref = oracle_mappm(pe1, q[name], pe2, iv, kord)
            print(f"split ncol {ncol} kn {kn} kord {kord} iv {iv} {name}: worst {_worst(got, ref):.3e}")
            _check_default(got, exact, ref, iv, kord, f"ncol {ncol} kn {kn} kord {kord} iv {iv} {name}")


@pytest.mark.parametrize("nfields", [2, 3])
@pytest.mark.parametrize("ncol", NCOLS)
def test_pairs_vs_oracle(gpu, ncol, nfields):
    """mappm_device_multi: two fields per pass (an odd last field goes down the
    single-field path), the K1 kernels (iv 1, kord 1) and the general ones.  The fields of
    a pair differ in scale by 1e5, so a register shared or swapped between them shows."""
    import torch

    from fv3net_amd.mappm import mappm_device_multi

    pe1, pe2, q, d1, d2, dq = _columns(ncol)
    small = (1e-5 * _family(np.random.default_rng(ncol), "temperature", q["temperature"].shape)).astype(np.float32)
    fields = [q["temperature"], small, q["zero_mean"]][:nfields]
    dfields = [dq["temperature"], torch.from_numpy(small).cuda(), dq["zero_mean"]][:nfields]
    for iv, kord in ((1, 1), (0, 4), (-1, 7)):
        got = mappm_device_multi(d1, dfields, d2, iv, kord)
        exact = mappm_device_multi(d1, dfields, d2, iv, kord, exact=True)
        for i, f in enumerate(fields):
            ref = oracle_mappm(pe1, f, pe2, iv, kord)
            g = got[i].cpu().numpy()
            print(f"pairs ncol {ncol} nf {nfields} kord {kord} iv {iv} field {i}: worst {_worst(g, ref):.3e}")
            _check_default(g, exact[i].cpu().numpy(), ref, iv, kord,
                           f"ncol {ncol} nfields {nfields} kord {kord} iv {iv} field {i}")


@pytest.mark.parametrize("kord", range(0, 8))
@pytest.mark.parametrize("ncol,shift", [(24576, 0.0), (24576, 0.5), (180224, 0.0)])
def test_lattice_pool_on_device(gpu, ncol, shift, kord):
    """The adversarial pool of tests/test_remap_fast_host.py (regular thicknesses, values
    on a lattice: exact ties in the limiters) through the default path, every iv: no value
    beyond 1e-5 of its level's scale, for the calls the fast kernels serve and for the
    ones routed to the exact kernels.

    Before the routing (every kord <= 7 on the fast kernels) an MI355X measured, at
    180,224 columns: kord 5 (each iv) 204 values in 87 columns beyond 1e-5, worst 0.13 of
    the level's scale; kord 7 / iv 0 4 values in 2 columns, worst 0.045; at 24,576 columns
    24 in 12 (0.13) and 5 in 2 (0.051); every other call none (worst 7.1e-7); the pool
    shifted by -0.5 none in any call.  As the CPU emulation has it."""
    import torch

    from fv3net_amd.mappm import mappm_device

    pe1, q, pe2 = lattice_pool(ncol, shift)
    d1, dq, d2 = (torch.from_numpy(a).cuda() for a in (pe1, q, pe2))
    for iv in (-1, 0, 1, 2):
        got = mappm_device(d1, dq, d2, iv, kord).cpu().numpy()
        exact = mappm_device(d1, dq, d2, iv, kord, exact=True).cpu().numpy()
        ref = oracle_mappm(pe1, q, pe2, iv, kord)
        bad = exceedances(got, ref)
        print(f"lattice ncol {ncol} shift {shift} kord {kord} iv {iv}: {int(bad.sum())} values in "
              f"{int(bad.any(0).sum())} columns beyond 1e-5, worst {_worst(got, ref):.3e}")
        _check_default(got, exact, ref, iv, kord, f"lattice ncol {ncol} shift {shift} kord {kord} iv {iv}")


# ---- the fused coarsen on the default path ----

def _check_coarse(got, exact, ref, iv, kord, what):
    """(tile, z, y, x) coarse fields; a coarse cell whose fine columns are all masked at a
    level is 0 / 0 in the reference: NaN in the same places, the rest held to the bound."""
    from fv3net_amd.mappm import runs_exact

    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), f"{what}: NaN positions differ"
    lev = lambda a: np.moveaxis(np.where(nan, 0, a), 1, -1).reshape(-1, a.shape[1])  # noqa: E731
    assert_per_level(lev(got), lev(ref), 1e-5, what)
    same = bool(((_bits(got) == _bits(exact)) | (np.isnan(got) & np.isnan(exact))).all())
    if runs_exact(iv, kord):
        assert same, f"{what}: rejected by fast_arith_serves but not the exact result"
    else:
        assert not same, f"{what}: identical to exact=True (the fast kernels did not run)"
    rel, _ = per_level_errors(lev(got), lev(ref))
    return float(np.nanmax(rel)) if np.isfinite(rel).any() else 0.0


COARSEN_CASES = ((1, 1), (0, 4), (1, 6), (-1, 7), (0, 5))


@functools.lru_cache(maxsize=None)
def _coarsen_state(n, km=33):
    rng = np.random.default_rng(50 + n)
    base = np.linspace(200, 1800, km)[None, :, None, None]
    delp = base * rng.uniform(0.9, 1.1, (6, km, n, n))
    delp[:, -4:] *= rng.uniform(0.3, 2.0, (6, 1, n, n))  # the mask drops fine columns near the surface
    area = rng.uniform(0.5, 1.0, (6, n, n)).astype(np.float32)
    fields = {name: _family(rng, name, (6, km, n, n)) for name in ("zero_mean", "temperature", "non_negative")}
    return delp, area, fields


def _run_coarsen(delp, area, fields, factor, iv, kord, what):
    from fv3net_amd.coarsen import coarsen_on_pressure

    got, dc = coarsen_on_pressure(delp, area, fields, factor, iv=iv, kord=kord)
    exact, _ = coarsen_on_pressure(delp, area, fields, factor, iv=iv, kord=kord, exact=True)
    ref, ref_dc = OC.coarsen_on_pressure(delp, area, list(fields.values()), factor, iv=iv, kord=kord)
    assert _same_bits(dc.cpu().numpy(), ref_dc), f"{what}: coarse delp"  # pass 1 keeps the reference's arithmetic
    for name, r in zip(fields, ref):
        w = _check_coarse(got[name].cpu().numpy(), exact[name].cpu().numpy(), r, iv, kord, f"{what} {name}")
        print(f"coarsen {what} {name}: worst {w:.3e}")


@pytest.mark.parametrize("iv,kord", COARSEN_CASES)
@pytest.mark.parametrize("nfields", [1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("factor,n", [(8, 48), (4, 24)])
def test_coarsen_vs_oracle(gpu, factor, n, dtype, nfields, iv, kord):
    """coarsen_on_pressure, factor 8 and 4, both delp dtypes, 1 and 3 fields (zero-mean;
    plus temperature-like and non-negative with exact zeros), 33 levels with the mask
    active near the surface.  The coarse delp stays bit-identical to the oracle."""
    delp, area, fields = _coarsen_state(n)
    fields = dict(list(fields.items())[:nfields])
    _run_coarsen(delp.astype(dtype), area, fields, factor, iv, kord, f"f{factor} {np.dtype(dtype).name} iv {iv} kord {kord}")


@pytest.mark.parametrize("iv,kord", COARSEN_CASES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_coarsen_steep_cells_vs_oracle(gpu, dtype, iv, kord):
    """The state of test_coarsen.py::test_kernel_steep_cells_overflow_columns (79 levels,
    the lowest 40 scaled by 0.05 .. 4 per column: the per-wave ring of 12 / 16 levels
    overflows into the per-lane global columns) on the default path, factor 8 and 4."""
    from tests.test_coarsen import _smooth_state

    rng = np.random.default_rng(11)
    delp, area, T, q = _smooth_state(rng, 6, 79, 16, 16)
    delp[:, -40:] *= rng.uniform(0.05, 4.0, (6, 1, 16, 16)).astype(np.float32)
    for f in (8, 4):
        _run_coarsen(delp.astype(dtype), area, {"T": T, "q": q}, f, iv, kord,
                     f"steep f{f} {np.dtype(dtype).name} iv {iv} kord {kord}")


@pytest.mark.parametrize("iv,kord", COARSEN_CASES)
def test_coarsen_masked_levels_vs_oracle(gpu, iv, kord):
    """The state of test_coarsen.py::test_kernel_masked_levels_and_kord (strongly varying
    surface pressure: the mask drops fine columns at the lowest coarse levels)."""
    from tests.test_coarsen import _smooth_state

    rng = np.random.default_rng(7)
    delp, area, T, q = _smooth_state(rng, 2, 40, 16, 16)
    delp[:, -5:] *= rng.uniform(0.2, 3.0, (2, 1, 16, 16)).astype(np.float32)
    _run_coarsen(delp, area, {"q": q}, 4, iv, kord, f"masked iv {iv} kord {kord}")


@pytest.mark.parametrize("iv,kord", [(1, 1), (0, 4), (-1, 7)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("edge", ["x", "y"])
def test_coarsen_edges_vs_oracle(gpu, edge, dtype, iv, kord):
    """coarsen_edges_on_pressure, factor 4 of n = 16, a zero-mean wind on both edges."""
    from fv3net_amd.coarsen import coarsen_edges_on_pressure

    rng = np.random.default_rng(60 + (edge == "y"))
    n, km, f = 16, 33, 4
    base = np.linspace(200, 1800, km)[None, :, None, None]
    delp = (base * rng.uniform(0.9, 1.1, (6, km, n, n))).astype(dtype)
    es = (6, n + 1, n) if edge == "x" else (6, n, n + 1)
    spacing = rng.uniform(0.5, 1.0, es).astype(np.float32)
    u = rng.normal(0, 10, (6, km) + es[1:]).astype(np.float32)
    got = coarsen_edges_on_pressure(delp, spacing, {"u": u}, f, edge, iv=iv, kord=kord)["u"].cpu().numpy()
    exact = coarsen_edges_on_pressure(delp, spacing, {"u": u}, f, edge, iv=iv, kord=kord, exact=True)["u"].cpu().numpy()
    ref = OC.coarsen_edges_on_pressure(delp, spacing, [u], f, edge, iv=iv, kord=kord)[0]
    w = _check_coarse(got, exact, ref, iv, kord, f"edge {edge} {np.dtype(dtype).name} iv {iv} kord {kord}")
    print(f"edges {edge} {np.dtype(dtype).name} iv {iv} kord {kord}: worst {w:.3e}")


# ---- non-finite inputs ----

def _with_nans(q):
    """A NaN layer at the top, at an interior level and at the bottom of a few columns,
    and one all-NaN column."""
    q = q.copy()
    km, ncol = q.shape
    q[0, 1] = q[km // 2, 2] = q[km - 1, 3] = np.nan
    q[0, ncol - 2] = q[km - 1, ncol - 2] = np.nan
    q[:, ncol // 2] = np.nan
    return q


def _same_bits_or_nan(got, ref, what, expect_nan=True):
    got, ref = np.asarray(got), np.asarray(ref)
    assert (np.isnan(got) == np.isnan(ref)).all(), f"{what}: NaN positions differ"
    ok = (_bits(got) == _bits(ref)) | np.isnan(ref)
    assert ok.all(), f"{what}: {int((~ok).sum())} finite values differ"
    assert np.isnan(ref).any() == expect_nan and np.isfinite(ref).any(), what


@pytest.mark.parametrize("ncol", NCOLS)
def test_exact_path_nan_inputs(gpu, ncol):
    """exact=True propagates a NaN by position as the reference does: mappm_device and
    mappm_device_multi give NaN exactly where oracle_mappm does and its bits elsewhere,
    on each of the four kernels."""
    import torch

    from fv3net_amd.mappm import mappm_device, mappm_device_multi

    pe1, pe2, q, d1, d2, dq = _columns(ncol)
    qa, qb = _with_nans(q["temperature"]), _with_nans(q["zero_mean"][:, ::-1])
    da, db = torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda()
    for iv, kord in ((1, 1), (0, 4), (-1, 7)):
        ra, rb = oracle_mappm(pe1, qa, pe2, iv, kord), oracle_mappm(pe1, qb, pe2, iv, kord)
        _same_bits_or_nan(mappm_device(d1, da, d2, iv, kord, exact=True).cpu().numpy(), ra, f"single {ncol} {iv} {kord}")
        for nf in (2, 3):
            outs = mappm_device_multi(d1, [da, db, da][:nf], d2, iv, kord, exact=True)
            for o, r in zip(outs, (ra, rb, ra)):
                _same_bits_or_nan(o.cpu().numpy(), r, f"multi {nf} fields {ncol} {iv} {kord}")


@pytest.mark.parametrize("factor,n", [(8, 48), (4, 24)])
def test_exact_coarsen_nan_inputs(gpu, factor, n):
    """coarsen_on_pressure(exact=True) with NaN layers in a field.  The reference's block
    sums skip NaN (xarray's coarsen().sum()), so a remapped NaN leaves its coarse value
    finite, made of the other fine columns: the remap has to put every NaN where the
    reference's does for the coarse values to carry oracle/coarsen.py's bits."""
    from fv3net_amd.coarsen import coarsen_on_pressure

    delp, area, fields = _coarsen_state(n)
    T = fields["temperature"].copy()
    km = T.shape[1]
    T[0, 0, 1, 1] = T[1, km // 2, 2, 5] = T[2, km - 1, 3, 3] = np.nan
    T[3, :, n - 1, n - 2] = np.nan
    for iv, kord in ((1, 1), (0, 4)):
        got, _ = coarsen_on_pressure(delp.astype(np.float32), area, {"T": T}, factor, iv=iv, kord=kord, exact=True)
        (ref,), _ = OC.coarsen_on_pressure(delp.astype(np.float32), area, [T], factor, iv=iv, kord=kord)
        (clean,), _ = OC.coarsen_on_pressure(delp.astype(np.float32), area, [fields["temperature"]], factor, iv=iv,
                                             kord=kord)
        assert int((ref != clean).sum()) >= 4  # the NaNs reach the coarse values
        _same_bits_or_nan(got["T"].cpu().numpy(), ref, f"coarsen f{factor} iv {iv} kord {kord}", expect_nan=False)


def test_regrid_vertical_default_nan_inputs(gpu):
    """regrid_vertical mirrors a reference function on data from files: on its default
    path a NaN-bearing input gives NaN exactly where the oracle does and stays within 1e-5
    per level elsewhere (it tests its inputs for finiteness and runs the reference's
    arithmetic when the test fails); finite inputs still run the fast kernels."""
    from fv3net_amd.coarsen import regrid_vertical

    pe1, pe2, q, *_ = _columns(NCOLS[0])
    pe1, pe2 = pe1.copy(), pe2.copy()
    for iv, kord in ((1, 1), (0, 4), (-1, 7)):
        qn = _with_nans(q["temperature"])
        ref = oracle_mappm(pe1, qn, pe2, iv, kord)
        got = regrid_vertical(pe1, qn, pe2, iv=iv, kord=kord, z_axis=0).cpu().numpy()
        nan = np.isnan(ref)
        assert nan.any() and (np.isnan(got) == nan).all(), (iv, kord)
        assert_per_level(np.where(nan, 0, got).T, np.where(nan, 0, ref).T, 1e-5, f"NaN input iv {iv} kord {kord}")
        fin = regrid_vertical(pe1, q["temperature"], pe2, iv=iv, kord=kord, z_axis=0).cpu().numpy()
        exact = regrid_vertical(pe1, q["temperature"], pe2, iv=iv, kord=kord, z_axis=0, exact=True).cpu().numpy()
        assert not _same_bits(fin, exact), (iv, kord)
    inf = q["temperature"].copy()
    inf[5, 7] = np.inf
    got = regrid_vertical(pe1, inf, pe2, z_axis=0).cpu().numpy()
    ref = oracle_mappm(pe1, inf, pe2, 1, 1)
    assert ((_bits(got) == _bits(ref)) | (np.isnan(got) & np.isnan(ref))).all()


def test_restarts_default_nan_inputs(gpu):
    """coarsen_restarts_on_pressure on its default path with NaNs in a core field, a
    tracer and a wind: every variable has NaN exactly where oracle/restarts.py does (its
    block sums skip a remapped NaN, so the coarse values stay finite but are made of the
    other fine columns) and is within 1e-5 per level elsewhere; the same inputs without the
    NaNs still run the fast kernels."""
    from fv3net_amd.restarts import coarsen_restarts_on_pressure
    from tests.test_restarts import LOG_VARS, _random_restarts, _to_np

    grid, restarts, _ = _random_restarts(np.random.default_rng(33), 16, 20, True)
    clean = _to_np(coarsen_restarts_on_pressure(4, grid, restarts, coarsen_agrid_winds=True))
    clean_exact = _to_np(coarsen_restarts_on_pressure(4, grid, restarts, coarsen_agrid_winds=True, exact=True))
    assert not _same_bits(clean["fv_core.res"]["T"], clean_exact["fv_core.res"]["T"])
    core, tracer = restarts["fv_core.res"], restarts["fv_tracer.res"]
    core["T"][0, 0, 0, 1, 1] = core["T"][1, 0, 10, 5, 6] = core["T"][2, 0, 19, 9, 9] = np.nan
    core["T"][3, 0, :, 14, 2] = np.nan
    tracer["sphum"][4, 0, 7, 3, 3] = np.nan
    core["u"][5, 0, 3, 16, 4] = np.nan
    got = _to_np(coarsen_restarts_on_pressure(4, grid, restarts, coarsen_agrid_winds=True))
    ref = OR.coarsen_restarts_on_pressure(4, grid, restarts, True)
    moved = 0
    for cat, names in ref.items():
        for name, r in names.items():
            g = got[cat][name]
            assert g.shape == r.shape and g.dtype == r.dtype, (cat, name)
            nan = np.isnan(r)
            assert (np.isnan(g) == nan).all(), f"{cat}/{name}: NaN positions differ"
            if (cat, name) in LOG_VARS:
                np.testing.assert_allclose(g, r, rtol=1e-12, atol=0, err_msg=f"{cat}/{name}")
            elif r.ndim == 5:  # (tile, Time, z, y, x)
                lev = lambda a: np.moveaxis(np.where(nan, 0, a), 2, -1).reshape(-1, a.shape[2])  # noqa: E731
                assert_per_level(lev(g), lev(r), 1e-5, f"{cat}/{name}")
            moved += int((g != clean[cat][name]).sum())
    assert moved > 0  # the NaNs reach the coarse values
