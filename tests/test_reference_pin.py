"""The CPU oracle against the REFERENCE's own compiled Fortran (oracle/_ref/libfv3ref.so through tests/ref_lib.py): live, on
seeded inputs, and against the recorded reference outputs of tests/golden/refpin_*.npz.

Pure stencil arithmetic is asserted bit for bit (np.array_equal).  The Riemann solvers go through libm's exp / log in the
reference and through include/fv3_math.h in the oracle; there the bound is, field by field, 10 x the measured worst relative
RMS difference (refpin_common.MEASURED, which also says why RMS and gives the max-norm figures; floor 1e-15, ceiling the
project's 1e-12).

Where the reference tree and amdflang are both present a library that does not build FAILS the live tests; where neither
the tree nor a built library is there they skip.  The golden tests always run.

Not cases, with the reason:
  * fv_tp_2d / deln_flux with nord = 3: the reference overruns its own arrays (tp_core.F90:1273 says so).
  * map1_q2 with iv = -2: the reference passes an uninitialised local qs to scalar_profile (fv_operators.F90:380, :396).
  * a2b_ord4 on a tile that owns a cube corner, d_sw with nord > 0 and dddmp there, d_sw with nord > 1 there: they need
    great_circle_dist / fill_corners, which the stand-ins stop at.  Unpinned.
"""
from __future__ import annotations

import glob
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import parity_common as P
import ref_lib as R
import refpin_common as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRIDS = ["dp", "dp_perturbed"] + list(RC.TILES) + ["face"]


@pytest.fixture(scope="module")
def ref():
    if R.can_build():
        assert R.available()          # builds; a failure here is a failure of the test
    elif not os.path.isfile(R.SO):
        pytest.skip("no reference tree and no oracle/_ref/libfv3ref.so")
    R.lib()
    return R


def grid_and_state(name, npz, hydrostatic=False):
    if name.startswith("dp"):
        g = RC.periodic_grid(13, 9, name == "dp_perturbed")
        return g, RC.smooth_state(g.bd, npz, hydrostatic=hydrostatic)
    return RC.tile_state(name, npz, hydrostatic=hydrostatic, npx=13 if name == "face" else 25)


def report(routine, what, figures):
    """each figure before it is asserted: field rel_rms / rel_max (asserted bound on rel_rms)"""
    print(f"refpin {routine} {what}: " + ", ".join(f"{n} {r:.2e} / {m:.2e} ({RC.bound(routine, n):.1e})" for n, (r, m) in figures.items()))


# ---- fv_tp_2d ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("hord", RC.ALL_HORD)
def test_fv_tp_2d_every_hord_and_mode(ref, grid, hord):
    """plain, mass-flux and mass-flux + damping (nord 0, 1, 2); tiles with a face edge run the xppm / yppm edge branches
    below hord 8, tiles with a corner run copy_corners"""
    g, st = grid_and_state(grid, 2)
    inp = RC.tp_inputs(g, q=None if grid.startswith("dp") else st["delp"][:, :, 0])
    for mode in RC.TP_MODES:
        RC.compare("fv_tp_2d", RC.run_fv_tp_2d(O, g, inp, hord, mode), RC.run_fv_tp_2d(ref, g, inp, hord, mode), what=f"{grid} {mode}")


@pytest.mark.parametrize("grid", ["dp_perturbed", "west", "corner_sw", "face"])
@pytest.mark.parametrize("lim_fac", [0.85, 1.3])
def test_fv_tp_2d_lim_fac(ref, grid, lim_fac):
    g, st = grid_and_state(grid, 2)
    g.lim_fac = lim_fac
    inp = RC.tp_inputs(g, q=None if grid.startswith("dp") else st["pt"][:, :, 1], seed=6)
    different = False
    for hord in RC.ALL_HORD:
        a = RC.run_fv_tp_2d(O, g, inp, hord, "mass_flux")
        RC.compare("fv_tp_2d", a, RC.run_fv_tp_2d(ref, g, inp, hord, "mass_flux"), what=f"{grid} hord {hord}")
        if abs(hord) == 1:
            g.lim_fac = 1.0
            different |= not np.array_equal(RC.run_fv_tp_2d(O, g, inp, hord, "mass_flux")["fx"], a["fx"])
            g.lim_fac = lim_fac
    assert different, "lim_fac does not reach the scheme it belongs to"


@pytest.mark.parametrize("grid", ["corner_sw", "corner_ne", "face", "west"])
@pytest.mark.parametrize("dir_", [1, 2])
def test_copy_corners(ref, grid, dir_):
    g, st = grid_and_state(grid, 2)
    q = st["delp"][:, :, 1].copy(order="F")
    a = RC.run_copy_corners(O, g, q, dir_)
    RC.compare("copy_corners", a, RC.run_copy_corners(ref, g, q, dir_), what=grid)
    assert np.array_equal(a["q"], q) == (grid == "west")     # a corner tile's halo corners really are rewritten


# ---- c_sw, a2b_ord4 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("hydrostatic", [False, True])
def test_c_sw(ref, grid, hydrostatic):
    g, st = grid_and_state(grid, 3, hydrostatic)
    a, _ = RC.run_c_sw(O, g, st, 3, 3.0, hydrostatic)
    b, _ = RC.run_c_sw(ref, g, st, 3, 3.0, hydrostatic)
    RC.compare("c_sw", a, b, what=grid)


@pytest.mark.parametrize("grid", ["dp", "dp_perturbed", "interior", "west", "east", "south", "north"])
@pytest.mark.parametrize("replace", [False, True])
def test_a2b_ord4(ref, grid, replace):
    """every tile without a cube corner (the corner's extrap_corner needs great_circle_dist: unpinned)"""
    g, st = grid_and_state(grid, 3)
    for k, n in ((0, "delp"), (1, "pt"), (2, "w")):
        q = st[n][:, :, k].copy(order="F")
        RC.compare("a2b_ord4", RC.run_a2b_ord4(O, g, q, replace), RC.run_a2b_ord4(ref, g, q, replace), what=f"{grid} {n}")


# ---- d_sw ----------------------------------------------------------------------------------------------------------------
CORNER_GRIDS = ("corner_sw", "corner_ne", "face")


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", list(RC.DSW_CASES))
@pytest.mark.parametrize("hydrostatic", [False, True])
def test_d_sw(ref, grid, hydrostatic, case):
    """every branch check_d_sw is parametrised with, on every grid.  Tiles that own a cube corner run each case with nord = 0 on
    every level (nord > 0 there needs fill_corners / great_circle_dist: unpinned, module docstring): the hord families, lim_fac,
    use_cond, d_con, do_diss_est and inline_q all reach the corner and edge code of the cubed-sphere lines that way"""
    g, st = grid_and_state(grid, 4, hydrostatic)
    assert R._has_corner(g) == (grid in CORNER_GRIDS)
    g, par, lev, f = RC.dsw_inputs(g, st, 4, hydrostatic, case, nord0=grid in CORNER_GRIDS)
    a = RC.run_d_sw(O, g, par, lev, f, 4)
    RC.compare("d_sw", a, RC.run_d_sw(ref, g, par, lev, f, 4), what=f"{grid} {case}")
    assert np.any(a["u"]) and np.any(a["delp"])


def test_d_sw_cases_reach_their_branches(ref):
    """the damping / heating cases really differ from the defaults (a case that silently ran the default branch would pin nothing)"""
    g, st = grid_and_state("dp_perturbed", 4)
    out = {}
    for case in ("defaults", "nord0", "nord2_vort_dcon", "nord3_diss_est", "hord5", "hord_lin", "lim_fac"):
        g2, par, lev, f = RC.dsw_inputs(RC.periodic_grid(13, 9, True), st, 4, False, case)
        out[case] = RC.run_d_sw(O, g2, par, lev, f, 4)
    for case in out:
        if case != "defaults":
            assert any(not np.array_equal(out[case][n], out["defaults"][n]) for n in out[case]), case
    assert np.any(out["nord3_diss_est"]["diss_est"]) and np.any(out["nord2_vort_dcon"]["heat_source"][:, :, 2:])


# ---- update_dz_c / update_dz_d ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("km", [3, 8, 79])
def test_update_dz_c(ref, perturb, km):
    g = RC.periodic_grid(13, 9, perturb)
    s = RC.nh_inputs(g, km)
    _, f = RC.run_c_sw(O, g, RC.smooth_state(g.bd, km), km, 3.0, False)
    RC.compare("update_dz_c", RC.run_update_dz_c(O, g, s, km, f["ut"], f["vt"]), RC.run_update_dz_c(ref, g, s, km, f["ut"], f["vt"]))


@pytest.mark.parametrize("grid", ["interior", "west", "north", "corner_sw", "face"])
def test_update_dz_c_on_the_cube(ref, grid):
    """the edge and corner branches of update_dz_c (nh_utils.F90:59-200): the fluxes of c_sw on a face tile, a smooth height field"""
    km = 4
    g, st = grid_and_state(grid, km)
    _, f = RC.run_c_sw(O, g, st, km, 3.0, False)
    bd = g.bd
    s = dict(dp0=np.linspace(400.0, 3000.0, km), zs=np.asfortranarray(0.05 * st["delp"][:, :, 0]), zh=bd.zeros("A", km + 1))
    s["zh"][:, :, km] = s["zs"]
    for k in range(km - 1, -1, -1):
        s["zh"][:, :, k] = s["zh"][:, :, k + 1] + 0.3 * st["delp"][:, :, k]
    RC.compare("update_dz_c", RC.run_update_dz_c(O, g, s, km, f["ut"], f["vt"]), RC.run_update_dz_c(ref, g, s, km, f["ut"], f["vt"]), what=grid)


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("km,hord,lev_over", [(3, 10, None), (8, 5, None), (8, 6, None), (8, 8, None), (8, -5, None), (8, 1, None),
                                              (8, 10, dict(nord=2, do_vort_damp=True, vtdm4=0.06)),
                                              (79, 10, dict(nord=3, do_vort_damp=True, vtdm4=0.03))])
def test_update_dz_d(ref, perturb, km, hord, lev_over):
    g = RC.periodic_grid(13, 9, perturb)
    s = RC.nh_inputs(g, km)
    arr, _ = RC.dz_d_inputs(g, km, lev_over=lev_over)
    RC.compare("update_dz_d", RC.run_update_dz_d(O, g, s, km, arr, hord), RC.run_update_dz_d(ref, g, s, km, arr, hord))


# ---- the Riemann solvers -------------------------------------------------------------------------------------------------
MOIST = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("km", [3, 8, 79, 127])
@pytest.mark.parametrize("use_cond,moist_kappa", MOIST)
def test_riem_solver_c(ref, km, use_cond, moist_kappa, capsys):
    """the default SIM1 path (a_imp = 1); measured worst relative RMS over these cases: refpin_common.MEASURED"""
    g = RC.periodic_grid(13, 9, False)
    s = RC.nh_inputs(g, km)
    kw = dict(use_cond=use_cond, moist_kappa=moist_kappa)
    fig = {}
    RC.compare("riem_solver_c", RC.run_riem_solver_c(O, g, s, km, **kw), RC.run_riem_solver_c(ref, g, s, km, **kw), figures=fig)
    with capsys.disabled():
        report("riem_solver_c", f"km={km} {kw}", fig)


@pytest.mark.parametrize("km", [3, 8, 79, 127])
@pytest.mark.parametrize("use_cond,moist_kappa", MOIST)
@pytest.mark.parametrize("use_logp", [False, True])
@pytest.mark.parametrize("last_call", [False, True])
def test_riem_solver3(ref, km, use_cond, moist_kappa, use_logp, last_call, capsys):
    g = RC.periodic_grid(13, 9, False)
    s = RC.nh_inputs(g, km)
    kw = dict(use_cond=use_cond, moist_kappa=moist_kappa, use_logp=use_logp, last_call=last_call)
    fig = {}
    RC.compare("riem_solver3", RC.run_riem_solver3(O, g, s, km, **kw), RC.run_riem_solver3(ref, g, s, km, **kw), figures=fig)
    with capsys.disabled():
        report("riem_solver3", f"km={km} {kw}", fig)


# ---- the remap operators and fillz -----------------------------------------------------------------------------------------
def _ivs(which):
    # map1_q2 with iv = -2 reads an uninitialised qs in the reference; mapn_tracer is iv = 0 by construction
    return {0: (-2, -1, 0, 1), 1: (-2, -1, 0, 1), 2: (-1, 0, 1), 3: (0,)}[which]


@pytest.mark.parametrize("which", list(RC.REMAP_OPS))
@pytest.mark.parametrize("kord", RC.KORDS)
def test_remap_operators(ref, which, kord):
    """map_scalar, map1_ppm, map1_q2, mapn_tracer through oracle_lib.remap_column: every kord the project accepts, both signs of
    it where a map routine tests the signed kord, every iv"""
    for km in (12, 33, 79):
        for seed in (1, 2):
            pe1, pe2, q = RC.remap_columns(km, seed)
            for iv in _ivs(which):
                for kk in (kord, -kord):
                    qq = q - 280.0 if iv == 0 else q
                    qmin = 184.0 if iv == 1 else 0.0
                    a = O.remap_column(which, pe1, pe2, qq, 1.5, iv, kk, qmin)
                    b = ref.remap_column(which, pe1, pe2, qq, 1.5, iv, kk, qmin)
                    assert np.array_equal(a, b), f"{RC.REMAP_OPS[which]} km={km} iv={iv} kord={kk}: rel max {RC.rel_max(a, b):.3e}"


@pytest.mark.parametrize("im,km,nq", [(5, 12, 3), (7, 79, 2), (4, 5, 1)])
def test_fillz(ref, im, km, nq):
    q, dp = RC.fillz_inputs(im, km, nq)
    a, b = q.copy(order="F"), q.copy(order="F")
    R.oracle_fillz(a, dp)
    ref.fillz(b, dp)
    assert np.array_equal(a, b)
    assert np.sum(b < 0) < np.sum(q < 0) and not np.array_equal(b, q)


# ---- goldens ---------------------------------------------------------------------------------------------------------------
sys.path.insert(0, GOLDEN)
import make_refpin_golden as G  # noqa: E402

GOLDEN_FILES = tuple("grid_" + n for n in G.GRID_NAMES) + G.ROUTINES


def test_goldens_are_there_and_small():
    names = {os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "refpin_*.npz"))}
    assert names == {f"refpin_{r}.npz" for r in GOLDEN_FILES}, names
    for r in GOLDEN_FILES:
        f = os.path.join(GOLDEN, f"refpin_{r}.npz")
        assert os.path.getsize(f) <= 213341, f      # no larger than the largest golden before them (ppm1d_golden.npz)


@pytest.mark.parametrize("routine", G.ROUTINES)
def test_oracle_reproduces_the_golden(routine):
    """always runs: the recorded inputs through the oracle against the recorded reference outputs, same bounds as live"""
    n = 0
    for name, key, got, want in G.replay(routine, G.oracle_runner()):
        RC.compare(key, got, want, what=name)
        n += 1
    assert n > 0


@pytest.mark.parametrize("routine", GOLDEN_FILES)
def test_reference_rebuilds_the_golden(ref, routine):
    """with the reference library at hand the generator reproduces the committed file bit for bit"""
    have = np.load(os.path.join(GOLDEN, f"refpin_{routine}.npz"))
    made = G.make(routine)
    assert sorted(have.files) == sorted(made)
    for k in have.files:
        assert have[k].dtype == made[k].dtype and np.array_equal(have[k], made[k]), k
