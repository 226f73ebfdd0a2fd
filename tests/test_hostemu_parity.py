"""Kernel-logic tests on the CPU: the HIP tile kernels compiled by g++ in host-emulation mode
(tests/hostemu; one thread per workgroup) against the oracle.  This is a development harness for
the GPU-less build container; the real parity gate is tests/test_gpu_parity.py (-m gpu)."""
import os
import subprocess

import numpy as np
import pytest

import parity_common as P
from gfdl_atmos_cubed_sphere_amd.lib import Fv3Lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "hostemu"), "-s"])
    return Fv3Lib(os.path.join(HERE, "hostemu", "libfv3_hostemu.so"))


@pytest.mark.parametrize("hord", [5, -5, 6, 7, 8, 10, 9, 11, 12, 13])
def test_fv_tp_2d_plain(emu, hord):
    P.check_fv_tp_2d(emu, hord)


@pytest.mark.parametrize("mode,nord,damp_c", [("mass_flux", -1, 0.0), ("mass_flux_damp", 1, 0.06),
                                             ("mass_flux_damp", 2, 0.06), ("plain", 0, 0.05), ("plain", 2, 0.06)])
def test_fv_tp_2d_modes(emu, mode, nord, damp_c):
    P.check_fv_tp_2d(emu, 10, mode=mode, nord=nord, damp_c=damp_c)


def test_fv_tp_2d_tile_multiple_and_ragged(emu):
    P.check_fv_tp_2d(emu, 10, nx=64, ny=16)   # exact multiples of the tile
    P.check_fv_tp_2d(emu, 8, nx=33, ny=9)     # one extra column/row
    P.check_fv_tp_2d(emu, 10, nx=7, ny=5)     # smaller than a tile


@pytest.mark.parametrize("hydrostatic", [False, True])
@pytest.mark.parametrize("perturb", [False, True, "ortho"])
def test_c_sw(emu, hydrostatic, perturb):
    P.check_c_sw(emu, hydrostatic=hydrostatic, perturb=perturb)


def test_c_sw_ragged(emu):
    P.check_c_sw(emu, nx=28, ny=4, npz=2)
    P.check_c_sw(emu, nx=64, ny=16, npz=1)
    P.check_c_sw(emu, nx=61, ny=13, npz=1)


@pytest.mark.parametrize("hydrostatic", [False, True])
def test_d_sw_defaults(emu, hydrostatic):
    P.check_d_sw(emu, hydrostatic=hydrostatic)


def test_d_sw_cartesian_metrics(emu):
    P.check_d_sw(emu, perturb=False)


def test_d_sw_damping_heating(emu):
    # do_vort_damp + d_con + Smagorinsky-type divergence damping + higher-order nord
    P.check_d_sw(emu, par_over=dict(dddmp=0.2, kgb=1e-3),
                 lev_over=dict(nord=2, do_vort_damp=True, vtdm4=0.06, d_con=1.0, d2_bg=0.0075))


def test_d_sw_nord3_and_no_cooling_limiter(emu):
    P.check_d_sw(emu, lev_over=dict(nord=3, do_vort_damp=True, vtdm4=0.03, d_con=0.5),
                 flags=dict(prevent_diss_cooling=False, do_diss_est=True))


def test_d_sw_dcon_without_vort_damp(emu):
    P.check_d_sw(emu, lev_over=dict(nord=1, d_con=1.0))


def test_d_sw_use_cond_low_order(emu):
    P.check_d_sw(emu, use_cond=True, par_over=dict(hord_mt=6, hord_vt=6, hord_tm=5, hord_dp=-5))


def test_d_sw_ragged(emu):
    P.check_d_sw(emu, nx=33, ny=9, npz=2)
    P.check_d_sw(emu, nx=64, ny=16, npz=2)


def test_halo_fill_periodic(emu):
    P.check_halo_periodic(emu)


# ---- nonhydrostatic column path ------------------------------------------------------------------
import parity_nh as N


def test_nh_update_dz_c(emu):
    N.check_update_dz_c(emu)


@pytest.mark.parametrize("a_imp", [1.0, 0.75])
def test_nh_riem_solver_c(emu, a_imp):
    N.check_riem_solver_c(emu, a_imp=a_imp)


@pytest.mark.parametrize("a_imp,use_logp,last_call,fp_out", [(1.0, False, True, False), (0.75, False, True, False),
                                                            (1.0, True, False, True), (0.75, True, True, True)])
def test_nh_riem_solver3(emu, a_imp, use_logp, last_call, fp_out):
    N.check_riem_solver3(emu, a_imp=a_imp, use_logp=use_logp, last_call=last_call, fp_out=fp_out)


def test_nh_update_dz_d(emu):
    N.check_update_dz_d(emu)
    N.check_update_dz_d(emu, lev_over=dict(nord=2, do_vort_damp=True, vtdm4=0.06), hord=8)
    N.check_update_dz_d(emu, nx=33, ny=9, km=3)


@pytest.mark.parametrize("hydrostatic", [False, True])
def test_nh_p_grad_c(emu, hydrostatic):
    N.check_p_grad_c(emu, hydrostatic=hydrostatic)


def test_nh_p_grad(emu):
    N.check_nh_p_grad(emu)
    N.check_nh_p_grad(emu, nx=33, ny=9, km=3)


def test_one_grad_p_in_the_nonhydrostatic_loop(emu, tmp_path):
    """beta < -0.1 (dyn_core.F90:939, :1029-1030, :1909-2030 with hydrostatic = .false.): Riem_Solver3 leaves the full pressure, one_grad_p
    with a2b_ord4 of delp as the layer weights takes the place of nh_p_grad -- the kernel, then the substep loops, doubly periodic
    (with and without the external-mode damping) and on the sphere"""
    N.check_one_grad_p_nh(emu)
    N.check_one_grad_p_nh(emu, nx=33, ny=9, km=3, d_ext=0.0)
    D.check_substeps(emu, n_split=3, flags=dict(beta=-1.0))
    D.check_substeps(emu, n_split=2, flags=dict(beta=-1.0, d_ext=0.0, a_imp=0.75))
    cs, gs = PC.CC.sphere(13)
    for t in (1, 5):
        N.check_one_grad_p_nh(emu, km=4, grid=gs[t], d_ext=0.0)
    assert max(PC.check_substeps_nh(emu, npx=13, npz=5, n_split=3, flags=dict(beta=-1.0)).values()) <= 1e-13
    # ... and through the Fortran host (fv3_host_mod's loop), bit-identical to the Python host
    import fortran_host as F
    assert "fv3_solo: done" in F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=8, nq=1, beta=-1.0)
    assert "fv3_solo_sphere: done" in F.check_fortran_sphere(emu, tmp_path, npx=13, npz=8, nq=1, n_split=2, k_split=1, beta=-1.0)


def test_split_p_grad_and_grad1_p_update(emu):
    """beta > 0 (dyn_core.F90:1795-1900, :2033-2116): kernels over three calls, then both substep loops, doubly periodic and sphere"""
    N.check_split_p_grad(emu)
    N.check_split_p_grad(emu, nx=33, ny=9, km=3, beta=0.25)
    N.check_grad1_p_update(emu)
    N.check_grad1_p_update(emu, nx=33, ny=9, km=3, d_ext=0.0)
    D.check_substeps(emu, n_split=3, flags=dict(beta=0.4, a_imp=0.6))
    D.check_substeps_hydrostatic(emu, n_split=3, flags=dict(beta=0.4))
    assert D.check_fv_step(emu, flags=dict(beta=0.3)) is not None
    cs, gs = PC.CC.sphere(13)
    for t in (0, 4):
        N.check_split_p_grad(emu, km=4, grid=gs[t])
        N.check_grad1_p_update(emu, km=4, grid=gs[t], d_ext=0.0)
    assert max(PC.check_substeps_nh(emu, npx=13, npz=5, n_split=3, flags=dict(beta=0.4)).values()) <= 1e-13
    assert max(PC.check_substeps_hydrostatic(emu, npx=13, npz=4, n_split=3, flags=dict(beta=0.4)).values()) <= 1e-13
    r = PC.check_jw_step(emu, npx=13, npz=20, k_split=2, n_split=2, bdt=900.0, hydrostatic=False, flags=dict(beta=0.4))
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


def test_inline_q(emu):
    """inline_q (sw_core.F90:1020-1043): the tracers inside d_sw every substep, nonhydrostatic and hydrostatic, with and without the
    del-n damping whose mass is d_sw's half-updated delp; doubly periodic and sphere"""
    D.check_fv_step(emu, n_split=3, flags=dict(inline_q=True))
    D.check_fv_step(emu, nq=3, flags=dict(inline_q=True, do_vort_damp=True, vtdm4=0.06, nord=2, hord_tr=5))
    D.check_fv_step_hydrostatic(emu, n_split=3, flags=dict(inline_q=True))
    D.check_fv_step_hydrostatic(emu, flags=dict(inline_q=True, do_vort_damp=True, vtdm4=0.06, nord=1))
    r = PC.check_jw_step(emu, npx=13, npz=12, k_split=2, n_split=2, bdt=900.0, hydrostatic=False, nq=2, flags=dict(inline_q=True))
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12
    r = PC.check_jw_step(emu, npx=13, npz=12, k_split=1, n_split=2, bdt=900.0, hydrostatic=True, nq=2,
                         flags=dict(inline_q=True, do_vort_damp=True, vtdm4=0.06, nord=2))
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


def test_fill2d(emu):
    """fill2D (fv_fill.F90:183-258): the kernels against the oracle, then after tracer_2d in whole steps (hord_tr < 8, moist_phys)"""
    assert T.check_fill2d(emu) <= 1e-15
    assert T.check_fill2d(emu, nx=33, ny=9, npz=3) <= 1e-15
    D.check_fv_step(emu, flags=dict(hord_tr=5), fill2d=(0, 1), q_range=(-0.3, 1.0))
    r = PC.check_jw_step(emu, npx=13, npz=12, k_split=2, n_split=2, bdt=900.0, hydrostatic=False, nq=2, flags=dict(hord_tr=5),
                         fill2d=(0,), q_shift=1.0)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


def test_prt_maxmin_and_the_reference_timers(emu):
    """f4: prt_mxm (tools/fv_diagnostics.F90:4265-4313) -- max, min and g_sum's area mean of the last level (fv_grid_utils.F90:2879-2925),
    restated here in the reference's loop order -- and fv3_profile's events under the reference's timing_on / timing_off names"""
    import math
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynCore, DynFlags
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    from gfdl_atmos_cubed_sphere_amd.lib import Context
    bd = Bounds(1, 37, 1, 22)
    g = P.make_grid(bd, True)
    rng = np.random.default_rng(8)
    q = np.asfortranarray(rng.normal(250.0, 30.0, bd.shape("A", 7)))
    area = np.asarray(g.m["area"])
    ctx = Context(g, 7, lib=emu)
    try:
        got = ctx.prt_maxmin(ctx.from_host(q), 0.01)
        c = (slice(bd.ng, bd.ng + bd.nx), slice(bd.ng, bd.ng + bd.ny))
        gsum = 0.0
        for j in range(bd.ng, bd.ng + bd.ny):          # g_sum's "quick local sum": do j; do i
            for i in range(bd.ng, bd.ng + bd.nx):
                gsum = gsum + q[i, j, 6] * area[i, j]
        garea = math.fsum(area[c].ravel())
        assert got[0] == q[c].max() * 0.01 and got[1] == q[c].min() * 0.01
        assert abs(got[2] - gsum / garea * 0.01) <= 4e-16 * abs(got[2])
        # the timers: a substep loop under fv3_profile, reported under the reference's names
        st, dp0 = D.make_state(Bounds(1, 37, 1, 22), 7)
        dc = DynCore(ctx, DynFlags(n_split=2, ptop=N.PTOP), dp0)
        dc.set_state(st["u"], st["v"], st["w"], st["delp"], st["pt"], st["delz"], st["phis"])
        ctx.profile(True)
        dc.run(4.0)
        per_kernel = ctx.profile_report()
        dc.run(4.0)
        timers = ctx.profile_report_timers()
        ctx.profile(False)
        assert set(timers) <= {"C_SW", "D_SW", "UPDATE_DZ_C", "UPDATE_DZ", "Riem_Solver", "PG_D", "COMM_TOTAL", "tracer_2d", "Fill2D", "Remapping",
                               "DYN_CORE"}
        assert {"C_SW", "D_SW", "UPDATE_DZ_C", "UPDATE_DZ", "Riem_Solver", "PG_D", "COMM_TOTAL"} <= set(timers)
        assert sum(n for n, _ in timers.values()) == sum(n for n, _ in per_kernel.values())     # every launch under exactly one timer
        assert timers["Riem_Solver"][0] == per_kernel["riem_solver3"][0] + per_kernel["riem_solver_c"][0] == 4
    finally:
        ctx.close()


def test_remap_in_lds_and_in_slabs(emu):
    """Lagrangian_to_Eulerian with the column in LDS (csrc/remap_fast.h: levels across the lanes, the spline's elimination in the
    reference's order by hand-over rounds, the limiters' curvature re-formed from a one-byte code) -- the default where it is built, and
    BIT-IDENTICAL to the oracle like the slab kernels (csrc/remap_kernels.h), which the same cases run through with
    FV3_MI355X_REMAP_LDS=0 and which keep what the LDS kernels are not built for (kord_tm > 0, remap_te)"""
    for kw in (dict(), dict(km=20, nx=33, ny=9), dict(hydrostatic=True), dict(last_step=True, adiabatic=False),
               dict(hydrostatic=True, last_step=True, adiabatic=False, kord_tm=-10, kord=10), dict(kord=9, kord_tm=-9, nq=7),
               dict(km=127, nx=17, ny=3, nq=1), dict(km=79, nq=4, kord=13, kord_tm=-14), dict(kord=15, kord_tm=-15, km=8)):
        assert R.check_remap(emu, **kw) == 0.0
        assert R.check_remap(emu, lds=False, **kw) == 0.0
    # round 4, second half: use_cond / moist_kappa in the LDS kernels too (RemapFastScalars<false, true>: cappa from moist_cv of the
    # un-remapped tracers in the temperature transform, of the remapped ones in pkz, the last step's conversion with the condensates)
    for kw in (dict(moist_kappa=True), dict(moist_kappa=True, use_cond=True, last_step=True, kord_tm=-8, nwat=6, adiabatic=False),
               dict(moist_kappa=False, use_cond=True, last_step=True, kord_tm=-8, nwat=6, adiabatic=False),
               dict(moist_kappa=True, use_cond=True, kord_tm=-9, nwat=3, km=79, nx=17, ny=3)):
        assert R.check_remap(emu, **kw) == 0.0
        assert R.check_remap(emu, lds=False, **kw) == 0.0
    # ... and flagstruct%fill: fillz on the column in LDS, one thread per column that holds a negative value
    for kw in (dict(fill=True), dict(fill=True, nq=7, kord=9, kord_tm=-9), dict(fill=True, km=79, nx=17, ny=3, nq=3),
               dict(fill=True, moist_kappa=True, use_cond=True, nwat=6)):
        assert R.check_remap(emu, **kw) == 0.0
        assert R.check_remap(emu, lds=False, **kw) == 0.0
    # 5 levels per lane up to km = 79, 8 from km = 80 (RemapFastCoreT<L>): both sides of the switch, many tracers on few levels
    for kw in (dict(km=79, nx=17, ny=3, nq=3), dict(km=78, nx=17, ny=3, nq=1, hydrostatic=True), dict(km=80, nx=17, ny=3, nq=1),
               dict(km=5, nx=17, ny=3), dict(km=79, nq=9, kord=9, kord_tm=-9, last_step=True, adiabatic=False)):
        assert R.check_remap(emu, **kw) == 0.0
    assert R.check_remap(emu, kord_tm=9) <= 1e-14


def test_remap_te(emu):
    """flagstruct%remap_te (fv_mapz.F90:232-286, :348-360, :576-619, :655-663): total energy through map_scalar (kord_tm /= 0) or
    map1_cubic (kord_tm = 0), T_v and pkz from it; columns, then whole steps on both domains"""
    for kw in (dict(), dict(kord_tm=9), dict(kord_tm=0), dict(hydrostatic=True), dict(hydrostatic=True, kord_tm=0),
               dict(last_step=True, adiabatic=False), dict(hydrostatic=True, last_step=True, adiabatic=False, kord_tm=10),
               dict(moist_kappa=True), dict(moist_kappa=True, use_cond=True, last_step=True, adiabatic=False)):
        assert R.check_remap(emu, remap_te=True, **kw) <= 1e-14
    D.check_fv_step(emu, remap_te=True)
    D.check_fv_step(emu, remap_te=True, kord_tm=0, nq=0)
    D.check_fv_step_hydrostatic(emu, remap_te=True)
    D.check_fv_cycle_consv(emu, remap_te=True)                       # te_2d of the energy fixer from the remapped energy (:655-663)
    D.check_fv_cycle_consv(emu, hydrostatic=True, remap_te=True)
    r = PC.check_jw_step(emu, npx=13, npz=12, k_split=2, n_split=2, bdt=900.0, hydrostatic=False, nq=1, remap_te=True)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12
    r = PC.check_jw_step(emu, npx=13, npz=12, k_split=1, n_split=2, bdt=900.0, hydrostatic=True, remap_te=True, kord_tm=0)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


def test_nh_halos_and_geopk(emu):
    N.check_halos_and_geopk(emu)


# ---- whole acoustic substeps ---------------------------------------------------------------------
import parity_dyn as D


def test_dyn_core_substeps(emu):
    print(D.check_substeps(emu, n_split=2))


def test_dyn_core_substeps_sim_solver_damping(emu):
    D.check_substeps(emu, n_split=3, flags=dict(a_imp=0.75, nord=2, do_vort_damp=True, vtdm4=0.06, dddmp=0.2))


# ---- vertical remap -----------------------------------------------------------------------------
import parity_remap as R


@pytest.mark.parametrize("hydrostatic,last_step,kord_tm,kord,nq", [(False, False, -8, 8, 2), (False, True, -9, 9, 6),
                                                                    (True, False, -8, 8, 1), (False, False, 8, 10, 0),
                                                                    (True, True, 10, 11, 3), (False, True, -10, 13, 2),
                                                                    (False, True, -14, 14, 3), (True, False, 15, 15, 7),
                                                                    (False, False, -15, 14, 6), (False, True, -12, 12, 4),
                                                                    (True, False, 12, 12, 7)])
def test_remap(emu, hydrostatic, last_step, kord_tm, kord, nq):
    R.check_remap(emu, hydrostatic=hydrostatic, last_step=last_step, kord_tm=kord_tm, kord=kord, nq=nq)


@pytest.mark.parametrize("hydrostatic,last_step,kord_tm,kord,nq", [(False, False, -7, 7, 3), (True, True, 7, 7, 6), (False, True, -6, 6, 2),
                                                                    (True, False, 5, 5, 7), (False, False, -4, 4, 3), (False, True, 4, 3, 2),
                                                                    (True, False, -9, -8, 2), (False, True, -10, 6, 0)])
def test_remap_ppm_profile(emu, hydrostatic, last_step, kord_tm, kord, nq):
    """kord <= 7: the map routines take ppm_profile + ppm_limiters (fv_operators.F90:1382-1723) instead of cs_profile: Huynh's
    2nd constraint (7), the positive-definite / full-monotonicity / standard limiters (6, 5, 4, 3), for winds, w, T (|kord_tm|)
    and tracers (iv = -1, -2, 1, 0); a NEGATIVE kord_mt / kord_tr also fails the reference's "kord > 7" test and lands there.
    The tracers of the two cases with nq > 5 go through mapn_tracer, which has no such test and runs scalar_profile whatever the
    kord (fv_operators.F90:273, case (0:8) at :753; held to the reference's compiled mapn_tracer by tests/test_reference_pin.py)."""
    R.check_remap(emu, hydrostatic=hydrostatic, last_step=last_step, kord_tm=kord_tm, kord=kord, nq=nq)


@pytest.mark.parametrize("nt,nq,kord", [(1, 4, 9), (2, 5, 10), (3, 4, 9), (3, 5, 8), (3, 7, 10), (3, 7, 11), (3, 3, 13)])
def test_remap_tracer_groups(emu, nt, nq, kord, monkeypatch):
    """tracers remapped side by side in groups of up to nt per thread (remap_tracers_col): even dealing (4 = 2 + 2,
    7 = 3 + 2 + 2), both tracer forms (nq <= 5, nq > 5), |kord| = 11 falling back to one tracer at a time"""
    monkeypatch.setenv("FV3_MI355X_REMAP_NT", str(nt))
    R.check_remap(emu, nq=nq, kord=kord, last_step=True)
    R.check_remap(emu, nq=nq, kord=kord, hydrostatic=True, kord_tm=-kord if kord != 13 else -10, fill=(nq == 7))


# ---- tracer_2d -------------------------------------------------------------------------------------
import parity_tracer as T


def test_tracer_2d(emu):
    _, nsplt = T.check_tracer_2d(emu)
    assert nsplt == 1
    _, nsplt = T.check_tracer_2d(emu, big_courant=True, hord=-5)
    assert nsplt > 1
    T.check_tracer_2d(emu, q_split=2, trdm=0.06, nord_tr=1, hord=10)
    T.check_tracer_2d(emu, nx=33, ny=9, npz=7, nq=7, big_courant=True)


@pytest.mark.parametrize("nt", [1, 2, 3, 4])
def test_tracer_2d_tracers_per_wavefront(emu, nt, monkeypatch):
    """the sub-cycle kernel with 1..4 tracers per wavefront (short last group, finished levels, sub-cycling)"""
    monkeypatch.setenv("FV3_MI355X_TRACER_NT", str(nt))
    T.check_tracer_2d(emu, nx=70, ny=21, npz=3, nq=5, big_courant=True)
    T.check_tracer_2d(emu, nq=4, hord=10)


@pytest.mark.parametrize("nq,k_split", [(2, 2), (0, 1)])
def test_fv_dynamics_step(emu, nq, k_split):
    import parity_dyn as D
    D.check_fv_step(emu, nq=nq, k_split=k_split)


@pytest.mark.parametrize("hord,hord_mt", [(10, 10), (8, 6), (5, 5), (6, 8)])
def test_d_sw_multi_strip_march(emu, hord, hord_mt):
    """several 58-column strips and several row segments of the wave-marching kernels"""
    P.check_d_sw(emu, nx=130, ny=100, npz=3, par_over=dict(hord_dp=hord, hord_tm=hord, hord_vt=hord, hord_mt=hord_mt))


@pytest.mark.parametrize("hydrostatic", [False, True])
@pytest.mark.parametrize("hord,hord_mt", [(10, 10), (8, 6), (5, 5), (-5, 8), (6, 8)])
def test_d_sw_uniform_metrics(emu, hord, hord_mt, hydrostatic):
    """Cartesian doubly periodic gridstruct (Grid::geom == 2): the kernels that carry the metric terms as scalars"""
    P.check_d_sw(emu, nx=130, ny=64, npz=3, perturb=False, hydrostatic=hydrostatic,
                 par_over=dict(hord_dp=hord, hord_tm=hord, hord_vt=hord, hord_mt=hord_mt))


@pytest.mark.parametrize("perturb", [False, "ortho"])
def test_geometry_modes_off_same_result(emu, perturb, monkeypatch):
    """FV3_MI355X_GEOM=0 sends an orthogonal / uniform gridstruct through the general kernels: same parity"""
    monkeypatch.setenv("FV3_MI355X_GEOM", "0")
    P.check_c_sw(emu, nx=70, ny=30, npz=2, perturb=perturb)
    P.check_d_sw(emu, nx=70, ny=30, npz=2, perturb=perturb)


@pytest.mark.parametrize("nx,ny,hydro", [(130, 100, False), (55, 44, True)])
def test_c_sw_multi_strip_march(emu, nx, ny, hydro):
    P.check_c_sw(emu, nx=nx, ny=ny, npz=2, hydrostatic=hydro)


def test_update_dz_d_and_tracers_multi_strip_march(emu):
    import parity_tracer as T
    N.check_update_dz_d(emu, nx=130, ny=100, km=3)
    T.check_tracer_2d(emu, nx=130, ny=100, npz=3, nq=2)
    T.check_tracer_2d(emu, nx=70, ny=60, npz=3, nq=2, big_courant=True)


def test_halo_pack_unpack_kernels(emu):
    P.check_halo_packed(emu)


@pytest.mark.parametrize("hydro,n_con,nmax", [(False, None, 2), (True, None, 3), (False, 2, 1)])
def test_heat_source_path(emu, hydro, n_con, nmax):
    N.check_heat_source_path(emu, hydrostatic=hydro, n_con=n_con, nmax=nmax)


def test_dyn_core_substeps_with_dissipative_heating(emu):
    D.check_substeps(emu, n_split=2, flags=dict(d_con=1.0, do_vort_damp=True, vtdm4=0.06, nord=2))
    D.check_substeps(emu, n_split=2, flags=dict(d_con=0.5))


@pytest.mark.parametrize("d_ext", [0.02, 0.0])
def test_one_grad_p_hydrostatic(emu, d_ext):
    N.check_one_grad_p(emu, d_ext=d_ext)


def test_dyn_core_substeps_hydrostatic(emu):
    D.check_substeps_hydrostatic(emu)
    D.check_substeps_hydrostatic(emu, nx=70, ny=60, npz=6, flags=dict(d_ext=0.0))
    D.check_substeps_hydrostatic(emu, n_split=3, flags=dict(d_con=1.0, do_vort_damp=True, vtdm4=0.06, nord=2))


def test_fv_dynamics_step_hydrostatic(emu):
    D.check_fv_step_hydrostatic(emu)


def test_fv_dynamics_cycle_from_temperature(emu):
    D.check_fv_cycle_from_temperature(emu)


def test_d_sw_interior_then_rest_equals_d_sw(emu):
    """3 x 3 strips/segments: the interior box first, the frame afterwards (halo-exchange overlap form)"""
    assert max(P.check_d_sw(emu, nx=130, ny=100, npz=3, phases=True).values()) <= P.TOL
    assert max(P.check_d_sw(emu, nx=130, ny=100, npz=3, hydrostatic=True, phases=True).values()) <= P.TOL
    assert max(P.check_d_sw(emu, nx=40, ny=19, npz=3, phases=True).values()) <= P.TOL      # no interior: rest does all


@pytest.mark.parametrize("nx,ny,tj", [(130, 100, None), (117, 100, None), (175, 100, None), (130, 97, 8), (131, 26, 8),
                                      (118, 98, 8), (119, 99, 8)])
def test_d_sw_interior_does_not_read_halos_in_flight(emu, nx, ny, tj, monkeypatch):
    """uc, vc halos poisoned during 'interior' and restored before 'rest': shapes whose last strip owns 1-3 cells
    (nx % 58 = 1, 2, 3) or whose last segment has 1-3 rows"""
    if tj:
        monkeypatch.setenv("FV3_MI355X_MARCH_TJ_FUSED", str(tj))
    assert max(P.check_d_sw(emu, nx=nx, ny=ny, npz=3, phases="poison").values()) <= P.TOL


@pytest.mark.parametrize("nx,ny", [(6, 5), (58, 48), (59, 49), (117, 97), (8, 64), (61, 4)])
def test_march_strip_and_segment_boundaries(emu, nx, ny):
    """tiny tiles, exactly one strip / segment, one column / row more than a strip / segment, ragged last ones"""
    assert P.check_c_sw(emu, nx=nx, ny=ny, npz=2) <= P.TOL
    assert max(P.check_d_sw(emu, nx=nx, ny=ny, npz=3).values()) <= P.TOL
    assert max(P.check_d_sw(emu, nx=nx, ny=ny, npz=3, hydrostatic=True, phases=True).values()) <= P.TOL


@pytest.mark.parametrize("state", ["rest", "tophat", "checker"])
@pytest.mark.parametrize("hord", [10, 5])
def test_limiter_branch_point_states(emu, state, hord):
    """no wind + constant scalars (all Courant numbers / slopes exactly zero), top-hats, 2-cell oscillations"""
    assert P.check_c_sw(emu, nx=64, ny=40, npz=2, state=state) <= P.TOL
    over = dict(hord_dp=hord, hord_tm=hord, hord_vt=hord, hord_mt=hord)
    assert max(P.check_d_sw(emu, nx=64, ny=40, npz=3, state=state, par_over=over).values()) <= P.TOL


def test_error_behaviour_of_the_c_abi(emu):
    """the reference aborts through mpp_error(FATAL); the C ABI returns a status and a message instead"""
    import ctypes as C
    from gfdl_atmos_cubed_sphere_amd import lib as L
    from gfdl_atmos_cubed_sphere_amd.grid import doubly_periodic
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    bd = Bounds(1, 8, 1, 8)
    g = doubly_periodic(bd, 9, 9)
    ctx = L.Context(g, 2, lib=emu)
    try:
        a, b = ctx.zeros("A", 2), ctx.zeros("A", 2)
        with pytest.raises(L.Fv3Error, match="hord"):
            ctx.fv_tp_2d(a, a, a, 3, a, a, a, a)                       # unsupported scheme
        par = dict(P.DSW_PAR, hydrostatic=1, use_cond=0)
        u, v = ctx.zeros("U", 2), ctx.zeros("V", 2)
        cx, cy = ctx.zeros("CX", 2), ctx.zeros("CY", 2)
        fx, fy, cc = ctx.zeros("FX", 2), ctx.zeros("FY", 2), ctx.zeros("CC", 2)
        dv = ctx.zeros("B", 2)
        args = [par, None, a, a, u, v, None, v, u, a, a, dv, fx, fy, cx, cy, cx, cy, cx, cy, None, b, b, u, v, None, None,
                cc, cc]
        with pytest.raises(L.Fv3Error, match="coefficients"):
            ctx.d_sw(*args)                                            # per-level coefficients not uploaded
        from test_oracle_properties import default_levels
        ctx.dsw_levels(default_levels(2))
        with pytest.raises(L.Fv3Error, match="alias"):
            ctx.d_sw(*args)                                            # u_out aliases u
    finally:
        ctx.close()
    g.grid_type = 3                                                    # not a supported geometry (4, or 0..2 = cubed sphere)
    with pytest.raises(L.Fv3Error, match="grid_type"):
        L.Context(g, 2, lib=emu)
    g.grid_type, g.npx, g.npy = 0, 20, 20                              # a cubed-sphere context must be one whole face
    with pytest.raises(L.Fv3Error, match="whole face"):
        L.Context(g, 2, lib=emu)


def test_geometry_mode_detection(emu):
    """fv3_grid_upload classifies the gridstruct from its arrays (general / orthogonal / orthogonal + uniform)."""
    from gfdl_atmos_cubed_sphere_amd.lib import Context
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    bd = Bounds(1, 12, 1, 9)
    for perturb, want in ((True, 0), ("ortho", 1), (False, 2)):
        ctx = Context(P.make_grid(bd, perturb), 2, lib=emu)
        try:
            assert ctx.geom == want
        finally:
            ctx.close()


@pytest.mark.parametrize("a_imp", [1.0, 0.75])
def test_riem_solvers_fast_tau_w_sec(emu, a_imp):
    """fast_tau_w_sec > 0: the Rayleigh damping of w inside SIM1_solver / SIM_solver (nh_utils.F90:356-367, :1363-1371, :1498-1506),
    the levels-across-the-lanes kernels and the slab kernels, dry and moist"""
    N.check_riem_solver3(emu, a_imp=a_imp, tau_w=25.0)
    N.check_riem_solver3(emu, a_imp=a_imp, tau_w=25.0, lds=False, use_logp=True, last_call=True, fp_out=True)
    N.check_riem_solver3(emu, a_imp=a_imp, tau_w=40.0, use_cond=True, moist_kappa=True, nx=40, ny=9, km=19)
    if a_imp > 0.999:
        N.check_riem_solver_c(emu, tau_w=25.0)
        N.check_riem_solver_c(emu, tau_w=25.0, lds=False)
        N.check_riem_solver_c(emu, tau_w=25.0, use_cond=True, nx=40, ny=9, km=19)


@pytest.mark.parametrize("dims", [dict(), dict(nx=33, ny=9, km=3), dict(nx=70, ny=35, km=37), dict(nx=64, ny=32, km=16), dict(nx=31, ny=15, km=17)])
def test_nh_p_grad_in_one_kernel(emu, dims):
    """NhPGradFused (a2b_ord4 of pp, pk, gz, delp and nh_p_grad in one kernel: the corner values never leave LDS) against the oracle and,
    bit for bit, against the two-kernel path; tiles and layer chunks that end inside the domain / the column"""
    N.check_nh_p_grad_fused_bits(emu, **dims)


def test_consv_am(emu):
    """flagstruct%consv_am: compute_aam before and after the k_split loop, the reproducible sums, u00 and the wind correction
    (fv_dynamics.F90:358-361, :747-800, :1266-1314)"""
    N.check_consv_am_kernels(emu)
    D.check_fv_cycle_from_temperature(emu, consv_am=True)


def test_substeps_with_fast_tau_w_sec_and_rf_fast(emu):
    """the acoustic substeps with the Rayleigh damping of w inside the solvers and Ray_fast at their end (dyn_core.F90:536, :940, :1057-1060)"""
    npz = 10
    pfull = N.PTOP * 1.2 + (1.0e5 - N.PTOP) * (np.arange(npz) + 0.5) / npz
    fl = dict(fast_tau_w_sec=40.0, rf_fast=True, tau=0.002, rf_cutoff=float(pfull[4]) + 1.0)
    D.check_substeps(emu, npz=npz, n_split=3, bdt=6.0, flags=fl, pfull=pfull, ks=7)
    D.check_substeps(emu, npz=npz, n_split=2, bdt=4.0, flags=dict(fl, a_imp=0.75, rf_fast=False), pfull=pfull, ks=7)


@pytest.mark.parametrize("hydrostatic", [False, True])
def test_ray_fast(emu, hydrostatic):
    """Ray_fast (RF_fast, dyn_core.F90:1057-1060, :2485-2601), bit for bit; k_rf beyond kmax and no level above the cutoff too"""
    kmax, k_rf = N.check_ray_fast(emu, hydrostatic=hydrostatic)
    assert kmax == 7 and k_rf == 7
    N.check_ray_fast(emu, hydrostatic=hydrostatic, nx=64, ny=5, km=7, ks=2)            # k_rf < kmax
    assert N.check_ray_fast(emu, hydrostatic=hydrostatic, rf_cutoff=10.0) == (1, 0)    # nothing above the cutoff: rf = 1, nothing moves ...


@pytest.mark.parametrize("hydrostatic,conserve", [(False, True), (True, True), (False, False)])
def test_c2l_and_rayleigh_friction(emu, hydrostatic, conserve):
    """fv_dynamics around the k_split loop: cubed_to_latlon (ord 2, 4) and Rayleigh_Friction, grid_type = 4"""
    N.check_c2l_and_rayleigh(emu, hydrostatic=hydrostatic, conserve=conserve)


def test_fv_dynamics_call_with_rayleigh_friction(emu):
    """T -> pkz, Rayleigh_Friction, theta_v, k_split loop, last remap back to T, cubed_to_latlon"""
    D.check_fv_cycle_from_temperature(emu, tau=0.01)


@pytest.mark.parametrize("hydrostatic", [False, True])
def test_mix_dp(emu, hydrostatic):
    """mix_dp (flagstruct%fill_dp, dyn_core.F90:820, :2119-2200) against the oracle, bit for bit; then inside the substep loop"""
    N.check_mix_dp(emu, hydrostatic=hydrostatic)
    if hydrostatic:
        D.check_substeps_hydrostatic(emu, flags=dict(fill_dp=True))
    else:
        D.check_substeps(emu, flags=dict(fill_dp=True), akbk="thin")


def test_registry_forget(emu):
    """a host array that is freed and allocated again at the same address leaves the lazy registry"""
    P.check_registry_forget(emu)


def test_dyn_core_substeps_with_do_diss_est(emu):
    """flagstruct%do_diss_est through DynCore: d_sw's diss_e of every level summed into diss_est over the substeps (dyn_core.F90:805-811);
    with the heating on top (d_con = 1) in the second run"""
    D.check_substeps(emu, do_diss_est=True)
    D.check_substeps(emu, do_diss_est=True, flags=dict(d_con=1.0), npz=10)
    D.check_substeps_hydrostatic(emu, do_diss_est=True)


def test_fv_dynamics_call_with_rf_fast(emu):
    """flagstruct%tau > 0 with RF_fast given to FvDynamics: no Rayleigh_Friction (fv_dynamics.F90:362), Ray_fast after every acoustic
    substep instead (dyn_core.F90:1057-1060) -- ONE tau for both (with tau in two places this ran undamped)"""
    D.check_fv_cycle_from_temperature(emu, tau=0.002, rf_fast=True)


def test_fortran_host_drives_the_library(emu, tmp_path):
    """the Fortran host (fv3_host_mod + fv3_solo, amdflang) against the host-emulation build of the same C ABI"""
    import fortran_host as F
    if F.fortran_compiler() is None:
        pytest.skip("no Fortran compiler in this image")
    out = F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=8, nq=1)
    assert "fv3_solo: done" in out
    # the same with the group halo updates through the exchange behind the C ABI (fv3_halo_start / fv3_halo_complete)
    out = F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=8, nq=1, host_comm=True)
    assert "fv3_solo: done" in out
    # the hydrostatic branch of dyn_core (geopk, external-mode damping, one_grad_p) and the dissipative heating of both branches
    assert "fv3_solo: done" in F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=12, nq=1, hydrostatic=True)
    assert "fv3_solo: done" in F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=12, nq=1, hydrostatic=True, d_con=1.0)
    assert "fv3_solo: done" in F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=12, nq=0, hydrostatic=False, d_con=1.0)
    assert "fv3_solo: done" in F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=8, nq=2, hydrostatic=False, inline_q=True)
    assert "fv3_solo: done" in F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=8, nq=1, hydrostatic=True, inline_q=True, beta=0.3)
    # thermostruct%use_cond / moist_kappa through the Fortran loop: q_con in d_sw and the Riemann solvers, cappa, the moist remap
    assert "fv3_solo: done" in F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=8, nq=7, use_cond=True, moist_kappa=True, d_con=1.0)
    assert "fv3_solo: done" in F.check_fortran_host(emu, tmp_path, nx=24, ny=16, npz=8, nq=6, use_cond=True)


def test_fortran_dyn_core_with_the_reference_argument_list(emu, tmp_path):
    """fv3_dyn_core_mod's dyn_core: the reference's argument list (model/dyn_core.F90:94-98: host arrays with the fv_arrays bounds,
    gridstruct / flagstruct / bd by their reference names) over the device-resident loop; both branches, with the heating"""
    import fortran_host as F
    if F.fortran_compiler() is None:
        pytest.skip("no Fortran compiler in this image")
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path)
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=12, d_con=1.0)
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=12, hydrostatic=True, d_con=1.0)
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=8, beta=0.4)
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=8, nsteps=3, registry=True)    # the lazy host-address registry
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=8, hydrostatic=True, d_con=1.0, registry=True)
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=10, fast_tau_w_sec=40.0, rf_fast_tau=0.002)   # fast_tau_w_sec, RF_fast
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=10, hydrostatic=True, rf_fast_tau=0.002)
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=8, hydrostatic=True, beta=0.4)
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=8, moist=True, d_con=1.0)     # thermostruct%use_cond / moist_kappa
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=8, do_diss_est=True, d_con=1.0)   # flagstruct%do_diss_est: diss_est in and out
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=8, hydrostatic=True, do_diss_est=True)
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=8, fill_dp=True)          # flagstruct%fill_dp: mix_dp after d_sw
    assert "fv3_solo_refsig: done" in F.check_fortran_refsig(emu, tmp_path, npz=8, hydrostatic=True, fill_dp=True)
    # fv_dynamics with ITS reference argument list (model/fv_dynamics.F90:79-85): T -> theta_v, the k_split loop with tracers and
    # the remap, last_step, cubed_to_latlon
    assert "fv3_solo_refsig: done" in F.check_fortran_fv_dynamics(emu, tmp_path)
    assert "fv3_solo_refsig: done" in F.check_fortran_fv_dynamics(emu, tmp_path, hydrostatic=True, npz=12, nq=1)
    # thermostruct%use_cond = moist_kappa = .true. -- the reference's DEFAULTS (fv_arrays.F90:1226-1227) -- through the reference-signature
    # fv_dynamics: the water species by get_tracer_index, q_con / cappa formed by moist_cv inside, q_con handed back
    assert "fv3_solo_refsig: done" in F.check_fortran_fv_dynamics(emu, tmp_path, nq=7, moist=True)
    assert "fv3_solo_refsig: done" in F.check_fortran_fv_dynamics(emu, tmp_path, nq=6, moist=True, consv_te=1.0, npz=10)
    assert "fv3_solo_refsig: done" in F.check_fortran_fv_dynamics(emu, tmp_path, nq=1, do_diss_est=True)     # diss_est out of fv_dynamics
    assert "fv3_solo_refsig: done" in F.check_fortran_fv_dynamics(emu, tmp_path, nq=0, consv_am=True)        # flagstruct%consv_am
    assert "fv3_solo_refsig: done" in F.check_fortran_fv_dynamics(emu, tmp_path, nq=1, beta=-1.0, hybrid_z=True)             # one_grad_p in the nonhydrostatic loop (beta < -0.1); hybrid_z = .true. is accepted (the reference never reads it)


@pytest.mark.parametrize("use_cond,moist_kappa", [(True, False), (True, True), (False, True)])
@pytest.mark.parametrize("a_imp", [1.0, 0.75])
def test_riem_solvers_moist(emu, use_cond, moist_kappa, a_imp):
    """use_cond / moist_kappa branches of Riem_Solver3 (nh_core.F90:96-166) and Riem_Solver_c (nh_utils.F90:383-438)"""
    N.check_riem_solver3(emu, a_imp=a_imp, use_cond=use_cond, moist_kappa=moist_kappa)
    if a_imp > 0.999 and use_cond:
        N.check_riem_solver_c(emu, use_cond=True, moist_kappa=moist_kappa)


@pytest.mark.parametrize("moist_kappa,use_cond,last_step,kord_tm,nwat", [(True, True, False, -9, 6), (True, True, True, -8, 6),
                                                                          (False, True, True, -8, 6), (True, False, False, 9, 3)])
def test_remap_moist(emu, moist_kappa, use_cond, last_step, kord_tm, nwat):
    """moist_kappa / use_cond branches of Lagrangian_to_Eulerian (fv_mapz.F90:212-219, :463-478, :806-811) with moist_cv"""
    R.check_remap(emu, moist_kappa=moist_kappa, use_cond=use_cond, last_step=last_step, kord_tm=kord_tm, nwat=nwat,
                  adiabatic=False)


@pytest.mark.parametrize("kw", [dict(), dict(with_qv=False), dict(hydrostatic=True), dict(split=True),
                                dict(moist_kappa=True, use_cond=True), dict(moist_kappa=True, use_cond=True, split=True),
                                dict(use_cond=True), dict(hydrostatic=True, use_cond=True)])
def test_pt_to_theta_v(emu, kw):
    """T -> theta_v before the k_split loop (fv_dynamics.F90:296-329, :379-399), dry / zvir / moist_kappa / use_cond"""
    N.check_pt_to_theta_v(emu, **kw)


@pytest.mark.parametrize("moist_kappa", [True, False])
def test_fv_dynamics_call_moist(emu, moist_kappa):
    """whole fv_dynamics call with use_cond (+ moist_kappa): moist_cv conversions, q_con through d_sw and the Riemann
    solvers, moist remap, T on return"""
    D.check_fv_cycle_moist(emu, moist_kappa=moist_kappa)


def test_fv_dynamics_call_moist_heating(emu):
    """the dissipative heating of dyn_core with moist_kappa: pkz from the per-cell cappa (dyn_core.F90:1338-1340)"""
    D.check_fv_cycle_moist(emu, moist_kappa=True, flags=dict(d_con=1.0, do_vort_damp=True, vtdm4=0.06, nord=2))


@pytest.mark.parametrize("nq", [2, 6])
def test_remap_fillz(emu, nq):
    """flagstruct%fill: fillz (fv_fill.F90:34-137) on the remapped tracers, both tracer remap forms (nq <= 5, nq > 5)"""
    R.check_remap(emu, nq=nq, fill=True)


def test_baseline_config1_test_case_1(emu):
    """BASELINE configs[0]: doubly periodic 48 x 48 x 32, hydrostatic, the reference's test_case = 1 initial condition
    (uniform flow carrying a block of mass): one dt_atmos of the k_split loop (substeps, tracer_2d, remap) vs the oracle"""
    D.check_fv_step_hydrostatic(emu, nx=48, ny=48, npz=32, nq=1, k_split=1, n_split=3, bdt=6.0, ic="test_case_1")


@pytest.mark.parametrize("hord", [7, 9, 11, 12, 13])
def test_tracer_2d_positive_definite_schemes(emu, hord):
    """hord_tr = 9 / 13 (pert_ppm), 11 (ppm_fac slopes), 12 (Lin & Rood positive definite), tp_core.F90:604-641: the marching
    kernels (one and three tracers per wavefront) and, with the first sub-cycle damped, the tile kernel"""
    T.check_tracer_2d(emu, nq=4, hord=hord, big_courant=True)
    T.check_tracer_2d(emu, nx=70, ny=21, npz=3, nq=1, hord=hord)
    T.check_tracer_2d(emu, q_split=2, trdm=0.06, nord_tr=1, hord=hord)


@pytest.mark.parametrize("state", ["westward", "swirl"])
@pytest.mark.parametrize("hydrostatic", [False, True])
def test_reversed_and_mixed_winds_three_strips(emu, state, hydrostatic):
    """u < 0 / winds of both signs on 3 strips x 2-3 segments: every upwind select takes the other neighbour, also in the
    first and last lanes a strip owns (the default states have u > 0 everywhere)"""
    for perturb in (False, True):
        assert P.check_c_sw(emu, nx=130, ny=70, npz=3, hydrostatic=hydrostatic, perturb=perturb, state=state) <= P.TOL
        assert max(P.check_d_sw(emu, nx=130, ny=70, npz=3, hydrostatic=hydrostatic, perturb=perturb, state=state).values()) <= P.TOL


def test_reversed_winds_whole_substeps_and_tracers(emu):
    D.check_substeps(emu, nx=130, ny=30, npz=6, n_split=2, bdt=8.0, ic="westward")
    D.check_substeps_hydrostatic(emu, nx=96, ny=24, npz=6, n_split=2, bdt=8.0)
    D.check_substeps_hydrostatic(emu, nx=130, ny=30, npz=6, n_split=2, bdt=8.0, ic="westward")
    T.check_tracer_2d(emu, nx=130, ny=30, npz=3, nq=3, reverse=True)
    T.check_tracer_2d(emu, nx=130, ny=30, npz=3, nq=4, reverse=True, big_courant=True)


# ---- cubed sphere (grid_type < 3): the pass kernels against the oracle, all six faces ----------------------------------
import parity_cubed as PC


@pytest.mark.parametrize("hydrostatic", [False, True])
def test_cubed_c_sw(emu, hydrostatic):
    assert PC.check_c_sw(emu, npx=13, npz=3, hydrostatic=hydrostatic) <= P.TOL
    assert PC.check_c_sw(emu, npx=25, npz=2, hydrostatic=hydrostatic, faces=(0, 2, 5)) <= P.TOL


@pytest.mark.parametrize("hord", [10, 8, 5, -5, 6, 7, 9, 11, 12, 13])
def test_cubed_fv_tp_2d(emu, hord):
    assert PC.check_fv_tp_2d(emu, hord, faces=(0, 3)) <= P.TOL
    assert PC.check_fv_tp_2d(emu, hord, mass_flux=True, faces=(2, 5)) <= P.TOL


@pytest.mark.parametrize("kw", [dict(hydrostatic=True), dict(hydrostatic=True, flags=dict(nord=2)),
                                dict(hydrostatic=True, flags=dict(nord=3), faces=(1, 4)),
                                dict(hydrostatic=True, par_over=dict(hord_mt=5, hord_vt=5, hord_tm=5, hord_dp=5), faces=(0, 5)),
                                dict(hydrostatic=True, par_over=dict(hord_mt=6, hord_vt=6, hord_tm=6, hord_dp=-5), faces=(2,)),
                                dict(hydrostatic=True, par_over=dict(hord_mt=8, hord_vt=8, hord_tm=8, hord_dp=8), faces=(3,)),
                                dict(hydrostatic=True, par_over=dict(hord_mt=9), faces=(4,)),
                                dict(hydrostatic=False, flags=dict(n_sponge=-1))])
def test_cubed_d_sw(emu, kw):
    assert max(PC.check_d_sw(emu, npx=13, npz=3, **kw).values()) <= P.TOL


def test_cubed_c384_face_pair_vs_oracle(emu):
    """one gnomonic C384 face (7 strips of wavefronts, the width of BASELINE config 3): the ownership arithmetic of the cubed hybrid --
    marching interior with its store masks, frame passes, the fused frame kernel -- against the oracle (the GPU suite runs all six
    faces, both branches and the production damping set: test_cubed_c384_pair_vs_oracle)"""
    assert PC.check_c_sw(emu, npx=385, npz=3, hydrostatic=False, faces=(4,)) <= P.TOL
    assert max(PC.check_d_sw(emu, npx=385, npz=3, hydrostatic=False, faces=(4,)).values()) <= P.TOL


def test_cubed_d_sw_nonhydrostatic_default(emu):
    """the default level coefficients: del-2 damping of w in the sponge layer (damp_w > 0, nord_w = 0)"""
    assert max(PC.check_d_sw(emu, npx=13, npz=4, hydrostatic=False).values()) <= P.TOL


def test_cubed_sphere_nonhydrostatic_substeps(emu):
    """two substeps of the nonhydrostatic core on the whole C12 sphere: update_dz_c with fill_4corners, update_dz_d through the
    cubed fv_tp_2d, both Riemann solvers, nh_p_grad with the cubed a2b_ord4"""
    assert max(PC.check_substeps_nh(emu, npx=13, npz=5, n_split=2).values()) <= 1e-13


def test_cubed_a2b_ord4_through_the_pressure_gradients(emu):
    cs, gs = PC.CC.sphere(13)
    for t in (0, 3):
        N.check_nh_p_grad(emu, km=4, grid=gs[t])
        N.check_one_grad_p(emu, km=4, grid=gs[t], d_ext=0.0)


def test_cubed_halo_gather_equals_the_table_update(emu):
    """the device gather (fv3_gather_run) against the numpy application of the same topology tables, every field kind"""
    import numpy as np
    from gfdl_atmos_cubed_sphere_amd.cubed_halo import CubeHalo
    from gfdl_atmos_cubed_sphere_amd.lib import Context
    npx, npz = 9, 3
    cs, gs = PC.CC.sphere(npx)
    ctxs = [Context(g, npz, lib=emu) for g in gs]
    try:
        H = CubeHalo(ctxs, npx, topo=PC.CC.product_topo(npx))
        rng = np.random.default_rng(0)
        bd = gs[0].bd
        for kind, kinds in (("A", ("A",)), ("B", ("B",)), ("D", ("U", "V")), ("C", ("V", "U")), ("Dedge", ("U", "V"))):
            host = [[np.asfortranarray(rng.uniform(-1, 1, bd.shape(k, npz))) for _ in range(6)] for k in kinds]
            dev = [[ctxs[t].from_host(a[t]) for t in range(6)] for a in host]
            ref = [[x.copy(order="F") for x in a] for a in host]
            cs.topo.update(kind, ref[0] if len(kinds) == 1 else (ref[0], ref[1]))
            H.update(kind, dev[0] if len(kinds) == 1 else (dev[0], dev[1]))
            for m in range(len(kinds)):
                for t in range(6):
                    assert np.array_equal(dev[m][t].download(), ref[m][t]), (kind, m, t)
        H.close()
    finally:
        for c in ctxs:
            c.close()


def test_cubed_sphere_hydrostatic_substeps(emu):
    """two acoustic substeps of the hydrostatic core on the whole C12 sphere (six contexts, device halo gathers, edge sync
    of the last substep) against the six-face orchestration of the oracle"""
    assert max(PC.check_substeps_hydrostatic(emu, npx=13, npz=4, n_split=2).values()) <= 1e-13


def test_cubed_sphere_jablonowski_williamson_step(emu):
    """test_case = 13 on a C12 sphere with the reference's L79 levels: one dt_atmos (k_split = 2: substeps + remap)"""
    r = PC.check_jw_step(emu, npx=13, npz=79, k_split=2, n_split=2, bdt=1800.0)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


def test_cubed_sphere_jablonowski_williamson_nonhydrostatic_step(emu):
    """BASELINE configs[2] in small: the nonhydrostatic baroclinic wave on a C12 sphere, L79, one dt_atmos (k_split = 2)"""
    r = PC.check_jw_step(emu, npx=13, npz=79, k_split=2, n_split=2, bdt=900.0, hydrostatic=False)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


@pytest.mark.parametrize("kw", [dict(), dict(courant_scale=40.0, hord=5, nq=2), dict(courant_scale=70.0, hord=10, nq=1, q_split=0),
                                dict(q_split=2, hord=13, nq=1)])
def test_cubed_tracer_2d(emu, kw):
    """tracer_2d on the whole sphere: the Courant maximum reduced over the six faces, sub-cycled levels, q halos per sub-cycle"""
    assert PC.check_tracer_2d(emu, **kw)["q"] <= P.TOL


def test_cubed_sphere_jw_step_with_tracers(emu):
    r = PC.check_jw_step(emu, npx=13, npz=79, k_split=2, n_split=2, bdt=900.0, hydrostatic=True, nq=3)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12
    r = PC.check_jw_step(emu, npx=13, npz=20, k_split=1, n_split=2, bdt=900.0, hydrostatic=False, nq=2)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


# ---- cubed-sphere hybrid: faces wide enough that the marching kernels take the interior and the passes the frame ----------------
@pytest.mark.parametrize("kw", [dict(hydrostatic=True, npz=6), dict(hydrostatic=False, npz=12, faces=(1, 4)),
                                dict(hydrostatic=True, npz=12, faces=(2, 5), flags=dict(nord=2)),
                                dict(hydrostatic=True, npz=12, faces=(0,), par_over=dict(hord_mt=5, hord_vt=5, hord_tm=5, hord_dp=5)),
                                dict(hydrostatic=True, npz=12, faces=(3,), par_over=dict(hord_mt=6, hord_vt=6, hord_tm=6, hord_dp=-5)),
                                dict(hydrostatic=True, npz=12, faces=(4,), par_over=dict(hord_mt=8, hord_vt=8, hord_tm=8, hord_dp=8)),
                                dict(hydrostatic=True, npz=12, faces=(5,), par_over=dict(hord_mt=9)),
                                dict(hydrostatic=True, npz=12, faces=(1,), par_over=dict(hord_mt=11))])
def test_cubed_hybrid_d_sw(emu, kw):
    """C40 faces: the fused marching kernels over the whole face (interior formulas, frame masked) + the pass kernels on the
    frame; levels 1, 2 (sponge) stay with the full-face passes.  Bit for bit the oracle's d_sw."""
    assert max(PC.check_d_sw(emu, npx=41, **kw).values()) <= P.TOL


@pytest.mark.parametrize("hydrostatic", [False, True])
def test_cubed_hybrid_c_sw(emu, hydrostatic):
    """C48 faces: CswMarch over the whole face (cubed vt form, frame of 7 masked, no divergence), the passes on the frame, the
    non-orthogonal divergence as a pass of its own"""
    assert PC.check_c_sw(emu, npx=49, npz=3, hydrostatic=hydrostatic) <= P.TOL
    assert PC.check_c_sw(emu, npx=49, npz=3, hydrostatic=hydrostatic, nord=0, faces=(1,)) <= P.TOL


@pytest.mark.parametrize("lane_d2", ["1", "0"])
def test_cubed_hybrid_two_lanes(emu, monkeypatch, lane_d2):
    """the order of the two lanes (fv3_api.hip dsw_cubed / csw_cubed: the marching kernels first, the passes from their own work
    copies and, for the frame's transports, Courant numbers of their own) forced on faces of any size: on this harness the launches run
    one after the other, so what is tested is that no pass depends on the marching kernel overwriting it afterwards -- bit for bit the
    oracle's c_sw, d_sw and substeps (sphere: the six faces as a group)"""
    monkeypatch.setenv("FV3_MI355X_SIDE_STREAM", "2")
    monkeypatch.setenv("FV3_MI355X_LANE_D2", lane_d2)
    assert PC.check_c_sw(emu, npx=49, npz=3, hydrostatic=False) <= P.TOL
    assert PC.check_c_sw(emu, npx=49, npz=3, hydrostatic=True, nord=0, faces=(1,)) <= P.TOL
    assert max(PC.check_d_sw(emu, npx=41, hydrostatic=False, npz=12, faces=(1, 4)).values()) <= P.TOL
    assert max(PC.check_d_sw(emu, npx=41, hydrostatic=True, npz=12, faces=(2, 5), flags=dict(nord=2)).values()) <= P.TOL
    assert max(PC.check_substeps_nh(emu, npx=33, npz=12, n_split=2).values()) <= 1e-13
    # every level damped (production namelist): the momentum half up to the absolute vorticity beside the transport half
    prod_flags = dict(do_vort_damp=True, vtdm4=0.06, nord=3, d_con=1.0, dddmp=0.5)
    assert max(PC.check_d_sw(emu, npx=41, npz=6, hydrostatic=False, faces=(0, 4), flags=prod_flags, par_over=dict(dddmp=0.5)).values()) <= P.TOL


def test_cubed_hybrid_c_sw_frame_is_not_marginal(emu, monkeypatch):
    """d2a2c_vect's edge forms reach six points into a face (npt = 4, the 4-point A -> C interpolation, ke, the wind update)"""
    monkeypatch.setenv("FV3_MI355X_CUBED_FRAME_C", "6")
    monkeypatch.setenv("FV3_MI355X_CUBED_REACH", "3")
    assert PC.check_c_sw(emu, npx=49, npz=3, hydrostatic=False, faces=(0, 3)) <= P.TOL


def test_cubed_hybrid_substeps(emu):
    assert max(PC.check_substeps_hydrostatic(emu, npx=33, npz=12, n_split=2).values()) <= 1e-13
    assert max(PC.check_substeps_nh(emu, npx=33, npz=12, n_split=2).values()) <= 1e-13


def test_cubed_hybrid_frame_width_is_not_marginal(emu, monkeypatch):
    """the frame the passes own is 4 wide with intermediates 5 wider; 3 + 3 already reproduces the oracle (the edge rules of the
    PPM operators touch three cells), so the defaults carry a margin"""
    monkeypatch.setenv("FV3_MI355X_CUBED_FRAME", "3")
    monkeypatch.setenv("FV3_MI355X_CUBED_REACH", "3")
    assert max(PC.check_d_sw(emu, npx=41, npz=12, hydrostatic=False, faces=(0, 3)).values()) <= P.TOL


def test_cubed_hybrid_tracers_and_pressure_gradient(emu):
    """the other hybrids: tracer_2d (marching kernels + frame passes per tracer, sub-cycled levels), a2b_ord4 in the pressure
    gradients (LDS-tile kernel in the sum form of the cubed branch + frame passes), update_dz_d (ZhMarch + frame) in a
    nonhydrostatic Jablonowski-Williamson step with tracers on C32 faces"""
    assert PC.check_tracer_2d(emu, npx=33, npz=6, nq=5, courant_scale=100.0, hord=5)["q"] <= P.TOL
    assert PC.check_tracer_2d(emu, npx=41, npz=6, nq=2, q_split=2, hord=13)["q"] <= P.TOL
    cs, gs = PC.CC.sphere(41)
    for t in (0, 3, 5):
        N.check_nh_p_grad(emu, km=4, grid=gs[t])
        N.check_one_grad_p(emu, km=4, grid=gs[t], d_ext=0.0)
    r = PC.check_jw_step(emu, npx=33, npz=20, k_split=1, n_split=2, bdt=900.0, hydrostatic=False, nq=2)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


def test_exchange_behind_the_c_abi_single_rank(emu):
    """fv3_comm_init + fv3_halo_start / fv3_halo_complete (the transfers inside the library; here the host-emulation build's
    self copies) fill the halos of every field kind like the periodic fill, and a substep loop driven through them equals the
    oracle"""
    import numpy as np
    from gfdl_atmos_cubed_sphere_amd.halo import HaloExchanger
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds, periodic_fill
    from gfdl_atmos_cubed_sphere_amd.lib import Context
    bd = Bounds(1, 14, 1, 9)
    g = P.make_grid(bd, False)
    ctx = Context(g, 3, lib=emu)
    try:
        hx = HaloExchanger(ctx, 1, 1, 0, 1, native=True)
        rng = np.random.default_rng(2)
        host = {k: np.asfortranarray(rng.uniform(-1, 1, bd.shape(k, 3))) for k in ("A", "U", "V", "B")}
        dev = {k: ctx.from_host(v) for k, v in host.items()}
        hx.update([(dev[k], k) for k in ("A", "U", "V", "B")])
        for k, v in host.items():
            ref = v.copy(order="F")
            for n in range(3):
                periodic_fill(bd, ref[:, :, n], k)
            assert np.array_equal(dev[k].download(), ref), k
        # several groups (> 8 fields) and the deferred start / finish protocol of the overlapped d_sw
        many = [(ctx.from_host(host["A"]), "A") for _ in range(11)]
        pend = hx.start(many, defer=True)
        hx.post(pend)
        hx.finish(pend)
        ref = host["A"].copy(order="F")
        for n in range(3):
            periodic_fill(bd, ref[:, :, n], "A")
        assert all(np.array_equal(f.download(), ref) for f, _ in many)
        assert np.array_equal(ctx.allreduce_max(np.array([1.0, -2.0])), [1.0, -2.0])
    finally:
        ctx.close()


# ---- cubed sphere: the damping / heating branches a production namelist switches on ------------------------------------------------
PROD = dict(do_vort_damp=True, vtdm4=0.06, nord=3, d_con=1.0, dddmp=0.5)


@pytest.mark.parametrize("hydrostatic", [True, False])
@pytest.mark.parametrize("kw", [dict(flags=dict(do_vort_damp=True, vtdm4=0.06, nord=2)), dict(flags=dict(d_con=1.0)),
                                dict(flags=dict(dddmp=0.2, nord=2), par_over=dict(dddmp=0.2)),
                                dict(flags=PROD, par_over=dict(dddmp=0.5))])
def test_cubed_d_sw_damping_and_heating(emu, kw, hydrostatic):
    """deln_flux on delp / pt, del6_vt_flux on w and on the relative vorticity (copy_corners as index maps), Smagorinsky damping
    through the cubed a2b_ord4, the dissipative heat source: d_sw on the faces against the oracle, heat_source included"""
    assert max(PC.check_d_sw(emu, npx=13, npz=12, hydrostatic=hydrostatic, faces=(0, 3), **kw).values()) <= P.TOL


@pytest.mark.parametrize("hydrostatic", [True, False])
def test_cubed_d_sw_damping_fused_chains(emu, hydrostatic):
    """the same on a C32 face, where the del-2n chains run as one LDS-tile launch away from the corners (cubed_damp.h DelnFused) and
    the damped whole-face levels take the fused transport with delp's damping fluxes as an input (cubed_tpf.h): equal to the passes"""
    assert max(PC.check_d_sw(emu, npx=33, npz=17, hydrostatic=hydrostatic, faces=(0, 5), flags=PROD, par_over=dict(dddmp=0.5)).values()) <= P.TOL
    assert max(PC.check_d_sw(emu, npx=33, npz=3, hydrostatic=hydrostatic, faces=(2,),
                             flags=dict(do_vort_damp=True, vtdm4=0.06, nord=1)).values()) <= P.TOL


@pytest.mark.parametrize("kw", [dict(flags=dict(d_con=1.0), grid_flags=dict(do_diss_est=True, prevent_diss_cooling=False)),
                                dict(flags=dict(), grid_flags=dict(do_diss_est=True, prevent_diss_cooling=True)),
                                dict(flags=PROD, par_over=dict(dddmp=0.5), grid_flags=dict(do_diss_est=True, prevent_diss_cooling=True))])
def test_cubed_d_sw_dissipation_estimate(emu, kw):
    """do_diss_est on a cubed-sphere face (sw_core.F90:964-978, :1462, :1516-1586): diss_est of every level, with and without the
    heating, the vorticity damping and the cooling limiter; the work arrays are zeroed where nothing damps the vorticity"""
    assert max(PC.check_d_sw(emu, npx=13, npz=6, hydrostatic=False, faces=(1, 4), **kw).values()) <= P.TOL


@pytest.mark.parametrize("hydrostatic,conserve", [(False, True), (True, True), (False, False)])
def test_cubed_sphere_rayleigh_friction(emu, hydrostatic, conserve):
    """Rayleigh_Friction on the six faces: u2f through the cubed-sphere cubed_to_latlon, its halo across the cube edges, heating +
    implicit damping of u, v, w (fv_dynamics.F90:1126-1264)"""
    assert PC.check_rayleigh(emu, npx=13, hydrostatic=hydrostatic, conserve=conserve) <= 1e-14


@pytest.mark.parametrize("moist_kappa", [True, False])
def test_cubed_sphere_moist_fv_dynamics_call(emu, moist_kappa):
    """use_cond (+ moist_kappa) through a whole nonhydrostatic fv_dynamics call on the six faces: moist_cv conversion, q_con in d_sw
    and both Riemann solvers with its halo across the cube edges, moist remap, back to T (SURVEY 8(f) item 3 on the sphere)"""
    r = PC.check_jw_step_moist(emu, npx=13, npz=12, moist_kappa=moist_kappa)
    assert max(r.values()) <= 1e-12


@pytest.mark.parametrize("hydrostatic,ideal", [(False, False), (True, False), (False, True)])
def test_cubed_sphere_rayleigh_super(emu, hydrostatic, ideal):
    """Rayleigh_Super, the form fv_dynamics applies on the cubed sphere for tau > 0 (fv_dynamics.F90:362-366, :953-1124), through the
    host's dispatch on the six faces; is_ideal_case: relaxation towards the winds of the first call"""
    assert PC.check_rayleigh_super(emu, npx=13, hydrostatic=hydrostatic, ideal=ideal) <= 1e-14


@pytest.mark.parametrize("kw", [dict(), dict(hydrostatic=True), dict(hydrostatic=True, adiabatic=True), dict(adiabatic=True),
                                dict(consv_te=-2.0), dict(consv_te=-2.0, hydrostatic=True)])
def test_total_energy_conservation(emu, kw):
    """consv_te: compute_total_energy before the loop, the energy fixer of the last remap (te_2d, zsum0 / zsum1, the reproducing
    global sums, dtmp) and the final T_v -> T step with dtmp; a prescribed flux for consv_te < 0; the energy of the final state
    closes on the initial one"""
    assert max(D.check_fv_cycle_consv(emu, **kw).values()) <= 1e-12


def test_energy_fixer_refuses_an_unset_or_stale_te0(emu):
    """a bare step(..., last_cycle_is_last_step=True) with consv_te > 0 never computed te0_2d (step_from_temperature does,
    fv_dynamics.F90:345-355); the fixer must stop instead of applying dtmp = -E / zsum to pt, and a te0_2d of an earlier call must
    not be reused"""
    import numpy as np
    from gfdl_atmos_cubed_sphere_amd import synthetic as N
    from gfdl_atmos_cubed_sphere_amd.dyn_core import DynFlags
    from gfdl_atmos_cubed_sphere_amd.fv_dynamics import FvDynamics
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    from gfdl_atmos_cubed_sphere_amd.lib import Context
    bd, npz = Bounds(1, 16, 1, 12), 6
    g = P.make_grid(bd, False)
    st, _ = N.balanced_nh_state(bd, npz)
    sig = np.linspace(0.0, 1.0, npz + 1) ** 1.5
    ak, bk = N.PTOP * (1.0 - sig), sig.copy()
    ctx = Context(g, npz, lib=emu)
    try:
        fv = FvDynamics(ctx, DynFlags(n_split=2, ptop=N.PTOP), ak, bk, nq=0, k_split=1, consv_te=1.0)
        fv.dc.set_state(st["u"], st["v"], st["w"], st["delp"], st["pt"], st["delz"], st["phis"])
        with pytest.raises(RuntimeError, match="total_energy_before"):
            fv.step(4.0, last_cycle_is_last_step=True)
        fv.dc.set_state(st["u"], st["v"], st["w"], st["delp"], st["pt"], st["delz"], st["phis"])
        fv.total_energy_before()
        fv.step(4.0, last_cycle_is_last_step=True)          # consumes te0_2d
        with pytest.raises(RuntimeError, match="total_energy_before"):
            fv.step(4.0, last_cycle_is_last_step=True)      # ... which is stale now
    finally:
        ctx.close()


def test_ordered_sum_is_exact_and_order_independent(emu):
    """fv3_ordered_sum (g_sum with reproduce = .true.: the extended-fixed-point sum) against math.fsum and the host's own
    implementation (global_sum.py), on addends spread over 23 orders of magnitude, permuted and split"""
    import math
    from gfdl_atmos_cubed_sphere_amd.global_sum import reproducing_sum
    from gfdl_atmos_cubed_sphere_amd.layout import Bounds
    from gfdl_atmos_cubed_sphere_amd.lib import Context
    ctx = Context(P.make_grid(Bounds(1, 8, 1, 8), False), 5, lib=emu)
    try:
        rng = np.random.default_rng(1)
        a = rng.normal(0, 1e9, 200000) * rng.choice([1e-14, 1.0, 1e9], 200000)
        s = ctx.ordered_sum(a)
        assert abs(s - math.fsum(a)) <= abs(s) * 2.3e-16
        p_ = rng.permutation(a)
        assert ctx.ordered_sum(p_) == s == reproducing_sum([p_[:777], p_[777:90000], p_[90000:]])
        # the range of the extended fixed point format: both implementations refuse what FMS aborts on (|a| >= 2**138), and a
        # leading digit that would not survive the int64 all-reduce
        for bad in (np.array([1.0, 2.0 ** 138]), np.full(3000, 2.0 ** 131)):
            with pytest.raises(Exception):
                ctx.ordered_sum(bad)
            with pytest.raises(OverflowError):
                reproducing_sum([bad])
        assert ctx.ordered_sum(np.array([2.0 ** 130, 1.0, -2.0 ** 130])) == 1.0 == reproducing_sum([np.array([2.0 ** 130, 1.0, -2.0 ** 130])])
    finally:
        ctx.close()


def test_cubed_sphere_total_energy_conservation(emu):
    """the same on the six faces (hydrostatic JW): global sums over the sphere"""
    assert max(PC.check_jw_consv(emu, npx=13).values()) <= 1e-12


def test_cubed_adv_pe(emu):
    """the advective term of the omega diagnostic on the six faces (adv_pe, dyn_core.F90:1195, :1529-1632)"""
    assert PC.check_adv_pe(emu, npx=13) <= 1e-14


def test_config4_supercell_initial_condition(emu):
    """BASELINE configs[3]'s initial condition (doubly periodic supercell, test_case = 17: Weisman-Klemp sounding, sheared wind, warm
    bubble, vapour) through a whole nonhydrostatic fv_dynamics call against the oracle loop; air mass to rounding, the bubble rises"""
    assert max(D.check_supercell_step(emu, nx=24, ny=16, npz=12, n_split=2, bdt=6.0).values()) <= 1e-12


def test_cubed_del2_cubed_and_damped_transports(emu):
    for nmax in (1, 2, 3):
        assert PC.check_del2_cubed(emu, nmax=nmax) <= P.TOL
    for kw in (dict(nord=0, damp_c=0.05), dict(nord=2, damp_c=0.05), dict(nord=2, damp_c=0.05, mass_flux=True)):
        assert PC.check_fv_tp_2d(emu, 8, faces=(0, 2, 5), **kw) <= P.TOL
    for kw in (dict(nord_tr=1, trdm=0.1), dict(nord_tr=2, trdm=0.1, courant_scale=40.0, hord=5, nq=2)):
        assert PC.check_tracer_2d(emu, **kw)["q"] <= P.TOL


def test_cubed_sphere_substeps_with_production_flags(emu):
    """nord = 3, do_vort_damp (vtdm4 = 0.06), d_con = 1, dddmp = 0.5: whole substep loops on the six faces incl. the heating of pt
    after them (del2_cubed with the corner means) and update_dz_d's del6 damping of the interface heights"""
    assert max(PC.check_substeps_hydrostatic(emu, npx=13, npz=12, n_split=2, flags=PROD).values()) <= 1e-13
    assert max(PC.check_substeps_nh(emu, npx=13, npz=12, n_split=2, flags=PROD).values()) <= 1e-13
    r = PC.check_jw_step(emu, npx=13, npz=20, k_split=2, n_split=2, bdt=900.0, hydrostatic=False, nq=2, flags=PROD)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


def test_cubed_sphere_hydrostatic_external_mode_damping(emu):
    """d_ext = 0.02 (the reference's default): a2b_ord2 of delp with its edge weights and corner means, the column-weighted
    divergence, one_grad_p with it -- hydrostatic substeps on the six faces, pass kernels (C12) and hybrid (C32)"""
    assert max(PC.check_substeps_hydrostatic(emu, npx=13, npz=8, n_split=2, flags=dict(d_ext=0.02)).values()) <= 1e-13
    assert max(PC.check_substeps_hydrostatic(emu, npx=33, npz=12, n_split=2, flags=dict(d_ext=0.02)).values()) <= 1e-13


@pytest.mark.parametrize("hydrostatic", [True, False])
def test_cubed_d_sw_use_cond(emu, hydrostatic):
    """thermostruct%use_cond on a face: q_con transported with delp's mass fluxes (and pt's damping when it is on)"""
    assert max(PC.check_d_sw(emu, npx=13, npz=12, hydrostatic=hydrostatic, faces=(0, 4), use_cond=True).values()) <= P.TOL
    assert max(PC.check_d_sw(emu, npx=13, npz=12, hydrostatic=hydrostatic, faces=(2,), use_cond=True,
                             flags=dict(do_vort_damp=True, vtdm4=0.06, nord=2)).values()) <= P.TOL


@pytest.mark.parametrize("c2l_ord", [2, 4])
def test_cubed_to_latlon_on_the_sphere(emu, c2l_ord):
    """cubed_to_latlon on the six faces (the a11 .. a22 rotation of init_cubed_to_latlon, the two-point forms next to the face
    edges): device = oracle, and the result is the analytic (east, north) wind of the test state to discretisation error"""
    assert PC.check_c2l(emu, c2l_ord, npx=13) <= P.TOL


def test_cube_table_of_the_library_equals_the_oracle(emu):
    """fv3_cube_table (csrc/cube_topo.h: the topology the pack / unpack lists of the cube-edge messages are built from, derived from
    the cube's geometry) row for row against the oracle's tables (oracle/fv_grid.c: from the reference's 12 contacts)"""
    import numpy as np
    import grid_oracle as GO
    from gfdl_atmos_cubed_sphere_amd.lib import cube_table
    npx = 9
    ref = GO.ref_sphere(npx)
    for kind in ("A", "B", "D", "C", "Dedge"):
        rt = ref.table(kind)
        for t in range(6):
            for m in range(len(rt[t])):
                a, b = rt[t][m], cube_table(emu, npx, kind, m, t)
                oa, ob = np.argsort(a["dst"], kind="stable"), np.argsort(b["dst"], kind="stable")
                for k in ("dst", "tile", "comp", "src") + (("sign",) if kind in ("D", "C", "Dedge") else ()):
                    assert np.array_equal(a[k][oa], b[k][ob]), (kind, t, m, k)


def test_cube_edge_exchange_behind_the_c_abi(emu):
    """fv3_cube_halo_start / _complete with the six faces in one process (the host-emulation build copies the messages; on the GPU the
    same call routes every message through RCCL, tests/test_gpu_parity.py): every field kind, a group of several fields in one call,
    SCALAR_PAIR, mpp_get_boundary -- against the oracle's update of the six tiles"""
    import numpy as np
    from gfdl_atmos_cubed_sphere_amd.cubed_halo import CubeHaloNative
    from gfdl_atmos_cubed_sphere_amd.lib import Context
    npx, npz = 9, 3
    cs, gs = PC.CC.sphere(npx)
    ctxs = [Context(g, npz, lib=emu) for g in gs]
    try:
        H = CubeHaloNative(ctxs, range(6), [0] * 6)
        rng = np.random.default_rng(0)
        bd = gs[0].bd
        mk = lambda k, nk=npz: [np.asfortranarray(rng.uniform(-1, 1, bd.shape(k, nk))) for _ in range(6)]      # noqa: E731
        for kind, kinds, vector in (("A", ("A",), True), ("B", ("B",), True), ("D", ("U", "V"), True), ("C", ("V", "U"), True),
                                    ("C", ("V", "U"), False), ("Dedge", ("U", "V"), True)):
            host = [mk(k) for k in kinds]
            dev = [[ctxs[t].from_host(a[t]) for t in range(6)] for a in host]
            ref = [[x.copy(order="F") for x in a] for a in host]
            cs.topo.update(kind, ref[0] if len(kinds) == 1 else (ref[0], ref[1]), vector=vector)
            H.update(kind, dev[0] if len(kinds) == 1 else (dev[0], dev[1]), vector=vector)
            for m in range(len(kinds)):
                for t in range(6):
                    assert np.array_equal(dev[m][t].download(), ref[m][t]), (kind, vector, m, t)
        # a group: two A fields of different depth, a B field and a D pair in ONE start (one message per pair of faces)
        a1, a2, b1, u, v = mk("A"), mk("A", 1), mk("B"), mk("U"), mk("V")
        dev = {n: [ctxs[t].from_host(x[t]) for t in range(6)] for n, x in dict(a1=a1, a2=a2, b1=b1, u=u, v=v).items()}
        cs.topo.update("A", a1); cs.topo.update("A", a2); cs.topo.update("B", b1); cs.topo.update("D", (u, v))
        H.start([("A", dev["a1"]), ("A", dev["a2"]), ("B", dev["b1"]), ("D", (dev["u"], dev["v"]))])
        H.finish()
        for n, x in dict(a1=a1, a2=a2, b1=b1, u=u, v=v).items():
            for t in range(6):
                assert np.array_equal(dev[n][t].download(), x[t]), (n, t)
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("hydrostatic", [True, False])
def test_sphere_step_through_the_cube_edge_exchange_of_the_c_abi(emu, hydrostatic):
    """a whole fv_dynamics call on the six faces with EVERY halo update going through fv3_cube_halo_start / _complete (groups of
    fields in one message per pair of faces, delp + pt and zh + pkc kept in flight across kernels, mpp_get_boundary at the end) --
    the state of the device-gather run, i.e. the six-face oracle's"""
    r = PC.check_jw_step(emu, npx=13, npz=20, k_split=1, n_split=2, bdt=900.0, hydrostatic=hydrostatic, nq=2, native_halo=True)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12, r


def test_fortran_host_on_the_cubed_sphere(emu, tmp_path):
    """the Fortran host on grid_type = 0 (fortran/fv3_sphere_mod.F90 + fv3_solo_sphere.F90, built with amdflang): one
    context per face, fv3_grid_upload_cubed, every halo update of dyn_core / tracer_2d through the cube-edge exchange behind the C ABI,
    mpp_get_boundary and adv_pe after the last substep -- a C12 Jablonowski-Williamson fv_dynamics call bit-identical to the Python
    host's on every face, nonhydrostatic with tracers and hydrostatic with the dissipative heating"""
    import fortran_host as F
    if F.fortran_compiler() is None:
        pytest.skip("no amdflang in this environment")
    assert "fv3_solo_sphere: done" in F.check_fortran_sphere(emu, tmp_path, npx=13, npz=12, nq=2, hydrostatic=False)
    assert "fv3_solo_sphere: done" in F.check_fortran_sphere(emu, tmp_path, npx=13, npz=12, nq=0, hydrostatic=True, d_con=1.0, k_split=1)
    assert "fv3_solo_sphere: done" in F.check_fortran_sphere(emu, tmp_path, npx=13, npz=8, nq=0, hydrostatic=False, beta=0.4, n_split=3)
    assert "fv3_solo_sphere: done" in F.check_fortran_sphere(emu, tmp_path, npx=13, npz=8, nq=2, hydrostatic=False, inline_q=True)
    assert "fv3_solo_sphere: done" in F.check_fortran_sphere(emu, tmp_path, npx=13, npz=8, nq=1, hydrostatic=False, remap_te=True)


def test_switched_off_paths_still_agree(emu):
    """the forms the round-3 kernels replaced stay in the library behind switches that are read once per process: the column-kernel
    geopk (faces above FV3_MI355X_GEOPK_PHASED columns), the pass chains of the damping operators (FV3_MI355X_DELN_FUSED=0) and the
    LDS-tile transports of the damped levels (FV3_MI355X_FLUX_MARCH=0) against the oracle, in a process of their own"""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import parity_common as P, parity_nh as N, parity_cubed as PC
        from gfdl_atmos_cubed_sphere_amd.lib import Fv3Lib
        emu = Fv3Lib(%r)
        N.check_halos_and_geopk(emu)
        PROD = dict(do_vort_damp=True, vtdm4=0.06, nord=3, d_con=1.0, dddmp=0.5)
        for hyd in (True, False):
            assert max(PC.check_d_sw(emu, npx=33, npz=17, hydrostatic=hyd, faces=(1,), flags=PROD, par_over=dict(dddmp=0.5)).values()) <= P.TOL
        print("ok")
    """) % (os.path.dirname(HERE), HERE, os.path.join(HERE, "hostemu", "libfv3_hostemu.so"))
    env = dict(os.environ, FV3_MI355X_GEOPK_PHASED="0", FV3_MI355X_DELN_FUSED="0", FV3_MI355X_FLUX_MARCH="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("hydrostatic", [False, True])
def test_face_group(emu, hydrostatic):
    """fv3_group_create: the six faces of a sphere as one group (queued launches, one merged launch per kernel, stream operations in
    each member's order, flushes at gathers / downloads) against six separate launches per kernel -- bit for bit, and merged"""
    PC.check_face_group(emu, hydrostatic=hydrostatic)
    if not hydrostatic:
        PC.check_face_group(emu, npx=17, npz=6, n_split=3, flags=dict(do_vort_damp=True, vtdm4=0.06, nord=3, d_con=1.0))


@pytest.mark.parametrize("dims", [dict(), dict(nx=37, ny=13, km=32), dict(nx=20, ny=5, km=79), dict(nx=18, ny=3, km=127), dict(km=5),
                                  dict(km=16), dict(km=2)])
def test_riem_lds_bit_identical_to_the_slab_kernels(emu, dims):
    """RiemFast<CG, true> (the default of the dry SIM1 solvers): the same bits as the slab kernels in every output"""
    N.check_riem_lds_bits(emu, **dims)


@pytest.mark.parametrize("kw", [dict(), dict(hydrostatic=True), dict(consv_te=-2.0, tau=0.0, nq=0), dict(face_rank=(0, 1, 2, 3, 4, 5)),
                                dict(face_rank=(0, 0, 1, 1, 2, 2)), dict(face_rank=(0, 1, 0, 1, 0, 1), hydrostatic=True),
                                dict(have_grid=True), dict(what="dyn_core"), dict(what="dyn_core", hydrostatic=True),
                                dict(what="dyn_core", face_rank=(0, 0, 1, 1, 2, 2)),
                                dict(thermo=True), dict(thermo=True, what="dyn_core"), dict(thermo=True, face_rank=(0, 0, 1, 1, 2, 2)),   # use_cond = moist_kappa = .true.
                                dict(do_diss_est=True), dict(do_diss_est=True, what="dyn_core", hydrostatic=True),      # flagstruct%do_diss_est: diss_est in and out
                                dict(fill_dp=True, what="dyn_core"), dict(fill_dp=True, what="dyn_core", hydrostatic=True),   # flagstruct%fill_dp
                                dict(beta=-1.0), dict(beta=-1.0, what="dyn_core")])                                           # one_grad_p (beta < -0.1)
def test_fortran_fv_dynamics_with_the_reference_argument_list_on_the_sphere(emu, tmp_path, kw):
    """VERDICT r3 item 6 (row a21): fv_dynamics with the REFERENCE'S argument list (model/fv_dynamics.F90:79-85) on grid_type = 0 --
    fv3_dyn_core_mod.F90 binds one context per tile held (fv3_grid_upload_cubed from gridstruct's own members, corner factors from
    grid / agrid with have_grid), exchanges through fv3_cube_halo_* with domain -> face_rank, and carries compute_total_energy + the
    energy fixer (consv_te > 0 and the prescribed flux < 0), Rayleigh_Super (tau = 10 days) and the virtual effect in Fortran: a C12
    Jablonowski-Williamson call bit-identical to FvDynamics.step_from_temperature on every tile -- six tiles in one process, and
    6 x 1 / 3 x 2 / 2 x 3 tiles over PROCESSES (the exchange between them; here the harness' file transport in the place of RCCL).
    what = "dyn_core": one dyn_core call with ITS reference argument list (dyn_core.F90:94-98) on the tiles, against DynCore.run"""
    import fortran_host as F
    if F.fortran_compiler() is None:
        pytest.skip("no amdflang in this environment")
    assert F.check_refsig_sphere(emu, tmp_path, npx=13, npz=12, n_split=2, k_split=2, bdt=900.0, **kw) == 0.0


@pytest.mark.parametrize("kw", [dict(), dict(hydrostatic=True, face_rank=(0, 0, 1, 1, 2, 2))])
def test_fortran_fv_dynamics_consv_am_on_the_sphere(emu, tmp_path, kw):
    """flagstruct%consv_am through the reference-signature fv_dynamics on the cubed sphere (fv_dynamics.F90:358-361, :747-800): compute_aam
    of every tile before and after the k_split loop, the two reproducing sums over the tiles (and the processes), u00, the wind correction
    -- against FvDynamics.step_from_temperature; the wrapper takes cos(lat) of gridstruct%agrid with the Fortran run-time's cos(), the
    Python host with numpy's, and u00 carries that last-bit difference into every wind: 1e-11, as on the doubly periodic domain"""
    import fortran_host as F
    if F.fortran_compiler() is None:
        pytest.skip("no Fortran compiler in this image")
    if False:
        kw = dict(kw, face_rank=(0, 0, 0, 0, 0, 0))     # one GPU here: the tiles of one process
    worst = F.check_refsig_sphere(emu, tmp_path, npx=13, npz=12, n_split=2, k_split=2, bdt=900.0, nq=0, consv_am=True, have_grid=True, tol=1e-11, **kw)
    assert worst <= 1e-11


@pytest.mark.parametrize("kw", [dict(), dict(nx=33, ny=9, km=20), dict(nx=33, ny=9, km=79), dict(nx=17, ny=5, km=127), dict(km=3), dict(km=8),
                                dict(km=16), dict(km=40, lev_over=dict(do_vort_damp=True, vtdm4=0.06, nord=2))])
def test_edge_profile_lds_bit_identical_to_the_slab_kernel(emu, kw):
    """EdgeProfileLds (the default of update_dz_d's edge_profile, nh_utils.F90:1590-1696): the same bits as the slab kernel"""
    N.check_edge_profile_lds_bits(emu, **kw)


@pytest.mark.parametrize("which,kw", [("dyn_core", dict(layout=(2, 1))), ("dyn_core", dict(layout=(2, 2), hydrostatic=True, d_con=1.0)),
                                      ("fv_dynamics", dict(layout=(2, 2))), ("fv_dynamics", dict(layout=(1, 2), hydrostatic=True))])
def test_fortran_reference_argument_lists_on_several_ranks_of_the_periodic_domain(emu, tmp_path, which, kw):
    """dyn_core / fv_dynamics with the reference's argument lists on 2 and 4 PROCESSES of a doubly periodic layout (domain%layout, %pe,
    %npes, %comm_id -> fv3_host_comm_layout: the group halo updates through fv3_halo_start / _complete with the neighbour PEs,
    tracer_2d's mp_reduce_max through fv3_allreduce_max): every block bit-identical to the single-domain Python host"""
    import fortran_host as F
    if F.fortran_compiler() is None:
        pytest.skip("no amdflang in this environment")
    (F.check_fortran_refsig if which == "dyn_core" else F.check_fortran_fv_dynamics)(emu, tmp_path, **kw)


@pytest.mark.parametrize("dims", [dict(), dict(nx=37, ny=13, km=32), dict(nx=9, ny=5, km=127), dict(km=3)])
def test_riem_solvers_sim3_sim3p0_rim_2d(emu, dims):
    """the other vertical solvers Riem_Solver3 / Riem_Solver_c dispatch on a_imp (nh_core.F90:169-177, nh_utils.F90:449-459):
    SIM3p0_solver (a_imp < -0.999; C grid < -0.01, nh_utils.F90:1134-1274), SIM3_solver (a_imp < -0.5, :984-1132), RIM_2D (a_imp <= 0.5,
    :751-982) with one, four (the one-step branch of the layers the sound wave does not cross) and ten sub-steps -- against the oracle"""
    for a_imp, ms in ((-1.0, 1), (-0.75, 1), (0.3, 1), (0.3, 4), (0.0, 10), (-0.3, 3)):
        assert N.check_riem_solver3(emu, a_imp=a_imp, m_split=ms, use_logp=True, last_call=True, fp_out=True, **dims) <= 1e-13
        assert N.check_riem_solver3(emu, a_imp=a_imp, m_split=ms, last_call=False, **dims) <= 1e-13
        assert N.check_riem_solver_c(emu, a_imp=a_imp, m_split=ms, **dims) <= 1e-13


@pytest.mark.parametrize("kw", [dict(consv_te=1.0), dict(consv_te=1.0, tau=10.0, npz=16), dict(consv_te=-2.0, hydrostatic=True),
                                dict(consv_te=1.0, tau=10.0, npz=16, layout=(2, 2)), dict(tau=10.0, npz=16, hydrostatic=True, layout=(2, 1))])
def test_fortran_fv_dynamics_reference_argument_list_with_the_energy_fixer_and_rayleigh_friction(emu, tmp_path, kw):
    """fv_dynamics with the reference's argument list on the doubly periodic domain with consv_te (compute_total_energy, the energy fixer
    of the last remap with the reproducing sum over the ranks, the prescribed flux) and tau > 0 (Rayleigh_Friction: u2f, its halo update,
    the damping) carried in Fortran (fv3_host_mod fv3_fv_dynamics_call), one rank and 2 / 4 processes: bit-identical to
    FvDynamics.step_from_temperature"""
    import fortran_host as F
    if F.fortran_compiler() is None:
        pytest.skip("no amdflang in this environment")
    F.check_fortran_fv_dynamics(emu, tmp_path, **kw)


@pytest.mark.parametrize("hydrostatic", [False, True])
@pytest.mark.parametrize("flags", [None, dict(prevent_diss_cooling=False)])
def test_sponge_levels_run_on_the_marching_kernels(emu, hydrostatic, flags, monkeypatch):
    """levels 1, 2 of the default coefficients (del-2 damping of the divergence and of w, the heating of the latter) inside the branch-free
    marching kernels on a uniform grid: the oracle's values, and no LDS-tile launch left"""
    worst, rep = P.check_sponge_levels_march(emu, hydrostatic=hydrostatic, flags=flags)
    assert not ({"d_sw_transport", "d_sw_momentum", "d_sw_courant"} & set(rep)), rep
    # ... and the switch back to the tile kernels gives the same parity
    monkeypatch.setenv("FV3_MI355X_SPONGE_MARCH", "0")
    worst0, rep0 = P.check_sponge_levels_march(emu, hydrostatic=hydrostatic, flags=flags)
    assert "d_sw_transport" in rep0 and "d_sw_momentum" in rep0, rep0


def test_sponge_levels_march_smagorinsky_term(emu):
    """dddmp > 0 keeps the nord = 1 levels off the marching momentum kernel; the sponge form carries the term (sw_core.F90:1367) -- checked
    through the transport half, which still marches its sponge levels"""
    P.check_d_sw(emu, nx=70, ny=30, npz=4, perturb=False, par_over=dict(dddmp=0.2))


def test_mixed_segmentation_of_the_marching_launches(emu, monkeypatch):
    """balance_segments (tp2d_march.h): the first levels of a launch cut into one segment less than the others, so that the launch fills
    whole rounds of the chip.  FV3_MI355X_ROUND_SIMDS=35 makes that happen at test size in c_sw, the fused transport and the fused momentum
    kernel (70 x 60 x 9: the first 3 level slots in 7 segments, the others in 8); the oracle's values either way"""
    monkeypatch.setenv("FV3_MI355X_ROUND_SIMDS", "35")
    P.check_c_sw(emu, nx=70, ny=60, npz=9, perturb=False)
    P.check_d_sw(emu, nx=70, ny=60, npz=9, perturb=False)
    P.check_d_sw(emu, nx=70, ny=60, npz=9, perturb=False, hydrostatic=True)


@pytest.mark.parametrize("direction", ["x", "y"])
@pytest.mark.parametrize("iord", [5, -5, 6, 8])
def test_golden_ppm_lines_through_fv_tp_2d(emu, iord, direction):
    """the reference-held PPM vectors (tests/golden/, from the reference's own tp_core.ipynb) straight through the library's fv_tp_2d"""
    P.check_golden_ppm_through_fv_tp_2d(emu, iord, direction)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("iord", [5, -5, 6, 8, 10])
def test_golden_ppm_lines_through_the_1d_operators(emu, iord, which):
    """all 144 reference-held PPM vectors (hord 10 among them) through the kernel sources' three 1-D operators (fv3_ppm_line)"""
    P.check_golden_ppm_lines(emu, iord, which)
