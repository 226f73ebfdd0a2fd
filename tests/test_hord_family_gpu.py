"""The transport-scheme table on the GPU: every order of the reference through the product library against the oracle -- the cases of
tests/test_hord_family_hostemu.py, no fallback."""
import pytest

import parity_cubed as C
import parity_dyn as D
import parity_hord as H
import parity_nh as N
import parity_tracer as T

from gfdl_atmos_cubed_sphere_amd import lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prod():
    return L.load()


def lim_of(hord):
    return 2.0 if abs(hord) == 1 else 1.0


@pytest.mark.parametrize("hord", H.NEW_SCALAR)
def test_fv_tp_2d_plain(prod, hord):
    H.check_fv_tp_2d(prod, hord, lim_of(hord))


@pytest.mark.parametrize("hord", H.NEW_SCALAR)
def test_fv_tp_2d_mass_fluxes_and_damping(prod, hord):
    H.check_fv_tp_2d(prod, hord, lim_of(hord), mode="mass_flux")
    H.check_fv_tp_2d(prod, hord, lim_of(hord), mode="mass_flux_damp", nord=2, damp_c=0.06)


@pytest.mark.parametrize("hord", H.NEW_SCALAR)
def test_fv_tp_2d_several_tiles(prod, hord):
    """a larger, ragged shape: doubly periodic fv_tp_2d is the LDS-tile kernel at every size (the marching operators of the new orders are
    reached through d_sw, update_dz_d and the tracers below)"""
    H.check_fv_tp_2d(prod, hord, lim_of(hord), nx=130, ny=100, nk=2)


@pytest.mark.parametrize("hord", H.NEW_SCALAR)
def test_fv_tp_2d_six_faces(prod, hord):
    """C12: the pass kernels over the whole face; C40: the size at which d_sw and the tracers run the hybrid"""
    H.check_fv_tp_2d_cubed(prod, hord, lim_of(hord))
    H.check_fv_tp_2d_cubed(prod, hord, lim_of(hord), mass_flux=True, faces=(1, 4))
    H.check_fv_tp_2d_cubed(prod, hord, lim_of(hord), npx=41, nk=2, faces=(0, 3))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_golden_hord1_lines_through_the_1d_operators(prod, which):
    """the reference notebook's own hord 1 face values, lim_fac 1, 2, 3 (tests/golden/ppm1d_lin_golden.npz), no oracle in between"""
    assert H.check_golden_lin_lines(prod, which) < 5e-15


@pytest.mark.parametrize("direction", ["x", "y"])
def test_golden_hord1_lines_through_fv_tp_2d(prod, direction):
    assert H.check_golden_lin_through_fv_tp_2d(prod, direction) < 5e-15


@pytest.mark.parametrize("hydrostatic", [False, True])
@pytest.mark.parametrize("s,lim", H.DSW_SETS, ids=H.DSW_IDS)
def test_d_sw_multi_strip(prod, s, lim, hydrostatic):
    """several 58-column strips and row segments: the per-field marching kernels take every order of the table"""
    H.check_d_sw(prod, s, lim, nx=130, ny=100, npz=3, hydrostatic=hydrostatic)


@pytest.mark.parametrize("s,lim", H.DSW_SETS, ids=H.DSW_IDS)
def test_d_sw_uniform_metrics(prod, s, lim):
    H.check_d_sw(prod, s, lim, nx=70, ny=30, npz=2, perturb=False)


@pytest.mark.parametrize("mt", [1, 2, 3, 4])
def test_d_sw_linear_wind_orders_beside_the_fused_scalar_orders(prod, mt):
    """hord_mt 1 .. 4 with (10, 10, 10): the fused transport kernel beside the unfused momentum kernels"""
    H.check_d_sw(prod, (mt, 10, 10, 10), 2.0, nx=130, ny=64, npz=3)
    H.check_d_sw(prod, (mt, 10, 10, 10), 2.0, nx=130, ny=64, npz=3, perturb=False, hydrostatic=True)


def test_d_sw_use_cond_and_damped_levels(prod):
    H.check_d_sw(prod, (2, -2, 2, -2), use_cond=True)
    H.check_d_sw(prod, (6, 6, 6, -6), nx=70, ny=40, use_cond=True)
    # the damped levels (nord = 2, vorticity damping, d_con heating): they stay on the tile kernels, beside or without the marching ones
    lev = dict(nord=2, do_vort_damp=True, vtdm4=0.06, d_con=1.0, d2_bg=0.0075)
    for s, lim in (((6, -6, 6, -6), 1.0), ((1, 1, 1, -1), 2.0), ((3, -3, 3, -3), 1.0), ((10, 9, 12, 7), 1.0)):
        H.check_d_sw(prod, s, lim, lev_over=lev)
        H.check_d_sw(prod, s, lim, nx=130, ny=64, npz=4, lev_over=dict(lev, nord=1))


def test_d_sw_interior_then_rest_with_an_all_equal_new_order(prod):
    """(2, 2, 2, 2) and (-6, -6, -6) pass the all-equal test of the fused predicate: they must take the per-field kernels, and the
    interior phase must not read halos in flight"""
    H.check_d_sw(prod, (2, 2, 2, 2), nx=200, ny=100, npz=2, phases="poison")
    H.check_d_sw(prod, (6, -6, -6, -6), nx=200, ny=100, npz=2, phases="poison")
    H.check_d_sw(prod, (6, 12, 12, 12), nx=200, ny=100, npz=2, phases=True)


@pytest.mark.parametrize("s,lim", H.DSW_SETS, ids=H.DSW_IDS)
def test_d_sw_six_faces(prod, s, lim):
    H.check_d_sw_cubed(prod, s, lim, hydrostatic=False)
    H.check_d_sw_cubed(prod, s, lim, hydrostatic=True, faces=(0, 2, 5))


@pytest.mark.parametrize("s,lim", H.DSW_SETS, ids=H.DSW_IDS)
def test_d_sw_six_faces_c40(prod, s, lim):
    """the size of the hybrid: an order the fused kernels are not built for sends the whole face through the pass kernels"""
    H.check_d_sw_cubed(prod, s, lim, npx=41, npz=2, hydrostatic=False, faces=(0, 4))
    H.check_d_sw_cubed(prod, s, lim, npx=41, npz=2, hydrostatic=True, faces=(2,))


@pytest.mark.parametrize("mt", [1, 2, 3, 4])
def test_d_sw_six_faces_linear_wind_orders(prod, mt):
    H.check_d_sw_cubed(prod, (mt, 10, 10, 10), 2.0, hydrostatic=False)
    H.check_d_sw_cubed(prod, (mt, 8, 8, 8), 2.0, npx=41, npz=2, hydrostatic=True, faces=(1, 3))


@pytest.mark.parametrize("hord", [-6, 2, 3, 12])
def test_update_dz_d(prod, hord):
    N.check_update_dz_d(prod, hord=hord)
    N.check_update_dz_d(prod, nx=130, ny=100, km=3, hord=hord)
    # heights that straddle zero: -6 differs from 6 (asserted on the oracle)
    H.check_update_dz_d_signed(prod, hord)
    H.check_update_dz_d_signed(prod, hord, nx=130, ny=100, km=3)


@pytest.mark.parametrize("hord_tm", [-6, 3, 1])
def test_update_dz_d_in_the_cubed_hybrid(prod, hord_tm):
    """C32 faces, the size of the hybrid: ZhMarch<hord_tm> over the interior with the frame passes along the edges, in nonhydrostatic
    substeps (d_sw itself takes the pass kernels over the whole face for an order outside the fused kernels' set)"""
    fl = dict(hord_mt=6, hord_vt=6, hord_tm=hord_tm, hord_dp=6)
    assert max(C.check_substeps_nh(prod, npx=33, npz=6, n_split=2, flags=fl).values()) <= 1e-12


@pytest.mark.parametrize("hord", [2, -3, -6])
def test_tracer_2d(prod, hord):
    T.check_tracer_2d(prod, hord=hord)
    T.check_tracer_2d(prod, nx=130, ny=100, npz=3, nq=2, hord=hord)
    T.check_tracer_2d(prod, nx=70, ny=60, npz=3, nq=2, big_courant=True, hord=hord)
    T.check_tracer_2d(prod, q_split=2, trdm=0.06, nord_tr=1, hord=hord)
    C.check_tracer_2d(prod, hord=hord)
    C.check_tracer_2d(prod, npx=41, npz=2, nq=2, hord=hord)
    # tracers with zeros: a negative order differs from its positive twin (asserted on the oracle, for these inputs)
    H.check_tracer_2d_zeros(prod, hord)
    H.check_tracer_2d_zeros(prod, hord, nx=130, ny=100, npz=3, nq=2)
    H.check_tracer_2d_zeros(prod, hord, nx=70, ny=60, npz=3, nq=2, big_courant=True)
    H.check_tracer_2d_cubed_zeros(prod, hord)
    H.check_tracer_2d_cubed_zeros(prod, hord, npx=41, npz=2, nq=2)


@pytest.mark.parametrize("hord_tr", [2, -3, -6])
def test_inline_q(prod, hord_tr):
    D.check_fv_step(prod, n_split=3, flags=dict(inline_q=True, hord_tr=hord_tr))
    H.check_fv_step_signed_tracers(prod, dict(inline_q=True, hord_tr=hord_tr), n_split=3)     # tracers of both signs: -n bites (asserted)
    r = C.check_jw_step(prod, npx=13, npz=12, k_split=1, n_split=2, bdt=900.0, hydrostatic=False, nq=2, flags=dict(inline_q=True, hord_tr=hord_tr))
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


@pytest.mark.parametrize("fl", [dict(hord_mt=6, hord_vt=6, hord_tm=6, hord_dp=-6, hord_tr=8), dict(hord_mt=2, hord_vt=2, hord_tm=2, hord_dp=2, hord_tr=-2)],
                         ids=["6_6_6_-6_tr8", "2_2_2_2_tr-2"])
def test_whole_steps(prod, fl):
    """whole substeps through DynCore and a whole step through FvDynamics, doubly periodic and on the C12 sphere, at the whole-step bound"""
    D.check_substeps(prod, flags=fl)
    D.check_fv_step(prod, flags=fl)
    H.check_fv_step_signed_tracers(prod, fl)
    assert max(C.check_substeps_nh(prod, flags=fl).values()) <= 1e-12
    r = C.check_jw_step(prod, npx=13, npz=12, k_split=1, n_split=2, bdt=900.0, hydrostatic=False, nq=2, flags=fl)
    assert r.pop("finite") == 1.0 and max(r.values()) <= 1e-12


def test_fv_tp_2d_refuses_aliased_outputs(prod):
    H.check_fv_tp_2d_refuses_aliased_outputs(prod)


def test_refusals(prod):
    msg = H.check_refusals(prod)
    assert "1 .. 13" in msg and "-1 .. -6" in msg and "1 .. 11" in msg


def test_fv_tp_2d_and_d_sw_on_the_tile_kernels(prod, monkeypatch):
    """FV3_MI355X_MARCH=0: the one-face operators of the LDS-tile kernels (ppm.h) take the order at run time"""
    monkeypatch.setenv("FV3_MI355X_MARCH", "0")
    for hord in H.NEW_SCALAR:
        H.check_fv_tp_2d(prod, hord, lim_of(hord))
    for s, lim in H.DSW_SETS:
        H.check_d_sw(prod, s, lim)
        H.check_d_sw(prod, s, lim, hydrostatic=True, nx=70, ny=30, npz=2)
    for mt in (1, 2, 3, 4):
        H.check_d_sw(prod, (mt, 10, 10, 10), 2.0)
    for hord in (-6, 2, 3, 12):
        N.check_update_dz_d(prod, hord=hord)
    for hord in (2, -3, -6):
        T.check_tracer_2d(prod, hord=hord)
