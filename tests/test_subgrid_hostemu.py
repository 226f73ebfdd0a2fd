"""fv_subgrid_z on the CPU: the numpy restatement tests/ref_fv_sg.py against the outputs of the reference's compiled Fortran
(tests/golden/subgrid_*.npz), and fv3_fv_subgrid_z / fv3_update_dwinds_phys of the host-emulation library (tests/hostemu) against
those outputs, against the restatement at larger shapes, and in their properties.  The same check bodies run on the product library
in tests/test_subgrid_gpu.py."""

import pytest

import parity_common as P
import parity_subgrid as S
import subgrid_inputs as SI

from parity_phys import emu  # noqa: F401


@pytest.mark.parametrize("name", list(SI.SG_CASES))
def test_restatement_is_the_compiled_reference(name):
    """no library: bit for bit, and the recorded cases run every branch the checks rely on"""
    S.check_checker_against_golden(name)


@pytest.mark.parametrize("name", list(SI.SG_CASES))
def test_library_against_the_compiled_reference(emu, name):
    worst, bits = S.check_lib_against_golden(emu, name)
    print(name, worst, bits)
    assert worst <= P.TOL


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("nwat,nq", S.NWATS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=["40x19x12", "130x100x5", "21x7x2", "21x7x3"])
def test_library_against_the_restatement(emu, shape, nwat, nq, hydrostatic):
    assert S.check_against_checker(emu, shape, hydrostatic, nwat, nq) <= P.TOL


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("kw", [dict(k_bot_full=5), dict(k_bot_full=5, weak=900), dict(k_bot_full=7, nqa=9)], ids=["kbot5", "weak900", "nq_below_array"])
def test_library_kbot_and_weak_relaxation(emu, kw, hydrostatic):
    assert S.check_against_checker(emu, (40, 19, 12), hydrostatic, 6, 7, **kw) <= P.TOL


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", S.SHAPES[:2], ids=["40x19x12", "130x100x5"])
def test_properties(emu, shape, hydrostatic):
    S.check_properties(emu, shape, hydrostatic)


@pytest.mark.parametrize("name", list(SI.DW_CASES))
def test_dwinds_restatement_is_the_compiled_reference(name):
    S.check_dwinds_checker_against_golden(name)


@pytest.mark.parametrize("name", list(SI.DW_CASES))
def test_update_dwinds_phys_against_the_compiled_reference(emu, name):
    worst, bits = S.check_dwinds_lib_against_golden(emu, name)
    print(name, worst, bits)
    assert worst <= P.TOL


def test_update_dwinds_phys_on_the_tile(emu):
    for shape in ((40, 19, 3), (130, 100, 2)):
        assert S.check_dwinds_tile(emu, shape) <= P.TOL


def test_refusals(emu):
    S.check_refusals(emu)


def test_geometry_against_the_grid_oracle():
    """vlon, vlat, es, ew, edge_vect_* of cubed_sphere.py against oracle/fv_grid.c at the tolerance of tests/test_grid_oracle.py"""
    import test_grid_oracle as TG
    S.check_geometry_against_oracle(13, TG.TOL)


def test_update_dwinds_phys_on_six_faces(emu):
    assert S.check_dwinds_sphere(emu) <= P.TOL


def test_solid_body_rotation_converges_at_second_order():
    """independent of the restatement's source: the tendency of a solid-body rotation in (east, north) components must come out as
    that wind's components along the cell edges, to the accuracy of the two-point average -- second order: a quarter of the error
    at twice the resolution in the limit; 3.5 allows for C12 not being in the limit.  Measured: 2.63e-3 at C12, 6.61e-4 at C24
    (of the wind's strength), ratio 3.98."""
    e12, e24 = S.solid_body_error(13), S.solid_body_error(25)
    print(f"solid-body rotation: relative error {e12:.3e} at C12, {e24:.3e} at C24, ratio {e12 / e24:.2f}")
    assert e12 < 1.0e-2 and e12 / e24 >= 3.5


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
def test_six_faces_in_one_launch(emu, hydrostatic):
    S.check_six_faces(emu, hydrostatic=hydrostatic)


@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_atmosphere_step(emu, where):
    assert S.check_atmosphere_step(emu, where) <= P.TOL

