"""fv_subgrid_z on the MI355X: the check bodies of tests/parity_subgrid.py (see tests/test_subgrid_hostemu.py) on the product library."""
import pytest

import parity_common as P
import parity_subgrid as S
import subgrid_inputs as SI

from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu


def test_library_against_the_compiled_reference(lib):
    """every recorded case, with nothing in between; the figures and which fields are bit-identical are printed before the assertion"""
    rows = {name: S.check_lib_against_golden(lib, name) for name in SI.SG_CASES}
    for name, (worst, bits) in rows.items():
        print(f"{name}: worst rel-rms {worst:.3e}, bit-identical: {bits}")
    assert max(w for w, _ in rows.values()) <= P.TOL


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", S.SHAPES, ids=["40x19x12", "130x100x5", "21x7x2", "21x7x3"])
def test_library_against_the_restatement(lib, shape, hydrostatic):
    for nwat, nq in S.NWATS:
        assert S.check_against_checker(lib, shape, hydrostatic, nwat, nq) <= P.TOL


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("kw", [dict(k_bot_full=5), dict(k_bot_full=5, weak=900), dict(k_bot_full=7, nqa=9)], ids=["kbot5", "weak900", "nq_below_array"])
def test_library_kbot_and_weak_relaxation(lib, kw, hydrostatic):
    assert S.check_against_checker(lib, (40, 19, 12), hydrostatic, 6, 7, **kw) <= P.TOL


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", S.SHAPES[:2], ids=["40x19x12", "130x100x5"])
def test_properties(lib, shape, hydrostatic):
    S.check_properties(lib, shape, hydrostatic)


@pytest.mark.parametrize("name", list(SI.DW_CASES))
def test_update_dwinds_phys_against_the_compiled_reference(lib, name):
    worst, bits = S.check_dwinds_lib_against_golden(lib, name)
    print(f"{name}: worst rel-rms {worst:.3e}, bit-identical: {bits}")
    assert worst <= P.TOL


def test_update_dwinds_phys_on_the_tile(lib):
    for shape in ((40, 19, 3), (130, 100, 2)):
        assert S.check_dwinds_tile(lib, shape) <= P.TOL


def test_refusals(lib):
    S.check_refusals(lib)


def test_update_dwinds_phys_on_six_faces(lib):
    assert S.check_dwinds_sphere(lib) <= P.TOL


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
def test_six_faces_in_one_launch(lib, hydrostatic):
    S.check_six_faces(lib, hydrostatic=hydrostatic)


@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_atmosphere_step(lib, where):
    assert S.check_atmosphere_step(lib, where) <= P.TOL

