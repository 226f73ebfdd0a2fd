"""fv_update_phys on the MI355X: the check bodies of tests/parity_update_phys.py (see tests/test_update_phys_hostemu.py) on the product
library, the same cases and the same bounds."""
import pytest

import parity_common as P
import parity_update_phys as S
import update_phys_inputs as UI

from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu

IDS = ["21x7x1", "21x7x2", "40x19x12", "130x100x5"]
MODES = [(True, True), (False, True), (False, False)]      # (hydrostatic, phys_hydrostatic)
MODE_IDS = ["hydro", "nh_phys_hydro", "nh"]


def test_library_against_the_compiled_reference(lib):
    """every recorded case, with nothing in between; the figures and which fields are bit-identical are printed before the assertion"""
    rows = {name: S.check_lib_against_golden(lib, name) for name in UI.CASES}
    assert max(w for w, _, _ in rows.values()) <= P.TOL
    for name, (_, bits, _) in rows.items():
        assert all(bits[n] for n in bits if n not in S.BOUND), (name, bits)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_library_against_the_restatement(lib, shape, mode):
    for nwat in S.NWATS:
        assert S.check_against_checker(lib, shape, mode[0], mode[1], nwat) <= P.TOL


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_library_options_against_the_restatement(lib, shape, mode):
    for kw in (dict(has_qdt=False), dict(gfs_phys=True), dict(has_qdt=False, gfs_phys=True), dict(tau_h2o=2.0), dict(tau_h2o=-1.0)):
        for nwat in (0, 2, 6):
            assert S.check_against_checker(lib, shape, mode[0], mode[1], nwat, **kw) <= P.TOL


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", S.SHAPES[2:], ids=IDS[2:])
def test_zero_tendencies_keep_the_bits(lib, shape, mode):
    S.check_zero_tendencies(lib, shape, mode[0], mode[1])


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
def test_dry_mass_is_conserved(lib, hydrostatic):
    for nwat in (1, 3, 6):
        S.check_dry_mass(lib, (40, 19, 12), hydrostatic, nwat)


def test_refusals(lib):
    S.check_refusals(lib)


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
def test_six_faces_in_one_launch(lib, hydrostatic):
    S.check_six_faces(lib, hydrostatic=hydrostatic)


@pytest.mark.parametrize("gfs_phys", [False, True], ids=["winds", "gfs_phys"])
@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fv_dynamics_fv_update_phys(lib, where, gfs_phys):
    assert S.check_host(lib, where, gfs_phys) <= P.TOL
