"""The Kessler warm-rain microphysics on the MI355X: the check bodies of tests/parity_kessler.py (see tests/test_kessler_hostemu.py) on
the product library, the same cases and the same bounds."""
import pytest

import kessler_inputs as KI
import parity_kessler as S

from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu

FLAGS = list(KI.FLAGS)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("km", [1, 2, 12, 32])
def test_library_against_the_compiled_reference(lib, km, flags):
    """every recorded case of the km and flag set, with nothing in between; the figures are printed before the assertion"""
    for name, c in KI.CASES.items():
        if c["km"] == km and c["flags"] == flags:
            S.check_lib_against_golden(lib, name)


def test_table_is_the_compilers(lib):
    S.check_table(lib)


@pytest.mark.parametrize("flags", FLAGS)
def test_library_against_the_restatement(lib, flags):
    for hydrostatic, moist_kappa in ((True, False), (False, True)):
        for K_cycle in (1, 3):
            S.check_against_checker(lib, (37, 21, 12), flags, hydrostatic, moist_kappa, K_cycle)


@pytest.mark.parametrize("flags", ["none", "trwh"])
def test_water_is_conserved(lib, flags):
    S.check_conservation(lib, (37, 21, 12), flags)


def test_refusals(lib):
    S.check_refusals(lib)


@pytest.mark.parametrize("flags", ["none", "trwh"])
def test_six_faces_in_one_launch(lib, flags):
    S.check_six_faces(lib, flags)


@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fv_dynamics_k_warm_rain(lib, where):
    assert S.check_host(lib, where) <= 1.0


def test_chained_golden_through_the_host_method(lib):
    S.check_chain(lib)
