"""The Reed-Jablonowski simple physics and the terminator chemistry on the MI355X: the check bodies of tests/parity_reed.py (see
tests/test_reed_hostemu.py) on the product library, the same cases and the same bounds."""
import pytest

import parity_common as P
import parity_reed as S
import reed_inputs as RI

from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu

FLAGS = list(RI.FLAGS)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("km", [1, 2, 12, 32])
def test_library_against_the_compiled_reference(lib, km, flags):
    """every recorded case of the km and flag set, with nothing in between; the figures are printed before the assertion"""
    for name, c in RI.CASES.items():
        if c["km"] == km and c["flags"] == flags:
            S.check_lib_against_golden(lib, name)


def test_host_formed_planes_are_the_compilers(lib):
    S.check_planes(lib)


@pytest.mark.parametrize("flags", FLAGS)
def test_library_against_the_restatement(lib, flags):
    for hydrostatic in (True, False):
        S.check_against_checker(lib, (37, 21, 12), flags, hydrostatic)


@pytest.mark.parametrize("flags", FLAGS)
def test_fresh_is_zero_then_call_and_writes_every_cell(lib, flags):
    S.check_fresh(lib, (37, 21, 12), flags)


def test_reed_test_2_and_rain_without_condensation(lib):
    S.check_test2_and_rain(lib, (21, 13, 12))


def test_terminator_against_the_compiled_reference(lib):
    for name in RI.TERM_CASES:
        S.check_term_against_golden(lib, name)


@pytest.mark.parametrize("fill", [True, False])
def test_terminator_conserves_chlorine(lib, fill):
    S.check_term_conserves(lib, (37, 21, 12), fill)


def test_refusals(lib):
    S.check_refusals(lib)


@pytest.mark.parametrize("flags", ["cond", "alt"])
def test_six_faces_in_one_launch(lib, flags):
    S.check_six_faces(lib, flags)


@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fv_dynamics_reed_sim_phys(lib, where):
    assert S.check_host(lib, where) <= P.TOL


def test_chained_golden_through_the_host_method(lib):
    S.check_chain(lib)
