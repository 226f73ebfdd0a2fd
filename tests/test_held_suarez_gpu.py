"""The Held-Suarez forcing on the MI355X: the check bodies of tests/parity_held_suarez.py (see tests/test_held_suarez_hostemu.py) on the
product library, the same cases and the same bounds."""
import pytest

import held_suarez_inputs as HI
import parity_common as P
import parity_held_suarez as S

from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu

SETS = list(HI.SETS)


@pytest.mark.parametrize("set_name", SETS)
def test_library_against_the_compiled_reference(lib, set_name):
    """every recorded case of the set, with nothing in between; the figures are printed before the assertion"""
    for name, c in HI.CASES.items():
        if c["group"] == set_name:
            S.check_lib_against_golden(lib, name)


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_library_against_the_restatement(lib, shape):
    for set_name in SETS:
        S.check_against_checker(lib, shape, set_name)


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_fresh_is_zero_then_call_and_writes_every_cell(lib, shape):
    for set_name in SETS:
        S.check_fresh(lib, shape, set_name)


@pytest.mark.parametrize("shape", S.SHAPES[1:3], ids=S.IDS[1:3])
def test_equilibrium_has_no_tendency(lib, shape):
    for set_name in SETS:
        S.check_equilibrium(lib, shape, set_name)


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_friction_leaves_the_rest_alone(lib, shape):
    for set_name in SETS:
        S.check_friction_bits(lib, shape, set_name)


def test_age_of_air_against_the_compiled_reference(lib):
    for name in HI.AGE_CASES:
        S.check_age_against_golden(lib, name)


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_age_of_air_against_the_restatement(lib, shape):
    for time in (0.0, 86400.0):
        S.check_age_against_checker(lib, shape, time)


def test_refusals(lib):
    S.check_refusals(lib)


@pytest.mark.parametrize("set_name", SETS)
def test_six_faces_in_one_launch(lib, set_name):
    S.check_six_faces(lib, set_name)


@pytest.mark.parametrize("set_name", ["strat", "zurita"])
@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fv_dynamics_held_suarez(lib, where, set_name):
    assert S.check_host(lib, where, set_name) <= P.TOL


def test_chained_golden_through_the_host_method(lib):
    S.check_chain(lib)
