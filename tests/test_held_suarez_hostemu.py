"""The Held-Suarez forcing on the CPU: the numpy restatement tests/ref_held_suarez.py against the outputs of the reference's compiled
Fortran (tests/golden/held_suarez_*.npz), and fv3_held_suarez_tend / fv3_age_of_air of the host-emulation library (tests/hostemu) and
FvDynamics.held_suarez against those outputs, against the restatement at larger shapes, and in their properties.  The same check
bodies run on the product library in tests/test_held_suarez_gpu.py."""

import pytest

import held_suarez_inputs as HI
import parity_common as P
import parity_held_suarez as S

from parity_phys import emu  # noqa: F401

SETS = list(HI.SETS)


@pytest.mark.parametrize("name", list(HI.CASES))
def test_restatement_is_the_compiled_reference(name):
    """no library: u_dt, v_dt bit for bit, t_dt at its bound, and the recorded cases reach the branches they are there for"""
    S.check_checker_against_golden(name)


def test_recorded_cases_cover_the_cross():
    """(strat) x (zurita) with km 1, 2, 12, 32, two pdt, a small earth, non-zero and zero incoming tendencies"""
    c = HI.CASES
    for s, z in HI.SETS.values():
        mine = [v for v in c.values() if v["strat"] == s and v["zurita"] == z]
        assert {v["km"] for v in mine} >= {1, 2, 12, 32}
        assert len({v["pdt"] for v in mine}) >= 2 and any(v["radius"] != HI.RADIUS for v in mine)
        assert any(v["zero"] for v in mine) and any(not v["zero"] for v in mine)
    assert any(v["time"] == 0.0 for v in HI.AGE_CASES.values()) and any(v["time"] > 1.0 for v in HI.AGE_CASES.values())


@pytest.mark.parametrize("name", list(HI.CASES))
def test_library_against_the_compiled_reference(emu, name):
    S.check_lib_against_golden(emu, name)


@pytest.mark.parametrize("set_name", SETS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_library_against_the_restatement(emu, shape, set_name):
    S.check_against_checker(emu, shape, set_name)


@pytest.mark.parametrize("set_name", SETS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_fresh_is_zero_then_call_and_writes_every_cell(emu, shape, set_name):
    S.check_fresh(emu, shape, set_name)


@pytest.mark.parametrize("set_name", SETS)
@pytest.mark.parametrize("shape", S.SHAPES[1:3], ids=S.IDS[1:3])
def test_equilibrium_has_no_tendency(emu, shape, set_name):
    S.check_equilibrium(emu, shape, set_name)


@pytest.mark.parametrize("set_name", SETS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_friction_leaves_the_rest_alone(emu, shape, set_name):
    S.check_friction_bits(emu, shape, set_name)


@pytest.mark.parametrize("name", list(HI.AGE_CASES))
def test_age_of_air_against_the_compiled_reference(emu, name):
    S.check_age_against_golden(emu, name)


@pytest.mark.parametrize("time", [0.0, 86400.0])
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_age_of_air_against_the_restatement(emu, shape, time):
    S.check_age_against_checker(emu, shape, time)


def test_refusals(emu):
    S.check_refusals(emu)


@pytest.mark.parametrize("set_name", SETS)
def test_six_faces_in_one_launch(emu, set_name):
    S.check_six_faces(emu, set_name)


@pytest.mark.parametrize("set_name", ["strat", "zurita"])
@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fv_dynamics_held_suarez(emu, where, set_name):
    assert S.check_host(emu, where, set_name) <= P.TOL


def test_chained_golden_through_the_host_method(emu):
    S.check_chain(emu)
