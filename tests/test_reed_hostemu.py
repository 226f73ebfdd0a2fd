"""The Reed-Jablonowski simple physics and the terminator chemistry on the CPU: the numpy restatement tests/ref_reed.py against the
outputs of the reference's compiled Fortran (tests/golden/reed/*.npz), and fv3_reed_sim_phys / fv3_terminator_advance of the
host-emulation library (tests/hostemu) and FvDynamics.reed_sim_phys against those outputs, against the restatement at shapes with
several blocks and a tail block, and in their properties.  The same check bodies run on the product library in
tests/test_reed_gpu.py."""

import pytest

import parity_common as P
import parity_reed as S
import reed_inputs as RI

from parity_phys import emu  # noqa: F401

FLAGS = list(RI.FLAGS)


def cases_of(group):
    return [n for n, c in RI.CASES.items() if c["group"] == group]


@pytest.mark.parametrize("group", RI.GROUPS)
def test_restatement_is_the_compiled_reference(group):
    """no library: every recorded case of the file at the library's bounds, and the branches the cases are there for"""
    for name in cases_of(group):
        S.check_checker_against_golden(name)


def test_recorded_cases_cover_the_cross():
    """km 1, 2, 12, 32 x (hydrostatic, not) x reed_test 0, 1 x the four flag sets x two pdt x (non-zero, zero) incoming tendencies"""
    seen = {(c["km"], c["hydrostatic"], c["reed_test"], c["flags"], c["pdt"], c["zero"]) for c in RI.CASES.values()}
    assert len(seen) == len(RI.CASES) == 4 * 2 * 2 * 4 * 2 * 2
    assert {c["km"] for c in RI.CASES.values()} == {1, 2, 12, 32} and (RI.NX, RI.NY) == (12, 7)
    assert set(RI.FLAGS.values()) == {(True, False, False), (False, False, False), (True, True, False), (True, False, True)}
    assert len(RI.TERM_CASES) == 4 and {c["fill"] for c in RI.TERM_CASES.values()} == {True, False}
    assert set(S.MEASURED) == {(f, n) for f, (c, _, _) in RI.FLAGS.items() for n in S.TEND + (("rain",) if c else ())}


@pytest.mark.parametrize("group", RI.GROUPS)
def test_library_against_the_compiled_reference(emu, group):
    for name in cases_of(group):
        S.check_lib_against_golden(emu, name)


def test_host_formed_planes_are_the_compilers(emu):
    S.check_planes(emu)


@pytest.mark.parametrize("hydrostatic", [True, False])
@pytest.mark.parametrize("flags", FLAGS)
def test_library_against_the_restatement(emu, flags, hydrostatic):
    S.check_against_checker(emu, (37, 21, 12), flags, hydrostatic)


@pytest.mark.parametrize("flags", FLAGS)
def test_fresh_is_zero_then_call_and_writes_every_cell(emu, flags):
    S.check_fresh(emu, (37, 21, 12), flags)


def test_reed_test_2_and_rain_without_condensation(emu):
    S.check_test2_and_rain(emu, (21, 13, 12))


@pytest.mark.parametrize("name", list(RI.TERM_CASES))
def test_terminator_restatement_is_the_compiled_reference(name):
    S.check_term_against_golden(None, name)


@pytest.mark.parametrize("name", list(RI.TERM_CASES))
def test_terminator_against_the_compiled_reference(emu, name):
    S.check_term_against_golden(emu, name)


@pytest.mark.parametrize("fill", [True, False])
def test_terminator_conserves_chlorine(emu, fill):
    S.check_term_conserves(emu, (37, 21, 12), fill)


def test_refusals(emu):
    S.check_refusals(emu)


@pytest.mark.parametrize("flags", ["cond", "alt"])
def test_six_faces_in_one_launch(emu, flags):
    S.check_six_faces(emu, flags)


@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fv_dynamics_reed_sim_phys(emu, where):
    assert S.check_host(emu, where) <= P.TOL


def test_chained_golden_through_the_host_method(emu):
    S.check_chain(emu)
