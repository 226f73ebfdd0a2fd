"""The Kessler warm-rain microphysics on the CPU: the numpy restatement tests/ref_kessler.py against the outputs of the reference's
compiled Fortran (tests/golden/kessler/*.npz), and fv3_k_warm_rain / fv3_qs_wat_init of the host-emulation library (tests/hostemu) and
FvDynamics.k_warm_rain against those outputs, against the restatement at a shape with several blocks and a tail block, and in their
properties.  The same check bodies run on the product library in tests/test_kessler_gpu.py."""

import pytest

import kessler_inputs as KI
import parity_kessler as S
import ref_kessler as R

from parity_phys import emu  # noqa: F401

FLAGS = list(KI.FLAGS)
KMS = (1, 2, 12, 32)


def cases_of(km, flags):
    return [n for n, c in KI.CASES.items() if c["km"] == km and c["flags"] == flags]


def test_restatement_is_the_compiled_reference_and_takes_every_branch():
    """no library: every recorded case at the library's bounds, and over the recorded set every branch the inputs are there for"""
    total = dict.fromkeys(R.COUNTS, 0)
    for name in KI.CASES:
        for k, v in S.check_checker_against_golden(name).items():
            total[k] += v
    assert all(total[k] > 0 for k in R.COUNTS), {k: v for k, v in total.items() if v == 0}


def test_recorded_cases_cover_what_the_issue_lists():
    """km 1, 2, 12, 32; hydrostatic or not; moist_kappa on / off; the five flag sets; K_cycle 1 and 3 at km 12 and 32 for every
    flag set; two pdt; K_cycle = 0 once per km <= 12 (at km 12 with pdt = 75: nint(2.5) = 3)"""
    cs = KI.CASES.values()
    assert {c["km"] for c in cs} == set(KMS) and (KI.NX, KI.NY) == (12, 7)
    assert set(KI.FLAGS.values()) == {(False, False, False), (True, False, False), (True, True, False), (True, True, True), (False, False, True)}
    for km in KMS:
        sub = [c for c in cs if c["km"] == km]
        assert {c["hydrostatic"] for c in sub} == {True, False} and {c["moist_kappa"] for c in sub} == {True, False}
        assert {c["pdt"] for c in sub} == set(KI.PDTS) and (0 in {c["K_cycle"] for c in sub}) == (km <= 12)
        assert {c["tracers"] for c in sub} == {(1, 2, 3), (4, 1, 3)}
        for f in FLAGS:
            assert {c["hydrostatic"] for c in sub if c["flags"] == f} == {True, False}
            if km >= 12:
                assert {1, 3} <= {c["K_cycle"] for c in sub if c["flags"] == f}, (km, f)
    assert set(S.MEASURED) == {(f, n) for f in FLAGS for n in S.FIELDS} == set(S.LIBRARY)
    for f, (tr, sw, _) in KI.FLAGS.items():      # bit-identical exactly where nothing is added
        for n in S.WINDS:
            assert (S.MEASURED[(f, n)] == 0.0) == (not tr or (n == "w" and not sw)), (f, n)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("km", KMS)
def test_library_against_the_compiled_reference(emu, km, flags):
    for name in cases_of(km, flags):
        S.check_lib_against_golden(emu, name)


def test_table_is_the_compilers(emu):
    S.check_table(emu)


@pytest.mark.parametrize("K_cycle", [1, 3])
@pytest.mark.parametrize("hydrostatic,moist_kappa", [(True, False), (False, True)])
@pytest.mark.parametrize("flags", FLAGS)
def test_library_against_the_restatement(emu, flags, hydrostatic, moist_kappa, K_cycle):
    S.check_against_checker(emu, (37, 21, 12), flags, hydrostatic, moist_kappa, K_cycle)


@pytest.mark.parametrize("flags", ["none", "trwh"])
def test_water_is_conserved(emu, flags):
    S.check_conservation(emu, (37, 21, 12), flags)


def test_refusals(emu):
    S.check_refusals(emu)


@pytest.mark.parametrize("flags", ["none", "trwh"])
def test_six_faces_in_one_launch(emu, flags):
    S.check_six_faces(emu, flags)


@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fv_dynamics_k_warm_rain(emu, where):
    assert S.check_host(emu, where) <= 1.0


def test_chained_golden_through_the_host_method(emu):
    S.check_chain(emu)
