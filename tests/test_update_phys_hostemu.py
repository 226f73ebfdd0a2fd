"""fv_update_phys on the CPU: the numpy restatement tests/ref_update_phys.py against the outputs of the reference's compiled Fortran
(tests/golden/update_phys_*.npz), and fv3_fv_update_phys of the host-emulation library (tests/hostemu) with the sequence behind it
against those outputs, against the restatement at larger shapes, and in its properties.  The same check bodies run on the product
library in tests/test_update_phys_gpu.py."""

import pytest

import parity_common as P
import parity_update_phys as S
import update_phys_inputs as UI

from parity_phys import emu  # noqa: F401

IDS = ["21x7x1", "21x7x2", "40x19x12", "130x100x5"]
MODES = [(True, True), (False, True), (False, False)]      # (hydrostatic, phys_hydrostatic)
MODE_IDS = ["hydro", "nh_phys_hydro", "nh"]


@pytest.mark.parametrize("name", list(UI.CASES))
def test_restatement_is_the_compiled_reference(name):
    """no library: bit for bit in every field without a transcendental, and the recorded cases reach every branch they are there for"""
    S.check_checker_against_golden(name)


def test_recorded_cases_cover_the_branches():
    """hydrostatic x nwat 0..6; both nonhydrostatic forms x nwat 0, 2, 6; q_dt absent; both signs of tau_h2o; adjust_mass off"""
    c = UI.CASES
    assert {(v["hydrostatic"], v["nwat"]) for v in c.values() if v["hydrostatic"]} >= {(True, n) for n in range(7)}
    for ph in (True, False):
        assert {v["nwat"] for v in c.values() if not v["hydrostatic"] and v["phys_hydrostatic"] == ph} >= {0, 2, 6}
    assert any(not v["has_qdt"] for v in c.values()) and any(v["tau_h2o"] < 0 for v in c.values()) and any(v["tau_h2o"] > 0 for v in c.values())
    assert any(v["adjust_off"] for v in c.values()) and all(v["ncnst"] > v["nq"] and v["cld_amt"] and v["w_diff"] for v in c.values())


@pytest.mark.parametrize("name", list(UI.CASES))
def test_library_against_the_compiled_reference(emu, name):
    worst, bits, trans = S.check_lib_against_golden(emu, name)
    assert worst <= P.TOL
    assert all(bits[n] for n in bits if n not in S.BOUND), bits      # every field without a transcendental is bit-identical


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nwat", S.NWATS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_library_against_the_restatement(emu, shape, nwat, mode):
    assert S.check_against_checker(emu, shape, mode[0], mode[1], nwat) <= P.TOL


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kw", [dict(has_qdt=False), dict(gfs_phys=True), dict(has_qdt=False, gfs_phys=True), dict(tau_h2o=2.0), dict(tau_h2o=-1.0)],
                         ids=["no_q_dt", "gfs_phys", "no_q_dt_gfs_phys", "tau_pos", "tau_neg"])
@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_library_options_against_the_restatement(emu, shape, kw, mode):
    for nwat in (0, 2, 6):
        assert S.check_against_checker(emu, shape, mode[0], mode[1], nwat, **kw) <= P.TOL


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", S.SHAPES[2:], ids=IDS[2:])
def test_zero_tendencies_keep_the_bits(emu, shape, mode):
    S.check_zero_tendencies(emu, shape, mode[0], mode[1])


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("nwat", [1, 3, 6])
def test_dry_mass_is_conserved(emu, nwat, hydrostatic):
    S.check_dry_mass(emu, (40, 19, 12), hydrostatic, nwat)


def test_refusals(emu):
    S.check_refusals(emu)


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
def test_six_faces_in_one_launch(emu, hydrostatic):
    S.check_six_faces(emu, hydrostatic=hydrostatic)


@pytest.mark.parametrize("gfs_phys", [False, True], ids=["winds", "gfs_phys"])
@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fv_dynamics_fv_update_phys(emu, where, gfs_phys):
    assert S.check_host(emu, where, gfs_phys) <= P.TOL
