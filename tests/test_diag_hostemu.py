"""fv_diag on the CPU: fv3_interpolate_vertical of the host-emulation library (tests/hostemu) against the outputs of the reference's compiled Fortran
(tests/golden/diag_interpolate_vertical.npz) and the numpy restatement tests/ref_fv_diag.py, its refusals, the memory contract and the six-face launch.  The same check bodies (tests/parity_diag.py) run on
the product library in tests/test_diag_gpu.py."""

import pytest

import parity_diag as D

from parity_phys import emu  # noqa: F401


@pytest.mark.parametrize("in_ng", [0, 3])
@pytest.mark.parametrize("km", D.KMS)
@pytest.mark.parametrize("shape", D.SHAPES, ids=["21x7", "40x19", "130x100"])
def test_library_against_the_restatement(emu, shape, km, in_ng):
    D.check_against_restatement(emu, shape, km, in_ng)


@pytest.mark.parametrize("name", list(D.GOLDEN_CASES))
def test_restatement_is_the_compiled_reference(name):
    D.check_restatement_against_golden(name)


@pytest.mark.parametrize("in_ng", [0, 3])
@pytest.mark.parametrize("name", list(D.GOLDEN_CASES))
def test_library_against_the_compiled_reference(emu, name, in_ng):
    D.check_lib_against_golden(emu, name, in_ng)


def test_level_on_a_layer_mean(emu):
    D.check_on_a_layer_mean(emu)


def test_refusals(emu):
    D.check_refusals(emu)


def test_memory_contract(emu, monkeypatch):
    D.check_memory_contract(emu, monkeypatch)


def test_six_faces_in_one_launch(emu):
    D.check_six_faces(emu)
