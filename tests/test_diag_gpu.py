"""fv_diag on the MI355X: the check bodies of tests/parity_diag.py (see tests/test_diag_hostemu.py) on the product library."""
import pytest

import parity_diag as D

from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("in_ng", [0, 3])
@pytest.mark.parametrize("km", D.KMS)
@pytest.mark.parametrize("shape", D.SHAPES, ids=["21x7", "40x19", "130x100"])
def test_library_against_the_restatement(lib, shape, km, in_ng):
    D.check_against_restatement(lib, shape, km, in_ng)


@pytest.mark.parametrize("in_ng", [0, 3])
@pytest.mark.parametrize("name", list(D.GOLDEN_CASES))
def test_library_against_the_compiled_reference(lib, name, in_ng):
    D.check_lib_against_golden(lib, name, in_ng)


def test_level_on_a_layer_mean(lib):
    D.check_on_a_layer_mean(lib)


def test_refusals(lib):
    D.check_refusals(lib)


def test_memory_contract(lib, monkeypatch):
    D.check_memory_contract(lib, monkeypatch)


def test_six_faces_in_one_launch(lib):
    D.check_six_faces(lib)
