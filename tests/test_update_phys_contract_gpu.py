"""The memory contract of fv3_fv_update_phys and the sequence behind it on the MI355X: the cases of
tests/test_update_phys_contract_hostemu.py on the product library."""
import pytest

import memory_contract as MC
import parity_common as P
import parity_update_phys as S

from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", [(40, 19, 12), (130, 100, 5)], ids=["40x19x12", "130x100x5"])
def test_fv_update_phys_under_the_contract(lib, monkeypatch, shape, hydrostatic):
    assert MC.run_case(lib, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, hydrostatic)) <= P.TOL
