"""The memory contract of fv3_fv_subgrid_z and fv3_update_dwinds_phys on the MI355X: the cases of tests/test_subgrid_contract_hostemu.py
on the product library."""
import pytest

import memory_contract as MC
import parity_common as P
import parity_subgrid as S

from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", [(40, 19, 12), (130, 100, 5)], ids=["40x19x12", "130x100x5"])
def test_fv_subgrid_z_under_the_contract(lib, monkeypatch, shape, hydrostatic):
    assert MC.run_case(lib, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, hydrostatic)) <= P.TOL


def test_update_dwinds_phys_under_the_contract(lib, monkeypatch):
    assert MC.run_case(lib, monkeypatch, {}, lambda lib: max(S.check_dwinds_tile(lib, (40, 19, 3)), S.check_dwinds_sphere(lib))) <= P.TOL
