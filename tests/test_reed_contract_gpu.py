"""The memory contract of fv3_reed_sim_phys and fv3_terminator_advance on the MI355X: the cases of
tests/test_reed_contract_hostemu.py on the product library."""
import pytest

import memory_contract as MC
import parity_reed as S
import reed_inputs as RI

from test_reed_contract_hostemu import IDS, SHAPES
from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flags", list(RI.FLAGS))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_reed_under_the_contract(lib, monkeypatch, shape, flags):
    assert MC.run_case(lib, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, flags)) <= max(S.MEASURED.values()) * 10.0
