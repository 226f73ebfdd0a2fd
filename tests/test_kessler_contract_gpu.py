"""The memory contract of fv3_k_warm_rain on the MI355X: the cases of tests/test_kessler_contract_hostemu.py on the product library."""
import pytest

import kessler_inputs as KI
import memory_contract as MC
import parity_kessler as S

from test_kessler_contract_hostemu import IDS, SHAPES
from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flags", list(KI.FLAGS))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kessler_under_the_contract(lib, monkeypatch, shape, flags):
    assert MC.run_case(lib, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, flags)) <= 1.0
