"""The memory contract of fv3_held_suarez_tend and fv3_age_of_air on the MI355X: the cases of
tests/test_held_suarez_contract_hostemu.py on the product library."""
import pytest

import held_suarez_inputs as HI
import memory_contract as MC
import parity_held_suarez as S

from parity_phys import lib  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("set_name", list(HI.SETS))
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_held_suarez_under_the_contract(lib, monkeypatch, shape, set_name):
    assert MC.run_case(lib, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, set_name)) <= max(S.BOUND.values())
