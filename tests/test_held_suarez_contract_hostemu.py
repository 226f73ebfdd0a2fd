"""The memory contract of fv3_held_suarez_tend and fv3_age_of_air on the CPU (tests/memory_contract.py): FV3_MI355X_POISON=1, every
device array between guard bands of 1024 doubles -- the five layouts the kernel reads among them: A x npz with halo, the halo-less
t_dt / pkz, pe, peln and the latitude planes --, with fresh the outputs prefilled with the pattern, inputs, halos and q_dt
bit-unchanged, and a call made after an fv3_fv_update_phys in the same context against a fresh context."""

import pytest

import held_suarez_inputs as HI
import memory_contract as MC
import parity_held_suarez as S

from parity_phys import emu  # noqa: F401


@pytest.mark.parametrize("set_name", list(HI.SETS))
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_held_suarez_under_the_contract(emu, monkeypatch, shape, set_name):
    assert MC.run_case(emu, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, set_name)) <= max(S.BOUND.values())
