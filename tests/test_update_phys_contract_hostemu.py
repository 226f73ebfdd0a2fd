"""The memory contract of fv3_fv_update_phys and the sequence behind it on the CPU (tests/memory_contract.py): FV3_MI355X_POISON=1,
every device array between guard bands -- the halo-less t_dt / q_dt and the three pressure layouts among them --, the pure outputs
prefilled with the pattern, halos and everything the header calls unwritten bit-unchanged, and a call made after other kinds of
call in the same context against a fresh context."""

import pytest

import memory_contract as MC
import parity_common as P
import parity_update_phys as S

from parity_phys import emu  # noqa: F401


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", [(40, 19, 12), (130, 100, 5)], ids=["40x19x12", "130x100x5"])
def test_fv_update_phys_under_the_contract(emu, monkeypatch, shape, hydrostatic):
    assert MC.run_case(emu, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, hydrostatic)) <= P.TOL
