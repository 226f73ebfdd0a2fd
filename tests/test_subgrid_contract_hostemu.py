"""The memory contract of fv3_fv_subgrid_z and fv3_update_dwinds_phys on the CPU (tests/memory_contract.py): FV3_MI355X_POISON=1, every
device array between guard bands, the outputs u_dt / v_dt prefilled with the pattern, halos / levels below kbot / tracers beyond nq
bit-unchanged, and a call made after another kind of call in the same context against a fresh context."""

import pytest

import memory_contract as MC
import parity_common as P
import parity_subgrid as S

from parity_phys import emu  # noqa: F401


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", [(40, 19, 12), (130, 100, 5)], ids=["40x19x12", "130x100x5"])
def test_fv_subgrid_z_under_the_contract(emu, monkeypatch, shape, hydrostatic):
    assert MC.run_case(emu, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, hydrostatic)) <= P.TOL


def test_update_dwinds_phys_under_the_contract(emu, monkeypatch):
    assert MC.run_case(emu, monkeypatch, {}, lambda lib: max(S.check_dwinds_tile(lib, (40, 19, 3)), S.check_dwinds_sphere(lib))) <= P.TOL
