"""The memory contract of fv3_reed_sim_phys and fv3_terminator_advance on the CPU (tests/memory_contract.py): FV3_MI355X_POISON=1, every
device array between guard bands of 1024 doubles -- the layouts the kernel reads among them: A x npz with halo, the halo-less t_dt /
q_dt / delz, pe, peln, phis, rain -- and the six coefficient planes of the boundary-layer solve, a work array of the context, between
bands of their own and filled with the pattern at the head of every call; with fresh the outputs prefilled with the pattern; inputs
and halos bit-unchanged; calls made after an fv3_fv_update_phys, a terminator call and another branch set in the same context against
a fresh context."""

import pytest

import memory_contract as MC
import parity_reed as S
import reed_inputs as RI

from parity_phys import emu  # noqa: F401

SHAPES = ((21, 7, 1), (21, 7, 2), (37, 21, 12))
IDS = ["21x7x1", "21x7x2", "37x21x12"]


@pytest.mark.parametrize("flags", list(RI.FLAGS))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_reed_under_the_contract(emu, monkeypatch, shape, flags):
    assert MC.run_case(emu, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, flags)) <= max(S.MEASURED.values()) * 10.0
