"""The memory contract of fv3_k_warm_rain on the CPU (tests/memory_contract.py): FV3_MI355X_POISON=1, every device array between guard
bands of 1024 doubles -- the layouts the kernel reads and writes among them: A x npz with halo, the tracer array, the halo-less delz,
pe, peln, pk, ps, rain -- and the twelve planes that hold a column's state between cycles, a work array of the context, between bands
of their own and filled with the pattern at the head of every call: written by the first cycle before a later one reads them; rain
prefilled with the pattern and written in every cell; halos and the other tracer planes bit-unchanged; calls made after an
fv3_fv_update_phys, a call without work planes (K_cycle = 1) and another instantiation in the same context against a fresh context."""

import pytest

import kessler_inputs as KI
import memory_contract as MC
import parity_kessler as S

from parity_phys import emu  # noqa: F401

SHAPES = ((21, 7, 1), (21, 7, 2), (37, 21, 12))
IDS = ["21x7x1", "21x7x2", "37x21x12"]


@pytest.mark.parametrize("flags", list(KI.FLAGS))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kessler_under_the_contract(emu, monkeypatch, shape, flags):
    assert MC.run_case(emu, monkeypatch, {}, lambda lib: S.check_contract(lib, shape, flags)) <= 1.0
