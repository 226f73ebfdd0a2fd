"""The memory contract on the MI355X: the cases of tests/test_memory_contract_hostemu.py against the product library under
FV3_MI355X_POISON=1.  What only the GPU has -- block counts rounded up to the XCD count, partial wavefronts, ragged last strips and
segments of real wavefronts -- writes into guard bands here or nowhere.  (LDS cannot be poisoned on the GPU: docs/SWITCHES.md.)"""
import pytest

import memory_contract as MC
from gfdl_atmos_cubed_sphere_amd import lib as L

pytestmark = pytest.mark.gpu
CASES = MC.cases()


@pytest.fixture(scope="module")
def prod():
    return L.load()


@pytest.mark.parametrize("env,run", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_memory_contract(prod, monkeypatch, env, run):
    MC.run_case(prod, monkeypatch, env, run)


def test_guard_band_detects_an_overrun_of_one_element(prod, monkeypatch):
    MC.check_guard_detects_overrun(prod, monkeypatch)


def test_no_poison_fill_without_the_switch(prod, monkeypatch):
    MC.check_switch_off_makes_no_fill(prod, monkeypatch)
