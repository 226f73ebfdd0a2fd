"""The memory contract on the CPU: the HIP kernels compiled by g++ in host-emulation mode (tests/hostemu) under FV3_MI355X_POISON=1 --
every work array of the library poisoned at every compute entry and guarded, the emulated LDS poisoned before every workgroup -- with
every test array between guard bands and every `out` array holding the pattern (tests/memory_contract.py).  The same cases run against
the product library in tests/test_memory_contract_gpu.py."""
import os
import subprocess

import pytest

import memory_contract as MC
from gfdl_atmos_cubed_sphere_amd.lib import Fv3Lib

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = MC.cases()


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "hostemu"), "-s"])
    return Fv3Lib(os.path.join(HERE, "hostemu", "libfv3_hostemu.so"))


@pytest.mark.parametrize("env,run", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_memory_contract(emu, monkeypatch, env, run):
    MC.run_case(emu, monkeypatch, env, run)


def test_guard_band_detects_an_overrun_of_one_element(emu, monkeypatch):
    MC.check_guard_detects_overrun(emu, monkeypatch)


def test_no_poison_fill_without_the_switch(emu, monkeypatch):
    MC.check_switch_off_makes_no_fill(emu, monkeypatch)
