"""The kernels' logic against the REFERENCE's compiled Fortran on the CPU, with no oracle in between: the recorded cases of
tests/golden/refpin_*.npz (always) and, where oracle/_ref/libfv3ref.so is at hand, live cases at the shapes where kernels go
wrong, through the host-emulation build of the kernel sources (tests/hostemu).  The same checks run on the product library in
tests/test_reference_pin_gpu.py.

Bound: the kernel-versus-oracle TOL of parity_common (1e-14) plus the measured oracle-versus-reference bound of the routine
(refpin_common.MEASURED): relative RMS of every output field."""
import os
import subprocess
import sys

import pytest

import parity_common as P
import parity_remap as PR
import ref_lib as R
import refpin_common as RC

from gfdl_atmos_cubed_sphere_amd.lib import Fv3Lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_refpin_golden as G  # noqa: E402

KERNEL_ROUTINES = [r for r in G.ROUTINES if r not in ("a2b_ord4", "remap")]   # a2b_ord4 and the map routines have no entry point of their own


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "hostemu"), "-s"])
    return Fv3Lib(os.path.join(HERE, "hostemu", "libfv3_hostemu.so"))


@pytest.fixture(scope="module")
def ref():
    if R.can_build():
        assert R.available()
    elif not os.path.isfile(R.SO):
        pytest.skip("no reference tree and no oracle/_ref/libfv3ref.so")
    R.lib()
    return R


@pytest.mark.parametrize("form", list(RC.KERNEL_FORMS))
@pytest.mark.parametrize("routine", KERNEL_ROUTINES)
def test_kernels_reproduce_the_golden(emu, routine, form, monkeypatch):
    """the recorded cases under each kernel form: the default dispatch, d_sw as its unfused marching kernels, and the LDS-tile
    kernels for c_sw / d_sw / fv_tp_2d (the switches are read when a context is created)"""
    for k, v in RC.KERNEL_FORMS[form].items():
        monkeypatch.setenv(k, v)
    n, failures = 0, []
    for name, key, got, want in G.replay(routine, G.lib_runner(emu)):
        try:
            w = RC.compare(key, got, want, extra=P.TOL, what=name)
            print(f"refpin {form} {name}: {w:.3e}")
        except AssertionError as e:
            failures.append(f"{name}: {str(e).splitlines()[0]}")
        n += 1
    assert n > 0 and not failures, "\n".join(failures)


@pytest.mark.parametrize("form", list(RC.KERNEL_FORMS))
def test_kernels_against_the_reference_live(emu, ref, form, monkeypatch):
    """the live cases (refpin_common.live_kernel_cases) under each kernel form, so that the marching operators, fused and
    unfused, AND the tile form of c_sw, d_sw, fv_tp_2d and update_dz_d's transport are each held to the reference"""
    for k, v in RC.KERNEL_FORMS[form].items():
        monkeypatch.setenv(k, v)
    lines, n = RC.check_live(emu, ref, True, "emu")
    assert n > 60
    print("\n".join(f"refpin live {form} {x}" for x in lines))


@pytest.mark.parametrize("kord", [4, 6, 7])
@pytest.mark.parametrize("nq", [2, 6])
def test_tracer_remap_below_kord_8(emu, nq, kord):
    """nq > 5 is mapn_tracer, which runs scalar_profile whatever the kord (fv_operators.F90:273; the pin found the oracle and the
    kernel running ppm_profile there); nq <= 5 is map1_q2, which keeps ppm_profile below 8.  tests/test_reference_pin.py holds
    the oracle's two operators to the reference; this holds the kernel to the oracle through a whole Lagrangian_to_Eulerian."""
    PR.check_remap(emu, nq=nq, kord=kord)
