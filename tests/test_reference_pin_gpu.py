"""The HIP kernels against the REFERENCE's compiled Fortran, with no oracle in between (-m gpu).

Always: every pinned routine runs through the C ABI on the recorded inputs of tests/golden/refpin_*.npz and is compared with
the recorded reference outputs.  Where oracle/_ref/libfv3ref.so travelled with the tree, the same check also runs live at
the shapes where kernels go wrong (refpin_common.live_kernel_cases: widths that are no multiple of the wavefront or segment
size, one strip and several, km that is no multiple of the column kernels' chunk; the LDS-tile and marching kernels on
doubly periodic tiles, the pass / frame kernels on a whole cube face).

Bound: the kernel-versus-oracle TOL of parity_common (1e-14) plus the measured oracle-versus-reference bound of the routine
(refpin_common.MEASURED): relative RMS of every output field.  The Riemann solvers evaluate exp / log with the device's math
library, not correctly rounded either, which is what parity_nh's own tolerance is about; their reference bound here is the
project's 1e-12 ceiling already.

These tests read tests/golden/ and oracle/_ref/ only."""
import os
import sys

import pytest

import parity_common as P
import parity_remap as PR
import ref_lib as R
import refpin_common as RC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_refpin_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu
KERNEL_ROUTINES = [r for r in G.ROUTINES if r not in ("a2b_ord4", "remap")]


@pytest.fixture(scope="module")
def prod():
    from gfdl_atmos_cubed_sphere_amd import lib
    return lib.load()


@pytest.mark.parametrize("form", list(RC.KERNEL_FORMS))
@pytest.mark.parametrize("routine", KERNEL_ROUTINES)
def test_kernels_reproduce_the_golden(prod, routine, form, monkeypatch):
    """the recorded cases under each kernel form: the default dispatch, d_sw as its unfused marching kernels, and the LDS-tile
    kernels for c_sw / d_sw / fv_tp_2d (the switches are read when a context is created)"""
    for k, v in RC.KERNEL_FORMS[form].items():
        monkeypatch.setenv(k, v)
    n, failures = 0, []
    for name, key, got, want in G.replay(routine, G.lib_runner(prod)):
        try:
            w = RC.compare(key, got, want, extra=P.TOL, what=name)
            print(f"refpin {form} {name}: {w:.3e}")
        except AssertionError as e:
            failures.append(f"{name}: {str(e).splitlines()[0]}")
        n += 1
    assert n > 0 and not failures, "\n".join(failures)


@pytest.mark.parametrize("form", list(RC.KERNEL_FORMS))
def test_kernels_against_the_reference_live(prod, form, monkeypatch):
    """the live cases (refpin_common.live_kernel_cases) under each kernel form, so that the marching operators, fused and
    unfused, AND the tile form of c_sw, d_sw, fv_tp_2d and update_dz_d's transport are each held to the reference"""
    if not os.path.isfile(R.SO):
        pytest.skip("oracle/_ref/libfv3ref.so did not travel here: the golden leg above is the check")
    for k, v in RC.KERNEL_FORMS[form].items():
        monkeypatch.setenv(k, v)
    lines, n = RC.check_live(prod, R, False, "prod")
    assert n > 120
    print("\n".join(f"refpin live {form} {x}" for x in lines))


@pytest.mark.parametrize("kord", [4, 6, 7])
@pytest.mark.parametrize("nq", [2, 6])
def test_tracer_remap_below_kord_8(prod, nq, kord):
    """nq > 5 is mapn_tracer, which runs scalar_profile whatever the kord (fv_operators.F90:273); nq <= 5 is map1_q2, which keeps
    ppm_profile below 8.  tests/test_reference_pin.py holds the oracle's two operators to the reference; this holds the kernel
    to the oracle through a whole Lagrangian_to_Eulerian."""
    PR.check_remap(prod, nq=nq, kord=kord)
