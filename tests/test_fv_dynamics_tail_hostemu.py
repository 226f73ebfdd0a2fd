"""The tail of fv_dynamics for moist runs on the CPU: fv3_neg_adj3 (fv_sg.F90:968-1370) of the host-emulation library (tests/hostemu)
against the numpy restatement tests/ref_neg_adj3.py, its properties, and the Python host's switches neg_adj, nf_omega, dnats / dnrts
and cld_amt (fv_dynamics.F90:200-201, :569-572, :658-662, :722-745).  The same cases run on the product library in
tests/test_fv_dynamics_tail_gpu.py."""
import functools

import pytest

import parity_common as P
import parity_negadj as NA
import ref_neg_adj3 as R

from parity_phys import emu  # noqa: F401


@functools.lru_cache(maxsize=None)
def base_run(lib, where):
    """the run without the filter that the nf_omega cases start from"""
    return (NA.run_tile if where == "tile" else NA.run_sphere)(lib)


def test_restatement_counts_every_branch():
    """no library: the planted states reach every branch the restatement counts, in both modes and at both shapes"""
    for shape in NA.SHAPES:
        for hyd in (False, True):
            bd, st = NA.planted_state(*shape, seed=41 if hyd else 43)
            ref, cnt = NA.reference(bd, st, hyd, True)
            NA.assert_every_branch(cnt, True)
            assert set(cnt) == set(R.BRANCHES)


@pytest.mark.parametrize("with_qa", [True, False], ids=["qa", "no_qa"])
@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", NA.SHAPES, ids=["40x19x12", "130x100x5"])
def test_neg_adj3_against_the_restatement(emu, shape, hydrostatic, with_qa):
    assert NA.check_against_restatement(emu, shape, hydrostatic, with_qa) <= P.TOL


@pytest.mark.parametrize("with_qa", [True, False], ids=["qa", "no_qa"])
@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", NA.SHAPES, ids=["40x19x12", "130x100x5"])
def test_neg_adj3_is_a_noop_without_negatives(emu, shape, hydrostatic, with_qa):
    NA.check_noop(emu, shape, hydrostatic, with_qa)


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", NA.SHAPES, ids=["40x19x12", "130x100x5"])
def test_neg_adj3_properties(emu, shape, hydrostatic):
    NA.check_properties(emu, shape, hydrostatic)


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
def test_neg_adj3_six_faces_in_one_launch(emu, hydrostatic):
    NA.check_six_faces(emu, hydrostatic=hydrostatic)


@pytest.mark.parametrize("nf", [1, 2, 4])
@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_nf_omega(emu, where, nf):
    run = NA.run_tile if where == "tile" else NA.run_sphere
    assert NA.check_nf_omega(emu, base_run(emu, where), run, nf) <= P.TOL


def test_cld_amt_dnats_dnrts(emu):
    NA.check_cld_amt_rules(emu)


@pytest.mark.parametrize("with_qa", [True, False], ids=["qa", "no_qa"])
@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_step_with_neg_adj(emu, where, with_qa):
    assert NA.check_step_with_neg_adj(emu, NA.run_tile if where == "tile" else NA.run_sphere, with_qa) <= P.TOL


@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fortran_reference_signature_with_the_tail(emu, tmp_path, where):
    """the reference-signature fv_dynamics in Fortran with FV3_REFSIG_NEG_ADJ / _NF_OMEGA / _DNATS against the Python host with the same
    options: bit-identical, omga included"""
    import fortran_host as F
    if F.fortran_compiler() is None:
        pytest.skip("no Fortran compiler in this image")
    NA.check_fortran_tail(emu, tmp_path, where)


def test_refusals(emu):
    NA.check_refusals(emu)
    NA.check_host_refusals(emu)
