"""The tail of fv_dynamics for moist runs on the GPU: fv3_neg_adj3 of the product library against the numpy restatement
tests/ref_neg_adj3.py, its properties, the six faces in one launch, and the Python host's switches neg_adj, nf_omega, dnats / dnrts and
cld_amt -- the cases of tests/test_fv_dynamics_tail_hostemu.py, no fallback."""
import functools

import pytest

import parity_common as P
import parity_negadj as NA

from gfdl_atmos_cubed_sphere_amd import lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prod():
    return L.load()


@functools.lru_cache(maxsize=None)
def base_run(lib, where):
    """the run without the filter that the nf_omega cases start from"""
    return (NA.run_tile if where == "tile" else NA.run_sphere)(lib)


@pytest.mark.parametrize("with_qa", [True, False], ids=["qa", "no_qa"])
@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", NA.SHAPES, ids=["40x19x12", "130x100x5"])
def test_neg_adj3_against_the_restatement(prod, shape, hydrostatic, with_qa):
    assert NA.check_against_restatement(prod, shape, hydrostatic, with_qa) <= P.TOL


@pytest.mark.parametrize("with_qa", [True, False], ids=["qa", "no_qa"])
@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", NA.SHAPES, ids=["40x19x12", "130x100x5"])
def test_neg_adj3_is_a_noop_without_negatives(prod, shape, hydrostatic, with_qa):
    NA.check_noop(prod, shape, hydrostatic, with_qa)


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
@pytest.mark.parametrize("shape", NA.SHAPES, ids=["40x19x12", "130x100x5"])
def test_neg_adj3_properties(prod, shape, hydrostatic):
    NA.check_properties(prod, shape, hydrostatic)


@pytest.mark.parametrize("hydrostatic", [False, True], ids=["nh", "hydro"])
def test_neg_adj3_six_faces_in_one_launch(prod, hydrostatic):
    NA.check_six_faces(prod, hydrostatic=hydrostatic)


@pytest.mark.parametrize("nf", [1, 2, 4])
@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_nf_omega(prod, where, nf):
    run = NA.run_tile if where == "tile" else NA.run_sphere
    assert NA.check_nf_omega(prod, base_run(prod, where), run, nf) <= P.TOL


def test_cld_amt_dnats_dnrts(prod):
    NA.check_cld_amt_rules(prod)


@pytest.mark.parametrize("with_qa", [True, False], ids=["qa", "no_qa"])
@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_step_with_neg_adj(prod, where, with_qa):
    assert NA.check_step_with_neg_adj(prod, NA.run_tile if where == "tile" else NA.run_sphere, with_qa) <= P.TOL


@pytest.mark.parametrize("where", ["tile", "sphere"])
def test_fortran_reference_signature_with_the_tail(prod, tmp_path, where):
    """the reference-signature fv_dynamics in Fortran with FV3_REFSIG_NEG_ADJ / _NF_OMEGA / _DNATS against the Python host with the same
    options: bit-identical, omga included"""
    import fortran_host as F
    if F.fortran_compiler() is None:
        pytest.skip("no Fortran compiler in this image")
    NA.check_fortran_tail(prod, tmp_path, where)


def test_refusals(prod):
    NA.check_refusals(prod)
    NA.check_host_refusals(prod)
