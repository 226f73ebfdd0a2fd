"""Golden fixture of fv3_interpolate_vertical from the REFERENCE's own compiled Fortran:

    python tests/golden/make_diag_golden.py

interpolate_vertical (tools/fv_diagnostics.F90:4910-4948) reads no module state.  The generator cuts the routine -- from its
`subroutine` line to its `end subroutine` line, unmodified -- out of the file where it lies (FV3_REFERENCE) into a module of its own in
a temporary directory, compiles it with REF_FFLAGS of oracle/Makefile beside the bind(C) driver tests/golden/diag_ref/iv_driver.F90,
runs it on the cases of tests/parity_diag.GOLDEN_CASES and records the outputs:

    tests/golden/diag_interpolate_vertical.npz:  "<case>|out|<field>" (nx, ny, levels) and "<case>|sha" = the checksum of the inputs

(The whole module fv_diagnostics_mod needs stand-ins for some twenty FMS and model modules, which this project has not written; the
routine alone needs none.)  Data only: no line of the reference is written anywhere but the temporary directory.  The inputs are not
stored: the tests form them again from the seeds and compare the checksum.  Before anything is recorded the generator asserts that
the cases take every branch (above the first layer mean, below the last, inside) and that the numpy restatement gives the same bits.
Runs only where the reference tree and amdflang are present; no test reads the reference."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import diag_inputs as DI  # noqa: E402
import parity_diag as D  # noqa: E402

REFERENCE = os.environ.get("FV3_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))
LIMIT = 213341        # the largest golden committed before (ppm1d_golden.npz)


def ref_fflags():
    mk = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "Makefile")).read()
    return re.search(r"^REF_FFLAGS \?= (.*)$", mk, flags=re.M).group(1).split()


def build(tmp):
    lines = open(os.path.join(REFERENCE, "tools", "fv_diagnostics.F90")).read().split("\n")
    first = [n for n, l in enumerate(lines) if re.match(r"\s*subroutine\s+interpolate_vertical\s*\(", l)]
    last = [n for n, l in enumerate(lines) if re.match(r"\s*end\s+subroutine\s+interpolate_vertical\b", l)]
    assert len(first) == 1 and len(last) == 1 and first[0] < last[0], (first, last)
    with open(os.path.join(tmp, "iv_ref.F90"), "w") as f:
        f.write("module iv_ref_mod\n implicit none\ncontains\n" + "\n".join(lines[first[0]:last[0] + 1]) + "\nend module iv_ref_mod\n")
    fc = shutil.which("amdflang") or "/opt/rocm/bin/amdflang"
    objs = []
    for src in (os.path.join(tmp, "iv_ref.F90"), os.path.join(HERE, "diag_ref", "iv_driver.F90")):
        o = os.path.join(tmp, os.path.basename(src)[:-4] + ".o")
        subprocess.check_call([fc, *ref_fflags(), "-c", src, "-o", o], cwd=tmp)
        objs.append(o)
    so = os.path.join(tmp, "libivref.so")
    subprocess.check_call([fc, "-shared", "-o", so, *objs], cwd=tmp)
    return C.CDLL(so)


def run(dll, name):
    nx, ny, km, seed = D.GOLDEN_CASES[name]
    bd, st = DI.columns(nx, ny, km, seed)
    cnt = {}
    ref = D.run_ref(bd, st, km, cnt=cnt)
    assert cnt["above_top"] > 0 and cnt["below_bottom"] > 0 and (km < 3 or cnt["interior"] > 0), (name, cnt)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    out = {f"{name}|sha": np.array(DI.checksum(st))}
    for field, a3 in (("t", np.asfortranarray(D.cc(bd, st["pt"]))), ("vort", st["vort"])):
        got = np.zeros((nx, ny, len(D.LEVELS)), order="F")
        for n, plev in enumerate(D.LEVELS):
            a2 = np.zeros((nx, ny), order="F")
            dll.iv_run(C.c_int(1), C.c_int(nx), C.c_int(1), C.c_int(ny), C.c_int(km), C.c_double(plev), p(st["peln"]), p(a3), p(a2))
            got[:, :, n] = a2
        assert D.bits_equal(got, ref[field]), f"{name}: the restatement of {field} is not the compiled reference's"
        out[f"{name}|out|{field}"] = got
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        dll = build(tmp)
        d = {}
        for name in D.GOLDEN_CASES:
            d.update(run(dll, name))
    path = os.path.join(HERE, "diag_interpolate_vertical.npz")
    np.savez_compressed(path, **d)
    print(f"{os.path.basename(path)}: {len(d)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) <= LIMIT, "larger than the largest golden committed before"


if __name__ == "__main__":
    main()
