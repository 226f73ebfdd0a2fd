"""ctypes binding of the REFERENCE's own compiled Fortran (oracle/_ref/libfv3ref.so).  TEST INFRASTRUCTURE ONLY.

oracle/Makefile's `ref` target compiles the reference's hot-path modules, unmodified, against the stand-ins of
oracle/ref/fms_standins.F90 and links them with the bind(C) wrappers of oracle/ref/ref_driver.F90.  This module only LOADS
that library; it never reads the reference tree.  The functions take the project's GridStruct / Bounds and the same
arguments as their namesakes in oracle_lib, so a test can hand one set of inputs to the oracle and to the reference.

The product package never imports this module (tests/test_product_isolation.py checks that).

What the stand-ins cannot serve stops the process (Fortran `error stop`), so the guards below refuse such a call first:
a2b_ord4 on a tile that owns a cube corner (great_circle_dist) and d_sw with nord > 1 on such a tile (fill_corners).
"""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import oracle_lib as O
from oracle_lib import DswLevels, DswPar, _d, _dp, _ip, make_grid, p

_HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE_DIR = os.path.join(os.path.dirname(_HERE), "oracle")
SO = os.path.join(_ORACLE_DIR, "_ref", "libfv3ref.so")
# where oracle/Makefile finds the reference's sources (its REF_MODEL default); only its presence is looked at here
_REF_MODEL = os.environ.get("FV3_REF_MODEL", "/root/reference/model")
_LIB = None


def can_build() -> bool:
    """the reference's sources and a Fortran compiler are both at hand"""
    return os.path.isfile(os.path.join(_REF_MODEL, "sw_core.F90")) and shutil.which("amdflang") is not None


def available() -> bool:
    """True when the library is there (building it first where that is possible); raises where it should build and does not"""
    if can_build():
        # make is a no-op when the library is newer than the stand-ins, the wrappers and the reference's sources
        subprocess.check_call(["make", "-C", _ORACLE_DIR, "-s", "_ref/libfv3ref.so"], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        assert os.path.isfile(SO), "oracle/_ref/libfv3ref.so did not build although the reference tree and amdflang are present"
    return os.path.isfile(SO)


def lib():
    global _LIB
    if _LIB is None:
        assert available(), "oracle/_ref/libfv3ref.so is absent"
        _LIB = C.CDLL(SO)
    return _LIB


def _has_corner(g):
    return g.grid_type < 3 and not g.bounded_domain and (g.sw_corner or g.se_corner or g.ne_corner or g.nw_corner)


def fv_tp_2d(g, q, crx, cry, hord, xfx, yfx, ra_x, ra_y, mfx=None, mfy=None, mass=None, nord=-1, damp_c=0.0):
    b = g.bd
    fx, fy = b.zeros("FX"), b.zeros("FY")
    gs = make_grid(g)
    lib().ref_fv_tp_2d(C.byref(gs), p(q), p(crx), p(cry), C.c_int(hord), p(fx), p(fy), p(xfx), p(yfx), p(ra_x), p(ra_y),
                       p(mfx), p(mfy), p(mass), C.c_int(nord), C.c_double(damp_c))
    return fx, fy


def copy_corners(g, q, dir_):
    gs = make_grid(g)
    lib().ref_copy_corners(C.byref(gs), p(q), C.c_int(dir_))


def a2b_ord4(g, qin, qout, replace=False):
    assert not _has_corner(g), "a2b_ord4 at a cube corner needs great_circle_dist: not pinned"
    gs = make_grid(g)
    lib().ref_a2b_ord4(C.byref(gs), p(qin), p(qout), C.c_int(int(replace)))


def c_sw_3d(g, npz, f, nord, dt2, hydrostatic, dord4=True):
    gs = make_grid(g)
    lib().ref_c_sw_3d(C.byref(gs), C.c_int(npz), p(f["delpc"]), p(f["delp"]), p(f["ptc"]), p(f["pt"]), p(f["u"]), p(f["v"]),
                      p(f.get("w")), p(f["uc"]), p(f["vc"]), p(f["ua"]), p(f["va"]), p(f.get("wc")), p(f["ut"]), p(f["vt"]),
                      p(f["divg_d"]), C.c_int(nord), C.c_double(dt2), C.c_int(int(hydrostatic)), C.c_int(int(dord4)))


def d_sw_3d(g, npz, par: dict, lev: dict, f):
    if _has_corner(g):
        assert max(int(n) for n in lev["nord_k"]) <= 1, "d_sw with nord > 1 at a cube corner needs fill_corners: not pinned"
        assert max(int(n) for n in lev["nord_k"]) == 0 or par["dddmp"] < 1.e-5, \
            "d_sw with nord > 0 and dddmp at a cube corner needs a2b_ord4's great_circle_dist: not pinned"
    gs = make_grid(g)
    pr = DswPar()
    for k, v in par.items():
        setattr(pr, k, v)
    if f.get("inline_q") is not None:
        q = f["inline_q"]
        assert q.flags.f_contiguous and q.ndim == 4 and q.shape[2] == npz
        pr.inline_q, pr.nq, pr.q, pr.q_stride = 1, q.shape[3], p(q), q.shape[0] * q.shape[1] * q.shape[2]
    lv = DswLevels()
    keep = []
    for n in ["nord_k", "nord_v", "nord_w", "nord_t"]:
        a = np.ascontiguousarray(lev[n], dtype=np.int32)
        keep.append(a)
        setattr(lv, n, a.ctypes.data_as(_ip))
    for n in ["d2_divg", "damp_vt", "damp_w", "damp_t", "d_con_k"]:
        a = np.ascontiguousarray(lev[n], dtype=np.float64)
        keep.append(a)
        setattr(lv, n, a.ctypes.data_as(_dp))
    lib().ref_d_sw_3d(C.byref(gs), C.c_int(npz), C.byref(pr), C.byref(lv), p(f["delpc"]), p(f["delp"]), p(f["ptc"]),
                      p(f["pt"]), p(f["u"]), p(f["v"]), p(f.get("w")), p(f["uc"]), p(f["vc"]), p(f["ua"]), p(f["va"]),
                      p(f["divg_d"]), p(f["mfx"]), p(f["mfy"]), p(f["cx"]), p(f["cy"]), p(f["crx"]), p(f["cry"]),
                      p(f["xfx"]), p(f["yfx"]), p(f.get("q_con")), p(f["heat_source"]), p(f["diss_est"]))


def update_dz_c(g, km, dt, dp0, zs, ut, vt, gz, ws):
    gs = make_grid(g)
    dp0 = np.ascontiguousarray(dp0, dtype=np.float64)
    lib().ref_update_dz_c(C.byref(gs), C.c_int(km), _d(dt), dp0.ctypes.data_as(_dp), p(zs), p(ut), p(vt), p(gz), p(ws))


def update_dz_d(g, km, ndif, damp, hord, dp0, zs, zh, crx, cry, xfx, yfx, ws, rdt):
    gs = make_grid(g)
    ndif = np.ascontiguousarray(ndif, dtype=np.int32)
    damp = np.ascontiguousarray(damp, dtype=np.float64)
    dp0 = np.ascontiguousarray(dp0, dtype=np.float64)
    assert ndif.size == km + 1 and damp.size == km + 1
    lib().ref_update_dz_d(C.byref(gs), C.c_int(km), ndif.ctypes.data_as(_ip), damp.ctypes.data_as(_dp), C.c_int(hord),
                          dp0.ctypes.data_as(_dp), p(zs), p(zh), p(crx), p(cry), p(xfx), p(yfx), p(ws), _d(rdt))


def _check_consts(cn):
    from gfdl_atmos_cubed_sphere_amd.lib import GRAV, RDGAS
    assert cn["grav"] == GRAV and cn["rdgas"] == RDGAS, "the reference library carries the project's grav and rdgas"


def riem_solver_c(g, km, dt, cn, hs, w3, pt, delp, gz, pef, ws, q_con=None, cappa=None):
    _check_consts(cn)
    gs = make_grid(g)
    lib().ref_riem_solver_c(C.byref(gs), C.c_int(km), C.c_int(int(cn.get("m_split", 1))), _d(dt), _d(cn["akap"]),
                            _d(cn["ptop"]), p(hs), p(w3), p(pt), p(delp), p(gz), p(pef), p(ws), _d(cn["p_fac"]),
                            _d(cn["a_imp"]), p(q_con), p(cappa))


def riem_solver3(g, km, dt, cn, zs, w, delz, pt, delp, zh, pe, ppe, pk3, pk, peln, ws, use_logp, last_call, fp_out,
                 q_con=None, cappa=None):
    _check_consts(cn)
    gs = make_grid(g)
    lib().ref_riem_solver3(C.byref(gs), C.c_int(km), C.c_int(int(cn.get("m_split", 1))), _d(dt), _d(cn["akap"]),
                           _d(cn["ptop"]), p(zs), p(w), p(delz), p(pt), p(delp), p(zh), p(pe), p(ppe), p(pk3), p(pk),
                           p(peln), p(ws), _d(cn["p_fac"]), _d(cn["a_imp"]), C.c_int(int(use_logp)),
                           C.c_int(int(last_call)), C.c_int(int(fp_out)), p(q_con), p(cappa))


def remap_column(which, pe1, pe2, q1, qs, iv, kord, qmin=0.0):
    """0-based numpy columns in, 0-based out; which: 0 map_scalar, 1 map1_ppm, 2 map1_q2, 3 mapn_tracer"""
    km = q1.size
    a = lambda x: np.concatenate([[0.0], np.asarray(x, dtype=np.float64)])
    p1, p2, qq = a(pe1), a(pe2), a(q1)
    out = np.zeros(km + 1)
    lib().ref_remap_column(C.c_int(which), C.c_int(km), p1.ctypes.data_as(_dp), p2.ctypes.data_as(_dp),
                           qq.ctypes.data_as(_dp), out.ctypes.data_as(_dp), _d(qs), C.c_int(iv), C.c_int(kord), _d(qmin))
    return out[1:]


def fillz(q, dp):
    """q (im, km, nq), dp (im, km), F-ordered; q in place"""
    assert q.ndim == 3 and dp.shape == q.shape[:2]
    lib().ref_fillz(C.c_int(q.shape[0]), C.c_int(q.shape[1]), C.c_int(q.shape[2]), p(q), p(dp))


def oracle_fillz(q, dp):
    """the oracle's fillz of one column (fvo_fillz_column), applied to the same (im, km, nq) array"""
    fn = O.lib().fvo_fillz_column
    fn.restype = None
    km = q.shape[1]
    for n in range(q.shape[2]):
        for i in range(q.shape[0]):
            col = np.concatenate([[0.0], q[i, :, n]])
            d = np.concatenate([[0.0], dp[i, :]])
            fn(C.c_int(km), col.ctypes.data_as(_dp), d.ctypes.data_as(_dp))
            q[i, :, n] = col[1:]
