"""ctypes binding of the product library libfv3_mi355x.so (C ABI: include/fv3_mi355x.h).

There is NO CPU fallback: ``load()`` raises if the HIP library has not been built
(``python -c "import __graft_entry__ as g; g.build()"``), and every entry point raises
``Fv3Error`` on a non-zero status.  Device memory comes from the library's own ``fv3_malloc``
(hipMalloc); ``DeviceArray`` exposes ``__cuda_array_interface__`` so that torch (used only for
streams and torch.distributed) can alias a buffer without copying.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi
from .grid import GridStruct
from .layout import Bounds

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
PRODUCT_SO = os.path.join(_CSRC, "libfv3_mi355x.so")

# every symbol include/fv3_mi355x.h declares: what a loaded object must export (a tool that loads a variant build with fewer
# entry points assigns a shorter list first); signatures are bound for whatever of the header the object has
EXPORTS = list(abi.ROUTINES)


class Fv3Error(RuntimeError):
    pass


def _struct(name, src=None, /, default=None, **kw):
    """the header's struct `name` (fv3_ left out) filled from keywords, then from the mapping src (whose other keys are ignored);
    a member given by neither takes `default`, and is an error without one"""
    s = abi.CLASSES["fv3_" + name]()
    for n, _ in s._fields_:
        v = kw[n] if n in kw else src[n] if src is not None and n in src else default
        if v is None:
            raise Fv3Error(f"fv3_{name}: no value for the member {n}")
        setattr(s, n, v)
    return s


HaloField = abi.CLASSES["fv3_halo_field"]
CUBE_KINDS = {"A": 0, "B": 1, "D": 2, "C": 3, "Dedge": 4}


def cube_table(lib, npx: int, kind: str, member: int, face: int, ng: int = 3):
    """fv3_cube_table: the library's own halo topology of the cubed sphere (csrc/cube_topo.h) -> dict(dst, tile, comp, src, sign)"""
    args = (npx, ng, CUBE_KINDS[kind], member, face)
    n = lib.dll.fv3_cube_table(*args, None, None, None, None, None)     # the count alone: no table is written
    if n < 0:
        raise Fv3Error("fv3_cube_table: bad argument")
    dst, src = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    st, cp, sg = (np.zeros(n, dtype=np.int32) for _ in range(3))
    lib.dll.fv3_cube_table(*args, dst.ctypes, st.ctypes, cp.ctypes, src.ctypes, sg.ctypes)
    return dict(dst=dst, tile=st.astype(np.int64), comp=cp.astype(np.int64), src=src, sign=sg.astype(np.int64))


def _handles(ctxs):
    return (C.c_void_p * len(ctxs))(*[c.h.value for c in ctxs])


def cube_halo_start(ctxs, faces, face_rank, groups):
    """fv3_cube_halo_start.  ctxs: the contexts of the faces this rank holds (faces ascending; ctxs[0] has the communicator);
    groups: list of (kind, f0s, f1s, scalar_pair) with f0s / f1s = one DeviceArray per context (f1s None for kinds 'A' / 'B')"""
    n, nf = len(ctxs), len(groups)
    arr = (abi.CLASSES["fv3_cube_field"] * (n * nf))()
    for i in range(n):
        for f, (kind, f0s, f1s, sp) in enumerate(groups):
            a0 = f0s[i]
            e = arr[i * nf + f]
            e.kind, e.f0, e.f1 = CUBE_KINDS[kind], a0.ptr, (f1s[i].ptr if f1s is not None else None)
            e.nk = int(np.prod(a0.shape[2:])) if len(a0.shape) > 2 else 1
            e.scalar_pair = int(bool(sp))
    ctxs[0].lib.call("fv3_cube_halo_start", n, _handles(ctxs), (C.c_int * n)(*faces), (C.c_int * 6)(*face_rank), nf, arr)


def cube_halo_complete(ctxs):
    ctxs[0].lib.call("fv3_cube_halo_complete", len(ctxs), _handles(ctxs))


# FMS constants_mod (GFDL defaults, FMS 2024.03 constants/gfdl_constants.fh): not in the reference tree
GRAV, RDGAS, KAPPA = 9.80, 287.04, 2.0 / 7.0
CP_AIR = RDGAS / KAPPA
# what neg_adj3 (fv_sg.F90:968) takes from its host modules, the defaults of Context.neg_adj3 / FvDynamics(neg_adj_consts=...)
NEG_ADJ_CONSTS = dict(
    rdgas=RDGAS, grav=GRAV, cp_air=CP_AIR,   # constants_mod, as above
    rvgas=461.50,       # constants_mod RVGAS (gfdl_constants.fh)
    cp_vapor=4.0 * 461.50,   # constants_mod CP_VAPOR = 4 * RVGAS
    hlv=2.500e6,        # constants_mod HLV
    hlf=3.34e5,         # constants_mod HLF
    c_liq=4.218e3,      # gfdl_mp_mod c_liq (model/gfdl_mp.F90:137, used by fv_sg.F90:34): heat capacity of water at 0 deg C
    c_ice=2.106e3,      # gfdl_mp_mod c_ice (model/gfdl_mp.F90:136): heat capacity of ice at 0 deg C
)


def nh_consts(ptop, p_fac=0.05, a_imp=1.0, akap=KAPPA, grav=GRAV, rdgas=RDGAS, cp_air=CP_AIR, m_split=1):
    return dict(grav=grav, rdgas=rdgas, cp_air=cp_air, akap=akap, ptop=ptop, p_fac=p_fac, a_imp=a_imp, m_split=m_split)


# what reed_sim_physics and its wrapper (driver/solo/fv_phys.F90:74-85, :546-602, :2516-2520) take from constants_mod and gfdl_mp_mod
REED_CONSTS = dict(grav=GRAV, rdgas=RDGAS, rvgas=461.50, cp_air=CP_AIR, cp_vapor=4.0 * 461.50, c_liq=4.218e3, hlv=2.500e6, radius=6.3712e6,
                   omega=7.2921e-5, pi=3.14159265358979323846)


# what K_warm_rain, kessler_imp and qs_tables_mod (driver/solo/fv_phys.F90:74-85, :1992-2291; qs_tables.F90:24-43) take from constants_mod
# and gfdl_mp_mod
KESSLER_CONSTS = dict(rdgas=RDGAS, rvgas=461.50, cp_air=CP_AIR, cp_vapor=4.0 * 461.50, hlv=2.500e6, c_liq=4.218e3, grav=GRAV, kappa=RDGAS / CP_AIR)
QS_LENGTH = 2621


def _consts(name, defaults, consts):
    """the header's struct of constants `name`: the defaults, overridden by the caller's consts where it names one of them"""
    return _struct(name, {**defaults, **{n: float(v) for n, v in (consts or {}).items() if n in defaults}})


SG_SPECIES = ("sphum", "liq_wat", "rainwat", "ice_wat", "snowwat", "graupel")


class _Bound(dict):
    def __missing__(self, name):
        raise Fv3Error(f"the loaded library has no {name}")


class Fv3Lib:
    """A loaded shared object exporting the fv3_* C ABI."""

    def __init__(self, path: str):
        if not os.path.exists(path):
            raise Fv3Error(f"{path} not found: the HIP library is not built (run __graft_entry__.build()); "
                           "there is no CPU fallback")
        self.path = path
        self.host_memory = "hostemu" in os.path.basename(path)   # the tests' logic harness, never the product
        if not self.host_memory:
            # torch (streams, torch.distributed for the halo exchange) ships its own libamdhip64 with the same SONAME as
            # the one this library is linked to; whichever is mapped first serves the whole process.  Map torch's first:
            # the other order (this library's runtime initialised, torch importing later) leaves torch without a device
            # ("No HIP GPUs are available").
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        self.dll = C.CDLL(path)
        missing = [s for s in EXPORTS if not hasattr(self.dll, s)]
        if missing:
            raise Fv3Error(f"{path} does not export {missing}")
        self.fn = _Bound(abi.bind(self.dll))     # {routine: the function, restype and argtypes as the header declares them}

    def check(self, rc: int, what: str):
        if rc != 0:
            raise Fv3Error(f"{what}: {self.dll.fv3_last_error().decode()}")

    def call(self, name: str, *args):
        """the routine `name` of the header; a non-zero status raises with the library's message.  None is refused here, before the
        library sees it: a pointer the routine takes as optional is passed as _pp(x)."""
        if None in args:
            self.refuse(name, args)
        try:
            rc = self.fn[name](*args)
        except C.ArgumentError:
            rc = self.fn[name](*_addressed(args))
        if rc:
            self.check(1, name)

    @staticmethod
    def refuse(name, args):
        n = args.index(None)
        raise Fv3Error(f"{name}: argument {n} ({abi.ROUTINES[name].params[n].name}) is None")


_PRODUCT: Fv3Lib | None = None


def build_id() -> str:
    """Short hash of the kernel / C-ABI sources the product library is built from: measurements kept under profiles/
    (HBM traffic counters) carry it so that bench.py can tell a stale file from one taken on the build it is timing."""
    import hashlib
    h = hashlib.sha256()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith((".h", ".hip"))]
    files += [os.path.join(root, "include", f) for f in sorted(os.listdir(os.path.join(root, "include"))) if f.endswith(".h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:12]


def load() -> Fv3Lib:
    """The product library (HIP, gfx950).  Raises if it is missing."""
    global _PRODUCT
    if _PRODUCT is None:
        # FV3_MI355X_SO selects another build of the same HIP library (e.g. a contraction-on build)
        _PRODUCT = Fv3Lib(os.environ.get("FV3_MI355X_SO", PRODUCT_SO))
    return _PRODUCT


class DeviceArray:
    """A device buffer holding one field in the reference layout (Fortran order)."""

    def __init__(self, ctx: "Context", shape):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.nbytes = int(np.prod(self.shape)) * 8
        ptr = C.c_void_p()
        ctx.lib.call("fv3_malloc", C.byref(ptr), self.nbytes)
        self.ptr = ptr.value
        ctx._buffers.append(self)

    @property
    def p(self):
        return C.cast(C.c_void_p(self.ptr), C.POINTER(C.c_double))

    @property
    def _as_parameter_(self):      # what a call of the library passes for this array: its address
        return self.ptr

    @property
    def __cuda_array_interface__(self):
        # Fortran-ordered strides
        strides, acc = [], 8
        for s in self.shape:
            strides.append(acc)
            acc *= s
        return {"shape": self.shape, "typestr": "<f8", "data": (self.ptr, False), "version": 3,
                "strides": tuple(strides)}

    def upload(self, a: np.ndarray):
        a = np.asfortranarray(a, dtype=np.float64)
        assert a.shape == self.shape, (a.shape, self.shape)
        self.ctx.call("fv3_memcpy_h2d", self, a.ctypes, self.nbytes)
        self.ctx.sync()  # pageable host memory: keep `a` alive until the copy is done
        return self

    def download(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float64, order="F")
        self.ctx.call("fv3_memcpy_d2h", out.ctypes, self, self.nbytes)
        self.ctx.sync()
        return out

    def copy_from(self, other: "DeviceArray"):
        assert other.nbytes == self.nbytes
        self.ctx.call("fv3_memcpy_d2d", self, other, self.nbytes)
        return self

    def zero(self):
        self.ctx.call("fv3_memset", self, 0, self.nbytes)
        return self

    def free(self):
        if self.ptr:
            self.ctx.lib.dll.fv3_free(self)
            self.ptr = None


_NULL = 0     # the address a pointer left out has for the library


def _pp(x):
    """an argument the routine takes as optional: None goes to the library as NULL"""
    return _NULL if x is None else x


def _addressed(args):
    """the arguments again after ctypes refused one: a wrapper takes for an array any object with DeviceArray's .p (a caller's view of
    a level, say), not only one with _as_parameter_.  Whatever has neither is refused again"""
    return [getattr(a, "p", a) for a in args]


class FaceGroup:
    """fv3_group: the faces (contexts) one rank holds, launched together -- every member queues its launches, and when all of them
    have issued the same kernel ONE launch runs them (include/fv3_mi355x.h).  The members share the first member's stream."""

    def __init__(self, ctxs):
        self.lib = ctxs[0].lib
        self.ctxs = list(ctxs)
        self.h = C.c_void_p()
        self.lib.call("fv3_group_create", _handles(self.ctxs), len(self.ctxs), C.byref(self.h))
        for c in self.ctxs:
            c.stream = self.ctxs[0].stream
            c.group = self

    def flush(self):
        self.lib.call("fv3_group_flush", self.h)

    def stats(self):
        """(launches that ran all members at once, launches that ran alone) since the last call"""
        a, b = C.c_long(0), C.c_long(0)
        self.lib.call("fv3_group_stats", self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def close(self):
        if self.h:
            self.lib.call("fv3_group_destroy", self.h)
            self.h = None
            for c in self.ctxs:
                c.group = None


class Context:
    """fv3_ctx: one rank's block of the domain + its gridstruct on the device."""

    def __init__(self, grid: GridStruct, npz: int, lib: Fv3Lib | None = None, stream: int | None = None):
        self.lib = lib or load()
        self.grid = grid
        self.bd: Bounds = grid.bd
        self.npz = npz
        self._buffers: list[DeviceArray] = []
        self.group = None      # lib.FaceGroup this context is a member of
        b = grid.bd
        d = _struct("domain", is_=b.is_, ie=b.ie, js=b.js, je=b.je, ng=b.ng, npx=grid.npx, npy=grid.npy, npz=npz, grid_type=grid.grid_type,
                    do_diss_est=int(grid.do_diss_est), prevent_diss_cooling=int(grid.prevent_diss_cooling),
                    stretched_grid=int(grid.stretched_grid), lim_fac=grid.lim_fac)
        self.h = C.c_void_p()
        self.lib.call("fv3_create", C.byref(d), C.byref(self.h))
        self.stream = 0
        if stream is not None:
            self.set_stream(stream)
        ptrs = [f.name for s in ("fv3_grid_host", "fv3_grid_cubed") for f in abi.STRUCTS[s] if "*" in f.kind]
        keep = {n: np.asfortranarray(grid.m[n], dtype=np.float64) for n in ptrs if n in grid.m}     # alive over the uploads
        m = {n: a.ctypes.data for n, a in keep.items()}
        self.call("fv3_grid_upload", C.byref(_struct("grid_host", m, da_min=grid.da_min, da_min_c=grid.da_min_c)))
        self.geom = int(self.lib.dll.fv3_grid_geom(self.h))  # 0 general, 1 orthogonal, 2 orthogonal + uniform
        if grid.grid_type < 3:      # a face of the cubed sphere: edge weights, rsina, corner extrapolation factors
            opt = dict.fromkeys(("a11", "a12", "a21", "a22", "ec1", "ec2", "en1", "en2"), 0)     # absent from the gridstruct: NULL
            gc = _struct("grid_cubed", {**opt, **m}, corner_f=tuple(np.asarray(grid.m["corner_f"], dtype=np.float64).ravel()))
            self.call("fv3_grid_upload_cubed", C.byref(gc))

    # -- plumbing ------------------------------------------------------------------------------
    def call(self, name: str, *args):
        """Fv3Lib.call of a routine whose first argument is the context (spelled out, not forwarded: the host loop's calls go here)"""
        lib = self.lib
        if None in args:
            lib.refuse(name, (self.h,) + args)
        try:
            rc = lib.fn[name](self.h, *args)
        except C.ArgumentError:
            rc = lib.fn[name](self.h, *_addressed(args))
        if rc:
            lib.check(1, name)

    def _lat(self, lat, who):
        """the latitude of the cell centres on the compute domain (is:ie, js:je); default: the gridstruct's agrid(is:ie, js:je, 2)"""
        if lat is None:
            if "agrid" not in self.grid.m:
                raise Fv3Error(f"{who}: the gridstruct has no agrid")
            b = self.bd
            lat = b.view(np.asarray(self.grid.m["agrid"])[..., 1], "A", b.is_, b.ie, b.js, b.je)
        lat = np.asfortranarray(lat, dtype=np.float64)
        if lat.shape != (self.bd.nx, self.bd.ny):
            raise Fv3Error(f"{who}: lat has the shape {lat.shape}, the compute domain {(self.bd.nx, self.bd.ny)}")
        return lat

    def set_stream(self, stream: int):
        self.stream = int(stream or 0)      # raw hipStream_t of every launch of this context (0 = the null stream)
        self.call("fv3_set_stream", self.stream)

    def sync(self):
        self.call("fv3_sync")

    def empty(self, kind: str, nk: int | None = None) -> DeviceArray:
        return DeviceArray(self, self.bd.shape(kind, nk))

    def zeros(self, kind: str, nk: int | None = None) -> DeviceArray:
        return self.empty(kind, nk).zero()

    def from_host(self, a: np.ndarray) -> DeviceArray:
        return DeviceArray(self, a.shape).upload(a)

    def close(self):
        for b in self._buffers:
            b.free()
        self._buffers.clear()
        if self.h:
            rc = self.lib.dll.fv3_destroy(self.h)   # everything is freed whatever the status
            self.h = None
            self.lib.check(rc, "fv3_destroy")       # FV3_MI355X_POISON: a damaged guard band of a work array

    # -- operators (argument names follow the reference routines) ------------------------------------
    def fv_tp_2d(self, q, crx, cry, hord, fx, fy, xfx, yfx, ra_x=None, ra_y=None, mfx=None, mfy=None, mass=None,
                 nord=-1, damp_c=0.0, nk=None):
        """model/tp_core.F90:85 fv_tp_2d for nk slabs."""
        nk = self.npz if nk is None else nk
        self.call("fv3_fv_tp_2d", nk, q, crx, cry, hord, fx, fy, xfx, yfx, _pp(ra_x), _pp(ra_y), _pp(mfx), _pp(mfy), _pp(mass), nord,
                  damp_c)

    def ppm_line(self, iord, which, h, c, flux, n):
        """xppm / yppm (model/tp_core.F90:324-1152) on one line: h = the line with 3 halo cells either side (device, n + 6), c and flux
        n + 1; which: 0 the tile kernels' operator, 1 / 2 the marching kernels' (along the lanes / register window).  Unit tests only."""
        self.call("fv3_ppm_line", iord, which, h, c, flux, n)

    def c_sw(self, delpc, delp, ptc, pt, u, v, w, uc, vc, ua, va, wc, ut, vt, divg_d, nord, dt2, hydrostatic,
             dord4=True):
        """model/sw_core.F90:79 c_sw over all levels (the k loop of dyn_core.F90:436-447)."""
        self.call("fv3_c_sw", delpc, delp, ptc, pt, u, v, _pp(w), uc, vc, ua, va, _pp(wc), ut, vt, divg_d, nord, dt2, int(hydrostatic),
                  int(dord4))

    def dsw_levels(self, lev: dict):
        keep = {f.name: np.ascontiguousarray(lev[f.name], dtype=np.int32 if "int" in f.kind else np.float64)
                for f in abi.STRUCTS["fv3_dsw_levels"]}
        assert all(a.size == self.npz for a in keep.values())
        self.call("fv3_dsw_levels_upload", C.byref(_struct("dsw_levels", {n: a.ctypes.data for n, a in keep.items()})))

    def d_sw(self, par: dict, delpc, delp, pt, u, v, w, uc, vc, ua, va, divg_d, mfx, mfy, cx, cy, crx, cry, xfx, yfx,
             q_con, delp_out, pt_out, u_out, v_out, w_out, q_con_out, heat_s, diss_e, phase: str = "all"):
        """model/sw_core.F90:494 d_sw over all levels (the k loop of dyn_core.F90:658-812).
        phase: "all", or "interior" (the part that needs no halo of uc, vc, divg_d) followed by "rest"."""
        fn = {"all": "fv3_d_sw", "interior": "fv3_d_sw_interior", "rest": "fv3_d_sw_rest"}[phase]
        self.call(fn, C.byref(_struct("dsw_params", par)), _pp(delpc), delp, pt, u, v, _pp(w), uc, vc, ua, va, divg_d, mfx, mfy, cx, cy, crx,
                  cry, xfx, yfx, _pp(q_con), delp_out, pt_out, u_out, v_out, _pp(w_out), _pp(q_con_out), _pp(heat_s), _pp(diss_e))

    def fv_subgrid_z(self, hydrostatic, nq, nwat, species, k_bot_full, fv_sg_adj, fv_sg_adj_weak, dt, ptop, delp, pe, peln, pkz, ta, qa,
                     ua, va, w, delz, u_dt, v_dt, consts=None):
        """fv_sg_SHiELD (model/fv_sg.F90:76-505) in place on ta, qa(.., 1:nq), ua, va, w; the A-grid wind tendencies into u_dt, v_dt.
        species: {name: 1-based index} of sphum, liq_wat, rainwat, ice_wat, snowwat, graupel (absent = 0); consts: overrides of
        NEG_ADJ_CONSTS (the caller's constants_mod / gfdl_mp_mod values)."""
        pr = _struct("sg_params", {**dict.fromkeys(SG_SPECIES, 0), **(species or {}), **NEG_ADJ_CONSTS, **(consts or {})},
                     hydrostatic=int(bool(hydrostatic)), nq=int(nq), nwat=int(nwat), k_bot_full=int(k_bot_full), fv_sg_adj=int(fv_sg_adj),
                     fv_sg_adj_weak=int(fv_sg_adj_weak), dt=float(dt), ptop=float(ptop))
        self.call("fv3_fv_subgrid_z", C.byref(pr), _pp(delp), _pp(pe), _pp(peln), _pp(pkz), _pp(ta), _pp(qa), _pp(ua), _pp(va), _pp(w),
                  _pp(delz), _pp(u_dt), _pp(v_dt))

    def upload_dwinds(self, m=None):
        """fv3_grid_upload_dwinds: vlon, vlat, es1, ew2, edge_vect_* of the gridstruct (or of the mapping m) -- what
        update_dwinds_phys reads on the sphere.  Once per context."""
        m = self.grid.m if m is None else m
        keep = {}
        for f in abi.STRUCTS["fv3_grid_dwinds"]:
            if f.name not in m:
                raise Fv3Error(f"upload_dwinds: the gridstruct has no {f.name}")
            keep[f.name] = np.asfortranarray(m[f.name], dtype=np.float64)
        self.call("fv3_grid_upload_dwinds", C.byref(_struct("grid_dwinds", {n: a.ctypes.data for n, a in keep.items()})))
        self.dwinds_ready = True

    def update_dwinds_phys(self, dt, u_dt, v_dt, u, v):
        """update_dwinds_phys (model/fv_grid_utils.F90:3291-3475): u, v += the A-grid tendencies u_dt, v_dt (halo updated) on the D grid.
        On the sphere the geometry is uploaded on first use."""
        if self.grid.grid_type < 3 and not getattr(self, "dwinds_ready", False):
            self.upload_dwinds()
        self.call("fv3_update_dwinds_phys", dt, _pp(u_dt), _pp(v_dt), _pp(u), _pp(v))

    def fv_update_phys(self, dt, ptop, hydrostatic, nq, ncnst, nwat, species, u_dt, v_dt, t_dt, q_dt, delp, pt, q, qdiag, ua, va, w, delz,
                       ps, pe, peln, pk, pkz, u_srf, v_srf, phys_hydrostatic=True, gfs_phys=False, adjust_mass=None, tau_h2o=0.0, ak=None,
                       bk=None, consts=None):
        """fv_update_phys (model/fv_update_phys.F90:67-767), the column part, in place: the physics tendencies t_dt, q_dt (no halo; q_dt may
        be None), u_dt, v_dt added to the state, the air mass and the mixing ratios adjusted for the change in water, pe / peln / pk / ps
        (pkz when hydrostatic) and u_srf / v_srf rebuilt.  The caller goes on with the halo update of u_dt, v_dt and update_dwinds_phys.
        species: {name: 1-based index} of sphum, liq_wat, rainwat, ice_wat, snowwat, graupel, cld_amt, w_diff (absent = 0); adjust_mass:
        ncnst flags (default: all true); consts: overrides of NEG_ADJ_CONSTS and kappa."""
        am = np.ascontiguousarray(np.ones(max(int(ncnst), 1)) if adjust_mass is None else adjust_mass, dtype=np.int32)
        if am.size < ncnst:
            raise Fv3Error(f"fv_update_phys: adjust_mass has {am.size} flags for ncnst = {ncnst} tracers")
        keep = {n: np.ascontiguousarray(a, dtype=np.float64) for n, a in (("ak", ak), ("bk", bk)) if a is not None}
        for n, a in keep.items():
            if a.size != self.npz + 1:
                raise Fv3Error(f"fv_update_phys: {n} has {a.size} values for npz + 1 = {self.npz + 1}")
        pr = _struct("update_phys_params", {**dict.fromkeys(SG_SPECIES + ("cld_amt", "w_diff", "ak", "bk"), 0), **(species or {}),
                                            **NEG_ADJ_CONSTS, "kappa": KAPPA, **(consts or {}), **{n: a.ctypes.data for n, a in keep.items()}},
                     hydrostatic=int(bool(hydrostatic)), phys_hydrostatic=int(bool(phys_hydrostatic)), gfs_phys=int(bool(gfs_phys)),
                     nq=int(nq), ncnst=int(ncnst), nwat=int(nwat), adjust_mass=am.ctypes.data, dt=float(dt), ptop=float(ptop),
                     tau_h2o=float(tau_h2o))
        self.call("fv3_fv_update_phys", C.byref(pr), _pp(u_dt), _pp(v_dt), _pp(t_dt), _pp(q_dt), _pp(delp), _pp(pt), _pp(q), _pp(qdiag),
                  _pp(ua), _pp(va), _pp(w), _pp(delz), _pp(ps), _pp(pe), _pp(peln), _pp(pk), _pp(pkz), _pp(u_srf), _pp(v_srf))

    def upload_lat(self, lat=None):
        """fv3_grid_upload_lat: the latitude of the cell centres on the compute domain, agrid(is:ie, js:je, 2) -- what Held_Suarez_Tend
        reads of the gridstruct.  Default: the gridstruct's agrid (A x 2, as cubed_sphere.py forms it).  Once per context."""
        self.call("fv3_grid_upload_lat", self._lat(lat, "upload_lat").ctypes)
        self.lat_ready = True

    def held_suarez_tend(self, pdt, delp, peln, pe, pkz, pt, ua, va, u_dt, v_dt, t_dt, strat=True, zurita=False, rd_zur=1.0 / 25.0,
                         fresh=False, radius=6.3712e6, pi=3.14159265358979323846):
        """Held_Suarez_Tend (driver/solo/hswf.F90:41-207): the Held-Suarez forcing added to t_dt (is:ie, js:je, npz; no halo) and, where
        the bottom friction acts, to u_dt, v_dt (A x npz).  fresh: the incoming tendencies are taken as zero, not read, and every cell
        of the three on the compute domain is written.  radius: fv_arrays_mod's (scaled for a small earth); pi: constants_mod's.  The
        latitude table is uploaded from the gridstruct on first use."""
        if not getattr(self, "lat_ready", False):
            self.upload_lat()
        pr = _struct("held_suarez_params", pdt=float(pdt), strat=int(bool(strat)), zurita=int(bool(zurita)), rd_zur=float(rd_zur),
                     fresh=int(bool(fresh)), radius=float(radius), pi=float(pi))
        self.call("fv3_held_suarez_tend", C.byref(pr), _pp(delp), _pp(peln), _pp(pe), _pp(pkz), _pp(pt), _pp(ua), _pp(va), _pp(u_dt),
                  _pp(v_dt), _pp(t_dt))

    def age_of_air(self, km, time, pe, q):
        """age_of_air (driver/solo/hswf.F90:209-245): the age tracer q (ONE tracer, A x km) zeroed when time < 1e-6, else set to
        5e-6 / 60 * time where pe(i, k, j) >= 75000 Pa"""
        self.call("fv3_age_of_air", int(km), float(time), _pp(pe), _pp(q))

    def grid_upload_reed(self, reed_test=0, lat=None, consts=None):
        """fv3_grid_upload_reed: Tsurf and the SST factor of qsats (driver/solo/fv_phys.F90:2571-2586, :2719) on the compute domain, formed
        on the host from the latitude of the cell centres, agrid(is:ie, js:je, 2), for one reed_test.  Default: the gridstruct's agrid.
        consts: overrides of REED_CONSTS."""
        self.call("fv3_grid_upload_reed", self._lat(lat, "grid_upload_reed").ctypes, int(reed_test),
                  C.byref(_consts("reed_consts", REED_CONSTS, consts)))
        self.reed_ready = int(reed_test)

    def grid_download_reed(self):
        """fv3_grid_download_reed -> (Tsurf, the SST factor of qsats), each (is:ie, js:je), as fv3_grid_upload_reed formed them"""
        tab = np.zeros((self.bd.nx, self.bd.ny, 2), order="F")
        self.call("fv3_grid_download_reed", tab.ctypes)
        return np.asfortranarray(tab[..., 0]), np.asfortranarray(tab[..., 1])

    def reed_sim_phys(self, pdt, delp, pt, ua, va, q, pe, peln, phis, delz, u_dt, v_dt, t_dt, q_dt, rain, hydrostatic=True, reed_test=0,
                      do_reed_cond=True, reed_cond_only=False, reed_alt_mxg=False, fresh=False, consts=None):
        """the column loop of do_reed_sim_phys with reed_sim_physics inside it (driver/solo/fv_phys.F90:551-602, :2332-2817): the
        tendencies of the Reed-Jablonowski simple physics added to u_dt, v_dt (A x npz), t_dt and q_dt, the sphum plane of the
        tendency array (is:ie, js:je, npz; no halo); rain (is:ie, js:je) is written with do_reed_cond.  q: the sphum tracer (A x npz);
        delz may be None when hydrostatic.  fresh: the incoming tendencies are taken as zero, not read, and every cell of the four
        on the compute domain is written.  The table is uploaded from the gridstruct on first use of a reed_test."""
        if getattr(self, "reed_ready", None) is None:
            self.grid_upload_reed(reed_test, consts=consts)
        pr = _struct("reed_params", pdt=float(pdt), hydrostatic=int(bool(hydrostatic)), reed_test=int(reed_test),
                     do_reed_cond=int(bool(do_reed_cond)), reed_cond_only=int(bool(reed_cond_only)), reed_alt_mxg=int(bool(reed_alt_mxg)),
                     fresh=int(bool(fresh)), k=_consts("reed_consts", REED_CONSTS, consts))
        self.call("fv3_reed_sim_phys", C.byref(pr), _pp(delp), _pp(pt), _pp(ua), _pp(va), _pp(q), _pp(pe), _pp(peln), _pp(phis), _pp(delz),
                  _pp(u_dt), _pp(v_dt), _pp(t_dt), _pp(q_dt), _pp(rain))

    def qs_wat_init(self, consts=None):
        """fv3_qs_wat_init: table_w and des_w of qs_tables_mod (driver/solo/qs_tables.F90:95-132), formed on the host and uploaded.
        consts: overrides of KESSLER_CONSTS."""
        k = _consts("kessler_consts", KESSLER_CONSTS, consts)
        self.call("fv3_qs_wat_init", C.byref(k))
        self.qs_wat_ready = tuple(getattr(k, n) for n, _ in k._fields_)

    def qs_wat_download(self):
        """fv3_qs_wat_download -> (table_w, des_w), 2621 each, as fv3_qs_wat_init formed them"""
        tw, dw = np.zeros(QS_LENGTH), np.zeros(QS_LENGTH)
        self.call("fv3_qs_wat_download", tw.ctypes, dw.ctypes)
        return tw, dw

    def k_warm_rain(self, pdt, ua, va, w, u_dt, v_dt, q, pt, delp, delz, pe, peln, pk, ps, rain, nq, sphum=1, liq_wat=2, rainwat=3, K_cycle=0,
                    K_sedi_transport=False, do_K_sedi_w=False, do_K_sedi_heat=False, hydrostatic=False, moist_kappa=False, consts=None):
        """K_warm_rain with kessler_imp inside it (driver/solo/fv_phys.F90:1992-2291): the Kessler warm-rain microphysics on the state in
        place.  q: the whole tracer array (A x npz x nq); sphum, liq_wat, rainwat: 1-based planes of it.  pt is the temperature.  rain
        (is:ie, js:je) is written in every cell [kg/dA].  K_cycle = 0: max(1, nint(pdt/30.)).  delz may be None when hydrostatic without
        do_K_sedi_heat, w unless K_sedi_transport and do_K_sedi_w.  The table is formed on first use, or when the constants change."""
        k = _consts("kessler_consts", KESSLER_CONSTS, consts)
        if getattr(self, "qs_wat_ready", None) != tuple(getattr(k, n) for n, _ in k._fields_):
            self.qs_wat_init(consts)
        pr = _struct("kessler_params", pdt=float(pdt), K_cycle=int(K_cycle), K_sedi_transport=int(bool(K_sedi_transport)),
                     do_K_sedi_w=int(bool(do_K_sedi_w)), do_K_sedi_heat=int(bool(do_K_sedi_heat)), hydrostatic=int(bool(hydrostatic)),
                     moist_kappa=int(bool(moist_kappa)), nq=int(nq), sphum=int(sphum), liq_wat=int(liq_wat), rainwat=int(rainwat), k=k)
        self.call("fv3_k_warm_rain", C.byref(pr), _pp(ua), _pp(va), _pp(w), _pp(u_dt), _pp(v_dt), _pp(q), _pp(pt), _pp(delp), _pp(delz),
                  _pp(pe), _pp(peln), _pp(pk), _pp(ps), _pp(rain))

    def grid_upload_terminator(self, agrid=None, pi=REED_CONSTS["pi"]):
        """fv3_grid_upload_terminator: k1 of DCMIP2016_terminator_advance (driver/solo/fv_phys.F90:2873) over the A layout, formed on the
        host from agrid (A x 2: longitude, latitude).  Default: the gridstruct's agrid."""
        if agrid is None:
            if "agrid" not in self.grid.m:
                raise Fv3Error("grid_upload_terminator: the gridstruct has no agrid")
            agrid = self.grid.m["agrid"]
        agrid = np.asfortranarray(agrid, dtype=np.float64)
        if agrid.shape != self.bd.shape("A") + (2,):
            raise Fv3Error(f"grid_upload_terminator: agrid has the shape {agrid.shape}, the A layout x 2 is {self.bd.shape('A') + (2,)}")
        self.call("fv3_grid_upload_terminator", agrid.ctypes, float(pi))
        self.terminator_ready = True

    def grid_download_terminator(self):
        """fv3_grid_download_terminator -> k1 over the A layout, as fv3_grid_upload_terminator formed it"""
        k1 = np.zeros(self.bd.shape("A"), order="F")
        self.call("fv3_grid_download_terminator", k1.ctypes)
        return k1

    def terminator_advance(self, km, pdt, cl, cl2, term_fill_negative=False):
        """DCMIP2016_terminator_advance (driver/solo/fv_phys.F90:2819-2894) on the tracer planes Cl and Cl2 (A x km each), halo included.
        The k1 plane is uploaded from the gridstruct on first use."""
        if not getattr(self, "terminator_ready", False):
            self.grid_upload_terminator()
        self.call("fv3_terminator_advance", int(km), float(pdt), int(bool(term_fill_negative)), _pp(cl), _pp(cl2))

    def interpolate_vertical(self, km, plev, peln, a3, a2, in_ng=0):
        """interpolate_vertical (tools/fv_diagnostics.F90:4910-4948): a2 (is:ie, js:je) = a3 (km layers) at the pressure plev [Pa], linear
        in the layer-mean log pressure of peln (is:ie, km+1, js:je).  in_ng: 0 = a3 on the compute domain, ng = a state field with halo"""
        self.call("fv3_interpolate_vertical", km, plev, _pp(peln), _pp(a3), in_ng, _pp(a2))

    def profile(self, enable: bool):
        self.call("fv3_profile", int(enable))

    def profile_report(self) -> dict:
        """{label: (count, total_ms)} measured with HIP events on the launch stream."""
        return self._report("fv3_profile_report")

    def profile_report_timers(self) -> dict:
        """the same events under the reference's timing_on / timing_off names: {timer: (count, total_ms)}"""
        return self._report("fv3_profile_report_timers")

    def _report(self, routine):
        buf = C.create_string_buffer(1 << 16)
        self.call(routine, buf, len(buf))
        return {name: (int(n), float(ms)) for name, n, ms in map(str.split, buf.value.decode().splitlines())}

    def prt_maxmin(self, q, fac=1.0):
        """prt_mxm (tools/fv_diagnostics.F90:4265-4313) of an A-kind field: (max, min, area mean of the last level), times fac"""
        out = (C.c_double * 3)()
        nk = q.shape[2] if len(q.shape) > 2 else 1
        self.call("fv3_prt_maxmin", q, nk, fac, out)
        return float(out[0]), float(out[1]), float(out[2])

    # -- nonhydrostatic column path -------------------------------------------------------------------
    def set_dp_ref(self, dp0):
        a = np.ascontiguousarray(dp0, dtype=np.float64)
        assert a.size == self.npz
        self.call("fv3_set_dp_ref", a.ctypes)

    def update_dz_c(self, dt, zs, ut, vt, gz_in, gz, ws):
        """model/nh_utils.F90:59 update_dz_c"""
        self.call("fv3_update_dz_c", dt, zs, ut, vt, gz_in, gz, ws)

    def riem_solver_c(self, dt, cn, hs, w3, pt, delp, gz, pef, ws):
        """model/nh_utils.F90:323 Riem_Solver_c"""
        self.call("fv3_riem_solver_c", dt, C.byref(_struct("nh_consts", cn, default=0)), hs, w3, pt, delp, gz, pef, ws)

    def update_dz_d(self, hord, zs, zh_in, zh_out, crx, cry, xfx, yfx, ws, rdt):
        """model/nh_utils.F90:204 update_dz_d"""
        self.call("fv3_update_dz_d", hord, zs, zh_in, zh_out, crx, cry, xfx, yfx, ws, rdt)

    def set_fast_tau_w(self, rff=None):
        """fast_tau_w_sec > 0: rff(1:k_rf) of nh_utils.F90:356-367 (host array; None / empty = off) for the following Riemann solver calls"""
        rff = np.ascontiguousarray(rff if rff is not None else [], dtype=np.float64)
        self.call("fv3_set_fast_tau_w", len(rff), rff.ctypes if len(rff) else _NULL)

    def set_ray_fast(self, kmax, k_rf, dm, rf, dp):
        """what Ray_fast keeps from its first call (dyn_core.F90:2519-2545): rf(1:kmax), dp_ref(1:npz), k_rf, dm"""
        rf = np.ascontiguousarray(rf, dtype=np.float64)
        dp = np.ascontiguousarray(dp, dtype=np.float64)
        self.call("fv3_set_ray_fast", int(kmax), int(k_rf), dm, rf.ctypes, dp.ctypes)

    def ray_fast(self, u, v, w, hydrostatic):
        """Ray_fast (dyn_core.F90:2549-2597) on the compute domain; w may be None when hydrostatic"""
        self.call("fv3_ray_fast", u, v, _pp(w), int(hydrostatic))

    def mix_dp(self, hydrostatic, w, delp, pt):
        """mix_dp (dyn_core.F90:2119-2200; flagstruct%fill_dp, :820): thin layers borrow mass from their neighbour, pt and w mixed; in place"""
        self.call("fv3_mix_dp", int(hydrostatic), _pp(w), delp, pt)

    def set_condensate(self, q_con=None, cappa=None):
        """use_cond / moist_kappa arrays of the following riem_solver_c / riem_solver3 calls (None = .false.)"""
        self.call("fv3_set_condensate", _pp(q_con), _pp(cappa))

    def riem_solver3(self, dt, cn, zs, w, delz, pt, delp, zh, pe, ppe, pk3, pk, peln, ws, use_logp=False,
                     last_call=False, fp_out=False):
        """model/nh_core.F90:47 Riem_Solver3"""
        self.call("fv3_riem_solver3", dt, C.byref(_struct("nh_consts", cn, default=0)), zs, w, delz, pt, delp, zh, _pp(pe), ppe, pk3, _pp(pk),
                  _pp(peln), ws, int(use_logp), int(last_call), int(fp_out))

    def p_grad_c(self, dt2, delpc, pkc, gz, uc, vc, hydrostatic):
        """model/dyn_core.F90:1635 p_grad_c"""
        self.call("fv3_p_grad_c", dt2, delpc, pkc, gz, uc, vc, int(hydrostatic))

    def nh_p_grad(self, u, v, pp, gz, delp, pk, dt, top_value, gz_scale=1.0):
        """model/dyn_core.F90:1697 nh_p_grad (gz_scale: read gz*gz_scale, fusing gz = zh*grav of :982-989)"""
        self.call("fv3_nh_p_grad", u, v, pp, gz, gz_scale, delp, pk, dt, top_value)

    def zh_from_delz(self, zs, delz, zh):
        self.call("fv3_zh_from_delz", zs, delz, zh)

    def pk3_halo(self, ptop, akap, pk3, delp, use_logp=False):
        self.call("fv3_pk3_halo", ptop, akap, pk3, delp, int(use_logp))

    def pe_halo(self, ptop, pe, delp):
        self.call("fv3_pe_halo", ptop, pe, delp)

    def geopk(self, ptop, akap, cp_air, pe, peln, delp, pk, gz, hs, pt, pkz, CG):
        """model/dyn_core.F90:2202 geopk"""
        self.call("fv3_geopk", ptop, akap, cp_air, ptop ** akap, _pp(pe), _pp(peln), delp, pk, gz, hs, pt, _pp(pkz), int(CG))

    # -- vertical remap ---------------------------------------------------------------------------------
    def set_ak_bk(self, ak, bk):
        a = np.ascontiguousarray(ak, dtype=np.float64)
        b = np.ascontiguousarray(bk, dtype=np.float64)
        assert a.size == self.npz + 1 and b.size == self.npz + 1
        self.call("fv3_set_ak_bk", a.ctypes, b.ctypes)

    def set_moist(self, par: dict | None, q_con=None, cappa=None):
        """moist_kappa / use_cond branches of the remap (fv_mapz.F90:212-219, :463-478, :806-811); None = off"""
        if par is None:
            self.call("fv3_set_moist", _NULL, _NULL, _NULL)
            return
        self.call("fv3_set_moist", C.byref(_struct("moist_params", par, default=0)), _pp(q_con), _pp(cappa))

    def lagrangian_to_eulerian(self, par: dict, ps, pe, delp, pkz, pk, u, v, w, delz, pt, q, peln, omga, ws):
        """model/fv_mapz.F90:56 Lagrangian_to_Eulerian"""
        s = _struct("remap_params", par, fill=int(par.get("fill", 0)))
        kt = np.ascontiguousarray(par.get("kord_tr", []), dtype=np.int32)
        self.call("fv3_lagrangian_to_eulerian", C.byref(s), kt.ctypes if kt.size else _NULL, ps, pe, delp, pkz, pk, u, v,
                  _pp(w), _pp(delz), pt, _pp(q), peln, omga, _pp(ws))

    @staticmethod
    def _remap_params(par: dict):
        return _struct("remap_params", par, last_step=par.get("last_step", 0), fill=int(par.get("fill", 0)))

    # -- consv_te: compute_total_energy (fv_thermodynamics.F90:90) and the energy fixer of the last remap (fv_mapz.F90:643-821)
    def compute_total_energy(self, par: dict, moist_phys, u, v, w, delz, pt, delp, q, qc, pe, peln, phis, te_2d):
        s = self._remap_params(par)
        self.call("fv3_compute_total_energy", C.byref(s), int(moist_phys), u, v, _pp(w), _pp(delz), pt, delp, _pp(q), _pp(qc), _pp(pe),
                  _pp(peln), phis, te_2d)

    def energy_fixer_sums(self, par: dict, only_sums, u, v, w, delz, pt, delp, q, pe, peln, phis, pkz, pk, te0_2d, te_2d, zsum1,
                          zsum0):
        s = self._remap_params(par)
        self.call("fv3_energy_fixer_sums", C.byref(s), int(only_sums), u, v, _pp(w), _pp(delz), pt, delp, _pp(q), _pp(pe), _pp(peln), phis,
                  pkz, _pp(pk), _pp(te0_2d), _pp(te_2d), zsum1, _pp(zsum0))

    def ordered_sum(self, values) -> float:
        """g_sum(..., reproduce=.true.) of host values over the ranks of the context's communicator (fv3_ordered_sum)"""
        a = np.ascontiguousarray(values, dtype=np.float64).ravel()
        out = C.c_double(0.0)
        self.call("fv3_ordered_sum", a.ctypes, a.size, C.byref(out))
        return out.value

    def remap_finish(self, par: dict, dtmp, pt, pkz, q):
        s = self._remap_params(par)
        self.call("fv3_remap_finish", C.byref(s), dtmp, pt, pkz, _pp(q))

    # -- tracer_2d ---------------------------------------------------------------------------------------
    def tracer_2d_prep(self, q_split, cx, cy, xfx, yfx) -> np.ndarray:
        cmax = np.zeros(self.npz)
        self.call("fv3_tracer_2d_prep", q_split, cx, cy, xfx, yfx, cmax.ctypes)
        return cmax

    def tracer_2d_scale(self, frac, cx, xfx, mfx, cy, yfx, mfy):
        f = np.ascontiguousarray(frac, dtype=np.float64)
        self.call("fv3_tracer_2d_scale", f.ctypes, cx, xfx, mfx, cy, yfx, mfy)

    def tracer_2d_step(self, it, nsplt, ksplt, nq, hord, nord_tr, trdm, q, q_out, dp1, dp1_out, mfx, mfy, cx, cy, xfx, yfx):
        ks = np.ascontiguousarray(ksplt, dtype=np.int32)
        self.call("fv3_tracer_2d_step", it, nsplt, ks.ctypes, nq, hord, nord_tr, trdm, q, q_out, dp1, dp1_out, mfx, mfy, cx, cy, xfx, yfx)

    def set_remap_te(self, on, hs=None, te=None):
        """flagstruct%remap_te (fv_mapz.F90:232-286, :348-360, :576-619): hs = phis (A), te: A x npz work array"""
        self.call("fv3_set_remap_te", int(bool(on)), hs if on else _NULL, te if on else _NULL)

    def d_sw_inline_q(self, nq, hord_tr, nord_t, damp_t, q, q_out, delp_old, delp_new, fx, fy, crx, cry, xfx, yfx):
        """sw_core.F90:1020-1043: the tracers of one acoustic substep (after d_sw of the same substep, see the header)"""
        self.call("fv3_d_sw_inline_q", nq, hord_tr, nord_t, damp_t, q, q_out, delp_old, delp_new, fx, fy, crx, cry, xfx, yfx)

    def flux_accum(self, mfx, mfy, fx, fy):
        self.call("fv3_flux_accum", mfx, mfy, fx, fy)

    def fill2d_mass(self, nk, q, delp, qt, q_offset=0):
        """fv_fill.F90:228-235; q_offset: element offset of the tracer inside an A x npz x nq array"""
        self.call("fv3_fill2d_mass", nk, q.ptr + 8 * q_offset, delp, qt)

    def fill2d_apply(self, nk, qt, delp, q, q_offset=0):
        """fv_fill.F90:238-256"""
        self.call("fv3_fill2d_apply", nk, qt, delp, q.ptr + 8 * q_offset)

    def neg_adj3(self, hydrostatic, peln, delz, delp, pt, q, species=(1, 2, 3, 4, 5, 6), qa=0, consts=None):
        """neg_adj3 (fv_sg.F90:968-1335; fv_dynamics.F90:722-745) in place on pt (= T) and the tracer array q (A x npz x nq).
        species: the 1-based tracer indices of sphum, liq_wat, rainwat, ice_wat, snowwat, graupel; qa: that of cld_amt, 0 = absent;
        consts: overrides of NEG_ADJ_CONSTS"""
        pr = _struct("neg_adj_params", {**NEG_ADJ_CONSTS, **(consts or {})}, hydrostatic=int(bool(hydrostatic)))
        n3 = int(np.prod(q.shape[:3]))
        nq = q.shape[3] if len(q.shape) > 3 else 1
        if any(not 1 <= int(s) <= nq for s in species) or len(set(species)) != 6 or not 0 <= int(qa) <= nq:
            raise Fv3Error(f"neg_adj3: species {tuple(species)} / cld_amt {qa} are not six distinct tracers of 1..{nq}")
        sp = [q.ptr + 8 * n3 * (int(s) - 1) for s in species]
        qap = q.ptr + 8 * n3 * (int(qa) - 1) if qa else _NULL
        self.call("fv3_neg_adj3", C.byref(pr), _pp(peln), _pp(delz), delp, pt, *sp, qap)

    def omga_update(self, rdt, ptop, pe, delp_before, omga):
        """dyn_core.F90:1182-1191: omga = (pe - pem)*rdt on the last substep (local part, see the header)"""
        self.call("fv3_omga_update", rdt, ptop, pe, delp_before, omga)

    def pt_to_theta_v(self, hydrostatic, zvir, kappa, rdgas, grav, pt, delp, delz, qv, pkz):
        """fv_dynamics.F90:284-329, :379-399: T -> theta_v before the k_split loop"""
        self.call("fv3_pt_to_theta_v", int(hydrostatic), zvir, kappa, rdgas, grav, pt, _pp(delp), _pp(delz), _pp(qv), pkz)

    def c2l(self, c2l_ord, u, v, ua, va):
        """cubed_to_latlon (fv_grid_utils.F90:2319), grid_type = 4 branches; ord 4 needs the halo of u, v"""
        self.call("fv3_c2l", int(c2l_ord), u, v, ua, va)

    def rayleigh_u2f(self, kmax, hydrostatic, u, v, w, ua, va, u2f):
        """Rayleigh_Friction up to the halo update of u2f (fv_dynamics.F90:1186-1205)"""
        self.call("fv3_rayleigh_u2f", int(kmax), int(hydrostatic), u, v, _pp(w), ua, va, u2f)

    def rayleigh_apply(self, kmax, conserve, hydrostatic, cp, rg, ptop, pm, rf, u2f, pt, delz, u, v, w):
        """Rayleigh_Friction after the halo update of u2f (fv_dynamics.F90:1211-1260); pm, rf: host arrays"""
        pm = np.ascontiguousarray(pm, dtype=np.float64)
        rf = np.ascontiguousarray(rf, dtype=np.float64)
        self.call("fv3_rayleigh_apply", int(kmax), int(conserve), int(hydrostatic), cp, rg, ptop, pm.ctypes, rf.ctypes, u2f, pt, _pp(delz),
                  u, v, _pp(w))

    def rayleigh_super(self, kmax, conserve, hydrostatic, cp, rg, ptop, pm, rf, ua, va, pt, u, v, w, u00=None, v00=None):
        """Rayleigh_Super after cubed_to_latlon (fv_dynamics.F90:1044-1121; grid_type < 4); pm, rf: host arrays"""
        pm = np.ascontiguousarray(pm, dtype=np.float64)
        rf = np.ascontiguousarray(rf, dtype=np.float64)
        self.call("fv3_rayleigh_super", int(kmax), int(conserve), int(hydrostatic), cp, rg, ptop, pm.ctypes, rf.ctypes, ua, va, pt, u, v,
                  _pp(w), _pp(u00), _pp(v00))

    def compute_aam(self, radius, omega, agrav, ptop, coslat, ua, delp, aam, m_fac, ps):
        """compute_aam (fv_dynamics.F90:1266-1314) after c2l(2, ...): aam, m_fac (CC), ps (A)"""
        self.call("fv3_compute_aam", radius, omega, agrav, ptop, coslat, ua, delp, aam, m_fac, ps)

    def consv_am_apply(self, u00, l2c_u, l2c_v, u, v):
        """fv_dynamics.F90:784-798: u += u00 l2c_u, v += u00 l2c_v"""
        self.call("fv3_consv_am_apply", u00, l2c_u, l2c_v, u, v)

    def adv_pe(self, ptop, ua, va, delp_before, omga):
        """adv_pe (dyn_core.F90:1195, :1529-1632): the advective term of omega on a cubed-sphere face"""
        self.call("fv3_adv_pe", ptop, ua, va, delp_before, omga)

    # ---- hydrostatic pressure gradient (dyn_core.F90:828-848, :1021, :1001-1010) ------------------------------------
    def divg2_ext(self, d_ext, delp, vt, divg2):
        self.call("fv3_divg2_ext", d_ext, delp, vt, divg2)

    def split_p_grad(self, u, v, pp, gz, delp, pk, beta, dt, top_value, du, dv, gz_scale=1.0):
        """model/dyn_core.F90:1795 split_p_grad (beta: the caller's beta_d; du, dv: U / V x npz, zero before the first call)"""
        self.call("fv3_split_p_grad", u, v, pp, gz, gz_scale, delp, pk, beta, dt, top_value, du, dv)

    def grad1_p_update(self, divg2, u, v, pk, gz, dt, ptk, beta, du, dv):
        """model/dyn_core.F90:2033 grad1_p_update (divg2 None: zeros)"""
        self.call("fv3_grad1_p_update", _pp(divg2), u, v, pk, gz, dt, ptk, beta, du, dv)

    def one_grad_p(self, u, v, pk, gz, divg2, dt, ptk):
        self.call("fv3_one_grad_p", u, v, pk, gz, _pp(divg2), dt, ptk)

    def one_grad_p_nh(self, u, v, pk, gz, divg2, delp, dt, ptop, gz_scale=1.0):
        """one_grad_p of the nonhydrostatic loop (beta < -0.1, dyn_core.F90:1029-1030): pk = the full pressure"""
        self.call("fv3_one_grad_p_nh", u, v, pk, gz, _pp(divg2), delp, dt, ptop, gz_scale)

    def copy_a_to_cc(self, src, dst):
        nk = int(np.prod(src.shape[2:])) if len(src.shape) > 2 else 1
        self.call("fv3_copy_a_to_cc", src, dst, nk)

    # ---- dissipative heating after the substep loop (dyn_core.F90:798-803, :1300-1355) ---------------------------
    def heat_source_accum(self, heat_source, heat_s):
        self.call("fv3_heat_source_accum", heat_source, heat_s)

    def del2_cubed(self, q, cd: float, nmax: int):
        nk = int(np.prod(q.shape[2:])) if len(q.shape) > 2 else 1
        self.call("fv3_del2_cubed", q, nk, cd, nmax)

    def apply_heat_source(self, n_con, hydrostatic, bdt, delt_max, cp_air, cv_air, rdgas, grav, pt, heat_source, delp, delz,
                          pkz):
        self.call("fv3_apply_heat_source", n_con, int(hydrostatic), bdt, delt_max, cp_air, cv_air, rdgas, grav, pt, heat_source, delp,
                  _pp(delz), pkz)

    # ---- multi-rank halo exchange: pack / unpack (the transfers are halo.py's) ---------------------------
    def _halo_fields(self, fields):
        arr = (HaloField * len(fields))()
        for n, (dev, kind) in enumerate(fields):
            arr[n].field = dev.ptr
            arr[n].kind = {"A": 0, "U": 1, "V": 2, "B": 3}[kind]
            arr[n].nk = int(np.prod(dev.shape[2:])) if len(dev.shape) > 2 else 1
        return arr

    def halo_message_elems(self, fields):
        out = (C.c_size_t * 8)()
        self.call("fv3_halo_message_elems", len(fields), self._halo_fields(fields), out)
        return [int(v) for v in out]

    def halo_pack(self, fields, bufs):
        ptrs = (C.c_void_p * 8)(*[b.ptr for b in bufs])
        self.call("fv3_halo_pack", len(fields), self._halo_fields(fields), ptrs)

    def halo_periodic_group(self, fields):
        """one rank, doubly periodic: the halos of the group from its own opposite edges in one launch"""
        self.call("fv3_halo_periodic_group", len(fields), self._halo_fields(fields))

    def halo_unpack(self, fields, bufs):
        ptrs = (C.c_void_p * 8)(*[b.ptr for b in bufs])
        self.call("fv3_halo_unpack", len(fields), self._halo_fields(fields), ptrs)

    # -- the exchange behind the C ABI (RCCL owned by the context): what a Fortran host without an RCCL binding uses ----------
    def comm_init(self, rank: int, nranks: int, unique_id: bytes | None = None) -> bytes:
        """fv3_comm_init; rank 0 of a one-rank run may leave unique_id out.  Returns the id used."""
        if unique_id is None:
            buf = (C.c_ubyte * 128)()
            self.lib.call("fv3_comm_get_unique_id", buf)
            unique_id = bytes(buf)
        self.call("fv3_comm_init", rank, nranks, (C.c_ubyte * 128)(*unique_id))
        return unique_id

    def halo_start(self, fields, to, frm):
        """start_group_halo_update: to[d] / frm[d] = the ranks at offsets d / -d, halo.DIRECTIONS order"""
        self.call("fv3_halo_start", len(fields), self._halo_fields(fields), (C.c_int * 8)(*to), (C.c_int * 8)(*frm))

    def halo_complete(self):
        self.call("fv3_halo_complete")

    def allreduce_max(self, a: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float64).copy()
        self.call("fv3_allreduce_max", a.ctypes, a.size)
        return a

    def halo_fill_periodic(self, field: DeviceArray, kind: str):
        code = {"A": 0, "U": 1, "V": 2, "B": 3}[kind]
        nk = int(np.prod(field.shape[2:])) if len(field.shape) > 2 else 1
        self.call("fv3_halo_fill_periodic", field, code, nk)
