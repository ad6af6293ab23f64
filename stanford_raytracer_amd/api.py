"""Host-side mirror of the reference's interface for the hot path, over the C ABI (include/srt.h).

Names follow the reference: a *model* is what `--modelnum` selects and `setup()` builds
(raytracer_driver.f95:256-770); `plasma_params` is `funcPlasmaParams` (raytracer.f95:121-129);
`trace` is the driver's ray loop around `raytracer_run` (raytracer_driver.f95:1144-1232).
The library is HIP-only: importing works anywhere, but every call needs an MI355X and raises
`SrtError` otherwise -- there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

ROW = 20
STOP_NAMES = {0: "tmax", 1: "minalt", 2: "k=0", 3: "vgroup", 5: "dt", 6: "maxsteps", 9: "numeric"}


class SrtError(RuntimeError):
    pass


class Params(C.Structure):
    """srt_params: scalar arguments of raytracer_run + the driver's outputper."""
    _fields_ = [("dt0", C.c_double), ("dtmax", C.c_double), ("tmax", C.c_double), ("maxerr", C.c_double),
                ("minalt", C.c_double), ("del_", C.c_double), ("maxsteps", C.c_int32), ("root", C.c_int32),
                ("fixedstep", C.c_int32), ("outputper", C.c_int32), ("first_attempt_policy", C.c_int32),
                ("refill_threshold", C.c_int32), ("ray_order", C.c_int32)]


def make_params(dt0=1e-3, dtmax=0.1, tmax=1.0, maxerr=5e-4, minalt=6371.2e3 + 100e3, del_=1e-6, maxsteps=2000,
                root=2, fixedstep=0, outputper=1, first_attempt_policy=0, refill_threshold=0, ray_order=0):
    return Params(dt0, dtmax, tmax, maxerr, minalt, del_, maxsteps, root, fixedstep, outputper,
                  first_attempt_policy, refill_threshold, ray_order)


_lib = None
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)


class SamplerParams(C.Structure):
    """srt_sampler_params of include/srt.h (the flags of gcpm_dens_model_buildgrid_random.f95:56-90)."""
    _fields_ = [("bounds", C.c_double * 6), ("n_zero_altitude", C.c_int64), ("n_iri_pad", C.c_int64),
                ("n_initial_radial", C.c_int64), ("n_initial_uniform", C.c_int64), ("adaptive_nmax", C.c_int64),
                ("initial_tol", C.c_double), ("max_recursion", C.c_int32), ("numincrease", C.c_int32),
                ("max_passes", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class DampingParams(C.Structure):
    """srt_damping_params of include/srt.h."""
    _fields_ = [("dist", C.c_int32), ("mode", C.c_int32), ("nres", C.c_int32), ("m", C.c_int32 * 8),
                ("Ne_h", C.c_double), ("kT", C.c_double), ("tol", C.c_double)]


class Segment(C.Structure):
    """srt_segment of include/srt.h: what one call of srt_trace_run_next hands out."""
    _fields_ = [("segment", C.c_int32), ("reserved", C.c_int32), ("nrays", C.c_int64), ("ray", ip),
                ("offsets", C.POINTER(C.c_int64)), ("rows", dp), ("nrows", ip), ("stopcond", ip),
                ("accepted_steps", C.c_int64)]


class Surface(C.Structure):
    """srt_surface of include/srt.h: kind 0 sphere, 1 dipole L-shell, 2 magnetic latitude, 3 plane; see sphere() .. plane()."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 4)]


class Observer(C.Structure):
    """srt_observer of include/srt.h: a point x[3] in SM metres and its detection radius in metres; see observer_array()."""
    _fields_ = [("x", C.c_double * 3), ("radius", C.c_double)]


class BinAxis(C.Structure):
    """srt_bin_axis of include/srt.h: a coordinate kind, n cells, n + 1 edges in host memory; see axis() and axis_maglat()."""
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("edges", C.POINTER(C.c_double))]


class BinParams(C.Structure):
    """srt_bin_params of include/srt.h."""
    _fields_ = [("naxes", C.c_int32), ("nsub", C.c_int32), ("quantum", C.c_double), ("axis", BinAxis * 3)]


MAXSURF = 16  # SRT_MAXSURF
MAXOBS = 65536  # SRT_MAXOBS
RUNNING = -1  # SRT_RUNNING: stopcond of a paused ray
STATE = 17    # SRT_STATE: doubles in a paused ray's record
STASH_STATS = 7  # SRT_STASH_STATS: counts of srt_launch_stash_stats


def library_path():
    return _build.LIB


def lib():
    """Load libsrt_hip.so (building it if the sources are newer).  Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SRT_LIB_OVERRIDE") or _build.LIB  # override: A/B builds of the same sources (tools/ab.sh)
    if not os.path.exists(path):
        _build.build()
    if not os.path.exists(path):
        raise SrtError("libsrt_hip.so is missing and could not be built; the HIP path is the only path")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.srt_last_error.restype = C.c_char_p
    L.srt_init.argtypes = [C.c_int]
    L.srt_device_info.argtypes = [C.c_char_p, C.c_int, ip, C.POINTER(C.c_int64)]
    L.srt_model_create_ngo.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.srt_model_create_interp_file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.srt_model_create_interp.argtypes = [C.c_int] * 4 + [dp, dp, dp, dp, C.POINTER(dp), C.c_int, C.c_int,
                                                          C.POINTER(vp)]
    L.srt_model_create_interp_file_layout.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.srt_model_create_interp_layout.argtypes = [C.c_int] * 4 + [dp, dp, dp, dp, C.POINTER(dp), C.c_int, C.c_int, C.c_int,
                                                                 C.POINTER(vp)]
    L.srt_model_create_interp_from_model_layout.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int,
                                                            C.c_int, C.POINTER(vp)]
    L.srt_model_interp_layout.argtypes = [vp]
    L.srt_interp_layout_bytes.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.srt_interp_layout_choose.argtypes = [C.c_int] * 4 + [C.c_int64]
    L.srt_model_create_scattered_file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                                  C.c_double, C.POINTER(vp)]
    L.srt_model_create_scattered_file_root.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                                       C.c_double, C.c_int64, C.POINTER(vp)]
    L.srt_model_create_simple3d.argtypes = [C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(vp)]
    L.srt_model_create_ngo3d.argtypes = [C.c_char_p, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(vp)]
    L.srt_model_create_at64thch.argtypes = [C.c_int, dp, C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.srt_field_line_foot.argtypes = [vp, C.c_int64, dp, dp]
    L.srt_model_set_field.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    L.srt_model_set_tsyganenko_params.argtypes = [vp, dp]
    L.srt_model_destroy.argtypes = [vp]
    L.srt_model_destroy.restype = None
    L.srt_model_trim.argtypes = [vp]
    L.srt_model_kind.argtypes = [vp]
    L.srt_model_nspec.argtypes = [vp]
    L.srt_model_species.argtypes = [vp, dp, dp]
    L.srt_model_device_bytes.argtypes = [vp]
    L.srt_model_device_struct.argtypes = [vp]
    L.srt_model_device_struct.restype = vp
    L.srt_model_device_bytes.restype = C.c_int64
    L.srt_plasma_params.argtypes = [vp, C.c_int64, dp, dp, dp, dp, dp, dp]
    L.srt_dispersion.argtypes = [vp, C.c_int64, dp, dp, dp, dp]
    L.srt_is_right_handed.argtypes = [C.c_int64, dp, ip]
    L.srt_gradients.argtypes = [vp, C.c_int64, dp, dp, dp, C.c_double, dp]
    L.srt_rk_step.argtypes = [vp, C.c_int64, dp, dp, C.c_double, dp]
    L.srt_rows_per_ray.argtypes = [C.POINTER(Params)]
    L.srt_rows_per_ray.restype = C.c_int32
    L.srt_trace_batch.argtypes = [vp, C.POINTER(Params), C.c_int64, dp, dp, dp, dp, ip, ip, C.POINTER(C.c_int64)]
    L.srt_trace_batch_device.argtypes = [vp, C.POINTER(Params), C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.srt_pack_rows_device.argtypes = [C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, vp, C.c_int64, vp]
    L.srt_trace_segments.argtypes = [C.POINTER(Params), C.c_int32]
    L.srt_trace_segments.restype = C.c_int32
    L.srt_trace_segment_device.argtypes = [vp, C.POINTER(Params), C.c_int64, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_int64,
                                           vp, vp, vp, vp, vp, vp]
    L.srt_running_rays_device.argtypes = [C.c_int64, vp, vp, vp, vp]
    L.srt_trace_run_open.argtypes = [vp, C.POINTER(Params), C.c_int64, dp, dp, dp, C.c_int32, C.POINTER(vp)]
    L.srt_trace_run_next.argtypes = [vp, C.POINTER(Segment)]
    L.srt_trace_run_close.argtypes = [vp]
    L.srt_trace_run_close.restype = None
    L.srt_write_ray_file_packed.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_int64, C.c_int, dp, dp, dp,
                                            C.POINTER(C.c_int64), dp, ip]
    L.srt_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.srt_launch_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    if hasattr(L, "srt_launch_stash_stats"):  # (an A/B build of older sources, SRT_LIB_OVERRIDE, has none)
        L.srt_launch_stash_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    L.srt_read_rays_file.argtypes = [C.c_char_p, C.POINTER(dp), C.POINTER(dp), C.POINTER(dp)]
    L.srt_read_rays_file.restype = C.c_int64
    L.srt_write_ray_file.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(Params), C.c_int, dp, dp,
                                     dp, dp, ip, ip]
    L.srt_read_ray_file.argtypes = [C.c_char_p, ip, dp, dp, C.POINTER(C.c_int64), C.POINTER(C.POINTER(C.c_int64)), C.POINTER(ip),
                                    C.POINTER(ip), C.POINTER(dp), C.POINTER(dp)]
    L.srt_read_ray_file.restype = C.c_int64
    L.srt_free.argtypes = [vp]
    L.srt_free.restype = None
    L.srt_build_grid.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, dp]
    L.srt_model_create_interp_from_model.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int,
                                                     C.POINTER(vp)]
    L.srt_build_samples.argtypes = [vp, C.POINTER(SamplerParams), C.c_int64, dp, C.POINTER(C.c_int64), C.POINTER(dp),
                                    C.POINTER(C.c_int64)]
    L.srt_damping.argtypes = [C.POINTER(DampingParams), C.c_int, dp, dp, C.c_int32, C.c_int32, C.c_int64, dp, ip, dp, dp,
                              dp, ip]
    L.srt_damping_device.argtypes = [C.POINTER(DampingParams), C.c_int, dp, dp, C.c_int32, C.c_int32, C.c_int64, vp, vp,
                                     vp, vp, vp, vp, vp]
    i32p = C.POINTER(C.c_int32)
    L.srt_grid_file_read.argtypes = [C.c_char_p, i32p, dp, dp, dp, C.POINTER(dp), C.POINTER(dp)]
    L.srt_grid_file_write.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp]
    L.srt_grid_file_convert.argtypes = [C.c_char_p, C.c_char_p]
    L.srt_grid_file_is_binary.argtypes = [C.c_char_p]
    L.srt_points_file_write.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int64, dp, dp, dp, dp]
    L.srt_points_file_convert.argtypes = [C.c_char_p, C.c_char_p]
    L.srt_points_file_is_binary.argtypes = [C.c_char_p]
    L.srt_dump_model.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, C.c_int, dp]
    L.srt_sm_to_mag.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, dp, dp]
    L.srt_dump_file_write.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp]
    L.srt_dump_file_read.argtypes = [C.c_char_p, i32p, dp, C.POINTER(dp)]
    i64p = C.POINTER(C.c_int64)
    L.srt_crossings_device.argtypes = [C.c_int, C.POINTER(Surface), C.c_int64, vp, vp, vp, vp, C.c_int64, vp, vp]
    L.srt_crossings.argtypes = [C.c_int, C.POINTER(Surface), C.c_int64, i64p, dp, i64p, C.POINTER(dp), C.POINTER(ip)]
    L.srt_crossings_file_write.argtypes = [C.c_char_p, C.c_int64, i64p, ip, dp]
    obp = C.POINTER(Observer)
    L.srt_approaches_device.argtypes = [C.c_int, obp, C.c_int64, vp, vp, vp, vp, vp, C.c_int64, vp, vp]
    L.srt_approaches.argtypes = [C.c_int, obp, C.c_int64, i64p, dp, i64p, C.POINTER(dp), C.POINTER(ip), C.POINTER(dp)]
    L.srt_approaches_file_write.argtypes = [C.c_char_p, C.c_int64, i64p, ip, dp, dp]
    L.srt_tubes_device.argtypes = [C.c_int64, i64p, vp, vp, vp, vp, vp]
    L.srt_tubes.argtypes = [C.c_int64, i64p, i64p, dp, dp, ip]
    L.srt_tubes_file_write.argtypes = [C.c_char_p, C.c_int64, i64p, i64p, dp, dp, ip]
    bpp = C.POINTER(BinParams)
    L.srt_bin_rays_device.argtypes = [bpp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.srt_bin_rays.argtypes = [bpp, C.c_int64, i64p, dp, dp, dp, C.POINTER(i64p), C.POINTER(i64p), i64p]
    L.srt_bin_cells.argtypes = [bpp, i64p]
    L.srt_bin_file_write.argtypes = [C.c_char_p, bpp, i64p, i64p]
    L.srt_bin_file_read.argtypes = [C.c_char_p, bpp, C.POINTER(dp), i64p, C.POINTER(dp), C.POINTER(i64p)]
    _lib = L
    return L


# error codes of include/srt.h
SRT_OK, SRT_EINVAL, SRT_EIO, SRT_EDEVICE, SRT_ENOMEM = 0, -1, -2, -3, -4


# device layouts of the interp model (include/srt.h)
INTERP_EXPANDED, INTERP_NODES, INTERP_AUTO = 0, 1, 2
INTERP_LAYOUTS = {"expanded": INTERP_EXPANDED, "nodes": INTERP_NODES, "auto": INTERP_AUTO}


def _layout(layout):
    """'expanded' | 'nodes' | 'auto' (or the number) -> SRT_INTERP_*"""
    if isinstance(layout, str):
        if layout not in INTERP_LAYOUTS:
            raise ValueError("layout %r is not one of %s" % (layout, ", ".join(INTERP_LAYOUTS)))
        return INTERP_LAYOUTS[layout]
    return int(layout)


def interp_layout_bytes(nspec, nx, ny, nz, layout):
    """-> (bytes of the table, the most that creation holds on the device at once); needs no GPU."""
    t, pk = C.c_int64(), C.c_int64()
    _check(lib().srt_interp_layout_bytes(nspec, nx, ny, nz, _layout(layout), C.byref(t), C.byref(pk)))
    return t.value, pk.value


def interp_layout_choose(nspec, nx, ny, nz, free_bytes):
    """What layout='auto' picks with `free_bytes` free on the device: INTERP_EXPANDED or INTERP_NODES; SrtError (SRT_ENOMEM)
    when neither fits.  Needs no GPU."""
    rc = lib().srt_interp_layout_choose(nspec, nx, ny, nz, int(free_bytes))
    if rc < 0:
        _check(rc)
    return rc


def _take(*arrays):
    """Copies of the arrays the library handed over in one call, each given as (pointer, shape) or (pointer, shape, dtype) -> a
    list of them.  Every pointer is srt_free'd here, also when a copy fails; a null pointer, which the library returns for
    nothing, gives zeros (float64 unless a dtype is named)."""
    try:
        return [np.ctypeslib.as_array(a[0], a[1]).copy() if a[0] else np.zeros(a[1], dtype=a[2] if len(a) > 2 else np.float64)
                for a in arrays]
    finally:
        for a in arrays:
            lib().srt_free(a[0])


def _check(rc):
    if rc != 0:
        raise SrtError("srt error %d: %s" % (rc, (lib().srt_last_error() or b"").decode()))


def _f64(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None:
        a = a.reshape(shape)
    return a


def _dp(a):
    return a.ctypes.data_as(dp)


def init(device=0):
    _check(lib().srt_init(device))


def device_info():
    name = C.create_string_buffer(256)
    cu = C.c_int32()
    mem = C.c_int64()
    _check(lib().srt_device_info(name, 256, C.byref(cu), C.byref(mem)))
    return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}


class Model:
    """Opaque density/field model living on the device (replaces the adapters' state blob)."""

    def __init__(self, handle):
        self.h = handle
        self.kind = lib().srt_model_kind(handle)
        self.nspec = lib().srt_model_nspec(handle)

    @classmethod
    def ngo(cls, configfile, yearday=2010001, msec=0):
        h = C.c_void_p()
        _check(lib().srt_model_create_ngo(os.fsencode(configfile), yearday, msec, C.byref(h)))
        return cls(h)

    @classmethod
    def interp_file(cls, gridfile, yearday=2010001, msec=0, layout="expanded"):
        """layout: 'expanded' (the coefficient table), 'nodes' (the node table, an eighth of the bytes) or 'auto'."""
        h = C.c_void_p()
        _check(lib().srt_model_create_interp_file_layout(os.fsencode(gridfile), yearday, msec, _layout(layout), C.byref(h)))
        return cls(h)

    @classmethod
    def interp(cls, F, bounds, qs, ms, derivs=None, yearday=2010001, msec=0, layout="expanded"):
        """F[nz, ny, nx, nspec] = ln N_s in the grid file's order (species fastest, then x, y, z).  layout: as interp_file."""
        F = _f64(F)
        nz, ny, nx, ns = F.shape
        b, q, m = _f64(bounds, 6), _f64(qs, ns), _f64(ms, ns)
        dptr = None
        keep = []
        if derivs is not None:
            keep = [_f64(d, F.shape) for d in derivs]
            dptr = (dp * 7)(*[_dp(d) for d in keep])
        h = C.c_void_p()
        _check(lib().srt_model_create_interp_layout(ns, nx, ny, nz, _dp(b), _dp(q), _dp(m), _dp(F), dptr, yearday, msec,
                                                    _layout(layout), C.byref(h)))
        return cls(h)

    @classmethod
    def scattered_file(cls, ptsfile, yearday=2010001, msec=0, window_scale=1.5, order=2, exact=0,
                       local_window_scale=5.0, root_sample=-1):
        """root_sample: 0-based record number of the sample at the root of the REFERENCE's kd-tree (its stored spacing stays
        0 there, include/srt.h srt_model_create_scattered_file_root); -1 = the true distance for every sample."""
        h = C.c_void_p()
        _check(lib().srt_model_create_scattered_file_root(os.fsencode(ptsfile), yearday, msec, window_scale, order,
                                                          exact, local_window_scale, int(root_sample), C.byref(h)))
        return cls(h)

    @classmethod
    def simple3d(cls, kp, yearday=2010001, msec=0, fixed_mlt=None):
        """modelnum 6, the closed-form simplified GCPM (simple_3d_model_adapter.f95).  fixed_mlt: None = MLT from each point's
        longitude; a number = every point is held at that many hours MLT (the driver's --fixed_MLT=1 --MLT=...)."""
        h = C.c_void_p()
        fixed = 0 if fixed_mlt is None else 1
        _check(lib().srt_model_create_simple3d(float(kp), fixed, 0.0 if fixed_mlt is None else float(fixed_mlt), yearday,
                                               msec, C.byref(h)))
        return cls(h)

    @classmethod
    def ngo3d(cls, configfile, kp, yearday=2010001, msec=0, fixed_mlt=None):
        """modelnum 5, the 3-D Ngo model (ngo_3d_dens_model_adapter.f95): the Ngo model of `configfile` with the plasmapause
        of every evaluated point at a8(MLT, kp) - ddk.  fixed_mlt: None = MLT from each point's longitude (all the reference's
        driver does); a number = every point is held at that many hours MLT."""
        h = C.c_void_p()
        fixed = 0 if fixed_mlt is None else 1
        _check(lib().srt_model_create_ngo3d(os.fsencode(configfile), float(kp), fixed,
                                            0.0 if fixed_mlt is None else float(fixed_mlt), yearday, msec, C.byref(h)))
        return cls(h)

    @classmethod
    def at64thch(cls, gcpm_kp, parmod, yearday=2010001, msec=0, igrf_coeff_file=None):
        """modelnum 7, the AT64ThCh diffusive-equilibrium plasmasphere (AT64ThCh_adapter.f95): above 400 km the electron density
        is scaled by |B(point)| / |B(foot)|, the foot found by a field-line trace through T04_s + IGRF for every evaluated
        point.  gcpm_kp: the driver's --gcpm_kp, an integer; parmod = Pdyn, Dst, ByIMF, BzIMF, W1..W6 (--tsyganenko_*), always
        needed: the trace uses T04_s and IGRF whatever set_field() says (include/srt.h has the three decisions on what the
        adapter leaves undefined)."""
        if int(gcpm_kp) != gcpm_kp:
            raise ValueError("gcpm_kp is an integer")
        h = C.c_void_p()
        _check(lib().srt_model_create_at64thch(int(gcpm_kp), _dp(_f64(parmod, (10,))),
                                               os.fsencode(igrf_coeff_file) if igrf_coeff_file else None, yearday, msec, C.byref(h)))
        return cls(h)

    def field_line_foot(self, x):
        """geopack's TRACE_08 from x[n,3] (SM, metres) through T04_s + IGRF with the AT64ThCh adapter's constants ->
        [n,6] = XF, YF, ZF (GSM, R_E), |IGRF| there (nT), ending (0 sphere, 1 outer boundary, 2 reversals, 3 no end within 500
        points: NaN), number of points.  The handle needs a coefficient table and parmod (set_field(..., parmod=...))."""
        x = _f64(x, (-1, 3))
        out = np.zeros((x.shape[0], 6))
        _check(lib().srt_field_line_foot(self.h, x.shape[0], _dp(x), _dp(out)))
        return out

    def build_grid(self, nx, ny, nz, bounds, compder=False):
        """Sample this model on a regular grid in log space on the device (the reference's grid builder with this
        model in place of GCPM).  -> F[nz,ny,nx,nspec], derivs (list of 7 arrays or None)."""
        ns = self.nspec
        F = np.empty((nz, ny, nx, ns))
        D = np.empty((7, nz, ny, nx, ns)) if compder else None
        _check(lib().srt_build_grid(self.h, int(bool(compder)), nx, ny, nz, _dp(_f64(bounds, (6,))), _dp(F),
                                    _dp(D) if compder else None))
        return F, (list(D) if compder else None)

    def dump(self, nx, ny, nz, bounds, mag_coords=False):
        """The reference's dumpmodel on the device: funcPlasmaParams at every node of a regular grid (any axis may have one
        node: a slice).  -> f[nz, ny, nx, 4*nspec+3] = qs, Ns, ms, nus (all zeros), B0 of the node, the dump file's order.
        mag_coords: the grid is in MAG (geomagnetic dipole) coordinates; each node goes through sm_to_mag for the model's date
        first, as dumpmodel.f95 does.  Every node is bit-equal to plasma_params at its coordinates."""
        f = np.empty((nz, ny, nx, 4 * self.nspec + 3))
        _check(lib().srt_dump_model(self.h, nx, ny, nz, _dp(_f64(bounds, (6,))), int(mag_coords), _dp(f)))
        return f

    def build_samples(self, bounds, n_zero_altitude=0, n_iri_pad=0, n_initial_radial=0, n_initial_uniform=0,
                      adaptive_nmax=0, initial_tol=1.0, max_recursion=20, numincrease=5, max_passes=0, seed=0,
                      input_points=None):
        """The reference's random / adaptive sample-set builder with this model in place of GCPM, on the device.
        -> (samples[n, 3+nspec] = the lines "x y z lnN_1.." of a model-4 file, stage_counts[6])."""
        sp = SamplerParams()
        sp.bounds[:] = [float(b) for b in bounds]
        sp.n_zero_altitude, sp.n_iri_pad = int(n_zero_altitude), int(n_iri_pad)
        sp.n_initial_radial, sp.n_initial_uniform = int(n_initial_radial), int(n_initial_uniform)
        sp.adaptive_nmax, sp.initial_tol, sp.max_recursion = int(adaptive_nmax), float(initial_tol), int(max_recursion)
        sp.numincrease, sp.max_passes, sp.seed = int(numincrease), int(max_passes), int(seed)
        w = 3 + self.nspec
        n_in, inp = 0, None
        if input_points is not None:
            inp = _f64(input_points).reshape(-1, w)
            n_in = inp.shape[0]
        n_out = C.c_int64()
        out = dp()
        counts = (C.c_int64 * 6)()
        _check(lib().srt_build_samples(self.h, C.byref(sp), n_in, _dp(inp) if n_in else None, C.byref(n_out),
                                       C.byref(out), counts))
        return _take((out, (n_out.value, w)))[0], list(counts)

    def to_interp(self, nx, ny, nz, bounds, compder=False, yearday=2010001, msec=0, layout="expanded"):
        """A modelnum=3 model tabulating this one, built without leaving the device.  layout: as interp_file."""
        h = C.c_void_p()
        _check(lib().srt_model_create_interp_from_model_layout(self.h, int(bool(compder)), nx, ny, nz,
                                                               _dp(_f64(bounds, (6,))), yearday, msec, _layout(layout),
                                                               C.byref(h)))
        return Model(h)

    @property
    def layout(self):
        """Device layout of an interp model: INTERP_EXPANDED (0) or INTERP_NODES (1); -1 for the other kinds."""
        return lib().srt_model_interp_layout(self.h)

    def set_field(self, use_igrf=0, use_tsyganenko=0, igrf_coeff_file=None, parmod=None):
        """--use_igrf / --use_tsyganenko of the driver; parmod = Pdyn, Dst, ByIMF, BzIMF, W1..W6 (--tsyganenko_*)."""
        if parmod is not None:
            _check(lib().srt_model_set_tsyganenko_params(self.h, _dp(_f64(parmod, (10,)))))
        _check(lib().srt_model_set_field(self.h, int(use_igrf), int(use_tsyganenko),
                                         os.fsencode(igrf_coeff_file) if igrf_coeff_file else None))
        return self

    def trim(self):
        """Give back the grow-only device scratch (host-buffer staging, per-launch buffers); the tables stay."""
        _check(lib().srt_model_trim(self.h))
        return self

    def close(self):
        if self.h:
            lib().srt_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self):
        return lib().srt_model_device_bytes(self.h)

    def species(self):
        qs, ms = np.zeros(4), np.zeros(4)
        _check(lib().srt_model_species(self.h, _dp(qs), _dp(ms)))
        return qs, ms

    # ---- layered entry points
    def plasma_params(self, x):
        """funcPlasmaParams at x[n,3] -> [n,19] = qs(4) Ns(4) ms(4) nus(4) B0(3)."""
        x = _f64(x, (-1, 3))
        n = x.shape[0]
        qs, Ns, ms, nus, B0 = (np.zeros((n, 4)) for _ in range(4)) if False else \
            (np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 3)))
        _check(lib().srt_plasma_params(self.h, n, _dp(x), _dp(qs), _dp(Ns), _dp(ms), _dp(nus), _dp(B0)))
        return np.concatenate([qs, Ns, ms, nus, B0], axis=1)

    def dispersion(self, x, k, w):
        x, k, w = _f64(x, (-1, 3)), _f64(k, (-1, 3)), _f64(w, (-1,))
        out = np.zeros((x.shape[0], 10))
        _check(lib().srt_dispersion(self.h, x.shape[0], _dp(x), _dp(k), _dp(w), _dp(out)))
        return out

    def gradients(self, x, k, w, del_):
        x, k, w = _f64(x, (-1, 3)), _f64(k, (-1, 3)), _f64(w, (-1,))
        out = np.zeros((x.shape[0], 14))
        _check(lib().srt_gradients(self.h, x.shape[0], _dp(x), _dp(k), _dp(w), del_, _dp(out)))
        return out

    def rk_step(self, args, dt, del_):
        args = _f64(args, (-1, 7))
        dt = _f64(np.broadcast_to(dt, (args.shape[0],)))
        out = np.zeros((args.shape[0], 21))
        _check(lib().srt_rk_step(self.h, args.shape[0], _dp(args), _dp(dt), del_, _dp(out)))
        return out

    # ---- the hot path
    def trace(self, pos0, dir0, w0, params=None, **kw):
        """Batched raytracer_run.  Returns rows[n, slots, 20], nrows[n], stopcond[n], accepted_steps."""
        p = params if params is not None else make_params(**kw)
        pos0, dir0, w0 = _f64(pos0, (-1, 3)), _f64(dir0, (-1, 3)), _f64(w0, (-1,))
        n = pos0.shape[0]
        slots = lib().srt_rows_per_ray(C.byref(p))
        rows = np.zeros((n, slots, ROW))
        nrows = np.zeros(n, dtype=np.int32)
        stop = np.zeros(n, dtype=np.int32)
        steps = C.c_int64()
        _check(lib().srt_trace_batch(self.h, C.byref(p), n, _dp(pos0), _dp(dir0), _dp(w0), _dp(rows),
                                     nrows.ctypes.data_as(ip), stop.ctypes.data_as(ip), C.byref(steps)))
        return rows, nrows, stop, steps.value

    def trace_segments(self, pos0, dir0, w0, segment_rows, params=None, **kw):
        """The same rays traced in segments of `segment_rows` kept rows per ray and launch: device memory for
        n * segment_rows rows instead of n * slots, and only rows that exist come back.  A generator; each item is a dict
        of one segment: segment (its number), ray[m] (ids of the rays that ran, ascending), offsets[m+1] and
        rows[offsets[m], 20] (their kept rows of this segment, ray after ray), nrows[m] (rows so far), stopcond[m]
        (RUNNING = -1 for a paused ray), steps (accepted in this segment), kernel_ms.  Every model but the scattered one
        gives the rows of `trace` bit for bit (include/srt.h)."""
        p = params if params is not None else make_params(**kw)
        pos0, dir0, w0 = _f64(pos0, (-1, 3)), _f64(dir0, (-1, 3)), _f64(w0, (-1,))
        run = C.c_void_p()
        _check(lib().srt_trace_run_open(self.h, C.byref(p), pos0.shape[0], _dp(pos0), _dp(dir0), _dp(w0), int(segment_rows),
                                        C.byref(run)))
        try:
            seg = Segment()
            for _ in range(trace_segment_count(p, segment_rows)):  # the bound; the run ends sooner when no ray is left
                rc = lib().srt_trace_run_next(run, C.byref(seg))
                if rc < 0:
                    _check(rc)
                if rc == 0:
                    break
                m = seg.nrays
                off = np.ctypeslib.as_array(seg.offsets, (m + 1,)).copy()
                total = int(off[m])
                yield {"segment": seg.segment,
                       "ray": np.ctypeslib.as_array(seg.ray, (m,)).copy(),
                       "offsets": off,
                       "rows": np.ctypeslib.as_array(seg.rows, (total, ROW)).copy() if total else np.zeros((0, ROW)),
                       "nrows": np.ctypeslib.as_array(seg.nrows, (m,)).copy(),
                       "stopcond": np.ctypeslib.as_array(seg.stopcond, (m,)).copy(),
                       "steps": seg.accepted_steps, "kernel_ms": self.last_kernel_ms()}
        finally:
            lib().srt_trace_run_close(run)

    def trace_packed(self, pos0, dir0, w0, segment_rows, params=None, **kw):
        """`trace` through trace_segments, whole trajectories in the packed layout: offsets[n+1], rows[offsets[n], 20] = the
        kept rows of ray 0, ray 1, .. back to back (what read_ray_file returns and write_ray_file_packed takes), nrows[n],
        stopcond[n], accepted_steps."""
        n = _f64(pos0, (-1, 3)).shape[0]
        return assemble_segments(n, self.trace_segments(pos0, dir0, w0, segment_rows, params=params, **kw))

    def launch_ms(self, back=0):
        ms = C.c_float()
        _check(lib().srt_launch_ms(self.h, back, C.byref(ms)))
        return float(ms.value)

    def stash_stats(self, back=0):
        """The tail stash of a past trace launch (include/srt.h, srt_launch_stash_stats): a dict of banked[4] (rays banked at
        1/2, 3/4, 7/8, 15/16 of maxsteps), resumed, max_fill (most records one wave held) and tail_trips (loop trips after
        a wave saw the queue empty).  All zero for a launch that banked nothing."""
        s = (C.c_int64 * STASH_STATS)()
        _check(lib().srt_launch_stash_stats(self.h, back, s))
        return {"banked": [int(v) for v in s[0:4]], "resumed": int(s[4]), "max_fill": int(s[5]), "tail_trips": int(s[6])}

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(lib().srt_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value


def damping_params(dist=0, mode=0, m=(), Ne_h=0.0, kT=0.0, tol=0.0):
    p = DampingParams()
    p.dist, p.mode, p.nres, p.Ne_h, p.kT, p.tol = dist, mode, len(m), Ne_h, kT, tol
    for i, v in enumerate(m):
        p.m[i] = int(v)
    return p


def damping(species, outputper, rows, nrows, w0, **kw):
    """Hot-plasma damping along the kept rows (the reference's matlab/damping post-processor, on the device).
    rows [nrays, slots, 20], nrows [nrays], w0 [nrays] as Model.trace returns them -> rate, magnitude, flag."""
    qs, ms = species
    rows = _f64(rows)
    nrays, slots, _ = rows.shape
    nrows = np.ascontiguousarray(nrows, dtype=np.int32)
    qs, ms, w0 = _f64(qs), _f64(ms), _f64(w0, (nrays,))
    rate, mag = np.zeros((nrays, slots)), np.zeros((nrays, slots))
    flag = np.zeros((nrays, slots), dtype=np.int32)
    p = damping_params(**kw)
    _check(lib().srt_damping(C.byref(p), qs.size, _dp(qs), _dp(ms), slots, outputper, nrays, _dp(rows),
                             nrows.ctypes.data_as(ip), _dp(w0), _dp(rate), _dp(mag), flag.ctypes.data_as(ip)))
    return rate, mag, flag


def is_right_handed(rows):
    """rows[n,5] = n2, phi (degrees, as the reference passes it), S, D, P -> bool[n]."""
    rows = _f64(rows, (-1, 5))
    out = np.zeros(rows.shape[0], dtype=np.int32)
    _check(lib().srt_is_right_handed(rows.shape[0], _dp(rows), out.ctypes.data_as(ip)))
    return out.astype(bool)


def read_rays_file(path):
    a, b, c = dp(), dp(), dp()
    n = lib().srt_read_rays_file(os.fsencode(path), C.byref(a), C.byref(b), C.byref(c))
    if n < 0:
        _check(int(n))
    pos0 = np.ctypeslib.as_array(a, (n, 3)).copy() if n else np.zeros((0, 3))
    dir0 = np.ctypeslib.as_array(b, (n, 3)).copy() if n else np.zeros((0, 3))
    w0 = np.ctypeslib.as_array(c, (n,)).copy() if n else np.zeros((0,))
    for ptr in (a, b, c):
        lib().srt_free(ptr)
    return pos0, dir0, w0


def write_ray_file(path, species, params, w0, rows, nrows, stopcond, raynum0=1, append=False):
    """species: a Model, or (nspec, qs, ms)."""
    if isinstance(species, Model):
        qs, ms = species.species()
        nspec = species.nspec
    else:
        nspec, qs, ms = species
        qs, ms = _f64(qs), _f64(ms)
    w0 = _f64(w0, (-1,))
    rows = _f64(rows)
    nrows = np.ascontiguousarray(nrows, dtype=np.int32)
    stopcond = np.ascontiguousarray(stopcond, dtype=np.int32)
    _check(lib().srt_write_ray_file(os.fsencode(path), int(append), raynum0, w0.shape[0], C.byref(params), nspec,
                                    _dp(qs), _dp(ms), _dp(w0), _dp(rows), nrows.ctypes.data_as(ip),
                                    stopcond.ctypes.data_as(ip)))


def assemble_segments(n, segments):
    """The items of Model.trace_segments for n rays -> offsets[n+1], rows[offsets[n], 20] (whole trajectories, ray-major),
    nrows[n], stopcond[n], accepted_steps."""
    nrows, stop = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    kept = np.zeros(n, dtype=np.int64)
    segs, steps = [], 0
    for sg in segments:
        ids = sg["ray"]
        nrows[ids], stop[ids] = sg["nrows"], sg["stopcond"]
        kept[ids] += np.diff(sg["offsets"])
        steps += sg["steps"]
        segs.append(sg)
    offsets = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    rows = np.zeros((int(offsets[n]), ROW))
    fill = offsets[:-1].copy()  # where each ray's next rows go
    for sg in segs:
        cnt = np.diff(sg["offsets"])
        if cnt.sum() == 0:
            continue
        # row j of the segment belongs to ray[i] with offsets[i] <= j < offsets[i+1]
        owner = np.repeat(np.arange(len(cnt)), cnt)
        rows[fill[sg["ray"]][owner] + (np.arange(cnt.sum()) - sg["offsets"][:-1][owner])] = sg["rows"]
        fill[sg["ray"]] += cnt
    return offsets, rows, nrows, stop, steps


def trace_segment_count(params, segment_rows):
    """srt_trace_segments: segments a segmented trace has at most = ceil(slots / segment_rows); needs no GPU."""
    return lib().srt_trace_segments(C.byref(params), int(segment_rows))


def write_ray_file_packed(path, species, w0, offsets, rows, stopcond, raynum0=1, append=False):
    """write_ray_file from the packed layout (read_ray_file, Model.trace_packed): offsets[n+1], rows[offsets[n], 20].
    species: a Model, or (nspec, qs, ms).  Equal rows give the bytes write_ray_file gives."""
    if isinstance(species, Model):
        qs, ms = species.species()
        nspec = species.nspec
    else:
        nspec, qs, ms = species
        qs, ms = _f64(qs), _f64(ms)
    w0 = _f64(w0, (-1,))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets.shape != (w0.shape[0] + 1,):
        raise ValueError("offsets has %d entries for %d rays" % (offsets.size, w0.shape[0]))
    rows = _f64(rows).reshape(-1, ROW)
    if rows.shape[0] < (offsets[-1] if offsets.size else 0):
        raise ValueError("offsets name %d rows, rows holds %d" % (offsets[-1], rows.shape[0]))
    stopcond = np.ascontiguousarray(stopcond, dtype=np.int32)
    _check(lib().srt_write_ray_file_packed(os.fsencode(path), int(append), raynum0, w0.shape[0], nspec, _dp(qs), _dp(ms),
                                           _dp(w0), offsets.ctypes.data_as(C.POINTER(C.c_int64)), _dp(rows),
                                           stopcond.ctypes.data_as(ip)))


def read_ray_file(path):
    """A .ray file (this library's or the reference driver's) -> dict(raynum, stopcond, kept, w0 per ray; rows[nrecords, 20] =
    the kept rows of all rays back to back; nspec, qs, ms).  `padded(slots)` rebuilds the [nrays, slots, 20] layout."""
    nspec, nrec = C.c_int32(), C.c_int64()
    qs, ms = np.zeros(4), np.zeros(4)
    pr, ps, pk, pw, prow = C.POINTER(C.c_int64)(), ip(), ip(), dp(), dp()
    n = lib().srt_read_ray_file(os.fsencode(path), C.byref(nspec), _dp(qs), _dp(ms), C.byref(nrec), C.byref(pr), C.byref(ps),
                                C.byref(pk), C.byref(pw), C.byref(prow))
    if n < 0:
        _check(int(n))
    try:
        out = {"raynum": np.ctypeslib.as_array(pr, (n,)).copy() if n else np.zeros(0, dtype=np.int64),
               "stopcond": np.ctypeslib.as_array(ps, (n,)).copy() if n else np.zeros(0, dtype=np.int32),
               "kept": np.ctypeslib.as_array(pk, (n,)).copy() if n else np.zeros(0, dtype=np.int32),
               "w0": np.ctypeslib.as_array(pw, (n,)).copy() if n else np.zeros(0),
               "rows": np.ctypeslib.as_array(prow, (nrec.value, ROW)).copy() if nrec.value else np.zeros((0, ROW)),
               "nspec": nspec.value, "qs": qs[:nspec.value].copy(), "ms": ms[:nspec.value].copy()}
    finally:
        for ptr in (pr, ps, pk, pw, prow):
            lib().srt_free(ptr)
    return out


def padded_rows(ray):
    """read_ray_file's packed rows -> (rows[nrays, slots, 20], nrows[nrays]) with slots = the longest ray (outputper = 1)."""
    kept = ray["kept"]
    n, slots = len(kept), int(kept.max()) if len(kept) else 1
    rows = np.zeros((n, slots, ROW))
    off = np.concatenate([[0], np.cumsum(kept)])
    for i in range(n):
        rows[i, :kept[i]] = ray["rows"][off[i]:off[i + 1]]
    return rows, kept.astype(np.int32)


# ---- surface crossings along the kept rows (include/srt.h) -------
R_E = 6371.2e3


def sphere(r):
    """|x| = r metres."""
    return Surface(0, 0, (C.c_double * 4)(float(r), 0.0, 0.0, 0.0))


def lshell(L):
    """The dipole L-shell |x|^3 = L R_E (x^2 + y^2)."""
    return Surface(1, 0, (C.c_double * 4)(float(L), 0.0, 0.0, 0.0))


def maglat(rad):
    """The cone of magnetic latitude `rad` radians (0: the magnetic equator)."""
    return Surface(2, 0, (C.c_double * 4)(float(rad), 0.0, 0.0, 0.0))


def plane(normal, d):
    """normal . x = d."""
    nx, ny, nz = (float(v) for v in normal)
    return Surface(3, 0, (C.c_double * 4)(nx, ny, nz, float(d)))


def surface_array(surfaces):
    """A sequence of Surface -> (ctypes array, count), as the C ABI takes them."""
    surfaces = list(surfaces)
    arr = (Surface * max(len(surfaces), 1))()
    for i, s in enumerate(surfaces):
        arr[i] = s
    return arr, len(surfaces)


def _packed(offsets, rows):
    """A packed row set as the C ABI takes it -> (offsets int64[nrays + 1], rows float64[>= offsets[nrays], 20]), contiguous."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    rows = _f64(rows).reshape(-1, ROW)
    if offsets.ndim != 1 or offsets.size < 1:
        raise ValueError("offsets holds nrays + 1 entries")
    if rows.shape[0] < offsets[-1]:
        raise ValueError("offsets name %d rows, rows holds %d" % (offsets[-1], rows.shape[0]))
    return offsets, rows


def crossings(offsets, rows, surfaces):
    """Where and when the rays of a packed row set (offsets[n+1], rows[offsets[n], 20]: read_ray_file, Model.trace_packed) cross
    `surfaces`, located on the cubic Hermite curve through consecutive kept rows -> (event_rows[E, 20], meta[E, 4] int32 =
    ray, surface index, interval, direction), ordered by (ray, interval, surface)."""
    offsets, rows = _packed(offsets, rows)
    arr, ns = surface_array(surfaces)
    n, pe, pm = C.c_int64(), dp(), ip()
    _check(lib().srt_crossings(ns, arr, offsets.size - 1, offsets.ctypes.data_as(C.POINTER(C.c_int64)), _dp(rows), C.byref(n),
                               C.byref(pe), C.byref(pm)))
    ev, meta = _take((pe, (n.value, ROW)), (pm, (n.value, 4), np.int32))
    return ev, meta


def pack_rows(rows, nrows, outputper):
    """rows[n, slots, 20], nrows[n] as Model.trace returns them -> (offsets[n+1], packed[offsets[n], 20]), on the host."""
    rows = _f64(rows)
    n, slots, _ = rows.shape
    nr = np.asarray(nrows, dtype=np.int64)
    kept = np.clip(np.where(nr > 0, (nr - 1) // int(outputper) + 1, 0), 0, slots)
    offsets = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    return offsets, rows[np.arange(slots)[None, :] < kept[:, None]].reshape(-1, ROW)


def crossings_padded(rows, nrows, outputper, surfaces):
    """crossings() of rows[n, slots, 20], nrows[n] as Model.trace returns them: packs first."""
    offsets, packed = pack_rows(rows, nrows, outputper)
    return crossings(offsets, packed, surfaces)


def write_crossings_file(path, raynum, meta, event_rows):
    """One record per event, (4 i10, 20 es24.15e3): raynum[e], surface index + 1, interval + 1, direction, the event's row."""
    meta = np.ascontiguousarray(meta, dtype=np.int32).reshape(-1, 4)
    event_rows = _f64(event_rows).reshape(-1, ROW)
    raynum = np.ascontiguousarray(raynum, dtype=np.int64).reshape(-1)
    if not (len(raynum) == len(meta) == len(event_rows)):
        raise ValueError("raynum, meta and event_rows name %d, %d and %d events" % (len(raynum), len(meta), len(event_rows)))
    _check(lib().srt_crossings_file_write(os.fsencode(path), len(meta), raynum.ctypes.data_as(C.POINTER(C.c_int64)),
                                          meta.ctypes.data_as(ip), _dp(event_rows)))


# ---- closest approaches to observer points along the kept rows (include/srt.h) -------
def observer_array(observers):
    """Observers as the C ABI takes them -> (ctypes array, count): a sequence of Observer, or an array [n, 4] of x, y, z (SM
    metres) and the detection radius (metres)."""
    if isinstance(observers, np.ndarray) or (len(observers) and not isinstance(observers[0], Observer)):
        a = _f64(observers).reshape(-1, 4)
        arr = (Observer * max(len(a), 1))()
        if len(a):
            C.memmove(arr, a.ctypes.data, a.nbytes)
        return arr, len(a)
    observers = list(observers)
    arr = (Observer * max(len(observers), 1))()
    for i, o in enumerate(observers):
        arr[i] = o
    return arr, len(observers)


def approaches(observers, offsets, rows):
    """Each ray's closest approach to each observer, where it comes within the observer's radius, located on the cubic Hermite
    curve through consecutive kept rows of a packed row set (offsets[n+1], rows[offsets[n], 20]) -> (event_rows[E, 20],
    meta[E, 4] int32 = ray, observer index, interval, 0, dist[E]), ordered by (ray, interval, observer)."""
    offsets, rows = _packed(offsets, rows)
    arr, no = observer_array(observers)
    n, pe, pm, pd = C.c_int64(), dp(), ip(), dp()
    _check(lib().srt_approaches(no, arr, offsets.size - 1, offsets.ctypes.data_as(C.POINTER(C.c_int64)), _dp(rows), C.byref(n),
                                C.byref(pe), C.byref(pm), C.byref(pd)))
    ev, meta, dist = _take((pe, (n.value, ROW)), (pm, (n.value, 4), np.int32), (pd, (n.value,)))
    return ev, meta, dist


def approaches_padded(rows, nrows, outputper, observers):
    """approaches() of rows[n, slots, 20], nrows[n] as Model.trace returns them: packs first."""
    offsets, packed = pack_rows(rows, nrows, outputper)
    return approaches(observers, offsets, packed)


def write_approaches_file(path, raynum, meta, dist, event_rows):
    """One record per event, (4 i10, 21 es24.15e3): raynum[e], observer index + 1, interval + 1, 0, the distance, the event's row."""
    meta = np.ascontiguousarray(meta, dtype=np.int32).reshape(-1, 4)
    event_rows = _f64(event_rows).reshape(-1, ROW)
    dist = _f64(dist).reshape(-1)
    raynum = np.ascontiguousarray(raynum, dtype=np.int64).reshape(-1)
    if not (len(raynum) == len(meta) == len(event_rows) == len(dist)):
        raise ValueError("raynum, meta, dist and event_rows name %d, %d, %d and %d events" % (len(raynum), len(meta), len(dist), len(event_rows)))
    _check(lib().srt_approaches_file_write(os.fsencode(path), len(meta), raynum.ctypes.data_as(C.POINTER(C.c_int64)),
                                           meta.ctypes.data_as(ip), _dp(dist), _dp(event_rows)))


# ---- ray tubes: the cross-section a ray and two neighbours span (include/srt.h) -------
def neighbour_table(neighbours, nrays):
    """neighbours as the C ABI takes them -> int64[nrays, 2], contiguous (-1, -1: no tube)."""
    nb = np.ascontiguousarray(neighbours, dtype=np.int64).reshape(-1, 2)
    if len(nb) != nrays:
        raise ValueError("neighbours holds %d pairs for %d rays" % (len(nb), nrays))
    return nb if len(nb) else np.full((1, 2), -1, dtype=np.int64)


def tubes(offsets, rows, neighbours):
    """The section of every ray's tube at each of its kept rows: neighbours[n, 2] names the two rays that span ray a's tube
    (-1, -1: none), each is taken at the row's time on the cubic Hermite curve through its own kept rows -> (section[total, 4] =
    the area vector of the triangle (m^2) and its component along the row's group velocity, A_perp, signed; flag[total] int32:
    0 ok, 1 no tube, 2 bad centre row, 3 a neighbour has no row at this time, 4 a neighbour's row or interval is unusable,
    5 no group velocity).  The flux of a tube of power P is P magnitude^2 / |A_perp|."""
    offsets, rows = _packed(offsets, rows)
    n, total = offsets.size - 1, int(offsets[-1])
    nb = neighbour_table(neighbours, n)
    section = np.full((max(total, 0), 4), np.nan)
    flag = np.ones(max(total, 0), dtype=np.int32)
    _check(lib().srt_tubes(n, nb.ctypes.data_as(C.POINTER(C.c_int64)), offsets.ctypes.data_as(C.POINTER(C.c_int64)), _dp(rows),
                           _dp(section), flag.ctypes.data_as(ip)))
    return section, flag


def tubes_padded(rows, nrows, outputper, neighbours):
    """tubes() of rows[n, slots, 20], nrows[n] as Model.trace returns them: packs first."""
    offsets, packed = pack_rows(rows, nrows, outputper)
    return tubes(offsets, packed, neighbours)


def write_tubes_file(path, raynum, offsets, rows, section, flag):
    """One record per packed row whose flag is not 1, (3 i10, 5 es24.15e3): raynum[ray], the row's index in its ray + 1, the flag,
    t, the area vector, A_perp."""
    offsets, rows = _packed(offsets, rows)
    total = int(offsets[-1])
    raynum = np.ascontiguousarray(raynum, dtype=np.int64).reshape(-1)
    section = _f64(section).reshape(-1, 4)
    flag = np.ascontiguousarray(flag, dtype=np.int32).reshape(-1)
    if len(raynum) != offsets.size - 1 or len(section) < total or len(flag) < total:
        raise ValueError("raynum, section and flag name %d rays, %d and %d rows: the packed set has %d rays, %d rows"
                         % (len(raynum), len(section), len(flag), offsets.size - 1, total))
    _check(lib().srt_tubes_file_write(os.fsencode(path), offsets.size - 1, raynum.ctypes.data_as(C.POINTER(C.c_int64)),
                                      offsets.ctypes.data_as(C.POINTER(C.c_int64)), _dp(rows), _dp(section), flag.ctypes.data_as(ip)))


def tube_frame(direction):
    """The two vectors across a ray that tube_fan offsets along, for direction[n, 3] -> (u[n, 3], v[n, 3]).  With d = direction /
    |direction| and e the coordinate axis along which |d| is smallest (the first such axis of x, y, z): u = (d x e) / |d x e|,
    v = (d x u) / |d x u|.  u, v and d are unit and perpendicular to one another, and u x v = d."""
    d = _f64(direction).reshape(-1, 3)
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    e = np.zeros_like(d)
    e[np.arange(len(d)), np.argmin(np.abs(d), axis=1)] = 1.0
    u = np.cross(d, e)
    u = u / np.sqrt((u * u).sum(axis=1))[:, None]
    v = np.cross(d, u)
    v = v / np.sqrt((v * v).sum(axis=1))[:, None]
    return u, v


def tube_fan(pos0, dir0, w0, delta_pos=None, delta_angle=None):
    """A launch set whose rays carry their own tubes: each ray of (pos0[n, 3], dir0[n, 3], w0[n]) is followed by two companions
    -> (pos[3n, 3], dir[3n, 3], w[3n], neighbours[3n, 2]); ray k of the input is ray 3k of the set, its companions b and c are
    3k + 1 and 3k + 2, neighbours[3k] = (3k + 1, 3k + 2) and the companions have no tube of their own (-1, -1).
    With (u, v) = tube_frame(dir0) and d = dir0 / |dir0|:
      delta_pos (metres):    b starts at pos0 + delta_pos u, c at pos0 + delta_pos v, so that the section at t = 0 is
                             1/2 delta_pos^2 d;
      delta_angle (radians): b starts along d cos(delta_angle) + u sin(delta_angle) (d turned about v), c along
                             d cos(delta_angle) + v sin(delta_angle) (d turned about -u), scaled to |dir0|.
    Either or both may be given, not neither.  The companions keep the ray's frequency."""
    if delta_pos is None and delta_angle is None:
        raise ValueError("tube_fan: give delta_pos (metres), delta_angle (radians) or both")
    pos0, dir0, w0 = _f64(pos0).reshape(-1, 3), _f64(dir0).reshape(-1, 3), _f64(w0).reshape(-1)
    n = len(w0)
    if not (len(pos0) == len(dir0) == n):
        raise ValueError("pos0, dir0 and w0 name %d, %d and %d rays" % (len(pos0), len(dir0), n))
    u, v = tube_frame(dir0)
    pos = np.repeat(pos0, 3, axis=0)
    direction = np.repeat(dir0, 3, axis=0)
    if delta_pos is not None:
        pos[1::3] = pos0 + float(delta_pos) * u
        pos[2::3] = pos0 + float(delta_pos) * v
    if delta_angle is not None:
        c, s = np.cos(float(delta_angle)), np.sin(float(delta_angle))
        norm = np.sqrt((dir0 * dir0).sum(axis=1))[:, None]
        direction[1::3] = dir0 * c + norm * s * u
        direction[2::3] = dir0 * c + norm * s * v
    neighbours = np.full((3 * n, 2), -1, dtype=np.int64)
    neighbours[0::3, 0] = 3 * np.arange(n) + 1
    neighbours[0::3, 1] = 3 * np.arange(n) + 2
    return pos, direction, np.repeat(w0, 3), neighbours


# ---- traced rays binned onto a grid: dwell time and power maps (include/srt.h) -------
AXIS_KINDS = {"x": 0, "y": 1, "z": 2, "r": 3, "rho": 4, "L": 5, "sinlat": 6, "mlt": 7}


def axis(kind_name, edges):
    """An axis of a binning grid: kind_name of AXIS_KINDS (x y z r rho in metres, dipole L, sinlat = z / r, mlt in hours) and
    its n + 1 increasing edges -> (kind, edges as float64)."""
    if kind_name not in AXIS_KINDS:
        raise ValueError("unknown axis kind %r (one of %s)" % (kind_name, " ".join(AXIS_KINDS)))
    return AXIS_KINDS[kind_name], _f64(edges).reshape(-1).copy()


def axis_maglat(edges_rad):
    """An axis of magnetic latitude from edges in radians: the sines are taken here (monotone on [-pi/2, pi/2]), as maglat()
    does for a surface."""
    e = _f64(edges_rad).reshape(-1)
    if not np.all(np.abs(e) <= np.pi / 2):
        raise ValueError("latitude edges lie within -pi/2 .. pi/2 radians")
    return AXIS_KINDS["sinlat"], np.sin(e)


def bin_params(axes, nsub=8, quantum=2.0 ** -30):
    """A sequence of axis() results -> BinParams (it keeps the edge arrays alive as ._edges)."""
    axes = list(axes)
    p = BinParams()
    p.naxes, p.nsub, p.quantum = len(axes), int(nsub), float(quantum)
    p._edges = []
    for a, (kind, edges) in enumerate(axes[:3]):
        e = _f64(edges).reshape(-1)
        p._edges.append(e)
        p.axis[a] = BinAxis(int(kind), e.size - 1, _dp(e))
    return p


def bin_shape(p):
    """The numpy shape of a map of BinParams p: [n2][n1][n0] with absent axes dropped."""
    return tuple(int(p.axis[a].n) for a in range(p.naxes))[::-1]


def bin_cells(p):
    n = C.c_int64()
    _check(lib().srt_bin_cells(C.byref(p), C.byref(n)))
    return n.value


def bin_rays(offsets, rows, axes, nsub=8, quantum=2.0 ** -30, row_weight=None, ray_weight=None):
    """The rays of a packed row set (offsets[n+1], rows[offsets[n], 20]) binned onto the grid of `axes` (axis(), axis_maglat()):
    every interval of consecutive kept rows is cut into nsub pieces on the cubic Hermite curve, and each piece deposits its
    weight x duration into the cell of its midpoint, in integer ticks of `quantum` seconds.  row_weight[offsets[n]] and
    ray_weight[n] are optional.  -> dict(sum = ticks * quantum as float64, ticks, hits (int64), all shaped [n2][n1][n0] with
    absent axes dropped, and counters[4] = intervals used, intervals skipped, samples deposited, samples outside)."""
    offsets, rows = _packed(offsets, rows)
    n = offsets.size - 1
    rw = yw = None
    if row_weight is not None:
        rw = _f64(row_weight).reshape(-1)
        if rw.size < offsets[-1]:
            raise ValueError("offsets name %d rows, row_weight holds %d" % (offsets[-1], rw.size))
    if ray_weight is not None:
        yw = _f64(ray_weight).reshape(-1)
        if yw.size != n:
            raise ValueError("ray_weight holds %d entries for %d rays" % (yw.size, n))
    p = bin_params(axes, nsub, quantum)
    i64p = C.POINTER(C.c_int64)
    pt, ph = i64p(), i64p()
    counters = np.zeros(4, dtype=np.int64)
    _check(lib().srt_bin_rays(C.byref(p), n, offsets.ctypes.data_as(i64p), _dp(rows), _dp(rw) if rw is not None else None,
                              _dp(yw) if yw is not None else None, C.byref(pt), C.byref(ph), counters.ctypes.data_as(i64p)))
    nc, shape = bin_cells(p), bin_shape(p)
    ticks, hits = (a.reshape(shape) for a in _take((pt, (nc,), np.int64), (ph, (nc,), np.int64)))
    return {"sum": ticks.astype(np.float64) * float(quantum), "ticks": ticks, "hits": hits, "counters": counters}


def bin_rays_padded(rows, nrows, outputper, axes, nsub=8, quantum=2.0 ** -30, row_weight_padded=None, ray_weight=None):
    """bin_rays() of rows[n, slots, 20], nrows[n] as Model.trace returns them: packs first, and packs row_weight_padded[n, slots]
    (e.g. the square of the magnitude damping() returns) with the rows."""
    offsets, packed = pack_rows(rows, nrows, outputper)
    rw = None
    if row_weight_padded is not None:
        w = _f64(row_weight_padded)
        n, slots = w.shape
        kept = np.diff(offsets)
        rw = w[np.arange(slots)[None, :] < kept[:, None]]
    return bin_rays(offsets, packed, axes, nsub, quantum, rw, ray_weight)


def write_bin_file(path, axes, ticks, hits, nsub=8, quantum=2.0 ** -30):
    """A map as text (include/srt.h): the grid, then per cell ticks * quantum (es24.15e3) and hits (i20)."""
    p = bin_params(axes, nsub, quantum)
    i64p = C.POINTER(C.c_int64)
    t = None if ticks is None else np.ascontiguousarray(ticks, dtype=np.int64).reshape(-1)
    h = None if hits is None else np.ascontiguousarray(hits, dtype=np.int64).reshape(-1)
    nc = bin_cells(p)
    for name, a in (("ticks", t), ("hits", h)):
        if a is not None and a.size != nc:
            raise ValueError("%s holds %d cells, the grid has %d" % (name, a.size, nc))
    _check(lib().srt_bin_file_write(os.fsencode(path), C.byref(p), t.ctypes.data_as(i64p) if t is not None else None,
                                    h.ctypes.data_as(i64p) if h is not None else None))


def read_bin_file(path):
    """-> dict(axes = [(kind, edges)], nsub, quantum, sum, hits), the maps shaped [n2][n1][n0] with absent axes dropped."""
    p = BinParams()
    i64p = C.POINTER(C.c_int64)
    pe, ps, ph, nc = dp(), dp(), i64p(), C.c_int64()
    _check(lib().srt_bin_file_read(os.fsencode(path), C.byref(p), C.byref(pe), C.byref(nc), C.byref(ps), C.byref(ph)))
    shape = bin_shape(p)
    try:  # (each axis' edges lie somewhere in the one array behind pe)
        axes = [(int(p.axis[a].kind), np.ctypeslib.as_array(p.axis[a].edges, (p.axis[a].n + 1,)).copy()) for a in range(p.naxes)]
    finally:
        lib().srt_free(pe)
        sums, hits = (a.reshape(shape) for a in _take((ps, (nc.value,)), (ph, (nc.value,), np.int64)))
    return {"axes": axes, "nsub": int(p.nsub), "quantum": float(p.quantum), "sum": sums, "hits": hits}


# ---- model-3 grid files: text of the reference's grid builder <-> binary side-format (host code, no GPU) -------
def read_grid_file(path):
    """-> dict(F[nz,ny,nx,nspec], bounds[6], qs, ms, derivs = None | [7] arrays of F's shape)."""
    dims = (C.c_int32 * 5)()
    bounds, qs, ms = np.zeros(6), np.zeros(4), np.zeros(4)
    pF, pD = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
    _check(lib().srt_grid_file_read(path.encode(), dims, _dp(bounds), _dp(qs), _dp(ms), C.byref(pF), C.byref(pD)))
    compder, nspec, nx, ny, nz = (int(v) for v in dims)
    n = nspec * nx * ny * nz
    try:
        F = np.ctypeslib.as_array(pF, shape=(n,)).copy().reshape(nz, ny, nx, nspec)
        derivs = None
        if compder:
            derivs = list(np.ctypeslib.as_array(pD, shape=(7 * n,)).copy().reshape(7, nz, ny, nx, nspec))
    finally:
        lib().srt_free(pF)
        if pD:
            lib().srt_free(pD)
    return {"F": F, "bounds": bounds, "qs": qs[:nspec], "ms": ms[:nspec], "derivs": derivs}


def write_grid_file(path, F, bounds, qs, ms, derivs=None, binary=False):
    F = _f64(F)
    nz, ny, nx, nspec = F.shape
    d = None
    if derivs is not None:
        d = _f64(np.stack([np.asarray(a, dtype=np.float64) for a in derivs]), (7, nz, ny, nx, nspec))
    q4, m4 = np.zeros(4), np.zeros(4)
    q4[:nspec], m4[:nspec] = qs[:nspec], ms[:nspec]
    _check(lib().srt_grid_file_write(path.encode(), int(binary), nspec, nx, ny, nz, _dp(_f64(bounds, (6,))), _dp(q4),
                                     _dp(m4), _dp(F), _dp(d) if d is not None else None))


def convert_grid_file(src, dst_binary):
    _check(lib().srt_grid_file_convert(src.encode(), dst_binary.encode()))


def grid_file_is_binary(path):
    return bool(lib().srt_grid_file_is_binary(path.encode()))


def sm_to_mag(x, yearday, msec, inverse=False):
    """xform_double's sm_to_mag_d (inverse: mag_to_sm_d) for x[n,3] at itime = (yearday, msec); host code, no GPU."""
    x = _f64(x, (-1, 3))
    out = np.empty_like(x)
    _check(lib().srt_sm_to_mag(int(yearday), int(msec), int(bool(inverse)), x.shape[0], _dp(x), _dp(out)))
    return out


# ---- dump files: the output of the reference's dumpmodel and of Model.dump (host code, no GPU) -------
def write_dump_file(path, f, bounds):
    """f[nz, ny, nx, 4*nspec+3] as Model.dump returns it -> the text file dumpmodel.f95 writes, byte for byte."""
    f = _f64(f)
    nz, ny, nx, per = f.shape
    if per % 4 != 3:
        raise ValueError("the last axis holds 4*nspec+3 values, not %d" % per)
    _check(lib().srt_dump_file_write(os.fsencode(path), (per - 3) // 4, nx, ny, nz, _dp(_f64(bounds, (6,))), _dp(f)))


def read_dump_file(path):
    """-> dict(f[nz, ny, nx, 4*nspec+3], bounds[6], nspec)."""
    dims = (C.c_int32 * 4)()
    bounds = np.zeros(6)
    pf = dp()
    _check(lib().srt_dump_file_read(os.fsencode(path), dims, _dp(bounds), C.byref(pf)))
    nspec, nx, ny, nz = (int(v) for v in dims)
    f = _take((pf, (nz * ny * nx * (4 * nspec + 3),)))[0].reshape(nz, ny, nx, 4 * nspec + 3)
    return {"f": f, "bounds": bounds, "nspec": nspec}


def write_points_file(path, records, bounds, qs, ms, binary=False):
    """Model-4 sample file from records[n, 3+nspec] (e.g. Model.build_samples' output): the reference builder's text
    layout, or the binary side-format."""
    rec = _f64(records)
    n, w = rec.shape
    _check(lib().srt_points_file_write(os.fsencode(path), int(bool(binary)), w - 3, n, _dp(_f64(bounds, (6,))),
                                       _dp(_f64(qs)), _dp(_f64(ms)), _dp(rec)))


def convert_points_file(src_text, dst_binary):
    _check(lib().srt_points_file_convert(os.fsencode(src_text), os.fsencode(dst_binary)))


def points_file_is_binary(path):
    return bool(lib().srt_points_file_is_binary(os.fsencode(path)))
