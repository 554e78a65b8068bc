"""refprobe.py — one Python face for two libraries that export the same batched probes (TEST INFRASTRUCTURE ONLY):

  Probes("ref")     oracle/_ref/libref_probe.so: the reference's own sources compiled for the CPU (oracle/build.py build_ref)
  Probes("oracle")  oracle/_build/liboracle.so:  oracle.cpp's restatement (the oracle_fn_* probes)

Every method takes and returns float32 / int32 / uint32 numpy arrays, n cases per call. Scene probes act on the scene last given
to use_scene() (a ptss_types.SceneDesc) or, for "ref" only, built by build_scene()."""
import ctypes as C
import os

import numpy as np

import oracle as _oracle
from ptss_types import AreaLight, Camera, Material, PointLight, SceneDesc, Sphere, Triangle

HERE = os.path.dirname(os.path.abspath(__file__))
REF_LIB = os.path.join(HERE, "_ref", "libref_probe.so")
DIM = 512   # CudaUtils.h:7

SPHERE_DTYPE = np.dtype([("position", np.float32, 3), ("radius", np.float32), ("materialIdx", np.int32)])
TRIANGLE_DTYPE = np.dtype([("vertex0", np.float32, 3), ("vertex1", np.float32, 3), ("vertex2", np.float32, 3), ("normal0", np.float32, 3),
                           ("normal1", np.float32, 3), ("normal2", np.float32, 3), ("materialIdx", np.int32)])
MATERIAL_DTYPE = np.dtype([("diffuseColor", np.float32, 3), ("specularColor", np.float32, 3), ("absorption", np.float32, 3),
                           ("emmitance", np.float32, 3), ("specularExponent", np.float32), ("indexOfRefraction", np.float32),
                           ("diffAvg", np.float32), ("specAvg", np.float32), ("refrAvg", np.float32), ("roughness", np.float32),
                           ("flags", np.int8), ("pad", np.int8, 3)])
POINT_LIGHT_DTYPE = np.dtype([("position", np.float32, 3), ("power", np.float32, 3)])
AREA_LIGHT_DTYPE = np.dtype([("power", np.float32, 3), ("area", np.float32), ("triangleIdx", np.int32), ("pad", np.int32),
                             ("numTriangles", np.uint64)])
assert SPHERE_DTYPE.itemsize == C.sizeof(Sphere) and TRIANGLE_DTYPE.itemsize == C.sizeof(Triangle)
assert MATERIAL_DTYPE.itemsize == C.sizeof(Material) and POINT_LIGHT_DTYPE.itemsize == C.sizeof(PointLight)
assert AREA_LIGHT_DTYPE.itemsize == C.sizeof(AreaLight)
TABLES = (("spheres", SPHERE_DTYPE), ("triangles", TRIANGLE_DTYPE), ("materials", MATERIAL_DTYPE), ("pointLights", POINT_LIGHT_DTYPE),
          ("areaLights", AREA_LIGHT_DTYPE))


def reference_dir():
    return os.environ.get("PTSS_REFERENCE_DIR", "/root/reference")


def availability():
    """"built" | "missing" (the reference is there, its library is not: a failed build) | "absent" (neither exists)."""
    if os.path.exists(REF_LIB):
        return "built"
    return "missing" if os.path.isdir(os.path.join(reference_dir(), "CudaTracer")) else "absent"


def scene_tables(desc):
    """The five tables of a SceneDesc as structured numpy arrays (copies)."""
    out = {}
    for (name, dt), (ptr, n) in zip(TABLES, ((desc.spheres, desc.numSpheres), (desc.triangles, desc.numTriangles),
                                             (desc.materials, desc.numMaterials), (desc.pointLights, desc.numPointLights),
                                             (desc.areaLights, desc.numAreaLights))):
        a = np.zeros(n, dtype=dt)
        if n:
            C.memmove(a.ctypes.data, ptr, n * dt.itemsize)
        out[name] = a
    return out


def desc_of_tables(tables):
    """A SceneDesc over structured arrays (kept alive on the returned object)."""
    d = SceneDesc()
    keep = {k: np.ascontiguousarray(v) for k, v in tables.items()}
    for (name, _), (pf, nf, ct) in zip(TABLES, (("spheres", "numSpheres", Sphere), ("triangles", "numTriangles", Triangle),
                                                ("materials", "numMaterials", Material), ("pointLights", "numPointLights", PointLight),
                                                ("areaLights", "numAreaLights", AreaLight))):
        a = keep[name]
        setattr(d, pf, C.cast(a.ctypes.data, C.POINTER(ct)))
        setattr(d, nf, len(a))
    d._keep = keep
    return d


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cam10(cam):
    return np.frombuffer(bytes(cam), dtype=np.float32).copy()


class Probes:
    def __init__(self, which):
        assert which in ("ref", "oracle")
        self.which = which
        self.is_ref = which == "ref"
        if self.is_ref:
            if not os.path.exists(REF_LIB):
                raise RuntimeError(f"{REF_LIB} missing: run `python __graft_entry__.py build` with the reference in {reference_dir()}")
            self.L = C.CDLL(REF_LIB)
            self.prefix = "ref_"
            self.L.ref_frames_create.restype = C.c_void_p
        else:
            self.L = _oracle.lib()
            self.prefix = "oracle_fn_"
        self._ctx = None
        self._desc = None

    def _fn(self, name):
        fn = getattr(self.L, self.prefix + name)
        fn.restype = None
        return fn

    def _scene_args(self):
        if self.is_ref:
            return []
        assert self._ctx, "use_scene() first"
        return [C.c_void_p(self._ctx)]

    # ---- scenes ----------------------------------------------------------------------------------------
    def use_scene(self, desc):
        self._desc = desc
        if self.is_ref:
            self.L.ref_set_scene(desc.spheres, C.c_size_t(desc.numSpheres), desc.triangles, C.c_size_t(desc.numTriangles), desc.materials,
                                 C.c_size_t(desc.numMaterials), desc.pointLights, C.c_size_t(desc.numPointLights), desc.areaLights,
                                 C.c_size_t(desc.numAreaLights))
        else:
            self.close()
            self.L.oracle_create.restype = C.c_void_p
            self._ctx = self.L.oracle_create(C.byref(desc), 1, 1, 1, 1, 0, 1)

    def close(self):
        if self._ctx and not self.is_ref:
            self.L.oracle_destroy(C.c_void_p(self._ctx))
        self._ctx = None

    def build_scene(self, kind):
        """ref only. kind 0: Scene::build(); 1: addDefinedSpheres(4) + addCornellBox(8). Returns the five tables."""
        assert self.is_ref
        self.L.ref_build_scene.restype = C.c_int
        assert self.L.ref_build_scene(kind) == 0
        counts = (C.c_size_t * 5)()
        self.L.ref_scene_counts(counts)
        out = {name: np.zeros(counts[k], dtype=dt) for k, (name, dt) in enumerate(TABLES)}
        self.L.ref_scene_copy(*[_p(out[name]) for name, _ in TABLES])
        out["materials"]["pad"] = 0
        out["areaLights"]["pad"] = 0
        return out

    # ---- functions ---------------------------------------------------------------------------------------
    def _isect(self, name, prim, rays, tmax, update):
        rays = _f(rays)
        n = len(rays)
        tmax = _f(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,)))
        hit, out = np.zeros(n, np.int32), np.zeros((n, 8), np.float32)
        self._fn(name)(n, _p(_f(prim)), _p(rays), _p(tmax), 1 if update else 0, _p(hit), _p(out))
        return hit.astype(bool), out

    def sphere(self, sph4, rays, tmax=np.inf, update=True):
        return self._isect("sphere", sph4, rays, tmax, update)

    def triangle(self, tri18, rays, tmax=np.inf, update=True):
        return self._isect("triangle", tri18, rays, tmax, update)

    def closest_hit(self, rays, tmax=np.inf):
        rays = _f(rays)
        n = len(rays)
        tmax = _f(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,)))
        kind, prim, out = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 8), np.float32)
        self._fn("closest_hit")(*self._scene_args(), n, _p(rays), _p(tmax), _p(kind), _p(prim), _p(out))
        return kind, prim, out

    def line_of_sight(self, normal, p0, p1):
        normal, p0, p1 = _f(normal), _f(p0), _f(p1)
        n = len(p0)
        vis, out = np.zeros(n, np.int32), np.zeros((n, 4), np.float32)
        self._fn("line_of_sight")(*self._scene_args(), n, _p(normal), _p(p0), _p(p1), _p(vis), _p(out))
        return vis.astype(bool), out

    def fresnel(self, refr_index, cos_i):
        a, b = _f(refr_index), _f(cos_i)
        out = np.zeros((len(a), 6), np.float32)
        self._fn("fresnel")(len(a), _p(a), _p(b), _p(out))
        return out

    def refl_surfel(self, direction, point, normal, cos_i):
        d, p, nn, c = _f(direction), _f(point), _f(normal), _f(cos_i)
        out = np.zeros((len(d), 6), np.float32)
        self._fn("refl_surfel")(len(d), _p(d), _p(p), _p(nn), _p(c), _p(out))
        return out

    def refl_normal(self, direction, point, normal):
        d, p, nn = _f(direction), _f(point), _f(normal)
        out = np.zeros((len(d), 6), np.float32)
        self._fn("refl_normal")(len(d), _p(d), _p(p), _p(nn), _p(out))
        return out

    def refr(self, direction, point, normal, cos_i, sin_t2, n_ratio):
        d, p, nn, c, s, r = _f(direction), _f(point), _f(normal), _f(cos_i), _f(sin_t2), _f(n_ratio)
        act, out = np.zeros(len(d), np.int32), np.zeros((len(d), 6), np.float32)
        self._fn("refr")(len(d), _p(d), _p(p), _p(nn), _p(c), _p(s), _p(r), _p(act), _p(out))
        return act.astype(bool), out

    def rotate_v2v(self, source, target):
        s, t = _f(source), _f(target)
        out = np.zeros((len(s), 4), np.float32)
        self._fn("rotate_v2v")(len(s), _p(s), _p(t), _p(out))
        return out

    def sampler(self, kind, axis, param, seed):
        a = _f(axis)
        prm = _f(np.broadcast_to(np.asarray(param, dtype=np.float32), (len(a),)))
        out, st = np.zeros((len(a), 3), np.float32), np.zeros((len(a), 6), np.uint32)
        self._fn("sampler")(kind, len(a), _p(a), _p(prm), C.c_ulonglong(seed), _p(out), _p(st))
        return out, st

    def area_light_point(self, light, seed):
        li = _i(light)
        out, st = np.zeros((len(li), 3), np.float32), np.zeros((len(li), 6), np.uint32)
        self._fn("area_light_point")(*self._scene_args(), len(li), _p(li), C.c_ulonglong(seed), _p(out), _p(st))
        return out, st

    def shade(self, point, normal, material_idx, seed):
        p, nn, m = _f(point), _f(normal), _i(material_idx)
        out, st = np.zeros((len(p), 3), np.float32), np.zeros((len(p), 6), np.uint32)
        self._fn("shade")(*self._scene_args(), len(p), _p(p), _p(nn), _p(m), C.c_ulonglong(seed), _p(out), _p(st))
        return out, st

    def eye_ray(self, x, y, cam, seed):
        """At DIM x DIM (the reference's size is fixed)."""
        x, y = _i(x), _i(y)
        out, st = np.zeros((len(x), 6), np.float32), np.zeros((len(x), 6), np.uint32)
        if self.is_ref:
            c = cam10(cam)
            self._fn("eye_ray")(len(x), _p(x), _p(y), _p(c), C.c_ulonglong(seed), _p(out), _p(st))
        else:
            self._fn("eye_ray")(len(x), _p(x), _p(y), DIM, DIM, C.byref(cam), C.c_ulonglong(seed), _p(out), _p(st))
        return out, st

    def scatter(self, direction, point, normal, materials, cos_i, distance, seed):
        d, p, nn, c, dist = _f(direction), _f(point), _f(normal), _f(cos_i), _f(distance)
        mats = np.ascontiguousarray(materials)
        assert mats.dtype == MATERIAL_DTYPE and len(mats) == len(d)
        act, out, st = np.zeros(len(d), np.int32), np.zeros((len(d), 9), np.float32), np.zeros((len(d), 6), np.uint32)
        self._fn("scatter")(len(d), _p(d), _p(p), _p(nn), _p(mats), _p(c), _p(dist), C.c_ulonglong(seed), _p(act), _p(out), _p(st))
        return act.astype(bool), out, st

    def tonemap(self, radiance):
        r = _f(radiance)
        out = np.zeros(len(r), np.uint32)
        self._fn("tonemap")(len(r), _p(r), _p(out))
        return out

    # ---- ref only -----------------------------------------------------------------------------------------
    def any_hit(self, rays, tmax):
        assert self.is_ref
        rays = _f(rays)
        tmax = _f(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (len(rays),)))
        out = np.zeros(len(rays), np.int32)
        self.L.ref_any_hit(len(rays), _p(rays), _p(tmax), _p(out))
        return out.astype(bool)

    def move_camera(self, cam, key):
        """Returns (moved, Camera afterwards); `cam` is left alone."""
        assert self.is_ref
        c = cam10(cam)
        self.L.ref_move_camera.restype = C.c_int
        moved = self.L.ref_move_camera(_p(c), ord(key))
        out = Camera()
        C.memmove(C.byref(out), c.ctypes.data, C.sizeof(Camera))
        return bool(moved), out

    def default_camera(self):
        assert self.is_ref
        c = np.zeros(10, np.float32)
        self.L.ref_default_camera(_p(c))
        out = Camera()
        C.memmove(C.byref(out), c.ctypes.data, C.sizeof(Camera))
        return out

    def rng(self, seed, sequence, n):
        assert self.is_ref
        state, raw, uni = np.zeros(6, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
        self.L.ref_rng(C.c_ulonglong(seed), C.c_uint(sequence), n, _p(state), _p(raw), _p(uni))
        return state, raw, uni


class RefFrames:
    """The reference's generateFrame loop on the CPU, DIM x DIM, over the scene the "ref" Probes hold."""

    def __init__(self, probes, seed, use_path_tracer=True, max_iterations=15):
        assert probes.is_ref and seed < 2 ** 32   # curand_init gets (unsigned int)clock64(), CudaTracer.cu:28
        self.L = probes.L
        self.L.ref_set_threads(_oracle.cpu_share())
        self._h = C.c_void_p(self.L.ref_frames_create(C.c_uint(seed), 1 if use_path_tracer else 0))
        self.L.ref_frames_set_max_iterations(self._h, C.c_uint(max_iterations))   # ProgramData::maxIterations, CudaTracer.h:39
        self.ticks = 1
        self.n = DIM * DIM

    def generate_frame(self):
        self.L.ref_frames_step(self._h, self.ticks)
        self.ticks += 1

    def accumulator(self):
        out = np.zeros((self.n, 3), np.uint32)
        self.L.ref_frames_totals(self._h, _p(out))
        return out

    def pixels(self):
        out = np.zeros((self.n, 4), np.uint8)
        self.L.ref_frames_pixels(self._h, _p(out))
        return out

    def launched_counts(self):
        buf = (C.c_long * 65)()
        n = self.L.ref_frames_counts(self._h, buf, 65)
        return np.array(buf[:n], dtype=np.int64)

    def live_counts(self):
        buf = (C.c_long * 65)()
        n = self.L.ref_frames_live(self._h, buf, 65)
        return np.array(buf[:n], dtype=np.int64)

    def close(self):
        if self._h:
            self.L.ref_frames_destroy(self._h)
            self._h = None
