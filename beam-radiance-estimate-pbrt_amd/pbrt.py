"""Python view of libbre_host.so (include/bre_pbrt.h): the .pbrt scene front end, the
photon-beam integrator's Render on the GPU, and the film / PFM output.

    sc = pbrt.parse_file("scenes/cornell_fog_c2.pbrt")   # pbrtParseFile (api.cpp, pbrtparse.y)
    sc.scene, sc.params, sc.film                          # bre_scene, bre_render_params, film
    img = sc.render(device=0, write_files=False)          # WorldEnd -> PhotonBeamIntegrator::Render

The parser, integrator mirror and film code are C++ (host/pbrt_scene.cpp, host/photonbeam_gpu.cpp);
this module only declares their C signatures.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import load_library
from .scene import Light, Material, MaterialEx, Medium, RenderParams, Scene

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(HERE, "libbre_host.so")
CLI_PATH = os.path.join(HERE, "host", "bre_pbrt")

PBRT_MEDIA = 1  # BRE_PBRT_MEDIA
PBRT_LIGHTS = 2  # BRE_PBRT_LIGHTS: LightSource "distant" and "point", two-sided area lights
PBRT_MATERIALS = 4  # BRE_PBRT_MATERIALS: rough glass, direct Material "glass", "uber", "translucent", "substrate", "mix",
#                     "subsurface" / "kdsubsurface" (their dielectric boundary)
EXPORTS = ["bre_pbrt_parse_file", "bre_pbrt_parse_string", "bre_pbrt_parse_file_ex", "bre_pbrt_parse_string_ex",
           "bre_pbrt_get_media", "bre_pbrt_free", "bre_pbrt_messages",
           "bre_pbrt_get_scene", "bre_pbrt_get_lights", "bre_pbrt_get_materials", "bre_pbrt_get_materials_ex", "bre_pbrt_make_spot_light", "bre_pbrt_get_render_params", "bre_pbrt_get_film", "bre_pbrt_render",
           "bre_pbrt_render_devices", "bre_film_finalize", "bre_write_pfm", "bre_read_pfm"]

_HOST = None


def load_host_library(path: str = HOST_LIB_PATH) -> ctypes.CDLL:
    global _HOST
    if _HOST is not None:
        return _HOST
    load_library()  # libbre.so first (torch's HIP runtime ordering, see load_library)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build it with `make -C {HERE}/host`")
    lib = ctypes.CDLL(path)
    P, I64, I32, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    lib.bre_pbrt_parse_file.argtypes = [ctypes.c_char_p, ctypes.POINTER(P)]
    lib.bre_pbrt_parse_string.argtypes = [ctypes.c_char_p, ctypes.POINTER(P)]
    lib.bre_pbrt_parse_file_ex.argtypes = [ctypes.c_char_p, I32, ctypes.POINTER(P)]
    lib.bre_pbrt_parse_string_ex.argtypes = [ctypes.c_char_p, I32, ctypes.POINTER(P)]
    lib.bre_pbrt_get_media.argtypes = [P, I32, P, ctypes.POINTER(I32), I64, P, P, ctypes.POINTER(I64),
                                       ctypes.POINTER(I32), I32, P, ctypes.POINTER(I32)]
    lib.bre_pbrt_free.argtypes = [P]
    lib.bre_pbrt_free.restype = None
    lib.bre_pbrt_messages.argtypes = [P, ctypes.POINTER(I32), ctypes.POINTER(I32)]
    lib.bre_pbrt_messages.restype = ctypes.c_char_p
    lib.bre_pbrt_get_scene.argtypes = [P, P]
    lib.bre_pbrt_get_lights.argtypes = [P, I32, P, ctypes.POINTER(I32)]
    lib.bre_pbrt_get_materials.argtypes = [P, I32, P, ctypes.POINTER(I32), I64, P, ctypes.POINTER(I64)]
    lib.bre_pbrt_get_materials_ex.argtypes = [P, I32, P, ctypes.POINTER(I32), I64, P, ctypes.POINTER(I64)]
    lib.bre_pbrt_make_spot_light.argtypes = [P, P, P, F, F, P, P, I32, P]
    lib.bre_pbrt_get_render_params.argtypes = [P, I32, P, ctypes.POINTER(I32)]
    lib.bre_pbrt_get_film.argtypes = [P, ctypes.POINTER(I32), ctypes.POINTER(I32), ctypes.POINTER(F),
                                      ctypes.c_char_p, I32]
    lib.bre_pbrt_render.argtypes = [P, I32, I32, ctypes.c_char_p, I32, P]
    lib.bre_pbrt_render_devices.argtypes = [P, ctypes.POINTER(I32), I32, I32, ctypes.c_char_p, I32, P]
    lib.bre_film_finalize.argtypes = [I64, P, F, P]
    lib.bre_write_pfm.argtypes = [ctypes.c_char_p, P, I32, I32]
    lib.bre_read_pfm.argtypes = [ctypes.c_char_p, P, I64, ctypes.POINTER(I32), ctypes.POINTER(I32)]
    for n in EXPORTS:
        if n not in ("bre_pbrt_free", "bre_pbrt_messages"):
            getattr(lib, n).restype = I32
    _HOST = lib
    return lib


class PbrtError(RuntimeError):
    pass


class PbrtScene:
    """A parsed scene (owns the C handle)."""

    def __init__(self, handle, ok: bool, quick: bool = False):
        self._lib = load_host_library()
        self._h = handle
        ne, nw = ctypes.c_int32(), ctypes.c_int32()
        self.messages = self._lib.bre_pbrt_messages(self._h, ctypes.byref(ne), ctypes.byref(nw)).decode()
        self.n_errors, self.n_warnings = ne.value, nw.value
        self.ok = ok
        self.quick = quick
        if not ok:
            return
        self.scene = Scene()
        assert self._lib.bre_pbrt_get_scene(self._h, ctypes.byref(self.scene)) == 0
        n = ctypes.c_int32()
        assert self._lib.bre_pbrt_get_lights(self._h, 0, None, ctypes.byref(n)) == 0
        arr = (Light * max(n.value, 1))()
        assert self._lib.bre_pbrt_get_lights(self._h, n.value, arr, ctypes.byref(n)) == 0
        # LightSource "spot" (with lights=True also "point" and "distant"), for BeamGather.set_lights
        self.lights = [arr[i] for i in range(n.value)]
        self._lights_ref = arr
        # mirror / glass materials and the per-triangle index into them, for BeamGather.set_materials
        nm, nt = ctypes.c_int32(), ctypes.c_int64()
        # .materials_ex: the table in its wide records (plastic, metal and matte with sigma are entries too);
        # .materials: the narrow records where the scene has none of those (bre_pbrt_get_materials: BRE_ERR_STATE
        # otherwise), else the wide ones
        assert self._lib.bre_pbrt_get_materials_ex(self._h, 0, None, ctypes.byref(nm), 0, None, ctypes.byref(nt)) == 0
        warr = (MaterialEx * max(nm.value, 1))()
        tm = np.full(nt.value, -1, np.int32)
        assert self._lib.bre_pbrt_get_materials_ex(self._h, nm.value, warr, None, nt.value,
                                                   tm.ctypes.data if nt.value else None, None) == 0
        self.materials_ex = [warr[i] for i in range(nm.value)]
        self.triangle_material = tm
        marr = (Material * max(nm.value, 1))()
        self.materials_status = self._lib.bre_pbrt_get_materials(self._h, nm.value, marr, None, 0, None, None)
        assert self.materials_status in (0, 4)
        self.materials = [marr[i] for i in range(nm.value)] if self.materials_status == 0 else self.materials_ex
        self._materials_ref = (marr, warr)
        # media bounded by surfaces (parse_*(..., media=True)), for BeamGather.set_media; the grids stay the handle's
        nd, nt, cm, nl = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        assert self._lib.bre_pbrt_get_media(self._h, 0, None, ctypes.byref(nd), 0, None, None, ctypes.byref(nt),
                                            ctypes.byref(cm), 0, None, ctypes.byref(nl)) == 0
        darr = (Medium * max(nd.value, 1))()
        ti, to = np.full(nt.value, -1, np.int32), np.full(nt.value, -1, np.int32)
        lm = np.full(nl.value, -1, np.int32)
        assert self._lib.bre_pbrt_get_media(self._h, nd.value, darr, None, nt.value, ti.ctypes.data if nt.value else None,
                                            to.ctypes.data if nt.value else None, None, None, nl.value,
                                            lm.ctypes.data if nl.value else None, None) == 0
        self.media = [darr[i] for i in range(nd.value)]
        self.tri_inside, self.tri_outside, self.camera_medium, self.light_medium = ti, to, cm.value, lm
        self._media_ref = darr
        self.params = RenderParams()
        wf = ctypes.c_int32()
        assert self._lib.bre_pbrt_get_render_params(self._h, int(quick), ctypes.byref(self.params), ctypes.byref(wf)) == 0
        self.write_frequency = wf.value
        w, h, sc = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_float()
        buf = ctypes.create_string_buffer(4096)
        assert self._lib.bre_pbrt_get_film(self._h, ctypes.byref(w), ctypes.byref(h), ctypes.byref(sc), buf, 4096) == 0
        self.film = dict(xres=w.value, yres=h.value, scale=sc.value, filename=buf.value.decode())

    def render(self, device: int = 0, outfile: str | None = None, write_files: bool = True,
               devices=None) -> np.ndarray:
        """PhotonBeamIntegrator::Render on GPU `device`, or split over the GPUs of `devices` (a list of
        ordinals, one context each; bre_pbrt_render_devices); returns the last film image (H, W, 3)."""
        if not self.ok:
            raise PbrtError(self.messages)
        img = np.zeros((self.film["yres"], self.film["xres"], 3), np.float32)
        out = outfile.encode() if outfile else None
        if devices is None:
            fn = "bre_pbrt_render"
            st = self._lib.bre_pbrt_render(self._h, int(device), int(self.quick), out, int(write_files),
                                           img.ctypes.data_as(ctypes.c_void_p))
        else:
            fn = "bre_pbrt_render_devices"
            dev = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
            st = self._lib.bre_pbrt_render_devices(self._h, dev, len(devices), int(self.quick), out, int(write_files),
                                                   img.ctypes.data_as(ctypes.c_void_p))
        if st != 0:
            raise PbrtError(f"{fn} failed with status {st}")
        return img

    def close(self):
        if self._h:
            self._lib.bre_pbrt_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _parse(fn, arg: bytes, quick: bool, media: bool, lights: bool = False, materials: bool = False) -> PbrtScene:
    lib = load_host_library()
    h = ctypes.c_void_p()
    if media or lights or materials:
        flags = (PBRT_MEDIA if media else 0) | (PBRT_LIGHTS if lights else 0) | (PBRT_MATERIALS if materials else 0)
        st = getattr(lib, fn + "_ex")(arg, flags, ctypes.byref(h))
    else:
        st = getattr(lib, fn)(arg, ctypes.byref(h))
    return PbrtScene(h, st == 0, quick)


def parse_file(path: str, quick: bool = False, media: bool = False, lights: bool = False,
               materials: bool = False) -> PbrtScene:
    """`media`: BRE_PBRT_MEDIA -- media bounded by surfaces are accepted (.media, .tri_inside, .tri_outside,
    .camera_medium, .light_medium on the result) instead of refused.
    `lights`: BRE_PBRT_LIGHTS -- LightSource "distant" and "point" and "bool twosided" "true" on an
    AreaLightSource "diffuse" are accepted instead of refused.
    `materials`: BRE_PBRT_MATERIALS -- Material "glass" with a roughness or as a direct statement, "uber",
    "translucent" and "substrate" become entries of .materials_ex instead of being reported."""
    return _parse("bre_pbrt_parse_file", os.fsencode(path), quick, media, lights, materials)


def parse_string(text: str, quick: bool = False, media: bool = False, lights: bool = False,
                 materials: bool = False) -> PbrtScene:
    return _parse("bre_pbrt_parse_string", text.encode(), quick, media, lights, materials)


def make_spot_light(frm, to, I, coneangle: float = 30.0, conedelta: float = 5.0, order: int = 0, ctm=None,
                    ctm_inv=None) -> Light:
    """bre_pbrt_make_spot_light: the bre_light CreateSpotLight (spot.cpp:104-124) builds for these
    parameters under the current transform `ctm` (4x4 row-major, None = identity; `ctm_inv` its tracked
    inverse, None = computed), by the parser's code."""
    F3 = ctypes.c_float * 3
    out = Light()
    mat = lambda a: None if a is None else (ctypes.c_float * 16)(*[float(v) for v in np.asarray(a, np.float32).reshape(-1)])  # noqa: E731
    m, mi = mat(ctm), mat(ctm_inv)
    st = load_host_library().bre_pbrt_make_spot_light(F3(*frm), F3(*to), F3(*I), float(coneangle), float(conedelta), m, mi,
                                                      int(order), ctypes.byref(out))
    if st != 0:
        raise PbrtError(f"bre_pbrt_make_spot_light failed with status {st}")
    return out


def film_finalize(L: np.ndarray, scale: float = 1.0) -> np.ndarray:
    """Film::SetImage(L) + Film::WriteImage's per-pixel conversion (film.cpp:132-210)."""
    L = np.ascontiguousarray(L, dtype=np.float32)
    out = np.empty_like(L)
    st = load_host_library().bre_film_finalize(L.size // 3, L.ctypes.data_as(ctypes.c_void_p), float(scale),
                                               out.ctypes.data_as(ctypes.c_void_p))
    if st != 0:
        raise PbrtError(f"bre_film_finalize failed with status {st}")
    return out


def write_pfm(path: str, rgb: np.ndarray) -> None:
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    if load_host_library().bre_write_pfm(os.fsencode(path), rgb.ctypes.data_as(ctypes.c_void_p), w, h) != 0:
        raise PbrtError(f"cannot write {path}")


def read_pfm(path: str) -> np.ndarray:
    lib = load_host_library()
    w, h = ctypes.c_int32(), ctypes.c_int32()
    if lib.bre_read_pfm(os.fsencode(path), None, 0, ctypes.byref(w), ctypes.byref(h)) != 0:
        raise PbrtError(f"cannot read {path}")
    out = np.empty((h.value, w.value, 3), np.float32)
    lib.bre_read_pfm(os.fsencode(path), out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(w), ctypes.byref(h))
    return out
