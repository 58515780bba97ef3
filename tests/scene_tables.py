"""The well-formed PpScene of the CPU ABI tests of pp_vsd_errors, pp_depth_refine and pp_scene_gt (no GPU: every call made with it is
rejected before a launch).  Two objects (4 vertices / 2 faces, 3 vertices / 1 face), two images, three views: a 10 x 10 window, a
window in the frame's far corner and an empty one: 200 window samples, 2 + 2 + 1 faces."""
import ctypes

from picopose_amd import _lib


def _arr(ty):
    return lambda *v: (ty * len(v))(*v)


i32, f32, i64 = _arr(ctypes.c_int), _arr(ctypes.c_float), _arr(ctypes.c_longlong)
WINDOW_SAMPLES, VIEW_FACES = 200, 5


def aligned_buffer(n=16384):
    """-> (the buffer, to be kept alive; a 256-byte aligned address inside it)."""
    buf = (ctypes.c_char * n)()
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256


def fields(p, H=48, W=64):
    """The members of the well-formed scene by name: every device table is the address `p`, every host table a ctypes array."""
    return dict(vertices=p, vert_off=p, faces=p, face_off=p, diameters=p, cams=p, view_obj=p, view_img=p, poses=p, windows=p, view_zoff=p,
                vert_off_host=i32(0, 4, 7), faces_host=i32(0, 1, 2, 0, 2, 3, 0, 1, 2), face_off_host=i32(0, 2, 3),
                diameters_host=f32(100.0, 50.0), cams_host=f32(100, 100, 32, 24, 90, 95, 30, 20), view_obj_host=i32(0, 0, 1),
                view_img_host=i32(0, 0, 1), windows_host=i32(0, 0, 10, 10, 54, 38, 64, 48, 5, 5, 5, 9), view_zoff_host=i64(0, 100, 200, 200),
                n_objects=2, n_images=2, H=H, W=W, n_views=3, near=1.0)


DEVICE_TABLES = tuple(fields(0))[:11]
HOST_TABLES = tuple(k for k in fields(0) if k.endswith("_host"))


def pack(values):
    """fields()-shaped dict (a member may be None: a null pointer) -> _lib.PpScene; the arrays stay alive with the struct."""
    s = _lib.PpScene()
    s.keep = dict(values)
    for k, v in values.items():
        setattr(s, k, ctypes.addressof(v) if isinstance(v, ctypes.Array) else v)
    return s


def caller(entry, scene_fields, own):
    """-> call(**changes): `entry` with the scene and its own arguments (a dict in the ABI's order), each changed by name; scene=None
    passes a null scene.  The stream is null."""
    def call(scene="packed", **kw):
        assert set(kw) <= set(scene_fields) | set(own), kw
        sc = pack({k: kw.get(k, v) for k, v in scene_fields.items()})
        return entry(ctypes.byref(sc) if scene == "packed" else scene, *[kw.get(k, v) for k, v in own.items()], None)
    return call
