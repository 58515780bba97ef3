"""Onboarding an object from its mesh: the template bank rendered, cropped and featurised on the device.

Replaces the reference's offline step rendering/scripts/render_bop_templates.py -> rendering/src/custom_megapose/call_panda3d.py
(Panda3D inside MegaPose's image, 324 PNG files per object) followed by provider/bop_test_dataset.py:212-308 (`_get_template`,
`get_templates`) and run_test.py:120-134 (the bank features):

    mesh = load_model(path)                                  # PLY + the texture it names; or arrays of your own: {"vertices",
                                                             # "faces"} + "colors" or "texture" with "uv" / "face_uv"
    bank = onboard_objects(net, [mesh, ...], view_poses)     # templates_data + template_feature
    pipeline.infer_image(net, data, bank, indexed_bank=True)

The default render recipe is the reference's for LM-O, YCB-V, HB, IC-BIN and TUD-L (Panda3D): one ambient light of colour 1 (the
pixel is the surface colour, unshaded), TEMPLATE_K at
480 x 640, object pose = a view rotation with t = (0, 0, diameter), RGBA uint8 with alpha = 255 on the object, depth in whole
millimetres.  The rasteriser's conventions (pixel centres at integer coordinates, 1/256 px snapping, top-left fill rule, no
back-face culling, no near-plane clipping) are stated in include/picopose_hip.h; parity with Panda3D's or BlenderProc's pixels
is UNPINNED — neither renderer is available to compare against.

A UV-textured model (BOP's `obj_NNNNNN.ply` with `texture_u texture_v` or a per-face `texcoord` list, and `comment TextureFile
obj_NNNNNN.png`) is rendered from its texture, with no baking step: load_model reads the PLY and the image, a mip pyramid is built on
the device once per render call, and the resolve pass samples it perspective-correctly — one mip level per (view, face) chosen by
area, bilinear, wrap mode repeat, v = 0 at the bottom row (THE TEXTURE CONTRACT in include/picopose_hip.h, T1-T5).  Out of scope
(T6): anisotropic and trilinear filtering, clamp / mirror wrap, texture alpha, several textures per mesh.

The reference anti-aliases its templates (4x MSAA: panda3d_scene_renderer.py:72-73, :99), so its PNGs hold partial alpha along the
silhouette.  `render_views` / `render_templates` / `onboard_objects` take `samples=4` (THE MULTISAMPLE CONTRACT in
include/picopose_hip.h, M1-M6): four rotated-grid samples per pixel, every sample shaded (unlit, textured or lit), colour and alpha
their rounded integer mean, so alpha is one of 0, 64, 128, 191, 255 and colour fades to black at silhouettes; depth and face ids stay
those of the pixel centre.  The default samples=1 is byte for byte what it was.  Pixel parity with Panda3D stays unpinned and the
effect of the option on pose accuracy is UNMEASURED (no trained weights were available).

T-LESS and ITODD need shading: the reference renders their untextured CAD meshes (`models_cad`) with BlenderProc under eight point
lights (render_bop_templates.py:131, blenderproc.py:29-39) and, for T-LESS, a uniform grey 0.4 material (:54-57); unlit, such a
mesh — or any untextured CAD part of your own — is a flat silhouette with nothing for the features to match inside the outline.
`render_views` / `render_templates` / `onboard_objects` take `shading=` (a Shading, a dict of its fields, or "tless"): Lambert
diffuse plus ambient under up to 16 point lights, flat or smooth normals, an optional tone table, on top of any of the three colour
sources (THE SHADING CONTRACT in include/picopose_hip.h, S1-S8; out of scope, S9: specular terms, shadows, coloured or spot
lights, sRGB decoding of base colours, auto-smooth).  Shading is opt-in: without it every render is byte for byte what it was.
The package reads no fixture: `view_poses` is the caller's array (the reference's is
rendering/src/lib3d/predefined_poses/obj_poses_level1.npy, 162 views)."""
import ctypes
import dataclasses
import os

import numpy as np
import torch

from .. import _lib
from ..utils.preprocess import CLIP_MEAN, CLIP_STD, _square

TEMPLATE_K = np.array([[572.4114, 0.0, 320.0], [0.0, 573.57043, 240.0], [0.0, 0.0, 1.0]])     # call_panda3d.py:48-50
DEFAULT_WORKSPACE_BYTES = 256 << 20      # bound of the render workspace: 100 views of 480 x 640 for a 20 k-triangle mesh
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def load_ply(path):
    """A BOP model file -> {"vertices" (Nv,3) f32, "faces" (Nf,3) i32, "colors" (Nv,3) u8 or None, "uv" (Nv,2) f32 or None,
    "face_uv" (Nf,3,2) f32 or None, "normals" (Nv,3) f32 or None, "texture_file" str or None}.  ASCII and binary_little_endian PLY;
    element `vertex` with x y z (red green blue, nx ny nz and texture_u texture_v / s t / u v are returned; alpha and any other scalar
    property are skipped),
    element `face` with a `vertex_indices` / `vertex_index` list, optionally a `texcoord` list of 6 floats (u v per corner: MeshLab's
    wedge UVs) and scalar properties such as `texnumber`, which are skipped.  "texture_file" is the NAME in `comment TextureFile
    NAME`, as written (load_model resolves and reads it).
    ValueError: not a PLY file, big-endian, a missing element or property, a face that is not a triangle or whose texcoord list
    does not hold 6 values (named), a truncated body."""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic / 'end_header')")
    body = raw.find(b"\n", end) + 1
    fmt, elements, texture_file = None, [], None
    for line in raw[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if len(tok) >= 3 and tok[0] == "comment" and tok[1] == "TextureFile" and texture_file is None:
            texture_file = line.split(None, 2)[2].strip()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if tok[1] == "list":
                if tok[2] not in _PLY_TYPES or tok[3] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unknown PLY type in '{line}'")
                elements[-1][2].append((tok[4], (_PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
            else:
                if tok[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unknown PLY type in '{line}'")
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt == "binary_big_endian":
        raise ValueError(f"{path}: big-endian PLY is not supported")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: unknown PLY format {fmt!r}")
    names = [e[0] for e in elements]
    for need in ("vertex", "face"):
        if need not in names:
            raise ValueError(f"{path}: no '{need}' element")
    out = {"uv": None, "face_uv": None, "normals": None, "texture_file": texture_file}
    tokens, pos = (raw[body:].split(), 0) if fmt == "ascii" else (None, body)
    for name, count, props in elements:
        lists = [p for p in props if isinstance(p[1], tuple)]
        if name == "vertex":
            if lists:
                raise ValueError(f"{path}: list property in the vertex element")
            pn = [p[0] for p in props]
            for need in ("x", "y", "z"):
                if need not in pn:
                    raise ValueError(f"{path}: vertex element has no '{need}' property")
            if fmt == "ascii":
                if pos + count * len(props) > len(tokens):
                    raise ValueError(f"{path}: truncated vertex data")
                tab = np.array(tokens[pos:pos + count * len(props)], dtype=np.float64).reshape(count, len(props))
                pos += count * len(props)
                col = {n: tab[:, k] for k, n in enumerate(pn)}
            else:
                dt = np.dtype([(n, "<" + t) for n, t in props])
                if pos + count * dt.itemsize > len(raw):
                    raise ValueError(f"{path}: truncated vertex data")
                tab = np.frombuffer(raw, dtype=dt, count=count, offset=pos)
                pos += count * dt.itemsize
                col = {n: tab[n] for n in pn}
            out["vertices"] = np.ascontiguousarray(np.stack([col["x"], col["y"], col["z"]], axis=1).astype(np.float32))
            out["colors"] = (np.ascontiguousarray(np.stack([col["red"], col["green"], col["blue"]], axis=1).astype(np.uint8))
                             if all(c in col for c in ("red", "green", "blue")) else None)
            if all(c in col for c in ("nx", "ny", "nz")):
                out["normals"] = np.ascontiguousarray(np.stack([col["nx"], col["ny"], col["nz"]], axis=1).astype(np.float32))
            for un, vn in (("texture_u", "texture_v"), ("s", "t"), ("u", "v")):
                if un in col and vn in col:
                    out["uv"] = np.ascontiguousarray(np.stack([col[un], col[vn]], axis=1).astype(np.float32))
                    break
        elif name == "face":
            want = {p[0]: 6 if p[0] == "texcoord" else 3 for p in lists}
            index = [n for n in want if n in ("vertex_indices", "vertex_index")]
            if len(index) != 1 or len(want) != len(lists) or set(want) - {index[0], "texcoord"}:
                raise ValueError(f"{path}: face element must hold one 'vertex_indices' / 'vertex_index' list (besides it only a "
                                 "'texcoord' list and scalar properties are read past)")
            # every row has the same layout when each list has the length it should: read the table in one piece, and walk the
            # rows one by one only to name the first that differs
            if fmt == "ascii":
                width = sum(1 + want[n] if isinstance(t, tuple) else 1 for n, t in props)
                fits = pos + count * width <= len(tokens)
                if fits:
                    tab = np.array(tokens[pos:pos + count * width], dtype=np.float64).reshape(count, width)
                    col, o = {}, 0
                    for n, t in props:
                        if isinstance(t, tuple):
                            col[n] = (tab[:, o], tab[:, o + 1:o + 1 + want[n]])
                            o += want[n]
                        o += 1
                size = count * width
            else:
                dt = np.dtype([f for n, t in props for f in ([(n + "#", "<" + t[0]), (n, "<" + t[1], (want[n],))]
                                                             if isinstance(t, tuple) else [(n, "<" + t)])])
                fits = pos + count * dt.itemsize <= len(raw)
                if fits:
                    tab = np.frombuffer(raw, dtype=dt, count=count, offset=pos)
                    col = {n: (tab[n + "#"], tab[n]) for n in want}
                size = count * dt.itemsize
            if not fits or any(np.any(col[n][0] != want[n]) for n in want):
                _raise_on_face_rows(path, fmt, tokens if fmt == "ascii" else raw, pos, count, props, want)
            pos += size
            out["faces"] = np.ascontiguousarray(col[index[0]][1].astype(np.int32))
            if "texcoord" in want:
                out["face_uv"] = np.ascontiguousarray(col["texcoord"][1].astype(np.float32).reshape(count, 3, 2))
        else:                                                   # another element: skipped (fixed-size properties only)
            if lists:
                raise ValueError(f"{path}: cannot skip element '{name}' with a list property")
            if fmt == "ascii":
                pos += count * len(props)
            else:
                pos += count * np.dtype([(n_, "<" + t) for n_, t in props]).itemsize
    return out


def _raise_on_face_rows(path, fmt, data, pos, count, props, want):
    """Walk the face rows one by one and name the first whose list has another length than want[name], or the truncation."""
    def take(t):                                                 # the next scalar of PLY type t, None past the end
        nonlocal pos
        if fmt == "ascii":
            val = float(data[pos]) if pos < len(data) else None
            pos += 1
        else:
            dt = np.dtype("<" + t)
            val = np.frombuffer(data, dtype=dt, count=1, offset=pos)[0] if pos + dt.itemsize <= len(data) else None
            pos += dt.itemsize
        return val

    for row in range(count):
        for name, t in props:
            n = take(t[0] if isinstance(t, tuple) else t)
            if n is None:
                raise ValueError(f"{path}: truncated face data (or a face that is not a triangle)")
            if isinstance(t, tuple):
                if int(n) != want[name]:
                    raise ValueError(f"{path}: face {row} holds a texcoord list of {int(n)} values (6 expected: u v per corner)"
                                     if name == "texcoord" else f"{path}: face {row} is not a triangle ({int(n)} vertices)")
                for _ in range(want[name]):
                    take(t[1])
    raise ValueError(f"{path}: truncated face data (or a face that is not a triangle)")


def load_texture(path):
    """An image file -> (Ht, Wt, 3) uint8 RGB, row 0 the top row (PIL, `convert("RGB")`: alpha is dropped, a palette resolved)."""
    from PIL import Image

    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def load_model(ply_path, texture=None):
    """load_ply plus the model's texture under "texture": `texture` (a path or an (Ht, Wt, 3) uint8 array) when given, else the
    file that `comment TextureFile NAME` names, looked up next to the PLY.  A model without UVs or without a texture comes back as
    load_ply gives it.  ValueError: the named texture file does not exist (it says which)."""
    mesh = load_ply(ply_path)
    if texture is None and mesh["texture_file"] is not None and (mesh["uv"] is not None or mesh["face_uv"] is not None):
        texture = os.path.join(os.path.dirname(os.path.abspath(ply_path)), mesh["texture_file"])
        if not os.path.isfile(texture):
            raise ValueError(f"{ply_path}: its texture file {texture} (comment TextureFile {mesh['texture_file']}) does not exist")
    if isinstance(texture, (str, bytes)) or hasattr(texture, "__fspath__"):
        if not os.path.isfile(texture):
            raise ValueError(f"texture file {texture} does not exist")
        texture = load_texture(texture)
    if texture is not None:
        mesh["texture"] = texture
    return mesh


def mesh_diameter(vertices):
    """rendering/src/utils/trimesh.py:20-23: the norm of twice the axis-aligned extents, in the vertices' unit."""
    v = np.asarray(vertices, dtype=np.float64)
    return float(np.linalg.norm((v.max(axis=0) - v.min(axis=0)) * 2))


def template_object_poses(view_poses, vertices):
    """render_bop_templates.py:109-115: the view poses (V,4,4) with every translation replaced by (0, 0, diameter)."""
    poses = np.array(view_poses, dtype=np.float64)
    poses[:, :3, 3] = np.array([0.0, 0.0, mesh_diameter(vertices)])[None].repeat(len(poses), axis=0)
    return poses


def _mesh_arrays(mesh):
    v = np.asarray(mesh["vertices"])
    f = np.asarray(mesh["faces"])
    if v.ndim != 2 or v.shape[1] != 3 or len(v) == 0 or not np.issubdtype(v.dtype, np.floating):
        raise ValueError(f"vertices must be a non-empty (Nv, 3) float array, got {v.dtype} {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"faces must be a non-empty (Nf, 3) integer array, got {f.dtype} {f.shape}")
    if not np.all(np.isfinite(v)):
        raise ValueError("vertices contain a non-finite value")
    if f.min() < 0 or f.max() >= len(v):
        bad = int(np.argmax(np.any((f < 0) | (f >= len(v)), axis=1)))
        raise ValueError(f"face {bad} = {f[bad].tolist()} indexes outside the {len(v)} vertices")
    c = mesh.get("colors")
    if c is None:
        c = np.full((len(v), 3), 128, dtype=np.uint8)
    c = np.asarray(c)
    if c.shape != (len(v), 3) or c.dtype != np.uint8:
        raise ValueError(f"colors must be (Nv, 3) uint8, got {c.dtype} {c.shape}")
    return (np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32), np.ascontiguousarray(c))


def _mesh_texture(mesh, n_vertices, f):
    """The texture (Ht, Wt, 3) uint8 and the per-corner UVs (Nf, 3, 2) f32 of a textured mesh dict, or None when it holds no
    texture.  "face_uv" wins over "uv", which is expanded to corners here (the only device layout)."""
    tex = mesh.get("texture")
    if tex is None:
        return None
    tex = np.asarray(tex)
    if tex.ndim != 3 or tex.shape[2] != 3 or tex.dtype != np.uint8 or not (1 <= tex.shape[0] <= 16384 and 1 <= tex.shape[1] <= 16384):
        raise ValueError(f"texture must be (Ht, Wt, 3) uint8 with 1 <= Ht, Wt <= 16384, got {tex.dtype} {tex.shape}")
    if mesh.get("face_uv") is not None:
        uv = np.asarray(mesh["face_uv"])
        if uv.shape != (len(f), 3, 2) or not np.issubdtype(uv.dtype, np.floating):
            raise ValueError(f"face_uv must be a (Nf, 3, 2) float array, got {uv.dtype} {uv.shape}")
    elif mesh.get("uv") is not None:
        uv = np.asarray(mesh["uv"])
        if uv.shape != (n_vertices, 2) or not np.issubdtype(uv.dtype, np.floating):
            raise ValueError(f"uv must be a (Nv, 2) float array, got {uv.dtype} {uv.shape}")
        uv = uv[f]
    else:
        raise ValueError("a mesh with a texture needs 'face_uv' (Nf, 3, 2) or 'uv' (Nv, 2)")
    if not np.all(np.isfinite(uv)):
        raise ValueError("the UVs contain a non-finite value")
    return np.ascontiguousarray(tex), np.ascontiguousarray(uv, dtype=np.float32)


def texture_mips(image):
    """The mip pyramid of an (Ht, Wt, 3) uint8 device tensor, built on the device (T2 of the texture contract): a flat uint8 tensor
    of uchar4 texels, level 0 first, as pp_render_views_textured reads it."""
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or not image.is_cuda:
        raise ValueError(f"image must be an (Ht, Wt, 3) uint8 device tensor, got {image.dtype} {tuple(image.shape)} on {image.device}")
    image = image.contiguous()
    Ht, Wt = image.shape[:2]
    need = ctypes.c_size_t()
    _lib.call("pp_texture_mips_bytes", Wt, Ht, ctypes.byref(need), None)
    mips = torch.empty(need.value, dtype=torch.uint8, device=image.device)
    _lib.call("pp_texture_build_mips", image, Wt, Ht, mips, mips.numel())
    return mips


@dataclasses.dataclass
class Shading:
    """The lit render's description (THE SHADING CONTRACT, S1).  lights (Nl, 3) and intensity (Nl,), Nl <= 16: point lights in METRES
    in the OpenCV camera frame (x right, y down, z forward) — not scaled by `units`, only vertices and translations are; a light
    adds intensity * cos / distance^2 to the multiplier of the base colour.  ambient >= 0 is added to it.  normals: "flat" (the
    face's) or "smooth" (interpolated vertex normals: the mesh's "normals" when present, else vertex_normals(mesh)).  base_color: a
    uint8 triple that replaces the mesh's colours / texture, or None.  tone: None (the multiplied colour, rounded and clamped to
    255), "srgb" (srgb_tone_table()) or a uint8 array of 2 ... 65536 entries indexed by the colour / 255."""
    lights: object = None
    intensity: object = None
    ambient: float = 0.0
    normals: str = "flat"
    base_color: object = None
    tone: object = None


def template_lights(distance_m, recipe="blenderproc", key=1.0):
    """Light sets for templates rendered at `distance_m` metres -> {"lights" (Nl, 3), "intensity" (Nl,)} float64, Shading's fields.
    "blenderproc": the eight point lights of rendering/src/lib3d/blenderproc.py:29-33 at (+-1, +-1, {0, 1}) m around the camera,
    mapped from Blender's camera frame to ours, (x, -y, -z).  "headlight": one light at the camera (the pyrender recipe's).
    The intensities are equal and chosen, in float64, so that a point at (0, 0, distance_m) with normal (0, 0, -1) receives a
    multiplier of `key`: a camera-facing surface at the template distance shows its base colour for key = 1.  This normalisation
    is this project's own: Blender's absolute exposure (50 W per light through Cycles and its view transform) cannot be reproduced
    here, only the geometry of the light set is the reference's."""
    d = float(distance_m)
    if not (np.isfinite(d) and d > 0) or not (np.isfinite(key) and key >= 0):
        raise ValueError(f"distance_m must be positive and key non-negative, got {distance_m!r}, {key!r}")
    if recipe == "blenderproc":
        L = np.array([[x, -y, -z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (0.0, 1.0)])
    elif recipe == "headlight":
        L = np.zeros((1, 3))
    else:
        raise ValueError(f"recipe must be 'blenderproc' or 'headlight', got {recipe!r}")
    to_light = L - np.array([0.0, 0.0, d])
    d2 = (to_light ** 2).sum(axis=1)
    gain = (-to_light[:, 2]) / (d2 * np.sqrt(d2))               # n . L / |L|^3 with n = (0, 0, -1): every light is in front of it
    return {"lights": L, "intensity": np.full(len(L), float(key) / gain.sum())}


def srgb_tone_table(T=4096):
    """The sRGB OETF as a tone table of T uint8 entries: entry i is 255 * oetf(i / (T - 1)), evaluated in float64 and rounded."""
    if not 2 <= int(T) <= 65536:
        raise ValueError(f"T must be in [2, 65536], got {T}")
    x = np.arange(int(T), dtype=np.float64) / (int(T) - 1)
    y = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
    return np.floor(255.0 * np.clip(y, 0.0, 1.0) + 0.5).astype(np.uint8)


def _parse_shading(shading, distance_m):
    """Shading / dict / "tless" -> (lights4 (Nl, 4) f32, ambient, smooth, base_color (3,) u8 or None, tone (T,) u8 or None), validated."""
    if isinstance(shading, str):
        if shading != "tless":
            raise ValueError(f"shading must be a Shading, a dict of its fields or 'tless', got {shading!r}")
        shading = Shading(**template_lights(distance_m), normals="flat", base_color=(102, 102, 102))     # 0.4 * 255
    elif isinstance(shading, dict):
        unknown = set(shading) - {f.name for f in dataclasses.fields(Shading)}
        if unknown:
            raise ValueError(f"unknown shading field(s) {sorted(unknown)}")
        shading = Shading(**shading)
    elif not isinstance(shading, Shading):
        raise ValueError(f"shading must be a Shading, a dict of its fields or 'tless', got {type(shading).__name__}")
    try:
        lights = np.zeros((0, 3)) if shading.lights is None else np.asarray(shading.lights, dtype=np.float64)
        inten = np.zeros(0) if shading.intensity is None else np.asarray(shading.intensity, dtype=np.float64)
        ambient = float(shading.ambient)
    except (TypeError, ValueError) as e:
        raise ValueError(f"shading lights, intensity and ambient must be numeric: {e}") from None
    if lights.ndim != 2 or lights.shape[1] != 3 or len(lights) > 16 or not np.all(np.isfinite(lights)):
        raise ValueError(f"shading lights must be a finite (Nl, 3) array with Nl <= 16, got {lights.shape}")
    if inten.shape != (len(lights),) or not np.all(np.isfinite(inten)) or np.any(inten < 0):
        raise ValueError(f"shading intensity must be (Nl,) = ({len(lights)},) finite and non-negative, got {inten.shape}")
    with np.errstate(over="ignore"):
        lights4 = np.ascontiguousarray(np.concatenate([lights, inten[:, None]], axis=1).astype(np.float32))
    if not np.all(np.isfinite(lights4)):
        raise ValueError("a shading light or intensity overflows float32")
    if not (np.isfinite(ambient) and ambient >= 0 and np.isfinite(np.float32(ambient))):
        raise ValueError(f"shading ambient must be finite and non-negative, got {shading.ambient!r}")
    if shading.normals not in ("flat", "smooth"):
        raise ValueError(f"shading normals must be 'flat' or 'smooth', got {shading.normals!r}")
    base = shading.base_color
    if base is not None:
        b = np.asarray(base)
        if b.shape != (3,) or not np.issubdtype(b.dtype, np.integer) or b.min() < 0 or b.max() > 255:
            raise ValueError(f"shading base_color must be three integers in [0, 255], got {base!r}")
        base = np.ascontiguousarray(b.astype(np.uint8))
    tone = shading.tone
    if isinstance(tone, str):
        if tone != "srgb":
            raise ValueError(f"shading tone must be None, 'srgb' or a uint8 array, got {tone!r}")
        tone = srgb_tone_table()
    elif tone is not None:
        tone = np.asarray(tone)
        if tone.ndim != 1 or tone.dtype != np.uint8 or not 2 <= len(tone) <= 65536:
            raise ValueError(f"shading tone must be a 1-D uint8 array of 2 ... 65536 entries, got {tone.dtype} {tone.shape}")
        tone = np.ascontiguousarray(tone)
    return lights4, ambient, shading.normals == "smooth", base, tone


def vertex_face_csr(faces, n_vertices):
    """The vertex -> face adjacency of S8 -> (vf_offsets (Nv + 1,), vf_faces (3 Nf,)) int32: a stable sort of faces.reshape(-1),
    so the faces of a vertex come in ascending face index."""
    flat = np.asarray(faces, dtype=np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_vertices))])
    return offsets.astype(np.int32), np.ascontiguousarray((order // 3).astype(np.int32))


def vertex_normals(mesh, device="cuda"):
    """Area-weighted unit vertex normals of `mesh` ({"vertices", "faces"}) on the device (S8 of the shading contract) -> (Nv, 3)
    float32 device tensor; zeros for a vertex no face with area references.  One launch; the bytes do not depend on launch order."""
    v, f, _ = _mesh_arrays(mesh)
    if len(f) > (2 ** 31 - 1) // 3:
        raise ValueError(f"too many faces for the adjacency list ({len(f)})")
    off, adj = vertex_face_csr(f, len(v))
    v_d, f_d, off_d, adj_d = (torch.from_numpy(a).to(device) for a in (v, f, off, adj))
    out = torch.empty(len(v), 3, dtype=torch.float32, device=device)
    _lib.call("pp_vertex_normals", v_d, len(v), f_d, len(f), off_d, adj_d, out)
    return out


def _mesh_normals(mesh, n_vertices):
    """The mesh's own "normals" as (Nv, 3) float32, or None when it has none."""
    n = mesh.get("normals")
    if n is None:
        return None
    n = np.asarray(n)
    if n.shape != (n_vertices, 3) or not np.issubdtype(n.dtype, np.floating) or not np.all(np.isfinite(n)):
        raise ValueError(f"normals must be a finite (Nv, 3) float array, got {n.dtype} {n.shape}")
    return np.ascontiguousarray(n, dtype=np.float32)


def _unit_scale(units, vertices):
    if units == "auto":                                          # call_panda3d.py:39-40
        units = "m" if mesh_diameter(vertices) < 10 else "mm"
    if units not in ("m", "mm"):
        raise ValueError(f"units must be 'mm', 'm' or 'auto', got {units!r}")
    return 1.0 if units == "m" else 1e-3


def render_views(mesh, poses, K=TEMPLATE_K, resolution=(480, 640), units="mm", near=1e-3, return_depth_m=False, return_face_id=False,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES, check_near=True, device="cuda", shading=None, samples=1):
    """Render `mesh` ({"vertices", "faces", "colors" or None}, or with "texture" (Ht,Wt,3) uint8 and "face_uv" (Nf,3,2) or "uv"
    (Nv,2): the textured path, which wins over "colors") under the object -> camera poses (V,4,4) whose translation is in
    the mesh's `units` ("mm" as BOP models are, "m", or "auto": the reference's rule, diameter < 10 -> metres).  The kernels work
    in metres: vertices and translations are scaled by 1e-3 in float64 for "mm" and rounded to float32 once.
    -> {"rgba" (V,H,W,4) uint8, "depth_mm" (V,H,W) uint16 [, "depth_m" (V,H,W) f32, "face_id" (V,H,W) int32], "near_count"
    (1,) int32 device tensor}.  A mesh without colours and without a texture renders mid-grey (128, 128, 128) (unlit; pass `shading` for an
    untextured model).  shading: None (unlit, the default), a Shading, a dict of its fields, or "tless" = template_lights at the
    object's template distance (its diameter), flat normals, base_color (102, 102, 102), no tone table; the base colour of a sample is
    what the unlit render shows there, or base_color.  ValueError for a malformed shading field, before any device work.  A texture's mip
    pyramid is built on the device once per call, before the views are rendered.  `workspace_bytes` bounds the
    rasteriser's workspace; the views are rendered in as many chunks as that takes (at least one view's worth is allocated).
    check_near: synchronise and raise ValueError when a triangle was dropped at the near plane (`near` metres); False leaves the
    count on the device for the caller.
    samples: 1 (default: one sample at the pixel centre) or 4 (THE MULTISAMPLE CONTRACT): rgba is the rounded integer mean of four
    rotated-grid samples, each shaded on its own, an uncovered one counting (0, 0, 0, 0) — alpha in {0, 64, 128, 191, 255}, colour
    fading to black at silhouettes; depth_mm, depth_m, face_id and near_count stay the pixel centre's, equal to samples=1 bit for
    bit, so pixels with alpha > 0 and depth 0, and with depth > 0 and alpha < 255, exist.  Its effect on pose accuracy is unmeasured.
    ValueError for anything but the ints 1 and 4, before any device work."""
    _check_samples(samples)
    v, f, c = _mesh_arrays(mesh)
    tex = _mesh_texture(mesh, len(v), f)
    scale = _unit_scale(units, v)
    lit = None if shading is None else _parse_shading(shading, mesh_diameter(v) * scale)
    own_normals = _mesh_normals(mesh, len(v)) if lit is not None and lit[2] else None
    poses = np.array(poses, dtype=np.float64)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4) or len(poses) == 0 or not np.all(np.isfinite(poses)):
        raise ValueError(f"poses must be a non-empty finite (V, 4, 4) array, got {poses.shape}")
    poses[:, :3, 3] *= scale
    K = np.asarray(K, dtype=np.float64)
    H, W = int(resolution[0]), int(resolution[1])
    V = len(poses)
    v_m = np.ascontiguousarray((v.astype(np.float64) * scale).astype(np.float32))
    v_d, f_d, c_d = (torch.from_numpy(a).to(device) for a in (v_m, f, c))
    p_d = torch.from_numpy(np.ascontiguousarray(poses.astype(np.float32))).to(device)
    if samples == 1:
        per_view = _lib.workspace_bytes("pp_render_workspace_bytes", H, W, len(f), 1) - 256
    else:
        per_view = _lib.workspace_bytes("pp_render_ms_workspace_bytes", H, W, len(f), 1, samples) - 256
    chunk = max(1, min(V, (int(workspace_bytes) - 256) // per_view))
    ws = torch.empty(256 + chunk * per_view, dtype=torch.uint8, device=device)
    out = {"rgba": torch.empty(V, H, W, 4, dtype=torch.uint8, device=device),
           "depth_mm": torch.empty(V, H, W, dtype=torch.uint16, device=device),
           "near_count": torch.empty(1, dtype=torch.int32, device=device)}
    if return_depth_m:
        out["depth_m"] = torch.empty(V, H, W, dtype=torch.float32, device=device)
    if return_face_id:
        out["face_id"] = torch.empty(V, H, W, dtype=torch.int32, device=device)
    tail = (p_d, V, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), H, W, float(near), ws, ws.numel(),
            out["rgba"], out["depth_mm"], out.get("depth_m"), out.get("face_id"), out["near_count"])
    Ht = Wt = 0
    if tex is not None:
        image, face_uv = tex
        Ht, Wt = image.shape[:2]
        mips = texture_mips(torch.from_numpy(image).to(device))           # once per call: the chunk loop is inside the entry
        uv_d = torch.from_numpy(face_uv).to(device)
    if lit is not None:
        lights4, ambient, smooth, base, tone = lit
        n_d = None
        if smooth:                                                        # direction only: the unit of the vertices does not matter
            n_d = torch.from_numpy(own_normals).to(device) if own_normals is not None else vertex_normals(mesh, device)
        tone_d = None if tone is None else torch.from_numpy(tone).to(device)
        source = (c_d if tex is None and base is None else None, uv_d if tex is not None and base is None else None,
                  mips if tex is not None and base is None else None, Wt, Ht)
        light_args = (lights4 if len(lights4) else None, len(lights4), ambient, int(smooth), n_d, base, tone_d,
                      0 if tone is None else len(tone))
    if samples != 1:                                                      # one entry for the three colour sources, lit or not
        if lit is None:
            source = (c_d, None, None, 0, 0) if tex is None else (None, uv_d, mips, Wt, Ht)
            light_args = (None, 0, 0.0, 0, None, None, None, 0)
        _lib.call("pp_render_views_ms", v_d, len(v), f_d, f, len(f), *source, *tail, int(lit is not None), *light_args, samples)
    elif lit is not None:
        _lib.call("pp_render_views_lit", v_d, len(v), f_d, f, len(f), *source, *tail, *light_args)
    elif tex is None:
        _lib.call("pp_render_views", v_d, len(v), f_d, f, len(f), c_d, *tail)
    else:
        _lib.call("pp_render_views_textured", v_d, len(v), f_d, f, len(f), uv_d, mips, Wt, Ht, *tail)
    if check_near:
        _raise_on_near(int(out["near_count"].item()), near)
    return out


def _check_samples(samples):
    if type(samples) is not int or samples not in (1, 4):                 # (True is not 1)
        raise ValueError(f"samples must be the int 1 or 4, got {samples!r}")


def _raise_on_near(count, near):
    if count:
        raise ValueError(f"{count} triangle(s) reach the near plane (Zc <= {near} m) and were dropped: move the object away "
                         "from the camera (there is no near-plane clipping)")


def _crop_frames(rgba, depth, depth_is_f32, K, poses_mm, near_count, near, img_size, pts_size, rgb_mask_flag):
    """extents -> one device->host copy -> boxes -> one crop launch.  rgba (V,H,W,4) uint8 and depth (V,H,W) on the device."""
    V, H, W = rgba.shape[:3]
    dev = rgba.device
    meta = torch.empty(V * 4 + 1, dtype=torch.int32, device=dev)
    if near_count is None:
        meta[-1] = 0
    else:
        meta[-1:] = near_count
    _lib.call("pp_template_extents", rgba, V, H, W, meta, None)
    host = meta.cpu().numpy()                                    # the one device->host copy (it synchronises the stream)
    _raise_on_near(int(host[-1]), near)
    ext = host[:-1].reshape(V, 4)
    empty = np.where(ext[:, 1] < 0)[0]
    if len(empty):
        raise ValueError(f"template view {int(empty[0])} covers no pixel" + (f" (and {len(empty) - 1} more)" if len(empty) > 1 else ""))
    boxes = np.array([_square(int(e[0]), int(e[1]) + 1, int(e[2]), int(e[3]) + 1, H, W) for e in ext], dtype=np.int32)    # get_bbox
    if np.any(boxes[:, 0] < 0) or np.any(boxes[:, 2] < 0):
        raise ValueError("a template's square crop window leaves the frame (object larger than the smaller image dimension)")
    boxes_d = torch.from_numpy(boxes).to(dev)
    K = np.asarray(K, dtype=np.float64)
    S, P = int(img_size), int(pts_size)
    rgb = torch.empty(V, 3, S, S, dtype=torch.float32, device=dev)
    mask = torch.empty(V, S, S, dtype=torch.float32, device=dev)
    pts = torch.empty(V, P, P, 3, dtype=torch.float32, device=dev)
    mean, std = (ctypes.c_double * 3)(*CLIP_MEAN), (ctypes.c_double * 3)(*CLIP_STD)
    _lib.call("pp_templates_crop", rgba, depth, int(depth_is_f32), V, H, W, boxes_d, boxes, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
              float(K[1, 2]), S, P, int(rgb_mask_flag), mean, std, rgb, mask, pts)
    y1, y2, x1, x2 = (boxes[:, k].astype(np.float64) for k in range(4))
    M = np.zeros((V, 3, 3), dtype=np.float32)                    # M_resize @ M_crop of :246-254, entry by entry in float32
    M[:, 0, 0] = (S / (y2 - y1)).astype(np.float32)
    M[:, 1, 1] = (S / (x2 - x1)).astype(np.float32)
    M[:, 0, 2] = M[:, 0, 0] * (-boxes[:, 2]).astype(np.float32)
    M[:, 1, 2] = M[:, 1, 1] * (-boxes[:, 0]).astype(np.float32)
    M[:, 2, 2] = 1
    pose = np.array(poses_mm, dtype=np.float64)
    pose[:, :3, 3] = pose[:, :3, 3] / 1000.0                     # :244
    return {"tem_rgb": rgb, "tem_mask": mask, "tem_pts3d": pts, "tem_bbox": torch.from_numpy(boxes.astype(np.float32)).to(dev),
            "tem_M": torch.from_numpy(M).to(dev), "tem_K": torch.from_numpy(K.astype(np.float32))[None].repeat(V, 1, 1).to(dev),
            "tem_pose": torch.from_numpy(pose.astype(np.float32)).to(dev)}


def templates_from_frames(rgba, depth_mm, K, poses_mm, img_size=224, pts_size=64, rgb_mask_flag=False, device="cuda"):
    """The bank entries of frames the caller already has (decoded `NNNNNN.png` / `NNNNNN_depth.png`): rgba (V,H,W,4) uint8,
    depth_mm (V,H,W) (any integer or float dtype holding whole millimetres up to 65535), poses (V,4,4) with t in mm -> the `tem_*`
    tensors of one object, each view equal to utils.preprocess.crop_template's — with one upload, one extents launch, one
    device->host copy and one crop launch instead of three uploads and three launches per view."""
    rgba_d = torch.as_tensor(np.ascontiguousarray(rgba) if isinstance(rgba, np.ndarray) else rgba).to(device).contiguous()
    if rgba_d.dtype != torch.uint8 or rgba_d.dim() != 4 or rgba_d.shape[-1] != 4:
        raise ValueError(f"rgba must be (V, H, W, 4) uint8, got {rgba_d.dtype} {tuple(rgba_d.shape)}")
    if isinstance(depth_mm, np.ndarray):
        if depth_mm.dtype != np.uint16:
            if depth_mm.min() < 0 or depth_mm.max() > 65535 or np.any(depth_mm != np.floor(depth_mm)):
                raise ValueError("depth_mm must hold whole millimetres in [0, 65535] (a 16-bit depth PNG's values)")
            depth_mm = depth_mm.astype(np.uint16)
        depth_d = torch.from_numpy(np.ascontiguousarray(depth_mm)).to(device)
    else:
        depth_d = depth_mm.to(device).contiguous()
        if depth_d.dtype != torch.uint16:
            raise ValueError(f"a depth_mm tensor must be uint16, got {depth_d.dtype}")
    if tuple(depth_d.shape) != tuple(rgba_d.shape[:3]) or len(poses_mm) != rgba_d.shape[0]:
        raise ValueError("rgba, depth_mm and poses_mm disagree on (V, H, W)")
    return _crop_frames(rgba_d, depth_d, False, K, poses_mm, None, 0.0, img_size, pts_size, rgb_mask_flag)


def render_templates(mesh, view_poses, K=TEMPLATE_K, resolution=(480, 640), units="mm", depth="png", img_size=224, pts_size=64,
                     rgb_mask_flag=False, near=1e-3, workspace_bytes=DEFAULT_WORKSPACE_BYTES, device="cuda", shading=None, samples=1):
    """One object's template bank from its mesh: `tem_rgb` (V,3,S,S), `tem_mask` (V,S,S), `tem_pts3d` (V,P,P,3) metres, `tem_bbox`
    (V,4), `tem_M` (V,3,3), `tem_K` (V,3,3), `tem_pose` (V,4,4) (t in metres), float32 device tensors with `_get_template`'s values
    for the rendered frames (bop_test_dataset.py:212-264).  view_poses (V,4,4): only the rotations are used; the object sits at
    (0, 0, diameter) (template_object_poses).  Render, extents, ONE device->host copy (extents + near-plane count), one crop launch.
    depth="png" (default): the lookup points come from the uint16 millimetres a depth file would hold, as the reference's do;
    depth="float": from the float32 depth directly — a deviation from the reference that removes the 0.5 mm quantisation.
    shading: render_views' (None: unlit; "tless" for T-LESS / ITODD-like untextured CAD models); it changes `tem_rgb` only.
    samples: render_views' (1, or 4: colour and alpha are the integer mean of four shaded rotated-grid samples, depth stays the pixel
    centre's).  With 4 the box comes from alpha > 0 and `tem_mask` from alpha == 255, `_get_template`'s rule for an anti-aliased PNG, so
    boxes can grow by a pixel and lookup points on the rim can be empty; the effect on pose accuracy is unmeasured.
    ValueError: a triangle at the near plane, a view that covers no pixel (named), samples other than the ints 1 and 4."""
    _check_samples(samples)
    if depth not in ("png", "float"):
        raise ValueError(f"depth must be 'png' or 'float', got {depth!r}")
    v = _mesh_arrays(mesh)[0]
    to_mm = 1.0 / (_unit_scale(units, v) * 1000.0)               # the returned pose follows the file convention: t in mm, then / 1000
    poses = template_object_poses(view_poses, v)
    r = render_views(mesh, poses, K=K, resolution=resolution, units=units, near=near, return_depth_m=depth == "float",
                     workspace_bytes=workspace_bytes, check_near=False, device=device, shading=shading, samples=samples)
    poses_mm = poses.copy()
    poses_mm[:, :3, 3] *= to_mm
    return _crop_frames(r["rgba"], r["depth_m"] if depth == "float" else r["depth_mm"], depth == "float", K, poses_mm, r["near_count"],
                        near, img_size, pts_size, rgb_mask_flag)


def onboard_objects(net, meshes, view_poses, bs=16, extended=False, **render_kw):
    """`templates_data` for a list of meshes, stacked over objects as `get_templates` returns it (bop_test_dataset.py:266-308:
    every `tem_*` tensor (n_objects, V, ...)), plus `template_feature` (n_objects, V, C, 16, 16) computed as run_test.py:123-134
    does (the feature extractor's last level in mini-batches of `bs`).  extended=True adds the extended bank under
    `template_cache` (Net.precompute_templates with chunk=bs; its "feature" then serves as `template_feature`).  The result goes
    to pipeline.infer_image(net, data, templates_data, indexed_bank=True) as it is.  render_kw: render_templates' keywords."""
    banks = [render_templates(m, view_poses, **render_kw) for m in meshes]
    if not banks:
        raise ValueError("no meshes")
    data = {k: torch.stack([b[k] for b in banks]) for k in banks[0]}
    feats, dpt = [], []
    with torch.no_grad():
        for b in banks:
            if extended:
                pre = net.precompute_templates(b["tem_rgb"], chunk=bs)
                feats.append(pre["feature"])
                dpt.append(pre["dpt"])
            else:
                n = b["tem_rgb"].shape[0]
                feats.append(torch.cat([net.feature_extractor(b["tem_rgb"][s:s + bs].contiguous())[-1] for s in range(0, n, bs)]))
    data["template_feature"] = torch.stack(feats)
    if extended:
        data["template_cache"] = {"dpt": [torch.stack([d[k] for d in dpt]) for k in range(3)]}
    return data
