"""ctypes binding of libpicopose_hip.so — the C ABI declared in include/picopose_hip.h.

The binding is DERIVED from that header, once per process at import: every prototype's restype / argtypes, every
`typedef struct` as a ctypes.Structure (PpGemmDesc, PpScene, PpAdamTensor, PpAdamStep) and every integer `#define PP_*`
as a module constant.  A new entry point is declared in the header and nowhere else.  `parse_header` reads this one
header: plain `re`, no C grammar; a construct it does not know raises instead of being guessed at.

There is deliberately no CPU or eager-torch fallback: if the HIP library is
missing the import of any compute entry point raises.
"""
import ctypes
import os
import re

import numpy as np
# torch before the library is opened: PyTorch-ROCm bundles its own libamdhip64, and this library must bind to THAT runtime (it
# launches on torch's streams and takes torch's device pointers).  Loaded before torch, it would pull in /opt/rocm's copy — two
# HIP runtimes in one process, and every launch fails (seen on the GPU box with build() followed by smoke()).
import torch

from .build import LIB

_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "picopose_hip.h")

_SCALARS = {
    "int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
    "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
}
_TYPE_WORDS = {"void", "char", "short", "int", "long", "signed", "unsigned", "float", "double"}     # never a parameter's name
# structs whose arrays live in DEVICE memory: a pointer to one is a raw address (tensor.data_ptr()) like every other device pointer
# (the typedef's comment in the header points here)
_DEVICE_STRUCTS = ("PpAdamStep",)

_lib = None


class PicoPoseHipError(RuntimeError):
    pass


def _ctype(decl, structs, where, param=False):
    """ctypes type of the C type `decl` (None for void); param: `decl` is a parameter, which may end in its name."""
    if "[" in decl or "(" in decl:
        raise ValueError(f"{where}: cannot bind `{decl}`")
    if "*" in decl:
        base = " ".join(t for t in decl[:decl.index("*")].split() if t != "const")
        if decl.count("*") == 1:
            if base == "char":
                return ctypes.c_char_p
            if base in structs and base not in _DEVICE_STRUCTS:
                return ctypes.POINTER(structs[base])
        return ctypes.c_void_p
    words = [t for t in decl.split() if t != "const"]
    if param and len(words) > 1 and words[-1] not in _TYPE_WORDS:
        words.pop()                              # the parameter's name; `unsigned char` has none and stays whole
    if " ".join(words) in _SCALARS:
        return _SCALARS[" ".join(words)]
    if words == ["void"]:
        return None
    raise ValueError(f"{where}: unknown type in `{decl}`")


def _struct(name, body, structs):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = (d.strip() for d in decl.split(","))
        m = re.fullmatch(r"(.*[\s*])(\w+)", first)
        if m is None or (more and "*" in decl):
            raise ValueError(f"struct {name}: cannot bind `{decl}`")
        ctype = _ctype(m.group(1), structs, f"struct {name}")
        if ctype is None:
            raise ValueError(f"struct {name}: void member `{decl}`")
        if "*" in first:
            ctype = ctypes.c_void_p              # members are raw addresses, device or host
        fields += [(f, ctype) for f in (m.group(2), *more)]
    return type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} of include/picopose_hip.h"})


def parse_header(text):
    """C header text -> (prototypes {name: (restype, argtypes)}, structs {name: ctypes.Structure}, constants {PP_X: int},
    streamed: the names of the prototypes whose last parameter is `void* stream`)."""
    text = re.sub(r"/\*.*?\*/", " ", text.replace("\\\n", ""), flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PP_\w+)[ \t]+(.+?)[ \t]*$", text, flags=re.M):
        m = re.fullmatch(r"(\(\s*)?(-?(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]*(?(1)\s*\))", value)
        if m:
            constants[name] = int(m.group(2), 0)
    text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    structs = {}

    def take_struct(m):
        if m.group(1) != m.group(3):
            raise ValueError(f"struct {m.group(1)}: typedef'd as {m.group(3)}")
        structs[m.group(1)] = _struct(m.group(1), m.group(2), structs)
        return ""

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", take_struct, text)
    prototypes, streamed = {}, set()
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.*[\s*])(\w+)\s*\(([^()]*)\)", stmt, flags=re.S)
        if m is None:
            raise ValueError(f"cannot bind `{' '.join(stmt.split())[:80]}`")
        name, params = m.group(2), m.group(3).strip()
        restype = _ctype(m.group(1), structs, f"{name}: return type")
        argtypes = [] if params in ("", "void") else [_ctype(p, structs, name, param=True) for p in params.split(",")]
        if None in argtypes or name in prototypes:
            raise ValueError(f"{name}: void parameter or second declaration")
        prototypes[name] = (restype, argtypes)
        if re.fullmatch(r"void\s*\*\s*stream", params.split(",")[-1].strip()):
            streamed.add(name)
    return prototypes, structs, constants, streamed


with open(_HEADER) as _f:
    _PROTOTYPES, _STRUCTS, _CONSTANTS, _STREAMED = parse_header(_f.read())
globals().update(_STRUCTS)       # PpGemmDesc, PpScene, PpAdamTensor, PpAdamStep
globals().update(_CONSTANTS)     # PP_OK, PP_EINVAL, PP_MATCH_FAST, ...
PP_OK = _CONSTANTS["PP_OK"]      # (named for check() below)


def declared_symbols():
    """Every function name declared in include/picopose_hip.h."""
    return sorted(_PROTOTYPES)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise PicoPoseHipError(
                f"{LIB} not found: build it with `python -m picopose_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback."
            )
        L = ctypes.CDLL(LIB)
        for name, (restype, argtypes) in _PROTOTYPES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise PicoPoseHipError(f"{LIB} does not export {name}, which include/picopose_hip.h declares: rebuild it") from None
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_f32(*tensors):
    """Contiguous fp32 device views of the inputs (the ABI takes raw device pointers)."""
    out = []
    for t in tensors:
        if not t.is_cuda:
            raise PicoPoseHipError("picopose_amd runs on the GPU only: inputs must be CUDA(HIP) tensors")
        out.append(t.contiguous().float())
    return out


def check(rc, what):
    if rc != PP_OK:
        raise PicoPoseHipError(f"{what} failed: {lib().pp_strerror(rc).decode()} (code {rc})")


def address(v):
    """What a `void*` parameter or struct member takes for `v`: a tensor's data_ptr() (a view's own address), a numpy array's
    buffer; everything else — None (null), an int address, a ctypes array or pointer — as it is.  Nothing is validated here."""
    kind = _KINDS.get(type(v))
    if kind is None:         # (isinstance against torch.Tensor runs a metaclass hook: asked once per type, not per argument)
        kind = _KINDS[type(v)] = 1 if isinstance(v, torch.Tensor) else 2 if isinstance(v, np.ndarray) else 0
    return v.data_ptr() if kind == 1 else v.ctypes.data if kind == 2 else v


_KINDS = {}              # type of a pointer argument -> 1 tensor (and subclasses: Parameter), 2 numpy array, 0 passed as it is


_CURRENT = object()      # call()'s default stream: torch's current one
_PLANS = {}              # entry name -> (function, the `void*` parameters' positions, takes a stream, parameter count)


def _plan(name):
    restype, argtypes = _PROTOTYPES[name]
    if restype is not ctypes.c_int:
        raise TypeError(f"{name} does not return a status (its return type is {restype.__name__}): call lib().{name}(...) directly")
    # the conversion is chosen by the bound argtype: `void*` parameters (bar the appended stream, a handle already) go through
    # address(); POINTER(struct) takes an instance or an array by reference and scalars convert, both inside ctypes
    streamed = name in _STREAMED
    pointers = tuple(i for i, t in enumerate(argtypes[:len(argtypes) - streamed]) if t is ctypes.c_void_p)
    _PLANS[name] = plan = (getattr(lib(), name), pointers, streamed, len(argtypes))
    return plan


def call(name, *args, stream=_CURRENT, what=None):
    """Launch the status-returning entry `name` of include/picopose_hip.h: tensors and numpy arrays go in as themselves
    (see address()), an entry whose last parameter is `void* stream` gets torch's current stream appended (`stream=None`: the
    null stream, `stream=<int>`: that handle), and a status other than PP_OK raises PicoPoseHipError labelled `what` or `name`."""
    fn, pointers, streamed, count = _PLANS.get(name) or _plan(name)
    args = list(args)
    if streamed:
        args.append(torch.cuda.current_stream().cuda_stream if stream is _CURRENT else stream)
    elif stream is not _CURRENT:
        raise TypeError(f"{name} takes no stream")
    if len(args) != count:
        raise TypeError(f"{name} takes {count - streamed} arguments{' and a stream' if streamed else ''}, {len(args) - streamed} given")
    kinds = _KINDS
    for i in pointers:       # (address(), with the two frequent cases — a tensor, None or an int — decided here without a call)
        v = args[i]
        kind = kinds.get(type(v))
        if kind == 1:
            args[i] = v.data_ptr()
        elif kind != 0:
            args[i] = address(v)
    rc = fn(*args)
    if rc != PP_OK:
        check(rc, what or name)


def workspace_bytes(query, *args):
    """What the size query named `query` — an `int pp_*_workspace_bytes(args..., size_t* bytes)` entry — reports for `args`."""
    need = ctypes.c_size_t()
    call(query, *args, ctypes.byref(need))
    return need.value
