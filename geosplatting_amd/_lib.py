"""ctypes binding of libgeosplat_hip.so (the C-ABI declared in include/geosplat_hip.h).

There is NO fallback: if the HIP library is missing the import of any op raises.  PyTorch is only used for
device memory (``tensor.data_ptr()``) and the current HIP stream.

The header is the one table of prototypes: ``lib()`` sets ``restype`` and ``argtypes`` of every ``gs_*`` symbol from it, so callers
pass plain Python numbers and ``ptr(tensor)``; ctypes refuses a wrong argument count or kind before the call.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgeosplat_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "geosplat_hip.h")

GS_MAX_LEVELS = 16


class GsEnv(C.Structure):
    _fields_ = [("lut", C.c_void_p), ("lut_res", C.c_int), ("base", C.c_void_p), ("base_res", C.c_int),
                ("num_levels", C.c_int), ("levels", C.c_void_p * GS_MAX_LEVELS), ("res", C.c_int * GS_MAX_LEVELS),
                ("min_roughness", C.c_float), ("max_roughness", C.c_float)]


class GsTailView(C.Structure):
    _fields_ = [("viewmat", C.c_void_p), ("K", C.c_void_p), ("cam_pos", C.c_void_p), ("vis_records", C.c_void_p), ("v_packed", C.c_void_p),
                ("packed_index", C.c_void_p), ("W", C.c_int), ("H", C.c_int)]


class GsTileLevel(C.Structure):
    _fields_ = [("R", C.c_int), ("n_mirrors", C.c_int), ("margin", C.c_int), ("bw", C.c_int), ("nb", C.c_int), ("tile_begin", C.c_int),
                ("tile_end", C.c_int), ("reserved", C.c_int), ("src", C.c_void_p), ("scale", C.c_void_p), ("out_scale", C.c_void_p),
                ("bounds", C.c_void_p), ("tiles", C.c_void_p), ("segments", C.c_void_p), ("row_begin", C.c_void_p), ("row_counts", C.c_void_p),
                ("desc", C.c_void_p), ("weights", C.c_void_p), ("dst", C.c_void_p), ("lds_bytes", C.c_size_t)]


class GsDensifyTensor(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("floats_per_row", C.c_int), ("kind", C.c_int)]


class GsTsdfView(C.Structure):
    _fields_ = [("depth_alpha", C.c_void_p), ("viewmat", C.c_void_p), ("K", C.c_void_p), ("W", C.c_int), ("H", C.c_int)]


class GsEnvGrad(C.Structure):
    _fields_ = [("base", C.c_void_p), ("levels", C.c_void_p * GS_MAX_LEVELS)]


class GeoSplatHipError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_RETURNS = {**_SCALARS, "const char*": C.c_char_p}
_PROTOTYPE = re.compile(r"(const\s+char\s*\*|\w+)\s*\b(gs_\w+)\s*\((.*)\)", re.S)


def _ctype(where: str, decl: str):
    """ctypes type of one parameter declaration ("const float* means", "size_t ws_bytes"): every pointer is a c_void_p."""
    if "*" in decl and "(" not in decl:
        return C.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if len(words) != 2 or words[0] not in _SCALARS:
        raise GeoSplatHipError(f"{where}: parameter type of `{decl.strip()}` is not one the binding knows")
    return _SCALARS[words[0]]


def parse_header(path: str) -> dict:
    """{name: (restype, argtypes)} of every gs_* prototype the header declares -- the header is the one table of the C ABI.  It is
    plain C: comments, preprocessor lines, the extern "C" brace and the typedef struct blocks are dropped, every remaining statement
    must be a prototype over the scalar types above and pointers."""
    if not os.path.exists(path):
        raise GeoSplatHipError(f"{path} not found: the binding takes every prototype from it (the package runs from a checkout)")
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\b.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    protos = {}
    for stmt in text.split(";"):
        stmt = stmt.strip()
        if stmt in ("", "}"):
            continue
        m = _PROTOTYPE.fullmatch(stmt)
        if m is None:
            raise GeoSplatHipError(f"{path}: cannot read `{' '.join(stmt.split())[:80]}` as a gs_* prototype")
        ret, name, params = m.groups()
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise GeoSplatHipError(f"{path}: {name}: return type `{ret}` is not one the binding knows")
        params = params.strip()
        protos[name] = (_RETURNS[ret], [] if params in ("", "void") else [_ctype(f"{path}: {name}", p) for p in params.split(",")])
    return protos


PROTOTYPES = parse_header(HEADER_PATH)
SYMBOLS = list(PROTOTYPES)                 # every symbol include/geosplat_hip.h declares

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load the HIP library; raises (never falls back) if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GeoSplatHipError(
                f"{LIB_PATH} not found: build it with `python -m geosplatting_amd.build` "
                "(hipcc --offload-arch=gfx950).  geosplatting_amd has no CPU / PyTorch fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            try:
                fn = getattr(l, name)
            except AttributeError:
                raise GeoSplatHipError(f"{LIB_PATH} does not export {name}, which {HEADER_PATH} declares: rebuild the library") from None
            fn.restype, fn.argtypes = restype, argtypes
        _lib = l
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise GeoSplatHipError(f"{what} failed ({rc}): {lib().gs_last_error().decode()}")


def ptr(t: Optional[torch.Tensor]) -> Optional[C.c_void_p]:
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensors only"
    return C.c_void_p(t.data_ptr())


def stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(x: float) -> C.c_float:
    return C.c_float(float(x))


def i64(x: int) -> C.c_int64:
    return C.c_int64(int(x))


def require_cuda(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise GeoSplatHipError("geosplatting_amd ops run on the GPU only (tensor on %s); there is no CPU path" % t.device)


_alloc_workspace = torch.empty               # the one allocator of caller-side scratch; tests swap it to hand out poisoned, guarded blocks


def workspace(nbytes: int, device) -> torch.Tensor:
    """Scratch for a `ws` argument of the C ABI: a 1-D uint8 device tensor of max(nbytes, 1) bytes with UNDEFINED contents -- every
    entry point writes each segment of its workspace before it reads it (or states the cross-call contract in its header comment)."""
    return _alloc_workspace(max(int(nbytes), 1), dtype=torch.uint8, device=device)


_shared_streams = {}


def shared_stream(device: torch.device, role: str) -> "torch.cuda.Stream":
    """ONE HIP stream per (device, role) for the whole process -- "front0", "front1", "tail", "comm": the step engine, the call shape
    (viewbatch) and the gradient buckets all take theirs from here.  HIP maps its streams onto four hardware queues; with a private
    set per object a process that holds an engine AND renders through the call shape had eight streams, two per queue."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), role)
    st = _shared_streams.get(key)
    if st is None:
        st = _shared_streams[key] = torch.cuda.Stream(device=device)
    return st
