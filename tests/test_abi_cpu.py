"""No-GPU checks of the drop-in boundary: the C-ABI library loads, exports exactly the symbols include/geosplat_hip.h declares,
every one of them is bound with the header's own argument and return types (geosplatting_amd/_lib.py reads the prototypes from the
header; the checks here read the header on their own and state a few prototypes literally), the ctypes struct mirrors and the call
sites of the whole tree agree with the header, and the product path fails LOUDLY without a GPU / without the library -- it never
falls back to the oracle or to PyTorch."""
import ast
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VP = ctypes.c_void_p
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}


def _header():
    text = open(os.path.join(ROOT, "include", "geosplat_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", _header())))


def _kind(decl):
    """ctypes type of one parameter / field declaration, read here and not by the binding's parser"""
    if "*" in decl:
        return VP
    return SCALARS[[w for w in decl.split() if w != "const"][0]]


def _prototypes():
    """{name: (restype, [argtypes])} by one regular expression over the header (no function pointers: a parameter list has no
    parenthesis inside)"""
    text = re.sub(r"^\s*#.*$", "", _header(), flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(gs_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.replace("*", " * ").split())
        restype = ctypes.c_char_p if ret == "const char *" else SCALARS[ret]
        params = params.strip()
        assert name not in out
        out[name] = (restype, [] if params in ("", "void") else [_kind(p) for p in params.split(",")])
    return out


def test_library_exports_every_declared_symbol():
    """Declared == exported, in both directions, by the library's dynamic symbol table."""
    from geosplatting_amd import _lib
    lib = _lib.lib()
    decl = _declared()
    assert len(decl) >= 20 and sorted(_lib.SYMBOLS) == decl
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "llvm-nm")
    nm = next((t for t in (llvm, shutil.which("llvm-nm"), shutil.which("nm")) if t and os.path.exists(t)), None)
    assert nm is not None, "neither llvm-nm nor nm found"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("gs_")})
    assert [n for n in decl if n not in exported] == [], "declared in geosplat_hip.h but not exported"
    assert [n for n in exported if n not in decl] == [], "exported but not declared in geosplat_hip.h"
    assert lib.gs_version() >= 100
    assert lib.gs_last_error() is not None


def test_every_declared_symbol_is_typed():
    from geosplatting_amd import _lib
    lib = _lib.lib()
    protos = _prototypes()
    assert sorted(protos) == _declared()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes), name
        assert list(fn.argtypes) == argtypes, name
        assert fn.restype is restype, name
    I, I64, F, D, Z = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    literal = {
        "gs_raster_ws_bytes": (Z, [I64, I, I, I, I]),
        "gs_shade_fwd": (I, [I, VP, VP, VP, VP, VP, F, F, I, VP, VP, VP]),
        "gs_denoise_fwd": (I, [I, I, I, I, I, VP, VP, VP, D, I, VP, VP, VP]),
        "gs_isect_bin_front": (I, [I, VP, VP, VP, VP, I64, I, I, I, VP, VP, VP, Z, VP, VP]),
        "gs_last_error": (ctypes.c_char_p, []),
    }
    for name, (restype, argtypes) in literal.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_width_survives_without_a_wrapper():
    from geosplatting_amd import _lib
    lib = _lib.lib()
    # a 64-bit argument arrives intact and a size_t above 2^32 comes back intact
    assert lib.gs_raster_ws_bytes((1 << 33) + 1, 1, 16, 16, 16) >= 3 * 16 * (1 << 33)
    assert lib.gs_mlp_wgrad_ws_bytes(1 << 21) == 4 * 1024 * 1024


def test_wrong_kind_is_refused_before_the_call():
    from geosplatting_amd import _lib
    lib = _lib.lib()
    with pytest.raises(ctypes.ArgumentError):
        lib.gs_project_ws_bytes(1.5)
    wrong = ctypes.c_float(1.0)                 # (by name: the scan below would rightly report the literal wrapper in the call)
    with pytest.raises(ctypes.ArgumentError):
        lib.gs_raster_ws_bytes(wrong, 1, 16, 16, 16)


def test_binding_refuses_what_it_cannot_read(tmp_path, monkeypatch):
    """An unknown parameter or return type, a missing header and a declared symbol the library lacks all raise: no guessing."""
    from geosplatting_amd import _lib
    hdr = tmp_path / "h.h"
    for text, word in (("int gs_a(int n, GsEnv env);", "GsEnv env"), ("int gs_a(long n);", "long n"), ("long gs_a(int n);", "long"),
                       ("int gs_a(int n, void (*cb)(int));", "cb"), ("int other(int n);", "other")):
        hdr.write_text("/* c */\n#define X 1\n" + text + "\n")
        with pytest.raises(_lib.GeoSplatHipError, match=re.escape(word)):
            _lib.parse_header(str(hdr))
    hdr.write_text("size_t gs_a(const float* p, uint64_t n);\n")
    assert _lib.parse_header(str(hdr)) == {"gs_a": (ctypes.c_size_t, [VP, ctypes.c_uint64])}
    with pytest.raises(_lib.GeoSplatHipError, match="not found"):
        _lib.parse_header(str(tmp_path / "absent.h"))
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "PROTOTYPES", {**_lib.PROTOTYPES, "gs_not_there": (ctypes.c_int, [])})
    with pytest.raises(_lib.GeoSplatHipError, match="does not export gs_not_there"):
        _lib.lib()


def test_struct_mirrors_match_the_header():
    from geosplatting_amd import _lib
    text = _header()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    blocks = re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S)
    assert sorted(b[0] for b in blocks) == ["GsDensifyTensor", "GsEnv", "GsEnvGrad", "GsTailView", "GsTileLevel", "GsTsdfView"]
    for name, body, alias in blocks:
        assert alias == name
        want = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            kind = _kind(decl)
            names = decl.rsplit("*", 1)[1] if "*" in decl else decl.split(None, 1)[1]
            if "*" in decl or "const" in decl.split():
                assert "," not in names, decl                        # `const float* a, b` would make b a float: not written here
            for field in names.split(","):
                m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", field.strip())
                length = m.group(2) and (int(m.group(2)) if m.group(2).isdigit() else defines[m.group(2)])
                want.append((m.group(1), kind, length))
        got = [(f, t._type_, t._length_) if issubclass(t, ctypes.Array) else (f, t, None) for f, t in getattr(_lib, name)._fields_]
        assert got == want, name
    assert _lib.GS_MAX_LEVELS == defines["GS_MAX_LEVELS"]


def test_call_sites_agree_with_the_header():
    """Every `x.gs_name(...)` call of the tree, by its syntax tree: the declared number of arguments, every literal wrapper
    (L.i64, C.c_size_t, L.ptr, ...) of the declared type of its position, and no scalar wrapper left in the package (the typed
    functions convert plain Python numbers).  Calls with *args or keywords cannot be counted this way: skipped, and bounded."""
    protos = _prototypes()
    wrappers = {"i64": ctypes.c_int64, "f32": ctypes.c_float, "c_size_t": ctypes.c_size_t, "c_int64": ctypes.c_int64,
                "c_float": ctypes.c_float, "c_int": ctypes.c_int, "c_double": ctypes.c_double, "ptr": VP}
    files = (glob.glob(os.path.join(ROOT, "geosplatting_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "*.py"))
             + glob.glob(os.path.join(ROOT, "scripts", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "oracle", "*.py"))
             + [os.path.join(ROOT, "bench.py")])
    checked, skipped, bad = 0, 0, []
    for path in sorted(files):
        rel = os.path.relpath(path, ROOT)
        in_package = rel.startswith("geosplatting_amd" + os.sep)
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in protos):
                continue
            name, where = node.func.attr, f"{rel}:{node.lineno} {node.func.attr}"
            if node.keywords or any(isinstance(a, ast.Starred) for a in node.args):
                skipped += 1
                continue
            checked += 1
            argtypes = protos[name][1]
            if len(node.args) != len(argtypes):
                bad.append(f"{where}: {len(node.args)} arguments, the header declares {len(argtypes)}")
                continue
            for k, a in enumerate(node.args):
                f = a.func if isinstance(a, ast.Call) else None
                w = f.attr if isinstance(f, ast.Attribute) else f.id if isinstance(f, ast.Name) else None
                if w not in wrappers:
                    continue
                if wrappers[w] is not argtypes[k]:
                    bad.append(f"{where}: argument {k} is wrapped by {w}, the header declares {argtypes[k].__name__}")
                elif in_package and w != "ptr":
                    bad.append(f"{where}: argument {k} still carries the scalar wrapper {w}")
    assert not bad, "\n".join(bad)
    print(f"call sites: {checked} checked, {skipped} skipped (*args / keywords)")
    assert checked >= 300 and skipped <= 0.1 * (checked + skipped), (checked, skipped)


def test_argument_validation_without_gpu():
    """Entry points validate arguments before touching the device (no compute, no GPU needed)."""
    from geosplatting_amd import _lib
    lib = _lib.lib()
    assert lib.gs_project_ws_bytes(0) > 0 and lib.gs_project_ws_bytes(1 << 21) >= 4 * 8 * (1 << 11)
    assert lib.gs_raster_ws_bytes(ctypes.c_int64(1000), 500, 800, 800, 16) >= 3 * 16 * 1000 + 4 * 2500 + 3 * 16 * 500
    rc = lib.gs_raster_fwd(0, 0, 16, 3, 0, None, None, None, None, None, ctypes.c_int64(0), None, None, None, None, None,
                           None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"bad image size" in lib.gs_last_error()
    rc = lib.gs_raster_fwd(16, 16, 8, 3, 0, None, None, None, None, None, ctypes.c_int64(0), None, None, None, None, None,
                           None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"tile_size" in lib.gs_last_error()
    rc = lib.gs_shade_fwd(1, None, None, None, None, None, ctypes.c_float(0.1), ctypes.c_float(1.0), 7, None, None, None)
    assert rc == -1
    # FlexiCubes / field entry points
    assert lib.gs_flexicubes_ws_bytes(0, 4, 4) == 0 and lib.gs_flexicubes_ws_bytes(4, 4, 4) > 4 * 64 + 2 * 4 * 64 + 4 * 3 * 125
    assert lib.gs_flexicubes_ws_bytes(2000, 2000, 2000) == 0                       # 3 * vertices would overflow int32
    rc = lib.gs_flexicubes_count(0, 4, 4, None, None, ctypes.c_size_t(0), None, None)
    assert rc == -1 and b"resolution" in lib.gs_last_error()
    rc = lib.gs_flexicubes_count(4, 4, 4, None, None, ctypes.c_size_t(8), None, None)
    assert rc == -1 and b"workspace" in lib.gs_last_error()
    rc = lib.gs_mlp_wgrad(ctypes.c_int64(10), 33, 32, None, None, ctypes.c_float(1.0), None, 0, None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"[1, 32]" in lib.gs_last_error()
    assert lib.gs_mlp_wgrad_ws_bytes(ctypes.c_int64(1 << 21)) == 1024 * 1024 * 4
    rc = lib.gs_hashgrid_fwd(10, 16, 3, 18, None, None, None, None, None)
    assert rc == -1


def test_ops_refuse_cpu_tensors():
    import geosplatting_amd as gs
    from geosplatting_amd._lib import GeoSplatHipError
    z = torch.zeros(1, 3)
    with pytest.raises(GeoSplatHipError, match="GPU only"):
        gs.rasterization(z, torch.ones(1, 4), z + 1, torch.ones(1), z, torch.eye(4)[None], torch.eye(3)[None], 16, 16)
    with pytest.raises(GeoSplatHipError):
        gs.as_splitsum(torch.rand(6, 64, 64, 3))
    with pytest.raises(GeoSplatHipError):
        gs.tone_map(torch.rand(4, 4, 4), torch.tensor(1.0))


def test_missing_library_fails_loudly(tmp_path):
    """With the .so absent the import of an op must raise -- no silent CPU path."""
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import geosplatting_amd._lib as L\n"
        "L.LIB_PATH = %r\n"
        "try:\n"
        "    L.lib()\n"
        "except L.GeoSplatHipError as e:\n"
        "    print('RAISED', 'no CPU' in str(e))\n" % (ROOT, str(tmp_path / "nope.so")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert "RAISED True" in out.stdout, out.stdout + out.stderr


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "geosplatting_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), fn
    bench = open(os.path.join(ROOT, "bench.py")).read()
    # bench.py may use the oracle only inside its cpu_baseline leg (functions named cpu_baseline*)
    parts = bench.split("\ndef ")
    legs = [q for q in parts if q.startswith("cpu_baseline")]
    assert legs and all("import oracle" in q for q in legs)
    assert all("import oracle" not in q for q in parts if not q.startswith("cpu_baseline"))


def test_prefetch_registers_are_never_copied(tmp_path):
    """The compositor kernels prefetch three raw batches with inline-assembly loads and wait for them with a static
    `s_waitcnt vmcnt(6)` (csrc/gs_raster.hip: raw_load / raw_wait / raw_drain).  The compiler does not know that those registers
    are in flight between the load and the wait: if its register allocator ever split such a live range (a `v_mov`, an AGPR or
    scratch spill of the destination registers), the copy would read data that has not arrived.  This test disassembles the
    shipped kernels and checks that, after the initial loads, no move / spill instruction has one of the prefetch registers as
    its SOURCE -- the build is only valid while that holds (a register-pressure change in these kernels can break it)."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from geosplatting_amd import build as B
    out = tmp_path / "raster.s"
    subprocess.check_call([hipcc, *[f for f in B.FLAGS if f not in ("-shared", "-fPIC")], "-S", "--cuda-device-only",
                           os.path.join(B.CSRC, "gs_raster.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    src = out.read_text().split("\n")

    def regs(tok):
        m = re.match(r"v\[(\d+):(\d+)\]$", tok)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.match(r"v(\d+)$", tok)
        return {int(m.group(1))} if m else set()

    checked = 0
    for i, line in enumerate(src):
        if not re.match(r"_Z2[345]raster_(fwd_lanes|fwd_window|bwd_lanes|bwd_lanes2)_kernelILi\d+E", line):
            continue
        end = next(j for j in range(i, len(src)) if "s_endpgm" in src[j])
        # the prefetch loads are the INLINE-ASSEMBLY ones (";;#ASMSTART" in front of them): the compiler's own 16-byte loads (e.g. the
        # backward's checkpoint reads) are tracked by its wait-count pass and may live anywhere
        body, asm_line = [], set()
        for l in src[i:end]:
            t = l.strip()
            if t.startswith(";;#ASMSTART"):
                asm_line.add(len(body))
            if t and not t.startswith(";"):
                body.append(t)
        loads = [k for k, l in enumerate(body) if l.startswith("global_load_dwordx4") and k in asm_line]
        if len(loads) < 9:
            continue
        raw = set()
        for k in loads:
            raw |= regs(body[k].split()[1].strip(","))
        assert len(raw) == 36, (line, len(raw))                      # three batches x three 16-byte records, fixed registers
        drain = next(k for k in range(loads[-1], len(body)) if body[k].startswith("s_waitcnt vmcnt(0)"))   # raw_drain: all arrived
        for l in body[loads[8] + 1:drain]:
            if not re.match(r"(v_mov_b32|v_mov_b64|v_accvgpr_write|scratch_store|buffer_store)", l):
                continue
            ops = [t.strip(",") for t in l.split()[1:]]
            srcs = set().union(*[regs(t) for t in ops[1:]]) if len(ops) > 1 else set()
            assert not (srcs & raw), f"{line.split(':')[0]}: prefetch register copied while possibly in flight: {l}"
        checked += 1
    assert checked >= 4
