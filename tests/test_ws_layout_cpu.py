"""Workspace layouts without a GPU.

Walker: tests/ws_layout_host.cpp includes csrc/gs_ws.h alone and walks a few mixed segment lists (one zero-count segment among them)
at alignments 16 and 256, once with a NULL base (sizing) and once over a malloc(bytes) block (carving).  It checks that both walks
give the same size, that every pointer is aligned, that the segments are disjoint, in order and end inside `bytes`, that `pad`
advances, that 2^33 eight-byte items do not wrap, and it writes the first and last byte of every carved segment.  The program is
built with AddressSanitizer and UBSan where the host toolchain links them (a write outside the block then ends it).

Pinned sizes: every `*_bytes` export whose layout is written with that walker, and every export that only rounds with gs_align_up,
returns for every argument of the grid below exactly what tests/golden/ws_bytes_parent.json records.  The table was written by
`python tests/test_ws_layout_cpu.py --record` on a checkout of the commit before the layouts moved to the walker, with that
checkout's library built: the engine and the call shape cache their allocations by these values, and every kernel keeps its offsets
only while they hold.  The test reads the table; it computes no expected value itself."""
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "geosplatting_amd", "csrc")
TABLE = os.path.join(HERE, "golden", "ws_bytes_parent.json")

N_ISECTS = [0, 1, 2047, 2048, 2049, 50_000, 3_400_000, 2**31 - 1]              # radix blocks of 2048 items; int32 limit
V = [0, 1, 1023, 1024, 1025, 2_000_000]                                       # emission blocks of 1024 ranks
TILE_GRIDS = [(1, 1), (50, 50), (90, 91), (64, 128), (91, 91)]                # 8190 tiles, exactly BF_HIST_MAX = 8192, above it
IMAGES = [(16, 16), (800, 800), (801, 799)]
TILE_SIZES = [16, 0]
N_POINTS = [0, 1, 255, 256, 257, 511, 512, 513, 1_966_080]                    # chunks of 256 and 512 Gaussians
FACES = [0, 1, 63, 64, 65, 1000, 100_000]
RES = [(0, 4, 4), (1, 1, 1), (4, 4, 4), (7, 5, 3), (33, 31, 32), (128, 128, 128)]


def grid():
    """{export: [argument tuples]}"""
    g = {}
    g["gs_sort_ws_bytes"] = [(n, tw, th) for n in N_ISECTS for tw, th in TILE_GRIDS]
    g["gs_isect_bin_ws_bytes"] = [(v, n, tw, th) for v in V for n in N_ISECTS for tw, th in ((1, 1), (91, 91))]
    g["gs_isect_bin_front_ws_bytes"] = [(v, n, tw, th) for v in V for n in N_ISECTS for tw, th in TILE_GRIDS]
    g["gs_raster_ws_bytes"] = [(n, v, w, h, ts) for n in N_ISECTS for v in V for w, h in IMAGES for ts in TILE_SIZES]
    g["gs_raster_log_ws_bytes"] = [(n, w, h, ts) for n in N_ISECTS for w, h in IMAGES for ts in TILE_SIZES]
    for name in ("gs_project_ws_bytes", "gs_front_ws_bytes", "gs_surfel_project_ws_bytes"):
        g[name] = [(n,) for n in N_POINTS]
    # 4 .. 64 slabs of 8192 rows per level are supported: 2^15 .. 2^19 rows
    g["gs_hashgrid_bwd_fixed_ws_bytes"] = [(n, 16, 2, t) for n in (0, 1, 100_000) for t in (14, 15, 19, 20)]
    # exports that only lose a private rounding helper
    g["gs_densify_ws_bytes"] = [(n, s) for n in (0, 1, 255, 256, 257, 100_000) for s in (0, 2, 3)]
    g["gs_tsdf_extract_ws_bytes"] = list(RES)
    g["gs_flexicubes_ws_bytes"] = list(RES)
    g["gs_grid_splat_ws_bytes"] = [(c, *r) for c in (0, 1, 3) for r in RES]
    for name in ("gs_bvh_bytes", "gs_bvh_ws_bytes", "gs_nn_grid_bytes", "gs_nn_ws_bytes", "gs_mesh_topology_bytes"):
        g[name] = [(f,) for f in FACES]
    for name in ("gs_meshraster_ws_bytes", "gs_meshclip_ws_bytes"):
        g[name] = [(f, h, w) for f in FACES for h, w in ((1, 1), (17, 33), (800, 800))]
    return g


def _sizes():
    from geosplatting_amd import _lib
    lib = _lib.lib()
    return {name: [[*args, int(getattr(lib, name)(*args))] for args in cases] for name, cases in grid().items()}


def test_exported_sizes_are_those_of_the_recorded_table():
    want = json.load(open(TABLE))
    g = grid()
    assert sorted(want) == sorted(g)
    for name, cases in g.items():
        assert [tuple(row[:-1]) for row in want[name]] == cases, name            # the table covers the grid, row for row
    assert sum(len(c) for c in g.values()) > 700 and all(len(set(c)) == len(c) for c in g.values())
    got = _sizes()
    bad = [(name, a, b) for name in g for a, b in zip(got[name], want[name]) if a != b]
    assert not bad, f"{len(bad)} sizes differ from the recorded ones (export, now, recorded): {bad[:10]}"


def _compile(cxx, out, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I", CSRC, *extra, os.path.join(HERE, "ws_layout_host.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_walker_sizes_and_carves_alike(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ws_layout_host")
    built = _compile(cxx, exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0:
        built = _compile(cxx, exe, [])
    assert built.returncode == 0, built.stdout + built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().startswith("ok "), run.stdout
    assert int(run.stdout.split()[1]) == 2 * 4                                   # alignments x segment lists


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_ws_layout_cpu.py --record   (on the parent checkout, library built)"
    sys.path.insert(0, ROOT)
    with open(TABLE, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in _sizes().items()) + "\n}\n")
    print(TABLE)
