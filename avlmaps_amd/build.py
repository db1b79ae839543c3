"""Builds libavlmaps_hip.so (gfx950) in-tree with hipcc.  `python -m avlmaps_amd.build [--force]`."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
LIBDIR = PKG / "lib"
LIB = LIBDIR / "libavlmaps_hip.so"
ARCH = "gfx950"

# per-source extra flags; the builder's index math must not be contracted into FMAs implicitly
SOURCES = {
    "avl_api.hip": [],
    "avl_sim.hip": [],
    "avl_builder.hip": ["-ffp-contract=off"],      # the frame path: the only fused multiply-adds of K1 are the explicit fma() of the reference's BLAS order
    "avl_finalize.hip": ["-ffp-contract=off"],     # finished rows and merge payloads are the reference's float64 expressions, operation for operation
    "avl_replay.hip": ["-ffp-contract=off"],       # the replay rounds weight / grid_rgb like the reference's running mean, step by step
    "avl_rows.hip": ["-ffp-contract=off"],         # rows_div_f32 is finalize_kernel's division; the sums it divides are plain adds
    "avl_heat.hip": [],
    "avl_map2d.hip": [],
    "avl_lseg.hip": [],
    "avl_merge.hip": [],
    "avl_merge2.hip": [],
    "avl_field2d.hip": ["-ffp-contract=off"],      # the goal fields reproduce NumPy's float64 / float32 rounding step by step
    "avl_nav.hip": ["-ffp-contract=off"],          # the query predicates and path lengths round like the float64 oracle
    "avl_goal.hip": ["-ffp-contract=off"],         # every term of the fused goal is the stand-alone query's value bit for bit
    "avl_morph2d.hip": ["-ffp-contract=off"],      # the gaussian multiplies and adds in SciPy's order, without fused multiply-adds
    "avl_edt2d.hip": ["-ffp-contract=off"],        # the decay and the normalisation round like NumPy's float64 expressions
    "avl_islands.hip": ["-ffp-contract=off"],      # integer kernels; the flag keeps the file in line with the other 2-D sources
    "avl_render.hip": ["-ffp-contract=off"],       # the colour blend rounds like NumPy's float32 and float64 products, unfused
    "avl_pnp.hip": ["-ffp-contract=off"],          # the inlier test and the lift are NumPy's float64 expressions, operation for operation
    "avl_audio.hip": ["-ffp-contract=off"],        # compares, one product and one division per sample: nothing to fuse, and it stays so
    "avl_resample.hip": ["-ffp-contract=off"],     # a filter term is a float64 product, then a float64 add: SciPy's upfirdn, unfused
    "avl_explore.hip": ["-ffp-contract=off"],      # avl_sightray.h: a ray's points are K1's (the explicit fma chain), its slab and end points plain float64 operations
    "avl_gtmap.hip": ["-ffp-contract=off"],        # avl_sightray.h's pixel, K1's point and cell (the explicit fma chain); everything after it is integer
    "avl_resize.hip": ["-ffp-contract=off"],       # integer kernels; the flag keeps the file in line with the other 2-D sources
    "avl_instances.hip": ["-ffp-contract=off"],    # integer kernels; the flag keeps the file in line with the other integer sources
    "avl_colselect.hip": ["-ffp-contract=off"],    # integer kernels and one float64 comparison; nothing to fuse, and it stays so
    "avl_audit.hip": ["-ffp-contract=off"],        # avl_sightray.h: the ray's points, slab and end points are the carver's by one definition
    "avl_sight.hip": ["-ffp-contract=off"],        # integer kernels; the flag keeps the file in line with the other integer sources
    "avl_match.hip": ["-ffp-contract=off"],        # avl_sightray.h's pixel and K1's point; the rotation is plain float64 products and sums, unfused
    "avl_objects.hip": ["-ffp-contract=off"],      # integer kernels and float64 additions in a pinned order: nothing to fuse, and it stays so
    "avl_relations.hip": ["-ffp-contract=off"],    # integer kernels; the flag keeps the file in line with the other integer sources
    "avl_travel.hip": ["-ffp-contract=off"],       # the field is integer; a + b * sqrt(2), the decay and the normalisation round like NumPy, unfused
    "avl_rooms.hip": ["-ffp-contract=off"],        # integer kernels and one float64 comparison; the flag keeps the file in line with avl_travel.hip
    "avl_viewshed.hip": ["-ffp-contract=off"],     # integer kernels; the flag keeps the file in line with the other integer sources
    "avl_costfield.hip": ["-ffp-contract=off"],    # the field is integer; the costmap's d * d is one float64 product that rint() takes alone
    "avl_travel_many.hip": ["-ffp-contract=off"],  # the fields are integer; the sound sum's a + b * sqrt(2) and p - (p * d) * decay round like NumPy, unfused
    "avl_mapdiff.hip": ["-ffp-contract=off"],      # a row's sums are float64 products and additions in a pinned order, none fused; the status predicate rounds each product once
    "avl_mapfuse.hip": ["-ffp-contract=off"],      # the moved point and a fused element are float64 products and sums in a pinned order, each rounded once
    "avl_mappull.hip": ["-ffp-contract=off"],      # the pulled-back point, the corner weights and a gathered element are float64 products and sums in a pinned order
}
COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-fvisibility=hidden", "-Wall",
          "-Wno-unused-function", "-munsafe-fp-atomics"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and Path(c).exists():
            return c
    raise RuntimeError("hipcc not found (need ROCm with gfx950 support)")


def _stale(out: Path, deps) -> bool:
    if not out.exists():
        return True
    t = out.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


LAST_BUILD = dict(compiled=[], reused=[], linked=False)      # what the last build() call actually did (checked by the driver's log)


def build(force: bool = False, verbose: bool = False) -> Path:
    force = force or os.environ.get("AVLMAPS_FORCE_BUILD") == "1"
    hipcc = _hipcc()
    LIBDIR.mkdir(exist_ok=True)
    objdir = PKG / "build"
    objdir.mkdir(exist_ok=True)
    headers = list(CSRC.glob("*.h")) + [PKG.parent / "include" / "avlmaps_hip.h"]
    srcs = [s for s in SOURCES if (CSRC / s).exists()]
    jobs = []
    for s in srcs:
        src, obj = CSRC / s, objdir / (Path(s).stem + ".o")
        if force or _stale(obj, [src] + headers):
            jobs.append((s, [hipcc, *COMMON, *SOURCES[s], "-c", str(src), "-o", str(obj)]))

    def run(job):
        name, cmd = job
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {name}:\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr)
        return name

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    LAST_BUILD.update(compiled=[j[0] for j in jobs], reused=[s for s in srcs if s not in {j[0] for j in jobs}], linked=False)
    objs = [objdir / (Path(s).stem + ".o") for s in srcs]
    if force or jobs or _stale(LIB, objs):
        LAST_BUILD["linked"] = True
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", str(LIB), *map(str, objs)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")
    return LIB


if __name__ == "__main__":
    p = build(force="--force" in sys.argv, verbose=True)
    print("built", p)
