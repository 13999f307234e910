#!/usr/bin/env python3
"""Generates tests/golden/mesh_contains.npz by RUNNING THE REFERENCE's own MeshIntersector (utils/libmesh/inside_mesh.py).

Run in the authoring container only (needs the reference checkout, REF below):

    python tests/golden/make_golden_contains.py

* `triangle_hash.pyx` is compiled with the local Cython into a throw-away folder outside the repository and imported from there; when
  that fails, an all-candidates stand-in for TriangleHash (OUR code: every triangle is offered for every point inside the hash's index
  range) takes its place and the fixture's `note` says so.  The hash only generates candidates -- a point that passes the strict
  barycentric test of a triangle lies inside that triangle's xy box -- so either way the result is the reference's answer.
* the reference module is imported UNMODIFIED from where it lies, as a package `libmesh` with only inside_mesh + triangle_hash in it
  (its __init__ also pulls in modules this image cannot build); `np.bool`, which the module uses and numpy dropped, is restored for
  the duration of the run.
* the fixture holds data only: vertices, faces, points and `contains` of three meshes (tests/mesh_contains_model.py builds them), and
  `contains` of the cube at the integer lattice (mesh_contains_model.lattice) and of the cube without its top at the cube's points.
"""
from __future__ import annotations

import importlib
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import mesh_contains_model as mc  # noqa: E402

STANDIN = '''
import numpy as np

class TriangleHash:
    def __init__(self, triangles, resolution):
        self.n, self.resolution = len(triangles), resolution

    def query(self, points):
        xy = np.asarray(points)[:, :2]
        with np.errstate(invalid="ignore"):
            c = xy.astype(np.int64)
            ok = np.nonzero(((0 <= c) & (c < self.resolution)).all(axis=1))[0]
        return np.repeat(ok, self.n).astype(np.int32), np.tile(np.arange(self.n), len(ok)).astype(np.int32)
'''


def reference_intersector():
    """-> (MeshIntersector class of the reference, note)"""
    tmp = tempfile.mkdtemp(prefix="libmesh_build_")
    pkg = os.path.join(tmp, "libmesh")
    os.makedirs(pkg)
    open(os.path.join(pkg, "__init__.py"), "w").close()
    src = os.path.join(REF, "utils", "libmesh")
    note = "reference MeshIntersector with the reference triangle_hash.pyx compiled by the local Cython"
    try:
        shutil.copy(os.path.join(src, "triangle_hash.pyx"), pkg)
        setup = ("from setuptools import setup, Extension\nfrom Cython.Build import cythonize\nimport numpy\n"
                 "setup(ext_modules=cythonize([Extension('triangle_hash', ['triangle_hash.pyx'], language='c++', "
                 "include_dirs=[numpy.get_include()])], language_level=3))\n")
        with open(os.path.join(pkg, "setup.py"), "w") as fh:
            fh.write(setup)
        subprocess.run([sys.executable, "setup.py", "build_ext", "--inplace"], cwd=pkg, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    except Exception as e:  # noqa: BLE001
        print("triangle_hash.pyx did not compile (%s): using the all-candidates stand-in" % (str(e).splitlines() or [""])[0])
        with open(os.path.join(pkg, "triangle_hash.py"), "w") as fh:
            fh.write(STANDIN)
        note = "reference MeshIntersector with an all-candidates stand-in for TriangleHash (triangle_hash.pyx did not compile here)"
    os.symlink(os.path.join(src, "inside_mesh.py"), os.path.join(pkg, "inside_mesh.py"))
    sys.path.insert(0, tmp)
    if not hasattr(np, "bool"):
        np.bool = bool
    return importlib.import_module("libmesh.inside_mesh").MeshIntersector, note


def main():
    MeshIntersector, note = reference_intersector()
    meshes = {"tet": mc.tetrahedron(), "cube": mc.cube(), "sphere": mc.sphere_interface(300)}
    out = {"note": np.array(note)}
    for k, (name, (v, f)) in enumerate(meshes.items()):
        lo, hi = v[np.unique(f)].min(axis=0), v[np.unique(f)].max(axis=0)
        pts = lo - 0.1 * (hi - lo) + np.random.default_rng(100 + k).random((2000, 3)) * 1.2 * (hi - lo)
        got = MeshIntersector(types.SimpleNamespace(vertices=v, faces=f.astype(np.int64)), 512).query(pts)
        out.update({name + "_vertices": v, name + "_faces": f.astype(np.int32), name + "_points": pts, name + "_contains": np.asarray(got, dtype=bool)})
        print("%-6s %5d faces, %d points, %d inside" % (name, len(f), len(pts), int(got.sum())))
    # exact ties, and a mesh whose two parities differ: the cube at the integer lattice through it, and without its top (z = hi) faces
    v, f = mc.cube()
    lat = mc.lattice(-1, 6)
    out["cube_lattice_contains"] = np.asarray(MeshIntersector(types.SimpleNamespace(vertices=v, faces=f.astype(np.int64)), 512).query(lat), dtype=bool)
    out["cube_open_contains"] = np.asarray(MeshIntersector(types.SimpleNamespace(vertices=v, faces=f[:-2].astype(np.int64)), 512).query(out["cube_points"]),
                                           dtype=bool)
    path = os.path.join(HERE, "mesh_contains.npz")
    np.savez_compressed(path, **out)
    print(note)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
