"""Generates tests/golden/reference_meshes.json: what the mesh route (oracle.shapes.shape_from_urdf_file, the reference's
loader restated: merge order of geometry.py:9-21, 2-D face filter of assembly_env.py:50) yields on the reference's shape
files, one entry per name in oracle.shapes.SHAPES.  The files themselves are not stored; only the outlines read from them.

Run with a checkout of the reference:  python tests/golden/make_reference_meshes.py <reference checkout>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.shapes import SHAPES, shape_from_urdf_file  # noqa: E402

if __name__ == "__main__":
    REF_SHAPES = os.path.join(sys.argv[1], "assembly_gym", "shapes")
    out = {"_doc": "shape_from_urdf_file(<reference>/assembly_gym/shapes/<name>.urdf) -> verts [[x, z]], faces "
                   "[[i, j]], depth; written by make_reference_meshes.py"}
    for name in sorted(SHAPES):
        verts, faces, depth = shape_from_urdf_file(os.path.join(REF_SHAPES, name + ".urdf"))
        out[name] = {"verts": [list(map(float, v)) for v in verts], "faces": [list(map(int, f)) for f in faces],
                     "depth": float(depth)}
    with open(os.path.join(HERE, "reference_meshes.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
