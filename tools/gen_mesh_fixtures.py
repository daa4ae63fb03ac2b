#!/usr/bin/env python3
"""Writes tests/golden/meshes/ico1_*.obj: the level-1 icosphere (worlds.icosphere: 42 vertices, 80 triangles, radius
1 about the origin) as Wavefront OBJ, once per face-corner syntax load_obj reads -- ``i``, ``i/j``, ``i/j/k`` and
``i//k`` -- with the vt / vn lines those refer to (which the loader ignores).  Coordinates are printed with 9
significant digits: every float32 survives the round trip.

    python tools/gen_mesh_fixtures.py
"""
import importlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden", "meshes")

CORNER = {"v": "{i}", "vt": "{i}/{i}", "vtn": "{i}/{i}/{i}", "vn": "{i}//{i}"}


def main():
    rtw = importlib.import_module("zig-raytracing-weekend_amd")
    mesh = rtw.worlds.icosphere(1, [0, 0, 0], 1, rtw.Lambertian.fromColor([0.5, 0.5, 0.5]))
    os.makedirs(OUT, exist_ok=True)
    for name, corner in CORNER.items():
        lines = [f"# level-1 icosphere, face corners as {corner.format(i='i')} (tools/gen_mesh_fixtures.py)", "o ico1"]
        lines += ["v " + " ".join(f"{x:.9g}" for x in v) for v in mesh.vertices]
        if "t" in name:
            for v in mesh.vertices.astype(np.float64):
                lines.append(f"vt {np.arctan2(v[2], v[0]) / (2 * np.pi) + 0.5:.6f} {np.arcsin(v[1]) / np.pi + 0.5:.6f}")
        if "n" in name:
            lines += ["vn " + " ".join(f"{x:.6f}" for x in v) for v in mesh.vertices]
        lines.append("s off")
        lines += ["f " + " ".join(corner.format(i=int(i) + 1) for i in f) for f in mesh.faces]
        with open(os.path.join(OUT, f"ico1_{name}.obj"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
