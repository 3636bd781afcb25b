"""Writes tests/golden/raycast_obj.npz: the vertices and faces of the reference's examples/data/pose_estimation/model/obj.ply
(an ASCII PLY; data only) and the two poses and the intrinsics of its ray_cast_rendering example.

    python tests/golden/make_raycast_golden.py <path to obj.ply>

The vertices are kept as the single-precision numbers a PLY `float` property holds, in the file's unit (millimetres); the
example scales the mesh by 0.001 about the origin, which the tests do in double precision as Open3D's scale() does.
Tests never run this script."""
import os
import sys

import numpy as np


def read_ascii_ply(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"ply"
        n_vert = n_face = 0
        while True:
            line = f.readline().split()
            if line[:1] == [b"format"]:
                assert line[1] == b"ascii"
            elif line[:2] == [b"element", b"vertex"]:
                n_vert = int(line[2])
            elif line[:2] == [b"element", b"face"]:
                n_face = int(line[2])
            elif line[:1] == [b"end_header"]:
                break
        verts = np.array([f.readline().split()[:3] for _ in range(n_vert)], dtype=np.float64).astype(np.float32)
        faces = np.array([f.readline().split()[1:4] for _ in range(n_face)], dtype=np.int64)
    return verts, faces


if __name__ == "__main__":
    verts, faces = read_ascii_ply(sys.argv[1])
    assert faces.min() >= 0 and faces.max() < len(verts) < 65536
    poses = np.array([[[0.29493218, 0.95551309, 0.00312103, -0.14527225],
                       [0.89692822, -0.27572004, -0.34568516, 0.12533501],
                       [-0.32944616, 0.10475302, -0.93834537, 0.99371838],
                       [0., 0., 0., 1.]],
                      [[0.29493218, 0.95551309, 0.00312103, -0.04527225],
                       [0.89692822, -0.27572004, -0.34568516, 0.02533501],
                       [-0.32944616, 0.10475302, -0.93834537, 0.99371838],
                       [0., 0., 0., 1.]]])
    intrinsic = np.array([640, 480, 572.4114, 573.5704, 325.2611, 242.0489])   # width, height, fx, fy, cx, cy
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "raycast_obj.npz")
    np.savez_compressed(out, vertices=verts, triangles=faces.astype(np.uint16), poses=poses, intrinsic=intrinsic, scale=np.float64(0.001))
    print(out, os.path.getsize(out), "bytes;", len(verts), "vertices,", len(faces), "triangles")
