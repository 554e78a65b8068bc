"""Procedural meshes for the mesh tests, written as Wavefront OBJ text (no fixture files): tessellated rectangles and
subdivided icospheres."""
import numpy as np


def grid_obj(corner, u, v, nu, nv, normals=True):
    """A rectangle corner + s u + t v, s, t in [0, 1], cut into nu x nv quads (2 nu nv triangles once loaded), as OBJ text."""
    corner, u, v = (np.asarray(x, dtype=np.float64) for x in (corner, u, v))
    lines = []
    for j in range(nv + 1):
        for i in range(nu + 1):
            p = corner + u * (i / nu) + v * (j / nv)
            lines.append(f"v {p[0]:.7g} {p[1]:.7g} {p[2]:.7g}")
    n = np.cross(u, v)
    n = n / np.linalg.norm(n)
    if normals:
        lines.append(f"vn {n[0]:.7g} {n[1]:.7g} {n[2]:.7g}")
    for j in range(nv):
        for i in range(nu):
            a = j * (nu + 1) + i + 1
            b, c, d = a + 1, a + nu + 2, a + nu + 1
            lines.append(f"f {a}//1 {b}//1 {c}//1 {d}//1" if normals else f"f {a} {b} {c} {d}")
    return "\n".join(lines) + "\n"


def icosphere(level):
    """(vertices, faces) of a unit icosahedron subdivided `level` times: 20 * 4^level triangles sharing their vertices."""
    g = (1 + 5 ** 0.5) / 2
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
             (-g, 0, -1), (-g, 0, 1)]
    verts = [tuple(np.asarray(p) / np.linalg.norm(p)) for p in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = np.asarray(verts[key[0]]) + np.asarray(verts[key[1]])
                verts.append(tuple(p / np.linalg.norm(p)))
                mid[key] = len(verts) - 1
            return mid[key]

        nxt = []
        for f in faces:
            a, b, c = midpoint(f[0], f[1]), midpoint(f[1], f[2]), midpoint(f[2], f[0])
            nxt += [(f[0], a, c), (f[1], b, a), (f[2], c, b), (a, b, c)]
        faces = nxt
    return np.asarray(verts), np.asarray(faces)


def icosphere_obj(level, centre=(0, 0, 0), radius=1.0, normals=True):
    v, f = icosphere(level)
    p = np.asarray(centre) + radius * v
    lines = [f"v {x:.7g} {y:.7g} {z:.7g}" for x, y, z in p]
    if normals:
        lines += [f"vn {x:.7g} {y:.7g} {z:.7g}" for x, y, z in v]
        lines += [f"f {a + 1}//{a + 1} {b + 1}//{b + 1} {c + 1}//{c + 1}" for a, b, c in f]
    else:
        lines += [f"f {a + 1} {b + 1} {c + 1}" for a, b, c in f]
    return "\n".join(lines) + "\n"


def strip_obj(n):
    """n triangles in a row across the back of the box."""
    lines = []
    for i in range(n + 2):
        lines.append(f"v {-3.5 + 7.0 * (i // 2) / (n // 2 + 1):.7g} {-1.0 + 2.0 * (i % 2):.7g} -7.5")
    lines += [f"f {i + 1} {i + 2} {i + 3}" for i in range(n)]
    return "\n".join(lines) + "\n"


def write(tmp_path, name, text):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def translate_scale(x, y, z, s):
    """Row-major 4x4 placing a model at (x, y, z) with uniform scale s."""
    return [[s, 0, 0, x], [0, s, 0, y], [0, 0, s, z], [0, 0, 0, 1]]
