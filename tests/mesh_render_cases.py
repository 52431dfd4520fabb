"""Scenes of the mesh-render tests (``tests/test_mesh_render_host.py`` without a GPU, ``tests/test_mesh_render.py`` with one):
plain numpy, fp32-representable values."""
import numpy as np

from catre_amd import meshes as MS

EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)


def lattice_K(cx=0.0, cy=0.0):
    """fx = fy = 128: a vertex (x, y, 1) with x, y on multiples of 1/128 lands on an integer pixel"""
    return np.array([[128, 0, cx], [0, 128, cy], [0, 0, 1]], np.float32)


def on_lattice(uv, K, z=1.0):
    """pixel positions [n,2] (multiples of 1/256) -> vertices [n,3] at depth z that project there exactly"""
    uv = np.asarray(uv, np.float64)
    return np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z, (uv[:, 1] - K[1, 2]) / K[1, 1] * z, np.full(len(uv), z)], 1).astype(np.float32)


def quad(diagonal, reverse, swap, K):
    """The quad [8,24] x [8,16] px at z = 1 split by either diagonal, either winding, either face order"""
    verts = on_lattice([[8, 8], [24, 8], [24, 16], [8, 16]], K)
    faces = [[0, 1, 2], [0, 2, 3]] if diagonal == 0 else [[0, 1, 3], [1, 2, 3]]
    if reverse:
        faces = [f[::-1] for f in faces]
    if swap:
        faces = faces[::-1]
    return verts, np.asarray(faces, np.int32)


def fan(center_uv, K):
    """Six faces about a vertex placed on ``center_uv``"""
    ring = [[8, 0], [4, 7], [-4, 7], [-8, 0], [-4, -7], [4, -7]]
    verts = on_lattice([center_uv] + [[center_uv[0] + a, center_uv[1] + b] for a, b in ring], K)
    return verts, np.asarray([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.int32)


def random_pose(rng, z=(0.6, 1.0), xy=0.1):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    t = [rng.uniform(-xy, xy), rng.uniform(-xy, xy), rng.uniform(*z)]
    return np.concatenate([q, np.reshape(t, (3, 1))], 1).astype(np.float32)


def tilted_plane(K, nu=6, nv=4, u0=10, v0=8, step=6, normal=(2.0, -1.0, 1.0), d=0.8):
    """The topology of ``grid_mesh(nu, nv)`` with its vertices on the plane n . X = d, each on the ray of an integer pixel"""
    _, faces = MS.grid_mesh(nu, nv)
    uv = np.array([[u0 + step * i, v0 + step * j] for j in range(nv + 1) for i in range(nu + 1)], np.float64)
    rays = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(uv))], 1)
    z = d / (rays @ np.asarray(normal, np.float64))
    return (rays * z[:, None]).astype(np.float32), faces


def strip(n_faces):
    """A triangle strip of ``n_faces`` faces in the plane z = 0 of a unit-sized model: x in [-0.5, 0.5], y in {-0.1, 0.1}"""
    n = n_faces + 2
    verts = np.array([[-0.5 + k / (n - 1), 0.1 if k % 2 else -0.1, 0.0] for k in range(n)], np.float32)
    faces = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(n_faces)], np.int32)
    return verts, faces


def scene(name):
    """-> dict(meshes, mesh_of, pose, scale, K [F,3,3], frame_of, F, size, depth or None).  64x48 or 7x9 images, at most
    1300 faces per mesh."""
    rng = np.random.default_rng(sum(map(ord, name)))
    K1 = np.array([[70, 0, 31.5], [0, 70, 23.5], [0, 0, 1]], np.float32)
    size, F, depth = (48, 64), 1, None
    if name == "counts":           # faces per instance 1, 63, 64, 65, 257: the edges of the lanes-per-wave mapping
        meshes = [strip(n) for n in (1, 63, 64, 65, 257)]
        mesh_of = [0, 1, 2, 3, 4]
    elif name == "shared":         # ragged meshes shared through mesh_of, two cameras, two frames
        meshes = [MS.icosphere(1, 0.5), MS.box_mesh((1.0, 0.6, 0.8)), MS.icosphere(3, 0.5)]
        mesh_of = [2, 0, 1, 0, 2, 1]
        F = 2
    elif name == "tiny":           # 7 x 9 image, one face covering all of it, faces partly and wholly outside
        size = (9, 7)
        K1 = np.array([[8, 0, 3], [0, 8, 4], [0, 0, 1]], np.float32)
        big = (np.array([[-40, -40, 1], [40, -40, 1], [0, 60, 1]], np.float32), np.array([[0, 1, 2]], np.int32))
        part = (np.array([[-0.1, -0.1, 0.5], [0.6, 0.0, 0.5], [0.1, 0.9, 0.5]], np.float32), np.array([[0, 2, 1]], np.int32))
        out = (np.array([[5, 5, 1], [6, 5, 1], [5, 6, 1]], np.float32), np.array([[0, 1, 2]], np.int32))
        meshes, mesh_of = [big, part, out], [0, 1, 2]
    elif name == "edges":          # sliver, zero-area face, vertex behind the camera, index out of range, duplicates, coplanar ties
        v = np.array([[-0.3, -0.2, 1], [0.3, -0.2, 1], [0.0, 0.3, 1],                    # 0-2 a plain face
                      [-0.4, 0.0031, 1], [0.4, 0.0032, 1], [0.0, 0.0033, 1],            # 3-5 a sliver between sample rows
                      [0.1, 0.1, -0.5], [0.2, 0.2, 0.0]], np.float32)                   # 6 behind the camera, 7 on its plane
        f = np.array([[0, 1, 2], [0, 1, 2], [3, 4, 5], [0, 0, 1], [0, 1, 1], [0, 1, 6], [0, 7, 2], [0, 1, 8], [0, -1, 2],
                      [2, 1, 0]], np.int32)
        meshes, mesh_of = [(v, f)], [0, 0]                                              # two instances hold the same faces
    else:
        raise KeyError(name)
    I = len(mesh_of)
    if name in ("tiny", "edges"):
        pose = np.stack([EYE] * I)
        scale = np.ones((I, 3), np.float32)
    else:
        pose = np.stack([random_pose(rng) for _ in range(I)])
        scale = rng.uniform(0.15, 0.3, (I, 3)).astype(np.float32)
    K = np.stack([K1] * F)
    if F == 2:
        K[1] = [[90, 0, 20.25], [0, 85, 30.5], [0, 0, 1]]
    frame_of = [i % F for i in range(I)]
    return dict(meshes=meshes, mesh_of=mesh_of, pose=pose, scale=scale, K=K, frame_of=frame_of, F=F, size=size, depth=depth)


SCENES = ("counts", "shared", "tiny", "edges")


def observed(zbuf, delta, rng):
    """An observed depth against a rendered one that produces all five classes"""
    d = np.asarray(zbuf, np.float32).copy()
    pick = rng.integers(0, 5, d.shape)
    d[pick == 1] += np.float32(3 * delta)       # FREE
    d[pick == 2] -= np.float32(3 * delta)       # OCCLUDED
    d[pick == 3] = 0                            # HOLE
    d[(pick == 4) & (d > 0)] += np.float32(delta / 4)
    d[d < 0] = 0
    return d
