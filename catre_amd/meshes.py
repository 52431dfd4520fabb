"""Triangle meshes for the rasteriser (``render.render_mesh``, ``csrc/catre_mesh.h``).

* :class:`MeshSet` - the meshes of a batch as one ragged table on the device; ``mesh_of`` lets instances share meshes (the
  layout of ``pose_errors.SymSets``).
* :func:`box_mesh`, :func:`icosphere`, :func:`grid_mesh` - host numpy makers, faces wound outwards (counter-clockwise seen
  from outside; ``grid_mesh``: normal +z).
* :func:`load_obj` - the ``v`` and ``f`` lines of a Wavefront ``.obj`` (what NOCS / CAMERA ship per object), host only.

The rasteriser draws either winding; the makers keep one so that the meshes also serve renderers that cull."""
import numpy as np
import torch


def _int_list(v, name):
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise ValueError(f"{name}: a list or a CPU tensor (it is checked on the host), got a tensor on {v.device}")
        v = v.tolist()
    try:
        return [int(x) for x in v]
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected a list of integers, got {v!r}") from None


def _one_mesh(mesh, where):
    try:
        verts, faces = mesh
    except (TypeError, ValueError):
        raise ValueError(f"{where}: expected a (verts [V,3], faces [T,3]) pair") from None
    v = np.asarray(verts.detach().cpu() if isinstance(verts, torch.Tensor) else verts)
    f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1 or v.dtype.kind not in "fiu":
        raise ValueError(f"{where}: verts must be [V,3] numbers with V >= 1, got {v.dtype} {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in "iu":
        raise ValueError(f"{where}: faces must be [T,3] integers with T >= 1, got {f.dtype} {f.shape}")
    f = f.astype(np.int64)
    if np.abs(f).max() >= 2 ** 31:
        raise ValueError(f"{where}: face indices must fit int32")
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)


class MeshSet:
    """The meshes of a batch as a ragged table on the device: ``verts`` [V_tot,3] fp32, ``faces`` [T_tot,3] int32 with
    indices LOCAL to their mesh, ``vert_off`` / ``face_off`` [G+1] int32 (mesh g is rows ``off[g] .. off[g+1] - 1``),
    ``mesh_of`` [I] int32 (the mesh of instance i).  ``host`` keeps the (verts, faces) pairs as numpy arrays, ``n_verts`` /
    ``n_faces`` the sizes per mesh, ``mesh_of_host`` the map as a list.  Face indices are NOT checked against the vertex
    count: the rasteriser culls a face with an index outside its mesh (and counts it), it never reads out of bounds."""

    def __init__(self, verts, faces, vert_off, face_off, mesh_of, host, mesh_of_host):
        self.verts, self.faces, self.vert_off, self.face_off, self.mesh_of = verts, faces, vert_off, face_off, mesh_of
        self.host, self.mesh_of_host = host, list(mesh_of_host)
        self.n_verts = tuple(len(v) for v, _ in host)
        self.n_faces = tuple(len(f) for _, f in host)
        self.n_meshes, self.n_inst = len(host), len(self.mesh_of_host)
        self.v_tot, self.t_tot = sum(self.n_verts), sum(self.n_faces)
        self.device = verts.device

    @classmethod
    def from_list(cls, meshes, device, mesh_of=None):
        """``meshes``: a list of (verts [V,3], faces [T,3]) pairs (numpy arrays or tensors).  ``mesh_of`` (a list of I mesh
        indices) lets the instances of a batch share meshes; None: one mesh per instance, in order."""
        meshes = list(meshes)
        if not meshes:
            raise ValueError("meshes: needs at least one mesh")
        host = [_one_mesh(m, f"meshes[{g}]") for g, m in enumerate(meshes)]
        mesh_of = list(range(len(host))) if mesh_of is None else _int_list(mesh_of, "mesh_of")
        if not mesh_of:
            raise ValueError("mesh_of: needs at least one instance")
        for i, g in enumerate(mesh_of):
            if not 0 <= g < len(host):
                raise ValueError(f"mesh_of[{i}] = {g} is outside the {len(host)} meshes")
        voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in host])])
        foff = np.concatenate([[0], np.cumsum([len(f) for _, f in host])])
        if voff[-1] >= 2 ** 31 or foff[-1] >= 2 ** 31:
            raise ValueError("the table holds 2^31 vertices or faces or more")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return cls(up(np.concatenate([v for v, _ in host], 0)), up(np.concatenate([f for _, f in host], 0)),
                   up(voff.astype(np.int32)), up(foff.astype(np.int32)), up(np.asarray(mesh_of, np.int32)), host, mesh_of)

    def with_mesh_of(self, mesh_of):
        """The same table (no copy of the meshes) with another instance -> mesh map."""
        mesh_of = _int_list(mesh_of, "mesh_of")
        if not mesh_of:
            raise ValueError("mesh_of: needs at least one instance")
        for i, g in enumerate(mesh_of):
            if not 0 <= g < self.n_meshes:
                raise ValueError(f"mesh_of[{i}] = {g} is outside the {self.n_meshes} meshes")
        return MeshSet(self.verts, self.faces, self.vert_off, self.face_off,
                       torch.tensor(mesh_of, dtype=torch.int32).to(self.device), self.host, mesh_of)

    def instance_offsets(self):
        """Host -> (inst_vert_off [I+1], inst_face_off [I+1]) int64: the running sums of the sizes of ``mesh_of[i]``."""
        nv = np.asarray(self.n_verts, np.int64)[self.mesh_of_host]
        nf = np.asarray(self.n_faces, np.int64)[self.mesh_of_host]
        return np.concatenate([[0], np.cumsum(nv)]), np.concatenate([[0], np.cumsum(nf)])


# ---- makers (host numpy) -----------------------------------------------------------------------------------------------------
def box_mesh(extent=(1.0, 1.0, 1.0)):
    """An axis-aligned box of side lengths ``extent`` about the origin -> (verts [8,3] fp32, faces [12,3] int32)."""
    e = np.broadcast_to(np.asarray(extent, np.float64), (3,)) / 2
    verts = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * e
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # -x +x -y +y -z +z
    faces = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return verts.astype(np.float32), np.asarray(faces, np.int32)


def icosphere(subdiv=0, radius=1.0):
    """A unit icosahedron subdivided ``subdiv`` times, every vertex pushed to the sphere of ``radius`` ->
    (verts [10 * 4^s + 2, 3] fp32, faces [20 * 4^s, 3] int32)."""
    subdiv = int(subdiv)
    if subdiv < 0 or subdiv > 7:
        raise ValueError(f"subdiv must be 0 .. 7, got {subdiv}")
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    verts = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid = {}

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return (np.asarray(verts) * float(radius)).astype(np.float32), np.asarray(faces, np.int32)


def grid_mesh(nu, nv, extent=(1.0, 1.0)):
    """The rectangle ``extent`` about the origin in the plane z = 0 as ``nu`` x ``nv`` cells of two faces each, normal +z ->
    (verts [(nu+1)(nv+1), 3] fp32, faces [2 nu nv, 3] int32).  Vertex (i, j) is row ``j * (nu + 1) + i``."""
    nu, nv = int(nu), int(nv)
    if nu < 1 or nv < 1:
        raise ValueError(f"grid_mesh needs at least one cell each way, got {nu} x {nv}")
    ex, ey = (float(e) for e in extent)
    xs, ys = np.linspace(-ex / 2, ex / 2, nu + 1), np.linspace(-ey / 2, ey / 2, nv + 1)
    gx, gy = np.meshgrid(xs, ys)
    verts = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1)
    faces = []
    for j in range(nv):
        for i in range(nu):
            a = j * (nu + 1) + i
            b, c, d = a + 1, a + nu + 2, a + nu + 1
            faces += [(a, b, c), (a, c, d)]
    return verts.astype(np.float32), np.asarray(faces, np.int32)


def load_obj(path):
    """The geometry of a Wavefront ``.obj`` -> (verts [V,3] fp32, faces [T,3] int32, zero-based).  Reads ``v x y z`` (further
    numbers on the line - a weight, colours - are ignored) and ``f`` lines: ``i``, ``i/t``, ``i//n`` and ``i/t/n`` corners (the
    suffixes are ignored), negative indices (relative to the vertices read so far), polygons (fan-triangulated about their
    first corner).  Everything else - normals, texture coordinates, groups, materials - is skipped."""
    verts, faces = [], []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            parts = line.split("#", 1)[0].split()
            if not parts:
                continue
            if parts[0] == "v":
                if len(parts) < 4:
                    raise ValueError(f"{path}:{n}: a vertex needs three coordinates")
                verts.append([float(x) for x in parts[1:4]])
            elif parts[0] == "f":
                if len(parts) < 4:
                    raise ValueError(f"{path}:{n}: a face needs three corners")
                idx = []
                for corner in parts[1:]:
                    k = int(corner.split("/", 1)[0])
                    k = k - 1 if k > 0 else len(verts) + k
                    if k < 0 or k >= len(verts) or corner.startswith("0"):
                        raise ValueError(f"{path}:{n}: corner {corner!r} names no vertex read so far")
                    idx.append(k)
                faces += [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]
    if not verts or not faces:
        raise ValueError(f"{path}: no vertices or no faces")
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)
