"""Panoptic surface-mesh export: the labelled, coloured triangle mesh of the trained field (beyond the reference, whose map is a point cloud).

The extractor is SURFACE NETS on the density lattice: one vertex per sign-changing cell, one quad per sign-changing lattice edge.  It needs no case
table, and it is two ordered appends (csrc/mesh.hip on ordered_append.h): cells give vertices, edges give faces, both in an order that does not
depend on the launch geometry.  surface_nets_reference below is THE DEFINITION, written in tensor ops; surface_nets is the device path and gives its
bits.  DESIGN 4.33 has the algorithm, the kernels and the measurements.

    density_lattice   the nef's density at the lattice points i / resolution * 2 - 1, i = 0 .. resolution (queried at the points themselves)
    surface_nets      field, iso -> vertices, normals, faces, cell_vertex
    extract_mesh      both, then instance / semantic labels (the argmax kernel of the map export) and the colour seen along -normal at the vertices
    save_mesh / load_mesh   a little-endian binary PLY with faces;  mesh_report: counts, closed / oriented, Euler characteristic, area, volume

Memory: the lattice is held whole - 4 bytes per point for the field and 4 per cell for cell_vertex, plus the outputs (36 bytes per vertex pair of
faces and 24 per vertex); a lattice that does not fit has to be cut into slabs by the caller (`limits`).
"""
import numpy as np
import torch

from . import ops
from .map_export import MapAccumulator, _labels_of

MAX_CELLS = 2 ** 31
DEFAULT_CHANNELS = ("inst_embedding", "semantics")
_CORNERS = [(bx, by, bz) for bx in (0, 1) for by in (0, 1) for bz in (0, 1)]


def _cell_edges():
    """The 12 edges of a cell, axis-major; per axis the two other axes in increasing order with bits (bu, bv) = 00, 01, 10, 11, the lower axis's bit
    slower -> [(axis, corner A, corner B)] with bit 0 / 1 on the axis."""
    out = []
    for a in range(3):
        u, v = [x for x in range(3) if x != a]
        for bu in (0, 1):
            for bv in (0, 1):
                A = [0, 0, 0]
                A[u], A[v] = bu, bv
                B = list(A)
                B[a] = 1
                out.append((a, tuple(A), tuple(B)))
    return out


_EDGES = _cell_edges()


def _check_field(field, what):
    field = torch.as_tensor(field)
    if field.dim() != 3:
        raise ValueError("%s: field must be [nx, ny, nz], got %s" % (what, tuple(field.shape)))
    if min(field.shape) < 2:
        raise ValueError("%s: every axis of the lattice needs at least 2 points, got %s" % (what, tuple(field.shape)))
    nx, ny, nz = (int(s) for s in field.shape)
    if (nx - 1) * (ny - 1) * (nz - 1) >= MAX_CELLS:
        raise ValueError("%s: %d x %d x %d lattice has 2^31 cells or more (vertex ids are int32): cut it into slabs" % (what, nx, ny, nz))
    return field.detach().to(torch.float32)


def _frame(lo, h, index0):
    """-> (lo f32 x 3, h f32, index0 int x 3) as Python numbers already rounded to fp32; lo is one number or three."""
    lo = np.asarray(lo.detach().cpu() if torch.is_tensor(lo) else lo, dtype=np.float32).reshape(-1)
    if lo.size not in (1, 3):
        raise ValueError("lo must be one number or three, got %d" % lo.size)
    lo = [float(v) for v in (np.repeat(lo, 3) if lo.size == 1 else lo)]
    index0 = [int(v) for v in index0]
    if len(index0) != 3 or min(index0) < 0:
        raise ValueError("index0 must be three indices >= 0, got %r" % (index0,))
    return lo, float(np.float32(h)), index0


def _corner(t, bits):
    nx, ny, nz = t.shape
    bx, by, bz = bits
    return t[bx:nx - 1 + bx, by:ny - 1 + by, bz:nz - 1 + bz]


@torch.no_grad()
def surface_nets_reference(field, iso, lo, h, index0=(0, 0, 0)):
    """THE DEFINITION of the surface-nets mesh of field f32 [nx,ny,nz] (z fastest) at `iso`, in tensor ops on the field's device.

    A lattice point is INSIDE when v >= iso (a NaN is outside).  Cell (i,j,k), corners (i+bx, j+by, k+bz), is ACTIVE when its 8 corners are finite
    and neither all inside nor all outside; the active cells, in cell linear order (x slowest), are the vertices.  All arithmetic is fp32 in the
    order written; every sum is a chain of adds.  Over the 12 cell edges (_cell_edges: A -> B along the axis a) whose ends differ in `inside`:
    t = (iso - vA) / (vB - vA), p = A's bits with p[a] = t, S = S + p, n += 1;  local = S / float(n);  per axis
    vertex = (float(index0 + cell index) + local) * h + lo.  Normal: g[a] = the chain sum of (vB - vA) over the axis's four edges,
    m = sqrt((g0*g0 + g1*g1) + g2*g2), normal = -g / m, or 0 when m == 0 (towards falling density).
    Faces: edge row r = ((i*ny + j)*nz + k)*3 + a is the lattice edge from P = (i,j,k) to P + e_a.  It gives a quad when its ends differ in `inside`
    and the four cells at P with offsets (du,dv) = (-1,-1), (0,-1), (0,0), (-1,0) on the axes u = (a+1)%3, v = (a+2)%3 exist and have a vertex:
    q0..q3, reversed when P is outside; the s-th kept row gives the triangles (q0,q1,q2), (q0,q2,q3) at face rows 2s, 2s+1.  Face normals point
    from inside to outside.
    -> {'vertices' f32 [V,3], 'normals' f32 [V,3], 'faces' i32 [F,3], 'cell_vertex' i32 [nx-1,ny-1,nz-1] (-1: no vertex)}."""
    f = _check_field(field, "surface_nets")
    lo, h, index0 = _frame(lo, h, index0)
    dev = f.device
    nx, ny, nz = f.shape
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)          # noqa: E731
    iso_t = f32(float(iso))
    inside = f >= iso_t
    finite = torch.isfinite(f)
    all_finite = _corner(finite, _CORNERS[0]).clone()
    n_inside = _corner(inside, _CORNERS[0]).to(torch.int32)
    for bits in _CORNERS[1:]:
        all_finite &= _corner(finite, bits)
        n_inside = n_inside + _corner(inside, bits)
    active = all_finite & (n_inside > 0) & (n_inside < 8)
    cell_vertex = torch.where(active, torch.cumsum(active.reshape(-1), 0).reshape(active.shape) - 1, -1).to(torch.int32)
    # the arithmetic, on the active cells only (in cell order): 12 steps over whole tensors
    val = {bits: _corner(f, bits)[active] for bits in _CORNERS}
    ins = {bits: v >= iso_t for bits, v in val.items()}
    V = int(val[_CORNERS[0]].numel())
    zero = torch.zeros(V, dtype=torch.float32, device=dev)
    S, g, n = [zero, zero, zero], [None, None, None], torch.zeros(V, dtype=torch.int32, device=dev)
    for a, A, B in _EDGES:
        cross = ins[A] != ins[B]
        d = val[B] - val[A]
        t = (iso_t - val[A]) / d
        for x in range(3):
            S[x] = S[x] + torch.where(cross, t if x == a else f32(float(A[x])), zero)
        n = n + cross
        g[a] = d if g[a] is None else g[a] + d
    cell = torch.nonzero(active)                                               # [V,3] int64, cell order
    nf = n.to(torch.float32)
    h_t = f32(h)
    vertices = torch.stack([((cell[:, x] + index0[x]).to(torch.float32) + S[x] / nf) * h_t + f32(lo[x]) for x in range(3)], -1)
    # the correctly rounded fp32 square root, formed in fp64: 53 >= 2 * 24 + 2 bits make the second rounding harmless, also where the library's own
    # fp32 (or fp64) square root is an ulp off - torch's CPU sqrt is a vendor routine on some hosts, and a normal differed from the kernel's there
    m = torch.sqrt(((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).double()).float()
    normals = torch.stack([torch.where(m == 0, zero, (-g[x]) / m) for x in range(3)], -1)
    # faces: per axis the keep mask and the four cells' vertices of every lattice point, then the kept rows in row order
    pad = torch.full((nx + 1, ny + 1, nz + 1), -1, dtype=torch.int32, device=dev)      # pad[c + 1] = cell_vertex[c]; -1 for a cell that does not exist
    pad[1:nx, 1:ny, 1:nz] = cell_vertex
    dims = (nx, ny, nz)
    keep, quads = [], []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        cross = torch.zeros_like(inside)
        head, tail = [slice(None)] * 3, [slice(None)] * 3
        head[a], tail[a] = slice(0, dims[a] - 1), slice(1, dims[a])
        cross[tuple(head)] = inside[tuple(head)] != inside[tuple(tail)]
        q = []
        for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            sl = [None] * 3
            sl[a], sl[u], sl[v] = slice(1, dims[a] + 1), slice(1 + du, dims[u] + 1 + du), slice(1 + dv, dims[v] + 1 + dv)
            q.append(pad[tuple(sl)])
        q = torch.stack(q, -1)                                                 # [nx,ny,nz,4]
        keep.append(cross & (q >= 0).all(-1))
        quads.append(torch.where(inside[..., None], q, q.flip(-1)))
    keep = torch.stack(keep, -1).reshape(-1)                                   # row r = point * 3 + a
    quads = torch.stack(quads, -2).reshape(-1, 4)[keep]
    faces = torch.stack((quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]), 1).reshape(-1, 3).contiguous()
    return {"vertices": vertices.reshape(-1, 3), "normals": normals.reshape(-1, 3), "faces": faces, "cell_vertex": cell_vertex}


def _overflow(what, needed, cap):
    if needed > cap:
        raise RuntimeError("surface_nets kept %d %s, the buffers hold %d: pass capacity >= (vertices, faces) with %s >= %d"
                           % (needed, what, cap, what, needed))


@torch.no_grad()
def surface_nets(field, iso, lo, h, index0=(0, 0, 0), device=None, capacity=None):
    """surface_nets_reference on the device (pag_mesh_vertices / pag_mesh_faces: two ordered appends), same dict, same bits; the tensors stay on the
    field's device (a CPU field goes to `device`, default "cuda", and the result comes back; device="cpu" is the definition).
    Sizing: by default the vertex launches run once as a count (they also fill cell_vertex) and ONE read of the counter sizes the buffers - V
    vertices and 6 V faces, the most V vertices can carry: a quad has four of the 12 V (cell, edge) pairs; the launches then run again into the
    buffers and a SECOND read trims the faces.  capacity=(V, F): one read at the end; more vertices or faces than that raises with the counts."""
    f = _check_field(field, "surface_nets")
    home = f.device
    dev = torch.device(device) if device is not None else (home if home.type != "cpu" else torch.device("cuda"))
    if dev.type == "cpu":
        out = surface_nets_reference(f.cpu(), iso, lo, h, index0)
        return {k: v.to(home) for k, v in out.items()}
    lo, h, index0 = _frame(lo, h, index0)
    f = f.to(dev).contiguous()
    nx, ny, nz = f.shape
    cell_vertex = torch.empty(nx - 1, ny - 1, nz - 1, dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)                      # [vertices, quads]
    if capacity is None:
        ops.mesh_vertices(f, iso, lo, h, index0, None, None, cell_vertex, count[0:1])
        cap_v = int(count[0].item())                                           # the first read
        cap_f = 6 * cap_v
        count.zero_()
    else:
        cap_v, cap_f = (int(c) for c in capacity)
    vertices, normals = torch.empty(cap_v, 3, device=dev), torch.empty(cap_v, 3, device=dev)
    faces = torch.empty(cap_f, 3, dtype=torch.int32, device=dev)
    ops.mesh_vertices(f, iso, lo, h, index0, vertices, normals, cell_vertex, count[0:1])
    ops.mesh_faces(f, iso, cell_vertex, faces, count[1:2])
    V, Q = count.tolist()                                                      # the last read
    _overflow("vertices", V, cap_v)
    _overflow("faces", 2 * Q, cap_f)
    out = {"vertices": vertices[:V], "normals": normals[:V], "faces": faces[:2 * Q] if capacity is not None else faces[:2 * Q].clone(),
           "cell_vertex": cell_vertex}
    return {k: v.to(home) for k, v in out.items()}


@torch.no_grad()
def density_lattice(nef, resolution, limits=None, batch=1 << 20):
    """The nef's density on the lattice i / resolution * 2 - 1, i = 0 .. resolution (f32), queried AT the lattice points (not with the shift of the
    reference's get_dense_occupied_points) `batch` points at a time.  limits [2,3] = [[min], [max]] keeps the index sub-box strictly inside, as
    _lattice_box does.  -> (field f32 [nx,ny,nz] on the nef's device, lo = -1.0, h = 2 / resolution, index0 = the global index of field[0,0,0])."""
    resolution = int(resolution)
    if resolution < 1:
        raise ValueError("density_lattice: resolution must be >= 1")
    dev = nef.device
    axis = torch.arange(resolution + 1, dtype=torch.float32) / float(resolution) * 2.0 - 1.0
    if limits is None or torch.as_tensor(limits).numel() == 0:
        keep = [torch.arange(resolution + 1)] * 3
    else:
        lim = torch.as_tensor(limits, dtype=torch.float32).cpu()
        keep = [torch.nonzero((axis > lim[0, a]) & (axis < lim[1, a])).reshape(-1) for a in range(3)]
    if min(int(k.numel()) for k in keep) < 2:
        raise ValueError("density_lattice: fewer than 2 lattice points strictly inside the limits on an axis")
    ax = [axis[k].to(dev) for k in keep]
    nx, ny, nz = (int(k.numel()) for k in keep)
    P = nx * ny * nz
    field = torch.empty(P, dtype=torch.float32, device=dev)
    batch = max(1, int(batch))
    for s in range(0, P, batch):
        e = min(s + batch, P)
        i = torch.arange(s, e, device=dev)
        points = torch.stack((ax[0][i // (ny * nz)], ax[1][(i // nz) % ny], ax[2][i % nz]), -1)
        field[s:e] = nef(coords=points[:, None], ray_d=None, channels="density").reshape(-1).float()
    return field.reshape(nx, ny, nz), -1.0, 2.0 / resolution, tuple(int(k[0]) for k in keep)


def _argmax_ids(rows):
    """torch.argmax of every row of rows f32 [n, I] by the map export's kernel (pag_map_select with a predicate that keeps every row) -> i64 [n]."""
    n = rows.shape[0]
    out = MapAccumulator(n, rows.device, color=False)
    if n:
        ops.map_select(torch.zeros(n, 3, device=rows.device), out.points, out.count, value=torch.ones(n, device=rows.device), threshold=0.0,
                       inst=rows, ids_out=out.ids)
    return out.ids


@torch.no_grad()
def extract_mesh(nef, resolution=256, min_density=None, limits=None, color=True, channels=DEFAULT_CHANNELS, labels="argmax", batch=1 << 20,
                 name="nerf_mesh"):
    """The panoptic mesh of a trained nef: density_lattice, surface_nets at iso = min_density (default: get_dense_occupied_points' 0.01 * 512 /
    sqrt(3)), then per vertex, `batch` vertices at a time, the label of every channel of `channels` the nef has ('inst_embedding' -> 'instances'
    through `labels`: 'argmax' - the map export's kernel - or a callable f(embedding [n,D]) -> i64 [n], as in generate_pc_map; 'semantics' ->
    'semantics' by argmax) and with color=True the 'rgb' channel seen along ray_d = -normal, a camera looking straight at the surface ((0,0,-1)
    for a zero normal).  A channel the nef lacks is left out when `channels` is the default and raises when it was asked for.
    -> {'name', 'vertices' f32 [V,3], 'normals' f32 [V,3], 'faces' i32 [F,3], 'instances' / 'semantics' i64 [V], 'color' f32 [V,3]} on the device."""
    if labels != "argmax" and not callable(labels):
        raise ValueError("labels must be 'argmax' or a callable f(inst_embedding [n, D]) -> int64 [n]")
    names = {"inst_embedding": "instances", "semantics": "semantics"}
    unknown = [c for c in channels if c not in names]
    if unknown:
        raise ValueError("extract_mesh: channels are 'inst_embedding' and / or 'semantics', got %r" % (unknown,))
    supported = nef.get_supported_channels()
    if channels is DEFAULT_CHANNELS:
        channels = tuple(c for c in channels if c in supported)
    missing = [c for c in tuple(channels) + (("rgb",) if color else ()) if c not in supported]
    if missing:
        raise ValueError("extract_mesh: %s has no channel %s" % (type(nef).__name__, ", ".join(missing)))
    if min_density is None:
        min_density = (0.01 * 512) / np.sqrt(3)
    field, lo, h, index0 = density_lattice(nef, resolution, limits, batch)
    mesh = surface_nets(field, min_density, lo, h, index0)
    del field
    vertices, normals = mesh["vertices"], mesh["normals"]
    V, dev = vertices.shape[0], vertices.device
    out = {"name": name, "vertices": vertices, "normals": normals, "faces": mesh["faces"]}
    for c in channels:
        out[names[c]] = torch.empty(V, dtype=torch.int64, device=dev)
    if color:
        out["color"] = torch.empty(V, 3, dtype=torch.float32, device=dev)
    batch = max(1, int(batch))
    for s in range(0, V, batch):
        pts = vertices[s:s + batch]
        for c in channels:
            emb = nef(coords=pts[:, None], ray_d=None, channels=c)
            inst, ids = _labels_of(labels if c == "inst_embedding" else "argmax", emb)
            out[names[c]][s:s + batch] = ids if ids is not None else _argmax_ids(inst.float())
        if color:
            nrm = normals[s:s + batch]
            ray_d = torch.where((nrm == 0).all(-1, keepdim=True), torch.tensor([0.0, 0.0, -1.0], device=dev), -nrm)
            out["color"][s:s + batch] = nef(coords=pts[:, None], ray_d=ray_d, channels="rgb").reshape(-1, 3).float()
    return out


_PLY_TYPES = {"float": "<f4", "uchar": "u1", "int": "<i4"}


def save_mesh(mesh, path):
    """A little-endian binary PLY, written with numpy only: element vertex with x y z nx ny nz float, red green blue uchar when the mesh has 'color'
    (save_map's bytes: rint(clip(nan_to_num(c), 0, 1) * 255)), instance / semantic int when it has 'instances' / 'semantics'; element face with
    `property list uchar int vertex_indices`."""
    arr = lambda k, dt: np.ascontiguousarray(np.asarray(mesh[k].detach().cpu() if torch.is_tensor(mesh[k]) else mesh[k], dtype=dt))      # noqa: E731
    v, n, f = arr("vertices", "<f4").reshape(-1, 3), arr("normals", "<f4").reshape(-1, 3), arr("faces", "<i4").reshape(-1, 3)
    fields = [(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")]
    if mesh.get("color") is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    fields += [(p, "<i4") for k, p in (("instances", "instance"), ("semantics", "semantic")) if mesh.get(k) is not None]
    rows = np.empty(v.shape[0], dtype=fields)
    for j, k in enumerate(("x", "y", "z")):
        rows[k], rows["n" + k] = v[:, j], n[:, j]
    if mesh.get("color") is not None:
        col = np.rint(np.clip(np.nan_to_num(arr("color", np.float32).reshape(-1, 3)), 0.0, 1.0) * 255.0).astype(np.uint8)
        rows["red"], rows["green"], rows["blue"] = col[:, 0], col[:, 1], col[:, 2]
    for k, p in (("instances", "instance"), ("semantics", "semantic")):
        if mesh.get(k) is not None:
            rows[p] = arr(k, np.int64).reshape(-1).astype("<i4")
    tri = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    tri["n"], tri["v"] = 3, f
    names = {t: s for s, t in _PLY_TYPES.items()}
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % v.shape[0]
    header += "".join("property %s %s\n" % (names[t], k) for k, t in fields)
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % f.shape[0]
    with open(str(path), "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rows.tobytes())
        fh.write(tri.tobytes())
    return str(path)


def load_mesh(path):
    """What save_mesh wrote -> {'vertices', 'normals' f32 [V,3], 'faces' i32 [F,3], 'color' u8 [V,3] (the stored bytes), 'instances' / 'semantics'
    i64 [V]} as CPU tensors, each only when the file has it."""
    with open(str(path), "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("%s: not a binary little-endian PLY" % path)
    counts, fields, element = {}, [], None
    for line in lines[2:]:
        w = line.split()
        if w[:1] == ["element"]:
            element, counts[w[1]] = w[1], int(w[2])
        elif w[:1] == ["property"] and element == "vertex":
            fields.append((w[2], _PLY_TYPES[w[1]]))
        elif w[:1] == ["property"] and element == "face" and w[1:] != ["list", "uchar", "int", "vertex_indices"]:
            raise ValueError("%s: faces must be `property list uchar int vertex_indices`" % path)
    V, F = counts.get("vertex", 0), counts.get("face", 0)
    vdt = np.dtype(fields)
    rows = np.frombuffer(data, dtype=vdt, count=V, offset=end)
    tri = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=F, offset=end + V * vdt.itemsize)
    if F and not (tri["n"] == 3).all():
        raise ValueError("%s: a face that is not a triangle" % path)
    has = {k for k, _ in fields}
    out = {"vertices": torch.from_numpy(np.stack([rows[k] for k in ("x", "y", "z")], -1).astype(np.float32)),
           "normals": torch.from_numpy(np.stack([rows[k] for k in ("nx", "ny", "nz")], -1).astype(np.float32)),
           "faces": torch.from_numpy(tri["v"].astype(np.int32).reshape(-1, 3))}
    if "red" in has:
        out["color"] = torch.from_numpy(np.stack([rows[k] for k in ("red", "green", "blue")], -1).astype(np.uint8))
    for k, p in (("instances", "instance"), ("semantics", "semantic")):
        if p in has:
            out[k] = torch.from_numpy(rows[p].astype(np.int64))
    return out


def mesh_report(mesh):
    """Plain tensor ops in float64 on a CPU copy -> {'vertices', 'faces', 'edges' (undirected), 'closed' (every edge in exactly two faces),
    'oriented' (every directed edge exactly once, its reverse present), 'euler' = V - E + F, 'area', 'volume' (signed, the divergence theorem:
    positive when the face normals point outwards)}."""
    v = torch.as_tensor(mesh["vertices"]).detach().cpu().to(torch.float64).reshape(-1, 3)
    f = torch.as_tensor(mesh["faces"]).detach().cpu().to(torch.int64).reshape(-1, 3)
    V, F = int(v.shape[0]), int(f.shape[0])
    a, b = torch.cat((f[:, 0], f[:, 1], f[:, 2])), torch.cat((f[:, 1], f[:, 2], f[:, 0]))
    stride = max(V, 1)
    directed, n_directed = torch.unique(a * stride + b, return_counts=True)
    undirected, n_undirected = torch.unique(torch.minimum(a, b) * stride + torch.maximum(a, b), return_counts=True)
    reverse = torch.unique(b * stride + a)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cr = torch.cross(p1 - p0, p2 - p0, dim=-1)
    return {"vertices": V, "faces": F, "edges": int(undirected.numel()),
            "closed": bool((n_undirected == 2).all()), "oriented": bool((n_directed == 1).all() and torch.equal(directed, reverse)),
            "euler": V - int(undirected.numel()) + F, "area": float(0.5 * torch.linalg.norm(cr, dim=-1).sum()),
            "volume": float((p0 * torch.cross(p1, p2, dim=-1)).sum() / 6.0)}


def report_line(report):
    """mesh_report's dict as the one line the train command prints."""
    return ("mesh: %(vertices)d vertices, %(faces)d faces, %(edges)d edges, closed %(closed)s, oriented %(oriented)s, euler %(euler)d, "
            "area %(area).6g, volume %(volume).6g") % report
