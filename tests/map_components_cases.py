"""The connected-component cases shared by tests/test_map_components_host.py and tests/test_gpu_map_components.py: fused maps built directly from
voxel indices and ids (no rendering), a breadth-first search over a dict as a second, independent form of the definition, and comparison helpers.
Every case is a name; case(name) -> (map dict on the CPU, keyword arguments of connected_components)."""
import collections
import itertools

import numpy as np
import torch

TOP = 2 ** 21 - 1                                          # the last index of an axis
ORIGIN = (-1.0, -1.0, -1.0)
MAP_KEYS = ("points", "color", "instances", "count", "agreement", "voxels", "component")


def key_of(vox):
    v = np.asarray(vox, np.int64).reshape(-1, 3)
    return v[:, 2] | (v[:, 1] << 21) | (v[:, 0] << 42)


def make_map(vox, ids, color=True, sort=True, voxel_size=2.0 ** -20):
    """A fused-map dict as VoxelMap.finish returns it: rows ascending by key (sort=False: as given, for the contract cases), points the voxel centres,
    counts 1 + row % 5, colours multiples of 1 / 256."""
    vox = np.asarray(vox, np.int64).reshape(-1, 3)
    ids = np.broadcast_to(np.asarray(ids, np.int64), (vox.shape[0],)).copy()
    if sort:
        order = np.argsort(key_of(vox), kind="stable")
        vox, ids = vox[order], ids[order]
        assert (np.diff(key_of(vox)) > 0).all(), "a voxel twice"
    n = vox.shape[0]
    m = dict(points=torch.from_numpy(((vox + 0.5) * voxel_size - 1.0).astype(np.float32)), instances=torch.from_numpy(ids),
             count=torch.from_numpy((1 + np.arange(n) % 5).astype(np.int32)), agreement=torch.ones(n), voxels=torch.from_numpy(vox.astype(np.int32)),
             voxel_size=voxel_size, origin=torch.tensor(ORIGIN))
    if color:
        m["color"] = torch.from_numpy((np.arange(n * 3).reshape(n, 3) % 257 / 256.0).astype(np.float32))
    return m


def lattice(seed, n_ids):
    """A 24^3 lattice occupied at p = 0.3; one id (n_ids = 1) or ids drawn from 1 .. n_ids."""
    rng = np.random.default_rng(seed)
    vox = np.argwhere(rng.random((24, 24, 24)) < 0.3)
    ids = np.ones(vox.shape[0], np.int64) if n_ids == 1 else rng.integers(1, n_ids + 1, vox.shape[0])
    return vox, ids


def serpentine(n=16):
    """Every cell of an n^3 block visited by one path of face steps: x back and forth inside a row, the rows back and forth inside a layer."""
    path = []
    for z in range(n):
        ys = range(n) if z % 2 == 0 else range(n - 1, -1, -1)
        for row, y in enumerate(ys):
            xs = range(n) if (z * n + row) % 2 == 0 else range(n - 1, -1, -1)
            path += [(x, y, z) for x in xs]
    return np.array(path)


def blob(corner, shape):
    return np.array([(corner[0] + x, corner[1] + y, corner[2] + z) for x in range(shape[0]) for y in range(shape[1]) for z in range(shape[2])])


def x_line_with_fillers(n=600, fillers=40):
    """A line along x at (., 7, 7) with id 1; between successive line voxels in key order `fillers` voxels of id 2 at (x, 100 + 2 k, 9): the line's links
    lie fillers + 1 rows apart.  The fillers of one x are two cells apart; those of neighbouring x touch by faces (lines of their own along x)."""
    line = np.array([(x, 7, 7) for x in range(n)])
    fill = np.array([(x, 100 + 2 * k, 9) for x in range(n) for k in range(fillers)])
    return np.concatenate([line, fill]), np.concatenate([np.full(n, 1), np.full(fill.shape[0], 2)])


# (9, TOP, TOP) and (10, 0, 0) have consecutive keys and are no neighbours; the last pair is one component; everything else is alone
BORDER_VOXELS = [(5, 5, 0), (5, 4, TOP), (5, 0, 7), (4, TOP, 7), (0, 0, 0), (TOP, TOP, TOP), (9, TOP, TOP), (10, 0, 0), (TOP - 3, TOP, TOP - 1),
                 (TOP - 3, TOP, TOP)]
CLEAN_SPECKS = [(30, 30, 30), (2, 40, 2), (45, 3, 3)]


def clean_voxels(first=(5, 4, 2), second=(2, 2, 3)):
    """Case 10: id 5 on a blob of `first` (40 voxels) at (10, 10, 10) and a blob of `second` (12 voxels) at (18, 10, 10), three empty cells after the
    first along x; three single specks of id 5; a 3 x 3 x 1 background patch of id 0.  In key order the components are: speck (2, 40, 2), first blob,
    second blob, speck (30, 30, 30), speck (45, 3, 3); the background rows come last."""
    assert first[0] <= 5
    a, b = blob((10, 10, 10), first), blob((18, 10, 10), second)
    specks, back = np.array(CLEAN_SPECKS), blob((60, 60, 60), (3, 3, 1))
    vox = np.concatenate([a, b, specks, back])
    ids = np.concatenate([np.full(a.shape[0] + b.shape[0] + 3, 5), np.zeros(back.shape[0], np.int64)])
    return vox, ids


def case(name):
    kw = {}
    if name.startswith("one_id_"):                                                         # 1
        vox, ids = lattice(1, 1)
        kw = dict(connectivity=int(name[7:]))
    elif name.startswith("five_ids_"):                                                     # 2: five_ids_<seed>_<connectivity>_<same|any|no3>
        _, _, seed, conn, how = name.split("_")
        vox, ids = lattice(int(seed), 5)
        kw = dict(connectivity=int(conn), same_id=how != "any", ignore=(0, 3) if how == "no3" else (0,))
    elif name == "z_line":                                                                 # 3
        vox, ids = np.array([(3, 4, z) for z in range(600)]), 1
    elif name == "x_line":
        vox, ids = x_line_with_fillers()
    elif name == "serpentine":                                                             # 4
        vox, ids = serpentine(), 9
        kw = dict(connectivity=6)
    elif name.startswith("contact_"):                                                      # 5
        vox = np.array([(4, 4, 4), (5, 5, 5), (9, 4, 4), (10, 5, 4), (14, 4, 4), (15, 4, 4), (19, 4, 4), (19, 5, 4), (24, 4, 4), (24, 4, 5)])
        ids = np.array([1, 1, 1, 1, 1, 1, 1, 2, 1, 1])                                     # corner, edge, face, face with two ids, face along z
        kw = dict(connectivity=int(name[8:]))
    elif name.startswith("borders_"):                                                      # 6
        vox = np.array(BORDER_VOXELS)
        ids = 1
        kw = dict(connectivity=int(name[8:]))
    elif name.startswith("checker_"):                                                      # 7
        vox, ids = np.array([c for c in itertools.product(range(12), repeat=3) if sum(c) % 2 == 0]), 4
        kw = dict(connectivity=int(name[8:]))
    elif name.startswith("bridge_"):                                                       # 8
        vox, ids = bridge_voxels(), 1
        kw = dict(connectivity=int(name[7:]))
    elif name == "empty":                                                                  # 9
        vox, ids = np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    elif name == "single":
        vox, ids = np.array([(7, 7, 7)]), 3
    elif name == "all_ignored":
        vox, ids = blob((1, 1, 1), (4, 4, 4)), 0
    else:
        raise KeyError(name)
    return make_map(vox, ids), kw


def bridge_voxels():
    """Two 8^3 blobs, [0, 8)^3 and [0, 8) x [9, 17) x [0, 8), and one voxel (8, 8, 7) that shares an edge with (7, 7, 7) of the first and with
    (7, 9, 7) of the second: its x is the largest, so it is the map's last row, and it joins the blobs under 18 and 26 neighbours, not under 6."""
    return np.concatenate([blob((0, 0, 0), (8, 8, 8)), blob((0, 9, 0), (8, 8, 8)), np.array([(8, 8, 7)])])


CASES_1_TO_9 = (["one_id_%d" % c for c in (6, 18, 26)]
                + ["five_ids_%d_%d_%s" % (seed, c, how) for seed in range(5) for c in (6, 18, 26) for how in ("same", "any", "no3")]
                + ["z_line", "x_line", "serpentine"] + ["%s_%d" % (n, c) for n in ("contact", "borders", "checker", "bridge") for c in (6, 18, 26)]
                + ["empty", "single", "all_ignored"])


def contract_maps():
    """Case 12: rows out of key order, a key twice, an index of 2^21 (and a negative one)."""
    good = blob((3, 3, 3), (3, 3, 3))
    swapped = good.copy()
    swapped[[4, 20]] = swapped[[20, 4]]
    twice = np.concatenate([good[:10], good[9:]])
    beyond = np.concatenate([good, np.array([(4, 4, 2 ** 21)])])
    below = np.concatenate([np.array([(-1, 4, 4)]), good])
    return {"order": make_map(swapped, 1, sort=False), "duplicate": make_map(twice, 1, sort=False), "beyond": make_map(beyond, 1, sort=False),
            "negative": make_map(below, 1, sort=False)}


# ------------------------------------------------------------------------------------------- the definition once more, by breadth-first search
def bfs_components(m, connectivity=26, same_id=True, ignore=(0,)):
    """-> (component list, count): a dict of voxels, a queue per unvisited row in row order (so components are numbered by their first row)."""
    vox = [tuple(v) for v in m["voxels"].tolist()]
    ids = m["instances"].tolist()
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    offsets = [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(c != 0 for c in o) <= most]
    row_of = {v: r for r, v in enumerate(vox)}
    comp = [0] * len(vox)
    count = 0
    for r0 in range(len(vox)):
        if comp[r0] or ids[r0] in ignore:
            continue
        count += 1
        comp[r0] = count
        queue = collections.deque([r0])
        while queue:
            r = queue.popleft()
            for o in offsets:
                nb = (vox[r][0] + o[0], vox[r][1] + o[1], vox[r][2] + o[2])
                if not all(0 <= c <= TOP for c in nb):
                    continue
                j = row_of.get(nb)
                if j is None or comp[j] or ids[j] in ignore or (same_id and ids[j] != ids[r]):
                    continue
                comp[j] = count
                queue.append(j)
    return comp, count


def assert_same(got, want, keys, what=""):
    """torch.equal on every tensor of `keys` that either side has, same shapes and dtypes."""
    for k in keys:
        assert (k in got) == (k in want), (what, k)
        if k in want:
            g, w = got[k].cpu(), want[k].cpu()
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
            assert torch.equal(g, w), (what, k)
