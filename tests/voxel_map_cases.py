"""The voxel-map cases shared by tests/test_voxel_map_host.py and tests/test_gpu_voxel_map.py: seeded point clouds, the exactly representable ones
among them (every fp32 sum of a run is exact in any order, so the device path must equal the fp64 definition bit for bit), a brute-force fusion in
plain Python, and the comparison helpers."""
import collections

import numpy as np
import torch

# seven ids: negative ones, zero, small ones and two beyond 2^31
IDS = np.array([-5, -1, 0, 3, 7, (1 << 31) + 3, 1 << 40], np.int64)
ORIGIN = (-1.0, -1.0, -1.0)
FUSED_KEYS = ("points", "color", "instances", "count", "agreement", "voxels")
TABLE_KEYS = ("ids", "voxels", "observations", "centroid", "bbox_min", "bbox_max", "color", "volume")


def exact_cloud(runs, G, q, seed, color=True, shuffle=True):
    """runs: [(voxel (ix, iy, iz) on the lattice of G cells per axis, ids of the members)] -> dict(points, ids, color, voxel_size = 2 / G).  Coordinates
    are multiples of 1 / q inside the member's voxel, colours multiples of 1 / 256 in [0, 1].  Checks what makes fp32 sums exact: G and q are powers
    of two with G <= q, and members * q <= 2^24 for every run (|x| <= 1: every partial sum is a multiple of 1 / q below 2^24 / q)."""
    assert G & (G - 1) == 0 and q & (q - 1) == 0 and G <= q
    rs = np.random.RandomState(seed)
    per_cell = 2 * q // G                                  # positions per axis inside one voxel
    pts, ids = [], []
    for voxel, members in runs:
        members = np.asarray(members, np.int64)
        assert 1 <= members.size and members.size * q <= 1 << 24 and members.size * 256 <= 1 << 24, "a run too long for exact fp32 sums"
        assert all(0 <= v < G for v in voxel)
        steps = np.asarray(voxel, np.int64)[None, :] * per_cell + rs.randint(0, per_cell, (members.size, 3))
        pts.append((steps.astype(np.float64) / q - 1.0).astype(np.float32))
        ids.append(members)
    pts, ids = np.concatenate(pts), np.concatenate(ids)
    assert np.abs(pts).max() <= 1.0 and np.array_equal(pts * q, np.round(pts * q))
    col = (rs.randint(0, 257, (pts.shape[0], 3)) / 256.0).astype(np.float32)
    order = rs.permutation(pts.shape[0]) if shuffle else np.arange(pts.shape[0])
    out = dict(points=torch.from_numpy(pts[order]), ids=torch.from_numpy(ids[order]), voxel_size=2.0 / G)
    out["color"] = torch.from_numpy(col[order]) if color else None
    return out


def distinct_voxels(count, G, rs):
    flat = rs.permutation(G ** 3)[:count]
    return [(int(f // (G * G)), int(f // G % G), int(f % G)) for f in flat]


def straddle_runs(K, rs):
    """K rows in two or three voxels whose sorted runs cross row 64 (K >= 65) or row 256 (K >= 257): a run that starts in one wave / block and ends in
    the next."""
    lengths = [50, K - 50] if K < 200 else [40, 200, K - 240]
    voxels = sorted(distinct_voxels(len(lengths), 16, rs))
    return [(v, IDS[rs.randint(0, 7, n)]) for v, n in zip(voxels, lengths)]


def tie_runs(rs, voxels=300):
    """Run lengths 1..40 over 300 voxels, 7 ids; every even-length run is split evenly between two ids (a tie the smaller id must win), every run
    of a length divisible by three between three."""
    runs = []
    for i, v in enumerate(distinct_voxels(voxels, 16, rs)):
        n = 1 + i % 40
        if n % 3 == 0:
            a = rs.choice(7, 3, replace=False)
            members = np.repeat(IDS[a], n // 3)
        elif n % 2 == 0:
            a = rs.choice(7, 2, replace=False)
            members = np.repeat(IDS[a], n // 2)
        else:
            members = IDS[rs.randint(0, 7, n)]
        runs.append((v, rs.permutation(members)))
    return runs


def exact_case(name):
    """-> (cloud dict of exact_cloud, keyword arguments of the fusion)."""
    rs = np.random.RandomState(sum(map(ord, name)))
    if name == "k1":
        return exact_cloud([((3, 0, 15), IDS[[5]])], 16, 64, 1), {}
    if name.startswith("straddle"):
        return exact_cloud(straddle_runs(int(name[8:]), rs), 16, 64, 2), {}
    if name == "own_voxel_1000":
        return exact_cloud([(v, IDS[rs.randint(0, 7, 1)]) for v in distinct_voxels(1000, 16, rs)], 16, 64, 3), {}
    if name == "one_voxel_65536":
        return exact_cloud([((7, 8, 9), IDS[rs.randint(0, 7, 65536)])], 16, 64, 4), {}
    if name == "ties_300":
        return exact_cloud(tie_runs(rs), 16, 64, 5), {}
    if name == "ties_300_no_color":
        return exact_cloud(tie_runs(rs), 16, 64, 5, color=False), {}
    if name == "min_votes_3":
        return exact_cloud(tie_runs(rs), 16, 64, 6), dict(min_votes=3)
    if name == "limits":
        return exact_cloud(tie_runs(rs), 16, 64, 7), dict(limits=[[-0.5, -0.75, -1.0], [0.5, 0.25, 0.875]])
    raise KeyError(name)


EXACT_CASES = ("k1", "straddle63", "straddle64", "straddle65", "straddle255", "straddle256", "straddle257", "own_voxel_1000", "one_voxel_65536",
               "ties_300", "ties_300_no_color", "min_votes_3", "limits")


def dropped_rows(n, seed):
    """Rows that every fusion drops: NaN, +-inf, below the origin, beyond 2^21 cells - with finite rows mixed into the coordinates that stay."""
    rs = np.random.RandomState(seed)
    p = (rs.randint(-64, 65, (n, 3)) / 64.0).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, -1.5, -1.0 - 2.0 ** -20, 4.0e6], np.float32)
    p[np.arange(n), rs.randint(0, 3, n)] = bad[rs.randint(0, bad.size, n)]
    return torch.from_numpy(p), torch.from_numpy(IDS[rs.randint(0, 7, n)]), torch.from_numpy((rs.randint(0, 257, (n, 3)) / 256.0).astype(np.float32))


def random_cloud(K=20000, cells=13, seed=11):
    """K uniform fp32 points in (-1, 1)^3 with 7 ids and colours: about cells^3 voxels of edge 2 / cells."""
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-1.0, 1.0, (K, 3)).astype(np.float32)
    return dict(points=torch.from_numpy(pts), ids=torch.from_numpy(IDS[rs.randint(0, 7, K)]),
                color=torch.from_numpy(rs.rand(K, 3).astype(np.float32)), voxel_size=2.0 / cells)


def exact_table_map(sizes, seed, color=True):
    """A fused-map dict (CPU) whose label i owns sizes[i] voxel rows, rows shuffled; points multiples of 1/64, colours of 1/256: exact fp32 sums for
    sizes up to 2^18."""
    rs = np.random.RandomState(seed)
    assert max(sizes) * 64 <= 1 << 24
    labels = np.repeat(np.arange(len(sizes), dtype=np.int64) * 3 - 6, sizes)               # ids -6, -3, 0, 3, ...: 0 is among them
    n = labels.size
    order = rs.permutation(n)
    m = dict(points=torch.from_numpy((rs.randint(-64, 65, (n, 3)) / 64.0).astype(np.float32)), instances=torch.from_numpy(labels[order]),
             count=torch.from_numpy(rs.randint(1, 50, n).astype(np.int32)), agreement=torch.ones(n), voxels=torch.zeros(n, 3, dtype=torch.int32),
             voxel_size=2.0 / 64, origin=torch.tensor(ORIGIN))
    if color:
        m["color"] = torch.from_numpy((rs.randint(0, 257, (n, 3)) / 256.0).astype(np.float32))
    return m


# ------------------------------------------------------------------------------------------- brute force
def brute_fuse(points, ids, color, voxel_size, origin=ORIGIN, limits=None, min_votes=1):
    """The fusion with a Python dict: numpy scalars in fp32 for the key, fp64 sums, one fp32 division."""
    p = points.numpy().astype(np.float32)
    o, v = np.asarray(origin, np.float32), np.float32(voxel_size)
    cells = collections.defaultdict(list)
    for r in range(p.shape[0]):
        if not np.isfinite(p[r]).all():
            continue
        with np.errstate(over="ignore"):
            idx = np.floor((p[r] - o) / v)
        if not ((idx >= 0) & (idx < 2 ** 21)).all():
            continue
        if limits is not None and not ((p[r] > np.asarray(limits[0], np.float32)) & (p[r] < np.asarray(limits[1], np.float32))).all():
            continue
        cells[tuple(int(i) for i in idx)].append(r)
    out = collections.defaultdict(list)
    for voxel in sorted(cells):                            # tuples sort with x slowest
        rows = cells[voxel]
        if len(rows) < min_votes:
            continue
        n = np.float32(len(rows))
        votes = collections.Counter(int(ids[r]) for r in rows)
        top = max(votes.values())
        out["points"].append(p[rows].astype(np.float64).sum(0).astype(np.float32) / n)
        if color is not None:
            out["color"].append(color.numpy()[rows].astype(np.float64).sum(0).astype(np.float32) / n)
        out["instances"].append(min(i for i, c in votes.items() if c == top))
        out["count"].append(len(rows))
        out["agreement"].append(np.float32(top) / n)
        out["voxels"].append(voxel)
    V = len(out["count"])
    res = dict(points=torch.tensor(np.array(out["points"], np.float32).reshape(V, 3)), instances=torch.tensor(out["instances"], dtype=torch.int64),
               count=torch.tensor(out["count"], dtype=torch.int32), agreement=torch.tensor(np.array(out["agreement"], np.float32)),
               voxels=torch.tensor(np.array(out["voxels"], np.int32).reshape(V, 3)))
    if color is not None:
        res["color"] = torch.tensor(np.array(out["color"], np.float32).reshape(V, 3))
    return res


def brute_table(m, ignore=(0,)):
    rows = collections.defaultdict(list)
    for r, lab in enumerate(m["instances"].tolist()):
        if lab not in ignore:
            rows[lab].append(r)
    out = collections.defaultdict(list)
    for lab in sorted(rows):
        idx = rows[lab]
        n = np.float32(len(idx))
        p = m["points"].numpy()[idx]
        out["ids"].append(lab)
        out["voxels"].append(len(idx))
        out["observations"].append(int(m["count"].numpy()[idx].astype(np.int64).sum()))
        out["centroid"].append(p.astype(np.float64).sum(0).astype(np.float32) / n)
        out["bbox_min"].append(p.min(0))
        out["bbox_max"].append(p.max(0))
        if "color" in m:
            out["color"].append(m["color"].numpy()[idx].astype(np.float64).sum(0).astype(np.float32) / n)
    T = len(out["ids"])
    res = {k: torch.tensor(out[k], dtype=torch.int64) for k in ("ids", "voxels", "observations")}
    for k in ("centroid", "bbox_min", "bbox_max") + (("color",) if "color" in m else ()):
        res[k] = torch.tensor(np.array(out[k], np.float32).reshape(T, 3))
    res["volume"] = res["voxels"].double() * float(m["voxel_size"]) ** 3
    return res


# ------------------------------------------------------------------------------------------- comparisons
def assert_same(got, want, keys, what=""):
    """torch.equal on every tensor of `keys` that either side has (so a missing or an extra colour fails), same shapes and dtypes."""
    for k in keys:
        assert (k in got) == (k in want), (what, k)
        if k in want:
            g, w = got[k].cpu(), want[k].cpu()
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
            assert torch.equal(g, w), (what, k)


def run_mean_bound(values, inv, groups):
    """Per group and component: (fp64 mean, n * 2^-24 * max|x|) - the error bound of an fp32 sum of n terms in any order, (n - 1) u sum|x| <=
    (n - 1) u n max|x|, divided by n, plus the division's rounding u |mean| <= u max|x|, with u = 2^-24.  Derived, not tuned."""
    v = values.double()
    n = torch.zeros(groups, dtype=torch.float64).index_add_(0, inv, torch.ones(inv.numel(), dtype=torch.float64))
    mean = torch.zeros(groups, v.shape[1], dtype=torch.float64).index_add_(0, inv, v) / n[:, None]
    big = torch.zeros(groups, v.shape[1], dtype=torch.float64).scatter_reduce_(0, inv[:, None].expand(-1, v.shape[1]), v.abs(), "amax", include_self=False)
    return mean, n[:, None] * 2.0 ** -24 * big
