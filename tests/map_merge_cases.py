"""The cases shared by tests/test_map_merge_host.py and tests/test_gpu_map_merge.py: pairs (and one chain) of fused maps built directly from integer
voxel arrays, the results that can be written down by hand, and a second, independent form of the definitions over dicts and sets.
pair(name) -> (a, b, keyword arguments of associate_maps); EXPECT[name] -> what the association must give."""
import itertools

import numpy as np
import torch

from map_components_cases import TOP, blob, key_of, lattice, make_map  # noqa: F401

BIG = 2 ** 40


def with_votes(m, count, votes):
    """The map with the given counts and agreement = votes / count (fp32), so that rint(agreement * count) gives the votes back."""
    m = dict(m)
    m["count"] = torch.tensor(count, dtype=torch.int32)
    m["agreement"] = torch.tensor(votes, dtype=torch.float32) / m["count"].float()
    assert m["count"].numel() == m["instances"].numel()
    return m


def _cat(*parts):
    vox = np.concatenate([np.asarray(v, np.int64).reshape(-1, 3) for v, _ in parts])
    ids = np.concatenate([np.broadcast_to(np.asarray(i, np.int64), (np.asarray(v).reshape(-1, 3).shape[0],)) for v, i in parts])
    return vox, ids


def line(z0, n, x=3, y=4):
    return np.array([(x, y, z) for z in range(z0, z0 + n)], np.int64).reshape(-1, 3)


def _wave_rows():
    """Case 10, all on one column so that the rows keep this order and every 64 rows are one wave: a wave of 64 distinct pairs, two waves alternating
    between two pairs, then one wave each whose rows cycle through 1, 3, 7, 16 and 33 pairs of their own.  The combining loop's trip counts are the
    pairs of a wave: 64, 2, 2, 1, 3, 7, 16, 33 (big_pair adds full and partial waves of one pair)."""
    a_ids = [1 + z for z in range(64)] + [70 + z % 2 for z in range(128)]
    b_ids = [1001 + z for z in range(64)] + [1070 + z % 2 for z in range(128)]
    for first, pairs in ((100, 1), (110, 3), (120, 7), (130, 16), (150, 33)):
        a_ids += [first + z % pairs for z in range(64)]
        b_ids += [1000 + first + z % pairs for z in range(64)]
    return line(0, 512), np.array(a_ids), np.array(b_ids)


def _many(n):
    """Case 13: n single-voxel instances on either side, b's ids in the opposite order."""
    vox = np.array([(i, 0, 0) for i in range(n)])
    return make_map(vox, 1 + np.arange(n)), make_map(vox, 2 * n - np.arange(n))


def pair(name):
    kw = {}
    if name == "same_permuted":                                                            # 1
        vox, ids = lattice(1, 5)
        a, b = make_map(vox, ids), make_map(vox, np.array([0, 4, 5, 1, 2, 3])[ids])
    elif name == "disjoint":                                                               # 2
        a = make_map(*_cat((blob((0, 0, 0), (2, 2, 2)), 1), (blob((4, 0, 0), (2, 2, 1)), 2)))
        b = make_map(*_cat((blob((10, 0, 0), (2, 2, 2)), 4), (blob((14, 0, 0), (2, 1, 1)), 3), (blob((20, 0, 0), (2, 2, 1)), 0)))
    elif name == "window_cut":                                                             # 3: 40 voxels of a, the last x slab (8) shared
        a = make_map(*_cat((blob((10, 10, 10), (5, 4, 2)), 5), (blob((0, 0, 0), (2, 2, 2)), 1)))
        b = make_map(*_cat((blob((14, 10, 10), (3, 4, 2)), 2), (blob((30, 0, 0), (2, 2, 2)), 1)))
    elif name == "one_over_two":                                                           # 4
        a = make_map(line(0, 8), 1)
        b = make_map(*_cat((line(0, 6), 3), (line(6, 2), 4), (line(8, 3), 4)))
    elif name == "equal_iou":                                                              # 5
        a = make_map(line(0, 4), 1)
        b = make_map(*_cat((line(0, 2), 3), (line(2, 2), 4)))
    elif name == "equal_iou_mirrored":
        b, a, _ = pair("equal_iou")
    elif name == "background":                                                             # 6: without the background in r_1 the IoU of (1, 2) is 1
        a = make_map(*_cat((line(0, 10), 1), (line(20, 6), 0)))
        b = make_map(*_cat((line(0, 7), 0), (line(7, 3), 2), (line(20, 4), 6), (line(24, 2), 0)))
        kw = dict(min_iou=0.5)
    elif name == "threshold":                                                              # 7: IoU 1/2 and 1/3 at min_iou = 0.5
        a = make_map(*_cat((line(0, 4), 1), (line(10, 6), 2)))
        b = make_map(*_cat((line(0, 2), 3), (line(2, 2), 0), (line(10, 2), 4), (line(12, 4), 0)))
        kw = dict(min_iou=0.5)
    elif name == "five_by_two":                                                            # 8: a's id k on k + 1 voxels of column x = k
        a = make_map(*_cat(*[(line(0, k + 1, x=k), k) for k in range(1, 6)]))
        b = make_map(*_cat(*[(line(0, k + 1, x=k), 7 if k <= 3 else 8) for k in range(1, 6)]))
    elif name == "two_by_five":
        b, a, _ = pair("five_by_two")
    elif name == "big_pair":                                                               # 9: 4166 = 16 workgroups and 70 rows, the last wave partial
        a = make_map(*_cat((line(0, 4166), 1), (blob((9, 0, 0), (3, 5, 2)), 3)))
        b = make_map(*_cat((line(0, 4166), 2), (blob((1, 0, 0), (2, 2, 2)), 2)))
    elif name == "wave_pairs":                                                             # 10
        vox, ia, ib = _wave_rows()
        a, b = make_map(vox, ia), make_map(vox, ib)
    elif name == "below_and_above":                                                        # 11
        a = make_map(np.array([(0, 0, 0), (0, 0, 1), (5, 5, 5), (TOP, TOP, TOP)]), np.array([1, 1, 2, 3]))
        b = make_map(np.array([(5, 5, 5), (5, 5, 6), (6, 0, 0)]), np.array([4, 4, 5]))
    elif name == "one_row_b":
        a, b = make_map(line(0, 70), 1), make_map(line(33, 1), 9)
    elif name == "one_row_b_missing":
        a, b = make_map(line(0, 70), 1), make_map(line(90, 1), 9)
    elif name == "empty_a":
        a, b = make_map(np.zeros((0, 3), np.int64), np.zeros(0, np.int64)), make_map(line(0, 5), 2)
    elif name == "empty_b":
        b, a, _ = pair("empty_a")
    elif name == "both_empty":
        a = b = make_map(np.zeros((0, 3), np.int64), np.zeros(0, np.int64))
    elif name == "borders":                                                                # indices 0 and 2^21 - 1; (5,5,0) / (5,4,TOP): consecutive keys
        corners = [c for c in itertools.product((0, TOP), repeat=3)]
        a = make_map(np.array(corners + [(5, 5, 0), (7, 7, 7)]), np.array([1, 2, 3, 4, 1, 2, 3, 4, 5, 6]))
        b = make_map(np.array(corners + [(5, 4, TOP), (7, 7, 7)]), np.array([4, 3, 2, 1, 4, 3, 2, 1, 5, 9]))
    elif name == "signed_ids":                                                             # 12
        a = make_map(*_cat((line(0, 4), -3), (line(10, 5), 0), (line(20, 3), 7), (line(30, 6), BIG)))
        b = make_map(*_cat((line(0, 4), BIG), (line(10, 5), 0), (line(20, 2), -3), (line(30, 6), 7), (line(40, 2), 5), (line(50, 2), -8)))
    elif name in ("many_256", "many_257"):                                                 # 13
        a, b = _many(int(name[5:]))
    else:
        raise KeyError(name)
    return a, b, kw


PAIRS = ["same_permuted", "disjoint", "window_cut", "one_over_two", "equal_iou", "equal_iou_mirrored", "background", "threshold", "five_by_two",
         "two_by_five", "big_pair", "wave_pairs", "below_and_above", "one_row_b", "one_row_b_missing", "empty_a", "empty_b", "both_empty", "borders",
         "signed_ids", "many_256"]

# what can be written down by hand: pairs (id_a, id_b) ascending by id_a, mapping per ascending id of b, single table entries (id_a, id_b, shared)
EXPECT = {
    "same_permuted": dict(pairs=[(1, 4), (2, 5), (3, 1), (4, 2), (5, 3)], mapping=[3, 4, 5, 1, 2], iou_of_pairs=1.0),
    "disjoint": dict(pairs=[], mapping=[0, 5, 6], shared=0),
    "window_cut": dict(pairs=[(5, 2)], mapping=[6, 5], entries=[(5, 2, 8)], iou_of_pairs=1.0),
    "one_over_two": dict(pairs=[(1, 3)], mapping=[1, 5], entries=[(1, 3, 6), (1, 4, 2)]),
    "background": dict(pairs=[], mapping=[0, 7, 8], entries=[(1, 0, 7), (1, 2, 3), (0, 6, 4), (0, 0, 2)]),
    "threshold": dict(pairs=[(1, 3)], mapping=[0, 1, 5], iou_of_pairs=0.5),
    "five_by_two": dict(pairs=[(3, 7), (5, 8)], mapping=[3, 5]),
    "two_by_five": dict(pairs=[(7, 3), (8, 5)], mapping=[9, 10, 7, 11, 8]),
    "big_pair": dict(pairs=[(1, 2)], mapping=[1], entries=[(1, 2, 4166)], shared=4166),
    "below_and_above": dict(pairs=[(2, 4)], mapping=[2, 6], shared=1),
    "one_row_b": dict(pairs=[(1, 9)], mapping=[1], shared=1),
    "one_row_b_missing": dict(pairs=[], mapping=[10], shared=0),
    "empty_a": dict(pairs=[], mapping=[3], shared=0),
    "empty_b": dict(pairs=[], mapping=[], shared=0),
    "both_empty": dict(pairs=[], mapping=[], shared=0),
    "borders": dict(pairs=[(1, 4), (2, 3), (3, 2), (4, 1), (6, 9)], mapping=[4, 3, 2, 1, 10, 6], shared=9),
    "signed_ids": dict(pairs=[(-3, BIG), (7, -3), (BIG, 7)], mapping=[BIG + 1, 7, 0, BIG + 2, BIG, -3]),
}


def contract_pairs():
    """Case 14: -> {name: (a, b, text the ValueError must carry)}."""
    from map_components_cases import contract_maps
    good = make_map(blob((3, 3, 3), (3, 3, 3)), 1)
    bad = contract_maps()
    other_origin = dict(good, origin=torch.tensor((-1.0, -1.0, -0.5)))
    return {"order_a": (bad["order"], good, "ascend"), "order_b": (good, bad["duplicate"], "ascend"), "range_a": (bad["beyond"], good, r"outside \[0, 2\^21\)"),
            "range_b": (good, bad["negative"], r"outside \[0, 2\^21\)"), "voxel_size": (good, dict(good, voxel_size=2.0 ** -19), "voxel_size"),
            "origin": (good, other_origin, "origin")}


# ----------------------------------------------------------------------------------------------- the merge cases (15 - 20): an explicit mapping
def merge_case(color_a=True, color_b=True, component=False):
    """Six shared voxels on the column (3, 4, .) and singles of either map around them.  b's ids go through the identity mapping.
         z   a: id count votes   b: id count votes   result
         0      3    4     3        3    5     5      id 3, votes 8 of 9              (15: equal ids, the votes add)
         1      3    5     4        4    2     2      id 3, votes 4 of 7              (16: a has more votes)
         2      3    2     1        4    6     5      id 4, votes 5 of 8              (16: b has more votes)
         3      5    3     2        4    4     2      id 4, votes 2 of 7              (17: a tie, b's id is the smaller)
         4      3    3     3        4    7     3      id 3, votes 3 of 10             (17: a tie, a's id is the smaller)
         5      0    1     1        0    1     1      id 0, votes 2 of 2"""
    a_only, b_only = blob((1, 1, 1), (2, 2, 1)), blob((8, 1, 1), (1, 3, 1))
    a = make_map(*_cat((a_only, 3), (line(0, 6), np.array([3, 3, 3, 5, 3, 0]))), color=color_a)
    b = make_map(*_cat((line(0, 6), np.array([3, 4, 4, 4, 4, 0])), (b_only, 4)), color=color_b)
    a = with_votes(a, [3, 2, 5, 1, 4, 5, 2, 3, 3, 1], [2, 2, 3, 1, 3, 4, 1, 2, 3, 1])
    b = with_votes(b, [5, 2, 6, 4, 7, 1, 2, 3, 9], [5, 2, 5, 2, 3, 1, 1, 3, 5])
    b["points"] = b["points"] + torch.tensor(2.0 ** -23)                                  # the means of the shared voxels differ between the maps
    if component:
        a["component"] = torch.arange(a["count"].numel(), dtype=torch.int64)
    want = dict(instances=[3, 3, 3, 3, 3, 3, 4, 4, 3, 0, 4, 4, 4], count=[3, 2, 5, 1, 9, 7, 8, 7, 10, 2, 2, 3, 9], votes=[2, 2, 3, 1, 8, 4, 5, 2, 3, 2, 1, 3, 5])
    return a, b, torch.tensor([0, 3, 4]), want


def chain():
    """Case 21: three windows along z; the instance on the column (3, 4, .) is id 2 in the first, 7 in the second, 1 in the third, and the third
    window overlaps only the second.  Each window also has an instance of its own."""
    w1 = make_map(*_cat((line(0, 10), 2), (line(0, 4, x=9), 5)))
    w2 = make_map(*_cat((line(6, 10), 7), (line(8, 4, x=12), 2)))
    w3 = make_map(*_cat((line(12, 10), 1), (line(14, 3, x=15), 7)))
    return [w1, w2, w3]


# ----------------------------------------------------------------------------------------------- the definitions once more, over dicts and sets
def brute_table(a, b):
    """-> (ids_a, ids_b, {(id_a, id_b): shared voxels}) from a dict of a's voxels."""
    row_a = {tuple(v): int(i) for v, i in zip(a["voxels"].tolist(), a["instances"].tolist())}
    shared = {}
    for v, i in zip(b["voxels"].tolist(), b["instances"].tolist()):
        if tuple(v) in row_a:
            shared[(row_a[tuple(v)], int(i))] = shared.get((row_a[tuple(v)], int(i)), 0) + 1
    return sorted(set(a["instances"].tolist())), sorted(set(b["instances"].tolist())), shared


def brute_iou(ids_a, ids_b, shared):
    r = {i: sum(n for (x, _), n in shared.items() if x == i) for i in ids_a}
    c = {j: sum(n for (_, y), n in shared.items() if y == j) for j in ids_b}
    return {(i, j): (np.float32(shared.get((i, j), 0)) / np.float32(r[i] + c[j] - shared.get((i, j), 0)) if r[i] + c[j] else np.float32(0.0))
            for i in ids_a for j in ids_b}


def brute_best_cost(ids_a, ids_b, shared, iou, ignore):
    """The least total cost of a full assignment of the active ids (exhaustive; float64 sums of the fp32 costs), None when nothing is active."""
    act_a = [i for i in ids_a if i not in ignore and any(n > 0 and x == i and y not in ignore for (x, y), n in shared.items())]
    act_b = [j for j in ids_b if j not in ignore and any(n > 0 and y == j and x not in ignore for (x, y), n in shared.items())]
    if not act_a or not act_b or max(len(act_a), len(act_b)) > 6:                          # 6! orders at the most
        return None, act_a, act_b
    small, large, flip = (act_a, act_b, False) if len(act_a) <= len(act_b) else (act_b, act_a, True)
    cost = lambda s, l: float(np.float32(1.0) - (iou[(l, s)] if flip else iou[(s, l)]))     # noqa: E731
    return min(sum(cost(s, l) for s, l in zip(small, chosen)) for chosen in itertools.permutations(large, len(small))), act_a, act_b


def brute_merge(a, b, new_id):
    """The merged rows as a list of dicts in key order; new_id: b's id -> its id in a's numbering.  fp32 scalar arithmetic in the definition's order."""
    f = np.float32
    colored = "color" in a and "color" in b

    def rows(m, relabel):
        out = {}
        for r, v in enumerate(m["voxels"].tolist()):
            i = int(m["instances"][r])
            out[tuple(v)] = dict(id=relabel(i), count=int(m["count"][r]), agreement=m["agreement"][r].numpy(), points=m["points"][r].numpy(),
                                 color=m["color"][r].numpy() if colored else None)
        return out
    ra, rb = rows(a, lambda i: i), rows(b, lambda i: new_id[i])
    merged = []
    for v in sorted(set(ra) | set(rb), key=lambda v: (v[0], v[1], v[2])):
        if v in ra and v in rb:
            x, y = ra[v], rb[v]
            ca, cb, cn = f(x["count"]), f(y["count"]), f(x["count"] + y["count"])
            va, vb = int(np.rint(f(x["agreement"]) * ca)), int(np.rint(f(y["agreement"]) * cb))
            if x["id"] == y["id"]:
                idw, votes = x["id"], va + vb
            elif va > vb or (va == vb and x["id"] < y["id"]):
                idw, votes = x["id"], va
            else:
                idw, votes = y["id"], vb
            mix = lambda k: np.array([(f(x[k][c]) * ca + f(y[k][c]) * cb) / cn for c in range(3)], np.float32)      # noqa: E731
            merged.append(dict(voxel=v, id=idw, count=x["count"] + y["count"], agreement=f(votes) / cn, points=mix("points"),
                               color=mix("color") if colored else None))
        else:
            merged.append(dict(ra[v] if v in ra else rb[v], voxel=v))
    return merged


def assert_rows(got, rows, what=""):
    """A merged map against brute_merge's rows: integers equal, floats bit for bit."""
    n = len(rows)
    assert got["instances"].numel() == n and got["instances"].dtype == torch.int64 and got["count"].dtype == torch.int32, what
    assert got["voxels"].tolist() == [list(r["voxel"]) for r in rows] and got["voxels"].dtype == torch.int32, what
    assert got["instances"].tolist() == [r["id"] for r in rows], (what, got["instances"].tolist(), [r["id"] for r in rows])
    assert got["count"].tolist() == [r["count"] for r in rows], what
    bits = lambda x: np.asarray(x, np.float32).reshape(-1).view(np.int32).tolist()         # noqa: E731
    assert bits(got["agreement"]) == bits([r["agreement"] for r in rows]), what
    assert bits(got["points"]) == bits([r["points"] for r in rows]), what
    if n:
        assert ("color" in got) == (rows[0]["color"] is not None), what
    if n and rows[0]["color"] is not None:
        assert bits(got["color"]) == bits([r["color"] for r in rows]), what


RESULT_KEYS = ("ids_a", "ids_b", "table", "iou", "pairs", "mapping")
MERGED_KEYS = ("points", "color", "instances", "count", "agreement", "voxels", "component", "origin")
