"""The decoder launch rules of csrc/mlp.hip as a table: the answers of the host-only entry points

    pag_mlp_fwd_pair_supported   pag_mlp_fwd_producer_supported   pag_mlp_fwd_composite_supported
    pag_mlp_bwd_fused_supported  pag_mlp_bwd_pair_supported       pag_mlp_bwd_fused_workspace_bytes

on the shipped decoder shapes and on every one-field and two-field change of them (tests/test_abi_and_host.py compares the library with the
recorded table, tests/golden/mlp_launch_rules.json).  The enumeration is deterministic: per rule and base case the unchanged arguments, then
the single changes in the order of the value lists below, then the pairs of changes to two different fields in the same order.  The workspace
bytes take M from BYTES_M and, per M, the unchanged arguments and every single change (M is the second changed "field").

Recording (from a library built from the commit BEFORE a change of the rules, never from the code under test):

    python tests/mlp_launch_rules.py --lib OTHER_TREE/pagnerf_amd/lib/libpagnerf_hip.so --source OTHER_TREE/pagnerf_amd/csrc/mlp.hip \
        --commit $(git -C OTHER_TREE rev-parse HEAD)

writes the fixture with that commit's id and the sha256 of its host layer, after checking that every base case answers 1 unchanged and that every field
of the lists flips at least one answer.  No pointer in these structs is followed by the rules except pair / x1_producer, which point at
real structs; all others are made-up addresses.
"""
import ctypes
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from pagnerf_amd import _lib as L      # noqa: E402  (the structs and signatures; nothing is loaded or built)

FIXTURE = os.path.join(HERE, "golden", "mlp_launch_rules.json")
MAX_M = L.MLP_FUSED_WIDE_MAX_M
BYTES_M = [1, 31, 32, 33, 4097, MAX_M]
A0, A1 = 0x10000, 0x20000      # two made-up addresses: "this tensor" and "another tensor"
DTYPES, ACTS, MODES, LAYOUTS = [L.F32, L.F16, L.BF16], [L.ACT_NONE, L.ACT_SIGMOID, L.ACT_SOFTMAX], [L.MLP_MFMA_BF16, L.MLP_FP32], [L.LAYOUT_STRIDED, L.LAYOUT_XCD8]
OUT_DIMS = [4, 5, 8, 9, 16, 32, 33, 192, 193, 224, 225]
GRIDS = [(24, 2), (7, 8), (8, 8), (32, 2)]      # (x1_levels, x1_feats): 7 x 8 leaves staged position 63 free, 8 x 8 and 32 x 2 do not
PTR = [None, A0, A1]

# field -> values, on both sides of every constant the rules compare it with and through its other states
FWD_VALUES = {
    "x1": PTR, "x1_dtype": DTYPES, "k1": [16, 64], "x1_layout": LAYOUTS, "grid": GRIDS, "x2": PTR[:2], "k2p": [0, 16, 32], "x2_index": PTR[:2],
    "in_dim": [48, 49], "n_layers": [2, 3], "out_dim": OUT_DIMS + [0], "W0": PTR[:2], "W1": PTR[:2], "b0": PTR[:2], "b1": PTR[:2], "out_act": ACTS,
    "out": PTR, "out_dtype": DTYPES, "hidden_save0": PTR[:2], "hidden_save1": PTR[:2], "mode": MODES, "softmax_stats": PTR[:2],
    "x1_col0_relu": PTR[:2], "pair": ["null", "other"], "composite": ["null", "other"], "x1_producer": ["null", "other"],
}
BWD_VALUES = {
    "grad_out": PTR[:2], "out": PTR[:2], "out_dtype": DTYPES, "out_act": ACTS, "k1": [16, 64], "in_dim": [48, 49], "n_layers": [2, 3, 4],
    "out_dim": OUT_DIMS + [0], "x1_layout": LAYOUTS, "grid": GRIDS + [(0, 2), (24, 0)], "dx1": PTR, "dx1_dtype": DTYPES, "mode": MODES, "g_ray": PTR[:2],
    "g_scale": PTR[:2], "g_index": PTR[:2], "softmax_stats": PTR[:2], "b_last": PTR[:2], "dx1_accumulate": [0, 1], "dx1_col0_add": PTR[:2],
    "dx1_col0_gate": PTR[:2], "g_ray_scale": PTR[:2], "x1": PTR, "x1_dtype": DTYPES, "x2": PTR[:2], "k2p": [0, 16, 32], "x2_index": PTR[:2],
}
M_VALUES = [0, 1, MAX_M, MAX_M + 1]


def _set(s, field, value, keep):
    """One change of struct `s`; `keep` holds the structs that pointer fields point at."""
    if field == "grid":
        s.x1_levels, s.x1_feats = value
    elif field[:-1] in ("W", "b", "hidden_save"):
        getattr(s, field[:-1])[int(field[-1])] = value
    elif field in ("pair", "x1_producer"):
        setattr(s, field, None if value == "null" else ctypes.pointer(keep.setdefault("other" + type(s).__name__, type(s)())))
    elif field == "composite":
        s.composite = None if value == "null" else ctypes.pointer(keep.setdefault("comp", L.HeadCompositeArgs()))
    else:
        setattr(s, field, value)


def _make(cls, keep, **fields):
    s = cls()
    for k, v in fields.items():
        _set(s, k, v, keep)
    return s


def fwd_bases(keep):
    """The shipped forward argument blocks (pagnerf_amd/ops.py fills them so): name -> struct."""
    xcd = dict(x1=A0, x1_dtype=L.BF16, k1=64, x1_layout=L.LAYOUT_XCD8, grid=(24, 2), in_dim=48, mode=L.MLP_MFMA_BF16, W0=A0, W1=A0, b0=A0, b1=A0)
    f = lambda **kw: _make(L.MlpFwdArgs, keep, **kw)
    return {
        "density": f(**xcd, n_layers=2, out_dim=16, out_act=L.ACT_NONE, out=A1, out_dtype=L.BF16),
        "colour": f(x1=A1, x1_dtype=L.BF16, k1=16, x2=A0, k2p=32, x2_index=A0, in_dim=43, n_layers=3, out_dim=3, W0=A0, W1=A0, W2=A0, b0=A0, b1=A0, b2=A0,
                    out_act=L.ACT_SIGMOID, out=A0, out_dtype=L.F32, mode=L.MLP_MFMA_BF16, x1_col0_relu=A0),
        "semantic": f(**xcd, n_layers=2, out_dim=6, out_act=L.ACT_SOFTMAX, out=A0, out_dtype=L.BF16),
        "instance": f(**xcd, W2=A0, b2=A0, n_layers=3, out_dim=200, out_act=L.ACT_SOFTMAX, out_dtype=L.BF16, hidden_save1=A0, softmax_stats=A0),
    }


def bwd_bases(keep):
    """The shipped backward argument blocks, and the accepted shapes of test_forward_time_fused_backward_decision: name -> struct."""
    xcd = dict(x1=A0, x1_dtype=L.BF16, dx1=A0, dx1_dtype=L.BF16, k1=64, x1_layout=L.LAYOUT_XCD8, grid=(24, 2), in_dim=48, mode=L.MLP_MFMA_BF16)
    rank1 = dict(g_ray=A0, g_scale=A0, g_index=A0, g_ray_scale=A0)
    f = lambda **kw: _make(L.MlpBwdArgs, keep, **kw)
    return {
        "density": f(**xcd, n_layers=2, out_dim=16, out_act=L.ACT_NONE, out_dtype=L.BF16, grad_out=A0, out=A0),
        "density 7x8": f(**dict(xcd, grid=(7, 8), in_dim=56), n_layers=2, out_dim=16, out_act=L.ACT_NONE, out_dtype=L.BF16, grad_out=A0, out=A0),
        "colour": f(x1=A0, x1_dtype=L.BF16, dx1=A0, dx1_dtype=L.BF16, k1=16, x2=A0, k2p=32, x2_index=A0, in_dim=43, n_layers=3, out_dim=3, out_act=L.ACT_SIGMOID,
                    out_dtype=L.F32, grad_out=A0, out=A0, mode=L.MLP_MFMA_BF16, dx1_col0_add=A0, dx1_col0_gate=A0),
        "semantic": f(**xcd, **rank1, n_layers=2, out_dim=6, out_act=L.ACT_SOFTMAX, out_dtype=L.BF16, out=A0, dx1_accumulate=1),
        "semantic, three layers": f(**xcd, **rank1, n_layers=3, out_dim=6, out_act=L.ACT_SOFTMAX, out_dtype=L.BF16, out=A0),
        "instance": f(**xcd, **rank1, n_layers=3, out_dim=200, out_act=L.ACT_SOFTMAX, out_dtype=L.BF16, softmax_stats=A0, b_last=A0),
        "instance 224": f(**xcd, **rank1, n_layers=3, out_dim=224, out_act=L.ACT_SOFTMAX, out_dtype=L.BF16, softmax_stats=A0, b_last=A0),
    }


def rules(lib):
    """(rule name, [(base name, {role: struct}, M or None)], call(structs, M) -> int, {role: value table})."""
    keep = {}
    fw, bw = fwd_bases(keep), bwd_bases(keep)
    ref = ctypes.byref
    inst_pair = _copy(fw["instance"])
    inst_pair.pair = ctypes.pointer(keep.setdefault("sem", _copy(fw["semantic"])))
    colour_prod = _copy(fw["colour"])      # ops.py hands the colour decoder the density decoder's `out` as x1
    out = [
        ("fwd_pair", [("instance + semantic", {"a": fw["instance"], "b": fw["semantic"]}, None)],
         lambda s, M: lib.pag_mlp_fwd_pair_supported(ref(s["a"]), ref(s["b"])), {"a": FWD_VALUES, "b": FWD_VALUES}),
        ("fwd_producer", [("colour + density", {"a": colour_prod, "d": fw["density"]}, 1000)],
         lambda s, M: lib.pag_mlp_fwd_producer_supported(ref(s["a"]), ref(s["d"]), M), {"a": FWD_VALUES, "d": FWD_VALUES}),
        ("fwd_composite", [("instance", {"a": fw["instance"]}, 1000), ("instance + semantic", {"a": inst_pair, "a.pair": keep["sem"]}, 1000)],
         lambda s, M: lib.pag_mlp_fwd_composite_supported(ref(s["a"]), M), {"a": FWD_VALUES, "a.pair": FWD_VALUES}),
        ("bwd_fused", [(n, {"a": s}, None) for n, s in bw.items()], lambda s, M: lib.pag_mlp_bwd_fused_supported(ref(s["a"])), {"a": BWD_VALUES}),
        ("bwd_pair", [("instance + semantic", {"a": bw["instance"], "b": bw["semantic"]}, None)],
         lambda s, M: lib.pag_mlp_bwd_pair_supported(ref(s["a"]), ref(s["b"])), {"a": BWD_VALUES, "b": BWD_VALUES}),
    ]
    return out, keep, bw


def _copy(s):
    return type(s).from_buffer_copy(s)


def _changes(structs, tables, with_m):
    ch = [(role, f, v) for role in structs for f, vals in tables[role].items() for v in vals]
    return ch + ([("M", "M", m) for m in M_VALUES] if with_m else [])


def _apply(structs, M, changes, keep):
    """Copies of the base structs with `changes` applied; a struct that another points at (role "a.pair") is re-linked to its copy."""
    s = {role: _copy(b) for role, b in structs.items()}
    if "a.pair" in s:
        s["a"].pair = ctypes.pointer(s["a.pair"])
    for role, f, v in changes:
        if role == "M":
            M = v
        else:
            _set(s[role], f, v, keep)
    return s, M


def sweep(lib):
    """-> (bits, byte counts, flips): the answers in enumeration order, and per (direction, field) whether a change of it changed an answer."""
    table, keep, bw = rules(lib)
    bits, flips, base_answers = [], {}, []
    for name, bases, call, values in table:
        for base_name, structs, M in bases:
            changes = _changes(structs, values, M is not None)
            s, m = _apply(structs, M, [], keep)
            base = call(s, m)
            base_answers.append((name, base_name, base))
            bits.append(base)
            single = []
            for c in changes:
                s, m = _apply(structs, M, [c], keep)
                single.append(call(s, m))
                flips[(name[:3], c[1])] = flips.get((name[:3], c[1]), False) or single[-1] != base
            bits += single
            for (i, c), (j, d) in itertools.combinations(enumerate(changes), 2):
                if c[:2] == d[:2]:
                    continue
                s, m = _apply(structs, M, [c, d], keep)
                bits.append(call(s, m))
                for k, other in ((c, single[j]), (d, single[i])):      # the pair against the single change without k
                    flips[(name[:3], k[1])] = flips[(name[:3], k[1])] or bits[-1] != other
    nbytes = []
    for base_name, b in bw.items():
        for M in BYTES_M:
            for ch in [[]] + [[c] for c in _changes({"a": b}, {"a": BWD_VALUES}, False)]:
                s, _ = _apply({"a": b}, None, ch, keep)
                nbytes.append(lib.pag_mlp_bwd_fused_workspace_bytes(ctypes.byref(s["a"]), M))
    assert all(b in (0, 1) for b in bits)
    return bits, nbytes, flips, base_answers


def to_hex(bits):
    return "%0*x" % ((len(bits) + 3) // 4, int("".join(map(str, bits)) + "0" * (-len(bits) % 4), 2))


def host_layer_sha(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def open_lib(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in L._SIGS.items():
        if name.startswith("pag_mlp_"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="record tests/golden/mlp_launch_rules.json from another tree's library")
    ap.add_argument("--lib", required=True)
    ap.add_argument("--source", required=True, help="that tree's pagnerf_amd/csrc/mlp.hip (its hash names where the table came from)")
    ap.add_argument("--commit", required=True, help="the full id of the commit that tree is a checkout of")
    a = ap.parse_args()
    assert len(a.commit) == 40 and set(a.commit) <= set("0123456789abcdef"), "--commit takes the full 40-digit id"
    bits, nbytes, flips, base_answers = sweep(open_lib(a.lib))
    bad = [b for b in base_answers if b[2] != 1]
    assert not bad, "base cases that do not answer 1: %r" % bad
    dead = sorted(k for k, v in flips.items() if not v)
    assert not dead, "fields whose changes flip no answer: %r" % dead
    assert any(nbytes) and 0 in nbytes
    with open(FIXTURE, "w") as fh:
        json.dump({"recorded_from_commit": a.commit, "recorded_from_mlp_hip_sha256": host_layer_sha(a.source), "n_bits": len(bits), "bits": to_hex(bits), "bytes": nbytes}, fh)
        fh.write("\n")
    print("recorded %d answers (%d ones), %d byte counts (%d nonzero)" % (len(bits), sum(bits), len(nbytes), sum(1 for b in nbytes if b)))
