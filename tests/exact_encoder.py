"""Grid-encoder problems whose arithmetic is exact, shared by tests/test_exact_encoder_host.py and tests/test_gpu_exact_encoders.py.

Construction.  In three dimensions every permutohedral barycentric weight is a difference of elevated coordinates divided by 4, and a hash-grid weight is
(x - vmin) / cell.  With power-of-two scale factors / resolutions, shifts in eighths and dyadic positions every weight is a short dyadic number; with
small-integer upstream gradients, integer tables and power-of-two feature scales every product and every partial sum of csrc/encode.hip is exact in f32, in
the 18-bit mantissa of a packed workspace entry, in the fixed-point accumulator and in an f32 atomic.  The forward, the table gradient and the position
gradient must then EQUAL an fp64 reference element by element, whatever the order of the sums.

problem() builds a problem, levels() its vertices and fp64 weights (vertices from oracle.permuto_encode / oracle.hash_encode, which the forward kernels match
bit for bit), reference() evaluates everything in fp64, check_exact() proves conditions (a)-(e) for one problem (it raises otherwise), bin_model() restates
the branches of the binned table gradient on the CPU, and assert_bit_equal() is torch.equal with a message that names the level, slice and rows at fault.

Conditions, per level, with the lines of csrc/encode.hip they come from (term = g * feat_scale * w, one per (sample, vertex, feature)):
 (a) every weight, recomputed in fp64, equals the oracle's f32 weight, and every term has at most 24 significant bits - at most 18 when F = 2, where a bf16
     gradient takes the packed entry: `pack_entry` keeps `(a & ~63u)` of `__float_as_uint(v) + 0x20u`, an fp32 with the low 6 mantissa bits rounded away.
 (b) all terms of the level are multiples of one quantum q = 2^k and, for every table row, sum |term| < 2^18 * q.  Then every partial sum, in any order, has
     at most 18 significant bits: exact in `run_combine` (f32 adds over a wave's run), in the packed word, and in `atomicAdd(tab + idx * F + f, gv[f] * w)`.
 (c) q >= 2^(ex - 24) with 2^(ex - 1) <= max |g * feat_scale| < 2^ex over the level: `to_fixed<true>` is `__float2int_rn(ldexpf(v, S - 14)) << 14` with
     `S = 38 - ex` from `frexpf(maxabs, &ex)` in reduce_kernel, so a packed value is added exactly only as a multiple of 2^(ex - 24).
 (d) held table + gradient is exact in f32: `dst[j] = overwrite ? v : dst[j] + v`.
 (e) the forward output and the position gradient are exact in f32: every f32 intermediate of the kernels' formulas, restated here in f32, equals its fp64
     value, and every sum over levels, XCD groups and a ray's samples stays below 2^24 quanta.  A bf16 output is the one correctly rounded cast of that
     exact f32 value (`store_grouped`: `(bf16_t)v`, then `(bf16_t)((float)a[e] + (float)o[e])` with an addend); the reference rounds its fp64 value alike."""
import types

import numpy as np
import torch

from exact_decoder import from_xcd8, to_xcd8          # noqa: F401  (the XCD8 staging of a [M, L*F] tensor, shared with the decoder problems)
from oracle import hash_encode as HE
from oracle import permuto_encode as PE

TS = {"permuto": 1024, "hash": 512}          # tile_samples(): samples per bin_kernel workgroup
NV = {"permuto": 4, "hash": 8}
SLICE_SHIFT, NS_MAX, DISTINCT_SEG, RED_HEAD, REDUCE_WAVES = 13, 256, 12, 8, 16
PERIOD = 512                                 # the positions repeat their STRUCTURE (not their values) every 8 waves
ZERO_WAVE = (7, 2)                           # upstream gradient: waves with index % 7 == 2 are zero, ...
ZERO_TILE = 1                                # ... so is tile 1 (of TS[kind] samples) ...
#                                              ... and level L - 2 (L >= 3)


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def bin_plan(M, F, kind, rows):
    """bin_plan() of csrc/encode.hip restated: slice shift, slices per level, tiles, rows of the last slice."""
    shift = SLICE_SHIFT
    while shift > 0 and (1 << shift) * F * 8 > 65536:
        shift -= 1
    NS = (rows + (1 << shift) - 1) >> shift
    assert NS <= NS_MAX
    return types.SimpleNamespace(shift=shift, NS=NS, ntiles=(M + TS[kind] - 1) // TS[kind], last_rows=rows - ((NS - 1) << shift), TS=TS[kind])


def _segments():
    """One period of 512 samples = 8 waves as (first, length, kind) with kind 'ray' (consecutive samples a small step apart), 'same' (one point repeated),
    'special' (lattice vertices, cell faces, +-1) or 'scatter' (every sample on its own)."""
    rays = [(3, 9, "ray"), (14, 5, "ray"), (28, 9, "ray"), (44, 16, "ray"),          # wave 0: inside a 16-lane row; across lanes 16, 32 and 48
            (64, 85, "ray"),                                                         # wave 1 filled, continued into 21 lanes of wave 2
            (256, 7, "same"), (272, 3, "ray"),                                       # wave 4: 6 + 2 repeats and nothing else: the early return with runs
            (320, 24, "special"),                                                    # wave 5
            (384, 128, "ray")]                                                       # waves 6, 7: one ray across the wave boundary; wave 3 is all scatter
    segs, at = [], 0
    for first, n, kind in rays:
        segs += [(i, 1, "scatter") for i in range(at, first)]
        segs.append((first, n, kind))
        at = first + n
    segs += [(i, 1, "scatter") for i in range(at, PERIOD)]
    return segs


_SEGS = _segments()
_STEPS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (-1, 0, 1), (1, -1, 1), (2, 1, 0), (0, -1, -2)])


def positions(M, start_bits, step_bits, special, seed):
    """f32 [M,3] dyadic positions in [-1,1]: segment starts are multiples of 2^-start_bits, ray steps multiples of 2^-step_bits (>= start_bits <= 10: exact
    in fp16); a ray that reaches +-1 is reflected.  `special`: [n,3] points in units of 2^-step_bits placed in wave 5 of every period."""
    rs = np.random.RandomState(seed)
    seg_of = np.concatenate([np.full(n, s) for s, (_, n, _) in enumerate(_SEGS)])
    first = np.array([f for f, _, _ in _SEGS])
    is_ray = np.array([k == "ray" for _, _, k in _SEGS])
    periods = (M + PERIOD - 1) // PERIOD
    N, unit = 1 << step_bits, 1 << (step_bits - start_bits)
    start = rs.randint(-(N // unit), N // unit + 1, size=(periods, len(_SEGS), 3)) * unit
    step = _STEPS[rs.randint(0, len(_STEPS), size=(periods, len(_SEGS)))] * is_ray[None, :, None]
    i = np.arange(M)
    per, lane = i // PERIOD, i % PERIOD
    s = seg_of[lane]
    n = start[per, s] + step[per, s] * (lane - first[s])[:, None]
    n = (n + N) % (4 * N)                         # reflect into [-N, N]
    n = np.where(n > 2 * N, 4 * N - n, n) - N
    sp = np.flatnonzero(np.array([k == "special" for _, _, k in _SEGS])[s])
    sp = sp[per[sp] < SPECIAL_PERIODS]
    if len(sp) and len(special):
        n[sp] = np.asarray(special)[(lane[sp] - first[s[sp]] + per[sp]) % len(special)]
    assert np.abs(n).max() <= N and step_bits <= 10
    return (n / float(N)).astype(np.float32)


def _permuto_levels(L, seed, lo, hi):
    """Per-axis scale factors 2^lo .. 2^hi, different on every level and axis, and shifts in eighths."""
    rs = np.random.RandomState(seed)
    base = np.round(np.linspace(lo, hi, L)) if L > 1 else np.array([2.0])
    ex = np.array([[np.clip(base[l] + (l + a) % 3 - 1, lo, hi) for a in range(3)] for l in range(L)])
    return (2.0 ** ex).astype(np.float32), (rs.randint(-8, 9, size=(L, 3)) / 8.0).astype(np.float32)


HASH_OCTAVES = {"hash": ((16, 32, 64), 6), "hash_lo": ((2, 4, 8), 3), "hash_big": ((64,), 7)}          # resolutions, position bits: weights in 8ths .. halves (big: quarters)
PERMUTO_SCALES = {"permuto": (0, 4, 4, 6), "permuto_coarse": (0, 3, 2, 3)}          # scale factors 2^lo .. 2^hi; segment starts / ray steps in 2^-bits
SPECIAL_PERIODS = 8          # the special points are placed in the first periods only: at M = 2^19 they would be the one row everything lands on


def problem(kind, L, F, rows, M, seed=11, feat_scale=False, held=False, zero_level=True):
    """kind: 'permuto' (scale factors 1 .. 16, positions in 64ths), 'permuto_coarse' (1 .. 8, positions in 8ths: hot rows stay exact at a large M),
    'hash' (resolutions 16, 32, 64 repeated over the levels, positions in 64ths), 'hash_lo' (2, 4, 8, positions in 8ths) or 'hash_big' (64, positions in
    128ths).  rows: permutohedral capacity, or 2^log2_T.
    -> namespace: xyz f32 [M,3], tables f64 [L,rows,F] (integers), g f64 [M,L*F] (integers), scale f64 [L*F] (powers of two, or None), held f64 or None."""
    key = (kind, L, F, rows, M, seed, feat_scale, held, zero_level)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    p = types.SimpleNamespace(kind=kind, enc="permuto" if kind in PERMUTO_SCALES else "hash", L=L, F=F, rows=rows, M=M, seed=seed)
    rs = np.random.RandomState(seed + 1000 * L + F)
    if p.enc == "permuto":
        lo, hi, start_bits, step_bits = PERMUTO_SCALES[kind]
        p.sf, p.shift = _permuto_levels(L, seed, lo, hi)
        N = 1 << step_bits
        special = [(0, 0, 0), (N, N, N), (-N, -N, -N), (N, -N, 0), (N // 2, 0, -N // 2), (N // 8, N // 8, N // 8), (-N // 4, 3 * N // 8, 5 * N // 8)]
        special += [tuple(np.clip(-p.shift[l] * N, -N, N).astype(int)) for l in range(min(L, 6))]          # cf = 0 on level l: a lattice vertex
        p.xyz = positions(M, start_bits, step_bits, special, seed)
    else:
        res, bits = HASH_OCTAVES[kind]
        p.res = [float(res[l % len(res)]) for l in range(L)]
        assert rows & (rows - 1) == 0
        p.log2_T = rows.bit_length() - 1
        N = 1 << bits
        special = [(0, 0, 0), (N, N, N), (-N, -N, -N), (N, -N, 0), (N // 2, 0, -N // 2), (N // 4, N // 4, 1), (-N // 8, 3 * N // 8, N - 1), (N - 1, 1 - N, 1)]
        p.xyz = positions(M, bits, bits, special, seed)
    p.tables = rs.randint(-4, 5, size=(L, rows, F)).astype(np.float64)
    g = rs.randint(-2, 3, size=(M, L * F)).astype(np.float64)
    wave = np.arange(M) // 64
    g[wave % ZERO_WAVE[0] == ZERO_WAVE[1]] = 0
    g[ZERO_TILE * TS[p.enc]:(ZERO_TILE + 1) * TS[p.enc]] = 0
    p.zero_level = L - 2 if (zero_level and L >= 3) else None
    if p.zero_level is not None:
        g[:, p.zero_level * F:(p.zero_level + 1) * F] = 0
    p.g = g
    p.scale = 2.0 ** rs.randint(-2, 3, size=L * F).astype(np.float64) if feat_scale else None
    p.held = rs.randint(-8, 9, size=(L, rows, F)).astype(np.float64) if held else None
    p.plan = bin_plan(M, F, p.enc, rows)
    p.packed = F == 2                              # a bf16 gradient takes the 8-byte packed entries
    _PROBLEMS[key] = p
    return p


_PROBLEMS = {}


def rays_for(M, seed=5):
    """Samples sorted by ray, one pack per ray: lengths 1 .. 300 in a fixed cycle -> (ridx i32 [M], depths f32 [M] in quarters, pack_start i64 [N+1])."""
    lens, cycle, left = [], (1, 5, 64, 100, 17, 300, 63, 130), M
    while left > 0:
        lens.append(min(cycle[len(lens) % len(cycle)], left))
        left -= lens[-1]
    pack_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ridx = np.repeat(np.arange(len(lens)), lens).astype(np.int32)
    depths = (np.random.RandomState(seed).randint(1, 17, size=M) / 4.0).astype(np.float32)
    return ridx, depths, pack_start


# ------------------------------------------------------------------------------------------------- vertices, fp64 weights, reference
def levels(p):
    """Per level: idx int64 [M,NV], w f64 [M,NV] (the fp64 weights - check_exact proves them equal to the oracle's f32 ones), w32 f32 [M,NV], and what the
    position gradient needs (permuto: slot [M,4]; hash: w3 f64 [M,3], dw f64 [3])."""
    if hasattr(p, "_levels"):
        return p._levels
    out = []
    x64 = p.xyz.astype(np.float64)
    rows_i = np.arange(p.M)
    for l in range(p.L):
        if p.enc == "permuto":
            rem0, rank, bary = PE.lattice_simplex(p.xyz, p.shift[l], p.sf[l])
            idx = PE.vertex_indices(rem0, rank, p.rows).astype(np.int64)
            cf = (x64 + p.shift[l].astype(np.float64)) * p.sf[l].astype(np.float64)
            E = np.stack([cf[:, 0] + cf[:, 1] + cf[:, 2], cf[:, 2] + cf[:, 1] - cf[:, 0], cf[:, 2] - 2 * cf[:, 1], -3 * cf[:, 2]], 1)
            b5 = np.zeros((p.M, 5))
            for a in range(4):
                delta = (E[:, a] - rem0[:, a]) * 0.25
                b5[rows_i, 3 - rank[:, a]] += delta
                b5[rows_i, 4 - rank[:, a]] -= delta
            b5[:, 0] += 1.0 + b5[:, 4]
            out.append(types.SimpleNamespace(idx=idx, w=b5[:, :4].copy(), w32=bary, slot=(3 - rank).astype(np.int64)))
        else:
            xt = torch.from_numpy(p.xyz)
            vmin, vmax, idx = HE.hash_level_indices(xt, p.res[l], p.log2_T)
            w3_32 = ((xt - vmin) / (vmax - vmin)).numpy()
            vmin64, vmax64 = vmin.double().numpy(), vmax.double().numpy()
            w3 = (x64 - vmin64) / (vmax64 - vmin64)
            w, w32 = np.empty((p.M, 8)), np.empty((p.M, 8), dtype=np.float32)
            one = np.float32(1.0)
            for k, (i, j, kk) in enumerate(HE.CORNERS):
                w[:, k] = (w3[:, 0] if i else 1 - w3[:, 0]) * (w3[:, 1] if j else 1 - w3[:, 1]) * (w3[:, 2] if kk else 1 - w3[:, 2])
                w32[:, k] = ((w3_32[:, 0] if i else one - w3_32[:, 0]) * (w3_32[:, 1] if j else one - w3_32[:, 1])).astype(np.float32) * \
                    (w3_32[:, 2] if kk else one - w3_32[:, 2])
            out.append(types.SimpleNamespace(idx=idx.astype(np.int64), w=w, w32=w32, w3=w3, dw=p.res[l] / 2.0))
    p._levels = out
    return out


def _scaled_g(p, dtype=np.float64):
    return (p.g if p.scale is None else p.g * p.scale[None, :]).astype(dtype)


def _xyz_grad_level(p, l, lv, gs, tab, dt):
    """d loss / d xyz of one level by the kernels' closed forms (xyz_grad_sample), in dtype dt."""
    F = p.F
    e = tab[lv.idx].astype(dt)                                   # [M,NV,F]
    g = gs[:, l * F:(l + 1) * F].astype(dt)
    if p.enc == "permuto":
        gb = (e * g[:, None, :]).sum(2, dtype=dt) if F > 1 else (e * g[:, None, :])[:, :, 0]
        gb = np.concatenate([gb, gb[:, :1]], 1)
        r = np.arange(p.M)
        gE = [dt(0.25) * (gb[r, lv.slot[:, a]] - gb[r, lv.slot[:, a] + 1]) for a in range(4)]
        s = p.sf[l].astype(dt)
        return np.stack([(gE[0] - gE[1]) * s[0], (gE[0] + gE[1] - dt(2) * gE[2]) * s[1], (gE[0] + gE[1] + gE[2] - dt(3) * gE[3]) * s[2]], 1)
    w = lv.w3.astype(dt)
    wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
    ox, oy, oz = dt(1) - wx, dt(1) - wy, dt(1) - wz
    c00, c01, c10, c11 = e[:, 0] * ox + e[:, 4] * wx, e[:, 1] * ox + e[:, 5] * wx, e[:, 2] * ox + e[:, 6] * wx, e[:, 3] * ox + e[:, 7] * wx
    c0, c1 = c00 * oy + c10 * wy, c01 * oy + c11 * wy
    gx = (g * (oz * (oy * (e[:, 4] - e[:, 0]) + wy * (e[:, 6] - e[:, 2])) + wz * (oy * (e[:, 5] - e[:, 1]) + wy * (e[:, 7] - e[:, 3])))).sum(1, dtype=dt)
    gy = (g * (oz * (c10 - c00) + wz * (c11 - c01))).sum(1, dtype=dt)
    gz = (g * (c1 - c0)).sum(1, dtype=dt)
    return np.stack([gx, gy, gz], 1) * dt(lv.dw)


def reference(p, rays=None):
    """fp64: out [M,L*F], gtab [L,rows,F], dxyz [M,3] (and dxyz_levels [L,M,3]); with rays = (ridx, depths, pack_start) also drays [N,6]."""
    ref = getattr(p, "_ref", None)
    if ref is None:
        ref = types.SimpleNamespace(out=np.empty((p.M, p.L * p.F)), gtab=np.zeros((p.L, p.rows, p.F)), dxyz_levels=np.zeros((p.L, p.M, 3)))
        gs = _scaled_g(p)
        for l, lv in enumerate(levels(p)):
            for f in range(p.F):
                c = l * p.F + f
                ref.out[:, c] = (lv.w * p.tables[l][lv.idx, f]).sum(1) * (1.0 if p.scale is None else p.scale[c])
                ref.gtab[l, :, f] = np.bincount(lv.idx.ravel(), weights=(lv.w * gs[:, c:c + 1]).ravel(), minlength=p.rows)
            ref.dxyz_levels[l] = _xyz_grad_level(p, l, lv, gs, p.tables[l], np.float64)
        ref.dxyz = ref.dxyz_levels.sum(0)
        p._ref = ref
    if rays is not None:
        ridx, depths, pack_start = rays
        N = len(pack_start) - 1
        ref.drays = np.zeros((N, 6))
        for c in range(3):
            ref.drays[:, c] = np.bincount(ridx, weights=ref.dxyz[:, c], minlength=N)
            ref.drays[:, 3 + c] = np.bincount(ridx, weights=ref.dxyz[:, c] * depths.astype(np.float64), minlength=N)
    return ref


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).double().numpy()


# ------------------------------------------------------------------------------------------------------------------------------- exactness
def sig_bits(a):
    """Significant bits of every element of an fp64 array (0 for 0) and the exponent of its lowest set bit (a large number for 0)."""
    a = np.abs(np.asarray(a, dtype=np.float64)).ravel()
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    tz = np.where(mi == 0, 53, np.frexp(low.astype(np.float64))[1] - 1)
    return np.where(mi == 0, 0, 53 - tz), np.where(mi == 0, 10 ** 6, e - 53 + tz)


def _f32_exact(a):
    return np.array_equal(np.asarray(a, np.float64).astype(np.float32).astype(np.float64), a)


def check_exact(p, rays=None):
    """Conditions (a)-(e) of the module docstring, per level.  -> the figures (max significant bits of weights / terms / gradient rows, row-sum headroom)."""
    def need(ok, what):
        if not ok:
            raise AssertionError("%s L=%d F=%d rows=%d M=%d: %s" % (p.kind, p.L, p.F, p.rows, p.M, what))

    ref = reference(p, rays)
    gs = _scaled_g(p)
    lim = 18 if p.packed else 24
    need(np.array_equal(p.xyz.astype(np.float16).astype(np.float32), p.xyz) and np.abs(p.xyz).max() <= 1.0, "positions not exact in fp16 / outside [-1,1]")
    need(np.array_equal(bf16_round(p.g), p.g), "upstream gradient not exact in bf16")
    fig = types.SimpleNamespace(w_bits=0, term_bits=0, grad_bits=0, row_sum_log2=-99.0)
    for l, lv in enumerate(levels(p)):
        need(np.array_equal(lv.w32.astype(np.float64), lv.w), "(a) level %d: f32 weights differ from fp64" % l)
        need(lv.w.min() >= 0.0 and np.array_equal(lv.w.sum(1), np.ones(p.M)), "(a) level %d: weights are no partition of one" % l)
        g = gs[:, l * p.F:(l + 1) * p.F]
        terms = lv.w[:, :, None] * g[:, None, :]
        bits, low = sig_bits(terms)
        fig.w_bits, fig.term_bits = max(fig.w_bits, int(sig_bits(lv.w)[0].max())), max(fig.term_bits, int(bits.max()))
        need(bits.max() <= lim, "(a) level %d: a term has %d significant bits > %d" % (l, bits.max(), lim))
        if not terms.any():
            continue
        k = int(low.min())
        for f in range(p.F):
            rs_ = np.bincount(lv.idx.ravel(), weights=np.abs(terms[:, :, f]).ravel(), minlength=p.rows).max()
            fig.row_sum_log2 = max(fig.row_sum_log2, float(np.log2(max(rs_, 1e-300))) - k - 18)
            need(rs_ < 2.0 ** (18 + k), "(b) level %d: a row's sum of |term| %g reaches 2^18 quanta of 2^%d" % (l, rs_, k))
        ex = int(np.frexp(np.abs(g).max())[1])
        need(k >= ex - 24, "(c) level %d: quantum 2^%d below to_fixed's 2^%d" % (l, k, ex - 24))
        fig.grad_bits = max(fig.grad_bits, int(sig_bits(ref.gtab[l])[0].max()))
    need(_f32_exact(ref.gtab), "(b) table gradient not exact in f32")
    if p.held is not None:
        need(_f32_exact(p.held + ref.gtab), "(d) held + gradient not exact in f32")
    need(_f32_exact(ref.out), "(e) forward not exact in f32")
    # (e) the kernels' formulas in f32: forward (lerps / weighted sum in the oracle's order), position gradient
    gs32 = _scaled_g(p, np.float32)
    for l, lv in enumerate(levels(p)):
        d32 = _xyz_grad_level(p, l, lv, gs32, p.tables[l].astype(np.float32), np.float32)
        need(d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), ref.dxyz_levels[l]), "(e) level %d: f32 position gradient differs from fp64" % l)
    nz = ref.dxyz_levels[ref.dxyz_levels != 0]
    if nz.size:
        k = int(sig_bits(nz)[1].min())
        need(np.abs(ref.dxyz_levels).sum(0).max() < 2.0 ** (24 + k), "(e) position-gradient sum over the levels reaches 2^24 quanta")
        if rays is not None:
            ridx, depths, _ = rays
            dep = depths.astype(np.float64)
            kd = k + int(sig_bits(dep)[1].min())
            tot = np.abs(ref.dxyz_levels).sum(0) * dep[:, None]
            need(max(np.bincount(ridx, weights=tot[:, c]).max() for c in range(3)) < 2.0 ** (24 + kd), "(e) per-ray sum reaches 2^24 quanta")
            need(_f32_exact(ref.drays), "(e) per-ray gradient not exact in f32")
    need(_f32_exact(ref.dxyz), "(e) position gradient not exact in f32")
    return fig


def f32_reordered_gtab(p, seed):
    """The table gradient accumulated in f32, one addend at a time, in a random order of the (sample, vertex) entries."""
    gs = _scaled_g(p, np.float32)
    out = np.zeros((p.L, p.rows, p.F), dtype=np.float32)
    rs = np.random.RandomState(seed)
    for l, lv in enumerate(levels(p)):
        perm = rs.permutation(lv.idx.size)
        rows = lv.idx.ravel()[perm]
        for f in range(p.F):
            terms = (lv.w32 * gs[:, l * p.F + f:l * p.F + f + 1]).astype(np.float32).ravel()[perm]
            np.add.at(out[l, :, f], rows, terms)
    return out


# ------------------------------------------------------------------------------------------- the branches of the binned table gradient
def bin_model(p, l, grouped=False):
    """bin_kernel / reduce_kernel of csrc/encode.hip restated for level l: which branches the problem's entries take.
    -> repeats [waves, NV] (adjacent-equal vertex ids per wave and vertex slot: run_combine merges from 8), seg [ntiles, NS] (entries per (tile, slice)
    segment after the merge), per (slice, tile group) stream of the reduce pass: distinct flags, chunks on the three-compare path (`fast`: fewer than 4 tile
    boundaries ahead) and on the binary search (`slow`), and `hot`: the largest number of entries of one row that some 64-entry chunk of a non-distinct
    stream must hold whatever the order inside a segment (entries of the row / chunks of the stream, pigeonhole)."""
    plan, lv = p.plan, levels(p)[l]
    M, nv, ts = p.M, NV[p.enc], plan.TS
    i = np.arange(M)
    lane, wave = i % 64, i // 64
    eq = np.zeros((M, nv), dtype=bool)
    eq[1:] = lv.idx[1:] == lv.idx[:-1]
    eq[lane == 0] = False
    repeats = np.zeros((wave[-1] + 1, nv), dtype=np.int64)
    np.add.at(repeats, wave, eq)
    nxt = np.zeros((M, nv), dtype=bool)
    nxt[:-1] = eq[1:]
    emit = ~((repeats[wave] >= 8) & nxt)
    if grouped:          # wave_live: a wave whose gradient pieces are all zero emits nothing (here: all of the sample's columns)
        live = np.zeros(wave[-1] + 1, dtype=bool)
        np.logical_or.at(live, wave, p.g.any(1))
        emit &= live[wave][:, None]
    e_tile = np.broadcast_to((i // ts)[:, None], (M, nv))[emit]
    e_row = lv.idx[emit]
    seg = np.zeros((plan.ntiles, plan.NS), dtype=np.int64)
    np.add.at(seg, (e_tile, e_row >> plan.shift), 1)
    G = int(min(64, max(1, (plan.ntiles + REDUCE_WAVES - 1) // REDUCE_WAVES)))
    res = types.SimpleNamespace(repeats=repeats, seg=seg, G=G, distinct=0, shared=0, fast=0, slow=0, hot=0.0, entries=int(emit.sum()))
    per_group_row = {}
    for key, n in zip(*np.unique((e_tile // G) * p.rows + e_row, return_counts=True)):
        g_, r_ = divmod(int(key), p.rows)
        per_group_row.setdefault((g_, r_ >> plan.shift), []).append(int(n))
    for s in range(plan.NS):
        for t0 in range(0, plan.ntiles, G):
            lens = seg[t0:t0 + G, s]
            total = int(lens.sum())
            if total == 0:
                continue
            distinct = total >= DISTINCT_SEG * len(lens)
            res.distinct += distinct
            res.shared += not distinct
            if not distinct:
                res.hot = max(res.hot, max(per_group_row[(t0 // G, s)]) / float((total + 63) // 64))
            excl = np.full(72, np.iinfo(np.int64).max)
            excl[:64] = total
            excl[:len(lens)] = np.cumsum(lens) - lens
            t = 0
            for c0 in range(0, total, 64):
                i63 = c0 + 63
                if excl[t + 4] >= c0 + 64:
                    res.fast += 1
                    t = t + int(i63 >= excl[t + 1]) + int(i63 >= excl[t + 2]) + int(i63 >= excl[t + 3])
                else:
                    res.slow += 1
                    t = int(np.searchsorted(excl[:64], i63, side="right")) - 1
    return res


# ---------------------------------------------------------------------------------------------------------------------------- comparison
def assert_bit_equal(name, got, want_fp64, shift=None):
    """torch.equal after casting the fp64 reference to the dtype of `got` (NaN equals NaN); the message names the first element and, for a table
    gradient [L,rows,F] (shift given), the levels and slices at fault."""
    got = got.detach().cpu()
    want = torch.from_numpy(np.ascontiguousarray(want_fp64)).to(got.dtype)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (name, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    g, w = got.double(), want.double()
    bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w)))
    if not bool(bad.any()):
        return
    at = torch.nonzero(bad)
    first = tuple(at[0].tolist())
    where = ""
    if shift is not None and bad.dim() == 3:
        where = "; levels %s, slices %s" % (sorted(set(at[:, 0].tolist()))[:32], sorted(set((at[:, 1] >> shift).tolist()))[:32])
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r%s" % (name, int(bad.sum()), bad.numel(), first, float(g[first]), float(w[first]), where))


# ------------------------------------------------------------------------------------------------------------------------------------ cases
# (kind, L, F, rows, M): every problem tests/test_gpu_exact_encoders.py runs; tests/test_exact_encoder_host.py proves each exact.
ROWS = 1 << 15          # F = 2: 8 slices (the XCD-interleaved block order), F = 1: 4, F = 4: 16
SIZES = {kind: (1, TS[enc] - 1, TS[enc], TS[enc] + 1, 3 * TS[enc] + 1) for kind, enc in (("permuto", "permuto"), ("hash", "hash"), ("hash_lo", "hash"))}
M_MAIN = {"permuto": 3 * 1024 + 1, "hash": 3 * 512 + 1}
BIG = ("hash_big", 1, 2, 1 << 20, 512 * 1024 + 1)          # 1025 tiles: a reduce wave walks a second group of 64; 256 slices of ~16 entries per tile
MANY_TILES = ("permuto_coarse", 4, 2, 1 << 20, 66 * 1024 + 1)     # 67 tiles, 256 slices: groups of 5 tiles per reduce wave, short segments, chunks that cross 4 and more tile boundaries
XCD8_LEVELS = (5, 8, 16, 17, 24, 32)
GEOMETRY = {          # (rows, L, F): NS = 1, 4, 8, 16; partial last slice; capacity below one slice; log2_T below the slice shift; RED_HEAD level orders
    "permuto": [(1 << 12, 1, 2), (1 << 14, 2, 2), (1 << 15, 3, 2), (1 << 16, 24, 2), (3 * 4096 + 1000, 3, 2), (3001, 2, 2), (5 * 2048 + 77, 3, 4), (1 << 15, 2, 1)],
    "hash": [(1 << 12, 1, 2), (1 << 14, 2, 2), (1 << 15, 3, 2), (1 << 16, 24, 2), (1 << 10, 3, 2), (1 << 9, 2, 4), (1 << 15, 2, 1)],
}


ENTRY_CASES = [(kind, 6, 2, ROWS, M_MAIN[kind]) for kind in ("permuto", "hash")]          # run with feat_scale and a held table as well


def variants(case):
    return [dict(feat_scale=True, held=True)] if case in ENTRY_CASES else []


def xyz_cases():
    """The cases whose position gradient (per sample and per ray) is compared: their per-ray sums are exact too."""
    cases = [(kind, 6, F, ROWS, M) for kind in ("permuto", "hash") for M in SIZES[kind] for F in (1, 2, 4)]
    return cases + [(kind, L, F, ROWS, M_MAIN[kind]) for kind in ("permuto", "hash") for L, F in ((8, 2), (16, 1))]


def halves(p):
    """The problem cut in two in the middle of its second tile: two problems on the same tables."""
    cut, out = p.plan.TS + p.plan.TS // 2 - 3, []
    for part in (slice(0, cut), slice(cut, p.M)):
        q = types.SimpleNamespace(**{k: v for k, v in vars(p).items() if not k.startswith("_")})
        q.xyz, q.g = p.xyz[part].copy(), p.g[part].copy()
        q.M, q.plan = len(q.xyz), bin_plan(len(q.xyz), p.F, p.enc, p.rows)
        out.append(q)
    return out


def all_cases():
    cases = []
    for kind, sizes in SIZES.items():
        cases += [(kind, 6, F, ROWS, M) for M in sizes for F in (1, 2, 4)]
    for kind in ("permuto", "hash"):
        cases += [(kind, L, F, ROWS, M_MAIN[kind]) for L in XCD8_LEVELS for F in (1, 2, 4) if ((L + 7) // 8) * F <= 8 and L * F <= 64]
        cases += [(kind, L, F, rows, M_MAIN[kind]) for rows, L, F in GEOMETRY[kind]]
    cases += [BIG, MANY_TILES]
    return sorted(set(cases))
