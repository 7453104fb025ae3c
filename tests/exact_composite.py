"""Per-ray problems whose arithmetic is exact, shared by tests/test_exact_composite_host.py and tests/test_gpu_exact_composite.py.

The per-ray kernels of csrc/render.hip sum along a ray's packed samples: in 64-sample chunks with a carried total (composite_fwd / composite_bwd), in four
contiguous wave quarters (the composite_feats_* family), or a lane per sample (the narrow feature kernel, ray_sample_grad).  Three problems make every one
of those sums independent of the order it is taken in:

  transmittance()   every sample is transparent (sigma = 0) or opaque (sigma * delta = 2048): exp(-0) = 1 and exp(-2048 k) = 0 exactly, in f32 and in f64,
                    so the weights are one-hot at a ray's first opaque sample; colours, depths, deltas are dyadic and the upstream gradients small integers;
  features()        weights in {0..8}/8, alpha in {0, 1/4, 1/2, 1}, features and upstream gradients integers in [-2, 2] (exact in bf16);
  ray_samples()     integer gradients on the samples, depths in {0..64}/16.

reference() evaluates a problem in fp64 per ray from the definition (the transmittance gradients by autograd), check_exact() raises unless the claims
above hold for it, f32_*() re-evaluate a reference in f32 one addend at a time, and assert_bit_equal() is torch.equal by value with a message that names
the ray, its pack length, the 64-sample chunk or wave quarter and the column at fault."""
import functools
import types

import numpy as np
import torch

# Pack lengths: around one load group of the narrow kernels (4, 8), half a wave, the 64-sample chunk, the quarters of the 64-wide bf16 kernel (32 rows per
# wave iteration: packs of 124..133 put 31..34 rows in a quarter), four chunks, and two long packs.  Empty packs first, twice inside and (appended) last.
PACKS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 31, 32, 33, 63, 64, 65, 124, 125, 127, 128, 129, 132, 133, 0, 255, 256, 257, 1037, 5000)
EXTRA = (6, 11, 13)          # appended until P % 4 is what the case asks for
FORMS = ("identity", "boundary", "permuted")
PMODS = (0, 1, 3)
SPARE_RAYS = 5               # form "permuted": rays that no pack points to
OPAQUE = 2048.0              # sigma * delta of an opaque sample
LAST = "last"
# first opaque sample by pack length (None: a transparent ray): 0, 1, 62 | 63, 64, 65 and 127 | 128, 129 on either side of the chunk boundaries, the last sample
FIRST = {1: 0, 2: 1, 3: LAST, 4: 0, 5: 1, 7: None, 8: LAST, 9: 0, 31: 1, 32: LAST, 33: None, 63: 62, 64: LAST, 65: LAST, 124: 0, 125: 1, 127: 62, 128: LAST,
         129: 63, 132: 64, 133: 65, 255: 127, 256: 128, 257: 129, 1037: None, 5000: LAST, 6: None, 11: LAST, 13: 0}
UPSTREAM = ("full", "rgb", "depth", "alpha")


def pack_lengths(form, pmod):
    lens = list(PACKS) + [0]
    count = lambda: sum(1 for n in lens if n) if form == "boundary" else len(lens)
    k = 0
    while count() % 4 != pmod:
        lens.insert(len(lens) - 1, EXTRA[k])
        k += 1
    return lens


def _table(form, pmod, seed, scale=1, pad=0):
    """The pack table of one case.  lens: samples per RAY-ORDERED pack (all forms list the empty ones); the table itself (pack_start, ray_of_pack) leaves
    them out in form "boundary".  pad: filler samples behind pack_start[P] (a padded batch)."""
    assert form in FORMS and pmod in PMODS
    lens = np.array(pack_lengths(form, pmod), dtype=np.int64) * scale
    p = types.SimpleNamespace(form=form, pmod=pmod, seed=seed, pad=pad, lens_all=lens)
    starts = np.concatenate([[0], np.cumsum(lens)])
    p.M = int(starts[-1])
    p.rows = p.M + pad
    if form == "identity":
        p.N, p.ray_of_pack, p.pack_start = len(lens), np.arange(len(lens), dtype=np.int32), starts
    elif form == "boundary":
        keep = np.flatnonzero(lens)
        p.N, p.ray_of_pack, p.pack_start = len(lens), keep.astype(np.int32), np.concatenate([starts[keep], [p.M]])
    else:
        p.N = len(lens) + SPARE_RAYS
        p.ray_of_pack, p.pack_start = np.random.RandomState(1000 + seed).permutation(p.N)[:len(lens)].astype(np.int32), starts
    p.P = len(p.ray_of_pack)
    assert p.P % 4 == pmod
    p.lens = np.diff(p.pack_start)
    p.pack_of_sample = np.repeat(np.arange(p.P), p.lens)
    p.ray_of_sample = p.ray_of_pack[p.pack_of_sample].astype(np.int32)
    p.pos = np.arange(p.M) - p.pack_start[p.pack_of_sample]
    p.boundary = p.pos == 0
    p.has_pack = np.zeros(p.N, dtype=bool)
    p.has_pack[p.ray_of_pack] = True
    p.len_of_ray = np.zeros(p.N, dtype=np.int64)
    p.len_of_ray[p.ray_of_pack] = p.lens
    return p


def _padded(p, x):
    """[M, ...] -> [M + pad, ...] with NaN in the filler rows."""
    if not p.pad:
        return x
    return np.concatenate([x, np.full((p.pad,) + x.shape[1:], np.nan)])


# ------------------------------------------------------------------------------------------------------------------------------- transmittance
@functools.lru_cache(maxsize=None)
def transmittance(form, pmod, bg_white=True, seed=0, pad=0):
    p = _table(form, pmod, seed, pad=pad)
    rs = np.random.RandomState(seed)
    p.kind, p.bg_white = "transmittance", bg_white
    p.delta = 2.0 ** -rs.randint(4, 8, size=p.M)
    opaque = np.zeros(p.M, dtype=bool)
    p.first = np.full(p.P, -1, dtype=np.int64)
    for pk in range(p.P):
        n, b = int(p.lens[pk]), int(p.pack_start[pk])
        f = FIRST[n] if n else None
        if f is None:
            continue
        f = n - 1 if f == LAST else f
        p.first[pk] = f
        opaque[b + f] = True
        behind = rs.random_sample(n - f - 1) < 0.125          # further opaque samples behind the first: their weight must be exactly 0
        if f in (63, 127) and n > f + 1:
            behind[0] = True                                  # ... one of them right behind a chunk's last lane
        opaque[b + f + 1:b + n] = behind
    p.opaque = opaque
    p.sigma = opaque * OPAQUE / p.delta
    p.rgb = rs.randint(0, 9, size=(p.M, 3)) / 8.0
    p.depths = rs.randint(0, 65, size=p.M) / 16.0
    p.g_rgb = rs.randint(-2, 3, size=(p.N, 3)).astype(np.float64)
    p.g_depth = rs.randint(-2, 3, size=p.N).astype(np.float64)
    p.g_alpha = rs.randint(-2, 3, size=p.N).astype(np.float64)
    for g in (p.g_rgb, p.g_depth, p.g_alpha):          # the long rays carry the bulk of the samples: none of their upstream gradients is zero
        g[(p.len_of_ray >= 129) & (g.reshape(p.N, -1) == 0).all(1)] = 1.0
    p.sigma_in, p.delta_in, p.rgb_in, p.depths_in = (_padded(p, x) for x in (p.sigma, p.delta, p.rgb, p.depths))
    return p


def _render(p, sigma, rgb, pk):
    """One ray from the definition (torch, any dtype): tau = sigma delta, T_i = exp(-sum_{j<i} tau_j), w_i = T_i (1 - exp(-tau_i)), alpha = sum w,
    rgb = bg (1 - alpha) + alpha sum w c (the tracer composites colour with the weights and scales by alpha once more), depth = sum w d."""
    s = slice(int(p.pack_start[pk]), int(p.pack_start[pk + 1]))
    tau = sigma[s] * torch.from_numpy(p.delta[s]).to(sigma.dtype)
    T = torch.exp(-(torch.cumsum(tau, 0) - tau))
    w = T * (1.0 - torch.exp(-tau))
    alpha = w.sum()
    colour = (w[:, None] * rgb[s]).sum(0)
    out_rgb = (1.0 - alpha if p.bg_white else 0.0) + alpha * colour
    depth = (w * torch.from_numpy(p.depths[s]).to(sigma.dtype)).sum()
    return w, alpha, out_rgb, depth


def _reference_transmittance(p):
    r = types.SimpleNamespace()
    sigma = torch.from_numpy(p.sigma).requires_grad_()
    rgb = torch.from_numpy(p.rgb).requires_grad_()
    r.weights = np.zeros(p.M)
    r.alpha, r.depth = np.zeros(p.N), np.zeros(p.N)
    r.rgb = np.full((p.N, 3), 1.0 if p.bg_white else 0.0)
    loss = {u: 0.0 for u in UPSTREAM}
    for pk in range(p.P):
        ray = int(p.ray_of_pack[pk])
        w, alpha, out_rgb, depth = _render(p, sigma, rgb, pk)
        r.weights[int(p.pack_start[pk]):int(p.pack_start[pk + 1])] = w.detach().numpy()
        r.alpha[ray], r.depth[ray], r.rgb[ray] = float(alpha.detach()), float(depth.detach()), out_rgb.detach().numpy()
        terms = {"rgb": (torch.from_numpy(p.g_rgb[ray]) * out_rgb).sum(), "depth": p.g_depth[ray] * depth, "alpha": p.g_alpha[ray] * alpha}
        for u in ("rgb", "depth", "alpha"):
            loss[u] = loss[u] + terms[u]
            loss["full"] = loss["full"] + terms[u]
    r.hit = (r.alpha > 0).astype(np.uint8)
    r.d_sigma, r.d_rgb = {}, {}
    for u in UPSTREAM:
        ds, dc = torch.autograd.grad(loss[u], (sigma, rgb), retain_graph=True, allow_unused=True)
        r.d_sigma[u] = np.zeros(p.M) if ds is None else ds.numpy()
        r.d_rgb[u] = np.zeros((p.M, 3)) if dc is None else dc.numpy()
    return r


def _upstream(p, which):
    z = np.zeros_like
    return (p.g_rgb if which in ("full", "rgb") else z(p.g_rgb), p.g_depth if which in ("full", "depth") else z(p.g_depth),
            p.g_alpha if which in ("full", "alpha") else z(p.g_alpha))


def f32_transmittance(p, order_seed=None, chunked=False):
    """The forward and, per upstream gradient of UPSTREAM, the backward in f32 (numpy), every sum taken one addend at a time: in a random order
    (order_seed), or along the ray with the total of the finished 64-sample chunks carried in a scalar (chunked) - the two shapes a kernel's summation can
    take.  Written from the closed form d tau_i = gw_i (T_i - w_i) - sum_{k>i} gw_k w_k, gw_i = gA + gC . c_i + gD d_i, not by autograd."""
    f = np.float32
    rs = np.random.RandomState(order_seed if order_seed is not None else 0)
    r = types.SimpleNamespace(weights=np.zeros(p.M, f), alpha=np.zeros(p.N, f), depth=np.zeros(p.N, f), rgb=np.full((p.N, 3), 1.0 if p.bg_white else 0.0, f),
                              d_sigma={u: np.zeros(p.M, f) for u in UPSTREAM}, d_rgb={u: np.zeros((p.M, 3), f) for u in UPSTREAM})
    bg = f(1.0 if p.bg_white else 0.0)

    def total(x, order):          # [n, ...] -> the sum over axis 0, one addend at a time
        acc = np.zeros(x.shape[1:], f)
        for j in order:
            acc = (acc + x[j]).astype(f)
        return acc

    def before(x, order):         # [n] -> sum_{j<i} x_j for every i
        n, acc, at = len(x), np.zeros(len(x), f), np.arange(len(x))
        if chunked:
            carry = f(0.0)
            for c0 in range(0, n, 64):
                incl = np.cumsum(x[c0:c0 + 64], dtype=f)
                acc[c0:c0 + 64] = carry + (incl - x[c0:c0 + 64])
                carry = f(carry + incl[-1])
            return acc
        for j in order:
            acc[at > j] += x[j]
        return acc

    for pk in range(p.P):
        b, e, ray = int(p.pack_start[pk]), int(p.pack_start[pk + 1]), int(p.ray_of_pack[pk])
        n = e - b
        order = np.arange(n) if (chunked or order_seed is None) else rs.permutation(n)
        tau = (p.sigma[b:e].astype(f) * p.delta[b:e].astype(f)).astype(f)
        c, d, dl = p.rgb[b:e].astype(f), p.depths[b:e].astype(f), p.delta[b:e].astype(f)
        T = np.exp(-before(tau, order)).astype(f)
        w = (T * (f(1.0) - np.exp(-tau).astype(f))).astype(f)
        alpha = total(w, order)
        colour = total(w[:, None] * c, order)
        r.weights[b:e], r.alpha[ray], r.depth[ray] = w, alpha, total(w * d, order)
        r.rgb[ray] = bg * (f(1.0) - alpha) + alpha * colour
        for u in UPSTREAM:
            g_rgb, g_depth, g_alpha = (x[ray].astype(f) for x in _upstream(p, u))
            gC = g_rgb * alpha
            gA = f(g_alpha + total(g_rgb * (colour - bg), np.arange(3)))
            gw = (gA + total((gC[None] * c).T, np.arange(3)) + g_depth * d).astype(f)
            gww = (gw * w).astype(f)
            suffix = (total(gww, order) - (before(gww, order) + gww)).astype(f)
            r.d_sigma[u][b:e] = (gw * (T - w) - suffix) * dl
            r.d_rgb[u][b:e] = gC[None] * w[:, None]
    r.hit = (r.alpha > 0).astype(np.uint8)
    return r


def _fits_f32(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.isfinite(x).all()) and np.array_equal(x.astype(np.float32).astype(np.float64), x)


def _significant_bits(x):
    """Most significant bits any element of x needs (0 for zeros)."""
    m, _ = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    m = np.round(m * 2.0 ** 53).astype(np.int64)
    low = np.where(m != 0, m & -m, 1 << 53)
    return int(np.max(np.where(m != 0, 53 - np.log2(low).astype(np.int64), 0), initial=0))


def _check_transmittance(p):
    r = reference(p)
    fig = types.SimpleNamespace(samples=p.M, rays=p.N, packs=p.P)
    nz = r.d_sigma["full"] != 0
    fig.nonzero_d_sigma = int(nz.sum())
    assert 4 * fig.nonzero_d_sigma >= p.M, "only %d of %d samples have a non-zero d sigma" % (fig.nonzero_d_sigma, p.M)
    assert ((p.first < 0) & (p.lens >= 129)).any(), "no transparent ray of 129 or more samples"
    for edge in (64, 128):
        for at in (edge - 1, edge, edge + 1):
            assert (p.first == at).any(), "no ray whose first opaque sample is %d" % at
    for at in (0, 1, 62):
        assert (p.first == at).any()
    assert ((p.first == p.lens - 1) & (p.lens > 129)).any()
    # weights are one-hot at the first opaque sample; every opaque sample behind it weighs exactly nothing
    want = np.zeros(p.M)
    want[(p.pack_start[:-1] + p.first)[p.first >= 0]] = 1.0
    assert np.array_equal(r.weights, want)
    fig.opaque_behind = int((p.opaque & (want == 0)).sum())
    assert fig.opaque_behind >= 16
    for edge in (63, 127):          # the carry out of a chunk whose last lane is the first opaque sample decides the weight of the opaque sample behind it
        assert any(p.first[pk] == edge and p.lens[pk] > edge + 1 and p.opaque[p.pack_start[pk] + edge + 1] for pk in range(p.P))
    # sizes: the scan of tau counts opaque samples in units of 2048; sum |gw w| in units of the finest product (g/8 . c/8, g . d/16 -> 1/64 covers all)
    fig.tau_quanta = int(max((np.cumsum(p.opaque[int(b):int(e)]).max(initial=0) for b, e in zip(p.pack_start[:-1], p.pack_start[1:])), default=0))
    assert fig.tau_quanta < 2 ** 24
    g_rgb, g_depth, g_alpha = _upstream(p, "full")
    ray = p.ray_of_sample
    colour = np.zeros((p.N, 3))
    np.add.at(colour, ray, r.weights[:, None] * p.rgb)
    gA = g_alpha + (g_rgb * (colour - (1.0 if p.bg_white else 0.0))).sum(1)
    gw = gA[ray] + ((g_rgb * r.alpha[:, None])[ray] * p.rgb).sum(1) + g_depth[ray] * p.depths
    per_ray = np.zeros(p.N)
    np.add.at(per_ray, ray, np.abs(gw * r.weights))
    fig.gww_quanta = float(per_ray.max() * 64.0)
    assert np.array_equal(gw * 64.0, np.round(gw * 64.0)) and fig.gww_quanta < 2 ** 24
    for name in ("weights", "alpha", "rgb", "depth"):
        assert _fits_f32(getattr(r, name)), name
    for u in UPSTREAM:
        assert _fits_f32(r.d_sigma[u]) and _fits_f32(r.d_rgb[u]), u
    for x in (p.sigma, p.delta, p.rgb, p.depths):
        assert _fits_f32(x)
    # single upstream gradients: each still reaches d sigma (alpha alone only on the transparent rays: gw is constant along a ray)
    fig.nonzero_single = {u: int((r.d_sigma[u] != 0).sum()) for u in UPSTREAM[1:]}
    assert all(v >= 256 for v in fig.nonzero_single.values())
    return fig


# ------------------------------------------------------------------------------------------------------------------------------------ features
@functools.lru_cache(maxsize=None)
def features(form, pmod, C, seed=0, pad=0):
    p = _table(form, pmod, seed, pad=pad)
    rs = np.random.RandomState(seed * 7919 + C)
    p.kind, p.C = "features", C
    p.weights = rs.randint(0, 9, size=p.M) / 8.0
    p.alpha = rs.choice([0.0, 0.25, 0.5, 1.0], size=p.N)
    p.alpha[p.len_of_ray == 5000] = 0.5         # the long rays hold most rows of d feats
    p.alpha[p.len_of_ray == 1037] = 0.25
    p.feats = rs.randint(-2, 3, size=(p.M, C)).astype(np.float64)
    p.g = rs.randint(-2, 3, size=(p.N, C)).astype(np.float64)
    p.g[p.len_of_ray >= 1037, 0] = 1.0
    p.weights_in, p.feats_in = _padded(p, p.weights), _padded(p, p.feats)
    return p


def quarters(p):
    """[P, 5]: the sample ranges of the four wave quarters of every pack (q = ceil(n / 4) samples each, as the feature kernels split a pack)."""
    q = (p.lens + 3) // 4
    edges = p.pack_start[:-1, None] + np.arange(5)[None] * q[:, None]
    return np.minimum(edges, p.pack_start[1:, None])


def _reference_features(p):
    r = types.SimpleNamespace(out=np.zeros((p.N, p.C)), parts=np.zeros((p.P, 4, p.C)))
    edges = quarters(p)
    for pk in range(p.P):
        ray = int(p.ray_of_pack[pk])
        for q in range(4):
            s = slice(int(edges[pk, q]), int(edges[pk, q + 1]))
            r.parts[pk, q] = p.alpha[ray] * (p.weights[s, None] * p.feats[s]).sum(0)
        s = slice(int(p.pack_start[pk]), int(p.pack_start[pk + 1]))
        r.out[ray] = p.alpha[ray] * (p.weights[s, None] * p.feats[s]).sum(0)
    r.d_feats = (p.weights * p.alpha[p.ray_of_sample])[:, None] * p.g[p.ray_of_sample]
    return r


def f32_features(p, order_seed):
    """out in f32, one addend at a time in a random order per ray."""
    f = np.float32
    rs = np.random.RandomState(order_seed)
    out = np.zeros((p.N, p.C), f)
    w, x = p.weights.astype(f), p.feats.astype(f)
    for pk in range(p.P):
        b, e = int(p.pack_start[pk]), int(p.pack_start[pk + 1])
        acc = np.zeros(p.C, f)
        for j in rs.permutation(e - b):
            acc = (acc + w[b + j] * x[b + j]).astype(f)
        out[p.ray_of_pack[pk]] = f(p.alpha[p.ray_of_pack[pk]]) * acc
    return out


def _check_features(p):
    r = reference(p)
    fig = types.SimpleNamespace(samples=p.M, rays=p.N, packs=p.P)
    mag = np.zeros((p.N, p.C))
    np.add.at(mag, p.ray_of_sample, np.abs(p.weights[:, None] * p.feats))
    fig.sum_quanta = float(mag.max() * 8.0)          # units of 1/8
    assert fig.sum_quanta < 2 ** 24
    assert np.array_equal(p.weights * 8.0, np.round(p.weights * 8.0)) and p.weights.min() >= 0 and p.weights.max() <= 1
    fig.d_feats_bits = _significant_bits(r.d_feats)
    assert fig.d_feats_bits <= 8, "d feats needs %d significant bits: the bf16 store would round" % fig.d_feats_bits
    assert _significant_bits(p.feats) <= 8 and _fits_f32(r.out) and _fits_f32(r.d_feats)
    with_pack = p.has_pack & (p.len_of_ray > 0)
    fig.alpha_zero_rays = int((with_pack & (p.alpha == 0)).sum())
    assert fig.alpha_zero_rays >= 1 and all((with_pack & (p.alpha == a)).any() for a in (0.25, 0.5, 1.0))
    assert not r.d_feats[p.alpha[p.ray_of_sample] == 0].any() and (r.d_feats != 0).sum() * 4 >= r.d_feats.size
    fig.nonzero_out = int((r.out != 0).sum())
    assert fig.nonzero_out * 2 >= int(with_pack.sum()) * p.C          # most sums do not cancel
    return fig


# ------------------------------------------------------------------------------------------------- features composited with their own weights
@functools.lru_cache(maxsize=None)
def feature_weights(form, pmod, C=20, seed=0):
    """The transmittance problem (black background) with integer features on the samples: ops.composite_features computes the one-hot weights itself and
    hands sigma a gradient too (the delta-density tracer's node)."""
    t = transmittance(form, pmod, False, seed)
    p = types.SimpleNamespace(**{k: v for k, v in vars(t).items() if k != "_reference"})
    rs = np.random.RandomState(seed + 4242)
    p.kind, p.C = "feature_weights", C
    p.feats = rs.randint(-2, 3, size=(p.M, C)).astype(np.float64)
    p.g = rs.randint(-2, 3, size=(p.N, C)).astype(np.float64)
    return p


def _reference_feature_weights(p):
    r = types.SimpleNamespace(out=np.zeros((p.N, p.C)), alpha=np.zeros(p.N))
    sigma = torch.from_numpy(p.sigma).requires_grad_()
    feats = torch.from_numpy(p.feats).requires_grad_()
    loss = 0.0
    for pk in range(p.P):
        ray = int(p.ray_of_pack[pk])
        w, alpha, _, _ = _render(p, sigma, torch.from_numpy(p.rgb), pk)
        out = alpha * (w[:, None] * feats[int(p.pack_start[pk]):int(p.pack_start[pk + 1])]).sum(0)
        r.out[ray], r.alpha[ray] = out.detach().numpy(), float(alpha.detach())
        loss = loss + (torch.from_numpy(p.g[ray]) * out).sum()
    r.d_sigma, r.d_feats = (x.numpy() for x in torch.autograd.grad(loss, (sigma, feats)))
    return r


def _check_feature_weights(p):
    r = reference(p)
    fig = types.SimpleNamespace(samples=p.M, rays=p.N, packs=p.P, nonzero_d_sigma=int((r.d_sigma != 0).sum()), d_feats_bits=_significant_bits(r.d_feats))
    assert 4 * fig.nonzero_d_sigma >= p.M and fig.d_feats_bits <= 8
    assert all(_fits_f32(x) for x in (r.out, r.alpha, r.d_sigma, r.d_feats))
    s = (p.feats * p.g[p.ray_of_sample]).sum(1)          # the per-sample scalar the node hands to composite_bwd as a one-channel colour
    fig.s_max = float(np.abs(s).max())
    assert fig.s_max * p.lens.max() < 2 ** 24
    assert (r.d_feats != 0).any(1).sum() == int(((p.first >= 0) & (np.abs(p.g[p.ray_of_pack]).sum(1) > 0)).sum())          # one row per opaque ray: the weights are one-hot
    return fig


# --------------------------------------------------------------------------------------------------------------------------------- ray samples
@functools.lru_cache(maxsize=None)
def ray_samples(form, pmod, k=1, seed=0):
    """k = 1: samples [M, 3]; k = 2: the voxel march's [M / 2, 2, 3] (every pack an even number of samples)."""
    p = _table(form, pmod, seed, scale=k)
    rs = np.random.RandomState(seed + 31 * k)
    p.kind, p.k = "ray_samples", k
    p.g = rs.randint(-2, 3, size=(p.M, 3)).astype(np.float64)
    p.depths = rs.randint(0, 65, size=p.M) / 16.0
    p.origins, p.dirs = rs.randint(-4, 5, size=(p.N, 3)) / 4.0, rs.randint(-4, 5, size=(p.N, 3)) / 4.0
    p.samples = p.origins[p.ray_of_sample] + p.dirs[p.ray_of_sample] * p.depths[:, None]
    return p


def _reference_ray_samples(p):
    r = types.SimpleNamespace(d_origins=np.zeros((p.N, 3)), d_dirs=np.zeros((p.N, 3)))
    for pk in range(p.P):
        s = slice(int(p.pack_start[pk]), int(p.pack_start[pk + 1]))
        r.d_origins[p.ray_of_pack[pk]] = p.g[s].sum(0)
        r.d_dirs[p.ray_of_pack[pk]] = (p.g[s] * p.depths[s, None]).sum(0)
    return r


def f32_ray_samples(p, order_seed):
    f = np.float32
    rs = np.random.RandomState(order_seed)
    out = np.zeros((p.N, 6), f)
    g, d = p.g.astype(f), p.depths.astype(f)
    for pk in range(p.P):
        b, e = int(p.pack_start[pk]), int(p.pack_start[pk + 1])
        acc = np.zeros(6, f)
        for j in rs.permutation(e - b):
            acc = (acc + np.concatenate([g[b + j], g[b + j] * d[b + j]])).astype(f)
        out[p.ray_of_pack[pk]] = acc
    return out[:, :3], out[:, 3:]


def _check_ray_samples(p):
    r = reference(p)
    fig = types.SimpleNamespace(samples=p.M, rays=p.N, packs=p.P)
    mag = np.zeros((p.N, 3))
    np.add.at(mag, p.ray_of_sample, np.abs(p.g) * np.maximum(p.depths, 1.0)[:, None])
    fig.sum_quanta = float(mag.max() * 16.0)          # units of 1/16
    assert fig.sum_quanta < 2 ** 24 and _fits_f32(r.d_origins) and _fits_f32(r.d_dirs) and _fits_f32(p.samples)
    assert (p.lens % p.k == 0).all() and (r.d_dirs != 0).sum() * 2 >= int((p.len_of_ray > 0).sum()) * 3
    return fig


# --------------------------------------------------------------------------------------------------------------------------------------- common
def reference(p):
    """The fp64 reference of a problem, computed once and shared (read-only)."""
    if getattr(p, "_reference", None) is None:
        with torch.enable_grad():          # the transmittance gradients come from autograd, whatever mode the caller is in
            p._reference = {"transmittance": _reference_transmittance, "features": _reference_features, "ray_samples": _reference_ray_samples,
                            "feature_weights": _reference_feature_weights}[p.kind](p)
    return p._reference


def check_exact(p):
    """Raises unless the problem is exact in the sense of the module docstring; -> figures."""
    assert (p.lens_all == 0).sum() >= 4 and p.lens_all[0] == 0 and p.lens_all[-1] == 0
    assert set(PACKS) <= set((p.lens_all // getattr(p, "k", 1)).tolist())
    assert p.form != "boundary" or (p.lens > 0).all()
    assert p.form != "permuted" or (p.N > p.P and (np.diff(p.ray_of_pack) < 0).any())
    return {"transmittance": _check_transmittance, "features": _check_features, "ray_samples": _check_ray_samples,
            "feature_weights": _check_feature_weights}[p.kind](p)


def _where(p, kind, index, parts=None, got=None, want=None):
    """Names the ray, pack length, chunk / quarter and column of one element of a per-sample ("sample") or per-ray ("ray") tensor."""
    row, col = index[0], (index[1] if len(index) > 1 else None)
    column = "" if col is None else ", column %d" % col
    if kind == "sample":
        if row >= p.M:
            return "filler row %d of a padded batch (pack_start[P] = %d)%s" % (row, p.M, column)
        pk, pos = int(p.pack_of_sample[row]), int(p.pos[row])
        n = int(p.lens[pk])
        return "sample %d = position %d of pack %d (ray %d, %d samples): 64-sample chunk %d lane %d, wave quarter %d%s" % (
            row, pos, pk, int(p.ray_of_pack[pk]), n, pos // 64, pos % 64, pos // ((n + 3) // 4), column)
    packs = np.flatnonzero(p.ray_of_pack == row)
    if not len(packs):
        return "ray %d, which has no pack%s" % (row, column)
    pk = int(packs[0])
    text = "ray %d = pack %d of %d samples (%d chunks of 64, quarters of %d)" % (row, pk, int(p.lens[pk]), (int(p.lens[pk]) + 63) // 64, (int(p.lens[pk]) + 3) // 4)
    if getattr(p, "first", None) is not None:
        f = int(p.first[pk])
        text += ", transparent" if f < 0 else ", first opaque sample at position %d (chunk %d lane %d)" % (f, f // 64, f % 64)
    if parts is not None and col is not None:          # which wave quarter's partial sum accounts for the difference
        share = parts[pk, :, col]
        text += "; wave quarter sums %s" % share.tolist()
        for q in range(4):
            if share[q] != 0 and got == want - share[q]:
                text += " - the value is the reference without quarter %d" % q
    return text + column


def assert_bit_equal(name, got, want_fp64, p, kind, parts=None):
    """torch.equal by value (signed zeros compare equal) after casting the fp64 reference to the dtype of `got`."""
    got = got.detach().cpu()
    want = torch.from_numpy(np.ascontiguousarray(want_fp64)).to(got.dtype)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (name, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    g, w = got.double(), want.double()
    bad = g != w          # NaN differs from everything: no reference value is NaN
    at = torch.nonzero(bad)
    first = tuple(at[0].tolist())
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r; %s" % (
        name, int(bad.sum()), bad.numel(), first, float(g[first]), float(w[first]), _where(p, kind, first, parts, float(g[first]), float(w[first]))))


# ---------------------------------------------------------------------------------------------------------------------------------------- cases
TABLES = [(form, pmod) for form in FORMS for pmod in PMODS]
# feature widths by the branch of pag_composite_feats_fwd they take (the table next to the dispatcher's conditions is in test_gpu_exact_composite.py)
C_SMALL = (1, 7, 16)
C_SCALAR = (17, 30, 63, 65, 201, 255)
C_VECTOR = (20, 64, 200, 256)
C_BWD = (1, 16, 17, 64, 65, 200, 256)
PAD = 77          # filler rows of the padded-batch cases
FEATURE_PAD_CASES = [("identity", 1, 20), ("boundary", 3, 7)]


def feature_cases():
    """(form, pmod, C): every table form and P % 4 at one width per kernel family, every width on one table of each form."""
    cases = [(form, pmod, C) for form, pmod in TABLES for C in (7, 30, 64)]
    widths = sorted(set(C_SMALL + C_SCALAR + C_VECTOR + C_BWD))
    cases += [(FORMS[i % 3], PMODS[(i // 3) % 3], C) for i, C in enumerate(widths)]
    return sorted(set(cases + FEATURE_PAD_CASES))          # the padded cases' tables also run unpadded (C = 20: at a one-element offset too)


def transmittance_cases():
    """(form, pmod, bg_white, pad)"""
    return [(form, pmod, bg, 0) for form, pmod in TABLES for bg in (True, False)] + [("identity", 1, True, PAD)]


def ray_sample_cases():
    """(form, pmod, k): the layouts [M, 3] and [M / 2, 2, 3]."""
    return [(form, pmod, k) for form in FORMS[:2] for pmod in PMODS for k in (1, 2)]
