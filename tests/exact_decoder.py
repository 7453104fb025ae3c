"""Decoder problems whose arithmetic is exact, shared by tests/test_exact_decoder_host.py and tests/test_gpu_exact_decoders.py.

Every value a decoder kernel rounds to bf16 (inputs, weights, post-ReLU hidden activations, dz and hidden gradients, bf16 outputs and input gradients) is
a small integer here, so every product is an integer and every f32 sum stays far below 2^24: the result does not depend on the summation order, the MFMA
layout, the slicing of the weight gradients or atomics, and no ReLU decision can flip.  The forward and every gradient of a decoder without output
activation must then EQUAL an fp64 reference, element by element.  With a sigmoid / softmax head the last layer is scaled by a power of two (|logit| <= 16):
the logits stay exact and only the activation itself (exp2, rcp) and the bf16 rounding of dz after it carry an error.

make_problem() builds a problem, reference() evaluates it in fp64, check_exact() proves the claims above for one problem (it raises otherwise), and
assert_bit_equal() is torch.equal with a message that names the tile, workgroup or slice at fault."""
import types

import numpy as np
import torch

ACT_NONE, ACT_SIGMOID, ACT_SOFTMAX = 0, 1, 2
MAX_LOGIT = 16.0
INACTIVE_CAP = 0.05          # share of hidden units per layer that may be always-on or always-off
SMALL_ROW = 2.0 ** -6        # (b) backward: rows whose reference gradient norm is below this share of the median row norm are exempt ...
SMALL_ROW_CAP = 0.01         # ... and at most this share of the rows may be


def xcd8_columns(levels, feats):
    from pagnerf_amd import ops
    return ops.xcd8_columns(levels, feats)


def to_xcd8(x, levels, feats, fill):
    """[M, levels*feats] -> bf16 [8, M, 8]; padding positions hold `fill`."""
    x8 = torch.full((8, x.shape[0], 8), float(fill))
    for p, c in enumerate(xcd8_columns(levels, feats)):
        if c >= 0:
            x8[p >> 3, :, p & 7] = x[:, c].float()
    return x8.bfloat16()


def from_xcd8(x8, levels, feats):
    """bf16 [8, M, 8] -> (f32 [M, levels*feats], the padding positions as [n_pad, M])."""
    x8 = x8.float().cpu()
    out = torch.zeros(x8.shape[1], levels * feats)
    pad = []
    for p, c in enumerate(xcd8_columns(levels, feats)):
        if c >= 0:
            out[:, c] = x8[p >> 3, :, p & 7]
        else:
            pad.append(x8[p >> 3, :, p & 7])
    return out, torch.stack(pad)


def _sparse(rs, n_out, n_in, nnz, values):
    """[n_out, n_in] with `nnz` non-zeros per row drawn from `values`, then one more in every column that got none."""
    W = np.zeros((n_out, n_in))
    cols = np.argsort(rs.random_sample((n_out, n_in)), axis=1)[:, :min(nnz, n_in)]
    vals = rs.choice(values, size=cols.shape)
    vals[:, 0::2], vals[:, 1::2] = np.abs(vals[:, 0::2]), -np.abs(vals[:, 1::2])          # both signs in every row: a ReLU unit behind it switches
    np.put_along_axis(W, cols, vals, axis=1)
    for c in np.flatnonzero(~W.any(0)):
        W[rs.randint(n_out), c] = rs.choice(values)
    return W


def make_problem(dims, M, seed, form, out_act=ACT_NONE, pad_fill=0.0, zero_go_rows=None, R=50, max_logit=MAX_LOGIT, x1_values=None):
    """dims = (in_dim, hidden ..., out_dim).  form: "xcd8" (in_dim = 24 levels x 2) | "strided" (f32 x1) | "strided_bf16" | k1 (f32 x1 [M, k1] followed by
    a gathered x2 [R, 32]) | ("bf16", k1) (the same with a bf16 x1) | ("packs", k1) (bf16 x1, and the index's packs handed over).
    pad_fill: what the XCD8 padding positions hold (NaN for forward-only use, 0 where a backward follows).  Strided inputs carry NaN in the columns at or
    beyond in_dim.  zero_go_rows = (r0, r1): those rows of the upstream gradient are zero.  x1_values: the integer-valued x1 columns to use instead of
    drawn ones (a decoder fed by another decoder's exact output, two heads on one input)."""
    rs = np.random.RandomState(seed)
    p = types.SimpleNamespace(dims=tuple(dims), M=M, seed=seed, form=form, out_act=out_act, zero_go_rows=zero_go_rows)
    in_dim, n = dims[0], len(dims) - 1
    W = [_sparse(rs, dims[i + 1], dims[i], 6 if i == 0 else 4, [-2, -1, 1, 2] if i == 0 else [-1, 1]) for i in range(n)]
    b = [rs.randint(-1, 2, size=dims[i + 1]).astype(np.float64) for i in range(n)]
    p.grouped = p.x2 = p.idx = p.packs = None
    if form in ("xcd8", "strided", "strided_bf16"):
        x = rs.randint(-1, 2, size=(M, in_dim)).astype(np.float64)
        if x1_values is not None:
            x = x1_values.double().numpy().copy()
        p.k1 = p.n1 = in_dim
    else:
        k1 = form[1] if isinstance(form, tuple) else form
        x1 = rs.randint(-1, 2, size=(M, k1))
        if x1_values is not None:
            x1 = x1_values.double().numpy()
        x2 = rs.randint(-1, 2, size=(R, in_dim - k1))
        idx = np.sort(rs.randint(0, R, size=M)).astype(np.int32)
        x = np.concatenate([x1, x2[idx]], 1).astype(np.float64)
        p.k1 = p.n1 = k1
        p.x2 = torch.zeros(R, 32)
        p.x2[:, :in_dim - k1] = torch.from_numpy(x2).float()
        p.idx = torch.from_numpy(idx)
    p.x = torch.from_numpy(x)
    go = rs.choice([-1.0, 1.0], size=(M, dims[-1])) * (rs.random_sample((M, dims[-1])) < 6.0 / dims[-1])
    if out_act != ACT_NONE and dims[-1] <= 8:          # both signs in every row: a softmax row whose upstream gradient is constant has no gradient at all
        go[:, 0], go[:, 1] = 1.0, -1.0
    if zero_go_rows is not None:
        go[zero_go_rows[0]:zero_go_rows[1]] = 0.0
    p.go = torch.from_numpy(go)
    p.scale = 1.0
    if out_act != ACT_NONE:          # the last layer scaled by a power of two: |logit| <= max_logit, and the logits stay exact
        h = p.x
        for i in range(n):
            h = h @ torch.from_numpy(W[i]).t() + torch.from_numpy(b[i])
            if i + 1 < n:
                h = torch.relu(h)
        top = float(h.abs().max())
        while top * p.scale > max_logit:
            p.scale *= 0.5
        W[-1], b[-1] = W[-1] * p.scale, b[-1] * p.scale
    p.W = [torch.from_numpy(w) for w in W]
    p.b = [torch.from_numpy(v) for v in b]
    # ---- the forms the ops take
    xf = p.x.float()
    if form == "xcd8":
        assert in_dim == 48
        p.grouped = (24, 2)
        p.x1 = to_xcd8(xf, 24, 2, pad_fill)
    elif form in ("strided", "strided_bf16"):
        p.k1 = (in_dim + 7) // 8 * 8
        p.x1 = torch.full((M, p.k1), float("nan"))
        p.x1[:, :in_dim] = xf
        if form == "strided_bf16":
            p.x1 = p.x1.bfloat16()
    else:
        p.x1 = xf[:, :p.k1].contiguous()
        if isinstance(form, tuple):
            p.x1 = p.x1.bfloat16()
            if form[0] == "packs":          # one pack per run of equal indices
                rays, counts = torch.unique_consecutive(p.idx, return_counts=True)
                p.packs = (torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)]), rays.int())
    return p


def bf16_round(t):
    return t.float().bfloat16().to(t.dtype)


def reference(p, out_act=None, round_dz=False, out_bf16=False):
    """fp64.  -> namespace with out, logits, hidden[i] (post-ReLU), dz[i], dh[i] (the gradient of hidden[i]), dx (all columns), dx1, dx2, dW[i], db[i].
    round_dz / out_bf16: the kernels' rounding points behind an output activation - the backward reads the saved output in its own dtype, and dz and the
    hidden gradients travel as bf16.  out_bf16 = "outer": the 64-wide family's wide softmax head, dz = bf16(y) * (g - <y, g>) with the f32 probabilities
    it rebuilds in the inner product and their bf16 rounding ("the precision the stored probabilities had") as the outer factor (mlp_bwd_wide_mfma and
    the fused wide-head backward in csrc/mlp.hip).  On a problem without output activation those roundings change nothing (check_exact)."""
    act = p.out_act if out_act is None else out_act
    n = len(p.W)
    r = types.SimpleNamespace(hidden=[], dz=[None] * n, dh=[None] * (n - 1), dW=[None] * n, db=[None] * n)
    h = p.x
    for i in range(n):
        z = h @ p.W[i].t() + p.b[i]
        if i + 1 < n:
            h = torch.relu(z)
            r.hidden.append(h)
    r.logits = z
    r.out = torch.sigmoid(z) if act == ACT_SIGMOID else (torch.softmax(z, -1) if act == ACT_SOFTMAX else z)
    o = bf16_round(r.out) if out_bf16 else r.out
    o_dot = r.out if out_bf16 == "outer" else o
    if act == ACT_SIGMOID:
        dz = p.go * o * (1 - o)
    elif act == ACT_SOFTMAX:
        dz = o * (p.go - (p.go * o_dot).sum(-1, keepdim=True))
    else:
        dz = p.go.clone()
    for i in range(n - 1, -1, -1):
        if round_dz:
            dz = bf16_round(dz)
        r.dz[i] = dz
        a = p.x if i == 0 else r.hidden[i - 1]
        r.dW[i], r.db[i] = dz.t() @ a, dz.sum(0)
        d = dz @ p.W[i]
        if i:
            r.dh[i - 1] = d
            dz = d * (r.hidden[i - 1] > 0)
    r.dx = d
    r.dx1 = d[:, :p.n1]
    r.dx2 = None
    if p.x2 is not None:
        r.dx2 = torch.zeros(p.x2.shape[0], p.dims[0] - p.n1, dtype=torch.float64).index_add_(0, p.idx.long(), d[:, p.n1:])
    return r


def _is_bf16(t):
    return torch.equal(bf16_round(t), t)


def unit_activity(p, ref):
    """Per hidden layer: the share of units that are active for every row or for none."""
    return [float((((h > 0).all(0)) | ((h <= 0).all(0))).double().mean()) for h in ref.hidden]


def check_exact(p, ref=None, out_bf16=False, dx1_bf16=False):
    """Raises unless the problem is exact at every rounding point of the kernels (module docstring) and exercises every unit, weight and gradient tile."""
    ref = reference(p) if ref is None else ref
    lim = 2.0 ** 24

    def need(ok, what):
        if not ok:
            raise AssertionError("%s M=%d seed=%d %s: %s" % (p.dims, p.M, p.seed, p.form, what))
    need(_is_bf16(p.x), "input not bf16")
    if p.x2 is not None:
        need(_is_bf16(p.x2), "x2 not bf16")
    n = len(p.W)
    for i in range(n):
        need(_is_bf16(p.W[i]), "W%d not bf16" % i)
        need(bool((p.W[i] != 0).any(0).all()) and bool((p.W[i] != 0).any(1).all()), "W%d has an unused row or column" % i)
        a = p.x if i == 0 else ref.hidden[i - 1]
        # every partial sum of the forward, in units of the last layer's scale: sum_k |a||W| + |b|
        unit = p.scale if i == n - 1 else 1.0
        need(float((a.abs() @ p.W[i].abs().t() + p.b[i].abs()).max()) / unit < lim, "forward sum of layer %d reaches 2^24" % i)
        need(torch.equal(torch.round(p.W[i] / unit), p.W[i] / unit) and torch.equal(torch.round(p.b[i] / unit), p.b[i] / unit), "layer %d not integer" % i)
    for i, h in enumerate(ref.hidden):
        need(_is_bf16(h), "hidden %d not bf16" % i)
    if p.M >= 31:
        for i, share in enumerate(unit_activity(p, ref)):
            need(share <= INACTIVE_CAP, "hidden %d: %.1f %% of the units never change state" % (i, 100 * share))
    else:          # a single row cannot switch a unit: both states must occur within every layer instead
        for i, h in enumerate(ref.hidden):
            need(bool((h > 0).any()) and bool((h <= 0).any()), "hidden %d: one state only" % i)
    go = p.go
    tiles = (go != 0).any(1)
    for t0 in range(0, p.M, 32):
        inside = p.zero_go_rows is not None and t0 >= p.zero_go_rows[0] and t0 + 32 <= p.zero_go_rows[1]
        need(inside or bool(tiles[t0:t0 + 32].any()), "upstream gradient tile at row %d is zero" % t0)
        need(not inside or not bool(tiles[t0:t0 + 32].any()), "upstream gradient tile at row %d should be zero" % t0)
    need(_is_bf16(go), "upstream gradient not bf16")
    if p.out_act != ACT_NONE:
        need(float(ref.logits.abs().max()) <= MAX_LOGIT, "logit beyond %g" % MAX_LOGIT)
        need(torch.equal(ref.logits.float().double(), ref.logits), "logits not exact in f32")
        return ref
    if out_bf16:
        need(_is_bf16(ref.out), "output not bf16")
    for i in range(n):
        need(_is_bf16(ref.dz[i]), "dz %d not bf16" % i)
        a = p.x if i == 0 else ref.hidden[i - 1]
        need(float((ref.dz[i].abs().t() @ a.abs()).max()) < lim and float(ref.dz[i].abs().sum(0).max()) < lim, "dW / db sum of layer %d reaches 2^24" % i)
        need(float((ref.dz[i].abs() @ p.W[i].abs()).max()) < lim, "backward sum of layer %d reaches 2^24" % i)
    for i, d in enumerate(ref.dh):
        need(_is_bf16(d), "hidden gradient %d not bf16" % i)
    if dx1_bf16:
        need(_is_bf16(ref.dx1), "dx1 not bf16")
    if ref.dx2 is not None:
        seg = torch.zeros(p.x2.shape[0], p.dims[1], dtype=torch.float64).index_add_(0, p.idx.long(), ref.dz[0].abs())
        need(float((seg @ p.W[0][:, p.n1:].abs()).max()) < lim, "dx2 sum reaches 2^24")
    return ref


def mismatch_report(name, got, want):
    """The message of assert_bit_equal: first differing (row, column), count, and the differing rows modulo 32, 128 and 256."""
    g2, w2 = got.reshape(got.shape[0], -1) if got.dim() > 1 else got.reshape(-1, 1), want.reshape(want.shape[0], -1) if want.dim() > 1 else want.reshape(-1, 1)
    bad = ~((g2 == w2) | (torch.isnan(g2) & torch.isnan(w2)))
    rows, cols = torch.nonzero(bad, as_tuple=True)
    r0, c0 = int(rows[0]), int(cols[0])
    ur = torch.unique(rows)
    mods = "; ".join("mod %d: %s" % (m, sorted(set((ur % m).tolist()))[:40]) for m in (32, 128, 256))
    return ("%s: %d of %d elements differ in %d of %d rows; first at (row %d, column %d): got %r, want %r; differing columns %s; differing rows %s ... %s"
            % (name, int(bad.sum()), bad.numel(), ur.numel(), g2.shape[0], r0, c0, float(g2[r0, c0]), float(w2[r0, c0]),
               sorted(set(cols.tolist()))[:40], ur[:8].tolist(), mods))


def assert_bit_equal(name, got, want_fp64):
    """torch.equal after casting the fp64 reference to the dtype of `got`."""
    got = got.detach().cpu()
    want = want_fp64.to(got.dtype)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (name, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        raise AssertionError(mismatch_report(name, got.float(), want.float()))


# --------------------------------------------------------------------------------------------------------- (b): heads with an output activation
def forward_rel_error(got, want_fp64):
    """Worst relative error per element of an activated output against the fp64 value."""
    return float(((got.detach().cpu().double() - want_fp64).abs() / want_fp64.abs()).max())


def row_errors(got, want_fp64):
    """Per row |got - want| / |want| (L2), and which rows count: those whose reference norm is at least SMALL_ROW of the median row norm."""
    want = want_fp64.reshape(want_fp64.shape[0], -1)
    got = got.detach().cpu().double().reshape(want.shape)
    norm = want.norm(dim=1)
    keep = norm >= SMALL_ROW * norm.median()
    return (got - want).norm(dim=1) / norm.clamp_min(1e-300), keep


def f32_backward(p, out_bf16=False):
    """The plain f32 tensor-op evaluation of the backward behind an output activation, with the kernels' rounding points: what it loses per row against
    reference(round_dz=True) is the yardstick of the kernels' own loss (the bound is 4 x its worst row, floor 2^-8)."""
    n = len(p.W)
    W, b = [w.float() for w in p.W], [v.float() for v in p.b]
    h, hidden = p.x.float(), []
    for i in range(n):
        z = h @ W[i].t() + b[i]
        if i + 1 < n:
            h = torch.relu(z)
            hidden.append(h)
    o = torch.sigmoid(z) if p.out_act == ACT_SIGMOID else torch.softmax(z, -1)
    o_dot = o
    if out_bf16:
        o = o.bfloat16().float()
        o_dot = o_dot if out_bf16 == "outer" else o
    go = p.go.float()
    dz = go * o * (1 - o) if p.out_act == ACT_SIGMOID else o * (go - (go * o_dot).sum(-1, keepdim=True))
    r = types.SimpleNamespace(dW=[None] * n, db=[None] * n)
    for i in range(n - 1, -1, -1):
        dz = dz.bfloat16().float()
        a = p.x.float() if i == 0 else hidden[i - 1]
        r.dW[i], r.db[i] = dz.t() @ a, dz.sum(0)
        d = dz @ W[i]
        if i:
            dz = d * (hidden[i - 1] > 0)
    r.dx1 = d[:, :p.n1]
    return r


def backward_bound(p, ref, out_bf16=False):
    """-> (bound, worst row of the f32 evaluation, share of exempt rows) for d x1 of an activated head."""
    err, keep = row_errors(f32_backward(p, out_bf16).dx1, ref.dx1)
    worst = float(err[keep].max())
    return max(4.0 * worst, 2.0 ** -8), worst, float((~keep).double().mean())


# ------------------------------------------------------------------------------------------------------------------------------------- cases
SEED = 7
GRID_ROUND_128 = 256 * 256          # one round of the 128-wide kernels' grid: 256 samples x 256 workgroups
GRID_FAST_FWD, GRID_MLP = 768 * 128, 1536 * 128          # the 64-wide family: FAST_FWD_GRID_CAP and mlp_grid's cap, in samples

# ---- (a) 128-wide.  The input forms and the in_dim each is run at: 27 and 43 leave NaN columns in a strided x1
FORMS_128 = [("xcd8", 48), ("strided", 27), ("strided_bf16", 43), (16, 43), (("packs", 16), 43)]
OUT_DIMS_128 = (3, 16, 32, 33, 128, 129, 200, 224)
# the four cases that differ in kernel instantiation, run at every other M: (dims, form, out bf16)
CORNERS_128 = [((48, 128, 16), "xcd8", True), ((27, 128, 128, 200), "strided", False), ((43, 128, 128, 128, 3), 16, False),
               ((43, 128, 128, 33), ("packs", 16), True)]
M_OTHER_128 = (1, 31, 33, 255, 257, GRID_ROUND_128 + 37)


def dims_128(n_hidden, in_dim, out_dim):
    return (in_dim,) + (128,) * n_hidden + (out_dim,)


# ---- (a) 64-wide: (form, in_dim, out bf16, modes).  XCD8 input exists on the MFMA path only
FORMS_64 = [("strided", 32, False, ("fp32", "bf16")), ("strided_bf16", 27, False, ("fp32", "bf16")), ("xcd8", 48, False, ("bf16",)),
            ("xcd8", 48, True, ("bf16",)), (16, 43, False, ("fp32", "bf16")), (("bf16", 16), 43, False, ("fp32", "bf16"))]
OUT_DIMS_64 = (16, 40, 100, 200)
M_64 = (1, 31, 33, 127, 129, 1037)
GRID_CASES_64 = [((48, 64, 16), GRID_FAST_FWD + 37), ((48, 64, 64, 32), GRID_FAST_FWD + 37), ((48, 64, 16), GRID_MLP + 37), ((48, 64, 64, 32), GRID_MLP + 37)]
AFFINE_CASES = [(1, 1), (8, 33), (8, 1037), (3, 257)]          # (n_out <= AFF_MAX_OUT = 8, M)
ZERO_TILE_ROWS = (64, 128)


def dims_64(n_layers, in_dim, out_dim):
    return (in_dim,) + (64,) * (n_layers - 1) + (out_dim,)


# ---- (b): (dims, out_act, form, out bf16, max |logit|).  All run below 16: a saturated head leaves too many rows without a gradient
HEADS_128 = [((48, 128, 128, 200), ACT_SOFTMAX, "xcd8", True, 8.0), ((48, 128, 6), ACT_SOFTMAX, "xcd8", False, 2.0), ((43, 128, 128, 3), ACT_SIGMOID, 16, False, 4.0)]
HEADS_64 = [((48, 64, 64, 200), ACT_SOFTMAX, "xcd8", True, 8.0), ((48, 64, 6), ACT_SOFTMAX, "xcd8", False, 2.0), ((43, 64, 64, 3), ACT_SIGMOID, ("bf16", 16), False, 4.0)]
M_HEADS_128 = (33, 1037, GRID_ROUND_128 + 37)
M_HEADS_64 = (33, 1037, GRID_FAST_FWD + 37)

_CACHE = {}


def backward_reads_bf16_out(family, dims, out_bf16):
    """How the backward behind an output activation reads the output (reference()'s out_bf16): as saved, i.e. bf16 wherever the output is bf16 - except
    the 64-wide family's wide softmax head, which rebuilds the f32 probabilities from the saved softmax statistics and rounds the outer factor only."""
    if family == 64 and dims[-1] > 64 and out_bf16:
        return "outer"
    return bool(out_bf16)


def with_go(p, go):
    """A copy of the (shared) problem with another upstream gradient."""
    q = types.SimpleNamespace(**vars(p))
    q.go = go
    return q


def rays_for(M, seed):
    """Samples packed ray by ray, at most 64 per ray, with a one-sample ray and an empty ray up front.  -> counts (numpy int64 [N])"""
    rs = np.random.RandomState(seed)
    counts, left = [1, 0], M - 1
    while left > 0:
        c = min(left, int(rs.randint(1, 65)))
        counts.append(c)
        left -= c
    return np.asarray(counts, dtype=np.int64)


def problem(dims, M, form, out_act=ACT_NONE, max_logit=MAX_LOGIT, zero_go_rows=None, seed=SEED):
    """make_problem + reference, computed once per session and shared (nobody writes into them)."""
    key = (tuple(dims), M, form, out_act, max_logit, zero_go_rows, seed)
    if key in _CACHE:
        return _CACHE[key]
    p = make_problem(dims, M, seed, form, out_act=out_act, zero_go_rows=zero_go_rows, max_logit=max_logit)
    res = (p, reference(p))
    if M <= 2048:          # the large ones are used once
        if len(_CACHE) >= 64:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = res
    return res


def cases_a():
    """Every (dims, M, form, zero_go_rows) of section (a), each once: what the host test proves exact."""
    seen = []
    for n_hidden in (1, 2, 3):
        for form, in_dim in FORMS_128:
            for out_dim in OUT_DIMS_128:
                seen.append((dims_128(n_hidden, in_dim, out_dim), 1037, form, None))
    for dims, form, _ in CORNERS_128:
        seen += [(dims, M, form, None) for M in M_OTHER_128]
    seen.append((CORNERS_128[1][0], 257, CORNERS_128[1][1], ZERO_TILE_ROWS))
    seen.append(((48, 128, 128, 200), 1037, "xcd8", None))          # dx1_accumulate
    for form, in_dim, _, _ in FORMS_64:
        for n_layers in (2, 3):
            for out_dim in OUT_DIMS_64:
                seen += [(dims_64(n_layers, in_dim, out_dim), M, form, None) for M in M_64]
    seen += [(dims, M, "xcd8", None) for dims, M in GRID_CASES_64]
    seen.append(((48, 64, 16), 257, "xcd8", ZERO_TILE_ROWS))
    seen += [((48, n_out), M, "xcd8", None) for n_out, M in AFFINE_CASES]
    out = []
    for c in seen:
        if c not in out:
            out.append(c)
    return out
