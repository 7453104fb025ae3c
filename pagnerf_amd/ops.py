"""torch.autograd wrappers around the C-ABI kernels (include/pagnerf_hip.h).

Everything here runs on GPU tensors only; there is no CPU fallback (the oracle under oracle/
is test infrastructure and is never imported from this package).
"""
import ctypes
import os
import threading
import time

import torch

from . import _lib as L


# Optional per-entry-point device timing (bench.py): HIP events recorded on the launch stream
# (torch's current stream, which is the stream every kernel is launched on) around each C-ABI call.
_PROFILE = None


_PROFILE_ONLY = None


def profile_start(only=None):
    """only: optional set of entry-point names - events are then recorded around those calls alone (two event records per
    call cost host time and a marker packet on the stream; ~50 of them per training step are measurable)."""
    global _PROFILE, _PROFILE_ONLY
    _PROFILE = {}
    _PROFILE_ONLY = set(only) if only is not None else None


def profile_stop():
    """-> {entry point: [milliseconds per call]} (synchronises)."""
    global _PROFILE
    prof, _PROFILE = _PROFILE, None
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in (prof or {}).items()}


def _call(name, *args):
    fn = getattr(L.load(), name)
    if _PROFILE is None or (_PROFILE_ONLY is not None and name not in _PROFILE_ONLY):
        L.check(fn(*args), name)
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    L.check(fn(*args), name)
    b.record()
    _PROFILE.setdefault(name, []).append((a, b))


def _check_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("pagnerf_amd ops need GPU tensors (no CPU fallback); got a tensor on %s" % t.device)


# ------------------------------------------------------------------------------------------- encode
class _EncodeSpec:
    """Static description of a grid encoder (host-side per-level parameters).  Holds plain Python numbers (picklable:
    `torch.save(pipeline)` is the reference's default checkpoint format, config_parser.py:753-756); the ctypes float arrays
    the C ABI takes are built from them once per process."""

    def __init__(self, kind, n_levels, n_feat, **kw):
        self.kind = kind
        self.L = int(n_levels)
        self.F = int(n_feat)
        if kind == "hash":
            self.kw = dict(log2_T=int(kw["log2_T"]), resolutions=_float_list(kw["resolutions"]), half_coords=bool(kw.get("half_coords", False)))
        elif kind == "permuto":
            self.kw = dict(capacity=int(kw["capacity"]), scale_factor=_float_list(kw["scale_factor"]), shift=_float_list(kw["shift"]),
                           half_coords=bool(kw.get("half_coords", False)))
        else:
            raise ValueError(kind)
        self._bind()

    def _bind(self):
        kw = self.kw
        self.flags = L.ENC_HALF_COORDS if kw["half_coords"] else 0
        if self.kind == "hash":
            self.log2_T = kw["log2_T"]
            self.res = L.host_floats(kw["resolutions"])
            self.vertices, self._mid = 8, (self.log2_T, self.res)
        else:
            self.capacity = kw["capacity"]
            self.sf = L.host_floats(kw["scale_factor"])
            self.shift = L.host_floats(kw["shift"])
            self.vertices, self._mid = 4, (self.capacity, self.sf, self.shift)

    def mid(self, feat_scale):
        """The kind-specific middle of every pag_<kind>_encode_* argument list (the prototypes of include/pagnerf_hip.h): hash log2_T, resolutions, feat_scale; permuto capacity,
        scale_factor, shift, feat_scale."""
        return self._mid + (L.host_floats(feat_scale),)

    def __getstate__(self):
        return dict(kind=self.kind, L=self.L, F=self.F, kw=self.kw)

    def __setstate__(self, state):
        self.kind, self.L, self.F, self.kw = state["kind"], state["L"], state["F"], state["kw"]
        self._bind()

    def rows(self):
        return (1 << self.log2_T) if self.kind == "hash" else self.capacity


def _float_list(values):
    if isinstance(values, torch.Tensor):
        return values.detach().cpu().float().reshape(-1).tolist()
    import numpy as np
    return np.asarray(values, dtype=np.float32).reshape(-1).tolist()


def hash_spec(resolutions, log2_T, n_feat, half_coords=False):
    return _EncodeSpec("hash", len(resolutions), n_feat, log2_T=log2_T, resolutions=resolutions, half_coords=half_coords)


def permuto_spec(scale_factor, shift, capacity, n_feat, half_coords=False):
    """scale_factor, shift: [L,3] (torch CPU / numpy).  half_coords: the kernels round xyz to fp16 first - what the reference's
    `custom_fwd(cast_inputs=torch.half)` does to the coordinates under the trainer's autocast (grids/permuto_grid.py:65,71)."""
    return _EncodeSpec("permuto", len(scale_factor), n_feat, capacity=capacity, scale_factor=scale_factor, shift=shift,
                       half_coords=half_coords)


def _layout_args(t):
    """(stride_m, stride_c, layout) of a feature tensor: [M, C] strided or bf16 [8, M, 8] XCD-grouped."""
    if t.dim() == 3:
        assert t.shape[0] == 8 and t.shape[2] == 8 and t.dtype == torch.bfloat16 and t.is_contiguous()
        return 0, 0, L.LAYOUT_XCD8
    return t.stride(0), t.stride(1), L.LAYOUT_STRIDED


def _encode_call(op, spec, feat_scale, flags, head, tail):
    """pag_<kind>_encode_<op>(*head, the spec's middle, *tail, flags, stream); flags None = as the spec says."""
    _call("pag_%s_encode_%s" % (spec.kind, op), *head, *spec.mid(feat_scale), *tail, spec.flags if flags is None else flags, L.stream())


def _encode_fwd(spec, xyz, tables, feat_scale, out, addend=None, flags=None):
    head = (L.ptr(xyz), xyz.shape[0], L.ptr(tables), L.dtype_code(tables), spec.L, spec.F)
    sm, sc, lay = _layout_args(out)
    if addend is not None:                    # out = bf16(addend + bf16(features)), XCD8 layout only
        assert lay == L.LAYOUT_XCD8 and addend.shape == out.shape and addend.dtype == torch.bfloat16 and addend.is_contiguous()
        _encode_call("fwd_add", spec, feat_scale, flags, head, (L.ptr(addend), out.data_ptr()))
    else:
        _encode_call("fwd", spec, feat_scale, flags, head, (out.data_ptr(), L.dtype_code(out), sm, sc, lay))


BWD_ALGO = "binned"     # "binned": atomic-free two-pass scatter (default); "atomic": per-vertex fp32 global atomics


def _encode_bwd(spec, xyz, grad_out, feat_scale, grad_tables, overwrite=False, flags=None):
    """overwrite: grad_tables is uninitialised memory that the binned reduce pass fills completely (pag_*_encode_bwd_set)."""
    M = xyz.shape[0]
    sm, sc, lay = _layout_args(grad_out)
    ws, ws_ptr, ws_bytes = None, None, 0
    if BWD_ALGO == "binned" or lay == L.LAYOUT_XCD8:
        ws_bytes = L.load().pag_encode_bwd_workspace_bytes(M, spec.L, spec.F, spec.vertices, spec.rows())
        ws = torch.empty(ws_bytes, device=xyz.device, dtype=torch.uint8)
        ws_ptr = ws.data_ptr()
    assert not overwrite or ws_ptr is not None
    _encode_call("bwd_set" if overwrite else "bwd", spec, feat_scale, flags,
                 (L.ptr(xyz), M, grad_out.data_ptr(), L.dtype_code(grad_out), sm, sc, lay, spec.L, spec.F), (L.ptr(grad_tables), ws_ptr, ws_bytes))


def _encode_bwd_xyz(spec, xyz, tables, grad_out, feat_scale, flags=None, rays=None):
    """d loss / d xyz f32 [M,3] (pose optimisation: ba_pipeline.py:85-92) or, with rays = (ridx, depths, pack_start, N), reduced per ray inside the
    gather pass: f32 [N,6] (d origin | d dir)."""
    M = xyz.shape[0]
    sm, sc, lay = _layout_args(grad_out)
    head = (L.ptr(xyz), M, L.ptr(tables), L.dtype_code(tables), grad_out.data_ptr(), L.dtype_code(grad_out), sm, sc, lay, spec.L, spec.F)
    if rays is None:
        out, ws = torch.empty(M, 3, device=xyz.device), torch.empty(8 * M * 3, device=xyz.device)
        _encode_call("bwd_xyz", spec, feat_scale, flags, head, (L.ptr(out), L.ptr(ws), ws.numel() * 4))
    else:
        ridx, depths, pack_start, N = rays
        out = torch.empty(N, 6, device=xyz.device)
        ws_bytes = L.load().pag_encode_bwd_rays_workspace_bytes(max(M, 1), N)
        ws = torch.empty(ws_bytes // 4, device=xyz.device)
        _encode_call("bwd_rays", spec, feat_scale, flags, head, (L.ptr(ridx), L.ptr(depths), L.ptr(pack_start), N, L.ptr(out), L.ptr(ws), ws_bytes))
    return out


def _encode_forward(xyz, tables, spec, feat_scale, out_dtype, feature_major, addend, flags):
    """What the forward of both autograd nodes does: shape check, output allocation, launch -> (xyz as f32 contiguous, the tables contiguous, features)."""
    xyz = xyz.detach().contiguous().float()
    M, C = xyz.shape[0], spec.L * spec.F
    if tables.shape != (spec.L, spec.rows(), spec.F):
        raise RuntimeError("tables shape %s does not match the encoder spec %s" % (tuple(tables.shape), (spec.L, spec.rows(), spec.F)))
    if feature_major == "xcd8":
        out = torch.empty(8, M, 8, device=xyz.device, dtype=torch.bfloat16)
    elif feature_major:
        out = torch.empty(C, M, device=xyz.device, dtype=out_dtype).t()
    else:
        out = torch.empty(M, C, device=xyz.device, dtype=out_dtype)
    tc = tables.detach().contiguous()
    if M:
        _encode_fwd(spec, xyz, tc, feat_scale, out, addend.detach() if addend is not None else None, flags=flags)
    return xyz, tc, out


def _table_grad(ctx, xyz, g):
    """The table gradient of both autograd nodes, in the tables' dtype."""
    M = xyz.shape[0]
    if M and (BWD_ALGO == "binned" or g.dim() == 3):       # the reduce pass writes every row: no zero fill, no read-modify-write
        gt = torch.empty(ctx.tshape, device=xyz.device, dtype=torch.float32)
        _encode_bwd(ctx.spec, xyz, g, ctx.feat_scale, gt, overwrite=True, flags=ctx.flags)
    else:
        gt = torch.zeros(ctx.tshape, device=xyz.device, dtype=torch.float32)
        if M:
            _encode_bwd(ctx.spec, xyz, g, ctx.feat_scale, gt, flags=ctx.flags)
    return gt.to(ctx.tdtype)


class _Encode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, tables, spec, feat_scale, out_dtype, feature_major, addend=None, flags=None):
        _check_gpu(xyz, tables)
        xyz, tc, out = _encode_forward(xyz, tables, spec, feat_scale, out_dtype, feature_major, addend, flags)
        ctx.spec, ctx.feat_scale, ctx.flags = spec, feat_scale, flags
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(xyz, tc)           # d/d xyz needs the table rows again
        else:
            ctx.save_for_backward(xyz)
        ctx.tshape, ctx.tdtype = tables.shape, tables.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        xyz = ctx.saved_tensors[0]
        gt = d_xyz = None
        if g.dtype not in (torch.float32, torch.bfloat16):
            g = g.float()
        if g.dim() == 3:
            g = g.contiguous()
        if ctx.needs_input_grad[1]:
            gt = _table_grad(ctx, xyz, g)
        if ctx.needs_input_grad[0]:
            d_xyz = _encode_bwd_xyz(ctx.spec, xyz, ctx.saved_tensors[1], g, ctx.feat_scale, flags=ctx.flags) if xyz.shape[0] \
                else torch.zeros_like(xyz)
        return d_xyz, gt, None, None, None, None, None, None


RAYS_FUSED = os.environ.get("PAG_RAYS_FUSED", "1") != "0"      # A/B switch: position gradient reduced per ray inside the gather pass (_EncodeRays)


class _EncodeRays(torch.autograd.Function):
    """encode() on samples that come straight from the ray march with a pose gradient attached (ray_samples(): samples = origins[ray] +
    dirs[ray] * depth, pc_nerf/ba_pipeline.py:85-92) as ONE autograd node from (origins, dirs, tables) to the features: what the backward wants of
    d loss / d xyz is its per-ray sum and its per-ray sum weighted by depth, and pag_*_encode_bwd_rays forms both inside the gather pass (6 floats per
    wave and ray leave the kernel instead of 8 x 3 floats per sample - 1.4 GB and two launches less on a dense 24 576-ray step).  The samples
    themselves enter detached: their _RaySamples node receives nothing from here."""

    @staticmethod
    def forward(ctx, origins, dirs, xyz, tables, spec, feat_scale, out_dtype, xcd8, flags, depths, pack_start, ridx):
        _check_gpu(xyz, tables, depths, pack_start, ridx)
        xyz, tc, out = _encode_forward(xyz, tables, spec, feat_scale, out_dtype, "xcd8" if xcd8 else False, None, flags)
        ctx.spec, ctx.feat_scale, ctx.flags, ctx.N = spec, feat_scale, flags, origins.shape[0]
        ctx.save_for_backward(xyz, tc, depths.detach().reshape(-1).float().contiguous(), pack_start, ridx.detach().reshape(-1).contiguous())
        ctx.tshape, ctx.tdtype = tables.shape, tables.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        xyz, tc, depths, pack_start, ridx = ctx.saved_tensors
        if g.dtype not in (torch.float32, torch.bfloat16):
            g = g.float()
        g = g.contiguous()
        gt = d_o = d_d = None
        if ctx.needs_input_grad[3]:
            gt = _table_grad(ctx, xyz, g)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            out = _encode_bwd_xyz(ctx.spec, xyz, tc, g, ctx.feat_scale, flags=ctx.flags, rays=(ridx, depths, pack_start, ctx.N))
            d_o, d_d = out[:, :3], out[:, 3:]
        return d_o, d_d, None, gt, None, None, None, None, None, None, None, None


def encode(xyz, tables, spec, feat_scale=None, out_dtype=torch.float32, feature_major=False, layout=None, addend=None, half_coords=None, rays=None):
    """Grid features [M, L*F] (column = level*F + f); layout="xcd8" returns the bf16 [8, M, 8] XCD-grouped tensor the
    fused decoders consume directly.  Differentiable w.r.t. tables and (when xyz.requires_grad) xyz.
    addend (xcd8 only, treated as a constant): the result is bf16(addend + bf16(features)) in the same launch.
    half_coords: None = as the spec says; True / False override it for this call (forward and both gradients).
    rays = ray_samples()'s tag of xyz (origins, dirs, depths, pack_start, ridx): the position gradient then goes to origins / dirs directly (_EncodeRays)."""
    flags = None if half_coords is None else (L.ENC_HALF_COORDS if half_coords else 0)
    if rays is not None and RAYS_FUSED and addend is None and not feature_major and xyz.requires_grad and torch.is_grad_enabled() and xyz.shape[0]:
        origins, dirs, depths, pack_start, ridx = rays
        if depths.numel() == xyz.shape[0] and ridx.numel() == xyz.shape[0]:
            # (xyz enters detached: as a differentiable input its _RaySamples node would still be run - on materialised zeros - by the engine)
            return _EncodeRays.apply(origins, dirs, xyz.detach(), tables, spec, feat_scale, out_dtype, layout == "xcd8", flags, depths, pack_start, ridx)
    return _apply(_Encode, xyz, tables, spec, feat_scale, out_dtype, "xcd8" if layout == "xcd8" else feature_major, addend, flags)


def xcd8_supported(n_levels, n_feat):
    return ((n_levels + 7) // 8) * n_feat <= 8


def xcd8_level(g, j):
    """Level in slot j of XCD group g (csrc/common.h xcd8_level): even bands of 8 levels ascend with g, odd bands descend."""
    return 8 * j + 7 - g if j & 1 else 8 * j + g


def xcd8_columns(n_levels, n_feat):
    """staged position p = 8*g + e  ->  feature column level*F + f (or -1 for padding), as a list of 64."""
    cols = []
    for p in range(64):
        g, e = p >> 3, p & 7
        j, f = divmod(e, n_feat)
        level = xcd8_level(g, j)
        cols.append(level * n_feat + f if (j < (n_levels + 7) // 8 and level < n_levels) else -1)
    return cols


# ---------------------------------------------------------------------------------------------- MLP
def _mm_f32(a, b):
    """a^T-free helper: a [K,M] @ b [M,N] with fp32 result (bf16 inputs accumulate in fp32)."""
    if a.dtype == torch.float32:
        return a @ b
    try:
        return torch.mm(a, b, out_dtype=torch.float32)
    except (TypeError, RuntimeError):
        return (a @ b).float()


class _InferCtx:
    """Stand-in for the autograd ctx of a Function whose result nobody will differentiate (torch.no_grad(): validation renders, prune): nothing is saved,
    nothing needs a gradient; attributes a forward() parks on the ctx for its backward land on a plain object and die with it."""
    saved_tensors = ()

    def __init__(self, n):
        self.needs_input_grad = (False,) * n

    def save_for_backward(self, *tensors):
        pass

    def mark_non_differentiable(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


def _apply(fn, *args):
    """fn.apply(*args); under torch.no_grad() the forward is called directly with an _InferCtx - torch.autograd.Function.apply costs 10 - 15 us of host time
    per call whether or not a graph is recorded, six to eight of them per forward-only trace (a third of the host side of a validation pack)."""
    if torch.is_grad_enabled():
        return fn.apply(*args)
    return fn.forward(_InferCtx(len(args)), *args)


def _need_grad(*tensors):
    """Will anybody differentiate a decoder called on these inputs now?  Asked by the public wrappers BEFORE Function.apply: inside a Function's forward
    grad mode is always off, and ctx.needs_input_grad / tensor.requires_grad still say True for a parameter inside a no_grad region.  Under
    torch.no_grad() (validation renders, prune) the decoder launches keep nothing for a backward - no hidden activations, no softmax statistics beyond
    what the statistics-only wide head hands to its own compositing launch."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class _Launch:
    """One decoder launch that is PREPARED but not yet issued: it rides in another decoder's call where the library can, else its holder issues it.
    args: the argument struct (None until a decoder parked its launch here); keep: the tensors the struct points into."""
    __slots__ = ("entry", "bare", "args", "M", "keep", "taken", "fused", "out_ptr")

    def __init__(self, entry, bare=False):
        self.entry, self.bare = entry, bare        # bare: park only a launch that writes nothing but its output (all a consumer's launch can carry)
        self.args, self.M, self.keep, self.taken, self.fused, self.out_ptr = None, 0, (), False, False, 0

    def park(self, args, M, keep, fused=False, out_ptr=0):
        self.args, self.M, self.keep, self.fused, self.out_ptr = args, M, keep, fused, out_ptr

    @property
    def pending(self):
        return self.args is not None and not self.taken

    def issue(self):
        if self.pending:
            _call(self.entry, ctypes.byref(self.args), self.M, L.stream())
            self.taken = True


class _DecoderCall:
    """What a public wrapper asks of one decoder launch beyond its tensor operands - the single non-tensor argument handed to Function.apply.
    x2_packs = (pack_start, ray_of_pack): x2_index is constant inside each pack (d/d x2 only).  need_grad: _need_grad() of the wrapper's inputs.
    col0_relu: also write relu(x1[:, 0]) (_ColourDensity).  rank1: the backward will hand over its gradient in rank-1 form (head_composite).
    stats_only: a wide softmax head writes its statistics and last hidden layer, no [M,out] tensor.  composite: HeadCompositeArgs for the per-ray sum in
    the decoder's own launch.  park: the _Launch in which this launch waits instead of being issued.  pair: the parked companion narrow head.
    producer: the parked decoder whose output is this one's x1.  n_rays: N of head_composite()."""
    __slots__ = ("in_dim", "out_act", "mode", "out_dtype", "grouped", "x2_packs", "need_grad", "col0_relu", "rank1", "stats_only", "composite", "park",
                 "pair", "producer", "n_rays")

    def __init__(self, in_dim, out_act, mode, out_dtype, grouped, x2_packs=None, need_grad=False, col0_relu=False, rank1=False, stats_only=False,
                 composite=None, park=None, pair=None, producer=None, n_rays=0):
        self.in_dim, self.out_act, self.mode, self.out_dtype = int(in_dim), out_act, mode, out_dtype
        self.grouped = grouped if grouped is None else tuple(grouped)
        self.x2_packs, self.need_grad, self.col0_relu, self.rank1, self.stats_only = x2_packs, need_grad, col0_relu, rank1, stats_only
        self.composite, self.park, self.pair, self.producer, self.n_rays = composite, park, pair, producer, n_rays


class _DecoderState:
    """What a decoder forward leaves for its backward and for its caller (both families)."""
    __slots__ = ("in_dim", "out_act", "mode", "out_dtype", "grouped", "x2_packs", "needs", "M", "k1", "n_layers", "n_hidden", "has_stats", "bc", "saved",
                 "col0_relu", "composited", "head", "hc", "x1_shape", "x1_dtype")

    def __init__(self, call, needs, M, k1, n_layers, saved, x1):
        self.in_dim, self.out_act, self.mode, self.out_dtype, self.grouped = call.in_dim, call.out_act, call.mode, call.out_dtype, call.grouped
        self.x2_packs = call.x2_packs
        self.needs = (bool(needs[0]), bool(needs[1]))      # does x1 / x2 need a gradient?
        self.M, self.k1, self.n_layers, self.saved = M, k1, n_layers, saved      # saved: the tensors of the backward, until an autograd ctx takes them
        self.x1_shape, self.x1_dtype = tuple(x1.shape), x1.dtype
        self.n_hidden, self.has_stats, self.bc = 0, False, None
        self.col0_relu = None          # f32 [M] relu(x1[:, 0]) where the launch wrote it
        self.composited = False        # the launch formed the per-ray sums itself (call.composite)
        self.head = None               # statistics-only head: (last hidden layer, W_last, b_last, statistics) for the compositing launch
        self.hc = None                 # head_composite: (weights, alpha, ridx) of the rank-1 gradient


def _save(ctx, st):
    """Hand the state's tensors to the autograd ctx (saved tensors) and the rest to ctx.state."""
    ctx.save_for_backward(*st.saved)
    st.saved = None
    ctx.state, ctx.x2_packs = st, st.x2_packs      # x2_packs also on the node itself: out.grad_fn.x2_packs says whether d x2 will take the segmented sum


def _operands(x1, x2, x2_index, Ws, bs, grouped):
    """The decoders' operands as the kernels read them -> (x1 f32 / bf16, x2 f32, x2_index i32, W f32, b f32, M, k1), detached and contiguous."""
    _check_gpu(x1, x2, x2_index, *Ws, *bs)
    if grouped is not None:
        M, k1 = x1.shape[1], 64
    else:
        M, k1 = x1.shape
    x1 = x1.detach()
    if not x1.is_contiguous():
        x1 = x1.contiguous()
    if x1.dtype not in (torch.float32, torch.bfloat16):
        x1 = x1.float()
    if x2 is not None:
        x2 = x2.detach().contiguous().float()
        x2_index = x2_index.detach().contiguous()
        if x2_index.dtype != torch.int32:
            x2_index = x2_index.int()
    return x1, x2, x2_index, [w.detach().contiguous().float() for w in Ws], [b.detach().contiguous().float() for b in bs], M, k1


def _fill_shape(a, k1, in_dim, out_dim, out_act, out_dtype, grouped):
    """The shape fields the four decoder argument structs share by name - plain ints and dtypes, no tensor needed."""
    a.k1, a.in_dim, a.out_dim, a.out_act, a.out_dtype = k1, in_dim, out_dim, out_act, L._DT[out_dtype]
    if grouped is not None:
        a.x1_layout, a.x1_levels, a.x1_feats = L.LAYOUT_XCD8, grouped[0], grouped[1]


def _fill_operands(a, x1=None, x2=None, x2_index=None, W=(), b=()):
    """The operand pointers the decoder argument structs share by name (those given)."""
    if x1 is not None:
        a.x1, a.x1_dtype = L.ptr(x1), L.dtype_code(x1)
    if x2 is not None:
        a.x2, a.k2p, a.x2_index = L.ptr(x2), x2.shape[1], L.ptr(x2_index)
    for i, w in enumerate(W):
        a.W[i] = L.ptr(w)
    for i, v in enumerate(b):
        a.b[i] = L.ptr(v)


def _dx2(x2, x2_index, x2_packs, dz0, w_tail, seg=None):
    """d x2[r] = (sum of dz_0 over the samples that gathered row r) @ w_tail, w_tail = W_0[:, k1:in_dim] - the per-ray view embedding's gradient (pose
    optimisation: the view direction depends on the camera rotation, ba_pipeline.py:89-90).  seg: the per-row sums where the caller already has them.
    With x2_packs (the tracer's calls) the sum is the segmented-sum launch, in a fixed order; without them it is index_add_, whose float atomics make
    d x2 - and only d x2: d x1, dW and db never pass through an atomic - differ in the last bits from run to run."""
    R, dev = x2.shape[0], x2.device
    if seg is not None:
        pass
    elif x2_packs is not None:                 # rows gathered pack by pack: one segmented-sum launch (deterministic)
        pack_start, ray_of_pack = x2_packs
        seg = composite_feats(dz0, torch.ones(dz0.shape[0], device=dev), torch.ones(R, device=dev), pack_start, ray_of_pack, R)
    else:
        seg = torch.zeros(R, dz0.shape[1], device=dev).index_add_(0, x2_index.long(), dz0.float())
    dx2 = torch.zeros_like(x2)
    dx2[:, :w_tail.shape[1]] = seg @ w_tail
    return dx2


_NON_NULL = 1      # stands for a tensor that does not exist yet: pag_mlp_bwd_fused_supported() tests pointers for NULL only
_BWD_FUSABLE = {}      # decoder shape -> the library's answer (a pure function of the shape: the struct is built once per shape, not in every eager forward)


def _bwd_fusable(M, x1_dtype, needs, k1, k2p, in_dim, n_layers, out_dim, out_act, out_dtype, mode, grouped, rank1=False, has_stats=False,
                 stats_only=False, col0=False):
    """Forward-time question: will the backward of this decoder be one of the fused kernels (pag_mlp_bwd with wgrad_workspace), which recompute the
    hidden activations, so that the forward need not write them?  Answered by the library's own rule (pag_mlp_bwd_fused_supported, host only) on the
    backward's argument struct as it WILL be filled: a dense gradient or (rank1) g_ray / g_scale / g_index / g_ray_scale; has_stats: the softmax
    statistics tensor is allocated; stats_only: no `out`; col0: the launch writes relu(x1[:, 0]), so the backward gets dx1_col0_add and _gate.
    What the library cannot know stays here: the switch, the batch bound, whether d x1 is wanted, and d x2 with a grouped input (only the colour-like
    kernel hands out dz_0 for the per-ray input's gradient).  A mismatch that still slips through (a _ColourDensity backward that receives no sigma
    gradient) takes _recompute_hidden(), which is correct but costs a second forward - it warns once."""
    if not (WGRAD_FUSED and 0 < M <= L.MLP_FUSED_WIDE_MAX_M and needs[0]) or (needs[1] and grouped is not None):
        return False
    key = (x1_dtype, k1, k2p, in_dim, n_layers, out_dim, out_act, out_dtype, mode, grouped, rank1, has_stats, stats_only, col0)
    if key in _BWD_FUSABLE:
        return _BWD_FUSABLE[key]
    a = L.MlpBwdArgs()
    _fill_shape(a, k1, in_dim, out_dim, out_act, out_dtype, grouped)
    a.n_layers, a.mode = n_layers, mode
    a.x1, a.x1_dtype, a.dx1, a.dx1_dtype = _NON_NULL, L._DT[x1_dtype], _NON_NULL, L._DT[x1_dtype]
    if k2p:
        a.x2, a.k2p, a.x2_index = _NON_NULL, k2p, _NON_NULL
    if rank1:
        a.g_ray = a.g_scale = a.g_index = a.g_ray_scale = _NON_NULL
    else:
        a.grad_out = _NON_NULL
    if has_stats:
        a.softmax_stats = a.b_last = _NON_NULL
    if col0:
        a.dx1_col0_add = a.dx1_col0_gate = _NON_NULL
    if not stats_only:
        a.out = _NON_NULL
    _BWD_FUSABLE[key] = L.load().pag_mlp_bwd_fused_supported(ctypes.byref(a)) == 1
    return _BWD_FUSABLE[key]


_WARNED_RECOMPUTE = False


def _recompute_hidden(st, x1, x2, x2_index, Wc, hidden):
    """Fill the missing entries of `hidden` by re-running the forward (pag_mlp_fwd with hidden_save) - the fallback for a backward
    that the fused kernels cannot serve although the forward did not save the activations."""
    global _WARNED_RECOMPUTE
    if not _WARNED_RECOMPUTE:
        _WARNED_RECOMPUTE = True
        import warnings
        warnings.warn("pagnerf_amd: a decoder backward could not use the fused kernels although its forward skipped the hidden activations; "
                      "re-running the forward for them (correct, but one extra launch and an [M, out] scratch per backward)")
    M, dev = st.M, x1.device
    full = [h if h is not None else torch.empty(M, 64, device=dev, dtype=torch.bfloat16 if st.mode == L.MLP_MFMA_BF16 else torch.float32) for h in hidden]
    out_dim = Wc[-1].shape[0]
    scratch = torch.empty(M, out_dim, device=dev, dtype=torch.bfloat16)
    a = L.MlpFwdArgs()
    _fill_shape(a, st.k1, st.in_dim, out_dim, L.ACT_NONE, torch.bfloat16, st.grouped)
    _fill_operands(a, x1, x2, x2_index, Wc, st.bc)
    a.n_layers, a.mode, a.out = st.n_layers, st.mode, L.ptr(scratch)
    for i, h in enumerate(full):
        a.hidden_save[i] = L.ptr(h)
    _call("pag_mlp_fwd", ctypes.byref(a), M, L.stream())
    return full


def _mlp_forward(call, needs, x1, x2, x2_index, *wb):
    """The 64-wide decoders' forward (pag_mlp_fwd).  needs = (x1 needs a gradient, x2 needs one) -> (out | None, _DecoderState)."""
    lib = L.load()
    n_layers = len(wb) // 2
    x1, x2, x2_index, Wc, bc, M, k1 = _operands(x1, x2, x2_index, wb[:n_layers], wb[n_layers:], call.grouped)
    in_dim, out_act, mode, out_dtype, grouped, need_grad = call.in_dim, call.out_act, call.mode, call.out_dtype, call.grouped, call.need_grad
    dev, out_dim = x1.device, Wc[-1].shape[0]
    mfma = mode == L.MLP_MFMA_BF16
    wide_softmax = mfma and out_act == L.ACT_SOFTMAX and out_dim > 64 and out_dtype == torch.bfloat16
    stats_only = call.stats_only and wide_softmax       # head_composite: no [M,out] tensor at all
    # wide softmax heads: per-sample (max*log2e, 1/sum) lets the backward rebuild the probabilities from the saved
    # hidden layer instead of streaming `out` through twice (pag_mlp_bwd_args.softmax_stats)
    has_stats = wide_softmax and (need_grad or stats_only)
    col0 = bool(call.col0_relu and mfma and grouped is None and x1.dtype == torch.bfloat16 and out_dim <= 64 and M)
    out = None if stats_only else torch.empty(M, out_dim, device=dev, dtype=out_dtype)
    # The fused backward kernels RECOMPUTE the hidden activations from x1 (bit-identical MFMA sequence), so the forward of a
    # decoder they will serve does not write them: 268 MB per hidden layer at M = 2.1 M, in launches that run at the HBM rate.
    # Wide head: the LAST hidden layer is kept (the probabilities are rebuilt from it).  A backward that turns out not to be
    # fusable (no column-0 gradient, d x2 requested, ...) re-runs the forward for them (_recompute_hidden: rare, slow, correct).
    recompute = need_grad and _bwd_fusable(M, x1.dtype, needs, k1, x2.shape[1] if x2 is not None else 0, in_dim, n_layers, out_dim, out_act, out_dtype,
                                           mode, grouped, call.rank1, has_stats, stats_only, col0)
    hidden = []
    if need_grad or stats_only:
        for i in range(n_layers - 1):
            keep = (need_grad and not recompute) or (stats_only and i == n_layers - 2)
            hidden.append(torch.empty(M, 64, device=dev, dtype=torch.bfloat16 if mfma else torch.float32) if keep else None)
    a = L.MlpFwdArgs()
    _fill_shape(a, k1, in_dim, out_dim, out_act, out_dtype, grouped)
    _fill_operands(a, x1, x2, x2_index, Wc, bc)
    a.n_layers, a.mode, a.out = n_layers, mode, L.ptr(out)
    for i, h in enumerate(hidden):
        a.hidden_save[i] = L.ptr(h)
    stats = torch.empty(M, 2, device=dev) if has_stats else None
    a.softmax_stats = L.ptr(stats)
    st = _DecoderState(call, needs, M, k1, n_layers, (x1, x2, x2_index, out, *hidden, *Wc, *((stats, bc[-1]) if has_stats else ())), x1)
    st.n_hidden, st.has_stats, st.bc = len(hidden), has_stats, bc
    if col0:
        st.col0_relu = torch.empty(M, device=dev)           # _ColourDensity: sigma from the same launch
        a.x1_col0_relu = L.ptr(st.col0_relu)
    if stats_only:
        st.head = (hidden[-1], Wc[-1], bc[-1], stats)
    park = call.park
    if park is not None and park.bare and not (mfma and all(t is None for t in hidden) and stats is None and not col0):
        park = None                              # nothing a consumer's launch could carry: issue it now
    producer = call.producer
    if producer is not None:
        # the decoder whose output is this one's x1 waits in `producer`: in this launch where the library can (pag_mlp_fwd_args.x1_producer),
        # else its own launch FIRST
        if producer.pending and M and x1.data_ptr() == producer.out_ptr \
                and lib.pag_mlp_fwd_producer_supported(ctypes.byref(a), ctypes.byref(producer.args), M) == 1:
            a.x1_producer = ctypes.pointer(producer.args)
            producer.taken = True
        else:
            producer.issue()
    if M and park is not None:
        park.park(a, M, [x1, x2, x2_index, out, stats, st.col0_relu, *hidden, *Wc, *bc], out_ptr=out.data_ptr() if out is not None else 0)
    elif M:
        # A pair of decoders on one input (head_composite_pair): the narrow one's launch is PREPARED and parked (its call.park) and rides
        # in the wide one's call (call.pair -> pag_mlp_fwd_args.pair) where the library can; else the caller issues it.
        pair = call.pair
        if pair is not None and pair.pending and M <= L.MLP_FUSED_WIDE_MAX_M and lib.pag_mlp_fwd_pair_supported(ctypes.byref(a), ctypes.byref(pair.args)) == 1:
            a.pair = ctypes.pointer(pair.args)
            pair.taken = True
        # head_composite: the per-ray weighted sum in the decoder's own launch, one pass over the logits (pag_mlp_fwd_args.composite)
        if call.composite is not None and HEAD_FWD_ONCE and stats_only and lib.pag_mlp_fwd_composite_supported(ctypes.byref(a), M) == 1:
            a.composite = ctypes.pointer(call.composite)
            st.composited = True
        _call("pag_mlp_fwd", ctypes.byref(a), M, L.stream())
    return out, st


def _mlp_backward(st, saved, g, rank1=None, dx1_into=None, dx1_out=None, col0_add=None, col0_gate=None, wgrad_queue=None, hold=None, pair=None):
    """The 64-wide decoders' backward (pag_mlp_bwd) -> (d x1, d x2, [dW], [db]).
    rank1 = (g_ray f32 [N,out], g_scale f32 [M], g_index i32 [M], g_ray_scale f32 [N]) replaces the dense upstream gradient g.
    dx1_into: an XCD8 gradient tensor of another decoder on the same input - this one's d x1 is added to it in place.
    dx1_out: write d x1 into this tensor instead of a new one.
    hold (_Launch): a fused launch is PREPARED, not issued - args and everything they point to are parked there, to ride in the
    call of the other decoder of a pair (pair = that _Launch; pag_mlp_bwd_args.pair) or to be issued by the caller."""
    lib = L.load()
    in_dim, out_act, mode, out_dtype, grouped, n_layers, k1, M = st.in_dim, st.out_act, st.mode, st.out_dtype, st.grouped, st.n_layers, st.k1, st.M
    x1, x2, x2_index, out = saved[:4]
    hidden = list(saved[4:4 + st.n_hidden])
    Wc = list(saved[4 + st.n_hidden:4 + st.n_hidden + n_layers])
    stats, b_last = (saved[-2], saved[-1]) if st.has_stats else (None, None)
    out_dim = Wc[-1].shape[0]
    dev = x1.device
    zdt = torch.bfloat16 if mode == L.MLP_MFMA_BF16 else torch.float32
    need_dx = st.needs[0]
    need_dx2 = st.needs[1] and x2 is not None
    dx1 = (dx1_into if dx1_into is not None else (dx1_out if dx1_out is not None else torch.empty(x1.shape, device=dev, dtype=x1.dtype))) \
        if need_dx else None
    a = L.MlpBwdArgs()
    if rank1 is None:
        g = g.contiguous().to(out_dtype)       # grad_out travels in the output's dtype
        a.grad_out = L.ptr(g)
    else:
        a.g_ray, a.g_scale, a.g_index, a.g_ray_scale = (L.ptr(t) for t in rank1)
    _fill_shape(a, k1, in_dim, out_dim, out_act, out_dtype, grouped)
    _fill_operands(a, W=Wc, b=st.bc)
    a.out, a.n_layers, a.mode = L.ptr(out), n_layers, mode
    a.dx1, a.dx1_dtype = L.ptr(dx1), (L.dtype_code(dx1) if need_dx else 0)
    a.softmax_stats, a.b_last = L.ptr(stats), L.ptr(b_last)
    a.dx1_accumulate = 1 if (need_dx and dx1_into is not None) else 0
    fuse_col0 = col0_add is not None and need_dx and grouped is None and mode == L.MLP_MFMA_BF16 and out_dim <= 64
    if col0_gate is not None and not fuse_col0:          # the gate only exists on the fused path's preconditions
        col0_add, col0_gate = col0_add * (col0_gate > 0), None
    if fuse_col0:
        a.dx1_col0_add = L.ptr(col0_add)
        if col0_gate is not None:
            a.dx1_col0_gate = L.ptr(col0_gate)
    # Weight gradients inside the backward-data launch (pag_mlp_bwd_args.wgrad_workspace) where the library has a fused
    # kernel for this decoder shape: no dz tensors, no second pass over the activations.  d x2 (pose optimisation) is formed
    # from dz_0, so that case keeps the dz tensors and the separate weight-gradient launches.
    fused = False
    dz0_fused = dz0_slots = ws = None
    if WGRAD_FUSED and 0 < M <= L.MLP_FUSED_WIDE_MAX_M and mode == L.MLP_MFMA_BF16 and x1.dtype == torch.bfloat16 \
            and (not need_dx2 or grouped is None):
        _fill_operands(a, x1, x2, x2_index)
        fused = lib.pag_mlp_bwd_fused_supported(ctypes.byref(a)) == 1
        if fused and need_dx2:        # colour-like kernel: d x2 is formed from dz_0 below
            packs = st.x2_packs
            if DZ0_SLOTS and packs is not None and _one_pack_per_ray(packs[1], x2.shape[0]) and packs[0].shape[0] == x2.shape[0] + 1:
                # samples packed ray by ray (x2_index non-decreasing): the per-ray sum of dz_0 starts inside the kernel - one 64-float row per
                # (tile, ray) instead of the [M,64] tensor (pag_mlp_bwd_args.dz0_slots)
                dz0_slots = torch.empty(lib.pag_mlp_dz0_slots_bytes(M, x2.shape[0]) // 4, device=dev)
                a.dz0_slots = L.ptr(dz0_slots)
            else:                     # dz_0 comes out as a tensor (pag_mlp_bwd_args.dz[0])
                dz0_fused = torch.empty(M, 64, device=dev, dtype=torch.bfloat16)
                a.dz[0] = L.ptr(dz0_fused)
    if not fused and any(h is None for h in hidden):      # the forward counted on the fused kernels: rebuild what it skipped
        hidden = _recompute_hidden(st, x1, x2, x2_index, Wc, hidden)
    for i, h in enumerate(hidden):
        a.hidden_save[i] = L.ptr(h)
    dz = None
    gW, gb = [], []
    if fused:
        ws_bytes = lib.pag_mlp_bwd_fused_workspace_bytes(ctypes.byref(a), M)
        ws = torch.empty(ws_bytes // 4, device=dev)
        a.wgrad_workspace, a.wgrad_workspace_bytes = L.ptr(ws), ws_bytes
        for l in range(n_layers):
            gW.append(torch.empty(Wc[l].shape[0], in_dim if l == 0 else 64, device=dev))
            gb.append(torch.empty(Wc[l].shape[0], device=dev))
            a.dW[l], a.db[l] = L.ptr(gW[l]), L.ptr(gb[l])
    else:
        dz = [torch.empty(M, 64, device=dev, dtype=zdt) for _ in range(n_layers - 1)] + [torch.empty(M, out_dim, device=dev, dtype=zdt)]
        for i in range(n_layers):
            a.dz[i] = L.ptr(dz[i])
    if M and hold is not None:       # issued later: inside the pair's other call or by the caller
        hold.park(a, M, [x1, x2, x2_index, out, stats, b_last, g, dx1, col0_add, col0_gate, dz0_slots, dz0_fused, ws, *(rank1 or ()), *hidden, *Wc, *gW,
                         *gb, *(dz or ())], fused=fused)
    elif M:
        if pair is not None and fused and pair.pending and pair.fused and lib.pag_mlp_bwd_pair_supported(ctypes.byref(a), ctypes.byref(pair.args)) == 1:
            a.pair = ctypes.pointer(pair.args)
            pair.taken = True
        _call("pag_mlp_bwd", ctypes.byref(a), M, L.stream())
    if col0_add is not None and need_dx and not fuse_col0:
        dx1[:, 0] += col0_add.to(dx1.dtype)          # parity path: same sum with torch ops
    if fused:
        pass
    elif mode == L.MLP_MFMA_BF16 and M:
        # weight gradients on the matrix cores: per-workgroup fp32 slabs, summed here (deterministic)
        specs = []
        for l in range(n_layers):
            n_out = Wc[l].shape[0]
            sp = dict(dz=dz[l], n_out=n_out, a2=None, k2p=0, a2_index=None, levels=0, feats=0)
            if l == 0 and grouped is not None:
                sp.update(a1=x1, a1_dtype=L.BF16, a1_layout=L.LAYOUT_XCD8, k1=64, n_in=64, levels=grouped[0], feats=grouped[1])
            elif l == 0:
                sp.update(a1=x1, a1_dtype=L.dtype_code(x1), a1_layout=L.LAYOUT_STRIDED, k1=k1, n_in=in_dim,
                          a2=x2, k2p=(x2.shape[1] if x2 is not None else 0), a2_index=x2_index)
            else:
                sp.update(a1=hidden[l - 1], a1_dtype=L.BF16, a1_layout=L.LAYOUT_STRIDED, k1=64, n_in=64)
            sp["w"] = torch.empty(n_out, in_dim if l == 0 else 64, device=dev)
            sp["b"] = torch.empty(n_out, device=dev)
            gW.append(sp["w"])
            gb.append(sp["b"])
            specs.append(sp)
        if wgrad_queue is not None:
            wgrad_queue.extend(specs)          # the caller launches several decoders' weight gradients together
        else:
            _launch_wgrad(specs, M)
    else:
        # fp32 parity path: dz_l^T @ input_l as plain fp32 GEMMs (BLAS)
        for l in range(n_layers):
            z = dz[l]
            if l == 0:
                n1 = min(k1, in_dim)
                w = _mm_f32(z.t(), x1[:, :n1].to(z.dtype))
                if in_dim > k1:
                    seg = torch.zeros(x2.shape[0], 64, device=dev, dtype=torch.float32)
                    seg.index_add_(0, x2_index.long(), z.float())
                    w = torch.cat([w, seg.t() @ x2[:, :in_dim - k1]], dim=1)
            else:
                w = _mm_f32(z.t(), hidden[l - 1])
            gW.append(w)
            gb.append(z.sum(0, dtype=torch.float32))
    dx2 = None
    if need_dx2:
        R, seg = x2.shape[0], None
        if dz0_slots is not None and M:                # the kernel left per-(tile, ray) sums: add each ray's rows
            seg = torch.empty(R, 64, device=dev)
            _call("pag_mlp_dz0_slots_sum", L.ptr(st.x2_packs[0]), R, L.ptr(dz0_slots), L.ptr(seg), L.stream())
        elif M == 0:
            seg = torch.zeros(R, 64, device=dev)
        dx2 = _dx2(x2, x2_index, st.x2_packs, dz0_fused if dz0_fused is not None else dz[0] if dz else None, Wc[0][:, k1:in_dim], seg)
    return dx1, dx2, gW, gb


DZ0_SLOTS = os.environ.get("PAG_DZ0_SLOTS", "1") != "0"      # A/B switch: per-(tile, ray) sums of dz_0 inside the colour backward (pag_mlp_bwd_args.dz0_slots)
WGRAD_MAX_BATCH = 6      # WG_MAX_BATCH of csrc/mlp_common.h
WGRAD_FUSED = os.environ.get("PAG_NO_FUSED_WGRAD") is None      # narrow decoders: weight gradients inside pag_mlp_bwd (no dz tensors)


def _launch_wgrad(specs, M):
    """Weight / bias gradients of the given decoder layers (dicts built by _FusedMLP._backward_impl; all over the same M samples)
    through pag_mlp_wgrad_batch: the narrow layers share ONE slab launch (grid.y = layer) whose ~1024 workgroups - one wave of
    workgroups on the chip; a second, partial wave cost 10 % - are split between them; one finish launch sums every layer's slabs."""
    lib = L.load()
    nblk_max = lib.pag_mlp_wgrad_blocks(M)
    for c0 in range(0, len(specs), WGRAD_MAX_BATCH):
        part = specs[c0:c0 + WGRAD_MAX_BATCH]
        n_narrow = max(1, sum(1 for sp in part if sp["n_out"] <= 64))
        layers = (L.WgradLayer * len(part))()
        keep = []
        for y, sp in zip(layers, part):
            n_out = sp["n_out"]
            nblk = max(1, nblk_max // n_narrow) if n_out <= 64 else min(nblk_max, 512)      # wide layers: fewer, larger slabs
            slabs = torch.empty(nblk, (n_out + 31) // 32 * 32, 96, device=sp["dz"].device)
            keep.append(slabs)
            y.dz, y.dz_cols, y.n_out = L.ptr(sp["dz"]), sp["dz"].shape[1], n_out
            y.a1, y.a1_dtype, y.a1_layout, y.k1, y.n_in = L.ptr(sp["a1"]), sp["a1_dtype"], sp["a1_layout"], sp["k1"], sp["n_in"]
            y.a2, y.k2p, y.a2_index = L.ptr(sp["a2"]), sp["k2p"], L.ptr(sp["a2_index"])
            y.a1_levels, y.a1_feats = sp["levels"], sp["feats"]
            y.slabs, y.n_blocks, y.dW, y.db = L.ptr(slabs), nblk, L.ptr(sp["w"]), L.ptr(sp["b"])
        _call("pag_mlp_wgrad_batch", layers, len(part), M, L.stream())


class _AffineXCD8(torch.autograd.Function):
    """out f32 [M, n_out] = x . W^T + b on the encoders' bf16 [8, M, 8] features (pag_affine_xcd8_fwd); backward: d x in the same
    layout (pag_affine_xcd8_bwd_dx), d W / d b through the decoders' weight-gradient kernels (pag_mlp_wgrad_batch)."""

    @staticmethod
    def forward(ctx, x8, W, b, grouped):
        _check_gpu(x8, W, b)
        M, (n_out, in_dim) = x8.shape[1], W.shape
        Wc, bc = W.detach().float().contiguous(), b.detach().float().contiguous()
        out = torch.empty(M, n_out, device=x8.device)
        _call("pag_affine_xcd8_fwd", L.ptr(x8), M, grouped[0], grouped[1], L.ptr(Wc), L.ptr(bc), n_out, in_dim, L.ptr(out), L.stream())
        ctx.save_for_backward(x8, Wc)
        ctx.grouped = grouped
        return out

    @staticmethod
    def backward(ctx, g):
        x8, Wc = ctx.saved_tensors
        M, (n_out, in_dim) = x8.shape[1], Wc.shape
        g = g.float().contiguous()
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x8)
            _call("pag_affine_xcd8_bwd_dx", L.ptr(g), M, ctx.grouped[0], ctx.grouped[1], L.ptr(Wc), n_out, in_dim, L.ptr(dx), L.stream())
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dW, db = torch.empty(n_out, in_dim, device=g.device), torch.empty(n_out, device=g.device)
            if M:
                _launch_wgrad([dict(dz=g.to(torch.bfloat16), n_out=n_out, a1=x8, a1_dtype=L.BF16, a1_layout=L.LAYOUT_XCD8, k1=64, n_in=64,
                                    a2=None, k2p=0, a2_index=None, levels=ctx.grouped[0], feats=ctx.grouped[1], w=dW, b=db)], M)
            else:
                dW.zero_(), db.zero_()
        return dx, dW, db, None


def affine_xcd8(x8, W, b, grouped):
    """x8 bf16 [8, M, 8] (grouped = (levels, feats)), W [n_out, levels*feats], b [n_out] -> f32 [M, n_out]."""
    return _AffineXCD8.apply(x8, W, b, grouped)


def _decoder_grads(grads):
    """(d x1, d x2, [dW], [db]) -> the backward's return for the inputs (call, x1, x2, x2_index, *W, *b)."""
    dx1, dx2, gW, gb = grads
    return (None, dx1, dx2, None, *gW, *gb)


class _FusedMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, call, x1, x2, x2_index, *wb):
        out, st = _mlp_forward(call, ctx.needs_input_grad[1:3], x1, x2, x2_index, *wb)
        _save(ctx, st)
        return out

    @staticmethod
    def backward(ctx, g):
        return _decoder_grads(_mlp_backward(ctx.state, ctx.saved_tensors, g))


class _ColourDensity(torch.autograd.Function):
    """The colour decoder on cat(density_feats, PE) AND the density sigma = relu(density_feats[:, 0]) that
    pc_nerf/panoptic_delta_nef.py:188 reads off its x1, as one autograd node: the gradient of sigma is added to column 0 of
    the decoder's d x1 inside the backward kernel - no zero-padded [M,16] gradient, slice / cast / relu backward or add pass."""

    @staticmethod
    def forward(ctx, call, x1, x2, x2_index, *wb):
        rgb, st = _mlp_forward(call, ctx.needs_input_grad[1:3], x1, x2, x2_index, *wb)
        _save(ctx, st)
        ctx.pre = None
        if st.col0_relu is not None:            # written by the decoder launch; the backward gates on it inside the kernel
            return rgb, st.col0_relu
        ctx.pre = x1.detach()[:, 0].float()
        return rgb, torch.relu(ctx.pre)

    @staticmethod
    def backward(ctx, g_rgb, g_sigma):
        st, saved = ctx.state, ctx.saved_tensors
        if g_rgb is None:
            g_rgb = torch.zeros_like(saved[3])
        if g_sigma is None:
            return _decoder_grads(_mlp_backward(st, saved, g_rgb))
        if ctx.pre is None:
            return _decoder_grads(_mlp_backward(st, saved, g_rgb, col0_add=g_sigma.float().contiguous(), col0_gate=st.col0_relu))
        return _decoder_grads(_mlp_backward(st, saved, g_rgb, col0_add=(g_sigma.float() * (ctx.pre > 0)).contiguous()))


def colour_and_density(x1, weights, biases, x2, x2_index, in_dim, out_act=L.ACT_SIGMOID, mode=L.MLP_MFMA_BF16,
                       out_dtype=torch.float32, x2_packs=None, producer=None):
    """-> (rgb [M,3], sigma f32 [M] = relu(x1[:,0])); x1 = the density decoder's [M,16] output (see _ColourDensity).
    producer: the decoder_hold() in which the density decoder's launch waits - evaluated in this decoder's launch where the library can."""
    call = _DecoderCall(in_dim, out_act, mode, out_dtype, None, x2_packs=x2_packs, need_grad=_need_grad(x1, x2, x2_index, *weights, *biases),
                        col0_relu=True, producer=producer)
    return _apply(_ColourDensity, call, x1, x2, x2_index, *weights, *biases)


def fused_mlp(x1, weights, biases, x2=None, x2_index=None, in_dim=None, out_act=L.ACT_NONE, mode=L.MLP_MFMA_BF16,
              out_dtype=torch.float32, x1_grouped=None, x2_packs=None, hold=None):
    """wisp BasicDecoder (Linear+ReLU ... Linear) [+ sigmoid/softmax] in one launch.
    x1 [M,k1] (+ optional per-ray x2 [R,k2p] gathered by x2_index [M]); weights[i] is [out,in].
    x1_grouped=(levels, feats): x1 is the encoders' bf16 [8, M, 8] XCD-grouped tensor.
    x2_packs=(pack_start, ray_of_pack): x2_index is constant inside each pack (d/d x2 only).
    hold: a decoder_hold() - the launch is prepared and parked there for the decoder that consumes its output."""
    if in_dim is None:
        in_dim = weights[0].shape[1]
    call = _DecoderCall(in_dim, out_act, mode, out_dtype, x1_grouped, x2_packs=x2_packs, need_grad=_need_grad(x1, x2, x2_index, *weights, *biases),
                        park=hold)
    return _apply(_FusedMLP, call, x1, x2, x2_index, *weights, *biases)


# ----------------------------------------------------------------------------- 128-wide decoders
def wide_mlp_reference(x, W, b, out_act=L.ACT_NONE, round_bf16=False):
    """The DEFINITION of the 128-wide decoders (pag_mlp128_fwd) in tensor ops, on any device: Linear + ReLU ... Linear [+ sigmoid / softmax].
    round_bf16: the input, the weights and the hidden activations are rounded to bf16 straight-through (the kernels' rounding points; sums,
    biases and the output activation stay f32) - at width 128 this is also the precision='fp32' / CPU path of nef.BasicDecoder."""
    def r(t):
        return t + (t.detach().bfloat16().to(t.dtype) - t.detach()) if round_bf16 else t
    h = r(x)
    for i in range(len(W)):
        h = torch.nn.functional.linear(h, r(W[i]), None if b[i] is None else b[i])
        if i + 1 < len(W):
            h = r(torch.relu(h))
    if out_act == L.ACT_SIGMOID:
        h = torch.sigmoid(h)
    elif out_act == L.ACT_SOFTMAX:
        h = torch.softmax(h, -1)
    return h


def _native_plane(ws, col0, width, M):
    """Columns [col0, col0 + width) of a pag_mlp128 workspace (uint8 tensor of "native" bf16 planes, include/pagnerf_hip.h) as a bf16 [M, width] tensor."""
    Mp = (M + L.MLP128_BATCH - 1) // L.MLP128_BATCH * L.MLP128_BATCH
    p = ws.view(torch.bfloat16)[Mp * col0:Mp * (col0 + width)].view(Mp // 32, width // 32, 4, 2, 32, 4)     # tile, block, g, lane half, sample, value
    return p.permute(0, 4, 1, 2, 3, 5).reshape(Mp, width)[:M]


def _mlp128_forward(call, needs, x1, x2, x2_index, *wb):
    """The 128-wide decoders' forward (pag_mlp128_fwd) -> (out, _DecoderState)."""
    n_hidden = len(wb) // 2 - 1
    if any(v is None for v in wb[n_hidden + 1:]):
        raise NotImplementedError("fused_mlp128 needs biases")
    x1, x2, x2_index, Wc, bc, M, k1 = _operands(x1, x2, x2_index, wb[:n_hidden + 1], wb[n_hidden + 1:], call.grouped)
    out_dim = Wc[-1].shape[0]
    out = torch.empty(M, out_dim, device=x1.device, dtype=call.out_dtype)
    a = L.Mlp128FwdArgs()
    _fill_shape(a, k1, call.in_dim, out_dim, call.out_act, call.out_dtype, call.grouped)
    _fill_operands(a, x1, x2, x2_index, Wc, bc)
    a.n_hidden, a.hidden, a.out = n_hidden, Wc[0].shape[0], L.ptr(out)
    ws = None
    if call.need_grad and M:          # under torch.no_grad() nothing is saved and no workspace is asked for
        nbytes = L.load().pag_mlp128_workspace_bytes(M, n_hidden, out_dim, 1)
        L.check(min(nbytes, 0), "pag_mlp128_workspace_bytes")
        ws = torch.empty(nbytes, device=x1.device, dtype=torch.uint8)
        a.workspace, a.workspace_bytes = L.ptr(ws), nbytes
    if M:
        _call("pag_mlp128_fwd", ctypes.byref(a), M, L.stream())
    return out, _DecoderState(call, needs, M, k1, n_hidden + 1, (x2, x2_index, out, ws, *Wc), x1)


def _mlp128_backward(st, saved, g, dx1_into=None):
    """The 128-wide decoders' backward (pag_mlp128_bwd) -> (d x1, d x2, [dW], [db]).
    dx1_into: an XCD8 gradient tensor of another decoder on the same input - this one's d x1 is added to it in place."""
    in_dim, out_dtype, k1, M, n_hidden = st.in_dim, st.out_dtype, st.k1, st.M, st.n_layers - 1
    x2, x2_index, out, ws = saved[:4]
    Wc = list(saved[4:])
    dev, out_dim = out.device, out.shape[1]
    need_dx = st.needs[0]
    need_dx2 = st.needs[1] and x2 is not None
    dx1 = (dx1_into if dx1_into is not None else torch.empty(st.x1_shape, device=dev, dtype=st.x1_dtype)) if need_dx else None
    gW = [torch.empty_like(w) for w in Wc]
    gb = [torch.empty(w.shape[0], device=dev) for w in Wc]
    if M == 0:
        for t in gW + gb:
            t.zero_()
        return dx1, (torch.zeros_like(x2) if need_dx2 else None), gW, gb
    g = g.contiguous().to(out_dtype)       # grad_out travels in the output's dtype
    a = L.Mlp128BwdArgs()
    _fill_shape(a, k1, in_dim, out_dim, st.out_act, out_dtype, st.grouped)
    _fill_operands(a, W=Wc)
    a.grad_out, a.out, a.k2p, a.n_hidden, a.hidden = L.ptr(g), L.ptr(out), (x2.shape[1] if x2 is not None else 0), n_hidden, Wc[0].shape[0]
    nbytes = L.load().pag_mlp128_workspace_bytes(M, n_hidden, out_dim, 2)
    L.check(min(nbytes, 0), "pag_mlp128_workspace_bytes")
    bws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    a.workspace, a.workspace_bytes, a.bwd_workspace, a.bwd_workspace_bytes = L.ptr(ws), ws.numel(), L.ptr(bws), nbytes
    a.dx1, a.dx1_dtype = L.ptr(dx1), (L.dtype_code(dx1) if need_dx else 0)
    a.dx1_accumulate = 1 if (need_dx and dx1_into is not None) else 0
    for i in range(n_hidden + 1):
        a.dW[i], a.db[i] = L.ptr(gW[i]), L.ptr(gb[i])
    _call("pag_mlp128_bwd", ctypes.byref(a), M, L.stream())
    dx2 = None
    if need_dx2:
        # dz_0 is the first plane of the backward workspace.  Not a hot path at this width: a segmented sum and one small matmul, with the weights
        # as the kernels round them
        dx2 = _dx2(x2, x2_index, st.x2_packs, _native_plane(bws, 0, 128, M), Wc[0][:, k1:in_dim].bfloat16().float())
    return dx1, dx2, gW, gb


class _FusedMLP128(torch.autograd.Function):
    """One BasicDecoder at hidden width 128 (pag_mlp128_fwd / pag_mlp128_bwd): no host read of device data, no shape that depends on device
    data, every buffer from torch's allocator - a captured step replays it."""

    @staticmethod
    def forward(ctx, call, x1, x2, x2_index, *wb):
        out, st = _mlp128_forward(call, ctx.needs_input_grad[1:3], x1, x2, x2_index, *wb)
        _save(ctx, st)
        return out

    @staticmethod
    def backward(ctx, g):
        return _decoder_grads(_mlp128_backward(ctx.state, ctx.saved_tensors, g))


def fused_mlp128(x1, weights, biases, x2=None, x2_index=None, in_dim=None, out_act=L.ACT_NONE, mode=L.MLP_MFMA_BF16,
                 out_dtype=torch.float32, x1_grouped=None, x2_packs=None):
    """fused_mlp at hidden width 128: 1 - 3 Linear + ReLU layers, then lout [+ sigmoid / softmax], in one launch (pag_mlp128_fwd).  Same arguments
    as fused_mlp; bf16 operands on the matrix cores only (the precision='fp32' path at this width is wide_mlp_reference)."""
    if mode != L.MLP_MFMA_BF16:
        raise NotImplementedError("fused_mlp128 runs in MLP_MFMA_BF16 mode; the fp32 form at width 128 is ops.wide_mlp_reference")
    if in_dim is None:
        in_dim = weights[0].shape[1]
    call = _DecoderCall(in_dim, out_act, mode, out_dtype, x1_grouped, x2_packs=x2_packs, need_grad=_need_grad(x1, x2, x2_index, *weights, *biases))
    return _apply(_FusedMLP128, call, x1, x2, x2_index, *weights, *biases)


# ------------------------------------------------------------------------------------------ ray march
def raymarch_ray(origins, dirs, dist_min, dist_max, num_samples, jitter=None, occupancy_bits=None, blas_level=7, want_ridx64=False):
    """'ray'-mode march + occupancy filter + pack.  Returns
    (ridx i32[M], pidx i32[M], samples f32[M,3], depths f32[M], deltas f32[M], boundary bool[M],
     pack_start i64[P+1], ray_of_pack i32[P])."""
    _check_gpu(origins, dirs)
    dev = origins.device
    N, S = origins.shape[0], int(num_samples)
    origins = origins.detach().contiguous().float()
    dirs = dirs.detach().contiguous().float()
    if jitter is None:
        jitter = torch.rand(N, S, device=dev)
    jitter = jitter.contiguous().float()
    tvals = _tvals(S, dev)
    counts = torch.empty(N, device=dev, dtype=torch.int32)
    occ = L.ptr(occupancy_bits) if occupancy_bits is not None else None
    st = L.stream()
    if N:
        _call("pag_raymarch_count", L.ptr(origins), L.ptr(dirs), N, S, L.ptr(tvals), L.ptr(jitter), float(dist_min),
                                       float(dist_max), occ, blas_level, L.ptr(counts), st)
    pack_start = torch.empty(N + 1, device=dev, dtype=torch.int64)      # [i] = first sample of ray i, [N] = M
    mailbox = _count_mailbox() if POLL_SAMPLE_COUNT else None
    if mailbox is not None:
        mailbox[1][0] = -1
    _call("pag_pack_offsets", L.ptr(counts), N, L.ptr(pack_start), mailbox[0].data_ptr() if mailbox is not None else None, st)
    # The pack kernel takes its write offsets from the device, so it is queued BEFORE the host learns the sample count:
    # buffers are sized for the N * S upper bound and trimmed to M afterwards.  The GPU then idles only for the read-back
    # itself instead of read-back + six allocations + four launches (0.11 ms per step).
    cap = N * S
    ridx = torch.empty(cap, device=dev, dtype=torch.int32)
    pidx = torch.empty(cap, device=dev, dtype=torch.int32)
    samples = torch.empty(cap, 3, device=dev)
    depths = torch.empty(cap, device=dev)
    deltas = torch.empty(cap, device=dev)
    boundary = torch.empty(cap, device=dev, dtype=torch.uint8)
    ridx64 = torch.empty(cap, device=dev, dtype=torch.int64) if want_ridx64 else None     # wisp hands out int64 ray ids
    if cap:
        _call("pag_raymarch_pack", L.ptr(origins), L.ptr(dirs), N, S, L.ptr(tvals), L.ptr(jitter), float(dist_min),
                                      float(dist_max), occ, blas_level, L.ptr(pack_start), L.ptr(ridx), L.ptr(pidx),
                                      L.ptr(samples), L.ptr(depths), L.ptr(deltas), L.ptr(boundary), L.ptr(ridx64), st)
    # one pack per RAY (empty packs allowed): no nonzero() / second host sync.  A ray without samples composites to the
    # background with alpha = depth = 0 and hit = False, exactly what the pre-filled buffers hold (Appendix E.10).
    M = _poll_count(mailbox) if mailbox is not None else -1
    if M < 0:
        M = int(pack_start[N].item())          # stream-synchronising read-back
        if mailbox is not None and int(mailbox[1][0]) < 0:
            # the kernel has finished (the read-back above waited for it) and its store never reached the mailbox: device
            # writes to this pinned allocation are not visible to the host on this system - stop polling for good
            _disable_polling()
    if mailbox is not None:
        if int(mailbox[1][0]) >= 0:       # the kernel has written its word: nobody else will touch it, back to the pool
            _release_mailbox(mailbox)
        # else: a store may still arrive later (timed-out poll) - the word is dropped, never lent again
    if want_ridx64:
        return (ridx[:M], pidx[:M], samples[:M], depths[:M], deltas[:M], boundary[:M].view(torch.bool), pack_start, _ray_iota(N, dev),
                ridx64[:M])
    return (ridx[:M], pidx[:M], samples[:M], depths[:M], deltas[:M], boundary[:M].view(torch.bool),   # kernel writes 0 / 1
            pack_start, _ray_iota(N, dev))


POLL_SAMPLE_COUNT = os.environ.get("PAG_NO_POLL") is None
_MAILBOX_LOCK = threading.Lock()
_MAILBOX_FREE = []          # pinned int64[1] words not lent to a march in flight


def _disable_polling():
    global POLL_SAMPLE_COUNT
    POLL_SAMPLE_COUNT = False


def _count_mailbox(dev=None):
    """(pinned i64[1] tensor, its numpy view) lent to ONE raymarch_ray call: the pack-offset kernel stores the sample count there
    (system-scope release) and the host polls it - it continues as soon as that tiny kernel has run instead of after a
    stream-synchronising copy behind the pack kernel (~50 us of the GPU-idle window at the head of every step).  Words come from a
    small pool under a lock and go back with _release_mailbox(), so two marches in flight (another stream or thread, e.g. an
    interactive render next to training) never preset and poll the same word."""
    with _MAILBOX_LOCK:
        if _MAILBOX_FREE:
            return _MAILBOX_FREE.pop()
    t = torch.empty(1, dtype=torch.int64).pin_memory()
    return (t, t.numpy())


def _release_mailbox(mailbox):
    with _MAILBOX_LOCK:
        if len(_MAILBOX_FREE) < 16:
            _MAILBOX_FREE.append(mailbox)


def _poll_count(mailbox, timeout_s=0.5):
    """Wait for the mailbox; -1 if nothing arrived in time (the caller then falls back to the synchronous read-back).  The first
    ~50 us are a tight spin (the usual case: the count arrives within 10-20 us); after that the loop yields the GIL with short
    sleeps so a delayed kernel (earlier work queued on the stream) does not starve other Python threads."""
    arr = mailbox[1]
    t0 = time.perf_counter()
    spins = 0
    while True:
        v = int(arr[0])
        if v >= 0:
            return v
        spins += 1
        if spins % 256 == 0:
            el = time.perf_counter() - t0
            if el > timeout_s:
                return -1
            if el > 50e-6:
                time.sleep(20e-6)


_IOTA = {}


def _one_pack_per_ray(ray_of_pack, N):
    """True when the pack table is the cached identity of raymarch_ray (pack i = ray i, empty packs included): the compositing
    kernels then write every ray's outputs themselves (an empty pack yields the background / zeros) and need no pre-filled buffers."""
    return ray_of_pack.shape[0] == N and _IOTA.get((N, str(ray_of_pack.device))) is ray_of_pack


def _ray_iota(N, dev):
    """arange(N) i32, cached per (N, device): ray_of_pack of the one-pack-per-ray layout (read-only by contract)."""
    key = (N, str(dev))
    if key not in _IOTA:
        if len(_IOTA) > 16:
            _IOTA.clear()
        _IOTA[key] = torch.arange(N, device=dev, dtype=torch.int32)
    return _IOTA[key]


def view_embed(dirs, n_freq, width):
    """f32 [R, width] = wisp PositionalEmbedder(-dirs) zero padded (pag_view_embed); no gradient (callers keep the tensor-op
    form when the directions are learnable)."""
    _check_gpu(dirs)
    d = dirs.detach().contiguous().float()
    out = torch.empty(d.shape[0], width, device=d.device)
    _call("pag_view_embed", L.ptr(d), d.shape[0], int(n_freq), int(width), L.ptr(out), L.stream())
    return out


class _ViewEmbed(torch.autograd.Function):
    """view_embed() with d / d dirs (pose optimisation: the view direction depends on the camera rotation, ba_pipeline.py:89-90):
    pag_view_embed forward - the SAME values as the gradient-free path - and pag_view_embed_bwd instead of the ~25 launches of the
    tensor-op form's forward + backward."""

    @staticmethod
    def forward(ctx, dirs, n_freq, width):
        d = dirs.detach().contiguous().float()
        ctx.save_for_backward(d)
        ctx.cfg = (int(n_freq), int(width))
        out = torch.empty(d.shape[0], width, device=d.device)
        _call("pag_view_embed", L.ptr(d), d.shape[0], int(n_freq), int(width), L.ptr(out), L.stream())
        return out

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        n_freq, width = ctx.cfg
        g = g.contiguous().float()
        out = torch.empty_like(d)
        _call("pag_view_embed_bwd", L.ptr(d), d.shape[0], n_freq, width, L.ptr(g), L.ptr(out), L.stream())
        return out, None, None


def view_embed_grad(dirs, n_freq, width):
    """view_embed() differentiable with respect to `dirs` (f32 [R,3] on the GPU)."""
    _check_gpu(dirs)
    return _apply(_ViewEmbed, dirs, n_freq, width)


class _PoseRays(torch.autograd.Function):
    """pc_nerf/ba_pipeline.py:85-92 as one launch each way (pag_pose_rays_fwd / _bwd): camera-frame rays -> world-frame rays through the
    camera parameters [C,9], differentiable with respect to the parameters."""

    @staticmethod
    def forward(ctx, params, cam, rays_per_entry, origins_c, dirs_c):
        p = params.detach().contiguous().float()
        oc, dc = origins_c.detach().contiguous().float(), dirs_c.detach().contiguous().float()
        N = oc.shape[0]
        ow, dw = torch.empty(N, 3, device=p.device), torch.empty(N, 3, device=p.device)
        _call("pag_pose_rays_fwd", L.ptr(p), p.shape[0], L.ptr(cam), int(rays_per_entry), L.ptr(oc), L.ptr(dc), N, L.ptr(ow), L.ptr(dw), L.stream())
        ctx.save_for_backward(p, cam, oc, dc)
        ctx.rpe = int(rays_per_entry)
        ctx.set_materialize_grads(False)
        return ow, dw

    @staticmethod
    def backward(ctx, g_o, g_d):
        p, cam, oc, dc = ctx.saved_tensors
        if g_o is None and g_d is None:
            return None, None, None, None, None
        g_o = g_o.contiguous().float() if g_o is not None else None
        g_d = g_d.contiguous().float() if g_d is not None else None
        d_params = torch.empty_like(p)
        ws_bytes = L.load().pag_pose_rays_bwd_workspace_bytes(p.shape[0])
        ws = torch.empty(ws_bytes // 4, device=p.device)
        _call("pag_pose_rays_bwd", L.ptr(p), p.shape[0], L.ptr(cam), ctx.rpe, L.ptr(oc), L.ptr(dc), oc.shape[0], L.ptr(g_o), L.ptr(g_d), L.ptr(d_params),
              L.ptr(ws), ws_bytes, L.stream())
        return d_params, None, None, None, None


def pose_rays(params, cam, rays_per_entry, origins_c, dirs_c):
    """-> (origins_w, dirs_w) f32 [N,3]: ray i through camera cam[i // rays_per_entry] (row of params f32 [C,9] = a1, a2, t); cam i32."""
    _check_gpu(params, cam, origins_c, dirs_c)
    if origins_c.shape != dirs_c.shape or origins_c.dim() != 2 or origins_c.shape[1] != 3:
        raise RuntimeError("pose_rays: origins / dirs must both be [N,3], got %s and %s" % (tuple(origins_c.shape), tuple(dirs_c.shape)))
    n_entries = (origins_c.shape[0] + rays_per_entry - 1) // rays_per_entry
    if cam.dtype != torch.int32 or cam.numel() < n_entries or params.dim() != 2 or params.shape[1] != 9:
        raise RuntimeError("pose_rays: cam must be int32 with one entry per %d rays, params [C,9]" % rays_per_entry)
    return _PoseRays.apply(params, cam.contiguous(), int(rays_per_entry), origins_c, dirs_c)


def pose_points(params, cam, rays_per_entry, origins_c, dirs_c, depth):
    """-> points f32 [N,3] (no gradient): sum_k (o_c - t + d_c * depth)[k] R[k] of ray i's camera cam[i // rays_per_entry] - utils/outlier_rejection.py:74-97."""
    _check_gpu(params, cam, origins_c, dirs_c, depth)
    N = origins_c.shape[0]
    if origins_c.shape != dirs_c.shape or origins_c.dim() != 2 or origins_c.shape[1] != 3 or depth.numel() != N:
        raise RuntimeError("pose_points: origins / dirs [N,3] and depth [N], got %s, %s, %s" % (tuple(origins_c.shape), tuple(dirs_c.shape), tuple(depth.shape)))
    n_entries = (N + rays_per_entry - 1) // rays_per_entry
    if cam.dtype != torch.int32 or cam.numel() < n_entries or params.dim() != 2 or params.shape[1] != 9:
        raise RuntimeError("pose_points: cam must be int32 with one entry per %d rays, params [C,9]" % rays_per_entry)
    prm, oc, dc = params.detach().contiguous().float(), origins_c.detach().contiguous().float(), dirs_c.detach().contiguous().float()
    dep = depth.detach().reshape(-1).contiguous().float()
    out = torch.empty(N, 3, device=oc.device)
    _call("pag_pose_points", prm.data_ptr(), prm.shape[0], cam.contiguous().data_ptr(), int(rays_per_entry), oc.data_ptr(), dc.data_ptr(), dep.data_ptr(), N,
          out.data_ptr(), L.stream())
    return out


class _RaySamples(torch.autograd.Function):
    """samples = origins[ray] + dirs[ray] * depth with the march kernel's values as the forward result (bit-identical to
    the non-differentiable path) and d/d origins, d/d dirs as per-ray segmented sums - what autograd gives through
    wisp's `torch.addcmul(origins[ridx], dirs[ridx], depth)` when the rays come from learnable extrinsics
    (ba_pipeline.py:85-92)."""

    @staticmethod
    def forward(ctx, origins, dirs, samples, depths, pack_start, ray_of_pack):
        ctx.save_for_backward(depths, pack_start, ray_of_pack)
        ctx.N = origins.shape[0]
        return samples.view_as(samples)

    @staticmethod
    def backward(ctx, g):
        depths, pack_start, ray_of_pack = ctx.saved_tensors
        N = ctx.N
        g = g.reshape(-1, 3).float().contiguous()
        P = ray_of_pack.shape[0]
        # [N,6]: d/d origin | d/d dir, one launch (pag_ray_sample_grad); every ray has a pack on the one-pack-per-ray layout
        seg = (torch.empty if (P and _one_pack_per_ray(ray_of_pack, N)) else torch.zeros)(N, 6, device=g.device)
        if P and g.shape[0]:
            _call("pag_ray_sample_grad", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(g), L.ptr(depths.reshape(-1).float().contiguous()),
                  L.ptr(seg), L.stream())
        elif P:
            seg.zero_()
        return seg[:, :3], seg[:, 3:], None, None, None, None


def ray_samples(origins, dirs, samples, depths, pack_start, ray_of_pack, ridx=None):
    """Attach the pose gradient to march-kernel samples (samples [M,3] or [M',k,3], depths alike, one pack per ray).
    ridx (i32, the ray of every SAMPLE, as the march kernels write it): the result is tagged (`_pag_rays`) so that an encoder that interpolates exactly these
    samples can send its position gradient to origins / dirs directly, reduced per ray inside its gather pass (encode(..., rays=...))."""
    out = _RaySamples.apply(origins, dirs, samples, depths, pack_start, ray_of_pack)
    if ridx is not None and _one_pack_per_ray(ray_of_pack, origins.shape[0]) and ridx.dtype == torch.int32:
        out._pag_rays = (origins, dirs, depths, pack_start, ridx)
    return out


_TVALS = {}


def _tvals(S, dev):
    """linspace(0,1,S) computed on the CPU (bit-identical to the oracle's) and cached per (S, device)."""
    key = (S, str(dev))
    if key not in _TVALS:
        _TVALS[key] = torch.linspace(0, 1.0, S).to(dev)
    return _TVALS[key]


VOXEL_SCRATCH_MAX = 1 << 30      # bytes of nugget scratch raymarch_voxel() may hold at a time: more rays than that are marched in chunks


def raymarch_voxel(origins, dirs, dist_min, dist_max, samples_per_voxel, occupancy_bits=None, blas_level=7, max_travel=None, want_packs=False):
    """'voxel'-mode march (3-D DDA over the occupancy grid).  Returns per NUGGET ridx i32[M'], pidx i32[M'] and per sample
    samples f32[M',k,3], depths f32[M',k], deltas f32[M'*k], boundary bool[M'*k].
    max_travel: the tracer's travel filter (tracers/panoptic_packed_rf_tracer.py:88-108) applied inside the walk (None = off).
    want_packs: also (pack_start i64[N+1] in samples, ray_of_pack i32[N] = arange, ridx_sample i32[M'*k], ridx64 i64[M']) - one
    (possibly empty) pack per ray, straight from the kernels: no unique / nonzero / repeat_interleave passes, and the sample
    count reaches the host through the polled mailbox of raymarch_ray()."""
    return raymarch_voxel_finish(raymarch_voxel_begin(origins, dirs, dist_min, dist_max, samples_per_voxel, occupancy_bits, blas_level, max_travel, want_packs))


def raymarch_voxel_begin(origins, dirs, dist_min, dist_max, samples_per_voxel, occupancy_bits=None, blas_level=7, max_travel=None, want_packs=False):
    """First half of raymarch_voxel(): the walk (nugget candidates, selection, counts) and the pack offsets are QUEUED, nothing is waited for.  -> state for
    raymarch_voxel_finish(), which reads the sample count, sizes the packed tensors and queues the expansion.  A caller with several marches to do
    (PanopticPackedRFTracer.render_packs) begins the next one before it finishes this one: the walk - a latency-bound DDA per ray - then runs while the
    host is busy elsewhere, and the count is there when it is asked for.
    More rays than VOXEL_SCRATCH_MAX bytes of nugget scratch serve (2 x [cap][N] entries of 12 bytes) queue nothing here: raymarch_voxel_finish() marches
    them in chunks."""
    _check_gpu(origins, dirs)
    dev = origins.device
    N, k = origins.shape[0], int(samples_per_voxel)
    cap = int(L.load().pag_raymarch_voxel_nugget_capacity(blas_level))
    chunk = max(1, VOXEL_SCRATCH_MAX // (24 * cap))
    if N > chunk:
        return chunk, (origins, dirs, dist_min, dist_max, k, occupancy_bits, blas_level, max_travel, want_packs)
    origins = origins.detach().contiguous().float()
    dirs = dirs.detach().contiguous().float()
    counts = torch.empty(N, device=dev, dtype=torch.int32)
    st = L.stream()
    nug_t = nug_cell = None
    if N:
        nug_t = torch.empty(2, cap, N, 2, device=dev)              # [0]: the walk's candidates [step][ray], [1]: the kept nuggets [ray][slot]
        nug_cell = torch.empty(2, cap, N, device=dev, dtype=torch.int32)
        _call("pag_raymarch_voxel_count_nuggets", L.ptr(origins), L.ptr(dirs), N, k, float(dist_min), float(dist_max),
              L.ptr(occupancy_bits) if occupancy_bits is not None else None, blas_level, float("inf") if max_travel is None else float(max_travel),
              L.ptr(counts), L.ptr(nug_t), L.ptr(nug_cell), st)
    pack_start = torch.empty(N + 1, device=dev, dtype=torch.int64)      # [i] = first SAMPLE of ray i, [N] = M' * k
    mailbox = _count_mailbox() if POLL_SAMPLE_COUNT else None
    if mailbox is not None:
        mailbox[1][0] = -1
    _call("pag_pack_offsets", L.ptr(counts), N, L.ptr(pack_start), mailbox[0].data_ptr() if mailbox is not None else None, st)
    return None, (origins, dirs, N, k, occupancy_bits, blas_level, counts, nug_t, nug_cell, pack_start, mailbox, want_packs)


def _raymarch_voxel_chunks(chunk, origins, dirs, *rest):
    """raymarch_voxel() of more rays than one call's scratch serves: consecutive chunks of rays through the same code, one after the other (so one chunk's
    scratch is alive at a time), and the results joined.  Rays are independent: bit for bit the result of one march of them all."""
    N, want_packs = origins.shape[0], rest[-1]
    parts, s0 = [], 0                    # s0: samples before the chunk
    for r0 in range(0, N, chunk):
        part = list(raymarch_voxel_finish(raymarch_voxel_begin(origins[r0:r0 + chunk], dirs[r0:r0 + chunk], *rest)))
        part[0] += r0                                   # ridx
        if want_packs:
            part[6] = part[6][:-1] + s0                 # pack_start, without the chunk's total
            part[8] += r0                               # ridx_sample
            part[9] += r0                               # ridx64
        s0 += part[3].numel()
        parts.append(part)
    out = [torch.cat(p) for p in zip(*parts)]
    if want_packs:
        out[6] = torch.cat([out[6], torch.full((1,), s0, device=origins.device, dtype=torch.int64)])
        out[7] = _ray_iota(N, origins.device)
    return tuple(out)


def raymarch_voxel_finish(state):
    chunk, state = state
    if chunk is not None:
        return _raymarch_voxel_chunks(chunk, *state)
    (origins, dirs, N, k, _occ_t, blas_level, counts, nug_t, nug_cell, pack_start, mailbox, want_packs) = state
    dev = origins.device
    st = L.stream()
    total = _poll_count(mailbox) if mailbox is not None else -1
    if total < 0:
        total = int(pack_start[N].item())          # stream-synchronising read-back
        if mailbox is not None and int(mailbox[1][0]) < 0:
            _disable_polling()
    if mailbox is not None and int(mailbox[1][0]) >= 0:
        _release_mailbox(mailbox)
    Mn = total // k
    ridx = torch.empty(Mn, device=dev, dtype=torch.int32)
    pidx = torch.empty(Mn, device=dev, dtype=torch.int32)
    samples = torch.empty(Mn, k, 3, device=dev)
    depths = torch.empty(Mn, k, device=dev)
    deltas = torch.empty(Mn * k, device=dev)
    boundary = torch.empty(Mn * k, device=dev, dtype=torch.uint8)
    ridx_sample = torch.empty(Mn * k, device=dev, dtype=torch.int32) if want_packs else None
    ridx64 = torch.empty(Mn, device=dev, dtype=torch.int64) if want_packs else None
    if Mn:
        _call("pag_raymarch_voxel_pack_nuggets", L.ptr(origins), L.ptr(dirs), N, k, L.ptr(pack_start), L.ptr(nug_t), L.ptr(nug_cell), blas_level,
              L.ptr(ridx), L.ptr(pidx), L.ptr(samples), L.ptr(depths), L.ptr(deltas), L.ptr(boundary), L.ptr(ridx_sample), L.ptr(ridx64), st)
    if want_packs:
        return (ridx, pidx, samples, depths, deltas, boundary.view(torch.bool), pack_start, _ray_iota(N, dev), ridx_sample, ridx64)
    return ridx, pidx, samples, depths, deltas, boundary.view(torch.bool)


class MarchBuffers:
    """Upper-bound packed-sample buffers of one march configuration, for the graph path (pagnerf_amd/graphs.py): the march kernels write
    into them without the host knowing the sample count, pad_to() appends inert samples up to a fixed capacity, and the first
    `capacity` elements are the STATIC tensors a captured HIP graph reads.  mode 'ray': per_ray = samples per ray (k = 1);
    mode 'voxel': per_ray = pag_raymarch_voxel_nugget_capacity(level), k = samples per nugget."""

    def __init__(self, mode, N, per_ray, k, dev):
        self.mode, self.N, self.k = mode, int(N), int(k)
        ne = self.N * int(per_ray)                 # entries (nuggets; = samples in 'ray' mode)
        self.cap = ne * self.k                     # samples
        self.samples = torch.zeros(self.cap, 3, device=dev)
        self.depths = torch.zeros(self.cap, device=dev)
        self.deltas = torch.zeros(self.cap, device=dev)
        self.boundary = torch.zeros(self.cap, device=dev, dtype=torch.uint8)
        self.ridx_entry = torch.zeros(ne, device=dev, dtype=torch.int32)
        self.ridx_sample = self.ridx_entry if self.k == 1 else torch.zeros(self.cap, device=dev, dtype=torch.int32)
        self.ridx64 = torch.zeros(ne, device=dev, dtype=torch.int64)
        self.pidx = torch.zeros(ne, device=dev, dtype=torch.int32)
        self.counts = torch.zeros(self.N, device=dev, dtype=torch.int32)
        self.pack_start = torch.zeros(self.N + 1, device=dev, dtype=torch.int64)
        # min(pack_start, capacity), written by pad_to(): the pack table of every launch that is queued on the capacity-sized views before
        # the host knows the sample count - no per-ray kernel can walk past the capacity when a batch overflows it
        self.pack_start_c = torch.zeros(self.N + 1, device=dev, dtype=torch.int64)
        if mode == "voxel":
            self.nug_t = torch.empty(2, int(per_ray), self.N, 2, device=dev)
            self.nug_cell = torch.empty(2, int(per_ray), self.N, device=dev, dtype=torch.int32)

    def pad_to(self, capacity):
        """Queue pag_pad_packed: samples [M, capacity) become filler samples outside every pack (pack_start is left alone) and
        pack_start_c = min(pack_start, capacity)."""
        assert 0 < capacity <= self.cap and capacity % self.k == 0
        _call("pag_pad_packed", L.ptr(self.pack_start), self.N, int(capacity), self.k, L.ptr(self.samples), L.ptr(self.depths), L.ptr(self.deltas),
              L.ptr(self.ridx_sample) if self.k > 1 else None, L.ptr(self.ridx_entry), L.ptr(self.ridx64), L.ptr(self.pidx), L.ptr(self.boundary),
              L.ptr(self.pack_start_c), L.stream())


def _offsets(buf, N, mb_ptr, st, pad_capacity, dirs, dirs_out):
    """The scan of the per-ray counts into the pack table, alone or fused with the padding / direction copy of the graph path."""
    if pad_capacity is None:
        _call("pag_pack_offsets", L.ptr(buf.counts), N, L.ptr(buf.pack_start), mb_ptr, st)
        return
    assert 0 < pad_capacity <= buf.cap and pad_capacity % buf.k == 0
    copy = dirs_out is not None and dirs_out.data_ptr() != dirs.data_ptr()
    _call("pag_pack_offsets_pad", L.ptr(buf.counts), N, L.ptr(buf.pack_start), mb_ptr, int(pad_capacity), buf.k, L.ptr(buf.samples), L.ptr(buf.depths),
          L.ptr(buf.deltas), L.ptr(buf.ridx_sample) if buf.k > 1 else None, L.ptr(buf.ridx_entry), L.ptr(buf.ridx64), L.ptr(buf.pidx),
          L.ptr(buf.boundary), L.ptr(buf.pack_start_c), L.ptr(dirs) if copy else None, L.ptr(dirs_out) if copy else None, st)


def march_into(buf, origins, dirs, dist_min, dist_max, num_samples, jitter=None, occupancy_bits=None, blas_level=7, max_travel=None, pad_capacity=None,
               dirs_out=None):
    """The ray march of raymarch_ray() / raymarch_voxel() written into `buf` (MarchBuffers) WITHOUT waiting for the sample count:
    count -> offsets (+ pinned mailbox) -> pack are queued back to back.  -> the mailbox (poll it with _poll_count() when convenient;
    give it back with _release_mailbox()) or None when polling is disabled (the caller then reads buf.pack_start[N] itself).
    pad_capacity: the offsets launch also pads the batch to that capacity (MarchBuffers.pad_to) and, with dirs_out, copies the ray
    directions into that static tensor - one launch instead of three (pag_pack_offsets_pad)."""
    _check_gpu(origins, dirs)
    dev = origins.device
    N = origins.shape[0]
    assert N == buf.N
    origins = origins.detach().contiguous().float()
    dirs = dirs.detach().contiguous().float()
    occ = L.ptr(occupancy_bits) if occupancy_bits is not None else None
    st = L.stream()
    mailbox = _count_mailbox() if POLL_SAMPLE_COUNT else None
    if mailbox is not None:
        mailbox[1][0] = -1
    mb_ptr = mailbox[0].data_ptr() if mailbox is not None else None
    if buf.mode == "ray":
        S = int(num_samples)
        if jitter is None:
            jitter = torch.rand(N, S, device=dev)
        jitter = jitter.contiguous().float()
        tvals = _tvals(S, dev)
        _call("pag_raymarch_count", L.ptr(origins), L.ptr(dirs), N, S, L.ptr(tvals), L.ptr(jitter), float(dist_min), float(dist_max), occ,
              blas_level, L.ptr(buf.counts), st)
        _offsets(buf, N, mb_ptr, st, pad_capacity, dirs, dirs_out)
        _call("pag_raymarch_pack", L.ptr(origins), L.ptr(dirs), N, S, L.ptr(tvals), L.ptr(jitter), float(dist_min), float(dist_max), occ,
              blas_level, L.ptr(buf.pack_start), L.ptr(buf.ridx_entry), L.ptr(buf.pidx), L.ptr(buf.samples), L.ptr(buf.depths),
              L.ptr(buf.deltas), L.ptr(buf.boundary), L.ptr(buf.ridx64), st)
    else:
        k = buf.k
        travel = float("inf") if max_travel is None else float(max_travel)
        _call("pag_raymarch_voxel_count_nuggets", L.ptr(origins), L.ptr(dirs), N, k, float(dist_min), float(dist_max), occ,
              blas_level, travel, L.ptr(buf.counts), L.ptr(buf.nug_t), L.ptr(buf.nug_cell), st)
        _offsets(buf, N, mb_ptr, st, pad_capacity, dirs, dirs_out)
        _call("pag_raymarch_voxel_pack_nuggets", L.ptr(origins), L.ptr(dirs), N, k, L.ptr(buf.pack_start), L.ptr(buf.nug_t), L.ptr(buf.nug_cell), blas_level,
              L.ptr(buf.ridx_entry), L.ptr(buf.pidx), L.ptr(buf.samples), L.ptr(buf.depths), L.ptr(buf.deltas), L.ptr(buf.boundary),
              L.ptr(buf.ridx_sample), L.ptr(buf.ridx64), st)
    return mailbox, jitter


def copy_batch(dsts, srcs):
    """dst[i].copy_(src[i]) for lists of same-shape, same-dtype contiguous GPU tensors as ONE launch per 16 tensors (pag_copy_batch);
    pairs that need a conversion or are not contiguous take torch's copy_."""
    easy, hard = [], []
    for d, s_ in zip(dsts, srcs):
        (easy if (d.dtype == s_.dtype and d.shape == s_.shape and d.is_contiguous() and s_.is_contiguous() and d.is_cuda and s_.is_cuda)
         else hard).append((d, s_))
    for c0 in range(0, len(easy), 16):
        part = easy[c0:c0 + 16]
        n = len(part)
        _call("pag_copy_batch", n, (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in part]), (ctypes.c_void_p * n)(*[s_.data_ptr() for _, s_ in part]),
              (ctypes.c_int64 * n)(*[d.numel() * d.element_size() for d, _ in part]), L.stream())
    for d, s_ in hard:
        d.copy_(s_)


def packs_from_boundary(ridx, boundary):
    """(pack_start i64[P+1], ray_of_pack i32[P]) from kaolin-style (ridx, boundary) arrays."""
    starts = torch.nonzero(boundary).reshape(-1)
    end = torch.tensor([boundary.shape[0]], device=boundary.device, dtype=torch.int64)
    return torch.cat([starts, end]).contiguous(), ridx[starts].int().contiguous()


def occupancy_update(density, occupancy, bits, decay, min_density):
    """In place: occupancy <- max(density, occupancy*decay); bits <- occupancy > min_density  (prune, nef :74-104).
    density f32 [cells] (any stride over dim 0), occupancy f32 [cells], bits i32 [ceil(cells/32)]."""
    _check_gpu(density, occupancy, bits)
    cells = occupancy.shape[0]
    density = density.detach()
    if density.dim() != 1 or density.dtype != torch.float32:
        density = density.reshape(cells, -1)[:, 0].float()
    assert occupancy.is_contiguous() and bits.is_contiguous() and bits.numel() * 32 >= cells
    _call("pag_occupancy_update", density.data_ptr(), density.stride(0), L.ptr(occupancy), L.ptr(bits), cells, float(decay),
          float(min_density), L.stream())


def _carve_bits(name, what, bits, blas_level):
    words = max(1, (2 ** int(blas_level)) ** 3 // 32)
    if bits.dtype != torch.int32 or bits.numel() != words or not bits.is_contiguous():
        raise ValueError("%s: %s must be a contiguous int32 [%d] bitfield of level %d, got %s %s" % (name, what, words, blas_level, bits.dtype, tuple(bits.shape)))


def carve_rays(origins, dirs, t_hit, dist_min, dist_max, margin, blas_level, free_bits, surface_bits):
    """pag_carve_rays (carve.carve_reference is the definition): the cells that the rays (origins, dirs f32 [N,3]; t_hit f32 [N] the measured distance
    along the ray, <= 0 / NaN / inf = no measurement) cross in front of t_hit - margin are OR-ed into free_bits, the cells within margin of t_hit
    into surface_bits: int32 [max(1, R^3/32)] each, zeroed by the caller before the first call.  One launch."""
    _check_gpu(origins, dirs, t_hit, free_bits, surface_bits)
    N = t_hit.numel()
    if origins.shape != (N, 3) or dirs.shape != (N, 3) or any(t.dtype != torch.float32 for t in (origins, dirs, t_hit)):
        raise ValueError("carve_rays: origins / dirs must be f32 [N,3] and t_hit f32 [N], got %s %s %s" % (tuple(origins.shape), tuple(dirs.shape), tuple(t_hit.shape)))
    _carve_bits("carve_rays", "free_bits", free_bits, blas_level)
    _carve_bits("carve_rays", "surface_bits", surface_bits, blas_level)
    _call("pag_carve_rays", L.ptr(origins), L.ptr(dirs), L.ptr(t_hit), N, float(dist_min), float(dist_max), float(margin), int(blas_level),
          L.ptr(free_bits), L.ptr(surface_bits), L.stream())


def carve_finish(free_bits, surface_bits, blas_level, dilate=1, mode="hull", out=None):
    """pag_carve_finish (carve.carve_finish_reference is the definition): surface dilated `dilate` times by the 26-neighbourhood = D;
    'hull': ~free | D, 'band': D -> int32 bits (a new tensor, or `out`).  One launch."""
    _check_gpu(free_bits, surface_bits, out)
    modes = {"hull": L.CARVE_HULL, "band": L.CARVE_BAND}
    if mode not in modes:
        raise ValueError("carve_finish: unknown mode %r (hull / band)" % (mode,))
    _carve_bits("carve_finish", "free_bits", free_bits, blas_level)
    _carve_bits("carve_finish", "surface_bits", surface_bits, blas_level)
    if out is None:
        out = torch.empty_like(free_bits)
    _carve_bits("carve_finish", "out", out, blas_level)
    if out.data_ptr() in (free_bits.data_ptr(), surface_bits.data_ptr()):
        raise ValueError("carve_finish: out must not alias an input")
    _call("pag_carve_finish", L.ptr(free_bits), L.ptr(surface_bits), int(blas_level), int(dilate), modes[mode], L.ptr(out), L.stream())
    return out


# ----------------------------------------------------------------------------------------- composite
class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sigma, rgb, deltas, depths, pack_start, ray_of_pack, N, bg_white):
        _check_gpu(sigma, deltas)
        dev = sigma.device
        M = sigma.shape[0]
        P = ray_of_pack.shape[0]
        sigma = sigma.detach().contiguous().float()
        deltas = deltas.detach().contiguous().float()
        rgbc = rgb.detach().contiguous().float() if rgb is not None else None
        depc = depths.detach().contiguous().float() if depths is not None else None
        # padded batches (graphs.py): the weights of the filler samples past pack_start[P] are zeroed by the launch itself (n_samples)
        w = torch.empty(M, device=dev) if (P and M) else torch.zeros(M, device=dev)
        ctx.tail_zero = TAIL_ZERO
        if M and _one_pack_per_ray(ray_of_pack, N):      # the kernel writes every ray (background for empty packs): no fills
            alpha = torch.empty(N, device=dev)
            hit = torch.empty(N, device=dev, dtype=torch.uint8)
            out_rgb = torch.empty(N, 3, device=dev) if rgb is not None else None
            out_depth = torch.empty(N, device=dev) if depths is not None else None
        else:
            alpha = torch.zeros(N, device=dev)
            hit = torch.zeros(N, device=dev, dtype=torch.uint8)
            out_rgb = (torch.ones if bg_white else torch.zeros)(N, 3, device=dev) if rgb is not None else None
            out_depth = torch.zeros(N, device=dev) if depths is not None else None
        if P and M:                     # M == 0: every pack is empty, the outputs already hold the background
            _call("pag_composite_fwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(sigma), L.ptr(deltas), L.ptr(depc),
                                          L.ptr(rgbc), L.BG_WHITE if bg_white else L.BG_BLACK, L.ptr(w), L.ptr(alpha),
                                          L.ptr(out_rgb), L.ptr(out_depth), L.ptr(hit), M if TAIL_ZERO else 0, L.stream())
        ctx.save_for_backward(sigma, rgbc, deltas, depc, pack_start, ray_of_pack, w, alpha)
        ctx.bg_white = bg_white
        ctx.mark_non_differentiable(hit, w)
        ctx.set_materialize_grads(False)      # unused outputs (alpha, depth, hit, w) arrive as None, not as zero-filled tensors
        return alpha, hit, out_rgb, out_depth, w

    @staticmethod
    def backward(ctx, g_alpha, _g_hit, g_rgb, g_depth, _g_w):
        sigma, rgbc, deltas, depc, pack_start, ray_of_pack, w, alpha = ctx.saved_tensors
        M, P = sigma.shape[0], ray_of_pack.shape[0]
        mk = torch.empty if (P and M) else torch.zeros          # samples covered by packs: the kernel writes every element; fillers: zeroed by the launch (n_samples)
        d_sigma = mk(M, device=sigma.device)
        d_rgb = mk(M, 3, device=sigma.device) if rgbc is not None else None
        gc = lambda t: t.contiguous().float() if t is not None else None
        g_alpha, g_rgb, g_depth = gc(g_alpha), gc(g_rgb), gc(g_depth)
        if P and M:
            _call("pag_composite_bwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(sigma), L.ptr(deltas), L.ptr(depc),
                                          L.ptr(rgbc), L.BG_WHITE if ctx.bg_white else L.BG_BLACK, L.ptr(w), L.ptr(alpha),
                                          L.ptr(g_rgb), L.ptr(g_depth), L.ptr(g_alpha), L.ptr(d_sigma), L.ptr(d_rgb),
                                          M if ctx.tail_zero else 0, L.stream())
        return d_sigma, d_rgb, None, None, None, None, None, None


def composite(sigma, rgb, deltas, depths, pack_start, ray_of_pack, N, bg_white=True):
    """-> (alpha [N], hit u8 [N], rgb [N,3] | None, depth [N] | None, weights [M]); tracer :134-176."""
    return _apply(_Composite, sigma, rgb, deltas, depths, pack_start, ray_of_pack, N, bg_white)


class _CompositeFeats(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, weights, alpha, pack_start, ray_of_pack, N):
        _check_gpu(feats, weights, alpha)
        feats = feats.detach().contiguous()
        if feats.dtype not in (torch.float32, torch.bfloat16):
            feats = feats.float()
        C = feats.shape[1]
        P = ray_of_pack.shape[0]
        out = torch.zeros(N, C, device=feats.device)
        weights = weights.detach().contiguous()
        alpha = alpha.detach().contiguous()
        if P and feats.shape[0]:
            _call("pag_composite_feats_fwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(weights), L.ptr(alpha),
                                                L.ptr(feats), L.dtype_code(feats), C, L.ptr(out), L.stream())
        ctx.save_for_backward(weights, alpha, pack_start, ray_of_pack)
        ctx.shape, ctx.fdtype = feats.shape, feats.dtype
        ctx.tail_zero = TAIL_ZERO
        return out

    @staticmethod
    def backward(ctx, g):
        weights, alpha, pack_start, ray_of_pack = ctx.saved_tensors
        M, C = ctx.shape
        P = ray_of_pack.shape[0]
        # every packed sample belongs to a pack, so the kernel writes every row: no zero fill of the [M,C] buffer
        d = torch.empty(M, C, device=weights.device, dtype=ctx.fdtype) if (P and not ctx.tail_zero) else torch.zeros(M, C, device=weights.device, dtype=ctx.fdtype)
        if P and M:
            _call("pag_composite_feats_bwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(weights), L.ptr(alpha),
                  L.ptr(g.contiguous().float()), C, L.ptr(d), L.dtype_code(d), L.stream())
        return d, None, None, None, None, None


def composite_feats(feats, weights, alpha, pack_start, ray_of_pack, N):
    """out[ray] = alpha[ray] * sum_i w_i feats[i]  (weights/alpha detached; tracer :148-155,:197-205)."""
    return _apply(_CompositeFeats, feats, weights, alpha, pack_start, ray_of_pack, N)


class _CompositeFeatsWeights(torch.autograd.Function):
    """out[ray] = alpha_r * sum_i w_i f_i with w, alpha computed from (sigma, deltas) INSIDE the node and differentiable:
    the delta-density tracer composites the panoptic channels with the panoptic density's own weights and keeps their
    gradient (tracers/panoptic_dd_packed_rf_tracer.py:124-135,162-166).
    Backward: d f_i = alpha w_i G_r (composite_feats_bwd).  For sigma, sum_c G_rc out_rc = alpha_r sum_i w_i s_i with the
    per-sample scalar s_i = <G_r, f_i>, which is the black-background colour formula of pag_composite_bwd on the
    one-channel "colour" s - so d sigma comes from that kernel with rgb = (s,0,0) and upstream gradient (1,0,0)."""

    @staticmethod
    def forward(ctx, sigma, deltas, feats, ridx, pack_start, ray_of_pack, N):
        _check_gpu(sigma, deltas, feats)
        dev = sigma.device
        M, P = sigma.shape[0], ray_of_pack.shape[0]
        sigma = sigma.detach().contiguous().float()
        deltas = deltas.detach().contiguous().float()
        feats = feats.detach().contiguous()
        if feats.dtype not in (torch.float32, torch.bfloat16):
            feats = feats.float()
        C = feats.shape[1]
        w = torch.empty(M, device=dev)
        alpha = torch.zeros(N, device=dev)
        hit = torch.zeros(N, device=dev, dtype=torch.uint8)
        out = torch.zeros(N, C, device=dev)
        if P and M:
            _call("pag_composite_fwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(sigma), L.ptr(deltas), None, None, L.BG_BLACK,
                  L.ptr(w), L.ptr(alpha), None, None, L.ptr(hit), 0, L.stream())
            _call("pag_composite_feats_fwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(w), L.ptr(alpha), L.ptr(feats),
                  L.dtype_code(feats), C, L.ptr(out), L.stream())
        ctx.save_for_backward(sigma, deltas, feats, ridx, pack_start, ray_of_pack, w, alpha)
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, g, _g_alpha):
        sigma, deltas, feats, ridx, pack_start, ray_of_pack, w, alpha = ctx.saved_tensors
        M, C = feats.shape
        P = ray_of_pack.shape[0]
        dev = sigma.device
        g = g.contiguous().float()
        d_feats = torch.zeros(M, C, device=dev, dtype=feats.dtype)
        d_sigma = torch.zeros(M, device=dev)
        if P and M:
            if ctx.needs_input_grad[2]:
                _call("pag_composite_feats_bwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(w), L.ptr(alpha), L.ptr(g), C,
                      L.ptr(d_feats), L.dtype_code(d_feats), L.stream())
            if ctx.needs_input_grad[0]:
                s3 = torch.zeros(M, 3, device=dev)
                rl = ridx.long()
                step = max(1, (1 << 24) // max(C, 1))                        # bound the [chunk, C] temporary
                for lo in range(0, M, step):
                    hi = min(M, lo + step)
                    s3[lo:hi, 0] = (feats[lo:hi].float() * g[rl[lo:hi]]).sum(1)
                ones = torch.zeros(alpha.shape[0], 3, device=dev)
                ones[:, 0] = 1.0
                d_rgb = torch.empty(M, 3, device=dev)
                _call("pag_composite_bwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(sigma), L.ptr(deltas), None, L.ptr(s3),
                      L.BG_BLACK, L.ptr(w), L.ptr(alpha), L.ptr(ones), None, None, L.ptr(d_sigma), L.ptr(d_rgb), 0, L.stream())
        return d_sigma, None, (d_feats if ctx.needs_input_grad[2] else None), None, None, None, None


def composite_features(sigma, deltas, feats, ridx, pack_start, ray_of_pack, N):
    """-> (out f32 [N,C], alpha f32 [N]) with gradients to sigma AND feats (delta-density tracer); ridx i32 [M]."""
    return _apply(_CompositeFeatsWeights, sigma, deltas, feats, ridx, pack_start, ray_of_pack, N)


CD_FUSED = os.environ.get("PAG_CD_FUSED", "1") != "0"      # density decoder + colour decoder in one launch (pag_mlp_fwd_args.x1_producer)


def decoder_hold():
    """-> hold (_Launch): fused_mlp(..., hold=hold) prepares its launch and parks it in `hold` instead of issuing it; hand `hold` to the decoder that
    consumes its output (colour_and_density(..., producer=hold)), which carries it in its own launch or issues it first, and call flush_hold(hold)
    afterwards in any case (issues the parked launch if nobody took it)."""
    return _Launch("pag_mlp_fwd", bare=True)


def flush_hold(hold):
    if hold is not None:
        hold.issue()


HEAD_FWD_ONCE = os.environ.get("PAG_HEAD_FWD_ONCE", "1") != "0"      # wide softmax head: decoder + per-ray sum in one launch (0: statistics launch + pag_head_composite_fwd)
HEAD_FWD_ONCE_MIN_PER_RAY = int(os.environ.get("PAG_HEAD_FWD_ONCE_MIN_PER_RAY", "160"))      # average samples per ray from which the one-launch form is taken
TAIL_ZERO = False        # graphs.py: batches carry filler samples past pack_start[N] - per-sample tensors written pack by pack start as zeros
SAMPLES_HINT = None      # graphs.py: the REAL sample count expected in a padded batch (pag_head_composite_fwd picks its per-pack work split from it)


def _head_call(in_dim, out_act, out_dtype, grouped, need_grad, **kw):
    """The decoder request of head_composite(): a statistics-only forward where the head is a wide softmax (the probabilities are rebuilt from the last
    hidden layer), and a backward that hands the decoder its gradient in rank-1 form (_head_backward)."""
    return _DecoderCall(in_dim, out_act, L.MLP_MFMA_BF16, out_dtype, grouped, need_grad=need_grad, rank1=True, stats_only=True, **kw)


def _head_forward(call, needs_x1, x1, weights_w, alpha, ridx, pack_start, ray_of_pack, *wb):
    """Decoder, then the per-ray weighted sum -> (out f32 [N,C], _DecoderState)."""
    # wide softmax head: where the library can, the decoder's launch forms the per-ray sums itself (pag_mlp_fwd_args.composite) - the output
    # tensor and the compositing arguments are prepared first and ride in the request
    C = wb[len(wb) // 2 - 1].shape[0]
    M = x1.shape[1] if call.grouped is not None else x1.shape[0]
    P, N = ray_of_pack.shape[0], call.n_rays
    n_samples = int(M if SAMPLES_HINT is None else SAMPLES_HINT)
    pre = None
    # (one wave per SIMD holds a ray's 112 partial sums next to the 112 logits: worth it where rays are long - the dense march, 16 tiles per ray:
    # 288 -> 260 us per 2.1 M samples; with the ~3 tiles per ray of the voxel march the two-launch form is faster, 375 against 434 us per 2.2 M)
    if HEAD_FWD_ONCE and n_samples >= HEAD_FWD_ONCE_MIN_PER_RAY * P and C > 192 and P and M and call.out_act == L.ACT_SOFTMAX \
            and call.out_dtype == torch.bfloat16:
        pre = (weights_w.detach().contiguous(), alpha.detach().contiguous(),
               (torch.empty if _one_pack_per_ray(ray_of_pack, N) else torch.zeros)(N, C, device=x1.device))
        hc = call.composite = L.HeadCompositeArgs()
        hc.pack_start, hc.ray_of_pack, hc.P = L.ptr(pack_start), L.ptr(ray_of_pack), P
        hc.weights, hc.alpha, hc.out, hc.n_samples = L.ptr(pre[0]), L.ptr(pre[1]), L.ptr(pre[2]), n_samples
    probs, st = _mlp_forward(call, (needs_x1, False), x1, None, None, *wb)
    call.composite = None
    if st.composited:
        st.head = None
        st.hc = (pre[0], pre[1], ridx)
        return pre[2], st
    return _head_composite(st, probs, x1.device, C, weights_w, alpha, ridx, pack_start, ray_of_pack, N), st


def _head_composite(st, probs, dev, C, weights_w, alpha, ridx, pack_start, ray_of_pack, N):
    """The per-ray weighted sum of a head whose decoder launch has been issued: of probs [M,C], or (probs None) of the statistics-only form."""
    P, M = ray_of_pack.shape[0], st.M
    # both compositing kernels used below write a row for every pack (zeros for an empty one)
    full = M and _one_pack_per_ray(ray_of_pack, N) and (probs is None or C <= 16)
    out = (torch.empty if full else torch.zeros)(N, C, device=dev)
    weights_w = weights_w.detach().contiguous()
    alpha = alpha.detach().contiguous()
    if probs is None:
        # wide softmax head: the forward wrote only the softmax statistics; the per-ray sums are formed from
        # probabilities rebuilt on the fly (pag_head_composite_fwd) - the [M, C] tensor never exists
        hidden_last, W_last, b_last, stats = st.head
        st.head = None
        if P and M:
            _call("pag_head_composite_fwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(hidden_last), L.ptr(W_last),
                  L.ptr(b_last), C, L.ptr(stats), L.ptr(weights_w), L.ptr(alpha), L.ptr(out),
                  int(M if SAMPLES_HINT is None else SAMPLES_HINT), L.stream())
    elif P and M:
        _call("pag_composite_feats_fwd", L.ptr(pack_start), L.ptr(ray_of_pack), P, L.ptr(weights_w), L.ptr(alpha),
              L.ptr(probs), L.dtype_code(probs), C, L.ptr(out), L.stream())
    st.hc = (weights_w, alpha, ridx)
    return out


def _head_backward(st, saved, g, **kw):
    """-> (d x1, _, [dW], [db]): the upstream gradient goes to the decoder in rank-1 form, alpha[ray] * w_m * g[ray] (detached weights, :148-155);
    the kernel forms the product."""
    weights_w, alpha, ridx = st.hc
    return _mlp_backward(st, saved, None, rank1=(g.contiguous().float(), weights_w.contiguous(), ridx.contiguous(), alpha.contiguous().float()), **kw)


class _HeadComposite(torch.autograd.Function):
    """decoder (+ softmax) followed by the per-ray weighted sum of tracer :197-205, as ONE autograd node: the
    backward hands the decoder the gradient in rank-1 form (alpha * w_m * d out[ray]) so neither the [M,C] gradient
    nor a separate composite-backward launch exists."""

    @staticmethod
    def forward(ctx, call, x1, weights_w, alpha, ridx, pack_start, ray_of_pack, *wb):
        out, st = _head_forward(call, ctx.needs_input_grad[1], x1, weights_w, alpha, ridx, pack_start, ray_of_pack, *wb)
        _save(ctx, st)
        return out

    @staticmethod
    def backward(ctx, g):
        dx1, _, gW, gb = _head_backward(ctx.state, ctx.saved_tensors, g)
        return (None, dx1, None, None, None, None, None, *gW, *gb)


class _HeadCompositePair(torch.autograd.Function):
    """Two head_composite() decoders on the SAME grouped input (semantic + instance heads on the panoptic features) as one
    autograd node: the second decoder's backward adds its input gradient into the first one's tensor in place
    (pag_mlp_bwd_args.dx1_accumulate) instead of autograd summing two [8,M,8] tensors in a separate pass."""

    @staticmethod
    def forward(ctx, calls, x1, weights_w, alpha, ridx, pack_start, ray_of_pack, *wb):
        call_a, call_b, n_a = calls
        part_a, part_b = wb[:n_a], wb[n_a:]
        needs_x1 = ctx.needs_input_grad[1]
        # the second (narrow) decoder is prepared first and parked (call_b.park): where the library can, it is evaluated inside the first one's launch
        # (call_a.pair -> pag_mlp_fwd_args.pair: the features are read once); its compositing pass follows either way
        probs_b, st_b = _mlp_forward(call_b, (needs_x1, False), x1, None, None, *part_b)
        out_a, st_a = _head_forward(call_a, needs_x1, x1, weights_w, alpha, ridx, pack_start, ray_of_pack, *part_a)
        call_b.park.issue()
        out_b = _head_composite(st_b, probs_b, x1.device, part_b[len(part_b) // 2 - 1].shape[0], weights_w, alpha, ridx, pack_start, ray_of_pack,
                                call_b.n_rays)
        ctx.states = (st_a, st_b)          # the tensors stay in the states: saved tensors would add version-counter checks
        return out_a, out_b

    @staticmethod
    def backward(ctx, g_a, g_b):
        st_a, st_b = ctx.states
        # wide head first (it writes dx1), the narrow one accumulates.  Where the library can, the narrow head's backward rides in the wide
        # head's call (pag_mlp_bwd_args.pair: one read of the features, one write of the summed gradient): it is prepared first and parked.
        queue = []
        x1 = st_a.saved[0]
        dx = torch.empty(x1.shape, device=x1.device, dtype=x1.dtype) if st_a.needs[0] else None
        hold = _Launch("pag_mlp_bwd")
        _, _, gW_b, gb_b = _head_backward(st_b, st_b.saved, g_b, dx1_into=dx, wgrad_queue=queue, hold=hold if dx is not None else None)
        dx1, _, gW_a, gb_a = _head_backward(st_a, st_a.saved, g_a, wgrad_queue=queue, dx1_out=dx, pair=hold)
        hold.issue()                                # not paired after all: the narrow head's own launch, after the wide one
        if queue:                                   # both heads' weight gradients: one narrow + one wide + one finish launch
            _launch_wgrad(queue, queue[0]["dz"].shape[0])
        return (None, dx1, None, None, None, None, None, *gW_a, *gb_a, *gW_b, *gb_b)


def head_composite_pair(x1, heads, w, alpha, ridx, pack_start, ray_of_pack, N, out_dtype=torch.bfloat16, x1_grouped=None):
    """heads = ((weights, biases, in_dim), (weights, biases, in_dim)) -> (out_a, out_b), each as head_composite()."""
    (wa, ba, ia), (wb_, bb, ib) = heads
    need_grad = _need_grad(x1, w, alpha, ridx, pack_start, ray_of_pack, *wa, *ba, *wb_, *bb)
    parked = _Launch("pag_mlp_fwd")
    calls = (_head_call(ia, L.ACT_SOFTMAX, out_dtype, x1_grouped, need_grad, n_rays=N, pair=parked),
             _head_call(ib, L.ACT_SOFTMAX, out_dtype, x1_grouped, need_grad, n_rays=N, park=parked), len(wa) + len(ba))
    return _apply(_HeadCompositePair, calls, x1, w, alpha, ridx, pack_start, ray_of_pack, *wa, *ba, *wb_, *bb)


def head_composite(x1, weights, biases, w, alpha, ridx, pack_start, ray_of_pack, N, in_dim=None, out_act=L.ACT_NONE,
                   out_dtype=torch.bfloat16, x1_grouped=None):
    """alpha[ray] * sum_i w_i * act(decoder(x1))[i]  ->  f32 [N, out_dim]; ridx i32 [M] = ray of each sample."""
    if in_dim is None:
        in_dim = weights[0].shape[1]
    call = _head_call(in_dim, out_act, out_dtype, x1_grouped, _need_grad(x1, w, alpha, ridx, pack_start, ray_of_pack, *weights, *biases), n_rays=N)
    return _apply(_HeadComposite, call, x1, w, alpha, ridx, pack_start, ray_of_pack, *weights, *biases)


# --------------------------------------------------------------------------------------- render loss
_LOSS_WS = {}


class NllTerm:
    """One `weight * mean(-log(prob[n, target_n] + eps) / temperature * conf_n)` term of render_loss."""

    def __init__(self, prob, target, weight=1.0, temperature=1.0, conf=None, mean_over="valid"):
        assert mean_over in ("valid", "all")
        self.prob, self.target, self.weight, self.temperature, self.conf, self.mean_over = prob, target, weight, temperature, conf, mean_over


class _RenderLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, prob_a, prob_b, rgb_gt, rgb_weight, term_a, term_b, eps):
        src = rgb if rgb is not None else (prob_a if prob_a is not None else prob_b)
        _check_gpu(src)
        dev = src.device
        N = src.shape[0]
        f = lambda t: t.detach().contiguous().float() if t is not None else None
        rgb_c, gt_c = f(rgb), f(rgb_gt)
        if rgb_c is not None:
            rgb_c, gt_c = rgb_c.reshape(N, 3), gt_c.reshape(N, 3)
        targs, keep = [], [rgb_c, gt_c]
        for prob, t in ((prob_a, term_a), (prob_b, term_b)):
            if prob is None:
                targs += [None, 0, None, None, 0.0, 1.0, 0]
                continue
            p = f(prob).reshape(N, -1)
            tg = t.target.detach().reshape(-1).long().contiguous()
            cf = f(t.conf).reshape(-1) if t.conf is not None else None
            keep += [p, tg, cf]
            targs += [L.ptr(p), p.shape[1], L.ptr(tg), L.ptr(cf), float(t.weight), 1.0 / float(t.temperature), int(t.mean_over == "all")]
        key = (dev.type, dev.index)
        if key not in _LOSS_WS:
            _LOSS_WS[key] = torch.zeros(L.load().pag_render_loss_workspace_bytes(), device=dev, dtype=torch.uint8)
        out = torch.empty(6, device=dev)
        head = [L.ptr(rgb_c), L.ptr(gt_c), N, float(rgb_weight)]
        _call("pag_render_loss_fwd", *head, *targs, float(eps), L.ptr(_LOSS_WS[key]), L.ptr(out), L.stream())
        ctx.call = (head, targs, float(eps))
        ctx.keep = keep                      # plain tensors (detached copies / inputs), not autograd-tracked
        ctx.out = out
        ctx.shapes = tuple(None if t is None else (t.shape, t.dtype) for t in (rgb, prob_a, prob_b))
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return out[0], out

    @staticmethod
    def backward(ctx, g, _g_terms):
        head, targs, eps = ctx.call
        dev = ctx.out.device
        if g is None:
            return (None,) * 8
        grads = []
        for need, sh in zip(ctx.needs_input_grad[:3], ctx.shapes):
            grads.append(torch.empty(sh[0], device=dev) if (need and sh is not None) else None)
        g = g.detach().float().contiguous()
        _call("pag_render_loss_bwd", L.ptr(g), L.ptr(ctx.out), *head, *targs, eps, L.ptr(grads[0]), L.ptr(grads[1]), L.ptr(grads[2]), L.stream())
        grads = [None if d is None else (d if sh[1] == torch.float32 else d.to(sh[1])) for d, sh in zip(grads, ctx.shapes)]
        return grads[0], grads[1], grads[2], None, None, None, None, None


def render_loss(rgb=None, rgb_gt=None, rgb_weight=1.0, term_a=None, term_b=None, eps=1e-27):
    """-> (loss 0-dim, terms f32 [6] = total, rgb, A, B, denom A, denom B - detached).  The trainer's per-ray objective
    (pc_nerf/trainer.py:443-446, :459-465, loss/lin_assignment_things.py:80) as one launch forward and one backward."""
    if rgb is None and term_a is None and term_b is None:
        raise ValueError("render_loss needs at least one term")
    return _RenderLoss.apply(rgb, term_a.prob if term_a is not None else None, term_b.prob if term_b is not None else None,
                             rgb_gt, rgb_weight, term_a, term_b, eps)


# ------------------------------------------------------------------------------------------- map export (csrc/map.hip)
def _map_inst(name, n, inst, ids):
    """-> (inst pointer, I, row stride, ids pointer, tensors to keep alive) for the instance-id arguments of pag_map_points / pag_map_select."""
    if inst is not None and ids is not None:
        raise RuntimeError("%s: give either inst or ids" % name)
    if inst is not None:
        if inst.dim() != 2 or inst.shape[0] != n:
            raise RuntimeError("%s: inst must be [n, I], got %s" % (name, tuple(inst.shape)))
        inst = inst.detach()
        if inst.dtype != torch.float32:
            inst = inst.float()
        if (inst.shape[1] > 1 and inst.stride(1) != 1) or (n > 1 and inst.stride(0) < inst.shape[1]):
            inst = inst.contiguous()
        return inst.data_ptr(), inst.shape[1], (inst.stride(0) if n > 1 else inst.shape[1]), None, (inst,)
    if ids is not None:
        if ids.dtype != torch.int64 or ids.numel() != n:
            raise RuntimeError("%s: ids must be int64 [n]" % name)
        ids = ids.detach().reshape(-1).contiguous()
        return None, 0, 0, ids.data_ptr(), (ids,)
    return None, 0, 0, None, ()


def _workspace(size_fn, n, dev):
    """The scratch buffer of an ordered append over n rows; size_fn names the library's pag_*_workspace_bytes function."""
    return torch.empty(max(int(getattr(L.load(), size_fn)(n)), 8), dtype=torch.uint8, device=dev)


def _bad_columns(cols):
    """cols: [(tensor, dtype, shape)] -> True when one is missing, of another dtype or shape, or not contiguous."""
    return any(t is None or t.dtype != d or tuple(t.shape) != s or not t.is_contiguous() for t, d, s in cols)


def _ignore_array(ignore):
    """An ignore list -> (c_int64 array of at least one element, its length)."""
    ignore = [int(v) for v in ignore]
    return (ctypes.c_int64 * max(1, len(ignore)))(*ignore), len(ignore)


def map_points(params, cam, rays_per_camera, origins_c, dirs_c, ray0, depth, alpha, hit, density, rgb, points, color, ids_out, count, inst=None,
               ids=None, min_density=40.0, min_alpha=0.9, depth_min=0.6, depth_max=0.8):
    """utils/render_map.py:107-120 on one rendered chunk: the kept rays' world points, colours and instance ids appended in ray order to
    points / color f32 [cap,3] and ids_out i64 [cap] behind the device counter `count` i64 [1] (pag_map_points; no host synchronisation)."""
    _check_gpu(params, cam, origins_c, dirs_c, depth, alpha, hit, density, rgb, points, color, ids_out, count, inst, ids)
    n = depth.numel()
    if n == 0:
        return
    if alpha.numel() != n or hit.numel() != n or density.numel() != n or rgb.numel() != 3 * n:
        raise RuntimeError("map_points: depth / alpha / hit / density [n] and rgb [n,3] must describe the same rays")
    if cam.dtype != torch.int32 or params.dim() != 2 or params.shape[1] != 9 or origins_c.shape != dirs_c.shape or origins_c.shape != (rays_per_camera, 3):
        raise RuntimeError("map_points: cam must be int32, params [C,9], base rays [rays_per_camera,3]")
    if hit.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("map_points: hit must be bool / uint8")
    if points.dtype != torch.float32 or color.dtype != torch.float32 or ids_out.dtype != torch.int64 or count.dtype != torch.int64:
        raise RuntimeError("map_points: points / color f32, ids_out / count int64")
    cap = points.shape[0]
    if color.shape[0] != cap or ids_out.shape[0] != cap or not (points.is_contiguous() and color.is_contiguous() and ids_out.is_contiguous()):
        raise RuntimeError("map_points: points [cap,3], color [cap,3], ids_out [cap], contiguous")
    f = lambda t: t.detach().reshape(-1).contiguous().float()                      # noqa: E731
    prm, oc, dc = params.detach().contiguous().float(), origins_c.detach().contiguous().float(), dirs_c.detach().contiguous().float()
    dep, alp, den, col, h = f(depth), f(alpha), f(density), f(rgb), hit.detach().reshape(-1).contiguous()
    ip, I, stride, idp, keep = _map_inst("map_points", n, inst, ids)
    if ip is None and idp is None:
        raise RuntimeError("map_points: needs inst or ids")
    cam = cam.contiguous()
    ws = _workspace("pag_map_workspace_bytes", n, dep.device)
    _call("pag_map_points", prm.data_ptr(), prm.shape[0], cam.data_ptr(), cam.numel(), int(rays_per_camera), oc.data_ptr(), dc.data_ptr(), int(ray0), n,
          dep.data_ptr(), alp.data_ptr(), h.data_ptr(), den.data_ptr(), col.data_ptr(), ip, I, stride, idp, float(min_density), float(min_alpha),
          float(depth_min), float(depth_max), points.data_ptr(), color.data_ptr(), ids_out.data_ptr(), cap, count.data_ptr(), ws.data_ptr(), ws.numel(),
          L.stream())


def map_select(points_in, points, count, value=None, threshold=0.0, inst=None, ids=None, ids_out=None):
    """utils/render_map.py:77-79 / :160-165: rows of points_in f32 [n,3] with value > threshold (or, without value, with instance id != 0)
    appended in row order to points f32 [cap,3] (and their ids to ids_out i64 [cap]) behind the device counter (pag_map_select)."""
    _check_gpu(points_in, points, count, value, inst, ids, ids_out)
    n = points_in.shape[0]
    if n == 0:
        return
    if points_in.dim() != 2 or points_in.shape[1] != 3 or (value is not None and value.numel() != n):
        raise RuntimeError("map_select: points_in [n,3], value [n]")
    if points.dtype != torch.float32 or count.dtype != torch.int64 or not points.is_contiguous() or (ids_out is not None and (
            ids_out.dtype != torch.int64 or ids_out.shape[0] != points.shape[0] or not ids_out.is_contiguous())):
        raise RuntimeError("map_select: points f32 [cap,3], ids_out int64 [cap], count int64 [1]")
    pin = points_in.detach().contiguous().float()
    val = value.detach().reshape(-1).contiguous().float() if value is not None else None
    ip, I, stride, idp, keep = _map_inst("map_select", n, inst, ids)
    if val is None and ip is None and idp is None:
        raise RuntimeError("map_select: needs value, inst or ids")
    ws = _workspace("pag_map_workspace_bytes", n, pin.device)
    _call("pag_map_select", pin.data_ptr(), n, val.data_ptr() if val is not None else None, float(threshold), ip, I, stride, idp, points.data_ptr(),
          ids_out.data_ptr() if ids_out is not None else None, points.shape[0], count.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())


# ------------------------------------------------------------------------------------------- surface-mesh export (csrc/mesh.hip)
def _mesh_lattice(name, field, cell_vertex):
    """-> (nx, ny, nz, workspace) of the lattice `field` f32 [nx,ny,nz] with its cell table i32 [(nx-1)(ny-1)(nz-1)]; refuses what the library refuses."""
    if field.dim() != 3 or field.dtype != torch.float32 or not field.is_contiguous():
        raise RuntimeError("%s: field must be f32 [nx,ny,nz], contiguous, got %s %s" % (name, field.dtype, tuple(field.shape)))
    nx, ny, nz = (int(s) for s in field.shape)
    need = int(L.load().pag_mesh_workspace_bytes(nx, ny, nz))
    if need == 0:
        raise RuntimeError("%s: lattice %d x %d x %d: every axis needs 2 points, fewer than 2^31 cells and 2^32 / 3 points" % (name, nx, ny, nz))
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    if cell_vertex.dtype != torch.int32 or cell_vertex.numel() != cells or not cell_vertex.is_contiguous():
        raise RuntimeError("%s: cell_vertex must be int32 with the lattice's %d cells, contiguous" % (name, cells))
    return nx, ny, nz, torch.empty(need, dtype=torch.uint8, device=field.device)


def mesh_vertices(field, iso, lo, h, index0, vertices, normals, cell_vertex, count):
    """Surface nets, the vertices: the active cells of field f32 [nx,ny,nz] in cell order -> their vertex and normal appended to vertices / normals
    f32 [cap,3] (None, None: count only) behind the device counter `count` i64 [1], and every cell's slot (-1: no vertex) in cell_vertex i32
    [nx-1,ny-1,nz-1] (pag_mesh_vertices; lo three floats, h a float, index0 three ints are host values; no host synchronisation)."""
    _check_gpu(field, vertices, normals, cell_vertex, count)
    nx, ny, nz, ws = _mesh_lattice("mesh_vertices", field, cell_vertex)
    cap = 0 if vertices is None else vertices.shape[0]
    if count.dtype != torch.int64 or (vertices is None) != (normals is None) or (vertices is not None and _bad_columns(
            [(vertices, torch.float32, (cap, 3)), (normals, torch.float32, (cap, 3))])):
        raise RuntimeError("mesh_vertices: vertices / normals f32 [cap,3], contiguous; count int64 [1]")
    lo3, idx3 = (ctypes.c_float * 3)(*[float(v) for v in lo]), (ctypes.c_int * 3)(*[int(v) for v in index0])
    _call("pag_mesh_vertices", field.data_ptr(), nx, ny, nz, float(iso), lo3, float(h), idx3, _ptr(vertices), _ptr(normals), cap, cell_vertex.data_ptr(),
          count.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())


def mesh_faces(field, iso, cell_vertex, faces, count):
    """Surface nets, the faces: the sign-changing lattice edges of `field` whose four cells have a vertex in cell_vertex (as mesh_vertices wrote it),
    in edge-row order -> two triangles each, appended to faces i32 [cap,3] (None: count only) behind the device counter `count` i64 [1], which counts
    quads (pag_mesh_faces; no host synchronisation)."""
    _check_gpu(field, cell_vertex, faces, count)
    nx, ny, nz, ws = _mesh_lattice("mesh_faces", field, cell_vertex)
    cap = 0 if faces is None else faces.shape[0]
    if count.dtype != torch.int64 or (faces is not None and _bad_columns([(faces, torch.int32, (cap, 3))])):
        raise RuntimeError("mesh_faces: faces int32 [cap,3], contiguous; count int64 [1]")
    _call("pag_mesh_faces", field.data_ptr(), nx, ny, nz, float(iso), cell_vertex.data_ptr(), _ptr(faces), cap, count.data_ptr(), ws.data_ptr(), ws.numel(),
          L.stream())


# ------------------------------------------------------------------------------------------- voxel map fusion (csrc/voxelmap.hip)
def voxel_keys(points, origin, voxel_size, limits=None):
    """points f32 [n,3] -> keys i64 [n]: iz | iy << 21 | ix << 42 with i = floor((p - origin) / voxel_size) in fp32, INT64_MAX for a row that is not
    finite, outside [0, 2^21) on an axis or not strictly inside limits [[min], [max]] (pag_voxel_keys; origin / limits are host values)."""
    _check_gpu(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("voxel_keys: points [n,3], got %s" % (tuple(points.shape),))
    n = points.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device=points.device)
    pts = points.detach().contiguous().float()
    org = (ctypes.c_float * 3)(*[float(v) for v in origin])
    lim = None
    if limits is not None:
        flat = [float(v) for v in torch.as_tensor(limits, dtype=torch.float32).reshape(-1).tolist()]
        if len(flat) != 6:
            raise RuntimeError("voxel_keys: limits must be [2,3] = [[min], [max]]")
        lim = (ctypes.c_float * 6)(*flat)
    _call("pag_voxel_keys", pts.data_ptr(), n, org, float(voxel_size), lim, keys.data_ptr(), L.stream())
    return keys


def voxel_fuse(keys, ids, points, color, min_votes, points_out, color_out, ids_out, count_out, agreement, voxels, count):
    """Rows ordered by (key, id) -> one row per run of equal keys with at least min_votes rows, appended in key order behind the device counter
    `count` i64 [1]: mean point / colour, the most frequent id (ties: the smaller), the rows, the winner's share, the voxel index (pag_voxel_fuse)."""
    _check_gpu(keys, ids, points, color, points_out, color_out, ids_out, count_out, agreement, voxels, count)
    n = keys.numel()
    if n == 0:
        return
    if keys.dtype != torch.int64 or ids.dtype != torch.int64 or ids.numel() != n or tuple(points.shape) != (n, 3) or points.dtype != torch.float32 or (
            color is not None and (tuple(color.shape) != (n, 3) or color.dtype != torch.float32)):
        raise RuntimeError("voxel_fuse: keys / ids int64 [n], points / color f32 [n,3]")
    cap = points_out.shape[0]
    outs = [(points_out, torch.float32, (cap, 3)), (ids_out, torch.int64, (cap,)), (count_out, torch.int32, (cap,)), (agreement, torch.float32, (cap,)),
            (voxels, torch.int32, (cap, 3))] + ([(color_out, torch.float32, (cap, 3))] if color is not None else [])
    if count.dtype != torch.int64 or _bad_columns(outs):
        raise RuntimeError("voxel_fuse: points_out / color_out f32 [cap,3], ids_out int64 [cap], count_out int32 [cap], agreement f32 [cap], "
                           "voxels int32 [cap,3], contiguous; count int64 [1]")
    keys, ids, points = keys.contiguous(), ids.contiguous(), points.contiguous()
    color = color.contiguous() if color is not None else None
    ws = _workspace("pag_voxel_workspace_bytes", n, keys.device)
    _call("pag_voxel_fuse", keys.data_ptr(), ids.data_ptr(), points.data_ptr(), color.data_ptr() if color is not None else None, n, int(min_votes),
          points_out.data_ptr(), color_out.data_ptr() if color is not None else None, ids_out.data_ptr(), count_out.data_ptr(), agreement.data_ptr(),
          voxels.data_ptr(), cap, count.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())


def label_table(labels, points, color, voxel_count, ignore, ids_out, voxels_out, observations, centroid, bbox_min, bbox_max, color_out, count):
    """Voxel rows ordered by label -> one row per run of a label outside `ignore`, appended in label order behind the device counter: the label, its
    voxels, the sum of voxel_count, the centroid, the bounding box and the mean colour (pag_label_table)."""
    _check_gpu(labels, points, color, voxel_count, ids_out, voxels_out, observations, centroid, bbox_min, bbox_max, color_out, count)
    n = labels.numel()
    if n == 0:
        return
    if labels.dtype != torch.int64 or tuple(points.shape) != (n, 3) or points.dtype != torch.float32 or voxel_count.dtype != torch.int32 or (
            voxel_count.numel() != n) or (color is not None and (tuple(color.shape) != (n, 3) or color.dtype != torch.float32)):
        raise RuntimeError("label_table: labels int64 [n], points / color f32 [n,3], voxel_count int32 [n]")
    cap = ids_out.shape[0]
    outs = [(t, torch.int64, (cap,)) for t in (ids_out, voxels_out, observations)] + [(t, torch.float32, (cap, 3)) for t in (centroid, bbox_min, bbox_max)]
    outs += [(color_out, torch.float32, (cap, 3))] if color is not None else []
    if count.dtype != torch.int64 or _bad_columns(outs):
        raise RuntimeError("label_table: ids_out / voxels_out / observations int64 [cap], centroid / bbox_min / bbox_max / color_out f32 [cap,3], "
                           "contiguous; count int64 [1]")
    ign, n_ignore = _ignore_array(ignore)
    labels, points, voxel_count = labels.contiguous(), points.contiguous(), voxel_count.contiguous()
    color = color.contiguous() if color is not None else None
    ws = _workspace("pag_voxel_workspace_bytes", n, labels.device)
    _call("pag_label_table", labels.data_ptr(), points.data_ptr(), color.data_ptr() if color is not None else None, voxel_count.data_ptr(), n, ign,
          n_ignore, ids_out.data_ptr(), voxels_out.data_ptr(), observations.data_ptr(), centroid.data_ptr(), bbox_min.data_ptr(),
          bbox_max.data_ptr(), color_out.data_ptr() if color is not None else None, cap, count.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())


def voxel_components(voxels, ids, connectivity, same_id, ignore, component, count_status):
    """The connected components of a fused map's rows (voxels i32 [n,3] ascending by key, ids i64 [n]) -> component i64 [n] (1 .. C by first row, 0
    for an ignored id); count_status i64 [2] receives (C, status word), both overwritten (pag_voxel_components).  No synchronisation."""
    _check_gpu(voxels, ids, component, count_status)
    n = ids.numel()
    if voxels.dtype != torch.int32 or tuple(voxels.shape) != (n, 3) or ids.dtype != torch.int64 or ids.dim() != 1:
        raise RuntimeError("voxel_components: voxels int32 [n,3], ids int64 [n]")
    if component.dtype != torch.int64 or tuple(component.shape) != (n,) or not component.is_contiguous() or count_status.dtype != torch.int64 or (
            tuple(count_status.shape) != (2,)) or not count_status.is_contiguous():
        raise RuntimeError("voxel_components: component int64 [n], count_status int64 [2], contiguous")
    count_status.zero_()                                                                   # the status is an int32 word: its slot's upper half stays zero
    if n == 0:
        return
    ign, n_ignore = _ignore_array(ignore)
    voxels, ids = voxels.contiguous(), ids.contiguous()
    ws = _workspace("pag_voxel_components_workspace_bytes", n, ids.device)
    _call("pag_voxel_components", voxels.data_ptr(), ids.data_ptr(), n, int(connectivity), int(bool(same_id)), ign, n_ignore, ws.data_ptr(), ws.numel(),
          component.data_ptr(), count_status.data_ptr(), count_status.data_ptr() + 8, L.stream())


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() > 0 else None


def voxel_overlap(voxels_a, ids_a, uniq_a, voxels_b, ids_b, uniq_b, status, combine=True):
    """The join of two fused maps' rows (voxels i32 [n,3] ascending by key, ids i64 [n], uniq i64 [T] the distinct ids ascending) ->
    {'keys_a', 'keys_b' i64 [n], 'slot_a', 'slot_b' i32 [n], 'table' i32 [Ta,Tb]}; status i32 [1] is overwritten
    with the contract bits (pag_voxel_overlap).  No synchronisation."""
    _check_gpu(voxels_a, ids_a, uniq_a, voxels_b, ids_b, uniq_b, status)
    na, nb, Ta, Tb = ids_a.numel(), ids_b.numel(), uniq_a.numel(), uniq_b.numel()
    for v, i, u in ((voxels_a, ids_a, uniq_a), (voxels_b, ids_b, uniq_b)):
        if v.dtype != torch.int32 or tuple(v.shape) != (i.numel(), 3) or i.dtype != torch.int64 or i.dim() != 1 or u.dtype != torch.int64 or u.dim() != 1:
            raise RuntimeError("voxel_overlap: voxels int32 [n,3], ids int64 [n], uniq int64 [T]")
    if status.dtype != torch.int32 or status.numel() != 1:
        raise RuntimeError("voxel_overlap: status int32 [1]")
    dev = status.device
    out = {"keys_a": torch.empty(na, dtype=torch.int64, device=dev), "keys_b": torch.empty(nb, dtype=torch.int64, device=dev),
           "slot_a": torch.empty(na, dtype=torch.int32, device=dev), "slot_b": torch.empty(nb, dtype=torch.int32, device=dev),
           "table": torch.zeros(Ta, Tb, dtype=torch.int32, device=dev)}
    voxels_a, ids_a, uniq_a, voxels_b, ids_b, uniq_b = (t.contiguous() for t in (voxels_a, ids_a, uniq_a, voxels_b, ids_b, uniq_b))
    _call("pag_voxel_overlap", _ptr(voxels_a), _ptr(ids_a), na, _ptr(uniq_a), Ta, _ptr(voxels_b), _ptr(ids_b), nb, _ptr(uniq_b), Tb, int(bool(combine)),
          _ptr(out["keys_a"]), _ptr(out["slot_a"]), _ptr(out["keys_b"]), _ptr(out["slot_b"]), _ptr(out["table"]), status.data_ptr(), L.stream())
    return out


def overlap_cost(table, row_sum, col_sum, act_a, act_b):
    """table i32 [Ta,Tb] with its sums i64 [Ta] / [Tb] and the active positions act_a / act_b i32 -> (iou f32 [Ta,Tb], cost f32 [R,C], transposed):
    the fp32 IoU of every entry and 1 - IoU of the active sub-matrix with R = min(n_a, n_b) rows, b's ids as rows when transposed (pag_overlap_cost)."""
    _check_gpu(table, row_sum, col_sum, act_a, act_b)
    Ta, Tb = table.shape
    n_a, n_b = act_a.numel(), act_b.numel()
    if table.dtype != torch.int32 or row_sum.dtype != torch.int64 or col_sum.dtype != torch.int64 or row_sum.numel() != Ta or col_sum.numel() != Tb or (
            act_a.dtype != torch.int32 or act_b.dtype != torch.int32):
        raise RuntimeError("overlap_cost: table int32 [Ta,Tb], row_sum int64 [Ta], col_sum int64 [Tb], act_a / act_b int32")
    transposed = n_a > n_b
    iou = torch.empty(Ta, Tb, dtype=torch.float32, device=table.device)
    cost = torch.empty(min(n_a, n_b), max(n_a, n_b), dtype=torch.float32, device=table.device)
    table, row_sum, col_sum, act_a, act_b = (t.contiguous() for t in (table, row_sum, col_sum, act_a, act_b))
    _call("pag_overlap_cost", _ptr(table), _ptr(row_sum), _ptr(col_sum), Ta, Tb, _ptr(act_a), n_a, _ptr(act_b), n_b, _ptr(iou), _ptr(cost), L.stream())
    return iou, cost, transposed


def voxel_merge(keys, order, a, b, slot_b, mapping, out, count, status):
    """The rows of two fused maps (a, b: dicts of 'points', 'instances' (a only), 'count', 'agreement', 'voxels', optionally 'color'), given both maps'
    keys sorted stably and that sort's permutation, merged into the columns of `out` in key order behind the device counter `count` i64 [1]; b's ids
    are mapping[slot_b]; colour is merged when out has 'color'; status i32 [1] is ORed into (pag_voxel_merge).  No synchronisation."""
    cols = [a[k] for k in ("points", "instances", "count", "agreement", "voxels")] + [b[k] for k in ("points", "count", "agreement", "voxels")]
    _check_gpu(keys, order, slot_b, mapping, count, status, *cols, *out.values())
    na, nb = a["count"].numel(), b["count"].numel()
    n, cap = na + nb, out["points"].shape[0]
    if n == 0:
        return
    color = "color" in out
    want = [(keys, torch.int64, (n,)), (order, torch.int64, (n,)), (slot_b, torch.int32, (nb,)), (a["instances"], torch.int64, (na,))]
    for m, k in ((a, na), (b, nb), (out, cap)):
        want += [(m["points"], torch.float32, (k, 3)), (m["count"], torch.int32, (k,)), (m["agreement"], torch.float32, (k,)), (m["voxels"], torch.int32, (k, 3))]
        want += [(m.get("color"), torch.float32, (k, 3))] if color else []
    want += [(out["instances"], torch.int64, (cap,))]
    if _bad_columns(want) or mapping.dtype != torch.int64 or (
            not mapping.is_contiguous()) or count.dtype != torch.int64 or status.dtype != torch.int32:
        raise RuntimeError("voxel_merge: keys / order int64 [na + nb], slot_b int32 [nb], mapping int64 [Tb]; per map points / color f32 [n,3], instances "
                           "int64 [n], count int32 [n], agreement f32 [n], voxels int32 [n,3], contiguous; count int64 [1], status int32 [1]")
    ws = _workspace("pag_voxel_workspace_bytes", n, keys.device)
    _call("pag_voxel_merge", keys.data_ptr(), order.data_ptr(), na, nb, _ptr(a["points"]), _ptr(a.get("color")) if color else None, _ptr(a["instances"]),
          _ptr(a["count"]), _ptr(a["agreement"]), _ptr(a["voxels"]), _ptr(b["points"]), _ptr(b.get("color")) if color else None, _ptr(slot_b), _ptr(mapping),
          mapping.numel(), _ptr(b["count"]), _ptr(b["agreement"]), _ptr(b["voxels"]), _ptr(out["points"]), _ptr(out.get("color")), _ptr(out["instances"]),
          _ptr(out["count"]), _ptr(out["agreement"]), _ptr(out["voxels"]), cap, count.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), L.stream())


def sample_copy_width(src_ptr, dst_ptr, row_bytes, convert=L.SAMPLE_COPY):
    """Bytes per copy element pag_sample_batch uses for a mode with these base addresses and destination row size (16 / 8 / 4 / 2 / 1; for the uint8 -> f32
    conversion 4 or 1 source bytes per step); 0 = the mode would be refused.  Host arithmetic only."""
    return L.load().pag_sample_copy_width(src_ptr, dst_ptr, int(row_bytes), int(convert))


def sample_mode_array(modes):
    """[(src tensor, dst tensor, destination row bytes, per_view, convert)] -> ctypes array of pag_sample_mode."""
    if len(modes) > L.SAMPLE_MAX_MODES:
        raise RuntimeError("sample_batch: %d modes, at most %d per launch" % (len(modes), L.SAMPLE_MAX_MODES))
    arr = (L.SampleMode * max(1, len(modes)))()
    for a, (src, dst, row_bytes, per_view, convert) in zip(arr, modes):
        _check_gpu(src, dst)
        if not (src.is_contiguous() and dst.is_contiguous()):
            raise RuntimeError("sample_batch: modes and outputs must be contiguous")
        a.src, a.dst, a.row_bytes, a.per_view, a.convert = src.data_ptr(), dst.data_ptr(), int(row_bytes), int(bool(per_view)), int(convert)
    return arr


def sample_batch(state, views, num_views, n, k, slot_begin, slot_count, modes, ray_idx=None, cam_idx=None):
    """datasets/transforms/ray_sampler.py:17-40 + the collation of datasets/multiview_dataset.py:177-192 as one launch (pag_sample_batch): for each of
    the B views (device int32 [B]) slots [slot_begin, slot_begin + slot_count) of the keyed permutation of [0, n) under the device state int64 [2] =
    {seed, draw}, and the rows of every mode at those pixels.  modes: a ctypes array from sample_mode_array (with its length) or the list it takes."""
    _check_gpu(state, views, ray_idx, cam_idx)
    if state.dtype != torch.int64 or state.numel() != 2 or views.dtype != torch.int32 or views.dim() != 1 or not views.is_contiguous():
        raise RuntimeError("sample_batch: state int64 [2], views int32 [B]")
    B = views.shape[0]
    if (ray_idx is not None and (ray_idx.dtype != torch.int64 or ray_idx.numel() != B * slot_count or not ray_idx.is_contiguous())) or \
            (cam_idx is not None and (cam_idx.dtype != torch.int32 or cam_idx.numel() != B * slot_count or not cam_idx.is_contiguous())):
        raise RuntimeError("sample_batch: ray_idx int64 [B, slot_count], cam_idx int32 [B * slot_count]")
    arr, n_modes = modes if isinstance(modes, tuple) else (sample_mode_array(modes), len(modes))
    _call("pag_sample_batch", state.data_ptr(), views.data_ptr(), B, int(num_views), int(n), int(k), int(slot_begin), int(slot_count), arr, n_modes,
          ray_idx.data_ptr() if ray_idx is not None else None, cam_idx.data_ptr() if cam_idx is not None else None, L.stream())


def sample_advance(state):
    """state[1] += 1 on the device (pag_sample_advance): the next draw, inside a captured graph too."""
    _check_gpu(state)
    if state.dtype != torch.int64 or state.numel() != 2:
        raise RuntimeError("sample_advance: state int64 [2]")
    _call("pag_sample_advance", state.data_ptr(), L.stream())


def _prepare_sizes(name, src, mip, planes_dims):
    mip = int(mip)
    if not 0 <= mip <= 8:
        raise RuntimeError("%s: mip %d not in [0, 8]" % (name, mip))
    if src.dtype != torch.uint8 or src.dim() != planes_dims or not src.is_contiguous():
        raise RuntimeError("%s: the source is a contiguous uint8 tensor of %d axes, got %s %s" % (name, planes_dims, src.dtype, tuple(src.shape)))
    B, H0, W0 = src.shape[:3]
    f = 1 << mip
    if H0 % f or W0 % f:
        raise RuntimeError("%s: source size %d x %d is not divisible by 2^mip = %d" % (name, H0, W0, f))
    return mip, B, H0, W0, H0 // f, W0 // f


def _prepare_dst(name, what, t, dtype, V, h, w, C, view_offset, B):
    if t is None:
        return V
    _check_gpu(t)
    if t.dtype != dtype or t.dim() != 4 or tuple(t.shape[1:]) != (h, w, C) or not t.is_contiguous():
        raise RuntimeError("%s: %s is a contiguous %s [V, %d, %d, %d], got %s %s" % (name, what, dtype, h, w, C, t.dtype, tuple(t.shape)))
    if V is not None and t.shape[0] != V:
        raise RuntimeError("%s: %s holds %d views, the other outputs %d" % (name, what, t.shape[0], V))
    if view_offset < 0 or view_offset + B > t.shape[0]:
        raise RuntimeError("%s: views [%d, %d) outside %s's [0, %d)" % (name, view_offset, view_offset + B, what, t.shape[0]))
    return t.shape[0]


def prepare_views(src_u8, mip, bg_color, view_offset=0, imgs=None, masks=None, origins=None, dirs=None, c2w=None, intrinsics=None):
    """datasets/formats/nerf_standard.py:57-60 and :239-282 for the decoded frames of a chunk, as one launch (pag_prepare_views): src_u8 uint8
    [B, H0, W0, 3 or 4] on the GPU -> views [view_offset, view_offset + B) of the requested outputs, each the whole dataset's tensor: imgs f32 [V, h, w, 3],
    masks bool (or uint8) [V, h, w, 1], origins / dirs f32 [V, h, w, 3].  The rays need c2w f32 [V, 3, 4] (of the DESTINATION views) and
    intrinsics = (fx, fy, x0, y0) at the output size.  pagnerf_amd.formats holds the definition."""
    name = "prepare_views"
    _check_gpu(src_u8, c2w)
    view_offset = int(view_offset)
    mip, B, H0, W0, h, w = _prepare_sizes(name, src_u8, mip, 4)
    C0 = src_u8.shape[3]
    if C0 not in (3, 4):
        raise RuntimeError("%s: %d source channels, 3 or 4 expected" % (name, C0))
    if bg_color not in ("white", "black"):
        raise RuntimeError("%s: bg_color %r is neither 'white' nor 'black'" % (name, bg_color))
    if masks is not None and masks.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("%s: masks is bool or uint8, got %s" % (name, masks.dtype))
    V = _prepare_dst(name, "imgs", imgs, torch.float32, None, h, w, 3, view_offset, B)
    V = _prepare_dst(name, "masks", masks, masks.dtype if masks is not None else None, V, h, w, 1, view_offset, B)
    V = _prepare_dst(name, "origins", origins, torch.float32, V, h, w, 3, view_offset, B)
    V = _prepare_dst(name, "dirs", dirs, torch.float32, V, h, w, 3, view_offset, B)
    if V is None:
        return
    fx = fy = x0 = y0 = 0.0
    if origins is not None or dirs is not None:
        if c2w is None or c2w.dtype != torch.float32 or tuple(c2w.shape) != (V, 3, 4) or not c2w.is_contiguous():
            raise RuntimeError("%s: the rays need c2w, a contiguous f32 [%d, 3, 4]" % (name, V))
        if dirs is not None:
            if intrinsics is None or len(intrinsics) != 4:
                raise RuntimeError("%s: dirs needs intrinsics = (fx, fy, x0, y0)" % name)
            fx, fy, x0, y0 = (float(v) for v in intrinsics)
    p = lambda t: t.data_ptr() if t is not None else None
    _call("pag_prepare_views", src_u8.data_ptr(), B, H0, W0, C0, mip, L.BG_WHITE if bg_color == "white" else L.BG_BLACK, p(c2w), fx, fy, x0, y0, view_offset, V,
          p(imgs), p(masks), p(origins), p(dirs), L.stream())


def prepare_labels(planes, mip, view_offset=0):
    """datasets/formats/bup20.py:203-229 (nearest resample at an integer factor) for every label plane of a chunk in one launch (pag_prepare_labels):
    planes = [(src uint8 [B, H0, W0], dst int64 [V, h, w, 1])] on the GPU; dst[view_offset + b, y, x] = src[b, y * 2^mip, x * 2^mip]."""
    name = "prepare_labels"
    view_offset = int(view_offset)
    if len(planes) > L.PREPARE_MAX_PLANES:
        raise RuntimeError("%s: %d planes, at most %d per launch" % (name, len(planes), L.PREPARE_MAX_PLANES))
    if not planes:
        return
    arr = (L.LabelPlane * len(planes))()
    size, V = None, None
    for a, (src, dst) in zip(arr, planes):
        _check_gpu(src, dst)
        mip, B, H0, W0, h, w = _prepare_sizes(name, src, mip, 3)
        if size is not None and (B, H0, W0) != size:
            raise RuntimeError("%s: planes of different sizes, %s and %s" % (name, size, (B, H0, W0)))
        size = (B, H0, W0)
        V = _prepare_dst(name, "a destination", dst, torch.int64, V, h, w, 1, view_offset, B)
        a.src, a.dst = src.data_ptr(), dst.data_ptr()
    B, H0, W0 = size
    _call("pag_prepare_labels", arr, len(planes), B, H0, W0, mip, view_offset, V, L.stream())


# ------------------------------------------------------------------------------------------- BUP20 loader
_COCO_ARRAYS = ("verts", "part_vert_begin", "point_begin", "part_key_begin", "part_key_count", "keys", "ann_part_begin", "ann_label", "ann_cover", "cand",
                "frame_ann_begin", "frame_labelled")


class CocoDeviceTables:
    """The tables of bup20.coco_tables on the GPU: the tensors (kept alive here) and the pag_coco_tables struct that points at them."""

    def __init__(self, tensors, max_part_keys):
        self.tensors = tensors
        n = {k: t.numel() for k, t in tensors.items()}
        self.B, n_parts, n_anns = n["frame_labelled"], n["part_key_count"], n["ann_label"]
        if (n["part_vert_begin"], n["part_key_begin"], n["ann_part_begin"], n["ann_cover"], n["frame_ann_begin"], n["point_begin"]) != \
                (n_parts + 1, n_parts + 1, n_anns + 1, n_anns, self.B + 1, n["verts"] // 2 + 1):
            raise RuntimeError("coco_upload: table lengths disagree: %r" % (n,))
        s = L.CocoTables()
        for k, t in tensors.items():
            setattr(s, k, t.data_ptr() if t.numel() else None)
        s.n_verts, s.n_parts, s.n_anns, s.n_cand, s.B, s.max_part_keys = n["verts"] // 2, n_parts, n_anns, n["cand"], self.B, int(max_part_keys)
        self.struct = s


def coco_upload(tables, device):
    """bup20.coco_tables' dict of int32 numpy arrays -> CocoDeviceTables on `device`.  The offsets are checked here, on the host, so that no kernel reads
    or writes outside a table."""
    t = {k: tables[k] for k in _COCO_ARRAYS}
    for k, a in t.items():
        if a.dtype.name != "int32":
            raise RuntimeError("coco_upload: %s is %s, int32 expected" % (k, a.dtype))
    nv, nk, n_parts, n_anns = len(t["verts"].reshape(-1)) // 2, len(t["keys"]), len(t["part_key_count"]), len(t["ann_label"])

    def rising(name, top):
        a = t[name]
        if len(a) < 1 or a[0] != 0 or (a[1:] < a[:-1]).any() or a[-1] != top:
            raise RuntimeError("coco_upload: %s does not rise from 0 to %d" % (name, top))

    rising("part_vert_begin", nv)
    rising("part_key_begin", nk)
    rising("ann_part_begin", n_parts)
    rising("frame_ann_begin", n_anns)
    if len(t["point_begin"]) != nv + 1 or t["point_begin"][0] != 0 or (t["point_begin"][1:] <= t["point_begin"][:-1]).any():
        raise RuntimeError("coco_upload: point_begin does not rise strictly from 0 over %d edges" % nv)
    if n_parts and (t["part_key_count"] > t["part_key_begin"][1:] - t["part_key_begin"][:-1]).any():
        raise RuntimeError("coco_upload: a part_key_count beyond its slice of keys")
    if len(t["cand"]) and (int(t["cand"].min()) < 0 or int(t["cand"].max()) >= n_anns):
        raise RuntimeError("coco_upload: a candidate outside the annotations")
    return CocoDeviceTables({k: torch.from_numpy(a.reshape(-1)).to(device) for k, a in t.items()}, tables["max_part_keys"])


def coco_keys(dev, H0, W0):
    """pag_coco_keys: the sorted keys of every polygon part of the uploaded tables (bup20.polygon_keys_reference is the definition).  A part whose key bound
    exceeds COCO_MAX_PART_KEYS is refused before any launch."""
    _call("pag_coco_keys", ctypes.byref(dev.struct), int(H0), int(W0), L.stream())


def coco_labels(dev, H0, W0, mip, max_label, view_offset=0, semantics=None, instance=None):
    """pag_coco_labels after coco_keys: views [view_offset, view_offset + B) of semantics / instance int64 [V, h, w, 1] at h = H0 / 2^mip
    (bup20.coco_labels_reference is the definition); frames without labels become -1.  Once per uploaded tables (the counting pass adds into them)."""
    name = "coco_labels"
    mip, view_offset, f = int(mip), int(view_offset), 1 << int(mip)
    if not 0 <= mip <= 8 or H0 % f or W0 % f:
        raise RuntimeError("%s: mip %d with source size %d x %d" % (name, mip, H0, W0))
    V = _prepare_dst(name, "semantics", semantics, torch.int64, None, H0 // f, W0 // f, 1, view_offset, dev.B)
    V = _prepare_dst(name, "instance", instance, torch.int64, V, H0 // f, W0 // f, 1, view_offset, dev.B)
    if V is None:
        return
    p = lambda t: t.data_ptr() if t is not None else None
    _call("pag_coco_labels", ctypes.byref(dev.struct), int(H0), int(W0), mip, int(max_label), view_offset, V, p(semantics), p(instance), L.stream())


def _bup20_plane(name, what, t, dtype, shape):
    if t is None:
        return
    _check_gpu(t)
    if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise RuntimeError("%s: %s is a contiguous %s %s, got %s %s" % (name, what, dtype, shape, t.dtype, tuple(t.shape)))


def bup20_pred_stats(inst, depth_raw, max_depth, n_ids):
    """pag_bup20_pred_stats: inst int32 [B, H0, W0] with ids in [0, n_ids), depth_raw int16 bit patterns of the 16-bit depth [B, H0, W0] -> a new int32
    [B, n_ids, 2] of (pixels, pixels with 0 < depth <= max_depth) per view and id (bup20.pred_stats_reference is the definition)."""
    name = "bup20_pred_stats"
    _check_gpu(inst, depth_raw)
    if inst.dim() != 3:
        raise RuntimeError("%s: inst is [B, H0, W0], got %s" % (name, tuple(inst.shape)))
    B, H0, W0 = inst.shape
    _bup20_plane(name, "inst", inst, torch.int32, (B, H0, W0))
    _bup20_plane(name, "depth_raw", depth_raw, torch.int16, (B, H0, W0))
    counts = torch.zeros(B, int(n_ids), 2, dtype=torch.int32, device=inst.device)
    _call("pag_bup20_pred_stats", inst.data_ptr(), depth_raw.data_ptr(), B, H0, W0, float(max_depth), int(n_ids), counts.data_ptr(), L.stream())
    return counts


def bup20_prepare(img_u8, mip, bg_color="white", view_offset=0, depth_raw=None, sem=None, inst=None, sem_conf=None, inst_conf=None, counts=None, imgs=None,
                  masks=None, depths=None, semantics_pred=None, instance_pred=None, sem_conf_out=None, inst_conf_out=None):
    """pag_bup20_prepare for the frames of a chunk (bup20.prepare_frames_reference is the definition): img_u8 uint8 [B, H0, W0, 3 or 4], depth_raw int16 bit
    patterns, sem / inst int32, sem_conf / inst_conf f32 [B, H0, W0], counts from bup20_pred_stats or None -> views [view_offset, view_offset + B) of the
    requested destinations, each the whole dataset's tensor: imgs f32 [V, h, w, 3], masks bool (or uint8), depths / sem_conf_out / inst_conf_out f32,
    semantics_pred / instance_pred int64 [V, h, w, 1]."""
    name = "bup20_prepare"
    _check_gpu(img_u8, counts)
    view_offset = int(view_offset)
    mip, B, H0, W0, h, w = _prepare_sizes(name, img_u8, mip, 4)
    C0 = img_u8.shape[3]
    if C0 not in (3, 4):
        raise RuntimeError("%s: %d source channels, 3 or 4 expected" % (name, C0))
    if bg_color not in ("white", "black"):
        raise RuntimeError("%s: bg_color %r is neither 'white' nor 'black'" % (name, bg_color))
    if masks is not None and masks.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("%s: masks is bool or uint8, got %s" % (name, masks.dtype))
    for what, t, dtype in (("depth_raw", depth_raw, torch.int16), ("sem", sem, torch.int32), ("inst", inst, torch.int32), ("sem_conf", sem_conf, torch.float32),
                           ("inst_conf", inst_conf, torch.float32)):
        _bup20_plane(name, what, t, dtype, (B, H0, W0))
    n_ids = 0
    if counts is not None:
        if counts.dtype != torch.int32 or counts.dim() != 3 or counts.shape[0] != B or counts.shape[2] != 2 or not counts.is_contiguous():
            raise RuntimeError("%s: counts is a contiguous int32 [%d, n_ids, 2], got %s %s" % (name, B, counts.dtype, tuple(counts.shape)))
        n_ids = counts.shape[1]
    V = None
    for what, t, dtype, C in (("imgs", imgs, torch.float32, 3), ("masks", masks, masks.dtype if masks is not None else None, 1),
                              ("depths", depths, torch.float32, 1), ("semantics_pred", semantics_pred, torch.int64, 1),
                              ("instance_pred", instance_pred, torch.int64, 1), ("sem_conf_out", sem_conf_out, torch.float32, 1),
                              ("inst_conf_out", inst_conf_out, torch.float32, 1)):
        V = _prepare_dst(name, what, t, dtype, V, h, w, C, view_offset, B)
    if V is None:
        return
    p = lambda t: t.data_ptr() if t is not None else None
    a = L.Bup20PrepareArgs(img=img_u8.data_ptr(), depth=p(depth_raw), sem=p(sem), inst=p(inst), sem_conf=p(sem_conf), inst_conf=p(inst_conf), counts=p(counts),
                           B=B, H0=H0, W0=W0, C0=C0, mip=mip, bg=L.BG_WHITE if bg_color == "white" else L.BG_BLACK, n_ids=n_ids, view_offset=view_offset, V=V,
                           imgs=p(imgs), masks=p(masks), depths=p(depths), semantics_pred=p(semantics_pred), instance_pred=p(instance_pred),
                           sem_conf_out=p(sem_conf_out), inst_conf_out=p(inst_conf_out))
    _call("pag_bup20_prepare", ctypes.byref(a), L.stream())
