"""TriplanarGridHIP - the tri-plane feature grid (`grid_type: 'TriplanarGrid'`, configs/bup20/mean_shift_contrastive_app.yaml:137-144) on the gfx950
kernels of csrc/triplanar.hip.

wisp's TriplanarGrid is third party and not in the reference tree: parity to it is UNPINNED.  The spec of record is this project's own,
written in terms of torch.nn.functional.grid_sample.  Level l = 0 .. L-1 has R_l = 2**(base_lod + l) + 1 and three planes fmx, fmy, fmz of [1, F, R_l, R_l],
initialised as randn * feature_std + feature_bias, and for a sample c = (x, y, z)

    feat_l(c) = gs(fmx_l, (y, z)) + gs(fmy_l, (x, z)) + gs(fmz_l, (x, y))      gs = grid_sample(bilinear, padding_mode='reflection', align_corners=True)
    out[:, l*F + f] = feat_l[f] * feat_scale[l*F + f]

(the first coordinate of a pair indexes the LAST table dimension; the planes are summed in the order x, y, z).

The tables are STORED as one flat fp32 nn.Parameter `tables` - per level [3][R][R][F], channel-last, level after level - so that the tracer's graph key,
optim.Adam and the gradient exchange see one tensor, as for every other grid here; state_dict() / load_state_dict() translate to and from the
`features.{i}.fmx|fmy|fmz` [1, F, R, R] names.

Where it runs: GPU fp32 tensors with F in {2, 4, 8} and L <= 8 take the kernels (one launch forward, one per gradient); everything else, CPU tensors
included, takes the tensor-op form below, which IS the definition.  `use_kernel=False` forces the tensor-op form, `use_kernel=True` refuses to fall back.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .grids import _GridBase

PLANES = ("fmx", "fmy", "fmz")
PAIRS = ((1, 2), (0, 2), (0, 1))          # fmx reads (y, z), fmy (x, z), fmz (x, y): the first indexes the columns (W), the second the rows (H)
KERNEL_FEATS = (2, 4, 8)
KERNEL_MAX_LEVELS = 8


class TriplanarSpec:
    """Static description of the level pyramid: resolutions and the float offset of every level in the flat buffer.  Plain Python numbers
    (picklable); the ctypes array the C ABI takes is rebuilt on unpickling."""

    def __init__(self, resolutions, n_feat):
        self.res = [int(r) for r in resolutions]
        self.L, self.F = len(self.res), int(n_feat)
        self._bind()

    def _bind(self):
        self.offsets, off = [], 0
        for r in self.res:
            self.offsets.append(off)
            off += 3 * r * r * self.F
        self.numel = off
        self.res_c = (ctypes.c_int * self.L)(*self.res)

    def __getstate__(self):
        return dict(res=self.res, F=self.F)

    def __setstate__(self, state):
        self.res, self.F = state["res"], state["F"]
        self.L = len(self.res)
        self._bind()


# ------------------------------------------------------------------------------------------------------------------------- layout helpers
def plane_to_stored(t):
    """reference [1,F,R,R] -> stored [R,R,F]"""
    return t[0].permute(1, 2, 0).contiguous()


def plane_to_reference(t):
    """stored [R,R,F] -> reference [1,F,R,R] (a view)"""
    return t.permute(2, 0, 1)[None]


def reference_planes(tables, spec):
    """The flat buffer as L tuples (fmx, fmy, fmz) of [1,F,R,R] views (gradients flow back into `tables`)."""
    out = []
    for r, off in zip(spec.res, spec.offsets):
        lvl = tables[off:off + 3 * r * r * spec.F].view(3, r, r, spec.F)
        out.append(tuple(plane_to_reference(lvl[p]) for p in range(3)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------- tensor ops
def triplanar_tensor_forward(planes, xyz, feat_scale=None):
    """The definition: planes = L tuples (fmx, fmy, fmz) of [1,F,R,R], xyz [M,3] in the planes' dtype -> [M, L*F] (column l*F + f).
    Differentiable with respect to the planes and xyz."""
    M = xyz.shape[0]
    if M == 0:                                  # grid_sample takes no empty grid: an empty result that still hangs on the planes (zero gradients)
        width = sum(level[0].shape[1] for level in planes)
        return xyz.new_zeros(0, width) + (sum(t.sum() for level in planes for t in level) + xyz.sum()) * 0
    grids = [xyz[:, list(p)].reshape(1, M, 1, 2) for p in PAIRS]
    feats = []
    for level in planes:
        s = [F.grid_sample(t, g, mode="bilinear", padding_mode="reflection", align_corners=True).reshape(t.shape[1], M).t() for t, g in zip(level, grids)]
        feats.append(s[0] + s[1] + s[2])
    out = torch.cat(feats, dim=-1)
    if feat_scale is not None:
        out = out * torch.as_tensor(feat_scale, dtype=out.dtype, device=out.device)
    return out


# -------------------------------------------------------------------------------------------------------------------------------- kernels
def _check(xyz, tables, spec):
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != torch.float32 or not xyz.is_contiguous():
        raise ValueError("tri-plane grid: xyz must be a contiguous f32 [M,3] tensor, got %s %s" % (tuple(xyz.shape), xyz.dtype))
    if tables.dim() != 1 or tables.numel() != spec.numel or tables.dtype != torch.float32 or not tables.is_contiguous():
        raise ValueError("tri-plane grid: tables must be a contiguous f32 [%d] tensor, got %s %s" % (spec.numel, tuple(tables.shape), tables.dtype))


def _grad_arg(g):
    if g.dtype not in (torch.float32, torch.bfloat16):
        g = g.float()
    if g.stride(0) < 1 or g.stride(1) < 1:          # an expanded gradient (sum().backward()): the kernels take positive strides
        g = g.contiguous()
    return g


def triplanar_forward(tables, spec, xyz, feat_scale=None, out_dtype=torch.float32):
    """One launch: xyz f32 [M,3] -> [M, L*F] in fp32 or bf16 (the fp32 result rounded once)."""
    _check(xyz, tables, spec)
    M = xyz.shape[0]
    out = torch.empty(M, spec.L * spec.F, device=xyz.device, dtype=out_dtype)
    if M:
        ops._call("pag_triplanar_fwd", L.ptr(xyz), M, L.ptr(tables), spec.L, spec.F, spec.res_c, L.host_floats(feat_scale), L.ptr(out), L.dtype_code(out),
                  out.stride(0), out.stride(1), L.stream())
    return out


def triplanar_backward_tables(spec, xyz, g, feat_scale=None):
    """-> the flat fp32 table gradient (zero-filled here, the kernel adds into it)."""
    M = xyz.shape[0]
    gt = torch.zeros(spec.numel, device=xyz.device, dtype=torch.float32)
    if M:
        g = _grad_arg(g)
        ops._call("pag_triplanar_bwd_tables", L.ptr(xyz), M, g.data_ptr(), L.dtype_code(g), g.stride(0), g.stride(1), spec.L, spec.F, spec.res_c,
                  L.host_floats(feat_scale), L.ptr(gt), L.stream())
    return gt


def triplanar_backward_xyz(tables, spec, xyz, g, feat_scale=None):
    """-> d loss / d xyz f32 [M,3]."""
    M = xyz.shape[0]
    d_xyz = torch.empty(M, 3, device=xyz.device, dtype=torch.float32)
    if M:
        g = _grad_arg(g)
        ops._call("pag_triplanar_bwd_xyz", L.ptr(xyz), M, L.ptr(tables), g.data_ptr(), L.dtype_code(g), g.stride(0), g.stride(1), spec.L, spec.F, spec.res_c,
                  L.host_floats(feat_scale), L.ptr(d_xyz), L.stream())
    return d_xyz


class _Triplanar(torch.autograd.Function):
    """The grid as one node from (xyz, tables) to the features.  The backward recomputes the taps from xyz; the position gradient (pose optimisation)
    leaves as a plain [M,3] tensor."""

    @staticmethod
    def forward(ctx, xyz, tables, spec, feat_scale, out_dtype):
        xyz = xyz.detach().contiguous().float()
        tc = tables.detach()
        out = triplanar_forward(tc, spec, xyz, feat_scale, out_dtype)
        ctx.spec, ctx.feat_scale = spec, feat_scale
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(xyz, tc)           # d / d xyz needs the table rows again
        else:
            ctx.save_for_backward(xyz)
        return out

    @staticmethod
    def backward(ctx, g):
        xyz = ctx.saved_tensors[0]
        gt = d_xyz = None
        if ctx.needs_input_grad[1]:
            gt = triplanar_backward_tables(ctx.spec, xyz, g, ctx.feat_scale)
        if ctx.needs_input_grad[0]:
            d_xyz = triplanar_backward_xyz(ctx.saved_tensors[1], ctx.spec, xyz, g, ctx.feat_scale)
        return d_xyz, gt, None, None, None


# ----------------------------------------------------------------------------------------------------------------------------------- grid
class TriplanarGridHIP(_GridBase):
    """wisp TriplanarGrid's constructor keywords (the rest of the config namespace is swallowed) and plugin API on the tri-plane kernels.
    `use_kernel`: None = the kernels where they apply, False = tensor ops, True = the kernels or an error."""

    offers_xcd8 = False        # strided features only: the nef takes its ungrouped decoder path
    half_coords = False        # wisp's TriplanarGrid does no fp16 cast of the coordinates

    def __init__(self, feature_dim, base_lod=2, num_lods=1, interpolation_type="linear", multiscale_type="cat", feature_std=0.0, feature_bias=0.0,
                 blas_level=7, use_kernel=None, **kwargs):
        super().__init__(feature_dim, base_lod=base_lod, num_lods=num_lods, interpolation_type=interpolation_type, multiscale_type=multiscale_type,
                         feature_std=feature_std, feature_bias=feature_bias, blas_level=blas_level)
        if interpolation_type != "linear":
            raise NotImplementedError("TriplanarGrid: interpolation_type '%s' (linear only)" % interpolation_type)
        self.use_kernel = use_kernel
        self.active_lods = [int(base_lod) + i for i in range(self.num_lods)]
        self.max_lod = self.active_lods[-1]
        self.resolutions = [2 ** lod + 1 for lod in self.active_lods]
        self._spec = TriplanarSpec(self.resolutions, self.feature_dim)
        flat = []
        for r in self.resolutions:          # the draws are made in the reference's shapes and order (fmx, fmy, fmz per level)
            for _ in PLANES:
                flat.append(plane_to_stored(torch.randn(1, self.feature_dim, r, r) * feature_std + feature_bias).reshape(-1))
        self.tables = nn.Parameter(torch.cat(flat))
        self._register_state_dict_hook(self._to_reference_layout)
        self._register_load_state_dict_pre_hook(self._from_reference_layout)

    # ------------------------------------------------------------------------------------------------ reference layout
    def planes(self, tables=None):
        """L tuples (fmx, fmy, fmz) of [1,F,R,R] views of the flat buffer."""
        return reference_planes(self.tables if tables is None else tables, self._spec)

    def set_planes(self, planes):
        """Copy L tuples (fmx, fmy, fmz) of [1,F,R,R] into the flat buffer."""
        with torch.no_grad():
            for mine, theirs in zip(self.planes(), planes):
                for m, t in zip(mine, theirs):
                    m.copy_(t.to(device=m.device, dtype=m.dtype))

    @staticmethod
    def _to_reference_layout(module, state_dict, prefix, local_metadata):
        flat = state_dict.pop(prefix + "tables", None)
        if flat is not None:
            for i, level in enumerate(reference_planes(flat, module._spec)):
                for name, t in zip(PLANES, level):
                    state_dict["%sfeatures.%d.%s" % (prefix, i, name)] = t.contiguous()
        return state_dict

    def _from_reference_layout(self, state_dict, prefix, *args):
        keys = [["%sfeatures.%d.%s" % (prefix, i, name) for name in PLANES] for i in range(self.num_lods)]
        if prefix + "tables" in state_dict or not all(k in state_dict for level in keys for k in level):
            return                             # the flat form, or an incomplete set: load_state_dict reports what is missing
        flat = []
        for level, r in zip(keys, self.resolutions):
            for k in level:
                t = state_dict.pop(k)
                if tuple(t.shape) != (1, self.feature_dim, r, r):
                    raise RuntimeError("TriplanarGrid: %s has shape %s, expected %s" % (k, tuple(t.shape), (1, self.feature_dim, r, r)))
                flat.append(plane_to_stored(t).reshape(-1))
        state_dict[prefix + "tables"] = torch.cat(flat)

    # ------------------------------------------------------------------------------------------------------- evaluation
    def kernel_supported(self, xyz):
        t = self.tables
        return bool(xyz.is_cuda and xyz.dtype == torch.float32 and t.is_cuda and t.device == xyz.device and t.dtype == torch.float32 and t.is_contiguous()
                    and self.feature_dim in KERNEL_FEATS and self.num_lods <= KERNEL_MAX_LEVELS)

    def tensor_forward(self, xyz, feat_scale=None):
        return triplanar_tensor_forward(self.planes(), xyz.to(self.tables.dtype), feat_scale)

    def interpolate_scaled(self, coords, feat_scale=None, out_dtype=torch.float32, layout=None, addend=None):
        """[M, L*F] features with the nef's lod_weights folded in, in out_dtype (strided; this grid offers no XCD-grouped layout and no addend)."""
        if layout is not None or addend is not None:
            raise NotImplementedError("TriplanarGrid: strided features only (layout=%r, addend given: %s)" % (layout, addend is not None))
        xyz = self._coords(coords)
        use_kernel = self.use_kernel
        if use_kernel is None:
            use_kernel = self.kernel_supported(xyz)
        elif use_kernel and not self.kernel_supported(xyz):
            raise RuntimeError("TriplanarGrid: use_kernel=True but the kernels do not apply (GPU fp32 tensors, F in %s, at most %d levels)"
                               % (KERNEL_FEATS, KERNEL_MAX_LEVELS))
        if not use_kernel:
            return self.tensor_forward(xyz, feat_scale).to(out_dtype)
        if torch.is_grad_enabled() and (self.tables.requires_grad or xyz.requires_grad):
            return _Triplanar.apply(xyz, self.tables, self._spec, feat_scale, out_dtype)
        return triplanar_forward(self.tables.detach(), self._spec, xyz.detach().contiguous().float(), feat_scale, out_dtype)

    def interpolate(self, coords, lod_idx=None, pidx=None):
        """coords [B,S,3] -> [B, S, L*F] ('cat') or [B, S, F] ('sum'); lod_idx is ignored, as in the other grids here."""
        batch, num_samples, _ = coords.shape
        width = self.num_lods * self.feature_dim if self.multiscale_type == "cat" else self.feature_dim
        if coords.numel() == 0:
            return torch.empty(batch, num_samples, width, device=coords.device)
        feats = self.interpolate_scaled(coords).reshape(batch, num_samples, -1)
        return self._finish(feats, batch, num_samples)
