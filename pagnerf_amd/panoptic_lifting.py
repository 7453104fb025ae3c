"""PanopticLiftingNeF - the Panoptic Lifting comparison baseline (pc_nerf/panoptic_lifting.py, grids/tensorf.py,
configs/bup20/panoptic_lifting_app.yaml) on the gfx950 kernels.

    TensoRF vector-matrix grid -> sigma_feature (density = relu) and a 27-wide appearance feature -> MLPRenderFeature (150 -> 128 -> 128 -> 3) = rgb
    raw coords -> BasicDecoder -> semantics;  raw coords -> BasicDecoder -> inst_embedding

Where it runs: the grid - 12 bilinear gathers, the plane x line products, the density sum and the 144 -> 27 basis projection - is one launch
(csrc/vm.hip) behind one autograd.Function for GPU fp32 tensors of a supported shape (16 / 48 components, 27 appearance channels); everything else,
CPU tensors included, takes the tensor-op path below in fp32, which is the reference's arithmetic.  The three decoders are plain nn.Linear stacks
in tensor ops: precision="fp32" (the DEFAULT) is the reference's arithmetic, precision="bf16" runs them under bf16 autocast on GPU tensors (the grid
stays fp32).  fp32 is the default because the two panoptic heads read the RAW coordinates: bf16 rounds a position to 8 significant bits in front of
their first layer.

The tables are STORED channel-last (plane [R,R,C], line [R,C]; contiguous fp32, so that optim.Adam takes its kernel on them and a bilinear tap is
one contiguous row); state_dict() / load_state_dict() translate to and from the reference's [1,C,R,R] / [1,C,R,1], names unchanged.

The grid's coordinates are detached, as in the reference: the Function returns no gradient for coords.  Gradients with respect to coords through
the semantic / instance heads and ray_d through the colour head come from autograd.  The nef does not set `accepts_ray_index`: the tracer hands it
a per-sample ray_d and training traces take the eager path.

The reference's grid reshapes with `.view(-1, batch)`, which is only meaningful for num_samples == 1 (what every tracer hands it); it is not well
defined for S > 1.  Here coords [B,S,3] with S > 1 are flattened to B * S samples and ray_d is repeated per sample.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .grids import OccupancyBLAS
from .nef import _param_names
from .semantic_nef import SkipDecoder, _ACTS, sample_unif_sphere

APP_DIM = 27
MAT_MODE = ((0, 1), (0, 2), (1, 2))      # plane i reads these two coordinates: the first indexes the columns (W), the second the rows (H)
VEC_MODE = (2, 1, 0)                     # line i runs along this coordinate


# ------------------------------------------------------------------------------------------------------------------------- layout helpers
def plane_to_stored(t):
    """reference [1,C,R,R] -> stored [R,R,C]"""
    return t[0].permute(1, 2, 0).contiguous()


def plane_to_reference(t):
    """stored [R,R,C] -> reference [1,C,R,R] (a view)"""
    return t.permute(2, 0, 1)[None]


def line_to_stored(t):
    """reference [1,C,R,1] -> stored [R,C]"""
    return t[0, :, :, 0].t().contiguous()


def line_to_reference(t):
    """stored [R,C] -> reference [1,C,R,1] (a view)"""
    return t.t()[None, :, :, None]


# ---------------------------------------------------------------------------------------------------------------------------- tensor ops
def vm_tensor_forward(density_plane, density_line, app_plane, app_line, basis_weight, xyz, need_sigma=True, need_app=True):
    """The vector-matrix grid in tensor ops on reference-layout tables ([1,C,R,R] planes, [1,C,R,1] lines): bilinear grid_sample with
    align_corners and zero padding, sigma = sum over planes and components of plane * line, app = basis . cat(plane * line).
    xyz [M,3] (detached here) -> (sigma [M] | None, app [M,27] | None)."""
    x = xyz.detach()
    M = x.shape[0]
    zeros = torch.zeros_like(x[:, 0])
    cp = [x[:, list(MAT_MODE[i])].reshape(1, M, 1, 2) for i in range(3)]
    cl = [torch.stack([zeros, x[:, VEC_MODE[i]]], dim=-1).reshape(1, M, 1, 2) for i in range(3)]

    def sample(table, grid):
        return F.grid_sample(table, grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(table.shape[1], M)

    sigma = app = None
    if need_sigma:
        sigma = torch.zeros(M, device=x.device, dtype=density_plane[0].dtype)
        for i in range(3):
            sigma = sigma + (sample(density_plane[i], cp[i]) * sample(density_line[i], cl[i])).sum(dim=0)
    if need_app:
        prod = torch.cat([sample(app_plane[i], cp[i]) * sample(app_line[i], cl[i]) for i in range(3)], dim=0)
        app = F.linear(prod.t(), basis_weight)
    return sigma, app


# -------------------------------------------------------------------------------------------------------------------------------- kernels
def _vm_args(tables, basis, res):
    a = L.VmArgs()
    dp, dl, ap, al = tables
    for i in range(3):
        a.density_plane[i], a.density_line[i], a.app_plane[i], a.app_line[i] = L.ptr(dp[i]), L.ptr(dl[i]), L.ptr(ap[i]), L.ptr(al[i])
    a.basis = L.ptr(basis)
    a.density_n_comp, a.app_n_comp, a.app_dim, a.res = dp[0].shape[-1], ap[0].shape[-1], basis.shape[0], res
    return a


def _check_tables(tables, basis, res):
    dp, dl, ap, al = tables
    for group, shape_of in ((dp, lambda C: (res, res, C)), (dl, lambda C: (res, C)), (ap, lambda C: (res, res, C)), (al, lambda C: (res, C))):
        C = group[0].shape[-1]
        for t in group:
            if tuple(t.shape) != shape_of(C) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("vm grid: table must be a contiguous f32 %s tensor, got %s %s" % (shape_of(C), tuple(t.shape), t.dtype))
    if tuple(basis.shape) != (APP_DIM, 3 * ap[0].shape[-1]) or basis.dtype != torch.float32 or not basis.is_contiguous():
        raise ValueError("vm grid: basis must be a contiguous f32 [27,%d] tensor, got %s" % (3 * ap[0].shape[-1], tuple(basis.shape)))


def _check_xyz(xyz):
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != torch.float32 or not xyz.is_contiguous():
        raise ValueError("vm grid: xyz must be a contiguous f32 [M,3] tensor, got %s %s" % (tuple(xyz.shape), xyz.dtype))


def vm_forward(tables, basis, res, xyz, need_sigma=True, need_app=True):
    """One launch: stored-layout tables (four lists of three), basis [27,144], xyz f32 [M,3] -> (sigma [M] | None, app [M,27] | None)."""
    _check_tables(tables, basis, res)
    _check_xyz(xyz)
    if not (need_sigma or need_app):
        raise ValueError("vm grid: neither sigma nor app requested")
    M, dev = xyz.shape[0], xyz.device
    sigma = torch.empty(M, device=dev) if need_sigma else None
    app = torch.empty(M, APP_DIM, device=dev) if need_app else None
    if M:
        a = _vm_args(tables, basis, res)
        a.xyz, a.sigma, a.app = L.ptr(xyz), L.ptr(sigma), L.ptr(app)
        with torch.cuda.device(dev):
            L.check(L.load().pag_vm_fwd(ctypes.byref(a), M, L.stream()), "pag_vm_fwd")
    return sigma, app


def vm_backward(tables, basis, res, xyz, g_sigma, g_app):
    """-> (four lists of three table gradients, basis gradient), in the stored layouts; a set without an upstream gradient gets None."""
    _check_tables(tables, basis, res)
    _check_xyz(xyz)
    M, dev = xyz.shape[0], xyz.device
    for g, shape in ((g_sigma, (M,)), (g_app, (M, APP_DIM))):
        if g is not None and (tuple(g.shape) != shape or g.dtype != torch.float32 or not g.is_contiguous()):
            raise ValueError("vm grid: upstream gradient must be a contiguous f32 %s tensor, got %s %s" % (shape, tuple(g.shape), g.dtype))
    dp, dl, ap, al = tables
    zeros = lambda ts, on: [torch.zeros_like(t) if on else None for t in ts]
    grads = (zeros(dp, g_sigma is not None), zeros(dl, g_sigma is not None), zeros(ap, g_app is not None), zeros(al, g_app is not None))
    g_basis = torch.zeros_like(basis) if g_app is not None else None
    if M and (g_sigma is not None or g_app is not None):
        a = _vm_args(tables, basis, res)
        a.xyz, a.g_sigma, a.g_app = L.ptr(xyz), L.ptr(g_sigma), L.ptr(g_app)
        for i in range(3):
            a.g_density_plane[i], a.g_density_line[i] = L.ptr(grads[0][i]), L.ptr(grads[1][i])
            a.g_app_plane[i], a.g_app_line[i] = L.ptr(grads[2][i]), L.ptr(grads[3][i])
        a.g_basis = L.ptr(g_basis)
        if g_app is not None:                 # the basis gradient's per-workgroup partial sums
            n = L.load().pag_vm_bwd_workspace_bytes(M)
            if n < 0:
                L.check(-1, "pag_vm_bwd_workspace_bytes")
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            a.workspace, a.workspace_bytes = L.ptr(ws), n
        with torch.cuda.device(dev):
            L.check(L.load().pag_vm_bwd(ctypes.byref(a), M, L.stream()), "pag_vm_bwd")
    return grads, g_basis


class _VMGrid(torch.autograd.Function):
    """The grid as one node.  Inputs after the flags: 3 density planes, 3 density lines, 3 appearance planes, 3 appearance lines (stored layout), the
    basis weight.  The backward recomputes the taps from xyz; there is no gradient for xyz (the reference detaches the coordinates)."""

    @staticmethod
    def forward(ctx, xyz, res, need_sigma, need_app, *params):
        ps = [p.detach() for p in params]
        tables, basis = (ps[0:3], ps[3:6], ps[6:9], ps[9:12]), ps[12]
        sigma, app = vm_forward(tables, basis, res, xyz, need_sigma, need_app)
        ctx.save_for_backward(xyz, *ps)
        ctx.res = res
        ctx.set_materialize_grads(False)
        return sigma, app

    @staticmethod
    def backward(ctx, g_sigma, g_app):
        xyz, ps = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        if g_sigma is None and g_app is None:
            return (None,) * 17
        tables, basis = (ps[0:3], ps[3:6], ps[6:9], ps[9:12]), ps[12]
        prep = lambda g: None if g is None else g.detach().float().contiguous()
        grads, g_basis = vm_backward(tables, basis, ctx.res, xyz, prep(g_sigma), prep(g_app))
        return (None, None, None, None, *grads[0], *grads[1], *grads[2], *grads[3], g_basis)


# ----------------------------------------------------------------------------------------------------------------------------------- grid
class VMSplitFeatureVolume(nn.Module):
    """grids/tensorf.py::VMSplitFeatureVolume: three planes and three lines per set, 0.1 * randn, and basis_mat = Linear(3 * app_n_comp, 27).
    Parameter names are the reference's; the tables are stored channel-last (module docstring) and translated in the state-dict hooks."""

    def __init__(self, density_n_comp, app_n_comp, res):
        super().__init__()
        self.density_n_comp, self.app_n_comp, self.res, self.app_dim = int(density_n_comp), int(app_n_comp), int(res), APP_DIM
        self.density_plane, self.density_line = self._init_set(self.density_n_comp, self.res, 0.1)
        self.app_plane, self.app_line = self._init_set(self.app_n_comp, self.res, 0.1)
        self.basis_mat = nn.Linear(3 * self.app_n_comp, self.app_dim, bias=False)
        self._register_state_dict_hook(self._to_reference_layout)
        self._register_load_state_dict_pre_hook(self._from_reference_layout)

    @staticmethod
    def _init_set(C, R, scale):
        planes, lines = [], []
        for _ in range(3):           # the draws are made in the reference's shapes and order, so that a seed gives the reference's tables
            planes.append(nn.Parameter(plane_to_stored(scale * torch.randn(1, C, R, R))))
            lines.append(nn.Parameter(line_to_stored(scale * torch.randn(1, C, R, 1))))
        return nn.ParameterList(planes), nn.ParameterList(lines)

    _SETS = (("density_plane", plane_to_reference, plane_to_stored), ("density_line", line_to_reference, line_to_stored),
             ("app_plane", plane_to_reference, plane_to_stored), ("app_line", line_to_reference, line_to_stored))

    @staticmethod
    def _to_reference_layout(module, state_dict, prefix, local_metadata):
        for name, to_ref, _ in VMSplitFeatureVolume._SETS:
            for i in range(3):
                k = "%s%s.%d" % (prefix, name, i)
                if k in state_dict:
                    state_dict[k] = to_ref(state_dict[k]).contiguous()
        return state_dict

    def _from_reference_layout(self, state_dict, prefix, *args):
        for name, _, to_stored in self._SETS:
            for i in range(3):
                k = "%s%s.%d" % (prefix, name, i)
                if k in state_dict and state_dict[k].dim() == 4:
                    state_dict[k] = to_stored(state_dict[k])

    def tables(self):
        return list(self.density_plane), list(self.density_line), list(self.app_plane), list(self.app_line)

    def kernel_supported(self, xyz):
        ts = [t for group in self.tables() for t in group] + [self.basis_mat.weight]
        if not (xyz.is_cuda and xyz.dtype == torch.float32 and all(t.is_cuda and t.dtype == torch.float32 and t.device == xyz.device and t.is_contiguous() for t in ts)):
            return False
        return bool(L.load().pag_vm_supported(self.density_n_comp, self.app_n_comp, self.app_dim, self.res))

    def tensor_forward(self, xyz, need_sigma=True, need_app=True):
        dp, dl, ap, al = self.tables()
        return vm_tensor_forward([plane_to_reference(t) for t in dp], [line_to_reference(t) for t in dl], [plane_to_reference(t) for t in ap],
                                 [line_to_reference(t) for t in al], self.basis_mat.weight, xyz, need_sigma, need_app)

    def forward(self, xyz, need_sigma=True, need_app=True, use_kernel=None):
        """xyz [M,3] -> (sigma_feature [M] | None, app [M,27] | None).  use_kernel: None = the kernels where they apply, False = tensor ops."""
        if use_kernel is None:
            use_kernel = self.kernel_supported(xyz)
        if not use_kernel:
            return self.tensor_forward(xyz.float(), need_sigma, need_app)
        dp, dl, ap, al = self.tables()
        x = xyz.detach().contiguous()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _VMGrid.apply(x, self.res, need_sigma, need_app, *dp, *dl, *ap, *al, self.basis_mat.weight)
        return vm_forward((dp, dl, ap, al), self.basis_mat.weight, self.res, x, need_sigma, need_app)

    @torch.no_grad()
    def upsample_volume_grid(self, res_target):
        """Bilinear (align_corners) resampling of every table to res_target; the parameters are replaced by new ones, as in the reference, so
        the optimiser has to be created again."""
        r = int(res_target)
        for planes, lines in ((self.app_plane, self.app_line), (self.density_plane, self.density_line)):
            for i in range(3):
                p = F.interpolate(plane_to_reference(planes[i].data), size=(r, r), mode="bilinear", align_corners=True)
                l = F.interpolate(line_to_reference(lines[i].data), size=(r, 1), mode="bilinear", align_corners=True)
                planes[i] = nn.Parameter(plane_to_stored(p))
                lines[i] = nn.Parameter(line_to_stored(l))
        self.res = r


class TensoRF(OccupancyBLAS):
    """grids/tensorf.py::TensoRF: one vector-matrix feature volume that grows over training, on the dense occupancy structure (used as an AABB
    tracer).  `num_resolutions` keeps the reference's name: the trainer keys its upsampling schedule on it."""

    def __init__(self, density_n_comp=16, color_n_comp=48, base_resolution=128, max_resolution=192, num_resolution=5, blas_level=7, **kwargs):
        super().__init__(blas_level)
        self.kwargs = kwargs
        self.density_n_comp, self.color_n_comp = int(density_n_comp), int(color_n_comp)
        self.base_resolution, self.max_resolution, self.num_resolutions = int(base_resolution), int(max_resolution), int(num_resolution)
        self.current_resolution = self.base_resolution
        d_res = (self.max_resolution - self.base_resolution) // (self.num_resolutions - 1)
        self.resolutions = list(range(self.base_resolution, self.max_resolution + d_res, d_res))
        self.num_lods, self.base_lod, self.active_lods, self.max_lod = 1, 0, [0], 0
        self.features = VMSplitFeatureVolume(self.density_n_comp, self.color_n_comp, self.current_resolution)
        self.num_feat = self.features.density_n_comp + self.features.app_dim * self.features.app_n_comp

    def freeze(self):
        self.features.requires_grad_(False)

    def interpolate(self, coords, lod_idx, pidx=None, need_sigma=True, need_app=True, use_kernel=None):
        """coords [B,S,3] -> (sigma_feature [B,S,1], app [B,S,27]); an output that is not needed is None."""
        batch, num_samples = coords.shape[:2]
        sigma, app = self.features(coords.reshape(-1, 3), need_sigma, need_app, use_kernel)
        return (sigma.reshape(batch, num_samples, -1) if sigma is not None else None,
                app.reshape(batch, num_samples, -1) if app is not None else None)

    def step_upsample_vm_grid(self):
        i = self.resolutions.index(self.current_resolution)
        if i + 1 < len(self.resolutions):
            self.upsample_vm_grid(self.resolutions[i + 1])

    def upsample_vm_grid(self, target_res):
        self.features.upsample_volume_grid(target_res)
        self.current_resolution = int(target_res)


# ------------------------------------------------------------------------------------------------------------------------------- decoders
class MLPRenderFeature(nn.Module):
    """The colour head: cat[features, viewdirs, PE(features), PE(viewdirs)] -> Linear -> ReLU -> Linear -> ReLU -> Linear -> sigmoid, the last
    bias zero.  PE(p) = cat[sin(q), cos(q)] with q = (p[..., None] * [1, 2, .. 2^(freqs-1)]) flattened coordinate-major."""

    def __init__(self, in_channels, out_channels=3, pe_view=2, pe_feat=2, dim_mlp_color=128):
        super().__init__()
        self.pe_view, self.pe_feat, self.in_channels, self.output_channels = pe_view, pe_feat, in_channels, out_channels
        self.view_independent = pe_view == 0 and pe_feat == 0
        self.in_feat_mlp = 2 * pe_view * 3 + 2 * pe_feat * in_channels + in_channels + (0 if self.view_independent else 3)
        self.mlp = nn.Sequential(nn.Linear(self.in_feat_mlp, dim_mlp_color), nn.ReLU(), nn.Linear(dim_mlp_color, dim_mlp_color), nn.ReLU(),
                                 nn.Linear(dim_mlp_color, out_channels))
        nn.init.constant_(self.mlp[-1].bias, 0)

    @staticmethod
    def positional_encoding(p, freqs):
        bands = 2.0 ** torch.arange(freqs, device=p.device, dtype=torch.float32)
        q = (p[..., None] * bands).reshape(p.shape[:-1] + (freqs * p.shape[-1],))
        return torch.cat([torch.sin(q), torch.cos(q)], dim=-1)

    def forward(self, viewdirs, features):
        f = features.reshape(-1, features.shape[-1])
        parts = [f]
        if not self.view_independent:
            parts.append(viewdirs)
        if self.pe_feat > 0:
            parts.append(self.positional_encoding(f, self.pe_feat))
        if self.pe_view > 0:
            parts.append(self.positional_encoding(viewdirs, self.pe_view))
        return torch.sigmoid(self.mlp(torch.cat(parts, dim=-1)))


class PanopticLiftingNeF(nn.Module):
    """pc_nerf/panoptic_lifting.py::PanopticLiftingNeF: same constructor keywords (the rest is swallowed), parameter names, channels and shapes.
    With coords [M,1,3]: density [M,1,1], rgb [M,3], semantics [M,1,C], inst_embedding [M,1,I].  The grid keywords (density_n_comp .. blas_level)
    are this class' additions: the reference always builds TensoRF() with its defaults, which they default to."""

    def __init__(self, num_classes=-1, num_instances=-1, sem_activation_type=None, sem_num_layers=None, sem_hidden_dim=None, sem_normalize=False,
                 sem_softmax=False, sem_sigmoid=False, sem_detach=True, inst_num_layers=None, inst_hidden_dim=None, inst_normalize=False,
                 inst_softmax=False, inst_sigmoid=False, inst_detach=True, panoptic_features_type=None, activation_type="relu", layer_type="none",
                 num_layers=1, hidden_dim=128, density_n_comp=16, color_n_comp=48, base_resolution=128, max_resolution=192, num_resolution=5,
                 blas_level=7, precision="fp32", **kwargs):
        super().__init__()
        assert num_classes >= 1, "PanopticLiftingNeF needs num_classes"
        assert num_instances > 2, "'num_instances' needs to be > 2, but %d was given" % num_instances
        self.num_classes, self.num_instances = num_classes, num_instances
        self.activation_type, self.layer_type, self.num_layers, self.hidden_dim = activation_type, layer_type, num_layers, hidden_dim
        self.sem_activation_type = sem_activation_type if sem_activation_type else activation_type
        if self.sem_activation_type not in _ACTS:
            raise NotImplementedError("sem_activation_type '%s'" % self.sem_activation_type)
        self.sem_num_layers = sem_num_layers if sem_num_layers else num_layers
        self.sem_hidden_dim = sem_hidden_dim if sem_hidden_dim else hidden_dim
        self.inst_num_layers = inst_num_layers if inst_num_layers else num_layers
        self.inst_hidden_dim = inst_hidden_dim if inst_hidden_dim else hidden_dim
        self.sem_normalize, self.sem_softmax, self.sem_sigmoid, self.sem_detach = sem_normalize, sem_softmax, sem_sigmoid, sem_detach
        self.inst_normalize, self.inst_softmax, self.inst_sigmoid, self.inst_detach = inst_normalize, inst_softmax, inst_sigmoid, inst_detach
        self.panoptic_features_type = panoptic_features_type
        self.kwargs = kwargs
        self.grid = TensoRF(density_n_comp=density_n_comp, color_n_comp=color_n_comp, base_resolution=base_resolution,
                            max_resolution=max_resolution, num_resolution=num_resolution, blas_level=blas_level)
        self.input_dim_inst = self.input_dim_sem = 3
        self.decoder_color = MLPRenderFeature(in_channels=APP_DIM)
        if self.sem_num_layers < 2 or self.inst_num_layers < 2:
            raise NotImplementedError("sem_num_layers / inst_num_layers below 2 (a head without a hidden layer)")
        self.decoder_semantics = SkipDecoder(self.input_dim_sem, num_classes, self.sem_num_layers - 1, self.sem_hidden_dim)
        self.decoder_inst = SkipDecoder(self.input_dim_inst, num_instances, self.inst_num_layers - 1, self.inst_hidden_dim)
        self.set_precision(precision)

    def set_precision(self, precision):
        """'fp32' (default): the reference's arithmetic; 'bf16': the three decoders under bf16 autocast on GPU tensors.  The grid is fp32 in both."""
        assert precision in ("bf16", "fp32")
        self.precision = precision

    @property
    def device(self):
        return self.grid.features.basis_mat.weight.device

    def get_nef_type(self):
        return "panoptic_nef"

    def get_supported_channels(self):
        return {"density", "rgb", "semantics", "inst_embedding"}

    def forward(self, channels=None, **kwargs):
        """wisp BaseNeuralField.forward semantics: str -> tensor, list -> list, set -> dict."""
        kwargs["compute_channels"] = channels
        req = {channels} if isinstance(channels, str) else set(channels)
        unsupported = req - self.get_supported_channels()
        if unsupported:
            raise Exception("Channels %s are not supported in %s" % (unsupported, type(self).__name__))
        fn = self.rgb_semantics
        params = _param_names(fn)
        out = fn(**{k: v for k, v in kwargs.items() if k in params})
        if isinstance(channels, str):
            return out[channels]
        if isinstance(channels, list):
            return [out[c] for c in channels]
        return {c: out[c] for c in req}

    def _decode(self, fn, *inputs):
        if self.precision == "bf16" and inputs[0].is_cuda:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return fn(*inputs).float()
        return fn(*[t.float() for t in inputs])

    @staticmethod
    def _post(x, sigmoid, normalize, softmax):
        x = torch.sigmoid(x) if sigmoid else x
        x = F.normalize(x, dim=-1) if normalize else x
        return F.softmax(x, dim=-1) if softmax else x

    def rgb_semantics(self, coords, ray_d=None, compute_channels=None, pidx=None, lod_idx=None, use_kernel=None):
        out = {}
        if not compute_channels:
            return out
        channels = {compute_channels} if isinstance(compute_channels, str) else set(compute_channels)
        batch, num_samples, _ = coords.shape
        if "density" in channels or "rgb" in channels:
            sigma, app = self.grid.interpolate(coords, 0, need_sigma="density" in channels, need_app="rgb" in channels, use_kernel=use_kernel)
            if "density" in channels:
                out["density"] = torch.relu(sigma[..., 0:1]).reshape(batch, num_samples, 1)
        if "rgb" in channels:
            if ray_d is None or tuple(ray_d.shape) != (batch, 3):
                raise ValueError("PanopticLiftingNeF: rgb needs ray_d of shape [%d,3] (one direction per batch entry), got %s"
                                 % (batch, None if ray_d is None else tuple(ray_d.shape)))
            if num_samples != 1:
                ray_d = ray_d[:, None].repeat(1, num_samples, 1).reshape(-1, 3)
            out["rgb"] = self._decode(self.decoder_color, -ray_d, app.reshape(-1, APP_DIM))
        act = _ACTS[self.sem_activation_type]
        if "semantics" in channels:
            sem = self._decode(lambda x: self.decoder_semantics(x, act), coords)
            out["semantics"] = self._post(sem, self.sem_sigmoid, self.sem_normalize, self.sem_softmax)
        if "inst_embedding" in channels:
            inst = self._decode(lambda x: self.decoder_inst(x, act), coords)        # the reference's quirk: the semantic head's activation
            out["inst_embedding"] = self._post(inst, self.inst_sigmoid, self.inst_normalize, self.inst_softmax)
        return out

    @torch.no_grad()
    def prune(self, jitter=None, views=None):
        """Occupancy update: occupancy <- max(density at one jittered sample per dense cell, 0.6 * occupancy), cells above (0.01 * 512) / sqrt(3)
        stay.  Density only (the density-only launch on the GPU); the views do not enter it."""
        density_decay = 0.6
        min_density = (0.01 * 512) / np.sqrt(3)
        dev, g = self.device, self.grid
        points = g.dense_points.to(dev)
        res = 2.0 ** g.blas_level
        if jitter is None:
            jitter = torch.rand(points.shape[0], 3, device=dev)
        samples = (points.float() + jitter.to(dev)) / res * 2.0 - 1.0
        if views is None:
            views = sample_unif_sphere(points.shape[0], device=dev)
        density = self.forward(coords=samples[:, None], ray_d=views.to(dev), channels="density")
        g.occupancy = g.occupancy.to(dev).float().contiguous()
        if dev.type == "cuda":
            bits = torch.empty(max(1, (g.num_cells + 31) // 32), dtype=torch.int32, device=dev)
            ops.occupancy_update(density.reshape(-1), g.occupancy, bits, density_decay, min_density)
            g.blas_init_bits(bits)
        else:
            g.occupancy = torch.stack([density[:, 0, 0], g.occupancy * density_decay], -1).max(dim=-1)[0]
            g.blas_init(g.occupancy > min_density)
