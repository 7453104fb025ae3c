"""SemanticNeF - the Semantic-NeRF comparison baseline (pc_nerf/semantic_nerf.py, configs/bup20/semantic_nerf_app.yaml) on the gfx950 kernels.

No feature grid: PE10(position) -> decoder_features (eight Linear + ReLU at hidden_dim with a skip into layer 5, then lout) -> three heads
(density Linear, colour and semantic BasicDecoders at hidden_dim / 2).  The grid is an `Occtree`: occupancy only, which OccupancyBLAS already is.

Where it runs: GPU tensors with hidden_dim = 256, ReLU and <= 16 classes take ONE fused launch for the whole network (mlp_deep.hip, bf16 operands /
fp32 accumulation; include/pagnerf_hip.h states the rounding points) behind one autograd.Function; anything else - other widths, activations, class
counts, precision="fp32", CPU tensors - takes the tensor-op path below in fp32, which is the reference's arithmetic.

The skip layer's column order is [x | h] (the embedded position in the first 63 columns), wisp BasicDecoder(skip=[5])'s: SURVEY Appendix A1.
The nef does not set `accepts_ray_index`, so the tracer hands it a per-sample ray_d and training traces take the eager path (GraphRunner.eligible).
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .grids import OccupancyBLAS
from .nef import _param_names, positional_embed

_ACTS = {"relu": torch.relu, "sin": torch.sin, "none": (lambda x: x)}
CH_BITS = {"density": 1, "rgb": 2, "semantics": 4}
POS_FREQS = 10          # semantic_nerf.py:37-38: both embedders are get_positional_embedder(10, True), whatever pos_multires / view_multires say


class Occtree(OccupancyBLAS):
    """grids/occtree.py::Occtree - an occupancy structure without features: one level of detail, the dense bitfield as the acceleration structure."""

    def __init__(self, blas_level=7, **kwargs):
        super().__init__(blas_level)
        self.kwargs = kwargs
        self.num_lods = 1
        self.active_lods = [0]


class PositionalEmbedder(nn.Module):
    """wisp PositionalEmbedder's parameter layout (a non-trainable `bands`) and arithmetic."""

    def __init__(self, num_freq):
        super().__init__()
        self.num_freq = num_freq
        self.bands = nn.Parameter(2.0 ** torch.linspace(0.0, num_freq - 1, num_freq), requires_grad=False)

    def forward(self, x):
        return positional_embed(x, self.num_freq)


class SkipDecoder(nn.Module):
    """wisp BasicDecoder's parameter layout (layers[i], lout) with skip connections: a layer i in `skip` reads cat([x, h])."""

    def __init__(self, input_dim, output_dim, num_layers, hidden_dim, skip=(), bias=True):
        super().__init__()
        self.input_dim, self.output_dim, self.skip = input_dim, output_dim, tuple(skip)
        self.layers = nn.ModuleList([nn.Linear(input_dim if i == 0 else (hidden_dim + input_dim if i in self.skip else hidden_dim), hidden_dim, bias=bias)
                                     for i in range(num_layers)])
        self.lout = nn.Linear(hidden_dim, output_dim, bias=bias)

    def linears(self):
        return list(self.layers) + [self.lout]

    def forward(self, x, act=torch.relu):
        h = x
        for i, l in enumerate(self.layers):
            if i in self.skip and i > 0:
                h = torch.cat([x, h], dim=-1)
            h = act(l(h))
        return self.lout(h)


def sample_unif_sphere(n, generator=None, device=None):
    """n points uniform on the unit sphere (wisp.ops.geometric.sample_unif_sphere's construction: z uniform, azimuth uniform)."""
    u = torch.rand(2, n, generator=generator, device=device)
    z = 1.0 - 2.0 * u[0]
    r = torch.sqrt(torch.clamp(1.0 - z * z, min=0.0))
    phi = 2.0 * np.pi * u[1]
    return torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], dim=-1)


# --------------------------------------------------------------------------------------------------------------------------- fused launch
def _args(coords, ray_d, C, mask, save, W, b):
    a = L.DeepMlpArgs()
    a.coords, a.ray_d = L.ptr(coords), L.ptr(ray_d)
    a.hidden, a.num_classes, a.channels, a.save = 256, C, mask, int(save)
    for i in range(14):
        a.W[i], a.b[i] = L.ptr(W[i]), L.ptr(b[i])
    return a


def _workspace(M, C, mode, dev):
    n = L.load().pag_deep_mlp_workspace_bytes(M, 256, C, mode)
    if n < 0:
        L.check(-1, "pag_deep_mlp_workspace_bytes")
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def _prep(t):
    return t.detach().float().contiguous()


def deep_forward(coords, ray_d, C, mask, W, b, save=False):
    """One launch: -> (density [M] | None, rgb [M,3] | None, semantics [M,C] | None, workspace).  coords / ray_d f32 [M,3] GPU tensors; the kernel
    reads M rows of both, so their shapes are checked here (ray_d only where the colour head is launched)."""
    dev, M = coords.device, coords.shape[0]
    if tuple(coords.shape) != (M, 3) or coords.dtype != torch.float32 or not coords.is_contiguous():
        raise ValueError("deep_forward: coords must be a contiguous f32 [M,3] tensor, got %s %s" % (tuple(coords.shape), coords.dtype))
    if mask & 2 and (ray_d is None or tuple(ray_d.shape) != (M, 3) or ray_d.dtype != torch.float32 or not ray_d.is_contiguous()
                     or ray_d.device != dev):
        raise ValueError("deep_forward: the colour head needs one direction per sample, a contiguous f32 [%d,3] tensor on %s, got %s"
                         % (M, dev, None if ray_d is None else (tuple(ray_d.shape), ray_d.dtype, ray_d.device)))
    density = torch.empty(M, device=dev) if mask & 1 else None
    rgb = torch.empty(M, 3, device=dev) if mask & 2 else None
    sem = torch.empty(M, C, device=dev) if mask & 4 else None
    if M == 0:
        return density, rgb, sem, None
    a = _args(coords, ray_d if mask & 2 else None, C, mask, save, W, b)
    ws, n = _workspace(M, C, 1 if save else 0, dev)
    a.density, a.rgb, a.semantics = L.ptr(density), L.ptr(rgb), L.ptr(sem)
    a.workspace, a.workspace_bytes = L.ptr(ws), n
    with torch.cuda.device(dev):
        L.check(L.load().pag_deep_mlp_fwd(ctypes.byref(a), M, L.stream()), "pag_deep_mlp_fwd")
    return density, rgb, sem, ws


class _DeepMLP(torch.autograd.Function):
    """The whole network as one node: forward = one launch that keeps every Linear's bf16 input, backward = data-gradient chain + weight gradients
    (pag_deep_mlp_bwd).  Inputs after C: the 14 weights, then the 14 biases (trunk 0..7, lout, density, colour 0 / lout, semantics 0 / lout)."""

    @staticmethod
    def forward(ctx, coords, ray_d, C, *params):
        W, b = [_prep(p) for p in params[:14]], [_prep(p) for p in params[14:]]
        density, rgb, sem, ws = deep_forward(coords, ray_d, C, 7, W, b, save=True)
        ctx.save_for_backward(coords, ray_d, density, rgb, *W, *b)
        ctx.ws, ctx.C, ctx.M = ws, C, coords.shape[0]
        ctx.set_materialize_grads(False)
        return density, rgb, sem

    @staticmethod
    def backward(ctx, g_density, g_rgb, g_sem):
        if ctx.ws is None and ctx.M:
            raise RuntimeError("SemanticNeF: the fused decoder's saved activations are released by its first backward (they are 5.4 KB per sample); "
                               "a second backward through the same forward (retain_graph=True) is not supported - run the forward again")
        coords, ray_d, density, rgb = ctx.saved_tensors[:4]
        W, b = ctx.saved_tensors[4:18], ctx.saved_tensors[18:]
        dev, M, C = coords.device, coords.shape[0], ctx.C
        dW, db = [torch.zeros_like(w) for w in W], [torch.zeros_like(x) for x in b]
        if M:
            a = _args(coords, ray_d, C, 7, True, W, b)
            g = [_prep(t) if t is not None else None for t in (g_density, g_rgb, g_sem)]
            a.density, a.rgb = L.ptr(density), L.ptr(rgb)
            a.workspace, a.workspace_bytes = L.ptr(ctx.ws), ctx.ws.numel()
            a.g_density, a.g_rgb, a.g_semantics = L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2])
            for i in range(14):
                a.dW[i], a.db[i] = L.ptr(dW[i]), L.ptr(db[i])
            ws, n = _workspace(M, C, 2, dev)
            a.bwd_workspace, a.bwd_workspace_bytes = L.ptr(ws), n
            with torch.cuda.device(dev):
                L.check(L.load().pag_deep_mlp_bwd(ctypes.byref(a), M, L.stream()), "pag_deep_mlp_bwd")
            ctx.ws = None
        return (None, None, None, *dW, *db)


class SemanticNeF(nn.Module):
    """pc_nerf/semantic_nerf.py::SemanticNeF: same constructor keywords (the rest is swallowed), parameter names and shapes, channels and shapes."""

    def __init__(self, num_classes=-1, hidden_dim=128, activation_type="relu", layer_type="none", blas_level=7, precision="bf16", **kwargs):
        super().__init__()
        if activation_type not in _ACTS:
            raise NotImplementedError("activation_type '%s'" % activation_type)
        assert num_classes >= 1, "SemanticNeF needs num_classes"
        self.num_classes, self.hidden_dim, self.activation_type, self.layer_type = num_classes, hidden_dim, activation_type, layer_type
        self.kwargs = kwargs
        self.grid = Occtree(blas_level=blas_level)                                          # :83-90
        self.view_embedder, self.view_embed_dim = PositionalEmbedder(POS_FREQS), 3 + 6 * POS_FREQS      # :37-38
        self.pos_embedder, self.pos_embed_dim = PositionalEmbedder(POS_FREQS), 3 + 6 * POS_FREQS
        self.decoder_features = SkipDecoder(self.pos_embed_dim, hidden_dim, 8, hidden_dim, skip=(5,))    # :48-55
        self.decoder_density = nn.Linear(hidden_dim, 1, bias=True)                           # :57-58
        with torch.no_grad():
            self.decoder_density.bias[0] = 1.0
        self.decoder_color = SkipDecoder(hidden_dim + self.view_embed_dim, 3, 1, hidden_dim // 2)        # :60-67
        self.decoder_semantics = SkipDecoder(hidden_dim, num_classes, 1, hidden_dim // 2)                # :69-76
        self.set_precision(precision)
        self._fns = [(self.rgb_semantics, {"density", "rgb", "semantics"})]

    def set_precision(self, precision):
        """'bf16': the fused bf16-operand launch where it applies; 'fp32': always the fp32 tensor-op path."""
        assert precision in ("bf16", "fp32")
        self.precision = precision

    @property
    def device(self):
        return self.decoder_density.weight.device

    def get_nef_type(self):
        return "panoptic_nef"                                                                 # :92-98

    def get_supported_channels(self):
        return {"density", "rgb", "semantics"}

    def forward(self, channels=None, **kwargs):
        """wisp BaseNeuralField.forward semantics: str -> tensor, list -> list, set -> dict."""
        kwargs["compute_channels"] = channels                                                 # :127-130
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

    # ------------------------------------------------------------------------------------------------------------------------ the network
    def linears(self):
        """The 14 Linears in the order of the C ABI: trunk layers 0..7, lout, density, colour layers[0] / lout, semantics layers[0] / lout."""
        return self.decoder_features.linears() + [self.decoder_density] + self.decoder_color.linears() + self.decoder_semantics.linears()

    def fused_supported(self):
        return self.hidden_dim == 256 and self.activation_type == "relu" and 1 <= self.num_classes <= 16

    def tensor_forward(self, x, ray_d, channels):
        """The reference's arithmetic in tensor ops (:188-224) on flat [M,3] positions and per-sample directions."""
        act = _ACTS[self.activation_type]
        out = {}
        feats = self.decoder_features(self.pos_embedder(x), act)
        if "density" in channels or "rgb" in channels:
            density = torch.relu(self.decoder_density(feats)[..., 0:1])
            if "density" in channels:
                out["density"] = density
        if "rgb" in channels:
            out["rgb"] = torch.sigmoid(self.decoder_color(torch.cat([feats, self.view_embedder(-ray_d)], dim=-1), act))
        if "semantics" in channels:
            out["semantics"] = self.decoder_semantics(feats, act)
        return out

    def rgb_semantics(self, coords, ray_d=None, compute_channels=None, pidx=None, lod_idx=None):
        out = {}
        if not compute_channels:
            return out
        channels = {compute_channels} if isinstance(compute_channels, str) else set(compute_channels)
        batch, num_samples, _ = coords.shape
        x = coords.reshape(-1, 3)
        if "rgb" in channels:
            if ray_d is None or tuple(ray_d.shape) != (batch, 3):
                raise ValueError("SemanticNeF: rgb needs ray_d of shape [%d,3] (one direction per batch entry), got %s"
                                 % (batch, None if ray_d is None else tuple(ray_d.shape)))
            if num_samples != 1:                                                               # :209-210: one direction per batch entry
                ray_d = ray_d[:, None].repeat(1, num_samples, 1).reshape(-1, 3)
        else:
            ray_d = None                                                                       # only the colour head reads it (:209-216)
        if not (x.is_cuda and self.precision == "bf16" and self.fused_supported()):
            res = self.tensor_forward(x.float(), ray_d.float() if ray_d is not None else None, channels)
        else:
            res = self._fused(x, ray_d, channels)
        shapes = {"density": (batch, num_samples, 1), "rgb": (batch, num_samples, 3)}
        for c in channels:
            out[c] = res[c].reshape(shapes[c]) if c in shapes else res[c]                      # semantics stays [M, C] (:224)
        return out

    def _fused(self, x, ray_d, channels):
        """x [M,3]; ray_d [M,3] per sample, or None when rgb is not requested.  Under no_grad the launch runs the heads of the requested channels
        only.  With gradients enabled it ignores the channel mask: the one autograd node always runs all three heads and keeps every Linear's
        input (5.4 KB per sample), whatever was asked for; channels that were not requested get directions of zero where none were given, are
        dropped by the caller and receive no gradient.  A density-only call that needs no gradient belongs under no_grad (as prune() does)."""
        lins = self.linears()
        W, b = [l.weight for l in lins], [l.bias for l in lins]
        train = torch.is_grad_enabled() and any(p.requires_grad for p in W + b)
        if torch.is_grad_enabled() and (x.requires_grad or (ray_d is not None and ray_d.requires_grad)):
            raise RuntimeError("SemanticNeF: the fused decoder has no gradient with respect to coords / ray_d (the configuration does not optimise "
                               "extrinsics); detach them, or use precision='fp32' for the tensor-op path")
        x = _prep(x)
        if train:
            d = _prep(ray_d) if "rgb" in channels else torch.zeros_like(x)
            density, rgb, sem = _DeepMLP.apply(x, d, self.num_classes, *W, *b)
        else:
            mask = sum(CH_BITS[c] for c in channels)
            density, rgb, sem, _ = deep_forward(x, _prep(ray_d) if mask & 2 else None, self.num_classes, mask, [_prep(w) for w in W], [_prep(v) for v in b])
        return {"density": density, "rgb": rgb, "semantics": sem}

    # ------------------------------------------------------------------------------------------------------------------------------ prune
    @torch.no_grad()
    def prune(self, jitter=None, views=None):
        """Occupancy update (:100-125): occupancy <- max(density at one jittered sample per dense cell, 0.6 * occupancy), cells above
        (0.01 * 512) / sqrt(3) stay.  Density only; the views (uniform on the sphere, as the reference draws them) do not enter it."""
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
            ops.occupancy_update(density.reshape(-1), g.occupancy, bits, density_decay, min_density)   # EMA-max + threshold + pack, as nef.py
            g.blas_init_bits(bits)
        else:
            g.occupancy = torch.stack([density[:, 0, 0], g.occupancy * density_decay], -1).max(dim=-1)[0]
            g.blas_init(g.occupancy > min_density)
