"""The grid total-variation regularisers (loss/regularizers.py:41-70, called at pc_nerf/trainer.py:556-574; switched by `grid_tvl1_reg`, `grid_tvl2_reg`,
`delta_grid_tvl1_reg`, `delta_grid_tvl2_reg` with `tv_window_size` and `tv_edge_num_samples`) on pag_tv_fwd / pag_tv_bwd (csrc/regularizer.hip).

    tv_loss(values, power), tv_l1_loss, tv_l2_loss        the total variation of a channel-last lattice
    grid_tv_loss(encoder, fn, ...), grid_tv_l1_loss, grid_tv_l2_loss      the lattice of points, the encoder on it, the total variation of what it returns
    step_tv_terms(nef, ...)                               trainer.py:556-574 as one call: the four weighted terms of a step's loss, a 0-dim tensor

The tensor-op form `tv_loss_form` is the definition (the convention of triplanar.py): the kernels are tested against it, and it is what CPU tensors, ranks
above 4, fp64 and `TV_KERNELS = False` / PAG_TV_KERNELS=0 take.  What the reference does and this module reproduces on purpose:
the lattice spacing is 1.0, not sample_size / n; 'ij' mesh indexing; every axis's sum is divided by values.shape[0]; the `delta_grid_tvl2_reg` branch calls
the L1 function; both delta branches run only when the nef has a `delta_grid`.
"""
import os

import torch

from . import _lib as L
from . import ops

TV_KERNELS = os.environ.get("PAG_TV_KERNELS", "1") != "0"      # False / PAG_TV_KERNELS=0: the tensor-op form on GPU tensors too (tests, A/B)


def tv_loss_form(values, power):
    """loss/regularizers.py:41-54 as written: per lattice axis the |.| (power 1) or (.)^2 (power 2) of the differences of neighbours, summed, every axis
    divided by values.shape[0] (:43, :47).  Half inputs: the same on values.float() (autograd casts the gradient back to the input dtype)."""
    if values.dtype in (torch.float16, torch.bfloat16):
        values = values.float()
    size = values.shape[0]
    loss = values.new_zeros(())
    for d in range(values.dim() - 1):
        vals_d = torch.swapdims(values, d, 0)
        diff = vals_d[1:] - vals_d[:-1]
        loss = loss + (torch.abs(diff) if power == 1 else torch.pow(diff, 2)).sum() / size
    return loss


class _TV(torch.autograd.Function):
    """pag_tv_fwd / pag_tv_bwd: two launches forward, one backward; the upstream scalar is read on the device."""

    @staticmethod
    def forward(ctx, values, power):
        dims = list(values.shape[:-1]) + [1] * (4 - values.dim())
        C = values.shape[-1]
        lib = L.load()
        nbytes = int(lib.pag_tv_workspace_bytes(*dims, C))
        ws = torch.empty(max(nbytes, 1), device=values.device, dtype=torch.uint8)
        out = torch.empty(1, device=values.device)
        ops._call("pag_tv_fwd", values.data_ptr(), L.dtype_code(values), *dims, C, power, ws.data_ptr(), nbytes, out.data_ptr(), L.stream())
        ctx.save_for_backward(values)
        ctx.power, ctx.dims = power, dims
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        values, = ctx.saved_tensors
        g = g.reshape(1).float().contiguous()
        grad = torch.empty_like(values)
        ops._call("pag_tv_bwd", values.data_ptr(), L.dtype_code(values), *ctx.dims, values.shape[-1], ctx.power, g.data_ptr(), grad.data_ptr(), L.stream())
        return grad, None


def tv_loss(values, power):
    """Total variation of `values` [..., C] (any rank >= 2, the last dimension is the channels): a 0-dim fp32 tensor (the dtype of fp64 input for fp64).

    Non-empty CUDA tensors of rank 2 - 4 in fp32 / fp16 / bf16 take the kernels (one read forward, one read and one write backward, fixed-order sums: the
    same input gives the same bits); a non-contiguous input is made contiguous first.  Everything else takes tv_loss_form."""
    if power not in (1, 2):
        raise ValueError("tv_loss: power must be 1 or 2, got %r" % (power,))
    if values.dim() < 2:
        raise ValueError("tv_loss: values must have rank >= 2 ([..., C]), got shape %s" % (tuple(values.shape),))
    if TV_KERNELS and values.is_cuda and values.dim() <= 4 and values.dtype in L._DT and values.numel() > 0:
        return _TV.apply(values.contiguous(), power)
    return tv_loss_form(values, power)


def tv_l1_loss(values):
    return tv_loss(values, 1)


def tv_l2_loss(values):
    return tv_loss(values, 2)


def grid_tv_loss(encoder, fn, sample_size=0.2, num_dim_samples=50, device="cuda", *, step=1.0, min_vertex=None):
    """loss/regularizers.py:56-64: `fn` of the encoder's output on a lattice of (num_dim_samples + 1)^3 points.

    `encoder` is any callable on [K,1,3] coordinates: `grid.interpolate` of any grid class here, or
    `lambda x: nef(coords=x, ray_d=None, channels='inst_embedding')` (trainer.py:566).  Its output is reshaped to [n+1, n+1, n+1, -1].

    As in the reference the lattice is `min_vertex + arange(n + 1)` - spacing 1.0 - with `min_vertex = randn(3) * 2 * (1 - sample_size) - 1` drawn from the
    CPU default generator, and coords[i, j, k] = (ex[i], ey[j], ez[k]).  `step` and `min_vertex` (keyword only, this project's additions) set the spacing and
    the first vertex for callers who want the window the option name suggests: `step=sample_size / num_dim_samples` spans a cube of edge sample_size; a given
    `min_vertex` draws no random number."""
    n = int(num_dim_samples)
    if min_vertex is None:
        min_vertex = torch.randn(3) * 2 * (1 - sample_size) - 1
    else:
        min_vertex = torch.as_tensor(min_vertex, dtype=torch.float32).reshape(3).cpu()
    steps = torch.arange(n + 1).to(torch.float32) * float(step)                       # step 1.0: the reference's arange(n + 1), exactly
    edge_coords = min_vertex + torch.stack([steps for _ in range(3)], dim=-1)         # [n+1, 3]
    coords = torch.stack(torch.meshgrid(*edge_coords.unbind(dim=-1), indexing="ij"), dim=-1).to(device)
    values = encoder(coords.reshape(-1, 1, 3))
    return fn(values.reshape(n + 1, n + 1, n + 1, -1))


def grid_tv_l1_loss(encoder, *args, **kwargs):
    return grid_tv_loss(encoder, tv_l1_loss, *args, **kwargs)


def grid_tv_l2_loss(encoder, *args, **kwargs):
    return grid_tv_loss(encoder, tv_l2_loss, *args, **kwargs)


def _nef_device(nef):
    for p in (nef.parameters() if hasattr(nef, "parameters") else ()):
        return p.device
    return torch.device("cpu")


def step_tv_terms(nef, grid_tvl1_reg=0.0, grid_tvl2_reg=0.0, delta_grid_tvl1_reg=0.0, delta_grid_tvl2_reg=0.0, tv_window_size=0.0001, tv_edge_num_samples=100,
                  **lattice):
    """pc_nerf/trainer.py:556-574 as one call: the weighted TV terms a step adds to its loss, a 0-dim tensor on the nef's device (zero when every weight is 0).
    The defaults of `tv_window_size` / `tv_edge_num_samples` are the shipped YAMLs' (0.0001, 100).

        grid_tvl1_reg        * grid_tv_l1_loss(nef.grid.interpolate)
        grid_tvl2_reg        * grid_tv_l2_loss(nef.grid.interpolate)
        delta_grid_tvl1_reg  * grid_tv_l1_loss(lambda x: nef(coords=x, ray_d=None, channels='inst_embedding'))      only with a nef.delta_grid
        delta_grid_tvl2_reg  * grid_tv_l1_loss(the same)     - the L1 function, as the reference (:571-574)       only with a nef.delta_grid

    Each term draws its own lattice (one randn(3) from the CPU generator each, in this order).  `lattice` passes `step=` / `min_vertex=` on to grid_tv_loss.
    The instance terms go through the nef's forward, which leaves its per-trace caches set; they are cleared here, as the tracer does after a trace."""
    dev = _nef_device(nef)
    kw = dict(sample_size=tv_window_size, num_dim_samples=tv_edge_num_samples, device=dev, **lattice)
    total = torch.zeros((), device=dev)
    if grid_tvl1_reg > 0.0:
        total = total + grid_tv_l1_loss(nef.grid.interpolate, **kw).mean() * grid_tvl1_reg
    if grid_tvl2_reg > 0.0:
        total = total + grid_tv_l2_loss(nef.grid.interpolate, **kw).mean() * grid_tvl2_reg

    def inst_nef_func(x):
        try:
            return nef(coords=x, ray_d=None, channels="inst_embedding")
        finally:
            for attr in ("_feat_cache", "_density_feats", "_prefetched"):
                if getattr(nef, attr, None) is not None:
                    setattr(nef, attr, None)
    has_delta = "delta_grid" in dir(nef)
    if delta_grid_tvl1_reg > 0.0 and has_delta:
        total = total + grid_tv_l1_loss(inst_nef_func, **kw).mean() * delta_grid_tvl1_reg
    if delta_grid_tvl2_reg > 0.0 and has_delta:
        total = total + grid_tv_l1_loss(inst_nef_func, **kw).mean() * delta_grid_tvl2_reg
    return total
