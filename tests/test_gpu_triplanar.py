"""TriplanarGridHIP's kernels (csrc/triplanar.hip) on the GPU against the grid's own tensor-op form (the grid_sample expression that defines it) on the
same inputs, and through the nefs, the tracer (graph and eager path), the optimiser, pose optimisation and prune.  Reads only the repository.

Gates (the project's own for this arithmetic, as in test_gpu_panoptic_lifting.py): fp32 outputs rtol 1e-5 / atol 2e-6, fp32 gradients rtol 2e-4 /
atol 2e-5, and per tensor a rel-L2 distance to the tensor-op form run in fp64 of at most 3 x floor + 1e-6, where the floor is the distance between the
tensor-op form in fp32 and in fp64 on those inputs (computed here from the reference alone and printed; the g15 / g16 convention).  The table gradients
are float atomic sums on both sides: their last bits depend on the arrival order.  The absolute tolerances are sized for tables of the configuration's
scale: feature_std is the configuration's 0.01 at the configuration's shape and 0.1 at the small shapes (the position gradient carries a factor (R - 1) / 2)."""
import copy

import numpy as np
import pytest
import torch

import test_gpu_parity as T

pytestmark = pytest.mark.gpu


def _grid(dev, base_lod=1, L=2, F=4, seed=3, std=0.1, **kw):
    from pagnerf_amd import TriplanarGridHIP
    torch.manual_seed(seed)
    return TriplanarGridHIP(F, base_lod=base_lod, num_lods=L, feature_std=std, feature_bias=0.1, blas_level=3, **kw).to(dev)


def _border_points():
    pts = [[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]
    pts += [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]
    pts += [[1.25, -1.25, 0.999999], [-1.25, 0.999999, 1.25], [0.0, 0.5, -0.5], [0.999999, 0.999999, 0.999999]]
    return torch.tensor(pts)


def _inputs(M, dev, seed, borders=True, C=8):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(M, 3, generator=g) * 2.6 - 1.3                                # some points outside the cube
    if borders and M >= 33:
        b = _border_points()
        x[:b.shape[0]] = b
    return x.to(dev), torch.randn(M, C, generator=g).to(dev)


def _run(grid, x, G, use_kernel, need_x=False, feat_scale=None, dtype=torch.float32):
    """-> (features, table gradient, position gradient | None) of sum(features * G)."""
    grid.use_kernel = use_kernel
    grid.tables.grad = None
    xx = x.detach().to(dtype).clone().requires_grad_(need_x)
    out = grid.interpolate_scaled(xx[:, None], feat_scale, out_dtype=dtype)
    (out * G.to(dtype)).sum().backward()
    grid.use_kernel = None
    return out.detach(), grid.tables.grad.detach().clone(), (xx.grad.detach().clone() if need_x else None)


def _close(a, b, rtol, atol, what):
    np.testing.assert_allclose(a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy(), rtol=rtol, atol=atol, err_msg=what)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def _check(grid, x, G, need_x=False, feat_scale=None, what=""):
    """The kernels against the tensor-op form: elementwise gates, and per tensor within 3 x floor + 1e-6 of the fp64 run."""
    got = _run(grid, x, G, True, need_x, feat_scale)
    want = _run(grid, x, G, False, need_x, feat_scale)
    g64 = copy.deepcopy(grid).double()
    ref = _run(g64, x, G, False, need_x, feat_scale, dtype=torch.float64)
    assert got[0].shape == want[0].shape and got[1].shape == grid.tables.shape and got[1].dtype == torch.float32 and got[1].is_contiguous()
    _close(got[0], want[0], 1e-5, 2e-6, what + " features")
    _close(got[1], want[1], 2e-4, 2e-5, what + " table gradient")
    names = ["features", "table gradient"] + (["position gradient"] if need_x else [])
    if need_x:
        assert got[2].shape == x.shape
        _close(got[2], want[2], 2e-4, 2e-5, what + " position gradient")
    if x.shape[0] == 0:
        return got
    for n, k, w, r in zip(names, got, want, ref):
        floor, dist = _rel(w, r), _rel(k, r)
        print("%s %-18s floor (tensor-op fp32 vs fp64) %.3e   kernel vs fp64 %.3e" % (what, n, floor, dist))
        assert dist <= 3.0 * floor + 1e-6, (what, n, dist, floor)
    return got


SHAPES = [(1, 2, 4), (1, 4, 2), (1, 4, 8)]


@pytest.mark.parametrize("M", [0, 1, 33, 1000])
@pytest.mark.parametrize("base_lod,L,F", SHAPES)
def test_sizes_forward_and_table_gradient(gpu_device, M, base_lod, L, F):
    grid = _grid(gpu_device, base_lod, L, F)
    x, G = _inputs(M, gpu_device, seed=M + F, C=L * F)
    assert grid.kernel_supported(x)
    got = _check(grid, x, G, what="M=%d L=%d F=%d" % (M, L, F))
    assert got[0].shape == (M, L * F)
    if M == 0:
        assert float(got[1].abs().sum()) == 0.0


def test_config_shape_and_feat_scale(gpu_device):
    """configs/bup20/mean_shift_contrastive_app.yaml:137-144: base_lod 5, 4 levels, F = 4, feature_std 0.01; M = 4096 is more than one workgroup of every kernel."""
    grid = _grid(gpu_device, 5, 4, 4, std=0.01)
    assert grid.resolutions == [33, 65, 129, 257] and grid.tables.numel() == (33 ** 2 + 65 ** 2 + 129 ** 2 + 257 ** 2) * 12
    x, G = _inputs(4096, gpu_device, seed=11, C=16)
    _check(grid, x, G, what="config")
    fs = torch.linspace(0.5, 2.0, 16)
    _check(grid, x, G, feat_scale=fs, what="config feat_scale")


@pytest.mark.parametrize("kind", ["one_cell", "one_ray"])
def test_contention(gpu_device, kind):
    """2000 samples inside one coarse cell / 2000 consecutive samples along one ray: the register-merged runs and the atomics meet the same gates."""
    grid = _grid(gpu_device, 5, 4, 4, std=0.01)
    g = torch.Generator().manual_seed(4)
    if kind == "one_cell":                    # one cell of the 33-wide level is 1/16 wide: [0.0625, 0.125]^3
        x = 0.0625 + torch.rand(2000, 3, generator=g) * 0.0625
    else:
        t = torch.linspace(0.0, 2.0, 2000)[:, None]
        x = torch.tensor([[-0.9, -0.7, -0.8]]) + t * torch.nn.functional.normalize(torch.tensor([[1.0, 0.8, 0.9]]), dim=-1)
    G = torch.randn(2000, 16, generator=g)
    _check(grid, x.to(gpu_device), G.to(gpu_device), what=kind)


def test_zero_upstream_gradient_contributes_nothing(gpu_device):
    from pagnerf_amd import triplanar as TP
    grid = _grid(gpu_device, 1, 4, 4)
    x, G = _inputs(500, gpu_device, seed=8, C=16)
    G[100:300] = 0.0
    g1 = TP.triplanar_backward_tables(grid._spec, x, G)
    keep = torch.cat([torch.arange(0, 100), torch.arange(300, 500)]).to(gpu_device)
    g2 = TP.triplanar_backward_tables(grid._spec, x[keep].contiguous(), G[keep].contiguous())
    _close(g1, g2, 2e-4, 2e-5, "zeroed block")
    assert float(g1.abs().sum()) > 0
    x_bad = x.clone()
    x_bad[100:300] = float("nan")             # skipped samples are not even looked at
    _close(TP.triplanar_backward_tables(grid._spec, x_bad, G), g2, 2e-4, 2e-5, "zeroed block, NaN coordinates")
    g0 = TP.triplanar_backward_tables(grid._spec, x, torch.zeros_like(G))
    assert float(g0.abs().max()) == 0.0
    out = grid.interpolate_scaled(x[:, None])
    (out * 0.0).sum().backward()
    assert float(grid.tables.grad.abs().max()) == 0.0


@pytest.mark.parametrize("base_lod,L,F", SHAPES + [(5, 4, 4)])
def test_position_gradient(gpu_device, base_lod, L, F):
    """Random coordinates only: the gradient is discontinuous on lattice lines and at the reflection border, where two correct implementations may
    take either side.  No sample is excluded."""
    grid = _grid(gpu_device, base_lod, L, F, std=0.01 if base_lod == 5 else 0.1)          # the config's feature_std at the config's shape
    x, G = _inputs(1000, gpu_device, seed=21 + F, borders=False, C=L * F)
    got = _check(grid, x, G, need_x=True, what="xyz L=%d F=%d" % (L, F))
    assert float(got[2].abs().sum()) > 0
    fs = torch.linspace(0.5, 2.0, L * F)
    _check(grid, x, G, need_x=True, feat_scale=fs, what="xyz feat_scale L=%d F=%d" % (L, F))


def test_non_finite_and_huge_coordinates_stay_inside_the_table(gpu_device):
    grid = _grid(gpu_device, 1, 2, 4)
    x = torch.tensor([[float("nan"), 0.0, 0.0], [float("inf"), 0.1, 0.2], [-float("inf"), 0.1, 0.2], [1e30, -1e30, 3e38], [0.2, 0.3, 0.4]], device=gpu_device)
    xx = x.clone().requires_grad_(True)
    out = grid.interpolate_scaled(xx[:, None])
    out[4].sum().backward()
    torch.cuda.synchronize()
    ref = grid.tensor_forward(x[4:5])
    _close(out[4:5], ref, 1e-5, 2e-6, "finite row")
    assert torch.isfinite(xx.grad[4]).all() and float(xx.grad[:4].abs().sum()) == 0.0


def test_bf16_output_and_bf16_upstream_gradient(gpu_device):
    grid = _grid(gpu_device, 1, 4, 4)
    x, G = _inputs(1000, gpu_device, seed=5, C=16)
    fs = torch.linspace(0.5, 2.0, 16)
    with torch.no_grad():
        f32 = grid.interpolate_scaled(x[:, None], fs)
        b16 = grid.interpolate_scaled(x[:, None], fs, out_dtype=torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and torch.equal(b16, f32.to(torch.bfloat16))
    xx = x.clone().requires_grad_(True)
    out = grid.interpolate_scaled(xx[:, None], fs, out_dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and torch.equal(out.detach(), b16)
    out.backward(G.bfloat16())
    got_t, got_x = grid.tables.grad.clone(), xx.grad.clone()
    want = _run(grid, x, G.bfloat16().float(), False, need_x=True, feat_scale=fs)
    _close(got_t, want[1], 2e-4, 2e-5, "table gradient from a bf16 upstream gradient")
    _close(got_x, want[2], 2e-4, 2e-5, "position gradient from a bf16 upstream gradient")


# ---------------------------------------------------------------------------------------------------------------------------- through the nef
NEF_KW = dict(grid_type="TriplanarGrid", feature_dim=4, base_lod=1, num_lods=4, feature_std=0.3, num_classes=6, num_instances=8, sem_softmax=True,
              inst_softmax=False, inst_normalize=True, blas_level=3)


def _nef(cls_name, dev, precision, seed=0, **kw):
    import pagnerf_amd
    torch.manual_seed(seed)
    args = dict(NEF_KW, precision=precision)
    args.update(kw)
    if cls_name == "PanopticDeltaNeF":
        args.update(panoptic_features_type="delta")
    return getattr(pagnerf_amd, cls_name)(**args).to(dev)


def _set_kernel(nef, use):
    for g in (nef.grid, getattr(nef, "delta_grid", None)):
        if g is not None:
            g.use_kernel = use


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("cls_name", ["MeanShiftPanopticNeF", "PanopticDeltaNeF"])
def test_nef_channels_and_gradients_match_the_tensor_op_grid(gpu_device, cls_name, precision):
    """64 rays x 32 samples through the nef with the grid on the kernels and on tensor ops: fp32 at the fp32 gates above; bf16 at the gates of this
    repository's bf16 nef tests (channels rtol 3e-2 / atol 3e-2: test_gpu_base_nef; gradients rel-L2 2e-2: test_gpu_train_step)."""
    dev = gpu_device
    nef = _nef(cls_name, dev, precision)
    assert nef._grouped() is None
    gen = torch.Generator().manual_seed(2)
    M = 64 * 32
    coords = (torch.rand(M, 1, 3, generator=gen) * 2.2 - 1.1).to(dev)
    ray_d = torch.nn.functional.normalize(torch.randn(M, 3, generator=gen), dim=-1).to(dev)
    chans = {"density", "rgb", "semantics", "inst_embedding"}
    res = {}
    for use in (True, False):
        _set_kernel(nef, use)
        nef.zero_grad(set_to_none=True)
        out = nef(coords=coords, ray_d=ray_d, pidx=None, lod_idx=None, channels=chans)
        gg = torch.Generator().manual_seed(3)
        loss = sum((out[c].float() * (torch.randn(out[c].shape, generator=gg) / 45.0).to(dev)).sum() for c in sorted(chans))
        loss.backward()
        res[use] = ({c: out[c].detach().float() for c in chans}, {n: p.grad.detach().clone() for n, p in nef.named_parameters() if p.grad is not None})
    assert set(res[True][1]) == set(res[False][1]) and "grid.tables" in res[True][1]
    assert ("delta_grid.tables" in res[True][1]) == (cls_name == "PanopticDeltaNeF")
    for c in chans:
        tol = dict(rtol=1e-5, atol=2e-6) if precision == "fp32" else dict(rtol=3e-2, atol=3e-2)
        _close(res[True][0][c], res[False][0][c], what="%s %s" % (precision, c), **tol)
    for n, want in res[False][1].items():
        got = res[True][1][n]
        assert torch.isfinite(got).all() and float(want.abs().max()) > 0, n
        if precision == "fp32":
            _close(got, want, 2e-4, 2e-5, n)
        else:
            assert T._rel_l2(got.float(), want.float()) < 2e-2, (n, T._rel_l2(got.float(), want.float()))


def _scene(dev, precision, N=64, S=32, seed=0):
    import pagnerf_amd
    nef = _nef("MeanShiftPanopticNeF", dev, precision, seed=seed, inst_detach=False, sem_detach=False)
    gen = torch.Generator().manual_seed(seed + 1)
    o = ((torch.rand(N, 3, generator=gen) - 0.5) * 0.6).to(dev)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1).to(dev)
    jitter = torch.rand(N, S, generator=gen).to(dev)
    gt = torch.rand(N, 3, generator=gen).to(dev)
    return nef, pagnerf_amd.Rays(o, d, dist_min=0.0, dist_max=2.0), jitter, gt


def _loss(rb, gt):
    return 10.0 * torch.abs(rb.rgb - gt).mean() - 0.1 * torch.log(rb.semantics.float()[:, 0] + 1e-27).mean() + 0.1 * rb.inst_embedding.float().pow(2).mean()


def test_training_steps_graph_path_equals_eager(gpu_device):
    """Four optim.Adam steps through PanopticPackedRFTracer on the graph path (eager, capture, replays) and with use_graphs=False from the same
    initial state: the losses to rtol 2e-3 (test_gpu_graphs.py::test_graph_training_tracks_eager_training) and the accumulated parameter updates to a
    rel-L2 of 1e-2 (test_gpu_graphs.py::test_graph_zero_grad_in_place_tracks_eager)."""
    import pagnerf_amd
    dev, S = gpu_device, 32
    finals = {}
    for use in (False, True):
        nef, rays, jitter, gt = _scene(dev, "bf16")
        tr = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=S, bg_color="white", use_graphs=use)
        opt = pagnerf_amd.optim.Adam(nef.parameters(), lr=1e-3)
        init = {n: p.detach().clone() for n, p in nef.named_parameters()}
        losses = []
        for it in range(4):
            opt.zero_grad(set_to_none=True)
            rb = tr(nef, channels={"rgb", "semantics", "inst_embedding"}, rays=rays, jitter=jitter, stage="train")
            loss = _loss(rb, gt)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        if use:
            assert tr._graphs.captures == 1 and tr._graphs.replays >= 2 and tr._graphs.overflows == 0, (tr._graphs.captures, tr._graphs.replays, tr._graphs.overflows)
        finals[use] = (losses, {n: p.detach() - init[n] for n, p in nef.named_parameters()})
    print("losses eager %s graph %s" % (finals[False][0], finals[True][0]))
    assert all(np.isfinite(finals[False][0])) and finals[False][0][-1] != finals[False][0][0]
    np.testing.assert_allclose(finals[True][0], finals[False][0], rtol=2e-3)
    assert float(finals[False][1]["grid.tables"].abs().max()) > 0
    for n, want in finals[False][1].items():
        e = T._rel_l2(finals[True][1][n].float(), want.float())
        assert e < 1e-2, (n, e)


def test_pose_step_gives_an_extrinsics_gradient(gpu_device):
    """One pose-optimisation step through BAPipeline (fp32 nef): d loss / d camera_extrinsics - through the grid's position gradient into the ray
    samples' node - is finite, non-zero and matches the run with the grid on tensor ops within the fp32 gradient gate."""
    from pagnerf_amd.ba_pipeline import BAPipeline
    import pagnerf_amd
    dev, N, S, C = gpu_device, 64, 32, 3
    nef, rays, jitter, gt = _scene(dev, "fp32")
    views = torch.eye(4).repeat(C, 1, 1)
    views[:, :3, 3] = torch.tensor([[0.01, -0.02, 0.0], [0.0, 0.015, -0.01], [-0.02, 0.0, 0.02]])
    tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=S, bg_color="white", use_graphs=False)
    pipe = BAPipeline(nef, views, tracer=tracer, near=0.0, far=2.0).to(dev)
    cam = torch.arange(N, device=dev) * C // N
    grads = {}
    for use in (True, False):
        _set_kernel(nef, use)
        nef.zero_grad(set_to_none=True)
        pipe.camera_extrinsics.grad = None
        world = pipe.transform_rays_indexed(rays.origins, rays.dirs, cam)
        assert world.origins.requires_grad
        rb = tracer(nef, channels={"rgb", "depth", "semantics", "inst_embedding"}, rays=world, jitter=jitter, stage="train")
        (_loss(rb, gt) + rb.depth.sum() * 0.01).backward()
        grads[use] = (pipe.camera_extrinsics.grad.clone(), nef.grid.tables.grad.clone())
    g = grads[True][0]
    print("extrinsics gradient: kernels %s\n tensor ops %s" % (g.cpu().numpy(), grads[False][0].cpu().numpy()))
    assert torch.isfinite(g).all() and float(g.abs().sum()) > 0 and g.shape == (C, 9)
    _close(g, grads[False][0], 2e-4, 2e-5, "camera_extrinsics gradient")
    _close(grads[True][1], grads[False][1], 2e-4, 2e-5, "grid.tables gradient")


def test_prune_then_voxel_march_render(gpu_device):
    import pagnerf_amd
    dev = gpu_device
    nef, rays, jitter, gt = _scene(dev, "bf16")
    with torch.no_grad():
        nef.decoder_density.lout.bias[0] = 4.0             # a dense enough field that the threshold keeps cells
    nef.prune(jitter=torch.rand(nef.grid.dense_points.shape[0], 3, generator=torch.Generator().manual_seed(1)).to(dev))
    mask = nef.grid.occupancy_mask()
    assert mask.numel() == 512 and nef.grid.occupancy.shape == (512,) and torch.isfinite(nef.grid.occupancy).all()
    tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="voxel", num_steps=2, bg_color="white", use_graphs=False)
    with torch.no_grad():
        rb = tracer(nef, channels={"rgb", "depth", "semantics", "inst_embedding"}, rays=rays, stage="val")
    assert rb.rgb.shape == (rays.origins.shape[0], 3) and torch.isfinite(rb.rgb).all() and torch.isfinite(rb.depth).all()
    if bool(mask.any()):
        assert float(rb.alpha.sum()) > 0
