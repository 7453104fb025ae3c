"""PanopticLiftingNeF's grid kernels (csrc/vm.hip) on the GPU: against the reference's golden (g16_panoptic_lifting.npz), against the nef's own
tensor-op path at the real shapes, and through the tracer, the optimiser, prune and the upsampling schedule.  Reads only the repository.

Gates (the project's own): fp32 outputs rtol 1e-5 / atol 2e-6, fp32 gradients rtol 2e-4 / atol 2e-5, and per tensor a rel-L2 distance to the golden
of at most 3 x the stored floor + 1e-6, where the floor is the distance between the reference run in fp32 and in fp64 (the g15 convention).  The table
gradients are float atomic sums, whose last bits depend on the arrival order.  The second floor the issue asks for - the distance between two GPU
runs of the tensor-op path - was measured on an MI355X (8.5e-8 .. 2.5e-7 on the table gradients, 0 elsewhere) and is smaller than the
stored floors (7.4e-7 .. 9.4e-7), so the stored floor is the larger of the two and is what gates here; the rerun test below prints the distances
and holds them to the same per-tensor gate."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
import test_panoptic_lifting_host as H

pytestmark = pytest.mark.gpu
ALL = set(H.CHANNELS)


@pytest.fixture(scope="module")
def g16():
    return golden("g16_panoptic_lifting.npz")


def _features(dev, res=H.RES, seed=5):
    from pagnerf_amd import panoptic_lifting as PL
    torch.manual_seed(seed)
    return PL.VMSplitFeatureVolume(H.DC, H.AC, res).to(dev)


def _grads(f):
    return {n: p.grad.clone() for n, p in f.named_parameters() if p.grad is not None}


def _close(a, b, rtol, atol, what):
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=what)


def test_kernel_path_matches_golden(gpu_device, g16):
    """The nef on the GPU, grid on the kernels: four channels and every parameter gradient against the reference's fp32 run, elementwise and
    within 3 x the fp32-vs-fp64 floor + 1e-6 per tensor (figures are printed first)."""
    nef = H.make_nef(device=gpu_device)
    assert nef.grid.features.kernel_supported(torch.zeros(1, 3, device=gpu_device))
    out, grads = H.run_with_upstream(nef, g16, gpu_device)
    H.check_against_golden(g16, out, grads)


def test_tensor_op_path_on_gpu_matches_golden_and_its_own_rerun(gpu_device, g16):
    """The tensor-op path on GPU tensors meets the same gates; the distance between two of its runs (its atomics' arrival order) is printed per
    tensor - the second floor DESIGN 4.17 records - and held to the gate every other comparison here uses, 3 x the stored floor + 1e-6."""
    nef = H.make_nef(device=gpu_device)
    out, grads = H.run_with_upstream(nef, g16, gpu_device, use_kernel=False)
    H.check_against_golden(g16, out, grads)
    _, again = H.run_with_upstream(nef, g16, gpu_device, use_kernel=False)
    for n in grads:
        print("tensor-op path, two GPU runs: %-40s rel-L2 %.3e" % (n, H.rel_l2(again[n], grads[n])))
    check_runs = {n: H.rel_l2(again[n], grads[n]) for n in grads}
    floors = dict(zip([str(n) for n in g16["grad_names"]], g16["grad_floors"]))
    assert all(check_runs[n] <= 3.0 * floors[n] + 1e-6 for n in grads), check_runs      # the same per-tensor gate, run against run


@pytest.mark.parametrize("M", [0, 1, 33, 1000])
def test_sizes_forward_and_backward(gpu_device, M):
    f = _features(gpu_device)
    g = torch.Generator().manual_seed(M)
    x = (torch.rand(M, 3, generator=g) * 2.2 - 1.1).to(gpu_device)              # some points outside the cube
    gs, ga = torch.randn(M, generator=g).to(gpu_device), torch.randn(M, H.APP, generator=g).to(gpu_device)
    sigma, app = f(x)
    assert sigma.shape == (M,) and app.shape == (M, H.APP) and sigma.grad_fn is not None
    (sigma * gs).sum().add((app * ga).sum()).backward()
    got = _grads(f)
    f.zero_grad()
    rs, ra = f(x, use_kernel=False)
    (rs * gs).sum().add((ra * ga).sum()).backward()
    want = _grads(f)
    _close(sigma, rs, 1e-5, 2e-6, "sigma")
    _close(app, ra, 1e-5, 2e-6, "app")
    assert set(got) == set(want) and len(got) == 13
    for n in want:
        assert got[n].is_contiguous() and got[n].shape == want[n].shape
        _close(got[n], want[n], 2e-4, 2e-5, n)
        if M == 0:
            assert float(got[n].abs().sum()) == 0.0


def test_density_only_and_appearance_only_calls(gpu_device):
    f = _features(gpu_device)
    x = (torch.rand(777, 3) * 2 - 1).to(gpu_device)
    gs, ga = torch.randn(777, device=gpu_device), torch.randn(777, H.APP, device=gpu_device)
    with torch.no_grad():
        full_s, full_a = f(x)
        s, none_a = f(x, need_app=False)                    # the 16-lanes-per-sample launch
        none_s, a = f(x, need_sigma=False)
    assert none_a is None and none_s is None
    _close(s, full_s, 1e-5, 2e-6, "density only")
    assert torch.equal(a, full_a)
    # gradients: only the requested set's tables receive one
    s, _ = f(x, need_app=False)
    (s * gs).sum().backward()
    got = _grads(f)
    assert sorted(got) == sorted(n for n, _ in f.named_parameters() if n.startswith("density"))
    f.zero_grad(set_to_none=True)
    rs, _ = f(x, need_app=False, use_kernel=False)
    (rs * gs).sum().backward()
    for n, v in _grads(f).items():
        _close(got[n], v, 2e-4, 2e-5, n)
    f.zero_grad(set_to_none=True)
    _, a = f(x, need_sigma=False)
    (a * ga).sum().backward()
    got = _grads(f)
    assert sorted(got) == sorted(n for n, _ in f.named_parameters() if not n.startswith("density"))
    f.zero_grad(set_to_none=True)
    _, ra = f(x, need_sigma=False, use_kernel=False)
    (ra * ga).sum().backward()
    for n, v in _grads(f).items():
        _close(got[n], v, 2e-4, 2e-5, n)
    # both requested, but only one used downstream: the other's upstream gradient is None
    f.zero_grad(set_to_none=True)
    s, a = f(x)
    (s * gs).sum().backward()
    assert sorted(_grads(f)) == sorted(n for n, _ in f.named_parameters() if n.startswith("density"))


def test_zero_gradient_samples_write_nothing(gpu_device):
    """Samples whose upstream gradients are exactly zero are skipped: a zeroed block gives what the call without those samples gives, and with
    every upstream gradient zero every gradient stays exactly zero."""
    from pagnerf_amd import panoptic_lifting as PL
    f = _features(gpu_device)
    x = (torch.rand(500, 3) * 2 - 1).to(gpu_device)
    tables, basis = tuple([t.detach() for t in grp] for grp in f.tables()), f.basis_mat.weight.detach()
    gs, ga = torch.randn(500, device=gpu_device), torch.randn(500, H.APP, device=gpu_device)
    gs[100:300], ga[100:300] = 0.0, 0.0
    (g1, b1) = PL.vm_backward(tables, basis, H.RES, x, gs, ga)
    keep = torch.cat([torch.arange(0, 100), torch.arange(300, 500)]).to(gpu_device)
    (g2, b2) = PL.vm_backward(tables, basis, H.RES, x[keep].contiguous(), gs[keep].contiguous(), ga[keep].contiguous())
    for a, b in zip([t for grp in g1 for t in grp] + [b1], [t for grp in g2 for t in grp] + [b2]):
        _close(a, b, 2e-4, 2e-5, "zero block")
    (g0, b0) = PL.vm_backward(tables, basis, H.RES, x, torch.zeros_like(gs), torch.zeros_like(ga))
    assert all(float(t.abs().sum()) == 0.0 for grp in g0 for t in grp) and float(b0.abs().sum()) == 0.0


def _marched_samples(dev, n_rays, steps, seed=1):
    """~n_rays x steps samples marched along rays through the unit cube by the grid's own ray march, in ray order (as a training step sees them)."""
    import pagnerf_amd
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(n_rays, 3, generator=g) * 0.6 - 0.3
    o[:, 2] = -1.6
    d = F.normalize(torch.stack([torch.rand(n_rays, generator=g) * 0.6 - 0.3, torch.rand(n_rays, generator=g) * 0.6 - 0.3, torch.ones(n_rays)], -1) - o * 0.2, dim=-1)
    grid = pagnerf_amd.TensoRF(base_resolution=2, max_resolution=6, blas_level=4).to(dev)
    rays = pagnerf_amd.Rays(o.to(dev), d.to(dev), 0.5, 2.9)          # the cube is entered at ~0.6 and left at ~2.6: ~430 of the steps fall inside
    ridx, _, samples, _, _, _ = grid.raymarch(rays, num_samples=steps, raymarch_type="ray")
    return samples.reshape(-1, 3).contiguous(), ridx


def _real_shapes(gpu_device, upsampled, n_rays, m_min, m_max):
    """Ray-ordered samples of n_rays marched rays, every third ray with zero upstream gradients: kernels against the nef's tensor-op path, the
    project's elementwise tolerances."""
    import pagnerf_amd
    torch.manual_seed(3)
    grid = pagnerf_amd.TensoRF(blas_level=4).to(gpu_device)
    if upsampled:
        grid.step_upsample_vm_grid()
    f = grid.features
    assert f.res == (144 if upsampled else 128)
    x, ridx = _marched_samples(gpu_device, n_rays, 512)
    M = x.shape[0]
    print("%d rays: %d samples, %d backward chunks" % (n_rays, M, (M + 255) // 256))
    assert m_min <= M <= m_max, M
    gs, ga = torch.randn(M, device=gpu_device), torch.randn(M, H.APP, device=gpu_device)
    dead = (ridx % 3 == 0)
    gs[dead], ga[dead] = 0.0, 0.0
    sigma, app = f(x)
    (sigma * gs).sum().add((app * ga).sum()).backward()
    got = _grads(f)
    f.zero_grad(set_to_none=True)
    rs, ra = f(x, use_kernel=False)
    (rs * gs).sum().add((ra * ga).sum()).backward()
    want = _grads(f)
    _close(sigma, rs, 1e-5, 2e-6, "sigma")
    _close(app, ra, 1e-5, 2e-6, "app")
    for n in want:
        print("%-18s rel-L2 %.3e" % (n, H.rel_l2(got[n].cpu().numpy(), want[n].cpu().numpy())))
    for n in want:
        _close(got[n], want[n], 2e-4, 2e-5, n)


@pytest.mark.parametrize("upsampled", [False, True])
def test_real_shapes_against_the_tensor_op_path(gpu_device, upsampled):
    """16 / 48 components at R = 128 (and upsampled to 144), about 2 x 10^5 samples marched along real rays, a third of them with zero upstream
    gradients: kernels against the nef's tensor-op path, the project's elementwise tolerances."""
    _real_shapes(gpu_device, upsampled, 480, 150_000, 250_000)


def test_real_shapes_past_the_backward_stride(gpu_device):
    """The backward launches at most 1024 workgroups that stride over 256-sample chunks, so a workgroup takes a second chunk - and carries the tap
    sums of the cell it was in from one chunk into the next - only with more than 1024 x 256 samples: more marched rays than above, same ray
    order, same dead-ray pattern, same gates."""
    _real_shapes(gpu_device, False, 840, 1024 * 256 + 256 + 1, 450_000)


def test_bf16_decoders_stay_within_the_bf16_tolerance(gpu_device, g16):
    """precision='bf16': the three decoders under bf16 autocast, forward only, rtol = atol = 3e-2 against the fp32 golden; the grid stays fp32, so
    the density is held to the fp32 tolerance."""
    nef = H.make_nef(device=gpu_device, precision="bf16")
    x, d = torch.from_numpy(g16["coords"]).to(gpu_device), torch.from_numpy(g16["dirs"]).to(gpu_device)
    with torch.no_grad():
        out = nef(channels=ALL, coords=x[:, None], ray_d=d)
    for c in H.CHANNELS:
        assert out[c].dtype == torch.float32 and tuple(out[c].shape) == tuple(g16[c].shape)
        tol = (1e-5, 2e-6) if c == "density" else (3e-2, 3e-2)
        np.testing.assert_allclose(out[c].cpu().numpy(), g16[c], rtol=tol[0], atol=tol[1], err_msg=c)


def _train_setup(dev, res=H.RESOLUTIONS[0], steps=64, n_rays=256, seed=0):
    import pagnerf_amd
    torch.manual_seed(seed)
    nef = H.make_nef(device=dev, weights=H.make_weights(density_scale=8.0), blas_level=4)
    tracer = pagnerf_amd.PanopticPackedRFTracer(raymarch_type="ray", num_steps=steps, bg_color="white")
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(n_rays, 3, generator=g) * 0.6 - 0.3
    o[:, 2] = -1.6
    d = F.normalize(torch.stack([torch.rand(n_rays, generator=g) * 0.4 - 0.2, torch.rand(n_rays, generator=g) * 0.4 - 0.2, torch.ones(n_rays)], -1), dim=-1)
    rays = pagnerf_amd.Rays(o.to(dev), d.to(dev), 0.0, 6.0)
    target = torch.rand(n_rays, 3, generator=g).to(dev) * 0.5
    return nef, tracer, rays, target


def _optimizer(nef):
    from pagnerf_amd import optim
    grid = [p for n, p in nef.named_parameters() if n.startswith("grid.")]
    rest = [p for n, p in nef.named_parameters() if not n.startswith("grid.")]
    opt = optim.Adam([{"params": grid, "lr": 0.02}, {"params": rest, "lr": 0.001}], eps=1e-15)
    fallbacks = []
    real = opt._torch_step
    opt._torch_step = lambda ids: (fallbacks.append(list(ids)), real(ids))
    return opt, fallbacks


def _step(nef, tracer, rays, target, opt, **kw):
    opt.zero_grad(set_to_none=True)
    rb = tracer(nef, channels={"rgb"}, rays=rays, stage="train", **kw)
    loss = ((rb.rgb - target) ** 2).mean()
    loss.backward()
    opt.step()
    return float(loss.detach())


def test_training_through_the_tracer_prune_and_upsample(gpu_device):
    """Eager training traces through PanopticPackedRFTracer with pagnerf_amd.optim.Adam on its kernel path for every group (no torch fallback):
    the loss falls; then prune() and a voxel-march step; then step_upsample_vm_grid(), a new optimiser and a step at the new resolution."""
    from pagnerf_amd.graphs import GraphRunner
    nef, tracer, rays, target = _train_setup(gpu_device)
    assert not GraphRunner.eligible(tracer, nef, {"rgb"}, set(), rays, "train")
    opt, fallbacks = _optimizer(nef)
    losses = [_step(nef, tracer, rays, target, opt) for _ in range(12)]
    print("losses", ["%.5f" % v for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert not fallbacks and all(opt._plans[gi].ok for gi in range(2))
    for n, p in nef.named_parameters():
        if n.startswith(("grid.", "decoder_color.")):
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    # prune, then a voxel-march step
    nef.prune()
    kept = int(nef.grid.occupancy_mask().sum())
    assert 0 < kept < nef.grid.num_cells, kept
    after = _step(nef, tracer, rays, target, opt, raymarch_type="voxel", num_steps=4)
    assert np.isfinite(after) and not fallbacks
    # upsample: the table parameters are new objects, so the optimiser is created again (pc_nerf/trainer.py:348-358)
    old = nef.grid.features.app_plane[0]
    nef.grid.step_upsample_vm_grid()
    assert nef.grid.current_resolution == H.RESOLUTIONS[1] and nef.grid.features.app_plane[0] is not old
    opt, fallbacks = _optimizer(nef)
    l0 = _step(nef, tracer, rays, target, opt)
    l1 = _step(nef, tracer, rays, target, opt)
    assert np.isfinite(l0) and np.isfinite(l1) and not fallbacks and all(opt._plans[gi].ok for gi in range(2))
    assert nef.grid.features.app_plane[0].grad.shape == (H.RESOLUTIONS[1], H.RESOLUTIONS[1], H.AC)


def test_one_step_with_all_channels_and_the_linear_assignment_loss(gpu_device):
    """rgb + semantics + inst_embedding in one trace, LinAssignmentThingsLoss on the composited instance probabilities: finite, non-zero gradients on
    every parameter group."""
    from pagnerf_amd.loss import LinAssignmentThingsLoss
    nef, tracer, rays, target = _train_setup(gpu_device, n_rays=256)
    rb = tracer(nef, channels={"rgb", "semantics", "inst_embedding"}, rays=rays, stage="train")
    assert rb.semantics.shape == (256, H.CLASSES) and rb.inst_embedding.shape == (256, H.INSTANCES)
    g = torch.Generator().manual_seed(4)
    sem_gt = torch.randint(0, H.CLASSES, (256,), generator=g).to(gpu_device)
    inst_gt = torch.randint(0, 5, (2, 128), generator=g).to(gpu_device)
    stuff = inst_gt == 0
    loss_inst = LinAssignmentThingsLoss()(rb.inst_embedding.reshape(2, 128, H.INSTANCES), inst_gt, stuff).mean()
    loss = ((rb.rgb - target) ** 2).mean() + F.nll_loss(torch.log(rb.semantics + 1e-8), sem_gt) + loss_inst
    assert torch.isfinite(loss)
    loss.backward()
    groups = {"grid.features.density": 0.0, "grid.features.app": 0.0, "grid.features.basis_mat": 0.0, "decoder_color": 0.0, "decoder_semantics": 0.0,
              "decoder_inst": 0.0}
    for n, p in nef.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        for k in groups:
            if n.startswith(k):
                groups[k] += float(p.grad.abs().sum())
    assert all(v > 0 for v in groups.values()), groups
