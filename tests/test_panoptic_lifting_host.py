"""PanopticLiftingNeF on the CPU (the fp32 tensor-op path) against the reference's golden (g16_panoptic_lifting.npz,
tests/golden/make_golden_panoptic_lifting.py), its host logic, and the argument validation of the pag_vm_* entry points.  No GPU.

The upper part of this file is shared with the fixture's maker and with tests/test_gpu_panoptic_lifting.py: the sizes, the seeded weights (they are
not stored; drawn in the REFERENCE's layout, [1,C,R,R] planes and [1,C,R,1] lines), the inputs, the upstream gradients, and a numpy restatement of
the vector-matrix density."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden

RES, RESOLUTIONS, BLAS = 16, [16, 19, 22, 25, 28], 3           # an odd step: the upsampled grid is no multiple of the base
DC, AC, APP = 16, 48, 27
CLASSES, INSTANCES, HEAD_HIDDEN, HEAD_LAYERS = 7, 16, 32, 3
N_GOLD = 2048
SEED = 2203
CHANNELS = ("density", "rgb", "semantics", "inst_embedding")
N_RAYS, RAY_LEN = 8, 128                                       # the block of consecutive samples along rays
ZERO_EPS = 1e-4                                                # |sigma_feature| below this: the density's upstream gradient is zeroed (relu' jumps there)

NEF_KW = dict(num_classes=CLASSES, num_instances=INSTANCES, sem_num_layers=HEAD_LAYERS, sem_hidden_dim=HEAD_HIDDEN, inst_num_layers=HEAD_LAYERS,
              inst_hidden_dim=HEAD_HIDDEN, sem_softmax=True, inst_softmax=True)
GRID_KW = dict(density_n_comp=DC, color_n_comp=AC, base_resolution=RESOLUTIONS[0], max_resolution=RESOLUTIONS[-1], num_resolution=len(RESOLUTIONS),
               blas_level=BLAS)


def param_shapes(res=RES, classes=CLASSES, instances=INSTANCES, hidden=HEAD_HIDDEN, layers=HEAD_LAYERS):
    """name -> shape in the reference's layout, in the order of the reference's named_parameters()."""
    s = {}
    for name, C in (("density", DC), ("app", AC)):
        for i in range(3):
            s["grid.features.%s_plane.%d" % (name, i)] = (1, C, res, res)
        for i in range(3):
            s["grid.features.%s_line.%d" % (name, i)] = (1, C, res, 1)
    s["grid.features.basis_mat.weight"] = (APP, 3 * AC)
    for i, (n_out, n_in) in zip((0, 2, 4), ((128, 150), (128, 128), (3, 128))):
        s["decoder_color.mlp.%d.weight" % i], s["decoder_color.mlp.%d.bias" % i] = (n_out, n_in), (n_out,)
    for head, n_out in (("decoder_semantics", classes), ("decoder_inst", instances)):
        for i in range(layers - 1):
            s["%s.layers.%d.weight" % (head, i)], s["%s.layers.%d.bias" % (head, i)] = (hidden, 3 if i == 0 else hidden), (hidden,)
        s["%s.lout.weight" % head], s["%s.lout.bias" % head] = (n_out, hidden), (n_out,)
    return s


def make_weights(seed=SEED, res=RES, density_scale=1.0, **kw):
    """Tables 0.1 * N(0,1) (the reference's initialisation), basis uniform in +- 1/12 (nn.Linear's), He-normal decoder weights with small uniform
    biases (nn.Linear's default leaves the heads' logits nearly constant, which exercises nothing)."""
    rs = np.random.RandomState(seed)
    w = {}
    for name, shape in param_shapes(res, **kw).items():
        if "features" in name and name.endswith("weight"):
            w[name] = rs.uniform(-1.0 / 12, 1.0 / 12, size=shape).astype(np.float32)
        elif "features" in name:
            w[name] = (0.1 * (density_scale if "density" in name else 1.0) * rs.standard_normal(shape)).astype(np.float32)
        elif name.endswith("weight"):
            w[name] = (rs.standard_normal(shape) * np.sqrt((1.0 if ".lout" in name or "mlp.4" in name else 2.0) / shape[1])).astype(np.float32)
        else:
            w[name] = rs.uniform(-0.1, 0.1, size=shape).astype(np.float32)
    return w


def make_inputs(seed=SEED, n=N_GOLD, res=RES):
    """-> coords [n,3], dirs [n,3].  In order: the 8 corners; 64 points up to 1e-4 outside the cube; 128 points on integer pixel coordinates;
    N_RAYS x RAY_LEN consecutive samples along rays (step 2 sqrt(3) / 512, the configuration's); uniform points."""
    rs = np.random.RandomState(seed + 1)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float32)
    outside = rs.uniform(-1, 1, size=(64, 3)).astype(np.float32)
    axis, sign = rs.randint(0, 3, size=64), rs.choice([-1.0, 1.0], size=64)
    outside[np.arange(64), axis] = (sign * (1.0 + rs.uniform(0, 1e-4, size=64))).astype(np.float32)
    outside[:8, :] = np.sign(outside[:8, :]) * np.float32(1.0 + 1e-4)                      # outside along all three axes
    pixels = (rs.randint(0, res, size=(128, 3)).astype(np.float32) / np.float32(res - 1) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    o = rs.uniform(-0.9, -0.6, size=(N_RAYS, 3)).astype(np.float32)
    d = rs.uniform(0.1, 1.0, size=(N_RAYS, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = (np.arange(RAY_LEN, dtype=np.float32) + 0.5) * np.float32(2 * np.sqrt(3) / 512)
    rays = (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 3).astype(np.float32)
    assert np.abs(rays).max() < 1.0
    rest = rs.uniform(-1, 1, size=(n - 8 - 64 - 128 - N_RAYS * RAY_LEN, 3)).astype(np.float32)
    x = np.concatenate([corners, outside, pixels, rays, rest]).astype(np.float32)
    v = rs.standard_normal((n, 3)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return x, v.astype(np.float32)


RAY0 = 8 + 64 + 128                                            # first sample of the ray block


def make_upstream(seed=SEED, n=N_GOLD, classes=CLASSES, instances=INSTANCES):
    """Seeded upstream gradients.  The second half of every ray of the ray block gets exactly zero density and rgb gradients (a sample the grid's
    backward must skip); the first 100 uniform points get a zero rgb gradient only, the next 100 a zero density gradient only."""
    rs = np.random.RandomState(seed + 2)
    up = {"density": rs.standard_normal((n, 1, 1)).astype(np.float32), "rgb": rs.standard_normal((n, 3)).astype(np.float32),
          "semantics": rs.standard_normal((n, 1, classes)).astype(np.float32), "inst_embedding": rs.standard_normal((n, 1, instances)).astype(np.float32)}
    for r in range(N_RAYS):
        a = RAY0 + r * RAY_LEN + RAY_LEN // 2
        up["density"][a:a + RAY_LEN // 2] = 0.0
        up["rgb"][a:a + RAY_LEN // 2] = 0.0
    u0 = RAY0 + N_RAYS * RAY_LEN
    up["rgb"][u0:u0 + 100] = 0.0
    up["density"][u0 + 100:u0 + 200] = 0.0
    return up


def reference_state_dict(w):
    return {k: torch.from_numpy(v) for k, v in w.items()}


def load_weights(nef, w):
    """Through load_state_dict of a dict in the reference's layout (strict=False: the occupancy buffers are not part of it)."""
    res = nef.load_state_dict(reference_state_dict(w), strict=False)
    assert not res.unexpected_keys and all("blas" in k for k in res.missing_keys), res


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def np_bilinear(table, px, py):
    """table [C,H,W], pixel coordinates px (W), py (H) [M] -> [C,M]: zero padding."""
    C, H, W = table.shape
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    out = np.zeros((C, px.shape[0]), dtype=np.float32)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wx = (px - x0) if dx else (x0 + 1 - px)
            wy = (py - y0) if dy else (y0 + 1 - py)
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            v = table[:, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]
            out += np.where(ok, (wx * wy).astype(np.float32), np.float32(0.0)) * v
    return out


def np_vm_products(w, xyz, name):
    """The three [C,M] plane x line products of the set `name` ('density' / 'app') from reference-layout weights."""
    R = w["grid.features.%s_plane.0" % name].shape[-1]
    pix = ((xyz.astype(np.float32) + np.float32(1.0)) / np.float32(2.0) * np.float32(R - 1)).astype(np.float32)
    out = []
    for i, ((a, b), l) in enumerate(zip(((0, 1), (0, 2), (1, 2)), (2, 1, 0))):
        plane = np_bilinear(w["grid.features.%s_plane.%d" % (name, i)][0], pix[:, a], pix[:, b])
        line = np_bilinear(w["grid.features.%s_line.%d" % (name, i)][0], np.zeros_like(pix[:, l]), pix[:, l])
        out.append(plane * line)
    return out


def np_vm_sigma(w, xyz):
    return sum(p.sum(0) for p in np_vm_products(w, xyz, "density")).astype(np.float32)


def np_vm_app(w, xyz):
    return (np.concatenate(np_vm_products(w, xyz, "app"), 0).T.astype(np.float64) @ w["grid.features.basis_mat.weight"].T.astype(np.float64)).astype(np.float32)


def make_nef(seed=SEED, device=None, weights=None, **kw):
    import pagnerf_amd
    args = dict(NEF_KW)
    args.update(GRID_KW)
    args.update(kw)
    nef = pagnerf_amd.PanopticLiftingNeF(**args)
    load_weights(nef, weights if weights is not None else make_weights(seed))
    return nef.to(device) if device is not None else nef


def reference_grads(nef):
    """name -> gradient in the reference's layout."""
    from pagnerf_amd import panoptic_lifting as PL
    out = {}
    for n, p in nef.named_parameters():
        g = p.grad
        if "_plane." in n:
            g = PL.plane_to_reference(g)
        elif "_line." in n:
            g = PL.line_to_reference(g)
        out[n] = g.detach().cpu().numpy()
    return out


def check_against_golden(g16, out, grads, factor=3.0):
    """Elementwise tolerances of the project (outputs rtol 1e-5 / atol 2e-6, gradients rtol 2e-4 / atol 2e-5) and, per tensor, rel-L2 <= factor x the
    stored fp32-vs-fp64 floor of the reference + 1e-6.  Every figure is printed before the assertions."""
    failures = []
    for c in CHANNELS:
        assert tuple(out[c].shape) == tuple(g16[c].shape), c
        d, floor = rel_l2(out[c], g16[c]), float(g16["floor_" + c])
        print("output %-16s rel-L2 %.3e floor %.3e max|diff| %.3e" % (c, d, floor, np.abs(out[c] - g16[c]).max()))
        if d > factor * floor + 1e-6 or not np.allclose(out[c], g16[c], rtol=1e-5, atol=2e-6):
            failures.append(c)
    floors = dict(zip([str(n) for n in g16["grad_names"]], g16["grad_floors"]))
    for n in floors:
        want = g16["grad_" + n]
        d = rel_l2(grads[n], want)
        print("grad   %-40s rel-L2 %.3e floor %.3e max|diff| %.3e" % (n, d, floors[n], np.abs(grads[n] - want).max()))
        if d > factor * floors[n] + 1e-6 or not np.allclose(grads[n], want, rtol=2e-4, atol=2e-5):
            failures.append(n)
    assert not failures, failures


def run_with_upstream(nef, g16, device="cpu", **fw):
    x, d = torch.from_numpy(g16["coords"]).to(device), torch.from_numpy(g16["dirs"]).to(device)
    nef.zero_grad()
    out = nef(channels=set(CHANNELS), coords=x[:, None], ray_d=d, **fw)
    loss = sum((out[c] * torch.from_numpy(g16["up_" + c]).to(device)).sum() for c in CHANNELS)
    loss.backward()
    return {c: out[c].detach().cpu().numpy() for c in CHANNELS}, reference_grads(nef)


# ------------------------------------------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def g16():
    return golden("g16_panoptic_lifting.npz")


def test_fixture_inputs_are_the_seeded_ones(g16):
    x, d = make_inputs()
    assert np.array_equal(g16["coords"], x) and np.array_equal(g16["dirs"], d)
    assert np.array_equal(np.abs(x[:8]), np.ones((8, 3), np.float32)) and (np.abs(x[8:72]).max(1) > 1.0).all() and np.abs(x).max() <= 1.0 + 1.0001e-4
    up = make_upstream()
    near = np.abs(g16["sigma_feature"]) < ZERO_EPS
    up["density"][near] = 0.0
    for c in CHANNELS:
        assert np.array_equal(g16["up_" + c], up[c]), c
    both = (g16["up_density"].reshape(-1) == 0) & (np.abs(g16["up_rgb"]).max(1) == 0)
    assert both.sum() >= N_RAYS * RAY_LEN // 2


def test_cpu_path_matches_reference_golden(g16):
    nef = make_nef()
    out, grads = run_with_upstream(nef, g16)
    check_against_golden(g16, out, grads)
    assert nef.grid.features.density_plane[0].grad.is_contiguous()


def test_numpy_restatement_matches_golden_grid(g16):
    w = make_weights()
    np.testing.assert_allclose(np_vm_sigma(w, g16["coords"]), g16["sigma_feature"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(np.maximum(np_vm_sigma(w, g16["coords"]), 0).reshape(-1, 1, 1), g16["density"], rtol=1e-5, atol=2e-6)
    nef = make_nef()
    with torch.no_grad():
        _, app = nef.grid.interpolate(torch.from_numpy(g16["coords"])[:, None], 0)
    np.testing.assert_allclose(app[:, 0].numpy(), np_vm_app(w, g16["coords"]), rtol=1e-5, atol=2e-6)


def test_parameter_names_and_shapes_are_the_references(g16):
    nef = make_nef()
    ref = list(zip([str(n) for n in g16["param_names"]], [tuple(int(v) for v in s if v >= 0) for s in g16["param_shapes"]]))
    assert ref == list(param_shapes().items())
    assert [n for n, _ in nef.named_parameters()] == [n for n, _ in ref]
    sd = nef.state_dict()
    assert [(k, tuple(sd[k].shape)) for k, _ in ref] == ref
    assert all(p.is_contiguous() and p.dtype == torch.float32 for p in nef.parameters())          # what optim.Adam's kernel path needs
    assert nef.get_supported_channels() == set(CHANNELS) and nef.get_nef_type() == "panoptic_nef"
    assert nef.grid.num_lods == 1 and nef.grid.active_lods == [0] and not getattr(nef, "accepts_ray_index", False)
    assert "num_resolutions" in vars(nef.grid) and nef.grid.resolutions == RESOLUTIONS and nef.grid.current_resolution == RES
    import pagnerf_amd
    full = pagnerf_amd.TensoRF(blas_level=2)
    assert full.resolutions == [128, 144, 160, 176, 192] and full.features.density_plane[0].shape == (128, 128, 16)
    assert float(type(nef.decoder_color)(27).mlp[4].bias.detach().abs().max()) == 0.0 and nef.decoder_color.in_feat_mlp == 150


def test_state_dict_round_trip_through_the_reference_layout():
    w = make_weights()
    nef = make_nef()
    sd = nef.state_dict()
    for k, v in w.items():
        assert torch.equal(sd[k], torch.from_numpy(v)), k
    other = make_nef(seed=SEED + 1)
    other.load_state_dict(sd)
    for (n, a), (_, b) in zip(nef.named_parameters(), other.named_parameters()):
        assert torch.equal(a, b) and b.is_contiguous(), n
    # stored layout: channel-last
    assert torch.equal(nef.grid.features.app_plane[1][3, 5, :], torch.from_numpy(w["grid.features.app_plane.1"][0, :, 3, 5]))
    assert torch.equal(nef.grid.features.density_line[2][7, :], torch.from_numpy(w["grid.features.density_line.2"][0, :, 7, 0]))


def test_channel_selective_forward_return_types():
    nef = make_nef()
    x, d = torch.rand(7, 1, 3) * 2 - 1, F.normalize(torch.randn(7, 3), dim=-1)
    with torch.no_grad():
        dens = nef(channels="density", coords=x, ray_d=d)
        lst = nef(channels=["semantics", "density"], coords=x, ray_d=d)
        dct = nef(channels={"rgb", "inst_embedding"}, coords=x, ray_d=d, pidx=None, lod_idx=0)
    assert isinstance(dens, torch.Tensor) and dens.shape == (7, 1, 1)
    assert isinstance(lst, list) and lst[0].shape == (7, 1, CLASSES) and torch.equal(lst[1], dens)
    assert isinstance(dct, dict) and set(dct) == {"rgb", "inst_embedding"} and dct["rgb"].shape == (7, 3) and dct["inst_embedding"].shape == (7, 1, INSTANCES)
    assert torch.allclose(lst[0].sum(-1), torch.ones(7, 1), atol=1e-5) and torch.allclose(dct["inst_embedding"].sum(-1), torch.ones(7, 1), atol=1e-5)
    with pytest.raises(Exception, match="not supported"):
        nef(channels={"delta"}, coords=x, ray_d=d)
    with pytest.raises(ValueError, match="ray_d of shape"):
        nef(channels="rgb", coords=x, ray_d=d[:3])
    # [batch, num_samples > 1]: flattened to batch * num_samples samples, one direction per batch entry repeated over its samples
    xs = torch.rand(3, 4, 3) * 2 - 1
    with torch.no_grad():
        a = nef(channels=set(CHANNELS), coords=xs, ray_d=d[:3])
        b = nef(channels=set(CHANNELS), coords=xs.reshape(12, 1, 3), ray_d=d[:3].repeat_interleave(4, 0))
    assert a["density"].shape == (3, 4, 1) and a["rgb"].shape == (12, 3) and a["semantics"].shape == (3, 4, CLASSES)
    assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["density"].reshape(12, 1, 1), b["density"])
    assert torch.allclose(a["semantics"].reshape(12, 1, CLASSES), b["semantics"], atol=1e-6)


def test_post_activations_and_the_instance_heads_activation_quirk():
    """sigmoid / normalize / softmax are applied in that order, and the instance head runs with the SEMANTIC head's activation."""
    x = torch.rand(9, 1, 3) * 2 - 1
    plain = make_nef(sem_softmax=False, inst_softmax=False)
    both = make_nef(sem_sigmoid=True, sem_normalize=True, sem_softmax=True, inst_softmax=False, inst_normalize=True)
    with torch.no_grad():
        raw_s, raw_i = plain(channels=["semantics", "inst_embedding"], coords=x)
        s, i = both(channels=["semantics", "inst_embedding"], coords=x)
    assert torch.allclose(s, F.softmax(F.normalize(torch.sigmoid(raw_s), dim=-1), dim=-1), atol=1e-6)
    assert torch.allclose(i, F.normalize(raw_i, dim=-1), atol=1e-6)
    sin = make_nef(sem_activation_type="sin", sem_softmax=False, inst_softmax=False)
    with torch.no_grad():
        got = sin(channels="inst_embedding", coords=x)
        h = x
        for l in sin.decoder_inst.layers:
            h = torch.sin(l(h))
    assert torch.equal(got, sin.decoder_inst.lout(h))


def test_coords_gradient_comes_from_the_heads_only():
    """The grid detaches its coordinates: density and the appearance feature give no gradient for coords; the heads and the view direction do."""
    nef = make_nef()
    x = (torch.rand(6, 1, 3) * 2 - 1).requires_grad_(True)
    d = F.normalize(torch.randn(6, 3), dim=-1).requires_grad_(True)
    out = nef(channels=set(CHANNELS), coords=x, ray_d=d)
    gx, gd = torch.autograd.grad(out["density"].sum() + out["rgb"].sum(), (x, d), retain_graph=True, allow_unused=True)
    assert gx is None and gd is not None and gd.abs().sum() > 0
    gx2, = torch.autograd.grad((out["semantics"] ** 2).sum(), x)
    assert gx2.abs().sum() > 0


def test_upsampling_matches_the_reference_and_replaces_the_parameters(g16):
    nef = make_nef()
    before = {n: p for n, p in nef.named_parameters()}
    nef.grid.step_upsample_vm_grid()
    assert nef.grid.current_resolution == RESOLUTIONS[1] == nef.grid.features.res
    sd = nef.state_dict()
    np.testing.assert_allclose(sd["grid.features.density_plane.0"].numpy(), g16["upsampled_density_plane_0"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(sd["grid.features.app_line.1"].numpy(), g16["upsampled_app_line_1"], rtol=1e-5, atol=2e-6)
    after = {n: p for n, p in nef.named_parameters()}
    assert list(after) == list(before)
    for n in after:
        assert (after[n] is not before[n]) == ("_plane." in n or "_line." in n), n
        assert after[n].requires_grad and after[n].is_contiguous()
    for _ in range(6):
        nef.grid.step_upsample_vm_grid()
    assert nef.grid.current_resolution == RESOLUTIONS[-1] and nef.grid.features.app_plane[2].shape == (28, 28, AC)
    nef.grid.upsample_vm_grid(31)
    assert nef.grid.current_resolution == 31
    with torch.no_grad():
        assert nef(channels="density", coords=torch.zeros(2, 1, 3)).shape == (2, 1, 1)
    nef.grid.freeze()
    assert not any(p.requires_grad for p in nef.grid.features.parameters())


def test_prune_matches_numpy_restatement():
    w = make_weights(density_scale=8.0)
    nef = make_nef(weights=w)
    R = 2 ** BLAS
    rs = np.random.RandomState(3)
    jitter = rs.uniform(0, 1, size=(R ** 3, 3)).astype(np.float32)
    occ0 = rs.uniform(0, 8, size=R ** 3).astype(np.float32)
    nef.grid.occupancy = torch.from_numpy(occ0.copy())
    nef.prune(jitter=torch.from_numpy(jitter))
    ar = np.arange(R)
    pts = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    samples = ((pts + jitter) / np.float32(R) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    dens = np.maximum(np_vm_sigma(w, samples), 0)
    assert (dens > 3).mean() > 0.02                      # the scaled density tables put part of the cells above the threshold on their own
    want = np.maximum(dens, occ0 * np.float32(0.6))
    np.testing.assert_allclose(nef.grid.occupancy.numpy(), want, rtol=1e-5, atol=2e-6)
    thr = (0.01 * 512) / np.sqrt(3)
    clear = np.abs(want - thr) > 1e-4
    mask = nef.grid.occupancy_mask().numpy()
    assert np.array_equal(mask[clear], (want > thr)[clear]) and 0 < mask.sum() < mask.size


def test_trace_through_the_tracer_on_cpu():
    """The tracer's shade() drives the nef the way a training trace does (per-sample ray_d, channels as a set, the two panoptic channels through
    composite_feats); the GPU-only compositing ops are replaced by the tensor-op stand-ins of test_semantic_nef_host."""
    from test_semantic_nef_host import cpu_trace, make_rays
    nef = make_nef(weights=make_weights(density_scale=8.0))
    o, d = make_rays()
    out = cpu_trace(nef, o, d, 16, channels=("rgb", "depth", "semantics", "inst_embedding"))
    assert out["rgb"].shape == (24, 3) and out["depth"].shape == (24, 1) and out["semantics"].shape == (24, CLASSES)
    assert out["inst_embedding"].shape == (24, INSTANCES) and out["alpha"].shape == (24, 1)
    assert torch.isfinite(out["rgb"]).all() and float(out["alpha"].max()) > 0
    (out["rgb"].sum() + (out["semantics"] ** 2).sum() + (out["inst_embedding"] ** 2).sum()).backward()
    f = nef.grid.features
    for p in (f.density_plane[0], f.density_line[1], f.app_plane[2], f.app_line[0], f.basis_mat.weight, nef.decoder_color.mlp[0].weight,
              nef.decoder_semantics.lout.weight, nef.decoder_inst.layers[0].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0


def test_precision_default_and_bf16_is_a_gpu_only_switch():
    nef = make_nef()
    assert nef.precision == "fp32"
    x, d = torch.rand(5, 1, 3) * 2 - 1, F.normalize(torch.randn(5, 3), dim=-1)
    with torch.no_grad():
        a = nef(channels=set(CHANNELS), coords=x, ray_d=d)
        nef.set_precision("bf16")                       # CPU tensors: still the fp32 tensor ops
        b = nef(channels=set(CHANNELS), coords=x, ray_d=d)
    assert all(torch.equal(a[c], b[c]) for c in CHANNELS)
    with pytest.raises(AssertionError):
        nef.set_precision("fp16")


def _args(L, res=RES):
    a = L.VmArgs()
    a.density_n_comp, a.app_n_comp, a.app_dim, a.res = DC, AC, APP, res
    return a


def test_vm_entry_points_validate_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from pagnerf_amd import _lib as L
    lib = L.load()
    assert lib.pag_vm_supported(16, 48, 27, 128) == 1 and lib.pag_vm_supported(16, 48, 27, 2) == 1 and lib.pag_vm_supported(16, 48, 27, 2048) == 1
    for bad in ((8, 48, 27, 128), (16, 32, 27, 128), (16, 48, 3, 128), (16, 48, 27, 1), (16, 48, 27, 2049), (16, 48, 27, -5)):
        assert lib.pag_vm_supported(*bad) == 0, bad
    assert lib.pag_vm_bwd_workspace_bytes(-1) == -1 and b"M" in lib.pag_last_error_string()
    assert lib.pag_vm_bwd_workspace_bytes(0) == 0 and lib.pag_vm_bwd_workspace_bytes(1) == 27 * 144 * 4
    assert lib.pag_vm_bwd_workspace_bytes(257) == 2 * 27 * 144 * 4 and lib.pag_vm_bwd_workspace_bytes(6291456) == 1024 * 27 * 144 * 4
    a = _args(L)
    assert lib.pag_vm_fwd(ctypes.byref(a), 0, None) == 0 and lib.pag_vm_bwd(ctypes.byref(a), 0, None) == 0             # M == 0: no-op
    assert lib.pag_vm_fwd(None, 4, None) == -1 and lib.pag_vm_bwd(None, 4, None) == -1
    assert lib.pag_vm_fwd(ctypes.byref(a), -1, None) == -1 and b"M" in lib.pag_last_error_string()
    assert lib.pag_vm_fwd(ctypes.byref(a), 4, None) == -1 and b"xyz" in lib.pag_last_error_string()
    buf = (ctypes.c_float * 64)()
    one = ctypes.cast(buf, ctypes.c_void_p).value          # a non-NULL value; every call below is refused before it is ever dereferenced
    a.xyz = one
    assert lib.pag_vm_fwd(ctypes.byref(a), 4, None) == -1 and b"sigma and app" in lib.pag_last_error_string()
    a.sigma = one
    assert lib.pag_vm_fwd(ctypes.byref(a), 4, None) == -1 and b"density table" in lib.pag_last_error_string()
    a.sigma, a.app = None, one
    assert lib.pag_vm_fwd(ctypes.byref(a), 4, None) == -1 and b"appearance table" in lib.pag_last_error_string()
    for i in range(3):
        a.app_plane[i] = a.app_line[i] = one
    assert lib.pag_vm_fwd(ctypes.byref(a), 4, None) == -1 and b"basis" in lib.pag_last_error_string()
    a.res = 1
    assert lib.pag_vm_fwd(ctypes.byref(a), 4, None) == -1 and b"unsupported" in lib.pag_last_error_string()
    a.res, a.app_n_comp = RES, 24
    assert lib.pag_vm_bwd(ctypes.byref(a), 4, None) == -1 and b"unsupported" in lib.pag_last_error_string()
    a.app_n_comp = AC
    assert lib.pag_vm_bwd(ctypes.byref(a), 4, None) == -1 and b"g_sigma and g_app" in lib.pag_last_error_string()
    a.g_sigma = one
    assert lib.pag_vm_bwd(ctypes.byref(a), 4, None) == -1 and b"density table" in lib.pag_last_error_string()
    a.g_sigma, a.g_app = None, one
    assert lib.pag_vm_bwd(ctypes.byref(a), 4, None) == -1 and b"appearance table / gradient" in lib.pag_last_error_string()
    for i in range(3):
        a.g_app_plane[i] = a.g_app_line[i] = one
    assert lib.pag_vm_bwd(ctypes.byref(a), 4, None) == -1 and b"basis" in lib.pag_last_error_string()
    a.basis = a.g_basis = one
    assert lib.pag_vm_bwd(ctypes.byref(a), 4, None) == -1 and b"workspace" in lib.pag_last_error_string()              # NULL workspace
    a.workspace, a.workspace_bytes = one, 64
    assert lib.pag_vm_bwd(ctypes.byref(a), 4, None) == -1 and b"workspace" in lib.pag_last_error_string()              # short workspace


def test_python_wrappers_refuse_cpu_tensors_and_wrong_layouts():
    """vm_forward / vm_backward are the GPU path: CPU tensors, reference-layout tables and non-f32 inputs are refused in front of the launch."""
    from pagnerf_amd import panoptic_lifting as PL
    nef = make_nef()
    f = nef.grid.features
    x = torch.zeros(4, 3)
    assert not f.kernel_supported(x)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        PL.vm_forward(f.tables(), f.basis_mat.weight, RES, x)
    ref_layout = ([PL.plane_to_reference(t).contiguous() for t in f.density_plane],) + f.tables()[1:]
    with pytest.raises(ValueError, match="table"):
        PL.vm_forward(ref_layout, f.basis_mat.weight, RES, x)
    with pytest.raises(ValueError, match="xyz"):
        PL.vm_forward(f.tables(), f.basis_mat.weight, RES, x.double())
    with pytest.raises(ValueError, match="upstream"):
        PL.vm_backward(f.tables(), f.basis_mat.weight, RES, x, torch.zeros(5), None)
