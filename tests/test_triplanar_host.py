"""TriplanarGridHIP, host side (no GPU): the tensor-op form against an independent NumPy restatement of the per-axis pixel form,
column order, feat_scale, 'sum', the flat level offsets, the reference-layout state_dict, deepcopy / pickling, and the nef wiring."""
import copy
import itertools

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401


def _axis(c, R):
    """The explicit per-axis pixel form: (i0, w0, w1) in fp64."""
    p = ((c + 1.0) / 2.0) * (R - 1)
    a = np.abs(p)
    k = np.floor(a / (R - 1))
    e = a - k * (R - 1)
    q = np.where(k % 2 == 0, e, (R - 1) - e)
    q = np.clip(q, 0.0, R - 1)
    i0 = np.floor(q)
    return i0.astype(np.int64), (i0 + 1.0) - q, q - i0


def _plane(table, a, b, R):
    """table [F,R,R] (rows = second coordinate, columns = first), taps nw, ne, sw, se; the tap at index R is skipped."""
    x0, wx0, wx1 = _axis(a, R)
    y0, wy0, wy1 = _axis(b, R)
    out = np.zeros((a.shape[0], table.shape[0]))
    for dy, dx, w in ((0, 0, wx0 * wy0), (0, 1, wx1 * wy0), (1, 0, wx0 * wy1), (1, 1, wx1 * wy1)):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi < R) & (yi < R)
        vals = table[:, np.minimum(yi, R - 1), np.minimum(xi, R - 1)].T
        out += np.where(ok[:, None], vals * w[:, None], 0.0)
    return out


def numpy_triplanar(planes, xyz, feat_scale=None):
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    cols = []
    for fmx, fmy, fmz in planes:
        R = fmx.shape[-1]
        cols.append(_plane(fmx[0], y, z, R) + _plane(fmy[0], x, z, R) + _plane(fmz[0], x, y, R))
    out = np.concatenate(cols, axis=1)
    return out if feat_scale is None else out * feat_scale[None, :]


def _coords():
    rs = np.random.RandomState(5)
    pts = [rs.uniform(-1.3, 1.3, size=(2000, 3))]
    pts.append(np.array(list(itertools.product((-1.0, 1.0), repeat=3))))                       # the eight corners
    faces = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            c = np.zeros(3)
            c[ax] = sgn
            faces.append(c)
    pts.append(np.array(faces))                                                                 # the face centres
    pts.append(np.array([[1.25, -1.25, 0.999999], [-1.25, 0.999999, 1.25], [0.999999, 1.25, -1.25], [0.999999, 0.999999, 0.999999]]))
    return np.concatenate(pts)


def _grid(**kw):
    from pagnerf_amd import TriplanarGridHIP
    torch.manual_seed(3)
    args = dict(feature_dim=4, base_lod=1, num_lods=2, feature_std=1.0, feature_bias=0.25, blas_level=3)
    args.update(kw)
    return TriplanarGridHIP(**args)


def test_tensor_op_form_matches_numpy_pixel_form_fp64():
    g = _grid().double()
    assert g.resolutions == [3, 5] and g.active_lods == [1, 2] and g.half_coords is False and g.rounds_coords() is False
    xyz = _coords()
    planes = [[t.detach().numpy() for t in level] for level in g.planes()]
    with torch.no_grad():
        got = g.tensor_forward(torch.from_numpy(xyz)).numpy()
    want = numpy_triplanar(planes, xyz)
    assert got.shape == (xyz.shape[0], 8)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # feat_scale per column, through interpolate_scaled (the contract nef._interp relies on)
    fs = np.linspace(0.5, 2.0, 8)
    with torch.no_grad():
        got = g.interpolate_scaled(torch.from_numpy(xyz)[:, None], torch.from_numpy(fs), out_dtype=torch.float64).numpy()
    np.testing.assert_allclose(got, numpy_triplanar(planes, xyz, fs), rtol=0, atol=1e-12)


def test_column_order_sum_and_empty_input():
    g = _grid().double()
    xyz = torch.from_numpy(_coords()[:50])
    with torch.no_grad():
        cat = g.interpolate(xyz[:, None])
        assert cat.shape == (50, 1, 8)
        for l in range(2):                                       # columns l*F .. l*F + F - 1 come from level l alone
            h = copy.deepcopy(g)
            for m, lev in enumerate(h.planes()):
                if m != l:
                    for t in lev:
                        t.zero_()
            only = h.interpolate(xyz[:, None])
            assert torch.equal(only[..., l * 4:(l + 1) * 4], cat[..., l * 4:(l + 1) * 4])
            assert float(only[..., (1 - l) * 4:(2 - l) * 4].abs().max()) == 0.0
        g.multiscale_type = "sum"
        s = g.interpolate(xyz[:, None])
        assert s.shape == (50, 1, 4)
        np.testing.assert_allclose(s.numpy(), (cat[..., :4] + cat[..., 4:]).numpy(), rtol=0, atol=1e-14)
        assert g.interpolate(torch.zeros(0, 1, 3, dtype=torch.float64)).shape == (0, 1, 4)
        g.multiscale_type = "cat"
        assert g.interpolate(torch.zeros(0, 1, 3, dtype=torch.float64)).shape == (0, 1, 8)
    with pytest.raises(NotImplementedError):
        g.interpolate_scaled(xyz[:, None], layout="xcd8")


def test_flat_offsets_and_channel_last_layout():
    g = _grid(base_lod=1, num_lods=3, feature_dim=2)
    assert g._spec.res == [3, 5, 9] and g._spec.offsets == [0, 3 * 9 * 2, 3 * 9 * 2 + 3 * 25 * 2] and g.tables.shape == (3 * (9 + 25 + 81) * 2,)
    flat = g.tables.detach()
    for (off, R), level in zip(zip(g._spec.offsets, g._spec.res), g.planes(flat)):
        for p, t in enumerate(level):
            assert t.shape == (1, 2, R, R)
            for f, row, col in ((0, 0, 0), (1, R - 1, 1), (1, 1, R - 1)):
                assert float(t[0, f, row, col]) == float(flat[off + ((p * R + row) * R + col) * 2 + f])
    # feature_std / feature_bias
    h = _grid(feature_std=0.0, feature_bias=0.5)
    assert float(h.tables.min()) == float(h.tables.max()) == 0.5


def test_state_dict_roundtrip_deepcopy_and_pickle(tmp_path):
    g = _grid()
    sd = g.state_dict()
    want = {"features.%d.%s" % (i, n) for i in range(2) for n in ("fmx", "fmy", "fmz")} | {"blas_bits"}
    assert set(sd) == want and sd["features.0.fmx"].shape == (1, 4, 3, 3) and sd["features.1.fmz"].shape == (1, 4, 5, 5)
    assert sd["features.1.fmy"].is_contiguous()
    torch.manual_seed(99)
    h = _grid()
    h.tables.data.normal_()
    res = h.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys and torch.equal(h.tables, g.tables)
    xyz = torch.from_numpy(_coords()[:64]).float()
    with torch.no_grad():
        assert torch.equal(h.interpolate(xyz[:, None]), g.interpolate(xyz[:, None]))
    # the flat form loads too; a wrong shape is refused
    h.tables.data.zero_()
    h.load_state_dict({"tables": g.tables.detach().clone(), "blas_bits": g.blas_bits})
    assert torch.equal(h.tables, g.tables)
    bad = dict(sd)
    bad["features.0.fmx"] = torch.zeros(1, 4, 4, 4)
    with pytest.raises(RuntimeError):
        h.load_state_dict(bad)
    # deepcopy (the delta grid is one) keeps working hooks and its own storage
    d = copy.deepcopy(g)
    assert d.tables.data_ptr() != g.tables.data_ptr() and set(d.state_dict()) == want
    d.tables.data.zero_()
    d.load_state_dict(sd)
    assert torch.equal(d.tables, g.tables)
    # torch.save / torch.load of the module: the spec is plain numbers and is bound again
    path = tmp_path / "grid.pth"
    torch.save(g, path)
    back = torch.load(path, weights_only=False)
    assert back._spec.res == [3, 5] and back._spec.offsets == g._spec.offsets and list(back._spec.res_c) == [3, 5]
    with torch.no_grad():
        assert torch.equal(back.interpolate(xyz[:, None]), g.interpolate(xyz[:, None]))


def test_nef_builds_with_triplanar_grid():
    """Fails before this grid existed: KeyError('TriplanarGrid') in the nef's constructor."""
    import pagnerf_amd
    kw = dict(feature_dim=4, base_lod=2, num_lods=4, feature_std=0.01, num_classes=6, num_instances=8, blas_level=3, some_cli_flag=1)
    nef = pagnerf_amd.PanopticNeF(grid_type="TriplanarGrid", **kw)
    assert isinstance(nef.grid, pagnerf_amd.TriplanarGridHIP) and nef.grid.resolutions == [5, 9, 17, 33]
    assert nef.decoder_density.input_dim == 16 and nef.decoder_semantics.input_dim == 16 and nef.decoder_inst.input_dim == 16
    assert nef._grouped() is None and not nef.can_fuse_panoptic({"semantics"})
    assert not hasattr(nef, "delta_grid")
    delta = pagnerf_amd.PanopticDeltaNeF(grid_type="TriplanarGridHIP", panoptic_features_type="delta", **kw)
    assert delta.delta_grid.tables.shape == delta.grid.tables.shape and delta.delta_grid.tables.data_ptr() != delta.grid.tables.data_ptr()
    assert any(n == "grid.tables" for n, _ in delta.named_parameters()) and any(n == "delta_grid.tables" for n, _ in delta.named_parameters())
    ms = pagnerf_amd.MeanShiftPanopticNeF(grid_type="TriplanarGrid", **kw)
    assert ms.decoder_inst.input_dim == 16
    s = pagnerf_amd.PanopticNeF(grid_type="TriplanarGrid", multiscale_type="sum", **dict(kw, num_lods=3))
    assert s.decoder_density.input_dim == 4
    with pytest.raises(ValueError, match="multiple of 8"):
        pagnerf_amd.PanopticNeF(grid_type="TriplanarGrid", **dict(kw, num_lods=3))
    # the other grids keep the grouped layout
    p = pagnerf_amd.PanopticDeltaNeF(grid_type="PermutoGrid", feature_dim=2, num_lods=24, num_classes=6, num_instances=8, capacity_log_2=6, blas_level=3)
    assert p._grouped() == (24, 2)


def test_checkpoint_roundtrip_through_reference_names():
    import pagnerf_amd
    from pagnerf_amd import checkpoint
    kw = dict(grid_type="TriplanarGrid", feature_dim=4, base_lod=1, num_lods=2, feature_std=0.1, num_classes=6, num_instances=8, blas_level=3,
              panoptic_features_type="delta")
    torch.manual_seed(0)
    a = pagnerf_amd.Pipeline(pagnerf_amd.PanopticDeltaNeF(**kw), pagnerf_amd.PanopticPackedRFTracer(num_steps=8))
    a.nef.grid.blas_init(torch.rand(512) > 0.5)
    sd = checkpoint.save_reference_state_dict(a)
    assert sd["nef.grid.features.1.fmy"].shape == (1, 4, 5, 5) and "nef.delta_grid.features.0.fmz" in sd
    torch.manual_seed(1)
    b = pagnerf_amd.Pipeline(pagnerf_amd.PanopticDeltaNeF(**kw), pagnerf_amd.PanopticPackedRFTracer(num_steps=8))
    assert not torch.equal(a.nef.grid.tables, b.nef.grid.tables)
    unused = checkpoint.load_reference_state_dict(b, sd)
    assert not [k for k in unused if "features" in k or "decoder" in k]
    assert torch.equal(a.nef.grid.tables, b.nef.grid.tables) and torch.equal(a.nef.delta_grid.tables, b.nef.delta_grid.tables)
    assert torch.equal(a.nef.grid.occupancy_mask(), b.nef.grid.occupancy_mask())
