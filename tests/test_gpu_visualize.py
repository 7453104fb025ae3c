"""csrc/visualize.hip on the GPU: every picture of ValidationPictures.render, and every single-picture function, must be BIT-equal (torch.equal on
uint8 / int32) to the tensor-op forms of pagnerf_amd/visualize.py - the file is built without FMA contraction, nothing here has a tolerance.

Shapes: 1 x 1; 37 x 53 (1961 pixels: no multiple of a wave, of the 4 pixels a thread paints, or of 4 bytes per plane, so the planes after the first
are not dword-aligned and take the byte stores); 130 x 257 (33410 pixels: 33 paint workgroups, 17 statistics workgroups, odd row length).
The reference pictures of one (shape, dtype) case are computed once and shared."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (37, 53), (130, 257)]
DTYPES = [torch.int64, torch.int32, torch.uint8]
NAN, INF = float("nan"), float("inf")


def rect(lab, y0, y1, x0, x1, value):
    """value on the inclusive rectangle, clipped to the image."""
    H, W = lab.shape
    lab[max(0, y0):min(H, y1 + 1), max(0, x0):min(W, x1 + 1)] = value


def make_inputs(H, W, dtype, seed):
    """CPU inputs that take every branch: ids 0, -1, 1, 255, 256, 70000 (where the dtype holds them), a single-pixel box, boxes on all four borders, two
    overlapping boxes, depth with nan / +inf / -inf, confidences below 0 and above 1, colours below 0, above 1 and nan."""
    g = torch.Generator().manual_seed(seed)
    wide = dtype != torch.uint8

    def labels(kind):
        lab = torch.zeros(H, W, dtype=torch.int64)
        if kind == "sem":
            lab = torch.randint(0, 6, (H, W), generator=g)
            if wide:
                lab[torch.rand(H, W, generator=g) < 0.1] = -1
            return lab
        rect(lab, 0, H // 3, 0, W // 3, 1)                                   # touches the top and left borders
        rect(lab, H - 1 - H // 4, H - 1, W - 1 - W // 4, W - 1, 255)        # touches the bottom and right borders
        rect(lab, H // 4, H // 2 + 3, W // 4, W // 2 + 3, 7)                 # overlaps the box of id 1 ...
        rect(lab, H // 3 + 2, H // 3 + 2, W // 3 + 5, W // 3 + 5, 9)         # a single pixel (inside the box of id 7)
        rect(lab, H // 2, H // 2 + 20, W // 2 - 2, W // 2 + 30, 3 if kind == "inst" else 12)      # ... and a lower / higher id overlapping id 7
        if wide:
            rect(lab, H - 3, H - 2, 1, 4, 256)
            rect(lab, H - 6, H - 5, 1, 4, 70000)
            rect(lab, 1, 2, W - 4, W - 2, -1)
        return lab

    def f32(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(*shape, generator=g)

    rgb, gts = f32(-0.2, 1.2, H, W, 3), f32(-0.1, 1.1, H, W, 4)
    depth, conf, conf_pred = f32(0.3, 5.0, H, W, 1), f32(-0.3, 1.3, H, W), f32(-0.3, 1.3, H, W, 1)
    if H * W > 8:
        flat = depth.reshape(-1)
        flat[1], flat[3], flat[5] = NAN, INF, -INF
        rgb.reshape(-1)[2], conf.reshape(-1)[4], conf.reshape(-1)[6] = NAN, NAN, INF
    d = dict(rgb=rgb, depth=depth, gts=gts, semantics=labels("sem"), instances=labels("inst"), inst_conf=conf, sem_gt=labels("sem"),
             inst_gt=labels("gt"), sem_pred=labels("sem"), inst_pred=labels("pred"), inst_conf_pred=conf_pred)
    for k in ("semantics", "instances", "sem_gt", "inst_gt", "sem_pred", "inst_pred"):
        d[k] = d[k].to(dtype)
    return d


LABEL_KEYS = ("semantics", "instances", "inst_conf", "sem_gt", "inst_gt", "sem_pred", "inst_pred", "inst_conf_pred")


def to_device(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def render(vp, d, **drop):
    import pagnerf_amd
    rb = pagnerf_amd.RenderBuffer(rgb=d["rgb"], depth=d["depth"])
    return vp.render(rb, d["gts"], **{k: (None if k in drop else d[k]) for k in LABEL_KEYS})


@functools.lru_cache(maxsize=None)
def case(H, W, dtype, seed=0):
    """(CPU inputs, reference pictures on the CPU) of one case, computed once."""
    import pagnerf_amd
    from pagnerf_amd import visualize as V
    d = make_inputs(H, W, dtype, seed)
    ref = V.validation_pictures_reference(pagnerf_amd.RenderBuffer(rgb=d["rgb"], depth=d["depth"]), d["gts"], **{k: d[k] for k in LABEL_KEYS})
    return d, ref


def assert_same(got, ref, where=""):
    assert list(got) == list(ref), (list(got), list(ref))
    for name in ref:
        a, b = got[name].cpu(), ref[name]
        assert a.dtype == torch.uint8 and a.shape == b.shape
        bad = (a != b).any(-1)
        assert not bool(bad.any()), "%s picture %s: %d pixels differ, first at %s: got %s, want %s" % (
            where, name, int(bad.sum()), bad.nonzero()[0].tolist(), a[bad][0].tolist(), b[bad][0].tolist())


@pytest.mark.parametrize("dtype", DTYPES, ids=["int64", "int32", "uint8"])
@pytest.mark.parametrize("shape", SHAPES, ids=["1x1", "37x53", "130x257"])
def test_every_picture_is_bit_equal_to_the_tensor_op_form(gpu_device, shape, dtype):
    from pagnerf_amd import visualize as V
    d, ref = case(shape[0], shape[1], dtype)
    assert tuple(ref) == V.PICTURES
    vp = V.ValidationPictures()
    got = render(vp, to_device(d, gpu_device))
    assert vp.stack.shape == (15,) + shape + (3,) and got["rgb"].data_ptr() == vp.stack.data_ptr()
    assert_same(got, ref)


def test_reference_form_on_the_gpu_agrees_with_the_cpu(gpu_device):
    """The tensor-op form is the definition on either device: on the GPU (where the benchmark runs it) it gives the CPU's pictures."""
    import pagnerf_amd
    from pagnerf_amd import visualize as V
    d, ref = case(37, 53, torch.int64)
    g = to_device(d, gpu_device)
    on_gpu = V.validation_pictures_reference(pagnerf_amd.RenderBuffer(rgb=g["rgb"], depth=g["depth"]), g["gts"], **{k: g[k] for k in LABEL_KEYS})
    assert_same(on_gpu, ref)


def test_image_without_instances_constant_depth_and_no_finite_depth(gpu_device):
    import pagnerf_amd
    from pagnerf_amd import visualize as V
    H, W = 37, 53
    d = dict(make_inputs(H, W, torch.int64, 3))
    d["instances"] = torch.where(d["instances"] > 0, torch.zeros_like(d["instances"]), d["instances"])          # ids 0 and -1 only
    d["inst_pred"] = torch.zeros_like(d["inst_pred"])
    d["depth"] = torch.full((H, W, 1), 2.5)
    g = to_device(d, gpu_device)
    boxes = V.instance_boxes(g["instances"])
    assert bool((boxes[:, 0] > boxes[:, 2]).all())
    ref = V.validation_pictures_reference(pagnerf_amd.RenderBuffer(rgb=d["rgb"], depth=d["depth"]), d["gts"], **{k: d[k] for k in LABEL_KEYS})
    assert torch.equal(ref["depth"], V.default_table()[0].expand(H, W, 3))
    vp = V.ValidationPictures()
    assert_same(render(vp, g), ref)
    d["depth"] = torch.full((H, W, 1), NAN)
    d["depth"][0, 0], d["depth"][1, 1] = INF, -INF
    ref = V.validation_pictures_reference(pagnerf_amd.RenderBuffer(rgb=d["rgb"], depth=d["depth"]), d["gts"], **{k: d[k] for k in LABEL_KEYS})
    assert int(ref["depth"].sum()) == 0
    assert_same(render(vp, to_device(d, gpu_device)), ref, "no finite depth:")


@pytest.mark.parametrize("shape", SHAPES, ids=["1x1", "37x53", "130x257"])
def test_instance_boxes_equal_the_reference_form(gpu_device, shape):
    from pagnerf_amd import visualize as V
    for dtype in DTYPES:
        d, _ = case(shape[0], shape[1], dtype)
        for key in ("instances", "inst_pred"):
            got = V.instance_boxes(d[key].to(gpu_device))
            assert got.dtype == torch.int32 and torch.equal(got.cpu(), V.instance_boxes_reference(d[key]))
    lab = case(shape[0], shape[1], torch.int64)[0]["instances"]
    assert torch.equal(V.instance_boxes(lab.to(gpu_device), max_id=8).cpu(), V.instance_boxes_reference(lab, max_id=8))


def test_single_picture_functions(gpu_device):
    from pagnerf_amd import visualize as V
    d, ref = case(37, 53, torch.int64)
    g = to_device(d, gpu_device)
    assert torch.equal(V.label_colors(g["inst_pred"]).cpu(), ref["inst_pred"])
    assert torch.equal(V.label2rgb(g["semantics"]).cpu(), ref["sem"])
    rgb8 = ref["rgb"].to(gpu_device)
    assert torch.equal(V.label2rgb(g["semantics"], image=rgb8).cpu(), ref["sem_rgb"])
    assert torch.equal(V.label2rgb(g["semantics"], image=rgb8, alpha=0.3).cpu(), V.label2rgb_reference(d["semantics"], image=ref["rgb"], alpha=0.3))
    assert torch.equal(V.depth2rgb(g["depth"]).cpu(), ref["depth"])
    assert torch.equal(V.depth2rgb(g["inst_conf"], 0.0, 1.0).cpu(), ref["inst_conf"])
    assert torch.equal(V.depth2rgb(g["depth"], 1.0, 4.0).cpu(), V.depth2rgb_reference(d["depth"], 1.0, 4.0))
    assert torch.equal(V.depth2rgb(g["depth"], max_value=4.0).cpu(), V.depth2rgb_reference(d["depth"], max_value=4.0))
    assert torch.equal(V.overlay_instances(rgb8, g["instances"]).cpu(), ref["inst_rgb"])
    assert torch.equal(V.overlay_instances(rgb8, g["instances"], width=2, alpha=0.4, max_id=8).cpu(),
                       V.overlay_instances_reference(ref["rgb"], d["instances"], width=2, alpha=0.4, max_id=8))
    with pytest.raises(RuntimeError, match="GPU"):
        V.label_colors(d["instances"])
    with pytest.raises(TypeError):
        V.label_colors(g["instances"].to(torch.int16))


def test_absent_inputs_leave_their_pictures_out(gpu_device):
    from pagnerf_amd import visualize as V
    d, ref = case(37, 53, torch.int32)
    g = to_device(d, gpu_device)
    vp = V.ValidationPictures()
    drop = ("instances", "inst_conf", "sem_pred", "inst_gt")
    got = render(vp, g, **dict.fromkeys(drop))
    want = V.ValidationPictures.names(semantics=1, sem_gt=1, inst_pred=1, inst_conf_pred=1)
    assert tuple(got) == want == ("rgb", "gt", "depth", "sem", "sem_rgb", "sem_gt", "inst_pred", "inst_pred_rgb", "inst_conf_pred")
    assert vp.stack.shape[0] == len(want)
    assert_same(got, {n: ref[n] for n in want})
    import pagnerf_amd
    only = vp.render(pagnerf_amd.RenderBuffer(rgb=g["rgb"]), None)
    assert tuple(only) == ("rgb",) and torch.equal(only["rgb"].cpu(), ref["rgb"])


def test_second_render_shows_no_stale_state_and_overwrites_garbage(gpu_device):
    """Three renders on one object (both workspace halves used again): other inputs of the same shape, smaller boxes and a narrower depth range than
    the render before - stale minima / maxima would show; the stack is filled with garbage before each render and must be overwritten completely."""
    from pagnerf_amd import visualize as V
    H, W = 130, 257
    vp = V.ValidationPictures()
    assert_same(render(vp, to_device(case(H, W, torch.int64)[0], gpu_device)), case(H, W, torch.int64)[1])
    for seed in (1, 2, 0):
        d, ref = case(H, W, torch.int64, seed)
        if seed:
            d = dict(d)
            small = torch.zeros(H, W, dtype=torch.int64)
            rect(small, 40 + seed, 60, 50, 90 + seed, 1)                     # id 1 again, with a smaller box than before
            rect(small, 70, 75, 100, 130, 255)
            d["instances"], d["inst_pred"] = small, small.flip(0)
            d["depth"] = d["depth"].nan_to_num(1.0, 1.0, 1.0).clamp(1.0 + 0.1 * seed, 2.0)
            import pagnerf_amd
            ref = V.validation_pictures_reference(pagnerf_amd.RenderBuffer(rgb=d["rgb"], depth=d["depth"]), d["gts"], **{k: d[k] for k in LABEL_KEYS})
        vp._planes.fill_(0xA5)
        got = render(vp, to_device(d, gpu_device))
        assert_same(got, ref, "seed %d:" % seed)


def test_entry_points_refuse_bad_arguments(gpu_device):
    from pagnerf_amd import visualize as V
    lab = torch.zeros(4, 4, dtype=torch.int64, device=gpu_device)
    with pytest.raises(ValueError):
        V.instance_boxes(lab, max_id=5000)
    with pytest.raises(ValueError):
        V.ValidationPictures(max_id=0)
    with pytest.raises(RuntimeError, match="workspace"):
        V._launch(4, 4, {}, torch.zeros(8, dtype=torch.int32, device=gpu_device), 0, labels={"instances": lab}, paint=False)
    out = torch.empty(4, 4, 3, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(RuntimeError, match="sem"):
        V._launch(4, 4, {"sem": out}, V.new_workspace(255, gpu_device), 0, stats=False)
