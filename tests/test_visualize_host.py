"""pagnerf_amd/visualize.py without a GPU: the tensor-op forms that define the validation pictures against hand-written expectations, the PNG writer
and reader, the picture names per input set, and the frame-selection rule."""
import struct
import zlib

import numpy as np
import pytest
import torch

from pagnerf_amd import visualize as V


def test_label_colours_are_the_voc_bit_procedure():
    ids = torch.tensor([0, 1, 2, 3, 4, 255, 256, -1, 70000])
    want = [(0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128), (224, 224, 192), (0, 0, 32), (0, 0, 0)]
    got = V.label_colors_reference(ids)
    assert got.dtype == torch.uint8 and got.shape == (9, 3)
    assert [tuple(r) for r in got[:8].tolist()] == want
    # 70000 = 0b1_0001_0001_0111_0000 -> octal digits (low first) 0 6 5 0 1 2: r = bit0 of each digit from the top bit down
    digits = [(70000 >> (3 * j)) & 7 for j in range(8)]
    expect = tuple(sum(((d >> c) & 1) << (7 - j) for j, d in enumerate(digits)) for c in range(3))
    assert tuple(got[8].tolist()) == expect
    for dtype in (torch.int32, torch.uint8):
        assert torch.equal(V.label_colors_reference(torch.tensor([1, 4, 255]).to(dtype)), got[[1, 4, 5]])


def test_image_to_uint8_truncates_and_clamps():
    x = torch.tensor([[[0.0, 1.0, 0.5], [-0.2, 1.7, 0.999], [float("nan"), float("inf"), 0.25]]])
    assert V.image_u8_reference(x).tolist() == [[[0, 255, 127], [0, 255, 254], [0, 255, 63]]]
    assert V.image_u8_reference(torch.rand(2, 2, 4)).shape == (2, 2, 3)


def test_depth_ramp_with_non_finite_values_and_constant_depth():
    table = torch.stack((torch.arange(256), 255 - torch.arange(256), torch.full((256,), 7)), 1).to(torch.uint8)
    d = torch.tensor([[1.0, 2.0, 3.0], [float("nan"), float("inf"), 1.5], [2.999, 1.0078125, -float("inf")]])
    got = V.depth2rgb_reference(d, table=table)
    # min 1, max 3: t = (d - 1) / 2, index min(255, floor(256 t))
    idx = [[0, 128, 255], [None, None, 64], [255, 1, None]]
    for y in range(3):
        for x in range(3):
            want = [0, 0, 0] if idx[y][x] is None else [idx[y][x], 255 - idx[y][x], 7]
            assert got[y, x].tolist() == want, (y, x)
    const = V.depth2rgb_reference(torch.full((2, 3), 4.25), table=table)
    assert const.reshape(-1, 3).tolist() == [[0, 255, 7]] * 6
    # the fixed range of the confidence pictures: t clamped
    conf = V.depth2rgb_reference(torch.tensor([[-0.5, 0.0, 0.5, 1.0, 1.5]]), 0.0, 1.0, table=table)
    assert conf[0, :, 0].tolist() == [0, 0, 128, 255, 255]
    assert V.depth2rgb_reference(torch.tensor([[0.0, 1.0]]))[0].tolist() == [V.default_table()[0].tolist(), V.default_table()[255].tolist()]
    assert V.default_table().shape == (256, 3) and V.default_table().dtype == torch.uint8


def test_half_blend_rounds_half_to_even():
    # grey of (10, 10, 10) is rint(2.99 + 5.87 + 1.14) = 10; colour of id 1 is (128, 0, 0): (69, 5, 5).  grey 11: 0.5 * 11 = 5.5 -> 6 (even), 69.5 -> 70
    lab = torch.tensor([[1, 1, 0, 0]])
    img = torch.tensor([[[10, 10, 10], [11, 11, 11], [13, 13, 13], [255, 0, 0]]], dtype=torch.uint8)
    got = V.label2rgb_reference(lab, image=img)
    assert got[0].tolist() == [[69, 5, 5], [70, 6, 6], [6, 6, 6], [38, 38, 38]]          # 6.5 -> 6 (even); rint(0.299 * 255) = 76 -> 38
    assert torch.equal(V.label2rgb_reference(lab), V.label_colors_reference(lab))
    neg = V.label2rgb_reference(torch.tensor([[-1]]), image=img[:, :1])
    assert neg[0, 0].tolist() == [5, 5, 5]                                             # a negative id takes colour 0


def hand_drawn():
    lab = torch.zeros(12, 16, dtype=torch.int64)
    lab[2:5, 3:9] = 1                       # box (3, 2, 8, 4)
    lab[7, 10] = 2                          # a single pixel
    lab[0, 0] = 3
    lab[11, 15] = 3                         # two far pixels: the whole image
    lab[5, 5] = 300                         # above max_id
    lab[6, 6] = -1
    return lab


def test_box_tables_of_a_hand_drawn_label_image():
    boxes = V.instance_boxes_reference(hand_drawn(), max_id=255)
    assert boxes.shape == (256, 4) and boxes.dtype == torch.int32
    assert boxes[1].tolist() == [3, 2, 8, 4] and boxes[2].tolist() == [10, 7, 10, 7] and boxes[3].tolist() == [0, 0, 15, 11]
    absent = [2 ** 31 - 1, 2 ** 31 - 1, -1, -1]
    assert boxes[0].tolist() == absent and boxes[4].tolist() == absent and boxes[255].tolist() == absent
    assert bool((boxes[4:, 0] > boxes[4:, 2]).all())
    assert V.instance_boxes_reference(hand_drawn(), max_id=2).shape == (3, 4)


def test_outline_rule_on_a_large_and_on_a_small_box():
    grey = torch.full((24, 24, 3), 50, dtype=torch.uint8)
    lab = torch.zeros(24, 24, dtype=torch.int64)
    lab[2, 2] = 2
    lab[21, 21] = 2                         # id 2 (colour (0,128,0)): box (2,2)-(21,21), 20 x 20
    got = V.overlay_instances_reference(grey, lab, width=6)
    on = torch.zeros(24, 24, dtype=torch.bool)
    on[2:22, 2:22] = True
    on[8:16, 8:16] = False                  # 6 pixels inward on every side leave the inner 8 x 8 free
    want = torch.where(on[..., None], torch.tensor([0, 128, 0], dtype=torch.uint8), grey)
    # the two labelled pixels blend on the green channel only: trunc(0.3 * 128 + 0.7 * 128) = 128 (on the outline)
    assert torch.equal(got, want)
    small = torch.zeros(12, 12, dtype=torch.int64)
    small[3, 2] = 2
    small[7, 10] = 2                        # box x 2..10, y 3..7: 9 wide, 5 high - every pixel lies within 6 of the top or bottom edge
    got = V.overlay_instances_reference(grey[:12, :12], small, width=6)
    on = torch.zeros(12, 12, dtype=torch.bool)
    on[3:8, 2:11] = True
    assert torch.equal(got, torch.where(on[..., None], torch.tensor([0, 128, 0], dtype=torch.uint8), grey[:12, :12]))


def test_overlapping_outlines_the_highest_id_wins():
    base = torch.full((20, 20, 3), 10, dtype=torch.uint8)
    lab = torch.zeros(20, 20, dtype=torch.int64)
    lab[0, 0] = lab[9, 9] = 4               # colour (0,0,128), box (0,0)-(9,9)
    lab[5, 5] = lab[14, 14] = 2             # colour (0,128,0), box (5,5)-(14,14)
    got = V.overlay_instances_reference(base, lab, width=2)
    assert got[5, 8].tolist() == [0, 0, 128]          # column 8 is on id 4's outline, row 5 on id 2's: id 4 is drawn last
    assert got[5, 12].tolist() == [0, 128, 0]         # only id 2's outline
    assert got[9, 6].tolist() == [0, 0, 128]          # id 4's bottom edge crosses id 2's left edge: id 4
    assert got[7, 7].tolist() == [10, 10, 10]         # inside both boxes, on neither outline
    swapped = V.overlay_instances_reference(base, torch.where(lab == 4, 1, torch.where(lab == 2, 6, lab)), width=2)
    assert swapped[9, 6].tolist() == [0, 128, 128]    # now the box (5,5)-(14,14) carries the higher id 6 (colour (0,128,128)) and is on top
    assert swapped[9, 2].tolist() == [128, 0, 0]      # id 1's bottom edge where id 6's box does not reach


def test_overlay_mask_is_per_channel():
    base = torch.tensor([[[200, 100, 50], [200, 100, 50]]], dtype=torch.uint8)
    lab = torch.tensor([[1, 0]])
    got = V.overlay_instances_reference(base, lab, width=1, max_id=1)
    # id 1 = (128, 0, 0); its 1 x 1 box outline paints the pixel (128, 0, 0) first, then only the red channel blends: trunc(0.3 * 128 + 0.7 * 128)
    red = int(np.float32(np.float32(1.0 - 0.7) * np.float32(128)) + np.float32(np.float32(0.7) * np.float32(128)))
    assert got[0, 0].tolist() == [red, 0, 0] and got[0, 1].tolist() == [200, 100, 50]
    # an id above max_id has no box: only the channels where its colour is non-zero blend
    far = V.overlay_instances_reference(base, torch.tensor([[257, 0]]), width=1)      # 257 = colour (128, 0, 32): red and blue blend, green stays
    r = int(np.float32(np.float32(1.0 - 0.7) * np.float32(200)) + np.float32(np.float32(0.7) * np.float32(128)))
    b = int(np.float32(np.float32(1.0 - 0.7) * np.float32(50)) + np.float32(np.float32(0.7) * np.float32(32)))
    assert far[0, 0].tolist() == [r, 100, b] and (r, b) == (149, 37)
    # id 1 inside its own box, off the 1-pixel outline: only the red channel blends
    block = torch.zeros(5, 5, dtype=torch.int64)
    block[1:4, 1:4] = 1
    mid = V.overlay_instances_reference(base[:, :1].expand(5, 5, 3).contiguous(), block, width=1)
    assert mid[2, 2].tolist() == [149, 100, 50] and mid[1, 1].tolist() == [128, 0, 0] and mid[0, 0].tolist() == [200, 100, 50]


@pytest.mark.parametrize("shape", [(1, 1, 3), (37, 53, 3), (1, 1), (37, 53)])
def test_png_round_trip(tmp_path, shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.integers(0, 256, size=shape, dtype=np.uint8)
    path = str(tmp_path / "a.png")
    V.write_png(path, a)
    back = V.read_png(path)
    assert back.dtype == np.uint8 and back.shape == a.shape and np.array_equal(back, a)
    V.write_png(path, torch.from_numpy(a))
    assert np.array_equal(V.read_png(path), a)


def test_png_header_bytes(tmp_path):
    path = str(tmp_path / "h.png")
    V.write_png(path, np.zeros((37, 53, 3), np.uint8))
    blob = open(path, "rb").read()
    assert blob[:8] == bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])
    assert blob[8:12] == struct.pack(">I", 13) and blob[12:16] == b"IHDR"
    width, height, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", blob[16:29])
    assert (width, height, depth, colour, compression, filt, interlace) == (53, 37, 8, 2, 0, 0, 0)
    assert struct.unpack(">I", blob[29:33])[0] == zlib.crc32(blob[12:29]) & 0xffffffff
    assert blob[-12:] == struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND") & 0xffffffff)
    V.write_png(path, np.zeros((4, 5), np.uint8))
    assert struct.unpack(">IIBBBBB", open(path, "rb").read()[16:29]) == (5, 4, 8, 0, 0, 0, 0)
    with pytest.raises(TypeError):
        V.write_png(path, np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError):
        V.write_png(path, np.zeros((4, 5, 2), np.uint8))


def test_picture_names_per_input_set():
    names = V.ValidationPictures.names
    assert names() == ("rgb", "gt", "depth")
    assert names(depth=None, gts=None) == ("rgb",)
    assert names(semantics=1) == ("rgb", "gt", "depth", "sem", "sem_rgb")
    assert names(semantics=1, sem_gt=1, sem_pred=1) == ("rgb", "gt", "depth", "sem", "sem_rgb", "sem_gt", "sem_pred", "sem_pred_rgb")
    assert names(instances=1, inst_conf=1) == ("rgb", "gt", "depth", "inst", "inst_conf", "inst_rgb")
    assert names(inst_pred=1, inst_conf_pred=1, inst_gt=1) == ("rgb", "gt", "depth", "inst_gt", "inst_pred", "inst_pred_rgb", "inst_conf_pred")
    full = names(semantics=1, instances=1, inst_conf=1, sem_gt=1, inst_gt=1, sem_pred=1, inst_pred=1, inst_conf_pred=1)
    assert full == V.PICTURES and len(full) == 15
    t = torch.zeros(2, 2, dtype=torch.int64)
    assert names(semantics=t, instances=None) == ("rgb", "gt", "depth", "sem", "sem_rgb")


def test_reference_pictures_follow_the_names():
    import pagnerf_amd
    rb = pagnerf_amd.RenderBuffer(rgb=torch.rand(5, 7, 3), depth=torch.rand(5, 7, 1))
    lab = torch.randint(-1, 6, (5, 7))
    pics = V.validation_pictures_reference(rb, torch.rand(5, 7, 3), semantics=lab, instances=lab.clamp_min(0), inst_conf=torch.rand(5, 7))
    assert tuple(pics) == ("rgb", "gt", "depth", "sem", "sem_rgb", "inst", "inst_conf", "inst_rgb")
    assert all(p.shape == (5, 7, 3) and p.dtype == torch.uint8 for p in pics.values())
    assert torch.equal(pics["sem"], V.label_colors_reference(lab))


def test_frame_selection_rule():
    sel = V.select_frame
    # first clause: every n-th frame
    assert [i for i in range(40) if sel(i, 40, 15)] == [0, 15, 30]
    assert [i for i in range(5) if sel(i, 5, 1)] == [0, 1, 2, 3, 4]
    # second clause: at least as many frames asked for as there are
    assert all(sel(i, 10, 15) for i in range(10)) and all(sel(i, 15, 15) for i in range(15))
    assert [i for i in range(16) if sel(i, 16, 15)] == [0, 15]
    # third clause: labelled frames with render_val_labels
    assert not sel(7, 40, 15, render_val_labels=True, has_labels=False)
    assert sel(7, 40, 15, render_val_labels=True, has_labels=True)
    assert not sel(7, 40, 15, render_val_labels=False, has_labels=True)
    # num_val_frames_to_save <= 0: only the third clause
    assert not any(sel(i, 4, 0) for i in range(4)) and not any(sel(i, 4, -1) for i in range(4))
    assert sel(0, 4, 0, render_val_labels=True, has_labels=True) and not sel(0, 4, 0, render_val_labels=True, has_labels=False)


def test_public_names_are_exported():
    import pagnerf_amd
    for name in ("ValidationPictures", "label_colors", "label2rgb", "depth2rgb", "instance_boxes", "overlay_instances", "write_png", "read_png"):
        assert hasattr(pagnerf_amd, name), name
    tr = pagnerf_amd.PanopticTrainer(None, None)
    assert tr.val_pictures is False
    assert pagnerf_amd.PanopticTrainer(None, None, val_pictures=True).val_pictures is True
