"""The validation pictures: label colours, label / image blends, depth and confidence ramps, boxed instance overlays, and PNG files.

The reference paints these per validation image with a chain of .cpu() copies and numpy calls (pc_nerf/trainer.py:710-829, written at :855-896): imgviz
`label_colormap` / `label2rgb` / `depth2rgb`, torchvision `masks_to_boxes` / `draw_bounding_boxes`, a 0.7 blend.  Here one image is two launches of
csrc/visualize.hip on device tensors (pag_vis_stats: finite depth range and per-id pixel boxes; pag_vis_paint: every picture, each pixel written once).

The `*_reference` functions are the DEFINITION of every picture, as tensor operations that also run on CPU tensors; the kernels are tested bit for
bit against them.  imgviz and torchvision are third party and not part of the reference tree: their behaviour is restated here from memory, so parity
with them is unpinned.  Stated divergences:
  * a negative label (unlabelled, -1) is painted black; imgviz paints seeded noise there;
  * boxes are drawn for every present id in [1, max_id]; the reference drops the smallest present id, whatever it is;
  * the colour of an id does not depend on the `n` of label_colormap(n), so no maximum is taken;
  * the overlay's mask is per CHANNEL (`inst_imgs[-1] != 0` on an [H,W,3] array, :804): a channel blends where the label colour's channel is
    non-zero - the reference's quirk, kept.
"""
import ctypes
import os
import struct
import zlib
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

# picture order of the stack = the PAG_VIS_* codes of include/pagnerf_hip.h
PICTURES = ("rgb", "gt", "depth", "sem", "sem_rgb", "sem_gt", "sem_pred", "sem_pred_rgb", "inst", "inst_conf", "inst_rgb", "inst_gt", "inst_pred",
            "inst_pred_rgb", "inst_conf_pred")
_LABELS = ("semantics", "instances", "sem_gt", "inst_gt", "sem_pred", "inst_pred")           # PAG_VIS_L_*
_LABEL_DTYPES = {torch.int64: 8, torch.int32: 4, torch.uint8: 1}
_INT_MAX = 2 ** 31 - 1
_TABLE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "magma_u8.txt")
_TABLES = {}


def default_table(device="cpu"):
    """The 256-entry `magma` colour map as uint8 [256,3]: 768 values shipped with the package as a text file, one `r g b` line per entry (generated
    once from matplotlib's `magma`; matplotlib is not imported at run time)."""
    key = str(device)
    if key not in _TABLES:
        with open(_TABLE_FILE) as f:
            raw = [int(v) for line in f if not line.startswith("#") for v in line.split()]
        if len(raw) != 768 or min(raw) < 0 or max(raw) > 255:
            raise RuntimeError("%s: expected 768 values in [0, 255], found %d" % (_TABLE_FILE, len(raw)))
        _TABLES[key] = torch.tensor(raw, dtype=torch.uint8).reshape(256, 3).to(device)
    return _TABLES[key]


def select_frame(idx, num_imgs, num_val_frames_to_save, render_val_labels=False, has_labels=False):
    """pc_nerf/trainer.py:855-857: frame `idx` of `num_imgs` is written when idx % num_val_frames_to_save == 0, or num_val_frames_to_save >= num_imgs,
    or (render_val_labels and the frame carries labels).  num_val_frames_to_save <= 0 leaves only the third clause (the reference divides by it)."""
    n = int(num_val_frames_to_save)
    if n > 0 and (idx % n == 0 or n >= num_imgs):
        return True
    return bool(render_val_labels and has_labels)


# --------------------------------------------------------------------------------------------------------------------- the tensor-op forms
def image_u8_reference(x):
    """f32 [..., >=3] in [0, 1] -> uint8 [..., 3]: trunc(clamp(x, 0, 1) * 255), NaN as 0 (:710 `rb.image().byte()`, :862)."""
    return (torch.nan_to_num(x[..., :3].float(), nan=0.0).clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def label_colors_reference(labels):
    """Integer labels [...] -> uint8 [..., 3]: imgviz.label_colormap's PASCAL-VOC bit procedure, computed (no table): for j = 0..7
    r |= bit0(id) << (7-j), g |= bit1(id) << (7-j), b |= bit2(id) << (7-j), id >>= 3.  Negative ids are black."""
    v = labels.long()
    neg = v < 0
    v = v.clamp_min(0)
    r, g, b = torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)
    for j in range(8):
        r |= (v & 1) << (7 - j)
        g |= ((v >> 1) & 1) << (7 - j)
        b |= ((v >> 2) & 1) << (7 - j)
        v = v >> 3
    out = torch.stack((r, g, b), -1)
    out[neg] = 0
    return out.to(torch.uint8)


def label2rgb_reference(labels, image=None, alpha=0.5):
    """imgviz.label2rgb(label, image=image, alpha=alpha) (:721-727): the label colours; with a uint8 [H,W,3] image
    rint((1 - alpha) * grey + alpha * colour), grey = rint(0.299 R + 0.587 G + 0.114 B), all in f32, round-half-even."""
    colour = label_colors_reference(labels)
    if image is None:
        return colour
    im = image.float()
    grey = torch.round(0.299 * im[..., 0] + 0.587 * im[..., 1] + 0.114 * im[..., 2])
    return torch.round((1.0 - alpha) * grey[..., None] + alpha * colour.float()).to(torch.uint8)


def depth2rgb_reference(depth, min_value=None, max_value=None, table=None):
    """imgviz.depth2rgb (:712, and with the range 0..1 :742, :746): t = (d - min) / (max - min) clamped to [0, 1], index min(255, floor(t * 256)) into the
    256 x 3 table.  min / max default to the finite minimum / maximum of d; a non-finite d is black; max == min gives index 0."""
    d = depth.float().reshape(depth.shape[0], depth.shape[1])
    table = default_table(d.device) if table is None else table
    fin = torch.isfinite(d)
    lo = torch.where(fin, d, torch.full_like(d, float("inf"))).min() if min_value is None else torch.tensor(float(min_value), device=d.device)
    hi = torch.where(fin, d, torch.full_like(d, float("-inf"))).max() if max_value is None else torch.tensor(float(max_value), device=d.device)
    ok = fin & (hi != lo)
    t = (d - lo) / (hi - lo)
    t = torch.where(ok, t, torch.zeros_like(t)).clamp(0.0, 1.0)
    idx = torch.floor(t * 256.0).clamp(max=255.0).long()
    out = table[idx]
    out[~fin] = 0
    return out


def instance_boxes_reference(labels, max_id=255):
    """torchvision.ops.masks_to_boxes per id (:775, :822): int32 [max_id + 1, 4], row id = the inclusive pixel box (x0, y0, x1, y1) of the pixels that carry
    id, for ids in [1, max_id]; an absent id (and row 0) keeps (INT32_MAX, INT32_MAX, -1, -1), so x0 > x1."""
    H, W = labels.shape
    v = labels.long().reshape(-1)
    ok = (v >= 1) & (v <= max_id)
    ys, xs = torch.meshgrid(torch.arange(H, device=v.device), torch.arange(W, device=v.device), indexing="ij")
    ids, xs, ys = v[ok], xs.reshape(-1)[ok], ys.reshape(-1)[ok]
    lo = torch.full((max_id + 1,), _INT_MAX, dtype=torch.int64, device=v.device)
    hi = torch.full((max_id + 1,), -1, dtype=torch.int64, device=v.device)
    return torch.stack((lo.scatter_reduce(0, ids, xs, "amin"), lo.scatter_reduce(0, ids, ys, "amin"), hi.scatter_reduce(0, ids, xs, "amax"),
                        hi.scatter_reduce(0, ids, ys, "amax")), 1).to(torch.int32)


def overlay_instances_reference(rgb_u8, labels, width=6, alpha=0.7, max_id=255):
    """:751-806 / :815-829: the uint8 rgb picture, then draw_bounding_boxes: the outline of every present id's box in ascending id order, in the id's colour,
    `width` pixels inward (a pixel of the inclusive box is on the outline when it lies fewer than `width` pixels from one of the four edges), then per
    channel where the label colour's channel is non-zero trunc((1 - alpha) * base + alpha * colour) in f32."""
    H, W = labels.shape
    out = rgb_u8[..., :3].clone()
    boxes = instance_boxes_reference(labels, max_id)
    ys, xs = torch.meshgrid(torch.arange(H, device=labels.device), torch.arange(W, device=labels.device), indexing="ij")
    ids = torch.arange(max_id + 1, device=labels.device)
    colours = label_colors_reference(ids)
    for i, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
        if i < 1 or x0 > x1:
            continue
        on = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1) & ((xs - x0 < width) | (x1 - xs < width) | (ys - y0 < width) | (y1 - ys < width))
        out[on] = colours[i]
    colour = label_colors_reference(labels)
    blended = ((1.0 - alpha) * out.float() + alpha * colour.float()).to(torch.uint8)
    return torch.where(colour != 0, blended, out)


def _picture_names(depth, gts, semantics, instances, inst_conf, sem_gt, inst_gt, sem_pred, inst_pred, inst_conf_pred):
    have = {"rgb": True, "gt": gts, "depth": depth, "sem": semantics, "sem_rgb": semantics, "sem_gt": sem_gt, "sem_pred": sem_pred,
            "sem_pred_rgb": sem_pred, "inst": instances, "inst_conf": inst_conf, "inst_rgb": instances, "inst_gt": inst_gt, "inst_pred": inst_pred,
            "inst_pred_rgb": inst_pred, "inst_conf_pred": inst_conf_pred}
    return tuple(n for n in PICTURES if have[n] is not None and have[n] is not False)


def validation_pictures_reference(rb, gts, semantics=None, instances=None, inst_conf=None, sem_gt=None, inst_gt=None, sem_pred=None, inst_pred=None,
                                  inst_conf_pred=None, max_id=255, table=None):
    """ValidationPictures.render as tensor operations: the ordered dict name -> uint8 [H,W,3] that the two launches must reproduce exactly."""
    rgb = image_u8_reference(rb.rgb)
    H, W = rgb.shape[:2]
    depth = getattr(rb, "depth", None)
    sq = lambda x: None if x is None else x.reshape(H, W)
    semantics, instances, sem_gt, inst_gt, sem_pred, inst_pred = (sq(x) for x in (semantics, instances, sem_gt, inst_gt, sem_pred, inst_pred))
    make = {
        "rgb": lambda: rgb,
        "gt": lambda: image_u8_reference(gts),
        "depth": lambda: depth2rgb_reference(depth.reshape(H, W), table=table),
        "sem": lambda: label_colors_reference(semantics),
        "sem_rgb": lambda: label2rgb_reference(semantics, image=rgb),
        "sem_gt": lambda: label_colors_reference(sem_gt),
        "sem_pred": lambda: label_colors_reference(sem_pred),
        "sem_pred_rgb": lambda: label2rgb_reference(sem_pred, image=rgb),
        "inst": lambda: label_colors_reference(instances),
        "inst_conf": lambda: depth2rgb_reference(sq(inst_conf), 0.0, 1.0, table=table),
        "inst_rgb": lambda: overlay_instances_reference(rgb, instances, max_id=max_id),
        "inst_gt": lambda: label_colors_reference(inst_gt),
        "inst_pred": lambda: label_colors_reference(inst_pred),
        "inst_pred_rgb": lambda: overlay_instances_reference(rgb, inst_pred, max_id=max_id),
        "inst_conf_pred": lambda: depth2rgb_reference(sq(inst_conf_pred), 0.0, 1.0, table=table),
    }
    names = _picture_names(depth, gts, semantics, instances, inst_conf, sem_gt, inst_gt, sem_pred, inst_pred, inst_conf_pred)
    return OrderedDict((n, make[n]()) for n in names)


# ------------------------------------------------------------------------------------------------------------------------- the device path
def new_workspace(max_id, device):
    """The int32 workspace of pag_vis_stats / pag_vis_paint in its initial state (include/pagnerf_hip.h): two halves of {-1, 0, 0, 0} and a
    (INT32_MAX, INT32_MAX, -1, -1) row per id and table."""
    words = _lib.load().pag_vis_workspace_bytes(int(max_id)) // 4
    if words == 0:
        raise ValueError("max_id %d not in [1, %d]" % (max_id, _lib.VIS_MAX_ID))
    half = torch.cat((torch.tensor([-1, 0, 0, 0], dtype=torch.int32), torch.tensor([_INT_MAX, _INT_MAX, -1, -1], dtype=torch.int32).repeat(2 * (max_id + 1))))
    return half.repeat(2).to(device)


def _label(x, H, W):
    if x is None:
        return None
    if x.dtype not in _LABEL_DTYPES:
        raise TypeError("label image of dtype %s: int64, int32 or uint8 expected" % x.dtype)
    return x.reshape(H, W).contiguous()


def _f32(x, shape):
    if x is None:
        return None
    return x.reshape(shape).float().contiguous()


def _launch(H, W, outs, ws, phase, *, rgb=None, gt=None, depth=None, labels=None, conf=(None, None), table=None, max_id=255, width=6, blend_alpha=0.5,
            overlay_alpha=0.7, conf_range=(0.0, 1.0), stats=True, paint=True):
    """Fill pag_vis_args and run the two launches on torch's current stream.  outs: {picture name: uint8 plane [H,W,3]}.  The tensors named here
    stay referenced by the caller until the launches are enqueued (same stream: that is enough for torch's allocator)."""
    lib = _lib.load()
    a = _lib.VisArgs()
    a.H, a.W, a.phase = H, W, phase
    if rgb is not None:
        a.rgb, a.rgb_is_u8, a.rgb_stride = _lib.ptr(rgb), int(rgb.dtype == torch.uint8), rgb.shape[-1]
    if gt is not None:
        a.gt, a.gt_stride = _lib.ptr(gt), gt.shape[-1]
    a.depth = _lib.ptr(depth)
    for i, name in enumerate(_LABELS):
        x = (labels or {}).get(name)
        if x is not None:
            a.labels[i], a.label_bytes[i] = _lib.ptr(x), _LABEL_DTYPES[x.dtype]
    a.conf[0], a.conf[1] = _lib.ptr(conf[0]), _lib.ptr(conf[1])
    a.table = _lib.ptr(table)
    a.max_id, a.box_width = int(max_id), int(width)
    a.blend_keep, a.blend_alpha = 1.0 - blend_alpha, blend_alpha
    a.overlay_keep, a.overlay_alpha = 1.0 - overlay_alpha, overlay_alpha
    a.conf_min, a.conf_max = conf_range
    a.workspace, a.workspace_bytes = _lib.ptr(ws), ws.numel() * 4
    for name, plane in outs.items():
        a.out[PICTURES.index(name)] = _lib.ptr(plane)
    if stats:
        _lib.check(lib.pag_vis_stats(ctypes.byref(a), _lib.stream()), "pag_vis_stats")
    if paint:
        _lib.check(lib.pag_vis_paint(ctypes.byref(a), _lib.stream()), "pag_vis_paint")


def _gpu_table(table, device):
    table = default_table(device) if table is None else table
    if table.dtype != torch.uint8 or tuple(table.shape) != (256, 3):
        raise ValueError("colour table: uint8 [256,3] expected")
    return table.to(device).contiguous()


def label_colors(labels):
    """label_colors_reference on the device: integer labels [H,W] (int64 / int32 / uint8) -> uint8 [H,W,3]."""
    H, W = labels.shape
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=labels.device)
    _launch(H, W, {"sem": out}, new_workspace(1, labels.device), 0, labels={"semantics": _label(labels, H, W)}, max_id=1, stats=False)
    return out


def label2rgb(labels, image=None, alpha=0.5):
    """label2rgb_reference on the device; image: uint8 [H,W,3] or None."""
    if image is None:
        return label_colors(labels)
    H, W = labels.shape
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=labels.device)
    _launch(H, W, {"sem_rgb": out}, new_workspace(1, labels.device), 0, rgb=image.contiguous(), labels={"semantics": _label(labels, H, W)}, max_id=1,
            blend_alpha=alpha, stats=False)
    return out


def depth2rgb(depth, min_value=None, max_value=None, table=None):
    """depth2rgb_reference on the device: f32 [H,W] (or [H,W,1]) -> uint8 [H,W,3].  With neither bound given the finite range comes from the statistics
    launch and nothing is read back; with one bound given the other is read from the device once."""
    H, W = depth.shape[:2]
    d = _f32(depth, (H, W))
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=d.device)
    ws, table = new_workspace(1, d.device), _gpu_table(table, d.device)
    if min_value is None and max_value is None:
        _launch(H, W, {"depth": out}, ws, 0, depth=d, table=table, max_id=1)
        return out
    fin = torch.isfinite(d)
    if min_value is None:
        min_value = float(torch.where(fin, d, torch.full_like(d, float("inf"))).min())
    if max_value is None:
        max_value = float(torch.where(fin, d, torch.full_like(d, float("-inf"))).max())
    _launch(H, W, {"inst_conf": out}, ws, 0, conf=(d, None), table=table, max_id=1, conf_range=(min_value, max_value), stats=False)
    return out


def instance_boxes(labels, max_id=255):
    """instance_boxes_reference on the device (the statistics launch alone): int32 [max_id + 1, 4]."""
    H, W = labels.shape
    ws = new_workspace(max_id, labels.device)
    _launch(H, W, {}, ws, 0, labels={"instances": _label(labels, H, W)}, max_id=max_id, paint=False)
    return ws[4:4 + 4 * (max_id + 1)].reshape(max_id + 1, 4).clone()


def overlay_instances(rgb_u8, labels, width=6, alpha=0.7, max_id=255):
    """overlay_instances_reference on the device: uint8 [H,W,3] picture, integer labels [H,W] -> uint8 [H,W,3]."""
    H, W = labels.shape
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=labels.device)
    _launch(H, W, {"inst_rgb": out}, new_workspace(max_id, labels.device), 0, rgb=rgb_u8.contiguous(), labels={"instances": _label(labels, H, W)},
            max_id=max_id, width=width, overlay_alpha=alpha)
    return out


class ValidationPictures:
    """Every picture of one validation image in two launches (pc_nerf/trainer.py:710-829).

    render(rb, gts, ...) -> OrderedDict name -> uint8 [H,W,3], views into ONE stack [P,H,W,3] (`self.stack`, P = the pictures these inputs produce, in
    the order of PICTURES).  The stack and the workspace are kept and reused for images of the same shape, so the views of one render() are
    overwritten by the next: copy what must survive.  names(...) tells which pictures a set of inputs produces, without rendering.
    Inputs: rb.rgb f32 [H,W,>=3], rb.depth f32 [H,W,1] or absent, gts f32 [H,W,>=3]; label images int64 / int32 / uint8 [H,W] (or [H,W,1]);
    confidences f32.  max_id: boxes are drawn for ids 1..max_id (save_preds stores uint8, hence 255)."""

    def __init__(self, max_id=255, table=None):
        self.max_id = int(max_id)
        if not 1 <= self.max_id <= _lib.VIS_MAX_ID:
            raise ValueError("max_id %d not in [1, %d]" % (max_id, _lib.VIS_MAX_ID))
        self.table = table
        self.stack = None
        self._planes = self._ws = self._table = None
        self._phase = 0

    @staticmethod
    def names(depth=True, gts=True, semantics=None, instances=None, inst_conf=None, sem_gt=None, inst_gt=None, sem_pred=None, inst_pred=None,
              inst_conf_pred=None):
        """The picture names, in stack order, that render() produces for these inputs (anything that is not None / False counts as present)."""
        return _picture_names(depth, gts, semantics, instances, inst_conf, sem_gt, inst_gt, sem_pred, inst_pred, inst_conf_pred)

    def render(self, rb, gts, semantics=None, instances=None, inst_conf=None, sem_gt=None, inst_gt=None, sem_pred=None, inst_pred=None,
               inst_conf_pred=None):
        rgb = rb.rgb
        H, W = rgb.shape[:2]
        dev = rgb.device
        rgb = rgb.float().contiguous()
        depth = getattr(rb, "depth", None)
        names = _picture_names(depth, gts, semantics, instances, inst_conf, sem_gt, inst_gt, sem_pred, inst_pred, inst_conf_pred)
        if self._planes is None or self._planes.shape[1:3] != (H, W) or self._planes.device != dev:
            self._planes = torch.empty(len(PICTURES), H, W, 3, dtype=torch.uint8, device=dev)
            self._ws, self._phase = new_workspace(self.max_id, dev), 0
            self._table = _gpu_table(self.table, dev)
        self.stack = self._planes[:len(names)]
        outs = OrderedDict((n, self.stack[i]) for i, n in enumerate(names))
        labels = {k: _label(x, H, W) for k, x in zip(_LABELS, (semantics, instances, sem_gt, inst_gt, sem_pred, inst_pred))}
        try:
            _launch(H, W, outs, self._ws, self._phase, rgb=rgb, gt=None if gts is None else gts.float().contiguous(), depth=_f32(depth, (H, W)),
                    labels=labels, conf=(_f32(inst_conf, (H, W)), _f32(inst_conf_pred, (H, W))), table=self._table, max_id=self.max_id)
        except Exception:
            self._planes = None             # a refused launch leaves the workspace's halves in an unknown state: start again
            raise
        self._phase ^= 1
        return outs


# ------------------------------------------------------------------------------------------------------------------------------------- PNG
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, array_u8, level=3):
    """8-bit PNG from a uint8 array [H,W,3] (RGB) or [H,W] / [H,W,1] (grey) with the standard library alone: one IDAT, filter 0 on every row, no
    interlace.  array_u8: numpy array or CPU tensor."""
    a = array_u8.numpy() if isinstance(array_u8, torch.Tensor) else np.asarray(array_u8)
    if a.dtype != np.uint8:
        raise TypeError("write_png: uint8 expected, got %s" % a.dtype)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: [H,W,3] or [H,W] expected, got %s" % (a.shape,))
    H, W = a.shape[:2]
    raw = np.empty((H, 1 + a.size // H), dtype=np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = a.reshape(H, -1)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(_PNG_SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + _chunk(b"IEND", b""))


def read_png(path):
    """The inverse of write_png for its subset (8-bit RGB or grey, no interlace, filter 0 rows): numpy uint8 [H,W,3] or [H,W]."""
    with open(path, "rb") as f:
        blob = f.read()
    if blob[:8] != _PNG_SIGNATURE:
        raise ValueError("%s: not a PNG file" % path)
    pos, idat, head = 8, [], None
    while pos < len(blob):
        n, kind = struct.unpack(">I4s", blob[pos:pos + 8])
        data = blob[pos + 8:pos + 8 + n]
        if struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(kind + data) & 0xffffffff):
            raise ValueError("%s: bad CRC in chunk %r" % (path, kind))
        pos += 12 + n
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif kind == b"IDAT":
            idat.append(data)
        elif kind == b"IEND":
            break
    if head is None or head[2] != 8 or head[3] not in (0, 2) or head[4:] != (0, 0, 0):
        raise ValueError("%s: only 8-bit RGB / grey without interlace is read (IHDR %r)" % (path, head))
    W, H, C = head[0], head[1], 3 if head[3] == 2 else 1
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8).reshape(H, 1 + W * C)
    if raw[:, 0].any():
        raise ValueError("%s: a row filter other than 0" % path)
    out = raw[:, 1:].reshape(H, W, C).copy()
    return out if C == 3 else out[:, :, 0]
