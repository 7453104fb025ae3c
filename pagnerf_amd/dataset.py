"""A device-resident multiview dataset and its ray sampler (datasets/multiview_dataset.py:120-192, datasets/transforms/ray_sampler.py:17-40, the
DataLoader of pc_nerf/trainer.py:216-219): posed, labelled images in, the collated `data` dict of pc_nerf/trainer.py:388-423 out.

The reference draws `torch.randperm(H*W)[:k]` per image (`torch.rand(B, H*W).argsort(1)[:, :k]` in batch mode) in DataLoader workers, indexes every mode
with it and copies the batch to the device.  Here the modes live on the device, and the pixels of a step are the first k entries of a KEYED
PERMUTATION of [0, n) that is evaluated per slot without a table - O(k) instead of O(n log n) - by one launch that also gathers every mode
(csrc/sample.hip).  The contract is the distribution (k pixels of an image without replacement, every k-subset order equally likely up to the quality of
the permutation family), not torch's random stream.

THE DEFINITION is the tensor-op form in this module (`sample_indices`, `DeviceMultiviewDataset.gather`); it serves CPU tensors, and the kernel reproduces
it bit for bit (integers and byte copies only):

    key     s = DOMAIN;  for w in (seed lo32, seed hi32, draw lo32, draw hi32, view):  s = fmix32((s ^ w) + 0x9e3779b9)
            rk[r] = fmix32(s + (r + 1) * 0x9e3779b9),  r = 0 .. 5                      (fmix32: the murmur3 finaliser; all arithmetic mod 2^32)
    round   (L, R) -> (R, L ^ (fmix32(R ^ rk[r]) & (2^h - 1))) on two h-bit halves, 2h = the smallest even width >= max(2, bit_length(n - 1))
    walk    x = slot;  do x = six rounds of x  while x >= n

Six rounds of a balanced Feistel network are a bijection of [0, 2^2h) whatever the round function; following it from a slot < n until it re-enters
[0, n) is a bijection of [0, n) (cycle walking), and terminates because the slot's own cycle returns to it.  2^2h <= 4n, so a slot walks fewer than 4
times on average.  Slot j of (seed, draw, view) is a function of those and n alone: not of k, of the other slots asked for, or of who computes it - a
rank of a sharded step draws its slice (`slots=`) of the single-GPU batch.
"""
import torch

from .core import Rays

ROUNDS = 6
GOLDEN = 0x9E3779B9
DOMAIN_RAYS = 0x52415953        # "RAYS": pixels of a view (csrc/sample.hip carries the same constant)
DOMAIN_EPOCH = 0x45504F43       # "EPOC": the order of the views in an epoch
MAX_PIXELS = 1 << 30
EXCLUDE = ("cameras", "cameras_ts", "filenames")
_M32 = 0xFFFFFFFF


def fmix32(x):
    """The murmur3 finaliser on a Python int (mod 2^32)."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    x ^= x >> 16
    return x


def _mul32(x, c):
    """x * c mod 2^32 on an int64 tensor of uint32 values, without leaving the int64 range."""
    return ((x & 0xFFFF) * c + ((((x >> 16) * c) & 0xFFFF) << 16)) & _M32


def _fmix32_t(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x85EBCA6B)
    x = x ^ (x >> 13)
    x = _mul32(x, 0xC2B2AE35)
    return x ^ (x >> 16)


def round_keys(seed, draw, view, domain=DOMAIN_RAYS):
    """The six round keys of (seed, draw, view): Python ints.  seed and draw are taken as 64-bit two's-complement words, view as a 32-bit one."""
    seed, draw = int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF
    s = domain
    for w in (seed & _M32, seed >> 32, draw & _M32, draw >> 32, int(view) & _M32):
        s = fmix32((s ^ w) + GOLDEN)
    return [fmix32(s + (r + 1) * GOLDEN) for r in range(ROUNDS)]


def half_bits(n):
    """h: the permutation of [0, n) walks a network on 2h bits, the smallest even width >= max(2, bit_length(n - 1))."""
    return (max(2, (int(n) - 1).bit_length()) + 1) // 2


def _network(x, rk, h):
    mask = (1 << h) - 1
    l, r = x >> h, x & mask
    for key in rk:
        l, r = r, l ^ (_fmix32_t(r ^ key) & mask)
    return (l << h) | r


def _check_slots(n, k, slot_begin, slot_count):
    n, k, slot_begin = int(n), int(k), int(slot_begin)
    if not 1 <= n <= MAX_PIXELS:
        raise ValueError("sample_indices: n %d not in [1, 2^30]" % n)
    if k < 1:
        raise ValueError("sample_indices: k %d < 1" % k)
    take = min(k, n)                                   # randperm(n)[:k] yields n rows when k > n
    slot_count = take - slot_begin if slot_count is None else int(slot_count)
    if slot_begin < 0 or slot_count < 0 or slot_begin + slot_count > take:
        raise ValueError("sample_indices: slots [%d, %d) outside [0, min(k, n) = %d)" % (slot_begin, slot_begin + slot_count, take))
    return n, take, slot_begin, slot_count


def _word64(v, device):
    """A seed / draw / view (Python int of any sign, or an integer tensor of them) as an int64 tensor of 64-bit two's-complement words."""
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=torch.int64)
    if isinstance(v, (list, tuple)):
        return torch.stack([_word64(w, device) for w in v]) if len(v) else torch.empty(0, dtype=torch.int64, device=device)
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor(v - (1 << 64) if v >> 63 else v, dtype=torch.int64, device=device)


def _round_keys_t(seed, draw, view, domain, device):
    """round_keys() on tensors: seed, draw and view broadcast against each other; six int64 tensors of uint32 values."""
    seed, draw, view = torch.broadcast_tensors(_word64(seed, device), _word64(draw, device), _word64(view, device))
    s = torch.full_like(seed, domain)
    for w in (seed & _M32, (seed >> 32) & _M32, draw & _M32, (draw >> 32) & _M32, view & _M32):
        s = _fmix32_t(((s ^ w) + GOLDEN) & _M32)
    return [_fmix32_t((s + (r + 1) * GOLDEN) & _M32) for r in range(ROUNDS)]


def sample_indices(n, k, seed, draw, view, slot_begin=0, slot_count=None, device=None, domain=DOMAIN_RAYS):
    """Slots slot_begin .. slot_begin + slot_count of the first min(k, n) entries of the keyed permutation of [0, n): int64 [slot_count].
    seed, draw and view are ints; any of them may also be a list or an integer tensor [B] (they broadcast): the result is then [B, slot_count], row b
    being the draw of the b-th key."""
    n, _, slot_begin, slot_count = _check_slots(n, k, slot_begin, slot_count)
    h = half_bits(n)
    rk = _round_keys_t(seed, draw, view, domain, device)
    single = rk[0].dim() == 0
    rk = [r.reshape(-1) for r in rk]
    rows = rk[0].shape[0]
    slots = torch.arange(slot_begin, slot_begin + slot_count, dtype=torch.int64, device=device)
    x = _network(slots.expand(rows, slot_count), [r[:, None] for r in rk], h).reshape(-1)
    todo = (x >= n).nonzero().reshape(-1)              # cycle walking: only the slots still outside [0, n) go round again
    while todo.numel():
        row = todo // slot_count
        y = _network(x[todo], [r[row] for r in rk], h)
        x[todo] = y
        todo = todo[y >= n]
    return x if single else x.reshape(rows, slot_count)


def epoch_views(num_views, batch_size, seed, epoch, drop_last=False):
    """The view batches of one epoch, as DataLoader(shuffle=True, batch_size=) deals them (pc_nerf/trainer.py:216-219): the keyed permutation of
    [0, num_views) under (seed, epoch) - its own key domain - cut into consecutive batches, the last one short unless drop_last.  Host side: list of
    int64 CPU tensors."""
    if batch_size < 1:
        raise ValueError("epoch_views: batch_size %d < 1" % batch_size)
    order = sample_indices(num_views, num_views, seed, epoch, 0, domain=DOMAIN_EPOCH)
    batches = list(order.split(int(batch_size)))
    if drop_last and batches and batches[-1].numel() < batch_size:
        batches.pop()
    return batches


def _u8_table(device):
    """u / 255 for u = 0 .. 255 in IEEE float32 division, computed on the CPU whatever the device: a device's `x / 255` may multiply by the rounded
    reciprocal instead, which differs in the last bit for some u.  The kernel divides ((float)u / 255.0f, correctly rounded)."""
    return (torch.arange(256, dtype=torch.float32) / 255).to(device)


def _is_rays(v):
    return hasattr(v, "origins") and hasattr(v, "dirs")


class _Leaf:
    """One gathered array: a tensor mode, or one field of a Rays mode."""

    def __init__(self, key, field, src, per_view, convert=0):
        self.key, self.field, self.src, self.per_view, self.convert = key, field, src, per_view, convert
        self.channels = src.shape[-1]
        self.dtype = torch.float32 if convert else src.dtype
        self.row_bytes = self.channels * (4 if convert else src.element_size())        # of a destination row


class DeviceMultiviewDataset:
    """The dict MultiviewDataset.init() builds (datasets/multiview_dataset.py:120-132), moved to `device` once.

    data: every mode a tensor [V, H*W, C] or [V, H, W, C] (reshaped as :125-132 does: the last axis is the channel axis); 'rays' a Rays with [V, H*W, 3]
    (or [V, H, W, 3]) fields; 'base_rays' a Rays or a tensor [H*W, 3] (or [H, W, 3]) shared by the views; the keys in `exclude` are left out.
    store_uint8: float32 modes kept as uint8 (a quarter of the memory) and handed out as `u / 255` - accepted only if that reproduces every element.

    sample() returns the collated batch of pc_nerf/trainer.py:396-422; on a CUDA device it is one pag_sample_batch launch (two beyond 12 arrays), on the
    CPU - or with `use_kernel = False` - the tensor-op form, and the two return the same bits.  `state` is the device int64 [2] = {seed, draw} the kernel
    reads, and the tensor-op form on a CUDA device reads it too (a synchronisation); `draw` is its host mirror (no synchronisation) and does not see the
    advances of a replayed graph - re-seed with seed(seed, draw) after replays if the mirror is needed.  A view outside [0, V) in a DEVICE views
    tensor gives zero rows and ray_idx -1 in both forms; views that come from the host are refused there (IndexError)."""

    def __init__(self, data, device, exclude=EXCLUDE, store_uint8=(), shared=("base_rays",)):
        self.device = torch.device(device)
        self.exclude = tuple(exclude)
        keys = [k for k in data if k not in self.exclude]
        per_view = [k for k in keys if k not in shared]
        if not per_view:
            raise ValueError("DeviceMultiviewDataset: no per-view mode in %r" % (list(data),))
        first = data["imgs"] if "imgs" in keys else data[per_view[0]]
        self.num_imgs = int((first.origins if _is_rays(first) else first).shape[0])
        self.modes, self._leaves, self._rays_range = keys, [], {}
        n = None
        for k in keys:
            v = data[k]
            is_shared = k in shared
            if k in store_uint8 and (_is_rays(v) or v.dtype != torch.float32):
                raise ValueError("DeviceMultiviewDataset: store_uint8 takes float32 tensor modes, %r is not one" % k)
            if _is_rays(v):
                self._rays_range[k] = (getattr(v, "dist_min", 0.0), getattr(v, "dist_max", 6.0))
                fields = [("origins", v.origins), ("dirs", v.dirs)]
            else:
                fields = [(None, v)]
            for field, t in fields:
                if is_shared:
                    t = t.reshape(-1, t.shape[-1])
                else:
                    if t.dim() < 3 or t.shape[0] != self.num_imgs:
                        raise ValueError("DeviceMultiviewDataset: mode %r has shape %s, expected [%d, H*W, C] or [%d, H, W, C]"
                                         % (k, tuple(t.shape), self.num_imgs, self.num_imgs))
                    t = t.reshape(self.num_imgs, -1, t.shape[-1])
                if n is None:
                    n = t.shape[-2]
                if t.shape[-2] != n or t.shape[-1] < 1:
                    raise ValueError("DeviceMultiviewDataset: mode %r has %d pixels per view, the others %d" % (k, t.shape[-2], n))
                convert = 0
                if k in store_uint8:
                    t, convert = self._quantise(k, t), 1
                self._leaves.append(_Leaf(k, field, t.detach().to(self.device).contiguous(), not is_shared, convert))
        if not 1 <= n <= MAX_PIXELS:
            raise ValueError("DeviceMultiviewDataset: %d pixels per view not in [1, 2^30]" % n)
        self.num_pixels = int(n)
        self.use_kernel = True
        self._seed, self.draw = 0, 0
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)

    @staticmethod
    def _quantise(key, t):
        q = torch.round(t * 255.0).clamp(0, 255).long()
        if not torch.equal(_u8_table(t.device)[q], t):
            raise ValueError("DeviceMultiviewDataset: store_uint8 mode %r is not exactly round(x * 255) / 255" % key)
        return q.to(torch.uint8)

    def __len__(self):
        return self.num_imgs

    @property
    def nbytes(self):
        return sum(l.src.numel() * l.src.element_size() for l in self._leaves)

    def source(self, key, field=None):
        """The stored array of mode `key` (`field` 'origins' / 'dirs' of a Rays mode) on the device - [V, H*W, C], a shared mode [H*W, C] - or None when
        the dataset has no such mode.  What a pass over whole images reads (the depth carve); a uint8-stored mode comes as stored."""
        return next((l.src for l in self._leaves if l.key == key and l.field == field), None)

    def rays_range(self, key):
        """(dist_min, dist_max) of the Rays mode `key`."""
        return self._rays_range[key]

    # ------------------------------------------------------------------------------------------------------------------ state
    def seed(self, seed, draw=0):
        """Start the stream of (seed, draw): an asynchronous 16-byte copy on a CUDA device."""
        self._seed, self.draw = int(seed), int(draw)
        host = torch.tensor([self._seed, self.draw], dtype=torch.int64)
        if self.device.type == "cuda":
            self.state.copy_(host.pin_memory(), non_blocking=True)
        else:
            self.state.copy_(host)
        return self

    def advance(self):
        """The next draw: state[1] += 1 on the device (a launch a graph can capture), and the host mirror."""
        if self.device.type == "cuda":
            from . import ops
            ops.sample_advance(self.state)
        else:
            self.state[1] += 1
        self.draw += 1

    # ------------------------------------------------------------------------------------------------------------------ batches
    def _views(self, views):
        """-> the views as an index tensor on the device: int32 on CUDA, int64 on the CPU; checked on the host when they come from there."""
        if isinstance(views, torch.Tensor) and views.device.type == "cuda":
            if views.device != self.device:
                raise ValueError("DeviceMultiviewDataset: views on %s, dataset on %s" % (views.device, self.device))
            return views.reshape(-1).to(torch.int32).contiguous()
        host = torch.as_tensor(views, dtype=torch.int64).reshape(-1)
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= self.num_imgs):
            raise IndexError("DeviceMultiviewDataset: view outside [0, %d)" % self.num_imgs)
        if self.device.type == "cuda":
            return host.to(torch.int32).pin_memory().to(self.device, non_blocking=True)
        return host

    def empty_batch(self, batch_size, num_samples, ray_idx=False, slots=None):
        """The buffers sample(..., out=) fills: reuse them across steps, or capture a graph over them."""
        count = _check_slots(self.num_pixels, num_samples, *(slots or (0, None)))[3]
        out = {}
        for l in self._leaves:
            t = torch.empty(batch_size, count, l.channels, dtype=l.dtype, device=self.device)
            if l.field is None:
                out[l.key] = t
            else:
                r = out.setdefault(l.key, Rays(None, None, *self._rays_range[l.key]))
                setattr(r, l.field, t)
        out["cam_id"] = torch.empty(batch_size, dtype=torch.int32 if self.device.type == "cuda" else torch.int64, device=self.device)
        out["cam_idx"] = torch.empty(batch_size * count, dtype=torch.int32, device=self.device)
        if ray_idx:
            out["ray_idx"] = torch.empty(batch_size, count, dtype=torch.int64, device=self.device)
        return out

    @staticmethod
    def _leaf_out(out, leaf):
        v = out[leaf.key]
        return v if leaf.field is None else getattr(v, leaf.field)

    def sample(self, views, num_samples, out=None, slots=None, ray_idx=False):
        """min(num_samples, H*W) pixels of each of `views` (host ints, or a device int32 tensor [B]; repeats allowed) under the current (seed, draw):
        every mode [B, k, C], 'rays' / 'base_rays' as Rays with [B, k, 3] fields, cam_id = the views, cam_idx int32 [B * k] = the view of each ray
        (BAPipeline.transform_rays_indexed takes it), ray_idx int64 [B, k] on request.  slots=(begin, count): that slice of the k slots only.
        out: a dict from empty_batch() / an earlier call, filled in place.  Does not advance the draw."""
        n = self.num_pixels
        _, k, begin, count = _check_slots(n, num_samples, *(slots or (0, None)))
        ray_idx = ray_idx or (out is not None and "ray_idx" in out)
        v = self._views(views)
        B = v.shape[0]
        if self.device.type != "cuda" or not self.use_kernel:
            vl, bad, seed, draw = v.long(), None, self._seed, self.draw
            if self.device.type == "cuda":
                seed, draw = self.state.tolist()           # what the kernel would read (replayed graphs advance it behind the host mirror); waits
                bad = (vl < 0) | (vl >= self.num_imgs)      # device views are not checked on the host: the kernel's answer to them, below
            idx = sample_indices(n, k, seed, draw, vl, begin, count, device=self.device)
            res = self.gather(vl if bad is None else vl.clamp(0, self.num_imgs - 1), idx, ray_idx=ray_idx)
            if bad is not None:                             # zero rows and ray_idx -1 for a view outside the dataset; cam_id / cam_idx carry it
                for key, val in res.items():
                    for t in ((val.origins, val.dirs) if _is_rays(val) else (val,)):
                        if key == "ray_idx":
                            t[bad] = -1
                        elif key not in ("cam_id", "cam_idx"):
                            t[bad] = 0
                res["cam_id"] = vl.to(torch.int32)
                res["cam_idx"] = vl[:, None].expand(B, count).reshape(-1).to(torch.int32)
            if out is None:
                return res
            for key, val in res.items():
                if _is_rays(val):
                    out[key].origins.copy_(val.origins)
                    out[key].dirs.copy_(val.dirs)
                else:
                    out[key].copy_(val)
            return out
        from . import ops
        if out is None:
            out = self.empty_batch(B, k, ray_idx=ray_idx, slots=(begin, count))
            out["cam_id"] = v
        elif out["cam_id"].data_ptr() != v.data_ptr():
            out["cam_id"].copy_(v, non_blocking=True)
        ridx, cidx = out.get("ray_idx"), out["cam_idx"]
        if cidx.numel() != B * count or (ridx is not None and ridx.numel() != B * count):
            raise ValueError("DeviceMultiviewDataset.sample: out= was made for another batch shape")
        for i in range(0, max(1, len(self._leaves)), 12):
            chunk = self._leaves[i:i + 12]
            modes = []
            for l in chunk:
                dst = self._leaf_out(out, l)
                if dst.shape != (B, count, l.channels) or dst.dtype != l.dtype:
                    raise ValueError("DeviceMultiviewDataset.sample: out[%r] is %s %s, expected %s %s"
                                     % (l.key, tuple(dst.shape), dst.dtype, (B, count, l.channels), l.dtype))
                modes.append((l.src, dst, l.row_bytes, l.per_view, l.convert))
            ops.sample_batch(self.state, v, self.num_imgs, n, k, begin, count, modes, ray_idx=ridx if i == 0 else None, cam_idx=cidx if i == 0 else None)
        return out

    def gather(self, views, idx, ray_idx=False):
        """The gather and collation alone, as tensor ops: rows idx int64 [B, k] of views [B] of every mode -> the batch dict sample() returns.  This is
        the definition the kernel's copies are held to; the reference's own SampleRays output is reproduced from its indices (tests/golden/g18)."""
        views = torch.as_tensor(views, dtype=torch.int64, device=self.device).reshape(-1)
        idx = torch.as_tensor(idx, dtype=torch.int64, device=self.device)
        out = {}
        for l in self._leaves:
            t = l.src[views[:, None], idx] if l.per_view else l.src[idx]
            if l.convert:
                t = _u8_table(self.device)[t.long()]
            t = t.contiguous()
            if l.field is None:
                out[l.key] = t
            else:
                r = out.setdefault(l.key, Rays(None, None, *self._rays_range[l.key]))
                setattr(r, l.field, t)
        out["cam_id"] = views.to(torch.int32) if self.device.type == "cuda" else views
        out["cam_idx"] = views[:, None].expand(idx.shape).reshape(-1).to(torch.int32)
        if ray_idx:
            out["ray_idx"] = idx.clone()
        return out


class BatchSampler:
    """One epoch of training batches: DataLoader(dataset, batch_size, shuffle=True) + SampleRays(num_samples) of pc_nerf/trainer.py:216-219 on a
    DeviceMultiviewDataset.  Item i is ds.sample(epoch_views(...)[i], num_samples), followed by ds.advance().  The epoch's view batches go to the
    device once, through a pinned buffer and an asynchronous copy; an iteration never waits for the device."""

    def __init__(self, ds, batch_size, num_samples, seed=0, drop_last=False, ray_idx=False):
        if batch_size < 1:
            raise ValueError("BatchSampler: batch_size %d < 1" % batch_size)
        self.ds, self.batch_size, self.num_samples, self.drop_last, self.ray_idx = ds, int(batch_size), int(num_samples), drop_last, ray_idx
        self.seed, self.epoch = int(seed), 0
        ds.seed(seed)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        V = self.ds.num_imgs
        return V // self.batch_size if self.drop_last else (V + self.batch_size - 1) // self.batch_size

    def views(self):
        return epoch_views(self.ds.num_imgs, self.batch_size, self.seed, self.epoch, self.drop_last)

    def __iter__(self):
        batches = self.views()
        self.epoch += 1
        if not batches:
            return
        if self.ds.device.type == "cuda":
            flat = torch.cat(batches).to(torch.int32).pin_memory().to(self.ds.device, non_blocking=True)
            batches = list(flat.split(self.batch_size))
        for v in batches:
            batch = self.ds.sample(v, self.num_samples, ray_idx=self.ray_idx)
            self.ds.advance()
            yield batch


class SampleRays:
    """The reference's transform (datasets/transforms/ray_sampler.py) for a dict of DEVICE tensors, in its two modes (:20-31): a single image - every
    mode [H*W, C], `rays` of shape [H*W] - yields num_samples rows per mode; a batch - modes [B, H*W, C] - yields num_samples // B rows per image,
    [B, k, C].  A mode without the batch axis ([H*W, C], e.g. base_rays) is shared by the images.  Every call is one draw of the stream `seed`.
    A compatibility shim, not the fast path: each call wraps its inputs in a DeviceMultiviewDataset (shape checks per mode, a 16-byte state copy and a
    views copy through pinned memory) for one draw; a training loop holds a DeviceMultiviewDataset and uses BatchSampler or sample()."""

    def __init__(self, num_samples, seed=0, exclude=EXCLUDE):
        self.num_samples, self.seed, self.exclude, self.draw = int(num_samples), int(seed), tuple(exclude), 0

    def __call__(self, inputs):
        rays = inputs["rays"]
        shape = _lead(rays)
        if len(shape) not in (1, 2):
            raise NotImplementedError("raysampling only implemented for single image and batch")
        single = len(shape) == 1
        batch = 1 if single else shape[0]
        data, shared = {}, []
        for k, v in inputs.items():
            if k in self.exclude:
                continue
            if single:                                                       # one image: a dataset of one view
                data[k] = Rays(v.origins[None], v.dirs[None], getattr(v, "dist_min", 0.0), getattr(v, "dist_max", 6.0)) if _is_rays(v) else v[None]
            else:
                data[k] = v
                if _lead(v) != shape:                                 # no batch axis ([H*W, C], e.g. base_rays): shared by the images
                    shared.append(k)
        if not single and self.num_samples // batch < 1:
            raise ValueError("SampleRays: num_samples %d gives no ray per image for a batch of %d images" % (self.num_samples, batch))
        ds = DeviceMultiviewDataset(data, (rays.origins if _is_rays(rays) else rays).device, exclude=(), shared=tuple(shared))
        ds.seed(self.seed, self.draw)
        self.draw += 1
        out = ds.sample(list(range(batch)), self.num_samples if single else self.num_samples // batch)
        for k in ("cam_id", "cam_idx"):
            del out[k]
        if single:
            out = {k: (Rays(v.origins[0], v.dirs[0], v.dist_min, v.dist_max) if _is_rays(v) else v[0]) for k, v in out.items()}
        return out


def _lead(v):
    """The axes in front of the channel axis."""
    return tuple((v.origins if _is_rays(v) else v).shape[:-1])
