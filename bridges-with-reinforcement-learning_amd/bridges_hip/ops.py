"""Thin host wrappers of the stand-alone HIP operators (single calls on caller-shaped batches).

Used by the single-environment ``assembly_gym`` API; every function launches a kernel of
libbridges_hip.so on the current torch stream and returns device tensors."""
import ctypes as C

import numpy as np
import torch

from . import abi
from .shapes import ShapeGeometry

_tables = {}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_stream = abi.current_stream


class ShapeRegistry:
    """Process-wide device table of every ShapeGeometry seen so far (ids are stable)."""

    def __init__(self):
        self.geoms = []
        self._dev = None
        self._dev_count = 0

    def id_of(self, geom: ShapeGeometry):
        for i, g in enumerate(self.geoms):
            if g is geom:
                return i
        self.geoms.append(geom)
        return len(self.geoms) - 1

    def device_table(self):
        L = abi.require_gpu()
        if self._dev is None or self._dev_count != len(self.geoms):
            if self._dev is not None:
                L.bridges_shapes_free(self._dev)
            arr = (abi.Shape * len(self.geoms))(*[g.to_struct() for g in self.geoms])
            dev = C.c_void_p()
            abi.check(L.bridges_shapes_upload(arr, len(self.geoms), C.byref(dev)), "bridges_shapes_upload")
            self._dev, self._dev_count = dev, len(self.geoms)
        return self._dev


REGISTRY = ShapeRegistry()


class _TorchDtypes(dict):
    def __missing__(self, dt):                              # any other numpy dtype torch has a name for
        self[dt] = getattr(torch, np.dtype(dt).name)
        return self[dt]


_TORCH_DTYPE = _TorchDtypes({np.dtype(n): getattr(torch, n) for n in ("float32", "float64", "int32", "int64", "uint8", "int8", "int16", "bool")})


class _Stager:
    """Small host arrays -> device tensors through ONE pinned staging buffer and ONE asynchronous copy per call.

    ``torch.tensor(array, device=...)`` of pageable memory is a blocking copy: the host waits for everything queued on the
    stream before it.  An operator of the single-environment API takes three to seven such arrays (stability: poses,
    vertices, shape ids, count, frozen mask), i.e. as many host waits per call -- 30 of the ~50 waits of one env-step of the
    reference-style loop.  Here the arrays are packed (16-byte aligned) into one of a ring of pinned buffers, copied with one
    non-blocking transfer, and handed out as typed views of one device buffer; a slot is reused only after the event
    recorded behind its copy has passed."""
    SLOTS, MIN_BYTES = 16, 1 << 16

    def __init__(self):
        self.slots, self.turn = [], 0

    def upload(self, dev, *arrays):
        arrays = [a if a.flags.c_contiguous else np.ascontiguousarray(a) for a in arrays]
        offs, total = [], 0
        for a in arrays:
            offs.append(total)
            total += -(-max(a.nbytes, 1) // 16) * 16
        if len(self.slots) < self.SLOTS:
            pinned = torch.empty(max(total, self.MIN_BYTES), dtype=torch.uint8).pin_memory()
            self.slots.append([pinned, torch.cuda.Event(), pinned.numpy()])     # buffer, "copy done" event, numpy view
            slot = self.slots[-1]
        else:
            slot = self.slots[self.turn]
            self.turn = (self.turn + 1) % self.SLOTS
            slot[1].synchronize()                           # (passed long ago unless 16 uploads are in flight)
            if slot[0].numel() < total:
                slot[0] = torch.empty(total, dtype=torch.uint8).pin_memory()
                slot[2] = slot[0].numpy()
        host = slot[2]
        for a, off in zip(arrays, offs):
            host[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
        d = torch.empty(total, dtype=torch.uint8, device=dev)
        d.copy_(slot[0][:total], non_blocking=True)
        slot[1].record()
        if len(arrays) == 1:
            a = arrays[0]
            return [d[:a.nbytes].view(_TORCH_DTYPE[a.dtype]).reshape(a.shape)]
        return [d[off:off + a.nbytes].view(_TORCH_DTYPE[a.dtype]).reshape(a.shape) for a, off in zip(arrays, offs)]


_STAGER = _Stager()


def upload(dev, *arrays):
    """numpy arrays (any dtypes) -> device tensors of the same shapes, one pinned staging copy for all of them."""
    return _STAGER.upload(dev, *arrays)


def download(*tensors):
    """Device tensors -> numpy arrays with ONE device-to-host copy (one host wait): they are packed into a float64 buffer on
    the device first (integer and byte tensors are exact in float64 here: counts, flags, small ids)."""
    flat = torch.cat([t.reshape(-1).to(torch.float64) for t in tensors])
    host = flat.cpu().numpy()
    out, off = [], 0
    for t in tensors:
        n = t.numel()
        a = host[off:off + n].reshape(tuple(t.shape))
        off += n
        out.append(a if t.dtype == torch.float64 else a.astype(np.dtype(str(t.dtype).replace("torch.", ""))))
    return out


_grids = {}


def pixel_grid(dev, xlim, ylim, S):
    """(grid_x, grid_y) of render_blocks_2d on the device, cached per (device, limits, size)."""
    key = (str(dev), float(xlim[0]), float(xlim[1]), float(ylim[0]), float(ylim[1]), int(S))
    g = _grids.get(key)
    if g is None:
        if len(_grids) > 64:
            _grids.clear()
        g = _grids[key] = tuple(upload(dev, np.linspace(xlim[0], xlim[1], S), np.linspace(ylim[1], ylim[0], S)))
    return g


def device():
    abi.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def place(frame1, geom, face, ox, oy):
    """create_block / align_frames_2d (gym_env.py:204-216, geometry.py:39-50) for ONE placement.
    frame1 = (cx, cz, tx, tz, nx, nz).  Returns (pose[4], verts[nv,2]) as float64 numpy arrays."""
    L = abi.require_gpu()
    dev = device()
    sid = REGISTRY.id_of(geom)
    tab = REGISTRY.device_table()
    f1, sh, fc, oxs, oys = upload(dev, np.array([list(frame1)], dtype=np.float64), np.array([sid], dtype=np.int32),
                                  np.array([int(face)], dtype=np.int32), np.array([float(ox)]), np.array([float(oy)]))
    pose = torch.empty((1, 4), dtype=torch.float64, device=dev)
    verts = torch.empty((1, 6, 2), dtype=torch.float64, device=dev)
    abi.check(L.bridges_place(tab, 1, _ptr(f1), _ptr(sh), _ptr(fc), _ptr(oxs), _ptr(oys), _ptr(pose), _ptr(verts),
                              _stream()), "bridges_place")
    pose_h, verts_h = download(pose, verts)
    return pose_h[0], verts_h[0, :len(geom.verts)]


def image_size(img_size):
    """-> S of an S x S image the rasteriser renders (2 <= S <= 64, one wave lane per pixel column)."""
    w, h = (int(v) for v in img_size)
    if w != h or not 2 <= w <= 64:
        raise NotImplementedError(f"the HIP rasteriser renders square images of 2..64 pixels, not {w}x{h} "
                                  "(successor_dqn.py:585 default: 64x64)")
    return w


def crop(images, img_size):
    """[..., 64, 64] canvas -> the [..., S, S] image in its top-left corner (no-op for 64x64)."""
    S = image_size(img_size)
    return images if S == 64 else images[..., :S, :S]


def raster_bits(blocks, xlim, ylim, img_size=(64, 64)):
    """One bit raster per posed block: int64 [n,64] on the device (rendering.py:105-113 per block).  For S x S
    images with S < 64 the words / bits >= S are zero."""
    S = image_size(img_size)
    L = abi.require_gpu()
    dev = device()
    n = len(blocks)
    if n == 0:
        return torch.zeros((0, 64), dtype=torch.int64, device=dev)
    verts = np.zeros((n, 6, 2))
    ids = np.zeros(n, dtype=np.int32)
    for i, b in enumerate(blocks):
        verts[i, :len(b.verts_2d)] = b.verts_2d
        ids[i] = REGISTRY.id_of(b.geometry)
    tab = REGISTRY.device_table()
    v, s = upload(dev, verts, ids)
    gx, gy = pixel_grid(dev, xlim, ylim, S)
    bits = torch.empty((n, 64), dtype=torch.int64, device=dev)
    abi.check(L.bridges_raster_sized(tab, n, _ptr(v), _ptr(s), _ptr(gx), _ptr(gy), S, _ptr(bits), None, _stream()),
              "bridges_raster")
    return bits


def render_blocks(blocks, xlim, ylim, img_size):
    """render_blocks_2d at any image size (bridges_render_blocks): the union of the posed blocks on the grid
    X = linspace(xlim, img_size[0]), Y = linspace(ylim[1], ylim[0], img_size[1]) -> uint8 [img_size[1], img_size[0]] (rows
    top to bottom) on the device."""
    L = abi.require_gpu()
    dev = device()
    W, H = int(img_size[0]), int(img_size[1])
    if W < 1 or H < 1:
        raise ValueError(f"image size {img_size}")
    n = len(blocks)
    verts = np.zeros((max(n, 1), 6, 2))
    ids = np.zeros(max(n, 1), dtype=np.int32)
    for i, b in enumerate(blocks):
        verts[i, :len(b.verts_2d)] = b.verts_2d
        ids[i] = REGISTRY.id_of(b.geometry)
    tab = REGISTRY.device_table()
    v, s, gx, gy = upload(dev, verts, ids, np.linspace(xlim[0], xlim[1], W), np.linspace(ylim[1], ylim[0], H))
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    abi.check(L.bridges_render_blocks(tab, n, _ptr(v), _ptr(s), _ptr(gx), W, _ptr(gy), H, _ptr(out), _stream()), "bridges_render_blocks")
    return out


def reward_prefix(reward_map):
    """float64 row prefix sums [64, 65] of a reward map ([64,64] f32 tensor), accumulated left to right on the host: what
    bridges_action_features takes the linear reward of a candidate from (build it once per task)."""
    pre = np.zeros((64, 65), dtype=np.float64)
    pre[:, 1:] = np.cumsum(reward_map.detach().cpu().numpy().astype(np.float64).reshape(64, 64), axis=1)
    return upload(device(), pre)[0]                        # the kernel's table: on the GPU whatever device the map is on


def action_features(blocks, xlim, ylim, state_bits=None, obstacle_bits=None, reward_map=None, img_size=(64, 64), want_f32=False,
                    prefix=None):
    """bridges_action_features for a list of posed candidate blocks against one state: -> (bits [n,64] int64, img
    [n,64,64] f32 or None, mask [n] bool, lin [n] f32 or None) on the device.  state_bits / obstacle_bits: [64] int64 bit
    rasters (None = empty); reward_map: [64,64] f32 tensor (None: no linear reward) or ``prefix`` = reward_prefix(map),
    built once."""
    S = image_size(img_size)
    L = abi.require_gpu()
    dev = device()
    n = len(blocks)
    bits = torch.empty((n, 64), dtype=torch.int64, device=dev)
    img = torch.empty((n, 64, 64), dtype=torch.float32, device=dev) if want_f32 else None
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    lin = torch.zeros(n, dtype=torch.float32, device=dev) if (reward_map is not None or prefix is not None) else None
    if n == 0:
        return bits, img, mask.bool(), lin
    verts = np.zeros((n, 6, 2))
    ids = np.zeros(n, dtype=np.int32)
    for i, b in enumerate(blocks):
        verts[i, :len(b.verts_2d)] = b.verts_2d
        ids[i] = REGISTRY.id_of(b.geometry)
    tab = REGISTRY.device_table()
    v, s_ = upload(dev, verts, ids)
    gx, gy = pixel_grid(dev, xlim, ylim, S)
    if prefix is None and reward_map is not None:
        prefix = reward_prefix(reward_map)
    abi.check(L.bridges_action_features(tab, n, _ptr(v), _ptr(s_), _ptr(gx), _ptr(gy), S, float(xlim[0]), float(xlim[1]),
                                        float(ylim[0]), float(ylim[1]), _ptr(state_bits), _ptr(obstacle_bits), _ptr(prefix),
                                        _ptr(bits), _ptr(img), _ptr(mask), _ptr(lin), _stream()), "bridges_action_features")
    return bits, img, mask.bool(), lin


def bits_or(bits):
    L = abi.require_gpu()
    dev = bits.device
    out = torch.zeros(64, dtype=torch.int64, device=dev)
    if bits.shape[0] == 0:
        return out
    off, = upload(dev, np.array([0, bits.shape[0]], dtype=np.int32))
    abi.check(L.bridges_bits_or(1, _ptr(off), _ptr(bits), _ptr(out), _stream()), "bridges_bits_or")
    return out


def bits_to_f32(bits):
    """[n,64] int64 -> [n,64,64] float32 {0,1}."""
    L = abi.require_gpu()
    bits = bits.reshape(-1, 64).contiguous()
    img = torch.empty((bits.shape[0], 64, 64), dtype=torch.float32, device=bits.device)
    if bits.shape[0]:
        abi.check(L.bridges_bits_to_f32(bits.shape[0], _ptr(bits), _ptr(img), _stream()), "bridges_bits_to_f32")
    return img


def bits_discounted_sum(bits, first, h, gamma, want_sum=True):
    """The discounted sum of consecutive block rasters (bridges_bits_discounted_sum): bits [R, 64] int64, first [B] int64 and
    h [B] int32 (1..abi.NSTEP_MAX) -> (sum [B, 64, 64] float32, disc [B] float32) with
    sum[i] = sum_{k < h[i]} d_k * image(bits[first[i] + k]) and disc[i] = d_{h[i]}, d_0 = 1, d_{k+1} = d_k * gamma in float32;
    h = 1 everywhere gives bits_to_f32(bits[first]) bit for bit.  want_sum=False: (None, disc)."""
    L = abi.require_gpu()
    bits = bits.reshape(-1, 64)
    assert bits.is_contiguous() and bits.dtype == torch.int64
    first = first.to(torch.int64).contiguous()
    h = h.to(torch.int32).contiguous()
    B = first.numel()
    assert h.numel() == B
    img = torch.empty((B, 64, 64), dtype=torch.float32, device=bits.device) if want_sum else None
    disc = torch.empty(B, dtype=torch.float32, device=bits.device)
    if B:
        abi.check(L.bridges_bits_discounted_sum(B, _ptr(bits), bits.shape[0], _ptr(first), _ptr(h), float(gamma), _ptr(img), _ptr(disc),
                                                _stream()), "bridges_bits_discounted_sum")
    return img, disc


def bits_linear(bits, wt, bits_row=None, base=None, base_row=None):
    """out[r] = base[base_row[r]] + sum of the rows of ``wt`` ([4096, d], pixel-major) selected by the set pixels of the
    bit-packed raster ``bits[bits_row[r]]`` ([*,64] int64): a linear layer applied to flattened binary images without
    expanding them (bridges_bits_linear).  Returns [n, d] float32."""
    L = abi.require_gpu()
    bits = bits.reshape(-1, 64)
    assert bits.is_contiguous() and bits.dtype == torch.int64
    wt = wt.to(torch.float32).contiguous()
    assert wt.shape[0] == 4096 and wt.shape[1] % 4 == 0, "wt must be [4096, d] with d % 4 == 0"
    d = wt.shape[1]
    n = bits_row.numel() if bits_row is not None else bits.shape[0]
    if bits_row is not None:
        bits_row = bits_row.to(torch.int64).contiguous()
    if base is not None:
        base = base.to(torch.float32).reshape(-1, d).contiguous()
        if base_row is not None:
            base_row = base_row.to(torch.int64).contiguous()
            assert base_row.numel() == n
    out = torch.empty((n, d), dtype=torch.float32, device=bits.device)
    abi.check(L.bridges_bits_linear(n, _ptr(bits), _ptr(bits_row), _ptr(wt), d, _ptr(base), _ptr(base_row), _ptr(out),
                                    _stream()), "bridges_bits_linear")
    return out


def bits_linear2(bits_a, wt_a, bits_b, wt_b, bits_row_a=None, bits_row_b=None, base=None, base_row=None):
    """bits_linear over two bit-packed operands in one launch (bridges_bits_linear2):
    out[r] = base[base_row[r]] + sum of the rows of ``wt_a`` selected by ``bits_a[bits_row_a[r]]`` + sum of the rows of ``wt_b``
    selected by ``bits_b[bits_row_b[r]]``, added in that order -- bit for bit
    ``bits_linear(bits_b, wt_b, bits_row_b, base=bits_linear(bits_a, wt_a, bits_row_a, base, base_row))``.  Returns [n, d] float32;
    n = the length of a row index that is given, else the rows of ``bits_a``."""
    L = abi.require_gpu()
    bits_a, bits_b = bits_a.reshape(-1, 64), bits_b.reshape(-1, 64)
    assert bits_a.is_contiguous() and bits_a.dtype == torch.int64 and bits_b.is_contiguous() and bits_b.dtype == torch.int64
    wt_a, wt_b = wt_a.to(torch.float32).contiguous(), wt_b.to(torch.float32).contiguous()
    assert wt_a.shape[0] == 4096 and wt_a.shape[1] % 4 == 0 and wt_b.shape == wt_a.shape, "wt_a / wt_b must be [4096, d] with d % 4 == 0"
    d = wt_a.shape[1]
    n = bits_row_a.numel() if bits_row_a is not None else bits_a.shape[0]
    if bits_row_a is not None:
        bits_row_a = bits_row_a.to(torch.int64).contiguous()
    if bits_row_b is not None:
        bits_row_b = bits_row_b.to(torch.int64).contiguous()
        assert bits_row_b.numel() == n
    else:
        assert bits_b.shape[0] >= n, f"{bits_b.shape[0]} rasters in bits_b for {n} rows"
    if base is not None:
        base = base.to(torch.float32).reshape(-1, d).contiguous()
        if base_row is not None:
            base_row = base_row.to(torch.int64).contiguous()
            assert base_row.numel() == n
    out = torch.empty((n, d), dtype=torch.float32, device=bits_a.device)
    abi.check(L.bridges_bits_linear2(n, _ptr(bits_a), _ptr(bits_row_a), _ptr(wt_a), _ptr(bits_b), _ptr(bits_row_b), _ptr(wt_b), d,
                                     _ptr(base), _ptr(base_row), _ptr(out), _stream()), "bridges_bits_linear2")
    return out


def conv_input(block_bits, action_bits, reward, obstacle_bits, block_row=None, action_row=None, reward_row=None, obstacle_row=None,
               out=None):
    """The stacked input of the conv Q-networks in one launch (bridges_conv_input_rows): x [n, 4, 64, 64] float32 whose row r is
    (raster of ``block_bits[block_row[r]]``, raster of ``action_bits[action_row[r]]``, ``reward[reward_row[r]]`` copied bit for
    bit, raster of ``obstacle_bits[obstacle_row[r]]``) -- cv.py's cat([block, action, reward, obstacle], dim=1) without the f32
    images of the rasters.  block_bits / action_bits / obstacle_bits [*, 64] int64, reward [*, 64, 64] (or [*, 4096]) float32; a
    row index that is None is the identity; a 1-row ``reward`` / ``obstacle_bits`` without an index is shared by every row
    (stride 0).  n = the length of a row index that is given, else the rows of ``block_bits``.  ``out``: a contiguous float32
    buffer of n * 4 * 64 * 64 elements to write into (e.g. a slice of a static buffer) instead of a new tensor."""
    L = abi.require_gpu()
    block_bits, action_bits, obstacle_bits = block_bits.reshape(-1, 64), action_bits.reshape(-1, 64), obstacle_bits.reshape(-1, 64)
    for b in (block_bits, action_bits, obstacle_bits):
        assert b.is_contiguous() and b.dtype == torch.int64
    reward = reward.reshape(-1, 4096)
    assert reward.is_contiguous() and reward.dtype == torch.float32
    rows = [r for r in (block_row, action_row, reward_row, obstacle_row) if r is not None]
    n = rows[0].numel() if rows else block_bits.shape[0]
    assert all(r.numel() == n for r in rows), "the row indices differ in length"
    block_row, action_row, reward_row, obstacle_row = (r.to(torch.int64).contiguous() if r is not None else None
                                                       for r in (block_row, action_row, reward_row, obstacle_row))
    assert block_row is not None or block_bits.shape[0] >= n, f"{block_bits.shape[0]} rasters in block_bits for {n} rows"
    assert action_row is not None or action_bits.shape[0] >= n, f"{action_bits.shape[0]} rasters in action_bits for {n} rows"
    reward_stride = 0 if (reward_row is None and reward.shape[0] == 1) else 4096
    obstacle_stride = 0 if (obstacle_row is None and obstacle_bits.shape[0] == 1) else 64
    assert reward_stride == 0 or reward_row is not None or reward.shape[0] >= n, f"{reward.shape[0]} maps in reward for {n} rows"
    assert obstacle_stride == 0 or obstacle_row is not None or obstacle_bits.shape[0] >= n, \
        f"{obstacle_bits.shape[0]} rasters in obstacle_bits for {n} rows"
    if out is None:
        out = torch.empty((n, 4, 64, 64), dtype=torch.float32, device=block_bits.device)
    else:
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n * 4 * 4096 and out.device == block_bits.device
        out = out.view(n, 4, 64, 64)
    if n == 0:
        return out
    abi.check(L.bridges_conv_input_rows(n, _ptr(block_bits), _ptr(block_row), _ptr(action_bits), _ptr(action_row), _ptr(reward),
                                        _ptr(reward_row), reward_stride, _ptr(obstacle_bits), _ptr(obstacle_row), obstacle_stride,
                                        _ptr(out), _stream()), "bridges_conv_input_rows")
    return out


def _head_splits(n_rows, n_tiles, slots=512):
    """Column ranges per 128-row workgroup: enough workgroups that the chip's 2 x 256 resident slots stay evenly filled to the
    end of the launch, few enough that the 128-KB row slab each one loads first stays small against its tiles (measured on
    45 k rows x 128 tiles: 1: 1.12 ms, 2: 0.87, 4: 0.86, 8: 0.81, 16: 0.85, 32: 0.94)."""
    wgs = (n_rows + 127) // 128
    best, best_cost = 1, None
    for s in (1, 2, 4, 8, 16, 32):
        if s > n_tiles:
            break
        per = -(-n_tiles // s)
        used = -(-n_tiles // per)
        unit = per + 2.0                                    # tile-times of one workgroup: its tiles + the slab load
        cost = max(wgs * used / slots, 1.0) * unit + unit   # the even part + the tail of the last workgroups
        if best_cost is None or cost < best_cost:
            best, best_cost = s, cost
    return best


def _row_maps(w, w_row, N, n):
    """The per-row form of a head's weights: w [M, N] float32 (one map per task), w_row int32 [n] (the map of every row)."""
    w = w.to(torch.float32).reshape(-1, N).contiguous()
    assert w_row.dtype == torch.int32 and w_row.numel() == n and w_row.is_contiguous() and w_row.device == w.device
    assert 1 <= w.shape[0] and w.shape[0] * N < 2 ** 31
    return w


def head_sigmoid_dot(h, Wd, bd, w, splits=None, w_row=None):
    """out[r] = sum_j w[j] * sigmoid(h[r] . Wd[j] + bd[j]) without materialising the [n, N] product (bridges_head_sigmoid_dot):
    h [n, 256] float32 (rows contiguous), Wd [N, 256], bd [N], w [N].  With ``w_row`` (int32 [n]; per-env tasks) w is [M, N], one
    map per task, and row r is weighed with w[w_row[r]] (bridges_head_sigmoid_dot_rows; entries must lie in [0, M))."""
    L = abi.require_gpu()
    assert h.dtype == torch.float32 and h.dim() == 2 and h.stride(1) == 1 and h.shape[1] == 256
    Wd, bd = Wd.to(torch.float32).contiguous(), bd.to(torch.float32).contiguous()
    N = Wd.shape[0]
    n = h.shape[0]
    w = w.to(torch.float32).reshape(-1).contiguous() if w_row is None else _row_maps(w, w_row, N, n)
    assert Wd.shape[1] == 256 and bd.numel() == N and (w_row is not None or w.numel() == N)
    if splits is None:
        splits = _head_splits(n, (N + 31) // 32)
    out = torch.empty(n, dtype=torch.float32, device=h.device)
    part = torch.empty((splits, n), dtype=torch.float32, device=h.device) if splits > 1 else None
    if w_row is not None:
        abi.check(L.bridges_head_sigmoid_dot_rows(n, 256, N, _ptr(h), h.stride(0), _ptr(Wd), _ptr(bd), _ptr(w), _ptr(w_row), w.shape[0],
                                                  _ptr(out), _ptr(part) if part is not None else None, splits, _stream()),
                  "bridges_head_sigmoid_dot_rows")
        return out
    abi.check(L.bridges_head_sigmoid_dot(n, 256, N, _ptr(h), h.stride(0), _ptr(Wd), _ptr(bd), _ptr(w), _ptr(out),
                                         _ptr(part) if part is not None else None, splits, _stream()), "bridges_head_sigmoid_dot")
    return out


def eps_greedy_select(seg, q, join, u, eps, greedy, idx, cand_offset, rep=None):
    """EpsilonGreedy.select for every env in one launch (bridges_eps_greedy_select): seg int32 [E + 1] row ranges -- or a pair
    (lo, hi) of int32 [E] tensors, with rep int32 [E] = the env whose candidates the rows of env e index (envs in the same
    state share rows, bridges_env_groups) --, q / join float32 [n] (n >= 1), u float32 [E] uniform draws, idx int64 [n] compact
    candidate index of every row, cand_offset int32 [E].
    -> (sel_compact int64 [E], sel_index int32 [E], q_sel float32 [E], explore_w float32 [E])."""
    L = abi.require_gpu()
    if isinstance(seg, (tuple, list)):
        seg_lo, seg_hi = seg
        E = seg_lo.numel()
    else:
        E = seg.numel() - 1
        seg_lo, seg_hi = seg[:E], seg[1:]
    n = q.numel()
    assert seg_lo.dtype == torch.int32 and seg_hi.dtype == torch.int32 and seg_lo.is_contiguous() and seg_hi.is_contiguous()
    assert idx.dtype == torch.int64 and cand_offset.dtype == torch.int32 and n >= 1
    assert rep is None or (rep.dtype == torch.int32 and rep.numel() == E and rep.is_contiguous())
    q, join, u = q.to(torch.float32).contiguous(), join.to(torch.float32).contiguous(), u.to(torch.float32).contiguous()
    idx, cand_offset = idx.contiguous(), cand_offset.contiguous()
    assert join.numel() == n and idx.numel() == n and u.numel() == E and cand_offset.numel() >= E
    dev = q.device
    sel_compact = torch.empty(E, dtype=torch.int64, device=dev)
    sel_index = torch.empty(E, dtype=torch.int32, device=dev)
    q_sel, explore_w = torch.empty(E, dtype=torch.float32, device=dev), torch.empty(E, dtype=torch.float32, device=dev)
    abi.check(L.bridges_eps_greedy_select(E, n, _ptr(seg_lo), _ptr(seg_hi), _ptr(q), _ptr(join), _ptr(u), float(eps), int(bool(greedy)),
                                          _ptr(idx), _ptr(cand_offset), _ptr(rep), _ptr(sel_compact), _ptr(sel_index), _ptr(q_sel), _ptr(explore_w), _stream()),
              "bridges_eps_greedy_select")
    return sel_compact, sel_index, q_sel, explore_w


def boltzmann_select(seg, q, u, temperature, greedy, idx, cand_offset, rep=None, relative=False, spread_floor=1e-3):
    """Boltzmann exploration for every env in one launch (bridges_boltzmann_select): env e draws one of its rows with probability
    proportional to exp(q / temperature) by the inverse CDF at u[e] (the rule stands in include/bridges_hip.h; float64 on the
    device).  seg, q, u, idx, cand_offset and rep as for eps_greedy_select; temperature > 0 and finite (the library refuses any
    other, and an empty q).
    -> (sel_compact int64 [E], sel_index int32 [E], q_sel float32 [E], explore_w float32 [E] = 1 where the drawn row is not the
    first maximum, p_sel float32 [E] = the probability the drawn row had).
    ``relative`` (bridges_boltzmann_select_rel): env e draws at temperature * max(the standard deviation of its finite q,
    spread_floor), formed on the device in the same launch; that effective temperature is a further result, temp_out float64 [E]
    (0 where greedy)."""
    L = abi.require_gpu()
    if isinstance(seg, (tuple, list)):
        seg_lo, seg_hi = seg
        E = seg_lo.numel()
    else:
        E = seg.numel() - 1
        seg_lo, seg_hi = seg[:E], seg[1:]
    n = q.numel()
    assert seg_lo.dtype == torch.int32 and seg_hi.dtype == torch.int32 and seg_lo.is_contiguous() and seg_hi.is_contiguous()
    assert seg_hi.numel() == E and idx.dtype == torch.int64 and cand_offset.dtype == torch.int32
    assert rep is None or (rep.dtype == torch.int32 and rep.numel() == E and rep.is_contiguous())
    q, u = q.to(torch.float32).contiguous(), u.to(torch.float32).contiguous()
    idx, cand_offset = idx.contiguous(), cand_offset.contiguous()
    assert idx.numel() == n and u.numel() == E and cand_offset.numel() >= E
    dev = q.device
    sel_compact = torch.empty(E, dtype=torch.int64, device=dev)
    sel_index = torch.empty(E, dtype=torch.int32, device=dev)
    q_sel, explore_w, p_sel = (torch.empty(E, dtype=torch.float32, device=dev) for _ in range(3))
    if relative:
        temp_out = torch.empty(E, dtype=torch.float64, device=dev)
        abi.check(L.bridges_boltzmann_select_rel(E, n, _ptr(seg_lo), _ptr(seg_hi), _ptr(q), _ptr(u), float(temperature),
                                                 float(spread_floor), int(bool(greedy)), _ptr(idx), _ptr(cand_offset), _ptr(rep),
                                                 _ptr(sel_compact), _ptr(sel_index), _ptr(q_sel), _ptr(explore_w), _ptr(p_sel),
                                                 _ptr(temp_out), _stream()), "bridges_boltzmann_select_rel")
        return sel_compact, sel_index, q_sel, explore_w, p_sel, temp_out
    abi.check(L.bridges_boltzmann_select(E, n, _ptr(seg_lo), _ptr(seg_hi), _ptr(q), _ptr(u), float(temperature), int(bool(greedy)),
                                         _ptr(idx), _ptr(cand_offset), _ptr(rep), _ptr(sel_compact), _ptr(sel_index), _ptr(q_sel),
                                         _ptr(explore_w), _ptr(p_sel), _stream()), "bridges_boltzmann_select")
    return sel_compact, sel_index, q_sel, explore_w, p_sel


def beam_select(seg, q, width, live, ret, disc, idx, cand_offset, rep=None, out=None):
    """The top-``width`` candidates of every group of ``width`` beams in one launch (bridges_beam_select; the rule stands in
    include/bridges_hip.h): E = G * width envs, seg / q / idx / cand_offset / rep as for eps_greedy_select, live uint8 [E], ret and
    disc float64 [E].  A candidate (live env e, row j with q neither NaN nor -inf) scores ret[e] + disc[e] * q[j] in float64;
    slot i of a group takes its i-th candidate by (score desc, q desc, env asc, row asc).
    -> dict(src int32 [E] -- what VecAssemblyGym.fork takes --, sel_compact int64 [E], sel_index int32 [E], q_sel float32 [E],
    score float64 [E], live uint8 [E]); ``out``: such a dict to write into (no allocation)."""
    L = abi.require_gpu()
    if isinstance(seg, (tuple, list)):
        seg_lo, seg_hi = seg
        E = seg_lo.numel()
    else:
        E = seg.numel() - 1
        seg_lo, seg_hi = seg[:E], seg[1:]
    n = q.numel()
    assert seg_lo.dtype == torch.int32 and seg_hi.dtype == torch.int32 and seg_lo.is_contiguous() and seg_hi.is_contiguous()
    assert seg_hi.numel() == E and idx.dtype == torch.int64 and cand_offset.dtype == torch.int32
    assert rep is None or (rep.dtype == torch.int32 and rep.numel() == E and rep.is_contiguous())
    assert live.dtype == torch.uint8 and ret.dtype == torch.float64 and disc.dtype == torch.float64
    assert live.numel() == E and ret.numel() == E and disc.numel() == E
    q = q.to(torch.float32).contiguous()
    idx, cand_offset, live, ret, disc = idx.contiguous(), cand_offset.contiguous(), live.contiguous(), ret.contiguous(), disc.contiguous()
    assert idx.numel() == n and cand_offset.numel() >= E
    dev = q.device
    if out is None:
        out = dict(src=torch.empty(E, dtype=torch.int32, device=dev), sel_compact=torch.empty(E, dtype=torch.int64, device=dev),
                   sel_index=torch.empty(E, dtype=torch.int32, device=dev), q_sel=torch.empty(E, dtype=torch.float32, device=dev),
                   score=torch.empty(E, dtype=torch.float64, device=dev), live=torch.empty(E, dtype=torch.uint8, device=dev))
    abi.check(L.bridges_beam_select(E, int(width), n, _ptr(seg_lo), _ptr(seg_hi), _ptr(q), _ptr(idx), _ptr(cand_offset), _ptr(rep),
                                    _ptr(live), _ptr(ret), _ptr(disc), _ptr(out["src"]), _ptr(out["sel_compact"]), _ptr(out["sel_index"]),
                                    _ptr(out["q_sel"]), _ptr(out["score"]), _ptr(out["live"]), _stream()), "bridges_beam_select")
    return out


def particle_select_args(seg, q, width, live, ret, disc, idx, cand_offset, u_act, u_res, temperature, resample_temperature, rep=None,
                         out=None):
    """The argument checks of particle_select that need no device -> (seg_lo, seg_hi, E, B, G, n).  ValueError in words."""
    import math
    B = int(width)
    if not 1 <= B <= abi.BEAM_MAX_WIDTH:
        raise ValueError(f"particle_select: the width must be 1..{abi.BEAM_MAX_WIDTH}, got {B}")
    T, Tr = float(temperature), float(resample_temperature)
    if not (math.isfinite(T) and T > 0.0):
        raise ValueError(f"particle_select: the temperature must be finite and > 0, got {temperature!r}")
    if not Tr > 0.0:                                         # (a NaN fails the comparison; +inf passes)
        raise ValueError(f"particle_select: the resampling temperature must be > 0 (inf allowed), got {resample_temperature!r}")
    if isinstance(seg, (tuple, list)):
        seg_lo, seg_hi = seg
        E = seg_lo.numel()
    else:
        E = seg.numel() - 1
        seg_lo, seg_hi = seg[:E], seg[1:]
    if E < 0 or E % B != 0:
        raise ValueError(f"particle_select: E = {E} envs is no multiple of the width {B}")
    G, n = E // B, q.numel()
    if E and n < 1:
        raise ValueError("particle_select: q holds no rows")
    want = (("seg_lo", seg_lo, torch.int32, E), ("seg_hi", seg_hi, torch.int32, E), ("q", q, torch.float32, n),
            ("idx", idx, torch.int64, n), ("live", live, torch.uint8, E), ("ret", ret, torch.float64, E),
            ("disc", disc, torch.float64, E), ("u_act", u_act, torch.float32, E), ("u_res", u_res, torch.float32, G),
            ("rep", rep, torch.int32, E))
    for name, t, dt, count in want:
        if t is None and name == "rep":
            continue
        if t.dtype != dt or t.numel() != count:
            raise ValueError(f"particle_select: {name} must be {dt} [{count}], got {t.dtype} {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"particle_select: {name} must be contiguous")
    if cand_offset.dtype != torch.int32 or cand_offset.numel() < E or not cand_offset.is_contiguous():
        raise ValueError(f"particle_select: cand_offset must be contiguous int32 [>= {E}], got {cand_offset.dtype} "
                         f"{tuple(cand_offset.shape)}")
    if out is not None:
        for name, dt, count in (("src", torch.int32, E), ("sel_compact", torch.int64, E), ("sel_index", torch.int32, E),
                                ("q_sel", torch.float32, E), ("score", torch.float64, E), ("live", torch.uint8, E),
                                ("p_sel", torch.float32, E), ("ess", torch.float64, G)):
            t = out.get(name)
            if t is None or t.dtype != dt or t.numel() != count or not t.is_contiguous():
                raise ValueError(f"particle_select: out[{name!r}] must be contiguous {dt} [{count}]")
    return seg_lo, seg_hi, E, B, G, n


def particle_select(seg, q, width, live, ret, disc, idx, cand_offset, u_act, u_res, temperature, resample_temperature, elite=True,
                    rep=None, out=None):
    """Best-of-N rollouts with resampling, one launch (bridges_particle_select; the rule stands in include/bridges_hip.h): the
    sampled sibling of beam_select, same layout and inputs.  A live env with an eligible row is a parent valued ret + disc * (its
    largest q); slot k of a group takes a parent by systematic resampling at u_res[g] over the weights exp((S - max S) /
    resample_temperature) -- inf: every particle keeps its place --, then one of that parent's rows by the Boltzmann rule at
    ``temperature`` with u_act[slot].  ``elite``: slot 0 is the best parent's first maximum instead.  u_act float32 [E], u_res
    float32 [G], uniform in [0, 1).
    -> beam_select's dict plus p_sel float32 [E] (the probability the drawn row had; 1 for the elite) and ess float64 [G] (the
    effective sample size of the group's weights; 0 without parents); ``out``: such a dict to write into (no allocation)."""
    seg_lo, seg_hi, E, B, G, n = particle_select_args(seg, q, width, live, ret, disc, idx, cand_offset, u_act, u_res, temperature,
                                                      resample_temperature, rep, out)
    L = abi.require_gpu()
    dev = q.device
    if out is None:
        out = dict(src=torch.empty(E, dtype=torch.int32, device=dev), sel_compact=torch.empty(E, dtype=torch.int64, device=dev),
                   sel_index=torch.empty(E, dtype=torch.int32, device=dev), q_sel=torch.empty(E, dtype=torch.float32, device=dev),
                   score=torch.empty(E, dtype=torch.float64, device=dev), live=torch.empty(E, dtype=torch.uint8, device=dev),
                   p_sel=torch.empty(E, dtype=torch.float32, device=dev), ess=torch.empty(G, dtype=torch.float64, device=dev))
    abi.check(L.bridges_particle_select(E, B, n, _ptr(seg_lo), _ptr(seg_hi), _ptr(q), _ptr(idx), _ptr(cand_offset), _ptr(rep), _ptr(live),
                                        _ptr(ret), _ptr(disc), _ptr(u_act), _ptr(u_res), float(temperature), float(resample_temperature),
                                        int(bool(elite)), _ptr(out["src"]), _ptr(out["sel_compact"]), _ptr(out["sel_index"]),
                                        _ptr(out["q_sel"]), _ptr(out["score"]), _ptr(out["live"]), _ptr(out["p_sel"]), _ptr(out["ess"]),
                                        _stream()), "bridges_particle_select")
    return out


def beam_merge(n_blocks, blk_shape, blk_pose, blk_occ, targets_left, width, live, ret, key_last=True, out=None):
    """The beams of every group of ``width`` that hold the same structure, in one launch (bridges_beam_merge; the rule stands in
    include/bridges_hip.h): E = G * width envs whose state arrays are n_blocks int32 [E], blk_shape int32 [E, K], blk_pose float64
    [E, K, 4], blk_occ uint8 [E, K] and targets_left int32 [E] (a VecAssemblyGym's own); live uint8 [E], ret float64 [E].  Two live
    envs of a group are equivalent iff they hold the same multiset of (shape, occupancy, pose bits) blocks, the same targets_left
    and -- with key_last -- the same last block; the first of a class by (ret desc, env asc) represents it.
    -> dict(rep int32 [E], live uint8 [E] = live & (rep == env), n_merged int32 [G] = the live envs closed per group); ``out``: such
    a dict to write into (no allocation)."""
    L = abi.require_gpu()
    E, B = n_blocks.numel(), int(width)
    assert blk_shape.dim() == 2 and blk_shape.shape[0] == E
    K = blk_shape.shape[1]
    assert n_blocks.dtype == torch.int32 and blk_shape.dtype == torch.int32 and blk_pose.dtype == torch.float64
    assert blk_occ.dtype == torch.uint8 and targets_left.dtype == torch.int32 and live.dtype == torch.uint8 and ret.dtype == torch.float64
    assert tuple(blk_pose.shape) == (E, K, 4) and tuple(blk_occ.shape) == (E, K)
    assert targets_left.numel() == E and live.numel() == E and ret.numel() == E
    for t in (n_blocks, blk_shape, blk_pose, blk_occ, targets_left, live, ret):
        assert t.is_contiguous()
    if out is None:
        dev = n_blocks.device
        out = dict(rep=torch.empty(E, dtype=torch.int32, device=dev), live=torch.empty(E, dtype=torch.uint8, device=dev),
                   n_merged=torch.empty(E // B if B > 0 else 0, dtype=torch.int32, device=dev))
    abi.check(L.bridges_beam_merge(E, B, K, _ptr(n_blocks), _ptr(blk_shape), _ptr(blk_pose), _ptr(blk_occ), _ptr(targets_left), _ptr(live),
                                   _ptr(ret), int(bool(key_last)), _ptr(out["rep"]), _ptr(out["live"]), _ptr(out["n_merged"]), _stream()),
              "bridges_beam_merge")
    return out


def beam_trace_args(rec, valid, parent, end_env, end_depth, B, gamma, n_step=1, tail=None):
    """The argument checks of beam_trace that need no device -> (E, B, D, n_step, n_tail, W_out).  ValueError in words."""
    import math
    B, n_step = int(B), int(n_step)
    if not 1 <= B <= abi.BEAM_MAX_WIDTH:
        raise ValueError(f"beam_trace: the width must be 1..{abi.BEAM_MAX_WIDTH}, got {B}")
    if not 1 <= n_step <= abi.NSTEP_MAX:
        raise ValueError(f"beam_trace: n_step must be 1..{abi.NSTEP_MAX}, got {n_step}")
    if not math.isfinite(float(gamma)):
        raise ValueError(f"beam_trace: gamma must be finite, got {gamma!r}")
    if rec.dim() != 3 or rec.shape[2] != abi.REC_WIDTH or rec.dtype != torch.float64:
        raise ValueError(f"beam_trace: rec must be float64 [D, E, {abi.REC_WIDTH}], got {rec.dtype} {tuple(rec.shape)}")
    D, E = int(rec.shape[0]), int(rec.shape[1])
    if not 1 <= D <= abi.BEAM_TRACE_MAX_DEPTH:
        raise ValueError(f"beam_trace: 1..{abi.BEAM_TRACE_MAX_DEPTH} depths, got {D}")
    if E % B != 0:
        raise ValueError(f"beam_trace: E = {E} envs is no multiple of the width {B}")
    G = E // B
    if valid.dtype not in (torch.uint8, torch.bool) or tuple(valid.shape) != (D, E):
        raise ValueError(f"beam_trace: valid must be uint8 or bool [{D}, {E}], got {valid.dtype} {tuple(valid.shape)}")
    if parent.dtype != torch.int32 or tuple(parent.shape) != (D, E):
        raise ValueError(f"beam_trace: parent must be int32 [{D}, {E}], got {parent.dtype} {tuple(parent.shape)}")
    for name, t in (("end_env", end_env), ("end_depth", end_depth)):
        if t.dtype != torch.int32 or tuple(t.shape) != (G,):
            raise ValueError(f"beam_trace: {name} must be int32 [{G}], got {t.dtype} {tuple(t.shape)}")
    n_tail = 0
    if tail is not None:
        if tail.dtype != torch.float64 or tail.dim() != 2 or tail.shape[0] != E:
            raise ValueError(f"beam_trace: tail must be float64 [{E}, n_tail], got {tail.dtype} {tuple(tail.shape)}")
        n_tail = int(tail.shape[1])
    for name, t in (("rec", rec), ("valid", valid), ("parent", parent), ("end_env", end_env), ("end_depth", end_depth), ("tail", tail)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"beam_trace: {name} must be contiguous")
    return E, B, D, n_step, n_tail, abi.REC_WIDTH + n_tail + (1 if n_step > 1 else 0)


def beam_trace(rec, valid, parent, end_env, end_depth, B, gamma, n_step=1, tail=None, priority=0.0, out=None, offset=None, status=None):
    """The transition records of one finished beam per group of ``B`` beams, traced back through the slots it occupied
    (bridges_beam_trace; the rule stands in include/bridges_hip.h).  rec float64 [D, E, 111], valid uint8 [D, E] and parent int32
    [D, E] are what a search kept per depth (the step's record, whether the env made one, the src of that depth's beam_select);
    end_env, end_depth int32 [G] name the end of one episode per group (end_depth < 0: none).  An intact chain of L = end_depth + 1
    steps emits L rows in the width a replay ring stores: the record of the last of h = min(n_step, L - t) steps with the start's
    STABLE_S, ``priority`` as TD and, for h > 1, the h-step return as LIN; then tail[end_env] (float64 [E, n_tail]: the task), then
    h when n_step > 1.
    -> dict(rows float64 [G * D, W_out] -- group g's rows are rows[offset[g] : offset[g + 1]], rows from offset[G] on are not
    written --, offset int32 [G + 1], status int32 [G]: 1 where the chain is broken); ``out`` / ``offset`` / ``status``: tensors to
    write into (no allocation).  Nothing here waits for the GPU."""
    E, B, D, n_step, n_tail, Wo = beam_trace_args(rec, valid, parent, end_env, end_depth, B, gamma, n_step, tail)
    L = abi.require_gpu()
    G, dev = E // B, rec.device
    if out is None:
        out = torch.empty((G * D, Wo), dtype=torch.float64, device=dev)
    if offset is None:
        offset = torch.empty(G + 1, dtype=torch.int32, device=dev) if E else torch.zeros(1, dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(G, dtype=torch.int32, device=dev)
    assert out.dtype == torch.float64 and tuple(out.shape) == (G * D, Wo) and out.is_contiguous()
    assert offset.dtype == torch.int32 and offset.numel() == G + 1 and offset.is_contiguous()
    assert status.dtype == torch.int32 and status.numel() == G and status.is_contiguous()
    if E:
        abi.check(L.bridges_beam_trace(E, B, D, n_step, n_tail, _ptr(rec), _ptr(valid), _ptr(parent), _ptr(end_env), _ptr(end_depth),
                                       _ptr(tail), float(gamma), float(priority), _ptr(out), _ptr(offset), _ptr(status), _stream()),
                  "bridges_beam_trace")
    return dict(rows=out, offset=offset, status=status)


def episode_stats_(out, rec, valid, gpow, n_targets, run, counted, count_first_only=False):
    """Folds one lock-step's records rec float64 [E, W] / valid bool [E] into the per-episode sums ``out`` float64 [8] in place
    (bridges_episode_stats): run float32 [E, 2] and counted int32 [E] carry the episodes that span calls, gpow float32 [K] =
    float32(gamma ** i).  Slots of out: episodes, sum reward, sum lin_reward, sum num_steps, sum stable, sum success, 2 spare."""
    L = abi.require_gpu()
    E = valid.numel()
    assert rec.dtype == torch.float64 and rec.dim() == 2 and rec.shape[0] == E and rec.is_contiguous()
    assert valid.dtype in (torch.bool, torch.uint8) and valid.is_contiguous()
    assert run.dtype == torch.float32 and run.shape == (E, 2) and run.is_contiguous()
    assert counted.dtype == torch.int32 and counted.numel() == E and counted.is_contiguous()
    assert out.dtype == torch.float64 and out.numel() == 8 and out.is_contiguous()
    assert gpow.dtype == torch.float32 and gpow.dim() == 1 and gpow.numel() >= 1 and gpow.is_contiguous()
    abi.check(L.bridges_episode_stats(E, gpow.numel(), _ptr(rec), _ptr(valid), _ptr(gpow), int(n_targets), int(bool(count_first_only)),
                                      _ptr(run), _ptr(counted), _ptr(out), _stream()), "bridges_episode_stats")
    return out


def episode_stats_by_class_(out, rec, valid, gpow, n_targets, run, counted, cls, count_first_only=False):
    """episode_stats_ by class (bridges_episode_stats_by_class): out float64 [n_classes, 8], 1 <= n_classes <= 8, cls int32 [E] =
    the class every env's episode is played under (a task family's task_class as it was before the step); an ended episode of env
    e goes into row cls[e], a class outside [0, n_classes) into none.  One class and cls all zero: episode_stats_' bits."""
    L = abi.require_gpu()
    E = valid.numel()
    assert rec.dtype == torch.float64 and rec.dim() == 2 and rec.shape[0] == E and rec.is_contiguous()
    assert valid.dtype in (torch.bool, torch.uint8) and valid.is_contiguous()
    assert run.dtype == torch.float32 and run.shape == (E, 2) and run.is_contiguous()
    assert counted.dtype == torch.int32 and counted.numel() == E and counted.is_contiguous()
    assert out.dtype == torch.float64 and out.dim() == 2 and out.shape[1] == 8 and out.is_contiguous()
    assert 1 <= out.shape[0] <= abi.EPISODE_STATS_MAX_CLASSES
    assert cls.dtype == torch.int32 and cls.numel() == E and cls.is_contiguous()
    assert gpow.dtype == torch.float32 and gpow.dim() == 1 and gpow.numel() >= 1 and gpow.is_contiguous()
    abi.check(L.bridges_episode_stats_by_class(E, gpow.numel(), _ptr(rec), _ptr(valid), _ptr(gpow), int(n_targets),
                                               int(bool(count_first_only)), _ptr(cls), int(out.shape[0]), _ptr(run), _ptr(counted),
                                               _ptr(out), _stream()), "bridges_episode_stats_by_class")
    return out


def family_thresholds_(thr, w):
    """thr int64 [C-1] <- the threshold table of the weights w int32 [C] (both on the device; the bits are the header's uint64 /
    uint32 -- a weight is <= 2^20, a threshold <= 2^32), 1 <= C <= 8 (bridges_family_thresholds).  A weight above 2^20 counts as
    2^20 and a zero sum gives the table of equal weights: neither is knowable here without a host wait."""
    L = abi.require_gpu()
    C_ = w.numel()
    assert w.dtype == torch.int32 and w.dim() == 1 and w.is_contiguous() and 1 <= C_ <= abi.FAMILY_MAX_CLASSES
    assert thr.dtype == torch.int64 and thr.dim() == 1 and thr.numel() == C_ - 1 and thr.is_contiguous()
    abi.check(L.bridges_family_thresholds(_ptr(w), C_, _ptr(thr) if C_ > 1 else None, _stream()), "bridges_family_thresholds")
    return thr


def family_draw(seed, env_id_base, episode, n_lo, n_hi, thr=None):
    """-> int32 [E]: the class env env_id_base + i draws in its episode episode[i] (int32 [E], the bits of the env's uint32
    task_episode) from n_lo..n_hi, uniformly or -- thr int64 [n_hi - n_lo] -- by the threshold table (bridges_family_draw)."""
    L = abi.require_gpu()
    E = episode.numel()
    assert episode.dtype == torch.int32 and episode.dim() == 1 and episode.is_contiguous()
    C_ = int(n_hi) - int(n_lo) + 1
    if thr is not None:
        assert thr.dtype == torch.int64 and thr.dim() == 1 and thr.numel() == C_ - 1 and thr.is_contiguous()
        assert thr.device == episode.device
    out = torch.empty(E, dtype=torch.int32, device=episode.device)
    abi.check(L.bridges_family_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_base), E, _ptr(episode), int(n_lo), int(n_hi),
                                    _ptr(thr) if thr is not None and C_ > 1 else None, _ptr(out), _stream()), "bridges_family_draw")
    return out


def family_curriculum_(sums, state, n_lo, n_hi, beta, w_min, min_episodes, w, thr):
    """One curriculum update in place (bridges_family_curriculum): sums float64 [n_classes, 8] (episode_stats_by_class_'s rows;
    consumed rows are zeroed), state float64 [n_classes, 2] = (ema, seen), w int32 [C] and thr int64 [C-1] the new weights and
    table of the classes n_lo..n_hi."""
    L = abi.require_gpu()
    C_ = int(n_hi) - int(n_lo) + 1
    assert sums.dtype == torch.float64 and sums.dim() == 2 and sums.shape[1] == 8 and sums.is_contiguous()
    assert state.dtype == torch.float64 and state.shape == (sums.shape[0], 2) and state.is_contiguous()
    assert w.dtype == torch.int32 and w.dim() == 1 and w.numel() == C_ and w.is_contiguous()
    assert thr.dtype == torch.int64 and thr.dim() == 1 and thr.numel() == C_ - 1 and thr.is_contiguous()
    abi.check(L.bridges_family_curriculum(_ptr(sums), int(sums.shape[0]), _ptr(state), int(n_lo), int(n_hi), float(beta), int(w_min),
                                          int(min_episodes), _ptr(w), _ptr(thr) if C_ > 1 else None, _stream()),
              "bridges_family_curriculum")
    return w, thr


def bits_dot(bits, img, slot, bits_row=None):
    """out[r] = sum(img[slot[r]] * raster(bits[bits_row[r]])) for bit-packed 64x64 rasters (bridges_bits_dot): img
    [n_slots,64,64] float32, slot [n] int64 -> [n] float32."""
    L = abi.require_gpu()
    bits = bits.reshape(-1, 64)
    assert bits.is_contiguous() and bits.dtype == torch.int64 and img.dtype == torch.float32 and img.is_contiguous()
    assert tuple(img.shape[-2:]) == (64, 64)
    slot = slot.to(torch.int64).contiguous()
    n = slot.numel()
    if bits_row is not None:
        bits_row = bits_row.to(torch.int64).contiguous()
        assert bits_row.numel() == n
    out = torch.empty(n, dtype=torch.float32, device=bits.device)
    abi.check(L.bridges_bits_dot(n, _ptr(bits), _ptr(bits_row), _ptr(img), _ptr(slot), _ptr(out), _stream()), "bridges_bits_dot")
    return out


def bits_accumulate_(img, bits, slot, weight=None, bits_row=None):
    """img[slot[r]] += weight[r] * raster(bits[bits_row[r]]) in place (bridges_bits_accumulate)."""
    L = abi.require_gpu()
    bits = bits.reshape(-1, 64)
    assert bits.is_contiguous() and bits.dtype == torch.int64 and img.dtype == torch.float32 and img.is_contiguous()
    assert tuple(img.shape[-2:]) == (64, 64)
    slot = slot.to(torch.int64).contiguous()
    n = slot.numel()
    if bits_row is not None:
        bits_row = bits_row.to(torch.int64).contiguous()
    if weight is not None:
        weight = weight.to(torch.float32).contiguous()
    abi.check(L.bridges_bits_accumulate(n, _ptr(bits), _ptr(bits_row), _ptr(weight), _ptr(slot), _ptr(img), _stream()),
              "bridges_bits_accumulate")
    return img


def sigmoid_dot(d, w, w_row=None):
    """out[r] = sum_j w[j] * sigmoid(d[r, j]) in one pass over ``d`` ([n, k] float32, k % 4 == 0; bridges_sigmoid_dot).  With
    ``w_row`` (int32 [n]) w is [M, k] and row r is weighed with w[w_row[r]] (bridges_sigmoid_dot_rows)."""
    L = abi.require_gpu()
    assert d.dtype == torch.float32 and d.dim() == 2 and d.stride(1) == 1
    n, k = d.shape
    out = torch.empty(n, dtype=torch.float32, device=d.device)
    if w_row is not None:
        w = _row_maps(w, w_row, k, n)
        abi.check(L.bridges_sigmoid_dot_rows(n, _ptr(d), d.stride(0), _ptr(w), _ptr(w_row), k, _ptr(out), _stream()),
                  "bridges_sigmoid_dot_rows")
        return out
    w = w.to(torch.float32).reshape(-1).contiguous()
    assert w.numel() == k
    abi.check(L.bridges_sigmoid_dot(n, _ptr(d), d.stride(0), _ptr(w), k, _ptr(out), _stream()), "bridges_sigmoid_dot")
    return out


def stability(blocks, fixed, mu, density, floor_half_width, floor_depth, tension_tol=None):
    """is_stable_rbe (stability.py:49-71) of ONE assembly.  Returns (stable: bool, info: dict).
    With ``tension_tol`` the penalty variant (is_stable_rbe_penalty, stability.py:75-88): contact points may pull, stable
    iff an equilibrium with total tension <= tension_tol exists; info['forces'] then holds that equilibrium's contact
    forces [n_interfaces, 2, 3] = (compression, tension, tangential) per contact point."""
    L = abi.require_gpu()
    dev = device()
    K = abi.MAX_BLOCKS
    n = len(blocks)
    if n > K:
        raise abi.BridgesHipError(f"{n} blocks > BRIDGES_MAX_BLOCKS ({K})")
    if n == 0:                                   # empty assembly: no edges, no free node (stability.py:53-56)
        out = dict(objective=0.0, n_interfaces=0, pivots=0)
        if tension_tol is not None:
            out["forces"] = np.zeros((0, 2, 3))
        return True, out
    pose = np.zeros((1, K, 4))
    verts = np.zeros((1, K, 6, 2))
    ids = np.zeros((1, K), dtype=np.int32)
    mask = 0
    for i, b in enumerate(blocks):
        pose[0, i] = b.pose
        verts[0, i, :len(b.verts_2d)] = b.verts_2d
        ids[0, i] = REGISTRY.id_of(b.geometry)
        if i in fixed:
            mask |= 1 << i
    tab = REGISTRY.device_table()
    ws_stride = abi.lp_ws_stride(K)
    ws = torch.empty((1, ws_stride), dtype=torch.float64, device=dev)
    stable = torch.zeros(1, dtype=torch.uint8, device=dev)
    info = torch.zeros((1, 8), dtype=torch.float64, device=dev)
    # one staging copy for all five inputs; the tensors stay alive until the call returned
    a_pose, a_verts, a_ids, a_n, a_mask = upload(dev, pose, verts, ids, np.array([n], dtype=np.int32), np.array([mask], dtype=np.int32))
    forces = None
    if tension_tol is None:
        abi.check(L.bridges_stability(tab, 1, K, _ptr(a_pose), _ptr(a_verts), _ptr(a_ids), _ptr(a_n), _ptr(a_mask),
                                      float(mu), float(density), float(floor_half_width), float(floor_depth),
                                      _ptr(stable), _ptr(info), _ptr(ws), ws_stride, _stream()), "bridges_stability")
    else:
        forces = torch.zeros((1, abi.MAX_INTERFACES, 2, 3), dtype=torch.float64, device=dev)
        abi.check(L.bridges_stability_penalty(tab, 1, K, _ptr(a_pose), _ptr(a_verts), _ptr(a_ids), _ptr(a_n), _ptr(a_mask),
                                              float(mu), float(density), float(floor_half_width), float(floor_depth),
                                              float(tension_tol), _ptr(stable), _ptr(info), _ptr(forces), _ptr(ws), ws_stride,
                                              _stream()), "bridges_stability_penalty")
    if forces is None:
        inf, st = download(info[0], stable)                   # verdict and diagnostics in ONE copy back
    else:
        inf, st, fo = download(info[0], stable, forces[0])
    if inf[3] != 0:
        return None, dict(error="lp", objective=float(inf[0]), n_interfaces=int(inf[1]), pivots=int(inf[2]))
    out = dict(objective=float(inf[0]), n_interfaces=int(inf[1]), pivots=int(inf[2]))
    if forces is not None:
        out["forces"] = fo[:int(inf[1])]
    return bool(st[0]), out


def stability_variants(blocks, fixed_sets, mu, density, floor_half_width, floor_depth):
    """is_stable_rbe of the SAME blocks under several frozen sets, in one operator call and one copy back: a list of
    (stable, info) as ``stability`` returns them.  (AssemblyGym.step asks for the new block frozen and, right after, for it
    free: gym_env.py:238-243 with :325-333 of the reference.)"""
    L = abi.require_gpu()
    dev = device()
    K = abi.MAX_BLOCKS
    n, m = len(blocks), len(fixed_sets)
    if n > K:
        raise abi.BridgesHipError(f"{n} blocks > BRIDGES_MAX_BLOCKS ({K})")
    if n == 0:
        return [(True, dict(objective=0.0, n_interfaces=0, pivots=0)) for _ in fixed_sets]
    pose = np.zeros((m, K, 4))
    verts = np.zeros((m, K, 6, 2))
    ids = np.zeros((m, K), dtype=np.int32)
    for i, b in enumerate(blocks):
        pose[:, i] = b.pose
        verts[:, i, :len(b.verts_2d)] = b.verts_2d
        ids[:, i] = REGISTRY.id_of(b.geometry)
    masks = np.array([sum(1 << i for i in fixed if i < n) for fixed in fixed_sets], dtype=np.int32)
    tab = REGISTRY.device_table()
    ws_stride = abi.lp_ws_stride(K)
    ws = torch.empty((m, ws_stride), dtype=torch.float64, device=dev)
    stable = torch.zeros(m, dtype=torch.uint8, device=dev)
    info = torch.zeros((m, 8), dtype=torch.float64, device=dev)
    a_pose, a_verts, a_ids, a_n, a_mask = upload(dev, pose, verts, ids, np.full(m, n, dtype=np.int32), masks)
    abi.check(L.bridges_stability(tab, m, K, _ptr(a_pose), _ptr(a_verts), _ptr(a_ids), _ptr(a_n), _ptr(a_mask),
                                  float(mu), float(density), float(floor_half_width), float(floor_depth),
                                  _ptr(stable), _ptr(info), _ptr(ws), ws_stride, _stream()), "bridges_stability")
    inf, st = download(info, stable)
    out = []
    for j in range(m):
        d = dict(objective=float(inf[j, 0]), n_interfaces=int(inf[j, 1]), pivots=int(inf[j, 2]))
        out.append((None, dict(d, error="lp")) if inf[j, 3] != 0 else (bool(st[j]), d))
    return out


def action_stability(blocks, fixed, candidates, mu, density, floor_half_width, floor_depth):
    """is_action_stable_rbe (stability.py:122-130) of every candidate placement of ONE assembly in one bridges_stability launch
    and one copy back: item i is ``blocks`` followed by ``candidates[i]`` (free), the frozen set ``fixed`` (indices into
    ``blocks``) stays.  ``blocks`` / ``candidates``: objects with ``pose``, ``verts_2d`` and ``geometry`` (assembly_gym Blocks).
    Returns bool numpy [n]: True = stable; a solver error counts as unstable (stability.py:68)."""
    L = abi.require_gpu()
    dev = device()
    K = abi.MAX_BLOCKS
    nb, m = len(blocks), len(candidates)
    if m == 0:
        return np.zeros(0, dtype=bool)
    if nb + 1 > K:
        raise abi.BridgesHipError(f"{nb + 1} blocks > BRIDGES_MAX_BLOCKS ({K})")
    pose = np.zeros((m, K, 4))
    verts = np.zeros((m, K, 6, 2))
    ids = np.zeros((m, K), dtype=np.int32)
    for i, b in enumerate(blocks):
        pose[:, i] = b.pose
        verts[:, i, :len(b.verts_2d)] = b.verts_2d
        ids[:, i] = REGISTRY.id_of(b.geometry)
    for j, c in enumerate(candidates):
        pose[j, nb] = c.pose
        verts[j, nb, :len(c.verts_2d)] = c.verts_2d
        ids[j, nb] = REGISTRY.id_of(c.geometry)
    mask = sum(1 << i for i in fixed if i < nb)
    tab = REGISTRY.device_table()
    ws_stride = abi.lp_ws_stride(K)
    ws = torch.empty((m, ws_stride), dtype=torch.float64, device=dev)
    stable = torch.zeros(m, dtype=torch.uint8, device=dev)
    info = torch.zeros((m, 8), dtype=torch.float64, device=dev)
    a_pose, a_verts, a_ids, a_n, a_mask = upload(dev, pose, verts, ids, np.full(m, nb + 1, dtype=np.int32),
                                                 np.full(m, mask, dtype=np.int32))
    abi.check(L.bridges_stability(tab, m, K, _ptr(a_pose), _ptr(a_verts), _ptr(a_ids), _ptr(a_n), _ptr(a_mask),
                                  float(mu), float(density), float(floor_half_width), float(floor_depth),
                                  _ptr(stable), _ptr(info), _ptr(ws), ws_stride, _stream()), "bridges_stability")
    inf, st = download(info, stable)
    return (st != 0) & (inf[:, 3] == 0)


def create_blocks(target_blocks, target_faces, geoms, faces, oxs, oys):
    """AssemblyGym.create_block for n candidate placements in ONE bridges_create_block + ONE bridges_face_frames launch
    and three device-to-host copies (the per-candidate form costs a launch pair and three blocking copies each).
    target_blocks[i] = None for the floor, else an object with ``verts_2d`` / ``geometry``.  Returns per placement
    (pose[4], verts[nv,2], frames[nv,6]) float64 numpy -- the same values as n single calls (the kernels work per item)."""
    L = abi.require_gpu()
    dev = device()
    n = len(geoms)
    if n == 0:
        return []
    sid = np.array([REGISTRY.id_of(g) for g in geoms], dtype=np.int32)
    tsid = np.array([REGISTRY.id_of(t.geometry) if t is not None else sid[i] for i, t in enumerate(target_blocks)], dtype=np.int32)
    tab = REGISTRY.device_table()
    tv = np.zeros((n, 6, 2))
    tf = np.full(n, -1, dtype=np.int32)
    for i, t in enumerate(target_blocks):
        if t is not None:
            tv[i, :len(t.verts_2d)] = t.verts_2d
            tf[i] = int(target_faces[i])
    pose = torch.empty((n, 4), dtype=torch.float64, device=dev)
    verts = torch.empty((n, 6, 2), dtype=torch.float64, device=dev)
    frames = torch.empty((n, 6, 6), dtype=torch.float64, device=dev)
    sh, a_tv, a_ts, a_tf, a_face, a_ox, a_oy = upload(dev, sid, tv, tsid, tf, np.asarray(faces, dtype=np.int32),
                                                      np.asarray(oxs, dtype=np.float64), np.asarray(oys, dtype=np.float64))
    abi.check(L.bridges_create_block(tab, n, _ptr(a_tv), _ptr(a_ts), _ptr(a_tf), _ptr(sh), _ptr(a_face), _ptr(a_ox),
                                     _ptr(a_oy), _ptr(pose), _ptr(verts), None, _stream()), "bridges_create_block")
    abi.check(L.bridges_face_frames(tab, n, _ptr(sh), _ptr(verts), _ptr(frames), _stream()), "bridges_face_frames")
    pose_h, verts_h, frames_h = download(pose, verts, frames)
    return [(pose_h[i], verts_h[i, :len(g.verts)], frames_h[i, :len(g.verts)]) for i, g in enumerate(geoms)]


def create_block(target_block, target_face, geom, face, ox, oy):
    """AssemblyGym.create_block on the device.  target_block = None for the floor, else an object with
    ``verts_2d`` / ``geometry``.  Returns (pose[4], verts[nv,2], frames[nv,6]) float64 numpy."""
    return create_blocks([target_block], [target_face], [geom], [face], [ox], [oy])[0]


def pose_block(geom, pose4):
    """Block.__init__ on the device: world vertices and face frames of a shape posed by (x, z, cos, sin)."""
    L = abi.require_gpu()
    dev = device()
    sid = REGISTRY.id_of(geom)
    tab = REGISTRY.device_table()
    sh, p = upload(dev, np.array([sid], dtype=np.int32), np.array([list(pose4)], dtype=np.float64))
    verts = torch.empty((1, 6, 2), dtype=torch.float64, device=dev)
    frames = torch.empty((1, 6, 6), dtype=torch.float64, device=dev)
    abi.check(L.bridges_pose_block(tab, 1, _ptr(sh), _ptr(p), _ptr(verts), _stream()), "bridges_pose_block")
    abi.check(L.bridges_face_frames(tab, 1, _ptr(sh), _ptr(verts), _ptr(frames), _stream()), "bridges_face_frames")
    nv = len(geom.verts)
    verts_h, frames_h = download(verts, frames)
    return verts_h[0, :nv], frames_h[0, :nv]


def contains_points(block, points):
    """Shape.contains_2d (assembly_env.py:126-137): bool per (x, z) sample point, numpy in / numpy out."""
    L = abi.require_gpu()
    dev = device()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 2))
    n = pts.shape[0]
    sid = REGISTRY.id_of(block.geometry)
    tab = REGISTRY.device_table()
    v = np.zeros((6, 2))
    v[:len(block.verts_2d)] = block.verts_2d
    tv, tp = upload(dev, v, pts)
    out = torch.zeros(n, dtype=torch.uint8, device=dev)
    abi.check(L.bridges_contains_points(tab, sid, _ptr(tv), n, _ptr(tp), _ptr(out), _stream()), "bridges_contains_points")
    return out.cpu().numpy().astype(bool)
