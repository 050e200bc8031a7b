"""VecAssemblyGym: E independent assembly_gym environments advanced in lock-step
on one MI355X by the HIP kernels of libbridges_hip.so.

Host-side mirror of ``AssemblyGym`` + the per-step feature pipeline of
``rollout_episode`` (assembly_gym/assembly_gym/envs/gym_env.py:112-333,
robotoddler/training/successor_dqn.py:365-475).  All state lives in device
tensors allocated here (struct of arrays, see ``abi.ENV_BUFFER_FIELDS``); the
library gets raw pointers.  Nothing in here computes the simulation on the
host -- without the library or a GPU construction fails.

Lock-step protocol: after ``reset()`` every env holds the candidate
set of its (fresh) state.  ``step(sel)`` places candidate ``sel[e]`` of every
env (or performs a reset-only step for envs whose state had no valid
candidate), evaluates both stability variants, reward and termination,
auto-resets finished envs and produces the candidate set of the new state.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import abi
from .shapes import ShapeGeometry, load_urdf

DEFAULT_BOUNDS = ((-3.0, -3.0, -1.0), (7.0, 7.0, 9.0))      # assembly_env.py:168


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_stream = abi.current_stream


def gaussian_vector(kernel_size=101, sigma=16):
    """The normalised float32 vector k of the reference's Gaussian kernel k k^T (utils.py:93-115), built as the reference
    builds it: torch float32 on the host.  gaussian_reward_map and the device's per-env reward maps (k_task_features) both
    start from these 101 numbers."""
    coords = torch.arange(kernel_size) - kernel_size // 2
    k = torch.exp(-(coords.float() ** 2) / (2 * sigma ** 2))
    return k / k.sum()


def gaussian_reward_map(target_image, kernel_size=101, sigma=16):
    """convolve_with_gaussian(targets raster, 101, 16) of get_task_features (successor_dqn.py:77-82, utils.py:93-115): the
    zero-padded 'same' cross-correlation of the 0/1 target image with the float32 kernel k k^T, k as the reference builds it
    (torch float32 on the host).  Evaluated on the host, in float64, set pixel by set pixel in row-major order, and rounded
    to float32 once: ONE fixed order on every box.  The library convolution this replaces (conv2d on the GPU) picked its
    algorithm from MIOpen's find results, which depend on the box and on what an earlier process left in MIOpen's cache --
    the same training run ended with different weights after an unrelated process had run convolutions on the box.
    target_image: numpy array [S, S] (the 0/1 targets raster; any weights work); returns float32 [S, S] (within 1e-7 relative
    of the library's float32 sum)."""
    k = gaussian_vector(kernel_size, sigma)
    k2 = (k.unsqueeze(0) * k.unsqueeze(1)).numpy().astype(np.float64)       # the float32 products, as the reference's kernel
    img = np.asarray(target_image, dtype=np.float64)
    S0, S1 = img.shape
    half = kernel_size // 2
    out = np.zeros((S0, S1), dtype=np.float64)
    ys, xs = np.arange(S0)[:, None], np.arange(S1)[None, :]
    for py, px in zip(*np.nonzero(img)):                                     # row-major
        i, j = py - ys + half, px - xs + half                                # out[y, x] += k2[py - y + half, px - x + half]
        ok = (i >= 0) & (i < kernel_size) & (j >= 0) & (j < kernel_size)
        out += img[py, px] * np.where(ok, k2[np.clip(i, 0, kernel_size - 1), np.clip(j, 0, kernel_size - 1)], 0.0)
    return out.astype(np.float32)


class ShapeTable:
    """Device copy of a list of shapes for the stand-alone operators."""

    def __init__(self, geoms):
        L = abi.require_gpu()
        self.geoms = list(geoms)
        arr = (abi.Shape * len(self.geoms))(*[g.to_struct() for g in self.geoms])
        self._dev = C.c_void_p()
        abi.check(L.bridges_shapes_upload(arr, len(self.geoms), C.byref(self._dev)), "bridges_shapes_upload")

    @property
    def ptr(self):
        return self._dev

    def __del__(self):
        try:
            if self._dev:
                abi.lib().bridges_shapes_free(self._dev)
        except Exception:
            pass


def raster_posed(table, verts, shape_ids, grid_x, grid_y, want_bits=True, want_f32=False):
    """bridges_raster_sized on n posed outlines (verts [n,6,2] f64, shape_ids [n] i32, device tensors); the image
    size S = len(grid_x) <= 64, outputs on the 64-word / 64x64 canvas (image = top-left S x S corner)."""
    L = abi.require_gpu()
    n = int(verts.shape[0])
    dev = verts.device
    size = int(grid_x.numel())
    if int(grid_y.numel()) != size:
        raise NotImplementedError("the HIP rasteriser renders square images")
    bits = torch.empty((n, 64), dtype=torch.int64, device=dev) if want_bits else None
    img = torch.empty((n, 64, 64), dtype=torch.float32, device=dev) if want_f32 else None
    abi.check(L.bridges_raster_sized(table.ptr, n, _ptr(verts), _ptr(shape_ids), _ptr(grid_x), _ptr(grid_y), size,
                                     _ptr(bits), _ptr(img), _stream()), "bridges_raster")
    return bits, img


def check_img_size(img_size):
    from .ops import image_size
    return image_size(img_size)


class RandomTargets:
    """``targets=RandomTargets()``: every env draws ``num_targets`` fresh targets whenever it starts an episode, as the
    reference's tower_setup does per env.reset(**setup_fct()) (assembly_gym/envs/gym_env.py:64-79, successor_dqn.py:371):
    x ~ U[x_range), z ~ U[z_range), y = 0.  The draw happens on the device, keyed by (seed, global env id, episode, target,
    axis); its formula is in include/bridges_hip.h (bridges_env_set_task_buffers).  The stream is not numpy's Mersenne
    Twister; the distribution is the reference's."""

    def __init__(self, num_targets=3, x_range=(-4.0, 4.0), z_range=(0.0, 4.0)):
        self.num_targets = int(num_targets)
        self.x_range = (float(x_range[0]), float(x_range[1]))
        self.z_range = (float(z_range[0]), float(z_range[1]))
        if not 1 <= self.num_targets <= abi.MAX_TARGETS:
            raise ValueError(f"num_targets must be 1..{abi.MAX_TARGETS}")
        if self.x_range[0] > self.x_range[1] or self.z_range[0] > self.z_range[1]:
            raise ValueError("empty x_range / z_range")


class RandomObstacles:
    """``obstacles=RandomObstacles(ranges=[((x0, x1), (z0, z1)), ...])``: every env draws one obstacle per range pair whenever it
    starts an episode, as the reference's connecting_setup draws its obstacle with its targets per env.reset(**setup_fct())
    (assembly_gym/envs/gym_env.py:91-99): obstacle o has x ~ U[x0, x1), z ~ U[z0, z1) of ITS pair, y = 0.  The draw happens on the
    device on the episode counter the targets use, keyed by (seed, global env id, episode, obstacle, axis), a stream of its own;
    its formula is in include/bridges_hip.h (bridges_env_set_task_buffers)."""

    def __init__(self, ranges):
        self.ranges = [((float(xr[0]), float(xr[1])), (float(zr[0]), float(zr[1]))) for xr, zr in ranges]
        if not 1 <= len(self.ranges) <= abi.MAX_OBSTACLES:
            raise ValueError(f"RandomObstacles takes 1..{abi.MAX_OBSTACLES} range pairs, one per obstacle")
        for xr, zr in self.ranges:
            if xr[0] > xr[1] or zr[0] > zr[1]:
                raise ValueError("empty x range / z range")

    @property
    def num_obstacles(self):
        return len(self.ranges)


class RandomBridges:
    """``targets=RandomBridges(kind, sizes=(lo, hi))``: a task family -- every env draws ONE integer n in [lo, hi] whenever it
    starts an episode, and its target and obstacles are those of the reference's
    ``horizontal_bridge_setup(square_size=size, num_obstacles=n)`` (kind "span", gym_env.py:25-42) or
    ``bridge_setup(H=size, num_stories=n)`` at ``x`` (kind "tower", gym_env.py:46-61).  The env has one target and ``hi``
    obstacle slots; the slots a drawn task does not use are parked at z = abi.PARK_Z, where they rasterise to nothing.  The
    draw happens on the device, keyed by (seed, global env id, episode); its formula and the coordinates are in
    include/bridges_hip.h (bridges_env_set_task_family).  Pass ``obstacles=[]`` (or None, or the same object) beside it.
    ``weights``: hi - lo + 1 non-negative integers, each <= 2^20, not all zero -- class lo + k is drawn with probability
    weights[k] / sum(weights) through a threshold table (bridges_env_set_family_thresholds); None is the uniform draw, and
    equal weights give the uniform draw's classes draw for draw."""

    KINDS = dict(span=abi.FAMILY_SPAN, tower=abi.FAMILY_TOWER)
    DEFAULT_SIZE = dict(span=0.6, tower=0.8)

    def __init__(self, kind="span", sizes=(1, 4), size=None, x=0.5, weights=None):
        if kind not in self.KINDS:
            raise ValueError(f"kind must be 'span' or 'tower', got {kind!r}")
        try:
            lo, hi = sizes
            ok = int(lo) == lo and int(hi) == hi
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"sizes must be two integers (lo, hi), got {sizes!r}")
        self.kind, self.lo, self.hi = kind, int(lo), int(hi)
        if not 0 <= self.lo <= self.hi or not 1 <= self.hi <= abi.MAX_OBSTACLES:
            raise ValueError(f"sizes must satisfy 0 <= lo <= hi and 1 <= hi <= {abi.MAX_OBSTACLES}, got {sizes!r}")
        self.size = float(self.DEFAULT_SIZE[kind] if size is None else size)
        if not self.size > 0:
            raise ValueError("size must be > 0")
        self.x = float(x)
        self.weights = None if weights is None else check_family_weights(weights, self.hi - self.lo + 1)

    @property
    def family(self):
        return self.KINDS[self.kind]

    @property
    def num_obstacles(self):
        return self.hi

    @property
    def n_classes(self):
        """Rows of per-class statistics: class = n, 0..hi."""
        return self.hi + 1

    def task(self, n):
        """-> (targets [(x, y, z)], obstacles [hi x (x, y, z)]) of the task n names, parked slots included: the numbers the
        device writes (and, for the live ones, the reference's setup functions return)."""
        s = self.size
        if self.kind == "span":
            target = (n * s + 2.5 * s, 0.0, s / 2)
            live = [((o + 1) * s, 0.0, s / 2) for o in range(n)]
        else:
            target = (self.x, 0.0, n * s + s / 2)
            live = [(self.x, 0.0, o * s + s / 2) for o in range(n)]
        return [target], live + [(0.0, 0.0, abi.PARK_Z)] * (self.hi - n)


def check_family_weights(weights, n):
    """-> the weights of a family of n classes as a tuple of ints; ValueError unless they are n non-negative integers, each at
    most 2^20 (abi.FAMILY_MAX_WEIGHT), with a sum > 0."""
    try:
        ws = list(weights)
        ok = all(int(w) == w for w in ws)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"weights must be a sequence of integers, got {weights!r}")
    ws = tuple(int(w) for w in ws)
    if len(ws) != n:
        raise ValueError(f"weights must hold one weight per class (hi - lo + 1 = {n}), got {len(ws)}")
    if any(w < 0 or w > abi.FAMILY_MAX_WEIGHT for w in ws):
        raise ValueError(f"weights must satisfy 0 <= w <= {abi.FAMILY_MAX_WEIGHT}, got {weights!r}")
    if sum(ws) == 0:
        raise ValueError("weights must not all be zero")
    return ws


def family_thresholds(weights):
    """The threshold table of a weighted class draw as Python ints: thr[k] = ceil((w[0] + .. + w[k]) * 2^32 / sum(w)),
    k = 0..C-2 -- what bridges_family_thresholds writes on the device."""
    total, cum, out = sum(weights), 0, []
    for w in weights[:-1]:
        cum += w
        out.append(-((-cum << 32) // total))
    return out


def _is_per_env_targets(targets):
    return isinstance(targets, (torch.Tensor, np.ndarray)) and targets.ndim == 3


_is_per_env_obstacles = _is_per_env_targets          # an [E, O, 3] array, as the targets' [E, T, 3]


def _single_task_attribute(name, per_env_name, flag="per_env_tasks"):
    """An attribute that describes THE task of a fixed-task env.  An env with per-env tasks (``flag``: the part of the task
    the attribute belongs to) has no such thing: reading it raises instead of handing one env's map to every row."""
    key = "_single_task_" + name

    def get(self):
        if getattr(self, flag, False):
            raise abi.BridgesHipError(f"this env has per-env tasks: there is no single `{name}`; read `{per_env_name}` "
                                      "(one entry per env)")
        return self.__dict__[key]

    def put(self, value):
        self.__dict__[key] = value
    return property(get, put)


class VecAssemblyGym:
    """``targets``: a list of (x, y, z) all envs share (the fixed task); a float64 array / tensor [E, T, 3] of per-env targets
    that stay until set_targets() replaces them; RandomTargets(): per-env targets redrawn on the device every episode; or
    RandomBridges(): one target and up to ``hi`` obstacles per env, both named by one integer drawn every episode
    (``task_family`` the sampler, ``task_class`` int32 [E] the env's current n; random_targets / random_obstacles stay None).
    Per-env tasks add env_targets [E,T,3], target_bits [E,64], reward_maps [E,64,64] (reward_maps_img: its [E,S,S] corner),
    reward_prefix [E,64,65] and task_episode [E]: 49 KiB per env.
    ``obstacles``: a list of (x, y, z) all envs share; a float64 array / tensor [E, O, 3] of per-env obstacles that stay until
    set_obstacles() replaces them; or RandomObstacles(ranges): per-env obstacles redrawn on the device every episode, on the
    episode counter of the targets.  Per-env obstacles (``per_env_obstacles``) ride on the per-env task buffers -- with one
    shared target list the targets are replicated into env_targets -- and add env_obstacles [E,O,3], env_obstacle_bits [E,64]
    and obstacle_rasters ([E,S,S] f32, expanded from the bits when read); the candidate filter tests env e against its own."""

    reward_map = _single_task_attribute("reward_map", "reward_maps")
    reward_features = _single_task_attribute("reward_features", "reward_maps_img")
    _reward_obstacle_flat = _single_task_attribute("_reward_obstacle_flat", "reward_maps_img")
    obstacle_raster = _single_task_attribute("obstacle_raster", "obstacle_rasters", flag="per_env_obstacles")

    def __init__(self, num_envs, shapes, obstacles, targets, max_steps=None, mu=0.8, density=1.0, bounds=None,
                 xlim=(-3.0, 7.0), ylim=(0.0, 10.0), x_discr_ground=None, offset_values=(0.0,), seed=0,
                 device="cuda:0", f32_rasters=True, a_max=None, img_size=(64, 64), debug=0, env_id_base=0,
                 sparse_raster_update=False, candidate_snapshots=True, stable_actions_only=False):
        L = abi.require_gpu()
        self.img = check_img_size(img_size)          # S; every image buffer stays a 64x64 canvas, see crop()
        self.L = L
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.E = int(num_envs)
        self.shapes = [s if isinstance(s, ShapeGeometry) else s.geometry for s in shapes]
        self.shape_target_faces = [list(getattr(s, "target_faces_2d", range(g.num_faces_2d)))
                                   for s, g in zip(shapes, self.shapes)]
        self.per_env_tasks = False                   # set by _attach_task_buffers
        self.task_buf = None
        self.random_targets = None
        self.per_env_obstacles = False               # set by _init_obstacles
        self.obstacle_buf = None
        self.random_obstacles = None
        self.task_family = None                      # set by _attach_task_family
        self.task_class = None
        self.family_weights = None                   # set by set_family_weights: int32 [C], int64 [C-1] on the device
        self.family_thresholds = None
        if isinstance(targets, RandomBridges):
            if not (obstacles is None or obstacles is targets or (isinstance(obstacles, (list, tuple)) and len(obstacles) == 0)):
                raise ValueError("RandomBridges draws the obstacles with the target: pass obstacles=[] (or None) beside it")
            obstacles = []
            self.obstacles, self.n_obstacles = [], targets.num_obstacles
        elif isinstance(obstacles, RandomObstacles):
            self.obstacles, self.n_obstacles = [], obstacles.num_obstacles
        elif _is_per_env_obstacles(obstacles):
            if tuple(obstacles.shape[::2]) != (int(num_envs), 3) or not 1 <= obstacles.shape[1] <= abi.MAX_OBSTACLES:
                raise ValueError(f"per-env obstacles must be [num_envs, 1..{abi.MAX_OBSTACLES}, 3], got {tuple(obstacles.shape)}")
            self.obstacles, self.n_obstacles = [], int(obstacles.shape[1])
        else:
            self.obstacles = [tuple(float(v) for v in o) for o in obstacles]
            self.n_obstacles = 0                     # per-env obstacles of one env; a shared list is not counted here
        if isinstance(targets, RandomBridges):
            self.targets, self.n_targets = None, 1
        elif isinstance(targets, RandomTargets):
            self.targets, self.n_targets = None, targets.num_targets
        elif _is_per_env_targets(targets):
            if tuple(targets.shape[::2]) != (int(num_envs), 3) or not 1 <= targets.shape[1] <= abi.MAX_TARGETS:
                raise ValueError(f"per-env targets must be [num_envs, 1..{abi.MAX_TARGETS}, 3], got {tuple(targets.shape)}")
            self.targets, self.n_targets = None, int(targets.shape[1])
        else:
            self.targets = [tuple(float(v) for v in t) for t in targets]
            self.n_targets = len(self.targets)
        self.max_steps = int(max_steps) if max_steps else 0
        self.K = self.max_steps if self.max_steps else abi.MAX_BLOCKS
        if self.K > abi.MAX_BLOCKS:
            raise ValueError(f"max_steps {self.K} > {abi.MAX_BLOCKS} (BRIDGES_MAX_BLOCKS)")
        self.mu, self.density = float(mu), float(density)
        bounds = DEFAULT_BOUNDS if bounds is None else bounds
        self.bounds = tuple(tuple(float(v) for v in b) for b in bounds)
        self.xlim, self.ylim = tuple(map(float, xlim)), tuple(map(float, ylim))
        if x_discr_ground is None:
            x_discr_ground = np.linspace(-2, 0, 10)               # successor_dqn.py:611
        self.x_discr_ground = [float(v) for v in x_discr_ground]
        self.offset_values = [float(v) for v in offset_values]
        self.seed = int(seed)
        self.debug = int(debug)                     # kernel timing experiments only (bench.py --debug echoes it in its line)
        self.env_id_base = int(env_id_base)
        # the task's shape table = the env's shapes + cube06 for obstacles/targets (gym_env.py:277)
        self.cube06 = load_urdf("shapes/cube06.urdf")
        self.table_geoms = self.shapes + [self.cube06]
        self.groups = [(si, f) for si in range(len(self.shapes)) for f in self.shape_target_faces[si]]
        if len(self.groups) > abi.MAX_GROUPS:
            raise ValueError("too many (shape, target face) pairs")
        max_faces = max(g.num_faces_2d for g in self.shapes)
        bound = len(self.groups) * (len(self.x_discr_ground) + self.K * max_faces * len(self.offset_values))
        self.a_max = int(a_max) if a_max else bound
        self.f32_rasters = bool(f32_rasters)
        self.sparse_raster_update = bool(sparse_raster_update)
        # keep the "last block frozen" tableau of every env for candidate_stability_mask() (123 KB per env)
        self.candidate_snapshots = bool(candidate_snapshots)
        # the available actions of a state are filter_actions ∩ is_action_stable_rbe: reset / step / refresh narrow the
        # candidate mask to the stable candidates (restrict_to_stable), so every consumer of cand_mask / n_valid sees only those
        self.stable_actions_only = bool(stable_actions_only)
        self.grid_x = np.linspace(self.xlim[0], self.xlim[1], self.img)    # rendering.py:108
        self.grid_y = np.linspace(self.ylim[1], self.ylim[0], self.img)
        self._alloc()
        self._task_features()
        self._create()
        if isinstance(targets, RandomBridges):
            # explicit per-env buffers of one target and `hi` obstacle slots; the family then writes them on the device
            self._init_obstacles(torch.zeros((self.E, self.n_obstacles, 3), dtype=torch.float64))
            self._attach_task_buffers(None)
            self._attach_task_family(targets)
            if targets.weights is not None:
                self.set_family_weights(targets.weights)
            self.reset()
            return
        if self.n_obstacles:
            self._init_obstacles(obstacles)
        if isinstance(targets, RandomTargets):
            self._attach_task_buffers(targets)
            self.reset()
        elif self.targets is None:
            self.set_targets(targets)
        elif self.per_env_obstacles:
            self.set_targets(self._replicated_targets())     # one target list under per-env obstacles: every env holds a copy
        else:
            self.reset()

    # ------------------------------------------------------------------ buffers
    def _alloc(self):
        E, K, Cc = self.E, self.K, self.E * self.a_max
        self.ws_stride = abi.ENV_LP_WS_DOUBLES            # per-env persistent tableau of the incremental simplex
        self.cand_ws_stride = abi.lp_ws_stride(K)
        dims = dict(E=E, K=K, C=Cc, E1=E + 1, IF=abi.MAX_INTERFACES, WS=self.ws_stride, CWS=abi.CAND_WS_SLOTS,
                    WSC=self.cand_ws_stride)
        self.buf = {}
        for name, dt, shape in abi.ENV_BUFFER_FIELDS:
            if name in ("cand_raster", "state_raster") and not self.f32_rasters:
                self.buf[name] = None
                continue
            if name in ("cand_raster_nz", "state_raster_nz") and not (self.f32_rasters and self.sparse_raster_update):
                self.buf[name] = None
                continue
            shp = tuple(dims[s] if s in dims else int(s) for s in shape.split(","))
            self.buf[name] = torch.zeros(shp, dtype=getattr(torch, dt), device=self.device)
        for name, dt, shape in abi.ENV_BUFFER_FIELDS_TAIL:
            shp = tuple(dims[s] if s in dims else int(s) for s in shape.split(","))
            self.buf[name] = torch.zeros(shp, dtype=getattr(torch, dt), device=self.device)
        self.stats = torch.zeros(16, dtype=torch.int64, device=self.device)
        self.lp_snap = (torch.zeros((E, abi.ENV_LP_SNAP_DOUBLES), dtype=torch.float64, device=self.device)
                        if self.candidate_snapshots else None)
        for k, v in self.buf.items():
            setattr(self, k, v)
        self._contacts_current = True

    def _task_features(self):
        """get_task_features (successor_dqn.py:67-85): obstacle raster and the Gaussian-blurred target raster,
        both rasterised by the HIP kernel from cube06 blocks (gym_env.py:277-284)."""
        dev = self.device
        self.table = ShapeTable(self.table_geoms)
        cube_id = len(self.table_geoms) - 1
        gx = torch.tensor(self.grid_x, dtype=torch.float64, device=dev)
        gy = torch.tensor(self.grid_y, dtype=torch.float64, device=dev)
        self.grid_x_dev, self.grid_y_dev = gx, gy

        def raster_points(points):
            if len(points) == 0:
                return torch.zeros(64, dtype=torch.int64, device=dev)
            verts = torch.zeros((len(points), 6, 2), dtype=torch.float64)
            for i, p in enumerate(points):              # Block(shape=cube06, position=p): identity rotation
                for k, (vx, vz) in enumerate(self.cube06.verts):
                    verts[i, k, 0] = p[0] + vx
                    verts[i, k, 1] = p[2] + vz
            ids = torch.full((len(points),), cube_id, dtype=torch.int32, device=dev)
            bits, _ = raster_posed(self.table, verts.to(dev), ids, gx, gy)
            off = torch.tensor([0, len(points)], dtype=torch.int32, device=dev)
            out = torch.empty(64, dtype=torch.int64, device=dev)
            abi.check(self.L.bridges_bits_or(1, _ptr(off), _ptr(bits), _ptr(out), _stream()), "bridges_bits_or")
            return out

        self.buf["obstacle_bits"].copy_(raster_points(self.obstacles))
        tbits = raster_points(self.targets or [])      # per-env tasks: the single-task tables stay empty and unread
        self.target_bits = tbits                       # [64] raster of the target blocks (per-env tasks: [E,64])
        timg = torch.empty((1, 64, 64), dtype=torch.float32, device=dev)
        abi.check(self.L.bridges_bits_to_f32(1, _ptr(tbits), _ptr(timg), _stream()), "bridges_bits_to_f32")
        S = self.img                                                       # the map of the S x S image, rest of the canvas 0
        rm = np.zeros((64, 64), dtype=np.float32)
        rm[:S, :S] = gaussian_reward_map(timg[0, :S, :S].cpu().numpy())    # successor_dqn.py:80-82, once per task, on the host
        self.buf["reward_map"].copy_(torch.from_numpy(rm))
        # float64 row prefix sums of the map, accumulated left to right on the host (one fixed order on every box): the
        # rasteriser takes sum(raster * reward_map) of a candidate from the runs of its rows (bridges_env_buffers.reward_prefix)
        pre = np.zeros((64, 65), dtype=np.float64)
        pre[:, 1:] = np.cumsum(rm.astype(np.float64), axis=1)
        self.buf["reward_prefix"].copy_(torch.from_numpy(pre))
        oimg = torch.empty((1, 64, 64), dtype=torch.float32, device=dev)
        abi.check(self.L.bridges_bits_to_f32(1, _ptr(self.buf["obstacle_bits"]), _ptr(oimg), _stream()),
                  "bridges_bits_to_f32")
        self.obstacle_raster = self.crop(oimg)                            # [1,S,S] f32
        self.reward_features = self.crop(self.buf["reward_map"].unsqueeze(0))   # [1,S,S] f32
        self._reward_obstacle_flat = None                                        # (cache of the trainer: both maps, flattened)

    def crop(self, images):
        """[..., 64, 64] canvas -> the [..., S, S] image (a no-op view for the default S = 64)."""
        return images if self.img == 64 else images[..., :self.img, :self.img]

    def _create(self):
        t = abi.Task()
        t.n_envs, t.max_blocks, t.max_steps, t.a_max = self.E, self.K, self.max_steps, self.a_max
        t.n_shapes, t.n_groups = len(self.table_geoms), len(self.groups)
        for i, (si, f) in enumerate(self.groups):
            t.group_shape[i], t.group_face[i] = si, f
        t.n_ground, t.n_offsets, t.n_targets = len(self.x_discr_ground), len(self.offset_values), self.n_targets
        t.mu, t.density = self.mu, self.density
        t.floor_half_width = (self.bounds[1][0] - self.bounds[0][0]) / 2.0      # assembly_env.py:290-296
        t.floor_depth = self.bounds[1][1] - self.bounds[0][1]
        self._create_args = (float(t.floor_half_width), float(t.floor_depth))
        t.xlim[0], t.xlim[1], t.ylim[0], t.ylim[1] = *self.xlim, *self.ylim
        if self.n_targets > abi.MAX_TARGETS:
            raise ValueError("too many targets")
        for i, tg in enumerate(self.targets or []):
            for k in range(3):
                t.targets[i][k] = tg[k]
        t.seed = self.seed
        t.debug = self.debug
        t.env_id_base = self.env_id_base
        self._shape_arr = (abi.Shape * len(self.table_geoms))(*[g.to_struct() for g in self.table_geoms])
        self._xg = (C.c_double * len(self.x_discr_ground))(*self.x_discr_ground)
        self._off = (C.c_double * len(self.offset_values))(*self.offset_values)
        t.img_size = self.img
        self._gx = (C.c_double * self.img)(*self.grid_x.tolist())
        self._gy = (C.c_double * self.img)(*self.grid_y.tolist())
        t.shapes = C.cast(self._shape_arr, C.POINTER(abi.Shape))
        dp = C.POINTER(C.c_double)
        t.x_ground, t.offsets = C.cast(self._xg, dp), C.cast(self._off, dp)
        t.grid_x, t.grid_y = C.cast(self._gx, dp), C.cast(self._gy, dp)
        b = abi.EnvBuffers()
        for name, _, _ in abi.ENV_BUFFER_FIELDS:
            setattr(b, name, self.buf[name].data_ptr() if self.buf[name] is not None else None)
        b.lp_ws_stride = self.ws_stride
        b.stats = self.stats.data_ptr()
        for name, _, _ in abi.ENV_BUFFER_FIELDS_TAIL:
            setattr(b, name, self.buf[name].data_ptr())
        b.cand_ws_stride = self.cand_ws_stride
        b.lp_snap = self.lp_snap.data_ptr() if self.lp_snap is not None else None
        b.lp_snap_stride = abi.ENV_LP_SNAP_DOUBLES
        self._env = C.c_void_p()
        abi.check(self.L.bridges_env_create(C.byref(t), C.byref(b), C.byref(self._env)), "bridges_env_create")

    def __del__(self):
        try:
            if getattr(self, "_env", None):
                self.L.bridges_env_destroy(self._env)
        except Exception:
            pass

    # ------------------------------------------------------------------ per-env tasks
    def _attach_task_buffers(self, sampler=None):
        """Allocate (once) and attach the per-env task buffers (bridges_env_set_task_buffers); ``sampler``: a RandomTargets
        to redraw the targets on the device every episode, None to keep env_targets as they are written."""
        if self.n_targets < 1:
            raise ValueError("per-env tasks need at least one target per env")
        if sampler is not None and sampler.num_targets != self.n_targets:
            raise ValueError(f"the env was built for {self.n_targets} targets per env, the sampler draws {sampler.num_targets}")
        if self.task_buf is None:
            dims = dict(E=self.E, T=self.n_targets)
            self.task_buf = {name: torch.zeros(tuple(dims[d] if d in dims else int(d) for d in shape.split(",")),
                                               dtype=getattr(torch, dt), device=self.device)
                             for name, dt, shape in abi.TASK_BUFFER_FIELDS}
            self._gauss_k = gaussian_vector().to(self.device)
            assert self._gauss_k.numel() == abi.GAUSS_TAPS and self._gauss_k.dtype == torch.float32
        tb = abi.TaskBuffers()
        for name, _, _ in abi.TASK_BUFFER_FIELDS:
            setattr(tb, name, self.task_buf[name].data_ptr())
        if self.per_env_obstacles:
            ob, so = self.obstacle_buf, self.random_obstacles
            tb.env_obstacle_bits, tb.env_obstacles = ob["env_obstacle_bits"].data_ptr(), ob["env_obstacles"].data_ptr()
            tb.n_obstacles, tb.sample_obstacles = self.n_obstacles, 1 if so is not None else 0
            for o, (xr, zr) in enumerate(so.ranges if so is not None else []):
                tb.obs_x_range[o][0], tb.obs_x_range[o][1] = xr
                tb.obs_z_range[o][0], tb.obs_z_range[o][1] = zr
        else:
            tb.env_obstacle_bits = None                      # obstacles stay the shared raster (n_obstacles = 0)
        tb.gauss_k = self._gauss_k.data_ptr()
        tb.target_shape = len(self.table_geoms) - 1          # cube06 (gym_env.py:277)
        tb.sample = 1 if sampler is not None else 0
        if sampler is not None:
            tb.x_range[0], tb.x_range[1] = sampler.x_range
            tb.z_range[0], tb.z_range[1] = sampler.z_range
        abi.check(self.L.bridges_env_set_task_buffers(self._env, C.byref(tb)), "bridges_env_set_task_buffers")
        self.random_targets = sampler
        self.task_family = None                              # the library drops a family with the buffers it was set on
        self.family_weights = self.family_thresholds = None  # and the family's threshold table with it
        self.per_env_tasks = True
        self.targets = None
        b = self.task_buf
        self.env_targets, self.target_bits, self.task_episode = b["env_targets"], b["target_bits"], b["task_episode"]
        self.reward_maps, self.reward_prefix = b["reward_map"], b["reward_prefix"]
        self.reward_maps_img = self.crop(self.reward_maps)

    def _attach_task_family(self, sampler):
        """Hand a RandomBridges to the library (bridges_env_set_task_family) on the attached per-env task buffers; the next
        reset() draws episode 0.  Any later _attach_task_buffers (set_targets / set_obstacles) detaches it again."""
        if self.task_class is None:
            self.task_class = torch.zeros(self.E, dtype=torch.int32, device=self.device)
        fam = abi.TaskFamily()
        fam.family, fam.n_lo, fam.n_hi = sampler.family, sampler.lo, sampler.hi
        fam.size, fam.x = sampler.size, sampler.x
        fam.task_class = self.task_class.data_ptr()
        abi.check(self.L.bridges_env_set_task_family(self._env, C.byref(fam)), "bridges_env_set_task_family")
        self.task_family = sampler
        self.family_weights = self.family_thresholds = None

    def set_family_weights(self, weights):
        """Weights of the family's classes lo..hi (RandomBridges(weights=...) documents them), or None for the uniform draw.
        Takes effect from the next episode each env starts; resets nothing and waits for nothing.  The table is built on the
        device (ops.family_thresholds_) into ``family_thresholds`` (int64 [C-1]: the bits of the library's uint64) from
        ``family_weights`` (int32 [C]); both tensors stay the same objects over later calls, and a kernel that rewrites
        family_thresholds in the env's stream (ops.family_curriculum_) changes the draws of the lock-steps after it."""
        if self.task_family is None:
            raise ValueError("set_family_weights needs a task family (targets=RandomBridges(...))")
        if weights is None:
            abi.check(self.L.bridges_env_set_family_thresholds(self._env, None), "bridges_env_set_family_thresholds")
            self.family_weights = self.family_thresholds = None
            return
        n = self.task_family.hi - self.task_family.lo + 1
        ws = check_family_weights(weights, n)
        if self.family_weights is None:
            self.family_weights = torch.zeros(n, dtype=torch.int32, device=self.device)
            self.family_thresholds = torch.zeros(n - 1, dtype=torch.int64, device=self.device)
        self.family_weights.copy_(torch.tensor(ws, dtype=torch.int32))
        from .ops import family_thresholds_
        family_thresholds_(self.family_thresholds, self.family_weights)
        if n > 1:                                            # one class: no table, the draw is lo either way
            abi.check(self.L.bridges_env_set_family_thresholds(self._env, self.family_thresholds.data_ptr()),
                      "bridges_env_set_family_thresholds")

    def set_targets(self, targets, reset=True):
        """Explicit per-env targets ([E, T, 3] float64, T = the env's number of targets) that stay until set again; a sampler
        is switched off.  reset=True starts every env on its new task (reset()); reset=False keeps the block lists and
        target bookkeeping of the current states (a replay env re-creating the task of a loaded state) and only rebuilds
        the task features and the candidates' linear rewards.  No host wait."""
        t = torch.as_tensor(targets, dtype=torch.float64).to(self.device)
        if tuple(t.shape) != (self.E, self.n_targets, 3):
            raise ValueError(f"targets must be [{self.E}, {self.n_targets}, 3], got {tuple(t.shape)}")
        self._attach_task_buffers(None)
        self.env_targets.copy_(t)
        if reset:
            self.reset()                                 # rebuilds the task features of every env
        else:
            abi.check(self.L.bridges_env_load_targets(self._env, _stream()), "bridges_env_load_targets")
            self.refresh()

    def load_targets(self, targets):
        """Per-env targets ([E, T, 3] or [E, 3 T] float64, already on the device) for a scratch env whose states are about to be
        loaded (load_records / load_states, whose refresh gives the candidates the new tasks' linear rewards): env_targets and
        everything derived from them -- target_bits, reward_maps, reward_prefix (bridges_env_load_targets) -- and nothing
        else; task_episode and the states stay.  One copy, one launch sequence, no host wait."""
        if not self.per_env_tasks or self.random_targets is not None:
            raise ValueError("load_targets needs an env with explicit per-env targets (created with an [E, T, 3] array / set_targets)")
        if targets.numel() != self.env_targets.numel() or targets.dtype != torch.float64:
            raise ValueError(f"targets must hold {tuple(self.env_targets.shape)} float64 values, got {tuple(targets.shape)} {targets.dtype}")
        self.env_targets.copy_(targets.reshape(self.env_targets.shape))
        abi.check(self.L.bridges_env_load_targets(self._env, _stream()), "bridges_env_load_targets")

    # ------------------------------------------------------------------ per-env obstacles
    def _replicated_targets(self):
        return torch.tensor(self.targets, dtype=torch.float64).reshape(1, self.n_targets, 3).expand(self.E, -1, -1).contiguous()

    def _init_obstacles(self, obstacles):
        """Allocate (once) the per-env obstacle buffers; ``obstacles``: a RandomObstacles (the sampler) or an [E, O, 3] array
        (explicit obstacles, a sampler is switched off).  The next _attach_task_buffers hands them to the library."""
        sampler = obstacles if isinstance(obstacles, RandomObstacles) else None
        if sampler is not None:
            O = sampler.num_obstacles
        else:
            obstacles = torch.as_tensor(obstacles, dtype=torch.float64)
            if obstacles.ndim != 3 or tuple(obstacles.shape[::2]) != (self.E, 3) or not 1 <= obstacles.shape[1] <= abi.MAX_OBSTACLES:
                raise ValueError(f"obstacles must be [{self.E}, 1..{abi.MAX_OBSTACLES}, 3], got {tuple(obstacles.shape)}")
            O = int(obstacles.shape[1])
        if self.obstacle_buf is None:
            if self.n_targets < 1:
                raise ValueError("per-env obstacles ride on the per-env task buffers, which need at least one target per env")
            dims = dict(E=self.E, O=O)
            self.obstacle_buf = {name: torch.zeros(tuple(dims[d] if d in dims else int(d) for d in shape.split(",")),
                                                   dtype=getattr(torch, dt), device=self.device)
                                 for name, dt, shape in abi.OBSTACLE_BUFFER_FIELDS}
            self.n_obstacles = O
            self.env_obstacles, self.env_obstacle_bits = self.obstacle_buf["env_obstacles"], self.obstacle_buf["env_obstacle_bits"]
        elif O != self.n_obstacles:
            raise ValueError(f"the env was built for {self.n_obstacles} obstacles per env, got {O}")
        if sampler is None:
            self.env_obstacles.copy_(obstacles.to(self.device))
        self.random_obstacles = sampler
        self.per_env_obstacles = True
        self.obstacles = []                                  # there is no shared list any more (obstacle_bits is not read)

    @property
    def obstacle_rasters(self):
        """[E, S, S] float32: every env's obstacle raster, expanded from env_obstacle_bits when read."""
        if not self.per_env_obstacles:
            raise abi.BridgesHipError("this env has one shared obstacle list: read `obstacle_raster`")
        img = torch.empty((self.E, 64, 64), dtype=torch.float32, device=self.device)
        abi.check(self.L.bridges_bits_to_f32(self.E, _ptr(self.env_obstacle_bits), _ptr(img), _stream()), "bridges_bits_to_f32")
        return self.crop(img)

    def set_obstacles(self, obstacles, reset=True):
        """Explicit per-env obstacles ([E, O, 3] float64, O = the env's number of per-env obstacles; an env with a shared list
        becomes a per-env one) that stay until set again; an obstacle sampler is switched off, the targets (and their sampler)
        stay.  reset=True starts every env anew (reset()); reset=False keeps the states and only rebuilds the obstacle rasters
        and the candidates' masks.  No host wait."""
        self._init_obstacles(obstacles)
        if self.per_env_tasks:
            self._attach_task_buffers(self.random_targets)
        else:
            t = self._replicated_targets()
            self._attach_task_buffers(None)
            self.env_targets.copy_(t)
        if reset:
            self.reset()
        else:
            abi.check(self.L.bridges_env_load_targets(self._env, _stream()), "bridges_env_load_targets")
            self.refresh()

    def load_obstacles(self, obstacles):
        """Per-env obstacles ([E, O, 3] or [E, 3 O] float64, already on the device) for a scratch env whose states are about to
        be loaded or refreshed: env_obstacles and env_obstacle_bits (bridges_env_load_targets, which rebuilds the target tables
        beside them) and nothing else; task_episode and the states stay.  One copy, one launch, no host wait."""
        if not self.per_env_obstacles or self.random_obstacles is not None:
            raise ValueError("load_obstacles needs an env with explicit per-env obstacles (created with an [E, O, 3] array / set_obstacles)")
        if obstacles.numel() != self.env_obstacles.numel() or obstacles.dtype != torch.float64:
            raise ValueError(f"obstacles must hold {tuple(self.env_obstacles.shape)} float64 values, got {tuple(obstacles.shape)} {obstacles.dtype}")
        self.env_obstacles.copy_(obstacles.reshape(self.env_obstacles.shape))
        abi.check(self.L.bridges_env_load_targets(self._env, _stream()), "bridges_env_load_targets")

    def load_task(self, targets, obstacles):
        """load_targets and load_obstacles in one: both copies, then ONE bridges_env_load_targets, which rebuilds the target
        tables and the obstacle rasters of every env together (the two methods in a row would run its map work twice).  For a
        scratch env with explicit per-env targets AND obstacles; task_episode and the states stay.  No host wait."""
        if not self.per_env_tasks or self.random_targets is not None:
            raise ValueError("load_task needs an env with explicit per-env targets (created with an [E, T, 3] array / set_targets)")
        if not self.per_env_obstacles or self.random_obstacles is not None:
            raise ValueError("load_task needs an env with explicit per-env obstacles (created with an [E, O, 3] array / set_obstacles)")
        if targets.numel() != self.env_targets.numel() or targets.dtype != torch.float64:
            raise ValueError(f"targets must hold {tuple(self.env_targets.shape)} float64 values, got {tuple(targets.shape)} {targets.dtype}")
        if obstacles.numel() != self.env_obstacles.numel() or obstacles.dtype != torch.float64:
            raise ValueError(f"obstacles must hold {tuple(self.env_obstacles.shape)} float64 values, got {tuple(obstacles.shape)} {obstacles.dtype}")
        self.env_targets.copy_(targets.reshape(self.env_targets.shape))
        self.env_obstacles.copy_(obstacles.reshape(self.env_obstacles.shape))
        abi.check(self.L.bridges_env_load_targets(self._env, _stream()), "bridges_env_load_targets")

    # ------------------------------------------------------------------ lock-step API
    def reset(self):
        abi.check(self.L.bridges_env_reset(self._env, _stream()), "bridges_env_reset")
        self._contacts_current = True
        if self.stable_actions_only:
            self.restrict_to_stable()
        self._cand_version = getattr(self, "_cand_version", 0) + 1

    def select_random(self):
        """Synthetic uniform-random policy over each env's valid candidates -> sel_index."""
        abi.check(self.L.bridges_env_select_random(self._env, _stream()), "bridges_env_select_random")

    def step(self, sel_index=None):
        if sel_index is not None:
            self.buf["sel_index"].copy_(sel_index.to(device=self.device, dtype=torch.int32))
        abi.check(self.L.bridges_env_step(self._env, _stream()), "bridges_env_step")
        if self.stable_actions_only:
            self.restrict_to_stable()
        self._cand_version += 1

    def timing_begin(self, max_launches):
        abi.check(self.L.bridges_env_timing_begin(self._env, int(max_launches)), "bridges_env_timing_begin")

    def timing_end(self):
        """-> (total ms of the rasteriser launches, number of launches), measured with HIP events on the stream."""
        ms, n = C.c_double(0.0), C.c_int32(0)
        abi.check(self.L.bridges_env_timing_end(self._env, C.byref(ms), C.byref(n)), "bridges_env_timing_end")
        return ms.value, n.value

    def refresh(self):
        """Recompute the candidate set (enumerate, rasterise, mask) after the host edited the state arrays."""
        abi.check(self.L.bridges_env_refresh(self._env, _stream()), "bridges_env_refresh")
        if self.stable_actions_only:
            self.restrict_to_stable()
        self._cand_version += 1

    def fork(self, src):
        """Env e continues from the state of env src[e] (bridges_env_fork; src: int32 [E] on the device, any pattern --
        permutation, duplicates, broadcast, swap; an entry outside [0, E) keeps env e as it is): every per-env state array,
        the contact list, the persisted tableaux and, on per-env tasks, the env's task are copied bit for bit through a
        scratch allocated on first use (bridges_env_fork_scratch bytes); then the candidate sets are rebuilt as refresh()
        rebuilds them, narrowed to the stable placements under stable_actions_only.  The copied contacts and snapshots are as
        current as their sources', so nothing has to be rebuilt.  No host wait."""
        src = torch.as_tensor(src)
        if src.numel() != self.E:
            raise ValueError(f"fork: src must hold one source env per env ({self.E}), got {tuple(src.shape)}")
        src = src.to(device=self.device, dtype=torch.int32).contiguous()
        n = C.c_int64(0)                                     # (a host-side sum; it grows when task buffers are attached later)
        abi.check(self.L.bridges_env_fork_scratch(self._env, C.byref(n)), "bridges_env_fork_scratch")
        if getattr(self, "_fork_scratch", None) is None or self._fork_scratch.numel() < n.value:
            self._fork_scratch = torch.empty(max(int(n.value), 16), dtype=torch.uint8, device=self.device)
        abi.check(self.L.bridges_env_fork(self._env, _ptr(src), _ptr(self._fork_scratch), self._fork_scratch.numel(), _stream()),
                  "bridges_env_fork")
        self._fork_src = src                                 # alive until the stream has consumed it
        self.refresh()                                       # bumps _cand_version: the row caches of the old sets are stale

    def restrict_to_stable(self):
        """Narrow the candidate set to the stable placements (bridges_env_restrict_to_stable): is_action_stable_rbe of every
        valid candidate (candidate_stability_mask), then cand_mask &= (cand_stable == 1) and n_valid recounted; an env left
        without a stable candidate is marked no_actions and resets on the next step().  reset() / step() / refresh() call it
        when the env was created with stable_actions_only=True.  No host synchronisation."""
        if not self._contacts_current:
            raise abi.BridgesHipError("candidate stability needs the persistent contact lists of the current states: call "
                                      "rebuild_contacts() after load_states()")
        abi.check(self.L.bridges_env_restrict_to_stable(self._env, _stream()), "bridges_env_restrict_to_stable")
        self._cand_version = getattr(self, "_cand_version", 0) + 1

    def rebuild_contacts(self):
        """Rebuild the persistent contact list of every env's current block list (bridges_env_rebuild_contacts), as step()
        would hold it had it placed the blocks one by one, and invalidate the persisted tableaux: after load_states() /
        load_records() candidate_stability_mask() then decides the loaded states' candidates (from scratch)."""
        abi.check(self.L.bridges_env_rebuild_contacts(self._env, _stream()), "bridges_env_rebuild_contacts")
        self._contacts_current = True

    def load_states(self, n_blocks, blk_shape, blk_pose, blk_occ):
        """Overwrite the state of every env with caller-supplied block lists (replay re-rasterisation): world
        vertices, the state raster and the candidate set are rebuilt by the HIP operators."""
        E, K = self.E, self.K
        self.buf["n_blocks"].copy_(n_blocks)
        self.buf["blk_shape"].copy_(blk_shape)
        self.buf["blk_pose"].copy_(blk_pose)
        self.buf["blk_occ"].copy_(blk_occ)
        self.buf["needs_reset"].zero_()
        self.buf["n_if"].zero_()                      # interfaces: rebuild_contacts() (stable_actions_only) or none
        self._contacts_current = False
        flat_shape = self.buf["blk_shape"].reshape(E * K)
        abi.check(self.L.bridges_pose_block(self.table.ptr, E * K, _ptr(flat_shape), _ptr(self.buf["blk_pose"]),
                                            _ptr(self.buf["blk_verts"]), _stream()), "bridges_pose_block")
        bits = torch.empty((E * K, 64), dtype=torch.int64, device=self.device)
        abi.check(self.L.bridges_raster_sized(self.table.ptr, E * K, _ptr(self.buf["blk_verts"]), _ptr(flat_shape),
                                              _ptr(self.grid_x_dev), _ptr(self.grid_y_dev), self.img, _ptr(bits), None,
                                              _stream()), "bridges_raster")
        start = torch.arange(E, dtype=torch.int32, device=self.device) * K
        ranges = torch.stack([start, start + self.buf["n_blocks"]], dim=1).contiguous()
        abi.check(self.L.bridges_bits_or(E, _ptr(ranges), _ptr(bits), _ptr(self.buf["state_bits"]), _stream()),
                  "bridges_bits_or")
        self._keep = (bits, ranges, flat_shape)       # alive until the stream has consumed them
        # candidate counts of the loaded states, then the usual refresh
        nfree = torch.zeros(E, dtype=torch.int32, device=self.device)
        if getattr(self, "_nv_dev", None) is None:      # once: a host list -> device copy makes the host wait
            self._nv_dev = torch.tensor([g.num_faces_2d for g in self.table_geoms], dtype=torch.int32, device=self.device)
        nv = self._nv_dev
        kidx = torch.arange(K, device=self.device)[None, :]
        live = kidx < self.buf["n_blocks"][:, None]
        faces = nv[self.buf["blk_shape"].long()]
        occ = self.buf["blk_occ"].to(torch.int32)
        popc = sum(((occ >> f) & 1) for f in range(abi.MAX_VERTS))
        nfree = ((faces - popc) * live).sum(dim=1).to(torch.int32)
        n_cand = len(self.groups) * (len(self.x_discr_ground) + nfree * len(self.offset_values))
        self.buf["n_cand"].copy_(n_cand.to(torch.int32))       # raw count: refresh clamps to a_max and flags / counts a truncation
        if self.stable_actions_only:
            self.rebuild_contacts()
        self.refresh()

    def load_records(self, rec, prev=False):
        """load_states for the next states s' of sampled transition records ([n <= E, RECORD_WIDTH] float64,
        robotoddler/training/records.py): ONE launch (bridges_replay_unpack) writes the block lists, the candidate
        counts and the block ranges instead of the ~60 slice / cast / index launches of unpack_states + load_states;
        envs beyond n repeat record 0.  Returns (bits of s, lin_reward f32, stable(s) f32, done u8, stable(s') u8), [E] each.
        ``prev=True`` (bridges_replay_unpack_prev): the env is loaded with the states s the transitions were taken IN -- the
        block lists as stored, their candidate counts -- and everything else is as above (the returned bits are the env's own)."""
        E, K, dev = self.E, self.K, self.device
        assert rec.dtype == torch.float64 and rec.is_contiguous() and 1 <= rec.shape[0] <= E
        if getattr(self, "_nv_dev", None) is None:
            self._nv_dev = torch.tensor([g.num_faces_2d for g in self.table_geoms], dtype=torch.int32, device=dev)
        ranges = torch.empty((2, E, 2), dtype=torch.int32, device=dev)
        lin, stable_s = torch.empty(E, dtype=torch.float32, device=dev), torch.empty(E, dtype=torch.float32, device=dev)
        done, stable_n = torch.empty(E, dtype=torch.uint8, device=dev), torch.empty(E, dtype=torch.uint8, device=dev)
        b = self.buf
        unpack, name = ((self.L.bridges_replay_unpack_prev, "bridges_replay_unpack_prev") if prev
                        else (self.L.bridges_replay_unpack, "bridges_replay_unpack"))
        abi.check(unpack(E, rec.shape[0], K, _ptr(rec), _ptr(self._nv_dev), self._nv_dev.numel(),
                         len(self.groups), len(self.x_discr_ground), len(self.offset_values),
                         _ptr(b["n_blocks"]), _ptr(b["blk_shape"]), _ptr(b["blk_pose"]), _ptr(b["blk_occ"]),
                         _ptr(b["n_cand"]), _ptr(ranges[0]), _ptr(ranges[1]), _ptr(lin), _ptr(stable_s),
                         _ptr(done), _ptr(stable_n), _stream()), name)
        b["needs_reset"].zero_()
        b["n_if"].zero_()                             # interfaces: rebuild_contacts() (stable_actions_only) or none
        self._contacts_current = False
        flat_shape = b["blk_shape"].reshape(E * K)
        abi.check(self.L.bridges_pose_block(self.table.ptr, E * K, _ptr(flat_shape), _ptr(b["blk_pose"]), _ptr(b["blk_verts"]),
                                            _stream()), "bridges_pose_block")
        bits = torch.empty((E * K, 64), dtype=torch.int64, device=dev)
        abi.check(self.L.bridges_raster_sized(self.table.ptr, E * K, _ptr(b["blk_verts"]), _ptr(flat_shape), _ptr(self.grid_x_dev),
                                              _ptr(self.grid_y_dev), self.img, _ptr(bits), None, _stream()), "bridges_raster")
        abi.check(self.L.bridges_bits_or(E, _ptr(ranges[0]), _ptr(bits), _ptr(b["state_bits"]), _stream()), "bridges_bits_or")
        bits_s = torch.empty((E, 64), dtype=torch.int64, device=dev)
        abi.check(self.L.bridges_bits_or(E, _ptr(ranges[1]), _ptr(bits), _ptr(bits_s), _stream()), "bridges_bits_or")
        self._keep = (bits, ranges[0], flat_shape)    # alive until the stream has consumed them
        if self.stable_actions_only:
            self.rebuild_contacts()
        self.refresh()
        return bits_s, lin, stable_s, done, stable_n

    def prefix_state_bits(self, n_prefix):
        """Bit raster of the first n_prefix[e] blocks of every env as loaded by the last load_states call (int32/int64
        [E]): the state a transition started from, when the env holds the state it led to."""
        bits, _, _ = self._keep
        start = torch.arange(self.E, dtype=torch.int32, device=self.device) * self.K
        ranges = torch.stack([start, start + n_prefix.to(torch.int32)], dim=1).contiguous()
        out = torch.empty((self.E, 64), dtype=torch.int64, device=self.device)
        abi.check(self.L.bridges_bits_or(self.E, _ptr(ranges), _ptr(bits), _ptr(out), _stream()), "bridges_bits_or")
        return out

    def candidate_stability_mask(self):
        """is_action_stable_rbe (assembly_gym/utils/stability.py:122-130 of the reference) for EVERY valid candidate of
        every env, fused on the device (bridges_env_candidate_stability): one wave per candidate appends the candidate
        block to its env's persistent contact list in LDS (the last placed block stays frozen, gym_env.py:238-240) and
        solves the feasibility LP.  Fills ``cand_stable`` (uint8 [C]: 1 stable, 0 unstable / masked-out, 2 solver
        error) without any host synchronisation; returns the number of decisions as a device scalar."""
        if not self._contacts_current:
            raise abi.BridgesHipError("candidate stability needs the persistent contact lists of states reached through "
                                      "reset()/step(); this env was overwritten by load_states()")
        abi.check(self.L.bridges_env_candidate_stability(self._env, _stream()), "bridges_env_candidate_stability")
        return self.buf["n_valid"].sum()

    def candidate_stability(self):
        """-> (rows, stable): compact indices of the valid candidates and a bool per row (errors count as unstable,
        stability.py:68 + gym_env.py:182)."""
        self.candidate_stability_mask()
        idx, _ = self.valid_rows()
        return idx, self.buf["cand_stable"][idx] == 1

    def state_groups(self, flag=None, task=False):
        """rep int32 [E]: the smallest env index that holds exactly this env's state -- block count and the shape, pose bits
        and face occupancy of its blocks, plus the caller's per-env ``flag`` byte (e.g. the 'stable' feature) -- found by a
        64-bit hash and verified word for word (bridges_env_groups; two launches, no wait).  Envs in the same state hold the
        same candidates in the same order, so valid_rows(rep) lets them share one set of rows.
        ``task=True`` (an env with per-env tasks): the bit patterns of the env's own targets, env_targets[e], are part of its
        identity as well (bridges_env_groups_keyed) -- what a network says about a state depends on the task it is asked
        under, so only envs in the same state AND under the same task share rows.  Per-env obstacles are part of the task: the
        bit patterns of env_obstacles[e] follow the targets' in the key."""
        hkey = getattr(self, "_hkey", None)
        if hkey is None:
            hkey = self._hkey = torch.empty(self.E, dtype=torch.int64, device=self.device)
        rep = torch.empty(self.E, dtype=torch.int32, device=self.device)
        if flag is not None:
            flag = flag.to(torch.uint8).contiguous()
        b = self.buf
        if task:
            if not self.per_env_tasks:
                raise ValueError("state_groups(task=True) needs an env with per-env tasks (targets=RandomTargets() / set_targets)")
            key = self.env_targets
            if self.per_env_obstacles:
                key = torch.cat([key.reshape(self.E, -1), self.env_obstacles.reshape(self.E, -1)], dim=1).contiguous()
            assert key.dtype == torch.float64 and key.is_contiguous() and key.shape[0] == self.E
            abi.check(self.L.bridges_env_groups_keyed(self.E, self.K, _ptr(b["n_blocks"]), _ptr(b["blk_shape"]), _ptr(b["blk_pose"]),
                                                      _ptr(b["blk_occ"]), _ptr(flag), _ptr(key), key.numel() // self.E, _ptr(hkey),
                                                      _ptr(rep), _stream()), "bridges_env_groups_keyed")
            return rep
        abi.check(self.L.bridges_env_groups(self.E, self.K, _ptr(b["n_blocks"]), _ptr(b["blk_shape"]), _ptr(b["blk_pose"]),
                                            _ptr(b["blk_occ"]), _ptr(flag), _ptr(hkey), _ptr(rep), _stream()), "bridges_env_groups")
        return rep

    def valid_rows(self, rep=None):
        """Compact indices of the valid (filtered) candidates and their owning env: the rows a Q-network is fed
        (bridges_valid_rows: two launches and ONE wait for the row count; torch.nonzero + gather were six launches and two
        waits).  With ``rep`` (state_groups) only the envs that represent their state get rows, and valid_segments() gives
        every env the range of its representative.  The returned tensors are views of two alternating buffers: they stay
        intact until the call after next."""
        cached = getattr(self, "_valid_rows", None)
        if cached is not None and cached[0] == self._cand_version and cached[5] is rep:     # same candidate set, same grouping
            return cached[1], cached[2]
        if getattr(self, "_vr_buf", None) is None:
            cap = self.buf["cand_mask"].numel()
            mk = lambda: (torch.empty(cap, dtype=torch.int64, device=self.device), torch.empty(cap, dtype=torch.int64, device=self.device),
                          torch.empty(self.E + 1, dtype=torch.int32, device=self.device),
                          torch.empty((2, self.E), dtype=torch.int32, device=self.device))
            self._vr_buf, self._vr_flip = (mk(), mk()), 0
            self._vr_total = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._vr_flip ^= 1
        idx_b, env_b, seg, lohi = self._vr_buf[self._vr_flip]
        b = self.buf
        abi.check(self.L.bridges_valid_rows(self.E, _ptr(b["cand_offset"]), _ptr(b["n_cand"]), _ptr(b["n_valid"]), _ptr(b["cand_mask"]),
                                            _ptr(rep), _ptr(seg), _ptr(lohi[0]) if rep is not None else None,
                                            _ptr(lohi[1]) if rep is not None else None, _ptr(idx_b), _ptr(env_b),
                                            C.c_void_p(self._vr_total.data_ptr()), _stream()), "bridges_valid_rows")
        torch.cuda.current_stream(self.device).synchronize()             # the one wait: the count is on the host now
        n = int(self._vr_total[0])
        idx, row_env = idx_b[:n], env_b[:n]
        segs = (lohi[0], lohi[1]) if rep is not None else (seg[:self.E], seg[1:])
        self._valid_rows = (self._cand_version, idx, row_env, seg, segs, rep)
        return idx, row_env

    def valid_segments(self):
        """Row ranges of the envs in the last ``valid_rows()``: (lo, hi), int32 [E] each -- rows lo[e] .. hi[e] are env e's
        (with a grouping: its representative's); without a grouping they are seg[:-1], seg[1:] of the prefix sums of n_valid."""
        if getattr(self, "_valid_rows", None) is None or self._valid_rows[0] != self._cand_version:
            self.valid_rows()
        return self._valid_rows[4]

    # ------------------------------------------------------------------ views
    def flags(self):
        f = self.buf["step_flags"]
        out = {n: f[:, i].bool() for i, n in enumerate(abi.FLAG_NAMES)}
        out["lp_error"] = (f[:, 7] & 3) != 0                    # bit 0 solver error, bit 1 contact-list overflow
        out["cand_overflow"] = (f[:, 7] & 8) != 0               # the state has more raw candidates than a_max: the set was cut
        out["warm_resolved"] = (f[:, 7] & 4) != 0               # a continued tableau's marginal 'unstable' was re-solved cold
        return out

    def binary_features(self):
        """get_state_features' binary vector [stable, collision x5] (successor_dqn.py:53-60).  The vector of the
        current state: 'stable' of a freshly reset env is True (empty assembly, stability.py:53-56)."""
        out = torch.zeros((self.E, 6), dtype=torch.float32, device=self.device)
        f = self.buf["step_flags"]
        fresh = self.buf["n_blocks"] == 0
        out[:, 0] = torch.where(fresh, torch.ones_like(fresh), f[:, 1].bool()).float()
        return out

    def total_candidates(self):
        return int(self.buf["cand_offset"][self.E].item())

    def read_stats(self):
        return dict(zip(abi.STAT_NAMES, self.stats.tolist()))


class VecAssemblyGymGroups:
    """E environments split into G independent groups, each a VecAssemblyGym on its own HIP stream.

    The lock-step of one group is a dependent chain (latency-bound wave-per-env task kernel, then the
    bandwidth-bound rasteriser); with two or more groups in flight the task kernel of one group overlaps the
    rasteriser of another.  Environments are independent, so results are identical to a single group with the same
    global env ids (policy RNG streams are keyed by seed and global env id)."""

    def __init__(self, num_envs, *args, groups=2, device="cuda:0", raster_gate=None, env_id_base=0, **kw):
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.G = int(groups)
        base = num_envs // self.G
        sizes = [base + (1 if g < num_envs % self.G else 0) for g in range(self.G)]
        self.E = int(num_envs)
        self.envs, self.streams, start = [], [], int(env_id_base)
        # `targets` (VecAssemblyGym's argument after num_envs, shapes, obstacles): a list or RandomTargets() goes to every group as
        # it is (the draw is keyed by the global env id); a per-env array [E, T, 3] is cut into the groups' slices
        # `obstacles` (the argument before it) likewise: a list or RandomObstacles() as it is, an [E, O, 3] array in slices
        args, lo = list(args), 0
        positional = "targets" not in kw
        targets = args[2] if positional else kw.pop("targets")
        obst_positional = "obstacles" not in kw
        obstacles = args[1] if obst_positional else kw.pop("obstacles")
        for n in sizes:
            st = torch.cuda.Stream(device=self.device)
            tg = targets[lo:lo + n] if _is_per_env_targets(targets) else targets
            if positional:
                args[2] = tg
            else:
                kw["targets"] = tg
            ob = obstacles[lo:lo + n] if _is_per_env_obstacles(obstacles) else obstacles
            if obst_positional:
                args[1] = ob
            else:
                kw["obstacles"] = ob
            with torch.cuda.stream(st):
                self.envs.append(VecAssemblyGym(n, *args, device=device, env_id_base=start, **kw))
            self.streams.append(st)
            start += n
            lo += n
        self._stream_ptrs = [C.c_void_p(st.cuda_stream) for st in self.streams]
        # one raster gate per GPU: the bandwidth-bound rasterisers of the groups run one after another, the
        # latency-bound task kernels of the other groups run beside them
        self._gate = C.c_void_p()
        L = self.envs[0].L
        abi.check(L.bridges_gate_create(C.byref(self._gate)), "bridges_gate_create")
        if raster_gate is None:                     # the gate pays when the rasterisers are HBM-bound (full rewrite);
            # measured 3 groups, sparse row-group update: 6.89 M env-steps/s without it, 6.18 M with it
            raster_gate = not kw.get("sparse_raster_update")
        if self.G > 1 and raster_gate:
            for env in self.envs:
                abi.check(L.bridges_env_set_gate(env._env, self._gate), "bridges_env_set_gate")
        self.sync()

    def sync(self):
        for st in self.streams:
            st.synchronize()

    def __del__(self):
        try:
            self.sync()
            for env in self.envs:
                env.L.bridges_env_set_gate(env._env, None)
            self.envs[0].L.bridges_gate_destroy(self._gate)
        except Exception:
            pass

    def reset(self):
        for env, st in zip(self.envs, self.streams):
            with torch.cuda.stream(st):
                env.reset()

    def set_targets(self, targets, reset=True):
        """VecAssemblyGym.set_targets for all E envs ([E, T, 3]): every group takes its slice, on its own stream."""
        if int(targets.shape[0]) != self.E:
            raise ValueError(f"targets must hold {self.E} envs, got {tuple(targets.shape)}")
        lo = 0
        for env, st in zip(self.envs, self.streams):
            with torch.cuda.stream(st):
                env.set_targets(targets[lo:lo + env.E], reset=reset)
            lo += env.E

    def set_family_weights(self, weights):
        """VecAssemblyGym.set_family_weights for every group, on its own stream (every group keeps a table of its own)."""
        for env, st in zip(self.envs, self.streams):
            with torch.cuda.stream(st):
                env.set_family_weights(weights)

    def set_obstacles(self, obstacles, reset=True):
        """VecAssemblyGym.set_obstacles for all E envs ([E, O, 3]): every group takes its slice, on its own stream."""
        if int(obstacles.shape[0]) != self.E:
            raise ValueError(f"obstacles must hold {self.E} envs, got {tuple(obstacles.shape)}")
        lo = 0
        for env, st in zip(self.envs, self.streams):
            with torch.cuda.stream(st):
                env.set_obstacles(obstacles[lo:lo + env.E], reset=reset)
            lo += env.E

    def lockstep_random(self):
        """select_random + step for every group, each on its own stream (one C call per group)."""
        fn = self.envs[0].L.bridges_env_lockstep_random
        for env, st, sp in zip(self.envs, self.streams, self._stream_ptrs):
            rc = fn(env._env, sp)
            env._cand_version += 1
            if rc != 0:
                abi.check(rc, "bridges_env_lockstep_random")
            if env.stable_actions_only:
                with torch.cuda.stream(st):
                    env.restrict_to_stable()

    def lockstep_random_candidates(self, timed=None):
        """lockstep_random, then is_action_stable_rbe for every valid candidate of the new states (candidate_stability_mask),
        group by group on the groups' own streams: the latency-bound LP pass of one group runs beside the bandwidth-bound
        rasteriser of the next.  The envs must have been created with candidate_snapshots=True.  ``timed``: a list that
        receives (start event, end event, decisions as a device scalar) of every group's LP pass."""
        fn = self.envs[0].L.bridges_env_lockstep_random
        for env, st, sp in zip(self.envs, self.streams, self._stream_ptrs):
            with torch.cuda.stream(st):
                rc = fn(env._env, sp)
                env._cand_version += 1
                if rc != 0:
                    abi.check(rc, "bridges_env_lockstep_random")
                if env.stable_actions_only:
                    env.restrict_to_stable()
                if timed is not None:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    n = env.candidate_stability_mask()
                    b.record()
                    timed.append((a, b, n))
                else:
                    env.candidate_stability_mask()

    def timing_begin(self, max_launches):
        for env in self.envs:
            env.timing_begin(max_launches)

    def timing_end(self):
        ms = n = 0
        for env in self.envs:
            a, b = env.timing_end()
            ms += a
            n += b
        return ms, n

    def read_stats(self):
        out = {}
        for env in self.envs:
            for k, v in env.read_stats().items():
                out[k] = out.get(k, 0) + v
        return out
