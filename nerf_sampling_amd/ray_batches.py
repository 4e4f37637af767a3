"""Training ray batches drawn on the device: "B training rays and their target colours" from a dataset uploaded once.

``DeviceRayDataset`` keeps the images and poses of a scene in device memory and hands out batches through two kernels of
csrc/ns_rays.hip: ``gather`` (the caller names image and pixel of every ray: Trainer.sample_random_ray_batch's host draws,
without the full-frame ray generation and the per-step image upload) and ``draw`` (the kernel derives the indices itself).
``DrawBatchSource`` is ``draw`` with its step counter and window in device memory, which is what a captured hipGraph replays.

``draw`` samples WITHOUT replacement with a generator of its own -- it is not numpy's stream, so a run
in "draw" mode sees other batches than the reference does under the same np.random.seed.  ``permute_index`` and
``draw_indices`` restate that generator in integers on the host.  They are the yardstick the kernel is tested against, not a
fallback: nothing on the training path calls them.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

SCOPES = ("per_image", "all_images")
ROUNDS = 6                                     # NS_RAY_DRAW_ROUNDS
SSIM_WINDOW = 11                               # NS_SSIM_WINDOW
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_IMAGE_SALT = 0xD1B54A32D192ED03


def _mix64(z: int) -> int:
    """splitmix64's finaliser on a Python int"""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _mix32(h: np.ndarray) -> np.ndarray:
    """murmur3's finaliser on uint64 arrays holding 32-bit values"""
    m = np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & m
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & m
    return h ^ (h >> np.uint64(16))


def draw_key(seed: int, counter: int) -> int:
    return _mix64((int(seed) & _M64) ^ _mix64(int(counter) + _GOLDEN))


def permute_index(n: int, seed: int, counter: int, i) -> np.ndarray:
    """P_{seed,counter}(i) for every i of an integer array, 0 <= i < n < 2^31: the keyed bijection of [0, n) that
    ns_ray_batch_draw evaluates per ray -- a balanced Feistel network of ROUNDS rounds over the smallest even bit width that
    covers n (round function: murmur3's 32-bit finaliser of half + round key, round key r: the low 32 bits of
    mix64(key + (r + 1) * golden), key = mix64(seed ^ mix64(counter + golden)), mix64 = splitmix64's finaliser), walked along
    its cycle until the value is below n."""
    n = int(n)
    i = np.asarray(i)
    if not 1 <= n < 1 << 31:
        raise ValueError("permute_index: 1 <= n < 2^31")
    if i.size and (int(i.min()) < 0 or int(i.max()) >= n):
        raise ValueError("permute_index: indices must lie in [0, n)")
    half = 1
    while (1 << (2 * half)) < n:
        half += 1
    key = draw_key(seed, counter)
    rk = [np.uint64(_mix64(key + (r + 1) * _GOLDEN) & 0xFFFFFFFF) for r in range(ROUNDS)]
    mask, sh, m32 = np.uint64((1 << half) - 1), np.uint64(half), np.uint64(0xFFFFFFFF)
    v = i.astype(np.uint64).reshape(-1).copy()
    todo = np.arange(v.size)
    while todo.size:
        w = v[todo]
        left, right = w >> sh, w & mask
        for k in range(ROUNDS):
            left, right = right, left ^ (_mix32((right + rk[k]) & m32) & mask)
        w = (left << sh) | right
        v[todo] = w
        todo = todo[w >= np.uint64(n)]
    return v.astype(np.int64).reshape(i.shape)


def full_window(H: int, W: int) -> Tuple[int, int, int, int]:
    return (0, int(H), 0, int(W))


def precrop_window(H: int, W: int, frac: float) -> Tuple[int, int, int, int]:
    """(row0, row1, col0, col1) of the reference's centre crop (Trainer.py:437-452)"""
    dH, dW = int(H // 2 * frac), int(W // 2 * frac)
    return (H // 2 - dH, H // 2 + dH, W // 2 - dW, W // 2 + dW)


def _check_window(window, H, W, B, scope):
    r0, r1, c0, c1 = (int(x) for x in window)
    if r0 < 0 or r1 > H or c0 < 0 or c1 > W:
        raise ValueError(f"window {window} lies outside the {H} x {W} frame")
    if r0 >= r1 or c0 >= c1:
        raise ValueError(f"window {window} is empty")
    if scope == "per_image" and B > (r1 - r0) * (c1 - c0):
        raise ValueError(f"a per-image batch is drawn without replacement: B = {B} exceeds the window's "
                         f"{(r1 - r0) * (c1 - c0)} pixels")
    return r0, r1, c0, c1


def draw_indices(B: int, step: int, seed: int, scope: str, H: int, W: int, train_idx: Sequence[int],
                 window=None) -> Tuple[np.ndarray, np.ndarray]:
    """(image_idx [B], pixel [B]) int32, the indices ns_ray_batch_draw derives for this batch (see its header comment)."""
    if scope not in SCOPES:
        raise ValueError(f"scope must be one of {SCOPES}, got {scope!r}")
    B, step, H, W = int(B), int(step), int(H), int(W)
    train_idx = np.asarray(train_idx, dtype=np.int64).reshape(-1)
    if B < 0 or step < 0 or train_idx.size == 0:
        raise ValueError("draw_indices: B >= 0, step >= 0 and at least one training image")
    i = np.arange(B, dtype=np.int64)
    if scope == "all_images":
        N = train_idx.size * H * W
        pos = step * B + i
        epoch, within = pos // N, pos % N
        g = np.empty(B, dtype=np.int64)
        for e in np.unique(epoch):
            sel = epoch == e
            g[sel] = permute_index(N, seed, int(e), within[sel])
        return train_idx[g // (H * W)].astype(np.int32), (g % (H * W)).astype(np.int32)
    r0, r1, c0, c1 = _check_window(full_window(H, W) if window is None else window, H, W, B, scope)
    cols = c1 - c0
    img = int(train_idx[_mix64(draw_key(seed, step) ^ _IMAGE_SALT) % train_idx.size])
    w = permute_index((r1 - r0) * cols, seed, step, i)
    return np.full(B, img, dtype=np.int32), ((r0 + w // cols) * W + c0 + w % cols).astype(np.int32)


def _intrinsics(hwf_or_K, H, W):
    a = np.asarray(hwf_or_K, dtype=np.float64)
    if a.shape == (3, 3):
        return float(a[0, 0]), float(a[1, 1]), float(a[0, 2]), float(a[1, 2])
    if a.shape == (3,):
        if (int(a[0]), int(a[1])) != (H, W):
            raise ValueError(f"hwf says {int(a[0])} x {int(a[1])}, the images are {H} x {W}")
        return float(a[2]), float(a[2]), 0.5 * W, 0.5 * H
    raise ValueError("hwf_or_K: [H, W, focal] or a 3 x 3 intrinsics matrix")


class DeviceRayDataset:
    """Images [n,H,W,3|4] (fp32), poses [n,3|4,4], intrinsics ([H, W, focal] or K) and the training split of a scene, uploaded
    once.  ``white_bkgd`` composites 4-channel images onto white as BlenderTrainer.load_data does, per drawn pixel."""

    def __init__(self, images, poses, hwf_or_K, i_train, white_bkgd: bool = False, device="cuda"):
        import torch

        from . import _lib

        images = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(images)))
        if images.dtype != torch.float32:
            raise TypeError(f"images must be float32 (got {images.dtype}); uint8 images are not supported")
        if images.dim() != 4 or images.shape[-1] not in (3, 4):
            raise ValueError(f"images must be [n, H, W, 3 or 4], got {tuple(images.shape)}")
        poses = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(poses)))
        if poses.dim() != 3 or poses.shape[0] != images.shape[0] or tuple(poses.shape[1:]) not in ((3, 4), (4, 4)):
            raise ValueError(f"poses must be [n, 3 or 4, 4] with one pose per image, got {tuple(poses.shape)}")
        self.n_images, self.H, self.W, self.C = (int(s) for s in images.shape)
        if self.n_images * self.H * self.W >= 1 << 31:
            raise ValueError("n_images * H * W must stay below 2^31")
        self.device = torch.device(device)
        self.images = images.to(self.device).contiguous()
        self.poses = poses.to(device=self.device, dtype=torch.float32).contiguous()
        self.white_bkgd = bool(white_bkgd)
        fx, fy, cx, cy = _intrinsics(hwf_or_K, self.H, self.W)
        self.train_idx_host = self._host_indices(i_train, self.n_images, "i_train")
        if self.train_idx_host.size == 0:
            raise ValueError("i_train is empty")
        self.train_idx = torch.from_numpy(self.train_idx_host).to(self.device)
        self.desc = _lib.RayDataset(self.images.data_ptr(), self.poses.data_ptr(), self.n_images, self.H, self.W, self.C,
                                    int(self.poses.shape[1]) * 4, int(self.white_bkgd), fx, fy, cx, cy)

    @staticmethod
    def _host_indices(x, bound, name) -> np.ndarray:
        a = np.asarray(x)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"{name} must hold integers")
        a = a.astype(np.int64).reshape(-1)
        if a.size and (int(a.min()) < 0 or int(a.max()) >= bound):
            raise ValueError(f"{name} out of range [0, {bound})")
        return a.astype(np.int32)

    def _outputs(self, B, out, want_viewdirs):
        import torch

        if out is None:
            rays = torch.empty((2, B, 3), dtype=torch.float32, device=self.device)
            target = torch.empty((B, 3), dtype=torch.float32, device=self.device)
        else:
            rays, target = out
            for t, shape in ((rays, (2, B, 3)), (target, (B, 3))):
                if (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                        or t.device.type != self.device.type):
                    raise ValueError(f"out: contiguous float32 device tensors of shape (2, {B}, 3) and ({B}, 3)")
        view = torch.empty((B, 3), dtype=torch.float32, device=self.device) if want_viewdirs else None
        return rays, target, view

    def _device_indices(self, x, bound, name, B=None):
        """int32 device tensor of indices: host arrays are range-checked, device tensors are not read (the kernel clamps)"""
        import torch

        if isinstance(x, torch.Tensor) and x.is_cuda:
            if x.dtype != torch.int32:
                x = x.to(torch.int32)
            x = x.contiguous().reshape(-1)
        else:
            x = x.numpy() if isinstance(x, torch.Tensor) else x
            x = torch.from_numpy(self._host_indices(x, bound, name)).to(self.device)
        if B is not None and x.numel() != B:
            raise ValueError(f"{name}: {x.numel()} indices for {B} rays")
        return x

    def gather(self, image_idx, pixels, want_viewdirs: bool = False, out=None):
        """(batch_rays [2,B,3], target [B,3][, viewdirs [B,3]]): ray i is pixel ``pixels[i]`` (flat row * W + col) of image
        ``image_idx`` (one int for all rays) or ``image_idx[i]``.  Index arrays on the host are range-checked (ValueError);
        device tensors are used as they are, and the kernel clamps what it reads."""
        from . import _lib, ops

        lib = _lib.load()
        pix = self._device_indices(pixels, self.H * self.W, "pixels")
        B = pix.numel()
        if isinstance(image_idx, (int, np.integer)):
            if not 0 <= int(image_idx) < self.n_images:
                raise ValueError(f"image_idx out of range [0, {self.n_images})")
            img_dev, img = None, int(image_idx)
        else:
            img_dev, img = self._device_indices(image_idx, self.n_images, "image_idx", B), 0
        rays, target, view = self._outputs(B, out, want_viewdirs)
        _lib.check(lib.ns_ray_batch_gather(C.byref(self.desc), ops._ptr(img_dev), img, ops._ptr(pix), B, ops._ptr(rays[0]),
                                           ops._ptr(rays[1]), ops._ptr(view), ops._ptr(target), ops._stream(self.device)),
                   "ns_ray_batch_gather")
        return (rays, target, view) if want_viewdirs else (rays, target)

    def draw(self, B: int, step: Optional[int] = 0, window=None, scope: str = "per_image", seed: int = 0,
             want_viewdirs: bool = False, want_indices: bool = False, out=None, params_dev=None, train_idx=None):
        """(batch_rays [2,B,3], target [B,3][, viewdirs [B,3]][, (image_idx [B], pixel [B]) int32]) of batch ``step``.

        ``window``: (row0, row1, col0, col1) the per-image scope draws from (None: the whole frame; the pre-crop of the first
        iterations is ``precrop_window``).  ``params_dev``: an int32 device tensor {step, row0, row1, col0, col1} read by the
        kernel INSTEAD of ``step`` / ``window`` -- no host value of the launch changes between steps, so it can be captured
        (DrawBatchSource).  ``train_idx``: an int32 device tensor replacing the dataset's training split."""
        import torch

        from . import _lib, ops

        lib = _lib.load()
        if scope not in SCOPES:
            raise ValueError(f"scope must be one of {SCOPES}, got {scope!r}")
        B = int(B)
        if B < 0:
            raise ValueError("negative batch size")
        host = None
        if params_dev is None:
            if int(step) < 0:
                raise ValueError("negative step")
            r0, r1, c0, c1 = _check_window(full_window(self.H, self.W) if window is None else window, self.H, self.W, B, scope)
            host = C.byref(_lib.RayDrawParams(int(step), r0, r1, c0, c1))
        elif params_dev.dtype != torch.int32 or params_dev.numel() != 5 or not params_dev.is_cuda:
            raise ValueError("params_dev: five int32 in device memory")
        tidx = self.train_idx if train_idx is None else train_idx
        rays, target, view = self._outputs(B, out, want_viewdirs)
        idx = (torch.empty((2, B), dtype=torch.int32, device=self.device) if want_indices else None)
        _lib.check(lib.ns_ray_batch_draw(C.byref(self.desc), ops._ptr(tidx), tidx.numel(), SCOPES.index(scope),
                                         ops._ptr(params_dev), host, int(seed) & _M64, B,
                                         ops._ptr(None if idx is None else idx[0]), ops._ptr(None if idx is None else idx[1]),
                                         ops._ptr(rays[0]), ops._ptr(rays[1]), ops._ptr(view), ops._ptr(target),
                                         ops._stream(self.device)), "ns_ray_batch_draw")
        res = (rays, target) + ((view,) if want_viewdirs else ()) + (((idx[0], idx[1]),) if want_indices else ())
        return res

    def _score_args(self, rgb, R, out, slot, workspace, need):
        """what image_sqerr and image_ssim ask of a frame [R,3], the result array and the workspace (``need`` bytes):
        -> (rgb stride in floats, out, slot, workspace), ``out`` and ``workspace`` allocated where None"""
        import torch

        from . import ops

        if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.float32 and tuple(rgb.shape) == (R, 3)):
            raise ValueError(f"rgb: a float32 device tensor of shape ({R}, 3)")
        if rgb.is_contiguous():
            stride = 3
        elif tuple(rgb.stride()) == (4, 1):
            stride = 4
        else:
            raise ValueError("rgb: contiguous [R,3], or the [:, :3] view of a contiguous [R,4] shard")
        dev = self.images.device                                # the dataset's device, with its index
        return (stride, *ops._sum_slot(out, slot, dev), ops._scratch(workspace, need, dev, "the dataset"))

    @staticmethod
    def sqerr_workspace_bytes(n_pixels: int) -> int:
        """ns_image_sqerr_workspace_bytes: the partial sums ``image_sqerr`` needs for a band of ``n_pixels`` pixels"""
        from . import _lib

        return int(_lib.load().ns_image_sqerr_workspace_bytes(int(n_pixels)))

    def image_sqerr(self, image_idx: int, rgb, rows=None, out=None, slot: int = 0, workspace=None):
        """ns_image_sqerr: the squared error of a rendered frame -- or of its rows ``rows`` = (row0, row1) -- against image
        ``image_idx``, summed over pixels and the three channels in double on the device: sum (double)(fl32(rgb - target))^2,
        target as ``gather`` returns it.  ``rgb``: fp32 [R,3] on the device, R = (row1 - row0) * W, contiguous or the
        ``[:, :3]`` view of a contiguous [R,4] shard.  Returns a 1-element float64 device tensor, or writes ``out[slot]``
        (``out``: a contiguous 1-d float64 device tensor) and returns ``out``.  ``workspace``: a contiguous device tensor of
        at least ``sqerr_workspace_bytes(R)`` bytes (None: allocated for the call).  Nothing is read back: see
        ``psnr_from_sqerr``.  What is wrong with the arguments raises ValueError before any launch."""
        from . import _lib, ops

        lib = _lib.load()
        if not isinstance(image_idx, (int, np.integer)) or not 0 <= int(image_idx) < self.n_images:
            raise ValueError(f"image_idx {image_idx!r} out of range [0, {self.n_images})")
        r0, r1 = (0, self.H) if rows is None else (int(rows[0]), int(rows[1]))
        if r0 < 0 or r1 > self.H:
            raise ValueError(f"rows {(r0, r1)} lie outside the {self.H} x {self.W} frame")
        if r0 >= r1:
            raise ValueError(f"rows {(r0, r1)} are empty")
        R = (r1 - r0) * self.W
        stride, out, slot, workspace = self._score_args(rgb, R, out, slot, workspace, self.sqerr_workspace_bytes(R))
        _lib.check(lib.ns_image_sqerr(C.byref(self.desc), int(image_idx), r0, r1, ops._ptr(rgb), stride,
                                      C.c_void_p(out.data_ptr() + 8 * slot), ops._ptr(workspace), ops._stream(self.device)),
                   "ns_image_sqerr")
        return out

    @staticmethod
    def psnr_from_sqerr(sums, n_values):
        """-10 log10(sum / n_values) in float64, on the host: the PSNR of frames whose ``image_sqerr`` sums are ``sums`` (a
        device or host tensor, an array or a number) over ``n_values`` = 3 * pixels values each.  A device tensor is read back
        here, once."""
        if hasattr(sums, "detach"):
            sums = sums.detach().cpu().numpy()
        with np.errstate(divide="ignore"):
            return -10.0 * np.log10(np.asarray(sums, dtype=np.float64) / np.asarray(n_values, dtype=np.float64))

    @staticmethod
    def ssim_tile():
        """ns_image_ssim_tile: (rows, columns) of window origins one workgroup of ``image_ssim`` owns"""
        from . import _lib

        th, tw = C.c_int(0), C.c_int(0)
        _lib.load().ns_image_ssim_tile(C.byref(th), C.byref(tw))
        return th.value, tw.value

    def ssim_workspace_bytes(self) -> int:
        """ns_image_ssim_workspace_bytes: the partial sums ``image_ssim`` needs for a frame of this dataset"""
        from . import _lib

        return int(_lib.load().ns_image_ssim_workspace_bytes(self.H, self.W))

    def image_ssim(self, image_idx: int, rgb, out=None, slot: int = 0, workspace=None):
        """ns_image_ssim: the SSIM of a rendered frame against image ``image_idx`` (Wang et al. 2004: 11 x 11 gaussian windows,
        sigma 1.5, C1 = 1e-4, C2 = 9e-4, data range 1; target as ``gather`` returns it), summed in double on the device over the
        (H - 10)(W - 10) windows inside the frame and the three channels.  ``rgb``: the whole frame, fp32 [H*W,3] on the device,
        contiguous or the ``[:, :3]`` view of a contiguous [H*W,4] shard.  ``out`` / ``slot`` / ``workspace`` (at least
        ``ssim_workspace_bytes()`` bytes) and the return value as ``image_sqerr``'s.  Nothing is read back: see
        ``ssim_from_sum``.  What is wrong with the arguments raises ValueError before any launch."""
        from . import _lib, ops

        lib = _lib.load()
        if not isinstance(image_idx, (int, np.integer)) or not 0 <= int(image_idx) < self.n_images:
            raise ValueError(f"image_idx {image_idx!r} out of range [0, {self.n_images})")
        if self.H < SSIM_WINDOW or self.W < SSIM_WINDOW:
            raise ValueError(f"a {self.H} x {self.W} frame is smaller than the {SSIM_WINDOW} x {SSIM_WINDOW} window")
        stride, out, slot, workspace = self._score_args(rgb, self.H * self.W, out, slot, workspace, self.ssim_workspace_bytes())
        _lib.check(lib.ns_image_ssim(C.byref(self.desc), int(image_idx), ops._ptr(rgb), stride,
                                     C.c_void_p(out.data_ptr() + 8 * slot), ops._ptr(workspace), ops._stream(self.device)),
                   "ns_image_ssim")
        return out

    @staticmethod
    def ssim_from_sum(sums, H, W):
        """sum / (3 (H - 10)(W - 10)) in float64, on the host: the mean SSIM of H x W frames whose ``image_ssim`` sums are
        ``sums`` (a device or host tensor, an array or a number).  A device tensor is read back here, once."""
        H, W = int(H), int(W)
        if H < SSIM_WINDOW or W < SSIM_WINDOW:
            raise ValueError(f"a {H} x {W} frame is smaller than the {SSIM_WINDOW} x {SSIM_WINDOW} window")
        if hasattr(sums, "detach"):
            sums = sums.detach().cpu().numpy()
        return np.asarray(sums, dtype=np.float64) / np.float64(3 * (H - SSIM_WINDOW + 1) * (W - SSIM_WINDOW + 1))


class DrawBatchSource:
    """``DeviceRayDataset.draw`` with the step counter and the window in device memory: ``launch`` is the draw kernel and the
    counter increment (ns_add_i32), and reads nothing from the host -- trainers.GraphedDepthNetStep captures it in front of
    the training step.  ``window_fn(i)`` names the window of iteration ``i`` (None: the whole frame); ``begin(i)`` rewrites the
    device copy when it changes (the end of the pre-crop).  Calling the source, ``source(i)``, is the eager form: one batch."""

    def __init__(self, dataset: DeviceRayDataset, B: int, scope: str = "per_image", seed: int = 0, first_step: int = 0,
                 window_fn=None, train_idx=None):
        import torch

        self.ds, self.B, self.scope, self.seed = dataset, int(B), scope, int(seed)
        self.window_fn = window_fn
        self.train_idx = None
        if train_idx is not None:
            self.train_idx = torch.from_numpy(dataset._host_indices(train_idx, dataset.n_images, "train_idx")).to(dataset.device)
        self.window = self._window_of(None)
        if int(first_step) < 0:
            raise ValueError("negative first step")
        self.params = torch.tensor([int(first_step), *self.window], dtype=torch.int32).to(dataset.device)

    def _window_of(self, i):
        w = None if (self.window_fn is None or i is None) else self.window_fn(i)
        return _check_window(full_window(self.ds.H, self.ds.W) if w is None else w, self.ds.H, self.ds.W, self.B, self.scope)

    def begin(self, i):
        """host side of iteration ``i``, before the launch (or the replay holding it)"""
        import torch

        w = self._window_of(i)
        if w != self.window:
            self.window = w
            self.params[1:].copy_(torch.tensor(w, dtype=torch.int32))

    def launch(self, rays, target):
        """draw into ``rays`` [2,B,3] / ``target`` [B,3], then advance the device step"""
        from . import _lib, ops

        self.ds.draw(self.B, scope=self.scope, seed=self.seed, out=(rays, target), params_dev=self.params,
                     train_idx=self.train_idx)
        _lib.check(_lib.load().ns_add_i32(ops._ptr(self.params), 1, ops._stream(self.ds.device)), "ns_add_i32")

    def empty_batch(self):
        import torch

        return (torch.empty((2, self.B, 3), dtype=torch.float32, device=self.ds.device),
                torch.empty((self.B, 3), dtype=torch.float32, device=self.ds.device))

    def __call__(self, i):
        self.begin(i)
        rays, target = self.empty_batch()
        self.launch(rays, target)
        return rays, target
