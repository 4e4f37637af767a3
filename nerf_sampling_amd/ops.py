"""Tensor-level wrappers over the C ABI: torch CUDA (ROCm) tensors in, torch tensors out.

PyTorch is used for device memory and streams only; every arithmetic step runs in
libnerf_sampling_hip.so.  All inputs must be fp32 device tensors; outputs are freshly allocated on
the same device.  Calls are asynchronous on torch's current stream.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check

Tensor = torch.Tensor

_DTYPES = {"f32": _lib.DTYPE_F32, "fp32": _lib.DTYPE_F32, "float32": _lib.DTYPE_F32,
           "bf16": _lib.DTYPE_BF16, "bfloat16": _lib.DTYPE_BF16,
           "f16": _lib.DTYPE_F16, "fp16": _lib.DTYPE_F16, "float16": _lib.DTYPE_F16,
           "f16x3": _lib.DTYPE_F16X3,     # split fp16 operands: fp32-grade results on the 16-bit engine
           "f16m": _lib.DTYPE_F16M}       # DepthNet only (production trunk): first three layers split, the rest plain fp16
_MODES = {"depth_only": _lib.MODE_DEPTH_ONLY, "uniform": _lib.MODE_UNIFORM, "gaussian": _lib.MODE_GAUSSIAN}

_compute_dtype = "f32"


def set_compute_dtype(name: str) -> None:
    """MFMA operand precision used when a network is packed without an explicit dtype."""
    global _compute_dtype
    if name not in _DTYPES:
        raise ValueError(f"unknown dtype {name!r}; expected one of {sorted(_DTYPES)}")
    _compute_dtype = name


def get_compute_dtype() -> str:
    return _compute_dtype


def dtype_code(name: Optional[str]) -> int:
    return _DTYPES[name or _compute_dtype]


# Operand type of the DepthNet when a network is packed WITHOUT an explicit dtype under compute dtype X.  Under bf16 the
# DepthNet runs on f16 operands: it costs nothing (same MFMA rate, 0.64 ms of a 28 ms frame) and its depth error -- which
# moves a ray's whole +-0.1 sampling window -- drops sevenfold (z rms 4.6e-4 instead of 3.3e-3), which is what the scene
# PSNR of a sharp, trained field is sensitive to (per-image delta to fp32: 0.005 dB instead of 0.020 dB,
# tools/scene_psnr_sweep.py).  A DepthNet whose weights exceed fp16's range falls back to bf16 (DepthNet.packed).
# Explicit requests -- packed("bf16") -- are always honoured as given.
_DEPTHNET_PAIRING = {"bf16": "f16"}


def depthnet_dtype_for(name: Optional[str] = None) -> str:
    name = name or _compute_dtype
    if _psnr_guard and name in ("bf16", "f16"):
        return _guard_depthnet
    return _DEPTHNET_PAIRING.get(name, name)


# PSNR guard of the 16-bit compute dtypes.  north_star's acceptance bar is a scene PSNR within 0.05 dB of the reference's; on
# a fitted scene that renders at 28-30 dB, plain 16-bit operands sit AT that bar (tools/scene_psnr_sweep.py: worst per-image
# |delta| 0.13 dB for bf16 + bf16, 0.052 dB for the default bf16 + f16 pairing), and the error has two sources that touch
# 1/64 of the arithmetic: the DepthNet's depth (it moves a ray's whole sampling window) and sigma of the LAST sample of a
# ray, which the reference composites with dist = 1e10 (alpha = step(sigma), sampling_trainer.py:176-180).  With the guard
# on, the DepthNet runs on (partly) split fp16 operands (_guard_depthnet below) and that one sample per ray is evaluated a
# second time through an "f16x3" packing of the field (ns_render_args::nerf_guard); the other N - 1 samples keep the fast path.
_psnr_guard = False
# Which rays the guard re-evaluates (ns_render_args::guard_threshold): only those whose own 16-bit sigma of the last sample lies
# within this distance of zero -- a sigma beyond it composites to alpha = 0 or 1 whatever its last bits are.  16 is > 30 x the
# rms bf16 error of sigma_last on the production network (bench.py: sigma_last_err_rms ~ 0.5); 0 = every ray.
_guard_threshold = 16.0
# The guard's DepthNet operands.  "f16x3" (the default): every layer on split fp16 operands, fp32-grade depths (z rms 8e-7 on the
# fitted scene) at 2.9 x the fp16 kernel's time: PSNR(build || fp32) 63-64 dB, every frame and band within 0.03 dB.  "f16m": the
# first three trunk layers split, the other seven plain fp16 -- the rounding of the first layers' wide-ranged activations is where
# a TRAINED fp16 DepthNet loses its depth (z rms 8.9e-4 -> 1.2e-4 there; tools/depthnet_mix_check.py) -- at 1.7 x: 50-53 dB, whole
# frames within 0.03 dB but a 60-row band can read 0.06 (tools/guard_experiment.py, tests/test_scene_psnr.py): the economy setting,
# built for the production trunk (ten layers, 256 wide; any other shape falls back to "f16x3").
_guard_depthnet = "f16x3"
# Which form of the guard rays of several 64-sample chunks take in the one-kernel renderer (n_samples = 128 .. 512,
# ns_render_args::guard_long_selective).  "every" (the default): every ray, before the kernel, whatever the threshold -- the
# every-ray guard's bits on all rays.  "selective": as n_samples <= 64 does -- the kernel flags the rays within the threshold, and
# an unflagged ray whose step flips on its 16-bit sigma keeps the 16-bit one.
_GUARD_LONG_RAYS = ("every", "selective")
_guard_long_rays = "every"


def _check_guard_long_rays(value) -> str:
    if value not in _GUARD_LONG_RAYS:
        raise ValueError(f"guard_long_rays: 'every' or 'selective', got {value!r}")
    return value


def set_psnr_guard(on: bool, threshold: Optional[float] = None, depthnet: Optional[str] = None,
                   long_rays: Optional[str] = None) -> None:
    """``long_rays``: "every" or "selective", the guard's form for rays of several chunks (see _guard_long_rays); None leaves
    it as it is."""
    global _psnr_guard, _guard_threshold, _guard_depthnet, _guard_long_rays
    if long_rays is not None:
        _check_guard_long_rays(long_rays)
    _psnr_guard = bool(on)
    if threshold is not None:
        if not threshold >= 0.0:
            raise ValueError("guard threshold must be >= 0 (0 = every ray)")
        _guard_threshold = float(threshold)
    if depthnet is not None:
        if depthnet not in ("f16m", "f16x3"):
            raise ValueError("the guard's DepthNet runs on 'f16m' or 'f16x3' operands")
        _guard_depthnet = depthnet
    if long_rays is not None:
        _guard_long_rays = long_rays


def psnr_guard() -> bool:
    return _psnr_guard


def guard_long_rays() -> str:
    """The module's setting of the guard's form for rays of several chunks (set_psnr_guard(long_rays=...))."""
    return _guard_long_rays


def psnr_guard_handles(depth_net, nerf, mode: Optional[str] = None, n_samples: Optional[int] = None):
    """(DepthNet handle, field handle, guard handle or None) for the current compute dtype and guard setting: what the
    one-call renderers take.  ``depth_net`` / ``nerf``: this package's DepthNet / NeRF modules.  Given the sampling ``mode``
    / ``n_samples`` of the render, the guard is None where it does not apply: the guard pass is defined for uniform placement
    with n_samples >= 2.  Which rays the guard re-evaluates is the caller's to pass on: guard_threshold (None = the module's)
    and guard_long_rays=ops.guard_long_rays(), as nerf_utils.render_rays_test and parallel.hip_row_renderer do."""
    dn, nf = depth_net.packed(), nerf.packed()
    applies = mode in (None, "uniform") and (n_samples is None or n_samples >= 2)
    guard = nerf.packed("f16x3") if (_psnr_guard and applies and nf.dtype in ("bf16", "f16")) else None
    return dn, nf, guard


def _dev(t: Tensor, name: str) -> Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); this path has no CPU fallback")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _ptr(t: Optional[Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _scratch(workspace, need: int, dev, what: str):
    """the caller's ``workspace`` -- a contiguous 8-byte-aligned tensor of at least ``need`` bytes on ``dev``, the device of
    ``what`` -- or, for None, ``need`` fresh bytes there"""
    if workspace is None:
        return torch.empty((need,), dtype=torch.uint8, device=dev)
    if not (isinstance(workspace, Tensor) and workspace.is_cuda and workspace.device == dev and workspace.is_contiguous()
            and workspace.numel() * workspace.element_size() >= need and workspace.data_ptr() % 8 == 0):
        raise ValueError(f"workspace: a contiguous 8-byte-aligned tensor of at least {need} bytes on {what}'s device")
    return workspace


def _rows(t, name: str, dev):
    """(R, N, row stride in floats) of ``t``: float32 [R,N] or [R] on ``dev``, contiguous or a column slice (unit inner stride)"""
    if not (isinstance(t, Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.dim() in (1, 2)):
        raise ValueError(f"{name}: a float32 tensor [R,N] or [R] on the device of the call's other tensors")
    R, N = int(t.shape[0]), (int(t.shape[1]) if t.dim() == 2 else 1)
    if N < 1:
        raise ValueError(f"{name}: at least one sample per ray, got {tuple(t.shape)}")
    if t.dim() == 1:
        stride = 1 if R <= 1 else int(t.stride(0))              # one column of a wider buffer: its row stride
        if stride < 1:
            raise ValueError(f"{name}: a vector [R] with a positive stride")
    else:
        stride = N if R <= 1 else int(t.stride(0))
        if (N > 1 and t.stride(1) != 1) or stride < N:
            raise ValueError(f"{name}: contiguous [R,N], or a column slice of a wider contiguous buffer (unit inner stride)")
    return R, N, stride


def _sum_slot(out, slot, dev):
    """(out, slot) of a double sum: ``out`` a contiguous 1-d float64 device tensor and ``slot`` an index into it; for None a
    fresh one-element tensor on ``dev`` and slot 0.  ``dev`` only places that tensor: a caller's ``out`` is taken on whatever
    device it lives, as it always was"""
    if out is None:
        return torch.empty((1,), dtype=torch.float64, device=dev), 0
    if not (isinstance(out, Tensor) and out.is_cuda and out.dtype == torch.float64 and out.dim() == 1 and out.is_contiguous()):
        raise ValueError("out: a contiguous 1-d float64 device tensor")
    slot = int(slot)
    if not 0 <= slot < out.numel():
        raise ValueError(f"slot {slot} out of range [0, {out.numel()})")
    return out, slot


def _c2w_host(c2w) -> np.ndarray:
    """camera-to-world matrix (tensor or array) -> contiguous host float32 [3,4]"""
    c2w = c2w.detach().cpu().numpy() if isinstance(c2w, Tensor) else np.asarray(c2w)
    return np.ascontiguousarray(c2w.astype(np.float32)[:3, :4])


# ---- a1 -------------------------------------------------------------------------------------------
def get_rays(H: int, W: int, K, c2w, row0: int = 0, row1: Optional[int] = None, near: float = 0.0,
             far: float = 1.0, device=None, want_batch: bool = False):
    """rays_o, rays_d, viewdirs [R,3] (and ray_batch [R,11]) for image rows [row0,row1)."""
    lib = _lib.load()
    row1 = H if row1 is None else row1
    device = torch.device(device if device is not None else (c2w.device if isinstance(c2w, Tensor) and c2w.is_cuda else "cuda"))
    c2w_h = _c2w_host(c2w)
    R = (row1 - row0) * W
    o = torch.empty((R, 3), dtype=torch.float32, device=device)
    d = torch.empty_like(o)
    v = torch.empty_like(o)
    b = torch.empty((R, 11), dtype=torch.float32, device=device) if want_batch else None
    check(lib.ns_get_rays(H, W, float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]),
                          c2w_h.ctypes.data_as(C.c_void_p), row0, row1, float(near), float(far),
                          _ptr(o), _ptr(d), _ptr(v), _ptr(b), _stream(device)), "ns_get_rays")
    return (o, d, v, b) if want_batch else (o, d, v)


# ---- training ray batches from a device-resident dataset (ray_batches.py holds the dataset and the generator) -----------
def ray_dataset(images, poses, hwf_or_K, i_train, white_bkgd: bool = False, device="cuda"):
    """Upload a scene once: ray_batches.DeviceRayDataset."""
    from .ray_batches import DeviceRayDataset

    return DeviceRayDataset(images, poses, hwf_or_K, i_train, white_bkgd=white_bkgd, device=device)


def ray_batch_gather(dataset, image_idx, pixels, want_viewdirs: bool = False, out=None):
    """ns_ray_batch_gather: (batch_rays [2,B,3], target [B,3][, viewdirs]) of the named pixels (DeviceRayDataset.gather)."""
    return dataset.gather(image_idx, pixels, want_viewdirs=want_viewdirs, out=out)


def ray_batch_draw(dataset, B: int, step: int = 0, window=None, scope: str = "per_image", seed: int = 0, **kw):
    """ns_ray_batch_draw: batch ``step`` drawn in the kernel, without replacement (DeviceRayDataset.draw)."""
    return dataset.draw(B, step=step, window=window, scope=scope, seed=seed, **kw)


# ---- placed samples against the field's depth (not an operator of the reference: nerf_utils.py:311-317 on the host) ----
def depth_sqerr_workspace_bytes(R: int, N: int) -> int:
    """ns_depth_sqerr_workspace_bytes: the partial sums ``depth_sqerr`` needs for R rays of N samples (0: a shape it refuses)"""
    return int(_lib.load().ns_depth_sqerr_workspace_bytes(int(R), int(N)))


def depth_sqerr(z, ref, out=None, slot: int = 0, workspace=None):
    """ns_depth_sqerr: sum over rays and samples of (double)(fl32(z[r, k] - ref[r]))^2, in double on the device -- the numerator
    of render_path's ``MSE:`` under compare_nerf (mse_loss(max_z_vals, depth_net_z_vals)) with ``z`` the placed samples, and of
    the training's depth_net_loss with ``z`` the DepthNet's own depth.  ``z``: fp32 [R,N] or [R] on the device, contiguous or a
    column slice with unit inner stride; ``ref``: fp32 [R] or [R,1] on the same device.  Returns a 1-element float64 device
    tensor, or writes ``out[slot]`` (``out``: a contiguous 1-d float64 device tensor) and returns ``out``.  ``workspace``: a
    contiguous 8-byte-aligned device tensor of at least ``depth_sqerr_workspace_bytes(R, N)`` bytes (None: allocated for the
    call).  The same bits on every call; a NaN anywhere makes the sum NaN.  Nothing is read back: see ``mse_from_sqerr``.  What
    is wrong with the arguments raises ValueError before any launch."""
    if not (isinstance(z, Tensor) and z.is_cuda and z.dtype == torch.float32 and z.dim() in (1, 2)):
        raise ValueError("z: a float32 device tensor [R,N] or [R]")
    R, N, stride = _rows(z, "z", z.device)
    if R < 1:
        raise ValueError(f"z: at least one ray and one sample, got {tuple(z.shape)}")
    if R * N >= 2 ** 31:
        raise ValueError(f"z: R * N = {R * N} is not below 2^31")
    if not (isinstance(ref, Tensor) and ref.is_cuda and ref.device == z.device and ref.dtype == torch.float32
            and tuple(ref.shape) in ((R,), (R, 1)) and ref.is_contiguous()):
        raise ValueError(f"ref: a contiguous float32 tensor of shape ({R},) or ({R}, 1) on z's device")
    out, slot = _sum_slot(out, slot, z.device)
    workspace = _scratch(workspace, depth_sqerr_workspace_bytes(R, N), z.device, "z")
    check(_lib.load().ns_depth_sqerr(_ptr(z), stride, _ptr(ref), R, N, C.c_void_p(out.data_ptr() + 8 * slot), _ptr(workspace),
                                     _stream(z.device)), "ns_depth_sqerr")
    return out


def mse_from_sqerr(sums, n_values):
    """sum / n_values in float64, on the host: the mean squared error of ``depth_sqerr`` sums ``sums`` (a device or host tensor,
    an array or a number) over ``n_values`` = R * N values each.  A device tensor is read back here, once."""
    if hasattr(sums, "detach"):
        sums = sums.detach().cpu().numpy()
    return np.asarray(sums, dtype=np.float64) / np.asarray(n_values, dtype=np.float64)


# ---- the scene's point cloud (experiments/plot.py:13-22 all_pts[all_weights >= t], selected on the device) ---------------
def cloud_workspace_bytes(R: int, N: int) -> int:
    """ns_cloud_workspace_bytes: the per-share counts ``cloud_append`` needs for R rays of N samples (0: a shape it refuses, or
    no rays)"""
    return int(_lib.load().ns_cloud_workspace_bytes(int(R), int(N)))


def cloud_append(cloud, o, d, z, w, rgb=None, min_weight: float = 0.0):
    """ns_cloud_append: append the samples of one batch of rays whose weight passes the threshold to ``cloud`` (a PointCloud), on
    the device and in order -- ray-major, sample-minor, call after call: ``torch.cat(all_pts)[torch.cat(all_weights) >= t]`` of
    the reference's scene data (experiments/plot.py:13-22, utils.py:36-43).  ``o``, ``d``: contiguous fp32 [R,3]; ``z``, ``w``:
    fp32 [R,N] (or [R]), contiguous or column slices of wider buffers; ``rgb``: the rays' colours [R,3] with unit inner stride
    and any row stride >= 3 (``shard[:, :3]`` of an [R,4] tensor), required iff the cloud keeps colours.  A kept record is
    ``o + d * z`` (ops.points_along_rays' bits), the weight and the ray's colour; a NaN weight is dropped.  Records beyond the
    cloud's capacity are counted, not written.  Nothing is read back; what is wrong with the arguments raises ValueError before
    any launch.  Returns ``cloud``."""
    if not isinstance(cloud, PointCloud):
        raise ValueError("cloud: an ops.PointCloud")
    dev = cloud.count_dev.device
    for name, t in (("o", o), ("d", d)):
        if not (isinstance(t, Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.dim() == 2
                and t.shape[1] == 3 and t.is_contiguous()):
            raise ValueError(f"{name}: a contiguous float32 tensor [R,3] on the cloud's device")
    R = int(o.shape[0])
    if int(d.shape[0]) != R:
        raise ValueError("o and d: the same number of rays")
    Rz, N, z_stride = _rows(z, "z", dev)
    Rw, Nw, w_stride = _rows(w, "w", dev)
    if (Rz, Rw, Nw) != (R, R, N):
        raise ValueError(f"z and w: both [{R}, N], got {tuple(z.shape)} and {tuple(w.shape)}")
    if R * N >= 2 ** 31:
        raise ValueError(f"R * N = {R * N} is not below 2^31")
    if (rgb is not None) != cloud.colours:
        raise ValueError("rgb: required by a cloud with colours, and only by it")
    rgb_stride = 0
    if rgb is not None:
        if not (isinstance(rgb, Tensor) and rgb.is_cuda and rgb.device == dev and rgb.dtype == torch.float32 and rgb.dim() == 2
                and tuple(rgb.shape) == (R, 3) and (R == 0 or rgb.stride(1) == 1) and (R <= 1 or rgb.stride(0) >= 3)):
            raise ValueError(f"rgb: a float32 tensor [{R},3] on the cloud's device, unit inner stride, row stride >= 3")
        rgb_stride = 3 if R <= 1 else int(rgb.stride(0))
    min_weight = float(min_weight)
    if R == 0:
        return cloud
    check(_lib.load().ns_cloud_append(_ptr(o), _ptr(d), _ptr(z), z_stride, _ptr(w), w_stride, _ptr(rgb), rgb_stride, R, N,
                                      min_weight, _ptr(cloud.pts), _ptr(cloud.weights), _ptr(cloud.rgb), cloud.capacity,
                                      _ptr(cloud.count_dev), _ptr(cloud._workspace_for(R, N)), _stream(dev)),
          "ns_cloud_append")
    return cloud


class PointCloud:
    """The compact arrays ns_cloud_append fills: ``pts`` [capacity,3], ``weights`` [capacity], ``rgb`` [capacity,3] (None without
    ``colours``), the int64 record counter ``count_dev`` (one element, zeroed) and a workspace that only ever grows -- all on the
    device.  ``capacity`` = 0 counts without storing.  The counter keeps counting beyond the capacity, so ``count()`` -- one
    8-byte readback -- is the capacity a rerun needs."""

    def __init__(self, capacity: int, colours: bool = False, device="cuda"):
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity must be >= 0")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"a PointCloud lives on the GPU (got {device}); this path has no CPU fallback")
        self.capacity, self.colours = capacity, bool(colours)
        self.pts = torch.empty((capacity, 3), dtype=torch.float32, device=device)
        self.weights = torch.empty((capacity,), dtype=torch.float32, device=device)
        self.rgb = torch.empty((capacity, 3), dtype=torch.float32, device=device) if colours else None
        self.count_dev = torch.zeros((1,), dtype=torch.int64, device=device)
        self._workspace = None

    def _workspace_for(self, R: int, N: int):
        need = cloud_workspace_bytes(R, N)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty((need,), dtype=torch.uint8, device=self.count_dev.device)
        return self._workspace

    def append(self, o, d, z, w, rgb=None, min_weight: float = 0.0):
        return cloud_append(self, o, d, z, w, rgb=rgb, min_weight=min_weight)

    def count(self) -> int:
        """the number of records kept so far, those beyond the capacity included (reads the counter back)"""
        return int(self.count_dev.cpu()[0])

    def tensors(self, truncate: bool = False):
        """(pts[:M], weights[:M], rgb[:M] or None), M = count().  More records than the capacity: RuntimeError naming the capacity
        needed, or with ``truncate`` the first ``capacity`` records."""
        M = self.count()
        if M > self.capacity:
            if not truncate:
                raise RuntimeError(f"the point cloud kept {M} records but has room for {self.capacity}: "
                                   f"a capacity of {M} is needed (or tensors(truncate=True))")
            M = self.capacity
        return self.pts[:M], self.weights[:M], (self.rgb[:M] if self.colours else None)


# ---- the field's isosurface mesh (marching tetrahedra on the Kuhn split, on the device; not in the reference) -------------
def mesh_workspace_bytes(Gx: int, Gy: int, Gz: int) -> int:
    """ns_mesh_workspace_bytes: the per-share counts ``mesh_extract`` needs for a Gx x Gy x Gz lattice (0: a shape it refuses)"""
    return int(_lib.load().ns_mesh_workspace_bytes(int(Gx), int(Gy), int(Gz)))


def _mesh_lattice(sigma):
    """(Gx, Gy, Gz, stride in floats) of ``sigma``: float32 [Gz,Gy,Gx] on the device, contiguous or one column of a contiguous
    [Gz,Gy,Gx,C] array (``raw[..., 3]``)"""
    if not (isinstance(sigma, Tensor) and sigma.is_cuda and sigma.dtype == torch.float32 and sigma.dim() == 3):
        raise ValueError("sigma: a float32 device tensor [Gz,Gy,Gx]")
    Gz, Gy, Gx = (int(v) for v in sigma.shape)
    if min(Gx, Gy, Gz) < 2:
        raise ValueError(f"sigma: at least two lattice points along every axis, got {tuple(sigma.shape)}")
    if Gx * Gy * Gz >= 2 ** 31:
        raise ValueError(f"sigma: Gx * Gy * Gz = {Gx * Gy * Gz} is not below 2^31")
    stride = int(sigma.stride(2))
    if stride < 1 or tuple(sigma.stride()) != (Gy * Gx * stride, Gx * stride, stride):
        raise ValueError("sigma: contiguous [Gz,Gy,Gx], or one column of a contiguous [Gz,Gy,Gx,C] array")
    return Gx, Gy, Gz, stride


def mesh_extract(sigma, iso, lo, h, capacity: Optional[int] = None, workspace=None):
    """ns_mesh_extract: the triangles of the isosurface ``sigma == iso`` of a lattice, by marching tetrahedra on the device, in
    the order (cell, tetrahedron, triangle) and wound from inside (sigma >= iso) to outside.  ``sigma``: fp32 [Gz,Gy,Gx] on the
    device, contiguous or a column view such as ``raw[..., 3]`` of a contiguous [Gz,Gy,Gx,4] array; lattice point (i, j, k)
    lies at ``lo + (float32) idx * h`` per axis (``lo``, ``h``: three numbers each, rounded to float32; h > 0).  A cell with a
    NaN or infinite corner emits nothing and is counted.  ``capacity`` None: a counting call, ONE readback of the two counters,
    an allocation of exactly that many triangles and the emitting call; given: one emitting call and one readback, and the
    tensors returned are cut to min(n_triangles, capacity) -- triangles beyond it are counted, never written.  ``workspace``: a
    contiguous 8-byte-aligned device tensor of at least ``mesh_workspace_bytes(Gx, Gy, Gz)`` bytes (None: allocated).  Returns
    dict(triangles [n,3,3] fp32, keys [n,3] int64, n_triangles, n_skipped): a vertex's key names its lattice edge, and equal
    keys carry equal position bits (``mesh_weld``).  What is wrong with the arguments raises ValueError before any launch."""
    Gx, Gy, Gz, stride = _mesh_lattice(sigma)
    dev = sigma.device
    lo3, h3 = [float(np.float32(v)) for v in lo], [float(np.float32(v)) for v in h]
    if len(lo3) != 3 or len(h3) != 3:
        raise ValueError("lo and h: three numbers each")
    if capacity is not None and int(capacity) < 0:
        raise ValueError("capacity must be >= 0")
    workspace = _scratch(workspace, mesh_workspace_bytes(Gx, Gy, Gz), dev, "sigma")
    lib = _lib.load()
    counters = torch.empty((2,), dtype=torch.int64, device=dev)

    def call(tri, keys, cap):
        check(lib.ns_mesh_extract(_ptr(sigma), stride, Gx, Gy, Gz, float(iso), *lo3, *h3, _ptr(tri), _ptr(keys), cap,
                                  _ptr(counters), _ptr(workspace), _stream(dev)), "ns_mesh_extract")

    def outputs(cap):
        return (torch.empty((cap, 3, 3), dtype=torch.float32, device=dev), torch.empty((cap, 3), dtype=torch.int64, device=dev))

    if capacity is None:
        call(None, None, 0)
        n_triangles, n_skipped = (int(v) for v in counters.cpu())              # the one readback
        capacity = n_triangles
        tri, keys = outputs(capacity)
        if capacity > 0:
            call(tri, keys, capacity)                                          # counts the same lattice again
    else:
        capacity = int(capacity)
        tri, keys = outputs(capacity)
        call(tri, keys, capacity)
        n_triangles, n_skipped = (int(v) for v in counters.cpu())              # the one readback
    n = min(n_triangles, capacity)
    return {"triangles": tri[:n], "keys": keys[:n], "n_triangles": n_triangles, "n_skipped": n_skipped}


def mesh_weld(triangles, keys):
    """(vertices [V,3], faces [F,3] int64) of ``mesh_extract``'s triangles, on the device: one vertex per distinct key, in
    ascending key order (``torch.unique(keys, return_inverse=True)``); its position is that of any occurrence, since all
    occurrences of a key are bit-identical."""
    if not (isinstance(triangles, Tensor) and isinstance(keys, Tensor) and triangles.dim() == 3 and keys.dim() == 2
            and tuple(triangles.shape[1:]) == (3, 3) and tuple(keys.shape) == (triangles.shape[0], 3)
            and keys.dtype == torch.int64 and keys.device == triangles.device):
        raise ValueError("triangles [n,3,3] and keys [n,3] int64 on one device")
    unique, inverse = torch.unique(keys.reshape(-1), return_inverse=True)
    vertices = torch.empty((unique.shape[0], 3), dtype=triangles.dtype, device=triangles.device)
    vertices[inverse] = triangles.reshape(-1, 3)
    return vertices, inverse.reshape(-1, 3)


def mesh_components_workspace_bytes(n_vertices: int, n_faces: int) -> int:
    """ns_mesh_components_workspace_bytes: the counters ``mesh_components`` needs (0: a shape it refuses)"""
    return int(_lib.load().ns_mesh_components_workspace_bytes(int(n_vertices), int(n_faces)))


def mesh_components(faces, n_vertices: int, workspace=None):
    """ns_mesh_components: the connected components of a mesh's faces, on the device.  ``faces``: int64 contiguous [F,3] on the
    device, as ``mesh_weld`` returns them; two vertices are connected iff a chain of faces joins them (a shared vertex is
    enough).  A face with an index outside [0, n_vertices) joins nothing and is counted.  ``workspace``: a contiguous
    8-byte-aligned device tensor of at least ``mesh_components_workspace_bytes(n_vertices, F)`` bytes (None: allocated); what it
    holds does not matter.  Returns dict(labels int32 [V]: the smallest vertex index of the vertex's component; triangles int32
    [V] and vertices int32 [V]: at a root ``r == labels[r]`` the faces and the vertices of its component, 0 elsewhere;
    n_components; n_ignored) after ONE readback of the two counters.  What is wrong with the arguments raises ValueError before
    any launch.  Not part of this: per-component area or volume, and meshes of 2^31 vertices or faces or more."""
    if not (isinstance(faces, Tensor) and faces.is_cuda and faces.dtype == torch.int64 and faces.dim() == 2
            and faces.shape[1] == 3 and faces.is_contiguous()):
        raise ValueError("faces: a contiguous int64 device tensor [F,3]")
    V, F = int(n_vertices), int(faces.shape[0])
    if V < 0 or V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError(f"n_vertices = {V} and F = {F} must lie in [0, 2^31)")
    dev = faces.device
    workspace = _scratch(workspace, mesh_components_workspace_bytes(V, F), dev, "faces")
    labels, triangles, vertices = (torch.empty((V,), dtype=torch.int32, device=dev) for _ in range(3))
    counters = torch.empty((2,), dtype=torch.int64, device=dev)
    check(_lib.load().ns_mesh_components(_ptr(faces), F, V, _ptr(labels), _ptr(triangles), _ptr(vertices), _ptr(counters),
                                         _ptr(workspace), _stream(dev)), "ns_mesh_components")
    n_components, n_ignored = (int(v) for v in counters.cpu())                 # the one readback
    return {"labels": labels, "triangles": triangles, "vertices": vertices, "n_components": n_components,
            "n_ignored": n_ignored}


def mesh_normals_workspace_bytes(n_vertices: int) -> int:
    """ns_mesh_normals_workspace_bytes: the per-share counts ``mesh_normals`` needs for that many keys (0: a count it refuses, or
    none)"""
    return int(_lib.load().ns_mesh_normals_workspace_bytes(int(n_vertices)))


def mesh_normals(sigma, iso, h, keys, workspace=None):
    """ns_mesh_normals: unit normals of mesh vertices from the density lattice they were cut from, on the device -- the
    finite-difference gradient of ``sigma`` (central, one-sided on the lattice boundary) interpolated along each vertex's own
    lattice edge, negated (it points outward, from sigma >= iso to below) and normalised in fp64; a function of the edge alone.
    ``sigma``: what ``mesh_extract`` takes, and ``h`` its three spacings.  ``keys``: int64 on sigma's device, any shape -- [V],
    such as ``torch.unique`` of ``mesh_extract``'s keys (``mesh_weld``'s vertex order), or its [n,3] as they are; they need not
    be sorted or distinct.  ``workspace``: a contiguous 8-byte-aligned device tensor of at least
    ``mesh_normals_workspace_bytes(keys.numel())`` bytes (None: allocated).  Returns dict(normals fp32 keys.shape + (3,),
    n_degenerate: vertices whose gradient is zero or not finite, normal (0, 0, 0); n_invalid: keys that name no lattice edge,
    normal (0, 0, 0)) after ONE readback of the two counters.  What is wrong with the arguments raises ValueError before any
    launch."""
    Gx, Gy, Gz, stride = _mesh_lattice(sigma)
    dev = sigma.device
    if not (isinstance(keys, Tensor) and keys.dtype == torch.int64 and keys.device == dev):
        raise ValueError("keys: an int64 tensor on sigma's device")
    h3 = [float(np.float32(v)) for v in h]
    if len(h3) != 3 or not all(np.isfinite(v) and v > 0.0 for v in h3):
        raise ValueError("h: three finite positive numbers")
    iso = float(np.float32(iso))
    if not np.isfinite(iso):
        raise ValueError("iso must be finite")
    flat = keys.reshape(-1).contiguous()
    V = int(flat.shape[0])
    if V >= 2 ** 31:
        raise ValueError(f"{V} keys are not below 2^31")
    workspace = _scratch(workspace, mesh_normals_workspace_bytes(V), dev, "sigma")
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    counters = torch.empty((2,), dtype=torch.int64, device=dev)
    check(_lib.load().ns_mesh_normals(_ptr(sigma), stride, Gx, Gy, Gz, iso, *h3, _ptr(flat), V, _ptr(normals), _ptr(counters),
                                      _ptr(workspace), _stream(dev)), "ns_mesh_normals")
    n_degenerate, n_invalid = (int(v) for v in counters.cpu())                 # the one readback
    return {"normals": normals.reshape(tuple(keys.shape) + (3,)), "n_degenerate": n_degenerate, "n_invalid": n_invalid}


def mesh_raster_workspace_bytes(n_vertices: int, n_faces: int, H: int, W: int) -> int:
    """ns_mesh_raster_workspace_bytes: the z-buffer words, projected vertices and face list ``mesh_rasterize`` needs (0: a shape
    it refuses, or no face)"""
    return int(_lib.load().ns_mesh_raster_workspace_bytes(int(n_vertices), int(n_faces), int(H), int(W)))


def mesh_rasterize(vertices, faces, c2w, H, W, K, near, rgb=None, background=0.0, cull=0, workspace=None):
    """ns_mesh_raster: a mesh rasterised from the pinhole camera (H, W, K, c2w) of ``get_rays``, on the device -- a z-buffer frame
    that sits on the field's: pixel (i, j) is the ray through (i - cx) / fx, and ``depth`` is the one-call renderers' ``depth``
    extra's unit (the ray parameter along the unnormalised direction).  ``vertices``: fp32 contiguous [V,3] on the device;
    ``faces``: int64 contiguous [F,3] there, as ``mesh_weld`` returns them; ``rgb``: fp32 contiguous [V,3] vertex colours, or
    None (no colour frame).  ``near`` > 0: a face with a vertex nearer than that (or behind the camera, or farther than 2^20
    pixels off the axis) is dropped and counted -- there is no near-plane clipping.  ``cull``: 0 none, 1 back faces, 2 front
    faces (front: ``mesh_extract``'s outward winding seen from outside).  ``workspace``: a contiguous 8-byte-aligned device
    tensor of at least ``mesh_raster_workspace_bytes(V, F, H, W)`` bytes (None: allocated); what it holds does not matter.
    Returns dict(depth fp32 [H*W]: 0 where no face is; tri int32 [H*W]: the face seen, -1 where none; rgb fp32 [H*W,3] or None:
    the colours interpolated perspective-correctly, ``background`` where no face is; n_clipped; n_degenerate: faces of zero
    area on the screen; n_invalid: faces with an index outside [0, V); n_covered: pixels with a face) after ONE readback of
    the four counters; the frames stay on the device.  The same bits on every call.  What is wrong with the arguments raises
    ValueError before any launch."""
    if not (isinstance(vertices, Tensor) and vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 2
            and vertices.shape[1] == 3 and vertices.is_contiguous()):
        raise ValueError("vertices: a contiguous float32 device tensor [V,3]")
    dev = vertices.device
    if not (isinstance(faces, Tensor) and faces.device == dev and faces.dtype == torch.int64 and faces.dim() == 2
            and faces.shape[1] == 3 and faces.is_contiguous()):
        raise ValueError("faces: a contiguous int64 tensor [F,3] on vertices' device")
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    if rgb is not None and not (isinstance(rgb, Tensor) and rgb.device == dev and rgb.dtype == torch.float32
                                and tuple(rgb.shape) == (V, 3) and rgb.is_contiguous()):
        raise ValueError(f"rgb: a contiguous float32 tensor ({V}, 3) on vertices' device, or None")
    H, W, cull = int(H), int(W), int(cull)
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"H and W must lie in [1, 16384], got {H} x {W}")
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError(f"V = {V} and F = {F} must be below 2^31")
    if cull not in (0, 1, 2):
        raise ValueError(f"cull: 0 (none), 1 (back faces) or 2 (front faces), got {cull}")
    near, background = float(np.float32(near)), float(np.float32(background))
    if not (np.isfinite(near) and near > 0.0):
        raise ValueError("near must be finite and positive")
    if not np.isfinite(background):
        raise ValueError("background must be finite")
    c2w_h = _c2w_host(c2w)
    cam = [float(np.float32(v)) for v in (K[0][0], K[1][1], K[0][2], K[1][2])]
    if not (np.isfinite(c2w_h).all() and np.isfinite(cam).all() and cam[0] != 0.0 and cam[1] != 0.0):
        raise ValueError("c2w and K must be finite, fx and fy not 0")
    workspace = _scratch(workspace, mesh_raster_workspace_bytes(V, F, H, W), dev, "vertices")
    depth = torch.empty((H * W,), dtype=torch.float32, device=dev)
    tri = torch.empty((H * W,), dtype=torch.int32, device=dev)
    frame = torch.empty((H * W, 3), dtype=torch.float32, device=dev) if rgb is not None else None
    counters = torch.empty((4,), dtype=torch.int64, device=dev)
    # an empty vertex tensor has no address, and the entry asks for one wherever there are faces (all of them invalid, then)
    vertex_ptr = _ptr(vertices) if V > 0 else _ptr(counters)
    check(_lib.load().ns_mesh_raster(vertex_ptr, V, _ptr(faces), F, _ptr(rgb), c2w_h.ctypes.data_as(C.c_void_p), *cam, H, W,
                                     near, cull, background, _ptr(depth), _ptr(tri), _ptr(frame), _ptr(counters),
                                     _ptr(workspace), _stream(dev)), "ns_mesh_raster")
    n_clipped, n_degenerate, n_invalid, n_covered = (int(v) for v in counters.cpu())     # the one readback
    return {"depth": depth, "tri": tri, "rgb": frame, "n_clipped": n_clipped, "n_degenerate": n_degenerate,
            "n_invalid": n_invalid, "n_covered": n_covered}


def mesh_select(vertices, faces, labels, keep, extras=()):
    """The part of a mesh whose components are kept -- plain torch on whatever device the tensors live on, no kernel of this
    library.  ``vertices`` [V,...], ``faces`` int64 [F,3], ``labels`` [V] as ``mesh_components`` returns them, ``keep`` bool [V],
    read at the component roots only: vertex v stays iff ``keep[labels[v]]``, a face iff its first vertex does (a face with an
    index outside [0, V) never does).  Returns dict(vertices: the kept ones in ascending index order -- ascending key order for
    ``mesh_weld``'s --; faces: the kept ones in their original order, renumbered; extras: every tensor of ``extras`` (one row per
    vertex, such as colours; a None stays None) cut as the vertices are; index int64 [V]: the new index of an old vertex, -1 for
    a dropped one)."""
    V = int(labels.shape[0])
    if not (vertices.shape[0] == V and keep.shape == labels.shape and keep.dtype == torch.bool and faces.dim() == 2
            and faces.shape[1] == 3 and all(e is None or e.shape[0] == V for e in extras)):
        raise ValueError("vertices [V,...], faces [F,3], labels [V], keep bool [V], extras of V rows each")
    faces = faces.long()
    kept_vertex = keep[labels.long()]
    index = torch.where(kept_vertex, torch.cumsum(kept_vertex, 0) - 1, torch.full_like(labels, -1, dtype=torch.int64))
    in_range = ((faces >= 0) & (faces < V)).all(dim=1)
    first = faces[:, 0].clamp(0, max(V - 1, 0))
    kept_face = in_range & kept_vertex[first] if V > 0 else in_range            # V == 0: no face is in range
    return {"vertices": vertices[kept_vertex], "faces": index[faces[kept_face]],
            "extras": tuple(None if e is None else e[kept_vertex] for e in extras), "index": index}


def _cluster_lattice(lo, cell, dims):
    """(lo [3], cell [3] as float32 values, dims [3]) of ``mesh_simplify``'s cluster lattice, or ValueError: what
    ns_mesh_simplify refuses (csrc/ns_mesh_cluster.h's lattice_ok)"""
    try:
        lo3, cell3 = [float(np.float32(v)) for v in lo], [float(np.float32(v)) for v in cell]
        dims3 = [int(v) for v in dims]
        whole = all(float(v) == int(v) for v in dims)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError(f"lo, cell and dims: three numbers each ({e})") from e
    if len(lo3) != 3 or len(cell3) != 3 or len(dims3) != 3:
        raise ValueError("lo, cell and dims: three numbers each")
    if not all(np.isfinite(v) for v in lo3):
        raise ValueError(f"lo must be finite, got {lo3}")
    if not all(np.isfinite(v) and v > 0.0 for v in cell3):
        raise ValueError(f"cell must be finite and positive in float32, got {cell3}")
    if not (whole and all(1 <= c <= 2 ** 15 for c in dims3) and dims3[0] * dims3[1] * dims3[2] <= 2 ** 24):
        raise ValueError(f"dims: three whole numbers in [1, 2^15] whose product is at most 2^24, got {list(dims)}")
    return lo3, cell3, dims3


def mesh_simplify_workspace_bytes(n_vertices: int, n_faces: int, dims) -> int:
    """ns_mesh_simplify_workspace_bytes: the counters, per-share face counts and the dense cluster table (40 bytes per cell)
    ``mesh_simplify`` needs (0: a shape it refuses)"""
    Cx, Cy, Cz = (int(v) for v in dims)
    fits = all(-2 ** 31 <= c < 2 ** 31 for c in (Cx, Cy, Cz))
    return int(_lib.load().ns_mesh_simplify_workspace_bytes(int(n_vertices), int(n_faces), Cx, Cy, Cz)) if fits else 0


def _first_of_each_vertex_set(faces, n_vertices: int):
    """bool [F]: True where no earlier face has the same three vertices as a set -- plain torch.  The rows sorted, then two
    rounds of (pair -> dense id): id * n_vertices + vertex stays below 2^62"""
    F = int(faces.shape[0])
    if F == 0:
        return torch.zeros((0,), dtype=torch.bool, device=faces.device)
    s = torch.sort(faces, dim=1).values
    pair = torch.unique(s[:, 0] * n_vertices + s[:, 1], return_inverse=True)[1]
    sets, which = torch.unique(pair * n_vertices + s[:, 2], return_inverse=True)
    order = torch.arange(F, device=faces.device)
    first = torch.full((sets.shape[0],), F, dtype=torch.int64, device=faces.device).scatter_reduce_(0, which, order, "amin")
    return first[which] == order


def mesh_simplify(vertices, faces, lo, cell, dims, extras=(), dedupe=True, workspace=None):
    """ns_mesh_simplify: a mesh simplified by vertex clustering on the device.  The cluster lattice has ``dims`` = (Cx, Cy, Cz)
    cells of size ``cell`` from ``lo`` on (three numbers each, rounded to float32; a vertex outside belongs to the nearest
    boundary cell); the vertices of a cell collapse onto ONE OF THEM, the member nearest the cell's centroid (a tie: the smaller
    index), so every vertex of the result is an input vertex bit for bit and its colour, normal and key stay valid.  A face
    with two corners in one cell is dropped.  ``vertices``: fp32 contiguous [V,3] on the device; ``faces``: int64 contiguous
    [F,3] there.  ONE call of the entry with room for F faces and ONE readback of its counters; then the renumbering of
    ``mesh_select``, in plain torch: the kept vertices are the representatives in ascending input index, the kept faces stay
    in their order and winding, every tensor of ``extras`` (one row per vertex; a None stays None) is cut as the vertices are.
    ``dedupe``: a face whose three vertices, as a set, already occurred in an earlier kept face is dropped and counted --
    collapsing a thin sheet produces such faces in pairs; the first occurrence stays, with its winding.  ``workspace``: a
    contiguous 8-byte-aligned device tensor of at least ``mesh_simplify_workspace_bytes(V, F, dims)`` bytes (None: allocated);
    what it holds does not matter.  Returns dict(vertices, faces, extras, index int64 [V]: old -> new vertex, -1 where it is not
    kept; rep int32 [V]: the representative of every input vertex in the input numbering, -1 for a non-finite one; n_collapsed;
    n_invalid: faces with an index outside [0, V); n_nonfinite: vertices with a NaN or infinite coordinate; n_nonfinite_faces:
    faces on one; n_duplicate; n_clusters: the occupied cells, which is the number of vertices kept).  The same bits on every
    call.  What is wrong with the arguments raises ValueError before any launch.  Not part of this: quadric error metrics, new
    vertex positions at the centroid, manifold or topology guarantees, meshes of 2^31 vertices or faces or more."""
    lo3, cell3, dims3 = _cluster_lattice(lo, cell, dims)
    if not (isinstance(vertices, Tensor) and vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 2
            and vertices.shape[1] == 3 and vertices.is_contiguous()):
        raise ValueError("vertices: a contiguous float32 device tensor [V,3]")
    dev = vertices.device
    if not (isinstance(faces, Tensor) and faces.device == dev and faces.dtype == torch.int64 and faces.dim() == 2
            and faces.shape[1] == 3 and faces.is_contiguous()):
        raise ValueError("faces: a contiguous int64 tensor [F,3] on vertices' device")
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError(f"V = {V} and F = {F} must be below 2^31")
    extras = tuple(extras)
    if not all(e is None or (isinstance(e, Tensor) and e.device == dev and e.dim() >= 1 and e.shape[0] == V) for e in extras):
        raise ValueError(f"extras: tensors of {V} rows on vertices' device, or None")
    workspace = _scratch(workspace, mesh_simplify_workspace_bytes(V, F, dims3), dev, "vertices")
    rep = torch.empty((V,), dtype=torch.int32, device=dev)
    mapped = torch.empty((F, 3), dtype=torch.int64, device=dev)
    counters = torch.empty((6,), dtype=torch.int64, device=dev)
    lo_h, cell_h, dims_h = np.array(lo3, np.float32), np.array(cell3, np.float32), np.array(dims3, np.int32)
    host = lambda a: a.ctypes.data_as(C.c_void_p)                              # noqa: E731
    check(_lib.load().ns_mesh_simplify(_ptr(vertices) if V else None, V, _ptr(faces) if F else None, F, host(lo_h), host(cell_h),
                                       host(dims_h), _ptr(rep) if V else None, _ptr(mapped) if F else None, F, _ptr(counters),
                                       _ptr(workspace), _stream(dev)), "ns_mesh_simplify")
    n_kept, n_collapsed, n_invalid, n_nonfinite, n_nonfinite_faces, n_clusters = (int(v) for v in counters.cpu())   # the one readback
    kept_vertex = rep.long() == torch.arange(V, device=dev)
    index = torch.where(kept_vertex, torch.cumsum(kept_vertex, 0) - 1, torch.full((V,), -1, dtype=torch.int64, device=dev))
    new_faces = index[mapped[:n_kept]]
    n_duplicate = 0
    if dedupe:
        first = _first_of_each_vertex_set(new_faces, max(n_clusters, 1))
        n_duplicate = n_kept - int(first.sum())
        new_faces = new_faces[first]
    return {"vertices": vertices[kept_vertex], "faces": new_faces,
            "extras": tuple(None if e is None else e[kept_vertex] for e in extras), "index": index, "rep": rep,
            "n_collapsed": n_collapsed, "n_invalid": n_invalid, "n_nonfinite": n_nonfinite,
            "n_nonfinite_faces": n_nonfinite_faces, "n_duplicate": n_duplicate, "n_clusters": n_clusters}


# ---- a rendered frame as 8-bit pixels (run_nerf_helpers.py:11 to8b, quantised on the device) -----------------------------
def frame_to8b(rgb, alpha=None, out=None, channels: int = 3):
    """ns_frame_to8b: ``run_nerf_helpers.to8b`` of a rendered frame on the device -- (uint8) trunc(255 * clip(x, 0, 1)), one fp32
    multiply, numpy's bits for every finite x; NaN gives 0.  ``rgb``: what DeviceRayDataset.image_sqerr accepts, fp32 [R,3] on
    the device, contiguous or the ``[:, :3]`` view of a contiguous [R,4] shard.  ``channels``: 3 or 4; with 4 the fourth byte
    is the same map of ``alpha`` (contiguous fp32 [R] or [R,1] on rgb's device), or 255 without one; ``alpha`` with 3 channels
    is ignored.  ``out``: a contiguous uint8 tensor of R * channels elements on rgb's device (a slot of a ring of frames; it
    may start at any byte); None: allocated.  Returns the bytes as a uint8 tensor [R, channels].  Asynchronous on the current
    stream, nothing is read back; what is wrong with the arguments raises before the launch."""
    if not isinstance(rgb, Tensor):
        raise TypeError("rgb must be a torch.Tensor")
    if not rgb.is_cuda:
        raise RuntimeError(f"rgb must live on the GPU (got {rgb.device}); this path has no CPU fallback")
    if not (rgb.dtype == torch.float32 and rgb.dim() == 2 and rgb.shape[1] == 3):
        raise ValueError("rgb: a float32 device tensor of shape (R, 3)")
    R = int(rgb.shape[0])
    if rgb.is_contiguous():
        stride = 3
    elif tuple(rgb.stride()) == (4, 1):
        stride = 4
    else:
        raise ValueError("rgb: contiguous [R,3], or the [:, :3] view of a contiguous [R,4] shard")
    channels = int(channels)
    if channels not in (3, 4):
        raise ValueError(f"channels: 3 or 4, got {channels}")
    if R * 4 >= 2 ** 31:
        raise ValueError(f"rgb: R * 4 = {R * 4} is not below 2^31")
    if alpha is not None and not (isinstance(alpha, Tensor) and alpha.is_cuda and alpha.device == rgb.device
                                  and alpha.dtype == torch.float32 and tuple(alpha.shape) in ((R,), (R, 1))
                                  and alpha.is_contiguous()):
        raise ValueError(f"alpha: a contiguous float32 tensor of shape ({R},) or ({R}, 1) on rgb's device")
    if out is None:
        out = torch.empty((R, channels), dtype=torch.uint8, device=rgb.device)
    elif not (isinstance(out, Tensor) and out.dtype == torch.uint8 and out.device == rgb.device and out.is_contiguous()
              and out.numel() == R * channels):
        raise ValueError(f"out: a contiguous uint8 tensor of {R * channels} elements on rgb's device")
    if R > 0:
        check(_lib.load().ns_frame_to8b(_ptr(rgb), stride, _ptr(alpha) if channels == 4 else None, R, _ptr(out), channels,
                                        _stream(rgb.device)), "ns_frame_to8b")
    return out.view(R, channels)


# ---- the turntable's disparity sequence (Trainer.py:371-376 to8b(disps / np.max(disps)), the divisor kept on the device) ----
def _map_layout(t, name: str):
    """(R, stride in floats) of a per-ray map: a contiguous fp32 [R] on the device, or the [:, 3] view of a contiguous [R,4]
    shard (the one-call renderers' interleaved layout)"""
    if not isinstance(t, Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); this path has no CPU fallback")
    if not (t.dtype == torch.float32 and t.dim() == 1):
        raise ValueError(f"{name}: a float32 device tensor of shape (R,)")
    R = int(t.shape[0])
    if R >= 2 ** 31:
        raise ValueError(f"{name}: R = {R} is not below 2^31")
    if t.is_contiguous():
        return R, 1
    if int(t.stride(0)) == 4:
        return R, 4
    raise ValueError(f"{name}: contiguous [R], or the [:, 3] view of a contiguous [R,4] shard")


def map_max_workspace_bytes(n: int) -> int:
    """ns_map_max_workspace_bytes: the per-workgroup (max, flag) pairs ``map_max`` needs for a map of ``n`` values"""
    return int(_lib.load().ns_map_max_workspace_bytes(int(n)))


def map_max(map, state=None, accumulate: bool = False, workspace=None):
    """ns_map_max: the maximum of a per-ray map folded into a two-float state on the device -- ``np.max(disps)`` of
    Trainer.py:371-376 kept where the frames are, so that the divisor of a whole sequence is never read back between views.
    ``state[0]`` is the maximum over the values that are not NaN (-inf when there are none), ``state[1]`` is 1.0 if a NaN was
    seen and 0.0 otherwise.  ``map``: fp32 [R] on the device, contiguous or the ``[:, 3]`` view of a contiguous [R,4] shard.
    ``state``: a contiguous float32 [2] tensor on map's device (None: allocated).  ``accumulate`` False initialises the state
    from this map alone, True folds the map into the state already there (it needs ``state``): calls over the maps of a
    sequence leave the state of their concatenation.  ``workspace``: a contiguous 8-byte-aligned device tensor of at least
    ``map_max_workspace_bytes(R)`` bytes (None: allocated for the call).  Returns the state tensor.  Asynchronous on the
    current stream, nothing is read back; what is wrong with the arguments raises before the launch."""
    R, stride = _map_layout(map, "map")
    accumulate = bool(accumulate)
    if state is None:
        if accumulate:
            raise ValueError("accumulate=True folds the map into a state: state is required")
        state = torch.empty((2,), dtype=torch.float32, device=map.device)
    elif not (isinstance(state, Tensor) and state.is_cuda and state.device == map.device and state.dtype == torch.float32
              and tuple(state.shape) == (2,) and state.is_contiguous()):
        raise ValueError("state: a contiguous float32 tensor of shape (2,) on map's device")
    workspace = _scratch(workspace, map_max_workspace_bytes(R), map.device, "map")
    check(_lib.load().ns_map_max(_ptr(map) if R else None, stride, R, int(accumulate), _ptr(state),
                                 _ptr(workspace) if R else None, _stream(map.device)), "ns_map_max")
    return state


def map_to8b(map, denom=None, out=None):
    """ns_map_to8b: a per-ray map as 8-bit pixels, (uint8) trunc(255 * clip(x / denom, 0, 1)) -- ``to8b(disps / np.max(disps))``
    of Trainer.py:371-376 with the divisor read from device memory: one correctly rounded fp32 division (numpy's float32 /
    float32), then ``frame_to8b``'s clip, multiply and truncation; a NaN quotient (a NaN value, 0 / 0, inf / inf, a NaN divisor)
    gives 0.  ``map``: as ``map_max``'s.  ``denom``: a float32 device tensor of one element on map's device -- ``state[:1]`` of
    ``map_max`` -- or None: no division.  ``out``: a contiguous uint8 tensor of R elements on map's device (a slot of a ring
    of frames; it may start at any byte); None: allocated.  Returns the bytes as a uint8 tensor [R].  Asynchronous on the
    current stream, nothing is read back; what is wrong with the arguments raises before the launch."""
    R, stride = _map_layout(map, "map")
    if denom is not None and not (isinstance(denom, Tensor) and denom.is_cuda and denom.device == map.device
                                  and denom.dtype == torch.float32 and denom.numel() == 1):
        raise ValueError("denom: a float32 tensor of one element on map's device, or None")
    if out is None:
        out = torch.empty((R,), dtype=torch.uint8, device=map.device)
    elif not (isinstance(out, Tensor) and out.dtype == torch.uint8 and out.device == map.device and out.is_contiguous()
              and out.numel() == R):
        raise ValueError(f"out: a contiguous uint8 tensor of {R} elements on map's device")
    if R > 0:
        check(_lib.load().ns_map_to8b(_ptr(map), stride, R, _ptr(denom), _ptr(out), _stream(map.device)), "ns_map_to8b")
    return out.view(R)


# ---- a2 -------------------------------------------------------------------------------------------
def sphere_intersect(o: Tensor, d: Tensor, radius: float) -> Tuple[Tensor, Tensor]:
    lib = _lib.load()
    o, d = _dev(o, "origin"), _dev(d, "direction")
    R = o.shape[0]
    t = torch.empty((R, 2), dtype=torch.float32, device=o.device)
    p = torch.empty((R, 2, 3), dtype=torch.float32, device=o.device)
    check(lib.ns_sphere_intersect(_ptr(o), _ptr(d), R, float(radius), _ptr(t), _ptr(p), _stream(o.device)),
          "ns_sphere_intersect")
    return t, p


def solve_quadratic(a: Tensor, b: Tensor, c: Tensor) -> Tensor:
    lib = _lib.load()
    a, b, c = _dev(a, "a"), _dev(b, "b"), _dev(c, "c")
    out = torch.empty((2,) + tuple(a.shape), dtype=torch.float32, device=a.device)
    check(lib.ns_solve_quadratic(_ptr(a), _ptr(b), _ptr(c), a.numel(), _ptr(out), _stream(a.device)),
          "ns_solve_quadratic")
    return out


# ---- a3 -------------------------------------------------------------------------------------------
def posenc(x: Tensor, n_freqs: int) -> Tensor:
    lib = _lib.load()
    x = _dev(x, "x")
    d = x.shape[-1]
    M = x.numel() // d
    out = torch.empty(tuple(x.shape[:-1]) + (d * (1 + 2 * n_freqs),), dtype=torch.float32, device=x.device)
    check(lib.ns_posenc(_ptr(x), M, d, n_freqs, _ptr(out), _stream(x.device)), "ns_posenc")
    return out


# ---- packed networks ------------------------------------------------------------------------------
class PackedWeights:
    """Owner of an ns_weights handle (device weight stream)."""

    def __init__(self, handle: int, kind: str, dtype: str, device):
        self.handle = C.c_void_p(handle)
        self.kind, self.dtype, self.device = kind, dtype, device

    @property
    def stream_bytes(self) -> int:
        return int(_lib.load().ns_weights_stream_bytes(self.handle))

    def __del__(self):
        try:
            if self.handle:
                _lib.load().ns_weights_destroy(self.handle)
                self.handle = None
        except Exception:  # interpreter shutdown
            pass


def _host_ptr_array(tensors: Sequence[Tensor]):
    keep = [np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32)) for t in tensors]
    arr = (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
    return arr, keep


def pack_nerf(weights: Sequence[Tensor], biases: Sequence[Tensor], D: int, W: int, skip,
              dtype: Optional[str] = None, device="cuda", use_viewdirs: bool = True, output_ch: int = 4,
              unit_ordered: bool = False) -> PackedWeights:
    """weights/biases in the order pts_linears.0..D-1, then feature_linear, alpha_linear, views_linears.0, rgb_linear
    (use_viewdirs) or output_linear (use_viewdirs=False: raw has ``output_ch`` channels).  ``skip``: the reference's
    ``skips`` list (or one index / -1): layer i + 1 sees cat[x, h] for every i in it.  ``unit_ordered``: the caller sorted the
    hidden units by firing rate (NeRF.packed); marks the handle for the dispatch (ns_weights_set_unit_ordered)."""
    lib = _lib.load()
    skips = [skip] if isinstance(skip, int) else list(skip)
    skips = [int(i) for i in skips if int(i) >= 0]
    if any(i >= 32 for i in skips):
        raise NotImplementedError("skip indices beyond 31 are not supported")
    mask = 0
    for i in skips:
        mask |= 1 << i
    wa, k1 = _host_ptr_array(weights)
    ba, k2 = _host_ptr_array(biases)
    out = C.c_void_p()
    name = dtype or _compute_dtype
    with torch.cuda.device(device):
        check(lib.ns_pack_nerf_ex(D, W, mask, int(bool(use_viewdirs)), int(output_ch), wa, ba, dtype_code(name),
                                  C.byref(out)), "ns_pack_nerf_ex")
    pw = PackedWeights(out.value, "nerf", name, torch.device(device))
    pw.out_ch = int(lib.ns_nerf_out_channels(pw.handle))
    pw.use_viewdirs = bool(use_viewdirs)
    if unit_ordered:
        check(lib.ns_weights_set_unit_ordered(pw.handle, 1), "ns_weights_set_unit_ordered")
    return pw


def pack_depthnet(weights: Sequence[Tensor], biases: Sequence[Tensor], hidden_sizes: Sequence[int],
                  cat_hidden_sizes: Sequence[int], dtype: Optional[str] = None, device="cuda") -> PackedWeights:
    """order: origin_layers.*, direction_layers.*, intersection_layers.*, cat_layers.{0,2,..}, to_depth.0

    ``hidden_sizes``: the widths of the three skip branches (any); ``cat_hidden_sizes``: the trunk widths (each <= 256).
    The affine branches are folded into the first trunk layer by the packer (ns_pack_depthnet_ex)."""
    lib = _lib.load()
    hs = (C.c_int * len(hidden_sizes))(*[int(v) for v in hidden_sizes])
    cs = (C.c_int * len(cat_hidden_sizes))(*[int(v) for v in cat_hidden_sizes])
    if len(weights) != 3 * len(hidden_sizes) + len(cat_hidden_sizes) + 1 or len(biases) != len(weights):
        raise ValueError("pack_depthnet: expected 3 * len(hidden_sizes) + len(cat_hidden_sizes) + 1 weight tensors")
    wa, k1 = _host_ptr_array(weights)
    ba, k2 = _host_ptr_array(biases)
    out = C.c_void_p()
    name = dtype or _compute_dtype
    with torch.cuda.device(device):
        check(lib.ns_pack_depthnet_ex(len(hidden_sizes), hs, len(cat_hidden_sizes), cs, wa, ba, dtype_code(name),
                                      C.byref(out)), "ns_pack_depthnet_ex")
    return PackedWeights(out.value, "depthnet", name, torch.device(device))


# ---- a4 -------------------------------------------------------------------------------------------
def depthnet_forward(net: PackedWeights, o: Tensor, d: Tensor, near: float = 2.0, far: float = 6.0,
                     sphere_radius: float = 2.0) -> Tensor:
    lib = _lib.load()
    o, d = _dev(o, "rays_o"), _dev(d, "rays_d")
    R = o.shape[0]
    z = torch.empty((R, 1), dtype=torch.float32, device=o.device)
    check(lib.ns_depthnet_forward(net.handle, _ptr(o), _ptr(d), R, float(near), float(far), float(sphere_radius),
                                  _ptr(z), _stream(o.device)), "ns_depthnet_forward")
    return z


# ---- a5 -------------------------------------------------------------------------------------------
def place_samples(o: Tensor, d: Tensor, mean: Tensor, n_samples: int, mode: str, std: float,
                  noise: Optional[Tensor] = None, want_pts: bool = True):
    lib = _lib.load()
    if mode not in _MODES:
        raise ValueError(f"unknown sampling mode {mode!r}")
    o, d, mean = _dev(o, "rays_o"), _dev(d, "rays_d"), _dev(mean, "mean")
    R = o.shape[0]
    N = 1 if mode == "depth_only" else int(n_samples)
    if mode == "gaussian" and noise is None:
        # same draw shape / order as the reference's torch.randn(mean.shape[0], n_samples - 1)
        noise = torch.randn(R, N - 1, device=o.device)
    if noise is not None:
        noise = _dev(noise, "noise")
    z = torch.empty((R, N), dtype=torch.float32, device=o.device)
    pts = torch.empty((R, N, 3), dtype=torch.float32, device=o.device) if want_pts else None
    check(lib.ns_place_samples(_MODES[mode], _ptr(o), _ptr(d), _ptr(mean), _ptr(noise), R, N, float(std),
                               _ptr(pts), _ptr(z), _stream(o.device)), "ns_place_samples")
    return pts, z


def points_along_rays(o: Tensor, d: Tensor, z: Tensor) -> Tensor:
    lib = _lib.load()
    o, d, z = _dev(o, "rays_o"), _dev(d, "rays_d"), _dev(z, "z")
    R, N = z.shape
    pts = torch.empty((R, N, 3), dtype=torch.float32, device=o.device)
    check(lib.ns_points_along_rays(_ptr(o), _ptr(d), _ptr(z), R, N, _ptr(pts), _stream(o.device)),
          "ns_points_along_rays")
    return pts


# ---- a6 / a7 ----------------------------------------------------------------------------------------
def nerf_forward(net: PackedWeights, pts: Tensor, viewdirs: Optional[Tensor]) -> Tensor:
    """pts [R,N,3], viewdirs [R,3] (None for a network without view directions) -> raw [R,N,C], C = net.out_ch"""
    lib = _lib.load()
    pts = _dev(pts, "pts")
    if getattr(net, "use_viewdirs", True):
        viewdirs = _dev(viewdirs, "viewdirs")
    else:
        viewdirs = None
    R, N = pts.shape[0], pts.shape[1]
    raw = torch.empty((R, N, getattr(net, "out_ch", 4)), dtype=torch.float32, device=pts.device)
    check(lib.ns_nerf_forward(net.handle, _ptr(pts), None, None, None, _ptr(viewdirs), R, N, _ptr(raw),
                              _stream(pts.device)), "ns_nerf_forward")
    return raw


def nerf_forward_rays(net: PackedWeights, o: Tensor, d: Tensor, z: Tensor, viewdirs: Optional[Tensor]) -> Tensor:
    """points formed in-kernel as o + d*z; z [R,N] -> raw [R,N,C]"""
    lib = _lib.load()
    o, d, z = _dev(o, "rays_o"), _dev(d, "rays_d"), _dev(z, "z")
    viewdirs = _dev(viewdirs, "viewdirs") if getattr(net, "use_viewdirs", True) else None
    R, N = z.shape
    raw = torch.empty((R, N, getattr(net, "out_ch", 4)), dtype=torch.float32, device=z.device)
    check(lib.ns_nerf_forward(net.handle, None, _ptr(o), _ptr(d), _ptr(z), _ptr(viewdirs), R, N, _ptr(raw),
                              _stream(z.device)), "ns_nerf_forward")
    return raw


def nerf_forward_embedded(net: PackedWeights, x: Tensor) -> Tensor:
    lib = _lib.load()
    x = _dev(x, "x")
    width = 90 if getattr(net, "use_viewdirs", True) else 63
    if x.shape[-1] != width:
        raise NotImplementedError(f"embedded input must be {width} wide (63 point + 27 direction features), got {x.shape[-1]}")
    M = x.numel() // width
    raw = torch.empty(tuple(x.shape[:-1]) + (getattr(net, "out_ch", 4),), dtype=torch.float32, device=x.device)
    check(lib.ns_nerf_forward_embedded(net.handle, _ptr(x), M, _ptr(raw), _stream(x.device)),
          "ns_nerf_forward_embedded")
    return raw


# ---- a8 -------------------------------------------------------------------------------------------
def raw2outputs(raw: Tensor, z: Tensor, rays_d: Tensor, noise: Optional[Tensor] = None,
                white_bkgd: bool = True, want_per_sample: bool = True):
    """-> rgb [R,3], disp [R], acc [R], depth [R], alphas [R,N] | None, weights [R,N] | None"""
    lib = _lib.load()
    if raw.shape[-1] > 4:        # output_ch = 5 networks (no view directions, N_importance > 0): channel 4 is never read
        raw = raw[..., :4]
    raw, z, rays_d = _dev(raw, "raw"), _dev(z, "z_vals"), _dev(rays_d, "rays_d")
    R, N = z.shape
    dev = raw.device
    rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
    disp = torch.empty((R,), dtype=torch.float32, device=dev)
    acc = torch.empty_like(disp)
    depth = torch.empty_like(disp)
    # one sample: the reference's alphas / weights are [R, 0] (see ns_raw2outputs in the header)
    n_out = 0 if N == 1 else N
    alphas = torch.empty((R, n_out), dtype=torch.float32, device=dev) if want_per_sample else None
    weights = torch.empty((R, n_out), dtype=torch.float32, device=dev) if want_per_sample else None
    if noise is not None:
        noise = _dev(noise, "noise")
    check(lib.ns_raw2outputs(_ptr(raw), _ptr(z), _ptr(rays_d), _ptr(noise), R, N, int(bool(white_bkgd)),
                             _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(depth), _ptr(alphas), _ptr(weights),
                             _stream(dev)), "ns_raw2outputs")
    return rgb, disp, acc, depth, alphas, weights


def raw2outputs_backward(raw: Tensor, z: Tensor, rays_d: Tensor, noise: Optional[Tensor], white_bkgd: bool,
                         grads: Sequence[Optional[Tensor]], want: Sequence[bool] = (True, True, True)):
    """Backward of raw2outputs from its inputs (ns_raw2outputs_backward re-runs the forward).  grads: the upstream gradients of
    (rgb, disp, acc, depth, alphas, weights), None where an output takes no part.  want: which of (d_raw, d_z, d_rays_d) to
    compute.  -> (d_raw [R,N,C] | None, d_z [R,N] | None, d_rays_d [R,3] | None); channels past the fourth get zeros."""
    lib = _lib.load()
    C_ = raw.shape[-1]
    raw4 = raw[..., :4] if C_ > 4 else raw
    raw4, z, rays_d = _dev(raw4, "raw"), _dev(z, "z_vals"), _dev(rays_d, "rays_d")
    R, N = z.shape
    dev = raw4.device
    g = [None if t is None or t.numel() == 0 else _dev(t, "grad") for t in grads]
    if noise is not None:
        noise = _dev(noise, "noise")
    d_raw = torch.empty((R, N, 4), dtype=torch.float32, device=dev) if want[0] else None
    d_z = torch.empty((R, N), dtype=torch.float32, device=dev) if want[1] else None
    d_d = torch.empty((R, 3), dtype=torch.float32, device=dev) if want[2] else None
    check(lib.ns_raw2outputs_backward(_ptr(raw4), _ptr(z), _ptr(rays_d), _ptr(noise), R, N, int(bool(white_bkgd)),
                                      *[_ptr(t) for t in g], _ptr(d_raw), _ptr(d_z), _ptr(d_d), _stream(dev)),
          "ns_raw2outputs_backward")
    if d_raw is not None and C_ > 4:
        d_raw = torch.cat([d_raw, torch.zeros((R, N, C_ - 4), dtype=torch.float32, device=dev)], -1)
    return d_raw, d_z, d_d


def place_samples_backward(mean: Tensor, d_z: Tensor, mode: str, std: float) -> Tensor:
    """d mean [R] of place_samples from d z [R,N] (ns_place_samples_backward)"""
    lib = _lib.load()
    mean, d_z = _dev(mean.reshape(-1), "mean"), _dev(d_z, "d_z")
    R, N = d_z.shape
    d_mean = torch.empty((R,), dtype=torch.float32, device=mean.device)
    check(lib.ns_place_samples_backward(_MODES[mode], _ptr(mean), R, N, float(std), _ptr(d_z), _ptr(d_mean),
                                        _stream(mean.device)), "ns_place_samples_backward")
    return d_mean


# ---- a11 ------------------------------------------------------------------------------------------
def coarse_z(near: Tensor, far: Tensor, n_samples: int, lindisp: bool, t_rand: Optional[Tensor] = None) -> Tensor:
    lib = _lib.load()
    near, far = _dev(near.reshape(-1), "near"), _dev(far.reshape(-1), "far")
    R = near.shape[0]
    if t_rand is not None:
        t_rand = _dev(t_rand, "t_rand")
    z = torch.empty((R, n_samples), dtype=torch.float32, device=near.device)
    check(lib.ns_coarse_z(_ptr(near), _ptr(far), R, n_samples, int(bool(lindisp)), _ptr(t_rand), _ptr(z),
                          _stream(near.device)), "ns_coarse_z")
    return z


def sample_pdf(bins: Tensor, weights: Tensor, n_samples: int, u: Optional[Tensor] = None) -> Tensor:
    lib = _lib.load()
    bins, weights = _dev(bins, "bins"), _dev(weights, "weights")
    R, Nb = bins.shape
    if weights.shape[-1] != Nb - 1:
        raise ValueError("weights must have one element fewer than bins")
    if u is not None:
        u = _dev(u, "u")
    out = torch.empty((R, n_samples), dtype=torch.float32, device=bins.device)
    check(lib.ns_sample_pdf(_ptr(bins), _ptr(weights), R, Nb, n_samples, _ptr(u), _ptr(out), _stream(bins.device)),
          "ns_sample_pdf")
    return out


def importance_z(z: Tensor, weights: Tensor, n_importance: int, u: Optional[Tensor] = None) -> Tensor:
    lib = _lib.load()
    z, weights = _dev(z, "z_vals"), _dev(weights, "weights")
    R, Nc = z.shape
    if u is not None:
        u = _dev(u, "u")
    out = torch.empty((R, Nc + n_importance), dtype=torch.float32, device=z.device)
    check(lib.ns_importance_z(_ptr(z), _ptr(weights), R, Nc, n_importance, _ptr(u), _ptr(out), _stream(z.device)),
          "ns_importance_z")
    return out


def sort_rows(x: Tensor) -> Tensor:
    lib = _lib.load()
    x = _dev(x, "x")
    R, N = x.shape
    out = torch.empty_like(x)
    check(lib.ns_sort_rows(_ptr(x), R, N, _ptr(out), _stream(x.device)), "ns_sort_rows")
    return out


def argmax_gather(weights: Tensor, z: Tensor, raw: Optional[Tensor] = None):
    lib = _lib.load()
    weights, z = _dev(weights, "weights"), _dev(z, "z_vals")
    R, N = weights.shape
    dev = weights.device
    max_z = torch.empty((R, 1), dtype=torch.float32, device=dev)
    max_w = torch.empty((R, 1), dtype=torch.float32, device=dev)
    max_rgb = None
    if raw is not None:
        raw = _dev(raw, "raw")
        max_rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
    check(lib.ns_argmax_gather(_ptr(weights), _ptr(z), _ptr(raw), R, N, _ptr(max_z), _ptr(max_w), _ptr(max_rgb),
                               _stream(dev)), "ns_argmax_gather")
    return max_z, max_w, max_rgb


# ---- a9 fused -------------------------------------------------------------------------------------
class RenderWorkspace:
    """Reusable device workspace for render_rays_depthnet (grown on demand, never shrunk)."""

    def __init__(self):
        self.buf: Optional[Tensor] = None

    def get(self, nbytes: int, device) -> Tensor:
        # + 256: callers align the base pointer up to 256 bytes
        if self.buf is None or self.buf.numel() < nbytes + 256 or self.buf.device != torch.device(device):
            self.buf = torch.empty((nbytes + 256,), dtype=torch.uint8, device=device)
        return self.buf


_default_ws = RenderWorkspace()


def _set_workspace(a, workspace: Optional[RenderWorkspace], nbytes: int, device) -> None:
    """a.workspace_dev = the 256-byte-aligned base of ``nbytes`` bytes of ``workspace`` (None: the module's own)."""
    a.workspace_dev = ((workspace or _default_ws).get(nbytes, device).data_ptr() + 255) & ~255


def _set_ray_source(a, rays, camera, device):
    """The ray-source fields of a RenderArgs / HierArgs from rays = (o, d, viewdirs) device tensors or camera = (H, W, K,
    c2w, row0, row1) -> (R, device, tensors to keep alive until the call)."""
    if rays is not None:
        o, d, v = (_dev(t, n) for t, n in zip(rays, ("rays_o", "rays_d", "viewdirs")))
        a.o_dev, a.d_dev, a.viewdirs_dev, a.R = o.data_ptr(), d.data_ptr(), v.data_ptr(), o.shape[0]
        return o.shape[0], o.device, [o, d, v]
    H, W, K, c2w, row0, row1 = camera
    a.H, a.W, a.row0, a.row1 = H, W, row0, row1
    a.fx, a.fy, a.cx, a.cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    a.c2w[:] = _c2w_host(c2w).reshape(-1).tolist()
    a.R = (row1 - row0) * W
    return a.R, torch.device(device), []


def _rgb_disp_outputs(a, R: int, device, shard: Optional[Tensor]):
    """Per-ray outputs of the one-call renderers: fresh packed tensors, or views of an interleaved [.., 4] shard."""
    if shard is None:
        out = {"rgb": torch.empty((R, 3), dtype=torch.float32, device=device),
               "disp": torch.empty((R,), dtype=torch.float32, device=device)}
        a.rgb_dev, a.disp_dev = out["rgb"].data_ptr(), out["disp"].data_ptr()
        return out
    if not (shard.is_cuda and shard.dtype == torch.float32 and shard.dim() == 2 and shard.shape[1] == 4
            and shard.is_contiguous() and shard.shape[0] >= R):
        raise ValueError(f"shard must be a contiguous fp32 device tensor [>= {R}, 4], got {tuple(shard.shape)} {shard.dtype}")
    a.rgb_dev, a.disp_dev = shard.data_ptr(), shard.data_ptr() + 12
    a.rgb_stride = a.disp_stride = 4
    return {"rgb": shard[:R, :3], "disp": shard[:R, 3]}


def _extras_names(extras, per_sample: Tuple[str, ...], more: Tuple[str, ...] = ()) -> Tuple[str, ...]:
    """``extras`` of a one-call renderer -> the names asked for: True = its per-sample arrays, False / None = none, or a tuple
    drawn from those, the per-ray maps "depth" / "acc" and what else the renderer offers (``more``)."""
    if isinstance(extras, (bool, int, np.bool_)):
        return per_sample if extras else ()
    names = tuple(extras or ())
    allowed = per_sample + ("depth", "acc") + more
    if not set(names) <= set(allowed):
        raise ValueError(f"extras: True, False or a tuple of {', '.join(repr(n) for n in allowed)}, got {extras!r}")
    return names


def _per_ray_maps(a, names, R: int, device, out: dict) -> None:
    """The expected-depth and opacity maps [R] asked for in ``names`` (RenderArgs / HierArgs depth_dev / acc_dev)."""
    for name in ("depth", "acc"):
        if name in names:
            out[name] = torch.empty((R,), dtype=torch.float32, device=device)
            setattr(a, name + "_dev", out[name].data_ptr())


def render_rays_depthnet(depthnet: PackedWeights, nerf: PackedWeights, *, rays=None, camera=None,
                         n_samples: int, mode: str, std: float, noise: Optional[Tensor] = None,
                         near: float = 2.0, far: float = 6.0, sphere_radius: float = 2.0,
                         white_bkgd: bool = True, extras=False, workspace: Optional[RenderWorkspace] = None,
                         device="cuda", mlp_events=None, shard: Optional[Tensor] = None,
                         one_kernel: Optional[bool] = None, guard: Optional[PackedWeights] = None,
                         guard_threshold: Optional[float] = None, guard_long_rays: str = "every"):
    """DepthNet -> placement -> NeRF MLP -> compositing as one C call.

    rays = (o, d, viewdirs) device tensors, or camera = (H, W, K, c2w, row0, row1) to generate
    the rays on the device.  Returns dict(rgb [R,3], disp [R], and with extras z/weights/pts).
    ``extras``: True = z [R,N], weights [R,N] and pts [R,N,3]; or a tuple naming the ones wanted from "z", "weights", "pts",
    "depth", "acc" -- depth / acc [R] are the expected-depth and opacity maps (acc before the white background), bit for bit
    what raw2outputs returns for the call's own raw and z; per-ray, so they cost no per-sample traffic.
    ``shard``: a contiguous fp32 [>= R, 4] device tensor; the compositing kernel then writes (r, g, b, disp) of ray i
    straight into shard[i] (the unit parallel.FrameRenderer all-gathers) and rgb / disp are returned as views of it.
    ``one_kernel``: None (default) = ns_render_rays_fused -- placement, MLP and compositing in ONE persistent kernel, per-sample
    data never in HBM -- whenever the configuration supports it (uniform placement, bf16 / f16 / f16x3 field, n_samples a power of
    two <= 64 or a multiple of 64 up to 512), else the five-launch chain ns_render_rays_depthnet; True = require it; False = the chain.  Both produce the
    same bits.  Known cost: at N >= 128 (a ray of several 64-sample chunks) the one-kernel frame runs about 1 % behind the chain
    (f16x3, 1600 x 1600 x 192: 1098 vs 1087 ms) while needing a workspace that does not grow with N.
    ``guard``: the SAME radiance field packed "f16x3" (fp32-grade).  The last sample of every ray -- the one the reference
    composites with dist = 1e10, so that alpha = step(sigma) -- is then evaluated a second time through it and its sigma
    replaces the 16-bit one (R of the R * N samples; uniform placement only).  Pair it with an "f16x3" DepthNet handle:
    the two together are the PSNR guard of the 16-bit paths (see psnr_guard_handles).
    ``guard_threshold`` (one-kernel renderer; n_samples <= 64, or 128 .. 512 under guard_long_rays="selective"): None = the
    module setting (set_psnr_guard, 16.0); > 0 = only the rays whose own sigma of the last sample lies within it of zero are
    re-evaluated, after the kernel, on a compacted list (the same bits as the every-ray guard wherever |sigma16 - sigma32|
    stays below it); 0 = every ray, before the kernel.
    ``guard_long_rays``: "every" (default) or "selective" -- the guard's form for rays of several 64-sample chunks (n_samples a
    multiple of 64 in [128, 512]) in the one-kernel renderer on a 16-bit field with an "f16x3" guard and a threshold > 0.
    "every": every ray before the kernel, whatever the threshold.  "selective": the kernel flags the rays within the threshold
    as it does for n_samples <= 64, and an unflagged ray whose step flips on its 16-bit sigma keeps the 16-bit one.  Ignored
    where it does not apply (n_samples <= 64, an f16x3 field, threshold 0, another guard packing, the chain).
    extras "guard_count": a 1-element int32 device tensor, initialised to -1; a call that ran the selective form (either ray
    length) writes the number of flagged rays there, on the stream, without a host synchronisation.
    """
    names = _extras_names(extras, ("z", "weights", "pts"), ("guard_count",))
    _check_guard_long_rays(guard_long_rays)
    lib = _lib.load()
    a = _lib.RenderArgs()
    a.depthnet, a.nerf = depthnet.handle, nerf.handle
    if rays is not None and rays[0].shape[0] == 0:     # empty batch: nothing to launch
        dev0, n0 = rays[0].device, (1 if mode == "depth_only" else int(n_samples))
        out = {"rgb": torch.empty((0, 3), device=dev0), "disp": torch.empty((0,), device=dev0)}
        empty = dict(z=torch.empty((0, n0), device=dev0), weights=torch.empty((0, 0 if n0 == 1 else n0), device=dev0),
                     pts=torch.empty((0, n0, 3), device=dev0), depth=torch.empty((0,), device=dev0),
                     acc=torch.empty((0,), device=dev0), guard_count=torch.full((1,), -1, dtype=torch.int32, device=dev0))
        out.update((k, empty[k]) for k in names)
        return out
    R, device, keep = _set_ray_source(a, rays, camera, device)
    N = 1 if mode == "depth_only" else int(n_samples)
    a.mode, a.N, a.std_ = _MODES[mode], N, float(std)
    if mode == "gaussian":
        if noise is None:
            noise = torch.randn(R, N - 1, device=device)
        noise = _dev(noise, "noise")
        keep.append(noise)
        a.noise_dev = noise.data_ptr()
    a.near_, a.far_, a.sphere_radius, a.white_bkgd = float(near), float(far), float(sphere_radius), int(bool(white_bkgd))
    fused_ok = bool(lib.ns_render_fused_supported(nerf.handle, a.mode, N)) and noise is None
    if one_kernel and not fused_ok:
        raise NotImplementedError(f"the one-kernel renderer needs uniform placement, a bf16 / f16 / f16x3 field with view directions and "
                                  f"n_samples a power of two in [2, 64] or a multiple of 64 up to 512 (mode {mode!r}, n_samples {N}, dtype {getattr(nerf, 'dtype', '?')})")
    use_fused = fused_ok if one_kernel is None else bool(one_kernel)
    if use_fused and guard is not None and guard_long_rays == "selective" and N > 64:   # 192-byte records (ns_render_args)
        nbytes = int(lib.ns_render_fused_guard_long_workspace_bytes(R))
    else:
        nbytes = int(lib.ns_render_fused_workspace_bytes(R) if use_fused else lib.ns_render_workspace_bytes(R, N))
    _set_workspace(a, workspace, nbytes, device)
    out = _rgb_disp_outputs(a, R, device, shard)
    # one sample: the reference's weights are [R, 0] (its dists are empty) and ns_raw2outputs writes none
    for name, shape in (("z", (R, N)), ("weights", (R, 0 if N == 1 else N)), ("pts", (R, N, 3))):
        if name in names:
            out[name] = torch.empty(shape, dtype=torch.float32, device=device)
            if out[name].numel():
                setattr(a, name + "_dev", out[name].data_ptr())
    _per_ray_maps(a, names, R, device, out)
    if mlp_events is not None:
        a.ev_mlp_begin, a.ev_mlp_end = mlp_events[0].handle, mlp_events[1].handle
    if guard is not None:
        a.nerf_guard = guard.handle
        a.guard_threshold = float(_guard_threshold if guard_threshold is None else guard_threshold)
        a.guard_long_selective = int(guard_long_rays == "selective")
    if "guard_count" in names:
        out["guard_count"] = torch.full((1,), -1, dtype=torch.int32, device=device)
        a.guard_count_dev = out["guard_count"].data_ptr()
    if use_fused:
        check(lib.ns_render_rays_fused(C.byref(a), _stream(device)), "ns_render_rays_fused")
    else:
        check(lib.ns_render_rays_depthnet(C.byref(a), _stream(device)), "ns_render_rays_depthnet")
    return out


def _tangent_samples_ok(n: int) -> bool:
    return (2 <= n <= 64 and n & (n - 1) == 0) or (64 < n <= 512 and n % 64 == 0)


def render_rays_depthnet_tangent(depthnet_or_mean, nerf: PackedWeights, *, rays=None, camera=None, n_samples: int,
                                 std: float, extras=(), near: float = 2.0, far: float = 6.0, sphere_radius: float = 2.0,
                                 white_bkgd: bool = True, workspace: Optional[RenderWorkspace] = None, device="cuda",
                                 mlp_events=None, approximate: bool = False, mode: str = "uniform"):
    """The one-kernel renderer with forward-mode tangents in every ray's DepthNet depth (ns_render_rays_fused_tangent).

    ``depthnet_or_mean``: a packed DepthNet (its depth is computed as render_rays_depthnet does) or a device tensor [R] of
    depths.  ``nerf``: an "f16x3" NeRF handle.  Uniform placement, n_samples a power of two in [2, 64] or a multiple of 64
    up to 512.  Returns (out, J): out = dict(rgb [R,3], disp [R], and "depth" / "acc" [R] if named in ``extras``), bit for bit
    those of render_rays_depthnet(one_kernel=True) on the same handle and depth; J = dict(rgb [R,3], disp, depth, acc [R]), the
    derivatives of those maps w.r.t. the depth of their ray -- what torch autograd of place_samples -> the field ->
    raw2outputs gives, per ray.

    ``approximate=True`` (keyword only) also accepts an "f16" NeRF handle, one of the renderer's production fields.  J is then
    the derivative carried through that field's 16-bit arithmetic: the field's weights and activations are fp16, and so is the
    tangent of every layer, so J is the Jacobian of the f16 field, not the fp32-grade Jacobian of the chain.  Against autograd
    of a model of the same f16 field the error of J is ~1e-3 of its column's RMS at the median or below; against the f16x3 kernel
    it is 10 .. 100 x larger, because the f16 field's rounding moves ReLU and opacity kinks.  The DepthNet gradients of
    autograd.render_depthnet_differentiable keep a cosine of at least 0.9989 with the same f16 field's and of 0.979 .. 0.99996
    with the f16x3 path's, as the f16 field itself does (tests/test_gpu_render_tangent16.py).  The outputs
    are those of the f16 one-kernel forward bit for bit.  bf16 and f32 handles are refused either way.

    ``mode="depth_only"`` (keyword only; default "uniform"): one sample per ray at the depth itself, unclipped -- the DepthNet
    branch of the training operator (render_rays).  ``n_samples`` and ``std`` are ignored.  out is raw2outputs' single-sample
    rule, bit for bit render_rays_depthnet(mode="depth_only") on the same handles: rgb = sigmoid(raw rgb) whatever the
    background, disp = 1e10, depth = acc = 0; J["rgb"] = rgb (1 - rgb) d raw rgb / d depth, J["disp"] = J["depth"] =
    J["acc"] = 0.  A NaN depth gives a NaN rgb and a NaN J["rgb"] for its ray, as torch autograd of the chain does.  An "f16x3"
    handle only: ``approximate=True`` with an "f16" handle raises NotImplementedError."""
    names = _extras_names(extras, ())
    if mode not in ("uniform", "depth_only"):
        raise ValueError(f"mode: 'uniform' or 'depth_only', got {mode!r}")
    single = mode == "depth_only"
    ok_dtypes = ("f16x3", "f16") if approximate and not single else ("f16x3",)
    if not isinstance(nerf, PackedWeights) or nerf.dtype not in ok_dtypes:
        got = getattr(nerf, "dtype", type(nerf).__name__)
        if single:
            raise NotImplementedError(f"depth_only tangents need an f16x3 NeRF handle, got {got}")
        if approximate:
            raise NotImplementedError(f"tangents need an f16x3 or f16 NeRF handle, got {got}")
        raise NotImplementedError(f"tangents need an f16x3 NeRF handle, got {got}")
    N = 1 if single else int(n_samples)
    if not single and not _tangent_samples_ok(N):
        raise NotImplementedError(f"n_samples must be a power of two in [2, 64] or a multiple of 64 up to 512, got {N}")
    if (rays is None) == (camera is None):
        raise ValueError("exactly one of rays= and camera= is required")
    if isinstance(depthnet_or_mean, PackedWeights):
        if depthnet_or_mean.kind != "depthnet":
            raise TypeError("depthnet_or_mean: a packed DepthNet or a depth tensor [R]")
        mean = None
    elif isinstance(depthnet_or_mean, Tensor):
        mean = _dev(depthnet_or_mean.detach().reshape(-1), "mean")
        R_ = rays[0].shape[0] if rays is not None else (camera[5] - camera[4]) * camera[1]
        if mean.shape[0] != R_:
            raise ValueError(f"mean has {mean.shape[0]} depths for {R_} rays")
    else:
        raise TypeError("depthnet_or_mean: a packed DepthNet or a depth tensor [R]")
    lib = _lib.load()
    a = _lib.RenderArgs()
    t = _lib.TangentArgs()
    a.nerf = nerf.handle
    if mean is None:
        a.depthnet = depthnet_or_mean.handle
    R, device, _keep = _set_ray_source(a, rays, camera, device)
    if mean is not None:
        t.mean_dev = mean.data_ptr()
    a.mode, a.N, a.std_ = _MODES[mode], N, float(std)
    a.near_, a.far_, a.sphere_radius, a.white_bkgd = float(near), float(far), float(sphere_radius), int(bool(white_bkgd))
    out = {"rgb": torch.empty((R, 3), dtype=torch.float32, device=device), "disp": torch.empty((R,), dtype=torch.float32, device=device)}
    J = {"rgb": torch.empty((R, 3), dtype=torch.float32, device=device)}
    J.update((k, torch.empty((R,), dtype=torch.float32, device=device)) for k in ("disp", "depth", "acc"))
    _per_ray_maps(a, names, R, device, out)
    if R == 0:
        return out, J
    a.rgb_dev, a.disp_dev = out["rgb"].data_ptr(), out["disp"].data_ptr()
    t.d_rgb_dev, t.d_disp_dev, t.d_depth_dev, t.d_acc_dev = (J[k].data_ptr() for k in ("rgb", "disp", "depth", "acc"))
    _set_workspace(a, workspace, int(lib.ns_render_tangent_workspace_bytes(R)), device)
    if mlp_events is not None:
        a.ev_mlp_begin, a.ev_mlp_end = mlp_events[0].handle, mlp_events[1].handle
    check(lib.ns_render_rays_fused_tangent(C.byref(a), C.byref(t), _stream(device)), "ns_render_rays_fused_tangent")
    return out, J


def render_rays_hierarchical(coarse: PackedWeights, fine: Optional[PackedWeights], *, rays=None, camera=None,
                             n_coarse: int = 64, n_importance: int = 128, lindisp: bool = True,
                             white_bkgd: bool = True, near: float = 2.0, far: float = 6.0,
                             t_rand: Optional[Tensor] = None, u: Optional[Tensor] = None, extras=False,
                             workspace: Optional[RenderWorkspace] = None, device="cuda", mlp_events=None,
                             shard: Optional[Tensor] = None, coarse_events=None, max_sample: bool = False):
    """Vanilla coarse + fine pass (sample_as_in_NeRF) as one C call; returns the FINE pass outputs.
    ``extras``: True = z / weights [R,Nc+Nf] and raw [R,Nc+Nf,4] too; or a tuple naming the ones wanted, e.g. ("z", "weights"),
    from those and "depth" / "acc": the fine pass's (the coarse pass's when n_importance == 0) expected-depth and opacity maps
    [R], bit for bit what raw2outputs returns for that pass's z and raw.
    ``max_sample``: also the max-weight fine sample of every ray (nerf_utils.py:813-819), max_z / max_weights [R,1] and
    max_rgb [R,3], bit-identical to argmax_gather(weights, z, raw) of the same call; needs n_importance > 0.
    ``shard``: as in render_rays_depthnet.  ``mlp_events`` / ``coarse_events``: (begin, end) ops.Event pairs recorded around
    the fine-pass / coarse-pass MLP kernel."""
    if max_sample and int(n_importance) <= 0:
        raise ValueError("max_sample: the max-weight sample is one of the fine pass, n_importance must be > 0")
    names = _extras_names(extras, ("z", "weights", "raw"))
    lib = _lib.load()
    a = _lib.HierArgs()
    a.coarse = coarse.handle
    a.fine = fine.handle if fine is not None else None
    R, device, keep = _set_ray_source(a, rays, camera, device)
    a.Nc, a.Nf, a.lindisp, a.white_bkgd = int(n_coarse), int(n_importance), int(bool(lindisp)), int(bool(white_bkgd))
    a.near_, a.far_ = float(near), float(far)
    for name, t in (("t_rand_dev", t_rand), ("u_dev", u)):
        if t is not None:
            t = _dev(t, name)
            keep.append(t)
            setattr(a, name, t.data_ptr())
    size_fn = lib.ns_hier_max_workspace_bytes if max_sample else lib.ns_hier_workspace_bytes
    _set_workspace(a, workspace, int(size_fn(R, a.Nc, a.Nf)), device)
    Nt = a.Nc + a.Nf
    out = _rgb_disp_outputs(a, R, device, shard)
    for name, shape in (("z", (R, Nt)), ("weights", (R, Nt)), ("raw", (R, Nt, 4))):
        if name in names:
            out[name] = torch.empty(shape, dtype=torch.float32, device=device)
            setattr(a, name + "_dev", out[name].data_ptr())
    _per_ray_maps(a, names, R, device, out)
    if max_sample:
        for name, field, shape in (("max_z", "max_z_dev", (R, 1)), ("max_weights", "max_w_dev", (R, 1)),
                                   ("max_rgb", "max_rgb_dev", (R, 3))):
            out[name] = torch.empty(shape, dtype=torch.float32, device=device)
            setattr(a, field, out[name].data_ptr())
    if mlp_events is not None:
        a.ev_mlp_begin, a.ev_mlp_end = mlp_events[0].handle, mlp_events[1].handle
    if coarse_events is not None:
        a.ev_coarse_begin, a.ev_coarse_end = coarse_events[0].handle, coarse_events[1].handle
    check(lib.ns_render_rays_hierarchical(C.byref(a), _stream(device)), "ns_render_rays_hierarchical")
    return out


class debug_switch:
    """Context manager around ns_debug_set: ``with ops.debug_switch(generic_kernels=1, prod_tiles=4): ...`` (tests compare the
    kernel variants inside one process); every switch is reset to 0 (= the dispatcher's own choice) on exit, ``kblock_suffix`` to its initial value."""

    RESET = {"kblock_suffix": -1}

    def __init__(self, **switches):
        self.switches = switches

    def __enter__(self):
        for k, v in self.switches.items():
            check(_lib.load().ns_debug_set(k.encode(), int(v)), "ns_debug_set")
        return self

    def __exit__(self, *exc):
        for k in self.switches:
            check(_lib.load().ns_debug_set(k.encode(), self.RESET.get(k, 0)), "ns_debug_set")
        return False


def colour_skip_count() -> int:
    """Waves that skipped the colour layers in the last 16-bit radiance-field launch made under
    ``debug_switch(count_colour_skips=1)`` (0 when that launch did not run the render kernel); waits for the device."""
    n = C.c_int64(0)
    check(_lib.load().ns_colour_skip_count(C.byref(n)), "ns_colour_skip_count")
    return int(n.value)


def kblock_skip_count() -> int:
    """Chunk steps whose MFMAs the K-block-skipping render kernel jumped over (their input K-block was all zero bits for the
    wave), summed over the waves of the last 16-bit radiance-field launch made under ``debug_switch(count_colour_skips=1)``
    (0 when that launch ran another kernel); waits for the device."""
    n = C.c_int64(0)
    check(_lib.load().ns_kblock_skip_count(C.byref(n)), "ns_kblock_skip_count")
    return int(n.value)


def kblock_suffix_count() -> int:
    """Chunk steps absent from the bodies the dead-suffix render kernel's waves ran (sub-blocks x trailing dead K-blocks of each
    statement's input), summed over the waves of the last 16-bit radiance-field launch made under
    ``debug_switch(count_colour_skips=1)`` (0 when that launch ran another kernel); waits for the device."""
    n = C.c_int64(0)
    check(_lib.load().ns_kblock_suffix_count(C.byref(n)), "ns_kblock_suffix_count")
    return int(n.value)


class Event:
    """hipEvent wrapper for timing a kernel on the stream it is launched on."""

    def __init__(self):
        self.handle = C.c_void_p()
        check(_lib.load().ns_event_create(C.byref(self.handle)), "ns_event_create")

    def record(self, device="cuda"):
        check(_lib.load().ns_event_record(self.handle, _stream(torch.device(device))), "ns_event_record")

    def elapsed_ms(self, end: "Event") -> float:
        ms = C.c_float()
        check(_lib.load().ns_event_elapsed_ms(self.handle, end.handle, C.byref(ms)), "ns_event_elapsed_ms")
        return float(ms.value)

    def __del__(self):
        try:
            if self.handle:
                _lib.load().ns_event_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
