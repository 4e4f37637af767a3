"""Backward of the DepthNet training step (Trainer.core_optimization_loop, Trainer.py:506-544) on HIP kernels.

What needs gradients in the reference's training step (`train_depth_net_only`, run.py:105):
  * DepthNet: all weights (depth_net.py:117-169), from d(loss)/d(z)
  * the frozen NeRF: only w.r.t. its input point (one sample per ray at the predicted depth,
    nerf_utils.py:692-715) -- its weights are frozen (Trainer.py:724-728)
  * pts = o + d*z, and the single-sample compositing (rgb = sigmoid(raw rgb), see ns_raw2outputs N == 1)
Beyond the training step, compositing at any N (Composite: ns_raw2outputs_backward) and sample placement (PlaceSamples:
ns_place_samples_backward) make the DepthNet branch of render_rays_test differentiable end to end.
The vanilla coarse+fine pass that produces the target depth runs without gradients on the fused path.

Each torch.autograd.Function below runs its arithmetic in libnerf_sampling_hip.so (ns_gemm_strided,
ns_act_*, ns_posenc[_backward], ns_points_backward, ns_raw2outputs_backward, ns_place_samples_backward); torch is used for tensor storage and `cat`/slicing.
Training batches are N_rand = 1024 rays: launch-bound, so layers are individual fp32 GEMMs here rather than
the fused inference kernels.
The field fit (NerfFunction, trainers.FieldFitter) runs the same layers over 1024 rays x 64 .. 192 samples: its grad-weight
products are ns_gemm_wgrad (split-K), and with engine="tall" its layer forwards and grad-input products are ns_gemm_tall (a
workgroup per 128 rows and all columns) instead of ns_gemm_fused.
"""

from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch

from . import _lib, ops
from ._lib import check
from .ops import _dev, _ptr, _stream

Tensor = torch.Tensor
NONE, RELU, LEAKY, SIGMOID = 0, 1, 2, 3


def _gemm(A: Tensor, sa0: int, sa1: int, B: Tensor, sb0: int, sb1: int, bias: Optional[Tensor], M: int, N: int, K: int,
          out: Optional[Tensor] = None, accumulate: bool = False, act: int = 0, dact: int = 0,
          dact_ref: Optional[Tensor] = None, a_rowsum: Optional[Tensor] = None) -> Tensor:
    """C = A B^T (+ bias) through ns_gemm_fused; ``out`` may be a strided [M, N] view (its row stride is the leading
    dimension).  Epilogues: ``act`` on the result; ``dact``: result *= act'(.) evaluated from the activation OUTPUT
    ``dact_ref`` [M, N] (may be strided); ``a_rowsum`` [M] <- sum_k A[i, k]."""
    lib = _lib.load()
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    check(lib.ns_gemm_fused(_ptr(A), sa0, sa1, _ptr(B), sb0, sb1, _ptr(bias), _ptr(out), out.stride(0), M, N, K,
                            int(accumulate), int(act), int(dact), _ptr(dact_ref), 0 if dact_ref is None else dact_ref.stride(0),
                            _ptr(a_rowsum), _stream(A.device)), "ns_gemm_fused")
    return out


def _gemm_batched(problems) -> None:
    """Up to four GEMMs of the same kind in ONE launch (ns_gemm_fused_batched).  Each problem: the keyword arguments of
    ``_gemm`` with ``out`` given (A, sa0, sa1, B, sb0, sb1, bias, M, N, K, out, accumulate, act, dact, dact_ref, a_rowsum)."""
    lib = _lib.load()
    arr = (_lib.GemmProblem * len(problems))()
    dev = problems[0]["A"].device
    for q, pr in zip(arr, problems):
        out, ref = pr["out"], pr.get("dact_ref")
        q.A_dev, q.sa0, q.sa1 = pr["A"].data_ptr(), pr["sa0"], pr["sa1"]
        q.B_dev, q.sb0, q.sb1 = pr["B"].data_ptr(), pr["sb0"], pr["sb1"]
        q.bias_dev = None if pr.get("bias") is None else pr["bias"].data_ptr()
        q.C_dev, q.ldc = out.data_ptr(), out.stride(0)
        q.M, q.N, q.K = pr["M"], pr["N"], pr["K"]
        q.accumulate, q.act, q.dact = int(pr.get("accumulate", False)), int(pr.get("act", 0)), int(pr.get("dact", 0))
        q.dact_ref_dev, q.ld_ref = (None, 0) if ref is None else (ref.data_ptr(), ref.stride(0))
        q.a_rowsum_dev = None if pr.get("a_rowsum") is None else pr["a_rowsum"].data_ptr()
    check(lib.ns_gemm_fused_batched(arr, len(problems), _stream(dev)), "ns_gemm_fused_batched")


def linear_forward(x: Tensor, W: Tensor, b: Optional[Tensor], act: int = NONE) -> Tensor:
    """act(x @ W.T + b): x [M,K], W [N,K] (nn.Linear layout)."""
    x, W = _dev(x, "x"), _dev(W, "weight")
    M, K = x.shape
    N = W.shape[0]
    y = _gemm(x, K, 1, W, K, 1, None if b is None else _dev(b, "bias"), M, N, K)
    if act != NONE:
        check(_lib.load().ns_act_forward(_ptr(y), y.numel(), act, _stream(y.device)), "ns_act_forward")
    return y


def linear_backward_input(dy: Tensor, W: Tensor, n_cols: Optional[int] = None) -> Tensor:
    """dx[:, :n_cols] = dy @ W[:, :n_cols]   (dy [M,N], W [N,K])."""
    dy, W = _dev(dy, "dy"), _dev(W, "weight")
    M, N = dy.shape
    K = W.shape[1]
    return _gemm(dy, N, 1, W, 1, K, None, M, n_cols or K, N)


GEMM_ENGINES = ("tile", "tall")


def _check_engine(engine: str) -> str:
    if engine not in GEMM_ENGINES:
        raise ValueError(f"gemm engine must be one of {GEMM_ENGINES}, got {engine!r}")
    return engine


def _tall_operand(t: Tensor, name: str) -> Tensor:
    """A [rows, n] float32 GPU matrix that is contiguous along its columns (a column slice of a wider buffer is fine)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); this path has no CPU fallback")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if t.dim() != 2:
        raise ValueError(f"{name}: a 2-D tensor expected, got {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name} must be contiguous along its columns (strides {tuple(t.stride())})")
    return t


def _gemm_tall(A: Tensor, B: Tensor, sb0: int, sb1: int, bias: Optional[Tensor], N: int, K: int, out: Optional[Tensor] = None,
               accumulate: bool = False, act: int = 0, dact: int = 0, dact_ref: Optional[Tensor] = None) -> Tensor:
    """C = A B^T (+ bias), act, dact through ns_gemm_tall: A [rows, K], ``out`` [rows, N] and ``dact_ref`` [rows, N] may be
    column slices of wider buffers (their row strides are the leading dimensions)."""
    rows = A.shape[0]
    if out is None:
        out = torch.empty((rows, N), dtype=torch.float32, device=A.device)
    elif tuple(out.shape) != (rows, N):
        raise ValueError(f"out must be [{rows}, {N}], got {tuple(out.shape)}")
    if dact_ref is not None and tuple(dact_ref.shape) != (rows, N):
        raise ValueError(f"dact_ref must be [{rows}, {N}], got {tuple(dact_ref.shape)}")
    if rows == 0:
        return out
    check(_lib.load().ns_gemm_tall(_ptr(A), A.stride(0), _ptr(B), sb0, sb1, _ptr(bias), _ptr(out), out.stride(0), rows, N, K,
                                   int(accumulate), int(act), int(dact), _ptr(dact_ref),
                                   0 if dact_ref is None else dact_ref.stride(0), _stream(A.device)), "ns_gemm_tall")
    return out


def linear_forward_tall(x: Tensor, W: Tensor, b: Optional[Tensor], act: int = NONE, out: Optional[Tensor] = None) -> Tensor:
    """act(x @ W.T + b) on ns_gemm_tall: x [M,K] and ``out`` [M,N] may be column slices of wider buffers (contiguous along
    their columns), W [N,K] is in nn.Linear layout, N and K at most 512."""
    x, W = _tall_operand(x, "x"), _dev(W, "weight")
    if W.dim() != 2 or W.shape[1] != x.shape[1] or not W.is_contiguous():
        raise ValueError(f"weight must be a contiguous [N, {x.shape[1]}] matrix, got {tuple(W.shape)}")
    if b is not None:
        b = _dev(b, "bias")
        if tuple(b.shape) != (W.shape[0],) or not b.is_contiguous():
            raise ValueError(f"bias must be a contiguous [{W.shape[0]}] vector, got {tuple(b.shape)}")
    if out is not None:
        out = _tall_operand(out, "out")
    N, K = W.shape
    return _gemm_tall(x, W, K, 1, b, N, K, out=out, act=act)


def linear_backward_input_tall(dy: Tensor, W: Tensor, n_cols: Optional[int] = None, dact_ref: Optional[Tensor] = None,
                               dact: int = RELU, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """dx[:, :n_cols] = dy @ W[:, :n_cols] on ns_gemm_tall (dy [M,N], W [N,K], N and n_cols at most 512), times
    act'(``dact_ref``) when the activation output ``dact_ref`` [M,n_cols] of the layer below is given (``dact``: which
    activation, ReLU by default).  dy, ``dact_ref`` and ``out`` may be column slices of wider buffers; ``accumulate`` adds the
    product to ``out`` before the derivative is applied."""
    dy, W = _tall_operand(dy, "dy"), _dev(W, "weight")
    if W.dim() != 2 or W.shape[0] != dy.shape[1] or not W.is_contiguous():
        raise ValueError(f"weight must be a contiguous [{dy.shape[1]}, K] matrix, got {tuple(W.shape)}")
    Kw = W.shape[1]
    n = Kw if n_cols is None else int(n_cols)
    if not 1 <= n <= Kw:
        raise ValueError(f"n_cols must be in [1, {Kw}], got {n_cols}")
    if dact_ref is not None:
        dact_ref = _tall_operand(dact_ref, "dact_ref")
    if out is not None:
        out = _tall_operand(out, "out")
    return _gemm_tall(dy, W, 1, Kw, None, n, dy.shape[1], out=out, accumulate=accumulate,
                      dact=dact if dact_ref is not None else 0, dact_ref=dact_ref)


def linear_backward_weight(dy: Tensor, x: Tensor):
    """dW = dy.T @ x [N,K], db = dy.sum(0) [N]."""
    dy, x = _dev(dy, "dy"), _dev(x, "x")
    M, N = dy.shape
    K = x.shape[1]
    dW = _gemm(dy, 1, N, x, 1, K, None, N, K, M)
    db = torch.empty((N,), dtype=torch.float32, device=dy.device)
    check(_lib.load().ns_colsum(_ptr(dy), N, M, N, _ptr(db), _stream(dy.device)), "ns_colsum")
    return dW, db


_WGRAD_WORKSPACE = {}        # device -> byte tensor: the split-K partial tiles of ns_gemm_wgrad, one buffer per device


def _wgrad_workspace(dev, nbytes: int) -> Optional[Tensor]:
    """The device's split-K workspace, grown on demand (calls on one stream run in order, so one buffer serves them all)"""
    if nbytes == 0:
        return None
    ws = _WGRAD_WORKSPACE.get(dev)
    if ws is None or ws.numel() < nbytes:
        ws = _WGRAD_WORKSPACE[dev] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    return ws


def linear_backward_weight_splitk(dy: Tensor, x: Tensor, want_db: bool = True):
    """dW = dy.T @ x [N,K], db = dy.sum(0) [N] (None without ``want_db``) on ns_gemm_wgrad: the rows are split over workgroups
    and the slices summed in a fixed order.  dy [M,N] and x [M,K] may be strided views (x contiguous along K)."""
    lib = _lib.load()
    if not (dy.is_cuda and x.is_cuda and dy.dtype == torch.float32 and x.dtype == torch.float32):
        raise RuntimeError("dy and x must be float32 tensors on the GPU; this path has no CPU fallback")
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] != x.shape[0]:
        raise ValueError(f"dy [M,N] and x [M,K] expected, got {tuple(dy.shape)} and {tuple(x.shape)}")
    if x.stride(1) != 1 and x.shape[1] > 1:
        x = x.contiguous()
    M, N = dy.shape
    K = x.shape[1]
    dev = dy.device
    dW = torch.empty((N, K), dtype=torch.float32, device=dev)
    db = torch.empty((N,), dtype=torch.float32, device=dev) if want_db else None
    ws = _wgrad_workspace(dev, int(lib.ns_gemm_wgrad_workspace_bytes(M, N, K)))
    check(lib.ns_gemm_wgrad(_ptr(dy), dy.stride(0), dy.stride(1), _ptr(x), x.stride(0), M, N, K, _ptr(dW), K, 0, _ptr(db),
                            _ptr(ws), _stream(dev)), "ns_gemm_wgrad")
    return dW, db


def act_backward_(dy: Tensor, y: Tensor, act: int) -> Tensor:
    if act != NONE:
        check(_lib.load().ns_act_backward(_ptr(dy), _ptr(y), dy.numel(), act, _stream(dy.device)), "ns_act_backward")
    return dy


def posenc_backward(x: Tensor, de: Tensor, n_freqs: int) -> Tensor:
    x, de = _dev(x, "x"), _dev(de, "de")
    dx = torch.empty_like(x)
    check(_lib.load().ns_posenc_backward(_ptr(x), _ptr(de), x.shape[0], x.shape[1], n_freqs, _ptr(dx), _stream(x.device)),
          "ns_posenc_backward")
    return dx


# ---- pts = o + d * z -----------------------------------------------------------------------------------
class PointsAlongRays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o: Tensor, d: Tensor, z: Tensor):
        ctx.save_for_backward(d)
        return ops.points_along_rays(o, d, z)

    @staticmethod
    def backward(ctx, dpts: Tensor):
        (d,) = ctx.saved_tensors
        dpts = _dev(dpts, "dpts")
        R, N = dpts.shape[0], dpts.shape[1]
        dz = torch.empty((R, N), dtype=torch.float32, device=dpts.device)
        check(_lib.load().ns_points_backward(_ptr(dpts), _ptr(_dev(d, "d")), R, N, _ptr(dz), _stream(dpts.device)),
              "ns_points_backward")
        return None, None, dz


def points_along_rays(o: Tensor, d: Tensor, z: Tensor) -> Tensor:
    if torch.is_grad_enabled() and z.requires_grad:
        return PointsAlongRays.apply(o, d, z)
    return ops.points_along_rays(o, d, z)


# ---- single-sample compositing: rgb_map = sigmoid(raw rgb) -------------------------------------------------
class SingleSampleComposite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw: Tensor, z: Tensor, rays_d: Tensor, white_bkgd: bool):
        rgb, disp, acc, depth, alphas, weights = ops.raw2outputs(raw, z, rays_d, None, white_bkgd)
        ctx.save_for_backward(rgb)
        ctx.mark_non_differentiable(disp, acc, depth, alphas, weights)
        return rgb, disp, acc, depth, alphas, weights

    @staticmethod
    def backward(ctx, drgb, *_unused):
        (rgb,) = ctx.saved_tensors
        g = _dev(drgb, "drgb").clone()
        act_backward_(g, rgb, SIGMOID)                      # d sigmoid = y (1 - y)
        draw = torch.zeros((rgb.shape[0], 1, 4), dtype=torch.float32, device=rgb.device)
        draw[:, 0, :3] = g
        return draw, None, None, None


# ---- compositing at any N, with or without noise (sampling_trainer.py:153-230) ------------------------------------
class Composite(torch.autograd.Function):
    """forward: ns_raw2outputs; backward: ns_raw2outputs_backward, which re-runs the forward from the saved INPUTS (raw, z,
    rays_d, noise) and returns the gradients of raw, z and rays_d (the noise is a constant).  An output that takes no part in
    the loss sends no gradient (NULL), not zeros: a zero times an inf of the forward would be a NaN torch does not produce."""

    @staticmethod
    def forward(ctx, raw: Tensor, z: Tensor, rays_d: Tensor, noise: Optional[Tensor], white_bkgd: bool):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(raw, z, rays_d, noise)
        ctx.white_bkgd = bool(white_bkgd)
        out = ops.raw2outputs(raw, z, rays_d, noise, white_bkgd)
        return out

    @staticmethod
    def backward(ctx, *grads):
        raw, z, rays_d, noise = ctx.saved_tensors
        want = ctx.needs_input_grad[:3]
        if not any(want) or all(g is None for g in grads):
            return None, None, None, None, None
        d_raw, d_z, d_d = ops.raw2outputs_backward(raw, z, rays_d, noise, ctx.white_bkgd, grads, want)
        return d_raw, d_z, d_d, None, None


def composite(raw: Tensor, z: Tensor, rays_d: Tensor, noise: Optional[Tensor], white_bkgd: bool):
    """raw2outputs' six maps (rgb, disp, acc, depth, alphas, weights), differentiable in raw, z and rays_d"""
    return Composite.apply(raw, z, rays_d, noise, bool(white_bkgd))


# ---- sample placement around the predicted depth (utils.py:220-244) --------------------------------------------------
class PlaceSamples(torch.autograd.Function):
    """z [R,N] from mean [R] (ns_place_samples, its own draws for the gaussian mode); backward: ns_place_samples_backward."""

    @staticmethod
    def forward(ctx, mean: Tensor, o: Tensor, d: Tensor, n_samples: int, mode: str, std: float):
        _, z = ops.place_samples(o, d, mean, n_samples, mode, std, want_pts=False)
        ctx.save_for_backward(mean)
        ctx.mode, ctx.std = mode, float(std)
        return z

    @staticmethod
    def backward(ctx, dz: Tensor):
        (mean,) = ctx.saved_tensors
        return ops.place_samples_backward(mean, dz, ctx.mode, ctx.std), None, None, None, None, None


def place_samples(o: Tensor, d: Tensor, mean: Tensor, n_samples: int, mode: str, std: float):
    """pts [R,N,3], z [R,N] of sample_points_around_mean, differentiable in mean: mean -> z (PlaceSamples) -> pts
    (PointsAlongRays).  The same kernels as ops.place_samples, so the same values."""
    z = PlaceSamples.apply(mean.reshape(-1), o, d, n_samples, mode, std)
    return PointsAlongRays.apply(o, d, z), z


# ---- the NeRF layer by layer: shared by NerfInputGrad (frozen field) and NerfFunction (field fit) --------------------------
def _nerf_layers_forward(net, xe: Tensor, ve: Optional[Tensor], want_raw: bool, engine: str = "tile"):
    """NeRF.forward (run_nerf_helpers.py:114-133) on _gemm with the ReLU in the epilogue, from the module's live parameters.
    xe [M,63], ve [M,27] (view-direction head only).  Returns (raw [M,C] or None, saved): saved holds what the backward reads --
    ``acts`` (each trunk layer's output), ``ins`` (each trunk layer's input: xe, the layer below's output or the cat[xe, h]
    buffer), ``h`` (the trunk's output), and for the view-direction head ``vin`` = cat[feature, ve] and ``hv``.
    ``engine``: "tile" (ns_gemm_fused) or "tall" (ns_gemm_tall, the throughput kernel for the field fit's row counts)."""
    skips = net._check_supported()
    M = xe.shape[0]
    tall = _check_engine(engine) == "tall"

    def fwd(x, lin, act, out=None):    # act(x W^T + b), activation in the GEMM epilogue
        if tall:
            return linear_forward_tall(x, lin.weight, lin.bias, act, out=out)
        return _gemm(x, x.stride(0), 1, lin.weight, lin.weight.shape[1], 1, lin.bias, M, lin.weight.shape[0], x.shape[1], act=act,
                     out=out)

    acts, ins = [], []
    h = xe
    for i, lin in enumerate(net.pts_linears):               # (run_nerf_helpers.py:114-118)
        ins.append(h)
        if tall and i in skips:          # the layer writes its output into its column slice of the cat[xe, h] buffer
            cat = torch.empty((M, xe.shape[1] + lin.weight.shape[0]), dtype=torch.float32, device=xe.device)
            cat[:, :xe.shape[1]] = xe
            acts.append(fwd(h, lin, RELU, out=cat[:, xe.shape[1]:]))
            h = cat
            continue
        h = fwd(h, lin, RELU)
        acts.append(h)
        if i in skips:
            h = torch.cat([xe, h], -1)
    saved = dict(xe=xe, acts=acts, ins=ins, h=h, skips=skips)
    raw = None
    if net.use_viewdirs:                  # alpha / feature / views / rgb head (run_nerf_helpers.py:119-131)
        feat = fwd(h, net.feature_linear, NONE)
        vin = torch.cat([feat, ve], -1)
        hv = fwd(vin, net.views_linears[0], RELU)
        saved.update(vin=vin, hv=hv)
        if want_raw:
            raw = torch.empty((M, 4), dtype=torch.float32, device=xe.device)
            fwd(hv, net.rgb_linear, NONE, out=raw[:, :3])
            fwd(h, net.alpha_linear, NONE, out=raw[:, 3:4])
    elif want_raw:                        # output_linear head (:132-133)
        raw = fwd(h, net.output_linear, NONE)
    return raw, saved


def _nerf_layers_backward(net, saved, draw: Tensor, weight_grad=None, want_input: bool = True,
                          engine: str = "tile") -> Optional[Tensor]:
    """The transposed chain from d raw down to the embedded point: returns d xe [M,63] (None without ``want_input``: the
    grad-input GEMM of layer 0 is then skipped).  ``weight_grad(lin, dy, x)`` is called once per Linear with the gradient of its
    pre-activation output and its input.  ``engine``: as in _nerf_layers_forward, for every grad-input product."""
    xe, acts, skips = saved["xe"], saved["acts"], saved["skips"]
    lins = list(net.pts_linears)
    M = xe.shape[0]
    h = saved["h"]
    tall = _check_engine(engine) == "tall"

    def bwd(dy, lin, n_cols=None, dref=None):   # dy W[:, :n_cols], times relu'(dref) when the layer below has a ReLU
        Wt = lin.weight
        if tall:
            return linear_backward_input_tall(dy, Wt, n_cols, dact_ref=dref)
        return _gemm(dy, dy.stride(0), 1, Wt, 1, Wt.shape[1], None, M, n_cols or Wt.shape[1], dy.shape[1],
                     dact=RELU if dref is not None else 0, dact_ref=dref)

    wg = weight_grad or (lambda lin, dy, x: None)
    last = len(lins) - 1
    # d h_last: through the head, then times relu'(trunk output) -- the trunk's last activation.  When that output was
    # concatenated with the embedding (a skip after the last layer cannot occur: _check_supported), plain [M, W].
    if net.use_viewdirs:
        hv = saved["hv"]
        g = _dev(draw, "draw").reshape(-1, 4)
        g_rgb, g_sigma = g[:, :3], g[:, 3:4]                         # strided views, no copies
        wg(net.rgb_linear, g_rgb, hv)
        d_hv = bwd(g_rgb, net.rgb_linear, dref=hv)
        wg(net.views_linears[0], d_hv, saved["vin"])
        d_feat = bwd(d_hv, net.views_linears[0], n_cols=net.W)
        wg(net.feature_linear, d_feat, h)
        d_h = bwd(d_feat, net.feature_linear)
        # + the sigma head, accumulated in place, then the trunk's last ReLU on the sum
        wg(net.alpha_linear, g_sigma, h)
        Wa = net.alpha_linear.weight
        if tall:
            linear_backward_input_tall(g_sigma, Wa, dact_ref=acts[last], out=d_h, accumulate=True)
        else:
            _gemm(g_sigma, g_sigma.stride(0), 1, Wa, 1, Wa.shape[1], None, M, Wa.shape[1], 1, out=d_h, accumulate=True,
                  dact=RELU, dact_ref=acts[last])
    else:                             # output_linear head (:132-133): raw = h W_out^T + b, no view directions
        g = _dev(draw, "draw").reshape(-1, net.output_channels)
        wg(net.output_linear, g, h)
        d_h = bwd(g, net.output_linear, dref=acts[last])
    d_xe = torch.zeros_like(xe) if want_input else None
    for i in range(last, -1, -1):     # d_h is the gradient w.r.t. the PRE-activation of layer i here
        wg(lins[i], d_h, saved["ins"][i])
        below = i - 1
        if below >= 0 and below in skips and tall:      # layer i saw cat[xe, h_{i-1}]: the two column ranges of W apart
            Wt = lins[i].weight
            if want_input:
                d_xe = d_xe + bwd(d_h, lins[i], n_cols=63)   # the xe part has no activation
            d_h = _gemm_tall(d_h, Wt[:, 63:], 1, Wt.shape[1], None, Wt.shape[1] - 63, d_h.shape[1], dact=RELU,
                             dact_ref=acts[below])
        elif below >= 0 and below in skips:
            d_in = bwd(d_h, lins[i])                     # [M, 63 + W]: the xe part has no activation
            if want_input:
                d_xe = d_xe + d_in[:, :63]
            d_h = d_in[:, 63:].contiguous()
            act_backward_(d_h, acts[below], RELU)
        elif below >= 0:
            d_h = bwd(d_h, lins[i], dref=acts[below])
        elif want_input:
            d_h = bwd(d_h, lins[i])                      # layer 0's input is xe
    return d_xe + d_h if want_input else None


def _nerf_embed(pts: Tensor, viewdirs: Optional[Tensor], use_viewdirs: bool):
    """flat points [M,3], their embedding [M,63] and the samples' embedded view directions [M,27] (or None)"""
    flat = pts.reshape(-1, 3).contiguous()
    xe = ops.posenc(flat, 10)
    ve = None
    if use_viewdirs:
        dirs = viewdirs[:, None].expand(pts.shape).reshape(-1, 3).contiguous()
        ve = ops.posenc(dirs, 4)
    return flat, xe, ve


# ---- frozen NeRF, gradient w.r.t. the input points -------------------------------------------------------
class NerfInputGrad(torch.autograd.Function):
    """forward: the fused MFMA kernel; backward: recompute the layers in fp32 (masks for ReLU), then the
    transposed chain down to the embedded point and through the positional encoding."""

    @staticmethod
    def forward(ctx, pts: Tensor, viewdirs: Tensor, net):
        ctx.net = net
        ctx.save_for_backward(pts, viewdirs)
        return ops.nerf_forward(net.packed(), pts, viewdirs)

    @staticmethod
    def backward(ctx, draw: Tensor):
        pts, viewdirs = ctx.saved_tensors
        net = ctx.net
        R, N = pts.shape[0], pts.shape[1]
        flat, xe, ve = _nerf_embed(pts, viewdirs, net.use_viewdirs)
        _, saved = _nerf_layers_forward(net, xe, ve, want_raw=False)     # recompute (run_nerf_helpers.py:114-118)
        d_xe = _nerf_layers_backward(net, saved, draw)
        dpts = posenc_backward(flat, d_xe.contiguous(), 10)
        return dpts.reshape(R, N, 3), None, None


# ---- the NeRF, gradient w.r.t. its weights (and its points, when they ask for one) -----------------------------------------
def nerf_params(net) -> List[Tensor]:
    """The NeRF's parameters in NerfFunction's order: [w, b] of pts_linears, then feature, alpha, views, rgb (view-direction
    head) or output_linear."""
    mods = list(net.pts_linears) + ([net.feature_linear, net.alpha_linear, net.views_linears[0], net.rgb_linear]
                                    if net.use_viewdirs else [net.output_linear])
    params = []
    for m in mods:
        params += [m.weight, m.bias]
    return params


class NerfFunction(torch.autograd.Function):
    """raw [R,N,C] of NeRF.forward (run_nerf_helpers.py:67-134) from the module's live parameters, layer by layer on
    ns_gemm_fused (``engine`` "tile") or ns_gemm_tall ("tall") (no packed stream: nothing is repacked inside a training loop); the activations are kept.  backward: the
    grad-input chain NerfInputGrad runs, one ns_gemm_wgrad per Linear for (dW, db), and the gradient of ``pts`` (through the
    positional encoding) only when pts.requires_grad.  Any ``skips``, both heads, any W <= 256."""

    @staticmethod
    def forward(ctx, pts: Tensor, viewdirs: Optional[Tensor], net, engine: str, *params: Tensor):
        flat, xe, ve = _nerf_embed(pts, viewdirs, net.use_viewdirs)
        raw, saved = _nerf_layers_forward(net, xe, ve, want_raw=True, engine=engine)
        ctx.net, ctx.saved, ctx.flat, ctx.engine = net, saved, flat, engine
        ctx.pts_shape = tuple(pts.shape)
        return raw.reshape(pts.shape[0], pts.shape[1], raw.shape[1])

    @staticmethod
    def backward(ctx, draw: Tensor):
        net, saved = ctx.net, ctx.saved
        params = nerf_params(net)
        slot = {id(p): k for k, p in enumerate(params)}
        grads: List[Optional[Tensor]] = [None] * len(params)

        def weight_grad(lin, dy, x):
            kw, kb = slot[id(lin.weight)], slot[id(lin.bias)]
            if not (ctx.needs_input_grad[4 + kw] or ctx.needs_input_grad[4 + kb]):
                return
            grads[kw], grads[kb] = linear_backward_weight_splitk(dy, x)

        want_pts = ctx.needs_input_grad[0]
        d_xe = _nerf_layers_backward(net, saved, draw, weight_grad=weight_grad, want_input=want_pts, engine=ctx.engine)
        dpts = posenc_backward(ctx.flat, d_xe.contiguous(), 10).reshape(ctx.pts_shape) if want_pts else None
        ctx.saved = None
        return (dpts, None, None, None, *grads)


def nerf_forward_train(net, pts: Tensor, viewdirs: Optional[Tensor], engine: str = "tile") -> Tensor:
    """raw [R,N,C] of ``net`` at pts [R,N,3] (viewdirs [R,3], or None for a network without view directions), differentiable in
    the network's parameters and, when it requires a gradient, in ``pts`` (NerfFunction).  ``engine``: "tile" runs the layer
    forwards and grad-input products on ns_gemm_fused, "tall" on ns_gemm_tall; grad-weight is ns_gemm_wgrad either way."""
    _check_engine(engine)
    pts = _dev(pts, "pts")
    if net.use_viewdirs:
        viewdirs = _dev(viewdirs, "viewdirs")
    else:
        viewdirs = None
    return NerfFunction.apply(pts, viewdirs, net, engine, *nerf_params(net))


# ---- DepthNet, gradient w.r.t. its weights -----------------------------------------------------------------
class DepthNetFunction(torch.autograd.Function):
    """forward/backward of depth_net.py:117-169 layer by layer (affine skip branches, LeakyReLU trunk, sigmoid
    head).  params = [w, b] * (4 n + 1) in the order origin, direction, intersection, trunk, head.

    Round 4: no elementwise kernels beside the GEMMs.  A branch layer's input cat[h, e] is a row of ONE buffer per branch
    whose embedding columns are filled once, and each layer's GEMM writes its output straight into the next layer's h
    columns (the last one into the trunk's input): no torch.cat.  Activations (forward) and their derivatives (backward: the
    grad-input GEMM of the layer above multiplies by this layer's act') run in the GEMM epilogues, the bias gradient is a
    row sum the grad-weight GEMM takes along, and strided views replace the .contiguous() copies (ns_gemm_fused)."""

    @staticmethod
    def forward(ctx, o: Tensor, d: Tensor, near: float, far: float, radius: float, n: int, *params: Tensor):
        W_ = params[0::2]
        B_ = params[1::2]
        ctx.no_rays = o.shape[0] == 0
        if ctx.no_rays:        # nothing to launch (the batched GEMM takes no empty problem): z is empty, every gradient zero
            ctx.param_like = [(p.shape, p.device) for p in params]
            return torch.empty((0, 1), dtype=torch.float32, device=o.device)
        e_o, e_d = ops.posenc(o, 10), ops.posenc(d, 10)
        _, P = ops.sphere_intersect(o, d, radius)
        e_x = ops.posenc(P.reshape(-1, 6), 10)
        M, width, dev = o.shape[0], W_[0].shape[0], o.device
        embs = (e_o, e_d, e_x)
        Es = [e.shape[1] for e in embs]
        # trunk input: cat[h_o, h_d, h_x, e_o, e_d, e_x]; the branches write their last layer into the h columns
        y0 = torch.empty((M, 3 * width + sum(Es)), dtype=torch.float32, device=dev)
        col = 3 * width
        for e, E in zip(embs, Es):
            y0[:, col : col + E] = e
            col += E
        saved_in: List[Optional[Tensor]] = [None] * (3 * n)
        bufs, inp = [], []
        for b, (e, E) in enumerate(zip(embs, Es)):
            inp.append(torch.cat([e, e], -1))                           # layer 0 sees cat[h = e, e]
            bufs.append(torch.empty((max(n - 1, 1), M, width + E), dtype=torch.float32, device=dev))   # inputs of layers 1 .. n-1
            if n > 1:
                bufs[b][:, :, width:] = e                               # one broadcast copy: the e columns of every layer
        for i in range(n):                                              # layer i of the three branches in ONE launch
            probs = []
            for b in range(3):
                x, Wt = inp[b], W_[b * n + i]
                saved_in[b * n + i] = x
                out = y0[:, b * width : (b + 1) * width] if i == n - 1 else bufs[b][i][:, :width]
                probs.append(dict(A=x, sa0=x.stride(0), sa1=1, B=Wt, sb0=Wt.shape[1], sb1=1, bias=B_[b * n + i], M=M, N=width,
                                  K=x.shape[1], out=out))
                if i < n - 1:
                    inp[b] = bufs[b][i]
            _gemm_batched(probs)
        y = y0
        trunk_io = []
        for i in range(n):
            out = _gemm(y, y.stride(0), 1, W_[3 * n + i], W_[3 * n + i].shape[1], 1, B_[3 * n + i], M, width, y.shape[1], act=LEAKY)
            trunk_io.append((y, out))
            y = out
        s = _gemm(y, y.stride(0), 1, W_[4 * n], W_[4 * n].shape[1], 1, B_[4 * n], M, 1, width, act=SIGMOID)
        ctx.n, ctx.scale, ctx.width = n, float(far) - float(near), width
        ctx.saved_in, ctx.trunk_io, ctx.last, ctx.s = saved_in, trunk_io, y, s
        ctx.weights = W_
        return near * (1 - s) + far * s                      # depth_net.py:168

    @staticmethod
    def backward(ctx, dz: Tensor):
        if ctx.no_rays:
            zeros = [torch.zeros(shape, dtype=torch.float32, device=dev) for shape, dev in ctx.param_like]
            return (None, None, None, None, None, None, *zeros)
        n, W_, width = ctx.n, ctx.weights, ctx.width
        grads: List[Optional[Tensor]] = [None] * (2 * (4 * n + 1))
        dev = ctx.s.device

        def weight_grads(slot, dy, x):
            """dW = dy^T x [N, K] and db = column sums of dy (the row sums of A = dy^T) in ONE launch"""
            M_, N_, K_ = dy.shape[0], dy.shape[1], x.shape[1]
            db = torch.empty((N_,), dtype=torch.float32, device=dev)
            dW = _gemm(dy, 1, dy.stride(0), x, 1, x.stride(0), None, N_, K_, M_, a_rowsum=db)
            grads[2 * slot], grads[2 * slot + 1] = dW, db

        g = _dev(dz, "dz") * ctx.scale
        act_backward_(g, ctx.s, SIGMOID)
        weight_grads(4 * n, g, ctx.last)
        # d(trunk output n-1) = (g W_head) * leaky'(out_{n-1})
        Wh = W_[4 * n]
        d_y = _gemm(g, g.stride(0), 1, Wh, 1, Wh.shape[1], None, g.shape[0], width, 1, dact=LEAKY, dact_ref=ctx.trunk_io[n - 1][1])
        for i in range(n - 1, -1, -1):
            y_in, _y_out = ctx.trunk_io[i]
            weight_grads(3 * n + i, d_y, y_in)
            Wi = W_[3 * n + i]
            if i > 0:      # through the trunk layer below and ITS activation
                d_y = _gemm(d_y, d_y.stride(0), 1, Wi, 1, Wi.shape[1], None, d_y.shape[0], width, width, dact=LEAKY,
                            dact_ref=ctx.trunk_io[i - 1][1])
            else:          # below trunk layer 0 only the three (affine) branch outputs need a gradient
                d_y = _gemm(d_y, d_y.stride(0), 1, Wi, 1, Wi.shape[1], None, d_y.shape[0], 3 * width, width)
        d_h = [d_y[:, b * width : (b + 1) * width] for b in range(3)]   # strided views: no copies
        M = d_y.shape[0]
        for i in range(n - 1, -1, -1):                                  # layer i of the three branches: two launches
            probs = []
            for b in range(3):
                x = ctx.saved_in[b * n + i]
                db = torch.empty((width,), dtype=torch.float32, device=dev)
                dW = torch.empty((width, x.shape[1]), dtype=torch.float32, device=dev)
                grads[2 * (b * n + i)], grads[2 * (b * n + i) + 1] = dW, db
                probs.append(dict(A=d_h[b], sa0=1, sa1=d_h[b].stride(0), B=x, sb0=1, sb1=x.stride(0), M=width, N=x.shape[1], K=M,
                                  out=dW, a_rowsum=db))
            _gemm_batched(probs)
            if i > 0:
                probs, nxt = [], []
                for b in range(3):
                    Wi = W_[b * n + i]
                    out = torch.empty((M, width), dtype=torch.float32, device=dev)
                    nxt.append(out)
                    probs.append(dict(A=d_h[b], sa0=d_h[b].stride(0), sa1=1, B=Wi, sb0=1, sb1=Wi.shape[1], M=M, N=width, K=width, out=out))
                _gemm_batched(probs)
                d_h = nxt
        return (None, None, None, None, None, None, *grads)


def depthnet_params(net) -> List[Tensor]:
    """The DepthNet's parameters in DepthNetFunction's order: [w, b] of the origin, direction and intersection branches, the
    trunk, the head."""
    mods = (list(net.origin_layers) + list(net.direction_layers) + list(net.intersection_layers)
            + [m for m in net.cat_layers if isinstance(m, torch.nn.Linear)] + [net.to_depth[0]])
    params = []
    for m in mods:
        params += [m.weight, m.bias]
    return params


def depthnet_forward_train(net, o: Tensor, d: Tensor) -> Tensor:
    n, _width = net._train_shape()
    params = depthnet_params(net)
    return DepthNetFunction.apply(_dev(o, "rays_o"), _dev(d, "rays_d"), float(net.near), float(net.far),
                                  float(net.sphere_radius.reshape(-1)[0]), n, *params)


# ---- Adam on the HIP kernel, state-dict compatible with torch.optim.Adam -------------------------------------
class HipAdam(torch.optim.Adam):
    """torch.optim.Adam whose step() runs ns_adam_step; state ('step', 'exp_avg', 'exp_avg_sq') and therefore
    state_dict()/load_state_dict() are torch's, so the reference's checkpoints round-trip (utils.py:59-122).

    ``use_device_step()`` moves the step counter (and the learning rate) into device memory: step() then launches
    ns_add_i32 + ns_adam_step_dev and reads nothing from the host, which is what lets trainers.GraphedDepthNetStep
    capture forward + backward + update in one hipGraph.  The per-parameter 'step' entries of the state are brought up
    to date whenever the state is read (state_dict())."""

    _dev_step: Optional[Tensor] = None
    _dev_lr: Optional[Tensor] = None
    _table_event = None
    _host_steps = 0          # steps taken through the device counter (eager calls and graph replays alike)

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)
        return st

    def use_device_step(self):
        """Switch to the device-resident step counter (idempotent).  All parameters must share one step count."""
        if self._dev_step is not None:
            return
        params = [p for g in self.param_groups for p in g["params"]]
        dev = params[0].device
        self._host_steps = self._common_step(params)
        self._dev_step = torch.full((1,), self._host_steps, dtype=torch.int32, device=dev)
        self._dev_lr = torch.full((1,), float(self.param_groups[0]["lr"]), dtype=torch.float32, device=dev)
        self._lr_seen = float(self.param_groups[0]["lr"])
        # (a parameter gets its state with its first gradient, as in torch: one that never has a gradient keeps none)
        # two row tables, [0] for eager steps and [1] for a captured step (a replayed graph re-reads its pinned rows on
        # every replay, so eager steps taken after a capture must not touch them)
        self._table_host = [torch.empty((5 * len(params),), dtype=torch.int64, device="cpu").pin_memory() for _ in range(2)]
        self._table_dev = [torch.empty((5 * len(params),), dtype=torch.int64, device=dev) for _ in range(2)]
        self._table_event = None

    def _common_step(self, params) -> int:
        """The one step count all parameters share ('step' is a tensor in torch's own state, a plain int in older checkpoints)."""
        def as_int(v):
            return int(v.item()) if isinstance(v, torch.Tensor) else int(v)

        steps = {as_int(self.state[p]["step"]) for p in params if len(self.state.get(p, ()))}    # (stateless: no gradient yet)
        if len(steps) > 1 or len(self.param_groups) != 1:
            raise NotImplementedError("the device step counter needs one parameter group and one common step count")
        return steps.pop() if steps else 0

    def load_state_dict(self, state_dict):
        """torch's loader; in device-step mode the device counter, the host count and the learning-rate scalar are re-seeded
        from the loaded state (a checkpoint loaded AFTER use_device_step() must not keep the old bias corrections)."""
        super().load_state_dict(state_dict)
        for st in self.state.values():                       # torch's step() convention: 'step' is a CPU fp32 tensor
            if "step" in st and not isinstance(st["step"], torch.Tensor):
                st["step"] = torch.tensor(float(st["step"]))
        if self._dev_step is not None:
            params = [p for g in self.param_groups for p in g["params"]]
            self._host_steps = self._common_step(params)
            self._dev_step.fill_(self._host_steps)
            self._lr_seen = None
            self.sync_device_lr()

    def claim_capture_table(self):
        """Called once by the (single) captured step of this optimizer: the captured update re-reads row table [1] on every
        replay, so a second capture from the same optimizer would overwrite the rows the first graph points at.

        Every parameter gets its moments here, ahead of the capture: allocated and zeroed inside it, they would be zeroed
        again by every replay."""
        if getattr(self, "_capture_claimed", False):
            raise RuntimeError("this HipAdam already backs a captured step: one hipGraph capture per optimizer "
                               "(build a new optimizer, or reuse the existing GraphedDepthNetStep)")
        self._capture_claimed = True
        for g in self.param_groups:
            for p in g["params"]:
                self._init_state(p)

    def note_replayed_step(self):
        """A captured graph containing step() was replayed once."""
        self._host_steps += 1

    def sync_device_lr(self):
        """Publish param_groups[0]['lr'] to the device scalar the captured update reads (one tiny fill, only on change)."""
        lr = float(self.param_groups[0]["lr"])
        if self._dev_lr is not None and lr != self._lr_seen:
            self._dev_lr.fill_(lr)
            self._lr_seen = lr

    def state_dict(self):
        if self._dev_step is not None:
            for st in self.state.values():
                if "step" in st:
                    st["step"].fill_(float(self._host_steps))
        return super().state_dict()

    @torch.no_grad()
    def step(self, closure=None):
        lib = _lib.load()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            if group.get("weight_decay", 0) or group.get("amsgrad", False) or group.get("maximize", False):
                raise NotImplementedError("HipAdam implements plain Adam only")
            if self._dev_step is not None:
                capturing = torch.cuda.is_current_stream_capturing()
                if not capturing:
                    self.sync_device_lr()
                    self._host_steps += 1
                dev = self._dev_step.device
                check(lib.ns_add_i32(_ptr(self._dev_step), 1, _stream(dev)), "ns_add_i32")
                # one launch for all parameter tensors: {p, g, m, v, n} rows, staged through a pinned host tensor that was
                # allocated BEFORE any capture (use_device_step): an asynchronous copy from pinned memory is something a
                # hipGraph capture records (an allocation is not), and the rows stay valid across replays because the
                # captured backward writes its gradients to the same addresses every time
                rows, keep, max_n = [], [], 0
                for p in group["params"]:
                    if p.grad is None:
                        continue
                    st = self._init_state(p)
                    g = p.grad.contiguous()
                    keep.append(g)
                    rows += [p.data.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()]
                    max_n = max(max_n, p.numel())
                if rows:
                    if not capturing and self._table_event is not None:
                        self._table_event.synchronize()          # the previous step's copy of the rows has been taken
                    n_rows, k = len(rows) // 5, int(capturing)
                    self._table_host[k][: len(rows)].copy_(torch.tensor(rows, dtype=torch.int64, device="cpu"))
                    self._table_dev[k][: len(rows)].copy_(self._table_host[k][: len(rows)], non_blocking=True)
                    if not capturing:
                        self._table_event = torch.cuda.Event()
                        self._table_event.record(torch.cuda.current_stream(dev))
                    self._table_keep = keep                      # gradient tensors the launch reads
                    check(lib.ns_adam_step_multi_dev(_ptr(self._table_dev[k]), n_rows, max_n, float(group["lr"]),
                                                     _ptr(self._dev_lr), float(b1), float(b2), float(group["eps"]),
                                                     _ptr(self._dev_step), _stream(dev)), "ns_adam_step_multi_dev")
                continue
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self._init_state(p)
                g = p.grad.contiguous()
                if self._dev_step is not None:
                    check(lib.ns_adam_step_dev(_ptr(p.data), _ptr(g), _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"]), p.numel(),
                                               float(group["lr"]), _ptr(self._dev_lr), float(b1), float(b2),
                                               float(group["eps"]), _ptr(self._dev_step), _stream(p.device)),
                          "ns_adam_step_dev")
                    continue
                st["step"] += 1
                check(lib.ns_adam_step(_ptr(p.data), _ptr(g), _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"]), p.numel(),
                                       float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                       int(st["step"].item()), _stream(p.device)), "ns_adam_step")
        return None


# ---- the one-kernel renderer, differentiable in the DepthNet's depth (ns_render_rays_fused_tangent) ------------------------
def tangent_d_mean(J: dict, g_rgb, g_disp, g_depth, g_acc) -> Tensor:
    """d mean [R] = sum_k g_k J_k per ray, from the tangent kernel's Jacobian J = dict(rgb [R,3], disp, depth, acc [R]) and the
    upstream gradients of those maps (None: no gradient): the backward of DepthNetTangentRender down to the DepthNet's depth."""
    d_mean = torch.zeros_like(J["disp"])
    if g_rgb is not None:
        d_mean += (g_rgb * J["rgb"]).sum(-1)
    for g, k in ((g_disp, "disp"), (g_depth, "depth"), (g_acc, "acc")):
        if g is not None:
            d_mean += g.reshape(-1) * J[k]
    return d_mean


class DepthNetTangentRender(torch.autograd.Function):
    """rgb, disp, depth, acc of rays through DepthNet -> uniform placement -> a frozen f16x3 (or f16) field -> compositing, rendered in
    chunks by the tangent kernel; differentiable in the DepthNet's parameters.  The kernel returns each ray's Jacobian
    J = d{rgb, disp, depth, acc} / d mean beside its outputs, so the backward is d mean = sum_k g_k J_k per ray, then the DepthNet
    is run again chunk by chunk through DepthNetFunction and its gradients summed: what is held between forward and backward is
    J (six floats per ray); in the backward, one chunk's DepthNet activations."""

    @staticmethod
    def forward(ctx, o: Tensor, d: Tensor, viewdirs: Tensor, cfg: dict, *params: Tensor):
        net, nerf, chunk = cfg["depth_net"], cfg["nerf"], cfg["chunk"]
        outs = {k: [] for k in ("rgb", "disp", "depth", "acc")}
        jac = {k: [] for k in outs}
        for s in range(0, o.shape[0], chunk):
            sl = slice(s, s + chunk)
            mean = depthnet_forward_train(net, o[sl], d[sl]).reshape(-1)
            out, J = ops.render_rays_depthnet_tangent(mean, nerf, rays=(o[sl], d[sl], viewdirs[sl]), n_samples=cfg["n_samples"],
                                                      std=cfg["std"], extras=("depth", "acc"), white_bkgd=cfg["white_bkgd"],
                                                      approximate=cfg["approximate"], mode=cfg["mode"])
            for k in outs:
                outs[k].append(out[k])
                jac[k].append(J[k])
        ctx.cfg, ctx.n_params = cfg, len(params)
        ctx.jac = {k: torch.cat(v) for k, v in jac.items()}
        ctx.save_for_backward(o, d, *params)
        return tuple(torch.cat(outs[k]) for k in ("rgb", "disp", "depth", "acc"))

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_depth, g_acc):
        o, d, *params = ctx.saved_tensors
        d_mean = tangent_d_mean(ctx.jac, g_rgb, g_disp, g_depth, g_acc)
        net, chunk = ctx.cfg["depth_net"], ctx.cfg["chunk"]
        grads = [torch.zeros_like(p) for p in params]
        for s in range(0, o.shape[0], chunk):
            sl = slice(s, s + chunk)
            with torch.enable_grad():
                mean = depthnet_forward_train(net, o[sl], d[sl]).reshape(-1)
                gs = torch.autograd.grad(mean, params, d_mean[sl], allow_unused=True)
            for acc, g in zip(grads, gs):
                if g is not None:
                    acc += g
        return (None, None, None, None, *grads)


class SingleSampleTangentRender(torch.autograd.Function):
    """The DepthNet branch of the training operator (render_rays, nerf_utils.py:692-715) as ONE kernel: rgb_map [R,3] and disp_map
    [R] of one sample per ray at ``depth`` [R,1] (DepthNetFunction's output) through a frozen f16x3 field and raw2outputs'
    single-sample rule -- points_along_rays -> NerfInputGrad -> SingleSampleComposite, forward and derivative together
    (ns_render_rays_fused_tangent, NS_MODE_DEPTH_ONLY).  The forward saves J = d rgb / d depth [R,3]; the backward is
    d depth = sum_c g_rgb[:, c] J[:, c].  disp is the constant 1e10 and carries no gradient."""

    @staticmethod
    def forward(ctx, depth: Tensor, o: Tensor, d: Tensor, viewdirs: Tensor, nerf, workspace):
        out, J = ops.render_rays_depthnet_tangent(depth.reshape(-1), nerf, rays=(o, d, viewdirs), n_samples=1, std=0.0,
                                                  mode="depth_only", workspace=workspace, device=depth.device)
        ctx.save_for_backward(J["rgb"])
        ctx.depth_shape = depth.shape
        ctx.mark_non_differentiable(out["disp"])
        return out["rgb"], out["disp"]

    @staticmethod
    def backward(ctx, g_rgb, _g_disp):
        (J,) = ctx.saved_tensors
        return (g_rgb * J).sum(-1).reshape(ctx.depth_shape), None, None, None, None, None


def render_single_sample(depth: Tensor, o: Tensor, d: Tensor, viewdirs: Tensor, nerf, workspace=None):
    """(rgb_map [R,3], disp_map [R]) of one sample per ray at ``depth`` [R,1] or [R], differentiable in ``depth``
    (SingleSampleTangentRender); ``nerf``: an "f16x3" NeRF handle."""
    if getattr(nerf, "dtype", None) != "f16x3":
        raise NotImplementedError(f"the one-sample render needs an f16x3 NeRF handle, got {getattr(nerf, 'dtype', None)}")
    o, d, viewdirs = (_dev(t, n) for t, n in zip((o, d, viewdirs), ("rays_o", "rays_d", "viewdirs")))
    return SingleSampleTangentRender.apply(depth, o, d, viewdirs, nerf, workspace)


def render_depthnet_differentiable(depth_net, nerf, *, rays=None, camera=None, n_samples: int, std: float, chunk: int = 65536,
                                   white_bkgd: bool = True, approximate: bool = False, mode: str = "uniform"):
    """DepthNet -> sample_points_around_mean("uniform") -> frozen NeRF -> raw2outputs on the one-kernel renderer, differentiable
    in ``depth_net``'s parameters: dict(rgb [R,3], disp, depth, acc [R]) with a grad_fn (DepthNetTangentRender).  ``nerf``: an
    "f16x3" NeRF handle; ``rays`` = (o, d, viewdirs) device tensors or ``camera`` = (H, W, K, c2w, row0, row1); ``chunk`` rays
    per DepthNet pass.  The depth is DepthNetFunction's (the training step's), so the gradients are those of the autograd chain
    PlaceSamples -> NerfInputGrad -> Composite, without its per-sample arrays.

    ``approximate=True`` (keyword only) also accepts an "f16" NeRF handle.  The Jacobian is then the derivative carried through
    the field's 16-bit arithmetic (ops.render_rays_depthnet_tangent): the maps are the f16 one-kernel forward's, and the DepthNet
    gradients are those of the f16 field -- measured, a cosine of at least 0.9989 with autograd through a model of that field, and
    of 0.979 .. 0.99996 with the f16x3 path's on lego_synth and a fitted-scene band, as close as the f16 field itself comes
    (tests/test_gpu_render_tangent16.py).  bf16 and f32 handles are refused either way.

    ``mode="depth_only"`` (keyword only): one sample per ray at the DepthNet's depth, the training operator's DepthNet branch;
    ``n_samples`` and ``std`` are ignored, "f16x3" handles only (ops.render_rays_depthnet_tangent): rgb = sigmoid(raw rgb),
    disp = 1e10, depth = acc = 0, and only rgb carries a gradient."""
    if mode not in ("uniform", "depth_only"):
        raise ValueError(f"mode: 'uniform' or 'depth_only', got {mode!r}")
    single = mode == "depth_only"
    dtypes = ("f16x3", "f16") if approximate and not single else ("f16x3",)
    if getattr(nerf, "dtype", None) not in dtypes:
        if single:
            raise NotImplementedError(f"the depth_only differentiable renderer needs an f16x3 NeRF handle, got {getattr(nerf, 'dtype', None)}")
        if approximate:
            raise NotImplementedError("the differentiable renderer needs an f16x3 or f16 NeRF handle, got "
                                      f"{getattr(nerf, 'dtype', None)}")
        raise NotImplementedError(f"the differentiable renderer needs an f16x3 NeRF handle, got {getattr(nerf, 'dtype', None)}")
    if not single and not ops._tangent_samples_ok(int(n_samples)):
        raise NotImplementedError(f"n_samples must be a power of two in [2, 64] or a multiple of 64 up to 512, got {n_samples}")
    if (rays is None) == (camera is None):
        raise ValueError("exactly one of rays= and camera= is required")
    if int(chunk) < 1:
        raise ValueError("chunk must be >= 1")
    if rays is None:
        H, W, K, c2w, row0, row1 = camera
        rays = ops.get_rays(H, W, K, c2w, row0, row1)
    o, d, v = (_dev(t, n) for t, n in zip(rays, ("rays_o", "rays_d", "viewdirs")))
    depth_net._train_shape()          # (raises for shapes the layer-by-layer path does not cover)
    params = depthnet_params(depth_net)
    cfg = dict(depth_net=depth_net, nerf=nerf, chunk=int(chunk), n_samples=int(n_samples), std=float(std),
               white_bkgd=bool(white_bkgd), approximate=bool(approximate), mode=mode)
    rgb, disp, depth, acc = DepthNetTangentRender.apply(o, d, v, cfg, *params)
    return {"rgb": rgb, "disp": disp, "depth": depth, "acc": acc}
