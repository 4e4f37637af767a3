"""Mirror of nerf_sampling/nerf_pytorch/run_nerf_helpers.py for the hot path (HIP-backed)."""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops

img2mse = lambda x, y: torch.mean((x - y) ** 2)  # noqa: E731   run_nerf_helpers.py:9
_TEN = {}


def mse2psnr(x):
    """-10 log(x) / log(10) as run_nerf_helpers.py:10; the constant tensor is cached per device (creating it per call is
    a blocking host-to-device copy, i.e. a stream synchronisation inside every training step)."""
    ten = _TEN.get(x.device)
    if ten is None:
        ten = _TEN[x.device] = torch.tensor([10.0], device=x.device)
    return -10.0 * torch.log(x) / torch.log(ten)


to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)  # noqa: E731


class Embedder:
    """Positional encoding (run_nerf_helpers.py:15-45); ``embed`` runs the ns_posenc kernel."""

    def __init__(self, **kwargs):
        self.kwargs = kwargs
        if not (kwargs.get("include_input", True) and kwargs.get("log_sampling", True)):
            raise NotImplementedError("only include_input=True, log_sampling=True embedders are built")
        self.input_dims = kwargs["input_dims"]
        self.num_freqs = kwargs["num_freqs"]
        if kwargs["max_freq_log2"] != self.num_freqs - 1:
            raise NotImplementedError("max_freq_log2 must equal num_freqs - 1")
        self.out_dim = self.input_dims * (1 + 2 * self.num_freqs)

    def embed(self, inputs):
        return ops.posenc(inputs, self.num_freqs)

    __call__ = embed


def get_embedder(multires, i=0, input_dims=4):
    """Same signature/returns as run_nerf_helpers.py:48-63: (embed_fn, out_dim)."""
    if i == -1:
        return nn.Identity(), 3
    embedder = Embedder(include_input=True, input_dims=input_dims, max_freq_log2=multires - 1,
                        num_freqs=multires, log_sampling=True, periodic_fns=[torch.sin, torch.cos])
    return embedder, embedder.out_dim


# ---- the pack-time unit order of a production 16-bit field ---------------------------------------------------------
# The K-block-skipping render kernel (csrc/ns_nerf_mlp_ob16.hip) jumps over the MFMAs of a chunk step whose input K-block
# -- 32 hidden units x the wave's 80 samples -- is all zero bits after the ReLU.  With the units in the order they were
# trained in that never happens; with every trunk layer's units sorted by how often they fire, the rarely firing ones share
# K-blocks and those are dead for whole waves of empty space.  The order is a permutation of a layer's output units and of the
# matching input columns of its consumers: the function is unchanged (16-bit results move by the summation order inside the
# matrix cores only), and no kernel's correctness depends on it.  DESCENDING frequency: the kernel tests the LAST K-blocks of a
# layer's input and never the first, whose MFMAs carry the bias in.
UNIT_ORDER_POINTS = 32768
UNIT_ORDER_RADIUS = 2.0
UNIT_ORDER_SEED = 20240


def firing_counts(net, radius: float = UNIT_ORDER_RADIUS, points: int = UNIT_ORDER_POINTS, seed: int = UNIT_ORDER_SEED):
    """How many of `points` seeded points, uniform in the ball of `radius`, make each unit of each trunk layer positive, from the
    module's own fp32 forward (the trunk never sees directions): a list of D int64 tensors [W]."""
    gen = torch.Generator(device="cpu").manual_seed(seed)      # (explicit: a caller may have set a default device)
    v = torch.randn(points, 3, generator=gen, dtype=torch.float64, device="cpu")
    r = torch.rand(points, 1, generator=gen, dtype=torch.float64, device="cpu") ** (1.0 / 3.0) * radius
    x = (v / v.norm(dim=1, keepdim=True) * r).float()
    w0 = net.pts_linears[0].weight
    with torch.no_grad():
        x = x.to(w0.device)
        n_freqs = (net.input_ch // 3 - 1) // 2
        emb = torch.cat([x] + [f(x * 2.0 ** k) for k in range(n_freqs) for f in (torch.sin, torch.cos)], dim=1)
        h, counts = emb, []
        for i, lin in enumerate(net.pts_linears):
            h = torch.relu(torch.nn.functional.linear(h, lin.weight.float(), lin.bias.float()))
            counts.append((h > 0).sum(dim=0).to(torch.int64).cpu())
            if i in net.skips:
                h = torch.cat([emb, h], dim=1)
    return counts


def unit_orders(counts):
    """per layer: the units by descending firing count, ties by index (a permutation of range(W))"""
    return [torch.argsort(-c, stable=True) for c in counts]


def permute_units(weights, biases, orders, skips, input_ch=63):
    """The tensors ops.pack_nerf takes (pts_linears.0..D-1, feature, alpha, views, rgb), with unit orders[i][j] of trunk layer i
    moved to position j: rows and bias of layer i, and the matching input columns of pts_linears[i + 1] (behind the embedded
    point when i is a skip) or, for the last layer, of feature_linear and alpha_linear.  New tensors; the function is the same."""
    D = len(orders)
    ws, bs = [w.clone() for w in weights], [b.clone() for b in biases]
    for i, perm in enumerate(orders):
        perm = perm.to(ws[i].device)
        ws[i], bs[i] = ws[i][perm], bs[i][perm]
        for c in ([i + 1] if i + 1 < D else [D, D + 1]):
            off = input_ch if (i in skips and i + 1 < D) else 0
            cols = torch.cat([torch.arange(off, device=perm.device), off + perm])
            ws[c] = ws[c][:, cols]
    return ws, bs


class NeRF(nn.Module):
    """Weight container with the reference's state-dict keys (run_nerf_helpers.py:67-105).

    ``forward`` takes the embedded [M, 90] input like the reference and runs the fused MFMA kernel;
    ``run_network`` bypasses the embedding round trip entirely (trainers.DepthNetTrainer).
    """

    def __init__(self, D=8, W=256, input_ch=3, input_ch_views=3, output_ch=4, skips=[4], use_viewdirs=False):
        super().__init__()
        self.D, self.W = D, W
        self.input_ch, self.input_ch_views = input_ch, input_ch_views
        self.skips, self.use_viewdirs = skips, use_viewdirs
        self.pts_linears = nn.ModuleList(
            [nn.Linear(input_ch, W)]
            + [nn.Linear(W, W) if i not in self.skips else nn.Linear(W + input_ch, W) for i in range(D - 1)]
        )
        self.views_linears = nn.ModuleList([nn.Linear(input_ch_views + W, W // 2)])
        if use_viewdirs:
            self.feature_linear = nn.Linear(W, W)
            self.alpha_linear = nn.Linear(W, 1)
            self.rgb_linear = nn.Linear(W // 2, 3)
        else:
            self.output_linear = nn.Linear(W, output_ch)
        self._packed = {}

    # -- packing ---------------------------------------------------------------------------------
    def _check_supported(self):
        """The HIP kernels cover the reference's whole constructor (run_nerf_helpers.py:67-105) for W <= 256 (the packer
        zero-pads a width to the next kernel width, 128 or 256: the same arithmetic plus exact zeros): any D <= 32, any
        ``skips`` list, both heads (use_viewdirs True / False with output_linear).  Returns the active skips."""
        if self.input_ch != 63 or (self.use_viewdirs and self.input_ch_views != 27):
            raise NotImplementedError("the HIP kernel is built for multires=10 / multires_views=4 (63+27 inputs)")
        if not 2 <= self.W <= 256:
            raise NotImplementedError(f"the HIP kernels are built for 2 <= W <= 256, got {self.W}")
        return sorted({int(s_) for s_ in self.skips if 0 <= int(s_) < self.D - 1})

    @property
    def output_channels(self) -> int:
        return 4 if self.use_viewdirs else self.output_linear.out_features

    def packed(self, dtype: Optional[str] = None) -> ops.PackedWeights:
        """Device weight stream for the MFMA kernels (cached per dtype; call ``repack`` after updates)."""
        name = dtype or ops.get_compute_dtype()
        if name not in self._packed:
            skips = self._check_supported()
            mods = list(self.pts_linears) + ([self.feature_linear, self.alpha_linear, self.views_linears[0], self.rgb_linear]
                                             if self.use_viewdirs else [self.output_linear])
            dev = self.pts_linears[0].weight.device
            ws, bs = [m.weight for m in mods], [m.bias for m in mods]
            self.unit_orders = None      # the order of the most recent pack (None: that pack kept the trained order)
            if self._orders_units(name, skips):
                # once per pack (repack() drops it with the handle): calibrated on seeded points, not on any frame
                self.unit_orders = unit_orders(firing_counts(self, self.unit_order_radius))
                with torch.no_grad():
                    ws, bs = permute_units(ws, bs, self.unit_orders, skips, self.input_ch)
            self._packed[name] = ops.pack_nerf(ws, bs, self.D, self.W, skips, name,
                                               dev if dev.type == "cuda" else "cuda", use_viewdirs=self.use_viewdirs,
                                               output_ch=self.output_channels, unit_ordered=self.unit_orders is not None)
        return self._packed[name]

    unit_order = True                  # False (or NS_NO_UNIT_ORDER=1 in the environment): pack the units in their own order
    unit_order_radius = UNIT_ORDER_RADIUS
    unit_orders = None

    def _orders_units(self, name, skips) -> bool:
        """production-shaped 16-bit handles only (the ones that get the sigma-first second stream): 8 x 256, skips = [4], view
        directions, bf16 or f16; f16x3, f32 and generic shapes keep their order"""
        import os
        return (self.unit_order and os.environ.get("NS_NO_UNIT_ORDER", "0") != "1" and name in ("bf16", "f16") and self.D == 8
                and self.W == 256 and list(skips) == [4] and bool(self.use_viewdirs))

    def repack(self):
        self._packed = {}

    def __getstate__(self):
        # packed device weight streams are caches of the parameters: never pickled / deep-copied
        state = self.__dict__.copy()
        state["_packed"] = {}
        return state

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.repack()
        return r

    def forward(self, x):
        return ops.nerf_forward_embedded(self.packed(), x)


def get_rays(H, W, K, c2w):
    """rays_o, rays_d [H,W,3] (run_nerf_helpers.py:187-202)."""
    o, d, _ = ops.get_rays(H, W, K, c2w)
    return o.reshape(H, W, 3), d.reshape(H, W, 3)


def sample_pdf(bins, weights, N_samples, det=False, pytest=False):
    """Inverse-CDF sampling (run_nerf_helpers.py:250-293); random draws come from torch's generator."""
    u = None
    if pytest:
        np.random.seed(0)
        shape = list(bins.shape[:-1]) + [N_samples]
        u_np = np.broadcast_to(np.linspace(0.0, 1.0, N_samples), shape) if det else np.random.rand(*shape)
        u = torch.tensor(np.ascontiguousarray(u_np), dtype=torch.float32, device=bins.device)
    elif not det:
        u = torch.rand(list(bins.shape[:-1]) + [N_samples], device=bins.device)
    return ops.sample_pdf(bins, weights, N_samples, u)
