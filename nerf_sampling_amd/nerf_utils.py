"""Mirror of the render driver / ray-batch operators of nerf_sampling/nerf_pytorch/nerf_utils.py.

Same function names, arguments and returned keys as the reference (render_rays :614-733,
render_rays_test :736-876, sample_as_in_NeRF :497-611, render / render_test :88-255,
batchify* :45-85, create_nerf :393-494); the arithmetic runs in HIP kernels.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from . import ops, run_nerf_helpers
from .utils import sample_points_around_mean

DEBUG = False


def raw2alpha(raw, dists):
    """nerf_utils.py:27-42 -- kept for API parity (plain tensor expression, not on the hot path)."""
    return 1.0 - torch.exp(-torch.relu(raw) * dists)


def batchify(fn, chunk):
    if chunk is None:
        return fn

    def ret(inputs):
        return torch.cat([fn(inputs[i : i + chunk]) for i in range(0, inputs.shape[0], chunk)], 0)

    return ret


class _HostSink:
    """Frame-sized pinned host buffers that the per-chunk host copies of render_rays_test (the reference's four
    `.cpu()` calls per chunk, nerf_utils.py:866-870) land in directly, asynchronously, on a side stream.

    The reference serialises the GPU on every chunk (a blocking D2H of ~42 MB at 32768 rays x 64 samples) and then
    concatenates the chunks on the host (another pass over ~0.8 GB per 800x800 frame).  Here the "concatenation" is the
    buffer itself and the copies of chunk i run UNDER THE NeRF-MLP KERNEL OF CHUNK i+1: put() only queues a copy, and
    release(after=ev) starts the queued ones once `ev` -- the event the one-call renderer records right before its MLP
    kernel -- has been reached.  (Measured on MI355X: started right after a chunk the copies run beside the next chunk's
    small kernels -- DepthNet, placement -- and stretch them tenfold, while the MFMA-bound MLP kernel that follows runs
    alone; under the MLP kernel they are nearly free.  The copies go through the SDMA engines -- a kernel trace shows shader
    blits only because the profiler switches the engines off -- at ~27 GB/s beside the MLP kernel, 57 GB/s alone:
    profiles/r04f_api_path_copy_engines.log.)  The caller
    gets the same host tensors (same keys, shapes, dtypes, values).  Buffers come from torch's caching pinned allocator,
    fresh per frame, so tensors returned for one frame are never overwritten by the next (render_path keeps references
    across frames)."""

    def __init__(self, total_rows: int, device, pooled: bool = False):
        self.total, self.device, self.pooled = int(total_rows), torch.device(device), pooled
        self.stream = torch.cuda.Stream(self.device)
        self.bufs, self.keep, self.row0 = {}, [], 0
        self.pending, self.events, self.whole = [], [], []

    def _pinned(self, key, shape, dtype):
        """A pinned host buffer: fresh from torch's caching pinned allocator, or -- pooled=True, render_path's own loop,
        which knows when a frame's host tensors are dead -- one that recycle() handed back (torch's allocator took tens of
        frames to settle on 0.8 GB-per-frame requests: 35-55 ms/frame instead of 31)."""
        # device="cpu" explicitly: the experiment scripts switch torch's DEFAULT device to cuda (utils.py:143-149)
        free = _sink_pool.get((key, tuple(shape), dtype)) if self.pooled else None
        return free.pop() if free else torch.empty(tuple(shape), dtype=dtype, device="cpu", pin_memory=True)

    def recycle(self):
        """Hand this (finished, consumed) frame's pinned buffers to the pool.  Only render_path calls this: the tensors it
        got from render_test for this frame must not be read afterwards."""
        self.finish()
        for key, buf in self.bufs.items():
            _sink_pool.setdefault((key, tuple(buf.shape), buf.dtype), []).append(buf)
        for buf in self.whole:
            _sink_pool.setdefault(("__whole__", tuple(buf.shape), buf.dtype), []).append(buf)
        self.bufs, self.whole = {}, []

    def put(self, key: str, t: torch.Tensor) -> torch.Tensor:
        n = t.shape[0]
        buf = self.bufs.get(key)
        if buf is None:
            buf = self.bufs[key] = self._pinned(key, (self.total,) + tuple(t.shape[1:]), t.dtype)
        dst = buf[self.row0 : self.row0 + n]
        self.pending.append((dst, t))
        return dst

    def new_event_pair(self):
        pair = (ops.Event(), ops.Event())
        self.events.append(pair)           # alive until the frame's copies are done
        return pair

    def release(self, after=None):
        """Start every queued copy on the side stream: after the ops.Event ``after`` (already recorded on the compute
        stream by work submitted earlier), or after everything submitted to the compute stream so far."""
        if not self.pending:
            return
        if after is None:
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.device))
            self.stream.wait_event(done)
        else:
            from ._lib import check, load

            check(load().ns_stream_wait_event(ops.C.c_void_p(self.stream.cuda_stream), after.handle), "ns_stream_wait_event")
        with torch.cuda.stream(self.stream):
            for dst, t in self.pending:
                dst.copy_(t, non_blocking=True)
        self.keep.extend(t for _, t in self.pending)      # the device tensors stay alive until finish()
        self.pending.clear()

    def copy_whole(self, t: torch.Tensor) -> torch.Tensor:
        """A pinned host copy of a whole device tensor, queued on the side stream behind everything submitted to the
        compute stream so far; valid after finish()."""
        dst = self._pinned("__whole__", t.shape, t.dtype)
        self.whole.append(dst)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        self.stream.wait_event(done)
        with torch.cuda.stream(self.stream):
            dst.copy_(t, non_blocking=True)
        self.keep.append(t)
        return dst

    def advance(self, n_rows: int):
        self.row0 += int(n_rows)

    def finish(self):
        self.release()
        self.stream.synchronize()
        self.keep.clear()
        self.events.clear()


_sink_pool = {}          # (key, shape, dtype) -> pinned buffers recycled by render_path (emptied when it returns)
_held_sink = None        # render_path's pipeline: the previous frame's sink, its copies queued but not started yet -- they are
                         # released when the NEXT frame's MLP kernel starts (render_rays_test), or by finish()
# A standard-configuration frame may go through render_rays_test in ONE call when its per-sample outputs fit this many bytes
# (NS_WHOLE_FRAME_BYTES; 0 = off, the default: the reference's chunk loop).  Measured on MI355X, 800x800x64, render_path steady
# state (profiles/r04_api_path_whole_frame_vs_chunks.log): one call per frame 35.5 ms, twenty chunks 30.5 ms -- the path is bound
# by the device-to-host copies (0.82 GB per frame at ~27 GB/s beside the MLP kernel), and chunks let them start a chunk
# after the frame does instead of a frame later; the 16-21 ms of Python the chunk loop costs stay hidden under the GPU's 27.
_WHOLE_FRAME_BYTES = int(os.environ.get("NS_WHOLE_FRAME_BYTES", 0))
_pending_sinks = []      # frames whose host copies may still be in flight (only with _defer_host_sync, see _batchify)
_last_sink = None        # the sink of the most recent _batchify call (None: that call made blocking copies)


def drain_host_copies():
    """Wait for the host copies of every frame rendered with ``_defer_host_sync=True``; their host tensors are valid
    afterwards.  render_path calls this before it reads a frame's host tensors and when it is done."""
    for sink in _pending_sinks:
        sink.finish()
    _pending_sinks.clear()


def _batchify(render_fn, rays_flat, chunk, **kwargs):
    """Chunked calls + concatenation (nerf_utils.py:58-85).  Host outputs of render_rays_test land asynchronously in
    frame-sized pinned buffers (_HostSink).  By default the copies are complete when this returns, as with the
    reference's blocking `.cpu()` calls.  With ``_defer_host_sync=True`` (render_path's own loop) the tail of frame i's
    copies stays in flight under frame i+1's kernels: frame i-1 is drained here, frame i by drain_host_copies() or by
    the next frame."""
    global _last_sink, _held_sink
    all_returned = {}
    sink = None
    defer = bool(kwargs.pop("_defer_host_sync", False))
    if render_fn is render_rays_test and rays_flat.is_cuda and not kwargs.get("_blocking_host_copies", False):
        sink = kwargs["_host_sink"] = _HostSink(rays_flat.shape[0], rays_flat.device, pooled=defer)
        # Optionally (_WHOLE_FRAME_BYTES > 0) the standard configuration renders a frame as ONE render_rays_test call: the
        # reference's chunk loop (:58-85) bounds its memory, not its results -- rays are independent, the concatenated chunks
        # ARE the whole-frame tensors.  One call = three launches and four host copies per frame; bigger frames fall back to
        # chunks of the largest size under the bound.  Off by default: see _WHOLE_FRAME_BYTES.
        tr = kwargs.get("trainer")
        net = kwargs.get("network_fine") if kwargs.get("network_fine") is not None else kwargs.get("network_fn")
        if (tr is not None and rays_flat.shape[-1] > 8 and not (tr.compare_nerf or tr.use_nerf_max_pts or tr.use_full_nerf)
                and _one_call_eligible(kwargs.get("depth_network"), net, kwargs.get("network_query_fn"), tr, True)):
            per_ray = 20 * (1 if tr.sampling_mode == "depth_only" else int(tr.n_depth_samples))
            chunk = max(chunk, min(rays_flat.shape[0], _WHOLE_FRAME_BYTES // per_ray))
    # A frame is rendered for its values: render_rays_test's maps carry a graph back to a trainable DepthNet (call it on a ray
    # batch for gradients), the frame's chunks are detached so that each chunk's graph is freed with the chunk.
    frame = render_fn is render_rays_test
    for i in range(0, rays_flat.shape[0], chunk):
        returned = render_fn(rays_flat[i : i + chunk], **kwargs)
        for key in returned:
            all_returned.setdefault(key, []).append(returned[key].detach() if frame else returned[key])
        if sink is not None:
            sink.advance(min(chunk, rays_flat.shape[0] - i))
    _last_sink = sink if defer else None
    if sink is not None:
        if defer:
            # render_path's pipeline: this frame's (last chunk's) copies wait for the NEXT frame's MLP kernel -- beside the
            # next frame's small kernels (rays, DepthNet) the blit kernels that move them stretch those tenfold -- or for
            # finish(), whichever comes first
            if _held_sink is not None and _held_sink is not sink:
                _held_sink.release()
            _held_sink = sink
            drain_host_copies()          # the frame before the previous one: long finished by now
            _pending_sinks.append(sink)
        else:
            sink.release()               # the last chunk's copies
            sink.finish()
    return {key: (sink.bufs[key] if sink is not None and key in sink.bufs else torch.cat(all_returned[key], 0))
            for key in all_returned}


def batchify_rays(rays_flat, chunk=1024 * 32, **kwargs):
    return _batchify(render_rays, rays_flat, chunk, **kwargs)


def batchify_rays_test(rays_flat, chunk=1024 * 32, **kwargs):
    return _batchify(render_rays_test, rays_flat, chunk, **kwargs)


def prepare_rays(c2w, c2w_staticcam, use_viewdirs, ndc, H, W, K, near, far, rays):
    """rays [R,11], rays_o, rays_d, shape -- nerf_utils.py:156-188 (ndc=False only).  ``c2w_staticcam`` (:172-176, "visualize
    effect of viewdirs"): the view directions come from ``c2w`` (or ``rays``), origins and directions from the static
    camera."""
    if ndc:
        raise NotImplementedError("NDC rays (LLFF forward-facing scenes) are out of scope (SURVEY.md section 2)")
    if c2w is not None and c2w_staticcam is None:
        rays_o, rays_d, viewdirs, batch = ops.get_rays(H, W, K, c2w, near=near, far=far, want_batch=True)
        sh = (H, W, 3)
        if not use_viewdirs:
            batch = batch[:, :8].contiguous()
        return batch, rays_o, rays_d, sh
    viewdirs = None
    if c2w is not None:
        rays_o, rays_d, viewdirs = ops.get_rays(H, W, K, c2w)          # viewdirs = rays_d / |rays_d|, [H*W, 3]
        sh = (H, W, 3)
    else:
        rays_o, rays_d = rays
        sh = rays_d.shape
        if use_viewdirs:
            viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
            viewdirs = torch.reshape(viewdirs, [-1, 3]).float()
    if use_viewdirs and c2w_staticcam is not None:
        rays_o, rays_d, _ = ops.get_rays(H, W, K, c2w_staticcam)
        sh = (H, W, 3)
    rays_o = torch.reshape(rays_o, [-1, 3]).float()
    rays_d = torch.reshape(rays_d, [-1, 3]).float()
    near_t, far_t = near * torch.ones_like(rays_d[..., :1]), far * torch.ones_like(rays_d[..., :1])
    batch = torch.cat([rays_o, rays_d, near_t, far_t], -1)
    if use_viewdirs:
        batch = torch.cat([batch, viewdirs], -1)
    return batch, rays_o, rays_d, sh


def _render(batch_fn, H, W, K, chunk, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam, **kwargs):
    rays, rays_o, rays_d, sh = prepare_rays(c2w=c2w, c2w_staticcam=c2w_staticcam, use_viewdirs=use_viewdirs,
                                            ndc=ndc, H=H, W=W, K=K, near=near, far=far, rays=rays)
    if batch_fn is batchify_rays_test or kwargs.get("fused_step", False):
        # internal: the scalar bounds every row of the batch carries, for the one-call vanilla pass of render_rays_test and of
        # render_rays under fused_step (which then need not read the batch's near / far columns back from the device)
        kwargs["_near_far"] = (float(near), float(far))
    all_returned = batch_fn(rays, chunk, **kwargs)
    for key in all_returned:
        all_returned[key] = torch.reshape(all_returned[key], list(sh[:-1]) + list(all_returned[key].shape[1:]))
    key_extract = ["depth_net_rgb_map", "depth_net_disp_map"]
    ret_list = [all_returned[key] for key in key_extract]
    ret_dict = {key: all_returned[key] for key in all_returned if key not in key_extract}
    ret_dict["rays_o"], ret_dict["rays_d"] = rays_o, rays_d
    return ret_list + [ret_dict]


def render(H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0.0, far=1.0, use_viewdirs=False,
           c2w_staticcam=None, **kwargs):
    """[rgb, disp, extras] through render_rays (nerf_utils.py:88-153)."""
    return _render(batchify_rays, H, W, K, chunk, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam, **kwargs)


def render_test(H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0.0, far=1.0, use_viewdirs=False,
                c2w_staticcam=None, **kwargs):
    """[rgb, disp, extras] through render_rays_test (nerf_utils.py:191-255)."""
    return _render(batchify_rays_test, H, W, K, chunk, rays, c2w, ndc, near, far, use_viewdirs, c2w_staticcam,
                   **kwargs)


def render_path(render_poses, hwf, K, chunk, render_kwargs, step, wandb_log=False, save_scene_data=False,
                gt_imgs=None, savedir=None, render_factor=0):
    """Per-image loop with PSNR / PNG / psnr.txt / scene_data.pt outputs in the reference's format
    (nerf_utils.py:258-360).  wandb logging is out of scope; PNGs are written with PIL."""
    import numpy as np

    H, W, focal = hwf
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor
    if wandb_log:
        raise NotImplementedError("wandb logging is out of scope")
    rgbs, disps, all_pts, all_weights = [], [], [], []
    total_psnr, total_mse, psnr_info = 0, 0, None
    n_render_poses = render_poses.shape[0]

    def consume(i, rgb, disp, extras, sink):
        """Everything the reference does with a finished frame (:303-355): host arrays, PSNR, PNG, psnr.txt, scene data."""
        nonlocal total_psnr, total_mse, psnr_info
        if sink is not None:
            sink.finish()                                # this frame's host copies (rgb / disp included) are complete
            rgbs.append(np.array(rgb.numpy()))           # pageable copies: the pinned buffers go back to the cache
            disps.append(np.array(disp.numpy()))
        else:
            rgbs.append(rgb.cpu().numpy())
            disps.append(disp.cpu().numpy())
        if gt_imgs is not None and render_factor == 0:
            psnr = -10.0 * np.log10(np.mean(np.square(rgbs[-1] - np.asarray(gt_imgs[i]))))
            psnr_info = f"{i:03d}.png, PSNR: {psnr}"
            if render_kwargs["trainer"].compare_nerf and extras.get("max_z_vals") is not None:
                mse = torch.nn.functional.mse_loss(extras["max_z_vals"], extras["depth_net_z_vals"])
                total_mse += mse
                psnr_info += f", MSE: {mse}"
            total_psnr += psnr
        if savedir is not None:
            from PIL import Image

            Image.fromarray(run_nerf_helpers.to8b(rgbs[-1])).save(os.path.join(savedir, "{:03d}.png".format(i)))
            if psnr_info is not None:
                f = os.path.join(savedir, "psnr.txt")
                with open(f, "a") as file:
                    file.write(f"{psnr_info}\n")
                if i == n_render_poses - 1:
                    to_write = f"Avg of {n_render_poses} images:\nPSNR: {total_psnr/n_render_poses}\n"
                    if total_mse > 0:
                        to_write += f"MSE: {total_mse/n_render_poses}"
                    with open(f, "a") as file:
                        file.write(to_write)
            if save_scene_data:
                # pageable copies: the frame's pinned buffers go back to the allocator's cache instead of piling up
                # (0.7 GB of page-locked memory per 800x800 frame otherwise)
                for dst, key in ((all_pts, "depth_net_pts"), (all_weights, "depth_net_weights")):
                    flat = torch.flatten(extras[key], end_dim=2)
                    dst.append(torch.empty(flat.shape, dtype=flat.dtype, device="cpu", pin_memory=False).copy_(flat))
        if sink is not None:
            sink.recycle()                               # nothing of this frame's host tensors is read from here on

    # Software pipeline (SURVEY 8f-1 "asynchronous D2H of frames"): frame i+1 is submitted to the GPU BEFORE frame i is
    # consumed on the host, so the PNG / PSNR work and the tail of frame i's host copies run under frame i+1's kernels.
    # rgb / disp go to the host through the frame's copy stream too: a `.cpu()` on the compute stream would wait for
    # frame i+1.  Output files, their order and their contents are the reference's.
    prev = None
    for i, c2w in enumerate(render_poses):
        rgb, disp, extras = render_test(H, W, K, chunk=chunk, c2w=c2w[:3, :4], _defer_host_sync=True, **render_kwargs)
        sink = _last_sink if rgb.is_cuda else None
        if sink is not None:
            # rgb is a device tensor (nerf_utils.py:867 keeps it there); disp already IS this frame's pinned sink buffer
            # (depth_net_disp_map, filled chunk by chunk on the sink's stream): a host-to-host copy_ of it would run at once,
            # ahead of the queued device-to-host copies, and snapshot stale data.  consume() reads it after sink.finish().
            rgb = sink.copy_whole(rgb)
            if disp.is_cuda:
                disp = sink.copy_whole(disp)
        if prev is not None:
            consume(*prev)
        prev = (i, rgb, disp, extras, sink)
    if prev is not None:
        consume(*prev)
    global _held_sink
    _held_sink = None                                    # (finished by consume(): nothing is left in flight)
    _sink_pool.clear()                                   # the pinned buffers go back to torch's cache
    drain_host_copies()
    if save_scene_data and savedir is not None:
        torch.save({"all_pts": torch.cat(all_pts), "all_weights": torch.cat(all_weights)},
                   os.path.join(savedir, "scene_data.pt"))
    return np.stack(rgbs, 0), np.stack(disps, 0), total_psnr / n_render_poses


# ---- held-out views scored on the device (not in the reference: its Trainer.log / render_path score on the host) ---------
def format_psnr_txt(psnrs, avg) -> str:
    """psnr.txt of a set of views in render_path's format (nerf_utils.py:318-336): one "NNN.png, PSNR: x" line per view, then
    the average."""
    lines = [f"{i:03d}.png, PSNR: {p}\n" for i, p in enumerate(psnrs)]
    return "".join(lines) + f"Avg of {len(lines)} images:\nPSNR: {avg}\n"


def _write_psnr_txt(savedir, psnrs, avg):
    os.makedirs(savedir, exist_ok=True)
    with open(os.path.join(savedir, "psnr.txt"), "a") as file:      # appended to, as render_path does
        file.write(format_psnr_txt(psnrs, avg))


def format_ssim_txt(ssims, avg) -> str:
    """ssim.txt of a set of views, psnr.txt's layout: one "NNN.png, SSIM: x" line per view, then the average"""
    lines = [f"{i:03d}.png, SSIM: {s}\n" for i, s in enumerate(ssims)]
    return "".join(lines) + f"Avg of {len(lines)} images:\nSSIM: {avg}\n"


def _write_ssim_txt(savedir, ssims, avg):
    os.makedirs(savedir, exist_ok=True)
    with open(os.path.join(savedir, "ssim.txt"), "a") as file:
        file.write(format_ssim_txt(ssims, avg))


def format_depth_txt(sample_mses, avg_sample_mse, mean_mses, avg_mean_mse) -> str:
    """depth.txt of a set of views, psnr.txt's layout: one "NNN.png, MSE: x, mean MSE: y" line per view -- x the reference's
    compare_nerf ``MSE:`` (nerf_utils.py:311-317), y the DepthNet's own depth against the field's -- then the averages"""
    lines = [f"{i:03d}.png, MSE: {s}, mean MSE: {m}\n" for i, (s, m) in enumerate(zip(sample_mses, mean_mses))]
    return "".join(lines) + f"Avg of {len(lines)} images:\nMSE: {avg_sample_mse}\nmean MSE: {avg_mean_mse}\n"


def _write_depth_txt(savedir, sample_mses, avg_sample_mse, mean_mses, avg_mean_mse):
    os.makedirs(savedir, exist_ok=True)
    with open(os.path.join(savedir, "depth.txt"), "a") as file:
        file.write(format_depth_txt(sample_mses, avg_sample_mse, mean_mses, avg_mean_mse))


class FrameWriter:
    """The frames of a device evaluation as ``{k:03d}.png`` under ``savedir``, the files render_path(savedir=...) writes
    (nerf_utils.py:322-325), without a float frame on the host and without the PNG encoder on the rendering thread.

    The writer owns ``n_buffers`` slots, allocated once: a uint8 [H,W,channels] device tensor and its pinned host twin each.
    ``put(k, rgb, alpha=None)`` takes a free slot, quantises the frame into its device tensor on the CURRENT stream
    (ops.frame_to8b: to8b's bits) and records an event; the writer's own copy stream waits for that event, copies the slot to
    its twin (non-blocking, a quarter of the fp32 frame's bytes) and records a second event; (k, slot) goes to a queue.
    ``workers`` plain threads (at most MAX_WORKERS, a number the caller chooses: never the machine's CPU count) take jobs
    from it: wait for the slot's copy event, ``Image.fromarray(slot).save(...)`` -- render_path's call, so equal pixels at an
    equal ``compress_level`` (None: PIL's default, as render_path) give equal files -- and hand the slot back.  A slot is
    therefore reused only after its copy AND its file are done.  put() blocks only while every slot is in flight, and then on
    the return of a slot -- a worker's wait on that slot's copy event; the compute stream is never synchronised and nothing but
    the frames is read back.  The writer keeps no reference to ``rgb``: it is read by a launch on the stream that produced it.

    ``close()`` drains the queue, joins the workers, releases the buffers and raises the first exception a worker met (the
    other frames are still written); it may be called twice, and a ``with`` block calls it -- quietly when the block itself
    raised, so that the block's exception is the one that surfaces.

    ``channels=1`` is a writer of per-ray maps: a slot is [H,W] uint8, saved as a mode-L PNG, and frames come in through
    ``put_map(k, map, denom=None)`` -- ops.map_to8b, the map divided by a float that lies in device memory -- instead of
    ``put``; from the slot on the pipeline is the same."""

    MAX_WORKERS = 8

    def __init__(self, savedir, H, W, channels=3, n_buffers=4, workers=4, compress_level=None, device=None):
        import queue
        import threading

        H, W, channels, n_buffers, workers = int(H), int(W), int(channels), int(n_buffers), int(workers)
        if savedir is None:
            raise ValueError("FrameWriter: a directory to write into")
        if H < 1 or W < 1 or channels not in (1, 3, 4):
            raise ValueError(f"FrameWriter: a frame of at least 1 x 1 pixels with 1, 3 or 4 channels, got {H} x {W} x {channels}")
        if n_buffers < 1 or workers < 1:
            raise ValueError("FrameWriter: at least one buffer and one worker")
        if compress_level is not None and not 0 <= int(compress_level) <= 9:
            raise ValueError("FrameWriter: compress_level is None (PIL's default) or 0 .. 9")
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError(f"a FrameWriter's frames live on the GPU (got {device}); this path has no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        from PIL import Image  # noqa: F401  (a missing encoder fails here, not in a worker)

        os.makedirs(savedir, exist_ok=True)
        self.savedir, self.H, self.W, self.channels = savedir, H, W, channels
        self.compress_level = None if compress_level is None else int(compress_level)
        self.device, self.n_buffers, self.workers = device, n_buffers, min(workers, self.MAX_WORKERS)
        slots = (n_buffers, H, W) if channels == 1 else (n_buffers, H, W, channels)      # [H,W] is PIL's mode L
        self._dev = torch.empty(slots, dtype=torch.uint8, device=device)
        # device="cpu" explicitly: the experiment scripts switch torch's default device to cuda
        self._host = torch.empty(slots, dtype=torch.uint8, device="cpu", pin_memory=True)
        self._quantised = [torch.cuda.Event() for _ in range(n_buffers)]
        self._copied = [torch.cuda.Event() for _ in range(n_buffers)]
        self._stream = torch.cuda.Stream(device)
        self._free, self._jobs = queue.Queue(), queue.Queue()
        for s in range(n_buffers):
            self._free.put(s)
        self._error, self._closed, self.n_written = None, False, 0
        self._lock = threading.Lock()
        self._threads = [threading.Thread(target=self._work, name=f"frame-writer-{i}", daemon=True)
                         for i in range(self.workers)]
        for t in self._threads:
            t.start()

    def _work(self):
        from PIL import Image

        while True:
            job = self._jobs.get()
            if job is None:
                return
            k, s = job
            try:
                self._copied[s].synchronize()
                view = self._host[s].numpy()
                path = os.path.join(self.savedir, "{:03d}.png".format(k))
                if self.compress_level is None:
                    Image.fromarray(view).save(path)
                else:
                    Image.fromarray(view).save(path, compress_level=self.compress_level)
                with self._lock:
                    self.n_written += 1
            except BaseException as e:  # noqa: BLE001  (kept for close(); the worker goes on, so no slot is ever lost)
                with self._lock:
                    if self._error is None:
                        self._error = e
            finally:
                self._free.put(s)

    def put(self, k, rgb, alpha=None):
        """Queue frame ``k``: ``rgb`` fp32 [H*W,3] on the writer's device (contiguous, or the [:, :3] view of a [H*W,4] shard),
        ``alpha`` fp32 [H*W] for the fourth channel of a 4-channel writer (None: opaque)."""
        k = self._check_put("put", k)
        if self.channels == 1:
            raise ValueError("FrameWriter.put: a one-channel writer takes maps (put_map)")
        if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.device == self.device
                and tuple(rgb.shape) == (self.H * self.W, 3)):
            raise ValueError(f"FrameWriter.put: rgb is a float32 tensor of shape ({self.H * self.W}, 3) on {self.device}")
        self._submit(k, lambda slot: ops.frame_to8b(rgb, alpha=alpha, out=slot, channels=self.channels))

    def put_map(self, k, map, denom=None):
        """Queue frame ``k`` of a one-channel writer: ``map`` fp32 [H*W] on the writer's device (contiguous, or the [:, 3] view of
        a [H*W,4] shard), quantised as ops.map_to8b does -- divided by ``denom``, one float32 element in device memory that the
        kernel reads (None: no division)."""
        k = self._check_put("put_map", k)
        if self.channels != 1:
            raise ValueError(f"FrameWriter.put_map: a {self.channels}-channel writer takes rgb frames (put)")
        if not (isinstance(map, torch.Tensor) and map.is_cuda and map.device == self.device
                and tuple(map.shape) == (self.H * self.W,)):
            raise ValueError(f"FrameWriter.put_map: map is a float32 tensor of shape ({self.H * self.W},) on {self.device}")
        self._submit(k, lambda slot: ops.map_to8b(map, denom=denom, out=slot))

    def _check_put(self, who, k):
        if self._closed:
            raise RuntimeError(f"FrameWriter.{who} after close()")
        k = int(k)
        if k < 0:
            raise ValueError(f"FrameWriter.{who}: a frame number >= 0")
        return k

    def _submit(self, k, quantise):
        """a free slot, ``quantise(slot's device tensor)`` on the current stream, the copy on the writer's, the job to the workers"""
        s = self._free.get()                                   # blocks only while every slot is in flight
        queued = False
        try:
            quantise(self._dev[s])
            compute = torch.cuda.current_stream(self.device)
            self._quantised[s].record(compute)
            self._stream.wait_event(self._quantised[s])
            with torch.cuda.stream(self._stream):
                self._host[s].copy_(self._dev[s], non_blocking=True)
            self._copied[s].record(self._stream)
            self._jobs.put((k, s))
            queued = True
        finally:
            if not queued:                                     # refused arguments, or a failed launch: the slot goes back once
                self._stream.synchronize()                     # whatever of it reached the copy stream is over
                self._free.put(s)

    def close(self, reraise=True):
        if not self._closed:
            self._closed = True
            for _ in self._threads:
                self._jobs.put(None)                           # behind every queued frame: the queue drains first
            for t in self._threads:
                t.join()
            self._stream.synchronize()
            self._threads = []
            self._dev = self._host = None
            self._quantised = self._copied = None
        error, self._error = self._error, None
        if error is not None and reraise:
            raise error

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close(reraise=exc_type is None)
        return False


def _frame_writer(frames, savedir, H, W, device):
    """the FrameWriter of ``frames`` (True, or a dict of FrameWriter's keyword arguments: n_buffers, workers, compress_level),
    or a context that does nothing when ``frames`` is off"""
    import contextlib

    if not frames:
        return contextlib.nullcontext()
    return FrameWriter(savedir, H, W, device=device, **(frames if isinstance(frames, dict) else {}))


def _check_frames(frames, savedir, who):
    if frames and savedir is None:
        raise ValueError(f"{who}(frames=...) writes the frames as PNGs under savedir: savedir is required")
    if isinstance(frames, dict) and not set(frames) <= {"n_buffers", "workers", "compress_level"}:
        raise ValueError(f"{who}: frames is True or a dict of n_buffers / workers / compress_level")


def score_views(dataset, image_ids, poses, render_frame, savedir=None, return_frames=False, ssim=False, depth=False,
                field_depths=None, return_depths=False, frames=False):
    """The loop of evaluate_views over any whole-frame renderer: ``render_frame(c2w [3,4], workspace)`` returns the view's rgb
    [H*W,3] on the device (or the [:, :3] view of a [H*W,4] shard), which is scored against image ``image_ids[k]`` into slot
    k of one float64 device array (DeviceRayDataset.image_sqerr).  The workspace is this call's own, and the sums are read back
    once, after the last frame.  -> (psnr per view [n] float64, their mean[, the frames]).  ``ssim``: every frame is also scored
    by DeviceRayDataset.image_ssim into slot k of a second row of that array (still one read-back), ``savedir`` also gets
    ssim.txt -> (psnr per view, their mean, ssim per view [n] float64, their mean[, the frames]).

    ``depth``: ``render_frame`` returns (rgb, z [R,N], mean [R] or [R,1], field_depth) instead -- the samples the frame was
    composited from, the DepthNet's own depth of the same rays, and a function without arguments that renders the field's
    max-weight depth max_z [R,1] of those rays.  ops.depth_sqerr scores z and mean against max_z into slot k of two further
    rows of the array (still one read-back): sample_mse = mean (max_z - z_k)^2 over all placed samples, the reference's
    compare_nerf ``MSE:`` (nerf_utils.py:311-317), and mean_mse = mean (max_z - mean)^2, the training's depth_net_loss on
    held-out rays.  ``field_depths``: max_z of every view from an earlier call (``return_depths``); ``field_depth`` is then
    not called.  ``savedir`` also gets depth.txt.  The result grows in this order:
    (psnrs, avg[, ssims, avg_ssim][, sample_mses, avg_sample_mse, mean_mses, avg_mean_mse][, frames][, depths]) -- ``depths``
    (``return_depths``): per view (z, mean, max_z) as device tensors.

    ``frames`` (needs ``savedir``; True, or a dict of FrameWriter's n_buffers / workers / compress_level): every view's rgb,
    after it is scored, also goes through a FrameWriter -- ``{k:03d}.png`` beside psnr.txt, render_path's files, quantised on the
    device and encoded by the writer's threads while the next view renders.  The writer only reads ``rgb`` and is closed before
    the sums are read back: the scores, their text files and ``return_frames`` are those of frames=False."""
    import numpy as np

    _check_frames(frames, savedir, "score_views")
    ids = [int(i) for i in np.asarray(image_ids).reshape(-1)]
    if len(ids) == 0 or len(ids) != len(poses):
        raise ValueError(f"{len(ids)} image ids for {len(poses)} poses (at least one view)")
    if not depth and (field_depths is not None or return_depths):
        raise ValueError("field_depths / return_depths belong to the depth report: depth=True")
    if field_depths is not None and len(field_depths) != len(ids):
        raise ValueError(f"{len(field_depths)} field depths for {len(ids)} views")
    workspace = ops.RenderWorkspace()
    rows = 1 + int(bool(ssim)) + 2 * int(bool(depth))
    sums = torch.empty((rows, len(ids)) if rows > 1 else (len(ids),), dtype=torch.float64, device=dataset.device)
    sq_sums = sums[0] if rows > 1 else sums
    ssim_sums = sums[1] if ssim else None
    sample_sums, mean_sums = (sums[rows - 2], sums[rows - 1]) if depth else (None, None)
    ssim_ws = (torch.empty((dataset.ssim_workspace_bytes(),), dtype=torch.uint8, device=dataset.device) if ssim else None)
    depth_ws, n_placed = None, 0
    kept_frames, depths = [], []
    with torch.no_grad(), _frame_writer(frames, savedir, dataset.H, dataset.W, dataset.device) as writer:
        for k, (img, c2w) in enumerate(zip(ids, poses)):
            rgb = render_frame(c2w[:3, :4], workspace)
            if depth:
                rgb, z, mean, field_depth = rgb
            dataset.image_sqerr(img, rgb, out=sq_sums, slot=k)
            if ssim:
                dataset.image_ssim(img, rgb, out=ssim_sums, slot=k, workspace=ssim_ws)
            if depth:
                max_z = field_depths[k] if field_depths is not None else field_depth()
                if depth_ws is None:                                           # every view has the same R and N
                    n_placed = z.numel()
                    depth_ws = torch.empty((ops.depth_sqerr_workspace_bytes(z.shape[0], z.numel() // z.shape[0]),),
                                           dtype=torch.uint8, device=dataset.device)
                ops.depth_sqerr(z, max_z, out=sample_sums, slot=k, workspace=depth_ws)
                ops.depth_sqerr(mean, max_z, out=mean_sums, slot=k, workspace=depth_ws)
                if return_depths:
                    depths.append((z, mean, max_z))
            if writer is not None:
                writer.put(k, rgb)
            if return_frames:
                kept_frames.append(rgb)
    sums = sums.cpu().numpy()                                                 # the one device-to-host copy
    psnrs = dataset.psnr_from_sqerr(sums[0] if rows > 1 else sums, 3 * dataset.H * dataset.W)
    avg = float(np.mean(psnrs))                                               # the mean of the dB values, as the reference's
    if savedir is not None:
        _write_psnr_txt(savedir, psnrs, avg)
    out = (psnrs, avg)
    if ssim:
        ssims = dataset.ssim_from_sum(sums[1], dataset.H, dataset.W)
        avg_ssim = float(np.mean(ssims))
        if savedir is not None:
            _write_ssim_txt(savedir, ssims, avg_ssim)
        out += (ssims, avg_ssim)
    if depth:
        sample_mses = ops.mse_from_sqerr(sums[rows - 2], n_placed)
        mean_mses = ops.mse_from_sqerr(sums[rows - 1], dataset.H * dataset.W)
        avg_sample, avg_mean = float(np.mean(sample_mses)), float(np.mean(mean_mses))
        if savedir is not None:
            _write_depth_txt(savedir, sample_mses, avg_sample, mean_mses, avg_mean)
        out += (sample_mses, avg_sample, mean_mses, avg_mean)
    if return_frames:
        out += (kept_frames,)
    return out + (depths,) if return_depths else out


def hierarchical_frame_renderer(network_fn, network_fine, H, W, K, N_samples, N_importance, lindisp, white_bkgd, near, far,
                                perturb=0.0, device="cuda", with_disp=False):
    """``render_frame`` of score_views through ops.render_rays_hierarchical: the vanilla coarse + fine pass of a whole view from
    its camera, one call, no per-sample outputs.  The random draws of ``perturb`` > 0 come from a generator of this renderer's
    own, in _vanilla_one_call's order.  ``with_disp``: ``render_frame`` returns (rgb, disp [H*W]) -- the same call's second
    output, which it writes anyway."""
    gen = None

    def draw(n):
        nonlocal gen
        if gen is None:
            gen = torch.Generator(device=device)
            gen.manual_seed(0)
        return torch.rand([H * W, n], device=device, generator=gen)

    def render_frame(c2w, workspace):
        t_rand = draw(int(N_samples)) if perturb > 0.0 else None
        u = draw(int(N_importance)) if perturb != 0.0 and int(N_importance) > 0 else None
        fine = network_fine.packed() if (network_fine is not None and int(N_importance) > 0) else None
        out = ops.render_rays_hierarchical(network_fn.packed(), fine, camera=(H, W, K, c2w, 0, H), n_coarse=int(N_samples),
                                           n_importance=int(N_importance), lindisp=bool(lindisp), white_bkgd=bool(white_bkgd),
                                           near=float(near), far=float(far), t_rand=t_rand, u=u, extras=False, device=device,
                                           workspace=workspace)
        return (out["rgb"], out["disp"]) if with_disp else out["rgb"]

    return render_frame


def _dataset_targets_host(dataset, image_ids):
    """the ground truth of the named views as host arrays [n,H,W,3], blended as the dataset's kernels blend it"""
    import numpy as np

    img = dataset.images[torch.as_tensor(np.asarray(image_ids, dtype=np.int64), device=dataset.device)].cpu().numpy()
    if dataset.C == 4 and dataset.white_bkgd:
        a = img[..., 3:]
        return img[..., :3] * a + (np.float32(1.0) - a)
    return img[..., :3]


_evaluate_fallback_warned = False


def _depth_frame_renderer(kw, trainer, net, H, W, K, dev):
    """``render_frame`` of score_views(depth=True): the view's rays are generated once and feed the DepthNet one-call render
    (evaluate_views' own, plus the z extra), ops.depthnet_forward on the handle that render used, and -- when asked -- the
    field's max-weight depth through ops.render_rays_hierarchical with the trainer's N_samples / N_importance / lindisp /
    bounds, in a workspace of its own.  The draws of gaussian placement and of ``perturb`` > 0 come from generators of the
    evaluation's own."""
    dn = kw["depth_network"]
    coarse, fine = kw["network_fn"], kw.get("network_fine")
    n_coarse, n_importance, perturb = int(kw["N_samples"]), int(trainer.N_importance), float(kw.get("perturb", 0.0))
    hier_ws = ops.RenderWorkspace()
    gens = {}

    def generator(name):
        if name not in gens:
            gens[name] = torch.Generator(device=dev)
            gens[name].manual_seed(0)
        return gens[name]

    def render_frame(c2w, workspace):
        rays = ops.get_rays(H, W, K, c2w, device=dev)
        noise = None
        if trainer.sampling_mode == "gaussian" and int(trainer.n_depth_samples) > 1:
            noise = torch.randn(H * W, int(trainer.n_depth_samples) - 1, device=dev, generator=generator("placement"))
        out = _depthnet_one_call(dn, net, trainer, rays=rays, extras=("z",), device=dev, noise=noise, workspace=workspace)
        dn_w = ops.psnr_guard_handles(dn, net, mode=trainer.sampling_mode, n_samples=trainer.n_depth_samples)[0]
        mean = ops.depthnet_forward(dn_w, rays[0], rays[1], dn.near, dn.far, float(dn.sphere_radius.reshape(-1)[0]))

        def field_depth():
            # the chain's draws, in _vanilla_one_call's order
            t_rand = torch.rand([H * W, n_coarse], device=dev, generator=generator("field")) if perturb > 0.0 else None
            u = torch.rand([H * W, n_importance], device=dev, generator=generator("field")) if perturb != 0.0 else None
            return ops.render_rays_hierarchical(coarse.packed(), fine.packed() if fine is not None else None, rays=rays,
                                                n_coarse=n_coarse, n_importance=n_importance,
                                                lindisp=bool(kw.get("lindisp", False)), white_bkgd=bool(kw["white_bkgd"]),
                                                near=float(kw["near"]), far=float(kw["far"]), t_rand=t_rand, u=u, extras=False,
                                                device=dev, max_sample=True, workspace=hier_ws)["max_z"]

        return out["rgb"], out["z"], mean, field_depth

    return render_frame


def _one_call_frame_renderer(kw, H, W, K, dev, with_disp=False):
    """``render_frame(c2w, workspace)`` -> rgb [H*W,3] of score_views / write_views for the configuration ``kw`` (a trainer's
    render_kwargs): ops.render_rays_hierarchical under trainer.use_full_nerf, otherwise ops.render_rays_depthnet with the
    choices of render_rays_test's one-call branch; None when the configuration is neither's.  ``with_disp`` (write_video):
    ``render_frame`` returns (rgb, disp [H*W]) -- the disparity map every one-call render writes beside its rgb
    (ops._rgb_disp_outputs), handed back instead of dropped: no further render and no copy."""
    trainer = kw["trainer"]
    net = kw.get("network_fine") if kw.get("network_fine") is not None else kw.get("network_fn")
    with torch.no_grad():
        basics = bool(kw.get("use_viewdirs", False)) and not kw.get("ndc", True)
        if trainer.use_full_nerf:
            eligible = basics and _hier_one_call_eligible(kw["network_fn"], kw.get("network_fine"), kw["network_query_fn"],
                                                          trainer, True, kw["N_samples"], kw.get("raw_noise_std", 0.0), False)
        else:
            eligible = basics and _one_call_eligible(kw.get("depth_network"), net, kw["network_query_fn"], trainer, True)
    if not eligible:
        return None
    if trainer.use_full_nerf:
        return hierarchical_frame_renderer(kw["network_fn"], kw.get("network_fine"), H, W, K, kw["N_samples"],
                                           trainer.N_importance, kw.get("lindisp", False), kw["white_bkgd"],
                                           kw["near"], kw["far"], perturb=float(kw.get("perturb", 0.0)), device=dev,
                                           with_disp=with_disp)
    dn = kw["depth_network"]
    gen = None

    def render_frame(c2w, workspace):
        nonlocal gen
        noise = None
        if trainer.sampling_mode == "gaussian" and int(trainer.n_depth_samples) > 1:
            # the draws come from a generator of the evaluation's own: the global one belongs to the training step
            if gen is None:
                gen = torch.Generator(device=dev)
                gen.manual_seed(0)
            noise = torch.randn(H * W, int(trainer.n_depth_samples) - 1, device=dev, generator=gen)
        out = _depthnet_one_call(dn, net, trainer, camera=(H, W, K, c2w, 0, H), extras=False, device=dev, noise=noise,
                                 workspace=workspace)
        return (out["rgb"], out["disp"]) if with_disp else out["rgb"]

    return render_frame


def _warn_render_path_fallback(who):
    global _evaluate_fallback_warned
    if not _evaluate_fallback_warned:
        import warnings

        warnings.warn(f"{who}: this configuration is not one of the one-call renderers'; the views go through render_path")
        _evaluate_fallback_warned = True


def evaluate_views(dataset, image_ids, poses, hwf, K, render_kwargs, savedir=None, return_frames=False, ssim=False,
                   depth=False, field_depths=None, return_depths=False, frames=False):
    """The device counterpart of render_path(gt_imgs=...): the PSNR of view ``poses[k]`` against image ``image_ids[k]`` of
    ``dataset`` (a ray_batches.DeviceRayDataset, whose images are already on the device), nothing per pixel leaving it.  Every
    view is rendered from its camera in ONE call without per-sample outputs -- ops.render_rays_depthnet with the choices of
    render_rays_test's one-call branch, or ops.render_rays_hierarchical under trainer.use_full_nerf -- and scored by
    ns_image_sqerr (score_views).  Returns (psnr per view as a float64 array, their mean[, the rgb frames as device tensors with
    ``return_frames``]); with ``savedir``, psnr.txt in render_path's format and no PNG (``frames`` below adds them).  A
    configuration the one-call renderers
    do not take falls back to render_path (PNGs included), with one warning.  The reports of compare_nerf / use_nerf_max_pts are
    more than a PSNR: ValueError.  ``ssim``: every view is also scored by ns_image_ssim -- the frames render_path returned are
    uploaded for it on the fallback -- and the result is (psnr per view, their mean, ssim per view, their mean[, frames]), with
    ssim.txt beside psnr.txt.

    ``depth`` (the DepthNet frame only): every view's placed samples z [R,N] and the DepthNet's own depth are also scored
    against the frozen field's max-weight fine sample max_z of the same rays (ns_depth_sqerr; score_views states the two
    numbers): the reference's compare_nerf ``MSE:`` without compare_nerf's per-sample host copies.  The view's rays are
    generated once and feed the frame's render, ops.depthnet_forward and ops.render_rays_hierarchical(max_sample=True); the
    PSNRs and SSIMs are those of depth=False bit for bit.  ``field_depths``: the max_z tensors of an earlier call
    (``return_depths``), one per view, valid while the field and its sampling stay as they were -- no hierarchical render is
    launched then.  The result is (psnrs, avg[, ssims, avg_ssim][, sample_mses, avg_sample_mse, mean_mses, avg_mean_mse]
    [, frames][, depths]), ``depths`` per view (z, mean, max_z) on the device, and ``savedir`` gets depth.txt
    (format_depth_txt).  The depth report has no render_path fallback: a configuration that is not eligible for both
    one-call renderers, or use_full_nerf (no DepthNet in that frame), raises ValueError.

    ``frames`` (needs ``savedir``, otherwise ValueError; True, or a dict of FrameWriter's n_buffers / workers /
    compress_level): the views are also written as ``{k:03d}.png`` beside psnr.txt -- render_path's files -- by a FrameWriter:
    quantised on the device (ns_frame_to8b), copied as bytes, encoded off this thread (score_views).  Every score and text
    file keeps its bits.  The render_path fallback writes its PNGs itself."""
    import numpy as np

    _check_frames(frames, savedir, "evaluate_views")
    kw = render_kwargs
    trainer = kw["trainer"]
    if trainer.compare_nerf or trainer.use_nerf_max_pts:
        raise ValueError("evaluate_views reports a PSNR only: compare_nerf / use_nerf_max_pts go through render_path")
    if not depth and (field_depths is not None or return_depths):
        raise ValueError("field_depths / return_depths belong to the depth report: depth=True")
    if depth and trainer.use_full_nerf:
        raise ValueError("evaluate_views(depth=True): a use_full_nerf frame has no DepthNet whose depth could be scored")
    H, W = int(hwf[0]), int(hwf[1])
    if (H, W) != (dataset.H, dataset.W):
        raise ValueError(f"hwf says {H} x {W}, the dataset's images are {dataset.H} x {dataset.W}")
    dev = dataset.device
    net = kw.get("network_fine") if kw.get("network_fine") is not None else kw.get("network_fn")
    if depth:
        with torch.no_grad():
            if not (bool(kw.get("use_viewdirs", False)) and not kw.get("ndc", True)):
                why = "it needs view directions and ndc=False"
            elif not _one_call_eligible(kw.get("depth_network"), net, kw["network_query_fn"], trainer, True):
                why = "the frame is not one of the one-call DepthNet renderer's"
            elif not _hier_one_call_eligible(kw["network_fn"], kw.get("network_fine"), kw["network_query_fn"], trainer, True,
                                             kw["N_samples"], kw.get("raw_noise_std", 0.0), False):
                why = ("the field's depth is not one of the one-call hierarchical renderer's (N_importance > 0, N_samples >= 3, "
                       "no raw noise, this package's NeRF modules and operators)")
            else:
                why = None
        if why is not None:
            raise ValueError(f"evaluate_views(depth=True): {why}; the depth report has no render_path fallback")
        render_frame = _depth_frame_renderer(kw, trainer, net, H, W, K, dev)
        return score_views(dataset, image_ids, poses, render_frame, savedir=savedir, return_frames=return_frames, ssim=ssim,
                           depth=True, field_depths=field_depths, return_depths=return_depths, frames=frames)
    render_frame = _one_call_frame_renderer(kw, H, W, K, dev)
    if render_frame is None:
        _warn_render_path_fallback("evaluate_views")
        gt = _dataset_targets_host(dataset, image_ids)
        if savedir is not None:
            os.makedirs(savedir, exist_ok=True)
        with torch.no_grad():
            rgbs, _disps, avg = render_path(poses, hwf, K, trainer.chunk, kw, step=0, gt_imgs=gt, savedir=savedir)
        psnrs = np.array([-10.0 * np.log10(np.mean(np.square(r - g))) for r, g in zip(rgbs, gt)], dtype=np.float64)
        out = (psnrs, float(avg))
        host_frames = [torch.from_numpy(r).reshape(-1, 3).to(dev) for r in rgbs] if (return_frames or ssim) else None
        if ssim:
            ids = [int(i) for i in np.asarray(image_ids).reshape(-1)]
            sums = torch.empty((len(ids),), dtype=torch.float64, device=dev)
            for k, (img, rgb) in enumerate(zip(ids, host_frames)):
                dataset.image_ssim(img, rgb, out=sums, slot=k)
            ssims = dataset.ssim_from_sum(sums, H, W)
            avg_ssim = float(np.mean(ssims))
            if savedir is not None:
                _write_ssim_txt(savedir, ssims, avg_ssim)
            out += (ssims, avg_ssim)
        return out + (host_frames,) if return_frames else out
    return score_views(dataset, image_ids, poses, render_frame, savedir=savedir, return_frames=return_frames, ssim=ssim,
                       frames=frames)


def write_views(poses, hwf, K, render_kwargs, savedir, return_frames=False, n_buffers=4, workers=4, compress_level=None,
                device="cuda"):
    """evaluate_views' loop without a dataset and without scores: every pose rendered in one call by the frame renderer
    evaluate_views builds and written as ``{k:03d}.png`` under ``savedir`` through a FrameWriter -- the frames of
    render_path(savedir=...) for poses that have no ground truth (render_only without render_test: the spiral
    ``render_poses``).  Nothing but the quantised frames leaves the device.  -> the number of views[, the rgb frames as device
    tensors with ``return_frames``].  A configuration the one-call renderers do not take goes through render_path, with one
    warning, as evaluate_views' does."""
    kw = render_kwargs
    trainer = kw["trainer"]
    if savedir is None:
        raise ValueError("write_views writes the frames as PNGs under savedir: savedir is required")
    if len(poses) == 0:
        raise ValueError("write_views: at least one pose")
    H, W = int(hwf[0]), int(hwf[1])
    dev = torch.device(device)
    render_frame = _one_call_frame_renderer(kw, H, W, K, dev)
    if render_frame is None:
        _warn_render_path_fallback("write_views")
        os.makedirs(savedir, exist_ok=True)
        with torch.no_grad():
            rgbs, _disps, _ = render_path(poses, hwf, K, trainer.chunk, kw, step=0, savedir=savedir)
        host_frames = [torch.from_numpy(r).reshape(-1, 3).to(dev) for r in rgbs] if return_frames else None
        return (len(rgbs), host_frames) if return_frames else len(rgbs)
    workspace = ops.RenderWorkspace()
    kept_frames = []
    with torch.no_grad(), FrameWriter(savedir, H, W, n_buffers=n_buffers, workers=workers, compress_level=compress_level,
                                      device=dev) as writer:
        for k, c2w in enumerate(poses):
            rgb = render_frame(c2w[:3, :4], workspace)
            writer.put(k, rgb)
            if return_frames:
                kept_frames.append(rgb)
    return (len(poses), kept_frames) if return_frames else len(poses)


VIDEO_MAX_DEVICE_BYTES = 2 ** 31              # write_video's default budget for the fp32 disparity maps it holds
_video_png_notice_given = False


def disp_to8b_host(disps, m):
    """write_video's disparity bytes in numpy: to8b(disps / m) of Trainer.py:371-376 -- numpy's float32 division, clip,
    multiply and cast -- with a NaN quotient written as 0 (numpy leaves that cast to the platform)"""
    import numpy as np

    with np.errstate(all="ignore"):
        q = np.asarray(disps, dtype=np.float32) / np.float32(m)
        return np.where(np.isnan(q), 0, 255 * np.clip(q, 0, 1)).astype(np.uint8)


def _write_mp4s(base, n_views):
    """{base}rgb.mp4 and {base}disp.mp4 by the reference's imageio.mimwrite(..., fps=30, quality=8) (Trainer.py:365-376), from
    the bytes of the PNG sequences; without imageio the PNGs are the deliverable, said once.  -> whether they were written"""
    global _video_png_notice_given
    import numpy as np

    try:
        import imageio
    except ImportError:
        if not _video_png_notice_given:
            print("write_video: imageio is not installed; the PNG sequences under rgb/ and disp/ are the deliverable "
                  "(no rgb.mp4 / disp.mp4)")
            _video_png_notice_given = True
        return False
    from PIL import Image

    for name in ("rgb", "disp"):
        frames = []
        for k in range(n_views):
            with Image.open(os.path.join(base + name, "{:03d}.png".format(k))) as im:
                frames.append(np.array(im))
        imageio.mimwrite(base + name + ".mp4", np.stack(frames, 0), fps=30, quality=8)
    return True


def write_video(poses, hwf, K, render_kwargs, base, n_buffers=4, workers=4, compress_level=None, device="cuda",
                max_device_bytes=VIDEO_MAX_DEVICE_BYTES, return_maps=False):
    """The two sequences of the reference's i_video branch (Trainer.py:350-376: ``to8b(rgbs)`` and
    ``to8b(disps / np.max(disps))`` of render_path over the spiral) without render_path: every pose is ONE one-call render (the
    frame renderer of evaluate_views, handing back the disparity map it writes anyway).  The rgb frame goes at once through a
    3-channel FrameWriter to ``{base}rgb/{k:03d}.png``.  The disparity is divided by the maximum over ALL frames, so no frame
    can be quantised before the last one is rendered: the fp32 map is copied device-to-device into slot k of one preallocated
    [n_views, H*W] stack and folded into a two-float state on the device (ops.map_max, accumulate from the second view on).
    After the last view every slot goes through a one-channel FrameWriter (put_map: ops.map_to8b with ``state[:1]`` as the
    divisor, read by the kernel) to ``{base}disp/{k:03d}.png``.  Nothing is read back until the writers are closed; then the
    state, once.  -> {"n_views", "disp_max", "has_nan"}, and with ``return_maps`` "maps": the stack, on the device.

    A disparity can be NaN here and in the reference: torch.max(1e-10, depth / acc) propagates a NaN depth (finish_totals in
    ns_composite_ray.h; a DepthNet ray that misses the sphere has one).  np.max of the reference is then NaN and its disp.mp4
    black.  This path divides by the maximum over the values that are not NaN (``disp_max``; -inf when there are none), writes
    NaN pixels as 0 and reports ``has_nan``.  Where no disparity is NaN the files hold the reference's expression bit for bit
    (``disp_to8b_host`` states it in numpy) -- its weakness included: a ray without any opacity has depth 0 and disparity
    1 / 1e-10 = 1e10, which is then the maximum of the sequence, and every other pixel is 0, as in the reference's video.

    The stack costs n_views * H * W * 4 bytes (102 MB for the 40-pose spiral at 800 x 800); more than ``max_device_bytes``
    raises ValueError naming the bytes needed before anything is rendered or any directory is made.  With imageio installed
    ``{base}rgb.mp4`` and ``{base}disp.mp4`` are also written, as the reference does, from the PNGs' bytes; without it the PNG
    sequences are the deliverable.  ``n_buffers`` / ``workers`` / ``compress_level``: each FrameWriter's (workers are capped by
    FrameWriter.MAX_WORKERS, never sized by the CPU count).  A configuration the one-call renderers do not take goes through
    render_path and numpy, with evaluate_views' one warning, and writes the same files."""
    import numpy as np

    if base is None:
        raise ValueError("write_video writes {base}rgb/ and {base}disp/: base is required")
    n_views = len(poses)
    if n_views == 0:
        raise ValueError("write_video: at least one pose")
    H, W = int(hwf[0]), int(hwf[1])
    need = n_views * H * W * 4
    if need > int(max_device_bytes):
        raise ValueError(f"write_video: the disparity maps of {n_views} views of {H} x {W} need {need} bytes on the device, "
                         f"more than max_device_bytes = {int(max_device_bytes)}")
    kw = render_kwargs
    trainer = kw["trainer"]
    base = str(base)
    rgb_dir, disp_dir = base + "rgb", base + "disp"
    dev = torch.device(device)
    writer_kw = dict(n_buffers=n_buffers, workers=workers, compress_level=compress_level)
    render_frame = _one_call_frame_renderer(kw, H, W, K, dev, with_disp=True)
    if render_frame is None:
        _warn_render_path_fallback("write_video")
        from PIL import Image

        save_kw = {} if compress_level is None else {"compress_level": int(compress_level)}
        for d in (rgb_dir, disp_dir):
            os.makedirs(d, exist_ok=True)
        with torch.no_grad():
            rgbs, disps, _ = render_path(poses, hwf, K, trainer.chunk, kw, step=0, savedir=rgb_dir)
        disps = np.asarray(disps, dtype=np.float32)
        nan = np.isnan(disps)
        disp_max = float(disps[~nan].max()) if not nan.all() else float("-inf")
        for k, d8 in enumerate(disp_to8b_host(disps, disp_max)):
            Image.fromarray(d8.reshape(H, W)).save(os.path.join(disp_dir, "{:03d}.png".format(k)), **save_kw)
        _write_mp4s(base, n_views)
        out = {"n_views": n_views, "disp_max": disp_max, "has_nan": bool(nan.any())}
        if return_maps:
            out["maps"] = torch.from_numpy(disps.reshape(n_views, H * W)).to(dev)
        return out
    workspace = ops.RenderWorkspace()
    stack = torch.empty((n_views, H * W), dtype=torch.float32, device=dev)
    state = torch.empty((2,), dtype=torch.float32, device=dev)
    max_ws = torch.empty((max(ops.map_max_workspace_bytes(H * W), 8),), dtype=torch.uint8, device=dev)
    with torch.no_grad():
        with FrameWriter(rgb_dir, H, W, device=dev, **writer_kw) as writer:
            for k, c2w in enumerate(poses):
                rgb, disp = render_frame(c2w[:3, :4], workspace)
                writer.put(k, rgb)
                stack[k].copy_(disp)                                   # device to device; disp is this call's own tensor
                ops.map_max(stack[k], state=state, accumulate=k > 0, workspace=max_ws)
        with FrameWriter(disp_dir, H, W, channels=1, device=dev, **writer_kw) as writer:
            for k in range(n_views):
                writer.put_map(k, stack[k], denom=state[:1])           # the divisor stays where it is
    disp_max, has_nan = (float(v) for v in state.cpu())                # the one read-back, after the writers are closed
    _write_mp4s(base, n_views)
    out = {"n_views": n_views, "disp_max": disp_max, "has_nan": has_nan != 0.0}
    if return_maps:
        out["maps"] = stack
    return out


# ---- the scene's point cloud selected on the device (the reference: scene_data.pt on the host, then experiments/plot.py) ----
CLOUD_MAX_DEFAULT_CAPACITY = 2 ** 26          # records of a cloud whose capacity the caller leaves open (1.9 GB with colours)


def write_ply(path, pts, rgb, weights) -> None:
    """A binary little-endian PLY point cloud from host arrays: per vertex float x y z, uchar red green blue (``rgb`` in [0, 1]
    through to8b; None: white) and float weight -- 19 bytes each."""
    import numpy as np

    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    n = pts.shape[0]
    weights = np.asarray(weights, dtype=np.float32).reshape(-1)
    colours = np.full((n, 3), 255, dtype=np.uint8) if rgb is None else run_nerf_helpers.to8b(np.asarray(rgb, dtype=np.float32).reshape(-1, 3))
    if weights.shape[0] != n or colours.shape[0] != n:
        raise ValueError(f"{n} points, {colours.shape[0]} colours, {weights.shape[0]} weights")
    vertex = np.empty((n,), dtype=[("xyz", "<f4", (3,)), ("rgb", "u1", (3,)), ("weight", "<f4")])
    vertex["xyz"], vertex["rgb"], vertex["weight"] = pts, colours, weights
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {n}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              "property float weight\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vertex.tobytes())


def _cloud_frame_renderer(kw, trainer, H, W, K, dev, seed):
    """``render(c2w)`` -> (rays_o, rays_d, z [R,N], weights [R,N], rgb [R,3]) of one view, all on the device: the per-sample
    arrays the frame render_rays_test makes for this trainer is composited from, through the one-call renderers and without the
    points.  A configuration they do not take, or one without a weight per sample, raises ValueError."""
    coarse, fine = kw["network_fn"], kw.get("network_fine")
    net = fine if fine is not None else coarse
    if not (bool(kw.get("use_viewdirs", False)) and not kw.get("ndc", True)):
        raise ValueError("scene_cloud: it needs view directions and ndc=False")
    hier = trainer.use_nerf_max_pts or trainer.use_full_nerf
    with torch.no_grad():
        if hier and not _hier_one_call_eligible(coarse, fine, kw["network_query_fn"], trainer, True, kw["N_samples"],
                                                kw.get("raw_noise_std", 0.0), False):
            raise ValueError("scene_cloud: the frame is not one of the one-call hierarchical renderer's (N_importance > 0, "
                             "N_samples >= 3, no raw noise, this package's NeRF modules and operators)")
        if not hier and not _one_call_eligible(kw.get("depth_network"), net, kw["network_query_fn"], trainer, True):
            raise ValueError("scene_cloud: the frame is not one of the one-call DepthNet renderer's")
    if not hier and (trainer.sampling_mode == "depth_only" or int(trainer.n_depth_samples) == 1):
        raise ValueError("scene_cloud: one sample per ray has no weights to threshold (the reference's are [R, 0])")
    workspace = ops.RenderWorkspace()
    perturb = float(kw.get("perturb", 0.0))
    gen = None

    def generator():
        nonlocal gen
        if gen is None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
        return gen

    def render(c2w):
        rays = ops.get_rays(H, W, K, c2w, device=dev)
        if hier:
            # the chain's draws, in _vanilla_one_call's order
            t_rand = torch.rand([H * W, int(kw["N_samples"])], device=dev, generator=generator()) if perturb > 0.0 else None
            u = torch.rand([H * W, int(trainer.N_importance)], device=dev, generator=generator()) if perturb != 0.0 else None
            full = not trainer.use_nerf_max_pts
            out = ops.render_rays_hierarchical(coarse.packed(), fine.packed() if fine is not None else None, rays=rays,
                                               n_coarse=int(kw["N_samples"]), n_importance=int(trainer.N_importance),
                                               lindisp=bool(kw.get("lindisp", False)), white_bkgd=bool(kw["white_bkgd"]),
                                               near=float(kw["near"]), far=float(kw["far"]), t_rand=t_rand, u=u,
                                               extras=("z", "weights") if full else False, device=dev, max_sample=not full,
                                               workspace=workspace)
            if full:
                return rays[0], rays[1], out["z"], out["weights"], out["rgb"]
            return rays[0], rays[1], out["max_z"], out["max_weights"], out["max_rgb"]
        noise = None
        if trainer.sampling_mode == "gaussian":
            noise = torch.randn(H * W, int(trainer.n_depth_samples) - 1, device=dev, generator=generator())
        out = _depthnet_one_call(kw["depth_network"], net, trainer, rays=rays, extras=("z", "weights"), device=dev, noise=noise,
                                 workspace=workspace)
        return rays[0], rays[1], out["z"], out["weights"], out["rgb"]

    return render


def scene_cloud(render_poses, hwf, K, render_kwargs, min_weight=0.0, max_points=None, capacity=None, colours=True,
                savedir=None, seed=0):
    """The scene's point cloud, selected on the device: the device counterpart of render_path(save_scene_data=True) followed by
    experiments/plot.py:13-22 -- ``all_pts[all_weights >= min_weight]`` over the samples of every view of ``render_poses``, and
    then ``max_points`` of them at random -- without a per-sample array ever leaving the device or the points [R,N,3] of a view
    ever being written.  Per view the rays are generated once and rendered in one call by what the trainer in ``render_kwargs``
    selects -- the DepthNet frame (its z and weights [R,N], the frame's rgb), under use_nerf_max_pts the field's max-weight
    sample (max_z / max_weights [R,1], max_rgb), under use_full_nerf the fine pass (z and weights [R,Nc+Nf], its rgb) -- and
    ns_cloud_append appends the samples whose weight is at least ``min_weight`` to one ops.PointCloud, in the order of
    torch.cat(all_pts)[torch.cat(all_weights) >= min_weight]: views, rays, samples.  The points and weights are the bits of that
    expression on render_path's scene_data.pt; a record's colour is its RAY's.

    ``min_weight``: 0.0 is the reference's own (plot.py:17) and keeps every sample with a non-negative weight; raise it.
    ``capacity``: records the cloud has room for; None = the number of candidates, at most 2^26.  More kept than that:
    RuntimeError naming the count (a rerun's capacity).  ``max_points``: when more are kept, exactly that many, drawn uniformly
    without replacement by torch.randperm on a device generator seeded with ``seed`` and kept in the cloud's order (the
    reference's get_random_indices).  ``seed`` also seeds the draws of gaussian placement and of a perturbed field pass.
    One sample per ray through the DepthNet frame (depth_only, n_depth_samples == 1), or a configuration the one-call
    renderers do not take: ValueError.

    Returns dict(pts [M,3], weights [M], rgb [M,3] or None, n_candidates, n_kept) with device tensors; n_kept counts before
    ``max_points``.  ``savedir`` gets scene_cloud.pt -- all_pts, all_weights, all_rgb, min_weight, n_candidates, host tensors
    and numbers only (torch.load(weights_only=True)); a script that reads scene_data.pt's all_pts / all_weights reads it too --
    and scene_cloud.ply (write_ply)."""
    kw = render_kwargs
    trainer = kw["trainer"]
    H, W = int(hwf[0]), int(hwf[1])
    n_views = len(render_poses)
    if n_views == 0:
        raise ValueError("scene_cloud: at least one view")
    if max_points is not None and int(max_points) < 0:
        raise ValueError("max_points must be >= 0")
    net = kw.get("network_fine") if kw.get("network_fine") is not None else kw.get("network_fn")
    dev = next(net.parameters()).device
    render = _cloud_frame_renderer(kw, trainer, H, W, K, dev, seed)
    cloud, n_candidates = None, 0
    with torch.no_grad():
        for c2w in render_poses:
            o, d, z, w, rgb = render(c2w[:3, :4])
            if cloud is None:                                                  # every view has the same R and N
                if capacity is None:
                    capacity = min(n_views * z.numel(), CLOUD_MAX_DEFAULT_CAPACITY)
                cloud = ops.PointCloud(int(capacity), colours=bool(colours), device=dev)
            n_candidates += z.numel()
            cloud.append(o, d, z, w, rgb=rgb if colours else None, min_weight=min_weight)
        n_kept = cloud.count()                                                 # the one device-to-host copy
        if n_kept > cloud.capacity:
            raise RuntimeError(f"scene_cloud: {n_kept} of {n_candidates} samples pass min_weight={min_weight} but the cloud has "
                               f"room for {cloud.capacity}: pass capacity={n_kept}, or raise min_weight")
        pts, weights, rgb = cloud.tensors()
        if max_points is not None and n_kept > int(max_points):
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed))
            idx = torch.sort(torch.randperm(n_kept, device=dev, generator=gen)[:int(max_points)]).values
            pts, weights, rgb = pts[idx], weights[idx], (rgb[idx] if rgb is not None else None)
    out = dict(pts=pts, weights=weights, rgb=rgb, n_candidates=n_candidates, n_kept=n_kept)
    if savedir is not None:
        os.makedirs(savedir, exist_ok=True)
        host = {k: (None if out[k] is None else out[k].cpu()) for k in ("pts", "weights", "rgb")}
        torch.save({"all_pts": host["pts"], "all_weights": host["weights"], "all_rgb": host["rgb"],
                    "min_weight": float(min_weight), "n_candidates": int(n_candidates)}, os.path.join(savedir, "scene_cloud.pt"))
        write_ply(os.path.join(savedir, "scene_cloud.ply"), host["pts"].numpy(),
                  None if host["rgb"] is None else host["rgb"].numpy(), host["weights"].numpy())
    return out


# ---- the field's isosurface mesh extracted on the device (the original NeRF code's extract_mesh notebook; not in the reference) --
def mesh_lattice(lo, hi, resolution):
    """(lo [3], h [3], (Gx, Gy, Gz)) of the lattice over the box [lo, hi]: ``lo`` / ``hi`` one number or three, ``resolution``
    one count of points per axis or (Gx, Gy, Gz).  lo and h = (hi - lo) / (G - 1) are Python floats holding float32 values:
    lattice point idx lies at lo + (float32) idx * h in float32, for field_density_grid and ns_mesh_extract alike."""
    import numpy as np

    def three(v):
        v = [float(x) for x in v] if hasattr(v, "__len__") else [float(v)] * 3
        if len(v) != 3:
            raise ValueError("one number or three")
        return v

    G = tuple(int(x) for x in resolution) if hasattr(resolution, "__len__") else (int(resolution),) * 3
    if len(G) != 3 or min(G) < 2:
        raise ValueError(f"resolution: at least two lattice points per axis, got {resolution!r}")
    lo3 = [float(np.float32(v)) for v in three(lo)]
    h3 = [float(np.float32((b - a) / (g - 1))) for a, b, g in zip(lo3, three(hi), G)]
    if not all(v > 0.0 and np.isfinite(v) for v in h3):
        raise ValueError("hi must lie above lo on every axis")
    return lo3, h3, G


def field_density_grid(network, lo, hi, resolution, chunk=1 << 20):
    """The density relu(raw[..., 3]) of ``network`` (this package's NeRF module) on the lattice mesh_lattice(lo, hi, resolution),
    as one fp32 [Gz,Gy,Gx] device tensor.  A lattice row (fixed j, k) is a ray with o = (lo_x, y_j, z_k), d = (h_x, 0, 0) and
    z = 0 .. Gx - 1: ops.points_along_rays forms lo_x + h_x * i with the multiply and the add rounded separately, so the points
    carry the bits of ns_mesh_extract's lattice positions, and ops.nerf_forward evaluates them on the network's packed handle
    for the current compute dtype -- about ``chunk`` points at a time: the raw of the whole lattice never exists.  The density
    does not depend on the view direction; (0, 0, -1) is passed."""
    lo3, h3, (Gx, Gy, Gz) = mesh_lattice(lo, hi, resolution)
    dev = next(network.parameters()).device
    net = network.packed()
    f32 = dict(dtype=torch.float32, device=dev)
    with torch.no_grad():
        o = torch.empty((Gz, Gy, 3), **f32)
        o[..., 0] = lo3[0]
        o[..., 1] = (lo3[1] + torch.arange(Gy, **f32) * h3[1])[None, :]          # two roundings, as the kernel's
        o[..., 2] = (lo3[2] + torch.arange(Gz, **f32) * h3[2])[:, None]
        o = o.reshape(-1, 3)
        rows = max(1, int(chunk) // Gx)
        d = torch.tensor([h3[0], 0.0, 0.0], **f32).expand(rows, 3).contiguous()
        view = torch.tensor([0.0, 0.0, -1.0], **f32).expand(rows, 3).contiguous()
        steps = torch.arange(Gx, **f32).expand(rows, Gx).contiguous()
        grid = torch.empty((Gz, Gy, Gx), **f32)
        flat = grid.view(Gz * Gy, Gx)
        for r0 in range(0, Gz * Gy, rows):
            n = min(rows, Gz * Gy - r0)
            raw = ops.nerf_forward(net, ops.points_along_rays(o[r0:r0 + n], d[:n], steps[:n]), view[:n])
            flat[r0:r0 + n] = torch.relu(raw[..., 3])
    return grid


def write_mesh_ply(path, vertices, faces, rgb=None) -> None:
    """A binary little-endian PLY triangle mesh from host arrays: per vertex float x y z and, with ``rgb`` (in [0, 1], through
    to8b), uchar red green blue; per face ``property list uchar int vertex_indices`` -- a count of 3 and three int32.
    write_mesh_ply_normals without normals."""
    write_mesh_ply_normals(path, vertices, faces, rgb=rgb, normals=None)


def write_mesh_ply_normals(path, vertices, faces, rgb=None, normals=None) -> None:
    """The one PLY writer: write_mesh_ply's file and, with ``normals`` [V,3], ``property float nx / ny / nz`` directly after z,
    before the colours -- the order MeshLab, Blender and Open3D read."""
    import numpy as np

    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    V, F = vertices.shape[0], faces.shape[0]
    if V >= 2 ** 31 or (F and (faces.min() < 0 or faces.max() >= V)):
        raise ValueError(f"faces index {V} vertices with int32")
    fields = [("xyz", "<f4", (3,))]
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
        if normals.shape[0] != V:
            raise ValueError(f"{V} vertices, {normals.shape[0]} normals")
        fields.append(("n", "<f4", (3,)))
    if rgb is not None:
        colours = run_nerf_helpers.to8b(np.asarray(rgb, dtype=np.float32).reshape(-1, 3))
        if colours.shape[0] != V:
            raise ValueError(f"{V} vertices, {colours.shape[0]} colours")
        fields.append(("rgb", "u1", (3,)))
    vertex = np.empty((V,), dtype=fields)
    vertex["xyz"] = vertices
    if normals is not None:
        vertex["n"] = normals
    if rgb is not None:
        vertex["rgb"] = colours
    face = np.empty((F,), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    face["n"], face["idx"] = 3, faces
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {V}\n"
              "property float x\nproperty float y\nproperty float z\n"
              + ("property float nx\nproperty float ny\nproperty float nz\n" if normals is not None else "")
              + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if rgb is not None else "")
              + f"element face {F}\n"
              "property list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vertex.tobytes())
        f.write(face.tobytes())


def mesh_component_keep(labels, triangles, min_component_triangles=0, keep_largest=0):
    """Which components a filter keeps, as a bool [V] that is set at component roots only -- plain torch on the tensors' device.
    ``labels`` / ``triangles``: ops.mesh_components' (a root r has labels[r] == r and triangles[r] faces).  Kept: the
    components of at least ``min_component_triangles`` faces and, with ``keep_largest`` = k > 0, among those only the k with
    the most faces, a tie going to the smaller label; both given, both hold."""
    min_component_triangles, keep_largest = int(min_component_triangles), int(keep_largest)
    if min_component_triangles < 0 or keep_largest < 0:
        raise ValueError("min_component_triangles and keep_largest must be >= 0")
    V = int(labels.shape[0])
    keep = (labels.long() == torch.arange(V, device=labels.device)) & (triangles >= min_component_triangles)
    if keep_largest > 0:
        roots = torch.nonzero(keep)[:, 0]                                      # ascending label
        order = torch.sort(triangles[roots], descending=True, stable=True).indices     # stable: a tie keeps that order
        keep = torch.zeros_like(keep)
        keep[roots[order[:keep_largest]]] = True
    return keep


def mesh_filter(vertices, faces, rgb=None, min_component_triangles=0, keep_largest=0):
    """Drop a mesh's floaters on the device: split it into the connected components of its faces (ops.mesh_components; two
    faces that share a vertex are connected) and keep what mesh_component_keep keeps.  ``vertices`` [V,3] and ``faces`` int64
    [F,3] on the device, as ops.mesh_weld returns them or from anywhere else; ``rgb`` [V,3] or None is cut as the vertices are.
    The kept vertices and faces stay in their order, the faces renumbered (ops.mesh_select).  Returns dict(vertices, faces, rgb,
    index int64 [V]: old -> new vertex, -1 where dropped; n_components; n_kept_components; n_dropped_triangles: the faces that
    left, those with an index out of range among them; component_triangles: the face counts of all components in label order,
    an int32 device tensor).  Not part of this: per-component area or volume, normals (they need the lattice: scene_mesh_shaded),
    simplification."""
    kept = _mesh_filter(vertices, faces, (rgb,), min_component_triangles, keep_largest)
    return {("rgb" if k == "extras" else k): (v[0] if k == "extras" else v) for k, v in kept.items()}


def _mesh_filter(vertices, faces, extras, min_component_triangles, keep_largest):
    """mesh_filter with any number of per-vertex tensors (colours, normals; a None stays None) cut as the vertices are: its dict
    with ``extras`` a tuple in place of rgb"""
    faces = faces.contiguous()
    comp = ops.mesh_components(faces, int(vertices.shape[0]))
    keep = mesh_component_keep(comp["labels"], comp["triangles"], min_component_triangles, keep_largest)
    got = ops.mesh_select(vertices, faces, comp["labels"], keep, extras=tuple(extras))
    roots = comp["labels"].long() == torch.arange(vertices.shape[0], device=vertices.device)
    return dict(vertices=got["vertices"], faces=got["faces"], extras=got["extras"], index=got["index"],
                n_components=comp["n_components"], n_kept_components=int(keep.sum()),
                n_dropped_triangles=int(faces.shape[0] - got["faces"].shape[0]), component_triangles=comp["triangles"][roots])


def scene_mesh(network, bound=1.5, resolution=256, threshold=50.0, colours=True, savedir=None, capacity=None,
               return_grid=False):
    """A triangle mesh of the field's density, extracted on the device: scene_mesh_filtered without a filter -- its launches,
    its dict, its scene_mesh.ply.  ``threshold``: 50 is a starting value, not a property of a scene -- lower it where the
    surface has holes; the floaters that brings are dropped by scene_mesh_filtered's ``min_component_triangles`` and
    ``keep_largest``, which this signature, kept as it was, does not carry."""
    return scene_mesh_filtered(network, bound=bound, resolution=resolution, threshold=threshold, colours=colours, savedir=savedir,
                               capacity=capacity, return_grid=return_grid)


def scene_mesh_filtered(network, bound=1.5, resolution=256, threshold=50.0, colours=True, savedir=None, capacity=None,
                        return_grid=False, min_component_triangles=0, keep_largest=0):
    """A triangle mesh of the field's density, extracted on the device: what the original NeRF code's extract_mesh notebook
    makes on the host with marching cubes.  field_density_grid samples ``network`` on ``resolution`` points per axis over
    [-bound, bound]^3; ops.mesh_extract turns the lattice into the triangles of the surface density == ``threshold`` by
    marching tetrahedra (closed and facing outwards wherever it stays off the lattice boundary); ops.mesh_weld joins them on
    their lattice-edge keys.  ``threshold``: 50 is a starting value, not a property of a scene -- lower it where the surface
    has holes; the floaters a low threshold brings, small closed blobs of stray density around the object, are what
    ``min_component_triangles`` and ``keep_largest`` drop (mesh_filter: the connected components of the welded faces; only
    those of at least that many triangles stay, and of those only the ``keep_largest`` largest; 0 and 0, the default, launch
    and return what scene_mesh always did).  The filter runs before the colour query, so a dropped vertex is never evaluated; the
    dict then also has n_components, n_kept_components, n_dropped_triangles and component_triangles (mesh_filter), while
    n_triangles stays what ops.mesh_extract counted.  ``colours``: the field is queried once more at the welded vertices, looking
    along the unit vector from the vertex towards the box centre: rgb = sigmoid(raw[:, :3]).  ``capacity``: triangles to make
    room for; None counts first (ops.mesh_extract); fewer than the surface has: RuntimeError naming the count.
    Returns dict(vertices [V,3], faces [F,3] int64, rgb [V,3] or None, n_triangles, n_skipped, lo, h[, grid]) with device
    tensors; lo and h are the lattice's (mesh_lattice).  ``savedir`` gets scene_mesh.ply (write_mesh_ply).  Per-vertex normals
    are scene_mesh_shaded's, of which this is the call without them: the same launches, the same dict, the same file.  Not part
    of this: simplification, per-component area or volume, and lattices of 2^31 points or more."""
    return scene_mesh_shaded(network, bound=bound, resolution=resolution, threshold=threshold, colours=colours, savedir=savedir,
                             capacity=capacity, return_grid=return_grid, min_component_triangles=min_component_triangles,
                             keep_largest=keep_largest, normals=False, colour_view="centre")


def scene_mesh_shaded(network, bound=1.5, resolution=256, threshold=50.0, colours=True, savedir=None, capacity=None,
                      return_grid=False, min_component_triangles=0, keep_largest=0, normals=True, colour_view="centre"):
    """scene_mesh_filtered with per-vertex normals, so that a viewer shades the surface and not the Kuhn split's slivers.
    ``normals``: ops.mesh_normals on the density lattice the mesh was cut from -- the lattice's finite-difference gradient at
    each vertex's own lattice edge, pointing outward; a function of the edge alone, not of the triangles around the vertex.  It
    runs before the filter and the normals are cut as the vertices are.  The dict gains normals [V,3] and n_degenerate_normals
    (vertices of the unfiltered surface whose gradient is zero or not finite: their normal is (0, 0, 0)), and scene_mesh.ply
    carries nx ny nz (write_mesh_ply_normals).  ``colour_view``: "centre" is scene_mesh_filtered's colour query, unchanged;
    "normal" (it needs ``normals``) looks at the surface along its inward normal -n -- on a concave part of an object the
    direction to the box centre is arbitrary --, and along the centre direction exactly where the normal is (0, 0, 0).  With
    ``normals=False`` and "centre" this is scene_mesh_filtered to the launch and to the byte.  Not part of this: normals of
    meshes that did not come from a lattice (no keys), the field's analytic gradient, normal maps of rendered frames.
    Simplification is scene_mesh_simplified's, of which this is the call without it: the same launches, the same dict, the
    same file."""
    return scene_mesh_simplified(network, bound=bound, resolution=resolution, threshold=threshold, colours=colours,
                                 savedir=savedir, capacity=capacity, return_grid=return_grid,
                                 min_component_triangles=min_component_triangles, keep_largest=keep_largest, normals=normals,
                                 colour_view=colour_view, simplify=0)


SIMPLIFY_COUNTERS = ("n_collapsed", "n_invalid", "n_nonfinite", "n_nonfinite_faces", "n_duplicate", "n_clusters")


def simplify_lattice(lo, h, G, simplify):
    """(lo [3], cell [3], dims [3]) of the cluster lattice whose cells are ``simplify`` density-lattice cells wide: it starts at
    the density lattice's own ``lo``, cell = (float32)(simplify * h) per axis, and ceil((G - 1) / simplify) cells cover it (a
    vertex on the far boundary belongs to the last cell: ops.mesh_simplify clamps)."""
    import math

    import numpy as np

    k = float(simplify)
    if not (math.isfinite(k) and k > 0.0):
        raise ValueError(f"simplify must be finite and positive, got {simplify!r}")
    cell = [float(np.float32(k * float(v))) for v in h]
    dims = [max(1, int(math.ceil((int(g) - 1) / k))) for g in G]
    return [float(v) for v in lo], cell, dims


def mesh_simplify(mesh, lo, cell, dims, dedupe=True):
    """Any mesh dict -- scene_mesh_shaded's, or dict(vertices, faces[, rgb][, normals]) from anywhere else -- simplified by
    vertex clustering on the device (ops.mesh_simplify): the vertices of one cell of the lattice (``lo``, ``cell``, ``dims``)
    collapse onto the one of them nearest the cell's centroid, so every vertex that stays keeps its bits, and rgb and normals
    (where the dict has them; a None stays None) are cut as the vertices are.  Returns a copy of the dict with vertices, faces,
    rgb and normals replaced, and with index (old -> new vertex, -1 where not kept), rep, n_input_vertices, n_input_faces and
    ops.mesh_simplify's counters.  Not part of this: quadric error metrics, new vertex positions at the centroid, manifold or
    topology guarantees."""
    vertices, faces, _ = _mesh_tensors(mesh)
    names = [k for k in ("rgb", "normals") if k in mesh]
    got = ops.mesh_simplify(vertices, faces, lo, cell, dims, extras=tuple(mesh[k] for k in names), dedupe=dedupe)
    out = dict(mesh, vertices=got["vertices"], faces=got["faces"], index=got["index"], rep=got["rep"],
               n_input_vertices=int(vertices.shape[0]), n_input_faces=int(faces.shape[0]))
    out.update({k: got["extras"][i] for i, k in enumerate(names)})
    out.update({k: got[k] for k in SIMPLIFY_COUNTERS})
    return out


def scene_mesh_simplified(network, bound=1.5, resolution=256, threshold=50.0, colours=True, savedir=None, capacity=None,
                          return_grid=False, min_component_triangles=0, keep_largest=0, normals=True, colour_view="centre",
                          simplify=0):
    """scene_mesh_shaded, and the mesh simplified by vertex clustering before it is coloured: the lattice-resolution surface
    is millions of slivers, which nobody hands to a viewer.  ``simplify`` = k > 0 (a float): ops.mesh_simplify on a cluster
    lattice of cells k density-lattice cells wide, on the density lattice's own lo (simplify_lattice) -- about k^2 times fewer
    triangles; every vertex that stays is a vertex of the unsimplified surface, bit for bit, with its normal.  The order is
    extract, weld, normals, filter, simplify, colour query: a vertex that leaves is never evaluated.  The dict gains
    n_input_vertices and n_input_faces (what went into the simplification), its counters (n_collapsed, n_invalid, n_nonfinite,
    n_nonfinite_faces, n_duplicate, n_clusters) and simplify_index (int64: the new index of a vertex that went in, -1 where
    it left); scene_mesh.ply is the simplified mesh.  0, the default: nothing is launched and nothing changes -- this is
    scene_mesh_shaded to the launch and to the byte.  Not part of this: quadric error metrics, new vertex positions at the
    centroid, manifold or topology guarantees."""
    lo3, h3, _G = mesh_lattice(-float(bound), float(bound), resolution)
    cluster = None
    import numbers

    if isinstance(simplify, bool) or not isinstance(simplify, numbers.Real) or not float(simplify) >= 0.0:
        raise ValueError(f"simplify must be a number >= 0, got {simplify!r}")
    if float(simplify) != 0.0:
        cluster = simplify_lattice(lo3, h3, _G, simplify)
        ops._cluster_lattice(*cluster)
    if int(min_component_triangles) < 0 or int(keep_largest) < 0:
        raise ValueError("min_component_triangles and keep_largest must be >= 0")
    if colour_view not in ("centre", "normal"):
        raise ValueError(f"colour_view: 'centre' or 'normal', got {colour_view!r}")
    if colour_view == "normal" and not normals:
        raise ValueError("colour_view='normal' needs normals=True")
    with torch.no_grad():
        grid = field_density_grid(network, -float(bound), float(bound), resolution)
        got = ops.mesh_extract(grid, float(threshold), lo3, h3, capacity=capacity)
        if got["n_triangles"] > got["triangles"].shape[0]:
            raise RuntimeError(f"scene_mesh: the surface has {got['n_triangles']} triangles but there is room for "
                               f"{got['triangles'].shape[0]}: pass capacity={got['n_triangles']}")
        vertices, faces = ops.mesh_weld(got["triangles"], got["keys"])
        vertex_normals = n_degenerate = None
        if normals:
            # torch.unique(keys) is the keys in ascending order: ops.mesh_weld's vertex order, so row v is vertex v's normal
            shaded = ops.mesh_normals(grid, float(threshold), h3, torch.unique(got["keys"]))
            vertex_normals, n_degenerate = shaded["normals"], shaded["n_degenerate"]
        kept = None
        if int(min_component_triangles) != 0 or int(keep_largest) != 0:
            kept = _mesh_filter(vertices, faces, (vertex_normals,), min_component_triangles, keep_largest)
            vertices, faces, vertex_normals = kept["vertices"], kept["faces"], kept["extras"][0]
        simplified = None
        if cluster is not None:
            n_input = (int(vertices.shape[0]), int(faces.shape[0]))
            simplified = ops.mesh_simplify(vertices.contiguous(), faces.contiguous(), *cluster, extras=(vertex_normals,))
            vertices, faces, vertex_normals = simplified["vertices"], simplified["faces"], simplified["extras"][0]
        rgb = None
        if colours:
            rgb = torch.empty((vertices.shape[0], 3), dtype=torch.float32, device=vertices.device)
            if vertices.shape[0] > 0:
                towards = -vertices                                            # the box centre is the origin
                towards = towards / towards.norm(dim=-1, keepdim=True).clamp_min(1e-12)
                if colour_view == "normal":                                    # along -n; the centre direction where n is zero
                    flat = (vertex_normals == 0).all(dim=-1, keepdim=True)
                    towards = torch.where(flat, towards, -vertex_normals)
                rgb = torch.sigmoid(ops.nerf_forward(network.packed(), vertices[:, None, :], towards)[:, 0, :3])
    out = dict(vertices=vertices, faces=faces, rgb=rgb, n_triangles=got["n_triangles"], n_skipped=got["n_skipped"], lo=lo3, h=h3)
    if normals:
        out.update(normals=vertex_normals, n_degenerate_normals=n_degenerate)
    if kept is not None:
        out.update({k: kept[k] for k in ("n_components", "n_kept_components", "n_dropped_triangles", "component_triangles")})
    if simplified is not None:
        out.update(n_input_vertices=n_input[0], n_input_faces=n_input[1], simplify_index=simplified["index"])
        out.update({k: simplified[k] for k in SIMPLIFY_COUNTERS})
    if return_grid:
        out["grid"] = grid
    if savedir is not None:
        os.makedirs(savedir, exist_ok=True)
        write_mesh_ply_normals(os.path.join(savedir, "scene_mesh.ply"), vertices.cpu().numpy(), faces.cpu().numpy(),
                               None if rgb is None else rgb.cpu().numpy(),
                               None if vertex_normals is None else vertex_normals.cpu().numpy())
    return out


# ---- the device mesh seen from the held-out cameras and scored where it is made (ns_mesh_raster) ----
def format_mesh_txt(label, values, avg) -> str:
    """mesh_psnr.txt / mesh_depth.txt / mesh_iou.txt of a set of views, psnr.txt's layout: one "NNN.png, LABEL: x" line per view,
    then the average"""
    lines = [f"{i:03d}.png, {label}: {v}\n" for i, v in enumerate(values)]
    return "".join(lines) + f"Avg of {len(lines)} images:\n{label}: {avg}\n"


def _write_mesh_txt(savedir, name, label, values, avg):
    os.makedirs(savedir, exist_ok=True)
    with open(os.path.join(savedir, name), "a") as file:           # appended to, as psnr.txt is
        file.write(format_mesh_txt(label, values, avg))


def _mesh_tensors(mesh):
    if not (isinstance(mesh, dict) and "vertices" in mesh and "faces" in mesh):
        raise ValueError("mesh: the dict of scene_mesh_shaded (vertices, faces, rgb)")
    return mesh["vertices"].contiguous(), mesh["faces"].contiguous(), mesh.get("rgb")


def render_mesh_views(mesh, poses, hwf, K, near, savedir=None, background=0.0, cull=0, n_buffers=4, workers=4,
                      compress_level=None):
    """The mesh of scene_mesh_shaded seen from every pose: ops.mesh_rasterize per view, nothing but the four counters of each
    view read back.  ``mesh``: that dict (vertices, faces, rgb; rgb None: no colour frames).  ``near``: as ops.mesh_rasterize's,
    the near bound of the scene.  With ``savedir`` the colour frames go to ``mesh_rgb/NNN.png`` through a FrameWriter and the
    depth maps to ``mesh_depth/NNN.png`` as write_video writes its disparity: kept in one [n_views, H*W] stack, divided by
    the maximum over ALL views, which stays on the device (ops.map_max, accumulated; FrameWriter.put_map) -- a pixel without a
    face has depth 0 and is black.  -> dict(rgb, depth, tri: one device tensor per view (rgb: None per view without colours);
    n_clipped, n_degenerate, n_invalid, n_covered: one int per view).  A view whose n_clipped is not 0 has a camera inside or
    too close to the mesh: faces were dropped, not clipped."""
    vertices, faces, colours = _mesh_tensors(mesh)
    n_views = len(poses)
    if n_views == 0:
        raise ValueError("render_mesh_views: at least one pose")
    H, W = int(hwf[0]), int(hwf[1])
    dev = vertices.device
    workspace = torch.empty((ops.mesh_raster_workspace_bytes(vertices.shape[0], faces.shape[0], H, W),), dtype=torch.uint8,
                            device=dev)
    out = {k: [] for k in ("rgb", "depth", "tri", "n_clipped", "n_degenerate", "n_invalid", "n_covered")}
    import contextlib

    writer_kw = dict(n_buffers=n_buffers, workers=workers, compress_level=compress_level, device=dev)
    rgb_writer = (FrameWriter(os.path.join(savedir, "mesh_rgb"), H, W, **writer_kw)
                  if savedir is not None and colours is not None else contextlib.nullcontext())
    state = max_ws = None
    if savedir is not None:
        state = torch.empty((2,), dtype=torch.float32, device=dev)
        max_ws = torch.empty((max(ops.map_max_workspace_bytes(H * W), 8),), dtype=torch.uint8, device=dev)
    with torch.no_grad():
        with rgb_writer as writer:
            for k, c2w in enumerate(poses):
                got = ops.mesh_rasterize(vertices, faces, c2w[:3, :4], H, W, K, near, rgb=colours, background=background,
                                         cull=cull, workspace=workspace)
                for name in out:
                    out[name].append(got[name])
                if writer is not None:
                    writer.put(k, got["rgb"])
                if state is not None:
                    ops.map_max(got["depth"], state=state, accumulate=k > 0, workspace=max_ws)
        if savedir is not None:
            with FrameWriter(os.path.join(savedir, "mesh_depth"), H, W, channels=1, **writer_kw) as writer:
                for k in range(n_views):
                    writer.put_map(k, out["depth"][k], denom=state[:1])        # the divisor stays where it is
    return out


def _field_map_renderer(kw, H, W, K, dev):
    """``render(c2w)`` -> (depth [H*W], acc [H*W]) of the field seen from a camera: the one-call renderer evaluate_views would
    take for the configuration ``kw``, asked for its "depth" and "acc" extras -- the expected depth sum w_i z_i in the unit
    ns_mesh_raster writes, and the opacity before the background.  A configuration that is neither renderer's: ValueError."""
    render_frame = _one_call_frame_renderer(kw, H, W, K, dev)
    if render_frame is None:
        raise ValueError("score_mesh_views: the field's depth and opacity maps come from the one-call renderers, and this "
                         "configuration is neither's; pass field_depths and field_accs")
    trainer = kw["trainer"]
    workspace = ops.RenderWorkspace()
    gen = None

    def draw(shape, normal=False):
        nonlocal gen
        if gen is None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(0)
        return (torch.randn if normal else torch.rand)(shape, device=dev, generator=gen)

    def render(c2w):
        if trainer.use_full_nerf:
            fine, perturb, n_imp = kw.get("network_fine"), float(kw.get("perturb", 0.0)), int(trainer.N_importance)
            t_rand = draw([H * W, int(kw["N_samples"])]) if perturb > 0.0 else None
            u = draw([H * W, n_imp]) if perturb != 0.0 and n_imp > 0 else None
            out = ops.render_rays_hierarchical(kw["network_fn"].packed(), fine.packed() if (fine is not None and n_imp > 0) else None,
                                               camera=(H, W, K, c2w, 0, H), n_coarse=int(kw["N_samples"]), n_importance=n_imp,
                                               lindisp=bool(kw.get("lindisp", False)), white_bkgd=bool(kw["white_bkgd"]),
                                               near=float(kw["near"]), far=float(kw["far"]), t_rand=t_rand, u=u,
                                               extras=("depth", "acc"), device=dev, workspace=workspace)
        else:
            net = kw.get("network_fine") if kw.get("network_fine") is not None else kw.get("network_fn")
            noise = None
            if trainer.sampling_mode == "gaussian" and int(trainer.n_depth_samples) > 1:
                noise = draw([H * W, int(trainer.n_depth_samples) - 1], normal=True)
            out = _depthnet_one_call(kw["depth_network"], net, trainer, camera=(H, W, K, c2w, 0, H), extras=("depth", "acc"),
                                     device=dev, noise=noise, workspace=workspace)
        return out["depth"], out["acc"]

    return render


def score_mesh_views(dataset, image_ids, poses, hwf, K, mesh, near, field_depths=None, field_accs=None, render_kwargs=None,
                     savedir=None, cull=0, background=None, frames=False):
    """The mesh of scene_mesh_shaded scored against the photographs and against the field it was cut from, per held-out view,
    nothing per pixel leaving the device.  Every pose is rasterised (render_mesh_views; ``background`` None: white where the
    dataset is ``white_bkgd``, black otherwise -- a dataset of images that were blended before the upload does not know, and
    the caller says 1.0 or 0.0) and gets three numbers:
      mesh_psnr       the mesh's colour frame against image ``image_ids[k]`` of ``dataset`` (DeviceRayDataset.image_sqerr);
      depth_mse       the mesh's depth against the field's expected depth of the same rays, over all H * W pixels
                      (ops.depth_sqerr with one sample per ray; an empty pixel is 0 in both);
      silhouette_iou  |tri >= 0 and acc > 0.5| / |tri >= 0 or acc > 0.5| (1 where both are empty).
    The field's maps are ``field_depths`` / ``field_accs`` (one [H*W] device tensor per view, both or neither), or are rendered
    here from ``render_kwargs`` by the one-call renderer of that configuration with extras=("depth", "acc").  One read-back for
    the whole call, beside render_mesh_views' counters.  ``savedir`` gets mesh_psnr.txt, mesh_depth.txt and mesh_iou.txt in
    psnr.txt's format, and with ``frames`` also render_mesh_views' mesh_rgb/ and mesh_depth/ PNGs.  -> dict(mesh_psnr, depth_mse, silhouette_iou:
    float64 [n]; avg_mesh_psnr, avg_depth_mse, avg_silhouette_iou; n_clipped: per view; views: render_mesh_views' dict;
    field_depths, field_accs: the maps used)."""
    import numpy as np

    ids = [int(i) for i in np.asarray(image_ids).reshape(-1)]
    if len(ids) == 0 or len(ids) != len(poses):
        raise ValueError(f"{len(ids)} image ids for {len(poses)} poses (at least one view)")
    if (field_depths is None) != (field_accs is None):
        raise ValueError("score_mesh_views: field_depths and field_accs come together")
    if field_depths is None and render_kwargs is None:
        raise ValueError("score_mesh_views: the field's maps (field_depths, field_accs) or render_kwargs to render them")
    if field_depths is not None and not (len(field_depths) == len(ids) == len(field_accs)):
        raise ValueError(f"{len(field_depths)} field depths and {len(field_accs)} opacities for {len(ids)} views")
    if mesh.get("rgb") is None:
        raise ValueError("score_mesh_views: the mesh has no colours (scene_mesh_shaded(colours=True))")
    H, W = int(hwf[0]), int(hwf[1])
    if (H, W) != (dataset.H, dataset.W):
        raise ValueError(f"hwf says {H} x {W}, the dataset's images are {dataset.H} x {dataset.W}")
    dev = dataset.device
    n = len(ids)
    if background is None:
        background = 1.0 if dataset.white_bkgd else 0.0
    if frames and savedir is None:
        raise ValueError("score_mesh_views(frames=True) writes the PNGs under savedir: savedir is required")
    views = render_mesh_views(mesh, poses, hwf, K, near, savedir=savedir if frames else None, background=float(background),
                              cull=cull)
    render = _field_map_renderer(render_kwargs, H, W, K, dev) if field_depths is None else None
    sums = torch.empty((4, n), dtype=torch.float64, device=dev)       # squared colour error, squared depth error, |and|, |or|
    depth_ws = torch.empty((ops.depth_sqerr_workspace_bytes(H * W, 1),), dtype=torch.uint8, device=dev)
    depths, accs = [], []
    with torch.no_grad():
        for k, (img, c2w) in enumerate(zip(ids, poses)):
            depth, acc = (field_depths[k], field_accs[k]) if render is None else render(c2w[:3, :4])
            depth, acc = depth.reshape(-1).contiguous(), acc.reshape(-1)
            depths.append(depth)
            accs.append(acc)
            dataset.image_sqerr(img, views["rgb"][k], out=sums[0], slot=k)
            ops.depth_sqerr(views["depth"][k], depth, out=sums[1], slot=k, workspace=depth_ws)
            solid, seen = acc > 0.5, views["tri"][k] >= 0
            sums[2, k] = (solid & seen).sum()
            sums[3, k] = (solid | seen).sum()
    sums = sums.cpu().numpy()                                                 # the one device-to-host copy
    psnrs = dataset.psnr_from_sqerr(sums[0], 3 * H * W)
    mses = ops.mse_from_sqerr(sums[1], H * W)
    ious = np.where(sums[3] > 0, sums[2] / np.maximum(sums[3], 1.0), 1.0)
    out = dict(mesh_psnr=psnrs, depth_mse=mses, silhouette_iou=ious, avg_mesh_psnr=float(np.mean(psnrs)),
               avg_depth_mse=float(np.mean(mses)), avg_silhouette_iou=float(np.mean(ious)), n_clipped=views["n_clipped"],
               views=views, field_depths=depths, field_accs=accs)
    if savedir is not None:
        _write_mesh_txt(savedir, "mesh_psnr.txt", "PSNR", psnrs, out["avg_mesh_psnr"])
        _write_mesh_txt(savedir, "mesh_depth.txt", "MSE", mses, out["avg_depth_mse"])
        _write_mesh_txt(savedir, "mesh_iou.txt", "IoU", ious, out["avg_silhouette_iou"])
    return out


def create_nerf(args, model):
    """(render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer) -- nerf_utils.py:393-494."""
    embed_fn, input_ch = run_nerf_helpers.get_embedder(args.multires, args.i_embed, args.input_dims_embed)
    input_ch_views, embeddirs_fn = 0, None
    if args.use_viewdirs:
        embeddirs_fn, input_ch_views = run_nerf_helpers.get_embedder(args.multires_views, args.i_embed,
                                                                     args.input_dims_embed)
    output_ch = 5 if args.N_importance > 0 else 4
    skips = [4]
    dev = "cuda" if args.device == "cuda" else args.device
    model_nerf = model(D=args.netdepth, W=args.netwidth, input_ch=input_ch, output_ch=output_ch, skips=skips,
                       input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(dev)
    grad_vars = list(model_nerf.parameters())
    model_fine = None
    if args.N_importance > 0:
        model_fine = model(D=args.netdepth_fine, W=args.netwidth_fine, input_ch=input_ch, output_ch=output_ch,
                           skips=skips, input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(dev)
        grad_vars += list(model_fine.parameters())
    network_query_fn = lambda inputs, viewdirs, network_fn: args.run_network(  # noqa: E731
        inputs, viewdirs, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, netchunk=args.netchunk)
    if (isinstance(embed_fn, run_nerf_helpers.Embedder) and isinstance(embeddirs_fn, run_nerf_helpers.Embedder)
            and embed_fn.num_freqs == 10 and embeddirs_fn.num_freqs == 4 and embed_fn.input_dims == 3
            and embeddirs_fn.input_dims == 3):
        standard_query_fn(network_query_fn)
    optimizer = torch.optim.Adam(params=grad_vars, lr=args.lrate, betas=(0.9, 0.999))
    start = 0
    ckpts = []
    if args.ft_path is not None and args.ft_path != "None":
        ckpts = [args.ft_path]
    elif os.path.isdir(os.path.join(args.basedir, args.expname)):
        d = os.path.join(args.basedir, args.expname)
        ckpts = [os.path.join(d, f) for f in sorted(os.listdir(d)) if "tar" in f]
    if len(ckpts) > 0 and not args.no_reload:
        from .utils import load_nerf

        ckpt = torch.load(ckpts[-1], weights_only=True, map_location=dev)
        start = ckpt["global_step"]
        load_nerf(model_nerf, model_fine, optimizer, ckpt)
    render_kwargs_train = {
        "network_query_fn": network_query_fn, "perturb": args.perturb, "N_importance": args.N_importance,
        "network_fine": model_fine, "N_samples": args.N_samples, "network_fn": model_nerf,
        "use_viewdirs": args.use_viewdirs, "white_bkgd": args.white_bkgd, "raw_noise_std": args.raw_noise_std,
        "trainer": args,
    }
    if args.dataset_type != "llff" or getattr(args, "no_ndc", False):
        render_kwargs_train["ndc"] = False
        render_kwargs_train["lindisp"] = args.lindisp
    render_kwargs_test = dict(render_kwargs_train)
    render_kwargs_test["perturb"] = False
    render_kwargs_test["raw_noise_std"] = 0.0
    return render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer


def sample_as_in_NeRF(ray_batch, network_fn, network_fine, network_query_fn, N_samples, trainer, perturb,
                      raw_noise_std, lindisp, white_bkgd, kwargs, pytest):
    """Vanilla coarse+fine pass; 8-tuple (density, z, pts, rgb_map, weights, alphas, disp, raw) -- :497-611."""
    N_rays = ray_batch.shape[0]
    rays_o, rays_d = ray_batch[:, 0:3].contiguous(), ray_batch[:, 3:6].contiguous()
    viewdirs = ray_batch[:, -3:].contiguous() if ray_batch.shape[-1] > 8 else None
    near, far = ray_batch[:, 6].contiguous(), ray_batch[:, 7].contiguous()
    (c_rgb, c_disp, c_acc, c_w, _c_depth, c_z, c_w, _c_raw, _c_alphas) = trainer.sample_coarse_points(
        near=near, far=far, perturb=perturb, N_rays=N_rays, N_samples=N_samples, viewdirs=viewdirs,
        network_fn=network_fn, network_query_fn=network_query_fn, rays_o=rays_o, rays_d=rays_d,
        raw_noise_std=raw_noise_std, white_bkgd=white_bkgd, pytest=pytest, lindisp=lindisp, kwargs=kwargs)
    (_r0, _d0, _a0, f_rgb, f_disp, _f_acc, f_raw, f_z, f_pts, f_density, f_alphas, f_w) = trainer.sample_fine_points(
        z_vals=c_z, weights=c_w, perturb=perturb, pytest=pytest, rays_d=rays_d, rays_o=rays_o, rgb_map=c_rgb,
        disp_map=c_disp, acc_map=c_acc, network_fn=network_fn, network_fine=network_fine,
        network_query_fn=network_query_fn, viewdirs=viewdirs, raw_noise_std=raw_noise_std, white_bkgd=white_bkgd)
    return f_density, f_z, f_pts, f_rgb, f_w, f_alphas, f_disp, f_raw


_fused_step_warned = False


def _fused_step_field(net, network_query_fn, trainer, viewdirs):
    """The f16x3 handle of the frozen field when render_rays' DepthNet branch may run as one kernel (``fused_step``): the
    standard query function, this package's NeRF with view directions, the trainer's own raw2outputs / run_network, and a field
    that packs as f16x3.  None otherwise; a field that does not pack warns once and takes the layer-by-layer path."""
    global _fused_step_warned
    from .trainers import DepthNetTrainer

    if not (viewdirs is not None and getattr(network_query_fn, "_ns_standard_query", False)
            and isinstance(net, run_nerf_helpers.NeRF) and net.use_viewdirs
            and type(trainer).raw2outputs is DepthNetTrainer.raw2outputs
            and type(trainer).run_network is DepthNetTrainer.run_network):
        return None
    try:
        return net.packed("f16x3")
    except (NotImplementedError, RuntimeError, ValueError) as e:
        if not _fused_step_warned:
            import warnings

            warnings.warn(f"fused_step: the field does not pack as f16x3 ({e}); render_rays takes the layer-by-layer path")
            _fused_step_warned = True
        return None


def _render_rays_fused_step(ray_batch, rays_o, rays_d, viewdirs, field, network_fn, network_query_fn, N_samples, trainer,
                            lindisp, perturb, network_fine, white_bkgd, raw_noise_std, pytest, kwargs):
    """render_rays with ``fused_step``: the target pass as one ns_render_rays_hierarchical call where it is eligible (the values of
    sample_as_in_NeRF + argmax_gather bit for bit, random draws in the same order), the DepthNet branch as one
    ns_render_rays_fused_tangent call (autograd.SingleSampleTangentRender).  The same keys as render_rays except ``raw``, which
    stays in the CU."""
    from .autograd import render_single_sample

    ws = kwargs.get("_workspaces") or {}
    with torch.no_grad():
        near_far = kwargs.get("_near_far")
        if near_far is not None and _hier_one_call_eligible(network_fn, network_fine, network_query_fn, trainer, viewdirs,
                                                            N_samples, raw_noise_std, pytest):
            max_z_vals = _vanilla_one_call(rays_o, rays_d, viewdirs, network_fn, network_fine, N_samples, trainer, perturb,
                                           lindisp, white_bkgd, near_far, False, workspace=ws.get("vanilla"))["max_z"]
        else:
            (_dens, fine_z, _pts, _rgb, fine_w, _al, _disp, _raw) = sample_as_in_NeRF(
                ray_batch=ray_batch, N_samples=N_samples, network_fn=network_fn, network_fine=network_fine,
                network_query_fn=network_query_fn, trainer=trainer, perturb=perturb, raw_noise_std=raw_noise_std,
                lindisp=lindisp, white_bkgd=white_bkgd, pytest=pytest, kwargs=kwargs)
            max_z_vals, _, _ = ops.argmax_gather(fine_w, fine_z)
        max_pts = ops.points_along_rays(rays_o, rays_d, max_z_vals)
    depth_net_z_vals = kwargs["depth_network"](rays_o, rays_d)
    rgb_map, disp_map = render_single_sample(depth_net_z_vals, rays_o, rays_d, viewdirs, field, ws.get("tangent"))
    with torch.no_grad():
        depth_net_pts = ops.points_along_rays(rays_o, rays_d, depth_net_z_vals.detach())
    to_host = (lambda t: t) if kwargs.get("_skip_host_copies", False) else (lambda t: t.cpu())
    return {"depth_net_rgb_map": rgb_map, "depth_net_disp_map": disp_map, "depth_net_z_vals": depth_net_z_vals,
            "max_z_vals": max_z_vals, "depth_net_pts": to_host(depth_net_pts), "max_pts": to_host(max_pts)}


def render_rays(ray_batch, network_fn, network_query_fn, N_samples, trainer, retraw=True, lindisp=False,
                perturb=0.0, N_importance=0, network_fine=None, white_bkgd=False, raw_noise_std=0.0,
                verbose=False, pytest=False, **kwargs):
    """Training operator, forward (nerf_utils.py:614-733); same keys / host copies as the reference.

    ``fused_step`` (render kwarg, not in the reference; default off): with the standard configuration (see _fused_step_field)
    the DepthNet branch -- points, the frozen field, single-sample compositing and, in the backward, the field's input-gradient
    chain -- runs as ONE kernel on the field's f16x3 packing, which returns d rgb / d depth beside rgb, and the target pass as one
    hierarchical-renderer call.  ``raw`` is then omitted from the returned keys (it never leaves the CU; nothing in the trainer
    reads it); max_z_vals and depth_net_z_vals are the default path's bits, depth_net_rgb_map is the f16x3 field's (fp32-grade)
    instead of the exact-fp32 kernel's."""
    rays_o, rays_d = ray_batch[:, 0:3].contiguous(), ray_batch[:, 3:6].contiguous()
    viewdirs = ray_batch[:, -3:].contiguous() if ray_batch.shape[-1] > 8 else None
    if kwargs.get("fused_step", False):
        field = _fused_step_field(network_fine if network_fine is not None else network_fn, network_query_fn, trainer, viewdirs)
        if field is not None:
            return _render_rays_fused_step(ray_batch, rays_o, rays_d, viewdirs, field, network_fn, network_query_fn, N_samples,
                                           trainer, lindisp, perturb, network_fine, white_bkgd, raw_noise_std, pytest, kwargs)
    # the vanilla pass only provides the regression target max_z: frozen networks, detached samples
    # (Trainer.py:569) -- no gradient reaches the DepthNet through it
    with torch.no_grad():
        (_dens, fine_z, _pts, _rgb, fine_w, _al, _disp, _raw) = sample_as_in_NeRF(
            ray_batch=ray_batch, N_samples=N_samples, network_fn=network_fn, network_fine=network_fine,
            network_query_fn=network_query_fn, trainer=trainer, perturb=perturb, raw_noise_std=raw_noise_std,
            lindisp=lindisp, white_bkgd=white_bkgd, pytest=pytest, kwargs=kwargs)
        max_z_vals, _, _ = ops.argmax_gather(fine_w, fine_z)
        max_pts = ops.points_along_rays(rays_o, rays_d, max_z_vals)
    from .autograd import points_along_rays as points_along_rays_ag

    depth_net_z_vals = kwargs["depth_network"](rays_o, rays_d)
    depth_net_pts = points_along_rays_ag(rays_o, rays_d, depth_net_z_vals)
    net = network_fine if network_fine is not None else network_fn
    depth_net_raw = network_query_fn(depth_net_pts, viewdirs, net)
    (rgb_map, disp_map, _acc, _depth, _density, _alphas, _weights) = trainer.raw2outputs(
        raw=depth_net_raw, z_vals=depth_net_z_vals, rays_d=rays_d, raw_noise=raw_noise_std, white_bkdg=white_bkgd,
        pytest=pytest)  # (sic) misspelled keywords, as in the reference: noise 0, white background
    # host copies of the reference (:723-727); `_skip_host_copies` (internal: the graph-captured training step, where a
    # blocking copy cannot be recorded and nothing reads these three) leaves them on the device
    to_host = (lambda t: t) if kwargs.get("_skip_host_copies", False) else (lambda t: t.cpu())
    ret = {"depth_net_rgb_map": rgb_map, "depth_net_disp_map": disp_map, "depth_net_z_vals": depth_net_z_vals,
           "max_z_vals": max_z_vals, "depth_net_pts": to_host(depth_net_pts.detach()), "max_pts": to_host(max_pts)}
    if retraw:
        ret["raw"] = to_host(depth_net_raw.detach())
    return ret


def standard_query_fn(fn):
    """Mark a network_query_fn as the standard one (embed + Trainer.run_network through this package's 10 / 4-frequency
    embedders, exactly what create_nerf builds): render_rays_test may then run its DepthNet branch as one fused C call."""
    fn._ns_standard_query = True
    return fn


def _one_call_eligible(depth_network, net, network_query_fn, trainer, viewdirs) -> bool:
    from .depth_net import DepthNet
    from .trainers import DepthNetTrainer

    return (viewdirs is not None and getattr(network_query_fn, "_ns_standard_query", False)
            and isinstance(depth_network, DepthNet) and isinstance(net, run_nerf_helpers.NeRF) and net.use_viewdirs
            and type(trainer).raw2outputs is DepthNetTrainer.raw2outputs
            and type(trainer).run_network is DepthNetTrainer.run_network
            and trainer.sampling_mode in ("uniform", "gaussian", "depth_only")
            and not (torch.is_grad_enabled() and any(p.requires_grad for p in depth_network.parameters())))


def _hier_one_call_eligible(network_fn, network_fine, network_query_fn, trainer, viewdirs, N_samples, raw_noise_std,
                            pytest) -> bool:
    """sample_as_in_NeRF + argmax_gather of render_rays_test as ONE ns_render_rays_hierarchical call: the standard query function,
    this package's NeRF modules with view directions, the trainer's own operators, a fine pass, no noise, no gradient."""
    from .trainers import DepthNetTrainer

    nets = [network_fn] + ([network_fine] if network_fine is not None else [])
    return (viewdirs is not None and getattr(network_query_fn, "_ns_standard_query", False)
            and all(isinstance(n, run_nerf_helpers.NeRF) and n.use_viewdirs for n in nets)
            and all(getattr(type(trainer), f, None) is getattr(DepthNetTrainer, f)
                    for f in ("raw2outputs", "sample_coarse_points", "sample_fine_points", "run_network"))
            and int(trainer.N_importance) > 0 and int(N_samples) >= 3 and raw_noise_std == 0 and not pytest
            and not (torch.is_grad_enabled() and any(p.requires_grad for n in nets for p in n.parameters())))


def _vanilla_one_call(rays_o, rays_d, viewdirs, network_fn, network_fine, N_samples, trainer, perturb, lindisp, white_bkgd,
                      near_far, full, workspace=None):
    """The fine pass's max-weight sample (and with ``full`` its z / weights / pts / rgb / disp) through one
    ns_render_rays_hierarchical call: the values sample_as_in_NeRF + argmax_gather give, bit for bit."""
    R, dev = rays_o.shape[0], rays_o.device
    # the chain's random draws, in its order: stratified jitter (sample_coarse_points), then the inverse-CDF draws
    t_rand = torch.rand([R, N_samples], device=dev) if perturb > 0.0 else None
    u = torch.rand([R, trainer.N_importance], device=dev) if perturb != 0.0 else None
    out = ops.render_rays_hierarchical(network_fn.packed(), network_fine.packed() if network_fine is not None else None,
                                       rays=(rays_o, rays_d, viewdirs), n_coarse=int(N_samples),
                                       n_importance=int(trainer.N_importance), lindisp=bool(lindisp),
                                       white_bkgd=bool(white_bkgd), near=near_far[0], far=near_far[1], t_rand=t_rand, u=u,
                                       extras=("z", "weights") if full else False, device=dev, max_sample=True,
                                       workspace=workspace)
    if full:
        out["pts"] = ops.points_along_rays(rays_o, rays_d, out["z"])
    return out


def _depthnet_one_call(dn, net, trainer, **source):
    """The DepthNet-guided render of the standard configuration as one ops.render_rays_depthnet call, with the choices that are
    the trainer's and the module's to make: the handles of the current compute dtype and their PSNR guard, the renderer (the
    one-kernel renderer wherever it is supported), the trainer's mode / n_samples / std and the DepthNet's bounds.  ``source``:
    the ray source (rays= or camera=), the extras, the device and what else the call takes.  render_rays_test's one-call
    branch and evaluate_views both render through here."""
    dn_w, net_w, guard_w = ops.psnr_guard_handles(dn, net, mode=trainer.sampling_mode, n_samples=trainer.n_depth_samples)
    return ops.render_rays_depthnet(dn_w, net_w, n_samples=trainer.n_depth_samples, mode=trainer.sampling_mode,
                                    std=trainer.distance, near=dn.near, far=dn.far,
                                    sphere_radius=float(dn.sphere_radius.reshape(-1)[0]), white_bkgd=True, guard=guard_w,
                                    guard_long_rays=ops.guard_long_rays(), **source)


def render_rays_test(ray_batch, network_fn, network_query_fn, N_samples, trainer, retraw=True, lindisp=False,
                     perturb=0.0, N_importance=0, network_fine=None, white_bkgd=False, raw_noise_std=0.0,
                     verbose=False, pytest=False, **kwargs):
    """Inference operator (nerf_utils.py:736-876); same keys, shapes and host copies as the reference."""
    rays_o, rays_d = ray_batch[:, 0:3].contiguous(), ray_batch[:, 3:6].contiguous()
    viewdirs = ray_batch[:, -3:].contiguous() if ray_batch.shape[-1] > 8 else None
    ret = {}
    # host copies (nerf_utils.py:820-822, 866-870): blocking `.cpu()` when called on its own; inside batchify_rays_test
    # they go asynchronously into the frame's pinned buffers (_HostSink)
    sink = kwargs.get("_host_sink")
    released_early = False
    to_host = (lambda key, t: sink.put(key, t.detach())) if sink is not None else (lambda key, t: t.cpu())
    if trainer.compare_nerf or trainer.use_nerf_max_pts or trainer.use_full_nerf:
        near_far = kwargs.get("_near_far")
        if near_far is not None and _hier_one_call_eligible(network_fn, network_fine, network_query_fn, trainer, viewdirs,
                                                            N_samples, raw_noise_std, pytest):
            # coarse pass, importance sampling, fine pass and the argmax as one C call: no per-sample array of the coarse pass
            # in HBM, and on 16-bit fields none of the fine pass either (the argmax runs in the MLP kernel's epilogue)
            v = _vanilla_one_call(rays_o, rays_d, viewdirs, network_fn, network_fine, N_samples, trainer, perturb, lindisp,
                                  white_bkgd, near_far, trainer.use_full_nerf and not trainer.use_nerf_max_pts)
            max_z_vals, max_weights, max_rgb_map = v["max_z"], v["max_weights"], v["max_rgb"]
            fine_rgb, fine_disp = v["rgb"], v["disp"]
            fine_w, fine_z, fine_pts = v.get("weights"), v.get("z"), v.get("pts")
        else:
            (_dens, fine_z, fine_pts, fine_rgb, fine_w, _al, fine_disp, fine_raw) = sample_as_in_NeRF(
                ray_batch=ray_batch, N_samples=N_samples, network_fn=network_fn, network_fine=network_fine,
                network_query_fn=network_query_fn, trainer=trainer, perturb=perturb, raw_noise_std=raw_noise_std,
                lindisp=lindisp, white_bkgd=white_bkgd, pytest=pytest, kwargs=kwargs)
            max_z_vals, max_weights, max_rgb_map = ops.argmax_gather(fine_w, fine_z, fine_raw)
        max_pts = ops.points_along_rays(rays_o, rays_d, max_z_vals)
        ret["max_z_vals"], ret["max_pts"] = to_host("max_z_vals", max_z_vals), to_host("max_pts", max_pts)
        ret["max_weights"] = to_host("max_weights", max_weights)
    if trainer.use_nerf_max_pts:
        rgb_map, disp_map = max_rgb_map, torch.zeros_like(max_rgb_map)  # [R,3] disp: reference quirk, :826
        weights, pts, z_vals = max_weights, max_pts, max_z_vals
    elif trainer.use_full_nerf:
        rgb_map, disp_map, weights, pts, z_vals = fine_rgb, fine_disp, fine_w, fine_pts, fine_z
    elif _one_call_eligible(kwargs.get("depth_network"), network_fine if network_fine is not None else network_fn,
                            network_query_fn, trainer, viewdirs):
        # The standard configuration (this package's DepthNet / NeRF modules, the query function create_nerf builds, the
        # trainer's own raw2outputs): DepthNet -> placement -> MLP -> compositing as ONE C call, bit-identical to the
        # operator chain below (tests/test_gpu_render.py::test_fused_matches_operator_chain and the tagged-path test).
        dn = kwargs["depth_network"]
        net = network_fine if network_fine is not None else network_fn
        ev = sink.new_event_pair() if sink is not None else None
        held = _held_sink
        out = _depthnet_one_call(dn, net, trainer, rays=(rays_o, rays_d, viewdirs), extras=True, device=rays_o.device,
                                 mlp_events=ev)
        if sink is not None:
            sink.release(after=ev[0])    # the PREVIOUS chunk's host copies start with this chunk's MLP kernel
            if held is not None and held is not sink:
                held.release(after=ev[0])          # ... and so do the previous FRAME's (render_path's pipeline)
        released_early = True
        rgb_map, disp_map, weights, pts, z_vals = out["rgb"], out["disp"], out["weights"], out["pts"], out["z"]
    else:
        mean = kwargs["depth_network"](rays_o, rays_d)
        pts, z_vals = sample_points_around_mean(rays_o=rays_o, rays_d=rays_d, mean=mean,
                                                n_samples=trainer.n_depth_samples, mode=trainer.sampling_mode,
                                                std=trainer.distance)
        net = network_fine if network_fine is not None else network_fn
        raw = network_query_fn(pts, viewdirs, net)
        (rgb_map, disp_map, _acc, _depth, _density, _alphas, weights) = trainer.raw2outputs(
            raw=raw, z_vals=z_vals, rays_d=rays_d, raw_noise=raw_noise_std, white_bkdg=white_bkgd, pytest=pytest)
    ret["depth_net_rgb_map"] = rgb_map
    ret["depth_net_weights"] = to_host("depth_net_weights", weights)
    ret["depth_net_disp_map"] = to_host("depth_net_disp_map", disp_map)
    ret["depth_net_z_vals"] = to_host("depth_net_z_vals", z_vals)
    ret["depth_net_pts"] = to_host("depth_net_pts", pts)
    if sink is not None and not released_early:
        sink.release()                   # branches without a single MLP kernel to hide behind: copy right away
    return ret
