"""Multi-GPU layer: one process per GPU (torch.distributed, backend "nccl" == RCCL over xGMI).

The path shards by image rows: rank r renders the rows j with j % world == r of the SAME
image (cyclic, because cost is strongly row dependent; single rows, because cost also grows steadily towards the
bottom of the picture: with 4-row blocks the rank that always got the lowest rows of each band had 2 % more
work than the mean, with single rows 0.5 % -- tools/shard_balance_probe.py), every rank holds
the whole (tiny) scene, and the only exchange step is one gather of the finished strips to rank 0,
which de-interleaves them.  Each pixel depends only on (global pixel id, s, seed), so the assembled
image is byte-identical to the single-GPU image.  No other collective exists on the path.

Denoising the sharded picture (PostExchange, denoise_gathered) is again one gather: hdr, second moments and features of every rank's
strip in one buffer, filtered on rank 0 by rt_denoise_shards, which reads the gathered parts through the row mapping.  With the
feature ids in the same buffer (PostExchange(with_ids=True)) rank 0 also keeps the temporal history of the sharded picture
(denoise_gathered_temporal, rt_denoise_shards_temporal).
"""
import numpy as np

from ._capi import BLOCK_ROWS, RT_VARIANCE_SPATIAL, RtRowset


def shard_rowset(H, rank, world, block_rows=BLOCK_ROWS):
    return RtRowset(0, H, block_rows, rank, world)


def local_rows(H, rank, world, block_rows=BLOCK_ROWS):
    nblocks = (H + block_rows - 1) // block_rows
    rows = 0
    for b in range(rank, nblocks, world):
        rows += min(block_rows, H - b * block_rows)
    return rows


def global_row(lr, rank, world, block_rows=BLOCK_ROWS):
    return ((lr // block_rows) * world + rank) * block_rows + lr % block_rows


def max_local_rows(H, world, block_rows=BLOCK_ROWS):
    return max(local_rows(H, r, world, block_rows) for r in range(world))


def assemble(parts, H, world, block_rows=BLOCK_ROWS):
    """parts[r]: array [>= local_rows(r), W, C] (padding rows beyond local_rows are ignored)."""
    first = np.asarray(parts[0])
    out = np.zeros((H,) + first.shape[1:], dtype=first.dtype)
    for r in range(world):
        p = np.asarray(parts[r])
        for lr in range(local_rows(H, r, world, block_rows)):
            out[global_row(lr, r, world, block_rows)] = p[lr]
    return out


def gather_strip(strip, H, rank, world, dst=0, group=None):
    """Gather per-rank strips (torch tensors [rows_r, W, C] on the rank's device) to `dst`.

    Strips are padded to the largest shard so that one equal-count gather serves ragged heights.
    Returns the list of tensors on dst, None elsewhere."""
    import torch
    import torch.distributed as dist
    rows_max = max_local_rows(H, world)
    if strip.shape[0] < rows_max:
        pad = torch.zeros((rows_max - strip.shape[0],) + tuple(strip.shape[1:]), dtype=strip.dtype, device=strip.device)
        strip = torch.cat([strip, pad], 0)
    strip = strip.contiguous()
    if world == 1:
        return [strip]
    out = [torch.empty_like(strip) for _ in range(world)] if rank == dst else None
    dist.gather(strip, out, dst=dst, group=group)
    return out


class StripExchange:
    """One buffer per rank holding its HDR strip (float32) followed by its LDR strip (uint8), both padded to the largest shard,
    and ONE gather per step for the two of them (two collectives of a megabyte each cost twice the launch and rendezvous)."""

    def __init__(self, H, W, rank, world, device):
        import torch
        self.H, self.W, self.rank, self.world = H, W, rank, world
        self.rows = local_rows(H, rank, world)
        self.rows_max = max_local_rows(H, world)
        self.hdr_bytes = self.rows_max * W * 3 * 4
        self.buf = torch.zeros(self.hdr_bytes + self.rows_max * W * 3, dtype=torch.uint8, device=device)
        self.hdr = self.buf[:self.hdr_bytes].view(torch.float32).view(self.rows_max, W, 3)
        self.ldr = self.buf[self.hdr_bytes:].view(self.rows_max, W, 3)
        self.out = [torch.empty_like(self.buf) for _ in range(world)] if (rank == 0 and world > 1) else None

    def gather(self, through_host=False):
        """-> (hdr parts, ldr parts) on rank 0, (None, None) elsewhere.  through_host: CPU tensors over gloo (rehearsal)."""
        import torch
        import torch.distributed as dist
        if self.world == 1:
            return [self.hdr], [self.ldr]
        if through_host:
            src = self.buf.cpu()
            out = [torch.empty_like(src) for _ in range(self.world)] if self.rank == 0 else None
        else:
            src, out = self.buf, self.out
        dist.gather(src, out, dst=0)
        if self.rank != 0:
            return None, None
        W, rm, hb = self.W, self.rows_max, self.hdr_bytes
        return ([o[:hb].view(torch.float32).view(rm, W, 3) for o in out], [o[hb:].view(rm, W, 3) for o in out])


class PostExchange:
    """What the denoiser needs of a row-sharded picture, brought to rank 0 in ONE gather: each rank's buffer holds its HDR strip, its
    strip of second moments (rt_set_noise_estimate) and its feature strip (rt_render_features), all float32 sums, each padded to the
    largest shard: [rows_max * W * 3 | rows_max * W * 3 | rows_max * W * 8].  On rank 0 the gathered buffers are regrouped -- three
    strided copies on the device, no pass over the host -- into hdr_parts, sq_parts [world, rows_max, W, 3] and feat_parts
    [world, rows_max, W, 8], each contiguous and an allocation of its own: exactly the layout rt_shard_parts takes
    (HipRenderer.denoise_shards, denoise_gathered below).  The padding rows are never read by the filter.

    with_ids=True (temporal accumulation, denoise_gathered_temporal below) adds a tail of rows_max * W words to the buffer: the rank's
    feature ids.  They are uint32 and travel as the bytes they are -- the buffer's float32 is only its element size, nothing ever
    converts them -- viewed as int32 at both ends, and rank 0 regroups them into ids_parts [world, rows_max, W] int32 (torch has no
    arithmetic-free uint32 tensor everywhere; the bits are the ids').  Without it the buffer, cut and the results are what they were.

    with_moments=False (the spatial variance source, denoise_gathered(..., variance=...) below) leaves the strip of second moments out:
    the buffer is [hdr 3 | feat 8 | ids 1 if with_ids] words per pixel, 11 or 12 instead of 14 or 15; fill() copies no moments, so the
    ranks may render ONE sample with the noise estimate off; sq and sq_parts are None and gather() returns None in their place.  With the
    default the buffer, cut and the results are what they were."""

    def __init__(self, H, W, rank, world, device, block_rows=BLOCK_ROWS, with_ids=False, with_moments=True):
        import torch
        self.H, self.W, self.rank, self.world, self.block_rows, self.device = H, W, rank, world, block_rows, device
        self.with_ids, self.with_moments = with_ids, with_moments
        self.rows = local_rows(H, rank, world, block_rows)
        self.rows_max = max_local_rows(H, world, block_rows)
        px = self.rows_max * W
        self.cut = (3 * px, 6 * px, 14 * px) if with_moments else (3 * px, 3 * px, 11 * px)  # floats: end of hdr, of sq, of feat
        self.words = self.cut[2] + (px if with_ids else 0)  # 4-byte elements of the buffer
        self.buf = torch.zeros(self.words, dtype=torch.float32, device=device)
        self.hdr = self.buf[:self.cut[0]].view(self.rows_max, W, 3)
        self.sq = self.buf[self.cut[0]:self.cut[1]].view(self.rows_max, W, 3) if with_moments else None
        self.feat = self.buf[self.cut[1]:self.cut[2]].view(self.rows_max, W, 8)
        self.ids = self.buf[self.cut[2]:].view(torch.int32).view(self.rows_max, W) if with_ids else None
        self.hdr_parts = self.sq_parts = self.feat_parts = self.ids_parts = None
        if rank == 0:
            self.all = torch.empty((world, self.words), dtype=torch.float32, device=device) if world > 1 else self.buf.view(1, -1)
            self.hdr_parts = torch.empty((world, self.rows_max, W, 3), dtype=torch.float32, device=device)
            self.sq_parts = torch.empty_like(self.hdr_parts) if with_moments else None
            self.feat_parts = torch.empty((world, self.rows_max, W, 8), dtype=torch.float32, device=device)
            if with_ids:
                self.ids_parts = torch.empty((world, self.rows_max, W), dtype=torch.int32, device=device)

    def fill(self, renderer):
        """This rank's three strips (with_ids: and its ids), device to device into the buffer.  Asynchronous on the renderer's stream.
        Where that is the stream the gather runs on -- a torch.cuda.Stream() made current and handed to renderer.set_stream(), as in
        bench.py -- the gather is ordered behind the copies and nothing has to wait.  Where it is not, call renderer.synchronize()
        before gather(): that is also the case after set_stream(torch.cuda.current_stream().cuda_stream) under torch's DEFAULT
        stream, whose handle is 0 and therefore selects the renderer's own stream (rt_api.h at rt_set_stream)."""
        renderer.copy_to_device(self.hdr.data_ptr(), None)
        if self.with_moments:
            renderer.copy_moments_to_device(self.sq.data_ptr())
        renderer.copy_features_to_device(self.feat.data_ptr(), self.ids.data_ptr() if self.with_ids else None)

    def gather(self, through_host=False):
        """-> (hdr_parts, sq_parts, feat_parts) on rank 0, (None, None, None) elsewhere; with_ids: ids_parts as a fourth value (a fourth
        None); with_moments=False: sq_parts is None.  through_host: CPU tensors over gloo (rehearsal: ranks that share a device); the parts still end on rank 0's device."""
        import torch.distributed as dist
        if self.world > 1:
            if through_host:
                import torch
                src = self.buf.cpu()
                got = torch.empty((self.world, self.words), dtype=torch.float32) if self.rank == 0 else None
                dist.gather(src, [got[s] for s in range(self.world)] if self.rank == 0 else None, dst=0)
                if self.rank == 0:
                    self.all.copy_(got)
            else:
                dist.gather(self.buf, [self.all[s] for s in range(self.world)] if self.rank == 0 else None, dst=0)
        if self.rank != 0:
            return (None, None, None, None) if self.with_ids else (None, None, None)
        shape3, shape8 = (self.world, self.rows_max, self.W, 3), (self.world, self.rows_max, self.W, 8)
        self.hdr_parts.copy_(self.all[:, :self.cut[0]].reshape(shape3))
        if self.with_moments:
            self.sq_parts.copy_(self.all[:, self.cut[0]:self.cut[1]].reshape(shape3))
        self.feat_parts.copy_(self.all[:, self.cut[1]:self.cut[2]].reshape(shape8))
        if self.with_ids:
            import torch
            self.ids_parts.copy_(self.all[:, self.cut[2]:].view(torch.int32).reshape(self.world, self.rows_max, self.W))
            return self.hdr_parts, self.sq_parts, self.feat_parts, self.ids_parts
        return self.hdr_parts, self.sq_parts, self.feat_parts


def _sq_ptr(who, xch, variance):
    """The gathered second moments' address, or None where the exchange carries none -- which only the spatial source accepts."""
    if xch.sq_parts is not None:
        return xch.sq_parts.data_ptr()
    if variance is None or variance.source != RT_VARIANCE_SPATIAL:
        raise ValueError(who + ": the moments source needs the second moments, and the exchange carries none (PostExchange(..., with_moments=True))")
    return None


def denoise_gathered(renderer, xch, n, m, params=None, timed=False, variance=None):
    """Rank 0, after xch.gather() of a PostExchange on the renderer's device: rt_denoise_shards over the gathered parts (n samples in
    hdr and sq, m in feat).  The H x W result is the renderer's download_denoised() / copy_denoised_to_device().  The regrouping copies
    of gather() ran on torch's current stream: they are waited for here.  variance (HipRenderer.denoise_shards): None, or an
    RtVarianceParams; the spatial source runs on one-sample frames and over an exchange without moments (with_moments=False)."""
    import torch
    if xch.rank != 0 or xch.hdr_parts is None:
        raise ValueError("denoise_gathered: rank 0 holds the gathered parts")
    sq = _sq_ptr("denoise_gathered", xch, variance)
    if xch.hdr_parts.is_cuda:
        torch.cuda.current_stream(xch.hdr_parts.device).synchronize()
    return renderer.denoise_shards(xch.hdr_parts.data_ptr(), sq, xch.feat_parts.data_ptr(), xch.W, xch.H, xch.world, xch.rows_max, n, m, params=params,
                                   timed=timed, block_rows=xch.block_rows, variance=variance)


def denoise_gathered_temporal(renderer, xch, n, m, camera, params=None, tparams=None, fetch=1, timed=False):
    """Rank 0, after xch.gather() of a PostExchange(with_ids=True) on the renderer's device: rt_denoise_shards_temporal over the gathered
    parts -- denoise_gathered with the renderer's history blended in (HipRenderer.denoise_shards_temporal).  camera: the rt_camera record
    every rank rendered the frame with (scene.camera).  Call it frame after frame on the same renderer: the history is the renderer's."""
    return denoise_gathered_temporal_variance(renderer, xch, n, m, camera, params, tparams, fetch, timed)


def denoise_gathered_temporal_variance(renderer, xch, n, m, camera, params=None, tparams=None, fetch=1, timed=False, variance=None):
    """denoise_gathered_temporal with the variance source chosen (HipRenderer.denoise_shards_temporal_variance), over the same history:
    variance None is denoise_gathered_temporal; the spatial source runs on one-sample frames and over an exchange without moments."""
    import torch
    who = "denoise_gathered_temporal" if variance is None else "denoise_gathered_temporal_variance"
    if xch.rank != 0 or xch.hdr_parts is None:
        raise ValueError(who + ": rank 0 holds the gathered parts")
    if xch.ids_parts is None:
        raise ValueError(who + ": the exchange carries no ids (PostExchange(..., with_ids=True))")
    sq = _sq_ptr(who, xch, variance)
    if xch.hdr_parts.is_cuda:
        torch.cuda.current_stream(xch.hdr_parts.device).synchronize()
    return renderer.denoise_shards_temporal_variance(xch.hdr_parts.data_ptr(), sq, xch.feat_parts.data_ptr(), xch.ids_parts.data_ptr(), xch.W, xch.H, xch.world,
                                                     xch.rows_max, n, m, camera, params=params, tparams=tparams, fetch=fetch, timed=timed,
                                                     block_rows=xch.block_rows, variance=variance)
