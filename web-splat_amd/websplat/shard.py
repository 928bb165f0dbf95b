"""View sharding across the GPUs of one node.

A frame is a pure function of (scene, camera): the scene is replicated, view i goes to rank i mod N, and no
collective sits on the data path.  The only communication is the reduction of the timing at the end.
`dist` is torch.distributed (backend "nccl" = RCCL on the GPU box, "gloo" in the CPU tests).
"""
from typing import List, Optional, Tuple


def views_for_rank(n_views: int, rank: int, world: int) -> List[int]:
    if world < 1 or not (0 <= rank < world):
        raise ValueError("bad rank / world size")
    return list(range(rank, n_views, world))


def aggregate_throughput(frames_local: int, elapsed_local: float, dist=None, device: str = "cpu") -> Tuple[int, float]:
    """(total frames over all ranks, MAX elapsed over ranks).  Whole-job fps = frames / elapsed."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return frames_local, elapsed_local
    import torch
    t = torch.tensor([float(elapsed_local)], dtype=torch.float64, device=device)
    f = torch.tensor([float(frames_local)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(f, op=dist.ReduceOp.SUM)
    return int(round(f.item())), float(t.item())


def gather_view_assignment(my_views: List[int], dist=None) -> Optional[List[List[int]]]:
    """All ranks' view lists (verification only; never on the timed path)."""
    if dist is None or not dist.is_initialized():
        return [my_views]
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, my_views)
    return out


def reduce_contrib(sum_q32, max_weight, dist=None, device: str = "cpu"):
    """All-reduce the per-Gaussian contribution arrays of ranks that scored disjoint camera subsets (Contrib.download()):
    (sum_q32 uint64, max_weight float32) over the default process group -- integer SUM and float MAX, both exact, so every
    rank ends with the accumulator one rank would have built from all cameras.  The sums travel as int64: a q32 sum must stay
    below 2^63, i.e. a Gaussian's total weight below 2^31 (one that covers every pixel of a 1080p frame at weight 1 reaches
    that after a thousand frames); a value at or above 2^63, before or after the reduction, raises OverflowError."""
    import numpy as np
    q = np.ascontiguousarray(sum_q32, dtype=np.uint64)
    m = np.ascontiguousarray(max_weight, dtype=np.float32)
    if q.size and int(q.max()) >= 1 << 63:
        raise OverflowError("reduce_contrib: a q32 sum of 2^63 or more does not travel as int64")
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return q.copy(), m.copy()
    import torch
    tq = torch.from_numpy(q.view(np.int64).copy()).to(device)
    tm = torch.from_numpy(m.copy()).to(device)
    dist.all_reduce(tq, op=dist.ReduceOp.SUM)
    dist.all_reduce(tm, op=dist.ReduceOp.MAX)
    if tq.numel() and int(tq.min().item()) < 0:
        raise OverflowError("reduce_contrib: the reduced q32 sums left the int64 range")
    return tq.cpu().numpy().view(np.uint64), tm.cpu().numpy()


def reduce_grad(q32, dist=None, device: str = "cpu"):
    """All-reduce the per-Gaussian gradient sums of ranks that scored disjoint camera subsets (Grad.download(): (N, 4) int64)
    over the default process group: an int64 SUM, exact, so every rank ends with the accumulator one rank would have built
    from all cameras.  The sums wrap silently in int64, so the magnitudes travel beside them: where the ranks' |q| together reach
    2^62 (a Gaussian's gradient magnitude 2^30 times the calls' scales) the result is not trusted and OverflowError is raised."""
    import numpy as np
    q = np.ascontiguousarray(q32, dtype=np.int64)
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return q.copy()
    import torch
    tq = torch.from_numpy(q.copy()).to(device)
    # |sum| <= sum of |q|, taken in float64: its rounding is far below the factor of two left to 2^63
    mag = torch.from_numpy(np.abs(q.astype(np.float64))).to(device)
    dist.all_reduce(tq, op=dist.ReduceOp.SUM)
    dist.all_reduce(mag, op=dist.ReduceOp.SUM)
    if mag.numel() and float(mag.max().item()) >= 2.0 ** 62:
        raise OverflowError("reduce_grad: the reduced q32 sums may have left the int64 range")
    return tq.cpu().numpy()


def reduce_shgrad(sums, dist=None, device: str = "cpu"):
    """All-reduce the SH gradient sums of ranks that scored disjoint camera subsets (ShGrad.download(): {"sh": (N, ncoef, 3)
    int64, "opacity": (N,) int64}) over the default process group: reduce_grad on each array, under its overflow rule.  Every
    rank ends with what ShGrad.add needs to hold the accumulator one rank would have built from all cameras."""
    return {"sh": reduce_grad(sums["sh"], dist, device), "opacity": reduce_grad(sums["opacity"], dist, device)}
