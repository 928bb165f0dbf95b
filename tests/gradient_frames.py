"""What test_gpu_gradient.py and test_gradient_abi.py need beyond attrib_frames: the signed ramp plane, a Grad per call, the frame's
per-Gaussian Splat halves."""
import numpy as np

from attrib_frames import BG, F


def signed_ramp(width, height):
    """A smooth signed ramp in all four components (H x W x 4 float32), every value inside (-1, 1) and none of them 0."""
    x = (np.arange(width, dtype=np.float64)[None, :] + 0.5) / width
    y = (np.arange(height, dtype=np.float64)[:, None] + 0.5) / height
    g = np.stack([0.9 * np.sin(2.3 * x + 1.1 * y + 0.3), 0.8 * np.cos(1.7 * x - 2.9 * y + 0.2) + 0.05, 0.7 * (x - y) + 0.013,
                  0.6 * np.sin(3.1 * (x + y)) - 0.21], axis=-1).astype(F)
    assert np.abs(g).max() < 1 and (g != 0).all() and (g < 0).any(axis=(0, 1)).all() and (g > 0).any(axis=(0, 1)).all()
    return g


def gradient(f, plane, background=BG, scale=1.0, opacity_scale=1.0, base=False, **kw):
    """(N, 4) int64 sums of one accumulate_gradient call on the attrib_frames._Frame f (and the base plane with base=True)."""
    acc = f.ws.Grad(f.c, f.n)
    try:
        f.r.accumulate_gradient(f.pc, acc, plane, background=background, scale=scale, opacity_scale=opacity_scale, base=base, **kw)
        assert acc.frames == 1
        q = acc.download()
    finally:
        acc.close()
    return (q, f.r.download_removal_base()) if base else q


def splat_halves(frame, num_points):
    """(num_points, 10) float64: the Splat record's halves per SOURCE Gaussian (NaN where it is not in the frame)."""
    h = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    src = frame["src_index"].astype(np.int64)
    out = np.full((num_points, 10), np.nan)
    out[src] = h[: src.size]
    return out
