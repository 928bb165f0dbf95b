"""Float64 front-to-back composite of a device frame (its Splat records, draw order and z plane) over a target, with an optional
per-pixel occluder: the reference of tests/test_gpu_composite.py.  Decode and cut-off as gaussian.wgsl:40-66 (scenes.BoundaryProof);
no early termination.  A pair takes part iff keep(a) and z < D(p)."""
import numpy as np

import scenes


def composite_f64(frame, z, width, height, dst=None, occluder=None, drop=None, swap=None, planes=None):
    """Returns (out [H, W, 4] = C + T dst, T, undecided): `undecided` marks pixels with a fragment within f32 rounding of the
    cut-off.  dst: [H, W, 4] float (None = zeros); occluder: [H, W] view-space depths (None = no test).

    The walk can be mutated (tests/blend_ref.py: what a kernel that loses or exchanges one record would draw): `drop` = a list
    position, counted from the near end, whose record is skipped; `swap` = (i, j), two list positions that change places.
    `planes`: a dict that receives what the depth forms of the blend accumulate (needs z): "wz" = sum of w z, "wsum" = sum of w,
    "median" = the z of the record at which T crosses 0.5 (0 where it never does), "tcross" = how far from 0.5 the T on either
    side of that crossing lies (inf where none), and "first_below" = the list position of the first record that MEETS a
    T < T_MIN = 2^-14 at the pixel (the list's length where none does)."""
    order = frame["sorted"].astype(np.int64)[::-1].copy()  # near -> far
    if swap is not None:
        i, j = swap
        order[i], order[j] = order[j], order[i]
    if drop is not None:
        order = np.delete(order, drop)
    if planes is not None:
        planes.update(wz=np.zeros((height, width)), wsum=np.zeros((height, width)), median=np.zeros((height, width)),
                      tcross=np.full((height, width), np.inf), first_below=np.full((height, width), len(order), dtype=np.int64))
    h = np.ascontiguousarray(frame["splats"]).view(np.float16).reshape(-1, 10).astype(np.float64)
    W, H = float(width), float(height)
    T = np.ones((height, width))
    C = np.zeros((height, width, 4))
    undecided = np.zeros((height, width), dtype=bool)
    D = None if occluder is None else np.asarray(occluder, dtype=np.float32)
    e = 2.0 ** -24
    rad = np.sqrt(scenes.CUT_A) * 1.001
    for pos, s in enumerate(order):
        if planes is not None:
            np.minimum(planes["first_below"], np.where(T < 2.0 ** -14, pos, len(order)), out=planes["first_below"])
        m00, m01, m10, m11 = h[s, 0] * W, h[s, 2] * W, -h[s, 1] * H, -h[s, 3] * H
        det = m00 * m11 - m01 * m10
        if not np.isfinite(det) or det == 0:
            continue
        i00, i01, i10, i11 = m11 / det, -m01 / det, -m10 / det, m00 / det
        cx, cy = (h[s, 4] * 0.5 + 0.5) * W, (0.5 - h[s, 5] * 0.5) * H
        ex, ey = rad * np.hypot(m00, m01) + 2, rad * np.hypot(m10, m11) + 2
        x0, x1 = max(int(np.floor(cx - ex)), 0), min(int(np.ceil(cx + ex)), width - 1)
        y0, y1 = max(int(np.floor(cy - ey)), 0), min(int(np.ceil(cy + ey)), height - 1)
        if x0 > x1 or y0 > y1:
            continue
        xs = np.arange(x0, x1 + 1) + 0.5 - cx
        ys = np.arange(y0, y1 + 1)[:, None] + 0.5 - cy
        t00, t01, t10, t11 = i00 * xs, i01 * ys, i10 * xs, i11 * ys
        p0, p1 = t00 + t01, t10 + t11
        a = p0 * p0 + p1 * p1
        e0 = 6 * e * (np.abs(t00) + np.abs(t01)) + 4 * e * 64.0 * (abs(i00) + abs(i01))
        e1 = 6 * e * (np.abs(t10) + np.abs(t11)) + 4 * e * 64.0 * (abs(i10) + abs(i11))
        tol = 4.0 * (2 * np.abs(p0) * e0 + 2 * np.abs(p1) * e1 + 2 * e * a) + 1e-7
        keep = a <= scenes.CUT_A
        if D is not None:
            front = np.float32(z[s]) < D[y0:y1 + 1, x0:x1 + 1]  # the f32 comparison the kernel makes
            keep &= front
            undecided[y0:y1 + 1, x0:x1 + 1] |= (np.abs(a - scenes.CUT_A) <= tol) & front
        else:
            undecided[y0:y1 + 1, x0:x1 + 1] |= np.abs(a - scenes.CUT_A) <= tol
        b = np.where(keep, np.minimum(0.99, np.exp(-a) * h[s, 9]), 0.0)
        Tb = T[y0:y1 + 1, x0:x1 + 1]
        w = b * Tb
        for c in range(3):
            C[y0:y1 + 1, x0:x1 + 1, c] += w * h[s, 6 + c]
        C[y0:y1 + 1, x0:x1 + 1, 3] += w
        if planes is not None:
            box = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            cross = keep & (Tb > 0.5) & (Tb - w <= 0.5)
            planes["median"][box] = np.where(cross, z[s], planes["median"][box])
            planes["tcross"][box] = np.where(cross, np.minimum(np.abs(Tb - 0.5), np.abs(Tb - w - 0.5)), planes["tcross"][box])
            planes["wz"][box] += w * float(z[s])
            planes["wsum"][box] += w
        T[y0:y1 + 1, x0:x1 + 1] = Tb - w
    d = np.zeros((height, width, 4)) if dst is None else np.asarray(dst, dtype=np.float64)
    return C + T[..., None] * d, T, undecided


def saturated_quadrants(alpha, qw=8, qh=8):
    """Pixels of 8x8 blocks (the FAST blend's waves) whose every pixel has coverage >= 1 - 2^-14: only there may a wave have
    ended its walk early, so only there may two lists of different make-up composite different post-saturation
    remainders."""
    h, w = alpha.shape
    sat = alpha >= np.float32(1.0 - 2.0 ** -14)
    out = np.zeros_like(sat)
    for y in range(0, h, qh):
        for x in range(0, w, qw):
            blk = sat[y:y + qh, x:x + qw]
            if blk.all():
                out[y:y + qh, x:x + qw] = True
    return out
