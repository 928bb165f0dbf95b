"""What test_gpu_sh_gradient.py and test_gpu_sh_refit.py need beyond attrib_frames: a camera off the optical axis of the stack (on
it the direction is (0, 0, 1) and most of the SH basis is exactly 0), the stack turned towards it, clouds of any degree."""
import numpy as np

import blend_ref
from attrib_frames import F, _stack
from websplat import synth

TILE = (32, 32)
EYE = np.array([-1.8, 1.2, -2.0994], np.float64)   # |EYE| ~ 3.0: every basis of degree 1 .. 3 is far from 0 along it


def _oblique(ws, rows, sh_deg, viewport=TILE, max_sh_deg=3, eye=EYE):
    """(GenericGaussianPointCloud, SplattingArgs): blend_ref.device_scene with the cloud's degree and a camera at `eye`."""
    w, h = viewport
    gpc = ws.GenericGaussianPointCloud.from_ply_rows(rows, sh_deg)
    cj = synth.look_at_camera(0, [float(v) for v in eye], [0.0, 0.0, 0.0], w, h, blend_ref.FOCAL, blend_ref.FOCAL)
    cam = ws.PerspectiveCamera.from_scene_camera(cj.position, cj.rotation, cj.fx, cj.fy, w, h)
    cam.fit_near_far(ws.Aabb([-1, -1, -1], [1, 1, 1]))
    return gpc, ws.SplattingArgs(camera=cam, viewport=(w, h), max_sh_deg=max_sh_deg)


def _line(k, opacity, sh_deg=3, eye=EYE, seed=0, length=1.0):
    """attrib_frames._stack(k, opacity) turned onto the optical axis of the camera at `eye` (its depths times `length`), a little
    off it sideways: k isotropic Gaussians that each cover the whole 32 x 32 viewport, every one of them in view.  Rest
    coefficients 0, as many as the degree has."""
    rows3 = _stack(k, opacity)
    rng = np.random.default_rng(seed + k)
    axis = -eye / np.linalg.norm(eye)
    xyz = length * rows3[:, 2:3].astype(np.float64) * axis[None, :] + rng.uniform(-0.02, 0.02, size=(k, 3))
    nrest = 3 * ((sh_deg + 1) ** 2 - 1)
    return synth._rows(xyz.astype(F), rows3[:, 6:9], np.zeros((k, nrest), F), rows3[:, 54], rows3[:, 55:58], rows3[:, 58:62])


def _cam32(args):
    """view_inv[12:15] of the camera uniform the library builds for these arguments: where K1 takes the SH direction from"""
    return np.array(list(args.camera.uniform(args.viewport).view_inv)[12:15], F)


def _xyz(pc):
    g, _ = pc.download()
    return np.ascontiguousarray(g[:, :12]).view(F).reshape(-1, 3)
