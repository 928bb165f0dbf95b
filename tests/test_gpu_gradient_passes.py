"""GPU pin of how the gradient family's four public calls are sequenced (csrc/api_attrib.cpp ws_internal_gradient_passes): the one
timer label each call leaves, which scripts/*_cost.py select on, and whether the call counts a frame in its accumulator.  What the
launches compute is test_gpu_gradient's, test_gpu_sh_gradient's and test_gpu_geometry's."""
import pytest

from attrib_frames import BG, _ctx, _Frame
from gradient_frames import signed_ramp
from sh_frames import _line, _oblique

pytestmark = pytest.mark.gpu

VIEW = (48, 40)   # not a multiple of the 32-px tile either way: 2 x 2 tiles, the right column and the lower row partly outside
# (call, accumulator, the second scale's name, extra arguments, label, frames added)
CALLS = (("accumulate_gradient", "Grad", "opacity_scale", {}, "k_removal_base+k_gradient", 1),
         ("accumulate_sh_gradient", "ShGrad", "opacity_scale", {}, "k_removal_base+k_gradient+k_sh_spread", 1),
         ("accumulate_geometry_gradient", "GeomGrad", "geometry_scale", {}, "k_removal_base+k_geometry+k_geom_spread", 1),
         ("accumulate_geometry_gradient", "GeomGrad", "geometry_scale", {"_stage_a_only": True}, "k_removal_base+k_geometry", 0))


def test_each_call_leaves_its_label_and_counts_its_frame(ws):
    c = _ctx(ws)
    try:
        f = _Frame(ws, c, *_oblique(ws, _line(3, 0.3), 3, viewport=VIEW))   # three Gaussians that each cover the viewport
        try:
            assert f.n == 3 and f.view == VIEW and f.r.frame_stats()["num_visible"] == 3
            plane = signed_ramp(*VIEW)
            f.r.enable_timers(2)   # (behind prepare(): the marks hold the calls' launches only)
            labels = []
            for call, kind, second, extra, label, added in CALLS:
                acc = getattr(ws, kind)(c, f.n, 3) if kind == "ShGrad" else getattr(ws, kind)(c, f.n)
                try:
                    for n in (1, 2):   # twice: the count goes on from where it was
                        before = acc.frames
                        getattr(f.r, call)(f.pc, acc, plane, background=BG, **{second: 0.25}, **extra)
                        labels.append(label)
                        assert [name for name, _ in f.r.kernel_times()] == labels
                        assert acc.frames - before == added and acc.frames == n * added
                    if extra:      # the sums stayed in the scratch, which the spread would have cleared
                        assert acc._debug_scratch().any()
                        acc._debug_clear_scratch()
                        assert not any(a.any() for a in acc.download().values())
                    else:
                        got = acc.download()
                        assert any(a.any() for a in (got.values() if isinstance(got, dict) else (got,)))
                finally:
                    acc.close()
        finally:
            f.close()
    finally:
        c.close()
