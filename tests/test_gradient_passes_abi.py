"""CPU pins of what the gradient family's entry points say, and in which order, about a descriptor alone (csrc/api_attrib.cpp):
ws_renderer_accumulate_gradient, _sh_gradient, _geometry_gradient, ws_debug_geometry_stage_a and ws_renderer_accumulate_removal.
The descriptor is judged before the handles, so no device is needed: the handles are null throughout.  Every descriptor here
carries two faults that are neighbours in the order of refusals, and the whole text of the earlier one is what comes back, the
entry point's own name in front."""
import ctypes as C

import pytest

INF, NAN = float("inf"), float("nan")
MUL16 = "pointer and {}_pitch_bytes must be multiples of 16"
# (entry point, its descriptor, the name of its second scale)
GRADIENT_ENTRIES = (("ws_renderer_accumulate_gradient", "ws_gradient_params", "opacity_scale"),
                    ("ws_renderer_accumulate_sh_gradient", "ws_gradient_params", "opacity_scale"),
                    ("ws_renderer_accumulate_geometry_gradient", "ws_geometry_params", "geometry_scale"),
                    ("ws_debug_geometry_stage_a", "ws_geometry_params", "geometry_scale"))


@pytest.fixture(scope="module")
def ptr():
    """host memory standing in for a device pointer, 16-B aligned: nothing dereferences it"""
    buf = (C.c_float * 64)()
    yield (C.addressof(buf) + 15) // 16 * 16


def _refusal(ws, entry, p):
    from websplat import _lib as L
    rc = getattr(ws.lib, entry)(None, None, None, C.byref(p) if p is not None else None, None)
    assert rc == L.WS_ERR_INVALID
    return ws.lib.ws_last_error().decode()


@pytest.mark.parametrize("entry,struct,second", GRADIENT_ENTRIES, ids=[e[0] for e in GRADIENT_ENTRIES])
def test_gradient_descriptor_refusals_in_order(ws, ptr, entry, struct, second):
    from websplat import _lib as L

    def refusal(**faults):
        p = getattr(L, struct)()
        p.scale = 1.0
        setattr(p, second, 1.0)
        p.d_grad, p.grad_pitch_bytes = ptr, 64
        for name, v in faults.items():
            if name in ("background", "reserved"):
                for i, x in enumerate(v):
                    getattr(p, name)[i] = x
            else:
                setattr(p, second if name == "second" else name, v)
        return _refusal(ws, entry, p)

    bad_base = dict(d_base=ptr + 4, base_pitch_bytes=64)
    # the order of refusals, each with the one behind it in the same descriptor
    steps = [("reserved words must be zero", dict(reserved0=1)),
             ("reserved words must be zero", dict(reserved=(0, 0, 0, 1))),
             ("scale must be finite and above 0", dict(scale=0.0)),
             (second + " must be finite and above 0", dict(second=NAN)),
             ("background must be finite", dict(background=(0.0, INF, 0.0))),
             ("null d_grad", dict(d_grad=None, grad_pitch_bytes=72)),
             ("d_grad: " + MUL16.format("grad"), dict(d_grad=ptr + 8)),
             ("d_base: " + MUL16.format("base"), bad_base),
             ("null argument", {})]
    assert _refusal(ws, entry, None) == entry + ": null params"
    for (text, fault), (_, behind) in zip(steps, steps[1:]):
        assert refusal(**fault) == entry + ": " + text                     # alone
        assert refusal(**{**behind, **fault}) == entry + ": " + text, behind   # and in front of its neighbour
    assert refusal() == entry + ": null argument"
    assert refusal(d_grad=ptr, grad_pitch_bytes=72, **bad_base) == entry + ": d_grad: " + MUL16.format("grad")   # (the pitch alone)
    assert refusal(d_base=ptr, base_pitch_bytes=72) == entry + ": d_base: " + MUL16.format("base")
    # the second scale is judged under its own name, and `scale` in front of it under its own
    other = "opacity_scale" if second == "geometry_scale" else "geometry_scale"
    for bad in (0.0, -1.0, INF, NAN):
        assert other not in refusal(second=bad) and refusal(second=bad).startswith(entry + ": " + second + " must")
        assert refusal(scale=bad, second=bad) == entry + ": scale must be finite and above 0"


def test_removal_descriptor_refusals_in_order(ws, ptr):
    from websplat import _lib as L
    entry = "ws_renderer_accumulate_removal"
    keep = []

    def plane(pointer=ptr, pitch=64, scale=1.0, bias=0.0):
        v = L.ws_plane_view()
        v.d_values, v.row_pitch_bytes, v.scale, v.bias = pointer, pitch, scale, bias
        keep.append(v)
        return C.pointer(v)

    def refusal(**faults):
        p = L.ws_removal_params()
        p.kind, p.scale = L.WS_ERROR_SQ, 1.0
        for name, v in faults.items():
            if name in ("background", "reserved"):
                for i, x in enumerate(v):
                    getattr(p, name)[i] = x
            else:
                setattr(p, name, v)
        return _refusal(ws, entry, p)

    # (kind and weight are one member each: where two neighbours are faults of the same member, the later one is paired with
    # the refusal in front of both instead)
    steps = [("reserved words must be zero", dict(reserved=(0, 1, 0, 0))),
             ("kind WS_ERROR_DSSIM has no removal effect (sq or abs)", dict(kind=L.WS_ERROR_DSSIM)),
             ("scale must be finite and above 0", dict(scale=-1.0)),
             ("background must be finite", dict(background=(NAN, 0.0, 0.0))),
             ("weight: null d_values", dict(weight=plane(pointer=None))),
             ("d_base: " + MUL16.format("base"), dict(d_base=ptr + 4, base_pitch_bytes=64)),
             ("null argument", {})]
    assert _refusal(ws, entry, None) == entry + ": null params"
    for (text, fault), (_, behind) in zip(steps, steps[1:]):
        assert refusal(**fault) == entry + ": " + text
        assert refusal(**{**behind, **fault}) == entry + ": " + text, behind
    bad_base = dict(d_base=ptr, base_pitch_bytes=72)
    assert refusal(reserved=(1, 0, 0, 0), kind=7) == entry + ": reserved words must be zero"
    assert refusal(kind=7, scale=0.0) == entry + ": unknown kind"
    assert refusal(background=(0.0, 0.0, INF), weight=plane(scale=NAN)) == entry + ": background must be finite"
    # within the weight: its pointer, then its two numbers, then its alignment; all of it in front of d_base
    assert refusal(weight=plane(pointer=None, scale=NAN, pitch=66)) == entry + ": weight: null d_values"
    assert refusal(weight=plane(bias=INF, pitch=66), **bad_base) == entry + ": weight: scale and bias must be finite"
    assert refusal(weight=plane(pitch=66), **bad_base) == entry + ": weight: plane pointer and row pitch must be multiples of 4"
    assert refusal(weight=plane(pointer=ptr + 2), **bad_base) == entry + ": weight: plane pointer and row pitch must be multiples of 4"
    assert refusal(**bad_base) == entry + ": d_base: " + MUL16.format("base")
    assert refusal(kind=L.WS_ERROR_ABS, weight=plane(), d_base=ptr, base_pitch_bytes=64) == entry + ": null argument"
