"""Per-Gaussian values drawn to pixel planes, and the winner-id plane (include/websplat.h "Rendering per-Gaussian values";
values.hip k_values).

   1. a one-hot channel equals k_contrib's sums, bitwise               6. the winner plane
   2. channels, strides and powers of two, bitwise                     7. frame edges, pitches, a skipped plane, empty tiles
   3. against float64 (tests/values_ref.py)                            8. no side effects
   4. the adjoint identity against accumulate_weighted                 9. the error cases
   5. tile lists at the staging boundaries"""
import ctypes as C

import numpy as np
import pytest

import attrib_ref
import contrib_ref
import scenes
import values_ref
from attrib_frames import VIEW, F, _c1_frame, _compressed, _ctx, _Frame, _ramp_checker, _stack_frame, _u32
from websplat import _lib as L

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
T_MIN = 2.0 ** -14


def _one_hot(n, picks):
    f = np.zeros((n, len(picks)), F)
    f[list(picks), np.arange(len(picks))] = 1
    return f


def _assert_plane_is_the_weights_of(o, q_j, m_j, what):
    """k_contrib's two results from the plane of a one-hot channel: the sum of the truncated q32 and, over the pixels whose q32 is
    not 0, the largest weight on its bits."""
    q32 = (o.astype(np.float64) * 4294967296.0).astype(np.uint64)   # (w < 1: exact product, truncating conversion)
    assert int(q32.sum(dtype=np.uint64)) == int(q_j), what
    counted = o[q32 != 0]
    top = counted.max() if counted.size else F(0.0)
    assert _u32(np.array([top], F))[0] == _u32(np.array([m_j], F))[0], what


CONFIGS = [{}, {"tile_qw": 2, "tile_qh": 2}, {"bin_request": 2}]
_ids = lambda cfgs: ["-".join(f"{k}{v}" for k, v in c.items()) or "default" for c in cfgs]  # noqa: E731


# ---- 1. one-hot == k_contrib -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids(CONFIGS))
def test_one_hot_channel_equals_the_contribution_sums_bitwise(ws, oracle, cfg):
    """A Gaussian is listed at most once per tile, fmaf(w, 1, 0) == w and fmaf(w, 0, acc) == acc: the plane of a one-hot channel
    holds the very weights k_contrib converts and reduces.  No tolerance."""
    c = _ctx(ws, **cfg)
    try:
        f = _c1_frame(ws, oracle, c)
        try:
            q, m = f.plain()
            drawn = np.nonzero(q > 0)[0]
            assert drawn.size > 1000
            picks = [int(drawn[np.argmax(q[drawn])]), int(drawn[np.argmin(q[drawn])])]
            faint = drawn[m[drawn] < T_MIN]
            if faint.size:
                picks.append(int(faint[0]))
            rest = np.setdiff1d(drawn, picks)
            picks += [int(j) for j in np.random.default_rng(7).choice(rest, 8 - len(picks), replace=False)]
            print(f"drawn {drawn.size} picks {picks} with max_weight below 2^-14: {int(faint.size)}")
            for half in (picks[:4], picks[4:]):
                planes = f.values(_one_hot(f.n, half))
                assert planes.shape == (VIEW[1], VIEW[0], 4)
                for ch, j in enumerate(half):
                    _assert_plane_is_the_weights_of(planes[..., ch], q[j], m[j], j)
        finally:
            f.close()
    finally:
        c.close()


# ---- 2. channels are independent ----------------------------------------------------------------------------------------------
def test_channels_strides_and_powers_of_two_bitwise(ws, oracle):
    c = _ctx(ws)
    try:
        f = _c1_frame(ws, oracle, c)
        try:
            vals = np.random.default_rng(2).uniform(-1, 1, size=(f.n, 4)).astype(F)
            together = f.values(vals)
            assert (together != 0).all(axis=-1).sum() > 1000
            for ch in range(4):
                alone = f.values(vals[:, ch])
                assert alone.shape == (VIEW[1], VIEW[0], 1)
                assert np.array_equal(_u32(alone[..., 0]), _u32(together[..., ch])), ch
            # a strided view: 3 channels in records of 32 B, the other five floats NaN
            packed3 = f.values(vals[:, :3])
            assert np.array_equal(_u32(packed3), _u32(together[..., :3]))
            wide = np.full((f.n, 8), np.nan, F)
            wide[:, :3] = vals[:, :3]
            d = c.malloc(wide.nbytes)
            try:
                c.upload(d, wide)
                f.r.render_values(f.pc, d, stride=32, channels=3)
                strided = f.r.download_values()["values"]
            finally:
                c.sync()
                c.free(d)
            assert np.array_equal(_u32(strided), _u32(packed3))
            # powers of two commute with every rounding here
            doubled = f.values(F(2.0) * vals)
            assert np.array_equal(_u32(doubled), _u32(F(2.0) * together))
        finally:
            f.close()
    finally:
        c.close()


# ---- 3. against float64 ------------------------------------------------------------------------------------------------------
def _compare(got, ref, fmax, min_nonzero, ch=0):
    tol = values_ref.tolerance(ref, fmax)
    d = np.abs(got.astype(np.float64) - ref["out"][..., ch])
    drawn = ref["n"] > 0
    und = int(((ref["und"] > 0) & drawn).sum())
    worst = np.unravel_index(int(np.argmax(d - tol)), d.shape)
    print(f"pixels {d.size} drawn {int(drawn.sum())} non-zero {int((got != 0).sum())} undecided {und} ({und / max(int(drawn.sum()), 1):.3%}) "
          f"below T_P {int((ref['T'] < contrib_ref.T_P).sum())}; max |d| {d.max():.3e}, worst excess {(d - tol)[worst]:.3e} at {worst} "
          f"(ref {ref['out'][..., ch][worst]:.6e}, tol {tol[worst]:.3e}, n {int(ref['n'][worst])})")
    assert (got != 0).sum() >= min_nonzero
    assert und < 0.01 * drawn.sum()
    assert np.all(d <= tol), f"{int((d > tol).sum())} pixels out of bound"


def _uniform_values(n, seed=3):
    return np.random.default_rng(seed).uniform(-1, 1, size=n).astype(F)


F64_CONFIGS = [{}, {"tile_qw": 2, "tile_qh": 2}, {"blend_split": 1}]
_REF = {}  # K1 and the depth sort do not depend on the tile configuration: one float64 walk serves the three


def _c1_ref(f, fv):
    frame = f.frame()
    hit = _REF.get("c1")
    if hit is None or not all(np.array_equal(hit[0][k], frame[k]) for k in ("splats", "sorted", "src_index")):
        hit = _REF["c1"] = (frame, values_ref.values_f64(frame, VIEW[0], VIEW[1], fv))
    return hit[1]


@pytest.mark.parametrize("cfg", F64_CONFIGS, ids=_ids(F64_CONFIGS))
def test_against_f64_c1(ws, oracle, cfg):
    c = _ctx(ws, **cfg)
    try:
        f = _c1_frame(ws, oracle, c, seed=0)
        try:
            fv = _uniform_values(f.n)
            got = f.values(fv)[..., 0]
            _compare(got, _c1_ref(f, fv), 1.0, 1000)
        finally:
            f.close()
    finally:
        c.close()


def test_against_f64_compressed(ws):
    c = _ctx(ws)
    try:
        gpc, args = _compressed(ws)
        f = _Frame(ws, c, gpc, args, compressed=True)
        try:
            fv = _uniform_values(f.n)
            got = f.values(fv)[..., 0]
            _compare(got, values_ref.values_f64(f.frame(), 400, 300, fv), 1.0, 1000)
        finally:
            f.close()
    finally:
        c.close()


# ---- 4. the adjoint identity --------------------------------------------------------------------------------------------------
def test_adjoint_identity_against_accumulate_weighted(ws, oracle):
    """<E, A f> on the pixels against <A^T E, f> on the Gaussians, from one prepared frame.  The weights w are bit-identical on both
    sides; per kept pair the left side rounds one fma (at most 2^-24 fmax), the right side rounds w E once (at most 2^-25) and
    truncates below 2^-32: |lhs - rhs| <= fmax K (2^-23 + 2^-32), K the kept pairs at pixels with E > 0."""
    c = _ctx(ws)
    try:
        f = _c1_frame(ws, oracle, c)
        try:
            E = _ramp_checker(*VIEW)
            fv = np.random.default_rng(4).uniform(0, 1, size=f.n).astype(F)
            out = f.values(fv)[..., 0]
            q, _ = f.weighted(E)
            lhs = float((E.astype(np.float64) * out.astype(np.float64)).sum())
            rhs = float((fv.astype(np.float64) * (q.astype(np.float64) / 4294967296.0)).sum())
            K = int(attrib_ref.attrib_f64(f.frame(), VIEW[0], VIEW[1], f.n, E)["kept"].sum())
            bound = 1.0 * K * (2.0 ** -23 + 2.0 ** -32)
            print(f"lhs {lhs:.9e} rhs {rhs:.9e} |lhs - rhs| {abs(lhs - rhs):.3e} relative {abs(lhs - rhs) / rhs:.3e} bound {bound:.3e} K {K}")
            assert rhs > 100 and K > 100_000
            assert abs(lhs - rhs) <= bound
        finally:
            f.close()
    finally:
        c.close()


# ---- 5. staging boundaries ----------------------------------------------------------------------------------------------------
BOUNDARY_CASES = [({}, k) for k in (1, 512, 513, 1025)] + [({"tile_qw": 2, "tile_qh": 2}, k) for k in (256, 257)]


@pytest.mark.parametrize("opacity", [0.002, 0.9], ids=["faint", "opaque"])
@pytest.mark.parametrize("cfg,k", BOUNDARY_CASES, ids=[f"{'2x2' if c else '4x4'}-{k}" for c, k in BOUNDARY_CASES])
def test_list_lengths_at_staging_boundaries(ws, cfg, k, opacity):
    """Tile lists of exactly k entries (STAGE = 512 at the 4x4 tile, 256 at 2x2); every quadrant walks.  Channel 0: f[j] = j + 1,
    against float64 with fmax = k.  Channel 1: one-hot at k - 1, the last slot of the last batch, against k_contrib bitwise.
    Opaque: every quadrant saturates inside the first batch; a wave looks at its pixels' T after every fourth record, so at most
    three records behind the first one whose pixels are ALL below T_MIN in front of it still add something -- one more for the gap
    between the device's f32 T and the reference's -- and channel 2, the indicator of everything from the eighth on, is exactly 0
    at every pixel (test_gpu_attrib.test_list_lengths_at_staging_boundaries' argument)."""
    c = _ctx(ws, bin_request=0, **cfg)
    try:
        f = _stack_frame(ws, c, k, opacity)
        try:
            assert int(f.r.tile_stats()["list_len"].max()) == k
            frame = f.frame()
            front = attrib_ref.attrib_f64(frame, 32, 32, k, np.ones((32, 32), F), watch=np.ones((32, 32), bool))["front"]
            saturated = np.nonzero(front < T_MIN)[0]   # (index = depth order: 0 is nearest)
            vals = np.zeros((k, 3), F)
            vals[:, 0] = np.arange(1, k + 1)
            vals[k - 1, 1] = 1
            if opacity > 0.5 and k > 1:
                assert saturated.size and saturated[0] + 8 < k
                vals[saturated[0] + 8:, 2] = 1
            got = f.values(vals)
            ref = values_ref.values_f64(frame, 32, 32, vals)
            # (how many pixels a layer keeps is the frame's business -- a cloud of one Gaussian keeps a dozen -- so only the opaque
            #  stacks, whose argument below needs every quadrant to saturate, are asked to cover the viewport)
            _compare(got[..., 0], ref, float(k), 1024 if opacity > 0.5 and k > 1 else 1)
            q, m = f.plain()
            _assert_plane_is_the_weights_of(got[..., 1], q[k - 1], m[k - 1], k - 1)
            print(f"k {k} opacity {opacity} last drawn {bool(q[k - 1])} first saturated {saturated[:1]}")
            if opacity < 0.5 or k == 1:
                assert q[k - 1] > 0 and (got[..., 1] > 0).any()
            else:
                assert q[k - 1] == 0 and not _u32(got[..., 2]).any()
        finally:
            f.close()
    finally:
        c.close()


# ---- 6. the winner ------------------------------------------------------------------------------------------------------------
def test_winner_in_the_second_batch(ws):
    """512 faint layers (each weighs at most 0.002) in front of one of opacity 0.9: where that one draws anything it outweighs all
    of them, and it sits in slot 0 of the second batch of the 4x4 tile.  Elsewhere the nearest layer is the heaviest."""
    c = _ctx(ws, bin_request=0)
    try:
        op = np.full(513, 0.002)
        op[512] = 0.9
        f = _stack_frame(ws, c, 513, op)
        try:
            assert int(f.r.tile_stats()["list_len"].max()) == 513
            planes, winner = f.values(_one_hot(513, [512]), winner=True)
            far = planes[..., 0] != 0
            assert far.sum() > 512
            assert np.all(winner[far] == 512) and np.all(winner[~far] == 0)
        finally:
            f.close()
    finally:
        c.close()


def test_winner_c1(ws, oracle):
    c = _ctx(ws)
    try:
        f = _c1_frame(ws, oracle, c)
        try:
            ones = np.ones(f.n, F)
            planes, winner = f.values(ones, winner=True)
            assert winner.dtype == np.uint32 and winner.shape == (VIEW[1], VIEW[0])
            # nothing under the pixel <=> nothing drawn
            nothing = winner == NONE
            assert np.array_equal(nothing, planes[..., 0] == 0)
            assert (~nothing).sum() > 1000 and winner[~nothing].max() < f.n
            assert np.unique(winner[~nothing]).size > 100
            # winner alone
            _, alone = f.values(None, winner=True)
            assert np.array_equal(alone, winner)
            # the device's winner weighs, in float64, what the heaviest pair weighs -- up to test 3's tolerance
            ref = values_ref.values_f64(f.frame(), VIEW[0], VIEW[1], ones, watch=winner.astype(np.int64))
            tol = values_ref.tolerance(ref, 1.0)
            short = ref["wmax"] - ref["wwatch"]
            same = int((winner.astype(np.int64) == ref["win"])[~nothing].sum())
            print(f"winners {int((~nothing).sum())} equal to the reference's {same}; largest shortfall {short[~nothing].max():.3e}, "
                  f"worst excess {(short - tol)[~nothing].max():.3e}")
            assert np.all(short[~nothing] <= tol[~nothing])
        finally:
            f.close()
    finally:
        c.close()


# ---- 7. frame edges, pitches, a skipped plane, empty tiles ----------------------------------------------------------------------
def _raw(ws, f, vals, planes, winner, pad_px, sentinel=0x7FC12345):
    """ws_renderer_render_values into caller's buffers of rows pad_px pixels longer than the viewport, pre-filled with `sentinel`;
    returns ({channel: H x (W + pad) uint32}, winner H x (W + pad) uint32 or None)."""
    c = f.c
    w, h = f.view
    row = w + pad_px
    fill = np.full((h, row), sentinel, np.uint32)
    ptrs = []

    def buf():
        d = c.malloc(fill.nbytes)
        ptrs.append(d)
        c.upload(d, fill)
        return d

    try:
        v = None
        if vals is not None:
            dv = c.malloc(vals.nbytes)
            ptrs.append(dv)
            c.upload(dv, vals)
            v = L.ws_values_view()
            v.d_values, v.stride_bytes, v.num_points, v.channels = dv, vals.shape[1] * 4, vals.shape[0], vals.shape[1]
        t = L.ws_value_targets()
        for ch in planes:
            t.plane[ch], t.pitch[ch] = buf(), row * 4
        if winner:
            t.winner, t.winner_pitch = buf(), row * 4
        ws.check(ws.lib.ws_renderer_render_values(f.r.handle, f.pc.handle, C.byref(v) if v is not None else None, C.byref(t), None))
        c.sync()
        return ({ch: c.download(t.plane[ch], (h, row), np.uint32) for ch in planes},
                c.download(t.winner, (h, row), np.uint32) if winner else None)
    finally:
        c.sync()
        for p in ptrs:
            c.free(p)


def test_odd_viewport_padded_pitch_and_a_skipped_plane(ws, oracle):
    c = _ctx(ws)
    try:
        f = _c1_frame(ws, oracle, c, viewport=(37, 29))
        try:
            w, h = 37, 29
            vals = np.random.default_rng(5).uniform(-1, 1, size=(f.n, 3)).astype(F)
            want, want_w = f.values(vals, winner=True)
            assert (want != 0).all(axis=-1).sum() > 100
            sentinel = 0x7FC12345
            for attempt in range(2):   # (reproducible: two calls give the same bits)
                got, got_w = _raw(ws, f, vals, (0, 2), True, 5, sentinel)    # plane[1] == NULL in the middle
                for ch in (0, 2):
                    assert np.array_equal(got[ch][:, :w], _u32(want[..., ch])), (attempt, ch)
                    assert np.all(got[ch][:, w:] == sentinel), (attempt, ch)
                assert np.array_equal(got_w[:, :w], want_w) and np.all(got_w[:, w:] == sentinel)
            # pitch == 4 x width exactly, one plane
            tight, _ = _raw(ws, f, vals, (1,), False, 0)
            assert np.array_equal(tight[1], _u32(want[..., 1]))
        finally:
            f.close()
    finally:
        c.close()


def test_empty_tiles_are_written(ws):
    """A 256 x 96 viewport around the 3-stack (sigma ~13 px around the centre): the tile columns at both ends list nothing, and
    their pixels read 0.0f / 0xFFFFFFFF over the sentinel."""
    c = _ctx(ws, bin_request=0)
    try:
        f = _stack_frame(ws, c, 3, 0.5, viewport=(256, 96))
        try:
            lens = f.r.tile_stats()["list_len"].reshape(3, 8)
            assert (lens == 0).any() and (lens > 0).any()
            vals = np.array([[1.0], [2.0], [4.0]], F)
            got, got_w = _raw(ws, f, vals, (0,), True, 3)
            empty = np.repeat(np.repeat(lens == 0, 32, axis=0), 32, axis=1)
            plane, winner = got[0][:, :256], got_w[:, :256]
            assert not plane[empty].any() and np.all(winner[empty] == NONE)
            assert np.array_equal(plane == 0, winner == NONE)            # ... and of listed tiles where no pair is kept
            assert (plane != 0).any() and set(np.unique(winner).tolist()) <= {0, 1, 2, NONE}
            assert np.all(got[0][:, 256:] == 0x7FC12345) and np.all(got_w[:, 256:] == 0x7FC12345)
            # winner only, over the same sentinel
            _, alone = _raw(ws, f, None, (), True, 3)
            assert np.array_equal(alone, got_w)
        finally:
            f.close()
    finally:
        c.close()


# ---- 8. no side effects ---------------------------------------------------------------------------------------------------------
def test_no_side_effects(ws, oracle):
    c = _ctx(ws)
    try:
        f = _c1_frame(ws, oracle, c)
        try:
            bg = (0.1, 0.2, 0.3, 0.4)
            f.r.render(f.pc, background=bg)
            before = f.r.download_target().copy()
            q0, m0 = f.plain()
            errors = f.r.errors()
            vals = np.random.default_rng(6).uniform(-1, 1, size=(f.n, 4)).astype(F)
            planes, winner = f.values(vals, winner=True)
            assert (planes != 0).any() and (winner != NONE).any()
            assert f.r.errors() == errors
            f.r.render(f.pc, background=bg)
            after = f.r.download_target().copy()
            q1, m1 = f.plain()
            assert (before[..., 3] > 0.5).mean() > 0.05
            assert np.array_equal(_u32(before), _u32(after))
            assert np.array_equal(q0, q1) and np.array_equal(_u32(m0), _u32(m1)) and (q0 > 0).sum() > 1000
        finally:
            f.close()
    finally:
        c.close()


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------
def test_error_cases(ws, oracle):
    def code_of(fn):
        with pytest.raises(ws.WebSplatError) as e:
            fn()
        assert "ws_renderer_render_values" in str(e.value)
        return e.value.code

    c = _ctx(ws)
    try:
        sc = scenes.c1(ws, oracle, n=10_000, viewport=VIEW)
        pc = ws.PointCloud(c, sc.gpc)
        other = pc.subset(np.arange(0, pc.num_points(), 2, dtype=np.uint32))
        n = pc.num_points()
        r = ws.GaussianRenderer(c, "rgba32float", 3, False)
        ones = np.ones(n, F)
        d = c.malloc((VIEW[0] + 1) * VIEW[1] * 4 + 16)
        dv = c.malloc(n * 4)
        c.upload(dv, ones)

        def raw(pitch, ptr=None, num_points=n):
            v = L.ws_values_view()
            v.d_values, v.stride_bytes, v.num_points, v.channels = dv, 4, num_points, 1
            t = L.ws_value_targets()
            t.plane[0], t.pitch[0] = d if ptr is None else ptr, pitch
            return ws.lib.ws_renderer_render_values(r.handle, pc.handle, C.byref(v), C.byref(t), None)

        try:
            # not prepared; prepared without contributions
            r.enable_contrib(True)
            assert code_of(lambda: r.render_values(pc, ones)) == L.WS_ERR_STATE
            r.enable_contrib(False)
            r.prepare(pc, sc.args)
            assert code_of(lambda: r.render_values(pc, ones)) == L.WS_ERR_STATE
            assert code_of(lambda: r.render_values(pc, None, winner=True)) == L.WS_ERR_STATE
            r.enable_contrib(True)
            r.prepare(pc, sc.args)
            # prepared for another cloud; values laid out for another number of points
            assert code_of(lambda: r.render_values(other, np.ones(other.num_points(), F))) == L.WS_ERR_STATE
            assert code_of(lambda: r.render_values(pc, np.ones(n - 1, F))) == L.WS_ERR_INVALID
            assert raw(VIEW[0] * 4, num_points=n + 1) == L.WS_ERR_INVALID
            # the pitch against the viewport
            assert raw(VIEW[0] * 4) == L.WS_OK
            assert raw(VIEW[0] * 4 + 4) == L.WS_OK
            assert raw(VIEW[0] * 4 - 4) == L.WS_ERR_INVALID and b"pitch" in ws.lib.ws_last_error()
            assert raw(VIEW[0] * 4, ptr=d + 2) == L.WS_ERR_INVALID
            # nothing asked for
            assert code_of(lambda: r.render_values(pc, None, winner=False)) == L.WS_ERR_INVALID
        finally:
            c.sync()
            c.free(d)
            c.free(dv)
            r.close()
            other.close()
            pc.close()
        # a context that stops its frames early
        cut = _ctx(ws, debug_cut=2)
        try:
            pc2 = ws.PointCloud(cut, sc.gpc)
            r2 = ws.GaussianRenderer(cut, "rgba32float", 3, False)
            try:
                r2.enable_contrib(True)
                r2.prepare(pc2, sc.args)
                assert code_of(lambda: r2.render_values(pc2, ones, winner=True)) == L.WS_ERR_UNSUPPORTED
            finally:
                r2.close()
                pc2.close()
        finally:
            cut.close()
    finally:
        c.close()
