"""tests/k1_edges.py on the CPU: the cases are what they are named for.  Every threshold window holds both verdicts under the
oracle and agrees with float64 away from the threshold; K1 and K1c part at the exact points; every maths case reaches its
branch (asserted from k1_f64's intermediates); and the oracle alone meets the float64 caps tests/test_gpu_k1_edges.py then
holds the device to.  No GPU."""
import numpy as np
import pytest

import k1_edges as ke

FORMS = [(cam, vp) for cam in ke.CAMERAS for vp in ke.VIEWPORTS]
FORM_IDS = [f"{cam}-{vp[0]}x{vp[1]}" for cam, vp in FORMS]
NAN_KEY = 0x7FC00000


def _halves(frame, cl, name):
    """The ten f16 bit patterns of special `name` in a frame, or None when it is not visible."""
    slot = np.nonzero(np.asarray(frame["src_index"]) == cl.index[name])[0]
    if not len(slot):
        return None
    return np.ascontiguousarray(frame["splats"]).view(np.uint16).reshape(-1, 10)[slot[0]]


def _is_nan16(h):
    return (h & 0x7FFF) > 0x7C00


# ---- threshold windows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ke.LAYOUTS)
@pytest.mark.parametrize("cam,vp", FORMS, ids=FORM_IDS)
def test_frustum_windows_straddle_their_threshold(ws, oracle, cam, vp, layout):
    cl = ke.window_cloud(ws, oracle, "frustum", cam, vp, layout)
    fr = cl.oracle_frame(oracle)
    got = ke.window_verdicts(cl, fr["src_index"])
    f = cl.f64(oracle)
    far = np.abs(np.arange(2 * ke.HALF + 1) - ke.HALF) > 8
    assert len(cl.info["windows"]) == 10
    vis = np.zeros(cl.n, dtype=bool)
    vis[fr["src_index"]] = True
    for w in cl.info["windows"]:
        idx = [cl.index[nm] for nm in w.names]
        want = ~f["culled"][idx]
        v = got[w.name]
        assert len(np.unique(w.values)) == 33 and np.all(np.diff(w.values) > 0), w.name
        assert v.any() and not v.all(), (w.name, "one verdict only", v)
        assert want.any() and not want.all(), (w.name, "float64 sees one verdict only")
        # A window that f32 decides once changes its verdict once, and then agrees with float64 outside +-8 floats.  The far
        # plane can be another matter: clip z and w are both near zfar and differ by (cz - zfar) * znear / (zfar - znear), less
        # than their own spacing over tens of floats of cz, so z / w alternates between 1 and its neighbours from one float to
        # the next through the whole window.  Only a far window that DOES alternate is excused from the +-8 rule; there both
        # verdicts are present (above) and what float64 decides holds at the guard points, 256 floats out (below).
        flips = int(np.count_nonzero(v[1:] != v[:-1]))
        if not (w.name == "far" and flips >= 3):
            assert flips == 1, (w.name, v)
            assert np.array_equal(v[far], want[far]), (w.name, v, want)
        g = [cl.index[nm] for nm in w.guards]
        assert vis[g[0]] != vis[g[1]] and np.array_equal(vis[g], ~f["culled"][g]), (w.name, "guards")
        others = np.delete(np.abs(f["margins"][idx]), w.margin, axis=1)
        assert np.abs(f["margins"][idx, w.margin]).max() * 10 < others.min(), (w.name, "another threshold is as close")
    for nm in ("w_zero", "w_zero_off", "w_neg", "w_neg_off"):
        assert not vis[cl.index[nm]] and f["culled"][cl.index[nm]], nm
    assert f["w"][cl.index["w_neg"]] < 0
    if cam == "axis":
        assert f["w"][cl.index["w_zero"]] == 0
    assert vis[cl.ordinary].sum() > 0.9 * len(cl.ordinary)          # the rows between them are ordinary, visible Gaussians
    assert np.array_equal(vis[cl.ordinary], ~f["culled"][cl.ordinary])


@pytest.mark.parametrize("layout", ke.LAYOUTS)
@pytest.mark.parametrize("cam,vp", FORMS, ids=FORM_IDS)
def test_box_windows_are_exact_and_closed(ws, oracle, cam, vp, layout):
    cl = ke.window_cloud(ws, oracle, "box", cam, vp, layout)
    fr = cl.oracle_frame(oracle)
    got = ke.window_verdicts(cl, fr["src_index"])
    f = cl.f64(oracle)
    assert len(cl.info["windows"]) == 6
    for w in cl.info["windows"]:
        idx = [cl.index[nm] for nm in w.names]
        v = got[w.name]
        assert np.array_equal(v, ~f["culled"][idx]), w.name              # a comparison of two floats: nothing rounds
        assert v[ke.HALF] and v.sum() == ke.HALF + 1, (w.name, v)       # the face itself is kept: the box is closed
        assert f["margins"][idx[ke.HALF], w.margin] == 0.0, w.name


def test_k1_and_k1c_part_at_the_exact_points(ws, oracle):
    """clip z / w == 0 exactly at camera depth znear = 0.5, and == 1 exactly at some floats under zfar = 8: K1 culls both
    (<=, >=), K1c keeps both (<, >)."""
    vp = (640, 480)
    k1 = ke.window_cloud(ws, oracle, "frustum", "axis", vp, "uncompressed")
    k1c = ke.window_cloud(ws, oracle, "frustum", "axis", vp, "compressed")
    assert np.array_equal(k1.xyz[[k1.index[n] for n in k1.index]], k1c.xyz[[k1c.index[n] for n in k1.index]])
    v1 = ke.window_verdicts(k1, k1.oracle_frame(oracle)["src_index"])
    vc = ke.window_verdicts(k1c, k1c.oracle_frame(oracle)["src_index"])
    near = next(w for w in k1.info["windows"] if w.name == "near")
    at = np.nonzero(near.values == np.float32(ke.AXIS_ZNEAR))[0]
    assert len(at) == 1
    assert k1.f64(oracle)["margins"][k1.index[near.names[at[0]]], 6] == 0.0          # clip z is 0 in float64 as well
    assert not v1["near"][at[0]] and vc["near"][at[0]]
    assert np.array_equal(np.delete(v1["near"], at[0]), np.delete(vc["near"], at[0]))
    apart = v1["far"] != vc["far"]
    assert apart.any() and np.all(vc["far"][apart]) and not np.any(v1["far"][apart])    # z / w == 1: only K1c keeps them
    for nm in v1:
        if nm not in ("near", "far"):
            assert np.array_equal(v1[nm], vc[nm]), nm


# ---- maths cases ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maths(ws, oracle):
    cl = ke.maths_cloud(ws)
    out = {}
    for frame, kw in ke.MATHS_FRAMES.items():
        args = cl.with_args(ws, **kw)
        out[frame] = (cl.f64(oracle, args), cl.oracle_frame(oracle, args))
    return cl, out


def test_every_maths_case_reaches_its_branch(maths):
    cl, fr = maths
    i = cl.index
    f, o = fr["k0"]
    for nm in ("iso_on_axis", "wide_on_axis", "zero_cov", "tiny_iso"):
        assert np.array_equal(f["dv"][i[nm]], [0.0, 0.0]) and np.array_equal(f["e"][i[nm]], [1.0, 0.0]), nm     # the (1, 0) default
    assert f["dv"][i["tall_on_axis"]][0] == 0.0 and np.array_equal(f["e"][i["tall_on_axis"]], [0.0, 1.0])
    assert np.array_equal(f["cov2d"][i["wide_on_axis"]], [25.0, 0.0, 6.25])
    for nm in ("needle", "tiny_iso", "zero_cov"):                                                               # the 0.1 clamp
        assert f["lambda2_raw"][i[nm]] < ke.C_0P1 and f["lambda2"][i[nm]] == ke.C_0P1, nm
    assert f["lambda2_raw"][i["iso_on_axis"]] > ke.C_0P1
    assert f["lambda1"][i["zero_cov"]] == 0.0 and np.array_equal(f["v1"][i["zero_cov"]], [0.0, 0.0])
    h = _halves(o, cl, "zero_cov")
    assert h[0] == 0 and (h[1] & 0x7FFF) == 0 and (h[2] & 0x7FFF) == 0 and h[3] != 0                       # v1 == (0, 0), v2 is not
    h = _halves(o, cl, "iso_on_axis")
    assert h[0] != 0 and (h[1] & 0x7FFF) == 0 and (h[2] & 0x7FFF) == 0 and h[3] & 0x8000                   # v1 = (s1, 0), v2 = (0, -s2)

    f, o = fr["k03"]
    assert f["lambda2"][i["zero_cov"]] == f["lambda2_raw"][i["zero_cov"]] == np.float64(np.float32(0.3))
    assert f["lambda1"][i["negative_diag"]] < 0 and np.isnan(f["v1"][i["negative_diag"]]).all()
    assert _is_nan16(_halves(o, cl, "negative_diag")[0:2]).all()
    v = f["v1"][i["huge"]] / 640.0, f["v2"][i["huge"]] / 480.0
    assert 172 < v[0][0] < 174 and -232 < v[1][1] < -230                                                      # in NDC halves
    assert 0 < f["cov2d"][i["subnormal_cov"]][0] < 0.01
    assert abs(f["colour_raw"][i["col_exact_zero"]]).max() < 1e-6 and not _halves(o, cl, "col_exact_zero")[6:9].any()
    assert (f["colour_raw"][i["col_negative"]] < -0.3).all() and not _halves(o, cl, "col_negative")[6:9].any()
    assert (f["colour_raw"][i["col_overflow"]] > ke.F16_MAX).all() and (_halves(o, cl, "col_overflow")[6:9] == 0x7C00).all()
    for nm, bits in (("op_zero", 0x0000), ("op_one", 0x3C00), ("op_1p5", 0x3E00), ("op_subnormal", 0x0001)):
        assert _halves(o, cl, nm)[9] == bits, nm
    assert _is_nan16(_halves(o, cl, "op_nan")[9])
    for nm in ("nan_x", "nan_y", "nan_z"):                    # every comparison with a NaN is false: not culled
        assert not f["culled"][i[nm]], nm
        h = _halves(o, cl, nm)
        # v1 and the centre are NaN; v2 = (0, -s2) is not: fmax(NaN, 0.1) = 0.1 and a NaN length takes the (1, 0) default
        assert h is not None and _is_nan16(h[[0, 1, 4, 5]]).all() and not _is_nan16(h[2:4]).any(), nm
        assert o["keys"][np.nonzero(o["src_index"] == i[nm])[0][0]] == NAN_KEY, nm
    for nm in ("inf_x", "neg_inf_x", "inf_z"):
        assert f["culled"][i[nm]] and _halves(o, cl, nm) is None, nm
    for nm in ("nan_cov", "inf_cov"):
        h = _halves(o, cl, nm)
        assert not f["culled"][i[nm]] and _is_nan16(h[0:4]).any() and not _is_nan16(h[4:6]).any(), nm
    h = _halves(o, cl, "nan_sh")
    assert h[7] == 0 and h[6] != 0 and np.isnan(f["colour_raw"][i["nan_sh"]][1])                            # fmax(0, NaN) == 0

    f, o = fr["mip"]
    assert f["det_0"][i["zero_cov"]] <= ke.C_1EM6 and f["coef"][i["zero_cov"]] == 0.0                         # mip_cut
    assert _halves(o, cl, "zero_cov")[9] == 0x0000
    assert 0.5 < f["coef"][i["iso_on_axis"]] < 0.99                                                            # mip_mid
    f, o = fr["scaling_zero"]
    assert not f["cov2d"][~np.isnan(f["cov2d"]).any(axis=1)].any()
    f, o = fr["deg1"]
    assert abs(f["colour_raw"][i["col_exact_zero"]]).max() < 1e-6


def _finite_names(frame):
    skip = () if frame in ("k0", "scaling_zero") else ("wide_on_axis", "needle")        # their axis is rounding noise unless exact
    return [n for n in ke.FINITE if n not in skip]


def _oracle_deviation(cl, f, o, names, viewport):
    rows = np.array([cl.index[n] for n in names])
    slots = np.array([np.nonzero(np.asarray(o["src_index"]) == r)[0][0] for r in rows])
    fields = {k: v[slots] for k, v in ke.splat_fields(o["splats"], viewport).items()}
    return ke.f64_deviation(fields, f, rows)


def test_oracle_meets_the_float64_caps(maths):
    """The caps of tests/k1_edges.py (sigma within 2^-9 of its largest entry; centre, colour, opacity within half an f16 ulp of
    the float64 value plus 2e-6) are conditions the cases were chosen for, not measurements: the f32 oracle alone meets them."""
    cl, fr = maths
    worst = {}
    for frame, (f, o) in fr.items():
        dev = _oracle_deviation(cl, f, o, _finite_names(frame), cl.viewport)
        for q, x in dev.items():
            worst[q] = max(worst.get(q, 0.0), x)
        assert all(x <= 1.0 for x in dev.values()), (frame, dev)
    print("oracle / float64, as a fraction of the cap:", worst)


def test_compressed_maths_cases(ws, oracle):
    cl = ke.maths_cloud(ws, "compressed")
    i = cl.index
    for kw in ({}, {"kernel_size": 0.0}):
        args = cl.with_args(ws, **kw)
        f, o = cl.f64(oracle, args), cl.oracle_frame(oracle, args)
        dev = _oracle_deviation(cl, f, o, ke.COMPRESSED_FINITE if kw else ("iso_on_axis",), cl.viewport)
        assert all(x <= 1.0 for x in dev.values()), (kw, dev)
    # kernel_size 0: K1c clamps the RADIUS, so lambda2 = mid - 0.1 goes negative where K1 would have clamped it to 0.1
    for nm in ("tiny_iso", "zero_cov"):
        assert f["lambda2"][i[nm]] < 0 and np.isnan(f["v2"][i[nm]]).any(), nm
        assert _is_nan16(_halves(o, cl, nm)[2:4]).any(), nm
    assert f["lambda2"][i["needle"]] > 0 and f["lambda2"][i["needle"]] == f["lambda2_raw"][i["needle"]] < ke.C_0P1


def test_overflow_and_hostile_clouds(ws, oracle):
    for vp in ke.VIEWPORTS:
        cl = ke.overflow_cloud(ws, vp)
        f, o = cl.f64(oracle), cl.oracle_frame(oracle)
        for nm in cl.index:
            h = _halves(o, cl, nm)
            if nm.startswith("f16_overflow"):
                assert (np.abs(f["v1"][cl.index[nm]]) / np.array(vp) > ke.F16_MAX).any(), nm
                assert ((h[0:4] & 0x7FFF) >= 0x7C00).any(), nm                  # an axis half is inf (or NaN)
            else:
                assert _is_nan16(h[[0, 1, 4, 5]]).all(), nm
        vis = np.zeros(cl.n, dtype=bool)
        vis[o["src_index"]] = True
        assert vis[cl.ordinary].sum() > 0.9 * len(cl.ordinary)
        cl = ke.hostile_cloud(ws, vp)
        o = cl.oracle_frame(oracle)
        for nm in cl.index:
            h = _halves(o, cl, nm)
            assert h is not None, nm
            if nm.startswith("zero_cov"):
                assert h[0] == 0 and (h[1] & 0x7FFF) == 0, nm
            else:
                assert ((h[0:4] & 0x7FFF) >= 0x7C00).any(), nm


def test_one_hot_sh(ws, oracle):
    cl = ke.one_hot_cloud(ws)
    for deg in range(4):
        args = cl.with_args(ws, max_sh_deg=deg)
        f = cl.f64(oracle, args)
        want = ke.one_hot_expected(deg)
        for d in range(3):
            for k in range(16):
                for ch in range(3):
                    got = f["colour"][cl.index[f"onehot_d{d}_k{k}_c{ch}"]]
                    assert np.allclose(got, want[d, k, ch], rtol=0, atol=1e-12), (deg, d, k, ch)
                    if k >= (deg + 1) ** 2:
                        assert np.array_equal(got, [0.5, 0.5, 0.5])            # above the active degree: nothing


# ---- fade-in -------------------------------------------------------------------------------------------------------------------
def test_fade_cases(ws, oracle):
    cl = ke.fade_cloud(ws)
    names = list(ke.FADE_POINTS)
    rows = [cl.index[n] for n in names]
    seen = set()
    for wt in ke.FADE_WALLTIMES:
        args = cl.with_args(ws, walltime=wt)
        f, o = cl.f64(oracle, args), cl.oracle_frame(oracle, args)
        for n, r in zip(names, rows):
            dd = ke.FADE_POINTS[n][1]
            assert f["dd"][r] == dd, n
            t = wt - dd
            kind = "zero" if wt <= dd else ("rising" if t < 1 else "done")
            if wt == dd and wt > 0:
                kind = "equal"                                              # strict >: scale 0
            seen.add(kind)
            assert (f["scale_mod"][r] == 0) == (kind in ("zero", "equal")), (n, wt)
            assert (f["scale_mod"][r] == 1) == (kind == "done"), (n, wt)
        dev = _oracle_deviation(cl, f, o, names, cl.viewport)
        assert all(x <= 1.0 for x in dev.values()), (wt, dev)
    assert seen == {"zero", "equal", "rising", "done"}


def test_oracle_on_the_centre_outside_cloud(ws, oracle):
    """The reference behaviour: with the declared centre far outside the bbox, dd is near 50, the Gaussians are still at scale 0
    at walltime 11 and 12 and fully there at 100."""
    cl = ke.outside_cloud(ws)
    fr = {wt: cl.oracle_frame(oracle, cl.with_args(ws, walltime=wt)) for wt in ke.OUTSIDE_WALLTIMES}
    f = cl.f64(oracle, cl.with_args(ws, walltime=12.0))
    assert 12.0 < f["dd"].min() and f["dd"].max() < 100.0 - 1.0
    assert np.array_equal(fr[11.0]["splats"], fr[12.0]["splats"])
    assert np.array_equal(fr[12.0]["src_index"], fr[100.0]["src_index"]) and not np.array_equal(fr[12.0]["splats"], fr[100.0]["splats"])
    rows = [cl.index[f"corner_{k}"] for k in range(8)]
    assert not f["scale_mod"][rows].any()
    cc = ke.corner_cloud(ws)
    f = cc.f64(oracle, cc.with_args(ws, walltime=10.999))
    assert np.allclose(f["dd"][[cc.index[f"corner_{k}"] for k in range(8)]], 5.0) and (f["scale_mod"] == 1).all()
