"""tests/ply_rows.py without a device: the numpy restatement of the PLY row decode equals the oracle (wso_ply_rows_convert) and
the host twin (ws_ply_rows_convert) on every edge cloud, every cloud reaches the edge it is named for, no committed row is
undecided between two f64 exp implementations, and the f64-exp and libm forms stay inside the envelope that
tests/test_gpu_ply_decode.py states for the device."""
import numpy as np
import pytest

import ply_rows as pr
import scenes

F = np.float32
DEGREES = (0, 1, 2, 3)
ALL = [(name, d) for name in pr.CLOUDS for d in DEGREES]
IDS = [f"{name}-deg{d}" for name, d in ALL]


def _opacity(name, d, exp="f64"):
    return pr.computed_halves(pr.reference(name, d, exp)[0])[:, 0]


def _cov(name, d, exp="f64"):
    return pr.computed_halves(pr.reference(name, d, exp)[0])[:, 1:]


def _subnormal(h):
    return ((h & 0x7C00) == 0) & ((h & 0x03FF) != 0)


@pytest.mark.parametrize("name,d", ALL + [("bulk", d) for d in DEGREES], ids=IDS + [f"bulk-deg{d}" for d in DEGREES])
def test_restatement_equals_the_oracle_and_the_host_twin(ws, oracle, name, d):
    rows = pr.bulk_rows(d) if name == "bulk" else pr.cloud(name, d)
    g, s = pr.reference(name, d, "libm")
    twin = ws.GenericGaussianPointCloud.from_ply_rows(rows, d)
    for who, (g0, s0) in (("oracle", oracle.ply_rows_convert(rows, d)), ("host twin", (twin.gaussians, twin.sh_coefs))):
        bad, bad_sh, fixed = pr.compare(g, s, g0, s0)
        assert fixed, who
        assert not bad.any(), (who, np.argwhere(bad)[:8].tolist())
        assert not bad_sh.any(), (who, np.argwhere(bad_sh)[:8].tolist())


@pytest.mark.parametrize("name,d", ALL + [("bulk", d) for d in DEGREES], ids=IDS + [f"bulk-deg{d}" for d in DEGREES])
def test_no_row_is_undecided(name, d):
    """A condition on the committed clouds and seeds (about 1e-8 per exp): were a row undecided, another seed is chosen."""
    rows = pr.bulk_rows(d) if name == "bulk" else pr.cloud(name, d)
    und = pr.undecided(rows, d)
    assert not und.any(), np.flatnonzero(und)[:8].tolist()


def test_undecided_marks_a_boundary_and_nothing_else():
    """exp(x) for x = ln of an f32 midpoint lies on a rounding boundary to within the f64 error of the logarithm"""
    mid = (np.float64(F(1.5)) + np.float64(np.nextafter(F(1.5), F(2)))) / 2
    x64 = np.log(mid)
    rows = pr.ordinary(4, 0, 0).copy()
    t = pr.tail_col(0)
    rows[:, t + 1:t + 4] = -3.0
    rows[:, t] = 1.0
    assert not pr.undecided(rows, 0).any()
    # no f32 argument hits the midpoint to 2 f64 ulps, so the marking itself is checked on the f64 value
    y = np.exp(np.array([x64, x64 + 1e-9]))
    lo = hi = y
    for _ in range(2):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    assert (lo.astype(F) != hi.astype(F)).tolist() == [True, False]


@pytest.mark.parametrize("d", DEGREES)
def test_block_clouds_name_every_slot(d):
    """every DC / SH slot of every row carries its own (row, coefficient, channel) code, exact in f16"""
    nc = (d + 1) ** 2
    for n in pr.BLOCK_NS:
        rows = pr.cloud(f"block_{n}", d)
        assert rows.shape == (n, pr.row_len(d)) and pr.row_len(d) == (17, 26, 41, 62)[d]
        sh = np.ascontiguousarray(pr.reference(f"block_{n}", d)[1]).view(np.uint16).reshape(n, 16, 3)
        i = np.arange(n)[:, None, None]
        c = np.arange(nc)[None, :, None]
        j = np.arange(3)[None, None, :]
        assert np.array_equal(sh[:, :nc], pr.slot_code(i, c, j))
        assert not sh[:, nc:].any()
        assert len(np.unique(sh[:, :nc])) == n * nc * 3
        for col in range(6, pr.tail_col(d)):
            cc, jj = pr.sh_slot_of_column(col, d)
            assert np.array_equal(rows[:, col].astype(np.float16).view(np.uint16), pr.slot_code(np.arange(n), cc, jj))


@pytest.mark.parametrize("d", DEGREES)
def test_opacity_cloud_reaches_its_edges(d):
    h = dict(zip(pr.OPACITY_LOGITS, _opacity("opacity", d).tolist()))
    h_nan = _opacity("opacity", d)[-1]
    assert h[0.0] == 0x3800 and _opacity("opacity", d)[1] == 0x3800                 # 0 and -0: one half
    assert h[-9.70] == 0x0400 or not _subnormal(np.uint16(h[-9.70]))                # the window's upper end: (just) normal
    for x in pr.OPACITY_SUBNORMAL + (-16.64,):
        assert _subnormal(np.uint16(h[x])), x
    assert h[-16.64] == 0x0001 and h[-17.33] in (0x0000, 0x0001) and h[-17.4] == 0x0000
    assert h[17.33] == 0x3C00 and h[30.0] == 0x3C00 and h[88.8] == 0x3C00 and h[745.0] == 0x3C00 and h[np.inf] == 0x3C00
    for x in (-30.0, -87.3, -88.8, -103.97, -104.0, -745.0, -np.inf):
        assert h[x] == 0x0000, x
    assert pr.is_nan_half(h_nan)
    # the f32 facts the names rest on
    e = pr.exp_f64(np.array([-17.33, -88.8, -103.97, -104.0, 88.8], F))
    assert F(1) + e[0] == F(1)                                                       # 1 + e rounds to 1
    assert 0 < e[1] < np.finfo(F).tiny and e[2] == np.nextafter(F(0), F(1)) and e[3] == 0 and np.isinf(e[4])


@pytest.mark.parametrize("d", DEGREES)
def test_scale_clouds_reach_their_edges(d):
    cov = _cov("scales_identity", d)
    iso = {v: cov[4 * k] for k, v in enumerate(pr.LOG_SCALES) if not np.isnan(v)}      # rows 4k: the value in all three axes
    diag = [0, 3, 5]
    for v, want in ((-np.inf, 0x0000), (-104.0, 0x0000), (-20.0, 0x0000), (-12.5, 0x0000), (-8.5, 0x0001),
                    (0.0, 0x3C00), (5.5449, 0x7BFF), (5.55, 0x7C00), (44.4, 0x7C00)):
        assert iso[v][diag].tolist() == [want] * 3, (v, iso[v])
    assert ((iso[-4.85][diag] >= 0x0400) & (iso[-4.85][diag] < 0x0408)).all()                 # the first normal halves
    assert set(iso[-8.664][diag].tolist()) <= {0x0000, 0x0001}                         # beside the 2^-25 tie
    with np.errstate(over="ignore"):
        sq = pr.exp_f64(np.array([-8.664, 44.4, -12.5], F)) ** 2
    assert abs(float(sq[0]) / 2.0 ** -25 - 1) < 1e-3 and np.isinf(sq[1]) and 0 < sq[2] < 2.0 ** -25
    # an infinite scale beside the rotation's zeros: 0 * inf, the zero terms of R * diag(s) included
    for v in (88.8, np.inf):
        assert pr.is_nan_half(iso[v]).all(), v
    assert pr.is_nan_half(cov[4 * len(pr.LOG_SCALES) - 4:]).any()                      # the NaN rows
    gen = _cov("scales_generic", d)
    assert _subnormal(gen).any() and (gen == 0x7C00).any() and pr.is_nan_half(gen).any()
    assert ((gen & 0x7FFF) == 0).any()


@pytest.mark.parametrize("d", DEGREES)
def test_quaternion_cloud_reaches_its_edges(d):
    cov = _cov("quaternions", d)
    q = np.array(pr.QUATERNIONS, F)
    tiny = np.finfo(F).tiny
    with np.errstate(all="ignore"):
        sq = q * q
        mag2 = sq[:, 0] + (sq[:, 1] + sq[:, 2] + sq[:, 3])
    for k in pr.Q_SUBNORMAL_SQUARES:
        nz = q[k] != 0
        assert ((sq[k][nz] > 0) & (sq[k][nz] < tiny)).all(), k                         # flushed, they would be 0 and the row NaN
        assert not pr.is_nan_half(cov[k]).any() and ((cov[k] & 0x7FFF) < 0x7C00).all(), (k, cov[k])
    assert np.array_equal(cov[12], cov[0])                                             # (1e-20, 0, 0, 0) normalises to the identity
    for k in (16, 17):
        assert mag2[k] == 0 and pr.is_nan_half(cov[k]).any(), k
    for k in pr.Q_OVERFLOW:
        assert np.isinf(mag2[k]) and np.array_equal(cov[k], cov[0]), (k, cov[k], cov[0])   # inverse 0: the identity's covariance
    assert np.array_equal(cov[1], cov[0])                                              # -identity
    for k in (8, 9, 10, 11):                                                           # generic, unnormalised by 1e-3 and 1e3
        assert ((cov[k] & 0x7FFF) < 0x7C00).all() and (scenes.half_ulp_diff(cov[k], cov[8]) <= 2).all(), (k, cov[k], cov[8])
    for k in (21, 22, 23, 24):
        assert pr.is_nan_half(cov[k]).any(), k
    assert (cov[:12] == 0x8000).any() or (_cov("mixed", d) == 0x8000).any()


def test_some_covariance_half_is_a_negative_zero():
    found = {name: int((_cov(name, 3) == 0x8000).sum()) for name in ("quaternions", "scales_generic", "scales_identity", "mixed")}
    assert sum(found.values()) >= 1, found


@pytest.mark.parametrize("d", DEGREES)
def test_sh_cloud_reaches_its_edges(d):
    rows = pr.cloud("sh_values", d)
    k = len(pr.SH_VALUES)
    assert len(pr.SH_HALVES) == k
    sh = np.ascontiguousarray(pr.reference("sh_values", d)[1]).view(np.uint16).reshape(k, 16, 3)
    seen = set()
    for col in range(6, pr.tail_col(d)):
        c, j = pr.sh_slot_of_column(col, d)
        for i in range(k):
            v = (i + col - 6) % k
            seen.add((col, v))
            want = pr.SH_HALVES[v]
            assert pr.is_nan_half(sh[i, c, j]) if want is None else sh[i, c, j] == want, (i, col, v, hex(sh[i, c, j]))
    assert len(seen) == k * (pr.tail_col(d) - 6)                                        # every value in every slot
    def value(bits):                                   # 0x7C00 stands for 2^16 here: 65520 is the tie between 65504 and 2^16
        return 65536.0 if bits == 0x7C00 else float(np.uint16(bits).view(np.float16))

    for v in pr.SH_TIES:                                                               # exact ties in f32, to the even neighbour
        x = abs(float(F(pr.SH_VALUES[v])))
        r = pr.SH_HALVES[v] & 0x7FFF
        mids = [(value(r) + value(r + 1)) / 2] + ([(value(r - 1) + value(r)) / 2] if r else [])
        assert r % 2 == 0 and x in mids, (v, x, hex(r))


@pytest.mark.parametrize("d", DEGREES)
def test_positions_pass_through(d):
    rows = pr.cloud("positions", d)
    g, _ = pr.reference("positions", d)
    assert np.array_equal(g[:, :12], np.ascontiguousarray(rows[:, :3]).view(np.uint8).reshape(-1, 12))
    bits = np.ascontiguousarray(rows[:, :3]).view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 1).any() and (bits == 0x80000001).any()
    assert (np.abs(rows[:, :3]) == F(3e38)).any()


@pytest.mark.parametrize("d", DEGREES)
def test_mixed_cloud_holds_every_class(d):
    cov, op = _cov("mixed", d), _opacity("mixed", d)
    assert pr.is_nan_half(cov).sum() > 100 and ((cov & 0x7FFF) == 0x7C00).sum() > 100
    assert (cov == 0x8000).sum() >= 1 and _subnormal(cov).sum() > 10
    assert pr.is_nan_half(op).any() and _subnormal(op).any() and (op == 0).any() and (op == 0x3C00).any()
    assert len(pr.cloud("mixed", d)) == pr.MIXED_N


@pytest.mark.parametrize("d", DEGREES)
def test_f64_and_libm_forms_within_the_device_envelope(d):
    """tests/test_gpu_ply_decode.py's envelope for the kernel against the oracle, held by the two forms of the restatement:
    at most one f16 ulp (off-diagonal elements that cancel: 4e-7 of the row's largest element) on at most 0.2 % of the halves"""
    h = pr.computed_halves(pr.reference("bulk", d, "f64")[0])
    h0 = pr.computed_halves(pr.reference("bulk", d, "libm")[0])
    ulp = scenes.half_ulp_diff(h, h0)
    v, v0 = h.view(np.float16).astype(np.float64), h0.view(np.float16).astype(np.float64)
    row_scale = np.abs(v0[:, 1:]).max(axis=1, keepdims=True)
    bad = (ulp > 1) & ~(np.abs(v - v0) <= 4e-7 * row_scale)
    assert not bad.any(), (int(bad.sum()), int(ulp.max()))
    assert float((ulp != 0).mean()) <= 2e-3
    assert np.array_equal(pr.reference("bulk", d, "f64")[1], pr.reference("bulk", d, "libm")[1])


@pytest.mark.parametrize("defect,name", [("flush", "quaternions"), ("fused", "bulk"), ("fused", "mixed"),
                                         ("approx_rcp", "quaternions"), ("approx_rcp", "bulk")])
def test_a_named_defect_would_show(defect, name):
    """The exact comparison is worth what it can tell apart: a restatement with f32 subnormals flushed in the normalisation,
    with the sum of squares contracted into fused multiply-adds, or with a reciprocal one ulp off differs from the reference in
    some half of the cloud that is there for it -- while each of them stays inside the one-ulp envelope on the bulk scene."""
    rows = pr.bulk_rows(3) if name == "bulk" else pr.cloud(name, 3)
    g, s = pr.decode_ref(rows, 3, "f64", defect=defect)
    bad, bad_sh, fixed = pr.compare(g, s, *pr.reference(name, 3))
    assert fixed and not bad_sh.any()
    assert bad.any(), (defect, name)
    if name == "bulk":
        ulp = scenes.half_ulp_diff(pr.computed_halves(g), pr.computed_halves(pr.reference(name, 3)[0]))
        assert float((ulp != 0).mean()) <= 2e-3                                  # the old envelope let it through
