"""The Gaussian adapter (csrc/adapter.hip through ops.adapter) at the values and shapes test_gpu_adapter.py keeps away from: the planted
cases of tests/adapter_edges.py (degenerate quaternions, saturated sigmoids, depths at and around zero, a very large depth), one NaN or
inf at a time in every kind of input, the block and shape edges (S = 3, exactly 64 and 65 Gaussians, one Gaussian, one row, one column,
one view, `raw` expanded over the views), gradients handed over as None, the cameras kernel at the identity, at axis rotations, on strided
and on singular intrinsics, and a zero row of `raw` through functional.gaussian_head -> functional.pixel_gaussians.

Bars.  Always against the float64 restatement, by the rule of DESIGN 4.12 exactly as adapter_restated.bar: elementwise max(1e-4 |x| +
1.25e-6 max|x|, 4 x the float32 restatement's own largest distance from float64).  For a planted group the rule is applied to the arrays
RESTRICTED TO THAT GROUP'S GAUSSIANS: max|x| and the own distance come from those rows alone, so a gradient of 1e9 at a quaternion of
norm 5e-9 or a covariance of 1e8 at depth 3e4 widens nothing else's bar; the Gaussians no group names are a group of their own.  Leaks
between Gaussians are checked by bits against a run of the unplanted case: a Gaussian is one lane's work.  Every test prints its
figures before it asserts (pytest -s); the measured ones are in DESIGN.md 4.16.
"""
import numpy as np
import pytest
import torch

import adapter_edges as E
import adapter_restated as A
import gshead_restated as G

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
_CLEAN = {}


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def compare(tag, got, x64, x32):
    """got against the float64 value under the bar of the arrays handed in; prints the figures first; returns the worst err / bar."""
    x64, x32 = np.asarray(x64, np.float64), np.asarray(x32, np.float64)
    bar, own = A.bar(x64, x32)
    err = np.abs(np.asarray(got, np.float64) - x64)
    worst = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    print(f"{tag}: max|x| {np.abs(x64).max():.4g}  kernel-f64 {err.max():.3g}  restated f32-f64 {own:.3g}  worst err/bar {worst:.3f}")
    assert np.isfinite(got).all(), tag
    assert (err <= bar).all(), (tag, worst)
    return worst


def launch(c, gpu, weights=None, raw=None, depth=None):
    """ops.adapter called directly on a case (raw / depth: device tensors instead of the case's) -> dict of numpy arrays: the five
    fields and, with weights (a field missing or None: handed over as None), "d raw" (V,R,S,C), "g_depth" (V,R,S) per Gaussian and
    "d depth" (V,R), its sum over S on the device as the registered autograd forms it."""
    from mvsdet_amd.ops import adapter
    L = A.degree_of(c["d_sh"])
    cams = adapter.adapter_cameras(dev(c["extrinsics"], gpu), dev(c["intrinsics"], gpu), c["h"], c["w"], L)
    raw = dev(c["raw"], gpu) if raw is None else raw
    depth = dev(c["depth"], gpu) if depth is None else depth
    out = adapter.pixel_gaussians(raw, depth, cams, c["h"], c["w"], c["s_min"], c["s_max"], L, True)
    res = {k: o.cpu().numpy() for k, o in zip(E.OUT_FIELDS, out)}
    if weights is not None:
        gw = [None if weights.get(k) is None else dev(weights[k], gpu) for k in A.FIELDS]
        g_raw, g_depth = adapter.pixel_gaussians_backward(raw, depth, cams, *gw, c["h"], c["w"], c["s_min"], c["s_max"], L)
        res.update({"d raw": g_raw.cpu().numpy(), "g_depth": g_depth.cpu().numpy(), "d depth": g_depth.sum(dim=2).cpu().numpy()})
    return res


def weights_of(c):
    n = c["V"] * c["h"] * c["w"] * c["S"]
    return A.loss_weights(c["seed"], dict(means=(n, 3), covariances=(n, 3, 3), harmonics=(n, 3, c["d_sh"])))


def clean_run(key, c, gpu):
    """The kernels on an unplanted case, computed once and shared, unchanged."""
    if key not in _CLEAN:
        _CLEAN[key] = launch(c, gpu, weights_of(c))
        assert all(np.isfinite(v).all() for v in _CLEAN[key].values())
    return _CLEAN[key]


PER_GAUSSIAN = E.OUT_FIELDS + ("d raw", "g_depth")


def rows(c, x):
    return np.asarray(x).reshape(c["V"] * c["h"] * c["w"] * c["S"], -1)


# ------------------------------------------------------------------------------------------- 1. planted values
@pytest.mark.parametrize("name", E.NAMES)
def test_planted_groups_against_the_restatement(gpu, name):
    """Every field and both gradients, finite and under the group's own bar, for the planted Gaussians and for the rest; the zero
    quaternions' gradient bit-zero; every unplanted Gaussian with the bits of the unplanted case's run."""
    c, groups, _, weights, o64, g64, o32, g32 = E.reference(name)
    got = launch(c, gpu, weights)
    want64, want32 = E.quantities(c, o64, g64), E.quantities(c, o32, g32)
    worst = {}
    for group, gaussians in dict(groups, rest=E.rest(c, groups)).items():
        idx = E.flat(c, gaussians)
        worst[group] = max(compare(f"{name} / {group} {k}", E.rows_of(c, got[k], idx, pp), E.rows_of(c, x64, idx, pp), E.rows_of(c, x32, idx, pp))
                           for (k, x64, pp), (_, x32, _) in zip(want64, want32))
    print(f"{name}: worst ratio to the bar {worst}")
    idx = E.flat(c, groups[name])
    if name == "quat_zero":
        assert not bits(rows(c, got["d raw"])[idx][:, 5:9]).any()
    base = clean_run("base", E.clean(), gpu)
    keep = np.ones(c["V"] * c["h"] * c["w"] * c["S"], bool)
    keep[idx] = False
    assert keep.sum() >= keep.size - 12
    for k in PER_GAUSSIAN:
        assert same(rows(c, got[k])[keep], rows(c, base[k])[keep]), (name, k)


# ------------------------------------------------------------------------------------------- 2. non-finite inputs
NONFINITE_CASES = {"v2_3x43_s2_sh25": (161, 2, 3, 43, 2, 25), "v2_5x7_s2_sh4": (E.SEED, E.V, E.H, E.W, E.S, E.D_SH)}


def spots(c):
    """The last Gaussian of a 64-block, the first of the next, the last of the last view, as (v, r, s)."""
    N = c["h"] * c["w"] * c["S"]
    return [(0, 63 // c["S"], 63 % c["S"]), (0, 64 // c["S"], 64 % c["S"]), (c["V"] - 1, (N - 1) // c["S"], (N - 1) % c["S"])]


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
@pytest.mark.parametrize("case", list(NONFINITE_CASES))
def test_one_non_finite_input_stays_where_the_formulas_put_it(gpu, case, value):
    """One NaN (or inf) in an offset, a scale, a quaternion component, a degree-0 coefficient of colour 1, a degree-2 coefficient of
    colour 2 (degree 1 where d_sh = 4 has no degree 2) or a depth, at three Gaussians.  Everything outside the Gaussian (for a depth:
    the pixel's S Gaussians) has the clean run's bits, forward and backward; inside, every field the formulas do not connect to the
    element has them too, the connected ones are non-finite; the gradient's harmonics columns, a linear map that never reads `raw`, keep
    their bits, and a coefficient changes nothing in the backward at all.  A non-finite coefficient stays inside its colour's d_sh values
    and covers its degree's block (the kernel multiplies block by block; a dense block-diagonal product would spread 0 * NaN over the
    whole colour: both are accepted).  inf through a sigmoid is not non-finite: sigmoid(inf) = 1, so an inf offset or scale must give the
    bits of a planted 104, where the fp32 sigmoid is exactly 1 as well (test_planted_groups holds that value to the restatement)."""
    c = A.case(*NONFINITE_CASES[case])
    d_sh, Sn, C = c["d_sh"], c["S"], 9 + 3 * c["d_sh"]
    L = A.degree_of(d_sh)
    weights = weights_of(c)
    base = clean_run(case, c, gpu)
    deg = min(2, L)
    coeff1, coeff2 = 9 + 1 * d_sh, 9 + 2 * d_sh + deg * deg + deg              # degree 0 of colour 1; the middle of degree `deg` of colour 2
    elements = {
        "offset": (0, ("means",), slice(2, C), True),
        "scale": (3, ("covariances", "scales"), np.r_[0:2, 9:C], True),
        "quaternion": (6, ("covariances", "rotations"), np.r_[0:2, 9:C], True),
        "coefficient 0 of colour 1": (coeff1, ("harmonics",), slice(0, C), False),
        f"coefficient of degree {deg} of colour 2": (coeff2, ("harmonics",), slice(0, C), False),
        "depth": (None, ("means", "covariances", "scales"), slice(9, C), True),
    }
    for v, r, s in spots(c):
        for tag, (col, connected, quiet_cols, depth_connected) in elements.items():
            raw, depth = dev(c["raw"], gpu), dev(c["depth"], gpu)
            through_sigmoid = value == INF and col in (0, 3)
            if col is None:
                depth[v, r] = value
                unit = E.flat(c, [(v, r, k) for k in range(Sn)])
            else:
                raw[v, r, s, col] = value
                unit = E.flat(c, [(v, r, s)])
            got = launch(c, gpu, weights, raw, depth)
            where = f"{case} {tag} = {value} at {(v, r, s)}"
            keep = np.ones(c["V"] * c["h"] * c["w"] * Sn, bool)
            keep[unit] = False
            for k in PER_GAUSSIAN:
                assert same(rows(c, got[k])[keep], rows(c, base[k])[keep]), (where, k, "outside the Gaussian")
            if through_sigmoid:
                raw[v, r, s, col] = 104.0
                finite = launch(c, gpu, weights, raw, depth)
                for k in PER_GAUSSIAN:
                    assert same(got[k], finite[k]) and np.isfinite(got[k]).all(), (where, k, "sigmoid(inf) = 1")
                continue
            for k in E.OUT_FIELDS:
                inside, clean = rows(c, got[k])[unit], rows(c, base[k])[unit]
                if k in connected:
                    assert not np.isfinite(inside).all(axis=1).any(), (where, k, "connected, yet finite")
                else:
                    assert same(inside, clean), (where, k, "not connected, yet changed")
            assert same(rows(c, got["d raw"])[unit][:, quiet_cols], rows(c, base["d raw"])[unit][:, quiet_cols]), (where, "d raw")
            loud = np.concatenate([rows(c, got["d raw"])[unit], rows(c, got["g_depth"])[unit]], axis=1)
            if depth_connected:
                assert not np.isfinite(loud).all(axis=1).any(), (where, "gradient finite")
            else:
                assert same(rows(c, got["g_depth"])[unit], rows(c, base["g_depth"])[unit]), (where, "g_depth")
            if "harmonics" in connected:
                colour = 1 if col == coeff1 else 2
                l = 0 if col == coeff1 else deg
                bad = ~np.isfinite(got["harmonics"].reshape(-1, 3, d_sh)[unit[0]])
                assert bad[colour, l * l:(l + 1) * (l + 1)].all() and not np.delete(bad, colour, axis=0).any(), (where, bad)


@pytest.mark.parametrize("case", list(NONFINITE_CASES))
def test_one_nan_in_a_gradient_reaches_exactly_its_row(gpu, case):
    """One NaN in g_means, in g_covariances or in g_harmonics: g_raw and g_depth are non-finite in that Gaussian's row, every other row
    has the clean run's bits, and inside the row the parts the formulas do not connect keep theirs (g_means: scales, quaternion,
    harmonics columns; g_covariances: offset and harmonics columns; g_harmonics: the nine geometry columns, g_depth, the other colours)."""
    c = A.case(*NONFINITE_CASES[case])
    d_sh, C = c["d_sh"], 9 + 3 * c["d_sh"]
    weights = weights_of(c)
    base = clean_run(case, c, gpu)
    plants = {"means": ((1,), slice(2, C), True), "covariances": ((1, 2), np.r_[0:2, 9:C], True),
              "harmonics": ((2, d_sh - 1), slice(0, 9 + 2 * d_sh), False)}
    for v, r, s in spots(c):
        g = int(E.flat(c, [(v, r, s)])[0])
        for field, (at, quiet_cols, depth_connected) in plants.items():
            w = {k: a.copy() for k, a in weights.items()}
            w[field][(g,) + at] = NAN
            got = launch(c, gpu, w)
            where = f"{case} NaN in g_{field} at {(v, r, s)}"
            keep = np.arange(rows(c, got["d raw"]).shape[0]) != g
            for k in ("d raw", "g_depth"):
                assert same(rows(c, got[k])[keep], rows(c, base[k])[keep]), (where, k, "another row")
            row, depth_g = rows(c, got["d raw"])[g], rows(c, got["g_depth"])[g]
            assert same(row[quiet_cols], rows(c, base["d raw"])[g][quiet_cols]), (where, "not connected, yet changed")
            assert not np.isfinite(row).all(), where
            assert (not np.isfinite(depth_g).all()) if depth_connected else same(depth_g, rows(c, base["g_depth"])[g]), (where, "g_depth")
            for k in E.OUT_FIELDS:
                assert same(got[k], base[k]), (where, k)


# ------------------------------------------------------------------------------------------- 3. block and shape edges
# name -> (V, h, w, S, d_sh).  S = 3: 64 % 3 != 0, so a pixel's samples straddle the 64-Gaussian block and r = g / S changes inside one
SHAPES = {
    "s3_5x7_sh4": (2, 5, 7, 3, 4),
    "s3_3x43_sh9": (2, 3, 43, 3, 9),
    "n64_8x8_s1_sh16": (2, 8, 8, 1, 16),
    "n65_5x13_s1_sh4": (2, 5, 13, 1, 4),
    "one_gaussian_sh25": (2, 1, 1, 1, 25),
    "h1_w35_s2_sh1": (2, 1, 35, 2, 1),
    "h35_w1_s2_sh25": (2, 35, 1, 2, 25),
    "v1_5x7_s2_sh9": (1, 5, 7, 2, 9),
    "v1_one_gaussian_sh1": (1, 1, 1, 1, 1),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_block_and_shape_edges_against_the_restatement(gpu, name):
    """Each shape against the restatement under the ordinary whole-case bar: the five fields and both gradients."""
    c = A.case(170 + list(SHAPES).index(name), *SHAPES[name])
    _, weights, o64, g64, o32, g32 = E.restated(c)
    got = launch(c, gpu, weights)
    worst = [compare(f"{name} {k}", got[k].reshape(np.shape(x64)), x64, x32)
             for (k, x64, _), (_, x32, _) in zip(E.quantities(c, o64, g64), E.quantities(c, o32, g32))]
    print(f"{name}: worst ratio to the bar {max(worst):.3f}")
    assert got["means"].shape == (c["V"] * c["h"] * c["w"] * c["S"], 3)


def test_raw_expanded_over_the_views_is_read_in_place(gpu):
    """raw (1,R,S,C) expanded over 3 views (stride(0) == 0): handed to the kernels as it is, the bits of the materialised copy."""
    from mvsdet_amd.ops import adapter
    c = A.case(180, 3, 5, 7, 2, 9)
    c["raw"] = np.ascontiguousarray(np.broadcast_to(c["raw"][:1], c["raw"].shape))
    weights = weights_of(c)
    expanded = dev(c["raw"][:1], gpu).expand(3, -1, -1, -1)
    assert expanded.stride(0) == 0
    handed, view, row = adapter._rows(expanded)
    assert handed is expanded and view == 0 and row == c["raw"].shape[3]
    a, b = launch(c, gpu, weights, raw=expanded), launch(c, gpu, weights)
    for k in PER_GAUSSIAN:
        assert same(a[k], b[k]), k
    assert not same(rows(c, a["means"])[:70], rows(c, a["means"])[70:140])           # the views differ: each used its own camera


# ------------------------------------------------------------------------------------------- 4. a gradient that is None
def test_a_gradient_that_is_none_counts_as_zeros(gpu):
    """pixel_gaussians_backward with only g_means, only g_covariances, only g_harmonics: the bits of the call with explicit zeros for
    the other two, and under the bar against the restatement with those weights zero."""
    c = A.case(181, 2, 3, 43, 2, 9)
    full = weights_of(c)
    for only in A.FIELDS:
        zeros = {k: (a if k == only else np.zeros_like(a)) for k, a in full.items()}
        none = {k: (a if k == only else None) for k, a in full.items()}
        a, b = launch(c, gpu, none), launch(c, gpu, zeros)
        assert same(a["d raw"], b["d raw"]) and same(a["g_depth"], b["g_depth"]), only
        _, _, _, g64, _, g32 = E.restated(c, zeros)
        compare(f"only g_{only}: d raw", a["d raw"], g64[0], g32[0])
        compare(f"only g_{only}: d depth", a["d depth"], g64[1], g32[1])
        assert np.abs(a["d raw"]).max() > 0


# ------------------------------------------------------------------------------------------- 5. the cameras kernel
def axis_rotation(axis, angle):
    """A rotation about a coordinate axis; multiples of 90 degrees give exact 0 and +-1."""
    quarter = angle / (np.pi / 2)
    co, si = (float(np.round(np.cos(angle))), float(np.round(np.sin(angle)))) if quarter == round(quarter) else (np.cos(angle), np.sin(angle))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = co, -si, si, co
    return m


def test_cameras_at_the_identity_and_at_axis_rotations(gpu):
    """The rotations adapter_restated.case avoids: the identity, 90 degrees about x, y and z, 180 degrees about z, 1e-4 rad about z.
    The probe directions meet zeros of the basis there.  The blocks against the float64 builder; at the identity also |D - I| <= bar."""
    from mvsdet_amd.ops import adapter
    Cs = np.stack([np.eye(3), axis_rotation(0, np.pi / 2), axis_rotation(1, np.pi / 2), axis_rotation(2, np.pi / 2), axis_rotation(2, np.pi),
                   axis_rotation(2, 1e-4)]).astype(np.float32)
    assert np.array_equal(np.abs(Cs[1:5]), np.round(np.abs(Cs[1:5]))) and abs(float(Cs[5, 1, 0]) - 1e-4) < 1e-8
    base = A.case(182, len(Cs), 5, 7, 1, 25)
    ext = base["extrinsics"].copy()
    ext[:, :3, :3] = Cs
    cams = adapter.adapter_cameras(dev(ext, gpu), dev(base["intrinsics"], gpu), 5, 7, 4).cpu().numpy()
    blocks = A.sh_rotation_blocks(Cs, 25)
    D = cams[:, adapter.ADAPTER_ROT:adapter.ADAPTER_ROT + 165]
    for v, tag in enumerate(("identity", "x 90", "y 90", "z 90", "z 180", "z 1e-4")):
        compare(f"blocks at {tag}", D[v], blocks[v], blocks[v].astype(np.float32))
    identity = np.concatenate([np.eye(2 * l + 1).reshape(-1) for l in range(5)])
    bar, _ = A.bar(identity, identity)
    err = np.abs(D[0].astype(np.float64) - identity)
    print(f"identity: |D - I| {err.max():.3g}  worst err/bar {float((err / bar).max()):.3f}")
    assert (err <= bar).all()
    assert np.abs(D[5].astype(np.float64) - identity).max() > 1e-5             # 1e-4 rad is not the identity
    assert np.array_equal(cams[:, :9], Cs.reshape(-1, 9))


def test_cameras_on_skewed_strided_and_singular_intrinsics(gpu):
    """K with skew and unequal focal lengths against numpy's float64 inverse; K as the [:, :3, :3] slice of a (V,4,4) tensor and the
    extrinsics as a [::2] slice, both read in place: the bits of contiguous copies.  One view with det K = 0 (and a singular 2 x 2
    corner): its K^-1 and multiplier are non-finite -- a division by zero, nothing is caught --, the other views' records have the bits
    of a run without it, and the call returns normally."""
    from mvsdet_amd.ops import adapter
    base = A.case(183, 3, 5, 7, 1, 9)
    K = base["intrinsics"].copy()
    K[0] = [[0.7, 0.31, 0.42], [0.0, 1.9, 0.58], [0.0, 0.0, 1.0]]
    K[1] = [[1.3, -0.4, 0.5], [0.05, 0.6, 0.45], [0.0, 0.0, 1.0]]
    ext = base["extrinsics"]
    plain = adapter.adapter_cameras(dev(ext, gpu), dev(K, gpu), 5, 7, 2)
    Kd = K.astype(np.float64)
    Ki = np.linalg.inv(Kd).reshape(-1, 9)
    compare("K^-1 with skew", plain[:, 12:21].cpu().numpy(), Ki, Ki.astype(np.float32))
    m = 0.1 * (np.linalg.inv(Kd[:, :2, :2]) @ np.array([1.0 / 7, 1.0 / 5])).sum(-1)
    compare("multiplier with skew", plain[:, 21].cpu().numpy(), m, m.astype(np.float32))
    K4 = torch.full((3, 4, 4), NAN, device=gpu)
    K4[:, :3, :3] = dev(K, gpu)
    E8 = torch.full((6, 4, 4), NAN, device=gpu)
    E8[::2] = dev(ext, gpu)
    k_view, e_view = K4[:, :3, :3], E8[::2]
    assert k_view.stride() == (16, 4, 1) and e_view.stride() == (32, 4, 1) and not k_view.is_contiguous() and not e_view.is_contiguous()
    assert same(adapter.adapter_cameras(e_view, k_view, 5, 7, 2), plain)
    singular = K.copy()
    singular[1] = [[1.0, 0.0, 0.5], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0]]
    assert np.linalg.det(singular[1].astype(np.float64)) == 0.0
    got = adapter.adapter_cameras(dev(ext, gpu), dev(singular, gpu), 5, 7, 2)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert not np.isfinite(got[1, 12:22]).any()
    assert same(got[[0, 2]], plain[[0, 2]]) and same(got[1, :12], plain[1, :12]) and same(got[1, 22:], plain[1, 22:])


# ------------------------------------------------------------------------------------------- 6. through the chain
def test_a_zero_row_through_the_head_and_the_adapter(gpu):
    """functional.gaussian_head -> functional.pixel_gaussians on 5 x 7 pixels, C = 8, d_sh = 4, S = 2, zero bias; one pixel's features,
    depth_coding and rgb are all <= 0 (exact zeros of both signs among them), so its rows of `raw` are exactly 0: zero quaternions.
    With a linear loss on means, covariances and harmonics the head's weight and bias gradients -- sums over all pixels -- are finite
    and under the bar of the two restatements chained (gshead_restated -> adapter_restated, float64 and float32)."""
    from mvsdet_amd import functional as F_
    ids, h, w, S, d_sh = [0, 2], 5, 7, 2, 4
    hc = G.case(310, 3, ids, 8, 6, 9, h, w, S, d_sh, "rows", 4)
    hc["bias"][:] = 0.0
    v, y, x = 1, 2, 3
    hc["feature"][ids[v], :, y, x] = np.array([-1.0, 0.0, -0.0, -0.3, -2.5, 0.0, -1e-3, -0.0], np.float32)
    hc["depth_coding"][ids[v], 0, y, x] = -0.5
    hc["rgb_raw"][v, y * w + x] = np.array([-0.1, 0.0, -0.0], np.float32)
    ac = A.case(311, len(ids), h, w, S, d_sh)
    weights = weights_of(ac)
    blocks = A.sh_rotation_blocks(ac["extrinsics"][:, :3, :3], d_sh)
    chain = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [torch.from_numpy(hc[k]).to(dtype).requires_grad_(True) for k in ("weight", "bias")]
        raw = G.gaussian_head(torch.from_numpy(hc["feature"]).to(dtype), torch.from_numpy(hc["depth_coding"]).to(dtype), torch.tensor(ids),
                              leaves[0], leaves[1], h, w, S, rgb_raw=torch.from_numpy(hc["rgb_raw"]).to(dtype))
        assert not raw.detach()[v, y * w + x].numpy().any()
        out = A.pixel_gaussians(ac["extrinsics"], ac["intrinsics"], raw, ac["depth"], ac["opacity"], h, w, ac["s_min"], ac["s_max"], d_sh,
                                blocks if dtype == torch.float64 else blocks.astype(np.float32), dtype)
        loss = sum((out[k] * torch.from_numpy(weights[k]).to(dtype)).sum() for k in A.FIELDS)
        chain[dtype] = [g.numpy() for g in torch.autograd.grad(loss, leaves)]
        assert all(np.isfinite(g).all() for g in chain[dtype])
    weight, bias = (dev(hc[k], gpu).requires_grad_(True) for k in ("weight", "bias"))
    raw = F_.gaussian_head(dev(hc["feature"], gpu), dev(hc["depth_coding"], gpu), weight, bias, ids, h, w, S, rgb_raw=dev(hc["rgb_raw"], gpu))
    assert not raw.detach()[v, y * w + x].cpu().numpy().any()
    g = F_.pixel_gaussians(dev(ac["extrinsics"], gpu), dev(ac["intrinsics"], gpu), raw, dev(ac["depth"], gpu), dev(ac["opacity"], gpu), (h, w),
                           ac["s_min"], ac["s_max"], A.degree_of(d_sh))
    loss = sum((getattr(g, k)[0] * dev(weights[k], gpu)).sum() for k in A.FIELDS)
    grads = [t.cpu().numpy() for t in torch.autograd.grad(loss, [weight, bias])]
    for k, got, g64, g32 in zip(("weight", "bias"), grads, chain[torch.float64], chain[torch.float32]):
        compare(f"chain d {k}", got, g64, g32)
