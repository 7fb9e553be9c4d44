"""The Gaussian adapter's restatement (tests/adapter_restated.py) on the CPU: the properties of its float64 rotation builder for the
harmonics, to 1e-10, and the restatement against fixture G27 (the reference's own GaussianAdapter.forward,
tests/golden/make_goldens_g27.py).  The GPU tests (test_gpu_adapter.py) compare the kernels with this restatement.  Also the planted
cases of tests/adapter_edges.py on the restatements alone: finite, and inside the bar that test_gpu_adapter_edges.py sets for the kernels.
"""
import numpy as np
import pytest
import torch

import adapter_edges as E
import adapter_restated as A
import splat_restated as R
import splat_scenes as S
from conftest import load_golden

TOL = 1e-10
# sh_basis, degree 1: Y = C1 (-y, z, -x) = C1 P d
P = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])


def rotations(seed, n):
    rng = np.random.RandomState(seed)
    return np.stack([A.rotation(rng) for _ in range(n)])


def matrix(C, d_sh=25):
    return A.blocks_to_matrix(A.sh_rotation_blocks(C, d_sh), d_sh).numpy()


@pytest.mark.parametrize("d_sh", [1, 4, 9, 16, 25])
def test_defining_identity_at_random_directions(d_sh):
    """sum_j (D c)_j Y_j(C d) = sum_j c_j Y_j(d) for random d and c, with Y = sh_basis."""
    C = rotations(41, 3)
    D = matrix(C, d_sh)
    rng = np.random.RandomState(42)
    d = rng.normal(size=(50, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = rng.normal(size=(50, d_sh))
    want = (R.sh_basis(torch.from_numpy(d), d_sh).numpy() * c).sum(-1)
    for v in range(3):
        got = (R.sh_basis(torch.from_numpy(d @ C[v].T), d_sh).numpy() * (c @ D[v].T)).sum(-1)
        assert np.abs(got - want).max() < TOL


def test_identity_orthogonality_and_composition():
    Cs = rotations(43, 2)
    assert np.abs(matrix(np.eye(3)[None])[0] - np.eye(25)).max() < TOL
    Da, Db = matrix(Cs)
    assert np.abs(Da @ Da.T - np.eye(25)).max() < TOL
    Dab = matrix((Cs[0] @ Cs[1])[None])[0]
    assert np.abs(Dab - Da @ Db).max() < TOL
    assert np.abs(Da - np.eye(25)).max() > 0.1        # the rotations are well away from the identity


def test_degree_one_block_is_the_signed_permutation_of_the_rotation():
    Cs = rotations(44, 3)
    D = matrix(Cs, 4)
    for v in range(3):
        assert np.abs(D[v][1:4, 1:4] - P @ Cs[v] @ P.T).max() < TOL
        assert abs(D[v][0, 0] - 1.0) < TOL


def test_restatement_against_g27():
    """Every field the reference's GaussianAdapter.forward returned (fp32, with its rotate_sh replaced by the identity), against the
    float64 restatement with identity blocks: within twice the distance the generator recorded, and that distance is at rounding level."""
    g = load_golden("g27_adapter")
    assert "576-578" in str(g["restated_offset_lines"])
    for tag in [str(t) for t in g["cases"]]:
        V, h, w, S_, d_sh = (int(v) for v in g[tag + ".shape"])
        c = dict(V=V, h=h, w=w, S=S_, d_sh=d_sh, s_min=float(g[tag + ".scale_range"][0]), s_max=float(g[tag + ".scale_range"][1]),
                 **{k: g[f"{tag}.in_{k}"] for k in ("extrinsics", "intrinsics", "raw", "depth", "opacity")})
        assert np.array_equal(g[tag + ".handed_rotations"], c["extrinsics"][:, :3, :3])
        L = A.degree_of(d_sh)
        identity = np.zeros((V, A.ROT_OFF[L + 1]))
        for l in range(L + 1):
            identity[:, A.ROT_OFF[l]:A.ROT_OFF[l + 1]] = np.eye(2 * l + 1).reshape(-1)
        o64, _ = A.restate(c, identity, torch.float64)
        for name in ("means", "covariances", "harmonics", "opacities", "scales", "rotations"):
            own = float(g[f"{tag}.own_{name}"])
            err = float(np.abs(g[f"{tag}.{name}"].astype(np.float64) - o64[name]).max())
            top = float(np.abs(o64[name]).max())
            print(f"{tag} {name}: reference - restatement {err:.3g}, recorded {own:.3g}, largest entry {top:.3g}")
            assert err <= 2.0 * own + 1e-12 and own <= 2e-6 * max(top, 1.0), (tag, name)


def test_case_inputs_meet_their_promises():
    c = A.case(7, 3, 5, 7, 2, 25)
    assert float(np.linalg.norm(c["raw"][..., 5:9], axis=-1).min()) >= 0.1 - 1e-6
    assert 0.3 <= c["depth"].min() and c["depth"].max() <= 5.0
    for v in range(3):
        Cv = c["extrinsics"][v, :3, :3].astype(np.float64)
        assert abs(np.linalg.det(Cv) - 1.0) < 1e-5 and np.abs(Cv - np.eye(3)).max() > 0.05


@pytest.mark.parametrize("name", E.NAMES)
def test_planted_edges_are_finite_and_inside_their_own_bar(name):
    """tests/adapter_edges.py: on every planted case both restatements are finite in every field and both gradients, and within each
    group (and among the Gaussians no group names) the float32 restatement lies under the group's bar against float64 -- the reference
    alone stays inside the condition test_gpu_adapter_edges.py sets for the kernel.  The zero quaternion's gradient is 0 (torch's norm
    has the subgradient 0 at 0); the underflowing ones get a finite gradient of ordinary size."""
    c, groups, _, _, o64, g64, o32, g32 = E.reference(name)
    assert list(groups) == [name] and len(set(groups[name])) == len(groups[name])
    for o, g in ((o64, g64), (o32, g32)):
        for k, x, _ in E.quantities(c, o, g):
            assert np.isfinite(x).all(), (name, k, x.dtype)
    sets = dict(groups, rest=E.rest(c, groups))
    assert sum(len(v) for v in sets.values()) == c["V"] * c["h"] * c["w"] * c["S"]           # no Gaussian is left out
    for group, gaussians in sets.items():
        idx = E.flat(c, gaussians)
        for (k, x64, pp), (_, x32, _) in zip(E.quantities(c, o64, g64), E.quantities(c, o32, g32)):
            a, b = E.rows_of(c, x64, idx, pp).astype(np.float64), E.rows_of(c, x32, idx, pp).astype(np.float64)
            bar, own = E.group_bar(a, b)
            print(f"{name} / {group} {k}: max|x| {np.abs(a).max():.4g}  restated f32-f64 {own:.3g}")
            assert (np.abs(b - a) <= bar).all(), (name, group, k)
    if name == "quat_zero":
        for g in (g64, g32):
            assert not E.rows_of(c, g[0], E.flat(c, groups[name]))[:, 5:9].any()
    if name == "quat_underflow":
        q = np.abs(E.rows_of(c, g64[0], E.flat(c, groups[name]))[:, 5:9])
        assert np.isfinite(q).all() and q[0].max() > 0.1 and q[0].max() < 1e3


def test_planted_edges_leave_the_case_and_the_other_gaussians_alone():
    """adapter_restated.case keeps its promises (the planted values live in adapter_edges); a planted case differs from the clean one
    only in the rows it names."""
    base = E.clean()
    assert float(np.linalg.norm(base["raw"][..., 5:9], axis=-1).min()) >= 0.1 - 1e-6 and base["depth"].min() >= 0.3
    for name in E.NAMES:
        c, groups = E.planted(name)
        keep = np.ones(c["V"] * c["h"] * c["w"] * c["S"], bool)
        keep[E.flat(c, groups[name])] = False
        assert np.array_equal(c["raw"].reshape(keep.size, -1)[keep], base["raw"].reshape(keep.size, -1)[keep]), name
        same_depth = np.repeat(c["depth"].reshape(-1).view(np.int32) == base["depth"].reshape(-1).view(np.int32), c["S"])
        assert same_depth[keep].all() and not (name.startswith("depth") and same_depth[~keep].any()), name


def test_composition_seed_stays_under_the_left_out_cap():
    """The chained float64 restatement of the composition case: every Gaussian-level decision of the rasteriser has its 1e-3 margin and
    at most 1 % of the pixels are left out (splat_scenes' cap, unchanged)."""
    import adapter_scene
    ref = adapter_scene.composition_reference()
    print("left out", float((~ref["kept"]).mean()), "smallest Gaussian margin", ref["gaussian_margin"])
    assert float((~ref["kept"]).mean()) <= S.MAX_LEFT_OUT
    assert ref["gaussian_margin"] >= S.MARGIN
    assert np.isfinite(ref["loss64"]) and ref["loss64"] > 0
