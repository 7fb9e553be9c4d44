"""Seeded scenes for the Gaussian rasteriser's tests (test_splat_host.py, test_gpu_splat.py, test_gpu_splat_edges.py).

A scene is drawn so that every Gaussian-level decision of the algorithm is DECIDED: a Gaussian whose margin to one of them (the near
bound, the radius' ceil, the tile rectangle's truncations, the two tan clamps, the colour clamp) is under 1e-3 -- relative, or in
pixels -- in any view is drawn again.  Per-pixel decisions (alpha against 1/255, T' against 1e-4, the 0.99 cap) cannot be drawn
away: `kept` leaves a pixel with a relative margin under 1e-3 out of comparisons, `with_gradients` gives it weight 0 in the loss, and
test_splat_host.py asserts that at most 1 % of a case's pixels go that way.
"""
import numpy as np
import torch

import splat_restated as R

MARGIN = 1e-3
MAX_LEFT_OUT = 0.01

# name -> scene arguments: the general cases of test_gpu_splat.py (image 40x56 = 3x4 tiles with half tiles last) and the special ones
CASES = {
    "sh1": dict(seed=11, d_sh=1),
    "sh4": dict(seed=12, d_sh=4),
    "sh25": dict(seed=13, d_sh=25),
    "plain": dict(seed=14, d_sh=9, scale_invariant=False),
    "one_tile": dict(seed=15, d_sh=4, G=700, H=16, W=16, V=1, spread=0.25, sigma=(0.01, 0.05)),
}


def _rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


def _draw(rng, n, d_sh, spread, sigma):
    means = np.stack([rng.uniform(-2.2, 2.2, n) * spread, rng.uniform(-1.6, 1.6, n) * spread, rng.uniform(-0.6, 5.0, n)], -1)
    L = rng.normal(size=(n, 3, 3)) * np.exp(rng.uniform(np.log(sigma[0]), np.log(sigma[1]), n))[:, None, None]
    covs = L @ L.transpose(0, 2, 1) + 1e-5 * np.eye(3)
    sh = rng.normal(size=(n, 3, d_sh)) * 0.25
    sh[:, :, 0] = rng.normal(size=(n, 3)) * 0.6
    opac = rng.uniform(0.05, 1.0, n)
    return [a.astype(np.float32) for a in (means, covs, sh, opac)]


def gaussian_margin(means, covs, sh, opac, cams, H, W, use_sh=True):
    """(G) the smallest Gaussian-level margin over the views, float64 restatement."""
    t = [torch.from_numpy(a).double() for a in (means, covs, sh, opac)]
    worst = torch.full((means.shape[0],), 1.0, dtype=torch.float64)
    for v in range(cams.shape[0]):
        p = R.preprocess(*t, torch.from_numpy(cams[v]), H, W, use_sh)
        m, front = p["margins"], p["depth"] > R.NEAR_Z
        rest = torch.minimum(torch.minimum(m["radius"], m["rect"]), torch.minimum(m["tan"], m["colour"]))
        worst = torch.minimum(worst, torch.minimum(m["z"], torch.where(front, rest, torch.ones_like(rest))))
    return worst.numpy()


def scene(seed, G=256, V=2, H=40, W=56, d_sh=25, scale_invariant=True, spread=1.0, sigma=(0.02, 0.2), shared_k=False):
    rng = np.random.RandomState(seed)
    ext = np.zeros((V, 4, 4), np.float32)
    K = np.zeros((V, 3, 3), np.float32)
    for v in range(V):
        ext[v, :3, :3] = _rot(rng.uniform(-0.1, 0.1), rng.uniform(-0.25, 0.25))
        ext[v, :3, 3] = rng.uniform(-0.3, 0.3, 3)
        ext[v, 3, 3] = 1
        K[v] = [[rng.uniform(0.8, 1.1), 0, rng.uniform(0.45, 0.55)], [0, rng.uniform(1.0, 1.4), rng.uniform(0.45, 0.55)], [0, 0, 1]]
    if shared_k:
        K[:] = K[0]
    near = rng.uniform(0.4, 0.6, V).astype(np.float32)
    far = rng.uniform(8.0, 12.0, V).astype(np.float32)
    bg = rng.uniform(0.0, 1.0, (V, 3)).astype(np.float32)
    cams = R.cameras(ext, K, near, far, scale_invariant)
    means, covs, sh, opac = _draw(rng, G, d_sh, spread, sigma)
    for _ in range(64):
        bad = np.nonzero(gaussian_margin(means, covs, sh, opac, cams, H, W) < MARGIN)[0]
        if bad.size == 0:
            break
        m2, c2, s2, o2 = _draw(rng, bad.size, d_sh, spread, sigma)
        means[bad], covs[bad], sh[bad], opac[bad] = m2, c2, s2, o2
    else:
        raise AssertionError("scene: Gaussians with an undecided decision remain")
    g_image = rng.normal(size=(V, 3, H, W)).astype(np.float32)
    return dict(means=means, covs=covs, sh=sh, opac=opac, extrinsics=ext, intrinsics=K, near=near, far=far, bg=bg, cams=cams, H=H, W=W,
                V=V, G=G, d_sh=d_sh, scale_invariant=scale_invariant, g_image=g_image)


def kept(info):
    """(V,H,W) bool: pixels whose every per-(pixel, Gaussian) decision has a relative margin of at least 1e-3."""
    return info["pixel"] >= MARGIN


def restate(sc, dtype=torch.float64, use_sh=True, grad=True):
    """The restatement on a scene -> dict(image, info, kept, grads of sum(image * g_image * kept) in means, covs, sh, opac).  The kept
    mask is always the float64 run's."""
    leaves = [torch.from_numpy(sc[k]).clone().requires_grad_(grad) for k in ("means", "covs", "sh", "opac")]
    image, info = R.render(*leaves, torch.from_numpy(sc["cams"]), torch.from_numpy(sc["bg"]), sc["H"], sc["W"], dtype, use_sh)
    out = dict(image=image.detach().numpy(), info=info)
    if dtype == torch.float64:
        out["kept"] = kept(info).numpy()
    return out, image, leaves


_CACHE = {}


def reference(name):
    """Computed once per case and shared, unchanged: the scene, the float64 and float32 restatements and their gradients."""
    if name in _CACHE:
        return _CACHE[name]
    sc = scene(**CASES[name])
    _CACHE[name] = (sc,) + with_gradients(sc)
    return _CACHE[name]


# ------------------------------------------------------------------------------------------- special scenes
def iso(sigma):
    return (np.eye(3) * sigma * sigma).tolist()


def special(means, covs, opac, sh=None, H=33, W=41, bg=(0.2, 0.3, 0.4), seed=3):
    """One identity camera (cx = cy = 0.5: the optical axis hits pixel (20, 16) exactly on 41x33), scale_invariant off, d_sh 1."""
    G = len(means)
    rng = np.random.RandomState(seed)
    ext = np.eye(4, dtype=np.float32)[None]
    K = np.array([[[0.9, 0, 0.5], [0, 1.1, 0.5], [0, 0, 1]]], np.float32)
    near, far = np.array([0.5], np.float32), np.array([10.0], np.float32)
    sh = (rng.normal(size=(G, 3, 1)) * 0.8).astype(np.float32) if sh is None else np.asarray(sh, np.float32)
    return dict(means=np.asarray(means, np.float32), covs=np.asarray(covs, np.float32), sh=sh, opac=np.asarray(opac, np.float32),
                extrinsics=ext, intrinsics=K, near=near, far=far, bg=np.array([bg], np.float32), H=H, W=W, V=1, G=G, d_sh=sh.shape[2],
                scale_invariant=False, cams=R.cameras(ext, K, near, far, False), g_image=rng.normal(size=(1, 3, H, W)).astype(np.float32))


def _culled():
    """behind the camera; z just under and just over the near bound 0.2; far off-screen; an empty tile rectangle just left of the image;
    two ordinary ones"""
    means = [[0.0, 0.0, -1.0], [0.01, 0.0, 0.1995], [0.0003, 0.01, 0.2005], [30.0, 0.0, 2.0], [-1.4, 0.0, 2.0], [0.1, -0.1, 1.5], [-0.2, 0.1, 2.5]]
    covs = [iso(0.05), iso(0.005), iso(0.005), iso(0.05), iso(0.002), iso(0.08), iso(0.1)]
    return special(means, covs, [0.9, 0.9, 0.9, 0.9, 0.9, 0.7, 0.6])


def _cap():
    """opacity 0; opacity 1 centred exactly on pixel (20, 16): opacity * exp(0) = 1 meets the 0.99 cap; one behind them"""
    return special([[0.3, 0.2, 2.0], [0.0, 0.0, 1.5], [0.05, 0.02, 3.0]], [iso(0.1), iso(0.06), iso(0.3)], [0.0, 1.0, 0.8])


def _stack():
    """six of opacity 0.95 centred on pixel (20, 16): T goes 0.05, 0.0025, 1.25e-4, the fourth would take it under 1e-4; the loss sits on
    that pixel alone"""
    G = 6
    sc = special([[0.0, 0.0, 1.0 + 0.25 * i] for i in range(G)], [iso(0.03 * (1.0 + 0.25 * i)) for i in range(G)], [0.95] * G)
    sc["g_image"] = np.zeros_like(sc["g_image"])
    sc["g_image"][0, :, 16, 20] = (1.0, -0.7, 0.4)
    return sc


def _equal_depths():
    """five overlapping Gaussians of one bit-equal depth between a nearer and a farther one"""
    means = [[0.02 * i - 0.04, 0.01 * i, 2.0] for i in range(5)] + [[0.004, 0.003, 1.2], [0.03, -0.02, 3.0]]
    return special(means, [iso(0.08)] * 5 + [iso(0.03), iso(0.3)], [0.6, 0.5, 0.7, 0.4, 0.8, 0.5, 0.9])


SPECIAL = {"culled": _culled, "cap": _cap, "stack": _stack, "equal_depths": _equal_depths}


def with_gradients(sc, use_sh=True):
    """(o64, o32, weights): both restatements of a scene with the gradients of sum(image * g_image * kept)."""
    o64, img64, l64 = restate(sc, torch.float64, use_sh)
    w = torch.from_numpy(sc["g_image"] * o64["kept"][:, None].astype(np.float32))
    o64["grads"] = [g.numpy() for g in torch.autograd.grad((img64 * w.double()).sum(), l64)]
    o32, img32, l32 = restate(sc, torch.float32, use_sh)
    o32["grads"] = [g.numpy() for g in torch.autograd.grad((img32 * w).sum(), l32)]
    return o64, o32, w.numpy()


def special_reference(name):
    key = "special:" + name
    if key not in _CACHE:
        sc = SPECIAL[name]()
        _CACHE[key] = (sc,) + with_gradients(sc)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------- edge scenes (test_gpu_splat_edges.py)
LIST_LENGTHS = (63, 64, 65, 255, 256, 257)            # one under, at and one over the backward's and the forward's LDS batch
SMALL_IMAGES = ((1, 1), (5, 7), (16, 17), (17, 16), (15, 33), (32, 48))
BIT_SHAPES = ((2, 16, 16), (3, 16, 16), (4, 16, 16), (2, 32, 32), (4, 32, 32))       # V * tiles = 2, 3, 4, 8, 16
PAD_SIZES = (257, 511, 513, 1000)
BEHIND = (0.0, 0.0, -1.0)                             # a mean behind every camera that `scene` draws


def visible(sc):
    """(V,G) bool: not culled, by the float64 restatement's preprocess."""
    t = [torch.from_numpy(sc[k]).double() for k in ("means", "covs", "sh", "opac")]
    return np.stack([R.preprocess(*t, torch.from_numpy(sc["cams"][v]), sc["H"], sc["W"])["ok"].numpy() for v in range(sc["V"])])


def subset(sc, idx):
    """The scene of the Gaussians idx, in that order."""
    idx = np.asarray(idx)
    return dict(sc, G=int(idx.size), **{k: np.ascontiguousarray(sc[k][idx]) for k in ("means", "covs", "sh", "opac")})


def spread_out(sc, G, at):
    """The scene's Gaussians at the ascending indices `at` of a set of G; every other one sits behind the cameras and is culled."""
    at = np.asarray(at)
    assert at.size == sc["G"] and (np.diff(at) > 0).all() and at[0] >= 0 and at[-1] < G
    means = np.tile(np.asarray(BEHIND, np.float32), (G, 1))
    covs = np.tile(np.eye(3, dtype=np.float32) * np.float32(0.01), (G, 1, 1))
    sh = np.full((G, 3, sc["d_sh"]), 0.25, np.float32)
    opac = np.full(G, 0.5, np.float32)
    for big, k in zip((means, covs, sh, opac), ("means", "covs", "sh", "opac")):
        big[at] = sc[k]
    return dict(sc, G=G, means=means, covs=covs, sh=sh, opac=opac)


def padded(sc, G, where, seed=23):
    """spread_out with the padding in front of the live Gaussians ("front": they come last), behind them ("behind": they come first) or
    around them, at seeded indices that include 0 and G - 1 ("interleaved") -> (scene, the live indices)."""
    n = sc["G"]
    if where == "front":
        at = np.arange(G - n, G)
    elif where == "behind":
        at = np.arange(n)
    else:
        inner = np.random.RandomState(seed).choice(np.arange(1, G - 1), n - 2, replace=False)
        at = np.sort(np.concatenate([[0, G - 1], inner]))
    return spread_out(sc, G, at), at


def both_views(sc):
    """The first Gaussian that no view culls."""
    return int(np.nonzero(visible(sc).all(0))[0][0])


def _list(n):
    """the first n non-culled Gaussians of `one_tile` (16x16, one view): one key each, a tile list of exactly n entries"""
    def build():
        sc = scene(**CASES["one_tile"])
        return subset(sc, np.nonzero(visible(sc)[0])[0][:n])
    return build


def _first(n):
    """sh4 cut to its first n Gaussians; n = 1 keeps the first that no view culls"""
    def build():
        sc = scene(**CASES["sh4"])
        return subset(sc, [both_views(sc)] if n == 1 else np.arange(n))
    return build


def small_image(h, w):
    return scene(seed=41, G=96, V=2, d_sh=4, H=h, W=w)


def bit_scene(V, H, W):
    return scene(seed=43, G=96, V=V, d_sh=4, H=H, W=W)


def _front():
    """a small nearest Gaussian at pixel (24, 8), radius 4, well inside tile (1, 0) of 41x33; three ordinary ones behind it that
    cover the image centre"""
    tanx, tany = 0.5 / 0.9, 0.5 / 1.1
    x, y = (49.0 / 41.0 - 1.0) * tanx, (17.0 / 33.0 - 1.0) * tany
    return special([[x, y, 1.0], [0.05, 0.02, 2.0], [-0.1, 0.05, 3.0], [0.1, -0.12, 2.5]],
                   [iso(0.02), iso(0.25), iso(0.45), iso(0.3)], [0.8, 0.7, 0.9, 0.6])


EDGES = {f"list{n}": _list(n) for n in LIST_LENGTHS}
EDGES.update({"first1": _first(1), "first255": _first(255), "front": _front})
EDGES.update({f"small{h}x{w}": (lambda h=h, w=w: small_image(h, w)) for h, w in SMALL_IMAGES})
EDGES.update({f"bits{v}x{h}x{w}": (lambda v=v, h=h, w=w: bit_scene(v, h, w)) for v, h, w in BIT_SHAPES})


def edge_reference(name):
    key = "edge:" + name
    if key not in _CACHE:
        sc = EDGES[name]()
        _CACHE[key] = (sc,) + with_gradients(sc)
    return _CACHE[key]
