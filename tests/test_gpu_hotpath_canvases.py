"""The hot path's own kernels (stages a1-a10: pack.h, planesweep.hip, planesweep_bwd.hip, depthprob.hip, backproject.hip) called
through the C ABI inside guarded memory (tests/canvas.py), as test_gpu_conv_edges.py does for the cost network:

  * every input sits in a NaN frame: strided inputs (features, est_depth / est_dens crops, the (N, 2, D, H, W) logits) as views
    with NaN in every gap, dense inputs (packed maps, projections, planes, cotangents) exactly as long as the ABI says with NaN
    on both sides -- a read one texel past a footprint box, the row after the last, or channel C of a ragged slab lands in owned
    memory and shows up as NaN instead of being multiplied by a zero weight;
  * every output, scratch buffer and workspace is exactly as long as its size query says and sits between 1 MiB guards of a fixed
    bit pattern; outputs start out as NaN, so a word the kernel should have written and did not shows up too.

Per case: (a) guards intact, (b) the bits of the same call on clean framework-allocated buffers through mvsdet_amd.ops (for the
float atomics of the backward sweep and the backproject backward: the tolerance of test_gpu_corners._check_bwd), (c) NaN only
where the clean run has NaN.  Every call is a legal one whose documented sizes are honoured."""
import ctypes

import numpy as np
import pytest
import torch

from canvas import GUARD, SENTINEL, Guarded, guarded_f32, nan_view, ok, strides

pytestmark = pytest.mark.gpu

NAN_WORD = 0x7FC00000
FRAME = 1 << 14          # NaN words on each side of a dense input


def framed(t, dev):
    """A dense copy of t, exactly t.numel() long, between NaN: (canvas, tensor).  4-byte element types only."""
    t = t.contiguous()
    n = t.numel()
    assert t.element_size() == 4
    canvas = torch.full((FRAME + n + FRAME,), NAN_WORD, dtype=torch.int32, device=dev)
    region = canvas[FRAME:FRAME + n].view(t.dtype)
    region.copy_(t.reshape(-1))
    return canvas, region.view(t.shape)


def crop4(x, dev, **gaps):
    """x (N, C, H, W) as a strided view with NaN in the row pitch, between channels and between views."""
    canvas, v = nan_view(x.unsqueeze(2), dev, **gaps)
    return canvas, v[:, :, 0]


def out_f32(shape, dev, fill=NAN_WORD):
    g, v = guarded_f32(shape, dev)
    g.region.fill_(fill)
    return g, v


def out_words(nwords, dev, fill=NAN_WORD):
    g = Guarded(nwords, dev)
    g.region.fill_(fill)
    return g


def same(a, b, what=""):
    """Equal bit for bit; a NaN for a NaN."""
    a, b = a.reshape(-1), b.reshape(-1)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"{what}: NaN in other places than the clean run ({int(na.sum())} vs {int(nb.sum())})"
    assert torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)), f"{what}: other bits than the clean run"


def close(a, b, what=""):
    """The tolerance of test_gpu_corners._check_bwd (float atomics: the order of the additions is not fixed)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"{what}: NaN in other places than the clean run"
    scale = float(b[~nb].abs().max()) if (~nb).any() else 0.0
    torch.testing.assert_close(a[~na], b[~nb], rtol=1e-4, atol=2e-5 * max(scale, 1.0), msg=lambda m: f"{what}: {m}")


def intact(*gs):
    for i, g in enumerate(gs):
        assert g.guards_intact(), f"guard of buffer {i} overwritten"


def L():
    from mvsdet_amd import _lib
    return _lib.load()


def S(dev):
    from mvsdet_amd import _lib
    return _lib.current_stream(dev)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


# --------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("C", [5, 32, 33, 256])
@pytest.mark.parametrize("H,W", [(6, 8), (5, 7)])      # H * W a multiple of 4 (the float4 kernel's shape) and not
def test_pack_features_in_canvases(gpu, C, H, W, half):
    from mvsdet_amd import ops
    N = 2
    x = torch.randn((N, C, H, W), generator=torch.Generator().manual_seed(C + W))
    canvas, v = crop4(x, gpu)
    if half:
        c16 = canvas.half()
        v = c16.as_strided(v.shape, v.stride(), v.storage_offset())
        x = x.half()
    lib = L()
    nbytes = lib.mvsdet_packed_bytes(N, C, H, W)
    g = out_words(nbytes // 4, gpu)
    fn = lib.mvsdet_pack_features_f16 if half else lib.mvsdet_pack_features_f32
    ok(fn(P(v), strides(v), g.ptr(), N, C, H, W, S(gpu)))
    intact(g)
    got = g.region.view(torch.float32)
    assert not torch.isnan(got).any(), "a packed word is NaN: read outside the crop, or never written"
    same(got, ops.pack_features(x.to(gpu)), "pack")
    Sl = (C + 31) // 32
    q = got.view(N, Sl, H, W, 8, 4)                      # [n][s][y][x][g][i] holds channel 32 s + 8 i + g
    ch = (32 * torch.arange(Sl).view(Sl, 1, 1) + 8 * torch.arange(4).view(1, 1, 4) + torch.arange(8).view(1, 8, 1)).to(gpu)
    pad = (ch >= C).view(1, Sl, 1, 1, 8, 4).expand_as(q)
    assert float(q[pad].abs().max()) == 0.0 if pad.any() else True, "the padded channels of the last slab must be zero"


# --------------------------------------------------------------------------------------------- sweep
def _scene(N, K, C, D, H, W, seed=5):
    from mvsdet_amd import functional as F_, synthetic
    from oracle import oracle
    meta = synthetic.make_img_meta(N, (H, W), seed=seed)
    feat = synthetic.make_features(N, C, (H, W), seed=seed)
    rng = np.random.default_rng(7)
    nbr = np.stack([rng.permutation([j for j in range(N) if j != n] * 4)[:K] for n in range(N)]).astype(np.int64).reshape(N, K)
    w2c = torch.tensor(np.array(meta["lidar2img"]["extrinsic"]))
    Kf = torch.tensor(oracle.feat_intrinsics(meta["lidar2img"]["intrinsic"], meta["img_shape"], meta["ori_shape"]))
    ref_proj, nei = F_.collect_proj(w2c, Kf, torch.tensor(nbr)) if K else (None, ())
    proj = torch.stack([torch.matmul(p, torch.inverse(ref_proj)) for p in nei], 1) if K else torch.zeros(N, 0, 4, 4)
    depth = torch.tensor(oracle.depth_planes(0.2, 5.0, D)).unsqueeze(0).repeat(N, 1)
    return feat, torch.tensor(nbr), proj, depth


def _degenerate():
    """The projections of test_gpu_parity.test_sweep_degenerate_geometry."""
    N, K, C, D, H, W = 3, 2, 8, 4, 12, 16
    feat = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(5))
    nbr = torch.tensor([[1, 2], [2, 0], [0, 1]])
    proj = torch.eye(4).repeat(N, K, 1, 1)
    proj[0, 0, 2, :] = 0.0
    proj[0, 1, 2, :] = torch.tensor([0.0, 0.0, -1.0, -0.5])
    proj[1, 0, 0, 3] = 1e6
    proj[1, 1, :3, :3] *= 40.0
    proj[2, 0, 0, 3], proj[2, 0, 1, 3] = 3.3, -2.1
    return feat, nbr, proj, torch.tensor([0.5, 1.0, 2.0, 4.0]).repeat(N, 1)


def _over_capacity():
    """The projections of test_gpu_corners.test_backward_stage1_over_box_capacity, on a smaller channel count."""
    N, K, C, H, W = 4, 2, 40, 40, 48
    feat = torch.from_numpy(np.random.default_rng(5).standard_normal((N, C, H, W)).astype(np.float32))
    nbr = torch.tensor([[1, 2], [2, 3], [3, 0], [0, 1]])
    proj = np.tile(np.eye(4, dtype=np.float32), (N, K, 1, 1))
    proj[0, 0, :2, :2] *= 3.0
    proj[0, 1, :2, :2] *= 0.25
    proj[0, 1, :2, 3] = (10.0, 7.0)
    proj[1, 0, :2, :2] *= 6.0
    proj[1, 1, :2, 3] = (2.5, -1.25)
    proj[2, 0, :2, :2] = np.array([[0.8, -0.6], [0.6, 0.8]], np.float32) * 2.5
    proj[2, 1, :2, 3] = (1e5, 0.0)
    proj[3, 0, 2, :2] = (0.01, -0.02)
    proj[3, 1, 2, :] = (0.0, 0.0, -1.0, -0.5)                                      # z <= 0
    return feat, nbr, torch.from_numpy(proj), torch.tensor([[0.5, 1.0, 2.0]]).repeat(N, 1)


GEOMETRIES = {
    "33x47": lambda: _scene(3, 2, 20, 5, 33, 47), "21x80": lambda: _scene(3, 2, 20, 6, 21, 80),
    "9x48_k4": lambda: _scene(5, 4, 20, 4, 9, 48), "12x16_c300": lambda: _scene(2, 2, 300, 3, 12, 16),
    "k0": lambda: _scene(2, 0, 20, 3, 12, 16), "k1": lambda: _scene(3, 1, 20, 2, 9, 48),
    "degenerate": _degenerate, "over_capacity": _over_capacity,
}
OPTIONS = [(tw, cap) for tw in (16, 32) for cap in (0, 40, None)]


class _options:
    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        from mvsdet_amd import _lib
        self.saved = {k: _lib.get_option(k) for k in ("sweep_tw", "sweep_boxcap", "bwd_groups")}
        for k, v in self.kv.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        from mvsdet_amd import _lib
        for k, v in self.saved.items():
            _lib.set_option(k, v)


@pytest.mark.parametrize("tw,cap", OPTIONS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_sweep_forward_in_canvases(gpu, name, tw, cap):
    from mvsdet_amd import ops
    feat, nbr, proj, depth = GEOMETRIES[name]()
    N, C, H, W = feat.shape
    K, D = nbr.shape[1], depth.shape[1]
    lib = L()
    with _options(sweep_tw=tw, sweep_boxcap=cap):
        nbr_d, featg = nbr.to(gpu), feat.to(gpu)
        clean_packed = ops.pack_features(featg)
        clean = ops.plane_sweep_variance_packed(clean_packed, nbr_d, proj.to(gpu), depth.to(gpu), C, H, W)
        assert clean_packed.numel() * 4 == lib.mvsdet_packed_bytes(N, C, H, W)
        c1, packed = framed(clean_packed, gpu)
        c2, proj_f = framed(proj, gpu)
        c3, depth_f = framed(depth, gpu)
        sbytes = lib.mvsdet_plane_sweep_scratch_bytes(N, K, D, H, W)
        assert sbytes % 16 == 0 and (sbytes > 0) == (K > 0)          # no neighbour: no geometry, nothing to write
        # geometry + per-channel sweep
        gs, (go, out) = out_words(sbytes // 4, gpu), out_f32((N, C, D, H, W), gpu)
        ok(lib.mvsdet_plane_sweep_table_f32(P(proj_f), P(depth_f), gs.ptr(), sbytes, N, K, D, H, W, S(gpu)))
        ok(lib.mvsdet_plane_sweep_variance_tabled_f32(P(packed), P(nbr_d), gs.ptr(), sbytes, P(out), N, K, C, D, H, W, S(gpu)))
        intact(gs, go)
        same(out, clean, "tabled")
        # the same into a row-pitched volume: the pad columns keep their fill
        wp = ops.sweep_row_pitch(W) if W % 32 else W + 32
        gs2, (gp, outp) = out_words(sbytes // 4, gpu), out_f32((N, C, D, H, wp), gpu, fill=SENTINEL)
        ok(lib.mvsdet_plane_sweep_table_pitched_f32(P(proj_f), P(depth_f), gs2.ptr(), sbytes, N, K, D, H, W, wp, S(gpu)))
        ok(lib.mvsdet_plane_sweep_variance_tabled_pitched_f32(P(packed), P(nbr_d), gs2.ptr(), sbytes, P(outp), N, K, C, D, H, W, wp,
                                                              S(gpu)))
        intact(gs2, gp)
        same(outp[..., :W].contiguous(), clean, "pitched")
        assert bool((outp[..., W:].contiguous().view(torch.int32) == SENTINEL).all()), "the pitch padding was written"
        # one call (geometry + sweep), and the view shard of views 1 .. N-1 in fp32 and fp16
        gs3, (go3, out3) = out_words(sbytes // 4, gpu), out_f32((N, C, D, H, W), gpu)
        ok(lib.mvsdet_plane_sweep_variance_packed_f32(P(packed), P(nbr_d), P(proj_f), P(depth_f), P(out3), gs3.ptr(), sbytes, N, K, C,
                                                      D, H, W, S(gpu)))
        intact(gs3, go3)
        same(out3, clean, "packed")
        M = N - 1
        mbytes = lib.mvsdet_plane_sweep_scratch_bytes(M, K, D, H, W)
        c4, proj_m = framed(proj[1:], gpu)
        c5, depth_m = framed(depth[1:], gpu)
        nbr_m = nbr_d[1:].contiguous()
        gs4, (go4, out4) = out_words(mbytes // 4, gpu), out_f32((M, C, D, H, W), gpu)
        ok(lib.mvsdet_plane_sweep_variance_shard_f32(P(packed), P(nbr_m), P(proj_m), P(depth_m), P(out4), gs4.ptr(), mbytes, N, 1, M,
                                                     K, C, D, H, W, S(gpu)))
        intact(gs4, go4)
        same(out4, clean[1:], "shard")
        nh = M * C * D * H * W
        gs5, gh = out_words(mbytes // 4, gpu), out_words((nh + 1) // 2, gpu, fill=0x7E007E00)      # two fp16 NaNs a word
        ok(lib.mvsdet_plane_sweep_variance_shard_f16(P(packed), P(nbr_m), P(proj_m), P(depth_m), gh.ptr(), gs5.ptr(), mbytes, N, 1, M,
                                                     K, C, D, H, W, S(gpu)))
        intact(gs5, gh)
        clean_h = ops.plane_sweep_variance_shard(clean_packed, nbr_m, proj[1:].to(gpu), depth[1:].to(gpu), N, 1, C, H, W, half_out=True)
        got_h = gh.region.view(torch.float16)[:nh]
        assert torch.equal(torch.isnan(got_h), torch.isnan(clean_h.reshape(-1)))
        assert torch.equal(torch.nan_to_num(got_h).view(torch.int16), torch.nan_to_num(clean_h.reshape(-1)).view(torch.int16))
        # from the dense feature maps: packs into the workspace first
        wbytes = lib.mvsdet_plane_sweep_workspace_bytes(N, K, C, D, H, W)
        c6, feat_f = framed(feat, gpu)
        gw, (go6, out6) = out_words(wbytes // 4, gpu), out_f32((N, C, D, H, W), gpu)
        ok(lib.mvsdet_plane_sweep_variance_f32(P(feat_f), P(nbr_d), P(proj_f), P(depth_f), P(out6), gw.ptr(), wbytes, N, K, C, D, H, W,
                                               S(gpu)))
        intact(gw, go6)
        same(out6, clean, "from dense maps")


@pytest.mark.parametrize("name", ["33x47", "k1", "degenerate", "over_capacity"])
def test_homo_warp_in_canvases(gpu, name):
    from mvsdet_amd import ops
    feat, nbr, proj, depth = GEOMETRIES[name]()
    B, C, H, W = feat.shape
    D = depth.shape[1]
    p0 = proj[:, 0].contiguous()
    clean = ops.homo_warp(feat.to(gpu), p0.to(gpu), depth.to(gpu))
    c1, src = framed(feat, gpu)
    c2, pf = framed(p0, gpu)
    c3, df = framed(depth, gpu)
    go, out = out_f32((B, C, D, H, W), gpu)
    ok(L().mvsdet_homo_warp_f32(P(src), P(pf), P(df), P(out), B, C, D, H, W, S(gpu)))
    intact(go)
    same(out, clean, "homo_warp")


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("tw,cap", [(16, None), (32, None), (16, 0), (32, 40)])
@pytest.mark.parametrize("name", [n for n in GEOMETRIES if n != "k0"])      # no neighbour: nothing to differentiate
def test_sweep_backward_in_canvases(gpu, name, tw, cap, groups):
    from mvsdet_amd import ops
    feat, nbr, proj, depth = GEOMETRIES[name]()
    N, C, H, W = feat.shape
    K, D = nbr.shape[1], depth.shape[1]
    lib = L()
    R = torch.randn((N, C, D, H, W), generator=torch.Generator().manual_seed(1))
    with _options(sweep_tw=tw, sweep_boxcap=cap, bwd_groups=groups):
        nbr_d, featg = nbr.to(gpu), feat.to(gpu)
        clean_packed = ops.pack_features(featg)
        table = ops.plane_sweep_table(proj.to(gpu), depth.to(gpu), H, W)
        clean = ops.plane_sweep_variance_backward_packed(clean_packed, nbr_d, table, R.to(gpu))
        sbytes = lib.mvsdet_plane_sweep_scratch_bytes(N, K, D, H, W)
        c1, packed = framed(clean_packed, gpu)
        c2, proj_f = framed(proj, gpu)
        c3, depth_f = framed(depth, gpu)
        c4, g = framed(R, gpu)
        gs = out_words(sbytes // 4, gpu)
        ok(lib.mvsdet_plane_sweep_table_f32(P(proj_f), P(depth_f), gs.ptr(), sbytes, N, K, D, H, W, S(gpu)))
        pb = (int(lib.mvsdet_packed_bytes(N, C, H, W)) + 255) // 256 * 256
        gw, (gg, gfeat) = out_words(pb // 4, gpu), out_f32((N, C, H, W), gpu)
        ok(lib.mvsdet_plane_sweep_variance_bwd_packed_f32(P(packed), P(nbr_d), gs.ptr(), sbytes, P(g), P(gfeat), gw.ptr(), pb, N, K, C,
                                                          D, H, W, S(gpu)))
        intact(gs, gw, gg)
        close(gfeat, clean, "bwd_packed")
        # from the dense maps, with the workspace the size query names
        wbytes = lib.mvsdet_plane_sweep_bwd_workspace_bytes(N, K, C, D, H, W)
        c5, feat_f = framed(feat, gpu)
        gw2, (gg2, gfeat2) = out_words(wbytes // 4, gpu), out_f32((N, C, H, W), gpu)
        ok(lib.mvsdet_plane_sweep_variance_bwd_f32(P(feat_f), P(nbr_d), P(proj_f), P(depth_f), P(g), P(gfeat2), gw2.ptr(), wbytes, N, K,
                                                   C, D, H, W, S(gpu)))
        intact(gw2, gg2)
        close(gfeat2, clean, "bwd")


# --------------------------------------------------------------------------------------------- stage 2
@pytest.mark.parametrize("D,topk", [(12, 3), (12, 8), (65, 3), (65, 8)])
@pytest.mark.parametrize("H,W", [(1, 1), (15, 17), (1, 257)])
def test_stage2_in_canvases(gpu, D, topk, H, W):
    from mvsdet_amd import ops
    N, HW = 3, H * W
    near, iv = 0.2, 4.8 / D
    lib = L()
    both = torch.randn((N, 2, D, H, W), generator=torch.Generator().manual_seed(D + W))
    both[:, 0] *= 3
    gap = 37
    vs = 2 * (D * HW + gap)                                           # view stride > D * H * W
    lead = 256
    canvas = torch.full((lead + N * vs + lead,), float("nan"), device=gpu)
    cost = canvas.as_strided((N, D, H, W), (vs, HW, W, 1), lead)
    offl = canvas.as_strided((N, D, H, W), (vs, HW, W, 1), lead + D * HW + gap)
    cost.copy_(both[:, 0])
    offl.copy_(both[:, 1])
    clean = ops.depth_prob_topk(both[:, 0].to(gpu), both[:, 1].to(gpu), near, iv, topk)
    (g0, prob), (g1, off) = out_f32((N, D, H, W), gpu), out_f32((N, D, H, W), gpu)
    (g2, ed), (g3, en), (g5, av) = out_f32((N, topk, H, W), gpu), out_f32((N, topk, H, W), gpu), out_f32((N, H, W), gpu)
    g4 = out_words(N * topk * HW, gpu, fill=-1)
    fl = ctypes.c_float
    ok(lib.mvsdet_depth_prob_topk_strided_f32(P(cost), P(offl), vs, P(prob), P(off), P(ed), P(en), g4.ptr(), P(av), N, D, H, W, topk,
                                              fl(near), fl(iv), S(gpu)))
    intact(g0, g1, g2, g3, g4, g5)
    ei = g4.region.view(N, topk, H, W)
    for got, want, what in zip((prob, off, ed, en, av), (clean[0], clean[1], clean[2], clean[3], clean[5]),
                               ("prob", "off", "est_depth", "est_dens", "avg_depth")):
        assert not torch.isnan(got).any(), f"{what}: NaN from outside the views, or a word never written"
        same(got, want, what)
    assert torch.equal(ei, clean[4])
    # a6 + a7 alone on dense framed prob / off
    c1, pf = framed(clean[0], gpu)
    c2, of = framed(clean[1], gpu)
    (h2, ed2), (h3, en2), (h5, av2) = out_f32((N, topk, H, W), gpu), out_f32((N, topk, H, W), gpu), out_f32((N, H, W), gpu)
    h4 = out_words(N * topk * HW, gpu, fill=-1)
    ok(lib.mvsdet_sample_depth_prob_f32(P(pf), P(of), P(ed2), P(en2), h4.ptr(), P(av2), N, D, H, W, topk, fl(near), fl(iv), S(gpu)))
    intact(h2, h3, h4, h5)
    for got, want in zip((ed2, en2, h4.region.view(N, topk, H, W), av2), ops.sample_depth_prob(clean[0], clean[1], near, iv, topk)):
        assert torch.equal(got, want)
    # backward
    gen = torch.Generator().manual_seed(2)
    cots = [torch.randn(s, generator=gen) for s in ((N, D, H, W), (N, topk, H, W), (N, topk, H, W), (N, H, W))]
    want = ops.depth_prob_topk_backward(clean[0], clean[1], clean[4], *[c.to(gpu) for c in cots], near, iv)
    fr = [framed(c, gpu) for c in cots]
    c3, idx_f = framed(clean[4], gpu)
    (k0, gc), (k1, gofl) = out_f32((N, D, H, W), gpu), out_f32((N, D, H, W), gpu)
    ok(lib.mvsdet_depth_prob_topk_bwd_f32(P(pf), P(of), P(idx_f), P(fr[0][1]), P(fr[1][1]), P(fr[2][1]), P(fr[3][1]), P(gc), P(gofl), N,
                                          D, H, W, topk, fl(near), fl(iv), S(gpu)))
    intact(k0, k1)
    same(gc, want[0], "d/d cost logits")
    same(gofl, want[1], "d/d offset logits")
    assert not torch.isnan(gc).any() and not torch.isnan(gofl).any()


# --------------------------------------------------------------------------------------------- stage 3
def test_stage3_in_canvases(gpu):
    """65 views (two mask chunks), V = 257 (no multiple of the 32-voxel or the 256-voxel tile), features and candidate maps as
    strided crops with NaN beyond the crop."""
    from mvsdet_amd import ops
    from test_gpu_lift_forward_edges import VZ, _stage3_fixture
    N, C, J, V = 65, 40, 3, 257
    fx = _stage3_fixture(N, C, J, V, (6, 7), seed=3)
    h, w, H, W = fx["h"], fx["w"], fx["H"], fx["W"]
    dens_np = np.nan_to_num(fx["dens"], nan=0.3)
    dens_np[:, :, 1, 1] = 0.2
    feat, depth, dens = torch.from_numpy(fx["feat"]), torch.from_numpy(np.nan_to_num(fx["depth"], nan=2.0)), torch.from_numpy(dens_np)
    pts, proj = torch.from_numpy(fx["pts"]), torch.from_numpy(np.nan_to_num(fx["proj"], nan=0.5))
    lib, fl = L(), ctypes.c_float
    # clean
    fg, dg, ng, ptg, prg = [t.to(gpu) for t in (feat, depth, dens, pts, proj)]
    fcrop, dcrop, ncrop = fg[:, :, :h, :w], dg[:, :, :h, :w], ng[:, :, :h, :w]
    vol, valid = ops.backproject_weigh(fcrop, ptg, prg, dcrop, ncrop, VZ)
    packed_clean = ops.pack_features(fg)
    mean, count = ops.backproject_weigh_mean(fcrop, packed_clean, ptg, prg, dcrop, ncrop, H, W, VZ)
    total, count_s = ops.backproject_weigh_sum_shard(packed_clean, ptg, prg, dcrop, ncrop, N, 0, C, H, W, VZ)
    assert 0.05 < float(valid.float().mean()) < 0.95 and int(count.max()) > 1
    # framed: only the (h, w) crops exist, inside NaN
    cf, fv = crop4(feat[:, :, :h, :w], gpu)
    cd, dv = crop4(depth[:, :, :h, :w], gpu)
    cn, nv = crop4(dens[:, :, :h, :w], gpu)
    assert dv.stride() == nv.stride()
    c1, pts_f = framed(pts, gpu)
    c2, proj_f = framed(proj, gpu)
    (g0, vol2), g1 = out_f32((N, C, V), gpu), out_words((N * V + 3) // 4, gpu, fill=0x02020202)
    g2, g3 = out_words(N * V, gpu), out_words(N * V, gpu)
    ok(lib.mvsdet_backproject_weigh_f32(P(fv), strides(fv), P(pts_f), P(proj_f), P(dv), P(nv), strides(dv), P(vol2), g1.ptr(), g2.ptr(),
                                        g3.ptr(), N, C, h, w, V, J, fl(VZ), S(gpu)))
    intact(g0, g1, g2, g3)
    same(vol2, vol, "volume")
    assert not torch.isnan(vol2).any()
    assert torch.equal(g1.region.view(torch.uint8)[:N * V].view(N, V), valid.to(torch.uint8))
    # the fused forms read the packed full-size maps
    full = torch.full((N, C, H, W), float("nan"))
    full[:, :, :h, :w] = feat[:, :, :h, :w]
    c3, packed = framed(ops.pack_features(full.to(gpu)), gpu)                 # NaN where the crop ends, too
    for fn, want, wcount in ((lib.mvsdet_backproject_weigh_mean_packed_f32, mean, count),
                             (lib.mvsdet_backproject_weigh_sum_packed_f32, total, count_s)):
        (m0, out), m1 = out_f32((C, V), gpu), out_words(V, gpu, fill=-1)
        ok(fn(P(packed), P(pts_f), P(proj_f), P(dv), P(nv), strides(dv), P(out), m1.ptr(), N, C, H, W, h, w, V, J, fl(VZ), S(gpu)))
        intact(m0, m1)
        same(out, want, "fused")
        assert not torch.isnan(out).any() and torch.equal(m1.region, wcount)
    # backward, both forms
    gen = torch.Generator().manual_seed(4)
    gv, gm = torch.randn((N, C, V), generator=gen), torch.randn((C, V), generator=gen)
    want_v = ops.backproject_weigh_backward(fcrop, ptg, prg, dcrop, ncrop, VZ, gv.to(gpu))
    want_m = ops.backproject_weigh_mean_backward(fcrop, ptg, prg, dcrop, ncrop, count, VZ, gm.to(gpu))
    c4, gv_f = framed(gv, gpu)
    c5, gm_f = framed(gm, gpu)
    c6, cnt_f = framed(count, gpu)
    (b0, gf), (b1, gd) = out_f32((N, C, h, w), gpu), out_f32((N, J, h, w), gpu)
    ok(lib.mvsdet_backproject_weigh_bwd_f32(P(fv), strides(fv), P(pts_f), P(proj_f), P(dv), P(nv), strides(dv), P(gv_f), P(gf), P(gd), N,
                                            C, h, w, V, J, fl(VZ), S(gpu)))
    intact(b0, b1)
    close(gf, want_v[0], "per-view d/d feat")
    close(gd, want_v[1], "per-view d/d dens")
    (b2, gf2), (b3, gd2) = out_f32((N, C, h, w), gpu), out_f32((N, J, h, w), gpu)
    ok(lib.mvsdet_backproject_weigh_mean_bwd_f32(P(fv), strides(fv), P(pts_f), P(proj_f), P(dv), P(nv), strides(dv), P(cnt_f), P(gm_f),
                                                 P(gf2), P(gd2), N, C, h, w, V, J, fl(VZ), S(gpu)))
    intact(b2, b3)
    close(gf2, want_m[0], "mean d/d feat")
    close(gd2, want_m[1], "mean d/d dens")
    for t in (gf, gd, gf2, gd2):
        assert not torch.isnan(t).any()


# --------------------------------------------------------------------------------------------- ray_depth
@pytest.mark.parametrize("J", [0, 3])
def test_ray_depth_in_canvases(gpu, J):
    from mvsdet_amd import ops
    N, H, W, h, w = 3, 13, 21, 11, 18
    intr = torch.tensor([[20.0, 19.0, 9.3, 5.1, 0.0], [15.5, 16.5, 8.0, 6.0, 0.7], [31.0, 29.0, 2.5, 9.5, -1.3]])
    est = None
    if J:
        est = torch.rand((N, J, H, W), generator=torch.Generator().manual_seed(J)) * 4.8 + 0.2
        est[:, :, h:] = float("nan")
        est[:, :, :, w:] = float("nan")
    scale, ray = ops.ray_depth(intr.to(gpu), None if est is None else est.to(gpu), h, w)
    c1, intr_f = framed(intr, gpu)
    g0, sc = out_f32((N, h * w, 1), gpu)
    if J:
        c2, est_f = framed(est, gpu)
        g1, rd = out_f32((N, J, h * w), gpu)
    ok(L().mvsdet_ray_depth_f32(P(intr_f), P(est_f) if J else None, P(sc), P(rd) if J else None, N, J, H, W, h, w, S(gpu)))
    intact(g0)
    same(sc, scale, "depth_scale")
    assert not torch.isnan(sc).any()
    if J:
        intact(g1)
        same(rd, ray.squeeze(2).transpose(2, 1).contiguous(), "est_ray_depth")
        assert not torch.isnan(rd).any(), "the NaN padding of est_depth was read"
