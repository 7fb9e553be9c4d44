"""Parity tests proper: the HIP kernels (through the C ABI, via mvsdet_amd.ops / functional) against the CPU
oracle on the same seeded inputs, and against the committed golden vectors of the reference.

Bars (BASELINE.json north_star): fp32 outputs within 1e-4 of the reference; voxel indices bit-exact.
Where the oracle and the kernel share rounding points the tests demand bit-for-bit equality instead.
Nothing here reads /root/reference.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-4  # north_star tolerance, fp32


def dev(a, gpu, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(gpu)


# --------------------------------------------------------------------------------------------- a3
def test_homo_warp_vs_golden_and_oracle(gpu, oracle):
    from mvsdet_amd import functional as F_, ops
    g = load_golden("g1_homo_warping")
    out = ops.homo_warp(dev(g["src_fea"], gpu), dev(g["proj_rel"], gpu), dev(g["depth_values"], gpu)).cpu().numpy()
    ref = oracle.homo_warp(g["src_fea"], g["proj_rel"], g["depth_values"])
    np.testing.assert_array_equal(out, ref)  # identical rounding points -> identical bits
    np.testing.assert_allclose(out, g["warped"], rtol=0, atol=TOL)
    # reference signature (mvs_models/module.py:105): proj computed on the host from src_proj / ref_proj
    out2 = F_.homo_warping(dev(g["src_fea"], gpu), dev(g["src_proj"], gpu), dev(g["ref_proj"], gpu),
                           dev(g["depth_values"], gpu)).cpu().numpy()
    np.testing.assert_allclose(out2, g["warped"], rtol=0, atol=TOL)
    assert out2.shape == g["warped"].shape


# --------------------------------------------------------------------------------------------- a3+a4
@pytest.mark.parametrize("tag", ["n3_d8", "n2_k1", "n6_d12_arkit"])
def test_plane_sweep_variance_golden(gpu, oracle, tag):
    from mvsdet_amd import ops
    g = load_golden("g2_variance_" + tag)
    cs = int(g["variance_channel_stride"])
    var = ops.plane_sweep_variance(dev(g["feature"], gpu), dev(g["neighbor_ids"], gpu), dev(g["proj_rel"], gpu),
                                   dev(g["depth_values"], gpu)).cpu().numpy()
    np.testing.assert_allclose(var[:, ::cs], g["variance"], rtol=0, atol=TOL)
    ref = oracle.plane_sweep_variance(g["feature"], g["neighbor_ids"], g["proj_rel"], g["depth_values"], mode=1)
    np.testing.assert_array_equal(var, ref)  # device-rounding oracle: bit for bit


@pytest.mark.parametrize("N,K,C,D,H,W", [
    (4, 2, 256, 3, 20, 28),   # C=256: one pixel per wave-instruction, ragged last tile (560 = 8*64+48)
    (3, 2, 32, 8, 48, 64),    # BASELINE config 1
    (5, 2, 20, 4, 9, 13),     # C not a multiple of 16, tiny odd map
    (3, 1, 7, 2, 6, 5),       # C < 8, k = 1
    (2, 0, 12, 3, 8, 8),      # no neighbour: variance of a single view is 0
    (6, 4, 64, 2, 12, 16),    # k = 4
    (2, 2, 300, 2, 10, 12),   # C > 256: more than 8 slabs
    (50, 2, 32, 96, 12, 16),  # BASELINE config 4 plane / view counts (ARKit-like: 50 views, 96 planes)
    (4, 2, 64, 128, 10, 12),  # BASELINE config 5 plane count
    (3, 2, 32, 5, 33, 47),    # odd map: ragged tiles in x and y, unaligned rows (scalar store path)
    (3, 2, 64, 6, 21, 80),    # width 32 m + 16 with few planes: 16x8 tiles
    (2, 3, 40, 4, 9, 48),     # the same with a partial slab and k = 3
    (2, 2, 32, 3, 12, 16),    # width 16: one column of 16x8 tiles
])
def test_plane_sweep_variance_shapes(gpu, oracle, N, K, C, D, H, W):
    from mvsdet_amd import functional as F_, ops, synthetic
    meta = synthetic.make_img_meta(N, (H, W), seed=5)
    feat = synthetic.make_features(N, C, (H, W), seed=5)
    rng = np.random.default_rng(7)
    nbr = np.stack([rng.permutation([j for j in range(N) if j != n] * 4)[:K] for n in range(N)]).astype(np.int64).reshape(N, K)
    w2c = torch.tensor(np.array(meta["lidar2img"]["extrinsic"]))
    Kf = torch.tensor(oracle.feat_intrinsics(meta["lidar2img"]["intrinsic"], meta["img_shape"], meta["ori_shape"]))
    ref_proj, nei = F_.collect_proj(w2c, Kf, torch.tensor(nbr)) if K else (None, ())
    proj_rel = torch.stack([torch.matmul(p, torch.inverse(ref_proj)) for p in nei], 1) if K else torch.zeros(N, 0, 4, 4)
    depth = torch.tensor(oracle.depth_planes(0.2, 5.0, D)).unsqueeze(0).repeat(N, 1)
    var = ops.plane_sweep_variance(feat.to(gpu), torch.tensor(nbr).to(gpu), proj_rel.to(gpu), depth.to(gpu)).cpu().numpy()
    ref = oracle.plane_sweep_variance(feat, nbr, proj_rel, depth, mode=1)
    np.testing.assert_array_equal(var, ref)
    if K == 0:
        assert np.abs(var).max() < 1e-6


@pytest.mark.parametrize("N,C,H,W", [(2, 64, 12, 16), (1, 33, 7, 20), (3, 5, 3, 4), (2, 32, 9, 13), (1, 256, 60, 80)])
def test_pack_features_layout(gpu, N, C, H, W):
    """packed[n][s][y][x][4g+i] = feat[n][32s + 8i + g][y][x] (include/mvsdet_hip.h), zero where the channel does not exist -- for dense
    maps (the float4 kernel where H*W is a multiple of 4), for a cropped view of a larger tensor and for a channel slice (the
    general kernel): all the same bits."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(C + W)
    big = torch.randn(N, C + 3, H + 2, W + 5, generator=g).to(gpu)
    feat = big[:, 1:C + 1, :H, :W].contiguous()
    S = (C + 31) // 32
    want = torch.zeros(N, S * 32, H, W, device=gpu)
    want[:, :C] = feat
    want = want.view(N, S, 4, 8, H, W).permute(0, 1, 4, 5, 3, 2).reshape(N, S, H, W, 32)   # [n][s][y][x][g][i] -> q = 4g + i
    got = ops.pack_features(feat)
    assert torch.equal(got.view(N, S, H, W, 32), want)
    assert torch.equal(ops.pack_features(big[:, 1:C + 1, :H, :W]), got)          # a strided view: the general kernel


def test_plane_sweep_both_tile_sizes_and_packed_entry(gpu, oracle, monkeypatch):
    """packed entry point == dense entry point; pack handles a non-contiguous crop view."""
    from mvsdet_amd import ops
    g = load_golden("g2_variance_n3_d8")
    feat = dev(g["feature"], gpu)
    N, C, H, W = feat.shape
    big = torch.zeros((N, C, H + 3, W + 5), device=gpu)
    big[:, :, :H, :W] = feat
    view = big[:, :, :H, :W]
    assert not view.is_contiguous()
    packed = ops.pack_features(view)
    assert torch.equal(packed, ops.pack_features(feat))
    var = ops.plane_sweep_variance_packed(packed, dev(g["neighbor_ids"], gpu), dev(g["proj_rel"], gpu),
                                          dev(g["depth_values"], gpu), C, H, W)
    ref = oracle.plane_sweep_variance(g["feature"], g["neighbor_ids"], g["proj_rel"], g["depth_values"], mode=1)
    np.testing.assert_array_equal(var.cpu().numpy(), ref)


def test_plane_sweep_properties_full_size(gpu):
    """Reference-true ScanNet shape (N=40,k=2,C=256,D=12,60x80): size-independent properties.
    (i) a view whose neighbours are itself under the identity homography... is NOT its input, so
        instead: (ii) var >= -eps everywhere, (iii) scaling features by s scales var by s^2 (bit-exact for s=2),
        (iv) permuting the two neighbours leaves var unchanged up to summation order, (v) per-view independence:
        the first 3 views computed alone (same neighbours present) equal the batched result."""
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 40, 256, 12, (60, 80)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D)
    meta = synthetic.make_img_meta(N, hw, seed=0)
    feat = synthetic.make_features(N, C, hw, seed=0, device=gpu)
    geo = hp.prepare_scene(meta, gpu)
    var = ops.plane_sweep_variance(feat, geo.neighbor_ids, geo.proj_rel, geo.depth_values)
    assert var.shape == (N, C, D, 60, 80)
    assert torch.isfinite(var).all()
    assert var.min().item() > -1e-4
    var2 = ops.plane_sweep_variance(feat * 2.0, geo.neighbor_ids, geo.proj_rel, geo.depth_values)
    assert torch.equal(var2, var * 4.0)
    swapped = ops.plane_sweep_variance(feat, geo.neighbor_ids.flip(1), geo.proj_rel.flip(1), geo.depth_values)
    assert (swapped - var).abs().max().item() < 1e-4
    # checksum of checksums against a second, independent evaluation path: homo_warp (NCHW gather kernel)
    n0 = 7
    acc_s = feat[n0:n0 + 1].unsqueeze(2).repeat(1, 1, D, 1, 1)
    acc_q = acc_s ** 2
    for j in range(2):
        nb = geo.neighbor_ids[n0, j]
        w = ops.homo_warp(feat[nb:nb + 1], geo.proj_rel[n0:n0 + 1, j], geo.depth_values[n0:n0 + 1])
        acc_s = acc_s + w
        acc_q = acc_q + w * w
    ref = acc_q / 3 - (acc_s / 3) ** 2
    assert (ref[0] - var[n0]).abs().max().item() < 1e-4


# --------------------------------------------------------------------------------------------- a5-a7
@pytest.mark.parametrize("tag", ["d8", "d12", "d12_arkit"])
def test_depth_prob_topk(gpu, oracle, tag):
    from mvsdet_amd import ops
    g = load_golden("g4_depth_prob")
    near, far = [float(v) for v in g[f"near_far_{tag}"]]
    D = g[f"cost_reg_{tag}"].shape[1]
    iv = (far - near) / D
    prob, off, est_depth, est_dens, est_idx, avg = [t.cpu().numpy() for t in ops.depth_prob_topk(
        dev(g[f"cost_reg_{tag}"], gpu), dev(g[f"off_logit_{tag}"], gpu), near, iv, 3)]
    np.testing.assert_allclose(prob, g[f"prob_{tag}"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(off, g[f"off_{tag}"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(est_dens, g[f"est_dens_{tag}"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(est_depth, g[f"est_depth_{tag}"], rtol=0, atol=TOL)
    np.testing.assert_allclose(avg, g[f"avg_depth_{tag}"], rtol=0, atol=TOL)
    r = oracle.depth_prob_topk(g[f"cost_reg_{tag}"], g[f"off_logit_{tag}"], near, iv, 3)
    np.testing.assert_array_equal(est_idx, r["est_idx"])  # plane indices bit-exact
    np.testing.assert_allclose(prob, r["prob"], rtol=0, atol=1e-6)
    # a6+a7 entry point on the reference's own prob/off: exact arithmetic, exact result
    ed, en, ei, av = [t.cpu().numpy() for t in ops.sample_depth_prob(dev(g[f"prob_{tag}"], gpu), dev(g[f"off_{tag}"], gpu),
                                                                     near, iv, 3)]
    np.testing.assert_array_equal(en, g[f"est_dens_{tag}"])
    np.testing.assert_array_equal(ed, g[f"est_depth_{tag}"])
    np.testing.assert_allclose(av, g[f"avg_depth_{tag}"], rtol=0, atol=5e-6)


def test_depth_prob_topk_ties_and_edges(gpu, oracle):
    from mvsdet_amd import ops
    # all-equal logits: exact ties -> lowest plane indices first; D == topk; H*W not a multiple of 256
    cost = torch.zeros((2, 3, 5, 7), device=gpu)
    offl = torch.zeros((2, 3, 5, 7), device=gpu)
    prob, off, ed, en, ei, av = ops.depth_prob_topk(cost, offl, 0.2, 0.4, 3)
    assert torch.equal(ei[:, 0], torch.zeros_like(ei[:, 0])) and torch.equal(ei[:, 2], torch.full_like(ei[:, 2], 2))
    assert torch.allclose(prob, torch.full_like(prob, 1 / 3))
    assert torch.allclose(off, torch.full_like(off, 0.5))
    with pytest.raises(ValueError):
        ops.depth_prob_topk(cost, offl, 0.2, 0.4, 4)  # topk > D
    # large D, extreme logits (no overflow in the softmax)
    g = torch.Generator().manual_seed(3)
    cost = (torch.randn((1, 128, 9, 11), generator=g) * 60).to(gpu)
    offl = (torch.randn((1, 128, 9, 11), generator=g) * 30).to(gpu)
    out = ops.depth_prob_topk(cost, offl, 0.5, 5 / 128, 3)
    r = oracle.depth_prob_topk(cost.cpu(), offl.cpu(), 0.5, 5 / 128, 3)
    assert all(torch.isfinite(t.float()).all() for t in out)
    np.testing.assert_allclose(out[0].cpu().numpy(), r["prob"], rtol=0, atol=1e-6)
    # with logits this extreme the 2nd/3rd probabilities underflow (exact ties at 0 / denormals): compare the
    # depth of a pick only where its probability is a normal number
    ok = r["est_dens"] > 1e-30
    np.testing.assert_allclose(out[2].cpu().numpy()[ok], r["est_depth"][ok], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(out[4].cpu().numpy()[:, 0], r["est_idx"][:, 0])


# --------------------------------------------------------------------------------------------- a9 / a10
@pytest.mark.parametrize("tag", ["scannet", "arkit"])
def test_backproject_weigh_golden(gpu, oracle, tag):
    from mvsdet_amd import _lib, functional as F_, ops
    g = load_golden("g5_backproject_" + tag)
    h, w = int(g["img_shape"][0] // 4), int(g["img_shape"][1] // 4)
    feat_full = dev(g["feature"], gpu)
    feat = feat_full[:, :, :h, :w]  # the reference's non-contiguous crop (mvsdet.py:499)
    N, C = feat.shape[:2]
    points, projection = dev(g["points"], gpu), dev(g["projection"], gpu)
    est_depth, est_dens = dev(g["est_depth"], gpu), dev(g["est_dens"], gpu)
    vz = float(g["voxel_size"][-1])
    # reference signature: depth / prob as (N, h*w, 1, J) transposed views (mvsdet.py:484,495)
    d_r = est_depth.reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)
    p_r = est_dens.reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)
    volume, valid, gap, rmse = F_.backproject_Weigh(feat, points, projection, d_r, list(g["voxel_size"]), p_r)
    assert volume.shape == g["volume"].shape and valid.shape == g["valid"].shape and valid.dtype == torch.bool
    assert float(gap) == 1.0 and float(rmse) == 1.0
    np.testing.assert_array_equal(valid.cpu().numpy(), g["valid"])
    np.testing.assert_array_equal(volume.cpu().numpy(), g["volume"])  # same rounding points: bit-exact
    # voxel indices, straight through the C ABI (xi / yi outputs)
    import ctypes
    V = points.numel() // 3
    xi = torch.empty((N, V), dtype=torch.int32, device=gpu)
    yi = torch.empty((N, V), dtype=torch.int32, device=gpu)
    vol2 = torch.empty((N, C, V), device=gpu)
    val2 = torch.empty((N, V), dtype=torch.uint8, device=gpu)
    lib = _lib.load()
    rc = lib.mvsdet_backproject_weigh_f32(_lib.ptr(feat), _lib.strides4(feat), _lib.ptr(points), _lib.ptr(projection),
                                          _lib.ptr(est_depth), _lib.ptr(est_dens), _lib.strides4(est_depth),
                                          _lib.ptr(vol2), _lib.ptr(val2), _lib.ptr(xi), _lib.ptr(yi), N, C, h, w, V, 3,
                                          ctypes.c_float(vz), _lib.current_stream(gpu))
    assert rc == 0
    torch.cuda.synchronize()
    vf = g["valid_frustum"]
    np.testing.assert_array_equal(xi.cpu().numpy()[vf], g["x"][vf])  # bit-exact, including the 3e-6 px near-ties
    np.testing.assert_array_equal(yi.cpu().numpy()[vf], g["y"][vf])
    o = oracle.backproject_weigh(g["feature"][:, :, :h, :w], g["points"], g["projection"], g["est_depth"], g["est_dens"],
                                 vz, want_index=True)
    np.testing.assert_array_equal(xi.cpu().numpy(), o["x"])
    np.testing.assert_array_equal(yi.cpu().numpy(), o["y"])
    # fused mean (a9+a10)
    packed = ops.pack_features(feat_full)
    H, W = feat_full.shape[2:]
    mean, count = ops.backproject_weigh_mean(feat, packed, points, projection, est_depth, est_dens, H, W, vz)
    np.testing.assert_array_equal(count.cpu().numpy(), g["valid_count"].reshape(-1))
    np.testing.assert_array_equal(mean.cpu().numpy(), g["volume_mean"].reshape(C, -1))


def test_backproject_mean_many_views_and_channels(gpu, oracle):
    """N > 64 (two view chunks of the mask), C = 256 and C > 256, voxel count not a multiple of the tile."""
    from mvsdet_amd import functional as F_, ops, synthetic
    for N, C, nv in ((70, 256, [9, 7, 5]), (5, 300, [8, 8, 4]), (3, 6, [5, 5, 3])):
        hw = (24, 32)
        meta = synthetic.make_img_meta(N, hw, seed=9)
        feat = synthetic.make_features(N, C, hw, seed=9)
        logits = synthetic.make_cost_logits(N, 12, hw, seed=9, sharp=2.0)
        r = oracle.depth_prob_topk(logits[:, 0], logits[:, 1], 0.2, 0.4, 3)
        h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
        proj = oracle.compute_projection(meta["lidar2img"]["extrinsic"], meta["lidar2img"]["intrinsic"], meta["img_shape"], meta["ori_shape"])
        pts = oracle.get_points(nv, [0.5, 0.5, 0.5], meta["lidar2img"]["origin"])
        ed, en = r["est_depth"][:, :, :h, :w], r["est_dens"][:, :, :h, :w]
        ref = oracle.backproject_weigh_mean(feat.numpy()[:, :, :h, :w], pts, proj, ed, en, 0.5)
        featg = feat.to(gpu)
        mean, count = ops.backproject_weigh_mean(featg[:, :, :h, :w], ops.pack_features(featg), dev(pts, gpu), dev(proj, gpu),
                                                 dev(r["est_depth"], gpu)[:, :, :h, :w], dev(r["est_dens"], gpu)[:, :, :h, :w],
                                                 hw[0], hw[1], 0.5)
        assert ref["valid_count"].max() > 0
        np.testing.assert_array_equal(count.cpu().numpy(), ref["valid_count"])
        np.testing.assert_array_equal(mean.cpu().numpy(), ref["volume_mean"])


# --------------------------------------------------------------------------------------------- end to end
def test_end_to_end_scene_vs_reference_chain(gpu, oracle):
    """a1..a10 through MVSDetHotPath.forward_scene against the chained reference outputs (G7)."""
    from mvsdet_amd.hotpath import MVSDetHotPath
    g = load_golden("g7_end_to_end")
    meta = {"lidar2img": {"extrinsic": list(g["extrinsic"]), "intrinsic": g["intrinsic"], "origin": g["origin"]},
            "img_shape": tuple(int(v) for v in g["img_shape"]), "ori_shape": tuple(int(v) for v in g["ori_shape"])}
    D = g["depth_values"].shape[1]
    Wc = dev(g["Wc"], gpu)

    def stand_in_net(var):  # the fixed linear stand-in for CostRegNet_3DGS used by make_goldens.g7
        lg = torch.einsum("oc,ncdhw->nodhw", Wc, var)
        lg[:, 0] += torch.linspace(0, 0.6, D, device=var.device).view(1, D, 1, 1)
        return lg

    hp = MVSDetHotPath(list(g["n_voxels"]), list(g["voxel_size"]), list(g["near_far"]), D, topk=3,
                       cost_regularization=stand_in_net)
    out = hp.forward_scene(dev(g["feature"], gpu), meta)
    geo = out["geometry"]
    np.testing.assert_array_equal(geo.neighbor_ids.cpu().numpy(), g["neighbor_ids"])
    np.testing.assert_allclose(geo.proj_rel.cpu().numpy(), g["proj_rel"], rtol=1e-5, atol=1e-4)
    # host BLAS (3x3 @ 3x4) may round differently on this machine than on the golden-generating one
    np.testing.assert_allclose(geo.projection.cpu().numpy(), g["projection"], rtol=2e-6, atol=1e-5)
    np.testing.assert_allclose(out["variance"].cpu().numpy()[:, :, :, ::6, ::8], g["variance_sample"], rtol=0, atol=TOL)
    np.testing.assert_allclose(out["prob_volume"].cpu().numpy(), g["prob"], rtol=0, atol=TOL)
    np.testing.assert_allclose(out["est_densities"].cpu().numpy(), g["est_dens"], rtol=0, atol=TOL)
    np.testing.assert_allclose(out["depth_coding"].cpu().numpy(), g["depth_coding"], rtol=0, atol=TOL)
    # NVS branch: mvsdet.py:582 `opacity = torch.max(prob_volume, dim=1)[0]` -- the kernel's first top-k value, the same bits
    assert torch.equal(out["opacity"], out["prob_volume"].max(dim=1)[0])
    # est_depth / voxel volume depend on discrete choices (plane ranking, depth-window tests) that flip when a
    # probability gap or a window margin is below the fp32 noise of the chain: compare where they are decided
    srt = np.sort(g["prob"], axis=1)[:, ::-1]
    h, w = geo.height, geo.width
    clear = ((srt[:, :3] - srt[:, 1:4]).min(axis=1) > 1e-5)[:, :h, :w]
    m3 = np.broadcast_to(clear[:, None], g["est_depth"].shape)
    np.testing.assert_allclose(out["est_depth"].cpu().numpy()[m3], g["est_depth"][m3], rtol=0, atol=TOL)
    cnt = out["valid"].cpu().numpy()
    agree = (cnt == g["valid_count"])
    assert agree.mean() > 0.999, agree.mean()
    vol = out["volume"].cpu().numpy()
    sel = np.broadcast_to(agree, vol.shape)
    close = np.abs(vol - g["volume_mean"]) <= 2e-4
    assert close[sel].mean() > 0.999, close[sel].mean()


# --------------------------------------------------------------------------------------------- backward
def test_backward_stage1(gpu, oracle):
    from mvsdet_amd import ops
    g = load_golden("g6_backward")
    feat = dev(g["s1_feature"], gpu).requires_grad_(True)
    var = ops.plane_sweep_variance(feat, dev(g["s1_neighbor_ids"], gpu), dev(g["s1_proj_rel"], gpu), dev(g["s1_depth_values"], gpu))
    np.testing.assert_allclose(var.detach().cpu().numpy(), g["s1_variance"], rtol=0, atol=TOL)
    (var * dev(g["s1_R"], gpu)).sum().backward()
    # gradients of scale 10 (max |.|; rms 1.6): the bar 1e-4 of scale would be 1e-3; measured 1.2e-6 (tools/study/r06_grad_tolerances.py: the
    # summation order of the atomics), held to 2e-5 absolute = 2e-6 of scale
    np.testing.assert_allclose(feat.grad.cpu().numpy(), g["s1_grad_feature"], rtol=1e-4, atol=2e-5)


def test_backward_stage1_shapes(gpu, oracle):
    from mvsdet_amd import ops
    for tag in ("n3_d8", "n6_d12_arkit"):
        g = load_golden("g2_variance_" + tag)
        feat = dev(g["feature"], gpu).requires_grad_(True)
        args = (dev(g["neighbor_ids"], gpu), dev(g["proj_rel"], gpu), dev(g["depth_values"], gpu))
        var = ops.plane_sweep_variance(feat, *args)
        R = torch.randn(var.shape, generator=torch.Generator().manual_seed(1)).to(gpu)
        (var * R).sum().backward()
        ref = oracle.plane_sweep_variance_bwd(g["feature"], g["neighbor_ids"], g["proj_rel"], g["depth_values"], R.cpu())
        # scale 15-18, measured 1.9e-6: held to 2e-5 absolute (about 1e-6 of scale; the 1e-4 bar would be 1.5e-3)
        np.testing.assert_allclose(feat.grad.cpu().numpy(), ref, rtol=1e-4, atol=2e-5)


def test_backward_stage2(gpu):
    from mvsdet_amd import ops
    g = load_golden("g6_backward")
    logits = dev(g["s2_logits"], gpu).requires_grad_(True)
    D = logits.shape[2]
    prob, off, ed, en, ei, av = ops.depth_prob_topk(logits[:, 0], logits[:, 1], 0.2, (5.0 - 0.2) / D, 3)
    loss = (ed * dev(g["s2_R_depth"], gpu)).sum() + (en * dev(g["s2_R_dens"], gpu)).sum() + \
           (av * dev(g["s2_R_avg"], gpu)).sum() + (prob * dev(g["s2_R_prob"], gpu)).sum()
    loss.backward()
    np.testing.assert_allclose(logits.grad.cpu().numpy(), g["s2_grad_logits"], rtol=1e-4, atol=5e-6)


def test_backward_stage3(gpu):
    from mvsdet_amd import functional as F_, ops
    g = load_golden("g6_backward")
    meta = {"lidar2img": {"extrinsic": list(g["s3_extrinsic"]), "intrinsic": g["s3_intrinsic"], "origin": g["s3_origin"]},
            "img_shape": tuple(int(v) for v in g["s3_img_shape"]), "ori_shape": tuple(int(v) for v in g["s3_ori_shape"])}
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    projection = F_.compute_projection(meta, 4).to(gpu)
    points = F_.get_points(torch.tensor(g["s3_n_voxels"]), torch.tensor(g["s3_voxel_size"], dtype=torch.float32),
                           torch.tensor(g["s3_origin"])).to(gpu)
    vz = float(g["s3_voxel_size"][-1])
    feat = dev(g["s3_feature"], gpu).requires_grad_(True)
    dens = dev(g["s3_est_dens"], gpu).requires_grad_(True)
    depth = dev(g["s3_est_depth"], gpu)
    N = feat.shape[0]
    d_r = depth.reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)
    p_r = dens.reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)
    volume, valid, _, _ = F_.backproject_Weigh(feat[:, :, :h, :w], points, projection, d_r, list(g["s3_voxel_size"]), p_r)
    np.testing.assert_array_equal(valid.cpu().numpy(), g["s3_valid"])
    np.testing.assert_array_equal(volume.detach().cpu().numpy(), g["s3_volume"])
    (volume * dev(g["s3_R"], gpu)).sum().backward()
    np.testing.assert_allclose(feat.grad.cpu().numpy(), g["s3_grad_feature"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dens.grad.cpu().numpy(), g["s3_grad_dens"], rtol=1e-4, atol=1e-5)
    # fused mean
    feat.grad = None
    dens.grad = None
    H, W = feat.shape[2:]
    mean, count = ops.backproject_weigh_mean(feat[:, :, :h, :w], ops.pack_features(feat.detach()), points, projection,
                                             depth, dens, H, W, vz)
    (mean.view(g["s3_Rmean"].shape) * dev(g["s3_Rmean"], gpu)).sum().backward()
    np.testing.assert_allclose(feat.grad.cpu().numpy(), g["s3_grad_feature_mean"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dens.grad.cpu().numpy(), g["s3_grad_dens_mean"], rtol=1e-4, atol=1e-5)


# --------------------------------------------------------------------------------------------- errors
def test_error_behaviour(gpu):
    from mvsdet_amd import _lib, ops
    feat = torch.zeros((2, 4, 8, 8), device=gpu)
    nbr = torch.zeros((2, 5), dtype=torch.int64, device=gpu)  # K = 5 > MVSDET_MAX_NEIGHBORS
    with pytest.raises(ValueError, match="K=5"):
        ops.plane_sweep_variance(feat, nbr, torch.zeros((2, 5, 4, 4), device=gpu), torch.ones((2, 3), device=gpu))
    with pytest.raises(ValueError):
        ops.plane_sweep_variance(feat, nbr[:, :2], torch.zeros((2, 3, 4, 4), device=gpu), torch.ones((2, 3), device=gpu))
    with pytest.raises(TypeError):
        ops.homo_warp(feat.double(), torch.zeros((2, 4, 4), device=gpu), torch.ones((2, 3), device=gpu))
    with pytest.raises((RuntimeError, NotImplementedError)):
        ops.homo_warp(feat.cpu(), torch.zeros((2, 4, 4)), torch.ones((2, 3)))  # no CPU path
    # out-of-range neighbour ids are clamped, never dereferenced out of bounds
    bad = torch.tensor([[99, -7], [1, 0]], dtype=torch.int64, device=gpu)
    out = ops.plane_sweep_variance(feat, bad, torch.eye(4, device=gpu).repeat(2, 2, 1, 1), torch.ones((2, 3), device=gpu))
    assert torch.isfinite(out).all()
    rc = _lib.load().mvsdet_homo_warp_f32(None, None, None, None, 1, 1, 1, 2, 2, None)
    assert rc == 1 and b"NULL" in _lib.load().mvsdet_last_error()


def test_plane_sweep_is_deterministic(gpu):
    """The sweep synchronises LDS-DMA, LDS tables and barriers by hand: repeated launches on the reference-true
    shape must be bit-identical (a missing wait shows up as rare stale reads in a few pixels of one block)."""
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 40, 256, 12, (60, 80)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D)
    feat = synthetic.make_features(N, C, hw, seed=3, device=gpu)
    geo = hp.prepare_scene(synthetic.make_img_meta(N, hw, seed=3), gpu)
    packed = ops.pack_features(feat)
    ref = ops.plane_sweep_variance_packed(packed, geo.neighbor_ids, geo.proj_rel, geo.depth_values, C, *hw)
    for _ in range(25):
        again = ops.plane_sweep_variance_packed(packed, geo.neighbor_ids, geo.proj_rel, geo.depth_values, C, *hw)
        assert torch.equal(again, ref)
        del again


def test_sweep_split_entry_points(gpu, oracle):
    """table + tabled sweep (the two halves of the packed entry point) == the one-call form."""
    from mvsdet_amd import ops
    g = load_golden("g2_variance_n3_d8")
    feat = dev(g["feature"], gpu)
    N, C, H, W = feat.shape
    nbr, proj, depth = dev(g["neighbor_ids"], gpu), dev(g["proj_rel"], gpu), dev(g["depth_values"], gpu)
    packed = ops.pack_features(feat)
    table = ops.plane_sweep_table(proj, depth, H, W)
    a = ops.plane_sweep_variance_tabled(packed, nbr, table, C, depth.shape[1], H, W)
    b = ops.plane_sweep_variance_packed(packed, nbr, proj, depth, C, H, W)
    assert torch.equal(a, b)
    ref = oracle.plane_sweep_variance(g["feature"], g["neighbor_ids"], g["proj_rel"], g["depth_values"], mode=1)
    np.testing.assert_array_equal(a.cpu().numpy(), ref)


def test_training_step_through_forward_scene(gpu):
    """Training configuration in miniature: a trainable stand-in for CostRegNet_3DGS between the stages; one
    optimiser step through a1..a10 (what DDP wraps on 8 GPUs).  Gradients reach the 2-D features and the module."""
    from mvsdet_amd import synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    torch.manual_seed(0)
    N, C, D, hw = 4, 32, 12, (60, 80)
    net = torch.nn.Conv3d(C, 2, 3, padding=1).to(gpu)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D, topk=3, cost_regularization=net)
    meta = synthetic.make_img_meta(N, hw, seed=11)
    feat = synthetic.make_features(N, C, hw, seed=11).to(gpu).requires_grad_(True)
    opt = torch.optim.SGD(list(net.parameters()), lr=1e-3)
    out = hp.forward_scene(feat, meta)
    loss = out["volume"].pow(2).mean() + out["depth_coding"].mean() + 0.1 * out["prob_volume"].max(dim=1)[0].mean()
    loss.backward()
    assert torch.isfinite(feat.grad).all() and feat.grad.abs().sum().item() > 0
    for p in net.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum().item() > 0
    before = [p.detach().clone() for p in net.parameters()]
    opt.step()
    assert any(not torch.equal(a, b) for a, b in zip(before, net.parameters()))
    # the op-level gradient agrees with a central finite difference of the loss in a random feature direction
    with torch.no_grad():
        v = torch.randn_like(feat)
        v /= v.norm()
    def L(f_):
        with torch.no_grad():
            o = hp.forward_scene(f_, meta)
            return (o["variance"].double() ** 2).mean()
    feat.grad = None
    o = hp.forward_scene(feat, meta)
    (o["variance"].double() ** 2).mean().backward()
    eps = 1e-2
    fd = (L(feat.detach() + eps * v) - L(feat.detach() - eps * v)) / (2 * eps)
    an = (feat.grad.double() * v.double()).sum()
    assert abs(fd.item() - an.item()) <= 2e-2 * max(abs(an.item()), 1e-6) + 1e-7, (fd.item(), an.item())


def test_sweep_variants_are_bit_identical(gpu):
    """The tuning options only change the schedule: tile shape 16x8 vs 32x4, resident LDS boxes of several capacities
    (runs of planes per box) vs the global-gather fallback give the same bits."""
    from mvsdet_amd import _lib, ops
    g = load_golden("g2_variance_n3_d8")
    feat = dev(g["feature"], gpu)
    N, C, H, W = feat.shape
    args = (ops.pack_features(feat), dev(g["neighbor_ids"], gpu), dev(g["proj_rel"], gpu), dev(g["depth_values"], gpu), C, H, W)
    ref = ops.plane_sweep_variance_packed(*args)
    saved = {k: _lib.get_option(k) for k in ("sweep_tw", "sweep_boxcap", "sweep_xcd", "sweep_dsplit", "sweep_groups")}
    try:
        for opts in ({"sweep_tw": 16}, {"sweep_tw": 32}, {"sweep_boxcap": 0}, {"sweep_boxcap": 40}, {"sweep_boxcap": 320},
                     {"sweep_tw": 16, "sweep_boxcap": 0}, {"sweep_tw": 32, "sweep_boxcap": 96, "sweep_xcd": 0},
                     {"sweep_tw": 16, "sweep_boxcap": 64}, {"sweep_dsplit": 1}, {"sweep_dsplit": 3}, {"sweep_dsplit": 8},
                     {"sweep_groups": 2}, {"sweep_groups": 6, "sweep_dsplit": 1}, {"sweep_groups": 4, "sweep_tw": 32, "sweep_dsplit": 1}):
            for k, v in {**saved, **opts}.items():
                _lib.set_option(k, v)
            out = ops.plane_sweep_variance_packed(*args)
            assert torch.equal(out, ref), opts
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
    # a geometry built under one "sweep_boxcap" and consumed under another (include/mvsdet_hip.h: the consuming call
    # sizes its LDS slots for the largest capacity the tile shape allows; the geometry carries its own runs)
    packed, nbr, proj, depth = args[:4]
    D = depth.shape[1]
    try:
        for build, consume in ((saved["sweep_boxcap"], 0), (saved["sweep_boxcap"], 40), (40, saved["sweep_boxcap"]), (0, 200)):
            _lib.set_option("sweep_boxcap", build)
            table = ops.plane_sweep_table(proj, depth, H, W)
            _lib.set_option("sweep_boxcap", consume)
            assert torch.equal(ops.plane_sweep_variance_tabled(packed, nbr, table, C, D, H, W), ref), (build, consume)
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)
    # the row-pitched volume (rows on 128-byte lines, 32x4 tiles): the same values behind other strides
    wp = ops.sweep_row_pitch(W)
    tp = ops.plane_sweep_table_pitched(proj, depth, H, W, wp)
    pv = ops.plane_sweep_variance_tabled_pitched(packed, nbr, tp, C, D, H, W, wp)
    assert pv.shape == ref.shape and pv.stride(3) == wp and torch.equal(pv, ref)
    with pytest.raises(ValueError):
        ops.plane_sweep_variance_tabled_pitched(packed, nbr, tp, C, D, H, W, W - 1)
    with pytest.raises(ValueError):
        _lib.set_option("no_such_option", 1)


def test_sweep_degenerate_geometry(gpu, oracle):
    """Planes through the source camera centre (z == 0 -> Inf/NaN sample positions), views entirely behind the
    source camera and wildly out-of-image footprints: no fault, and the same values as the oracle (NaN where the
    reference's ATen-CPU path produces NaN)."""
    from mvsdet_amd import ops
    N, K, C, D, H, W = 3, 2, 8, 4, 12, 16
    gen = torch.Generator().manual_seed(5)
    feat = torch.randn(N, C, H, W, generator=gen)
    nbr = torch.tensor([[1, 2], [2, 0], [0, 1]])
    proj = torch.eye(4).repeat(N, K, 1, 1)
    proj[0, 0, 2, :] = torch.tensor([0.0, 0.0, 0.0, 0.0])        # z = 0 for every pixel and plane -> NaN / Inf
    proj[0, 1, 2, :] = torch.tensor([0.0, 0.0, -1.0, -0.5])      # z < 0: mirrored positions, finite
    proj[1, 0, 0, 3] = 1e6                                        # far outside the image: all taps invalid
    proj[1, 1, :3, :3] *= 40.0                                    # 40x scale: footprint larger than any LDS box
    proj[2, 0, 0, 3], proj[2, 0, 1, 3] = 3.3, -2.1                # ordinary shift
    depth = torch.tensor([0.5, 1.0, 2.0, 4.0]).repeat(N, 1)
    out = ops.plane_sweep_variance(feat.to(gpu), nbr.to(gpu), proj.to(gpu), depth.to(gpu)).cpu().numpy()
    ref = oracle.plane_sweep_variance(feat, nbr, proj, depth, mode=1)
    assert np.isnan(ref[0]).any() and np.isfinite(ref[1:]).all()
    np.testing.assert_array_equal(np.isnan(out), np.isnan(ref))
    np.testing.assert_array_equal(out[~np.isnan(ref)], ref[~np.isnan(ref)])


def test_full_size_64_plane_shape(gpu, oracle):
    """BASELINE configs[1] at full size (40 views, 64 planes, 120x160, C=256: a 50 GB cost volume): exact x4
    scaling, finiteness, and a slice (one reference view, 8 channels) recomputed by the oracle on the 3-view
    sub-scene {view, neighbour 0, neighbour 1}."""
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < 130 * (1 << 30):
        pytest.skip("needs ~110 GB of free HBM")
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 40, 256, 64, (120, 160)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D)
    feat = synthetic.make_features(N, C, hw, seed=1, device=gpu)
    geo = hp.prepare_scene(synthetic.make_img_meta(N, hw, seed=1), gpu)
    var = ops.plane_sweep_variance(feat, geo.neighbor_ids, geo.proj_rel, geo.depth_values)
    assert var.shape == (N, C, D, 120, 160)
    n0, ch = 17, [0, 31, 32, 100, 129, 200, 254, 255]
    nb = geo.neighbor_ids[n0].tolist()
    sub_feat = feat[[n0] + nb][:, ch].cpu()
    sub = oracle.plane_sweep_variance(sub_feat, np.array([[1, 2], [0, 2], [0, 1]]), np.stack(
        [geo.proj_rel[n0].cpu().numpy()] * 3), geo.depth_values[:3].cpu(), mode=1)
    np.testing.assert_array_equal(var[n0, ch].cpu().numpy(), sub[0])
    mn = float(var.min())
    assert mn > -1e-4 and bool(torch.isfinite(var[::7, ::31]).all())
    var2 = ops.plane_sweep_variance(feat * 2.0, geo.neighbor_ids, geo.proj_rel, geo.depth_values)
    step = 5  # compare in slabs to keep temporaries small
    for i in range(0, N, step):
        assert torch.equal(var2[i:i + step], var[i:i + step] * 4.0)


# --------------------------------------------------------------------------------------------- view shards (8e)
def test_view_shards_reassemble_the_scene(gpu, oracle):
    """Intra-scene split: the per-shard sweep rows are bit-identical to the unsharded rows, the shards' stage-3
    sums and counts add up to the fused mean, and parallel.forward_scene_view_sharded (one rank) agrees with
    MVSDetHotPath.forward_scene."""
    from mvsdet_amd import ops, parallel, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 7, 40, 12, (24, 32)
    hp = MVSDetHotPath([16, 16, 8], [.4, .4, .4], [0.2, 5.0], D)
    meta = synthetic.make_img_meta(N, hw, seed=4)
    feat = synthetic.make_features(N, C, hw, seed=4).to(gpu)
    logits = synthetic.make_cost_logits(N, D, hw, seed=4, sharp=2.0).to(gpu)
    full = hp.forward_scene(feat, meta, cost_logits=logits)
    geo = full["geometry"]
    packed = ops.pack_features(feat)
    stages = parallel.HipStages(hp)
    total = torch.zeros((C, 16 * 16 * 8), device=gpu)
    count = torch.zeros((16 * 16 * 8,), dtype=torch.int32, device=gpu)
    for world in (2, 3):
        total.zero_(); count.zero_()
        for rank in range(world):
            first, m = parallel.view_shard(N, rank, world)
            var = stages.cost_volume_shard(packed, geo, first, m, N, C, *hw)
            assert torch.equal(var, full["variance"][first:first + m])
            prob, off, ed, en, _, avg = stages.depth_distribution(logits[first:first + m])
            assert torch.equal(ed[:, :, :geo.height, :geo.width], full["est_depth"][first:first + m])
            s, c = stages.lift_sum_shard(packed, geo, ed, en, first, m, N, C, *hw)
            total += s
            count += c
        assert torch.equal(count.view_as(full["valid"][0]).long(), full["valid"][0])
        mean = torch.where(count > 0, total / (count + 1e-8), torch.zeros((), device=gpu)).view_as(full["volume"])
        np.testing.assert_allclose(mean.cpu().numpy(), full["volume"].cpu().numpy(), rtol=0, atol=2e-6)
    # the un-normalised sum of ALL views against the oracle's per-view volumes
    h, w = geo.height, geo.width
    o = oracle.backproject_weigh(feat.cpu().numpy()[:, :, :h, :w], geo.points.reshape(3, -1).cpu().numpy(),
                                 geo.projection.cpu().numpy(), full["est_depth"].cpu().numpy(),
                                 full["est_densities"].cpu().numpy(), hp.voxel_size[-1])
    prob, off, ed, en, _, avg = stages.depth_distribution(logits)
    s, c = stages.lift_sum_shard(packed, geo, ed, en, 0, N, N, C, *hw)
    np.testing.assert_array_equal(c.cpu().numpy(), o["valid"].sum(0))
    acc = np.zeros_like(o["volume"][0])
    for i in range(N):                       # ascending view order, the kernel's order
        acc = acc + o["volume"][i]
    np.testing.assert_array_equal(s.cpu().numpy(), acc)
    one = parallel.forward_scene_view_sharded(hp, feat, meta, cost_logits=logits)
    assert one["view_range"] == (0, N) and torch.equal(one["valid"], full["valid"])
    assert torch.equal(one["variance"], full["variance"]) and torch.equal(one["depth_coding"], full["depth_coding"])
    np.testing.assert_allclose(one["volume"].cpu().numpy(), full["volume"].cpu().numpy(), rtol=0, atol=2e-6)
    with pytest.raises(ValueError):
        ops.plane_sweep_variance_shard(packed, geo.neighbor_ids[:3], geo.proj_rel[:3], geo.depth_values[:3], N, 5, C, *hw)


# --------------------------------------------------------------------------------------------- fp16 storage (configs[4])
@pytest.mark.parametrize("N,C,D,H,W,chunk", [(5, 40, 6, 24, 32, 2), (3, 32, 4, 33, 47, 3), (4, 256, 3, 20, 28, 1),
                                               (3, 32, 128, 10, 12, 2), (4, 64, 128, 12, 64, 3)])
def test_fp16_storage_and_view_chunks(gpu, oracle, N, C, D, H, W, chunk):
    """fp16 feature maps in, fp16 cost volume out, produced in chunks of reference views: the arithmetic is the
    fp32 path's, so the result must equal the oracle's fp32 variance of the (exactly converted) half features,
    rounded to nearest-even -- bit for bit; fp32 chunks must equal the unchunked rows."""
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    hp = MVSDetHotPath([8, 8, 4], [.8, .8, .8], [0.2, 5.0], D)
    meta = synthetic.make_img_meta(N, (H, W), seed=11)
    feat16 = synthetic.make_features(N, C, (H, W), seed=11).half()
    feat16[0, 0, 0, 0] = 300.0          # variance of this texel overflows fp16 somewhere -> +inf on both sides
    geo = hp.prepare_scene(meta, gpu)
    packed = ops.pack_features(feat16.to(gpu))
    assert packed.dtype == torch.float32
    assert torch.equal(packed, ops.pack_features(feat16.float().to(gpu)))          # exact conversion
    ref32 = oracle.plane_sweep_variance(feat16.float().numpy(), geo.neighbor_ids.cpu().numpy(), geo.proj_rel.cpu().numpy(),
                                        geo.depth_values.cpu().numpy(), mode=1)
    with np.errstate(over="ignore"):
        ref16 = ref32.astype(np.float16)                                            # numpy rounds to nearest-even
    got16 = torch.empty((N, C, D, H, W), dtype=torch.float16)
    got32 = torch.empty((N, C, D, H, W), dtype=torch.float32)
    firsts = []
    for first, var in hp.cost_volume_chunks(packed, geo, C, H, W, chunk, half_out=True):
        assert var.dtype == torch.float16
        got16[first:first + var.shape[0]] = var.cpu()
        firsts.append(first)
    for first, var in hp.cost_volume_chunks(packed, geo, C, H, W, chunk):
        got32[first:first + var.shape[0]] = var.cpu()
    assert firsts == list(range(0, N, chunk))
    np.testing.assert_array_equal(got32.numpy(), ref32)
    np.testing.assert_array_equal(got16.numpy().view(np.uint16), ref16.view(np.uint16))
    # the lifting from packed maps alone (no fp32 NCHW tensor) equals the fused mean of the fp32 form
    logits = synthetic.make_cost_logits(N, D, (H, W), seed=11, sharp=2.0).to(gpu)
    prob, off, ed, en, _, avg = hp.depth_distribution(logits)
    vol, valid = hp.lift_packed(packed, geo, ed, en, C, H, W)
    vol2, valid2 = hp.lift(feat16.float().to(gpu), packed, geo, ed, en)
    assert torch.equal(valid, valid2)
    np.testing.assert_allclose(vol.cpu().numpy(), vol2.cpu().numpy(), rtol=0, atol=2e-6)


def test_stress_config_full_size(gpu, oracle):
    """BASELINE configs[4] as worded and at its size: 100 views x 128 planes x 240x320 (HxW) maps, C=256, fp16 feature maps
    in and fp16 cost volume out (503 GB) produced in chunks of 10 reference views (50 GB each) through
    `cost_volume_chunks(..., half_out=True)` -- the route bench.py times.  Views spread over three chunks are recomputed
    by the oracle (mode 1) on their 3-view sub-scene {view, neighbour 0, neighbour 1}, 8 channels each, and rounded to
    fp16 to nearest-even: bit for bit.  One chunk is produced again from doubled features: exactly 4x wherever the
    fp16 value is normal (fp32 arithmetic scales exactly; fp16 rounding commutes with a power of two outside the
    subnormal range), finite and non-negative up to rounding everywhere."""
    torch.cuda.empty_cache()   # blocks cached by earlier tests count as used in mem_get_info
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < 200 * (1 << 30):
        pytest.skip("needs ~175 GB of free HBM (three 50 GB chunks + the packed maps)")
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw, chunk = 100, 256, 128, (240, 320), 10
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D)
    feat16 = synthetic.make_features(N, C, hw, seed=5, device=gpu).half()
    geo = hp.prepare_scene(synthetic.make_img_meta(N, hw, seed=5), gpu)
    packed = ops.pack_features(feat16)
    assert packed.dtype == torch.float32
    probes = {3: [0, 31, 32, 100, 129, 200, 254, 255], 47: [1, 30, 33, 64, 127, 128, 191, 255], 99: [7, 8, 15, 16, 95, 96, 223, 224]}
    seen, kept = [], None
    for first, var in hp.cost_volume_chunks(packed, geo, C, hw[0], hw[1], chunk, half_out=True):
        assert var.dtype == torch.float16 and var.shape == (min(chunk, N - first), C, D, hw[0], hw[1])
        for n0, ch in probes.items():
            if first <= n0 < first + var.shape[0]:
                nb = geo.neighbor_ids[n0].tolist()
                sub_feat = feat16[[n0] + nb][:, ch].float().cpu()
                sub = oracle.plane_sweep_variance(sub_feat, np.array([[1, 2], [0, 2], [0, 1]]), np.stack(
                    [geo.proj_rel[n0].cpu().numpy()] * 3), geo.depth_values[:3].cpu(), mode=1)
                with np.errstate(over="ignore"):
                    ref16 = sub[0].astype(np.float16)
                got = var[n0 - first, ch].cpu().numpy()
                np.testing.assert_array_equal(got.view(np.uint16), ref16.view(np.uint16))
                seen.append(first)
        if first == 40:
            kept = var            # the chunk of views 40..49 stays for the scaling property
        else:
            assert bool(torch.isfinite(var[::3, ::37, ::5]).all())
        del var
    assert sorted(set(seen)) == [0, 40, 90] and kept is not None
    packed2 = ops.pack_features(feat16 * 2.0)      # exact in fp16 (|f| < 6 sigma)
    sl = slice(40, 50)
    var2 = ops.plane_sweep_variance_shard(packed2, geo.neighbor_ids[sl], geo.proj_rel[sl], geo.depth_values[sl], N, 40, C,
                                          hw[0], hw[1], True)
    tiny = 2.0 ** -14                              # smallest normal fp16
    for i in range(chunk):                         # view by view, 64 channels at a time: temporaries of ~2.5 GB
        for c0 in range(0, C, 64):
            a, b = kept[i, c0:c0 + 64].float(), var2[i, c0:c0 + 64].float()
            assert bool(torch.isfinite(b).all()) and float(a.min()) > -1e-3
            err = (b - a * 4.0).abs()
            assert float(torch.where(a > tiny, err, torch.zeros_like(err)).max()) == 0.0   # exact where the UNROUNDED value is a normal fp16 (a == 2^-14 may be a rounded-up subnormal)
            assert float(err.max()) <= 4 * 2.0 ** -24


# --------------------------------------------------------------------------------------------- HIP graph capture
def test_hot_path_is_graph_capturable(gpu):
    """include/mvsdet_hip.h promises that every entry point only enqueues work on the given stream (no allocation,
    no host synchronisation): pack -> sweep -> depth distribution -> lifting captured into ONE HIP graph and
    replayed on new inputs gives the eager result bit for bit."""
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 5, 64, 12, (60, 80)
    hp = MVSDetHotPath([40, 40, 16], [.16, .16, .2], [0.2, 5.0], D)
    meta = synthetic.make_img_meta(N, hw, seed=2)
    geo = hp.prepare_scene(meta, gpu)
    feat = synthetic.make_features(N, C, hw, seed=2).to(gpu)
    logits = synthetic.make_cost_logits(N, D, hw, seed=2, sharp=2.0).to(gpu)

    def run(f, lg):   # forward_scene forks the sampling-table kernel onto a side stream: captured as a graph branch
        o = hp.forward_scene(f, meta, cost_logits=lg, geo=geo)
        return o["variance"], o["prob_volume"], o["volume"], o["valid"]

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):          # warm-up on a side stream, as graph capture requires
        run(feat, logits)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    sf, sl = feat.clone(), logits.clone()  # static inputs of the graph
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(sf, sl)
    for seed in (7, 8):
        f2 = synthetic.make_features(N, C, hw, seed=seed).to(gpu)
        l2 = synthetic.make_cost_logits(N, D, hw, seed=seed, sharp=2.0).to(gpu)
        sf.copy_(f2)
        sl.copy_(l2)
        graph.replay()
        torch.cuda.synchronize(gpu)
        eager = run(f2, l2)
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)
    assert int((outs[3] > 0).sum()) > 100


# --------------------------------------------------------------------------------------------- randomised sweep cases
@pytest.mark.parametrize("seed", range(12))
def test_sweep_randomised_against_oracle(gpu, oracle, seed):
    """Random shapes and random projective maps (shifts that push whole tiles out of view, shears, scales across the
    LDS-box limit, planes at and behind the source camera), each run three times: bit-identical to the oracle every
    time.  Covers the skipped-neighbour / staged / gathered paths in every mixture inside one launch."""
    from mvsdet_amd import ops
    rng = np.random.default_rng(1000 + seed)
    N = int(rng.integers(2, 7))
    K = int(rng.integers(1, min(4, N - 1) + 1))
    C = int(rng.choice([5, 32, 40, 64, 96]))
    D = int(rng.integers(1, 9))
    H, W = int(rng.integers(5, 41)), int(rng.integers(6, 81))
    feat = torch.from_numpy(rng.standard_normal((N, C, H, W)).astype(np.float32))
    nbr = np.stack([rng.permutation([j for j in range(N) if j != n] * 4)[:K] for n in range(N)]).astype(np.int64)
    proj = np.tile(np.eye(4, dtype=np.float32), (N, K, 1, 1))
    for n in range(N):
        for j in range(K):
            kind = rng.integers(0, 6)
            A = np.eye(3, dtype=np.float32)
            t = np.zeros(3, dtype=np.float32)
            if kind == 0:      # ordinary small motion
                A[:2, :2] += rng.normal(0, 0.05, (2, 2)); t[:2] = rng.normal(0, 3.0, 2)
            elif kind == 1:    # large shift: most or all of the footprint leaves the image
                t[:2] = rng.choice([-1, 1], 2) * rng.uniform(0.5, 2.5, 2) * np.array([W, H])
            elif kind == 2:    # strong scale: footprints across the LDS-box limit
                A[:2, :2] *= rng.uniform(1.5, 6.0)
            elif kind == 3:    # perspective: z varies over the image, partly negative
                A[2, :2] = rng.normal(0, 0.05, 2); t[2] = rng.normal(0, 0.5)
            elif kind == 4:    # shrink: many pixels share a texel
                A[:2, :2] *= rng.uniform(0.05, 0.5); t[:2] = rng.uniform(0, 1, 2) * np.array([W, H])
            else:              # plane through the source camera centre for one depth value
                A[2, 2] = 0.0; t[2] = 0.0 if rng.random() < 0.5 else 1.0
            proj[n, j, :3, :3] = A
            proj[n, j, :3, 3] = t
    depth = np.sort(rng.uniform(0.2, 5.0, (1, D)).astype(np.float32), axis=1).repeat(N, 0)
    ref = oracle.plane_sweep_variance(feat, nbr, proj, depth, mode=1)
    args = (feat.to(gpu), torch.from_numpy(nbr).to(gpu), torch.from_numpy(proj).to(gpu), torch.from_numpy(depth).to(gpu))
    for _ in range(3):
        out = ops.plane_sweep_variance(*args).cpu().numpy()
        np.testing.assert_array_equal(np.isnan(out), np.isnan(ref))
        np.testing.assert_array_equal(out[~np.isnan(ref)], ref[~np.isnan(ref)])


# --------------------------------------------------------------------------------------------- with the real cost network
def test_forward_scene_with_cost_regularisation_network(gpu, oracle):
    """a1..a10 with the 3-D U-Net between a4 and a5 (mvsdet_amd.costreg, MIOpen): forward_scene feeds the variance
    volume to the module and its logits to the a5-a7 kernel; the stages after the network equal the oracle's on the
    network's own output, and gradients reach both the features and the network."""
    from mvsdet_amd import synthetic
    from mvsdet_amd.costreg import CostRegNet3DGS
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 3, 32, 8, (24, 32)
    torch.manual_seed(0)
    net = CostRegNet3DGS(C, base=8).to(gpu)
    hp = MVSDetHotPath([16, 16, 8], [.4, .4, .4], [0.2, 5.0], D, cost_regularization=net)
    meta = synthetic.make_img_meta(N, hw, seed=6)
    feat = synthetic.make_features(N, C, hw, seed=6).to(gpu).requires_grad_(True)
    out = hp.forward_scene(feat, meta)
    logits = net(out["variance"].detach()).detach()
    r = oracle.depth_prob_topk(logits[:, 0].cpu().numpy(), logits[:, 1].cpu().numpy(), 0.2, hp.depth_interval, 3)
    np.testing.assert_allclose(out["prob_volume"].detach().cpu().numpy(), r["prob"], rtol=0, atol=2e-6)
    sep = np.sort(r["prob"], axis=1)
    clear = (sep[:, -1] - sep[:, -2] > 1e-4) & (sep[:, -2] - sep[:, -3] > 1e-4) & (sep[:, -3] - sep[:, -4] > 1e-4)
    h, w = out["geometry"].height, out["geometry"].width
    got = out["est_depth"].detach().cpu().numpy()
    np.testing.assert_allclose(got[np.broadcast_to(clear[:, None, :h, :w], got.shape)],
                               r["est_depth"][:, :, :h, :w][np.broadcast_to(clear[:, None, :h, :w], got.shape)], rtol=0, atol=1e-5)
    (out["volume"].square().mean() + out["depth_coding"].mean()).backward()
    assert feat.grad is not None and torch.isfinite(feat.grad).all() and float(feat.grad.abs().sum()) > 0
    assert all(p.grad is not None for p in net.parameters())


@pytest.mark.parametrize("N,Cin,D,H,W", [(2, 64, 12, 60, 80), (1, 64, 5, 7, 33), (3, 6, 4, 9, 40), (1, 10, 1, 1, 1)])
def test_cost_network_head_conv(gpu, N, Cin, D, H, W):
    """csrc/costreg_head.hip (Conv3d Cin -> 2, k=3, pad=1, bias) against ATen-CPU conv3d: same sums in a different
    order, so within 1e-5 of the output scale; ragged tiles in d, h and w, Cin not a multiple of the channel chunk."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + Cin)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    wgt = torch.randn(2, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    b = torch.randn(2, generator=g)
    ref = torch.nn.functional.conv3d(x, wgt, b, padding=1)
    out = ops.conv3d_k3_cout2(x.to(gpu), wgt.to(gpu), b.to(gpu)).cpu()
    assert out.shape == ref.shape
    torch.testing.assert_close(out, ref, rtol=0, atol=1e-5 * float(ref.abs().max()))
    out0 = ops.conv3d_k3_cout2(x.to(gpu), wgt.to(gpu), None).cpu()
    torch.testing.assert_close(out0, ref - b.view(1, 2, 1, 1, 1), rtol=0, atol=1e-5 * float(ref.abs().max()))
    with pytest.raises(ValueError):
        ops.conv3d_k3_cout2(x.to(gpu), wgt[:, :, :2].contiguous().to(gpu), None)


@pytest.mark.parametrize("N,Cin,D,H,W", [(1, 256, 4, 8, 32), (2, 32, 5, 7, 33), (1, 7, 3, 5, 80), (1, 2, 1, 1, 1),
                                         (1, 8, 4, 4, 16), (1, 6, 8, 12, 48)])   # the last two pick the 4-plane tile
def test_cost_network_first_conv_mfma(gpu, N, Cin, D, H, W):
    """csrc/costreg_conv0.hip (Conv3d Cin -> 64, k=3, pad=1 on the fp32 matrix cores) against ATen-CPU conv3d, with and
    without the folded BatchNorm + ReLU epilogue; ragged tiles in d, h, w and an odd channel count."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + Cin)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    wgt = torch.randn(64, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    scale, shift = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    ref = torch.nn.functional.conv3d(x, wgt, None, padding=1)
    tol = 2e-6 * float(ref.abs().max()) * max(1.0, (27 * Cin) ** 0.5 / 8)
    wp = ops.permute_conv_weight(wgt.to(gpu))
    out = ops.conv3d_k3_mfma(x.to(gpu), wp, None, None, False).cpu()
    assert out.shape == ref.shape
    torch.testing.assert_close(out, ref, rtol=0, atol=tol)
    out2 = ops.conv3d_k3_mfma(x.to(gpu), wp, scale.to(gpu), shift.to(gpu), True).cpu()
    ref2 = torch.relu(ref * scale.view(1, 64, 1, 1, 1) + shift.view(1, 64, 1, 1, 1))
    torch.testing.assert_close(out2, ref2, rtol=0, atol=2 * tol)
    with pytest.raises(ValueError):
        ops.conv3d_k3_mfma(x.to(gpu), wp, scale.to(gpu), None, True)
    # Cout = 128: two independent 64-channel slices of the weights (conv2 / conv4 of the network)
    wgt2 = torch.randn(128, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    ref3 = torch.nn.functional.conv3d(x, wgt2, None, padding=1)
    out3 = ops.conv3d_k3_mfma(x.to(gpu), ops.permute_conv_weight(wgt2.to(gpu)), None, None, False).cpu()
    torch.testing.assert_close(out3, ref3, rtol=0, atol=2e-6 * float(ref3.abs().max()) * max(1.0, (27 * Cin) ** 0.5 / 8))
    # stride 2 (conv1 / conv3 of the network)
    ref4 = torch.nn.functional.conv3d(x, wgt, None, padding=1, stride=2)
    out4 = ops.conv3d_k3_mfma(x.to(gpu), wp, None, None, False, 2).cpu()
    assert out4.shape == ref4.shape
    torch.testing.assert_close(out4, ref4, rtol=0, atol=tol)


def test_cost_network_hip_layers_match_torch_layers(gpu):
    """CostRegNet3DGS in eval mode without autograd (HIP first conv + folded BN + ReLU, HIP head) against the same
    module evaluated with torch's own layers (autograd on), on the GPU: same network, two execution routes."""
    from mvsdet_amd.costreg import CostRegNet3DGS
    torch.manual_seed(1)
    net = CostRegNet3DGS(256).to(gpu).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.1)
    x = torch.rand(2, 256, 8, 12, 32, device=gpu)
    with torch.no_grad():
        fast = net(x)
    slow = net(x.clone().requires_grad_(True)).detach()      # autograd on: torch layers throughout
    torch.testing.assert_close(fast, slow, rtol=0, atol=2e-5 * float(slow.abs().max()))
    net.conv0.conv.weight.data.mul_(0.5)                      # the kernel reads the current weights on every call
    with torch.no_grad():
        fast2 = net(x)
    slow2 = net(x.clone().requires_grad_(True)).detach()
    torch.testing.assert_close(fast2, slow2, rtol=0, atol=2e-5 * float(slow2.abs().max()))
    assert float((fast2 - fast).abs().max()) > 1e-4


@pytest.mark.parametrize("N,Cin,Cout,D,H,W", [(1, 256, 128, 3, 15, 20), (2, 6, 64, 2, 5, 33), (1, 3, 64, 1, 1, 1)])
def test_cost_network_transposed_conv_mfma(gpu, N, Cin, Cout, D, H, W):
    """ConvTranspose3d(k=3, s=2, p=1, output_padding=1) [+ affine + ReLU + residual] on the fp32 matrix cores (eight
    output parity classes) against ATen-CPU conv_transpose3d."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + Cin)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    wgt = torch.randn(Cin, Cout, 3, 3, 3, generator=g) / (27 * Cin / 8) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    ref = torch.nn.functional.conv_transpose3d(x, wgt, None, stride=2, padding=1, output_padding=1)
    res = torch.randn(ref.shape, generator=g)
    tol = 4e-6 * float(ref.abs().max()) * max(1.0, Cin ** 0.5 / 4)
    wp = ops.permute_convT_weight(wgt.to(gpu))
    out = ops.convT3d_k3_s2_mfma(x.to(gpu), wp, None, None, None, False).cpu()
    assert out.shape == ref.shape == (N, Cout, 2 * D, 2 * H, 2 * W)
    torch.testing.assert_close(out, ref, rtol=0, atol=tol)
    out2 = ops.convT3d_k3_s2_mfma(x.to(gpu), wp, scale.to(gpu), shift.to(gpu), res.to(gpu), True).cpu()
    ref2 = res + torch.relu(ref * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1))
    torch.testing.assert_close(out2, ref2, rtol=0, atol=2 * tol)


@pytest.mark.parametrize("seed", range(6))
def test_cost_network_convs_randomised(gpu, seed):
    """Random shapes through the three matrix-core convolution entry points (stride 1, stride 2, transposed) against
    ATen-CPU: every tile variant, ragged edges in all three dimensions, odd channel counts, Cout = 64 / 128."""
    from mvsdet_amd import ops
    rng = np.random.default_rng(500 + seed)
    N, Cin = int(rng.integers(1, 3)), int(rng.integers(1, 40))
    Cout = int(rng.choice([64, 128]))
    D, H, W = int(rng.integers(1, 10)), int(rng.integers(1, 21)), int(rng.integers(1, 70))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    wgt = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    wp = ops.permute_conv_weight(wgt.to(gpu))
    for stride in (1, 2):
        ref = torch.nn.functional.conv3d(x, wgt, None, padding=1, stride=stride)
        out = ops.conv3d_k3_mfma(x.to(gpu), wp, None, None, False, stride).cpu()
        assert out.shape == ref.shape
        torch.testing.assert_close(out, ref, rtol=0, atol=3e-6 * max(1.0, float(ref.abs().max())) * max(1.0, Cin ** 0.5))
    wt = torch.randn(Cin, Cout, 3, 3, 3, generator=g) / (27 * Cin / 8) ** 0.5
    ref = torch.nn.functional.conv_transpose3d(x, wt, None, stride=2, padding=1, output_padding=1)
    out = ops.convT3d_k3_s2_mfma(x.to(gpu), ops.permute_convT_weight(wt.to(gpu)), None, None, None, False).cpu()
    torch.testing.assert_close(out, ref, rtol=0, atol=3e-6 * max(1.0, float(ref.abs().max())) * max(1.0, Cin ** 0.5))


# --------------------------------------------------------------------------------------------- unmodified variance loop
def _reference_style_variance(F_, feature, c2w, w2c, K_feat, depth_values, training):
    """The operation sequence of mvsdet.py:430-467 (restated), on the patched functions."""
    num_src = feature.shape[0]
    k = min(2, num_src - 1)
    neighbor_ids = F_.get_nearest_pose_ids(c2w, c2w, k, maskself=True)
    num_depth = depth_values.shape[1]
    ref_volume = feature.unsqueeze(2).repeat(1, 1, num_depth, 1, 1)
    volume_sum = ref_volume
    volume_sq_sum = ref_volume ** 2
    del ref_volume
    nei_features = feature[neighbor_ids.view(-1)].view(num_src, k, *feature.shape[1:])
    nei_features = torch.unbind(nei_features, dim=1)
    ref_proj, nei_projs = F_.collect_proj(w2c, K_feat, neighbor_ids)
    for nei_fea, nei_proj in zip(nei_features, nei_projs):
        warped_volume = F_.homo_warping(nei_fea, nei_proj, ref_proj, depth_values)
        if training:
            volume_sum = volume_sum + warped_volume
            volume_sq_sum = volume_sq_sum + warped_volume ** 2
        else:
            volume_sum += warped_volume
            volume_sq_sum += warped_volume.pow_(2)
        del warped_volume
    return volume_sq_sum.div_(k + 1).sub_(volume_sum.div_(k + 1).pow_(2)), neighbor_ids


@pytest.mark.parametrize("training", [False, True])
def test_unmodified_variance_loop_collapses_into_the_fused_kernel(gpu, oracle, training):
    """With the function-level patch `homo_warping` returns deferred volumes (mvsdet_amd/lazywarp.py): the reference's
    own loop then costs ONE fused plane-sweep launch and gives the fused kernel's bits; a loop that does something
    else with the volumes falls back to the eager kernels and still gives the right values."""
    from mvsdet_amd import functional as F_, lazywarp, ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 5, 32, 8, (24, 32)
    hp = MVSDetHotPath([8, 8, 4], [.8, .8, .8], [0.2, 5.0], D)
    meta = synthetic.make_img_meta(N, hw, seed=8)
    geo = hp.prepare_scene(meta, gpu)
    w2c = torch.tensor(np.array(meta["lidar2img"]["extrinsic"]))
    K_feat = torch.tensor(oracle.feat_intrinsics(meta["lidar2img"]["intrinsic"], meta["img_shape"], meta["ori_shape"]))
    c2w = w2c.inverse()
    feature = synthetic.make_features(N, C, hw, seed=8).to(gpu).requires_grad_(training)
    expected = ops.plane_sweep_variance(feature.detach(), geo.neighbor_ids, geo.proj_rel, geo.depth_values)
    old = F_.LAZY_WARP
    F_.LAZY_WARP = True
    try:
        before = dict(lazywarp.stats)
        var, ids = _reference_style_variance(F_, feature, c2w, w2c, K_feat, geo.depth_values, training)
        assert type(var) is torch.Tensor and lazywarp.stats["fused"] == before["fused"] + 1
        assert lazywarp.stats["materialized"] == before["materialized"]            # no volume was ever materialised
        assert torch.equal(ids.to(gpu), geo.neighbor_ids) and torch.equal(var, expected)
        if training:
            var.square().mean().backward()
            g_lazy = feature.grad.clone()
            feature.grad = None
            ops.plane_sweep_variance(feature, geo.neighbor_ids, geo.proj_rel, geo.depth_values).square().mean().backward()
            torch.testing.assert_close(g_lazy, feature.grad, rtol=1e-4, atol=1e-7)
        # a different loop: the volume is inspected, then combined in another order -> eager kernels, same values
        nb = F_.get_nearest_pose_ids(c2w, c2w, 2, maskself=True)
        ref_proj, nei_projs = F_.collect_proj(w2c, K_feat, nb)
        w0 = F_.homo_warping(feature.detach()[nb[:, 0]], nei_projs[0], ref_proj, geo.depth_values)
        assert isinstance(w0, lazywarp.LazyVolume) and tuple(w0.shape) == (N, C, D) + hw and w0.device.type == "cuda"
        m = float(w0.mean())                                                         # materialises
        eager = ops.homo_warp(feature.detach()[nb[:, 0]], geo.proj_rel[:, 0].contiguous(), geo.depth_values)
        assert abs(m - float(eager.mean())) < 1e-6 and lazywarp.stats["materialized"] > before["materialized"]
        mixed = (w0 * 2.0 + 1.0)
        assert type(mixed) is torch.Tensor and torch.equal(mixed, eager * 2.0 + 1.0)
    finally:
        F_.LAZY_WARP = old


def test_patched_route_with_device_cameras_and_its_wall_time(gpu):
    """mvsdet.py:419-467 (restated) as the reference runs it: `w2c` and `K` are DEVICE tensors (:419-420), neighbour ids,
    projections and depth values live on the device.  Under the patch `MVSDet.collect_proj` copies the cameras to the host
    once and evaluates the k matrices `nei_proj @ inverse(ref_proj)` of the scene there (functional.collect_proj_for_scene),
    the k `homo_warping` calls look theirs up, and the loop collapses into one fused launch: the result is the fused
    kernel's, bit for bit, and the wall time of the whole route is recorded beside the fused stage alone (the rest is the
    reference's own `repeat` / `** 2` of the (N,C,D,H,W) reference volume and the recognition checks)."""
    import json
    import os
    import time
    from mvsdet_amd import functional as F_, integration, lazywarp, ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 40, 64, 12, (60, 80)
    hp = MVSDetHotPath([40, 40, 16], [.16, .16, .2], [0.2, 5.0], D)
    meta = synthetic.make_img_meta(N, hw, seed=12)
    geo = hp.prepare_scene(meta, gpu)
    feature = synthetic.make_features(N, C, hw, seed=12).to(gpu)
    w2c = torch.tensor(np.array(meta["lidar2img"]["extrinsic"]), device=gpu)
    # feature-level intrinsics evaluated on the host and uploaded: ATen's device kernel divides by a scalar as a multiplication
    # by its reciprocal -- one ulp in K, 1e-5 in the variance (DESIGN "tolerance budget") -- and this test is about the ROUTE
    K_feat = torch.tensor(np.array(meta["lidar2img"]["intrinsic"]))
    K_feat[:2] /= meta["ori_shape"][0] / (meta["img_shape"][0] / 4)
    K_feat = K_feat.to(gpu)
    expected = ops.plane_sweep_variance(feature, geo.neighbor_ids, geo.proj_rel, geo.depth_values)

    class Patched:          # the two patched entry points the block calls, as integration.patch_reference binds them
        get_nearest_pose_ids = staticmethod(F_.get_nearest_pose_ids)
        homo_warping = staticmethod(F_.homo_warping)
        collect_proj = staticmethod(lambda w, k, ids: integration.PATCHED_METHODS["collect_proj"](None, w, k, ids))

    old = F_.LAZY_WARP
    F_.LAZY_WARP = True
    try:
        times = []
        for rep in range(4):
            before = dict(lazywarp.stats)
            torch.cuda.synchronize(gpu)
            t0 = time.perf_counter()
            c2w = w2c.inverse()                                             # mvsdet.py:433, on the device
            var, ids = _reference_style_variance(Patched, feature, c2w, w2c, K_feat, geo.depth_values, False)
            torch.cuda.synchronize(gpu)
            times.append((time.perf_counter() - t0) * 1e3)
            assert lazywarp.stats["fused"] == before["fused"] + 1 and lazywarp.stats["materialized"] == before["materialized"]
            assert var.is_cuda and torch.equal(var, expected) and torch.equal(ids, geo.neighbor_ids)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.plane_sweep_variance(feature, geo.neighbor_ids, geo.proj_rel, geo.depth_values)
        e1.record()
        torch.cuda.synchronize(gpu)
        rec = {"shape": [N, C, D, *hw], "patched_route_ms": [round(t, 3) for t in times], "fused_stage_ms": round(e0.elapsed_time(e1), 3)}
        print("patched route timing", json.dumps(rec))
        out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
        if os.path.isdir(out_dir):
            with open(os.path.join(out_dir, "patched_route_timing.json"), "w") as fh:
                json.dump(rec, fh)
        assert min(times[1:]) < 50.0        # a few ms on an MI355X; the bound only catches a fall-back to k materialised volumes
    finally:
        F_.LAZY_WARP = old


def test_unmodified_lifting_block_uses_the_fused_kernel(gpu, oracle):
    """mvsdet.py:497-513 on the patched backproject_Weigh: `volume.sum(dim=0)` and `valid.sum(dim=0)` of the deferred
    volumes run ONE fused lifting launch; indexing the volume instead materialises the per-view result."""
    from mvsdet_amd import functional as F_, lazywarp, ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    N, C, D, hw = 6, 32, 12, (24, 32)
    hp = MVSDetHotPath([16, 16, 8], [.4, .4, .4], [0.2, 5.0], D)
    meta = synthetic.make_img_meta(N, hw, seed=12)
    feat = synthetic.make_features(N, C, hw, seed=12).to(gpu)
    logits = synthetic.make_cost_logits(N, D, hw, seed=12, sharp=2.0).to(gpu)
    out = hp.forward_scene(feat, meta, cost_logits=logits)
    geo = out["geometry"]
    h, w = geo.height, geo.width
    # the reference's argument layout: (N, h*w, 1, J)
    est_depth = out["est_depth"].reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)
    est_dens = out["est_densities"].reshape(N, 3, -1).transpose(2, 1).unsqueeze(2)
    old = F_.LAZY_WARP
    F_.LAZY_WARP = True
    try:
        before = dict(lazywarp.stats)
        volume, valid, _, _ = F_.backproject_Weigh(feat[:, :, :h, :w], geo.points, geo.projection, est_depth, hp.voxel_size,
                                                   est_dens)
        assert isinstance(volume, lazywarp.LazyVolume) and tuple(volume.shape) == (N, C, 16, 16, 8)
        volume_sum = volume.sum(dim=0)
        valid_cnt = valid.sum(dim=0)
        volume_mean = volume_sum / (valid_cnt + 1e-8)
        volume_mean[:, valid_cnt[0] == 0] = .0
        assert lazywarp.stats["fused"] == before["fused"] + 1 and lazywarp.stats["materialized"] == before["materialized"]
        assert torch.equal(valid_cnt, out["valid"])
        np.testing.assert_allclose(volume_mean.cpu().numpy(), out["volume"].cpu().numpy(), rtol=0, atol=2e-6)
        # another use of the volume: per-view slices -> the eager operator
        eager_vol, eager_valid = ops.backproject_weigh(feat[:, :, :h, :w], geo.points, geo.projection,
                                                       out["est_depth"], out["est_densities"], hp.voxel_size[-1])
        assert torch.equal(volume[2], eager_vol.view(N, C, 16, 16, 8)[2])
        assert torch.equal(valid.float().sum(), eager_valid.float().sum())
    finally:
        F_.LAZY_WARP = old


@pytest.mark.parametrize("N,Cin,Cout,D,H,W,nsplit", [(2, 32, 64, 3, 8, 16, 4), (1, 40, 70, 2, 5, 19, 3), (2, 5, 3, 1, 1, 1, 2),
                                                     (1, 64, 32, 4, 9, 33, 200)])
def test_cost_network_weight_gradient_mfma(gpu, N, Cin, Cout, D, H, W, nsplit):
    """dW of Conv3d(k=3, s=1, p=1) on the fp32 matrix cores (csrc/costreg_dw.hip) against ATen-CPU's conv3d_weight;
    the input gradient through the forward kernel with transposed, flipped weights against conv3d_input."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 100 + Cin)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    gy = torch.randn(N, Cout, D, H, W, generator=g)
    wgt = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    ref_w = torch.nn.grad.conv3d_weight(x, wgt.shape, gy, padding=1)
    got_w = ops.conv3d_k3_dw(x.to(gpu), gy.to(gpu), nsplit).cpu()
    assert got_w.shape == ref_w.shape
    torch.testing.assert_close(got_w, ref_w, rtol=0, atol=3e-6 * float(ref_w.abs().max()) * max(1.0, (N * D * H * W) ** 0.5 / 8))
    if Cin % 64 == 0:   # dX = conv(dY, W^T flipped): the output channel count of that convolution is Cin
        ref_x = torch.nn.grad.conv3d_input(x.shape, wgt, gy, padding=1)
        wflip = wgt.transpose(0, 1).flip(2, 3, 4).contiguous()
        got_x = ops.conv3d_k3_mfma(gy.to(gpu), ops.permute_conv_weight(wflip.to(gpu)), None, None, False).cpu()
        torch.testing.assert_close(got_x, ref_x, rtol=0, atol=3e-6 * float(ref_x.abs().max()) * max(1.0, (27 * Cout) ** 0.5 / 8))


@pytest.mark.parametrize("N,Cin,Cout,D,H,W,nsplit", [(2, 64, 128, 4, 8, 16, 4), (1, 40, 70, 2, 10, 36, 3), (2, 5, 3, 2, 2, 2, 2),
                                                     (1, 64, 64, 6, 14, 34, 200)])
def test_cost_network_stride2_gradients(gpu, N, Cin, Cout, D, H, W, nsplit):
    """The stride-2 layers (conv1, conv3) and the transposed ones (conv9, conv11) under autograd: dW on the strided
    weight-gradient kernel -- for the transposed layers with the two tensors exchanged -- and the input gradients through
    each other's forward kernels, against ATen-CPU's conv3d_weight / conv3d_input / autograd of conv_transpose3d."""
    from mvsdet_amd import ops
    F = torch.nn.functional
    g = torch.Generator().manual_seed(N * 100 + Cin)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    gy = torch.randn(N, Cout, D // 2, H // 2, W // 2, generator=g)
    wgt = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    nv = N * D * H * W / 8
    # Conv3d stride 2
    ref_w = torch.nn.grad.conv3d_weight(x, wgt.shape, gy, stride=2, padding=1)
    got_w = ops.conv3d_k3_dw(x.to(gpu), gy.to(gpu), nsplit, 2).cpu()
    assert got_w.shape == ref_w.shape
    torch.testing.assert_close(got_w, ref_w, rtol=0, atol=3e-6 * float(ref_w.abs().max()) * max(1.0, nv ** 0.5 / 8))
    if Cin % 64 == 0:
        ref_x = torch.nn.grad.conv3d_input(x.shape, wgt, gy, stride=2, padding=1)
        got_x = ops.convT3d_k3_s2_mfma(gy.to(gpu), ops.permute_convT_weight(wgt.to(gpu)), None, None, None, False).cpu()
        torch.testing.assert_close(got_x, ref_x, rtol=0, atol=3e-6 * float(ref_x.abs().max()) * max(1.0, (27 * Cout) ** 0.5 / 8))
    # ConvTranspose3d(k3, s2, p1, op1) with weight (Cout -> Cin): input `gy`-shaped, output `x`-shaped
    xt = gy.clone().requires_grad_(True)
    wt = wgt.clone().requires_grad_(True)          # (Cout, Cin, 3,3,3) = (in, out, ...) of the transposed layer
    F.conv_transpose3d(xt, wt, stride=2, padding=1, output_padding=1).backward(x)
    got_wt = ops.conv3d_k3_dw(x.to(gpu), gy.to(gpu), nsplit, 2).cpu()   # fine tensor first, coarse one second
    torch.testing.assert_close(got_wt, wt.grad, rtol=0, atol=3e-6 * float(wt.grad.abs().max()) * max(1.0, nv ** 0.5 / 8))
    if Cout % 64 == 0:
        got_xt = ops.conv3d_k3_mfma(x.to(gpu), ops.permute_conv_weight(wgt.to(gpu)), None, None, False, 2).cpu()
        torch.testing.assert_close(got_xt, xt.grad, rtol=0, atol=3e-6 * float(xt.grad.abs().max()) * max(1.0, (27 * Cin) ** 0.5 / 8))


def test_cost_network_training_gradients_hip_vs_torch(gpu):
    """CostRegNet3DGS under autograd: with `hip_backward` every convolution (stride 1, stride 2, transposed, head) runs
    forward, dX and dW on our kernels; outputs and every parameter / input gradient agree with the all-torch route."""
    from mvsdet_amd.costreg import CostRegNet3DGS
    torch.manual_seed(3)
    # BatchNorm on its running statistics: with batch statistics over the few quarter-resolution voxels of this small
    # volume the summation-order noise of two correct convolutions is amplified beyond any useful tolerance
    net = CostRegNet3DGS(256).to(gpu).eval()
    net.matrix_precision = "fp32"     # bit-level fp32 FMA sums on both routes: no ReLU decision differs (bf16x3: next test)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
    x = torch.rand(2, 256, 8, 12, 32, device=gpu)
    target = torch.randn(2, 2, 8, 12, 32, device=gpu)
    grads = {}
    for flag in (True, False):
        net.hip_backward = flag
        net.zero_grad(set_to_none=True)
        xin = x.clone().requires_grad_(True)
        out = net(xin)
        ((out - target) ** 2).mean().backward()
        grads[flag] = (out.detach().clone(), xin.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters()})
    o1, gx1, gp1 = grads[True]
    o0, gx0, gp0 = grads[False]
    torch.testing.assert_close(o1, o0, rtol=0, atol=2e-5 * float(o0.abs().max()))
    torch.testing.assert_close(gx1, gx0, rtol=0, atol=1e-4 * float(gx0.abs().max()))
    for k in gp0:
        torch.testing.assert_close(gp1[k], gp0[k], rtol=0, atol=1e-4 * max(float(gp0[k].abs().max()), 1e-12), msg=k)


def test_cost_network_training_on_bf16x3(gpu):
    """Under autograd with `matrix_precision = "bf16x3"` (the default) forward and input gradient of every 3x3x3 layer run
    on the bf16 matrix cores with three-term split operands, and so do the weight gradients of the stride-1 layers.  Every
    layer pass is within 1e-5 of its fp32 counterpart (checked per autograd Function); through the network a forward
    difference of that size flips the ReLU decision of the few activations that sit within it of zero, so gradients are
    compared in norm: a few 1e-3, set by how many activations flip, not by the arithmetic of a layer (2.4e-3 at this shape)."""
    from mvsdet_amd import costreg as CR, layers
    torch.manual_seed(5)
    for fn, xs, ws in ((layers.ConvK3S1, (2, 256, 8, 12, 32), (64, 256, 3, 3, 3)), (layers.ConvK3S2, (2, 64, 8, 12, 32), (128, 64, 3, 3, 3)),
                       (layers.ConvT3S2, (2, 128, 4, 6, 16), (128, 64, 3, 3, 3))):
        x, w = torch.randn(*xs, device=gpu), torch.randn(*ws, device=gpu) / 30
        res = {}
        for bf in (False, True):
            xi, wi = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            y = fn.apply(xi, wi, bf)
            y.backward(torch.randn(y.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1)))
            res[bf] = (y.detach(), xi.grad, wi.grad)
        for a, b in zip(res[False], res[True]):
            assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max()), fn.__name__
    net = CR.CostRegNet3DGS(256).to(gpu).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
    x = torch.rand(2, 256, 8, 12, 32, device=gpu)
    target = torch.randn(2, 2, 8, 12, 32, device=gpu)
    grads = {}
    for prec in ("bf16x3", "fp32"):
        net.matrix_precision = prec
        net.zero_grad(set_to_none=True)
        xin = x.clone().requires_grad_(True)
        out = net(xin)
        ((out - target) ** 2).mean().backward()
        grads[prec] = (out.detach().clone(), xin.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters()})
    o1, gx1, gp1 = grads["bf16x3"]
    o0, gx0, gp0 = grads["fp32"]
    torch.testing.assert_close(o1, o0, rtol=0, atol=2e-5 * float(o0.abs().max()))
    rel = lambda a, b: float((a - b).norm()) / max(float(b.norm()), 1e-30)   # noqa: E731
    assert rel(gx1, gx0) < 5e-3
    for k in gp0:
        assert rel(gp1[k], gp0[k]) < 5e-3, k


@pytest.mark.parametrize("N,Cin,D,H,W", [(2, 64, 12, 20, 40), (1, 6, 5, 7, 33), (1, 3, 1, 1, 1)])
def test_cost_network_head_backward(gpu, N, Cin, D, H, W):
    """Gradients of the head convolution (64 -> 2) from the streaming kernels against ATen-CPU's conv3d_input /
    conv3d_weight."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 10 + Cin)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    wgt = torch.randn(2, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    gy = torch.randn(N, 2, D, H, W, generator=g)
    ref_x = torch.nn.grad.conv3d_input(x.shape, wgt, gy, padding=1)
    ref_w = torch.nn.grad.conv3d_weight(x, wgt.shape, gy, padding=1)
    gx, gw = ops.conv3d_k3_cout2_backward(x.to(gpu), wgt.to(gpu), gy.to(gpu), 5)
    torch.testing.assert_close(gx.cpu(), ref_x, rtol=0, atol=1e-5 * float(ref_x.abs().max()))
    torch.testing.assert_close(gw.cpu(), ref_w, rtol=0, atol=3e-6 * float(ref_w.abs().max()) * max(1.0, (N * D * H * W) ** 0.5 / 8))


@pytest.mark.parametrize("N,C,D,H,W", [(2, 8, 4, 6, 12), (3, 5, 3, 5, 7)])
def test_batchnorm_relu_with_residual(gpu, N, C, D, H, W):
    """`skip + relu(bn(x))` (mvsnet.py:109-111) in the BatchNorm's second pass: the output is the two-pass result plus the skip
    tensor bit for bit, the skip's gradient is grad_out, the others are those of the call without a residual."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(C * 7 + N)
    x, skip, gy = (torch.randn(N, C, D, H, W, generator=g).to(gpu) for _ in range(3))
    wgt, b = (torch.rand(C, generator=g) + 0.5).to(gpu), torch.randn(C, generator=g).to(gpu)
    leaves = lambda: [t.clone().requires_grad_(True) for t in (x, wgt, b, skip)]   # noqa: E731
    x1, w1, b1, s1 = leaves()
    out1, mean1, inv1 = ops.bn3d_relu_train(x1, w1, b1, 1e-5, True, s1)
    out1.backward(gy)
    x0, w0, b0, s0 = leaves()
    out0, mean0, inv0 = ops.bn3d_relu_train(x0, w0, b0, 1e-5, True)
    (out0 + s0).backward(gy)
    assert torch.equal(out1, out0 + s0) and torch.equal(mean1, mean0) and torch.equal(inv1, inv0)
    assert torch.equal(s1.grad, gy) and torch.equal(x1.grad, x0.grad) and torch.equal(w1.grad, w0.grad) and torch.equal(b1.grad, b0.grad)


@pytest.mark.parametrize("N,Cin,D,H,W", [
    (2, 64, 12, 20, 40),   # the shipped head: 64 channels; W = 40: a second k-step with 8 of its 32 voxels
    (1, 64, 3, 5, 80),     # the reference-true row length (two and a half k-steps)
    (3, 32, 2, 7, 4),      # two channel tiles, rows shorter than one k-step, more waves than rows in some blocks
    (1, 16, 1, 1, 36),     # one channel tile, a single row: every neighbouring row is padding
    (2, 64, 4, 9, 128),    # whole k-steps only
])
def test_cost_network_head_weight_gradient_bf16x3(gpu, N, Cin, D, H, W):
    """The head's weight gradient on the bf16 matrix cores with three-term split operands (csrc/costreg_head.hip:
    conv3d_k3_cout2_dw_bf16x3_kernel) against ATen-CPU's conv3d_weight in double, and the input gradient it travels with."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(N * 10 + Cin + W)
    x = torch.randn(N, Cin, D, H, W, generator=g)
    wgt = torch.randn(2, Cin, 3, 3, 3, generator=g) / (27 * Cin) ** 0.5
    gy = torch.randn(N, 2, D, H, W, generator=g)
    ref_w = torch.nn.grad.conv3d_weight(x.double(), wgt.shape, gy.double(), padding=1)
    gx, gw = ops.conv3d_k3_cout2_backward(x.to(gpu), wgt.to(gpu), gy.to(gpu), 5, True)
    gx0, gw0 = ops.conv3d_k3_cout2_backward(x.to(gpu), wgt.to(gpu), gy.to(gpu), 5, False)
    assert torch.equal(gx, gx0)
    scale = float(ref_w.abs().max())
    # three-term split products: 2^-16 of |x||gy| per product, summed over N*D*H*W of them
    assert float((gw.cpu().double() - ref_w).abs().max()) <= 1e-5 * scale * max(1.0, (N * D * H * W) ** 0.5 / 8)
    assert float((gw - gw0).abs().max()) <= 2e-5 * scale * max(1.0, (N * D * H * W) ** 0.5 / 8)


@pytest.mark.parametrize("N,C,D,H,W,relu", [(2, 8, 4, 6, 12, True), (3, 5, 3, 5, 7, True), (1, 64, 2, 4, 8, False), (2, 3, 1, 1, 1, True)])
def test_batchnorm_relu_training_kernels(gpu, N, C, D, H, W, relu):
    """Training-mode BatchNorm3d [+ ReLU] (csrc/costreg_bn.hip) against ATen-CPU: output, batch statistics, and the gradients
    with respect to x, gamma and beta."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(C * 10 + N)
    x = (torch.randn(N, C, D, H, W, generator=g) * 2 + 0.5)
    wgt, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    gy = torch.randn(N, C, D, H, W, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), wgt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = torch.nn.functional.batch_norm(xr, None, None, wr, br, True, 0.1, 1e-5)
    if relu:
        ref = torch.relu(ref)
    ref.backward(gy)
    xg, wg, bg = x.to(gpu).requires_grad_(True), wgt.to(gpu).requires_grad_(True), b.to(gpu).requires_grad_(True)
    out, mean, invstd = ops.bn3d_relu_train(xg, wg, bg, 1e-5, relu)
    out.backward(gy.to(gpu))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(mean.detach().cpu().numpy(), x.mean(dim=(0, 2, 3, 4)).numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(invstd.detach().cpu().numpy(), (1.0 / torch.sqrt(x.var(dim=(0, 2, 3, 4), unbiased=False) + 1e-5)).numpy(), rtol=1e-5)
    for got, want in ((xg.grad, xr.grad), (wg.grad, wr.grad), (bg.grad, br.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5 * max(1.0, float(want.abs().max())))


def test_batchnorm_training_statistics_of_offset_channels(gpu):
    """Channels whose mean is ~1000x their spread (behind a large bias): E[x^2] - mean^2 on raw fp32 strips would lose the
    variance entirely; the kernel sums around a per-channel pivot.  Against a float64 evaluation (torch.nn.BatchNorm3d
    uses Welford and is itself within 1e-4 here)."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(77)
    N, C, D, H, W = 3, 6, 4, 10, 12
    off = torch.tensor([1000.0, -1000.0, 300.0, 0.0, 5000.0, -50.0]).view(1, C, 1, 1, 1)
    x = torch.randn(N, C, D, H, W, generator=g) * torch.tensor([1.0, 0.5, 0.3, 2.0, 4.0, 0.05]).view(1, C, 1, 1, 1) + off
    wgt, b = torch.ones(C), torch.zeros(C)
    out, mean, invstd = ops.bn3d_relu_train(x.to(gpu), wgt.to(gpu), b.to(gpu), 1e-5, False)
    x64 = x.double()
    m64 = x64.mean(dim=(0, 2, 3, 4))
    v64 = x64.var(dim=(0, 2, 3, 4), unbiased=False)
    np.testing.assert_allclose(mean.cpu().numpy(), m64.numpy(), rtol=1e-6)
    np.testing.assert_allclose(invstd.cpu().numpy(), (1.0 / torch.sqrt(v64 + 1e-5)).numpy(), rtol=2e-5)
    ref = ((x64 - m64.view(1, C, 1, 1, 1)) / torch.sqrt(v64 + 1e-5).view(1, C, 1, 1, 1)).float()
    # fp32 x * scale + shift at |x| = 5000 carries a few ulp(|x| / std) of absolute error: compare at that scale
    tol = (x.abs().amax(dim=(0, 2, 3, 4)) * 6e-7 / torch.sqrt(v64.float())).view(1, C, 1, 1, 1) + 1e-5
    assert bool(((out.cpu() - ref).abs() <= tol).all())


def test_cost_network_training_mode_batchnorm(gpu):
    """CostRegNet3DGS in train() mode: BatchNorm on batch statistics through our kernels (hip_backward) against the
    framework's layers -- outputs, running statistics and num_batches_tracked; gradients flow to every parameter."""
    from mvsdet_amd.costreg import CostRegNet3DGS
    torch.manual_seed(4)
    nets = [CostRegNet3DGS(64, base=64).to(gpu).train() for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    nets[1].hip_backward = False
    x = torch.rand(2, 64, 8, 16, 32, device=gpu)
    outs = []
    for net in nets:
        out = net(x)
        out.square().mean().backward()
        outs.append(out.detach())
    torch.testing.assert_close(outs[0], outs[1], rtol=0, atol=2e-4 * float(outs[1].abs().max()))
    sd0, sd1 = nets[0].state_dict(), nets[1].state_dict()
    for k in sd0:
        if "running_" in k:
            torch.testing.assert_close(sd0[k], sd1[k], rtol=1e-4, atol=1e-6, msg=k)
        if "num_batches_tracked" in k:
            assert int(sd0[k]) == int(sd1[k]) == 1, k
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in nets[0].parameters())


def test_cost_network_batchnorm_statistics_from_the_epilogues_or_from_their_own_pass(gpu):
    """The two training routes of the BatchNorm statistics -- partial sums left by the producing convolution's epilogue (default) and
    the separate pass over the tensor (`layers.FUSED_BN_STATS = False`, MVSDET_FUSED_BN_STATS=0) -- on one network at a shape whose
    stride-1 and transposed layers all have the fused form (12 x 60 x 80, as the reference-true shape), ELEMENT-WISE: statistics
    that differ in the last bits move activations by ~1e-7, and one activation of a layer's N on the other side of zero would
    move that layer's gradient by sqrt(2 / N) in norm (round 5 could only hold the gradients to their direction for that reason).
    So the ReLU decisions of ONE pass (the separate-pass route, on a copy of the network) are imposed on both routes
    (layers.RELU_MASKS): both then compute the same piecewise-linear function, and logits, running statistics and every parameter
    gradient must agree to 1e-5 of each tensor's scale -- a wrong term in either statistics form shows.  A second step starts from
    running means that are no longer zero (the pivots).  Against the REFERENCE's gradients the same routes are held by G12c
    (tests/test_f3_goldens.py)."""
    import copy
    from mvsdet_amd import layers
    from mvsdet_amd.costreg import CostRegNet3DGS
    torch.manual_seed(9)
    nets = [CostRegNet3DGS(64, base=64).to(gpu).train() for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    x = torch.rand(2, 64, 12, 60, 80, device=gpu)
    was = layers.FUSED_BN_STATS, layers.RELU_MASKS
    try:
        for step in range(2):
            xin = x + 0.1 * step
            # the decisions of this step: one pass of the separate-pass route on a copy (its running statistics move, not the nets')
            probe = copy.deepcopy(nets[1])
            layers.FUSED_BN_STATS, layers.RELU_MASKS = False, ("record", {})
            with torch.enable_grad():
                probe(xin)
            by_name = {name: layers.RELU_MASKS[1][m] for name, m in probe.named_modules() if m in layers.RELU_MASKS[1]}
            assert len(by_name) == 7 and all(0.2 < float(v.float().mean()) < 0.8 for v in by_name.values())
            outs = []
            for fused, net in zip((True, False), nets):
                mods = dict(net.named_modules())
                layers.FUSED_BN_STATS, layers.RELU_MASKS = fused, ("apply", {mods[k]: v for k, v in by_name.items()})
                net.zero_grad(set_to_none=True)
                out = net(xin)
                out.square().mean().backward()
                outs.append(out.detach())
            torch.testing.assert_close(outs[0], outs[1], rtol=0, atol=1e-5 * float(outs[1].abs().max()))
            sd0, sd1 = nets[0].state_dict(), nets[1].state_dict()
            for k in sd0:
                if "running_" in k:
                    torch.testing.assert_close(sd0[k], sd1[k], rtol=1e-5, atol=1e-7, msg=k)
            worst = 0.0
            for (name, p0), (_, p1) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
                scale = float(p1.grad.abs().max())
                err = float((p0.grad - p1.grad).abs().max())
                worst = max(worst, err / max(scale, 1e-30))
                assert err <= 1e-5 * scale, (step, name, err, scale)
            print(f"BatchNorm statistics routes, step {step}: max |d grad| / scale = {worst:.2e}")
    finally:
        layers.FUSED_BN_STATS, layers.RELU_MASKS = was


def test_depth_prob_topk_reads_the_network_output_in_place(gpu):
    """The two logit maps as channel slices of one (N, 2, D, H, W) tensor (mvsdet.py:469) are read through a view stride:
    the same bits as from contiguous copies, also for a batch-sliced and for a transposed (copied) input."""
    from mvsdet_amd import ops
    g = torch.Generator().manual_seed(11)
    both = torch.randn(5, 2, 12, 9, 14, generator=g).to(gpu)
    ref = ops.depth_prob_topk(both[:, 0].contiguous(), both[:, 1].contiguous(), 0.2, 0.4, 3)
    got = ops.depth_prob_topk(both[:, 0], both[:, 1], 0.2, 0.4, 3)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    got = ops.depth_prob_topk(both[1:4, 0], both[1:4, 1], 0.2, 0.4, 3)
    ref = ops.depth_prob_topk(both[1:4, 0].contiguous(), both[1:4, 1].contiguous(), 0.2, 0.4, 3)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    tr = both.transpose(3, 4)   # inner block not dense: falls back to a copy
    got = ops.depth_prob_topk(tr[:, 0], tr[:, 1], 0.2, 0.4, 3)
    ref = ops.depth_prob_topk(tr[:, 0].contiguous(), tr[:, 1].contiguous(), 0.2, 0.4, 3)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
