"""The reference's own `MVSDet.extract_feat` called with `depth=[gt]` (what `predict` does when the test pipeline collects depth:
the configs' `use_depth`), through `integration.patch_reference`.  Pattern of tests/test_integration.py: needs the reference tree
(skipped elsewhere), CPU only -- the fused launches are replaced by the oracle, the diagnostics operator by the restatement of
tests/depth_diag_restated.py fed the oracle's stage 3 and ATen-CPU's resize, and every call is counted.

The scene is fixture G5's ScanNet-like one (its feature maps, its cameras, the logits it was made from) with G20's planted ground
truth; the cost network is a stand-in that hands out those logits, so the patched and the unpatched run see the same depth
candidates.  `weight_gap` is compared with the unpatched reference run of the same call AND with G20's gap_all (the same voxels,
weights and ground truth); `src_rmse` with the unpatched run only: extract_feat hands backproject_Weigh the depth expectation over
all planes, G20 was made with the mean of the three candidates.  Bar: the fp32 summation bound of test_depth_diag_host.py.
"""
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
from depth_diag_restated import resize_aten_cpu, restate, summation_bound

pytestmark = pytest.mark.refcheck


@pytest.fixture(scope="module")
def reference():
    sys.path.insert(0, GOLDEN)
    try:
        from _ref_loader import load_reference
        return load_reference()
    except FileNotFoundError:
        pytest.skip("reference tree not mounted")


def test_extract_feat_with_depth_runs_through_the_patch(reference, oracle, monkeypatch, capsys):
    import torch
    from mvsdet_amd import integration, lazywarp, ops, synthetic
    from test_depth_diag_host import g20_case
    from test_host_logic import meta_from
    from test_integration import _oracle_backed_ops
    ref, _ = reference
    c = g20_case("scannet", oracle)
    g5, N = c["g5"], c["N"]
    C, D = g5["feature"].shape[1], 12
    feature = torch.from_numpy(g5["feature"])
    logits = synthetic.make_cost_logits(N, D, (60, 80), seed=51, sharp=2.0)        # what G5's candidates were made from
    meta = meta_from(g5)
    gt = torch.from_numpy(c["gt"])
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)

    def make_detector():
        det = ref.MVSDet.__new__(ref.MVSDet)                     # the reference class; __init__ needs mmengine's registry
        torch.nn.Module.__init__(det)
        det.backbone = lambda img: feature
        det.neck = lambda x: [x]
        det.neck_3d = lambda x: x
        det.head_2d = None
        det.n_voxels, det.voxel_size, det.near_far_range, det.topk = [40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], 3
        det.gs_cfg = SimpleNamespace(num_monocular_samples=D)
        det.depth_interval = (5.0 - 0.2) / D                      # mvsdet.py:221-225
        det.depth_values = np.arange(0.2, 5.0, det.depth_interval, dtype=np.float32)
        det.cost_regularization = lambda variance: logits
        det.eval()
        return det

    def run(det, **kw):
        with torch.no_grad():
            return det.extract_feat({"imgs": torch.zeros(1, N, 3, 240, 320)}, [SimpleNamespace(metainfo=meta)], "test", depth=[gt], **kw)

    plain = run(make_detector())                                  # the unpatched reference (prints its per-view line)
    capsys.readouterr()
    calls = _oracle_backed_ops(monkeypatch, oracle)
    calls["diag"] = 0
    seen = {}

    def diagnostics(points, projection, est_depth, est_dens, depth_mean, gt_depth, vz):
        calls["diag"] += 1
        n, _, h, w = est_depth.shape
        o = oracle.backproject_weigh(np.ones((n, 1, h, w), np.float32), points.reshape(3, -1).numpy(), projection.numpy(),
                                     est_depth.numpy(), est_dens.numpy(), vz, want_index=True)
        g = resize_aten_cpu(gt_depth, h, w)
        r = restate(o["x"], o["y"], o["z"], g, o["volume"][:, 0], o["valid"], depth_mean.numpy(), vz)
        seen.update(r, depth_mean_strides=depth_mean.stride(), shape=(h, w))
        return tuple(torch.from_numpy(np.asarray(v)) for v in (r["scalars"], r["per_view"], r["sums"], g))

    monkeypatch.setattr(ops, "depth_diagnostics", diagnostics)
    orig = integration.patch_reference(ref)
    try:
        before = dict(lazywarp.stats)
        got = run(make_detector())
        assert lazywarp.stats["fused"] == before["fused"] + 2 and lazywarp.stats["materialized"] == before["materialized"]
        assert lazywarp.stats["diagnostics"] == before["diagnostics"] + 1
        assert calls["sweep"] == 1 and calls["lift"] == 1 and calls["diag"] == 1      # one fused sweep, one fused lifting, one diagnostics call
        with pytest.raises(NotImplementedError, match="save_dir"):
            run(make_detector(), save_dir="x")
        with pytest.raises(ValueError, match="depth_mean"):
            ref.backproject_Weigh(feature[:, :, :59, :80], torch.zeros(3, 2, 2, 2), torch.zeros(N, 3, 4), torch.ones(N, 59 * 80, 1, 3),
                                  [0.16, 0.16, 0.2], torch.ones(N, 59 * 80, 1, 3), gt_depth=gt)
    finally:
        integration.unpatch_reference(ref, orig)
    assert seen["shape"] == (59, 80) and seen["depth_mean_strides"] == (60 * 80, 80, 1)   # the crop of the padded map, no copy
    # the lists extract_feat returns (mvsdet.py:698): one 0-dim fp32 tensor per scene, on the features' device
    gaps, rmses = got[5], got[6]
    assert len(gaps) == len(rmses) == 1 and gaps[0].dim() == 0 and rmses[0].dtype == torch.float32
    assert torch.equal(got[1], plain[1])                          # the valid counts did not move
    for name, mine, theirs, n in (("weight_gap", gaps[0], plain[5][0], seen["n_gap_terms"]), ("src_rmse", rmses[0], plain[6][0], seen["n_rmse_terms"]),
                                  ("weight_gap against G20", gaps[0], c["g20"]["gap_all"], seen["n_gap_terms"])):
        dist, bound = abs(float(mine) - float(theirs)) / abs(float(theirs)), summation_bound(n)
        print(f"{name}: {float(mine)!r} reference {float(theirs)!r} relative distance {dist:.3e} bound {bound:.3e}")
        assert dist <= bound, (name, dist, bound)
