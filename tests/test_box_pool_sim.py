"""tools/box_pool_sim.py: the CPU restatement of the sweep geometry's two run policies, at the headline workload's cameras."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_pooled_policy_stages_no_less_and_stalls_less_at_the_headline_cameras():
    import bench
    import box_pool_sim as sim
    w = bench.WORKLOADS["scannet_40v_64d_120x160"]
    proj, depth, H, W = sim.scene_cameras(w["N"], (w["H"], w["W"]), 1000, w["per_view_K"], w["near_far"], w["D"])
    assert proj.shape == (w["N"], 2, 4, 4) and depth.shape == (w["N"], w["D"]) and (H, W) == (w["H"], w["W"])
    boxes = sim.footprint_boxes(proj, depth, H, W)
    b = boxes.reshape(-1, *boxes.shape[2:])
    slot, pooled = sim.run_policy(b, 312, False), sim.run_policy(b, 312, True)
    assert (pooled["staged"] | ~slot["staged"]).all()          # every footprint the slot policy stages stays staged
    assert pooled["staged"].sum() >= slot["staged"].sum()
    assert (sim._area(slot["boxes"])[slot["staged"]] <= 312).all()
    area = sim._area(pooled["boxes"])
    assert (area[pooled["staged"]] <= 632).all() and (area[pooled["staged"]] > 312).any()
    # a wide box only where the other neighbour has no footprint
    wide = pooled["staged"] & (area > 312)
    assert not (wide & pooled["live"][:, ::-1]).any()
    ev_slot, ev_pool = slot["refill"].any(1).sum(), pooled["refill"].any(1).sum()
    assert ev_pool < ev_slot
    s = sim.simulate(proj, depth, H, W)
    assert np.isclose(s["slot"]["events_per_block"], ev_slot / b.shape[0]) and np.isclose(s["pooled"]["events_per_block"], ev_pool / b.shape[0])
