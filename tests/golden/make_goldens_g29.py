#!/usr/bin/env python3
"""Generate tests/golden/g29_gshead.npz (build container only: needs the reference tree).

G29: the first part of the novel-view branch of extract_feat (mvsdet.py:561-575): the rows of the chosen source views through
`to_gaussians`, in float32 torch on the CPU, with the gradients of a seeded linear loss.

The reference's OWN code here: MVSDet.process_rgb_raw (mvsdet.py:319-333), called unbound on the module loaded by _ref_loader
(metadata `process_rgb_raw` = "reference ..."; "restated" if that import route fails and its six lines are spelled out here instead).
Its `.view` refuses a cropped width, so it is called for the uncropped width and the columns are cut here.
RESTATED here (flagged in the metadata as `restated_lines`): the concatenation lines :561-569, which are inline in extract_feat, and
the constructor's nn.Sequential(nn.ReLU(), nn.Linear(...)) of :210-216 with the case's weight and bias loaded into it.

Cases (tests/gshead_restated.py::case): N = 3 views of C = 16 channels, 6 x 9 maps cropped to 5 x 7, ids [0, 2], images 24 x 36,
S in {1, 2} x d_sh in {4, 25} x {without rgb, with rgb from the images}.  The inputs are shared by the cases (stored once, `in_*`);
per case: weight, bias, the reference's rgb rows, raw, the four gradients of sum(raw * loss_weight(seed)), and `own_<name>`: the largest
distance of each from the float64 restatement (tests/gshead_restated.py) -- printed here; the tests' bars are 4 x these or the
project's bar, whichever is larger.

    python tests/golden/make_goldens_g29.py
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gshead_restated as G  # noqa: E402
from _ref_loader import load_reference  # noqa: E402

SEED = 2900
N, IDS, C, HF, WF, H, W = 3, [0, 2], 16, 6, 9, 5, 7


def reference_rgb_rows():
    try:
        mvsdet, _ = load_reference()
        fn = mvsdet.MVSDet.process_rgb_raw

        def own(images, ids):
            # its `.view` refuses a cropped WIDTH (the shipped shapes crop 60 x 80 to 59 x 80: rows only), so it is asked for the
            # uncropped width and the columns are cut here
            full = fn(None, images, 4, H, WF, ids)
            assert tuple(full.shape) == (1, len(ids), H * WF, 3)
            return full.reshape(1, len(ids), H, WF, 3)[:, :, :, :W].reshape(1, len(ids), H * W, 3)
        return own, "reference (resize and row crop; the column crop is restated: its .view refuses a cropped width)"
    except Exception as e:       # the import route failed: its six lines, restated
        print("process_rgb_raw could not be imported from the reference:", repr(e))

        def restated(images, ids):
            new_rgb = torch.nn.functional.interpolate(images[ids], scale_factor=1. / 4, mode='bilinear')[:, :, :H, :W]
            return new_rgb.view(*new_rgb.shape[:2], -1).transpose(2, 1).unsqueeze(0)
        return restated, "restated"


def main():
    rgb_rows, how = reference_rgb_rows()
    shared = G.case(SEED, N, IDS, C, HF, WF, H, W, 1, 4, rgb="images")
    out = {"restated_lines": np.array("mvsdet.py:561-569 (concatenation) and :210-216 (nn.Sequential(ReLU, Linear))"),
           "process_rgb_raw": np.array(how), "shape": np.array([N, C, HF, WF, H, W], np.int32), "ids": shared["ids"],
           "in_feature": shared["feature"], "in_depth_coding": shared["depth_coding"], "in_images": shared["images"]}
    tags = []
    for S in (1, 2):
        for d_sh in (4, 25):
            for rgb in (False, True):
                tag = f"s{S}_sh{d_sh}_{'rgb' if rgb else 'plain'}"
                tags.append(tag)
                seed = SEED + len(tags)
                c = G.case(seed, N, IDS, C, HF, WF, H, W, S, d_sh, rgb="images" if rgb else None)
                for k in ("feature", "depth_coding") + (("images",) if rgb else ()):
                    c[k] = shared[k]
                ids = torch.from_numpy(c["ids"])
                feature, depth_coding = (torch.from_numpy(c[k]).requires_grad_(True) for k in ("feature", "depth_coding"))
                # --- restated: mvsdet.py:210-216
                to_gaussians = nn.Sequential(nn.ReLU(), nn.Linear(c["K"], c["M"]))
                with torch.no_grad():
                    to_gaussians[1].weight.copy_(torch.from_numpy(c["weight"]))
                    to_gaussians[1].bias.copy_(torch.from_numpy(c["bias"]))
                # --- restated: mvsdet.py:561-569
                height, width, chosen_src = H, W, len(IDS)
                gs_feature = feature[ids, :, :height, :width].view(chosen_src, feature.shape[1], -1).transpose(1, 2).unsqueeze(0)
                dc = depth_coding.view(*depth_coding.shape[:2], -1).unsqueeze(0).transpose(3, 2)
                gs_feature = torch.cat([gs_feature, dc[:, ids]], dim=-1)
                if rgb:
                    rgb_raw = rgb_rows(torch.from_numpy(c["images"]), ids)                  # the reference's own function
                    assert tuple(rgb_raw.shape) == (1, len(IDS), H * W, 3)
                    gs_feature = torch.cat([gs_feature, rgb_raw], dim=-1)
                    out[f"{tag}.rgb_rows"] = rgb_raw[0].numpy().astype(np.float32)
                raw = to_gaussians(gs_feature)[0].reshape(len(IDS), H * W, S, -1)
                lw = torch.from_numpy(G.loss_weight(seed, tuple(raw.shape)))
                grads = torch.autograd.grad((raw * lw).sum(), [feature, depth_coding, to_gaussians[1].weight, to_gaussians[1].bias])
                got = dict(raw=raw.detach().numpy(), **{"g_" + k: g.numpy() for k, g in zip(G.GRADS, grads)})
                o64, g64 = G.restate(c, torch.float64)
                want = dict(raw=o64, **{"g_" + k: g64[k] for k in G.GRADS})
                for name, val in got.items():
                    own = float(np.abs(val.astype(np.float64) - want[name]).max())
                    print(f"{tag}: {name} reference fp32 - float64 restatement {own:.3g} (largest entry {np.abs(want[name]).max():.3g})")
                    out[f"{tag}.own_{name}"] = np.float64(own)
                    out[f"{tag}.{name}"] = val.astype(np.float32)
                if rgb:
                    r64 = G.process_rgb_raw(torch.from_numpy(c["images"]).double(), ids, H, W).numpy()
                    out[f"{tag}.own_rgb_rows"] = np.float64(np.abs(out[f"{tag}.rgb_rows"].astype(np.float64) - r64).max())
                out[f"{tag}.weight"], out[f"{tag}.bias"] = c["weight"], c["bias"]
                out[f"{tag}.meta"] = np.array([S, d_sh, int(rgb), seed], np.int32)
    out["cases"] = np.array(tags)
    path = os.path.join(HERE, "g29_gshead.npz")
    np.savez_compressed(path, **out)
    print("process_rgb_raw:", how)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
