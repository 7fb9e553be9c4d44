"""Do two builds of the library compute the same per-pixel sweep and group-wise correlation?  One fresh child process per library
(MVSDET_HIP_LIB selects it: mvsdet_amd/_lib.py); the parent process never touches the GPU.

    python tools/pixel_form_ab.py --before build_ab/libparent.so [--after mvsdet_amd/libmvsdet_hip.so]

Forward (no atomics, no contraction: any difference is a bug): a SHA-256 of the output bytes of ops.plane_sweep_variance_pixel,
ops.homo_warp_pixel and ops.sweep.plane_sweep_groupcorr on seeded inputs -- tools/sweep_pixel_timing.py's shape (40 views, K = 2,
C = 256, D = 12, 60x80; smooth and rough depths, plane depths for the correlation, G = 8 and 32) and four small shapes with
K = 1, 2, 3, 4 (tests/test_gpu_groupcorr.py's B, A, D, F with their group counts).  The digests of the two libraries must be equal.

Backward (float atomics: the last bits vary from run to run): at the timing shape, max |after - before| beside
max |before - before, second run| for the three backward operators.  Exit status 1 if a digest differs."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {"K1": ((2, 1, 48, 2, 8, 32), (3,), [[1], [1]]),
         "K2": ((3, 2, 40, 5, 9, 21), (10, 5), [[0, 1], [2, 2], [1, 0]]),
         "K3": ((4, 3, 64, 2, 6, 10), (1,), [[1, 2, 3], [0, 0, 2], [2, 3, 1], [0, 1, 2]]),
         "K4": ((5, 4, 32, 2, 6, 10), (8, 4, 2, 1), [[1, 2, 3, 4], [0, 0, 2, 2], [2, 3, 4, 0], [4, 1, 1, 0], [3, 2, 1, 0]])}


def child(out_path: str) -> None:
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from mvsdet_amd import ops, synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    from pixel_scenes import scene
    dev = torch.device("cuda:0")
    digests, grads = {}, {}

    def digest(name, t):
        digests[name] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:32]

    def operators(tag, feat, nbr, proj, planes, depths, groups):
        for dn, depth in depths.items():
            digest(f"{tag} variance_pixel {dn}", ops.plane_sweep_variance_pixel(feat, nbr, proj, depth))
            digest(f"{tag} homo_warp_pixel {dn}", ops.homo_warp_pixel(feat[nbr[:, 0]], proj[:, 0].contiguous(), depth))
        for G in groups:
            for dn, depth in {"plane": planes, **depths}.items():
                digest(f"{tag} groupcorr G={G} {dn}", ops.sweep.plane_sweep_groupcorr(feat, nbr, proj, depth, G))

    # the timing shape: tools/sweep_pixel_timing.py's scene and depth maps
    N, K, C, D, (H, W) = 40, 2, 256, 12, (60, 80)
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D, topk=3)
    geo = hp.prepare_scene(synthetic.make_img_meta(N, (H, W), seed=5), dev)
    nbr, proj, planes = geo.neighbor_ids, geo.proj_rel, geo.depth_values.contiguous()
    feat = synthetic.make_features(N, C, (H, W), seed=5).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    interval = 4.8 / D
    ys, xs = torch.meshgrid(torch.arange(H, device=dev) / H, torch.arange(W, device=dev) / W, indexing="ij")
    low = torch.sin(6.2832 * xs) * torch.cos(6.2832 * ys)
    depths = {"smooth": (planes[:, :, None, None] + 0.35 * interval * low
                         + 0.05 * interval * (2 * torch.rand(N, D, H, W, device=dev, generator=g) - 1)).clamp_min(0.2).contiguous(),
              "rough": 0.2 + 4.8 * torch.rand(N, D, H, W, device=dev, generator=g)}
    operators("timing", feat, nbr, proj, planes, depths, (8, 32))
    R = torch.rand(N, C, D, H, W, device=dev, generator=g)
    grads["variance_pixel_backward rough"] = ops.plane_sweep_variance_pixel_backward(feat, nbr, proj, depths["rough"], R).cpu()
    grads["homo_warp_pixel_backward rough"] = ops.homo_warp_pixel_backward(proj[:, 0].contiguous(), depths["rough"], R).cpu()
    del R
    for G in (8, 32):
        R = torch.rand(N, K, G, D, H, W, device=dev, generator=g)
        grads[f"groupcorr_backward G={G} rough"] = ops.sweep.plane_sweep_groupcorr_backward(feat, nbr, proj, depths["rough"], R, G).cpu()
    for tag, (shape, groups, table) in SMALL.items():
        N, K, C, D, H, W = shape
        feat, nbr, proj, planes = (t.to(dev) for t in scene(shape, table))
        rough = (2.3 + 1.7 * (2 * torch.rand(N, D, H, W, device=dev, generator=g) - 1)).contiguous()
        operators(tag, feat, nbr, proj, planes, {"rough": rough}, groups)
    torch.save({"digests": digests, "grads": grads}, out_path)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--before", help="library to compare against")
    ap.add_argument("--after", default=os.path.join(ROOT, "mvsdet_amd", "libmvsdet_hip.so"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    import torch
    runs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, lib in (("before", a.before), ("before, second run", a.before), ("after", a.after)):
            path = os.path.join(tmp, "run.pt")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, timeout=600,
                           env={**os.environ, "MVSDET_HIP_LIB": os.path.abspath(lib)})
            runs[tag] = torch.load(path)
    before, again, after = (runs[t] for t in ("before", "before, second run", "after"))
    bad = 0
    print("# forward: SHA-256 (first 32 hex digits) of the output bytes | before | before, second run | after | verdict")
    for name in before["digests"]:
        d = [r["digests"][name] for r in (before, again, after)]
        same = d[0] == d[1] == d[2]
        bad += not same
        print(f"{name} | {d[0]} | {d[1]} | {d[2]} | {'same' if same else 'DIFFERENT'}")
    print("# backward at the timing shape: max |after - before| | max |before - before, second run| | max |before|")
    for name, gb in before["grads"].items():
        print(f"{name} | {float((after['grads'][name] - gb).abs().max()):.3e} | {float((again['grads'][name] - gb).abs().max()):.3e} | "
              f"{float(gb.abs().max()):.3e}")
    print(f"# {len(before['digests'])} digests, {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
