"""One planted positive point through ops.head_loss / ops.head_loss_rotated, shared by the suites that plant box pairs
(tests/test_gpu_head_loss_arkit.py, tests/test_gpu_head_loss_edges.py)."""
import torch


def plant(gpu, geom, i, d, target, weight):
    """A one-level 2x2x2 grid with the geometry `geom` (1, 1, 6) whose point i is the only positive one, with the predicted channels
    d (6: ops.head_loss, 7: ops.head_loss_rotated) against the target row `target` and the centerness target `weight`: (the
    scene's sums, the gradient of the box loss sum by the bbox map as (channels, 8), on the host)."""
    from mvsdet_amd import ops
    n = int(d.numel())
    bbox = torch.ones(1, n, 2, 2, 2)
    bbox.view(n, 8)[:, i] = d
    bbox = bbox.to(gpu).requires_grad_(True)
    center = torch.zeros(1, 1, 2, 2, 2, device=gpu, requires_grad=True)
    cls = torch.zeros(1, 1, 2, 2, 2, device=gpu, requires_grad=True)
    labels = torch.full((1, 8), -1, dtype=torch.int64)
    labels[0, i] = 0
    center_t = torch.full((1, 8), -1.0 if n == 7 else 0.0)       # what each route's assignment gives a point without a box
    center_t[0, i] = weight
    bbox_t = torch.zeros(1, 8, n)
    bbox_t[0, i] = torch.as_tensor(target).float()
    targets = ops.HeadTargets(labels.to(gpu), labels.to(gpu).int(), center_t.to(gpu), bbox_t.to(gpu), geom.to(gpu))
    fn = ops.head_loss_rotated if n == 7 else ops.head_loss
    sums = fn([center], [bbox], [cls], torch.ones(1, 1, 2, 2, 2, device=gpu), targets)
    assert int(sums.n_pos[0]) == 1 and int(sums.n_valid[0]) == 8
    sums.bbox.sum().backward()
    g = bbox.grad.view(n, 8).cpu()
    assert not bool(g[:, [j for j in range(8) if j != i]].any())
    return sums, g
