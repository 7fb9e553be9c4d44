"""Cache policies of the plane sweep (options "sweep_store" and "sweep_box_load", csrc/sweep_kernel.h): the flavour of the output
stores and of the once-read loads of the slab kernel's FAST form with two neighbours.  A cache policy changes no value, so every
comparison here is torch.equal against the same call under sweep_store 0 (non-temporal stores, default loads) and
assert_array_equal against the device-rounding CPU oracle.

The flavours are instantiations: the default build carries what profiles/r10_sweep_store_policy_ab.txt kept, the A/B build
(make SWEEP_STORE_MATRIX=1, picked through MVSDET_HIP_LIB) all of them.  The tests ask the library which values it takes --
set_option refuses the others -- and run every pair it has."""
import numpy as np
import pytest
import torch

from test_gpu_sweep_inside import MAP_OF_TW, N, K, D, _feat, _options, _scaled, _scene, _shift

pytestmark = pytest.mark.gpu

STORE_VALUES = range(-1, 8)     # -1 what ships for the class (the default), 0 nt, 1 plain, 2 sc1, 3 sc0 sc1, 4 nt sc1, 5 nt through the buffer
                                # store; 6, 7: no such flavour
LOAD_VALUES = range(0, 4)       # 0 default, 1 nt; 2, 3: no such flavour


def _accepted(name, values):
    """the values of an option that this build takes; the option is left as it was"""
    from mvsdet_amd import _lib
    saved = _lib.get_option(name)
    ok = []
    try:
        for v in values:
            try:
                _lib.set_option(name, v)
                ok.append(v)
            except ValueError:
                pass
    finally:
        _lib.set_option(name, saved)
    return ok


@pytest.fixture(scope="module")
def flavours(gpu):
    """every compiled (sweep_store, sweep_box_load) pair but the non-temporal store with default loads, which is what they are compared with"""
    stores, loads = _accepted("sweep_store", STORE_VALUES), _accepted("sweep_box_load", LOAD_VALUES)
    assert 0 in stores and -1 in stores and 0 in loads
    pairs = [(s, l) for s in stores for l in loads if (s, l) != (0, 0)]
    print(f"sweep_store {stores} x sweep_box_load {loads}")
    return pairs


def _same_everywhere(run, flavours, ref=None, **opts):
    """run() under the defaults and under every flavour: the same bits (NaNs where they were), and the oracle's if `ref` is given"""
    with _options(**opts):
        with _options(sweep_store=0, sweep_box_load=0):
            base = run()
        if ref is not None:
            np.testing.assert_array_equal(base.float().cpu().numpy(), ref)
        for s, l in flavours:
            with _options(sweep_store=s, sweep_box_load=l):
                out = run()
            assert torch.equal(torch.isnan(out), torch.isnan(base)), (s, l)
            assert torch.equal(torch.nan_to_num(out, nan=0.0), torch.nan_to_num(base, nan=0.0)), (s, l)
            if ref is not None:
                np.testing.assert_array_equal(out.float().cpu().numpy(), ref)
    return base


def _dev(gpu, feat, nbr, proj, depth):
    return feat.to(gpu), torch.tensor(nbr).to(gpu), torch.tensor(proj).to(gpu), torch.tensor(depth).to(gpu)


def _oracle(oracle, feat, nbr, proj, depth):
    return oracle.plane_sweep_variance(feat, nbr, torch.tensor(proj), torch.tensor(depth), mode=1)


@pytest.mark.parametrize("tw", [32, 16])
@pytest.mark.parametrize("C", [32, 64])
def test_every_flavour_keeps_the_bits(gpu, oracle, flavours, tw, C):
    """the fused call; C = 64: two slabs, the second one's resource starts 32 channel rows into a view"""
    from mvsdet_amd import ops
    proj, depth, nbr = _scene()
    feat = _feat(N, C, *MAP_OF_TW[tw])
    f, nb, pr, de = _dev(gpu, feat, nbr, proj, depth)
    _same_everywhere(lambda: ops.plane_sweep_variance(f, nb, pr, de), flavours, _oracle(oracle, feat, nbr, proj, depth), sweep_tw=tw)


@pytest.mark.parametrize("C", [32, 64])
def test_tabled_on_the_pooled_table(gpu, oracle, flavours, C):
    from mvsdet_amd import ops
    proj, depth, nbr = _scene()
    H, W = MAP_OF_TW[32]
    feat = _feat(N, C, H, W)
    f, nb, pr, de = _dev(gpu, feat, nbr, proj, depth)
    with _options(sweep_tw=32):
        packed, table = ops.pack_features(f), ops.plane_sweep_table_pooled(pr, de, H, W)
    assert int(table.view(torch.int32)[0].item()) == 0x4d565350      # the pooled mark
    _same_everywhere(lambda: ops.plane_sweep_variance_tabled(packed, nb, table, C, D, H, W), flavours,
                     _oracle(oracle, feat, nbr, proj, depth), sweep_tw=32)


def test_pitched_route(gpu, oracle, flavours):
    """W = 48: a multiple of 16 and not of 32; rows pitched to 64 take the 32x4 tiles, whose second column is half empty"""
    from mvsdet_amd import ops
    proj, depth, nbr = _scene()
    H, W, C = 8, 48, 32
    pitch = ops.sweep_row_pitch(W)
    assert pitch % 32 == 0 and pitch > W
    feat = _feat(N, C, H, W)
    f, nb, pr, de = _dev(gpu, feat, nbr, proj, depth)
    packed, table = ops.pack_features(f), ops.plane_sweep_table_pooled(pr, de, H, W, pitch)
    assert int(table.view(torch.int32)[1].item()) & 0xff == 32
    _same_everywhere(lambda: ops.plane_sweep_variance_tabled_pitched(packed, nb, table, C, D, H, W, pitch).contiguous(), flavours,
                     _oracle(oracle, feat, nbr, proj, depth))


@pytest.mark.parametrize("tw", [32, 16])
def test_fp16_storage(gpu, flavours, tw):
    from mvsdet_amd import ops
    proj, depth, nbr = _scene()
    (H, W), C = MAP_OF_TW[tw], 64
    f, nb, pr, de = _dev(gpu, _feat(N, C, H, W), nbr, proj, depth)
    packed = ops.pack_features(f)
    args = (packed, nb, pr, de, N, 0, C, H, W)
    half = _same_everywhere(lambda: ops.plane_sweep_variance_shard(*args, half_out=True), flavours, sweep_tw=tw)
    with _options(sweep_tw=tw, sweep_store=0, sweep_box_load=0):
        assert torch.equal(half, ops.plane_sweep_variance_shard(*args).half())


@pytest.mark.parametrize("C,hw", [(40, (8, 64)), (32, (8, 42)), (40, (8, 40))])
def test_the_general_form_is_untouched(gpu, oracle, flavours, C, hw):
    """C = 40 (a partial slab) or W % 4 != 0: not the FAST form, which has no flavours -- the options select nothing there"""
    from mvsdet_amd import ops
    proj, depth, nbr = _scene()
    feat = _feat(N, C, *hw)
    f, nb, pr, de = _dev(gpu, feat, nbr, proj, depth)
    _same_everywhere(lambda: ops.plane_sweep_variance(f, nb, pr, de), flavours, _oracle(oracle, feat, nbr, proj, depth), sweep_tw=32)


def test_refilled_boxes(gpu, oracle, flavours):
    """test_lean_form_under_small_boxes' scene: boxes of 40 texels break into short runs on the near planes, so the load policy is
    on boxes that are refilled in the middle of a block's sweep, beside gathered footprints"""
    from mvsdet_amd import ops
    _, depth, nbr = _scene()
    proj = np.stack([np.stack([_scaled(0.25, 3.0, 2.0), _scaled(0.25, 2.0, 1.5)]),
                     np.stack([_scaled(0.25, 2.5, 1.0), _shift(1.5, 0.9)]),
                     np.stack([_scaled(0.25, -1.5, -1.0), _scaled(0.25, 1.0, 2.5)])]).astype(np.float32)
    H, W = 16, 32
    feat = _feat(N, 32, H, W)
    f, nb, pr, de = _dev(gpu, feat, nbr, proj, depth)
    with _options(sweep_tw=16, sweep_boxcap=40):
        flags = ops.sweep_flags(ops.plane_sweep_table(pr, de, H, W), N, K, D, H, W).cpu()
    nib = torch.stack([(flags >> (4 * j)) & 0xf for j in range(K)])
    assert ((nib[..., 1:] & 6) == 6).any()                  # staged and refilled past the first plane
    assert ((nib & 3) == 1).any()                           # and a gathered footprint
    _same_everywhere(lambda: ops.plane_sweep_variance(f, nb, pr, de), flavours, _oracle(oracle, feat, nbr, proj, depth),
                     sweep_tw=16, sweep_boxcap=40)


@pytest.mark.parametrize("tw", [32, 16])
def test_nan_and_out_of_view(gpu, oracle, flavours, tw):
    """test_out_of_view_nan_and_sign_change_beside_flagged's scene: the NaNs sit where the oracle has them"""
    from mvsdet_amd import ops
    proj, depth, nbr = _scene()
    proj[0, 1] = _shift(4000.0, 0.0)
    proj[1, 1, 0, 0] = np.nan
    proj[2, 1, 2, 0], proj[2, 1, 2, 2] = 1.0, -5.5
    feat = _feat(N, 32, *MAP_OF_TW[tw])
    f, nb, pr, de = _dev(gpu, feat, nbr, proj, depth)
    ref = _oracle(oracle, feat, nbr, proj, depth)
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    _same_everywhere(lambda: ops.plane_sweep_variance(f, nb, pr, de), flavours, ref, sweep_tw=tw)


def test_wrong_header_still_gives_nan(gpu, flavours):
    """a table of the other tile shape: the block-uniform exit fills the whole output with NaN under every flavour"""
    from mvsdet_amd import ops
    proj, depth, nbr = _scene()
    (H, W), C = MAP_OF_TW[32], 32
    f, nb, pr, de = _dev(gpu, _feat(N, C, H, W), nbr, proj, depth)
    packed = ops.pack_features(f)
    with _options(sweep_tw=16):
        table = ops.plane_sweep_table(pr, de, H, W)
    for s, l in [(0, 0)] + flavours:
        with _options(sweep_tw=32, sweep_store=s, sweep_box_load=l):
            out = ops.plane_sweep_variance_tabled(packed, nb, table, C, D, H, W)
        assert bool(torch.isnan(out).all()), (s, l)


def test_options_are_restored_and_unknown_values_refused(gpu):
    from mvsdet_amd import _lib
    for name, values in (("sweep_store", STORE_VALUES), ("sweep_box_load", LOAD_VALUES)):
        before = _lib.get_option(name)
        ok = _accepted(name, values)
        assert _lib.get_option(name) == before
        assert 0 in ok and max(values) not in ok and (-1 in _accepted(name, [-1])) == (name == "sweep_store")
        for v in list(values) + [-2, 99]:
            if v in ok:
                continue
            with pytest.raises(ValueError, match="not compiled"):
                _lib.set_option(name, v)
            assert _lib.get_option(name) == before      # a refused value is not mapped to another one
