"""Which route a layer call of the cost network, the neck and the head takes -- this library's eval kernels, its autograd kernels, or
the framework's own layers -- and the counters that record it (`layers.route_stats`, `layers.framework_calls`).

The truth tables below were read off the predicates of commit d0bb553 (the commit before the decisions moved into `layers`), cited
block by block as file:line of that commit; they are literals, never computed through the helpers under test.  A code per row:
E = eval kernels, G = autograd / training kernels, and for the framework the reason: t = "tensor", m = "mode", o = "option", s = "shape".
The reason is the one `layers.decide` documents: "tensor" first; "option" where the kernels for the call exist and an option chose
the framework; "mode" where the site has none for the call; "shape" last.
"""
import copy
import itertools
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from mvsdet_amd import layers
from mvsdet_amd import costreg as CR
from mvsdet_amd import neck as NK
from mvsdet_amd.costreg import CostRegNet3DGS
from mvsdet_amd.head import NerfDetHeadConvs
from mvsdet_amd.neck import IndoorImVoxelNeck

CODE = {"eval": "E", "grad": "G", "tensor": "t", "mode": "m", "option": "o", "shape": "s"}
DEVICES, DTYPES, ON_OFF = ("cpu", "cuda"), (torch.float32, torch.float16), (True, False)


def _stand_in(device, dtype):
    """What the call's facts read of a tensor: nothing here needs a GPU."""
    return SimpleNamespace(is_cuda=device == "cuda", dtype=dtype, shape=(1, 64, 8, 8, 8))


def _check(table, rest_axes, decide):
    """table: {(autograd, training): codes over the product of rest_axes} for a CUDA float32 tensor; every other tensor (CPU, or
    float16 on either device) goes to the framework for the reason "tensor" in every row, where the site has reasons at all
    (a table of "-" codes is a plain yes / no)."""
    plain = set("".join(table.values())) <= set("CGK-")
    for device, dtype, grad, training in itertools.product(DEVICES, DTYPES, ON_OFF, ON_OFF):
        want = table[grad, training] if (device, dtype) == ("cuda", torch.float32) else ("-" if plain else "t") * len(table[grad, training])
        with torch.set_grad_enabled(grad):
            got = "".join(decide(_stand_in(device, dtype), training, *rest) for rest in itertools.product(*rest_axes))
        assert got == want, (device, dtype, "autograd" if grad else "no_grad", "train" if training else "eval", got, want)


@pytest.fixture(scope="module")
def nets():
    return {64: CostRegNet3DGS(64, 64), 32: CostRegNet3DGS(64, 32)}


# ------------------------------------------------------------------------------------------------------------ the cost network
def test_truth_table_cost_network_layers(nets):
    """`_cbr` (costreg.py:241-242 eval, 258-259 autograd) and `_up` (costreg.py:285-286, 295-296): keyed on autograd, `training` only
    in eval form -- .train() under no_grad has no kernel route ("mode"), .eval() under autograd runs the convolution on ours."""
    net = nets[64]
    convs = {(c, s): nn.Conv3d(c, c, 3, stride=s, padding=1, bias=False) for c in (64, 32) for s in (1, 2, 3)}
    deconvs = {c: nn.ConvTranspose3d(c, c, 3, stride=2, padding=1, output_padding=1, bias=False) for c in (64, 32)}

    def cbr(x, training, channels, stride, hip_backward):
        net.train(training).hip_backward = hip_backward
        return CODE[net._route(layers.call_facts(x, net), convs[channels, stride])]

    def up(x, training, channels, hip_backward):
        net.train(training).hip_backward = hip_backward
        return CODE[net._route(layers.call_facts(x, net), deconvs[channels])]

    # (autograd, training): channels 64 | 32  x  stride 1 | 2 | 3 (no kernel)  x  hip_backward on | off
    _check({(True, True): "GoGo" "so" "sososo",
            (True, False): "GoGo" "so" "sososo",      # .eval() + autograd: the convolution on our kernels (its BatchNorm: below)
            (False, True): "mmmm" "mm" "mmmmmm",      # .train() + no_grad: the framework, whatever the layer
            (False, False): "EEEE" "ss" "ssssss"}, [(64, 32), (1, 2, 3), ON_OFF], cbr)
    # (autograd, training): channels 64 | 32  x  hip_backward on | off
    _check({(True, True): "Go" "so", (True, False): "Go" "so", (False, True): "mm" "mm", (False, False): "EE" "ss"},
           [(64, 32), ON_OFF], up)
    net.train(False).hip_backward = True
    # the eval kernels take any input channel count, the autograd kernels 64s only (costreg.py:259)
    mixed = nn.Conv3d(32, 64, 3, padding=1, bias=False)
    with torch.no_grad():
        assert net._route(layers.call_facts(_stand_in("cuda", torch.float32), net), mixed) == "eval"
    with torch.enable_grad():
        assert net._route(layers.call_facts(_stand_in("cuda", torch.float32), net), mixed) == "shape"


def test_truth_table_cost_network_head_chain_and_batchnorm(nets):
    """`_head` (costreg.py:313 eval, 315 autograd) never looks at `training` and has no channel rule; `_chain_ok` (costreg.py:126-129);
    `_bn_hip_ok` (costreg.py:36-37): a BatchNorm in eval mode beside an autograd convolution stays on the framework."""
    net = nets[64]

    def prob(x, training, hip_backward):
        net.train(training).hip_backward = hip_backward
        return CODE[net._route(layers.call_facts(x, net), net.prob)]

    # (autograd, training): hip_backward on | off
    _check({(True, True): "Go", (True, False): "Go", (False, True): "EE", (False, False): "EE"}, [ON_OFF], prob)
    net.train(False).hip_backward = True

    def chain(x, training, base, precision, forms):
        n = nets[base].train(training)
        n.matrix_precision, n.layer_forms = precision, forms
        try:
            return "C" if n._chain_ok(layers.call_facts(x, n)) else "-"
        finally:
            n.matrix_precision, n.layer_forms = "bf16x3", "scl"
            n.train(False)

    # (autograd, training): base 64 | 32  x  matrix_precision bf16x3 | fp32  x  layer_forms scl | f32
    _check({(True, True): "--------", (True, False): "--------", (False, True): "--------", (False, False): "C-------"},
           [(64, 32), ("bf16x3", "fp32"), ("scl", "f32")], chain)

    # device, dtype: bn.training on | off  x  bn.affine on | off -- autograd and the network's mode are not looked at
    want = {("cpu", torch.float32): "----", ("cpu", torch.float16): "----", ("cuda", torch.float32): "K---", ("cuda", torch.float16): "----"}
    for (device, dtype), codes in want.items():
        for grad, training in itertools.product(ON_OFF, ON_OFF):
            with torch.set_grad_enabled(grad):
                call = layers.call_facts(_stand_in(device, dtype), net.train(training))
                got = "".join("K" if CR._bn_hip_ok(nn.BatchNorm3d(4, affine=a).train(t), call) else "-"
                              for t, a in itertools.product(ON_OFF, ON_OFF))
            assert got == codes, (device, dtype, grad, training)
    net.train(False)


# ------------------------------------------------------------------------------------------------------------ neck and head
def test_truth_table_neck():
    """The blocks (neck.py:59-60 `_hip_ok` with the channel rule of neck.py:152, 199, 230): eval kernels only, keyed on the block's
    own `training`; a block in training mode is on the framework because `autograd_route` left it there ("option").  The training
    kernels (neck.py:265): `autograd_route` "hip", keyed on the neck's `training`, whatever autograd is."""
    blocks = {c: ((NK.ResModule(c, c), lambda b: b.conv0.conv), (NK._UpBlock(c, c), lambda b: b[3]), (NK._OutBlock(c, c), lambda b: b[0]))
              for c in (64, 32)}
    for kind in range(3):
        def block(x, training, channels):
            b, conv = blocks[channels][kind]
            return CODE[NK._block_route(x, b.train(training), conv(b))]

        # (autograd, training): channels 64 | 32
        _check({(True, True): "oo", (True, False): "mm", (False, True): "oo", (False, False): "Es"}, [(64, 32)], block)

    class TrainingKernels(Exception):
        pass

    def chosen(x):
        raise TrainingKernels

    neck = IndoorImVoxelNeck(8, 8, [1])
    neck._check_hip_train = chosen   # the first thing `forward` does once it has chosen the training kernels

    def training_kernels(x, training, route):
        neck.train(training).autograd_route = route
        try:
            neck(x)
        except TrainingKernels:
            return "G"
        except (TypeError, AttributeError):   # a framework layer met the stand-in: the blocks' own forward ran
            return "-"

    # (autograd, training): autograd_route aten | hip
    _check({(True, True): "-G", (True, False): "--", (False, True): "-G", (False, False): "--"}, [("aten", "hip")], training_kernels)


def test_truth_table_head():
    """`_hip_autograd` (head.py:100-101) and the eval branch of `_forward_single` (head.py:126): the autograd kernels are keyed on
    autograd, whatever `training` is (the neck's on `training`)."""
    head = NerfDetHeadConvs(4, 1, 64, 6)

    def level(x, training, route):
        head.train(training).autograd_route = route
        return CODE[head._route(x)]

    # (autograd, training): autograd_route aten | hip
    _check({(True, True): "oG", (True, False): "oG", (False, True): "mm", (False, False): "EE"}, [("aten", "hip")], level)


def test_counters_on_a_cpu_forward():
    """A CPU run takes the framework everywhere, quietly: one count per layer, reason "tensor"."""
    layers.reset_route_stats()
    with torch.no_grad():
        CostRegNet3DGS(64, 16).eval()(torch.zeros(1, 64, 4, 4, 4))
        assert layers.route_stats == {"hip": 0, "framework": 8}
        assert layers.framework_calls == {(f"CostRegNet3DGS.{n}", "tensor"): 1
                                          for n in ("conv0", "conv1", "conv2", "conv3", "conv4", "conv9", "conv11", "prob")}
        layers.reset_route_stats()
        assert layers.route_stats == {"hip": 0, "framework": 0} and layers.framework_calls == {}
        levels = IndoorImVoxelNeck(8, 8, [1]).eval()(torch.zeros(1, 8, 4, 4, 4))
        assert layers.route_stats == {"hip": 0, "framework": 3}
        assert layers.framework_calls == {("ResModule.conv0", "tensor"): 1, ("ResModule.conv1", "tensor"): 1, ("_OutBlock.0", "tensor"): 1}
        layers.reset_route_stats()
        NerfDetHeadConvs(4, 1, 8, 6).eval()(levels)
        assert layers.route_stats == {"hip": 0, "framework": 3}
        assert layers.framework_calls == {(f"NerfDetHeadConvs.{n}", "tensor"): 1 for n in ("conv_center", "conv_reg", "conv_cls")}
    layers.reset_route_stats()
    assert layers.route_stats == {"hip": 0, "framework": 0} and layers.framework_calls == {}


# ------------------------------------------------------------------------------------------------------------ on the GPU
def _counted(run):
    """run() twice, the counters reset in between: the second call's output, which must equal the first's bit for bit (counting does
    not perturb values), with the counters of that one call left behind."""
    first = run()
    layers.reset_route_stats()
    second = run()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    return second


def _reasons():
    return {reason for _, reason in layers.framework_calls}


COSTREG_LAYERS = ("conv0", "conv1", "conv2", "conv3", "conv4", "conv9", "conv11")


@pytest.mark.gpu
def test_cost_network_routes_on_the_gpu(gpu):
    torch.manual_seed(0)
    x = torch.rand(1, 64, 8, 8, 8, device=gpu)
    net = CostRegNet3DGS(in_channels=64, base=64).to(gpu).eval()
    with torch.no_grad():
        _counted(lambda: [net(x)])
        assert layers.route_stats == {"hip": 8, "framework": 0} and layers.framework_calls == {}
        # channel counts outside the kernels' multiples of 64.  The layers decide one by one, as before: with base=32 only conv0 and
        # conv11 (32 output channels) leave our kernels; with base=8 all seven layers with a BatchNorm do.  The head convolution has no
        # channel rule (costreg.py:313 of d0bb553) and stays on ours.
        narrow = CostRegNet3DGS(in_channels=64, base=32).to(gpu).eval()
        _counted(lambda: [narrow(x)])
        assert layers.route_stats == {"hip": 6, "framework": 2}
        assert layers.framework_calls == {("CostRegNet3DGS.conv0", "shape"): 1, ("CostRegNet3DGS.conv11", "shape"): 1}
        narrowest = CostRegNet3DGS(in_channels=64, base=8).to(gpu).eval()
        _counted(lambda: [narrowest(x)])
        assert layers.route_stats == {"hip": 1, "framework": 7}
        assert layers.framework_calls == {(f"CostRegNet3DGS.{n}", "shape"): 1 for n in COSTREG_LAYERS}
        # .train() under no_grad: no kernel route for a layer with a BatchNorm; the head convolution does not look at the mode
        net.train()
        twin = copy.deepcopy(net)   # (a training-mode call moves the running statistics: each call on a module of its own)
        first = twin(x)
        layers.reset_route_stats()
        assert torch.equal(first, net(x))
        assert layers.route_stats == {"hip": 1, "framework": 7}
        assert layers.framework_calls == {(f"CostRegNet3DGS.{n}", "mode"): 1 for n in COSTREG_LAYERS}
    # one training step: every layer (convolution with its BatchNorm; the head) on our kernels
    twin = copy.deepcopy(net)
    first = twin(x)
    layers.reset_route_stats()
    out = net(x)
    out.square().mean().backward()
    assert torch.equal(first.detach(), out.detach())
    assert layers.route_stats == {"hip": 8, "framework": 0} and layers.framework_calls == {}
    # .eval() with autograd on: the convolutions on our kernels, the seven BatchNorms (running statistics) on the framework
    net.eval()
    _counted(lambda: [net(x).detach()])
    assert layers.route_stats == {"hip": 8, "framework": 7}
    assert layers.framework_calls == {(f"CostRegNet3DGS.{n}.{'1' if n in ('conv9', 'conv11') else 'bn'}", "mode"): 1 for n in COSTREG_LAYERS}


@pytest.mark.gpu
def test_neck_routes_on_the_gpu(gpu):
    torch.manual_seed(1)
    x = torch.randn(1, 64, 8, 8, 8, device=gpu)
    neck = IndoorImVoxelNeck(64, 64, [1, 1]).to(gpu).eval()
    assert neck.autograd_route == "aten"
    with torch.no_grad():
        _counted(lambda: neck(x))
        # two ResModules (2 + 3 layers), the up block (2), two out blocks
        assert layers.route_stats == {"hip": 9, "framework": 0} and layers.framework_calls == {}
        # in_channels=32: the blocks whose 3x3x3 layers have 32 output channels, and the 32 -> 64 shortcut (64 rows: `ops.gemm_layer_ok`)
        narrow = IndoorImVoxelNeck(32, 64, [1, 1]).to(gpu).eval()
        _counted(lambda: narrow(x[:, :32].contiguous()))
        assert layers.framework_calls == {("ResModule.conv0", "shape"): 1, ("ResModule.conv1", "shape"): 1, ("ResModule.downsample", "shape"): 1,
                                          ("_UpBlock.0", "shape"): 1, ("_UpBlock.3", "shape"): 1}
        assert layers.route_stats == {"hip": 4, "framework": 5}
    # .train() with the default route: every layer on the framework, by choice
    neck.train()
    twin = copy.deepcopy(neck)
    first = twin(x)
    layers.reset_route_stats()
    for a, b in zip(first, neck(x)):
        assert torch.equal(a, b)
    assert layers.route_stats == {"hip": 0, "framework": 9} and _reasons() == {"option"}
    # autograd_route "hip" in .train().  This module's 64 -> 128 shortcut is a shape the training kernels refuse
    # (`_check_hip_train`: `ops.gemm_layer_ok(64, 128)`): the call raises before any layer runs instead of falling back ...
    neck.autograd_route = "hip"
    layers.reset_route_stats()
    with pytest.raises(ValueError, match="shortcut"):
        neck(x)
    assert layers.route_stats == {"hip": 0, "framework": 0}
    # ... so the route itself runs at the smallest channel count it takes, 128
    wide = IndoorImVoxelNeck(128, 64, [1, 1]).to(gpu).train()
    wide.autograd_route = "hip"
    x2 = torch.randn(1, 128, 8, 8, 8, device=gpu)
    twin = copy.deepcopy(wide)
    first = twin(x2)
    layers.reset_route_stats()
    for a, b in zip(first, wide(x2)):
        assert torch.equal(a, b)
    assert layers.route_stats == {"hip": 9, "framework": 0} and layers.framework_calls == {}


@pytest.mark.gpu
def test_head_routes_on_the_gpu(gpu):
    torch.manual_seed(2)
    x = [torch.randn(1, 64, 8, 8, 8, device=gpu)]
    head = NerfDetHeadConvs(n_channels=64, n_levels=1).to(gpu).eval()
    assert head.autograd_route == "aten"

    def run():
        return [t.detach() for part in head(x) for t in part]

    with torch.no_grad():
        _counted(run)
        assert layers.route_stats == {"hip": 1, "framework": 0} and layers.framework_calls == {}
    _counted(run)   # autograd on, the default route
    assert layers.route_stats == {"hip": 0, "framework": 3}
    assert layers.framework_calls == {(f"NerfDetHeadConvs.{n}", "option"): 1 for n in ("conv_center", "conv_reg", "conv_cls")}


@pytest.mark.gpu
def test_a_scene_through_cost_network_neck_and_head_hands_nothing_to_the_framework(gpu):
    """The smoke run's scene (5 views, 12 planes, 60 x 80 maps, the 40 x 40 x 16 grid) at 64 channels with the real modules attached:
    every layer of the three runs on a kernel of this library."""
    from mvsdet_amd import synthetic
    from mvsdet_amd.hotpath import MVSDetHotPath
    torch.manual_seed(3)
    N, C, D, hw = 5, 64, 12, (60, 80)
    net = CostRegNet3DGS(C).to(gpu).eval()
    neck = IndoorImVoxelNeck(C, 64, [1, 1, 1]).to(gpu).eval()
    head = NerfDetHeadConvs(18, 3, 64, 6).to(gpu).eval()
    hp = MVSDetHotPath([40, 40, 16], [0.16, 0.16, 0.2], [0.2, 5.0], D, topk=3, cost_regularization=net, neck_3d=neck, bbox_head=head)
    feat, meta = synthetic.make_features(N, C, hw, seed=123).to(gpu), synthetic.make_img_meta(N, hw, seed=123)
    layers.reset_route_stats()
    with torch.no_grad():
        out = hp.forward_scene(feat, meta)
        torch.cuda.synchronize(gpu)
    assert len(out["head"][0]) == 3
    assert layers.route_stats["framework"] == 0 and layers.framework_calls == {}
    assert layers.route_stats["hip"] == 8 + 15 + 3   # cost network; neck: ResModules 2 + 3 + 3, up blocks 2 + 2, out blocks 3; head levels
