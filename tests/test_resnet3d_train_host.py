"""resnet3d.py calls the training passes of train_ops; everywhere those passes do not apply (CPU, eval mode) the modules compute what the
plain network computes, bit for bit, and the checkpoint surface (state-dict keys, parameter shapes) is what it was.  No GPU."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

BN = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
BLOCKS = {"resnet10": [1, 1, 1, 1], "resnet18": [2, 2, 2, 2], "resnet34": [3, 4, 6, 3], "resnet50": [3, 4, 6, 3]}
WIDTHS = [64, 128, 256, 512]


def _expected_keys(arch):
    """The state-dict keys of the network as it has always been saved: stem, then per block conv1 / bn1 / conv2 / bn2 and, on the
    first block of layers 2-4, the projection `downsample.0` (convolution) / `downsample.1` (BatchNorm); the unused fc last."""
    keys = ["conv1.weight"] + ["bn1." + k for k in BN]
    for li, n in enumerate(BLOCKS[arch]):
        for b in range(n):
            p = "layer%d.%d." % (li + 1, b)
            keys += [p + "conv1.weight"] + [p + "bn1." + k for k in BN] + [p + "conv2.weight"] + [p + "bn2." + k for k in BN]
            if b == 0 and li > 0:
                keys += [p + "downsample.0.weight"] + [p + "downsample.1." + k for k in BN]
    return keys + ["fc.weight", "fc.bias"]


def _plain_block(blk, x):
    r = x if blk.downsample is None else blk.downsample[1](blk.downsample[0](x))
    y = F.relu(blk.bn1(blk.conv1(x)))
    y = blk.bn2(blk.conv2(y))
    return F.relu(y + r)


def _plain_net(net, x):
    x = net.maxpool(F.relu(net.bn1(net.conv1(x))))
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for blk in layer:
            x = _plain_block(blk, x)
    return net.avgpool(x)


@pytest.mark.parametrize("arch", ["resnet10", "resnet18", "resnet34", "resnet50"])
def test_state_dict_keys_and_shapes(avt, arch):
    from avtex import resnet3d

    net = resnet3d.build(arch, 64, 16)
    sd = net.state_dict()
    assert list(sd.keys()) == _expected_keys(arch)
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7, 7) and tuple(sd["fc.weight"].shape) == (1039, 512)
    cin = 64
    for li, c in enumerate(WIDTHS):
        p = "layer%d.0." % (li + 1)
        assert tuple(sd[p + "conv1.weight"].shape) == (c, cin, 3, 3, 3) and tuple(sd[p + "conv2.weight"].shape) == (c, c, 3, 3, 3)
        if li > 0:
            assert tuple(sd[p + "downsample.0.weight"].shape) == (c, cin, 1, 1, 1)
        cin = c


def test_initialisation_order_is_unchanged(avt):
    """The same seed gives the weights the plain constructor order gives: stem, then per block conv1, conv2, projection — drawn by ONE
    kaiming pass over modules() after every layer exists."""
    from avtex import resnet3d

    torch.manual_seed(7)
    a = resnet3d.build("resnet10", 64, 16)
    torch.manual_seed(7)
    b = resnet3d.build("resnet10", 64, 16)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    torch.manual_seed(7)
    convs = [nn.Conv3d(3, 64, 7, stride=(1, 2, 2), padding=3, bias=False)]
    cin = 64
    for li, c in enumerate(WIDTHS):  # construction order inside _make: the projection BEFORE the block's convolutions
        proj = [nn.Conv3d(cin, c, 1, stride=2, bias=False)] if li > 0 else []
        if proj:
            nn.BatchNorm3d(c)
        blk = [nn.Conv3d(cin, c, 3, stride=1 if li == 0 else 2, padding=1, bias=False), nn.Conv3d(c, c, 3, padding=1, bias=False)]
        convs += blk + proj  # modules() order: conv1, conv2, downsample
        cin = c
    nn.Linear(512, 1039)
    for m in convs:
        nn.init.kaiming_normal_(m.weight, mode="fan_out")
    got = [m.weight for m in a.modules() if isinstance(m, nn.Conv3d)]
    assert len(got) == len(convs) and all(torch.equal(g, w.weight) for g, w in zip(got, convs))


@pytest.mark.parametrize("training", [True, False])
def test_cpu_forward_is_the_plain_network_bit_for_bit(avt, training):
    from avtex import resnet3d, synth

    torch.manual_seed(3)
    net = synth.randomise_bn(resnet3d.build("resnet18", 64, 16), 5, 0.3)
    ref = resnet3d.build("resnet18", 64, 16)
    ref.load_state_dict(net.state_dict())
    net.train(training)
    ref.train(training)
    x = torch.randn(2, 3, 16, 64, 64)
    with torch.set_grad_enabled(training):
        y, yr = net(x), _plain_net(ref, x)
    assert y.shape == (2, 512, 1, 1, 1) and torch.equal(y, yr)
    for (k, a), b in zip(net.state_dict().items(), ref.state_dict().values()):
        assert torch.equal(a, b), k  # running statistics took the same update
    if training:
        y.square().sum().backward()
        yr.square().sum().backward()
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
    blk, rblk = net.layer2[0], ref.layer2[0]
    xb = torch.randn(2, 64, 4, 8, 8)
    assert torch.equal(blk(xb), _plain_block(rblk, xb))
    assert torch.equal(net.layer1[1](xb), _plain_block(ref.layer1[1], xb))


def test_max_pool3d_falls_through_to_the_module(avt):
    from avtex import train_ops

    x = torch.relu(torch.randn(2, 8, 5, 7, 9)).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    before = train_ops.CALLS["maxpool3d_hip"]
    stem_pool = nn.MaxPool3d(3, stride=2, padding=1).train()
    assert torch.equal(train_ops.max_pool3d(x, stem_pool), stem_pool(x))  # a CPU tensor
    for pool in (nn.MaxPool3d(2, stride=2, padding=1), nn.MaxPool3d(3, stride=1, padding=1), nn.MaxPool3d(3, stride=2, padding=0),
                 nn.MaxPool3d((1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1)), nn.MaxPool3d(3, stride=2, padding=1, ceil_mode=True)):
        assert torch.equal(train_ops.max_pool3d(x, pool), pool(x))
    assert train_ops.CALLS["maxpool3d_hip"] == before and "maxpool3d_hip" in train_ops.CALLS
