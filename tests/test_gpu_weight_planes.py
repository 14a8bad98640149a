"""The weight-plane cache (weight_planes.py) on the device: what a GraphedStep's capture leaves behind, how many launches keep the planes
current, and a model that moves to another GPU.  The small net of test_stale_weight_planes_are_remade_by_one_launch_bit_for_bit."""
import copy

import pytest
import torch


def _net_and_input(dev):
    from avtex.slowfast import ResBlock

    torch.manual_seed(11)
    net = torch.nn.Sequential(ResBlock(16, 64, 16, 3, 1), ResBlock(64, 128, 32, 1, 2)).to(dev).to(memory_format=torch.channels_last_3d).train()
    x = torch.randn(2, 16, 4, 16, 16, device=dev).contiguous(memory_format=torch.channels_last_3d)
    return net, x


def _forward(net, x):
    from avtex import train_ops

    with train_ops.bn_replicas(1):
        return net(x)


def _step(net, x):
    """Forward, backward and an in-place update of every parameter (the versions move, the tensors stay) -> the forward's output."""
    net.zero_grad(set_to_none=True)
    y = _forward(net, x)
    y.square().mean().backward()
    with torch.no_grad():
        for p in net.parameters():
            p.sub_(p.grad, alpha=0.01)
    return y.detach()


def _tensors(v, out):
    if torch.is_tensor(v):
        out.append(v)
    elif isinstance(v, (tuple, list)):
        for e in v:
            _tensors(e, out)
    return out


@pytest.mark.gpu
def test_a_capture_leaves_nothing_behind(dev):
    """GraphedStep's capture marks the planes current although nothing ran and records its refresh event inside the capture.  Without
    any invalidate by hand afterwards the cache is stale, a forward on a stream the process has not used yet waits for no captured event,
    and it computes with the planes of the weights as they are."""
    from avtex import train_ops, weight_planes

    net, x = _net_and_input(dev)
    train_ops.invalidate_weight_cache(drop=True)
    try:
        _step(net, x)            # the entries exist: the warm-up step re-makes them by one launch and builds its table, the capture reuses it
        n0 = train_ops.CALLS["planes_multi"]
        graphed = train_ops.GraphedStep(lambda: _step(net, x), dev, warmup=1)
        assert train_ops.CALLS["planes_multi"] == n0 + 2   # (the refresh launch really was part of the capture)
        assert train_ops.weight_cache_is_stale()
        assert dev not in weight_planes.CACHE.refreshed
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            y_side = _forward(net, x).detach()
        torch.cuda.synchronize(dev)
        train_ops.invalidate_weight_cache(drop=True)
        y_fresh = _forward(net, x).detach()
        torch.cuda.synchronize(dev)
        assert torch.equal(y_side, y_fresh)
        del graphed
    finally:
        train_ops.invalidate_weight_cache(drop=True)


@pytest.mark.gpu
def test_one_refresh_launch_per_step_and_no_new_entries(dev):
    from avtex import train_ops, weight_planes

    net, x = _net_and_input(dev)
    train_ops.invalidate_weight_cache(drop=True)
    keep, weight_planes._PLANES_MULTI = weight_planes._PLANES_MULTI, 1
    try:
        n0 = train_ops.CALLS["planes_multi"]
        _step(net, x)            # every entry made one by one
        assert train_ops.CALLS["planes_multi"] == n0
        _step(net, x)
        assert train_ops.CALLS["planes_multi"] == n0 + 1
        entries = len(weight_planes.CACHE.entries)
        _step(net, x)
        assert train_ops.CALLS["planes_multi"] == n0 + 2
        assert len(weight_planes.CACHE.entries) == entries > 0
        torch.cuda.synchronize(dev)
    finally:
        weight_planes._PLANES_MULTI = keep
        train_ops.invalidate_weight_cache(drop=True)


@pytest.mark.gpu
def test_planes_follow_a_model_to_another_gpu(dev):
    """net.to(another GPU) keeps every Parameter's identity and version; the device is part of the entries' signature, so their recipes
    are void and the planes are made anew where the weights now are."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from avtex import train_ops, weight_planes

    other = torch.device("cuda:1")
    net, x = _net_and_input(dev)
    train_ops.invalidate_weight_cache(drop=True)
    try:
        _step(net, x)
        torch.cuda.synchronize(dev)
        net.to(other)
        x1 = x.to(other)
        with torch.cuda.device(other):
            fresh = copy.deepcopy(net)
            y = _step(net, x1)
            own = {id(p) for p in net.parameters()}
            mine = [e for e in weight_planes.CACHE.entries.values() if e.ref() is not None and id(e.ref()) in own]
            assert mine and all(t.device == other for e in mine for t in _tensors(e.value, []))
            y_fresh = _forward(fresh, x1).detach()
            torch.cuda.synchronize(other)
        assert torch.equal(y, y_fresh)
    finally:
        train_ops.invalidate_weight_cache(drop=True)
