"""csrc/grad_pack.hip through train_ops.GradExchange on the MI355X: every gradient, times a scale the kernel LOADS, into one flat buffer
in one launch.  Sizes cross the 4-element (16-byte) and the 4096-element (block) boundaries; one source is a view one float off a
16-byte boundary (the dword path); one is a channels-last 5-D weight whose view of the flat buffer is strided.  One fp32 multiply on
each side, so the comparison with torch's `src * scale` is exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 4095, 4096, 4097, 8193]


def _exchange(dev, world, seed=0):
    """-> (GradExchange bound over the fixture's parameters, the parameters, a canary allocated right after `flat`)."""
    from avtex import train_ops

    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.zeros(n, device=dev)) for n in SIZES]
    for p in params:
        p.grad = torch.randn(p.numel(), generator=g).to(dev)
    # a gradient that is a view starting ONE float off a 16-byte boundary
    odd = torch.nn.Parameter(torch.zeros(4099, device=dev))
    base = torch.randn(4099 + 8, generator=g).to(dev)
    assert base.data_ptr() % 16 == 0
    odd.grad = base[1 : 1 + 4099]
    assert odd.grad.data_ptr() % 16 == 4
    # a channels-last 5-D weight: its gradient has the parameter's strides, its view of the flat buffer is an as_strided one
    w = torch.nn.Parameter(torch.zeros(8, 4, 1, 3, 3, device=dev).contiguous(memory_format=torch.channels_last_3d))
    w.grad = torch.randn(8, 4, 1, 3, 3, generator=g).to(dev).contiguous(memory_format=torch.channels_last_3d)
    assert not w.grad.is_contiguous()
    # ... and a parameter without a gradient, which bind() leaves out
    idle = torch.nn.Parameter(torch.zeros(7, device=dev))
    params += [odd, w, idle]
    ex = train_ops.GradExchange(params, world)
    ex.bind()
    canary = torch.full((4096,), 7.25, device=dev)
    return ex, params[:-1], canary


def _check(ex, params, canary):
    from avtex import train_ops

    torch.cuda.synchronize()
    assert len(ex.views) == len(params) == len(SIZES) + 2
    used = torch.zeros(ex.flat.numel(), dtype=torch.bool, device=ex.flat.device)
    for p, v, o in zip(params, ex.views, ex.offsets):
        assert v.shape == p.shape and v.stride() == p.stride() and o % 4 == 0
        assert torch.equal(v, p.grad * ex.scale), (tuple(p.shape), float((v - p.grad * ex.scale).abs().max()))
        used[o : o + p.numel()] = True
    assert ex.total == sum((p.numel() + 3) // 4 * 4 for p in params) == ex.flat.numel() == train_ops.exchange_layout(
        [p.numel() for p in params])[1]
    assert int((~used).sum()) == sum(-p.numel() % 4 for p in params) > 0
    assert bool((ex.flat[~used] == 0).all()), "the padding words of the flat buffer were written"
    assert bool((canary == 7.25).all()), "the launch wrote past the flat buffer"


@pytest.mark.parametrize("world", [2, 3])
def test_pack_equals_torch_scale_and_stays_in_bounds(avt, dev, world):
    from avtex import train_ops

    ex, params, canary = _exchange(dev, world)
    assert float(ex.scale) == float(torch.tensor(1.0 / world, dtype=torch.float32))
    assert not ex.views[-1].is_contiguous()  # (the channels-last weight: a strided view)
    before = train_ops.CALLS["grad_pack_multi"]
    ex.pack()
    _check(ex, params, canary)
    tab = ex._jobs.table
    ex.pack()  # the same addresses: the table is built once
    assert ex._jobs.table is tab and train_ops.CALLS["grad_pack_multi"] - before == 2
    _check(ex, params, canary)
    # new gradient tensors: a new table, the same result
    for p in params:
        p.grad = (p.grad * 3 + 1).clone(memory_format=torch.preserve_format)
    ex.pack()
    assert ex._jobs.table is not tab
    _check(ex, params, canary)
    # install(): the parameters' gradients ARE the views from then on; packing them onto themselves is refused
    ex.install()
    assert all(p.grad is v for p, v in zip(params, ex.views))
    with pytest.raises(avt._lib.AvtError):
        ex.pack()


def test_captured_pack_follows_the_values_and_the_scale(avt, dev):
    from avtex import train_ops

    ex, params, canary = _exchange(dev, 2, seed=1)
    ex.pack()  # (a warm-up launch, as a step has before its capture)
    _check(ex, params, canary)
    # gradients at NEW addresses, as the backward of a captured step produces them: the table is then built under the capture and its
    # upload is a node of the graph (the staging buffer was set aside by bind())
    for p in params:
        if p.grad.data_ptr() % 16:
            g = torch.empty(p.numel() + 8, device=dev)[1 : 1 + p.numel()]
            assert g.data_ptr() % 16 == 4
            p.grad = g.copy_(p.grad)
        else:
            p.grad = p.grad.clone(memory_format=torch.preserve_format)
    torch.cuda.synchronize()
    before = train_ops.CALLS["grad_pack_multi"]
    stream = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ex.pack()
    assert train_ops.CALLS["grad_pack_multi"] - before == 1 and ex._jobs.table.captured
    for scale, shift in ((0.5, 0.0), (1.0 / 3.0, 2.0), (0.5, -1.0)):
        with torch.no_grad():
            for p in params:
                p.grad.mul_(1.5).add_(shift)  # new VALUES at the captured addresses
            ex.scale.fill_(scale)
            ex.flat[0] = -1.0  # (stale output the replay must overwrite)
        graph.replay()
        _check(ex, params, canary)
    assert train_ops.CALLS["grad_pack_multi"] - before == 1  # replays do not pass the host
    ex.pack()  # an eager launch after the capture builds a table of its own and leaves the captured one alone
    assert not ex._jobs.table.captured and len(ex._jobs.kept) == 1
    _check(ex, params, canary)


def test_bad_gradients_are_refused(avt, dev):
    from avtex import train_ops

    p = torch.nn.Parameter(torch.zeros(8, 4, 1, 3, 3, device=dev).contiguous(memory_format=torch.channels_last_3d))
    q = torch.nn.Parameter(torch.zeros(6, device=dev))
    p.grad = torch.zeros_like(p)
    q.grad = torch.zeros_like(q)
    ex = train_ops.GradExchange([p, q], 2)
    with pytest.raises(avt._lib.AvtError):
        ex.pack()  # before bind()
    ex.bind()
    p.grad = torch.zeros(8, 4, 1, 3, 3, device=dev)  # torch's default strides for a channels-last parameter
    with pytest.raises(avt._lib.AvtError):
        ex.pack()
    p.grad = torch.zeros_like(p)
    q.grad = None
    with pytest.raises(avt._lib.AvtError):
        ex.pack()
    # a parameter that had no gradient at bind() and gains one later would be stepped on its un-exchanged gradient: refused
    late = torch.nn.Parameter(torch.zeros(5, device=dev))
    q.grad = torch.zeros_like(q)
    ex2 = train_ops.GradExchange([p, q, late], 2)
    ex2.bind()
    ex2.pack()
    late.grad = torch.zeros_like(late)
    with pytest.raises(avt._lib.AvtError, match="had none at bind"):
        ex2.pack()
