"""train_ops.ArenaSGD on the MI355X (csrc/sgd.hip, avt_sgd_multi): SGD with momentum / weight decay / Nesterov over every parameter in
one launch, hyper-parameters read from device memory.

Error bound of the arithmetic tests: with r64 = torch's SGD formula in float64 on the CPU from the same fp32 inputs, e_torch =
max |torch.optim.SGD's fp32 result - r64| and e_hip = max |kernel - r64| per tensor, the tests assert
e_hip <= 2 e_torch + 2^-24 max|r64| for the parameter and for the momentum buffer (half an fp32 ulp of the largest value: the kernel
may round a product that torch's multi-tensor form fuses, or the other way round).  Measured on an MI355X: profiles/r11/README.md.

The replay test holds a step captured as a HIP graph to the learning rate the host sets between replays: torch's SGD in the same
harness keeps the rate it was captured with, which is what ArenaSGD exists to fix."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sgd64(p, g, buf, lr, mu, wd, nesterov):
    """One step of torch.optim.SGD (dampening 0) in float64 -> (p, buf); buf None = first step."""
    p, g = p.double(), g.double()
    if wd != 0:
        g = g + wd * p
    d = g
    if mu != 0:
        buf = g.clone() if buf is None else mu * buf.double() + g
        d = g + mu * buf if nesterov else buf
    return p - lr * d, buf


def _errs(what, got, ref32, r64):
    """Print and assert e_hip <= 2 e_torch + 2^-24 max|r64| over the finite entries of r64 (non-finite ones must agree in kind)."""
    got, ref32 = got.detach().cpu().reshape(-1), ref32.detach().cpu().reshape(-1)
    r64 = r64.reshape(-1)
    fin = torch.isfinite(r64)
    assert torch.equal(torch.isnan(got), torch.isnan(ref32)) and torch.equal(torch.isinf(got), torch.isinf(ref32)), what
    assert torch.equal(torch.isfinite(got), fin), what
    if not bool(fin.any()):
        return
    e_hip = float((got.double() - r64)[fin].abs().max())
    e_torch = float((ref32.double() - r64)[fin].abs().max())
    bound = 2 * e_torch + 2.0 ** -24 * float(r64[fin].abs().max())
    print("%s: e_torch %.3e, e_hip %.3e, bound %.3e%s" % (what, e_torch, e_hip, bound, " (bit-identical to torch)" if torch.equal(got[fin], ref32[fin]) else ""))
    assert e_hip <= bound, (what, e_hip, e_torch, bound)


def _one_step(what, dev, groups, make_param=None):
    """groups: [(kwargs of the group, [(p0 fp32 CPU, g fp32 CPU or None, buf0 fp32 CPU or None)])].  One step of ArenaSGD, of
    torch.optim.SGD and of the float64 formula from the same values; asserts the bound per tensor."""
    from avtex import train_ops

    make_param = make_param or (lambda t: torch.nn.Parameter(t.to(dev)))

    def build(cls):
        pgs, params = [], []
        for kw, tensors in groups:
            ps = [make_param(p0.clone()) for p0, _, _ in tensors]
            pgs.append(dict(kw, params=ps))
            params.append(ps)
        opt = cls(pgs, lr=1.0)
        for ps, (kw, tensors) in zip(params, groups):
            for p, (_, g, b0) in zip(ps, tensors):
                p.grad = None if g is None else g.to(dev)
                if b0 is not None:
                    assert kw.get("momentum", 0) != 0
                    if cls is torch.optim.SGD:
                        opt.state[p]["momentum_buffer"] = b0.to(dev)
                    else:
                        opt.state[p]["momentum_buffer"].copy_(b0)
        return opt, params

    before = train_ops.CALLS["sgd_multi"]
    oh, ph = build(train_ops.ArenaSGD)
    oh.step()
    assert train_ops.CALLS["sgd_multi"] == before + 1  # ONE launch, whatever the number of tensors and groups
    ot, pt = build(torch.optim.SGD)
    ot.step()
    torch.cuda.synchronize()
    for gi, (kw, tensors) in enumerate(groups):
        mu, wd, lr, nest = kw.get("momentum", 0), kw.get("weight_decay", 0), kw["lr"], kw.get("nesterov", False)
        for ti, (p0, g, b0) in enumerate(tensors):
            name = "%s [group %d tensor %d, %d elements]" % (what, gi, ti, p0.numel())
            a, t = ph[gi][ti], pt[gi][ti]
            if g is None:  # no gradient: bit-unchanged, the buffer too
                assert torch.equal(a.detach().cpu(), p0) and torch.equal(t.detach().cpu(), p0), name
                if mu != 0:
                    assert torch.equal(oh.state[a]["momentum_buffer"].cpu(), b0 if b0 is not None else torch.zeros_like(p0)), name
                continue
            p64, b64 = _sgd64(p0, g, b0, lr, mu, wd, nest)
            _errs(name + " p", a, t, p64)
            if mu != 0:
                _errs(name + " buf", oh.state[a]["momentum_buffer"], ot.state[t]["momentum_buffer"], b64)
    return oh, ph


def _rand(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("numel", [1, 3, 4, 5, 4095, 4096, 4097])
def test_one_step_chunk_edges(avt, dev, numel):
    """One tensor around the 16-byte lane width and the 4096-element chunk: first step (zero buffer) and a later one (a given buffer)."""
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
    _one_step("numel %d first step" % numel, dev, [(kw, [(_rand(numel, 1), _rand(numel, 2, 0.1), None)])])
    _one_step("numel %d later step" % numel, dev, [(kw, [(_rand(numel, 3), _rand(numel, 4, 0.1), _rand(numel, 5, 0.1))])])


def test_one_step_many_tensors_one_launch(avt, dev):
    """2^20 + 3 elements among forty tiny tensors: 257 blocks of one job between jobs of one block each."""
    sizes = [1 + (7 * i) % 13 for i in range(20)] + [(1 << 20) + 3] + [2 + (5 * i) % 11 for i in range(20)]
    tensors = [(_rand(n, 10 + i), _rand(n, 100 + i, 0.1), _rand(n, 200 + i, 0.1)) for i, n in enumerate(sizes)]
    _one_step("forty-one tensors", dev, [(dict(lr=0.05, momentum=0.9, weight_decay=1e-4), tensors)])


def test_one_step_float_aligned_view(avt, dev):
    """A parameter that starts one float into its storage: not 16-byte aligned, over more than one chunk and a tail; next to it a
    gradient at a float offset under an aligned parameter, and an aligned tensor in the same launch."""
    n = 2 * 4096 + 7

    def make_param(t):
        base = torch.zeros(t.numel() + 1, device=dev)
        base[1:].copy_(t)
        p = torch.nn.Parameter(base[1:])
        assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        return p

    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
    _one_step("view one float in", dev, [(kw, [(_rand(n, 1), _rand(n, 2, 0.1), _rand(n, 3, 0.1)), (_rand(9, 4), _rand(9, 5), None)])], make_param)
    # an aligned parameter whose GRADIENT is the view
    from avtex import train_ops

    p = torch.nn.Parameter(_rand(n, 6).to(dev))
    q = torch.nn.Parameter(_rand(4096, 7).to(dev))
    gbase = torch.cat([torch.zeros(1), _rand(n, 8, 0.1)]).to(dev)
    opt = train_ops.ArenaSGD([p, q], lr=0.05, momentum=0.9)
    p.grad, q.grad = gbase[1:], _rand(4096, 9, 0.1).to(dev)
    assert p.grad.data_ptr() % 16 == 4
    p64, b64 = _sgd64(_rand(n, 6), _rand(n, 8, 0.1), None, 0.05, 0.9, 0, False)
    pt = torch.nn.Parameter(_rand(n, 6).to(dev))
    ot = torch.optim.SGD([pt], lr=0.05, momentum=0.9)
    pt.grad = _rand(n, 8, 0.1).to(dev)
    opt.step()
    ot.step()
    _errs("gradient one float in p", p, pt, p64)
    _errs("gradient one float in buf", opt.state[p]["momentum_buffer"], ot.state[pt]["momentum_buffer"], b64)


def test_one_step_two_groups_no_momentum_nesterov(avt, dev):
    n = 4097
    t = lambda s: (_rand(n, s), _rand(n, s + 1, 0.1), _rand(n, s + 2, 0.1))  # noqa: E731
    _one_step("two groups", dev, [(dict(lr=0.05, momentum=0.9, weight_decay=1e-4), [t(1), t(4)]),
                                  (dict(lr=0.3, momentum=0.9, weight_decay=0.01), [t(7)])])
    _one_step("momentum 0", dev, [(dict(lr=0.05, weight_decay=1e-4), [(_rand(n, 1), _rand(n, 2, 0.1), None), (_rand(5, 3), _rand(5, 4), None)])])
    _one_step("momentum 0, weight decay 0", dev, [(dict(lr=0.05), [(_rand(n, 1), _rand(n, 2, 0.1), None)])])
    _one_step("nesterov", dev, [(dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True), [t(1), (_rand(n, 5), _rand(n, 6, 0.1), None)])])
    _one_step("mixed groups", dev, [(dict(lr=0.05), [t(1)[:2] + (None,)]), (dict(lr=0.01, momentum=0.5, nesterov=True), [t(4)])])


def test_one_step_grad_none_and_non_finite(avt, dev):
    n = 4097
    g = _rand(n, 2, 0.1)
    g[5], g[4090], g[4096] = float("inf"), float("nan"), float("-inf")
    oh, ph = _one_step("grad None / inf / NaN", dev, [(dict(lr=0.05, momentum=0.9, weight_decay=1e-4),
                                                     [(_rand(n, 1), g, _rand(n, 3, 0.1)),
                                                      (_rand(300, 4), None, _rand(300, 5)),   # no gradient: untouched, buffer too
                                                      (_rand(4096, 6), _rand(4096, 7, 0.1), None)])])
    p = ph[0][0].detach().cpu()
    bad = torch.zeros(n, dtype=torch.bool)
    bad[[5, 4090, 4096]] = True
    assert torch.equal(~torch.isfinite(p), bad)  # ... reach those elements only
    assert torch.isnan(p[4090]) and p[5] == float("-inf") and p[4096] == float("inf")


def test_twenty_steps_with_a_rate_drop(avt, dev):
    """Twenty steps on a fixed gradient sequence, StepLR dividing the rate by 10 at step 10: the float64 trajectory, torch's SGD and the
    kernel from the same fp32 inputs; the bound of the one-step tests at the end, for parameters and buffers.  Also: the state goes
    into torch.optim.SGD and back, and a step after that continues the trajectory."""
    from avtex import train_ops

    sizes = [4097, 5, 1 << 14]
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
    p0 = [_rand(n, 1 + i) for i, n in enumerate(sizes)]
    grads = [[_rand(n, 1000 + 10 * s + i, 0.1) for i, n in enumerate(sizes)] for s in range(20)]
    ph, pt = [torch.nn.Parameter(p.to(dev)) for p in p0], [torch.nn.Parameter(p.to(dev)) for p in p0]
    oh, ot = train_ops.ArenaSGD(ph, **kw), torch.optim.SGD(pt, **kw)
    sh, st = (torch.optim.lr_scheduler.StepLR(o, step_size=10, gamma=0.1) for o in (oh, ot))
    p64, b64 = [p.double() for p in p0], [None] * len(p0)
    before = train_ops.CALLS["sgd_multi"]
    for s in range(20):
        lr = oh.param_groups[0]["lr"]
        assert lr == ot.param_groups[0]["lr"] and abs(lr - (0.05 if s < 10 else 0.005)) < 1e-12
        for i in range(len(p0)):
            ph[i].grad, pt[i].grad = grads[s][i].to(dev), grads[s][i].to(dev)
            g = grads[s][i].double() + kw["weight_decay"] * p64[i]
            b64[i] = g.clone() if b64[i] is None else kw["momentum"] * b64[i] + g
            p64[i] = p64[i] - lr * b64[i]
        oh.step()
        ot.step()
        sh.step()
        st.step()
    assert train_ops.CALLS["sgd_multi"] == before + 20
    for i, n in enumerate(sizes):
        _errs("20 steps, %d elements, p" % n, ph[i], pt[i], p64[i])
        _errs("20 steps, %d elements, buf" % n, oh.state[ph[i]]["momentum_buffer"], ot.state[pt[i]]["momentum_buffer"], b64[i])
    # without the rate drop the trajectories differ by far more than the bound: the drop is what was tested
    assert float((ph[0].detach().cpu().double() - p64[0]).abs().max()) < 1e-5
    # state_dict: into torch.optim.SGD and back (deep copies: load_state_dict may keep the very tensors it is given)
    bufs = [oh.state[p]["momentum_buffer"].clone() for p in ph]
    p2 = [torch.nn.Parameter(p.detach().clone()) for p in ph]
    o2 = torch.optim.SGD(p2, lr=1.0)
    o2.load_state_dict(copy.deepcopy(oh.state_dict()))
    assert abs(o2.param_groups[0]["lr"] - 0.0005) < 1e-12
    p3 = [torch.nn.Parameter(p.detach().clone()) for p in ph]
    o3 = train_ops.ArenaSGD(p3, lr=1.0)
    o3.load_state_dict(copy.deepcopy(o2.state_dict()))
    for a, b, c in zip(bufs, p2, p3):
        assert torch.equal(a, o2.state[b]["momentum_buffer"]) and torch.equal(a, o3.state[c]["momentum_buffer"])
        assert o3.state[c]["momentum_buffer"].data_ptr() not in (a.data_ptr(), o2.state[b]["momentum_buffer"].data_ptr())
    for i in range(len(p0)):
        p2[i].grad, p3[i].grad = grads[0][i].to(dev), grads[0][i].to(dev)
    o2.step()
    o3.step()
    for i, n in enumerate(sizes):
        r64, b64 = _sgd64(ph[i].detach().cpu(), grads[0][i], bufs[i].cpu(), 0.0005, 0.9, 1e-4, False)
        _errs("step after the round trip, %d elements, p" % n, p3[i], p2[i], r64)
        _errs("step after the round trip, %d elements, buf" % n, o3.state[p3[i]]["momentum_buffer"], o2.state[p2[i]]["momentum_buffer"], b64)


def test_refused_on_the_device(avt, dev):
    from avtex import train_ops

    AvtError = avt._lib.AvtError
    for bad in (torch.zeros(8, device=dev, dtype=torch.float16), torch.zeros(4, 8, device=dev)[:, ::2], torch.zeros(4, 8, device=dev).t(),
                torch.zeros(8)):
        with pytest.raises(AvtError):
            train_ops.ArenaSGD([torch.nn.Parameter(bad)], lr=0.1)
    w = torch.nn.Parameter(torch.zeros(8, 16, 1, 3, 3, device=dev).contiguous(memory_format=torch.channels_last_3d))
    opt = train_ops.ArenaSGD([w], lr=0.1, momentum=0.9)  # the training layout's convolution weights
    w.grad = torch.ones(8, 16, 1, 3, 3, device=dev)  # ... but a gradient in another layout is refused, not re-laid-out silently
    with pytest.raises(AvtError, match="strides"):
        opt.step()
    w.grad = torch.ones_like(w)
    opt.step()
    assert torch.equal(w.detach(), torch.full_like(w, -0.1))


def test_replay_follows_the_rate():
    """A step captured once as a HIP graph (train_ops.GraphedStep) with ArenaSGD inside: three replays at lr 0.05, the rate set to 0.005
    on the host + sync_hyper(), three more — against the same six steps run eagerly (the tolerance of
    test_graphed_step_equals_the_eager_step, which was set for six steps of this net).  Then lr = 0: one more replay leaves every
    parameter bit-identical.  torch.optim.SGD in the same harness keeps moving them: its rate is a kernel argument, frozen at capture."""
    from avtex import train_ops
    from avtex.slowfast import ResBlock
    from avtex.train import _restore, _snapshot

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net0 = torch.nn.Sequential(ResBlock(16, 64, 16, 3, 1), ResBlock(64, 64, 16, 3, 1)).to(dev).to(memory_format=torch.channels_last_3d).train()
    xs = [torch.randn(4, 16, 4, 12, 12, device=dev).contiguous(memory_format=torch.channels_last_3d) for _ in range(7)]

    def run(graphed, make_opt):
        net = copy.deepcopy(net0)
        train_ops.invalidate_weight_cache()
        opt = make_opt(net.parameters())
        x_buf = xs[0].clone()

        def step():
            opt.zero_grad(set_to_none=True)
            with train_ops.bn_replicas(2):
                y = net(x_buf)
            loss = y.square().mean()
            loss.backward()
            opt.step()
            return loss.detach()

        def set_lr(lr):
            opt.param_groups[0]["lr"] = lr
            if hasattr(opt, "sync_hyper"):
                assert opt.sync_hyper() and not opt.sync_hyper()  # copies once per change

        run_step = step
        if graphed:
            # what train() does for the first batch of a shape: one eager step fills the step's caches, the capture records the launches,
            # and the state goes back to where it was — the replays below are the only steps taken
            saved = _snapshot(net, opt)
            step()
            torch.cuda.synchronize()
            run_step = train_ops.GraphedStep(step, dev, warmup=0, before_capture=lambda: train_ops.weight_cache_is_stale() or pytest.fail("planes current"))
            _restore(saved)
            train_ops.invalidate_weight_cache()
        losses = []
        for i, x in enumerate(xs[:6]):
            if i == 3:
                set_lr(0.005)
            x_buf.copy_(x)
            losses.append(float(run_step()))
        torch.cuda.synchronize()
        params, bufs = [p.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()]
        set_lr(0.0)
        x_buf.copy_(xs[6])
        run_step()
        torch.cuda.synchronize()
        frozen = all(torch.equal(a, b.detach()) for a, b in zip(params, net.parameters()))
        return losses, params, bufs, frozen

    arena = lambda ps: train_ops.ArenaSGD(ps, lr=0.05, momentum=0.9)  # noqa: E731
    before = train_ops.CALLS["sgd_multi"]
    le, pe, be, frozen_eager = run(False, arena)
    assert train_ops.CALLS["sgd_multi"] == before + 7
    lg, pg, bg, frozen_graph = run(True, arena)
    assert train_ops.CALLS["sgd_multi"] == before + 7 + 2  # (the eager step and the capture: replays do not pass through the host)
    print("eager losses", le, "replayed losses", lg)
    assert all(abs(a - b) <= 1e-5 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    for a, b in zip(pe, pg):
        assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max()) + 1e-7
    for a, b in zip(be, bg):
        assert float((a.float() - b.float()).abs().max()) <= 1e-5 * float(a.float().abs().max()) + 1e-6
    assert frozen_eager and frozen_graph  # lr = 0 (no weight decay): p - 0 * d = p, bit for bit
    # what this guards: torch's SGD under the same replay still applies the rate it was captured with
    _, _, _, frozen_torch = run(True, lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=0.9))
    assert not frozen_torch


def test_table_lifetime_across_a_capture(avt, dev):
    """The job table of ArenaSGD.step() (train_ops._JobTable, shared with GradExchange and the weight-plane refresh): built once while the
    addresses stand, built under the capture when the gradients moved (its upload a node of the graph: the replays follow gradient VALUES
    written in place), never launched eagerly afterwards and kept alive.  Every update against torch.optim.SGD on an fp64 CPU copy and
    torch's fp32 step from the same gradients: the bound of the one-step tests (_errs).  A second capture in a row finds no staging
    buffer and is refused on the host, before any launch."""
    from avtex import train_ops

    kw = dict(lr=0.05, momentum=0.9)
    shapes = [(1,), (4097,), (8, 8, 1, 3, 3)]  # one element; one chunk and one element; a channels-last weight

    def tensor(shape, seed, scale=1.0):
        t = _rand(int(np.prod(shape)), seed, scale).view(shape)
        return t.contiguous(memory_format=torch.channels_last_3d) if len(shape) == 5 else t

    p0 = [tensor(s, 1 + i) for i, s in enumerate(shapes)]
    ph, pt = [torch.nn.Parameter(p.to(dev)) for p in p0], [torch.nn.Parameter(p.to(dev)) for p in p0]
    p64 = [torch.nn.Parameter(p.double()) for p in p0]
    assert not ph[2].is_contiguous() and ph[2].is_contiguous(memory_format=torch.channels_last_3d)
    oh, ot, o64 = train_ops.ArenaSGD(ph, **kw), torch.optim.SGD(pt, **kw), torch.optim.SGD(p64, **kw)
    for p in ph + pt:
        p.grad = torch.zeros_like(p)
    for p in p64:
        p.grad = torch.zeros_like(p)
    seed = [100]

    def new_gradients():
        for i, s in enumerate(shapes):
            g = tensor(s, seed[0] + i, 0.1)
            with torch.no_grad():
                ph[i].grad.copy_(g.to(dev))  # in place: the addresses stand
                pt[i].grad.copy_(g.to(dev))
                p64[i].grad.copy_(g.double())
        seed[0] += 10

    def move_gradients():
        for p in ph:
            p.grad = p.grad.clone(memory_format=torch.preserve_format)  # (the old tensor is alive during the clone: a new address)

    def check(what):
        ot.step()
        o64.step()
        torch.cuda.synchronize()
        for i, s in enumerate(shapes):
            _errs("%s, shape %s, p" % (what, s), ph[i], pt[i], p64[i].detach())
            _errs("%s, shape %s, buf" % (what, s), oh.state[ph[i]]["momentum_buffer"], ot.state[pt[i]]["momentum_buffer"],
                  o64.state[p64[i]]["momentum_buffer"])

    before = train_ops.CALLS["sgd_multi"]
    new_gradients()
    oh.step()
    check("eager step 1")
    tab = oh._jobs.table
    new_gradients()
    oh.step()
    check("eager step 2")
    assert oh._jobs.table is tab and not tab.captured and train_ops.CALLS["sgd_multi"] - before == 2
    # gradients at NEW addresses, as the backward of a captured step leaves them: the table is built under the capture
    move_gradients()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        oh.step()
    assert oh._jobs.table is not tab and oh._jobs.table.captured and train_ops.CALLS["sgd_multi"] - before == 3
    for k in range(3):
        new_gradients()
        graph.replay()
        check("replay %d" % (k + 1))
    assert train_ops.CALLS["sgd_multi"] - before == 3  # replays do not pass the host
    new_gradients()
    oh.step()  # an eager step after the capture builds a table of its own and leaves the captured one alone
    check("eager step after the capture")
    assert not oh._jobs.table.captured and len(oh._jobs.kept) == 1


def test_a_second_capture_in_a_row_is_refused(avt, dev):
    """The staging buffer of a captured table is set aside by an eager step() / sync_hyper(); a capture used it up.  A second capture with
    the gradients moved again, and nothing eager between, has none: AvtError on the host, before any launch."""
    from avtex import train_ops

    p = torch.nn.Parameter(torch.zeros(4097, device=dev))
    opt = train_ops.ArenaSGD([p], lr=0.05, momentum=0.9)
    p.grad = torch.ones_like(p)
    mark = torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    first = torch.cuda.CUDAGraph()
    with torch.cuda.graph(first, stream=stream):
        opt.step()
    assert opt._jobs.table.captured
    p.grad = p.grad.clone()
    before = train_ops.CALLS["sgd_multi"]
    second = torch.cuda.CUDAGraph()
    with pytest.raises(avt._lib.AvtError, match=r"ArenaSGD\.step\(\) under stream capture: no staging buffer is left .*sync_hyper\(\) or step\(\)"):
        with torch.cuda.graph(second, stream=stream):
            mark.add_(1)  # (so that the abandoned graph is not an empty one)
            opt.step()
    assert train_ops.CALLS["sgd_multi"] == before
