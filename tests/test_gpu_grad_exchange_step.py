"""The step train() replays on every rank, on layers that reach the hand-written kernels: two ResBlocks (channels-last Conv3d weights, whose
views of the exchange buffer are strided; BatchNorm3d with running statistics under bn_replicas(2); weight planes that the capture must
re-make, because the optimizer runs outside it).  One process, world 1 (the all-reduce has nobody to talk to; scale = 1): the captured
part is invalidate + zero_grad + forward + backward + GradExchange.pack(), the eager part train._exchange_and_step — six steps across a
change of the rate against the same six steps of the plain eager loop, in the tolerance of test_replay_follows_the_rate (same net, same
steps)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_exchange_step_equals_the_eager_step_on_conv_and_batchnorm_layers(avt, dev):
    from avtex import train_ops
    from avtex.slowfast import ResBlock
    from avtex.train import _exchange_and_step, _restore, _snapshot

    torch.manual_seed(0)
    net0 = torch.nn.Sequential(ResBlock(16, 64, 16, 3, 1), ResBlock(64, 64, 16, 3, 1)).to(dev).to(memory_format=torch.channels_last_3d).train()
    xs = [torch.randn(4, 16, 4, 12, 12, device=dev).contiguous(memory_format=torch.channels_last_3d) for _ in range(6)]
    seen = {}

    def run(exchange):
        net = copy.deepcopy(net0)
        train_ops.invalidate_weight_cache()
        opt = train_ops.ArenaSGD(net.parameters(), lr=0.05, momentum=0.9)
        x_buf = xs[0].clone()

        def forward_backward():
            opt.zero_grad(set_to_none=True)
            with train_ops.bn_replicas(2):
                y = net(x_buf)
            loss = y.square().mean()
            loss.backward()
            return loss.detach()

        if not exchange:
            def run_step():
                loss = forward_backward()
                opt.step()
                return loss
        else:
            ex = train_ops.GradExchange(net.parameters(), 1)

            def device_step():
                train_ops.invalidate_weight_cache()  # (the optimizer runs outside: the plane re-make must be a node of the graph)
                loss = forward_backward()
                if not ex.bound:
                    ex.bind()
                ex.pack()
                return loss

            saved = _snapshot(net, opt)
            graphed = train_ops.GraphedStep(device_step, dev, warmup=2, after_warmup=lambda: _exchange_and_step(opt, ex),
                                            before_capture=lambda: train_ops.weight_cache_is_stale() or pytest.fail("planes current"))
            _restore(saved)
            train_ops.invalidate_weight_cache()
            seen["ex"], seen["launches"] = ex, dict(train_ops.CALLS)

            def run_step():
                loss = graphed()
                _exchange_and_step(opt, ex)
                return loss

        losses = []
        for i, x in enumerate(xs):
            if i == 3:
                opt.param_groups[0]["lr"] = 0.005
            x_buf.copy_(x)
            losses.append(float(run_step()))
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()]

    le, pe, be = run(False)
    lg, pg, bg = run(True)
    ex = seen["ex"]
    # what the fixture is for: strided views of channels-last weights, buffers that move, planes re-made without the host
    assert any(not v.is_contiguous() for v in ex.views) and all(v.stride() == p.stride() for p, v in zip(ex.params, ex.views))
    assert len(be) > 0 and any(not torch.equal(a, b) for a, b in zip(be, net0.buffers()))
    after = train_ops.CALLS
    assert after["grad_pack_multi"] == seen["launches"]["grad_pack_multi"] and after["planes_multi"] == seen["launches"]["planes_multi"]
    assert after["conv_fwd_x3"] == seen["launches"]["conv_fwd_x3"] > 0  # (the replays ran the hand-written convolutions, not the host)
    assert after["sgd_multi"] - seen["launches"]["sgd_multi"] == 6      # (one eager optimizer launch per step)
    print("eager losses", le, "exchange-step losses", lg)
    assert all(abs(a - b) <= 1e-5 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    for a, b in zip(pe, pg):
        assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max()) + 1e-7
    for a, b in zip(be, bg):
        assert float((a.float() - b.float()).abs().max()) <= 1e-5 * float(a.float().abs().max()) + 1e-6
