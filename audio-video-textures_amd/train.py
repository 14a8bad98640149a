"""`train()` — one epoch of InfoNCE SGD, drop-in for contrastive_video_textures/train.py:39-210
(same signature, same meters and prints; tensorboard images are skipped when no logger is given).
The loss runs on the HIP softmax-CE kernels (models.InfoNCECriterion)."""
import time
from collections import OrderedDict

import torch

from . import train_ops
from ._lib import AvtError
from .models import InfoNCECriterion
from .utils import AverageMeter


def to_cuda(item):
    if isinstance(item[0], list):
        return [[x.cuda() for x in y] for y in item]
    elif isinstance(item, list):
        return [x.cuda() for x in item]
    return item.cuda()


def train(train_loader, model, optimizer, args, epoch, tb_logger=None):
    batch_time, data_time, losses = AverageMeter(), AverageMeter(), AverageMeter()
    model.train()
    if not next(model.parameters()).is_cuda:
        raise AvtError("train(): model must be on the MI355X (model.cuda()); the loss runs on the HIP kernels, no CPU fallback")
    criterion = InfoNCECriterion()
    # --train_graph: the device side of a step captured once per batch shape as a HIP graph and replayed (train_ops.GraphedStep) — for
    # small batches, whose ~3400 launches the host issues slower than the device runs them (config 5 on 8 GPUs: one item per rank;
    # DESIGN.md 5.2).  One process: forward, loss, backward and the optimizer are the graph.  Several ranks (the model prepared by
    # train_ops.prepare_ranks, not wrapped in DistributedDataParallel, whose bucketed all-reduce is not captured): the graph ends with the
    # backward and ONE launch that packs the gradients into a flat buffer (train_ops.GradExchange); one all-reduce and the optimizer
    # follow every replay eagerly.  A DistributedDataParallel model keeps the eager loop.  A model that prepare_ranks prepared takes the
    # same ranks form WITHOUT --train_graph too, eagerly: forward and backward, the pack, the exchange, the optimizer (main() prepares
    # it that way with --train_deterministic, whose ordered exchange DistributedDataParallel's bucketed all-reduce is not).
    graphed = model.__dict__.setdefault("_avt_graphed_steps", {})  # (kept on the model: train() is called once per epoch)
    if graphed.get("optimizer") is not optimizer:
        graphed.clear()
        graphed["optimizer"] = optimizer
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    world = torch.distributed.get_world_size() if dist_on else 1
    ddp = isinstance(model, torch.nn.parallel.DistributedDataParallel)
    # (a model that train_ops.prepare_ranks prepared takes the ranks form under a ONE-rank process group too:
    #  tools/probe_train_graph_ranks.py times it on one GPU; main() prepares a model only at world > 1)
    want_graph = bool(getattr(args, "train_graph", 0))
    ranks = dist_on and not ddp and (train_ops.prepared_for_ranks(model) or (want_graph and world > 1))
    use_graph = want_graph and (world == 1 or ranks)
    if ranks and "exchange" not in graphed:
        # (ordered: None = summed in rank order exactly when the step is deterministic; args.exchange_ordered lets a probe choose)
        graphed["exchange"] = train_ops.GradExchange(model.parameters(), world, ordered=getattr(args, "exchange_ordered", None))
    end = time.time()
    for i, batch_data in enumerate(train_loader):
        q_frames, q_audio_wav, q_audio_eg, t_frames, t_audio_wav, t_audio_eg = batch_data
        q_frames, t_frames = to_cuda(q_frames), to_cuda(t_frames)
        q_audio_eg, t_audio_eg = q_audio_eg.cuda(), t_audio_eg.cuda()
        data_time.update(time.time() - end)

        batch_size = (q_frames[0] if isinstance(q_frames, list) else q_frames).shape[0]
        if use_graph:
            flat = (list(q_frames) if isinstance(q_frames, list) else [q_frames]) + (list(t_frames) if isinstance(t_frames, list) else [t_frames]) + \
                   [q_audio_eg, t_audio_eg]
            key = tuple((tuple(v.shape), v.dtype) for v in flat)
            ent = graphed.get(key)
            if ent is None:
                static = [v.clone() for v in flat]
                nq = len(q_frames) if isinstance(q_frames, list) else 0
                nt = len(t_frames) if isinstance(t_frames, list) else 0

                def device_step(static=static, nq=nq, nt=nt, batch_size=batch_size):
                    qf = static[:nq] if nq else static[0]
                    tf = static[max(nq, 1) : max(nq, 1) + nt] if nt else static[max(nq, 1)]
                    return _eager_step(model, optimizer, criterion, args, qf, tf, static[-2], static[-1], batch_size)

                if ranks:
                    ent = graphed[key] = (static, _graphed_ranks_step(model, optimizer, criterion, args, static, nq, nt, batch_size,
                                                                      graphed["exchange"]))
                elif isinstance(optimizer, train_ops.ArenaSGD):
                    # the warm-up steps train on this batch; put the state back afterwards, so that the first replay is the ONE step the
                    # batch takes (as in the eager loop and the reference).  The capture must start from stale weight planes — their
                    # re-make launch is then part of the graph and every replay splits the weights it finds — which the step hook of the
                    # last warm-up step leaves behind
                    saved = _snapshot(model, optimizer)
                    ent = graphed[key] = (static, train_ops.GraphedStep(device_step, static[0].device, warmup=2, before_capture=_stale_planes))
                    _restore(saved)
                    train_ops.invalidate_weight_cache()
                else:
                    ent = graphed[key] = (static, train_ops.GraphedStep(device_step, static[0].device, warmup=2))
                    # (the warm-up steps and the capture consumed this batch: three optimizer steps on it, like a first batch seen thrice)
            else:
                for dst, src in zip(ent[0], flat):
                    dst.copy_(src, non_blocking=True)
            if ranks:
                loss = ent[1]()  # (the rank's own loss, as under DistributedDataParallel)
                _exchange_and_step(optimizer, graphed["exchange"])
            else:
                if hasattr(optimizer, "sync_hyper"):
                    optimizer.sync_hyper()  # (the replay reads the learning rate from device memory: what the scheduler set since the last one)
                loss = ent[1]()
            losses.update(loss.item(), batch_size)
        else:
            if ranks:
                loss = _eager_ranks_step(model, optimizer, criterion, args, q_frames, t_frames, q_audio_eg, t_audio_eg, batch_size,
                                         graphed["exchange"])
            else:
                loss = _eager_step(model, optimizer, criterion, args, q_frames, t_frames, q_audio_eg, t_audio_eg, batch_size)
            losses.update(loss.item(), batch_size)

        batch_time.update(time.time() - end)
        end = time.time()
        if i % args.print_freq == 0:
            print("Epoch: [{0}][{1}/{2}]\t"
                  "Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t"
                  "Data {data_time.val:.3f} ({data_time.avg:.3f})\t"
                  "Loss {loss.val:.4f} ({loss.avg:.4f})".format(epoch, i, len(train_loader), batch_time=batch_time,
                                                                data_time=data_time, loss=losses))
        if tb_logger is not None and i % args.log_freq == 0:
            logs = OrderedDict()
            logs["Train_IterLoss"] = losses.val
            iter_count = epoch * len(train_loader) + i
            for key, value in logs.items():
                tb_logger.log_scalar(value, key, iter_count)
            tb_logger.flush()
    return losses.avg


def _stale_planes():
    """GraphedStep's before_capture check of a step whose weight planes the capture must re-make."""
    assert train_ops.weight_cache_is_stale(), "the capture would start from current weight planes: no re-make in the graph"


def _snapshot(model, optimizer):
    """Clones of everything a training step changes: parameters, the model's buffers (BatchNorm statistics, num_batches_tracked) and the
    optimizer's momentum buffers -> [(tensor, clone)]."""
    seen, out = set(), []
    tensors = list(model.parameters()) + list(model.buffers()) + [p for g in optimizer.param_groups for p in g["params"]] + \
        [v for st in optimizer.state.values() for v in st.values() if isinstance(v, torch.Tensor)]
    for t in tensors:
        if id(t) not in seen:
            seen.add(id(t))
            out.append((t, t.detach().clone()))
    return out


def _restore(saved):
    with torch.no_grad():
        torch._foreach_copy_([t.detach() for t, _ in saved], [c for _, c in saved])


def _stateless(optimizer):
    """The parameters the optimizer keeps no state for yet (torch's SGD creates its momentum buffers at the first step)."""
    return [p for g in optimizer.param_groups for p in g["params"] if p not in optimizer.state or not optimizer.state[p]]


def _exchange_and_step(optimizer, exchange):
    """The eager rest of a step across ranks: one all-reduce of the packed gradients, the optimizer on their views, stale weight planes."""
    exchange.all_reduce()
    exchange.install()
    if hasattr(optimizer, "sync_hyper"):
        optimizer.sync_hyper()
    optimizer.step()
    train_ops.invalidate_weight_cache()  # (optimizers that update through .data do not bump Tensor._version)


def _eager_ranks_step(model, optimizer, criterion, args, q_frames, t_frames, q_audio_eg, t_audio_eg, batch_size, exchange):
    """One step across ranks without a graph: forward and backward, the pack of the gradients, the exchange and the optimizer -> the
    rank's own loss.  What _graphed_ranks_step captures and what follows its replays, issued launch by launch."""
    loss = _forward_backward(model, optimizer, criterion, args, q_frames, t_frames, q_audio_eg, t_audio_eg, batch_size)
    if not exchange.bound:
        exchange.bind()  # (the first backward of the run: which parameters have gradients; one small collective)
    exchange.pack()
    _exchange_and_step(optimizer, exchange)
    return loss.detach()


def _graphed_ranks_step(model, optimizer, criterion, args, static, nq, nt, batch_size, exchange):
    """The captured part of a step across ranks for one batch shape -> train_ops.GraphedStep: stale weight planes, zero_grad, forward,
    loss, backward, and the pack of the gradients as the last launch.  Every rank meets a new shape at the same iteration
    (DistributedSampler + drop_last), so the collectives of the warm-up steps match."""

    def device_step():
        # the optimizer runs OUTSIDE this function: whatever ran since the last call, the weight planes are re-made here — and that
        # launch is part of the capture (a capture that found the cache current would replay convolutions on old planes)
        train_ops.invalidate_weight_cache()
        qf = static[:nq] if nq else static[0]
        tf = static[max(nq, 1) : max(nq, 1) + nt] if nt else static[max(nq, 1)]
        loss = _forward_backward(model, optimizer, criterion, args, qf, tf, static[-2], static[-1], batch_size)
        if not exchange.bound:
            exchange.bind()  # (the first backward of the run: which parameters have gradients; one small collective)
        exchange.pack()
        return loss.detach()

    # the warm-up steps are whole steps on this batch, exchange and optimizer included; the state goes back afterwards — with either
    # optimizer — so that the first replay is the ONE step the batch takes.  State the optimizer did not have yet (torch's SGD creates
    # its momentum buffers at the first step) is restored as absent
    saved, absent = _snapshot(model, optimizer), _stateless(optimizer)
    step = train_ops.GraphedStep(device_step, static[0].device, warmup=2, before_capture=_stale_planes,
                                 after_warmup=lambda: _exchange_and_step(optimizer, exchange))
    _restore(saved)
    for p in absent:
        optimizer.state.pop(p, None)
    train_ops.invalidate_weight_cache()
    return step


def _forward_backward(model, optimizer, criterion, args, q_frames, t_frames, q_audio_eg, t_audio_eg, batch_size):
    """zero_grad, forward (train.py:114-116), InfoNCE + CE, backward -> the loss tensor (with its graph freed)."""
    groups = getattr(args, "bn_replicas", 1)
    groups = batch_size if groups < 0 else groups
    if groups > 1 and batch_size % groups:  # (a short last batch: say so instead of changing the BatchNorm semantics silently)
        if not getattr(train, "_warned_groups", False):
            print("train(): --bn_replicas %d does not divide a batch of %d items: that batch is normalised as ONE group "
                  "(use a batch size the replicas divide, or drop_last)" % (groups, batch_size))
            train._warned_groups = True
        groups = 1
    with train_ops.bn_replicas(groups):
        output = model(q_frames, t_frames, q_audio_eg=q_audio_eg, t_audio_eg=t_audio_eg)  # train.py:114-116
    labels = torch.zeros(batch_size, dtype=torch.long, device=output.device)  # positives at column 0
    loss = criterion(output, labels).mean()
    optimizer.zero_grad()
    loss.backward()
    return loss


def _eager_step(model, optimizer, criterion, args, q_frames, t_frames, q_audio_eg, t_audio_eg, batch_size):
    """One optimizer step of train(): forward, loss, backward, step -> the loss tensor."""
    loss = _forward_backward(model, optimizer, criterion, args, q_frames, t_frames, q_audio_eg, t_audio_eg, batch_size)
    optimizer.step()
    train_ops.invalidate_weight_cache()  # (optimizers that update through .data do not bump Tensor._version)
    return loss.detach()
