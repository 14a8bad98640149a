"""Training-step kernels on the MI355X, as torch.autograd.Functions the SlowFast modules call in train mode
when the model is in the training layout (channels_last_3d, main.py --train_layout ndhwc):

* `bn_act`: train-mode BatchNorm3d + shortcut add + ReLU as one HIP statistics pass + one apply pass in each direction
  (csrc/bn_train.hip) instead of MIOpenBatchNormFwdTrainSpatial / BwdSpatial + separate add / ReLU passes;
* `conv3d` / `conv3d_fork`: the convolutions' forward and stride-1 input gradient on the split-plane MFMA kernel
  (csrc/conv_x3.hip, fp32 in / fp32 out) and their weight gradient on csrc/wgrad_x3.hip; the two stems ([kt,7,7] on the
  3-channel clip) on the patch-resident kernels (csrc/stem_conv.hip forward with fp32 output, csrc/stem_train.hip weight
  gradient, both in the pixel-pair form); the strided layers' input gradients as one stride-1 convolution of dY per residue
  class of the input position (`_dgrad_strided`).  No MIOpen convolution is left in the step.
  The 3D-ResNet modules (resnet3d.py) call the same entries: 3x3x3 / 1x1x1 convolutions at stride 1 and (2,2,2), the 7x7x7 stem on the
  generic route (conv_x3 on the clip zero-padded to 8 channels, its weight gradient as seven [1,7,7] slices of wgrad_x3: the
  patch-resident weight-gradient kernel would need 284 KB of LDS at kt = 7), `max_pool3d` for the stem's MaxPool3d(3, 2, 1).

ARITHMETIC (main.py --train_conv, set_conv_mode): "x3" (the default on the MI355X) computes every product from two 16-bit
planes with fp32 accumulation — forward in fp16 planes (2^-22 per product), input and weight gradients in bf16 planes (2^-16
per product, fp32's exponent range; fp32 atomics in the weight gradient, so its summation order is not fixed) — NOT bit-for-bit
the reference's fp32 (train.py:114-141); "fp32" leaves every convolution to MIOpen's fp32 kernels (what the reference runs)
and keeps only the fused BatchNorm passes.  tests/test_gpu_train_step.py bounds the loss / gradient deviation of "x3" from an
fp64 step by the deviation of the stock fp32 step.
Weight planes are cached per tensor (weight_planes.py: the cache, its validity rule and the four makers of planes) and re-made
when `weight._version` changes (optimizer.step(), load_state_dict, any in-place op on the parameter), after every optimizer
step of the process and after a GraphedStep's capture.  In-place updates through `.data` (EMA / momentum encoders,
`p.data.clamp_()`) do NOT bump that counter: call `invalidate_weight_cache()` after them (train.train() does after every
optimizer step).  The device job tables of the step's multi-tensor launches and the launch counters (CALLS) are job_tables.py's."""
import contextlib
import struct
import weakref

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, ops, weight_planes
from .job_tables import _PACK_JOB, _SGD_JOB, CALLS, _chunks, _JobTable, _pack_jobs  # noqa: F401  (CALLS: read as train_ops.CALLS)
from .ops import K, _p, _stream
from .weight_planes import _grouped_planes, _weight_planes, pack_plane_jobs  # noqa: F401  (pack_plane_jobs: tests/test_abi.py)

# Which passes of the training step run on the hand-written kernels.  Module constants (no environment switches since round 4);
# `set_conv_mode` (main.py --train_conv) is the user-facing switch, tests set some of these to 0 for the stock-op reference path.
_FUSED = 1          # train-mode BatchNorm (+ shortcut + ReLU) on csrc/bn_train.hip
_CONV_X3 = 1        # convolution forward / stride-1 input gradient on conv_x3 (fp32 I/O)
_WGRAD_X3 = 1       # weight gradient on csrc/wgrad_x3.hip
_DGRAD_S_X3 = 1     # strided input gradients as residue-class convolutions on conv_x3 (0: MIOpen's bwd_data)
_STEM_WGRAD_X3 = 1  # the stems' weight gradient on the hand-written kernels
_STEM_PATCH = 1     # the stems on the patch-resident kernels (0: conv_x3 + wgrad slices)
_FORK = 1           # the shortcut's gradient summed in the a-convolution's input-gradient epilogue
_EPI_STATS = 1      # BatchNorm forward statistics on the producing convolution's epilogue (round 5: no statistics pass over its output)
_EPI_BWD = 1        # BatchNorm backward statistics on the epilogue of the consuming convolution's input-gradient launch (round 5)


def set_conv_mode(mode):
    """"x3": convolutions of the training step on the split-plane MFMA kernels (see the module docstring for the precision);
    "fp32": MIOpen's fp32 convolutions (the reference's arithmetic).  -> the mode now in force."""
    global _CONV_X3, _WGRAD_X3
    if mode not in ("x3", "fp32"):
        raise ValueError("train_conv must be 'x3' or 'fp32', got %r" % (mode,))
    if mode == "fp32" and _DETERMINISTIC:
        raise _no_miopen_in_deterministic_mode()
    _CONV_X3 = _WGRAD_X3 = 1 if mode == "x3" else 0
    return mode


def conv_mode():
    return "x3" if _CONV_X3 else "fp32"


_DETERMINISTIC = 0  # weight gradients through the workspace + fixed-order reduction entries (include/avt.h); set_deterministic


def _no_miopen_in_deterministic_mode():
    return _lib.AvtError("deterministic training needs the hand-written convolutions (--train_conv x3): MIOpen's fp32 weight gradients "
                         "(--train_conv fp32) sum in an order that changes from run to run")


def set_deterministic(flag):
    """True: every weight gradient of the training step (_conv_wgrad in all its branches, the patch-resident stems, conv2d) is written as
    per-chunk partial tiles and summed by a second launch in a fixed order, so that — with the rest of the step free of atomics already —
    one process on one GPU with one build repeats a seed bit for bit.  The default (False) is the atomic path, unchanged.  -> the
    previous setting.  Raises AvtError with --train_conv fp32 in force (MIOpen's order is not ours to fix)."""
    global _DETERMINISTIC
    was = bool(_DETERMINISTIC)
    if flag and not (_CONV_X3 and _WGRAD_X3):
        raise _no_miopen_in_deterministic_mode()
    _DETERMINISTIC = 1 if flag else 0
    return was


def deterministic():
    return bool(_DETERMINISTIC)


def invalidate_weight_cache(drop=False):
    """Mark every cached set of weight planes stale (needed after in-place updates through `.data`, which `_version` does not see): the
    next lookup re-makes them — all of them in one launch.  drop=True forgets the entries themselves (tests that compare two ways of
    MAKING the planes)."""
    weight_planes.CACHE.invalidate(drop)


def weight_cache_is_stale():
    """True when no cached set of weight planes is current (every lookup re-makes its planes): the state a capture must start from
    for the re-make launch to be part of its graph."""
    return weight_planes.CACHE.is_stale()


def _rows(x):
    """(m, c) of a [B,C,T,H,W] tensor whose memory is channels-last rows [B*T*H*W, C]."""
    return x.numel() // x.shape[1], x.shape[1]


_WS_BYTES = {}


def _workspace(m, c, groups, device):
    """Scratch for the per-workgroup partial sums and the per-channel coefficients (sized by the library)."""
    n = _WS_BYTES.get((m, c, groups))
    if n is None:
        n = _lib.lib().avt_bn_train_ws_bytes(m, c, groups)
        if n < 0:
            raise ValueError("bn_train: %d rows x %d channels in %d groups is outside the kernel's domain" % (m, c, groups))
        _WS_BYTES[(m, c, groups)] = n
    return torch.empty(n, dtype=torch.uint8, device=device)


# Per-replica BatchNorm in one launch: inside `with bn_replicas(n):` every fused BatchNorm treats its batch as n equal groups of
# consecutive samples, each normalised with its own statistics — the n items of a batch as the reference's DataParallel replicas
# see them (main.py:420: one item per GPU at batch 8 on 8 GPUs) — so that a rank's items go through the encoders as ONE batch
# (convolutions over 8 x 16 clips instead of 8 launches over 16: the deep layers have 8 x the tiles) with unchanged arithmetic.
# Running statistics and num_batches_tracked take GROUP 0's update only: DataParallel keeps the buffer updates of the replica on
# device 0 and drops the other replicas' (their buffers are per-forward broadcast copies), so a checkpoint trained here carries the
# eval-mode statistics the reference's would (one momentum step per forward, from item 0).
_BN_GROUPS = 1


class bn_replicas:
    def __init__(self, n):
        self.n = int(n)

    def __enter__(self):
        global _BN_GROUPS
        self.keep, _BN_GROUPS = _BN_GROUPS, self.n
        return self

    def __exit__(self, *exc):
        global _BN_GROUPS
        _BN_GROUPS = self.keep
        return False


def fusable(x, bn, res=None):
    c = x.shape[1]
    return (_FUSED and bn.training and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and c >= 8 and (c & (c - 1)) == 0 and
            x.is_contiguous(memory_format=torch.channels_last_3d) and bn.weight is not None and bn.weight.dtype == torch.float32 and
            (res is None or (res.shape == x.shape and res.dtype == torch.float32 and
                             res.is_contiguous(memory_format=torch.channels_last_3d))))


# Concatenation without the copy (round 4).  SlowFast's lateral fusion is torch.cat([slow, lateral], 1): on channels-last tensors a
# strided copy of both operands forward and, backward, a .contiguous() of each gradient slice — 13 GB per config-5 step that no
# convolution needs.  Instead the two producers (the stage's last BatchNorm / the stem's max-pool, and the lateral's BatchNorm)
# write channel slices of ONE buffer: bn_act / max_pool_hw(cat_extra = e) allocate rows of c + e channels and return their first
# c as a view tagged `_avt_cat = (buffer, c)`; bn_act(cat_into = (buffer, offset)) fills the rest; join_channels hands out the
# buffer as the concatenation, and its backward hands each producer its slice of the gradient, which the kernels read through a
# leading dimension (avt_bn_train_bwd ld_dy).  Only the fused HIP paths set the tag: anything else keeps torch.cat.
_JOIN = 1  # (tests set 0: torch.cat and contiguous gradients, the same numbers)


def _cat_buffer(shape, c_total, device):
    b, _, t, h, w = shape
    return torch.empty((b, c_total, t, h, w), dtype=torch.float32, device=device, memory_format=torch.channels_last_3d)


def _alias(buf, c_off, c):
    """Channels c_off .. c_off + c of the buffer's rows as a tensor that SHARES the storage without being an autograd view of it
    (set_: a version counter of its own) — the producers fill the slices through raw pointers, and the view bookkeeping ("a view's
    base was modified in place") has nothing to say about tensors whose only writers are those kernels."""
    t = torch.empty(0, dtype=buf.dtype, device=buf.device)
    size = (buf.shape[0], c) + tuple(buf.shape[2:])
    return t.set_(buf.untyped_storage(), buf.storage_offset() + c_off, size, buf.stride())


def _row_ld(t):
    """Leading dimension of a [B,C,T,H,W] tensor that is channels-last ROWS with a constant row pitch (a channel slice of a
    channels-last tensor, or a contiguous one: pitch C), else None."""
    if t.dim() != 5 or t.dtype != torch.float32 or t.data_ptr() % 16:
        return None
    b, c, tt, h, w = t.shape
    st = t.stride()
    if c > 1 and st[1] != 1:
        return None
    ld = st[4] if w > 1 else (st[3] if h > 1 else (st[2] if tt > 1 else (st[0] if b > 1 else c)))
    want = (tt * h * w * ld, 1, h * w * ld, w * ld, ld)
    if any(n > 1 and s != e for n, s, e in zip(t.shape, st, want)) or ld < c or ld % 4:
        return None
    return ld


class _JoinChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, buf):
        ctx.c0 = a.shape[1]
        # INVARIANT: the slices and the joined tensor share storage OUTSIDE autograd's view tracking — their only
        # writers are the producing kernels, and nothing may modify them in place afterwards (an nn.ReLU(inplace=True) or `+=` on
        # one of them would corrupt the others' saved activations without autograd noticing).  The version counters are stamped
        # here and compared in backward, so that such an edit raises instead of training on garbage.
        out = _alias(buf, 0, buf.shape[1])  # the buffer both producers wrote, as a tensor of this node's own
        # (the joined tensor by weak reference: a strong one is the cycle out -> grad_fn -> ctx -> out, which only backward broke —
        #  a grad-enabled forward that is never backpropagated kept the whole buffer until the cyclic collector ran)
        ctx.stamp = ((a, a._version), (b, b._version))
        ctx.out_ref, ctx.out_version = weakref.ref(out), out._version
        return out

    @staticmethod
    def backward(ctx, d):
        out = ctx.out_ref()
        for t, v in ctx.stamp + (((out, ctx.out_version),) if out is not None else ()):
            if t._version != v:
                raise RuntimeError("train_ops.join_channels: a channel slice of the concatenation buffer (or the joined tensor) was "
                                   "modified in place after the join; the slices share storage outside autograd's view tracking")
        ctx.stamp = ctx.out_ref = None
        return d[:, : ctx.c0], d[:, ctx.c0 :], None


def join_channels(a, b):
    """torch.cat([a, b], 1) — without a copy when a and b are the two channel slices of one buffer (see above)."""
    ta, tb = getattr(a, "_avt_cat", None), getattr(b, "_avt_cat", None)
    if (ta is not None and tb is not None and ta[0] is tb[0] and ta[1] == 0 and tb[1] == a.shape[1] and
            ta[0].shape[1] == a.shape[1] + b.shape[1]):
        return _JoinChannels.apply(a, b, ta[0])
    return torch.cat([a, b], 1)


class _BnHandle:
    """What the input-gradient launch of the convolution that consumes a fused BatchNorm's output needs to know about it (the
    tensors are the ones the BatchNorm's own backward keeps: no extra memory).  Travels as `y._avt_bn` on the BatchNorm's output."""
    __slots__ = ("x", "mask", "weight", "bias", "mean", "invstd", "relu", "groups", "has_res", "c")

    def __init__(self, x, mask, weight, bias, mean, invstd, relu, groups, has_res):
        self.x, self.mask, self.weight, self.bias, self.mean, self.invstd = x, mask, weight, bias, mean, invstd
        self.relu, self.groups, self.has_res, self.c = bool(relu), int(groups), bool(has_res), x.shape[1]


_LAST_BN = None   # the handle of the last _BNAct.forward, for bn_act to tag its output with
_BWD_STATS = {}   # data_ptr of a masked output gradient -> (workspace, rows of partials, handle): written by the input-gradient
#                   launch (_conv_backward), consumed by that BatchNorm's backward a moment later; emptied at the next forward


class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, res, relu, momentum, eps, tracked=None, groups=1, cat=None, pre=None):
        m, c = _rows(x)
        if cat is None:
            y, ldy = torch.empty_like(x), 0  # keeps the channels-last strides
        else:  # (buffer, channel offset): the output is that slice of the concatenation buffer's rows
            y, ldy = _alias(cat[0], cat[1], c), cat[0].shape[1]
        save_mean = torch.empty(groups * c, dtype=torch.float32, device=x.device)
        save_invstd = torch.empty(groups * c, dtype=torch.float32, device=x.device)
        CALLS["bn_fwd"] += 1
        # ReLU with a shortcut: the mask leaves the apply pass as 4 bits per float4 chunk and is what the backward reads;
        # without a shortcut the backward recomputes it from x.  Either way the output is not read again, nor kept alive here
        mask = torch.empty(m * c // 4, dtype=torch.uint8, device=x.device) if (relu and res is not None) else None
        if pre is not None:  # (workspace, rows of partials per group): the producing convolution's epilogue has summed the rows
            ws, pre_rows = pre
            CALLS["bn_fwd_pre"] += 1
            K.avt_bn_train_fwd_pre(_p(x), _p(res), _p(y), m, c, _p(weight), _p(bias), float(eps), float(momentum), 1 if relu else 0,
                                   groups, _p(ws), ws.numel(), _p(save_mean), _p(save_invstd), _p(running_mean), _p(running_var),
                                   _p(tracked), _p(mask), ldy, int(pre_rows), _stream())
        else:
            ws = _workspace(m, c, groups, x.device)
            K.avt_bn_train_fwd(_p(x), _p(res), _p(y), m, c, _p(weight), _p(bias), float(eps), float(momentum), 1 if relu else 0, groups,
                               _p(ws), ws.numel(), _p(save_mean), _p(save_invstd), _p(running_mean), _p(running_var), _p(tracked),
                               _p(mask), ldy, _stream())
        ctx.save_for_backward(x, mask, weight, bias, save_mean, save_invstd)
        ctx.has_res = res is not None
        ctx.relu = bool(relu)
        ctx.groups = groups
        global _LAST_BN
        if _BWD_STATS:
            _BWD_STATS.clear()  # (left-overs of a backward pass whose BatchNorm did not pick them up)
        ctx.handle = _LAST_BN = _BnHandle(x, mask, weight, bias, save_mean, save_invstd, relu, groups, res is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mask, weight, bias, save_mean, save_invstd = ctx.saved_tensors
        m, c = _rows(x)
        pre = _BWD_STATS.pop(dy.data_ptr(), None) if _BWD_STATS else None
        # (autograd frees saved_tensors after backward but never ctx.__dict__ — the handle holds x and the mask, so it
        #  is dropped here, before anything else can keep the node alive through the next step's forward)
        handle, ctx.handle = ctx.handle, None
        # (valid only for the very tensor the launch wrote: autograd sums gradients that reach a tensor by several paths — into a
        #  new tensor, or IN PLACE into one of them, which the version counter shows; a summed gradient takes the plain passes
        #  below, where masking an already masked part again changes nothing)
        if (pre is not None and pre[2] is handle and dy._version == pre[3] and dy.shape == x.shape and dy.dtype == torch.float32 and
                dy.is_contiguous(memory_format=torch.channels_last_3d)):
            # dy is ALREADY g = mask * dz, and its producer (the input-gradient launch of the convolution that consumed this
            # BatchNorm's output) left the sums of g and g * xhat behind: finalize + apply; the shortcut's gradient is g itself
            dx = torch.empty_like(x)
            dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
            dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
            CALLS["bn_bwd"] += 1
            CALLS["bn_bwd_pre"] += 1
            K.avt_bn_train_bwd_pre(_p(dy), _p(x), m, c, _p(weight), _p(save_mean), _p(save_invstd), ctx.groups, _p(pre[0]),
                                   pre[0].numel(), int(pre[1]), _p(dx), _p(dgamma), _p(dbeta), _stream())
            return dx, dgamma, dbeta, None, None, (dy if ctx.has_res else None), None, None, None, None, None, None, None
        ld_dy = _row_ld(dy)  # a slice of a concatenation's gradient is read in place (rows with a pitch)
        if ld_dy is None:
            dy, ld_dy = dy.contiguous(memory_format=torch.channels_last_3d), c
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if ctx.has_res else None
        ws = _workspace(m, c, ctx.groups, x.device)
        dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
        CALLS["bn_bwd"] += 1
        K.avt_bn_train_bwd(_p(dy), None, _p(x), m, c, _p(weight), _p(bias), _p(save_mean), _p(save_invstd), 1 if ctx.relu else 0,
                           ctx.groups, _p(mask), _p(ws), ws.numel(), _p(dx), _p(dres), _p(dgamma), _p(dbeta), ld_dy, _stream())
        return dx, dgamma, dbeta, None, None, dres, None, None, None, None, None, None, None


def bn_act(x, bn, res=None, relu=True, cat_extra=0, cat_into=None):
    """act(bn(x) [+ res]) for a BatchNorm3d module `bn`: the fused HIP pass in train mode on channels-last fp32 device tensors,
    the stock torch ops otherwise (eval mode, other layouts / dtypes, CPU) — same result, same running-statistics update.
    Inside `bn_replicas(n)` the batch is n groups with statistics of their own (the stock path: a loop over the groups).
    cat_extra = e / cat_into = (buffer, offset): the output is the first / a later channel slice of a concatenation buffer
    (join_channels; fused path only — the stock path returns a tensor of its own and the caller's join falls back to torch.cat)."""
    groups = _BN_GROUPS if (bn.training and _BN_GROUPS > 1) else 1
    if groups > 1 and x.shape[0] % groups:
        raise ValueError("bn_replicas(%d): a batch of %d samples does not split into the replicas" % (groups, x.shape[0]))
    if not fusable(x, bn, res):
        if groups > 1:  # per-replica statistics on the stock ops: one BatchNorm call per group; running statistics from group 0
            # only (DataParallel keeps the buffer updates of the replica on device 0 alone, reference main.py:420)
            xs = x.chunk(groups, 0)
            y = torch.cat([bn(xs[0])] + [F.batch_norm(xg, None, None, bn.weight, bn.bias, True, 0.0, bn.eps) for xg in xs[1:]], 0)
        else:
            y = bn(x)
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y
    momentum = bn.momentum
    tracked = bn.num_batches_tracked if bn.track_running_stats else None
    if tracked is not None and momentum is None:  # cumulative moving average: the factor needs the count on the host
        if groups > 1:
            raise ValueError("bn_replicas: BatchNorm with momentum=None (cumulative average) is not supported in groups")
        tracked.add_(1)
        momentum = 1.0 / float(tracked)
        tracked = None
    # (otherwise num_batches_tracked is incremented by the statistics kernel itself: a launch per BatchNorm and pass less)
    rm, rv = (bn.running_mean, bn.running_var) if bn.track_running_stats else (None, None)
    cat = None
    if not _JOIN:
        pass
    elif (cat_into is not None and cat_into[0].shape[1] >= cat_into[1] + x.shape[1] and cat_into[0].shape[0] == x.shape[0] and
            cat_into[0].shape[2:] == x.shape[2:]):
        cat = cat_into
    elif cat_extra:
        cat = (_cat_buffer(x.shape, x.shape[1] + int(cat_extra), x.device), 0)
    # statistics the producing convolution left behind (conv3d(..., stats=bn)): valid for exactly this BatchNorm geometry
    pre = getattr(x, "_avt_stats", None)
    if pre is not None and (pre[2] != groups or pre[3] != x.shape[1]):
        pre = None
    y = _BNAct.apply(x, bn.weight, bn.bias, rm, rv, res, relu, 0.0 if momentum is None else momentum, bn.eps, tracked, groups, cat,
                     None if pre is None else pre[:2])
    if cat is not None:
        y._avt_cat = cat
    global _LAST_BN
    if _LAST_BN is not None and _EPI_BWD and cat is None:
        y._avt_bn = _LAST_BN  # (the convolution that consumes y hands it to its input-gradient launch: conv3d / conv3d_fork)
    _LAST_BN = None
    return y


# ------------------------------------------------------------------------------------------------------------------------
# One training step as a replayed HIP graph (round 6).  Config 5 on 8 GPUs gives every rank ONE item (16 clips) per step: ~3000
# launches whose device time is below the host's time to issue them — the host never waits for the device in that step
# (profiles/r06/train_host_bound_one_item.log: 65 ms per step, 0.05 s of device waits in 4 s).  Every launch of the step goes to
# torch's current stream (the C ABI takes the stream), autograd replays the backward on the forward's streams, the side streams
# fork from and join the capturing stream by events, and no tensor of the step is read on the host — so the whole device side of a
# step (sample + pack, forward, loss, backward, optimizer, weight planes) is capturable as it stands.
class GraphedStep:
    """step_fn() -> tensor (e.g. the loss): run `warmup` times eagerly on a side stream, then captured ONCE; every call replays the
    graph and returns the same (graph-owned) result tensor.  Inputs must be STATIC tensors that step_fn closes over (fill them with
    copy_ before each call); anything the host decides inside step_fn (branches, cache lookups, shapes) is frozen at capture."""

    def __init__(self, step_fn, device, warmup=3, before_capture=None, after_warmup=None):
        self.graph, self.out = None, None
        # after_warmup: the eager rest of a step whose capture ends early (train() across ranks: exchange + optimizer), run after every
        # warm-up call of step_fn on that call's stream, never captured
        after = after_warmup if after_warmup is not None else (lambda: None)
        # warm-up and capture run on ONE stream of this object: the step's side streams are chosen per step stream
        # (models._side_stream), and a capture stream that differs from the warm-up's was handed the fast pathway's side stream for
        # its query encoder — two of the graph's three branches on one stream: 65 ms per one-item step instead of 52
        # (profiles/r06/graph_stream_order.log)
        # The first warm-up steps run eagerly on the CALLER's stream, the last one on the capture stream: the step's side streams of
        # the caller's stream exist before the capture stream and its own side streams are created.  Measured, not understood
        # (profiles/r06/graph_stream_order.log, ..._fixed.log): with the capture stream as the process's FIRST stream the replayed
        # one-item step takes 76 ms, after an eager step on the default stream 53 ms — the graph's parallel branches land on other
        # hardware queues
        for _ in range(max(warmup - 1, 0)):
            step_fn()
            after()
        torch.cuda.synchronize(device)
        self.stream = torch.cuda.Stream(device=device)
        self.stream.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(self.stream):
            if warmup > 0:
                step_fn()
                after()
        torch.cuda.current_stream(device).wait_stream(self.stream)
        torch.cuda.synchronize(device)
        if before_capture is not None:  # (the caller's checks of the state the capture starts from: train() with an ArenaSGD)
            before_capture()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.stream):
            self.out = step_fn()
        self.graph = g
        # the capture's lookups marked weight planes current and recorded their refresh event although nothing ran
        weight_planes.CACHE.capture_ended(device)

    def __call__(self):
        self.graph.replay()
        return self.out


# ------------------------------------------------------------------------------------------------------------------------
# SGD whose hyper-parameters live in device memory (csrc/sgd.hip): the optimizer of a step replayed as a HIP graph.  torch's SGD
# (fused or multi-tensor) takes the learning rate as a kernel ARGUMENT, which a capture freezes: after scheduler.step() every replay
# kept applying the first epoch's rate.  Here the rate is a load from `hyper`, which sync_hyper() rewrites outside the graph.
def pack_sgd_jobs(recs):
    """recs: (p, g, buf, numel, group) per parameter — addresses as ints, buf 0 without momentum -> (AvtSgdJob table as bytes,
    blk2job int32 array, blocks): job n owns ceil(numel / 4096) consecutive blocks from its blk0 (include/avt.h)."""
    return _pack_jobs(recs, lambda r: _chunks(r[3]),
                      lambda r, b0: struct.pack(_SGD_JOB, r[0], r[1], r[2], int(r[3]), int(r[4]), b0))


def _same_layout(a, b):
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)


class ArenaSGD(torch.optim.Optimizer):
    """torch.optim.SGD's update (momentum, weight decay, Nesterov; dampening 0) as ONE launch over all parameters
    (ops.sgd_multi: a device table of jobs, one per parameter with a gradient), its hyper-parameters read from a device tensor:
    a step captured in a HIP graph follows `param_groups` — StepLR, a hand-set rate — once sync_hyper() has run (eager step()
    calls it; train() does before every replay).  A torch.optim.Optimizer: schedulers, state_dict() (interchangeable with
    torch.optim.SGD's: `momentum_buffer` per parameter) and the process-wide step hook of the weight-plane cache work unchanged.
    Parameters: fp32, on the device, contiguous (in torch's default or the channels-last format), not sparse."""

    def __init__(self, params, lr, momentum=0, weight_decay=0, nesterov=False, dampening=0, maximize=False):
        self._hyper_dev, self._hyper_host = None, None
        self._jobs = _JobTable("ArenaSGD.step()", _SGD_JOB, ops.sgd_job_bytes, remedy="sync_hyper() or step()")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize)
        super().__init__(params, defaults)
        self._check_groups()
        with torch.no_grad():
            for group in self.param_groups:
                if group["momentum"] != 0:
                    for p in group["params"]:
                        self._buffer(p)
        if self.param_groups[0]["params"][0].is_cuda:
            self.sync_hyper()

    @staticmethod
    def _check_param(p):
        if not isinstance(p, torch.Tensor) or not p.is_cuda:
            raise _lib.AvtError("ArenaSGD: parameters must be device (HIP) tensors; the optimizer has no CPU path")
        if p.is_sparse or p.layout != torch.strided:
            raise _lib.AvtError("ArenaSGD: sparse parameters are not supported")
        if p.dtype != torch.float32:
            raise _lib.AvtError("ArenaSGD: parameters must be fp32, got %s" % p.dtype)
        dense = p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last)) or \
            (p.dim() == 5 and p.is_contiguous(memory_format=torch.channels_last_3d))
        if not dense:
            raise _lib.AvtError("ArenaSGD: parameters must be contiguous (torch's default or the channels-last format); got shape %s "
                                "strides %s" % (tuple(p.shape), tuple(p.stride())))

    def _check_groups(self):
        for group in self.param_groups:
            if group.get("dampening", 0) != 0:
                raise _lib.AvtError("ArenaSGD: dampening must be 0 (a zero-initialised buffer then gives torch's first-step rule)")
            if group.get("maximize", False):
                raise _lib.AvtError("ArenaSGD: maximize is not supported")
            if group["nesterov"] and group["momentum"] <= 0:
                raise _lib.AvtError("ArenaSGD: Nesterov momentum needs momentum > 0")
            if group["lr"] < 0 or group["momentum"] < 0 or group["weight_decay"] < 0:
                raise _lib.AvtError("ArenaSGD: lr, momentum and weight_decay must be >= 0")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            self._check_param(p)
        if self._hyper_host is not None:  # (after construction: the next sync_hyper() uploads a table with the new group's row)
            self._check_groups()
            self._jobs.keep_alive(self._hyper_dev)  # (a captured step may still read it)
            self._jobs.unreserve()  # (sized for the groups so far)
            self._hyper_dev, self._hyper_host = None, None

    def _blocks(self):
        """Per job of the table over ALL parameters: the largest a captured step() may build (what _JobTable.reserve sizes for)."""
        return (_chunks(p.numel()) for g in self.param_groups for p in g["params"])

    def _buffer(self, p):
        buf = self.state[p].get("momentum_buffer")
        if buf is None:
            if p.is_cuda and torch.cuda.is_current_stream_capturing():
                raise _lib.AvtError("ArenaSGD.step() under stream capture: a momentum buffer is missing (set the momentum before the capture)")
            buf = self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return buf

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """torch's load_state_dict (torch.optim.SGD's state is interchangeable), after which every momentum buffer again has its
        parameter's layout: a buffer that came back from a checkpoint with other strides (a channels-last weight's went through the host)
        is copied into one that has them, so that step() finds what it checks for.  The job table is built anew (new addresses)."""
        super().load_state_dict(state_dict)
        self._check_groups()
        for group in self.param_groups:
            for p in group["params"]:
                buf = self.state[p].get("momentum_buffer") if p in self.state else None
                if buf is None:
                    continue
                if buf.dtype != torch.float32 or buf.device != p.device or not _same_layout(buf, p):
                    if tuple(buf.shape) != tuple(p.shape):
                        raise _lib.AvtError("ArenaSGD.load_state_dict(): a momentum buffer of shape %s for a parameter of shape %s"
                                            % (tuple(buf.shape), tuple(p.shape)))
                    new = torch.zeros_like(p, memory_format=torch.preserve_format)
                    new.copy_(buf)
                    self.state[p]["momentum_buffer"] = new
        self._jobs.forget()

    def sync_hyper(self):
        """Make the device copy of (lr, momentum, weight_decay, nesterov) per group equal `param_groups`: one small host-to-device copy
        on the current stream when they differ from what was last uploaded (after scheduler.step(), once per epoch), nothing otherwise.
        -> True when it copied.  Not under stream capture: a replay must see the values the host set AFTER the capture."""
        vals = tuple((float(g["lr"]), float(g["momentum"]), float(g["weight_decay"]), 1.0 if g["nesterov"] else 0.0)
                     for g in self.param_groups)
        if self._hyper_dev is not None and vals == self._hyper_host:
            return False
        if torch.cuda.is_current_stream_capturing():
            raise _lib.AvtError("ArenaSGD.sync_hyper() under stream capture: call it before the capture / between replays")
        self._check_groups()
        self._jobs.reserve(self._blocks())
        device = self.param_groups[0]["params"][0].device
        host = torch.tensor(vals, dtype=torch.float32).pin_memory()  # (a new pinned tensor per change: an earlier copy may be in flight)
        if self._hyper_dev is None:
            self._hyper_dev = torch.empty((len(vals), 4), dtype=torch.float32, device=device)
        self._hyper_dev.copy_(host, non_blocking=True)
        self._hyper_host = vals
        return True

    @staticmethod
    def _pack(key, keep):
        """What _JobTable.get packs a NEW table with: the tensors behind the addresses checked first."""
        for p, g, buf in keep:
            if g.dtype != torch.float32 or g.device != p.device or g.layout != torch.strided or not _same_layout(g, p):
                raise _lib.AvtError("ArenaSGD.step(): a gradient must be an fp32 device tensor with its parameter's strides; got %s %s "
                                    "strides %s for a parameter with strides %s" % (g.dtype, g.device, tuple(g.stride()), tuple(p.stride())))
            if buf is not None and (buf.dtype != torch.float32 or buf.device != p.device or not _same_layout(buf, p)):
                raise _lib.AvtError("ArenaSGD.step(): a momentum buffer must be an fp32 device tensor with its parameter's strides")
        return pack_sgd_jobs(key)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.sync_hyper()  # (while capturing no hyper-parameter is uploaded: the graph reads what the host copies between replays)
            self._jobs.reserve(self._blocks())
        elif self._hyper_dev is None:
            raise _lib.AvtError("ArenaSGD.step() under stream capture before any sync_hyper()")
        key, keep = [], []
        for gi, group in enumerate(self.param_groups):
            mom = group["momentum"] != 0
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue  # (torch's rule: no gradient, no update — the momentum buffer stays as it is)
                buf = self._buffer(p) if mom else None
                key.append((p.data_ptr(), g.data_ptr(), buf.data_ptr() if buf is not None else 0, p.numel(), gi))
                keep.append((p, g, buf))
        if not key:
            return loss
        key = tuple(key)
        tab = self._jobs.get(key, keep[0][0].device, lambda: self._pack(key, keep))
        ops.sgd_multi(tab.jobs, tab.blk2job, tab.blocks, self._hyper_dev)
        CALLS["sgd_multi"] += 1
        return loss


# ------------------------------------------------------------------------------------------------------------------------
# The gradient exchange of a step that every rank replays as a HIP graph (train.train() at world > 1 with --train_graph 1).
# DistributedDataParallel's bucketed all-reduce is not capturable as it stands, and its hooks issue from the host.  Here the capture
# ends with ONE launch (csrc/grad_pack.hip) that copies every gradient, times 1 / world, into one flat buffer; the ranks all-reduce
# that buffer OUTSIDE the graph and the optimizer — any optimizer — steps on views of it.
# The ORDERED exchange (deterministic mode) replaces the all-reduce, whose order of summation is the backend's, by data movement and a sum
# of our own: one all-gather of the buffers into parts [world][total] and ONE launch (csrc/rank_sum.hip) that adds the rows in ascending
# rank order — every rank computes the same fp32 chain, so the ranks stay bit-identical and a seed repeats across ranks.  Its cost: the
# gather receives world x 4 * total bytes per rank where an all-reduce moves about 2 x 4 * total, `parts` takes world x 4 * total bytes
# of HBM (world x 269 MB on config 5), and the sum reads and writes (world + 1) x 4 * total bytes.
def exchange_layout(numels):
    """-> (offsets, total) in floats: tensor k of `numels` starts at a multiple of 4 floats (16 bytes, as _GradArena.take slices),
    total = sum of ceil4(numel)."""
    offsets, total = [], 0
    for n in numels:
        offsets.append(total)
        total += (int(n) + 3) // 4 * 4
    return offsets, total


def pack_grad_jobs(recs):
    """recs: (src, dst, numel) per gradient — addresses as ints -> (AvtPackJob table as bytes, blk2job int32 array, blocks): job n
    owns ceil(numel / 4096) consecutive blocks from its blk0 (include/avt.h)."""
    return _pack_jobs(recs, lambda r: _chunks(r[2]), lambda r, b0: struct.pack(_PACK_JOB, r[0], r[1], int(r[2]), b0, 0))


class GradExchange:
    """The mean gradient over `world` ranks through ONE flat fp32 buffer:

        ex = GradExchange(model.parameters(), world)
        loss.backward(); ex.bind()        # once, after the first backward: which parameters have gradients
        ex.pack()                         # one launch: flat views = grad * (1 / world)   — capturable, the graph's last node
        ex.all_reduce(); ex.install()     # eager: one all-reduce (sum), then p.grad = the parameter's view of the buffer
        optimizer.step()

    ordered=True (None: what deterministic() says when bind() runs): all_reduce() is exchange() — one all-gather of the ranks' buffers
    into `parts` [world][ceil4(total)] and one launch of ops.rank_sum that adds them in ascending rank order into `flat`: only data
    movement crosses the ranks, and `flat` holds the same bits on every rank.  The 1 / world scale stays in pack().

    `flat` holds parameter k at exchange_layout's offset, through a view with the PARAMETER's strides (a channels-last weight's view is
    an as_strided one: the same memory order as its gradient, so the pack is a flat copy); the padding between tensors stays zero.
    `scale` is a device tensor the kernel loads: a replay follows what the host last wrote there."""

    def __init__(self, params, world, group=None, ordered=None):
        self.candidates = [p for p in params if p.requires_grad]
        if not self.candidates:
            raise _lib.AvtError("GradExchange: no parameter requires a gradient")
        self.world, self.group = int(world), group
        if self.world < 1:
            raise _lib.AvtError("GradExchange: world must be >= 1, got %d" % self.world)
        self.params, self.views, self.flat, self.offsets, self.total = None, None, None, None, 0
        self.ordered, self.parts, self._parts_host = ordered, None, None
        self.scale = torch.full((1,), 1.0 / self.world, dtype=torch.float32, device=self.candidates[0].device)
        self._jobs = _JobTable("GradExchange.pack()", _PACK_JOB, ops.pack_job_bytes, remedy="pack()")

    @property
    def bound(self):
        return self.params is not None

    def bind(self):
        """After the first backward: the exchanged set is the parameters whose .grad is not None, in the order given.  Allocates the
        flat buffer and the views, and checks ONCE that every rank exchanges the same number of tensors and floats."""
        if torch.cuda.is_current_stream_capturing():
            raise _lib.AvtError("GradExchange.bind() under stream capture: bind after the first eager backward")
        params = [p for p in self.candidates if p.grad is not None and p.numel() > 0]
        if not params:
            raise _lib.AvtError("GradExchange.bind(): no parameter has a gradient (call it after backward)")
        for p in params:
            ArenaSGD._check_param(p)
        offsets, total = exchange_layout([p.numel() for p in params])
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            # (MAX of (x, -x): the largest and the smallest of both figures in one collective; host integers under gloo)
            host = dist.get_backend(self.group) == "gloo"
            t = torch.tensor([len(params), total, -len(params), -total], dtype=torch.int64, device="cpu" if host else params[0].device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
            hi_n, hi_t, lo_n, lo_t = (int(v) for v in t.cpu())
            if hi_n != -lo_n or hi_t != -lo_t:
                raise _lib.AvtError("GradExchange.bind(): the ranks do not exchange the same gradients: %d..%d tensors, %d..%d floats "
                                    "(this rank: %d, %d)" % (-lo_n, hi_n, -lo_t, hi_t, len(params), total))
        self.flat = torch.zeros(max(total, 4), dtype=torch.float32, device=params[0].device)
        self.views = [torch.as_strided(self.flat, tuple(p.shape), tuple(p.stride()), o) for p, o in zip(params, offsets)]
        self.params, self.offsets, self.total = params, offsets, total
        if self.ordered is None:
            self.ordered = deterministic()
        if self.ordered:  # (total is a sum of ceil4s: rows of `parts` start 16-byte aligned)
            self.parts = torch.empty((self.world, self.flat.numel()), dtype=torch.float32, device=self.flat.device)
        self._jobs.reserve(_chunks(p.numel()) for p in params)  # (outside any capture: what a captured pack() stages its table in)

    @torch.no_grad()
    def pack(self):
        """views[k] = params[k].grad * scale for every bound parameter, in one launch on the current stream."""
        if not self.bound:
            raise _lib.AvtError("GradExchange.pack() before bind()")
        if not torch.cuda.is_current_stream_capturing():
            self._jobs.reserve(_chunks(p.numel()) for p in self.params)
        # a parameter outside the bound set that gains a gradient later (another batch shape, a plugin encoder's branch) would be stepped
        # on its local gradient and the ranks would drift apart silently
        bound = {id(p) for p in self.params}
        for p in self.candidates:
            if id(p) not in bound and p.grad is not None and p.numel() > 0:
                raise _lib.AvtError("GradExchange.pack(): a parameter of shape %s has a gradient now but had none at bind(): it is not "
                                    "exchanged (the set of trained parameters must not change between steps)" % (tuple(p.shape),))
        key = []
        for p, v in zip(self.params, self.views):
            g = p.grad
            if g is None:
                raise _lib.AvtError("GradExchange.pack(): a bound parameter has no gradient in this step (shape %s)" % (tuple(p.shape),))
            if g.dtype != torch.float32 or g.device != v.device or g.layout != torch.strided or not _same_layout(g, p):
                raise _lib.AvtError("GradExchange.pack(): a gradient must be an fp32 device tensor with its parameter's strides; got %s %s "
                                    "strides %s for a parameter with strides %s" % (g.dtype, g.device, tuple(g.stride()), tuple(p.stride())))
            if g.data_ptr() == v.data_ptr():
                raise _lib.AvtError("GradExchange.pack(): a gradient still IS its exchange view (the step accumulated into the installed "
                                    "gradient: zero the gradients with set_to_none=True)")
            key.append((g.data_ptr(), v.data_ptr(), p.numel()))
        key = tuple(key)
        tab = self._jobs.get(key, self.flat.device, lambda: pack_grad_jobs(key))
        ops.grad_pack_multi(tab.jobs, tab.blk2job, tab.blocks, self.scale)
        CALLS["grad_pack_multi"] += 1

    def all_reduce(self):
        """The sum over the ranks of the packed buffer, one collective on the current stream (the scale made it the mean); ordered:
        exchange()."""
        import torch.distributed as dist
        if not self.bound:
            raise _lib.AvtError("GradExchange.all_reduce() before bind()")
        if self.ordered:
            return self.exchange()
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.flat, group=self.group)
        elif self.world > 1:
            raise _lib.AvtError("GradExchange.all_reduce(): world %d without an initialised process group" % self.world)

    def exchange(self):
        """The ordered sum: all_gather_into_tensor(parts, flat) — row r of `parts` is rank r's buffer — then flat = the rows added in
        ascending rank order by one launch (ops.rank_sum).  Eager, on the current stream.  Under a gloo group (ranks that share one GPU)
        the gather is staged through the host, as dist.all_gather_rows does; under RCCL it runs on the device tensors.  Without a
        process group (world 1) `parts` is the buffer itself, copied on the device."""
        import torch.distributed as dist
        if not self.bound:
            raise _lib.AvtError("GradExchange.exchange() before bind()")
        if not self.ordered:
            raise _lib.AvtError("GradExchange.exchange(): this exchange was made unordered (ordered=False): use all_reduce()")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.AvtError("GradExchange.exchange() under stream capture: the gather and the sum follow the replay eagerly")
        if dist.is_available() and dist.is_initialized():
            if dist.get_world_size(self.group) != self.world:
                raise _lib.AvtError("GradExchange.exchange(): made for world %d, the process group has %d ranks"
                                    % (self.world, dist.get_world_size(self.group)))
            if dist.get_backend(self.group) == "gloo":
                if self._parts_host is None:
                    self._parts_host = torch.empty(self.parts.shape, dtype=torch.float32)
                # (the output as ONE flat vector, rank r's buffer at r * total: gloo takes no [world, total] output for a [total] input)
                dist.all_gather_into_tensor(self._parts_host.view(-1), self.flat.cpu(), group=self.group)
                self.parts.copy_(self._parts_host)
            else:
                dist.all_gather_into_tensor(self.parts.view(-1), self.flat, group=self.group)
        elif self.world > 1:
            raise _lib.AvtError("GradExchange.exchange(): world %d without an initialised process group" % self.world)
        else:
            self.parts[0].copy_(self.flat)
        ops.rank_sum(self.parts, self.flat)
        CALLS["rank_sum"] += 1

    def install(self):
        """p.grad = the parameter's view of the exchange buffer: whatever optimizer steps next steps on the mean gradient, and on the
        same addresses every step (ArenaSGD builds its table once)."""
        if not self.bound:
            raise _lib.AvtError("GradExchange.install() before bind()")
        for p, v in zip(self.params, self.views):
            p.grad = v


def prepared_for_ranks(model):
    """True for a model that went through prepare_ranks()."""
    return bool(model.__dict__.get("_avt_prepared_for_ranks", False))


def freeze_checkpoint_only_modules(model):
    """Modules that exist only so reference checkpoints load by key and are never applied — q_a_mlp / t_a_mlp (models.py:267-284)
    and VGGish's fc stack (vggish.py:45) — take no gradient: nothing waits for or exchanges ~300 M dead parameters."""
    from .vggish import VGGish
    for name in ("q_a_mlp", "t_a_mlp"):
        if hasattr(model, name):
            getattr(model, name).requires_grad_(False)
    for name in ("q_a_encoder", "t_a_encoder"):
        enc = getattr(model, name, None)
        if isinstance(enc, VGGish) and hasattr(enc, "fc"):
            enc.fc.requires_grad_(False)
    return model


def prepare_ranks(model, group=None):
    """A model for train()'s step across ranks through GradExchange (replayed as a graph with --train_graph 1, eager without; main()
    prepares it for --train_graph 1 and for --train_deterministic), in place of the DistributedDataParallel wrapper: the checkpoint-only modules
    frozen, then every parameter and buffer broadcast from rank 0 ONCE (afterwards the ranks apply the same all-reduced gradient to the
    same weights; BatchNorm buffers stay per rank and rank 0 writes the checkpoint).  -> the model itself, unwrapped."""
    import torch.distributed as dist
    freeze_checkpoint_only_modules(model)
    world = 1
    if dist.is_available() and dist.is_initialized():
        world = dist.get_world_size(group)
        src = dist.get_global_rank(group, 0) if group is not None else 0
        with torch.no_grad():
            for t in list(model.parameters()) + list(model.buffers()):
                dist.broadcast(t.data, src=src, group=group)
    model.__dict__["_avt_prepared_for_ranks"] = True
    if world == 1 or dist.get_rank(group) == 0:
        print("prepare_ranks: %d rank(s), %d parameters and %d buffers broadcast from rank 0; gradients through train_ops.GradExchange, "
              "no DistributedDataParallel wrapper" % (world, len(list(model.parameters())), len(list(model.buffers()))))
    return model


# ------------------------------------------------------------------------------------------------------------------------
# The training state off the loop's critical path (main.py --ckpt_async, checkpoint.AsyncCheckpointWriter).  An epoch-end checkpoint
# that calls torch.save on device tensors copies them to the host one by one, synchronously, and serialises them while every rank
# waits.  Here the state leaves the training stream in ONE launch (csrc/state_copy.hip: every tensor into one flat device buffer) and
# one device-to-host copy on a stream of its own into pinned memory; a host thread does the rest.
_STATE_CHUNK = 16384  # bytes per block (csrc/state_copy.hip kChunk)
_STATE_JOB = "<2Qq2i"  # AvtStateJob (include/avt.h)


def state_layout(nbytes_list):
    """-> (offsets, total) in bytes: tensor k of `nbytes_list` starts at a multiple of 16 bytes, total = sum of ceil16(nbytes).  A
    zero-size tensor takes no room (its offset is the next tensor's)."""
    offsets, total = [], 0
    for n in nbytes_list:
        offsets.append(total)
        total += (int(n) + 15) // 16 * 16
    return offsets, total


def pack_state_jobs(recs):
    """recs: (src, dst, nbytes) per tensor — addresses as ints, nbytes > 0 -> (AvtStateJob table as bytes, blk2job int32 array, blocks):
    job n owns ceil(nbytes / 16384) consecutive blocks from its blk0 (include/avt.h)."""
    return _pack_jobs(recs, lambda r: (int(r[2]) + _STATE_CHUNK - 1) // _STATE_CHUNK,
                      lambda r, b0: struct.pack(_STATE_JOB, r[0], r[1], int(r[2]), b0, 0))


def _dense_in_storage_order(t):
    """True when the tensor's elements fill numel * itemsize consecutive bytes from data_ptr(), each once (contiguous in torch's default
    format, channels-last, or any permutation of one: what ArenaSGD._check_param accepts and more; a strided or expanded view is not)."""
    expect = 1
    for size, stride in sorted(((n, s) for n, s in zip(t.shape, t.stride()) if n > 1), key=lambda v: v[1]):
        if stride != expect:
            return False
        expect *= size
    return True


class SnapshotHandle:
    """One taken snapshot: wait() blocks the calling host thread until the copy into the pinned buffer has finished and -> {name: CPU
    view into that buffer} (shape, dtype and strides of the device tensor); release() hands the buffer back to the StateSnapshot (the
    views are dead from then on: clone what must outlive it)."""

    def __init__(self, owner, slot, event):
        import threading
        self._owner, self._slot, self._event, self._released = owner, slot, event, threading.Event()

    def wait(self):
        if self._released.is_set():
            raise _lib.AvtError("SnapshotHandle.wait() after release(): the buffer belongs to a later snapshot")
        self._event.synchronize()
        return self._owner._views(self._owner._host[self._slot])

    def release(self):
        self._released.set()


class StateSnapshot:
    """A list of named device tensors — parameters, buffers, momentum buffers — as ONE flat device buffer and two pinned host buffers:

        snap = StateSnapshot(named)          # named: [(name, tensor)] or a dict; layout and both job tables built once
        h = snap.take()                      # one launch + one async D2H copy; returns at once
        views = h.wait(); ...; h.release()   # on any host thread
        snap.restore(h)  /  snap.restore({name: CPU tensor})    # the inverse: host -> flat buffer -> one launch

    Tensors must be dense in storage order (contiguous, channels-last, a contiguous view at any offset); a zero-size tensor gets no job.
    The tensors are addressed by data_ptr(): the snapshot is valid for as long as they stay where they are (`key` tells)."""

    def __init__(self, named):
        named = list(named.items()) if isinstance(named, dict) else list(named)
        if not named:
            raise _lib.AvtError("StateSnapshot: no tensors")
        for name, t in named:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.layout != torch.strided:
                raise _lib.AvtError("StateSnapshot: %s must be a dense device (HIP) tensor" % name)
            if t.device != named[0][1].device:
                raise _lib.AvtError("StateSnapshot: %s is on %s, the first tensor on %s" % (name, t.device, named[0][1].device))
            if not _dense_in_storage_order(t):
                raise _lib.AvtError("StateSnapshot: %s is not dense in storage order (shape %s strides %s): a strided view cannot be "
                                    "copied as bytes" % (name, tuple(t.shape), tuple(t.stride())))
        self.names = [n for n, _ in named]
        self.tensors = [t.detach() for _, t in named]
        self.device = self.tensors[0].device
        self.nbytes = [t.numel() * t.element_size() for t in self.tensors]
        self.offsets, self.total = state_layout(self.nbytes)
        self.key = self.key_of(named)
        self.flat = torch.zeros(max(self.total, 16), dtype=torch.uint8, device=self.device)
        assert self.flat.data_ptr() % 16 == 0
        base = self.flat.data_ptr()
        live = [(t.data_ptr(), base + o, n) for t, o, n in zip(self.tensors, self.offsets, self.nbytes) if n > 0]
        self._pack_tab = self._upload(pack_state_jobs(live))
        self._unpack_tab = self._upload(pack_state_jobs([(d, s, n) for s, d, n in live]))
        self._host = [torch.zeros(max(self.total, 16), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._stage = None                       # restore() from loose CPU tensors: a third pinned buffer, made on first use
        self._handles = [None, None]             # the handle that owns each host buffer
        self._next = 0
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self.flat.record_stream(self._copy_stream)
        self._flat_read = None                   # event: the last device-to-host copy has read the flat buffer
        self._stage_read = None                  # event: the last host-to-device copy has read its pinned source

    @staticmethod
    def key_of(named):
        named = list(named.items()) if isinstance(named, dict) else list(named)
        return tuple((n, t.data_ptr(), t.numel() * t.element_size()) for n, t in named)

    def _upload(self, packed):
        raw, blk, blocks = packed
        if blocks == 0:
            return None
        assert len(raw) % ops.state_job_bytes() == 0 and ops.state_job_bytes() == struct.calcsize(_STATE_JOB), "AvtStateJob layout"
        dev = torch.from_numpy(np.frombuffer(raw + blk.tobytes(), dtype=np.uint8).copy()).to(self.device)
        return dev[:len(raw)], dev[len(raw):].view(torch.int32), blocks

    def _views(self, host):
        """{name: view of a host byte buffer laid out as the flat buffer, with the device tensor's shape, dtype and strides}."""
        out = {}
        for name, t, o, n in zip(self.names, self.tensors, self.offsets, self.nbytes):
            out[name] = torch.as_strided(host[o:o + n].view(t.dtype), tuple(t.shape), tuple(t.stride())) if n else \
                torch.empty_strided(tuple(t.shape), tuple(t.stride()), dtype=t.dtype)
        return out

    def _after_every_stream(self, who):
        """The current stream, once it has waited for every side stream of the training step (the query encoder's BatchNorm buffers are
        written on one: main._allreduce_after_every_stream's hazard) and for the default stream."""
        if torch.cuda.is_current_stream_capturing():
            raise _lib.AvtError("StateSnapshot.%s() under stream capture: a snapshot is taken between steps, not inside a graph" % who)
        from . import models
        cur = torch.cuda.current_stream(self.device)
        for s in models.training_side_streams(self.device) + [torch.cuda.default_stream(self.device)]:
            if s != cur:
                cur.wait_stream(s)
        return cur

    def _launch(self, tab):
        if tab is not None:
            ops.state_copy_multi(tab[0], tab[1], tab[2])
            CALLS["state_copy_multi"] += 1

    @torch.no_grad()
    def take(self):
        """Every tensor into the flat buffer (one launch on the current stream, after every training stream), the flat buffer into a
        pinned host buffer (one async copy on the snapshot's copy stream) -> SnapshotHandle.  With both host buffers still owned by
        earlier handles it first waits, on the host, for the older one's release(): no snapshot is ever dropped or overwritten."""
        cur = self._after_every_stream("take")
        slot = self._next
        old = self._handles[slot]
        if old is not None:
            old._released.wait()
        if self._flat_read is not None:
            cur.wait_event(self._flat_read)  # (the previous snapshot's copy still reads the flat buffer)
        with torch.cuda.device(self.device):
            self._launch(self._pack_tab)
            packed = torch.cuda.Event()
            packed.record(cur)
            self._copy_stream.wait_event(packed)
            with torch.cuda.stream(self._copy_stream):
                self._host[slot].copy_(self.flat, non_blocking=True)
                done = torch.cuda.Event()
                done.record(self._copy_stream)
        self._flat_read = done
        h = self._handles[slot] = SnapshotHandle(self, slot, done)
        self._next = 1 - slot
        return h

    @torch.no_grad()
    def restore(self, source):
        """The inverse of take(): `source` a SnapshotHandle not yet released (its pinned buffer) or {name: CPU tensor} for every name
        (shapes and dtypes of the device tensors; copied, strides and all, into a pinned staging buffer) -> one host-to-device copy of the
        flat buffer and one launch on the current stream, after every training stream.  The weight-plane cache is stale afterwards."""
        cur = self._after_every_stream("restore")
        if isinstance(source, SnapshotHandle):
            if source._owner is not self:
                raise _lib.AvtError("StateSnapshot.restore(): the handle belongs to another snapshot")
            source.wait()
            host = self._host[source._slot]
        else:
            missing = [n for n in self.names if n not in source]
            if missing:
                raise _lib.AvtError("StateSnapshot.restore(): no tensor for %s" % ", ".join(missing[:5]))
            if self._stage_read is not None:
                self._stage_read.synchronize()  # (the previous restore's copy still reads the staging buffer)
            if self._stage is None:
                self._stage = torch.zeros(max(self.total, 16), dtype=torch.uint8).pin_memory()
            host = self._stage
            for name, t, view in zip(self.names, self.tensors, self._views(host).values()):
                src = source[name]
                if src.is_cuda or src.dtype != t.dtype or tuple(src.shape) != tuple(t.shape):
                    raise _lib.AvtError("StateSnapshot.restore(): %s must be a CPU tensor of %s %s, got %s %s %s"
                                        % (name, t.dtype, tuple(t.shape), src.device, src.dtype, tuple(src.shape)))
                view.copy_(src)
        if self._flat_read is not None:
            cur.wait_event(self._flat_read)
        with torch.cuda.device(self.device):
            self.flat.copy_(host, non_blocking=True)
            self._stage_read = torch.cuda.Event()
            self._stage_read.record(cur)
            self._launch(self._unpack_tab)
        invalidate_weight_cache()


# ------------------------------------------------------------------------------------------------------------------------
# Gradient accumulation over micro-batches (one optimizer step = several forward/backward passes: config 5's batch of 8 items
# on fewer than 8 GPUs, each item with its own BatchNorm statistics as a DataParallel replica has, main.py:420).  Left to
# autograd, every parameter's gradient is added into .grad by its own 5-microsecond launch per pass (640 per item) and every
# weight-gradient kernel is preceded by its own memset: 39 ms of a 540 ms step in launches that move no data to speak of
# (profiles/r03/train_step_kernels_before_accumulator.log).  Here a pass's gradients are taken from .grad with ONE
# multi-tensor add, and the weight-gradient kernels write into slices of one arena zeroed by ONE memset per pass.
_ARENA = None


class _GradArena:
    def __init__(self):
        self.buf, self.used, self.want = {}, {}, {}

    def reset(self):
        """Start of a pass: zero what the last pass used; grow to what it asked for."""
        for dev in list(self.buf) + [d for d in self.want if d not in self.buf]:
            want = self.want.get(dev, 0)
            if dev not in self.buf or self.buf[dev].numel() < want:
                self.buf[dev] = torch.zeros(int(want * 1.05) + 1024, dtype=torch.float32, device=dev)
            elif self.used.get(dev, 0):
                self.buf[dev][: self.used[dev]].zero_()
            self.used[dev], self.want[dev] = 0, 0

    def take(self, n, device):
        n4 = (n + 3) // 4 * 4  # 16-byte aligned slices
        self.want[device] = self.want.get(device, 0) + n4
        buf, off = self.buf.get(device), self.used.get(device, 0)
        if buf is None or off + n4 > buf.numel():
            return None  # (first pass, or a pass larger than the last: the caller allocates and zeroes its own)
        self.used[device] = off + n4
        return buf[off : off + n]


class MicroBatchGradients:
    """Sums the gradients of several forward/backward passes into the parameters' .grad with one multi-tensor add per pass.

        acc = MicroBatchGradients(model.parameters())
        acc.begin(len(items))                # instead of optimizer.zero_grad()
        for k, item in enumerate(items):
            if k == len(items) - 1: acc.before_last_backward()   # (needed under DistributedDataParallel: its all-reduce
            loss(item).backward()                                #  must see the sum — the last pass accumulates in .grad)
            if k < len(items) - 1: acc.after_backward()
        acc.finish(); optimizer.step()

    Same sum as autograd's own accumulation (fp32 adds in the same order per parameter)."""

    def __init__(self, params, single_pass_arena=False):
        self.params = [p for p in params if p.requires_grad]
        self.acc = None
        self.seen = False
        self.arena = _GradArena()
        # single_pass_arena (round 6): a step of ONE pass also takes its weight gradients as slices of the arena — one memset per step
        # instead of one per convolution (110 of a one-item config-5 step's launches).  The gradients then ARE arena slices until the
        # next begin() drops them: for loops that read .grad only between backward and the optimizer step, on one rank (DDP's buckets
        # want gradients that own their storage)
        self.single_pass_arena = bool(single_pass_arena)
        self.passes = 1

    def begin(self, passes):
        """passes: forward/backward passes of this optimizer step (1: nothing to accumulate; the arena stays off unless single_pass_arena)."""
        global _ARENA
        for p in self.params:
            p.grad = None
        live = [a for a in (self.acc or []) if a is not None]
        if live:
            torch._foreach_zero_(live)
        self.seen = False
        self.passes = passes
        on = passes > 1 or self.single_pass_arena
        _ARENA = self.arena if on else None
        if on:
            self.arena.reset()

    def after_backward(self):
        if self.acc is None:
            self.acc = [None] * len(self.params)
        src, dst = [], []
        for i, p in enumerate(self.params):
            if p.grad is None:
                continue
            if self.acc[i] is None:  # own storage (a gradient may be a slice of the arena, which the next pass zeroes)
                self.acc[i] = torch.zeros_like(p.grad)
            dst.append(self.acc[i])
            src.append(p.grad)
            p.grad = None
        if src:
            torch._foreach_add_(dst, src)
        self.seen = True
        self.arena.reset()

    def before_last_backward(self):
        """Hand the sum so far to autograd: the next backward accumulates into it (and DDP all-reduces the total)."""
        if self.seen:
            for p, a in zip(self.params, self.acc):
                if a is not None:
                    p.grad = a

    def finish(self):
        global _ARENA
        arena_on, _ARENA = _ARENA is not None, None
        if not arena_on or self.passes == 1:  # (a single pass: every gradient owns its storage — or, single_pass_arena, its slice until begin())
            return
        # the gradients the last pass produced as arena slices live on in .grad only where autograd accumulated into the
        # accumulator's own tensors; a parameter first seen in the last pass keeps an arena slice: give it its own storage
        if self.acc is None:
            self.acc = [None] * len(self.params)
        for i, p in enumerate(self.params):
            if p.grad is not None and self.acc[i] is None:
                p.grad = p.grad.clone()


# ------------------------------------------------------------------------------------------------------------------------
# Convolutions of the training step on the split-plane MFMA kernel (csrc/conv_x3.hip, IO32 form): the forward of every
# Conv3d(bias=False) with channel counts in multiples of 8, and the input gradient of the stride-1 ones (a convolution of
# dy with the flipped, transposed filter).  fp32 tensors in and out; 2^-22 (forward, fp16 planes) / 2^-16 (dgrad, bf16
# planes: gradients need fp32's exponent range) per product instead of the fp32 MFMA's rate of 1/16 of the bf16 pipe.
# The weight gradient is csrc/wgrad_x3.hip (bf16 planes, transposing LDS stage, split over positions with fp32 atomics);
# the strided layers' input gradients are `_dgrad_strided` below; the stems have kernels of their own (`_StemX3`).
_TABS = {}


def _ktab(cin, kernel, h, w, ldi, device):
    key = (cin, tuple(kernel), h, w, ldi, str(device))
    tab = _TABS.get(key)
    if tab is None:
        tab = torch.from_numpy(ops.conv3d_ktab(cin, kernel, h, w, ldi)).to(device)
        _TABS[key] = tab
    return tab


# ---- few-channel layers: g adjacent pixels along W as g * C channels (round 4; the inference path's group_weights_w in the training
# step).  The fast pathway's 8-channel layers ran their forward / input gradient at 0.8-2.3 TB/s on the general tile (rows of 32
# bytes, a 32-wide MFMA tile that is 3/4 padding); the same bytes viewed as [.., W / g, g * C] rows with block-Toeplitz weights along W
# give 4 x fewer, 4 x fuller rows.  The weight gradient keeps the plain form (grouping would multiply its flops by g * g).
_GROUP = 1
_PW_F32 = 1         # pointwise layers (forward / stride-1 input gradient) on the streaming fp32-in / fp32-out kernel (csrc/pw_x3.hip)


_PW_FORM = 0  # _conv_form's answer for the streaming pointwise kernel (1: the general tile, g > 1: g pixels grouped)


def _conv_form(cin, cout, kernel, stride, pad, w):
    """The form a convolution of rows [.., cin] -> [.., cout] runs in — the one place that decides it, asked once per convolution and
    direction: _PW_FORM = the streaming pointwise kernel takes the layer as it is, g > 1 = g adjacent pixels along W grouped into
    g * C channels, 1 = the general tile."""
    if _PW_F32 and tuple(kernel) == (1, 1, 1) and tuple(stride) == (1, 1, 1) and tuple(pad) == (0, 0, 0):
        # (the kernel's 32-bit row count, rows < 2^31 - 16, needs no check of its own: every caller holds a tensor with at least as
        #  many ELEMENTS as these rows below 2^30 - 64 — conv_fusable and conv2d the input, of which a stem's zero-padded 8-channel
        #  copy has one row per position; _conv_dgrad the output gradient)
        if ops.pw_x3_f32_supported(cin, cout):
            return _PW_FORM
    if not _GROUP or tuple(stride) != (1, 1, 1) or pad[2] != kernel[2] // 2 or kernel[2] % 2 == 0 or cin % 8 or cout % 8:
        return 1
    small = min(cin, cout)
    g = 4 if small <= 16 else (2 if small <= 32 else 1)
    if kernel[2] == 1 and kernel[1] == 1 and kernel[0] > 1:  # temporal taps only: grouping just fills the tile; stop at 32 outputs
        while g > 1 and g * cout > 32:
            g //= 2
    while g > 1 and w % g:
        g //= 2
    return g


def _conv_planes(weight, transposed, cin, cout, kernel, stride, pad, w):
    """The weight planes of one direction of a convolution of rows [.., cin] -> [.., cout] of width w, in the form it runs in
    (_conv_form) — forward: fp16 planes; transposed, the input gradient as a convolution of dY: bf16 planes of the flipped filter.
    -> planes, form: (g, grouped kernel, rg) for the pixel-grouped form, _PW_FORM for the streaming pointwise kernel, None for the
    general tile: what _conv_x3_rows takes."""
    g = _conv_form(cin, cout, kernel, stride, pad, w)
    # (grouped planes are a gather of the weight itself: a stem's zero-padded 8-channel rows keep the plain planes, padded to match)
    if g > 1 and cin == weight.shape[0 if transposed else 1]:
        planes, gk, rg = _grouped_planes(weight, g, transposed, ops.X3_BF16 if transposed else ops.X3_F16)
        return planes, (g, gk, rg)
    return _weight_planes(weight, transposed), (_PW_FORM if g == _PW_FORM else None)


_STAT_GROUP_COLS = 128  # widest pixel-grouped output (g * cout columns) whose BatchNorm statistics ride on the epilogue: the copies of
#                         a channel must share one N tile (csrc/conv_args.h stat_fold_store; conv_x3.hip rejects wider forms)
_LAST_STATS = None  # (output data_ptr, workspace, rows of partials per group, groups, channels) of the last convolution that left
#                     BatchNorm statistics behind: handed from inside the autograd Function to conv3d(), which tags the output


def _bwd_bn_args(h):
    return (h.x, h.mean, h.invstd, h.weight, None if h.mask is not None else h.bias, h.mask, h.relu)


def _conv_x3_rows(x, planes, plane_dtype, cin, cout, kernel, stride, pad, add=None, form=None, stats=0, bwd_bn=None):
    """x [B, Cin, T, H, W] channels-last fp32 -> [B, Cout, To, Ho, Wo] channels-last fp32 (+ add, same shape, in the epilogue).
    planes, form: of _conv_planes.
    stats = n > 0: the output feeds a train-mode BatchNorm of n replica groups — the kernel's epilogue leaves its statistics'
    partial sums (ops.conv3d_igemm_x3_f32_stats / ops.pw_x3_f32_stats; recorded in _LAST_STATS).
    bwd_bn = a _BnHandle: x is an output gradient and the result the output gradient of that BatchNorm — masked on the way out, the
    BatchNorm's backward statistics summed in the epilogue (ops.conv3d_igemm_x3_f32_bwdstats / ops.pw_x3_f32_bwdstats; recorded in
    _BWD_STATS)."""
    global _LAST_STATS
    b, _, t, h, w = x.shape
    od = [(n + 2 * p - k) // s_ + 1 for n, p, k, s_ in zip((t, h, w), pad, kernel, stride)]
    y = torch.empty((b, cout, od[0], od[1], od[2]), dtype=torch.float32, device=x.device, memory_format=torch.channels_last_3d)
    stats = int(stats) if (stats and add is None and (cout & (cout - 1)) == 0 and cout >= 8 and b % int(stats) == 0) else 0
    # ---- the form: the rows the kernel sees, and whether statistics can ride on its epilogue
    xr, yr, addr = x.permute(0, 2, 3, 4, 1), y.permute(0, 2, 3, 4, 1), None if add is None else add.permute(0, 2, 3, 4, 1)
    pw = form == _PW_FORM
    if pw:
        # the pointwise layers with few K-steps and many outputs (the bottlenecks' expanding convolutions, the input gradients of the
        # reducing ones) on the streaming kernel: the 128 x 128 tile spent 55 % of a workgroup in its prologue + epilogue on them
        CALLS["pw_f32"] += 1  # (whichever epilogue it ends on: each of the three is a launch of csrc/pw_x3.hip)
        rides = True
    else:
        # pixel-grouped (g, grouped kernel, rg): the same memory as [.., w / g, g * C] rows, block-Toeplitz planes (stride 1 only:
        # _conv_form); the general tile is g = 1.  Grouped statistics fold a channel's pixel copies inside ONE N tile of <= 128 columns:
        # wider forms keep the BatchNorm's own pass
        g, kern, pad_e = (1, kernel, pad) if form is None else (form[0], form[1], (pad[0], pad[1], form[2]))
        wg, cin_e, cout_e = w // g, g * cin, g * cout
        dims, tab = (b, t, h, wg), _ktab(cin_e, kern, h, wg, cin_e, x.device)
        rides = g == 1 or cout_e <= _STAT_GROUP_COLS
    # ---- the epilogue: backward statistics, else forward statistics, else none (+ add); an attempt may decline (None: nothing was
    # launched — the 256 x 256 tile's layers and group counts outside a kernel's domain), and the next one runs
    if bwd_bn is not None and rides:
        if pw:
            st = ops.pw_x3_f32_bwdstats(xr, cin, planes[0], planes[1], yr, cout, plane_dtype, _bwd_bn_args(bwd_bn), bwd_bn.groups, add=addr)
        else:
            st = ops.conv3d_igemm_x3_f32_bwdstats(xr, planes[0], planes[1], yr, tab, dims, cin_e, cout_e, kern, pad_e, plane_dtype,
                                                  _bwd_bn_args(bwd_bn), bwd_bn.groups, cout, add=addr)
        if st is not None:
            CALLS["dgrad_bwdstats"] += 1
            _BWD_STATS[y.data_ptr()] = (st[0], st[1], bwd_bn, y._version)
            return y
    if stats and rides:
        if pw:
            st = ops.pw_x3_f32_stats(xr, cin, planes[0], planes[1], planes[2], yr, cout, plane_dtype, stats)
        else:
            st = ops.conv3d_igemm_x3_f32_stats(xr, planes[0], planes[1], planes[2], yr, tab, dims, cin_e, cout_e, kern, stride, pad_e,
                                               cin_e, cout_e, plane_dtype, stats, cout)
        if st is not None:
            _LAST_STATS = (y.data_ptr(), st[0], st[1], stats, cout)
            return y
    if pw:
        ops.pw_x3_f32(xr, cin, planes[0], planes[1], planes[2], yr, cout, plane_dtype, add=addr)
    else:
        ops.conv3d_igemm_x3_f32(xr, planes[0], planes[1], planes[2], yr, tab, dims, cin_e, cout_e, kern, stride, pad_e, cin_e, cout_e,
                                plane_dtype, add=addr)
    return y


def _tag_stats(y):
    """The statistics the convolution that produced y left behind (if it did) become an attribute of y: bn_act picks them up."""
    global _LAST_STATS
    st, _LAST_STATS = _LAST_STATS, None
    if st is not None and st[0] == y.data_ptr():
        y._avt_stats = st[1:]
    return y


class _ConvX3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride, padding, stats=0, bn_in=None):
        cout, cin = weight.shape[0], weight.shape[1]
        kernel = tuple(weight.shape[2:])
        ctx.conf = (stride, padding, kernel, cin, cout)
        ctx.bn_in = bn_in  # the fused BatchNorm whose output x is (a _BnHandle), or None: see _conv_backward
        xin = x
        if cin % 8:  # stem: [B, 3, T, H, W] -> 8 channels-last channels, the last 5 zero (weights padded to match)
            xin = torch.empty((x.shape[0], 8) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device, memory_format=torch.channels_last_3d)
            xin[:, :cin] = x
            xin[:, cin:] = 0
        # (the stems keep the padded channels-last copy: their weight gradient reads it 4 channels at a time)
        ctx.save_for_backward(xin if (cin % 8 and (_STEM_WGRAD_X3 or cin != 3)) else x, weight)
        CALLS["conv_fwd_x3"] += 1
        planes, form = _conv_planes(weight, False, xin.shape[1], cout, kernel, stride, padding, xin.shape[4])
        return _conv_x3_rows(xin, planes, ops.X3_F16, xin.shape[1], cout, kernel, stride, padding, form=form, stats=stats)

    @staticmethod
    def backward(ctx, dy):
        return _conv_backward(ctx, dy, None) + (None, None, None, None)


def _conv_backward(ctx, dy, dalias):
    """(dx, dw) of the convolution; dalias = a gradient that reached the input by another path (conv3d_fork), summed into dx
    in the stride-1 kernel's epilogue instead of by a separate pass.  (Weight gradients on a side stream of their own — nothing in the
    backward waits for a dW — were measured three times and not kept: round 5 at 8 items per rank, -4 ... -11 %; round 6 at one item
    per rank, eager 234 -> 227 clips/s, inside the replayed HIP graph 303 -> 280: profiles/r06/train_wgrad_side_stream_ab_not_kept.log)"""
    x, weight = ctx.saved_tensors
    stride, padding, kernel, cin, cout = ctx.conf
    dy = dy.contiguous(memory_format=torch.channels_last_3d)
    dw = _conv_wgrad(ctx, dy, x, weight, stride, padding, kernel, cin, cout) if ctx.needs_input_grad[1] else None
    return _conv_dgrad(ctx, dy, dalias, x, weight, stride, padding, kernel, cin, cout), dw


def _conv_wgrad(ctx, dy, x, weight, stride, padding, kernel, cin, cout):
    """dW of the convolution (split-plane weight-gradient kernels; MIOpen for the shapes they do not cover)."""
    dw = None
    taps = kernel[0] * kernel[1] * kernel[2]
    dims = (x.shape[0], x.shape[2], x.shape[3], x.shape[4])
    xr, dyr = x.permute(0, 2, 3, 4, 1), dy.permute(0, 2, 3, 4, 1)  # (views: channels-last memory as rows)
    if (_WGRAD_X3 and cin % 8 == 0 and taps <= 28 and max(x.numel(), dy.numel()) < (1 << 31) - 64 and
            weight.is_contiguous(memory_format=torch.channels_last_3d)):
        CALLS["wgrad_x3"] += 1
        flat = _ARENA.take(weight.numel(), weight.device) if _ARENA is not None else None
        if flat is not None:  # a zeroed slice of the micro-batch's gradient arena: no memset launch per convolution
            # (the weight's OWN strides, size-1 dimensions included: torch's multi-tensor optimizer kernels take their fast path only for
            #  gradients whose strides equal the parameters' — a permuted view differs in the stride of a one-tap dimension, and a
            #  foreach SGD then ran one launch per tensor: +4.8 ms on a 47 ms step, profiles/r06/train_one_item_arena_sgd_ab.log)
            dw = torch.as_strided(flat, tuple(weight.shape), tuple(weight.stride()))
            _wgrad_x3(dyr, xr, flat, dims, cin, cout, kernel, stride, padding, (0, 0, 0), cin, cout, taps * cin, False)
        else:
            dw = torch.empty_like(weight)  # channels-last strides: memory [cout][kt][kh][kw][cin], the kernel's order
            _wgrad_x3(dyr, xr, dw, dims, cin, cout, kernel, stride, padding, (0, 0, 0), cin, cout, taps * cin, True)
    elif (_WGRAD_X3 and cin % 8 and cin != 3 and x.shape[1] == 8 and taps <= 28 and max(x.numel(), dy.numel()) < (1 << 31) - 64):
        # a few-channel first layer (VGGish: 1 mel channel) on its zero-padded 8-channel copy; the padded taps' gradient is dropped
        CALLS["wgrad_x3"] += 1
        dw8 = torch.empty((cout, 8) + tuple(kernel), dtype=torch.float32, device=dy.device, memory_format=torch.channels_last_3d)
        _wgrad_x3(dyr, xr, dw8, dims, 8, cout, kernel, stride, padding, (0, 0, 0), 8, cout, taps * 8, True)
        dw = torch.empty_like(weight)
        dw.copy_(dw8[:, :cin])
    elif (_WGRAD_X3 and _STEM_WGRAD_X3 and cin == 3 and x.shape[1] == 8 and kernel[1] * kernel[2] <= 49 and
          max(x.numel(), dy.numel()) < (1 << 31) - 64):
        # the stems: 3 input channels travel as 4 of the forward's 8-channel padded clip; a [kt,7,7] filter is kt slices of
        # 49 taps, each a weight-gradient problem of its own with the temporal padding shifted by its frame tap
        kt, kh, kw = kernel
        # (deterministic: every slice WRITES its kh * kw * 4 columns of each row, and the kt slices cover the rows: no zeroing)
        acc = (torch.empty if _DETERMINISTIC else torch.zeros)((cout, kt, kh * kw, 4), dtype=torch.float32, device=dy.device)
        for dt in range(kt):
            _wgrad_x3(dyr, xr, acc[:, dt], dims, 4, cout, (1, kh, kw), stride, (padding[0] - dt, padding[1], padding[2]),
                      (dy.shape[2], dy.shape[3], dy.shape[4]), 8, cout, kt * kh * kw * 4, False)
        CALLS["wgrad_stem_x3"] += 1
        dw = torch.empty_like(weight)
        dw.copy_(acc.view(cout, kt, kh, kw, 4)[..., :3].permute(0, 4, 1, 2, 3))
    else:  # (stems when AVT_TRAIN_STEM_WGRAD_X3=0, filters of more than 28 taps): MIOpen
        if _DETERMINISTIC:
            raise _lib.AvtError("deterministic training: the weight gradient of a %s -> %s convolution with kernel %s has no hand-written "
                                "kernel and would run on MIOpen, whose summation order is not fixed" % (cin, cout, tuple(kernel)))
        if x.shape[1] != weight.shape[1]:  # the padded copy was saved: MIOpen wants the 3-channel clip
            x = x[:, : weight.shape[1]].contiguous(memory_format=torch.channels_last_3d)
        CALLS["miopen_wgrad"] += 1
        dw = torch.ops.aten.convolution_backward(dy, x, weight, None, stride, padding, (1, 1, 1), False, (0, 0, 0), 1,
                                                 [False, True, False])[1]
    return dw


def _wgrad_x3(dyr, xr, dw, dims, cin, cout, kernel, stride, padding, out_dims, ldx, ldy, ldw, fresh):
    """The one launch of the general weight-gradient kernel (csrc/wgrad_x3.hip).  fresh: dw is a tensor of the filter's own in the kernel's
    order, [cout][taps][cin], which the plain entry zeroes; else a zeroed accumulator or a column slice of one (the general entry, nothing
    zeroed).  Deterministic mode: one launch pair (tile + fixed-order reduction) that WRITES dw's taps * cin columns in either case."""
    if _DETERMINISTIC:
        CALLS["wgrad_det"] += 1
        ops.conv3d_wgrad_x3_det_sub_f32(dyr, xr, dw, dims, cin, cout, kernel, stride, padding, out_dims, ldx, ldy, ldw)
    elif fresh:
        ops.conv3d_wgrad_x3_f32(dyr, xr, dw.permute(0, 2, 3, 4, 1), dims, cin, cout, kernel, stride, padding, ldx, ldy)
    else:
        ops.conv3d_wgrad_x3_sub_f32(dyr, xr, dw, dims, cin, cout, kernel, stride, padding, out_dims, ldx, ldy, ldw, False)


def _conv_dgrad(ctx, dy, dalias, x, weight, stride, padding, kernel, cin, cout):
    dx = None
    if ctx.needs_input_grad[0]:
        if dalias is not None:
            dalias = dalias.contiguous(memory_format=torch.channels_last_3d)
        if (cin % 8 == 0 and stride == (1, 1, 1) and all(2 * p == k - 1 for p, k in zip(padding, kernel)) and
                dy.numel() < (1 << 30) - 64):
            CALLS["dgrad_x3"] += 1
            hb = getattr(ctx, "bn_in", None)  # x is a fused BatchNorm's output: dx is that BatchNorm's output gradient
            ctx.bn_in = None  # (the handle holds that BatchNorm's input and mask: not past this backward)
            if hb is not None and not (_EPI_BWD and hb.c == cin and tuple(hb.x.shape) == tuple(x.shape) and x.shape[0] % hb.groups == 0):
                hb = None
            planes, form = _conv_planes(weight, True, cout, cin, kernel, (1, 1, 1), padding, dy.shape[4])
            dx = _conv_x3_rows(dy, planes, ops.X3_BF16, cout, cin, kernel, (1, 1, 1), padding, add=dalias, form=form, bwd_bn=hb)
        else:
            dx = _dgrad_strided(dy, weight, stride, padding, kernel, tuple(x.shape)) if (_DGRAD_S_X3 and cin % 8 == 0) else None
            if dx is not None:
                CALLS["dgrad_strided_x3"] += 1
            else:
                CALLS["miopen_dgrad"] += 1
                dx = torch.ops.aten.convolution_backward(dy, x, weight, None, stride, padding, (1, 1, 1), False, (0, 0, 0), 1,
                                                         [True, False, False])[0]
            if dalias is not None:
                dx = dx + dalias
    return dx


def _dgrad_strided(dy, weight, stride, padding, kernel, xshape):
    """Input gradient of a STRIDED convolution as convolutions of dY, one per residue class of the input position modulo the
    stride (a transposed convolution decomposed so that no zero is multiplied): class r gathers the taps d = (r + p) mod s,
    + s, ... and writes the positions s i + r through the kernel's output-row remap.  SlowFast's three kinds: [1,3,3] stride
    (1,2,2) (4 classes of 1, 2, 2, 4 taps), 1x1x1 stride (1,2,2) (one class; the other positions are zeros), [7,1,1] stride
    (4,1,1) (4 temporal classes of 1, 2, 2, 2 taps).  The 3D-ResNets' kind: 3x3x3 and 1x1x1 at stride (2,2,2), 8 classes of
    1 ... 8 taps (seven of the projection's eight are zeros).  There frame i_t of a class is frame 2 i_t + r_t, which is the spatial
    remap over PAIRS of frames (2 h rows) as long as T is even — so odd extents (T = 5 and 3 at W = 20) are computed on a grid
    rounded up to even extents and cropped.  -> dx, or None outside that domain (the caller falls back to MIOpen)."""
    b, cin, t, h, w = xshape
    cout = weight.shape[0]
    st, sh, sw = stride
    cube = st == sh == sw == 2
    if not ((st == 1 and sh == sw and sh > 1) or (sh == 1 and sw == 1 and st > 1) or cube) or cin % 8 or cout % 8:
        return None
    if dy.numel() >= (1 << 30) - 64:
        return None
    full = (t, h, w)
    if cube:  # the grid the classes tile: every extent rounded up to the stride
        t, h, w = (-(-n // 2) * 2 for n in full)
        if b * t * h * w * cin >= (1 << 31) - 64:
            return None
    elif (st > 1 and t % st) or (sh > 1 and (h % sh or w % sw)):
        return None
    to, ho, wo = dy.shape[2], dy.shape[3], dy.shape[4]
    if st > 1 and not cube and to * st != t:
        return None
    classes = weight_planes._strided_planes(weight, kernel, stride, padding, (t, h, w), (to, ho, wo))
    if classes is None:
        return None
    dx = torch.empty((b, cin, t, h, w), dtype=torch.float32, device=dy.device, memory_format=torch.channels_last_3d)
    if any(c[1] is None for c in classes):  # classes no tap reaches (a 1x1x1 filter at stride 2: three of four) are zeros
        dx.zero_()
    rows = dx.permute(0, 2, 3, 4, 1).reshape(-1, cin)  # (a view: channels-last memory)
    dyr = dy.permute(0, 2, 3, 4, 1)
    for (rt, rh, rw), c in classes:
        if c is None:
            continue
        hi, lo, kern, pad_b, n = c
        if n[0] * n[1] * n[2] == 0:
            continue
        if cube:     # position (i_t, i_h, i_w) of class (rt, rh, rw) is (2 i_t + rt, 2 i_h + rh, 2 i_w + rw): a pair of frames as 2 h rows
            out_rows, first = (2, 2 * h, w), (rt * h + rh) * w + rw
        elif st > 1:  # temporal classes: frame i_t of class rt is frame st * i_t + rt: a grid of st * h rows per group of st frames
            out_rows, first = (1, st * h, w), rt * h * w
        else:        # spatial classes: position (i_h, i_w) of class (rh, rw) is (sh * i_h + rh, sw * i_w + rw)
            out_rows, first = (sh, h, w), rh * w + rw
        ops.conv3d_igemm_x3_f32_ex(dyr, hi, lo, None, rows[first:], _ktab(cout, kern, ho, wo, cout, dy.device), (b, to, ho, wo), cout,
                                   cin, kern, pad_b, n, cout, cin, ops.X3_BF16, out_rows=out_rows)
    if (t, h, w) != full:  # the rounded-up grid's last frame / row / column is no input position
        dx = dx[:, :, : full[0], : full[1], : full[2]].contiguous(memory_format=torch.channels_last_3d)
    return dx


class _ConvX3Fork(torch.autograd.Function):
    """conv(x) AND x itself (an alias): the block's shortcut takes the alias, so the gradient that comes back through the
    shortcut arrives HERE and is added in the epilogue of this convolution's input-gradient kernel — autograd would
    otherwise sum the two contributions to x with a separate elementwise pass (5.5 % of the step's device time)."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, stats=0, bn_in=None):
        y = _ConvX3.forward(ctx, x, weight, stride, padding, stats, bn_in)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dalias):
        if dy is None:  # (the convolution's output was not used: only the alias carries a gradient)
            return (dalias if ctx.needs_input_grad[0] else None), None, None, None, None, None
        return _conv_backward(ctx, dy, dalias) + (None, None, None, None)


# ------------------------------------------------------------------------------------------------------------------------
# The stems: Conv3d(3, C, [kt,7,7], stride [1,2,2], pad [kt//2,3,3]) on the raw clip.  As an implicit GEMM over 8 padded
# channels the fast stem's forward ran 4.7 ms and its weight gradient (five [1,7,7] slices of wgrad_x3) 9.5 ms of a 95 ms item
# (profiles/r03/train_layers_before_stem.log): both gather every pixel once per tap.  The patch-resident kernels stage the
# input rows once: the forward is the inference stem kernel (pixel-pair form, time-grouped for the 8-channel fast stem, fp16
# planes) writing fp32, the weight gradient csrc/stem_train.hip (bf16 planes).  The clip is re-split into planes in each
# direction (a 12-byte read and a 16-byte write per pixel) instead of kept: the saved tensor is the caller's clip itself.


def _stem_tgroup(cout, t):
    """Output frames computed together as channels of one MFMA tile (fused_slowfast.stem_conv): 32 / cout, or None."""
    if cout % 32 == 0:
        return 1
    g = 32 // cout if 32 % cout == 0 else 0
    return g if g > 1 and t % g == 0 else None


def stem_patch_ok(x, conv):
    if not (_STEM_PATCH and conv.in_channels == 3 and x.dim() == 5 and x.shape[1] == 3):
        return False
    kt = conv.kernel_size[0]
    _, _, t, h, w = x.shape
    return (tuple(conv.kernel_size[1:]) == (7, 7) and tuple(conv.stride) == (1, 2, 2) and tuple(conv.padding) == (kt // 2, 3, 3) and
            w % 2 == 0 and _stem_tgroup(conv.out_channels, t) is not None and
            bool(_lib.lib().avt_stem_conv_supported(h, w // 2, conv.out_channels * _stem_tgroup(conv.out_channels, t))) and
            ops.stem_wgrad_x3_supported(h, w // 2, conv.out_channels, kt) and x.numel() // 3 * 16 < (1 << 32) - 64)


class _StemX3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        b, _, t, h, w = x.shape
        c, kt = weight.shape[0], weight.shape[2]
        g = _stem_tgroup(c, t)
        xh, xl = ops.clip_planes_f32(x, ops.X3_F16)
        wh, wl, wscale, fpt = weight_planes._stem_weight_image(weight, g)
        y = torch.empty((b, c, t, h // 2, w // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last_3d)
        CALLS["conv_fwd_x3"] += 1
        CALLS["stem_fwd_patch"] += 1
        ops.stem_conv_x3_f32(xh, xl, wh, wl, wscale, y, b, t, h, w // 2, g * c, kt + g - 1, g, kt // 2, g, ops.X3_F16, frames_per_tile=fpt)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None
        b, _, t, h, w = x.shape
        c, kt = weight.shape[0], weight.shape[2]
        dy = dy.contiguous(memory_format=torch.channels_last_3d)
        xh, xl = ops.clip_planes_f32(x, ops.X3_BF16)
        CALLS["wgrad_stem_patch"] += 1
        CALLS["wgrad_det"] += _DETERMINISTIC
        stem_wgrad = ops.stem_wgrad_x3_det if _DETERMINISTIC else ops.stem_wgrad_x3
        dwp = stem_wgrad(xh, xl, dy, b, t, h, w // 2, c, kt, kt // 2)  # [c, kt, 7, 4 pair taps, 2 pixels x 4 channels]
        dw = torch.empty_like(weight)
        dw.copy_(dwp.view(c, kt, 7, 8, 4)[:, :, :, 1:, :3].permute(0, 4, 1, 2, 3))  # column tap k = 2 * pair + pixel - 1
        return None, dw


class _MaxPoolHW(torch.autograd.Function):
    """MaxPool3d((1,3,3),(1,2,2),(0,1,1)) on channels-last fp32 (csrc/stem_train.hip): the forward records which tap held each
    maximum (4 bits per element), the backward gathers the gradient from it."""

    @staticmethod
    def forward(ctx, x, cat=None):
        b, c, t, h, w = x.shape
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        if cat is None:
            y, ldy = torch.empty((b, c, t, ho, wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last_3d), 0
        else:  # the first c channels of a concatenation buffer's rows (join_channels)
            y, ldy = _alias(cat[0], cat[1], c), cat[0].shape[1]
        tap = torch.empty(y.numel() // 2, dtype=torch.uint8, device=x.device)
        CALLS["maxpool_hip"] += 1
        K.avt_maxpool_train_fwd(_p(x), _p(y), _p(tap), b * t, h, w, c, ldy, _stream())
        ctx.save_for_backward(tap)
        ctx.dims = (b, c, t, h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        (tap,) = ctx.saved_tensors
        b, c, t, h, w = ctx.dims
        ld_dy = _row_ld(dy)
        if ld_dy is None:
            dy, ld_dy = dy.contiguous(memory_format=torch.channels_last_3d), c
        dx = torch.empty((b, c, t, h, w), dtype=torch.float32, device=dy.device, memory_format=torch.channels_last_3d)
        K.avt_maxpool_train_bwd(_p(dy), _p(tap), _p(dx), b * t, h, w, c, ld_dy, _stream())
        return dx, None


def max_pool_hw(x, pool, cat_extra=0):
    """pool(x) for the stems' nn.MaxPool3d((1,3,3),(1,2,2),(0,1,1)): the HIP pair above on channels-last fp32 device tensors
    that carry a gradient in train mode, the module itself otherwise.  cat_extra: as in bn_act (the HIP path only)."""
    if (_FUSED and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and x.requires_grad and x.shape[1] % 4 == 0 and
            x.is_contiguous(memory_format=torch.channels_last_3d) and tuple(pool.kernel_size) == (1, 3, 3) and
            tuple(pool.stride) == (1, 2, 2) and tuple(pool.padding) == (0, 1, 1) and not pool.ceil_mode and
            pool.dilation in (1, (1, 1, 1)) and x.numel() // 4 < (1 << 32)):
        if not cat_extra or not _JOIN:
            return _MaxPoolHW.apply(x)
        b, c, t, h, w = x.shape
        cat = (_cat_buffer((b, c, t, (h - 1) // 2 + 1, (w - 1) // 2 + 1), c + int(cat_extra), x.device), 0)
        y = _MaxPoolHW.apply(x, cat)
        y._avt_cat = cat
        return y
    return pool(x)


class _MaxPool3d(torch.autograd.Function):
    """MaxPool3d(3, 2, 1) on channels-last fp32 (csrc/stem_train.hip, the 3D-ResNets' stem pool): the forward records which of the 27
    taps held each maximum (one byte per element, torch's tie / NaN rule), the backward gathers the gradient from it."""

    @staticmethod
    def forward(ctx, x):
        b, c, t, h, w = x.shape
        to, ho, wo = (t - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = torch.empty((b, c, to, ho, wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last_3d)
        tap = torch.empty(y.numel(), dtype=torch.uint8, device=x.device)
        CALLS["maxpool3d_hip"] += 1
        K.avt_maxpool3d_train_fwd(_p(x), _p(y), _p(tap), b, t, h, w, c, 0, _stream())
        ctx.save_for_backward(tap)
        ctx.dims = (b, c, t, h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        (tap,) = ctx.saved_tensors
        b, c, t, h, w = ctx.dims
        ld_dy = _row_ld(dy)
        if ld_dy is None:
            dy, ld_dy = dy.contiguous(memory_format=torch.channels_last_3d), c
        dx = torch.empty((b, c, t, h, w), dtype=torch.float32, device=dy.device, memory_format=torch.channels_last_3d)
        K.avt_maxpool3d_train_bwd(_p(dy), _p(tap), _p(dx), b, t, h, w, c, ld_dy, _stream())
        return dx


def _triple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


def max_pool3d(x, pool):
    """pool(x) for the 3D-ResNet stems' nn.MaxPool3d(3, stride=2, padding=1): the HIP pair above on channels-last fp32 device tensors
    that carry a gradient in train mode, the module itself otherwise (eval mode, CPU, other layouts / dtypes, any other window)."""
    if (_FUSED and pool.training and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and x.requires_grad and
            x.shape[1] % 4 == 0 and x.is_contiguous(memory_format=torch.channels_last_3d) and
            _triple(pool.kernel_size) == (3, 3, 3) and _triple(pool.stride) == (2, 2, 2) and _triple(pool.padding) == (1, 1, 1) and
            not pool.ceil_mode and _triple(pool.dilation) == (1, 1, 1) and not pool.return_indices and
            x.numel() // x.shape[1] < (1 << 31)):
        return _MaxPool3d.apply(x)
    return pool(x)


def conv_fusable(x, conv):
    """(in_channels == 3: the stems — the clip is zero-padded to 8 channels for the forward; it needs no input gradient.)"""
    return (_CONV_X3 and conv.training and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and conv.bias is None and
            conv.groups == 1 and tuple(conv.dilation) == (1, 1, 1) and conv.out_channels % 8 == 0 and
            (conv.in_channels % 8 == 0 or (conv.in_channels == 3 and not x.requires_grad)) and
            max(conv.kernel_size) <= 8 and conv.weight.dtype == torch.float32 and conv.padding_mode == "zeros" and
            not isinstance(conv.padding, str) and x.numel() < (1 << 30) - 64 and
            conv.weight.is_contiguous(memory_format=torch.channels_last_3d) and  # the model was put in the training layout
            (max(conv.kernel_size) > 1 or x.is_contiguous(memory_format=torch.channels_last_3d)))  # (a 1x1x1 weight is both layouts)


def conv2d(x, conv):
    """conv(x) for a Conv2d module (VGGish, models/audio_models/vggish.py:15-33, in the m=2 training branch, models.py:343-345,
    405-407): the same split-plane kernels, the image as a one-frame clip — NHWC rows are NDHWC rows with T = 1 — forward,
    input gradient and weight gradient; the bias is added by torch.  The module's weight is put in channels-last memory on first
    use (its [cout][kh][kw][cin] order is the kernels' K order).  Stock op otherwise (eval mode, CPU, other dtypes)."""
    ok = (_CONV_X3 and conv.training and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and conv.groups == 1 and
          tuple(conv.dilation) == (1, 1) and conv.out_channels % 8 == 0 and conv.weight.dtype == torch.float32 and
          conv.padding_mode == "zeros" and not isinstance(conv.padding, str) and max(conv.kernel_size) <= 5 and
          (conv.in_channels % 8 == 0 or (conv.in_channels < 8 and not x.requires_grad)) and x.numel() < (1 << 30) - 64)
    if not ok:
        return conv(x)
    if not conv.weight.is_contiguous(memory_format=torch.channels_last):
        # (main.py puts the model in the training layout BEFORE the optimizer / DDP buckets exist: training_layout(); this is the
        #  guard for callers that did not — a layout change, not a value change)
        conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    x5 = x.contiguous(memory_format=torch.channels_last).unsqueeze(2)   # [n, C, 1, H, W]: channels_last_3d strides
    w5 = conv.weight.unsqueeze(2)                                       # [cout, cin, 1, kh, kw], a view (autograd folds it back)
    y = _ConvX3.apply(x5, w5, (1,) + tuple(conv.stride), (0,) + tuple(conv.padding)).squeeze(2)
    return y if conv.bias is None else y + conv.bias.view(1, -1, 1, 1)


def training_layout(model):
    """The model in the layout the hand-written training passes read: channels_last_3d Conv3d weights / activations, channels_last
    Conv2d weights (VGGish) — once, at setup, before optimizers or DDP buckets are built over the parameters."""
    model = model.to(memory_format=torch.channels_last_3d)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.Conv2d) and not m.weight.is_contiguous(memory_format=torch.channels_last):
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
    return model


def _stat_groups(x, bn):
    """Replica groups of the train-mode BatchNorm `bn` that consumes a convolution's output (conv3d(..., stats=bn)), or 0 when the
    fused BatchNorm pass will not run on it (eval mode, switched off, a channel count outside its domain)."""
    if bn is None or not (_EPI_STATS and _FUSED and bn.training and bn.weight is not None and bn.weight.dtype == torch.float32):
        return 0
    groups = _BN_GROUPS if _BN_GROUPS > 1 else 1
    return groups if x.shape[0] % groups == 0 else 0


def conv3d_fork(x, conv, stats=None):
    """-> (conv(x), x'): x' is x for every purpose but autograd's — hand it to the OTHER consumers of x (the block's shortcut
    or projection) and their gradient is summed into conv's input gradient inside its kernel.  Stock path: (conv(x), x).
    stats = the BatchNorm module conv(x) feeds (see conv3d)."""
    if not _FORK:
        return conv3d(x, conv, stats), x
    if not conv_fusable(x, conv) or conv.in_channels % 8:
        return conv(x), x
    x = x.contiguous(memory_format=torch.channels_last_3d)
    y, alias = _ConvX3Fork.apply(x, conv.weight, tuple(conv.stride), tuple(conv.padding), _stat_groups(x, stats),
                                 getattr(x, "_avt_bn", None) if _EPI_BWD else None)
    return _tag_stats(y), alias


def conv3d(x, conv, stats=None):
    """conv(x) for a Conv3d module: the split-plane MFMA kernels in train mode on fp32 device tensors of a model in the
    training layout (forward, stride-1 input gradient, weight gradient), the module itself otherwise.
    stats = the nn.BatchNorm3d the output goes into next (bn_act(conv3d(x, conv, stats=bn), bn)): the convolution's epilogue sums
    the statistics that BatchNorm needs while the tile is still in the LDS, and bn_act skips its pass over the output."""
    if not conv_fusable(x, conv):
        return conv(x)
    if conv.in_channels == 3 and stem_patch_ok(x, conv):
        return _StemX3.apply(x, conv.weight)
    if conv.in_channels % 8 and not x.is_contiguous(memory_format=torch.channels_last_3d):
        pass  # (the stem's padded copy is built channels-last from any layout)
    else:
        x = x.contiguous(memory_format=torch.channels_last_3d)  # no-op inside the network; a clip handed over as NCDHW is transposed once
    return _tag_stats(_ConvX3.apply(x, conv.weight, tuple(conv.stride), tuple(conv.padding), _stat_groups(x, stats),
                                    getattr(x, "_avt_bn", None) if _EPI_BWD else None))
