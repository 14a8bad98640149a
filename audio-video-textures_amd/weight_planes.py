"""The 16-bit hi / lo planes of the training step's convolution weights: ONE cache (CACHE), one validity rule, four makers.

Every convolution looks its weight's planes up before it launches.  An entry belongs to the tensor it was made from (a weak reference:
an id can be reused) and is CURRENT while that tensor's `_version` and the cache's generation are the ones it was made at.  In-place
updates move `_version`; whatever does not — updates through `.data`, torch's fused optimizers — is followed by `CACHE.invalidate()`,
which moves the generation: every optimizer step of the process does (the hook below), and so does the end of a stream capture
(`capture_ended`: a capture marks entries current although nothing ran).  A stale entry that remembers the launches that made it
(`jobs`) is re-made in place, together with every other such entry of its device, by one launch (`refresh`); any other stale entry
misses and its maker builds it anew.  The recipe holds as long as the owner's `signature` — shape, strides, dtype, device — is the one
it was derived from; the signature is checked when a stale entry is about to be re-made, not on a hit.

The makers, each "look up; on a miss build, store, return": `_weight_planes` (plain and transposed), `_grouped_planes` (pixel-grouped
few-channel layers), `_strided_planes` (the residue classes of a strided layer's input gradient), `_stem_weight_image` (the stems' LDS
image).  Which form a convolution runs in is train_ops' business (_conv_form, _conv_planes).

Deliberately left as it was: the hook is process-wide (any optimizer's step marks every entry stale), and nothing orders an in-place
re-make after earlier reads of the same planes on other streams (autograd's join before the optimizer is what makes that safe)."""
import struct
import weakref

import torch

from . import ops
from .fused_slowfast import split_planes, stem_lds_image
from .job_tables import _PLANE_JOB, CALLS, _JobTable, _pack_jobs
from .ops import _RAW_STREAM

# switches the makers read (tests set them to 0 to compare two ways of making the same planes)
_PLANES_HIP = 1    # weight planes by csrc/stem_train.hip's two kernels (0: torch ops)
_PLANES_MULTI = 1  # stale planes are re-made by ONE launch over every cached weight (0: one by one, as rounds 3-5 did)
_GROUP_GATHER = 1  # the grouped planes by ONE gather launch per weight (0: the torch assembly of round 4)


def signature(t):
    """What an entry's recipe (sizes, offsets into the storage, the planes' device) was derived from."""
    return tuple(t.shape), tuple(t.stride()), t.dtype, t.device


class _PlaneEntry:
    """A cached set of weight planes: `value` is what the lookup returns; `jobs` describes the launches that made its tensors
    (None: not re-makeable in place — torch-assembled forms), as dicts {"off": byte offset of the source in the owner's storage,
    "fields": the AvtPlaneJob fields after `w` up to `blk0`, "sel": taps, "blocks": grid size}."""
    __slots__ = ("cache", "ref", "version", "gen", "value", "jobs", "sig")

    def __init__(self, cache, owner, value, jobs=None):
        self.cache, self.ref, self.version, self.gen, self.value, self.jobs = cache, weakref.ref(owner), owner._version, cache.gen, value, jobs
        self.sig = signature(owner)

    def stale(self, owner):
        return self.version != owner._version or self.gen != self.cache.gen


def _job_rows(w, owner, hi, lo, ws, f16, rows, k, idx_map=None):
    kind = 0 if idx_map is None else 2
    return {"off": w.data_ptr() - owner.data_ptr(), "blocks": int(rows),
            "fields": (hi.data_ptr(), lo.data_ptr(), ws.data_ptr() if ws is not None else 0, idx_map.data_ptr() if idx_map is not None else 0,
                       kind, int(bool(f16)), int(rows), int(k), 0, 0, 0, 0, 0, 0),
            "sel": (), "keep": (hi, lo, ws, idx_map)}


def _job_transposed(w, owner, hi, lo, cout, taps, cin, sel):
    gx, gy = (cin + 31) // 32, (cout + 31) // 32
    return {"off": w.data_ptr() - owner.data_ptr(), "blocks": gx * gy * len(sel),
            "fields": (hi.data_ptr(), lo.data_ptr(), 0, 0, 1, 0, 0, 0, int(cout), int(taps), int(cin), len(sel), gx, gy),
            "sel": tuple(int(v) for v in sel), "keep": (hi, lo)}


def pack_plane_jobs(jobs):
    """jobs: (address of the owner's storage, job dict of _job_rows / _job_transposed) per launch -> (AvtPlaneJob table as bytes,
    blk2job int32 array, blocks): job n reads its source at the address + "off", has `sel` zero-padded to 32 taps and owns "blocks"
    consecutive blocks from its blk0 (include/avt.h)."""
    return _pack_jobs(jobs, lambda r: r[1]["blocks"],
                      lambda r, b0: struct.pack(_PLANE_JOB, r[0] + r[1]["off"], *r[1]["fields"], b0, 0,
                                                *r[1]["sel"], *(0,) * (32 - len(r[1]["sel"]))))


class PlaneCache:
    def __init__(self):
        self.entries = {}     # key (the maker's: id of the owner, form) -> _PlaneEntry
        self.gen = 0          # invalidate() moves it
        self.job_tables = {}  # device -> _JobTable of the multi-job launch
        self.refreshed = {}   # device -> (event, stream handle, handles of the streams that wait for it) of the last refresh launch

    def invalidate(self, drop=False):
        """Mark every entry stale: the next lookup re-makes them — all of them in one launch (refresh).  drop=True forgets the entries
        themselves (tests that compare two ways of MAKING the planes)."""
        self.gen += 1
        if drop:
            self.entries.clear()
            for tabs in self.job_tables.values():
                tabs.forget()

    def capture_ended(self, device):
        """A stream capture on `device` is over (GraphedStep): its lookups marked entries current and recorded a refresh event although
        nothing ran.  Everything is stale, and no eager lookup waits for an event of the capture."""
        self.invalidate()
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        self.refreshed.pop(device, None)

    def is_stale(self):
        """True when no entry is current (every lookup re-makes its planes): the state a capture must start from for the re-make
        launch to be part of its graph."""
        for ent in self.entries.values():
            owner = ent.ref()
            if owner is not None and not ent.stale(owner):
                return False
        return True

    def select(self, device):
        """-> [(entry, owner)]: the stale entries of `device` whose recipe still fits their owner.  An owner whose signature changed
        (`param.data = other layout`, a move to another device) voids its entries' recipes: their lookups miss and the planes are made
        anew.  No GPU call."""
        todo = []
        for ent in self.entries.values():
            owner = ent.ref()
            if owner is None or not ent.jobs or not ent.stale(owner):
                continue
            if ent.sig != signature(owner):
                ent.jobs = None
            elif owner.device == device:
                todo.append((ent, owner))
        return todo

    def refresh(self, device):
        """Re-make EVERY stale entry of `device` whose recipe is known, in place, with one launch (ops.weight_planes_multi); -> False
        when there was nothing to do.  Other streams order themselves behind the launch in lookup (one event).  Under stream capture
        too the entries count as current afterwards: a later lookup of the same step must not capture the launch again."""
        todo = self.select(device)
        if not todo:
            return False
        jobs = [(owner.data_ptr(), j) for ent, owner in todo for j in ent.jobs]
        tabs = self.job_tables.get(device)
        if tabs is None:
            # capture_builds=False: the weights' addresses do not move, so the warm-up's table serves the capture (and is then kept alive)
            tabs = self.job_tables[device] = _JobTable("the weight-plane refresh", _PLANE_JOB, ops.weight_planes_job_bytes,
                                                       capture_builds=False)
        tab = tabs.get(tuple((base + j["off"],) + j["fields"] + j["sel"] for base, j in jobs), device, lambda: pack_plane_jobs(jobs))
        if tab is None:
            return False  # (a capture whose warm-up did not see this set of weights: no host-to-device copy inside it — one by one, as before)
        with torch.no_grad():
            ops.weight_planes_multi(tab.jobs, tab.blk2job, tab.blocks)
        for ent, owner in todo:
            ent.version, ent.gen = owner._version, self.gen
        cur = torch.cuda.current_stream(device)
        event = torch.cuda.Event()
        event.record(cur)
        self.refreshed[device] = (event, cur.cuda_stream, set())
        CALLS["planes_multi"] += 1
        return True

    def lookup(self, key, owner):
        """The value under `key` if it is `owner`'s and current — made current, together with every other stale entry, by one launch
        when only the optimizer step lies between (same tensors, new values) — else None."""
        ent = self.entries.get(key)
        if ent is None or ent.ref() is not owner:
            return None
        if ent.stale(owner):
            if not (_PLANES_MULTI and ent.jobs and owner.is_cuda and self.refresh(owner.device)) or ent.stale(owner):
                return None
        r = self.refreshed.get(owner.device) if owner.is_cuda else None
        if r is not None and ent.jobs:  # the launch that wrote these planes ran on another stream: behind it, once
            raw = _RAW_STREAM(owner.device.index) if _RAW_STREAM is not None else torch.cuda.current_stream(owner.device).cuda_stream
            if raw != r[1] and raw not in r[2]:
                torch.cuda.current_stream(owner.device).wait_event(r[0])
                r[2].add(raw)
        return ent.value

    def store(self, key, owner, value, jobs=None):
        if len(self.entries) > 4096:  # entries of models that are gone
            for k in [k for k, v in self.entries.items() if v.ref() is None]:
                del self.entries[k]
        self.entries[key] = _PlaneEntry(self, owner, value, jobs)


CACHE = PlaneCache()

# Optimizers that update their parameters without moving Tensor._version — torch's FUSED kernels (SGD / Adam(W) with fused=True:
# measured, _version 0 -> 0 over optimizer.step(), tools/experimental/debug_sgd_arena.py), updates through `.data` — would leave the
# version-keyed cache serving the OLD weights to every convolution after them.  Every optimizer step of the process therefore marks
# the cache stale (one global hook; the next lookup re-makes all planes in one launch, which a version bump would have asked for too).
try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _register_step_hook

    _STEP_HOOK = _register_step_hook(lambda *_a, **_k: CACHE.invalidate())
except ImportError:  # (torch < 2.0: callers invalidate by hand, as train() always has)
    _STEP_HOOK = None


def _row_scaled_planes(wt):
    """fp16 planes of rows scaled by a power of two into [2^9, 2^10), undone on the accumulator (fused_slowfast.FusedConv)
    -> hi, lo, the scales.  The bits of csrc/stem_train.hip's weight_planes_row: the maximum skips NaNs (fmaxf), its exponent comes from
    frexp — mx = m * 2^e, m in [0.5, 1), scale 2^(10 - e), assembled as the fp32 word (127 + 10 - e) << 23: exact on every device.
    (2^(9 - floor(log2(mx))) was half of it for a maximum one ulp below a power of two, where fp32 log2 rounds up to the integer; an
    infinity, whose frexp exponent is 0 here as on the device, made the scale 0 and the row NaNs; a NaN made the whole row NaNs.)"""
    mx = wt.abs().nan_to_num_(nan=0.0, posinf=float("inf")).amax(dim=1).clamp_min(1e-30)
    sc = (137 - torch.frexp(mx)[1]).to(torch.int32).bitwise_left_shift_(23).view(torch.float32)
    hi, lo = split_planes(wt * sc.view(-1, 1), ops.X3_F16)
    return hi, lo, sc


def _weight_planes(weight, transposed):
    """(hi, lo, wscale) planes of a Conv3d weight in the kernel's [Cout, taps * Cin] order, cached until the optimizer
    changes the tensor.  transposed: the dgrad filter W'[ci, co, flipped taps], as bf16 planes."""
    # keyed on the tensor that OWNS the storage: conv2d hands over `conv.weight.unsqueeze(2)`, a fresh view per call, which never
    # hit the cache and left an entry per call behind; a view shares its base's version counter
    owner = weight._base if weight._base is not None else weight
    key = (id(owner), bool(transposed), tuple(weight.shape))
    hit = CACHE.lookup(key, owner)
    if hit is not None:
        return hit
    jobs = None
    with torch.no_grad():
        w = weight.detach()
        fast = (_PLANES_HIP and w.dtype == torch.float32 and w.dim() == 5 and w.shape[1] % 8 == 0 and w.shape[0] % 2 == 0 and
                w.is_contiguous(memory_format=torch.channels_last_3d) and w.shape[2] * w.shape[3] * w.shape[4] <= 32)
        if fast:  # two launches per convolution and step instead of ~35 torch ops (the memory of a channels-last weight is
            #       already [cout][taps][cin], the kernels' K order)
            cout, cin = w.shape[0], w.shape[1]
            taps = w.shape[2] * w.shape[3] * w.shape[4]
            rows = w.permute(0, 2, 3, 4, 1).reshape(cout, taps * cin)  # a view
            if transposed:
                sel = list(range(taps - 1, -1, -1))
                planes = ops.weight_planes_t_f32(rows.view(cout, taps, cin), sel) + (None,)
                jobs = [_job_transposed(rows, owner, planes[0], planes[1], cout, taps, cin, sel)]
            else:
                planes = ops.weight_planes_f32(rows, ops.X3_F16)
                jobs = [_job_rows(rows, owner, planes[0], planes[1], planes[2], True, cout, taps * cin)]
        else:
            w = w.float()
            if w.shape[1] % 8:  # the stems' 3 input channels, padded with zero taps
                w = torch.cat([w, w.new_zeros((w.shape[0], 8 - w.shape[1] % 8) + tuple(w.shape[2:]))], 1)
            if transposed:
                w = w.flip(2, 3, 4).transpose(0, 1)
            wt = w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1)
            if transposed:
                hi, lo = split_planes(wt, ops.X3_BF16)
                planes = (hi, lo, None)
            else:
                hi, lo, sc = _row_scaled_planes(wt)
                planes = (hi, lo, (1.0 / sc).float().contiguous())
    CACHE.store(key, owner, planes, jobs)
    return planes


# ---- few-channel layers: g adjacent pixels along W as g * C channels (why and when: train_ops._conv_form)
_GROUP_IDX = {}
_GROUP_MAPS = {}  # (shape, strides, g, transposed, device) -> int32 [rows, cols] storage offsets of the grouped rows (-1: a zero tap)


def _grouped_rows(w, g, transposed):
    """The pixel-grouped row form of a [cout, cin, kt, kh, kw] tensor (the weight itself, or — round 6 — the tensor of its storage
    offsets): rows [(po, n)][(dt, dh, dg)][(pi, c)], block-Toeplitz along W over groups of g pixels; `pad` fills the taps no original
    tap meets.  -> rows [g * co, kt * kh * kwg * g * ci], (kt, kh, kwg), rg."""
    pad = 0 if w.is_floating_point() else -1
    if transposed:
        w = w.flip(2, 3, 4).transpose(0, 1)  # the input gradient as a convolution of dY: filter [cin][cout][flipped taps]
    co, ci, kt, kh, kw = w.shape
    r = kw // 2
    rg = -(-r // g)
    kwg = 1 + 2 * rg
    ikey = (g, kw, str(w.device))
    idx = _GROUP_IDX.get(ikey)
    if idx is None:  # tap of the ORIGINAL filter that (output pixel po, input pixel pi, group tap dg) meets; kw = the zero tap
        po, pi, dg = torch.meshgrid(torch.arange(g), torch.arange(g), torch.arange(kwg), indexing="ij")
        dw = g * (dg - rg) + pi - po + r
        idx = torch.where((dw >= 0) & (dw < kw), dw, torch.full_like(dw, kw)).to(w.device)
        _GROUP_IDX[ikey] = idx
    w_ext = torch.cat([w, w.new_full((co, ci, kt, kh, 1), pad)], 4)
    wg = w_ext[..., idx]  # [co, ci, kt, kh, po, pi, dg]
    rows = wg.permute(4, 0, 2, 3, 6, 5, 1).reshape(g * co, kt * kh * kwg * g * ci).contiguous()
    return rows, (kt, kh, kwg), rg


def _grouped_planes(weight, g, transposed, plane_dtype):
    """Planes of the pixel-grouped form of a Conv3d weight (transposed: of the input gradient's filter W'[ci][flipped taps][co])
    -> (hi, lo, wscale | None), (kt, kh, kwg), rg.  The grouped rows are a fixed GATHER of the weight's elements: the map of storage
    offsets is built once per (shape, layout, g, direction) by running the assembly on the offsets themselves, and every step is one
    launch (ops.weight_planes_gather_f32) instead of a flip, a cat, an index, a permute and a copy in front of the split."""
    key = (id(weight), "group", g, bool(transposed))
    hit = CACHE.lookup(key, weight)
    if hit is not None:
        return hit
    jobs = None
    with torch.no_grad():
        w = weight.detach()
        dense = w.dtype == torch.float32 and (w.is_contiguous() or w.is_contiguous(memory_format=torch.channels_last_3d))
        if _GROUP_GATHER and dense and w.is_cuda and w.numel() < (1 << 31):
            mkey = (tuple(w.shape), tuple(w.stride()), g, bool(transposed), str(w.device))
            ent = _GROUP_MAPS.get(mkey)
            if ent is None:
                offs = torch.arange(w.numel(), dtype=torch.int32).as_strided(tuple(w.shape), tuple(w.stride()))  # element -> storage offset
                rows, kern, rg = _grouped_rows(offs, g, transposed)
                ent = (rows.to(torch.int32).contiguous().to(w.device), kern, rg)
                _GROUP_MAPS[mkey] = ent
            pl = ops.weight_planes_gather_f32(w, ent[0], plane_dtype)
            planes = (pl, ent[1], ent[2])
            jobs = [_job_rows(w, weight, pl[0], pl[1], pl[2], plane_dtype == ops.X3_F16, ent[0].shape[0], ent[0].shape[1], idx_map=ent[0])]
        else:
            rows, kern, rg = _grouped_rows(w.float(), g, transposed)
            planes = (ops.weight_planes_f32(rows, plane_dtype), kern, rg)
    CACHE.store(key, weight, planes, jobs)
    return planes


def _stride_classes(k, s, p, x, y):
    """One dimension of a strided convolution's input gradient: for every residue r of the input index mod s, the taps that
    reach it (descending, so that the offsets into dY ascend), the padding in front of dY and the number of input positions
    -> [(r, taps, pad_before, count)]; None when a class would need dY shifted the other way (not a SlowFast shape)."""
    out = []
    for r in range(s):
        taps = list(range((r + p) % s, k, s))
        offs = [(r + p - d) // s for d in taps]  # descending with d ascending
        if offs and min(offs) > 0:
            return None
        out.append((r, taps[::-1], -min(offs) if offs else 0, max(0, -(-(x - r) // s))))
    return out


def _strided_planes(weight, kernel, stride, padding, grid, out):
    """The filters of a strided convolution's input gradient over the input grid (t, h, w) and dY's extents `out`, one per residue class
    of the input position modulo the stride (train_ops._dgrad_strided launches them) -> [((rt, rh, rw), None when no tap reaches the
    class, else (hi, lo bf16 planes of the class's taps, transposed; its kernel; the padding in front of dY; its positions))], or None
    outside the domain of _stride_classes."""
    cube = tuple(stride) == (2, 2, 2)
    key = (id(weight), "strided", tuple(stride), tuple(padding)) + ((tuple(grid),) if cube else ())
    classes = CACHE.lookup(key, weight)
    if classes is not None:
        return classes
    per_dim = [_stride_classes(k, s, p, x, y) for k, s, p, x, y in zip(kernel, stride, padding, grid, out)]
    if any(c is None for c in per_dim):
        return None
    if cube and any(taps and n > y for c, y in zip(per_dim, out) for _, taps, _, n in c):
        return None  # (a class longer than dY with its far-side taps: not a 3D-ResNet shape)
    cout, cin, ntaps = weight.shape[0], weight.shape[1], kernel[0] * kernel[1] * kernel[2]
    classes, jobs = [], []
    with torch.no_grad():
        wd = weight.detach()
        fast = _PLANES_HIP and wd.dtype == torch.float32 and wd.is_contiguous(memory_format=torch.channels_last_3d) and cout % 2 == 0
        wf = None if fast else wd.float()  # [cout, cin, kt, kh, kw]
        w3 = wd.permute(0, 2, 3, 4, 1).reshape(cout, ntaps, cin) if fast else None  # a view
        for rt, dt, pbt, nt in per_dim[0]:
            for rh, dh, pbh, nh in per_dim[1]:
                for rw, dw, pbw, nw in per_dim[2]:
                    if not (dt and dh and dw):
                        classes.append(((rt, rh, rw), None))
                        continue
                    if fast:  # one launch: the class's taps (row-major over its (dt, dh, dw) lists) gathered and transposed
                        sel = [(a * kernel[1] + b) * kernel[2] + c for a in dt for b in dh for c in dw]
                        hi, lo = ops.weight_planes_t_f32(w3, sel)
                        jobs.append(_job_transposed(w3, weight, hi, lo, cout, ntaps, cin, sel))
                    else:
                        sub = wf[:, :, dt][:, :, :, dh][:, :, :, :, dw]                  # [cout, cin, |dt|, |dh|, |dw|]
                        wt = sub.transpose(0, 1).permute(0, 2, 3, 4, 1).reshape(cin, -1)   # rows ci, K = (taps, co)
                        hi, lo = split_planes(wt, ops.X3_BF16)
                    classes.append(((rt, rh, rw), (hi, lo, (len(dt), len(dh), len(dw)), (pbt, pbh, pbw), (nt, nh, nw))))
    CACHE.store(key, weight, classes, jobs if fast else None)
    return classes


def _stem_weight_image(weight, g):
    """(hi, lo, wscale, frames per tile) of a stem weight [C, 3, kt, 7, 7] in the LDS image order of csrc/stem_conv.hip: pixel-pair
    taps (column tap k -> pair tap (k + 1) // 2, pixel (k + 1) % 2; the first is a structural zero), g output frames as g * C
    channels over kt + g - 1 frame taps, fp16 planes of rows scaled into [2^9, 2^10).  Torch-assembled: no recipe, rebuilt when stale."""
    key = (id(weight), "stem", g)
    hit = CACHE.lookup(key, weight)
    if hit is not None:
        return hit
    with torch.no_grad():
        w = weight.detach().float()
        c, kt = w.shape[0], w.shape[2]
        w8 = w.new_zeros((c, kt, 7, 8, 4))
        w8[:, :, :, 1:, :3] = w.permute(0, 2, 3, 4, 1)
        wg = w.new_zeros((g, c, kt + g - 1, 7, 8, 4))
        for j in range(g):
            wg[j, :, j : j + kt] = w8
        hi, lo, sc = _row_scaled_planes(wg.reshape(g * c, -1))
        fm = g == 4 and c == 8  # frame-major tiles: the kernel skips the frame taps a tile never meets
        img = (stem_lds_image(hi, kt + g - 1, fm), stem_lds_image(lo, kt + g - 1, fm), (1.0 / sc).float().contiguous(), 2 if fm else 0)
    CACHE.store(key, weight, img)
    return img
