"""Encode-once texture engine: the MI355X restructure of the reference's stitch hot path.

The reference re-encodes every target window at every step of its stitch loop
(contrastive_video_textures/validate.py:324, 442-479 -> models/models.py:358-399): about
steps x N SlowFast forwards where 2N suffice, plus a full-video CPU gather and zero-padded re-chunk
per step (validate.py:391-395).  Here every distinct clip window is packed (HIP clip_pack) and encoded
exactly once into embedding tables that stay resident in HBM; rows of the transition matrix are then
either one MFMA GEMM (`aligned`: sim = Q_hat T_hat^T / temp, N x N) or table lookups (`compat`, which
reproduces the reference's window/label map bit for bit, quirks Q3/Q4).

Data layout in HBM (N windows, D_v = 2304, D_a = 12288):
  frames      uint8 [F,H,W,3]            the video, uploaded once
  Qv, Tv      fp32  [N, D_v]             query / target encoder outputs (two encoders: sim is not symmetric, Q7)
  A           fp32  [N, D_a]             VGGish features of the source audio examples (m=2)
  Q_hat,T_hat fp32  [N, D_v(+D_a)]       jointly L2-normalised rows (+ bf16 hi/lo copies for the bf16 MFMA modes)
  sim         fp32  [N, N]               <q_i, t_j>/temp   (67 MB at N=4096)
"""
import math

import os

import numpy as np
import torch

from . import ops
from ._lib import AvtError

# contract-grade encoders: pack every distinct frame once and hand the stems a frame table + index (ops.FrameClip) instead of
# dense per-window clips (round 4; tests set False to compare the two forms: same embeddings bit for bit)
FRAME_TABLE = True


def num_segments(n_frames, window, stride):
    return math.floor((n_frames - window) / stride)  # validate.py:189


def target_segment_ids(q_id, n_seg):
    """validate.py:369-378: [pos] + every other segment ascending (q and pos removed)."""
    pos = min(q_id + 1, n_seg - 1)
    mask = np.ones(n_seg, dtype=bool)
    mask[[q_id, pos]] = False
    return np.concatenate((np.array([pos]), np.arange(n_seg)[mask]))


def compat_window_frames(q_id, n_frames, W, S, mbs, n_gpus):
    """Frame ids every output slot of the reference row really scores, and the labels it attaches.

    Pure index arithmetic restating validate.py:369-395 (target frames, order-preserving unique,
    zero-padded chunks starting at c*S*(mbs-1) [Q4]), models.py:358-367 (each replica re-windows its
    chunk at stride S [Q3]) and validate.py:442-493 (groups of n_gpus chunks, num_valid slice).
    Returns (ids [n_out, W] int64 with -1 = zero-padding frame, os_ids_t [n_out])."""
    L = num_segments(n_frames, W, S)
    seg = target_segment_ids(q_id, L)
    fid = np.concatenate([np.arange(i * S, i * S + W) for i in seg])
    _, first = np.unique(fid, return_index=True)
    fid = fid[np.sort(first)]
    n_in = len(fid)
    chunk = mbs * S + W
    n_chunks = math.ceil(math.ceil((n_in - W) / S) / mbs)
    n_out = len(seg)
    # window w of chunk c starts at c*S*(mbs-1) + w*S in t_video coordinates
    c = np.arange(n_chunks)[:, None, None]
    w = np.arange(mbs)[None, :, None]
    k = np.arange(W)[None, None, :]
    pos = c * S * (mbs - 1) + w * S + k  # [n_chunks, mbs, W]
    inside = (w * S + k < chunk) & (pos < np.minimum(c * S * (mbs - 1) + chunk, n_in))
    ids = np.where(inside, fid[np.minimum(pos, n_in - 1)], -1).reshape(-1, W)
    # outputs are written contiguously per group of n_gpus chunks; the num_valid slice only ever cuts the tail
    out = np.full((n_out, W), -1, np.int64)
    take = min(n_out, len(ids))
    out[:take] = ids[:take]
    return out, seg


def max_enc_batch(img_size, planes=True):
    """Largest SlowFast encoder batch the hand-written kernels take at `img_size`^2: their offsets are signed 32-bit ELEMENT
    counts (csrc/conv_args.h conv_args_fill), and the widest tensor of a forward is the slow res2 input with its lateral
    channels, [n, 8, hw/4, hw/4, 64 + 16 .. 256 + 64 = 320] (267 clips at 224^2, 204 at 256^2).  The bf16 path (planes=False)
    also reads DENSE packed fast clips [n, 32, hw, hw, 4] through 32-bit BYTE offsets (2 bytes each: 166 at 224^2)."""
    q = -(-int(img_size) // 4)
    cap = ((1 << 31) - 64) // (8 * q * q * 320)
    if not planes:
        cap = min(cap, ((1 << 30) - 64) // (32 * int(img_size) ** 2 * 4) - 1)
    return max(1, cap)


def max_enc_batch_resnet3d(img_size, window):
    """Largest 3D-ResNet encoder batch the split-plane kernels take (fused_resnet3d.ResNet3dMFMA): the widest tensor of a forward is
    the stem output [n, W, ceil(hw/2), ceil(hw/2), 64], addressed with signed 32-bit element offsets (133 clips at W = 20, 224^2)."""
    h2 = -(-int(img_size) // 2)
    return max(1, ((1 << 31) - 64) // (int(window) * h2 * h2 * 64))


class TextureEngine:
    # per-channel statistics of the reference's non-SlowFast transform (validate.py:90-92, dataset.py:50-52)
    GENERIC_MEAN = (0.4345, 0.4051, 0.3775)
    GENERIC_STD = (0.2768, 0.2713, 0.2737)

    def __init__(self, q_encoder, t_encoder, audio_encoder=None, *, window, stride, temp=0.1, img_size=224,
                 model_type=1, device=None, enc_batch=32, mean=0.45, std=0.225, enc_arch="slowfast"):
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.dev.type != "cuda":
            raise AvtError("TextureEngine needs an MI355X device; the hot path has no CPU fallback")
        self.q_enc, self.t_enc, self.a_enc = q_encoder, t_encoder, audio_encoder
        self.W, self.S, self.temp, self.hw = int(window), int(stride), float(temp), int(img_size)
        self.model_type = model_type
        self.slowfast = enc_arch == "slowfast"  # else: plugin encoders taking [B,C,T,H,W] (models.py:253-260)
        self.enc_batch = int(enc_batch)
        self.mean, self.std = mean, std
        p = next(q_encoder.parameters(), None)
        self.pack_dtype = p.dtype if p is not None and p.dtype in (torch.bfloat16, torch.float32) else torch.float32
        # encoders built on the MFMA conv kernel take channels-last clips directly (fused_slowfast.SlowFastMFMA)
        self.layout = "ndhwc4" if all(getattr(e, "input_layout", None) == "ndhwc4" for e in (q_encoder, t_encoder)) \
            else "ncthw"
        # contract-grade MFMA encoders read split-plane clips (ops.SplitClip); both encoders must agree on the format
        self.planes = getattr(q_encoder, "planes", None) if self.layout == "ndhwc4" else None
        if self.layout == "ndhwc4" and getattr(t_encoder, "planes", None) != self.planes:
            raise AvtError("q and t encoders must use the same precision mode (they share the packed clips)")
        if self.layout == "ndhwc4" and self.slowfast:
            # the MFMA kernels address a tensor with signed 32-bit element offsets: the batch is cut to what the widest
            # activation of THIS image size allows (the default of 249 is the 224^2 figure, 256^2 needs <= 204)
            cap = max_enc_batch(self.hw, self.planes is not None)
            if self.enc_batch > cap:
                self.enc_batch = cap
        # 3D-ResNet encoders on the split-plane kernels (fused_resnet3d.ResNet3dMFMA): set_video writes the normalised frames once
        # as a plane-pair table and embed_windows hands the encoders frame ids only — no clip is gathered per window
        self.frame_table = not self.slowfast and all(getattr(e, "frame_table_input", False) for e in (q_encoder, t_encoder))
        if self.frame_table:
            self.enc_batch = min(self.enc_batch, max_enc_batch_resnet3d(self.hw, self.W))
        self.frames = None
        self.A = self.A_da = self.Ad = None
        self._cache = {"q": {}, "t": {}}
        self._rows = {"q": None, "t": None}
        self._nrows = {"q": 0, "t": 0}
        self.encoded = 0  # windows pushed through an encoder (both encoders counted)
        # q / t encoders on two HIP streams: +8-13 % for the bf16 path; the contract-grade kernels (one workgroup per CU on their
        # XL / fused-block launches) fill the chip from one stream and measured 1.4 % slower with two
        self.n_streams = 1 if getattr(q_encoder, "x3", None) is not None else 2
        self._streams = None
        self._pending, self._inflight = [], []  # run_encoders(join=False): outputs / per-batch events not yet joined

    # ---- inputs -------------------------------------------------------------------
    def set_video(self, video_u8):
        """video_u8: uint8 [F,H,W,3] RGB, host or device (validate.py:79)."""
        v = torch.as_tensor(video_u8)
        if v.dtype != torch.uint8 or v.dim() != 4 or v.shape[3] != 3:
            raise AvtError("set_video expects uint8 [F,H,W,3]")
        self.frames = v.to(self.dev).contiguous()
        self.F = self.frames.shape[0]
        self.N = num_segments(self.F, self.W, self.S)
        # one all-zero frame appended for the zero padding of the compat path (utils.py:252)
        self._frames_pad = torch.cat([self.frames, torch.zeros_like(self.frames[:1])], 0)
        if not self.slowfast:
            # validate.py:85-93, 116-118: ToPILImage/Resize/ToTensor/Normalize per frame, RGB.  Device torch ops; the
            # resize (only when the frame is not img_size already) is antialiased bilinear like PIL's — unpinned.
            x = self.frames.permute(0, 3, 1, 2).float() / 255
            if x.shape[-2:] != (self.hw, self.hw):
                x = torch.nn.functional.interpolate(x, size=(self.hw, self.hw), mode="bilinear", antialias=True)
            m = torch.tensor(self.GENERIC_MEAN, device=self.dev).view(1, 3, 1, 1)
            sd = torch.tensor(self.GENERIC_STD, device=self.dev).view(1, 3, 1, 1)
            x = ((x - m) / sd).to(self.pack_dtype)
            self._norm_pad = torch.cat([x, torch.zeros_like(x[:1])], 0)  # padding is zero AFTER the transform
            if self.frame_table:  # ... as NDHWC plane pairs [F+1, hw, hw, 4] (channel 3 zero), one pass over the video
                hi, lo = ops.clip_planes_f32(self._norm_pad.permute(1, 0, 2, 3).unsqueeze(0), self.q_enc.x3)
                self._table = (hi[0], lo[0])
        return self.N

    def set_audio(self, audio_eg, driving_eg=None, da_encoder=None):
        """audio_eg [n,1,100,64] fp32 log-mel examples of the source (validate.py:159-161, cut to N at :192);
        driving_eg likewise for the driving audio; da_encoder = the separate VGGish the reference loads for
        the driving branch (validate.py:264-266; models.py:424-431 runs it on source AND driving examples).
        VGGish runs once per table, not once per step."""
        eg = torch.as_tensor(audio_eg)[: self.N]
        with torch.no_grad():
            if self.model_type == 2:
                if self.a_enc is None:
                    raise AvtError("model_type 2 needs an audio encoder")
                self.A = self._vgg(self.a_enc, eg)
            if driving_eg is not None:
                da = da_encoder if da_encoder is not None else self.a_enc
                if da is None:
                    raise AvtError("driving audio needs a VGGish encoder")
                self.A_da = self.A if (da is self.a_enc and self.A is not None) else self._vgg(da, eg)
                self.Ad = self._vgg(da, torch.as_tensor(driving_eg))

    def audio_block(self, audio_eg, lo, hi):
        """Rows [lo, hi) of the m=2 source-audio table: VGGish(audio_eg[min(j, max_audio_segment_id)]) (validate.py:346,
        398-401) — what a rank of the sharded build needs, instead of set_audio()'s whole table."""
        if self.a_enc is None:
            raise AvtError("model_type 2 needs an audio encoder")
        eg = torch.as_tensor(audio_eg)[: self.N]
        j = torch.clamp(torch.arange(lo, hi), max=eg.shape[0] - 1)
        with torch.no_grad():
            return self._vgg(self.a_enc, eg[j.to(eg.device)])

    def _vgg(self, enc, eg, batch=256):
        p = next(enc.parameters())
        outs = [enc(eg[i : i + batch].to(self.dev, p.dtype)).float() for i in range(0, len(eg), batch)]
        return torch.cat(outs, 0).contiguous()

    # ---- packing + encoding ----------------------------------------------------------
    def _pack(self, frames, starts):
        lo, hi = int(starts.min()), int(starts.max()) + self.W
        # (the table's slow stem runs on EVERY frame of [lo, hi): worth it while that is no more than the 8 slow frames per window
        #  the dense form convolves — overlapping windows, the default; windows scattered more thinly keep the dense clips)
        if self.planes is not None and self.layout == "ndhwc4" and FRAME_TABLE and hi - lo <= len(starts) * 8:
            # contract-grade encoders: every distinct frame packed once, the windows' sampling as an index (ops.FrameClip);
            # windows scattered so thinly that the span holds more frames than the dense clips would keep the dense form
            return ops.clip_pack_frames(frames[lo:hi], starts - lo, self.W, out_hw=self.hw, mean=self.mean, std=self.std,
                                        bgr=True, planes=self.planes)
        return ops.clip_pack(frames[lo:hi], starts - lo, self.W, out_hw=self.hw, mean=self.mean, std=self.std,
                             bgr=True, dtype=self.pack_dtype, layout=self.layout, planes=self.planes)

    def _run(self, enc, slow, fast):
        if self.layout == "ndhwc4":
            return enc.forward_ndhwc4(slow, fast).float()
        return enc([slow, fast]).float()

    def run_encoders(self, encoders, slow, fast, join=True):
        """Every encoder on the same packed clips.  Two encoders (query / target) run on separate HIP streams: their
        kernels are independent, and interleaving them fills the tail of each ~0.2 ms convolution launch with the
        other encoder's workgroups (+8-13 % windows/s measured, bit-identical outputs).  self.n_streams = 4 also
        splits the clip batch in halves (four independent forward chains).
        join=False: the caller's stream does NOT wait for the encoder streams — it goes on packing the next batch while
        they work, and each encoder stream runs its batches back to back (no per-batch rendezvous of the two streams,
        which idles one of them at every batch end and keeps the two forwards in lockstep).  The outputs may then only be
        used after join_streams().  At most two batches of packed clips are in flight."""
        if len(encoders) != 2 or self.n_streams <= 1:
            return [self._run(e, slow, fast) for e in encoders]
        main = torch.cuda.current_stream()
        if self._streams is None or len(self._streams) < self.n_streams:
            self._streams = ops.side_streams(self.dev, self.n_streams)  # (process-wide: see ops.side_streams)
        parts = 2 if self.n_streams >= 4 and slow.shape[0] >= 2 else 1
        sl, fa = slow.chunk(parts), fast.chunk(parts)
        tasks = [(e, k) for k in range(parts) for e in range(2)]
        outs, on = {}, {}
        for st, (e, k) in zip(self._streams, tasks):
            st.wait_stream(main)  # the clips were packed on `main`
            with torch.cuda.stream(st):
                outs[(e, k)] = self._run(encoders[e], sl[k], fa[k])
            on[(e, k)] = st
            slow.record_stream(st)
            fast.record_stream(st)
        res = []
        for e in range(2):
            if parts == 1:
                res.append(outs[(e, 0)])
                continue
            # the two halves of encoder e are concatenated on the stream of its FIRST half, after that stream has waited
            # for the second half's: never on the caller's stream, which (join=False) has not waited for either
            s0, s1 = on[(e, 0)], on[(e, 1)]
            s0.wait_stream(s1)
            with torch.cuda.stream(s0):
                res.append(torch.cat([outs[(e, 0)], outs[(e, 1)]], 0))
            outs[(e, 1)].record_stream(s0)
        if join:
            for st in self._streams[: len(tasks)]:
                main.wait_stream(st)
            for o in res:
                o.record_stream(main)
        else:
            done = []
            for st in self._streams[: len(tasks)]:
                ev = torch.cuda.Event()
                ev.record(st)
                done.append(ev)
            self._pending.extend(res)
            self._inflight.append(done)
            if len(self._inflight) > 2:  # bound the packed clips in flight: the NEXT pack waits for the batch before last
                for ev in self._inflight.pop(0):
                    main.wait_event(ev)
        return res

    def join_streams(self):
        """After run_encoders(..., join=False): the current stream waits for every encoder stream; the outputs returned
        since the last join become usable on it."""
        main = torch.cuda.current_stream()
        for st in self._streams or []:
            main.wait_stream(st)
        for o in self._pending:
            o.record_stream(main)
        self._pending, self._inflight = [], []

    def embed_windows(self, encoders, starts=None, ids=None):
        """Packs each window ONCE and runs every encoder in `encoders` on it -> list of fp32 [n,D]."""
        n = len(starts) if starts is not None else len(ids)
        outs = [[] for _ in encoders]
        if not self.slowfast:
            if ids is None:
                ids = np.asarray(starts, np.int64)[:, None] + np.arange(self.W)[None, :]
            with torch.no_grad():
                for i in range(0, n, self.enc_batch):
                    part = np.asarray(ids[i : i + self.enc_batch], np.int64)
                    if self.frame_table:
                        fidx = torch.from_numpy(np.where(part < 0, self.F, part).reshape(-1).astype(np.int32)).to(self.dev)
                        for k, enc in enumerate(encoders):
                            outs[k].append(enc.forward_frames(self._table[0], self._table[1], fidx, len(part), self.W))
                        self.encoded += len(part) * len(encoders)
                        continue
                    flat = torch.from_numpy(np.where(part < 0, self.F, part).reshape(-1)).to(self.dev)
                    x = self._norm_pad.index_select(0, flat).view(len(part), self.W, 3, self.hw, self.hw)
                    x = x.permute(0, 2, 1, 3, 4).contiguous()  # (B,window,C,H,W) -> (B,C,window,H,W), models.py:332
                    for k, enc in enumerate(encoders):
                        outs[k].append(enc(x).float().view(len(part), -1))
                    self.encoded += len(part) * len(encoders)
            return [torch.cat(o, 0).contiguous() for o in outs]
        with torch.no_grad():
            for i in range(0, n, self.enc_batch):
                if starts is not None:
                    slow, fast = self._pack(self.frames, np.asarray(starts[i : i + self.enc_batch], np.int64))
                else:  # explicit frame-id windows (spliced / zero padded): gather them into a scratch clip
                    part = np.asarray(ids[i : i + self.enc_batch], np.int64)
                    flat = torch.from_numpy(np.where(part < 0, self.F, part).reshape(-1)).to(self.dev)
                    scratch = self._frames_pad.index_select(0, flat)
                    slow, fast = self._pack(scratch, np.arange(len(part), dtype=np.int64) * self.W)
                for k, o in enumerate(self.run_encoders(encoders, slow, fast, join=False)):
                    outs[k].append(o)
                self.encoded += slow.shape[0] * len(encoders)
            self.join_streams()
        return [torch.cat(o, 0).contiguous() for o in outs]

    # ---- aligned mode: tables + one N x N GEMM --------------------------------------------
    def build_tables(self):
        starts = np.arange(self.N, dtype=np.int64) * self.S
        self.Qv, self.Tv = self.embed_windows([self.q_enc, self.t_enc], starts=starts)
        return self.Qv, self.Tv

    def normalise(self, split=False):
        a = self.A if self.model_type == 2 else None
        if a is not None and a.shape[0] < self.N:  # audio_eg[min(idx, max_audio_segment_id)] (validate.py:346, 398-401)
            a = a[torch.clamp(torch.arange(self.N, device=self.dev), max=a.shape[0] - 1)].contiguous()
        self.Qn, self.Qh, self.Ql = ops.l2norm_rows(self.Qv, a, want_split=split)
        self.Tn, self.Th, self.Tl = ops.l2norm_rows(self.Tv, a, want_split=split)
        return self.Qn, self.Tn

    def similarity(self, precision="f32", out=None):
        if precision == "f32":
            self.sim = ops.sim_gemm_nt(self.Qn, self.Tn, self.temp, "f32", out=out)
        else:
            self.sim = ops.sim_gemm_nt(self.Qh, self.Th, self.temp, precision, q_lo=self.Ql, t_lo=self.Tl, out=out)
        return self.sim

    def driving_similarity(self):
        """sim_a[k, j] = <vgg(driving_k), vgg(audio_j)>/temp (models.py:424-439, :457)."""
        dn, _, _ = ops.l2norm_rows(self.Ad)
        a = self.A_da
        if a.shape[0] < self.N:  # audio_eg[min(idx, max_audio_segment_id)] (validate.py:346, 398-401), as normalise() does
            a = a[torch.clamp(torch.arange(self.N, device=self.dev), max=a.shape[0] - 1)].contiguous()
        an, _, _ = ops.l2norm_rows(a)
        self.sim_a = ops.sim_gemm_nt(dn, an, self.temp, "f32")
        return self.sim_a

    def transitions(self, threshold, cap=64, alpha=0.5):
        """Row post-process (validate.py:524-572) for every query segment at once."""
        q_ids = torch.arange(self.N, device=self.dev, dtype=torch.int64)
        return ops.row_transition(self.sim, q_ids=q_ids, threshold=threshold, alpha=alpha, cap=cap)

    def aligned_row(self, q_id, step_iter, threshold, alpha=0.5):
        """One stitch step from the resident tables -> (choices positions, os_ids_t, stats)."""
        q = torch.tensor([q_id], device=self.dev, dtype=torch.int64)
        sa = None
        if self.Ad is not None:
            if not hasattr(self, "sim_a"):
                self.driving_similarity()
            sa = self.sim_a[step_iter : step_iter + 1]
        sel = ops.row_transition(self.sim[q_id : q_id + 1], q_ids=q, sim_a=sa, alpha=alpha, threshold=threshold,
                                 cap=self.N)
        k = int(sel["cnt"][0])
        return sel["idx"][0, :k].cpu().numpy(), sel["seg"][0, :k].cpu().numpy(), sel

    # ---- compat mode: the reference's rows, window for window ------------------------------------
    def _lookup(self, which, enc, keys, windows):
        cache = self._cache[which]
        miss = [i for i, k in enumerate(keys) if k not in cache]
        seen, uniq = set(), []
        for i in miss:
            if keys[i] not in seen:
                seen.add(keys[i])
                uniq.append(i)
        if uniq:
            contig = [i for i in uniq if keys[i][0] == "c"]
            other = [i for i in uniq if keys[i][0] != "c"]
            new = []
            if contig:
                new.append((contig, self.embed_windows([enc], starts=np.array([keys[i][1] for i in contig]))[0]))
            if other:
                new.append((other, self.embed_windows([enc], ids=np.stack([windows[i] for i in other]))[0]))
            for idxs, emb in new:
                base = self._nrows[which]
                need = base + emb.shape[0]
                tab = self._rows[which]
                if tab is None or need > tab.shape[0]:
                    grown = torch.empty((max(need, 2 * (0 if tab is None else tab.shape[0]), 256), emb.shape[1]),
                                        dtype=torch.float32, device=self.dev)
                    if tab is not None:
                        grown[:base] = tab[:base]
                    self._rows[which] = tab = grown
                tab[base:need] = emb
                for j, i in enumerate(idxs):
                    cache[keys[i]] = base + j
                self._nrows[which] = need
        idx = torch.tensor([cache[k] for k in keys], device=self.dev, dtype=torch.int64)
        return self._rows[which].index_select(0, idx)

    @staticmethod
    def _key(ids):
        if ids[0] >= 0 and np.all(np.diff(ids) == 1):
            return ("c", int(ids[0]))
        return tuple(int(x) for x in ids)

    def compat_row(self, q_id, step_iter, mbs, n_gpus=1):
        """Raw logits row exactly as the reference assembles it -> (out [n_out], out_a | None, os_ids_t)."""
        wins, seg = compat_window_frames(q_id, self.F, self.W, self.S, mbs, n_gpus)
        tv = self._lookup("t", self.t_enc, [self._key(w) for w in wins], wins)
        qw = np.arange(q_id * self.S, q_id * self.S + self.W)
        qv = self._lookup("q", self.q_enc, [self._key(qw)], [qw])
        ta = qa = None
        if self.model_type == 2:
            mx = self.A.shape[0] - 1
            aidx = torch.from_numpy(np.minimum(seg, mx)).to(self.dev)
            ta = self.A.index_select(0, aidx)
            qa = self.A[min(q_id, mx)].unsqueeze(0).contiguous()
        qn, _, _ = ops.l2norm_rows(qv, qa)
        tn, _, _ = ops.l2norm_rows(tv, ta)
        out = ops.sim_gemm_nt(qn, tn, self.temp, "f32")
        out_a = None
        if self.Ad is not None:
            mx = self.A_da.shape[0] - 1
            sa = self.A_da.index_select(0, torch.from_numpy(np.minimum(seg, mx)).to(self.dev))
            dn, _, _ = ops.l2norm_rows(self.Ad[step_iter].unsqueeze(0).contiguous())
            sn, _, _ = ops.l2norm_rows(sa)
            out_a = ops.sim_gemm_nt(dn, sn, self.temp, "f32")
        return out, out_a, seg

    @staticmethod
    def select(out, out_a, threshold, alpha=0.5):
        """validate.py:524-572 on an assembled row (identity column order)."""
        sel = ops.row_transition(out, sim_a=out_a, alpha=alpha, threshold=threshold, cap=out.shape[1])
        k = int(sel["cnt"][0])
        return sel["idx"][0, :k].cpu().numpy(), sel
