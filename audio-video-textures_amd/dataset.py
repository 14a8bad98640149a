"""`AudioVideoSegments` — the training / validation dataset plugin, drop-in for
contrastive_video_textures/dataset/dataset.py:24-253 (same constructor, __len__, item tuples, and the
same NumPy RNG consumption in the negative sampling, :183-190).

Host side by design: it only picks indices and slices the video held in RAM.  `segment_plan(idx)` exposes
the window starts of an item so a trainer can pack them on the MI355X with ops.clip_pack instead of the
per-item CPU preprocessing of dataset.py:145-209.
"""
import copy
import math
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from .audio_frontend import waveform_to_examples, waveform_to_examples_device
from .models import process_cv2_inputs
from .validate import load_audio, read_video


class AudioVideoSegments(Dataset):
    def __init__(self, args, video_name, split="train", video=None, audio=None):
        self.vdata, self.adata = args.vdata, args.adata
        self.video_name, self.split = video_name, split
        self.n_negs = args.n_negs
        self.crop_size = self.img_size = args.img_size
        self.enc_arch = args.enc_arch
        if video is None:
            self.video_filename = os.path.join(self.vdata, "{}.mp4".format(video_name))
            self.video_u8, fps = read_video(self.video_filename)
        else:
            self.video_u8, fps = torch.as_tensor(video[0]), video[1]
        self.fps = fps
        if self.enc_arch != "slowfast":
            # dataset.py:44-58 (ToPILImage/Resize/ToTensor/Normalize); resize by antialiased bilinear
            mean = torch.tensor([0.4345, 0.4051, 0.3775]).view(1, 3, 1, 1)
            std = torch.tensor([0.2768, 0.2713, 0.2737]).view(1, 3, 1, 1)
            v = self.video_u8.permute(0, 3, 1, 2).float() / 255
            if v.shape[-1] != args.img_size or v.shape[-2] != args.img_size:
                v = F.interpolate(v, size=(args.img_size, args.img_size), mode="bilinear", antialias=True)
            self.video = (v - mean) / std
        else:
            self.video = (self.video_u8.float() / 255)[:, :, :, [2, 1, 0]]  # dataset.py:68-73: 0-1, BGR
        print("Frame shape: ", self.video[0].shape)
        # Window of 0.5 seconds, stride of 0.2 seconds — overrides -w/-stride [quirk Q10] (dataset.py:78-80)
        args.window = math.ceil(self.fps / 2)
        args.stride = math.ceil(self.fps / 5)
        print("Stride {} Window {}".format(args.stride, args.window))
        self.stride, self.window = args.stride, args.window
        if self.adata is None and audio is None:
            # dummy audio (dataset.py:87-93); consumes the torch RNG in this order
            self.audio_w = torch.rand(len(self.video) * 10)
            self.apf = 10
            self.audio_eg = torch.rand((math.floor((len(self.video) - self.window) / self.stride)), 10)
        else:
            if audio is None:
                path = os.path.join(self.adata, "{}.wav".format(video_name))
                assert os.path.exists(path) or os.path.exists(os.path.splitext(path)[0] + ".npz"), \
                    "No audio found at {}".format(path)
                audio = path
            # --audio_resample / --audio_load_sr: with kaiser_best and --train_input device the waveform is resampled and its
            # examples are built on the MI355X (and stay there, where DeviceSegmentBatcher wants them); on the host otherwise
            resampler, load_sr = getattr(args, "audio_resample", "scipy"), int(getattr(args, "audio_load_sr", 0) or 0)
            dev = None
            if resampler == "kaiser_best" and getattr(args, "train_input", "loader") == "device":
                dev = torch.device("cuda", torch.cuda.current_device())
            self.audio_w, self.sr = load_audio(audio, load_sr, resampler, dev)
            self.apf = math.floor(self.sr / self.fps)
            if dev is not None:
                if not torch.is_tensor(self.audio_w):
                    self.audio_w = np.asarray(self.audio_w)
                self.audio_w = self.audio_w[: len(self.video) * self.apf]
                self.audio_eg = waveform_to_examples_device(self.audio_w, self.sr, dev, resampler).unsqueeze(dim=1)
                self.audio_w = torch.as_tensor(self.audio_w)
            else:
                self.audio_w = np.asarray(self.audio_w)[: len(self.video) * self.apf]
                self.audio_eg = torch.from_numpy(waveform_to_examples(self.audio_w, self.sr, resampler)).unsqueeze(dim=1).float()
                self.audio_w = torch.tensor(self.audio_w)

    def __len__(self):
        n = math.floor((len(self.video) - self.window) / self.stride)
        return n - 1 if self.split == "train" else n

    def sample_ids(self, idx):
        """Segment ids of an item: (positive id, negative ids) with dataset.py:128-139, 181-190 semantics:
        n_negs drawn without replacement, then the first len(hard) overwritten by the 8 temporal neighbours
        (idx-4..idx-1, idx+2..idx+5) that fall in [0, len] — duplicates possible [quirk]."""
        n = self.__len__()
        if self.split == "train":
            pos = idx + 1
            neg_ids = np.arange(n + 1)
            mask = np.ones(n + 1, dtype=bool)
            mask[[idx, idx + 1]] = False
        else:
            pos = (idx + 1) % n
            neg_ids = np.arange(n)
            mask = np.ones(n, dtype=bool)
            mask[[idx, pos]] = False
        neg = neg_ids[mask, ...]
        if self.split == "train":
            neg = np.random.choice(neg, self.n_negs, replace=False)
            hard = np.array([idx - 4, idx - 3, idx - 2, idx - 1, idx + 2, idx + 3, idx + 4, idx + 5])
            hard = hard[hard >= 0]
            hard = hard[hard <= n]
            neg[: len(hard)] = hard
        return pos, neg

    def segment_plan(self, idx):
        """Window start frames (query, [positive] + negatives) for device-side packing."""
        pos, neg = self.sample_ids(idx)
        return idx * self.stride, np.concatenate(([pos], neg)) * self.stride

    def _clip(self, start):
        S, W = self.stride, self.window
        if self.enc_arch != "slowfast":
            return self.video[start : start + W]
        return [F.interpolate(item.squeeze(0), size=(self.img_size, self.img_size), mode="bilinear")
                for item in process_cv2_inputs(self.video[start : start + W])]

    def __getitem__(self, idx):
        S, W = self.stride, self.window
        pos, neg = self.sample_ids(idx)
        q_v = self._clip(idx * S)
        q_aw = self.audio_w[idx * S * self.apf : (idx * S + W) * self.apf]
        q_ae = self.audio_eg[idx]
        t_v = [self._clip(pos * S)] + [self._clip(int(i) * S) for i in neg]
        t_aw = [self.audio_w[pos * S * self.apf : (pos * S + W) * self.apf]]
        t_aw += [self.audio_w[int(i) * S * self.apf : (int(i) * S + W) * self.apf] for i in neg]
        pos_ae = idx + 1 if self.split == "train" else pos  # dataset.py:179 uses idx+1
        t_ae = [self.audio_eg[pos_ae]] + list(self.audio_eg[neg])
        if self.enc_arch == "slowfast":
            t_v = copy.deepcopy([torch.stack([x[k] for x in t_v]) for k in range(2)])
        else:
            t_v = torch.stack(t_v)
        t_aw, t_ae = torch.stack(t_aw), torch.stack(t_ae)
        if self.split == "train":
            return (q_v, q_aw, q_ae, t_v, t_aw, t_ae)
        ordering = torch.cat((torch.tensor([pos]), torch.tensor(neg)))
        return (q_v, q_aw, q_ae, t_v, t_aw, t_ae, idx, ordering)


class DeviceSegmentBatcher:
    """Training batches assembled ON the MI355X — the video part of `AudioVideoSegments.__getitem__` + default collate
    (dataset.py:121-253) without its per-item CPU preprocessing (dataset.py:145-209: process_cv2_inputs + interpolate per
    segment in DataLoader workers) and without a host round trip per step:

      * the video (and the audio examples) stay resident in HBM: as uint8 frames for SlowFast; for every other encoder (the
        3D-ResNets) as the fp32 table [F, 3, hw, hw] the dataset keeps on the host — /255, antialiased resize, per-channel
        normalisation — built once by ops.frames_resize_aa_norm (F * 3 * hw^2 * 4 bytes: 361 MB per 600 frames at 224^2),
        after which the uint8 copy is dropped;
      * negatives are drawn by the device MT19937 kernel from NumPy's own stream (ops.train_batch_plan: the state of
        np.random is uploaded once by `seed_from_numpy()` and can be handed back by `sync_to_numpy()`), with the
        reference's hard-negative overwrite (dataset.py:183-190); the same launch writes the window starts;
      * query / positive / negative windows are packed by the gather kernels (ops.clip_pack_gather for SlowFast,
        ops.clip_gather_frames over the table otherwise), starts read on device.

    batch(idx) -> (q_frames, t_frames, q_audio_eg, t_audio_eg) with the shapes the DataLoader would deliver:
    SlowFast: q_frames [slow [B,3,8,hw,hw], fast [B,3,32,hw,hw]], t_frames [slow [B,1+negs,3,8,hw,hw], fast [B,1+negs,3,32,hw,hw]];
    otherwise: q_frames [B,W,3,hw,hw], t_frames [B,1+negs,W,3,hw,hw].
    loader(batch_size) is the form train() iterates.

    Several ranks (rank, world): every rank keeps the whole video resident and is handed the GLOBAL batch's item ids; sample(), _pack()
    and batch() return the rank's share only — item k of a global batch of world * per items belongs to rank k // per, the contiguous
    scatter of the reference's DataParallel (main.py:420).  The sampling kernel walks the stream over the whole global batch on every
    rank and materialises the rank's items, so that all ranks hold the same MT19937 state after every step, and a world-N run sees, item
    for item and bit for bit, the batches of a one-process run at N times the per-rank batch from the same np.random state
    (`seed_from_numpy()` broadcasts rank 0's)."""

    def __init__(self, dataset, device, dtype=torch.float32, rank=0, world=1):
        from . import ops

        if dataset.split != "train":
            raise ValueError("DeviceSegmentBatcher packs training items")
        if world < 1 or not 0 <= rank < world:
            raise ValueError("DeviceSegmentBatcher: rank %d is not one of %d" % (rank, world))
        self.rank, self.world = int(rank), int(world)
        self.slowfast = dataset.enc_arch == "slowfast"
        if not self.slowfast and dtype != torch.float32:
            raise ValueError("DeviceSegmentBatcher: the frame table of %s is float32, not %s" % (dataset.enc_arch, dtype))
        self.ops, self.ds, self.dev, self.dtype = ops, dataset, torch.device(device), dtype
        self.n_frames = int(dataset.video_u8.shape[0])
        # segment ids the sampler can produce are 0 .. len(ds) (positive = idx + 1, negatives from [0, len]); the gather kernels
        # read their starts on the device and CLAMP frame ids (a bad id cannot fault, but would silently repeat edge frames),
        # so the one check that every id is in range is made here, once
        need = len(dataset) * dataset.stride + dataset.window
        if need > self.n_frames:
            raise ValueError("DeviceSegmentBatcher: segment %d needs frames up to %d, the video has %d"
                             % (len(dataset), need, self.n_frames))
        self.frames = dataset.video_u8.to(self.dev).contiguous()
        self.table = None
        if not self.slowfast:
            self.table = ops.frames_resize_aa_norm(self.frames, dataset.img_size)
            self.frames = None  # (the table is all this branch reads)
        self.audio_eg = dataset.audio_eg.to(self.dev) if dataset.audio_eg.dim() == 4 else None
        self._audio_any = None  # loader(): the examples of any rank, the dummy [n, 10] of adata=None included
        self.state = None
        self._gauss = (0, 0.0)

    def seed_from_numpy(self):
        """Uploads np.random's state.  With several ranks under an initialised process group it is rank 0's state, its cached gaussian
        included, that every rank uploads (one broadcast of 2.5 KB — a collective: every rank calls this at the same point)."""
        st = np.random.get_state()
        words = np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)])
        gauss = (int(st[3]), float(st[4]))  # a cached gaussian of the host stream survives the round trip
        dist = torch.distributed
        if self.world > 1 and dist.is_available() and dist.is_initialized():
            host = dist.get_backend() == "gloo"  # (gloo moves host tensors, RCCL device tensors: as train_ops.GradExchange.bind)
            msg = np.concatenate([words.astype(np.int64), np.array([gauss[0]], np.int64), np.array([gauss[1]], np.float64).view(np.int64)])
            t = torch.from_numpy(msg).to("cpu" if host else self.dev)
            dist.broadcast(t, src=0)
            msg = t.cpu().numpy()
            words = msg[:625].astype(np.uint32)
            gauss = (int(msg[625]), float(msg[626:627].view(np.float64)[0]))
        self._gauss = gauss
        self.state = torch.from_numpy(words.view(np.int32).copy()).to(self.dev)
        return self

    def sync_to_numpy(self):
        """Hands the advanced stream back to np.random (one D2H of 2.5 KB; only needed when host code draws next)."""
        words = self.state.cpu().numpy().view(np.uint32)
        np.random.set_state(("MT19937", words[:624].copy(), int(words[624]), self._gauss[0], self._gauss[1]))

    def state_dict(self):
        """What the next batch's negatives depend on: the 625 words of the device MT19937 stream (None before the first upload: the
        stream then starts from np.random's state) and the host stream's cached gaussian (one D2H of 2.5 KB)."""
        return {"state": None if self.state is None else self.state.cpu().clone(), "gauss": (int(self._gauss[0]), float(self._gauss[1]))}

    def load_state_dict(self, sd):
        words = sd["state"]
        if words is not None:
            words = torch.as_tensor(words)
            if words.dtype != torch.int32 or words.numel() != 625:
                raise ValueError("DeviceSegmentBatcher.load_state_dict: the stream is 625 int32 words, got %s x %d" % (words.dtype, words.numel()))
            words = words.reshape(625).to(self.dev)
        self.state = words
        self._gauss = (int(sd["gauss"][0]), float(sd["gauss"][1]))

    def share(self, idx):
        """The rank's items of a global batch: ids [world * per] -> ids [rank * per : (rank + 1) * per] (DataParallel's contiguous
        scatter)."""
        b = int(idx.numel())
        if b % self.world:
            raise ValueError("DeviceSegmentBatcher: a global batch of %d items does not divide over %d ranks" % (b, self.world))
        per = b // self.world
        return idx[self.rank * per : (self.rank + 1) * per]

    def _plan(self, idx):
        """idx int64 [B] (device, the GLOBAL batch) -> (the rank's ids [b], target segment ids int32 [b, 1 + negs], window starts
        int32 [b (2 + negs)]): one launch; the stream is advanced past all B items."""
        if self.state is None:
            self.seed_from_numpy()
        mine = self.share(idx)
        tgt, starts = self.ops.train_batch_plan(self.state, idx, self.rank * mine.numel(), mine.numel(), len(self.ds), self.ds.n_negs,
                                                self.ds.stride)
        return mine, tgt, starts

    def sample(self, idx):
        """idx int64 [B] (the global batch) -> (positive ids [b], negative ids [b, n_negs]) of the rank's b = B / world items, on the
        device."""
        idx = torch.as_tensor(idx, dtype=torch.int64).to(self.dev).contiguous()
        mine, tgt, _ = self._plan(idx)
        return mine + 1, tgt[:, 1:]

    def _pack(self, idx):
        """idx int64 [B] (device, the global batch) -> (q_frames, t_frames, target segment ids [b, 1 + negs]) of the rank's b items."""
        ds, W = self.ds, self.ds.window
        mine, tgt, starts = self._plan(idx)
        b = mine.numel()
        tgt = tgt.to(torch.int64)  # (index tensors of the audio examples)
        hw, n = ds.img_size, tgt.shape[1]
        if not self.slowfast:
            clips = self.ops.clip_gather_frames(self.table, starts, W)  # [b + b n, W, 3, hw, hw]
            return clips[:b], clips[b:].view(b, n, W, 3, hw, hw), tgt
        slow, fast = self.ops.clip_pack_gather(self.frames, starts, W, out_hw=hw, dtype=self.dtype)
        q_frames = [slow[:b], fast[:b]]
        t_frames = [slow[b:].view(b, n, 3, 8, hw, hw), fast[b:].view(b, n, 3, 32, hw, hw)]
        return q_frames, t_frames, tgt

    def batch(self, idx):
        idx = torch.as_tensor(idx, dtype=torch.int64).to(self.dev).contiguous()
        q_frames, t_frames, tgt = self._pack(idx)
        q_ae = t_ae = None
        if self.audio_eg is not None:
            q_ae = self.audio_eg[self.share(idx)]
            t_ae = self.audio_eg[tgt.reshape(-1)].view(tgt.shape[0], tgt.shape[1], *self.audio_eg.shape[1:])
        return q_frames, t_frames, q_ae, t_ae

    def loader(self, batch_size, shuffle=True, drop_last=True, seed=None):
        """The DataLoader's place in train(): a re-iterable with __len__ whose epochs yield
        (q_frames, None, q_audio_eg, t_frames, None, t_audio_eg) — train() never touches the waveform fields.

        batch_size is PER RANK: every step draws one global batch of batch_size * world ids and the rank assembles its share.  With
        several ranks, or with a seed, the order of epoch e is torch.randperm(n, generator=Generator().manual_seed(seed + e)) — the same on
        every rank (a seed not given is drawn on rank 0 and broadcast), chosen by set_epoch(e) as with DistributedSampler; the loader is
        its own `.sampler`.  One process without a seed keeps torch.randperm(n) from the global generator.  Several ranks need
        drop_last: every rank must meet every batch shape at the same iteration.  The tail of an epoch that does not fill a global batch
        is DROPPED — not padded with repeated items as DistributedSampler pads its shards — so an epoch is n // (batch_size * world)
        steps and shows every item at most once."""
        return _DeviceLoader(self, int(batch_size), shuffle, drop_last, seed)


class _DeviceLoader:
    def __init__(self, batcher, batch_size, shuffle, drop_last, seed=None):
        if batch_size < 1:
            raise ValueError("DeviceSegmentBatcher.loader: batch_size must be positive")
        self.bat, self.batch_size, self.shuffle, self.drop_last = batcher, batch_size, shuffle, drop_last
        world = batcher.world
        self.global_batch = batch_size * world
        if world > 1 and not drop_last:
            raise ValueError("DeviceSegmentBatcher.loader: several ranks need drop_last=True (a short last batch would not divide over "
                             "the ranks, and every rank must meet every batch shape at the same iteration)")
        if drop_last and len(batcher.ds) < self.global_batch:
            raise ValueError("DeviceSegmentBatcher.loader: %d items do not fill one global batch of %d (%d per rank x %d ranks)"
                             % (len(batcher.ds), self.global_batch, batch_size, world))
        self.epoch, self.seed = 0, seed
        if shuffle and world > 1 and seed is None:
            dist = torch.distributed
            if not (dist.is_available() and dist.is_initialized()):
                raise ValueError("DeviceSegmentBatcher.loader: several ranks without a process group need a seed (one order for all)")
            t = torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64)  # (rank 0's draw counts; gloo and RCCL each move their own kind)
            t = t if dist.get_backend() == "gloo" else t.to(batcher.dev)
            dist.broadcast(t, src=0)
            self.seed = int(t.cpu()[0])

    @property
    def sampler(self):
        return self  # (main()'s train_loader.sampler.set_epoch(epoch))

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def state_dict(self):
        """The loader's seed and epoch (what order() draws from, next to torch's global generator when there is no seed) and the
        batcher's stream: with the host generators' states, everything the next epoch's batches depend on."""
        return {"seed": self.seed, "epoch": self.epoch, "batcher": self.bat.state_dict()}

    def load_state_dict(self, sd):
        self.seed = None if sd["seed"] is None else int(sd["seed"])
        self.epoch = int(sd["epoch"])
        self.bat.load_state_dict(sd["batcher"])

    def __len__(self):
        n = len(self.bat.ds)
        return n // self.global_batch if self.drop_last else -(-n // self.global_batch)

    def order(self):
        """The item ids of the current epoch, in the order the global batches are cut from."""
        n = len(self.bat.ds)
        if not self.shuffle:
            return torch.arange(n)
        if self.seed is None:
            return torch.randperm(n)  # (host order; not RandomSampler's stream)
        return torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + self.epoch))

    def __iter__(self):
        bat = self.bat
        if bat._audio_any is None:
            bat._audio_any = bat.audio_eg if bat.audio_eg is not None else bat.ds.audio_eg.to(bat.dev)
        audio = bat._audio_any
        order = self.order()
        for i in range(len(self)):
            idx = order[i * self.global_batch : (i + 1) * self.global_batch].to(bat.dev)
            q_frames, t_frames, tgt = bat._pack(idx)
            mine = bat.share(idx)
            # audio examples as the dataset indexes them (audio_eg[idx]; audio_eg[idx + 1] then audio_eg[neg]), whatever their rank
            t_ae = audio[tgt.reshape(-1)].view(mine.numel(), tgt.shape[1], *audio.shape[1:])
            yield q_frames, None, audio[mine], t_frames, None, t_ae
