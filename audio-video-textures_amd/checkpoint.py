"""Kinetics-400 SlowFast checkpoint ingestion: the caffe2 pickle the reference starts config 5 from.

The reference builds its encoders through PySlowFast's `ActionPredictor` with `cfg.TEST.CHECKPOINT_TYPE = "caffe2"` and
`CHECKPOINT_FILE_PATH = .../pretrained/SLOWFAST_8x8_R50.pkl` (contrastive_video_textures/models/models.py:565-580): the
model-zoo file is a pickle `{"blobs": {caffe2 blob name: ndarray}}` (latin1), and PySlowFast renames the blobs to its module
names while loading.  `slowfast.SlowFast` here uses those module names, so this file only has to restate the renaming
(third-party behaviour, not vendored by the reference: PARITY UNPINNED like the architecture itself — no real .pkl exists in
this environment; tests/test_host_logic.py covers every parameter and buffer of `SlowFast` with a synthetic blob dict).

Blob grammar of SLOWFAST_8x8_R50 (no non-local blocks):
    [t_]conv1_w                                   stem convolution          (t_ = fast pathway)
    [t_]res_conv1_bn_{s,b,rm,riv}                 stem BatchNorm: scale, bias, running mean, running (inverse-)variance slot
    [t_]res<S>_<I>_branch1_w / _branch1_bn_*      stage S (2..5) block I shortcut
    [t_]res<S>_<I>_branch2{a,b,c}_w / _bn_*       bottleneck convolutions
    t_pool1_subsample_w / _bn_*                   lateral fusion after the stem          -> s1_fuse
    t_res<S>_<I>_branch2c_bn_subsample_w / _bn_*  lateral fusion after stage S (2..4)    -> s<S>_fuse
    pred_w, pred_b                                classifier (the reference replaces the head's projection by Identity: dropped)
    *_momentum, lr, model_iter, ...               solver state: dropped

Also here: `AsyncCheckpointWriter`, the background thread that writes the TRAINING checkpoints of main.py --ckpt_async.
"""
import os
import pickle
import queue
import re
import shutil
import threading

import numpy as np
import torch

_BN_FIELD = {"s": "weight", "b": "bias", "rm": "running_mean", "riv": "running_var"}
_BLOCK = re.compile(r"^(t_)?res([2-5])_(\d+)_branch(1|2[abc])_(w|bn_(?:s|b|rm|riv))$")
_STEM = re.compile(r"^(t_)?(?:conv1_(w)|res_conv1_bn_(s|b|rm|riv))$")
_FUSE = re.compile(r"^t_(?:pool1|res([2-4])_\d+_branch2c_bn)_subsample_(w|bn_(?:s|b|rm|riv))$")


def caffe2_blob_to_module_name(blob):
    """One caffe2 blob name -> this package's `SlowFast` state-dict key, or None for blobs that have no place in it
    (classifier, solver state)."""
    m = _FUSE.match(blob)  # (before the block pattern: the fusion blobs of stages 2-4 carry a block prefix)
    if m:
        stage, what = m.group(1) or "1", m.group(2)
        return "s%s_fuse.%s" % (stage, "conv_f2s.weight" if what == "w" else "bn." + _BN_FIELD[what[3:]])
    m = _STEM.match(blob)
    if m:
        stem = "s1.pathway%d_stem." % (1 if m.group(1) else 0)
        return stem + ("conv.weight" if m.group(2) else "bn." + _BN_FIELD[m.group(3)])
    m = _BLOCK.match(blob)
    if m:
        fast, stage, idx, branch, what = m.groups()
        base = "s%s.pathway%d_res%s." % (stage, 1 if fast else 0, idx)
        if branch == "1":
            return base + ("branch1.weight" if what == "w" else "branch1_bn." + _BN_FIELD[what[3:]])
        conv = branch[1]
        return base + "branch2." + (conv + ".weight" if what == "w" else conv + "_bn." + _BN_FIELD[what[3:]])
    return None


def convert_caffe2_slowfast(blobs):
    """{caffe2 blob: ndarray} -> (state dict for slowfast.SlowFast, sorted list of the blobs that were dropped)."""
    sd, dropped = {}, []
    for blob, value in blobs.items():
        key = caffe2_blob_to_module_name(blob)
        if key is None:
            dropped.append(blob)
            continue
        if key in sd:
            raise ValueError("caffe2 checkpoint: blobs collide on %s" % key)
        sd[key] = torch.from_numpy(np.ascontiguousarray(np.asarray(value, dtype=np.float32)))
    return sd, sorted(dropped)


def load_caffe2_pkl(path):
    with open(path, "rb") as f:
        data = pickle.load(f, encoding="latin1")
    return data["blobs"] if isinstance(data, dict) and "blobs" in data else data


def load_kinetics_slowfast(model, path, strict=True):
    """Loads SLOWFAST_8x8_R50.pkl (caffe2) — or a torch state dict (.pth / .pyth, optionally under "state_dict" /
    "model_state") — into a `slowfast.SlowFast`.  strict: every parameter and running statistic of the model must be present
    with the right shape (num_batches_tracked, which caffe2 does not have, excepted).  -> list of dropped blob / key names."""
    if str(path).endswith(".pkl"):
        sd, dropped = convert_caffe2_slowfast(load_caffe2_pkl(path))
    else:
        sd = torch.load(path, map_location="cpu")
        for k in ("state_dict", "model_state"):
            if isinstance(sd, dict) and k in sd:
                sd = sd[k]
        dropped = [k for k in sd if k.startswith("head.projection")]
        sd = {k: v for k, v in sd.items() if not k.startswith("head.projection")}
    own = model.state_dict()
    want = [k for k in own if not k.endswith("num_batches_tracked")]
    missing = [k for k in want if k not in sd]
    extra = [k for k in sd if k not in own]
    bad = [k for k in sd if k in own and tuple(sd[k].shape) != tuple(own[k].shape)]
    if bad:
        raise ValueError("checkpoint %s: shape mismatch on %s" % (path, ", ".join(
            "%s %s vs %s" % (k, tuple(sd[k].shape), tuple(own[k].shape)) for k in bad[:5])))
    if strict and (missing or extra):
        raise ValueError("checkpoint %s: %d missing (%s ...), %d unexpected (%s ...)" % (
            path, len(missing), ", ".join(missing[:3]), len(extra), ", ".join(extra[:3])))
    model.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=False)
    return dropped


# ------------------------------------------------------------------------------------------------------------------------
# Writing the training checkpoints off the training loop (main.py --ckpt_async).
def write_atomically(state, path):
    """torch.save(state) into a temporary file beside `path`, then os.replace: a reader of `path` sees the old file or the new one,
    never a part of either."""
    tmp = "%s.tmp.%d" % (path, os.getpid())
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


class AsyncCheckpointWriter:
    """One background thread that turns snapshots into main.save_checkpoint's files:

        w = AsyncCheckpointWriter()
        w.submit(source, make_state, is_best, filename)   # returns at once
        w.close()                                         # every file complete, or the thread's exception raised

    source: an object with wait() -> {name: CPU tensor} (train_ops.SnapshotHandle: views into one pinned buffer; its release(), if it
    has one, is called once the tensors are cloned) or such a dict itself.  The thread CLONES every tensor — torch.save of a view
    serialises the whole buffer behind it — and calls make_state(clones) -> the checkpoint dict, which it writes to
    filename + "_latest.pth.tar" through a temporary file and os.replace, then copies to "_best.pth.tar" the same way when is_best: the
    files, keys and tensors of the synchronous path.  Jobs are written in the order submitted.  An exception in the thread is raised
    again by the next submit() or by close(); jobs after a failed one are dropped (their sources released)."""

    def __init__(self):
        self._queue, self._error, self._closed = queue.Queue(), None, False
        self._thread = threading.Thread(target=self._run, name="avt-checkpoint-writer", daemon=True)
        self._thread.start()

    def _raise_pending(self):
        if self._error is not None:
            err, self._error = self._error, None
            raise err

    def submit(self, source, make_state, is_best, filename):
        if self._closed:
            raise RuntimeError("AsyncCheckpointWriter.submit() after close()")
        self._raise_pending()
        self._queue.put((source, make_state, bool(is_best), filename))

    def pending(self):
        """Jobs submitted and not yet written (or dropped)."""
        return self._queue.unfinished_tasks

    def drain(self):
        """Waits until every job submitted so far is written (or has failed: the next submit() or close() tells); the writer stays open."""
        self._queue.join()

    def close(self):
        """Waits for every submitted job; raises what the thread raised.  Safe to call twice."""
        if not self._closed:
            self._closed = True
            self._queue.put(None)
            self._thread.join()
        self._raise_pending()

    def _run(self):
        while True:
            job = self._queue.get()
            try:
                if job is None:
                    return
                source, make_state, is_best, filename = job
                release = getattr(source, "release", None)
                try:
                    if self._error is not None:
                        continue  # (a write has failed: nothing after it is written; close() reports)
                    tensors = source.wait() if hasattr(source, "wait") else source
                    owned = {k: v.clone() for k, v in tensors.items()}
                finally:
                    if release is not None:
                        release()
                latest = filename + "_latest.pth.tar"
                write_atomically(make_state(owned), latest)
                if is_best:
                    best, tmp = filename + "_best.pth.tar", "%s_best.pth.tar.tmp.%d" % (filename, os.getpid())
                    try:
                        shutil.copyfile(latest, tmp)
                        os.replace(tmp, best)
                    finally:
                        if os.path.exists(tmp):
                            os.remove(tmp)
            except BaseException as e:  # noqa: BLE001 (kept for the training thread, which raises it)
                if self._error is None:
                    self._error = e
            finally:
                self._queue.task_done()
