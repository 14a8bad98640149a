"""What an epoch-end checkpoint costs the training loop, and the one-launch state copy behind --ckpt_async.

Part 1 — critical path.  For each model (the module main.main() builds, at 224^2, in the training layout) and each folder, the default
path — main.save_checkpoint on the device state_dict, synchronous — and the --ckpt_async path — main.save_checkpoint_async:
train_ops.StateSnapshot.take() plus the hand-off to checkpoint.AsyncCheckpointWriter — are interleaved in one process, `--rounds` times
each after a warm-up round, with is_best off and on.  Reported per leg: the median host time until the training loop may continue
and until the files are complete, the ratio of the two paths, and both as multiples of the one-item (46 ms) and eight-item (289 ms)
step times README.md records.  The async path's time until the files are complete is also the shortest epoch it can keep up with: with
shorter epochs the writer falls behind, both pinned buffers stay owned, and the third take() waits for the writer.

Part 2 — the kernel.  Pack and unpack (csrc/state_copy.hip, one launch each) over config 5's training state — parameters, buffers and
momentum buffers of the m = 1 SlowFast model — between device events, against train._snapshot's per-tensor clones of the same tensors:
achieved bytes per second (nbytes read + nbytes written) and the launch counts.

    python tools/probe_checkpoint.py [--rounds 7] [--models resnet18:1,slowfast:1,slowfast:2] [--dirs /tmp,/dev/shm] [--out LOG]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEP_MS = {"one item per rank": 46.0, "eight items": 289.0}  # README.md, config 5
COPY_PEAK = 6.29e12  # bytes/s read + written by a float4 copy kernel on this part (the microarchitecture notes' measured figure)


def build_model(arch, model_type, dev):
    from avtex import train_ops
    from avtex.models import ContrastivePredictionTemporal, ModelBuilder3D
    from avtex.vggish import VGGish

    builder = ModelBuilder3D()
    q, fc_dim = builder.build_network(arch=arch, img_size=224, window=20)
    t, fc_dim = builder.build_network(arch=arch, img_size=224, window=20)
    model = ContrastivePredictionTemporal(q, t, VGGish(), model_type, fc_dim, 0.1, 20, 4, 0.0, mini_batchsize=150, enc_arch=arch, img_size=224)
    model = model.to(dev)
    try:
        return train_ops.training_layout(model)
    except RuntimeError as e:
        # (m = 2: Module.to(memory_format=channels_last_3d) refuses VGGish's 4-D weights in this torch; the sizes, dtypes and strides a
        #  checkpoint sees are what matters here, so the tensors are laid out one by one)
        print("training_layout: %s — laying the tensors out one by one" % e)
        with torch.no_grad():
            for p in model.parameters():
                fmt = {5: torch.channels_last_3d, 4: torch.channels_last}.get(p.dim())
                if fmt is not None:
                    p.data = p.data.contiguous(memory_format=fmt)
        return model


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--models", default="resnet18:1,slowfast:1,slowfast:2")
    ap.add_argument("--dirs", default="%s,/dev/shm" % tempfile.gettempdir(), help="folders to write to (a local disk, a RAM disk)")
    ap.add_argument("--kernel_rounds", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the log to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_checkpoint: needs the MI355X (no timing without a device)")
    import avtex
    from avtex import train_ops
    from avtex.checkpoint import AsyncCheckpointWriter
    from avtex.main import save_checkpoint, save_checkpoint_async
    from avtex.train import _snapshot

    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("device: %s; torch %s; %d rounds per leg after one warm-up round" % (avtex.ops.device_check(), torch.__version__, a.rounds))
    try:
        with open("/proc/mounts") as f:
            mounts = [ln.split()[1:3] for ln in f]
        for folder in a.dirs.split(","):
            real = os.path.realpath(folder)
            best = max((m for m in mounts if real == m[0] or real.startswith(m[0].rstrip("/") + "/")), key=lambda m: len(m[0]))
            say("folder %s: file system %s (mounted at %s)" % (folder, best[1], best[0]))
    except (OSError, ValueError):
        pass
    torch.manual_seed(0)
    kernel_model = None
    for spec in a.models.split(","):
        arch, m = spec.split(":")
        model = build_model(arch, int(m), dev)
        sd = model.state_dict()
        nbytes = sum(v.numel() * v.element_size() for v in sd.values())
        say("")
        say("== %s, m = %s: %d tensors, %.1f MB in the state_dict" % (arch, m, len(sd), nbytes / 1e6))
        for folder in a.dirs.split(","):
            work = tempfile.mkdtemp(prefix="avt_probe_ckpt_", dir=folder)
            try:
                for is_best in (False, True):
                    writer, snap = AsyncCheckpointWriter(), None
                    cont_s, cont_a, done_a = [], [], []
                    for r in range(a.rounds + 1):
                        head = {"epoch": r + 1, "arch": arch, "best_loss": 1.0 / (r + 1)}
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        save_checkpoint(dict(head, state_dict=model.state_dict()), is_best, os.path.join(work, "sync"))
                        t1 = time.perf_counter()
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        snap = save_checkpoint_async(writer, snap, head, model.state_dict(), None, is_best, os.path.join(work, "async"))
                        t3 = time.perf_counter()
                        writer.drain()
                        t4 = time.perf_counter()
                        if r:  # (round 0: code objects, the snapshot's buffers and tables, the page cache)
                            cont_s.append((t1 - t0) * 1e3)
                            cont_a.append((t3 - t2) * 1e3)
                            done_a.append((t4 - t2) * 1e3)
                    writer.close()
                    ms, ma, md = statistics.median(cont_s), statistics.median(cont_a), statistics.median(done_a)
                    say("%-10s is_best %d  synchronous: continue = complete %9.1f ms (min %.1f max %.1f) | async: continue %7.2f ms (min %.2f max "
                        "%.2f), complete %9.1f ms (min %.1f max %.1f) | continue: sync / async = %.0fx"
                        % (folder, is_best, ms, min(cont_s), max(cont_s), ma, min(cont_a), max(cont_a), md, min(done_a), max(done_a), ms / ma))
                    for what, step in STEP_MS.items():
                        say("             in steps of %5.0f ms (%s): synchronous %.2f, async continue %.4f, async complete %.2f — the async "
                            "writer keeps up with epochs of %d steps or more" % (step, what, ms / step, ma / step, md / step, int(md / step) + 1))
                    flush_out()
            finally:
                shutil.rmtree(work, ignore_errors=True)
        if arch == "slowfast" and int(m) == 1:
            kernel_model = model
        else:
            del model, sd
            torch.cuda.empty_cache()

    if kernel_model is not None:
        say("")
        say("== the kernel: config 5's training state (slowfast, m = 1, ArenaSGD with momentum)")
        model = kernel_model
        opt = train_ops.ArenaSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        saved = _snapshot(model, opt)  # the tensors the graph warm-up clones: parameters, buffers, momentum buffers
        tensors = [t.detach() for t, _ in saved]
        del saved
        snap = train_ops.StateSnapshot([("t%d" % i, t) for i, t in enumerate(tensors)])
        total = sum(snap.nbytes)
        jobs = sum(1 for n in snap.nbytes if n)
        say("%d tensors (%d jobs, %d blocks of 16 KiB), %.1f MB" % (len(tensors), jobs, snap._pack_tab[2], total / 1e6))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            e0.record()
            out = fn()
            e1.record()
            h1 = time.perf_counter()
            e1.synchronize()
            del out
            return e0.elapsed_time(e1), (h1 - h0) * 1e3

        legs = {"pack (one launch)": lambda: snap._launch(snap._pack_tab), "unpack (one launch)": lambda: snap._launch(snap._unpack_tab),
                "train._snapshot (one clone per tensor)": lambda: _snapshot(model, opt)}
        times = {k: [] for k in legs}
        for r in range(a.kernel_rounds + 2):
            for k, fn in legs.items():
                dt = timed(fn)
                if r >= 2:
                    times[k].append(dt)
        for k, v in times.items():
            dev_ms, host_ms = statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)
            rate = 2 * total / (dev_ms * 1e-3)
            say("%-40s device %.3f ms (min %.3f max %.3f), host issue %.3f ms: %.2f TB/s read + written = %.0f %% of the %.2f TB/s a float4 "
                "copy reaches; launches: %d" % (k, dev_ms, min(x[0] for x in v), max(x[0] for x in v), host_ms, rate / 1e12,
                                                 100 * rate / COPY_PEAK, COPY_PEAK / 1e12, 1 if "one launch" in k else len(tensors)))
    flush_out()


if __name__ == "__main__":
    main()
