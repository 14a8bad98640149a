"""CLI / per-video driver, drop-in for contrastive_video_textures/main.py:41-548: every flag of the
reference parser with the same names, defaults and types; `main(args, video_name, itr=0)`; the per-video
loop with the fps -> window/stride override (main.py:511-516) and default checkpoint name (:520-534).

Additions (all optional): --stitch_mode {compat,aligned}, --ref_num_gpus, --enc_dtype {fp32,bf16},
--enc_batch, --train_input {loader,device}, --vcam (the flag validate.py:299 reads but the reference never defines [quirk Q2]),
--ckpt_async (the epoch-end save off the loop: train_ops.StateSnapshot + checkpoint.AsyncCheckpointWriter) and --ckpt_train_state
(optimizer, scheduler, generators and loader in the checkpoint; --resume then repeats the uninterrupted run),
--audio_resample {scipy,kaiser_best} and --audio_load_sr (the reference's resampy filter and librosa.load's rate, both off by default).
Multi-GPU: one process per GPU under torch.distributed.run instead of torch.nn.DataParallel (main.py:420).  --train_input device works
there too, with or without --train_graph 1: every rank assembles its share of each global batch in its own HBM
(dataset.DeviceSegmentBatcher(rank, world)), item for item the batch DataParallel would scatter from one NumPy stream.
--train_deterministic there also sums the gradients in rank order (train_ops.GradExchange, ordered: one all-gather, one HIP launch),
with or without --train_graph 1, so that a seed repeats across ranks for one world size.
"""
import argparse
import math
import os
import shutil

import torch

from . import dist as avt_dist
from .dataset import AudioVideoSegments
from .logger import Logger
from .models import ContrastivePredictionTemporal, ModelBuilder3D
from .train import train
from .validate import read_video, validate
from .vggish import VGGish


def build_parser():
    parser = argparse.ArgumentParser(description="PyTorch Video Textures (MI355X-native hot path)")
    a = parser.add_argument
    a("--enc_arch", "-ea", metavar="ARCH", default="resnet18", help="model architecture")
    a("--model_type", "-m", default=1, type=int, help="(1) Video Textures (2) Audio Video Textures")
    a("--vdata", "-vdata", default=None, type=str, help="Path to video dataset")
    a("--adata", "-adata", default=None, type=str, help="Path to audio")
    a("--pdata", "-pdata", default=None, type=str, help="Path to poses")
    a("--fdata", "-fdata", default=None, type=str, help="Path to flow")
    a("--dadata", "-dadata", default="audio/target", type=str, help="Path to driving audio dataset")
    a("--video_list", "-vl", default=None, type=str, nargs="+", help="list of input videos")
    a("--fps", "-fps", default=30, type=int, help="frame rate of input video")
    a("--subsample_rate", "-subsample", default=1, type=int, help="rate for subsampling the video")
    a("--temp", "-temp", default=0.1, type=float, help="Temperature value")
    a("--threshold", "-th", default=0.0, type=float, help="Threshold value")
    a("--l2", "-l2", default=True, action="store_false", help="To use l2 norm or not")
    a("--interpolation", "-nintp", default=True, action="store_false", help="Interpolate frames at eval")
    a("--img_size", "-size", default=224, type=int, help="resize image to this size")
    a("--n_negs", "-negs", default=20, type=int, help="Number negative frames to use when training")
    a("--window", "-w", default=20, type=int, help="Size of temporal window")
    a("--train_stride", "-train_stride", default=4, type=int, help="Stride length")
    a("--stride", "-stride", default=4, type=int, help="Stride length")
    a("--new_video_length", "-nvl", default=30, type=int, help="Length of new video")
    a("--alpha", "-alpha", default=0.5, type=float, help="alpha for validation to control driving audio")
    a("--SF", "-SF", default=5, type=int, help="slomo factor N")
    a("--train_layout", default="ndhwc", choices=["ndhwc", "ncdhw"],
      help="memory layout of the encoders in training: ndhwc = channels_last_3d (the hand-written training passes of train_ops, for the "
           "SlowFast and the 3D-ResNet encoders), ncdhw = torch default (MIOpen autograd)")
    a("--bn_replicas", default=1, type=int,
      help="train(): normalise the rank's batch as this many equal groups of items, each with its own BatchNorm statistics — "
           "what the reference's DataParallel gives every GPU's share of the batch (main.py:420), running statistics from "
           "the first group only as DataParallel keeps replica 0's buffers; 1 = over the rank's whole batch; -1 = one group "
           "per item (batch 8 on 8 GPUs in the reference)")
    a("--train_graph", default=0, type=int, choices=[0, 1],
      help="1: train() captures the device side of a step once per batch shape as a HIP graph and replays it (train_ops.GraphedStep) — "
           "for small batches whose launches the host issues slower than the device runs them.  One process: forward, loss, backward and "
           "optimizer are the graph; with torch's SGD the first batch of a shape also serves the two warm-up steps (not in the "
           "reference).  Under torch.distributed.run every rank replays forward, loss, backward and one launch that packs the gradients "
           "into a flat buffer (train_ops.GradExchange); one all-reduce and the optimizer follow each replay eagerly, the model is not "
           "wrapped in DistributedDataParallel, and every batch takes one step with either optimizer")
    a("--train_optimizer", default="torch", choices=["torch", "hip"],
      help="torch: torch.optim.SGD (the reference's, main.py:440); hip: train_ops.ArenaSGD — the same update as one HIP launch over all "
           "parameters with --lr / --momentum / --weight_decay read from device memory: with --train_graph 1 in one process the replayed "
           "step then follows the StepLR schedule (torch's SGD keeps the rate it was captured with) and the first batch of a shape takes "
           "one step; across ranks the optimizer runs outside the graph and both choices follow the schedule")
    a("--dist_backend", default=None, choices=["nccl", "gloo"],
      help="torch.distributed backend under torch.distributed.run: nccl = RCCL, one rank per GPU; gloo = ranks that may share a GPU (RCCL "
           "refuses two ranks on one device); default: nccl where a GPU is visible, gloo otherwise")
    a("--train_input", default="loader", choices=["loader", "device"],
      help="where train() gets its batches: loader = torch DataLoader over AudioVideoSegments (host preprocessing, the reference's "
           "path); device = dataset.DeviceSegmentBatcher: the video resident in HBM (SlowFast: uint8 frames; other encoders: the "
           "resized and normalised fp32 frame table), negatives drawn and windows gathered by HIP kernels, no per-step host copy.  "
           "Under torch.distributed.run every rank keeps the video and assembles its batch_size / world items of each global batch: "
           "the ranks share rank 0's NumPy stream and one epoch order, so their batches are those of one process at the global batch; "
           "the tail of an epoch that does not fill a global batch is dropped")
    a("--train_conv", default="x3", choices=["x3", "fp32"],
      help="arithmetic of the training convolutions (with --train_layout ndhwc): x3 = split-plane MFMA kernels, fp32 "
           "accumulation, forward 2^-22 / gradients 2^-16 per product (default; train_ops.py); fp32 = MIOpen's fp32 "
           "convolutions, the reference's arithmetic (train.py:114-141), with the fused BatchNorm / pool passes kept; both for SlowFast "
           "and for the 3D-ResNets")
    a("--train_deterministic", default=False, action="store_true",
      help="weight gradients of the training step as per-chunk partial tiles summed in a fixed order (train_ops.set_deterministic) "
           "instead of fp32 atomics: with the rest of the step already free of atomics, one process on one GPU with one build repeats "
           "a seed bit for bit, eagerly and with --train_graph 1, with either --train_optimizer.  Needs --train_layout ndhwc and "
           "--train_conv x3.  Under torch.distributed.run the gradients are also summed in rank order: the model is prepared by "
           "train_ops.prepare_ranks (no DistributedDataParallel, with or without --train_graph 1), the ranks all-gather their packed "
           "gradients and one HIP launch adds them in ascending rank order (train_ops.GradExchange, ordered), so a seed repeats bit "
           "for bit for the same world size, the same build and the same GPU type; the gathered rows cost world x 4 bytes per "
           "trained parameter of HBM per rank.  Default off: the atomic path and the backend's all-reduce, unchanged (not in the "
           "reference)")
    a("--ckpt_async", default=False, action="store_true",
      help="write the epoch-end checkpoints off the training loop: the state leaves the device in one launch and one copy into pinned "
           "memory (train_ops.StateSnapshot), a background thread writes *_latest.pth.tar and *_best.pth.tar through temporary files "
           "and os.replace (checkpoint.AsyncCheckpointWriter); the same files and keys as the default; every file is complete when "
           "main() returns.  Default off: torch.save on rank 0 inside the loop, as in the reference")
    a("--ckpt_train_state", default=False, action="store_true",
      help="checkpoints also carry `train_state` (one more key, which other loaders ignore): the optimizer's and the scheduler's state, "
           "the torch CPU / device and np.random generator states, the device loader's stream, seed and epoch, the world size and the "
           "--train_deterministic setting; with --resume all of it is restored (a checkpoint without the key is refused), and with "
           "--train_deterministic --train_input device (or -j 0) in one process on one GPU a run interrupted after any epoch and resumed "
           "equals the uninterrupted one bit for bit; across ranks, with --train_deterministic --train_input device and the same world "
           "size, it equals it in rank 0's checkpoint and in every rank's losses (the train_state is rank 0's; the BatchNorm running "
           "statistics of the other ranks are not saved and come back as rank 0's).  Default off: --resume restores the weights, the "
           "epoch and best_loss")
    a("--slomo_ckpt", default="ckpt/SuperSloMo.ckpt", type=str,
      help="SuperSloMo checkpoint (validate.py:183 hard-codes this path); 'random' = seeded weights; missing file = cuts")
    a("-long", "--long", dest="long", default=False, action="store_true", help="unused in the reference")
    a("-fb", "--frames_bar", dest="frames_bar", default=False, action="store_true", help="Visualize transitions.")
    a("--epochs", default=60, type=int, metavar="N", help="number of total epochs to run")
    a("--size", default=224, type=int, metavar="N", help="primary image input size")
    a("--start_epoch", default=None, type=int, metavar="N", help="manual epoch number (useful on restarts)")
    a("--batch_size", "-bs", default=32, type=int, metavar="N", help="mini-batch size (default: 32)")
    a("--mini_batchsize", "-mbs", default=150, type=int, help="mini-batch size for target frames")
    a("--lr", "-lr", default=10e-3, type=float, metavar="LR", help="initial learning rate")
    a("--lr_steps", default=30, type=int, metavar="LRSteps", help="epochs to decay learning rate by 10")
    a("--momentum", default=0.9, type=float, metavar="M", help="momentum")
    a("--weight_decay", "--wd", default=0.0001, type=float, metavar="W", help="weight decay (default: 1e-4)")
    a("--workers", "-j", default=4, type=int, metavar="N", help="number of data loading workers")
    a("--print_freq", "-p", default=5, type=int, metavar="N", help="print frequency")
    a("--log_freq", "-lf", default=10, type=int, metavar="N", help="frequency to write in tensorboard")
    a("--resume", default="", type=str, metavar="PATH", help="path to latest checkpoint (default: none)")
    a("-e", "--evaluate", dest="evaluate", action="store_true", help="evaluate model on validation set")
    a("-da", "--driving_audio", default=None, type=str, nargs="+", help="list of target audios")
    a("-daf", "--da_feats", default="VGG", type=str, help="type of feats for audio conditioning")
    a("-daf_resume", "--daf_resume", default="", type=str, nargs="+", help="List of paths to best VideoForAudio ckpt")
    a("-ve", "--visualize_evaluate", dest="visualize_evaluate", action="store_true",
      help="evaluate model on validation set and visualize logits")
    a("-vf", "--val_freq", default=5, type=int, metavar="VF", help="frequency to call validate during train)")
    a("--logdir", default="./logs", help="folder to output tensorboard logs")
    a("--logname", default="exp", help="name of the experiment for checkpoints and logs")
    a("-rf", "--results_folder", default="results", type=str, help="folder for result videos")
    a("--ckpt", default="./ckpt", help="folder to output checkpoints")
    # --- additions of the MI355X build ---
    a("--stitch_mode", default="compat", choices=["compat", "aligned"],
      help="compat: the shipped reference's window/label map; aligned: the N x N matrix the labels claim")
    a("--ref_num_gpus", default=None, type=int, help="reference GPU count to emulate in compat mode")
    a("--enc_dtype", default="fp32", choices=["fp32", "bf16", "bf16x3", "f16x3"],
      help="encoder arithmetic at -e: fp32 (default; on the MFMA kernels = the contract-grade split-plane mode f16x3), "
           "bf16 (fast path: 5x the throughput, scores off by up to 1e-1), or a split-plane mode by name")
    a("--sim_precision", default="f32", choices=["f32", "bf16x3", "bf16"],
      help="similarity arithmetic of the SHARDED aligned build (world > 1): f32 = exact, bit-identical to one GPU (all-gathers "
           "fp32 rows); bf16x3 = bf16 hi/lo planes through the MFMA bf16 pipe (all-gathers the planes, scores within 5e-6); "
           "bf16 = one plane (outside the 1e-3 score contract)")
    a("--enc_batch", default=249, type=int,
      help="windows per encoder batch (83 k: whole rounds of the 256 x 256 tile on the 256 CUs; 166 measured +2 %% over 83, "
           "249 +1.3-2 %% more; ~37 GB of activations at 224^2).  Cut to texture.max_enc_batch(img_size) — the kernels' signed "
           "32-bit element offsets allow 267 clips at 224^2, 204 at 256^2; the bf16 path's dense clips 166 at 224^2")
    a("--enc_impl", default="auto", choices=["auto", "mfma", "module"],
      help="encoders at -e: SlowFast on the hand-written MFMA convolutions (auto/mfma) or the nn.Module on MIOpen (module); "
           "ResNet3d (resnet10/18/34/50) on the contract-grade MFMA kernels with mfma (fp32 = f16x3, or bf16x3; not bf16), "
           "the nn.Module with auto / module")
    a("--audio_resample", default="scipy", choices=["scipy", "kaiser_best"],
      help="how audio at another rate is brought to VGGish's 16 kHz (and to --audio_load_sr): scipy = scipy.signal.resample_poly on the "
           "host (default); kaiser_best = resampy's windowed-sinc interpolation with its default filter, what the reference computes "
           "(vggish_utils.py:27-69) — on the MI355X in validate() and with --train_input device (csrc/resample.hip), the same "
           "arithmetic in NumPy on the DataLoader's host path")
    a("--audio_load_sr", default=0, type=int,
      help="resample every decoded source and driving waveform to this rate first and round it to float32, as librosa.load does in "
           "the reference (validate.py:154, 172; 22050 is librosa's rate); audio samples per frame then follow this rate.  0 "
           "(default) keeps the file's rate")
    a("--dump_png", default=False, action="store_true",
      help="also write the reference's per-frame PNG folder (validate.py:789-792); default: frames go to the encoder directly")
    a("--vcam", default=False, action="store_true", help="defined for validate.py:299; CAM dumps are out of scope")
    return parser


parser = build_parser()


def main(args, video_name, itr=0):
    best_loss = 1000000
    resume_state = None  # the checkpoint's train_state, with --ckpt_train_state --resume
    rank, world, local = avt_dist.init_from_env(backend=getattr(args, "dist_backend", None))
    device = torch.device("cuda", local)
    if world > 1 and torch.distributed.get_backend() == "gloo":  # (gloo ranks may share one GPU; RCCL ranks have one each)
        device = torch.device("cuda", local % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(device)
    if not args.evaluate and not args.visualize_evaluate:
        dataset_train = AudioVideoSegments(args, video_name, split="train")
        train_loader = build_train_loader(args, dataset_train, device, rank, world)
    print("=> creating model '{}'".format(args.model_type))
    builder = ModelBuilder3D()
    q_image_enc_model, fc_dim = builder.build_network(arch=args.enc_arch, img_size=args.size, window=args.window)
    t_image_enc_model, fc_dim = builder.build_network(arch=args.enc_arch, img_size=args.size, window=args.window)
    audio_enc_model = VGGish()
    if os.path.isfile("pytorch_vggish.pth"):  # main.py:338 loads it unconditionally
        audio_enc_model.load_state_dict(torch.load("pytorch_vggish.pth", map_location="cpu"))
    else:
        print("pytorch_vggish.pth not found in cwd: VGGish keeps its random init")
    model = ContrastivePredictionTemporal(q_image_enc_model, t_image_enc_model, audio_enc_model, args.model_type,
                                          fc_dim, args.temp, args.window, args.stride, args.threshold,
                                          mini_batchsize=args.mini_batchsize, enc_arch=args.enc_arch,
                                          img_size=args.img_size)
    if args.resume:
        assert os.path.isfile(args.resume), "No checkpoint found at '{}'".format(args.resume)
        print("=> loading checkpoint '{}'".format(args.resume))
        checkpoint = torch.load(args.resume, map_location="cpu")
        if args.start_epoch is None:
            args.start_epoch = checkpoint["epoch"]
        best_loss = checkpoint["best_loss"]
        model.load_state_dict(checkpoint["state_dict"])
        print("=> loaded checkpoint '{}' (epoch {})".format(args.resume, checkpoint["epoch"]))
        if getattr(args, "ckpt_train_state", False) and not args.evaluate and not args.visualize_evaluate:
            if "train_state" not in checkpoint:
                from ._lib import AvtError

                raise AvtError("--ckpt_train_state with --resume: '%s' holds no train_state (it was written without the flag); resume "
                               "it without the flag: weights, epoch and best_loss only" % args.resume)
            resume_state = checkpoint["train_state"]
        elif "train_state" in checkpoint:
            print("=> checkpoint holds a train_state (optimizer, scheduler, generators, loader) that is not used: give "
                  "--ckpt_train_state to resume the run exactly")
        del checkpoint
    os.makedirs("./ckpt", exist_ok=True)
    tag = "{}_model_{}_vd_{}_vn_{}_bs_{}_".format(args.logname, args.model_type, os.path.split(args.vdata)[-1],
                                                  video_name, args.batch_size)
    if not args.evaluate:
        tag += "negs_{}_".format(args.n_negs)
    logname = tag + "w_{}_stride_{}_temp_{}_th_{}_enca_{}_subr_{}_eval_{}".format(
        args.window, args.stride, args.temp, args.threshold, args.enc_arch, args.subsample_rate,
        args.evaluate or args.visualize_evaluate)
    if args.evaluate and args.driving_audio is not None:
        logname += "alpha_{}_daf_{}".format(args.alpha, args.da_feats)
    if args.start_epoch is None:
        args.start_epoch = 0

    model = model.to(device)
    if args.evaluate and args.enc_dtype == "bf16" and args.enc_impl == "module":
        for enc in (model.q_encoder, model.t_encoder):
            enc.to(torch.bfloat16).to(memory_format=torch.channels_last_3d)
    if not args.evaluate and getattr(args, "train_layout", "ndhwc") == "ndhwc":
        # training layout on the MI355X: channels-last convolution weights (MIOpen's fwd / dgrad / wgrad then run without
        # layout transposes) and the fused train-mode BatchNorm + shortcut + ReLU passes of csrc/bn_train.hip, which work
        # on channels-last rows (train_ops.bn_act; fp32 step 95 -> 130 clips/s).  The BatchNorm passes compute
        # what stock fp32 BatchNorm computes (fp64 statistics); the CONVOLUTIONS' arithmetic is --train_conv's choice: x3 (the
        # default) is split-plane MFMA, not bit-for-bit fp32 — printed so that a log says which one trained the model.
        from . import train_ops

        model = train_ops.training_layout(model)
        train_ops.set_deterministic(False)  # (a process-wide switch: this run's flag decides, not an earlier run's)
        mode = train_ops.set_conv_mode(getattr(args, "train_conv", "x3"))
        if rank == 0:
            print("training convolutions: %s" % ("split-plane MFMA (x3: fp16 planes forward 2^-22, bf16 planes gradients 2^-16, "
                                                  "fp32 accumulation)" if mode == "x3" else "MIOpen fp32"))
        if getattr(args, "train_deterministic", False):
            train_ops.set_deterministic(True)  # (raises with --train_conv fp32)
            if rank == 0 and world == 1:
                print("training step: deterministic weight gradients (fixed-order reduction): bit-reproducible within one process on "
                      "one GPU with this build")
            elif rank == 0:
                print("training step: deterministic weight gradients (fixed-order reduction) and gradients summed in rank order across "
                      "the %d ranks (train_ops.GradExchange, ordered): bit-reproducible for one world size, one build and one GPU type"
                      % world)
    elif not args.evaluate and getattr(args, "train_deterministic", False):
        from ._lib import AvtError

        raise AvtError("--train_deterministic needs --train_layout ndhwc (the hand-written training kernels)")
    if world > 1 and not args.evaluate:  # weights resident per rank, gradients all-reduced over RCCL
        if getattr(args, "train_graph", 0) or getattr(args, "train_deterministic", False):
            # every rank replays its step as a HIP graph and the gradients cross the ranks in one flat buffer outside it (train.train):
            # no DistributedDataParallel wrapper, whose bucketed all-reduce is not captured — nor ordered: with --train_deterministic
            # the flat buffer is gathered and summed in rank order (train_ops.GradExchange.exchange), with or without the graph
            from . import train_ops

            model = train_ops.prepare_ranks(model)
        else:
            model = wrap_ddp(model, device, local)
    torch.backends.cudnn.benchmark = True
    tb_logdir = os.path.join(args.logdir, logname)
    os.makedirs(tb_logdir, exist_ok=True)
    tb_logger = Logger(tb_logdir) if rank == 0 else None

    if args.evaluate:
        # aligned mode: every rank takes part (its block of windows / rows, dist.sharded_survivors); compat mode keeps
        # the reference's per-step window map, which is one rank's work
        if rank == 0 or (world > 1 and args.stitch_mode == "aligned"):
            validate(model, args, video_name=video_name, tb_logger=tb_logger, model_type=args.model_type, itr=itr)
        return
    if getattr(args, "train_optimizer", "torch") == "hip":
        from .train_ops import ArenaSGD

        optimizer = ArenaSGD(model.parameters(), lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    else:
        optimizer = torch.optim.SGD(params=model.parameters(), lr=args.lr, momentum=args.momentum,
                                    weight_decay=args.weight_decay)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=args.lr_steps)
    with_state = bool(getattr(args, "ckpt_train_state", False))
    if resume_state is not None:
        load_train_state(resume_state, optimizer, scheduler, train_loader, device, world, args)
        if rank == 0:
            print("=> restored the training state: optimizer, scheduler (learning rate %s), generators and loader"
                  % ", ".join("%g" % g["lr"] for g in optimizer.param_groups))
    writer = None
    if getattr(args, "ckpt_async", False) and rank == 0:
        from .checkpoint import AsyncCheckpointWriter

        writer, snapshot = AsyncCheckpointWriter(), None
    print("Training for {} epochs.".format(args.epochs - args.start_epoch))
    try:
        for epoch in range(args.start_epoch, args.epochs):
            if world > 1:
                train_loader.sampler.set_epoch(epoch)
            loss = train(train_loader, model, optimizer, args, epoch, tb_logger)
            is_best = loss < best_loss
            best_loss = min(loss, best_loss)
            if rank == 0:
                net = model.module if hasattr(model, "module") else model
                extra = train_state(optimizer, scheduler, train_loader, device, world, args) if with_state else None
                if writer is None:
                    state = {"epoch": epoch + 1, "arch": args.enc_arch, "state_dict": net.state_dict(), "best_loss": best_loss}
                    if extra is not None:
                        state["train_state"] = extra
                    save_checkpoint(state, is_best, os.path.join(args.ckpt, logname))
                else:
                    snapshot = save_checkpoint_async(writer, snapshot, {"epoch": epoch + 1, "arch": args.enc_arch, "best_loss": best_loss},
                                                     net.state_dict(), extra, is_best, os.path.join(args.ckpt, logname))
            scheduler.step()
            if loss < 0.07:
                print("Loss {}. Stopping at epoch {}.".format(loss, epoch))
                break
    finally:
        if writer is not None:
            writer.close()  # (every file complete, or the writer's exception, before main() returns — the stop rule's break included)


def build_train_loader(args, dataset_train, device, rank, world):
    """What train() iterates, batch_size // world items per rank and step: the DataLoader over the host dataset (sharded by
    DistributedSampler across ranks), or with --train_input device the loader of dataset.DeviceSegmentBatcher — on every rank, each
    assembling its share of one global batch per step from rank 0's NumPy stream and one epoch order."""
    per = max(args.batch_size // world, 1)
    if getattr(args, "train_input", "loader") == "device":
        from .dataset import DeviceSegmentBatcher

        loader = DeviceSegmentBatcher(dataset_train, device, rank=rank, world=world).loader(per, shuffle=True, drop_last=True)
        if rank == 0:
            print("training input: batches assembled on the device: world %d, per-rank batch %d, global batch %d, %d steps per epoch"
                  % (world, per, per * world, len(loader)))
        return loader
    sampler = torch.utils.data.distributed.DistributedSampler(dataset_train) if world > 1 else None
    return torch.utils.data.DataLoader(dataset_train, batch_size=per, shuffle=sampler is None, sampler=sampler,
                                       num_workers=args.workers, drop_last=True)


def wrap_ddp(model, device, local):
    """DistributedDataParallel over RCCL in place of the reference's DataParallel (main.py:420): weights resident per rank,
    gradients all-reduced.  Modules that exist only so reference checkpoints load by key and are never applied — q_a_mlp /
    t_a_mlp (models.py:267-284) and VGGish's fc stack (vggish.py:45) — are frozen first: DDP's reducer would otherwise wait
    for gradients that never come (DataParallel tolerated them), and ~300 M dead parameters would be all-reduced every
    step.  find_unused_parameters covers plugin encoders with dead parameters of their own."""
    from . import train_ops

    train_ops.freeze_checkpoint_only_modules(model)
    ddp = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local] if device.type == "cuda" else None,
                                                    find_unused_parameters=True)
    if device.type == "cuda":
        ddp.register_comm_hook(None, _allreduce_after_every_stream)
    return ddp


def _allreduce_after_every_stream(_state, bucket):
    """DDP's default all-reduce (mean over ranks), started only after EVERY stream of the training forward has produced its
    part of the bucket: the query encoder runs on a side stream (models.ContrastivePredictionTemporal.forward) and autograd
    replays its backward there, while the reducer orders the collective after the stream of the LAST gradient only."""
    import torch.distributed as dist
    from . import models
    buf = bucket.buffer()
    cur = torch.cuda.current_stream(buf.device)
    for s in models.training_side_streams(buf.device) + [torch.cuda.default_stream(buf.device)]:
        if s != cur:
            cur.wait_stream(s)
    buf.div_(dist.get_world_size())
    return dist.all_reduce(buf, async_op=True).get_future().then(lambda f: f.value()[0])


def save_checkpoint(state, is_best, filename):
    torch.save(state, filename + "_latest.pth.tar")
    if is_best:
        shutil.copyfile(filename + "_latest.pth.tar", filename + "_best.pth.tar")


def save_checkpoint_async(writer, snapshot, head, state_dict, extra, is_best, filename):
    """save_checkpoint off the loop (--ckpt_async): the model's state_dict and, with a train_state, the optimizer's device tensors leave
    the device through train_ops.StateSnapshot (one launch, one copy; built at the first save and again whenever a tensor has moved),
    the writer's thread does the rest.  head: epoch, arch, best_loss.  -> the snapshot, for the next call."""
    from . import train_ops

    named = [("state_dict." + k, v) for k, v in state_dict.items() if v.is_cuda]
    opt = extra["optimizer"] if extra is not None else None
    if opt is not None:
        named += [("optimizer.%s.%s" % (i, k), v) for i, st in opt["state"].items() for k, v in st.items()
                  if isinstance(v, torch.Tensor) and v.is_cuda]
    if snapshot is None or snapshot.key != train_ops.StateSnapshot.key_of(named):
        snapshot = train_ops.StateSnapshot(named)
    handle = snapshot.take()
    metadata = getattr(state_dict, "_metadata", None)
    keys = [(k, None if v.is_cuda else v.clone()) for k, v in state_dict.items()]  # (host tensors of a state_dict: copied now)
    if opt is not None:  # the optimizer's state_dict with its device tensors taken out: the thread puts the host copies in
        extra = dict(extra, optimizer={"state": {i: {k: (None if isinstance(v, torch.Tensor) and v.is_cuda else v) for k, v in st.items()}
                                                 for i, st in opt["state"].items()},
                                       "param_groups": opt["param_groups"]})

    def make_state(tensors):
        sd = type(state_dict)((k, tensors["state_dict." + k] if v is None else v) for k, v in keys)
        if metadata is not None:
            sd._metadata = metadata
        state = {"epoch": head["epoch"], "arch": head["arch"], "state_dict": sd, "best_loss": head["best_loss"]}
        if extra is not None:
            if opt is not None:
                for i, st in extra["optimizer"]["state"].items():
                    for k in st:
                        if "optimizer.%s.%s" % (i, k) in tensors:
                            st[k] = tensors["optimizer.%s.%s" % (i, k)]
            state["train_state"] = extra
        return state

    writer.submit(handle, make_state, is_best, filename)
    return snapshot


def train_state(optimizer, scheduler, train_loader, device, world, args):
    """What --ckpt_train_state adds to a checkpoint: everything epoch e + 1 depends on besides the weights.  Taken where main() saves —
    after epoch e's train(), BEFORE scheduler.step(): load_train_state makes that step."""
    import numpy as np

    kind, words, pos, has_gauss, gauss = np.random.get_state()
    # (tensors and Python scalars only: main()'s torch.load of a checkpoint, as the reference's, unpickles nothing else)
    numpy_rng = {"kind": str(kind), "words": torch.from_numpy(np.asarray(words, np.int64)), "pos": int(pos), "has_gauss": int(has_gauss),
                 "gauss": float(gauss)}
    return {"optimizer": optimizer.state_dict(), "scheduler": scheduler.state_dict(),
            "torch_rng": torch.get_rng_state(), "device_rng": torch.cuda.get_rng_state(device), "numpy_rng": numpy_rng,
            "loader": train_loader.state_dict() if hasattr(train_loader, "state_dict") else None,
            "world": int(world), "train_deterministic": bool(getattr(args, "train_deterministic", False))}


def load_train_state(state, optimizer, scheduler, train_loader, device, world, args):
    """The inverse, on every rank, right before the epoch loop: the optimizer (momentum buffers; torch's SGD and train_ops.ArenaSGD read
    each other's), the scheduler — stepped once, the step the interrupted run made after it saved, so that the resumed epoch trains at
    the rate the uninterrupted run gives it — the generators, and the device loader's stream, seed and epoch."""
    import warnings

    import numpy as np
    from ._lib import AvtError

    if int(state["world"]) != int(world) or bool(state["train_deterministic"]) != bool(getattr(args, "train_deterministic", False)):
        print("=> the checkpoint's run had world %d, --train_deterministic %s; this one has world %d, %s: the resumed run will not "
              "repeat it bit for bit" % (state["world"], state["train_deterministic"], world, bool(getattr(args, "train_deterministic", False))))
    has_loader = hasattr(train_loader, "load_state_dict")
    if (state["loader"] is not None) != has_loader:
        raise AvtError("--ckpt_train_state: the checkpoint was written with --train_input %s, this run uses %s"
                       % ("device" if state["loader"] is not None else "loader", "device" if has_loader else "loader"))
    optimizer.load_state_dict(state["optimizer"])
    scheduler.load_state_dict(state["scheduler"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (torch warns that no optimizer.step() came before: it did, in the interrupted run)
        scheduler.step()
    if has_loader:
        train_loader.load_state_dict(state["loader"])
    rng = state["numpy_rng"]
    np.random.set_state((rng["kind"], rng["words"].numpy().astype(np.uint32), rng["pos"], rng["has_gauss"], rng["gauss"]))
    torch.cuda.set_rng_state(state["device_rng"].cpu(), device)
    torch.set_rng_state(state["torch_rng"].cpu())


def cli(argv=None):
    args = parser.parse_args(argv)
    print(args)
    assert os.path.exists(args.vdata), "No videos found at {}".format(args.vdata)
    if args.adata is not None and os.path.exists(args.adata):
        print("Audio found at {}".format(args.adata))
    if args.video_list is None:
        args.video_list = sorted([f.split(".")[0] for f in sorted(os.listdir(args.vdata)) if not f.startswith(".")])
    for itr, video_name in enumerate(args.video_list):
        args.results_folder = "results_{}".format(video_name)
        if args.evaluate or args.visualize_evaluate:
            _, fps = read_video(os.path.join(args.vdata, "{}.mp4".format(video_name)))
            if fps:
                args.fps = fps
            print("Frame rate: ", args.fps)
            args.window = math.ceil(args.fps / 2)  # [quirk Q10] overrides -w / -stride (main.py:515-516)
            args.stride = math.ceil(args.fps / 5)
            print("Stride {} Window {}".format(args.stride, args.window))
            if args.resume == "":
                args.resume = ("ckpt/exp_model_{}_vd_{}_vn_{}_bs_{}_negs_{}_w_{}_"
                               "stride_{}_temp_0.1_th_0.0_enca_{}_subr_{}_eval_False_best.pth.tar".format(
                                   args.model_type, os.path.split(args.vdata)[-1], video_name, args.batch_size,
                                   args.n_negs, args.window, args.stride, args.enc_arch, args.subsample_rate))
            assert os.path.isfile(args.resume), "No checkpoint found at '{}'".format(args.resume)
            print("=> loading checkpoint '{}'".format(args.resume))
            if args.driving_audio is not None:
                args.results_folder += "_target_{}_{}".format(
                    video_name, os.path.split(args.driving_audio[itr])[-1].split(".")[0])
        print("Starting video {}".format(video_name))
        main(args, video_name, itr)


if __name__ == "__main__":
    cli()
