"""Host side of the device training input path: the CLI switch, and what DeviceSegmentBatcher and its ops refuse without a GPU."""
from types import SimpleNamespace

import pytest
import torch


def test_parser_knows_train_input(avt):
    from avtex.main import build_parser

    p = build_parser()
    assert p.parse_args([]).train_input == "loader"
    assert p.parse_args(["--train_input", "device"]).train_input == "device"
    with pytest.raises(SystemExit):
        p.parse_args(["--train_input", "host"])


def test_batcher_still_refuses_the_validation_split(avt):
    from avtex.dataset import DeviceSegmentBatcher

    for arch in ("resnet18", "slowfast"):
        args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=8, img_size=16, enc_arch=arch, window=0, stride=0)
        torch.manual_seed(0)
        ds = avt.AudioVideoSegments(args, "x", split="val", video=(torch.zeros((60, 16, 16, 3), dtype=torch.uint8), 10.0))
        with pytest.raises(ValueError):
            DeviceSegmentBatcher(ds, "cpu")


def test_new_ops_reject_host_tensors(avt):
    with pytest.raises(avt._lib.AvtError):
        avt.ops.frames_resize_aa_norm(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), 4)
    with pytest.raises(avt._lib.AvtError):
        avt.ops.clip_gather_frames(torch.zeros((4, 3, 8, 8)), torch.zeros(2, dtype=torch.int32), 2)
