"""3D-ResNet encoder plugins for the non-SlowFast path: forward([B,3,T,H,W]) -> [B,C',t,h,w].

Same layer layout and state-dict keys as the reference's Kensho-Hara style network
(contrastive_video_textures/models/video_models/resnet3d.py:119-191, factories :223-318), including
its final fixed-size AvgPool3d (the operator pools again with AdaptiveAvgPool3d(1), models.py:253-260)
and [quirk] that "resnet50" is built from BasicBlocks (resnet3d.py:265-304).  ResNeXt/DenseNet
factories of the reference cannot be reached (kwarg mismatch) and are not built.

MI355X notes: this nn.Module is the weight container and the plugin surface.  At `-e --enc_impl mfma` its weights run on
fused_resnet3d.ResNet3dMFMA; in train mode, in the training layout (channels_last_3d), its convolutions / BatchNorms / stem pool run on
the hand-written passes of train_ops, as SlowFast's do.  The fixed AvgPool3d head stays a torch op (a few KB).
"""
import math

import torch.nn as nn

from .train_ops import bn_act, conv3d, conv3d_fork, max_pool3d


def _is_projection(m):
    return isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[0], nn.Conv3d) and isinstance(m[1], nn.BatchNorm3d)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv3d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm3d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv3d(planes, planes, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm3d(planes)
        self.downsample = downsample

    def forward(self, x):
        # (train mode on the GPU in the training layout: the hand-written passes of train_ops — the shortcut's / projection's gradient
        #  is summed in conv1's input-gradient launch, BatchNorm statistics ride on the convolutions' epilogues, bn2 + shortcut + ReLU
        #  is one pass; every entry is the module's own op otherwise, so eval mode and the CPU compute what they always did)
        y, xs = conv3d_fork(x, self.conv1, stats=self.bn1)
        if self.downsample is None:
            r = xs
        elif _is_projection(self.downsample):
            r = bn_act(conv3d(xs, self.downsample[0], stats=self.downsample[1]), self.downsample[1], relu=False)
        else:
            r = self.downsample(xs)
        y = bn_act(y, self.bn1, relu=True)
        return bn_act(conv3d(y, self.conv2, stats=self.bn2), self.bn2, res=r, relu=True)


class ResNet3d(nn.Module):
    def __init__(self, layers, sample_size, sample_duration):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv3d(3, 64, 7, stride=(1, 2, 2), padding=(3, 3, 3), bias=False)
        self.bn1 = nn.BatchNorm3d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool3d(3, stride=2, padding=1)
        self.layer1 = self._make(64, layers[0], 1)
        self.layer2 = self._make(128, layers[1], 2)
        self.layer3 = self._make(256, layers[2], 2)
        self.layer4 = self._make(512, layers[3], 2)
        self.avgpool = nn.AvgPool3d((int(math.ceil(sample_duration / 16)), int(math.ceil(sample_size / 32)),
                                     int(math.ceil(sample_size / 32))), stride=1)
        self.fc_dim = 512
        self.fc = nn.Linear(512, 1039)  # present in the reference's checkpoints, never applied
        for m in self.modules():
            if isinstance(m, nn.Conv3d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")

    def _make(self, planes, blocks, stride):
        down = None
        if stride != 1 or self.inplanes != planes:
            down = nn.Sequential(nn.Conv3d(self.inplanes, planes, 1, stride=stride, bias=False), nn.BatchNorm3d(planes))
        layers = [BasicBlock(self.inplanes, planes, stride, down)]
        self.inplanes = planes
        layers += [BasicBlock(planes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x):
        x = max_pool3d(bn_act(conv3d(x, self.conv1, stats=self.bn1), self.bn1, relu=True), self.maxpool)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.avgpool(x)


LAYERS = {"resnet10": [1, 1, 1, 1], "resnet18": [2, 2, 2, 2], "resnet34": [3, 4, 6, 3], "resnet50": [3, 4, 6, 3]}


def build(arch, sample_size, sample_duration):
    return ResNet3d(LAYERS[arch], sample_size, sample_duration)
