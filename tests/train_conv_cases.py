"""The training convolutions' launch plan: the smallest layers that reach every cell of train_ops._conv_x3_rows (form: general /
pixel-grouped / streaming pointwise; epilogue: BatchNorm backward statistics / forward statistics / none, with and without `add`),
_conv_wgrad and _dgrad_strided, and a recorder of what they send to the C ABI.  tools/record_train_conv_launches.py writes the
sequences to tests/golden/train_conv_launch_plan.json; tests/test_gpu_train_conv_plan.py requires a tree to reproduce them."""
import contextlib
import ctypes as C

import torch
import torch.nn as nn

DEV = "cuda:0"
RECORDED = ("avt_conv3d_igemm_x3_f32", "avt_pw_x3_f32", "avt_conv3d_wgrad_x3")  # prefixes of the entries whose calls are noted


class _Proxy:
    """Stands in for _lib.checked: every entry is forwarded; the RECORDED ones leave (name, arguments) behind first — scalars as given,
    pointers only as "ptr" / "null" (no address is kept: the plan is the same on every machine and in every process)."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith(RECORDED):
            return fn
        from avtex import _lib
        types = _lib.SIGNATURES[name]

        def call(*args):
            assert len(args) == len(types), (name, len(args), len(types))
            noted = []
            for a, ty in zip(args, types):
                if ty in (C.c_void_p, C.c_char_p):
                    value = a.value if isinstance(a, (C.c_void_p, C.c_char_p)) else a  # (None, an int, or a ctypes array)
                    noted.append("null" if value is None or (isinstance(value, int) and value == 0) else "ptr")
                else:
                    assert isinstance(a, (int, float)), (name, a)
                    noted.append(int(a) if isinstance(a, bool) else a)
            self._calls.append([name, noted])
            return fn(*args)

        return call


@contextlib.contextmanager
def recorded():
    """-> the list that fills with [name, arguments] of every RECORDED entry called through ops.K / train_ops.K inside the block."""
    from avtex import ops, train_ops
    calls = []
    keep = (ops.K, train_ops.K)
    ops.K = train_ops.K = _Proxy(keep[0], calls)
    try:
        yield calls
    finally:
        ops.K, train_ops.K = keep


def _conv(cin, cout, kernel, stride=(1, 1, 1), pad=(0, 0, 0)):
    return nn.Conv3d(cin, cout, kernel, stride=stride, padding=pad, bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()


def _bn(c):
    return nn.BatchNorm3d(c).to(DEV).train()


def _clip(b, c, t, h, w, grad=True):
    x = torch.randn(b, c, t, h, w, device=DEV).contiguous(memory_format=torch.channels_last_3d)
    return x.requires_grad_(grad)


def _chain(cin, cout, kernel, stride=(1, 1, 1), pad=(0, 0, 0), dims=(2, 2, 8, 8), fork=False):
    """bn_act(conv3d(x, conv1, stats=bn1), bn1) -> conv3d(., conv2, stats=bn2) -> bn_act -> sum, conv2 the layer under test: its input
    gradient is the output gradient of a fused BatchNorm.  conv1 is the pointwise cin -> cin layer (x wants a gradient too: the same
    width's pointwise input gradient with no BatchNorm behind it).  fork: conv2 through conv3d_fork, its alias consumed."""
    def run():
        from avtex import train_ops
        conv1, bn1, conv2, bn2 = _conv(cin, cin, (1, 1, 1)), _bn(cin), _conv(cin, cout, kernel, stride, pad), _bn(cout)
        x = _clip(dims[0], cin, *dims[1:])
        h = train_ops.bn_act(train_ops.conv3d(x, conv1, stats=bn1), bn1)
        if fork:
            y, alias = train_ops.conv3d_fork(h, conv2, stats=bn2)
            loss = train_ops.bn_act(y, bn2).square().sum() + alias.square().sum()
        else:
            loss = train_ops.bn_act(train_ops.conv3d(h, conv2, stats=bn2), bn2).square().sum()
        loss.backward()
    return run


def _vggish():
    """conv2d: 1 -> 64 (the input wants no gradient: the padded-channel weight gradient) and 64 -> 128, kernel 3 pad 1, on 2 x C x 16 x 16."""
    from avtex import train_ops
    c1, c2 = nn.Conv2d(1, 64, 3, padding=1).to(DEV).train(), nn.Conv2d(64, 128, 3, padding=1).to(DEV).train()
    x = torch.randn(2, 1, 16, 16, device=DEV)
    train_ops.conv2d(torch.relu(train_ops.conv2d(x, c1)), c2).square().sum().backward()


def _stem():
    """3 -> 64, kernel (5,7,7), stride (1,2,2), pad (2,3,3) on 2 x 3 x 4 x 16 x 16 with the patch-resident stem kernels off: the generic
    route (the clip zero-padded to 8 channels, the weight gradient as kt slices of wgrad_x3_sub)."""
    from avtex import train_ops
    keep, train_ops._STEM_PATCH = train_ops._STEM_PATCH, 0
    try:
        stem, bn = _conv(3, 64, (5, 7, 7), (1, 2, 2), (2, 3, 3)), _bn(64)
        x = _clip(2, 3, 4, 16, 16, grad=False)
        train_ops.bn_act(train_ops.conv3d(x, stem, stats=bn), bn).square().sum().backward()
    finally:
        train_ops._STEM_PATCH = keep


S3, P3 = (1, 3, 3), (0, 1, 1)
# id -> (run, replica-group settings); every case runs as written on the commit the golden file was recorded at (no extent adjusted)
CASES = {
    "a_general_64_64_k133": (_chain(64, 64, S3, pad=P3), (1, 2)),
    "b_strided_64_64_k133_s122": (_chain(64, 64, S3, (1, 2, 2), P3), (1, 2)),
    "c_temporal_64_64_k311": (_chain(64, 64, (3, 1, 1), pad=(1, 0, 0)), (1, 2)),
    "d_grouped4_8_8_k133": (_chain(8, 8, S3, pad=P3), (1, 2)),
    "e_temporal_group_8_8_k511": (_chain(8, 8, (5, 1, 1), pad=(2, 0, 0)), (1, 2)),
    "e_temporal_group_8_32_k511": (_chain(8, 32, (5, 1, 1), pad=(2, 0, 0)), (1, 2)),
    "f_grouped_wide_16_64_k133": (_chain(16, 64, S3, pad=P3), (1, 2)),
    "g_grouped2_32_32_k133": (_chain(32, 32, S3, pad=P3), (1, 2)),
    "h_grouped_w6_8_8_k133": (_chain(8, 8, S3, pad=P3, dims=(2, 2, 8, 6)), (1, 2)),
    "i_pointwise_64_256": (_chain(64, 256, (1, 1, 1)), (1, 2)),
    "i_pointwise_256_64": (_chain(256, 64, (1, 1, 1)), (1, 2)),
    "j_pointwise_refused_96_64": (_chain(96, 64, (1, 1, 1)), (1, 2)),
    "k_fork_general_64_64_k133": (_chain(64, 64, S3, pad=P3, fork=True), (1, 2)),
    "k_fork_grouped4_8_8_k133": (_chain(8, 8, S3, pad=P3, fork=True), (1, 2)),
    "k_fork_pointwise_64_256": (_chain(64, 256, (1, 1, 1), fork=True), (1, 2)),
    "k_fork_pointwise_256_64": (_chain(256, 64, (1, 1, 1), fork=True), (1, 2)),
    "l_tile256_256_256_k133_m65536": (_chain(256, 256, S3, pad=P3, dims=(1, 4, 128, 128)), (1,)),
    "m_vggish_conv2d": (_vggish, (1, 2)),
    "n_stem_generic_3_64_k577": (_stem, (1, 2)),
}


def settings(case):
    """The settings a case runs in: (key, replica groups, _EPI_STATS = _EPI_BWD)."""
    return [("groups%d_epi%d" % (g, e), g, e) for g in CASES[case][1] for e in (1, 0)]


def launches(case, groups, epi):
    """One forward + backward of the case under bn_replicas(groups) with both epilogue switches = epi -> its recorded calls."""
    from avtex import train_ops
    keep = (train_ops._EPI_STATS, train_ops._EPI_BWD)
    train_ops._EPI_STATS = train_ops._EPI_BWD = epi
    torch.manual_seed(0)
    try:
        with train_ops.bn_replicas(groups), recorded() as calls:
            CASES[case][0]()
        torch.cuda.synchronize()
    finally:
        train_ops._EPI_STATS, train_ops._EPI_BWD = keep
    return calls


def plan(case):
    return {key: launches(case, g, e) for key, g, e in settings(case)}
