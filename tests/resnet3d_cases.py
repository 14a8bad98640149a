"""The convolution shapes of the 3D-ResNet encoders on the split-plane kernels (fused_resnet3d.ResNet3dMFMA), one case per kernel
path, shared by the GPU comparison against float64 (tests/test_gpu_resnet3d_shapes.py) and the host guard that every path the
encoders run has a case (tests/test_resnet3d_plan.py).

A path class is (kernel symbol without its plane type, kernel, stride, tap table in global memory, K % 32 == 0): what
avt_conv3d_igemm_x3 decides per launch.  The tap table stays in LDS up to kMaxTabSteps = 128 K-steps of 64 (csrc/conv_args.h).
"""
import re
from collections import namedtuple

K_STEP = 64
MAX_TAB_STEPS = 128
XL = "conv_x3_xl_kernel"
T64 = "conv_x3_kernel<128,64,64>"
T128 = "conv_x3_kernel<128,128,64>"
# the split-plane error bound of tests/test_gpu_x3.py (TOL[mode] * max(scale, 1) + 2 * torch fp32's own error there)
TOL = {"bf16x3": 2e-5, "f16x3": 2e-6}

# symbol: what FusedConv.kernel_symbol names without the plane type; blocked: the XL tile's K-blocked weight planes (None: not
# the XL tile); res / relu: the layer's epilogue
Case = namedtuple("Case", "name cin cout kernel stride pad dims res relu symbol blocked")

K3, K1, S1, S2, P1, P0 = (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 2, 2), (1, 1, 1), (0, 0, 0)

CASES = [
    Case("layer1_conv2_res", 64, 64, K3, S1, P1, (2, 10, 56, 56), True, True, T64, None),
    Case("layer2_0_conv1", 64, 128, K3, S2, P1, (2, 10, 56, 56), False, True, T128, None),
    Case("layer2_0_downsample", 64, 128, K1, S2, P0, (2, 10, 56, 56), False, False, T128, None),
    Case("layer2_conv2_res", 128, 128, K3, S1, P1, (2, 5, 28, 28), True, True, T128, None),
    # layer3.0 at the production batch (133 clips at 224^2, W = 20 run it at M = 78204; 28 clips reach M = 16464)
    Case("layer3_0_conv1_xl", 128, 256, K3, S2, P1, (28, 5, 28, 28), False, True, XL, True),
    Case("layer3_conv2_res_xl", 256, 256, K3, S1, P1, (28, 3, 14, 14), True, True, XL, True),
    Case("layer3_0_downsample", 128, 256, K1, S2, P0, (28, 5, 28, 28), False, False, T128, None),  # K = 128 < 256
    # layer4.0 on both sides of the XL rule; at 168 clips two 256-wide N tiles
    Case("layer4_0_conv1", 256, 512, K3, S2, P1, (4, 3, 14, 14), False, True, T128, None),
    Case("layer4_0_conv1_xl", 256, 512, K3, S2, P1, (168, 3, 14, 14), False, True, XL, True),
    Case("layer4_0_downsample_xl", 256, 512, K1, S2, P0, (168, 3, 14, 14), False, False, XL, True),
    # layer4 conv2: K = 13824, 216 K-steps, the tap table read from global memory
    Case("layer4_conv2_res", 512, 512, K3, S1, P1, (4, 2, 7, 7), True, True, T128, None),
    Case("layer4_conv2_res_b133", 512, 512, K3, S1, P1, (133, 2, 7, 7), True, True, T128, None),
    # extents that shrink to one frame (W = 5 / 8)
    Case("t1_layer4_0_conv1", 256, 512, K3, S2, P1, (3, 1, 4, 4), False, True, T128, None),
    Case("t1_layer3_0_conv1", 128, 256, K3, S2, P1, (2, 2, 7, 7), False, True, T128, None),
    # the dispatcher's boundaries: M = 16383 | 16384, K = 8192 (128 steps, the table in LDS) | 8256 (129 steps)
    Case("boundary_m16383", 256, 256, K3, S1, P1, (1, 3, 43, 127), True, True, T128, None),
    Case("boundary_m16384", 256, 256, K3, S1, P1, (4, 4, 32, 32), True, True, XL, True),
    Case("boundary_k8192", 1024, 256, (2, 2, 2), S1, P0, (4, 5, 33, 33), False, True, XL, True),
    Case("boundary_k8256", 1032, 256, (2, 2, 2), S1, P0, (4, 5, 33, 33), False, True, T128, None),
    # XL with a K tail (K = 7128: no K-blocked weights)
    Case("xl_k_tail", 264, 256, K3, S1, P1, (4, 4, 32, 32), True, True, XL, False),
]


def out_dims(case):
    return (case.dims[0],) + tuple((n + 2 * p - k) // s + 1 for n, p, k, s in zip(case.dims[1:], case.pad, case.kernel, case.stride))


def m_out(case):
    b, t, h, w = out_dims(case)
    return b * t * h * w


def k_all(cin, kernel):
    return cin * kernel[0] * kernel[1] * kernel[2]


def n_ksteps(k):
    return -(-k // K_STEP)


def bare_symbol(symbol):
    """conv_x3_kernel<128,64,64,f16> -> conv_x3_kernel<128,64,64>; conv_x3_xl_kernel<bf16> -> conv_x3_xl_kernel."""
    return re.sub(r"<b?f16>$", "", re.sub(r",b?f16>$", ">", symbol))


def path_class(symbol, cin, kernel, stride):
    k = k_all(cin, kernel)
    return (bare_symbol(symbol), tuple(kernel), tuple(stride), n_ksteps(k) > MAX_TAB_STEPS, k % 32 == 0)


def case_class(case):
    return path_class(case.symbol, case.cin, case.kernel, case.stride)
