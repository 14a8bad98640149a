"""The deterministic weight gradients (include/avt.h; csrc/wgrad_x3.hip and csrc/stem_train.hip with the storing epilogue,
csrc/wgrad_reduce.hip): per layer case, on fp32 NDHWC rows with seeded inputs,
  (a) two calls on the same inputs are bit-equal — the workspace filled with NaN and dW with a sentinel before each call, and dW's
      columns beyond E keep the sentinel where ldw > E;
  (b) the relative norm error against an fp64 weight gradient is below 1e-4 (the bound of this arithmetic in test_gpu_train_conv.py:
      bf16 planes, 2^-16 per product; only the fp32 summation tree differs from the atomic entry's);
  (c) the result agrees with the atomic entry on the same inputs to 2e-4;
  (d) the case really reduces across chunks: the workspace holds at least two partial filters.
The cases are the smallest that reach each tile form of the deterministic dispatch (128 x {32, 64, 128} outputs, either orientation,
buffer or plain loads; the stems' three instances): the form a case lands on is asserted through the library's per-form launch counter,
and one test asserts that the cases together cover every form."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5

# name: cin, cout, kernel, stride, pad, dims (b, t, h, w), extra dW columns, tile form (bn, swap)
CONV_CASES = {
    "3x3x3-8-16": (8, 16, (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 4, 12, 12), 12, (32, 0)),     # E = 216: a full and a ragged 128-tile, ragged cout
    "pointwise-64-256": (64, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 2, 14, 14), 0, (64, 1)),  # cout > E: swapped; 392 positions: ragged slab
    "1x3x3-s2-32-64": (32, 64, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 3, 15, 15), 0, (64, 0)),  # odd extents
    "7x1x1-s4-8-16": (8, 16, (7, 1, 1), (4, 1, 1), (3, 0, 0), (1, 16, 7, 7), 0, (32, 0)),
    # ... and the forms those four leave out
    "1x3x3-16-72": (16, 72, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 4, 9, 9), 4, (128, 0)),      # E = 144 (ragged second tile), cout 72 of 128
    "pointwise-72-136": (72, 136, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 3, 9, 9), 0, (128, 1)),  # swapped, two co tiles, E = 72 of 128
    "pointwise-8-32": (8, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 4, 8, 8), 0, (32, 1)),      # swapped, E = 8 of a 32-wide tile
}
_REF = {}


def _conv_case(name):
    """Inputs, the fp64 reference and the atomic entry's result of a case: computed once, shared by its tests, never written to."""
    if name not in _REF:
        from avtex import ops
        cin, cout, kernel, stride, pad, dims, extra, form = CONV_CASES[name]
        b, t, h, w = dims
        g = torch.Generator(DEV).manual_seed(sum(map(ord, name)))
        x = torch.randn(b, t, h, w, cin, device=DEV, generator=g)
        wgt = torch.zeros(cout, cin, *kernel, device=DEV, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3).double(), wgt, stride=stride, padding=pad)
        dy = torch.randn(y.shape[0], y.shape[2], y.shape[3], y.shape[4], cout, device=DEV, generator=g)
        y.backward(dy.permute(0, 4, 1, 2, 3).double())
        ref = wgt.grad.permute(0, 2, 3, 4, 1).reshape(cout, -1).contiguous()  # [cout][taps * cin] fp64
        atomic = torch.empty(cout, ref.shape[1], device=DEV)
        ops.conv3d_wgrad_x3_f32(dy, x, atomic, dims, cin, cout, kernel, stride, pad, cin, cout)
        _REF[name] = (x, dy, ref, atomic)
    return _REF[name]


def _rel(u, v):
    return float((u.double() - v.double()).norm()) / float(v.double().norm())


def _form_count(bn, swap, buf):
    from avtex import _lib
    return _lib.lib().avt_conv3d_wgrad_x3_det_launches(bn, swap, buf)


@pytest.mark.parametrize("buf", [1, 0], ids=["buffer-loads", "plain-loads"])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_weight_gradient_is_bit_reproducible_and_right(name, buf):
    from avtex import _lib, ops
    cin, cout, kernel, stride, pad, dims, extra, (bn, swap) = CONV_CASES[name]
    x, dy, ref, atomic = _conv_case(name)
    e = ref.shape[1]
    ldw = e + extra
    need = ops.conv3d_wgrad_x3_det_ws_bytes(dims, cin, cout, kernel, stride, pad, (0, 0, 0), cin, cout, ldw)
    assert need >= 2 * cout * e * 4 and need % (cout * e * 4) == 0, (need, cout * e * 4)  # (d)
    before = _form_count(bn, swap, buf)
    _lib.lib().avt_wgrad_x3_set_xl(6 if buf else 5)  # the phase-serial tile's buffer-load form on / off
    try:
        outs = []
        for _ in range(2):
            ws = torch.full((need // 4,), float("nan"), device=DEV)
            dw = torch.full((cout, ldw), SENTINEL, device=DEV)
            ops.conv3d_wgrad_x3_det_sub_f32(dy, x, dw, dims, cin, cout, kernel, stride, pad, (0, 0, 0), cin, cout, ldw, ws=ws)
            outs.append(dw)
    finally:
        _lib.lib().avt_wgrad_x3_set_xl(6)
    torch.cuda.synchronize()
    assert _form_count(bn, swap, buf) == before + 2  # the tile form this case is here for, by the library's own count
    assert torch.equal(outs[0], outs[1])  # (a)
    assert bool((outs[0][:, e:] == SENTINEL).all())  # columns beyond E are not the call's to write
    got = outs[0][:, :e]
    assert bool(torch.isfinite(got).all())  # nothing of the NaN workspace was read unwritten
    e64, eat = _rel(got, ref), _rel(got, atomic)
    print("det wgrad %s buf=%d: %d chunks, vs fp64 %.2e (atomic entry %.2e), vs atomic entry %.2e" % (name, buf, need // (cout * e * 4), e64,
                                                                                                 _rel(atomic, ref), eat))
    assert e64 < 1e-4, e64  # (b)
    assert eat < 2e-4, eat  # (c)


def test_resnet_stem_route_seven_slices_into_one_filter():
    """cin 4 (of 8-channel rows), [1,7,7], stride (1,2,2): the 3D-ResNet stem's [7,7,7] filter as seven frame-tap slices, each a call of
    its own that writes its E = 196 columns of dW's rows (ldw = 7 E); the slices are disjoint and the whole filter is compared."""
    from avtex import ops
    cout, kt, dims = 64, 7, (1, 8, 16, 16)
    b, t, h, w = dims
    g = torch.Generator(DEV).manual_seed(77)
    x = torch.randn(b, t, h, w, 8, device=DEV, generator=g)
    x[..., 3:] = 0.0  # the forward's zero-padded clip: 3 channels travel as 4 of 8
    wgt = torch.zeros(cout, 4, kt, 7, 7, device=DEV, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv3d(x[..., :4].permute(0, 4, 1, 2, 3).double(), wgt, stride=(1, 2, 2), padding=(3, 3, 3))
    out_dims = tuple(y.shape[2:])
    dy = torch.randn(b, *out_dims, cout, device=DEV, generator=g)
    y.backward(dy.permute(0, 4, 1, 2, 3).double())
    ref = wgt.grad.permute(0, 2, 3, 4, 1).reshape(cout, kt, 49 * 4)
    e, ldw = 49 * 4, kt * 49 * 4
    need = ops.conv3d_wgrad_x3_det_ws_bytes(dims, 4, cout, (1, 7, 7), (1, 2, 2), (3, 3, 3), out_dims, 8, cout, ldw)
    assert need >= 2 * cout * e * 4  # (d)
    before = _form_count(64, 0, 1)

    def run(det):
        acc = torch.full((cout, kt, e), SENTINEL if det else 0.0, device=DEV)
        for dt in range(kt):
            if det:
                ws = torch.full((need // 4,), float("nan"), device=DEV)
                ops.conv3d_wgrad_x3_det_sub_f32(dy, x, acc[:, dt], dims, 4, cout, (1, 7, 7), (1, 2, 2), (3 - dt, 3, 3), out_dims, 8, cout, ldw, ws=ws)
            else:
                ops.conv3d_wgrad_x3_sub_f32(dy, x, acc[:, dt], dims, 4, cout, (1, 7, 7), (1, 2, 2), (3 - dt, 3, 3), out_dims, 8, cout, ldw, False)
        return acc

    a0, a1, atomic = run(True), run(True), run(False)
    torch.cuda.synchronize()
    assert _form_count(64, 0, 1) == before + 2 * kt
    assert torch.equal(a0, a1) and bool(torch.isfinite(a0).all()) and not bool((a0 == SENTINEL).any())  # (a): every column written once
    assert _rel(a0, ref) < 1e-4, _rel(a0, ref)  # (b)
    assert _rel(a0, atomic) < 2e-4, _rel(a0, atomic)  # (c)


# kt, cout, clip dims (b, t, h, w): 64^2 = 32 pixel pairs per row
STEM_CASES = {"fast": (5, 8, (2, 8, 64, 64)), "slow": (1, 64, (2, 3, 64, 64)), "kt1-8-channels": (1, 8, (1, 2, 64, 64))}


@pytest.mark.parametrize("name", list(STEM_CASES))
def test_patch_stem_weight_gradient_is_bit_reproducible_and_right(name):
    from avtex import _lib, ops
    kt, cout, (b, t, h, w) = STEM_CASES[name]
    g = torch.Generator(DEV).manual_seed(kt * 100 + cout)
    x = torch.randn(b, 3, t, h, w, device=DEV, generator=g)
    wgt = torch.zeros(cout, 3, kt, 7, 7, device=DEV, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv3d(x.double(), wgt, stride=(1, 2, 2), padding=(kt // 2, 3, 3))
    dy = torch.randn(b, t, h // 2, w // 2, cout, device=DEV, generator=g)  # NDHWC rows
    y.backward(dy.permute(0, 4, 1, 2, 3).double())
    xh, xl = ops.clip_planes_f32(x, ops.X3_BF16)
    args = (xh, xl, dy, b, t, h, w // 2, cout, kt, kt // 2)
    need = ops.stem_wgrad_x3_det_ws_bytes(*args[3:])
    assert need >= 2 * cout * kt * 7 * 32 * 4  # (d): at least two persistent workgroups' partial filters
    count = lambda: _lib.lib().avt_stem_wgrad_x3_det_launches(kt, 8 if cout == 8 else 16)
    before = count()
    outs = []
    for _ in range(2):
        ws = torch.full((need // 4,), float("nan"), device=DEV)
        dw = torch.full((cout, kt, 7, 4, 8), SENTINEL, device=DEV)
        assert ops.stem_wgrad_x3_det(*args, ws=ws, dw=dw) is dw
        outs.append(dw)
    atomic = ops.stem_wgrad_x3(*args)
    torch.cuda.synchronize()
    assert count() == before + 2
    assert torch.equal(outs[0], outs[1])  # (a)
    assert bool(torch.isfinite(outs[0]).all()) and not bool((outs[0] == SENTINEL).any())  # the whole pair-form filter is written
    as_weight = lambda p: p.view(cout, kt, 7, 8, 4)[:, :, :, 1:, :3].permute(0, 4, 1, 2, 3)  # column tap k = 2 * pair + pixel - 1
    e64, eat = _rel(as_weight(outs[0]), wgt.grad), _rel(as_weight(outs[0]), as_weight(atomic))
    print("det stem wgrad %s: vs fp64 %.2e (atomic entry %.2e), vs atomic entry %.2e" % (name, e64, _rel(as_weight(atomic), wgt.grad), eat))
    assert e64 < 1e-4, e64  # (b)
    assert eat < 2e-4, eat  # (c)


def test_the_cases_cover_every_form_the_deterministic_dispatch_can_reach():
    """128 x {32, 64, 128} outputs in either orientation (each run with buffer and with plain loads above), and the three stem instances
    the deterministic entry launches (kt = 5 with 16-channel slices does not fit the LDS and is refused: test_abi_ext.py)."""
    assert {c[-1] for c in CONV_CASES.values()} == {(bn, swap) for bn in (32, 64, 128) for swap in (0, 1)}
    assert {(kt, 8 if co == 8 else 16) for kt, co, _ in STEM_CASES.values()} == {(5, 8), (1, 16), (1, 8)}


def test_training_convolutions_route_through_the_deterministic_entries():
    """train_ops.set_deterministic(True): _conv_wgrad's branches (plain, 8-channel padded, stem slices) and _StemX3.backward launch the
    deterministic entries — counted — and two backward passes give the same bits; CALLS keeps its other rows' counts."""
    import torch.nn as nn
    from avtex import train_ops
    cl = lambda v: v.contiguous(memory_format=torch.channels_last_3d)
    layers = [
        (nn.Conv3d(16, 24, (1, 3, 3), padding=(0, 1, 1), bias=False), (2, 16, 2, 10, 10), dict(wgrad_x3=1, wgrad_det=1)),
        (nn.Conv3d(3, 8, (5, 7, 7), stride=(1, 2, 2), padding=(2, 3, 3), bias=False), (1, 3, 8, 64, 64), dict(wgrad_stem_patch=1, wgrad_det=1)),
        (nn.Conv3d(3, 64, (7, 7, 7), stride=(1, 2, 2), padding=(3, 3, 3), bias=False), (1, 3, 8, 32, 32), dict(wgrad_stem_x3=1, wgrad_det=7)),
    ]
    assert train_ops.set_deterministic(True) is False
    try:
        for conv, shape, want in layers:
            conv = conv.to(DEV).to(memory_format=torch.channels_last_3d).train()
            g = torch.Generator(DEV).manual_seed(shape[1])
            x = torch.randn(shape, device=DEV, generator=g)
            x = cl(x) if shape[1] != 3 else x
            assert train_ops.conv_fusable(x, conv)
            grads = []
            for rep in range(2):
                conv.zero_grad(set_to_none=True)
                before = dict(train_ops.CALLS)
                y = train_ops.conv3d(x, conv)
                y.backward(cl(torch.randn(y.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(5))))
                ran = {k: train_ops.CALLS[k] - before[k] for k in before}
                assert all(ran[k] == v for k, v in want.items()) and ran["miopen_wgrad"] == 0, ran
                grads.append(conv.weight.grad.clone())
            assert torch.equal(grads[0], grads[1])
            ref = nn.Conv3d(conv.in_channels, conv.out_channels, conv.kernel_size, stride=conv.stride, padding=conv.padding, bias=False).to(DEV).double()
            ref.weight.data.copy_(conv.weight.detach().double())
            ref(x.double()).backward(cl(torch.randn(y.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(5))).double())
            assert _rel(grads[0], ref.weight.grad) < 1e-4
    finally:
        train_ops.set_deterministic(False)
