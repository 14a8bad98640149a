"""The deterministic weight-gradient entries (include/avt.h) on the host: the workspace queries answer from the geometry alone, bad
geometry and bad workspaces are refused before any launch, and the Python wrappers refuse host tensors and the fp32 mode.  No device
calls here."""
import pytest
import torch

AVT_ERR_ARG = -1  # include/avt.h


# batch t h w cin cout kt kh kw st sh sw pt ph pw to ho wo ldx ldy ldw
_GEOM = dict(batch=2, t=4, h=12, w=12, cin=8, cout=16, kt=3, kh=3, kw=3, st=1, sh=1, sw=1, pt=1, ph=1, pw=1, to=0, ho=0, wo=0,
             ldx=8, ldy=16, ldw=0)
_ORDER = "batch t h w cin cout kt kh kw st sh sw pt ph pw to ho wo ldx ldy ldw".split()
_STEM = dict(batch=2, t=8, h=64, pw=32, cout=8, kt=5, pt=2)
_STEM_ORDER = "batch t h pw cout kt pt".split()


def _g(base, order, **bad):
    return [dict(base, **bad)[k] for k in order]


def test_workspace_queries_answer_geometry_alone(avt):
    lib = avt._lib.lib()
    e = 27 * 8
    one = 16 * e * 4
    n = lib.avt_conv3d_wgrad_x3_det_ws_bytes(*_g(_GEOM, _ORDER))
    assert n > 0 and n % one == 0 and n >= 2 * one  # whole chunks of [cout][E] fp32, more than one of them (18 slabs of positions)
    assert lib.avt_conv3d_wgrad_x3_det_ws_bytes(*_g(_GEOM, _ORDER, ldw=e + 12)) == n  # the workspace is compact whatever dW's pitch
    for bad in (dict(cin=6), dict(cout=12), dict(kh=8, kw=8), dict(st=0), dict(batch=0), dict(ldx=4), dict(ldw=e - 4), dict(t=1, pt=0),
                dict(batch=1 << 12, h=1024, w=1024)):
        assert lib.avt_conv3d_wgrad_x3_det_ws_bytes(*_g(_GEOM, _ORDER, **bad)) <= 0, bad
    s = lib.avt_stem_wgrad_x3_det_ws_bytes(*_g(_STEM, _STEM_ORDER))
    units = 2 * 8 * (32 // 4)  # (clip, input frame, 4-row group): one persistent workgroup each at this size
    assert s == units * 8 * 5 * 7 * 32 * 4
    slow = lib.avt_stem_wgrad_x3_det_ws_bytes(*_g(_STEM, _STEM_ORDER, cout=64, kt=1, pt=0, t=3))
    assert slow == (2 * 3 * 8) * 64 * 7 * 32 * 4
    for bad in (dict(h=62), dict(pw=4), dict(kt=3, pt=1), dict(cout=12), dict(pt=5), dict(batch=0), dict(cout=16)):
        assert lib.avt_stem_wgrad_x3_det_ws_bytes(*_g(_STEM, _STEM_ORDER, **bad)) <= 0, bad
    assert "LDS" in lib.avt_last_error().decode()  # kt = 5 with 16-channel slices: refused here, not at the launch
    assert lib.avt_conv3d_wgrad_x3_det_launches(48, 0, 1) == -1 and lib.avt_conv3d_wgrad_x3_det_launches(32, 0, 1) >= 0
    assert lib.avt_stem_wgrad_x3_det_launches(3, 8) == -1 and lib.avt_stem_wgrad_x3_det_launches(5, 8) >= 0


_P = [0x10000 * (i + 1) for i in range(6)]  # made-up device addresses, 16-byte aligned, never dereferenced


def _conv_args(ws, ws_bytes, ptrs=(_P[0], _P[1], _P[2]), **bad):
    return list(ptrs) + _g(_GEOM, _ORDER, **bad) + [ws, ws_bytes, 0]


def _stem_args(ws, ws_bytes, ptrs=(_P[0], _P[1], _P[2], _P[3]), **bad):
    return list(ptrs) + _g(_STEM, _STEM_ORDER, **bad) + [ws, ws_bytes, 0]


# (with made-up addresses a check that went missing would be a real launch: never where a device is visible)
@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only on a box without a GPU")
def test_bad_workspaces_and_arguments_are_rejected_before_any_launch(avt):
    lib, checked = avt._lib.lib(), avt._lib.checked
    need = lib.avt_conv3d_wgrad_x3_det_ws_bytes(*_g(_GEOM, _ORDER))
    sneed = lib.avt_stem_wgrad_x3_det_ws_bytes(*_g(_STEM, _STEM_ORDER))
    before = [lib.avt_conv3d_wgrad_x3_det_launches(bn, s, b) for bn in (32, 64, 128) for s in (0, 1) for b in (0, 1)]
    sbefore = [lib.avt_stem_wgrad_x3_det_launches(kt, co) for kt in (1, 5) for co in (8, 16)]
    cases = [
        ("avt_conv3d_wgrad_x3_det_sub_f32", _conv_args(None, need), "workspace must be a 16-byte aligned device pointer"),
        ("avt_conv3d_wgrad_x3_det_sub_f32", _conv_args(_P[4] + 4, need), "workspace must be a 16-byte aligned device pointer"),
        ("avt_conv3d_wgrad_x3_det_sub_f32", _conv_args(_P[4], need - 1), "workspace of %d bytes, %d needed" % (need - 1, need)),
        ("avt_conv3d_wgrad_x3_det_sub_f32", _conv_args(_P[4], 0), "workspace of 0 bytes"),
        # ... and what the atomic entry refuses, with its words
        ("avt_conv3d_wgrad_x3_det_sub_f32", _conv_args(_P[4], need, ptrs=(_P[0], None, _P[2])), "NULL pointer"),
        ("avt_conv3d_wgrad_x3_det_sub_f32", _conv_args(_P[4], need, ptrs=(_P[0], _P[1], _P[2] + 8)), "pointers must be 16-byte aligned"),
        ("avt_conv3d_wgrad_x3_det_sub_f32", _conv_args(_P[4], need, cin=6), "input channels in multiples of 4"),
        ("avt_conv3d_wgrad_x3_det_sub_f32", _conv_args(_P[4], need, kh=8, kw=8), "kernel taps"),
        ("avt_conv3d_wgrad_x3_det_sub_f32", _conv_args(_P[4], need, ldw=100), "ldw (100) < taps * cin (216)"),
        ("avt_stem_wgrad_x3_det", _stem_args(None, sneed), "workspace must be a 16-byte aligned device pointer"),
        ("avt_stem_wgrad_x3_det", _stem_args(_P[4] + 8, sneed), "workspace must be a 16-byte aligned device pointer"),
        ("avt_stem_wgrad_x3_det", _stem_args(_P[4], sneed - 16), "workspace of %d bytes, %d needed" % (sneed - 16, sneed)),
        ("avt_stem_wgrad_x3_det", _stem_args(_P[4], sneed, ptrs=(_P[0], _P[1], None, _P[3])), "NULL pointer"),
        ("avt_stem_wgrad_x3_det", _stem_args(_P[4], sneed, h=62), "unsupported shape"),
        ("avt_stem_wgrad_x3_det", _stem_args(_P[4], sneed, cout=16), "LDS"),
    ]
    for entry, args, words in cases:
        assert getattr(lib, entry)(*args) == AVT_ERR_ARG, (entry, words)
        assert words in lib.avt_last_error().decode(), (entry, words, lib.avt_last_error())
        with pytest.raises(avt._lib.AvtError) as e:
            getattr(checked, entry)(*args)
        assert words in str(e.value) and entry in str(e.value)
    assert before == [lib.avt_conv3d_wgrad_x3_det_launches(bn, s, b) for bn in (32, 64, 128) for s in (0, 1) for b in (0, 1)]
    assert sbefore == [lib.avt_stem_wgrad_x3_det_launches(kt, co) for kt in (1, 5) for co in (8, 16)]


def test_python_wrappers_refuse_host_tensors_and_the_fp32_mode(avt):
    from avtex import ops, train_ops

    with pytest.raises(avt._lib.AvtError):
        ops.conv3d_wgrad_x3_det_sub_f32(torch.zeros(4, 16), torch.zeros(4, 8), torch.zeros(16, 8), (1, 1, 2, 2), 8, 16, (1, 1, 1), (1, 1, 1),
                                        (0, 0, 0), (0, 0, 0), 8, 16, 8)
    assert train_ops.set_deterministic(False) is False and "wgrad_det" in train_ops.CALLS
    try:
        assert train_ops.set_deterministic(True) is False and train_ops.deterministic()
        with pytest.raises(avt._lib.AvtError, match="train_conv x3"):
            train_ops.set_conv_mode("fp32")
        assert train_ops.conv_mode() == "x3"
        assert train_ops.set_deterministic(False) is True
        train_ops.set_conv_mode("fp32")
        with pytest.raises(avt._lib.AvtError, match="train_conv x3"):
            train_ops.set_deterministic(True)
        assert not train_ops.deterministic()
    finally:
        train_ops.set_conv_mode("x3")
        train_ops.set_deterministic(False)
    from avtex.main import build_parser

    p = build_parser()
    assert p.parse_args([]).train_deterministic is False and p.parse_args(["--train_deterministic"]).train_deterministic is True
