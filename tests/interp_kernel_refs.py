"""Plain fp32 restatements of the five passes of csrc/interp.hip (test infrastructure, never imported by the product): one
numpy float32 operation per operation of the kernel, in the kernel's order, so that a kernel whose arithmetic "follows the
reference's fp32 operation order" must give these bits.  Nothing here calls F.grid_sample, F.interpolate or F.avg_pool2d:
torch's fused CPU kernels associate differently (tests/test_interp_kernel_refs_host.py measures by how much) and serve as
a cross-check only.

Layouts are the kernels': images [2, H, W, 4] (frame, row, column, rgb + one zero lane), activations NHWC, flows as
channels (x, y).  Every array is float32 unless said otherwise; constants are np.float32 so that nothing is promoted."""
import numpy as np
import torch

BF16, F16 = 0, 1  # avt.h's plane_dtype (ops.X3_BF16, ops.X3_F16)
F32 = np.float32
_0, _H, _Q, _1, _2, _255 = F32(0.0), F32(0.5), F32(0.25), F32(1.0), F32(2.0), F32(255.0)


def _f32(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


# ---------------------------------------------------------------- the split-plane number format (csrc/split_planes.h)
def split(x, plane_dtype):
    """fp32 -> (hi, lo) planes as torch tensors typed bfloat16 (raw 16-bit words; fp16 planes are bit-cast), as split2 does:
    hi = rne16(x), lo = rne16(x - hi).  fp16 planes clamp FINITE values to +-65504 first and give a NaN / infinity lo = 0."""
    x = torch.from_numpy(_f32(x).copy())
    if plane_dtype == F16:
        fin = torch.isfinite(x)
        v = torch.where(fin, x.clamp(-65504.0, 65504.0), x)
        hi = v.to(torch.float16)
        lo = torch.where(fin, v - hi.float(), torch.zeros_like(v)).to(torch.float16)
    else:
        hi = x.to(torch.bfloat16)
        lo = (x - hi.float()).to(torch.bfloat16)
    return hi.view(torch.bfloat16).contiguous(), lo.view(torch.bfloat16).contiguous()


def join(hi, lo, plane_dtype):
    """(hi, lo) planes (typed bfloat16, raw words) -> the fp32 numpy array they stand for: fp32(hi) + fp32(lo), one rounding."""
    dt = torch.float16 if plane_dtype == F16 else torch.bfloat16
    return (hi.cpu().view(dt).float() + lo.cpu().view(dt).float()).numpy()


def words(t):
    """Raw 16-bit words of a plane tensor, for bit comparisons."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------- pack_pair
def pack_pair_ref(f0, f1, mean):
    """Two uint8 [H,W,3] frames -> img [2,H,W,4] = x / 255 - mean (fourth lane 0) and flowComp's rows [H,W,8] =
    (I0 rgb, I1 rgb, 0, 0).  The mean is rounded to fp32 once, as the C ABI receives it."""
    m = np.asarray([float(v) for v in mean], dtype=np.float32)
    h, w = f0.shape[0], f0.shape[1]
    img = np.zeros((2, h, w, 4), np.float32)
    for j, f in enumerate((f0, f1)):
        f = f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
        img[j, :, :, :3] = f.astype(np.float32) / _255 - m
    row = np.zeros((h, w, 8), np.float32)
    row[:, :, 0:3] = img[0, :, :, :3]
    row[:, :, 3:6] = img[1, :, :, :3]
    return img, row


# ---------------------------------------------------------------- avgpool2 / upsample2
def avgpool2_ref(x):
    """x [b,h,w,c], h and w even -> [b,h/2,w/2,c]: (((a + right) + below) + below-right) * 0.25"""
    x = _f32(x)
    a, r, d, e = x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]
    return (((a + r) + d) + e) * _Q


def up_src(n):
    """Source taps and weights of every output index 0..2n-1 along an axis of n (interp.hip `up_src`)."""
    d = np.arange(2 * n, dtype=np.float32)
    s = (d + _H) * _H - _H
    s = np.where(s < _0, _0, s).astype(np.float32)
    i0 = s.astype(np.int64)  # truncation; s >= 0
    i1 = i0 + (i0 < n - 1)
    l1 = s - i0.astype(np.float32)
    l0 = _1 - l1
    return i0, i1, l0, l1


def upsample2_ref(x):
    """x [b,h,w,c] -> [b,2h,2w,c]: ly0 (lx0 a + lx1 c) + ly1 (lx0 d + lx1 e)"""
    x = _f32(x)
    _, h, w, _ = x.shape
    y0, y1, ly0, ly1 = up_src(h)
    x0, x1, lx0, lx1 = up_src(w)
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    ly0, ly1 = ly0[None, :, None, None], ly1[None, :, None, None]
    a, c = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    d, e = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    return ly0 * (lx0 * a + lx1 * c) + ly1 * (lx0 * d + lx1 * e)


# ---------------------------------------------------------------- backwarp
def backwarp_ref(img, flow, masks=False):
    """img [H,W,C], flow [H,W,2] = (u, v) -> [H,W,C]: the sample of img at pixel + flow, bilinear with zero padding, by the
    arithmetic of interp.hip `backwarp`.  masks=True also returns (all four taps inside, at least one tap outside) per pixel."""
    img, flow = _f32(img), _f32(flow)
    H, W, _ = img.shape
    fw, fh = F32(W), F32(H)
    py, px = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = px + flow[:, :, 0], py + flow[:, :, 1]
        gx, gy = _2 * (x / fw - _H), _2 * (y / fh - _H)
        ix, iy = ((gx + _1) * fw - _1) / _2, ((gy + _1) * fh - _1) / _2
        fx, fy = np.floor(ix), np.floor(iy)
        wx1, wy1 = ix - fx, iy - fy
        wx0, wy0 = (fx + _1) - ix, (fy + _1) - iy
        nw, ne, sw, se = wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1
        okx0, okx1 = (fx >= _0) & (fx <= F32(W - 1)), (fx + _1 >= _0) & (fx + _1 <= F32(W - 1))
        oky0, oky1 = (fy >= _0) & (fy <= F32(H - 1)), (fy + _1 >= _0) & (fy + _1 <= F32(H - 1))
        x0 = np.where(okx0, fx, _0).astype(np.int64)
        x1 = np.where(okx1, fx + _1, _0).astype(np.int64)
        y0 = np.where(oky0, fy, _0).astype(np.int64)
        y1 = np.where(oky1, fy + _1, _0).astype(np.int64)

        def tap(ok, yy, xx):
            return np.where(ok[:, :, None], img[yy, xx], _0).astype(np.float32)

        ma, mb, mc, md = okx0 & oky0, okx1 & oky0, okx0 & oky1, okx1 & oky1
        a, b, c, d = tap(ma, y0, x0), tap(mb, y0, x1), tap(mc, y1, x0), tap(md, y1, x1)
        out = ((a * nw[:, :, None] + b * ne[:, :, None]) + c * sw[:, :, None]) + d * se[:, :, None]
    out = out.astype(np.float32)
    if masks:
        inside = ma & mb & mc & md
        return out, inside, ~inside
    return out


# ---------------------------------------------------------------- mid_input
def mid_coef(sf):
    """Per intermediate frame k = 1..sf-1: (-t(1-t), t^2, (1-t)^2, -t(1-t)) in Python doubles, rounded once to fp32."""
    out = np.zeros((sf - 1, 4), np.float32)
    for i in range(1, sf):
        t = float(i) / float(sf)
        temp = -t * (1.0 - t)
        out[i - 1] = (temp, t * t, (1.0 - t) * (1.0 - t), temp)
    return out


def mid_input_ref(img, flow4, sf, masks=False):
    """img [2,H,W,4], flow4 [H,W,4] = (F_0_1 x, y, F_1_0 x, y) -> ft [nt,H,W,4] = (t0x, t0y, t1x, t1y) and ArbTimeFlowIntrp's
    rows [nt,H,W,24] = (I0, I1, F_0_1, F_1_0, F_t_1, F_t_0, g1, g0, 0 x 4).  masks=True: also the tap masks of all 2 nt warps
    stacked, (inside, outside) [2 nt, H, W]."""
    img, f = _f32(img), _f32(flow4)
    _, H, W, _ = img.shape
    co = mid_coef(sf)
    nt = sf - 1
    ft = np.zeros((nt, H, W, 4), np.float32)
    row = np.zeros((nt, H, W, 24), np.float32)
    ins, outs = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(nt):
            c0, c1, c2, c3 = co[k]
            t0x, t0y = c0 * f[:, :, 0] + c1 * f[:, :, 2], c0 * f[:, :, 1] + c1 * f[:, :, 3]
            t1x, t1y = c2 * f[:, :, 0] + c3 * f[:, :, 2], c2 * f[:, :, 1] + c3 * f[:, :, 3]
            g0, i0, o0 = backwarp_ref(img[0, :, :, :3], np.stack((t0x, t0y), 2), masks=True)
            g1, i1, o1 = backwarp_ref(img[1, :, :, :3], np.stack((t1x, t1y), 2), masks=True)
            ins += [i0, i1]
            outs += [o0, o1]
            ft[k] = np.stack((t0x, t0y, t1x, t1y), 2)
            row[k, :, :, 0:3], row[k, :, :, 3:6] = img[0, :, :, :3], img[1, :, :, :3]
            row[k, :, :, 6:10] = f[:, :, :4]
            row[k, :, :, 10], row[k, :, :, 11], row[k, :, :, 12], row[k, :, :, 13] = t1x, t1y, t0x, t0y
            row[k, :, :, 14:17], row[k, :, :, 17:20] = g1, g0
    if masks:
        return ft, row, np.stack(ins), np.stack(outs)
    return ft, row


# ---------------------------------------------------------------- final
def fin_coef(sf):
    """(1 - t, t) per intermediate frame, from doubles."""
    t = [float(i) / float(sf) for i in range(1, sf)]
    return np.asarray([1.0 - v for v in t], np.float32), np.asarray(t, np.float32)


def final_ref(img, ft, o, sf, mean):
    """img [2,H,W,4], ft [nt,H,W,4], o [nt,H,W,>=5] = (dF_t_0 x, y, dF_t_1 x, y, visibility logit) -> (uint8 [nt,H,W,3], the
    fp32 value before truncation (r + mean) * 255).  Conversion: int() truncation, then & 255."""
    img, ft, o = _f32(img), _f32(ft), _f32(o)
    m = np.asarray([float(v) for v in mean], dtype=np.float32)
    w0, w1 = fin_coef(sf)
    pre = np.zeros(ft.shape[:3] + (3,), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(sf - 1):
            f0 = np.stack((o[k, :, :, 0] + ft[k, :, :, 0], o[k, :, :, 1] + ft[k, :, :, 1]), 2)
            f1 = np.stack((o[k, :, :, 2] + ft[k, :, :, 2], o[k, :, :, 3] + ft[k, :, :, 3]), 2)
            v0 = _1 / (_1 + np.exp(-o[k, :, :, 4]))
            v1 = _1 - v0
            g0, g1 = backwarp_ref(img[0, :, :, :3], f0), backwarp_ref(img[1, :, :, :3], f1)
            a0, a1 = (w0[k] * v0)[:, :, None], (w1[k] * v1)[:, :, None]
            r = (a0 * g0 + a1 * g1) / (a0 + a1)
            pre[k] = (r - (-m)) * _255
        u8 = (pre.astype(np.int64) & 255).astype(np.uint8)
    return u8, pre
