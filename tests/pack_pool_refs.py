"""Plain restatements of csrc/clip_pack.hip, csrc/split_planes.h and the head mean of csrc/pool.hip (test infrastructure,
never imported by the product, and calling nothing of the package): one numpy float32 operation per operation of the
kernel, in the kernel's order.  The library is built with -ffp-contract=off, so a kernel's arithmetic is what its source
says and these give its bits.  The max-pools need no restatement: F.max_pool2d on the joined fp32 values is exact.

Every array is float32 unless said otherwise; constants are np.float32 so that nothing is promoted."""
import numpy as np
import torch

BF16, F16 = 0, 1  # avt.h's plane_dtype (ops.X3_BF16, ops.X3_F16)
PLANE = {"bf16x3": BF16, "f16x3": F16}
FAST_T, SLOW_T = 32, 8
F32 = np.float32
_0, _1, _255 = F32(0.0), F32(1.0), F32(255.0)


# ---------------------------------------------------------------- clip packing (csrc/clip_pack.hip)
def src_scale(n_in, n_out):
    """The launcher's scale: (float)in / (float)out, one fp32 division."""
    return F32(n_in) / F32(n_out)


def src_index(scale_f32, n_out, n_in):
    """clip_pack.hip's src_index for dst = 0 .. n_out-1 -> (i0, i1 int64, l1 fp32).  s = fmaf(scale, dst + 0.5, -0.5) has ONE
    rounding: the product of a 24-bit and a <= 12-bit significand and its sum with -0.5 are exact in float64, so one cast
    to fp32 is the fused result."""
    scale = np.float64(F32(scale_f32))
    dst = np.arange(int(n_out), dtype=np.float64)
    s = (scale * (dst + 0.5) - 0.5).astype(F32)
    s = np.where(s < _0, _0, s).astype(F32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)  # (int)s truncates; s >= 0
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    return i0, i1, l1


def norm_lut(mean, std):
    """lut[v] = ((v / 255) - mean) / std, each step one fp32 rounding; mean and std rounded to fp32 once, as the C ABI
    receives them."""
    v = np.arange(256, dtype=F32)
    return ((v / _255) - F32(mean)) / F32(std)


def pack_plane(frame_u8, hw, mean, std):
    """uint8 [..., H, W] (one channel) -> fp32 [..., hw, hw]: normalise through the LUT, then the bilinear blend
    hy*(hx*p00 + lx*p01) + ly*(hx*p10 + lx*p11) in exactly that order, hx = 1 - lx, hy = 1 - ly."""
    f = np.asarray(frame_u8)
    assert f.dtype == np.uint8
    H, W = f.shape[-2], f.shape[-1]
    lut = norm_lut(mean, std)
    y0, y1, ly = src_index(src_scale(H, hw), hw, H)
    x0, x1, lx = src_index(src_scale(W, hw), hw, W)
    hy, hx = (_1 - ly)[:, None], (_1 - lx)[None, :]
    ly, lx = ly[:, None], lx[None, :]
    p00, p01 = lut[f[..., y0[:, None], x0[None, :]]], lut[f[..., y0[:, None], x1[None, :]]]
    p10, p11 = lut[f[..., y1[:, None], x0[None, :]]], lut[f[..., y1[:, None], x1[None, :]]]
    out = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11)
    assert out.dtype == F32
    return out


def sample_indices(win_len):
    """(fast[32], slow[8]) frame offsets inside a window: torch.linspace(..).long(), as oracle/ref_py.sample_indices."""
    fast = torch.linspace(0, win_len - 1, FAST_T).long()
    pick = torch.linspace(0, FAST_T - 1, SLOW_T).long()
    return fast.numpy(), fast[pick].numpy()


def pack_frames(frames_u8, hw, mean=0.45, std=0.225, bgr=True):
    """uint8 [F, H, W, 3] RGB -> fp32 [F, 3, hw, hw]: every frame packed once (output channel c reads source channel 2 - c
    when bgr)."""
    f = np.asarray(frames_u8.cpu() if isinstance(frames_u8, torch.Tensor) else frames_u8)
    f = np.ascontiguousarray(np.moveaxis(f, 3, 1))  # [F, 3, H, W]
    if bgr:
        f = np.ascontiguousarray(f[:, ::-1])
    return pack_plane(f, hw, mean, std)


def pack_clip(frames_u8, start, win_len, hw=224, mean=0.45, std=0.225, bgr=True, table=None):
    """uint8 [F, H, W, 3] RGB -> (slow [3, 8, hw, hw], fast [3, 32, hw, hw]) fp32 of the window [start, start + win_len).
    table: pack_frames(...) of the same arguments, to share among windows."""
    fast_idx, slow_idx = sample_indices(win_len)
    if table is None:
        f = np.asarray(frames_u8.cpu() if isinstance(frames_u8, torch.Tensor) else frames_u8)
        used = np.unique(start + fast_idx)
        packed = pack_frames(f[used], hw, mean, std, bgr)
        table = np.zeros((f.shape[0],) + packed.shape[1:], F32)
        table[used] = packed
    slow = np.ascontiguousarray(np.moveaxis(table[start + slow_idx], 0, 1))
    fast = np.ascontiguousarray(np.moveaxis(table[start + fast_idx], 0, 1))
    return slow, fast


# ---------------------------------------------------------------- the split-plane number format (csrc/split_planes.h)
def _rne_bf16(x):
    """fp32 -> bf16 words (uint16), round to nearest even on the integer bits; a NaN becomes the quiet NaN 0x7fc0."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r).astype(np.uint16)


def _bf16_f32(wd):
    return (np.ascontiguousarray(wd, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def plane_f32(wd, plane):
    """16-bit plane words (uint16) -> the fp32 values they hold."""
    wd = np.ascontiguousarray(wd, dtype=np.uint16)
    return wd.view(np.float16).astype(F32) if plane == F16 else _bf16_f32(wd)


def split(x, plane):
    """fp32 -> (hi, lo) plane words (uint16 arrays) as split2 does: hi = rne16(x), lo = rne16(x - hi).  fp16 planes clamp
    FINITE values to +-65504 first, and a value that is not finite (an infinity, a NaN) gets lo = 0, so an infinity stays
    that infinity and a NaN a NaN.  bf16 planes have no special cases (an infinity's lo is inf - inf = NaN)."""
    x = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        if plane == F16:
            fin = np.isfinite(x)
            v = np.where(fin, np.clip(x, F32(-65504.0), F32(65504.0)), x).astype(F32)
            hi = v.astype(np.float16)
            lo = np.where(fin, v - hi.astype(F32), _0).astype(F32).astype(np.float16)
            return hi.view(np.uint16), lo.view(np.uint16)
        hi = _rne_bf16(x)
        lo = _rne_bf16(x - _bf16_f32(hi))
        return hi, lo


def join(hi, lo, plane):
    """(hi, lo) plane words -> fp32(hi) + fp32(lo), one fp32 addition (exact for a pair that split made)."""
    with np.errstate(invalid="ignore"):
        return plane_f32(hi, plane) + plane_f32(lo, plane)


def words(t):
    """Raw 16-bit words (numpy uint16) of a plane tensor typed bfloat16 / float16."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def plane_tensor(wd):
    """uint16 plane words -> a CPU tensor typed bfloat16 holding those raw words (how the package passes planes around)."""
    return torch.from_numpy(np.ascontiguousarray(wd, dtype=np.uint16).view(np.int16).copy()).view(torch.bfloat16)


# ---------------------------------------------------------------- head mean (csrc/pool.hip: mean_positions kernels)
def sum_positions(rows_f32):
    """fp32 [P, C] -> the fp32 [C] sum in the kernel's order: row group g = 0..31 adds rows g, g + 32, ... one after the
    other (from 0), then s = (((0 + r0) + r1) + ... + r31)."""
    rows = np.ascontiguousarray(rows_f32, dtype=F32)
    P, C = rows.shape
    acc = np.zeros((32, C), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(P):
            acc[r % 32] = acc[r % 32] + rows[r]
        s = np.zeros(C, F32)
        for g in range(32):
            s = s + acc[g]
    return s


def mean_positions(rows_f32):
    """fp32 [P, C] -> fp32 [C]: sum_positions(rows) / fp32(P), one correctly rounded fp32 division."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (sum_positions(rows_f32) / F32(len(rows_f32))).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)
