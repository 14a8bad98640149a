// frame_table — the 3D-ResNet encoders' training input on the device, for gfx950.
// Replaces the host preprocessing of the reference's dataset for the non-SlowFast encoders
// (contrastive_video_textures/dataset/dataset.py:44-58: ToPILImage / Resize / ToTensor / Normalize, restated in
// avtex/dataset.py as /255, F.interpolate(bilinear, antialias=True), (x - mean) / std) and its per-item slicing (:145-209):
//
//   avt_frames_resize_aa_norm_u8   uint8 [F, H, W, 3] -> fp32 table [F, 3, hw, hw], once per video;
//   avt_clip_gather_frames_f32     out[n, t] = table[clamp(win_start[n] + t)], window starts read on the device.
//
// Resize: one workgroup per (frame, strip of AA_ROWS output rows, tile of <= 256 output columns).  Every source row the strip
// meets is read ONCE (dwords, coalesced), turned into v = u8 / 255 and laid out per channel in LDS; lane x filters it along x
// with its own normalised weights (a table in LDS, built once per workgroup) and adds the result, times the row's vertical
// weight, to the AA_ROWS x 3 sums it keeps in registers — the separable order of ATen's CPU kernel (x, then y, taps
// ascending).  Stores run along x.  Both kernels are HBM-bound.
#include <math.h>

#include "avt_common.h"

namespace {

constexpr int AA_ROWS = 8;            // output rows per workgroup
constexpr int AA_XT = 256;            // output columns per workgroup (one per lane)
constexpr int AA_LDS_BYTES = 65536;   // dynamic LDS a workgroup may ask for (include/avt.h states the limit this gives)

// ATen UpSampleKernel.cpp _compute_indices_min_size_weights_aa for the bilinear filter, with the C++ promotions of its
// float instantiation kept (the 0.5 literals are double): source range [xmin, xmin + xsize) of output index i.
struct AaRange {
  int xmin, xsize;
  float center, invscale;
};
__host__ __device__ inline AaRange aa_range(float scale, int i, int in_size, int max_taps) {
  AaRange r;
  const float support = scale >= 1.0f ? scale : 1.0f;
  r.center = (float)((double)scale * ((double)i + 0.5));
  r.invscale = scale >= 1.0f ? (float)(1.0 / (double)scale) : 1.0f;
  int lo = (int)((double)(r.center - support) + 0.5);
  int hi = (int)((double)(r.center + support) + 0.5);
  lo = lo < 0 ? 0 : lo;
  hi = hi > in_size ? in_size : hi;
  int n = hi - lo;
  n = n < 0 ? 0 : (n > max_taps ? max_taps : n);
  r.xmin = lo;
  r.xsize = n;
  return r;
}
// unnormalised triangle weight of tap j
__host__ __device__ inline float aa_weight(const AaRange& r, int j) {
  float x = (float)(((double)((float)(j + r.xmin) - r.center) + 0.5) * (double)r.invscale);
  x = x < 0.0f ? -x : x;
  return x < 1.0f ? (float)(1.0 - (double)x) : 0.0f;
}
inline int aa_max_taps(float scale) { return 2 * (int)ceilf(scale >= 1.0f ? scale : 1.0f) + 1; }

struct RArgs {
  const uint8_t* frames;
  float* out;
  int n_frames, H, W, hw;
  float scale_h, scale_w;
  float mean[3], std[3];
  int kx, ky;     // tap bounds per axis (2 ceil(support) + 1: odd, so lane-strided rows of the weight table spread over the banks)
  int n_xt;       // column tiles
  int n_strips;   // row strips
  int span_max;   // source pixels a column tile can meet (row buffer: 3 channels of this many floats)
  int nblk;
};

__global__ __launch_bounds__(AA_XT) void resize_aa_norm_kernel(RArgs a) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ float lut[256];
  __shared__ float s_wy[AA_ROWS];
  __shared__ float s_ytot[AA_ROWS], s_yc[AA_ROWS];
  __shared__ int s_ymin[AA_ROWS], s_ysz[AA_ROWS];
  float* wx = dyn;                              // [blockDim.x][kx]
  float* row = dyn + (int)blockDim.x * a.kx;    // [3][span_max]

  const int tid = threadIdx.x, nthr = blockDim.x;
  int b = avt::xcd_contiguous(blockIdx.x, a.nblk);
  const int strip = b % a.n_strips;
  b /= a.n_strips;
  const int xt = b % a.n_xt;
  const int f = b / a.n_xt;
  const int x0 = xt * AA_XT;
  const int nx = a.hw - x0 < AA_XT ? a.hw - x0 : AA_XT;  // columns of this tile
  const int y0 = strip * AA_ROWS;
  const int ny = a.hw - y0 < AA_ROWS ? a.hw - y0 : AA_ROWS;

  for (int t = tid; t < 256; t += nthr) lut[t] = __fdiv_rn((float)t, 255.0f);  // v = u8 / 255 comes first (dataset.py)
  // source span of the tile (the ranges are monotone in x) and this lane's weights, normalised by their sum as ATen does
  const AaRange first = aa_range(a.scale_w, x0, a.W, a.kx);
  const AaRange last = aa_range(a.scale_w, x0 + nx - 1, a.W, a.kx);
  const int s0 = first.xmin;
  int span = last.xmin + last.xsize - s0;
  span = span > a.span_max ? a.span_max : span;
  int xoff = 0, xsize = 0;
  if (tid < nx) {
    const AaRange r = aa_range(a.scale_w, x0 + tid, a.W, a.kx);
    xoff = r.xmin - s0;
    xsize = r.xsize;
    if (xoff + xsize > span) xsize = span - xoff > 0 ? span - xoff : 0;  // (cannot happen: the buffer's bound, not the filter's)
    float tot = 0.0f;
    for (int j = 0; j < xsize; ++j) tot += aa_weight(r, j);
    for (int j = 0; j < xsize; ++j) {
      const float w = aa_weight(r, j);
      wx[tid * a.kx + j] = tot != 0.0f ? __fdiv_rn(w, tot) : w;
    }
  }
  if (tid < AA_ROWS) {
    int ymin = 0, ysz = 0;
    float tot = 0.0f, yc = 0.0f;
    if (tid < ny) {
      const AaRange r = aa_range(a.scale_h, y0 + tid, a.H, a.ky);
      ymin = r.xmin;
      ysz = r.xsize;
      yc = r.center;
      for (int j = 0; j < ysz; ++j) tot += aa_weight(r, j);
    }
    s_ymin[tid] = ymin;
    s_ysz[tid] = ysz;
    s_ytot[tid] = tot;
    s_yc[tid] = yc;
  }
  const AaRange rfirst = aa_range(a.scale_h, y0, a.H, a.ky);
  const AaRange rlast = aa_range(a.scale_h, y0 + ny - 1, a.H, a.ky);
  const int r0 = rfirst.xmin, r1 = rlast.xmin + rlast.xsize;
  const float inv_h = rfirst.invscale;

  float acc[AA_ROWS][3];
#pragma unroll
  for (int i = 0; i < AA_ROWS; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.0f;

  const int nbytes = span * 3;
  const uint8_t* src = a.frames + (((int64_t)f * a.H + r0) * a.W + s0) * 3;
  const int pitch = a.W * 3;
  const float* wrow = wx + tid * a.kx;
  const float* pix = row + xoff;
  const int sm = a.span_max;
  __syncthreads();
  for (int r = r0; r < r1; ++r, src += pitch) {
    // stage the row: head bytes up to the first 4-byte boundary, whole dwords, tail bytes; byte e is channel e % 3 of pixel e / 3
    const int head0 = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(src) & 3u)) & 3u);
    const int head = head0 < nbytes ? head0 : nbytes;
    const int ndw = (nbytes - head) >> 2;
    const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src + head);
    for (int k = tid; k < ndw; k += nthr) {
      const uint32_t v = src4[k];
      const int e = head + 4 * k;
      int p = e / 3, c = e - p * 3;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        row[c * sm + p] = lut[(v >> (8 * q)) & 0xffu];
        if (++c == 3) {
          c = 0;
          ++p;
        }
      }
    }
    const int tail0 = head + 4 * ndw;
    const int nedge = head + (nbytes - tail0);  // <= 6 bytes outside the dwords
    if (tid < nedge) {
      const int e = tid < head ? tid : tail0 + (tid - head);
      const int p = e / 3, c = e - p * 3;
      row[c * sm + p] = lut[src[e]];
    }
    if (tid < AA_ROWS) {  // this source row's normalised vertical weight for each output row of the strip
      const int j = r - s_ymin[tid];
      float w = 0.0f;
      if (j >= 0 && j < s_ysz[tid]) {
        AaRange ry;
        ry.xmin = s_ymin[tid];
        ry.xsize = s_ysz[tid];
        ry.center = s_yc[tid];
        ry.invscale = inv_h;
        w = aa_weight(ry, j);
        if (s_ytot[tid] != 0.0f) w = __fdiv_rn(w, s_ytot[tid]);
      }
      s_wy[tid] = w;
    }
    __syncthreads();
    float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
    for (int j = 0; j < xsize; ++j) {
      const float w = wrow[j];
      h0 = __fmaf_rn(w, pix[j], h0);
      h1 = __fmaf_rn(w, pix[sm + j], h1);
      h2 = __fmaf_rn(w, pix[2 * sm + j], h2);
    }
#pragma unroll
    for (int i = 0; i < AA_ROWS; ++i) {
      const float w = s_wy[i];
      acc[i][0] = __fmaf_rn(w, h0, acc[i][0]);
      acc[i][1] = __fmaf_rn(w, h1, acc[i][1]);
      acc[i][2] = __fmaf_rn(w, h2, acc[i][2]);
    }
    __syncthreads();
  }
  if (tid >= nx) return;
  const int plane = a.hw * a.hw;
  float* dst = a.out + (int64_t)f * 3 * plane + y0 * a.hw + x0 + tid;
#pragma unroll
  for (int i = 0; i < AA_ROWS; ++i) {
    if (i < ny) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[c * plane + i * a.hw] = __fdiv_rn(__fsub_rn(acc[i][c], a.mean[c]), a.std[c]);
    }
  }
}

// H == W == hw: no filter (dataset.py skips F.interpolate), out = (u8 / 255 - mean_c) / std_c through one table per channel.
struct NArgs {
  const uint8_t* frames;
  float* out;
  int plane;  // hw * hw
  int bpf;    // workgroups per frame
  float mean[3], std[3];
};

__global__ __launch_bounds__(256) void norm_planes_kernel(NArgs a) {
  __shared__ float lut[3][256];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    lut[c][threadIdx.x] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)threadIdx.x, 255.0f), a.mean[c]), a.std[c]);
  __syncthreads();
  const int f = blockIdx.x / a.bpf;
  const int p = (blockIdx.x - f * a.bpf) * 256 + threadIdx.x;
  if (p >= a.plane) return;
  const uint8_t* src = a.frames + (int64_t)f * a.plane * 3 + p * 3;
  float* dst = a.out + (int64_t)f * a.plane * 3 + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c * a.plane] = lut[c][src[c]];
}

// ---- window gather ---------------------------------------------------------------------------------------------------
struct alignas(16) f32x4_a {  // 16-byte aligned lanes
  float v[4];
};
struct f32x4_u {  // the same 16 bytes at float alignment: frames of 3 hw^2 = 3 (mod 4) floats start anywhere
  float v[4];
};

constexpr int G_LANES = 4;                    // 16-byte lanes per thread
constexpr int G_CHUNK = 256 * G_LANES * 4;    // floats per workgroup

struct FArgs {
  const float* table;
  const int32_t* win_start;
  float* out;
  int n_frames, win_len;
  int fs;      // floats per frame, 3 hw^2
  int chunks;  // workgroups per frame
};

template <typename V>
__global__ __launch_bounds__(256) void clip_gather_frames_kernel(FArgs a) {
  const int slot = blockIdx.x / a.chunks;  // n * win_len + t
  const int chunk = blockIdx.x - slot * a.chunks;
  const int n = slot / a.win_len, t = slot - n * a.win_len;
  int f = a.win_start[n] + t;
  f = f < 0 ? 0 : (f > a.n_frames - 1 ? a.n_frames - 1 : f);  // a bad start cannot fault (range of the ids: checked once by dataset.DeviceSegmentBatcher)
  const float* __restrict__ src = a.table + (int64_t)f * a.fs;
  float* __restrict__ dst = a.out + (int64_t)slot * a.fs;
  const int nq = a.fs >> 2;
  const int q0 = chunk * (G_CHUNK / 4) + threadIdx.x;
  if (q0 + (G_LANES - 1) * 256 < nq) {  // a whole chunk: every load in flight before the first store
    V v[G_LANES];
#pragma unroll
    for (int i = 0; i < G_LANES; ++i) v[i] = reinterpret_cast<const V*>(src)[q0 + i * 256];
#pragma unroll
    for (int i = 0; i < G_LANES; ++i) reinterpret_cast<V*>(dst)[q0 + i * 256] = v[i];
  } else {
#pragma unroll
    for (int i = 0; i < G_LANES; ++i) {
      const int q = q0 + i * 256;
      if (q < nq) reinterpret_cast<V*>(dst)[q] = reinterpret_cast<const V*>(src)[q];
    }
  }
  if (chunk == a.chunks - 1) {  // scalar tail: fs % 4 floats
    const int e = (nq << 2) + threadIdx.x;
    if (e < a.fs) dst[e] = src[e];
  }
}

}  // namespace

extern "C" int avt_frames_resize_aa_norm_u8(const uint8_t* frames, int n_frames, int height, int width, int out_hw,
                                            const float* mean, const float* std, float* out, void* stream) {
  AVT_REQUIRE(n_frames >= 0 && height > 0 && width > 0 && out_hw > 0, "avt_frames_resize_aa_norm_u8: bad sizes");
  if (n_frames == 0) return AVT_OK;
  AVT_REQUIRE(frames && out && mean && std, "avt_frames_resize_aa_norm_u8: NULL pointer");
  AVT_REQUIRE(std[0] != 0.0f && std[1] != 0.0f && std[2] != 0.0f, "avt_frames_resize_aa_norm_u8: std == 0");
  AVT_REQUIRE(out_hw <= 8192 && (int64_t)height * width * 3 < (1ll << 31),
              "avt_frames_resize_aa_norm_u8: out_hw > 8192 or a source frame of 2^31 bytes");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (height == out_hw && width == out_hw) {
    NArgs n;
    n.frames = frames;
    n.out = out;
    n.plane = out_hw * out_hw;
    n.bpf = (n.plane + 255) / 256;
    for (int c = 0; c < 3; ++c) n.mean[c] = mean[c], n.std[c] = std[c];
    const int64_t nblk = (int64_t)n.bpf * n_frames;
    AVT_REQUIRE(nblk < (1ll << 31), "avt_frames_resize_aa_norm_u8: grid too large");
    hipLaunchKernelGGL(norm_planes_kernel, dim3((unsigned)nblk), dim3(256), 0, st, n);
    return avt::check_launch("avt_frames_resize_aa_norm_u8");
  }
  RArgs a;
  a.frames = frames;
  a.out = out;
  a.n_frames = n_frames;
  a.H = height;
  a.W = width;
  a.hw = out_hw;
  a.scale_h = (float)height / (float)out_hw;  // ATen area_pixel_compute_scale<float>, align_corners = False, no scale_factor
  a.scale_w = (float)width / (float)out_hw;
  for (int c = 0; c < 3; ++c) a.mean[c] = mean[c], a.std[c] = std[c];
  a.kx = aa_max_taps(a.scale_w);
  a.ky = aa_max_taps(a.scale_h);
  a.n_xt = (out_hw + AA_XT - 1) / AA_XT;
  a.n_strips = (out_hw + AA_ROWS - 1) / AA_ROWS;
  a.span_max = 1;
  for (int t = 0; t < a.n_xt; ++t) {
    const int xa = t * AA_XT, xb = (xa + AA_XT < out_hw ? xa + AA_XT : out_hw) - 1;
    const AaRange lo = aa_range(a.scale_w, xa, width, a.kx), hi = aa_range(a.scale_w, xb, width, a.kx);
    const int span = hi.xmin + hi.xsize - lo.xmin;
    if (span > a.span_max) a.span_max = span;
  }
  const int threads = out_hw >= AA_XT ? AA_XT : (out_hw + 63) / 64 * 64;
  const int64_t lds = ((int64_t)threads * a.kx + 3ll * a.span_max) * (int64_t)sizeof(float);
  AVT_REQUIRE(lds <= AA_LDS_BYTES,
              "avt_frames_resize_aa_norm_u8: %d x %d -> %d needs %lld bytes of LDS for its %d-tap weight table and row buffer, the "
              "limit is %d", height, width, out_hw, (long long)lds, a.kx, AA_LDS_BYTES);
  const int64_t nblk = (int64_t)a.n_strips * a.n_xt * n_frames;
  AVT_REQUIRE(nblk < (1ll << 31), "avt_frames_resize_aa_norm_u8: grid too large");
  a.nblk = (int)nblk;
  hipLaunchKernelGGL(resize_aa_norm_kernel, dim3((unsigned)nblk), dim3(threads), (size_t)lds, st, a);
  return avt::check_launch("avt_frames_resize_aa_norm_u8");
}

extern "C" int avt_clip_gather_frames_f32(const float* table, int n_frames, int out_hw, const int32_t* win_start, int n_win,
                                          int win_len, float* out, void* stream) {
  AVT_REQUIRE(n_frames > 0 && out_hw > 0 && n_win >= 0 && win_len > 0, "avt_clip_gather_frames_f32: bad sizes");
  if (n_win == 0) return AVT_OK;
  AVT_REQUIRE(table && win_start && out, "avt_clip_gather_frames_f32: NULL pointer");
  AVT_REQUIRE(out_hw <= 8192, "avt_clip_gather_frames_f32: out_hw > 8192");  // 3 hw^2 and every in-frame offset fit 31 bits
  AVT_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
              "avt_clip_gather_frames_f32: table / out are not float-aligned");
  FArgs a;
  a.table = table;
  a.win_start = win_start;
  a.out = out;
  a.n_frames = n_frames;
  a.win_len = win_len;
  a.fs = 3 * out_hw * out_hw;
  a.chunks = (a.fs + G_CHUNK - 1) / G_CHUNK;
  // frame bases are 64-bit in the kernel (the table and the output may both pass 2^31 elements); what has to fit 31 bits is the grid
  const int64_t nblk = (int64_t)n_win * win_len * a.chunks;
  AVT_REQUIRE(nblk < (1ll << 31), "avt_clip_gather_frames_f32: %d windows of %d frames need %lld workgroups (limit 2^31 - 1)",
              n_win, win_len, (long long)nblk);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool al = a.fs % 4 == 0 && avt::aligned16(table) && avt::aligned16(out);
  if (al)
    hipLaunchKernelGGL(clip_gather_frames_kernel<f32x4_a>, dim3((unsigned)nblk), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(clip_gather_frames_kernel<f32x4_u>, dim3((unsigned)nblk), dim3(256), 0, st, a);
  return avt::check_launch("avt_clip_gather_frames_f32");
}
