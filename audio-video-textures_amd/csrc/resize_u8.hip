// resize_u8 — Pillow's `Image.resize` for 8-bit RGB on the device, bit for bit: the Lanczos resize that takes the two frames
// of a jump to the networks' size (a multiple of 32) and the bilinear resize that takes the SF - 1 interpolated frames back
// (contrastive_video_textures/interpolate.py:43, 137; called from slowmo.Interpolator).  Pillow's 8-bit resampler is integer
// arithmetic over fixed-point coefficient tables, so the device result is equal, not close:
//   tables (HOST)  per output sample the first input sample, the tap count and the normalised filter weights, computed in
//                  double with libm's sin and rounded to 22 fractional bits, exactly as Pillow's precompute_coeffs /
//                  normalize_coeffs_8bpc do
//   a pass         out = clamp((2^21 + sum_t k[t] * in[first + t]) >> 22, 0, 255) in int32, arithmetic shift
//   order          horizontal into a uint8 intermediate (its rounding is part of the result), then vertical; a pass whose
//                  extent does not change is skipped
// Both passes are memory-bound with a handful of taps per output.  The vertical pass is a flat byte-row problem (W * 3 bytes
// per row, one set of taps for the whole row): 16 bytes per lane per tap.  Row starts are not aligned when W * 3 is odd, so
// the wide accesses go through memcpy — the compiler picks the instruction (unaligned dwordx4 on gfx950) and the row's tail
// is done byte by byte.  The horizontal pass gathers up to ksize neighbouring pixels per output pixel, one lane per pixel.
#include <math.h>
#include <string.h>

#include "avt_common.h"

namespace {

constexpr int kBits = 22;  // Pillow's PRECISION_BITS = 32 - 8 - 2: room for the filter's overshoot in int32
constexpr int kT = 128;
constexpr int kChunk = 16;  // bytes per lane in the vertical pass
constexpr int kMaxExtent = 1 << 20;

double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
double lanczos_filter(double x) { return -3.0 <= x && x < 3.0 ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }

struct Axis {
  double scale, fscale, support;
  int ksize;
};
Axis axis_of(int in_size, int out_size, int filter) {
  Axis a;
  a.scale = (double)in_size / out_size;
  a.fscale = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = (filter == AVT_RESIZE_LANCZOS ? 3.0 : 1.0) * a.fscale;
  const double c = ceil(a.support);
  a.ksize = c < (double)(1 << 20) ? (int)c * 2 + 1 : 0;
  return a;
}

__device__ __forceinline__ uint32_t clip8(int acc) { return (uint32_t)min(max(acc >> kBits, 0), 255); }

// one block row = one output row (b, y): its bounds and taps are block-uniform; a lane owns 16 bytes of the row
__global__ __launch_bounds__(kT) void vertical_kernel(const uint8_t* __restrict__ in, int h_in, int h_out, unsigned row_bytes,
                                                      const int32_t* __restrict__ k, const int32_t* __restrict__ bounds, int ksize,
                                                      uint8_t* __restrict__ out) {
  const unsigned r = blockIdx.x, b = r / (unsigned)h_out, y = r - b * (unsigned)h_out;
  const unsigned c0 = (blockIdx.y * kT + threadIdx.x) * kChunk;
  if (c0 >= row_bytes) return;
  const int first = bounds[2 * y], n = bounds[2 * y + 1];
  const int32_t* kr = k + (size_t)y * ksize;
  const uint8_t* src = in + ((size_t)b * h_in + first) * row_bytes + c0;
  uint8_t* dst = out + (size_t)r * row_bytes + c0;
  if (c0 + kChunk <= row_bytes) {
    int acc[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) acc[j] = 1 << (kBits - 1);
    for (int t = 0; t < n; ++t) {
      uint32_t v[kChunk / 4];
      __builtin_memcpy(v, src + (size_t)t * row_bytes, kChunk);
      const int kt = kr[t];
#pragma unroll
      for (int j = 0; j < kChunk; ++j) acc[j] += kt * (int)((v[j / 4] >> (8 * (j % 4))) & 255u);
    }
    uint32_t o[kChunk / 4];
#pragma unroll
    for (int q = 0; q < kChunk / 4; ++q)
      o[q] = clip8(acc[4 * q]) | clip8(acc[4 * q + 1]) << 8 | clip8(acc[4 * q + 2]) << 16 | clip8(acc[4 * q + 3]) << 24;
    __builtin_memcpy(dst, o, kChunk);
  } else {  // the row's tail: fewer than 16 bytes
    for (unsigned j = 0; j < row_bytes - c0; ++j) {
      int acc = 1 << (kBits - 1);
      for (int t = 0; t < n; ++t) acc += kr[t] * (int)src[(size_t)t * row_bytes + j];
      dst[j] = (uint8_t)clip8(acc);
    }
  }
}

// one block row = one image row (b, y); a lane owns one output pixel and reads its n neighbouring input pixels
__global__ __launch_bounds__(kT) void horizontal_kernel(const uint8_t* __restrict__ in, int w_in, int w_out,
                                                        const int32_t* __restrict__ k, const int32_t* __restrict__ bounds, int ksize,
                                                        uint8_t* __restrict__ out) {
  const unsigned x = blockIdx.y * kT + threadIdx.x;
  if (x >= (unsigned)w_out) return;
  const int first = bounds[2 * x], n = bounds[2 * x + 1];
  const int32_t* kr = k + (size_t)x * ksize;
  const uint8_t* src = in + ((size_t)blockIdx.x * w_in + first) * 3;
  int a0 = 1 << (kBits - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < n; ++t) {
    const int kt = kr[t];
    a0 += kt * (int)src[3 * t];
    a1 += kt * (int)src[3 * t + 1];
    a2 += kt * (int)src[3 * t + 2];
  }
  uint8_t* dst = out + ((size_t)blockIdx.x * w_out + x) * 3;
  dst[0] = (uint8_t)clip8(a0);
  dst[1] = (uint8_t)clip8(a1);
  dst[2] = (uint8_t)clip8(a2);
}

}  // namespace

extern "C" int avt_resize_u8_ksize(int in_size, int out_size, int filter) {
  AVT_REQUIRE(in_size > 0 && out_size > 0 && in_size <= kMaxExtent && out_size <= kMaxExtent,
              "avt_resize_u8_ksize: extents must be in 1..2^20 (got %d -> %d)", in_size, out_size);
  AVT_REQUIRE(filter == AVT_RESIZE_BILINEAR || filter == AVT_RESIZE_LANCZOS, "avt_resize_u8_ksize: filter must be 0 (bilinear) or 1 (Lanczos)");
  const Axis a = axis_of(in_size, out_size, filter);
  AVT_REQUIRE(a.ksize > 0, "avt_resize_u8_ksize: %d -> %d needs too many taps", in_size, out_size);
  return a.ksize;
}

extern "C" int avt_resize_u8_tables(int in_size, int out_size, int filter, int ksize, int32_t* k, int32_t* bounds) {
  AVT_REQUIRE(k && bounds, "avt_resize_u8_tables: NULL pointer");
  const int want = avt_resize_u8_ksize(in_size, out_size, filter);
  if (want < 0) return want;
  AVT_REQUIRE(ksize == want, "avt_resize_u8_tables: %d -> %d has %d taps, the buffers are for %d", in_size, out_size, want, ksize);
  const Axis a = axis_of(in_size, out_size, filter);
  double (*f)(double) = filter == AVT_RESIZE_LANCZOS ? lanczos_filter : bilinear_filter;
  const double ss = 1.0 / a.fscale;
  double* w = static_cast<double*>(malloc(sizeof(double) * ksize));
  AVT_REQUIRE(w, "avt_resize_u8_tables: out of memory");
  for (int i = 0; i < out_size; ++i) {
    const double center = (i + 0.5) * a.scale;
    int first = (int)(center - a.support + 0.5);
    if (first < 0) first = 0;
    int last = (int)(center + a.support + 0.5);
    if (last > in_size) last = in_size;
    const int n = last - first;  // <= ksize: the two roundings span at most 2 * support + 1
    double sum = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = f((x + first - center + 0.5) * ss);
      sum += w[x];
    }
    int32_t* kr = k + (size_t)i * ksize;
    for (int x = 0; x < ksize; ++x) {
      double v = x < n ? w[x] : 0.0;
      if (x < n && sum != 0.0) v /= sum;
      kr[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << kBits)) : (int32_t)(0.5 + v * (1 << kBits));
    }
    bounds[2 * i] = first;
    bounds[2 * i + 1] = n;
  }
  free(w);
  return AVT_OK;
}

extern "C" int avt_resize_u8(const uint8_t* in, uint8_t* tmp, uint8_t* out, int batch, int in_h, int in_w, int out_h, int out_w,
                             int channels, const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by,
                             int ksize_y, void* stream) {
  AVT_REQUIRE(channels == 3, "avt_resize_u8: 3 channels (RGB) only, got %d", channels);
  AVT_REQUIRE(batch > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0 && in_h <= kMaxExtent && in_w <= kMaxExtent && out_h <= kMaxExtent &&
                  out_w <= kMaxExtent,
              "avt_resize_u8: batch must be positive and extents in 1..2^20 (got %d x %d x %d -> %d x %d)", batch, in_h, in_w, out_h, out_w);
  const bool horiz = out_w != in_w, vert = out_h != in_h;
  AVT_REQUIRE(in && out && in != out, "avt_resize_u8: NULL pointer / in-place");
  AVT_REQUIRE(!horiz || (kx && bx && ksize_x > 0), "avt_resize_u8: the horizontal pass needs its tables");
  AVT_REQUIRE(!vert || (ky && by && ksize_y > 0), "avt_resize_u8: the vertical pass needs its tables");
  AVT_REQUIRE(!(horiz && vert) || (tmp && tmp != in && tmp != out), "avt_resize_u8: two passes need an intermediate of batch * in_h * out_w * 3 bytes");
  const int64_t lim = 1ll << 31;
  const int64_t wmax = in_w > out_w ? in_w : out_w, hmax = in_h > out_h ? in_h : out_h;
  AVT_REQUIRE((int64_t)batch * hmax * wmax * 3 < lim, "avt_resize_u8: tensor too large for 32-bit byte offsets");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!horiz && !vert) {
    const hipError_t e = hipMemcpyAsync(out, in, (size_t)batch * in_h * in_w * 3, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      avt::set_error("avt_resize_u8: hipMemcpyAsync: %s", hipGetErrorString(e));
      return AVT_ERR_LAUNCH;
    }
    return AVT_OK;
  }
  const uint8_t* src = in;
  if (horiz) {
    uint8_t* dst = vert ? tmp : out;
    hipLaunchKernelGGL(horizontal_kernel, dim3(batch * in_h, (out_w + kT - 1) / kT), dim3(kT), 0, st, src, in_w, out_w, kx, bx, ksize_x, dst);
    const int rc = avt::check_launch("avt_resize_u8 (horizontal)");
    if (rc != AVT_OK) return rc;
    src = dst;
  }
  if (vert) {
    const unsigned row_bytes = (unsigned)out_w * 3, chunks = (row_bytes + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(vertical_kernel, dim3(batch * out_h, (chunks + kT - 1) / kT), dim3(kT), 0, st, src, in_h, out_h, row_bytes, ky, by,
                       ksize_y, out);
    return avt::check_launch("avt_resize_u8 (vertical)");
  }
  return AVT_OK;
}
