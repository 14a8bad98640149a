// resample — band-limited sample-rate conversion on the device: resampy 0.4's windowed-sinc interpolation, which the reference
// reaches through resampy.resample (contrastive_video_textures/utils/vggish_utils.py:27-69) and librosa.load (validate.py:154,
// 172) with the filter "kaiser_best".  Built from the published algorithm; the filter table comes from the host
// (audio_frontend.sinc_filter), recomputed from the documented design.
//
// Every output is one sequential fp64 sum: the left wing's taps in ascending order, then the right wing's, each tap a linear
// interpolation of the table, win[o] + eta * delta[o], times one input sample.  One lane computes one output in exactly that
// order and the library is built with -ffp-contract=off, so the result is bit-identical to the host statement
// (audio_frontend.resample_sinc) — a sum split over lanes would be reordered.  inc, scale and step come from the host: the device
// derives none of them.  Neighbouring lanes read input samples `inc` apart and table entries inside one 512-entry span per
// tap, through the cache; the two 262 KB tables stay in L2.  Ten minutes at 48 kHz are 9.6 M outputs of at most 770 taps.
#include "avt_common.h"

namespace {

constexpr int kThreads = 256;  // (ops.RESAMPLE_BLOCK: the tests put n_out on both sides of it)

struct RArgs {
  const void* x;
  int64_t n_in;
  const double* win;
  const double* delta;
  int n_win, num_table, step;
  double scale, inc;
  void* y;
  int64_t n_out;
};

template <typename TX, typename TY>
__global__ __launch_bounds__(kThreads) void resample_sinc_kernel(RArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= a.n_out) return;
  const TX* __restrict__ x = static_cast<const TX*>(a.x);
  const double* __restrict__ win = a.win;
  const double* __restrict__ delta = a.delta;
  const double tr = (double)t * a.inc;  // the product, not a running sum
  const int64_t n = (int64_t)tr;        // < n_in: the launcher checks the last output's
  double frac = a.scale * (tr - (double)n);
  double acc = 0.0;
  {  // left wing: x[n], x[n-1], ...
    const double idx = frac * (double)a.num_table;
    const int off = (int)idx;
    const double eta = idx - (double)off;
    const int64_t taps = (a.n_win - off) / a.step, have = n + 1;
    const int64_t cnt = have < taps ? have : taps;
    const TX* xp = x + n;
    int o = off;
    for (int64_t i = 0; i < cnt; ++i, o += a.step) acc += (win[o] + eta * delta[o]) * (double)xp[-i];
  }
  frac = a.scale - frac;
  {  // right wing: x[n+1], x[n+2], ...
    const double idx = frac * (double)a.num_table;
    const int off = (int)idx;
    const double eta = idx - (double)off;
    const int64_t taps = (a.n_win - off) / a.step, have = a.n_in - n - 1;
    const int64_t cnt = have < taps ? have : taps;
    const TX* xp = x + n + 1;
    int o = off;
    for (int64_t k = 0; k < cnt; ++k, o += a.step) acc += (win[o] + eta * delta[o]) * (double)xp[k];
  }
  static_cast<TY*>(a.y)[t] = (TY)acc;  // float: round to nearest even, once
}

}  // namespace

extern "C" int avt_resample_sinc_f64(const void* x, int x_is_f64, int64_t n_in, const double* win, const double* delta,
                                     int n_win, int num_table, double scale, double time_increment, int index_step, void* y,
                                     int y_is_f64, int64_t n_out, void* stream) {
  AVT_REQUIRE(index_step >= 1 && n_win >= 1 && n_in >= 0 && n_out >= 0 && num_table >= 1,
              "avt_resample_sinc_f64: bad sizes (n_in=%lld n_out=%lld n_win=%d num_table=%d index_step=%d)", (long long)n_in,
              (long long)n_out, n_win, num_table, index_step);
  if (n_out == 0) return AVT_OK;
  AVT_REQUIRE(x && win && delta && y, "avt_resample_sinc_f64: NULL pointer");
  // 0 <= frac <= scale, so a wing's first table index is at most scale * num_table: it and every tap after it stay inside the table
  AVT_REQUIRE(scale > 0.0 && scale <= 1.0 && scale * (double)num_table < (double)n_win,
              "avt_resample_sinc_f64: scale=%g must be in (0, 1] with scale * num_table inside the table of %d", scale, n_win);
  // the device forms the same product for the last output: every output's centre sample int(t * inc) is then inside x
  AVT_REQUIRE(time_increment > 0.0 && (double)(n_out - 1) * time_increment < (double)n_in,
              "avt_resample_sinc_f64: output %lld lies past the %lld input samples at time_increment=%g", (long long)(n_out - 1),
              (long long)n_in, time_increment);
  const int64_t blocks = (n_out + kThreads - 1) / kThreads;
  AVT_REQUIRE(blocks < (1ll << 31), "avt_resample_sinc_f64: too many outputs");
  RArgs a;
  a.x = x;
  a.n_in = n_in;
  a.win = win;
  a.delta = delta;
  a.n_win = n_win;
  a.num_table = num_table;
  a.step = index_step;
  a.scale = scale;
  a.inc = time_increment;
  a.y = y;
  a.n_out = n_out;
  const dim3 grid((unsigned)blocks), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (x_is_f64 && y_is_f64) hipLaunchKernelGGL((resample_sinc_kernel<double, double>), grid, block, 0, s, a);
  else if (x_is_f64) hipLaunchKernelGGL((resample_sinc_kernel<double, float>), grid, block, 0, s, a);
  else if (y_is_f64) hipLaunchKernelGGL((resample_sinc_kernel<float, double>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((resample_sinc_kernel<float, float>), grid, block, 0, s, a);
  return avt::check_launch("avt_resample_sinc_f64");
}
