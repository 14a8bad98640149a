// wgrad_reduce — the second pass of the DETERMINISTIC weight gradients (include/avt.h): the weight-gradient tiles of
// wgrad_x3.hip and stem_train.hip have stored their partial filters to a workspace [nchunk][cout][E] (one slot per chunk of
// positions / per persistent workgroup, a function of the shapes alone), and
//     dW[co][e] = partial[0][co][e] + partial[1][co][e] + ... + partial[nchunk - 1][co][e]
// is summed here in ascending chunk order, one fp32 chain per element: the same bits on every run.  dW rows are ldw elements
// apart and only their first E columns are written (a frame-tap slice of a longer filter); dW is WRITTEN, never read.
// A thread owns four consecutive e of one row: a wave reads 1 KB runs of every chunk's plane (E is a multiple of 4 — taps x a
// multiple of 4 channels, or 32 per stem row), four independent chunk loads in flight per step.  HBM / L2 bound: the workspace
// has just been written by the launch in front of this one on the same stream.
#include "avt_common.h"
#include "wgrad_reduce.h"

namespace {

struct RdArgs {
  const float* ws;  // [nchunk][cout * E]
  float* dw;        // [cout][ldw]
  int nchunk, E, E4, ldw;  // E4 = E / 4
  int64_t plane;    // cout * E
  int64_t quads;    // cout * E / 4
};

// V: dW rows start 16-byte aligned (ldw % 4 == 0): one float4 store; otherwise four scalar stores
template <bool V>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(RdArgs a) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= a.quads) return;
  const float* p = a.ws + 4 * q;
  float4 s = *reinterpret_cast<const float4*>(p);
  int c = 1;
  for (; c + 4 <= a.nchunk; c += 4) {  // four loads in flight, added in ascending order
    const float4 v0 = *reinterpret_cast<const float4*>(p + (int64_t)c * a.plane);
    const float4 v1 = *reinterpret_cast<const float4*>(p + (int64_t)(c + 1) * a.plane);
    const float4 v2 = *reinterpret_cast<const float4*>(p + (int64_t)(c + 2) * a.plane);
    const float4 v3 = *reinterpret_cast<const float4*>(p + (int64_t)(c + 3) * a.plane);
    s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
    s.x += v1.x; s.y += v1.y; s.z += v1.z; s.w += v1.w;
    s.x += v2.x; s.y += v2.y; s.z += v2.z; s.w += v2.w;
    s.x += v3.x; s.y += v3.y; s.z += v3.z; s.w += v3.w;
  }
  for (; c < a.nchunk; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(p + (int64_t)c * a.plane);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const int64_t co = q / a.E4;
  const int e = 4 * (int)(q - co * a.E4);
  float* out = a.dw + co * a.ldw + e;
  if constexpr (V) {
    *reinterpret_cast<float4*>(out) = s;
  } else {
    out[0] = s.x; out[1] = s.y; out[2] = s.z; out[3] = s.w;
  }
}

}  // namespace

namespace avt {

int wgrad_reduce(const char* who, const float* ws, float* dw, int nchunk, int cout, int E, int ldw, hipStream_t st) {
  AVT_REQUIRE(ws && dw && nchunk >= 1 && cout >= 1 && E >= 4 && E % 4 == 0 && ldw >= E, "%s: bad reduction geometry", who);
  RdArgs a;
  a.ws = ws; a.dw = dw;
  a.nchunk = nchunk; a.E = E; a.E4 = E / 4; a.ldw = ldw;
  a.plane = (int64_t)cout * E;
  a.quads = a.plane / 4;
  const int64_t blocks = (a.quads + 255) / 256;
  AVT_REQUIRE(blocks < (1ll << 31), "%s: filter too large", who);
  if (ldw % 4 == 0) hipLaunchKernelGGL(wgrad_reduce_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(wgrad_reduce_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return check_launch(who);
}

}  // namespace avt
