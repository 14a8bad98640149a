// Every parameter's gradient, scaled, into ONE flat exchange buffer in ONE launch (include/avt.h avt_grad_pack_multi): the last node of
// a training step captured as a HIP graph on every rank (train_ops.GradExchange).  The ranks then all-reduce that one buffer outside the
// graph and the optimizer steps on views of it.  `scale` (1 / world: the all-reduce sums) is a LOAD from device memory, not an argument:
// a replay follows whatever the host last wrote there, as `hyper` does in csrc/sgd.hip.
//
// The pattern of sgd.hip and weight_planes_multi: a DEVICE table of jobs — one per gradient — and a block-to-job map; block b owns
// elements [(b - blk0) * 4096, + 4096) of its job's tensor.  HBM-bound: 8 B per element.  Lanes move 16 B each where src and dst are
// 16-byte aligned at the chunk; a gradient that is a view at an odd float offset takes dword accesses.  Vector stores only, no LDS, no
// atomics; nothing is written outside [dst, dst + numel).
//
// Arithmetic: dst[i] = src[i] * scale[0], one fp32 multiply, single rounding.
#include "avt_common.h"

namespace {

constexpr int kChunk = 4096;    // elements per block
constexpr int kThreads = 256;

struct PackJob {
  const float* src;
  float* dst;
  int64_t numel;
  int32_t blk0;        // the job's first block
  int32_t pad;
};
static_assert(sizeof(PackJob) == sizeof(AvtPackJob) && sizeof(PackJob) == 32, "AvtPackJob layout (include/avt.h)");

__global__ __launch_bounds__(kThreads) void grad_pack_multi_kernel(const PackJob* __restrict__ jobs, const int32_t* __restrict__ blk2job,
                                                                   const float* __restrict__ scale) {
  const PackJob j = jobs[blk2job[blockIdx.x]];
  const int64_t off = (int64_t)((int)blockIdx.x - j.blk0) * kChunk;
  const int64_t left = j.numel - off;
  if (left <= 0) return;
  const int n = left < kChunk ? (int)left : kChunk;  // this chunk: n <= kChunk elements
  const float s = scale[0];
  const float* __restrict__ src = j.src + off;
  float* __restrict__ dst = j.dst + off;
  const int t = (int)threadIdx.x;
  constexpr int R = kChunk / (4 * kThreads);  // float4 per lane
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
    const int n4 = n >> 2;
    float4 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = t + r * kThreads;
      if (i < n4) v[r] = reinterpret_cast<const float4*>(src)[i];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = t + r * kThreads;
      if (i < n4) reinterpret_cast<float4*>(dst)[i] = make_float4(v[r].x * s, v[r].y * s, v[r].z * s, v[r].w * s);
    }
    const int i = (n4 << 2) + t;  // the last chunk's tail: n % 4 elements
    if (t < (n & 3)) dst[i] = src[i] * s;
  } else {  // float-aligned (a view that starts off a 16-byte boundary): dword accesses, still coalesced
#pragma unroll 4
    for (int i = t; i < n; i += kThreads) dst[i] = src[i] * s;
  }
}

}  // namespace

extern "C" int avt_pack_job_bytes(void) { return (int)sizeof(PackJob); }

// jobs: DEVICE array of AvtPackJob, blk2job: DEVICE int32 [nblocks], scale: DEVICE fp32 [1]; the caller has validated the jobs
// (train_ops.GradExchange builds them from fp32 device tensors whose layout it checked against the views of its flat buffer)
extern "C" int avt_grad_pack_multi(const void* jobs, const int32_t* blk2job, int nblocks, const float* scale, void* stream) {
  AVT_REQUIRE(jobs && blk2job && scale && nblocks > 0, "avt_grad_pack_multi: NULL pointer / no blocks");
  AVT_REQUIRE(reinterpret_cast<uintptr_t>(jobs) % 8 == 0 && reinterpret_cast<uintptr_t>(scale) % 4 == 0,
              "avt_grad_pack_multi: the job table must be 8-byte aligned, scale 4-byte aligned");
  hipLaunchKernelGGL(grad_pack_multi_kernel, dim3((unsigned)nblocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const PackJob*>(jobs), blk2job, scale);
  return avt::check_launch("avt_grad_pack_multi");
}
