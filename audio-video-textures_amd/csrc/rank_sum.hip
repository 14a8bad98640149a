// rank_sum — the sum over the ranks of the ORDERED gradient exchange (include/avt.h avt_rank_sum_f32; train_ops.GradExchange with
// ordered=True): an all-gather has put rank r's packed gradients into row r of parts [world][ld], and
//     out[i] = parts[0][i] + parts[1][i] + ... + parts[world - 1][i]
// is summed here in ascending rank order, one fp32 chain per element, every add rounded on its own (the library is built with
// -ffp-contract=off and without fast-math: nothing is reassociated) — the same bits on every rank and on every run, which the
// backend's all-reduce does not promise.  world == 1 is a copy (no add: -0.0 and NaN payloads pass through).
// The pattern of wgrad_reduce.hip on a flat vector: a thread owns four consecutive floats (one 16-byte lane, 64-bit offsets), a wave
// reads 1 KB runs of every row, and the loads of four rows are issued before the first add of the group.  The n % 4 tail is owned by up
// to three more threads, one float each, through dword accesses: nothing outside [out, out + n) is written.  HBM bound:
// (world + 1) * n * 4 bytes.  No LDS, no atomics; the row loop is a run-time loop (world is not a template argument).
#include "avt_common.h"

namespace {

constexpr int kThreads = 256;
typedef float f32x4 __attribute__((ext_vector_type(4)));
// device memory, said so: global_load / global_store instead of flat accesses
#define AVT_GLOBAL __attribute__((address_space(1)))

// V = f32x4 (a 16-byte lane) or float (a tail element); p = the lane in row 0, ld = the row stride in units of V
template <typename V>
__device__ __forceinline__ V rank_chain(const V AVT_GLOBAL* __restrict__ p, int world, int64_t ld) {
  V s = p[0];
  int r = 1;
  if (world >= 4) {  // the first group is rows 0..3: s is its first load
    const V v1 = p[ld], v2 = p[2 * ld], v3 = p[3 * ld];
    s += v1; s += v2; s += v3;
    r = 4;
  }
  for (; r + 4 <= world; r += 4) {  // four loads in flight, added in ascending order
    const V v0 = p[r * ld], v1 = p[(r + 1) * ld], v2 = p[(r + 2) * ld], v3 = p[(r + 3) * ld];
    s += v0; s += v1; s += v2; s += v3;
  }
  for (; r < world; ++r) s += p[r * ld];
  return s;
}

__global__ __launch_bounds__(kThreads) void rank_sum_kernel(const float* __restrict__ parts, float* __restrict__ out, int world,
                                                            int64_t n, int64_t ld) {
  const int64_t quads = n >> 2;
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q < quads) {
    ((f32x4 AVT_GLOBAL*)out)[q] = rank_chain((const f32x4 AVT_GLOBAL*)parts + q, world, ld >> 2);
  } else {
    const int64_t i = 4 * quads + (q - quads);  // thread quads + k owns tail element k
    if (i < n) ((float AVT_GLOBAL*)out)[i] = rank_chain((const float AVT_GLOBAL*)parts + i, world, ld);
  }
}

}  // namespace

extern "C" int avt_rank_sum_f32(const float* parts, int world, int64_t n, int64_t ld, float* out, void* stream) {
  AVT_REQUIRE(parts && out, "avt_rank_sum_f32: NULL pointer");
  AVT_REQUIRE(world >= 1 && n >= 0, "avt_rank_sum_f32: world must be >= 1 and n >= 0 (world = %d, n = %lld)", world, (long long)n);
  AVT_REQUIRE(ld >= n && ld % 4 == 0, "avt_rank_sum_f32: ld must be a multiple of 4 floats and cover n (ld = %lld, n = %lld)",
              (long long)ld, (long long)n);
  AVT_REQUIRE(avt::aligned16(parts) && avt::aligned16(out), "avt_rank_sum_f32: parts and out must be 16-byte aligned");
  const int64_t items = (n >> 2) + (n & 3);  // 16-byte lanes + tail elements: one thread each
  const int64_t blocks = (items + kThreads - 1) / kThreads;
  AVT_REQUIRE(blocks < (1ll << 31), "avt_rank_sum_f32: vector too large (n = %lld: more than 2^31 - 1 blocks)", (long long)n);
  if (n == 0) return AVT_OK;
  hipLaunchKernelGGL(rank_sum_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), parts, out, world, n, ld);
  return avt::check_launch("avt_rank_sum_f32");
}
