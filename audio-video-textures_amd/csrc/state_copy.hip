// The training state — every parameter, buffer and momentum buffer — copied between its tensors and ONE flat device buffer in ONE launch
// (include/avt.h avt_state_copy_multi): what an epoch-end checkpoint costs the training stream (train_ops.StateSnapshot).  Per
// tensor, the same state is ~650 launches of a few microseconds each for config 5, most of them moving less than a kilobyte.
//
// The pattern of sgd.hip and grad_pack.hip: a DEVICE table of jobs — one per tensor — and a block-to-job map; block b owns bytes
// [(b - blk0) * 16384, + 16384) of its job.  Byte-granular: a job is (src, dst, nbytes), whatever the dtype (fp32 weights, int64
// num_batches_tracked, anything a state_dict holds).  Pack and unpack are the same kernel with src and dst exchanged in the table.
// HBM-bound: nbytes read, nbytes written.  Where src | dst is 16-byte aligned — a chunk starts a multiple of 16 KiB into its job, so the
// job's alignment is every chunk's — a lane issues its four 16-byte loads before the first store (16 KiB in flight per block, seven
// blocks per CU at the kernel's 69 registers); 4-byte aligned jobs (a view one float into its storage) take dwords, anything else bytes.  The nbytes % 16 tail of the
// last chunk goes through dwords and bytes, so nothing outside [dst, dst + nbytes) is ever written.  Vector loads and stores only: no LDS,
// no atomics.
#include "avt_common.h"

namespace {

constexpr int kChunk = 16384;   // bytes per block
constexpr int kThreads = 256;
// 16 bytes as the compiler's own vector type: registers (an array of HIP's uint4 struct, copied whole, was placed in the LDS)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// the table's pointers are device memory: said so, the accesses are global_load / global_store, not flat ones
#define AVT_GLOBAL __attribute__((address_space(1)))
typedef const unsigned char AVT_GLOBAL* gsrc_t;
typedef unsigned char AVT_GLOBAL* gdst_t;

struct StateJob {
  const unsigned char* src;
  unsigned char* dst;
  int64_t nbytes;
  int32_t blk0;        // the job's first block
  int32_t pad;
};
static_assert(sizeof(StateJob) == sizeof(AvtStateJob) && sizeof(StateJob) == 32, "AvtStateJob layout (include/avt.h)");

// bytes [0, n) with dword accesses where n allows and bytes for the rest: s and d 4-byte aligned
__device__ __forceinline__ void copy_dwords(gsrc_t __restrict__ s, gdst_t __restrict__ d, int n, int t) {
  const int n4 = n >> 2;
#pragma unroll 4
  for (int i = t; i < n4; i += kThreads) ((uint32_t AVT_GLOBAL*)d)[i] = ((const uint32_t AVT_GLOBAL*)s)[i];
  if (t < (n & 3)) d[(n4 << 2) + t] = s[(n4 << 2) + t];
}

__global__ __launch_bounds__(kThreads) void state_copy_multi_kernel(const StateJob* __restrict__ jobs, const int32_t* __restrict__ blk2job) {
  const StateJob j = jobs[blk2job[blockIdx.x]];
  const int64_t off = (int64_t)((int)blockIdx.x - j.blk0) * kChunk;
  const int64_t left = j.nbytes - off;
  if (left <= 0) return;
  const int n = left < kChunk ? (int)left : kChunk;
  gsrc_t __restrict__ s = (gsrc_t)(j.src + off);
  gdst_t __restrict__ d = (gdst_t)(j.dst + off);
  const int t = (int)threadIdx.x;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d);
  if ((bits & 15u) == 0) {
    constexpr int R = kChunk / (16 * kThreads);  // 16-byte accesses per lane
    const int n16 = n >> 4;
    u32x4 v[R];
    if (n == kChunk) {  // a whole chunk (all but the last block of a job): no predicates, the four loads issue back to back
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = ((const u32x4 AVT_GLOBAL*)s)[t + r * kThreads];
#pragma unroll
      for (int r = 0; r < R; ++r) ((u32x4 AVT_GLOBAL*)d)[t + r * kThreads] = v[r];
      return;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = t + r * kThreads;
      if (i < n16) v[r] = ((const u32x4 AVT_GLOBAL*)s)[i];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = t + r * kThreads;
      if (i < n16) ((u32x4 AVT_GLOBAL*)d)[i] = v[r];
    }
    copy_dwords(s + (n16 << 4), d + (n16 << 4), n & 15, t);  // the last chunk's tail: at most 3 dwords and 3 bytes
  } else if ((bits & 3u) == 0) {
    copy_dwords(s, d, n, t);
  } else {
#pragma unroll 4
    for (int i = t; i < n; i += kThreads) d[i] = s[i];
  }
}

}  // namespace

extern "C" int avt_state_job_bytes(void) { return (int)sizeof(StateJob); }

// jobs: DEVICE array of AvtStateJob, blk2job: DEVICE int32 [nblocks]; the caller has validated the jobs (train_ops.StateSnapshot builds
// them from dense device tensors and the slots of its own flat buffer)
extern "C" int avt_state_copy_multi(const void* jobs, const int32_t* blk2job, int nblocks, void* stream) {
  AVT_REQUIRE(jobs && blk2job, "avt_state_copy_multi: NULL pointer");
  AVT_REQUIRE(nblocks > 0, "avt_state_copy_multi: no blocks (nblocks = %d)", nblocks);
  AVT_REQUIRE(reinterpret_cast<uintptr_t>(jobs) % 8 == 0 && reinterpret_cast<uintptr_t>(blk2job) % 4 == 0,
              "avt_state_copy_multi: the job table must be 8-byte aligned, the block map 4-byte aligned");
  hipLaunchKernelGGL(state_copy_multi_kernel, dim3((unsigned)nblocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const StateJob*>(jobs), blk2job);
  return avt::check_launch("avt_state_copy_multi");
}
