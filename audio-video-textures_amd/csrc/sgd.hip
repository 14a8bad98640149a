// SGD (momentum, weight decay, Nesterov) over EVERY parameter of an optimizer in ONE launch, with the hyper-parameters read from
// device memory (include/avt.h avt_sgd_multi).  A training step replayed as a HIP graph (train_ops.GraphedStep) freezes every kernel
// ARGUMENT at capture: an optimizer whose learning rate is an argument keeps applying the first epoch's rate after the scheduler has
// stepped.  Here the rate is a load, so a replay applies whatever the host last copied into `hyper` (train_ops.ArenaSGD.sync_hyper).
//
// The pattern of weight_planes_multi (csrc/stem_train.hip): a DEVICE table of jobs — one per parameter — and a block-to-job map; block b
// owns elements [(b - blk0) * 4096, + 4096) of its job's tensor.  HBM-bound: 20 B per element with momentum (p, g, buf read; p, buf
// written), 12 B without.  Lanes move 16 B each (global_load_dwordx4, four per array and lane; eight waves per SIMD hide the latency) where p,
// g and buf are 16-byte aligned at the chunk; parameters that are views at a float offset take dword accesses.  No LDS, no atomics.
//
// Arithmetic: fp32, in the order of torch.optim.SGD's multi-tensor form, whose `add(alpha)` steps are single-rounded a + alpha * b:
//   g' = fma(wd, p, g)  (wd == 0: g as is)      buf = mu * buf + g'  (product rounded, then the sum)
//   d  = nesterov ? fma(mu, buf, g') : buf      p  = fma(-lr, d, p)
// (explicit fmaf: the library is built with -ffp-contract=off).  A zero buffer gives torch's first-step rule buf = g' exactly
// (dampening is 0).  inf / NaN in a gradient reach that element only.
#include "avt_common.h"

namespace {

constexpr int kChunk = 4096;    // elements per block
constexpr int kThreads = 256;

struct SgdJob {
  float* p;
  const float* g;
  float* buf;          // NULL: no momentum
  int64_t numel;
  int32_t group;       // row of `hyper`
  int32_t blk0;        // the job's first block
};
static_assert(sizeof(SgdJob) == sizeof(AvtSgdJob) && sizeof(SgdJob) == 40, "AvtSgdJob layout (include/avt.h)");

struct Hyper {
  float lr, mu, wd;
  bool nesterov;
};

template <bool MOM>
__device__ __forceinline__ float sgd_elem(float p, float g, float& b, const Hyper& h) {
  if (h.wd != 0.f) g = fmaf(h.wd, p, g);
  float d = g;
  if (MOM) {
    b = h.mu * b;
    b = b + g;
    d = h.nesterov ? fmaf(h.mu, b, g) : b;
  }
  return fmaf(-h.lr, d, p);
}

// one chunk: n <= kChunk elements at p / g / buf (already offset to the chunk)
template <bool MOM>
__device__ __forceinline__ void sgd_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int n, const Hyper& h) {
  const int t = (int)threadIdx.x;
  uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g);
  if (MOM) bits |= reinterpret_cast<uintptr_t>(buf);
  constexpr int R = kChunk / (4 * kThreads);  // float4 per lane
  if ((bits & 15u) == 0) {
    const int n4 = n >> 2;
    float4 vp[R], vg[R], vb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = t + r * kThreads;
      if (i < n4) {
        vp[r] = reinterpret_cast<const float4*>(p)[i];
        vg[r] = reinterpret_cast<const float4*>(g)[i];
        if (MOM) vb[r] = reinterpret_cast<const float4*>(buf)[i];
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = t + r * kThreads;
      if (i < n4) {
        float4 b = MOM ? vb[r] : make_float4(0.f, 0.f, 0.f, 0.f), o;
        o.x = sgd_elem<MOM>(vp[r].x, vg[r].x, b.x, h);
        o.y = sgd_elem<MOM>(vp[r].y, vg[r].y, b.y, h);
        o.z = sgd_elem<MOM>(vp[r].z, vg[r].z, b.z, h);
        o.w = sgd_elem<MOM>(vp[r].w, vg[r].w, b.w, h);
        reinterpret_cast<float4*>(p)[i] = o;
        if (MOM) reinterpret_cast<float4*>(buf)[i] = b;
      }
    }
    const int i = (n4 << 2) + t;  // the last chunk's tail: n % 4 elements
    if (t < (n & 3)) {
      float b = MOM ? buf[i] : 0.f;
      p[i] = sgd_elem<MOM>(p[i], g[i], b, h);
      if (MOM) buf[i] = b;
    }
  } else {  // float-aligned (a view that starts off a 16-byte boundary): dword accesses, still coalesced
#pragma unroll 4
    for (int i = t; i < n; i += kThreads) {
      float b = MOM ? buf[i] : 0.f;
      p[i] = sgd_elem<MOM>(p[i], g[i], b, h);
      if (MOM) buf[i] = b;
    }
  }
}

__global__ __launch_bounds__(kThreads) void sgd_multi_kernel(const SgdJob* __restrict__ jobs, const int32_t* __restrict__ blk2job,
                                                             const float* __restrict__ hyper) {
  const SgdJob j = jobs[blk2job[blockIdx.x]];
  const int64_t off = (int64_t)((int)blockIdx.x - j.blk0) * kChunk;
  const int64_t left = j.numel - off;
  if (left <= 0) return;
  const int n = left < kChunk ? (int)left : kChunk;
  const float* hy = hyper + (int64_t)j.group * 4;
  const Hyper h = {hy[0], hy[1], hy[2], hy[3] != 0.f};
  if (j.buf) sgd_chunk<true>(j.p + off, j.g + off, j.buf + off, n, h);
  else sgd_chunk<false>(j.p + off, j.g + off, nullptr, n, h);
}

}  // namespace

extern "C" int avt_sgd_job_bytes(void) { return (int)sizeof(SgdJob); }

// jobs: DEVICE array of AvtSgdJob, blk2job: DEVICE int32 [nblocks], hyper: DEVICE fp32 [n_groups][4]; the caller has validated the
// jobs (train_ops.ArenaSGD builds them from fp32, contiguous device tensors it checked at construction)
extern "C" int avt_sgd_multi(const void* jobs, const int32_t* blk2job, int nblocks, const float* hyper, void* stream) {
  AVT_REQUIRE(jobs && blk2job && hyper && nblocks > 0, "avt_sgd_multi: NULL pointer / no blocks");
  AVT_REQUIRE(reinterpret_cast<uintptr_t>(jobs) % 8 == 0 && reinterpret_cast<uintptr_t>(hyper) % 4 == 0,
              "avt_sgd_multi: the job table must be 8-byte aligned, hyper 4-byte aligned");
  hipLaunchKernelGGL(sgd_multi_kernel, dim3((unsigned)nblocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const SgdJob*>(jobs), blk2job, hyper);
  return avt::check_launch("avt_sgd_multi");
}

// The job table of a step that is being CAPTURED: the gradients of a captured step live in the graph's own memory pool, so their
// addresses — the table's contents — exist only once the capture runs.  This copy becomes a node of the graph (it re-reads `src_host`
// on every replay: PINNED memory the caller keeps alive and unchanged as long as the graph); outside a capture it is a plain async copy.
extern "C" int avt_sgd_upload(void* dst, const void* src_host, int64_t nbytes, void* stream) {
  AVT_REQUIRE(dst && src_host && nbytes > 0, "avt_sgd_upload: NULL pointer / nothing to copy");
  hipError_t e = hipMemcpyAsync(dst, src_host, (size_t)nbytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) {
    avt::set_error("avt_sgd_upload: %s", hipGetErrorString(e));
    return AVT_ERR_LAUNCH;
  }
  return AVT_OK;
}
