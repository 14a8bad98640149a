// classic_wide — the classic baseline past the 200 rows of classic.hip's LDS-resident q_learning kernel, and its P tail.
//
//   q_learning_wide   the same future-cost iteration (q_learning.py:27-68), bit for bit, for 2 <= n <= 65535.  Every row i >= 1
//                     receives the SAME addend a_t[j] = fl32(alpha * mins_t[j]), so the running matrix is never stored:
//                         old_0 = D3;   old_t[i, j] = fl32(D3[i, j] + a_{t-1}[j])  (i >= 1; row 0 stays D3's)
//                     and a sweep is one read-only pass over D3 with two n-vectors.  Launch s (s = 0, 1, ...) does, per row i:
//                         mins_s[i] = min_{k != i} old_s[i, k]  ->  a_s[i]              (needs a_{s-1})
//                         the row's share of residual_{s-1} = sum fl32(d * d), d = fl32(old_s - old_{s-1})   (needs a_{s-1}, a_{s-2})
//                     Sweep t's residual is therefore complete after launch t + 1, and launch t + 2 opens by reducing the
//                     per-workgroup fp64 partial sums (every workgroup does, in the same fixed order: no atomics) and deciding.
//                     The dependency between sweeps is the LAUNCH BOUNDARY: no workgroup waits for another.  Once a launch
//                     finds the stop rule met it sets a word in the workspace; every later launch returns on reading it.  A last
//                     launch writes D3 + a_{T-1}.
//   classic_p         sigma, exp, one-row shift, row-normalise and the optional threshold (computeD1.py:240-247; the same
//                     tail in computeD2.py and q_learning.py:53-64) in a statistics pass and a row pass.
#include "avt_common.h"

namespace {

constexpr int WT = 256;         // threads of every workgroup here
constexpr int WG_MAX = 1024;    // most workgroups of a launch = the length of one partial-sum buffer
constexpr int STATE_BYTES = 256;  // [0] stop word, [1] sweeps run
constexpr int POLL = 16;        // the host reads the stop word after every POLL launches

// ---- reductions over one workgroup, in a fixed order.  `slot` alternates between consecutive calls so that ONE barrier per call
// is enough: a slot is rewritten two calls later, behind the barrier of the call in between.
__device__ __forceinline__ double block_sum(double v, double (*red)[WT / 64], int slot) {
  v = avt::wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[slot][threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < WT / 64; ++w) s += red[slot][w];
  return s;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// a 16-byte load that asks for 4-byte alignment only: a row of an odd-sized matrix starts on any float
struct __attribute__((packed, aligned(4))) F4 {
  float x, y, z, w;
};
__device__ __forceinline__ F4 ld4(const float* p) { return *reinterpret_cast<const F4*>(p); }

// one element of row i: x = D3[i, k], a1 = a_{s-1}[k], a2 = a_{s-2}[k].  KIND 0: old_s = D3 and no residual (launch 0, and
// row 0 in every launch); 1: old_s = D3 + a1, old_{s-1} = D3 (launch 1); 2: old_s = D3 + a1, old_{s-1} = D3 + a2
template <int KIND>
__device__ __forceinline__ void q_elem(float x, float a1, float a2, bool diag, float& m, double& sq) {
  const float nw = KIND == 0 ? x : __fadd_rn(x, a1);
  if (!diag) m = fminf(m, nw);
  if (KIND >= 1) {
    const float od = KIND == 1 ? x : __fadd_rn(x, a2);
    const float d = __fsub_rn(nw, od);
    sq += (double)__fmul_rn(d, d);
  }
}

// one row by one wave: 16 bytes per lane and trip, the n % 4 last elements one per lane
template <int KIND>
__device__ __forceinline__ void q_row(const float* __restrict__ row, int n, int i, const float* __restrict__ a1,
                                      const float* __restrict__ a2, int lane, float& m, double& sq) {
  const int n4 = n >> 2;
#pragma unroll 4
  for (int q = lane; q < n4; q += 64) {
    const int k = q << 2;
    const F4 x = ld4(row + k);
    F4 u = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
    if (KIND >= 1) u = ld4(a1 + k);
    if (KIND >= 2) v = ld4(a2 + k);
    q_elem<KIND>(x.x, u.x, v.x, k == i, m, sq);
    q_elem<KIND>(x.y, u.y, v.y, k + 1 == i, m, sq);
    q_elem<KIND>(x.z, u.z, v.z, k + 2 == i, m, sq);
    q_elem<KIND>(x.w, u.w, v.w, k + 3 == i, m, sq);
  }
  const int k = (n4 << 2) + lane;
  if (lane < (n & 3)) q_elem<KIND>(row[k], KIND >= 1 ? a1[k] : 0.f, KIND >= 2 ? a2[k] : 0.f, k == i, m, sq);
}

// launch s of the iteration (see the head of this file): a wave per row, WT / 64 consecutive rows per workgroup and trip.
// part [2][WG_MAX] fp64, avec [3][astride] fp32; the grid size is the same for every launch of one run.
__global__ __launch_bounds__(WT) void q_wide_sweep_kernel(const float* __restrict__ d3, int n, float alpha, float tol, int max_iter, int s,
                                                          int* __restrict__ state, double* __restrict__ part,
                                                          float* __restrict__ avec, int astride) {
  __shared__ double red[2][WT / 64];
  __shared__ int stop_sh;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, G = gridDim.x;
  // one thread reads the word for the whole workgroup: workgroup 0 of THIS launch may be setting it, and either value read
  // leads to the same end (below), but all threads must take the same way to the barriers
  if (tid == 0) stop_sh = __hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (stop_sh) return;
  if (s >= 2) {  // residual of sweep s - 2, left by launch s - 1 as one fp64 partial per workgroup
    const double* pp = part + ((s - 1) & 1) * WG_MAX;
    double v = 0.0;
    for (int b = tid; b < G; b += WT) v += pp[b];
    const double sum = block_sum(v, red, 0);
    const float eps = (float)(sum / ((double)n * (double)n));
    if (!(eps > tol) || s - 1 >= max_iter) {  // the same decision in every workgroup: same values, same order
      if (blockIdx.x == 0 && tid == 0) {
        state[1] = s - 1;
        __hip_atomic_store(&state[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      return;
    }
  }
  const float* a1 = avec + (int64_t)((s + 2) % 3) * astride;  // a_{s-1}
  const float* a2 = avec + (int64_t)((s + 1) % 3) * astride;  // a_{s-2}
  float* a0 = avec + (int64_t)(s % 3) * astride;              // a_s
  double sq = 0.0;  // this lane's share of the residual, over all rows of its wave
  for (int i = blockIdx.x * (WT / 64) + wid; i < n; i += G * (WT / 64)) {
    const float* row = d3 + (int64_t)i * n;
    float m = INFINITY;
    if (s == 0 || i == 0)  // row 0 stays D3's and has no share in the residual
      q_row<0>(row, n, i, a1, a2, lane, m, sq);
    else if (s == 1)
      q_row<1>(row, n, i, a1, a2, lane, m, sq);
    else
      q_row<2>(row, n, i, a1, a2, lane, m, sq);
    m = wave_min(m);
    if (lane == 0) a0[i] = __fmul_rn(alpha, m);
  }
  const double wg = block_sum(sq, red, 1);
  if (tid == 0) part[(s & 1) * WG_MAX + blockIdx.x] = wg;
}

// out = D3 + a_{T-1} (rows >= 1), T = the sweeps run; *iters = T
__global__ __launch_bounds__(WT) void q_wide_final_kernel(const float* __restrict__ d3, int n, const int* __restrict__ state,
                                                          const float* __restrict__ avec, int astride, float* __restrict__ out,
                                                          int* __restrict__ iters) {
  const int T = state[1];
  const float* a = avec + (int64_t)((T + 2) % 3) * astride;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t base = (int64_t)i * n;
    for (int k = threadIdx.x; k < n; k += WT) out[base + k] = i == 0 ? d3[base + k] : __fadd_rn(d3[base + k], a[k]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && iters) *iters = T;
}

// ---- the P tail
// S = sum d (fp64) and Z = #(d != 0) as one partial per workgroup
template <bool VEC>
__global__ __launch_bounds__(WT) void classic_p_stats_kernel(const float* __restrict__ d, int64_t nn, double* __restrict__ psum,
                                                             long long* __restrict__ pcnt) {
  __shared__ double red[2][WT / 64];
  const int tid = threadIdx.x;
  double s = 0.0;
  long long z = 0;
  const int64_t t0 = (int64_t)blockIdx.x * WT + tid, step = (int64_t)gridDim.x * WT;
  if (VEC) {  // d 16-byte aligned; the nn % 4 last elements go to the first threads of the grid
    const int64_t n4 = nn >> 2;
    for (int64_t q = t0; q < n4; q += step) {
      const float4 x = reinterpret_cast<const float4*>(d)[q];
      s += (double)x.x;
      s += (double)x.y;
      s += (double)x.z;
      s += (double)x.w;
      z += (x.x != 0.f) + (x.y != 0.f) + (x.z != 0.f) + (x.w != 0.f);
    }
    if (t0 < (nn & 3)) {
      const float x = d[(n4 << 2) + t0];
      s += (double)x;
      z += x != 0.f;
    }
  } else {
    for (int64_t e = t0; e < nn; e += step) {
      const float x = d[e];
      s += (double)x;
      z += x != 0.f;
    }
  }
  const double ws = block_sum(s, red, 0);
  const double wz = block_sum((double)z, red, 1);  // at most 2^32 elements: exact in fp64
  if (tid == 0) {
    psum[blockIdx.x] = ws;
    pcnt[blockIdx.x] = (long long)wz;
  }
}

// sigma = fl32(fl32(sigma_factor) * fl32(fl32(S) / fl32(Z))), one workgroup
__global__ __launch_bounds__(WT) void classic_p_sigma_kernel(const double* __restrict__ psum, const long long* __restrict__ pcnt, int parts,
                                                             float sigma_factor, float* __restrict__ sigma) {
  __shared__ double red[2][WT / 64];
  double s = 0.0, z = 0.0;
  for (int b = threadIdx.x; b < parts; b += WT) {
    s += psum[b];
    z += (double)pcnt[b];
  }
  s = block_sum(s, red, 0);
  z = block_sum(z, red, 1);
  if (threadIdx.x == 0) *sigma = __fmul_rn(sigma_factor, __fdiv_rn((float)s, (float)z));  // z is an integer below 2^53
}

// row i of P from row min(i + 1, n - 1) of d
__global__ __launch_bounds__(WT) void classic_p_rows_kernel(const float* __restrict__ d, int n, const float* __restrict__ sigma_p, float th,
                                                            float* __restrict__ p, float* __restrict__ p_thr) {
  __shared__ double red[2][WT / 64];
  __shared__ float redx[2][WT / 64];
  const int tid = threadIdx.x;
  const float sigma = *sigma_p;
  int slot = 0;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const float* row = d + (int64_t)min(i + 1, n - 1) * n;
    double s = 0.0;
    float mx = 0.0f;  // every e >= 0
    for (int k = tid; k < n; k += WT) {
      const float e = expf(__fdiv_rn(-row[k], sigma));
      s += (double)e;
      mx = fmaxf(mx, e);
    }
    mx = avt::wave_max(mx);
    if ((tid & 63) == 0) redx[slot][tid >> 6] = mx;
    const float rs = (float)block_sum(s, red, slot);  // (its barrier publishes redx as well)
#pragma unroll
    for (int w = 0; w < WT / 64; ++w) mx = fmaxf(mx, redx[slot][w]);
    // the largest p of the row is the quotient of the largest e: a correctly rounded division is monotone
    const float cut = __fdiv_rn(mx, rs);
    const float lim = __fsub_rn(cut, __fmul_rn(th, cut));
    const int64_t base = (int64_t)i * n;
    for (int k = tid; k < n; k += WT) {
      const float v = __fdiv_rn(expf(__fdiv_rn(-row[k], sigma)), rs);
      p[base + k] = v;
      if (p_thr) p_thr[base + k] = v < lim ? 0.0f : v;
    }
    slot ^= 1;
  }
}

constexpr int64_t P_WS_BYTES = (int64_t)WG_MAX * (sizeof(double) + sizeof(long long));

}  // namespace

extern "C" int avt_q_learning_wide_supported(int n) { return (n >= 2 && n <= 65535) ? 1 : 0; }

extern "C" int64_t avt_q_learning_wide_workspace_bytes(int n) {
  if (!avt_q_learning_wide_supported(n)) return 0;
  return STATE_BYTES + 2 * (int64_t)WG_MAX * sizeof(double) + 3 * (int64_t)((n + 3) & ~3) * sizeof(float);
}

extern "C" int avt_q_learning_wide_f32(const float* d3, int n, float alpha, float tol, int max_iter, float* out, int* iters, void* ws,
                                       int64_t ws_bytes, void* stream) {
  AVT_REQUIRE(d3 && out && ws, "avt_q_learning_wide_f32: NULL pointer");
  AVT_REQUIRE(avt_q_learning_wide_supported(n), "avt_q_learning_wide_f32: the matrix must be 2..65535 rows square, got %d", n);
  AVT_REQUIRE(max_iter > 0 && max_iter <= (1 << 30), "avt_q_learning_wide_f32: max_iter must be 1..2^30");
  AVT_REQUIRE(ws_bytes >= avt_q_learning_wide_workspace_bytes(n), "avt_q_learning_wide_f32: the workspace holds %lld bytes, %lld needed",
              (long long)ws_bytes, (long long)avt_q_learning_wide_workspace_bytes(n));
  AVT_REQUIRE(avt::aligned16(ws), "avt_q_learning_wide_f32: the workspace must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* state = static_cast<int*>(ws);
  double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + STATE_BYTES);
  float* avec = reinterpret_cast<float*>(part + 2 * WG_MAX);
  const int astride = (n + 3) & ~3;
  const int rows_wg = WT / 64, want = (n + rows_wg - 1) / rows_wg;
  const dim3 grid((unsigned)(want < WG_MAX ? want : WG_MAX)), block(WT);
  hipError_t e = hipMemsetAsync(state, 0, STATE_BYTES, st);
  // launches 0 .. max_iter + 1: launch t + 2 decides on sweep t, and launch max_iter + 1 stops by the sweep count whatever the
  // residual is, so the word is set when the loop ends
  for (int s = 0; e == hipSuccess && s <= max_iter + 1; ++s) {
    hipLaunchKernelGGL(q_wide_sweep_kernel, grid, block, 0, st, d3, n, alpha, tol, max_iter, s, state, part, avec, astride);
    if (s % POLL == POLL - 1) {
      int stop = 0;
      e = hipMemcpyAsync(&stop, state, sizeof(int), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (stop) break;
    }
  }
  if (e != hipSuccess) {
    avt::set_error("avt_q_learning_wide_f32: %s", hipGetErrorString(e));
    return AVT_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(q_wide_final_kernel, grid, block, 0, st, d3, n, state, avec, astride, out, iters);
  return avt::check_launch("avt_q_learning_wide_f32");
}

extern "C" int64_t avt_classic_p_workspace_bytes(void) { return P_WS_BYTES; }

extern "C" int avt_classic_p_f32(const float* d, int n, float sigma_factor, int sigma_given, float* sigma, float threshold, float* p,
                                 float* p_thr, void* ws, int64_t ws_bytes, void* stream) {
  AVT_REQUIRE(d && sigma && p, "avt_classic_p_f32: NULL pointer");
  AVT_REQUIRE(n >= 2 && n <= 65535, "avt_classic_p_f32: the matrix must be 2..65535 rows square, got %d", n);
  AVT_REQUIRE(sigma_given || (ws && ws_bytes >= P_WS_BYTES && avt::aligned16(ws)),
              "avt_classic_p_f32: the statistics pass needs a 16-byte aligned workspace of %lld bytes", (long long)P_WS_BYTES);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!sigma_given) {
    const int64_t nn = (int64_t)n * n;
    const int64_t want = (nn + WT * 16 - 1) / (WT * 16);  // about 16 elements per thread
    const int parts = (int)(want < WG_MAX ? want : WG_MAX);
    double* psum = static_cast<double*>(ws);
    long long* pcnt = reinterpret_cast<long long*>(psum + WG_MAX);
    if (avt::aligned16(d))
      hipLaunchKernelGGL(classic_p_stats_kernel<true>, dim3(parts), dim3(WT), 0, st, d, nn, psum, pcnt);
    else
      hipLaunchKernelGGL(classic_p_stats_kernel<false>, dim3(parts), dim3(WT), 0, st, d, nn, psum, pcnt);
    hipLaunchKernelGGL(classic_p_sigma_kernel, dim3(1), dim3(WT), 0, st, psum, pcnt, parts, sigma_factor, sigma);
  }
  hipLaunchKernelGGL(classic_p_rows_kernel, dim3((unsigned)(n < 4 * WG_MAX ? n : 4 * WG_MAX)), dim3(WT), 0, st, d, n, sigma, threshold, p,
                     p_thr);
  return avt::check_launch("avt_classic_p_f32");
}
