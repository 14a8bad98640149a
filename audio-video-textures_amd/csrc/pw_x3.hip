// pw_x3 — the pointwise (1x1x1, stride 1) layers of the SlowFast encoder in the contract-grade split-plane arithmetic
// (see conv_x3.hip for the number format):  y = act( W x + b [+ r] )  on (hi, lo) plane pairs.
//
// Why a second x3 kernel: these layers — the bottlenecks' reducing / expanding convs (+ residual), 42 % of the x3
// encoder's time on the general tile — are HBM-bound (bytes/row = 4 (K + N [+ N]), two planes each), and the general
// tile serves them phase by phase (operands -> LDS -> MFMA -> fp32 staging -> residual -> stores, two barriers per tile,
// 2 workgroups per CU) at 2.5-3.7 TB/s.  Here, as in the bf16 path's pw_chain.hip, a WAVE owns 16 positions from load to
// store and nothing is staged: the input fragments (lane = position l & 15, k-group l >> 4: 16 contiguous bytes of a row)
// are the MFMA B operand as loaded; the weights are the first operand, resident in LDS as MFMA fragments for the whole
// launch (persistent workgroups), with their output rows permuted in the packing so that a lane ends up holding 8
// CONSECUTIVE channels of its position — one 16-byte store per plane, one 16-byte load per plane of the residual; no
// barrier in the position loop, 8 waves per CU keep ~20 KB of loads in flight each.
// A workgroup holds the fragments of NT1 x 16 output channels (both planes: NT1 x K1S x 2 KB <= 128 KB); wider layers
// are split into channel chunks handled by workgroups that are adjacent in the grid AND on one XCD (block b and b + 8
// share an XCD), so the chunks' re-reads of the same input rows meet in that XCD's L2.
// v_mfma_f32_16x16x32_{f16,bf16}: three passes per product, wl*xh + wh*xl + wh*xh, fp32 accumulate.
#include <limits.h>
#include <stdlib.h>

#include <iterator>
#include <type_traits>
#include <utility>

#include "avt_common.h"
#include "launch.h"
#include "mfma.h"
#include "split_planes.h"

namespace {

using avt::f32x4;
using avt::i32x4;
using avt::mfma16;

struct PxArgs {
  const uint16_t* xh;  // [M, ldx] input planes
  const uint16_t* xl;
  const uint16_t* rh;  // [M, ldr] residual planes or NULL
  const uint16_t* rl;
  uint16_t* yh;        // [M, ldy]
  uint16_t* yl;
  const i32x4* wh;     // [N/16][K1S][64 lanes] fragments (fused_slowfast.pack_pw_planes)
  const i32x4* wl;
  const float* bias;   // [N]
  const float* wscale; // [N] or NULL
  int M, ldx, ldr, ldy, k1c, ntiles, relu;
  int n_chunks, n_rg;  // channel chunks per row group, row groups (grid = 8-aligned n_rg * n_chunks)
  // temporal-tap form (avt_lateral_x3, round 4): the layer is Conv3d [taps,1,1] with temporal stride tst and padding tpad — the
  // lateral fast -> slow connections ([7,1,1] stride 4).  Output row p = ((b * To + to) * HW + pos); its K axis is tap-major
  // (k = dt * Cin + c, the convolution's own weight order), so 8-channel chunk ch of the operand is channels 8 (ch % cin8) .. + 7
  // of INPUT row ((b * T + to * tst - tpad + ch / cin8) * HW + pos): the same streaming kernel with a gathered operand — no im2col
  // pass, no tap table; frames outside [0, T) and chunks past the last tap are zero operands.  taps = 1: plain pointwise
  int taps, cin8, T, To, HW, tst, tpad;
  int n_valid;  // output channels that exist (the last 16-channel tile pair may be padding: cout 16 runs as one pair)
};

constexpr int PX_NW = 8;
// phase-skip diagnostic (tools/probe_pw_phases.sh builds one library per -DAVT_PW_DBG_CONST=n: 1 no stores, 2 no MFMAs,
// 4 no residual loads); the shipped library is built with 0
#ifndef AVT_PW_DBG_CONST
#define AVT_PW_DBG_CONST 0
#endif
#define PW_SKIP(bit) (((AVT_PW_DBG_CONST) & (bit)) != 0)
#ifndef PW_IL
#define PW_IL 2  // accumulators interleaved in the MFMA loop (NT1 is even)
#endif

// ---- the pieces the kernels share ----------------------------------------------------------------------------------------------------

// A wave's tile of 16 positions, as a lane sees it: does its position exist (`ok`: the stores' guard), the row it loads (`pc`: the
// last row where the tile is ragged), and its byte offset into a fragment
struct Tile {
  bool ok;
  int lofs;
  int64_t pc;
};

__device__ __forceinline__ Tile tile_of(int tile, int lane, int M) {
  const int p = tile * 16 + (lane & 15);
  const bool ok = p < M;
  int lofs = lane * 16;  // opaque per tile: keeps the loop-invariant fragment reads from being hoisted into registers
  asm volatile("" : "+v"(lofs));
  return Tile{ok, lofs, ok ? p : M - 1};
}

// the 8-channel chunk of k-step ks that k-group q reads: past the row's end the weights are zero: any finite value will do
__device__ __forceinline__ int row_chunk(int ks, int q, int k1c) {
  const int ch = 4 * ks + q;
  return ch < k1c ? ch : k1c - 1;
}

// a lane's part of its operand row — plane pairs: 16 bytes of each plane per k-step
template <int K1S>
__device__ __forceinline__ void load_row(const uint16_t* xh, const uint16_t* xl, int64_t pc, int ldx, int k1c, int q, i32x4 (&vh)[K1S],
                                         i32x4 (&vl)[K1S]) {
#pragma unroll
  for (int ks = 0; ks < K1S; ++ks) {
    const int ch = row_chunk(ks, q, k1c);
    vh[ks] = *reinterpret_cast<const i32x4*>(xh + pc * ldx + ch * 8);
    vl[ks] = *reinterpret_cast<const i32x4*>(xl + pc * ldx + ch * 8);
  }
}

// ... fp32 rows: the 8 channels as two 16-byte loads
template <int K1S>
__device__ __forceinline__ void load_row(const float* x, int64_t pc, int ldx, int k1c, int q, float4 (&xa)[K1S], float4 (&xb)[K1S]) {
#pragma unroll
  for (int ks = 0; ks < K1S; ++ks) {
    const float* px = x + pc * ldx + row_chunk(ks, q, k1c) * 8;
    xa[ks] = *reinterpret_cast<const float4*>(px);
    xb[ks] = *reinterpret_cast<const float4*>(px + 4);
  }
}

// packed fragments f0 .. f0 + n - 1 of both planes (fused_slowfast.pack_pw_planes: 1 KB each, 16 bytes per lane) -> LDS
__device__ __forceinline__ void stage_frags(char* dh, char* dl, const i32x4* wh, const i32x4* wl, int f0, int n, int wid, int lane) {
  for (int f = wid; f < n; f += PX_NW) {
    *reinterpret_cast<i32x4*>(dh + f * 1024 + lane * 16) = wh[(f0 + f) * 64 + lane];
    *reinterpret_cast<i32x4*>(dl + f * 1024 + lane * 16) = wl[(f0 + f) * 64 + lane];
  }
}

// channels c0 .. c0 + n - 1 of a layer's bias and row scales -> LDS (absent: 0 and 1)
__device__ __forceinline__ void stage_bias_scale(float* bl, float* sl, const float* bias, const float* wscale, int c0, int n, int tid) {
  for (int i = tid; i < n; i += PX_NW * 64) {
    bl[i] = bias ? bias[c0 + i] : 0.0f;
    sl[i] = wscale ? wscale[c0 + i] : 1.0f;
  }
}

// acc[n] += W[n] x for output tiles n = 0 .. NT - 1 over k-steps 0 .. NK - 1; fragment (n, ks) lies at whl / wll + (n * KS + ks) KB.
// IL accumulators in turn (round 4): every accumulator still sees its own three terms in the order wl*xh, wh*xl, wh*xh
// (bit-identical results), but no MFMA reads the result of the one issued just before it: -4.5 % on 256 -> 1024 + residual
// (pw_x3_kernel keeps its own copy, with its phase-skip hook: see profiles/r24)
template <bool F16, int KS, int NK, int NT, int IL>
__device__ __forceinline__ void product(const char* whl, const char* wll, int lofs, const i32x4* xh, const i32x4* xl, f32x4* acc) {
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) {
#pragma unroll
    for (int n = 0; n < NT; n += IL) {
      i32x4 wh[IL], wl[IL];
#pragma unroll
      for (int u = 0; u < IL; ++u) {
        const int f = (n + u) * KS + ks;
        wh[u] = *reinterpret_cast<const i32x4*>(whl + f * 1024 + lofs);
        wl[u] = *reinterpret_cast<const i32x4*>(wll + f * 1024 + lofs);
      }
#pragma unroll
      for (int u = 0; u < IL; ++u) acc[n + u] = mfma16<F16>(wl[u], xh[ks], acc[n + u]);
#pragma unroll
      for (int u = 0; u < IL; ++u) acc[n + u] = mfma16<F16>(wh[u], xl[ks], acc[n + u]);
#pragma unroll
      for (int u = 0; u < IL; ++u) acc[n + u] = mfma16<F16>(wh[u], xh[ks], acc[n + u]);
    }
  }
}

// A lane's two accumulators of a tile pair -> its 8 consecutive channels cl .. cl + 7 of the plane pair: scale + bias, the residual
// octet, ReLU, the split; stored at row `row` (of ld elements), column `col` of yh / yl when `store` — the offset is formed inside
// that branch, where the kernels formed it.  -> the planes as stored: the chained form's next operand.
// (pw_x3_kernel keeps its own copy, with its phase-skip hook: see profiles/r24)
struct Octet {
  uint4 h, l;
};

template <bool F16>
__device__ __forceinline__ Octet octet_epilogue(const f32x4& a0, const f32x4& a1, const float* bl, const float* sl, int cl, bool has_res,
                                                const uint4& rh, const uint4& rl, bool relu, bool store, uint16_t* yh, uint16_t* yl,
                                                int64_t row, int ld, int col) {
  const float4 ba = *reinterpret_cast<const float4*>(bl + cl), bb = *reinterpret_cast<const float4*>(bl + cl + 4);
  const float4 sa = *reinterpret_cast<const float4*>(sl + cl), sb = *reinterpret_cast<const float4*>(sl + cl + 4);
  float v[8] = {a0[0] * sa.x + ba.x, a0[1] * sa.y + ba.y, a0[2] * sa.z + ba.z, a0[3] * sa.w + ba.w,
                a1[0] * sb.x + bb.x, a1[1] * sb.y + bb.y, a1[2] * sb.z + bb.z, a1[3] * sb.w + bb.w};
  if (has_res) {
    const uint32_t* ph = reinterpret_cast<const uint32_t*>(&rh);
    const uint32_t* pl = reinterpret_cast<const uint32_t*>(&rl);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const avt::f32x2 r = avt::join2<F16>(ph[e], pl[e]);
      v[2 * e] += r.x;
      v[2 * e + 1] += r.y;
    }
  }
  if (relu) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = avt::relu_keep_nan(v[i]);
  }
  Octet y;
  avt::split2<F16>(v[0], v[1], y.h.x, y.l.x);
  avt::split2<F16>(v[2], v[3], y.h.y, y.l.y);
  avt::split2<F16>(v[4], v[5], y.h.z, y.l.z);
  avt::split2<F16>(v[6], v[7], y.h.w, y.l.w);
  if (store) {
    const int64_t o = row * ld + col;
    *reinterpret_cast<uint4*>(yh + o) = y.h;
    *reinterpret_cast<uint4*>(yl + o) = y.l;
  }
  return y;
}

template <int K1S, int NT1, bool F16>
__global__ __launch_bounds__(PX_NW * 64) void pw_x3_kernel(PxArgs a) {
  constexpr int NC = NT1 * 16;  // output channels of this workgroup's chunk
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* whl = lds;                                   // [NT1][K1S] fragments of 1 KB
  char* wll = whl + NT1 * K1S * 1024;
  float* bl = reinterpret_cast<float*>(wll + NT1 * K1S * 1024);  // [NC] bias, [NC] scale
  float* sl = bl + NC;

  // block -> (row group, channel chunk): the chunks of one row group are consecutive blocks of ONE XCD
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int chunk = j % a.n_chunks;
  const int rg = (j / a.n_chunks) * 8 + xcd;
  if (rg >= a.n_rg) return;
  const int c0 = chunk * NC;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4;
  const int f0 = chunk * NT1 * K1S;  // first fragment of the chunk
  stage_frags(whl, wll, a.wh, a.wl, f0, NT1 * K1S, wid, lane);
  stage_bias_scale(bl, sl, a.bias, a.wscale, c0, NC, tid);
  __syncthreads();
  const bool has_res = a.rh != nullptr;

  for (int tile = rg * PX_NW + wid; tile < a.ntiles; tile += a.n_rg * PX_NW) {
    const auto [ok, lofs, pc] = tile_of(tile, lane, a.M);
    i32x4 xh[K1S], xl[K1S];
    if (a.taps > 1) {  // uniform: the temporal-tap form
      const int bto = (int)pc / a.HW, pos = (int)pc - bto * a.HW;
      const int b = bto / a.To, to = bto - b * a.To;
#pragma unroll
      for (int ks = 0; ks < K1S; ++ks) {
        const int ch = 4 * ks + q;
        const int dt = ch / a.cin8, cc = ch - dt * a.cin8;
        const int t_in = to * a.tst - a.tpad + dt;
        const bool valid = dt < a.taps && (unsigned)t_in < (unsigned)a.T;
        const int64_t o = (((int64_t)b * a.T + (valid ? t_in : 0)) * a.HW + pos) * a.ldx + cc * 8;
        const i32x4 vh = *reinterpret_cast<const i32x4*>(a.xh + o), vl = *reinterpret_cast<const i32x4*>(a.xl + o);
        xh[ks] = valid ? vh : i32x4{0, 0, 0, 0};
        xl[ks] = valid ? vl : i32x4{0, 0, 0, 0};
      }
    } else {
      load_row<K1S>(a.xh, a.xl, pc, a.ldx, a.k1c, q, xh, xl);
    }
    uint4 rfh[NT1 / 2], rfl[NT1 / 2];
    if (has_res && !PW_SKIP(4)) {
#pragma unroll
      for (int jj = 0; jj < NT1 / 2; ++jj) {
        const int64_t o = pc * a.ldr + c0 + 32 * jj + 8 * q;
        rfh[jj] = *reinterpret_cast<const uint4*>(a.rh + o);
        rfl[jj] = *reinterpret_cast<const uint4*>(a.rl + o);
      }
    }
    f32x4 acc[NT1];
#pragma unroll
    for (int n = 0; n < NT1; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < K1S; ++ks) {
#pragma unroll
      for (int n = 0; n < NT1; n += PW_IL) {
        // PW_IL accumulators in turn (round 4): every accumulator still sees its own three terms in the order wl*xh, wh*xl, wh*xh
        // (bit-identical results), but no MFMA reads the result of the one issued just before it: -4.5 % on 256 -> 1024 + residual
        i32x4 wh[PW_IL], wl[PW_IL];
#pragma unroll
        for (int u = 0; u < PW_IL; ++u) {
          const int f = (n + u) * K1S + ks;
          wh[u] = *reinterpret_cast<const i32x4*>(whl + f * 1024 + lofs);
          wl[u] = *reinterpret_cast<const i32x4*>(wll + f * 1024 + lofs);
        }
        if (!PW_SKIP(2)) {
#pragma unroll
          for (int u = 0; u < PW_IL; ++u) acc[n + u] = mfma16<F16>(wl[u], xh[ks], acc[n + u]);
#pragma unroll
          for (int u = 0; u < PW_IL; ++u) acc[n + u] = mfma16<F16>(wh[u], xl[ks], acc[n + u]);
#pragma unroll
          for (int u = 0; u < PW_IL; ++u) acc[n + u] = mfma16<F16>(wh[u], xh[ks], acc[n + u]);
        } else {
#pragma unroll
          for (int u = 0; u < PW_IL; ++u)
            acc[n + u][0] += __builtin_bit_cast(float, wl[u][0] ^ xh[ks][0] ^ wh[u][1] ^ xl[ks][1]);  // keep the operands alive
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < NT1 / 2; ++jj) {  // tiles 2jj, 2jj+1 -> channels c0 + 32 jj + 8 q .. + 7
      const int cl = 32 * jj + 8 * q;
      const float4 ba = *reinterpret_cast<const float4*>(bl + cl), bb = *reinterpret_cast<const float4*>(bl + cl + 4);
      const float4 sa = *reinterpret_cast<const float4*>(sl + cl), sb = *reinterpret_cast<const float4*>(sl + cl + 4);
      float v[8] = {acc[2 * jj][0] * sa.x + ba.x,     acc[2 * jj][1] * sa.y + ba.y,
                    acc[2 * jj][2] * sa.z + ba.z,     acc[2 * jj][3] * sa.w + ba.w,
                    acc[2 * jj + 1][0] * sb.x + bb.x, acc[2 * jj + 1][1] * sb.y + bb.y,
                    acc[2 * jj + 1][2] * sb.z + bb.z, acc[2 * jj + 1][3] * sb.w + bb.w};
      if (has_res) {
        const uint32_t* ph = reinterpret_cast<const uint32_t*>(&rfh[jj]);
        const uint32_t* pl = reinterpret_cast<const uint32_t*>(&rfl[jj]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const avt::f32x2 r = avt::join2<F16>(ph[e], pl[e]);
          v[2 * e] += r.x;
          v[2 * e + 1] += r.y;
        }
      }
      if (a.relu) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = avt::relu_keep_nan(v[i]);
      }
      uint4 oh, ol;
      avt::split2<F16>(v[0], v[1], oh.x, ol.x);
      avt::split2<F16>(v[2], v[3], oh.y, ol.y);
      avt::split2<F16>(v[4], v[5], oh.z, ol.z);
      avt::split2<F16>(v[6], v[7], oh.w, ol.w);
      if (ok && c0 + cl < a.n_valid && (!PW_SKIP(1) || (oh.x ^ ol.x) == 0x12345678u)) {
        const int64_t o = pc * a.ldy + c0 + cl;
        *reinterpret_cast<uint4*>(a.yh + o) = oh;
        *reinterpret_cast<uint4*>(a.yl + o) = ol;
      }
    }
  }
}

// ---- chained form: y = act(W1 x + b1 [+ r]) AND z = relu(W2 y + b2) in one pass over the rows ---------------------------------
// The slow pathway's  c of block i (+ residual + ReLU)  ->  a of block i + 1 (+ ReLU)  (the x3 counterpart of pw_chain.hip):
// the first GEMM's D layout — a lane ends with 8 consecutive channels of its position, already split into the two planes it
// stores — IS the second GEMM's B-operand layout (k-group q of k-step jj = channels 32 jj + 8 q .. + 7), so y goes from the
// epilogue's registers into the next MFMAs without touching LDS or HBM again: the a layer's read of y (256 channels x 2 planes
// per row, a third of the pair's bytes) disappears.  z is computed from the SAME rounded planes the unchained a layer would
// read, in the same k order: bit-identical to the two launches.  One chunk holds all N1 channels (res2: 64 -> 256 -> 64:
// 64 + 64 KB of fragments, one 8-wave workgroup per CU).
struct PcArgs {
  PxArgs p;            // first layer (wh / wl / bias / wscale / relu of layer 1; n_chunks == 1)
  const i32x4* w2h;    // [N2/16][K2S][64 lanes] fragments of layer 2 over K2 = N1
  const i32x4* w2l;
  const float* bias2;
  const float* wscale2;
  uint16_t* zh;        // [M, ldz]
  uint16_t* zl;
  int ldz;
};

template <int K1S, int NT1, int NT2, bool F16>
__global__ __launch_bounds__(PX_NW * 64) void pw_chain_x3_kernel(PcArgs c) {
  const PxArgs& a = c.p;
  constexpr int NC = NT1 * 16, K2S = NT1 / 2, NC2 = NT2 * 16;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* whl = lds;
  char* wll = whl + NT1 * K1S * 1024;
  char* w2hl = wll + NT1 * K1S * 1024;
  char* w2ll = w2hl + NT2 * K2S * 1024;
  float* bl = reinterpret_cast<float*>(w2ll + NT2 * K2S * 1024);  // [NC] bias, [NC] scale, [NC2] bias2, [NC2] scale2
  float* sl = bl + NC;
  float* b2l = sl + NC;
  float* s2l = b2l + NC2;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4;
  stage_frags(whl, wll, a.wh, a.wl, 0, NT1 * K1S, wid, lane);
  stage_frags(w2hl, w2ll, c.w2h, c.w2l, 0, NT2 * K2S, wid, lane);
  stage_bias_scale(bl, sl, a.bias, a.wscale, 0, NC, tid);
  stage_bias_scale(b2l, s2l, c.bias2, c.wscale2, 0, NC2, tid);
  __syncthreads();
  const bool has_res = a.rh != nullptr;

  for (int tile = blockIdx.x * PX_NW + wid; tile < a.ntiles; tile += gridDim.x * PX_NW) {
    const auto [ok, lofs, pc] = tile_of(tile, lane, a.M);
    i32x4 xh[K1S], xl[K1S];
    load_row<K1S>(a.xh, a.xl, pc, a.ldx, a.k1c, q, xh, xl);
    uint4 rfh[NT1 / 2], rfl[NT1 / 2];
    if (has_res) {
#pragma unroll
      for (int jj = 0; jj < NT1 / 2; ++jj) {
        const int64_t o = pc * a.ldr + 32 * jj + 8 * q;
        rfh[jj] = *reinterpret_cast<const uint4*>(a.rh + o);
        rfl[jj] = *reinterpret_cast<const uint4*>(a.rl + o);
      }
    }
    f32x4 acc2[NT2];
#pragma unroll
    for (int n = 0; n < NT2; ++n) acc2[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < NT1 / 2; ++jj) {  // tiles 2jj, 2jj+1 of layer 1 -> channels 32 jj + 8 q .. + 7 = k-step jj of layer 2
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < K1S; ++ks) {
        const int f0 = (2 * jj) * K1S + ks, f1 = (2 * jj + 1) * K1S + ks;
        const i32x4 w0h = *reinterpret_cast<const i32x4*>(whl + f0 * 1024 + lofs), w0l = *reinterpret_cast<const i32x4*>(wll + f0 * 1024 + lofs);
        const i32x4 w1h = *reinterpret_cast<const i32x4*>(whl + f1 * 1024 + lofs), w1l = *reinterpret_cast<const i32x4*>(wll + f1 * 1024 + lofs);
        a0 = mfma16<F16>(w0l, xh[ks], a0);
        a0 = mfma16<F16>(w0h, xl[ks], a0);
        a0 = mfma16<F16>(w0h, xh[ks], a0);
        a1 = mfma16<F16>(w1l, xh[ks], a1);
        a1 = mfma16<F16>(w1h, xl[ks], a1);
        a1 = mfma16<F16>(w1h, xh[ks], a1);
      }
      const int cl = 32 * jj + 8 * q;
      const Octet y = octet_epilogue<F16>(a0, a1, bl, sl, cl, has_res, rfh[jj], rfl[jj], a.relu != 0, ok, a.yh, a.yl, pc, a.ldy, cl);
      const uint4 oh = y.h, ol = y.l;
      // layer 2, k-step jj: the planes just stored are the operand
      const i32x4 yh = __builtin_bit_cast(i32x4, oh), yl = __builtin_bit_cast(i32x4, ol);
      product<F16, K2S, 1, NT2, 1>(w2hl + jj * 1024, w2ll + jj * 1024, lofs, &yh, &yl, acc2);
    }
#pragma unroll
    for (int jj = 0; jj < NT2 / 2; ++jj) {
      const int cl = 32 * jj + 8 * q;
      octet_epilogue<F16>(acc2[2 * jj], acc2[2 * jj + 1], b2l, s2l, cl, false, uint4{}, uint4{}, true, ok, c.zh, c.zl, pc, c.ldz, cl);
    }
  }
}

// ---- the TRAINING form: fp32 rows in, fp32 rows out (train_ops.conv3d's pointwise layers: forward and stride-1 input gradient) -----
// The expanding 1x1x1 convolutions of the bottlenecks (64 -> 256, 128 -> 512, 256 -> 1024 and the fast pathway's 8 -> 32 ... 64 -> 256)
// and the input gradients of the reducing ones are the widest-output layers of the step, and K is one to four 64-wide steps: on
// the 128 x 128 tile a workgroup's prologue and epilogue were 26 + 29 % of its cycles and the layer ran at 1.1 TB/s (128 -> 512 at
// 28^2: 1.86 ms per 128 clips, profiles/r04/train_pw_f32_ab.log).  Same streaming structure as pw_x3_kernel: a wave owns 16 positions
// from load to store; its fp32 operand chunks (8 consecutive channels = two 16-byte loads) are split into the two planes in registers
// and are the MFMA B operand; the weight planes arrive in their plain [N][K] layout (they change every optimizer step: no host
// packing) and the prologue of the persistent workgroup lays them out as fragments in LDS; the epilogue scales (fp16 planes' row
// scales), adds the optional fp32 `add` rows and stores 8 consecutive channels per lane as two non-temporal 16-byte stores.
struct PfArgs {
  const float* x;        // [M, ldx]
  const float* add;      // [M, lda] or NULL
  float* y;              // [M, ldy]
  const uint16_t* wh;    // [N][K] plain planes
  const uint16_t* wl;
  const float* wscale;   // [N] or NULL
  int M, ldx, lda, ldy, K, k1c, ntiles, n_chunks, n_rg;
  // STATS (round 5; avt_pw_x3_f32_stats): the output feeds a train-mode BatchNorm — blockIdx.y walks its replica groups (slabs of
  // M rows each: `M` / `ntiles` are PER GROUP then), and every wave leaves the per-channel sum / sum of squares of the rows it
  // stored as one row of partials in bn_train.hip's channel_sums layout (row (group * n_rg + rg) * 8 + wave)
  double* stat_part;
  int n_total;           // channels of the whole layer (the BatchNorm's C)
  // STATS = 2 (avt_pw_x3_f32_bwdstats): the launch is an input gradient whose result is the OUTPUT gradient of a train-mode
  // BatchNorm (+ ReLU) — see conv_args.h (bst_*): the BatchNorm's input rows [M, ldy], its saved statistics [groups][N], scale,
  // shift (mask recomputed) or saved mask bits; the result is stored MASKED and the partial rows hold the sums of g and g * xhat
  const float* bst_x;
  const float* bst_mean;
  const float* bst_invstd;
  const float* bst_gamma;
  const float* bst_beta;
  const uint8_t* bst_mask;
  int bst_relu;
};

// pass width (channels) of the STATS transpose: the per-wave LDS scratch must fit beside the weight fragments
template <int K1S, int NT1>
struct PfStat {
  static constexpr int NC = NT1 * 16;
  static constexpr int PW = NC < 64 ? NC : ((2 * NT1 * K1S * 1024 >= 96 * 1024) ? 32 : 64);
  static constexpr int RS = PW + 4;                      // floats per scratch row (padded)
  static constexpr int BYTES = PX_NW * 16 * RS * 4;      // all waves
};

template <int K1S, int NT1, bool F16, int STATS = 0>
__global__ __launch_bounds__(PX_NW * 64) void pw_x3_f32_kernel(PfArgs a) {
  constexpr int NC = NT1 * 16;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* whl = lds;
  char* wll = whl + NT1 * K1S * 1024;
  float* sl = reinterpret_cast<float*>(wll + NT1 * K1S * 1024);  // [NC] scale

  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int chunk = j % a.n_chunks;
  const int rg = (j / a.n_chunks) * 8 + xcd;
  if (rg >= a.n_rg) return;
  const int c0 = chunk * NC;
  if constexpr (STATS != 0) {  // this workgroup's group: its slab of the rows
    const int64_t g = blockIdx.y;
    a.x += g * a.M * a.ldx;
    a.y += g * a.M * a.ldy;
    if constexpr (STATS == 2) {
      if (a.add) a.add += g * a.M * a.lda;
      a.bst_x += g * a.M * a.ldy;
      if (a.bst_mask) a.bst_mask += g * a.M * a.ldy / 4;
    }
  }

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  // fragments from the plain planes (fused_slowfast.pack_pw_planes' order): fragment (nt, ks), lane (n = l15, q): 8 consecutive k of
  // output row 32 (nt / 2) + 8 (n >> 2) + 4 (nt % 2) + (n & 3), k = 32 ks + 8 q ..; k past the row's end = zeros
  for (int f = wid; f < NT1 * K1S; f += PX_NW) {
    const int nt = f / K1S, ks = f - nt * K1S;
    const int row = c0 + 32 * (nt >> 1) + 8 * (l15 >> 2) + 4 * (nt & 1) + (l15 & 3);
    const int col = 32 * ks + 8 * q;
    i32x4 vh = {0, 0, 0, 0}, vl = {0, 0, 0, 0};
    if (col < a.K) {
      vh = *reinterpret_cast<const i32x4*>(a.wh + (int64_t)row * a.K + col);
      vl = *reinterpret_cast<const i32x4*>(a.wl + (int64_t)row * a.K + col);
    }
    *reinterpret_cast<i32x4*>(whl + f * 1024 + lane * 16) = vh;
    *reinterpret_cast<i32x4*>(wll + f * 1024 + lane * 16) = vl;
  }
  for (int i = tid; i < NC; i += PX_NW * 64) sl[i] = a.wscale ? a.wscale[c0 + i] : 1.0f;
  // STATS = 2: this (group, chunk)'s BatchNorm coefficients [mean | invstd * gamma | beta] behind the statistics scratch
  float* kc = reinterpret_cast<float*>(reinterpret_cast<char*>(sl) + NC * 4 + PfStat<K1S, NT1>::BYTES);
  if constexpr (STATS == 2) {
    for (int i = tid; i < NC; i += PX_NW * 64) {
      const size_t gc = (size_t)blockIdx.y * a.n_total + c0 + i;
      kc[i] = a.bst_mean[gc];
      kc[NC + i] = a.bst_invstd[gc] * a.bst_gamma[c0 + i];  // the forward's scale: the same product
      kc[2 * NC + i] = a.bst_beta ? a.bst_beta[c0 + i] : 0.0f;
    }
  }
  __syncthreads();
  const bool has_add = STATS != 1 && a.add != nullptr;
  // STATS: per-wave scratch [16 rows][PW channels] behind the scale floats; lane l owns column l of every pass (PW = 32: column
  // l & 31, rows 8 (l >> 5) ..), its sums over the wave's tiles in fp64 (fp32 over the 16 / 8 rows of one tile)
  typedef PfStat<K1S, NT1> PS;
  constexpr int NPASS = NC / PS::PW;
  float* scr = reinterpret_cast<float*>(reinterpret_cast<char*>(sl) + NC * 4) + wid * 16 * PS::RS;
  double st_s[STATS != 0 ? NPASS : 1], st_q[STATS != 0 ? NPASS : 1];
  if constexpr (STATS != 0) {
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) st_s[ps] = st_q[ps] = 0.0;
  }

  for (int tile = rg * PX_NW + wid; tile < a.ntiles; tile += a.n_rg * PX_NW) {
    const Tile t = tile_of(tile, lane, a.M);
    int kz = 0;  // opaque per tile as lofs is: the same for the STATS = 2 coefficient reads
    asm volatile("" : "+v"(kz));
    float4 xa[K1S], xb[K1S];
    load_row<K1S>(a.x, t.pc, a.ldx, a.k1c, q, xa, xb);
    // the epilogue's operands (`add` rows, STATS = 2: the BatchNorm input's octets + mask nibbles), requested ahead of their use.
    // (The three phases are lambdas, each called once: written straight into the tile loop, the uniform choices inside them come out
    //  as branches instead of selects and the plain instances take up to 6 more registers — profiles/r24)
    float4 ra[NT1 / 2], rb[NT1 / 2];
    float4 bxa[STATS == 2 ? NT1 / 2 : 1], bxb[STATS == 2 ? NT1 / 2 : 1];
    unsigned bbits[STATS == 2 ? NT1 / 2 : 1];
    auto epi_request = [&] {
#pragma unroll
    for (int jj = 0; jj < NT1 / 2; ++jj) {
      if (has_add) {
        const float* pr = a.add + t.pc * a.lda + c0 + 32 * jj + 8 * q;
        ra[jj] = *reinterpret_cast<const float4*>(pr);
        rb[jj] = *reinterpret_cast<const float4*>(pr + 4);
      }
      if constexpr (STATS == 2) {
        const int64_t o = t.pc * a.ldy + c0 + 32 * jj + 8 * q;
        bxa[jj] = *reinterpret_cast<const float4*>(a.bst_x + o);
        bxb[jj] = *reinterpret_cast<const float4*>(a.bst_x + o + 4);
        const unsigned v = a.bst_mask ? *reinterpret_cast<const uint16_t*>(a.bst_mask + (o >> 2)) : 0u;
        bbits[jj] = (v & 0xFu) | ((v >> 4) & 0xF0u);
      }
    }
    };
    epi_request();
    i32x4 xh[K1S], xl[K1S];
#pragma unroll
    for (int ks = 0; ks < K1S; ++ks) {
      const float f8[8] = {xa[ks].x, xa[ks].y, xa[ks].z, xa[ks].w, xb[ks].x, xb[ks].y, xb[ks].z, xb[ks].w};
      uint4 h, l;
      avt::split8<F16>(f8, h, l);
      xh[ks] = __builtin_bit_cast(i32x4, h);
      xl[ks] = __builtin_bit_cast(i32x4, l);
    }
    f32x4 acc[NT1];
    auto mfma_part = [&] {
#pragma unroll
      for (int n = 0; n < NT1; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
      product<F16, K1S, K1S, NT1, PW_IL>(whl, wll, t.lofs, xh, xl, acc);
    };
    f32x4 hv[4];  // (STATS = 2: the second statistic's addends of one pass)
    auto epilogue = [&] {
#pragma unroll
    for (int jj = 0; jj < NT1 / 2; ++jj) {  // tiles 2jj, 2jj+1 -> channels c0 + 32 jj + 8 q .. + 7
      const int cl = 32 * jj + 8 * q;
      f32x4 o0, o1;
      if constexpr (STATS == 2) {  // (gradients: bf16 planes, no row scales — and no 4 NT1 scale registers held across the tile loop)
        o0 = f32x4{acc[2 * jj][0], acc[2 * jj][1], acc[2 * jj][2], acc[2 * jj][3]};
        o1 = f32x4{acc[2 * jj + 1][0], acc[2 * jj + 1][1], acc[2 * jj + 1][2], acc[2 * jj + 1][3]};
      } else {
        const float4 sa = *reinterpret_cast<const float4*>(sl + cl), sb = *reinterpret_cast<const float4*>(sl + cl + 4);
        o0 = f32x4{acc[2 * jj][0] * sa.x, acc[2 * jj][1] * sa.y, acc[2 * jj][2] * sa.z, acc[2 * jj][3] * sa.w};
        o1 = f32x4{acc[2 * jj + 1][0] * sb.x, acc[2 * jj + 1][1] * sb.y, acc[2 * jj + 1][2] * sb.z, acc[2 * jj + 1][3] * sb.w};
      }
      if (has_add) {
        o0 += f32x4{ra[jj].x, ra[jj].y, ra[jj].z, ra[jj].w};
        o1 += f32x4{rb[jj].x, rb[jj].y, rb[jj].z, rb[jj].w};
      }
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;  // STATS = 2: g * (x - mean), the second statistic's addends
      if constexpr (STATS == 2) {  // o becomes g = mask * dz (what is stored)
        // (coefficients through an offset that is opaque per tile: read at constant addresses they are loop-invariant, and the
        //  compiler kept all 24 x NT1 / 2 of them in registers across the tile loop — 54-108 spilled registers)
        const float* kct = kc + kz;
        const float4 m0 = *reinterpret_cast<const float4*>(kct + cl), m1 = *reinterpret_cast<const float4*>(kct + cl + 4);
        const float4 s0 = *reinterpret_cast<const float4*>(kct + NC + cl), s1 = *reinterpret_cast<const float4*>(kct + NC + cl + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(kct + 2 * NC + cl), b1 = *reinterpret_cast<const float4*>(kct + 2 * NC + cl + 4);
        const float xc[8] = {bxa[jj].x - m0.x, bxa[jj].y - m0.y, bxa[jj].z - m0.z, bxa[jj].w - m0.w,
                             bxb[jj].x - m1.x, bxb[jj].y - m1.y, bxb[jj].z - m1.z, bxb[jj].w - m1.w};
        const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, be[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        float gg[8] = {o0[0], o0[1], o0[2], o0[3], o1[0], o1[1], o1[2], o1[3]}, vv[8];
        // (uniform choices folded into the select's operands: see bst_apply in conv_args.h)
        const bool by_bits = a.bst_relu != 0 && a.bst_mask != nullptr, by_x = a.bst_relu != 0 && a.bst_mask == nullptr;
        const unsigned mbits = by_bits ? bbits[jj] : 0xFFu;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float act = by_x ? xc[e] * sc[e] + be[e] : 1.0f;
          const float sel = (((mbits >> e) & 1u) != 0u && act > 0.0f) ? 1.0f : 0.0f;
          gg[e] = sel != 0.0f ? gg[e] : 0.0f;
          vv[e] = gg[e] * xc[e];
        }
        o0 = f32x4{gg[0], gg[1], gg[2], gg[3]};
        o1 = f32x4{gg[4], gg[5], gg[6], gg[7]};
        v0 = f32x4{vv[0], vv[1], vv[2], vv[3]};
        v1 = f32x4{vv[4], vv[5], vv[6], vv[7]};
      }
      if (t.ok) {
        float* po = a.y + t.pc * a.ldy + c0 + cl;
        avt::stg4(po, o0);
        avt::stg4(po + 4, o1);
      }
      if constexpr (STATS == 2) {
        // as below, with two blocks per pass: g for the first statistic, g * (x - mean) for the second (held in registers — at
        // most two octets — until the first block has been read back)
        constexpr int JPP = PS::PW / 32;
        const int jl = jj % JPP;
        if (!t.ok) o0 = o1 = v0 = v1 = f32x4{0.f, 0.f, 0.f, 0.f};
        float* pw_ = scr + l15 * PS::RS + 32 * jl + 8 * q;
        *reinterpret_cast<f32x4*>(pw_) = o0;
        *reinterpret_cast<f32x4*>(pw_ + 4) = o1;
        if (jl == 0) { hv[0] = v0; hv[1] = v1; } else { hv[2] = v0; hv[3] = v1; }
        if (jl == JPP - 1) {
          constexpr int NR = PS::PW == 64 ? 16 : 8;
          const float* pr = scr + (PS::PW == 64 ? lane : (lane & 31) + (lane >> 5) * 8 * PS::RS);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          float ts = 0.f, tq = 0.f;
          if (PS::PW >= 32 || lane < PS::PW) {
#pragma unroll
            for (int r = 0; r < NR; ++r) ts += pr[r * PS::RS];
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
          for (int k = 0; k < JPP; ++k) {
            float* pv = scr + l15 * PS::RS + 32 * k + 8 * q;
            *reinterpret_cast<f32x4*>(pv) = hv[2 * k];
            *reinterpret_cast<f32x4*>(pv + 4) = hv[2 * k + 1];
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (PS::PW >= 32 || lane < PS::PW) {
#pragma unroll
            for (int r = 0; r < NR; ++r) tq += pr[r * PS::RS];
          }
          st_s[jj / JPP] += (double)ts;
          st_q[jj / JPP] += (double)tq;
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
      }
      if constexpr (STATS == 1) {
        // the 16 x PW block of this pass goes through the wave's scratch: written as it lies (row = position, 8 consecutive
        // channels per lane; rows past the slab as zeros), read back one COLUMN per lane — LDS operations of one wave complete in
        // order, so a wait on the counter is the only synchronisation; no cross-lane traffic, 8 accumulator registers per pass
        constexpr int JPP = PS::PW / 32;  // jj's per pass
        const int jl = jj % JPP;
        if (!t.ok) o0 = o1 = f32x4{0.f, 0.f, 0.f, 0.f};
        float* pw_ = scr + l15 * PS::RS + 32 * jl + 8 * q;
        *reinterpret_cast<f32x4*>(pw_) = o0;
        *reinterpret_cast<f32x4*>(pw_ + 4) = o1;
        if (jl == JPP - 1) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          constexpr int NR = PS::PW == 64 ? 16 : 8;
          const float* pr = scr + (PS::PW == 64 ? lane : (lane & 31) + (lane >> 5) * 8 * PS::RS);
          float ts = 0.f, tq = 0.f;
          if (PS::PW >= 32 || lane < PS::PW) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
              const float v = pr[r * PS::RS];
              ts += v;
              tq += v * v;
            }
          }
          st_s[jj / JPP] += (double)ts;
          st_q[jj / JPP] += (double)tq;
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the reads are done before the next pass overwrites the block)
        }
      }
    }
    };
    mfma_part();
    epilogue();
  }
  if constexpr (STATS != 0) {  // this wave's row of partials: channel c0 + PW * pass + column
    const int C = a.n_total, q4 = C / 4, nq = q4 < 256 ? q4 : 256, unit = q4 > 256 ? q4 / 256 : 1;
    const size_t row = ((size_t)blockIdx.y * a.n_rg + rg) * PX_NW + wid;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      double s0 = st_s[ps], s1 = st_q[ps];
      if (PS::PW == 32) {  // the two row halves of a 32-wide pass meet here
        s0 += __shfl_xor(s0, 32, 64);
        s1 += __shfl_xor(s1, 32, 64);
      }
      if (lane < PS::PW) {
        const int c = c0 + ps * PS::PW + lane, quad = c >> 2, e = c & 3;
        if constexpr (STATS == 2) s1 *= (double)a.bst_invstd[(size_t)blockIdx.y * C + c];  // sum of g * (x - mean) -> of g * xhat
        double* dst = a.stat_part + (row * unit + (quad >> 8)) * nq * 8 + (size_t)(quad % nq) * 8 + e;
        dst[0] = s0;
        dst[4] = s1;
      }
    }
  }
}

// row groups (persistent workgroups along the rows) of one launch: as many workgroups as stay resident, over `groups` slabs
int pf_row_groups(int lds_bytes, int n_chunks, int ntiles, int groups) {
  const int per_cu = lds_bytes > 80 * 1024 ? 1 : (lds_bytes > 52 * 1024 ? 2 : 3);
  int n_rg = (256 * per_cu) / (n_chunks * groups);
  n_rg = n_rg < 8 ? 8 : (n_rg / 8) * 8;
  const int max_rg = (ntiles + PX_NW - 1) / PX_NW;
  if (n_rg > ((max_rg + 7) / 8) * 8) n_rg = ((max_rg + 7) / 8) * 8;
  return n_rg;
}

template <int K1S, int NT1>
constexpr int pf_lds_bytes(int stats) {  // 0 none, 1 forward statistics, 2 backward (+ the coefficient table)
  return 2 * NT1 * K1S * 1024 + NT1 * 16 * 4 + (stats ? PfStat<K1S, NT1>::BYTES : 0) + (stats == 2 ? 3 * NT1 * 16 * 4 : 0);
}

// ---- the instances ----------------------------------------------------------------------------------------------------------------
// A kernel family's instances are its K steps x the tiles per workgroup chunk that fit beside them (`fits`).  The two lists below
// are the only place that names them: the `*_supported` answers, the LDS-bytes query and the dispatch all walk them, and nothing
// else is instantiated.
constexpr int TILES[] = {16, 8, 4, 2};  // widest first
constexpr bool fits(int k1s, int t) { return 2 * t * k1s <= 128; }  // both planes' fragments within 128 KB of LDS

enum : unsigned { POINTWISE = 1, LATERAL = 2 };  // the entries that may ask for a K step
struct KStep {
  int k1s;
  unsigned users;
};
struct PxSteps {  // pw_x3_kernel
  static constexpr KStep at[] = {{1, POINTWISE}, {2, POINTWISE | LATERAL}, {3, POINTWISE}, {4, POINTWISE},  {5, POINTWISE},
                                 {7, LATERAL},   {8, POINTWISE},           {10, POINTWISE}, {14, LATERAL}, {16, POINTWISE}};
};
struct PfSteps {  // pw_x3_f32_kernel
  static constexpr KStep at[] = {{1, POINTWISE}, {2, POINTWISE}, {4, POINTWISE}, {8, POINTWISE}};
};

// tiles per workgroup chunk for (K1S, N): the widest of 16 / 8 / 4 / 2 that divides N/16 and keeps both planes' fragments
// within 128 KB of LDS; 0 = unsupported
int pick_nt1(int k1s, int n) {
  if (n % 32) return 0;
  const int nt = n / 16;
  for (int t : TILES)
    if (nt % t == 0 && fits(k1s, t)) return t;
  return 0;
}

// a layer of n outputs over k inputs that `user` may run on the family
template <class Steps>
int layer_supported(int k, int n, unsigned user) {
  const int k1s = (k + 31) / 32;
  bool listed = false;
  for (const KStep& s : Steps::at) listed |= s.k1s == k1s && (s.users & user) != 0;
  if (k % 8 || !listed) return 0;
  const int nt1 = pick_nt1(k1s, n);
  return (nt1 && n / (16 * nt1) <= 8) ? 1 : 0;  // more than 8 channel chunks re-read the input too often: the general tile is better
}

constexpr int NO_INSTANCE = INT_MIN;

template <int K1S, int NT1, class F>
bool try_instance(int k1s, int nt1, int& rc, F& f) {
  if constexpr (fits(K1S, NT1)) {
    if (k1s == K1S && nt1 == NT1) {
      rc = f(std::integral_constant<int, K1S>{}, std::integral_constant<int, NT1>{});
      return true;
    }
  }
  return false;
}

template <class Steps, class F, size_t... I>
int with_instance(int k1s, int nt1, F& f, std::index_sequence<I...>) {
  int rc = NO_INSTANCE;
  (void)(try_instance<Steps::at[I / std::size(TILES)].k1s, TILES[I % std::size(TILES)]>(k1s, nt1, rc, f) || ...);
  return rc;
}

// f(K1S, NT1), the two as integral constants, of the family's instance (k1s, nt1); NO_INSTANCE if it has none
template <class Steps, class F>
int with_instance(int k1s, int nt1, F f) {
  return with_instance<Steps>(k1s, nt1, f, std::make_index_sequence<std::size(Steps::at) * std::size(TILES)>{});
}

int no_instance(const char* who, int k1s, int nt1) {
  avt::set_error("%s: no kernel for K steps %d, tiles %d", who, k1s, nt1);
  return AVT_ERR_UNSUPPORTED;
}

// LDS bytes of the (K1S, NT1) instance, for the row-group queries (avt_pw_x3_f32_stat_rows, avt_pw_x3_f32_bwdstats_rows)
int pf_lds_of(int k1s, int nt1, int stats) {
  const int bytes = with_instance<PfSteps>(k1s, nt1, [&](auto k, auto t) { return pf_lds_bytes<k(), t()>(stats); });
  return bytes == NO_INSTANCE ? 0 : bytes;
}

// STATS != 0: blockIdx.y = the BatchNorm's replica group, a.M / a.ntiles per group
template <int K1S, int NT1, bool F16, int STATS>
int launch_pf(PfArgs& a, hipStream_t st, int groups) {
  constexpr int lds_bytes = pf_lds_bytes<K1S, NT1>(STATS);
  static_assert(lds_bytes <= 160 * 1024, "weights + the statistics scratch fit the LDS");
  a.n_rg = pf_row_groups(lds_bytes, a.n_chunks, a.ntiles, groups);
  return avt::launch<pw_x3_f32_kernel<K1S, NT1, F16, STATS>>(STATS ? "avt_pw_x3_f32_stats" : "avt_pw_x3_f32",
                                                             dim3((unsigned)(a.n_rg * a.n_chunks), (unsigned)groups), dim3(PX_NW * 64), lds_bytes,
                                                             lds_bytes, st, a);
}

// The one place where the run-time choices of the training form become template arguments: the instance, the plane type, and the
// mode (stats: 0 plain — one group —, 1 forward statistics, 2 backward).  Mode 2 has bf16 planes (gradients) and at most 8 tiles.
int run_pf(PfArgs& a, int k1s, int nt1, int plane_dtype, int stats, int groups, hipStream_t st) {
  const bool f16 = plane_dtype == AVT_X3_F16;
  if (stats == 2 && f16) {
    avt::set_error("avt_pw_x3_f32_bwdstats: bf16 planes only");
    return AVT_ERR_UNSUPPORTED;
  }
  const int rc = with_instance<PfSteps>(k1s, nt1, [&](auto k, auto t) {
    constexpr int K1S = k(), NT1 = t();
    if (stats == 2) {
      if constexpr (NT1 < 16) return launch_pf<K1S, NT1, false, 2>(a, st, groups);
      return NO_INSTANCE;
    }
    if (stats == 1) return f16 ? launch_pf<K1S, NT1, true, 1>(a, st, groups) : launch_pf<K1S, NT1, false, 1>(a, st, groups);
    return f16 ? launch_pf<K1S, NT1, true, 0>(a, st, 1) : launch_pf<K1S, NT1, false, 0>(a, st, 1);
  });
  return rc == NO_INSTANCE ? no_instance("avt_pw_x3_f32", k1s, nt1) : rc;
}

template <int K1S, int NT1, bool F16>
int launch_px(PxArgs& a, hipStream_t st) {
  constexpr int lds_bytes = 2 * NT1 * K1S * 1024 + 2 * NT1 * 16 * 4;
  // persistent workgroups: as many as stay resident (LDS-limited), split into row groups x channel chunks
  a.n_rg = pf_row_groups(lds_bytes, a.n_chunks, a.ntiles, 1);  // a multiple of 8: blocks of one XCD (b % 8) form whole row groups
  return avt::launch<pw_x3_kernel<K1S, NT1, F16>>("avt_pw_x3", dim3((unsigned)(a.n_rg * a.n_chunks)), dim3(PX_NW * 64), lds_bytes, lds_bytes,
                                                  st, a);
}

// ... and of the plane-pair form
int run_px(PxArgs& a, int k1s, int nt1, int plane_dtype, hipStream_t st) {
  const bool f16 = plane_dtype == AVT_X3_F16;
  const int rc = with_instance<PxSteps>(
      k1s, nt1, [&](auto k, auto t) { return f16 ? launch_px<k(), t(), true>(a, st) : launch_px<k(), t(), false>(a, st); });
  return rc == NO_INSTANCE ? no_instance("avt_pw_x3", k1s, nt1) : rc;
}

// The fields the PxArgs users share: a pointwise layer of n columns (nt1 tiles per chunk) over m rows.  The lateral and the chained
// entries then set what differs.
void px_fill(PxArgs& a, const void* x_hi, const void* x_lo, int ldx, int k, const void* w_hi, const void* w_lo, const float* bias,
             const float* wscale, const void* res_hi, const void* res_lo, int ldr, void* y_hi, void* y_lo, int ldy, int n, int nt1,
             int64_t m, int relu) {
  a.xh = static_cast<const uint16_t*>(x_hi);
  a.xl = static_cast<const uint16_t*>(x_lo);
  a.rh = static_cast<const uint16_t*>(res_hi);
  a.rl = static_cast<const uint16_t*>(res_lo);
  a.yh = static_cast<uint16_t*>(y_hi);
  a.yl = static_cast<uint16_t*>(y_lo);
  a.wh = static_cast<const i32x4*>(w_hi);
  a.wl = static_cast<const i32x4*>(w_lo);
  a.bias = bias;
  a.wscale = wscale;
  a.M = (int)m;
  a.ldx = ldx;
  a.ldr = ldr;
  a.ldy = ldy;
  a.k1c = k / 8;
  a.ntiles = (int)((m + 15) / 16);
  a.relu = relu;
  a.n_chunks = n / (16 * nt1);
  a.n_rg = 0;  // (launch_px)
  a.taps = 1;
  a.cin8 = a.T = a.To = a.HW = a.tst = a.tpad = 0;
  a.n_valid = n;
}

// ... and the PfArgs users: `rows` = the rows of one launch slab (all of them, or one BatchNorm group's); no backward statistics
void pf_fill(PfArgs& a, const float* x, int ldx, int k, const void* w_hi, const void* w_lo, const float* wscale, const float* add, int lda,
             float* y, int ldy, int n, int nt1, int rows, void* stat_part) {
  a.x = x; a.add = add; a.y = y;
  a.wh = static_cast<const uint16_t*>(w_hi);
  a.wl = static_cast<const uint16_t*>(w_lo);
  a.wscale = wscale;
  a.M = rows; a.ldx = ldx; a.lda = lda; a.ldy = ldy; a.K = k; a.k1c = k / 8;
  a.ntiles = (rows + 15) / 16;
  a.n_chunks = n / (16 * nt1);
  a.stat_part = static_cast<double*>(stat_part);
  a.n_total = n;
  a.bst_x = nullptr;
}

}  // namespace

extern "C" int avt_pw_x3_supported(int k, int n) { return layer_supported<PxSteps>(k, n, POINTWISE); }

extern "C" int avt_pw_x3(const void* x_hi, const void* x_lo, int ldx, int k, const void* w_hi, const void* w_lo, const float* bias,
                         const float* wscale, const void* res_hi, const void* res_lo, int ldr, void* y_hi, void* y_lo, int ldy,
                         int n, int64_t m, int relu, int plane_dtype, void* stream) {
  AVT_REQUIRE(x_hi && x_lo && w_hi && w_lo && y_hi && y_lo && (!res_hi == !res_lo), "avt_pw_x3: NULL pointer / half a plane pair");
  AVT_REQUIRE(avt_pw_x3_supported(k, n), "avt_pw_x3: unsupported layer K=%d N=%d", k, n);
  AVT_REQUIRE(m > 0 && m < (1ll << 31) - 16 && ldx >= k && ldy >= n && ldx % 8 == 0 && ldy % 8 == 0 && (!res_hi || (ldr >= n && ldr % 8 == 0)),
              "avt_pw_x3: bad sizes / leading dimensions");
  AVT_REQUIRE(avt::aligned16(x_hi) && avt::aligned16(x_lo) && avt::aligned16(w_hi) && avt::aligned16(w_lo) && avt::aligned16(y_hi) &&
                  avt::aligned16(y_lo) && (!res_hi || (avt::aligned16(res_hi) && avt::aligned16(res_lo))) &&
                  (!bias || avt::aligned16(bias)) && (!wscale || avt::aligned16(wscale)),
              "avt_pw_x3: pointers must be 16-byte aligned");
  AVT_REQUIRE(plane_dtype == AVT_X3_BF16 || plane_dtype == AVT_X3_F16, "avt_pw_x3: bad plane_dtype");
  const int k1s = (k + 31) / 32, nt1 = pick_nt1(k1s, n);
  PxArgs a;
  px_fill(a, x_hi, x_lo, ldx, k, w_hi, w_lo, bias, wscale, res_hi, res_lo, ldr, y_hi, y_lo, ldy, n, nt1, m, relu);
  return run_px(a, k1s, nt1, plane_dtype, static_cast<hipStream_t>(stream));
}

// Conv3d [kt,1,1], temporal stride st, padding pt, on plane pairs: the lateral fast -> slow connections (FuseFastToSlow: [7,1,1]
// stride 4 + BN + ReLU of the third-party SlowFast model the reference runs per clip window, models/models.py:335, 399)
extern "C" int avt_lateral_x3_supported(int cin, int cout, int kt) {
  if (cin % 8 || kt < 2 || cout % 16) return 0;
  return layer_supported<PxSteps>(kt * cin, (cout + 31) / 32 * 32, LATERAL);
}

extern "C" int avt_lateral_x3(const void* x_hi, const void* x_lo, int ldx, int cin, const void* w_hi, const void* w_lo, const float* bias,
                              const float* wscale, void* y_hi, void* y_lo, int ldy, int cout, int batch, int t, int hw, int kt, int st,
                              int pt, int relu, int plane_dtype, void* stream) {
  AVT_REQUIRE(x_hi && x_lo && w_hi && w_lo && y_hi && y_lo, "avt_lateral_x3: NULL pointer");
  AVT_REQUIRE(avt_lateral_x3_supported(cin, cout, kt), "avt_lateral_x3: unsupported layer Cin=%d Cout=%d kt=%d", cin, cout, kt);
  AVT_REQUIRE(batch > 0 && t > 0 && hw > 0 && st > 0 && pt >= 0 && pt < kt && ldx >= cin && ldy >= cout && ldx % 8 == 0 && ldy % 8 == 0,
              "avt_lateral_x3: bad sizes / leading dimensions");
  AVT_REQUIRE(avt::aligned16(x_hi) && avt::aligned16(x_lo) && avt::aligned16(w_hi) && avt::aligned16(w_lo) && avt::aligned16(y_hi) &&
                  avt::aligned16(y_lo) && (!bias || avt::aligned16(bias)) && (!wscale || avt::aligned16(wscale)),
              "avt_lateral_x3: pointers must be 16-byte aligned");
  AVT_REQUIRE(plane_dtype == AVT_X3_BF16 || plane_dtype == AVT_X3_F16, "avt_lateral_x3: bad plane_dtype");
  const int to = (t + 2 * pt - kt) / st + 1;
  const int64_t m = (int64_t)batch * to * hw;
  AVT_REQUIRE(to > 0 && m < (1ll << 31) - 16, "avt_lateral_x3: no output frames / too many rows");
  const int k = kt * cin, k1s = (k + 31) / 32, n = (cout + 31) / 32 * 32, nt1 = pick_nt1(k1s, n);
  PxArgs a;
  // (weights: fused_slowfast.pack_pw_planes over the conv's own [Cout (padded to 32), kt * Cin] rows; bias [n], padded with them)
  px_fill(a, x_hi, x_lo, ldx, k, w_hi, w_lo, bias, wscale, nullptr, nullptr, 0, y_hi, y_lo, ldy, n, nt1, m, relu);
  a.taps = kt;
  a.cin8 = cin / 8;
  a.T = t;
  a.To = to;
  a.HW = hw;
  a.tst = st;
  a.tpad = pt;
  a.n_valid = cout;
  return run_px(a, k1s, nt1, plane_dtype, static_cast<hipStream_t>(stream));
}

// (k1, n1, n2) of the chained form: the slow res2 pair 64 -> 256 (+ residual) -> 64
extern "C" int avt_pw_chain_x3_supported(int k1, int n1, int n2) { return (k1 == 64 && n1 == 256 && n2 == 64) ? 1 : 0; }

extern "C" int avt_pw_chain_x3(const void* x_hi, const void* x_lo, int ldx, int k1, const void* w1_hi, const void* w1_lo, const float* bias1,
                               const float* wscale1, const void* res_hi, const void* res_lo, int ldr, void* y_hi, void* y_lo, int ldy,
                               int n1, int relu1, const void* w2_hi, const void* w2_lo, const float* bias2, const float* wscale2,
                               void* z_hi, void* z_lo, int ldz, int n2, int64_t m, int plane_dtype, void* stream) {
  AVT_REQUIRE(x_hi && x_lo && w1_hi && w1_lo && y_hi && y_lo && w2_hi && w2_lo && z_hi && z_lo && (!res_hi == !res_lo),
              "avt_pw_chain_x3: NULL pointer / half a plane pair");
  AVT_REQUIRE(avt_pw_chain_x3_supported(k1, n1, n2), "avt_pw_chain_x3: unsupported pair K1=%d N1=%d N2=%d (64 -> 256 -> 64)", k1, n1, n2);
  AVT_REQUIRE(m > 0 && m < (1ll << 31) - 16 && ldx >= k1 && ldy >= n1 && ldz >= n2 && ldx % 8 == 0 && ldy % 8 == 0 && ldz % 8 == 0 &&
                  (!res_hi || (ldr >= n1 && ldr % 8 == 0)),
              "avt_pw_chain_x3: bad sizes / leading dimensions");
  AVT_REQUIRE(avt::aligned16(x_hi) && avt::aligned16(x_lo) && avt::aligned16(w1_hi) && avt::aligned16(w1_lo) && avt::aligned16(y_hi) &&
                  avt::aligned16(y_lo) && avt::aligned16(w2_hi) && avt::aligned16(w2_lo) && avt::aligned16(z_hi) && avt::aligned16(z_lo) &&
                  (!res_hi || (avt::aligned16(res_hi) && avt::aligned16(res_lo))) && (!bias1 || avt::aligned16(bias1)) &&
                  (!wscale1 || avt::aligned16(wscale1)) && (!bias2 || avt::aligned16(bias2)) && (!wscale2 || avt::aligned16(wscale2)),
              "avt_pw_chain_x3: pointers must be 16-byte aligned");
  AVT_REQUIRE(plane_dtype == AVT_X3_BF16 || plane_dtype == AVT_X3_F16, "avt_pw_chain_x3: bad plane_dtype");
  PcArgs c;
  constexpr int K1S = 2, NT1 = 16, NT2 = 4;
  px_fill(c.p, x_hi, x_lo, ldx, k1, w1_hi, w1_lo, bias1, wscale1, res_hi, res_lo, ldr, y_hi, y_lo, ldy, n1, NT1, m, relu1);  // one chunk
  c.w2h = static_cast<const i32x4*>(w2_hi);
  c.w2l = static_cast<const i32x4*>(w2_lo);
  c.bias2 = bias2;
  c.wscale2 = wscale2;
  c.zh = static_cast<uint16_t*>(z_hi);
  c.zl = static_cast<uint16_t*>(z_lo);
  c.ldz = ldz;
  constexpr int lds_bytes = 2 * NT1 * K1S * 1024 + 2 * NT2 * (NT1 / 2) * 1024 + (2 * NT1 * 16 + 2 * NT2 * 16) * 4;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int grid = (c.p.ntiles + PX_NW - 1) / PX_NW;
  if (grid > 256) grid = 256;  // persistent: one workgroup per CU (129 KB of fragments)
  const dim3 block(PX_NW * 64);
  if (plane_dtype == AVT_X3_F16)
    return avt::launch<pw_chain_x3_kernel<K1S, NT1, NT2, true>>("avt_pw_chain_x3", dim3((unsigned)grid), block, lds_bytes, lds_bytes, st, c);
  return avt::launch<pw_chain_x3_kernel<K1S, NT1, NT2, false>>("avt_pw_chain_x3", dim3((unsigned)grid), block, lds_bytes, lds_bytes, st, c);
}

// The training form of avt_pw_x3 (see include/avt.h): fp32 rows in / out, plain [n][k] weight planes
extern "C" int avt_pw_x3_f32_supported(int k, int n) { return layer_supported<PfSteps>(k, n, POINTWISE); }

extern "C" int avt_pw_x3_f32(const float* x, int ldx, int k, const void* w_hi, const void* w_lo, const float* wscale, const float* add,
                             int lda, float* y, int ldy, int n, int64_t m, int plane_dtype, void* stream) {
  AVT_REQUIRE(x && w_hi && w_lo && y, "avt_pw_x3_f32: NULL pointer");
  AVT_REQUIRE(avt_pw_x3_f32_supported(k, n), "avt_pw_x3_f32: unsupported layer K=%d N=%d", k, n);
  AVT_REQUIRE(m > 0 && m < (1ll << 31) - 16 && ldx >= k && ldy >= n && ldx % 4 == 0 && ldy % 4 == 0 && (!add || (lda >= n && lda % 4 == 0)),
              "avt_pw_x3_f32: bad sizes / leading dimensions");
  AVT_REQUIRE(avt::aligned16(x) && avt::aligned16(w_hi) && avt::aligned16(w_lo) && avt::aligned16(y) && (!add || avt::aligned16(add)) &&
                  (!wscale || avt::aligned16(wscale)),
              "avt_pw_x3_f32: pointers must be 16-byte aligned");
  AVT_REQUIRE(plane_dtype == AVT_X3_BF16 || plane_dtype == AVT_X3_F16, "avt_pw_x3_f32: bad plane_dtype");
  const int k1s = (k + 31) / 32, nt1 = pick_nt1(k1s, n);
  PfArgs a;
  pf_fill(a, x, ldx, k, w_hi, w_lo, wscale, add, lda, y, ldy, n, nt1, (int)m, nullptr);
  return run_pf(a, k1s, nt1, plane_dtype, 0, 1, static_cast<hipStream_t>(stream));
}

// ... leaving the train-mode BatchNorm statistics of its output behind (include/avt.h; the streaming counterpart of
// avt_conv3d_igemm_x3_f32_stats): rows of partials per group = 8 x the row groups of the launch
extern "C" int avt_pw_x3_f32_stat_rows(int k, int n, int64_t m, int groups) {
  if (!avt_pw_x3_f32_supported(k, n) || groups < 1 || m <= 0 || m % groups) return -1;
  const int k1s = (k + 31) / 32, nt1 = pick_nt1(k1s, n);
  const int ntiles = (int)((m / groups + 15) / 16);
  return pf_row_groups(pf_lds_of(k1s, nt1, 1), n / (16 * nt1), ntiles, groups) * PX_NW;
}

extern "C" int avt_pw_x3_f32_stats(const float* x, int ldx, int k, const void* w_hi, const void* w_lo, const float* wscale, float* y, int ldy,
                                   int n, int64_t m, int plane_dtype, void* stat_part, int groups, void* stream) {
  AVT_REQUIRE(x && w_hi && w_lo && y && stat_part, "avt_pw_x3_f32_stats: NULL pointer");
  AVT_REQUIRE(avt_pw_x3_f32_supported(k, n), "avt_pw_x3_f32_stats: unsupported layer K=%d N=%d", k, n);
  AVT_REQUIRE(groups >= 1 && groups <= 65535 && m > 0 && m % groups == 0 && m < (1ll << 31) - 16 && ldx >= k && ldy >= n && ldx % 4 == 0 &&
                  ldy % 4 == 0 && n >= 8 && (n & (n - 1)) == 0 && n <= 4096,
              "avt_pw_x3_f32_stats: bad sizes / leading dimensions / groups (n a power of two: the BatchNorm's domain)");
  AVT_REQUIRE(avt::aligned16(x) && avt::aligned16(w_hi) && avt::aligned16(w_lo) && avt::aligned16(y) && avt::aligned16(stat_part) &&
                  (!wscale || avt::aligned16(wscale)),
              "avt_pw_x3_f32_stats: pointers must be 16-byte aligned");
  AVT_REQUIRE(plane_dtype == AVT_X3_BF16 || plane_dtype == AVT_X3_F16, "avt_pw_x3_f32_stats: bad plane_dtype");
  const int k1s = (k + 31) / 32, nt1 = pick_nt1(k1s, n);
  PfArgs a;
  pf_fill(a, x, ldx, k, w_hi, w_lo, wscale, nullptr, 0, y, ldy, n, nt1, (int)(m / groups), stat_part);
  return run_pf(a, k1s, nt1, plane_dtype, 1, groups, static_cast<hipStream_t>(stream));
}

// The streaming input gradient whose result is a train-mode BatchNorm's OUTPUT gradient (include/avt.h; the counterpart of
// avt_conv3d_igemm_x3_f32_bwdstats for the pointwise layers)
extern "C" int avt_pw_x3_f32_bwdstats_rows(int k, int n, int64_t m, int groups) {
  if (!avt_pw_x3_f32_supported(k, n) || groups < 1 || m <= 0 || m % groups || n < 8 || (n & (n - 1)) || n > 4096) return -1;
  int k1s = (k + 31) / 32, nt1 = pick_nt1(k1s, n);
  if (nt1 == 16) nt1 = 8;  // (as the launch below)
  const int ntiles = (int)((m / groups + 15) / 16);
  return pf_row_groups(pf_lds_of(k1s, nt1, 2), n / (16 * nt1), ntiles, groups) * PX_NW;
}

extern "C" int avt_pw_x3_f32_bwdstats(const float* x, int ldx, int k, const void* w_hi, const void* w_lo, const float* add, int lda, float* y,
                                      int ldy, int n, int64_t m, int plane_dtype, const float* bn_x, const float* bn_mean,
                                      const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const void* bn_mask, int relu,
                                      void* stat_part, int groups, void* stream) {
  AVT_REQUIRE(x && w_hi && w_lo && y && stat_part && bn_x && bn_mean && bn_invstd && bn_gamma, "avt_pw_x3_f32_bwdstats: NULL pointer");
  AVT_REQUIRE(avt_pw_x3_f32_bwdstats_rows(k, n, m, groups) > 0, "avt_pw_x3_f32_bwdstats: unsupported layer K=%d N=%d / %lld rows in %d groups",
              k, n, (long long)m, groups);
  AVT_REQUIRE(m < (1ll << 31) - 16 && ldx >= k && ldy == n && ldx % 4 == 0 && (!add || (lda >= n && lda % 4 == 0)) &&
                  (!relu || bn_mask || bn_beta) && plane_dtype == AVT_X3_BF16,
              "avt_pw_x3_f32_bwdstats: contiguous output rows (ldy == n), bf16 planes, a mask or beta for the ReLU");
  AVT_REQUIRE(avt::aligned16(x) && avt::aligned16(w_hi) && avt::aligned16(w_lo) && avt::aligned16(y) && avt::aligned16(stat_part) &&
                  avt::aligned16(bn_x) && (!add || avt::aligned16(add)),
              "avt_pw_x3_f32_bwdstats: pointers must be 16-byte aligned");
  int k1s = (k + 31) / 32, nt1 = pick_nt1(k1s, n);
  // (16 tiles per wave spill 13-84 registers in this mode, and a scratch reload's s_waitcnt vmcnt(0) serializes the tile's loads: 8
  //  tiles and twice the chunks — the dy rows read twice, a small operand here — are 10 % (K = 64) to 27 % (K = 128) faster)
  //  tiles and twice the chunks — the dy rows read twice, a small operand here — are 10 % (K = 64) to 27 % (K = 128) faster.  The
  //  16 tiles split in two halves, the second half's operands requested under its MFMAs, were tried first: that form is in the
  //  history, in this file at the parent of the commit that removed it)
  if (nt1 == 16) nt1 = 8;
  PfArgs a;
  pf_fill(a, x, ldx, k, w_hi, w_lo, nullptr, add, lda, y, ldy, n, nt1, (int)(m / groups), stat_part);
  a.bst_x = bn_x; a.bst_mean = bn_mean; a.bst_invstd = bn_invstd; a.bst_gamma = bn_gamma; a.bst_beta = bn_beta;
  a.bst_mask = static_cast<const uint8_t*>(bn_mask); a.bst_relu = relu;
  return run_pf(a, k1s, nt1, plane_dtype, 2, groups, static_cast<hipStream_t>(stream));
}
