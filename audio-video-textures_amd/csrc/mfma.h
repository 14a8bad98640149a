// What every matrix-pipe kernel here has to agree on: the operand types, which MFMA instruction a plane type selects, the
// order of the three terms of a split-plane product, the buffer-resource flags, the transposed LDS read that yields an
// operand, and the non-temporal 16-byte access.  (The 2-wide types bf16x2 / f16x2 / f32x2 are in avt_common.h, with the
// packed conversions that use them.)
#pragma once
#include "avt_common.h"

namespace avt {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// One MFMA on operands held as four dwords (eight 16-bit values of one plane).  F16 = true: fp16 planes, false: bf16 planes
// (and the bf16-only kernels).  v_mfma_f32_16x16x32_{f16,bf16} / v_mfma_f32_32x32x16_{f16,bf16}, fp32 accumulate.
template <bool F16>
__device__ __forceinline__ f32x4 mfma16(i32x4 w, i32x4 x, f32x4 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, x), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ f32x16 mfma32(i32x4 w, i32x4 x, f32x16 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, x), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), c, 0, 0, 0);
}

// One split-plane product (w = wh + wl, x = xh + xl) into one fp32 accumulator: wl*xh, then wh*xl, then wh*xh — the two small
// terms first, the large one last (conv_x3.hip's order; wl*xl is below the split's own error and is never formed).  The order is
// part of the arithmetic: fp32 addition does not associate, another order gives other bits.  A kernel that writes the three
// passes out itself, interleaved over several accumulators, keeps this order per accumulator.
template <bool F16>
__device__ __forceinline__ f32x4 mfma3(i32x4 wh, i32x4 wl, i32x4 xh, i32x4 xl, f32x4 c) {
  c = mfma16<F16>(wl, xh, c);
  c = mfma16<F16>(wh, xl, c);
  return mfma16<F16>(wh, xh, c);
}

// Raw buffer resource over `bytes` bytes at p (stride 0, so the record count is a byte count).  The hardware checks every
// access through it against that count: a load at an offset outside [0, bytes) returns zeros and a store there is dropped —
// the kernels rely on both (padding read as "hardware zero fill", always-issued stores with an out-of-bounds offset).
// kBufferRsrcFlags is the last word of the descriptor; it is the value of the buffer-load recipe for gfx950
// (cdna_hip_programming.md T8) and the one every kernel here has always used — its fields are not decoded here.
// Build a resource from wave-uniform values only.
constexpr int kBufferRsrcFlags = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, kBufferRsrcFlags);
}

// One MFMA operand (eight 16-bit values along K) out of an LDS image that holds K along the rows: two transposed 8-byte reads
// (ds_read_b64_tr_b16) at byte offsets a0 and a1.
__device__ __forceinline__ i32x4 lds_tr_frag(const char* lds, int a0, int a1) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const uint2 u = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + a0)));
  const uint2 v = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + a1)));
  return i32x4{(int)u.x, (int)u.y, (int)v.x, (int)v.y};
}

// Non-temporal 16-byte accesses for data that is streamed once (tensors far larger than the caches).  The three-argument
// forms index p in 16-byte units: i counts float4s, not floats.
__device__ __forceinline__ void stg4(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }
__device__ __forceinline__ float4 ldg4(const float* p, int64_t i) {
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void stg4(float* p, int64_t i, float4 v) {
  __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(p) + i);
}

}  // namespace avt
