// The f16x3 plane split and its companions: the ONE home of the device helpers every MFMA kernel file shares.  Included after
// magat_common.h, at file scope or inside a file's anonymous namespace (block_walk.h is included inside one).
//
// "f16x3": x ~ h1 + h2, two RNE half planes = 22 significand bits; a product keeps h1g1 + h1g2 + h2g1, dropping
// h2g2 <= 2^-22 |xw|: THREE v_mfma_f32_32x32x16_f16 per product instead of six bf16 ones.  fp16 has the narrow exponent, so
// the clamping splits keep activations within +-65504 per plane (values up to 1.3e5 stay exact through the second plane;
// larger ones saturate - unreachable for this network) and residuals below 6e-5 go subnormal (absolute error <= 3e-8, the
// fp32 spacing of values near 0.5); weights are pre-scaled by a power of two so that both planes are normal numbers (the
// scale is undone in the epilogue).
//
// The latency forms are bit-identical to the batched forms because they execute THESE instruction sequences
// (tests/test_gpu_latency.py): a kernel file never writes its own copy (tests/test_host_sources.py).  Two variants become one
// only if every kernel that used either keeps its device assembly (tools/isa_same.py); otherwise both stay here under two names.
#pragma once

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;

// barrier for LDS hand-overs only: __syncthreads() carries s_waitcnt vmcnt(0) in its release fence and would wait for every
// global load in flight (weight prefetches, the next group's input, Y stores)
#define MAGAT_LDS_SYNC() do { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); } while (0)

// A lone wave issues in order: vector work only runs under the matrix pipe when MFMAs and vector instructions ALTERNATE in
// the instruction stream.  This fences the scheduler: what is written between two fences stays between them.
#define MAGAT_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ f32x16 mfma16(const uint4& a, const uint4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ---- the core, asm form: value pair -> its two f16 planes: hi = rne(v) (v_cvt_pk_f16_f32), lo = rne(v - hi).  No range clamp:
// a value beyond the f16 range turns into inf / nan planes.
__device__ __forceinline__ void f16x3_split(float x, float y, unsigned& p1, unsigned& p2) {
  const f16x2 h = __builtin_convertvector(f32x2{x, y}, f16x2);
  p1 = __builtin_bit_cast(unsigned, h);
  // residual x - hi: one mixed-precision fma per value (fma(hi, -1, x), exact; the f16 operand read from its half of the
  // packed register) - not two conversions + v_pk_add_f32: packed fp32 instructions do not issue while an MFMA runs
  // (tools/exp/mfma_valu.hip), and the loaders split while other waves of the SIMD multiply.  (v_fma_mixlo_f16 /
  // v_fma_mixhi_f16 - the same fma with the conversion folded in, two instructions per pair instead of three - was measured in
  // round 4: chain kernel 1900 -> 1904 us, stem 165 -> 169 us same-box: not cheaper.)
  float rx, ry;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(rx) : "v"(p1), "v"(x));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(ry) : "v"(p1), "v"(y));
  const f16x2 r = __builtin_convertvector(f32x2{rx, ry}, f16x2);
  p2 = __builtin_bit_cast(unsigned, r);
}
// ---- the core, compiler-visible form (same planes: value = p1 + p2 to 22 bits).  Compiler-visible conversions only: an asm
// statement reading a register an MFMA has just written gets none of the wait states the hazard recognizer inserts (round 6,
// gat_csr_fused.hip).  For splits of accumulators straight behind their MFMA (gat_mid.hip).
__device__ __forceinline__ void f16x3_split_cv(float x, float y, unsigned& p1, unsigned& p2) {
  const f16x2 h = __builtin_convertvector(f32x2{x, y}, f16x2);
  p1 = __builtin_bit_cast(unsigned, h);
  const f32x2 back = __builtin_convertvector(h, f32x2);
  const f16x2 r = __builtin_convertvector(f32x2{x - back[0], y - back[1]}, f16x2);
  p2 = __builtin_bit_cast(unsigned, r);
}

// ---- no clamp, `vmax` keeps the running maximum of |v|: the caller raises the range flag from it, which makes the float32
// form re-write every output of the launch
__device__ __forceinline__ void f16x3_split_absmax(float x, float y, unsigned& p1, unsigned& p2, float& vmax) {
  vmax = fmaxf(fmaxf(vmax, fabsf(x)), fabsf(y));
  f16x3_split(x, y, p1, p2);
}
__device__ __forceinline__ void f16x3_split_cv_absmax(float x, float y, unsigned& p1, unsigned& p2, float& vmax) {
  vmax = fmaxf(fmaxf(vmax, fabsf(x)), fabsf(y));
  f16x3_split_cv(x, y, p1, p2);
}

// ---- signed values (inputs, weights, pre-activation maps) clamped to +-65504
__device__ __forceinline__ void f16x3_split_clamp(float x, float y, unsigned& p1, unsigned& p2) {
  // one v_med3_f32 per value (fminf(fmaxf()) costs an extra canonicalising v_max each)
  x = __builtin_amdgcn_fmed3f(x, -65504.f, 65504.f);
  y = __builtin_amdgcn_fmed3f(y, -65504.f, 65504.f);
  f16x3_split(x, y, p1, p2);
}
// same, remembering in `clamped` whether a value was outside +-65504 (range guard)
__device__ __forceinline__ void f16x3_split_clamp_flag(float x, float y, unsigned& p1, unsigned& p2, bool& clamped) {
  // (negated compares: true for NaN as well - a NaN activation must take the float32 re-run, which hands it on like the
  // reference does, not come out of the v_med3 clamp as a finite number)
  clamped |= !(__builtin_fabsf(x) <= 65504.f) | !(__builtin_fabsf(y) <= 65504.f);
  f16x3_split_clamp(x, y, p1, p2);
}

// ---- non-negative activations: ReLU and the f16 range clamp are the same v_med3
__device__ __forceinline__ void f16x3_split_relu(float x, float y, unsigned& p1, unsigned& p2) {
  x = __builtin_amdgcn_fmed3f(x, 0.f, 65504.f);
  y = __builtin_amdgcn_fmed3f(y, 0.f, 65504.f);
  f16x3_split(x, y, p1, p2);
}
// same; `vmax` keeps the running maximum of the UNclamped values (one v_max3 per pair; the caller compares it with 65504 once
// per tile for the range guard)
__device__ __forceinline__ void f16x3_split_relu_max(float x, float y, unsigned& p1, unsigned& p2, float& vmax) {
  vmax = fmaxf(fmaxf(vmax, x), y);
  f16x3_split_relu(x, y, p1, p2);
}
