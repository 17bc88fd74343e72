// Microbenchmark: does the chip hold a higher clock on v_mfma_f32_16x16x32_f16 than on v_mfma_f32_32x32x16_f16?
// The loop is the chain kernel's layer3 walk in miniature: one wave per SIMD on every CU, 144 f32 accumulator registers per wave,
// f16x3 products (hi.hi, lo.hi, hi.lo), every operand re-read from LDS by ds_read_b128 at immediate offsets and prefetched one
// item ahead, random f16 data. Both shapes do the same FLOP from the same LDS bytes:
//   SHAPE 0: per k16 step 2 weight reads, 9 tiles of 32 columns   x (2 reads + 3 MFMAs 32x32x16); two k16 steps per iteration
//   SHAPE 1: per k32 step 4 weight reads, 18 half tiles of 16 cols x (2 reads + 6 MFMAs 16x16x32); one k32 step per iteration
// Reported per shape: wall TFLOP/s over >= 2 s of back-to-back launches, wave cycles per launch and the in-kernel clock
// (delta s_memtime / delta s_memrealtime x 100 MHz, median over workgroups) of the last launch.
// hipcc --offload-arch=gfx950 -O3 -o mfma_shape_f16.bin tools/exp/mfma_shape_f16.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int LDS_BYTES = 147456;
constexpr int STEP_BYTES = 1040;            // distance between two items' reads: 16-byte aligned, walks all banks
constexpr unsigned BASE_MASK = 0xfff0u;     // per-step base < 64 KB; base + largest immediate + 1 KB per wave row stays < LDS_BYTES

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// accumulators pinned to the accumulation registers, the products in source order (left to the compiler, the 16x16x32 loop's
// f32x4 accumulators travel through copies and s_nop pads: 27 cycles per MFMA instead of 16)
#define MFMA32(acc, a, b) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b))
#define MFMA16(acc, a, b) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b))

__device__ __forceinline__ f16x8 rd(const char* lds, unsigned a, int off) {
  return __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(lds + a + off));
}

template <int SHAPE>
__global__ __launch_bounds__(256, 1) void k(const unsigned* __restrict__ src, float* __restrict__ out,
                                            unsigned long long* __restrict__ stamps, int iters) {
  extern __shared__ __attribute__((aligned(1024))) char lds[];
  for (int i = threadIdx.x; i < LDS_BYTES / 4; i += blockDim.x) reinterpret_cast<unsigned*>(lds)[i] = src[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned base = (unsigned)(lane * 16 + wave * 1024);
  float s = 0.f;
  unsigned long long c0, c1, r0, r1;
  if (SHAPE == 0) {
    constexpr int NT = 9;
    f32x16 acc[NT];
    for (int t = 0; t < NT; ++t)
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    unsigned a = base & BASE_MASK;
    f16x8 bh = rd(lds, a, 0), bl = rd(lds, a, 16 * 1024);
    c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters * 2; ++it) {
      const unsigned an = (base + (unsigned)(it + 1) * 4112u) & BASE_MASK;
      const f16x8 wh = rd(lds, a, 32 * 1024), wl = rd(lds, a, 48 * 1024);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f16x8 nh, nl;
        if (t + 1 < NT) { nh = rd(lds, a, (t + 1) * STEP_BYTES); nl = rd(lds, a, 16 * 1024 + (t + 1) * STEP_BYTES); }
        else { nh = rd(lds, an, 0); nl = rd(lds, an, 16 * 1024); }
        __builtin_amdgcn_sched_barrier(0);
        MFMA32(acc[t], wh, bh);
        MFMA32(acc[t], wl, bh);
        MFMA32(acc[t], wh, bl);
        __builtin_amdgcn_sched_barrier(0);
        bh = nh; bl = nl;
      }
      a = an;
    }
    c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
    for (int t = 0; t < NT; ++t)
      for (int r = 0; r < 16; ++r) s += acc[t][r];
  } else {
    constexpr int NT = 18;
    f32x4 acc[2][NT];
    for (int h = 0; h < 2; ++h)
      for (int t = 0; t < NT; ++t)
        for (int r = 0; r < 4; ++r) acc[h][t][r] = 0.f;
    unsigned a = base & BASE_MASK;
    f16x8 bh = rd(lds, a, 0), bl = rd(lds, a, 20 * 1024);
    c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
      const unsigned an = (base + (unsigned)(it + 1) * 4112u) & BASE_MASK;
      f16x8 wh[2], wl[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) { wh[h] = rd(lds, a, 40 * 1024 + h * 2048); wl[h] = rd(lds, a, 44 * 1024 + h * 2048); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f16x8 nh, nl;
        if (t + 1 < NT) { nh = rd(lds, a, (t + 1) * STEP_BYTES); nl = rd(lds, a, 20 * 1024 + (t + 1) * STEP_BYTES); }
        else { nh = rd(lds, an, 0); nl = rd(lds, an, 20 * 1024); }
        __builtin_amdgcn_sched_barrier(0);
        MFMA16(acc[0][t], wh[0], bh);
        MFMA16(acc[1][t], wh[1], bh);
        MFMA16(acc[0][t], wl[0], bh);
        MFMA16(acc[1][t], wl[1], bh);
        MFMA16(acc[0][t], wh[0], bl);
        MFMA16(acc[1][t], wh[1], bl);
        __builtin_amdgcn_sched_barrier(0);
        bh = nh; bl = nl;
      }
      a = an;
    }
    c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime();
    for (int h = 0; h < 2; ++h)
      for (int t = 0; t < NT; ++t)
        for (int r = 0; r < 4; ++r) s += acc[h][t][r];
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if (threadIdx.x == 0) { stamps[2 * blockIdx.x] = c1 - c0; stamps[2 * blockIdx.x + 1] = r1 - r0; }
}

struct Result { double tflops, cycles, mhz, ms_per_launch; int launches; };

template <int SHAPE>
Result run(int cus, int iters, const unsigned* src, float* out, unsigned long long* stamps, double seconds) {
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k<SHAPE>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  CHECK(hipEventRecord(e0));
  hipLaunchKernelGGL((k<SHAPE>), dim3(cus), dim3(256), LDS_BYTES, 0, src, out, stamps, iters);
  CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
  float ms1; CHECK(hipEventElapsedTime(&ms1, e0, e1));
  const int launches = std::max(8, (int)(seconds * 1e3 / ms1) + 1);
  const auto t0 = std::chrono::steady_clock::now();
  CHECK(hipEventRecord(e0));
  for (int i = 0; i < launches; ++i) hipLaunchKernelGGL((k<SHAPE>), dim3(cus), dim3(256), LDS_BYTES, 0, src, out, stamps, iters);
  CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
  CHECK(hipGetLastError());
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> h(2 * cus);
  CHECK(hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost));
  std::vector<double> cyc(cus), mhz(cus);
  for (int b = 0; b < cus; ++b) { cyc[b] = (double)h[2 * b]; mhz[b] = (double)h[2 * b] / (double)h[2 * b + 1] * 100.0; }
  std::sort(cyc.begin(), cyc.end()); std::sort(mhz.begin(), mhz.end());
  // FLOP per iteration per wave: 54 MFMAs of 32x32x16 = 108 MFMAs of 16x16x32 = 54 * 32768
  const double flop = (double)cus * 4 * iters * 54.0 * 32768.0 * launches;
  (void)wall;
  return Result{flop / (ms * 1e-3) / 1e12, cyc[cus / 2], mhz[cus / 2], ms / launches, launches};
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 6000;
  const double seconds = argc > 2 ? atof(argv[2]) : 2.0;
  const int rounds = argc > 3 ? atoi(argv[3]) : 3;
  hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  std::vector<unsigned short> host(LDS_BYTES / 2);
  unsigned long long st = 0x9e3779b97f4a7c15ull;
  for (auto& v : host) {                      // random f16 in +-[0.5, 2): random sign, exponent 14..15, random mantissa
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    const unsigned r = (unsigned)(st >> 33);
    v = (unsigned short)(((r & 1u) << 15) | ((14u + ((r >> 1) & 1u)) << 10) | ((r >> 2) & 0x3ffu));
  }
  unsigned* src; float* out; unsigned long long* stamps;
  CHECK(hipMalloc(&src, LDS_BYTES)); CHECK(hipMalloc(&out, (size_t)cus * 256 * 4)); CHECK(hipMalloc(&stamps, (size_t)cus * 16));
  CHECK(hipMemcpy(src, host.data(), LDS_BYTES, hipMemcpyHostToDevice));
  printf("device %s, %d CUs, one wave per SIMD, %d iterations of 54 x 32768 FLOP per wave per launch, >= %.1f s per run\n",
         prop.name, cus, iters, seconds);
  printf("%-22s %9s %12s %14s %10s %9s\n", "shape", "launches", "ms/launch", "wave cycles", "clock MHz", "TFLOP/s");
  double best[2] = {0, 0};
  for (int r = 0; r < rounds; ++r) {
    const Result a = run<0>(cus, iters, src, out, stamps, seconds);
    printf("%-22s %9d %12.3f %14.0f %10.0f %9.1f\n", "v_mfma 32x32x16 f16", a.launches, a.ms_per_launch, a.cycles, a.mhz, a.tflops);
    const Result b = run<1>(cus, iters, src, out, stamps, seconds);
    printf("%-22s %9d %12.3f %14.0f %10.0f %9.1f\n", "v_mfma 16x16x32 f16", b.launches, b.ms_per_launch, b.cycles, b.mhz, b.tflops);
    printf("round %d: 16x16x32 / 32x32x16 = %.3f x wall FLOP/s, %.3f x cycles, %.3f x clock\n", r, b.tflops / a.tflops,
           b.cycles / a.cycles, b.mhz / a.mhz);
    best[0] = std::max(best[0], a.tflops); best[1] = std::max(best[1], b.tflops);
    fflush(stdout);
  }
  printf("best of %d rounds: 32x32x16 %.1f, 16x16x32 %.1f TFLOP/s, ratio %.3f\n", rounds, best[0], best[1], best[1] / best[0]);
  return 0;
}
