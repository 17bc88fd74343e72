// A stand-in for <hip/hip_runtime.h> that lets a row-board kernel of csrc/ - one workgroup of 1 to 4 wavefronts per case - compile
// for the host and run as one thread per lane (tools/host_wave/mapf_lns_check.cpp, mapf_lns_wide_check.cpp): every cross-lane
// operation (ballot, DPP wave shift, readfirstlane, shuffle) is a rendezvous of the 64 threads of ONE wavefront and exchanges
// inside it, __syncthreads is a rendezvous of all threads of the workgroup, blockDim.x is what the launch asked for.  So the
// kernel must keep a wavefront in wave-uniform control flow around the first and the workgroup in uniform control flow around
// the second - as the hardware wants it too.  Between two rendezvous the threads run in any order: a missing barrier between a
// store of one thread and a load of another, which lock step would hide, is a data race here (run under a thread sanitizer to
// see it).  Workgroups run one after another; __shared__ variables are statics.  Only what the row-board kernels use is provided.
#pragma once
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAGAT_HOST_WAVE 1      // for the few places where a kernel's text has to differ on the host (its dynamic LDS)
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))
#define __shared__ static
#define __launch_bounds__(n)
#define __align__(n) __attribute__((aligned(n)))
#define HIP_DYNAMIC_SHARED(type, var) type* var = reinterpret_cast<type*>(host_wave::dyn_lds);

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef void* hipStream_t;
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
inline hipError_t hipGetLastError() { return hipSuccess; }

namespace host_wave {
constexpr int kLanes = 64, kMaxWaves = 4;
inline thread_local int tid = 0, lane = 0, wave = 0;
inline unsigned block = 0, blocks = 1, threads = kLanes;
inline pthread_barrier_t barrier, wave_barrier[kMaxWaves];
inline unsigned long long slot[kMaxWaves][kLanes];
inline void meet() { pthread_barrier_wait(&barrier); }      // the workgroup
// every lane of a wavefront posts a value; fn(slots of the wavefront) is evaluated by every lane between the two rendezvous
template <typename F>
inline auto exchange(unsigned long long mine, F fn) {
  slot[wave][lane] = mine;
  pthread_barrier_wait(&wave_barrier[wave]);
  auto r = fn(slot[wave]);
  pthread_barrier_wait(&wave_barrier[wave]);
  return r;
}
inline unsigned long long ballot(bool p) {
  return exchange(p ? 1ull : 0ull, [](const unsigned long long* s) {
    unsigned long long m = 0;
    for (int i = 0; i < kLanes; ++i) m |= s[i] << i;
    return m;
  });
}
inline int update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
  const bool ror = ctrl > 0x120 && ctrl < 0x130;      // row_ror:n, a rotation inside each row of 16 lanes
  if (row_mask != 0xf || bank_mask != 0xf || !bound_ctrl || (ctrl != 0x130 && ctrl != 0x138 && !ror)) abort();      // else wave_shl:1, wave_shr:1 only
  (void)old;
  const int from = ror ? (lane & ~15) | ((lane - (ctrl & 15)) & 15) : ctrl == 0x130 ? lane + 1 : lane - 1;
  return exchange((unsigned)src, [from](const unsigned long long* s) { return from >= 0 && from < kLanes ? (int)(unsigned)s[from] : 0; });
}
inline int readlane(int v, int l) {
  return exchange((unsigned)v, [l](const unsigned long long* s) { return (int)(unsigned)s[l]; });
}
inline int shfl_xor(int v, int mask) {
  const int from = lane ^ mask;
  return exchange((unsigned)v, [from](const unsigned long long* s) { return (int)(unsigned)s[from]; });
}
struct Idx {
  struct X {
    operator unsigned() const { return (unsigned)tid; }
  } x;
};
struct BlockIdx {
  struct X {
    operator unsigned() const { return block; }
  } x;
  unsigned y = 0, z = 0;
};
struct BlockDim {
  struct X {
    operator unsigned() const { return threads; }
  } x;
  unsigned y = 1, z = 1;
};
inline unsigned long long dyn_lds[256 * 64];      // the dynamic LDS of a workgroup: 128 KB
struct GridDim {
  struct X {
    operator unsigned() const { return blocks; }
  } x;
  unsigned y = 1, z = 1;
};
// runs kernel(args...) for every workgroup of the grid, block.x threads each: whole wavefronts, 1 to 4 of them
template <typename K, typename... A>
inline void launch(K kernel, dim3 grid, dim3 block_dim, A... args) {
  if (block_dim.x == 0 || block_dim.x % kLanes || block_dim.x > kLanes * kMaxWaves || block_dim.y != 1 || block_dim.z != 1) abort();
  blocks = grid.x;
  threads = block_dim.x;
  const int nt = (int)threads, nw = nt / kLanes;
  for (block = 0; block < grid.x; ++block) {
    pthread_barrier_init(&barrier, nullptr, nt);
    for (int w = 0; w < nw; ++w) pthread_barrier_init(&wave_barrier[w], nullptr, kLanes);
    auto body = [&](int t) {
      tid = t;
      lane = t % kLanes;
      wave = t / kLanes;
      kernel(args...);
    };
    pthread_t th[kLanes * kMaxWaves];
    struct Arg {
      decltype(body)* b;
      int t;
    } arg[kLanes * kMaxWaves];
    for (int t = 0; t < nt; ++t) {
      arg[t] = {&body, t};
      if (pthread_create(&th[t], nullptr, [](void* p) -> void* {
        Arg* a = static_cast<Arg*>(p);
        (*a->b)(a->t);
        return nullptr;
      }, &arg[t]) != 0) abort();
    }
    for (int t = 0; t < nt; ++t) pthread_join(th[t], nullptr);
    for (int w = 0; w < nw; ++w) pthread_barrier_destroy(&wave_barrier[w]);
    pthread_barrier_destroy(&barrier);
  }
}
}  // namespace host_wave

static host_wave::Idx threadIdx;
static host_wave::BlockIdx blockIdx;
static host_wave::GridDim gridDim;
static host_wave::BlockDim blockDim;

#define __syncthreads() host_wave::meet()
#define __builtin_amdgcn_ballot_w64(p) host_wave::ballot(p)
#define __ballot(p) host_wave::ballot(p)
#define __builtin_amdgcn_fence(order, scope) ((void)0)
#define __builtin_amdgcn_wave_barrier() ((void)pthread_barrier_wait(&host_wave::wave_barrier[host_wave::wave]))
#define __builtin_amdgcn_update_dpp(o, s, c, r, b, bc) host_wave::update_dpp(o, s, c, r, b, bc)
#define __builtin_amdgcn_readfirstlane(v) host_wave::readlane(v, 0)
#define __builtin_amdgcn_readlane(v, l) host_wave::readlane(v, l)
#define __shfl_xor(v, m, w) host_wave::shfl_xor(v, m)
#define __popcll(v) __builtin_popcountll(v)
#define __clzll(v) __builtin_clzll(v)
inline unsigned long long __brevll(unsigned long long v) {
  unsigned long long r = 0;
  for (int i = 0; i < 64; ++i) r |= ((v >> i) & 1ull) << (63 - i);
  return r;
}
inline int atomicMin(int* p, int v) {
  int old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return old;
}
inline unsigned atomicOr(unsigned* p, unsigned v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
inline unsigned long long atomicOr(unsigned long long* p, unsigned long long v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_fetch_add(p, v, order, scope) __atomic_fetch_add(p, v, order)
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) host_wave::launch(kernel, grid, block, __VA_ARGS__)
