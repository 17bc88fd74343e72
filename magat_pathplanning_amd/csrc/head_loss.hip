// Training of the action head and the loss on the HIP path: the last Linear of actionsMLP (width -> 5 logits), log-softmax and
// the loss in ONE pass over the head's input rows, and their backward in one more.
//
// The reference trains with nn.CrossEntropyLoss() or, when config.label_smoothing != 0, with graphs/losses/label_smoothing.py
// (agents/decentralplannerlocal_OnlineExpert_GAT.py:103-107): LogSoftmax + KLDivLoss(size_average=False) against a smoothed
// one-hot - a SUM over the rows that carries the target distribution's entropy term.  Through torch that tail is about ten
// launches on a 5-column matrix (linear, log-softmax and NLL forward; three backward passes; two GEMMs with a 5-wide operand and
// a bias reduction).  Here:
//   forward   16 lanes per row (a DPP row), four rows per wave: every lane walks 16-byte quads of its row against the five weight
//             rows, row16_sum folds the five dot products, every lane of the row then holds the five logits and makes the
//             stable softmax (row maximum subtracted); lanes 0..4 store the logits and d loss / d logits, lane 0 the row loss.
//             A workgroup adds its rows' losses in double in a fixed order and writes one partial; a one-workgroup launch adds
//             the partials (double, fixed order).
//   backward  a thread owns one 16-byte column quad and walks rows: dX = g dlogits W row by row, and the five dW rows of its quad
//             summed over the workgroup's rows; the workgroup folds its row lanes through LDS and writes one float32 partial per
//             (class, column), a second launch adds the partials in double in a fixed order and scales by g.
// Deterministic: no floating-point atomics anywhere.  The class count is the reference's constant 5.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/magat_hip.h"
#include "magat_common.h"

namespace {

constexpr int HL_CLASSES = 5;
constexpr int HL_THREADS = 256;
constexpr int HL_ROW_LANES = 16;                        // lanes per row of the forward: one DPP row
constexpr int HL_GROUPS = HL_THREADS / HL_ROW_LANES;    // rows a workgroup has in flight
constexpr int HL_FWD_BLOCKS = 1024;                     // most loss partials of a forward
constexpr int HL_BWD_BLOCKS = 128;                      // most dW / db partials of a backward
constexpr int HL_BWD_ROWS = 32;                         // rows per workgroup of the backward, at least
constexpr int HL_MAX_WIDTH = 1024;

struct LossTerms {
  int mode;                  // 0: cross-entropy (mean), 1: the reference's LabelSmoothing (KL sum)
  float q_on, q_off;         // mode 1: the smoothed target distribution, 1 - s on the target and s / 4 off it
  float h_on, h_off;         // mode 1: q log q of either (0 where q = 0)
  float inv_m;               // mode 0: 1 / M
};

struct HeadLossParams {
  const float* x;
  const float* w;
  const float* b;
  const int64_t* target;
  const float* logits_in;    // magat_action_loss_f32: the logits something else produced
  float* logits;
  float* dlogits;
  float* row_loss;
  float* loss;
  double* part;
  long long M;
  int width, ldx, ld, blocks;
  LossTerms t;
};

__device__ __forceinline__ float pick5(const float (&v)[HL_CLASSES], int c) {
  return c == 0 ? v[0] : c == 1 ? v[1] : c == 2 ? v[2] : c == 3 ? v[3] : v[4];
}

// The loss of one row and d loss / d logits (for grad_loss = 1) from its five logits.  A target outside 0..4 is never an index:
// the row's loss and its gradient row are NaN.
__device__ __forceinline__ float row_loss_grad(const float (&z)[HL_CLASSES], long long tgt, const LossTerms& t,
                                               float (&dz)[HL_CLASSES]) {
  float m = z[0];
#pragma unroll
  for (int c = 1; c < HL_CLASSES; ++c) m = fmaxf(m, z[c]);
  float e[HL_CLASSES], s = 0.f;
#pragma unroll
  for (int c = 0; c < HL_CLASSES; ++c) {
    e[c] = expf(z[c] - m);
    s += e[c];
  }
  const float ls = logf(s), inv = 1.f / s;
  const bool ok = tgt >= 0 && tgt < HL_CLASSES;
  const float nan = __builtin_nanf("");
  float loss = 0.f;
  if (t.mode == 0) {
#pragma unroll
    for (int c = 0; c < HL_CLASSES; ++c) {
      const bool on = tgt == c;
      if (on) loss = ls - (z[c] - m);                    // -log p[t], no cancellation against the maximum
      dz[c] = ok ? (e[c] * inv - (on ? 1.f : 0.f)) * t.inv_m : nan;
    }
  } else {
#pragma unroll
    for (int c = 0; c < HL_CLASSES; ++c) {
      const bool on = tgt == c;
      const float q = on ? t.q_on : t.q_off;
      const float nlp = ls - (z[c] - m);                 // -log p[c]
      loss += q != 0.f ? (on ? t.h_on : t.h_off) + q * nlp : 0.f;
      dz[c] = ok ? e[c] * inv - q : nan;
    }
  }
  return ok ? loss : nan;
}

// sum of the workgroup's per-thread doubles in a fixed tree; thread 0 holds the result
__device__ __forceinline__ double block_sum_double(double v) {
  __shared__ double red[HL_THREADS];
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = HL_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(HL_THREADS) void head_loss_forward_kernel(const HeadLossParams p) {
  const int l = threadIdx.x & (HL_ROW_LANES - 1), grp = threadIdx.x / HL_ROW_LANES;
  const int quads = p.width >> 2;
  double acc_loss = 0.0;
  for (long long r = (long long)blockIdx.x * HL_GROUPS + grp; r < p.M; r += (long long)gridDim.x * HL_GROUPS) {
    const float* xr = p.x + r * p.ldx;
    float z[HL_CLASSES] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int q = l; q < quads; q += HL_ROW_LANES) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + 4 * q);
#pragma unroll
      for (int c = 0; c < HL_CLASSES; ++c) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(p.w + (long long)c * p.width + 4 * q);
        z[c] = fmaf(xv[0], wv[0], z[c]);
        z[c] = fmaf(xv[1], wv[1], z[c]);
        z[c] = fmaf(xv[2], wv[2], z[c]);
        z[c] = fmaf(xv[3], wv[3], z[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < HL_CLASSES; ++c) {
      z[c] = row16_sum(z[c]);                            // (all 16 lanes of a row are active or none is)
      if (p.b) z[c] += p.b[c];
    }
    float dz[HL_CLASSES];
    const float rl = row_loss_grad(z, (long long)p.target[r], p.t, dz);
    if (l < HL_CLASSES) {
      p.logits[r * HL_CLASSES + l] = pick5(z, l);
      p.dlogits[r * HL_CLASSES + l] = pick5(dz, l);
    }
    if (l == 0) {
      if (p.row_loss) p.row_loss[r] = rl;
      acc_loss += (double)rl;
    }
  }
  const double s = block_sum_double(acc_loss);
  if (threadIdx.x == 0) p.part[blockIdx.x] = s;
}

// the same loss on logits [M][ld >= 5] that something else produced: a thread per row
__global__ __launch_bounds__(HL_THREADS) void action_loss_kernel(const HeadLossParams p) {
  double acc_loss = 0.0;
  for (long long r = (long long)blockIdx.x * HL_THREADS + threadIdx.x; r < p.M; r += (long long)gridDim.x * HL_THREADS) {
    float z[HL_CLASSES], dz[HL_CLASSES];
#pragma unroll
    for (int c = 0; c < HL_CLASSES; ++c) z[c] = p.logits_in[r * p.ld + c];
    const float rl = row_loss_grad(z, (long long)p.target[r], p.t, dz);
    if (p.dlogits) {
#pragma unroll
      for (int c = 0; c < HL_CLASSES; ++c) p.dlogits[r * HL_CLASSES + c] = dz[c];
    }
    if (p.row_loss) p.row_loss[r] = rl;
    acc_loss += (double)rl;
  }
  const double s = block_sum_double(acc_loss);
  if (threadIdx.x == 0) p.part[blockIdx.x] = s;
}

__global__ __launch_bounds__(HL_THREADS) void loss_finalize_kernel(const HeadLossParams p) {
  double a = 0.0;
  for (int i = threadIdx.x; i < p.blocks; i += HL_THREADS) a += p.part[i];
  const double s = block_sum_double(a);
  if (threadIdx.x == 0) p.loss[0] = (float)(p.t.mode == 0 ? s / (double)p.M : s);
}

struct HeadBwdParams {
  const float* dlogits;
  const float* grad_loss;
  const float* x;
  const float* w;
  float* dx;
  float* dw;
  float* db;
  float* part;               // [blocks][5 * width + 8]: dW partials, then the five db partials
  long long M;
  int width, ldx, lddx, blocks, rows_per_block, reduce;
};

__global__ __launch_bounds__(HL_THREADS) void head_loss_backward_kernel(const HeadBwdParams p) {
  __shared__ float red[HL_CLASSES][HL_THREADS * 4];
  __shared__ float redb[HL_CLASSES][HL_THREADS];
  const int quads = p.width >> 2, lanes = HL_THREADS / quads;
  const int q = threadIdx.x % quads, rl = threadIdx.x / quads;
  const long long r0 = (long long)blockIdx.x * p.rows_per_block;
  const long long r1 = r0 + p.rows_per_block < p.M ? r0 + p.rows_per_block : p.M;
  const float g = p.grad_loss[0];
  f32x4 acc[HL_CLASSES], wq[HL_CLASSES];
  float sb[HL_CLASSES];
#pragma unroll
  for (int c = 0; c < HL_CLASSES; ++c) {
    acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    wq[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    sb[c] = 0.f;
  }
  if (rl < lanes) {
    if (p.dx) {
#pragma unroll
      for (int c = 0; c < HL_CLASSES; ++c) wq[c] = *reinterpret_cast<const f32x4*>(p.w + (long long)c * p.width + 4 * q);
    }
    for (long long r = r0 + rl; r < r1; r += lanes) {
      float d[HL_CLASSES];
#pragma unroll
      for (int c = 0; c < HL_CLASSES; ++c) d[c] = p.dlogits[r * HL_CLASSES + c];
      if (p.dx) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < HL_CLASSES; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) o[k] = fmaf(d[c], wq[c][k], o[k]);
        *reinterpret_cast<f32x4*>(p.dx + r * p.lddx + 4 * q) = o * g;
      }
      if (p.reduce) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(p.x + r * p.ldx + 4 * q);
#pragma unroll
        for (int c = 0; c < HL_CLASSES; ++c) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[c][k] = fmaf(d[c], xv[k], acc[c][k]);
          sb[c] += d[c];
        }
      }
    }
  }
  if (!p.reduce) return;                                 // (uniform: dX alone needs no partials)
#pragma unroll
  for (int c = 0; c < HL_CLASSES; ++c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[c][threadIdx.x * 4 + k] = acc[c][k];
    redb[c][threadIdx.x] = sb[c];
  }
  __syncthreads();
  // thread t folds column t over the row lanes in a fixed order
  float* out = p.part + (long long)blockIdx.x * (HL_CLASSES * p.width + 8);
  for (int t = threadIdx.x; t < p.width; t += HL_THREADS) {
    const int qq = t >> 2, cc = t & 3;
#pragma unroll
    for (int c = 0; c < HL_CLASSES; ++c) {
      float a = 0.f;
      for (int ln = 0; ln < lanes; ++ln) a += red[c][(ln * quads + qq) * 4 + cc];
      out[c * p.width + t] = a;
    }
  }
  if (threadIdx.x < HL_CLASSES) {                        // (the threads of quad 0 carry the same db sums as every other quad's)
    float a = 0.f;
    for (int ln = 0; ln < lanes; ++ln) a += redb[threadIdx.x][ln * quads];
    out[HL_CLASSES * p.width + threadIdx.x] = a;
  }
}

__global__ __launch_bounds__(HL_THREADS) void head_loss_backward_finalize_kernel(const HeadBwdParams p) {
  const int n = HL_CLASSES * p.width, stride = n + 8;
  const int i = blockIdx.x * HL_THREADS + threadIdx.x;
  if (i >= n + HL_CLASSES) return;
  double a = 0.0;
  for (int blk = 0; blk < p.blocks; ++blk) a += (double)p.part[(long long)blk * stride + i];
  const float v = (float)(a * (double)p.grad_loss[0]);
  if (i < n) {
    if (p.dw) p.dw[i] = v;
  } else if (p.db) {
    p.db[i - n] = v;
  }
}

int fwd_blocks(long long M, int rows_per_pass) {
  long long b = (M + rows_per_pass - 1) / rows_per_pass;
  if (b > HL_FWD_BLOCKS) b = HL_FWD_BLOCKS;
  return (int)(b < 1 ? 1 : b);
}

int bwd_blocks(long long M, int* rpb) {
  long long b = (M + HL_BWD_ROWS - 1) / HL_BWD_ROWS;
  if (b > HL_BWD_BLOCKS) b = HL_BWD_BLOCKS;
  if (b < 1) b = 1;
  const long long per = (M + b - 1) / b;
  *rpb = (int)per;
  return (int)((M + per - 1) / per);
}

bool width_ok(int width) { return width % 4 == 0 && width <= HL_MAX_WIDTH; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool loss_terms(int mode, float smoothing, long long M, LossTerms* t) {
  if ((mode != 0 && mode != 1) || !(smoothing >= 0.f && smoothing < 1.f)) return false;
  const double s = (double)smoothing, on = 1.0 - s, off = s / (HL_CLASSES - 1);
  t->mode = mode;
  t->q_on = (float)on;
  t->q_off = (float)off;
  t->h_on = (float)(on * std::log(on));
  t->h_off = off > 0.0 ? (float)(off * std::log(off)) : 0.f;
  t->inv_m = (float)(1.0 / (double)M);
  return true;
}

}  // namespace

size_t magat_head_loss_workspace_floats(long long M, int width) {
  if (M <= 0 || width <= 0 || !width_ok(width)) return 0;
  int rpb;
  const size_t bwd = (size_t)bwd_blocks(M, &rpb) * (HL_CLASSES * (size_t)width + 8);
  const size_t fwd = 2 * (size_t)HL_FWD_BLOCKS;          // loss partials in double
  return bwd > fwd ? bwd : fwd;
}

int magat_head_loss_forward_f32(const float* X, int ldx, const float* W, const float* b, const int64_t* target, int mode,
                                float smoothing, float* logits, float* dlogits, float* row_loss, float* loss, float* workspace,
                                long long M, int width, void* stream) {
  if (!X || !W || !target || !logits || !dlogits || !loss || !workspace) return MAGAT_ERR_NULL;
  if (M <= 0 || width <= 0) return MAGAT_ERR_BAD_SHAPE;
  HeadLossParams p = {};
  if (!width_ok(width) || ldx < width || ldx % 4 || !loss_terms(mode, smoothing, M, &p.t)) return MAGAT_ERR_UNSUPPORTED;
  if (!aligned16(X) || !aligned16(W)) return MAGAT_ERR_UNSUPPORTED;      // (rows are read in 16-byte pieces)
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return MAGAT_ERR_WORKSPACE;
  p.x = X; p.w = W; p.b = b; p.target = target; p.logits = logits; p.dlogits = dlogits; p.row_loss = row_loss; p.loss = loss;
  p.part = reinterpret_cast<double*>(workspace);
  p.M = M; p.width = width; p.ldx = ldx;
  p.blocks = fwd_blocks(M, HL_GROUPS);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int pid = magat_prof_begin(MAGAT_TAG_HEAD_LOSS, st);
  hipLaunchKernelGGL(head_loss_forward_kernel, dim3(p.blocks), dim3(HL_THREADS), 0, st, p);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(HL_THREADS), 0, st, p);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

int magat_action_loss_f32(const float* logits, int ld, const int64_t* target, int mode, float smoothing, float* dlogits,
                          float* row_loss, float* loss, float* workspace, long long M, void* stream) {
  if (!logits || !target || !loss || !workspace) return MAGAT_ERR_NULL;
  if (M <= 0) return MAGAT_ERR_BAD_SHAPE;
  HeadLossParams p = {};
  if (ld < HL_CLASSES || !loss_terms(mode, smoothing, M, &p.t)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return MAGAT_ERR_WORKSPACE;
  p.logits_in = logits; p.ld = ld; p.target = target; p.dlogits = dlogits; p.row_loss = row_loss; p.loss = loss;
  p.part = reinterpret_cast<double*>(workspace);
  p.M = M;
  p.blocks = fwd_blocks(M, HL_THREADS);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int pid = magat_prof_begin(MAGAT_TAG_HEAD_LOSS, st);
  hipLaunchKernelGGL(action_loss_kernel, dim3(p.blocks), dim3(HL_THREADS), 0, st, p);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(HL_THREADS), 0, st, p);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

int magat_head_loss_backward_f32(const float* dlogits, const float* grad_loss, const float* X, int ldx, const float* W, float* dX,
                                 int lddx, float* dW, float* db, float* workspace, long long M, int width, void* stream) {
  if (!dlogits || !grad_loss || !X || !W || !workspace) return MAGAT_ERR_NULL;
  if (M <= 0 || width <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (!width_ok(width) || ldx < width || ldx % 4 || (dX && (lddx < width || lddx % 4))) return MAGAT_ERR_UNSUPPORTED;
  if (!aligned16(X) || !aligned16(W) || !aligned16(dX)) return MAGAT_ERR_UNSUPPORTED;
  HeadBwdParams p = {};
  p.dlogits = dlogits; p.grad_loss = grad_loss; p.x = X; p.w = W; p.dx = dX; p.dw = dW; p.db = db; p.part = workspace;
  p.M = M; p.width = width; p.ldx = ldx; p.lddx = lddx;
  p.blocks = bwd_blocks(M, &p.rows_per_block);
  p.reduce = dW || db ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int pid = magat_prof_begin(MAGAT_TAG_HEAD_LOSS, st);
  if (dX || p.reduce) hipLaunchKernelGGL(head_loss_backward_kernel, dim3(p.blocks), dim3(HL_THREADS), 0, st, p);
  if (p.reduce) {
    const int n = HL_CLASSES * width + HL_CLASSES;
    hipLaunchKernelGGL(head_loss_backward_finalize_kernel, dim3((n + HL_THREADS - 1) / HL_THREADS), dim3(HL_THREADS), 0, st, p);
  }
  magat_prof_end(pid, st);
  return magat_check_launch();
}
