// Body of gat_small_kernel and gat_small_cos_kernel (gat_small.hip), included INTO each kernel: the kernel's parameter `p`, its
// template arguments F, KT, CONCAT and the constant COS are in scope.  (A shared __device__ function template was tried first:
// handing the parameter block to it by value or by reference changes the register allocation of the existing kernels.)
  extern __shared__ __align__(16) char lds_all[];
  constexpr int CT = F / 32, KF = F / 16;
  constexpr int RS = 2 * F + 16;             // row stride of the X / Q planes (bytes): rows land 20 / 36 banks apart
  constexpr int SA = 80;                     // row stride of the A / U^T planes: 32 columns + 16 bytes
  constexpr int XO = 0, QO = 64 * RS, AO = 128 * RS, UO = AO + 64 * SA, QN = UO + 2 * F * SA, WLDS = QN + (COS ? 128 : 0);
  constexpr float kInvScale = 1.f / 256.f;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int fr = lane & 31, fh = lane >> 5;
  char* const lds = lds_all + w * WLDS;      // everything below is private to this wave
  const int N = p.N, G = F;
  float xs = 1.f;
  if (p.x_scale) xs = *p.x_scale;
  if (xs == 0.f) xs = 1.f;
  const float ixs = 1.f / xs;
  const float kOutScale = kInvScale * ixs;
  const float kLog2e = COS ? 1.4426950408889634f : 1.4426950408889634f * ixs * ixs;
  float vmax = 0.f;
  const long long plane = (long long)p.NC * G;      // halves per weight plane
  float biasv[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) biasv[ct] = p.bias ? p.bias[32 * ct + fr] : 0.f;

  for (int inst = (int)blockIdx.x * 4 + w; inst < p.B; inst += (int)gridDim.x * 4) {
    // ---- X rows -> f16 planes (rows past N: zeros)
    {
      const float* Xb = p.X + (long long)inst * N * p.ldx;
      for (int idx = lane; idx < 32 * (F / 8); idx += 64) {
        const int row = idx / (F / 8), ch = idx % (F / 8);
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if (row < N) {
          v0 = *reinterpret_cast<const f32x4*>(Xb + (long long)row * p.ldx + 8 * ch);
          v1 = *reinterpret_cast<const f32x4*>(Xb + (long long)row * p.ldx + 8 * ch + 4);
        }
        float xv[8] = {v0[0] * xs, v0[1] * xs, v0[2] * xs, v0[3] * xs, v1[0] * xs, v1[1] * xs, v1[2] * xs, v1[3] * xs};
        bool bad = false;      // (a NaN must raise the flag too: fmaxf drops it from the running maximum)
#pragma unroll
        for (int e = 0; e < 8; ++e) bad |= !(fabsf(xv[e]) <= 65504.f);
        if (bad) vmax = __builtin_inff();
        uint4 hi, lo;
        f16x3_split_absmax(xv[0], xv[1], hi.x, lo.x, vmax);
        f16x3_split_absmax(xv[2], xv[3], hi.y, lo.y, vmax);
        f16x3_split_absmax(xv[4], xv[5], hi.z, lo.z, vmax);
        f16x3_split_absmax(xv[6], xv[7], hi.w, lo.w, vmax);
        char* dst = lds + XO + row * RS + ch * 16;
        *reinterpret_cast<uint4*>(dst) = hi;
        *reinterpret_cast<uint4*>(dst + 32 * RS) = lo;
      }
    }
    // ---- COS: 1 / max(|x_i|, 1e-9) of this lane's agent i = lane % 32, from the float32 row (each half of the lane pair sums F / 2)
    float xinv = 0.f;
    if constexpr (COS) {
      const float* xr = p.X + ((long long)inst * N + (fr < N ? fr : 0)) * p.ldx + fh * (F / 2);
      float ss = 0.f;
#pragma unroll
      for (int c = 0; c < F / 8; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + 4 * c);
        ss = fmaf(v[3], v[3], fmaf(v[2], v[2], fmaf(v[1], v[1], fmaf(v[0], v[0], ss))));
      }
      ss += __shfl_xor(ss, 32, 64);
      const float nx = sqrtf(ss);
      xinv = 1.f / fmaxf(nx, 1e-9f);
      if (fr < N && nx > 0.f && !(nx * xs >= kCosTiny)) vmax = __builtin_inff();
    }
    // ---- edge mask of this lane's row i = lane % 32 (bits j), |S| > 1e-9 (graphML.py:1274-1276; NaN entries are no edges)
    unsigned mk = 0u;
    if (p.rmask_pre) {
      if (fr < N) mk = p.rmask_pre[((long long)inst * N + fr) * 4];
    } else {
      // lane (fr, fh): row i = fr, columns j = 16 fh .. 16 fh + 15 of it; the two halves are OR-ed
      // (the sixteen entries are requested together - clamped addresses, the predicate on the loaded value - and pinned in front
      //  of the tests: as a loop with a run-time bound they were sixteen round trips, one after the other)
      unsigned bits = 0u;
      auto row_bits = [&](auto tag) __attribute__((always_inline)) {
        typedef decltype(tag) ST;
        const ST* Sp = static_cast<const ST*>(p.S) + ((long long)inst * N + (fr < N ? fr : N - 1)) * N;
        ST sv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) sv[u] = Sp[16 * fh + u < N ? 16 * fh + u : N - 1];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          bool e_ = (sv[u] < (ST)0 ? -sv[u] : sv[u]) > (ST)1e-9 && fr < N && 16 * fh + u < N;      // (NaN: no edge)
          if constexpr (COS)      // GAT_origin's rule, in float32: |float(S) + I| > 1e-9 (a diagonal -1 cancels the self-loop)
            e_ = fabsf((float)sv[u] + (16 * fh + u == fr ? 1.f : 0.f)) > 1e-9f && fr < N && 16 * fh + u < N;
          bits |= (e_ ? 1u : 0u) << (16 * fh + u);
        }
      };
      if (p.s_is_f64) row_bits(double{});
      else row_bits(float{});
      mk = bits | (unsigned)__shfl_xor((int)bits, 32, 64);
    }
    mk >>= 4 * fh;      // bit (8 (r / 4) + r % 4) = row j of accumulator register r

    float ysum[CT][16];
    if constexpr (!CONCAT) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) ysum[ct][r] = 0.f;
    }
#pragma unroll 1
    for (int hd = 0; hd < p.P; ++hd) {
      // this lane's 16-byte pieces of weight row (base + lane % 32): k step ks, plane pl at + pl * plane + 16 ks + 8 fh halves
      auto wfrag = [&](long long row0, int ks, int pl) __attribute__((always_inline)) {
        return *reinterpret_cast<const uint4*>(p.Hs + pl * plane + (row0 + fr) * G + 16 * ks + 8 * fh);
      };
      auto xfrag = [&](int ks, int pl) __attribute__((always_inline)) {
        return *reinterpret_cast<const uint4*>(lds + XO + pl * 32 * RS + fr * RS + (16 * ks + 8 * fh) * 2);
      };
      // ---- G1 (operands swapped): Q^T tile, lane = agent row j, register quads = 4 consecutive columns g -> Q planes [j][g]
      // (a product's weight fragments are requested together and pinned in front of its matrix instructions: the compiler moves
      //  every request next to its use otherwise - one exposed L2 round trip per k step at one or two waves per SIMD)
      uint4 wq[CT][KF][2];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int ks = 0; ks < KF; ++ks) {
          wq[ct][ks][0] = wfrag((long long)hd * G + 32 * ct, ks, 0);
          wq[ct][ks][1] = wfrag((long long)hd * G + 32 * ct, ks, 1);
        }
      __builtin_amdgcn_sched_barrier(0);
      float qss = 0.f;      // COS: this lane's share of |q_j|^2 (scaled by x_scale^2)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KF; ++ks) {
          const uint4 w0 = wq[ct][ks][0], w1 = wq[ct][ks][1], x0 = xfrag(ks, 0), x1 = xfrag(ks, 1);
          acc = mfma16(w0, x0, acc);
          acc = mfma16(w1, x0, acc);
          acc = mfma16(w0, x1, acc);
        }
        if constexpr (COS) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float a = acc[r] * kInvScale;
            qss = fmaf(a, a, qss);
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint2 hi, lo;
          f16x3_split_absmax(acc[4 * q] * kInvScale, acc[4 * q + 1] * kInvScale, hi.x, lo.x, vmax);
          f16x3_split_absmax(acc[4 * q + 2] * kInvScale, acc[4 * q + 3] * kInvScale, hi.y, lo.y, vmax);
          char* o = lds + QO + fr * RS + (32 * ct + 8 * q + 4 * fh) * 2;
          *reinterpret_cast<uint2*>(o) = hi;
          *reinterpret_cast<uint2*>(o + 32 * RS) = lo;
        }
      }
      if constexpr (COS) {      // qn[j] = 1 / (max(|q_j|, 1e-9) x_scale^2): the score's scale but for 1 / max(|x_i|, 1e-9)
        qss += __shfl_xor(qss, 32, 64);
        const float nq = sqrtf(qss);
        if (fr < N && nq > 0.f && !(nq >= kCosTiny)) vmax = __builtin_inff();
        if (fh == 0) *reinterpret_cast<float*>(lds + QN + 4 * fr) = ixs * ixs / fmaxf(nq * ixs, 1e-9f);
      }
      // 32 features: the K taps' fragments (4 K registers quads) are requested here, in flight under G2 and the softmax
      constexpr bool WEARLY = false;      // (requesting the taps in front of G2 cost the second wave per SIMD: 256 + registers)
      uint4 wt[WEARLY ? KT : 1][CT][KF][2];
      if constexpr (WEARLY) {
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int ks = 0; ks < KF; ++ks) {
              const long long row0 = (long long)p.P * G + ((long long)hd * KT + k) * F + 32 * ct;
              wt[k][ct][ks][0] = wfrag(row0, ks, 0);
              wt[k][ct][ks][1] = wfrag(row0, ks, 1);
            }
        __builtin_amdgcn_sched_barrier(0);
      }
      // ---- G2: E^T[j][i] = sum_g Q[j][g] X[i][g]; lane = column i, registers = rows j
      f32x16 e;
#pragma unroll
      for (int r = 0; r < 16; ++r) e[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KF; ++ks) {
        const char* qp = lds + QO + fr * RS + (16 * ks + 8 * fh) * 2;
        const uint4 q0 = *reinterpret_cast<const uint4*>(qp), q1 = *reinterpret_cast<const uint4*>(qp + 32 * RS);
        const uint4 x0 = xfrag(ks, 0), x1 = xfrag(ks, 1);
        e = mfma16(q0, x0, e);
        e = mfma16(q0, x1, e);
        e = mfma16(q1, x0, e);
      }
      if constexpr (COS) {      // rows j = 8 q + 4 fh + c of register 4 q + c: four qn per vector LDS read
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 qv = *reinterpret_cast<const f32x4*>(lds + QN + 4 * (8 * q + 4 * fh));
#pragma unroll
          for (int c = 0; c < 4; ++c) e[4 * q + c] *= qv[c] * xinv;
        }
      }
      // masked softmax of row i over its edges j (in-lane + the partner lane), A planes [j][i] * 2^8
      float mx = -__builtin_inff();
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)mk, 8 * (r >> 2) + (r & 3), 1);
        const float ev = e[r];      // (a scalar copy: bit-casting the vector element itself reads element 0)
        const float em = __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, ev) & m) | (0xff800000u & ~m));
        e[r] = em;
        mx = fmaxf(mx, em);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float cexp = mx > -__builtin_inff() ? -mx * kLog2e : 0.f;
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        e[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(e[r], kLog2e, cexp));
        sum += e[r];
      }
      sum += __shfl_xor(sum, 32, 64);
      const float inv = sum > 0.f ? 256.f / sum : 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        unsigned ha[2], la[2];
        f16x3_split(e[4 * q] * inv, e[4 * q + 1] * inv, ha[0], la[0]);
        f16x3_split(e[4 * q + 2] * inv, e[4 * q + 3] * inv, ha[1], la[1]);
        char* o = lds + AO + (8 * q + 4 * fh) * SA + fr * 2;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          *reinterpret_cast<unsigned short*>(o + c * SA) = (unsigned short)(ha[c >> 1] >> (16 * (c & 1)));
          *reinterpret_cast<unsigned short*>(o + c * SA + 32 * SA) = (unsigned short)(la[c >> 1] >> (16 * (c & 1)));
        }
      }
      // ---- G3: U_k[i][c] for the K taps (lane = column c, registers = rows i)
      f32x16 acc[KT][CT];
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        uint4 wk[WEARLY ? 1 : CT][KF][2];      // (wider layers: a tap's fragments together, in front of its products)
        if constexpr (!WEARLY) {
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int ks = 0; ks < KF; ++ks) {
              const long long row0 = (long long)p.P * G + ((long long)hd * KT + k) * F + 32 * ct;
              wk[ct][ks][0] = wfrag(row0, ks, 0);
              wk[ct][ks][1] = wfrag(row0, ks, 1);
            }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[k][ct][r] = 0.f;
#pragma unroll
          for (int ks = 0; ks < KF; ++ks) {
            uint4 w0, w1;
            if constexpr (WEARLY) { w0 = wt[k][ct][ks][0]; w1 = wt[k][ct][ks][1]; }
            else { w0 = wk[ct][ks][0]; w1 = wk[ct][ks][1]; }
            const uint4 x0 = xfrag(ks, 0), x1 = xfrag(ks, 1);
            acc[k][ct] = mfma16(x0, w0, acc[k][ct]);
            acc[k][ct] = mfma16(x0, w1, acc[k][ct]);
            acc[k][ct] = mfma16(x1, w0, acc[k][ct]);
          }
        }
      }
      // ---- hops (Horner): acc_k += A U_{k+1}; the U^T planes [c][i] are rewritten from acc_{k+1}
#pragma unroll
      for (int k = KT - 2; k >= 0; --k) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            uint2 hi, lo;
            f16x3_split_absmax(acc[k + 1][ct][4 * q] * kInvScale, acc[k + 1][ct][4 * q + 1] * kInvScale, hi.x, lo.x, vmax);
            f16x3_split_absmax(acc[k + 1][ct][4 * q + 2] * kInvScale, acc[k + 1][ct][4 * q + 3] * kInvScale, hi.y, lo.y, vmax);
            char* o = lds + UO + (32 * ct + fr) * SA + (8 * q + 4 * fh) * 2;
            *reinterpret_cast<uint2*>(o) = hi;
            *reinterpret_cast<uint2*>(o + F * SA) = lo;
          }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const char* ap = lds + AO + fr * SA + (16 * ks + 8 * fh) * 2;
          const uint4 a0 = *reinterpret_cast<const uint4*>(ap), a1 = *reinterpret_cast<const uint4*>(ap + 32 * SA);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const char* up = lds + UO + (32 * ct + fr) * SA + (16 * ks + 8 * fh) * 2;
            const uint4 u0 = *reinterpret_cast<const uint4*>(up), u1 = *reinterpret_cast<const uint4*>(up + F * SA);
            acc[k][ct] = mfma16(a0, u0, acc[k][ct]);
            acc[k][ct] = mfma16(a0, u1, acc[k][ct]);
            acc[k][ct] = mfma16(a1, u0, acc[k][ct]);
          }
        }
      }
      // ---- epilogue: lane = column c, registers = rows j
      float* yb = p.Y + (long long)inst * N * p.ldy;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 8 * (r >> 2) + 4 * fh + (r & 3);
          const float v = __builtin_fmaf(acc[0][ct][r], kOutScale, biasv[ct]);
          if constexpr (CONCAT) {
            if (j < N) yb[(long long)j * p.ldy + hd * F + 32 * ct + fr] = __builtin_amdgcn_fmed3f(v, 0.f, __builtin_inff());
          } else {
            ysum[ct][r] += v;      // (graphML.py:4663-4667: mean over the heads, then ReLU)
            if (hd == p.P - 1 && j < N)
              yb[(long long)j * p.ldy + 32 * ct + fr] = __builtin_amdgcn_fmed3f(ysum[ct][r] / (float)p.P, 0.f, __builtin_inff());
          }
        }
    }
  }
  if (p.range_flag && vmax > 65504.f) atomicOr(p.range_flag, 1);
