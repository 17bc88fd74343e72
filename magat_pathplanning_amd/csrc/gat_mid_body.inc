// Body of gat_mid_kernel and gat_mid_cos_kernel (gat_mid.hip), included INTO each kernel: the kernel's parameter `p`, its template
// arguments F, KT, NT, CONCAT, HS, XR and the constant COS are in scope (a shared __device__ function changes the register
// allocation of the existing kernels; see gat_small_body.inc).  COS: gat_small.hip's cosine form by row tiles - qn[ROWS] is
// workgroup LDS, written in front of the 'Q planes complete' barrier.
  extern __shared__ __align__(16) char lds[];
  constexpr int CT = F / 32, KF = F / 16, ROWS = 32 * NT, THREADS = 64 * NT;
  constexpr int RS = 2 * F + 16;             // row stride of the X / Q planes (bytes)
  constexpr int SA = 2 * ROWS + 16;          // row stride of the A / U^T planes (bytes): ROWS columns of halves + 16
  constexpr int XPL = ROWS * RS, APL = ROWS * SA, UPL = F * SA;
  constexpr int XO = 0, QO = XR ? 0 : 2 * XPL, UO = QO;      // (XR: the X planes live in registers)
  constexpr int AO = QO + (2 * XPL > 2 * UPL ? 2 * XPL : 2 * UPL);
  constexpr int QNO = AO + 2 * APL;          // COS: qn[ROWS] floats behind the A planes
  constexpr float kInvScale = 1.f / 256.f;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int fr = lane & 31, fh = lane >> 5;
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
  const int myrow = 32 * w + fr;                    // this lane's agent (row j of Q / A^T, column i of the scores, ...)

  const int ninst = HS ? (int)gridDim.x / p.P : (int)gridDim.x;      // (HS: gridDim.x = instances-in-flight x P)
  const int hlo = HS ? (int)blockIdx.x % p.P : 0;
  int hhi = HS ? hlo + 1 : p.P;
  if constexpr (HS && XR) asm volatile("" : "+s"(hhi));      // (a head LOOP for the compiler too: as straight-line code this form spilled 289 .. 468 registers)
  for (int inst = HS ? (int)blockIdx.x / p.P : (int)blockIdx.x; inst < p.B; inst += ninst) {
    __syncthreads();      // every wave is done with the previous instance's planes
    // ---- X rows -> f16 planes (rows past N: zeros): all waves into LDS, or (XR) every lane its own operand fragments
    uint4 xr[XR ? KF : 1][2];
    if constexpr (XR) {
      const float* xrow = p.X + ((long long)inst * N + (myrow < N ? myrow : N - 1)) * p.ldx + 8 * fh;
#pragma unroll
      for (int ks = 0; ks < KF; ++ks) {
        f32x4 v0 = *reinterpret_cast<const f32x4*>(xrow + 16 * ks), v1 = *reinterpret_cast<const f32x4*>(xrow + 16 * ks + 4);
        if (myrow >= N) { v0 = f32x4{0.f, 0.f, 0.f, 0.f}; v1 = v0; }
        float xv[8] = {v0[0] * xs, v0[1] * xs, v0[2] * xs, v0[3] * xs, v1[0] * xs, v1[1] * xs, v1[2] * xs, v1[3] * xs};
        bool bad = false;
#pragma unroll
        for (int e = 0; e < 8; ++e) bad |= !(fabsf(xv[e]) <= 65504.f);
        if (bad) vmax = __builtin_inff();
        f16x3_split_cv_absmax(xv[0], xv[1], xr[ks][0].x, xr[ks][1].x, vmax);
        f16x3_split_cv_absmax(xv[2], xv[3], xr[ks][0].y, xr[ks][1].y, vmax);
        f16x3_split_cv_absmax(xv[4], xv[5], xr[ks][0].z, xr[ks][1].z, vmax);
        f16x3_split_cv_absmax(xv[6], xv[7], xr[ks][0].w, xr[ks][1].w, vmax);
      }
    } else {
      const float* Xb = p.X + (long long)inst * N * p.ldx;
      for (int idx = t; idx < ROWS * (F / 8); idx += THREADS) {
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
        f16x3_split_cv_absmax(xv[0], xv[1], hi.x, lo.x, vmax);
        f16x3_split_cv_absmax(xv[2], xv[3], hi.y, lo.y, vmax);
        f16x3_split_cv_absmax(xv[4], xv[5], hi.z, lo.z, vmax);
        f16x3_split_cv_absmax(xv[6], xv[7], hi.w, lo.w, vmax);
        char* dst = lds + XO + row * RS + ch * 16;
        *reinterpret_cast<uint4*>(dst) = hi;
        *reinterpret_cast<uint4*>(dst + XPL) = lo;
      }
    }
    // ---- COS: 1 / max(|x_i|, 1e-9) of this lane's agent, from the float32 row (each half of the lane pair sums F / 2)
    float xinv = 0.f;
    if constexpr (COS) {
      const float* xrow = p.X + ((long long)inst * N + (myrow < N ? myrow : N - 1)) * p.ldx + fh * (F / 2);
      float ss = 0.f;
#pragma unroll
      for (int c = 0; c < F / 8; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xrow + 4 * c);
        ss = fmaf(v[3], v[3], fmaf(v[2], v[2], fmaf(v[1], v[1], fmaf(v[0], v[0], ss))));
      }
      ss += __shfl_xor(ss, 32, 64);
      const float nx = sqrtf(ss);
      xinv = 1.f / fmaxf(nx, 1e-9f);
      if (myrow < N && nx > 0.f && !(nx * xs >= kMidCosTiny)) vmax = __builtin_inff();
    }
    // ---- edge masks of this wave's 32 rows: bit j of word j / 32 <=> |S[i][j]| > 1e-9 (graphML.py:1274-1276; NaN: no edge).
    // A row is read by the whole wave (lane = column, 256-byte runs), the bits come from a ballot; lane (fr, .) keeps row fr's
    unsigned mk[NT];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) mk[jt] = 0u;
    // (eight rows per batch: their loads are in flight together - one row at a time was a serial chain of 64 L2 round trips.  The
    //  scheduling barrier keeps them so: without it the compiler moved every load next to its ballot again, one round trip a row)
    //  The float32 | float64 choice is made ONCE around the loop: inside it, every load sat in its own branch diamond.)
    constexpr int HC = (ROWS + 63) / 64;
    auto build_masks = [&](auto tag) __attribute__((always_inline)) {
      typedef decltype(tag) ST;
      const ST* Sp = static_cast<const ST*>(p.S) + (long long)inst * N * N;
#pragma unroll 1
      for (int il0 = 0; il0 < 32; il0 += 8) {
        ST sv[8][HC];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = 32 * w + il0 + u;
#pragma unroll
          for (int hc = 0; hc < HC; ++hc) {
            const int j = 64 * hc + lane;
            // (branch-free: clamped addresses, the predicate applied to the loaded value - the batch's loads issue back to back)
            sv[u][hc] = Sp[(long long)(i < N ? i : N - 1) * N + (j < N ? j : N - 1)];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int hc = 0; hc < HC; ++hc) {
            const int i = 32 * w + il0 + u, j = 64 * hc + lane;
            bool e_ = (sv[u][hc] < (ST)0 ? -sv[u][hc] : sv[u][hc]) > (ST)1e-9 && i < N && j < N;      // (NaN: no edge)
            if constexpr (COS)      // GAT_origin's rule, in float32: |float(S) + I| > 1e-9 (a diagonal -1 cancels the self-loop)
              e_ = fabsf((float)sv[u][hc] + (i == j ? 1.f : 0.f)) > 1e-9f && i < N && j < N;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(e_);
            if (fr == il0 + u) {
              if (2 * hc < NT) mk[2 * hc] = (unsigned)bal;
              if (2 * hc + 1 < NT) mk[2 * hc + 1] = (unsigned)(bal >> 32);
            }
          }
      }
    };
    if (p.s_is_f64) build_masks(double{});
    else build_masks(float{});
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) mk[jt] >>= 4 * fh;      // bit (8 (r / 4) + r % 4) = row j of accumulator register r
    __syncthreads();      // X planes complete

    float ysum[(CONCAT || HS || XR) ? 1 : CT][16];      // (XR: the heads' outputs go through Ypre like the head-split form's)
    if constexpr (!CONCAT && !HS && !XR) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) ysum[ct][r] = 0.f;
    }
#pragma unroll 1
    for (int hd = hlo; hd < hhi; ++hd) {
      MID_STAMP(0);
      // this lane's 16-byte pieces of weight row (base + lane % 32): k step ks, plane pl at + pl * plane + 16 ks + 8 fh halves
      auto wfrag = [&](long long row0, int ks, int pl) __attribute__((always_inline)) {
        if constexpr (XR)      // (row0 = 128 block + 32 tile: blocks and tiles are 64 KB / 16 KB apart)
          return *reinterpret_cast<const uint4*>(p.wfrag + row0 * 512 + (2 * ks + pl) * 1024 + lane * 16);
        else
          return *reinterpret_cast<const uint4*>(p.Hs + pl * plane + (row0 + fr) * G + 16 * ks + 8 * fh);
      };
      // operand rows of tile `tile` of the X planes
      // (only ever the wave's own tile - which is why XR can keep them in registers)
      auto xfrag = [&](int tile, int ks, int pl) __attribute__((always_inline)) {
        if constexpr (XR) return xr[ks][pl];
        else return *reinterpret_cast<const uint4*>(lds + XO + pl * XPL + (32 * tile + fr) * RS + (16 * ks + 8 * fh) * 2);
      };
      // ---- G1 (operands swapped): Q^T tile of this wave's agents, lane = agent row j, register quads = 4 consecutive columns g.
      // The weight fragments of a whole batch of column tiles (all of them; one at 128 features: 64 registers) are requested
      // before the first product: one exposed L2 round trip per batch - requested k step by k step in front of their three
      // matrix instructions, a wave (alone on its SIMD) sat out one per k step: 20 k cycles for 96 instructions at 128 features
      constexpr int WB = F == 128 ? 1 : CT;      // column tiles per weight batch
      float qss = 0.f;      // COS: this lane's share of |q_j|^2 (scaled by x_scale^2)
#pragma unroll
      for (int cb = 0; cb < CT; cb += WB) {
        uint4 wb[WB][KF][2];
#pragma unroll
        for (int c_ = 0; c_ < WB; ++c_)
#pragma unroll
          for (int ks = 0; ks < KF; ++ks) {
            wb[c_][ks][0] = wfrag((long long)hd * G + 32 * (cb + c_), ks, 0);
            wb[c_][ks][1] = wfrag((long long)hd * G + 32 * (cb + c_), ks, 1);
          }
        __builtin_amdgcn_sched_barrier(0);      // (the requests stay in front of the products: the scheduler sinks them otherwise)
#pragma unroll
        for (int c_ = 0; c_ < WB; ++c_) {
          const int ct = cb + c_;
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
          for (int ks = 0; ks < KF; ++ks) {
            const uint4 w0 = wb[c_][ks][0], w1 = wb[c_][ks][1], x0 = xfrag(w, ks, 0), x1 = xfrag(w, ks, 1);
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
            f16x3_split_cv_absmax(acc[4 * q] * kInvScale, acc[4 * q + 1] * kInvScale, hi.x, lo.x, vmax);
            f16x3_split_cv_absmax(acc[4 * q + 2] * kInvScale, acc[4 * q + 3] * kInvScale, hi.y, lo.y, vmax);
            char* o = lds + QO + myrow * RS + (32 * ct + 8 * q + 4 * fh) * 2;
            *reinterpret_cast<uint2*>(o) = hi;
            *reinterpret_cast<uint2*>(o + XPL) = lo;
          }
        }
      }
      if constexpr (COS) {      // qn[j] = 1 / (max(|q_j|, 1e-9) x_scale^2), in front of the barrier that completes the Q planes
        qss += __shfl_xor(qss, 32, 64);
        const float nq = sqrtf(qss);
        if (myrow < N && nq > 0.f && !(nq >= kMidCosTiny)) vmax = __builtin_inff();
        if (fh == 0) *reinterpret_cast<float*>(lds + QNO + 4 * myrow) = ixs * ixs / fmaxf(nq * ixs, 1e-9f);
      }
      MID_STAMP(1);
      __syncthreads();      // Q planes complete (and every wave is past the previous head's reads of the U^T region)
      MID_STAMP(2);
      // 32 features on more than 64 agents (one wave per SIMD whatever its registers: the LDS decides): the K taps' fragments -
      // 4 K register quads - are requested here, behind the barrier (which drains the request counter), and fly under G2, the
      // softmax and the A planes
      constexpr bool WEARLY = !XR && F == 32 && NT >= 3;
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
      // ---- G2: E^T[j][i] = sum_g Q[j][g] X[i][g] for this wave's columns i and ALL row tiles j; lane = column i, registers = rows j
      f32x16 e[NT];
#pragma unroll
      for (int jt = 0; jt < NT; ++jt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) e[jt][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KF; ++ks) {
          const char* qp = lds + QO + (32 * jt + fr) * RS + (16 * ks + 8 * fh) * 2;
          const uint4 q0 = *reinterpret_cast<const uint4*>(qp), q1 = *reinterpret_cast<const uint4*>(qp + XPL);
          const uint4 x0 = xfrag(w, ks, 0), x1 = xfrag(w, ks, 1);
          e[jt] = mfma16(q0, x0, e[jt]);
          e[jt] = mfma16(q0, x1, e[jt]);
          e[jt] = mfma16(q1, x0, e[jt]);
        }
      }
      MID_STAMP(3);
      if constexpr (COS) {      // rows j = 32 jt + 8 q + 4 fh + c of register 4 q + c: four qn per vector LDS read
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(lds + QNO + 4 * (32 * jt + 8 * q + 4 * fh));
#pragma unroll
            for (int c = 0; c < 4; ++c) e[jt][4 * q + c] *= qv[c] * xinv;
          }
      }
      // masked softmax of row i over its edges j (in-lane over the NT tiles + the partner lane), A planes [j][i] * 2^8
      float mx = -__builtin_inff();
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)mk[jt], 8 * (r >> 2) + (r & 3), 1);
          const float ev = e[jt][r];      // (a scalar copy: bit-casting the vector element itself reads element 0)
          const float em = __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, ev) & m) | (0xff800000u & ~m));
          e[jt][r] = em;
          mx = fmaxf(mx, em);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float cexp = mx > -__builtin_inff() ? -mx * kLog2e : 0.f;
      float sum = 0.f;
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          e[jt][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(e[jt][r], kLog2e, cexp));
          sum += e[jt][r];
        }
      sum += __shfl_xor(sum, 32, 64);
      const float inv = sum > 0.f ? 256.f / sum : 0.f;
      MID_STAMP(4);
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          unsigned ha[2], la[2];
          f16x3_split_cv(e[jt][4 * q] * inv, e[jt][4 * q + 1] * inv, ha[0], la[0]);
          f16x3_split_cv(e[jt][4 * q + 2] * inv, e[jt][4 * q + 3] * inv, ha[1], la[1]);
          char* o = lds + AO + (32 * jt + 8 * q + 4 * fh) * SA + myrow * 2;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            *reinterpret_cast<unsigned short*>(o + c * SA) = (unsigned short)(ha[c >> 1] >> (16 * (c & 1)));
            *reinterpret_cast<unsigned short*>(o + c * SA + APL) = (unsigned short)(la[c >> 1] >> (16 * (c & 1)));
          }
        }
      MID_STAMP(5);
      // ---- G3: U_k[i][c] for this wave's agents i and the K taps (lane = column c, registers = rows i).  XR: a tap's product is
      // formed when its accumulators are first needed (tap K - 1 here, tap k in front of hop k) - the same chain of products into
      // the same accumulators, but 64 instead of 192 of them live at 128 features and three taps
      f32x16 acc[KT][CT];
      auto g3 = [&](int k) __attribute__((always_inline)) {
#pragma unroll
        for (int cb = 0; cb < CT; cb += WB) {
          uint4 wb[WB][KF][2];      // (a batch of weight fragments up front, like G1)
#pragma unroll
          for (int c_ = 0; c_ < WB; ++c_)
#pragma unroll
            for (int ks = 0; ks < KF; ++ks) {
              const long long row0 = (long long)p.P * G + ((long long)hd * KT + k) * F + 32 * (cb + c_);
              if constexpr (WEARLY) { wb[c_][ks][0] = wt[k][cb + c_][ks][0]; wb[c_][ks][1] = wt[k][cb + c_][ks][1]; }
              else { wb[c_][ks][0] = wfrag(row0, ks, 0); wb[c_][ks][1] = wfrag(row0, ks, 1); }
            }
          if constexpr (!WEARLY) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int c_ = 0; c_ < WB; ++c_) {
            const int ct = cb + c_;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][ct][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KF; ++ks) {
              const uint4 w0 = wb[c_][ks][0], w1 = wb[c_][ks][1], x0 = xfrag(w, ks, 0), x1 = xfrag(w, ks, 1);
              acc[k][ct] = mfma16(x0, w0, acc[k][ct]);
              acc[k][ct] = mfma16(x0, w1, acc[k][ct]);
              acc[k][ct] = mfma16(x1, w0, acc[k][ct]);
            }
          }
        }
      };
      if constexpr (XR) g3(KT - 1);
      else {
#pragma unroll
        for (int k = 0; k < KT; ++k) g3(k);
      }
      MID_STAMP(6);
      __syncthreads();      // A planes complete; every wave is done reading the Q planes (the U^T planes take their place)
      MID_STAMP(7);
      // ---- hops (Horner): acc_k[j-tile w] += A[j][all i] U_{k+1}[all i]; the U^T planes [c][i] are rewritten from acc_{k+1}
#pragma unroll
      for (int k = KT - 2; k >= 0; --k) {
        if (k < KT - 2) __syncthreads();      // every wave is done reading the previous hop's U^T planes
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            uint2 hi, lo;
            f16x3_split_cv_absmax(acc[k + 1][ct][4 * q] * kInvScale, acc[k + 1][ct][4 * q + 1] * kInvScale, hi.x, lo.x, vmax);
            f16x3_split_cv_absmax(acc[k + 1][ct][4 * q + 2] * kInvScale, acc[k + 1][ct][4 * q + 3] * kInvScale, hi.y, lo.y, vmax);
            char* o = lds + UO + (32 * ct + fr) * SA + (32 * w + 8 * q + 4 * fh) * 2;
            *reinterpret_cast<uint2*>(o) = hi;
            *reinterpret_cast<uint2*>(o + UPL) = lo;
          }
        if constexpr (XR) g3(k);
        __syncthreads();      // U^T planes complete
#pragma unroll
        for (int ks = 0; ks < 2 * NT; ++ks) {
          const char* ap = lds + AO + myrow * SA + (16 * ks + 8 * fh) * 2;
          const uint4 a0 = *reinterpret_cast<const uint4*>(ap), a1 = *reinterpret_cast<const uint4*>(ap + APL);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const char* up = lds + UO + (32 * ct + fr) * SA + (16 * ks + 8 * fh) * 2;
            const uint4 u0 = *reinterpret_cast<const uint4*>(up), u1 = *reinterpret_cast<const uint4*>(up + UPL);
            acc[k][ct] = mfma16(a0, u0, acc[k][ct]);
            acc[k][ct] = mfma16(a0, u1, acc[k][ct]);
            acc[k][ct] = mfma16(a1, u0, acc[k][ct]);
          }
        }
      }
      MID_STAMP(8);
      // ---- epilogue: lane = column c, registers = rows j of this wave's tile
      float* yb = p.Y + (long long)inst * N * p.ldy;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * w + 8 * (r >> 2) + 4 * fh + (r & 3);
          const float v = __builtin_fmaf(acc[0][ct][r], kOutScale, biasv[ct]);
          if constexpr (CONCAT) {
            if (j < N) yb[(long long)j * p.ldy + hd * F + 32 * ct + fr] = __builtin_amdgcn_fmed3f(v, 0.f, __builtin_inff());
          } else if constexpr (HS || XR) {
            if (j < N) p.Ypre[((long long)inst * N + j) * p.ldpre + hd * F + 32 * ct + fr] = v;
          } else {
            ysum[ct][r] += v;      // (graphML.py:4663-4667: mean over the heads, then ReLU)
            if (hd == p.P - 1 && j < N)
              yb[(long long)j * p.ldy + 32 * ct + fr] = __builtin_amdgcn_fmed3f(ysum[ct][r] / (float)p.P, 0.f, __builtin_inff());
          }
        }
      MID_STAMP(9);
      __syncthreads();      // every wave is done with this head's U^T / A planes (the next head's G1 writes the Q planes)
      MID_STAMP(10);
    }
  }
  if (p.range_flag && vmax > 65504.f) atomicOr(p.range_flag, 1);
