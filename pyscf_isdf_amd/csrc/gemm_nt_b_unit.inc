// Body of one work unit of variant B (gemm_f64.hip): output tile (tm, tn) over K slab `slab` of the GemmArgs g, with sA / sB the
// workgroup's LDS buffers.  Included as text by gemm_nt_mfma_kernel_b and gram_tri_mfma_kernel, which differ only in how a
// workgroup finds its unit: the W product's kernel compiles to the same code as before the second user existed.
  const int64_t k0 = (int64_t)slab * g.kslab;
  const int64_t k1 = (k0 + g.kslab < g.K) ? k0 + g.kslab : g.K;
  const int nchunks = (int)((k1 - k0) / BK);            // even
  const int last = nchunks - 1;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;              // 4 x 2 waves, 64x64 each
  const int srow = tid >> 3;                            // 0..63
  const int sseg = tid & 7;
  const int mlast = g.M - 1, nlast = g.N - 1;
  // six row pointers (A: rows srow + 64 i, B: rows srow + 64 i), clamped at the matrix edge
  const double* pA0 = g.A + (int64_t)min(tm * BM2 + srow, mlast) * g.lda + k0 + sseg * 2;
  const double* pA1 = g.A + (int64_t)min(tm * BM2 + srow + 64, mlast) * g.lda + k0 + sseg * 2;
  const double* pA2 = g.A + (int64_t)min(tm * BM2 + srow + 128, mlast) * g.lda + k0 + sseg * 2;
  const double* pA3 = g.A + (int64_t)min(tm * BM2 + srow + 192, mlast) * g.lda + k0 + sseg * 2;
  const double* pB0 = g.B + (int64_t)min(tn * BN + srow, nlast) * g.ldb + k0 + sseg * 2;
  const double* pB1 = g.B + (int64_t)min(tn * BN + srow + 64, nlast) * g.ldb + k0 + sseg * 2;
  const double* pS = SCALED ? g.kscale + k0 + sseg * 2 : nullptr;

  double2 xa0, xa1, xa2, xa3, xb0, xb1, ya0, ya1, ya2, ya3, yb0, yb1;
#define ISDF_LOADB(C, A0, A1, A2, A3, B0, B1)                                                 \
  {                                                                                           \
    const int off = (C) * BK;                                                                 \
    A0 = *reinterpret_cast<const double2*>(pA0 + off);                                        \
    A1 = *reinterpret_cast<const double2*>(pA1 + off);                                        \
    A2 = *reinterpret_cast<const double2*>(pA2 + off);                                        \
    A3 = *reinterpret_cast<const double2*>(pA3 + off);                                        \
    B0 = *reinterpret_cast<const double2*>(pB0 + off);                                        \
    B1 = *reinterpret_cast<const double2*>(pB1 + off);                                        \
    if (SCALED) {                                                                             \
      const double2 sc = *reinterpret_cast<const double2*>(pS + off);                         \
      B0.x *= sc.x; B0.y *= sc.y; B1.x *= sc.x; B1.y *= sc.y;                                 \
    }                                                                                         \
  }
#define ISDF_ST1(P, R) { double* q_ = (P); q_[0] = R.x; q_[1] = R.y; }
#define ISDF_STOREB(BUF, A0, A1, A2, A3, B0, B1)                                              \
  {                                                                                           \
    double* qa = sA + (BUF) * BM2 * LDT + srow * LDT + sseg * 2;                              \
    double* qb = sB + (BUF) * BN * LDT + srow * LDT + sseg * 2;                               \
    ISDF_ST1(qa, A0) ISDF_ST1(qa + 64 * LDT, A1) ISDF_ST1(qa + 128 * LDT, A2)                 \
    ISDF_ST1(qa + 192 * LDT, A3) ISDF_ST1(qb, B0) ISDF_ST1(qb + 64 * LDT, B1)                 \
  }

  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  const int frow = lane & 15, fk = lane >> 4;

#define ISDF_FRAGB(KK, AF, BF)                                                                \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                           \
      AF[i] = pa[i * 16 * LDT + (KK) * 4];                                                    \
      BF[i] = pb[i * 16 * LDT + (KK) * 4];                                                    \
    }
#define ISDF_MFMAB(AF, BF)                                                                    \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                             \
      _Pragma("unroll") for (int j = 0; j < 4; ++j)                                           \
        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(AF[i], BF[j], acc[i][j], 0, 0, 0);
  // issue order inside a k-step region: one LDS fragment read (of the NEXT k-step) after every second MFMA, so that the
  // reads trickle in under the MFMAs instead of in one burst (+1%); the LDS writes of the next chunk are spread the same
  // way over the last k-step, which leaves only the barrier at the end of the chunk
#define ISDF_INTERLEAVE() _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) {                  \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
#define ISDF_INTERLEAVE_W() _Pragma("unroll") for (int q_ = 0; q_ < 6; ++q_) {                \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); }
  // first k-step: the six global loads of the chunk after next ride along (one per MFMA pair, after the fragment read)
#define ISDF_INTERLEAVE_L() _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) {                \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                \
    if (q_ < 6) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); }
  // exactly two fragment sets live (the scheduler would otherwise hoist all four k-steps' reads and
  // spill): reads of k-step kk+1 are issued before the MFMAs of kk, fenced by sched_barrier
  // One chunk = four k-steps.  Fragment sets alternate (k0: set 0, k1: set 1, k2: set 0, k3: set 1); each region issues
  // the LDS reads of the NEXT k-step under its own MFMAs.  The chunk's single barrier sits after k-step 2: by then every
  // wave has issued and completed (s_waitcnt in __syncthreads) all its reads of the current buffer and has written its
  // part of the next one, so k-step 3 can already prefetch the first fragments of the next chunk from the other buffer
  // and the MFMA stream runs across the chunk boundary without the post-barrier bubble.  A wave can only reach the next
  // chunk's writes of this buffer after passing this barrier, i.e. after all waves finished reading it.
  const int aoff = (wm * 64 + frow) * LDT + fk, boff = (wn * 64 + frow) * LDT + fk;
  double a0[4], b0[4], a1[4], b1[4];
#define ISDF_FRAGQ(BUF, KK, AF, BF)                                                           \
  {                                                                                           \
    const double* pa = sA + (BUF) * BM2 * LDT + aoff;                                         \
    const double* pb = sB + (BUF) * BN * LDT + boff;                                          \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                           \
      AF[i] = pa[i * 16 * LDT + (KK) * 4];                                                    \
      BF[i] = pb[i * 16 * LDT + (KK) * 4];                                                    \
    }                                                                                         \
  }
#define ISDF_INTERLEAVE_RW() _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) {               \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                \
    if (q_ < 6) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); }
#define ISDF_CHUNKB(BUF, LOAD_AHEAD, STORE_NEXT)                                              \
  {                                                                                           \
    ISDF_FRAGQ(BUF, 1, a1, b1)                                                                \
    LOAD_AHEAD                                                                                \
    ISDF_MFMAB(a0, b0)                                                                        \
    ISDF_INTERLEAVE_L()                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_FRAGQ(BUF, 2, a0, b0)                                                                \
    ISDF_MFMAB(a1, b1)                                                                        \
    ISDF_INTERLEAVE()                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_FRAGQ(BUF, 3, a1, b1)                                                                \
    STORE_NEXT                                                                                \
    ISDF_MFMAB(a0, b0)                                                                        \
    ISDF_INTERLEAVE_RW()                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    __syncthreads();                                                                          \
    ISDF_FRAGQ(1 - (BUF), 0, a0, b0)                                                          \
    ISDF_MFMAB(a1, b1)                                                                        \
    ISDF_INTERLEAVE()                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                        \
  }

  // prologue: chunk 0 -> LDS buffer 0; chunk 1 in flight in set Y; first fragments of chunk 0
  ISDF_LOADB(0, xa0, xa1, xa2, xa3, xb0, xb1)
  ISDF_LOADB(1, ya0, ya1, ya2, ya3, yb0, yb1)
  ISDF_STOREB(0, xa0, xa1, xa2, xa3, xb0, xb1)
  __syncthreads();
  ISDF_FRAGQ(0, 0, a0, b0)
  __builtin_amdgcn_sched_barrier(0);
  // steady state, two chunks per iteration: while chunk c computes, chunk c+1 sits in registers and
  // chunk c+2 is being loaded, so every load has two chunks of MFMAs to land
  for (int c = 0; c < nchunks; c += 2) {
    ISDF_CHUNKB(0, ISDF_LOADB(min(c + 2, last), xa0, xa1, xa2, xa3, xb0, xb1), ISDF_STOREB(1, ya0, ya1, ya2, ya3, yb0, yb1))
    ISDF_CHUNKB(1, ISDF_LOADB(min(c + 3, last), ya0, ya1, ya2, ya3, yb0, yb1), ISDF_STOREB(0, xa0, xa1, xa2, xa3, xb0, xb1))
  }

  double* out = g.P + (int64_t)slab * g.slab_stride;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = tm * BM2 + wm * 64 + i * 16 + (lane >> 4) + 4 * r;
      if (row >= g.M) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = tn * BN + wn * 64 + j * 16 + (lane & 15);
        if (col >= g.N) continue;
        double* q = out + (int64_t)row * g.ldp + col;
        const double v = acc[i][j][r];
        if (g.direct) *q = (g.beta == 0.0) ? g.alpha * v : g.alpha * v + g.beta * (*q);
        else *q = v;
      }
    }
  }
