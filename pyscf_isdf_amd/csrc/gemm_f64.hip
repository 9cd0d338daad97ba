// Dense FP64 products for the ISDF path.
//  * gemm_rm: row-major wrapper over rocBLAS dgemm for the well-shaped products (rocBLAS reaches
//    70-74 TF/s of the 78.6 TF/s FP64 MFMA peak on them: profiles/r01_probe_rocblas_hipfft_mfma64.log).
//  * gemm_nt_f64: C = alpha * A * (B .* kscale)^T + beta * C with K contiguous in BOTH operands and
//    K >> M, N — the shape of W = V Theta^T (K = ngrids) and of vj = ao (v .* ao)^T.  rocBLAS runs
//    this shape at 13-34 TF/s (profiles/r01_gemm_variants.log), so it gets hand-written v_mfma_f64_16x16x4_f64
//    kernels - three variants share the work-unit scheme below (the launcher picks: B when M fills 256-row tiles,
//    D for other aligned operands, A for unaligned ones; 69 TF/s = 0.88 of peak on the W product):
//      - A: 128x128 output tile per 256-thread workgroup, each wave a 64x64 sub-tile = 4x4 MFMA
//        accumulators (128 VGPRs), both operands through LDS;  B: 256x128, 8 waves, one workgroup per CU;
//        D: 128x128, A operand straight from global memory into MFMA registers, only B through LDS;
//      - K is cut into slabs; one work unit = (slab, tile).  Units are ordered slab-major with the
//        row tile fastest so that workgroups that share an operand panel run at the same time, and
//        the block id is remapped so that such neighbours land on the same XCD (its L2);
//      - operands are staged global -> registers -> LDS in 16-deep K chunks (one full 128-B line per
//        row per chunk), double buffered, rows padded to 136 B so that the ds_read_b64 fragment
//        reads are bank-conflict free;
//      - partial tiles of the slabs go to a workspace and are summed in a fixed order (deterministic,
//        no float atomics);
//      - B and D: the instruction ORDER inside a chunk is pinned with sched_group_barrier - one LDS read (of the next
//        k-step), LDS write (of the next chunk) or global load (of the chunk after next) after every second MFMA, the
//        chunk's single barrier after k-step 2, the next chunk's first fragments prefetched under k-step 3.  Worth
//        64 -> 69 TF/s, and it keeps co-scheduled workgroups in step so that shared operand panels hit in L2 (fabric
//        traffic 3.9x -> 1.3x the algorithmic bytes).
//    Algorithmic work: 2*M*N*K flop; bound: FP64 MFMA (78.6 TF/s).
//  * gemm_nt_had3: C_a += alpha (A o H) B_a^T for three B_a in one launch (the exchange derivative's T_a): variant D with the
//    factor H multiplied into the A operand registers and a 128 x 32 tile of all three components per unit.
//  * gemm_nn_had: C = alpha A (H o B) + beta C (the contracted exchange force's Z): the NN form's unit body with the factor H
//    multiplied into the B staging registers, alpha and beta in the epilogue, any M >= 1 (waves past the row edge only stage).
//  * Every kernel finds its unit with xcd_unit / decode_tile / slab_range (the NN form: decode_supertile) and stores its
//    accumulators with ISDF_STORE_ACC.  Variant B's unit body, tile_256x128, is a function template that leaves the tile in
//    accumulator registers: gemm_nt_mfma_kernel_b and the Gram triangles are that body between two ways of finding a unit
//    and of storing it, and a new user writes a kernel that decodes its unit, calls it and stores.  The NN form keeps a main
//    loop of its own: as a B-operand policy of tile_256x128 it compiled to another loop than the one measured.
#include "common.h"
#include "gemm_tile.h"
#include <cstdlib>

int gemm_rm(isdf_handle h, char opA, char opB, int64_t M, int64_t N, int64_t K, double alpha,
            const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
            int64_t ldc) {
  // Row-major C = op(A) op(B)  <=>  column-major C^T = op(B)^T op(A)^T.
  ARG_CHECK(h, M < 2147483647LL && N < 2147483647LL && K < 2147483647LL && lda < 2147483647LL &&
                   ldb < 2147483647LL && ldc < 2147483647LL);
  const rocblas_operation ta = (opA == 'N') ? rocblas_operation_none : rocblas_operation_transpose;
  const rocblas_operation tb = (opB == 'N') ? rocblas_operation_none : rocblas_operation_transpose;
  ProfScope ps(h, "rocblas_dgemm[flop]", 2.0 * M * N * (double)K);
  BLAS_TRY(h, rocblas_dgemm(h->blas, tb, ta, (rocblas_int)N, (rocblas_int)M, (rocblas_int)K, &alpha, B,
                            (rocblas_int)ldb, A, (rocblas_int)lda, &beta, C, (rocblas_int)ldc));
  return ISDF_OK;
}

namespace {

constexpr int BM = 128, BN = 128, BK = 16;
constexpr int LDT = 17;          // doubles per LDS row: 16 + 1 pad (136 B = 34 banks): the fragment reads (ds_read2_b64,
                                 // banked mod 32 in 16-lane groups) hit 16 distinct bank pairs
constexpr int TPB = 256;

struct GemmArgs {
  const double* A; int64_t lda;
  const double* B; int64_t ldb;
  const double* kscale;          // optional per-k scale applied to B (nullptr: none)
  double* P;                     // partials [nslab][M][N] (or C itself when nslab == 1 && direct)
  int64_t ldp, slab_stride;
  int M, N;
  int64_t K, kslab;              // kslab multiple of BK
  int ntm, ntn, nslab;
  int64_t nunits, nunits_pad;    // nunits_pad: rounded up to a multiple of 8 (XCD remap)
  double alpha, beta;            // used only when direct
  int direct;
};

// unit decode (xcd_unit / decode_tile / slab_range) and accumulator store (ISDF_STORE_ACC): gemm_tile.h, shared with thc.hip
// STORE of the NT kernels: the slab's partial tile, or C itself (direct) with alpha and beta
#define ISDF_SLAB_STORE                                                                       \
  {                                                                                           \
    double* q = out + (int64_t)row * g.ldp + col;                                             \
    const double v = acc[i][j][r];                                                            \
    if (g.direct) *q = (g.beta == 0.0) ? g.alpha * v : g.alpha * v + g.beta * (*q);           \
    else *q = v;                                                                              \
  }

// 16 MFMAs of one k-step of a 4 x 4 accumulator block
#define ISDF_MFMA16(AF, BF)                                                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                             \
      _Pragma("unroll") for (int j = 0; j < 4; ++j)                                           \
        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(AF[i], BF[j], acc[i][j], 0, 0, 0);
// issue order inside a k-step region (variants B and D, NN): one LDS fragment read (of the NEXT k-step) after every second MFMA,
// so that the reads trickle in under the MFMAs instead of in one burst (+1%); the first NX of the eight rounds carry one more
// instruction of class XMASK (0x020: a global load of the chunk after next, 0x200: an LDS write of the next chunk), which
// leaves only the barrier at the end of the chunk.  (0, 0) = no extra instruction: the mask of a round that never comes is
// not read (the dead branch folds away once the loop is unrolled)
#define ISDF_ISSUE(XMASK, NX) _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) {              \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                \
    if (q_ < (NX)) __builtin_amdgcn_sched_group_barrier(XMASK, 1, 0); }

// FAST: lda, ldb even (16-byte aligned rows given 16-byte aligned bases) and no K tail handling
// needed inside a chunk (K % BK == 0).  Otherwise the generic path loads element-wise with guards.
template <bool FAST>
__global__ __launch_bounds__(TPB, 2) void gemm_nt_mfma_kernel(GemmArgs g) {
  __shared__ double sA[2][BM * LDT];
  __shared__ double sB[2][BN * LDT];

  const int64_t unit = xcd_unit(g.nunits_pad);
  if (unit >= g.nunits) return;
  const Tile t = decode_tile(unit, g.ntm, g.ntn);
  const KRange kr = slab_range(t.slab, g.kslab, g.K);
  const int64_t k0 = kr.k0, k1 = kr.k1;
  const int nchunks = (int)((k1 - k0 + BK - 1) / BK);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // staging map: piece p = tid + 256*i, i < 4: row = p / 8, 16-byte segment = p % 8
  const int srow = tid >> 3;            // 0..31, +32*i
  const int sseg = tid & 7;             // k offset sseg*2
  // row offsets are recomputed per chunk (cheap next to 64 MFMAs) instead of keeping 8 pointers live;
  // out-of-range rows are clamped: they are computed but never stored
  const int arow0 = t.tm * BM + srow, brow0 = t.tn * BN + srow;
  const int mlast = g.M - 1, nlast = g.N - 1;
  const double* __restrict__ Ag = g.A;
  const double* __restrict__ Bg = g.B;
  const int64_t lda = g.lda, ldb = g.ldb;

  // staging registers as named scalars (arrays captured by the helpers below ended up in scratch)
  double2 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
#define ISDF_LOAD_ONE(I, RA, RB)                                                              \
  {                                                                                           \
    const int ra = min(arow0 + 32 * I, mlast), rb = min(brow0 + 32 * I, nlast);               \
    const double* pa = Ag + (int64_t)ra * lda + k;                                            \
    const double* pb = Bg + (int64_t)rb * ldb + k;                                            \
    if (FAST) {                                                                               \
      RA = *reinterpret_cast<const double2*>(pa);                                             \
      RB = *reinterpret_cast<const double2*>(pb);                                             \
    } else {                                                                                  \
      RA.x = v0 ? pa[0] : 0.0; RA.y = v1 ? pa[1] : 0.0;                                       \
      RB.x = v0 ? pb[0] : 0.0; RB.y = v1 ? pb[1] : 0.0;                                       \
    }                                                                                         \
    RB.x *= s0; RB.y *= s1;                                                                   \
  }
#define ISDF_LOAD_CHUNK(C)                                                                    \
  {                                                                                           \
    const int64_t k = k0 + (int64_t)(C) * BK + sseg * 2;                                      \
    const bool v0 = FAST || (k < k1), v1 = FAST || (k + 1 < k1);                              \
    double s0 = 1.0, s1 = 1.0;                                                                \
    if (g.kscale) { if (v0) s0 = g.kscale[k]; if (v1) s1 = g.kscale[k + 1]; }                 \
    ISDF_LOAD_ONE(0, ra0, rb0) ISDF_LOAD_ONE(1, ra1, rb1)                                     \
    ISDF_LOAD_ONE(2, ra2, rb2) ISDF_LOAD_ONE(3, ra3, rb3)                                     \
  }
#define ISDF_STORE_ONE(BUF, I, RA, RB)                                                        \
  { double* qa = &sA[BUF][(srow + 32 * I) * LDT + sseg * 2];                                  \
    double* qb = &sB[BUF][(srow + 32 * I) * LDT + sseg * 2];                                  \
    qa[0] = RA.x; qa[1] = RA.y; qb[0] = RB.x; qb[1] = RB.y; }
#define ISDF_STORE_CHUNK(BUF)                                                                 \
  { ISDF_STORE_ONE(BUF, 0, ra0, rb0) ISDF_STORE_ONE(BUF, 1, ra1, rb1)                         \
    ISDF_STORE_ONE(BUF, 2, ra2, rb2) ISDF_STORE_ONE(BUF, 3, ra3, rb3) }

  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

  const int frow = lane & 15, fk = lane >> 4;
  ISDF_LOAD_CHUNK(0)
  ISDF_STORE_CHUNK(0)
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) ISDF_LOAD_CHUNK(c + 1)
    const double* pa = &sA[buf][(wm * 64 + frow) * LDT + fk];
    const double* pb = &sB[buf][(wn * 64 + frow) * LDT + fk];
    // fragments of k-step kk+1 are fetched from LDS while the 16 MFMAs of k-step kk run
    double a0[4], b0[4], a1[4], b1[4];
#define ISDF_FRAGS(KK, AF, BF)                                                                \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                           \
      AF[i] = pa[i * 16 * LDT + (KK) * 4];                                                    \
      BF[i] = pb[i * 16 * LDT + (KK) * 4];                                                    \
    }
    ISDF_FRAGS(0, a0, b0)
    ISDF_FRAGS(1, a1, b1)
    ISDF_MFMA16(a0, b0)
    ISDF_FRAGS(2, a0, b0)
    ISDF_MFMA16(a1, b1)
    ISDF_FRAGS(3, a1, b1)
    ISDF_MFMA16(a0, b0)
    ISDF_MFMA16(a1, b1)
    if (c + 1 < nchunks) ISDF_STORE_CHUNK(buf ^ 1)
    __syncthreads();
  }
  double* out = g.P + (int64_t)t.slab * g.slab_stride;
  ISDF_STORE_ACC(4, 4, t.tm * BM + wm * 64, t.tn * BN + wn * 64, g.M, g.N, ISDF_SLAB_STORE)
#undef ISDF_LOAD_ONE
#undef ISDF_LOAD_CHUNK
#undef ISDF_STORE_ONE
#undef ISDF_STORE_CHUNK
#undef ISDF_FRAGS
}

// ---- variant B: 256x128 tile, 8 waves (one workgroup per CU), operand loads two chunks ahead ------
// Motivation (profiles/r01_pmc_gemm_nt_mfma_v1.json): with 128x128 tiles every workgroup streams its
// operands from the fabric (sharers run in lockstep and all miss in L2), and the single register
// staging set gives a load only one chunk of MFMAs (~3.5 us) to land: ~14% of the time is spent in
// s_waitcnt vmcnt(0).  Here the B panel is shared by twice as many rows inside the workgroup, and two
// staging register sets keep TWO chunks of loads in flight.
constexpr int BM2 = 256;
constexpr int TPB2 = 512;

// One work unit of variant B: output tile (tm, tn) of A (M rows) times B^T (N rows), both with K contiguous, over nchunks
// 16-deep chunks from k0, into acc (the wave's 64 x 64 part: 4 x 2 waves, see ISDF_STORE_ACC).  Aligned path only: an even
// number of chunks, 16-byte aligned rows.  No conditionals in the main loop: the tail re-loads the last chunk.
// smem: [2][BM2*LDT] A | [2][BN*LDT] B.
template <bool SCALED>
__device__ __forceinline__ void tile_256x128(const double* A, int64_t lda, const double* B, int64_t ldb, const double* kscale,
                                             int M, int N, int tm, int tn, int64_t k0, int nchunks, double* smem, d4 (&acc)[4][4]) {
  double* sA = smem;
  double* sB = smem + 2 * BM2 * LDT;
  const int last = nchunks - 1;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;              // 4 x 2 waves, 64x64 each
  const int srow = tid >> 3;                            // 0..63
  const int sseg = tid & 7;
  const int mlast = M - 1, nlast = N - 1;
  // six row pointers (A: rows srow + 64 i, B: rows srow + 64 i), clamped at the matrix edge
  const double* pA0 = A + (int64_t)min(tm * BM2 + srow, mlast) * lda + k0 + sseg * 2;
  const double* pA1 = A + (int64_t)min(tm * BM2 + srow + 64, mlast) * lda + k0 + sseg * 2;
  const double* pA2 = A + (int64_t)min(tm * BM2 + srow + 128, mlast) * lda + k0 + sseg * 2;
  const double* pA3 = A + (int64_t)min(tm * BM2 + srow + 192, mlast) * lda + k0 + sseg * 2;
  const double* pB0 = B + (int64_t)min(tn * BN + srow, nlast) * ldb + k0 + sseg * 2;
  const double* pB1 = B + (int64_t)min(tn * BN + srow + 64, nlast) * ldb + k0 + sseg * 2;
  const double* pS = SCALED ? kscale + k0 + sseg * 2 : nullptr;

  // staging registers as named scalars (arrays captured by helpers ended up in scratch)
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

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  const int frow = lane & 15, fk = lane >> 4;

  // exactly two fragment sets live (the scheduler would otherwise hoist all four k-steps' reads and
  // spill): reads of k-step kk+1 are issued before the MFMAs of kk, fenced by sched_barrier
  // One chunk = four k-steps.  Fragment sets alternate (k0: set 0, k1: set 1, k2: set 0, k3: set 1); each region issues
  // the LDS reads of the NEXT k-step under its own MFMAs (ISDF_ISSUE); the six global loads of the chunk after next ride
  // along in the first k-step and the LDS writes of the next chunk in the third.  The chunk's single barrier sits after
  // k-step 2: by then every wave has issued and completed (s_waitcnt in __syncthreads) all its reads of the current buffer
  // and has written its part of the next one, so k-step 3 can already prefetch the first fragments of the next chunk from
  // the other buffer and the MFMA stream runs across the chunk boundary without the post-barrier bubble.  A wave can only
  // reach the next chunk's writes of this buffer after passing this barrier, i.e. after all waves finished reading it.
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
#define ISDF_CHUNKB(BUF, LOAD_AHEAD, STORE_NEXT)                                              \
  {                                                                                           \
    ISDF_FRAGQ(BUF, 1, a1, b1)                                                                \
    LOAD_AHEAD                                                                                \
    ISDF_MFMA16(a0, b0)                                                                       \
    ISDF_ISSUE(0x020, 6)                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_FRAGQ(BUF, 2, a0, b0)                                                                \
    ISDF_MFMA16(a1, b1)                                                                       \
    ISDF_ISSUE(0, 0)                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_FRAGQ(BUF, 3, a1, b1)                                                                \
    STORE_NEXT                                                                                \
    ISDF_MFMA16(a0, b0)                                                                       \
    ISDF_ISSUE(0x200, 6)                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    __syncthreads();                                                                          \
    ISDF_FRAGQ(1 - (BUF), 0, a0, b0)                                                          \
    ISDF_MFMA16(a1, b1)                                                                       \
    ISDF_ISSUE(0, 0)                                                                          \
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
#undef ISDF_LOADB
#undef ISDF_ST1
#undef ISDF_STOREB
#undef ISDF_FRAGQ
#undef ISDF_CHUNKB
}

template <bool SCALED>
__global__ __launch_bounds__(TPB2, 2) void gemm_nt_mfma_kernel_b(GemmArgs g) {
  // K % 32 == 0, kslab % 32 == 0: an even number of 16-deep chunks per slab
  extern __shared__ double smem[];
  const int64_t unit = xcd_unit(g.nunits_pad);
  if (unit >= g.nunits) return;
  const Tile t = decode_tile(unit, g.ntm, g.ntn);
  const KRange kr = slab_range(t.slab, g.kslab, g.K);
  d4 acc[4][4];
  tile_256x128<SCALED>(g.A, g.lda, g.B, g.ldb, g.kscale, g.M, g.N, t.tm, t.tn, kr.k0, (int)((kr.k1 - kr.k0) / BK), smem, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* out = g.P + (int64_t)t.slab * g.slab_stride;
  ISDF_STORE_ACC(4, 4, t.tm * BM2 + (wave >> 1) * 64, t.tn * BN + (wave & 1) * 64, g.M, g.N, ISDF_SLAB_STORE)
}

// ---- grouped block-lower Gram triangles S_b = X_b X_b^T for the candidate selection (select_ip.hip) -----------------------
// X (rows = grid points of consecutive blocks, K contiguous, zero-padded to a multiple of 32).  One launch covers every
// (block, tile row, tile column) unit of a group of blocks; a unit is one 256 x 128 tile of variant B over the WHOLE K with
// accumulators starting at zero and k strictly ascending, so an entry is the k-ordered fma chain of the scalar dot product.
// Tile row tm of a block is stored as 256 rows of (tm + 1) * 256 columns, tile rows back to back (gram_tri_row, common.h).
struct GramTriArgs {
  const double* X; int64_t ldx; int K;
  const GramTriUnit* units;
  const int64_t* blk_off;        // absolute point offsets of the blocks; X row 0 is point row0
  int64_t row0;
  const int64_t* tri_off;        // per block: offset of its triangle in S (doubles)
  double* S;
  int64_t nunits, nunits_pad;
};

__global__ __launch_bounds__(TPB2, 2) void gram_tri_mfma_kernel(GramTriArgs t) {
  extern __shared__ double smem[];
  const int64_t unit = xcd_unit(t.nunits_pad);
  if (unit >= t.nunits) return;
  const GramTriUnit u = t.units[unit];
  const int64_t r0 = t.blk_off[u.blk];
  const double* X = t.X + (r0 - t.row0) * t.ldx;
  const int m = (int)(t.blk_off[u.blk + 1] - r0);
  // row r of the tile row sits at gram_tri_row(r) = gram_tri_row(256 tm) + (r - 256 tm) * ldp: the unit addresses rows by r
  const int64_t ldp = (int64_t)(u.tm + 1) * BM2;
  double* S = t.S + t.tri_off[u.blk] + (gram_tri_row((int64_t)u.tm * BM2) - (int64_t)u.tm * BM2 * ldp);
  d4 acc[4][4];
  tile_256x128<false>(X, t.ldx, X, t.ldx, nullptr, m, m, u.tm, u.tn, 0, t.K / BK, smem, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  ISDF_STORE_ACC(4, 4, u.tm * BM2 + (wave >> 1) * 64, u.tn * BN + (wave & 1) * 64, m, m, S[(int64_t)row * ldp + col] = acc[i][j][r];)
}

// ---- variant D: A straight from global memory into MFMA operand registers, only B through LDS ----------------------
// 128 x 128 tile, four waves stacked along M (each 32 rows x all 128 columns: 2 x 8 accumulators), two workgroups per
// CU.  The rows of A are private to a wave, so staging them through LDS buys nothing: lane (r = lane & 15, kq = lane >> 4)
// loads A[row r][16 c + 4 kq .. + 3] (32 contiguous bytes; the four kq lanes of a row cover one 128-byte line) and uses
// element j in the j-th MFMA of the chunk.  That permutes the order of the k index inside a 16-deep chunk
// (k = 4 kq + j instead of 4 j + kq) - the B fragments are read from LDS with the same map, the sum is the same set of
// products.  Only B (128 rows x 16) is written to LDS: a third of variant B's LDS writes per flop, 35 KB of LDS per
// workgroup, and the two resident workgroups hide each other's barrier.
constexpr int TPBD = 256;

template <bool SCALED>
__global__ __launch_bounds__(TPBD, 2) void gemm_nt_mfma_kernel_d(GemmArgs g) {
  __shared__ double sB[2][BN * LDT];
  const int64_t unit = xcd_unit(g.nunits_pad);
  if (unit >= g.nunits) return;
  const Tile t = decode_tile(unit, g.ntm, g.ntn);
  const int tm = t.tm, tn = t.tn;
  const KRange kr = slab_range(t.slab, g.kslab, g.K);
  const int64_t k0 = kr.k0;
  const int nchunks = (int)((kr.k1 - k0) / BK);         // even (kslab is a multiple of 2 BK, K % 32 == 0)
  const int last = nchunks - 1;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 15, fkq = lane >> 4;
  const int mlast = g.M - 1, nlast = g.N - 1;
  // A: two 16-row groups of this wave's 32 rows; four consecutive k per lane
  const double* pA0 = g.A + (int64_t)min(tm * BM + wave * 32 + frow, mlast) * g.lda + k0 + 4 * fkq;
  const double* pA1 = g.A + (int64_t)min(tm * BM + wave * 32 + 16 + frow, mlast) * g.lda + k0 + 4 * fkq;
  // B staging: 128 rows x 16 doubles per chunk = 8 doubles per thread: rows srow and srow + 64, k offset 4 sseg .. + 3
  const int srow = tid >> 2, sseg = tid & 3;
  const double* pB0 = g.B + (int64_t)min(tn * BN + srow, nlast) * g.ldb + k0 + 4 * sseg;
  const double* pB1 = g.B + (int64_t)min(tn * BN + srow + 64, nlast) * g.ldb + k0 + 4 * sseg;
  const double* pS = SCALED ? g.kscale + k0 + 4 * sseg : nullptr;

  // register sets: X / Y alternate between chunks (A operands + B staging)
  double2 xa00, xa01, xa10, xa11, xb00, xb01, xb10, xb11;
  double2 ya00, ya01, ya10, ya11, yb00, yb01, yb10, yb11;
#define ISDF_LOADD(C, A00, A01, A10, A11, B00, B01, B10, B11)                                 \
  {                                                                                           \
    const int off = (C) * BK;                                                                 \
    A00 = *reinterpret_cast<const double2*>(pA0 + off);                                       \
    A01 = *reinterpret_cast<const double2*>(pA0 + off + 2);                                   \
    A10 = *reinterpret_cast<const double2*>(pA1 + off);                                       \
    A11 = *reinterpret_cast<const double2*>(pA1 + off + 2);                                   \
    B00 = *reinterpret_cast<const double2*>(pB0 + off);                                       \
    B01 = *reinterpret_cast<const double2*>(pB0 + off + 2);                                   \
    B10 = *reinterpret_cast<const double2*>(pB1 + off);                                       \
    B11 = *reinterpret_cast<const double2*>(pB1 + off + 2);                                   \
    if (SCALED) {                                                                             \
      const double2 s0 = *reinterpret_cast<const double2*>(pS + off);                         \
      const double2 s1 = *reinterpret_cast<const double2*>(pS + off + 2);                     \
      B00.x *= s0.x; B00.y *= s0.y; B01.x *= s1.x; B01.y *= s1.y;                             \
      B10.x *= s0.x; B10.y *= s0.y; B11.x *= s1.x; B11.y *= s1.y;                             \
    }                                                                                         \
  }
#define ISDF_STORED(BUF, B00, B01, B10, B11)                                                  \
  {                                                                                           \
    double* q0 = &sB[BUF][srow * LDT + 4 * sseg];                                             \
    double* q1 = &sB[BUF][(srow + 64) * LDT + 4 * sseg];                                      \
    q0[0] = B00.x; q0[1] = B00.y; q0[2] = B01.x; q0[3] = B01.y;                               \
    q1[0] = B10.x; q1[1] = B10.y; q1[2] = B11.x; q1[3] = B11.y;                               \
  }

  d4 acc[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

  // Same issue order as variant B: the B fragments of the NEXT k-step are read from LDS under the MFMAs of the current one
  // (two fragment sets), the chunk's single barrier sits after k-step 2, and k-step 3 already prefetches the first
  // fragments of the next chunk from the other buffer.
  double bf0[8], bf1[8];
#define ISDF_FRAGD(BUF, J, BF)                                                                \
  {                                                                                           \
    const double* pb = &sB[BUF][frow * LDT + 4 * fkq + (J)];                                  \
    _Pragma("unroll") for (int jn = 0; jn < 8; ++jn) BF[jn] = pb[jn * 16 * LDT];              \
  }
#define ISDF_MFMAD(AV0, AV1, BF)                                                              \
    _Pragma("unroll") for (int jn = 0; jn < 8; ++jn) {                                        \
      acc[0][jn] = __builtin_amdgcn_mfma_f64_16x16x4f64(AV0, BF[jn], acc[0][jn], 0, 0, 0);    \
      acc[1][jn] = __builtin_amdgcn_mfma_f64_16x16x4f64(AV1, BF[jn], acc[1][jn], 0, 0, 0);    \
    }
#define ISDF_CHUNKD(BUF, A00, A01, A10, A11, LOAD_AHEAD, STORE_NEXT)                          \
  {                                                                                           \
    ISDF_FRAGD(BUF, 1, bf1)                                                                   \
    ISDF_MFMAD(A00.x, A10.x, bf0)                                                             \
    ISDF_ISSUE(0, 0)                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_FRAGD(BUF, 2, bf0)                                                                   \
    ISDF_MFMAD(A00.y, A10.y, bf1)                                                             \
    ISDF_ISSUE(0, 0)                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_FRAGD(BUF, 3, bf1)                                                                   \
    STORE_NEXT                                                                                \
    ISDF_MFMAD(A01.x, A11.x, bf0)                                                             \
    ISDF_ISSUE(0x200, 4)                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    __syncthreads();                                                                          \
    ISDF_FRAGD(1 - (BUF), 0, bf0)                                                             \
    ISDF_MFMAD(A01.y, A11.y, bf1)                                                             \
    LOAD_AHEAD                                                                                \
    ISDF_ISSUE(0x020, 8)                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                        \
  }

  // prologue: chunk 0 in set X (its B part published in buffer 0), chunk 1 in flight in set Y, first fragments of chunk 0
  ISDF_LOADD(0, xa00, xa01, xa10, xa11, xb00, xb01, xb10, xb11)
  ISDF_LOADD(min(1, last), ya00, ya01, ya10, ya11, yb00, yb01, yb10, yb11)
  ISDF_STORED(0, xb00, xb01, xb10, xb11)
  __syncthreads();
  ISDF_FRAGD(0, 0, bf0)
  __builtin_amdgcn_sched_barrier(0);
  for (int c = 0; c < nchunks; c += 2) {
    // chunk c: A operands in X, B in buffer 0, chunk c+1 sits in Y (its B part goes to buffer 1 during k-step 2);
    // X is refilled with chunk c+2 once its last use (k-step 3) has been issued
    ISDF_CHUNKD(0, xa00, xa01, xa10, xa11, ISDF_LOADD(min(c + 2, last), xa00, xa01, xa10, xa11, xb00, xb01, xb10, xb11),
                ISDF_STORED(1, yb00, yb01, yb10, yb11))
    ISDF_CHUNKD(1, ya00, ya01, ya10, ya11, ISDF_LOADD(min(c + 3, last), ya00, ya01, ya10, ya11, yb00, yb01, yb10, yb11),
                ISDF_STORED(0, xb00, xb01, xb10, xb11))
  }
  double* out = g.P + (int64_t)t.slab * g.slab_stride;
  ISDF_STORE_ACC(2, 8, tm * BM + wave * 32, tn * BN, g.M, g.N, ISDF_SLAB_STORE)
#undef ISDF_LOADD
#undef ISDF_STORED
#undef ISDF_FRAGD
#undef ISDF_MFMAD
#undef ISDF_CHUNKD
}

// ---- three-component Hadamard NT product: T_a = sum_g (F o V)(P, g) dphi_a(mu, g) of the exchange derivative
//   C_a = beta C_a + alpha sum_k A[m,k] H[m,k] B_a[n,k],  a = 0, 1, 2,  B_a = B + a bstride, C_a = C + a cstride.
// Variant D's operand scheme: a lane loads its four consecutive k of an A row straight into MFMA operand registers, so the
// factor H costs one more load of the same shape and one multiply per element, and A o H exists only in registers.  Three
// 128 x 128 accumulator sets (384 VGPRs) do not fit the 256 registers of two waves per SIMD, so the N tile is narrowed: one
// unit is 128 rows x 32 columns of ALL three components (four waves stacked along M, 32 rows x 32 columns x 3 each = 12
// accumulators, 96 VGPRs), and A o H is formed once for the three.  The staged B tile is 3 x 32 rows x 16: component a of
// thread tid is row tid / 8, k offset 2 (tid % 8) - one double2 per component.  Register sets X / Y alternate between chunks
// as in variant D (every load has a chunk of MFMAs to land); an odd chunk count ends with one more chunk after the paired
// loop (a break in the middle of the loop body cost 152 - 312 bytes of scratch), so K only has to be a multiple of 16.  Units,
// XCD remap, slabs and their fixed-order reduction are those of the NT kernels; the partials are [slab][component][M][N].
// 208 VGPRs with H, 176 without, no scratch (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage).
constexpr int BN3 = 32;

struct Had3Args {
  const double* A; int64_t lda;
  const double* H; int64_t ldh;  // nullptr: no Hadamard factor
  const double* B; int64_t ldb, bstride;
  double* P;                     // partials [nslab][3][M][N] (or C itself when direct)
  int64_t ldp, pstride, slab_stride;
  int M, N;
  int64_t K, kslab;              // kslab multiple of BK
  int ntm, ntn, nslab;
  int64_t nunits, nunits_pad;
  double alpha, beta;            // used only when direct
  int direct;
};

template <bool HAD>
__global__ __launch_bounds__(TPBD, 2) void gemm_nt_had3_kernel(Had3Args g) {
  __shared__ double sB[2][3 * BN3 * LDT];
  const int64_t unit = xcd_unit(g.nunits_pad);
  if (unit >= g.nunits) return;
  const Tile t = decode_tile(unit, g.ntm, g.ntn);
  const int tm = t.tm, tn = t.tn;
  const KRange kr = slab_range(t.slab, g.kslab, g.K);
  const int64_t k0 = kr.k0;
  const int nchunks = (int)((kr.k1 - k0) / BK);         // any count >= 1 (K % 16 == 0, kslab a multiple of 16)
  const int last = nchunks - 1;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int frow = lane & 15, fkq = lane >> 4;
  const int mlast = g.M - 1, nlast = g.N - 1;
  // A and H: two 16-row groups of this wave's 32 rows, four consecutive k per lane; rows past the edge are clamped
  const int ar0 = min(tm * BM + wave * 32 + frow, mlast), ar1 = min(tm * BM + wave * 32 + 16 + frow, mlast);
  const double* pA0 = g.A + (int64_t)ar0 * g.lda + k0 + 4 * fkq;
  const double* pA1 = g.A + (int64_t)ar1 * g.lda + k0 + 4 * fkq;
  const double* pH0 = HAD ? g.H + (int64_t)ar0 * g.ldh + k0 + 4 * fkq : nullptr;
  const double* pH1 = HAD ? g.H + (int64_t)ar1 * g.ldh + k0 + 4 * fkq : nullptr;
  // B staging: row srow of each component's 32-row tile, k offset 2 sseg
  const int srow = tid >> 3, sseg = tid & 7;
  const double* pB0 = g.B + (int64_t)min(tn * BN3 + srow, nlast) * g.ldb + k0 + 2 * sseg;
  const double* pB1 = pB0 + g.bstride;
  const double* pB2 = pB1 + g.bstride;

  double2 xa00, xa01, xa10, xa11, xh00, xh01, xh10, xh11, xb0, xb1, xb2;
  double2 ya00, ya01, ya10, ya11, yh00, yh01, yh10, yh11, yb0, yb1, yb2;
#define ISDF_LOAD3(C, A00, A01, A10, A11, H00, H01, H10, H11, B0, B1, B2)                     \
  {                                                                                           \
    const int off = (C) * BK;                                                                 \
    A00 = *reinterpret_cast<const double2*>(pA0 + off);                                       \
    A01 = *reinterpret_cast<const double2*>(pA0 + off + 2);                                   \
    A10 = *reinterpret_cast<const double2*>(pA1 + off);                                       \
    A11 = *reinterpret_cast<const double2*>(pA1 + off + 2);                                   \
    if (HAD) {                                                                                \
      H00 = *reinterpret_cast<const double2*>(pH0 + off);                                     \
      H01 = *reinterpret_cast<const double2*>(pH0 + off + 2);                                 \
      H10 = *reinterpret_cast<const double2*>(pH1 + off);                                     \
      H11 = *reinterpret_cast<const double2*>(pH1 + off + 2);                                 \
    }                                                                                         \
    B0 = *reinterpret_cast<const double2*>(pB0 + off);                                        \
    B1 = *reinterpret_cast<const double2*>(pB1 + off);                                        \
    B2 = *reinterpret_cast<const double2*>(pB2 + off);                                        \
  }
  // A <- A o H, in the operand registers
#define ISDF_MUL3(A00, A01, A10, A11, H00, H01, H10, H11)                                     \
  if (HAD) {                                                                                  \
    A00.x *= H00.x; A00.y *= H00.y; A01.x *= H01.x; A01.y *= H01.y;                           \
    A10.x *= H10.x; A10.y *= H10.y; A11.x *= H11.x; A11.y *= H11.y;                           \
  }
#define ISDF_STORE3(BUF, B0, B1, B2)                                                          \
  {                                                                                           \
    double* q = &sB[BUF][srow * LDT + 2 * sseg];                                              \
    q[0] = B0.x; q[1] = B0.y;                                                                 \
    q[BN3 * LDT] = B1.x; q[BN3 * LDT + 1] = B1.y;                                             \
    q[2 * BN3 * LDT] = B2.x; q[2 * BN3 * LDT + 1] = B2.y;                                     \
  }

  d4 acc[6][2];                                         // [2 a + jn][i]: component a, column group jn, row group i
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[q][i] = (d4){0.0, 0.0, 0.0, 0.0};

  // fragments: element j of a lane's four k is k = 4 fkq + j (variant D's map); the six 16-row groups of the staged tile
  // (component-major) are 16 LDT apart
  double bf0[6], bf1[6];
#define ISDF_FRAG3(BUF, J, BF)                                                                \
  {                                                                                           \
    const double* pb = &sB[BUF][frow * LDT + 4 * fkq + (J)];                                  \
    _Pragma("unroll") for (int q = 0; q < 6; ++q) BF[q] = pb[q * 16 * LDT];                   \
  }
#define ISDF_MFMA3(AV0, AV1, BF)                                                              \
    _Pragma("unroll") for (int q = 0; q < 6; ++q) {                                           \
      acc[q][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(AV0, BF[q], acc[q][0], 0, 0, 0);       \
      acc[q][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(AV1, BF[q], acc[q][1], 0, 0, 0);       \
    }
  // one chunk, variant D's order: the fragments of the NEXT k-step are read from LDS under the MFMAs of the current one (one
  // read after every second MFMA: six rounds for the twelve MFMAs of a k-step), the next chunk's B part goes to the other buffer
  // during k-step 2, the chunk's single barrier sits after k-step 2, and k-step 3 already prefetches the first fragments of the
  // next chunk from the other buffer while the loads of the chunk after next are issued
#define ISDF_ISSUE3(XMASK, NX) _Pragma("unroll") for (int q_ = 0; q_ < 6; ++q_) {             \
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                \
    if (q_ < (NX)) __builtin_amdgcn_sched_group_barrier(XMASK, 1, 0); }
#define ISDF_CHUNK3(BUF, A00, A01, A10, A11, LOAD_AHEAD, STORE_NEXT)                          \
  {                                                                                           \
    ISDF_FRAG3(BUF, 1, bf1)                                                                   \
    ISDF_MFMA3(A00.x, A10.x, bf0)                                                             \
    ISDF_ISSUE3(0, 0)                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_FRAG3(BUF, 2, bf0)                                                                   \
    ISDF_MFMA3(A00.y, A10.y, bf1)                                                             \
    ISDF_ISSUE3(0, 0)                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_FRAG3(BUF, 3, bf1)                                                                   \
    STORE_NEXT                                                                                \
    ISDF_MFMA3(A01.x, A11.x, bf0)                                                             \
    ISDF_ISSUE3(0x200, 6)                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    __syncthreads();                                                                          \
    ISDF_FRAG3(1 - (BUF), 0, bf0)                                                             \
    ISDF_MFMA3(A01.y, A11.y, bf1)                                                             \
    LOAD_AHEAD                                                                                \
    ISDF_ISSUE3(0x020, 6)                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                        \
  }

  // prologue: chunk 0 in set X (its B part published in buffer 0), chunk 1 in flight in set Y, first fragments of chunk 0
  ISDF_LOAD3(0, xa00, xa01, xa10, xa11, xh00, xh01, xh10, xh11, xb0, xb1, xb2)
  ISDF_LOAD3(min(1, last), ya00, ya01, ya10, ya11, yh00, yh01, yh10, yh11, yb0, yb1, yb2)
  ISDF_STORE3(0, xb0, xb1, xb2)
  __syncthreads();
  ISDF_FRAG3(0, 0, bf0)
  __builtin_amdgcn_sched_barrier(0);
  for (int c = 0; c + 1 < nchunks; c += 2) {
    // chunk c: A o H from set X, B in buffer 0; chunk c + 1 sits in Y (its B part goes to buffer 1 during k-step 2); X is
    // refilled with chunk c + 2 once its last use (k-step 3) has been issued
    ISDF_MUL3(xa00, xa01, xa10, xa11, xh00, xh01, xh10, xh11)
    ISDF_CHUNK3(0, xa00, xa01, xa10, xa11,
                ISDF_LOAD3(min(c + 2, last), xa00, xa01, xa10, xa11, xh00, xh01, xh10, xh11, xb0, xb1, xb2),
                ISDF_STORE3(1, yb0, yb1, yb2))
    ISDF_MUL3(ya00, ya01, ya10, ya11, yh00, yh01, yh10, yh11)
    ISDF_CHUNK3(1, ya00, ya01, ya10, ya11,
                ISDF_LOAD3(min(c + 3, last), ya00, ya01, ya10, ya11, yh00, yh01, yh10, yh11, yb0, yb1, yb2),
                ISDF_STORE3(0, xb0, xb1, xb2))
  }
  if (nchunks & 1) {
    // an odd count: the last chunk sits in set X with its B part in buffer 0 and its first fragments in bf0 (from the prologue
    // or the last pair); what its k-step 3 prefetches from buffer 1 is not used
    ISDF_MUL3(xa00, xa01, xa10, xa11, xh00, xh01, xh10, xh11)
    ISDF_CHUNK3(0, xa00, xa01, xa10, xa11, , )
  }
  // the unit's three tiles: the slab's partials, or C itself (direct) with alpha and beta
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double* out = g.P + (int64_t)t.slab * g.slab_stride + (int64_t)a * g.pstride;
    ISDF_STORE_ACC(2, 2, tm * BM + wave * 32, tn * BN3, g.M, g.N, {
      double* q = out + (int64_t)row * g.ldp + col;
      const double v = acc[2 * a + j][i][r];
      if (g.direct) *q = (g.beta == 0.0) ? g.alpha * v : g.alpha * v + g.beta * (*q);
      else *q = v;
    })
  }
#undef ISDF_LOAD3
#undef ISDF_MUL3
#undef ISDF_STORE3
#undef ISDF_FRAG3
#undef ISDF_MFMA3
#undef ISDF_ISSUE3
#undef ISDF_CHUNK3
}

// ---- NN form: C = A B (optionally squared element-wise), A (M x K) with K contiguous, B (K x N) with N contiguous, K short
// (the AO count) and N long (the grid): the pair-density rows (phi_P^T phi)^2 of the fit.  Same 256x128 tile, 8 waves, register
// double buffering and pinned issue order as variant B; what changes is the B operand: a chunk is 16 full 1-KB rows of the
// K x N matrix (one row per wave and load: perfectly coalesced), written to LDS as it comes ([k][n], rows padded to 144 doubles
// so that the four k-groups of a fragment read start 32 banks apart) and read back as fragments B[k = 4 kk + fk][n] - 16
// contiguous doubles per k-group.  One unit = one output tile over the whole K (no slabs: K is ~1e3, M N is ~1e10); units are
// dealt to the XCDs in super-tiles of stm x stn tiles (32 = the workgroups one XCD runs at a time) so that the co-running
// workgroups share stm A panels and stn B panels in that XCD's L2.
constexpr int LDN = 144;

struct GemmNNArgs {
  const double* A; int64_t lda;
  const double* B; int64_t ldb;
  double* C; int64_t ldc;
  int M, N, K;                   // K % 32 == 0, N even
  int ntm, ntn, stm, stn, ngm;   // tiles, super-tile shape, super-tiles along M
  int64_t nunits, nunits_pad;
  const double* H; int64_t ldh;  // gemm_nn_had_kernel only: the Hadamard factor on B, and the epilogue's factors
  double alpha, beta;
};

// super-tiles M-fastest, tiles M-fastest inside one; the tiles of a ragged super-tile past the edge do not exist
__device__ __forceinline__ Tile decode_supertile(int64_t unit, const GemmNNArgs& g) {
  const int per = g.stm * g.stn;
  const int64_t grp = unit / per;
  const int within = (int)(unit - grp * per);
  return {(int)(grp % g.ngm) * g.stm + within % g.stm, (int)(grp / g.ngm) * g.stn + within / g.stm, 0};
}

// The unit body of both NN kernels.  HAD: the Hadamard factor H (K x N, as B) is loaded at B's coordinates with B's edge clamping
// and multiplied into the B staging registers on their way to LDS (H o B is never stored, B is not modified), the six global
// loads per chunk become eight, and the epilogue applies alpha and beta (beta = 0 does not read C).
template <bool SQ, bool HAD>
__device__ __forceinline__ void nn_unit(const GemmNNArgs& g) {
  extern __shared__ double smem[];                      // [2][BM2*LDT] A | [2][BK*LDN] B
  double* sA = smem;
  double* sB = smem + 2 * BM2 * LDT;
  const int64_t unit = xcd_unit(g.nunits_pad);
  if (unit >= g.nunits) return;
  const Tile t = decode_supertile(unit, g);
  const int tm = t.tm, tn = t.tn;
  if (tm >= g.ntm || tn >= g.ntn) return;
  const int nchunks = g.K / BK;                         // even
  const int last = nchunks - 1;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;              // 4 x 2 waves, 64x64 each
  const int srow = tid >> 3, sseg = tid & 7;            // A staging: row srow + 64 i, k offset 2 sseg
  const int krow = tid >> 6, nseg = tid & 63;           // B staging: k rows krow and krow + 8, columns 2 nseg, 2 nseg + 1
  const int mlast = g.M - 1;
  const double* pA0 = g.A + (int64_t)min(tm * BM2 + srow, mlast) * g.lda + sseg * 2;
  const double* pA1 = g.A + (int64_t)min(tm * BM2 + srow + 64, mlast) * g.lda + sseg * 2;
  const double* pA2 = g.A + (int64_t)min(tm * BM2 + srow + 128, mlast) * g.lda + sseg * 2;
  const double* pA3 = g.A + (int64_t)min(tm * BM2 + srow + 192, mlast) * g.lda + sseg * 2;
  // columns past the edge re-read the last pair (computed, never stored)
  const double* pB0 = g.B + (int64_t)krow * g.ldb + min(tn * BN + 2 * nseg, g.N - 2);
  const double* pB1 = pB0 + 8 * g.ldb;
  const int64_t bstep = (int64_t)BK * g.ldb;
  const double* pH0 = HAD ? g.H + (int64_t)krow * g.ldh + min(tn * BN + 2 * nseg, g.N - 2) : nullptr;
  const double* pH1 = HAD ? pH0 + 8 * g.ldh : nullptr;
  const int64_t hstep = HAD ? (int64_t)BK * g.ldh : 0;

  double2 xa0, xa1, xa2, xa3, xb0, xb1, ya0, ya1, ya2, ya3, yb0, yb1;
  double2 xh0, xh1, yh0, yh1;                           // HAD only
#define ISDF_NN_LOAD(C, A0, A1, A2, A3, B0, B1, H0, H1)                                       \
  {                                                                                           \
    const int off = (C) * BK;                                                                 \
    const int64_t offb = (C) * bstep;                                                         \
    A0 = *reinterpret_cast<const double2*>(pA0 + off);                                        \
    A1 = *reinterpret_cast<const double2*>(pA1 + off);                                        \
    A2 = *reinterpret_cast<const double2*>(pA2 + off);                                        \
    A3 = *reinterpret_cast<const double2*>(pA3 + off);                                        \
    B0 = *reinterpret_cast<const double2*>(pB0 + offb);                                       \
    B1 = *reinterpret_cast<const double2*>(pB1 + offb);                                       \
    if (HAD) {                                                                                \
      H0 = *reinterpret_cast<const double2*>(pH0 + (C) * hstep);                              \
      H1 = *reinterpret_cast<const double2*>(pH1 + (C) * hstep);                              \
    }                                                                                         \
  }
#define ISDF_NN_ST1(P, R) { double* q_ = (P); q_[0] = R.x; q_[1] = R.y; }
#define ISDF_NN_STORE(BUF, A0, A1, A2, A3, B0, B1, H0, H1)                                    \
  {                                                                                           \
    double* qa = sA + (BUF) * BM2 * LDT + srow * LDT + sseg * 2;                              \
    double* qb = sB + (BUF) * BK * LDN + krow * LDN + 2 * nseg;                               \
    if (HAD) { B0.x *= H0.x; B0.y *= H0.y; B1.x *= H1.x; B1.y *= H1.y; }                      \
    ISDF_NN_ST1(qa, A0) ISDF_NN_ST1(qa + 64 * LDT, A1) ISDF_NN_ST1(qa + 128 * LDT, A2)        \
    ISDF_NN_ST1(qa + 192 * LDT, A3)                                                           \
    *reinterpret_cast<double2*>(qb) = B0;                                                     \
    *reinterpret_cast<double2*>(qb + 8 * LDN) = B1;                                           \
  }

  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  const int frow = lane & 15, fk = lane >> 4;
  const int aoff = (wm * 64 + frow) * LDT + fk, boff = fk * LDN + wn * 64 + frow;
  double a0[4], b0[4], a1[4], b1[4];
#define ISDF_NN_FRAG(BUF, KK, AF, BF)                                                         \
  {                                                                                           \
    const double* pa = sA + (BUF) * BM2 * LDT + aoff;                                         \
    const double* pb = sB + (BUF) * BK * LDN + boff;                                          \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                           \
      AF[i] = pa[i * 16 * LDT + (KK) * 4];                                                    \
      BF[i] = pb[(KK) * 4 * LDN + i * 16];                                                    \
    }                                                                                         \
  }
  // same issue order as variant B (see tile_256x128)
#define ISDF_NN_CHUNK(BUF, LOAD_AHEAD, STORE_NEXT)                                            \
  {                                                                                           \
    ISDF_NN_FRAG(BUF, 1, a1, b1)                                                              \
    LOAD_AHEAD                                                                                \
    ISDF_MFMA16(a0, b0)                                                                       \
    ISDF_ISSUE(0x020, HAD ? 8 : 6)                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_NN_FRAG(BUF, 2, a0, b0)                                                              \
    ISDF_MFMA16(a1, b1)                                                                       \
    ISDF_ISSUE(0, 0)                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    ISDF_NN_FRAG(BUF, 3, a1, b1)                                                              \
    STORE_NEXT                                                                                \
    ISDF_MFMA16(a0, b0)                                                                       \
    ISDF_ISSUE(0x200, 6)                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    __syncthreads();                                                                          \
    ISDF_NN_FRAG(1 - (BUF), 0, a0, b0)                                                        \
    ISDF_MFMA16(a1, b1)                                                                       \
    ISDF_ISSUE(0, 0)                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                        \
  }

  ISDF_NN_LOAD(0, xa0, xa1, xa2, xa3, xb0, xb1, xh0, xh1)
  ISDF_NN_LOAD(1, ya0, ya1, ya2, ya3, yb0, yb1, yh0, yh1)
  ISDF_NN_STORE(0, xa0, xa1, xa2, xa3, xb0, xb1, xh0, xh1)
  __syncthreads();
  ISDF_NN_FRAG(0, 0, a0, b0)
  __builtin_amdgcn_sched_barrier(0);
  // HAD takes any M: a wave whose 64 rows all lie past the edge (M = r of an SCF density is often 32 - 128) only stages its share of
  // the operands and meets the barriers - one per chunk, as the waves that compute - so that the live waves have their SIMD's
  // MFMA pipe to themselves.  The condition is uniform over a wave; without HAD it is constant and the loop is the one loop.
  if (!HAD || tm * BM2 + wm * 64 < g.M) {
    for (int c = 0; c < nchunks; c += 2) {
      ISDF_NN_CHUNK(0, ISDF_NN_LOAD(min(c + 2, last), xa0, xa1, xa2, xa3, xb0, xb1, xh0, xh1),
                    ISDF_NN_STORE(1, ya0, ya1, ya2, ya3, yb0, yb1, yh0, yh1))
      ISDF_NN_CHUNK(1, ISDF_NN_LOAD(min(c + 3, last), ya0, ya1, ya2, ya3, yb0, yb1, yh0, yh1),
                    ISDF_NN_STORE(0, xa0, xa1, xa2, xa3, xb0, xb1, xh0, xh1))
    }
  } else {
    for (int c = 0; c < nchunks; c += 2) {
      ISDF_NN_LOAD(min(c + 2, last), xa0, xa1, xa2, xa3, xb0, xb1, xh0, xh1)
      ISDF_NN_STORE(1, ya0, ya1, ya2, ya3, yb0, yb1, yh0, yh1)
      __syncthreads();
      ISDF_NN_LOAD(min(c + 3, last), ya0, ya1, ya2, ya3, yb0, yb1, yh0, yh1)
      ISDF_NN_STORE(0, xa0, xa1, xa2, xa3, xb0, xb1, xh0, xh1)
      __syncthreads();
    }
    return;
  }
  if (HAD) {
    ISDF_STORE_ACC(4, 4, tm * BM2 + wm * 64, tn * BN + wn * 64, g.M, g.N, {
      double* q = g.C + (int64_t)row * g.ldc + col;
      const double v = acc[i][j][r];
      *q = (g.beta == 0.0) ? g.alpha * v : g.alpha * v + g.beta * (*q);
    })
  } else {
    ISDF_STORE_ACC(4, 4, tm * BM2 + wm * 64, tn * BN + wn * 64, g.M, g.N,
                   { const double v = acc[i][j][r]; g.C[(int64_t)row * g.ldc + col] = SQ ? v * v : v; })
  }
#undef ISDF_NN_LOAD
#undef ISDF_NN_ST1
#undef ISDF_NN_STORE
#undef ISDF_NN_FRAG
#undef ISDF_NN_CHUNK
}

template <bool SQ>
__global__ __launch_bounds__(TPB2, 2) void gemm_nn_mfma_kernel(GemmNNArgs g) { nn_unit<SQ, false>(g); }

// C = alpha A (H o B) + beta C: the Z of the contracted exchange force
__global__ __launch_bounds__(TPB2, 2) void gemm_nn_had_kernel(GemmNNArgs g) { nn_unit<false, true>(g); }
#undef ISDF_MFMA16
#undef ISDF_ISSUE

__global__ void reduce_slabs_kernel(const double* __restrict__ P, int nslab, int64_t slab_stride,
                                    int M, int N, double alpha, double beta, double* __restrict__ C,
                                    int64_t ldc) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)M * N) return;
  const int m = (int)(idx / N), n = (int)(idx % N);
  double s = 0.0;
  for (int t = 0; t < nslab; ++t) s += P[(int64_t)t * slab_stride + idx];
  double* q = C + (int64_t)m * ldc + n;
  *q = (beta == 0.0) ? alpha * s : alpha * s + beta * (*q);
}

// ---- Hermitian twice-scaled NT product: the k-point M^q from the packed half spectra ------------------------
//   Cre = alpha sum_k A[m,k] s[k] B[n,k] + beta Cre,   Cim = alpha sum_k A[m,k] a[k] B~[n,k] + beta Cim,
//   B~[n,2j] = -B[n,2j+1], B~[n,2j+1] = B[n,2j]   (the columns are consecutive (Re, Im) pairs: B~ is i B).
// One pass: every staged 128 x 16 A and B tile feeds BOTH accumulator sets.  128 x 128 tile, eight waves in a 2 x 4 grid, each
// 64 rows x 32 columns = 4 x 2 accumulators per set (128 accumulator VGPRs for the two sets: the 256-register budget of two waves
// per SIMD holds them without scratch).  A and B go to LDS as they are; a lane reads its B fragment element k AND its pair partner
// k ^ 1 from LDS and multiplies them with s[k] and -+a[k] (the tables of the chunk sit in LDS next to the tiles; they are
// pair-repeated, a[k] = a[k ^ 1]), so neither a scaled copy nor i B is ever stored.  Work units, XCD remap, double-buffered
// 16-deep chunks and the fixed-order slab reduction are those of variant A above.  Aligned operands only: K % 16 == 0 (the packed
// rows are zero padded to a multiple of 128 and so are the tables), 16-byte aligned rows and tables.
constexpr int TPBH = 512;

struct HermArgs {
  const double* A; int64_t lda;
  const double* B; int64_t ldb;
  const double* s; const double* a;
  double* Pre; double* Pim;      // partials [nslab][2][M][N] (or Cre / Cim themselves when direct)
  int64_t ldp, slab_stride;
  int M, N;
  int64_t K, kslab;              // kslab multiple of BK
  int ntm, ntn, nslab;
  int64_t nunits, nunits_pad;
  double alpha, beta;
  int direct;
};

__global__ __launch_bounds__(TPBH, 2) void herm_kscale_nt_kernel(HermArgs g) {
  extern __shared__ double smem[];                      // [2][BM*LDT] A | [2][BN*LDT] B | [2][2*BK] tables (s, then a)
  double* sA = smem;
  double* sB = smem + 2 * BM * LDT;
  double* sT = smem + 2 * (BM + BN) * LDT;
  const int64_t unit = xcd_unit(g.nunits_pad);
  if (unit >= g.nunits) return;
  const Tile t = decode_tile(unit, g.ntm, g.ntn);
  const int tm = t.tm, tn = t.tn, slab = t.slab;
  const KRange kr = slab_range(slab, g.kslab, g.K);
  const int64_t k0 = kr.k0;
  const int nchunks = (int)((kr.k1 - k0) / BK);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;              // 2 x 4 waves, 64 rows x 32 columns each
  const int srow = tid >> 3;                            // 0..63, +64
  const int sseg = tid & 7;
  const int mlast = g.M - 1, nlast = g.N - 1;
  // rows past the matrix edge are clamped: computed, never stored
  const double* pA0 = g.A + (int64_t)min(tm * BM + srow, mlast) * g.lda + k0 + sseg * 2;
  const double* pA1 = g.A + (int64_t)min(tm * BM + srow + 64, mlast) * g.lda + k0 + sseg * 2;
  const double* pB0 = g.B + (int64_t)min(tn * BN + srow, nlast) * g.ldb + k0 + sseg * 2;
  const double* pB1 = g.B + (int64_t)min(tn * BN + srow + 64, nlast) * g.ldb + k0 + sseg * 2;
  // the chunk's tables: threads 0..7 fetch s, threads 8..15 fetch a (one double2 each)
  const bool tload = tid < 16;
  const double* pT = (tid < 8 ? g.s : g.a) + k0 + sseg * 2;

  double2 ra0, ra1, rb0, rb1, rt = make_double2(0.0, 0.0);
#define ISDF_LOADH(C)                                                                         \
  {                                                                                           \
    const int off = (C) * BK;                                                                 \
    ra0 = *reinterpret_cast<const double2*>(pA0 + off);                                       \
    ra1 = *reinterpret_cast<const double2*>(pA1 + off);                                       \
    rb0 = *reinterpret_cast<const double2*>(pB0 + off);                                       \
    rb1 = *reinterpret_cast<const double2*>(pB1 + off);                                       \
    if (tload) rt = *reinterpret_cast<const double2*>(pT + off);                              \
  }
#define ISDF_STH(P, R) { double* q_ = (P); q_[0] = R.x; q_[1] = R.y; }
#define ISDF_STOREH(BUF)                                                                      \
  {                                                                                           \
    double* qa = sA + (BUF) * BM * LDT + srow * LDT + sseg * 2;                               \
    double* qb = sB + (BUF) * BN * LDT + srow * LDT + sseg * 2;                               \
    ISDF_STH(qa, ra0) ISDF_STH(qa + 64 * LDT, ra1) ISDF_STH(qb, rb0) ISDF_STH(qb + 64 * LDT, rb1) \
    if (tload) ISDF_STH(sT + (BUF) * 2 * BK + (tid >> 3) * BK + sseg * 2, rt)                 \
  }

  d4 cre[4][2], cim[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) { cre[i][j] = (d4){0.0, 0.0, 0.0, 0.0}; cim[i][j] = (d4){0.0, 0.0, 0.0, 0.0}; }

  const int frow = lane & 15, fk = lane >> 4;
  // global k of a fragment element is 16 c + 4 kk + fk (k0 is a multiple of 16): its parity is that of fk
  const double sgn = (fk & 1) ? 1.0 : -1.0;
  const int aoff = (wm * 64 + frow) * LDT, boff = (wn * 32 + frow) * LDT;
  ISDF_LOADH(0)
  ISDF_STOREH(0)
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) ISDF_LOADH(c + 1)
    const double* pa = sA + buf * BM * LDT + aoff;
    const double* pb = sB + buf * BN * LDT + boff;
    const double* pt = sT + buf * 2 * BK;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = kk * 4 + fk;
      const double sv = pt[k], av = sgn * pt[BK + k];
      double af[4], br[2], bi[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = pa[i * 16 * LDT + k];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        br[j] = sv * pb[j * 16 * LDT + k];
        bi[j] = av * pb[j * 16 * LDT + (k ^ 1)];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          cre[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], br[j], cre[i][j], 0, 0, 0);
          cim[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bi[j], cim[i][j], 0, 0, 0);
        }
    }
    if (c + 1 < nchunks) ISDF_STOREH(buf ^ 1)
    __syncthreads();
  }

  double* ore = g.Pre + (int64_t)slab * g.slab_stride;
  double* oim = g.Pim + (int64_t)slab * g.slab_stride;
#define ISDF_HERM_STORE                                                                       \
  {                                                                                           \
    const int64_t o = (int64_t)row * g.ldp + col;                                             \
    const double vr = cre[i][j][r], vi = cim[i][j][r];                                        \
    if (g.direct) {                                                                           \
      ore[o] = (g.beta == 0.0) ? g.alpha * vr : g.alpha * vr + g.beta * ore[o];               \
      oim[o] = (g.beta == 0.0) ? g.alpha * vi : g.alpha * vi + g.beta * oim[o];               \
    } else {                                                                                  \
      ore[o] = vr;                                                                            \
      oim[o] = vi;                                                                            \
    }                                                                                         \
  }
  ISDF_STORE_ACC(4, 2, tm * BM + wm * 64, tn * BN + wn * 32, g.M, g.N, ISDF_HERM_STORE)
#undef ISDF_HERM_STORE
#undef ISDF_LOADH
#undef ISDF_STH
#undef ISDF_STOREH
}
#undef ISDF_STORE_ACC
#undef ISDF_SLAB_STORE

// ---- host side: slab plan, operand alignment, dynamic LDS -------------------------------------------------------------------------------
struct SlabPlan { int nslab; int64_t kslab, nunits, nunits_pad; };

// K slabs of an NT product of ntiles output tiles on `slots` resident workgroups: enough units to fill the slots about 8 times
// over, slabs at least 2048 deep, partial workspace (out_bytes per entry of the M x N output) at most 2 GiB, slab length a
// multiple of kmult.
// tune = wave quantisation: the units are dealt to `slots` resident workgroups, so the launch takes ceil(units / slots) unit
// times.  Among slab counts between the target and twice the target pick the one whose last round is fullest
// (512 x 15132 output: 238 tiles; 9 slabs = 8.37 rounds -> 9, 15 slabs = 13.95 rounds -> 14: 7 % less idle time)
SlabPlan plan_slabs(int64_t ntiles, int64_t slots, int M, int N, int64_t K, int out_bytes, int kmult, bool tune) {
  int64_t nslab = cdiv(8 * slots, ntiles);
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(1, K / 2048),
                                                             std::max<int64_t>(1, ((int64_t)2 << 30) / ((int64_t)M * N * out_bytes))));
  nslab = std::max<int64_t>(1, std::min<int64_t>(nslab, cap));
  if (tune && ntiles * nslab > slots) {
    double best = 1e30;
    int64_t pick = nslab;
    for (int64_t c = nslab; c <= std::min<int64_t>(2 * nslab, cap); ++c) {
      const double units = (double)ntiles * c;
      const double waste = (double)(cdiv((int64_t)units, slots) * slots) / units;
      if (waste < best - 1e-9) { best = waste; pick = c; }
    }
    nslab = pick;
  }
  SlabPlan p;
  p.kslab = cdiv(cdiv(K, nslab), kmult) * kmult;
  p.nslab = (int)cdiv(K, p.kslab);
  p.nunits = ntiles * p.nslab;
  p.nunits_pad = cdiv(p.nunits, 8) * 8;
  return p;
}

// rows of ld doubles from p start on 16-byte boundaries (ld = 0: a vector; a null pointer passes)
bool rows_aligned16(const double* p, int64_t ld = 0) { return ld % 2 == 0 && ((uintptr_t)p) % 16 == 0; }

// raise the dynamic-LDS limit of the kernels once per handle (= per device), not per process; `done` is the handle's flag
template <class... Kernels>
int raise_lds_once(isdf_handle h, int& done, size_t lds, Kernels... kernels) {
  if (done) return ISDF_OK;
  for (const void* k : {(const void*)kernels...})
    HIP_TRY(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  done = 1;
  return ISDF_OK;
}

}  // namespace

// Exposed as isdf_herm_kscale_nt (declared in include/mi355_isdf.h).
extern "C" int isdf_herm_kscale_nt(isdf_handle h, int M, int N, int64_t K, double alpha, const double* d_A, int64_t lda,
                                   const double* d_B, int64_t ldb, const double* d_s, const double* d_a, double beta,
                                   double* d_Cre, double* d_Cim, int64_t ldc) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, M > 0 && N > 0 && K > 0 && d_A && d_B && d_s && d_a && d_Cre && d_Cim && lda >= K && ldb >= K && ldc >= N);
  ARG_CHECK(h, K % BK == 0 && rows_aligned16(d_A, lda) && rows_aligned16(d_B, ldb) && rows_aligned16(d_s) && rows_aligned16(d_a));
  HermArgs g;
  g.A = d_A; g.lda = lda; g.B = d_B; g.ldb = ldb; g.s = d_s; g.a = d_a;
  g.M = M; g.N = N; g.K = K;
  g.ntm = (int)cdiv(M, BM); g.ntn = (int)cdiv(N, BN);
  // one workgroup of eight waves per CU; the two planes' partials share the 2 GiB
  const SlabPlan p = plan_slabs((int64_t)g.ntm * g.ntn, h->num_cu, M, N, K, 16, BK, true);
  g.kslab = p.kslab; g.nslab = p.nslab; g.nunits = p.nunits; g.nunits_pad = p.nunits_pad;
  ARG_CHECK(h, g.nunits_pad < 2147483647LL);
  g.alpha = alpha; g.beta = beta;
  const int64_t plane = (int64_t)M * N;
  if (g.nslab == 1) {
    g.direct = 1; g.Pre = d_Cre; g.Pim = d_Cim; g.ldp = ldc; g.slab_stride = 0;
  } else {
    g.direct = 0;
    g.Pre = (double*)isdf_ws(h, "gemm_partials", sizeof(double) * (size_t)g.nslab * 2 * plane);
    if (!g.Pre) return ISDF_ERR_HIP;
    g.Pim = g.Pre + plane;
    g.ldp = N; g.slab_stride = 2 * plane;
  }
  const size_t lds = sizeof(double) * (2 * (BM + BN) * LDT + 4 * BK);
  if (int rc = raise_lds_once(h, h->attr_herm, lds, herm_kscale_nt_kernel)) return rc;
  {
    ProfScope ps(h, "herm_kscale_nt_kernel[flop]", 4.0 * M * N * (double)K);
    hipLaunchKernelGGL(herm_kscale_nt_kernel, dim3((unsigned)g.nunits_pad), dim3(TPBH), lds, h->stream, g);
    KERNEL_CHECK(h);
  }
  if (!g.direct) {
    ProfScope ps(h, "gemm_reduce_slabs_kernel[byte]", 16.0 * (double)plane * (g.nslab + 1));
    const unsigned nb = (unsigned)cdiv(plane, 256);
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(nb), dim3(256), 0, h->stream, g.Pre, g.nslab, g.slab_stride, M, N, alpha, beta,
                       d_Cre, ldc);
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(nb), dim3(256), 0, h->stream, g.Pim, g.nslab, g.slab_stride, M, N, alpha, beta,
                       d_Cim, ldc);
    KERNEL_CHECK(h);
  }
  return ISDF_OK;
}

int gemm_nt_f64_scaled(isdf_handle h, int M, int N, int64_t K, double alpha, const double* A, int64_t lda,
                       const double* B, int64_t ldb, const double* kscale, double beta, double* C,
                       int64_t ldc) {
  ARG_CHECK(h, M > 0 && N > 0 && K > 0 && A && B && C && lda >= K && ldb >= K && ldc >= N);
  GemmArgs g;
  g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.kscale = kscale;
  g.M = M; g.N = N; g.K = K;
  // variant: -1 auto (default), 0 force the 128x128 kernel, 1 force the 256x128 kernel where legal, 3 the 128x128 kernel with
  // A direct to registers (variant D) where legal
  static const int variant = getenv("ISDF_GEMM_VARIANT") ? atoi(getenv("ISDF_GEMM_VARIANT")) : -1;
  static const int tune = getenv("ISDF_GEMM_SLAB_TUNE") ? atoi(getenv("ISDF_GEMM_SLAB_TUNE")) : 1;
  const bool aligned = rows_aligned16(A, lda) && rows_aligned16(B, ldb) && rows_aligned16(kscale);
  const bool alignedB = aligned && K % 32 == 0, fast = aligned && K % BK == 0;
  // auto: the 256x128 kernel (B) whenever M fills 256-row tiles (row padding < 15 %): after the issue-order work it leads on
  // every such shape measured, the k-point W^q batches most of all (MgO 2x2x2: 3.8 s against 4.5 s with D); variant D (A
  // direct to registers, 128x128, two workgroups per CU) for the other aligned shapes, variant A for unaligned operands
  const bool fitsB = (double)(cdiv(M, BM2) * BM2) <= 1.15 * (double)M;
  const bool useB = alignedB && M > BM && (variant == 1 || (variant == -1 && fitsB));
  const bool useD = alignedB && !useB && (variant == 3 || variant == -1);
  g.ntm = (int)cdiv(M, useB ? BM2 : BM); g.ntn = (int)cdiv(N, BN);
  // 2 workgroups per CU (B: one); an even number of chunks per slab
  const SlabPlan p = plan_slabs((int64_t)g.ntm * g.ntn, (int64_t)h->num_cu * (useB ? 1 : 2), M, N, K, 8, 2 * BK, tune != 0);
  g.kslab = p.kslab; g.nslab = p.nslab; g.nunits = p.nunits; g.nunits_pad = p.nunits_pad;
  g.alpha = alpha; g.beta = beta;
  if (g.nslab == 1) {
    g.direct = 1; g.P = C; g.ldp = ldc; g.slab_stride = 0;
  } else {
    g.direct = 0;
    g.P = (double*)isdf_ws(h, "gemm_partials", sizeof(double) * (size_t)g.nslab * M * N);
    if (!g.P) return ISDF_ERR_HIP;
    g.ldp = N; g.slab_stride = (int64_t)M * N;
  }
  ARG_CHECK(h, g.nunits_pad < 2147483647LL);
  // one profiling label per kernel instantiation, named as rocprofv3 names them
  const char* label = useD ? (kscale ? "gemm_nt_mfma_kernel_d<true>[flop]" : "gemm_nt_mfma_kernel_d<false>[flop]") : useB ? (kscale ? "gemm_nt_mfma_kernel_b<true>[flop]" : "gemm_nt_mfma_kernel_b<false>[flop]")
                           : (fast ? "gemm_nt_mfma_kernel<true>[flop]" : "gemm_nt_mfma_kernel<false>[flop]");
  {
    ProfScope ps(h, label, 2.0 * M * N * (double)K);
    if (useD) {
      if (kscale) hipLaunchKernelGGL(gemm_nt_mfma_kernel_d<true>, dim3((unsigned)g.nunits_pad), dim3(TPBD), 0, h->stream, g);
      else hipLaunchKernelGGL(gemm_nt_mfma_kernel_d<false>, dim3((unsigned)g.nunits_pad), dim3(TPBD), 0, h->stream, g);
    } else if (useB) {
      const size_t lds = sizeof(double) * 2 * (BM2 + BN) * LDT;
      if (int rc = raise_lds_once(h, h->attr_gemm_b, lds, gemm_nt_mfma_kernel_b<true>, gemm_nt_mfma_kernel_b<false>)) return rc;
      if (kscale) hipLaunchKernelGGL(gemm_nt_mfma_kernel_b<true>, dim3((unsigned)g.nunits_pad), dim3(TPB2), lds, h->stream, g);
      else hipLaunchKernelGGL(gemm_nt_mfma_kernel_b<false>, dim3((unsigned)g.nunits_pad), dim3(TPB2), lds, h->stream, g);
    } else if (fast) hipLaunchKernelGGL(gemm_nt_mfma_kernel<true>, dim3((unsigned)g.nunits_pad), dim3(TPB), 0, h->stream, g);
    else hipLaunchKernelGGL(gemm_nt_mfma_kernel<false>, dim3((unsigned)g.nunits_pad), dim3(TPB), 0, h->stream, g);
    KERNEL_CHECK(h);
  }
  if (!g.direct) {
    ProfScope ps(h, "gemm_reduce_slabs_kernel[byte]", 8.0 * (double)M * N * (g.nslab + 1));
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)cdiv((int64_t)M * N, 256)), dim3(256), 0, h->stream,
                       g.P, g.nslab, g.slab_stride, M, N, alpha, beta, C, ldc);
    KERNEL_CHECK(h);
  }
  return ISDF_OK;
}

int gemm_nt_f64(isdf_handle h, int M, int N, int64_t K, double alpha, const double* A, int64_t lda,
                const double* B, int64_t ldb, double beta, double* C, int64_t ldc) {
  return gemm_nt_f64_scaled(h, M, N, K, alpha, A, lda, B, ldb, nullptr, beta, C, ldc);
}

// Exposed for tests and benchmarks (declared in include/mi355_isdf.h).
extern "C" int isdf_gemm_nt(isdf_handle h, int M, int N, int64_t K, double alpha, const double* d_A,
                            int64_t lda, const double* d_B, int64_t ldb, const double* d_kscale,
                            double beta, double* d_C, int64_t ldc) {
  if (!h) return ISDF_ERR_ARG;
  return gemm_nt_f64_scaled(h, M, N, K, alpha, d_A, lda, d_B, ldb, d_kscale, beta, d_C, ldc);
}

// Exposed as isdf_gemm_nt_had3 (declared in include/mi355_isdf.h).
extern "C" int isdf_gemm_nt_had3(isdf_handle h, int M, int N, int64_t K, double alpha, const double* d_A, int64_t lda,
                                 const double* d_H, int64_t ldh, const double* d_B, int64_t ldb, int64_t bstride, double beta,
                                 double* d_C, int64_t ldc, int64_t cstride) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, M > 0 && N > 0 && K > 0 && d_A && d_B && d_C && lda >= K && (!d_H || ldh >= K) && ldb >= K && ldc >= N);
  ARG_CHECK(h, bstride >= 0 && cstride >= (int64_t)(M - 1) * ldc + N);
  const bool fused = K % BK == 0 && rows_aligned16(d_A, lda) && (!d_H || rows_aligned16(d_H, ldh)) && rows_aligned16(d_B, ldb) &&
                     bstride % 2 == 0;
  if (!fused) {
    // other alignments: the composition - a copy of A times H, then one NT product per component
    const double* A = d_A;
    int64_t la = lda;
    if (d_H) {
      double* AH = (double*)isdf_ws(h, "had3_AH", sizeof(double) * (size_t)M * (size_t)K);
      if (!AH) return ISDF_ERR_HIP;
      HIP_TRY(h, hipMemcpy2DAsync(AH, sizeof(double) * (size_t)K, d_A, sizeof(double) * (size_t)lda, sizeof(double) * (size_t)K,
                                  (size_t)M, hipMemcpyDeviceToDevice, h->stream));
      for (int r0 = 0; r0 < M; r0 += 32768) {
        const int nr = M - r0 < 32768 ? M - r0 : 32768;
        if (int rc = isdf_hadamard_rows(h, AH + (int64_t)r0 * K, K, d_H + (int64_t)r0 * ldh, ldh, nr, K)) return rc;
      }
      A = AH; la = K;
    }
    for (int a = 0; a < 3; ++a)
      if (int rc = gemm_nt_f64(h, M, N, K, alpha, A, la, d_B + a * bstride, ldb, beta, d_C + a * cstride, ldc)) return rc;
    return ISDF_OK;
  }
  Had3Args g;
  g.A = d_A; g.lda = lda; g.H = d_H; g.ldh = ldh; g.B = d_B; g.ldb = ldb; g.bstride = bstride;
  g.M = M; g.N = N; g.K = K;
  g.ntm = (int)cdiv(M, BM); g.ntn = (int)cdiv(N, BN3);
  // two workgroups per CU; three components per entry of the M x N output share the 2 GiB of partials
  const SlabPlan p = plan_slabs((int64_t)g.ntm * g.ntn, (int64_t)h->num_cu * 2, M, N, K, 24, BK, true);
  g.kslab = p.kslab; g.nslab = p.nslab; g.nunits = p.nunits; g.nunits_pad = p.nunits_pad;
  ARG_CHECK(h, g.nunits_pad < 2147483647LL);
  g.alpha = alpha; g.beta = beta;
  const int64_t plane = (int64_t)M * N;
  if (g.nslab == 1) {
    g.direct = 1; g.P = d_C; g.ldp = ldc; g.pstride = cstride; g.slab_stride = 0;
  } else {
    g.direct = 0;
    g.P = (double*)isdf_ws(h, "gemm_partials", sizeof(double) * (size_t)g.nslab * 3 * plane);
    if (!g.P) return ISDF_ERR_HIP;
    g.ldp = N; g.pstride = plane; g.slab_stride = 3 * plane;
  }
  {
    ProfScope ps(h, d_H ? "gemm_nt_had3_kernel<true>[flop]" : "gemm_nt_had3_kernel<false>[flop]", 6.0 * M * N * (double)K);
    if (d_H) hipLaunchKernelGGL(gemm_nt_had3_kernel<true>, dim3((unsigned)g.nunits_pad), dim3(TPBD), 0, h->stream, g);
    else hipLaunchKernelGGL(gemm_nt_had3_kernel<false>, dim3((unsigned)g.nunits_pad), dim3(TPBD), 0, h->stream, g);
    KERNEL_CHECK(h);
  }
  if (!g.direct) {
    ProfScope ps(h, "gemm_reduce_slabs_kernel[byte]", 24.0 * (double)plane * (g.nslab + 1));
    for (int a = 0; a < 3; ++a)
      hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)cdiv(plane, 256)), dim3(256), 0, h->stream, g.P + a * plane, g.nslab,
                         g.slab_stride, M, N, alpha, beta, d_C + a * cstride, ldc);
    KERNEL_CHECK(h);
  }
  return ISDF_OK;
}

int gram_tri_blocks(isdf_handle h, const double* X, int64_t ldx, int K, const GramTriUnit* d_units, int64_t nunits,
                    const int64_t* d_blk_off, int64_t row0, const int64_t* d_tri_off, double* S, double flop) {
  ARG_CHECK(h, X && d_units && d_blk_off && d_tri_off && S && nunits > 0 && K > 0 && K % 32 == 0 && ldx >= K &&
                   rows_aligned16(X, ldx));
  GramTriArgs t;
  t.X = X; t.ldx = ldx; t.K = K; t.units = d_units; t.blk_off = d_blk_off; t.row0 = row0; t.tri_off = d_tri_off; t.S = S;
  t.nunits = nunits; t.nunits_pad = cdiv(nunits, 8) * 8;
  ARG_CHECK(h, t.nunits_pad < 2147483647LL);
  const size_t lds = sizeof(double) * 2 * (BM2 + BN) * LDT;
  if (int rc = raise_lds_once(h, h->attr_gram_tri, lds, gram_tri_mfma_kernel)) return rc;
  ProfScope ps(h, "cand_gram_blocks[flop]", flop);
  hipLaunchKernelGGL(gram_tri_mfma_kernel, dim3((unsigned)t.nunits_pad), dim3(TPB2), lds, h->stream, t);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

bool gemm_nn_f64_supported(isdf_handle h, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B,
                           int64_t ldb) {
  // opt-in (isdf_set_option "gemm_nn_own"): measured on the pair-row shapes of configs[2] the kernel reaches 69.5-71 TF/s
  // alone and 66 TF/s inside the build, rocBLAS 74-75 and 74 (profiles/r02_gemm_nn_vs_rocblas.log) - the library keeps this
  // product by default
  return h->gemm_nn_own && M > BM && (double)(cdiv(M, BM2) * BM2) <= 1.15 * (double)M && N >= 2 && N % 2 == 0 && K >= 32 && K % 32 == 0 &&
         rows_aligned16(A, lda) && rows_aligned16(B, ldb) && M < 2147483647LL && N < 2147483647LL && K < 2147483647LL;
}

// tiles and super-tiles of the NN kernels for an M x N output
static GemmNNArgs nn_args(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
                          int64_t ldc) {
  GemmNNArgs g;
  g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc;
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.ntm = (int)cdiv(M, BM2); g.ntn = (int)cdiv(N, BN);
  g.stm = g.ntm >= 4 ? 4 : (g.ntm >= 2 ? 2 : 1);
  g.stn = 32 / g.stm;
  g.ngm = (int)cdiv(g.ntm, g.stm);
  g.nunits = (int64_t)g.ngm * cdiv(g.ntn, g.stn) * 32;
  g.nunits_pad = cdiv(g.nunits, 8) * 8;
  g.H = nullptr; g.ldh = 0; g.alpha = 1.0; g.beta = 0.0;
  return g;
}

int gemm_nn_f64(isdf_handle h, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb,
                double* C, int64_t ldc, bool square) {
  ARG_CHECK(h, A && B && C && lda >= K && ldb >= N && ldc >= N && gemm_nn_f64_supported(h, M, N, K, A, lda, B, ldb));
  const GemmNNArgs g = nn_args(M, N, K, A, lda, B, ldb, C, ldc);
  ARG_CHECK(h, g.nunits_pad < 2147483647LL);
  const size_t lds = sizeof(double) * 2 * (BM2 * LDT + BK * LDN);
  if (int rc = raise_lds_once(h, h->attr_gemm_nn, lds, gemm_nn_mfma_kernel<true>, gemm_nn_mfma_kernel<false>)) return rc;
  ProfScope ps(h, square ? "gemm_nn_mfma_kernel<true>[flop]" : "gemm_nn_mfma_kernel<false>[flop]", 2.0 * M * N * (double)K);
  if (square) hipLaunchKernelGGL(gemm_nn_mfma_kernel<true>, dim3((unsigned)g.nunits_pad), dim3(TPB2), lds, h->stream, g);
  else hipLaunchKernelGGL(gemm_nn_mfma_kernel<false>, dim3((unsigned)g.nunits_pad), dim3(TPB2), lds, h->stream, g);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

// Exposed as isdf_gemm_nn_had (declared in include/mi355_isdf.h).
extern "C" int isdf_gemm_nn_had(isdf_handle h, int M, int64_t N, int K, double alpha, const double* d_A, int64_t lda,
                                const double* d_H, int64_t ldh, const double* d_B, int64_t ldb, double beta, double* d_C,
                                int64_t ldc) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, M > 0 && N > 0 && K > 0 && d_A && d_H && d_B && d_C && lda >= K && ldh >= N && ldb >= N && ldc >= N);
  const bool aligned = N % 2 == 0 && N < 2147483647LL && rows_aligned16(d_A, lda) && rows_aligned16(d_H, ldh) && rows_aligned16(d_B, ldb);
  // the kernel takes the largest multiple-of-32 prefix of K; the K tail, or the whole K of operands it does not fit (an odd N or
  // leading dimension, an unaligned base), goes through the composition: a copy of B times H, then the NN product
  const int Kf = aligned ? K - K % 32 : 0, Kt = K - Kf;
  if (Kt) {
    const double* Bt = d_B + (int64_t)Kf * ldb;
    const double* Ht = d_H + (int64_t)Kf * ldh;
    double* HB = (double*)isdf_ws(h, "nn_had_HB", sizeof(double) * (size_t)Kt * (size_t)N);
    if (!HB) return ISDF_ERR_HIP;
    HIP_TRY(h, hipMemcpy2DAsync(HB, sizeof(double) * (size_t)N, Bt, sizeof(double) * (size_t)ldb, sizeof(double) * (size_t)N,
                                (size_t)Kt, hipMemcpyDeviceToDevice, h->stream));
    for (int r0 = 0; r0 < Kt; r0 += 32768) {
      const int nr = Kt - r0 < 32768 ? Kt - r0 : 32768;
      if (int rc = isdf_hadamard_rows(h, HB + (int64_t)r0 * N, N, Ht + (int64_t)r0 * ldh, ldh, nr, N)) return rc;
    }
    // the tail first, with the caller's beta; the prefix then accumulates onto it
    if (int rc = isdf_gemm_nn(h, M, N, Kt, alpha, d_A + Kf, lda, HB, N, beta, d_C, ldc)) return rc;
    if (!Kf) return ISDF_OK;
    beta = 1.0;
  }
  // any M >= 1: the kernel clamps the rows it loads and bounds the rows it stores
  K = Kf;
  GemmNNArgs g = nn_args(M, N, K, d_A, lda, d_B, ldb, d_C, ldc);
  ARG_CHECK(h, g.nunits_pad < 2147483647LL);
  g.H = d_H; g.ldh = ldh; g.alpha = alpha; g.beta = beta;
  const size_t lds = sizeof(double) * 2 * (BM2 * LDT + BK * LDN);
  if (int rc = raise_lds_once(h, h->attr_gemm_nn_had, lds, gemm_nn_had_kernel)) return rc;
  ProfScope ps(h, "gemm_nn_had_kernel[flop]", 2.0 * M * N * (double)K);
  hipLaunchKernelGGL(gemm_nn_had_kernel, dim3((unsigned)g.nunits_pad), dim3(TPB2), lds, h->stream, g);
  KERNEL_CHECK(h);
  return ISDF_OK;
}
