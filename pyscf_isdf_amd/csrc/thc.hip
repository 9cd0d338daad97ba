// Opposite-spin MP2 from the THC form of the ISDF factors (host orchestration in pyscf_isdf_amd/thc_mp2.py).
// Per Laplace point the energy is Tr[(W A)^2] with A = (Xo diag(so) Xo^T) o (Xv diag(sv) Xv^T); W A is isdf_gemm_nt's.  Here:
//  * thc_pair_kernel: A in ONE pass.  A 128 x 128 output tile per 512-thread workgroup, eight waves in a 2 x 4 grid, each 64 rows x
//    32 columns = 4 x 2 v_mfma_f64_16x16x4_f64 accumulators per factor.  The first K loop (over the occupied columns) fills set 0,
//    the second (over the virtual columns) set 1, the epilogue multiplies them: 2 x 64 = 128 accumulator VGPRs, which leaves the
//    256-register budget of two waves per SIMD room for the staging and fragment registers without scratch - a 64 x 64 sub-tile
//    per wave (2 x 128) would not.  Neither P x P factor is ever stored.  Both operands of a K loop are rows of the same matrix
//    (tile row tm and tile row tn); they go global -> registers -> LDS in 16-deep chunks, double buffered (one barrier per chunk),
//    rows padded to 17 doubles as in gemm_f64.hip.  The scale is multiplied into the B-side values on their way to LDS; a K tail
//    is zero-filled there, rows past P are clamped (computed, never stored).
//    Only tiles with tm >= tn are computed, and of a diagonal tile only the entries with row >= col: every value is stored at
//    (row, col) AND (col, row), so A is symmetric to the bit (the product a_p (s a_q) is not a_q (s a_p) in floating point).
//    Units are the tiles of the lower triangle, row-major, dealt to the XCDs by xcd_unit (neighbours share the tm row panel).
//    Algorithmic work: P (P + 1) (no + nv) flop (the lower triangle: the mirrored half is stores only); bound: FP64 MFMA.
//  * trace_sq: sum_ij B_ij B_ji.  32 x 32 tile pairs (ti >= tj): the tile (tj, ti) goes through LDS so that both reads are
//    coalesced; an off-diagonal pair counts twice.  One partial per workgroup, summed by a second kernel in a fixed order.
// Direct RPA from the same factors (host orchestration in pyscf_isdf_amd/thc_rpa.py): per frequency
// ln det(1 + W S) - Tr(W S) with S_PQ = sum_ia Y_P,ia d_ia Y_Q,ia, Y_P,ia = Xo_Pi Xv_Pa.
//  * thc_chi0_kernel: S in one launch with thc_pair_kernel's tile, wave grid, unit decode, triangle rule and mirrored store, one
//    accumulator set.  The K dimension is the pair index (i, a); the rows of Y are formed at the fragment read (one v_mul_f64 per
//    A fragment, two per B fragment, which carries d) and never stored.
//  * logdet_diag_kernel: sum ln|u_ii|, the count of negative u_ii and of row swaps behind rocsolver_dgetrf, in a fixed order.
#include "common.h"
#include "gemm_tile.h"
#include <cmath>

namespace {

constexpr int PT = 128;          // tile edge
constexpr int PK = 16;           // K chunk
constexpr int PLD = 17;          // doubles per LDS row (gemm_f64.hip's LDT)
constexpr int PTPB = 512;

struct PairArgs {
  const double* Xo; int64_t ldo; int no; const double* so;
  const double* Xv; int64_t ldv; int nv; const double* sv;
  double* A; int64_t lda;
  int P;
  int64_t nunits, nunits_pad;    // nunits_pad: rounded up to a multiple of 8 (XCD remap)
};

// unit u of the row-major lower triangle -> (tm, tn), tn <= tm
__device__ __forceinline__ void decode_tri(int64_t u, int& tm, int& tn) {
  int t = (int)((sqrt(8.0 * (double)u + 1.0) - 1.0) * 0.5);
  while ((int64_t)t * (t + 1) / 2 > u) --t;
  while ((int64_t)(t + 1) * (t + 2) / 2 <= u) ++t;
  tm = t;
  tn = (int)(u - (int64_t)t * (t + 1) / 2);
}

// One K loop of a unit: acc += X[rows of tm] diag(s) X[rows of tn]^T over K columns.  FAST: 16-byte aligned rows (double2 loads
// where the whole quad lies below K); otherwise element-wise with guards.  smem: [2][PT * PLD] A side | [2][PT * PLD] B side.
template <bool FAST>
__device__ __forceinline__ void pair_pass(const double* __restrict__ X, int64_t ld, int K, const double* __restrict__ s, int P,
                                          int tm, int tn, double* smem, d4 (&acc)[4][2]) {
  double* sA = smem;
  double* sB = smem + 2 * PT * PLD;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int srow = tid >> 2, sseg = tid & 3;            // staging: row srow of both tiles, k offset 4 sseg .. + 3
  const double* pa = X + (int64_t)min(tm * PT + srow, P - 1) * ld + 4 * sseg;
  const double* pb = X + (int64_t)min(tn * PT + srow, P - 1) * ld + 4 * sseg;
  const int nchunks = (K + PK - 1) / PK;
  double a0, a1, a2, a3, b0, b1, b2, b3;
#define ISDF_PAIR_LOAD(C)                                                                     \
  {                                                                                           \
    const int k = (C) * PK + 4 * sseg;                                                        \
    const double* qa = pa + (C) * PK;                                                         \
    const double* qb = pb + (C) * PK;                                                         \
    if (k + 3 < K) {                                                                          \
      if (FAST) {                                                                             \
        const double2 u0 = *reinterpret_cast<const double2*>(qa), u1 = *reinterpret_cast<const double2*>(qa + 2);       \
        const double2 v0 = *reinterpret_cast<const double2*>(qb), v1 = *reinterpret_cast<const double2*>(qb + 2);       \
        a0 = u0.x; a1 = u0.y; a2 = u1.x; a3 = u1.y; b0 = v0.x; b1 = v0.y; b2 = v1.x; b3 = v1.y;                         \
      } else {                                                                                \
        a0 = qa[0]; a1 = qa[1]; a2 = qa[2]; a3 = qa[3]; b0 = qb[0]; b1 = qb[1]; b2 = qb[2]; b3 = qb[3];                 \
      }                                                                                       \
      b0 *= s[k]; b1 *= s[k + 1]; b2 *= s[k + 2]; b3 *= s[k + 3];                             \
    } else {                                                                                  \
      a0 = (k < K) ? qa[0] : 0.0;     b0 = (k < K) ? qb[0] * s[k] : 0.0;                      \
      a1 = (k + 1 < K) ? qa[1] : 0.0; b1 = (k + 1 < K) ? qb[1] * s[k + 1] : 0.0;              \
      a2 = (k + 2 < K) ? qa[2] : 0.0; b2 = (k + 2 < K) ? qb[2] * s[k + 2] : 0.0;              \
      a3 = 0.0;                       b3 = 0.0;                                               \
    }                                                                                         \
  }
#define ISDF_PAIR_STORE(BUF)                                                                  \
  {                                                                                           \
    double* qa = sA + (BUF) * PT * PLD + srow * PLD + 4 * sseg;                               \
    double* qb = sB + (BUF) * PT * PLD + srow * PLD + 4 * sseg;                               \
    qa[0] = a0; qa[1] = a1; qa[2] = a2; qa[3] = a3; qb[0] = b0; qb[1] = b1; qb[2] = b2; qb[3] = b3;                     \
  }
  const int frow = lane & 15, fk = lane >> 4;
  const int aoff = (wm * 64 + frow) * PLD + fk, boff = (wn * 32 + frow) * PLD + fk;
  ISDF_PAIR_LOAD(0)
  ISDF_PAIR_STORE(0)
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) ISDF_PAIR_LOAD(c + 1)
    const double* fa = sA + buf * PT * PLD + aoff;
    const double* fb = sB + buf * PT * PLD + boff;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      double af[4], bf[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = fa[i * 16 * PLD + kk * 4];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = fb[j * 16 * PLD + kk * 4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    // the other buffer was last read in chunk c - 1, and every wave has passed that chunk's barrier
    if (c + 1 < nchunks) ISDF_PAIR_STORE(buf ^ 1)
    __syncthreads();
  }
#undef ISDF_PAIR_LOAD
#undef ISDF_PAIR_STORE
}

template <bool FAST>
__global__ __launch_bounds__(PTPB, 2) void thc_pair_kernel(PairArgs g) {
  extern __shared__ double smem[];
  const int64_t unit = xcd_unit(g.nunits_pad);
  if (unit >= g.nunits) return;
  int tm, tn;
  decode_tri(unit, tm, tn);
  d4 acco[4][2], accv[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) { acco[i][j] = (d4){0.0, 0.0, 0.0, 0.0}; accv[i][j] = (d4){0.0, 0.0, 0.0, 0.0}; }
  // the last barrier of the first loop separates its LDS reads from the second loop's first writes
  pair_pass<FAST>(g.Xo, g.ldo, g.no, g.so, g.P, tm, tn, smem, acco);
  pair_pass<FAST>(g.Xv, g.ldv, g.nv, g.sv, g.P, tm, tn, smem, accv);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool diag = tm == tn;
  ISDF_STORE_ACC(4, 2, tm * PT + (wave >> 2) * 64, tn * PT + (wave & 3) * 32, g.P, g.P, {
    if (!(diag && col > row)) {
      const double v = acco[i][j][r] * accv[i][j][r];
      g.A[(int64_t)row * g.lda + col] = v;
      if (row != col) g.A[(int64_t)col * g.lda + row] = v;
    }
  })
}

// ---- direct RPA: S(w) = Y diag(d) Y^T over the pair index, Y never stored --------------------------------------------------------------
struct Chi0Args {
  const double* Xo; int64_t ldo; int no;
  const double* Xv; int64_t ldv; int nv;
  const double* D; int64_t ldd;
  double* S; int64_t lds;
  int P;
  int64_t nunits, nunits_pad;
};

// four values of a row from column k on, zero past K; FAST: the quad is 16-byte aligned
template <bool FAST>
__device__ __forceinline__ void load_quad(const double* __restrict__ q, int k, int K, double (&v)[4]) {
  if (k + 3 < K) {
    if (FAST) {
      const double2 u0 = *reinterpret_cast<const double2*>(q), u1 = *reinterpret_cast<const double2*>(q + 2);
      v[0] = u0.x; v[1] = u0.y; v[2] = u1.x; v[3] = u1.y;
    } else {
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    }
  } else {
    v[0] = (k < K) ? q[0] : 0.0;
    v[1] = (k + 1 < K) ? q[1] : 0.0;
    v[2] = (k + 2 < K) ? q[2] : 0.0;
    v[3] = 0.0;
  }
}

__device__ __forceinline__ void store_quad(double* q, const double (&v)[4]) { q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3]; }

// A chunk is 16 occupied x 16 virtual pair columns: the 16-deep Xv chunk and the 16-wide Xo block of both tile rows and the
// 16 x 16 block of d are staged global -> registers (during the previous chunk's products) -> LDS.  Per chunk a wave reads its Xv
// fragments once and walks the occupied index: a = Xv Xo[., i], b = Xv (Xo[., i] d[i, .]), 4 K-steps of 8 MFMA each.  The Xo
// block is restaged only when the occupied block changes (the virtual chunk is the fast index).
// smem: Xv tm | Xv tn | Xo tm | Xo tn (PT * PLD each) | d (16 x 16)
template <bool FAST>
__global__ __launch_bounds__(PTPB, 2) void thc_chi0_kernel(Chi0Args g) {
  extern __shared__ double smem[];
  const int64_t unit = xcd_unit(g.nunits_pad);
  if (unit >= g.nunits) return;
  int tm, tn;
  decode_tri(unit, tm, tn);
  double* sVa = smem;
  double* sVb = sVa + PT * PLD;
  double* sOa = sVb + PT * PLD;
  double* sOb = sOa + PT * PLD;
  double* sD = sOb + PT * PLD;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int srow = tid >> 2, sseg = tid & 3;            // staging: row srow of both tiles, column offset 4 sseg .. + 3
  const int64_t ra = min(tm * PT + srow, g.P - 1), rb = min(tn * PT + srow, g.P - 1);
  const double* pva = g.Xv + ra * g.ldv + 4 * sseg;
  const double* pvb = g.Xv + rb * g.ldv + 4 * sseg;
  const double* poa = g.Xo + ra * g.ldo + 4 * sseg;
  const double* pob = g.Xo + rb * g.ldo + 4 * sseg;
  const int di = tid >> 4, da = tid & 15;               // staging of d: threads 0 .. 255, entry (di, da) of the block
  const int nvc = (g.nv + PK - 1) / PK, noc = (g.no + PK - 1) / PK;
  d4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  const int frow = lane & 15, fk = lane >> 4;
  const int aoff = (wm * 64 + frow) * PLD, boff = (wn * 32 + frow) * PLD;
  double va[4], vb[4], oa[4], ob[4], dd = 0.0;
#define ISDF_CHI0_LOAD(OB, VC)                                                                \
  {                                                                                           \
    const int k = (VC) * PK + 4 * sseg;                                                       \
    load_quad<FAST>(pva + (VC) * PK, k, g.nv, va);                                            \
    load_quad<FAST>(pvb + (VC) * PK, k, g.nv, vb);                                            \
    if ((VC) == 0) {                                                                          \
      const int i0 = (OB) * PK + 4 * sseg;                                                    \
      load_quad<FAST>(poa + (OB) * PK, i0, g.no, oa);                                         \
      load_quad<FAST>(pob + (OB) * PK, i0, g.no, ob);                                         \
    }                                                                                         \
    if (tid < 256) {                                                                          \
      const int i = (OB) * PK + di, a = (VC) * PK + da;                                       \
      dd = (i < g.no && a < g.nv) ? g.D[(int64_t)i * g.ldd + a] : 0.0;                        \
    }                                                                                         \
  }
#define ISDF_CHI0_STORE(VC)                                                                   \
  {                                                                                           \
    store_quad(sVa + srow * PLD + 4 * sseg, va);                                              \
    store_quad(sVb + srow * PLD + 4 * sseg, vb);                                              \
    if ((VC) == 0) {                                                                          \
      store_quad(sOa + srow * PLD + 4 * sseg, oa);                                            \
      store_quad(sOb + srow * PLD + 4 * sseg, ob);                                            \
    }                                                                                         \
    if (tid < 256) sD[tid] = dd;                                                              \
  }
  ISDF_CHI0_LOAD(0, 0)
  ISDF_CHI0_STORE(0)
  __syncthreads();
  for (int ob_ = 0; ob_ < noc; ++ob_) {
    const int ilen = min(PK, g.no - ob_ * PK);
    for (int vc = 0; vc < nvc; ++vc) {
      const int klen = min(PK, g.nv - vc * PK);
      int nob = ob_, nvc_ = vc + 1;                     // the next chunk
      if (nvc_ == nvc) { nvc_ = 0; ++nob; }
      const bool more = nob < noc;
      if (more) ISDF_CHI0_LOAD(nob, nvc_)
      double av[4][4], bv[4][2];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) av[kk][i] = sVa[aoff + i * 16 * PLD + kk * 4 + fk];
#pragma unroll
        for (int j = 0; j < 2; ++j) bv[kk][j] = sVb[boff + j * 16 * PLD + kk * 4 + fk];
      }
      for (int io = 0; io < ilen; ++io) {
        double xa[4], xb[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) xa[i] = sOa[aoff + i * 16 * PLD + io];
#pragma unroll
        for (int j = 0; j < 2; ++j) xb[j] = sOb[boff + j * 16 * PLD + io];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          if (kk * 4 < klen) {
            const double dk = sD[io * PK + kk * 4 + fk];
            double af[4], bf[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = av[kk][i] * xa[i];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = bv[kk][j] * (xb[j] * dk);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
          }
        }
      }
      __syncthreads();                                  // every wave has read this chunk
      if (more) ISDF_CHI0_STORE(nvc_)
      __syncthreads();
    }
  }
#undef ISDF_CHI0_LOAD
#undef ISDF_CHI0_STORE
  const bool diag = tm == tn;
  ISDF_STORE_ACC(4, 2, tm * PT + wm * 64, tn * PT + wn * 32, g.P, g.P, {
    if (!(diag && col > row)) {
      const double v = acc[i][j][r];
      g.S[(int64_t)row * g.lds + col] = v;
      if (row != col) g.S[(int64_t)col * g.lds + row] = v;
    }
  })
}

// ---- ln|det| from the LU factors ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_unit_diag_kernel(double* __restrict__ A, int64_t lda, int n, double shift) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) A[(int64_t)i * lda + i] += shift;
}

// out[0] = sum_i ln|u_ii|; out[1] = number of negative u_ii + number of row swaps (ipiv[i] != i + 1); out[2] = number of zero or
// non-finite u_ii.  One workgroup: thread t takes i = t, t + 256, ... in order, then the tree: a fixed order.
__global__ __launch_bounds__(256) void logdet_diag_kernel(const double* __restrict__ A, int64_t lda, int n, const int* __restrict__ ipiv,
                                                          double* __restrict__ out) {
  __shared__ double sh[256];
  __shared__ int sn[256], sz[256];
  double s = 0.0;
  int neg = 0, zero = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double u = A[(int64_t)i * lda + i];
    if (!(fabs(u) > 0.0) || !isfinite(u)) { ++zero; continue; }
    s += log(fabs(u));
    neg += (u < 0.0) + (ipiv[i] != i + 1);
  }
  sh[threadIdx.x] = s; sn[threadIdx.x] = neg; sz[threadIdx.x] = zero;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      sh[threadIdx.x] += sh[threadIdx.x + w];
      sn[threadIdx.x] += sn[threadIdx.x + w];
      sz[threadIdx.x] += sz[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = sh[0]; out[1] = (double)sn[0]; out[2] = (double)sz[0]; }
}

// ---- trace of the square -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trace_sq_partial_kernel(const double* __restrict__ B, int64_t ldb, int n,
                                                               double* __restrict__ partial) {
  __shared__ double sT[32][33];
  __shared__ double sh[256];
  int ti, tj;
  decode_tri(blockIdx.x, ti, tj);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  // the partner tile (tj, ti), read along its rows
  for (int rr = ty; rr < 32; rr += 8) {
    const int row = tj * 32 + rr, col = ti * 32 + tx;
    sT[rr][tx] = (row < n && col < n) ? B[(int64_t)row * ldb + col] : 0.0;
  }
  __syncthreads();
  double s = 0.0;
  for (int rr = ty; rr < 32; rr += 8) {
    const int row = ti * 32 + rr, col = tj * 32 + tx;
    if (row < n && col < n) s += B[(int64_t)row * ldb + col] * sT[tx][rr];
  }
  sh[threadIdx.x] = (ti != tj) ? 2.0 * s : s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void trace_sq_final_kernel(const double* __restrict__ partial, int64_t nb, double* __restrict__ out) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += 256) s += partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

bool rows16(const double* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 2 == 0; }

}  // namespace

extern "C" int isdf_thc_pair(isdf_handle h, int P, const double* d_Xo, int64_t ldo, int no, const double* d_so,
                             const double* d_Xv, int64_t ldv, int nv, const double* d_sv, double* d_A, int64_t lda) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, P > 0 && no > 0 && nv > 0 && d_Xo && d_so && d_Xv && d_sv && d_A);
  ARG_CHECK(h, ldo >= no && ldv >= nv && lda >= P);
  PairArgs g;
  g.Xo = d_Xo; g.ldo = ldo; g.no = no; g.so = d_so;
  g.Xv = d_Xv; g.ldv = ldv; g.nv = nv; g.sv = d_sv;
  g.A = d_A; g.lda = lda; g.P = P;
  const int64_t nt = cdiv(P, PT);
  g.nunits = nt * (nt + 1) / 2;
  g.nunits_pad = cdiv(g.nunits, 8) * 8;
  const size_t lds = sizeof(double) * 4 * PT * PLD;
  if (!h->attr_thc_pair) {
    HIP_TRY(h, hipFuncSetAttribute((const void*)thc_pair_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(h, hipFuncSetAttribute((const void*)thc_pair_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->attr_thc_pair = 1;
  }
  ProfScope ps(h, "thc_pair_kernel[flop]", (double)P * ((double)P + 1.0) * ((double)no + nv));   // the lower triangle
  if (rows16(d_Xo, ldo) && rows16(d_Xv, ldv))
    hipLaunchKernelGGL(thc_pair_kernel<true>, dim3((unsigned)g.nunits_pad), dim3(PTPB), lds, h->stream, g);
  else
    hipLaunchKernelGGL(thc_pair_kernel<false>, dim3((unsigned)g.nunits_pad), dim3(PTPB), lds, h->stream, g);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_thc_chi0(isdf_handle h, int P, const double* d_Xo, int64_t ldo, int no, const double* d_Xv, int64_t ldv, int nv,
                             const double* d_D, int64_t ldd, double* d_S, int64_t lds) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, P > 0 && no > 0 && nv > 0 && d_Xo && d_Xv && d_D && d_S);
  ARG_CHECK(h, ldo >= no && ldv >= nv && ldd >= nv && lds >= P);
  Chi0Args g;
  g.Xo = d_Xo; g.ldo = ldo; g.no = no;
  g.Xv = d_Xv; g.ldv = ldv; g.nv = nv;
  g.D = d_D; g.ldd = ldd;
  g.S = d_S; g.lds = lds; g.P = P;
  const int64_t nt = cdiv(P, PT);
  g.nunits = nt * (nt + 1) / 2;
  g.nunits_pad = cdiv(g.nunits, 8) * 8;
  const size_t smem = sizeof(double) * (4 * PT * PLD + PK * PK);
  if (!h->attr_thc_chi0) {
    HIP_TRY(h, hipFuncSetAttribute((const void*)thc_chi0_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    HIP_TRY(h, hipFuncSetAttribute((const void*)thc_chi0_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    h->attr_thc_chi0 = 1;
  }
  ProfScope ps(h, "thc_chi0_kernel[flop]", (double)P * ((double)P + 1.0) * (double)no * (double)nv);   // the lower triangle
  if (rows16(d_Xo, ldo) && rows16(d_Xv, ldv))
    hipLaunchKernelGGL(thc_chi0_kernel<true>, dim3((unsigned)g.nunits_pad), dim3(PTPB), smem, h->stream, g);
  else
    hipLaunchKernelGGL(thc_chi0_kernel<false>, dim3((unsigned)g.nunits_pad), dim3(PTPB), smem, h->stream, g);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_logdet_lu(isdf_handle h, int n, double* d_A, int64_t lda, double shift, double* logabs, int* sign) {
  // A <- the LU factors of A + shift I (rocsolver_dgetrf on the column-major view, which is A^T: the same determinant);
  // *logabs = ln|det|, *sign = +-1; synchronises the work stream
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, n > 0 && d_A && logabs && sign && lda >= n && lda < 2147483647LL);
  int* info = (int*)isdf_ws(h, "logdet_lu", 64 + sizeof(int) * (size_t)n);
  if (!info) return ISDF_ERR_HIP;
  double* out = (double*)(info + 2);                    // 8-byte aligned: the workspace is
  int* ipiv = info + 16;
  if (shift != 0.0) {
    hipLaunchKernelGGL(add_unit_diag_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_A, lda, n, shift);
    KERNEL_CHECK(h);
  }
  {
    ProfScope ps(h, "rocsolver_dgetrf[flop]", 2.0 * (double)n * n * n / 3.0);
    BLAS_TRY(h, rocsolver_dgetrf(h->blas, n, n, d_A, (rocblas_int)lda, ipiv, info));
  }
  hipLaunchKernelGGL(logdet_diag_kernel, dim3(1), dim3(256), 0, h->stream, d_A, lda, n, ipiv, out);
  KERNEL_CHECK(h);
  struct { int info, pad; double out[3]; } host;
  HIP_TRY(h, hipMemcpyAsync(&host, info, sizeof(host), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (host.info != 0 || host.out[2] != 0.0)
    return isdf_fail(h, ISDF_ERR_NUM, "isdf_logdet_lu: the matrix is singular (dgetrf status %d, %d zero or non-finite pivots)", host.info,
                     (int)host.out[2]);
  *logabs = host.out[0];
  *sign = (((int64_t)host.out[1]) & 1) ? -1 : 1;
  return ISDF_OK;
}

extern "C" int isdf_trace_sq(isdf_handle h, int n, const double* d_B, int64_t ldb, double* result) {
  // *result = sum_ij B_ij B_ji; fixed reduction order; synchronises the work stream
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, n > 0 && d_B && result && ldb >= n);
  const int64_t nt = cdiv(n, 32);
  const int64_t nb = nt * (nt + 1) / 2;
  ARG_CHECK(h, nb < 2147483647LL);
  double* part = (double*)isdf_ws(h, "trace_sq_partial", sizeof(double) * (size_t)(nb + 1));
  if (!part) return ISDF_ERR_HIP;
  {
    ProfScope ps(h, "trace_sq_kernel[byte]", 8.0 * n * (double)n);
    hipLaunchKernelGGL(trace_sq_partial_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, d_B, ldb, n, part);
    hipLaunchKernelGGL(trace_sq_final_kernel, dim3(1), dim3(256), 0, h->stream, part, nb, part + nb);
    KERNEL_CHECK(h);
  }
  HIP_TRY(h, hipMemcpyAsync(result, part + nb, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return ISDF_OK;
}
