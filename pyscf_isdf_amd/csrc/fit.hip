// S3: least-squares fit of the interpolation vectors Theta.
//   (a) from the selection's own Cholesky rows:  Theta = T^-1 L,  T = L[:, piv]  (upper triangular)
//   (b) for an arbitrary point set:  Theta = [(aoP aoP^T)^2]^-1 (aoP ao)^2  by Cholesky
// The triangular solves run over all G right-hand sides in place on the (P, G) row-major array.
#include "common.h"
#include <cstdlib>

namespace {

// T[t*k + s] = (s >= t) ? L[t*ldL + piv[s]] : 0
__global__ void gather_T_kernel(const double* __restrict__ L, int64_t ldL,
                                const int64_t* __restrict__ piv, int k, double* __restrict__ T) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = blockIdx.y;
  if (s >= k) return;
  T[(int64_t)t * k + s] = (s >= t) ? L[(int64_t)t * ldL + piv[s]] : 0.0;
}

__global__ void square_kernel(double* __restrict__ x, int64_t rows, int64_t cols, int64_t ld) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (c >= cols) return;
  const double v = x[r * ld + c];
  x[r * ld + c] = v * v;
}

// x = x^2 + y^2 (elementwise), x (rows, ld), y (rows, ldy)
__global__ void square_add_kernel(double* __restrict__ x, int64_t ld, const double* __restrict__ y, int64_t ldy,
                                  int64_t cols) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (c >= cols) return;
  const double a = x[r * ld + c], b = y[r * ldy + c];
  x[r * ld + c] = fma(b, b, a * a);
}

// rot[p, m] = (m < nh) ? aoP[p, nh + m] : -aoP[p, m - nh]     (aoP is (P, 2 nh))
__global__ void rotate_kernel(const double* __restrict__ aoP, int P, int nh, double* __restrict__ rot) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  if (m >= 2 * nh) return;
  rot[(int64_t)p * 2 * nh + m] = (m < nh) ? aoP[(int64_t)p * 2 * nh + nh + m] : -aoP[(int64_t)p * 2 * nh + m - nh];
}

__global__ void transpose_gather_kernel(const double* __restrict__ ao, int64_t ld,
                                        const int64_t* __restrict__ ip, int P, int nao,
                                        double* __restrict__ aoP) {
  // aoP[p*nao + mu] = ao[mu*ld + ip[p]]
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int mu = blockIdx.y;
  if (p >= P) return;
  aoP[(int64_t)p * nao + mu] = ao[(int64_t)mu * ld + ip[p]];
}

}  // namespace

// rows <- aoP ao (P x ng), element-wise squared when `square`: the own MFMA NN kernel with the square in its epilogue where the
// operands fit it (gemm_f64.hip), else rocBLAS and a separate pass
static int product_rows(isdf_handle h, int P, int64_t ng, int nao, const double* d_aoP, const double* d_ao, int64_t ld,
                        double* d_B, int64_t ldb, bool square) {
  if (gemm_nn_f64_supported(h, P, ng, nao, d_aoP, nao, d_ao, ld))
    return gemm_nn_f64(h, P, ng, nao, d_aoP, nao, d_ao, ld, d_B, ldb, square);
  int rc = gemm_rm(h, 'N', 'N', P, ng, nao, 1.0, d_aoP, nao, d_ao, ld, 0.0, d_B, ldb);
  if (rc || !square) return rc;
  hipLaunchKernelGGL(square_kernel, dim3((unsigned)cdiv(ng, 256), (unsigned)P), dim3(256), 0, h->stream, d_B, (int64_t)P, ng,
                     ldb);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_fit_from_chol(isdf_handle h, double* d_L, int k, int64_t m, int64_t ldL,
                                  const int64_t* d_piv) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_L && d_piv && k > 0 && m >= k && ldL >= m);
  double* T = (double*)isdf_ws(h, "fit_T", sizeof(double) * (size_t)k * k);
  if (!T) return ISDF_ERR_HIP;
  ARG_CHECK(h, k <= 65535);
  int rc = isdf_gather_T(h, d_L, k, ldL, d_piv, T);      // its own checks hold after the ones above
  if (rc) return rc;
  // Row-major Theta = T^-1 L  <=>  column-major X * (T as column-major = T^T, lower) = L^T.
  const double one = 1.0;
  ARG_CHECK(h, m < (int64_t)2147483647 && ldL < (int64_t)2147483647);
  BLAS_TRY(h, rocblas_dtrsm(h->blas, rocblas_side_right, rocblas_fill_lower, rocblas_operation_none,
                            rocblas_diagonal_non_unit, (rocblas_int)m, (rocblas_int)k, &one, T,
                            (rocblas_int)k, d_L, (rocblas_int)ldL));
  return ISDF_OK;
}

namespace {
__global__ void add_diag_kernel(double* __restrict__ A, int n, const double* __restrict__ maxdiag, double rel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[(int64_t)i * n + i] += rel * maxdiag[0];
}
__global__ void max_diag_kernel(const double* __restrict__ A, int n, double* __restrict__ out) {
  // single workgroup
  __shared__ double red[256];
  double m = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) m = fmax(m, A[(int64_t)i * n + i]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}
}  // namespace

// A (P, P) = (aoP aoP^T)^2, in complex mode (nh > 0, aoP stored [Re | Im]) (Re S)^2 + (Im S)^2 with Im S = aoP_rot aoP^T
static int gram_sq(isdf_handle h, const double* d_aoP, int P, int nao, int nh, double* d_A) {
  int rc = gemm_rm(h, 'N', 'T', P, P, nao, 1.0, d_aoP, nao, d_aoP, nao, 0.0, d_A, P);
  if (rc) return rc;
  if (nh > 0) {
    double* rot = (double*)isdf_ws(h, "fit_rot", sizeof(double) * (size_t)P * nao);
    double* tmp = (double*)isdf_ws(h, "fit_tmp", sizeof(double) * (size_t)P * P);
    if (!rot || !tmp) return ISDF_ERR_HIP;
    hipLaunchKernelGGL(rotate_kernel, dim3((unsigned)cdiv(nao, 256), (unsigned)P), dim3(256), 0, h->stream, d_aoP, P, nh, rot);
    rc = gemm_rm(h, 'N', 'T', P, P, nao, 1.0, rot, nao, d_aoP, nao, 0.0, tmp, P);
    if (rc) return rc;
    hipLaunchKernelGGL(square_add_kernel, dim3((unsigned)cdiv(P, 256), (unsigned)P), dim3(256), 0, h->stream, d_A,
                       (int64_t)P, tmp, (int64_t)P, (int64_t)P);
  } else {
    hipLaunchKernelGGL(square_kernel, dim3((unsigned)cdiv(P, 256), (unsigned)P), dim3(256), 0, h->stream, d_A,
                       (int64_t)P, (int64_t)P, (int64_t)P);
  }
  KERNEL_CHECK(h);
  return ISDF_OK;
}

// B (P, ng) = (aoP ao)^2, in complex mode (aoP ao)^2 + (aoP_rot ao)^2 with the second product in chunks of 8192 columns
static int pair_rows(isdf_handle h, const double* d_aoP, int P, int nao, int nh, const double* d_ao, int64_t ng, int64_t ld,
                     double* d_B, int64_t ldb) {
  int rc = product_rows(h, P, ng, nao, d_aoP, d_ao, ld, d_B, ldb, nh == 0);
  if (rc) return rc;
  if (nh > 0) {
    const int64_t CH = 8192;
    double* rot = (double*)isdf_ws(h, "fit_rot", sizeof(double) * (size_t)P * nao);
    double* tmp = (double*)isdf_ws(h, "fit_tmpB", sizeof(double) * (size_t)P * CH);
    if (!rot || !tmp) return ISDF_ERR_HIP;
    hipLaunchKernelGGL(rotate_kernel, dim3((unsigned)cdiv(nao, 256), (unsigned)P), dim3(256), 0, h->stream, d_aoP, P, nh, rot);
    for (int64_t c0 = 0; c0 < ng; c0 += CH) {
      const int64_t nc = std::min(CH, ng - c0);
      rc = gemm_rm(h, 'N', 'N', P, nc, nao, 1.0, rot, nao, d_ao + c0, ld, 0.0, tmp, CH);
      if (rc) return rc;
      hipLaunchKernelGGL(square_add_kernel, dim3((unsigned)cdiv(nc, 256), (unsigned)P), dim3(256), 0, h->stream,
                         d_B + c0, ldb, tmp, CH, nc);
    }
  }
  KERNEL_CHECK(h);
  return ISDF_OK;
}

// A (P, P) <- A + rel * max(diag A) * I, the maximum through the device scalar maxdiag
static int shift_diag(isdf_handle h, double* d_A, int P, double rel, double* maxdiag) {
  hipLaunchKernelGGL(max_diag_kernel, dim3(1), dim3(256), 0, h->stream, d_A, P, maxdiag);
  hipLaunchKernelGGL(add_diag_kernel, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, h->stream, d_A, P, maxdiag, rel);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

// The shift ladder of the fit's factorisations: an over-complete point set makes the matrix numerically singular, and a
// diagonal shift relative to its largest diagonal entry cures that.  attempt(i, reg), i = 0 .. attempts - 1, restores the
// matrix, shifts it by reg where reg > 0 and factorises it (rocsolver_dpotrf with its status in the device word info);
// the shifts are reg0, then 1e-14 if that was 0, then 100 times the last.  The first shift that factorises goes to *reg_used;
// when none does, fail(the last shift tried, potrf's status: the failing minor) makes the caller's error.
template <class Attempt, class Fail>
static int shift_ladder(isdf_handle h, int attempts, double reg0, int* info, double* reg_used, Attempt attempt, Fail fail) {
  double reg = reg0;
  int h_info = 0;
  for (int i = 0; i < attempts; ++i) {
    const int rc = attempt(i, reg);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h_info == 0) {
      if (reg_used) *reg_used = reg;
      return ISDF_OK;
    }
    reg = (reg > 0.0) ? reg * 100.0 : 1e-14;
  }
  return fail(reg / 100.0, h_info);
}

// X (P, n) row-major <- L^-1 X (forward), L^-T X (backward) or both in that order (A^-1 X, A = L L^T); d_fac: the row-major
// lower L == the column-major upper U of isdf_fit_prepare / isdf_chol_inplace.  Blocked left-looking (trsm.hip: tri_left)
static int factor_solve(isdf_handle h, const double* d_fac, int P, double* d_X, int64_t n, int64_t ldx, bool forward,
                        bool backward) {
  const int rc = forward ? tri_left(h, false, P, n, d_fac, P, d_X, ldx) : ISDF_OK;
  if (rc || !backward) return rc;
  return tri_left(h, true, P, n, d_fac, P, d_X, ldx);
}

extern "C" int isdf_fit_prepare(isdf_handle h, const double* d_ao, int nao, int64_t ld,
                                const int64_t* d_ip, int P, double reg_rel, double* d_aoP,
                                double* d_chol, double* reg_used) {
  return isdf_fit_prepare_cplx(h, d_ao, nao, 0, ld, d_ip, P, reg_rel, d_aoP, d_chol, reg_used);
}

extern "C" int isdf_fit_prepare_cplx(isdf_handle h, const double* d_ao, int nao, int nh, int64_t ld,
                                     const int64_t* d_ip, int P, double reg_rel, double* d_aoP,
                                     double* d_chol, double* reg_used) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, nh == 0 || 2 * nh == nao);
  ARG_CHECK(h, d_ao && d_ip && d_aoP && d_chol && nao > 0 && P > 0 && reg_rel >= 0.0);
  ARG_CHECK(h, nao <= 65535 && P <= 65535);
  int rc = isdf_gather_aoP(h, d_ao, nao, ld, d_ip, P, d_aoP);      // its own checks hold after the ones above
  if (rc) return rc;
  int* info = (int*)isdf_ws(h, "fit_info", 256);
  if (!info) return ISDF_ERR_HIP;
  double* maxdiag = (double*)(info + 16);
  return shift_ladder(
      h, 5, reg_rel, info, reg_used,
      [&](int, double reg) {
        // A_PP = (aoP aoP^T)^2 (+ reg * max diag * I), rebuilt at every attempt; Cholesky A = U^T U in the column-major view
        int rc = gram_sq(h, d_aoP, P, nao, nh, d_chol);
        if (!rc && reg > 0.0) rc = shift_diag(h, d_chol, P, reg, maxdiag);
        if (rc) return rc;
        ProfScope ps(h, "rocsolver_dpotrf[flop]", (double)P * P * P / 3.0);
        BLAS_TRY(h, rocsolver_dpotrf(h->blas, rocblas_fill_upper, P, d_chol, P, info));
        return ISDF_OK;
      },
      [&](double reg, int) {
        return isdf_fail(h, ISDF_ERR_NUM,
                         "A_PP = (aoP aoP^T)^2 is not numerically positive definite even with diagonal shift %g * max diag", reg);
      });
}

extern "C" int isdf_fit_apply(isdf_handle h, const double* d_chol, const double* d_aoP, int P, int nao,
                              const double* d_ao, int64_t ng, int64_t ld, int forward_only,
                              double* d_theta, int64_t ldt) {
  return isdf_fit_apply_cplx(h, d_chol, d_aoP, P, nao, 0, d_ao, ng, ld, forward_only, d_theta, ldt);
}

extern "C" int isdf_fit_apply_cplx(isdf_handle h, const double* d_chol, const double* d_aoP, int P, int nao,
                                   int nh, const double* d_ao, int64_t ng, int64_t ld, int forward_only,
                                   double* d_theta, int64_t ldt) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, nh == 0 || 2 * nh == nao);
  ARG_CHECK(h, d_chol && d_aoP && d_ao && d_theta && P > 0 && nao > 0 && ng > 0 && ld >= ng && ldt >= ng);
  ARG_CHECK(h, P <= 65535 && ldt < (int64_t)2147483647 && ng < (int64_t)2147483647);
  // B = (aoP ao)^2 (P x ng, row-major) written straight into theta; then in the column-major view
  // X = B_cm U^-1 U^-T  (A = U^T U).
  int rc = pair_rows(h, d_aoP, P, nao, nh, d_ao, ng, ld, d_theta, ldt);
  if (rc) return rc;
  // Theta = A^-1 B with A = Lr Lr^T (Lr = the factor read row-major, lower): forward solve Y = Lr^-1 B, then (unless the
  // caller wants Y, see isdf_W_from_factor) the backward solve Theta = Lr^-T Y
  return factor_solve(h, d_chol, P, d_theta, ng, ldt, true, !forward_only);
}

extern "C" int isdf_fit_global(isdf_handle h, const double* d_ao, int nao, int64_t ngrids, int64_t ld,
                               const int64_t* d_ip, int P, double reg_rel, double* d_theta,
                               int64_t ldt, double* d_aoP, double* reg_used) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, P > 0 && ngrids >= P);
  double* A = (double*)isdf_ws(h, "fit_APP", sizeof(double) * (size_t)P * P);
  if (!A) return ISDF_ERR_HIP;
  int rc = isdf_fit_prepare(h, d_ao, nao, ld, d_ip, P, reg_rel, d_aoP, A, reg_used);
  if (rc) return rc;
  return isdf_fit_apply(h, A, d_aoP, P, nao, d_ao, ngrids, ld, 0, d_theta, ldt);
}

extern "C" int isdf_gather_T(isdf_handle h, const double* d_L, int k, int64_t ldL, const int64_t* d_piv,
                             double* d_T) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_L && d_piv && d_T && k > 0 && k <= 65535);
  hipLaunchKernelGGL(gather_T_kernel, dim3((unsigned)cdiv(k, 256), (unsigned)k), dim3(256), 0, h->stream, d_L,
                     ldL, d_piv, k, d_T);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_W_from_factor(isdf_handle h, const double* d_F, int P, int kind, double* d_M,
                                  int64_t ldm) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_F && d_M && P > 0 && ldm >= P && (kind == 0 || kind == 1 || kind == 2));
  const double one = 1.0;
  // kinds 0 and 2: F is the column-major upper U of A = U^T U, i.e. the row-major lower L with A = L L^T
  if (kind == 2) {
    // M <- U^-T M U^-1 = L^-1 M L^-T  (the other half of A^-1 M A^-1; follow with kind 0)
    int rc = tri_left(h, false, P, P, d_F, P, d_M, ldm);
    if (rc) return rc;
    return tri_right(h, true, P, P, d_F, P, d_M, ldm);
  } else if (kind == 0) {
    // Theta = U^-1 Y  =>  W = U^-1 M U^-T = L^-T M L^-1
    int rc = tri_left(h, true, P, P, d_F, P, d_M, ldm);
    if (rc) return rc;
    return tri_right(h, false, P, P, d_F, P, d_M, ldm);
  } else {
    // F = T (row-major upper) from isdf_gather_T, i.e. column-major lower Lc = T^T,
    // Theta = T^-1 L  =>  W = T^-1 M T^-T = Lc^-T M Lc^-1   (global selection only: rocBLAS)
    ProfScope ps(h, "rocblas_dtrsm[flop]", 2.0 * (double)P * P * P, 2);
    BLAS_TRY(h, rocblas_dtrsm(h->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_transpose,
                              rocblas_diagonal_non_unit, P, P, &one, d_F, P, d_M, (rocblas_int)ldm));
    BLAS_TRY(h, rocblas_dtrsm(h->blas, rocblas_side_right, rocblas_fill_lower, rocblas_operation_none,
                              rocblas_diagonal_non_unit, P, P, &one, d_F, P, d_M, (rocblas_int)ldm));
  }
  return ISDF_OK;
}


// ---- block-Jacobi route: no triangular solve over the grid at all ------------------------------------
// With A = A_PP, B = A_P and D = blockdiag(chol(A_bb)) over the per-atom point blocks:
//   Y' = D^-1 B (cheap, block by block),  M' = w conv(Y') Y'^T,  A' = D^-1 A D^-T,
//   W  = A^-1 [w conv(B) B^T] A^-1 = D^-T [A'^-1 M' A'^-1] D^-1.
// Same W as the Cholesky routes in exact arithmetic; the block scaling keeps the small components of
// M' resolved and lowers the condition number that the two-sided inverse squares.

extern "C" int isdf_gram_sq(isdf_handle h, const double* d_aoP, int P, int nao, int nh, double* d_A) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_aoP && d_A && P > 0 && nao > 0 && P <= 65535 && (nh == 0 || 2 * nh == nao));
  return gram_sq(h, d_aoP, P, nao, nh, d_A);
}

extern "C" int isdf_pair_gram_rows(isdf_handle h, const double* d_aoP, int P, int nao, int nh, const double* d_ao,
                                   int64_t ng, int64_t ld, double* d_B, int64_t ldb) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_aoP && d_ao && d_B && P > 0 && P <= 65535 && nao > 0 && ng > 0 && ld >= ng && ldb >= ng);
  ARG_CHECK(h, nh == 0 || 2 * nh == nao);
  return pair_rows(h, d_aoP, P, nao, nh, d_ao, ng, ld, d_B, ldb);
}

namespace {
__global__ void copy_block_kernel(const double* __restrict__ A, int P, int off, int nb, double* __restrict__ D) {
  // D (P x P, zero elsewhere) diagonal block <- A diagonal block
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (c >= nb) return;
  D[(int64_t)(off + r) * P + off + c] = A[(int64_t)(off + r) * P + off + c];
}
// F (n <= 8 rows, ng) = E (n, P) * Y (P, ng): one grid column per lane, the P-long dot products streamed row by row
// (every load of a wave is one coalesced 512-byte row segment); E staged through LDS in 64-row pieces.  HBM-bound:
// reads Y once.  (rocBLAS dgemm with M = 8 moves the same bytes at under 1 TB/s.)
__global__ __launch_bounds__(256) void skinny_rows_kernel(const double* __restrict__ E, int n, int P, int64_t ldE,
                                                          const double* __restrict__ Y, int64_t ldy, int64_t ng,
                                                          double* __restrict__ F, int64_t ldf, int accumulate) {
  __shared__ double sE[8][64];
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < ng;
  double acc[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
  for (int p0 = 0; p0 < P; p0 += 64) {
    const int np = min(64, P - p0);
    __syncthreads();
    for (int t = threadIdx.x; t < 8 * 64; t += 256) {
      const int j = t >> 6, pp = t & 63;
      sE[j][pp] = (j < n && pp < np) ? E[(int64_t)j * ldE + p0 + pp] : 0.0;
    }
    __syncthreads();
    if (live) {
      const double* y = Y + (int64_t)p0 * ldy + g;
#pragma unroll 8
      for (int pp = 0; pp < np; ++pp) {
        const double v = y[(int64_t)pp * ldy];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fma(sE[j][pp], v, acc[j]);
      }
    }
  }
  if (live)
    for (int j = 0; j < n; ++j) F[(int64_t)j * ldf + g] = accumulate ? F[(int64_t)j * ldf + g] + acc[j] : acc[j];
}

__global__ void add_diag_const_kernel(double* __restrict__ A, int n, int64_t ld, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[(int64_t)i * ld + i] += v;
}
}  // namespace

extern "C" int isdf_block_chol(isdf_handle h, const double* d_A, int P, int nblk, const int32_t* blk_off,
                               double shift_rel, double* d_D, double* shift_used) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_A && d_D && blk_off && P > 0 && nblk > 0 && blk_off[0] == 0 && blk_off[nblk] == P && shift_rel >= 0);
  int* info = (int*)isdf_ws(h, "fit_info", 256);
  if (!info) return ISDF_ERR_HIP;
  double* maxdiag = (double*)(info + 16);
  HIP_TRY(h, hipMemsetAsync(d_D, 0, sizeof(double) * (size_t)P * P, h->stream));
  hipLaunchKernelGGL(max_diag_kernel, dim3(1), dim3(256), 0, h->stream, d_A, P, maxdiag);
  double md = 0.0;
  HIP_TRY(h, hipMemcpyAsync(&md, maxdiag, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  double worst = 0.0;
  for (int b = 0; b < nblk; ++b) {
    const int off = blk_off[b], nb = blk_off[b + 1] - off;
    if (nb <= 0) continue;
    ARG_CHECK(h, nb <= 65535);
    // D is only a preconditioner: any invertible block works as long as the same D is used throughout, so a block
    // that is not numerically positive definite (its points were selected on slightly different AO values, or the
    // set is over-complete) simply gets a larger diagonal shift: shift_rel, then 1e-14, x100 per retry
    // The block is copied afresh at every attempt and shifted by the host value reg * (max diag of the whole A)
    double* Db = d_D + (int64_t)off * P + off;
    double used = 0.0;
    const int rc = shift_ladder(
        h, 6, shift_rel, info, &used,
        [&](int, double reg) {
          hipLaunchKernelGGL(copy_block_kernel, dim3((unsigned)cdiv(nb, 128), (unsigned)nb), dim3(128), 0, h->stream, d_A, P,
                             off, nb, d_D);
          if (reg > 0)
            hipLaunchKernelGGL(add_diag_const_kernel, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, h->stream, Db, nb,
                               (int64_t)P, reg * md);
          KERNEL_CHECK(h);
          // column-major upper factor of the block == row-major lower D_b (A_bb = D_b D_b^T)
          BLAS_TRY(h, rocsolver_dpotrf(h->blas, rocblas_fill_upper, nb, Db, P, info));
          return ISDF_OK;
        },
        [&](double reg, int minor) {
          return isdf_fail(h, ISDF_ERR_NUM, "diagonal block %d of A_PP is not positive definite even with shift %g * max diag "
                           "(minor %d of %d)", b, reg, minor, nb);
        });
    if (rc) return rc;
    worst = std::max(worst, used);
  }
  if (shift_used) *shift_used = worst;
  return ISDF_OK;
}

extern "C" int isdf_block_solve(isdf_handle h, const double* d_D, int P, int nblk, const int32_t* blk_off, int side,
                                int trans, double* d_X, int64_t n, int64_t ldx) {
  // side 0: rows   X (P, n)  <- op(D)^-1 X          (per block of rows)
  // side 1: cols   X (n, P)  <- X op(D)^-1          (per block of columns)
  // op(D) = D (trans 0) or D^T (trans 1); D_b row-major lower = column-major upper U_b = D_b^T
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_D && d_X && blk_off && P > 0 && nblk > 0 && n > 0 && (side == 0 || side == 1) && (trans == 0 || trans == 1));
  ARG_CHECK(h, n < 2147483647LL && ldx < 2147483647LL);
  if (side == 0 && trans == 0 && !h->trsm_substitution) {
    // the hot one (Y' = D^-1 B over the whole grid): all blocks in one launch of the hand-written kernel
    ARG_CHECK(h, blk_off[0] == 0 && blk_off[nblk] <= P);
    return block_forward_solve(h, d_D, P, nblk, blk_off, d_X, ldx, n);
  }
  for (int b = 0; b < nblk; ++b) {
    const int off = blk_off[b], nb = blk_off[b + 1] - off;
    if (nb <= 0) continue;
    const double* Db = d_D + (int64_t)off * P + off;     // row-major lower D_b, leading dimension P
    const int rc = (side == 0) ? tri_left(h, trans != 0, nb, n, Db, P, d_X + (int64_t)off * ldx, ldx)
                               : tri_right(h, trans != 0, nb, n, Db, P, d_X + off, ldx);
    if (rc) return rc;
  }
  return ISDF_OK;
}

namespace {
__global__ void block_identity_kernel(double* __restrict__ E, int P, int n) {
  // ones on the first n diagonal entries of E (P x P, zeroed before): the right-hand side whose block solves are the inverses
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) E[(int64_t)i * P + i] = 1.0;
}
}  // namespace

extern "C" int isdf_block_invert(isdf_handle h, const double* d_D, int P, int nblk, const int32_t* blk_off, double* d_Dinv) {
  // Dinv <- blockdiag(D_b^-1): forward solves of the block factors against the identity.  Entries above the diagonal and
  // outside the blocks are exact zeros (forward substitution of a unit vector never touches the rows above it), so only the
  // columns of a block's own diagonal block are solved; the rest is the memset's +0.0.
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_D && d_Dinv && blk_off && P > 0 && nblk > 0 && blk_off[0] == 0 && blk_off[nblk] <= P);
  HIP_TRY(h, hipMemsetAsync(d_Dinv, 0, sizeof(double) * (size_t)P * (size_t)P, h->stream));
  hipLaunchKernelGGL(block_identity_kernel, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, h->stream, d_Dinv, P, P);
  KERNEL_CHECK(h);
  return block_forward_solve(h, d_D, P, nblk, blk_off, d_Dinv, P, P, true);
}

extern "C" int isdf_block_apply(isdf_handle h, const double* d_Dinv, int64_t ldd, int nblk, const int32_t* blk_off,
                                double* d_X, int64_t n, int64_t ldx) {
  // X (rows of the blocks, n columns) <- Dinv_b X_b, the MFMA form of isdf_block_solve(side 0, trans 0)
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_Dinv && d_X && blk_off && nblk > 0 && n > 0 && ldx >= n && blk_off[0] == 0 && blk_off[nblk] <= ldd);
  return block_apply_inverse(h, d_Dinv, ldd, nblk, blk_off, d_X, ldx, n);
}

extern "C" int isdf_pair_rows_block_apply(isdf_handle h, const double* d_aoP, int P, int nao, const double* d_ao, int64_t ng,
                                          int64_t ld, const double* d_Dinv, int64_t ldd, int nblk, const int32_t* blk_off,
                                          double* d_B, int64_t ldb) {
  // B (P rows = the rows of the blocks, ng) <- Dinv_b (aoP ao)^2: the pair-gram rows and the block solves of the S3c route
  // in two passes over B instead of three - the product aoP ao (rocBLAS; the own NN kernel under option gemm_nn_own, which
  // squares in its epilogue), then the MFMA block apply, which otherwise squares its input while staging it
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_aoP && d_ao && d_Dinv && d_B && blk_off && P > 0 && nao > 0 && ng > 0 && ld >= ng && ldb >= ng && nblk > 0);
  ARG_CHECK(h, blk_off[0] == 0 && blk_off[nblk] == P);
  const bool own = gemm_nn_f64_supported(h, P, ng, nao, d_aoP, nao, d_ao, ld);   // squares in its epilogue
  int rc = product_rows(h, P, ng, nao, d_aoP, d_ao, ld, d_B, ldb, own);
  if (rc) return rc;
  return block_apply_inverse(h, d_Dinv, ldd, nblk, blk_off, d_B, ldb, ng, !own);
}

extern "C" int isdf_pair_rows_squared(isdf_handle h, const double* d_aoP, int rows, int nao, const double* d_ao, int64_t ng,
                                      int64_t ld, int* squared) {
  // which of the two forms isdf_pair_rows_frontier's products take for pieces of `rows` rows: asked once per build
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_aoP && d_ao && squared && rows > 0 && nao > 0 && ng > 0 && ld >= ng);
  *squared = gemm_nn_f64_supported(h, rows, ng, nao, d_aoP, nao, d_ao, ld) ? 1 : 0;
  return ISDF_OK;
}

extern "C" int isdf_pair_rows_frontier(isdf_handle h, const double* d_aoP, int nnew, int nao, const double* d_ao, int64_t ng,
                                       int64_t ld, int squared, const double* d_Dinv, int64_t ldd, int nblk,
                                       const int32_t* blk_off, double* d_B, int64_t ldb, int have) {
  // isdf_pair_rows_block_apply with the product and the block apply on frontiers of their own: the product's row count is the
  // caller's (full GEMM tiles), the block boundaries bind the apply alone.  Rows [have, have + nnew) of B <- aoP ao, then
  // the blocks of blk_off (rows [0, blk_off[nblk]) of B, all of them produced) <- Dinv_b (.)^2.  squared: the products of this
  // build carry the square already (the own NN kernel's epilogue; a piece it does not take gets a pass of its own), else the
  // block apply squares while staging.  Rows past blk_off[nblk] stay as produced for a later call.
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_ao && d_B && nnew >= 0 && nnew <= 65535 && have >= 0 && nblk >= 0 && nao > 0 && ng > 0 && ld >= ng && ldb >= ng);
  ARG_CHECK(h, (nnew == 0 || d_aoP) && (nblk == 0 || (d_Dinv && blk_off && blk_off[0] == 0 && blk_off[nblk] <= have + nnew)));
  if (nnew > 0) {
    double* rows = d_B + (int64_t)have * ldb;
    int rc = squared ? product_rows(h, nnew, ng, nao, d_aoP, d_ao, ld, rows, ldb, true)
                     : gemm_rm(h, 'N', 'N', nnew, ng, nao, 1.0, d_aoP, nao, d_ao, ld, 0.0, rows, ldb);
    if (rc) return rc;
  }
  if (nblk == 0) return ISDF_OK;
  return block_apply_inverse(h, d_Dinv, ldd, nblk, blk_off, d_B, ldb, ng, !squared);
}

extern "C" int isdf_shift_diag(isdf_handle h, double* d_A, int P, double shift_rel) {
  // A <- A + shift_rel * max(diag A) * I  (the fit's regularisation, applied before the block scaling of S3c so that
  // both fit routes solve the same regularised normal equations)
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_A && P > 0 && shift_rel >= 0);
  if (shift_rel == 0.0) return ISDF_OK;
  int* info = (int*)isdf_ws(h, "fit_info", 256);
  if (!info) return ISDF_ERR_HIP;
  return shift_diag(h, d_A, P, shift_rel, (double*)(info + 16));
}

extern "C" int isdf_chol_inplace(isdf_handle h, double* d_A, int P, double shift_rel, double* d_scratch,
                                 double* reg_used) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_A && P > 0 && shift_rel >= 0);
  int* info = (int*)isdf_ws(h, "fit_info", 256);
  // the unshifted matrix is kept for the retries: in the caller's scratch (P*P doubles) when given
  double* keep = d_scratch ? d_scratch : (double*)isdf_ws(h, "chol_keep", sizeof(double) * (size_t)P * P);
  if (!info || !keep) return ISDF_ERR_HIP;
  double* maxdiag = (double*)(info + 16);
  HIP_TRY(h, hipMemcpyAsync(keep, d_A, sizeof(double) * (size_t)P * P, hipMemcpyDeviceToDevice, h->stream));
  return shift_ladder(
      h, 5, shift_rel, info, reg_used,
      [&](int attempt, double reg) {
        if (attempt > 0)
          HIP_TRY(h, hipMemcpyAsync(d_A, keep, sizeof(double) * (size_t)P * P, hipMemcpyDeviceToDevice, h->stream));
        if (reg > 0) {
          const int rc = shift_diag(h, d_A, P, reg, maxdiag);
          if (rc) return rc;
        }
        ProfScope ps(h, "rocsolver_dpotrf[flop]", (double)P * P * P / 3.0);
        BLAS_TRY(h, rocsolver_dpotrf(h->blas, rocblas_fill_upper, P, d_A, P, info));
        return ISDF_OK;
      },
      [&](double reg, int) {
        return isdf_fail(h, ISDF_ERR_NUM, "matrix is not numerically positive definite even with diagonal shift %g * max diag",
                         reg);
      });
}

extern "C" int isdf_factor_solve(isdf_handle h, const double* d_fac, int P, double* d_X, int64_t n, int64_t ldx) {
  // X (P, n) row-major <- A^-1 X = L^-T L^-1 X, A = L L^T (d_fac: row-major lower L == the column-major upper U of
  // isdf_fit_prepare / isdf_chol_inplace)
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_fac && d_X && P > 0 && n > 0 && ldx >= n && n < 2147483647LL && ldx < 2147483647LL);
  return factor_solve(h, d_fac, P, d_X, n, ldx, true, true);
}

extern "C" int isdf_bj_probe_vectors(isdf_handle h, double* d_T, int n, const double* d_fac, const double* d_D, int P,
                                     int nblk, const int32_t* blk_off) {
  // T (n, P) rows t_j  ->  e_j = A'^-1 D^-1 t_j (in place)
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_T && d_fac && d_D && n > 0 && P > 0);
  int rc = isdf_block_solve(h, d_D, P, nblk, blk_off, 1, 1, d_T, n, P);      // t^T D^-T = (D^-1 t)^T
  if (rc) return rc;
  // rows t^T <- t^T A'^-1 = t^T L^-T L^-1  (A' = L L^T symmetric)
  rc = tri_right(h, true, P, n, d_fac, P, d_T, P);
  if (rc) return rc;
  return tri_right(h, false, P, n, d_fac, P, d_T, P);
}

extern "C" int isdf_rows_combine(isdf_handle h, const double* d_E, int n, int64_t ldE, int rows, const double* d_Y,
                                 int64_t ng, int64_t ldy, double* d_F, int64_t ldf, int accumulate) {
  // F (n, ng) (+)= E (n, rows; leading dimension ldE) Y (rows, ng): a few combinations of many long rows, one pass over Y
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_E && d_Y && d_F && n > 0 && rows > 0 && ng > 0 && ldE >= rows && ldy >= ng && ldf >= ng);
  if (n > 8) return gemm_rm(h, 'N', 'N', n, ng, rows, 1.0, d_E, ldE, d_Y, ldy, accumulate ? 1.0 : 0.0, d_F, ldf);
  ProfScope ps(h, "skinny_rows_kernel[byte]", 8.0 * (double)rows * (double)ng);
  hipLaunchKernelGGL(skinny_rows_kernel, dim3((unsigned)cdiv(ng, 256)), dim3(256), 0, h->stream, d_E, n, rows, ldE, d_Y, ldy,
                     ng, d_F, ldf, accumulate ? 1 : 0);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_bj_probe_rows(isdf_handle h, double* d_T, int n, const double* d_fac, const double* d_D, int P,
                                  int nblk, const int32_t* blk_off, const double* d_Yp, int64_t ng, int64_t ldy,
                                  double* d_F, int64_t ldf) {
  // T (n, P) rows t_j  ->  e_j = A'^-1 D^-1 t_j (in place),  F (n, ng) = E Y' = (Theta^T t_j) on the grid columns
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_T && d_fac && d_D && d_Yp && d_F && n > 0 && P > 0 && ng > 0 && ldy >= ng && ldf >= ng);
  int rc = isdf_bj_probe_vectors(h, d_T, n, d_fac, d_D, P, nblk, blk_off);
  if (rc) return rc;
  return isdf_rows_combine(h, d_T, n, P, P, d_Yp, ng, ldy, d_F, ldf, 0);
}

// ---- (AO x occupied orbital) pair space ------------------------------------------------------------------------
// The exchange of a density D = sum_i psi_i psi_i^T only needs the pair products phi_mu psi_i (the reduction the reference makes
// with mo_coeff-tagged density matrices, pyscf/pbc/df/fft_jk.py:206-210,235-238).  Their Gram matrix is
//   A(r, r') = (sum_mu phi_mu(r) phi_mu(r')) * (sum_i psi_i(r) psi_i(r'))
// - the element-wise PRODUCT of two Gram matrices where the AO x AO pair space has the square of one.  Selection, fit, W and K
// keep their formulas; only these two products change.
namespace {
// x (rows, ld) .*= y (rows, ldy) on `cols` columns
__global__ void mul_rows_kernel(double* __restrict__ x, int64_t ld, const double* __restrict__ y, int64_t ldy, int64_t cols) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (c >= cols) return;
  x[r * ld + c] *= y[r * ldy + c];
}
// columns per chunk of the second factor: its (P x chunk) scratch stays under 2 GiB
inline int64_t prod_chunk(int P) {
  int64_t ch = ((int64_t)1 << 28) / std::max(P, 1);
  ch = std::max<int64_t>(1024, std::min<int64_t>(65536, ch));
  return ch / 256 * 256;
}
}  // namespace

extern "C" int isdf_gram_prod(isdf_handle h, const double* d_aoP, int P, int nao, const double* d_psiP, int nocc, double* d_A) {
  // A (P, P) = (aoP aoP^T) o (psiP psiP^T)
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_aoP && d_psiP && d_A && P > 0 && P <= 65535 && nao > 0 && nocc > 0);
  int rc = gemm_rm(h, 'N', 'T', P, P, nao, 1.0, d_aoP, nao, d_aoP, nao, 0.0, d_A, P);
  if (rc) return rc;
  const int64_t CH = prod_chunk(P);                          // rows of the second factor per pass
  double* tmp = (double*)isdf_ws(h, "fit_tmpB", sizeof(double) * (size_t)P * CH);
  if (!tmp) return ISDF_ERR_HIP;
  for (int64_t r0 = 0; r0 < P; r0 += CH) {
    const int64_t nr = std::min<int64_t>(CH, P - r0);
    rc = gemm_rm(h, 'N', 'T', nr, P, nocc, 1.0, d_psiP + r0 * nocc, nocc, d_psiP, nocc, 0.0, tmp, P);
    if (rc) return rc;
    hipLaunchKernelGGL(mul_rows_kernel, dim3((unsigned)cdiv(P, 256), (unsigned)nr), dim3(256), 0, h->stream, d_A + r0 * P,
                       (int64_t)P, tmp, (int64_t)P, (int64_t)P);
  }
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_pair_prod_rows(isdf_handle h, const double* d_aoP, int P, int nao, const double* d_psiP, int nocc,
                                   const double* d_ao, int64_t ld, const double* d_psi, int64_t ldpsi, int64_t ng,
                                   double* d_B, int64_t ldb) {
  // B (P, ng) = (aoP ao) o (psiP psi): the second product in column chunks through the library workspace
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_aoP && d_psiP && d_ao && d_psi && d_B && P > 0 && P <= 65535 && nao > 0 && nocc > 0 && ng > 0);
  ARG_CHECK(h, ld >= ng && ldpsi >= ng && ldb >= ng);
  int rc = product_rows(h, P, ng, nao, d_aoP, d_ao, ld, d_B, ldb, false);
  if (rc) return rc;
  const int64_t CH = prod_chunk(P);
  double* tmp = (double*)isdf_ws(h, "fit_tmpB", sizeof(double) * (size_t)P * CH);
  if (!tmp) return ISDF_ERR_HIP;
  for (int64_t c0 = 0; c0 < ng; c0 += CH) {
    const int64_t nc = std::min(CH, ng - c0);
    rc = gemm_rm(h, 'N', 'N', P, nc, nocc, 1.0, d_psiP, nocc, d_psi + c0, ldpsi, 0.0, tmp, CH);
    if (rc) return rc;
    ProfScope ps(h, "mul_rows_kernel[byte]", 24.0 * (double)P * (double)nc);
    hipLaunchKernelGGL(mul_rows_kernel, dim3((unsigned)cdiv(nc, 256), (unsigned)P), dim3(256), 0, h->stream, d_B + c0, ldb, tmp,
                       CH, nc);
  }
  KERNEL_CHECK(h);
  return ISDF_OK;
}

// ---- (AO x occupied orbital) pair space at k-points ------------------------------------------------------------
// Periodic parts stacked as real rows [Re; Im] (isdf_select_ip_cplx): ao = [Re u; Im u] (2 nh rows), psi = [Re psi~; Im psi~]
// (2 npsi_h rows).  With S_u = sum u(r) conj(u(r')) and S_psi likewise, the pair Gram matrix of conj(u) psi~ has the real part
//   A = Re[S_u conj(S_psi)] = Re S_u Re S_psi + Im S_u Im S_psi,   Re S = xP x,  Im S = xP_rot x,  xP_rot = [Im xP | -Re xP],
// so every product is a pair of real GEMMs with the rotated left factor, and the combine C = A0 o B0 + A1 o B1 is the pass
// over the result that the hand-written kernel below makes.
namespace {
// C (rows, ldc) = A0 o B0 + A1 o B1 on `cols` columns (each operand with its own leading dimension).  Two columns per lane,
// 16-byte loads and stores where the row addresses allow (wave-uniform: every operand row is 16-byte aligned or not), else
// 8-byte ones.  C may be A0 or B0: each element is read before it is written by the same lane.
__global__ __launch_bounds__(256) void prod_combine_kernel(const double* a0, int64_t lda0, const double* a1, int64_t lda1,
                                                           const double* b0, int64_t ldb0, const double* b1, int64_t ldb1,
                                                           double* c, int64_t ldc, int64_t cols) {
  const int64_t col = 2 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  const int64_t r = blockIdx.y;
  if (col >= cols) return;
  const double* pa0 = a0 + r * lda0 + col;
  const double* pa1 = a1 + r * lda1 + col;
  const double* pb0 = b0 + r * ldb0 + col;
  const double* pb1 = b1 + r * ldb1 + col;
  double* pc = c + r * ldc + col;
  const uintptr_t mis = ((uintptr_t)pa0 | (uintptr_t)pa1 | (uintptr_t)pb0 | (uintptr_t)pb1 | (uintptr_t)pc) & 15;
  if (mis == 0 && col + 1 < cols) {
    const double2 x0 = *reinterpret_cast<const double2*>(pa0);
    const double2 x1 = *reinterpret_cast<const double2*>(pa1);
    const double2 y0 = *reinterpret_cast<const double2*>(pb0);
    const double2 y1 = *reinterpret_cast<const double2*>(pb1);
    double2 z;
    z.x = fma(x1.x, y1.x, x0.x * y0.x);
    z.y = fma(x1.y, y1.y, x0.y * y0.y);
    *reinterpret_cast<double2*>(pc) = z;
    return;
  }
  pc[0] = fma(pa1[0], pb1[0], pa0[0] * pb0[0]);
  if (col + 1 < cols) pc[1] = fma(pa1[1], pb1[1], pa0[1] * pb0[1]);
}
// dst (2P, n): rows [0, P) = src (P, n), rows [P, 2P) = src_rot = [src[:, nh:] | -src[:, :nh]]  (n = 2 nh)
__global__ void stack_rot_kernel(const double* __restrict__ src, int P, int nh, double* __restrict__ dst) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = blockIdx.y;
  const int n = 2 * nh;
  if (m >= n) return;
  const double* s = src + (int64_t)p * n;
  dst[(int64_t)p * n + m] = s[m];
  dst[(int64_t)(P + p) * n + m] = (m < nh) ? s[nh + m] : -s[m - nh];
}
int prod_combine(isdf_handle h, const double* a0, int64_t lda0, const double* a1, int64_t lda1, const double* b0, int64_t ldb0,
                 const double* b1, int64_t ldb1, double* c, int64_t ldc, int rows, int64_t cols) {
  ProfScope ps(h, "prod_combine_kernel[byte]", 40.0 * (double)rows * (double)cols);
  hipLaunchKernelGGL(prod_combine_kernel, dim3((unsigned)cdiv(cols, 512), (unsigned)rows), dim3(256), 0, h->stream, a0, lda0,
                     a1, lda1, b0, ldb0, b1, ldb1, c, ldc, cols);
  KERNEL_CHECK(h);
  return ISDF_OK;
}
}  // namespace

extern "C" int isdf_gram_prod_cplx(isdf_handle h, const double* d_aoP, int P, int nao, int nh, const double* d_psiP, int npsi,
                                   int npsi_h, double* d_A) {
  // A (P, P) = (aoP aoP^T) o (psiP psiP^T) + (aoP_rot aoP^T) o (psiP_rot psiP^T); the last three products in row chunks
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_aoP && d_psiP && d_A && P > 0 && P <= 65535 && nh > 0 && nao == 2 * nh && npsi_h > 0 && npsi == 2 * npsi_h);
  int rc = gemm_rm(h, 'N', 'T', P, P, nao, 1.0, d_aoP, nao, d_aoP, nao, 0.0, d_A, P);
  if (rc) return rc;
  double* ao2 = (double*)isdf_ws(h, "occk_ao2", sizeof(double) * (size_t)2 * P * nao);
  double* psi2 = (double*)isdf_ws(h, "occk_psi2", sizeof(double) * (size_t)2 * P * npsi);
  // three (rows x P) products per chunk in at most 2 GiB
  const int64_t CH = std::max<int64_t>(1, std::min<int64_t>(P, ((int64_t)1 << 28) / (3 * (int64_t)P)));
  double* tmp = (double*)isdf_ws(h, "occk_tmp", sizeof(double) * (size_t)3 * CH * P);
  if (!ao2 || !psi2 || !tmp) return ISDF_ERR_HIP;
  hipLaunchKernelGGL(stack_rot_kernel, dim3((unsigned)cdiv(nao, 256), (unsigned)P), dim3(256), 0, h->stream, d_aoP, P, nh, ao2);
  hipLaunchKernelGGL(stack_rot_kernel, dim3((unsigned)cdiv(npsi, 256), (unsigned)P), dim3(256), 0, h->stream, d_psiP, P, npsi_h,
                     psi2);
  KERNEL_CHECK(h);
  double* T1 = tmp;
  double* U0 = tmp + CH * P;
  double* U1 = tmp + 2 * CH * P;
  for (int64_t r0 = 0; r0 < P; r0 += CH) {
    const int nr = (int)std::min<int64_t>(CH, P - r0);
    rc = gemm_rm(h, 'N', 'T', nr, P, nao, 1.0, ao2 + (P + r0) * nao, nao, d_aoP, nao, 0.0, T1, P);
    if (!rc) rc = gemm_rm(h, 'N', 'T', nr, P, npsi, 1.0, psi2 + r0 * npsi, npsi, d_psiP, npsi, 0.0, U0, P);
    if (!rc) rc = gemm_rm(h, 'N', 'T', nr, P, npsi, 1.0, psi2 + (P + r0) * npsi, npsi, d_psiP, npsi, 0.0, U1, P);
    if (!rc) rc = prod_combine(h, d_A + r0 * P, P, T1, P, U0, P, U1, P, d_A + r0 * P, P, nr, P);
    if (rc) return rc;
  }
  return ISDF_OK;
}

extern "C" int isdf_pair_prod_rows_cplx(isdf_handle h, const double* d_aoP, int P, int nao, int nh, const double* d_psiP,
                                        int npsi, int npsi_h, const double* d_ao, int64_t ld, const double* d_psi, int64_t ldpsi,
                                        int64_t ng, double* d_B, int64_t ldb) {
  // B (P, ng) = (aoP ao) o (psiP psi) + (aoP_rot ao) o (psiP_rot psi): per column chunk the two M = 2P products
  // [aoP; aoP_rot] ao and [psiP; psiP_rot] psi, then one combine pass into B
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_aoP && d_psiP && d_ao && d_psi && d_B && P > 0 && P <= 65535 && nh > 0 && nao == 2 * nh && npsi_h > 0 &&
               npsi == 2 * npsi_h && ng > 0);
  ARG_CHECK(h, ld >= ng && ldpsi >= ng && ldb >= ng);
  double* ao2 = (double*)isdf_ws(h, "occk_ao2", sizeof(double) * (size_t)2 * P * nao);
  double* psi2 = (double*)isdf_ws(h, "occk_psi2", sizeof(double) * (size_t)2 * P * npsi);
  // two (2P x CH) products in at most 2 GiB
  int64_t CH = ((int64_t)1 << 26) / P;
  CH = std::max<int64_t>(256, std::min<int64_t>(65536, CH)) / 256 * 256;
  double* tmp = (double*)isdf_ws(h, "occk_tmp", sizeof(double) * (size_t)4 * P * CH);
  if (!ao2 || !psi2 || !tmp) return ISDF_ERR_HIP;
  hipLaunchKernelGGL(stack_rot_kernel, dim3((unsigned)cdiv(nao, 256), (unsigned)P), dim3(256), 0, h->stream, d_aoP, P, nh, ao2);
  hipLaunchKernelGGL(stack_rot_kernel, dim3((unsigned)cdiv(npsi, 256), (unsigned)P), dim3(256), 0, h->stream, d_psiP, P, npsi_h,
                     psi2);
  KERNEL_CHECK(h);
  double* tA = tmp;
  double* tB = tmp + 2 * P * CH;
  for (int64_t c0 = 0; c0 < ng; c0 += CH) {
    const int64_t nc = std::min(CH, ng - c0);
    int rc = product_rows(h, 2 * P, nc, nao, ao2, d_ao + c0, ld, tA, CH, false);
    if (!rc) rc = product_rows(h, 2 * P, nc, npsi, psi2, d_psi + c0, ldpsi, tB, CH, false);
    if (!rc) rc = prod_combine(h, tA, CH, tA + P * CH, CH, tB, CH, tB + P * CH, CH, d_B + c0, ldb, P, nc);
    if (rc) return rc;
  }
  return ISDF_OK;
}

extern "C" int isdf_factor_solve_half(isdf_handle h, const double* d_fac, int P, int backward, double* d_X, int64_t n,
                                      int64_t ldx) {
  // X (P, n) row-major <- L^-1 X (backward 0) or L^-T X (backward 1), A = L L^T (d_fac as in isdf_factor_solve): the two halves
  // of the Cholesky fit route for rows the caller produced itself (isdf_pair_prod_rows)
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_fac && d_X && P > 0 && n > 0 && ldx >= n && n < 2147483647LL && ldx < 2147483647LL);
  return factor_solve(h, d_fac, P, d_X, n, ldx, backward == 0, backward != 0);
}

extern "C" int isdf_gather_aoP(isdf_handle h, const double* d_ao, int nao, int64_t ld, const int64_t* d_ip, int P,
                               double* d_aoP) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_ao && d_ip && d_aoP && nao > 0 && nao <= 65535 && P > 0);
  hipLaunchKernelGGL(transpose_gather_kernel, dim3((unsigned)cdiv(P, 256), (unsigned)nao), dim3(256), 0, h->stream, d_ao,
                     ld, d_ip, P, nao, d_aoP);
  KERNEL_CHECK(h);
  return ISDF_OK;
}
