// S4: the Coulomb convolution V = ifft(coulG fft(rows)) of a batch of real fields, hand-written for gfx950.
//
// hipFFT runs a batched 3-D real transform as three unfused passes per direction plus our separate kernel multiply:
// seven kernels, each reading and writing the whole batch (112 G bytes per row against 32 G algorithmic; measured 0.9 TB/s
// algorithmic in round 1).  Here the same arithmetic takes FIVE passes (80 G bytes per row), every one a streaming kernel
// whose 1-D transforms live in LDS:
//
//   1. z, real -> half complex   lines are contiguous; TWO real lines ride one complex transform (a + i b) and are
//                                separated afterwards (A_k = (Z_k + conj Z_{n-k}) / 2, B_k = (Z_k - conj Z_{n-k}) / 2i)
//   2. y forward                 lines strided by n2h; a workgroup takes all n1 elements of 16 ADJACENT lines, so every global
//                                access is a 256-byte run and the LDS layout [element][line] is bank-conflict free
//   3. x forward, x coulG, x inverse   the same kernel along the slowest axis, kernel multiply fused between the two
//                                transforms (the table already carries the 1/G of the inverse, pbc.py:182-211)
//   4. y inverse
//   5. z, half complex -> real   the inverse of pass 1 (imaginary parts of the self-conjugate entries are ignored, as
//                                hipFFT's Z2D does)
//
// The 1-D transform is a Stockham autosort FFT (decimation in frequency, natural order in and out) over the mixed radices of n;
// twiddles W_n^k = exp(-2 pi i k / n) come from a host-made double table.  One butterfly per thread and stage, consecutive
// threads on consecutive lines.  Meshes with a prime factor above 13 (or a dimension above 1024) fall back to hipFFT in
// coulomb.hip.
//
// Structure of this file.  Each of the five passes (z_r2c, strided_fft, z_c2r) exists in two forms:
//   FAST (every dimension 2-3-5 smooth, all production meshes)  ONE LDS buffer - a stage reads its butterflies' inputs, keeps
//     the outputs in registers across a barrier and writes them back in place (stage()), so a workgroup needs
//     n x 16 lines x 16 B <= 32 KB and five workgroups share a CU (the passes are latency chains of load / stages / store:
//     occupancy is what hides them); radices up to 16 in registers; twiddles staged in LDS; the number of lines per tile is a
//     compile-time power of two and the divisions by the stage stride go through a float reciprocal.
//   GENERIC (a factor 7, 11 or 13 somewhere)  two LDS buffers, plain Stockham out of place (stockham_stage()):
//     2, 3, 4, 5 hard-coded with the output twiddle fused in, 7 / 11 / 13 by an O(r^2) butterfly; twiddles from global memory.
// The two forms share the pair separation / merge, the real-line layout and the launch helpers (launch_z, launch_strided).
// The PLANE path fuses the z and y passes of one (y, z) plane in LDS (three passes instead of five): one body per direction
// (plane_fwd_body, plane_inv_body, plane_c2c_inv_body) over a dims type - PlaneAny (runtime sizes, one workgroup of 1024
// threads per plane) or PlaneSquare<N, RA, RB> (compile-time sizes, persistent workgroups of 768 threads with the next plane
// prefetched).  Both paths run the same register-held stage() through one fft(), which turns the runtime radix into the
// template argument.
// Host side: make_axes() (factorisation + twiddle tables), plane_geometry() (what fits the 160 KB of LDS), one table of the
// pipelined plane sizes (ISDF_PLANE_SIZES) behind the three plane launchers.
//
// Reference semantics: pyscf/pbc/tools/pbc.py:149-211 (fft unscaled, ifft 1/N, C order over the mesh).
#include "common.h"
#include <type_traits>

namespace {

constexpr int TPB = 256;
constexpr int MAXSTAGE = 12;

struct Axis {
  int n;
  int nstage;
  int radix[MAXSTAGE];
  const double2* tw;     // n entries, exp(-2 pi i k / n)
};

__device__ inline double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ inline double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ inline double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// multiply by SIGN * i
template <int SIGN>
__device__ inline double2 mul_si(double2 a) { return SIGN > 0 ? make_double2(-a.y, a.x) : make_double2(a.y, -a.x); }
template <int SIGN>
__device__ inline double2 twid(const double2* __restrict__ tw, int idx) {
  double2 w = tw[idx];
  if (SIGN > 0) w.y = -w.y;
  return w;
}

// c / n through the float reciprocal inv = 1.0f / n (exact for the index ranges here: c n < 2^23)
__device__ inline int fdiv(int c, float inv) { return (int)(((float)c + 0.5f) * inv); }

// the thread index, opaque to the optimiser (the pipelined plane kernels say why)
__device__ inline int opaque_tid() {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  return tid;
}

__device__ inline void stage_twiddles(double2* __restrict__ dst, const Axis& ax, int n, int nthreads) {
  for (int k = threadIdx.x; k < n; k += nthreads) dst[k] = ax.tw[k];
}

// Two real lines ride one complex transform, z = a + i b.  Sample e of line l of a tile sits in x[e * L + (l >> 1)], component
// l & 1: this is the scatter / gather between the real lines and that layout.
__device__ inline double& real_slot(double2* x, int L, int l, int e) { return ((double*)(x + e * L + (l >> 1)))[l & 1]; }

// after the transform: A_k = (Z_k + conj Z_{n-k}) / 2 (the even line), B_k = (Z_k - conj Z_{n-k}) / 2i (the odd one)
__device__ inline double2 separate_pair(double2 zk, double2 zn, bool odd) {
  if (!odd) return make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y - zn.y));
  return make_double2(0.5 * (zk.y + zn.y), -0.5 * (zk.x - zn.x));
}

// before the inverse: Z_k = A_k + i B_k (k <= n/2),  Z_{n-k} = conj(A_k) + i conj(B_k);  the imaginary parts of the
// self-conjugate bins (k = 0, 2 k = n) are ignored, and those bins have no Z_{n-k} to store
__device__ inline void merge_pair(double2 a, double2 b, bool selfconj, double2* z_lo, double2* z_hi) {
  if (selfconj) { a.y = 0.0; b.y = 0.0; }
  *z_lo = make_double2(a.x - b.y, a.y + b.x);
  *z_hi = make_double2(a.x + b.y, -a.y + b.x);
}

// ---- butterflies ---------------------------------------------------------------------------------------------------
template <int SIGN, int R>
__device__ inline void butterfly_r(const double2* a, double2* b) {
  if (R == 2) {
    b[0] = cadd(a[0], a[1]);
    b[1] = csub(a[0], a[1]);
  } else if (R == 3) {
    const double2 t1 = cadd(a[1], a[2]);
    const double2 t2 = make_double2(a[0].x - 0.5 * t1.x, a[0].y - 0.5 * t1.y);
    const double2 d = csub(a[1], a[2]);
    const double2 t3 = mul_si<SIGN>(make_double2(0.86602540378443864676 * d.x, 0.86602540378443864676 * d.y));
    b[0] = cadd(a[0], t1);
    b[1] = cadd(t2, t3);
    b[2] = csub(t2, t3);
  } else if (R == 4) {
    const double2 u0 = cadd(a[0], a[2]), u1 = csub(a[0], a[2]), u2 = cadd(a[1], a[3]), u3 = mul_si<SIGN>(csub(a[1], a[3]));
    b[0] = cadd(u0, u2);
    b[1] = cadd(u1, u3);
    b[2] = csub(u0, u2);
    b[3] = csub(u1, u3);
  } else {
    const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;
    const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;
    const double2 t1 = cadd(a[1], a[4]), t2 = cadd(a[2], a[3]), t3 = csub(a[1], a[4]), t4 = csub(a[2], a[3]);
    const double2 r1 = make_double2(a[0].x + c1 * t1.x + c2 * t2.x, a[0].y + c1 * t1.y + c2 * t2.y);
    const double2 r2 = make_double2(a[0].x + c2 * t1.x + c1 * t2.x, a[0].y + c2 * t1.y + c1 * t2.y);
    const double2 i1 = mul_si<SIGN>(make_double2(s1 * t3.x + s2 * t4.x, s1 * t3.y + s2 * t4.y));
    const double2 i2 = mul_si<SIGN>(make_double2(s2 * t3.x - s1 * t4.x, s2 * t3.y - s1 * t4.y));
    b[0] = make_double2(a[0].x + t1.x + t2.x, a[0].y + t1.y + t2.y);
    b[1] = cadd(r1, i1);
    b[2] = cadd(r2, i2);
    b[3] = csub(r2, i2);
    b[4] = csub(r1, i1);
  }
}

// exp(-2 pi i k / R) for the composite radices, as literals: the constant twiddles inside a composite butterfly then cost no
// LDS read (they were 6 of the 29 reads of a radix-12 butterfly) and the trivial ones (1, -i, ...) fold away.  k is a compile-time
// constant wherever this is called (fully unrolled loops).
template <int SIGN, int R>
__device__ inline double2 const_twid(int k) {
  if constexpr (R == 6) {
    constexpr double c[6] = {1.0, 0.5000000000000001, -0.4999999999999998, -1.0, -0.5000000000000004, 0.5000000000000001};
    constexpr double sn[6] = {-0.0, -0.8660254037844386, -0.8660254037844387, -1.2246467991473532e-16, 0.8660254037844384, 0.8660254037844386};
    return make_double2(c[k], SIGN > 0 ? -sn[k] : sn[k]);
  }
  else if constexpr (R == 8) {
    constexpr double c[8] = {1.0, 0.7071067811865476, 6.123233995736766e-17, -0.7071067811865475, -1.0, -0.7071067811865477, -1.8369701987210297e-16, 0.7071067811865474};
    constexpr double sn[8] = {-0.0, -0.7071067811865475, -1.0, -0.7071067811865476, -1.2246467991473532e-16, 0.7071067811865475, 1.0, 0.7071067811865477};
    return make_double2(c[k], SIGN > 0 ? -sn[k] : sn[k]);
  }
  else if constexpr (R == 9) {
    constexpr double c[9] = {1.0, 0.766044443118978, 0.17364817766693041, -0.4999999999999998, -0.9396926207859083, -0.9396926207859084, -0.5000000000000004, 0.17364817766692997, 0.7660444431189778};
    constexpr double sn[9] = {-0.0, -0.6427876096865393, -0.984807753012208, -0.8660254037844387, -0.3420201433256689, 0.34202014332566866, 0.8660254037844384, 0.9848077530122081, 0.6427876096865396};
    return make_double2(c[k], SIGN > 0 ? -sn[k] : sn[k]);
  }
  else if constexpr (R == 10) {
    constexpr double c[10] = {1.0, 0.8090169943749475, 0.30901699437494745, -0.30901699437494734, -0.8090169943749473, -1.0, -0.8090169943749476, -0.30901699437494756, 0.30901699437494723, 0.8090169943749473};
    constexpr double sn[10] = {-0.0, -0.5877852522924731, -0.9510565162951535, -0.9510565162951536, -0.5877852522924732, -1.2246467991473532e-16, 0.587785252292473, 0.9510565162951535, 0.9510565162951536, 0.5877852522924734};
    return make_double2(c[k], SIGN > 0 ? -sn[k] : sn[k]);
  }
  else if constexpr (R == 12) {
    constexpr double c[12] = {1.0, 0.8660254037844387, 0.5000000000000001, 6.123233995736766e-17, -0.4999999999999998, -0.8660254037844387, -1.0, -0.8660254037844388, -0.5000000000000004, -1.8369701987210297e-16, 0.5000000000000001, 0.8660254037844384};
    constexpr double sn[12] = {-0.0, -0.49999999999999994, -0.8660254037844386, -1.0, -0.8660254037844387, -0.49999999999999994, -1.2246467991473532e-16, 0.4999999999999997, 0.8660254037844384, 1.0, 0.8660254037844386, 0.5000000000000004};
    return make_double2(c[k], SIGN > 0 ? -sn[k] : sn[k]);
  }
  else if constexpr (R == 15) {
    constexpr double c[15] = {1.0, 0.9135454576426009, 0.6691306063588582, 0.30901699437494745, -0.10452846326765333, -0.4999999999999998, -0.8090169943749473, -0.9781476007338057, -0.9781476007338057, -0.8090169943749476, -0.5000000000000004, -0.10452846326765423, 0.30901699437494723, 0.6691306063588585, 0.913545457642601};
    constexpr double sn[15] = {-0.0, -0.40673664307580015, -0.7431448254773941, -0.9510565162951535, -0.9945218953682734, -0.8660254037844387, -0.5877852522924732, -0.20791169081775931, 0.20791169081775907, 0.587785252292473, 0.8660254037844384, 0.9945218953682733, 0.9510565162951536, 0.743144825477394, 0.40673664307580015};
    return make_double2(c[k], SIGN > 0 ? -sn[k] : sn[k]);
  }
  else if constexpr (R == 16) {
    constexpr double c[16] = {1.0, 0.9238795325112867, 0.7071067811865476, 0.38268343236508984, 6.123233995736766e-17, -0.3826834323650897, -0.7071067811865475, -0.9238795325112867, -1.0, -0.9238795325112868, -0.7071067811865477, -0.38268343236509034, -1.8369701987210297e-16, 0.38268343236509, 0.7071067811865474, 0.9238795325112865};
    constexpr double sn[16] = {-0.0, -0.3826834323650898, -0.7071067811865475, -0.9238795325112867, -1.0, -0.9238795325112867, -0.7071067811865476, -0.3826834323650899, -1.2246467991473532e-16, 0.38268343236508967, 0.7071067811865475, 0.9238795325112865, 1.0, 0.9238795325112866, 0.7071067811865477, 0.3826834323650904};
    return make_double2(c[k], SIGN > 0 ? -sn[k] : sn[k]);
  }
  else return make_double2(1.0, 0.0);
}

// Composite radices in registers: R = R1 R2 point DFT as R2 DFTs of length R1 (inputs R2 apart), the constant twiddles
// W_R^(n2 k1) = tw[n2 k1 N / R] (R divides N, so the axis table holds them), then R1 DFTs of length R2; output index k1 + R1 k2.
// A 120-point line is then two stages (15 x 8) instead of four (4 x 2 x 3 x 5): half the LDS round trips and barriers, which is
// what bounds these passes.
template <int SIGN, int R1, int R2, bool CT>
__device__ inline void butterfly_comp(const double2* a, double2* b, const double2* __restrict__ tw, int N) {
  constexpr int R = R1 * R2;
  double2 t[R2][R1];
#pragma unroll
  for (int n2 = 0; n2 < R2; ++n2) {
    double2 u[R1];
#pragma unroll
    for (int n1 = 0; n1 < R1; ++n1) u[n1] = a[R2 * n1 + n2];
    butterfly_r<SIGN, R1>(u, t[n2]);
  }
  // CT: literals (no LDS read; needs a few more registers for the constants - the 1024-thread plane kernels, at 113-115 of their
  // 128 VGPRs, keep the table)
  const int step = N / R;
#pragma unroll
  for (int n2 = 1; n2 < R2; ++n2)
#pragma unroll
    for (int k1 = 1; k1 < R1; ++k1)
      t[n2][k1] = cmul(t[n2][k1], CT ? const_twid<SIGN, R>(n2 * k1) : twid<SIGN>(tw, n2 * k1 * step));
#pragma unroll
  for (int k1 = 0; k1 < R1; ++k1) {
    double2 v[R2], w[R2];
#pragma unroll
    for (int n2 = 0; n2 < R2; ++n2) v[n2] = t[n2][k1];
    butterfly_r<SIGN, R2>(v, w);
#pragma unroll
    for (int k2 = 0; k2 < R2; ++k2) b[k1 + R1 * k2] = w[k2];
  }
}

template <int SIGN, int R, bool CT = true>
__device__ inline void butterfly_any(const double2* a, double2* b, const double2* __restrict__ tw, int N) {
  if (R <= 5) butterfly_r<SIGN, (R <= 5 ? R : 2)>(a, b);
  else if (R == 6) butterfly_comp<SIGN, 3, 2, CT>(a, b, tw, N);
  else if (R == 8) butterfly_comp<SIGN, 4, 2, CT>(a, b, tw, N);
  else if (R == 9) butterfly_comp<SIGN, 3, 3, CT>(a, b, tw, N);
  else if (R == 10) butterfly_comp<SIGN, 5, 2, CT>(a, b, tw, N);
  else if (R == 12) butterfly_comp<SIGN, 4, 3, CT>(a, b, tw, N);
  else if (R == 15) butterfly_comp<SIGN, 5, 3, CT>(a, b, tw, N);
  else butterfly_comp<SIGN, 4, 4, CT>(a, b, tw, N);        // 16
}

// ---- GENERIC stages: Stockham ping-pong between two LDS buffers ------------------------------------------------------------
// One stage of radix r on M lines held as x[element * Ls + line]:  n_cur = current sub-length, s = stride.
// The radix 2 - 5 legs stay written out, butterfly fused with the output twiddle: routed through butterfly_r the compiler
// contracts the radix-3 legs' twiddle multiply around the other product and two GENERIC meshes change in the last bit.
template <int SIGN>
__device__ inline void stockham_stage(const double2* __restrict__ x, double2* __restrict__ y, int N, int n_cur, int s, int r,
                                      int Ls, int M, const double2* __restrict__ tw) {
  const int mm = n_cur / r;
  const int nbf = N / r;
  for (int i = threadIdx.x; i < nbf * M; i += TPB) {
    const int m = i % M, bf = i / M;
    const int q = bf % s, p = bf / s;
    const double2* xi = x + (int64_t)(q + s * p) * Ls + m;
    double2* yo = y + (int64_t)(q + s * r * p) * Ls + m;
    const int sin_ = s * mm * Ls;      // input step between the r legs
    const int sout = s * Ls;           // output step
    const int tstep = (p * s) % N;     // twiddle exponent of leg 1
    if (r == 4) {
      const double2 a0 = xi[0], a1 = xi[sin_], a2 = xi[2 * sin_], a3 = xi[3 * sin_];
      const double2 u0 = cadd(a0, a2), u1 = csub(a0, a2), u2 = cadd(a1, a3), u3 = mul_si<SIGN>(csub(a1, a3));
      yo[0] = cadd(u0, u2);
      yo[sout] = cmul(cadd(u1, u3), twid<SIGN>(tw, tstep));
      yo[2 * sout] = cmul(csub(u0, u2), twid<SIGN>(tw, (2 * tstep) % N));
      yo[3 * sout] = cmul(csub(u1, u3), twid<SIGN>(tw, (3 * tstep) % N));
    } else if (r == 2) {
      const double2 a0 = xi[0], a1 = xi[sin_];
      yo[0] = cadd(a0, a1);
      yo[sout] = cmul(csub(a0, a1), twid<SIGN>(tw, tstep));
    } else if (r == 3) {
      const double2 a0 = xi[0], a1 = xi[sin_], a2 = xi[2 * sin_];
      const double2 t1 = cadd(a1, a2);
      const double2 t2 = make_double2(a0.x - 0.5 * t1.x, a0.y - 0.5 * t1.y);
      const double2 d = csub(a1, a2);
      const double2 t3 = mul_si<SIGN>(make_double2(0.86602540378443864676 * d.x, 0.86602540378443864676 * d.y));
      yo[0] = cadd(a0, t1);
      yo[sout] = cmul(cadd(t2, t3), twid<SIGN>(tw, tstep));
      yo[2 * sout] = cmul(csub(t2, t3), twid<SIGN>(tw, (2 * tstep) % N));
    } else if (r == 5) {
      const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;
      const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;
      const double2 a0 = xi[0], a1 = xi[sin_], a2 = xi[2 * sin_], a3 = xi[3 * sin_], a4 = xi[4 * sin_];
      const double2 t1 = cadd(a1, a4), t2 = cadd(a2, a3), t3 = csub(a1, a4), t4 = csub(a2, a3);
      const double2 r1 = make_double2(a0.x + c1 * t1.x + c2 * t2.x, a0.y + c1 * t1.y + c2 * t2.y);
      const double2 r2 = make_double2(a0.x + c2 * t1.x + c1 * t2.x, a0.y + c2 * t1.y + c1 * t2.y);
      const double2 i1 = mul_si<SIGN>(make_double2(s1 * t3.x + s2 * t4.x, s1 * t3.y + s2 * t4.y));
      const double2 i2 = mul_si<SIGN>(make_double2(s2 * t3.x - s1 * t4.x, s2 * t3.y - s1 * t4.y));
      yo[0] = make_double2(a0.x + t1.x + t2.x, a0.y + t1.y + t2.y);
      yo[sout] = cmul(cadd(r1, i1), twid<SIGN>(tw, tstep));
      yo[2 * sout] = cmul(cadd(r2, i2), twid<SIGN>(tw, (2 * tstep) % N));
      yo[3 * sout] = cmul(csub(r2, i2), twid<SIGN>(tw, (3 * tstep) % N));
      yo[4 * sout] = cmul(csub(r1, i1), twid<SIGN>(tw, (4 * tstep) % N));
    } else {
      // generic prime radix: b_j = sum_k a_k w_r^{jk}, w_r^t = W_N^{(N/r) t}
      const int wr = N / r;
      for (int j = 0; j < r; ++j) {
        double2 b = xi[0];
        for (int k = 1; k < r; ++k) b = cadd(b, cmul(xi[k * sin_], twid<SIGN>(tw, wr * ((j * k) % r))));
        yo[j * sout] = cmul(b, twid<SIGN>(tw, (int)(((int64_t)j * tstep) % N)));
      }
    }
  }
}

// All stages; returns the buffer that holds the result (natural order).
template <int SIGN>
__device__ inline double2* stockham_all(double2* x, double2* y, const Axis& ax, int Ls, int M) {
  int n_cur = ax.n, s = 1;
  for (int st = 0; st < ax.nstage; ++st) {
    const int r = ax.radix[st];
    stockham_stage<SIGN>(x, y, ax.n, n_cur, s, r, Ls, M, ax.tw);
    __syncthreads();
    n_cur /= r;
    s *= r;
    double2* t = x; x = y; y = t;
  }
  return x;
}

// ---- FAST and PLANE stages: in place, outputs held in registers across a barrier ------------------------------------------
// How an item index of a stage splits into (butterfly, line): the FAST kernels have a compile-time power of two of lines, the
// plane kernels any number (float reciprocal).
template <int ZCT>
struct FixedLines {
  __device__ explicit FixedLines(int) {}
  __device__ int count() const { return ZCT; }
  __device__ void split(int i, int& bf, int& m) const { m = i & (ZCT - 1); bf = i / ZCT; }
};
struct AnyLines {
  int M;
  float inv_M;
  __device__ explicit AnyLines(int M_) : M(M_), inv_M(1.0f / (float)M_) {}
  __device__ int count() const { return M; }
  __device__ void split(int i, int& bf, int& m) const { bf = fdiv(i, inv_M); m = i - bf * M; }
};

// One stage of radix R over the lines of buf[element * Ls + line] with NT threads, at most KMAX butterflies per thread.
// LEAN: the composite butterflies take their constant twiddles as literals and the last stage (p = 0: every output twiddle
// is 1) skips the twiddle multiply; off in the 1024-thread plane kernels, which sit at 113-115 of their 128 VGPRs.
template <int SIGN, int R, int NT, int KMAX, bool LEAN, class LINES>
__device__ inline void stage(double2* __restrict__ buf, int N, int n_cur, int s, int Ls, int M, const double2* __restrict__ tw,
                             const int tid) {
  const LINES lines(M);
  const int mm = n_cur / R;
  const int total = (N / R) * lines.count();
  const float inv_s = 1.0f / (float)s;
  double2 out[KMAX][R];
#pragma unroll
  for (int u = 0; u < KMAX; ++u) {
    const int i = tid + u * NT;
    if (i < total) {
      int bf, m;
      lines.split(i, bf, m);
      const int p = fdiv(bf, inv_s), q = bf - p * s;
      const double2* xi = buf + (q + s * p) * Ls + m;
      const int sin_ = s * mm * Ls;
      double2 a[R];
#pragma unroll
      for (int k = 0; k < R; ++k) a[k] = xi[k * sin_];
      butterfly_any<SIGN, R, LEAN>(a, out[u], tw, N);
      if (!LEAN || mm > 1) {
        const int tstep = p * s;         // < N
        int t = tstep;
#pragma unroll
        for (int j = 1; j < R; ++j) {
          out[u][j] = cmul(out[u][j], twid<SIGN>(tw, t));
          t += tstep;
          if (t >= N) t -= N;
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < KMAX; ++u) {
    const int i = tid + u * NT;
    if (i < total) {
      int bf, m;
      lines.split(i, bf, m);
      const int p = fdiv(bf, inv_s), q = bf - p * s;
      double2* yo = buf + (q + s * R * p) * Ls + m;
      const int sout = s * Ls;
#pragma unroll
      for (int j = 0; j < R; ++j) yo[j * sout] = out[u][j];
    }
  }
  __syncthreads();
}

// All stages of a runtime axis; PER = the most elements of the buffer a thread may own.
template <int SIGN, int NT, int PER, bool LEAN, class LINES>
__device__ inline void fft(double2* buf, const Axis& ax, int Ls, int M, const double2* tw) {
  int n_cur = ax.n, s = 1;
  for (int st = 0; st < ax.nstage; ++st) {
    const int r = ax.radix[st];
    // (the one dispatch from the runtime radix to the template argument; a switch and not a with_radix(r, lambda): through
    // the lambda the FAST strided kernels came out with other scalar shift instructions than before)
#define ISDF_STAGE(R) \
  case R: stage<SIGN, R, NT, (PER + R - 1) / R, LEAN, LINES>(buf, ax.n, n_cur, s, Ls, M, tw, (int)threadIdx.x); break;
    switch (r) {
      ISDF_STAGE(16) ISDF_STAGE(15) ISDF_STAGE(12) ISDF_STAGE(10) ISDF_STAGE(9) ISDF_STAGE(8) ISDF_STAGE(6) ISDF_STAGE(5)
      ISDF_STAGE(4) ISDF_STAGE(3)
      default: stage<SIGN, 2, NT, (PER + 2 - 1) / 2, LEAN, LINES>(buf, ax.n, n_cur, s, Ls, M, tw, (int)threadIdx.x); break;
    }
#undef ISDF_STAGE
    n_cur /= r;
    s *= r;
  }
}

// ---- the five passes ------------------------------------------------------------------------------------------------
// Each pass exists as a GENERIC kernel (two LDS buffers, runtime tile width, twiddles from global memory) and as a FAST one (one
// buffer, compile-time tile width, twiddles in LDS).  The frames stay apart, and the FAST ones keep their loads, separations and
// merges written out: written once over an engine type, or through stage_twiddles / merge_pair, the FAST instantiations came
// out with their instructions in another order and the five-pass convolution 0.2 - 0.4 % slower.  The GENERIC frames and the
// plane kernels share the helpers above.

// GENERIC tile width: two LDS buffers of n x (L + pad) complex numbers within 64 KB (two workgroups per CU)
int lines_per_tile(int n, int pad) {
  for (int L = 16; L >= 1; L >>= 1)
    if ((size_t)2 * n * (L + pad) * sizeof(double2) <= 64 * 1024) return L;
  return 0;
}

// Pass 1: real lines (n contiguous doubles each, nlines of them back to back) -> half-complex lines (nh = n/2 + 1).
// A workgroup takes LP line pairs.
__global__ __launch_bounds__(TPB) void z_r2c_kernel(const double* __restrict__ in, double2* __restrict__ out, int64_t nlines,
                                                    Axis ax, int LP) {
  extern __shared__ double2 lds[];
  const int n = ax.n, nh = n / 2 + 1, Ls = LP + 1;
  double2* x = lds;
  double2* y = lds + (int64_t)n * Ls;
  const int64_t line0 = (int64_t)blockIdx.x * 2 * LP;
  const int nl = (int)min((int64_t)2 * LP, nlines - line0);     // lines of this tile
  const int M = (nl + 1) / 2;
  const double* src = in + line0 * n;
  for (int c = threadIdx.x; c < 2 * M * n; c += TPB) {
    const int l = c / n, e = c - l * n;
    real_slot(x, Ls, l, e) = (l < nl) ? src[c] : 0.0;
  }
  __syncthreads();
  const double2* z = stockham_all<-1>(x, y, ax, Ls, M);
  double2* dstc = out + line0 * nh;
  for (int c = threadIdx.x; c < nl * nh; c += TPB) {
    const int l = c / nh, k = c - l * nh;
    const int m = l >> 1;
    dstc[c] = separate_pair(z[(int64_t)k * Ls + m], z[(int64_t)((n - k) % n) * Ls + m], l & 1);
  }
}

// Pass 5: half-complex lines -> real lines (unnormalised inverse; the 1/N sits in the kernel table).
__global__ __launch_bounds__(TPB) void z_c2r_kernel(const double2* __restrict__ in, double* __restrict__ out, int64_t nlines,
                                                    Axis ax, int LP) {
  extern __shared__ double2 lds[];
  const int n = ax.n, nh = n / 2 + 1, Ls = LP + 1;
  double2* x = lds;
  double2* y = lds + (int64_t)n * Ls;
  const int64_t line0 = (int64_t)blockIdx.x * 2 * LP;
  const int nl = (int)min((int64_t)2 * LP, nlines - line0);
  const int M = (nl + 1) / 2;
  const double2* src = in + line0 * nh;
  for (int c = threadIdx.x; c < M * nh; c += TPB) {
    const int m = c / nh, k = c - m * nh;
    const double2 a = src[(int64_t)(2 * m) * nh + k];              // A = even line, B = odd line of the pair
    const double2 b = (2 * m + 1 < nl) ? src[(int64_t)(2 * m + 1) * nh + k] : make_double2(0.0, 0.0);
    const bool selfconj = (k == 0) || (2 * k == n);
    double2 z_lo, z_hi;
    merge_pair(a, b, selfconj, &z_lo, &z_hi);
    x[(int64_t)k * Ls + m] = z_lo;
    if (!selfconj) x[(int64_t)(n - k) * Ls + m] = z_hi;
  }
  __syncthreads();
  double2* z = stockham_all<1>(x, y, ax, Ls, M);
  double* dst = out + line0 * n;
  for (int c = threadIdx.x; c < nl * n; c += TPB) {
    const int l = c / n, e = c - l * n;
    dst[c] = real_slot(z, Ls, l, e);
  }
}

// Passes 2-4: 1-D transforms along a strided axis, in place.  data[o * os + e * es + m], e < n (the transformed axis),
// m < Mtot adjacent lines (unit stride), o outer blocks.  MODE 0: forward, 1: inverse, 2: forward, multiply by
// table[e * es + m], inverse.
template <int MODE>
__global__ __launch_bounds__(TPB) void strided_fft_kernel(double2* __restrict__ data, int64_t os, int64_t es, int Mtot, Axis ax,
                                                          int ZC, int ntile, const double* __restrict__ table) {
  extern __shared__ double2 lds[];
  const int n = ax.n;
  double2* x = lds;
  double2* y = lds + (int64_t)n * ZC;
  const int64_t outer = blockIdx.x / ntile;              // 1-D grid: (outer block, tile of adjacent lines)
  const int m0 = (int)(blockIdx.x % ntile) * ZC;
  const int M = min(ZC, Mtot - m0);
  double2* base = data + outer * os + m0;
  for (int c = threadIdx.x; c < n * ZC; c += TPB) {
    const int e = c / ZC, m = c - e * ZC;
    if (m < M) x[c] = base[(int64_t)e * es + m];
  }
  __syncthreads();
  double2* z;
  if (MODE == 1) {
    z = stockham_all<1>(x, y, ax, ZC, M);
  } else {
    z = stockham_all<-1>(x, y, ax, ZC, M);
    if (MODE == 2) {
      const double* tb = table + m0;
      for (int c = threadIdx.x; c < n * ZC; c += TPB) {
        const int e = c / ZC, m = c - e * ZC;
        if (m < M) {
          const double g = tb[(int64_t)e * es + m];
          double2 v = z[c];
          v.x *= g;
          v.y *= g;
          z[c] = v;
        }
      }
      __syncthreads();
      z = stockham_all<1>(z, (z == x) ? y : x, ax, ZC, M);
    }
  }
  for (int c = threadIdx.x; c < n * ZC; c += TPB) {
    const int e = c / ZC, m = c - e * ZC;
    if (m < M) base[(int64_t)e * es + m] = z[c];
  }
}

// FAST.  LDS: [n * Ls complex work buffer][n complex twiddles].  Invariant (host): n * ZCT <= 2048, so a stage has at most 8 / R
// butterflies per thread.  Every one of the ZCT lines is transformed, whatever the tile holds.
template <int SIGN, int ZCT>
__device__ inline void fft_fast(double2* buf, const Axis& ax, int Ls, const double2* tw) {
  fft<SIGN, TPB, 2048 / TPB, true, FixedLines<ZCT>>(buf, ax, Ls, ZCT, tw);
}

template <int ZCT>
__global__ __launch_bounds__(TPB) void z_r2c_fast_kernel(const double* __restrict__ in, double2* __restrict__ out,
                                                         int64_t nlines, Axis ax) {
  extern __shared__ double2 lds[];
  const int n = ax.n, nh = n / 2 + 1;
  constexpr int Ls = ZCT + 1;
  double2* x = lds;
  double2* tw = lds + n * Ls;
  for (int k = threadIdx.x; k < n; k += TPB) tw[k] = ax.tw[k];
  const int64_t line0 = (int64_t)blockIdx.x * 2 * ZCT;
  const int nl = (int)min((int64_t)2 * ZCT, nlines - line0);
  const double* src = in + line0 * n;
  const float inv_n = 1.0f / (float)n;
  for (int c = threadIdx.x; c < 2 * ZCT * n; c += TPB) {
    const int l = (int)(((float)c + 0.5f) * inv_n), e = c - l * n;
    const double v = (l < nl) ? src[c] : 0.0;
    ((double*)(x + e * Ls + (l >> 1)))[l & 1] = v;
  }
  __syncthreads();
  fft_fast<-1, ZCT>(x, ax, Ls, tw);
  double2* dstc = out + line0 * nh;
  const float inv_nh = 1.0f / (float)nh;
  for (int c = threadIdx.x; c < nl * nh; c += TPB) {
    const int l = (int)(((float)c + 0.5f) * inv_nh), k = c - l * nh;
    const int m = l >> 1;
    const double2 zk = x[k * Ls + m];
    const double2 zn = x[(k == 0 ? 0 : n - k) * Ls + m];
    double2 r;
    if ((l & 1) == 0) r = make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y - zn.y));
    else r = make_double2(0.5 * (zk.y + zn.y), -0.5 * (zk.x - zn.x));
    dstc[c] = r;
  }
}

template <int ZCT>
__global__ __launch_bounds__(TPB) void z_c2r_fast_kernel(const double2* __restrict__ in, double* __restrict__ out,
                                                         int64_t nlines, Axis ax) {
  extern __shared__ double2 lds[];
  const int n = ax.n, nh = n / 2 + 1;
  constexpr int Ls = ZCT + 1;
  double2* x = lds;
  double2* tw = lds + n * Ls;
  for (int k = threadIdx.x; k < n; k += TPB) tw[k] = ax.tw[k];
  const int64_t line0 = (int64_t)blockIdx.x * 2 * ZCT;
  const int nl = (int)min((int64_t)2 * ZCT, nlines - line0);
  const int M = (nl + 1) / 2;
  const double2* src = in + line0 * nh;
  const float inv_nh = 1.0f / (float)nh;
  // Z_k = A_k + i B_k (k <= n/2),  Z_{n-k} = conj(A_k) + i conj(B_k);  A = even line, B = odd line of the pair
  for (int c = threadIdx.x; c < M * nh; c += TPB) {
    const int m = (int)(((float)c + 0.5f) * inv_nh), k = c - m * nh;
    double2 a = src[(int64_t)(2 * m) * nh + k];
    double2 b = (2 * m + 1 < nl) ? src[(int64_t)(2 * m + 1) * nh + k] : make_double2(0.0, 0.0);
    const bool selfconj = (k == 0) || (2 * k == n);
    if (selfconj) { a.y = 0.0; b.y = 0.0; }
    x[k * Ls + m] = make_double2(a.x - b.y, a.y + b.x);
    if (!selfconj) x[(n - k) * Ls + m] = make_double2(a.x + b.y, -a.y + b.x);
  }
  __syncthreads();
  fft_fast<1, ZCT>(x, ax, Ls, tw);
  double* dst = out + line0 * n;
  const float inv_n = 1.0f / (float)n;
  for (int c = threadIdx.x; c < nl * n; c += TPB) {
    const int l = (int)(((float)c + 0.5f) * inv_n), e = c - l * n;
    dst[c] = ((const double*)(x + e * Ls + (l >> 1)))[l & 1];
  }
}

template <int MODE, int ZCT>
__global__ __launch_bounds__(TPB) void strided_fft_fast_kernel(double2* __restrict__ data, int64_t os, int64_t es, int Mtot,
                                                               Axis ax, int ntile, const double* __restrict__ table) {
  extern __shared__ double2 lds[];
  const int n = ax.n;
  double2* x = lds;
  double2* tw = lds + n * ZCT;
  for (int k = threadIdx.x; k < n; k += TPB) tw[k] = ax.tw[k];
  // MODE 2 walks tile-major (consecutive workgroups = the same tile of consecutive rows): the kernel-table tile they all
  // multiply with stays in L2 instead of being fetched once per row (3.6 GB of 18.7 GB per 512-row launch in the PMC
  // counters); the plain transforms walk row-major
  const int nouter = gridDim.x / ntile;
  const int64_t outer = (MODE == 2) ? blockIdx.x % nouter : blockIdx.x / ntile;
  const int m0 = (int)((MODE == 2) ? blockIdx.x / nouter : blockIdx.x % ntile) * ZCT;
  const int M = min(ZCT, Mtot - m0);
  double2* base = data + outer * os + m0;
  for (int c = threadIdx.x; c < n * ZCT; c += TPB) {
    const int e = c / ZCT, m = c & (ZCT - 1);
    if (m < M) x[c] = base[(int64_t)e * es + m];
  }
  __syncthreads();
  if (MODE == 1) {
    fft_fast<1, ZCT>(x, ax, ZCT, tw);
  } else {
    fft_fast<-1, ZCT>(x, ax, ZCT, tw);
    if (MODE == 2) {
      const double* tb = table + m0;
      for (int c = threadIdx.x; c < n * ZCT; c += TPB) {
        const int e = c / ZCT, m = c & (ZCT - 1);
        if (m < M) {
          const double g = tb[(int64_t)e * es + m];
          double2 v = x[c];
          v.x *= g;
          v.y *= g;
          x[c] = v;
        }
      }
      __syncthreads();
      fft_fast<1, ZCT>(x, ax, ZCT, tw);
    }
  }
  for (int c = threadIdx.x; c < n * ZCT; c += TPB) {
    const int e = c / ZCT, m = c & (ZCT - 1);
    if (m < M) base[(int64_t)e * es + m] = x[c];
  }
}

// The forward x pass of the packed spectra over a LIST of x-lines, packing as it goes (spectral_rows_lines_own): tile t of a
// row takes the lines lines[ZCT t ... ZCT t + ZCT - 1] (ascending, -1 = no line: the padding of the last tile) into the layout
// x[e * ZCT + m] of the kernel above and runs the same fft_fast<-1, ZCT>: a line's butterflies depend neither on its slot m nor
// on its neighbours, so every value is bit for bit the one strided_fft_fast_kernel<0, ZCT> leaves there.  TPB is a multiple of
// ZCT: a thread keeps one slot m, one line.  Nothing goes back to the lines: slot[t][e][m] (the tile's own layout, so the loads
// coalesce; -1 = not a packed point) names the packed position j of the point e of line m, slot_scale[t][e][m] its scale, and
// the scaled value goes from LDS straight to out[row][j] (spectral_pack_kernel's arithmetic); tile 0 writes the zero padding
// [npts, ldx2) of its row.  The slots are fetched before the transform, the scales after it (133 VGPRs otherwise: 3 waves).
template <int ZCT>
__global__ __launch_bounds__(TPB) void strided_fft_lines_kernel(const double2* __restrict__ data, int64_t os, int64_t es, Axis ax,
                                                                int ntile, const int32_t* __restrict__ lines,
                                                                const int32_t* __restrict__ slot,
                                                                const double* __restrict__ slot_scale, int npts,
                                                                double2* __restrict__ out, int64_t ldx2) {
  static_assert(TPB % ZCT == 0, "one slot per thread");
  constexpr int KS = 2048 / TPB;
  extern __shared__ double2 lds[];
  const int n = ax.n;
  double2* x = lds;
  double2* tw = lds + n * ZCT;
  for (int k = threadIdx.x; k < n; k += TPB) tw[k] = ax.tw[k];
  const int64_t outer = blockIdx.x / ntile;
  const int t = blockIdx.x % ntile;
  const int l = lines[t * ZCT + (threadIdx.x & (ZCT - 1))];
  const double2* base = data + outer * os + l;
  if (l >= 0)
    for (int c = threadIdx.x; c < n * ZCT; c += TPB) x[c] = base[(int64_t)(c / ZCT) * es];
  const int64_t tile0 = (int64_t)t * n * ZCT;
  int js[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    const int c = threadIdx.x + k * TPB;
    js[k] = (c < n * ZCT) ? slot[tile0 + c] : -1;
  }
  __syncthreads();
  fft_fast<-1, ZCT>(x, ax, ZCT, tw);
  double2* o = out + outer * ldx2;
  double sc[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) sc[k] = (js[k] >= 0) ? slot_scale[tile0 + threadIdx.x + k * TPB] : 0.0;
#pragma unroll
  for (int k = 0; k < KS; ++k)
    if (js[k] >= 0) {
      const double2 v = x[threadIdx.x + k * TPB];
      const double s = sc[k];
      o[js[k]] = make_double2(v.x * s, v.y * s);
    }
  if (t == 0)
    for (int64_t j = npts + threadIdx.x; j < ldx2; j += TPB) o[j] = make_double2(0.0, 0.0);
}

// ---- PLANE path: z and y transforms of one (y, z) plane fused in LDS: three passes instead of five ---------------------------
// A workgroup of 1024 threads owns the plane of one (row, x): n1 real lines of n2 points = 115 KB at 120^3, the half-complex plane
// n1 x (n2/2+1) = 117 KB - the whole of it stays in LDS between the z and the y transform, so the pair
//   forward:  real plane -> z real-to-half-complex (two lines per complex transform) -> y forward -> complex plane
//   inverse:  complex plane -> y inverse -> z half-complex-to-real -> real plane
// reads and writes each plane ONCE (48 G bytes per row for the whole convolution with the fused x pass in between, against 80 G
// for the five passes; algorithmic 32 G).  One workgroup per CU; stages as in the FAST path (in place, outputs held in
// registers across a barrier), with any number of lines and 1024 threads.  Layouts: z stage x[z][pair] with the pitch
// chosen = 1 mod 16 (the real-plane load and the separation walk z fastest: a stride of 4 banks), y stage P[y][kz] with pitch
// n2/2+1 = the global layout of the half spectrum.  LDS: [bufsz complex plane][n2 twiddles of z][n1 twiddles of y].
//
// Pipelined form: ONE resident workgroup per CU walks over planes, the NEXT plane's global loads in flight (in registers) while
// the current plane goes through its stages in LDS.  A plane needs 115-117 KB of the CU's 160 KB, so a second workgroup cannot
// overlap its loads with the first one's arithmetic; a plane pass is then load + stages + store in sequence (26 us per 120^2
// plane: about 12 us of memory time at the CU's share of the achievable bandwidth, the rest LDS round trips and butterflies).
// 768 threads (12 waves, 170 VGPRs each) hold the prefetched plane next to the stage registers without spilling - 1024 threads
// have 128 VGPRs and sit at 113-115 already.  Everything about the plane is a compile-time constant (N x N points, two stages of
// radix RA and RB on both axes), so every per-thread array has exactly the size the plane needs.
constexpr int TPBP = 1024;
constexpr int PLANE_ENTRIES = 10240;             // complex numbers: the most a plane buffer may hold (160 KB of LDS)
constexpr int PIPE_NT = 768;                     // threads of the pipelined plane passes (12 waves: 170 VGPRs each)

template <int SIGN, int NT, int N, int RA, int RB, int MMAX>
__device__ __forceinline__ void fft_plane_fixed(double2* buf, int Ls, int M, const double2* tw) {
  static_assert(RA * RB == N, "two stages");
  stage<SIGN, RA, NT, ((N / RA) * MMAX + NT - 1) / NT, true, AnyLines>(buf, N, N, 1, Ls, M, tw, opaque_tid());
  stage<SIGN, RB, NT, ((N / RB) * MMAX + NT - 1) / NT, true, AnyLines>(buf, N, N / RA, RA, Ls, M, tw, opaque_tid());
}

// The dims types of the plane bodies: sizes, thread count, per-thread array sizes (KS_HALF for the n1 x n2h half-complex plane,
// KS_PAIR for its npair x n2h line pairs, KS_FULL for the n1 x n2 complex plane), the thread index of a phase and the transform
// along one axis (FULL: the lines are those of the complex plane).
struct PlaneAny {        // any plane that fits: one workgroup per plane
  static constexpr int NT = TPBP, PER = PLANE_ENTRIES / TPBP;
  static constexpr int KS_HALF = PER, KS_PAIR = PER / 2 + 1, KS_FULL = PER;
  int n1, n2, n2h, npair;
  __device__ PlaneAny(const Axis& az, const Axis& ay) : n1(ay.n), n2(az.n), n2h(az.n / 2 + 1), npair((ay.n + 1) / 2) {}
  __device__ static int tid() { return threadIdx.x; }
  template <int SIGN, bool FULL>
  __device__ __forceinline__ static void transform(double2* buf, const Axis& ax, int Ls, int M, const double2* tw) {
    fft<SIGN, NT, PER, false, AnyLines>(buf, ax, Ls, M, tw);
  }
};
template <int N, int RA, int RB>
struct PlaneSquare {     // N x N with the two stages RA, RB on both axes: the pipelined kernels
  static constexpr int NT = PIPE_NT, n1 = N, n2 = N, n2h = N / 2 + 1, npair = (N + 1) / 2;
  static constexpr int KS_HALF = (n1 * n2h + NT - 1) / NT, KS_PAIR = (npair * n2h + NT - 1) / NT, KS_FULL = (N * N + NT - 1) / NT;
  constexpr PlaneSquare() = default;
  // an opaque copy of the thread index per phase: index arithmetic that depends on it cannot be hoisted out of the plane loop
  // (hoisted, its per-element offsets were what the compiler spilled) and stays in its phase
  __device__ static int tid() { return opaque_tid(); }
  template <int SIGN, bool FULL>
  __device__ __forceinline__ static void transform(double2* buf, const Axis&, int Ls, int M, const double2* tw) {
    fft_plane_fixed<SIGN, NT, N, RA, RB, FULL ? N : N / 2 + 1>(buf, Ls, M, tw);
  }
};

__device__ inline double zero_of(const double*) { return 0.0; }
__device__ inline double2 zero_of(const double2*) { return make_double2(0.0, 0.0); }
// this thread's share of a plane, requested into registers (zero past the end)
template <int NT, int NPRE, class T>
__device__ __forceinline__ void prefetch(T (&pre)[NPRE], const T* __restrict__ src, int count, int tid) {
#pragma unroll
  for (int u = 0; u < NPRE; ++u) {
    const int c = tid + u * NT;
    pre[u] = c < count ? src[c] : zero_of(src);
  }
}

// The bodies.  The kernel owns the source (global memory, or the prefetch registers it refills between the scatter and the
// stages) and the per-thread arrays r / za, zb, which it hands in: declared inside a body their lifetimes end with the inlined
// call and the register allocation of the pipelined kernels moves (96^2 forward: 131 VGPRs against 128).  The bodies are forced
// inline: as calls they would keep those arrays and the stage outputs out of registers.
// forward, after the real plane went into x[z][pair]: z stages, separation of the line pairs and re-lay as P[y][k], y stages, store
template <class D>
__device__ __forceinline__ void plane_fwd_body(const D d, double2* lds, int Lz, int bufsz, const Axis& az, const Axis& ay,
                                               double2* __restrict__ dst, double2 (&r)[D::KS_HALF]) {
  double2* x = lds;
  const double2* twz = lds + bufsz;
  const double2* twy = twz + d.n2;
  d.template transform<-1, false>(x, az, Lz, d.npair, twz);
  int tid = D::tid();
  const float inv_nh = 1.0f / (float)d.n2h;
#pragma unroll
  for (int u = 0; u < D::KS_HALF; ++u) {
    const int c = tid + u * D::NT;
    if (c < d.n1 * d.n2h) {
      const int l = fdiv(c, inv_nh), k = c - l * d.n2h;
      const int m = l >> 1;
      r[u] = separate_pair(x[k * Lz + m], x[(k == 0 ? 0 : d.n2 - k) * Lz + m], l & 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < D::KS_HALF; ++u) {
    const int c = tid + u * D::NT;
    if (c < d.n1 * d.n2h) x[c] = r[u];
  }
  __syncthreads();
  d.template transform<-1, false>(x, ay, d.n2h, d.n2h, twy);
  tid = D::tid();
  for (int c = tid; c < d.n1 * d.n2h; c += D::NT) dst[c] = x[c];
}

// inverse, after the half-complex plane went into P[y][k]: y stages, pairs of lines back into one complex line each, z stages,
// store of the real plane
template <class D>
__device__ __forceinline__ void plane_inv_body(const D d, double2* lds, int Lz, int bufsz, const Axis& az, const Axis& ay,
                                               double* __restrict__ dst, double2 (&za)[D::KS_PAIR], double2 (&zb)[D::KS_PAIR]) {
  double2* x = lds;
  const double2* twz = lds + bufsz;
  const double2* twy = twz + d.n2;
  d.template transform<1, false>(x, ay, d.n2h, d.n2h, twy);
  int tid = D::tid();
  const float inv_nh = 1.0f / (float)d.n2h, inv_n2 = 1.0f / (float)d.n2;
#pragma unroll
  for (int u = 0; u < D::KS_PAIR; ++u) {
    const int c = tid + u * D::NT;
    if (c < d.npair * d.n2h) {
      const int m = fdiv(c, inv_nh), k = c - m * d.n2h;
      const double2 a = x[(2 * m) * d.n2h + k];
      const double2 b = (2 * m + 1 < d.n1) ? x[(2 * m + 1) * d.n2h + k] : make_double2(0.0, 0.0);
      merge_pair(a, b, k == 0 || 2 * k == d.n2, &za[u], &zb[u]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < D::KS_PAIR; ++u) {
    const int c = tid + u * D::NT;
    if (c < d.npair * d.n2h) {
      const int m = fdiv(c, inv_nh), k = c - m * d.n2h;
      x[k * Lz + m] = za[u];
      if (!(k == 0 || 2 * k == d.n2)) x[(d.n2 - k) * Lz + m] = zb[u];
    }
  }
  __syncthreads();
  d.template transform<1, false>(x, az, Lz, d.npair, twz);
  tid = D::tid();
  for (int c = tid; c < d.n1 * d.n2; c += D::NT) {
    const int l = fdiv(c, inv_n2), e = c - l * d.n2;
    dst[c] = real_slot(x, Lz, l, e);
  }
}

// forward: in = real planes (n1 x n2 each, back to back), out = half-complex planes (n1 x n2h), y already transformed
__global__ __launch_bounds__(TPBP) void plane_fwd_kernel(const double* __restrict__ in, double2* __restrict__ out, Axis az, Axis ay,
                                                         int Lz, int bufsz) {
  extern __shared__ double2 lds[];
  const PlaneAny d(az, ay);
  double2* x = lds;
  stage_twiddles(lds + bufsz, az, d.n2, TPBP);
  stage_twiddles(lds + bufsz + d.n2, ay, d.n1, TPBP);
  const double* src = in + (int64_t)blockIdx.x * d.n1 * d.n2;
  if (d.n1 & 1)                                         // the last line has no partner: its imaginary slot is zero
    for (int e = threadIdx.x; e < d.n2; e += TPBP) x[e * Lz + d.npair - 1].y = 0.0;
  const float inv_n2 = 1.0f / (float)d.n2;
  for (int c = threadIdx.x; c < d.n1 * d.n2; c += TPBP) {
    const int l = fdiv(c, inv_n2), e = c - l * d.n2;
    real_slot(x, Lz, l, e) = src[c];
  }
  __syncthreads();
  double2 r[PlaneAny::KS_HALF];
  plane_fwd_body(d, lds, Lz, bufsz, az, ay, out + (int64_t)blockIdx.x * d.n1 * d.n2h, r);
}

// inverse: in = half-complex planes, out = real planes (unnormalised: the 1/N sits in the kernel table)
__global__ __launch_bounds__(TPBP) void plane_inv_kernel(const double2* __restrict__ in, double* __restrict__ out, Axis az, Axis ay,
                                                         int Lz, int bufsz) {
  extern __shared__ double2 lds[];
  const PlaneAny d(az, ay);
  double2* x = lds;
  stage_twiddles(lds + bufsz, az, d.n2, TPBP);
  stage_twiddles(lds + bufsz + d.n2, ay, d.n1, TPBP);
  const double2* src = in + (int64_t)blockIdx.x * d.n1 * d.n2h;
  for (int c = threadIdx.x; c < d.n1 * d.n2h; c += TPBP) x[c] = src[c];
  __syncthreads();
  double2 za[PlaneAny::KS_PAIR], zb[PlaneAny::KS_PAIR];
  plane_inv_body(d, lds, Lz, bufsz, az, ay, out + (int64_t)blockIdx.x * d.n1 * d.n2, za, zb);
}

template <class D>
__global__ __launch_bounds__(D::NT) void plane_fwd_pipe_kernel(const double* __restrict__ in, double2* __restrict__ out, Axis az,
                                                               Axis ay, int Lz, int bufsz, int nplanes) {
  extern __shared__ double2 lds[];
  constexpr D d{};
  constexpr int NT = D::NT, nreal = d.n1 * d.n2;
  double2* x = lds;
  stage_twiddles(lds + bufsz, az, d.n2, NT);
  stage_twiddles(lds + bufsz + d.n2, ay, d.n1, NT);
  const float inv_n2 = 1.0f / (float)d.n2;
  double pre[(nreal + NT - 1) / NT];
  int pl = blockIdx.x;
  if (pl < nplanes) prefetch<NT>(pre, in + (int64_t)pl * nreal, nreal, (int)threadIdx.x);
  for (; pl < nplanes; pl += gridDim.x) {
    int tid = D::tid();
    if (d.n1 & 1)                                         // the last line has no partner: its imaginary slot is zero
      for (int e = tid; e < d.n2; e += NT) x[e * Lz + d.npair - 1].y = 0.0;
#pragma unroll
    for (int u = 0; u < (nreal + NT - 1) / NT; ++u) {
      const int c = tid + u * NT;
      if (c < nreal) {
        const int l = fdiv(c, inv_n2), e = c - l * d.n2;
        real_slot(x, Lz, l, e) = pre[u];
      }
    }
    __syncthreads();
    tid = D::tid();
    const int nxt = pl + (int)gridDim.x;                  // requested now, consumed at the top of the next round
    if (nxt < nplanes) prefetch<NT>(pre, in + (int64_t)nxt * nreal, nreal, tid);
    double2 r[D::KS_HALF];
    plane_fwd_body(d, lds, Lz, bufsz, az, ay, out + (int64_t)pl * d.n1 * d.n2h, r);
    __syncthreads();                                      // the next round overwrites the buffer
  }
}

template <class D>
__global__ __launch_bounds__(D::NT) void plane_inv_pipe_kernel(const double2* __restrict__ in, double* __restrict__ out, Axis az,
                                                               Axis ay, int Lz, int bufsz, int nplanes) {
  extern __shared__ double2 lds[];
  constexpr D d{};
  constexpr int NT = D::NT, ncplx = d.n1 * d.n2h;
  double2* x = lds;
  stage_twiddles(lds + bufsz, az, d.n2, NT);
  stage_twiddles(lds + bufsz + d.n2, ay, d.n1, NT);
  double2 pre[(ncplx + NT - 1) / NT];
  int pl = blockIdx.x;
  if (pl < nplanes) prefetch<NT>(pre, in + (int64_t)pl * ncplx, ncplx, (int)threadIdx.x);
  for (; pl < nplanes; pl += gridDim.x) {
    int tid = D::tid();
#pragma unroll
    for (int u = 0; u < (ncplx + NT - 1) / NT; ++u) {
      const int c = tid + u * NT;
      if (c < ncplx) x[c] = pre[u];
    }
    __syncthreads();
    tid = D::tid();
    const int nxt = pl + (int)gridDim.x;
    if (nxt < nplanes) prefetch<NT>(pre, in + (int64_t)nxt * ncplx, ncplx, tid);
    double2 za[D::KS_PAIR], zb[D::KS_PAIR];
    plane_inv_body(d, lds, Lz, bufsz, az, ay, out + (int64_t)pl * d.n1 * d.n2, za, zb);
    __syncthreads();
  }
}

// ---- k-point form: real rows in, COMPLEX rows out (the kernel table of q != 0 is not inversion symmetric, so the product
// spectrum is not Hermitian).  Forward = the real-input half spectrum of the plane path + an x pass; then the half spectrum is
// expanded to the full one under the table multiply; inverse = x pass + one fused (y, z) complex plane pass writing Re and Im.
// full[b][kx][ky][kz] = tab[kx][ky][kz] * scale * F(kx, ky, kz),  F = half[...] for kz <= n2/2, conj(half[-kx, -ky, n2 - kz]) above
__global__ void expand_mul_kernel(const double2* __restrict__ half, double2* __restrict__ full, const double* __restrict__ tab,
                                  int n0, int n1, int n2, double scale) {
  const int n2h = n2 / 2 + 1;
  const int64_t G = (int64_t)n0 * n1 * n2, gc = (int64_t)n0 * n1 * n2h;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= G) return;
  const int kz = (int)(idx % n2), ky = (int)((idx / n2) % n1), kx = (int)(idx / ((int64_t)n2 * n1));
  const double2* hb = half + (int64_t)blockIdx.y * gc;
  double2 v;
  if (kz < n2h) {
    v = hb[((int64_t)kx * n1 + ky) * n2h + kz];
  } else {
    const int mx = kx ? n0 - kx : 0, my = ky ? n1 - ky : 0;
    v = hb[((int64_t)mx * n1 + my) * n2h + (n2 - kz)];
    v.y = -v.y;
  }
  const double c = tab[idx] * scale;
  full[(int64_t)blockIdx.y * G + idx] = make_double2(c * v.x, c * v.y);
}

// inverse y and z transforms of one complex (y, z) plane P[y][z] (pitch n2) in LDS, Re and Im written to separate real arrays
template <class D>
__device__ __forceinline__ void plane_c2c_inv_body(const D d, double2* lds, int Lz, int bufsz, const Axis& az, const Axis& ay,
                                                   double* __restrict__ out_re, double* __restrict__ out_im, int64_t off,
                                                   double2 (&r)[D::KS_FULL]) {
  double2* x = lds;
  const double2* twz = lds + bufsz;
  const double2* twy = twz + d.n2;
  d.template transform<1, true>(x, ay, d.n2, d.n2, twy);                       // along y: element y, line z
  // transpose to X[z][y] (pitch Lz) through registers so that z becomes the element index
  int tid = D::tid();
  const float inv_n2 = 1.0f / (float)d.n2;
#pragma unroll
  for (int u = 0; u < D::KS_FULL; ++u) {
    const int c = tid + u * D::NT;
    const double2 v = x[c < d.n1 * d.n2 ? c : 0];
    r[u] = make_double2(v.x, v.y);                      // (component-wise: the struct copy kept the whole array in scratch)
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < D::KS_FULL; ++u) {
    const int c = tid + u * D::NT;
    if (c < d.n1 * d.n2) {
      const int y = fdiv(c, inv_n2), z = c - y * d.n2;
      x[z * Lz + y] = r[u];
    }
  }
  __syncthreads();
  d.template transform<1, true>(x, az, Lz, d.n1, twz);                         // along z: element z, line y
  tid = D::tid();
  for (int c = tid; c < d.n1 * d.n2; c += D::NT) {
    const int y = fdiv(c, inv_n2), z = c - y * d.n2;
    const double2 v = x[z * Lz + y];
    out_re[off + c] = v.x;
    out_im[off + c] = v.y;
  }
}

__global__ __launch_bounds__(TPBP) void plane_c2c_inv_kernel(const double2* __restrict__ in, double* __restrict__ out_re,
                                                             double* __restrict__ out_im, Axis az, Axis ay, int Lz, int bufsz) {
  extern __shared__ double2 lds[];
  const PlaneAny d(az, ay);
  double2* x = lds;
  stage_twiddles(lds + bufsz, az, d.n2, TPBP);
  stage_twiddles(lds + bufsz + d.n2, ay, d.n1, TPBP);
  const int64_t off = (int64_t)blockIdx.x * d.n1 * d.n2;
  const double2* src = in + off;
  for (int c = threadIdx.x; c < d.n1 * d.n2; c += TPBP) x[c] = src[c];
  __syncthreads();
  double2 r[PlaneAny::KS_FULL];
  plane_c2c_inv_body(d, lds, Lz, bufsz, az, ay, out_re, out_im, off, r);
}

// the same pass as a persistent workgroup with the next plane's loads in flight
template <class D>
__global__ __launch_bounds__(D::NT) void plane_c2c_inv_pipe_kernel(const double2* __restrict__ in, double* __restrict__ out_re,
                                                                   double* __restrict__ out_im, Axis az, Axis ay, int Lz, int bufsz,
                                                                   int nplanes) {
  extern __shared__ double2 lds[];
  constexpr D d{};
  constexpr int NT = D::NT, nent = d.n1 * d.n2;
  double2* x = lds;
  stage_twiddles(lds + bufsz, az, d.n2, NT);
  stage_twiddles(lds + bufsz + d.n2, ay, d.n1, NT);
  double2 pre[D::KS_FULL];
  int pl = blockIdx.x;
  if (pl < nplanes) prefetch<NT>(pre, in + (int64_t)pl * nent, nent, (int)threadIdx.x);
  for (; pl < nplanes; pl += gridDim.x) {
    int tid = D::tid();
#pragma unroll
    for (int u = 0; u < D::KS_FULL; ++u) {
      const int c = tid + u * NT;
      if (c < nent) x[c] = pre[u];
    }
    __syncthreads();
    tid = D::tid();
    const int nxt = pl + (int)gridDim.x;
    if (nxt < nplanes) prefetch<NT>(pre, in + (int64_t)nxt * nent, nent, tid);
    const int64_t off = (int64_t)pl * nent;
    double2 r[D::KS_FULL];
    plane_c2c_inv_body(d, lds, Lz, bufsz, az, ay, out_re, out_im, off, r);
    __syncthreads();
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
constexpr int LDS_MAX = 160 * 1024;

// Geometry of a plane pass: pitch of the z stage (= 1 mod 16), complex entries of the plane buffer and LDS bytes (buffer + both
// twiddle tables); bytes = 0 when the plane does not fit.  complex_plane: the n1 x n2 plane of the k-point form's inverse,
// else the real n1 x n2 plane / its n1 x (n2/2+1) half spectrum.
struct PlaneGeo {
  int Lz, bufsz;
  size_t bytes;
};
PlaneGeo plane_geometry(int n1, int n2, bool complex_plane) {
  const int n2h = n2 / 2 + 1, npair = (n1 + 1) / 2;
  const bool fits = complex_plane ? n1 * n2 <= PLANE_ENTRIES
                                  : std::max(n2 * npair, n1 * n2h) <= PLANE_ENTRIES && n1 * n2 <= 2 * PLANE_ENTRIES;
  int Lz = complex_plane ? n1 : npair;                   // lines of the z stage
  while (Lz % 16 != 1) ++Lz;
  const int bufsz = std::max(n2 * Lz, n1 * (complex_plane ? n2 : n2h));
  const size_t bytes = sizeof(double2) * ((size_t)bufsz + n1 + n2);
  if (!fits || bytes > LDS_MAX) return {0, 0, 0};
  return {Lz, bufsz, bytes};
}

template <class F>
void with_lines(int L, F f) {       // run f with the tile width as a compile-time constant
  switch (L) {
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 1>{}); break;
  }
}

bool smooth235(const Axis& ax) {          // every stage radix is one the register butterflies know (2-3-5 smooth length)
  for (int i = 0; i < ax.nstage; ++i) {
    const int r = ax.radix[i];
    if (r == 7 || r == 11 || r == 13) return false;
  }
  return true;
}
int fast_lines(int n) {          // largest power of two <= 16 with n * lines <= 2048
  for (int L = 16; L >= 1; L >>= 1)
    if (n * L <= 2048) return L;
  return 0;
}

bool factorise(int n, Axis* ax) {
  ax->n = n;
  ax->nstage = 0;
  // 2-3-5 smooth lengths (the FAST and PLANE paths): as few stages as the in-register radices up to 16 allow, the split with
  // the smallest largest radix among the shortest ones (120 = 12 x 10, 108 = 12 x 9, 128 = 16 x 8, 96 = 12 x 8)
  int m = n;
  for (int p : {2, 3, 5})
    while (m % p == 0) m /= p;
  if (m == 1 && n > 1) {
    static const int big[] = {16, 15, 12, 10, 9, 8, 6, 5, 4, 3, 2};
    int best[MAXSTAGE], nbest = MAXSTAGE + 1, bestmax = 1 << 30;
    int cur[MAXSTAGE];
    // depth-first over non-increasing radix sequences (tiny search: n <= 1024)
    struct Rec {
      static void go(int rest, int maxr, int depth, int* cur, int* best, int& nbest, int& bestmax) {
        if (rest == 1) {
          const int mx = depth ? cur[0] : 1;
          if (depth < nbest || (depth == nbest && mx < bestmax)) {
            nbest = depth; bestmax = mx;
            for (int i = 0; i < depth; ++i) best[i] = cur[i];
          }
          return;
        }
        if (depth + 1 > nbest || depth >= MAXSTAGE) return;
        for (int r : big)
          if (r <= maxr && rest % r == 0) { cur[depth] = r; go(rest / r, r, depth + 1, cur, best, nbest, bestmax); }
      }
    };
    Rec::go(n, 16, 0, cur, best, nbest, bestmax);
    if (nbest <= MAXSTAGE) {
      ax->nstage = nbest;
      for (int i = 0; i < nbest; ++i) ax->radix[i] = best[i];
      return true;
    }
  }
  // every other length (and n = 1): 4, 2, 3, 5, then the primes of the O(r^2) butterfly
  const int order[4] = {4, 2, 3, 5};
  for (int r : order)
    while (n % r == 0 && n > 1) {
      if (ax->nstage >= MAXSTAGE) return false;
      ax->radix[ax->nstage++] = r;
      n /= r;
    }
  for (int p = 7; n > 1 && p <= 13; p += 2)
    while (n % p == 0) {
      if (ax->nstage >= MAXSTAGE) return false;
      ax->radix[ax->nstage++] = p;
      n /= p;
    }
  return n == 1;
}

// The three axes of a mesh: factorisation and the twiddle table exp(-2 pi i k / n) (workspace "fft_tw_<n>", uploaded once).
int make_axes(isdf_handle h, const int32_t mesh[3], Axis ax[3], const char* who) {
  for (int d = 0; d < 3; ++d) {
    if (!factorise(mesh[d], &ax[d])) return isdf_fail(h, ISDF_ERR_ARG, "%s: unsupported mesh dimension %d", who, mesh[d]);
    char name[32];
    snprintf(name, sizeof(name), "fft_tw_%d", mesh[d]);
    const bool fresh = h->ws.find(name) == h->ws.end();
    double2* tw = (double2*)isdf_ws(h, name, sizeof(double2) * (size_t)mesh[d]);
    if (!tw) return ISDF_ERR_HIP;
    if (fresh) {
      std::vector<double2> host(mesh[d]);
      for (int k = 0; k < mesh[d]; ++k) {
        const double t = -2.0 * 3.14159265358979323846 * (double)k / (double)mesh[d];
        host[k] = make_double2(cos(t), sin(t));
      }
      HIP_TRY(h, hipMemcpyAsync(tw, host.data(), sizeof(double2) * (size_t)mesh[d], hipMemcpyHostToDevice, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    ax[d].tw = tw;
  }
  return ISDF_OK;
}

// ---- launches of the five-pass kernels ------------------------------------------------------------------------------------
// L = lines (on z: line pairs) per workgroup: a template argument of the FAST kernels, an argument of the GENERIC ones, and in
// both what sizes the grid and the LDS here.
// pass 1 (FWD: real lines in, half-complex lines out) or pass 5 over nlines lines
template <bool FWD, class IN, class OUT>
void launch_z(isdf_handle h, bool fast, int L, const IN* in, OUT* out, int64_t nlines, const Axis& ax) {
  const dim3 grid((unsigned)cdiv(nlines, 2 * L));
  const size_t n = ax.n;
  if (fast) {
    const size_t lds = sizeof(double2) * (n * (L + 1) + n);
    with_lines(L, [&](auto z) {
      constexpr int ZCT = decltype(z)::value;
      if constexpr (FWD) z_r2c_fast_kernel<ZCT><<<grid, dim3(TPB), lds, h->stream>>>(in, out, nlines, ax);
      else z_c2r_fast_kernel<ZCT><<<grid, dim3(TPB), lds, h->stream>>>(in, out, nlines, ax);
    });
  } else {
    const size_t lds = sizeof(double2) * 2 * n * (L + 1);
    if constexpr (FWD) z_r2c_kernel<<<grid, dim3(TPB), lds, h->stream>>>(in, out, nlines, ax, L);
    else z_c2r_kernel<<<grid, dim3(TPB), lds, h->stream>>>(in, out, nlines, ax, L);
  }
}

// passes 2-4 over nouter blocks of Mtot adjacent lines each
template <int MODE>
void launch_strided(isdf_handle h, bool fast, int L, double2* data, int64_t nouter, int64_t os, int64_t es, int Mtot, const Axis& ax,
                    const double* table) {
  const int nt = (int)cdiv(Mtot, L);
  const dim3 grid((unsigned)(nouter * nt));
  const size_t n = ax.n;
  if (fast)
    with_lines(L, [&](auto z) {
      strided_fft_fast_kernel<MODE, decltype(z)::value><<<grid, dim3(TPB), sizeof(double2) * (n * L + n), h->stream>>>(
          data, os, es, Mtot, ax, nt, table);
    });
  else
    strided_fft_kernel<MODE><<<grid, dim3(TPB), sizeof(double2) * 2 * n * L, h->stream>>>(data, os, es, Mtot, ax, L, nt, table);
}

// ---- launches of the plane passes ---------------------------------------------------------------------------------------
// The square planes that have pipelined kernels, with the two radices factorise() picks for them.  Two oddities of who uses
// which, kept as they are: spectral_rows_own pipes its forward pass at all seven sizes; the k-point form pipes both of its
// plane passes or neither and only up to PIPE_Q_MAX (above, the complex plane's prefetch does not fit the registers), so at
// 100^2 its forward pass would be the one-workgroup-per-plane kernel although the plain convolution pipes 100^2.  (Today the
// bound is not reached: plane_geometry() declines the complex 100 x 100 plane, so the k-point form leaves 100^2 to hipFFT.)
#define ISDF_PLANE_SIZES(X) X(64, 8, 8) X(72, 9, 8) X(80, 10, 8) X(96, 12, 8) X(100, 10, 10) X(108, 12, 9) X(120, 12, 10)
constexpr int PIPE_ANY = 1024, PIPE_Q_MAX = 96;

// runs f(PlaneSquare<N, RA, RB>{}) and returns true when this plane, not above nmax, is to take a pipelined kernel
template <class F>
bool with_pipe_size(isdf_handle h, const Axis& az, const Axis& ay, int nmax, F f) {
  if (h->conv_pipe == 0 || ay.n != az.n || ay.n > nmax || ay.nstage != 2) return false;
#define ISDF_PLANE_SIZE(NN, RA, RB)                                \
  if (ay.n == NN && ay.radix[0] == RA && ay.radix[1] == RB) {      \
    f(PlaneSquare<NN, RA, RB>{});                                  \
    return true;                                                   \
  }
  ISDF_PLANE_SIZES(ISDF_PLANE_SIZE)
#undef ISDF_PLANE_SIZE
  return false;
}

// (set on every call: the attribute is per device, a process-wide flag would skip a second device)
template <class K>
int raise_lds(isdf_handle h, K kernel) {
  HIP_TRY(h, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
  return ISDF_OK;
}
dim3 pipe_grid(isdf_handle h, int nplanes) { return dim3((unsigned)std::min<int64_t>(nplanes, h->num_cu)); }

// ax: the three axes of the mesh (the plane is (y, z) = ax[1], ax[2]); nplanes = rows x n0; pipe_max: see ISDF_PLANE_SIZES
int launch_plane_fwd(isdf_handle h, const double* in, double2* out, const Axis* ax, const PlaneGeo& g, int nplanes, int pipe_max) {
  int rc = ISDF_OK;
  const bool piped = with_pipe_size(h, ax[2], ax[1], pipe_max, [&](auto d) {
    auto kernel = plane_fwd_pipe_kernel<decltype(d)>;
    if ((rc = raise_lds(h, kernel)) == ISDF_OK)
      kernel<<<pipe_grid(h, nplanes), dim3(PIPE_NT), g.bytes, h->stream>>>(in, out, ax[2], ax[1], g.Lz, g.bufsz, nplanes);
  });
  if (!piped && (rc = raise_lds(h, plane_fwd_kernel)) == ISDF_OK)
    plane_fwd_kernel<<<dim3((unsigned)nplanes), dim3(TPBP), g.bytes, h->stream>>>(in, out, ax[2], ax[1], g.Lz, g.bufsz);
  return rc;
}

int launch_plane_inv(isdf_handle h, const double2* in, double* out, const Axis* ax, const PlaneGeo& g, int nplanes, int pipe_max) {
  int rc = ISDF_OK;
  const bool piped = with_pipe_size(h, ax[2], ax[1], pipe_max, [&](auto d) {
    auto kernel = plane_inv_pipe_kernel<decltype(d)>;
    if ((rc = raise_lds(h, kernel)) == ISDF_OK)
      kernel<<<pipe_grid(h, nplanes), dim3(PIPE_NT), g.bytes, h->stream>>>(in, out, ax[2], ax[1], g.Lz, g.bufsz, nplanes);
  });
  if (!piped && (rc = raise_lds(h, plane_inv_kernel)) == ISDF_OK)
    plane_inv_kernel<<<dim3((unsigned)nplanes), dim3(TPBP), g.bytes, h->stream>>>(in, out, ax[2], ax[1], g.Lz, g.bufsz);
  return rc;
}

int launch_plane_c2c_inv(isdf_handle h, const double2* in, double* out_re, double* out_im, const Axis* ax, const PlaneGeo& g,
                         int nplanes) {
  int rc = ISDF_OK;
  const bool piped = with_pipe_size(h, ax[2], ax[1], PIPE_Q_MAX, [&](auto d) {
    if constexpr (decltype(d)::n1 <= PIPE_Q_MAX) {
      auto kernel = plane_c2c_inv_pipe_kernel<decltype(d)>;
      if ((rc = raise_lds(h, kernel)) == ISDF_OK)
        kernel<<<pipe_grid(h, nplanes), dim3(PIPE_NT), g.bytes, h->stream>>>(in, out_re, out_im, ax[2], ax[1], g.Lz, g.bufsz, nplanes);
    } else {      // not instantiated above the bound; with_pipe_size() was given the same bound, so this is not reached
      rc = isdf_fail(h, ISDF_ERR_ARG, "launch_plane_c2c_inv: no pipelined kernel for %d^2", (int)decltype(d)::n1);
    }
  });
  if (!piped && (rc = raise_lds(h, plane_c2c_inv_kernel)) == ISDF_OK)
    plane_c2c_inv_kernel<<<dim3((unsigned)nplanes), dim3(TPBP), g.bytes, h->stream>>>(in, out_re, out_im, ax[2], ax[1], g.Lz, g.bufsz);
  return rc;
}

}  // namespace

// Whether conv_rows_own can take this mesh and this many rows at once (the batch-dependent launch limits it checks itself:
// callers fall back to hipFFT instead of failing).
bool conv_rows_own_supported(const int32_t mesh[3], int nb) {
  if (nb < 1 || (int64_t)nb * mesh[0] * mesh[1] * 4 >= 2147483647LL || (int64_t)nb * mesh[1] * (mesh[2] / 2 + 1) >= 2147483647LL)
    return false;
  for (int d = 0; d < 3; ++d) {
    Axis ax;
    if (mesh[d] < 1 || mesh[d] > 1024 || !factorise(mesh[d], &ax)) return false;
    if (lines_per_tile(mesh[d], d == 2 ? 1 : 0) < 1) return false;
  }
  return true;
}

// d_out (nb rows of G reals) = ifft(cg * fft(d_in rows)) with cg the scaled half-spectrum table of coulomb.hip
// (n0, n1, n2/2+1); zbuf: nb * gc complex scratch.  In place (d_out == d_in) allowed.
int conv_rows_own(isdf_handle h, const double* d_in, double* d_out, int nb, const int32_t mesh[3], const double* cg,
                  double2* zbuf) {
  const int n0 = mesh[0], n1 = mesh[1], n2 = mesh[2], n2h = n2 / 2 + 1;
  Axis ax[3];
  if (int rc = make_axes(h, mesh, ax, "conv_rows_own")) return rc;
  const int64_t gc = (int64_t)n0 * n1 * n2h;
  const int64_t nlines = (int64_t)nb * n0 * n1;
  ARG_CHECK(h, nlines * 4 < 2147483647LL && (int64_t)nb * cdiv((int64_t)n1 * n2h, 1) < 2147483647LL);
  const int LP = lines_per_tile(n2, 1);
  const int ZY = lines_per_tile(n1, 0), ZX = lines_per_tile(n0, 0);
  if (LP < 1 || ZY < 1 || ZX < 1) return isdf_fail(h, ISDF_ERR_ARG, "conv_rows_own: mesh too large for the LDS tiles");
  const int64_t G = (int64_t)n0 * n1 * n2;
  const int FZ = fast_lines(n2), FY = fast_lines(n1), FX = fast_lines(n0);
  const bool smooth = smooth235(ax[0]) && smooth235(ax[1]) && smooth235(ax[2]);
  const PlaneGeo geo = (h->own_fft == 2 && smooth && FX >= 1) ? plane_geometry(n1, n2, false) : PlaneGeo{0, 0, 0};
  ProfScope ps(h, geo.bytes ? "coulomb_conv_own_3pass[byte]" : "coulomb_conv_own_5pass[byte]", 32.0 * (double)G * nb,
               geo.bytes ? 3 : 5);
  if (geo.bytes) {
    // PLANE path: (z, y) forward per plane, x forward . table . x inverse, (y, z) inverse per plane
    // Sub-batches sized so that the half spectra of a sub-batch stay in the 256 MB Infinity Cache between the three passes
    // (option "conv_sub_rows": rows per sub-batch; 0 = the whole batch at once, the round-2 behaviour): the middle pass then
    // reads and writes cache-resident lines and the inverse plane pass reads them back from there - HBM sees the real rows in
    // and out only.  Every sub-batch still launches >= 256 workgroups (rows x n0 planes).
    const int sub = h->conv_sub_rows > 0 ? std::min(nb, h->conv_sub_rows) : nb;
    for (int r0 = 0; r0 < nb; r0 += sub) {
      const int nr = std::min(sub, nb - r0);
      double2* zb = zbuf + (int64_t)r0 * gc;
      const int nplanes = (int)((int64_t)nr * n0);
      if (int rc = launch_plane_fwd(h, d_in + (int64_t)r0 * G, zb, ax, geo, nplanes, PIPE_ANY)) return rc;
      launch_strided<2>(h, true, FX, zb, nr, gc, (int64_t)n1 * n2h, n1 * n2h, ax[0], cg);
      if (int rc = launch_plane_inv(h, zb, d_out + (int64_t)r0 * G, ax, geo, nplanes, PIPE_ANY)) return rc;
    }
    KERNEL_CHECK(h);
    return ISDF_OK;
  }
  // five passes: FAST, or GENERIC (a factor 7, 11 or 13 somewhere)
  const bool fast = smooth && FZ >= 1 && FY >= 1 && FX >= 1;
  const int Lz = fast ? FZ : LP, Ly = fast ? FY : ZY, Lx = fast ? FX : ZX;
  launch_z<true>(h, fast, Lz, d_in, zbuf, nlines, ax[2]);
  launch_strided<0>(h, fast, Ly, zbuf, (int64_t)nb * n0, (int64_t)n1 * n2h, (int64_t)n2h, n2h, ax[1], nullptr);
  launch_strided<2>(h, fast, Lx, zbuf, nb, gc, (int64_t)n1 * n2h, n1 * n2h, ax[0], cg);
  launch_strided<1>(h, fast, Ly, zbuf, (int64_t)nb * n0, (int64_t)n1 * n2h, (int64_t)n2h, n2h, ax[1], nullptr);
  launch_z<false>(h, fast, Lz, zbuf, d_out, nlines, ax[2]);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

// ---- spectral rows: X[r][2j], X[r][2j+1] = scale[j] * (Re, Im) fft(rows[r])[idx[j]] over a list of half-spectrum points.
// With scale^2 = multiplicity * w * coulG / G on the points inside a sphere, W = w conv(rows) rows^T = X X^T: the convolution's
// inverse transform and half of the P^2 G product's K dimension are never computed ("spectral W").
__global__ void spectral_pack_kernel(const double2* __restrict__ z, int64_t gc, const int32_t* __restrict__ idx,
                                     const double* __restrict__ scale, int npts, double2* __restrict__ out, int64_t ldx2) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ldx2) return;
  const int row = blockIdx.y;
  double2 v = make_double2(0.0, 0.0);                    // padding up to the leading dimension is zero
  if (j < npts) {
    const double2 t = z[(int64_t)row * gc + idx[j]];
    const double s = scale[j];
    v = make_double2(t.x * s, t.y * s);
  }
  out[(int64_t)row * ldx2 + j] = v;
}

bool spectral_rows_own_supported(isdf_handle h, const int32_t mesh[3], int nb) {
  if (h->own_fft != 2 || !conv_rows_own_supported(mesh, nb)) return false;
  Axis ax[3];
  for (int d = 0; d < 3; ++d)
    if (!factorise(mesh[d], &ax[d]) || !smooth235(ax[d])) return false;
  return fast_lines(mesh[0]) >= 1 && plane_geometry(mesh[1], mesh[2], false).bytes != 0;
}

// d_out (nb rows, leading dimension ldx doubles, ldx even and >= 2 npts) from nb real rows of G points; zbuf: nb * gc complex
int spectral_rows_own(isdf_handle h, const double* d_in, int nb, const int32_t mesh[3], const int32_t* d_idx,
                      const double* d_scale, int npts, double* d_out, int64_t ldx, double2* zbuf) {
  const int n0 = mesh[0], n1 = mesh[1], n2 = mesh[2], n2h = n2 / 2 + 1;
  Axis ax[3];
  if (int rc = make_axes(h, mesh, ax, "spectral_rows_own")) return rc;
  const int64_t gc = (int64_t)n0 * n1 * n2h;
  const PlaneGeo geo = plane_geometry(n1, n2, false);
  const int FX = fast_lines(n0);
  ARG_CHECK(h, geo.bytes && FX >= 1 && (int64_t)nb * n0 < 2147483647LL && nb <= 65535 && (ldx & 1) == 0 && ldx >= 2 * (int64_t)npts);
  // algorithmic bytes: the real rows in, the packed rows out
  ProfScope ps(h, "spectral_rows_own[byte]", (8.0 * (double)n0 * n1 * n2 + 8.0 * (double)ldx) * nb, 3);
  if (int rc = launch_plane_fwd(h, d_in, zbuf, ax, geo, (int)((int64_t)nb * n0), PIPE_ANY)) return rc;
  launch_strided<0>(h, true, FX, zbuf, nb, gc, (int64_t)n1 * n2h, n1 * n2h, ax[0], nullptr);
  const int64_t ldx2 = ldx / 2;
  spectral_pack_kernel<<<dim3((unsigned)cdiv(ldx2, 256), (unsigned)nb), dim3(256), 0, h->stream>>>(zbuf, gc, d_idx, d_scale, npts,
                                                                                                  (double2*)d_out, ldx2);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

// spectral_rows_own with the x pass over the listed x-lines only, packing as it goes (strided_fft_lines_kernel): the lines are
// read once and nothing but X is written.  d_lines = the distinct x-lines idx % (n1 n2h) of the packed points in ascending
// order, padded with -1 to nlines_pad (a multiple of 16: every x tile divides it); d_slot, d_slot_scale (nlines_pad / tile, n0,
// tile): the packed position of the point (line, kx) or -1, and its scale; tile = spectral_lines_tile(mesh).  Bit for bit
// spectral_rows_own's X.
int spectral_lines_tile(const int32_t mesh[3]) { return fast_lines(mesh[0]); }

int spectral_rows_lines_own(isdf_handle h, const double* d_in, int nb, const int32_t mesh[3], int npts, const int32_t* d_lines,
                            int nlines_pad, const int32_t* d_slot, const double* d_slot_scale, double* d_out, int64_t ldx,
                            double2* zbuf) {
  const int n0 = mesh[0], n1 = mesh[1], n2 = mesh[2], n2h = n2 / 2 + 1;
  Axis ax[3];
  if (int rc = make_axes(h, mesh, ax, "spectral_rows_lines_own")) return rc;
  const int64_t gc = (int64_t)n0 * n1 * n2h;
  const PlaneGeo geo = plane_geometry(n1, n2, false);
  const int FX = fast_lines(n0);
  ARG_CHECK(h, geo.bytes && FX >= 1 && (int64_t)nb * n0 < 2147483647LL && nb <= 65535 && (ldx & 1) == 0 && ldx >= 2 * (int64_t)npts);
  ARG_CHECK(h, d_lines && d_slot && d_slot_scale && nlines_pad >= 16 && nlines_pad % 16 == 0 &&
                   (int64_t)nb * (nlines_pad / FX) < 2147483647LL);
  ProfScope ps(h, "spectral_rows_own[byte]", (8.0 * (double)n0 * n1 * n2 + 8.0 * (double)ldx) * nb, 2);
  if (int rc = launch_plane_fwd(h, d_in, zbuf, ax, geo, (int)((int64_t)nb * n0), PIPE_ANY)) return rc;
  const int nt = nlines_pad / FX;
  with_lines(FX, [&](auto z) {
    strided_fft_lines_kernel<decltype(z)::value><<<dim3((unsigned)((int64_t)nb * nt)), dim3(TPB), sizeof(double2) * ((size_t)n0 * FX + n0),
                                                   h->stream>>>(zbuf, gc, (int64_t)n1 * n2h, ax[0], nt, d_lines, d_slot, d_slot_scale,
                                                                npts, (double2*)d_out, ldx / 2);
  });
  KERNEL_CHECK(h);
  return ISDF_OK;
}

// k-point convolution of real rows with a FULL real kernel table (n0, n1, n2; no 1/G inside): Vre + i Vim = ifft(tab fft(rows)).
// zhalf: nb * n0 n1 (n2/2+1) complex scratch, zfull: nb * G complex scratch.  Supported: 2-3-5 smooth meshes whose real and
// complex (y, z) planes fit LDS (up to ~100^2 per plane: the k-point configs of BASELINE.json); the caller falls back to hipFFT.
bool conv_rows_q_own_supported(isdf_handle h, const int32_t mesh[3], int nb) {
  if (!h->own_fft) return false;
  if (nb < 1 || nb > 65535 || (int64_t)nb * mesh[0] >= 2147483647LL) return false;
  Axis ax[3];
  for (int d = 0; d < 3; ++d)
    if (mesh[d] < 2 || mesh[d] > 1024 || !factorise(mesh[d], &ax[d]) || !smooth235(ax[d])) return false;
  return fast_lines(mesh[0]) >= 1 && plane_geometry(mesh[1], mesh[2], false).bytes && plane_geometry(mesh[1], mesh[2], true).bytes;
}

int conv_rows_q_own(isdf_handle h, const double* d_in, double* d_re, double* d_im, int nb, const int32_t mesh[3],
                    const double* tab, double2* zhalf, double2* zfull) {
  const int n0 = mesh[0], n1 = mesh[1], n2 = mesh[2], n2h = n2 / 2 + 1;
  Axis ax[3];
  if (int rc = make_axes(h, mesh, ax, "conv_rows_q_own")) return rc;
  const int64_t G = (int64_t)n0 * n1 * n2, gc = (int64_t)n0 * n1 * n2h;
  const PlaneGeo geo_r = plane_geometry(n1, n2, false), geo_c = plane_geometry(n1, n2, true);
  const int FX = fast_lines(n0);
  ARG_CHECK(h, geo_r.bytes && geo_c.bytes && FX >= 1 && (int64_t)nb * n0 < 2147483647LL && nb <= 65535);
  // algorithmic bytes as the hipFFT form's label counts them: 8 G in, 16 G out per row and the table
  ProfScope ps(h, "coulomb_conv_q_own[byte]", 64.0 * (double)G * nb, 5);
  const int nplanes = (int)((int64_t)nb * n0);
  if (int rc = launch_plane_fwd(h, d_in, zhalf, ax, geo_r, nplanes, PIPE_Q_MAX)) return rc;
  launch_strided<0>(h, true, FX, zhalf, nb, gc, (int64_t)n1 * n2h, n1 * n2h, ax[0], nullptr);
  expand_mul_kernel<<<dim3((unsigned)cdiv(G, 256), (unsigned)nb), dim3(256), 0, h->stream>>>(zhalf, zfull, tab, n0, n1, n2,
                                                                                            1.0 / (double)G);
  launch_strided<1>(h, true, FX, zfull, nb, G, (int64_t)n1 * n2, n1 * n2, ax[0], nullptr);
  if (int rc = launch_plane_c2c_inv(h, zfull, d_re, d_im, ax, geo_c, nplanes)) return rc;
  KERNEL_CHECK(h);
  return ISDF_OK;
}
