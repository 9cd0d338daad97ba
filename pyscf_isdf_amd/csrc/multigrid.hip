// Multigrid J / LDA potential (the role of pyscf/pbc/dft/multigrid/multigrid.py:500-680,838-935,
// 1046-1150): the density of the sharp basis functions is collocated on the dense mesh, that of smoother ones on coarser
// level meshes; the level spectra are added into the dense mesh's spectrum at the matching frequencies, the potential
// spectrum is cut back to each level and integrated there.
//
// What lives here: the spectrum traffic between a level mesh and the dense mesh (half spectra of real fields throughout:
// D2Z / Z2D, (n0, n1, n2/2+1) complex per field), the rectangular density contraction rho = sum_(mu in A, nu in B) aoA D aoB,
// the Coulomb kernel on a spectrum, the functionals (Slater, VWN, Becke-88, LYP: one device function per point each, their own
// kernels and the fused weighted sum), their second derivatives and a deterministic dot product.  The rectangular potential
// integral V = aoA (v .* aoB)^T is isdf_gemm_nt with its per-k scale.
//
// Frequencies follow numpy.fft.fftfreq like the reference's index lists (multigrid.py:669-673): index i of an n-point axis
// carries f = i for i < (n+1)/2, else i - n, and sits at index f (f >= 0) or N + f (f < 0) of the N-point dense axis.  Along
// the halved axis only f >= 0 is stored on both meshes.  The Nyquist entries of an even level mesh need care (see nyq_info):
// the reference keeps a non-Hermitian spectrum and the real part of the field; here the Hermitian equivalent is stored.
#include "common.h"

namespace {

constexpr int64_t RCHUNK = 32768;   // grid columns per pass of the density contraction

__device__ inline int dense_index(int i, int n, int N) {
  const int f = (i < (n + 1) / 2) ? i : i - n;
  return f >= 0 ? f : f + N;
}

// Nyquist entries of an even level mesh (index n/2 along an axis on which the dense mesh is finer - "proper" Nyquist below).
// The reference places such an entry v at dense frequency -n/2 ONLY (fftfreq labels it so, multigrid.py:669-673), leaves +n/2
// empty and takes .real of the transformed field at the end: the real field it keeps has the spectrum (R(f) + conj(R(-f)))/2,
// i.e. v/2 at f_L and conj(v)/2 at -f_L for an entry whose frequency vector f_L has a proper Nyquist component (every other entry
// meets its own Hermitian partner and keeps weight 1).  A half spectrum can only hold Hermitian fields, so that symmetrised
// form is what is stored: weight 1/2, at f_L when its z component is stored (>= 0), else as the conjugate at -f_L; in a
// self-conjugate z plane (z = 0, or the dense mesh's own Nyquist plane) both f_L and -f_L are stored and both are written; in an
// interior z plane the thread also writes for the level's unstored partner entry (see the kernel).
// The map stays injective: a +n/2 component is produced by these entries only.
struct NyqInfo { bool pnx, pny, pnz, any; };
__device__ inline NyqInfo nyq_info(int ix, int iy, int iz, int n0, int n1, int n2, int N0, int N1, int N2) {
  NyqInfo q;
  q.pnx = (n0 % 2 == 0) && ix == n0 / 2 && N0 > n0;
  q.pny = (n1 % 2 == 0) && iy == n1 / 2 && N1 > n1;
  q.pnz = (n2 % 2 == 0) && iz == n2 / 2 && N2 > n2;
  q.any = q.pnx || q.pny || q.pnz;
  return q;
}

// full[set][dense(ix,iy,iz)] (+)= scale * sub[set][ix,iy,iz]; the map is injective, so no two threads meet
__global__ void spectrum_embed_kernel(const double2* __restrict__ sub, int n0, int n1, int n2h, int n2, double2* __restrict__ full,
                                      int N0, int N1, int N2h, int N2, double scale, int accumulate) {
  const int64_t gc = (int64_t)n0 * n1 * n2h;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= gc) return;
  const int set = blockIdx.y;
  const int iz = (int)(idx % n2h);
  const int iy = (int)((idx / n2h) % n1);
  const int ix = (int)(idx / ((int64_t)n2h * n1));
  const NyqInfo q = nyq_info(ix, iy, iz, n0, n1, n2, N0, N1, N2);
  const int jx = dense_index(ix, n0, N0), jy = dense_index(iy, n1, N1);
  const int mx = (N0 - jx) % N0, my = (N1 - jy) % N1;                       // the dense indices of -fx, -fy
  const double2 v = sub[(int64_t)set * gc + idx];
  const double w = q.any ? 0.5 * scale : scale;
  double2* base = full + (int64_t)set * N0 * N1 * N2h;
  auto put = [&](int tx, int ty, int tz, double re, double im) {
    double2* p = base + ((int64_t)tx * N1 + ty) * N2h + tz;
    if (accumulate) { p->x += re; p->y += im; }
    else { p->x = re; p->y = im; }
  };
  if (q.pnz) {
    put(mx, my, iz, w * v.x, -w * v.y);                                      // f_L has z = -n2/2: stored as the conjugate at -f_L
  } else {
    put(jx, jy, iz, w * v.x, w * v.y);
    if (q.any) {
      const bool self_z = iz == 0 || ((n2 % 2 == 0) && iz == n2 / 2);       // (the second case: N2 == n2 here)
      if (self_z) {
        put(mx, my, iz, w * v.x, -w * v.y);                                  // -f_L lies in the same, self-conjugate, stored plane
      } else {
        // an interior z plane: the level's partner entry (-ix, -iy, -iz) is not stored on the level side, so this thread also
        // places ITS contribution conj(conj(v))/2 - at f_L with the proper Nyquist components flipped to +n/2
        put(q.pnx ? n0 / 2 : jx, q.pny ? n1 / 2 : jy, iz, w * v.x, w * v.y);
      }
    }
  }
}

// sub[set][ix,iy,iz] = scale * (the reference's level spectrum after its .real): for a Hermitian dense spectrum V that is
// V(f_L) for ordinary entries and (V(f_L) + V(f_L with its proper Nyquist components flipped to +n/2)) / 2 for Nyquist entries
// (multigrid.py:905-915 picks the fftfreq entries and keeps the real part of the level field)
__global__ void spectrum_restrict_kernel(const double2* __restrict__ full, int N0, int N1, int N2h, int N2, double2* __restrict__ sub,
                                         int n0, int n1, int n2h, int n2, double scale) {
  const int64_t gc = (int64_t)n0 * n1 * n2h;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= gc) return;
  const int set = blockIdx.y;
  const int iz = (int)(idx % n2h);
  const int iy = (int)((idx / n2h) % n1);
  const int ix = (int)(idx / ((int64_t)n2h * n1));
  const NyqInfo q = nyq_info(ix, iy, iz, n0, n1, n2, N0, N1, N2);
  const int jx = dense_index(ix, n0, N0), jy = dense_index(iy, n1, N1);
  const double2* base = full + (int64_t)set * N0 * N1 * N2h;
  auto get = [&](int tx, int ty, int tz) { return base[((int64_t)tx * N1 + ty) * N2h + tz]; };
  double2 r;
  if (!q.any) {
    r = get(jx, jy, iz);
  } else {
    const int fx = q.pnx ? n0 / 2 : jx, fy = q.pny ? n1 / 2 : jy;            // flipped components: +n/2
    double2 a, b = get(fx, fy, iz);                                          // (flipped z = +n2/2 = iz when pnz)
    if (q.pnz) {
      a = get((N0 - jx) % N0, (N1 - jy) % N1, iz);                           // V(fx, fy, -n2/2) = conj V(-fx, -fy, +n2/2)
      a.y = -a.y;
    } else {
      a = get(jx, jy, iz);
    }
    r = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y + b.y));
  }
  sub[(int64_t)set * gc + idx] = make_double2(scale * r.x, scale * r.y);
}

__global__ void spectrum_scale_kernel(double2* __restrict__ z, const double* __restrict__ table, int64_t gc) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= gc) return;
  double2* q = z + (int64_t)blockIdx.y * gc + idx;
  const double c = table[idx];
  q->x *= c; q->y *= c;
}

// rho[g] = sum_mu T[mu, g] * aoA[mu, g]
__global__ void rho_pair_reduce_kernel(const double* __restrict__ T, int64_t ldT, const double* __restrict__ aoA, int64_t ld, int nA,
                                       int64_t ng, double* __restrict__ rho) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ng) return;
  double s = 0.0;
#pragma unroll 4
  for (int mu = 0; mu < nA; ++mu) s = fma(T[(int64_t)mu * ldT + g], aoA[(int64_t)mu * ld + g], s);
  rho[g] = s;
}

// Per-point functionals.  Each is written once and called from its own kernel and from the fused one (xc_fused_kernel).
//
// Slater exchange of a spin-unpolarised density: exc = -(3/4) (3/pi)^(1/3) rho^(1/3) per particle, vxc = (4/3) exc.
// Densities at or below 1e-24 (the noise floor of the collocation, negative ripples of the FFT) give zero.
__device__ inline void slater_point(double r, double& e, double& v) {
  e = 0.0;
  if (r > 1e-24) e = -0.75 * cbrt(3.0 / 3.14159265358979323846) * cbrt(r);
  v = (4.0 / 3.0) * e;
}

__global__ void lda_exchange_kernel(const double* __restrict__ rho, int64_t n, double* __restrict__ exc, double* __restrict__ vxc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double e, v;
  slater_point(rho[i], e, v);
  exc[i] = e;
  vxc[i] = v;
}

// VWN correlation of a spin-unpolarised density (Vosko, Wilk, Nusair, Can. J. Phys. 58, 1200 (1980), eq. 4.4) with the
// paramagnetic parameters (A, b, c, x0) of one of the paper's fits:
// eps_c = A { ln(x^2/X) + 2b/Q atan(Q/(2x+b)) - b x0/X(x0) [ ln((x-x0)^2/X) + 2(b+2 x0)/Q atan(Q/(2x+b)) ] },  x = sqrt(rs),
// X = x^2 + b x + c, Q = sqrt(4c - b^2);  v_c = eps_c - (x/6) d eps_c/dx.  Densities at or below 1e-24 give zero.
struct VwnFit { double A, b, c, x0; };
// fit V (libxc LDA_C_VWN, the correlation of the reference's 'lda,vwn' and of B3LYP5) and the fit to the RPA energies (libxc
// LDA_C_VWN_RPA, the correlation of the reference's 'b3lyp')
__device__ inline VwnFit vwn_fit(int rpa) {
  return rpa ? VwnFit{0.0310907, 13.0720, 42.7198, -0.409286} : VwnFit{0.0310907, 3.72744, 12.9352, -0.10498};
}

__device__ inline void vwn_point(double r, const VwnFit p, double& ec, double& vc) {
  ec = 0.0;
  vc = 0.0;
  if (!(r > 1e-24)) return;
  const double A = p.A, b = p.b, c = p.c, x0 = p.x0;
  const double rs = cbrt(3.0 / (4.0 * 3.14159265358979323846 * r));
  const double x = sqrt(rs);
  const double X = x * x + b * x + c, X0 = x0 * x0 + b * x0 + c;
  const double Q = sqrt(4.0 * c - b * b);
  const double at = atan(Q / (2.0 * x + b));
  ec = A * (log(x * x / X) + 2.0 * b / Q * at - b * x0 / X0 * (log((x - x0) * (x - x0) / X) + 2.0 * (b + 2.0 * x0) / Q * at));
  const double den = Q * Q + (2.0 * x + b) * (2.0 * x + b);
  const double dec = A * (2.0 / x - (2.0 * x + b) / X - 4.0 * b / den
                          - b * x0 / X0 * (2.0 / (x - x0) - (2.0 * x + b) / X - 4.0 * (b + 2.0 * x0) / den));
  vc = ec - x / 6.0 * dec;
}

// VWN5 (fit V) ADDED to exc / vxc
__global__ void lda_vwn_add_kernel(const double* __restrict__ rho, int64_t n, double* __restrict__ exc, double* __restrict__ vxc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double r = rho[i];
  if (!(r > 1e-24)) return;
  double ec, vc;
  vwn_point(r, vwn_fit(0), ec, vc);
  exc[i] += ec;
  vxc[i] += vc;
}

// Becke-88 exchange of a spin-unpolarised density (libxc GGA_X_B88; Becke, PRA 38, 3098): per spin channel
// f(rho_s, g_s) = rho_s^(4/3) G(x), x = g_s / rho_s^(4/3), G = -C_x - beta x^2 / (1 + 6 beta x asinh x), C_x = (3/2)(3/4pi)^(1/3),
// beta = 0.0042; e(rho, grad rho) = 2 f(rho/2, |grad rho|/2).  Outputs: exc = e / rho, vrho = de/drho, and wfac with
// w = de/d(grad rho) = 2 vsigma grad rho = wfac grad rho (what multiplies grad(phi_mu phi_nu) in the potential matrix).
// rho <= 1e-14 gives zero.
struct B88Parts { double r13, r43, x, Gx, Gp_over_x; };        // rho_s^(1/3), rho_s^(4/3), x, G(x), G'(x) / x (finite at x = 0)
__device__ inline B88Parts b88_parts(double r, double g2) {
  const double beta = 0.0042;
  const double cx = 1.5 * cbrt(3.0 / (4.0 * 3.14159265358979323846));
  const double rs = 0.5 * r;
  const double r13 = cbrt(rs), r43 = rs * r13;
  const double gs = 0.5 * sqrt(g2);
  const double x = gs / r43;
  const double as = asinh(x);
  const double D = 1.0 + 6.0 * beta * x * as;
  const double Dp = 6.0 * beta * (as + x / sqrt(1.0 + x * x));
  const double Gx = -cx - beta * x * x / D;
  const double Gp_over_x = -beta * (2.0 * D - x * Dp) / (D * D);
  return B88Parts{r13, r43, x, Gx, Gp_over_x};
}

__device__ inline void b88_point(double r, double g2, double& e, double& vr, double& wfac) {
  e = 0.0;
  vr = 0.0;
  wfac = 0.0;
  if (r > 1e-14) {
    const B88Parts p = b88_parts(r, g2);
    e = 2.0 * p.r43 * p.Gx / r;
    vr = (4.0 / 3.0) * p.r13 * (p.Gx - p.x * p.x * p.Gp_over_x);
    // de/d|grad rho| = 2 f_gs / 2 = G'(x);  w = G'(x) grad rho / |grad rho| = (G'/x) grad rho / (2 rho_s^(4/3))
    wfac = p.Gp_over_x / (2.0 * p.r43);
  }
}

// Attenuation of the short-range exchange of Iikura, Tsuneda, Yanai and Hirao (JCP 115, 3540; libxc GGA_X_ITYH) and its derivative:
//   F(a) = 1 - (8/3) a [sqrt(pi) erf(1/(2a)) + 2a (b - c)],  b = exp(-1/(4a^2)) - 1,  c = 2 a^2 b + 1/2,
//   F'(a) = -(8/3) [sqrt(pi) erf(1/(2a)) + 2 a b - 16 a^3 b - 4 a].
// The direct form cancels as a grows (F(1) = 0.027 = 1 - 0.973; at the 1e-14 density threshold a is in the thousands): from a = 0.5
// on F is the expansion of the same expression in 1/(2a),
//   F = sum_(n >= 1) (-1)^(n+1) 2 / ((n+1)! (2n+1) (n+2) 4^n) a^(-2n) = 1/(36 a^2) - 1/(960 a^4) + 1/(26880 a^6) - ...,
// 16 terms (the 17th is 4e-18 of the first at a = 0.5).  In float64 against 30 digits on a from 1e-4 to 1e4: F 2.9e-15, F' 2.1e-15
// relative, both at the direct form just below the switch.  a = 0 gives F = 1 (exp underflows, erf(inf) = 1).
__device__ inline void ityh_attenuation(double a, double& F, double& dF) {
  if (a < 0.5) {
    const double rpi = 1.7724538509055160273;                              // sqrt(pi)
    const double er = erf(1.0 / (2.0 * a));
    const double b = exp(-1.0 / (4.0 * a * a)) - 1.0;
    const double c = 2.0 * a * a * b + 0.5;
    F = 1.0 - 8.0 * a * (rpi * er + 2.0 * a * (b - c)) / 3.0;
    dF = -8.0 * (rpi * er + 2.0 * a * b - 16.0 * a * a * a * b - 4.0 * a) / 3.0;
  } else {
    constexpr int NT = 16;
    constexpr double cn[NT] = {0.027777777777777776,    -0.0010416666666666667,  3.7202380952380956e-05,  -1.2056327160493827e-06,
                               3.522952741702742e-08,   -9.315500038156288e-10,  2.2426203795561436e-11,  -4.94695671960914e-13,
                               1.0059600984851122e-14,  -1.8961549475413822e-16, 3.3293690550475775e-18,  -5.469677733292448e-20,
                               8.440860699525384e-22,   -1.2279269336594038e-23, 1.689273295831248e-25,   -2.2040181890054163e-27};
    const double t = 1.0 / (a * a);
    double f = 0.0, d = 0.0;
#pragma unroll
    for (int n = NT; n >= 1; --n) {                                        // Horner from the smallest term
      f = (f + cn[n - 1]) * t;
      d = (d - 2.0 * n * cn[n - 1]) * t;
    }
    F = f;
    dF = d / a;
  }
}

// Short-range Becke-88 of a spin-unpolarised density: per spin f = rho_s^(4/3) G(x) F(a), a = omega / (2 k),
// k = sqrt(9 pi / K) rho_s^(1/3), K = -2 G(x) (the Fermi wave vector in the LDA limit); e = 2 f(rho/2, |grad rho|/2).  With
// d ln a / d rho_s = -(1 + 2 x G'/G) / (3 rho_s) and d ln a / d g_s = G' / (2 G rho_s^(4/3)):
//   vrho = rho_s^(1/3) [4 (G - x G') F - a F' (G + 2 x G')] / 3,   de/d|grad rho| = G' (F + a F'/2).
// Outputs as b88_point; rho <= 1e-14 gives zero.
__device__ inline void b88_sr_point(double r, double g2, double omega, double& e, double& vr, double& wfac) {
  e = 0.0;
  vr = 0.0;
  wfac = 0.0;
  if (r > 1e-14) {
    const B88Parts p = b88_parts(r, g2);
    const double k = sqrt(9.0 * 3.14159265358979323846 / (-2.0 * p.Gx)) * p.r13;
    const double a = omega / (2.0 * k);
    double F, dF;
    ityh_attenuation(a, F, dF);
    const double xGp = p.x * p.x * p.Gp_over_x;
    e = 2.0 * p.r43 * p.Gx * F / r;
    vr = p.r13 * (4.0 * (p.Gx - xGp) * F - a * dF * (p.Gx + 2.0 * xGp)) / 3.0;
    wfac = p.Gp_over_x * (F + 0.5 * a * dF) / (2.0 * p.r43);
  }
}

__global__ void gga_b88_kernel(const double* __restrict__ rho, const double* __restrict__ grad, int64_t gstride, int64_t n,
                               double* __restrict__ exc, double* __restrict__ vrho, double* __restrict__ w, int64_t wstride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double gx = grad[i], gy = grad[gstride + i], gz = grad[2 * gstride + i];
  double e, vr, wfac;
  b88_point(rho[i], gx * gx + gy * gy + gz * gz, e, vr, wfac);
  exc[i] = e;
  vrho[i] = vr;
  w[i] = wfac * gx;
  w[wstride + i] = wfac * gy;
  w[2 * wstride + i] = wfac * gz;
}

// Lee-Yang-Parr correlation (libxc GGA_C_LYP; Lee, Yang, Parr, PRB 37, 785) in the gradient-only form of Miehlich, Savin, Stoll,
// Preuss (CPL 157, 200), a = 0.04918, b = 0.132, c = 0.2533, d = 0.349.  With rho = rho_a + rho_b, t = rho^(-1/3),
// omega = exp(-c t) t^11 / (1 + d t), delta = c t + d t / (1 + d t), K = 2^(11/3) (3/10) (3 pi^2)^(2/3), the energy density is
//   e = -4a rho_a rho_b / (rho (1 + d t)) - a b omega G,
//   G = K rho_a rho_b (rho_a^(8/3) + rho_b^(8/3)) + G_aa sigma_aa + G_ab sigma_ab + G_bb sigma_bb,
//   G_aa = rho_a rho_b [(1 - 3 delta)/9 - (delta - 11)/9 rho_a/rho] - rho_b^2,  G_bb likewise,
//   G_ab = rho_a rho_b (47 - 7 delta)/9 - (4/3) rho^2.
// omega is formed from t (t^11 <= 1e52 at the threshold) and exp(-c t), which underflows to an exact zero below rho ~ 4e-11:
// nothing overflows for rho down to 1e-14.  d omega/d rho = omega (delta - 11)/(3 rho), d delta/d rho = -t (c + d/(1+dt)^2)/(3 rho).
// No division by a spin density: rho_b = 0 gives e = 0 and finite derivatives (LYP vanishes for a fully polarised density).
// A spin density <= 0 counts as zero with a zero gradient; rho <= 1e-14 gives zero, as in b88_point.
struct LypOut { double e, va, vb, vsaa, vsab, vsbb; };
__device__ inline LypOut lyp_point(double ra, double rb, double saa, double sab, double sbb) {
  LypOut o = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (!(ra > 0.0)) { ra = 0.0; saa = 0.0; sab = 0.0; }
  if (!(rb > 0.0)) { rb = 0.0; sbb = 0.0; sab = 0.0; }
  const double r = ra + rb;
  if (!(r > 1e-14)) return o;
  const double a = 0.04918, b = 0.132, c = 0.2533, d = 0.349;
  const double pi = 3.14159265358979323846;
  const double K = 8.0 * cbrt(4.0) * 0.3 * cbrt(9.0 * pi * pi * pi * pi);      // 2^(11/3) C_F, C_F = (3/10) (3 pi^2)^(2/3)
  const double t = 1.0 / cbrt(r);
  const double den = 1.0 + d * t;
  const double t2 = t * t, t4 = t2 * t2, t8 = t4 * t4;
  const double om = exp(-c * t) * (t8 * t2 * t) / den;
  const double dl = c * t + d * t / den;
  const double dlp = -t * (c + d / (den * den)) / (3.0 * r);
  const double omp = om * (dl - 11.0) / (3.0 * r);
  const double ca = cbrt(ra), cb = cbrt(rb);
  const double ra83 = ra * ra * ca * ca, rb83 = rb * rb * cb * cb;             // rho_s^(8/3)
  const double ab = ra * rb, xa = ra / r, xb = rb / r;
  const double c1 = (1.0 - 3.0 * dl) / 9.0, c2 = (dl - 11.0) / 9.0, c3 = (47.0 - 7.0 * dl) / 9.0;
  const double Gaa = ab * (c1 - c2 * xa) - rb * rb;
  const double Gbb = ab * (c1 - c2 * xb) - ra * ra;
  const double Gab = ab * c3 - (4.0 / 3.0) * r * r;
  const double G = K * ab * (ra83 + rb83) + Gaa * saa + Gab * sab + Gbb * sbb;
  // d/d rho_a and d/d rho_b of the three coefficients
  const double Gaa_a = rb * (c1 - c2 * xa) + ab * (-dlp / 3.0 - dlp * xa / 9.0 - c2 * xb / r);
  const double Gaa_b = ra * (c1 - c2 * xa) + ab * (-dlp / 3.0 - dlp * xa / 9.0 + c2 * xa / r) - 2.0 * rb;
  const double Gbb_b = ra * (c1 - c2 * xb) + ab * (-dlp / 3.0 - dlp * xb / 9.0 - c2 * xa / r);
  const double Gbb_a = rb * (c1 - c2 * xb) + ab * (-dlp / 3.0 - dlp * xb / 9.0 + c2 * xb / r) - 2.0 * ra;
  const double Gab_a = c3 * rb - (7.0 / 9.0) * dlp * ab - (8.0 / 3.0) * r;
  const double Gab_b = c3 * ra - (7.0 / 9.0) * dlp * ab - (8.0 / 3.0) * r;
  const double G_a = K * rb * ((11.0 / 3.0) * ra83 + rb83) + Gaa_a * saa + Gab_a * sab + Gbb_a * sbb;
  const double G_b = K * ra * ((11.0 / 3.0) * rb83 + ra83) + Gaa_b * saa + Gab_b * sab + Gbb_b * sbb;
  // F1 = rho_a rho_b / (rho den):  dF1/d rho_a = rho_b/(rho den) [1 - x_a + x_a d t / (3 den)]
  const double f1 = 1.0 / (r * den), f1t = d * t / (3.0 * den);
  o.e = -4.0 * a * ab * f1 - a * b * om * G;
  o.va = -4.0 * a * rb * f1 * (1.0 - xa + xa * f1t) - a * b * (omp * G + om * G_a);
  o.vb = -4.0 * a * ra * f1 * (1.0 - xb + xb * f1t) - a * b * (omp * G + om * G_b);
  o.vsaa = -a * b * om * Gaa;
  o.vsab = -a * b * om * Gab;
  o.vsbb = -a * b * om * Gbb;
  return o;
}

// exc per particle, vrho and w of  cs Slater + cb B88 + cv VWN (fit V, or the RPA fit with vwn_rpa) + cl LYP  of a spin-unpolarised
// density in one pass: 4 planes in, 5 planes out.  A component with weight 0 is not evaluated.  Closed-shell LYP is lyp_point at
// rho_a = rho_b = rho/2, sigma_aa = sigma_ab = sigma_bb = sigma/4: vrho = va, w = (vsaa + vsab + vsbb)/2 grad rho.
__device__ inline void xc_fused_point(double r, double g2, double cs, double cb, double cv, int vwn_rpa, double cl, double& e, double& vr,
                                      double& wfac) {
  e = 0.0;
  vr = 0.0;
  wfac = 0.0;
  if (cs != 0.0) {
    double es, vs;
    slater_point(r, es, vs);
    e += cs * es;
    vr += cs * vs;
  }
  if (cb != 0.0) {
    double eb, vb, wb;
    b88_point(r, g2, eb, vb, wb);
    e += cb * eb;
    vr += cb * vb;
    wfac += cb * wb;
  }
  if (cv != 0.0) {
    double ec, vc;
    vwn_point(r, vwn_fit(vwn_rpa), ec, vc);
    e += cv * ec;
    vr += cv * vc;
  }
  if (cl != 0.0 && r > 1e-14) {
    const double s = 0.25 * g2;
    const LypOut o = lyp_point(0.5 * r, 0.5 * r, s, s, s);
    e += cl * o.e / r;
    vr += cl * o.va;
    wfac += cl * 0.5 * (o.vsaa + o.vsab + o.vsbb);
  }
}

__global__ void xc_fused_kernel(const double* __restrict__ rho, const double* __restrict__ grad, int64_t gstride, int64_t n, double cs,
                                double cb, double cv, int vwn_rpa, double cl, double* __restrict__ exc, double* __restrict__ vrho,
                                double* __restrict__ w, int64_t wstride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double gx = grad[i], gy = grad[gstride + i], gz = grad[2 * gstride + i];
  double e, vr, wfac;
  xc_fused_point(rho[i], gx * gx + gy * gy + gz * gz, cs, cb, cv, vwn_rpa, cl, e, vr, wfac);
  exc[i] = e;
  vrho[i] = vr;
  w[i] = wfac * gx;
  w[wstride + i] = wfac * gy;
  w[2 * wstride + i] = wfac * gz;
}

// The same sum + csr short-range B88 at ``omega`` (the semilocal part of a range-separated hybrid; CAM-B3LYP is 0.35 B88 + 0.46
// short-range B88 + 0.19 VWN5 + 0.81 LYP at omega = 0.33): the fused point, then the one further term.  csr = 0 is xc_fused_kernel.
__global__ void xc_fused_rsh_kernel(const double* __restrict__ rho, const double* __restrict__ grad, int64_t gstride, int64_t n,
                                    double cs, double cb, double cv, int vwn_rpa, double cl, double csr, double omega,
                                    double* __restrict__ exc, double* __restrict__ vrho, double* __restrict__ w, int64_t wstride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double r = rho[i];
  const double gx = grad[i], gy = grad[gstride + i], gz = grad[2 * gstride + i];
  const double g2 = gx * gx + gy * gy + gz * gz;
  double e, vr, wfac;
  xc_fused_point(r, g2, cs, cb, cv, vwn_rpa, cl, e, vr, wfac);
  if (csr != 0.0) {
    double eb, vb, wb;
    b88_sr_point(r, g2, omega, eb, vb, wb);
    e += csr * eb;
    vr += csr * vb;
    wfac += csr * wb;
  }
  exc[i] = e;
  vrho[i] = vr;
  w[i] = wfac * gx;
  w[wstride + i] = wfac * gy;
  w[2 * wstride + i] = wfac * gz;
}

// Spin-polarised LYP, scaled by ``weight``: rho (spin s at s sstride), grad (component c of spin s at c gcstride + s sstride) ->
// ec = weight e (energy DENSITY), vrho[s] (+)= weight de/d rho_s, w[s] (+)= weight de/d(grad rho_s) = weight (2 vs_ss grad rho_s +
// vs_ab grad rho_s'), spin s at s osstride, component c of w at c wcstride.  LYP couples the spin channels: no spin scaling.
__global__ void lyp_polarised_kernel(const double* __restrict__ rho, const double* __restrict__ grad, int64_t gcstride, int64_t sstride,
                                     int64_t n, double weight, int accumulate, double* __restrict__ ec, double* __restrict__ vrho,
                                     double* __restrict__ w, int64_t wcstride, int64_t osstride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double ga[3], gb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ga[c] = grad[c * gcstride + i];
    gb[c] = grad[c * gcstride + sstride + i];
  }
  const double ra = rho[i], rb = rho[sstride + i];
  // a spin density <= 0 counts as zero with a zero gradient (lyp_point does the same to the invariants)
  if (!(ra > 0.0)) ga[0] = ga[1] = ga[2] = 0.0;
  if (!(rb > 0.0)) gb[0] = gb[1] = gb[2] = 0.0;
  const LypOut o = lyp_point(ra, rb, ga[0] * ga[0] + ga[1] * ga[1] + ga[2] * ga[2], ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2],
                             gb[0] * gb[0] + gb[1] * gb[1] + gb[2] * gb[2]);
  ec[i] = weight * o.e;
  const double va = weight * o.va, vb = weight * o.vb;
  if (accumulate) { vrho[i] += va; vrho[osstride + i] += vb; }
  else { vrho[i] = va; vrho[osstride + i] = vb; }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double wa = weight * (2.0 * o.vsaa * ga[c] + o.vsab * gb[c]);
    const double wb = weight * (2.0 * o.vsbb * gb[c] + o.vsab * ga[c]);
    if (accumulate) { w[c * wcstride + i] += wa; w[c * wcstride + osstride + i] += wb; }
    else { w[c * wcstride + i] = wa; w[c * wcstride + osstride + i] = wb; }
  }
}

// second derivative of the Slater exchange energy density: f = d2(rho exc)/d rho2 = (4/9) C rho^(-2/3), C = -(3/4)(3/pi)^(1/3)
__global__ void lda_exchange_fxc_kernel(const double* __restrict__ rho, int64_t n, double* __restrict__ fxc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double r = rho[i];
  double f = 0.0;
  if (r > 1e-24) {
    const double c = cbrt(r);
    f = -(1.0 / 3.0) * cbrt(3.0 / 3.14159265358979323846) / (c * c);
  }
  fxc[i] = f;
}

// d2(rho eps_c)/d rho2 of the VWN5 correlation of lda_vwn_add_kernel: with v_c = eps_c - (x/6) eps_c'(x) and dx/drho = -x/(6 rho),
// f_c = -x (5 eps_c' - x eps_c'') / (36 rho); ADDED to fxc (the exchange part comes from lda_exchange_fxc_kernel)
__global__ void lda_vwn_fxc_add_kernel(const double* __restrict__ rho, int64_t n, double* __restrict__ fxc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double r = rho[i];
  if (!(r > 1e-24)) return;
  const double A = 0.0310907, b = 3.72744, c = 12.9352, x0 = -0.10498;
  const double rs = cbrt(3.0 / (4.0 * 3.14159265358979323846 * r));
  const double x = sqrt(rs);
  const double X = x * x + b * x + c, X0 = x0 * x0 + b * x0 + c;
  const double Q = sqrt(4.0 * c - b * b);
  const double t = 2.0 * x + b;
  const double den = Q * Q + t * t;
  const double dec = A * (2.0 / x - t / X - 4.0 * b / den - b * x0 / X0 * (2.0 / (x - x0) - t / X - 4.0 * (b + 2.0 * x0) / den));
  const double dtX = (2.0 * X - t * t) / (X * X);                          // d/dx (2x + b) / X
  const double d2ec = A * (-2.0 / (x * x) - dtX + 16.0 * b * t / (den * den)
                           - b * x0 / X0 * (-2.0 / ((x - x0) * (x - x0)) - dtX + 16.0 * (b + 2.0 * x0) * t / (den * den)));
  fxc[i] += -x * (5.0 * dec - x * d2ec) / (36.0 * r);
}

// Becke-88 second derivative of the closed-shell energy density e(rho, grad rho) = 2 f(rho/2, |grad rho|/2) of gga_b88_kernel, in
// the layout of eval_xc_eff (spin 0, (4, 4) per point over (rho, d_x rho, d_y rho, d_z rho)):
//   fxc[0][0] = v2rho2 = (2/9) rho_s^(-2/3) (G - x G' + 4 x^2 G''),
//   fxc[0][i] = 2 v2rhosigma d_i rho = -G'' / (3 rho_s^(7/3)) d_i rho,
//   fxc[i][j] = 4 v2sigma2 d_i rho d_j rho + 2 vsigma delta_ij = (G'' - G'/x) / x^2 / (8 rho_s^4) d_i rho d_j rho
//               + G'/x / (2 rho_s^(4/3)) delta_ij.
// With u = x^2 / D, D = 1 + 6 beta x asinh x: G' = -beta u', G'' = -beta u'' and (G'' - G'/x) / x^2 = -beta (2 D'^2 - D D'' - 3 D D'/x)
// / D^3, where D'/x = 6 beta (asinh(x)/x + 1/sqrt(1 + x^2)) - every term finite at x = 0 once asinh(x)/x is taken from its series
// below x = 1e-3 (the next term, 5 x^6 / 112, is below the rounding there).  rho <= 1e-14 gives zero, as the potential.
// Output: the 10 unique components, row-major upper triangle (00 01 02 03 11 12 13 22 23 33).
__device__ inline void b88_fxc_point(double r, double gx, double gy, double gz, double f[10]) {
  for (int k = 0; k < 10; ++k) f[k] = 0.0;
  if (!(r > 1e-14)) return;
  const double beta = 0.0042;
  const double cx = 1.5 * cbrt(3.0 / (4.0 * 3.14159265358979323846));
  const double rs = 0.5 * r;
  const double r13 = cbrt(rs), r43 = rs * r13;
  const double x = 0.5 * sqrt(gx * gx + gy * gy + gz * gz) / r43;
  const double x2 = x * x;
  const double as = asinh(x);
  const double s = sqrt(1.0 + x2);
  const double ash_x = x < 1e-3 ? 1.0 - x2 / 6.0 + 0.075 * x2 * x2 : as / x;
  const double D = 1.0 + 6.0 * beta * x * as;
  const double Dp = 6.0 * beta * (as + x / s);
  const double Dpp = 6.0 * beta * (2.0 + x2) / (s * s * s);
  const double Dp_x = 6.0 * beta * (ash_x + 1.0 / s);
  const double D3 = D * D * D;
  const double Gx = -cx - beta * x2 / D;
  const double Gp_x = -beta * (2.0 * D - x * Dp) / (D * D);
  const double Gpp = -beta * ((2.0 * D - x2 * Dpp) * D - 2.0 * x * Dp * (2.0 * D - x * Dp)) / D3;
  const double H = -beta * (2.0 * Dp * Dp - D * Dpp - 3.0 * D * Dp_x) / D3;
  const double f00 = (2.0 / 9.0) * (Gx - x2 * Gp_x + 4.0 * x2 * Gpp) / (r13 * r13);
  const double c01 = -Gpp / (3.0 * rs * r43);
  const double vs2 = Gp_x / (2.0 * r43);
  const double s2 = H / (8.0 * rs * rs * rs * rs);
  f[0] = f00;
  f[1] = c01 * gx; f[2] = c01 * gy; f[3] = c01 * gz;
  f[4] = s2 * gx * gx + vs2; f[5] = s2 * gx * gy; f[6] = s2 * gx * gz;
  f[7] = s2 * gy * gy + vs2; f[8] = s2 * gy * gz;
  f[9] = s2 * gz * gz + vs2;
}

// index of (x, y) in the 10-component upper triangle
__device__ inline int sym4(int x, int y) {
  const int a = x < y ? x : y, b = x < y ? y : x;
  return a * 4 - a * (a - 1) / 2 + (b - a);
}

// wv[n][y] = sum_x rho1[n][x] fxc[x][y] with the B88 kernel of rho0 (4 planes, r0s apart): the kernel is made once per point and
// applied to all nset response 4-vectors (plane (x, n) at x * r1x + n * r1n, output at y * wx + n * wn); fout (optional): the 10
// unique components, fs apart
__global__ void gga_b88_fxc_kernel(const double* __restrict__ rho0, int64_t r0s, int64_t n, const double* __restrict__ rho1,
                                   int64_t r1x, int64_t r1n, int nset, double* __restrict__ wv, int64_t wx, int64_t wn,
                                   double* __restrict__ fout, int64_t fs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double f[10];
  b88_fxc_point(rho0[i], rho0[r0s + i], rho0[2 * r0s + i], rho0[3 * r0s + i], f);
  if (fout)
    for (int k = 0; k < 10; ++k) fout[k * fs + i] = f[k];
  for (int m = 0; m < nset; ++m) {
    double r1[4];
    for (int x = 0; x < 4; ++x) r1[x] = rho1[x * r1x + m * r1n + i];
    for (int y = 0; y < 4; ++y) {
      double acc = 0.0;
      for (int x = 0; x < 4; ++x) acc = fma(r1[x], f[sym4(x, y)], acc);
      wv[y * wx + m * wn + i] = acc;
    }
  }
}

// wv[n][y] (+)= sum_x rho1[n][x] fxc[x][y] for a caller's kernel (x, y < NX; fxc[x][y] at x * fx + y * fy)
template <int NX>
__global__ void xc_fxc_apply_kernel(const double* __restrict__ fxc, int64_t fx, int64_t fy, int64_t n, const double* __restrict__ rho1,
                                    int64_t r1x, int64_t r1n, int nset, double* __restrict__ wv, int64_t wx, int64_t wn, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double f[NX][NX];
  for (int x = 0; x < NX; ++x)
    for (int y = 0; y < NX; ++y) f[x][y] = fxc[x * fx + y * fy + i];
  for (int m = 0; m < nset; ++m) {
    double r1[NX];
    for (int x = 0; x < NX; ++x) r1[x] = rho1[x * r1x + m * r1n + i];
    for (int y = 0; y < NX; ++y) {
      double acc = 0.0;
      for (int x = 0; x < NX; ++x) acc = fma(r1[x], f[x][y], acc);
      double* p = wv + y * wx + m * wn + i;
      *p = accumulate ? *p + acc : acc;
    }
  }
}

// two-stage deterministic reduction: partial[b] = sum over block b's strided elements of x (* y)
__global__ void dot_partial_kernel(const double* __restrict__ x, const double* __restrict__ y, int64_t n, double* __restrict__ partial) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += y ? x[i] * y[i] : x[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ void dot_final_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

// coords[d][g] = sum_i f_i a[i][d], f_i = numpy.fft.fftfreq(n_i)[index_i]: the uniform grid in the order and with the folding of
// cell.get_uniform_grids (cell.py:874-898, wrap_around = True), structure of arrays
__global__ void uniform_grid_kernel(double* __restrict__ coords, int n0, int n1, int n2, const double a0, const double a1,
                                    const double a2, const double a3, const double a4, const double a5, const double a6,
                                    const double a7, const double a8) {
  const int64_t G = (int64_t)n0 * n1 * n2;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int iz = (int)(g % n2), iy = (int)((g / n2) % n1), ix = (int)(g / ((int64_t)n2 * n1));
  const double fx = (double)((ix < (n0 + 1) / 2) ? ix : ix - n0) / (double)n0;
  const double fy = (double)((iy < (n1 + 1) / 2) ? iy : iy - n1) / (double)n1;
  const double fz = (double)((iz < (n2 + 1) / 2) ? iz : iz - n2) / (double)n2;
  coords[g] = fx * a0 + fy * a3 + fz * a6;
  coords[G + g] = fx * a1 + fy * a4 + fz * a7;
  coords[2 * G + g] = fx * a2 + fy * a5 + fz * a8;
}

bool mesh_fits(const int32_t sub[3], const int32_t full[3]) {
  for (int d = 0; d < 3; ++d)
    if (sub[d] <= 0 || sub[d] > full[d]) return false;
  return true;
}

}  // namespace

extern "C" int isdf_uniform_grid(isdf_handle h, const int32_t mesh[3], const double a[9], double* d_coords_soa) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, mesh && a && d_coords_soa && mesh[0] > 0 && mesh[1] > 0 && mesh[2] > 0);
  const int64_t G = (int64_t)mesh[0] * mesh[1] * mesh[2];
  hipLaunchKernelGGL(uniform_grid_kernel, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, h->stream, d_coords_soa, mesh[0], mesh[1],
                     mesh[2], a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_rho_pair(isdf_handle h, const double* d_aoA, int nA, const double* d_aoB, int nB, int64_t ng, int64_t ld,
                             const double* d_dm, int nset, double* d_rho, int64_t ldrho) {
  // rho[i, g] = sum_(mu < nA, nu < nB) aoA[mu, g] dm[i, mu, nu] aoB[nu, g]
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_aoA && d_aoB && d_dm && d_rho && nA > 0 && nB > 0 && ng > 0 && ld >= ng && nset > 0 && ldrho >= ng);
  double* T = (double*)isdf_ws(h, "mg_T", sizeof(double) * (size_t)nA * RCHUNK);
  if (!T) return ISDF_ERR_HIP;
  for (int i = 0; i < nset; ++i) {
    for (int64_t g0 = 0; g0 < ng; g0 += RCHUNK) {
      const int64_t nc = std::min(RCHUNK, ng - g0);
      int rc = gemm_rm(h, 'N', 'N', nA, nc, nB, 1.0, d_dm + (int64_t)i * nA * nB, nB, d_aoB + g0, ld, 0.0, T, RCHUNK);
      if (rc) return rc;
      ProfScope ps(h, "rho_pair_reduce_kernel[byte]", 16.0 * (double)nA * (double)nc);
      hipLaunchKernelGGL(rho_pair_reduce_kernel, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, h->stream, T, RCHUNK, d_aoA + g0, ld,
                         nA, nc, d_rho + (int64_t)i * ldrho + g0);
      KERNEL_CHECK(h);
    }
  }
  return ISDF_OK;
}

extern "C" int isdf_mg_embed_density(isdf_handle h, const double* d_field, int nset, const int32_t mesh_sub[3], double scale,
                                     double* d_spec, const int32_t mesh[3], int accumulate) {
  // spec[set] (+)= scale * embed(fft(field[set] on mesh_sub)) - half spectra, fields contiguous (nset, prod(mesh_sub))
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_field && d_spec && mesh_sub && mesh && nset > 0 && nset <= 65535 && mesh_fits(mesh_sub, mesh));
  const int n2h = mesh_sub[2] / 2 + 1, N2h = mesh[2] / 2 + 1;
  const int64_t gc = (int64_t)mesh_sub[0] * mesh_sub[1] * n2h;
  double2* Z = (double2*)isdf_ws(h, "mg_Z", sizeof(double2) * (size_t)nset * gc);
  if (!Z) return ISDF_ERR_HIP;
  FftPlan* plan = nullptr;
  int rc = isdf_get_plan(h, mesh_sub, nset, &plan);
  if (rc) return rc;
  const int64_t G = (int64_t)mesh_sub[0] * mesh_sub[1] * mesh_sub[2];
  ProfScope ps(h, "mg_d2z_embed[byte]", (8.0 * G + 16.0 * gc * 3) * nset, 2);
  FFT_TRY(h, hipfftExecD2Z(plan->fwd, (hipfftDoubleReal*)d_field, (hipfftDoubleComplex*)Z));
  hipLaunchKernelGGL(spectrum_embed_kernel, dim3((unsigned)cdiv(gc, 256), (unsigned)nset), dim3(256), 0, h->stream, Z, mesh_sub[0],
                     mesh_sub[1], n2h, mesh_sub[2], (double2*)d_spec, mesh[0], mesh[1], N2h, mesh[2], scale, accumulate);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_mg_restrict_potential(isdf_handle h, const double* d_spec, int nset, const int32_t mesh[3],
                                          const int32_t mesh_sub[3], double scale, double* d_field) {
  // field[set] = scale * ifft_unnormalised(restrict(spec[set]) to mesh_sub)   (Z2D; pass scale = 1 / prod(mesh_sub) for numpy's ifft)
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_field && d_spec && mesh_sub && mesh && nset > 0 && nset <= 65535 && mesh_fits(mesh_sub, mesh));
  const int n2h = mesh_sub[2] / 2 + 1, N2h = mesh[2] / 2 + 1;
  const int64_t gc = (int64_t)mesh_sub[0] * mesh_sub[1] * n2h;
  double2* Z = (double2*)isdf_ws(h, "mg_Z", sizeof(double2) * (size_t)nset * gc);
  if (!Z) return ISDF_ERR_HIP;
  FftPlan* plan = nullptr;
  int rc = isdf_get_plan(h, mesh_sub, nset, &plan);
  if (rc) return rc;
  const int64_t G = (int64_t)mesh_sub[0] * mesh_sub[1] * mesh_sub[2];
  ProfScope ps(h, "mg_restrict_z2d[byte]", (8.0 * G + 16.0 * gc * 3) * nset, 2);
  hipLaunchKernelGGL(spectrum_restrict_kernel, dim3((unsigned)cdiv(gc, 256), (unsigned)nset), dim3(256), 0, h->stream,
                     (const double2*)d_spec, mesh[0], mesh[1], N2h, mesh[2], Z, mesh_sub[0], mesh_sub[1], n2h, mesh_sub[2], scale);
  KERNEL_CHECK(h);
  FFT_TRY(h, hipfftExecZ2D(plan->bwd, (hipfftDoubleComplex*)Z, (hipfftDoubleReal*)d_field));
  return ISDF_OK;
}

extern "C" int isdf_mg_coulomb_kernel(isdf_handle h, double* d_spec, int nset, const int32_t mesh[3], const double a[9]) {
  // spec[set] *= coulG (the handle's kernel: 4 pi / G^2 with its range-separation / truncation state, G = 0 -> 0)
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_spec && mesh && a && nset > 0 && nset <= 65535 && mesh[0] > 0 && mesh[1] > 0 && mesh[2] > 0);
  const int64_t G = (int64_t)mesh[0] * mesh[1] * mesh[2];
  const int64_t gc = (int64_t)mesh[0] * mesh[1] * (mesh[2] / 2 + 1);
  double* cg = nullptr;
  int rc = get_coulG_half(h, mesh, a, (double)G, &cg);   // the table carries 1/G by default; undo it
  if (rc) return rc;
  hipLaunchKernelGGL(spectrum_scale_kernel, dim3((unsigned)cdiv(gc, 256), (unsigned)nset), dim3(256), 0, h->stream, (double2*)d_spec,
                     cg, gc);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_lda_exchange(isdf_handle h, const double* d_rho, int64_t n, double* d_exc, double* d_vxc) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_rho && d_exc && d_vxc && n > 0);
  hipLaunchKernelGGL(lda_exchange_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_rho, n, d_exc, d_vxc);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_lda_vwn_add(isdf_handle h, const double* d_rho, int64_t n, double* d_exc, double* d_vxc) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_rho && d_exc && d_vxc && n > 0);
  hipLaunchKernelGGL(lda_vwn_add_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_rho, n, d_exc, d_vxc);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_gga_b88(isdf_handle h, const double* d_rho, const double* d_grad, int64_t gstride, int64_t n, double* d_exc,
                            double* d_vrho, double* d_w, int64_t wstride) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_rho && d_grad && d_exc && d_vrho && d_w && n > 0 && gstride >= n && wstride >= n);
  ProfScope ps(h, "gga_b88_kernel[byte]", 72.0 * (double)n);
  hipLaunchKernelGGL(gga_b88_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_rho, d_grad, gstride, n, d_exc,
                     d_vrho, d_w, wstride);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_xc_fused(isdf_handle h, const double* d_rho, const double* d_grad, int64_t gstride, int64_t n, double c_slater,
                             double c_b88, double c_vwn, int vwn_rpa, double c_lyp, double* d_exc, double* d_vrho, double* d_w,
                             int64_t wstride) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_rho && d_grad && d_exc && d_vrho && d_w && n > 0 && gstride >= n && wstride >= n && (vwn_rpa == 0 || vwn_rpa == 1));
  ProfScope ps(h, "xc_fused_kernel[byte]", 72.0 * (double)n);
  hipLaunchKernelGGL(xc_fused_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_rho, d_grad, gstride, n, c_slater, c_b88,
                     c_vwn, vwn_rpa, c_lyp, d_exc, d_vrho, d_w, wstride);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_xc_fused_rsh(isdf_handle h, const double* d_rho, const double* d_grad, int64_t gstride, int64_t n, double c_slater,
                                 double c_b88, double c_vwn, int vwn_rpa, double c_lyp, double c_b88_sr, double omega, double* d_exc,
                                 double* d_vrho, double* d_w, int64_t wstride) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_rho && d_grad && d_exc && d_vrho && d_w && n > 0 && gstride >= n && wstride >= n && (vwn_rpa == 0 || vwn_rpa == 1) &&
                   omega >= 0.0 && std::isfinite(omega));
  ProfScope ps(h, "xc_fused_rsh_kernel[byte]", 72.0 * (double)n);
  hipLaunchKernelGGL(xc_fused_rsh_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_rho, d_grad, gstride, n, c_slater,
                     c_b88, c_vwn, vwn_rpa, c_lyp, c_b88_sr, omega, d_exc, d_vrho, d_w, wstride);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_gga_lyp_polarised(isdf_handle h, const double* d_rho, const double* d_grad, int64_t gcstride, int64_t sstride,
                                      int64_t n, double weight, int accumulate, double* d_ec, double* d_vrho, double* d_w,
                                      int64_t wcstride, int64_t osstride) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_rho && d_grad && d_ec && d_vrho && d_w && n > 0 && gcstride >= n && sstride >= n && wcstride >= n && osstride >= n);
  ProfScope ps(h, "lyp_polarised_kernel[byte]", 8.0 * (double)n * (17.0 + (accumulate ? 8.0 : 0.0)));
  hipLaunchKernelGGL(lyp_polarised_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_rho, d_grad, gcstride, sstride, n,
                     weight, accumulate, d_ec, d_vrho, d_w, wcstride, osstride);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_lda_exchange_fxc(isdf_handle h, const double* d_rho, int64_t n, double* d_fxc) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_rho && d_fxc && n > 0);
  hipLaunchKernelGGL(lda_exchange_fxc_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_rho, n, d_fxc);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_lda_vwn_fxc_add(isdf_handle h, const double* d_rho, int64_t n, double* d_fxc) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_rho && d_fxc && n > 0);
  hipLaunchKernelGGL(lda_vwn_fxc_add_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_rho, n, d_fxc);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_gga_b88_fxc(isdf_handle h, const double* d_rho0, int64_t r0stride, int64_t n, const double* d_rho1,
                                int64_t r1xstride, int64_t r1nstride, int nset, double* d_wv, int64_t wxstride, int64_t wnstride,
                                double* d_fxc, int64_t fstride) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_rho0 && n > 0 && r0stride >= n && nset >= 0 && (nset > 0 || d_fxc));
  ARG_CHECK(h, nset == 0 || (d_rho1 && d_wv && r1xstride > 0 && r1nstride > 0 && wxstride > 0 && wnstride > 0));
  ARG_CHECK(h, !d_fxc || fstride >= n);
  ProfScope ps(h, "gga_b88_fxc_kernel[byte]", 8.0 * (double)n * (4.0 + 8.0 * nset + (d_fxc ? 10.0 : 0.0)));
  hipLaunchKernelGGL(gga_b88_fxc_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, h->stream, d_rho0, r0stride, n, d_rho1,
                     r1xstride, r1nstride, nset, d_wv, wxstride, wnstride, d_fxc, fstride);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_xc_fxc_apply(isdf_handle h, int nx, const double* d_fxc, int64_t fxstride, int64_t fystride, int64_t n,
                                 const double* d_rho1, int64_t r1xstride, int64_t r1nstride, int nset, double* d_wv, int64_t wxstride,
                                 int64_t wnstride, int accumulate) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, (nx == 1 || nx == 4) && d_fxc && d_rho1 && d_wv && n > 0 && nset > 0);
  ARG_CHECK(h, (nx == 1 || (fxstride > 0 && fystride > 0)) && r1nstride > 0 && wnstride > 0 && (nx == 1 || (r1xstride > 0 && wxstride > 0)));
  const dim3 grid((unsigned)cdiv(n, 256)), block(256);
  if (nx == 1)
    hipLaunchKernelGGL(xc_fxc_apply_kernel<1>, grid, block, 0, h->stream, d_fxc, fxstride, fystride, n, d_rho1, r1xstride, r1nstride,
                       nset, d_wv, wxstride, wnstride, accumulate);
  else
    hipLaunchKernelGGL(xc_fxc_apply_kernel<4>, grid, block, 0, h->stream, d_fxc, fxstride, fystride, n, d_rho1, r1xstride, r1nstride,
                       nset, d_wv, wxstride, wnstride, accumulate);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

extern "C" int isdf_dot(isdf_handle h, const double* d_x, const double* d_y, int64_t n, double* result) {
  // *result = sum_i x_i y_i (d_y NULL: sum_i x_i); fixed reduction order; synchronises the work stream
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_x && result && n > 0);
  const int nb = (int)std::min<int64_t>(cdiv(n, 256), 1024);
  double* part = (double*)isdf_ws(h, "dot_partial", sizeof(double) * 1025);
  if (!part) return ISDF_ERR_HIP;
  hipLaunchKernelGGL(dot_partial_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, d_x, d_y, n, part);
  hipLaunchKernelGGL(dot_final_kernel, dim3(1), dim3(256), 0, h->stream, part, nb, part + 1024);
  KERNEL_CHECK(h);
  HIP_TRY(h, hipMemcpyAsync(result, part + 1024, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return ISDF_OK;
}
