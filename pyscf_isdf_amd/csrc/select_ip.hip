// S2: interpolation-point selection — pivoted Cholesky of the implicit pair-density Gram matrix
// A(r,r') = (sum_mu ao[mu,r] ao[mu,r'])^2, batched over independent column blocks of ao.
//
// Left-looking, one pivot per step for every block at once.  Per step three launches:
//   find_first   every workgroup scans its slice of the residual diagonal d for the LOWEST index with
//                d >= (1 - tie_rtol) * blockmax  -> atomicMin into the block's candidate slot
//   take_pivot   one workgroup per block: records the pivot, decides termination, gathers the pivot's
//                AO column pv[nao] and its previous Cholesky entries pl[j] into contiguous scratch,
//                re-arms the block's max/argmin slots
//   update       every lane owns one grid point i:  s = sum_mu ao[mu,i] pv[mu]  (coalesced along the
//                grid), col = s^2 - sum_{t<j} L[t,i] pl[t], L[j,i] = col / sqrt(d_p), d[i] -= L[j,i]^2,
//                and the workgroup's max of the new d goes to the block's slot by atomicMax
// pv/pl are staged in LDS (panel of the factorisation) and broadcast to the lanes.
// The stream of ao (nao x m) and of the growing L (j x m) is the HBM cost: 8*(nao + j)*m bytes/step.
// Pivot rule: pyscf/lib/scipy_helper.py:71-110 plus the deterministic tie rule of mi355_isdf.h.
//
// Gram form (isdf_select_ip_ws with a workspace, real mode): the dot products s of all pivots of a block are entries of
// S_b = ao_b^T ao_b, so the block-lower triangles of a group of blocks are formed once on the matrix cores
// (gram_tri_blocks, gemm_f64.hip: one K slab, k ascending from a zero accumulator = the same fma chain, bit for bit) and
// update reads s = S_b[p, i] instead of streaming ao: 8*(j + 4)*m bytes/step.  Everything after s is the same code.
#include "common.h"
#include <cfloat>
#include <climits>

namespace {

constexpr int TPB = 256;

struct BlkState {
  unsigned long long dmax_bits;   // max residual diagonal of the block (bit pattern of a double >= 0)
  long long cand;                 // lowest local index within tolerance of the max (LLONG_MAX = none)
  double dp;                      // sqrt(d[pivot]) of the current step
  double tol;
  long long pivot;                // local index of the current pivot
  int done;
  int rank;
};

__device__ inline double wave_max_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ inline long long wave_min_ll(long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    long long u = __shfl_xor(v, o);
    v = u < v ? u : v;
  }
  return v;
}

// d[i] = (sum_mu ao[mu,i]^2)^2 ; block max -> state
__global__ __launch_bounds__(TPB) void init_diag_kernel(
    const double* __restrict__ ao, int nao, int64_t ld, const int* __restrict__ wg_blk,
    const int64_t* __restrict__ wg_lo, const int64_t* __restrict__ blk_off, double* __restrict__ d,
    BlkState* __restrict__ st) {
  __shared__ double red[TPB / 64];
  const int b = wg_blk[blockIdx.x];
  const int64_t i = wg_lo[blockIdx.x] + threadIdx.x;
  const bool valid = i < blk_off[b + 1];
  double s = 0.0;
  if (valid) {
    const double* __restrict__ p = ao + i;
#pragma unroll 8
    for (int mu = 0; mu < nao; ++mu) {
      const double v = p[(int64_t)mu * ld];
      s = fma(v, v, s);
    }
    s = s * s;
    d[i] = s;
  }
  double m = wave_max_d(valid ? s : 0.0);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TPB / 64; ++w) m = fmax(m, red[w]);
    atomicMax(&st[b].dmax_bits, (unsigned long long)__double_as_longlong(m));
  }
}

__global__ __launch_bounds__(TPB) void find_first_kernel(
    const double* __restrict__ d, const int* __restrict__ wg_blk, const int64_t* __restrict__ wg_lo,
    const int64_t* __restrict__ blk_off, BlkState* __restrict__ st, double tie_rtol) {
  __shared__ long long red[TPB / 64];
  const int b = wg_blk[blockIdx.x];
  if (st[b].done) return;
  const int64_t i = wg_lo[blockIdx.x] + threadIdx.x;
  const double dmax = __longlong_as_double((long long)st[b].dmax_bits);
  const double thr = dmax * (1.0 - tie_rtol);
  long long c = LLONG_MAX;
  if (i < blk_off[b + 1] && d[i] >= thr && d[i] > 0.0) c = i - blk_off[b];
  c = wave_min_ll(c);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TPB / 64; ++w) c = red[w] < c ? red[w] : c;
    if (c != LLONG_MAX) atomicMin(&st[b].cand, c);
  }
}

// one workgroup per block
__global__ __launch_bounds__(TPB) void take_pivot_kernel(
    const double* __restrict__ ao, int nao, int64_t ld, const double* __restrict__ L, int64_t ldL,
    const double* __restrict__ d, const int64_t* __restrict__ blk_off, const int* __restrict__ nip,
    int j, double tol_in, int kmax, BlkState* __restrict__ st, int64_t* __restrict__ piv,
    double* __restrict__ pv, double* __restrict__ pl, int nh, double* __restrict__ pvr, int b0) {
  const int b = b0 + blockIdx.x;   // ao == nullptr (Gram form): no pivot column to gather
  BlkState s = st[b];
  if (s.done) return;
  const double dmax = __longlong_as_double((long long)s.dmax_bits);
  const int64_t m = blk_off[b + 1] - blk_off[b];
  double tol = s.tol;
  if (j == 0) tol = tol_in < 0 ? (double)m * DBL_EPSILON * dmax : tol_in;
  const bool stop = (j >= nip[b]) || !(dmax > tol) || s.cand == LLONG_MAX;
  __syncthreads();
  if (stop) {
    if (threadIdx.x == 0) { st[b].done = 1; st[b].tol = tol; }
    return;
  }
  const int64_t p = blk_off[b] + s.cand;
  if (ao)
    for (int mu = threadIdx.x; mu < nao; mu += TPB) pv[(int64_t)b * nao + mu] = ao[(int64_t)mu * ld + p];
  if (nh > 0)   // rotated pivot vector [Im u_p ; -Re u_p] for the imaginary part of S
    for (int mu = threadIdx.x; mu < nao; mu += TPB)
      pvr[(int64_t)b * nao + mu] = (mu < nh) ? ao[(int64_t)(nh + mu) * ld + p] : -ao[(int64_t)(mu - nh) * ld + p];
  for (int t = threadIdx.x; t < j; t += TPB) pl[(int64_t)b * kmax + t] = L[(int64_t)t * ldL + p];
  if (threadIdx.x == 0) {
    piv[(int64_t)b * kmax + j] = s.cand;
    st[b].pivot = s.cand;
    st[b].dp = sqrt(d[p]);
    st[b].tol = tol;
    st[b].rank = j + 1;
    st[b].dmax_bits = 0ull;
    st[b].cand = LLONG_MAX;
  }
}

// GRAM: ao is the base of the group's Gram triangles, tri_off[b] the offset of block b's (layout: gram_tri_row, common.h);
// the panel is pl[j] alone and nh is 0
template <bool LDS_PANEL, bool GRAM>
__global__ __launch_bounds__(TPB) void update_kernel(
    const double* __restrict__ ao, int nao, int64_t ld, double* __restrict__ L, int64_t ldL,
    double* __restrict__ d, const int* __restrict__ wg_blk, const int64_t* __restrict__ wg_lo,
    const int64_t* __restrict__ blk_off, int j, int kmax, BlkState* __restrict__ st,
    const double* __restrict__ pv, const double* __restrict__ pl, int nh, const double* __restrict__ pvr,
    const int64_t* __restrict__ tri_off) {
  // nh > 0: complex mode, rows [0,nh) = Re u, rows [nh,2nh) = Im u (nao = 2 nh):
  //   S(p,i) = sum conj(u_p) u_i,  Re S = sum_m X[m,i] pv[m],  Im S = sum_m X[m,i] pvr[m],
  //   pvr = [Im u_p ; -Re u_p];  Gram entry = Re^2 + Im^2.
  extern __shared__ double panel[];   // pv[nao] | pl[j] (| pvr[nao] in complex mode)
  __shared__ double red[TPB / 64];
  const int b = wg_blk[blockIdx.x];
  if (st[b].done) return;
  // the pivot panel (pv | pl | pvr) is broadcast to all lanes: from LDS when it fits, otherwise straight
  // from global memory (wave-uniform addresses, L2 resident) — the k-point mode with many AOs
  const double* s_pv;
  const double* s_pl;
  const double* s_pvr;
  if (LDS_PANEL) {
    double* w_pv = panel;
    double* w_pl = panel + (GRAM ? 0 : nao);
    double* w_pvr = w_pl + j;
    if (!GRAM)
      for (int mu = threadIdx.x; mu < nao; mu += TPB) w_pv[mu] = pv[(int64_t)b * nao + mu];
    for (int t = threadIdx.x; t < j; t += TPB) w_pl[t] = pl[(int64_t)b * kmax + t];
    if (nh > 0)
      for (int mu = threadIdx.x; mu < nao; mu += TPB) w_pvr[mu] = pvr[(int64_t)b * nao + mu];
    __syncthreads();
    s_pv = w_pv; s_pl = w_pl; s_pvr = w_pvr;
  } else {
    s_pv = pv + (int64_t)b * nao;
    s_pl = pl + (int64_t)b * kmax;
    s_pvr = pvr + (int64_t)b * nao;
  }
  const int64_t i = wg_lo[blockIdx.x] + threadIdx.x;
  const bool valid = i < blk_off[b + 1];
  double dnew = 0.0;
  if (valid) {
    const double dp = st[b].dp;
    const int64_t ploc = blk_off[b] + st[b].pivot;
    const double dold = d[i];
    double row;
    if (i == ploc) {
      row = dp;
      dnew = -1.0;
    } else if (dold < 0.0) {       // an earlier pivot: residual row is exactly zero
      row = 0.0;
      dnew = -1.0;
    } else {
      const double* __restrict__ pa = ao + i;
      double s0 = 0.0, s1 = 0.0;
      if (GRAM) {
        // the pivot's own row where the stored triangle holds it (up to the end of the pivot's tile row), else the mirror
        // entry of row i: equal to the last bit (same products, same k order)
        const int64_t il = i - blk_off[b], pl_ = st[b].pivot;
        const double* __restrict__ S = ao + tri_off[b];
        s0 = il < (((pl_ >> 8) + 1) << 8) ? S[gram_tri_row(pl_) + il] : S[gram_tri_row(il) + pl_];
      } else if (nh > 0) {
#pragma unroll 8
        for (int mu = 0; mu < nao; ++mu) {
          const double x = pa[(int64_t)mu * ld];
          s0 = fma(x, s_pv[mu], s0);
          s1 = fma(x, s_pvr[mu], s1);
        }
      } else {
#pragma unroll 8
        for (int mu = 0; mu < nao; ++mu) s0 = fma(pa[(int64_t)mu * ld], s_pv[mu], s0);
      }
      double col = fma(s1, s1, s0 * s0);
      const double* __restrict__ pL = L + i;
#pragma unroll 8
      for (int t = 0; t < j; ++t) col = fma(-pL[(int64_t)t * ldL], s_pl[t], col);
      row = col / dp;
      dnew = fma(-row, row, dold);
      if (dnew < 0.0) dnew = 0.0;   // rounding can push an exhausted point below zero; keep it alive-but-empty
    }
    L[(int64_t)j * ldL + i] = row;
    d[i] = dnew;
  }
  double m = wave_max_d(valid ? fmax(dnew, 0.0) : 0.0);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TPB / 64; ++w) m = fmax(m, red[w]);
    atomicMax(&st[b].dmax_bits, (unsigned long long)__double_as_longlong(m));
  }
}

}  // namespace

namespace {
// owner[g] = the atom nearest to grid point g under the minimum-image convention (the 27 neighbouring images of every atom);
// among atoms within tie_atol of the smallest distance the LOWEST index wins (symmetric crystals put many points exactly
// between atoms).  Atom positions and the 27 lattice shifts sit in LDS; one grid point per lane, two sweeps over the atoms.
__global__ __launch_bounds__(256) void partition_kernel(const double* __restrict__ coords, int64_t G, const double* __restrict__ atoms,
                                                        int natm, const double* __restrict__ shifts, double tie_atol,
                                                        int32_t* __restrict__ owner) {
  extern __shared__ double sm[];            // atoms (3 natm) | shifts (81)
  double* s_at = sm;
  double* s_sh = sm + 3 * natm;
  for (int t = threadIdx.x; t < 3 * natm; t += 256) s_at[t] = atoms[t];
  for (int t = threadIdx.x; t < 81; t += 256) s_sh[t] = shifts[t];
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const double x = coords[g], y = coords[G + g], z = coords[2 * G + g];
  double dmin = 1e300;
  for (int a = 0; a < natm; ++a) {
    const double ax = x - s_at[3 * a], ay = y - s_at[3 * a + 1], az = z - s_at[3 * a + 2];
    double d2 = 1e300;
    for (int t = 0; t < 27; ++t) {
      const double dx = ax - s_sh[3 * t], dy = ay - s_sh[3 * t + 1], dz = az - s_sh[3 * t + 2];
      d2 = fmin(d2, dx * dx + dy * dy + dz * dz);
    }
    dmin = fmin(dmin, sqrt(d2));
  }
  int own = natm;
  for (int a = 0; a < natm && own == natm; ++a) {
    const double ax = x - s_at[3 * a], ay = y - s_at[3 * a + 1], az = z - s_at[3 * a + 2];
    double d2 = 1e300;
    for (int t = 0; t < 27; ++t) {
      const double dx = ax - s_sh[3 * t], dy = ay - s_sh[3 * t + 1], dz = az - s_sh[3 * t + 2];
      d2 = fmin(d2, dx * dx + dy * dy + dz * dz);
    }
    if (sqrt(d2) <= dmin + tie_atol) own = a;
  }
  owner[g] = own;
}
}  // namespace

extern "C" int isdf_partition_by_atom(isdf_handle h, const double* d_coords, int64_t ngrids, const double* atom_coords, int natm,
                                      const double a[9], double tie_atol, int32_t* d_owner) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, d_coords && atom_coords && a && d_owner && ngrids > 0 && natm > 0 && natm <= 2000 && tie_atol >= 0.0);
  std::vector<double> host(3 * (size_t)natm + 81);
  for (int i = 0; i < 3 * natm; ++i) host[i] = atom_coords[i];
  int t = 0;
  for (int i = -1; i <= 1; ++i)
    for (int j = -1; j <= 1; ++j)
      for (int k = -1; k <= 1; ++k, ++t)
        for (int c = 0; c < 3; ++c) host[3 * natm + 3 * t + c] = i * a[c] + j * a[3 + c] + k * a[6 + c];
  double* d_tab = (double*)isdf_ws(h, "partition_tab", sizeof(double) * host.size());
  if (!d_tab) return ISDF_ERR_HIP;
  HIP_TRY(h, hipMemcpyAsync(d_tab, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  ProfScope ps(h, "partition_kernel[byte]", 28.0 * (double)ngrids);
  hipLaunchKernelGGL(partition_kernel, dim3((unsigned)cdiv(ngrids, 256)), dim3(256), sizeof(double) * host.size(), h->stream,
                     d_coords, ngrids, d_tab, natm, d_tab + 3 * natm, tie_atol, d_owner);
  KERNEL_CHECK(h);
  return ISDF_OK;
}

namespace {

int64_t gram_kpad(int nao) { return cdiv(nao, 32) * 32; }   // the Gram product's K: zero padded to whole chunk pairs

// Blocks [b0, b1) whose Gram triangles and transposed AO rows share the workspace; workgroups [w0, w1), units [u0, u1)
struct BlkGroup { int b0, b1, w0, w1, kmax; int64_t u0, u1; };

int select_blocks(isdf_handle h, const double* d_ao, int nao, int nh, int64_t ld, int nblk,
                  const int64_t* blk_off, const int32_t* nip, double tol, double tie_rtol, double* d_L,
                  int64_t ldL, int64_t* d_piv, int32_t* rank, void* d_work, int64_t work_bytes) {
  if (!h) return ISDF_ERR_ARG;
  ARG_CHECK(h, nh == 0 || 2 * nh == nao);
  ARG_CHECK(h, d_ao && blk_off && nip && d_L && d_piv && rank);
  ARG_CHECK(h, nao > 0 && nblk > 0 && tie_rtol >= 0.0 && tie_rtol < 1.0);
  const int64_t mtot = blk_off[nblk];
  ARG_CHECK(h, blk_off[0] == 0 && mtot > 0 && ld >= mtot && ldL >= mtot);
  int kmax = 0;
  std::vector<int> h_wg_blk, h_wg_first(nblk + 1);
  std::vector<int64_t> h_wg_lo;
  for (int b = 0; b < nblk; ++b) {
    ARG_CHECK(h, blk_off[b + 1] >= blk_off[b] && nip[b] >= 0);
    if (nip[b] > kmax) kmax = nip[b];
    h_wg_first[b] = (int)h_wg_blk.size();
    for (int64_t lo = blk_off[b]; lo < blk_off[b + 1]; lo += TPB) {
      h_wg_blk.push_back(b);
      h_wg_lo.push_back(lo);
    }
  }
  ARG_CHECK(h, kmax > 0);
  const int nwg = (int)h_wg_blk.size();
  h_wg_first[nblk] = nwg;

  // Gram form: consecutive blocks are grouped greedily into what the workspace holds (triangles, then the group's AO rows
  // transposed to K-contiguous); one block that does not fit sends the whole call down the AO path
  std::vector<BlkGroup> groups;
  std::vector<GramTriUnit> h_units;
  std::vector<int64_t> h_tri_off(nblk, 0);
  const int kpad = (int)gram_kpad(nao);
  char* work = (char*)(((uintptr_t)d_work + 255) / 256 * 256);
  const int64_t avail = d_work ? (work_bytes - (int64_t)(work - (char*)d_work)) / 8 : 0;   // doubles
  bool gram = nh == 0 && h->cand_gram && avail > 0;
  if (gram) {
    BlkGroup g{0, 0, 0, 0, 0, 0, 0};
    int64_t used = 0, tri = 0;
    for (int b = 0; b < nblk && gram; ++b) {
      const int64_t m = blk_off[b + 1] - blk_off[b];
      const int64_t need = gram_tri_size(m) + m * kpad;
      if (need > avail) { gram = false; break; }
      if (used + need > avail) {
        g.b1 = b; g.u1 = (int64_t)h_units.size();
        groups.push_back(g);
        g = BlkGroup{b, b, 0, 0, 0, g.u1, g.u1};
        used = tri = 0;
      }
      h_tri_off[b] = tri;
      tri += gram_tri_size(m);
      used += need;
      if (nip[b] > g.kmax) g.kmax = nip[b];
      if (nip[b] > 0)   // a block that takes no pivot needs no triangle
        for (int tm = 0; tm < (int)cdiv(m, 256); ++tm)
          for (int tn = 0; tn <= 2 * tm + 1 && (int64_t)tn * 128 < m; ++tn) h_units.push_back(GramTriUnit{b, tm, tn, 0});
    }
    g.b1 = nblk; g.u1 = (int64_t)h_units.size();
    groups.push_back(g);
  }
  if (!gram) {
    groups.assign(1, BlkGroup{0, nblk, 0, 0, kmax, 0, 0});
    h_units.clear();
  }
  for (auto& g : groups) { g.w0 = h_wg_first[g.b0]; g.w1 = h_wg_first[g.b1]; }

  const size_t panel_bytes = sizeof(double) * (gram ? (size_t)kmax : (size_t)nao * (nh > 0 ? 2 : 1) + kmax);
  const bool lds_panel = panel_bytes <= 64 * 1024;

  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t b_d = al(sizeof(double) * mtot), b_st = al(sizeof(BlkState) * nblk);
  const size_t b_wb = al(sizeof(int) * nwg), b_wl = al(sizeof(int64_t) * nwg);
  const size_t b_off = al(sizeof(int64_t) * (nblk + 1)), b_nip = al(sizeof(int) * nblk);
  const size_t b_pv = al(sizeof(double) * (size_t)nblk * nao) * 2, b_pl = al(sizeof(double) * (size_t)nblk * kmax);
  const size_t b_tri = al(sizeof(int64_t) * nblk), b_un = al(sizeof(GramTriUnit) * h_units.size());
  char* ws = (char*)isdf_ws(h, "select", b_d + b_st + b_wb + b_wl + b_off + b_nip + b_pv + b_pl + b_tri + b_un);
  if (!ws) return ISDF_ERR_HIP;
  double* d_d = (double*)ws; ws += b_d;
  BlkState* d_st = (BlkState*)ws; ws += b_st;
  int* d_wg_blk = (int*)ws; ws += b_wb;
  int64_t* d_wg_lo = (int64_t*)ws; ws += b_wl;
  int64_t* d_off = (int64_t*)ws; ws += b_off;
  int* d_nip = (int*)ws; ws += b_nip;
  double* d_pv = (double*)ws; ws += b_pv;
  double* d_pvr = d_pv + (size_t)nblk * nao;
  double* d_pl = (double*)ws; ws += b_pl;
  int64_t* d_tri_off = (int64_t*)ws; ws += b_tri;
  GramTriUnit* d_units = (GramTriUnit*)ws;

  std::vector<BlkState> h_st(nblk);
  for (auto& s : h_st) { s.dmax_bits = 0; s.cand = LLONG_MAX; s.dp = 0; s.tol = 0; s.pivot = -1; s.done = 0; s.rank = 0; }
  HIP_TRY(h, hipMemcpyAsync(d_st, h_st.data(), sizeof(BlkState) * nblk, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(d_wg_blk, h_wg_blk.data(), sizeof(int) * nwg, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(d_wg_lo, h_wg_lo.data(), sizeof(int64_t) * nwg, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(d_off, blk_off, sizeof(int64_t) * (nblk + 1), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(d_nip, nip, sizeof(int) * nblk, hipMemcpyHostToDevice, h->stream));
  if (gram) {
    HIP_TRY(h, hipMemcpyAsync(d_tri_off, h_tri_off.data(), sizeof(int64_t) * nblk, hipMemcpyHostToDevice, h->stream));
    if (!h_units.empty())
      HIP_TRY(h, hipMemcpyAsync(d_units, h_units.data(), sizeof(GramTriUnit) * h_units.size(), hipMemcpyHostToDevice, h->stream));
  }
  HIP_TRY(h, hipMemsetAsync(d_piv, 0xff, sizeof(int64_t) * (size_t)nblk * kmax, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));   // host staging vectors go out of scope below

  hipLaunchKernelGGL(init_diag_kernel, dim3(nwg), dim3(TPB), 0, h->stream, d_ao, nao, ld, d_wg_blk,
                     d_wg_lo, d_off, d_d, d_st);
  KERNEL_CHECK(h);
  for (const BlkGroup& g : groups) {
    const int gwg = g.w1 - g.w0, gblk = g.b1 - g.b0;
    const int64_t p0 = blk_off[g.b0], mg = blk_off[g.b1] - p0;
    if (gwg == 0) continue;
    const double* d_S = nullptr;
    if (gram && g.u1 > g.u0) {
      int64_t tri = 0;
      double flop = 0.0;
      for (int b = g.b0; b < g.b1; ++b) {
        const int64_t m = blk_off[b + 1] - blk_off[b];
        tri += gram_tri_size(m);
        if (nip[b] > 0) flop += (double)m * (m + 1) * nao;
      }
      double* d_X = (double*)work + tri;
      {
        ProfScope ps(h, "cand_gram_transpose[byte]", 16.0 * (double)mg * nao);
        if (kpad != nao) HIP_TRY(h, hipMemsetAsync(d_X, 0, sizeof(double) * (size_t)mg * kpad, h->stream));
        const int rc = transpose_rm(h, d_ao + p0, ld, nao, mg, d_X, kpad);
        if (rc != ISDF_OK) return rc;
      }
      const int rc = gram_tri_blocks(h, d_X, kpad, kpad, d_units + g.u0, g.u1 - g.u0, d_off, p0, d_tri_off, (double*)work, flop);
      if (rc != ISDF_OK) return rc;
      d_S = (const double*)work;
    }
    for (int j = 0; j <= g.kmax; ++j) {
      hipLaunchKernelGGL(find_first_kernel, dim3(gwg), dim3(TPB), 0, h->stream, d_d, d_wg_blk + g.w0, d_wg_lo + g.w0,
                         d_off, d_st, tie_rtol);
      hipLaunchKernelGGL(take_pivot_kernel, dim3(gblk), dim3(TPB), 0, h->stream, gram ? nullptr : d_ao, nao, ld, d_L, ldL,
                         d_d, d_off, d_nip, j, tol, kmax, d_st, d_piv, d_pv, d_pl, nh, d_pvr, g.b0);
      if (j == g.kmax) break;   // the last take_pivot only marks every block done
      if (gram) {
        ProfScope ps(h, "select_update_gram_kernel[byte]", 8.0 * (double)mg * (j + 4));
        if (lds_panel)
          hipLaunchKernelGGL((update_kernel<true, true>), dim3(gwg), dim3(TPB), sizeof(double) * (size_t)j, h->stream, d_S, nao, ld,
                             d_L, ldL, d_d, d_wg_blk + g.w0, d_wg_lo + g.w0, d_off, j, kmax, d_st, d_pv, d_pl, 0, d_pvr, d_tri_off);
        else
          hipLaunchKernelGGL((update_kernel<false, true>), dim3(gwg), dim3(TPB), 0, h->stream, d_S, nao, ld, d_L, ldL, d_d,
                             d_wg_blk + g.w0, d_wg_lo + g.w0, d_off, j, kmax, d_st, d_pv, d_pl, 0, d_pvr, d_tri_off);
        continue;
      }
      ProfScope ps(h, "select_update_kernel[byte]", 8.0 * (double)mtot * (nao + j + 3));
      if (lds_panel)
        hipLaunchKernelGGL((update_kernel<true, false>), dim3(gwg), dim3(TPB), sizeof(double) * ((size_t)nao * (nh > 0 ? 2 : 1) + j),
                           h->stream, d_ao, nao, ld, d_L, ldL, d_d, d_wg_blk + g.w0, d_wg_lo + g.w0, d_off, j, kmax, d_st, d_pv, d_pl,
                           nh, d_pvr, d_tri_off);
      else
        hipLaunchKernelGGL((update_kernel<false, false>), dim3(gwg), dim3(TPB), 0, h->stream, d_ao, nao, ld, d_L, ldL, d_d,
                           d_wg_blk + g.w0, d_wg_lo + g.w0, d_off, j, kmax, d_st, d_pv, d_pl, nh, d_pvr, d_tri_off);
    }
    KERNEL_CHECK(h);
  }
  HIP_TRY(h, hipMemcpyAsync(h_st.data(), d_st, sizeof(BlkState) * nblk, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int b = 0; b < nblk; ++b) rank[b] = h_st[b].rank;
  return ISDF_OK;
}

}  // namespace

extern "C" int isdf_select_ip(isdf_handle h, const double* d_ao, int nao, int64_t ld, int nblk,
                              const int64_t* blk_off, const int32_t* nip, double tol,
                              double tie_rtol, double* d_L, int64_t ldL, int64_t* d_piv,
                              int32_t* rank) {
  return isdf_select_ip_ws(h, d_ao, nao, ld, nblk, blk_off, nip, tol, tie_rtol, d_L, ldL, d_piv, rank, nullptr, 0);
}

extern "C" int isdf_select_ip_cplx(isdf_handle h, const double* d_ao, int nao, int nh, int64_t ld, int nblk,
                                   const int64_t* blk_off, const int32_t* nip, double tol,
                                   double tie_rtol, double* d_L, int64_t ldL, int64_t* d_piv,
                                   int32_t* rank) {
  return select_blocks(h, d_ao, nao, nh, ld, nblk, blk_off, nip, tol, tie_rtol, d_L, ldL, d_piv, rank, nullptr, 0);
}

extern "C" int isdf_select_ip_ws(isdf_handle h, const double* d_ao, int nao, int64_t ld, int nblk,
                                 const int64_t* blk_off, const int32_t* nip, double tol,
                                 double tie_rtol, double* d_L, int64_t ldL, int64_t* d_piv,
                                 int32_t* rank, void* d_work, int64_t work_bytes) {
  return select_blocks(h, d_ao, nao, 0, ld, nblk, blk_off, nip, tol, tie_rtol, d_L, ldL, d_piv, rank, d_work, work_bytes);
}

extern "C" int64_t isdf_select_ip_work_bytes(int nao, int64_t m) {
  if (nao <= 0 || m <= 0) return 0;
  return (int64_t)sizeof(double) * (gram_tri_size(m) + m * gram_kpad(nao));
}
