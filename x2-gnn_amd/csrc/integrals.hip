// Overlap and core-Hamiltonian blocks from geometry (include/x2g_integrals.h; reference scf.py:27-48, which takes
// pyscf's get_ovlp() and get_hcore() and never runs an SCF).  float64 throughout.
//
// McMurchie-Davidson.  For a primitive pair (exponents a, b; p = a + b; P the weighted centre) the product of two
// Cartesian Gaussians is expanded in Hermite Gaussians at P with the 1-D coefficients E^{ij}_t:
//   overlap   S = (pi/p)^{3/2} Ex_0 Ey_0 Ez_0
//   kinetic   from 1-D overlaps at j - 2, j, j + 2 (so the tables run to j = l_b + 2)
//   nuclear   V = -(2 pi / p) sum_tuv Ex_t Ey_u Ez_v G_tuv,   G_tuv = sum_C Z_C R_tuv(p, P - C)
// G depends on the primitive pair alone, so the nuclei are summed once per primitive pair and every Cartesian
// component of the shell pair reads the same table.  R_tuv is not built by its recursion, whose table every lane would
// have to hold privately, but from the derivative's closed form: with F_n the Boys function at x = p |P - C|^2,
//   R_tuv = sum_{k1,k2,k3} c(t,k1) c(u,k2) c(v,k3) X^{t-2k1} Y^{u-2k2} Z^{v-2k3} p^n F_n(x),  n = t+u+v-k1-k2-k3,
// c(t, k) = (-1)^{t+k} t! 2^{t-2k} / (k! (t-2k)!)  (the Hermite polynomial's coefficients), at most 8 terms.
//
// One single-wave workgroup takes every fourth shell pair of an atom pair.  Per primitive pair: 27 lanes (dimension x
// t) build the three E tables in LDS, one (i, j) step per barrier; the lanes then take one nucleus each for the Boys
// values F_0..F_L (into LDS), and one (t, u, v) each for G, looping over the nuclei in order; then one Cartesian
// component pair each (two for d-f, f-d, f-f) for S, T and V, accumulated over the contraction in registers.  Per shell
// pair the Cartesian block goes through LDS into the real solid harmonics and out to both (i, j) and (j, i).  A
// single-wave workgroup makes every barrier a wave-local one.  Tables indexed by a runtime l live in LDS, not in
// registers: no scratch.
#include "common.hpp"

#include "../../include/x2g_integrals.h"

namespace x2g {
namespace {

constexpr int kMaxL = 3;
constexpr int kMaxAo = 39;            // functions of an atom: the features' pad
constexpr int kSplit = 4;             // workgroups per atom pair
constexpr int kThreads = kWave;       // one wave
constexpr int kIDim = kMaxL + 1;      // E^{ij}_t: i <= l_a
constexpr int kJDim = kMaxL + 3;      //           j <= l_b + 2 (kinetic)
constexpr int kTDim = 2 * kMaxL + 3;  //           t <= i + j <= 8
constexpr int kETab = kIDim * kJDim * kTDim;
constexpr int kRDim = 2 * kMaxL + 1;  // t, u, v <= l_a + l_b
constexpr int kNuc = 4 + kRDim;       // per nucleus in LDS: P - C (3), Z, F_0..F_6
constexpr int kCartMax = 10;          // Cartesian components of an f shell
constexpr double kBoysSwitch = 20.0;  // below: series at n = L and downward recursion; from here: erf and upward
constexpr double kPi = 3.14159265358979323846;

// Cartesian components of l = 0..3, lexicographic; l's start at l (l + 1) (l + 2) / 6
__constant__ int kCartPow[20][3] = {{0, 0, 0},
                                    {1, 0, 0}, {0, 1, 0}, {0, 0, 1},
                                    {2, 0, 0}, {1, 1, 0}, {1, 0, 1}, {0, 2, 0}, {0, 1, 1}, {0, 0, 2},
                                    {3, 0, 0}, {2, 1, 0}, {2, 0, 1}, {1, 2, 0}, {1, 1, 1}, {1, 0, 2}, {0, 3, 0},
                                    {0, 2, 1}, {0, 1, 2}, {0, 0, 3}};

// real solid harmonics normalised over the sphere, as polynomials in the components above: [l][function][component];
// p as (x, y, z), d and f as m = -l .. l
#define S0 0.28209479177387814   /* sqrt(1 / 4 pi) */
#define P1 0.4886025119029199    /* sqrt(3 / 4 pi) */
#define D1 1.0925484305920792    /* sqrt(15 / 4 pi) */
#define D0 0.31539156525252005   /* sqrt(5 / 16 pi) */
#define D2 0.5462742152960396    /* sqrt(15 / 16 pi) */
#define F3 0.5900435899266435    /* sqrt(35 / 32 pi) */
#define F2 2.890611442640554     /* sqrt(105 / 4 pi) */
#define F1 0.4570457994644658    /* sqrt(21 / 32 pi) */
#define F0 0.3731763325901154    /* sqrt(7 / 16 pi) */
#define F2B 1.445305721320277    /* sqrt(105 / 16 pi) */
__constant__ double kC2S[kMaxL + 1][2 * kMaxL + 1][kCartMax] = {
    {{S0}},
    {{P1, 0, 0}, {0, P1, 0}, {0, 0, P1}},
    //  xx   xy  xz   yy   yz  zz
    {{0, D1, 0, 0, 0, 0},
     {0, 0, 0, 0, D1, 0},
     {-D0, 0, 0, -D0, 0, 2 * D0},
     {0, 0, D1, 0, 0, 0},
     {D2, 0, 0, -D2, 0, 0}},
    //  xxx  xxy  xxz  xyy  xyz  xzz  yyy  yyz  yzz  zzz
    {{0, 3 * F3, 0, 0, 0, 0, -F3, 0, 0, 0},
     {0, 0, 0, 0, F2, 0, 0, 0, 0, 0},
     {0, -F1, 0, 0, 0, 0, -F1, 0, 4 * F1, 0},
     {0, 0, -3 * F0, 0, 0, 0, 0, -3 * F0, 0, 2 * F0},
     {-F1, 0, 0, -F1, 0, 4 * F1, 0, 0, 0, 0},
     {0, 0, F2B, 0, 0, 0, 0, -F2B, 0, 0},
     {F3, 0, 0, -3 * F3, 0, 0, 0, 0, 0, 0}}};
#undef S0
#undef P1
#undef D1
#undef D0
#undef D2
#undef F3
#undef F2
#undef F1
#undef F0
#undef F2B

// c(t, k) of the header comment
__constant__ double kHerm[kRDim][4] = {{1, 0, 0, 0},       {-2, 0, 0, 0},        {4, -2, 0, 0},         {-8, 12, 0, 0},
                                       {16, -48, 12, 0},   {-32, 160, -120, 0},  {64, -480, 720, -120}};

struct IntArgs {
  const int32_t* elem_shell;
  const int32_t* shell_l;
  const int32_t* shell_prim;
  const int32_t* shell_ao;
  const double* prim_exp;
  const double* prim_coef;
  const double* pos;
  const int32_t* charge;
  const int32_t* atom_elem;
  const int32_t* atom_mol;
  const int32_t* ao_begin;
  const int64_t* atom_start;
  const int64_t* mat_start;
  const int32_t* mol_nao;
  const int64_t* pairs;
  double* ovlp;
  double* hcore;
  int64_t n_elem, num_mols, num_atoms, mat_elems, num_pairs;
};

__device__ __forceinline__ int ncart(int l) { return (l + 1) * (l + 2) / 2; }
__device__ __forceinline__ int eidx(int i, int j, int t) { return (i * kJDim + j) * kTDim + t; }
__device__ __forceinline__ int gidx(int t, int u, int v) { return (t * kRDim + u) * kRDim + v; }

__device__ __forceinline__ double ipow(double b, int e) {
  double r = 1.0;
  for (int i = 0; i < e; ++i) r *= b;
  return r;
}

// F_0..F_nmax at x >= 0 into F.  x < kBoysSwitch: F_nmax = exp(-x) sum_k (2x)^k / ((2n+1)(2n+3)..(2n+2k+1)), every
// term positive, then F_{n-1} = (2x F_n + exp(-x)) / (2n - 1), which is stable downward.  Otherwise
// F_0 = sqrt(pi / x) erf(sqrt x) / 2 and F_{n+1} = ((2n+1) F_n - exp(-x)) / 2x, which is stable upward once
// exp(-x) is small against (2n+1) F_n: at x = 20 and n = 6 the ratio is 2e-4.
__device__ void boys(double x, int nmax, double* F) {
  const double ex = exp(-x);
  if (x < kBoysSwitch) {
    double term = 1.0 / (2 * nmax + 1), sum = term;
    for (int k = 1; k < 400; ++k) {
      term *= 2.0 * x / (2 * nmax + 2 * k + 1);
      sum += term;
      if (term < 1e-17 * sum) break;
    }
    double f = ex * sum;
    F[nmax] = f;
    for (int n = nmax; n > 0; --n) {
      f = (2.0 * x * f + ex) / (2 * n - 1);
      F[n - 1] = f;
    }
  } else {
    const double sx = sqrt(x);
    double f = 0.5 * 1.7724538509055160273 / sx * erf(sx);
    F[0] = f;
    for (int n = 0; n < nmax; ++n) {
      f = ((2 * n + 1) * f - ex) / (2.0 * x);
      F[n + 1] = f;
    }
  }
}

// R_tuv(p, (X, Y, Z)) from F_n, the closed form of the header comment
__device__ double r_tuv(int t, int u, int v, double p, double X, double Y, double Z, const double* F) {
  const double pX = p * X, pY = p * Y, pZ = p * Z;
  double r = 0.0;
  for (int k1 = 0; 2 * k1 <= t; ++k1) {
    const double hx = kHerm[t][k1] * ipow(pX, t - 2 * k1) * ipow(p, k1);
    for (int k2 = 0; 2 * k2 <= u; ++k2) {
      const double hy = hx * (kHerm[u][k2] * ipow(pY, u - 2 * k2) * ipow(p, k2));
      for (int k3 = 0; 2 * k3 <= v; ++k3) {
        const double hz = kHerm[v][k3] * ipow(pZ, v - 2 * k3) * ipow(p, k3);
        r += hy * hz * F[t + u + v - k1 - k2 - k3];
      }
    }
  }
  return r;
}

// the q-th (t, u, v) with t + u + v <= L, t outermost; false when there is none
__device__ bool tuv_of(int q, int L, int* t, int* u, int* v) {
  if (q >= (L + 1) * (L + 2) * (L + 3) / 6) return false;
  int tt = 0;
  for (;; ++tt) {
    const int cnt = (L - tt + 1) * (L - tt + 2) / 2;
    if (q < cnt) break;
    q -= cnt;
  }
  int uu = 0;
  for (;; ++uu) {
    const int cnt = L - tt - uu + 1;
    if (q < cnt) break;
    q -= cnt;
  }
  *t = tt, *u = uu, *v = q;
  return true;
}

__global__ __launch_bounds__(kThreads) void one_electron_blocks_kernel(const IntArgs a) {
  __shared__ double sE[3 * kETab];
  __shared__ double sG[kRDim * kRDim * kRDim];
  __shared__ double sNuc[kWave * kNuc];
  __shared__ double sCart[2 * kCartMax * kCartMax];
  const int lane = threadIdx.x;
  const int64_t pair = blockIdx.x / kSplit;
  const int split = blockIdx.x % kSplit;

  // every index is checked before anything is read through it (uniform over the workgroup: all return together)
  int64_t ai = a.pairs[pair], aj = a.pairs[a.num_pairs + pair];
  if (ai < 0 || ai >= a.num_atoms || aj < 0 || aj >= a.num_atoms) return;
  if (ai > aj) {
    const int64_t s = ai;
    ai = aj, aj = s;
  }
  const int m = a.atom_mol[ai];
  if (m != a.atom_mol[aj] || m < 0 || m >= a.num_mols) return;
  const int ei = a.atom_elem[ai], ej = a.atom_elem[aj];
  if (ei < 0 || ei >= a.n_elem || ej < 0 || ej >= a.n_elem) return;
  const int64_t n0 = a.atom_start[m], n1 = a.atom_start[m + 1];
  if (n0 < 0 || n1 > a.num_atoms || ai < n0 || aj >= n1) return;
  const int nao = a.mol_nao[m];
  const int64_t ms = a.mat_start[m];
  if (nao < 0 || ms < 0 || ms > a.mat_elems || static_cast<int64_t>(nao) * nao > a.mat_elems - ms) return;
  // (the basis tables were checked on the host)
  const int sa0 = a.elem_shell[ei], sa1 = a.elem_shell[ei + 1], sb0 = a.elem_shell[ej], sb1 = a.elem_shell[ej + 1];
  const int nsa = sa1 - sa0, nsb = sb1 - sb0;
  if (nsa <= 0 || nsb <= 0) return;
  const int nao_i = a.shell_ao[sa1 - 1] + 2 * a.shell_l[sa1 - 1] + 1;
  const int nao_j = a.shell_ao[sb1 - 1] + 2 * a.shell_l[sb1 - 1] + 1;
  const int bi = a.ao_begin[ai], bj = a.ao_begin[aj];
  if (bi < 0 || nao_i > nao - bi || bj < 0 || nao_j > nao - bj) return;
  const bool diag = ai == aj;

  const double Ax = a.pos[3 * ai], Ay = a.pos[3 * ai + 1], Az = a.pos[3 * ai + 2];
  const double Bx = a.pos[3 * aj], By = a.pos[3 * aj + 1], Bz = a.pos[3 * aj + 2];
  // the E tables' lanes: dimension d, Hermite index t
  const int ed = lane / kTDim, et = lane % kTDim;
  const bool elane = lane < 3 * kTDim;
  const double ab = ed == 0 ? Ax - Bx : ed == 1 ? Ay - By : Az - Bz;
  double* Ed = sE + (elane ? ed : 0) * kETab;
  const double* Ex = sE;
  const double* Ey = sE + kETab;
  const double* Ez = sE + 2 * kETab;

  for (int sp = split; sp < nsa * nsb; sp += kSplit) {
    const int sa = sa0 + sp / nsb, sb = sb0 + sp % nsb;
    if (diag && sa > sb) continue;  // the mirror of (sb, sa)
    const int la = a.shell_l[sa], lb = a.shell_l[sb], L = la + lb;
    const int nca = ncart(la), ncb = ncart(lb), ncomp = nca * ncb;
    const int ca_off = la * (la + 1) * (la + 2) / 6, cb_off = lb * (lb + 1) * (lb + 2) / 6;

    // this lane's Cartesian component pairs and its (t, u, v)
    int pa[2][3], pb[2][3], tu[2][3];
    bool has_c[2], has_t[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int c = lane + s * kWave;
      has_c[s] = c < ncomp;
      const int ca = has_c[s] ? c / ncb : 0, cb = has_c[s] ? c % ncb : 0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        pa[s][d] = kCartPow[ca_off + ca][d];
        pb[s][d] = kCartPow[cb_off + cb][d];
      }
      tu[s][0] = tu[s][1] = tu[s][2] = 0;
      has_t[s] = tuv_of(lane + s * kWave, L, &tu[s][0], &tu[s][1], &tu[s][2]);
    }

    double accS[2] = {0.0, 0.0}, accH[2] = {0.0, 0.0};
    for (int ka = a.shell_prim[sa]; ka < a.shell_prim[sa + 1]; ++ka) {
      for (int kb = a.shell_prim[sb]; kb < a.shell_prim[sb + 1]; ++kb) {
        const double alpha = a.prim_exp[ka], beta = a.prim_exp[kb];
        const double cc = a.prim_coef[ka] * a.prim_coef[kb];
        const double p = alpha + beta, inv2p = 0.5 / p, mu = alpha * beta / p;
        const double Px = (alpha * Ax + beta * Bx) / p, Py = (alpha * Ay + beta * By) / p,
                     Pz = (alpha * Az + beta * Bz) / p;

        // ---- E^{ij}_t, one (i, j) step per barrier: first j at i = 0, then i for every j
        const double PA = -beta / p * ab, PB = alpha / p * ab;
        if (elane) Ed[eidx(0, 0, et)] = et == 0 ? exp(-mu * ab * ab) : 0.0;
        __syncthreads();
        for (int j = 0; j < lb + 2; ++j) {
          if (elane) {
            const double* e = Ed + eidx(0, j, 0);
            const double lo = et > 0 ? e[et - 1] : 0.0, hi = et + 1 < kTDim ? e[et + 1] : 0.0;
            Ed[eidx(0, j + 1, et)] = inv2p * lo + PB * e[et] + (et + 1) * hi;
          }
          __syncthreads();
        }
        for (int i = 0; i < la; ++i) {
          if (elane) {
            for (int j = 0; j <= lb + 2; ++j) {
              const double* e = Ed + eidx(i, j, 0);
              const double lo = et > 0 ? e[et - 1] : 0.0, hi = et + 1 < kTDim ? e[et + 1] : 0.0;
              Ed[eidx(i + 1, j, et)] = inv2p * lo + PA * e[et] + (et + 1) * hi;
            }
          }
          __syncthreads();
        }

        // ---- G_tuv = sum_C Z_C R_tuv(p, P - C): the nuclei in their order, 64 at a time
        double g[2] = {0.0, 0.0};
        for (int64_t c0 = n0; c0 < n1; c0 += kWave) {
          const int64_t c = c0 + lane;
          if (c < n1) {
            double* nu = sNuc + lane * kNuc;
            const double X = Px - a.pos[3 * c], Y = Py - a.pos[3 * c + 1], Z = Pz - a.pos[3 * c + 2];
            nu[0] = X, nu[1] = Y, nu[2] = Z;
            nu[3] = static_cast<double>(a.charge[c]);
            boys(p * (X * X + Y * Y + Z * Z), L, nu + 4);
          }
          __syncthreads();
          const int cnt = static_cast<int>(n1 - c0 < kWave ? n1 - c0 : kWave);
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            if (has_t[s]) {
              for (int k = 0; k < cnt; ++k) {
                const double* nu = sNuc + k * kNuc;
                g[s] += nu[3] * r_tuv(tu[s][0], tu[s][1], tu[s][2], p, nu[0], nu[1], nu[2], nu + 4);
              }
            }
          }
          __syncthreads();
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
          if (has_t[s]) sG[gidx(tu[s][0], tu[s][1], tu[s][2])] = g[s];
        __syncthreads();

        // ---- this lane's components
        const double fac = kPi / p * sqrt(kPi / p);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (!has_c[s]) continue;
          const int ax = pa[s][0], ay = pa[s][1], az = pa[s][2], bx = pb[s][0], by = pb[s][1], bz = pb[s][2];
          const double* ex = Ex + eidx(ax, bx, 0);
          const double* ey = Ey + eidx(ay, by, 0);
          const double* ez = Ez + eidx(az, bz, 0);
          const double sx = ex[0], sy = ey[0], sz = ez[0];
          // 1-D kinetic: -1/2 (j (j - 1) S_{i,j-2} - 2 b (2j + 1) S_{ij} + 4 b^2 S_{i,j+2})
          const double tx = -0.5 * ((bx >= 2 ? bx * (bx - 1) * ex[-2 * kTDim] : 0.0) - 2.0 * beta * (2 * bx + 1) * sx +
                                    4.0 * beta * beta * ex[2 * kTDim]);
          const double ty = -0.5 * ((by >= 2 ? by * (by - 1) * ey[-2 * kTDim] : 0.0) - 2.0 * beta * (2 * by + 1) * sy +
                                    4.0 * beta * beta * ey[2 * kTDim]);
          const double tz = -0.5 * ((bz >= 2 ? bz * (bz - 1) * ez[-2 * kTDim] : 0.0) - 2.0 * beta * (2 * bz + 1) * sz +
                                    4.0 * beta * beta * ez[2 * kTDim]);
          double vsum = 0.0;
          for (int t = 0; t <= ax + bx; ++t)
            for (int u = 0; u <= ay + by; ++u) {
              const double eu = ex[t] * ey[u];
              for (int v = 0; v <= az + bz; ++v) vsum += eu * ez[v] * sG[gidx(t, u, v)];
            }
          const double S = fac * (sx * sy * sz);
          const double T = fac * (tx * sy * sz + sx * ty * sz + sx * sy * tz);
          const double V = -2.0 * kPi / p * vsum;
          accS[s] += cc * S;
          accH[s] += cc * (T + V);
        }
        __syncthreads();
      }
    }

    // ---- Cartesian -> real solid harmonics, out to (i, j) and (j, i)
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (has_c[s]) {
        sCart[lane + s * kWave] = accS[s];
        sCart[kCartMax * kCartMax + lane + s * kWave] = accH[s];
      }
    __syncthreads();
    const int nfa = 2 * la + 1, nfb = 2 * lb + 1;
    const int row0 = bi + a.shell_ao[sa], col0 = bj + a.shell_ao[sb];
    for (int e = lane; e < nfa * nfb; e += kWave) {
      const int fa = e / nfb, fb = e % nfb;
      double vS = 0.0, vH = 0.0;
      for (int ca = 0; ca < nca; ++ca) {
        const double wa = kC2S[la][fa][ca];
        if (wa == 0.0) continue;
        for (int cb = 0; cb < ncb; ++cb) {
          const double w = wa * kC2S[lb][fb][cb];
          vS += w * sCart[ca * ncb + cb];
          vH += w * sCart[kCartMax * kCartMax + ca * ncb + cb];
        }
      }
      const int row = row0 + fa, col = col0 + fb;
      if (diag && row > col) continue;  // the upper triangle is mirrored
      const int64_t rc = ms + static_cast<int64_t>(row) * nao + col, cr = ms + static_cast<int64_t>(col) * nao + row;
      a.ovlp[rc] = vS;
      a.ovlp[cr] = vS;
      a.hcore[rc] = vH;
      a.hcore[cr] = vH;
    }
    __syncthreads();
  }
}

// the host's copy of the basis tables: X2G_OK, or why they cannot be used
int check_basis(const int32_t* tab, int64_t n_elem, int64_t n_shells, int64_t n_prims) {
  const int32_t* elem_shell = tab;
  const int32_t* shell_l = elem_shell + n_elem + 1;
  const int32_t* shell_prim = shell_l + n_shells;
  const int32_t* shell_ao = shell_prim + n_shells + 1;
  if (elem_shell[0] != 0 || elem_shell[n_elem] != n_shells || shell_prim[0] != 0 || shell_prim[n_shells] != n_prims)
    return X2G_EINVAL;
  for (int64_t s = 0; s < n_shells; ++s)
    if (shell_prim[s + 1] < shell_prim[s] || shell_l[s] < 0) return X2G_EINVAL;
  for (int64_t e = 0; e < n_elem; ++e)
    if (elem_shell[e + 1] < elem_shell[e]) return X2G_EINVAL;
  for (int64_t s = 0; s < n_shells; ++s)
    if (shell_l[s] > kMaxL) return X2G_EUNSUPPORTED;
  for (int64_t e = 0; e < n_elem; ++e) {
    int64_t ao = 0;
    for (int32_t s = elem_shell[e]; s < elem_shell[e + 1]; ++s) ao += 2 * shell_l[s] + 1;
    if (ao > kMaxAo) return X2G_EUNSUPPORTED;
    ao = 0;
    for (int32_t s = elem_shell[e]; s < elem_shell[e + 1]; ++s) {
      if (shell_ao[s] != ao) return X2G_EINVAL;  // functions in shell order, without gaps
      ao += 2 * shell_l[s] + 1;
    }
  }
  return X2G_OK;
}

}  // namespace
}  // namespace x2g

using namespace x2g;

X2G_API int x2g_one_electron_blocks(const int32_t* basis_tab, const int32_t* basis_tab_host, const double* prim_exp,
                                    const double* prim_coef, int64_t n_elem, int64_t n_shells, int64_t n_prims,
                                    const double* atom_pos, const int32_t* atom_charge, const int32_t* atom_elem,
                                    const int32_t* atom_mol, const int32_t* ao_begin, const int64_t* atom_start,
                                    const int64_t* mat_start, const int32_t* mol_nao, int64_t num_mols,
                                    int64_t num_atoms, int64_t mat_elems, const int64_t* pairs, int64_t num_pairs,
                                    double* ovlp, double* hcore, void* stream) {
  if (!basis_tab || !basis_tab_host || !prim_exp || !prim_coef || !atom_pos || !atom_charge || !atom_elem ||
      !atom_mol || !ao_begin || !atom_start || !mat_start || !mol_nao || !pairs || !ovlp || !hcore || n_elem < 0 ||
      n_shells < 0 || n_prims < 0 || num_mols < 0 || num_atoms < 0 || mat_elems < 0 || num_pairs < 0)
    return X2G_EINVAL;
  constexpr int64_t k31 = int64_t(1) << 31;
  // 32-bit shell, primitive and atom indices in the kernel, and kSplit workgroups per pair in a 32-bit grid
  if (n_elem >= k31 || n_shells >= k31 || n_prims >= k31 || num_atoms >= k31 || num_pairs >= k31 / kSplit)
    return X2G_EUNSUPPORTED;
  const int rc = check_basis(basis_tab_host, n_elem, n_shells, n_prims);
  if (rc != X2G_OK) return rc;
  if (num_pairs == 0) return X2G_OK;
  const int32_t* elem_shell = basis_tab;
  const int32_t* shell_l = elem_shell + n_elem + 1;
  const int32_t* shell_prim = shell_l + n_shells;
  const int32_t* shell_ao = shell_prim + n_shells + 1;
  const IntArgs a{elem_shell, shell_l, shell_prim, shell_ao, prim_exp, prim_coef, atom_pos, atom_charge, atom_elem,
                  atom_mol, ao_begin, atom_start, mat_start, mol_nao, pairs, ovlp, hcore, n_elem, num_mols, num_atoms,
                  mat_elems, num_pairs};
  one_electron_blocks_kernel<<<static_cast<unsigned>(num_pairs * kSplit), kThreads, 0, as_stream(stream)>>>(a);
  return last_launch_status();
}
