// MMSE-IRC equalisation of L transmit layers on P receive ports for ONE resource element, shared by the stand-alone equaliser
// (equalizer.hip, miphy_channel_equalize_mmse_batch) and whatever fuses it later: the same inputs give the same bits through any kernel.
//   y = t H x + n,  E[n n^H] = C (P x P, Hermitian; only its lower triangle and the real parts of its diagonal are read),  t = tx_scaling
//   W = C^-1;  A = t^2 H^H W H + I;  B = A^-1;  x~ = t B H^H W y;  gamma_l = 1 - B_ll;  x_l = x~_l / gamma_l;  nvar_l = B_ll / gamma_l.
// Three parts: mmse_factor depends on C only (a thread runs it once per covariance matrix), mmse_prepare on the factor and H (once per
// subcarrier where the estimate is compact), mmse_apply on the sample.
//
// Arithmetic: single IEEE operations in the order written here (no contraction), exact division, no square roots; the complex products and
// the port sums are those of equalize_device.h (zf_mul, zf_conj_mul, zf_mul_conj, zf_norm, zf_dot, zf_col_norm: port order, from port 0).
// mmse_factor: LDL^H of C without pivoting, columns left to right (j = 0 .. P-1, rows i = j .. P-1, inner sums k = 0 .. j-1 ascending):
//        w_ij = C_ij - sum_k w_ik conj(l_jk)   (i = j: real parts only);   d_j = Re w_jj;   rc_j = 1 / d_j;   l_ij = w_ij rc_j
//      then the inverse of the unit lower factor, N = l^-1, column by column (rows ascending, inner sum k = j+1 .. i-1 ascending):
//        N_ij = -(l_ij + sum_k l_ik N_kj)
//      so that W = N^H diag(rc) N.
// mmse_prepare: the channel behind the factor, per layer a: u_a = N h_a, uw_a = diag(rc) u_a:
//        u_a[p] = h_a[p] + sum_{k<p} N_pk h_a[k]   (k ascending);   uw_a[p] = u_a[p] rc_p
//      S = H^H W H, lower triangle: S_jj = sum_p |u_j[p]|^2 rc_p (port order, from port 0), S_ij = sum_p conj(u_i[p]) uw_j[p] (zf_dot), i > j
//      T = t^2 S with t2 = t t:  T_jj = t2 S_jj, T_ij = t2 S_ij;   A = T + I:  A_jj = T_jj + 1
//      LDL^H of A exactly as above (pivots da_j, ra_j = 1 / da_j, unit lower factor, M = its inverse), so B = M^H diag(ra) M:
//        B_ab = sum_{k >= a} conj(M_ka) ra_k M_kb  for a >= b  (M_aa = 1: the first term is ra_a M_ab, or ra_a when a = b; k ascending;
//               term = (conj(M_ka) M_kb) ra_k, for a = b |M_ka|^2 ra_k)
//      gamma without the cancellation of 1 - B_ll at low SINR: I - B = B T, so
//        gamma_a = sum_k Re(B_ak T_ka)   (k = 0 .. L-1 ascending, from the term of k = 0; B_ak = conj(B_ka) for k > a, T_ka = conj(T_ak) for
//                  k < a; the term of k = a is B_aa T_aa, every other term is Re(b) Re(t) + Im(b) Im(t) with b, t the stored lower-triangle entries
//                  B_max,min and T_max,min)
//        g_a = 1 / gamma_a;   sc_a = t g_a;   nvar_a = B_aa g_a
// mmse_apply:   v = N y:  v[p] = y[p] + sum_{k<p} N_pk y[k]   (k ascending);   m_a = sum_p conj(uw_a[p]) v[p]   (zf_dot)
//        z_i = (m_i + sum_{j<i} M_ij m_j) ra_i   (j ascending);   x~_a = z_a + sum_{k>a} conj(M_ka) z_k   (k ascending);   x_a = x~_a sc_a
// Abnormal rule: if a pivot d_j of C, a pivot da_j of A or a gamma_a is not a normal positive number, every layer of the element gets symbol 0 and
// noise variance +inf. tests/pusch_mmse_cases.py restates all of it in numpy float32 (mmse_single) and holds it to numpy.linalg in float64.
#pragma once
#include "equalize_device.h"

__device__ __forceinline__ bool mmse_pos_normal(float x)
{
  return x >= 1.17549435e-38f && x < INFINITY; // normal and positive (false for NaN)
}

// LDL^H of an n x n Hermitian matrix (n <= K) given by its lower triangle a[i][j], i >= j (diagonal: .x only); r[j] = 1 / pivot; m[] = the inverse of
// the unit lower factor at i (i - 1) / 2 + j, i > j. Returns whether every pivot is a normal positive number. Entries at or behind n are not touched.
template <int K>
__device__ __forceinline__ bool mmse_ldl(const float2 (&a)[K][K], int n, float (&r)[K], float2 (&m)[K * (K - 1) / 2 + (K == 1)])
{
#pragma clang fp contract(off)
  float2 w[K][K], l[K][K]; // lower triangles
  bool   ok = true;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (j >= n)
      continue;
#pragma unroll
    for (int i = j; i < K; ++i) {
      if (i >= n)
        continue;
      float2 acc = (i == j) ? make_float2(a[j][j].x, 0.f) : a[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) {
        const float2 t = zf_mul_conj(w[i][k], l[j][k]);
        acc            = (i == j) ? make_float2(acc.x - t.x, 0.f) : make_float2(acc.x - t.x, acc.y - t.y);
      }
      w[i][j] = acc;
    }
    const float d = w[j][j].x;
    r[j]          = 1.0f / d;
    ok            = ok && mmse_pos_normal(d);
#pragma unroll
    for (int i = j + 1; i < K; ++i)
      if (i < n)
        l[i][j] = make_float2(w[i][j].x * r[j], w[i][j].y * r[j]);
  }
#pragma unroll
  for (int j = 0; j < K; ++j)
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      if (i >= n)
        continue;
      float2 acc = l[i][j];
#pragma unroll
      for (int k = j + 1; k < i; ++k) {
        const float2 t = zf_mul(l[i][k], m[k * (k - 1) / 2 + j]);
        acc            = make_float2(acc.x + t.x, acc.y + t.y);
      }
      m[i * (i - 1) / 2 + j] = make_float2(-acc.x, -acc.y);
    }
  return ok;
}

// v = N y for the unit lower N of a factor (n ports)
__device__ __forceinline__ void mmse_lower_mul(const float2 (&nm)[6], int n, const float2* y, float2* v)
{
#pragma clang fp contract(off)
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (p >= n)
      continue;
    float2 acc = y[p];
#pragma unroll
    for (int k = 0; k < p; ++k) {
      const float2 t = zf_mul(nm[p * (p - 1) / 2 + k], y[k]);
      acc            = make_float2(acc.x + t.x, acc.y + t.y);
    }
    v[p] = acc;
  }
}

// What mmse_factor leaves of one covariance matrix.
struct mmse_factored {
  bool   ok;
  float  rc[4];
  float2 N[6];
};

// c[p][q], p >= q: the lower triangle of C (np x np).
__device__ __forceinline__ void mmse_factor(const float2 (&c)[4][4], int np, mmse_factored& f)
{
  f.ok = mmse_ldl<4>(c, np, f.rc, f.N);
}

// What mmse_prepare leaves for mmse_apply. nvar[l] is final (+inf on an abnormal element).
template <int L>
struct mmse_prepared {
  bool   ok;
  float  nvar[L];
  float  sc[L];                              // t / gamma_l
  float  ra[L];                              // 1 / pivot of A
  float2 M[L * (L - 1) / 2 + (L == 1)];      // M_ij, i > j, at i (i - 1) / 2 + j
  float2 uw[L][4];                           // diag(rc) N h_l
};

// h[l][p]: estimate of layer l on port p (p < np <= 4).
template <int L>
__device__ __forceinline__ void mmse_prepare(const float2 (*h)[4], int np, const mmse_factored& f, float tx, mmse_prepared<L>& q)
{
#pragma clang fp contract(off)
  float2 u[L][4];
#pragma unroll
  for (int a = 0; a < L; ++a) {
    mmse_lower_mul(f.N, np, h[a], u[a]);
#pragma unroll
    for (int p = 0; p < 4; ++p)
      q.uw[a][p] = (p < np) ? make_float2(u[a][p].x * f.rc[p], u[a][p].y * f.rc[p]) : make_float2(0.f, 0.f);
  }
  const float t2 = tx * tx;
  float2      T[L][L], A[L][L]; // lower triangles
#pragma unroll
  for (int j = 0; j < L; ++j) {
    float s = zf_norm(u[j][0]) * f.rc[0];
#pragma unroll
    for (int p = 1; p < 4; ++p)
      if (p < np)
        s = s + zf_norm(u[j][p]) * f.rc[p];
    T[j][j] = make_float2(t2 * s, 0.f);
    A[j][j] = make_float2(T[j][j].x + 1.0f, 0.f);
#pragma unroll
    for (int i = j + 1; i < L; ++i) {
      const float2 sij = zf_dot(u[i], q.uw[j], np);
      T[i][j] = A[i][j] = make_float2(t2 * sij.x, t2 * sij.y);
    }
  }
  bool ok = mmse_ldl<L>(A, L, q.ra, q.M) && f.ok;
  // B = M^H diag(ra) M, lower triangle
  float2 B[L][L];
#pragma unroll
  for (int a = 0; a < L; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      float2 acc = (a == b) ? make_float2(q.ra[a], 0.f) : make_float2(q.M[a * (a - 1) / 2 + b].x * q.ra[a], q.M[a * (a - 1) / 2 + b].y * q.ra[a]);
#pragma unroll
      for (int k = a + 1; k < L; ++k) {
        if (a == b) {
          acc.x = acc.x + zf_norm(q.M[k * (k - 1) / 2 + a]) * q.ra[k];
        } else {
          const float2 t = zf_conj_mul(q.M[k * (k - 1) / 2 + a], q.M[k * (k - 1) / 2 + b]);
          acc            = make_float2(acc.x + t.x * q.ra[k], acc.y + t.y * q.ra[k]);
        }
      }
      B[a][b] = acc;
    }
#pragma unroll
  for (int a = 0; a < L; ++a) {
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const int   hi = k > a ? k : a, lo = k > a ? a : k;
      const float t  = (k == a) ? B[a][a].x * T[a][a].x : B[hi][lo].x * T[hi][lo].x + B[hi][lo].y * T[hi][lo].y;
      g              = (k == 0) ? t : g + t;
    }
    ok              = ok && mmse_pos_normal(g);
    const float rg  = 1.0f / g;
    q.sc[a]         = tx * rg;
    q.nvar[a]       = B[a][a].x * rg;
  }
#pragma unroll
  for (int a = 0; a < L; ++a)
    q.nvar[a] = ok ? q.nvar[a] : INFINITY;
  q.ok = ok;
}

// y[p]: the received sample on port p; x[l]: the equalised symbol of layer l (0 on an abnormal element).
template <int L>
__device__ __forceinline__ void mmse_apply(int np, const mmse_factored& f, const float2* y, const mmse_prepared<L>& q, float2* x)
{
#pragma clang fp contract(off)
  float2 v[4], m[L], z[L];
#pragma unroll
  for (int p = 0; p < 4; ++p)
    v[p] = make_float2(0.f, 0.f);
  mmse_lower_mul(f.N, np, y, v);
#pragma unroll
  for (int a = 0; a < L; ++a)
    m[a] = zf_dot(q.uw[a], v, np);
#pragma unroll
  for (int i = 0; i < L; ++i) {
    float2 acc = m[i];
#pragma unroll
    for (int j = 0; j < i; ++j) {
      const float2 t = zf_mul(q.M[i * (i - 1) / 2 + j], m[j]);
      acc            = make_float2(acc.x + t.x, acc.y + t.y);
    }
    z[i] = make_float2(acc.x * q.ra[i], acc.y * q.ra[i]);
  }
#pragma unroll
  for (int a = 0; a < L; ++a) {
    float2 acc = z[a];
#pragma unroll
    for (int k = a + 1; k < L; ++k) {
      const float2 t = zf_conj_mul(q.M[k * (k - 1) / 2 + a], z[k]);
      acc            = make_float2(acc.x + t.x, acc.y + t.y);
    }
    x[a] = q.ok ? make_float2(acc.x * q.sc[a], acc.y * q.sc[a]) : make_float2(0.f, 0.f);
  }
}
