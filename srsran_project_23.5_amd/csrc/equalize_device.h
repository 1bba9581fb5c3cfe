// Zero-forcing equalisation of L transmit layers on P receive ports for ONE resource element, shared by the stand-alone equaliser
// (equalizer.hip, miphy_channel_equalize_layers_batch) and the layered PUSCH demodulator (pusch_demod.hip): the same inputs give the same
// bits through either kernel.
//   H is P x L, G = H^H H, m = H^H y;  x = G^-1 m / tx_scaling;  nvar_l = noise_var [G^-1]_ll / tx_scaling^2.
// Two parts: zf_prepare depends on H only (a thread that holds a compact estimate runs it once per subcarrier), zf_apply on the sample.
//
// Arithmetic: single IEEE operations in the order written here (no contraction), exact division, no square roots. Every sum over the
// receive ports runs in port order and starts from the term of port 0. With a = h[l0][p], b = h[l1][p] the term of port p is
//   conj(a) b = (a.x b.x + a.y b.y,  a.x b.y - a.y b.x),      |a|^2 = a.x a.x + a.y a.y.
// L = 1: equalize_zf_1xn.h:120-158 (its sums start from 0).  d = tx * sum |h|^2, r = 1 / d, x = m r, nvar = r (noise_var / tx).
// L = 2: equalize_zf_2x2.cpp:58-118.  n0, n1 the column norms, xi = G_01, d_pinv = tx (n0 n1 - |xi|^2), d_nvars = tx d_pinv,
//        x0 = (n1 m0 - xi m1) / d_pinv, x1 = (n0 m1 - conj(xi) m0) / d_pinv, nvar_l = noise_var n_(1-l) / d_nvars. At P = 2 these are the
//        operations of the 2 x 2 kernel, bit for bit.
// L = 3, 4: LDL^H of G without pivoting, columns left to right (j = 0 .. L-1, rows i = j .. L-1, inner sums k = 0 .. j-1 ascending):
//        w_ij = G_ij - sum_k w_ik conj(l_jk);  d_j = Re w_jj;  l_ij = w_ij (1 / d_j)
//      then the inverse of the unit lower factor, M = l^-1, column by column (rows ascending, inner sum k = j+1 .. i-1 ascending):
//        M_ij = -(l_ij + sum_k l_ik M_kj)
//      and with r_k = 1 / (tx d_k):
//        nvar_a = (r_a + sum_{k>a} |M_ka|^2 r_k) (noise_var / tx)                       (k ascending)
//        z_i = (m_i + sum_{j<i} M_ij m_j) r_i                                           (j ascending)
//        x_a = z_a + sum_{k>a} conj(M_ka) z_k                                           (k ascending)
//      Products: a b = (a.x b.x - a.y b.y, a.x b.y + a.y b.x); a conj(b) = (a.x b.x + a.y b.y, a.y b.x - a.x b.y);
//      conj(a) b as above. tests/pusch_layers_cases.py restates all of it in numpy float32.
// Abnormal rule (every L): if a denominator (d of L = 1, d_pinv of L = 2, a pivot d_k or tx d_k of L >= 3) is not a normal number, or
// noise_var is not normal or not > 0, every layer of the element gets symbol 0 and noise variance +inf.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

__device__ __forceinline__ bool zf_is_normal(float x)
{
  const float a = fabsf(x);
  return a >= 1.17549435e-38f && a < INFINITY; // std::isnormal: neither zero, subnormal, infinite nor NaN
}

__device__ __forceinline__ float2 zf_conj_mul(float2 a, float2 b) // conj(a) b
{
#pragma clang fp contract(off)
  return make_float2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ float2 zf_mul(float2 a, float2 b)
{
#pragma clang fp contract(off)
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 zf_mul_conj(float2 a, float2 b) // a conj(b)
{
#pragma clang fp contract(off)
  return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ float zf_norm(float2 a)
{
#pragma clang fp contract(off)
  return a.x * a.x + a.y * a.y;
}

// sum over the ports of conj(a[p]) b[p]; FROM_ZERO: the sum starts at 0 + the term of port 0, as the one-layer reference does (only the sign of a
// zero can differ)
template <bool FROM_ZERO = false>
__device__ __forceinline__ float2 zf_dot(const float2* a, const float2* b, int np)
{
#pragma clang fp contract(off)
  float2 s = zf_conj_mul(a[0], b[0]);
  if (FROM_ZERO)
    s = make_float2(0.f + s.x, 0.f + s.y);
#pragma unroll
  for (int p = 1; p < 4; ++p)
    if (p < np) {
      const float2 t = zf_conj_mul(a[p], b[p]);
      s              = make_float2(s.x + t.x, s.y + t.y);
    }
  return s;
}
__device__ __forceinline__ float zf_col_norm(const float2* a, int np)
{
#pragma clang fp contract(off)
  float s = zf_norm(a[0]);
#pragma unroll
  for (int p = 1; p < 4; ++p)
    if (p < np)
      s = s + zf_norm(a[p]);
  return s;
}

// What zf_prepare leaves for zf_apply. nvar[l] is final (+inf on an abnormal element).
template <int L>
struct zf_prepared {
  bool   ok;
  float  nvar[L];
  float  r[L];                              // L = 1: 1 / d; L = 2: r[0] = 1 / d_pinv, r[1] unused; L >= 3: 1 / (tx d_k)
  float  n[L == 2 ? 2 : 1];                 // L = 2: column norms
  float2 M[L == 2 ? 1 : (L * (L - 1)) / 2 + (L == 1)]; // L = 2: xi; L >= 3: M_ij, i > j, at i (i - 1) / 2 + j
};

// h[l][p]: estimate of layer l on port p (p < np <= 4).
template <int L>
__device__ __forceinline__ void zf_prepare(const float2 (*h)[4], int np, float noise_var, float tx, zf_prepared<L>& q)
{
#pragma clang fp contract(off)
  const bool nv_ok = zf_is_normal(noise_var) && noise_var > 0.f;
  if constexpr (L == 1) {
    const float d = tx * (0.f + zf_col_norm(h[0], np));
    q.ok          = zf_is_normal(d) && nv_ok;
    q.r[0]        = 1.0f / d;
    q.nvar[0]     = q.ok ? q.r[0] * (noise_var / tx) : INFINITY;
  } else if constexpr (L == 2) {
    q.n[0]              = zf_col_norm(h[0], np);
    q.n[1]              = zf_col_norm(h[1], np);
    q.M[0]              = zf_dot(h[0], h[1], np);
    const float xm      = q.M[0].x * q.M[0].x + q.M[0].y * q.M[0].y;
    const float d_pinv  = tx * ((q.n[0] * q.n[1]) - xm);
    const float d_nvars = tx * d_pinv;
    q.ok                = zf_is_normal(d_pinv) && nv_ok;
    q.r[0]              = 1.0f / d_pinv;
    q.r[1]              = 0.f;
    const float rn      = 1.0f / d_nvars;
    q.nvar[0]           = q.ok ? noise_var * q.n[1] * rn : INFINITY;
    q.nvar[1]           = q.ok ? noise_var * q.n[0] * rn : INFINITY;
  } else {
    float2 w[L][L], l[L][L]; // lower triangles
    float  d[L];
    bool   ok = nv_ok;
#pragma unroll
    for (int j = 0; j < L; ++j) {
#pragma unroll
      for (int i = j; i < L; ++i) {
        float2 acc = (i == j) ? make_float2(zf_col_norm(h[j], np), 0.f) : zf_dot(h[i], h[j], np); // G_ij = sum conj(h_pi) h_pj
#pragma unroll
        for (int k = 0; k < j; ++k) {
          const float2 t = zf_mul_conj(w[i][k], l[j][k]);
          acc            = (i == j) ? make_float2(acc.x - t.x, 0.f) : make_float2(acc.x - t.x, acc.y - t.y);
        }
        w[i][j] = acc;
      }
      d[j]           = w[j][j].x;
      const float rd = 1.0f / d[j];
#pragma unroll
      for (int i = j + 1; i < L; ++i)
        l[i][j] = make_float2(w[i][j].x * rd, w[i][j].y * rd);
      const float dt = tx * d[j];
      q.r[j]         = 1.0f / dt;
      ok             = ok && zf_is_normal(d[j]) && zf_is_normal(dt);
    }
#pragma unroll
    for (int j = 0; j < L; ++j)
#pragma unroll
      for (int i = j + 1; i < L; ++i) {
        float2 acc = l[i][j];
#pragma unroll
        for (int k = j + 1; k < i; ++k) {
          const float2 t = zf_mul(l[i][k], q.M[k * (k - 1) / 2 + j]);
          acc            = make_float2(acc.x + t.x, acc.y + t.y);
        }
        q.M[i * (i - 1) / 2 + j] = make_float2(-acc.x, -acc.y);
      }
    const float s = noise_var / tx;
#pragma unroll
    for (int a = 0; a < L; ++a) {
      float acc = q.r[a];
#pragma unroll
      for (int k = a + 1; k < L; ++k)
        acc = acc + zf_norm(q.M[k * (k - 1) / 2 + a]) * q.r[k];
      q.nvar[a] = ok ? acc * s : INFINITY;
    }
    q.ok = ok;
  }
}

// y[p]: the received sample on port p; x[l]: the equalised symbol of layer l (0 on an abnormal element).
template <int L>
__device__ __forceinline__ void zf_apply(const float2 (*h)[4], int np, const float2* y, const zf_prepared<L>& q, float2* x)
{
#pragma clang fp contract(off)
  float2 m[L];
#pragma unroll
  for (int a = 0; a < L; ++a)
    m[a] = zf_dot<L == 1>(h[a], y, np);
  if constexpr (L == 1) {
    x[0] = make_float2(m[0].x * q.r[0], m[0].y * q.r[0]);
  } else if constexpr (L == 2) {
    const float xr = q.M[0].x, xi = q.M[0].y, n0 = q.n[0], n1 = q.n[1], rp = q.r[0];
    x[0] = make_float2((n1 * m[0].x - (xr * m[1].x - xi * m[1].y)) * rp, (n1 * m[0].y - (xr * m[1].y + xi * m[1].x)) * rp);
    x[1] = make_float2((n0 * m[1].x - (xr * m[0].x + xi * m[0].y)) * rp, (n0 * m[1].y - (xr * m[0].y - xi * m[0].x)) * rp);
  } else {
    float2 z[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
      float2 acc = m[i];
#pragma unroll
      for (int j = 0; j < i; ++j) {
        const float2 t = zf_mul(q.M[i * (i - 1) / 2 + j], m[j]);
        acc            = make_float2(acc.x + t.x, acc.y + t.y);
      }
      z[i] = make_float2(acc.x * q.r[i], acc.y * q.r[i]);
    }
#pragma unroll
    for (int a = 0; a < L; ++a) {
      float2 acc = z[a];
#pragma unroll
      for (int k = a + 1; k < L; ++k) {
        const float2 t = zf_conj_mul(q.M[k * (k - 1) / 2 + a], z[k]);
        acc            = make_float2(acc.x + t.x, acc.y + t.y);
      }
      x[a] = acc;
    }
  }
  if (!q.ok) {
#pragma unroll
    for (int a = 0; a < L; ++a)
      x[a] = make_float2(0.f, 0.f);
  }
}
