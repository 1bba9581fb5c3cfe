// Eigen-decomposition of ONE Hermitian matrix of order n <= 4 by cyclic Jacobi, in registers (precoding_weights.hip).
//   a: the full matrix (entries at or behind n are 0); on return its diagonal holds the eigenvalues, unsorted. v: on return the eigenvectors, by column.
// A fixed JACOBI_SWEEPS sweeps over (p, q) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3); pairs with q >= n are left out. One rotation, with b = a_pq:
//   g2 = Re b Re b + Im b Im b;  skipped unless g2 is a positive normal number (a zero or vanishing off-diagonal element: nothing is divided by it)
//   g = sqrt(g2);  e = (Re b / g, Im b / g);  tau = (a_qq - a_pp) / (g + g);  t = 1 / (|tau| + sqrt(1 + tau tau)), negated where tau < 0
//   c = 1 / sqrt(1 + t t);  s = t c;  z = (s Re e, s Im e)
//   J = the identity but J_pp = J_qq = c, J_pq = z, J_qp = -conj(z);   a <- J^H a J,   v <- v J:
//     columns, every row k < n:  (x_kp, x_kq) <- (c x_kp - x_kq conj(z),  x_kp z + c x_kq)        for x = a and for x = v
//     rows, every column k < n:  (a_pk, a_qk) <- (c a_pk - z a_qk,  conj(z) a_pk + c a_qk)
//     then a_pq = a_qp = 0 and the imaginary parts of a_pp and a_qq are 0.
// An infinite tau gives t = 0, c = 1, s = 0. Arithmetic: single IEEE operations in the order written (no contraction), exact division and square
// root; the complex products are zf_mul, zf_mul_conj and zf_conj_mul of equalize_device.h. tests/precoding_weights_ref.py restates it in numpy float32.
#pragma once
#include "mmse_device.h"

constexpr int JACOBI_SWEEPS = 5;

template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(float2 (&a)[4][4], float2 (&v)[4][4], int n)
{
#pragma clang fp contract(off)
  if (Q >= n)
    return;
  const float2 b  = a[P][Q];
  const float  g2 = b.x * b.x + b.y * b.y;
  if (!mmse_pos_normal(g2))
    return;
  const float  g   = sqrtf(g2);
  const float2 e   = make_float2(b.x / g, b.y / g);
  const float  tau = (a[Q][Q].x - a[P][P].x) / (g + g);
  const float  ta  = 1.0f / (fabsf(tau) + sqrtf(1.0f + tau * tau));
  const float  t   = tau < 0.f ? -ta : ta;
  const float  c   = 1.0f / sqrtf(1.0f + t * t);
  const float  s   = t * c;
  const float2 z   = make_float2(s * e.x, s * e.y);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= n)
      continue;
    {
      const float2 xp = a[k][P], xq = a[k][Q];
      const float2 u = zf_mul_conj(xq, z), w = zf_mul(xp, z);
      a[k][P] = make_float2(c * xp.x - u.x, c * xp.y - u.y);
      a[k][Q] = make_float2(w.x + c * xq.x, w.y + c * xq.y);
    }
    {
      const float2 xp = v[k][P], xq = v[k][Q];
      const float2 u = zf_mul_conj(xq, z), w = zf_mul(xp, z);
      v[k][P] = make_float2(c * xp.x - u.x, c * xp.y - u.y);
      v[k][Q] = make_float2(w.x + c * xq.x, w.y + c * xq.y);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= n)
      continue;
    const float2 xp = a[P][k], xq = a[Q][k];
    const float2 u = zf_mul(z, xq), w = zf_conj_mul(z, xp);
    a[P][k] = make_float2(c * xp.x - u.x, c * xp.y - u.y);
    a[Q][k] = make_float2(w.x + c * xq.x, w.y + c * xq.y);
  }
  a[P][Q] = a[Q][P] = make_float2(0.f, 0.f);
  a[P][P].y = a[Q][Q].y = 0.f;
}

__device__ __forceinline__ void jacobi_eig(float2 (&a)[4][4], float2 (&v)[4][4], int n)
{
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[i][k] = make_float2(i == k ? 1.f : 0.f, 0.f);
#pragma unroll 1
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(a, v, n);
    jacobi_rotate<0, 2>(a, v, n);
    jacobi_rotate<0, 3>(a, v, n);
    jacobi_rotate<1, 2>(a, v, n);
    jacobi_rotate<1, 3>(a, v, n);
    jacobi_rotate<2, 3>(a, v, n);
  }
}
