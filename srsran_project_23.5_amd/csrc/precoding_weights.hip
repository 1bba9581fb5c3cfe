// Precoding weights from SRS channel matrices, for a batch of jobs: per output PRG the eigen-beamforming (one UE) or regularised zero-forcing (2..4
// UEs) weights W[prg][port][layer] of every UE in the memory order of miphy_precoding, and per layer its eigenvalue, signal and leakage. Beyond the
// 23.5 reference, which computes no precoding; the contract is restated in numpy in tests/precoding_weights_ref.py.
//
// The job: K = nof_ues (1..4) UEs on A = nof_ports (1..4) antenna ports. UE k: H_k[g][a][u] from h_offset as miphy_srs_estimate_batch wrote it (G =
// nof_prb / prg_size SRS PRGs of s = prg_size PRBs from start_prb, U = nof_ue_ports), l_k = nof_layers; L = sum l_k <= min(4, A). Output PRG j covers the
// PRBs [j S, (j + 1) S), S = the job's prg_size, j < nof_prg.
//
// The arithmetic, per output PRG j:
//  1. Per UE, lo = max(j S, start_prb), hi = min((j + 1) S, start_prb + nof_prb). Where hi > lo the SRS PRGs i0 = (lo - start_prb) / s .. i1 =
//     (hi - 1 - start_prb) / s enter with w_i = the PRBs they share with [lo, hi) and w = hi - lo; else one PRG, i0 = i1 = 0 where the output PRG lies
//     below the band and G - 1 above it, w_i = w = 1.
//     P_i[a][b] = sum_u conj(H[i][a][u]) H[i][b][u], a >= b (u ascending from the term of u = 0; a = b: |H|^2, real);  acc += w_i P_i from acc = 0;
//     R[a][b] = acc / w. Lane form: i ascending. Wave form: lane t adds i0 + t, i0 + t + 64, ..., then the xor tree 32, 16, .. 1 over the 64 lanes.
//     The upper triangle is the conjugate of the lower.
//  2. jacobi_eig (jacobi_device.h) on R. lambda_c = Re R_cc; column c has rank #{c' : lambda_c' > lambda_c, or lambda_c' = lambda_c and c' < c}.
//  3. For i < l_k, with c the column of rank i: lam = lambda_c where that is > 0, else 0; q = sqrt(lam); row r = (sum of l_k' for k' < k) + i of G:
//     G[r][a] = (q Re v_ac, -(q Im v_ac)).
//  4. B = G G^H + reg I, lower triangle: B_ij = sum_a G[i][a] conj(G[j][a]) (a ascending from the term of a = 0), B_ii = (sum_a |G[i][a]|^2) + reg.
//     mmse_ldl (mmse_device.h) gives r_i = 1 / pivot and N, the inverse of the unit lower factor. Per port a: T[i] = G[i][a] + sum_(k<i) N_ik G[k][a]
//     (mmse_lower_mul); Z[i] = T[i] r_i; X[i] = Z[i] + sum_(k>i) conj(N_ki) Z[k] (k ascending); W[a][i] = conj(X[i]).
//     Column i: n2 = sum_a |W[a][i]|^2 (a ascending from a = 0); f = amplitude / sqrt(n2); W[a][i] <- (f Re, f Im).
//     Then p = W[0][i], m2 = |p|^2, m = sqrt(m2); where m2 is a positive normal number and m >= amplitude 2^-10: e = (Re p / m, -(Im p / m)),
//     W[a][i] <- W[a][i] e (zf_mul) for a >= 1 and W[0][i] = (m, 0).
//  5. Row r: d_c = sum_a G[r][a] W[a][c] (zf_mul, a ascending from a = 0); sig = |d_r|^2; leak = sum_(c != r, c < L) |d_c|^2 from 0, c ascending.
//  6. Abnormal rule: where a pivot or an n2 is not a positive normal number, every weight of the PRG is 0 and so are sig and leak; lam stays.
// Single IEEE operations in the order written (no contraction), exact division and square root: the convention of mmse_device.h.
//
// Geometry. The job alone decides its form, so its bits never depend on the batch or on the launch: with c_k the largest number of SRS PRGs of UE k
// under one output PRG (pw_max_count), the lane form where max c_k <= 8 and the wave form otherwise. Lane kernel: workgroups of one wavefront, (job,
// y): lane t takes the output PRGs 64 y + t + 64 Y m. Wave kernel: workgroups of four wavefronts, (job, y): wavefront w takes the output PRGs 4 y + w +
// 4 Y m, every lane computes the reduced problem and lane 0 stores. Each kernel leaves the jobs of the other form alone. Y comes from the largest
// nof_prg of the host jobs of that form (a form no host job takes is not launched); device jobs get Y = 5 and 69 and the stride loop covers more.
// Everything stays in registers; loops run to the compile-time bound 4 and are predicated on A, U, L.
#include "jacobi_device.h"
#include "miphy_ext.h"
#include <algorithm>
#include <cmath>

namespace {
constexpr uint32_t PW_LANE_MAX = 8; // SRS PRGs of one UE under one output PRG in the lane form
}

// SRS PRGs of `u` under output PRG j of size S: i0..i1, and the PRB range [lo, hi) they share with it (hi == lo: none is met, one PRG of weight 1).
__host__ __device__ static inline void pw_range(const miphy_precoding_weights_ue& u, uint32_t S, uint32_t j, uint32_t& i0, uint32_t& i1, uint32_t& lo,
                                                uint32_t& hi)
{
  const uint32_t b0 = u.start_prb, b1 = b0 + u.nof_prb, sh = u.prg_size >> 1; // s = 1, 2, 4: a shift by 0, 1, 2
  const uint32_t w0 = j * S, w1 = w0 + S;
  lo = w0 > b0 ? w0 : b0, hi = w1 < b1 ? w1 : b1;
  if (hi > lo) {
    i0 = (lo - b0) >> sh, i1 = (hi - 1 - b0) >> sh;
  } else {
    i0 = i1 = w1 <= b0 ? 0u : (u.nof_prb >> sh) - 1u;
    lo = hi = 0;
  }
}

// The largest i1 - i0 + 1 over the output PRGs of the job. Between the first and the last output PRG that meet the band the count repeats with a period
// of at most four PRGs (s divides 4), so the first five and the last five of them hold every value.
__host__ __device__ static inline uint32_t pw_max_count(const miphy_precoding_weights_ue& u, uint32_t S, uint32_t nof_prg)
{
  const uint32_t j0 = u.start_prb / S;
  uint32_t       j1 = (u.start_prb + u.nof_prb - 1u) / S;
  j1                = j1 < nof_prg - 1u ? j1 : nof_prg - 1u;
  uint32_t best = 1;
  if (j1 < j0)
    return best;
  for (uint32_t d = 0; d < 5; ++d) {
    uint32_t i0, i1, lo, hi;
    if (j0 + d <= j1) {
      pw_range(u, S, j0 + d, i0, i1, lo, hi);
      best = i1 - i0 + 1u > best ? i1 - i0 + 1u : best;
    }
    if (j1 >= j0 + d) {
      pw_range(u, S, j1 - d, i0, i1, lo, hi);
      best = i1 - i0 + 1u > best ? i1 - i0 + 1u : best;
    }
  }
  return best;
}

// The rules of one job, for the host and for the kernels (device jobs the host could not check): 0, or the number of the first rule it breaks
// (PW_RULE_TEXT). nof_weights < 0: the extent of `weights` is not judged (miphy_precoding_weights_info).
__host__ __device__ static inline int miphy_pw_rule(const miphy_precoding_weights_job& j, int64_t nof_weights)
{
  if (j.nof_ues < 1 || j.nof_ues > 4)
    return 1;
  if (j.nof_ports < 1 || j.nof_ports > 4)
    return 2;
  if (j.prg_size < 1 || j.nof_prg < 1)
    return 3;
  if (!(j.reg >= 0.f && j.reg < INFINITY))
    return 4;
  if (!(j.amplitude >= 1.17549435e-38f && j.amplitude < INFINITY))
    return 5;
  uint32_t L = 0;
  int      rule = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= j.nof_ues || rule)
      continue;
    const miphy_precoding_weights_ue& u = j.ue[k];
    if (u.prg_size != 1 && u.prg_size != 2 && u.prg_size != 4)
      rule = 6;
    else if (u.nof_prb < 4 || u.nof_prb > 272 || u.nof_prb % 4 != 0 || (uint32_t)u.start_prb + u.nof_prb > 275)
      rule = 7;
    else if (u.nof_ue_ports != 1 && u.nof_ue_ports != 2 && u.nof_ue_ports != 4)
      rule = 8;
    else if (u.nof_layers < 1 || u.nof_layers > u.nof_ue_ports)
      rule = 9;
    L += u.nof_layers;
  }
  if (rule)
    return rule;
  if (L > 4 || L > j.nof_ports)
    return 10;
  if (nof_weights >= 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < j.nof_ues && (int64_t)j.ue[k].weights_offset + (int64_t)j.nof_prg * j.nof_ports * j.ue[k].nof_layers > nof_weights)
        rule = 11;
  }
  return rule;
}

__host__ __device__ static inline bool miphy_pw_wave_form(const miphy_precoding_weights_job& j, uint32_t& max_count)
{
  max_count = 1;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < j.nof_ues) {
      const uint32_t c = pw_max_count(j.ue[k], j.prg_size, j.nof_prg);
      max_count        = c > max_count ? c : max_count;
    }
  return max_count > PW_LANE_MAX;
}

namespace {

const char* const PW_RULE_TEXT[12] = {"",
                                      "nof_ues is 1..4",
                                      "nof_ports is 1..4",
                                      "prg_size and nof_prg are at least 1",
                                      "reg is finite and not negative",
                                      "amplitude is a positive normal number",
                                      "the SRS prg_size of a UE is 1, 2 or 4 PRBs",
                                      "the sounded band of a UE is a multiple of 4 PRBs in 4..272 and ends within 275 PRBs",
                                      "nof_ue_ports of a UE is 1, 2 or 4",
                                      "nof_layers of a UE is 1..nof_ue_ports",
                                      "the layers of all UEs together are at most 4 and at most nof_ports",
                                      "the weights of a UE leave `weights`"};

constexpr int PW_WAVE_THREADS = 256;
constexpr int PW_LANE_Y_DEVICE = 5, PW_WAVE_Y_DEVICE = 69; // 275 output PRGs without a second pass of the stride loop

// R of one UE under output PRG j (step 1), as a full matrix with zeros at and behind A. d: the sums of the diagonal, o[a (a - 1) / 2 + b]: of the lower triangle.
template <bool WAVE>
__device__ __forceinline__ void pw_gram(const float2* __restrict__ h, const miphy_precoding_weights_ue& u, int A, uint32_t S, uint32_t j, int lane,
                                        float2 (&r)[4][4])
{
#pragma clang fp contract(off)
  uint32_t i0, i1, lo, hi;
  pw_range(u, S, j, i0, i1, lo, hi);
  const int      U  = u.nof_ue_ports;
  const uint32_t b0 = u.start_prb, s = u.prg_size;
  float          d[4]  = {0.f, 0.f, 0.f, 0.f};
  float2         o[6];
#pragma unroll
  for (int e = 0; e < 6; ++e)
    o[e] = make_float2(0.f, 0.f);
  for (uint32_t i = i0 + (WAVE ? (uint32_t)lane : 0u); i <= i1; i += WAVE ? 64u : 1u) {
    const float2* __restrict__ hi_ = h + u.h_offset + (size_t)i * (uint32_t)(A * U);
    float2 hh[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int p = 0; p < 4; ++p)
        hh[a][p] = (a < A && p < U) ? hi_[a * U + p] : make_float2(0.f, 0.f);
    float w = 1.f;
    if (hi > lo) {
      const uint32_t p0 = b0 + i * s, p1 = p0 + s;
      w                 = (float)((p1 < hi ? p1 : hi) - (p0 > lo ? p0 : lo));
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a >= A)
        continue;
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        if (a == b) {
          float t = zf_norm(hh[a][0]);
#pragma unroll
          for (int p = 1; p < 4; ++p)
            if (p < U)
              t = t + zf_norm(hh[a][p]);
          d[a] = d[a] + w * t;
        } else {
          const float2 t = zf_dot(hh[a], hh[b], U);
          float2&      x = o[a * (a - 1) / 2 + b];
          x              = make_float2(x.x + w * t.x, x.y + w * t.y);
        }
      }
    }
  }
  if (WAVE) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
        d[a] = d[a] + __shfl_xor(d[a], off);
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        const float x = __shfl_xor(o[e].x, off), y = __shfl_xor(o[e].y, off);
        o[e]          = make_float2(o[e].x + x, o[e].y + y);
      }
    }
  }
  const float wt = hi > lo ? (float)(hi - lo) : 1.f;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      if (a == b) {
        r[a][a] = make_float2(a < A ? d[a] / wt : 0.f, 0.f);
      } else {
        const float2 x = a < A ? make_float2(o[a * (a - 1) / 2 + b].x / wt, o[a * (a - 1) / 2 + b].y / wt) : make_float2(0.f, 0.f);
        r[a][b]        = x;
        r[b][a]        = make_float2(x.x, -x.y);
      }
    }
}

// Steps 2 .. 6 for output PRG j of one job; `store` lanes write.
template <bool WAVE>
__device__ __forceinline__ void pw_prg(const miphy_precoding_weights_job* __restrict__ job, int K, int A, uint32_t S, float reg, float amplitude, uint32_t j,
                                       int lane, const float2* __restrict__ h, float2* __restrict__ weights, float* __restrict__ metrics)
{
#pragma clang fp contract(off)
  float2 gt[4][4]; // gt[a][r] = G[r][a]
  float  lam[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    lam[a] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      gt[a][r] = make_float2(0.f, 0.f);
  }
  int L = 0;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const miphy_precoding_weights_ue u = load_words(&job->ue[k]);
    float2                           R[4][4], v[4][4];
    pw_gram<WAVE>(h, u, A, S, j, lane, R);
    jacobi_eig(R, v, A);
    int rank[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      rank[c] = 0;
#pragma unroll
      for (int c2 = 0; c2 < 4; ++c2)
        if (c2 != c && c2 < A)
          rank[c] += (R[c2][c2].x > R[c][c].x || (R[c2][c2].x == R[c][c].x && c2 < c)) ? 1 : 0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= u.nof_layers)
        continue;
      float  l = 0.f;
      float2 col[4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
        col[a] = make_float2(0.f, 0.f);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < A && rank[c] == i) {
          l = R[c][c].x;
#pragma unroll
          for (int a = 0; a < 4; ++a)
            col[a] = v[a][c];
        }
      l             = l > 0.f ? l : 0.f;
      const float q = sqrtf(l);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r == L + i) {
          lam[r] = l;
#pragma unroll
          for (int a = 0; a < 4; ++a)
            gt[a][r] = make_float2(q * col[a].x, -(q * col[a].y));
        }
    }
    L += u.nof_layers;
  }

  // B = G G^H + reg I
  float2 B[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c <= i; ++c) {
      if (i == c) {
        float t = zf_norm(gt[0][i]);
#pragma unroll
        for (int a = 1; a < 4; ++a)
          if (a < A)
            t = t + zf_norm(gt[a][i]);
        B[i][i] = make_float2(t + reg, 0.f);
      } else {
        float2 t = zf_mul_conj(gt[0][i], gt[0][c]);
#pragma unroll
        for (int a = 1; a < 4; ++a)
          if (a < A) {
            const float2 x = zf_mul_conj(gt[a][i], gt[a][c]);
            t              = make_float2(t.x + x.x, t.y + x.y);
          }
        B[i][c] = t;
      }
    }
  float  rp[4];
  float2 N[6];
  bool   ok = mmse_ldl<4>(B, L, rp, N);
  float2 W[4][4]; // W[a][i]
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float2 T[4], Z[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      T[i] = make_float2(0.f, 0.f);
    mmse_lower_mul(N, L, gt[a], T);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      Z[i] = i < L ? make_float2(T[i].x * rp[i], T[i].y * rp[i]) : make_float2(0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float2 acc = Z[i];
#pragma unroll
      for (int k = i + 1; k < 4; ++k)
        if (k < L) {
          const float2 t = zf_conj_mul(N[k * (k - 1) / 2 + i], Z[k]);
          acc            = make_float2(acc.x + t.x, acc.y + t.y);
        }
      W[a][i] = (a < A && i < L) ? make_float2(acc.x, -acc.y) : make_float2(0.f, 0.f);
    }
  }
  const float floor_ = amplitude * 0.0009765625f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= L)
      continue;
    float n2 = zf_norm(W[0][i]);
#pragma unroll
    for (int a = 1; a < 4; ++a)
      if (a < A)
        n2 = n2 + zf_norm(W[a][i]);
    ok            = ok && mmse_pos_normal(n2);
    const float f = amplitude / sqrtf(n2);
#pragma unroll
    for (int a = 0; a < 4; ++a)
      W[a][i] = make_float2(f * W[a][i].x, f * W[a][i].y);
    const float2 p  = W[0][i];
    const float  m2 = zf_norm(p), m = sqrtf(m2);
    if (mmse_pos_normal(m2) && m >= floor_) {
      const float2 e = make_float2(p.x / m, -(p.y / m));
#pragma unroll
      for (int a = 1; a < 4; ++a)
        W[a][i] = zf_mul(W[a][i], e);
      W[0][i] = make_float2(m, 0.f);
    }
  }
  float sig[4], leak[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sig[r] = 0.f, leak[r] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= L)
        continue;
      float2 dd = zf_mul(gt[0][r], W[0][c]);
#pragma unroll
      for (int a = 1; a < 4; ++a)
        if (a < A) {
          const float2 t = zf_mul(gt[a][r], W[a][c]);
          dd             = make_float2(dd.x + t.x, dd.y + t.y);
        }
      const float e = zf_norm(dd);
      if (c == r)
        sig[r] = e;
      else
        leak[r] = leak[r] + e;
    }
  }

  if (WAVE && lane != 0)
    return;
  int row0 = 0;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const miphy_precoding_weights_ue u = load_words(&job->ue[k]);
    const int                        l = u.nof_layers;
    float2* __restrict__ wo = weights + u.weights_offset + (size_t)j * (uint32_t)(A * l);
    float* __restrict__ mo  = metrics ? metrics + u.metrics_offset + (size_t)j * (uint32_t)(3 * l) : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = r - row0;
      if (i < 0 || i >= l)
        continue;
#pragma unroll
      for (int a = 0; a < 4; ++a)
        if (a < A)
          wo[a * l + i] = ok ? W[a][r] : make_float2(0.f, 0.f);
      if (mo) {
        mo[3 * i]     = lam[r];
        mo[3 * i + 1] = ok ? sig[r] : 0.f;
        mo[3 * i + 2] = ok ? leak[r] : 0.f;
      }
    }
    row0 += l;
  }
}

// The header of a job and whether this kernel takes it.
template <bool WAVE>
__device__ __forceinline__ bool pw_take(const miphy_precoding_weights_job* __restrict__ job, uint32_t nof_weights, miphy_precoding_weights_job& j)
{
  j = load_words(job);
  if (miphy_pw_rule(j, (int64_t)nof_weights) != 0) // a device job the host could not check: nothing is written
    return false;
  uint32_t mc;
  return miphy_pw_wave_form(j, mc) == WAVE;
}

__global__ void __launch_bounds__(64) precoding_weights_lane_kernel(const miphy_precoding_weights_job* __restrict__ jobs, const float2* __restrict__ h,
                                                                    float2* __restrict__ weights, uint32_t nof_weights, float* __restrict__ metrics)
{
  const miphy_precoding_weights_job* job = jobs + blockIdx.x;
  miphy_precoding_weights_job        j;
  if (!pw_take<false>(job, nof_weights, j)) // uniform
    return;
  for (uint32_t p = blockIdx.y * 64u + threadIdx.x; p < j.nof_prg; p += gridDim.y * 64u)
    pw_prg<false>(job, j.nof_ues, j.nof_ports, j.prg_size, j.reg, j.amplitude, p, (int)threadIdx.x, h, weights, metrics);
}

__global__ void __launch_bounds__(PW_WAVE_THREADS) precoding_weights_wave_kernel(const miphy_precoding_weights_job* __restrict__ jobs,
                                                                                 const float2* __restrict__ h, float2* __restrict__ weights,
                                                                                 uint32_t nof_weights, float* __restrict__ metrics)
{
  const miphy_precoding_weights_job* job = jobs + blockIdx.x;
  miphy_precoding_weights_job        j;
  if (!pw_take<true>(job, nof_weights, j)) // uniform
    return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t p = blockIdx.y * 4u + wave; p < j.nof_prg; p += gridDim.y * 4u) // uniform per wavefront
    pw_prg<true>(job, j.nof_ues, j.nof_ports, j.prg_size, j.reg, j.amplitude, p, lane, h, weights, metrics);
}

// The rules of one job on the host: MIPHY_EINVAL with the text of the first rule it breaks in miphy_last_error().
int pw_check(const char* who, uint32_t i, const miphy_precoding_weights_job& j, int64_t nof_weights)
{
  const int rule = miphy_pw_rule(j, nof_weights);
  MIPHY_REQUIRE(rule == 0, "%s: job %u: %s", who, i, PW_RULE_TEXT[rule]);
  return MIPHY_OK;
}

} // namespace

extern "C" int miphy_precoding_weights_info(const miphy_precoding_weights_job* job, miphy_precoding_weights_info_t* out)
{
  MIPHY_REQUIRE(job && out, "miphy_precoding_weights_info: null argument");
  if (const int rc = pw_check("miphy_precoding_weights_info", 0, *job, -1))
    return rc;
  *out = miphy_precoding_weights_info_t{};
  for (int k = 0; k < job->nof_ues; ++k) {
    out->nof_layers += job->ue[k].nof_layers;
    out->nof_weights[k] = (uint32_t)job->nof_prg * job->nof_ports * job->ue[k].nof_layers;
    out->nof_metrics[k] = 3u * job->nof_prg * job->ue[k].nof_layers;
  }
  out->wave_form = miphy_pw_wave_form(*job, out->max_srs_prg) ? 1u : 0u;
  return MIPHY_OK;
}

extern "C" int miphy_precoding_weights_batch(miphy_ctx* ctx, const miphy_precoding_weights_job* jobs, int jobs_on_device, uint32_t n, const float* h,
                                             float* weights, uint32_t nof_weights, float* metrics, void* stream)
{
  static const char* const who = "miphy_precoding_weights_batch";
  MIPHY_REQUIRE(ctx && jobs && h && weights, "%s: null argument", who);
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(n <= (1u << 24), "%s: at most 2^24 jobs per call", who);
  // Host jobs: every one is checked before anything is enqueued, and each kernel's grid follows the largest nof_prg of the jobs of its form.
  uint32_t y_lane = PW_LANE_Y_DEVICE, y_wave = PW_WAVE_Y_DEVICE;
  if (!jobs_on_device) {
    y_lane = y_wave = 0;
    for (uint32_t i = 0; i < n; ++i) {
      if (const int rc = pw_check(who, i, jobs[i], (int64_t)nof_weights))
        return rc;
      uint32_t mc;
      if (miphy_pw_wave_form(jobs[i], mc))
        y_wave = std::max(y_wave, (jobs[i].nof_prg + 3u) / 4u);
      else
        y_lane = std::max(y_lane, (jobs[i].nof_prg + 63u) / 64u);
    }
  }
  hipStream_t s      = (hipStream_t)stream;
  const void* d_jobs = nullptr;
  if (const int rc = miphy_stage_descs(ctx, jobs, jobs_on_device, sizeof(miphy_precoding_weights_job) * (size_t)n, s, &d_jobs))
    return rc;
  if (y_lane) {
    hipLaunchKernelGGL(precoding_weights_lane_kernel, dim3(n, y_lane), dim3(64), 0, s, (const miphy_precoding_weights_job*)d_jobs, (const float2*)h,
                       (float2*)weights, nof_weights, metrics);
    MIPHY_HIP_CHECK(hipGetLastError());
  }
  if (y_wave) {
    hipLaunchKernelGGL(precoding_weights_wave_kernel, dim3(n, y_wave), dim3(PW_WAVE_THREADS), 0, s, (const miphy_precoding_weights_job*)d_jobs,
                       (const float2*)h, (float2*)weights, nof_weights, metrics);
    MIPHY_HIP_CHECK(hipGetLastError());
  }
  return MIPHY_OK;
}
