// Device code shared by the polar decoding kernels (polar.hip, uci_polar.hip): the reference's LLR algebra, the rate dematcher as a
// gather, the pruned SSC schedule run by the lanes of one codeword on its LDS slice, and the list recursion run by one wavefront.
#pragma once
#include "polar_code.h"

// LLR algebra of log_likelihood_ratio.cpp:38-85 / .h:208-216.
__device__ __forceinline__ int llr_add(int a, int b)
{ // a + b (special cases inspect the right operand first, like `rhs += *this`)
  if (b == -a)
    return 0;
  if (b > 120 || b < -120)
    return b;
  if (a > 120 || a < -120)
    return a;
  return min(max(a + b, -120), 120);
}
__device__ __forceinline__ int llr_promotion_sum(int a, int b)
{
  if (a == -b)
    return 0;
  if (a > 120 || a < -120)
    return a;
  if (b > 120 || b < -120)
    return b;
  const int t = a + b;
  return (t > 120) ? 127 : ((t < -120) ? -127 : t);
}
__device__ __forceinline__ int llr_soft_xor(int x, int y)
{
  const int m = min(abs(x), abs(y));
  return (x * y < 0) ? -m : m;
}

// Rate dematching (polar_rate_dematcher_impl.cpp:29-118) of one codeword position as a gather: `first` is the position's rx_first
// entry, repetitions are accumulated in order.
__device__ __forceinline__ int polar_dematch_value(int first, int N, int E, const int8_t* __restrict__ f, const uint16_t* __restrict__ rx_fidx)
{
  if (first == -1)
    return 0;
  if (first == -2)
    return 127;
  int v = f[rx_fidx[first]];
  for (int k = first + N; k < E; k += N)
    v = llr_promotion_sum(v, f[rx_fidx[k]]);
  return v;
}

// The pruned SSC schedule (polar_decoder_impl.cpp:179-350) run by the W lanes of one codeword: L holds the stage-s LLRs at offset 2^s
// (the channel LLRs at N), est the partial sums, u the decisions; est and u start at zero. Every codeword of a workgroup runs the same
// schedule, so the barriers are uniform; the last one leaves u complete for every lane.
template <int W>
__device__ __forceinline__ void polar_ssc_run(int8_t* L, uint8_t* est, uint8_t* u, const uint32_t* __restrict__ sched, uint32_t sched_len, int lane)
{
  for (uint32_t k = 0; k < sched_len; ++k) {
    const uint32_t op   = sched[k];
    const int      type = op & 15, s = (op >> 4) & 15, pos = (int)(op >> 8);
    const int      size = 1 << s, half = size >> 1;
    int8_t*        ls   = L + size;
    int8_t*        lc   = L + half;
    if (type == POLAR_SSC_F) {
      for (int i = lane; i < half; i += W)
        lc[i] = (int8_t)llr_soft_xor(ls[i], ls[i + half]);
    } else if (type == POLAR_SSC_G) {
      for (int i = lane; i < half; i += W) {
        const int x = ls[i], y = ls[i + half];
        lc[i]       = (int8_t)(est[pos + i] ? llr_add(y, -x) : llr_add(y, x));
      }
    } else if (type == POLAR_SSC_R1) {
      for (int i = lane; i < size; i += W) {
        const uint8_t b = ls[i] <= 0;
        est[pos + i]    = b;
        u[pos + i]      = b;
      }
      __syncthreads();
      for (int h = 1; h < size; h <<= 1) { // re-encode the subtree (polar_decoder_impl.cpp:243-248)
        for (int t = lane; t < half; t += W) {
          const int b = ((t / h) * 2 * h) + (t % h);
          u[pos + b] ^= u[pos + b + h];
        }
        __syncthreads();
      }
    } else { // POLAR_SSC_COMB
      for (int i = lane; i < half; i += W)
        est[pos + i] ^= est[pos + half + i];
    }
    __syncthreads();
  }
}

// LDS of the list decoder for one codeword: channel LLRs [N] + two banks (current / scratch) of L paths x {llr[N], bl[N], u[N]} + path
// metrics [8] + selection scratch [24] + the information-set flags and rate-0 block exponents [2N].
__host__ __device__ inline size_t polar_scl_lds_bytes(uint32_t N, uint32_t L)
{
  return (size_t)N + 2 * (size_t)L * 3 * N + 8 * 4 + 24 * 4 + 2 * N + 64;
}

// The list recursion of orc_polar_scl_decode run by the 64 lanes of one wavefront (a workgroup of its own) on the LDS of one codeword.
//   ch: channel LLRs [N]; P, Q: the two banks, 3N bytes per path: llr (stage s node LLRs at offset 2^s, s < n), bl (left-child partial
//   sums of stage s at offset 2^s), u (decisions); pm: path metrics [8], zero on entry; sel: parent[8], bit[8], spare[8];
//   kset: [0, N) information-set flags, [N, 2N) rate-0 block exponents (polar_build_list_flags).
// All L paths advance together: a stage of size 2^s over `active` paths is one flat loop over active * 2^s lanes' worth of elements;
// forking ranks the 2 * active candidates with wavefront shuffles and copies the survivors bank to bank. Returns the number of
// survivors; they lie in P (which the banks' swaps may have exchanged with Q) in slot order, their metrics in pm.
__device__ __forceinline__ int polar_scl_run(const int8_t* ch, uint8_t*& P, uint8_t*& Q, int* pm, int* sel, const uint8_t* kset, int N, int n, int L, int lane)
{
  const int PSZ    = 3 * N; // bytes per path
  int       active = 1;
  for (int i = 0; i < N;) {
    // An aligned all-frozen block [i, i + 2^r) (rate-0 node) is processed at stage r in one step: its penalty is the sum of the
    // negative stage-r LLRs, its bits and partial sums are zero.
    const int r = kset[N + i], B = 1 << r;
    // ---- stage-r LLRs
    int t = n;
    if (i != 0) {
      t = __ffs(i) - 1;
      const int sz = 1 << t;
      for (int idx = lane; idx < active * sz; idx += 64) {
        const int     q = idx >> t, j = idx & (sz - 1);
        uint8_t*      a  = P + q * PSZ;
        const int8_t* up = (t + 1 == n) ? ch : reinterpret_cast<int8_t*>(a) + 2 * sz;
        const int     x = up[j], y = up[j + sz];
        reinterpret_cast<int8_t*>(a)[sz + j] = (int8_t)(a[N + sz + j] ? llr_add(y, -x) : llr_add(y, x));
      }
      __syncthreads();
    }
    for (int s = t - 1; s >= r; --s) {
      const int sz = 1 << s;
      for (int idx = lane; idx < active * sz; idx += 64) {
        const int     q = idx >> s, j = idx & (sz - 1);
        int8_t*       a  = reinterpret_cast<int8_t*>(P + q * PSZ);
        const int8_t* up = (s + 1 == n) ? ch : a + 2 * sz;
        a[sz + j]        = (int8_t)llr_soft_xor(up[j], up[j + sz]);
      }
      __syncthreads();
    }
    // ---- decision
    if (!kset[i]) {
      for (int idx = lane; idx < active * B; idx += 64) {
        const int q = idx >> r, j = idx & (B - 1);
        const int v = (r == n) ? ch[j] : reinterpret_cast<int8_t*>(P + q * PSZ)[B + j];
        P[q * PSZ + 2 * N + i + j] = 0;
        if (v < 0)
          atomicAdd(&pm[q], -v);
      }
      __syncthreads();
    } else {
      const int nc = 2 * active, keep = min(nc, L);
      int       met = 0x7fffffff, bit = 0;
      if (lane < nc) {
        const int q = lane >> 1, l0 = reinterpret_cast<int8_t*>(P + q * PSZ)[1];
        const int hard = l0 <= 0, al = abs(l0);
        met = pm[q] + ((lane & 1) ? al : 0);
        bit = (lane & 1) ? !hard : hard;
      }
      int rank = 0;
      for (int o = 0; o < nc; ++o) {
        const int mo = __shfl(met, o);
        rank += (mo < met) || (mo == met && o < lane);
      }
      __syncthreads(); // pm[] has been read by everyone
      if (lane < nc && rank < keep) {
        sel[rank]      = lane >> 1;
        sel[8 + rank]  = bit;
        pm[rank]       = met;
      }
      __syncthreads();
      // survivors: bank P (parent) -> bank Q (slot), 16 bytes per lane per step
      const int vec_per_path = PSZ >> 4;
      for (int idx = lane; idx < keep * vec_per_path; idx += 64) {
        const int r = idx / vec_per_path, v = idx - r * vec_per_path;
        reinterpret_cast<uint4*>(Q + r * PSZ)[v] = reinterpret_cast<const uint4*>(P + sel[r] * PSZ)[v];
      }
      __syncthreads();
      if (lane < keep)
        Q[lane * PSZ + 2 * N + i] = (uint8_t)sel[8 + lane];
      uint8_t* tmp = P;
      P            = Q;
      Q            = tmp;
      active       = keep;
      __syncthreads();
    }
    // ---- partial sums of the finished block at stage r (bank Q's u area serves as the per-path working vector)
    if (!((i >> r) & 1)) {
      for (int idx = lane; idx < active * B; idx += 64) {
        const int q = idx >> r, j = idx & (B - 1);
        P[q * PSZ + N + B + j] = P[q * PSZ + 2 * N + i + j];
      }
    } else {
      for (int idx = lane; idx < active * B; idx += 64) {
        const int q = idx >> r, j = idx & (B - 1);
        Q[q * PSZ + 2 * N + j] = P[q * PSZ + 2 * N + i + j];
      }
      __syncthreads();
      int sz = B, s = r;
      while (s < n && ((i >> s) & 1)) {
        for (int idx = lane; idx < active * sz; idx += 64) {
          const int q = idx >> s, j = idx & (sz - 1);
          uint8_t*  cur = Q + q * PSZ + 2 * N;
          const uint8_t c0 = cur[j];
          cur[sz + j]      = c0;
          cur[j]           = c0 ^ P[q * PSZ + N + sz + j];
        }
        __syncthreads();
        sz <<= 1;
        ++s;
      }
      if (s < n) {
        for (int idx = lane; idx < active * sz; idx += 64) {
          const int q = idx >> s, j = idx & (sz - 1);
          P[q * PSZ + N + sz + j] = Q[q * PSZ + 2 * N + j];
        }
      }
    }
    __syncthreads();
    i += B;
  }
  return active;
}
