// OFDM PRACH demodulator: srsran::ofdm_prach_demodulator_impl::demodulate (ofdm_prach_demodulator_impl.cpp:31-199) for a batch of
// windows. The host expands the jobs (prach_demod_geometry, prach_info.h) into symbol tasks, one per (window, time-domain occasion,
// symbol): the first sample after the cyclic prefix, the DFT size N, the row of frequency-domain occasion 0 in the PRACH buffer and, per
// frequency-domain occasion, the DFT bin of its first subcarrier, (k_start - grid / 2) mod N -- the lower half of the PRACH grid is the
// top of the spectrum, so a sequence that straddles the middle of the grid runs from bin N - 1 on to bin 0. Tasks are grouped by N, one
// launch (or pair of launches) per size of the call and per piece of at most 1 MiB of task table, each with the LDS and the twiddle
// tables of its size:
//  - N <= 4096: one workgroup per task loads the N samples into LDS, runs fft_lds<false> and copies the L bins of every occasion
//    straight into its row;
//  - N >= 4608: the four-step transform. Step 1 is the one of miphy_dft_batch (fft_device.h): A[k1][n2] of every task in the
//    context's workspace. Step 2 produces only the bins k = k1 + N1 k2 the occasions ask for and writes them into their rows: a
//    workgroup takes 16 rows k1 of A (one contiguous block) into LDS and evaluates, for each row, the ceil(L / N1) + 1 values of k2 an
//    occasion can reach (modulo N2: the range wraps when the sequence straddles bin 0) as direct sums over n2, four partial sums
//    each. The N-point spectrum is never written.
#include "fft_device.h"
#include "miphy_ext.h"
#include "prach_info.h"
#include <algorithm>
#include <map>
#include <vector>

extern "C" int miphy_prach_demod_info(uint32_t sampling_rate_hz, const miphy_prach_demod_job* job, miphy_prach_demod_info_t* out)
{
  MIPHY_REQUIRE(job && out, "miphy_prach_demod_info: null argument");
  return prach_demod_geometry(sampling_rate_hz, *job, *out);
}

namespace {

struct prach_demod_task {
  uint64_t src;       // cf_t offset in `samples` of the symbol's first sample (first member: step 1 reads it as its offset table)
  uint64_t dst;       // cf_t offset in `buffer` of the row (td, fd 0, symbol)
  uint32_t N, L, nfd; // DFT size, sequence length, frequency-domain occasions
  uint32_t fd_stride; // cf_t between the rows of consecutive frequency-domain occasions (max_nof_symbols L)
  uint32_t bin0[MIPHY_PRACH_MAX_FD_OCCASIONS]; // DFT bin of sequence element 0
};
static_assert(sizeof(prach_demod_task) == 64 && sizeof(prach_demod_task) % sizeof(uint64_t) == 0, "task layout");

__global__ void __launch_bounds__(512)
prach_demod_lds_kernel(const prach_demod_task* __restrict__ tasks, const float2* __restrict__ samples, float2* __restrict__ buffer, const cplx* __restrict__ tw)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cplx*                  x   = reinterpret_cast<cplx*>(smem);
  const prach_demod_task t   = load_words(tasks + blockIdx.x);
  const int              N   = (int)t.N;
  const float2*          src = samples + t.src;
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const float2 v = src[i];
    x[fpad(i)]     = {v.x, v.y};
  }
  __syncthreads();
  fft_lds<false>(x, N, tw, threadIdx.x, blockDim.x);
  for (uint32_t fd = 0; fd < t.nfd; ++fd) {
    float2* dst = buffer + t.dst + (size_t)fd * t.fd_stride;
    for (uint32_t i = threadIdx.x; i < t.L; i += blockDim.x) {
      uint32_t bin = tasks[blockIdx.x].bin0[fd] + i; // from memory: a register array indexed by fd would live in scratch
      if (bin >= t.N)
        bin -= t.N;
      const cplx v = x[fpad((int)bin)];
      dst[i]       = make_float2(v.x, v.y);
    }
  }
}

// Step 2 of the four-step transform for the bins of the occasions only. grid = (N1 / 16, tasks of this size), 256 threads.
// Item (r, fd, m): row k1 = 16 blockIdx.x + r, k2 = (bin0[fd] / N1 + m) mod N2, m < M = ceil(L / N1) + 1; it is sequence element
// i = (k1 + N1 k2 - bin0[fd]) mod N when that is below L. The 16 lanes of one (fd, m) hold consecutive k1, so consecutive i: a
// 128-byte store; they share k2, so the twiddle read is a broadcast, and their 16 rows of A lie an odd number of elements apart in LDS.
__global__ void __launch_bounds__(256)
prach_demod_fs_step2_kernel(const prach_demod_task* __restrict__ tasks, const float2* __restrict__ tmp, float2* __restrict__ buffer,
                            const cplx* __restrict__ tw2, int N1, int N2)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cplx*                  a      = reinterpret_cast<cplx*>(smem); // [16][N2 + 1]
  const int              stride = N2 + 1;
  cplx*                  w      = a + FS_TILE * stride;          // [N2]: exp(-2 pi i j / N2)
  const prach_demod_task t      = load_words(tasks + blockIdx.y);
  const uint32_t         N      = (uint32_t)N1 * (uint32_t)N2;
  const int              r0     = blockIdx.x * FS_TILE;
  const float2*          src    = tmp + (size_t)blockIdx.y * N + (size_t)r0 * N2; // rows r0 .. r0 + 15 of A: one contiguous block
  for (int i = threadIdx.x; i < FS_TILE * N2; i += blockDim.x) {
    const float2 v              = src[i];
    a[(i / N2) * stride + i % N2] = {v.x, v.y};
  }
  for (int i = threadIdx.x; i < N2; i += blockDim.x)
    w[i] = tw2[i];
  __syncthreads();
  const uint32_t M     = (t.L + (uint32_t)N1 - 1) / (uint32_t)N1 + 1;
  const uint32_t items = FS_TILE * t.nfd * M;
  for (uint32_t it = threadIdx.x; it < items; it += blockDim.x) {
    const uint32_t r = it % FS_TILE, c = it / FS_TILE, fd = c / M, m = c % M;
    const uint32_t bin0 = tasks[blockIdx.y].bin0[fd];
    uint32_t       k2   = bin0 / (uint32_t)N1 + m;
    if (k2 >= (uint32_t)N2)
      k2 -= (uint32_t)N2;
    const uint32_t k = (uint32_t)r0 + r + (uint32_t)N1 * k2;
    const uint32_t i = k >= bin0 ? k - bin0 : k + N - bin0;
    if (i >= t.L)
      continue;
    // X[k] = sum_n2 A[k1][n2] W_N2^(n2 k2): n2 = 4 q + p feeds partial sum p, its twiddle index advancing by 4 k2 mod N2 (N2 % 4 == 0)
    const cplx* row = a + r * stride;
    cplx        acc[4];
    uint32_t    idx[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      acc[p] = cplx{0.f, 0.f}, idx[p] = ((uint32_t)p * k2) % (uint32_t)N2;
    const uint32_t step = (4u * k2) % (uint32_t)N2;
    for (int n2 = 0; n2 < N2; n2 += 4) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        acc[p] += cmul(row[n2 + p], w[idx[p]]);
        idx[p] += step;
        if (idx[p] >= (uint32_t)N2)
          idx[p] -= (uint32_t)N2;
      }
    }
    const cplx v = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    buffer[t.dst + (size_t)fd * t.fd_stride + i] = make_float2(v.x, v.y);
  }
}

int threads_for(uint32_t N) // as the batched DFT: one radix-8 butterfly per thread where the workgroup size allows
{
  const int nt = (int)((N / 8 + 63) / 64) * 64;
  return nt < 64 ? 64 : (nt > 512 ? 512 : nt);
}

} // namespace

extern "C" int miphy_prach_demodulate_batch(miphy_ctx* ctx, uint32_t sampling_rate_hz, const miphy_prach_demod_job* jobs, uint32_t n, const float* samples,
                                            float* buffer, void* stream)
{
  if (n == 0)
    return MIPHY_OK;
  MIPHY_REQUIRE(ctx && jobs && samples && buffer, "miphy_prach_demodulate_batch: null argument");
  // Tasks by DFT size, in job order within a size.
  std::map<uint32_t, std::vector<prach_demod_task>> by_size;
  for (uint32_t i = 0; i < n; ++i) {
    const miphy_prach_demod_job& j = jobs[i];
    miphy_prach_demod_info_t     g;
    const int                    rc = prach_demod_geometry(sampling_rate_hz, j, g);
    if (rc)
      return rc; // the message names the rule; nothing has been enqueued
    const uint32_t grid = j.nof_prb_ul_grid * g.K * 12u; // below dft_size (checked in 64 bits)
    prach_demod_task t  = {};
    t.N = g.dft_size, t.L = g.L, t.nfd = j.nof_fd_occasions, t.fd_stride = j.max_nof_symbols * g.L; // strides <= 65535
    for (uint32_t fd = 0; fd < j.nof_fd_occasions; ++fd)
      t.bin0[fd] = g.k_start[fd] < grid / 2 ? g.dft_size - grid / 2 + g.k_start[fd] : g.k_start[fd] - grid / 2;
    std::vector<prach_demod_task>& v = by_size[g.dft_size];
    for (uint32_t td = 0; td < j.nof_td_occasions; ++td)
      for (uint32_t sym = 0; sym < g.nof_symbols; ++sym) {
        t.src = j.samples_offset + g.td_sample_offset[td] + g.td_cp_samples[td] + (uint64_t)sym * g.dft_size;
        t.dst = j.buffer_offset + (((uint64_t)td * j.max_nof_fd_occasions) * j.max_nof_symbols + sym) * g.L;
        v.push_back(t);
      }
  }
  // A piece = the tasks of one size that one staging and one launch (pair) take: at most 1 MiB of table (well inside the ring and inside
  // grid.y), and for the four-step sizes at most 64 MiB of A[k1][n2] -- 341 symbols of 24576 points put 4092 workgroups on step 1, far more
  // than the chip holds at once, so a larger piece buys nothing and the workspace, which is never given back, stays bounded.
  constexpr size_t PIECE_TASKS = (1u << 20) / sizeof(prach_demod_task), FS_SCRATCH = 64u << 20;
  auto piece_of = [&](uint32_t N) { return N <= 4096 ? PIECE_TASKS : std::min(PIECE_TASKS, std::max<size_t>(1, FS_SCRATCH / ((size_t)N * sizeof(float2)))); };
  size_t fs_scratch = 0;
  for (const auto& kv : by_size)
    if (kv.first > 4096)
      fs_scratch = std::max(fs_scratch, std::min(kv.second.size(), piece_of(kv.first)) * kv.first * sizeof(float2));
  hipStream_t s   = (hipStream_t)stream;
  void*       tmp = nullptr;
  int         rc;
  if (fs_scratch && (rc = miphy_get_workspace(ctx, MIPHY_WS_GENERAL, fs_scratch, &tmp)))
    return rc;
  for (const auto& kv : by_size) {
    const uint32_t N = kv.first;
    uint32_t       N1 = 0, N2 = 0;
    const float *  tw = nullptr, *tw1 = nullptr, *tw2 = nullptr;
    if (N <= 4096) {
      if ((rc = miphy_get_twiddles(ctx, N, &tw)))
        return rc;
    } else {
      if (!miphy_four_step_factors(N, N1, N2)) {
        miphy_set_error("prach_demod: DFT size %u has no four-step factors", N);
        return MIPHY_EUNSUPP;
      }
      if ((rc = miphy_get_twiddles(ctx, N1, &tw1)) || (rc = miphy_get_twiddles(ctx, N2, &tw2)) || (rc = miphy_get_twiddles(ctx, N, &tw)))
        return rc;
    }
    const size_t piece = piece_of(N);
    for (size_t c0 = 0; c0 < kv.second.size(); c0 += piece) { // the pieces share the scratch: the stream orders them
      const uint32_t nc = (uint32_t)std::min(piece, kv.second.size() - c0);
      const void*    dv = nullptr;
      if ((rc = miphy_stage_descs(ctx, kv.second.data() + c0, 0, nc * sizeof(prach_demod_task), s, &dv)))
        return rc;
      const prach_demod_task* d = (const prach_demod_task*)dv;
      if (N <= 4096) {
        hipLaunchKernelGGL(prach_demod_lds_kernel, dim3(nc), dim3(threads_for(N)), fft_lds_bytes(N), s, d, (const float2*)samples, (float2*)buffer,
                           (const cplx*)tw);
      } else {
        const size_t lds1 = FS_TILE * fft_lds_bytes(N1), lds2 = ((size_t)FS_TILE * (N2 + 1) + N2) * sizeof(cplx);
        hipLaunchKernelGGL(dft_fs_step1_kernel<false>, dim3(N2 / FS_TILE, nc), dim3(256), lds1, s, (const float2*)samples, (float2*)tmp, (const cplx*)tw1,
                           (const cplx*)tw, (int)N1, (int)N2, (const uint64_t*)d, (uint32_t)(sizeof(prach_demod_task) / sizeof(uint64_t)));
        hipLaunchKernelGGL(prach_demod_fs_step2_kernel, dim3(N1 / FS_TILE, nc), dim3(256), lds2, s, d, (const float2*)tmp, (float2*)buffer,
                           (const cplx*)tw2, (int)N1, (int)N2);
      }
      MIPHY_HIP_CHECK(hipGetLastError());
    }
  }
  return MIPHY_OK;
}
