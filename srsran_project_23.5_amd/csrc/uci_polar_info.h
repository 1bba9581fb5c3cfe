// Framing of a polar-coded UCI field (TS 38.212 6.3.1.2-6.3.1.5 and 6.3.2 with 5.2.1 and 5.3.1), stated once for miphy_uci_polar_info,
// the host planner of uci_polar.hip and the job builder of uci.hip. The kernel does not frame anything itself: it takes the pad bit
// from its task record and the CRC length from its code block. The 23.5 reference decodes no such field (uci_decoder_impl.cpp:44); it sizes
// them in lib/ran/pusch/ulsch_info.cpp:29-42 (6 CRC bits from 12 bits, 11 from 20), which is the L below.
#pragma once
#include "miphy_internal.h"

enum { UCI_POLAR_MIN_BITS = MIPHY_UCI_POLAR_MIN_BITS, UCI_POLAR_MAX_BITS = MIPHY_UCI_POLAR_MAX_BITS, UCI_POLAR_E_MAX = 8192 };
enum { UCI_POLAR_CRC6_POLY = 0x61, UCI_POLAR_CRC11_POLY = 0xE21 }; // crc_calculator's CRC6 and CRC11, top bit included

struct uci_polar_framing {
  uint32_t C;     // segments (5.2.1): 2 if (A >= 360 and E >= 1088) or A >= 1013
  uint32_t L;     // CRC bits of a segment (6.3.1.2.1): 6 up to 19 bits, 11 from 20 bits
  uint32_t A_seg; // payload bits of a segment, A' / C with A' = ceil(A / C) C
  uint32_t pad;   // 1: a zero bit in front of the first segment (C = 2, odd A)
  uint32_t K_r;   // A_seg + L
  uint32_t E_r;   // floor(E / C): segment r owns soft bits [r E_r, (r + 1) E_r)
  uint32_t nPC;   // 3 for K_r <= 25 (5.3.1.2), else 0
};
enum uci_polar_rule { UCI_POLAR_OK = 0, UCI_POLAR_RULE_BITS, UCI_POLAR_RULE_RATE, UCI_POLAR_RULE_EMAX };

__host__ __device__ inline uci_polar_rule uci_polar_frame(uint32_t A, uint32_t E, uci_polar_framing& f)
{
  f = uci_polar_framing();
  if (A < UCI_POLAR_MIN_BITS || A > UCI_POLAR_MAX_BITS)
    return UCI_POLAR_RULE_BITS;
  f.C     = ((A >= 360 && E >= 1088) || A >= 1013) ? 2u : 1u;
  f.L     = (A <= 19) ? 6u : 11u;
  f.A_seg = (A + f.C - 1) / f.C;
  f.pad   = f.A_seg * f.C - A;
  f.K_r   = f.A_seg + f.L;
  f.E_r   = E / f.C;
  f.nPC   = (f.K_r <= 25) ? 3u : 0u;
  if (!(f.K_r + f.nPC < f.E_r))
    return UCI_POLAR_RULE_RATE;
  if (f.E_r > UCI_POLAR_E_MAX)
    return UCI_POLAR_RULE_EMAX;
  return UCI_POLAR_OK;
}

// The CRC length of a segment from its polar message length alone: K_r = 18..25 only arises from 12..19 payload bits + CRC6 (a field of
// 20 bits or more has K_r >= 31, and a two-segment field K_r >= 191), so (K_r, E_r) identifies a code block together with its CRC.
__host__ __device__ inline uint32_t uci_polar_crc_bits_of_K(uint32_t K_r)
{
  return K_r <= 25 ? 6u : 11u;
}

// Host: the framing, or MIPHY_EINVAL with the rule that refuses the field in miphy_last_error().
inline int uci_polar_frame_or_error(const char* who, uint32_t idx, uint32_t A, uint32_t E, uci_polar_framing& f)
{
  const uci_polar_rule r = uci_polar_frame(A, E, f);
  MIPHY_REQUIRE(r != UCI_POLAR_RULE_BITS, "%s: field %u: %u bits (a polar-coded UCI field has 12 to 1706 bits)", who, idx, A);
  MIPHY_REQUIRE(r != UCI_POLAR_RULE_RATE, "%s: field %u: %u bits in %u soft bits: K_r + nPC < E_r does not hold (K_r = %u, nPC = %u, E_r = %u)", who, idx,
                A, E, f.K_r, f.nPC, f.E_r);
  MIPHY_REQUIRE(r != UCI_POLAR_RULE_EMAX, "%s: field %u: %u bits in %u soft bits: E_r = %u exceeds 8192", who, idx, A, E, f.E_r);
  return MIPHY_OK;
}
