// Fixture driver for tests/golden/short_block_detector.npz: runs the reference's short-block detector, obtained through its public
// factory (create_short_block_detector_factory_sw), on stimuli read from stdin and writes its verdicts to stdout. Built and run by
// tools/gen_short_block_golden.py against the reference library that build() compiles into oracle/_ref/.
//
// stdin:  uint32 n, then n records {uint32 K, uint32 bits_per_symbol, uint32 E, int8 llr[E]}
// stdout: n records {uint8 payload[K], uint8 valid}
#include "srsran/phy/upper/channel_coding/channel_coding_factories.h"
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace srsran;

static void read_exact(void* p, size_t n)
{
  if (fread(p, 1, n, stdin) != n) {
    fprintf(stderr, "gen_short_block_golden: short read\n");
    std::exit(1);
  }
}

int main()
{
  std::shared_ptr<short_block_detector_factory> factory  = create_short_block_detector_factory_sw();
  std::unique_ptr<short_block_detector>         detector = factory->create();

  uint32_t n = 0;
  read_exact(&n, sizeof(n));
  std::vector<int8_t>               raw;
  std::vector<log_likelihood_ratio> llr;
  std::vector<uint8_t>              payload;
  for (uint32_t i = 0; i != n; ++i) {
    uint32_t hdr[3];
    read_exact(hdr, sizeof(hdr));
    const uint32_t K = hdr[0], Qm = hdr[1], E = hdr[2];
    raw.resize(E);
    read_exact(raw.data(), E);
    llr.assign(raw.begin(), raw.end());
    payload.assign(K, 0);
    const bool valid = detector->detect(payload, llr, static_cast<modulation_scheme>(Qm));
    payload.push_back(valid ? 1 : 0);
    fwrite(payload.data(), 1, payload.size(), stdout);
  }
  return 0;
}
