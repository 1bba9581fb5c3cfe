"""CPU: the device-image builder (csrc/device_image.h) that lays out every plan buffer and TB-level workspace. A stand-alone program that
includes only that header is compiled with g++ under the address and undefined-behaviour sanitizers and run: offsets, alignment, byte
counts, contents of the staged part, pointer resolution and the refusal of a put behind a reserved region. The header includes no HIP
header, so no GPU and no ROCm is needed."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "srsran_project_23.5_amd", "csrc")

PROGRAM = r"""
#include "device_image.h"
#include <cstdio>
#include <cstdlib>

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #c); \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

struct rec32 { uint32_t w[8]; };  // the size of the decoder and dematcher descriptors
struct rec40 { uint64_t a; uint32_t w[8]; }; // the size of the TB assembly descriptor

struct span { size_t off, bytes, align; };
static std::vector<span> g_spans;

template <class T>
static image_slot<T> note(image_slot<T> s, size_t align)
{
  g_spans.push_back({s.offset, s.bytes(), align});
  return s;
}

template <class T>
static std::vector<T> filled(size_t n, unsigned seed)
{
  std::vector<T> v(n);
  uint8_t*       b = reinterpret_cast<uint8_t*>(v.data());
  for (size_t i = 0; i < n * sizeof(T); ++i)
    b[i] = (uint8_t)(seed * 31u + i * 7u + 1u);
  return v;
}

template <class T>
static void same_bytes(const std::vector<uint8_t>& host, image_slot<T> s, const std::vector<T>& v)
{
  CHECK(s.count == v.size());
  CHECK(s.offset + s.bytes() <= host.size());
  CHECK(s.bytes() == 0 || std::memcmp(host.data() + s.offset, v.data(), s.bytes()) == 0);
}

static void check_spans(const device_image& img, size_t nof_put)
{
  for (size_t i = 0; i < g_spans.size(); ++i) {
    const span& a = g_spans[i];
    CHECK(a.off % a.align == 0);
    CHECK(a.off + a.bytes <= img.total_bytes());
    CHECK(a.bytes == 0 || a.off < img.total_bytes());
    if (i < nof_put)
      CHECK(a.off + a.bytes <= img.staged_bytes()); // the put arrays are the staged prefix ...
    else
      CHECK(a.off >= img.staged_bytes()); // ... and every reserved region lies behind it
    for (size_t j = 0; j < i; ++j) { // appended in order: no slot begins before the one in front of it ends
      const span& b = g_spans[j];
      CHECK(b.off + b.bytes <= a.off);
    }
  }
}

int main()
{
  // ---- the PUSCH decode shape: ten arrays of mixed element sizes and odd counts, two reserved regions, a 256-aligned one
  {
    const auto rdm = filled<rec32>(3, 1), rdm_nf = filled<rec32>(1, 2), dec = filled<rec32>(3, 3);
    const auto order = filled<uint32_t>(3, 4), bundles = filled<uint32_t>(2, 5), slots = filled<uint32_t>(3, 6), reset = filled<uint32_t>(3, 7);
    const auto asmd  = filled<rec40>(2, 8);
    const auto cb_tb = filled<uint32_t>(3, 9), cbw = filled<uint32_t>(5, 10);
    device_image img;
    CHECK(img.staged_bytes() == 0 && img.total_bytes() == 0);
    const auto s_rdm = note(img.put(rdm), 16), s_rdm_nf = note(img.put(rdm_nf), 16);
    const auto s_order = note(img.put(order), 16), s_bundles = note(img.put(bundles), 16);
    const auto s_dec = note(img.put(dec), 16);
    const auto s_slots = note(img.put(slots), 16), s_reset = note(img.put(reset.data(), reset.size()), 16);
    const auto s_asmd = note(img.put(asmd), 16);
    const auto s_cb_tb = note(img.put(cb_tb), 16), s_cbw = note(img.put(cbw), 16);
    // the staged part ends with its last array: exactly the put arrays and the gaps between them
    CHECK(img.staged_bytes() == s_cbw.offset + s_cbw.bytes());
    CHECK(img.total_bytes() == img.staged_bytes());
    const size_t staged = img.staged_bytes();
    const auto   s_iters = note(img.reserve<int32_t>(3), 16);
    const auto   s_part  = note(img.reserve<uint32_t>(3), 16);
    const auto   s_gmsg  = note(img.reserve<uint8_t>(1000, 256), 256);
    CHECK(img.ok());
    CHECK(img.staged_bytes() == staged); // a reserved region does not move the staged part
    CHECK(img.total_bytes() == s_gmsg.offset + 1000);
    CHECK(s_iters.count == 3 && s_part.count == 3 && s_gmsg.count == 1000);
    check_spans(img, 10);
    // contents: the exact-size copy (the sanitizer sees a write past staged_bytes()) and the vector form
    std::vector<uint8_t> host(img.staged_bytes(), 0xee);
    img.copy_staged(host.data());
    CHECK(host == img.staged());
    same_bytes(host, s_rdm, rdm), same_bytes(host, s_rdm_nf, rdm_nf), same_bytes(host, s_order, order), same_bytes(host, s_bundles, bundles);
    same_bytes(host, s_dec, dec), same_bytes(host, s_slots, slots), same_bytes(host, s_reset, reset), same_bytes(host, s_asmd, asmd);
    same_bytes(host, s_cb_tb, cb_tb), same_bytes(host, s_cbw, cbw);
    // at(): base + offset, typed, on a base that is never dereferenced
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)0x7000000000ull);
    CHECK(reinterpret_cast<uint8_t*>(device_image::at(base, s_asmd)) == base + s_asmd.offset);
    CHECK(reinterpret_cast<uint8_t*>(s_gmsg.at(base)) == base + s_gmsg.offset);
    CHECK(device_image::at(base, s_iters) == reinterpret_cast<int32_t*>(base + s_iters.offset));
    CHECK(s_dec.at(static_cast<const void*>(base)) + 1 == reinterpret_cast<rec32*>(base + s_dec.offset + 32));
    // a put behind a reserved region is refused: nothing is appended and the image is no longer accepted
    const size_t total = img.total_bytes();
    const auto   late  = img.put(order);
    CHECK(!img.ok());
    CHECK(late.count == 0 && img.total_bytes() == total && img.staged_bytes() == staged);
    CHECK(img.staged() == host);
  }
  // ---- empty arrays: valid slots of length 0, in front, in between and at the end; an odd byte count in between
  {
    g_spans.clear();
    const std::vector<uint32_t> none;
    const auto                  bytes = filled<uint8_t>(7, 11);
    const auto                  halves = filled<uint16_t>(9, 12);
    device_image                img;
    const auto s0 = note(img.put(none), 16);
    const auto s1 = note(img.put(bytes), 16);
    const auto s2 = note(img.put(none), 16);
    const auto s3 = note(img.put(halves), 16);
    const auto s4 = note(img.put((const rec32*)nullptr, 0), 16);
    CHECK(img.ok());
    CHECK(s0.count == 0 && s0.offset == 0 && s2.count == 0 && s4.count == 0);
    CHECK(s1.offset == 0 && s2.offset == 16 && s3.offset == 16 && s4.offset == 48);
    CHECK(img.staged_bytes() == 48 && img.total_bytes() == 48); // 16 + 18 bytes, then the boundary of the empty array at the end
    const auto r0 = note(img.reserve<float>(0), 16);
    const auto r1 = note(img.reserve<uint8_t>(3, 64), 64);
    const auto r2 = note(img.reserve<uint64_t>(2), 16);
    CHECK(r0.offset == 48 && r1.offset == 64 && r2.offset == 80 && img.total_bytes() == 96 && img.staged_bytes() == 48);
    check_spans(img, 5);
    const std::vector<uint8_t> host = img.staged();
    same_bytes(host, s1, bytes), same_bytes(host, s3, halves), same_bytes(host, s0, none);
    for (size_t i = 7; i < 16; ++i)
      CHECK(host[i] == 0); // gaps are zeroed
    CHECK(!img.put(none).count && !img.ok()); // refused even when empty, and after an empty reserve
  }
  {
    device_image img;
    (void)img.reserve<uint8_t>(0);
    const auto v = filled<uint32_t>(1, 13);
    (void)img.put(v);
    CHECK(!img.ok() && img.total_bytes() == 0);
    device_image nothing;
    CHECK(nothing.ok() && nothing.staged().empty());
    nothing.copy_staged(nullptr);
  }
  std::puts("device_image OK");
  return 0;
}
"""


def test_device_image_layout_under_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "device_image_check.cpp"), os.path.join(tmp, "device_image_check")
        open(src, "w").write(PROGRAM)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-I", CSRC, src, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        assert "device_image OK" in r.stdout
