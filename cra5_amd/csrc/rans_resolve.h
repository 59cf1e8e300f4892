// Symbol -> rANS record against the quantised CDF tables (rans_interface.cpp:121-150 in taohan10200/CRA5): the one
// definition of the wire format's resolve step, shared by the host coder (host_entropy.cpp) and the device resolver
// (elementwise.hip, which includes this file between `#pragma clang force_cuda_host_device begin` / `end`).
// Plain C++: host_entropy.cpp is compiled without the HIP headers.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace cra5_rans {

constexpr uint64_t kRansL = 1ull << 31;  // rans64.h RANS64_L
constexpr uint32_t kProbBits = 16;       // rans_interface.cpp:49
constexpr uint32_t kBypassBits = 4;      // rans_interface.cpp:51
constexpr uint32_t kBypassMax = (1u << kBypassBits) - 1;
// A uint32 payload has at most 8 nibbles, so the nibble count always fits ONE count nibble: the reference's run of
// kBypassMax count nibbles (rans_interface.cpp:136-140) never happens.
static_assert(32 / kBypassBits < kBypassMax, "an escape's nibble count must fit one bypass nibble");

struct Tables {
  const int32_t *cdfs;  // [n_cdfs, stride]
  int n_cdfs;
  int stride;
  const int32_t *sizes;
  const int32_t *offsets;
};

// a row index the tables can code with: in range, with at least one bin and the escape bin, within the stride
inline bool row_ok(const Tables &t, int32_t ci) {
  return ci >= 0 && ci < t.n_cdfs && t.sizes[ci] >= 2 && t.sizes[ci] <= t.stride;
}

// One coded symbol resolved against its table row: bin + escape payload.
struct Resolved {
  uint32_t start, range;
  bool escape;
  uint32_t raw;   // escape payload (0 for a regular symbol)
  int n_nibbles;  // payload nibbles (0..8)
};

// for a row that passes row_ok()
inline Resolved resolve(const Tables &t, int32_t sym, int32_t ci) {
  const int32_t *cdf = t.cdfs + static_cast<size_t>(ci) * t.stride;
  const int32_t max_value = t.sizes[ci] - 2;
  int32_t value = sym - t.offsets[ci];
  Resolved r{0, 0, false, 0, 0};
  if (value < 0) {
    r.raw = static_cast<uint32_t>(-2 * value - 1);
    value = max_value;
  } else if (value >= max_value) {
    r.raw = static_cast<uint32_t>(2 * (value - max_value));
    value = max_value;
  }
  r.start = static_cast<uint32_t>(cdf[value]) & 0xFFFFu;
  r.range = static_cast<uint32_t>(cdf[value + 1] - cdf[value]) & 0xFFFFu;
  if (value == max_value) {
    r.escape = true;
    r.n_nibbles = r.raw ? (35 - __builtin_clz(r.raw)) >> 2 : 0;   // significant nibbles: ceil(bit length / 4)
  }
  return r;
}

}  // namespace cra5_rans
