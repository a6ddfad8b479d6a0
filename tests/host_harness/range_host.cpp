// Host build of csrc/orp_range.hpp (the fp16-pieces range rule) for tests/test_range_host.py: the same inline functions the
// gfx950 kernels use, compiled with g++.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../orientedreppoints_amd/csrc/orp_range.hpp"

extern "C" {

uint32_t host_range_bits(float v) { return orp::range_bits(v); }
uint32_t host_range_bound_bits(float v) { return orp::range_bound_bits(v); }
int host_range_exp(uint32_t am) { return orp::range_exp(am); }
float host_range_scale(int k) { return orp::range_scale(k); }
int host_range_exp_of(float s) { return orp::range_exp_of(s); }
float host_range_unscale(float acc, int k) { return orp::range_unscale(acc, k); }

// Every `step`-th float bit pattern in [lo, hi]: the range word of a tensor whose only element is that value, its k, and where
// 2^k |v| lands.  Returns the number of patterns that break the rule, the first one in *first.
long host_range_rule_violations(uint32_t lo, uint32_t hi, uint32_t step, uint32_t* first) {
  long bad = 0;
  for (uint64_t u = lo; u <= hi; u += step) {
    float v;
    const uint32_t b = (uint32_t)u;
    memcpy(&v, &b, sizeof v);
    const uint32_t am = orp::range_bits(v);
    const int k = orp::range_exp(am);
    bool ok = true;
    if (!isfinite(v) || v == 0.f) {
      ok = am == 0u && k == 0;
    } else {
      float a = fabsf(v);
      uint32_t ab;
      memcpy(&ab, &a, sizeof ab);
      ok = am == ab && k >= -126 && k <= 127;
      const float s = orp::range_scale(k);
      ok = ok && s == ldexpf(1.f, k) && isnormal(s) && orp::range_exp_of(s) == k;
      const double scaled = ldexp((double)a, k);                 // exact in double
      // representable: 2^k with k = 14 - floor(log2 |v|) is a normal float
      const int want = 14 - ilogb(a);
      if (want <= 127) ok = ok && k == want && scaled >= 16384.0 && scaled < 32768.0;
      else ok = ok && k == 127 && scaled < 16384.0;
    }
    if (!ok) {
      if (bad == 0) *first = b;
      bad++;
    }
  }
  return bad;
}

}
