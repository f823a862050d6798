// The integer lower-envelope scan shared by the separable exact squared-distance passes of metrics.hip (Hausdorff distance)
// and edt.hip (distance transform).
#pragma once
#include "common.hpp"

constexpr int INF = 0x7FFFFFFF;            // "no source in reach" (never added to)
constexpr int ENVELOPE_MAX_EXTENT = 2048;  // D, H, W: keeps every square, sum and packed stack entry inside int32

// Lower envelope of the parabolas p -> (p - i)^2 + f(i) over the finite f(i), i = 0..m-1 (f at in[i * st]); Meijster et
// al.'s first scan with integer separators.  Entry k of the stack (apex v, start t of its segment, t strictly increasing
// and >= k) is stored as v | t << 16 at stk[k * st]; the top is also returned in registers.  -> top index, -1: no finite f.
DEVI int envelope(const int* __restrict__ in, int* stk, size_t st, int m, int& tv, int& tt, int& tf) {
  int k = -1;
  int fn = in[0];
  for (int q = 0; q < m; ++q) {
    const int fq = fn;
    if (q + 1 < m) fn = in[(size_t)(q + 1) * st];
    if (fq == INF) continue;
    while (k >= 0) {
      const int a = tt - tv, c = tt - q;
      if (a * a + tf <= c * c + fq) break;  // the top still wins at the start of its segment
      if (--k >= 0) {
        const int e = stk[(size_t)k * st];
        tv = e & 0xFFFF;
        tt = e >> 16;
        tf = in[(size_t)tv * st];
      }
    }
    if (k < 0) {
      k = 0; tv = q; tt = 0; tf = fq;
      stk[0] = q;
    } else {
      // first integer p at which q is strictly below the top: 1 + floor(intersection); the numerator is >= 0 here
      const int w = 1 + (q * q - tv * tv + fq - tf) / (2 * (q - tv));
      if (w < m) {
        ++k; tv = q; tt = w; tf = fq;
        stk[(size_t)k * st] = q | (w << 16);
      }
    }
  }
  return k;
}
