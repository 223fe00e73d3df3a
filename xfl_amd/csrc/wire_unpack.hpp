// One quad (16 B) of a ciphertext row from the bytes of a received payload
// (Paillier.ciphertext_from, paillier.py:260-271): row i of k_wire_unpack is
// the len[i] little-endian bytes at bytes[off[i] ..], zero-extended to n2w
// words. off / len come from a scan of bytes a remote party sent
// (xhe_wire_scan), so nothing here trusts them: every load is clamped to
// [bytes, bytes + nbytes), whatever they hold.
//
// __host__ __device__: the kernel (xhe.hip) and the sanitized CPU program
// (tests/native/wire_scan_fuzz.cpp) run this very code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XHE_WIRE_HD __host__ __device__
#else
#define XHE_WIRE_HD
#endif

namespace xhe {
namespace wireu {

// dword k of `bytes` (4-byte aligned), zero where it lies outside
// [0, nbytes): the last, partial dword is put together from its bytes, so
// the aligned over-read of a value that ends at nbytes never happens
XHE_WIRE_HD inline uint32_t dword_at(const uint8_t* bytes, int64_t nbytes, int64_t k) {
  const int64_t b = 4 * k;
  if (k < 0 || b >= nbytes) return 0u;
  if (b + 4 <= nbytes) return *reinterpret_cast<const uint32_t*>(bytes + b);
  uint32_t v = 0;
  for (int j = 0; b + j < nbytes; ++j) v |= (uint32_t)bytes[b + j] << (8 * j);
  return v;
}

// out[0..4) = words 4q .. 4q+3 of the row whose value is the `len` bytes at
// bytes[off ..] (len cut to 4 n2w): aligned dwords, funnel-shifted by the
// source's residue mod 4, bytes at and above len masked to zero
XHE_WIRE_HD inline void unpack_quad(const uint8_t* bytes, int64_t nbytes, uint32_t off, uint32_t len, int n2w, int q,
                                    uint32_t out[4]) {
  const int64_t wbytes = 4 * (int64_t)n2w;
  const int64_t used = (int64_t)len < wbytes ? (int64_t)len : wbytes;
  const int64_t rem = used - 16 * (int64_t)q;  // value bytes from this quad on
  out[0] = out[1] = out[2] = out[3] = 0u;
  if (rem <= 0) return;
  const int64_t s = (int64_t)off + 16 * (int64_t)q;  // < 2^33: no overflow
  const int64_t k0 = s >> 2;
  const int sh = 8 * (int)(s & 3);
  const int nw = rem >= 16 ? 4 : (int)((rem + 3) >> 2);  // words that hold value bytes
  uint32_t lo = dword_at(bytes, nbytes, k0);
  for (int j = 0; j < nw; ++j) {
    // (the dword past the last one is read only where the shift needs it)
    const uint32_t hi = (sh || j + 1 < nw) ? dword_at(bytes, nbytes, k0 + j + 1) : 0u;
    uint32_t w = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
    const int64_t valid = rem - 4 * j;  // >= 1
    if (valid < 4) w &= (1u << (8 * (int)valid)) - 1u;
    out[j] = w;
    lo = hi;
  }
}

}  // namespace wireu
}  // namespace xhe
